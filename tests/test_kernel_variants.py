"""The selectors of rescan_line_sted_amd/csrc/kernel_variants.hpp -- which instantiation of k_colconv, k_colconv_outer,
k_rowpass and k_rowpair a launch gets -- swept on the CPU with the device's compile-time sizes, through the host entry points of
tests/emu/long_emu.cpp (emu_device_select runs the functions fft_kernels.hip's launchers call; emu_device_table prints the rows
their walks visit).  No kernel body runs here.  CPU only.
"""
import ctypes
import itertools
import math

import pytest

from test_long_rows_cpu import _build, _table, half_pitch

LENGTHS = (64, 192, 256, 576, 1152, 2304, 4608)
COL, ROW, PAIR = 0, 1, 2
# the image sizes some variants are compiled for (kernel_variants.hpp DeviceSpecial); elsewhere a size the length's plans have
SPECIAL = {576: 512, 1152: 1024, 2304: 2048, 4608: 4096}


@pytest.fixture(scope='module')
def rows():
    return ctypes.CDLL(_build(('long_emu',))['long_emu'])


def tiled_pitch(L):
    return math.ceil(half_pitch(L) / 48) * 48          # a multiple of every tile width (4, 8, 16; 3 and 6 at the long lengths)


def select(rows, L, esize, family, mode, n, V=1, pitch=None, realp=1, flag=0):
    """The row the device would launch, as a line of the table; None: hipErrorInvalidValue"""
    buf = ctypes.create_string_buffer(256)
    r = rows.emu_device_select(L, esize, family, mode, n, V, tiled_pitch(L) if pitch is None else pitch, realp, flag, buf, len(buf))
    assert r == -1 or 0 < r < len(buf)
    return None if r < 0 else buf.value.decode().strip()


@pytest.mark.parametrize('L', LENGTHS)
def test_the_selectors_reach_every_row_and_only_rows(rows, L):
    """Over every mode (and one past the last), V, sub_one / residual, real and complex multipliers, sizes at and around the
    compile-time one and pitches that are and are not whole tiles: the selected row exists for the length and type, and every
    row that exists is selected somewhere."""
    sp = SPECIAL.get(L, L * 8 // 9)
    for esize in (4, 8):
        exists = _table(rows.emu_device_table, L, esize)
        chosen = set()
        for family, modes in ((COL, range(7)), (ROW, range(6)), (PAIR, range(6))):
            for mode, V, flag, realp, n, dp in itertools.product(modes, (1, 2, 4), (0, 1), (0, 1), (sp, sp - 1, sp + 64), (0, 1)):
                line = select(rows, L, esize, family, mode, n, V, tiled_pitch(L) + dp, realp, flag)
                if line is not None:
                    assert line in exists, 'selected, but no such row: %s' % line
                    chosen.add(line)
        assert chosen == exists, 'rows no request selects: %s' % sorted(exists - chosen)


def test_selected_rows_by_hand(rows):
    """A table written out from the launch ladders the selectors replaced (fft_kernels.hip before the shared list)."""
    c, o, r, p = 'k_colconv L=%d T=%s ', 'k_colconv_outer L=%d ', 'k_rowpass L=%d T=%s ', 'k_rowpair L=%d T=%s '
    f32, f64 = 4, 8
    cases = [
        # 576 f32, 512 rows, one view: the compile-time row count; compact twiddles for the spectrum of `ratio - 1`
        ((576, f32, COL, 0, 512, 1, None, 1, 1), c % (576, 'f32') + 'MODE=0 REALP=1 NYC=512 CT=1'),
        ((576, f32, COL, 0, 512, 1, None, 0, 0), c % (576, 'f32') + 'MODE=0 REALP=0 NYC=512 CT=0'),
        # ... a pitch that is no multiple of the tile width, another row count, more views, float64: the generic kernel
        ((576, f32, COL, 0, 512, 1, tiled_pitch(576) + 1, 1, 1), c % (576, 'f32') + 'MODE=0 REALP=1 NYC=0 CT=0'),
        ((576, f32, COL, 0, 511, 1, None, 1, 1), c % (576, 'f32') + 'MODE=0 REALP=1 NYC=0 CT=0'),
        ((576, f32, COL, 0, 512, 4, None, 1, 1), c % (576, 'f32') + 'MODE=0 REALP=1 NYC=0 CT=0'),
        ((576, f64, COL, 0, 512, 1, None, 1, 1), c % (576, 'f64') + 'MODE=0 REALP=1 NYC=0 CT=0'),
        # the fused multi-view modes: compile-time row count with a real multiplier only, compact twiddles in H_t only
        ((576, f32, COL, 1, 512, 4, None, 1, 1), c % (576, 'f32') + 'MODE=1 REALP=1 NYC=512 CT=0'),
        ((576, f32, COL, 2, 512, 4, None, 1, 1), c % (576, 'f32') + 'MODE=2 REALP=1 NYC=512 CT=1'),
        ((576, f32, COL, 2, 512, 4, None, 1, 0), c % (576, 'f32') + 'MODE=2 REALP=1 NYC=512 CT=0'),
        ((576, f32, COL, 2, 512, 4, None, 0, 1), c % (576, 'f32') + 'MODE=2 REALP=0 NYC=0 CT=0'),
        # lengths that are not wave-private: one column kernel, the per-image mode only
        ((64, f32, COL, 0, 56, 1, None, 1, 0), c % (64, 'f32') + 'MODE=0 REALP=0 NYC=0 CT=0'),
        ((64, f32, COL, 1, 56, 2, None, 1, 0), None),
        ((576, f32, COL, 3, 512, 1, None, 1, 0), None),
        # the outer lengths: M x 512 rows and whole tiles of the mode's width; the split pass in f32 only, its first half complex
        ((2304, f32, COL, 0, 2048, 1, None, 1, 0), o % 2304 + 'C=16 REALP=1 MODE=0 T=f32 NYC=2048'),
        ((2304, f32, COL, 0, 2048, 1, tiled_pitch(2304) + 8, 1, 0), o % 2304 + 'C=16 REALP=1 MODE=0 T=f32 NYC=0'),
        ((2304, f32, COL, 4, 2048, 2, tiled_pitch(2304) + 8, 0, 0), o % 2304 + 'C=8 REALP=0 MODE=4 T=f32 NYC=2048'),
        ((4608, f32, COL, 3, 4096, 2, None, 1, 0), o % 4608 + 'C=8 REALP=0 MODE=3 T=f32 NYC=4096'),
        ((1152, f64, COL, 0, 1000, 1, None, 0, 0), o % 1152 + 'C=4 REALP=0 MODE=0 T=f64 NYC=0'),
        ((1152, f64, COL, 4, 1024, 2, None, 1, 0), None),
        ((1152, f32, COL, 1, 1024, 2, None, 1, 0), None),
        # row kernels: 512-pixel rows of `ratio - 1` plans at 576 f32 on the lean bodies; single view without accumulators
        ((576, f32, ROW, 2, 512, 4, None, 0, 1), r % (576, 'f32') + 'MODE=2 ONEV=0 PRESUM=0 NXC=512 SUBC=1'),
        ((576, f32, ROW, 3, 512, 1, None, 0, 1), r % (576, 'f32') + 'MODE=3 ONEV=1 PRESUM=0 NXC=512 SUBC=1'),
        ((576, f32, ROW, 3, 512, 1, None, 0, 0), r % (576, 'f32') + 'MODE=3 ONEV=1 PRESUM=0 NXC=0 SUBC=-1'),
        ((576, f32, ROW, 4, 512, 1, None, 0, 1), r % (576, 'f32') + 'MODE=4 ONEV=1 PRESUM=0 NXC=0 SUBC=-1'),
        ((576, f32, ROW, 4, 512, 2, None, 0, 1), r % (576, 'f32') + 'MODE=4 ONEV=0 PRESUM=0 NXC=0 SUBC=-1'),
        ((576, f32, ROW, 3, 512, 2, None, 0, 0), r % (576, 'f32') + 'MODE=3 ONEV=0 PRESUM=0 NXC=0 SUBC=-1'),
        ((576, f32, ROW, 5, 512, 1, None, 0, 0), None),
        # frame pairs: 2048-pixel rows at 2304 in f32 only, never the forward transform; no pair kernels at 64
        ((2304, f32, PAIR, 2, 2048, 1, None, 0, 1), p % (2304, 'f32') + 'MODE=2 NXC=2048 SUBC=1'),
        ((2304, f64, PAIR, 2, 2048, 1, None, 0, 1), p % (2304, 'f64') + 'MODE=2 NXC=0 SUBC=-1'),
        ((2304, f32, PAIR, 0, 2048, 1, None, 0, 1), p % (2304, 'f32') + 'MODE=0 NXC=0 SUBC=-1'),
        ((2304, f32, PAIR, 3, 2048, 1, None, 0, 0), p % (2304, 'f32') + 'MODE=3 NXC=0 SUBC=-1'),
        ((576, f32, PAIR, 3, 512, 1, None, 0, 1), p % (576, 'f32') + 'MODE=3 NXC=512 SUBC=1'),
        ((576, f32, PAIR, 1, 512, 1, None, 0, 1), None),
        ((64, f32, PAIR, 2, 56, 1, None, 0, 1), None),
    ]
    # ROW_UPDATE of a multi-view `ratio - 1` plan: the views' spectra summed on their way in, at every length and type
    for L in LENGTHS:
        for esize in (f32, f64):
            cases.append(((L, esize, ROW, 3, SPECIAL.get(L, 56), 2, None, 0, 1),
                          r % (L, 'f32' if esize == 4 else 'f64') + 'MODE=3 ONEV=1 PRESUM=1 NXC=0 SUBC=-1'))
    for args, want in cases:
        assert select(rows, *args) == want, args
