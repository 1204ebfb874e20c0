"""The peak search of the registration without a GPU (include/rlsted.h rl_register_peaks, rl_register_estimate;
rescan_line_sted_amd/csrc/register_kernels.hpp PEAKS): the kernel's body emulated thread by thread (tests/emu/register_peaks_emu.cpp)
against the host's ncc_surface + surface_peak bit for bit on constructed rows of sums (tests/peaks_reference.py) -- ties across
threads, within a thread and against the thread order, border peaks, flat pairs, a plateau; the estimate's stages and refine rules
against registration._estimate; the same body as a stand-alone program under the address and undefined-behaviour sanitizers; the
argument checks.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import peaks_reference as pr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'register_peaks_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(EMU_DIR, 'register_emu.cpp')] + \
       [os.path.join(CSRC, f) for f in ('register_kernels.hpp', 'ingest_kernels.hpp', 'tile_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
FLOATS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libregister_peaks_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_register_peaks.argtypes = [vp, i, i, d, vp, vp]
    lib.emu_register_estimate.argtypes = [vp, i, vp, vp, i, vp, i, i, i, i, i, i, vp, vp, vp]
    lib.emu_register_sums.argtypes = [vp, i, vp, vp, i, vp, i, i, i, i, i, vp, vp, vp]
    lib.emu_shift_images.argtypes = [vp, i, i, i, i, vp, i, d, vp, i, vp]
    return lib


def emu_peaks(emu, tot, R, n=pr.N_TERMS):
    """tot [pairs][nd * 3 + 2]: (fields [pairs][5], surfaces [pairs][nd]), each inside guard values that must stay."""
    pairs, nd = tot.shape[0], (2 * R + 1) ** 2
    pk, sf = np.full(pairs * 5 + 16, 7.0), np.full(pairs * nd + 16, 7.0)
    assert emu.emu_register_peaks(_p(np.ascontiguousarray(tot)), pairs, R, n, _p(pk[8:]), _p(sf[8:])) == 0
    assert np.all(pk[:8] == 7.0) and np.all(pk[8 + pairs * 5:] == 7.0) and np.all(sf[:8] == 7.0) and np.all(sf[8 + pairs * nd:] == 7.0)
    return pk[8:8 + pairs * 5].reshape(pairs, 5), sf[8:8 + pairs * nd].reshape(pairs, nd)


# ---- the body against the host ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('R', [1, 8, 32])
def test_emulated_peaks_are_the_host_bit_for_bit(emu, R):
    """Every constructed row alone and all of them in one call: flags, integer peak, value and sub-pixel part, and the surface, the
    bits of ncc_surface + surface_peak."""
    rows = pr.rows(R)
    names = list(rows)
    tot = np.stack([rows[k] for k in names])
    got, surf = emu_peaks(emu, tot, R)
    for k, name in enumerate(names):
        want, wsurf = pr.expected(rows[name], R)
        assert got[k].tobytes() == want.tobytes(), (name, got[k], want)
        assert surf[k].tobytes() == wsurf.tobytes(), name
        alone, _ = emu_peaks(emu, tot[k:k + 1], R)
        assert alone[0].tobytes() == want.tobytes(), name


def test_constructed_rows_mean_what_they_say():
    """The host's own answers on the constructed rows: ties resolve to the first index, border rows are at the limit with integer
    shifts, the flat rows are flat, the plateau has den = 0 on both axes and so no sub-pixel part."""
    from rescan_line_sted_amd import registration as reg
    for R in (1, 8, 32):
        W = 2 * R + 1
        rows = pr.rows(R)
        for name, (p, _) in ({'tie_threads': (1, 3)} if R == 1 else {'tie_threads': (5, 100), 'tie_same_thread': (10, 266),
                                                                    'tie_later_in_lower_thread': (200, 260)}).items():
            f, _ = pr.expected(rows[name], R)
            assert not f[4] and np.rint(f[0]) == p // W - R and np.rint(f[1]) == p % W - R, name
        for name in [k for k in rows if k.startswith('border_')]:
            f, _ = pr.expected(rows[name], R)
            assert f[3] == 1.0 and f[0] == int(f[0]) and f[1] == int(f[1]) and (abs(f[0]) == R or abs(f[1]) == R), name
        for name in ('flat_va', 'flat_vb', 'flat_vb_nan'):
            f, s = pr.expected(rows[name], R)
            assert f.tobytes() == np.array([0.0, 0, 0, 0, 1]).tobytes() and not s.any(), name
        f, s = pr.expected(rows['plateau'], R)
        c = s.reshape(W, W)
        assert f[0] == 0.0 and f[1] == 0.0 and f[2] == 1.0 and not f[3]
        assert c[R - 1, R] < c[R, R] == c[R + 1, R] and (c[R - 1, R] - 2.0 * c[R, R]) + c[R + 1, R] == 0.0
        surf, _ = reg.ncc_surface(rows['interior'][:W * W * 3].reshape(-1, 3), rows['interior'][W * W * 3:], pr.N_TERMS)
        assert np.argmax(surf) == (R + 1) * W + R + 1


# ---- the estimate's stages against registration._estimate ------------------------------------------------------------------------

class _Buf:
    def __init__(self, a, dtype):
        self.a, self.dtype = a, dtype


class _EmuDevice:
    """registration._estimate's device: the emulated sums and shift (the bits the emulated estimate is built from)."""

    def __init__(self, emu):
        self.emu = emu

    def sums(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M):
        W, n = 2 * R + 1, len(mov_offsets)
        S, A = np.empty((n, W * W, 3)), np.empty((n, 2))
        ro, mo = np.asarray(ref_offsets, dtype=np.int64), np.asarray(mov_offsets, dtype=np.int64)
        assert self.emu.emu_register_sums(_p(ref.a), FLOATS[ref.a.dtype], _p(ro), _p(mov.a), FLOATS[mov.a.dtype], _p(mo), n, ny, nx, R, M,
                                          _p(S), _p(A), None) == 0
        return S, A

    def gather_shift(self, src, offsets, ny, nx, shifts, dst, order=3):
        for k, o in enumerate(offsets):
            sh = np.ascontiguousarray(shifts[k], dtype=np.float64)
            out = np.empty(ny * nx)
            assert self.emu.emu_shift_images(_p(src.a[o:o + ny * nx]), FLOATS[src.a.dtype], 1, ny, nx, _p(sh), order, -np.inf, _p(out), 1, None) == 0
            dst.a[k * ny * nx:(k + 1) * ny * nx] = out


@pytest.mark.parametrize('refine', [0, 1, 2])
def test_emulated_estimate_is_the_host_estimate(emu, refine):
    """emu_register_estimate (sums, peaks, the product's rules for the first stage and the refine passes) against _estimate on the
    same emulated sums and shift: shifts, ncc, at_limit, flat and the surfaces byte for byte; f32 and f64 images; one flat pair,
    one pair at the limit."""
    from rescan_line_sted_amd import registration as reg
    R, M = 4, 6
    for dt in (np.float32, np.float64):
        imgs, ref = pr.estimate_images(dt)
        N, ny, nx = imgs.shape
        n_pix = ny * nx
        ref_off, mov_off = [0] * N, [k * n_pix for k in range(N)]
        want, winfo = reg._estimate(_EmuDevice(emu), _Buf(ref.ravel(), None), ref_off, _Buf(imgs.ravel(), None), mov_off, ny, nx, R, refine, M,
                                    _Buf(np.full(N * n_pix, np.nan), 'f64'), surfaces=True)
        assert winfo['flat'][5] and not winfo['flat'][:5].any() and winfo['at_limit'][4] and not winfo['at_limit'][:4].any()
        shifts, fields, surf = np.full((N, 2), np.nan), np.full((N, 3), np.nan), np.full((N, (2 * R + 1) ** 2), np.nan)
        ro, mo = np.asarray(ref_off, dtype=np.int64), np.asarray(mov_off, dtype=np.int64)
        assert emu.emu_register_estimate(_p(ref), FLOATS[ref.dtype], _p(ro), _p(imgs), FLOATS[imgs.dtype], _p(mo), N, ny, nx, R, M, refine,
                                         _p(shifts), _p(fields), _p(surf)) == 0
        assert shifts.tobytes() == want.tobytes(), (shifts, want)
        assert fields[:, 0].tobytes() == winfo['ncc'].tobytes()
        assert np.array_equal(fields[:, 1] != 0, winfo['at_limit']) and np.array_equal(fields[:, 2] != 0, winfo['flat'])
        assert surf.tobytes() == winfo['surfaces'].reshape(N, -1).tobytes()


def test_device_peaks_route_through_the_device_estimate(monkeypatch):
    """estimate_shifts(device_peaks=True) hands the whole estimate to dev.estimate with R, M, refine and the scratch, and turns its
    fields into the info of the default path: float64 ncc, bool at_limit and flat, surfaces (N, W, W)."""
    from rescan_line_sted_amd import registration as reg
    calls = []

    class Dev:
        def __init__(self, device=0):
            pass

        def alloc(self, elements, dtype):
            return _Buf(np.zeros(int(elements)), dtype)

        def upload(self, buf, array, byte_offset=0):
            pass

        def estimate(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M, refine, scratch, surfaces=False):
            calls.append((list(ref_offsets), list(mov_offsets), ny, nx, R, M, refine, scratch is not None, surfaces))
            n = len(mov_offsets)
            f = np.zeros((n, 3))
            f[0] = (0.5, 1.0, 0.0)
            f[1] = (0.0, 0.0, 1.0)
            return np.arange(2.0 * n).reshape(n, 2), f, np.ones((n, (2 * R + 1) ** 2)) if surfaces else None

        def close(self):
            calls.append('close')

    monkeypatch.setattr(reg, '_Device', Dev)
    a = np.zeros((3, 40, 48), dtype=np.float32)
    s, info = reg.estimate_shifts(a, a[0], max_shift=4, refine=2, surfaces=True, device_peaks=True)
    assert calls == [([0, 0, 0], [0, 1920, 3840], 40, 48, 4, 6, 2, True, True), 'close']
    assert np.array_equal(s, np.arange(6.0).reshape(3, 2)) and info['ncc'].dtype == np.float64 and info['ncc'][0] == 0.5
    assert info['at_limit'].tolist() == [True, False, False] and info['flat'].tolist() == [False, True, False]
    assert info['surfaces'].shape == (3, 9, 9)
    calls.clear()
    reg.estimate_shifts(a, a, max_shift=3, refine=0, device_peaks=True)
    assert calls[0][:8] == ([0, 1920, 3840], [0, 1920, 3840], 40, 48, 3, 5, 0, False)


# ---- sanitizers -------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulated peaks as a program of its own under -fsanitize=address,undefined, run directly: rows, fields and surfaces are
    heap blocks of exactly their byte counts, the tree's arrays exactly the kernel's LDS; R = 1, 2, 8, 32 with ties and flat pairs."""
    exe = str(tmp_path / 'register_peaks_emu_san')
    subprocess.check_call(['g++', '-DPEAKS_EMU_MAIN', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 4', r.stdout


# ---- argument checks --------------------------------------------------------------------------------------------------------------

def test_the_library_declares_and_checks_its_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert len(_lib.PROTOTYPES['rl_register_peaks'][1]) == 7 and len(_lib.PROTOTYPES['rl_register_estimate'][1]) == 17
    header = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_register_peaks(' in header and 'int rl_register_estimate(' in header and '#define RL_PEAK_FIELDS 5' in header
    ctx, tot = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)          # (never dereferenced)
    out = (ctypes.c_double * (5 * 4))()
    good = dict(ctx=ctx, tot=tot, n=4, R=3, nt=100.0, out=out, surf=None)
    for change in (dict(ctx=None), dict(tot=None), dict(out=None), dict(n=0), dict(n=-2), dict(R=0), dict(R=33), dict(nt=0.5), dict(nt=float('nan')),
                   dict(nt=float('inf')), dict(nt=-1.0)):
        g = {**good, **change}
        assert L.rl_register_peaks(g['ctx'], g['tot'], g['n'], g['R'], g['nt'], g['out'], g['surf']) == -1 and L.rl_last_error() != b'', change
    a, b = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)
    off, neg = (ctypes.c_int64 * 2)(0, 100), (ctypes.c_int64 * 2)(0, -1)
    sh, fl = (ctypes.c_double * 4)(), (ctypes.c_double * 6)()
    good = dict(ctx=ctx, a=a, adt=0, aoff=off, b=b, bdt=1, boff=off, n=2, ny=40, nx=56, R=3, M=5, refine=1, scratch=ctypes.c_void_p(0x2000000),
                sh=sh, fl=fl, surf=None)
    for change in (dict(ctx=None), dict(a=None), dict(b=None), dict(aoff=None), dict(boff=None), dict(sh=None), dict(fl=None), dict(adt=2),
                   dict(bdt=-1), dict(n=0), dict(R=0), dict(R=33, M=33), dict(M=2), dict(ny=17), dict(nx=17), dict(aoff=neg), dict(boff=neg),
                   dict(refine=-1), dict(scratch=None)):
        g = {**good, **change}
        rc = L.rl_register_estimate(g['ctx'], g['a'], g['adt'], g['aoff'], g['b'], g['bdt'], g['boff'], g['n'], g['ny'], g['nx'], g['R'], g['M'],
                                    g['refine'], g['scratch'], g['sh'], g['fl'], g['surf'])
        assert rc == -1 and L.rl_last_error() != b'', change


def test_new_keywords_are_refused_without_a_device():
    from rescan_line_sted_amd import registration as reg
    a = np.zeros((2, 40, 48), dtype=np.float32)
    with pytest.raises(ValueError):
        reg.estimate_shifts(a, a[0], max_shift=2, coarse=4, device_peaks=True)
    raw, psfs = np.zeros((3, 46, 61), dtype=np.uint16), [np.ones((3, 3)) / 9.0]
    for kwargs in (dict(pipeline=True, coarse=8), dict(pipeline=True, out_dtype='f16'), dict(out_dtype='u16'), dict(out_dtype='f64'),
                   dict(out_scale=2.0), dict(out=np.zeros((3, 46, 61), dtype=np.float32)),
                   dict(pipeline=True, out=np.zeros((3, 46, 61), dtype=np.float64)), dict(pipeline=True, out_dtype='u16', out=np.zeros((2, 46, 61), dtype=np.uint16))):
        with pytest.raises(ValueError):
            reg.deconvolve_stack_registered(raw, psfs, 1, **kwargs)
