"""The ring statistics without a GPU: the host builder of the ring table and the kernel bodies of
rescan_line_sted_amd/csrc/ring_kernels.hpp, emulated on the host (tests/emu/ring_emu.cpp), against the exact-integer table and
numpy's fft2 (tests/ring_reference.py); and the arithmetic of the Python wrappers on synthetic field arrays.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ring_reference as rr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')


@pytest.fixture(scope='module')
def emu():
    so = os.environ.get('RLSTED_RING_EMU_LIB') or os.path.join(EMU_DIR, 'libring_emu.so')      # (tools/asan_emu.sh: a sanitized build)
    src = os.path.join(EMU_DIR, 'ring_emu.cpp')
    deps = [src] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f) for f in ('ring_kernels.hpp', 'fft_core.hpp')]
    if not os.environ.get('RLSTED_RING_EMU_LIB') and (not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas',
                               src, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_ring_of_bin.argtypes = [i, i, i, i, i]
    lib.emu_ring_table.argtypes = [i, i, i, vp, vp]
    lib.emu_ring_geometry.argtypes = [vp]
    lib.emu_ring_stats.restype = None
    lib.emu_ring_stats.argtypes = [vp, i, vp, vp, i, vp, vp, i, i, i, i, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _emu_table(emu, ny, nx, R):
    ring = np.full((ny, nx), -7, dtype=np.int32)
    row_ptr = np.zeros(R + 1, dtype=np.int32)
    assert emu.emu_ring_table(ny, nx, R, _p(ring), _p(row_ptr)) == 0       # (the CSR lists every bin once, in order)
    return ring, row_ptr


# ------------------------------------------------------------------ the ring table
@pytest.mark.parametrize('shape', [(8, 8), (24, 40), (37, 50), (128, 128), (160, 160), (96, 160), (512, 512)])
def test_ring_table_matches_the_integer_definition(emu, shape):
    ny, nx = shape
    R = rr.default_rings(ny, nx)
    want = rr.ring_table(ny, nx)
    got, row_ptr = _emu_table(emu, ny, nx, R)
    assert np.array_equal(got, want)
    assert np.array_equal(np.diff(row_ptr), np.bincount(want.ravel(), minlength=R + 1)[:R])
    if ny == nx and ny % 2 == 0:                       # for an even square image the ring is floor(sqrt(sy^2 + sx^2))
        s = np.where(np.arange(ny) <= ny // 2, np.arange(ny), np.arange(ny) - ny)
        r2 = s[:, None] ** 2 + s[None, :] ** 2
        fl = np.array([[min(int(np.floor(np.sqrt(v))), R) for v in row] for row in r2])
        fl -= (fl * fl > r2)                           # (sqrt of a perfect square is exact; this guards the rest)
        assert np.array_equal(want, np.minimum(fl, R))
    # a non-default ring count, the definition again
    R2 = R + 3
    assert np.array_equal(_emu_table(emu, ny, nx, R2)[0], rr.ring_table(ny, nx, R2))


def test_ring_table_160_where_a_float_formula_is_wrong(emu):
    """The eight bins (+-33, +-56), (+-56, +-33), radius exactly 65: float64 puts sqrt((sy/ny)^2 + (sx/nx)^2) * 2R a hair below the
    integer."""
    want = rr.ring_table(160, 160)
    flt = rr.float_ring_table(160, 160)
    wrong = np.argwhere(flt != want)
    print('bins where the float formula differs:', wrong.tolist())
    assert len(wrong) == 8                             # the case cannot go vacuous
    got, _ = _emu_table(emu, 160, 160, 80)
    for ky, kx in wrong:
        assert got[ky, kx] == want[ky, kx] == flt[ky, kx] + 1


def test_ring_of_bin_4096_spot_check(emu):
    """4 R^2 q reaches 2^71 here: the 128-bit compares."""
    rng = np.random.default_rng(4096)
    ks = rng.integers(0, 4096, size=(10000, 2))
    ks[:8] = [(2048, 2048), (2047, 2049), (0, 0), (4095, 4095), (1, 0), (0, 2048), (2048, 0), (1229, 1638)]
    for R in (2048, 4096):
        for ky, kx in ks.tolist():
            assert emu.emu_ring_of_bin(ky, kx, 4096, 4096, R) == rr.ring_of_bin(ky, kx, 4096, 4096, R), (ky, kx, R)
    assert (4 * 2048 ** 2 * 2 * (2048 * 4096) ** 2).bit_length() == 72          # 2^71, the corner bin at the default R
    ks2 = rng.integers(0, [4095, 4096], size=(2000, 2))          # a non-square, odd shape
    for ky, kx in ks2.tolist():
        assert emu.emu_ring_of_bin(ky, kx, 4095, 4096, 2047) == rr.ring_of_bin(ky, kx, 4095, 4096, 2047)


# ------------------------------------------------------------------ the emulated kernels
DT = {'f32': (np.float32, 0), 'f64': (np.float64, 1)}


def _run_emu(emu, a_buf, a_dt, a_off, b_buf, b_dt, b_off, scale, ny, nx, R, want_f=False):
    n = len(a_off)
    out = np.full((n, R, rr.FIELDS), np.nan)
    f = np.full((n, ny, nx, 2), np.nan) if want_f else None
    emu.emu_ring_stats(_p(a_buf), DT[a_dt][1], _p(np.asarray(a_off, dtype=np.int64)), _p(b_buf), DT[b_dt][1],
                       _p(np.asarray(b_off, dtype=np.int64)), _p(np.asarray(scale, dtype=np.float64)), n, ny, nx, R, _p(out),
                       _p(f) if want_f else None)
    return out, f


def check_against_reference(got, a, b, scale, R, label):
    """fields of one pair against ring_reference with the derived bound; the bound itself at most 1e-9 of field 1 in every ring."""
    want = rr.ring_stats(a, b, scale, R)
    bound = rr.bound(a, b, scale, R)
    assert np.array_equal(got[:, 0], want[:, 0])
    err = np.abs(got[:, 1:] - want[:, 1:]).max(axis=1)
    print('%s: max err / bound %.3g, max bound / field1 %.3g' % (label, float(np.max(err / bound)), float(np.max(bound / want[:, 1]))))
    assert np.all(bound <= 1e-9 * want[:, 1]), float(np.max(bound / want[:, 1]))
    assert np.all(err <= bound), (label, float(np.max(err / bound)))


@pytest.mark.parametrize('dtypes', [('f32', 'f32'), ('f32', 'f64'), ('f64', 'f64')])
@pytest.mark.parametrize('shape', [(8, 8), (24, 40), (37, 50), (64, 64)])
def test_emulated_kernels_match_numpy(emu, shape, dtypes):
    """PACK, both products, the unpack and the ring reduction as launched: tiles that overhang the image (every shape but 64 x 64),
    more than one tile and k step (none a multiple of 16 but 64), images at odd element offsets, a shared b image under three
    scales."""
    ny, nx = shape
    R = rr.default_rings(ny, nx)
    rng = np.random.default_rng(ny * 1000 + nx)
    a0, a1, _ = rr.poisson_pair(rng, ny, nx)
    b0, _, obj = rr.poisson_pair(rng, ny, nx)
    ta, tb = DT[dtypes[0]][0], DT[dtypes[1]][0]
    pix = ny * nx
    a_buf = np.zeros(2 * pix + 5, dtype=ta)                      # images at element offsets 3 and 3 + pix + 2, the second ends the buffer
    a_off = [3, 3 + pix + 2, 3]
    a_buf[3:3 + pix] = a0.ravel()
    a_buf[a_off[1]:a_off[1] + pix] = a1.ravel()
    b_buf = np.zeros(1 + 2 * pix, dtype=tb)
    b_off = [1, 1, 1 + pix]
    b_buf[1:1 + pix] = b0.ravel()
    b_buf[1 + pix:] = (obj * 0.37).astype(tb).ravel()
    scale = [1.0, 0.73, 1.0 / 0.37]
    got, f = _run_emu(emu, a_buf, dtypes[0], a_off, b_buf, dtypes[1], b_off, scale, ny, nx, R, want_f=True)
    for k in range(3):
        a = a_buf[a_off[k]:a_off[k] + pix].reshape(ny, nx).astype(np.float64)
        b = b_buf[b_off[k]:b_off[k] + pix].reshape(ny, nx).astype(np.float64)
        z = np.fft.fft2(a + 1j * (scale[k] * b))
        E = rr.gamma(rr.chain_length(ny, nx)) * (np.abs(a).sum() + abs(scale[k]) * np.abs(b).sum())
        assert np.max(np.abs(f[k, ..., 0] + 1j * f[k, ..., 1] - z)) <= 2 * E          # F = fft2(Z) (both spectra's errors)
        check_against_reference(got[k], a, b, scale[k], R, '%dx%d %s/%s pair %d' % (ny, nx, dtypes[0], dtypes[1], k))
    # a pair alone gives the bits it gives in the batch, and a non-default ring count works
    alone, _ = _run_emu(emu, a_buf, dtypes[0], a_off[1:2], b_buf, dtypes[1], b_off[1:2], scale[1:2], ny, nx, R)
    assert np.array_equal(alone[0], got[1])
    R2 = 2 * R + 1
    more, _ = _run_emu(emu, a_buf, dtypes[0], a_off[:1], b_buf, dtypes[1], b_off[:1], scale[:1], ny, nx, R2)
    want = rr.ring_stats(a0.astype(ta), b0.astype(tb), 1.0, R2)
    assert np.array_equal(more[0, :, 0], want[:, 0])
    assert np.all(np.abs(more[0, :, 1:] - want[:, 1:]).max(axis=1) <= rr.bound(a0.astype(ta), b0.astype(tb), 1.0, R2))


def test_emulator_geometry(emu):
    g = np.zeros(5, dtype=np.int32)
    assert emu.emu_ring_geometry(_p(g)) == 5
    assert g.tolist()[:4] == [256, 64, 16, rr.FIELDS] and g[4] <= 64 * 1024


# ------------------------------------------------------------------ the Python wrappers' arithmetic
def test_frc_and_radial_error_from_synthetic_fields():
    from rescan_line_sted_amd import quality
    st = np.zeros((2, 4, 5))
    st[0] = [[1, 4.0, 9.0, 6.0, 1.0], [8, 2.0, 8.0, 2.0, 32.0], [0, 0.0, 0.0, 0.0, 0.0], [4, 0.0, 5.0, 0.0, 16.0]]
    st[1] = [[1, 1.0, 1.0, -1.0, 4.0], [8, 16.0, 4.0, 4.0, 0.0], [3, 1.0, 4.0, 1.0, 3.0], [4, 9.0, 0.0, 0.0, 1.0]]
    c = quality.frc_from_stats(st)
    assert c.shape == (2, 4)
    assert np.allclose(c[0, :2], [1.0, 0.5]) and np.isnan(c[0, 2]) and np.isnan(c[0, 3])      # empty ring; zero denominator
    assert np.allclose(c[1, :3], [-1.0, 0.5, 0.5]) and np.isnan(c[1, 3])
    e = quality.radial_error_from_stats(st, (4, 5))
    assert np.allclose(e[0, [0, 1, 3]], np.array([1.0, 2.0, 2.0]) / 20) and np.isnan(e[0, 2])
    assert np.allclose(e[1], np.array([2.0, 0.0, 1.0, 0.5]) / 20)
    assert np.allclose(quality.ring_frequencies(4), [0.0625, 0.1875, 0.3125, 0.4375])
    assert quality.RING_FIELDS == rr.FIELDS


def test_frc_resolution():
    from rescan_line_sted_amd import quality
    f = quality.ring_frequencies(5)                      # 0.05, 0.15, 0.25, 0.35, 0.45
    # crosses 1/7 between rings 2 and 3: 0.5 -> 0.1, linear
    curve = np.array([1.0, 0.9, 0.5, 0.1, 0.3])
    fx = 0.25 + (0.5 - 1 / 7) / (0.5 - 0.1) * 0.1
    assert quality.frc_resolution(f, curve) == pytest.approx(1.0 / fx, rel=1e-14)
    assert quality.frc_resolution(f, curve, threshold=0.7) == pytest.approx(1.0 / (0.15 + 0.2 / 0.4 * 0.1), rel=1e-14)
    # nan rings are passed over: the crossing is interpolated between rings 1 and 3
    curve_nan = np.array([1.0, 0.9, np.nan, 0.1, 0.0])
    assert quality.frc_resolution(f, curve_nan, 0.5) == pytest.approx(1.0 / (0.15 + 0.4 / 0.8 * 0.2), rel=1e-14)
    assert quality.frc_resolution(f, np.array([0.1, 0.9, 0.9, 0.9, 0.9])) == pytest.approx(1.0 / 0.05)     # starts below
    assert quality.frc_resolution(f, np.array([1.0, 0.9, 0.8, 0.7, 0.6])) == float('inf')                  # never crosses
    assert quality.frc_resolution(f, np.full(5, np.nan)) == float('inf')


def test_abi_declares_the_ring_entry_points():
    from rescan_line_sted_amd import _lib, quality
    assert 'rl_ring_stats' in _lib.PROTOTYPES and 'rl_ring_count' in _lib.PROTOTYPES
    assert quality.ring_count(160, 128) == 64 and quality.ring_count(37, 50) == 18
    hdr = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert '#define RL_RING_FIELDS 5' in hdr and 'int rl_ring_stats(' in hdr


def test_ring_kernels_do_not_spill(tmp_path):
    """The neighbour of test_host_logic.py::test_default_path_kernels_do_not_spill: ring_kernels.hip compiled device-only with the
    flags of _build.py; the six kernels (ROWS x 4 type pairs, COLS, REDUCE) have `.private_segment_fixed_size` 0, and the two
    products' LDS is RingLds alone (nothing was moved there from registers)."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'ring_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'ring_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    lds = dict(zip(names, [int(x) for x in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', txt)]))
    assert len(priv) == 6 and sum('k_ring_rows' in k for k in priv) == 4, priv
    assert all(v == 0 for v in priv.values()), priv
    assert all(v == 33024 for k, v in lds.items() if 'k_ring_rows' in k or 'k_ring_cols' in k), lds
