"""The angle-resolved ring statistics without a GPU (include/rlsted.h rl_ring_sector_stats): the host builder of the sector table and
the body of k_ring_reduce_sectors (rescan_line_sted_amd/csrc/ring_kernels.hpp), emulated on the host (tests/emu/sector_emu.cpp),
against the exact big-integer sector oracle and numpy's fft2 (tests/sector_reference.py); the same code as a stand-alone program
under the address and undefined-behaviour sanitizers; and the arithmetic of the Python wrappers on synthetic arrays.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ring_reference as rr
import sector_reference as sr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'sector_emu.cpp')


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libsector_emu.so')
    deps = [SRC, os.path.join(EMU_DIR, 'ring_emu.cpp')] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f)
                                                           for f in ('ring_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_sector_of_bin.argtypes = [i, i, i, i, i]
    lib.emu_sector_table.argtypes = [i, i, i, i, vp, vp]
    lib.emu_ring_table.argtypes = [i, i, i, vp, vp]
    lib.emu_sector_stats.argtypes = [vp, i, vp, vp, i, vp, vp, i, i, i, i, i, vp]
    lib.emu_ring_stats.restype = None
    lib.emu_ring_stats.argtypes = [vp, i, vp, vp, i, vp, vp, i, i, i, i, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _emu_table(emu, ny, nx, R, S):
    cell = np.full((ny, nx), -7, dtype=np.int32)
    cell_ptr = np.zeros(R * S + 1, dtype=np.int32)
    assert emu.emu_sector_table(ny, nx, R, S, _p(cell), _p(cell_ptr)) == 0        # (the CSR lists every ring bin once, in order)
    return cell, cell_ptr


# ------------------------------------------------------------------ the sector table
# bins that lie exactly on a sector boundary (X = 0 for odd S, |Y| = |X| for S = 2 mod 4), counted over the whole plane
TIES = {((160, 160), 3): 159, ((160, 160), 6): 317, ((24, 40), 2): 13, ((37, 50), 3): 36}
SECTORS = (1, 2, 3, 4, 6, 12)


@pytest.mark.parametrize('shape', [(8, 8), (24, 40), (37, 50), (96, 160), (160, 160), (512, 512)])
def test_sector_table_matches_the_exact_oracle(emu, shape):
    ny, nx = shape
    R = rr.default_rings(ny, nx)
    ring_of = np.full((ny, nx), -7, dtype=np.int32)
    row_ptr = np.zeros(R + 1, dtype=np.int32)
    assert emu.emu_ring_table(ny, nx, R, _p(ring_of), _p(row_ptr)) == 0
    for S in SECTORS:
        sec, tie = sr.sector_table(ny, nx, S)
        if (shape, S) in TIES:
            assert int(tie.sum()) == TIES[(shape, S)]                                # the tie cases cannot go vacuous
        if S % 2 == 0 and S % 4 != 2:
            assert not tie.any()
        got, cell_ptr = _emu_table(emu, ny, nx, R, S)
        want = sr.cell_table(ny, nx, S, R)
        assert np.array_equal(got, want), (S, np.argwhere(got != want)[:5].tolist())
        sizes = np.diff(cell_ptr).reshape(R, S)
        assert np.array_equal(sizes.sum(axis=1), np.diff(row_ptr))                   # a ring's cells are the ring, exactly
        assert np.array_equal(sizes.ravel(), np.bincount(want.ravel(), minlength=R * S + 1)[:R * S])
    R2 = R + 3                                                                       # a non-default ring count
    assert np.array_equal(_emu_table(emu, ny, nx, R2, 6)[0], sr.cell_table(ny, nx, 6, R2))


def test_tie_bins_go_to_the_upper_sector(emu):
    """By hand: 90 degrees with S = 3 (sectors centred on 0, 60, 120; the boundary of 1 and 2) belongs to sector 2; 45 degrees with
    S = 2 to sector 1, 135 degrees to sector 0 (which wraps around 180); with S = 6, 45 degrees is the boundary of 1 and 2."""
    assert emu.emu_sector_of_bin(5, 0, 37, 50, 3) == sr.sector_of_bin(5, 0, 37, 50, 3)[0] == 2
    assert sr.sector_of_bin(5, 0, 37, 50, 3)[1]
    assert emu.emu_sector_of_bin(3, 5, 24, 40, 2) == sr.sector_of_bin(3, 5, 24, 40, 2)[0] == 1
    assert emu.emu_sector_of_bin(24 - 3, 5, 24, 40, 2) == sr.sector_of_bin(24 - 3, 5, 24, 40, 2)[0] == 0
    assert emu.emu_sector_of_bin(7, 7, 160, 160, 6) == sr.sector_of_bin(7, 7, 160, 160, 6)[0] == 2
    assert emu.emu_sector_of_bin(160 - 7, 7, 160, 160, 6) == sr.sector_of_bin(160 - 7, 7, 160, 160, 6)[0] == 5
    assert emu.emu_sector_of_bin(0, 0, 160, 160, 6) == 0                             # DC
    assert emu.emu_sector_of_bin(0, 9, 160, 160, 6) == 0 and emu.emu_sector_of_bin(0, 160 - 9, 160, 160, 6) == 0


def test_sector_of_bin_4096_spot_check(emu):
    rng = np.random.default_rng(4096)
    for ny, nx in ((4096, 4096), (4095, 4096)):
        ks = rng.integers(0, [ny, nx], size=(10000, 2))
        ks[:6] = [(2048, 2048), (2047, 2049), (0, 0), (1, 0), (0, 2048), (1229, 1638)]
        for n, (ky, kx) in enumerate(ks.tolist()):
            S = (2, 3, 6, 12, 5, 64)[n % 6]
            assert emu.emu_sector_of_bin(ky, kx, ny, nx, S) == sr.sector_of_bin(ky, kx, ny, nx, S)[0], (ky, kx, ny, nx, S)


# ------------------------------------------------------------------ the emulated reduce
DT = {'f32': (np.float32, 0), 'f64': (np.float64, 1)}
def _run_emu(emu, a_buf, a_dt, a_off, b_buf, b_dt, b_off, scale, ny, nx, R, S):
    n = len(a_off)
    out = np.full((n, R, S, sr.FIELDS), np.nan)
    assert emu.emu_sector_stats(_p(a_buf), DT[a_dt][1], _p(np.asarray(a_off, dtype=np.int64)), _p(b_buf), DT[b_dt][1],
                                _p(np.asarray(b_off, dtype=np.int64)), _p(np.asarray(scale, dtype=np.float64)), n, ny, nx, R, S,
                                _p(out)) == 0
    return out


@pytest.mark.parametrize('dtypes', [('f32', 'f32'), ('f32', 'f64'), ('f64', 'f64')])
@pytest.mark.parametrize('case', [((8, 8), 12), ((37, 50), 6), ((96, 160), 5), ((160, 160), 1)])
def test_emulated_sector_reduce_matches_numpy(emu, case, dtypes):
    """k_ring_reduce_sectors lane by lane on the emulated F: mostly empty cells (8 x 8, S = 12), sectors that are no multiple of the
    four waves (S = 5, 6), cells of several hundred bins -- the stride loop and the whole tree (160 x 160, S = 1); two pairs at odd
    element offsets, the second against a scaled b."""
    (ny, nx), S = case
    R = rr.default_rings(ny, nx)
    rng = np.random.default_rng(ny * 7 + nx)
    a0, b0, _ = rr.poisson_pair(rng, ny, nx, *sr.LEVEL[(ny, nx)])
    ta, tb = DT[dtypes[0]][0], DT[dtypes[1]][0]
    pix = ny * nx
    a_buf = np.zeros(2 * pix + 4, dtype=ta)
    a_off = [1, 1 + pix + 2 - (pix % 2)]
    a_buf[a_off[0]:a_off[0] + pix] = a0.ravel()
    a_buf[a_off[1]:a_off[1] + pix] = b0.ravel()
    b_buf = np.zeros(3 + pix, dtype=tb)
    b_off = [3, 3]
    b_buf[3:] = b0.ravel()
    scale = [1.0, 0.73]
    got = _run_emu(emu, a_buf, dtypes[0], a_off, b_buf, dtypes[1], b_off, scale, ny, nx, R, S)
    empty = sr.check_cells(got[0], a0, b0, 1.0, R, S, '%dx%d S=%d %s/%s (a, b)' % (ny, nx, S, dtypes[0], dtypes[1]))
    sr.check_cells(got[1], b0, b0, 0.73, R, S, '%dx%d S=%d %s/%s (b, 0.73 b)' % (ny, nx, S, dtypes[0], dtypes[1]))
    if (ny, nx) == (8, 8):
        assert empty > R * S // 2                                                    # the empty cells are there
    if S == 1:
        assert got[0, :, 0, 0].max() > 4 * 64                                        # cells that take several passes of the wave
    alone = _run_emu(emu, a_buf, dtypes[0], a_off[1:], b_buf, dtypes[1], b_off[1:], scale[1:], ny, nx, R, S)
    assert np.array_equal(alone[0], got[1])                                          # a pair alone gives the bits it gives in the batch


@pytest.mark.parametrize('shape,S,f,sector', sr.GRATINGS)
def test_gratings_land_in_their_sector(emu, shape, S, f, sector):
    ny, nx = shape
    a = sr.grating(ny, nx, *f)
    got = _run_emu(emu, a.ravel(), 'f64', [0], np.zeros(ny * nx), 'f64', [0], [1.0], ny, nx, rr.default_rings(ny, nx), S)
    sr.check_grating(got[0], shape, S, f, sector)


@pytest.mark.parametrize('case', [((37, 50), 6), ((24, 40), 5), ((64, 64), 1)])
def test_sector_sums_give_the_ring_statistics(emu, case):
    (ny, nx), S = case
    R = rr.default_rings(ny, nx)
    rng = np.random.default_rng(ny + nx + S)
    a, b, _ = rr.poisson_pair(rng, ny, nx)
    args = (_p(a), 1, _p(np.zeros(1, dtype=np.int64)), _p(b), 1, _p(np.zeros(1, dtype=np.int64)), _p(np.array([0.61])), 1, ny, nx, R)
    ring = np.full((1, R, rr.FIELDS), np.nan)
    emu.emu_ring_stats(*args, _p(ring), None)
    sec = np.full((1, R, S, sr.FIELDS), np.nan)
    assert emu.emu_sector_stats(*args, S, _p(sec)) == 0
    assert np.array_equal(sec[0, ..., 0].sum(axis=1), ring[0, :, 0])
    allow = sr.bound(a, b, S, 0.61, R).sum(axis=1) + rr.bound(a, b, 0.61, R)
    err = np.abs(sec[0].sum(axis=1)[:, 1:] - ring[0, :, 1:]).max(axis=1)
    print('%dx%d S=%d: max |sum over sectors - ring| / allowance %.3g' % (ny, nx, S, float(np.max(err / allow))))
    assert np.all(err <= allow)


def test_table_builder_and_reduce_under_sanitizers(tmp_path):
    """sector_emu.cpp as a stand-alone program (its own main: tables over shapes and sector counts up to 64, the emulated kernels on
    pairs at odd offsets) built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / 'sector_emu_main')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-ffp-contract=off',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DSECTOR_EMU_MAIN', SRC, '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith('ok 84 ')


# ------------------------------------------------------------------ the Python wrappers' arithmetic
def test_sector_arithmetic_on_synthetic_fields():
    from rescan_line_sted_amd import quality
    assert np.allclose(quality.sector_angles(6), [0, 30, 60, 90, 120, 150]) and np.allclose(quality.sector_angles(1), [0])
    rng = np.random.default_rng(5)
    st = rng.integers(0, 9, size=(3, 4, 6, 5)).astype(np.float64)
    rings = quality.rings_from_sectors(st)
    assert rings.shape == (3, 4, 5) and np.array_equal(rings[1, 2], st[1, 2].sum(axis=0))
    # the readers work per cell as they do per ring, an empty cell is nan
    one = np.zeros((2, 2, 5))
    one[0, 0] = [2, 4.0, 9.0, 3.0, 8.0]
    one[1, 1] = [4, 1.0, 1.0, 1.0, 16.0]
    c = quality.frc_from_stats(one)
    assert c.shape == (2, 2) and c[0, 0] == 0.5 and c[1, 1] == 1.0 and np.isnan(c[0, 1]) and np.isnan(c[1, 0])
    e = quality.radial_error_from_stats(one, (2, 5))
    assert e.shape == (2, 2) and np.allclose([e[0, 0], e[1, 1]], [0.2, 0.2]) and np.isnan(e[0, 1])


def test_frc_resolution_by_angle():
    from rescan_line_sted_amd import quality
    f = quality.ring_frequencies(5)
    curves = np.array([[1.0, 0.9, 0.5, 0.1, 0.3], [1.0, 0.9, 0.8, 0.7, 0.6], [0.1, 0.9, 0.9, 0.9, 0.9]]).T      # [R][S]
    st = np.zeros((5, 3, 5))
    st[..., 0] = 4
    st[..., 1] = st[..., 2] = 2.0
    st[..., 3] = 2.0 * curves                                                        # f3 / sqrt(f1 f2) = the curve
    got = quality.frc_resolution_by_angle(st)
    assert got.shape == (3,)
    assert got[0] == pytest.approx(quality.frc_resolution(f, curves[:, 0]), rel=1e-14) and got[1] == float('inf')
    assert got[2] == pytest.approx(1.0 / 0.05)
    assert quality.frc_resolution_by_angle(st, threshold=0.7)[0] == pytest.approx(quality.frc_resolution(f, curves[:, 0], 0.7), rel=1e-14)
    with pytest.raises(ValueError):
        quality.frc_resolution_by_angle(np.zeros((2, 5, 3, 5)))


def test_abi_and_signatures_declare_the_sector_entry_points():
    import inspect
    from rescan_line_sted_amd import _lib, quality, sweep
    assert 'rl_ring_sector_stats' in _lib.PROTOTYPES and len(_lib.PROTOTYPES['rl_ring_sector_stats'][1]) == 14
    hdr = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_ring_sector_stats(' in hdr
    for fn in (sweep.DeviceResults.ring_stats, sweep.score_tasks, sweep.frc_between_seeds, sweep.run_and_score_tasks,
               sweep.figure_2_sweep, quality.ring_stats):
        assert inspect.signature(fn).parameters['n_sectors'].default is None, fn
    for name in ('sector_stats_device', 'sector_stats', 'directional_fourier_error'):
        assert 'n_sectors' in inspect.signature(getattr(quality, name)).parameters


def test_sector_kernel_does_not_spill(tmp_path):
    """ring_sector_kernels.hip compiled device-only with the flags of _build.py: one kernel, no scratch, no LDS."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'ring_sector_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'ring_sector_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    assert len(re.findall(r'\.name:\s+\S*k_ring_reduce_sectors\S*', txt)) == 1
    assert [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)] == [0]
    assert [int(x) for x in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', txt)] == [0]
