"""Total-variation regularised Richardson-Lucy without a GPU: the kernel bodies of rescan_line_sted_amd/csrc/tv_kernels.hpp,
emulated on the host (tests/emu/tv_emu.cpp), against the numpy reference (tests/tv_reference.py) bit for bit; the reference
against the oracle and the figures the feature was proposed with; and the device build's scratch.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import line_sted_oracle as orc
from tv_reference import RegularisedRL, frame_means, low_dose_case, ordered_sums, rmse, tv_seminorm, tv_weight

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
TV_SUM_ONLY = 1
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (33, 65), (64, 64), (107, 109)]
FRAMES = 3


@pytest.fixture(scope='module')
def emu():
    so = os.environ.get('RLSTED_TV_EMU_LIB') or os.path.join(EMU_DIR, 'libtv_emu.so')      # (tools/asan_emu.sh: a sanitized build)
    src = os.path.join(EMU_DIR, 'tv_emu.cpp')
    deps = [src] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f) for f in ('tv_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
    if not os.environ.get('RLSTED_TV_EMU_LIB') and (not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas',
                               src, '-o', so])
    lib = ctypes.CDLL(so)
    lib.emu_tv_blocks.restype = ctypes.c_int
    lib.emu_tv_blocks.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    for sfx in ('f32', 'f64'):
        getattr(lib, 'emu_tv_weight_' + sfx).argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_double] * 2 + [ctypes.c_int] * 3
        getattr(lib, 'emu_tv_apply_' + sfx).argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _inputs(kind, ny, nx, dtype):
    rng = np.random.default_rng(ny * 1000 + nx)
    if kind == 'random':
        x = rng.random((FRAMES, ny, nx)) * 3.0
    elif kind == 'constant':
        x = np.full((FRAMES, ny, nx), 2.75)
    elif kind == 'zero':
        x = np.zeros((FRAMES, ny, nx))
    else:                                                    # one 1e6 spike per frame on a random background
        x = rng.random((FRAMES, ny, nx))
        for f in range(FRAMES):
            x[f, rng.integers(ny), rng.integers(nx)] = 1e6
    return np.ascontiguousarray(x.astype(dtype))


# ---------------------------------------------------------------------------------------------- 1. WEIGHT
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', SHAPES)
def test_emulated_weight_matches_numpy_bit_for_bit(emu, dtype, shape):
    """Three frames each: an odd frame size puts the second frame off 16-byte alignment (the element-wise path), an odd row
    length every second row; 107 x 109 has more than one tile both ways in f64 and a partial last tile."""
    ny, nx = shape
    sfx = 'f64' if dtype == np.float64 else 'f32'
    nb = emu.emu_tv_blocks(ny * nx, np.dtype(dtype).itemsize)
    for kind in ('random', 'constant', 'zero', 'spike'):
        x = _inputs(kind, ny, nx, dtype)
        part = np.full((FRAMES, nb), np.nan)
        getattr(emu, 'emu_tv_apply_' + sfx)(_p(x), None, _p(part), ny, nx, FRAMES, TV_SUM_ONLY)
        s = frame_means(part, ny * nx)
        for eps_rel in (1e-3, 0.1):
            for lam in (0.002, 0.25):
                w = np.full_like(x, np.nan)                      # (all zero: s = 0, eps2 = 0, 0 / 0 -- the same nan on both sides)
                getattr(emu, 'emu_tv_weight_' + sfx)(_p(x), _p(w), _p(part), lam, eps_rel, ny, nx, FRAMES)
                with np.errstate(invalid='ignore', divide='ignore'):
                    want, den = tv_weight(x, lam, eps_rel, s)
                assert w.dtype == want.dtype
                assert np.array_equal(w, want, equal_nan=True), (kind, eps_rel, lam, np.nanmax(np.abs(w - want)))
                if kind != 'zero':
                    assert np.all(den >= dtype(0.146)), (kind, eps_rel, lam, den.min())
                    assert np.all(np.isfinite(w))
                if kind == 'constant':
                    assert np.all(w == 1)


# ---------------------------------------------------------------------------------------------- 2. APPLY / SUM
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('n', [1, 7, 11449, 70000])
def test_emulated_apply_and_sum_match_numpy(emu, dtype, n):
    """Odd frame sizes put every second frame off 16-byte alignment and leave a partial last vector; 70000 pixels of float64 take
    more than one workgroup."""
    rng = np.random.default_rng(n)
    sfx = 'f64' if dtype == np.float64 else 'f32'
    nb = emu.emu_tv_blocks(n, np.dtype(dtype).itemsize)
    assert (nb > 1) == (n >= 11449)
    est = (rng.random((FRAMES, n)) * 5).astype(dtype)
    w = (0.8 + 0.4 * rng.random((FRAMES, n))).astype(dtype)
    x0 = est.copy()
    part = np.full((FRAMES, nb), np.nan)
    getattr(emu, 'emu_tv_apply_' + sfx)(_p(est), None, _p(part), 1, n, FRAMES, TV_SUM_ONLY)     # SUM: nothing stored
    assert np.array_equal(est, x0)
    assert np.array_equal(part, ordered_sums(x0, nb, 256))
    getattr(emu, 'emu_tv_apply_' + sfx)(_p(est), _p(w), _p(part), 1, n, FRAMES, 0)
    want = x0 * w
    assert want.dtype == np.dtype(dtype)
    assert np.array_equal(est, want)
    assert np.array_equal(part, ordered_sums(want, nb, 256))


def test_mean_of_ones_is_one(emu):
    for dtype, sfx in ((np.float32, 'f32'), (np.float64, 'f64')):
        for ny, nx in ((107, 109), (512, 512)):
            x = np.ones((1, ny, nx), dtype=dtype)
            nb = emu.emu_tv_blocks(ny * nx, x.itemsize)
            part = np.zeros((1, nb))
            getattr(emu, 'emu_tv_apply_' + sfx)(_p(x), None, _p(part), ny, nx, 1, TV_SUM_ONLY)
            assert frame_means(part, ny * nx)[0] == 1.0


# ---------------------------------------------------------------------------------------------- 3. the reference
def test_reference_reproduces_the_low_dose_gain():
    """Astronaut at 128 x 128, 6 photons per pixel (brightness 1e5), lambda = 0.01, eps_rel = 0.1: plain Richardson-Lucy fits the
    noise, the regularised loop does not.  The figures the feature was proposed with, within 1 %."""
    psfs, truth, noisy = low_dose_case(1e5)
    plain, tv = RegularisedRL(psfs, noisy, lam=0), RegularisedRL(psfs, noisy, lam=0.01, eps_rel=0.1)
    plain.iterate(20)
    tv.iterate(20)
    assert abs(rmse(plain.estimate, truth) / 1.004 - 1) <= 0.01, rmse(plain.estimate, truth)
    assert abs(rmse(tv.estimate, truth) / 0.953 - 1) <= 0.01, rmse(tv.estimate, truth)
    plain.iterate(180)
    tv.iterate(180)
    assert abs(rmse(plain.estimate, truth) / 2.394 - 1) <= 0.01, rmse(plain.estimate, truth)
    assert abs(rmse(tv.estimate, truth) / 1.117 - 1) <= 0.01, rmse(tv.estimate, truth)
    assert abs(tv_seminorm(plain.estimate) / 2.16e4 - 1) <= 0.01, tv_seminorm(plain.estimate)
    assert abs(tv_seminorm(tv.estimate) / 7.7e3 - 1) <= 0.01, tv_seminorm(tv.estimate)


def test_reference_with_lambda_zero_is_the_oracle():
    psfs, truth, noisy = low_dose_case(1e8)
    d = orc.Deconvolver(psfs)
    d.noisy_measurement = [m.copy() for m in noisy]
    ref = RegularisedRL(psfs, noisy, lam=0)
    ref.iterate(6)
    for _ in range(6):
        d.iterate()
    assert np.array_equal(ref.estimate, d.estimate)


# ---------------------------------------------------------------------------------------------- 4. the device build of the same bodies
def test_tv_kernels_do_not_spill(tmp_path):
    """The neighbour of test_host_logic.py::test_default_path_kernels_do_not_spill: tv_kernels.hip compiled device-only with the
    flags of _build.py; the four kernels (WEIGHT and APPLY x 2 types) have `.private_segment_fixed_size` 0."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'tv_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'tv_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    assert len(priv) == 4 and sum('k_tv_weight' in k for k in priv) == 2 and sum('k_tv_apply' in k for k in priv) == 2, priv
    assert all(v == 0 for v in priv.values()), priv
