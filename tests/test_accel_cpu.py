"""Biggs-Andrews acceleration without a GPU: the kernel bodies of rescan_line_sted_amd/csrc/accel_kernels.hpp, emulated on the
host (tests/emu/accel_emu.cpp), against numpy -- the dot products to the last bit of the float64 sums in the order the header
states -- and the numpy reference (tests/accel_reference.py) against the oracle.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from accel_reference import AcceleratedRL, clamp_alpha
from conftest import GOLDEN, ROOT
from oracle import line_sted_oracle as orc

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
ACC_Y_ONES, ACC_HAVE_PREV, ACC_FRESH = 1, 2, 4


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libaccel_emu.so')
    src = os.path.join(EMU_DIR, 'accel_emu.cpp')
    deps = [src] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f) for f in ('accel_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas',
                               src, '-o', so])
    lib = ctypes.CDLL(so)
    lib.emu_accel_blocks.restype = ctypes.c_int
    lib.emu_accel_blocks.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.emu_accel_alpha.restype = ctypes.c_double
    lib.emu_accel_alpha.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for sfx in ('f32', 'f64'):
        getattr(lib, 'emu_accel_reduce_' + sfx).argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        getattr(lib, 'emu_accel_extrapolate_' + sfx).argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ordered_sums(g, gp, nb, threads):
    """The two dot products of every workgroup of every frame in the order accel_kernels.hpp states: per thread over its
    vectors in increasing order (the W elements of a vector in order), then the workgroup tree.  g, gp: (frames, n)."""
    frames, n = g.shape
    W = 16 // g.itemsize
    nvec = -(-n // W)
    vpb = -(-nvec // nb)
    part = np.zeros((frames, nb, 2))
    a = g.astype(np.float64) * gp.astype(np.float64)
    d = gp.astype(np.float64) * gp.astype(np.float64)
    for f in range(frames):
        for b in range(nb):
            sn, sd = np.zeros(threads), np.zeros(threads)
            j0, j1 = b * vpb, min((b + 1) * vpb, nvec)
            for s in range(j0, j1, threads):                 # one round of vectors: thread t takes vector s + t
                m = min(threads, j1 - s)
                for c in range(W):
                    e = (np.arange(s, s + m) * W + c)
                    ok = e < n
                    sn[:m][ok] = sn[:m][ok] + a[f, e[ok]]
                    sd[:m][ok] = sd[:m][ok] + d[f, e[ok]]
            h = threads // 2
            while h > 0:
                sn[:h] = sn[:h] + sn[h:2 * h]
                sd[:h] = sd[:h] + sd[h:2 * h]
                h //= 2
            part[f, b] = sn[0], sd[0]
    return part


def frame_alpha(part):
    num = den = 0.0
    for b in range(part.shape[0]):
        num, den = num + part[b, 0], den + part[b, 1]
    return float(clamp_alpha(num, den))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('n', [1, 7, 11449, 5000, 70000])
def test_emulated_reduce_and_extrapolate_match_numpy(emu, dtype, n):
    """Odd frame sizes put every second frame off 16-byte alignment (the element-wise path) and leave a partial last vector."""
    rng = np.random.default_rng(n)
    sfx = 'f64' if dtype == np.float64 else 'f32'
    frames = 3
    nb = emu.emu_accel_blocks(n, np.dtype(dtype).itemsize)
    threads = emu.emu_accel_threads()
    x1 = rng.random((frames, n)).astype(dtype)           # x_{k+1}
    y = rng.random((frames, n)).astype(dtype)            # y_k
    gp = (rng.random((frames, n)) - 0.4).astype(dtype)   # g_{k-1}
    g = gp.copy()
    part = np.full((frames, nb, 2), np.nan)
    getattr(emu, 'emu_accel_reduce_' + sfx)(_p(x1), _p(y), _p(g), _p(part), n, frames, ACC_HAVE_PREV)
    g_ref = (x1 - y).astype(dtype)
    assert np.array_equal(g, g_ref)
    want = ordered_sums(g_ref, gp, nb, threads)
    assert np.array_equal(part, want), np.max(np.abs(part - want))
    # first step from ones: y is not read, the partials are 0
    g2, part2 = gp.copy(), np.full((frames, nb, 2), np.nan)
    getattr(emu, 'emu_accel_reduce_' + sfx)(_p(x1), _p(y), _p(g2), _p(part2), n, frames, ACC_Y_ONES)
    assert np.array_equal(g2, (x1 - dtype(1)).astype(dtype))
    assert np.all(part2 == 0)
    # extrapolation with the frames' a from those partials
    est, yb, xb = x1.copy(), np.zeros_like(x1), (x1 - rng.random((frames, n)).astype(dtype) * dtype(0.5)).astype(dtype)
    x_prev = xb.copy()
    alpha = np.full(frames, np.nan)
    getattr(emu, 'emu_accel_extrapolate_' + sfx)(_p(est), _p(yb), _p(xb), _p(part), _p(alpha), n, frames, 0)
    for f in range(frames):
        a = frame_alpha(want[f])
        assert alpha[f] == a
        assert alpha[f] == emu.emu_accel_alpha(_p(np.ascontiguousarray(want[f])), nb)
        v = x1[f] + dtype(a) * (x1[f] - x_prev[f]) if a != 0 else x1[f].copy()
        v = np.where(v > 0, v, dtype(0)).astype(dtype)
        assert np.array_equal(est[f], v)
        assert np.array_equal(yb[f], v)
        assert np.array_equal(xb[f], x1[f])
    # no history: a = 0, y = max(x, 0), the previous point is not read
    est, xb = (x1 - dtype(0.5)).astype(dtype), np.full_like(x1, np.nan)
    getattr(emu, 'emu_accel_extrapolate_' + sfx)(_p(est), _p(yb), _p(xb), _p(part), _p(alpha), n, frames, ACC_FRESH)
    assert np.all(alpha == 0)
    assert np.array_equal(est, np.where(x1 - dtype(0.5) > 0, x1 - dtype(0.5), dtype(0)).astype(dtype))


def test_alpha_rule(emu):
    cases = [((1.0, 4.0), 0.25), ((-1.0, 4.0), 0.0), ((9.0, 4.0), 1.0), ((1.0, 0.0), 0.0), ((1.0, np.inf), 0.0),
             ((np.nan, 1.0), 0.0), ((np.inf, 1.0), 1.0)]
    for (num, den), want in cases:
        part = np.array([num, den], dtype=np.float64)
        assert emu.emu_accel_alpha(_p(part), 1) == want
        assert float(clamp_alpha(num, den)) == want


def _astronaut_case(views):
    g = np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))
    psfs = list(g['1p5x_lr/line_sted_psfs']) if views == 3 else list(g['1p5x_lr/point_sted_psf'])
    obj = np.load(os.path.join(GOLDEN, 'objects.npz'))['astronaut'].astype(np.float64)[:, :64, :64]
    d = orc.Deconvolver(psfs)
    d.create_data_from_object(obj.copy(), total_brightness=1e8, random_seed=3)
    return psfs, obj, d


@pytest.mark.parametrize('views', [1, 3])
def test_reference_with_alpha_zero_is_plain_rl(views):
    psfs, obj, d = _astronaut_case(views)
    acc = AcceleratedRL(psfs, d.noisy_measurement, force_alpha_zero=True)
    acc.iterate(6)
    for _ in range(6):
        d.iterate()
    assert np.max(np.abs(acc.estimate - d.estimate)) <= 1e-12 * np.max(d.estimate)
    assert np.all(acc.alpha == 0)


def test_reference_accelerates_and_restarts():
    psfs, obj, d = _astronaut_case(1)
    acc = AcceleratedRL(psfs, d.noisy_measurement)
    acc.iterate(2)
    assert np.all(acc.alpha == 0)                # a_1 = 0: the first extrapolated point is x_1
    acc.iterate(3)
    assert np.all(acc.alpha > 0)
    five = acc.estimate.copy()
    again = AcceleratedRL(psfs, d.noisy_measurement)
    again.iterate(5)
    assert np.array_equal(again.estimate, five)
    again.set_estimate(five)
    again.iterate(1)
    assert np.all(again.alpha == 0)
