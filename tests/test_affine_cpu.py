"""Affine registration without a GPU (include/rlsted.h rl_warp_images, rl_affine_sums; rescan_line_sted_amd/registration.py): the
bodies of the kernels emulated thread by thread (tests/emu/warp_emu.cpp) against the twin (tests/affine_reference.py) -- the warp
within the derived bound of the long double twin and of scipy.ndimage.affine_transform, both paths with the same bits, the
statistics bit for bit, the sums within their bound and bit-identical across runs and pair orderings; the same bodies as a
stand-alone program under the address and undefined-behaviour sanitizers; the twin of the whole method against the analytic truth;
the argument checks; the device build's private segments; and the wrappers on a numpy stand-in for the device.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import affine_reference as ar
import register_reference as rr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'warp_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('affine_kernels.hpp', 'register_kernels.hpp', 'ingest_kernels.hpp', 'tile_kernels.hpp', 'accel_kernels.hpp',
                                        'fft_core.hpp')]
FLOATS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
ROUND = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
# scipy.ndimage.affine_transform against the long double twin, in units of max|src|.  scipy forms its coordinates in another order
# than the kernel's two fused multiply-adds: they differ by a few units in the last place of the coordinate, and a spline of
# coefficients <= 9 max|src| moves by at most 18 max|src| per pixel -- that term is taken per case from the largest coordinate
# ('far': 1.3e-10 at 1e4).  What is left -- scipy's own recursive prefilter and float64 evaluation -- was measured over every case
# below: at most 3.4e-14 (130 x 70, order 3; 7.8e-15 at 37 x 53, 2.1e-15 below); asserted at 1e-13.
SCIPY_DISTANCE = 1e-13
# the twin of the whole method on the committed scenes (96 x 128, SEEDS, noise on): the worst corner displacement error per model,
# measured; asserted at twice these, and the assertion itself stays below 0.5 px where the untreated corner moves 3.2 - 4.4 px
TWIN_ERROR = {'rigid': 0.111, 'similarity': 0.163, 'affine': 0.140}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _build(src, so, deps):
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [src] + deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', src, '-o', so])
    return ctypes.CDLL(so)


@pytest.fixture(scope='module')
def emu():
    lib = _build(SRC, os.path.join(EMU_DIR, 'libwarp_emu.so'), DEPS)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_warp_images.argtypes = [vp, i, i, i, i, vp, i, d, vp, i, i, i, vp, i, vp]
    lib.emu_affine_sums.argtypes = [vp, i, vp, vp, i, vp, i, i, i, i, vp, vp]
    return lib


@pytest.fixture(scope='module')
def shift_emu():
    lib = _build(os.path.join(EMU_DIR, 'register_emu.cpp'), os.path.join(EMU_DIR, 'libregister_emu.so'), DEPS[1:])
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_shift_images.argtypes = [vp, i, i, i, i, vp, i, d, vp, i, vp]
    return lib


def emu_warp(emu, src, xf, order, floor, dst_dtype, out_shape, direct=0):
    """(dst (n, oy, ox), stats (n, 2), staged tiles) of the emulation, guard values around the destination checked."""
    n, sy, sx = src.shape
    oy, ox = out_shape
    xf = np.ascontiguousarray(xf, dtype=np.float64).reshape(n, 6)
    whole = np.full(n * oy * ox + 16, 7, dtype=dst_dtype)
    dst = whole[8:8 + n * oy * ox]
    stats, staged = np.full((n, 2), np.nan), ctypes.c_long(-1)
    assert emu.emu_warp_images(_p(src), FLOATS[src.dtype], n, sy, sx, _p(xf), order, -np.inf if floor is None else floor, _p(dst),
                               FLOATS[np.dtype(dst_dtype)], oy, ox, _p(stats), direct, ctypes.addressof(staged)) == 0
    assert np.all(whole[:8] == 7) and np.all(whole[8 + n * oy * ox:] == 7)
    return dst.reshape(n, oy, ox).copy(), stats, staged.value


# ---- the warp ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('order', [1, 3])
@pytest.mark.parametrize('shapes', ar.WARP_SHAPES, ids=lambda s: '%dx%d' % s[0])
def test_emulated_warp_is_the_twin_and_scipy(emu, shapes, order):
    """Every source shape (1 x 1; 1 x 17; 5 x 7, where the mirror extension wraps several times inside the taps' reach; 37 x 53 into
    41 x 29; 130 x 70) under every transform of warp_cases (identity, a fractional translation, rotations by 0.7, 30 and 90 degrees,
    scale 1.03, a shear, an offset of 1e4, a shrink by 3 whose footprint does not fit the LDS budget), f32 and f64 sources, f64 and
    f32 destinations: within the twin's bound plus the destination's rounding; within that, the tail and scipy's own distance of
    scipy; guard values intact; no pixel raised; the sum of the stored image bit for bit in the fixed order; the direct path forced
    on the same inputs gives the same bits."""
    (sy, sx), out_shape = shapes
    rng = np.random.default_rng(sy * 1000 + sx + order)
    cases = ar.warp_cases((sy, sx))
    names = list(cases)
    xf = np.stack([cases[k] for k in names])
    worst_twin = worst_scipy = 0.0
    for dt in (np.float32, np.float64):
        one = (rng.random((sy, sx)) * 1000.0).astype(dt)
        src = np.ascontiguousarray(np.broadcast_to(one, (len(names), sy, sx)))
        A = float(np.abs(one).max())
        coef = ar.coefficients(one) if order == 3 else None
        twins = [ar.warp(one, xf[k], out_shape, order, coef) for k in range(len(names))]
        for ddt in (np.float64, np.float32):
            got, stats, staged = emu_warp(emu, src, xf, order, None, ddt, out_shape)
            direct, dstats, none = emu_warp(emu, src, xf, order, None, ddt, out_shape, direct=1)
            assert none == 0 and direct.tobytes() == got.tobytes() and dstats.tobytes() == stats.tobytes()
            assert np.all(stats[:, 0] == 0)
            for k, name in enumerate(names):
                want, bound = twins[k]
                tol = bound + ROUND[np.dtype(ddt)] * np.abs(want).astype(np.float64) * (1 + 2.0 ** -20)
                err = np.abs(got[k].astype(np.longdouble) - want).astype(np.float64)
                assert np.all(err <= tol), (name, np.dtype(dt).name, np.dtype(ddt).name, (err / tol).max())
                assert stats[k, 1] == ar.stored_sum(got[k]), name
                if ddt is np.float64:
                    worst_twin = max(worst_twin, float((err / np.maximum(tol, 1e-300)).max()))
                    Y, X = ar.coords(xf[k], *out_shape)
                    coord = 18.0 * 4.0 * max(np.spacing(np.abs(Y).max()), np.spacing(np.abs(X).max()))
                    serr = np.abs(got[k] - ar.scipy_warp(one, xf[k], out_shape, order))
                    stol = tol + (SCIPY_DISTANCE + ar.TAIL + coord) * A
                    assert np.all(serr <= stol), (name, np.dtype(dt).name, (serr / stol).max())
                    if name != 'far':
                        worst_scipy = max(worst_scipy, float(np.abs(want.astype(np.float64) - ar.scipy_warp(one, xf[k], out_shape, order)).max() / A))
        assert staged > 0
    print('%d x %d order %d: worst error / bound %.3g, scipy - twin %.3g max|src|' % (sy, sx, order, worst_twin, worst_scipy))
    assert worst_scipy <= SCIPY_DISTANCE


def test_shrink_by_three_reads_directly_and_small_rotations_and_binning_are_staged(emu):
    """The path each transform takes on 130 x 70 -> 130 x 70: every tile of the identity, the rotations (30 degrees included) and
    2 x binning (order 1, 130 x 70 -> 65 x 35) is staged; a tile of 32 x 32 shrunk by three has a footprint of about 100 x 100
    samples and reads global memory."""
    src = np.random.default_rng(2).random((1, 130, 70))
    cases = ar.warp_cases((130, 70))
    tiles = 5 * 3
    for name in ('identity', 'rot0.7', 'rot30', 'rot90', 'far'):
        for order in (1, 3):
            assert emu_warp(emu, src, cases[name], order, None, np.float64, (130, 70))[2] == tiles, name
    assert emu_warp(emu, src, cases['shrink3'], 3, None, np.float64, (130, 70))[2] < tiles
    assert emu_warp(emu, src, cases['shrink3'], 3, None, np.float64, (32, 32))[2] == 0
    assert emu_warp(emu, src, np.array([2.0, 0.0, 0.0, 2.0, 0.5, 0.5]), 1, None, np.float64, (65, 35))[2] == 3 * 2


def test_binning_is_the_two_by_two_mean_bit_for_bit(emu):
    from rescan_line_sted_amd import registration as reg
    rng = np.random.default_rng(3)
    for sy, sx in ((37, 53), (130, 70), (2, 2)):
        for dt in (np.float32, np.float64):
            src = ((rng.random((2, sy, sx)) - 0.3) * 1e4).astype(dt)
            got, _, _ = emu_warp(emu, src, np.tile(reg.BIN2, (2, 1)), 1, None, np.float64, (sy // 2, sx // 2))
            for k in range(2):
                assert got[k].tobytes() == ar.bin2(src[k]).tobytes()


def test_fractional_translation_agrees_with_the_emulated_shift(emu, shift_emu):
    """A pure translation through the warp (prefilter, then the evaluation) and through rl_shift_images (one fused FIR per axis):
    two roundings of the same spline, each within a bound of this kind -- they differ by at most twice the warp's."""
    rng = np.random.default_rng(4)
    for sy, sx in ((5, 7), (37, 53), (130, 70)):
        src = rng.random((1, sy, sx)) * 1000.0
        s = np.array([[0.37, -0.81]])
        got, _, _ = emu_warp(emu, src, np.array([1.0, 0.0, 0.0, 1.0, s[0, 0], s[0, 1]]), 3, None, np.float64, (sy, sx))
        ref = np.empty_like(src)
        assert shift_emu.emu_shift_images(_p(src), 1, 1, sy, sx, _p(s), 3, -np.inf, _p(ref), 1, None) == 0
        _, bound = ar.warp(src[0], [1.0, 0.0, 0.0, 1.0, s[0, 0], s[0, 1]], (sy, sx), 3)
        assert np.all(np.abs(got[0] - ref[0]) <= 2.0 * bound + 2.0 ** -52 * np.abs(ref[0]))


def test_order_one_with_integer_translations_copies_the_displaced_pixels_bit_for_bit(emu):
    rng = np.random.default_rng(5)
    for dt in (np.float32, np.float64):
        src = ((rng.random((3, 37, 53)) - 0.5) * 1e6).astype(dt)
        src[0, 0, 0] = -0.0
        src[1, 5, 5] = np.inf                                              # (a zero weight does not read its sample: no nan around it)
        shifts = [(0.0, 0.0), (3.0, -2.0), (-40.0, 75.0)]
        xf = np.array([[1.0, 0.0, 0.0, 1.0, sy, sx] for sy, sx in shifts])
        for direct in (0, 1):
            got, _, _ = emu_warp(emu, src, xf, 1, None, dt, (37, 53), direct)
            for k, (sy, sx) in enumerate(shifts):
                iy = np.pad(np.arange(37), 120, mode='reflect')[120 + int(sy):120 + int(sy) + 37]
                ix = np.pad(np.arange(53), 120, mode='reflect')[120 + int(sx):120 + int(sx) + 53]
                assert got[k].tobytes() == src[k][iy][:, ix].tobytes()


def test_floor_and_raised_count_are_exact(emu):
    """A bright square on zero rotated by 5 degrees: the cubic spline rings below zero beside its edges.  The floor and the count of
    raised pixels are exact where the twin is not within 1e-9 of the floor; the stored sum is the fixed-order sum of what is stored."""
    src = np.zeros((1, 40, 56))
    src[0, 12:28, 20:40] = 1000.0
    xf = ar.centred(ar.rotation(5.0)[:, :2], (0.4, -0.3), (40, 56))
    want = ar.warp(src[0], xf, (40, 56), 3)[0].astype(np.float64)
    assert want.min() < -10.0
    floor = 1e-9
    for ddt in (np.float64, np.float32):
        got, stats, _ = emu_warp(emu, src, xf, 3, floor, ddt, (40, 56))
        stored = ddt(floor)
        sure = np.abs(want - floor) > 1e-9
        assert np.all(got >= stored) and np.all(got[0][sure & (want < floor)] == stored)
        low, high = int((want < floor - 1e-9).sum()), int((want < floor + 1e-9).sum())
        assert low <= stats[0, 0] <= high and low > 50, (low, stats, high)
        assert stats[0, 0] == (got == stored).sum() and stats[0, 1] == ar.stored_sum(got[0])


# ---- the sums ------------------------------------------------------------------------------------------------------------------------

def emu_aff(emu, a, a_off, w, w_off, ny, nx, M):
    n = len(a_off)
    S, geom = np.full((n, 45), np.nan), np.zeros(2, dtype=np.intc)
    ao, wo = np.asarray(a_off, dtype=np.int64), np.asarray(w_off, dtype=np.int64)
    assert emu.emu_affine_sums(_p(a), FLOATS[a.dtype], _p(ao), _p(w), FLOATS[w.dtype], _p(wo), n, ny, nx, M, _p(S), _p(geom)) == 0
    return S, geom


@pytest.mark.parametrize('ny,nx,M', [(10, 10, 1), (37, 53, 4), (48, 64, 4), (100, 120, 2)])
def test_emulated_affine_sums_are_within_the_bound_of_the_twin(emu, ny, nx, M):
    """Five pairs over three f32 references and five f64 warped images at non-trivial offsets (shared references), and the dtypes
    the other way round: each of the 45 sums within gamma_n sum |term| of the long double twin (100 x 120: two runs per pair); a
    second run and a reversed pair order give the same bits; a pair computed alone gives the same bits as in the call of five."""
    rng = np.random.default_rng(ny * 100 + M)
    n_pix = ny * nx
    for ta, tw in ((np.float32, np.float64), (np.float64, np.float32)):
        a = (rng.random(3 * n_pix + 5) * 100.0).astype(ta)
        w = (rng.random(5 * n_pix + 3) * 100.0).astype(tw)
        a_off = [5, n_pix + 5, 5, 2 * n_pix + 5, n_pix + 5]
        w_off = [3 + k * n_pix for k in (4, 0, 2, 1, 3)]
        S, geom = emu_aff(emu, a, a_off, w, w_off, ny, nx, M)
        assert geom[0] == -(-((ny - 2 * M) * (nx - 2 * M)) // 8192)
        worst = 0.0
        for i in range(5):
            want, bound = ar.affine_sums(a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), w[w_off[i]:w_off[i] + n_pix].reshape(ny, nx), M)
            err = np.abs(S[i].astype(np.longdouble) - want).astype(np.float64)
            assert np.all(err <= bound), (i, (err / bound).max())
            assert S[i, 35] == (ny - 2 * M) * (nx - 2 * M)
            worst = max(worst, (err / bound).max())
        print('%d x %d M %d: worst error / bound %.3g' % (ny, nx, M, worst))
        assert emu_aff(emu, a, a_off, w, w_off, ny, nx, M)[0].tobytes() == S.tobytes()
        assert emu_aff(emu, a, a_off[::-1], w, w_off[::-1], ny, nx, M)[0][::-1].tobytes() == S.tobytes()
        assert emu_aff(emu, a, a_off[3:4], w, w_off[3:4], ny, nx, M)[0][0].tobytes() == S[3].tobytes()


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation as a program of its own under -fsanitize=address,undefined, run directly: the images, the destination and the
    outputs are heap blocks of exactly their byte counts, the staged footprints exactly the kernel's LDS array; both paths."""
    exe = str(tmp_path / 'warp_emu_san')
    subprocess.check_call(['g++', '-DWARP_EMU_MAIN', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 40 16', r.stdout


# ---- the twin of the whole method against the truth ----------------------------------------------------------------------------------

@pytest.mark.parametrize('model', ['rigid', 'similarity', 'affine'])
def test_twin_finds_the_analytic_transform(model):
    """96 x 128 (two levels), two views blurred (1.5, 2.5) and (2.5, 1.5) px, peak 200 photons over 5, 5 passes, no initial
    translation; truths: rigid 3 degrees, similarity -2 degrees x 1.02, affine 3 degrees x 0.98; three seeds.  Measured worst corner
    displacement errors of the twin: 0.111, 0.163, 0.140 px (the different blurs of the views alone leave 0.05 - 0.1 px without any
    noise).  Asserted at twice the measured values, which stays below 0.5 px; the untreated corner moves 3.2 - 4.4 px.  With no true
    transform every model returns the identity within the same bound."""
    from rescan_line_sted_amd import registration as reg
    ny, nx = 96, 128
    T = ar.TRUTHS[model]
    eye = reg.identity_transforms(1)[0]
    assert 2.0 * TWIN_ERROR[model] <= 0.5 and reg.corner_displacement(eye, T, (ny, nx)) > 3.0
    worst = none = 0.0
    for seed in ar.SEEDS:
        a, b = ar.view_pair(seed, ny, nx, T)
        est, info = ar.estimate(b, a, model)
        assert not info['flat'][0] and info['levels'] == 2 and 0.8 < info['gain'][0] < 1.2
        worst = max(worst, float(reg.corner_displacement(est[0], T, (ny, nx))))
        a, b = ar.view_pair(seed, ny, nx, None)
        none = max(none, float(reg.corner_displacement(ar.estimate(b, a, model)[0][0], eye, (ny, nx))))
    print('%s: worst error %.4f px, with no transform %.4f px' % (model, worst, none))
    assert worst <= 2.0 * TWIN_ERROR[model] and none <= 2.0 * TWIN_ERROR[model]


def test_transform_helpers():
    from rescan_line_sted_amd import line_sted_tools, registration as reg
    for name in ('warp_images', 'estimate_transforms', 'transform_matrix_offset', 'compose_transforms', 'invert_transform'):
        assert getattr(line_sted_tools, name) is getattr(reg, name)
    T, S = ar.rotation(3.0, 1.02, (0.5, -1.5)), reg.shift_transforms([2.0, -3.0])
    both = reg.compose_transforms(S, T)                                     # the frame's shift, then the view's transform
    assert np.array_equal(both[:, :2], T[:, :2]) and np.allclose(both[:, 2], T[:, 2] + [2.0, -3.0], rtol=0, atol=1e-15)
    assert np.allclose(reg.compose_transforms(T, reg.invert_transform(T)), reg.identity_transforms(1)[0], rtol=0, atol=1e-15)
    # as maps of pixels: T(x) = c + L (x - c) + t is what transform_matrix_offset hands to the warp
    shape, x = (40, 56), np.array([7.0, 11.0])
    c = np.array([19.5, 27.5])
    xf = reg.transform_matrix_offset(T, shape)
    assert np.allclose(xf[:4].reshape(2, 2) @ x + xf[4:], c + T[:, :2] @ (x - c) + T[:, 2], rtol=0, atol=1e-12)
    # warp(warp(B, S), T) = warp(B, compose_transforms(S, T)) up to the interpolation, on a smooth scene
    p = rr.blobs(3, 40, 56)
    B = rr.scene(p)
    twice = ar.scipy_warp(ar.scipy_warp(B, reg.transform_matrix_offset(S, shape), shape), xf, shape)
    once = ar.scipy_warp(B, reg.transform_matrix_offset(both, shape), shape)
    assert np.abs(twice - once)[8:-8, 8:-8].max() < 2e-3 * B.max()
    assert reg.corner_displacement(T, T, shape) == 0.0 and abs(reg.corner_displacement(S, reg.identity_transforms(1)[0], shape) - np.hypot(2, 3)) < 1e-12
    # a step of pure gain and offset: no geometry
    a = rr.scene(p)
    s = reg.solve_transform(ar.affine_sums(2.0 * a + 3.0, a, 4, exact=False)[0], 'affine')
    assert not s['flat'] and abs(s['gain'] - 2.0) < 1e-9 and abs(s['offset'] - 3.0) < 1e-6 and np.abs(s['dt']).max() < 1e-9 and s['residual'] < 1e-6
    assert reg.solve_transform(ar.affine_sums(a, np.full_like(a, 5.0), 4, exact=False)[0], 'rigid')['flat']          # no gradient at all
    assert reg.solve_transform(ar.affine_sums(a, -a, 4, exact=False)[0], 'rigid')['flat']                            # g <= 0
    assert reg.pyramid_shapes(96, 128, 48) == [(96, 128), (48, 64)] and reg.pyramid_shapes(64, 80, 48) == [(64, 80)]


# ---- the library ---------------------------------------------------------------------------------------------------------------------

def test_the_library_declares_and_checks_its_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert len(_lib.PROTOTYPES['rl_warp_images'][1]) == 14 and len(_lib.PROTOTYPES['rl_affine_sums'][1]) == 12
    header = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_warp_images(' in header and 'int rl_affine_sums(' in header and '#define RL_AFFINE_FIELDS 45' in header
    assert 'int rl_warp_chunk_bytes(' in header
    ctx, a, b = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)          # (never dereferenced)

    def xf(*v):
        return (ctypes.c_double * 12)(*(list(v) + [1.0, 0.0, 0.0, 1.0, 0.0, 0.0] * 2)[:12])
    good = dict(ctx=ctx, src=a, sdt=0, n=2, sy=8, sx=16, xf=xf(), order=3, floor=0.0, dst=b, ddt=1, oy=9, ox=5, stats=None)
    bad = [dict(ctx=None), dict(src=None), dict(xf=None), dict(dst=None), dict(sdt=2), dict(ddt=-1), dict(n=0), dict(sy=0), dict(sx=0), dict(oy=0),
           dict(ox=0), dict(order=2), dict(order=0), dict(floor=float('nan')), dict(xf=xf(1.0, float('nan'))), dict(xf=xf(1.0, 0.0, float('inf'))),
           dict(xf=xf(1.0, 0.0, 0.0, 1.0, 2e9, 0.0)), dict(xf=xf(1e9, 0.0, 0.0, 1.0, 0.0, 0.0)), dict(dst=ctypes.c_void_p(0x100000 + 64)),
           dict(dst=ctypes.c_void_p(0x100000 - 64))]
    for change in bad:
        g = {**good, **change}
        rc = L.rl_warp_images(g['ctx'], g['src'], g['sdt'], g['n'], g['sy'], g['sx'], g['xf'], g['order'], g['floor'], g['dst'], g['ddt'], g['oy'],
                              g['ox'], g['stats'])
        assert rc == -1 and L.rl_last_error() != b'', change
    assert L.rl_warp_chunk_bytes(None, 1) == -1 and L.rl_warp_chunk_bytes(ctx, 0) == -1 and L.rl_warp_path(None, 0) == -1
    off = (ctypes.c_int64 * 2)(0, 100)
    neg = (ctypes.c_int64 * 2)(0, -1)
    out = (ctypes.c_double * 90)()
    good = dict(ctx=ctx, a=a, adt=0, aoff=off, w=b, wdt=1, woff=off, n=2, ny=40, nx=56, M=3, out=out)
    bad = [dict(ctx=None), dict(a=None), dict(w=None), dict(aoff=None), dict(woff=None), dict(out=None), dict(adt=2), dict(wdt=-1), dict(n=0), dict(M=0),
           dict(M=17), dict(ny=13), dict(nx=13), dict(aoff=neg), dict(woff=neg), dict(ny=50000, nx=50000)]
    for change in bad:
        g = {**good, **change}
        rc = L.rl_affine_sums(g['ctx'], g['a'], g['adt'], g['aoff'], g['w'], g['wdt'], g['woff'], g['n'], g['ny'], g['nx'], g['M'], g['out'])
        assert rc == -1 and L.rl_last_error() != b'', change


def test_affine_kernels_do_not_spill(tmp_path):
    """affine_kernels.hip compiled device-only with the flags of _build.py: the twelve kernels (the evaluation x 6, the sums x 4
    dtype pairs with their 45 accumulators in registers, the two totals) have `.private_segment_fixed_size` 0, and no kernel takes
    more than 64 KB of LDS."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'affine_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'affine_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    assert len(priv) == 12 and sum('k_warp_eval<' in k for k in priv) == 6 and sum('k_affine_sums<' in k for k in priv) == 4, priv
    assert sum('k_warp_totals' in k for k in priv) == 1 and sum('k_affine_totals' in k for k in priv) == 1, priv
    assert all(v == 0 for v in priv.values()), priv
    assert all(int(x) <= 65536 for x in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', txt))


# ---- the wrappers on a numpy stand-in -------------------------------------------------------------------------------------------------

def _stand_in():
    from test_register_cpu import _NumpyDevice

    class Device(_NumpyDevice):
        """The stand-in of test_register_cpu.py with the affine steps of the twin's stand-in (scipy's warp, numpy sums)."""
        warp = ar.NumpyDevice.warp
        gather_warp = ar.NumpyDevice.gather_warp
        affine_sums = ar.NumpyDevice.affine_sums
    return Device


def _rotated_stack(F=3, ny=96, nx=128, angle=2.0, constant_view=False):
    """A u16 stack of one scene: view 1 rotated by `angle` degrees and displaced, frame f displaced by f * DRIFT on top."""
    p = ar.blobs(21, ny, nx)
    T1, drift = ar.rotation(angle, 1.0, (0.6, -0.4)), np.array([0.7, 0.45])
    raw = np.zeros((F, 2, ny, nx), dtype=np.uint16)
    truth = np.zeros((F, 2, 2, 3))
    for f in range(F):
        for v in range(2):
            T = ar.rotation(0.0) if v == 0 else T1.copy()
            T[:, 2] += f * drift
            truth[f, v] = T
            raw[f, v] = np.rint(ar.scene(p, T, ar.BLURS[v]) * 4.0 + 100.0)
    if constant_view:
        raw[:, 1] = 300
    return raw, truth


def test_wrapper_composes_frame_shift_and_view_transform_into_one_warp(monkeypatch):
    """F = 3, V = 2, batch = 2 on the stand-in, model='rigid': the view estimate runs once, on frame 0; the frames are registered by
    translation as before; every chunk is ONE warp of batch * V images whose maps are [L_v | t_v + d_fv]; the transforms are close
    to the truth; the measurement handed to the plan is that warp of the ingest."""
    from rescan_line_sted_amd import registration as reg, stack
    import ingest_reference as ir
    Device = _stand_in()
    monkeypatch.setattr(reg, '_Device', Device)
    raw, truth = _rotated_stack()
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    cam = stack.CameraModel(dark=100.0, gain=0.25)
    est, info = reg.deconvolve_stack_registered(raw, psfs, 2, camera=cam, batch=2, dtype='f64', max_shift=6, model='rigid')
    calls = Device.log
    ny, nx = 96, 128
    n_pix = ny * nx
    sums = [c for c in calls if c[0] == 'affine_sums']
    assert len(sums) == 10 and all(c[1] == [0] for c in sums) and [c[3] for c in sums] == [(48, 64)] * 5 + [(96, 128)] * 5 and sums[-1][2] == [0]
    final = [c for c in calls if c[0] == 'warp' and c[1] == 4]
    assert len(final) == 2 and all(c[4] == 3 and c[5] == cam.epsilon for c in final)
    assert not [c for c in calls if c[0] == 'shift' and c[1] == 4]                            # no second interpolation
    T = info['transforms']
    assert T.shape == (3, 2, 2, 3) and np.array_equal(T[:, 0, :, :2], np.broadcast_to(np.eye(2), (3, 2, 2)))
    assert np.array_equal(T[:, 1, :, :2], np.broadcast_to(info['view_transforms'][1, :, :2], (3, 2, 2)))
    frame = [c for c in calls if c[0] == 'sums' and c[3] == 6]                               # the frames' translations, as before
    assert [c[1:3] for c in frame] == [([0, n_pix], [2 * n_pix, 3 * n_pix]), ([0, n_pix], [0, n_pix])]
    d = T[:, :, :, 2] - info['view_transforms'][:, :, 2]
    assert np.all(d[0] == 0) and np.abs(d[1:] - np.array([0.7, 0.45]) * np.arange(1, 3)[:, None, None]).max() < 0.15
    assert np.array_equal(info['shifts'], T[..., 2]) and not info['view_flat'].any() and not info['view_fit']['flat'].any()
    for f in range(3):
        assert reg.corner_displacement(T[f, 1], truth[f, 1], (ny, nx)) < 0.5
    assert np.array_equal(final[0][6], reg.transform_matrix_offset(T[:2].reshape(4, 2, 3), (ny, nx)))
    want_meas, _ = ir.measurement(raw, 2, 'frame-view', (0, 0, ny, nx), 100.0, 0.25)
    its = [c for c in calls if c[0] == 'iterate']
    m = np.maximum(ar.scipy_warp(want_meas[1, 1], reg.transform_matrix_offset(T[1, 1], (ny, nx)), (ny, nx)), cam.epsilon)
    assert np.array_equal(its[0][2][1, 1], m)


def test_wrapper_translation_default_given_transforms_flat_views_and_argument_errors(monkeypatch):
    from rescan_line_sted_amd import registration as reg
    Device = _stand_in()
    monkeypatch.setattr(reg, '_Device', Device)
    raw, truth = _rotated_stack(angle=0.0)
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    # the default is the translation path, call for call: no new step, no new entry
    est0, info0 = reg.deconvolve_stack_registered(raw, psfs, 1, max_shift=6)
    log0 = [c[0] for c in Device.log]
    est1, info1 = reg.deconvolve_stack_registered(raw, psfs, 1, max_shift=6, model='translation', view_transforms=None)
    assert [c[0] for c in Device.log] == log0 and 'warp' not in log0 and 'affine_sums' not in log0 and 'transforms' not in info1
    assert np.array_equal(est0, est1)
    # identities as view_transforms: the shift's own passes, the bits of the translation path without the view estimate
    est2, info2 = reg.deconvolve_stack_registered(raw, psfs, 1, max_shift=6, view_transforms=reg.identity_transforms(2))
    assert 'warp' not in [c[0] for c in Device.log] and 'affine_sums' not in [c[0] for c in Device.log]
    est3, info3 = reg.deconvolve_stack_registered(raw, psfs, 1, max_shift=6, register=('frames',))
    assert np.array_equal(est2, est3) and np.array_equal(info2['shifts'], info3['shifts']) and info2['view_fit'] is None
    # a calibration: the given transform is used, nothing is estimated for the views
    given = np.stack([ar.rotation(0.0), ar.rotation(1.0, 1.0, (0.5, 0.0))])
    est4, info4 = reg.deconvolve_stack_registered(raw, psfs, 1, max_shift=6, view_transforms=given, register=())
    assert not [c for c in Device.log if c[0] in ('affine_sums', 'sums')] and np.array_equal(info4['transforms'], np.broadcast_to(given, (3, 2, 2, 3)))
    assert len([c for c in Device.log if c[0] == 'warp']) == 1
    # a view without variance: flat, the identity
    blank, _ = _rotated_stack(constant_view=True)
    est5, info5 = reg.deconvolve_stack_registered(blank, psfs, 1, max_shift=6, model='affine', register=('views',))
    assert info5['view_flat'][1] and not info5['view_flat'][0] and np.array_equal(info5['view_transforms'], reg.identity_transforms(2))
    for kwargs in (dict(model='projective'), dict(model='rigid', pipeline=True), dict(view_transforms=given, pipeline=True),
                   dict(view_transforms=given[:1]), dict(view_transforms=np.full((2, 2, 3), np.nan))):
        with pytest.raises(ValueError):
            reg.deconvolve_stack_registered(raw, psfs, 1, **kwargs)
    with pytest.raises(ValueError):
        reg.deconvolve_stack_registered(raw, psfs, 1, roi=(0, 0, 15, 15), model='rigid', max_shift=1)   # 15 - 2 * 4 < 8: no interior for the fit
    reg.deconvolve_stack_registered(raw, psfs, 1, roi=(0, 0, 15, 15), max_shift=1)                      # (the translation path serves it)
    a = np.zeros((2, 96, 128), dtype=np.float32)
    for args, kwargs in (((a.astype(np.int16), a[0]), {}), ((a, a[0, :30]), {}), ((a, a[0]), dict(model='x')), ((a, a[0]), dict(passes=0)),
                         ((a, a[0]), dict(margin=0)), ((a, a[0]), dict(min_side=10)), ((a, a[0]), dict(init=np.zeros((3, 2)))),
                         ((a[:, :12], a[0, :12]), {})):
        with pytest.raises(ValueError):
            reg.estimate_transforms(*args, **kwargs)
    eye = reg.identity_transforms(2)
    for args, kwargs in (((a.astype(np.int32), eye), {}), ((a, eye[:1]), {}), ((a, np.zeros((2, 3))), {}), ((a, eye), dict(order=2)),
                         ((a, np.full((2, 2, 3), np.inf)), {}), ((a, eye), dict(output_shape=(0, 5))), ((a, eye), dict(floor=float('nan')))):
        with pytest.raises(ValueError):
            reg.warp_images(*args, **kwargs)


def test_estimate_transforms_on_the_stand_in_is_the_twin(monkeypatch):
    """estimate_transforms through the stand-in equals the twin's estimate (the same host code, the same steps): f64 images, a
    shared reference, an initial shift."""
    from rescan_line_sted_amd import registration as reg
    monkeypatch.setattr(reg, '_Device', _stand_in())
    a, b = ar.view_pair(11, 96, 128, ar.TRUTHS['similarity'])
    a2, b2 = ar.view_pair(12, 96, 128, ar.rotation(1.0, 1.0, (2.0, -1.0)))
    T, info = reg.estimate_transforms(np.stack([b, b2]), a, model='similarity')
    want, winfo = ar.estimate(np.stack([b, b2]), a, 'similarity')
    assert np.array_equal(T, want) and np.array_equal(info['residual'], winfo['residual'])
    one, _ = reg.estimate_transforms(b2, a2, model='rigid', init=[2.0, -1.0])
    assert one.shape == (1, 2, 3) and reg.corner_displacement(one[0], ar.rotation(1.0, 1.0, (2.0, -1.0)), (96, 128)) < 0.3
