"""Affine registration on the MI355X (include/rlsted.h rl_warp_images, rl_affine_sums; rescan_line_sted_amd/registration.py): the
warp against the long double twin within the derived bound (tests/affine_reference.py), both paths and any chunking with the same
bits, the statistics bit for bit; the sums within their bound, bit-identical across calls and independent of the other pairs;
estimate_transforms against the twin of the whole method; deconvolve_stack_registered(model='rigid') against deconvolve on the warped
twin measurement, against the translation path, and the plan afterwards."""
import numpy as np
import pytest

import affine_reference as ar
import ingest_reference as ir
import register_reference as rr

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
ROUND = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
GAIN, DARK, K = 0.25, 100.0, 10
# the corner displacement between the device's and the twin's transforms on the committed scenes (96 x 128, seed 11), measured on
# the MI355X per model; asserted at ten times these, and the assertion itself stays below 1e-6 px: both sides run the same steps,
# so anything looser would hide a wrong solve or update order
DEVICE_TWIN = {'rigid': 4.6e-15, 'similarity': 2.3e-15, 'affine': 5.5e-15}


def _reg():
    from rescan_line_sted_amd import registration
    return registration


@pytest.fixture()
def dev():
    d = _reg()._Device(device=0)
    yield d
    d.close()


def _buffer(dev, array, dtype):
    buf = dev.alloc(array.size, dtype)
    dev.upload(buf, np.ascontiguousarray(array, dtype=NP[dtype]))
    return buf


def _device_warp(dev, src, xf, order, floor, sdt, ddt, out_shape, path=0):
    """(dst (n, oy, ox) float64 holding the stored values, stats) of rl_warp_images, guard values around the destination checked."""
    from rescan_line_sted_amd._lib import check, lib
    n, sy, sx = src.shape
    oy, ox = out_shape
    sb = _buffer(dev, src, sdt)
    whole = dev.alloc(n * oy * ox + 16, ddt)
    dev.upload(whole, np.full(n * oy * ox + 16, 7, dtype=NP[ddt]))
    check(lib.rl_warp_path(dev.ctx.handle, path))
    try:
        stats = dev.warp(sb, 0, n, sy, sx, np.asarray(xf, dtype=np.float64).reshape(n, 6), order, floor, whole, 8, oy, ox)
    finally:
        check(lib.rl_warp_path(dev.ctx.handle, 0))
    back = dev.download(whole, n * oy * ox + 16)
    assert np.all(back[:8] == 7) and np.all(back[8 + n * oy * ox:] == 7)
    return back[8:8 + n * oy * ox].reshape(n, oy, ox), stats


# ---- rl_warp_images ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('order', [1, 3])
@pytest.mark.parametrize('shapes', ar.WARP_SHAPES, ids=lambda s: '%dx%d' % s[0])
def test_warp_is_within_the_bound_of_the_twin(dev, shapes, order):
    """The shapes and transforms of the CPU test (tests/test_affine_cpu.py): f32 and f64 sources, f64 and f32 destinations, within
    the twin's bound plus the destination's rounding; guard values intact; the stored sum bit for bit in the fixed order; the direct
    path forced on the same inputs gives the same bits."""
    (sy, sx), out_shape = shapes
    rng = np.random.default_rng(sy * 1000 + sx + order)
    cases = ar.warp_cases((sy, sx))
    names = list(cases)
    xf = np.stack([cases[k] for k in names])
    one = (rng.random((sy, sx)) * 1000.0).astype(np.float32)                 # (float32 numbers: one twin serves both source types)
    src = np.ascontiguousarray(np.broadcast_to(one, (len(names), sy, sx)))
    coef = ar.coefficients(one) if order == 3 else None
    twins = [ar.warp(one, xf[k], out_shape, order, coef) for k in range(len(names))]
    worst = 0.0
    for sdt in ('f32', 'f64'):
        for ddt in ('f64', 'f32'):
            got, stats = _device_warp(dev, src, xf, order, None, sdt, ddt, out_shape)
            direct, dstats = _device_warp(dev, src, xf, order, None, sdt, ddt, out_shape, path=1)
            assert direct.tobytes() == got.tobytes() and dstats.tobytes() == stats.tobytes()
            assert np.all(stats[:, 0] == 0)
            for k, name in enumerate(names):
                want, bound = twins[k]
                tol = bound + ROUND[ddt] * np.abs(want).astype(np.float64) * (1 + 2.0 ** -20)
                err = np.abs(got[k].astype(np.longdouble) - want).astype(np.float64)
                assert np.all(err <= tol), (name, sdt, ddt, (err / tol).max())
                assert stats[k, 1] == ar.stored_sum(got[k]), name
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print('%d x %d order %d: worst error / bound %.3g' % (sy, sx, order, worst))


def test_warp_of_a_large_image_rotated_by_one_degree(dev):
    """512 x 512, f32 -> f32, order 3, rotated by 1 degree about the centre (the corners move by 4.5 px), and order 1: against the
    twin within the bound, both paths the same bits."""
    rng = np.random.default_rng(512)
    one = (rng.random((512, 512)) * 1000.0).astype(np.float32)
    xf = ar.centred(ar.rotation(1.0)[:, :2], (0.3, -0.2), (512, 512))
    for order in (3, 1):
        want, bound = ar.warp(one, xf, (512, 512), order)
        got, stats = _device_warp(dev, one[None], xf, order, None, 'f32', 'f32', (512, 512))
        direct, dstats = _device_warp(dev, one[None], xf, order, None, 'f32', 'f32', (512, 512), path=1)
        assert direct.tobytes() == got.tobytes() and dstats.tobytes() == stats.tobytes()
        tol = bound + ROUND['f32'] * np.abs(want).astype(np.float64) * (1 + 2.0 ** -20)
        err = np.abs(got[0].astype(np.longdouble) - want).astype(np.float64)
        print('512 x 512 order %d: worst error / bound %.3g' % (order, (err / tol).max()))
        assert np.all(err <= tol) and stats[0, 1] == ar.stored_sum(got[0])


def test_warp_in_two_chunks_is_one_chunk_bit_for_bit(dev):
    """Five images of 37 x 53 into 41 x 29 under a cap of two images' intermediates (three chunks), and of one image's: the bits of
    the default cap, statistics included; order 1 under a cap of one byte."""
    from rescan_line_sted_amd._lib import check, lib
    rng = np.random.default_rng(7)
    src = (rng.random((5, 37, 53)) * 1000.0 - 100.0).astype(np.float32)
    cases = ar.warp_cases((37, 53))
    xf = np.stack([cases[k] for k in ('rot30', 'shear', 'translation', 'far', 'shrink3')])
    for order in (3, 1):
        want, wstats = _device_warp(dev, src, xf, order, 50.0, 'f32', 'f64', (41, 29))
        assert wstats[:, 0].min() > 0
        for cap in (2 * 16 * 37 * 53 + 4096, 16 * 37 * 53, 1):
            check(lib.rl_warp_chunk_bytes(dev.ctx.handle, cap))
            try:
                got, stats = _device_warp(dev, src, xf, order, 50.0, 'f32', 'f64', (41, 29))
            finally:
                check(lib.rl_warp_chunk_bytes(dev.ctx.handle, 512 << 20))
            assert got.tobytes() == want.tobytes() and stats.tobytes() == wstats.tobytes()


def test_order_one_integer_translation_and_binning_are_exact(dev):
    reg = _reg()
    rng = np.random.default_rng(5)
    src = ((rng.random((2, 37, 53)) - 0.5) * 1e6).astype(np.float32)
    got, _ = _device_warp(dev, src, [[1.0, 0.0, 0.0, 1.0, 3.0, -2.0], [1.0, 0.0, 0.0, 1.0, -40.0, 75.0]], 1, None, 'f32', 'f32', (37, 53))
    for k, (sy, sx) in enumerate([(3, -2), (-40, 75)]):
        iy = np.pad(np.arange(37), 120, mode='reflect')[120 + sy:120 + sy + 37]
        ix = np.pad(np.arange(53), 120, mode='reflect')[120 + sx:120 + sx + 53]
        assert np.array_equal(got[k], src[k][iy][:, ix])
    binned, _ = _device_warp(dev, src, np.tile(reg.BIN2, (2, 1)), 1, None, 'f32', 'f64', (18, 26))
    assert binned[0].tobytes() == ar.bin2(src[0]).tobytes() and binned[1].tobytes() == ar.bin2(src[1]).tobytes()
    out = reg.warp_images(src, reg.shift_transforms([[3.0, -2.0], [0.0, 0.0]]), order=1)
    assert out.dtype == np.float32 and np.array_equal(out[1], src[1])


# ---- rl_affine_sums ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ny,nx,M', [(10, 10, 1), (37, 53, 4), (512, 512, 8)])
def test_affine_sums_are_within_the_bound_of_the_twin(dev, ny, nx, M):
    """Five pairs over three references and five warped images (shared references, offsets of 5 and 3 elements), f32 / f64 in all
    four combinations (512 x 512: f32 / f64 alone; 31 runs per pair): each of the 45 sums within gamma_n sum |term| of the twin; two
    calls bit-identical; a pair alone the bits it has among five."""
    n_pix = ny * nx
    rng = np.random.default_rng(ny + M)
    a = (rng.random(3 * n_pix + 5) * 100.0).astype(np.float32)
    w = (rng.random(5 * n_pix + 3) * 100.0).astype(np.float32)
    a_off = [5, n_pix + 5, 5, 2 * n_pix + 5, n_pix + 5]
    w_off = [3 + k * n_pix for k in (4, 0, 2, 1, 3)]
    twins = [ar.affine_sums(a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), w[w_off[i]:w_off[i] + n_pix].reshape(ny, nx), M) for i in range(5)]
    for ta, tw in ((('f32', 'f64'),) if ny == 512 else (('f32', 'f32'), ('f32', 'f64'), ('f64', 'f32'), ('f64', 'f64'))):
        ab, wb = _buffer(dev, a, ta), _buffer(dev, w, tw)
        S = dev.affine_sums(ab, a_off, wb, w_off, ny, nx, M)
        worst = 0.0
        for i in range(5):
            want, bound = twins[i]
            err = np.abs(S[i].astype(np.longdouble) - want).astype(np.float64)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (ta, tw, i, worst)
            assert S[i, 35] == (ny - 2 * M) * (nx - 2 * M)
        print('%d x %d M %d %s/%s: worst error / bound %.3g' % (ny, nx, M, ta, tw, worst))
        assert dev.affine_sums(ab, a_off, wb, w_off, ny, nx, M).tobytes() == S.tobytes()
        assert dev.affine_sums(ab, a_off[3:4], wb, w_off[3:4], ny, nx, M)[0].tobytes() == S[3].tobytes()


# ---- estimate_transforms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('model', ['rigid', 'similarity', 'affine'])
def test_estimated_transforms_are_the_twins(model):
    """96 x 128, the committed scene of seed 11 with its truth, f64: the device's transform against the twin of the whole method
    (the same host code on scipy's warp and numpy's sums) in corner displacement; measured, asserted at ten times the measurement,
    which stays below 1e-6 px.  The fit's gain, offset and residual agree to 1e-9."""
    reg = _reg()
    assert 10.0 * DEVICE_TWIN[model] < 1e-6
    a, b = ar.view_pair(11, 96, 128, ar.TRUTHS[model])
    T, info = reg.estimate_transforms(b, a, model=model)
    want, winfo = ar.estimate(b, a, model)
    d = float(reg.corner_displacement(T[0], want[0], (96, 128)))
    print('%s: device against the twin %.3g px, against the truth %.4f px' % (model, d, reg.corner_displacement(T[0], ar.TRUTHS[model], (96, 128))))
    assert d <= 10.0 * DEVICE_TWIN[model]
    assert not info['flat'][0] and info['levels'] == 2
    for k in ('gain', 'offset', 'residual'):
        assert abs(info[k][0] - winfo[k][0]) < 1e-9 * max(1.0, abs(winfo[k][0]))
    T32, _ = reg.estimate_transforms(b.astype(np.float32), a.astype(np.float32), model=model)      # (counts are float32 numbers:
    assert reg.corner_displacement(T32[0], T[0], (96, 128)) <= 1e-9                                # the same values in another type)


# ---- deconvolve_stack_registered -----------------------------------------------------------------------------------------------------

VIEW_TRUTH = ar.rotation(3.0)


def _psfs():
    return [rr.gaussian_psf(0.9, 2.2), rr.gaussian_psf(2.2, 0.9)]


def _stack(T, F=4, seed=31, ny=96, nx=128):
    """(raw uint16 (F, 2, ny, nx), object): view 0 the object through a PSF narrow along y, view 1 the object transformed by T
    (analytically) through one narrow along x; Poisson noise on peak 400 counts over 100 of dark level, a drift of 0.3 px per frame."""
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(seed)
    p = ar.blobs(seed, ny, nx)
    psfs = _psfs()
    obj = ar.scene(p)
    raw = np.zeros((F, 2, ny, nx), dtype=np.uint16)
    for f in range(F):
        for v in range(2):
            Tv = ar.rotation(0.0) if v == 0 else np.array(T, dtype=np.float64)
            Tv[:, 2] += (0.3 * f, -0.2 * f)
            img = fftconvolve(ar.scene(p, Tv), psfs[v][0], mode='same')
            raw[f, v] = rng.poisson(np.maximum(img, 0.0) * (400.0 / obj.max()) / GAIN).astype(np.uint16) + 100
    return raw, obj * (400.0 / obj.max())


def _camera():
    from rescan_line_sted_amd.stack import CameraModel
    return CameraModel(dark=DARK, gain=GAIN)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_rigid_registration_is_deconvolve_on_the_warped_twin_measurement(dtype):
    """96 x 128, 2 views, 4 frames, K = 10, uint16, view 1 rotated by 3 degrees, batch 3: identities as view_transforms are the bits
    of the translation path with zero shifts; with model='rigid' the estimate is bit for bit `deconvolve` on (the twin's ingest ->
    warp_images on the device by info['transforms']), in float64 and in the multi-view f32 plan."""
    reg = _reg()
    from rescan_line_sted_amd.line_sted_tools import deconvolve
    raw, _ = _stack(VIEW_TRUTH)
    psfs = _psfs()
    plain, _ = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), dtype=dtype, batch=3, shifts=np.zeros((4, 2, 2)))
    same, sinfo = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), dtype=dtype, batch=3, register=(),
                                                  view_transforms=reg.identity_transforms(2))
    assert same.tobytes() == plain.tobytes() and np.array_equal(sinfo['transforms'], reg.identity_transforms(8).reshape(4, 2, 2, 3))
    est, info = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), dtype=dtype, batch=3, max_shift=4, model='rigid')
    T = info['transforms']
    assert not info['view_flat'].any() and reg.corner_displacement(info['view_transforms'][1], VIEW_TRUTH, (96, 128)) < 0.5
    meas, _ = ir.measurement(raw, 2, 'frame-view', (0, 0, 96, 128), DARK, GAIN, dtype=NP[dtype])
    moved = reg.warp_images(meas.reshape(-1, 96, 128), T.reshape(-1, 2, 3), order=3, floor=1e-9).reshape(4, 2, 96, 128)
    want = deconvolve(moved, psfs, K, dtype=dtype)
    assert est.tobytes() == want.tobytes()
    at_floor = (moved == NP[dtype](1e-9)).sum(axis=(2, 3))           # raised, or -- in float32 -- an empty pixel's 1e-9 rounded back onto it
    assert np.array_equal(info['raised'], at_floor) if dtype == 'f64' else (np.all(info['raised'] <= at_floor) and info['raised'].min() > 50)
    with pytest.raises(ValueError):
        reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), model='rigid', pipeline=True)


def test_registering_a_rotated_view_pays_and_leaves_the_plan_fresh(monkeypatch):
    """The error to the true object inside a border of 8 pixels, f64, K = 10: with model='rigid' below the translation-only error and
    within 1.5 times the error of the same stack without any rotation (what is left is the fit's 0.1 - 0.2 px at the corners against
    PSFs of 0.9 px and the spline's smoothing of the noise); measured 0.0498, 0.2584 and 0.0489, printed.  The plan of the run, used afterwards in
    the ordinary way, gives the bits of a fresh plan."""
    reg = _reg()
    from rescan_line_sted_amd import _lib as L
    kept = []

    class Keep(reg._Device):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            kept.append(self)
    monkeypatch.setattr(reg, '_Device', Keep)
    raw, obj = _stack(VIEW_TRUTH)
    still, _ = _stack(ar.rotation(0.0))
    psfs = _psfs()
    rigid, info = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), dtype='f64', max_shift=4, model='rigid')
    plan = kept[0].plan
    shifted, _ = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), dtype='f64', max_shift=4)
    straight, _ = reg.deconvolve_stack_registered(still, psfs, K, camera=_camera(), dtype='f64', max_shift=4)
    e_rigid, e_shift, e_still = (float(np.mean([rr.relative_error(e[f], obj) for f in range(4)])) for e in (rigid, shifted, straight))
    print('relative error to the object: rigid %.4f, translation only %.4f, no rotation in the data %.4f' % (e_rigid, e_shift, e_still))
    assert e_rigid < e_shift and e_rigid <= 1.5 * e_still
    meas, _ = ir.measurement(raw, 2, 'frame-view', (0, 0, 96, 128), DARK, GAIN)
    fresh = L.DeconvPlan(psfs, 4, 96, 128, dtype='f64')
    for q in (plan, fresh):
        q.set_measurement(meas)
        q.iterate(3)
    assert plan.estimate().tobytes() == fresh.estimate().tobytes()
