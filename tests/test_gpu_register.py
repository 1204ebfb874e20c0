"""Registration on the MI355X (include/rlsted.h rl_register_sums, rl_shift_images; rescan_line_sted_amd/registration.py): the sums
against the long double twin within the derived bound (tests/register_reference.py), bit-identical across calls and independent of
the other pairs; the shift against scipy; estimate_shifts against the twin's estimate; deconvolve_stack_registered against
deconvolve_stack and against deconvolve on the shifted twin measurement; the plan afterwards; and the benefit of registering."""
import numpy as np
import pytest

import ingest_reference as ir
import register_reference as rr
from conftest import max_rel

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
SHIFTS = [(0.0, 0.0), (3.0, -2.0), (-1.5, 0.25), (0.37, -0.81), (40.0, -40.0), (-40.3, 17.7)]
GAIN, DARK, K = 0.125, 100.0, 3
BLUR = (1.5, 0.7)


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


def _pair_data(seed, ny, nx, n_a=3, n_b=5):
    """Images whose values are float32 numbers, so that one twin serves every dtype combination; offsets 5 and 3 elements."""
    rng = np.random.default_rng(seed)
    a = (rng.random(n_a * ny * nx + 5) * 100.0).astype(np.float32)
    b = (rng.random(n_b * ny * nx + 3) * 100.0).astype(np.float32)
    return a, b


_TWINS = {}


def _twin(key, a, ao, b, bo, ny, nx, R, M):
    if key not in _TWINS:
        _TWINS[key] = rr.sums(a[ao:ao + ny * nx].reshape(ny, nx), b[bo:bo + ny * nx].reshape(ny, nx), R, M)
    return _TWINS[key]


# ---- rl_register_sums ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ny,nx,R,M', [(37, 53, 2, 2), (40, 56, 1, 1), (40, 56, 3, 3), (40, 56, 6, 6), (72, 48, 6, 8), (136, 120, 32, 32)])
def test_sums_are_within_the_bound_of_the_twin(dev, ny, nx, R, M):
    """Five pairs over three references and five moving images (shared references, offsets of 5 and 3 elements), f32 / f64 in all
    four combinations: every sum within gamma_N sum |t| of the twin; two calls bit-identical; a pair alone the bits it has among
    five.  136 x 120 at R = 32 is the maximal LDS footprint."""
    n_pix = ny * nx
    a, b = _pair_data(ny + R, ny, nx)
    a_off = [5, n_pix + 5, 5, 2 * n_pix + 5, n_pix + 5]
    b_off = [3 + k * n_pix for k in (4, 0, 2, 1, 3)]
    for ta in ('f32', 'f64'):
        for tb in ('f32', 'f64'):
            ab, bb = _buffer(dev, a, ta), _buffer(dev, b, tb)
            S, A = dev.sums(ab, a_off, bb, b_off, ny, nx, R, M)
            worst = 0.0
            for i in range(5):
                want, ref, bound, ref_bound = _twin((ny, nx, R, M, i), a, a_off[i], b, b_off[i], ny, nx, R, M)
                err = np.abs(S[i].astype(np.longdouble) - want).astype(np.float64)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (ta, tb, i, worst)
                assert np.all(np.abs(A[i].astype(np.longdouble) - ref).astype(np.float64) <= ref_bound)
            print('%d x %d R %d %s/%s: worst error / bound %.3g' % (ny, nx, R, ta, tb, worst))
            S2, A2 = dev.sums(ab, a_off, bb, b_off, ny, nx, R, M)
            assert S2.tobytes() == S.tobytes() and A2.tobytes() == A.tobytes()
            S1, A1 = dev.sums(ab, a_off[3:4], bb, b_off[3:4], ny, nx, R, M)
            assert S1[0].tobytes() == S[3].tobytes() and A1[0].tobytes() == A[3].tobytes()


def test_sums_of_many_tiles(dev):
    """512 x 512, R = 8, four pairs: 31 bands of 16 column blocks, two passes, the second-stage reduction over 31 strips; two of the
    pairs against the twin, all four bit-identical in a second call and alone."""
    ny = nx = 512
    n_pix = ny * nx
    a, b = _pair_data(512, ny, nx, 2, 2)
    a_off, b_off = [5, 5, n_pix + 5, n_pix + 5], [3, n_pix + 3, 3, n_pix + 3]
    ab, bb = _buffer(dev, a, 'f32'), _buffer(dev, b, 'f64')
    S, A = dev.sums(ab, a_off, bb, b_off, ny, nx, 8, 8)
    for i in (0, 3):
        want, ref, bound, ref_bound = rr.sums(a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), b[b_off[i]:b_off[i] + n_pix].reshape(ny, nx), 8, 8)
        err = np.abs(S[i].astype(np.longdouble) - want).astype(np.float64)
        print('512 x 512 R 8 pair %d: worst error / bound %.3g' % (i, (err / bound).max()))
        assert np.all(err <= bound) and np.all(np.abs(A[i].astype(np.longdouble) - ref).astype(np.float64) <= ref_bound)
    S2, A2 = dev.sums(ab, a_off, bb, b_off, ny, nx, 8, 8)
    assert S2.tobytes() == S.tobytes() and A2.tobytes() == A.tobytes()
    for i in (1, 2):
        S1, A1 = dev.sums(ab, a_off[i:i + 1], bb, b_off[i:i + 1], ny, nx, 8, 8)
        assert S1[0].tobytes() == S[i].tobytes() and A1[0].tobytes() == A[i].tobytes()


def test_an_interior_that_is_too_small_is_refused(dev):
    """96 x 80 at R = 32: with the margin the interior needs (from M = 37 on, 80 - 2 M < 8) the call is refused; 136 x 120 runs."""
    from rescan_line_sted_amd._lib import RlstedError
    a, b = _pair_data(1, 136, 120, 1, 1)
    ab, bb = _buffer(dev, a, 'f32'), _buffer(dev, b, 'f32')
    for M in (37, 40):
        with pytest.raises(RlstedError):
            dev.sums(ab, [0], bb, [0], 96, 80, 32, M)
    with pytest.raises(RlstedError):
        dev.sums(ab, [0], bb, [0], 96, 80, 32, 31)
    with pytest.raises(ValueError):
        _reg().estimate_shifts(np.zeros((96, 80), dtype=np.float32), np.zeros((96, 80), dtype=np.float32), max_shift=32, margin=37)
    S, A = dev.sums(ab, [0], bb, [0], 136, 120, 32, 40)
    assert np.all(np.isfinite(S)) and S.shape == (1, 4225, 3)


# ---- rl_shift_images -----------------------------------------------------------------------------------------------------------------

def _device_shift(dev, src, shifts, order, floor, dst_dtype, guard=8):
    """Through a destination with `guard` sentinel elements on either side, which must stay intact."""
    n, ny, nx = src.shape
    sb = _buffer(dev, src, 'f32' if src.dtype == np.float32 else 'f64')
    whole = np.full(src.size + 2 * guard, 7, dtype=NP[dst_dtype])
    db = _buffer(dev, whole, dst_dtype)
    stats = dev.shift(sb, 0, n, ny, nx, shifts, order, floor, db, guard)
    back = dev.download(db, whole.size)
    assert np.all(back[:guard] == 7) and np.all(back[guard + src.size:] == 7), 'written outside the destination'
    return back[guard:guard + src.size].reshape(src.shape), stats


@pytest.mark.parametrize('order', [1, 3])
def test_shift_is_scipy(dev, order):
    """37 x 53 and 70 x 130; shifts 0, integer, negative, fractional and beyond the image (|s| = 40 on 37 rows); f64 -> f64 within
    1e-12 max|image|; an f32 destination at most 1 ulp from the rounded twin; the sentinels intact; the sum within its bound."""
    rng = np.random.default_rng(order)
    for ny, nx in ((37, 53), (70, 130)):
        for dt in (np.float32, np.float64):
            src = (rng.random((len(SHIFTS), ny, nx)) * 1000.0).astype(dt)
            want = np.stack([rr.shift(src[k], SHIFTS[k], order) for k in range(len(SHIFTS))])
            got, stats = _device_shift(dev, src, SHIFTS, order, None, 'f64')
            err = np.abs(got - want).max() / np.abs(src).max()
            print('order %d %s %d x %d: max error %.3g max|image|' % (order, np.dtype(dt).name, ny, nx, err))
            assert err <= 1e-12 and np.all(stats[:, 0] == 0)
            for k in range(len(SHIFTS)):
                assert abs(stats[k, 1] - want[k].sum()) <= rr.gamma(ny * nx) * np.abs(want[k]).sum() + 1e-12 * np.abs(src).max() * ny * nx
            got32, _ = _device_shift(dev, src, SHIFTS, order, None, 'f32')
            w32 = want.astype(np.float32)
            assert np.all(np.abs(got32 - w32.astype(np.float64)) <= np.spacing(np.abs(w32)))


def test_order_one_with_integer_shifts_is_bit_exact(dev):
    rng = np.random.default_rng(5)
    for dt, name in ((np.float32, 'f32'), (np.float64, 'f64')):
        src = ((rng.random((3, 37, 53)) - 0.5) * 1e6).astype(dt)
        shifts = [(0.0, 0.0), (3.0, -2.0), (-40.0, 75.0)]
        got, _ = _device_shift(dev, src, shifts, 1, None, name)
        for k, (sy, sx) in enumerate(shifts):
            iy = np.pad(np.arange(37), 120, mode='reflect')[120 + int(sy):120 + int(sy) + 37]
            ix = np.pad(np.arange(53), 120, mode='reflect')[120 + int(sx):120 + int(sx) + 53]
            assert got[k].astype(dt).tobytes() == src[k][iy][:, ix].tobytes()
    out = _reg().shift_images(src, shifts, order=1)
    assert out.dtype == src.dtype and out.tobytes() == got.astype(dt).tobytes()


def test_floor_and_raised_count_are_exact(dev):
    """A bright square on zero, where the twin itself rings below zero at order 3 (checked on the CPU, tests/test_register_cpu.py):
    every pixel the twin puts below the floor is the floor, the count is that of the pixels at the floor."""
    src = np.zeros((1, 40, 56))
    src[0, 12:28, 20:40] = 1000.0
    want = rr.shift(src[0], (0.4, -0.3), 3)
    assert want.min() < -10.0
    floor = 1e-9
    got, stats = _device_shift(dev, src, [(0.4, -0.3)], 3, floor, 'f64')
    sure = np.abs(want - floor) > 1e-9
    assert np.all(got >= floor) and np.all(got[0][sure & (want < floor)] == floor)
    assert np.allclose(got[0][want > floor], want[want > floor], rtol=0, atol=1e-9)
    low, high = int((want < floor - 1e-9).sum()), int((want < floor + 1e-9).sum())
    assert low <= stats[0, 0] <= high and low > 50 and stats[0, 0] == (got == floor).sum()
    assert abs(stats[0, 1] - got.sum()) <= rr.gamma(got.size) * np.abs(got).sum()


# ---- estimate_shifts -----------------------------------------------------------------------------------------------------------------

def test_estimates_are_the_twins(dev):
    """Every committed scene (48 x 64 and 96 x 80, six displacements, same and different blur; their NCC margins exceed 1e-6, checked
    on the CPU): the integer peak is the twin's, the sub-pixel value within 1e-6 px, refine = 1."""
    worst = 0.0
    for seed, ny, nx in rr.SCENES:
        p = rr.blobs(seed, ny, nx)
        ref = rr.scene(p)
        imgs = np.stack([rr.scene(p, d, blur) for d in rr.DISPLACEMENTS for blur in ((0.0, 0.0), BLUR)])
        s, info = _reg().estimate_shifts(imgs, ref, max_shift=6, refine=1, surfaces=True)
        s0, _ = _reg().estimate_shifts(imgs, ref, max_shift=6, refine=0)
        for k in range(len(imgs)):
            w, wi = rr.estimate(imgs[k], ref, 6, 1)
            iy, ix = divmod(int(np.argmax(info['surfaces'][k])), 13)
            assert (iy - 6, ix - 6) == wi['integer'] and tuple(np.round(s0[k] - rr.estimate(imgs[k], ref, 6, 0)[0], 6)) == (0.0, 0.0)
            worst = max(worst, float(np.abs(s[k] - w).max()))
            assert not info['at_limit'][k] and not info['flat'][k] and abs(info['ncc'][k] - wi['ncc']) < 1e-9
    print('device estimate against the twin: worst %.3g px' % worst)
    assert worst <= 1e-6


# ---- deconvolve_stack_registered -----------------------------------------------------------------------------------------------------

def _stack(F, V, seed, sensor=(46, 61), roi=(3, 5, 40, 48)):
    """uint16 frames of a drifting blob scene inside a larger sensor frame, with noise."""
    rng = np.random.default_rng(seed)
    y0, x0, ny, nx = roi
    p = rr.blobs(seed, ny, nx, 10)
    raw = rng.integers(95, 106, (F, V) + sensor).astype(np.uint16)
    for f in range(F):
        for v in range(V):
            img = rr.scene(p, (0.4 * f + 0.8 * v, -0.3 * f + 0.5 * v)) * 8.0 + 100.0
            raw[f, v, y0:y0 + ny, x0:x0 + nx] = rng.poisson(img).astype(np.uint16)
    return raw, roi


def _psfs(V):
    return [rr.gaussian_psf(0.8 + 0.5 * v, 1.9 - 0.5 * v, 7) for v in range(V)]


def _camera():
    from rescan_line_sted_amd.stack import CameraModel
    return CameraModel(dark=DARK, gain=GAIN)


@pytest.mark.parametrize('dtype,V', [('f64', 1), ('f64', 2), ('f32', 2), ('f32', 1)])
def test_zero_shifts_at_order_one_are_deconvolve_stack(dtype, V):
    """u16 raw, a window of the sensor, F = 5, batch = 2 (it does not divide F), both orders: with all-zero given shifts and
    interp = 1 the registered path is deconvolve_stack bit for bit; single-view f32 plans (frames run as pairs, partners differ)
    within the 1e-5 normwise contract."""
    from rescan_line_sted_amd.stack import deconvolve_stack
    raw, roi = _stack(5, V, 20 + V)
    psfs = _psfs(V)
    want, winfo = deconvolve_stack(raw, psfs, K, camera=_camera(), roi=roi, dtype=dtype, out_dtype='f64', batch=2)
    for order in ('frame-view', 'view-frame'):
        r = raw if order == 'frame-view' else np.ascontiguousarray(raw.transpose(1, 0, 2, 3))
        est, info = _reg().deconvolve_stack_registered(r, psfs, K, camera=_camera(), order=order, roi=roi, dtype=dtype, batch=2,
                                                      shifts=np.zeros((5, V, 2)), interp=1)
        assert est.shape == (5, 40, 48) and info['chunks'] == 3 and not info['raised'].any() and not info['shifts'].any()
        if (dtype, V) == ('f32', 1):
            err = max(max_rel(est[f], want[f]) for f in range(5))
            print('f32 single view: normwise %.3e' % err)
            assert err <= 1e-5
        else:
            assert est.tobytes() == want.tobytes()
        assert info['level'].tobytes() == winfo['level'].tobytes() and np.array_equal(info['clipped'], winfo['clipped'])


@pytest.mark.parametrize('dtype,V', [('f64', 1), ('f64', 2), ('f32', 2)])
def test_given_shifts_are_deconvolve_on_the_shifted_twin_measurement(dtype, V):
    """Non-zero given shifts, order 3: bit for bit `deconvolve` on (the twin's ingest -> shift_images on the device)."""
    from rescan_line_sted_amd.line_sted_tools import deconvolve
    raw, roi = _stack(5, V, 30 + V)
    psfs = _psfs(V)
    rng = np.random.default_rng(3)
    shifts = rng.uniform(-3.0, 3.0, (5, V, 2))
    est, info = _reg().deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype=dtype, batch=2, shifts=shifts)
    meas, stats = ir.measurement(raw, V, 'frame-view', roi, DARK, GAIN, dtype=NP[dtype])
    moved = _reg().shift_images(meas.reshape(-1, 40, 48), shifts.reshape(-1, 2), order=3, floor=1e-9).reshape(5, V, 40, 48)
    want = deconvolve(moved, psfs, K, dtype=dtype)
    assert est.tobytes() == want.tobytes() and np.array_equal(info['shifts'], shifts)
    assert np.array_equal(info['raised'], (moved == NP[dtype](1e-9)).sum(axis=(2, 3)))


def test_estimated_registration_follows_the_drift_and_leaves_the_plan_fresh(monkeypatch):
    """Estimation on: the shifts follow the drift built into the frames (0.4, -0.3 per frame, 0.8, 0.5 per view) within the noise;
    the plan of the run, used afterwards in the ordinary way, gives the bits of a fresh plan."""
    reg = _reg()
    from rescan_line_sted_amd import _lib as L
    kept = []

    class Keep(reg._Device):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            kept.append(self)
    monkeypatch.setattr(reg, '_Device', Keep)
    raw, roi = _stack(5, 2, 44)
    psfs = _psfs(2)
    est, info = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=4)
    truth = np.array([[(0.4 * f + 0.8 * v, -0.3 * f + 0.5 * v) for v in range(2)] for f in range(5)])
    print('worst shift error %.3f px' % np.abs(info['shifts'] - truth).max())
    assert np.abs(info['shifts'] - truth).max() < 0.25 and not info['at_limit'].any() and not info['flat'].any()
    assert np.all(np.isfinite(est)) and info['unresolved'] == 0
    plan = kept[0].plan
    meas, _ = ir.measurement(raw, 2, 'frame-view', roi, DARK, GAIN)
    fresh = L.DeconvPlan(psfs, 2, 40, 48, dtype='f32')
    for q in (plan, fresh):
        q.set_measurement(meas[3:5])
        q.iterate(K)
    assert plan.estimate().tobytes() == fresh.estimate().tobytes()


def test_registering_a_displaced_view_pays():
    """64 x 64, V = 2, noise-free, view 1 displaced by (2.3, -3.7), K = 20: the oracle on the twin's registration improves the error
    by a factor of 25.4 (tests/test_register_cpu.py); the device must reach half of that."""
    reg = _reg()
    from rescan_line_sted_amd.stack import deconvolve_stack
    psfs, obj, meas = rr.benefit_case()
    raw = meas[None].astype(np.float32)
    est, info = reg.deconvolve_stack_registered(raw, psfs, 20, dtype='f64', register=('views',))
    plain, _ = deconvolve_stack(raw, psfs, 20, dtype='f64', out_dtype='f64')
    e1, e0 = rr.relative_error(est[0], obj), rr.relative_error(plain[0], obj)
    print('unregistered %.4f registered %.4f factor %.1f shift %s' % (e0, e1, e0 / e1, info['shifts'][0, 1]))
    assert np.abs(info['shifts'][0, 1] - rr.BENEFIT_DISPLACEMENT).max() < 0.15 and e0 / e1 >= 0.5 * rr.BENEFIT_FACTOR
