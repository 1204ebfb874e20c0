"""The coarse registration stage on the MI355X (include/rlsted.h rl_register_xcorr; rescan_line_sted_amd/registration.py
coarse_shifts, estimate_shifts(coarse=), deconvolve_stack_registered(coarse=)): the surface against the float64 twin within the
derived bound (tests/xcorr_reference.py), the integer peak the twin's, means and energies bit for bit, sentinels around the outputs,
bit-identical across calls, independent of the other pairs and of the chunking; the two-stage estimate against the twin of the whole
method and against the truth, where the window alone fails; the registered stack with a view displaced by more than 32 pixels."""
import ctypes

import numpy as np
import pytest

import ingest_reference as ir
import register_reference as rr
import xcorr_reference as xr

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
GAIN, DARK, K = 0.125, 100.0, 3


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


def _xcorr(dev, ab, a_off, bb, b_off, ny, nx, R, guard=8):
    """rl_register_xcorr through outputs with `guard` sentinel values on either side, which must stay intact."""
    from rescan_line_sted_amd import _lib
    n, W = len(a_off), 2 * R + 1
    wp, ws = np.full(n * 7 + 2 * guard, 7.0), np.full(n * W * W + 2 * guard, 7.0, dtype=np.float32)
    ao, bo = np.ascontiguousarray(a_off, dtype=np.int64), np.ascontiguousarray(b_off, dtype=np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    _lib.check(_lib.lib.rl_register_xcorr(dev.ctx.handle, ab.ptr, _lib.DTYPES[ab.dtype], ao.ctypes.data_as(i64), bb.ptr, _lib.DTYPES[bb.dtype],
                                          bo.ctypes.data_as(i64), n, ny, nx, R, _lib.ptr(wp[guard:]),
                                          ws[guard:].ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    assert np.all(wp[:guard] == 7) and np.all(wp[guard + n * 7:] == 7), 'written outside peaks_out'
    assert np.all(ws[:guard] == 7) and np.all(ws[guard + n * W * W:] == 7), 'written outside surface_out'
    return wp[guard:guard + n * 7].reshape(n, 7).copy(), ws[guard:guard + n * W * W].reshape(n, W, W).copy()


def _displaced(rng, ref, d, noise=0.05):
    """ref's content displaced by the integer d (B[y + d] = A[y]); what enters from outside is fresh noise"""
    ny, nx = ref.shape
    out = rng.random((ny, nx)) * ref.max()
    ys, xs = np.arange(ny) - d[0], np.arange(nx) - d[1]
    oky, okx = (ys >= 0) & (ys < ny), (xs >= 0) & (xs < nx)
    out[np.ix_(oky, okx)] = ref[np.ix_(ys[oky], xs[okx])]
    return out + noise * ref.max() * rng.random((ny, nx))


def _case(ny, nx, R, pairs):
    """Values that are float32 numbers, so that one twin serves every dtype combination: two references at offset 5 (shared), the
    moving images at offset 3 in reversed order; pair 0 displaced to the window's corner (-R, R), pair 1 much weaker."""
    rng = np.random.default_rng(ny * 1000 + nx)
    n_pix = ny * nx
    a = (rng.random(2 * n_pix + 5) * 1000.0 + 100.0).astype(np.float32)
    b = np.zeros(pairs * n_pix + 3, dtype=np.float32)
    a_off = [5 + (k % 2) * n_pix for k in range(pairs)]
    b_off = [3 + k * n_pix for k in reversed(range(pairs))]
    true = [(-R, R), (R // 2, -1), (0, 0), (R, -R)][:pairs]
    twins = []
    for k in range(pairs):
        ref = a[a_off[k]:a_off[k] + n_pix].reshape(ny, nx).astype(np.float64)
        b[b_off[k]:b_off[k] + n_pix] = (_displaced(rng, ref, true[k]) * (0.01 if k == 1 else 1.0)).ravel()
    for k in range(pairs):
        A, B = a[a_off[k]:a_off[k] + n_pix].reshape(ny, nx), b[b_off[k]:b_off[k] + n_pix].reshape(ny, nx)
        twins.append(xr.xcorr(A, B, R) + (xr.centred(A)[1], xr.centred(B)[1]))
    return a, b, a_off, b_off, true, twins


_CASES = {}
# image, R, pairs: the smallest length; ny + R = 64 exactly with the truth at the window's corner; odd sizes; mixed lengths on the
# sub-wave geometries; 256; equality at the workload's length; the workgroup-synchronous length
SHAPES = [(24, 40, 8, 4), (56, 48, 8, 4), (37, 51, 6, 4), (100, 40, 20, 4), (200, 200, 50, 3), (512, 512, 64, 3), (600, 520, 100, 2)]


@pytest.mark.parametrize('ny,nx,R,pairs', SHAPES)
def test_surface_is_within_the_bound_of_the_twin(dev, ny, nx, R, pairs):
    """f32 / f64 in all four combinations (the three large shapes: the two mixed ones), odd offsets, shared references: v within
    (bound + half an ulp of float32) of the twin's, the integer peak the twin's -- which leads its runner-up by more than twice the
    bound, asserted -- means and energies bit for bit, the window sums within the bound, sentinels intact, a second call and a pair
    alone the same bits."""
    key = (ny, nx, R, pairs)
    if key not in _CASES:
        _CASES[key] = _case(*key)
    a, b, a_off, b_off, true, twins = _CASES[key]
    W = 2 * R + 1
    cnt = xr.counts(ny, nx, R)
    combos = [('f32', 'f64'), ('f64', 'f32')] + ([('f32', 'f32'), ('f64', 'f64')] if ny * nx < 30000 else [])
    worst = 0.0
    for ta, tb in combos:
        ab, bb = _buffer(dev, a, ta), _buffer(dev, b, tb)
        P, S = _xcorr(dev, ab, a_off, bb, b_off, ny, nx, R)
        for i in range(pairs):
            f, v, C, bound, ma, mb = twins[i]
            lead = np.sort(v.ravel())
            assert (f[0], f[1]) == true[i] and lead[-1] - lead[-2] > 2 * bound / cnt.min()
            err = np.abs(S[i].astype(np.float64) - v) - 0.5 * np.spacing(np.abs(v).astype(np.float32))
            worst = max(worst, float((err * cnt / bound).max()))
            assert np.all(err <= bound / cnt), (ta, tb, i, worst)
            assert (P[i][0], P[i][1]) == true[i] and abs(P[i][2] - f[2]) <= bound / cnt.min()
            assert P[i][3] == f[3] and P[i][4] == f[4]
            assert abs(P[i][5] - f[5]) <= (bound / cnt).sum() and abs(P[i][6] - f[6]) <= (2 * np.abs(v) * bound / cnt + (bound / cnt) ** 2).sum() * 1.01
            iy, ix = divmod(int(np.argmax(S[i])), W)
            assert (iy - R, ix - R) == true[i]
        P2, S2 = _xcorr(dev, ab, a_off, bb, b_off, ny, nx, R)
        assert P2.tobytes() == P.tobytes() and S2.tobytes() == S.tobytes()
        P1, S1 = _xcorr(dev, ab, a_off[1:2], bb, b_off[1:2], ny, nx, R)
        assert P1[0].tobytes() == P[1].tobytes() and S1[0].tobytes() == S[1].tobytes()
        plain = dev.xcorr(ab, a_off, bb, b_off, ny, nx, R)                  # without the surface
        assert plain.tobytes() == P.tobytes()
    print('%d x %d R %d: worst error / bound %.3g' % (ny, nx, R, worst))


def test_two_chunks_give_the_bits_of_pairs_alone(dev):
    """70 pairs of 200 x 200 at R = 50 span two chunks of the workspace (51 pairs fit): the pairs on either side of the cut and the
    last one give the bits they have alone, and the twin's peak."""
    ny = nx = 200
    n_pix = ny * nx
    rng = np.random.default_rng(70)
    ref = (rng.random((2, ny, nx)) * 500.0).astype(np.float32)
    d = [((7 * k) % 91 - 45, (11 * k) % 89 - 44) for k in range(70)]
    mov = np.stack([_displaced(rng, ref[k % 2].astype(np.float64), d[k]) for k in range(70)]).astype(np.float32)
    ab, bb = _buffer(dev, ref, 'f32'), _buffer(dev, mov, 'f32')
    a_off, b_off = [(k % 2) * n_pix for k in range(70)], [k * n_pix for k in range(70)]
    P = dev.xcorr(ab, a_off, bb, b_off, ny, nx, 50)
    assert [(int(p[0]), int(p[1])) for p in P] == d
    for k in (0, 50, 51, 69):
        alone = dev.xcorr(ab, a_off[k:k + 1], bb, b_off[k:k + 1], ny, nx, 50)
        assert alone[0].tobytes() == P[k].tobytes()
    f, _, _, _ = xr.xcorr(ref[1], mov[51], 50)
    assert (f[0], f[1]) == d[51] and P[51][3] == f[3] and P[51][4] == f[4]


def test_flat_images_and_refused_arguments(dev):
    from rescan_line_sted_amd._lib import RlstedError
    rng = np.random.default_rng(8)
    a = (rng.random((40, 56)) * 100.0).astype(np.float32)
    ab, bb = _buffer(dev, a, 'f32'), _buffer(dev, np.full((2, 40, 56), 3.25), 'f64')
    P = dev.xcorr(ab, [0, 0], bb, [0, 40 * 56], 40, 56, 9)
    assert np.all(P[:, :3] == 0) and np.all(P[:, 4] == 0) and np.all(P[:, 3] > 0)
    P = dev.xcorr(bb, [0], ab, [0], 40, 56, 9)
    assert np.all(P[:, :4] == 0) and P[0, 4] > 0
    c, info = _reg().coarse_shifts(np.stack([a, np.full((40, 56), 2.0, dtype=np.float32)]), a, 9)
    assert c.tolist() == [[0, 0], [0, 0]] and info['flat'].tolist() == [False, True] and info['snr'][0] > 5.0
    for ny, nx, R in ((40, 56, 0), (40, 56, 21), (1100, 2, 53)):
        with pytest.raises(RlstedError):
            dev.xcorr(ab, [0], ab, [0], ny, nx, R)


# ---- estimate_shifts(coarse=) ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('scene', range(len(xr.COARSE_SCENES)))
def test_two_stage_estimate_is_the_twins_where_the_window_alone_fails(scene):
    """160 x 160 analytic scenes drifting 0 ... 40 px, coarse = 48, max_shift = 4: the coarse displacement is the twin's, the estimate
    within 1e-6 px of the twin of the whole method (the tolerance of the plain estimate, tests/test_gpu_register.py) and within
    0.01 px of the truth.  The same call without coarse is wrong by more than a pixel wherever the drift exceeds the window, and says
    at_limit for all of those but at most one (a spurious interior maximum, tests/test_xcorr_cpu.py): what was missing."""
    seed, ny, nx, count = xr.COARSE_SCENES[scene]
    p = rr.blobs(seed, ny, nx, count)
    ref = rr.scene(p)
    d = np.array(xr.COARSE_DISPLACEMENTS)
    imgs = np.stack([rr.scene(p, x) for x in d])
    s, info = _reg().estimate_shifts(imgs, ref, max_shift=xr.COARSE_MAX_SHIFT, refine=1, coarse=xr.COARSE_RADIUS)
    worst = 0.0
    for k in range(len(d)):
        w, wi = xr.estimate(imgs[k], ref, xr.COARSE_RADIUS, xr.COARSE_MAX_SHIFT, 1)
        assert np.array_equal(info['coarse'][k], wi['coarse']) and abs(info['ncc'][k] - wi['ncc']) < 1e-9
        worst = max(worst, float(np.abs(s[k] - w).max()))
    print('scene %d: device against the twin %.3g px, against the truth %.4f px' % (seed, worst, np.abs(s - d).max()))
    assert worst <= 1e-6 and np.abs(s - d).max() <= 0.01 and not info['at_limit'].any() and not info['flat'].any()
    ps, plain = _reg().estimate_shifts(imgs, ref, max_shift=xr.COARSE_MAX_SHIFT, refine=1)
    beyond = np.abs(d).max(axis=1) > xr.COARSE_MAX_SHIFT
    assert np.all(np.abs(ps - d).max(axis=1)[beyond] > 1.0) and plain['at_limit'][beyond].sum() >= beyond.sum() - 1
    assert not plain['at_limit'][~beyond].any() and ps[0].tobytes() == s[0].tobytes()      # c = 0: the bits of the plain path


# ---- deconvolve_stack_registered(coarse=) -----------------------------------------------------------------------------------------------

def _stack(F, V, seed, view=(34.3, -35.6), drift=(0.4, -0.3), sensor=(118, 131), roi=(3, 5, 112, 120)):
    """uint16 frames of a drifting blob scene inside a larger sensor frame, with noise; view v displaced by v * view"""
    rng = np.random.default_rng(seed)
    y0, x0, ny, nx = roi
    p = rr.blobs(seed, ny, nx, 40)
    raw = rng.integers(95, 106, (F, V) + sensor).astype(np.uint16)
    for f in range(F):
        for v in range(V):
            img = rr.scene(p, (drift[0] * f + view[0] * v, drift[1] * f + view[1] * v)) * 8.0 + 100.0
            raw[f, v, y0:y0 + ny, x0:x0 + nx] = rng.poisson(img).astype(np.uint16)
    return raw, roi


def _psfs(V):
    return [rr.gaussian_psf(0.8 + 0.5 * v, 1.9 - 0.5 * v, 7) for v in range(V)]


def _camera():
    from rescan_line_sted_amd.stack import CameraModel
    return CameraModel(dark=DARK, gain=GAIN)


def test_registered_stack_with_a_view_displaced_by_more_than_32_pixels(monkeypatch):
    """u16, F = 3, V = 2, batch = 2, view 1 displaced by (34.3, -35.6), coarse = 40, max_shift = 2: the shifts follow the truth; the
    call with shifts=info['shifts'] gives the same bits; the plan of the run, used afterwards in the ordinary way, gives the bits of
    a fresh plan."""
    reg = _reg()
    from rescan_line_sted_amd import _lib as L
    kept = []

    class Keep(reg._Device):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            kept.append(self)
    monkeypatch.setattr(reg, '_Device', Keep)
    raw, roi = _stack(3, 2, 61)
    psfs = _psfs(2)
    est, info = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=2, coarse=40)
    truth = np.array([[(0.4 * f + 34.3 * v, -0.3 * f - 35.6 * v) for v in range(2)] for f in range(3)])
    print('worst shift error %.3f px; view coarse %s snr %.1f' % (np.abs(info['shifts'] - truth).max(), info['view_coarse'][1], info['view_coarse_snr'][1]))
    assert info['view_coarse'].tolist() == [[0, 0], [34, -36]] and np.abs(info['shifts'] - truth).max() < 0.25
    assert not info['at_limit'].any() and not info['view_at_limit'].any() and not info['flat'].any() and info['unresolved'] == 0
    plan = kept[0].plan
    again, info2 = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype='f32', batch=2, shifts=info['shifts'])
    assert again.tobytes() == est.tobytes() and 'coarse' not in info2
    meas, _ = ir.measurement(raw, 2, 'frame-view', roi, DARK, GAIN)
    fresh = L.DeconvPlan(psfs, 2, 112, 120, dtype='f32')
    for q in (plan, fresh):
        q.set_measurement(meas[1:3])
        q.iterate(K)
    assert plan.estimate().tobytes() == fresh.estimate().tobytes()


def test_registered_stack_without_drift_is_the_plain_call():
    """Zero drift: every coarse displacement is 0, every pair keeps today's margin, and the estimates and shifts are those of the
    coarse=None call bit for bit."""
    reg = _reg()
    raw, roi = _stack(3, 2, 62, view=(0.0, 0.0), drift=(0.0, 0.0))
    psfs = _psfs(2)
    est, info = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=2, coarse=40)
    want, winfo = reg.deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=2)
    assert not info['coarse'].any() and not info['view_coarse'].any()
    assert est.tobytes() == want.tobytes() and info['shifts'].tobytes() == winfo['shifts'].tobytes() and info['ncc'].tobytes() == winfo['ncc'].tobytes()
