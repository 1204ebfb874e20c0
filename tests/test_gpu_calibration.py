"""Camera calibration on the MI355X (include/rlsted.h rl_calib_*, rl_repair_pixels, rl_stack_set_defects;
rescan_line_sted_amd/calibration.py): the accumulators against the twin's Python integers (tests/calibration_reference.py), the maps
against its correctly rounded rationals, the repair bit for bit; CameraModel(defects=...) through deconvolve_stack,
deconvolve_stack_registered and deconvolve_tiled against deconvolve on the twin's ingested-then-repaired measurement; the plan
afterwards; what the repair buys on a stack with hot pixels; and calibrate_camera end to end."""
import ctypes

import numpy as np
import pytest

import calibration_reference as cr
import ingest_reference as ir
from conftest import max_rel
from test_gpu_stack import _Bytes, _Params, _psfs

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
SENSOR, PITCH, ROI = 40, 80, (3, 5, 33, 61)          # 40 x 72 pixels in rows of 80; a partial last vector, an unaligned origin
GAIN, K = 0.4587, 5


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


def _frames(rng, dtype, F, sy, pitch):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.integers(0, 256, (F, sy, pitch)).astype(dtype)
    if dtype == np.uint16:
        return rng.integers(0, 65536, (F, sy, pitch)).astype(dtype)
    if dtype == np.int16:
        return rng.integers(-32768, 32768, (F, sy, pitch)).astype(dtype)
    return (rng.random((F, sy, pitch)) * 4000.0 - 200.0).astype(dtype)


class _Calib:
    def __init__(self, frames, roi):
        L = _lib()
        self.L, self.ctx, self.frames, self.roi = L, L.Context.get(0), frames, roi
        self.integer = frames.dtype != np.float32
        self.raw = _Bytes(frames.nbytes).upload(frames)
        self.h = ctypes.c_void_p()
        L.check(L.lib.rl_calib_create(self.ctx.handle, cr.RAW[frames.dtype], frames.shape[1], frames.shape[2], roi[0], roi[1], roi[2], roi[3],
                                      ctypes.byref(self.h)))

    def accumulate(self, first, n):
        at = ctypes.c_void_p(self.raw.dev.value + first * self.frames[0].nbytes)
        return self.L.lib.rl_calib_accumulate(self.h, at, n)

    def count(self):
        n = ctypes.c_longlong(-1)
        self.L.check(self.L.lib.rl_calib_frames(self.h, ctypes.byref(n)))
        return n.value

    def sums(self):
        ny, nx = self.roi[2:]
        S = np.empty((ny, nx), dtype=np.int64 if self.integer else np.float64)
        Q = np.empty((ny, nx), dtype=np.uint64 if self.integer else np.float64)
        self.L.check(self.L.lib.rl_calib_sums(self.h, S.ctypes.data_as(ctypes.c_void_p), Q.ctypes.data_as(ctypes.c_void_p)))
        return S, Q

    def maps(self):
        """(mean, var), each from a buffer of its own with sentinel bytes around it."""
        n = self.roi[2] * self.roi[3] * 8
        mean, var = _Bytes(n, 8).upload(), _Bytes(n).upload()
        self.L.check(self.L.lib.rl_calib_finalize(self.h, mean.dev, var.dev))
        self.ctx.synchronize()
        return mean.download(np.float64).reshape(self.roi[2:]), var.download(np.float64).reshape(self.roi[2:])

    def __del__(self):
        if self.L.lib is not None and self.h.value:
            self.L.lib.rl_calib_destroy(self.h)
            self.h = ctypes.c_void_p()


def _check_integer(c, calls, what, large=False):
    """The frames in `calls`, twice (a reset between): sums equal the twin's integers, the mean bit for bit and the variance within
    2 units in the last place of the correctly rounded rationals, both runs identical, the source and the maps' surroundings untouched."""
    F = sum(calls)
    S, Q = (cr.sums_int_large if large else cr.sums_int)(c.frames[:F], c.roi)
    want_mean, want_var = (cr.stats_int_large if large else cr.stats_int)(S, Q, F)
    runs = []
    for _ in range(2):
        first = 0
        for n in calls:
            assert c.accumulate(first, n) == 0
            first += n
        assert c.count() == F
        gotS, gotQ = c.sums()
        mean, var = c.maps()
        runs.append((gotS.tobytes(), gotQ.tobytes(), mean.tobytes(), var.tobytes()))
        c.L.check(c.L.lib.rl_calib_reset(c.h))
        assert c.count() == 0
    assert np.array_equal(gotS, S.astype(np.int64)) and np.array_equal(gotQ, Q.astype(np.uint64)), what
    d = cr.ulps(var, want_var)
    exact = max(F * int(q) - int(s) ** 2 for s, q in zip(S.ravel(), Q.ravel())) < 2 ** 53
    print('%s: variance off by at most %d ulp, %d of %d pixels bit-equal (N < 2^53: %s)' % (what, d.max(), (d == 0).sum(), d.size, exact))
    # the mean: two exact conversions and ONE correctly rounded division -- the twin's bits.  The variance: where N < 2^53 its
    # conversion is exact too and the division rounds the exact rational once -- the twin's bits again (every shape of this file; the
    # device delivers them); a larger N may round when it is converted (1/2 ulp) before the division rounds: within 2 ulp
    assert mean.tobytes() == want_mean.tobytes() and d.max() <= (0 if exact else 2), what
    assert runs[0] == runs[1]
    c.raw.download(c.frames.dtype)                       # (asserts the sentinel behind the source)


@pytest.mark.parametrize('dtype', [np.uint16, np.uint8, np.int16])
def test_integer_accumulate_and_finalize_are_the_twin(dtype):
    """Sensor 40 x 72 in rows of 80, window 33 x 61 at (3, 5), F = 5 as 2 + 3; frame 65536 is refused and nothing changes."""
    c = _Calib(_frames(np.random.default_rng(31), dtype, 5, SENSOR, PITCH), ROI)
    _check_integer(c, (2, 3), np.dtype(dtype).name)
    assert c.accumulate(0, 2) == 0 and c.accumulate(0, 65534) == -1 and c.accumulate(0, 0) == -1 and c.count() == 2
    S, Q = cr.sums_int(c.frames[:2], ROI)
    assert np.array_equal(c.sums()[0], cr.as_int64(S))
    L = c.L
    assert L.lib.rl_calib_finalize(c.h, None, None) == -1 and L.lib.rl_calib_accumulate(c.h, None, 1) == -1
    L.check(L.lib.rl_calib_reset(c.h))
    assert L.lib.rl_calib_finalize(c.h, c.raw.dev, None) == -1            # no frame yet


def test_frame_split_and_a_large_window():
    """8 x 8 with F = 300 in one call: the launch splits the frames in 37 parts and combines them with integer atomics; 512 x 512 with
    F = 16 is 128 workgroups x 2 parts.  Both equal the twin in any case, twice."""
    rng = np.random.default_rng(32)
    _check_integer(_Calib(_frames(rng, np.uint16, 300, 9, 11), (1, 2, 8, 8)), (300,), '8 x 8, F = 300')
    _check_integer(_Calib(_frames(rng, np.uint16, 16, 512, 512), (0, 0, 512, 512)), (16,), '512 x 512, F = 16', large=True)


def test_float_accumulate_is_the_sequential_twin():
    """float32 at the first shape, F = 5 as 2 + 3: S and Q the twin's bits (contraction cannot matter: the product of two widened
    floats is exact), the mean its bits, the variance numerator within F 2^-52 Q; a nan and an inf poison their pixels only."""
    frames = _frames(np.random.default_rng(33), np.float32, 5, SENSOR, PITCH)
    frames[1, 3 + 7, 5 + 9] = np.nan
    frames[4, 3 + 32, 5 + 60] = -np.inf
    c = _Calib(frames, ROI)
    S, Q = cr.sums_f32(frames, ROI)
    want_mean, want_var, want_num = cr.stats_f32(S, Q, 5)
    runs = []
    for _ in range(2):
        assert c.accumulate(0, 2) == 0 and c.accumulate(2, 3) == 0
        gotS, gotQ = c.sums()
        mean, var = c.maps()
        runs.append((gotS.tobytes(), gotQ.tobytes(), mean.tobytes(), var.tobytes()))
        c.L.check(c.L.lib.rl_calib_reset(c.h))
    assert gotS.tobytes() == S.tobytes() and gotQ.tobytes() == Q.tobytes() and runs[0] == runs[1]
    bad = ~np.isfinite(S) | ~np.isfinite(Q)
    assert np.array_equal(np.argwhere(bad), [[7, 9], [32, 60]]) and np.array_equal(~np.isfinite(mean) | ~np.isfinite(var), bad)
    ok = ~bad
    assert mean[ok].tobytes() == want_mean[ok].tobytes()
    off = np.abs(var[ok] * 4.0 - want_num[ok])
    print('f32 variance: numerator off by at most %.3e of a bound of %.3e; bits equal: %s' % (off.max(), (5 * 2.0 ** -52 * Q[ok]).min(),
                                                                                       var[ok].tobytes() == want_var[ok].tobytes()))
    assert np.all(off <= 5 * 2.0 ** -52 * Q[ok])


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_repair_is_the_twin(dtype):
    """The CPU test's cases at 64 x 96, 8 images: bit for bit the twin, in place, `unrepaired` its count, the bytes around the images
    untouched (an odd element offset), a second call on the repaired images changes nothing."""
    L = _lib()
    ctx = L.Context.get(0)
    rng = np.random.default_rng(34)
    ny, nx = 64, 96
    images = (rng.random((8, ny, nx)) * 500.0).astype(NP[dtype])
    for name, (mask, radius, left) in cr.repair_cases(ny, nx).items():
        want, want_left = cr.repair(images, mask, radius)
        assert want_left == left
        buf = _Bytes(images.nbytes, images.itemsize).upload(images)
        got_left = np.full(8, -1, dtype=np.int64)
        m8 = np.ascontiguousarray(mask).view(np.uint8)
        for again in range(2):
            L.check(L.lib.rl_repair_pixels(ctx.handle, buf.dev, L.DTYPES[dtype], 8, ny, nx, m8.ctypes.data_as(ctypes.c_void_p), radius,
                                           got_left.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
            ctx.synchronize()
            assert buf.download(NP[dtype]).tobytes() == want.tobytes(), (name, again)
            assert np.all(got_left == left)
    assert not np.array_equal(want, images)


def _window_stack(F, V, seed, hot, static=False):
    """uint16 frames of a 101 x 137 sensor whose window (2, 4, 96, 128) is deconvolved (static: the same scene in every image), a
    float32 dark map of the window, and a defect map: hot pixels (planted in the frames), a pair at the window's edge, a 2 x 2
    cluster, a corner."""
    rng = np.random.default_rng(seed)
    roi = (2, 4, 96, 128)
    yy, xx = np.mgrid[0:101, 0:137]
    raw = np.empty((F, V, 101, 137), dtype=np.uint16)
    for f in range(F):
        for v in range(V):
            a, b, c = (0.0, 0.0, 0.0) if static else (f, 0.4 * f, v)
            raw[f, v] = 100 + rng.poisson(300.0 + 250.0 * np.sin(0.21 * yy + a) * np.cos(0.17 * xx - b + c))
    mask = np.zeros((96, 128), dtype=bool)
    for y, x in hot:
        mask[y, x] = True
        raw[:, :, 2 + y, 4 + x] = 60000
    mask[0, 50] = mask[0, 51] = mask[95, 127] = True
    mask[40:42, 70:72] = True
    dark = (98.0 + 4.0 * rng.random((96, 128))).astype(np.float32)
    return raw, roi, dark, mask


def _repaired_measurement(raw, V, roi, dark, mask, dtype, radius=3):
    """The twin's ingest in the plan's element type, then the twin's repair in that type (what the device does: for an even number
    of candidates the mean of two float32 values is not the float32 of the mean of their float64 originals), widened to float64."""
    meas, stats = ir.measurement(raw, V, 'frame-view', roi, dark, GAIN, None, dtype=NP[dtype])
    F = meas.shape[0]
    fixed, _ = cr.repair(meas.reshape(F * V, roi[2], roi[3]), mask, radius)
    return fixed.reshape(meas.shape).astype(np.float64), meas.astype(np.float64), stats


HOT = [(10, 20), (33, 100), (77, 5), (90, 64)]


@pytest.mark.parametrize('dtype,V', [('f64', 1), ('f32', 2), ('f32', 1)])
def test_stack_with_defects_is_deconvolve_on_the_repaired_measurement(dtype, V):
    """F = 3, batch = 2: two chunks, a short last one; a 96 x 128 window of a larger sensor; a dark map.  Bit for bit deconvolve on the
    twin's ingested-then-repaired measurement (single-view f32 plans: the 1e-5 contract of their pair loop); the statistics are the
    ingest's; defects=None gives the bits of the call without the argument."""
    from rescan_line_sted_amd.line_sted_tools import deconvolve
    from rescan_line_sted_amd.stack import CameraModel, deconvolve_stack
    raw, roi, dark, mask = _window_stack(3, V, 40 + V, HOT)
    psfs = _psfs(V)
    fixed, meas, stats = _repaired_measurement(raw, V, roi, dark, mask, dtype)
    assert meas[:, :, 10, 20].min() > 20000 and fixed[:, :, 10, 20].max() < 1000
    want = deconvolve(fixed, psfs, K, dtype=dtype)
    kw = dict(roi=roi, dtype=dtype, out_dtype=dtype, batch=2)
    est, info = deconvolve_stack(raw, psfs, K, camera=CameraModel(dark, GAIN, defects=mask), **kw)
    assert info['chunks'] == 2 and info['defects'] == mask.sum() == 11 and info['unrepaired'] == 0
    if (dtype, V) == ('f32', 1):
        err = max(max_rel(est[f], want[f]) for f in range(3))
        print('f32 single view with defects: normwise %.3e' % err)
        assert err <= 1e-5
    else:
        assert est.astype(np.float64).tobytes() == want.tobytes()
    assert np.array_equal(info['clipped'], stats[:, :, 1]) and (np.array_equal(info['level'], stats[:, :, 0]) if dtype == 'f64' else True)
    unrepaired = deconvolve(meas, psfs, K, dtype=dtype)
    assert max_rel(unrepaired, want) > 1.0                               # (the hot pixels matter)
    a, ia = deconvolve_stack(raw, psfs, K, camera=CameraModel(dark, GAIN, defects=None), **kw)
    b, ib = deconvolve_stack(raw, psfs, K, camera=CameraModel(dark, GAIN), **kw)
    assert a.tobytes() == b.tobytes() and ia['defects'] == ib['defects'] == 0
    if (dtype, V) != ('f32', 1):
        assert a.astype(np.float64).tobytes() == unrepaired.tobytes()


@pytest.mark.parametrize('dtype,V', [('f64', 2), ('f32', 2), ('f32', 1)])
def test_registered_stack_with_defects(dtype, V):
    """The repair precedes references and estimates: pipeline=True equals the host loop bit for bit, shifts included; with zero shifts
    given (interp = 1) both are deconvolve_stack with the same defects."""
    from rescan_line_sted_amd.registration import deconvolve_stack_registered
    from rescan_line_sted_amd.stack import CameraModel, deconvolve_stack
    raw, roi, dark, mask = _window_stack(3, V, 50 + V, HOT, static=True)
    psfs = _psfs(V)
    cam = CameraModel(dark, GAIN, defects=mask, repair_radius=2)

    def same(got, want, what):
        if (dtype, V) == ('f32', 1):
            assert max(max_rel(got[f], want[f]) for f in range(len(want))) <= 1e-5, what
        else:
            assert got.tobytes() == want.tobytes(), what
    kw = dict(camera=cam, roi=roi, dtype=dtype, batch=2, max_shift=3)
    host, hinfo = deconvolve_stack_registered(raw, psfs, K, **kw)
    pipe, pinfo = deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='f64', **kw)
    assert pinfo['shifts'].tobytes() == hinfo['shifts'].tobytes() and pinfo['level'].tobytes() == hinfo['level'].tobytes()
    assert hinfo['defects'] == pinfo['defects'] == 11 and hinfo['unrepaired'] == 0
    same(pipe, host, 'pipeline against the host loop')
    plain, _ = deconvolve_stack_registered(raw, psfs, K, camera=CameraModel(dark, GAIN), roi=roi, dtype=dtype, batch=2, max_shift=3)
    assert max_rel(plain, host) > 1.0
    want, _ = deconvolve_stack(raw, psfs, K, camera=cam, roi=roi, dtype=dtype, out_dtype='f64', batch=2)
    zero = dict(camera=cam, roi=roi, dtype=dtype, batch=2, shifts=np.zeros((3, V, 2)), interp=1)
    same(deconvolve_stack_registered(raw, psfs, K, **zero)[0], want, 'host loop, zero shifts')
    same(deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='f64', **zero)[0], want, 'pipeline, zero shifts')


def test_tiled_with_defects_is_the_tiled_run_on_the_repaired_image():
    from rescan_line_sted_amd.stack import CameraModel
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    rng = np.random.default_rng(61)
    raw = (100 + rng.poisson(300.0, (2, 1, 150, 131))).astype(np.uint16)
    mask = np.zeros((150, 131), dtype=bool)
    mask[rng.integers(0, 150, 30), rng.integers(0, 131, 30)] = True
    mask[60:67, 60:67] = True                                             # (spans a tile seam; its centre stays)
    raw[:, :, mask] = 50000
    meas, _ = ir.measurement(raw, 1, dark=100.25, gain=GAIN)
    fixed, left = cr.repair(meas.reshape(2, 150, 131), mask, 3)
    psfs = _psfs(1)
    want, _ = deconvolve_tiled(fixed.reshape(2, 1, 150, 131), psfs, K, tile=64, overlap=24, margin=8, dtype='f64')
    got, info = deconvolve_tiled(raw, psfs, K, tile=64, overlap=24, margin=8, dtype='f64', camera=CameraModel(100.25, GAIN, defects=mask))
    assert got.tobytes() == want.tobytes() and info['defects'] == mask.sum() and info['unrepaired'] == left == 1


def test_a_plan_that_ran_a_stack_with_defects_is_a_fresh_plan():
    """rl_stack_set_defects, rl_stack_run, then an ordinary set_measurement / iterate on the same plan: the bits of a fresh plan.
    Setting the map again, and to none, works on a stack that has run."""
    from rescan_line_sted_amd.line_sted_tools import deconvolve
    L = _lib()
    raw, roi, dark, mask = _window_stack(3, 1, 71, HOT)
    psfs = _psfs(1)
    plan = L.DeconvPlan(psfs, 2, 96, 128, dtype='f64')
    p = _Params(1, 0, 101, 137, 137, 2, 4, 0.0, GAIN, 1e-9, 0.0, dark.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, 1.0)
    stack = ctypes.c_void_p()
    L.check(L.lib.rl_stack_create(plan.handle, ctypes.byref(p), ctypes.byref(stack)))
    m8 = np.ascontiguousarray(mask).view(np.uint8)
    assert L.lib.rl_stack_set_defects(stack, m8.ctypes.data_as(ctypes.c_void_p), 0) == -1
    assert L.lib.rl_stack_set_defects(stack, m8.ctypes.data_as(ctypes.c_void_p), 4) == -1
    out = np.zeros((3, 96, 128))

    def run():
        L.check(L.lib.rl_stack_run(stack, raw.ctypes.data_as(ctypes.c_void_p), 3, K, out.ctypes.data_as(ctypes.c_void_p), None, None, None))
        return out.copy()
    fixed, meas, _ = _repaired_measurement(raw, 1, roi, dark, mask, 'f64')
    L.check(L.lib.rl_stack_set_defects(stack, m8.ctypes.data_as(ctypes.c_void_p), 3))
    assert run().tobytes() == deconvolve(fixed, psfs, K, dtype='f64').tobytes()
    other = np.ascontiguousarray(meas[:2][::-1]) * 1.5
    fresh = L.DeconvPlan(psfs, 2, 96, 128, dtype='f64')
    for q in (plan, fresh):
        q.set_measurement(other)
        q.iterate(K)
    assert plan.estimate().tobytes() == fresh.estimate().tobytes()
    L.check(L.lib.rl_stack_set_defects(stack, None, 0))
    assert run().tobytes() == deconvolve(meas, psfs, K, dtype='f64').tobytes()
    L.check(L.lib.rl_stack_set_defects(stack, m8.ctypes.data_as(ctypes.c_void_p), 3))
    assert run().tobytes() == deconvolve(fixed, psfs, K, dtype='f64').tobytes()
    assert L.lib.rl_stack_destroy(stack) == 0


# The error of the K = 20 estimate with repaired hot pixels relative to that of the clean stack, ||est - object||_2 / ||object||_2,
# on calibration_reference.benefit_stack(): measured ON THE FLOAT64 ORACLE (oracle/line_sted_oracle.py through
# tile_reference.oracle_estimate) with the twin's repair at radius 3, no device code involved -- 1.000261 and 1.000431 for the two
# frames (errors 0.444182 / 0.444066 and 0.442849 / 0.442659; without the repair 2.1238 and 2.1228).
ORACLE_REPAIR_FACTOR = 1.000431


def test_repair_buys_back_the_clean_stacks_error():
    """Ten hot pixels at 20 times the frames' maximum on an object at about 100 photons per pixel, K = 20, f32 plan: the error to the
    true object is strictly smaller with defects= than without, and within 1.5 x the oracle's factor of the clean stack's error."""
    from rescan_line_sted_amd.stack import CameraModel, deconvolve_stack
    obj, psfs, clean, dirty, mask = cr.benefit_stack()
    assert mask.sum() == 10 and dirty.max() == 20 * clean.max()

    def errors(raw, **camera):
        est, _ = deconvolve_stack(raw, psfs, 20, camera=CameraModel(100.0, 1.0, **camera), dtype='f32')
        return np.array([np.linalg.norm(e.astype(np.float64) - obj) / np.linalg.norm(obj) for e in est])
    e_clean, e_dirty, e_fixed = errors(clean), errors(dirty), errors(dirty, defects=mask)
    print('error to the object: clean %s, hot pixels %s, repaired %s' % (e_clean, e_dirty, e_fixed))
    assert np.all(e_fixed < e_dirty) and np.all(e_fixed <= 1.5 * ORACLE_REPAIR_FACTOR * e_clean)


def test_calibrate_camera_end_to_end(monkeypatch):
    """The synthetic camera through the device: the CPU test's assertions, and the maps of the numpy stand-in path bit for bit (exact
    integer sums; at 96 frames of 12-bit data N < 2^53, so the one division rounds the exact rational)."""
    from rescan_line_sted_amd import calibration
    from test_calibration_cpu import _check_calibration
    cam = cr.Camera(3)
    dark, levels = cam.stacks()
    camera, report = calibration.calibrate_camera(dark, levels, saturation=65535, chunk_frames=40)
    _check_calibration(camera, report, cam)
    monkeypatch.setattr(calibration, '_Device', cr.NumpyDevice)
    twin, treport = calibration.calibrate_camera(dark, levels, saturation=65535)
    assert report['dark_mean'].tobytes() == treport['dark_mean'].tobytes() and report['dark_var'].tobytes() == treport['dark_var'].tobytes()
    for (m, v), (tm, tv) in zip(report['levels'], treport['levels']):
        assert m.tobytes() == tm.tobytes() and v.tobytes() == tv.tobytes()
    assert camera.gain == twin.gain and camera.dark_map.tobytes() == twin.dark_map.tobytes() and np.array_equal(camera.defects, twin.defects)
    monkeypatch.undo()
    images = np.random.default_rng(1).random((3, 48, 64)).astype(np.float32)
    assert np.array_equal(calibration.repair_defects(images, report['mask']), cr.repair(images, report['mask'], 3)[0])


def _median_is_a_neighbour(raw):
    """Pixels of (F, V, ny, nx) integer frames, at least 2 from the edge, whose 8 neighbours' two middle values are equal in every
    image: (mask of them, that value per image).  There the repaired pixel is exactly the ingest of an integer raw value."""
    F, V, ny, nx = raw.shape
    inner = raw[:, :, 2:-2, 2:-2].shape[2:]
    nb = np.stack([raw[:, :, 2 + dy:2 + dy + inner[0], 2 + dx:2 + dx + inner[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)])
    nb = np.sort(nb, axis=0)
    ok = np.zeros((ny, nx), dtype=bool)
    ok[2:-2, 2:-2] = (nb[3] == nb[4]).all(axis=(0, 1))
    value = np.zeros(raw.shape, dtype=raw.dtype)
    value[:, :, 2:-2, 2:-2] = nb[3]
    return ok, value


def test_measure_psfs_repairs_before_the_search():
    """Bead frames with hot pixels planted where the repair's result is known without the repair: the median of the 8 neighbours is
    one of them (their two middle values are equal), an integer, so a stack that holds that integer there ingests to the same bits.
    measure_psfs with the defect map on the hot stack equals measure_psfs without one on that stack, bit for bit."""
    import beads_reference as br
    from rescan_line_sted_amd import beads
    from rescan_line_sted_amd.stack import CameraModel
    raw, _ = br.bead_stack(3, 160, 192, 21, True, seed=11, spacing=23, edge=24)
    ok, value = _median_is_a_neighbour(raw)
    cells = []
    for y, x in np.argwhere(ok):
        if all(max(abs(y - a), abs(x - b)) > 2 for a, b in cells):
            cells.append((y, x))
    cells = cells[:6]
    assert len(cells) >= 3
    mask = np.zeros((160, 192), dtype=bool)
    hot, ref = raw.copy(), raw.copy()
    for y, x in cells:
        mask[y, x] = True
        hot[:, :, y, x] = 60000
        ref[:, :, y, x] = value[:, :, y, x]
    want, winfo = beads.measure_psfs(ref, 21, camera=CameraModel(dark=100.0, gain=1.0))
    got, info = beads.measure_psfs(hot, 21, camera=CameraModel(dark=100.0, gain=1.0, defects=mask, repair_radius=1))
    assert info['defects'] == len(cells) and info['unrepaired'] == 0 and winfo['defects'] == 0
    for v in range(2):
        assert got[v].tobytes() == want[v].tobytes() and info['positions'][v].tobytes() == winfo['positions'][v].tobytes()
        assert info['rejected'][v] == winfo['rejected'][v]
