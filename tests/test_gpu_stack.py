"""Acquired camera stacks on the MI355X (include/rlsted.h rl_ingest, rl_export, rl_stack_*; rescan_line_sted_amd/stack.py): the two
kernels bit for bit against the numpy twin (tests/ingest_reference.py), nothing written behind the destination or into a plan
buffer's slack; deconvolve_stack against deconvolve on the twin's float64 measurement, its orders, page-locked arrays, `out=`, the
u16 export, the ingest's counts and both opt-in modes; deconvolve_tiled(camera=...) against the float64 path; and the plan a
pipeline has used against a fresh one.  Images 40 x 48, PSFs 9 x 9, K = 3."""
import ctypes
import itertools

import numpy as np
import pytest

import ingest_reference as ir
from conftest import max_rel

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64, 'u16': np.uint16}
SHAPES = [(5, 13), (7, 16), (3, 33)]
ORIGINS = [(0, 0), (2, 1), (1, 5)]
GAIN, DARK, K = 0.4587, 100.25, 3
NY, NX = 40, 48
GUARD = 64


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


class _Bytes:
    """A device buffer holding `payload` bytes from byte `shift` on, followed by GUARD sentinel bytes (rl_device_upload /
    rl_device_download of float64 elements are plain copies of 8-byte words)."""

    def __init__(self, payload, shift=0):
        L = _lib()
        self.ctx = L.Context.get(0)
        self.shift, self.n = shift, payload
        self.words = np.zeros(-(-(shift + payload + GUARD) // 8), dtype=np.float64)
        self.host = self.words.view(np.uint8)
        self.host[:] = 0x5A
        self.base = ctypes.c_void_p()
        L.check(L.lib.rl_device_alloc(self.ctx.handle, self.words.nbytes, ctypes.byref(self.base)))
        self.dev = ctypes.c_void_p(self.base.value + shift)

    def upload(self, array=None):
        L = _lib()
        if array is not None:
            self.host[self.shift:self.shift + self.n] = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        L.check(L.lib.rl_device_upload(self.ctx.handle, self.base, L.RL_F64, self.words.size, L.ptr(self.words)))
        return self

    def download(self, dtype):
        """The payload as `dtype`; asserts that the bytes around it are still the sentinel."""
        L = _lib()
        back = np.zeros_like(self.words)
        L.check(L.lib.rl_device_download(self.ctx.handle, self.base, L.RL_F64, back.size, L.ptr(back)))
        b = back.view(np.uint8)
        assert np.all(b[:self.shift] == 0x5A) and np.all(b[self.shift + self.n:] == 0x5A), 'written outside the destination'
        return b[self.shift:self.shift + self.n].copy().view(dtype)

    def __del__(self):
        L = _lib()
        if L.lib is not None and self.base.value:
            L.lib.rl_device_free(self.ctx.handle, self.base)
            self.base = ctypes.c_void_p()


def _raw_frames(rng, dtype, shape):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.integers(60, 256, shape).astype(dtype)
    if dtype == np.float32:
        a = (rng.random(shape) * 4000.0 - 200.0).astype(dtype)
        r = rng.random(shape)
        a[r < 0.04], a[(r >= 0.04) & (r < 0.07)], a[(r >= 0.07) & (r < 0.10)], a[(r >= 0.10) & (r < 0.14)] = np.nan, np.inf, -np.inf, 65535.0
        return a
    a = rng.integers(-300 if dtype == np.int16 else 60, 4000, shape).astype(dtype)
    a[rng.random(shape) < 0.05] = np.iinfo(dtype).max
    return a


def _psfs(V, seed=0):
    rng = np.random.default_rng(100 + seed)
    yy, xx = np.mgrid[-4:5, -4:5]
    out = []
    for v in range(V):
        p = np.exp(-(yy ** 2 / (2.0 * (1.0 + v) ** 2) + xx ** 2 / 4.5)) * (1.0 + 0.2 * rng.random((9, 9)))
        out.append((p / p.sum())[None])
    return out


def _camera_frames(F, V, seed, shape=(NY, NX)):
    """uint16 frames of a few hundred counts over a dark level of 100, some pixels saturated, some below the dark level."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    raw = np.empty((F, V) + tuple(shape), dtype=np.uint16)
    for f in range(F):
        obj = 300.0 + 250.0 * np.sin(0.3 * yy + f) * np.cos(0.23 * xx - 0.5 * f)
        for v in range(V):
            raw[f, v] = 100 + rng.poisson(obj * (1.0 + 0.1 * v))
    hit = rng.random(raw.shape)
    raw[hit < 0.004] = 65535
    raw[(hit >= 0.004) & (hit < 0.012)] = 90
    return raw


# ---- the kernels -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dst_dtype', ['f32', 'f64'])
@pytest.mark.parametrize('raw_dtype', [np.uint8, np.uint16, np.int16, np.float32])
def test_ingest_is_the_numpy_twin(raw_dtype, dst_dtype):
    """The CPU test's shapes, pitches, origins, orders and dark forms: stored values and statistics bit for bit, the sentinel behind
    (and, at the odd offset, before) the destination untouched, a second run identical."""
    L = _lib()
    rng = np.random.default_rng(21)
    ctx = L.Context.get(0)
    sat = 250.0 if np.dtype(raw_dtype).itemsize == 1 else float(np.iinfo(np.int16).max if np.dtype(raw_dtype) == np.int16 else 65535)
    esize = np.dtype(NP[dst_dtype]).itemsize
    n = 0
    for (ny, nx), pad, (y0, x0), (V, view_frame, dark_map) in itertools.product(SHAPES, (0, 3), ORIGINS, ((1, False, True), (3, True, False), (3, False, True))):
        n += 1
        n_slots, n_valid = 3, 2
        src_ny, src_pitch = y0 + ny, x0 + nx + pad
        raw = _raw_frames(rng, raw_dtype, (n_valid * V, src_ny, src_pitch))
        dark = (90.0 + rng.random((ny, nx)) * 30.0).astype(np.float32) if dark_map else None
        fs, vs = (1, n_valid) if view_frame else (V, 1)
        want, want_stats = ir.ingest(raw, n_slots, n_valid, V, ny, nx, y0, x0, fs, vs, dark, DARK, GAIN, 1e-9, sat, NP[dst_dtype])
        raw_dev = _Bytes(raw.nbytes).upload(raw)
        dark_dev = _Bytes(dark.nbytes).upload(dark) if dark_map else None
        shift = esize * (n % 2)                                  # every other case: not 16-byte aligned
        dst, stats = _Bytes(want.nbytes, shift).upload(), _Bytes(want_stats.nbytes).upload()
        runs = []
        for _ in range(2):
            L.check(L.lib.rl_ingest(ctx.handle, raw_dev.dev, ir.RAW[raw.dtype], n_valid * V, src_ny, src_pitch, y0, x0, fs, vs, n_slots, n_valid,
                                    V, ny, nx, dark_dev.dev if dark_map else None, DARK, GAIN, 1e-9, sat, dst.dev, L.DTYPES[dst_dtype], stats.dev))
            runs.append((dst.download(NP[dst_dtype]).tobytes(), stats.download(np.float64).tobytes()))
        assert runs[0][0] == want.tobytes(), (ny, nx, pad, y0, x0, V, view_frame, dark_map)
        assert runs[0][1] == want_stats.tobytes(), (np.frombuffer(runs[0][1]), want_stats)
        assert runs[0] == runs[1]
        raw_dev.download(raw.dtype)                              # (the source is read only: its sentinel too)


@pytest.mark.parametrize('out_dtype', ['f32', 'f64', 'u16'])
@pytest.mark.parametrize('est_dtype', ['f32', 'f64'])
def test_export_is_the_numpy_twin(est_dtype, out_dtype):
    L = _lib()
    rng = np.random.default_rng(22)
    ctx = L.Context.get(0)
    osize = np.dtype(NP[out_dtype]).itemsize
    for i, (ny, nx) in enumerate(SHAPES + [(NY, NX), (70, 260)]):
        est = (rng.random((3, ny, nx)) * 900.0 - 50.0).astype(NP[est_dtype])
        est[1, 0, :4] = [np.nan, -3.0, 70000.0, 65535.2]
        est[2, 0, :4] = [0.5 / 80.5, 1.5 / 80.5, 2.5 / 80.5, 3.5 / 80.5]
        want, want_stats = ir.export(est, 80.5, NP[out_dtype])
        est_dev = _Bytes(est.nbytes).upload(est)
        out, stats = _Bytes(want.nbytes, osize * (i % 2)).upload(), _Bytes(want_stats.nbytes).upload()
        runs = []
        for _ in range(2):
            L.check(L.lib.rl_export(ctx.handle, est_dev.dev, L.DTYPES[est_dtype], 3, ny, nx, 80.5, out.dev, ir.OUT[np.dtype(NP[out_dtype])], stats.dev))
            runs.append((out.download(NP[out_dtype]).tobytes(), stats.download(np.float64).tobytes()))
        assert runs[0][0] == want.tobytes() and runs[0][1] == want_stats.tobytes(), (ny, nx)
        assert runs[0] == runs[1]
        if out_dtype == 'u16':
            assert want_stats[1, 1] >= 2 and np.array_equal(want_stats[:, 1], (est.astype(np.float64) * 80.5 > 65535.0).reshape(3, -1).sum(axis=1))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_ingest_into_a_plan_leaves_its_slack_zero(dtype):
    """The measurement buffer of a plan of 2 frames x 3 views of 40 x 48: the twin's values, and the 16 KiB behind them still zero."""
    L = _lib()
    plan = L.DeconvPlan(_psfs(3), 2, NY, NX, dtype=dtype)
    raw = _camera_frames(2, 3, 5, (NY + 3, NX + 7))
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    L.check(L.lib.rl_deconv_device_ptr(plan.handle, 1, ctypes.byref(p), ctypes.byref(n), None))
    assert n.value == 2 * 3 * NY * NX
    raw_dev = _Bytes(raw.nbytes).upload(raw)
    L.check(L.lib.rl_ingest(plan.ctx.handle, raw_dev.dev, 1, 6, NY + 3, NX + 7, 2, 5, 3, 1, 2, 2, 3, NY, NX, None, DARK, GAIN, 1e-9, 65535.0, p,
                            L.DTYPES[dtype], None))
    slack = 16384 // np.dtype(NP[dtype]).itemsize
    back = np.empty(n.value + slack)
    L.check(L.lib.rl_device_download(plan.ctx.handle, p, L.DTYPES[dtype], back.size, L.ptr(back)))
    want, _ = ir.ingest(raw.reshape(6, NY + 3, NX + 7), 2, 2, 3, NY, NX, 2, 5, 3, 1, None, DARK, GAIN, 1e-9, 65535.0, NP[dtype])
    assert np.array_equal(back[:n.value], want.astype(np.float64).ravel()) and np.all(back[n.value:] == 0.0)


def test_byte_upload_moves_exactly_its_bytes():
    """rl_device_upload_bytes: 13 bytes to an odd device address, the bytes around them untouched."""
    L = _lib()
    data = np.arange(200, 213, dtype=np.uint8)
    buf = _Bytes(13, 3).upload()
    L.check(L.lib.rl_device_upload_bytes(buf.ctx.handle, buf.dev, data.ctypes.data_as(ctypes.c_void_p), 13))
    assert np.array_equal(buf.download(np.uint8), data)


# ---- deconvolve_stack ------------------------------------------------------------------------------------------------------------

def _reference(raw, psfs, dtype, **modes):
    """deconvolve on the twin's float64 measurement of frame-view uint16 frames."""
    from rescan_line_sted_amd.line_sted_tools import deconvolve
    meas, stats = ir.measurement(raw, len(psfs), dark=DARK, gain=GAIN, saturation=65535.0)
    return deconvolve(meas, psfs, K, dtype=dtype, **modes), meas, stats


def _camera():
    from rescan_line_sted_amd.stack import CameraModel
    return CameraModel(dark=DARK, gain=GAIN, saturation=65535)


@pytest.mark.parametrize('dtype,V', [('f64', 1), ('f64', 3), ('f32', 3), ('f32', 1)])
def test_stack_is_deconvolve_on_the_twins_measurement(dtype, V):
    """uint16, F = 5, batch = 2: three chunks, both slots, one reuse, a filler.  Bit for bit, except single-view f32 plans: their
    frames run as pairs where the device-measured levels allow, a frame's partner differs between the two calls, and the result is
    held to the project's 1e-5 normwise contract (the caveat deconvolve_tiled documents)."""
    from rescan_line_sted_amd.stack import deconvolve_stack
    raw, psfs = _camera_frames(5, V, 31 + V), _psfs(V)
    want, _, stats = _reference(raw, psfs, dtype)
    est, info = deconvolve_stack(raw, psfs, K, camera=_camera(), dtype=dtype, out_dtype=dtype, batch=2)
    assert est.shape == (5, NY, NX) and est.dtype == NP[dtype] and info['chunks'] == 3 and info['batch'] == 2 and info['unresolved'] == 0
    if (dtype, V) == ('f32', 1):
        err = max(max_rel(est[f], want[f]) for f in range(5))
        print('f32 single view: normwise %.3e' % err)
        assert err <= 1e-5
    else:
        assert est.astype(np.float64).tobytes() == want.tobytes()
    assert np.array_equal(info['clipped'], stats[:, :, 1]) and np.array_equal(info['saturated'], stats[:, :, 2]) and not info['invalid'].any()
    assert np.array_equal(info['level'], stats[:, :, 0]) if dtype == 'f64' else np.allclose(info['level'], stats[:, :, 0], rtol=1e-6)
    assert all(t > 0 for t in info['times'].values())


def test_orders_pinned_arrays_and_out_give_the_same_bits():
    from rescan_line_sted_amd.stack import deconvolve_stack
    L = _lib()
    raw, psfs = _camera_frames(5, 3, 41), _psfs(3)
    est, _ = deconvolve_stack(raw, psfs, K, camera=_camera(), dtype='f64', out_dtype='f64', batch=2)
    by_view, _ = deconvolve_stack(np.ascontiguousarray(raw.transpose(1, 0, 2, 3)), psfs, K, camera=_camera(), order='view-frame', dtype='f64',
                                  out_dtype='f64', batch=2)
    assert by_view.tobytes() == est.tobytes()
    pinned_raw, pinned_out = L.pinned_empty(raw.shape, np.uint16), L.pinned_empty(est.shape, np.float64)
    pinned_raw[:] = raw
    pinned_out[:] = -1.0
    got, _ = deconvolve_stack(pinned_raw, psfs, K, camera=_camera(), dtype='f64', out_dtype='f64', batch=2, out=pinned_out)
    assert got is pinned_out and pinned_out.tobytes() == est.tobytes()
    out = np.full(est.shape, -1.0)
    got, _ = deconvolve_stack(raw, psfs, K, camera=_camera(), dtype='f64', out_dtype='f64', batch=2, out=out)
    assert got is out and out.tobytes() == est.tobytes()
    one, _ = deconvolve_stack(raw, psfs, K, camera=_camera(), dtype='f64', out_dtype='f64')           # one chunk of five
    assert one.tobytes() == est.tobytes()


def test_u16_export_and_ingest_counts():
    """out_dtype='u16' is the twin's rounding of the f32 path's estimate, `clamped` numpy's count at a scale that overflows a few
    pixels; `saturated` and `clipped` numpy's counts on frames built to hold some; a window of a larger sensor."""
    from rescan_line_sted_amd.stack import deconvolve_stack
    psfs = _psfs(1)
    sensor = _camera_frames(5, 1, 51, (NY + 6, NX + 9))
    roi = (4, 7, NY, NX)
    est, info = deconvolve_stack(sensor, psfs, K, camera=_camera(), roi=roi, batch=2)
    assert est.dtype == np.float32
    top = np.sort(est.astype(np.float64).ravel())[-6]
    scale = 65535.0 / top                                                 # the five largest pixels overflow
    as_u16, info16 = deconvolve_stack(sensor, psfs, K, camera=_camera(), roi=roi, batch=2, out_dtype='u16', out_scale=scale)
    want, want_stats = ir.export(est, scale, np.uint16)
    assert as_u16.dtype == np.uint16 and np.array_equal(as_u16, want)
    count = (est.astype(np.float64) * scale > 65535.0).reshape(5, -1).sum(axis=1)
    assert np.array_equal(info16['clamped'], count) and 1 <= count.sum() <= 6 and not info['clamped'].any()
    assert info16['flux'].tobytes() == want_stats[:, 0].tobytes()
    win = sensor[:, :, 4:4 + NY, 7:7 + NX].astype(np.float64)
    assert np.array_equal(info['saturated'], (win >= 65535).sum(axis=(2, 3))) and info['saturated'].sum() > 0
    assert np.array_equal(info['clipped'], (win < DARK).sum(axis=(2, 3))) and info['clipped'].sum() > 0


@pytest.mark.parametrize('modes', [dict(acceleration='biggs-andrews'), dict(tv_lambda=0.01)], ids=['biggs-andrews', 'rl-tv'])
def test_opt_in_modes_are_those_of_deconvolve(modes):
    from rescan_line_sted_amd.stack import deconvolve_stack
    raw, psfs = _camera_frames(5, 1, 61), _psfs(1)
    want, _, _ = _reference(raw, psfs, 'f64', **modes)
    plain, _, _ = _reference(raw, psfs, 'f64')
    est, _ = deconvolve_stack(raw, psfs, K, camera=_camera(), dtype='f64', out_dtype='f64', batch=2, **modes)
    assert est.tobytes() == want.tobytes() and est.tobytes() != plain.tobytes()


def test_tiled_with_a_camera_is_the_float64_path():
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    raw, psfs = _camera_frames(2, 1, 71, (150, 131)), _psfs(1)
    meas, _ = ir.measurement(raw, 1, dark=DARK, gain=GAIN)
    want, _ = deconvolve_tiled(meas, psfs, K, tile=64, overlap=24, margin=8, dtype='f64')
    got, info = deconvolve_tiled(raw, psfs, K, tile=64, overlap=24, margin=8, dtype='f64', camera=_camera())
    assert info['tiles'] == 24 and got.shape == (2, 150, 131) and got.tobytes() == want.tobytes()
    dark = np.full((150, 131), DARK, dtype=np.float32)                    # (100.25 is a float32: the map gives the same bits)
    from rescan_line_sted_amd.stack import CameraModel
    got, _ = deconvolve_tiled(raw, psfs, K, tile=64, overlap=24, margin=8, dtype='f64', camera=CameraModel(dark=dark, gain=GAIN))
    assert got.tobytes() == want.tobytes()


# ---- the plan afterwards ---------------------------------------------------------------------------------------------------------

class _Params(ctypes.Structure):
    _fields_ = [('raw_dtype', ctypes.c_int), ('order', ctypes.c_int), ('src_ny', ctypes.c_int), ('src_nx', ctypes.c_int),
                ('src_pitch', ctypes.c_int), ('y0', ctypes.c_int), ('x0', ctypes.c_int), ('offset', ctypes.c_double),
                ('gain', ctypes.c_double), ('epsilon', ctypes.c_double), ('saturation', ctypes.c_double),
                ('dark', ctypes.POINTER(ctypes.c_float)), ('out_dtype', ctypes.c_int), ('out_scale', ctypes.c_double)]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_a_plan_that_ran_a_stack_is_a_fresh_plan(dtype):
    """rl_stack_run on a plan, then an ordinary set_measurement / iterate on the same plan: the bits of a fresh plan.  Destroying the
    stack, then the plan, is clean; so is a sensor pitch wider than the frame."""
    L = _lib()
    psfs = _psfs(1)
    pitch = NX + 5
    sensor = np.zeros((3, 1, NY, pitch), dtype=np.uint16)
    sensor[..., :NX] = _camera_frames(3, 1, 81)
    plan = L.DeconvPlan(psfs, 2, NY, NX, dtype=dtype)
    p = _Params(1, 0, NY, NX, pitch, 0, 0, DARK, GAIN, 1e-9, 65535.0, None, 1, 1.0)
    stack = ctypes.c_void_p()
    L.check(L.lib.rl_stack_create(plan.handle, ctypes.byref(p), ctypes.byref(stack)))
    out, times = np.zeros((3, NY, NX)), np.zeros(4)
    istats, estats = np.zeros((3, 1, 4)), np.zeros((3, 2))
    L.check(L.lib.rl_stack_run(stack, sensor.ctypes.data_as(ctypes.c_void_p), 3, K, out.ctypes.data_as(ctypes.c_void_p), L.ptr(istats), L.ptr(estats),
                               L.ptr(times)))
    meas, stats = ir.measurement(sensor[..., :NX], 1, dark=DARK, gain=GAIN, saturation=65535.0, dtype=NP[dtype])
    assert np.all(times > 0) and times[0] >= times[2]
    assert istats.tobytes() == stats.tobytes() and np.array_equal(estats[:, 0], ir.export(out, 1.0, np.float64)[1][:, 0])
    meas = meas.astype(np.float64)
    other = np.ascontiguousarray(meas[:2][::-1]) * 1.5
    fresh = L.DeconvPlan(psfs, 2, NY, NX, dtype=dtype)
    for q in (plan, fresh):
        q.set_measurement(other)
        q.iterate(K)
    assert plan.estimate().tobytes() == fresh.estimate().tobytes() and plan.unresolved() == fresh.unresolved() == 0
    if dtype == 'f64':
        from rescan_line_sted_amd.line_sted_tools import deconvolve
        assert out.tobytes() == deconvolve(meas, psfs, K, dtype='f64').tobytes()
    L.check(L.lib.rl_stack_run(stack, sensor.ctypes.data_as(ctypes.c_void_p), 3, K, out.ctypes.data_as(ctypes.c_void_p), None, None, None))
    assert L.lib.rl_stack_destroy(stack) == 0
    del plan, fresh
