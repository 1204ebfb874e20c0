"""Richardson-Lucy on acquired camera stacks.

Cameras deliver uint16; np_tif.tif_to_array returns the file's own dtype.  deconvolve_stack takes such a stack as it is: the raw
frames cross PCIe in their own type, a kernel turns them into the plan's measurement on the device (dark level, gain, window, view
order: include/rlsted.h rl_ingest), a second one narrows the estimates before they come back (rl_export), and rl_stack_run
overlaps upload, iterations and download across chunks of the plan's batch.

    estimates, info = deconvolve_stack(raw, psfs, iterations, camera=CameraModel(dark=100.0, gain=0.46))
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import DTYPES, check, lib

RAW_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2, np.dtype(np.float32): 3}      # RL_RAW_*
OUT_DTYPES = {'f32': (0, np.float32), 'float32': (0, np.float32), 'f64': (1, np.float64), 'float64': (1, np.float64),
              'u16': (2, np.uint16), 'uint16': (2, np.uint16)}                                                    # RL_OUT_*
ORDERS = {'frame-view': 0, 'view-frame': 1}                                                                       # RL_ORDER_*
INGEST_FIELDS, EXPORT_FIELDS = 4, 2


class CameraModel:
    """What turns a sensor's numbers into photons: measurement = max((raw - dark) * gain, 0) + epsilon, formed in float64 on the
    device.  dark: one level, or a (ny, nx) map in the coordinates of the window that is deconvolved (kept as float32); gain:
    photons per count, positive; saturation: None, or the raw level from which a pixel is counted as saturated; epsilon: what
    load_data_from_tif adds (1e-9), at least 0.  defects: None, or a boolean (ny, nx) map in window coordinates of the pixels whose
    ingested values are replaced by the median of their good neighbours within repair_radius (1 .. 3) before the iterations
    (include/rlsted.h rl_repair_pixels; calibration.find_defects makes such a map)."""

    def __init__(self, dark=0.0, gain=1.0, saturation=None, epsilon=1e-9, defects=None, repair_radius=3):
        if np.ndim(dark) == 0:
            self.dark, self.dark_map = float(dark), None
            if not np.isfinite(self.dark):
                raise ValueError('dark must be finite; got %r' % (dark,))
        else:
            self.dark, self.dark_map = 0.0, np.ascontiguousarray(dark, dtype=np.float32)
            if self.dark_map.ndim != 2 or self.dark_map.size == 0:
                raise ValueError('dark: one level or a (ny, nx) map; got shape %s' % (self.dark_map.shape,))
        self.gain, self.epsilon = float(gain), float(epsilon)
        self.saturation = None if saturation is None else float(saturation)
        if not (self.gain > 0.0 and np.isfinite(self.gain)):
            raise ValueError('gain must be positive and finite; got %r' % (gain,))
        if not (self.epsilon >= 0.0 and np.isfinite(self.epsilon)):
            raise ValueError('epsilon must be finite and at least 0; got %r' % (epsilon,))
        if self.saturation is not None and not self.saturation > 0.0:
            raise ValueError('saturation must be None or positive; got %r' % (saturation,))
        self.defects, self.repair_radius = None, int(repair_radius)
        if defects is not None:
            defects = np.asarray(defects)
            if defects.dtype != np.bool_ or defects.ndim != 2 or defects.size == 0:
                raise ValueError('defects: None or a boolean (ny, nx) map; got %s of shape %s' % (defects.dtype, defects.shape))
            self.defects = np.ascontiguousarray(defects).view(np.uint8)
        if self.repair_radius != repair_radius or not 1 <= self.repair_radius <= 3:
            raise ValueError('repair_radius must be 1, 2 or 3; got %r' % (repair_radius,))

    def defect_info(self):
        """{'defects', 'unrepaired'} of the window: how many pixels the map names and how many of them have no good pixel within
        repair_radius (they stay as they are); both 0 without a map."""
        if self.defects is None:
            return {'defects': 0, 'unrepaired': 0}
        from .calibration import unrepairable
        return {'defects': int(np.count_nonzero(self.defects)), 'unrepaired': int(np.count_nonzero(unrepairable(self.defects, self.repair_radius)))}

    def check_window(self, ny, nx):
        if self.defects is not None and self.defects.shape != (ny, nx):
            raise ValueError('the defect map is %s, the deconvolved window %s' % (self.defects.shape, (ny, nx)))
        if self.dark_map is not None and self.dark_map.shape != (ny, nx):
            raise ValueError('the dark map is %s, the deconvolved window %s' % (self.dark_map.shape, (ny, nx)))


def raw_code(a):
    """RL_RAW_* of an array's dtype; ValueError for anything a camera path does not take as it is."""
    try:
        return RAW_DTYPES[np.asarray(a).dtype]
    except KeyError:
        raise ValueError('raw data must be uint8, uint16, int16 or float32 (taken without conversion); got %s' % np.asarray(a).dtype) from None


class _Params(ctypes.Structure):      # rl_stack_params of include/rlsted.h
    _fields_ = [('raw_dtype', ctypes.c_int), ('order', ctypes.c_int), ('src_ny', ctypes.c_int), ('src_nx', ctypes.c_int),
                ('src_pitch', ctypes.c_int), ('y0', ctypes.c_int), ('x0', ctypes.c_int), ('offset', ctypes.c_double),
                ('gain', ctypes.c_double), ('epsilon', ctypes.c_double), ('saturation', ctypes.c_double),
                ('dark', ctypes.POINTER(ctypes.c_float)), ('out_dtype', ctypes.c_int), ('out_scale', ctypes.c_double)]


class _Device:
    """What deconvolve_stack does on the GPU, one method per step (the CPU tests drive the wrapper with a numpy stand-in)."""

    def __init__(self, psfs, batch, shape, dtype, device, acceleration, tv_lambda, tv_epsilon):
        self.plan = _lib.DeconvPlan(psfs, batch, shape[0], shape[1], dtype=dtype, device=device, acceleration=acceleration,
                                    tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
        self.stack = None

    def open(self, raw_dtype, order, sensor, origin, camera, out_dtype, out_scale):
        """The pipeline of the plan: sensor (src_ny, src_nx), origin (y0, x0) of the plan's window, codes as in include/rlsted.h."""
        p = _Params(raw_dtype, order, sensor[0], sensor[1], sensor[1], origin[0], origin[1], camera.dark, camera.gain, camera.epsilon,
                    0.0 if camera.saturation is None else camera.saturation,
                    None if camera.dark_map is None else camera.dark_map.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out_dtype,
                    float(out_scale))
        h = ctypes.c_void_p()
        check(lib.rl_stack_create(self.plan.handle, ctypes.byref(p), ctypes.byref(h)))
        self.stack = h

    def set_defects(self, mask, radius):
        """The defect map (uint8, the plan's window) whose pixels every chunk repairs after its ingest (rl_stack_set_defects)."""
        check(lib.rl_stack_set_defects(self.stack, mask.ctypes.data_as(ctypes.c_void_p), int(radius)))

    def run(self, raw, frames, iterations, out, ingest_stats, export_stats, times):
        """All frames through the plan, chunk by chunk (rl_stack_run): fills out, the statistics and the four times."""
        check(lib.rl_stack_run(self.stack, raw.ctypes.data_as(ctypes.c_void_p), frames, iterations, out.ctypes.data_as(ctypes.c_void_p),
                               _lib.ptr(ingest_stats), _lib.ptr(export_stats), _lib.ptr(times)))

    def run_registered(self, raw, frames, iterations, params, given, out, ingest_stats, export_stats, register_out, times):
        """All frames through the plan with the registration in front (rl_stack_run_registered): params an rl_stack_register,
        given None or (F, V, 2) float64, register_out an rl_stack_register_out; fills out, the statistics and the five times."""
        check(lib.rl_stack_run_registered(self.stack, raw.ctypes.data_as(ctypes.c_void_p), frames, iterations, ctypes.byref(params),
                                          None if given is None else _lib.ptr(given), out.ctypes.data_as(ctypes.c_void_p),
                                          _lib.ptr(ingest_stats), _lib.ptr(export_stats), ctypes.byref(register_out), _lib.ptr(times)))

    def unresolved(self):
        return self.plan.unresolved()

    def strategy(self):
        return self.plan.strategy()

    def close(self):
        if self.stack is not None:
            lib.rl_stack_destroy(self.stack)
            self.stack = None


def _stack_shape(raw, views, order):
    """(F, sensor rows, sensor columns) of a raw stack: (F, V, sy, sx) in 'frame-view' order, (V, F, sy, sx) in 'view-frame' order,
    (F, sy, sx) for one view."""
    if raw.ndim == 3 and views == 1:
        return raw.shape
    if raw.ndim != 4:
        raise ValueError('raw: expected (F, V, sy, sx), (V, F, sy, sx) or, for one view, (F, sy, sx); got shape %s' % (raw.shape,))
    F, V = (raw.shape[0], raw.shape[1]) if order == 'frame-view' else (raw.shape[1], raw.shape[0])
    if V != views:
        raise ValueError('%d views in the stack, %d PSFs' % (V, views))
    return (F,) + raw.shape[2:]


def deconvolve_stack(raw, psfs, iterations, camera=None, order='frame-view', roi=None, dtype='f32', out_dtype='f32', out_scale=1.0,
                     batch=None, device=None, acceleration=None, tv_lambda=None, tv_epsilon=0.1, out=None):
    """`iterations` Richardson-Lucy iterations from ones on every frame of an acquired stack.  raw: uint8, uint16, int16 or float32,
    taken as it is (anything else: ValueError), (F, V, sy, sx) for order='frame-view', (V, F, sy, sx) for 'view-frame' (what
    record_data writes), (F, sy, sx) for one view.  camera: a CameraModel (default: dark 0, gain 1).  roi: (y0, x0, ny, nx), the
    window of the sensor that is deconvolved (default: all of it).  dtype: the plan's arithmetic, 'f32' or 'f64'.  out_dtype: 'f32',
    'f64' or 'u16' -- estimate * out_scale, rounded once; 'u16' rounds half to even, clamps to 0 .. 65535 and counts what exceeded
    65535.  batch: frames per chunk (default: all, 256 at most).  acceleration, tv_lambda, tv_epsilon: as for deconvolve, per frame.
    out: a C-contiguous (F, ny, nx) array of out_dtype to fill (pinned_empty(...) is copied to directly).
    Returns (estimates (F, ny, nx), info); info: 'saturated', 'clipped', 'invalid' (F, V) pixel counts of the ingest, 'level' (F, V)
    the sums of the measurement, 'clamped' (F,) and 'flux' (F,) the count of clamped pixels and the sum of each estimate,
    'unresolved', 'strategy' (the plan's, on the last chunk), 'chunks', 'batch' and 'times' (wall_ms, upload_ms, compute_ms,
    download_ms of rl_stack_run), 'defects' and 'unrepaired' (the camera's defect map: pixels named, pixels left as they are).  With
    camera.defects every chunk's ingested images are repaired on the device before the iterations; the ingest statistics stay those
    of the ingest."""
    _lib.tv_params(tv_lambda, tv_epsilon)
    _lib.accel_mode(acceleration)
    if dtype not in DTYPES:
        raise ValueError("dtype must be 'f32' or 'f64'; got %r" % (dtype,))
    if out_dtype not in OUT_DTYPES:
        raise ValueError("out_dtype must be 'f32', 'f64' or 'u16'; got %r" % (out_dtype,))
    if order not in ORDERS:
        raise ValueError("order must be 'frame-view' or 'view-frame'; got %r" % (order,))
    code = raw_code(raw)
    raw = np.ascontiguousarray(raw)                     # (the same dtype: no conversion)
    if 0 in raw.shape:
        raise ValueError('raw is empty: shape %s' % (raw.shape,))
    F, sy, sx = _stack_shape(raw, len(psfs), order)
    y0, x0, ny, nx = (0, 0, sy, sx) if roi is None else (int(v) for v in roi)
    if ny < 1 or nx < 1 or y0 < 0 or x0 < 0 or y0 + ny > sy or x0 + nx > sx:
        raise ValueError('roi %s overhangs the %d x %d sensor frame' % ((y0, x0, ny, nx), sy, sx))
    if int(iterations) < 0:
        raise ValueError('iterations must be at least 0')
    camera = CameraModel() if camera is None else camera
    camera.check_window(ny, nx)
    batch = min(F, 256) if batch is None else int(batch)
    if batch < 1:
        raise ValueError('batch must be at least 1')
    out_code, out_np = OUT_DTYPES[out_dtype]
    if out is None:
        out = np.empty((F, ny, nx), dtype=out_np)
    elif out.dtype != out_np or not out.flags.c_contiguous or out.shape != (F, ny, nx):
        raise ValueError('out must be a C-contiguous %s array of shape %s' % (np.dtype(out_np).name, (F, ny, nx)))
    V = len(psfs)
    dev = _Device(psfs, batch, (ny, nx), dtype, _lib.DEFAULT_DEVICE if device is None else device, acceleration, tv_lambda, tv_epsilon)
    try:
        dev.open(code, ORDERS[order], (sy, sx), (y0, x0), camera, out_code, out_scale)
        if camera.defects is not None:
            dev.set_defects(camera.defects, camera.repair_radius)
        ingest_stats, export_stats, times = np.zeros((F, V, INGEST_FIELDS)), np.zeros((F, EXPORT_FIELDS)), np.zeros(4)
        dev.run(raw, F, int(iterations), out, ingest_stats, export_stats, times)
        info = {'level': ingest_stats[:, :, 0].copy(), 'clipped': ingest_stats[:, :, 1].astype(np.int64),
                'saturated': ingest_stats[:, :, 2].astype(np.int64), 'invalid': ingest_stats[:, :, 3].astype(np.int64),
                'flux': export_stats[:, 0].copy(), 'clamped': export_stats[:, 1].astype(np.int64),
                'unresolved': dev.unresolved(), 'strategy': dev.strategy(), 'chunks': -(-F // batch), 'batch': batch,
                'times': dict(zip(('wall_ms', 'upload_ms', 'compute_ms', 'download_ms'), times.tolist()))}
        info.update(camera.defect_info())
        return out, info
    finally:
        dev.close()
