"""Tiled Richardson-Lucy for images of any size.

An image is cut into overlapping tiles; every tile is a frame of an ordinary DeconvPlan of the tile's shape (zero extension at
the tile border, exactly as the reference extends at the image border); the tile estimates are blended with weights that vanish
in a margin at every interior tile edge.  The measurement is uploaded once; the tiles are cut out (rl_tile_gather) and put
together (rl_tile_blend) on the device.

    estimate, info = deconvolve_tiled(measurement, psfs, iterations)

Plain Richardson-Lucy from ones moves information 2 * hw pixels per iteration (hw = max(py, px) // 2), so with
margin >= exact_margin(psfs, iterations) = 2 * iterations * hw the result IS the whole-image estimate up to rounding.  The
default margin is far smaller: the measured point from which, for the STED PSF sets of figure 2, the deviation from whole-image
Richardson-Lucy is under 1 % of the estimate's own shot-noise scatter (tools/tile_margin_study.py,
profiles/tiled/margin_study.json; INTEGRATION.md section 5g has the table and the sets it does not hold for).  Biggs-Andrews
acceleration, RL-TV and the stopping rules use per-frame sums: on tiles they act per tile.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import DTYPES, RL_F32, check, lib

# Measured (tools/tile_margin_study.py, profiles/tiled/margin_study.json): the smallest multiple of 8 whose K = 20 deviation from
# whole-image Richardson-Lucy stays below 1 % of the shot-noise floor of an estimate for every figure-2 STED set from 2.0x on and
# the 1.5x line set -- with the default overlap and, as a control, at fixed tile origins.  No margin up to 64 reaches that for the 1.5x point set (3 % of the floor at 64) and the two un-depleted 1.0x
# sets, whose wide PSFs carry a tile border far into the tile.  The default overlap leaves a 16-pixel
# ramp between the margins.
DEFAULT_MARGIN = 32
_INT_P = ctypes.POINTER(ctypes.c_int)


def default_overlap(margin):
    return 2 * int(margin) + 16


def _half_width(psfs):
    return max(max(np.shape(p)[-2:]) for p in psfs) // 2


def exact_margin(psfs, iterations):
    """The margin from which `iterations` plain Richardson-Lucy iterations on tiles equal the whole-image result up to rounding:
    2 * iterations * (max(py, px) // 2)."""
    return 2 * int(iterations) * _half_width(psfs)


def default_tile(psfs):
    """512 where 512 + hw fits the 576-point transform (the fastest kernels), otherwise the largest tile that fits the transform
    length 512 + hw selects."""
    hw = _half_width(psfs)
    if 512 + hw <= 576:
        return 512
    length = lib.rl_fft_length_for(512 + hw)
    if not length:
        raise ValueError('a PSF of half width %d fits no built transform length' % hw)
    return length - hw


def _pair(v, name):
    if np.isscalar(v):
        return int(v), int(v)
    v = tuple(int(x) for x in v)
    if len(v) != 2:
        raise ValueError('%s: one number or (y, x)' % name)
    return v


def _ints(a):
    return a.ctypes.data_as(_INT_P)


class TileLayout:
    """The tiles of a (NY, NX) image and their blend weights (include/rlsted.h rl_tile_axis, rl_tile_weights).  tile, overlap: one
    number or (y, x); 0 <= margin, 2 * margin < overlap < tile.  An axis no longer than the tile is one tile of the axis' length.
    origins_y, origins_x: int32 arrays; tile_shape (ty, tx); weights_y [len(origins_y)][ty], weights_x [len(origins_x)][tx]:
    normalised float64 weights, the weight of tile (iy, ix) at (j, i) is weights_y[iy][j] * weights_x[ix][i]."""

    def __init__(self, shape, tile, overlap, margin):
        self.shape = _pair(shape, 'shape')
        self.tile, self.overlap, self.margin = _pair(tile, 'tile'), _pair(overlap, 'overlap'), int(margin)
        axes = []
        for ax in (0, 1):
            n, t, o = self.shape[ax], self.tile[ax], self.overlap[ax]
            if self.margin < 0 or 2 * self.margin >= o:
                raise ValueError('the margin must satisfy 0 <= margin and 2 * margin < overlap; got margin %d, overlap %d' % (self.margin, o))
            count = ctypes.c_int()
            try:
                check(lib.rl_tile_axis(n, t, o, ctypes.byref(count), None))
                origins = np.zeros(count.value, dtype=np.intc)
                check(lib.rl_tile_axis(n, t, o, ctypes.byref(count), _ints(origins)))
                te = min(n, t)
                w = np.empty((count.value, te), dtype=np.float64)
                check(lib.rl_tile_weights(n, t, o, self.margin, count.value, _ints(origins), _lib.ptr(w), None, None))
            except _lib.RlstedError as e:
                raise ValueError(str(e)) from None
            axes.append((origins, te, w))
        (self.origins_y, ty, self.weights_y), (self.origins_x, tx, self.weights_x) = axes
        self.tile_shape = (ty, tx)

    @property
    def tiles_per_frame(self):
        return len(self.origins_y) * len(self.origins_x)

    def slots(self, frames):
        """(frames * tiles_per_frame, 3) int32 rows (frame, a_y, a_x): frame-major, then iy, then ix -- the order of the tile store."""
        f, ay, ax = np.meshgrid(np.arange(int(frames)), self.origins_y, self.origins_x, indexing='ij')
        return np.ascontiguousarray(np.stack([f.ravel(), ay.ravel(), ax.ravel()], axis=1), dtype=np.intc)


class TiledResult:
    """The blended estimates (F, NY, NX) of deconvolve_tiled(keep_on_device=True) in one device buffer of element type `dtype`:
    frame f at element offsets[f].  `dev`, `dtype`, `offsets` and `shape` are what quality.ring_stats_device takes."""

    def __init__(self, ctx, dev, dtype, frames, shape):
        self.ctx, self.dev, self.dtype, self.frames, self.shape = ctx, dev, dtype, int(frames), tuple(shape)
        self.offsets = np.arange(self.frames, dtype=np.int64) * (self.shape[0] * self.shape[1])

    def download(self):
        """(F, NY, NX) float64."""
        out = np.empty((self.frames,) + self.shape, dtype=np.float64)
        check(lib.rl_device_download(self.ctx.handle, self.dev, DTYPES[self.dtype], out.size, _lib.ptr(out)))
        return out

    def free(self):
        if getattr(self, 'dev', None) is not None and lib is not None:
            lib.rl_device_free(self.ctx.handle, self.dev)
            self.dev = None

    __del__ = free


class _Device:
    """What deconvolve_tiled does on the GPU, one method per step (the CPU tests drive the wrapper with a numpy stand-in)."""

    def __init__(self, psfs, batch, tile_shape, dtype, device, acceleration, tv_lambda, tv_epsilon):
        self.dtype, self.code = dtype, DTYPES[dtype]
        self.esize = 4 if self.code == RL_F32 else 8
        self.plan = _lib.DeconvPlan(psfs, batch, tile_shape[0], tile_shape[1], dtype=dtype, device=device, acceleration=acceleration,
                                    tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
        self.ctx = self.plan.ctx
        self.V = self.plan.V
        self.tile_shape = tuple(tile_shape)
        self.meas, self.est = self._plan_ptr(1), self._plan_ptr(0)
        self.owned = []

    def _plan_ptr(self, which):
        p = ctypes.c_void_p()
        check(lib.rl_deconv_device_ptr(self.plan.handle, which, ctypes.byref(p), None, None))
        return p

    def alloc(self, elements):
        p = ctypes.c_void_p()
        check(lib.rl_device_alloc(self.ctx.handle, max(int(elements), 1) * self.esize, ctypes.byref(p)))
        self.owned.append(p)
        return p

    def upload(self, measurement):
        """(F, V, NY, NX) float64 -> device, in the plan's element type, once."""
        self.src_shape = measurement.shape
        self.src = self.alloc(measurement.size)
        check(lib.rl_device_upload(self.ctx.handle, self.src, self.code, measurement.size, _lib.ptr(measurement)))

    def upload_raw(self, raw, camera):
        """(F, V, NY, NX) camera data in its own dtype -> device as it is (rl_device_upload_bytes: no host copy), then ingested ONCE
        (include/rlsted.h rl_ingest) into the full-size image of the plan's element type that gather() reads."""
        from .stack import raw_code
        F, V, NY, NX = self.src_shape = raw.shape

        def narrow(a):
            p = ctypes.c_void_p()
            check(lib.rl_device_alloc(self.ctx.handle, a.nbytes, ctypes.byref(p)))
            self.owned.append(p)
            check(lib.rl_device_upload_bytes(self.ctx.handle, p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
            return p
        raw_dev = narrow(raw)
        dark_dev = None if camera.dark_map is None else narrow(camera.dark_map)
        self.src = self.alloc(raw.size)
        check(lib.rl_ingest(self.ctx.handle, raw_dev, raw_code(raw), F * V, NY, NX, 0, 0, V, 1, F, F, V, NY, NX, dark_dev, camera.dark,
                            camera.gain, camera.epsilon, 0.0 if camera.saturation is None else camera.saturation, self.src, self.code, None))
        for p in (raw_dev, dark_dev):
            if p is not None:
                self.owned.remove(p)
                check(lib.rl_device_free(self.ctx.handle, p))      # (waits for the ingest)

    def repair(self, mask, radius):
        """The defect pixels of the whole ingested image, in place (include/rlsted.h rl_repair_pixels)."""
        F, V, NY, NX = self.src_shape
        check(lib.rl_repair_pixels(self.ctx.handle, self.src, self.code, F * V, NY, NX, mask.ctypes.data_as(ctypes.c_void_p), int(radius), None))

    def gather(self, slots):
        F, V, NY, NX = self.src_shape
        check(lib.rl_tile_gather(self.ctx.handle, self.src, self.code, F, V, NY, NX, _ints(slots), len(slots), self.tile_shape[0],
                                 self.tile_shape[1], self.meas, self.code))
        self.plan.measurement_written()

    def iterate(self, iterations, until):
        if until is None:
            self.plan.iterate(iterations)
            return None
        return self.plan.iterate_until(iterations, **until)['iterations']

    def store(self, store, first, count):
        """The estimates of the chunk's first `count` frames -> tiles [first, first + count) of the store."""
        n = self.tile_shape[0] * self.tile_shape[1] * self.esize
        check(lib.rl_device_copy(self.ctx.handle, ctypes.c_void_p(store.value + first * n), self.est, count * n))

    def blend(self, store, layout, frames, out):
        NY, NX = layout.shape
        check(lib.rl_tile_blend(self.ctx.handle, store, self.code, frames, NY, NX, len(layout.origins_y), len(layout.origins_x),
                                layout.tile_shape[0], layout.tile_shape[1], _ints(layout.origins_y), _ints(layout.origins_x),
                                _lib.ptr(layout.weights_y), _lib.ptr(layout.weights_x), out, self.code))

    def result(self, out, frames, shape):
        self.owned.remove(out)
        return TiledResult(self.ctx, out, self.dtype, frames, shape)

    def unresolved(self):
        return self.plan.unresolved()

    def strategy(self):
        return self.plan.strategy()

    def close(self):
        for p in self.owned:
            lib.rl_device_free(self.ctx.handle, p)
        self.owned = []


def deconvolve_tiled(measurement, psfs, iterations, tile=None, overlap=None, margin=None, dtype='f32', device=None, batch=None,
                     acceleration=None, tv_lambda=None, tv_epsilon=0.1, until=None, keep_on_device=False, camera=None):
    """`iterations` Richardson-Lucy iterations on images of any size, tile by tile: measurement (F, V, NY, NX) or (V, NY, NX).
    tile: one number or (y, x) (default_tile(psfs)); margin: pixels at every interior tile edge that do not contribute
    (DEFAULT_MARGIN; exact_margin(psfs, iterations) makes the result the whole-image one up to rounding); overlap: at least this
    many pixels shared by neighbouring tiles, more than 2 * margin (default 2 * margin + 16).  batch: tiles per plan (the tiles of
    all frames are worked through in chunks of `batch`; default: all of them, 32 at most; the result does not depend on it bit for
    bit in f64 and multi-view plans, within the f32 contract where f32 single-view tiles run as frame pairs).  acceleration, tv_lambda, tv_epsilon: as
    for deconvolve, acting per tile.  until: None, or dict(rule=..., threshold=..., check_every=...) -- every tile is stopped by its
    own divergence (DeconvPlan.iterate_until, `iterations` at most).
    Returns (estimate (F, NY, NX) float64, info); info: 'layout' (TileLayout), 'tiles', 'batch', 'chunks', 'unresolved' (the plan's
    count over all tiles), 'strategy' (DeconvPlan.strategy() of the tile plan on the last chunk) and, with until, 'iterations' (F, tiles down, tiles across).  keep_on_device=True: the estimate stays on
    the GPU, a TiledResult (.download(); .dev, .dtype, .offsets, .shape for quality.ring_stats_device).
    camera: None, or a stack.CameraModel -- the measurement is then camera data in its own dtype (uint8, uint16, int16, float32; a
    dark map has the image's shape), uploaded as it is and turned into the measurement on the device, max((raw - dark) * gain, 0)
    + epsilon in float64 rounded once to the plan's element type; camera.defects (a map of the image's
    shape) are repaired on the whole image after the ingest (section 5k), and info gains 'defects' and 'unrepaired'."""
    _lib.tv_params(tv_lambda, tv_epsilon)
    _lib.accel_mode(acceleration)
    if dtype not in DTYPES:
        raise ValueError("dtype must be 'f32' or 'f64'; got %r" % (dtype,))
    if camera is None:
        measurement = np.ascontiguousarray(measurement, dtype=np.float64)
    else:
        from .stack import raw_code
        raw_code(measurement)                                # (ValueError for a dtype that is not taken as it is)
        measurement = np.ascontiguousarray(measurement)
    if measurement.ndim == 3:
        measurement = measurement[None]
    if measurement.ndim != 4 or 0 in measurement.shape:
        raise ValueError('measurement: expected (F, V, NY, NX) or (V, NY, NX); got shape %s' % (measurement.shape,))
    F, V, NY, NX = measurement.shape
    if V != len(psfs):
        raise ValueError('%d views in the measurement, %d PSFs' % (V, len(psfs)))
    if int(iterations) < (0 if until is None else 1):
        raise ValueError('iterations must be at least %d' % (0 if until is None else 1))
    if until is not None:
        until = dict(until)
        if not set(until) <= {'rule', 'threshold', 'check_every'}:
            raise ValueError("until: a dict with the keys 'rule', 'threshold', 'check_every'")
    margin = DEFAULT_MARGIN if margin is None else int(margin)
    layout = TileLayout((NY, NX), default_tile(psfs) if tile is None else tile, default_overlap(margin) if overlap is None else overlap,
                        margin)
    if camera is not None:
        camera.check_window(NY, NX)
    slots = layout.slots(F)
    tiles = len(slots)
    batch = min(tiles, 32) if batch is None else int(batch)
    if batch < 1:
        raise ValueError('batch must be at least 1')
    ty, tx = layout.tile_shape
    dev = _Device(psfs, batch, (ty, tx), dtype, _lib.DEFAULT_DEVICE if device is None else device, acceleration, tv_lambda, tv_epsilon)
    try:
        if camera is None:
            dev.upload(measurement)
        else:
            dev.upload_raw(measurement, camera)
            if camera.defects is not None:
                dev.repair(camera.defects, camera.repair_radius)
        store = dev.alloc(tiles * ty * tx)
        counts = np.zeros(tiles, dtype=np.int64)
        chunks = 0
        for first in range(0, tiles, batch):
            n = min(batch, tiles - first)
            chunk = np.full((batch, 3), (-1, 0, 0), dtype=np.intc)   # a short last chunk: fillers
            chunk[:n] = slots[first:first + n]
            dev.gather(chunk)
            its = dev.iterate(int(iterations), until)
            if its is not None:
                counts[first:first + n] = its[:n]
            dev.store(store, first, n)
            chunks += 1
        out = dev.alloc(F * NY * NX)
        dev.blend(store, layout, F, out)
        info = {'layout': layout, 'tiles': tiles, 'batch': batch, 'chunks': chunks, 'unresolved': dev.unresolved(), 'strategy': dev.strategy()}
        if camera is not None:
            info.update(camera.defect_info())
        if until is not None:
            info['iterations'] = counts.reshape(F, len(layout.origins_y), len(layout.origins_x))
        result = dev.result(out, F, (NY, NX))
        if keep_on_device:
            return result, info
        try:
            return result.download(), info
        finally:
            result.free()
    finally:
        dev.close()

