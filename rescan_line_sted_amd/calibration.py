"""Camera calibration from dark and illuminated stacks, and the repair of known defect pixels (DESIGN.md
section 4m).

Every path for acquired data starts from a stack.CameraModel(dark=..., gain=..., saturation=...); this module makes one.  The stacks
are the largest data the project touches, so their per-pixel mean and variance are formed on the device: the raw frames cross PCIe
in their own type, chunk by chunk, and a kernel adds them to exact 64-bit integer sums (include/rlsted.h rl_calib_accumulate).  The
maps that come back are small; what is done with them -- defect rules, the photon-transfer line -- is numpy.

    camera, report = calibrate_camera(dark_stack, [level_1, level_2, level_3], saturation=65535)
    estimates, info = deconvolve_stack(raw, psfs, 20, camera=camera)      # dark map, gain and defect repair included

Out of scope: per-frame outliers (cosmic rays, pixels saturated in one exposure) -- the in-place repair needs a static mask; per-pixel
gain or flat-field maps -- a microscope's illumination is not uniform, so a flat stack does not separate response from light; read
noise and per-pixel weights inside the Richardson-Lucy iterations.
"""
import ctypes
import time

import numpy as np

from . import _lib
from ._lib import check, lib
from .stack import CameraModel, raw_code

HOT, NOISY, DEAD, INVALID = 1, 2, 4, 8            # the bits of find_defects' reasons map
MAX_INTEGER_FRAMES = 65535                        # an integer accumulator's limit (include/rlsted.h)
DEFAULT_CHUNK_BYTES = 256 << 20


class _Device:
    """What the calibration does on the GPU, one method per step (the CPU tests drive the functions with a numpy stand-in)."""

    def __init__(self, device):
        self.ctx = _lib.Context.get(device, 0)
        self.calib, self.raw, self.raw_bytes, self.owned = None, None, 0, []

    def _alloc(self, nbytes):
        p = ctypes.c_void_p()
        check(lib.rl_device_alloc(self.ctx.handle, max(int(nbytes), 1), ctypes.byref(p)))
        self.owned.append(p)
        return p

    def open(self, code, sensor, window):
        """The accumulators of the window (y0, x0, ny, nx) of sensor frames (sy, sx) of raw type `code` (rl_calib_create)."""
        self.window = window
        h = ctypes.c_void_p()
        check(lib.rl_calib_create(self.ctx.handle, code, sensor[0], sensor[1], window[0], window[1], window[2], window[3], ctypes.byref(h)))
        self.calib = h

    def accumulate(self, frames):
        """A chunk of whole sensor frames, C-contiguous, in its own dtype: uploaded as it is, then added to the sums.  Returns
        (upload_ms, kernel_ms), each waited for."""
        t0 = time.perf_counter()
        if frames.nbytes > self.raw_bytes:
            if self.raw is not None:
                self.owned.remove(self.raw)
                check(lib.rl_device_free(self.ctx.handle, self.raw))
            self.raw, self.raw_bytes = self._alloc(frames.nbytes), frames.nbytes
        check(lib.rl_device_upload_bytes(self.ctx.handle, self.raw, frames.ctypes.data_as(ctypes.c_void_p), frames.nbytes))
        t1 = time.perf_counter()
        check(lib.rl_calib_accumulate(self.calib, self.raw, frames.shape[0]))
        self.ctx.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def sums(self, integer):
        """(S, Q) as they are: int64 and uint64 for the integer raw types, float64 for float32."""
        ny, nx = self.window[2:]
        S, Q = np.empty((ny, nx), dtype=np.int64 if integer else np.float64), np.empty((ny, nx), dtype=np.uint64 if integer else np.float64)
        check(lib.rl_calib_sums(self.calib, S.ctypes.data_as(ctypes.c_void_p), Q.ctypes.data_as(ctypes.c_void_p)))
        return S, Q

    def finalize(self):
        """(mean, var), float64 (ny, nx) (rl_calib_finalize, downloaded)."""
        ny, nx = self.window[2:]
        n = ny * nx
        maps = self._alloc(2 * n * 8)
        var = ctypes.c_void_p(maps.value + n * 8)
        check(lib.rl_calib_finalize(self.calib, maps, var))
        out = np.empty((2, ny, nx))
        check(lib.rl_device_download(self.ctx.handle, maps, _lib.RL_F64, 2 * n, _lib.ptr(out)))
        return out[0].copy(), out[1].copy()

    def repair(self, images, mask, radius):
        """images (n, ny, nx) float32 / float64, C-contiguous: repaired in place through the device (rl_repair_pixels)."""
        n, ny, nx = images.shape
        buf = self._alloc(images.nbytes)
        check(lib.rl_device_upload_bytes(self.ctx.handle, buf, images.ctypes.data_as(ctypes.c_void_p), images.nbytes))
        code = _lib.RL_F32 if images.dtype == np.float32 else _lib.RL_F64
        left = np.zeros(n, dtype=np.int64)
        check(lib.rl_repair_pixels(self.ctx.handle, buf, code, n, ny, nx, mask.ctypes.data_as(ctypes.c_void_p), int(radius),
                                   left.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        wide = np.empty(images.shape)
        check(lib.rl_device_download(self.ctx.handle, buf, code, images.size, _lib.ptr(wide)))     # (f32 widens exactly)
        images[...] = wide
        return left

    def close(self):
        if self.calib is not None:
            lib.rl_calib_destroy(self.calib)
            self.calib = None
        for p in self.owned:
            lib.rl_device_free(self.ctx.handle, p)
        self.owned, self.raw, self.raw_bytes = [], None, 0


def temporal_stats(raw, roi=None, chunk_frames=None, device=None):
    """Per-pixel mean and variance over the frames of a raw stack, formed on the device.  raw: (..., sy, sx) of uint8, uint16, int16
    or float32, taken as it is (anything else: ValueError); the leading axes are flattened to frames.  roi: (y0, x0, ny, nx), the
    window of the sensor (default: all of it).  chunk_frames: frames per upload (default: about 256 MB).
    Integer types: exact 64-bit integer sums, at most 65535 frames; mean = S / F and the unbiased var = (F Q - S^2) / (F (F - 1)),
    each rounded from exact integers -- the result does not depend on chunk_frames.  float32: float64 sums in frame order.  F = 1
    gives var = 0.
    Returns (mean, var, info), float64 (ny, nx) maps; info: 'frames', 'chunks', 'chunk_frames', 'nonfinite' (pixels whose statistics
    are not finite: float32 input with nan or inf) and 'times' (wall_ms, upload_ms, kernel_ms)."""
    code = raw_code(raw)
    raw = np.ascontiguousarray(raw)
    if raw.ndim < 2 or 0 in raw.shape:
        raise ValueError('raw: expected (..., sy, sx) with at least one frame; got shape %s' % (raw.shape,))
    sy, sx = raw.shape[-2:]
    frames = raw.reshape(-1, sy, sx)
    F = frames.shape[0]
    integer = raw.dtype != np.float32
    if integer and F > MAX_INTEGER_FRAMES:
        raise ValueError('at most %d frames of an integer type in one accumulator; got %d' % (MAX_INTEGER_FRAMES, F))
    y0, x0, ny, nx = (0, 0, sy, sx) if roi is None else (int(v) for v in roi)
    if ny < 1 or nx < 1 or y0 < 0 or x0 < 0 or y0 + ny > sy or x0 + nx > sx:
        raise ValueError('roi %s overhangs the %d x %d sensor frame' % ((y0, x0, ny, nx), sy, sx))
    if chunk_frames is None:
        chunk_frames = max(1, DEFAULT_CHUNK_BYTES // (sy * sx * raw.dtype.itemsize))
    chunk_frames = int(chunk_frames)
    if chunk_frames < 1:
        raise ValueError('chunk_frames must be at least 1')
    chunk_frames = min(chunk_frames, F)
    t0 = time.perf_counter()
    dev = _Device(_lib.DEFAULT_DEVICE if device is None else device)
    try:
        dev.open(code, (sy, sx), (y0, x0, ny, nx))
        up_ms = k_ms = 0.0
        for first in range(0, F, chunk_frames):
            u, k = dev.accumulate(frames[first:first + chunk_frames])
            up_ms, k_ms = up_ms + u, k_ms + k
        mean, var = dev.finalize()
    finally:
        dev.close()
    info = {'frames': F, 'chunks': -(-F // chunk_frames), 'chunk_frames': chunk_frames,
            'nonfinite': int(np.count_nonzero(~(np.isfinite(mean) & np.isfinite(var)))),
            'times': {'wall_ms': (time.perf_counter() - t0) * 1e3, 'upload_ms': up_ms, 'kernel_ms': k_ms}}
    return mean, var, info


def _maps(stats, name):
    mean, var = np.asarray(stats[0], dtype=np.float64), np.asarray(stats[1], dtype=np.float64)
    if mean.ndim != 2 or mean.shape != var.shape or mean.size == 0:
        raise ValueError('%s: expected (mean, var), two (ny, nx) maps; got shapes %s, %s' % (name, mean.shape, var.shape))
    return mean, var


def _median(values):
    values = values[np.isfinite(values)]
    return float(np.median(values)) if values.size else float('nan')


def find_defects(dark_stats, top_stats=None, hot_sigma=8.0, hot_min=1.0, noisy_factor=4.0, dead_fraction=0.1):
    """The defect pixels of a sensor window from its temporal statistics.  dark_stats, top_stats: (mean, var[, ...]) as temporal_stats
    returns them, of a dark stack and -- optionally -- of the brightest level of an illuminated one.
      hot      dark_mean - median(dark_mean) > max(hot_sigma * 1.4826 * MAD(dark_mean), hot_min)
      noisy    dark_var > noisy_factor * median(dark_var)
      dead     (with top_stats) signal < dead_fraction * median(signal),  signal = top_mean - dark_mean
      invalid  any statistic that is not finite
    Medians and the MAD are taken over the finite values.  Returns (mask, reasons): a boolean (ny, nx) map for
    CameraModel(defects=...) and a uint8 map of the bits HOT = 1, NOISY = 2, DEAD = 4, INVALID = 8."""
    dm, dv = _maps(dark_stats, 'dark_stats')
    reasons = np.zeros(dm.shape, dtype=np.uint8)
    invalid = ~(np.isfinite(dm) & np.isfinite(dv))
    with np.errstate(invalid='ignore'):
        med = _median(dm)
        mad = _median(np.abs(dm - med))
        reasons[dm - med > max(float(hot_sigma) * 1.4826 * mad, float(hot_min))] |= HOT
        reasons[dv > float(noisy_factor) * _median(dv)] |= NOISY
        if top_stats is not None:
            tm, tv = _maps(top_stats, 'top_stats')
            if tm.shape != dm.shape:
                raise ValueError('top_stats maps are %s, dark_stats maps %s' % (tm.shape, dm.shape))
            invalid |= ~(np.isfinite(tm) & np.isfinite(tv))
            signal = tm - dm
            reasons[signal < float(dead_fraction) * _median(signal)] |= DEAD
    reasons[invalid] |= INVALID
    return reasons != 0, reasons


def photon_transfer(dark_stats, level_stats, mask, saturation=None, bins=32, min_count=16):
    """The photon-transfer line of a camera: variance against signal over the good pixels of several brightness levels of a static
    scene.  level_stats: a list of (mean, var[, ...]); mask: the defect map (True = left out).  Per good pixel and level
    s = mean - dark_mean and e = var - dark_var; pairs with mean >= 0.9 * saturation or a non-finite value are dropped; the rest
    are binned in `bins` equal bins of s over [0, max s]; bins with fewer than min_count pairs (or a mean e <= 0) are dropped; a
    straight line e = a + b s goes through the bin means (s_b, e_b) with weights n_b / e_b^2.  Shot noise gives b = 1 / gain.
    Returns {'gain' (photons per count: CameraModel.gain), 'a', 'b', 'read_noise' (sqrt(median dark_var), counts), 'signal',
    'variance', 'count' (the binned curve), 'residual' (the largest |e_b - (a + b s_b)| / (a + b s_b): the linearity figure), 'pairs'}."""
    dm, dv = _maps(dark_stats, 'dark_stats')
    good = ~np.asarray(mask, dtype=bool)
    if good.shape != dm.shape:
        raise ValueError('mask is %s, the maps %s' % (good.shape, dm.shape))
    s_all, e_all = [], []
    for k, st in enumerate(level_stats):
        m, v = _maps(st, 'level_stats[%d]' % k)
        if m.shape != dm.shape:
            raise ValueError('level_stats[%d] maps are %s, dark_stats maps %s' % (k, m.shape, dm.shape))
        keep = good & np.isfinite(m) & np.isfinite(v) & np.isfinite(dm) & np.isfinite(dv)
        if saturation is not None:
            keep &= m < 0.9 * float(saturation)
        s_all.append((m - dm)[keep])
        e_all.append((v - dv)[keep])
    s, e = (np.concatenate(a) if a else np.zeros(0) for a in (s_all, e_all))
    pos = s >= 0.0
    s, e = s[pos], e[pos]
    if s.size == 0 or not s.max() > 0.0:
        raise ValueError('no pixel with a positive signal is left for the photon-transfer line')
    bins = int(bins)
    idx = np.minimum((s / s.max() * bins).astype(np.int64), bins - 1)
    n = np.bincount(idx, minlength=bins).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        sb, eb = np.bincount(idx, weights=s, minlength=bins) / n, np.bincount(idx, weights=e, minlength=bins) / n
    keep = (n >= int(min_count)) & (eb > 0.0)
    if np.count_nonzero(keep) < 2:
        raise ValueError('fewer than two bins with %d pairs: the line needs at least two brightness levels' % int(min_count))
    sb, eb, n = sb[keep], eb[keep], n[keep]
    w = n / (eb * eb)
    W, Sx, Sy, Sxx, Sxy = w.sum(), (w * sb).sum(), (w * eb).sum(), (w * sb * sb).sum(), (w * sb * eb).sum()
    b = (W * Sxy - Sx * Sy) / (W * Sxx - Sx * Sx)
    a = (Sy - b * Sx) / W
    if not b > 0.0:
        raise ValueError('the variance does not grow with the signal (slope %g): no gain' % b)
    fit = a + b * sb
    return {'gain': 1.0 / b, 'a': float(a), 'b': float(b), 'read_noise': float(np.sqrt(max(_median(dv[good]), 0.0))), 'signal': sb,
            'variance': eb, 'count': n.astype(np.int64), 'residual': float(np.max(np.abs(eb - fit) / fit)), 'pairs': int(s.size)}


_DEFECT_RULES = ('hot_sigma', 'hot_min', 'noisy_factor', 'dead_fraction')
_TRANSFER_RULES = ('bins', 'min_count')


def calibrate_camera(dark, levels, roi=None, saturation=None, repair_radius=3, chunk_frames=None, device=None, **rules):
    """A CameraModel from calibration stacks.  dark: one raw stack taken without light; levels: a list of raw stacks of a static
    scene at different brightness (at least two); all of the same sensor shape, any of the raw dtypes.  roi, chunk_frames, device: as
    for temporal_stats -- the model is that of the window.  saturation: the raw level of a saturated pixel, if known.  rules: the
    keywords of find_defects (hot_sigma, hot_min, noisy_factor, dead_fraction) and of photon_transfer (bins, min_count).
    Returns (camera, report).  camera: CameraModel(dark=the dark map as float32 in window coordinates (the median at pixels without
    a finite one), gain=photons per count from the photon-transfer line, saturation=saturation, defects=the defect map,
    repair_radius=repair_radius).  report: 'dark_mean', 'dark_var', 'levels' (the (mean, var) of each), 'top' (index of the
    brightest), 'mask', 'reasons', 'defects' (count), 'transfer' (photon_transfer's dict), 'gain', 'read_noise', 'frames'."""
    unknown = set(rules) - set(_DEFECT_RULES) - set(_TRANSFER_RULES)
    if unknown:
        raise TypeError('calibrate_camera: unknown keyword(s) %s' % ', '.join(sorted(unknown)))
    levels = list(levels)
    if len(levels) < 2:
        raise ValueError('levels: at least two stacks of different brightness')
    dm, dv, dinfo = temporal_stats(dark, roi=roi, chunk_frames=chunk_frames, device=device)
    stats, frames = [], [dinfo['frames']]
    for lv in levels:
        m, v, li = temporal_stats(lv, roi=roi, chunk_frames=chunk_frames, device=device)
        if m.shape != dm.shape:
            raise ValueError('a level stack gives maps of %s, the dark stack %s' % (m.shape, dm.shape))
        stats.append((m, v))
        frames.append(li['frames'])
    top = int(np.argmax([_median(m) for m, _ in stats]))
    mask, reasons = find_defects((dm, dv), stats[top], **{k: v for k, v in rules.items() if k in _DEFECT_RULES})
    transfer = photon_transfer((dm, dv), stats, mask, saturation=saturation, **{k: v for k, v in rules.items() if k in _TRANSFER_RULES})
    dark_map = np.where(np.isfinite(dm), dm, _median(dm)).astype(np.float32)
    camera = CameraModel(dark=dark_map, gain=transfer['gain'], saturation=saturation, defects=mask, repair_radius=repair_radius)
    report = {'dark_mean': dm, 'dark_var': dv, 'levels': stats, 'top': top, 'mask': mask, 'reasons': reasons,
              'defects': int(np.count_nonzero(mask)), 'transfer': transfer, 'gain': transfer['gain'], 'read_noise': transfer['read_noise'],
              'frames': frames}
    return camera, report


def _check_mask(mask, shape, radius):
    mask = np.asarray(mask)
    if mask.dtype != np.bool_ or mask.shape != tuple(shape):
        raise ValueError('mask: a boolean map of shape %s; got %s of shape %s' % (tuple(shape), mask.dtype, mask.shape))
    if int(radius) != radius or not 1 <= int(radius) <= 3:
        raise ValueError('radius must be 1, 2 or 3; got %r' % (radius,))
    return np.ascontiguousarray(mask).view(np.uint8), int(radius)


def unrepairable(mask, radius=3):
    """The defects of a (ny, nx) map (bool, or uint8 with nonzero = defect) that have no good pixel within Chebyshev distance
    `radius`: the repair leaves them as they are."""
    bad = np.asarray(mask) != 0
    ny, nx = bad.shape
    r = int(radius)
    good = np.zeros((ny + 2 * r, nx + 2 * r), dtype=bool)
    good[r:r + ny, r:r + nx] = ~bad
    near = np.zeros((ny, nx), dtype=bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            near |= good[dy:dy + ny, dx:dx + nx]
    return bad & ~near


def repair_defects(images, mask, radius=3, device=None):
    """The defect pixels of host images replaced by the median of their good neighbours, through the device (include/rlsted.h
    rl_repair_pixels states the rule).  images: (..., ny, nx); float32 stays float32, anything else is taken as float64.  mask: a
    boolean (ny, nx) map; radius 1 .. 3.  Returns the repaired copy; pixels of unrepairable(mask, radius) keep their values."""
    images = np.asarray(images)
    if images.ndim < 2 or 0 in images.shape:
        raise ValueError('images: expected (..., ny, nx); got shape %s' % (images.shape,))
    out = np.array(images, dtype=np.float32 if images.dtype == np.float32 else np.float64, order='C')      # (a copy)
    mask8, radius = _check_mask(mask, out.shape[-2:], radius)
    dev = _Device(_lib.DEFAULT_DEVICE if device is None else device)
    try:
        dev.repair(out.reshape((-1,) + out.shape[-2:]), mask8, radius)
    finally:
        dev.close()
    return out
