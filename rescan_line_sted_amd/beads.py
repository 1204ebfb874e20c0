"""Per-view PSFs measured from bead stacks on the device.

On a rescan line-STED instrument every view's PSF differs from the model (depletion alignment, line orientation, aberrations), and
multi-view Richardson-Lucy multiplies every view's back-projection, so one wrong PSF biases the whole estimate.  measure_psfs images
sub-resolution beads and averages them: the camera stack is ingested on the device (rl_ingest), the beads are found on the full
frames (rl_find_peaks, the one new kernel), cut out (rl_tile_gather), aligned to their view's mean with the registration's estimate
and one-interpolation shift (rl_register_estimate, rl_shift_images) and averaged (rl_ensemble_stats).  The result is what
deconvolve_stack takes as psfs.

    psfs, info = measure_psfs(raw, 21, camera=CameraModel(dark=100.0, gain=0.46))
    estimates, _ = deconvolve_stack(raw_sample, psfs, 20, camera=...)
"""
import ctypes

import numpy as np

from . import _lib, registration
from ._lib import DTYPES, check, lib
from .psf import get_width
from .stack import INGEST_FIELDS, ORDERS, CameraModel, raw_code

PEAK_LEVELS = 3                     # rl_find_peaks
MAX_H = 16                          # the largest stencil half width
MAX_RADIUS = 16                     # the largest suppression radius
REASONS = ('cap', 'separation', 'saturated', 'flat', 'at_limit', 'ncc')
_I64P = ctypes.POINTER(ctypes.c_int64)
_FWHM = 2.0 * np.sqrt(2.0 * np.log(2.0))


def gaussian_taps(sigma):
    """(w, h): exp(-k^2 / 2 sigma^2) over k = -h .. h, normalised to sum 1, h = int(4 sigma + 0.5) (scipy's truncation)."""
    sigma = float(sigma)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError('sigma must be positive and finite; got %r' % (sigma,))
    h = int(4.0 * sigma + 0.5)
    if h > MAX_H:
        raise ValueError('sigma %g needs a stencil half width of %d > %d' % (sigma, h, MAX_H))
    k = np.arange(-h, h + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum(), h


class _BeadDevice(registration._Device):
    """registration._Device with the three calls of the bead measurement (the CPU tests replace the whole class with a numpy
    stand-in, tests/beads_reference.NumpyDevice)."""

    def find_peaks(self, src, offsets, ny, nx, w, r, b, rel, threshold, cap):
        """rl_find_peaks: ([per image dict(yx (K, 2) int64, s (K,), x (K,))], counts (n,) int64, levels (n, 3))."""
        n = len(offsets)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        yx = np.zeros((n, cap, 2), dtype=np.int32)
        sv, xv = np.zeros((n, cap)), np.zeros((n, cap))
        cnt, lev = np.zeros(n, dtype=np.int64), np.zeros((n, PEAK_LEVELS))
        check(lib.rl_find_peaks(self.ctx.handle, src.ptr, DTYPES[src.dtype], off.ctypes.data_as(_I64P), n, ny, nx, _lib.ptr(w), (len(w) - 1) // 2,
                                int(r), int(b), float(rel), float(threshold), int(cap), yx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                _lib.ptr(sv), _lib.ptr(xv), cnt.ctypes.data_as(_I64P), _lib.ptr(lev)))
        out = []
        for i in range(n):
            k = int(min(cnt[i], cap))
            out.append({'yx': yx[i, :k].astype(np.int64), 's': sv[i, :k].copy(), 'x': xv[i, :k].copy()})
        return out, cnt, lev

    def gather(self, src, n_images, ny, nx, slots, size, dst):
        """rl_tile_gather with V = 1: the size x size windows at slots (image, a_y, a_x) of the n_images images of src into dst."""
        s = np.ascontiguousarray(slots, dtype=np.intc).reshape(-1, 3)
        check(lib.rl_tile_gather(self.ctx.handle, src.ptr, DTYPES[src.dtype], n_images, 1, ny, nx, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                 len(s), size, size, dst.ptr, DTYPES[dst.dtype]))

    def group_stats(self, src, members, group_ptr, n_pixels, mean=None, var=None):
        """rl_ensemble_stats without a truth: the groups' sums [n_groups][6]; mean / var: float64 buffers [n_groups][n_pixels] or None."""
        off = np.ascontiguousarray(members, dtype=np.int64)
        gp = np.ascontiguousarray(group_ptr, dtype=np.int32)
        out = np.zeros((len(gp) - 1, 6))
        check(lib.rl_ensemble_stats(self.ctx.handle, src.ptr, DTYPES[src.dtype], off.ctypes.data_as(_I64P), gp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    len(gp) - 1, None, 0, None, None, int(n_pixels), None if mean is None else mean.ptr,
                                    None if var is None else var.ptr, _lib.ptr(out)))
        return out


_Device = _BeadDevice                 # (the indirection the CPU tests replace)


def _check_finder(sigma, radius, rel_threshold, threshold, max_beads):
    w, h = gaussian_taps(sigma)
    radius, max_beads = int(radius), int(max_beads)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError('radius must lie in 1 .. %d; got %r' % (MAX_RADIUS, radius))
    if max_beads < 1:
        raise ValueError('max_beads must be at least 1')
    if np.isnan(rel_threshold) or np.isnan(threshold):
        raise ValueError('rel_threshold and threshold must not be nan')
    return w, h, radius, max_beads


def find_beads(images, sigma=1.0, radius=3, border=None, rel_threshold=0.2, threshold=0.0, max_beads=4096, device=None):
    """The bright local maxima of Gaussian-smoothed images, on the device (include/rlsted.h rl_find_peaks).  images: (N, ny, nx) or
    (ny, nx), float32 or float64.  s = the image smoothed by the taps of gaussian_taps(sigma), separable, in float64; a pixel at least
    `border` (default and at least h + radius) from every edge is a bead when s there is >= max(threshold, lo + rel_threshold (hi -
    lo)) -- lo, hi the extremes of s over that domain -- and no pixel within `radius` (Chebyshev) beats it: a plateau gives its first
    pixel in row-major order.  Returns ([per image (K, 2) int64 (y, x) in row-major order, the first max_beads], info) with
    info['values'] (s at the beads), 'x' (the image there), 'counts' (N,) the true counts, 'levels' (N, 3) = lo, hi, t."""
    w, h, radius, max_beads = _check_finder(sigma, radius, rel_threshold, threshold, max_beads)
    images, dt = registration._float_images(images, 'images')
    if images.ndim == 2:
        images = images[None]
    if images.ndim != 3 or 0 in images.shape:
        raise ValueError('images: expected (N, ny, nx) or (ny, nx); got shape %s' % (images.shape,))
    N, ny, nx = images.shape
    b = h + radius if border is None else int(border)
    if b < h + radius:
        raise ValueError('border must be at least h + radius = %d; got %d' % (h + radius, b))
    if min(ny, nx) < 2 * b + 1:
        raise ValueError('a %d x %d image leaves no pixel inside a border of %d' % (ny, nx, b))
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        buf = dev.alloc(images.size, dt)
        dev.upload(buf, images)
        found, counts, levels = dev.find_peaks(buf, [i * ny * nx for i in range(N)], ny, nx, w, radius, b, rel_threshold, threshold, max_beads)
        return [f['yx'] for f in found], {'values': [f['s'] for f in found], 'x': [f['x'] for f in found], 'counts': counts, 'levels': levels}
    finally:
        dev.close()


def _stack_views(raw, order):
    """(F, V, sy, sx, frames [F][V] host view of raw) of a bead stack."""
    if raw.ndim == 3:
        return raw.shape[0], 1, raw.shape[1], raw.shape[2], raw[:, None]
    if raw.ndim != 4:
        raise ValueError('raw: expected (F, V, sy, sx), (V, F, sy, sx) or, for one view, (F, sy, sx); got shape %s' % (raw.shape,))
    frames = raw if order == 'frame-view' else raw.transpose(1, 0, 2, 3)
    return frames.shape + (frames,)


def ring_mean(a, width=2):
    """The mean of the outer `width`-pixel ring of a 2-D array, its pixels summed in row-major order from 0.0."""
    a = np.asarray(a, dtype=np.float64)
    m = np.ones(a.shape, dtype=bool)
    m[width:-width, width:-width] = False
    s = 0.0
    for v in a[m]:
        s += float(v)
    return s / int(m.sum())


def centroid_offset(mean, size):
    """(dy, dx): the centroid of max(crop - ring_mean(crop), 0) over the central size x size of a window's mean, minus its centre."""
    W = mean.shape[0]
    c0 = (W - size) // 2
    crop = mean[c0:c0 + size, c0:c0 + size]
    wts = np.maximum(crop - ring_mean(crop), 0.0)
    tot = wts.sum()
    if not tot > 0.0:
        return np.zeros(2)
    k = np.arange(size, dtype=np.float64) - size // 2
    return np.array([(wts.sum(axis=1) * k).sum() / tot, (wts.sum(axis=0) * k).sum() / tot])


def measure_psfs(raw, size, camera=None, order='frame-view', roi=None, sigma=1.0, radius=3, rel_threshold=0.2, threshold=0.0,
                 min_separation=None, max_beads=4096, max_shift=2, passes=2, min_ncc=0.9, margin=None, device=None):
    """One PSF per view from a stack of bead images.  raw, camera, order, roi: as for deconvolve_stack -- (F, V, sy, sx) 'frame-view',
    (V, F, sy, sx) 'view-frame', (F, sy, sx) for one view; uint8, uint16, int16 or float32 taken as they are.  size: the odd side of
    the PSFs.  sigma, radius, rel_threshold, threshold, max_beads: the finder's (find_beads), per image.  Per view, the images on the
    device from ingest to the mean maps:
      1. every image ingested to float64 (rl_ingest);
      2. rl_find_peaks with border b = max(c, h + radius), c = size // 2 + margin (margin default max_shift + 8: the mirrored
         boundary of the shift's spline stays out of the central size x size);
      3. rejected on the host, counted in info['rejected']: 'cap' (past max_beads), 'separation' (another candidate of the same image
         closer than min_separation, Chebyshev, default size: both go), 'saturated' (the raw (2c+1)^2 window reaches
         camera.saturation);
      4. the (2c+1)^2 windows cut out (rl_tile_gather);
      5. reference 0 = the mean of the integer-centred windows (rl_ensemble_stats); `passes` rounds of: every window estimated
         against the reference (rl_register_estimate, max_shift, margin max_shift + 2, refine 1), the ORIGINAL windows shifted by
         the estimate (rl_shift_images, order 3), the new mean.  A window that comes out flat or at_limit leaves the later means
         ('flat', 'at_limit');
      6. centring: the last mean's background-subtracted centroid offset d (centroid_offset) is added to every estimate, and each
         window is interpolated ONCE by that total;
      7. windows with ncc < min_ncc go ('ncc'); the mean and variance of the rest (rl_ensemble_stats);
      8. the central size x size, minus the mean of its outer 2-pixel ring, clipped at 0, normalised to sum 1.
    A view left without beads raises ValueError naming it.  Returns ([V arrays (1, size, size) float64], info): info['positions']
    [V] (K, 3) = (frame, y, x) of the accepted beads' centres in the coordinates of the roi window (the peak plus the applied shift),
    'flux' [V] (K,) = the sum of each accepted window's central size x size minus size^2 times its ring mean, 'ncc' [V], 'n_beads'
    (V,), 'rejected' [V] {reason: count}, 'std' [V] (1, size, size) the standard error of the mean map on the PSF's scale,
    'width' (V, 2) the FWHM along the PSF's central row and column (get_width), 'margin', 'border'.
    Limits: translation only; the centring assumes point-symmetric PSFs; PSFs narrower than about 1 pixel sigma are not served well
    by the spline; single-slice data."""
    size, passes, max_shift = int(size), int(passes), int(max_shift)
    if size < 5 or size % 2 == 0:
        raise ValueError('size must be odd and at least 5; got %r' % (size,))
    if passes < 1:
        raise ValueError('passes must be at least 1')
    if not 1 <= max_shift <= registration.MAX_RADIUS:
        raise ValueError('max_shift must lie in 1 .. %d; got %r' % (registration.MAX_RADIUS, max_shift))
    if order not in ORDERS:
        raise ValueError("order must be 'frame-view' or 'view-frame'; got %r" % (order,))
    w, h, radius, max_beads = _check_finder(sigma, radius, rel_threshold, threshold, max_beads)
    m = max_shift + 8 if margin is None else int(margin)
    if m < max_shift + 2:
        raise ValueError('margin must be at least max_shift + 2 = %d; got %d' % (max_shift + 2, m))
    min_sep = size if min_separation is None else int(min_separation)
    code = raw_code(raw)
    raw = np.ascontiguousarray(raw)
    if 0 in raw.shape:
        raise ValueError('raw is empty: shape %s' % (raw.shape,))
    F, V, sy, sx, frames = _stack_views(raw, order)
    y0, x0, ny, nx = (0, 0, sy, sx) if roi is None else (int(v) for v in roi)
    if ny < 1 or nx < 1 or y0 < 0 or x0 < 0 or y0 + ny > sy or x0 + nx > sx:
        raise ValueError('roi %s overhangs the %d x %d sensor frame' % ((y0, x0, ny, nx), sy, sx))
    camera = CameraModel() if camera is None else camera
    camera.check_window(ny, nx)
    c = size // 2 + m
    W, b, M = 2 * c + 1, max(c, h + radius), max_shift + 2
    if min(ny, nx) < 2 * b + 1:
        raise ValueError('a %d x %d window leaves no pixel inside a border of %d' % (ny, nx, b))
    if W - 2 * M < 8:
        raise ValueError('windows of %d pixels leave no 8 x 8 interior for the estimate inside max_shift + 2: raise size or margin' % W)
    n_pix, img_bytes = ny * nx, sy * sx * raw.dtype.itemsize
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        raw_dev = dev.alloc(F * V * img_bytes, None)
        dev.upload(raw_dev, raw)
        fs, vs = (V, 1) if order == 'frame-view' or V == 1 else (1, F)     # source image f fs + v vs
        imgs, stats = dev.alloc(F * V * n_pix, 'f64'), dev.alloc(F * V * INGEST_FIELDS, 'f64')
        dark = None
        if camera.dark_map is not None:
            dark = dev.alloc(n_pix, 'f32')
            dev.upload(dark, camera.dark_map)
        dev.ingest(raw_dev, code, F * V, (sy, sx), (y0, x0), fs, vs, F, F, V, (ny, nx), camera, dark, imgs, stats)   # -> [F][V][ny][nx]
        if camera.defects is not None:
            dev.repair(imgs, F * V, ny, nx, camera.defects, camera.repair_radius)
        psfs, info = [], {k: [] for k in ('positions', 'flux', 'ncc', 'rejected', 'std')}
        n_beads, width = np.zeros(V, dtype=np.int64), np.zeros((V, 2))
        for v in range(V):
            psf, vi = _measure_view(dev, imgs, frames, v, F, V, ny, nx, (y0, x0), camera, w, radius, b, rel_threshold, threshold, max_beads,
                                    min_sep, size, c, W, M, max_shift, passes, min_ncc)
            psfs.append(psf)
            for k in info:
                info[k].append(vi[k])
            n_beads[v] = len(vi['ncc'])
            width[v] = [_FWHM * abs(get_width(psf[0, size // 2, :])[0]), _FWHM * abs(get_width(psf[0, :, size // 2])[0])]
        info.update({'n_beads': n_beads, 'width': width, 'margin': m, 'border': b})
        info.update(camera.defect_info())
        return psfs, info
    finally:
        dev.close()


def _measure_view(dev, imgs, frames, v, F, V, ny, nx, origin, camera, w, radius, b, rel, threshold, cap, min_sep, size, c, W, M, max_shift,
                  passes, min_ncc):
    """Steps 2 - 8 of measure_psfs for view v: (psf (1, size, size), info of the view)."""
    rejected = dict.fromkeys(REASONS, 0)
    found, counts, _ = dev.find_peaks(imgs, [(f * V + v) * ny * nx for f in range(F)], ny, nx, w, radius, b, rel, threshold, cap)
    beads = []                                                       # (frame, y, x), in frame order, each frame's in row-major order
    for f in range(F):
        yx = found[f]['yx']
        rejected['cap'] += int(counts[f]) - len(yx)
        close = np.zeros(len(yx), dtype=bool)
        if len(yx) > 1:
            d = np.abs(yx[:, None, :] - yx[None, :, :]).max(axis=2)
            np.fill_diagonal(d, min_sep)
            close = (d < min_sep).any(axis=1)
        rejected['separation'] += int(close.sum())
        for (py, px), near in zip(yx, close):
            if near:
                continue
            if camera.saturation is not None:
                win = frames[f, v, origin[0] + py - c:origin[0] + py + c + 1, origin[1] + px - c:origin[1] + px + c + 1]
                if np.any(win >= camera.saturation):
                    rejected['saturated'] += 1
                    continue
            beads.append((f, int(py), int(px)))
    if not beads:
        raise ValueError('view %d: no bead left to measure (rejected: %s)' % (v, rejected))
    K, WW = len(beads), W * W
    windows, moved, scratch = dev.alloc(K * WW, 'f64'), dev.alloc(K * WW, 'f64'), dev.alloc(K * WW, 'f64')
    mean, var = dev.alloc(WW, 'f64'), dev.alloc(WW, 'f64')
    dev.gather(imgs, F * V, ny, nx, [(f * V + v, py - c, px - c) for f, py, px in beads], W, windows)
    offs = [k * WW for k in range(K)]
    dev.group_stats(windows, offs, [0, K], WW, mean=mean)
    live = np.ones(K, dtype=bool)
    for _ in range(passes):
        shifts, fields, _ = dev.estimate(mean, [0] * K, windows, offs, W, W, max_shift, M, 1, scratch)
        for reason, col in (('flat', 2), ('at_limit', 1)):
            out = live & (fields[:, col] != 0.0)
            rejected[reason] += int(out.sum())
            live &= ~out
        if not live.any():
            raise ValueError('view %d: every bead came out flat or at the search limit (rejected: %s)' % (v, rejected))
        dev.shift(windows, 0, K, W, W, shifts, 3, None, moved)
        dev.group_stats(moved, [offs[k] for k in np.flatnonzero(live)], [0, int(live.sum())], WW, mean=mean)
    total = shifts + centroid_offset(dev.download(mean, WW).reshape(W, W), size)
    dev.shift(windows, 0, K, W, W, total, 3, None, moved)
    ncc = fields[:, 0]
    low = live & ~(ncc >= min_ncc)
    rejected['ncc'] += int(low.sum())
    keep = np.flatnonzero(live & ~low)
    if keep.size == 0:
        raise ValueError('view %d: no bead reaches min_ncc = %g (rejected: %s)' % (v, min_ncc, rejected))
    dev.group_stats(moved, [offs[k] for k in keep], [0, keep.size], WW, mean=mean, var=var)
    c0 = c - size // 2
    full = dev.download(mean, WW).reshape(W, W)[c0:c0 + size, c0:c0 + size]
    spread = dev.download(var, WW).reshape(W, W)[c0:c0 + size, c0:c0 + size]
    P = np.maximum(full - ring_mean(full), 0.0)
    norm = P.sum()
    if not norm > 0.0:
        raise ValueError('view %d: the mean of the beads has no signal above its ring' % v)
    crops = dev.download(moved, K * WW).reshape(K, W, W)[keep][:, c0:c0 + size, c0:c0 + size]
    ring = np.ones((size, size), dtype=bool)
    ring[2:-2, 2:-2] = False
    flux = crops.reshape(len(keep), -1).sum(axis=1) - size * size * crops[:, ring].mean(axis=1)
    pos = np.array([(beads[k][0], beads[k][1] + total[k, 0], beads[k][2] + total[k, 1]) for k in keep], dtype=np.float64)
    std = np.sqrt(spread / keep.size) / norm
    return (P / norm)[None], {'positions': pos, 'flux': flux, 'ncc': ncc[keep].copy(), 'rejected': rejected, 'std': std[None]}
