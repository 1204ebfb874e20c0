"""Reconstruction-quality metrics of the figure-2 harness and of
Deconvolver.record_iteration, on the device (csrc/quality_kernels.hip, float64):

  fourier_error(estimate, true_object)        line_sted_figure_2.py:353-355
  ft_error_history(estimates, true_object)    line_sted_tools.py:539-547
  map_coordinates(image, coordinates)         scipy defaults, as used at :381-384
  error_vs_spatial_frequency(...)             line_sted_figure_2.py:362-390

and the ring statistics of image pairs (csrc/ring_kernels.hip; the definition: include/rlsted.h, rl_ring_stats) with what is
read off them -- no counterpart in the reference:

  ring_stats(a, b, n_rings, scale)            [..., R, 5]: bins, sum |A|^2, sum |B|^2, sum Re(A conj B), sum |A - B|^2 per ring
  frc(a, b), frc_resolution(freq, curve)      Fourier ring correlation of two noise realisations, and where it crosses 1/7
  radial_fourier_error(estimate, true_object) the ring RMS of fourier_error
  sector_stats(a, b, n_sectors, ...)          [..., R, S, 5]: the same fields per (ring, orientation sector) cell (rl_ring_sector_stats)
  directional_fourier_error(estimate, true_object, n_sectors)   the cell RMS of fourier_error: one error profile per orientation
  frc_resolution_by_angle(stats)              frc_resolution of each sector's curve

("ref2:NNN" = line numbers in figure_generation/line_sted_figure_2.py.)
"""
import ctypes

import numpy as np

from ._lib import DTYPES, lib, check, ptr, as_f64
from .psf import _ctx, gaussian_filter


def _fft2_magnitude(x, scale, log1p):
    x = as_f64(x)
    squeeze = x.ndim == 2
    if squeeze:
        x = x[None]
    if x.ndim != 3:
        raise ValueError('expected a 2-D image or a 3-D stack of images')
    out = np.empty_like(x)
    check(lib.rl_fft2_magnitude(_ctx().handle, ptr(x), x.shape[0], x.shape[1], x.shape[2],
                                float(scale), int(log1p), ptr(out)))
    return out[0] if squeeze else out


def fourier_error(estimate, true_object):
    """ref2:353-355: abs(fftshift(fftn(x - true_object))) / prod(true_object.shape), 2-D arrays
    (or stacks of them: one 2-D transform per leading index)."""
    d = as_f64(np.asarray(estimate, dtype=np.float64) - np.asarray(true_object, dtype=np.float64))
    return _fft2_magnitude(d, 1.0 / (d.shape[-2] * d.shape[-1]), False)


def ft_error_history(estimates, true_object):
    """line_sted_tools.py:539-547: log(1 + abs(fftshift(fft2(estimate_k - true_object)))) for a
    stack of saved estimates (k, ny, nx); a 2-D input is treated as one estimate."""
    d = np.asarray(estimates, dtype=np.float64) - np.asarray(true_object, dtype=np.float64)
    if d.ndim == 2:
        d = d.reshape(1, d.shape[0], d.shape[1])
    return _fft2_magnitude(as_f64(d), 1.0, True)


def map_coordinates(image, coordinates):
    """scipy.ndimage.map_coordinates(image, coordinates) for a 2-D image with scipy's defaults
    (order=3, mode='constant', cval=0.0, prefilter=True); coordinates = (2, ...) array-like."""
    image = as_f64(image)
    if image.ndim != 2:
        raise ValueError('expected a 2-D image')
    c = np.asarray(coordinates, dtype=np.float64)
    if c.shape[0] != 2:
        raise ValueError('coordinates must have shape (2, ...)')
    ys, xs = as_f64(c[0].ravel()), as_f64(c[1].ravel())
    out = np.empty(ys.size)
    check(lib.rl_spline_sample(_ctx().handle, ptr(image), image.shape[0], image.shape[1], ptr(ys), ptr(xs),
                               int(ys.size), ptr(out)))
    return out.reshape(c.shape[1:])


def error_vs_spatial_frequency(estimate, true_object, angle_degrees=0.0, radius=0.3, samples=1000,
                               smooth=True):
    """ref2:362-390: the Fourier error along a line through the centre of the shifted spectrum
    at `angle_degrees`, half length `radius` (fraction of the image size), `samples` points,
    cubic-spline interpolated and (smooth=True) Gaussian filtered with sigma = samples / 80.
    The figure plots angle 0 ("best") for point and line STED and 90/num_angles ("worst")."""
    fe = fourier_error(estimate, true_object)
    if fe.ndim != 2:
        raise ValueError('expected 2-D estimate and object')
    n_x, n_y = fe.shape                                    # ref2:363 names the axes this way round
    ang = angle_degrees * 2 * np.pi / 360
    x0, x1 = (0.5 + radius * np.array((-np.cos(ang), np.cos(ang)))) * n_x
    y0, y1 = (0.5 + radius * np.array((-np.sin(ang), np.sin(ang)))) * n_y
    xy = np.vstack((np.linspace(x0, x1, samples), np.linspace(y0, y1, samples)))
    z = map_coordinates(np.ascontiguousarray(np.transpose(fe)), xy)             # ref2:381
    if not smooth:
        return z
    return gaussian_filter(z.reshape(1, 1, -1), (0, 0, samples / 80))[0, 0]     # ref2:387


# ------------------------------------------------------------------ ring statistics
RING_FIELDS = 5


def ring_count(ny, nx):
    """The default number of rings of an (ny, nx) image: min(ny, nx) // 2."""
    return int(lib.rl_ring_count(int(ny), int(nx)))


def _stats_device(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, shape, scale, n_rings, n_sectors):
    """rl_ring_stats (n_sectors None) or rl_ring_sector_stats on device buffers."""
    ny, nx = int(shape[0]), int(shape[1])
    R = ring_count(ny, nx) if n_rings is None else int(n_rings)
    a_off = np.ascontiguousarray(a_offsets, dtype=np.int64).ravel()
    b_off = np.ascontiguousarray(b_offsets, dtype=np.int64).ravel()
    if a_off.size != b_off.size:
        raise ValueError('one offset per pair in both buffers; got %d and %d' % (a_off.size, b_off.size))
    sc = None
    if scale is not None:
        sc = as_f64(np.broadcast_to(np.asarray(scale, dtype=np.float64), a_off.shape))
    i64p = ctypes.POINTER(ctypes.c_int64)
    head = (ctx.handle, a_dev, DTYPES[a_dtype], a_off.ctypes.data_as(i64p), b_dev, DTYPES[b_dtype], b_off.ctypes.data_as(i64p),
            ptr(sc) if sc is not None else None, int(a_off.size), ny, nx, R)
    if n_sectors is None:
        out = np.empty((a_off.size, max(R, 0), RING_FIELDS))
        check(lib.rl_ring_stats(*head, ptr(out)))
    else:
        out = np.empty((a_off.size, max(R, 0), max(int(n_sectors), 0), RING_FIELDS))
        check(lib.rl_ring_sector_stats(*head, int(n_sectors), ptr(out)))
    return out


def ring_stats_device(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, shape, scale=None, n_rings=None):
    """rl_ring_stats on device buffers: image pair i = (a_dev + a_offsets[i], b_dev + b_offsets[i]), offsets in elements, all
    images of `shape`; dtypes 'f32' / 'f64'; scale None or one value per pair.  Returns [n_pairs][R][5] float64."""
    return _stats_device(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, shape, scale, n_rings, None)


def sector_stats_device(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, shape, n_sectors, scale=None, n_rings=None):
    """rl_ring_sector_stats on device buffers: ring_stats_device with every ring cut into `n_sectors` orientation sectors (sector
    j centred on j * 180 / n_sectors degrees, sector_angles).  Returns [n_pairs][R][S][5] float64; an empty cell is five zeros."""
    return _stats_device(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, shape, scale, n_rings, int(n_sectors))


def _stack(x, name):
    x = as_f64(x)
    if x.ndim == 2:
        return x[None], True
    if x.ndim != 3:
        raise ValueError('%s: expected a 2-D image or a 3-D stack of images' % name)
    return x, False


def ring_stats(a, b, n_rings=None, scale=None, n_sectors=None):
    """The ring statistics of host images: a, b (ny, nx) or stacks (n, ny, nx); a single image on either side pairs with every image
    of the other.  scale: None (1), a number, or one per pair -- b is multiplied by it.  Returns (R, 5) for two single images, else
    (n, R, 5); with n_sectors = S (sector_stats) (R, S, 5) and (n, R, S, 5).  The images are uploaded and go through the same entry
    point as device-resident ones."""
    a, one_a = _stack(a, 'a')
    b, one_b = _stack(b, 'b')
    if a.shape[1:] != b.shape[1:]:
        raise ValueError('a and b differ in image shape: %s, %s' % (a.shape[1:], b.shape[1:]))
    n = max(a.shape[0], b.shape[0])
    if a.shape[0] not in (1, n) or b.shape[0] not in (1, n):
        raise ValueError('stacks of %d and %d images do not pair up' % (a.shape[0], b.shape[0]))
    from .sweep import DeviceResults                     # (sweep imports this module)
    da, db = DeviceResults.from_host(list(a), 'f64', _ctx().device), DeviceResults.from_host(list(b), 'f64', _ctx().device)
    try:
        out = da.ring_stats(np.arange(n) if a.shape[0] == n else np.zeros(n, dtype=np.int64), truth=db,
                            truth_index=np.arange(n) if b.shape[0] == n else np.zeros(n, dtype=np.int64), scale=scale, n_rings=n_rings,
                            n_sectors=n_sectors)
    finally:
        da.free()
        db.free()
    return out[0] if one_a and one_b else out


def ring_frequencies(n_rings):
    """Cycles per pixel at the ring centres: ring r covers [r, r + 1) * 0.5 / R."""
    return (np.arange(int(n_rings)) + 0.5) * 0.5 / int(n_rings)


def sector_stats(a, b, n_sectors, n_rings=None, scale=None):
    """ring_stats per (ring, orientation sector) cell: (R, S, 5) for two single images, else (n, R, S, 5)."""
    return ring_stats(a, b, n_rings, scale, n_sectors=int(n_sectors))


def sector_angles(n_sectors):
    """The sector centres in degrees, j * 180 / S: measured from +kx towards +ky (error_vs_spatial_frequency's angle_degrees)."""
    return np.arange(int(n_sectors)) * 180.0 / int(n_sectors)


def rings_from_sectors(stats):
    """[..., R, S, 5] -> [..., R, 5]: every field summed over the sectors of its ring."""
    return np.asarray(stats, dtype=np.float64).sum(axis=-2)


def frc_from_stats(stats):
    """f3 / sqrt(f1 f2) per ring of [..., R, 5] (per cell of [..., R, S, 5]); nan where a ring is empty or a denominator is 0."""
    stats = np.asarray(stats, dtype=np.float64)
    den = np.sqrt(stats[..., 1] * stats[..., 2])
    ok = (stats[..., 0] > 0) & (den > 0)
    return np.where(ok, stats[..., 3] / np.where(ok, den, 1.0), np.nan)


def radial_error_from_stats(stats, shape):
    """sqrt(f4 / f0) / (ny nx): the RMS over each ring (each cell of [..., R, S, 5]) of |fft2(estimate) - fft2(scaled truth)| / (ny nx);
    nan for an empty ring."""
    stats = np.asarray(stats, dtype=np.float64)
    ok = stats[..., 0] > 0
    return np.where(ok, np.sqrt(stats[..., 4] / np.where(ok, stats[..., 0], 1.0)) / (int(shape[0]) * int(shape[1])), np.nan)


def frc(a, b, n_rings=None):
    """Fourier ring correlation of two images (two noise realisations of one object).  Returns (frequencies in cycles/pixel at the
    ring centres, curve)."""
    st = ring_stats(a, b, n_rings)
    return ring_frequencies(st.shape[-2]), frc_from_stats(st)


def frc_resolution(freq, curve, threshold=1.0 / 7.0):
    """The period in pixels, 1 / frequency, at which the curve first falls below `threshold`: linearly interpolated between the last
    ring at or above it and the first ring below (nan rings are passed over); the first ring's own frequency if the curve starts
    below; inf if it never crosses."""
    freq = np.asarray(freq, dtype=np.float64)
    curve = np.asarray(curve, dtype=np.float64)
    prev = None
    for f, c in zip(freq, curve):
        if np.isnan(c):
            continue
        if c < threshold:
            if prev is None:
                return 1.0 / f
            f0, c0 = prev
            return 1.0 / (f0 + (c0 - threshold) / (c0 - c) * (f - f0))
        prev = (f, c)
    return float('inf')


def radial_fourier_error(estimate, true_object, n_rings=None):
    """The ring RMS of fourier_error(estimate, true_object) (ref2:353-355): sqrt(mean over the ring of fourier_error^2).  Returns
    (frequencies in cycles/pixel at the ring centres, profile)."""
    est = as_f64(estimate)
    st = ring_stats(est, true_object, n_rings)
    return ring_frequencies(st.shape[-2]), radial_error_from_stats(st, est.shape[-2:])


def directional_fourier_error(estimate, true_object, n_sectors, n_rings=None):
    """The RMS of fourier_error(estimate, true_object) over each (ring, orientation sector) cell: what error_vs_spatial_frequency
    cuts out of the spectrum along one angle, for n_sectors angles at once.  Returns (frequencies in cycles/pixel at the ring
    centres, sector centres in degrees, profile [R][S]); nan where a cell is empty."""
    est = as_f64(estimate)
    st = sector_stats(est, true_object, n_sectors, n_rings)
    return ring_frequencies(st.shape[-3]), sector_angles(n_sectors), radial_error_from_stats(st, est.shape[-2:])


def frc_resolution_by_angle(stats, threshold=1.0 / 7.0):
    """frc_resolution of each sector's correlation curve of stats [R][S][5] (two noise realisations): [S] periods in pixels."""
    curves = frc_from_stats(stats)
    if curves.ndim != 2:
        raise ValueError('expected the statistics of one pair, [R][S][5]')
    freq = ring_frequencies(curves.shape[0])
    return np.array([frc_resolution(freq, curves[:, j], threshold) for j in range(curves.shape[1])])


# ------------------------------------------------------------------ ensemble statistics
ENSEMBLE_FIELDS = 6


def ensemble_stats_device(ctx, dev, dtype, groups_offsets, n_pixels, truth=None, mean_dev=None, var_dev=None):
    """rl_ensemble_stats (include/rlsted.h) on a device buffer: group g is the images of `n_pixels` values at the element offsets
    groups_offsets[g] (a list of offset lists; groups may differ in size) of `dev`, dtype 'f32' / 'f64'.  truth: None, or
    (truth_dev, truth_dtype, truth_offsets, scale) -- one element offset per group and scale None, a number or one per group.
    mean_dev, var_dev: None, or device float64 [G][n_pixels] that receive the per-pixel mean and unbiased variance.
    Returns [G][6] float64: n, and the pixel sums of mean, variance, bias^2, mean squared error and (scaled truth)^2."""
    groups = [np.ascontiguousarray(g, dtype=np.int64).ravel() for g in groups_offsets]
    G = len(groups)
    gp = np.zeros(G + 1, dtype=np.int32)
    gp[1:] = np.cumsum([g.size for g in groups]) if G else []
    off = np.ascontiguousarray(np.concatenate(groups)) if G else np.zeros(0, dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    t_dev, t_dtype, t_off, sc = None, 0, None, None
    if truth is not None:
        t_dev, t_name, t_offsets, scale = truth
        t_dtype = DTYPES[t_name]
        t_off = np.ascontiguousarray(t_offsets, dtype=np.int64).ravel()
        if t_off.size != G:
            raise ValueError('one truth offset per group; got %d for %d groups' % (t_off.size, G))
        if scale is not None:
            sc = as_f64(np.broadcast_to(np.asarray(scale, dtype=np.float64), (G,)))
    out = np.empty((G, ENSEMBLE_FIELDS))
    check(lib.rl_ensemble_stats(ctx.handle, dev, DTYPES[dtype], off.ctypes.data_as(i64p), gp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                G, t_dev, t_dtype, t_off.ctypes.data_as(i64p) if t_off is not None else None,
                                ptr(sc) if sc is not None else None, int(n_pixels), mean_dev, var_dev, ptr(out)))
    return out


def ensemble_stats(stack, truth=None, scale=None):
    """The ensemble statistics of host images: `stack` (n, ...) -- n members of one group, any image shape -- or a list of such
    stacks, one per group (the groups may differ in n, not in image shape).  truth: None, one image, or one per group; scale: None
    (1), a number or one per group, multiplied into the truth.  Returns (mean, variance, scalars): the float64 maps of the image
    shape and [6] (ensemble_stats_device) for a single stack, with a leading group axis for a list.  The images are uploaded and go
    through the same entry point as device-resident ones."""
    single = not isinstance(stack, (list, tuple))
    stacks = [as_f64(s) for s in ([stack] if single else stack)]
    if not stacks or any(s.ndim < 2 or s.shape[0] < 1 for s in stacks):
        raise ValueError('expected a stack (n, ...) of n >= 1 images, or a list of them')
    shape = stacks[0].shape[1:]
    if any(s.shape[1:] != shape for s in stacks):
        raise ValueError('the groups differ in image shape')
    flat = (int(np.prod(shape)), 1)
    from .sweep import DeviceResults                     # (sweep imports this module)
    members = [im.reshape(flat) for s in stacks for im in s]
    groups, at = [], 0
    for s in stacks:
        groups.append(list(range(at, at + s.shape[0])))
        at += s.shape[0]
    src = DeviceResults.from_host(members, 'f64', _ctx().device)
    tr = None
    try:
        if truth is not None:
            t = as_f64(truth)
            t = t.reshape((-1,) + flat) if t.shape != shape else t.reshape((1,) + flat)
            if t.shape[0] not in (1, len(stacks)):
                raise ValueError('one truth image, or one per group')
            tr = DeviceResults.from_host(list(t), 'f64', _ctx().device)
            t_idx = np.arange(len(stacks)) if t.shape[0] == len(stacks) else np.zeros(len(stacks), dtype=np.int64)
            means, variances, sc = src.ensemble(groups, truth=tr, truth_index=t_idx, scale=scale)
        else:
            means, variances, sc = src.ensemble(groups)
        try:
            m = np.stack(means.download()).reshape((len(stacks),) + shape)
            v = np.stack(variances.download()).reshape((len(stacks),) + shape)
        finally:
            means.free()
            variances.free()
    finally:
        src.free()
        if tr is not None:
            tr.free()
    return (m[0], v[0], sc[0]) if single else (m, v, sc)


def spectral_bias_variance_rms(spectrum, shape):
    """[..., 3] (bin count, bias power, variance power per ring or per (ring, sector) cell: sweep.bias_variance_spectrum) ->
    (bias RMS, noise RMS), each sqrt(power / count) / (ny nx): the units of radial_error_from_stats; nan for an empty ring."""
    spectrum = np.asarray(spectrum, dtype=np.float64)
    ok = spectrum[..., 0] > 0
    cnt = np.where(ok, spectrum[..., 0], 1.0)
    pix = int(shape[0]) * int(shape[1])
    return (np.where(ok, np.sqrt(spectrum[..., 1] / cnt) / pix, np.nan), np.where(ok, np.sqrt(spectrum[..., 2] / cnt) / pix, np.nan))


def ssnr_from(mean_stats, spectrum, n):
    """The spectral signal-to-noise ratio of an n-member ensemble mean per ring (or cell): field 1 of the ring statistics of the
    mean image (sum |fft2(mean)|^2: mean_stats [..., 5]) over the variance power of `spectrum` [..., 3] divided by n (the noise
    power left in a mean of n).  nan for an empty ring or a variance power of 0."""
    mean_stats = np.asarray(mean_stats, dtype=np.float64)
    spectrum = np.asarray(spectrum, dtype=np.float64)
    noise = spectrum[..., 2] / float(n)
    ok = (spectrum[..., 0] > 0) & (noise > 0)
    return np.where(ok, mean_stats[..., 1] / np.where(ok, noise, 1.0), np.nan)


# ------------------------------------------------------------------ iteration checkpoints
TRACE_FIELDS = 6


def trace_metrics(trace, n_pixels):
    """The error measures a checkpoint trace holds (include/rlsted.h rl_batch_submit_checkpoints): trace [..., 6] = the pixel sums of
    x, T, x^2, T^2, x T and (x - T)^2 of an estimate x against its scaled object T; n_pixels a number or an array that broadcasts
    against trace[..., 0].  Returns a dict of arrays of that shape:
        mse    f5 / n
        nrmse  sqrt(f5 / f3)
        ncc    the centred normalised correlation (n f4 - f0 f1) / sqrt((n f2 - f0^2) (n f3 - f1^2))
        flux   f0 / f1
    nan where a denominator is not positive."""
    t = np.asarray(trace, dtype=np.float64)
    if t.shape[-1] != TRACE_FIELDS:
        raise ValueError('expected [..., %d] sums; got shape %r' % (TRACE_FIELDS, t.shape))
    f = [t[..., c] for c in range(TRACE_FIELDS)]
    n = np.broadcast_to(np.asarray(n_pixels, dtype=np.float64), f[0].shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        den = (n * f[2] - f[0] * f[0]) * (n * f[3] - f[1] * f[1])
        return {'mse': np.where(n > 0, f[5] / n, np.nan),
                'nrmse': np.where(f[3] > 0, np.sqrt(f[5] / f[3]), np.nan),
                'ncc': np.where(den > 0, (n * f[4] - f[0] * f[1]) / np.sqrt(den), np.nan),
                'flux': np.where(f[1] != 0, f[0] / f[1], np.nan)}
