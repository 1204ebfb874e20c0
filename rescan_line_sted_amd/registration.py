"""Registration of the views and frames of acquired stacks on the device, in front of Richardson-Lucy (INTEGRATION.md section 5i,
DESIGN.md section 4k).

The V views of a frame are recorded one after the other and a time series runs for minutes: the sample drifts between exposures.
Multi-view Richardson-Lucy multiplies the back-projections of all views, so a view that is off by a pixel or two is not averaged
away.  estimate_shifts finds translations from normalised cross-correlation over a window of integer displacements plus a parabola
(include/rlsted.h rl_register_sums), shift_images undoes them with the scipy-compatible B-spline (rl_shift_images), and
deconvolve_stack_registered puts both between the narrow ingest of deconvolve_stack and the plan -- the data never leaves the device.

SIGN CONVENTION, used everywhere: the shift of an image is the displacement d of its content relative to the reference,
image[y + d] ~ reference[y].  The correlation surface peaks at d, and shift_images(image, d) undoes it.

    estimates, info = deconvolve_stack_registered(raw, psfs, iterations, camera=CameraModel(dark=100.0, gain=0.46))

Rotation, scale and shear between the views: estimate_transforms fits a
translation, rigid, similarity or affine transform by Gauss-Newton on the intensities over a pyramid (rl_affine_sums forms the normal
equations on the device, solve_transform solves them here), warp_images resamples through an affine map (rl_warp_images), and
deconvolve_stack_registered(model=...) composes the view's transform with the frame's shift into one interpolation per image.
"""
import ctypes

import numpy as np

from . import _lib, stack
from ._lib import DTYPES, check, lib
from .stack import EXPORT_FIELDS, INGEST_FIELDS, ORDERS, OUT_DTYPES, CameraModel, _stack_shape, raw_code

MAX_RADIUS = 32                       # rl_register_sums
XCORR_FIELDS = 7                      # rl_register_xcorr
PEAK_FIELDS = 5                       # rl_register_peaks
XCORR_MAX_LENGTH = 1152               # the largest transform length of the coarse stage: image side + radius
_NP = {'f32': np.float32, 'f64': np.float64}
_I64P = ctypes.POINTER(ctypes.c_int64)


# ---- host logic: NCC, peak, parabola -----------------------------------------------------------------------------------------------
def ncc_surface(sums, ref, n):
    """NCC(d) = (S_ab - S_a S_b / n) / sqrt((S_aa - S_a^2 / n)(S_bb - S_b^2 / n)) in float64 from one pair's sums [W * W][3] and
    (S_a, S_aa); returns (surface [W][W], flat) -- flat: a variance that is not positive, the surface is then zeros."""
    sums = np.asarray(sums, dtype=np.float64)
    W = int(round(np.sqrt(sums.shape[0])))
    sa, saa = float(ref[0]), float(ref[1])
    va = saa - sa * sa / n
    vb = sums[:, 1] - sums[:, 0] * sums[:, 0] / n
    if not va > 0.0 or not np.all(vb > 0.0):
        return np.zeros((W, W)), True
    return ((sums[:, 2] - sa * sums[:, 0] / n) / np.sqrt(va * vb)).reshape(W, W), False


def surface_peak(c):
    """(shift [2] = integer peak + parabola, peak value, at_limit) of a surface [W][W]: the first maximum in row-major order; a
    separable three-point parabola per axis, delta = (c- - c+) / (2 (c- - 2 c0 + c+)); a peak on the window's border: delta = 0."""
    W = c.shape[0]
    R = W // 2
    iy, ix = divmod(int(np.argmax(c)), W)
    if iy in (0, W - 1) or ix in (0, W - 1):
        return np.array([iy - R, ix - R], dtype=np.float64), float(c[iy, ix]), True
    delta = []
    for m, z, p in ((c[iy - 1, ix], c[iy, ix], c[iy + 1, ix]), (c[iy, ix - 1], c[iy, ix], c[iy, ix + 1])):
        den = m - 2.0 * z + p
        delta.append(0.5 * (m - p) / den if den != 0.0 else 0.0)
    return np.array([iy - R + delta[0], ix - R + delta[1]]), float(c[iy, ix]), False


def _check_search(ny, nx, max_shift, refine, margin):
    max_shift, refine = int(max_shift), int(refine)
    if not 1 <= max_shift <= MAX_RADIUS:
        raise ValueError('max_shift must lie in 1 .. %d; got %r' % (MAX_RADIUS, max_shift))
    if refine < 0:
        raise ValueError('refine must be at least 0')
    margin = max_shift + 2 if margin is None else int(margin)
    if margin < max_shift + (2 if refine else 0):
        raise ValueError('margin must be at least max_shift%s; got %d' % (' + 2 (mirrored border content stays outside the sums)' if refine else '', margin))
    if ny - 2 * margin < 8 or nx - 2 * margin < 8:
        raise ValueError('a %d x %d image leaves no 8 x 8 interior inside a margin of %d' % (ny, nx, margin))
    return max_shift, refine, margin


def _estimate(dev, ref, ref_offsets, mov, mov_offsets, ny, nx, max_shift, refine, margin, scratch, surfaces=False, coarse=None):
    """Stages 1 - 5 for the pairs (ref at ref_offsets[i], mov at mov_offsets[i]) through dev.sums / dev.shift; scratch: a float64
    buffer of len(pairs) images (refine > 0, or coarse).  coarse: None, or the radius of the coarse stage in front
    (_estimate_coarse).  Returns (shifts (N, 2), info)."""
    if coarse is not None:
        return _estimate_coarse(dev, ref, ref_offsets, mov, mov_offsets, ny, nx, max_shift, refine, coarse, scratch, surfaces)
    N = len(mov_offsets)
    n = (ny - 2 * margin) * (nx - 2 * margin)
    shifts, value = np.zeros((N, 2)), np.zeros(N)
    at_limit, flat = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    S, A = dev.sums(ref, ref_offsets, mov, mov_offsets, ny, nx, max_shift, margin)
    kept = []
    for i in range(N):
        c, flat[i] = ncc_surface(S[i], A[i], n)
        if surfaces:
            kept.append(c)
        if not flat[i]:
            shifts[i], value[i], at_limit[i] = surface_peak(c)
    for _ in range(refine):
        live = np.flatnonzero(~flat)
        if live.size == 0:
            break
        # every moving image by its current estimate into the scratch buffer (order 3, no floor), then a 3 x 3 window
        dev.gather_shift(mov, [mov_offsets[i] for i in live], ny, nx, shifts[live], scratch)
        S, A = dev.sums(ref, [ref_offsets[i] for i in live], scratch, [k * ny * nx for k in range(live.size)], ny, nx, 1, margin)
        for k, i in enumerate(live):
            c, f = ncc_surface(S[k], A[k], n)
            if not f:
                d, value[i], _ = surface_peak(c)
                shifts[i] += d
    info = {'ncc': value, 'at_limit': at_limit, 'flat': flat}
    if surfaces:
        info['surfaces'] = np.stack(kept)
    return shifts, info


def _estimate_on_device(dev, ref, ref_offsets, mov, mov_offsets, ny, nx, max_shift, refine, margin, scratch, surfaces=False):
    """_estimate (coarse=None) in one call through dev.estimate (rl_register_estimate): the NCC, the peaks and the parabolas on the
    device, the refine passes' offsets added on the host by the same rules; the same bits as _estimate."""
    shifts, fields, C = dev.estimate(ref, ref_offsets, mov, mov_offsets, ny, nx, max_shift, margin, refine, scratch, surfaces)
    info = {'ncc': fields[:, 0].copy(), 'at_limit': fields[:, 1] != 0.0, 'flat': fields[:, 2] != 0.0}
    if surfaces:
        info['surfaces'] = C.reshape(len(mov_offsets), 2 * max_shift + 1, 2 * max_shift + 1)
    return shifts, info


# ---- host logic: the coarse stage ----------------------------------------------------------------------------------------------------
def coarse_fields(peaks, radius):
    """(c (N, 2) int64, value, snr, flat) from the fields of rl_register_xcorr [N][7]: snr = (peak - window mean) / window standard
    deviation (0 where the window has no variance); flat: an energy that is not positive."""
    peaks = np.asarray(peaks, dtype=np.float64).reshape(-1, XCORR_FIELDS)
    n = float((2 * radius + 1) ** 2)
    mean = peaks[:, 5] / n
    var = peaks[:, 6] / n - mean * mean
    ok = var > 0.0
    snr = np.zeros(len(peaks))
    snr[ok] = (peaks[ok, 2] - mean[ok]) / np.sqrt(var[ok])
    flat = ~(peaks[:, 3] > 0.0) | ~(peaks[:, 4] > 0.0)
    return np.rint(peaks[:, :2]).astype(np.int64), peaks[:, 2].copy(), snr, flat


def coarse_margin(c, max_shift):
    """The margin of the pairs with coarse displacements c (N, 2): 8 ceil(|c|_inf / 8) + max_shift + 2 -- the band the order-1 copy
    fills by mirroring stays outside the sums; a function of the pair alone, so a pair's result does not depend on its call."""
    c = np.asarray(c).reshape(-1, 2)
    return 8 * ((np.abs(c).max(axis=1) + 7) // 8) + max_shift + 2


def _check_coarse(ny, nx, coarse, max_shift, margin):
    if coarse is None:
        return None
    if int(coarse) != coarse or int(coarse) < 1:
        raise ValueError('coarse must be None or a radius of at least 1 pixel; got %r' % (coarse,))
    coarse = int(coarse)
    if margin is not None:
        raise ValueError('margin cannot be given together with coarse: every pair gets 8 ceil(|c| / 8) + max_shift + 2')
    worst = coarse + max_shift + 2
    if ny - 2 * worst < 8 or nx - 2 * worst < 8:
        raise ValueError('a %d x %d image leaves no 8 x 8 interior inside coarse + max_shift + 2 = %d pixels' % (ny, nx, worst))
    if ny + coarse > XCORR_MAX_LENGTH or nx + coarse > XCORR_MAX_LENGTH:
        raise ValueError('the coarse stage serves image side + coarse <= %d; got %d x %d with coarse = %d' % (XCORR_MAX_LENGTH, ny, nx, coarse))
    return coarse


def _estimate_coarse(dev, ref, ref_offsets, mov, mov_offsets, ny, nx, max_shift, refine, coarse, scratch, surfaces=False):
    """The two-stage estimate: rl_register_xcorr proposes c_i; the moving image displaced by c_i (order 1: a copy of the displaced
    pixels) goes through the exact window of radius max_shift; shift = c_i + peak + parabola; the refine passes shift the ORIGINAL
    image by the total.  Pairs of equal margin share the device calls.  scratch: a float64 buffer of len(pairs) images."""
    N = len(mov_offsets)
    n_pix = ny * nx
    peaks = dev.xcorr(ref, ref_offsets, mov, mov_offsets, ny, nx, coarse)
    c, cvalue, csnr, cflat = coarse_fields(peaks, coarse)
    margins = coarse_margin(c, max_shift)
    shifts, value = c.astype(np.float64), np.zeros(N)
    at_limit, flat = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    kept = [None] * N
    for M in sorted(set(int(m) for m in margins)):
        idx = np.flatnonzero(margins == M)
        n = (ny - 2 * M) * (nx - 2 * M)
        dev.gather_shift(mov, [mov_offsets[i] for i in idx], ny, nx, c[idx].astype(np.float64), scratch, order=1)
        S, A = dev.sums(ref, [ref_offsets[i] for i in idx], scratch, [k * n_pix for k in range(idx.size)], ny, nx, max_shift, M)
        for k, i in enumerate(idx):
            s, flat[i] = ncc_surface(S[k], A[k], n)
            kept[i] = s
            if not flat[i]:
                d, value[i], at_limit[i] = surface_peak(s)
                shifts[i] = np.where(c[i] == 0, d, c[i] + d)
        for _ in range(refine):
            live = idx[~flat[idx]]
            if live.size == 0:
                break
            dev.gather_shift(mov, [mov_offsets[i] for i in live], ny, nx, shifts[live], scratch)
            S, A = dev.sums(ref, [ref_offsets[i] for i in live], scratch, [k * n_pix for k in range(live.size)], ny, nx, 1, M)
            for k, i in enumerate(live):
                s, f = ncc_surface(S[k], A[k], n)
                if not f:
                    d, value[i], _ = surface_peak(s)
                    shifts[i] += d
    info = {'ncc': value, 'at_limit': at_limit, 'flat': flat, 'coarse': c, 'coarse_value': cvalue, 'coarse_snr': csnr, 'coarse_flat': cflat}
    if surfaces:
        info['surfaces'] = np.stack(kept)
    return shifts, info


# ---- host logic: affine transforms -----------------------------------------------------------------------
# CONVENTION: a transform is T = [L | t], shape (..., 2, 3), in the centred form: with c = ((ny - 1) / 2, (nx - 1) / 2) the image B
# with transform T relative to the reference A satisfies B(c + L (x - c) + t) ~ A(x); with L = I, t is the shift of estimate_shifts.
# As a map of output pixels to source positions, T(x) = c + L (x - c) + t, and warp_images(B, T)(x) = B(T(x)).
MODELS = ('translation', 'rigid', 'similarity', 'affine')
AFFINE_FIELDS = 45                    # rl_affine_sums
_PROJECTIONS = {                      # columns of the 8 unknowns (q_0 .. q_5, g, b) a model keeps, as (index, weight) lists
    'translation': [[(0, 1.0)], [(1, 1.0)], [(6, 1.0)], [(7, 1.0)]],
    'rigid': [[(0, 1.0)], [(1, 1.0)], [(4, 1.0), (3, -1.0)], [(6, 1.0)], [(7, 1.0)]],
    'similarity': [[(0, 1.0)], [(1, 1.0)], [(2, 1.0), (5, 1.0)], [(4, 1.0), (3, -1.0)], [(6, 1.0)], [(7, 1.0)]],
    'affine': [[(k, 1.0)] for k in range(8)],
}
MAX_CONDITION = 1e10                  # of the projected system after scaling to a unit diagonal


def identity_transforms(n):
    T = np.zeros((int(n), 2, 3))
    T[:, 0, 0] = T[:, 1, 1] = 1.0
    return T


def shift_transforms(shifts):
    """[I | d] for shifts (..., 2) as estimate_shifts returns them."""
    shifts = np.asarray(shifts, dtype=np.float64)
    T = np.zeros(shifts.shape[:-1] + (2, 3))
    T[..., 0, 0] = T[..., 1, 1] = 1.0
    T[..., 2] = shifts
    return T


def transform_matrix_offset(T, shape):
    """(..., 6) = (m00, m01, m10, m11, o0, o1) of rl_warp_images -- the matrix and offset of scipy.ndimage.affine_transform -- for
    transforms (..., 2, 3) of images of `shape`: matrix L, offset c + t - L c."""
    T = np.asarray(T, dtype=np.float64)
    c = np.array([(shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0])
    L, t = T[..., :2], T[..., 2]
    out = np.empty(T.shape[:-2] + (6,))
    out[..., :4] = L.reshape(T.shape[:-2] + (4,))
    out[..., 4:] = c + t - L @ c
    return out


def compose_transforms(first, second):
    """The transform of applying `first`, then `second`: warp(warp(B, first), second) = warp(B, compose_transforms(first, second)) up
    to the interpolation -- as maps, first o second: L = L1 L2, t = L1 t2 + t1."""
    a, b = np.asarray(first, dtype=np.float64), np.asarray(second, dtype=np.float64)
    out = np.empty(np.broadcast(a, b).shape)
    out[..., :2] = a[..., :2] @ b[..., :2]
    out[..., 2] = (a[..., :2] @ b[..., 2:])[..., 0] + a[..., 2]
    return out


def invert_transform(T):
    """[L^-1 | -L^-1 t]: warp(warp(B, T), invert_transform(T)) ~ B."""
    T = np.asarray(T, dtype=np.float64)
    Li = np.linalg.inv(T[..., :2])
    out = np.empty(T.shape)
    out[..., :2] = Li
    out[..., 2] = -(Li @ T[..., 2:])[..., 0]
    return out


def corner_displacement(T, other, shape):
    """The largest distance in pixels between T(x) and other(x) over the four corners of an image of `shape`."""
    T, other = np.asarray(T, dtype=np.float64), np.asarray(other, dtype=np.float64)
    cy, cx = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    corners = np.array([[-cy, -cx], [-cy, cx], [cy, -cx], [cy, cx]]).T
    d = (T[..., :2] - other[..., :2]) @ corners + (T[..., 2:] - other[..., 2:])
    return np.sqrt((d * d).sum(axis=-2)).max(axis=-1)


def solve_transform(sums, model):
    """One Gauss-Newton step from a pair's row of rl_affine_sums [45], projected on `model`: the 8 x 8 system in (q, g, b) of
    a ~ g w + b + phi q restricted to the model's columns, scaled to a unit diagonal, solved in float64; d = q / g.  Returns a dict:
    'dt' (2,), 'dL' (2, 2) -- the update is t <- t + L dt, L <- L (I + dL) --, 'gain', 'offset', 'residual' (the root of the residual
    sum of squares over the reference's centred sum of squares) and 'flat' (a diagonal entry that is not positive, a condition number
    above 1e10 or not finite, g <= 0, a reference without variance: the step is zero).  The device path and its numpy twin share it."""
    sums = np.asarray(sums, dtype=np.float64)
    G = np.zeros((8, 8))
    G[np.triu_indices(8)] = sums[:36]
    G = G + np.triu(G, 1).T
    r, saa, n = sums[36:44], sums[44], sums[35]
    cols = _PROJECTIONS[model]
    P = np.zeros((8, len(cols)))
    for k, col in enumerate(cols):
        for i, wgt in col:
            P[i, k] = wgt
    flat = dict(dt=np.zeros(2), dL=np.zeros((2, 2)), gain=0.0, offset=0.0, residual=0.0, flat=True)
    Gp, rp = P.T @ G @ P, P.T @ r
    d = np.diag(Gp)
    if not np.all(np.isfinite(Gp)) or not np.all(np.isfinite(rp)) or not np.all(d > 0.0) or not n > 0.0:
        return flat
    d = np.sqrt(d)
    Gs = Gp / np.outer(d, d)
    cond = np.linalg.cond(Gs)
    var = saa - r[7] * r[7] / n
    if not np.isfinite(cond) or cond > MAX_CONDITION or not var > 0.0:
        return flat
    eta = np.linalg.solve(Gs, rp / d) / d
    theta = P @ eta
    g = theta[6]
    if not np.all(np.isfinite(theta)) or not g > 0.0:
        return flat
    q = theta[:6] / g
    rss = saa - float(eta @ rp)
    return dict(dt=q[:2].copy(), dL=q[2:].reshape(2, 2).copy(), gain=float(g), offset=float(theta[7]),
                residual=float(np.sqrt(max(rss, 0.0) / var)), flat=False)


def update_transform(T, step, model):
    """The forward-compositional update of T (2, 3) by a step of solve_transform: t <- t + L dt, L <- L (I + dL); 'rigid' puts L
    back on the rotations (the orthogonal factor of its polar decomposition)."""
    L, t = T[:, :2], T[:, 2]
    out = np.empty((2, 3))
    out[:, 2] = t + L @ step['dt']
    Ln = L @ (np.eye(2) + step['dL'])
    if model == 'rigid':
        u, _, vt = np.linalg.svd(Ln)
        Ln = u @ vt
        if np.linalg.det(Ln) < 0.0:
            Ln = u @ np.diag([1.0, -1.0]) @ vt
    out[:, :2] = Ln
    return out


def pyramid_shapes(ny, nx, min_side):
    """The levels' shapes, finest first: halved (rounded down) while the halved shorter side is at least min_side."""
    shapes = [(ny, nx)]
    while min(shapes[-1]) // 2 >= min_side:
        shapes.append((shapes[-1][0] // 2, shapes[-1][1] // 2))
    return shapes


BIN2 = (2.0, 0.0, 0.0, 2.0, 0.5, 0.5)     # rl_warp_images order 1 with this map is the 2 x 2 mean


def _check_model(ny, nx, model, passes, min_side, margin):
    if model not in MODELS:
        raise ValueError('model: one of %s; got %r' % (', '.join(MODELS), model))
    passes, min_side, margin = int(passes), int(min_side), int(margin)
    if passes < 1:
        raise ValueError('passes must be at least 1')
    if margin < 1:
        raise ValueError('margin must be at least 1')
    if min_side < 2 * margin + 8:
        raise ValueError('min_side must be at least 2 margin + 8 = %d (the interior of the coarsest level); got %d' % (2 * margin + 8, min_side))
    if ny - 2 * margin < 8 or nx - 2 * margin < 8:
        raise ValueError('a %d x %d image leaves no 8 x 8 interior inside a margin of %d' % (ny, nx, margin))
    return passes, min_side, margin


def _estimate_transforms(dev, ref, ref_offsets, mov, mov_offsets, ny, nx, model, passes, min_side, margin, init=None):
    """estimate_transforms for the pairs (ref at ref_offsets[i], mov at mov_offsets[i]) through dev.alloc, dev.gather_warp and
    dev.affine_sums.  The pyramid of both images by 2 x binning (rl_warp_images order 1), then per level, coarsest first, `passes`
    passes of: the moving image warped by the current transform (order 3) into a float64 scratch, rl_affine_sums, solve_transform,
    update_transform.  A fixed sequence of device calls whatever the data.  Returns (T (N, 2, 3), info)."""
    N = len(mov_offsets)
    shapes = pyramid_shapes(ny, nx, min_side)
    uniq = sorted(set(ref_offsets))
    ref_index = [uniq.index(o) for o in ref_offsets]
    refs, movs = [(ref, list(uniq))], [(mov, list(mov_offsets))]
    for lv in range(1, len(shapes)):
        (py, px), (sy, sx) = shapes[lv - 1], shapes[lv]
        for chain, count in ((refs, len(uniq)), (movs, N)):
            buf = dev.alloc(count * sy * sx, 'f64')
            dev.gather_warp(chain[-1][0], chain[-1][1], py, px, np.tile(BIN2, (count, 1)), 1, buf, sy, sx)
            chain.append((buf, [k * sy * sx for k in range(count)]))
    scratch = dev.alloc(N * ny * nx, 'f64')
    T = identity_transforms(N)
    if init is not None:
        T[:, :, 2] = np.asarray(init, dtype=np.float64).reshape(N, 2)
    T[:, :, 2] /= 2.0 ** (len(shapes) - 1)
    flat = np.zeros(N, dtype=bool)
    gain, offset, residual, step = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    for lv in range(len(shapes) - 1, -1, -1):
        sy, sx = shapes[lv]
        for _ in range(passes):
            dev.gather_warp(movs[lv][0], movs[lv][1], sy, sx, transform_matrix_offset(T, (sy, sx)), 3, scratch, sy, sx)
            S = dev.affine_sums(refs[lv][0], [refs[lv][1][k] for k in ref_index], scratch, [k * sy * sx for k in range(N)], sy, sx, margin)
            for i in range(N):
                if flat[i]:
                    continue
                s = solve_transform(S[i], model)
                if s['flat']:
                    flat[i] = True
                    continue
                new = update_transform(T[i], s, model)
                gain[i], offset[i], residual[i] = s['gain'], s['offset'], s['residual']
                step[i] = corner_displacement(new, T[i], (sy, sx)) * 2.0 ** lv
                T[i] = new
        if lv:
            T[:, :, 2] *= 2.0
    T[flat] = identity_transforms(1)[0]
    gain[flat] = offset[flat] = residual[flat] = step[flat] = 0.0
    return T, {'gain': gain, 'offset': offset, 'residual': residual, 'step': step, 'flat': flat, 'levels': len(shapes)}


# ---- the device ----------------------------------------------------------------------------------------------------------------------
class _Buffer:
    """A device allocation of `elements` values of dtype 'f32' / 'f64' (or raw bytes: dtype None)."""

    def __init__(self, ptr, elements, dtype):
        self.ptr, self.elements, self.dtype = ptr, elements, dtype

    def at(self, element):
        return ctypes.c_void_p(self.ptr.value + element * np.dtype(_NP[self.dtype]).itemsize)


class _Device:
    """What the registration does on the GPU, one method per step (the CPU tests drive the wrappers with a numpy stand-in).  A plan
    is made only when PSFs are given."""

    def __init__(self, psfs=None, batch=0, shape=None, dtype='f32', device=0, acceleration=None, tv_lambda=None, tv_epsilon=0.1):
        self.plan = None
        if psfs is not None:
            self.plan = _lib.DeconvPlan(psfs, batch, shape[0], shape[1], dtype=dtype, device=device, acceleration=acceleration,
                                        tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
            self.ctx = self.plan.ctx
        else:
            self.ctx = _lib.Context.get(device, 0)
        self.owned = []

    def alloc(self, elements, dtype):
        p = ctypes.c_void_p()
        size = 1 if dtype is None else np.dtype(_NP[dtype]).itemsize
        check(lib.rl_device_alloc(self.ctx.handle, max(int(elements) * size, 1), ctypes.byref(p)))
        self.owned.append(p)
        return _Buffer(p, int(elements), dtype)

    def upload(self, buf, array, byte_offset=0):
        """A host array's bytes as they are (rl_device_upload_bytes)."""
        array = np.ascontiguousarray(array)
        check(lib.rl_device_upload_bytes(self.ctx.handle, ctypes.c_void_p(buf.ptr.value + byte_offset), array.ctypes.data_as(ctypes.c_void_p),
                                         array.nbytes))

    def download(self, buf, elements, element_offset=0):
        out = np.empty(int(elements), dtype=np.float64)
        check(lib.rl_device_download(self.ctx.handle, buf.at(element_offset), DTYPES[buf.dtype], int(elements), _lib.ptr(out)))
        return out

    def copy(self, dst, dst_element, src, src_element, elements):
        assert dst.dtype == src.dtype
        check(lib.rl_device_copy(self.ctx.handle, dst.at(dst_element), src.at(src_element), int(elements) * np.dtype(_NP[src.dtype]).itemsize))

    def measurement(self):
        """The plan's measurement buffer [batch][V][ny][nx] (rl_deconv_device_ptr which = 1)."""
        p, n, dt = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        check(lib.rl_deconv_device_ptr(self.plan.handle, 1, ctypes.byref(p), ctypes.byref(n), ctypes.byref(dt)))
        return _Buffer(p, self.plan.B * self.plan.V * self.plan.ny * self.plan.nx, 'f32' if dt.value == _lib.RL_F32 else 'f64')

    def ingest(self, raw, code, images, sensor, origin, frame_stride, view_stride, n_slots, n_valid, V, shape, camera, dark, dst, stats):
        """rl_ingest of a chunk's raw frames into dst (the staging buffer, not the plan's); stats: a float64 buffer [n_slots * V][4]."""
        check(lib.rl_ingest(self.ctx.handle, raw.ptr, code, images, sensor[0], sensor[1], origin[0], origin[1], frame_stride, view_stride, n_slots,
                            n_valid, V, shape[0], shape[1], None if dark is None else dark.ptr, camera.dark, camera.gain, camera.epsilon,
                            0.0 if camera.saturation is None else camera.saturation, dst.ptr, DTYPES[dst.dtype], stats.ptr))

    def repair(self, buf, n_images, ny, nx, mask, radius):
        """rl_repair_pixels on the first n_images images of buf, in place."""
        check(lib.rl_repair_pixels(self.ctx.handle, buf.ptr, DTYPES[buf.dtype], n_images, ny, nx, mask.ctypes.data_as(ctypes.c_void_p),
                                   int(radius), None))

    def sums(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M):
        """rl_register_sums: (S [pairs][(2R+1)^2][3], A [pairs][2])."""
        n = len(mov_offsets)
        W = 2 * R + 1
        ro, mo = np.ascontiguousarray(ref_offsets, dtype=np.int64), np.ascontiguousarray(mov_offsets, dtype=np.int64)
        S, A = np.empty((n, W * W, 3)), np.empty((n, 2))
        check(lib.rl_register_sums(self.ctx.handle, ref.ptr, DTYPES[ref.dtype], ro.ctypes.data_as(_I64P), mov.ptr, DTYPES[mov.dtype],
                                   mo.ctypes.data_as(_I64P), n, ny, nx, R, M, _lib.ptr(S), _lib.ptr(A)))
        return S, A

    def peaks(self, tot, n_pairs, R, n_terms, surfaces=False):
        """rl_register_peaks on a float64 device buffer of sums rows [n_pairs][(2R+1)^2 * 3 + 2]: the fields [n_pairs][5]; with
        surfaces=True (fields, surfaces [n_pairs][(2R+1)^2])."""
        P = np.empty((n_pairs, PEAK_FIELDS))
        C = np.empty((n_pairs, (2 * R + 1) ** 2)) if surfaces else None
        check(lib.rl_register_peaks(self.ctx.handle, tot.ptr, n_pairs, R, float(n_terms), _lib.ptr(P), None if C is None else _lib.ptr(C)))
        return (P, C) if surfaces else P

    def estimate(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M, refine, scratch, surfaces=False):
        """rl_register_estimate: (shifts [pairs][2], fields [pairs][3] = ncc, at_limit, flat, surfaces [pairs][(2R+1)^2] or None)."""
        n = len(mov_offsets)
        ro, mo = np.ascontiguousarray(ref_offsets, dtype=np.int64), np.ascontiguousarray(mov_offsets, dtype=np.int64)
        shifts, fields = np.empty((n, 2)), np.empty((n, 3))
        C = np.empty((n, (2 * R + 1) ** 2)) if surfaces else None
        check(lib.rl_register_estimate(self.ctx.handle, ref.ptr, DTYPES[ref.dtype], ro.ctypes.data_as(_I64P), mov.ptr, DTYPES[mov.dtype],
                                       mo.ctypes.data_as(_I64P), n, ny, nx, R, M, refine, None if scratch is None else scratch.ptr,
                                       _lib.ptr(shifts), _lib.ptr(fields), None if C is None else _lib.ptr(C)))
        return shifts, fields, C

    def xcorr(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, surfaces=False):
        """rl_register_xcorr: the fields [pairs][7]; with surfaces=True (fields, v [pairs][2R+1][2R+1] float32)."""
        n = len(mov_offsets)
        W = 2 * R + 1
        ro, mo = np.ascontiguousarray(ref_offsets, dtype=np.int64), np.ascontiguousarray(mov_offsets, dtype=np.int64)
        P = np.empty((n, XCORR_FIELDS))
        V = np.empty((n, W, W), dtype=np.float32) if surfaces else None
        check(lib.rl_register_xcorr(self.ctx.handle, ref.ptr, DTYPES[ref.dtype], ro.ctypes.data_as(_I64P), mov.ptr, DTYPES[mov.dtype],
                                    mo.ctypes.data_as(_I64P), n, ny, nx, R, _lib.ptr(P),
                                    None if V is None else V.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return (P, V) if surfaces else P

    def shift(self, src, src_element, n, ny, nx, shifts, order, floor, dst, dst_element=0):
        """rl_shift_images on n consecutive images; returns the statistics [n][2] (raised, sum)."""
        sh = np.ascontiguousarray(shifts, dtype=np.float64).reshape(n, 2)
        stats = np.empty((n, 2))
        check(lib.rl_shift_images(self.ctx.handle, src.at(src_element), DTYPES[src.dtype], n, ny, nx, _lib.ptr(sh), order,
                                  -np.inf if floor is None else float(floor), dst.at(dst_element), DTYPES[dst.dtype], _lib.ptr(stats)))
        return stats

    def gather_shift(self, src, offsets, ny, nx, shifts, dst, order=3):
        """The images at the element offsets of src, each by its shift (order 3 unless given, no floor), to consecutive images of
        dst; runs of consecutive images go through one call."""
        offsets, k = list(offsets), 0
        while k < len(offsets):
            m = 1
            while k + m < len(offsets) and offsets[k + m] == offsets[k] + m * ny * nx:
                m += 1
            self.shift(src, offsets[k], m, ny, nx, shifts[k:k + m], order, None, dst, k * ny * nx)
            k += m

    def warp(self, src, src_element, n, sy, sx, xf, order, floor, dst, dst_element, oy, ox):
        """rl_warp_images on n consecutive images of sy x sx into n images of oy x ox; xf (n, 6); returns the statistics [n][2]."""
        xf = np.ascontiguousarray(xf, dtype=np.float64).reshape(n, 6)
        stats = np.empty((n, 2))
        check(lib.rl_warp_images(self.ctx.handle, src.at(src_element), DTYPES[src.dtype], n, sy, sx, _lib.ptr(xf), order,
                                 -np.inf if floor is None else float(floor), dst.at(dst_element), DTYPES[dst.dtype], oy, ox, _lib.ptr(stats)))
        return stats

    def gather_warp(self, src, offsets, sy, sx, xf, order, dst, oy, ox):
        """The images at the element offsets of src, each through its map (no floor), to consecutive images of dst; runs of
        consecutive images go through one call."""
        offsets, k = list(offsets), 0
        while k < len(offsets):
            m = 1
            while k + m < len(offsets) and offsets[k + m] == offsets[k] + m * sy * sx:
                m += 1
            self.warp(src, offsets[k], m, sy, sx, xf[k:k + m], order, None, dst, k * oy * ox, oy, ox)
            k += m

    def affine_sums(self, ref, ref_offsets, w, w_offsets, ny, nx, M):
        """rl_affine_sums: S [pairs][45]."""
        n = len(w_offsets)
        ro, wo = np.ascontiguousarray(ref_offsets, dtype=np.int64), np.ascontiguousarray(w_offsets, dtype=np.int64)
        S = np.empty((n, AFFINE_FIELDS))
        check(lib.rl_affine_sums(self.ctx.handle, ref.ptr, DTYPES[ref.dtype], ro.ctypes.data_as(_I64P), w.ptr, DTYPES[w.dtype],
                                 wo.ctypes.data_as(_I64P), n, ny, nx, M, _lib.ptr(S)))
        return S

    def iterate(self, iterations):
        """The measurement buffer was written on the device: from ones, `iterations` iterations; returns the estimates (B, ny, nx)."""
        check(lib.rl_deconv_measurement_written(self.plan.handle))
        check(lib.rl_deconv_reset_estimate(self.plan.handle))
        check(lib.rl_deconv_iterate(self.plan.handle, int(iterations)))
        return self.plan.estimate()

    def unresolved(self):
        return self.plan.unresolved()

    def strategy(self):
        return self.plan.strategy()

    def close(self):
        for p in self.owned:
            lib.rl_device_free(self.ctx.handle, p)
        self.owned = []


def _float_images(a, name):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError('%s must be float32 or float64 (taken without conversion); got %s' % (name, a.dtype))
    return np.ascontiguousarray(a), ('f32' if a.dtype == np.float32 else 'f64')


# ---- public ----------------------------------------------------------------------------------------------------------------------------
def _pairs_on_device(images, reference):
    images, dt = _float_images(images, 'images')
    reference, rdt = _float_images(reference, 'reference')
    if images.ndim == 2:
        images = images[None]
    if images.ndim != 3 or 0 in images.shape:
        raise ValueError('images: expected (N, ny, nx) or (ny, nx); got shape %s' % (images.shape,))
    N, ny, nx = images.shape
    if reference.shape not in ((ny, nx), (N, ny, nx)):
        raise ValueError('reference: expected %s or %s; got shape %s' % ((ny, nx), (N, ny, nx), reference.shape))
    return images, dt, reference, rdt


def coarse_shifts(images, reference, radius, device=None, surfaces=False):
    """The integer displacement of every image relative to its reference from the FFT cross-correlation over [-radius, radius]^2
    (rl_register_xcorr): a proposal for any drift radius at the cost of a few transforms per pair, to be judged by the exact window
    (estimate_shifts(coarse=radius) does both).  images, reference: as for estimate_shifts; radius: 1 .. min(ny, nx) / 2 with
    ny + radius and nx + radius <= 1152.  Returns (c (N, 2) int64 (dy, dx), info) with info['value'] (the overlap-normalised
    covariance at the peak), 'snr' ((peak - window mean) / window standard deviation: a peak that does not stand out of its window
    is not to be trusted), 'flat' (an image without variance: c = 0) and, with surfaces=True, 'surfaces' (N, W, W) float32."""
    images, dt, reference, rdt = _pairs_on_device(images, reference)
    N, ny, nx = images.shape
    if int(radius) != radius or not 1 <= int(radius) <= min(ny, nx) // 2:
        raise ValueError('radius must lie in 1 .. min(ny, nx) / 2 = %d; got %r' % (min(ny, nx) // 2, radius))
    radius = int(radius)
    if ny + radius > XCORR_MAX_LENGTH or nx + radius > XCORR_MAX_LENGTH:
        raise ValueError('the coarse stage serves image side + radius <= %d; got %d x %d with radius %d' % (XCORR_MAX_LENGTH, ny, nx, radius))
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        mov, ref = dev.alloc(images.size, dt), dev.alloc(reference.size, rdt)
        dev.upload(mov, images)
        dev.upload(ref, reference)
        n_pix = ny * nx
        out = dev.xcorr(ref, [i * n_pix if reference.ndim == 3 else 0 for i in range(N)], mov, [i * n_pix for i in range(N)], ny, nx, radius, surfaces)
        c, value, snr, flat = coarse_fields(out[0] if surfaces else out, radius)
        info = {'value': value, 'snr': snr, 'flat': flat}
        if surfaces:
            info['surfaces'] = out[1]
        return c, info
    finally:
        dev.close()


def estimate_shifts(images, reference, max_shift=8, refine=1, margin=None, device=None, surfaces=False, coarse=None, device_peaks=False):
    """The translation of every image relative to its reference.  images: (N, ny, nx) or (ny, nx), float32 or float64; reference:
    (ny, nx), shared, or (N, ny, nx).  max_shift: the search radius in pixels, 1 .. 32.  refine: passes that shift the image by
    the current estimate (order 3) and add the parabola offset of a 3 x 3 window.  margin: pixels at every border kept out of the
    sums (default, and at least with refine > 0, max_shift + 2).  Returns (shifts (N, 2) float64 (dy, dx), info) with info['ncc']
    (the peak value), 'at_limit' (the integer peak lay on the window's border: no sub-pixel part, the drift may be larger), 'flat' (an
    image without variance: shift 0) and, with surfaces=True, 'surfaces' (N, W, W).
    coarse: None -- the window alone, as above -- or a radius Rc: rl_register_xcorr proposes an integer displacement c within Rc
    pixels (any Rc with ny + Rc, nx + Rc <= 1152), the moving image displaced by c (order 1: a copy of the displaced pixels) goes
    through the window of radius max_shift, shift = c + peak + parabola, and the refine passes shift the ORIGINAL image by the
    total, so no image is interpolated twice.  Pair i keeps 8 ceil(|c_i| / 8) + max_shift + 2 pixels out of its sums (the
    mirror-filled band of the copy), so ny - 2 (Rc + max_shift + 2) >= 8 is required, likewise nx, and margin cannot be given.
    at_limit then says that the PROPOSAL was wrong (the fine peak lay on the border of the window around c), not that the drift was
    large.  info gains 'coarse' (N, 2) int64, 'coarse_value', 'coarse_snr', 'coarse_flat' (coarse_shifts).
    device_peaks: True -- the NCC, the first maximum and the parabola on the device (rl_register_estimate: the whole estimate in one
    call, 5 doubles per pair come down instead of the sums); the same bits as the default.  Not with coarse."""
    if device_peaks and coarse is not None:
        raise ValueError('device_peaks serves the window alone: coarse must be None')
    images, dt, reference, rdt = _pairs_on_device(images, reference)
    N, ny, nx = images.shape
    given_margin = margin
    max_shift, refine, margin = _check_search(ny, nx, max_shift, refine, None if coarse is not None else margin)
    coarse = _check_coarse(ny, nx, coarse, max_shift, given_margin)
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        mov, ref = dev.alloc(images.size, dt), dev.alloc(reference.size, rdt)
        dev.upload(mov, images)
        dev.upload(ref, reference)
        scratch = dev.alloc(images.size, 'f64') if refine or coarse is not None else None
        n_pix = ny * nx
        args = (dev, ref, [i * n_pix if reference.ndim == 3 else 0 for i in range(N)], mov, [i * n_pix for i in range(N)], ny, nx,
                max_shift, refine, margin, scratch, surfaces)
        return _estimate_on_device(*args) if device_peaks else _estimate(*args, coarse)
    finally:
        dev.close()


def shift_images(images, shifts, order=3, floor=None, device=None):
    """max(scipy.ndimage.shift(images[i], -shifts[i], order=order, mode='mirror'), floor) for every image, on the device: image i
    sampled at (y + sy_i, x + sx_i) -- shifts as estimate_shifts returns them undo the displacement.  images: (N, ny, nx) or (ny, nx),
    float32 or float64; the result has the same dtype (computed in float64, rounded once).  order: 3 (cubic B-spline) or 1 (bilinear;
    with integer shifts a bit-exact copy of the displaced pixels).  floor: None or the least value of the output."""
    images, dt = _float_images(images, 'images')
    single = images.ndim == 2
    if single:
        images = images[None]
    if images.ndim != 3 or 0 in images.shape:
        raise ValueError('images: expected (N, ny, nx) or (ny, nx); got shape %s' % (images.shape,))
    N, ny, nx = images.shape
    shifts = np.asarray(shifts, dtype=np.float64)
    if shifts.shape != ((2,) if single else (N, 2)) and shifts.shape != (N, 2):
        raise ValueError('shifts: expected shape %s; got %s' % ((N, 2), shifts.shape))
    if not np.all(np.isfinite(shifts)):
        raise ValueError('shifts must be finite')
    if order not in (1, 3):
        raise ValueError('order must be 1 or 3; got %r' % (order,))
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        src, dst = dev.alloc(images.size, dt), dev.alloc(images.size, dt)
        dev.upload(src, images)
        dev.shift(src, 0, N, ny, nx, shifts.reshape(N, 2), order, floor, dst)
        out = dev.download(dst, images.size).astype(images.dtype).reshape(images.shape)      # (exact: the values are of that type)
        return out[0] if single else out
    finally:
        dev.close()


def _check_transforms(transforms, shape, name='transforms'):
    T = np.asarray(transforms, dtype=np.float64)
    if T.shape != shape or not np.all(np.isfinite(T)):
        raise ValueError('%s: expected finite values of shape %s; got shape %s' % (name, shape, T.shape))
    return T


def warp_images(images, transforms, order=3, floor=None, output_shape=None, device=None):
    """max(scipy.ndimage.affine_transform(images[i], L_i, offset=c + t_i - L_i c, output_shape=..., order=order, mode='mirror'),
    floor) for every image, on the device (rl_warp_images): image i sampled at T_i(x) = c + L_i (x - c) + t_i -- transforms as
    estimate_transforms returns them undo the rotation, scale and displacement.  images: (N, ny, nx) or (ny, nx), float32 or float64;
    transforms: (N, 2, 3) or (2, 3) in the centred form [L | t], c = ((ny - 1) / 2, (nx - 1) / 2) of the IMAGE.  The result has the
    images' dtype (computed in float64, rounded once) and output_shape (default: the images').  order: 3 (cubic B-spline) or 1
    (bilinear; with L = I and integer t a bit-exact copy of the displaced pixels).  floor: None or the least value of the output."""
    images, dt = _float_images(images, 'images')
    single = images.ndim == 2
    if single:
        images = images[None]
    if images.ndim != 3 or 0 in images.shape:
        raise ValueError('images: expected (N, ny, nx) or (ny, nx); got shape %s' % (images.shape,))
    N, ny, nx = images.shape
    T = np.asarray(transforms, dtype=np.float64)
    T = _check_transforms(T[None] if T.ndim == 2 else T, (N, 2, 3))
    if order not in (1, 3):
        raise ValueError('order must be 1 or 3; got %r' % (order,))
    if floor is not None and np.isnan(floor):
        raise ValueError('floor is nan')
    oy, ox = (ny, nx) if output_shape is None else (int(output_shape[0]), int(output_shape[1]))
    if oy < 1 or ox < 1:
        raise ValueError('output_shape must be at least 1 x 1; got %r' % (output_shape,))
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        src, dst = dev.alloc(images.size, dt), dev.alloc(N * oy * ox, dt)
        dev.upload(src, images)
        dev.warp(src, 0, N, ny, nx, transform_matrix_offset(T, (ny, nx)), order, floor, dst, 0, oy, ox)
        out = dev.download(dst, N * oy * ox).astype(images.dtype).reshape(N, oy, ox)      # (exact: the values are of that type)
        return out[0] if single else out
    finally:
        dev.close()


def estimate_transforms(images, reference, model='rigid', passes=5, min_side=48, margin=4, init=None, device=None):
    """The transform [L | t] of every image relative to its reference, B(c + L (x - c) + t) ~ A(x), by Gauss-Newton on the
    intensities over a pyramid.  images: (N, ny, nx) or (ny, nx), float32 or float64; reference: (ny, nx), shared, or (N, ny, nx).
    model: 'translation', 'rigid' (rotation), 'similarity' (rotation and isotropic scale) or 'affine'; a gain and an offset between
    the two images are solved with the geometry in every model.  The pyramid: 2 x 2 binning of both images while the halved
    shorter side is at least min_side.  Per level, coarsest first, `passes` passes of: warp by the current transform (order 3),
    rl_affine_sums, solve_transform, update_transform; there is no data-dependent exit.  margin: pixels at every border kept out of
    the sums at every level (min_side >= 2 margin + 8).  init: None or shifts (N, 2) from estimate_shifts -- needed where the
    displacement exceeds a few pixels of the coarsest level.  Returns (transforms (N, 2, 3), info) with info['gain'], 'offset',
    'residual' (root of the residual over the reference's centred sum of squares) and 'step' (the last step's largest corner
    displacement in pixels: small where the iteration has settled), each (N,), 'flat' (N,) -- a singular or ill-conditioned system or
    a gain that is not positive: the identity is returned for that pair -- and 'levels'."""
    images, dt, reference, rdt = _pairs_on_device(images, reference)
    N, ny, nx = images.shape
    passes, min_side, margin = _check_model(ny, nx, model, passes, min_side, margin)
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        if init.shape not in ((N, 2), (2,)) or not np.all(np.isfinite(init)):
            raise ValueError('init: expected finite shifts of shape %s; got %s' % ((N, 2), init.shape))
        init = np.broadcast_to(init, (N, 2))
    dev = _Device(device=_lib.DEFAULT_DEVICE if device is None else device)
    try:
        mov, ref = dev.alloc(images.size, dt), dev.alloc(reference.size, rdt)
        dev.upload(mov, images)
        dev.upload(ref, reference)
        n_pix = ny * nx
        return _estimate_transforms(dev, ref, [i * n_pix if reference.ndim == 3 else 0 for i in range(N)], mov, [i * n_pix for i in range(N)],
                                    ny, nx, model, passes, min_side, margin, init)
    finally:
        dev.close()


def deconvolve_stack_registered(raw, psfs, iterations, camera=None, order='frame-view', roi=None, dtype='f32', batch=None, shifts=None,
                                register=('views', 'frames'), max_shift=8, refine=1, interp=3, acceleration=None, tv_lambda=None,
                                tv_epsilon=0.1, device=None, coarse=None, pipeline=False, out_dtype=None, out_scale=1.0, out=None,
                                model='translation', view_transforms=None):
    """deconvolve_stack with every image registered on the device before the iterations.  raw, camera, order, roi, dtype, batch,
    acceleration, tv_lambda, tv_epsilon: exactly those of deconvolve_stack.
    register: 'frames' in it -- image (f, v) is registered to image (0, v), the same PSF: drift over time; 'views' in it -- image
    (0, v) is registered to image (0, 0) (every PSF here is point-symmetric, so the correlation of two different blurs of one object
    still peaks at the true displacement); the shift applied to (f, v) is the sum of the two.  shifts: an (F, V, 2) array skips the
    estimation.  max_shift, refine, coarse: as for estimate_shifts (the margin is max_shift + 2; with coarse=Rc both the view and the
    frame estimates take the coarse stage first -- drift of any size up to Rc -- and info gains 'coarse' (F, V, 2), 'coarse_snr'
    (F, V), 'view_coarse' (V, 2), 'view_coarse_snr' (V,); given shifts=, no coarse call is made).  interp: 3 (cubic B-spline) or 1
    (bilinear); interpolating noisy counts correlates neighbouring pixels -- where the Poisson statistics must be kept exactly, run
    once for info['shifts'] and again with shifts=np.rint(...) and interp=1, which only moves pixels.
    Per chunk of `batch` frames, on the context's stream: upload of the raw bytes, rl_ingest into a staging buffer, the estimate,
    rl_shift_images (floor = camera.epsilon) into the plan's measurement buffer, the iterations from ones, download.  The ingested
    images of frame 0 stay on the device as the references for the whole call.  With pipeline=False (the default) there is NO overlap
    of transfers with the iterations and no u16 export: the estimates come back as float64.
    pipeline=True: the same steps in the overlapped chunk pipeline of deconvolve_stack (rl_stack_run_registered): uploads and
    downloads on copy streams beside the estimates and the iterations, the NCC and the peaks on the device (rl_register_estimate), and
    the narrow export -- out_dtype 'f32' (default), 'f64' or 'u16', out_scale and out exactly as for deconvolve_stack (page-locked
    raw and out arrays are copied to and from directly).  The shifts, the fields and, with out_dtype='f64', the estimates are the bits
    of pipeline=False.  Not with coarse; out_dtype, out_scale and out only with pipeline=True.
    model: 'translation' (the default: everything above, call for call), or 'rigid', 'similarity', 'affine' -- the views of a line
    scan differ by a residual rotation and magnification that no shift undoes: image (0, v) is registered to (0, 0) with
    estimate_transforms(model) (5 passes, min_side 48, margin 4) in place of the view shift, the frames (f, v) to (0, v) by translation
    as above, the two are composed to [L_v | t_v + d_fv], and ONE rl_warp_images (order interp, floor camera.epsilon) per image writes
    the plan's measurement.  view_transforms: (V, 2, 3) skips the view estimate -- a calibration measured once on beads or a test
    target; a chunk whose L are all exactly the identity goes through rl_shift_images, so identities give the bits of the translation
    path.  With shifts= given they are the frame shifts d.  No flux rescaling by |det L| is applied.  Not with pipeline=True.  info
    gains 'transforms' (F, V, 2, 3) as applied ('shifts' is their t), 'view_transforms' (V, 2, 3) and 'view_fit' (the info of
    estimate_transforms for views 1 .., or None); 'view_flat' marks a view whose fit was flat (it gets the identity).
    Returns (estimates (F, ny, nx) float64 -- pipeline: of out_dtype --, info); info: the ingest statistics of deconvolve_stack
    ('level', 'clipped', 'saturated', 'invalid', each (F, V)), 'shifts' (F, V, 2) as applied, 'ncc', 'at_limit', 'flat' (F, V) of the
    frame estimates, 'view_ncc', 'view_at_limit', 'view_flat' (V,) of the view estimates, 'raised' (F, V) pixels raised to
    camera.epsilon by the shift, 'unresolved', 'strategy', 'chunks', 'batch'; pipeline: also 'clamped' (F,) as deconvolve_stack and
    'times_ms' (wall_ms, upload_ms, compute_ms, download_ms, estimate_ms)."""
    _lib.tv_params(tv_lambda, tv_epsilon)
    _lib.accel_mode(acceleration)
    if dtype not in DTYPES:
        raise ValueError("dtype must be 'f32' or 'f64'; got %r" % (dtype,))
    if order not in ORDERS:
        raise ValueError("order must be 'frame-view' or 'view-frame'; got %r" % (order,))
    if interp not in (1, 3):
        raise ValueError('interp must be 1 or 3; got %r' % (interp,))
    register = (register,) if isinstance(register, str) else tuple(register)
    if any(r not in ('views', 'frames') for r in register):
        raise ValueError("register: any of 'views', 'frames'; got %r" % (register,))
    if model not in MODELS:
        raise ValueError('model: one of %s; got %r' % (', '.join(MODELS), model))
    affine = model != 'translation' or view_transforms is not None
    if affine and pipeline:
        raise ValueError("pipeline=True serves translations alone: model must be 'translation' and view_transforms None")
    if pipeline:
        if coarse is not None:
            raise ValueError('pipeline=True serves the window alone: coarse must be None')
        out_dtype = 'f32' if out_dtype is None else out_dtype
        if out_dtype not in OUT_DTYPES:
            raise ValueError("out_dtype must be 'f32', 'f64' or 'u16'; got %r" % (out_dtype,))
    elif out_dtype is not None or out_scale != 1.0 or out is not None:
        raise ValueError('out_dtype, out_scale and out need pipeline=True')
    code = raw_code(raw)
    raw = np.ascontiguousarray(raw)
    if 0 in raw.shape:
        raise ValueError('raw is empty: shape %s' % (raw.shape,))
    V = len(psfs)
    F, sy, sx = _stack_shape(raw, V, order)
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
    given = None
    if shifts is not None:
        given = np.asarray(shifts, dtype=np.float64)
        if given.shape != (F, V, 2) or not np.all(np.isfinite(given)):
            raise ValueError('shifts: expected finite values of shape %s; got shape %s' % ((F, V, 2), given.shape))
    elif register:
        max_shift, refine, margin = _check_search(ny, nx, max_shift, refine, None)
        coarse = _check_coarse(ny, nx, coarse, max_shift, None)
    estimating = given is None and bool(register)
    view_T, view_fit = identity_transforms(V), None
    if view_transforms is not None:
        view_T = _check_transforms(view_transforms, (V, 2, 3), 'view_transforms').copy()
    elif affine and given is None and 'views' in register and V > 1:
        _check_model(ny, nx, model, 5, 48, 4)
    if pipeline:
        return _registered_pipeline(raw, code, psfs, int(iterations), camera, order, (sy, sx), (y0, x0, ny, nx), dtype, batch, given, register,
                                    max_shift, refine, interp, acceleration, tv_lambda, tv_epsilon,
                                    _lib.DEFAULT_DEVICE if device is None else device, out_dtype, out_scale, out)
    frames = raw.reshape((F, V, sy, sx) if order == 'frame-view' else (V, F, sy, sx))
    n_pix, img_bytes = ny * nx, sy * sx * raw.dtype.itemsize
    dev = _Device(psfs, batch, (ny, nx), dtype, _lib.DEFAULT_DEVICE if device is None else device, acceleration, tv_lambda, tv_epsilon)
    try:
        raw_dev = dev.alloc(batch * V * img_bytes, None)
        staging, refs = dev.alloc(batch * V * n_pix, dtype), dev.alloc(V * n_pix, dtype)
        stats_dev = dev.alloc(batch * V * INGEST_FIELDS, 'f64')
        scratch = dev.alloc(batch * V * n_pix, 'f64') if estimating and (refine or coarse is not None) else None
        dark = None
        if camera.dark_map is not None:
            dark = dev.alloc(n_pix, 'f32')
            dev.upload(dark, camera.dark_map)
        meas = dev.measurement()
        out = np.empty((F, ny, nx))
        ingest_stats, applied, raised = np.zeros((F, V, INGEST_FIELDS)), np.zeros((F, V, 2)), np.zeros((F, V), dtype=np.int64)
        value, at_limit, flat = np.zeros((F, V)), np.zeros((F, V), dtype=bool), np.zeros((F, V), dtype=bool)
        transforms = identity_transforms(F * V).reshape(F, V, 2, 3)
        view_shift, view_info = np.zeros((V, 2)), {'ncc': np.zeros(V), 'at_limit': np.zeros(V, dtype=bool), 'flat': np.zeros(V, dtype=bool)}
        use_coarse = coarse if estimating else None
        coarse_c, coarse_snr = np.zeros((F, V, 2), dtype=np.int64), np.zeros((F, V))
        view_coarse, view_coarse_snr = np.zeros((V, 2), dtype=np.int64), np.zeros(V)
        for first in range(0, F, batch):
            nt = min(batch, F - first)
            if order == 'frame-view':                            # one piece [nt][V]
                dev.upload(raw_dev, frames[first:first + nt])
                fs, vs = V, 1
            else:                                                # V pieces [nt], view v of the chunk at device image v * nt
                for v in range(V):
                    dev.upload(raw_dev, frames[v, first:first + nt], v * nt * img_bytes)
                fs, vs = 1, nt
            dev.ingest(raw_dev, code, nt * V, (sy, sx), (y0, x0), fs, vs, batch, nt, V, (ny, nx), camera, dark, staging, stats_dev)
            if camera.defects is not None:
                dev.repair(staging, batch * V, ny, nx, camera.defects, camera.repair_radius)
            ingest_stats[first:first + nt] = dev.download(stats_dev, nt * V * INGEST_FIELDS).reshape(nt, V, INGEST_FIELDS)
            if first == 0:
                dev.copy(refs, 0, staging, 0, V * n_pix)
            chunk = np.zeros((batch, V, 2))                      # (fillers: no shift)
            if given is not None:
                chunk[:nt] = given[first:first + nt]
            else:
                if first == 0 and 'views' in register and V > 1 and affine:
                    if view_transforms is None:
                        view_T[1:], view_fit = _estimate_transforms(dev, refs, [0] * (V - 1), refs, [v * n_pix for v in range(1, V)], ny, nx,
                                                                   model, 5, 48, 4)
                        view_info['flat'][1:] = view_fit['flat']
                elif first == 0 and 'views' in register and V > 1:
                    view_shift[1:], vi = _estimate(dev, refs, [0] * (V - 1), refs, [v * n_pix for v in range(1, V)], ny, nx, max_shift, refine,
                                                   margin, scratch, coarse=use_coarse)
                    for k in view_info:
                        view_info[k][1:] = vi[k]
                    if use_coarse is not None:
                        view_coarse[1:], view_coarse_snr[1:] = vi['coarse'], vi['coarse_snr']
                if 'frames' in register:
                    pairs = [(f, v) for f in range(nt) for v in range(V) if first + f > 0]      # (frame 0 is its own reference)
                    if pairs:
                        s, fi = _estimate(dev, refs, [v * n_pix for _, v in pairs], staging, [(f * V + v) * n_pix for f, v in pairs], ny, nx,
                                          max_shift, refine, margin, scratch, coarse=use_coarse)
                        for k, (f, v) in enumerate(pairs):
                            chunk[f, v] = s[k]
                            if use_coarse is not None:
                                coarse_c[first + f, v], coarse_snr[first + f, v] = fi['coarse'][k], fi['coarse_snr'][k]
                            value[first + f, v], at_limit[first + f, v], flat[first + f, v] = fi['ncc'][k], fi['at_limit'][k], fi['flat'][k]
                chunk[:nt] += view_shift
            if affine:                                           # frame shift o view transform: [L_v | t_v + d_fv], ONE interpolation
                Tc = np.broadcast_to(view_T, (batch, V, 2, 3)).copy()
                Tc[..., 2] += chunk
                transforms[first:first + nt] = Tc[:nt]
                chunk = Tc[..., 2]
                if np.any(Tc[..., :2] != np.eye(2)):
                    st = dev.warp(staging, 0, batch * V, ny, nx, transform_matrix_offset(Tc.reshape(-1, 2, 3), (ny, nx)), interp, camera.epsilon,
                                  meas, 0, ny, nx)
                else:                                            # translations alone: the shift's fused passes, the bits of that path
                    st = dev.shift(staging, 0, batch * V, ny, nx, chunk.reshape(-1, 2), interp, camera.epsilon, meas)
            else:
                st = dev.shift(staging, 0, batch * V, ny, nx, chunk.reshape(-1, 2), interp, camera.epsilon, meas)
            applied[first:first + nt] = chunk[:nt]
            raised[first:first + nt] = st[:, 0].reshape(batch, V)[:nt].astype(np.int64)
            out[first:first + nt] = dev.iterate(iterations)[:nt]
        info = {'level': ingest_stats[:, :, 0].copy(), 'clipped': ingest_stats[:, :, 1].astype(np.int64),
                'saturated': ingest_stats[:, :, 2].astype(np.int64), 'invalid': ingest_stats[:, :, 3].astype(np.int64),
                'shifts': applied, 'ncc': value, 'at_limit': at_limit, 'flat': flat, 'view_ncc': view_info['ncc'],
                'view_at_limit': view_info['at_limit'], 'view_flat': view_info['flat'], 'raised': raised,
                'unresolved': dev.unresolved(), 'strategy': dev.strategy(), 'chunks': -(-F // batch), 'batch': batch}
        info.update(camera.defect_info())
        if affine:
            info.update({'transforms': transforms, 'view_transforms': view_T, 'view_fit': view_fit})
        if use_coarse is not None:
            info.update({'coarse': coarse_c, 'coarse_snr': coarse_snr, 'view_coarse': view_coarse, 'view_coarse_snr': view_coarse_snr})
        return out, info
    finally:
        dev.close()


class _RegisterParams(ctypes.Structure):      # rl_stack_register of include/rlsted.h
    _fields_ = [('views', ctypes.c_int), ('frames', ctypes.c_int), ('max_shift', ctypes.c_int), ('refine', ctypes.c_int),
                ('interp', ctypes.c_int)]


class _RegisterOut(ctypes.Structure):         # rl_stack_register_out
    _fields_ = [(k, ctypes.POINTER(ctypes.c_double)) for k in ('shifts', 'fields', 'view_shifts', 'view_fields', 'raised')]


def _registered_pipeline(raw, code, psfs, iterations, camera, order, sensor, window, dtype, batch, given, register, max_shift, refine, interp,
                         acceleration, tv_lambda, tv_epsilon, device, out_dtype, out_scale, out):
    """deconvolve_stack_registered(pipeline=True) after its checks: one rl_stack_run_registered over the whole stack."""
    y0, x0, ny, nx = window
    V = len(psfs)
    F = _stack_shape(raw, V, order)[0]
    out_code, out_np = OUT_DTYPES[out_dtype]
    if out is None:
        out = np.empty((F, ny, nx), dtype=out_np)
    elif out.dtype != out_np or not out.flags.c_contiguous or out.shape != (F, ny, nx):
        raise ValueError('out must be a C-contiguous %s array of shape %s' % (np.dtype(out_np).name, (F, ny, nx)))
    dev = stack._Device(psfs, batch, (ny, nx), dtype, device, acceleration, tv_lambda, tv_epsilon)
    try:
        dev.open(code, ORDERS[order], sensor, (y0, x0), camera, out_code, out_scale)
        if camera.defects is not None:
            dev.set_defects(camera.defects, camera.repair_radius)
        ingest_stats, export_stats, times = np.zeros((F, V, INGEST_FIELDS)), np.zeros((F, EXPORT_FIELDS)), np.zeros(5)
        shifts, fields, raised = np.zeros((F, V, 2)), np.zeros((F, V, 3)), np.zeros((F, V))
        view_shifts, view_fields = np.zeros((V, 2)), np.zeros((V, 3))
        params = _RegisterParams(int('views' in register), int('frames' in register), int(max_shift), int(refine), int(interp))
        reg_out = _RegisterOut(*[_lib.ptr(a) for a in (shifts, fields, view_shifts, view_fields, raised)])
        dev.run_registered(raw, F, iterations, params, None if given is None else np.ascontiguousarray(given, dtype=np.float64), out,
                           ingest_stats, export_stats, reg_out, times)
        info = {'level': ingest_stats[:, :, 0].copy(), 'clipped': ingest_stats[:, :, 1].astype(np.int64),
                'saturated': ingest_stats[:, :, 2].astype(np.int64), 'invalid': ingest_stats[:, :, 3].astype(np.int64),
                'shifts': shifts, 'ncc': fields[:, :, 0].copy(), 'at_limit': fields[:, :, 1] != 0.0, 'flat': fields[:, :, 2] != 0.0,
                'view_ncc': view_fields[:, 0].copy(), 'view_at_limit': view_fields[:, 1] != 0.0, 'view_flat': view_fields[:, 2] != 0.0,
                'raised': raised.astype(np.int64), 'unresolved': dev.unresolved(), 'strategy': dev.strategy(), 'chunks': -(-F // batch),
                'batch': batch, 'clamped': export_stats[:, 1].astype(np.int64),
                'times_ms': dict(zip(('wall_ms', 'upload_ms', 'compute_ms', 'download_ms', 'estimate_ms'), times.tolist()))}
        info.update(camera.defect_info())
        return out, info
    finally:
        dev.close()
