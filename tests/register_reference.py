"""Twin of the registration path (include/rlsted.h rl_register_sums, rl_shift_images; rescan_line_sted_amd/registration.py): the
correlation sums in numpy long double with the bound the float64 fixed-order sums are held to, NCC, peak and parabola as specified,
the shift through scipy.ndimage.shift(mode='mirror'), and an analytic scene whose true displacement involves no interpolation.
TEST INFRASTRUCTURE ONLY.

The bound.  u = 2^-53, gamma_k = k u / (1 - k u).  Every value is exact in float64 (a float32 widens without rounding).  A sum of N
terms t_i -- b, or the exact products b b and a b, which enter through ONE fused multiply-add each -- takes one rounding per term
whatever the order (thread, strips, totals are ONE summation order of the N terms; adding the 0.0 of an empty strip is exact), so
    |S^ - S| <= gamma_N sum |t_i|,       N = (ny - 2 M)(nx - 2 M)
for S_b, S_bb, S_ab, S_a and S_aa alike.  (The twin's own long double error, N 2^-64 sum |t_i|, is 2^-11 of that.)
"""
import numpy as np
from scipy import ndimage

U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


def sums(a, b, R, M):
    """(S [W*W][3] long double, ref [2] long double, bound [W*W][3] float64, ref_bound [2]) of one pair of 2-D arrays."""
    ny, nx = a.shape
    al = np.asarray(a, dtype=np.float64).astype(LD)[M:ny - M, M:nx - M]
    bl = np.asarray(b, dtype=np.float64).astype(LD)
    W = 2 * R + 1
    n = al.size
    S, bound = np.zeros((W * W, 3), dtype=LD), np.zeros((W * W, 3))
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            w = bl[M + dy:ny - M + dy, M + dx:nx - M + dx]
            k = (dy + R) * W + dx + R
            S[k] = [w.sum(), (w * w).sum(), (al * w).sum()]
            bound[k] = [float(np.abs(w).sum()), float((w * w).sum()), float(np.abs(al * w).sum())]
    ref = np.array([al.sum(), (al * al).sum()], dtype=LD)
    ref_bound = gamma(n) * np.array([float(np.abs(al).sum()), float((al * al).sum())])
    return S, ref, gamma(n) * bound, ref_bound


def ncc(S, ref, n):
    """NCC(d) in float64 from float64 sums, as the product forms it; (surface [W][W], flat)."""
    S = np.asarray(S, dtype=np.float64)
    sa, saa = float(ref[0]), float(ref[1])
    W = int(round(np.sqrt(S.shape[0])))
    va = saa - sa * sa / n
    vb = S[:, 1] - S[:, 0] * S[:, 0] / n
    if not va > 0.0 or not np.all(vb > 0.0):
        return np.zeros((W, W)), True
    return ((S[:, 2] - sa * S[:, 0] / n) / np.sqrt(va * vb)).reshape(W, W), False


def peak(c):
    """(dy, dx) with the parabola added, the integer peak, its value, at_limit; the first maximum in row-major order."""
    W = c.shape[0]
    R = W // 2
    k = int(np.argmax(c))
    iy, ix = divmod(k, W)
    if iy in (0, W - 1) or ix in (0, W - 1):
        return np.array([iy - R, ix - R], dtype=np.float64), (iy - R, ix - R), float(c[iy, ix]), True
    out = []
    for m, z, p in ((c[iy - 1, ix], c[iy, ix], c[iy + 1, ix]), (c[iy, ix - 1], c[iy, ix], c[iy, ix + 1])):
        den = m - 2.0 * z + p
        out.append(0.5 * (m - p) / den if den != 0.0 else 0.0)
    return np.array([iy - R + out[0], ix - R + out[1]]), (iy - R, ix - R), float(c[iy, ix]), False


def shift(src, s, order=3, floor=None):
    """max(scipy.ndimage.shift(src, (-sy, -sx), order, mode='mirror'), floor) in float64."""
    out = ndimage.shift(np.asarray(src, dtype=np.float64), (-s[0], -s[1]), order=order, mode='mirror')
    return out if floor is None else np.maximum(out, floor)


def estimate(image, reference, max_shift=8, refine=1, margin=None):
    """The twin of estimate_shifts for one pair: (shift [2], info)."""
    ny, nx = reference.shape
    M = max_shift + 2 if margin is None else margin
    n = (ny - 2 * M) * (nx - 2 * M)
    S, ref, _, _ = sums(reference, image, max_shift, M)
    c, flat = ncc(S.astype(np.float64), ref.astype(np.float64), n)
    if flat:
        return np.zeros(2), dict(flat=True, at_limit=False, ncc=0.0, integer=(0, 0), surface=c)
    s, integer, value, at_limit = peak(c)
    for _ in range(refine):
        moved = shift(image, s, 3)
        S1, ref1, _, _ = sums(reference, moved, 1, M)
        c1, flat1 = ncc(S1.astype(np.float64), ref1.astype(np.float64), n)
        if flat1:
            break
        ds, _, value, _ = peak(c1)
        s = s + ds
    return s, dict(flat=False, at_limit=at_limit, ncc=value, integer=integer, surface=c)


def margin_of(c):
    """Best minus second-best value of a correlation surface."""
    v = np.sort(c.ravel())
    return float(v[-1] - v[-2])


# ---- the analytic scene ------------------------------------------------------------------------------------------------------------
def blobs(seed, ny, nx, count=14):
    """Blob parameters: centres inside the image, anisotropic widths, an orientation, an amplitude."""
    rng = np.random.default_rng(seed)
    return dict(cy=rng.uniform(0.15 * ny, 0.85 * ny, count), cx=rng.uniform(0.15 * nx, 0.85 * nx, count),
                sy=rng.uniform(1.2, 3.0, count), sx=rng.uniform(1.2, 3.0, count), th=rng.uniform(0, np.pi, count),
                amp=rng.uniform(50.0, 400.0, count), ny=ny, nx=nx)


def scene(p, d=(0.0, 0.0), blur=(0.0, 0.0), background=20.0):
    """The blobs on a constant background with their content displaced by d -- B[y + d] = A[y]: evaluated at displaced centres, no
    interpolation -- each blob's covariance widened by diag(blur)^2 (a different anisotropic, point-symmetric PSF)."""
    y, x = np.mgrid[0:p['ny'], 0:p['nx']].astype(np.float64)
    out = np.full((p['ny'], p['nx']), background)
    for cy, cx, sy, sx, th, amp in zip(p['cy'], p['cx'], p['sy'], p['sx'], p['th'], p['amp']):
        c, s = np.cos(th), np.sin(th)
        cov = np.array([[c * c * sy * sy + s * s * sx * sx, c * s * (sy * sy - sx * sx)], [c * s * (sy * sy - sx * sx), s * s * sy * sy + c * c * sx * sx]])
        base = np.sqrt(np.linalg.det(cov))
        cov = cov + np.diag([blur[0] ** 2, blur[1] ** 2])
        inv = np.linalg.inv(cov)
        dy, dx = y - (cy + d[0]), x - (cx + d[1])
        out += amp * base / np.sqrt(np.linalg.det(cov)) * np.exp(-0.5 * (inv[0, 0] * dy * dy + 2 * inv[0, 1] * dy * dx + inv[1, 1] * dx * dx))
    return out


DISPLACEMENTS = [(0.0, 0.0), (0.5, -0.5), (2.3, -3.7), (-4.25, 1.6), (3.9, 4.4), (-0.1, 0.9)]
SCENES = [(3, 48, 64), (5, 96, 80)]          # (seed, ny, nx)


# ---- the benefit case: two views of one object, the second displaced ------------------------------------------------------------
BENEFIT_DISPLACEMENT = (2.3, -3.7)
BENEFIT_FACTOR = 25.4         # unregistered / registered error of the oracle on the twin's registration (tests/test_register_cpu.py)


def gaussian_psf(sy, sx, size=9):
    """A point-symmetric anisotropic Gaussian PSF (1, size, size), normalised."""
    r = np.arange(size) - size // 2
    p = np.exp(-0.5 * (r[:, None] / sy) ** 2) * np.exp(-0.5 * (r[None, :] / sx) ** 2)
    return (p / p.sum())[None]


def benefit_case():
    """(psfs, object (64, 64), measurement (2, 64, 64) float64): view 0 is the object through a PSF that is narrow along y, view 1
    the object displaced by BENEFIT_DISPLACEMENT (analytically) through one that is narrow along x; noise-free."""
    from scipy.signal import fftconvolve
    p = blobs(7, 64, 64)
    psfs = [gaussian_psf(0.9, 2.2), gaussian_psf(2.2, 0.9)]
    obj = scene(p)
    moved = scene(p, BENEFIT_DISPLACEMENT)
    meas = np.stack([fftconvolve(obj, psfs[0][0], mode='same'), fftconvolve(moved, psfs[1][0], mode='same')])
    return psfs, obj, np.maximum(meas, 0.0) + 1e-9


def relative_error(estimate, obj, border=8):
    """RMS error of an estimate inside the border, relative to the object's RMS there."""
    e, o = estimate[border:-border, border:-border], obj[border:-border, border:-border]
    return float(np.sqrt(((e - o) ** 2).mean() / (o ** 2).mean()))
