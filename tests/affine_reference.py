"""Twin of the affine path (include/rlsted.h rl_warp_images, rl_affine_sums; rescan_line_sted_amd/registration.py): the warp in
numpy long double with the bound the float64 kernel is held to, the 45 sums in long double with theirs, the fixed-order statistics
bit for bit, analytic scenes whose true transform involves no interpolation, and the whole method on a numpy stand-in for the device
(the very host code of the product, registration._estimate_transforms, driven by scipy's affine_transform and numpy sums).
TEST INFRASTRUCTURE ONLY.

THE WARP'S BOUND.  u = 2^-53, gamma_k = k u / (1 - k u).  The twin takes the kernel's own coordinates (Y, X; two fused multiply-adds
each, reproduced exactly, `fma`) and the product's own taps (the float64 values of h[k] = sqrt(3) z^|k|, |k| <= 30), and does
everything else in long double.  Against it the kernel's float64 arithmetic errs by
  x pass   e1 = gamma_61 sum_k |h_k| |src|                      (a product, then 60 fused multiply-adds: 61 roundings)
  y pass   e2 = gamma_61 sum_k |h_k| (|c1| + e1) + sum_k |h_k| e1
  weights  every cubic weight is at most 6 roundings on terms of magnitude <= 4 and is >= 0 with sum 1: relative error <= gamma_16
           where it matters (w >= 1/6 of the row's mass) and absolute error <= 16 u otherwise; both are covered by
           gamma_16 (|w| + 1) per weight, so the 16 products wy_i wx_j carry (gamma_32 + ...) <= gamma_40 (|wy_i| + 1)(|wx_j| + 1)
  evaluation  4 + 4 roundings of the two fma chains: gamma_8
  total    |v^ - v| <= sum_ij wy_i wx_j e2_ij + gamma_48 sum_ij (|wy_i| + 1)(|wx_j| + 1) |c_ij|
Order 1: gamma_6 sum |w w s| (1 - t is one rounding, two products and two fused multiply-adds).  The truncated tail of the prefilter,
at most 8.8e-18 max|src| per axis (three times that after the second axis), is in the twin too -- it uses the same taps -- and enters
only the comparison with scipy (TAIL).  The destination's rounding (u |v| for float64, 2^-24 |v| for float32) is added by the tests.

THE SUMS' BOUND.  phi is formed in float64 exactly as the kernel forms it (numpy rounds each operation on its own); each of the 45
sums then takes its n exact products through ONE fused multiply-add each, whatever the order: |S^ - S| <= gamma_n sum |term|.
"""
from fractions import Fraction

import numpy as np
from scipy import ndimage

U = 2.0 ** -53
LD = np.longdouble
K = 30
TAIL = 4 * 8.8e-18
TILE = 32


def gamma(k):
    return k * U / (1.0 - k * U)


def fma(a, b, c):
    """round(a b + c) in float64, exactly, for arrays; b must be integers below 2^11 in magnitude (pixel indices): a b is then
    exact in the 64-bit significand of long double, the sum rounds once to 64 bits, and the rare results that sit on a float64 tie
    after that rounding are redone in rationals."""
    assert np.finfo(LD).nmant == 63, 'the twin needs the 80-bit long double'
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    assert np.all(np.abs(b) < 2048) and np.all(b == np.rint(b))
    s = a.astype(LD) * b.astype(LD) + c.astype(LD)
    r = s.astype(np.float64)
    tie = np.abs(s - r.astype(LD)) == (0.5 * np.spacing(np.abs(r))).astype(LD)
    r = r.copy()
    for i in zip(*np.nonzero(tie)):
        r[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def coords(xf, oy, ox):
    """(Y, X) of the output grid as the kernel forms them."""
    y, x = np.mgrid[0:oy, 0:ox].astype(np.float64)
    return fma(xf[0], y, fma(xf[1], x, xf[4])), fma(xf[2], y, fma(xf[3], x, xf[5]))


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def taps():
    """The product's taps as long double values of their float64 roundings, index k + 30."""
    r3 = np.sqrt(LD(3))
    z = r3 - LD(2)
    h = [r3]
    for _ in range(K):
        h.append(h[-1] * z)
    h = np.array(h[:0:-1] + h, dtype=LD)
    return h.astype(np.float64).astype(LD)


def _fir(v, axis, h):
    n = v.shape[axis]
    out = np.zeros(v.shape, dtype=LD)
    base = np.arange(n)
    for k in range(-K, K + 1):
        out += h[k + K] * np.take(v, mirror(base + k, n), axis=axis)
    return out


def coefficients(src):
    """(c long double, e float64): the spline coefficients by the two FIR passes and the bound of the kernel's error in them."""
    h = taps()
    s = np.asarray(src, dtype=np.float64).astype(LD)
    c1 = _fir(s, 1, h)
    e1 = gamma(61) * _fir(np.abs(s), 1, np.abs(h))
    c = _fir(c1, 0, h)
    e2 = gamma(61) * _fir(np.abs(c1) + e1, 0, np.abs(h)) + _fir(e1, 0, np.abs(h))
    return c, e2.astype(np.float64)


def cubic_weights(t):
    t = t.astype(LD)
    u = 1 - t
    return [u * u * u / 6, (t * t * (t - 2) * 3 + 4) / 6, (u * u * (u - 2) * 3 + 4) / 6, t * t * t / 6]


def warp(src, xf, output_shape, order=3, coef=None):
    """(value long double (oy, ox), bound float64) of one image: the spline at the kernel's coordinates, before the floor.  coef:
    coefficients(src), where a test has them already."""
    src = np.asarray(src)
    sy, sx = src.shape
    oy, ox = output_shape
    Y, X = coords(np.asarray(xf, dtype=np.float64), oy, ox)
    Fy, Fx = np.floor(Y), np.floor(X)
    ty, tx = Y - Fy, X - Fx
    iy, ix = Fy.astype(np.int64), Fx.astype(np.int64)
    value, bound = np.zeros((oy, ox), dtype=LD), np.zeros((oy, ox))
    if order == 3:
        c, e = coefficients(src) if coef is None else coef
        wy, wx = cubic_weights(ty), cubic_weights(tx)
        for i in range(4):
            yy = mirror(iy - 1 + i, sy)
            for j in range(4):
                xx = mirror(ix - 1 + j, sx)
                w = wy[i] * wx[j]
                value += w * c[yy, xx]
                bound += w.astype(np.float64) * e[yy, xx]
                bound += gamma(48) * ((np.abs(wy[i]) + 1) * (np.abs(wx[j]) + 1) * np.abs(c[yy, xx])).astype(np.float64)
    else:
        s = src.astype(np.float64).astype(LD)
        wy, wx = [1 - ty.astype(LD), ty.astype(LD)], [1 - tx.astype(LD), tx.astype(LD)]
        for i in range(2):
            yy = mirror(iy + i, sy)
            for j in range(2):
                xx = mirror(ix + j, sx)
                # a weight that is exactly 0 does not read its sample: its term is left out, whatever the sample holds
                term = np.where((wy[i] == 0) | (wx[j] == 0), LD(0), wy[i] * wx[j] * s[yy, xx])
                value += term
                bound += gamma(6) * np.abs(term).astype(np.float64)
    return value, bound


def scipy_warp(src, xf, output_shape, order=3):
    return ndimage.affine_transform(np.asarray(src, dtype=np.float64), np.array([[xf[0], xf[1]], [xf[2], xf[3]]]), offset=(xf[4], xf[5]),
                                    output_shape=tuple(output_shape), order=order, mode='mirror')


def stored_sum(dst):
    """The float64 sum of one stored image (oy, ox) in the kernel's fixed order, bit for bit: per tile of 32 x 32 thread t sums column
    t mod 32, rows t / 32 + 8 k in increasing order; the halving tree over the 256 threads; the tiles in row-major order."""
    oy, ox = dst.shape
    nby, nbx = -(-oy // TILE), -(-ox // TILE)
    pad = np.zeros((nby * TILE, nbx * TILE))
    pad[:oy, :ox] = dst.astype(np.float64)
    total = 0.0
    for by in range(nby):
        for bx in range(nbx):
            tile = pad[by * TILE:(by + 1) * TILE, bx * TILE:(bx + 1) * TILE].reshape(4, 8, TILE)     # [k][t / 32][t mod 32]
            s = np.zeros(256)
            for k in range(4):
                s = s + tile[k].ravel()
            h = 128
            while h:
                s = s[:h] + s[h:2 * h]
                h //= 2
            total = total + s[0]
    return total


def bin2(a):
    """The 2 x 2 mean as rl_warp_images order 1 forms it with diag(2, 2), offset (0.5, 0.5): ((a + b) + (c + d)) / 4."""
    ny, nx = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
    a = np.asarray(a, dtype=np.float64)[:ny, :nx]
    return ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2])) * 0.25


WARP_SHAPES = [((1, 1), (1, 1)), ((1, 17), (1, 17)), ((5, 7), (5, 7)), ((37, 53), (41, 29)), ((130, 70), (130, 70))]   # source -> output


def centred(L, t, shape):
    """xf of the matrix L about the centre of an image of `shape`, plus t."""
    L = np.asarray(L, dtype=np.float64)
    c = np.array([(shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0])
    o = c + np.asarray(t, dtype=np.float64) - L @ c
    return np.array([L[0, 0], L[0, 1], L[1, 0], L[1, 1], o[0], o[1]])


def warp_cases(shape):
    """name -> xf: the transforms every warp test runs on a source of `shape`."""
    rot = lambda d: rotation(d)[:, :2]
    return {'identity': centred(np.eye(2), (0, 0), shape), 'translation': centred(np.eye(2), (0.37, -0.81), shape),
            'rot0.7': centred(rot(0.7), (0, 0), shape), 'rot30': centred(rot(30.0), (0.25, -0.5), shape), 'rot90': centred(rot(90.0), (0, 0), shape),
            'scale1.03': centred(1.03 * np.eye(2), (0, 0), shape), 'shear': centred([[1.0, 0.08], [-0.03, 1.0]], (0.5, 0.25), shape),
            'far': centred(rot(0.7), (1e4, -1e4 + 0.3), shape), 'shrink3': np.array([3.0, 0.1, -0.1, 3.0, 0.25, 0.75])}


# ---- the sums --------------------------------------------------------------------------------------------------------------------------
def basis(w):
    """phi (8, ny - 2, nx - 2) over the pixels with four neighbours, in float64 as the kernel forms it."""
    w = np.asarray(w, dtype=np.float64)
    ny, nx = w.shape
    y, x = np.mgrid[1:ny - 1, 1:nx - 1].astype(np.float64)
    yc, xc = y - 0.5 * (ny - 1), x - 0.5 * (nx - 1)
    gy, gx = 0.5 * (w[2:, 1:-1] - w[:-2, 1:-1]), 0.5 * (w[1:-1, 2:] - w[1:-1, :-2])
    return np.stack([gy, gx, gy * yc, gy * xc, gx * yc, gx * xc, w[1:-1, 1:-1], np.ones_like(gy)])


def affine_sums(a, w, M, exact=True):
    """(S [45], bound [45]) of one pair; exact=True: long double sums and the bound, False: float64 sums (the whole method's twin)."""
    ny, nx = w.shape
    phi = basis(w)[:, M - 1:ny - M - 1, M - 1:nx - M - 1]
    av = np.asarray(a, dtype=np.float64)[M:ny - M, M:nx - M]
    T = LD if exact else np.float64
    phi, av = phi.astype(T), av.astype(T)
    S, B = np.zeros(45, dtype=T), np.zeros(45)
    f = 0
    for j in range(8):
        for k in range(j, 8):
            t = phi[j] * phi[k]
            S[f], B[f] = t.sum(), float(np.abs(t).sum())
            f += 1
    for j in range(8):
        t = phi[j] * av
        S[36 + j], B[36 + j] = t.sum(), float(np.abs(t).sum())
    S[44] = B[44] = (av * av).sum()
    return S, gamma(av.size) * B


# ---- the analytic scene ----------------------------------------------------------------------------------------------------------------
def blobs(seed, ny, nx, count=120):
    """Blob parameters: centres anywhere in the field of view, anisotropic widths, an orientation, an amplitude.  The field is
    filled on purpose: scale and shear are fixed by structure far from the centre, and the error is measured at the corners (two
    dozen blobs kept away from the border leave the affine model's corner error at 0.3 - 0.7 px on 96 x 128, rigid at 0.09 px)."""
    rng = np.random.default_rng(seed)
    return dict(cy=rng.uniform(0.0, ny, count), cx=rng.uniform(0.0, nx, count),
                sy=rng.uniform(1.2, 3.0, count), sx=rng.uniform(1.2, 3.0, count), th=rng.uniform(0, np.pi, count),
                amp=rng.uniform(50.0, 400.0, count), ny=ny, nx=nx)


def scene(p, T=None, blur=(0.0, 0.0)):
    """The blobs, noise-free and without background, as the image B with transform T relative to the untransformed scene A:
    B(c + L (x - c) + t) = A(x) -- every blob's centre and covariance transformed analytically, no interpolation -- and then each
    covariance widened by diag(blur)^2 in B's own frame (the view's PSF)."""
    ny, nx = p['ny'], p['nx']
    T = np.array([[1.0, 0, 0], [0, 1.0, 0]]) if T is None else np.asarray(T, dtype=np.float64)
    L, t = T[:, :2], T[:, 2]
    c0 = np.array([(ny - 1) / 2.0, (nx - 1) / 2.0])
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    out = np.zeros((ny, nx))
    for cy, cx, sy, sx, th, amp in zip(p['cy'], p['cx'], p['sy'], p['sx'], p['th'], p['amp']):
        c, s = np.cos(th), np.sin(th)
        cov = np.array([[c * c * sy * sy + s * s * sx * sx, c * s * (sy * sy - sx * sx)], [c * s * (sy * sy - sx * sx), s * s * sy * sy + c * c * sx * sx]])
        mu = c0 + L @ (np.array([cy, cx]) - c0) + t
        covB = L @ cov @ L.T
        wide = covB + np.diag([blur[0] ** 2, blur[1] ** 2])
        inv = np.linalg.inv(wide)
        dy, dx = y - mu[0], x - mu[1]
        out += amp * np.sqrt(np.linalg.det(covB) / np.linalg.det(wide)) * np.exp(-0.5 * (inv[0, 0] * dy * dy + 2 * inv[0, 1] * dy * dx + inv[1, 1] * dx * dx))
    return out


def rotation(degrees, scale=1.0, t=(0.0, 0.0)):
    a = np.deg2rad(degrees)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), t[0]], [scale * np.sin(a), scale * np.cos(a), t[1]]])


TRUTHS = {'rigid': rotation(3.0), 'similarity': rotation(-2.0, 1.02), 'affine': rotation(3.0, 0.98)}
SEEDS = (11, 12, 13)
BLURS = ((1.5, 2.5), (2.5, 1.5))


def view_pair(seed, ny, nx, T, noise=True, peak=200.0, background=5.0):
    """(A, B) float64: two views of one scene through anisotropic blurs, B transformed by T, scaled to `peak` photons over
    `background` and, with noise, Poisson distributed."""
    p = blobs(seed, ny, nx)
    a, b = scene(p, None, BLURS[0]), scene(p, T, BLURS[1])
    k = peak / a.max()
    a, b = a * k + background, b * k + background
    if noise:
        rng = np.random.default_rng(seed + 1000)
        a, b = rng.poisson(a).astype(np.float64), rng.poisson(b).astype(np.float64)
    return a, b


# ---- the whole method on a numpy stand-in ------------------------------------------------------------------------------------------
class Buf:
    def __init__(self, a, dtype):
        self.a, self.dtype = a, dtype


class NumpyDevice:
    """Stands in for registration._Device in _estimate_transforms: alloc, gather_warp (scipy's affine_transform; the 2 x 2 mean for
    the binning map) and affine_sums (float64 numpy), with a log of the calls."""

    def __init__(self):
        self.calls = []

    def alloc(self, elements, dtype):
        return Buf(np.full(int(elements), np.nan, dtype=np.float32 if dtype == 'f32' else np.float64), dtype)

    def warp(self, src, src_element, n, sy, sx, xf, order, floor, dst, dst_element, oy, ox):
        xf = np.asarray(xf, dtype=np.float64).reshape(n, 6)
        stats = np.zeros((n, 2))
        for k in range(n):
            img = src.a[src_element + k * sy * sx:src_element + (k + 1) * sy * sx].reshape(sy, sx).astype(np.float64)
            raw = bin2(img)[:oy, :ox] if order == 1 and tuple(xf[k]) == (2.0, 0.0, 0.0, 2.0, 0.5, 0.5) and (oy, ox) == (sy // 2, sx // 2) \
                else scipy_warp(img, xf[k], (oy, ox), order)
            out = raw if floor is None else np.maximum(raw, floor)
            stats[k] = [0 if floor is None else (raw < floor).sum(), out.sum()]
            dst.a[dst_element + k * oy * ox:dst_element + (k + 1) * oy * ox] = out.ravel()
        self.calls.append(('warp', n, (sy, sx), (oy, ox), order, floor, xf.copy()))
        return stats

    def gather_warp(self, src, offsets, sy, sx, xf, order, dst, oy, ox):
        for k, o in enumerate(offsets):
            self.warp(src, o, 1, sy, sx, xf[k:k + 1], order, None, dst, k * oy * ox, oy, ox)

    def affine_sums(self, ref, ref_offsets, w, w_offsets, ny, nx, M):
        out = np.stack([affine_sums(ref.a[ro:ro + ny * nx].reshape(ny, nx), w.a[wo:wo + ny * nx].reshape(ny, nx), M, exact=False)[0]
                        for ro, wo in zip(ref_offsets, w_offsets)])
        self.calls.append(('affine_sums', list(ref_offsets), list(w_offsets), (ny, nx), M))
        return out


def estimate(images, reference, model='rigid', passes=5, min_side=48, margin=4, init=None):
    """The twin of estimate_transforms: the product's own host code on the stand-in.  images (N, ny, nx), reference (ny, nx)."""
    from rescan_line_sted_amd import registration as reg
    images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    N, ny, nx = images.shape
    dev = NumpyDevice()
    dt = 'f32' if images.dtype == np.float32 else 'f64'
    mov, ref = Buf(np.ascontiguousarray(images).ravel().copy(), dt), Buf(np.ascontiguousarray(reference).ravel().copy(), dt)
    return reg._estimate_transforms(dev, ref, [0] * N, mov, [i * ny * nx for i in range(N)], ny, nx, model, passes, min_side, margin, init)
