"""Twin of the camera calibration (include/rlsted.h rl_calib_*, rl_repair_pixels; rescan_line_sted_amd/csrc/calib_kernels.hpp), written
for reading: the integer sums with Python integers, mean and variance as the correctly rounded float64 of the exact rationals
(fractions.Fraction: int / int division of Python rounds correctly), the float32 path as the sequential float64 loop, the repair
rule in plain numpy, and the synthetic camera of the calibration tests.  Nothing here is shared with the product code."""
from fractions import Fraction

import numpy as np

RAW = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2, np.dtype(np.float32): 3}
MAX_FRAMES = 65535


def window(frames, roi):
    y0, x0, ny, nx = roi
    return frames[:, y0:y0 + ny, x0:x0 + nx]


def sums_int(frames, roi):
    """(S, Q) of the window of integer frames (F, sy, sx): object arrays of Python integers."""
    w = window(frames, roi).astype(object)
    S = np.zeros(w.shape[1:], dtype=object)
    Q = np.zeros(w.shape[1:], dtype=object)
    for f in range(w.shape[0]):
        S = S + w[f]
        Q = Q + w[f] * w[f]
    return S, Q


def as_int64(S):
    return np.array([[int(v) for v in row] for row in S], dtype=np.int64)


def as_uint64(Q):
    return np.array([[int(v) for v in row] for row in Q], dtype=np.uint64)


def _round(fr):
    return fr.numerator / fr.denominator          # (Python's int / int: correctly rounded)


def stats_int(S, Q, F):
    """mean = S / F and var = (F Q - S^2) / (F (F - 1)) (0 for F = 1): the exact rationals, each rounded once to float64."""
    mean, var = np.zeros(S.shape), np.zeros(S.shape)
    for i in np.ndindex(S.shape):
        s, q = int(S[i]), int(Q[i])
        mean[i] = _round(Fraction(s, F))
        n = F * q - s * s
        assert 0 <= n < 2 ** 64
        var[i] = _round(Fraction(n, F * (F - 1))) if F > 1 else 0.0
    return mean, var


def sums_int_large(frames, roi):
    """sums_int for windows too large for Python integers to stay quick: numpy int64 / uint64, exact too (F 65535^2 < 2^63) --
    returned as object arrays like sums_int's."""
    w = window(frames, roi).astype(np.int64)
    return w.sum(axis=0).astype(object), (w * w).sum(axis=0).astype(object)


def stats_int_large(S, Q, F):
    """stats_int where N = F Q - S^2 < 2^53: numerators and denominators are then exact float64 values and numpy's one division
    rounds the exact rational correctly -- the same values as stats_int, without a Fraction per pixel."""
    S, Q = S.astype(np.int64), Q.astype(np.int64)
    N = F * Q - S * S
    assert N.min() >= 0 and N.max() < 2 ** 53 and np.abs(S).max() < 2 ** 53
    return S.astype(np.float64) / float(F), (N.astype(np.float64) / float(F * (F - 1)) if F > 1 else np.zeros(S.shape))


def sums_f32(frames, roi, S=None, Q=None):
    """The float32 path: S = S + (double)x, Q = Q + (double)x * (double)x frame after frame (each operation of numpy float64 arrays
    rounds once: no contraction)."""
    w = window(frames, roi).astype(np.float64)
    S = np.zeros(w.shape[1:]) if S is None else S.copy()
    Q = np.zeros(w.shape[1:]) if Q is None else Q.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        for f in range(w.shape[0]):
            S = S + w[f]
            Q = Q + w[f] * w[f]
    return S, Q


def stats_f32(S, Q, F):
    with np.errstate(invalid='ignore', over='ignore'):
        mean = S / float(F)
        num = Q - S * mean
        var = num / (float(F) - 1.0) if F > 1 else np.zeros(S.shape)
    return mean, var, num


def ulps(a, b):
    """The distance of two finite float64 arrays in units in the last place."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.int64(-2 ** 63) - ia[ia < 0]
    ib[ib < 0] = np.int64(-2 ** 63) - ib[ib < 0]
    return np.abs(ia - ib)


def repair(images, mask, radius):
    """The repair rule on (n, ny, nx) images of float32 / float64: (repaired copy, defects without a good pixel within radius)."""
    out = images.copy()
    mask = np.asarray(mask) != 0
    n, ny, nx = images.shape
    left = 0
    for y, x in zip(*np.nonzero(mask)):
        found = False
        for r in range(1, radius + 1):
            ya, yb, xa, xb = max(y - r, 0), min(y + r, ny - 1) + 1, max(x - r, 0), min(x + r, nx - 1) + 1
            good = ~mask[ya:yb, xa:xb]
            if good.any():
                for i in range(n):
                    v = np.sort(images[i, ya:yb, xa:xb][good], kind='stable')          # (row-major candidates, ascending, nan last)
                    c = v.size
                    if c % 2:
                        out[i, y, x] = v[(c - 1) // 2]
                    else:
                        out[i, y, x] = images.dtype.type((np.float64(v[c // 2 - 1]) + np.float64(v[c // 2])) * 0.5)
                found = True
                break
        left += 0 if found else 1
    return out, left


class Camera:
    """The synthetic camera of the calibration tests: gain 0.46 photons per count, a dark level of 100 +- 3 counts (fixed pattern),
    read noise 2 counts, a vignetted static scene, three hot pixels (+500 counts) and two dead ones."""
    GAIN, DARK, DARK_SPREAD, READ = 0.46, 100.0, 3.0, 2.0
    LEVELS = (40.0, 150.0, 400.0, 900.0)        # photons per pixel at the centre

    def __init__(self, seed, shape=(48, 64), frames=96):
        self.rng = np.random.default_rng(seed)
        self.shape, self.frames = shape, frames
        ny, nx = shape
        self.dark = self.DARK + self.DARK_SPREAD * self.rng.standard_normal(shape)
        yy, xx = np.mgrid[0:ny, 0:nx]
        r2 = ((yy - (ny - 1) / 2) / ny) ** 2 + ((xx - (nx - 1) / 2) / nx) ** 2
        self.scene = 1.0 - 0.8 * r2                                   # 1 at the centre, 0.6 in the corners
        self.hot = [(5, 7), (20, 41), (44, 60)]
        self.dead = [(11, 30), (33, 3)]
        self.planted = np.zeros(shape, dtype=bool)
        for p in self.hot + self.dead:
            self.planted[p] = True

    def stack(self, photons):
        """frames x ny x nx uint16 at `photons` per pixel at the centre (0: a dark stack)."""
        lam = np.broadcast_to(photons * self.scene, (self.frames,) + self.shape).copy()
        for p in self.dead:
            lam[(slice(None),) + p] = 0.0
        counts = self.rng.poisson(lam) / self.GAIN + self.dark + self.READ * self.rng.standard_normal(lam.shape)
        for p in self.hot:
            counts[(slice(None),) + p] += 500.0
        return np.clip(np.rint(counts), 0, 65535).astype(np.uint16)

    def stacks(self):
        return self.stack(0.0), [self.stack(p) for p in self.LEVELS]


def repair_cases(ny, nx):
    """The masks of the repair tests at a shape of at least 16 x 16: {name: (mask, radius, unrepaired)}."""
    def m(*cells):
        a = np.zeros((ny, nx), dtype=bool)
        for c in cells:
            a[c] = True
        return a
    cy, cx = ny // 2, nx // 2
    block = m((slice(cy - 3, cy + 4), slice(cx - 3, cx + 4)))
    everything = m((slice(2, 4), slice(2, 4)), (0, 0), (ny - 1, nx - 1), (ny - 4, slice(None)), (0, cx), (0, cx + 1), (cy, 1))
    everything |= block
    return {'isolated': (m((cy, cx)), 1, 0), 'corners': (m((0, 0), (ny - 1, nx - 1), (0, nx - 1)), 2, 0),
            'cluster': (m((slice(2, 4), slice(2, 4))), 3, 0), 'row': (m((5, slice(None))), 1, 0),
            'even': (m((0, cx), (0, cx + 1)), 1, 0),                 # an edge pair: 6 - 2 = 4 candidates each
            'block7': (block, 3, 1),                                 # the centre has no good pixel within 3: it stays
            'block7_r2': (block, 2, 9), 'none': (m(), 3, 0), 'all': (everything, 3, 1)}


class NumpyDevice:
    """Stands in for calibration._Device: exact integer sums in numpy, the twin's correctly rounded maps, the twin's repair."""
    log = None

    def __init__(self, device):
        type(self).log = self.calls = []

    def open(self, code, sensor, window):
        self.code, self.sensor, self.window, self.F = code, sensor, window, 0
        self.S = self.Q = None
        self.calls.append(('open', code, tuple(sensor), tuple(window)))

    def accumulate(self, frames):
        assert frames.flags.c_contiguous and RAW[frames.dtype] == self.code and frames.shape[1:] == tuple(self.sensor)
        y0, x0, ny, nx = self.window
        if self.code == 3:
            self.S, self.Q = sums_f32(frames, self.window, self.S, self.Q)
        else:
            w = frames[:, y0:y0 + ny, x0:x0 + nx].astype(np.int64)
            S, Q = w.sum(axis=0), (w * w).sum(axis=0)
            self.S, self.Q = (S, Q) if self.S is None else (self.S + S, self.Q + Q)
        self.F += frames.shape[0]
        self.calls.append(('accumulate', frames.shape[0]))
        return 1.0, 0.5

    def finalize(self):
        if self.code == 3:
            return stats_f32(self.S, self.Q, self.F)[:2]
        return stats_int(self.S.astype(object), self.Q.astype(object), self.F)

    def repair(self, images, mask, radius):
        out, left = repair(images, mask, radius)
        images[...] = out
        return np.full(images.shape[0], left, dtype=np.int64)

    def close(self):
        self.calls.append(('close',))


def benefit_stack(seed=5, shape=(64, 80), frames=2, hot=10):
    """The stack of the benefit test: a test object of rings and lines at about 100 photons per pixel, blurred by a 9 x 9 Gaussian
    PSF, Poisson noise, a camera of gain 1 over a dark level of 100; `hot` pixels planted at 20 times the frames' maximum.
    Returns (object, psfs, clean uint16 (F, ny, nx), with hot pixels, mask)."""
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(seed)
    ny, nx = shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    rad = np.hypot(yy - ny / 2, xx - nx / 2)
    obj = 0.3 + (np.cos(rad * 0.55) > 0.6) + 1.5 * ((xx + 2 * yy) % 17 < 2)
    obj *= 100.0 / obj.mean()
    g = np.exp(-np.arange(-4, 5) ** 2 / (2 * 1.6 ** 2))
    psf = np.outer(g, g)
    psf /= psf.sum()
    blurred = np.clip(fftconvolve(obj, psf, mode='same'), 0, None)
    clean = (100 + rng.poisson(np.broadcast_to(blurred, (frames,) + shape))).astype(np.uint16)
    mask = np.zeros(shape, dtype=bool)
    cells = rng.choice(ny * nx, size=hot, replace=False)
    mask.flat[cells] = True
    dirty = clean.copy()
    dirty[:, mask] = 20 * int(clean.max())
    return obj, [psf[None]], clean, dirty, mask
