"""numpy reference of total-variation regularised Richardson-Lucy (include/rlsted.h rl_deconv_set_tv; Dey et al., Microsc. Res.
Tech. 69, 260, 2006), per element type: every operation below is one IEEE operation of `dtype` in the order the header states
(numpy's sqrt and / are correctly rounded, and numpy never contracts a multiply and an add).

psi(x) is the oracle's own iteration (oracle.line_sted_oracle.Deconvolver.iterate) applied to x.  Frames are the slices of the
(nz, ny, nx) data; the mean s is per frame.  Test infrastructure only.
"""
import os

import numpy as np

from accel_reference import AcceleratedRL
from oracle import line_sted_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def tv_eps2(eps_rel, s, dtype):
    """eps2 = T((eps_rel s) (eps_rel s)): formed in float64, rounded once.  s: (frames,) float64."""
    e = np.float64(eps_rel) * np.asarray(s, dtype=np.float64)
    return (e * e).astype(dtype)


def tv_divergence(x, eps2):
    """div (grad x / sqrt(|grad x|^2 + eps2)) with forward differences (0 in the last column / row) and their backward adjoint
    (the subtracted term is 0 in column 0 / row 0).  x: (frames, ny, nx) of the element type; eps2: (frames,) of the same."""
    dt = x.dtype
    dx, dy = np.zeros_like(x), np.zeros_like(x)
    dx[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    dy[:, :-1, :] = x[:, 1:, :] - x[:, :-1, :]
    m = np.sqrt((dx * dx + dy * dy) + eps2.astype(dt)[:, None, None])
    px, py = dx / m, dy / m
    pxw, pyn = np.zeros_like(x), np.zeros_like(x)
    pxw[:, :, 1:] = px[:, :, :-1]
    pyn[:, 1:, :] = py[:, :-1, :]
    div = (px - pxw) + (py - pyn)
    assert div.dtype == dt
    return div


def tv_weight(x, lam, eps_rel, s=None):
    """w = 1 / (1 - lambda div) of the frames x, in x's element type.  s: the frames' means (float64); None: the plain float64
    mean (a test of the kernels passes the ordered sums instead)."""
    x = np.asarray(x)
    dt = x.dtype.type
    if s is None:
        s = x.astype(np.float64).mean(axis=(1, 2))
    div = tv_divergence(x, tv_eps2(eps_rel, s, dt))
    den = dt(1) - dt(lam) * div
    w = dt(1) / den
    assert w.dtype == x.dtype
    return w, den


def tv_seminorm(x):
    """sum |grad x| of forward differences over the pixels that have both (all but the last row and column), float64."""
    x = np.asarray(x, dtype=np.float64)
    dx = x[..., :-1, 1:] - x[..., :-1, :-1]
    dy = x[..., 1:, :-1] - x[..., :-1, :-1]
    return float(np.sum(np.sqrt(dx * dx + dy * dy)))


class RegularisedRL:
    """x_new = psi(x) * w(x), float64; lambda = 0 is the oracle's iteration itself (no weight is formed)."""

    def __init__(self, psfs, noisy, lam=0.01, eps_rel=0.1):
        self.d = orc.Deconvolver([np.asarray(p, dtype=np.float64) for p in psfs])
        self.lam, self.eps_rel = lam, eps_rel
        self.set_measurement(noisy)

    def set_measurement(self, noisy):
        self.d.noisy_measurement = [np.asarray(m, dtype=np.float64) for m in noisy]
        self.d.num_iterations = 1                  # (the oracle's iterate() would otherwise restart from ones itself)
        self.estimate = np.ones(self.d.noisy_measurement[0].shape)

    def set_estimate(self, x):
        self.estimate = np.array(x, dtype=np.float64, copy=True)

    def step(self, x):
        self.d.estimate = np.array(x, dtype=np.float64, copy=True)
        self.d.iterate()
        if self.lam == 0:
            return self.d.estimate
        w, _ = tv_weight(np.asarray(x, dtype=np.float64), self.lam, self.eps_rel)
        return self.d.estimate * w

    def iterate(self, k=1):
        for _ in range(k):
            self.estimate = self.step(self.estimate)
        return self.estimate


class AcceleratedRegularisedRL(AcceleratedRL):
    """Biggs-Andrews extrapolation (accel_reference.AcceleratedRL) whose psi is the regularised step: the weight is formed at the
    extrapolated point y_k."""

    def __init__(self, psfs, noisy, lam=0.01, eps_rel=0.1):
        self.lam, self.eps_rel = lam, eps_rel
        super().__init__(psfs, noisy)

    def psi(self, y):
        y = np.array(y, dtype=np.float64, copy=True)
        out = super().psi(y)
        if self.lam == 0:
            return out
        w, _ = tv_weight(y, self.lam, self.eps_rel)
        return out * w


def ordered_sums(x, nb, threads):
    """The sum of every workgroup of every frame in the order accel_kernels.hpp states: per thread over its vectors in
    increasing order (the W elements of a vector in order), then the workgroup tree.  x: (frames, n) -> (frames, nb) float64."""
    frames, n = x.shape
    W = 16 // x.itemsize
    nvec = -(-n // W)
    vpb = -(-nvec // nb)
    part = np.zeros((frames, nb))
    a = x.astype(np.float64)
    for f in range(frames):
        for b in range(nb):
            ss = np.zeros(threads)
            j0, j1 = b * vpb, min((b + 1) * vpb, nvec)
            for s in range(j0, j1, threads):                 # one round of vectors: thread t takes vector s + t
                m = min(threads, j1 - s)
                for c in range(W):
                    e = (np.arange(s, s + m) * W + c)
                    ok = e < n
                    ss[:m][ok] = ss[:m][ok] + a[f, e[ok]]
            h = threads // 2
            while h > 0:
                ss[:h] = ss[:h] + ss[h:2 * h]
                h //= 2
            part[f, b] = ss[0]
    return part


def frame_means(part, n):
    s = np.zeros(part.shape[0])
    for b in range(part.shape[1]):
        s = s + part[:, b]
    return s / np.float64(n)


def low_dose_case(brightness):
    psfs = list(np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))['2p0x_lr/line_sted_psfs'])
    obj = np.load(os.path.join(GOLDEN, 'objects.npz'))['astronaut'].astype(np.float64)
    truth = obj * (brightness / obj.sum())
    rng = np.random.default_rng(3)
    noisy = [rng.poisson(m) + 1e-9 for m in orc.Deconvolver(psfs).H(truth)]
    return psfs, truth, noisy


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def sum_blocks(n, itemsize):
    """accel_blocks of csrc/accel_kernels.hpp: workgroups per frame of n pixels."""
    nvec = -(-n // (16 // itemsize))
    return min(max(-(-nvec // (256 * 8)), 1), 256)


def device_means(x):
    """The frames' means as the kernels form them (ordered float64 sums).  x: (frames, ny, nx) of the element type."""
    n = x.shape[1] * x.shape[2]
    return frame_means(ordered_sums(x.reshape(x.shape[0], n), sum_blocks(n, x.itemsize), 256), n)
