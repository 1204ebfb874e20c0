"""numpy reference of Biggs-Andrews accelerated Richardson-Lucy (include/rlsted.h rl_deconv_set_acceleration), float64.

psi(y) is the oracle's own iteration (oracle.line_sted_oracle.Deconvolver.iterate) applied to y: the estimate is set to y and
iterate() is called.  Frames are the slices of the (nz, ny, nx) data; every sum is per frame, over its ny x nx pixels.
Test infrastructure only.
"""
import numpy as np

from oracle import line_sted_oracle as orc


def clamp_alpha(num, den):
    """a = clamp(num / den, 0, 1); 0 where den is 0 or not finite (or the quotient is nan)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    ok = (den > 0) & np.isfinite(den)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(ok, num / np.where(ok, den, 1.0), 0.0)
    return np.where(r > 1.0, 1.0, np.where(r > 0.0, r, 0.0))


def extrapolate(x, x_prev, a):
    """y = max(x + a (x - x_prev), 0) per frame; frames with a == 0 do not read x_prev."""
    y = np.array(x, dtype=np.float64, copy=True)
    for f in range(y.shape[0]):
        if a[f] != 0.0:
            y[f] = x[f] + a[f] * (x[f] - x_prev[f])
    return np.where(y > 0, y, 0.0)


class AcceleratedRL:
    """x_{k+1} = psi(y_k), g_k = x_{k+1} - y_k, a_{k+1} = clamp(<g_k, g_{k-1}> / <g_{k-1}, g_{k-1}>, 0, 1),
    y_{k+1} = max(x_{k+1} + a_{k+1} (x_{k+1} - x_k), 0); y_0 = x_0 = ones.  `estimate` is x_k.
    force_alpha_zero: every a = 0 (then this is plain Richardson-Lucy)."""

    def __init__(self, psfs, noisy, force_alpha_zero=False):
        self.d = orc.Deconvolver([np.asarray(p, dtype=np.float64) for p in psfs])
        self.force_alpha_zero = force_alpha_zero
        self.set_measurement(noisy)

    def set_measurement(self, noisy):
        """New data: the next iteration starts from ones with no history."""
        self.d.noisy_measurement = [np.asarray(m, dtype=np.float64) for m in noisy]
        self.d.num_iterations = 1                  # (the oracle's iterate() would otherwise restart from ones itself)
        self.estimate = np.ones(self.d.noisy_measurement[0].shape)
        self._reset()

    def set_estimate(self, x):
        """A point with no history: the next step has a = 0."""
        self.estimate = np.array(x, dtype=np.float64, copy=True)
        self._reset()

    def _reset(self):
        self.x_prev = self.g_prev = None
        self.next_alpha = np.zeros(self.estimate.shape[0])
        self.alpha = np.zeros(self.estimate.shape[0])    # the a of the last extrapolated point
        self.steps = 0

    def psi(self, y):
        self.d.estimate = np.array(y, dtype=np.float64, copy=True)
        self.d.iterate()
        return self.d.estimate

    def iterate(self, k=1):
        for _ in range(k):
            x = self.estimate
            a = np.zeros(x.shape[0]) if self.steps == 0 else self.next_alpha
            y = extrapolate(x, self.x_prev, a)
            self.alpha = a
            x_new = self.psi(y)
            g = x_new - y
            if self.g_prev is None or self.force_alpha_zero:
                self.next_alpha = np.zeros(x.shape[0])
            else:
                num = np.array([np.sum(g[f] * self.g_prev[f]) for f in range(x.shape[0])])
                den = np.array([np.sum(self.g_prev[f] * self.g_prev[f]) for f in range(x.shape[0])])
                self.next_alpha = clamp_alpha(num, den)
            self.x_prev, self.g_prev, self.estimate = x, g, x_new
            self.steps += 1
        return self.estimate


def i_divergence(measurement, prediction):
    """Poisson I-divergence sum m log(m / Hx) - m + Hx over all pixels and views."""
    total = 0.0
    for m, p in zip(measurement, prediction):
        m = np.asarray(m, dtype=np.float64)
        p = np.asarray(p, dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(m > 0, m * np.log(m / p), 0.0) - m + p
        total += float(np.sum(t))
    return total
