"""One numpy model of a plan (include/rlsted.h rl_deconv_*), float64: the state rules between the oracle's iteration
(oracle.line_sted_oracle.Deconvolver), Biggs-Andrews acceleration (accel_reference), RL-TV (tv_reference) and the stopping rule
(stop_reference).  No arithmetic of its own: with no mode a step is the oracle's iterate(), with a mode it is the step of the
reference class; what is new is which of them runs, from which point and with which history.  Test infrastructure only.

    est is None          the plan holds no estimate: the next iterate starts from ones (new data, reset_estimate)
    fresh                the acceleration has no history: the next accelerated step has a = 0 (new data, a set estimate,
                         a change of mode, iterate_until's latched estimates)
"""
import numpy as np

import stop_reference as sr
from oracle import line_sted_oracle as orc
from tv_reference import AcceleratedRegularisedRL, RegularisedRL

BA = 'biggs-andrews'


class WatchedDeconvolver(orc.Deconvolver):
    """The oracle's Deconvolver; H also keeps the smallest min / max of a prediction it returned (per frame and view) and whether
    every one was finite -- what the admission of a case looks at (plan_cases.admit).  The values are the oracle's own."""

    def __init__(self, psfs):
        super().__init__(psfs)
        self.min_ratio = np.inf
        self.finite = True

    def H(self, x):
        out = super().H(x)
        for y in out:
            if not np.all(np.isfinite(y)):
                self.finite = False
                continue
            for f in range(y.shape[0]):
                top = float(y[f].max())
                self.min_ratio = min(self.min_ratio, float(y[f].min()) / top if top > 0 else 0.0)
        return out


class PlanModel:
    """The calls of rescan_line_sted_amd._lib.DeconvPlan with the same meaning, on (B, ny, nx) estimates and (B, V, ny, nx)
    measurements."""

    def __init__(self, psfs, B, ny, nx, acceleration=None, tv_lambda=None, tv_epsilon=0.1):
        self.psfs = [np.asarray(p, dtype=np.float64) for p in psfs]
        self.B, self.V, self.ny, self.nx = int(B), len(self.psfs), int(ny), int(nx)
        ones = [np.ones((self.B, self.ny, self.nx)) for _ in self.psfs]
        self.d = WatchedDeconvolver(self.psfs)            # one Deconvolver for every step: the references' psi goes through it
        self.rl = RegularisedRL(self.psfs, ones, lam=0.0)
        self.ba = AcceleratedRegularisedRL(self.psfs, ones, lam=0.0)
        self.rl.d = self.ba.d = self.d
        self.meas = None
        self.est = None
        self.fresh = True
        self.accel = False
        self.set_acceleration(acceleration)
        self.set_tv(tv_lambda, tv_epsilon)

    # ---- data and state
    def set_measurement(self, noisy):
        noisy = np.asarray(noisy, dtype=np.float64).reshape(self.B, self.V, self.ny, self.nx)
        self.meas = [np.ascontiguousarray(noisy[:, v]) for v in range(self.V)]
        self.d.noisy_measurement = self.meas
        self.d.num_iterations = 1                          # (the oracle's iterate() never restarts by itself: the model does)
        self.est = None
        self.fresh = True

    def measurement_written(self, noisy):
        """The measurement buffer was written on the device with these values: set_measurement without the upload."""
        self.set_measurement(noisy)

    def set_estimate(self, x):
        self.est = np.array(x, dtype=np.float64, copy=True).reshape(self.B, self.ny, self.nx)
        self.fresh = True

    def reset_estimate(self):
        self.est = None

    def set_acceleration(self, acceleration):
        on = acceleration == BA
        if acceleration not in (None, BA):
            raise ValueError(acceleration)
        if on != self.accel:
            self.fresh = True                              # a change of mode restarts the history; the estimate stays
        self.accel = on

    def set_tv(self, tv_lambda, tv_epsilon=0.1):
        lam = 0.0 if tv_lambda is None else float(tv_lambda)
        for r in (self.rl, self.ba):
            r.lam, r.eps_rel = lam, float(tv_epsilon)      # from the next iterate on

    def estimate(self):
        return self.est.copy()

    def alpha(self):
        """The a of every frame's last extrapolated point; 0 before one (no history: a set estimate, a change of mode,
        iterate_until's kept estimates) and on a plan that never was accelerated."""
        if self.fresh:
            return np.zeros(self.B)
        return np.array(self.ba.alpha, dtype=np.float64, copy=True)

    # ---- iterations
    def iterate(self, k=1):
        assert self.meas is not None
        if self.est is None:
            self.est = np.ones((self.B, self.ny, self.nx))
            self.fresh = True
        if self.accel:
            if self.fresh:
                self.ba.set_estimate(self.est)             # a point with no history
            if k > 0:
                self.fresh = False
            self.est = self.ba.iterate(k)
        else:
            if self.fresh:
                self.ba._reset()                           # (alpha() reads 0 after new data / a set estimate on the device too)
            self.rl.estimate = self.est
            self.est = self.rl.iterate(k)
        return self.est

    def iterate_until(self, max_iterations, rule=sr.DISCREPANCY, threshold=1.0, check_every=1):
        """iterate(check_every), D, the rule per frame, until every frame has stopped or max_iterations are done: a frame keeps the
        estimate, the count and the D of the check at which it stopped (or of the last check).  The kept estimates become the
        plan's estimate as a set estimate does.  Also returns every check's D ('trace': (checks, B)) for the margins and every
        check's estimates ('estimates': {iterations done: (B, ny, nx)})."""
        B, N = self.B, self.V * self.ny * self.nx
        its, div, stopped = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros(B, dtype=bool)
        kept = np.zeros((B, self.ny, self.nx))
        prev, done, trace, estimates = None, 0, [], {}
        while done < max_iterations and not stopped.all():
            c = min(check_every, max_iterations - done)
            self.iterate(c)
            done += c
            D = self.divergence()
            trace.append(D)
            estimates[done] = self.est.copy()
            for f in range(B):
                if stopped[f]:
                    continue
                kept[f], its[f], div[f] = self.est[f], done, D[f]
                stopped[f] = sr.rule_met(rule, threshold, N, D[f], None if prev is None else prev[f])
            prev = D
        self.set_estimate(kept)
        return {'iterations': its, 'divergence': div, 'stopped': stopped, 'trace': np.array(trace), 'estimates': estimates}

    # ---- operators: the estimate and the history stay
    def forward(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(self.B, self.ny, self.nx)
        return np.stack(self.d.H(x), axis=1)

    def adjoint(self, y, normalize=True):
        y = np.asarray(y, dtype=np.float64).reshape(self.B, self.V, self.ny, self.nx)
        return self.d.H_t([np.ascontiguousarray(y[:, v]) for v in range(self.V)], normalize=normalize)

    def prediction(self):
        """H(estimate): (B, V, ny, nx)."""
        return self.forward(self.est)

    def divergence(self):
        """(B,) D(measurement || H(estimate)) by stop_reference.divergence on the model's own prediction."""
        pred = self.prediction()
        return np.array([sr.divergence(np.stack([m[f] for m in self.meas]), pred[f]) for f in range(self.B)])
