"""Reference of the ensemble statistics (include/rlsted.h, rl_ensemble_stats): numpy long double, and the error bound the kernels
are held to.  TEST INFRASTRUCTURE ONLY.

The bound.  u = 2^-53, gamma_k = k u / (1 - k u).  A pixel has the members x_0 ... x_{n-1} (exact in float64: a float32 widens
without rounding) and the true value st = s t.  Hats are what the kernel computes (csrc/ensemble_kernels.hpp), in float64 without
contraction.

  mean   the sum is n - 1 additions in sequence (0 + x_0 is exact), then one division:
             |mean^ - mean| <= gamma_n A / n =: Em,            A = sum |x_m|
  ss     every term (x_m - mean^)^2 takes a subtraction and a product, the sum n - 1 more additions:
             |ss^ - sum (x_m - mean^)^2| <= gamma_(n+2) sum (x_m - mean^)^2
         and sum (x_m - mean^)^2 = ss + n (mean^ - mean)^2 EXACTLY (the cross term vanishes because sum (x_m - mean) = 0), so the
         mean's rounding error enters only to second order:
             |ss^ - ss| <= gamma_(n+2) (ss + n Em^2) + n Em^2 =: Ess
         (A one-pass sum x^2 - n mean^2 would instead carry gamma_n sum x^2: at x = 1e8 + N(0, 1) that is 1e1 against ss = 15.)
  var    one more division:  |var^ - var| <= (Ess + u (ss + Ess)) / (n - 1) =: Ev;   n = 1: var^ = 0 exactly.
  st     one rounding:  |st^ - st| <= u |st| =: tau
  b2     bias^ = fl(mean^ - st^):  |bias^ - bias| <= (Em + tau) (1 + u) + u |bias| =: Eb;  the product adds one rounding:
             |b2^ - b2| <= 2 |bias| Eb + Eb^2 + u (|bias| + Eb)^2 =: Eb2
  mse    the terms are (x_m - st + theta_m)^2 with |theta_m| <= tau, each through a subtraction and a product, n - 1 additions and
         one division -- gamma_(n+3) relative to their sum:
             |mse^ - mse| <= [gamma_(n+3) sum (|x_m - st| + tau)^2 + sum (2 |x_m - st| tau + tau^2)] / n =: Emse
  tt     (st^)^2: three roundings on st^2:  |tt^ - tt| <= gamma_3 st^2 =: Ett

  pixel sums   the thread sums, the workgroup tree and the partials are ONE summation order of the N per-pixel values v^_i (adding
         the zeros of idle threads is exact); any order of N terms obeys
             |sum^ - sum v_i| <= sum E_i + gamma_(N-1) sum (|v_i| + E_i)
         (the longest chain of the implementation is much shorter than N - 1; N - 1 needs no knowledge of the split).
"""
import numpy as np

FIELDS = 6
U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


class Reference:
    """Per-pixel reference values (long double) and bounds (float64) of one group: members [n][N] float64, truth [N] or None."""

    def __init__(self, members, truth=None, scale=1.0):
        x = np.asarray(members, dtype=np.float64)
        assert x.ndim == 2
        n, N = x.shape
        self.n, self.N = n, N
        xl = x.astype(LD)
        self.mean = xl.sum(axis=0) / LD(n)
        d = xl - self.mean
        self.ss = (d * d).sum(axis=0)
        self.var = self.ss / LD(n - 1) if n > 1 else np.zeros(N, dtype=LD)
        A = np.abs(x).sum(axis=0)
        ss = self.ss.astype(np.float64)
        self.e_mean = gamma(n) * A / n
        ne2 = n * self.e_mean ** 2
        self.e_ss = gamma(n + 2) * (ss + ne2) + ne2
        self.e_var = (self.e_ss + U * (ss + self.e_ss)) / (n - 1) if n > 1 else np.zeros(N)
        self.have_truth = truth is not None
        if self.have_truth:
            st = LD(scale) * np.asarray(truth, dtype=np.float64).ravel().astype(LD)
            bias = self.mean - st
            e = xl - st
            self.b2 = bias * bias
            self.mse = (e * e).sum(axis=0) / LD(n)
            self.tt = st * st
            tau = U * np.abs(st).astype(np.float64)
            ab = np.abs(bias).astype(np.float64)
            eb = (self.e_mean + tau) * (1 + U) + U * ab
            self.e_b2 = 2 * ab * eb + eb ** 2 + U * (ab + eb) ** 2
            ae = np.abs(e).astype(np.float64)
            self.e_mse = (gamma(n + 3) * ((ae + tau) ** 2).sum(axis=0) + (2 * ae * tau + tau ** 2).sum(axis=0)) / n
            self.e_tt = gamma(3) * self.tt.astype(np.float64)
        else:
            z = np.zeros(N, dtype=LD)
            self.b2 = self.mse = self.tt = z
            self.e_b2 = self.e_mse = self.e_tt = np.zeros(N)

    def sums(self):
        """(reference [6] long double, bound [6] float64) of the pixel sums; field 0 (n) is exact."""
        ref = np.zeros(FIELDS, dtype=LD)
        bnd = np.zeros(FIELDS)
        ref[0] = self.n
        g = gamma(max(self.N - 1, 0))
        for f, (v, e) in enumerate(((self.mean, self.e_mean), (self.var, self.e_var), (self.b2, self.e_b2), (self.mse, self.e_mse),
                                    (self.tt, self.e_tt)), start=1):
            ref[f] = v.sum()
            bnd[f] = e.sum() + g * (np.abs(v).astype(np.float64) + e).sum()
        return ref, bnd

    def check(self, out, mean=None, var=None, label=''):
        """Asserts the kernel's `out` [6] -- and its maps, where given -- within the bound; prints the worst error / bound."""
        ref, bnd = self.sums()
        err = np.abs(np.asarray(out, dtype=np.float64).astype(LD) - ref).astype(np.float64)
        assert out[0] == self.n, label
        worst = [float(np.max(err[1:] / np.where(bnd[1:] > 0, bnd[1:], 1.0)))]
        assert np.all(err <= bnd), '%s: sums off by %s, allowed %s' % (label, err, bnd)
        for got, want, e in ((mean, self.mean, self.e_mean), (var, self.var, self.e_var)):
            if got is None:
                continue
            pe = np.abs(np.asarray(got, dtype=np.float64).ravel().astype(LD) - want).astype(np.float64)
            assert np.all(pe <= e), '%s: a map off by %g at most, against its bound up to %g' % (label, pe.max(), e.max())
            worst.append(float(np.max(pe / np.where(e > 0, e, 1.0))))
        if not self.have_truth:
            assert np.all(np.asarray(out)[3:] == 0.0), label
        if self.n == 1:
            assert out[2] == 0.0 and (var is None or np.all(np.asarray(var) == 0.0)), label
        if self.have_truth:
            # mse = b2 + (n - 1) / n var, in the sums the kernel reports: each within its bound of an exact identity
            lhs = LD(out[4]) - (LD(out[3]) + LD(self.n - 1) / LD(self.n) * LD(out[2]))
            allow = bnd[4] + bnd[3] + (self.n - 1) / self.n * bnd[2]
            assert abs(float(lhs)) <= allow, '%s: mse - (b2 + (n-1)/n var) = %g, allowed %g' % (label, float(lhs), allow)
        print('%s: worst error / bound %s' % (label, ' '.join('%.3g' % w for w in worst)))


class Case:
    """One call's worth of data: groups of the given sizes, every image of N values in ONE buffer of `dtype` at element offsets
    that start at `shift` and advance by an odd stride, N or N + 1 (so the offsets take every residue modulo 4: 16-byte aligned
    images and misaligned ones, odd offsets among them); the first member of
    group 1 is the first image of group 0 (a member listed in two groups); a truth buffer of `truth_dtype` with one image per group
    at offsets of its own, and a scale per group."""

    def __init__(self, rng, dtype, N, sizes, shift=1, truth_dtype='f64', level=200.0, cancel=False):
        np_t = np.float32 if dtype == 'f32' else np.float64
        total = int(sum(sizes))
        stride = N + 1 - N % 2
        self.dtype, self.truth_dtype, self.N, self.sizes = dtype, truth_dtype, N, list(sizes)
        self.buf = np.zeros(shift + total * stride, dtype=np_t)
        obj = level * (0.2 + rng.random(N))
        self.offsets, k = [], 0
        for n in sizes:
            offs = []
            for _ in range(n):
                o = shift + k * stride
                vals = 1e8 + rng.standard_normal(N) if cancel else rng.poisson(obj) + rng.random(N)
                self.buf[o:o + N] = vals
                offs.append(o)
                k += 1
            self.offsets.append(offs)
        if len(sizes) > 1:
            self.offsets[1][0] = self.offsets[0][0]
        G = len(sizes)
        tt = np.float32 if truth_dtype == 'f32' else np.float64
        self.truth_buf = np.zeros(3 + G * stride, dtype=tt)
        self.truth_off = [3 + g * stride for g in range(G)]
        for o in self.truth_off:
            self.truth_buf[o:o + N] = (1e8 if cancel else 0.0) + obj * (0.9 + 0.2 * rng.random(N))
        self.scale = [1.0 if cancel else 0.75 + 0.25 * g for g in range(G)]

    def members(self, g):
        return np.stack([self.buf[o:o + self.N].astype(np.float64) for o in self.offsets[g]])

    def reference(self, g, truth=True):
        t = self.truth_buf[self.truth_off[g]:self.truth_off[g] + self.N].astype(np.float64) if truth else None
        return Reference(self.members(g), t, self.scale[g])
