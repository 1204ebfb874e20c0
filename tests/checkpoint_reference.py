"""Reference of the checkpoint trace (include/rlsted.h, rl_batch_submit_checkpoints): numpy long double, and the error bound the
kernels are held to.  TEST INFRASTRUCTURE ONLY.

The six sums over a frame's n pixels, x the estimate and T the scaled object (exact in float64: a float32 widens without rounding):
    0 sum x    1 sum T    2 sum x*x    3 sum T*T    4 sum x*T    5 sum (x-T)*(x-T)

The bound.  u = 2^-53, gamma_k = k u / (1 - k u).  A field is sum_i v_i; the kernel (csrc/checkpoint_kernels.hpp) forms every term in
float64 without contraction and adds the terms in ONE fixed order, the split of csrc/accel_kernels.hpp:

  term       r roundings: x and T none; x*x, T*T and x*T one product; (x-T)^2 a subtraction, whose error enters the square twice,
             and a product: three.  v^_i = v_i (1 + theta_r), |theta_r| <= gamma_r.
  thread     a thread owns at most vpt = ceil(vpb / 256) vectors of W = 16 / esize pixels (vpb = ceil(nvec / nb) vectors per
             workgroup, nvec = ceil(n / W), nb = accel_blocks): a pixel's term goes through at most vpt * W additions there
  workgroup  the binary tree over 256 slots: log2(256) = 8 additions
  frame      the nb partials in sequence: at most nb additions
  so a term passes through at most L = vpt * W + 8 + nb additions (adding the zeros of idle threads and 0 + first is exact and
  only shortens a chain), each a factor (1 + delta), |delta| <= u:

      |sum^ - sum v_i| <= gamma_(L + r) sum |v_i|

Chain length times unit roundoff times the sum of the terms' magnitudes; no constant is fitted.
"""
import numpy as np

FIELDS = 6
U = 2.0 ** -53
LD = np.longdouble
THREADS, VECS_PER_THREAD, MAX_BLOCKS = 256, 8, 256      # csrc/accel_kernels.hpp
ROUNDINGS = (0, 0, 1, 1, 1, 3)


def gamma(k):
    return k * U / (1.0 - k * U)


def blocks(n, esize):
    W = 16 // esize
    nvec = (n + W - 1) // W
    per = THREADS * VECS_PER_THREAD
    return min(max((nvec + per - 1) // per, 1), MAX_BLOCKS)


def chain_length(n, esize):
    """The longest chain of additions a term of an n-pixel frame of `esize`-byte elements passes through."""
    W = 16 // esize
    nvec = (n + W - 1) // W
    nb = blocks(n, esize)
    vpb = (nvec + nb - 1) // nb
    vpt = (vpb + THREADS - 1) // THREADS
    return vpt * W + 8 + nb


def terms(x, t):
    """The per-pixel terms of the six fields, long double [6][n], from float64 x and t."""
    x = np.asarray(x, dtype=np.float64).ravel().astype(LD)
    t = np.asarray(t, dtype=np.float64).ravel().astype(LD)
    d = x - t
    return np.stack([x, t, x * x, t * t, x * t, d * d])


def sums(x, t):
    return terms(x, t).sum(axis=1)


def bounds(x, t, esize):
    """[6] float64: gamma_(L + r) sum |v_i| per field, for a frame held in `esize`-byte elements."""
    v = terms(x, t)
    L = chain_length(v.shape[1], esize)
    mag = np.abs(v).sum(axis=1).astype(np.float64)
    return np.array([gamma(L + r) for r in ROUNDINGS]) * mag


def check(out, x, t, esize, label=''):
    """Asserts the trace `out` [6] of estimate x against object t within the bound; prints and returns the worst error / bound."""
    ref, bnd = sums(x, t), bounds(x, t, esize)
    err = np.abs(np.asarray(out, dtype=np.float64).astype(LD) - ref).astype(np.float64)
    ratio = err / np.where(bnd > 0, bnd, 1.0)
    print('%s: error / bound per field %s' % (label, ' '.join('%.3g' % r for r in ratio)))
    assert np.all(err <= bnd), '%s: sums off by %s, allowed %s' % (label, err, bnd)
    return float(ratio.max())
