"""numpy reference of the Poisson I-divergence and the stopping rules (include/rlsted.h rl_deconv_divergence,
rl_deconv_iterate_until), float64: the pixel term, the two rules, and plain Richardson-Lucy by the oracle
(oracle.line_sted_oracle.Deconvolver) with D looked at every `check_every` iterations.  Test infrastructure only.

The study cases (TABLE) -- one 128 x 128 frame each, all float64, nothing from a device:
    obj  = objects.npz[name][0][None] scaled to photons / obj.sum()
    psfs = g8_fig2_psfs.npz: '1p5x_lr/point_sted_psf' (1 view) or '2p0x_lr/line_sted_psfs' (4 views)
    nl   = Deconvolver(psfs).H(obj);  rng = np.random.default_rng(7), fresh per case;  m_v = rng.poisson(nl_v) + 1e-9, views in order
    plain iterate() from ones;  D = accel_reference.i_divergence(m, H(estimate)),  d = 2 D / (V ny nx), after every second iteration
"""
import functools
import math
import os

import numpy as np

from accel_reference import i_divergence
from oracle import line_sted_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DISCREPANCY, RELATIVE = 'discrepancy', 'relative'
POINT, LINE = '1p5x_lr/point_sted_psf', '2p0x_lr/line_sted_psfs'

# (object, PSF set, photons): d at k = 2, 10, 20, 60 as printed; first even k with d <= 1; first even k with
# (D_prev - D) / D_prev <= 1e-3 (None: none up to 60)
TABLE = {
    ('lines', POINT, 1e5): (('1.020', '0.998', '0.995', '0.991'), 8, 12),
    ('astronaut', POINT, 1e5): (('1.140', '1.018', '1.005', '0.995'), 34, 26),
    ('lines', POINT, 1e6): (('1.257', '1.034', '1.015', '1.003'), None, 28),
    ('lines', LINE, 1e6): (('1.053', '1.003', '0.997', '0.992'), 14, 18),
    ('astronaut', LINE, 1e6): (('1.296', '1.018', '1.000', '0.992'), 22, 26),
    ('lines', LINE, 1e7): (('1.558', '1.080', '1.033', '1.003'), None, 44),
    ('astronaut', LINE, 1e8): (('31.0', '3.46', '1.74', '1.12'), None, None),
}


def pixel_terms(m, p):
    """The term of every pixel, float64: p > 0: ((m > 0 ? m log(m / p) : 0) - m) + p;  p <= 0 or nan: m > 0 ? 0 : -m."""
    m = np.asarray(m, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    ok = p > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.where(m > 0, m * np.log(m / np.where(ok, p, 1.0)), 0.0)
        return np.where(ok, (a - m) + p, np.where(m > 0, 0.0, -m))


def divergence(m, p):
    """D of one frame: the exactly rounded sum (math.fsum) of its pixel terms."""
    return math.fsum(pixel_terms(m, p).ravel())


THREADS, VECS_PER_THREAD, MAX_BLOCKS = 256, 8, 256        # stop_kernels.hpp / accel_kernels.hpp


def stop_blocks(n_frame, itemsize):
    """Workgroups per frame of n_frame values (stop_kernels.hpp stop_blocks)."""
    nvec = -(-n_frame // (16 // itemsize))
    return min(max(-(-nvec // (THREADS * VECS_PER_THREAD)), 1), MAX_BLOCKS)


def chain_length(n_frame, itemsize):
    """L, the longest chain of additions of the order stop_kernels.hpp states for a frame of n_frame values: a thread's
    ceil(vpb / threads) vectors of W elements, the log2(threads) levels of the workgroup tree, the nb partials of the frame."""
    W = 16 // itemsize
    nb = stop_blocks(n_frame, itemsize)
    vpb = -(-(-(-n_frame // W)) // nb)
    return -(-vpb // THREADS) * W + int(math.log2(THREADS)) + nb


def summation_bound(m, p, chain):
    """|D - fsum| <= 2^-52 (8 sum(|m log(m / p)| + |m| + |p|) + chain * sum|term|) for a float64 sum of the terms in any order whose
    longest chain of additions is `chain`: a term's own rounding (a quotient, a log good to a few ulp, a product, two additions: 8 ulp
    of its largest part is generous) plus one rounding of at most the running sum's size per addition of the chain."""
    m = np.asarray(m, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    ok = p > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.where(ok & (m > 0), np.abs(m * np.log(m / np.where(ok, p, 1.0))), 0.0)
    mag = np.where(ok, a + np.abs(m) + np.abs(p), np.abs(m))
    t = np.abs(pixel_terms(m, p))
    return 2.0 ** -52 * (8.0 * float(np.sum(mag)) + chain * float(np.sum(t)))


def rule_met(rule, threshold, count, d, d_prev=None):
    """The rules exactly as the header writes them, on float64 scalars; d_prev None: no previous check."""
    d = float(d)
    if not math.isfinite(d):
        return False
    if rule == DISCREPANCY:
        return 2.0 * d / float(count) <= threshold
    if rule == RELATIVE:
        return d_prev is not None and math.isfinite(d_prev) and float(d_prev) - d <= threshold * float(d_prev)
    raise ValueError(rule)


def first_stop(ds, rule, threshold, count):
    """Index of the first check of the trace `ds` that meets the rule, or None."""
    for i, d in enumerate(ds):
        if rule_met(rule, threshold, count, d, ds[i - 1] if i > 0 else None):
            return i
    return None


def psf_set(key):
    return list(np.load(os.path.join(GOLDEN, 'g8_fig2_psfs.npz'))[key])


def case_measurement(name, key, photons):
    """(psfs, [m_v (1, ny, nx) per view]) of a study case."""
    psfs = psf_set(key)
    obj = np.load(os.path.join(GOLDEN, 'objects.npz'))[name][0][None].astype(np.float64)
    obj = obj * (photons / obj.sum())
    nl = orc.Deconvolver(psfs).H(obj)
    rng = np.random.default_rng(7)
    return psfs, [rng.poisson(v) + 1e-9 for v in nl]


def oracle_trace(psfs, meas, k_max, check_every, keep_estimates=True):
    """Plain Richardson-Lucy from ones on ONE frame by the oracle; after every check_every iterations (and after the last):
    (k, D, estimate, prediction).  meas: [m_v (1, ny, nx)]."""
    d = orc.Deconvolver(psfs)
    d.noisy_measurement = [np.asarray(m, dtype=np.float64) for m in meas]
    out = []
    for k in range(1, k_max + 1):
        d.iterate()
        if k % check_every == 0 or k == k_max:
            pred = d.H(d.estimate)
            out.append((k, i_divergence(d.noisy_measurement, pred), d.estimate.copy() if keep_estimates else None, pred))
    return out


@functools.lru_cache(maxsize=None)
def case_trace(name, key, photons, k_max=60, check_every=2):
    psfs, meas = case_measurement(name, key, photons)
    return psfs, meas, oracle_trace(psfs, meas, k_max, check_every)


def contract_bound(meas, pred, rel=1e-10):
    """How far D may move when the prediction moves by rel * max(pred) (the float64 plan's contract against the oracle, normwise
    over the frame's views): dD/dp = 1 - m / p, so |dD| <= sum|1 - m / p| * rel * max p."""
    m = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in meas])
    p = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in pred])
    return float(np.sum(np.abs(1.0 - m / p)) * rel * np.max(p))
