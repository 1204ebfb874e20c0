"""Reference of the ring statistics (include/rlsted.h, rl_ring_stats): numpy's fft2 and the ring table in exact Python integers
(math.isqrt), and the error bound the kernels are held to.  TEST INFRASTRUCTURE ONLY.

The bound, per ring and field 1..4 (field 0, the number of bins, is exact), with A = fft2(a), B = fft2(s b) from numpy:

    u = 2^-53,  gamma_k = k u / (1 - k u)
    E = gamma_L (||a||_1 + |s| ||b||_1)
    |field - reference| <= sum_bins [4 E (|A| + |B|) + 4 E^2] + gamma_nbins sum_bins (|A| + |B|)^2

E bounds the error of one spectrum value: |dA|, |dB| <= E turns |A - B + d|^2, |d| <= 2 E, into at most 4 E (|A| + |B|) + 4 E^2 of
change, and the other three fields into less.  The last term is the summation of the ring's terms in any order.

L, the longest accumulation chain of the implementation (csrc/ring_kernels.hpp), for an image (ny, nx):
  * PACK                 1 rounding (s * b)
  * ROWS                 a complex dot product of nx terms, each component 2 nx fused multiply-adds in sequence: 2 nx roundings,
                         plus 1 for the rounded table entry exp(-2 pi i m / nx)
  * COLS                 likewise 2 ny + 1; its inputs are bounded by the row sums of |Z|, so the two stages' relative errors add
  * unpack               1 (the sum F[k] +- conj F[-k]; the halving is exact)
  so each COMPONENT of F carries at most gamma_(2 nx + 2 ny + 4) sum |Z|; the complex modulus of the error sqrt(2) times that.
  sqrt(2) (2 nx + 2 ny + 4) <= 3 (nx + ny) + 6.
  * the ring terms       |A|^2 etc.: a product, a fused multiply-add, at most two differences -- at most 4 roundings relative to
                         (|A| + |B|)^2.  As |A| <= ||a||_1 and |B| <= |s| ||b||_1, 4 E (|A| + |B|) >= 2 gamma_L (|A| + |B|)^2, so two
                         more units of L pay for them; the thread sums and the workgroup tree are a summation order of the ring's
                         terms (adding the zeros of idle threads is exact), covered by the gamma_nbins term.
  L = 3 (ny + nx) + 16   (the remaining 8: second-order products of the gammas, generously)
"""
import math

import numpy as np

FIELDS = 5
U = 2.0 ** -53


def default_rings(ny, nx):
    return min(ny, nx) // 2


def chain_length(ny, nx):
    """L of the module docstring."""
    return 3 * (ny + nx) + 16


def gamma(k):
    return k * U / (1.0 - k * U)


def ring_of_bin(ky, kx, ny, nx, n_rings):
    """The definition, in Python integers."""
    sy = ky if ky <= ny // 2 else ky - ny
    sx = kx if kx <= nx // 2 else kx - nx
    q = (sy * nx) ** 2 + (sx * ny) ** 2
    return math.isqrt(4 * n_rings * n_rings * q) // (ny * nx)


_tables = {}


def ring_table(ny, nx, n_rings=None):
    """(ny, nx) int64 array: the ring of every bin, n_rings where the bin belongs to none.  (Each distinct q once.)"""
    R = default_rings(ny, nx) if n_rings is None else int(n_rings)
    key = (ny, nx, R)
    if key not in _tables:
        sy = np.array([k if k <= ny // 2 else k - ny for k in range(ny)], dtype=object)
        sx = np.array([k if k <= nx // 2 else k - nx for k in range(nx)], dtype=object)
        q = (sy[:, None] * nx) ** 2 + (sx[None, :] * ny) ** 2            # Python integers
        M = ny * nx
        ring_of_q = {v: min(math.isqrt(4 * R * R * v) // M, R) for v in set(q.ravel().tolist())}
        t = np.array([ring_of_q[v] for v in q.ravel().tolist()], dtype=np.int64).reshape(ny, nx)
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


def float_ring_table(ny, nx, n_rings=None):
    """What a float64 formula gives instead: int(sqrt((sy / ny)^2 + (sx / nx)^2) * 2 R) -- NOT the definition."""
    R = default_rings(ny, nx) if n_rings is None else int(n_rings)
    sy = np.where(np.arange(ny) <= ny // 2, np.arange(ny), np.arange(ny) - ny) / ny
    sx = np.where(np.arange(nx) <= nx // 2, np.arange(nx), np.arange(nx) - nx) / nx
    return np.minimum((np.sqrt(sy[:, None] ** 2 + sx[None, :] ** 2) * (2 * R)).astype(np.int64), R)


def _ring_sums(values, table, R):
    """Per-ring sums of `values` (ny, nx) in extended precision."""
    order = np.argsort(table.ravel(), kind='stable')
    rings = table.ravel()[order]
    v = values.ravel()[order].astype(np.longdouble)
    out = np.zeros(R + 1, dtype=np.longdouble)
    present, starts = np.unique(rings, return_index=True)
    out[present] = np.add.reduceat(v, starts)
    return out[:R]


def spectra(a, b, scale=1.0):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.fft.fft2(a), np.fft.fft2(float(scale) * b)


def ring_stats(a, b, scale=1.0, n_rings=None):
    """[R][5] float64 for one pair."""
    ny, nx = np.shape(a)
    R = default_rings(ny, nx) if n_rings is None else int(n_rings)
    table = ring_table(ny, nx, R)
    A, B = spectra(a, b, scale)
    out = np.zeros((R, FIELDS))
    out[:, 0] = np.bincount(table.ravel(), minlength=R + 1)[:R]
    out[:, 1] = _ring_sums(np.abs(A) ** 2, table, R)
    out[:, 2] = _ring_sums(np.abs(B) ** 2, table, R)
    out[:, 3] = _ring_sums((A * np.conj(B)).real, table, R)
    out[:, 4] = _ring_sums(np.abs(A - B) ** 2, table, R)
    return out


def bound(a, b, scale=1.0, n_rings=None):
    """[R] the largest admissible |field - reference| of fields 1..4 per ring (module docstring)."""
    ny, nx = np.shape(a)
    R = default_rings(ny, nx) if n_rings is None else int(n_rings)
    table = ring_table(ny, nx, R)
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    A, B = spectra(a, b, scale)
    E = gamma(chain_length(ny, nx)) * (np.abs(a).sum() + abs(float(scale)) * np.abs(b).sum())
    mag = np.abs(A) + np.abs(B)
    nb = np.bincount(table.ravel(), minlength=R + 1)[:R]
    first = _ring_sums(4.0 * E * mag + 4.0 * E * E, table, R).astype(np.float64)
    second = gamma(nb.astype(np.float64)) * _ring_sums(mag ** 2, table, R).astype(np.float64)
    return first + second


def poisson_pair(rng, ny, nx, mean=200.0, offset=20.0):
    """Two Poisson draws of a smooth object plus an offset: every ring holds noise power."""
    y, x = np.mgrid[0:ny, 0:nx]
    obj = offset + mean * (np.exp(-((y - 0.4 * ny) ** 2 / (0.02 * ny * ny + 1) + (x - 0.55 * nx) ** 2 / (0.03 * nx * nx + 1)))
                           + 0.5 * (1 + np.sin(0.7 * x + 0.3 * y)))
    return rng.poisson(obj).astype(np.float64), rng.poisson(obj).astype(np.float64), obj
