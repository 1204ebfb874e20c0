"""Reference of the angle-resolved ring statistics (include/rlsted.h, rl_ring_sector_stats): the sector of every bin decided
exactly, the cell statistics from numpy's fft2, and the error bound the kernels are held to.  TEST INFRASTRUCTURE ONLY.

The sector.  With Y = sy nx, X = sx ny folded into the upper half plane, u = S theta / pi + 1/2 and sector = floor(u) mod S.  A
float64 guess of u decides every bin that is further than 1e-6 from an integer (the guess is good to about 1e-15).  For the
others, with m the integer nearest to u, the question is whether theta is below the boundary (m - 1/2) pi / S or not:
z = X + i Y has argument theta, so z^(2 S) has argument 2 S theta = (2 m - 1) pi + d with d small, and Im z^(2 S) = -|z|^(2 S) sin d.
In Python integers: Im < 0 -> above the boundary, sector m; Im = 0 -> exactly on it, a TIE, which the half-open rule gives to the
upper sector m; Im > 0 -> sector m - 1.

The bound is ring_reference's, per cell instead of per ring: the per-bin spectrum error E = gamma_L (||a||_1 + |s| ||b||_1) with
the same chain length L (ROWS, COLS and the unpack are the same code), summed over the cell's bins, plus the cell's own
summation -- a lane's chain and the wave tree are one order of adding the cell's terms, gamma_nbins(cell) sum (|A| + |B|)^2:

    |field - reference| <= sum_{bins of the cell} [4 E (|A| + |B|) + 4 E^2] + gamma_nbins sum_{bins of the cell} (|A| + |B|)^2

An empty cell has bound 0: its five fields are exactly 0.
"""
import numpy as np

import ring_reference as rr

FIELDS = rr.FIELDS


def folded(ky, kx, ny, nx):
    """(Y, X) of the definition, as Python integers."""
    sy = ky if ky <= ny // 2 else ky - ny
    sx = kx if kx <= nx // 2 else kx - nx
    Y, X = sy * nx, sx * ny
    if Y < 0 or (Y == 0 and X < 0):
        Y, X = -Y, -X
    return Y, X


def _imag_power(X, Y, n):
    """Im (X + i Y)^n in Python integers."""
    re, im = 1, 0
    for _ in range(n):
        re, im = re * X - im * Y, re * Y + im * X
    return im


def _decide(Y, X, S, m):
    """(sector, tie) of a bin whose u is near the integer m."""
    im = _imag_power(X, Y, 2 * S)
    return (m if im <= 0 else m - 1) % S, im == 0


def sector_of_bin(ky, kx, ny, nx, S):
    """(sector, tie) of one bin: the definition."""
    Y, X = folded(ky, kx, ny, nx)
    if Y == 0 and X == 0:
        return 0, False
    u = S * float(np.arctan2(float(Y), float(X))) / np.pi + 0.5
    m = int(round(u))
    if abs(u - m) < 1e-6:
        return _decide(Y, X, S, m)
    return int(np.floor(u)) % S, False


_tables = {}


def sector_table(ny, nx, S):
    """((ny, nx) int64 sector of every bin, (ny, nx) bool: the bin lies exactly on a sector boundary)."""
    key = (ny, nx, int(S))
    if key not in _tables:
        sy = np.where(np.arange(ny) <= ny // 2, np.arange(ny), np.arange(ny) - ny).astype(np.int64)
        sx = np.where(np.arange(nx) <= nx // 2, np.arange(nx), np.arange(nx) - nx).astype(np.int64)
        Y = np.broadcast_to(sy[:, None] * nx, (ny, nx)).copy()
        X = np.broadcast_to(sx[None, :] * ny, (ny, nx)).copy()
        flip = (Y < 0) | ((Y == 0) & (X < 0))
        Y[flip], X[flip] = -Y[flip], -X[flip]
        u = S * np.arctan2(Y.astype(np.float64), X.astype(np.float64)) / np.pi + 0.5       # (|Y|, |X| < 2^24: exact in float64)
        sec = np.floor(u).astype(np.int64) % S
        tie = np.zeros((ny, nx), dtype=bool)
        m = np.rint(u).astype(np.int64)
        for ky, kx in np.argwhere(np.abs(u - m) < 1e-6):
            sec[ky, kx], tie[ky, kx] = _decide(int(Y[ky, kx]), int(X[ky, kx]), int(S), int(m[ky, kx]))
        sec[0, 0] = 0
        sec.setflags(write=False)
        tie.setflags(write=False)
        _tables[key] = (sec, tie)
    return _tables[key]


def cell_table(ny, nx, S, n_rings=None):
    """(ny, nx) int64: ring * S + sector of every bin, R * S where the bin belongs to no ring."""
    R = rr.default_rings(ny, nx) if n_rings is None else int(n_rings)
    ring = rr.ring_table(ny, nx, R)
    return np.where(ring < R, ring * S + sector_table(ny, nx, S)[0], R * S)


def _label_sums(values, labels, n):
    """Sums of `values` over the bins of each label 0 .. n - 1 (labels >= n: none), in extended precision."""
    order = np.argsort(labels.ravel(), kind='stable')
    lab = labels.ravel()[order]
    v = values.ravel()[order].astype(np.longdouble)
    out = np.zeros(n + 1, dtype=np.longdouble)
    present, starts = np.unique(lab, return_index=True)
    out[np.minimum(present, n)] = np.add.reduceat(v, starts)
    return out[:n]


def sector_stats(a, b, S, scale=1.0, n_rings=None):
    """[R][S][5] float64 for one pair."""
    ny, nx = np.shape(a)
    R = rr.default_rings(ny, nx) if n_rings is None else int(n_rings)
    cells = cell_table(ny, nx, S, R)
    A, B = rr.spectra(a, b, scale)
    out = np.zeros((R * S, FIELDS))
    out[:, 0] = np.bincount(cells.ravel(), minlength=R * S + 1)[:R * S]
    out[:, 1] = _label_sums(np.abs(A) ** 2, cells, R * S)
    out[:, 2] = _label_sums(np.abs(B) ** 2, cells, R * S)
    out[:, 3] = _label_sums((A * np.conj(B)).real, cells, R * S)
    out[:, 4] = _label_sums(np.abs(A - B) ** 2, cells, R * S)
    return out.reshape(R, S, FIELDS)


def bound(a, b, S, scale=1.0, n_rings=None):
    """[R][S] the largest admissible |field - reference| of fields 1..4 per cell (module docstring); 0 for an empty cell."""
    ny, nx = np.shape(a)
    R = rr.default_rings(ny, nx) if n_rings is None else int(n_rings)
    cells = cell_table(ny, nx, S, R)
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    A, B = rr.spectra(a, b, scale)
    E = rr.gamma(rr.chain_length(ny, nx)) * (np.abs(a).sum() + abs(float(scale)) * np.abs(b).sum())
    mag = np.abs(A) + np.abs(B)
    nb = np.bincount(cells.ravel(), minlength=R * S + 1)[:R * S]
    first = _label_sums(4.0 * E * mag + 4.0 * E * E, cells, R * S).astype(np.float64)
    second = rr.gamma(nb.astype(np.float64)) * _label_sums(mag ** 2, cells, R * S).astype(np.float64)
    return (first + second).reshape(R, S)


def grating(ny, nx, fy, fx):
    """cos(2 pi (fy y / ny + fx x / nx)): all of its power in the bins (fy, fx) and (-fy, -fx)."""
    y, x = np.mgrid[0:ny, 0:nx]
    return np.cos(2.0 * np.pi * (fy * y / ny + fx * x / nx))


# ------------------------------------------------------------------ what the CPU and the GPU tests share
# (mean, offset) of the Poisson images per shape, dim enough that the ORACLE's bound stays below 1e-9 of field 1 in every non-empty
# cell (a cell of two bins holds one Rayleigh draw of noise power: these seeds and levels were checked with the oracle alone)
LEVEL = {(8, 8): (200.0, 20.0), (37, 50): (100.0, 10.0), (96, 160): (0.05, 0.01), (160, 160): (0.05, 0.01)}


def check_cells(got, a, b, scale, R, S, label, guard=True):
    """The cells of one pair against sector_reference under the derived bound (printed first); guard: the bound is at most 1e-9 of
    field 1 in every non-empty cell.  Empty cells are five zeros."""
    want = sector_stats(a, b, S, scale, R)
    bnd = bound(a, b, S, scale, R)
    full = want[..., 0] > 0
    err = np.abs(got[..., 1:] - want[..., 1:]).max(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        print('%s: max err / bound %.3g, max bound / field1 %.3g, %d of %d cells empty'
              % (label, float(np.max(err[full] / bnd[full])), float(np.nanmax(bnd[full] / want[..., 1][full])), int((~full).sum()), full.size))
    assert np.array_equal(got[..., 0], want[..., 0]), label
    assert np.all(got[~full] == 0.0), label
    if guard:
        assert np.all(bnd[full] <= 1e-9 * want[..., 1][full]), (label, float(np.max(bnd[full] / want[..., 1][full])))
    assert np.all(err <= bnd), (label, float(np.max(err[full] / bnd[full])))
    return int((~full).sum())


# (shape, S, (fy, fx), the sector it must land in): along kx, along ky, the two diagonals (the second pins the sign of theta), and
# a grating exactly on the physical 45 degree boundary of S = 2, which the tie rule gives to the upper sector
GRATINGS = [((16, 16), 4, (0, 3), 0), ((16, 16), 4, (3, 0), 2), ((16, 16), 4, (2, 2), 1), ((16, 16), 4, (14, 2), 3),
            ((24, 40), 2, (3, 5), 1)]


def check_grating(got, shape, S, f, sector):
    """All of field 1 in the one cell (ring of the bin, `sector`); everything under the general bound."""
    ny, nx = shape
    R = rr.default_rings(ny, nx)
    a, b = grating(ny, nx, *f), np.zeros(shape)
    ring = int(rr.ring_table(ny, nx, R)[f[0] % ny, f[1] % nx])
    assert ring < R and sector_of_bin(f[0] % ny, f[1] % nx, ny, nx, S)[0] == sector
    check_cells(got, a, b, 1.0, R, S, 'grating %s at %dx%d S=%d' % (f, ny, nx, S), guard=False)
    total = 2.0 * (ny * nx / 2.0) ** 2                                               # |A|^2 of the two bins +-f
    assert abs(got[ring, sector, 1] - total) <= bound(a, b, S, 1.0, R)[ring, sector] + 1e-12 * total
    rest = got[..., 1].copy()
    rest[ring, sector] = 0.0
    assert np.all(rest <= bound(a, b, S, 1.0, R) + 1e-20 * total)                 # (numpy's own zeros are ~1e-28 of the total)


