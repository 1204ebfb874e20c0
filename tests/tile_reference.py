"""The numpy twin of tiled Richardson-Lucy (rescan_line_sted_amd/csrc/tile_layout.hpp, tile_kernels.hpp):
the layout rule and the weights in exact integer and float64 arithmetic -- bit for bit what the C++ computes --, the gather as
slicing, the blend in the device's order of operations, and the tiled oracle: oracle/line_sted_oracle.py's Deconvolver on every
tile, blended here.  Pure numpy: nothing of the product is imported."""
import numpy as np


def check_params(tile, overlap, margin):
    if tile < 1:
        raise ValueError('tile must be at least 1')
    if not 0 < overlap < tile:
        raise ValueError('the overlap must satisfy 0 < overlap < tile')
    if margin < 0 or 2 * margin >= overlap:
        raise ValueError('the margin must satisfy 0 <= margin and 2 * margin < overlap')


def axis_origins(n, tile, overlap):
    """Origins of the tiles of an axis of n pixels (int64 array) and the tiles' length."""
    if n < 1 or tile < 1:
        raise ValueError('n and tile must be at least 1')
    if not 0 < overlap < tile:
        raise ValueError('the overlap must satisfy 0 < overlap < tile')
    if n <= tile:
        return np.zeros(1, dtype=np.int64), n
    s = tile - overlap
    count = -(-(n - tile) // s) + 1
    return np.array([(i * (n - tile)) // (count - 1) for i in range(count)], dtype=np.int64), tile


def raw_weights(t, margin, origins):
    """[count][t] float64: min(1, left ramp, right ramp) of every tile."""
    count = len(origins)
    j = np.arange(t, dtype=np.float64)
    w = np.ones((count, t), dtype=np.float64)
    for i in range(count):
        if i > 0:
            R = np.float64(int(origins[i - 1]) + t - int(origins[i]) - 2 * margin)
            w[i] = np.minimum(w[i], np.clip(((j - margin) + 0.5) / R, 0.0, 1.0))
        if i < count - 1:
            R = np.float64(int(origins[i]) + t - int(origins[i + 1]) - 2 * margin)
            w[i] = np.minimum(w[i], np.clip(((t - margin - j) - 0.5) / R, 0.0, 1.0))
    return w


def axis_weights(n, t, margin, origins):
    """(normalised weights [count][t], first covering tile [n], number of covering tiles [n]).  W[g] sums the raw weights of the
    covering tiles in increasing tile order from 0.0."""
    w = raw_weights(t, margin, origins)
    W = np.zeros(n, dtype=np.float64)
    first = np.full(n, -1, dtype=np.int32)
    cover = np.zeros(n, dtype=np.int32)
    for i, a in enumerate(origins):
        a = int(a)
        W[a:a + t] = W[a:a + t] + w[i]
        first[a:a + t] = np.where(first[a:a + t] < 0, i, first[a:a + t])
        cover[a:a + t] += 1
    assert np.all(cover >= 1) and np.all(W > 0.0), 'a pixel without weight'
    wn = np.stack([w[i] / W[int(a):int(a) + t] for i, a in enumerate(origins)])
    return wn, first, cover


class Layout:
    """The tiles of a (NY, NX) image: tile and overlap one number or (y, x); tiles ordered frame-major, then iy, then ix."""

    def __init__(self, shape, tile, overlap, margin):
        self.shape = (int(shape[0]), int(shape[1]))
        tile = (tile, tile) if np.isscalar(tile) else tuple(tile)
        overlap = (overlap, overlap) if np.isscalar(overlap) else tuple(overlap)
        self.margin = int(margin)
        for ax in (0, 1):
            check_params(int(tile[ax]), int(overlap[ax]), self.margin)
        self.origins_y, ty = axis_origins(self.shape[0], int(tile[0]), int(overlap[0]))
        self.origins_x, tx = axis_origins(self.shape[1], int(tile[1]), int(overlap[1]))
        self.tile_shape = (ty, tx)
        self.weights_y, self.first_y, self.cover_y = axis_weights(self.shape[0], ty, self.margin, self.origins_y)
        self.weights_x, self.first_x, self.cover_x = axis_weights(self.shape[1], tx, self.margin, self.origins_x)

    @property
    def tiles_per_frame(self):
        return len(self.origins_y) * len(self.origins_x)

    def slots(self, frames):
        """(frames * tiles_per_frame, 3) int32: (frame, a_y, a_x)."""
        return np.array([(f, ay, ax) for f in range(frames) for ay in self.origins_y for ax in self.origins_x], dtype=np.int32).reshape(-1, 3)


def gather(src, slots, tile_shape, dtype):
    """src (F, V, NY, NX) -> (len(slots), V, ty, tx) of `dtype`: numpy slicing, fillers (frame -1) ones."""
    ty, tx = tile_shape
    out = np.empty((len(slots), src.shape[1], ty, tx), dtype=dtype)
    for k, (f, ay, ax) in enumerate(np.asarray(slots).reshape(-1, 3)):
        out[k] = 1 if f < 0 else src[f, :, ay:ay + ty, ax:ax + tx].astype(dtype)
    return out


def blend(tiles, layout, dtype=np.float64):
    """tiles (F, nyt, nxt, ty, tx) or (F * nyt * nxt, ty, tx), any float type -> (F, NY, NX) of `dtype`: per pixel the sum from 0.0 over
    iy ascending (outer) and ix ascending (inner) of (wy * wx) * float64(e), rounded once to `dtype`."""
    nyt, nxt = len(layout.origins_y), len(layout.origins_x)
    ty, tx = layout.tile_shape
    tiles = np.asarray(tiles).reshape(-1, nyt, nxt, ty, tx)
    acc = np.zeros((tiles.shape[0],) + layout.shape, dtype=np.float64)
    for iy, ay in enumerate(layout.origins_y):
        for ix, ax in enumerate(layout.origins_x):
            w = layout.weights_y[iy][:, None] * layout.weights_x[ix][None, :]
            region = acc[:, ay:ay + ty, ax:ax + tx]
            acc[:, ay:ay + ty, ax:ax + tx] = region + w[None] * tiles[:, iy, ix].astype(np.float64)
    return acc.astype(dtype)


def oracle_tile_estimates(measurement, psfs, iterations, layout):
    """The oracle's Richardson-Lucy on every tile: measurement (F, V, NY, NX) -> (F, nyt, nxt, ty, tx) float64."""
    from oracle import line_sted_oracle as orc
    measurement = np.asarray(measurement, dtype=np.float64)
    F, V = measurement.shape[:2]
    ty, tx = layout.tile_shape
    out = np.empty((F, len(layout.origins_y), len(layout.origins_x), ty, tx))
    for f in range(F):
        for iy, ay in enumerate(layout.origins_y):
            for ix, ax in enumerate(layout.origins_x):
                out[f, iy, ix] = oracle_estimate(measurement[f, :, ay:ay + ty, ax:ax + tx], psfs, iterations, orc)
    return out


def oracle_estimate(measurement, psfs, iterations, orc=None):
    """`iterations` oracle iterations from ones on one (V, ny, nx) measurement -> (ny, nx)."""
    if orc is None:
        from oracle import line_sted_oracle as orc
    d = orc.Deconvolver([np.asarray(p, dtype=np.float64) for p in psfs])
    d.noisy_measurement = [np.array(m, dtype=np.float64)[None] for m in measurement]
    for _ in range(iterations):
        d.iterate()
    return d.estimate[0]


def tiled_oracle(measurement, psfs, iterations, tile, overlap, margin):
    """Tiled Richardson-Lucy by the oracle: (estimate (F, NY, NX) float64, layout)."""
    measurement = np.asarray(measurement, dtype=np.float64)
    layout = Layout(measurement.shape[-2:], tile, overlap, margin)
    return blend(oracle_tile_estimates(measurement, psfs, iterations, layout), layout), layout


def normwise(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def pixelwise(a, b, floor=1e-3):
    """Largest relative deviation on the pixels of b above `floor` of its maximum."""
    m = np.abs(b) > floor * np.max(np.abs(b))
    return float(np.max(np.abs(a - b)[m] / np.abs(b)[m]))


# ---- shared cases of the CPU and the GPU tests ---------------------------------------------------------------------------------

def psf(shape, rank1, rng):
    """A random normalised (1, py, px) PSF, rank 1 (an outer product) or full."""
    if rank1:
        u, v = rng.random(shape[0]) + 0.2, rng.random(shape[1]) + 0.2
        p = np.outer(u, v)
    else:
        p = rng.random(shape) + 0.05
    return (p / p.sum())[None]


# (psf shape, rank 1, iterations): exact_margin = 2 K hw = 8 for each
EXACT_CASES = [((5, 5), True, 2), ((5, 5), False, 2), ((4, 4), False, 2), ((9, 9), False, 1)]


def exact_case(case, margin):
    """(measurement (1, 1, 60, 52), psfs, K, tile 40, overlap 2 m + 4 ...) of one exactness case."""
    shape, rank1, K = case
    rng = np.random.default_rng(100 * shape[0] + K + (1 if rank1 else 0))
    psfs = [psf(shape, rank1, rng)]
    meas = rng.random((1, 1, 60, 52)) * 50.0 + 10.0
    return meas, psfs, K, 40, 2 * margin + 4
