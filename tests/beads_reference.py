"""The numpy twin of rl_find_peaks (include/rlsted.h; rescan_line_sted_amd/csrc/bead_kernels.hpp) and the constructed images of its
tests.  The twin follows the definition's order exactly: the row and the column pass are loops over k with whole-array operations,
every value in float64, products and sums rounded on their own -- so its bits are the device's bits.  Also the analytic bead stacks
of the method tests (tests/test_beads_cpu.py, tests/test_gpu_beads.py)."""
import numpy as np

TY, TX = 16, 32              # the launcher's tile (bead_kernels.hpp kBpTY, kBpTX)


def taps(sigma):
    """(w, h) as beads.find_beads forms them: exp(-k^2 / 2 sigma^2) over k = -h .. h normalised, h = int(4 sigma + 0.5)."""
    h = int(4.0 * sigma + 0.5)
    k = np.arange(-h, h + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum(), h


def smooth(x, w):
    """s over the whole image, nan where the stencil does not fit (rows / columns within h of the border)."""
    x = np.asarray(x, dtype=np.float64)
    ny, nx = x.shape
    h = (len(w) - 1) // 2
    u = np.zeros((ny, nx - 2 * h))
    for j in range(2 * h + 1):
        u = u + w[j] * x[:, j:nx - 2 * h + j]
    s = np.zeros((ny - 2 * h, nx - 2 * h))
    for k in range(2 * h + 1):
        s = s + w[k] * u[k:ny - 2 * h + k, :]
    out = np.full((ny, nx), np.nan)
    out[h:ny - h, h:nx - h] = s
    return out


def find_peaks(image, w, r, b, rel, threshold):
    """Every candidate of one image: dict(yx (K, 2) int64 in row-major order, s (K,), x (K,), count, levels (lo, hi, t))."""
    x = np.asarray(image, dtype=np.float64)
    ny, nx = x.shape
    S = smooth(x, w)
    D = S[b:ny - b, b:nx - b]
    vals = D[~np.isnan(D)]
    lo = float(vals.min()) if vals.size else np.inf
    hi = float(vals.max()) if vals.size else -np.inf
    with np.errstate(invalid='ignore', over='ignore'):
        v = float(np.float64(lo) + np.float64(rel) * (np.float64(hi) - np.float64(lo)))
    t = v if v > threshold else float(threshold)
    with np.errstate(invalid='ignore'):
        cand = D >= t
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                Q = S[b + dy:ny - b + dy, b + dx:nx - b + dx]
                cand &= (Q < D) if (dy < 0 or (dy == 0 and dx < 0)) else (Q <= D)
    ys, xs = np.nonzero(cand)
    yx = np.stack([ys + b, xs + b], axis=1).astype(np.int64)
    return {'yx': yx, 's': D[ys, xs].copy(), 'x': x[yx[:, 0], yx[:, 1]].copy(), 'count': len(ys), 'levels': np.array([lo, hi, t])}


# ---- constructed images --------------------------------------------------------------------------------------------------------------

def seam_scene(h=2, r=3, seed=5):
    """An image of two whole tiles plus a partial tile on each axis plus 2 b, b = h + r, on a noisy background of small integers, with
    (name -> pixel) of what it holds: a plateau inside one tile and one across the column seam of the first two tiles (constant
    blocks: s is constant to the bit where the stencil lies inside), a tie after and a tie before a peak within r (identical
    neighbourhoods: the symmetric taps make the two sums the same bits), peaks at distance b (in D) and b - 1 (outside it) from the
    border, a peak with a nan pixel inside its window."""
    b = h + r
    ny, nx = 2 * TY + 7 + 2 * b, 2 * TX + 9 + 2 * b
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, size=(ny, nx)).astype(np.float64)
    marks = {}
    e = h + 1                                               # half size of a constant block with a 3 x 3 plateau of s

    def block(cy, cx, v):
        x[cy - e:cy + e + 1, cx - e:cx + e + 1] = v

    def quiet(y0, y1, x0, x1):                              # a zero box: equal neighbourhoods
        x[y0:y1, x0:x1] = 0.0
    block(b + 6, b + 10, 60.0)
    marks['plateau'] = (b + 6 - 1, b + 10 - 1)              # the plateau's first pixel
    block(b + 8, b + TX, 70.0)                              # across the seam x = b + TX
    marks['plateau_seam'] = (b + 8 - 1, b + TX - 1)
    quiet(b + TY + 1, b + TY + 1 + 2 * (h + r) + 4, b + 4, b + 4 + 2 * (h + r) + 6)
    py, px = b + TY + 1 + h + r + 2, b + 4 + h + r + 2
    x[py, px] = x[py, px + 2] = 50.0                        # tie after p: p is the candidate, p + (0, 2) is not
    marks['tie_after'], marks['tie_loser_after'] = (py, px), (py, px + 2)
    quiet(b + 2 * TY - 8, ny - b, b + 2 * TX - 20, b + 2 * TX + 2)
    qy, qx = b + 2 * TY - 8 + h + r + 1, b + 2 * TX - 20 + h + r + 4
    x[qy, qx] = x[qy + 1, qx - 2] = 45.0                    # tie before: (qy, qx) comes first in row-major order
    marks['tie_before'], marks['tie_loser_before'] = (qy, qx), (qy + 1, qx - 2)
    x[b, b + 60] = 80.0                                     # at distance b: in D
    x[b - 1, b + 70] = 90.0                                 # at distance b - 1: outside D
    x[ny - 1 - b, nx - 1 - b] = 80.0                        # the last pixel of D
    marks['border_in'], marks['border_out'], marks['border_last'] = (b, b + 60), (b - 1, b + 70), (ny - 1 - b, nx - 1 - b)
    x[b + 12, b + 50] = 85.0
    x[b + 12, b + 52] = np.nan                              # nan within r of the peak: disqualified
    marks['nan_peak'] = (b + 12, b + 50)
    return x, marks, b


def h0_scene(seed=9):
    """h = 0, r = 1: s is x; integer noise with repeated values (ties) and a few isolated highs."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 6, size=(TY * 2 + 3, TX + 5)).astype(np.float64)
    x[5, 7] = x[20, 30] = 12.0
    return x


# ---- analytic bead stacks ---------------------------------------------------------------------------------------------------------

SIGMAS = ((1.3, 2.0), (2.0, 1.3))        # per view (sigma_y, sigma_x)


def gauss_bead(ny, nx, cy, cx, sy, sx, flux):
    """A point-sampled anisotropic Gaussian of the given flux (its continuous integral) centred at (cy, cx)."""
    y = np.arange(ny)[:, None] - cy
    x = np.arange(nx)[None, :] - cx
    return flux / (2.0 * np.pi * sy * sx) * np.exp(-0.5 * (y * y / (sy * sy) + x * x / (sx * sx)))


def bead_centres(ny, nx, spacing, edge, rng):
    """Sub-pixel centres on a jittered grid at least `spacing` apart, `edge` pixels from the border."""
    ys = np.arange(edge, ny - edge, spacing)
    xs = np.arange(edge, nx - edge, spacing)
    c = np.array([(y, x) for y in ys for x in xs], dtype=np.float64)
    return c + rng.uniform(-0.5, 0.5, size=c.shape)


def bead_stack(F, ny, nx, size, noise, seed=3, flux=5000.0, background=20.0, dark=100.0, spacing=None, edge=None):
    """(raw (F, V, ny, nx), truths [V] of (size, size) normalised) for the views of SIGMAS: every frame holds beads at its own
    sub-pixel centres; noise=True: Poisson counts of (bead + background), plus the dark level, as uint16 (gain 1); noise=False: the
    float32 expectation plus dark."""
    rng = np.random.default_rng(seed)
    spacing = size + 3 if spacing is None else spacing
    edge = size // 2 + 14 if edge is None else edge
    V = len(SIGMAS)
    raw = np.empty((F, V, ny, nx), dtype=np.uint16 if noise else np.float32)
    for f in range(F):
        for v, (sy, sx) in enumerate(SIGMAS):
            img = np.full((ny, nx), background)
            for cy, cx in bead_centres(ny, nx, spacing, edge, rng):
                img += gauss_bead(ny, nx, cy, cx, sy, sx, flux)
            raw[f, v] = (rng.poisson(img) + dark) if noise else (img + dark)
    half = size // 2
    truths = []
    for sy, sx in SIGMAS:
        t = gauss_bead(size, size, half, half, sy, sx, 1.0)
        truths.append(t / t.sum())
    return raw, truths


def fwhm(sigma):
    return 2.0 * np.sqrt(2.0 * np.log(2.0)) * abs(sigma)


# ---- the twin of the whole method: measure_psfs on a numpy device ---------------------------------------------------------------------

class Buf:
    def __init__(self, a, dtype):
        self.a, self.dtype = a, dtype


_RAW = {0: np.uint8, 1: np.uint16, 2: np.int16, 3: np.float32}


class NumpyDevice:
    """beads._BeadDevice in numpy: the ingest of tests/ingest_reference.py, the twin above for rl_find_peaks, slicing for the gather,
    per-pixel folds in list order for rl_ensemble_stats, registration._estimate on the long-double sums and the scipy shift of
    tests/register_reference.py for rl_register_estimate, and that shift for rl_shift_images.  calls: the log of what was asked;
    fields: what every estimate answered, (n, 3) = ncc, at_limit, flat of ALL its windows, in call order."""

    def __init__(self, device=0):
        self.calls = []
        self.fields = []

    def alloc(self, elements, dtype):
        np_dt = {None: np.uint8, 'f32': np.float32, 'f64': np.float64}[dtype]
        return Buf(np.zeros(max(int(elements), 1), dtype=np_dt), dtype)

    def upload(self, buf, array, byte_offset=0):
        b = np.ascontiguousarray(array).view(np.uint8).ravel()
        buf.a.view(np.uint8)[byte_offset:byte_offset + b.size] = b

    def download(self, buf, elements, element_offset=0):
        return buf.a[element_offset:element_offset + int(elements)].astype(np.float64)

    def ingest(self, raw, code, images, sensor, origin, frame_stride, view_stride, n_slots, n_valid, V, shape, camera, dark, dst, stats):
        import ingest_reference as ir
        self.calls.append(('ingest', images, frame_stride, view_stride, n_slots, V, tuple(origin), tuple(shape)))
        src = raw.a.view(_RAW[code])[:images * sensor[0] * sensor[1]].reshape(images, sensor[0], sensor[1])
        out, st = ir.ingest(src, n_slots, n_valid, V, shape[0], shape[1], origin[0], origin[1], frame_stride, view_stride,
                            None if dark is None else dark.a.reshape(shape), camera.dark, camera.gain, camera.epsilon,
                            0.0 if camera.saturation is None else camera.saturation, dst.a.dtype)
        dst.a[:out.size] = out.ravel()
        stats.a[:st.size] = st.ravel()

    def find_peaks(self, src, offsets, ny, nx, w, r, b, rel, threshold, cap):
        self.calls.append(('find_peaks', list(offsets), ny, nx, len(w), r, b, rel, threshold, cap))
        out, counts, levels = [], [], []
        for o in offsets:
            p = find_peaks(src.a[o:o + ny * nx].reshape(ny, nx), w, r, b, rel, threshold)
            out.append({'yx': p['yx'][:cap], 's': p['s'][:cap], 'x': p['x'][:cap]})
            counts.append(p['count'])
            levels.append(p['levels'])
        return out, np.array(counts, dtype=np.int64), np.array(levels)

    def gather(self, src, n_images, ny, nx, slots, size, dst):
        self.calls.append(('gather', len(slots), size))
        for k, (i, ay, ax) in enumerate(slots):
            img = src.a[i * ny * nx:(i + 1) * ny * nx].reshape(ny, nx)
            assert 0 <= ay and ay + size <= ny and 0 <= ax and ax + size <= nx
            dst.a[k * size * size:(k + 1) * size * size] = img[ay:ay + size, ax:ax + size].ravel()

    def group_stats(self, src, members, group_ptr, n_pixels, mean=None, var=None):
        self.calls.append(('group_stats', len(members)))
        assert len(group_ptr) == 2
        xs = [src.a[o:o + n_pixels].astype(np.float64) for o in members]
        n = len(xs)
        m = np.zeros(n_pixels)
        for x in xs:
            m = m + x
        m = m / n
        ss = np.zeros(n_pixels)
        for x in xs:
            ss = ss + (x - m) * (x - m)
        if mean is not None:
            mean.a[:n_pixels] = m
        if var is not None:
            var.a[:n_pixels] = ss / (n - 1) if n > 1 else 0.0
        return np.array([[n, m.sum(), 0.0, 0.0, 0.0, 0.0]])

    def sums(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M):
        import register_reference as rr
        W = 2 * R + 1
        S, A = np.empty((len(mov_offsets), W * W, 3)), np.empty((len(mov_offsets), 2))
        for k, (ro, mo) in enumerate(zip(ref_offsets, mov_offsets)):
            s, a, _, _ = rr.sums(ref.a[ro:ro + ny * nx].reshape(ny, nx), mov.a[mo:mo + ny * nx].reshape(ny, nx), R, M)
            S[k], A[k] = s.astype(np.float64), a.astype(np.float64)
        return S, A

    def gather_shift(self, src, offsets, ny, nx, shifts, dst, order=3):
        import register_reference as rr
        for k, o in enumerate(offsets):
            dst.a[k * ny * nx:(k + 1) * ny * nx] = rr.shift(src.a[o:o + ny * nx].reshape(ny, nx), shifts[k], order).ravel()

    def estimate(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M, refine, scratch, surfaces=False):
        from rescan_line_sted_amd import registration
        self.calls.append(('estimate', len(mov_offsets), ny, nx, R, M, refine))
        s, info = registration._estimate(self, ref, list(ref_offsets), mov, list(mov_offsets), ny, nx, R, refine, M, scratch)
        fields = np.stack([info['ncc'], info['at_limit'].astype(np.float64), info['flat'].astype(np.float64)], axis=1)
        self.fields.append(fields.copy())
        return s, fields, None

    def shift(self, src, src_element, n, ny, nx, shifts, order, floor, dst, dst_element=0):
        import register_reference as rr
        self.calls.append(('shift', n, order))
        sh = np.asarray(shifts, dtype=np.float64).reshape(n, 2)
        for k in range(n):
            o = src_element + k * ny * nx
            out = rr.shift(src.a[o:o + ny * nx].reshape(ny, nx), sh[k], order, floor)
            dst.a[dst_element + k * ny * nx:dst_element + (k + 1) * ny * nx] = out.ravel()
        return np.zeros((n, 2))

    def close(self):
        self.calls.append('close')
