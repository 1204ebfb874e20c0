"""Constructed rows of registration sums for the peak search on the device (include/rlsted.h rl_register_peaks): every way the
first-maximum search, the tree, the border rule, the flat rule and the parabola can go wrong, and the host's answer for each
(rescan_line_sted_amd/registration.py ncc_surface + surface_peak), which the device must give bit for bit.

A row is [nd * 3 + 2] float64: S_b, S_bb, S_ab per displacement d = (dy + R)(2R + 1) + dx + R, then S_a, S_aa, as
rl_register_sums' totals leave them.  All values are generic doubles (random, not round numbers), so every division and square
root is a real rounding."""
import numpy as np

N_TERMS = 400.0


def _random_row(rng, R):
    nd = (2 * R + 1) ** 2
    s0 = rng.random(nd) * 100.0
    s1 = s0 * s0 / N_TERMS + 1.0 + rng.random(nd)
    s2 = rng.random(nd) * 10.0 - 5.0
    sa = rng.random() * 50.0
    row = np.empty(nd * 3 + 2)
    row[0:nd * 3:3], row[1:nd * 3:3], row[2:nd * 3:3] = s0, s1, s2
    row[nd * 3], row[nd * 3 + 1] = sa, sa * sa / N_TERMS + 2.0 + rng.random()
    return row


def _boost(row, d, by=1e3):
    """Displacement d becomes the largest NCC of the row."""
    row[3 * d + 2] += by


def _copy(row, src, dst):
    row[3 * dst:3 * dst + 3] = row[3 * src:3 * src + 3]


def rows(R, seed=0):
    """{name: row} for radius R: R = 1 has 9 displacements in 256 threads, R = 8 289 (one pass of the threads plus 33), R = 32 4225."""
    rng = np.random.default_rng(seed * 1000 + R)
    W, nd = 2 * R + 1, (2 * R + 1) ** 2
    c = R * W + R                                                          # the centre, d = (0, 0)
    out = {}
    for k in range(3):
        out['random_%d' % k] = _random_row(rng, R)
    r = _random_row(rng, R)
    _boost(r, c + W + 1, 40.0)                                             # an interior peak off the centre: both parabolas
    out['interior'] = r
    # equal maxima: the first in row-major order wins
    pairs = {'tie_threads': (1, 3)} if nd < 256 else {'tie_threads': (5, 100)}
    if nd > 266:
        pairs['tie_same_thread'] = (10, 266)                               # thread 10 sees both, in increasing order
        pairs['tie_later_in_lower_thread'] = (200, 260)                    # thread 200 holds the first, thread 4 the later one
    for name, (p, q) in pairs.items():
        r = _random_row(rng, R)
        _boost(r, p)
        _copy(r, p, q)
        out[name] = r
    # border peaks: each border and each corner gives at_limit and no sub-pixel part
    for name, (iy, ix) in {'top': (0, R), 'bottom': (W - 1, R), 'left': (R, 0), 'right': (R, W - 1), 'corner_00': (0, 0),
                           'corner_0w': (0, W - 1), 'corner_w0': (W - 1, 0), 'corner_ww': (W - 1, W - 1)}.items():
        r = _random_row(rng, R)
        _boost(r, iy * W + ix)
        out['border_' + name] = r
    # flat: va = 0; one vb = 0 away from the peak; one vb nan
    r = _random_row(rng, R)
    r[nd * 3 + 1] = r[nd * 3] * r[nd * 3] / N_TERMS
    out['flat_va'] = r
    r = _random_row(rng, R)
    _boost(r, c)
    far = nd - 1
    r[3 * far + 1] = r[3 * far] * r[3 * far] / N_TERMS
    out['flat_vb'] = r
    r = _random_row(rng, R)
    _boost(r, c)
    r[3 * far + 1] = np.nan
    out['flat_vb_nan'] = r
    # plateau: the peak z = 1 at the centre, p = 1 after it on both axes, m = 1 - 2^-53 before it (m = z exactly would make m the
    # first maximum).  (m - 2 z) rounds to -2 + ... = -1 exactly (a tie to even), so den = (m - 2 z) + p = 0 and delta = 0.
    r = _random_row(rng, R)
    r[0:nd * 3:3] = 0.0
    r[1:nd * 3:3] = 4.0
    r[2:nd * 3:3] = rng.random(nd) * 1.9
    r[nd * 3], r[nd * 3 + 1] = 0.0, 1.0
    for d, s2 in ((c, 2.0), (c + 1, 2.0), (c + W, 2.0), (c - 1, np.nextafter(2.0, 0.0)), (c - W, np.nextafter(2.0, 0.0))):
        r[3 * d + 2] = s2
    out['plateau'] = r
    return out


def estimate_images(dt):
    """Six 40 x 48 images of one scene and the scene as their reference: four small displacements, one of 6 px (beyond R = 4: at
    the limit) and a flat one."""
    import register_reference as rr
    p = rr.blobs(3, 40, 48)
    ref = rr.scene(p).astype(dt)
    imgs = [rr.scene(p, d) for d in ((0.3, -0.7), (-1.2, 2.4), (2.6, 0.9), (0.0, 0.0), (6.0, -1.0))] + [np.full((40, 48), 3.0)]
    return np.stack(imgs).astype(dt), ref


def expected(row, R, n=N_TERMS):
    """The host's (fields [5] = shift_y, shift_x, value, at_limit, flat; surface [nd]) of one row."""
    from rescan_line_sted_amd import registration as reg
    nd = (2 * R + 1) ** 2
    surf, flat = reg.ncc_surface(row[:nd * 3].reshape(nd, 3), row[nd * 3:], n)
    if flat:
        return np.array([0.0, 0.0, 0.0, 0.0, 1.0]), surf.ravel()
    s, v, lim = reg.surface_peak(surf)
    return np.array([s[0], s[1], v, float(lim), 0.0]), surf.ravel()
