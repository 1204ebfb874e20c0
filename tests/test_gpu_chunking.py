"""Every chunked host call of the C ABI run in several chunks on the MI355X (include/rlsted.h rl_chunk_bytes, rl_chunks_run).

The calls below cut their work into chunks whose workspace stays under a cap held by the context; at the default caps every shape
of the suite fits one chunk, so without this file nothing after the first trip of those loops -- the advanced offset tables and
output pointers, the reused per-chunk scratch, the state rl_fig3_scan carries from chunk to chunk -- is ever executed.  Every case
follows one pattern (_in_chunks): the call at the default cap (rl_chunks_run == 1), under a cap of one byte (one item per chunk:
n trips) and under the share of two items with an odd n (ceil(n / 2) trips, the last chunk short); every output of the chunked runs
equals the one-chunk output BIT FOR BIT (compared as unsigned integers, so nan payloads and signed zeros count), and the one-chunk
output is held to the call's twin under the bound its own test file uses.  The counter assertions are what holds each case to the
chunking it meant to run: with an ignored cap a run would be compared with itself.

The share of two items is known in closed form where the cap counts whole images (shift, ring, fig3); elsewhere (_cap_for) it is the
smallest cap at which the counter shows ceil(n / 2), found by bisection on the counter."""
import contextlib
import ctypes

import numpy as np
import pytest

import affine_reference as ar
import beads_reference as br
import register_reference as rr
import ring_reference as ring
import sector_reference as sr
import xcorr_reference as xr
from oracle import figure3_oracle as f3
from test_gpu_beads import device_peaks
from test_gpu_fig3 import device_simulate
from test_gpu_register import K, _camera, _psfs, _stack
from test_gpu_ring import _check as check_rings
from test_gpu_xcorr import _displaced

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}


def _L():
    from rescan_line_sted_amd import _lib
    return _lib


def _reg():
    from rescan_line_sted_amd import registration
    return registration


@pytest.fixture(scope='module')
def dev():
    """A registration device on a context of this module's own: the caps set here are not those of the default context."""
    L = _L()
    d = _reg()._Device(device=0)
    d.ctx = L.Context(0)
    yield d
    d.close()
    L.lib.rl_ctx_destroy(d.ctx.handle)


def _buffer(dev, array, dtype):
    buf = dev.alloc(array.size, dtype)
    dev.upload(buf, np.ascontiguousarray(array, dtype=NP[dtype]))
    return buf


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (what, k)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), (what, 'output %d' % k)


@contextlib.contextmanager
def _caps(ctx, **caps):
    """The caps given, in bytes, for the calls inside; the defaults afterwards whatever happens."""
    try:
        for which, nbytes in caps.items():
            ctx.chunk_bytes(which, nbytes)
        yield
    finally:
        for which in caps:
            ctx.chunk_bytes(which, _L().CHUNK_DEFAULTS[which])


def _cap_for(ctx, which, run, trips):
    """The smallest cap under which `run` makes at most `trips` trips of the loop of `which`: a bisection on the counter (a trip
    count never grows with the cap).  The caller asserts that the count at this cap is exactly `trips`."""
    lo, hi = 1, 1 << 24
    with _caps(ctx, **{which: hi}):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            ctx.chunk_bytes(which, mid)
            run()
            lo, hi = (lo, mid) if ctx.chunks_run(which) <= trips else (mid, hi)
    return hi


def _in_chunks(ctx, which, n, run, what, two=None):
    """The pattern of this file for a call of n items (n odd) under the cap `which`.  run() makes the call and returns a tuple of
    its output arrays; two: the share of two items in bytes where it is known, else it is searched.  Returns the one-chunk outputs."""
    assert n % 2 == 1 and n >= 3
    whole = run()
    assert ctx.chunks_run(which) == 1, what
    half = -(-n // 2)
    two = _cap_for(ctx, which, run, half) if two is None else two
    for cap, trips in ((1, n), (two, half)):
        with _caps(ctx, **{which: cap}):
            got = run()
            assert ctx.chunks_run(which) == trips, (what, 'cap %d: %d trips, meant %d' % (cap, ctx.chunks_run(which), trips))
        _assert_same(got, whole, (what, 'cap %d' % cap))
    _assert_same(run(), whole, (what, 'the default cap again'))
    assert ctx.chunks_run(which) == 1, what
    return whole


# ---- rl_register_sums, rl_affine_sums ------------------------------------------------------------------------------------------------

def test_register_sums_in_chunks(dev):
    """5 pairs of 40 x 56, R = 3, M = 3, ref f32 and moving f64; the reference offsets descend and repeat (pairs 0 and 4, 1 and 3
    share an image) and the moving ones are shuffled, so a chunk that restarted its offset tables at 0 would read other images."""
    ny, nx, R, M = 40, 56, 3, 3
    n_pix = ny * nx
    rng = np.random.default_rng(401)
    a = (rng.random(3 * n_pix + 5) * 100.0).astype(np.float32)
    b = (rng.random(5 * n_pix + 3) * 100.0).astype(np.float32)
    a_off = [2 * n_pix + 5, 5, n_pix + 5, 5, 2 * n_pix + 5]
    b_off = [3 + k * n_pix for k in (4, 0, 2, 1, 3)]
    ab, bb = _buffer(dev, a, 'f32'), _buffer(dev, b, 'f64')
    S, A = _in_chunks(dev.ctx, 'register_sums', 5, lambda: dev.sums(ab, a_off, bb, b_off, ny, nx, R, M), 'rl_register_sums')
    for i in range(5):
        want, ref, bound, ref_bound = rr.sums(a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), b[b_off[i]:b_off[i] + n_pix].reshape(ny, nx), R, M)
        assert np.all(np.abs(S[i].astype(np.longdouble) - want).astype(np.float64) <= bound), i
        assert np.all(np.abs(A[i].astype(np.longdouble) - ref).astype(np.float64) <= ref_bound), i


def test_affine_sums_in_chunks(dev):
    """5 pairs of 37 x 53, M = 4, ref f64 and warped f32, shuffled offsets with shared references (the cap is that of the register
    sums)."""
    ny, nx, M = 37, 53, 4
    n_pix = ny * nx
    rng = np.random.default_rng(402)
    a = (rng.random(3 * n_pix + 5) * 100.0).astype(np.float32)
    w = (rng.random(5 * n_pix + 3) * 100.0).astype(np.float32)
    a_off = [2 * n_pix + 5, 5, n_pix + 5, 5, 2 * n_pix + 5]
    w_off = [3 + k * n_pix for k in (4, 0, 2, 1, 3)]
    ab, wb = _buffer(dev, a, 'f64'), _buffer(dev, w, 'f32')
    S, = _in_chunks(dev.ctx, 'register_sums', 5, lambda: (dev.affine_sums(ab, a_off, wb, w_off, ny, nx, M),), 'rl_affine_sums')
    for i in range(5):
        want, bound = ar.affine_sums(a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), w[w_off[i]:w_off[i] + n_pix].reshape(ny, nx), M)
        assert np.all(np.abs(S[i].astype(np.longdouble) - want).astype(np.float64) <= bound), i
        assert S[i, 35] == (ny - 2 * M) * (nx - 2 * M)


# ---- rl_shift_images -------------------------------------------------------------------------------------------------------------------

SHIFTS5 = [(0.37, -0.81), (-1.5, 0.25), (2.6, 3.3), (-0.45, -2.75), (1.2, 0.9)]


def _shift_call(dev, sb, db, n, ny, nx, shifts, order, floor, with_stats, guard=8):
    """rl_shift_images into the destination db, refilled with sentinels: `guard` of them stay on either side; stats_out given or
    NULL."""
    L = _L()
    ddt = db.dtype
    whole = np.full(n * ny * nx + 2 * guard, 7, dtype=NP[ddt])
    dev.upload(db, whole)
    sh = np.ascontiguousarray(shifts, dtype=np.float64).reshape(n, 2)
    stats = np.full((n, 2), -7.0) if with_stats else None
    L.check(L.lib.rl_shift_images(dev.ctx.handle, sb.ptr, L.DTYPES[sb.dtype], n, ny, nx, L.ptr(sh), order, float(floor), db.at(guard),
                                  L.DTYPES[ddt], L.ptr(stats) if with_stats else None))
    back = dev.download(db, whole.size)
    assert np.all(back[:guard] == 7) and np.all(back[guard + n * ny * nx:] == 7), 'written outside the destination'
    return back[guard:guard + n * ny * nx].reshape(n, ny, nx), stats


@pytest.mark.parametrize('sdt,ddt', [('f32', 'f64'), ('f64', 'f32')])
@pytest.mark.parametrize('order', [1, 3])
def test_shift_images_in_chunks(dev, order, sdt, ddt):
    """5 images of 37 x 53 with distinct non-integer shifts; a floor of 50 that raises pixels in images 1 and 3 alone (the others
    stay above 400); stats_out given and NULL.  The one-chunk result against scipy as tests/test_gpu_register.py holds it."""
    n, ny, nx, floor = 5, 37, 53, 50.0
    rng = np.random.default_rng(403 + order)
    src = (rng.random((n, ny, nx)) * 1000.0).astype(np.float32)
    src[0::2] = 500.0 + 0.1 * src[0::2]
    src[1::2, 10:14, 20:30] = 0.0                        # (a patch that stays below the floor under either order)
    sb, db = _buffer(dev, src, sdt), dev.alloc(n * ny * nx + 16, ddt)
    two = 2 * ny * nx * 8
    for with_stats in (True, False):
        got, stats = _in_chunks(dev.ctx, 'shift', n, lambda: _shift_call(dev, sb, db, n, ny, nx, SHIFTS5, order, floor, with_stats),
                                'rl_shift_images order %d %s -> %s stats %s' % (order, sdt, ddt, with_stats), two)
        want = np.stack([rr.shift(src[k], SHIFTS5[k], order, floor) for k in range(n)])
        if ddt == 'f64':
            assert np.abs(got - want).max() / np.abs(src).max() <= 1e-12
        else:
            w32 = want.astype(np.float32)
            assert np.all(np.abs(got - w32.astype(np.float64)) <= np.spacing(np.abs(w32)))
        if with_stats:
            assert np.all(stats[1::2, 0] > 0) and np.all(stats[0::2, 0] == 0), stats[:, 0]
            assert np.array_equal(stats[:, 0], (got == floor).sum(axis=(1, 2)))
            for k in range(n):
                assert abs(stats[k, 1] - got[k].sum()) <= rr.gamma(ny * nx) * np.abs(got[k]).sum()
        else:
            assert stats is None


# ---- rl_register_estimate --------------------------------------------------------------------------------------------------------------

EST_D = [(1.3, -0.7), (-2.25, 1.6), None, (0.4, 2.2), (-1.1, -1.9), None, (2.3, 0.6)]      # None: a flat moving image
EST_SLOT = [0, 1, 5, 2, 4, 3, 7]                        # the moving image of pair i, in images of the buffer (slot 6 is not used)


def test_register_estimate_in_chunks(dev):
    """7 pairs of 40 x 56, R = 3, M = 6, refine = 2, surfaces asked for; ref f32, moving f64.  Pairs 2 and 5 are flat, so the
    refine passes run on 5 of 7.  The moving images of the live pairs lie at slots 0 1 2 | 4 | 7: by default a pass shifts them in 3
    launches (the run of three, two alone), under a shift cap of two images in 4, of one byte in 5.  The sums cap and the shift
    cap are lowered alone and together; both counters are asserted each time (the sums counter is that of the first stage: 7
    pairs).  The one-chunk call against the host path of estimate_shifts byte for byte and against the twin within 1e-6 px, as
    tests/test_gpu_register_pipeline.py and tests/test_gpu_register.py hold it."""
    reg = _reg()
    ny, nx, R, M, refine, n = 40, 56, 3, 6, 2, 7
    n_pix = ny * nx
    scenes = [rr.blobs(seed, ny, nx) for seed in (31, 32, 33)]
    refs = np.stack([rr.scene(p) for p in scenes]).astype(np.float32)
    ref_of = [2, 0, 1, 0, 2, 1, 1]
    mov = np.full((8, ny, nx), 1e30)
    for i, d in enumerate(EST_D):
        mov[EST_SLOT[i]] = 37.5 if d is None else rr.scene(scenes[ref_of[i]], d, (1.5, 0.7) if i % 2 else (0.0, 0.0))
    rb, mb = _buffer(dev, np.concatenate([np.zeros(5), refs.ravel()]), 'f32'), _buffer(dev, np.concatenate([np.zeros(3), mov.ravel()]), 'f64')
    ro, mo = [5 + k * n_pix for k in ref_of], [3 + k * n_pix for k in EST_SLOT]
    scratch = dev.alloc(n * n_pix, 'f64')
    ctx = dev.ctx

    def run():
        return dev.estimate(rb, ro, mb, mo, ny, nx, R, M, refine, scratch, True)

    def counters():
        return ctx.chunks_run('register_sums'), ctx.chunks_run('shift')
    whole = run()
    assert counters() == (1, 3)
    shifts, fields, C = whole
    live = [i for i in range(n) if EST_D[i] is not None]
    assert [bool(f) for f in fields[:, 2]] == [d is None for d in EST_D] and not fields[:, 1].any()
    two_sums, two_shift = _cap_for(ctx, 'register_sums', run, 4), 2 * n_pix * 8
    for caps, want in (({'register_sums': 1}, (7, 3)), ({'register_sums': two_sums}, (4, 3)), ({'shift': 1}, (1, 5)),
                       ({'shift': two_shift}, (1, 4)), ({'register_sums': 1, 'shift': 1}, (7, 5)),
                       ({'register_sums': two_sums, 'shift': two_shift}, (4, 4))):
        with _caps(ctx, **caps):
            got = run()
            assert counters() == want, (caps, counters(), want)
        _assert_same(got, whole, ('rl_register_estimate', caps))
    # the host path of the same estimate, at the default caps: the same bytes
    hs, hinfo = reg._estimate(dev, rb, ro, mb, mo, ny, nx, R, refine, M, dev.alloc(n * n_pix, 'f64'), surfaces=True)
    _assert_same((shifts, fields[:, 0], C.reshape(n, 2 * R + 1, 2 * R + 1)), (hs, hinfo['ncc'], hinfo['surfaces']), 'device against host estimate')
    assert np.array_equal(fields[:, 1] != 0, hinfo['at_limit']) and np.array_equal(fields[:, 2] != 0, hinfo['flat'])
    worst = 0.0
    for i in live:
        w, wi = rr.estimate(mov[EST_SLOT[i]], refs[ref_of[i]], R, refine, M)
        assert rr.margin_of(wi['surface']) > 1e-6 and not wi['at_limit']
        worst = max(worst, float(np.abs(shifts[i] - w).max()))
        assert abs(fields[i, 0] - wi['ncc']) < 1e-9
    print('rl_register_estimate against the twin: worst %.3g px' % worst)
    assert worst <= 1e-6
    assert not shifts[[2, 5]].any()


# ---- rl_register_xcorr -----------------------------------------------------------------------------------------------------------------

XC_TRUE = [(-8, 8), (4, -1), (0, 0), (8, -8), (-3, 5)]


@pytest.mark.parametrize('surfaces', [True, False])
def test_register_xcorr_in_chunks(dev, surfaces):
    """5 pairs of 40 x 56 at R = 8 (both transform lengths 64), ref f32 and moving f64, two shared references, the moving images in
    reversed order, pair 1 a hundred times weaker; with and without surface_out.  The one-chunk call against the twin as
    tests/test_gpu_xcorr.py holds it."""
    ny, nx, R, n = 40, 56, 8, 5
    n_pix, W = ny * nx, 17
    rng = np.random.default_rng(405)
    a = (rng.random(2 * n_pix + 5) * 1000.0 + 100.0).astype(np.float32)
    b = np.zeros(n * n_pix + 3, dtype=np.float32)
    a_off = [5 + (k % 2) * n_pix for k in range(n)]
    b_off = [3 + k * n_pix for k in reversed(range(n))]
    for k in range(n):
        ref = a[a_off[k]:a_off[k] + n_pix].reshape(ny, nx).astype(np.float64)
        b[b_off[k]:b_off[k] + n_pix] = (_displaced(rng, ref, XC_TRUE[k]) * (0.01 if k == 1 else 1.0)).ravel()
    ab, bb = _buffer(dev, a, 'f32'), _buffer(dev, b, 'f64')

    def run():
        out = dev.xcorr(ab, a_off, bb, b_off, ny, nx, R, surfaces)
        return out if surfaces else (out,)
    out = _in_chunks(dev.ctx, 'xcorr', n, run, 'rl_register_xcorr surfaces %s' % surfaces)
    P = out[0]
    cnt = xr.counts(ny, nx, R)
    for i in range(n):
        A, B = a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), b[b_off[i]:b_off[i] + n_pix].reshape(ny, nx)
        f, v, _, bound = xr.xcorr(A, B, R)
        lead = np.sort(v.ravel())
        assert (f[0], f[1]) == XC_TRUE[i] and lead[-1] - lead[-2] > 2 * bound / cnt.min()
        assert (P[i][0], P[i][1]) == XC_TRUE[i] and abs(P[i][2] - f[2]) <= bound / cnt.min()
        assert P[i][3] == f[3] and P[i][4] == f[4]
        assert abs(P[i][5] - f[5]) <= (bound / cnt).sum() and abs(P[i][6] - f[6]) <= (2 * np.abs(v) * bound / cnt + (bound / cnt) ** 2).sum() * 1.01
        if surfaces:
            err = np.abs(out[1][i].astype(np.float64) - v) - 0.5 * np.spacing(np.abs(v).astype(np.float32))
            assert np.all(err <= bound / cnt), i
            iy, ix = divmod(int(np.argmax(out[1][i])), W)
            assert (iy - R, ix - R) == XC_TRUE[i]


# ---- rl_ring_stats, rl_ring_sector_stats ---------------------------------------------------------------------------------------------

RING_SHAPE = (24, 36)
RING_SCALE = [1.0, 0.61, 1.7, 0.31, 2.5]


def _ring_case(dev):
    """5 pairs of 24 x 36: a in an f32 buffer and b in an f64 buffer (Poisson counts: float32 numbers), both at shuffled, odd
    offsets."""
    ny, nx = RING_SHAPE
    pix = ny * nx
    rng = np.random.default_rng(406)
    pairs = [ring.poisson_pair(rng, ny, nx)[:2] for _ in range(5)]
    a_slot, b_slot = (3, 0, 4, 1, 2), (1, 4, 0, 2, 3)
    ha, hb = np.zeros(5 * pix + 1), np.zeros(5 * pix + 3)
    a_off, b_off = [1 + s * pix for s in a_slot], [3 + s * pix for s in b_slot]
    for (x, y), ao, bo in zip(pairs, a_off, b_off):
        ha[ao:ao + pix], hb[bo:bo + pix] = x.ravel(), y.ravel()
    return pairs, _buffer(dev, ha, 'f32'), a_off, _buffer(dev, hb, 'f64'), b_off


def _ring_run(dev, case, scale, n_rings, S):
    from rescan_line_sted_amd import quality
    _, ab, a_off, bb, b_off = case
    head = (dev.ctx, ab.ptr, 'f32', a_off, bb.ptr, 'f64', b_off, RING_SHAPE)
    return (quality.ring_stats_device(*head, scale, n_rings) if S is None else quality.sector_stats_device(*head, S, scale, n_rings),)


@pytest.mark.parametrize('scaled', [True, False])
@pytest.mark.parametrize('S', [None, 3])
def test_ring_stats_in_chunks(dev, S, scaled):
    """rl_ring_stats (S None) and rl_ring_sector_stats (S = 3) with n_rings = rl_ring_count, b_scale distinct per pair and NULL.  A
    chunk's share is its two spectra, 2 * 16 * ny * nx bytes per pair (the 3-sector results are smaller).  The one-chunk call
    against numpy as tests/test_gpu_ring.py and tests/test_gpu_sector.py hold it."""
    from rescan_line_sted_amd import quality
    ny, nx = RING_SHAPE
    R = quality.ring_count(ny, nx)
    assert R == 12
    case = _ring_case(dev)
    scale = RING_SCALE if scaled else None
    two = 2 * 2 * 16 * ny * nx
    got, = _in_chunks(dev.ctx, 'ring', 5, lambda: _ring_run(dev, case, scale, R, S), 'ring statistics S %s scaled %s' % (S, scaled), two)
    for k, (x, y) in enumerate(case[0]):
        s = RING_SCALE[k] if scaled else 1.0
        if S is None:
            check_rings(got[k], x, y, s, R, '24x36 pair %d' % k, guard=False)
        else:
            sr.check_cells(got[k], x, y, s, R, S, '24x36 S=3 pair %d' % k, guard=False)


def test_sector_results_can_be_the_binding_cap(dev):
    """300 rings of 3 sectors are 36000 bytes of results per pair, more than the 27648 bytes of a pair's spectra.  Under a cap of two
    pairs' spectra the results allow one pair per chunk (5 trips) where 12 rings run in chunks of two (3 trips): the counter shows
    which share bound.  Under two pairs' results: 3 trips.  The bits of the default cap, and numpy."""
    ny, nx = RING_SHAPE
    R, S = 300, 3
    per_out, per_img = R * S * ring.FIELDS * 8, 2 * 16 * ny * nx
    assert per_img < per_out < 2 * per_img
    case = _ring_case(dev)
    ctx = dev.ctx
    whole = _ring_run(dev, case, RING_SCALE, R, S)
    assert ctx.chunks_run('ring') == 1
    for cap, rings, trips in ((2 * per_img, 12, 3), (2 * per_img, R, 5), (2 * per_out, R, 3), (1, R, 5)):
        with _caps(ctx, ring=cap):
            got = _ring_run(dev, case, RING_SCALE, rings, S)
            assert ctx.chunks_run('ring') == trips, (cap, rings, ctx.chunks_run('ring'), trips)
        if rings == R:
            _assert_same(got, whole, ('300 rings', cap))
    for k in (0, 4):
        sr.check_cells(whole[0][k], case[0][k][0], case[0][k][1], RING_SCALE[k], R, S, '24x36 300 rings S=3 pair %d' % k, guard=False)


# ---- rl_fig3_scan ----------------------------------------------------------------------------------------------------------------------

FIG3_TYPES = [('descan_point', 1), ('nondescan_multipoint', 1), ('descan_line', 3), ('rescan_line', 3)]
_FIG3 = {}


def _fig3_case(imaging_type, n_orient, monkeypatch):
    """The 27 x 38 object of tests/test_gpu_fig3.py's test_other_shapes_vs_oracle (R = 1.5, 3 pulses) through simulate_imaging on
    the default context, against the CPU oracle frame by frame at 1e-10, with every rl_fig3_scan it makes recorded: its arguments
    (copied) and what came back.  Returns (the oracle's frames, the recorded calls, obj, pad)."""
    if imaging_type in _FIG3:
        return _FIG3[imaging_type]
    from rescan_line_sted_amd import line_sted_figure_3 as fig3
    L = _L()
    real = L.lib.rl_fig3_scan
    calls = []

    def spy(ctx, prm, obj, exc, pos, n_pos, disp, n_disp, sc, vals, frames, cum):
        rc = real(ctx, prm, obj, exc, pos, n_pos, disp, n_disp, sc, vals, frames, cum)
        p = fig3._Params.from_buffer_copy(ctypes.cast(prm, ctypes.POINTER(fig3._Params)).contents)
        n = p.ny * p.nx

        def arr(ptr, shape):
            return None if ptr is None else np.ctypeslib.as_array(ptr, shape).copy()
        ry = -(-p.n_y // p.exc_sep) if p.exc_sep else 0
        rx = -(-p.n_x // p.exc_sep) if p.exc_sep else 0
        n_val = p.nx if p.imaging_type == 2 else ry * rx
        calls.append(dict(prm=p, obj=arr(obj, (n,)), exc=arr(exc, (n,)), pos=arr(pos, (n_pos, 2)), n_pos=n_pos, n_val=n_val,
                          sc=arr(sc, (n_pos, 4)), vals=arr(vals, (n_pos, n_val)) if n_val else None, cum=arr(cum, (p.ny, p.nx))))
        return rc
    monkeypatch.setattr(L.lib, 'rl_fig3_scan', spy)
    rng = np.random.default_rng(11)
    obj = rng.random((1, 27, 38)) + 1e-6
    pad = 9 if n_orient == 1 else int(0.45 * 38)
    want, got = [], []
    f3.simulate_imaging(obj, imaging_type, 9, 1.5, n_orient, 3, pad, lambda rot, pos, *a: want.append((rot, pos, a)))
    device_simulate(fig3)(obj, imaging_type, 9, 1.5, n_orient, 3, pad, lambda rot, pos, *a: got.append((rot, pos, a)))
    monkeypatch.undo()
    _fig3_compare(got, want)
    assert len(calls) == 1 + n_orient
    _FIG3[imaging_type] = (want, calls, obj, pad)
    return _FIG3[imaging_type]


def _fig3_compare(got, want):
    assert [(int(r), p) for r, p, _ in got] == [(int(r), p) for r, p, _ in want]
    for (_, _, a), (_, _, b) in zip(got, want):
        for x, y in zip(a[:7], b[:7]):
            assert np.abs(x - y).max() < 1e-10
        assert a[7:] == b[7:]


def _fig3_scan(ctx, c, display):
    """rl_fig3_scan on the recorded arguments of one call with a display list of this test's; (rc, outputs)."""
    L = _L()
    p, n_pos, n_val = c['prm'], c['n_pos'], c['n_val']
    ip = ctypes.POINTER(ctypes.c_int)
    display = np.ascontiguousarray(display, dtype=np.int32)
    sc = np.full((n_pos, 4), -7.0)
    vals = np.full((n_pos, n_val), -7.0) if n_val else None
    frames = np.full((len(display), 2, p.ny, p.nx), -7.0)
    cum = np.full((p.ny, p.nx), -7.0) if p.imaging_type == 3 else None
    rc = L.lib.rl_fig3_scan(ctx.handle, ctypes.cast(ctypes.byref(p), ctypes.c_void_p), L.ptr(c['obj']), L.ptr(c['exc']),
                            c['pos'].ctypes.data_as(ip), n_pos, display.ctypes.data_as(ip), len(display), L.ptr(sc),
                            L.ptr(vals) if n_val else None, L.ptr(frames), L.ptr(cum) if cum is not None else None)
    return rc, (sc, vals, frames, cum)


@pytest.mark.parametrize('imaging_type,n_orient', FIG3_TYPES)
def test_fig3_scan_in_chunks(dev, monkeypatch, imaging_type, n_orient):
    """The last scan simulate_imaging makes for the 27 x 38 object (a rotated object for the line types), again on this module's
    context: in one chunk -- the bits simulate_imaging got on the default context, which the oracle holds at 1e-10 --, then in chunks
    of 1 position, of 3, and of a count that does not divide n_pos.  The display list holds the first and the last position of a
    chunk of 3 (3, 5), two neighbours across a boundary (5, 6; for the other count c: c - 1, c) and the very last position.
    pos_scalars, pos_values, display_out and cum_final -- the running sum carried across the chunks -- bit for bit."""
    _, calls, _, _ = _fig3_case(imaging_type, n_orient, monkeypatch)
    c = calls[-1]
    n_pos, img = c['n_pos'], c['prm'].ny * c['prm'].nx * 8
    odd = next(k for k in range(4, n_pos) if n_pos % k)
    display = sorted({0, 3, 5, 6, odd - 1, odd, n_pos - 1})
    assert n_pos > 2 * odd and display[-2] < n_pos - 1
    ctx = dev.ctx
    rc, whole = _fig3_scan(ctx, c, display)
    assert rc == 0 and ctx.chunks_run('fig3') == 1
    _assert_same(whole[:2] + whole[3:], (c['sc'], c['vals'], c['cum']), 'one chunk against simulate_imaging')
    assert not any(np.any(x == -7.0) for x in whole if x is not None)
    for per in (1, 3, odd):
        for cap in ((1, img) if per == 1 else (per * img, (per + 1) * img - 1)):
            with _caps(ctx, fig3=cap):
                rc, got = _fig3_scan(ctx, c, display)
                assert rc == 0 and ctx.chunks_run('fig3') == -(-n_pos // per), (cap, ctx.chunks_run('fig3'))
            _assert_same(got, whole, (imaging_type, 'chunks of %d' % per))
    print('%s: %d positions in chunks of 1, 3 and %d' % (imaging_type, n_pos, odd))


def test_fig3_rescan_through_simulate_imaging_under_a_small_cap(monkeypatch):
    """simulate_imaging('rescan_line', three orientations) with the default context's cap at three positions' images: the oracle's
    frames at the existing 1e-10, and the reconstructions of the default cap bit for bit."""
    from rescan_line_sted_amd import line_sted_figure_3 as fig3
    want, calls, obj, pad = _fig3_case('rescan_line', 3, monkeypatch)
    ctx = fig3._ctx()
    n_pos, img = calls[-1]['n_pos'], calls[-1]['prm'].ny * calls[-1]['prm'].nx * 8
    got = []
    with _caps(ctx, fig3=3 * img):
        res = device_simulate(fig3)(obj, 'rescan_line', 9, 1.5, 3, 3, pad, lambda rot, pos, *a: got.append((rot, pos, a)))
        assert ctx.chunks_run('fig3') == -(-n_pos // 3) > 1
    _fig3_compare(got, want)
    again = fig3.simulate_imaging(obj, 'rescan_line', 9, 1.5, 3, 3, pad)
    assert ctx.chunks_run('fig3') == 1
    assert sorted(res['reconstructions']) == sorted(again['reconstructions']) and res['maxima'] == again['maxima']
    for rot in again['reconstructions']:
        _assert_same((res['reconstructions'][rot],), (again['reconstructions'][rot],), 'reconstruction at %s degrees' % rot)


def test_fig3_display_errors_under_chunking(dev, monkeypatch):
    """Chunks of three positions: a display list that descends across a chunk boundary (6, 5), one that repeats an index, and one
    beyond the last position are refused as in one chunk; the context then gives the bits it gave before."""
    _, calls, _, _ = _fig3_case('rescan_line', 3, monkeypatch)
    c = calls[-1]
    n_pos, img = c['n_pos'], c['prm'].ny * c['prm'].nx * 8
    ctx = dev.ctx
    _, whole = _fig3_scan(ctx, c, [5, 6])
    with _caps(ctx, fig3=3 * img):
        for bad, text in (([6, 5], b'ascend'), ([2, 2], b'ascend'), ([-1], b'ascend'), ([5, n_pos], b'beyond'), ([n_pos - 1, n_pos], b'beyond')):
            rc, _ = _fig3_scan(ctx, c, bad)
            assert rc == -1 and text in _L().lib.rl_last_error(), bad
        rc, got = _fig3_scan(ctx, c, [5, 6])
        assert rc == 0 and ctx.chunks_run('fig3') == -(-n_pos // 3)
    _assert_same(got, whole, 'after the refused calls')


# ---- end to end, on the Python layer's default context -----------------------------------------------------------------------------

def _small(ctx):
    return _caps(ctx, **{which: 1 for which in _L().CHUNK_CAPS})


@pytest.mark.parametrize('pipeline', [False, True])
def test_registered_stack_under_small_caps(pipeline):
    """The registered stack of tests/test_gpu_register.py (u16, F = 5, V = 2, f32 plan, batch 2, estimated shifts, refine = 1) with
    every cap of the default context at one byte and at the defaults: estimates, shifts and fields bit for bit.  pipeline=True runs
    the estimate through rl_register_estimate."""
    reg, L = _reg(), _L()
    ctx = L.Context.get(0)
    raw, roi = _stack(5, 2, 44)
    kw = dict(camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=4, refine=1)
    if pipeline:
        kw.update(pipeline=True, out_dtype='f64')
    want, winfo = reg.deconvolve_stack_registered(raw, _psfs(2), K, **kw)
    assert ctx.chunks_run('register_sums') == 1 and ctx.chunks_run('shift') == 1
    with _small(ctx):
        got, info = reg.deconvolve_stack_registered(raw, _psfs(2), K, **kw)
        assert ctx.chunks_run('register_sums') > 1 and ctx.chunks_run('shift') == 4          # (the last shift: a batch of 2 x 2 images)
    assert np.abs(winfo['shifts']).max() > 0.5 and not winfo['flat'].any()
    _assert_same((got,), (want,), 'estimates')
    for k in ('shifts', 'ncc', 'at_limit', 'flat', 'view_ncc', 'view_at_limit', 'view_flat', 'raised', 'level', 'clipped'):
        _assert_same((np.asarray(info[k]),), (np.asarray(winfo[k]),), k)


def test_quality_ring_statistics_under_small_caps():
    """quality.ring_stats and sector_stats on 5 pairs of 128 x 128 host images (estimate against object under a scale per pair): one
    pair per chunk against the default cap, bit for bit."""
    from rescan_line_sted_amd import quality
    ctx = _L().Context.get(0)
    rng = np.random.default_rng(407)
    pairs = [ring.poisson_pair(rng, 128, 128, 5.0, 1.0) for _ in range(5)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[2] for p in pairs])
    scale = [p[0].sum() / p[2].sum() for p in pairs]
    for S in (None, 3):
        want = quality.ring_stats(a, b, scale=scale, n_sectors=S)
        assert ctx.chunks_run('ring') == 1
        with _small(ctx):
            got = quality.ring_stats(a, b, scale=scale, n_sectors=S)
            assert ctx.chunks_run('ring') == 5
        _assert_same((got,), (want,), 'S %s' % S)
    check_rings(quality.ring_stats(a, b, scale=scale)[4], a[4], b[4], scale[4], 64, '128x128 pair 4', guard=False)


# ---- the setters -----------------------------------------------------------------------------------------------------------------------

def test_setters_refuse_and_share_their_caps(dev):
    """rl_chunk_bytes refuses 0 bytes, an unknown `which` and a NULL context and leaves the cap as it was: shown by the counter of
    the next call.  rl_warp_chunk_bytes / rl_find_peaks_chunk_bytes and rl_chunk_bytes(RL_CHUNK_WARP / RL_CHUNK_BEADS) write one
    cap: what either sets, the warp's and the finder's counters show, and the other undoes."""
    L = _L()
    lib, ctx, h = L.lib, dev.ctx, dev.ctx.handle
    rng = np.random.default_rng(408)
    src = _buffer(dev, (rng.random((5, 12, 16)) * 100.0).astype(np.float32), 'f32')
    dst = dev.alloc(5 * 12 * 16, 'f64')
    xf = np.tile([1.0, 0.02, -0.02, 1.0, 0.3, -0.2], (5, 1))
    img, _, b = br.seam_scene()
    img = np.nan_to_num(img, nan=1.0)
    w, _ = br.taps(0.6)
    beads = _buffer(dev, np.stack([img] * 5), 'f64')
    offsets = [k * img.size for k in (3, 0, 4, 1, 2)]

    def warp():
        stats = dev.warp(src, 0, 5, 12, 16, xf, 3, None, dst, 0, 12, 16)
        return (dev.download(dst, 5 * 12 * 16), stats), ctx.chunks_run('warp')

    def find():
        out = device_peaks(dev, beads, offsets, img.shape[0], img.shape[1], w, 3, b, 0.2, 0.0, 64)
        return tuple(np.asarray(x) for one in out for x in one), ctx.chunks_run('beads')
    for which, run, old in (('warp', warp, lib.rl_warp_chunk_bytes), ('beads', find, lib.rl_find_peaks_chunk_bytes)):
        code, default = L.CHUNK_CAPS[which], L.CHUNK_DEFAULTS[which]
        try:
            whole, trips = run()
            assert trips == 1
            L.check(lib.rl_chunk_bytes(h, code, 1))
            for bad in ((h, code, 0), (h, 7, 1), (h, -1, 1), (None, code, 1)):
                assert lib.rl_chunk_bytes(*bad) == -1, bad
            got, trips = run()
            assert trips == 5, 'the cap of one byte must have survived the refused calls'
            _assert_same(got, whole, which)
            L.check(old(h, default))                        # the old setter undoes the new one's cap
            assert run()[1] == 1
            L.check(old(h, 1))                              # and the new one the old one's
            got, trips = run()
            assert trips == 5
            _assert_same(got, whole, which)
            assert old(h, 0) != 0 and run()[1] == 5
            L.check(lib.rl_chunk_bytes(h, code, default))
            assert run()[1] == 1
        finally:
            ctx.chunk_bytes(which, default)
    assert lib.rl_chunks_run(None, 0) == 0 and lib.rl_chunks_run(h, 7) == 0 and lib.rl_chunks_run(h, -1) == 0
    fresh = L.Context(0)
    try:
        assert [fresh.chunks_run(which) for which in L.CHUNK_CAPS] == [0] * 7
    finally:
        lib.rl_ctx_destroy(fresh.handle)
