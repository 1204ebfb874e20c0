"""The separable strategy (sep_kernels.hip): plans whose views are all rank 1 and small run H / H_t as row +
column stencils.  Checked against the FFT strategy of the same library (RLSTED_SEP=0) and against the oracle;
the strategy choice itself is checked through rl_deconv_strategy."""
import numpy as np
import pytest

import sep_reference as sr
from conftest import max_rel, fuzz_seeds
from oracle import line_sted_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def plan_with(lib, sep, *args, one_kernel=True, **kw):
    """A plan created with RLSTED_SEP=sep (0 FFT, 1 automatic, 2 separable whenever rank 1); one_kernel=False
    keeps the two-pass form of the stencils (RLSTED_SEP_ONE=0), True asks for the one-kernel form whenever its tile fits LDS (=2)."""
    return lib.DeconvPlan(*args, options={'RLSTED_SEP': str(sep), 'RLSTED_SEP_ONE': '2' if one_kernel else '0'}, **kw)


def gauss(n, s, shift=0.0):
    x = np.arange(n) - (n - 1) / 2 - shift
    return np.exp(-x ** 2 / (2 * s ** 2))


def rank1_views(kind):
    if kind == 'row7':            # golden case G4's geometry: a 1 x 7 line
        return [np.array([[1, 2, 3, 4, 3, 2, 1.0]])]
    if kind == 'two_lines':       # 0 / 90 degree line PSFs: u v^T and its transpose
        u, v = gauss(17, 1.2), gauss(17, 4.0)
        return [np.outer(u, v), np.outer(v, u)]
    if kind == 'even_skew':       # even sizes, asymmetric taps: the centre convention (py-1)//2 matters
        return [np.outer(gauss(6, 1.5, 0.7), gauss(4, 1.0, -0.4)), np.outer(gauss(6, 0.8, -1.0), gauss(4, 2.0, 0.3))]
    raise KeyError(kind)


def planes(views):
    return [np.asarray(v)[None] for v in views]          # the reference's (1, py, px) PSF stacks


@pytest.mark.parametrize('one_kernel', [True, False])
@pytest.mark.parametrize('kind,shape', [('row7', (33, 70)), ('two_lines', (128, 128)), ('even_skew', (61, 300))])
def test_separable_matches_fft_strategy_and_oracle(lib, kind, shape, one_kernel):
    views = planes(rank1_views(kind))
    rng = np.random.default_rng(11)
    B, (ny, nx) = 3, shape
    obj = rng.random((B, ny, nx)) * 50
    sep = plan_with(lib, 2, views, B, ny, nx, dtype='f64', one_kernel=one_kernel)
    fft = plan_with(lib, 0, views, B, ny, nx, dtype='f64')
    assert sep.strategy()['separable'] and not fft.strategy()['separable']
    assert max_rel(sep.forward(obj), fft.forward(obj)) < 1e-12
    y = rng.random((B, len(views), ny, nx))
    for normalize in (True, False):
        assert max_rel(sep.adjoint(y, normalize), fft.adjoint(y, normalize)) < 1e-12
    for p in (sep, fft):
        p.set_object(obj, 1e7)
        p.simulate(seed=9)
    assert max_rel(sep.noiseless(), fft.noiseless()) < 1e-12
    assert np.array_equal(sep.measurement(), fft.measurement())      # ... and the same Poisson draws from it
    for p in (sep, fft):
        p.iterate(20)
    assert max_rel(sep.estimate(), fft.estimate()) < 1e-11
    for p in (sep, fft):                                             # continuing without a restart
        p.iterate(5)
    assert max_rel(sep.estimate(), fft.estimate()) < 1e-11
    o = orc.Deconvolver(views)
    o.create_data_from_object(obj[:1], noisy_measurement=[m[None] for m in sep.measurement()[0]])
    for _ in range(25):
        o.iterate()
    assert max_rel(sep.estimate()[0], o.estimate[0]) < 1e-10


def test_separable_f32_within_contract(lib):
    views = planes(rank1_views('two_lines'))
    rng = np.random.default_rng(12)
    obj = rng.random((2, 128, 128)) * 50
    p64 = plan_with(lib, 2, views, 2, 128, 128, dtype='f64')
    p32 = plan_with(lib, 2, views, 2, 128, 128, dtype='f32')
    assert p32.strategy()['separable']
    p64.set_object(obj, 1e7)
    p64.simulate(seed=2)
    p32.set_object(obj, 1e7)
    p32.set_measurement(p64.measurement())
    for p in (p64, p32):
        p.iterate(20)
    assert max_rel(p32.estimate(), p64.estimate()) < 1e-5       # BASELINE f32 contract


def test_strategy_choice(lib, golden):
    big = golden('g8_fig2_psfs')['2p0x_lr/line_sted_psfs'][::2, 0]        # 107 x 107, the 0 / 90 degree views: rank 1 but large
    assert not plan_with(lib, 1, planes(big), 1, 128, 128, dtype='f64').strategy()['separable']
    ref = plan_with(lib, 0, planes(big), 1, 128, 128, dtype='f64')
    x = np.random.default_rng(3).random((1, 128, 128))
    y = np.random.default_rng(4).random((1, 2, 128, 128))
    for one_kernel in (True, False):                                          # 107 taps: 120 KB of LDS in the one-kernel form
        forced = plan_with(lib, 2, planes(big), 1, 128, 128, dtype='f64', one_kernel=one_kernel)
        assert forced.strategy()['separable']
        assert max_rel(forced.forward(x), ref.forward(x)) < 1e-12
        assert max_rel(forced.adjoint(y), ref.adjoint(y)) < 1e-12
    rot = golden('g8_fig2_psfs')['2p0x_lr/line_sted_psfs'][:, 0]
    if len(rot) > 2:                                                          # a 45 degree view is not rank 1
        assert not plan_with(lib, 2, planes(rot), 1, 128, 128).strategy()['separable']
    small = planes([np.outer(gauss(7, 1.0), gauss(5, 2.0))])                 # automatic choice: rank 1 and py + px <= 16
    assert plan_with(lib, 1, small, 1, 64, 64).strategy()['separable']
    assert not plan_with(lib, 1, planes(rank1_views('two_lines')), 1, 64, 64).strategy()['separable']   # 17 + 17 taps: FFT is faster
    sp = plan_with(lib, 1, small, 1, 64, 64)
    sp.set_object(np.ones((1, 64, 64)), 1e6)
    sp.simulate(seed=1)
    with pytest.raises(lib.RlstedError):                                      # per-kernel timing is the FFT strategy's
        sp.time_kernels(2)
    blob = np.outer(gauss(9, 2), gauss(9, 2)) + np.eye(9) * 0.01             # small, full rank
    assert not plan_with(lib, 2, planes([blob]), 1, 64, 64).strategy()['separable']


@pytest.mark.parametrize('seed', fuzz_seeds(12))
def test_separable_random_small_cases_vs_oracle(lib, seed):
    """Automatic choice (py + px <= 16) on ragged shapes: images smaller than a tile, smaller than the PSF,
    1-pixel rows / columns, several views and frames -- H, H_t and three iterations against the oracle."""
    rng = np.random.default_rng(100 + seed)
    ny, nx = int(rng.integers(1, 71)), int(rng.integers(1, 140))
    py, px = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    V, B = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    views = planes([np.outer(rng.random(py) + 0.1, rng.random(px) + 0.1) for _ in range(V)])
    plan = lib.DeconvPlan(views, B, ny, nx, dtype='f64')
    assert plan.strategy()['separable']
    x = rng.random((B, ny, nx)) * 30
    o = orc.Deconvolver(views)
    h = plan.forward(x)
    for f in range(B):
        ref = o.H(x[f][None])
        errs = [max_rel(h[f, v], ref[v][0]) for v in range(V)]
        assert max(errs) < 1e-12, (ny, nx, py, px, V, B, errs)
    y = rng.random((B, V, ny, nx)) + 0.5
    ht = plan.adjoint(y, True)
    for f in range(B):
        assert max_rel(ht[f], o.H_t([y[f, v][None] for v in range(V)])[0]) < 1e-12
    plan.set_object(x)
    plan.set_measurement(y)
    plan.iterate(3)
    for f in range(B):
        d = orc.Deconvolver(views)
        d.create_data_from_object(x[f][None], noisy_measurement=[y[f, v][None] for v in range(V)])
        for _ in range(3):
            d.iterate()
        assert max_rel(plan.estimate()[f], d.estimate[0]) < 1e-11, (ny, nx, py, px, V, B)


@pytest.mark.parametrize('dtype,py,expect_sep', [('f64', 107, True), ('f32', 230, True), ('f64', 300, False)])
def test_long_column_stencils_raise_their_lds_limit_or_fall_back(lib, dtype, py, expect_sep):
    """the two-pass column stencil stages (32 + py - 1) x 64 values -- above the 64 KB default dynamic-LDS
    limit from py = 98 (f64) / 226 (f32) on, e.g. the 107-tap figure-2 line PSFs under RLSTED_SEP=2.  The kernel's limit is
    raised; where the tile would not fit the 160 KB of a compute unit the plan keeps the FFT strategy."""
    u, v = gauss(py, py / 8.0), gauss(9, 1.5)
    psf = [np.outer(u, v)[None] / np.outer(u, v).sum()]
    rng = np.random.default_rng(py)
    x = rng.random((2, 90, 70))
    sep = plan_with(lib, 2, psf, 2, 90, 70, one_kernel=False, dtype=dtype)
    assert sep.strategy()['separable'] == expect_sep
    fft = plan_with(lib, 0, psf, 2, 90, 70, dtype=dtype)
    assert not fft.strategy()['separable']
    assert max_rel(sep.forward(x), fft.forward(x)) < (1e-12 if dtype == 'f64' else 2e-6)
    d = orc.Deconvolver(psf)
    assert max_rel(sep.forward(x)[0, 0], d.H(x[:1])[0][0]) < (1e-12 if dtype == 'f64' else 2e-6)


# ------------------------------------------------------------------ the direct 2-D stencil (PSFs that are not rank 1)
def _direct_plan(lib, mode, psfs, B, ny, nx, dtype):
    return lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype, options={'RLSTED_DIRECT': str(mode)})


@pytest.mark.parametrize('py,px,V,shape', [(3, 5, 2, (40, 70)), (7, 7, 1, (128, 128)), (11, 9, 3, (61, 300)), (2, 6, 2, (33, 33)),
                                           (15, 13, 1, (200, 90)), (8, 4, 4, (17, 250))])
def test_direct_stencil_matches_fft_strategy_and_oracle(lib, py, px, V, shape):
    """PSFs that are small but not rank 1 run as a direct 2-D stencil (sep_kernels.hip k_sep2d DIRECT; the default up to 49 taps,
    RLSTED_DIRECT=2 beyond): H, H_t with and without the normaliser, the noiseless image, the Poisson draws from it and 25 RL
    iterations against the FFT strategy of the same library and against the oracle -- odd / even / two-row taps, 1-4 views, tiles
    that do not fill."""
    rng = np.random.default_rng(py * 100 + px)
    psfs = [rng.random((1, py, px)) + 0.05 for _ in range(V)]
    B, (ny, nx) = 2, shape
    obj = rng.random((B, ny, nx)) * 50
    d = _direct_plan(lib, 2, psfs, B, ny, nx, 'f64')
    fft = _direct_plan(lib, 0, psfs, B, ny, nx, 'f64')
    assert d.strategy()['direct_stencil'] and not d.strategy()['separable']
    assert not fft.strategy()['direct_stencil'] and not fft.strategy()['separable']
    if py * px <= 49:
        assert lib.DeconvPlan(psfs, B, ny, nx, dtype='f64').strategy()['direct_stencil']     # the default
    assert max_rel(d.forward(obj), fft.forward(obj)) < 1e-12
    y = rng.random((B, V, ny, nx))
    for normalize in (True, False):
        assert max_rel(d.adjoint(y, normalize), fft.adjoint(y, normalize)) < 1e-12
    for p in (d, fft):
        p.set_object(obj, 1e7)
        p.simulate(seed=9)
    assert max_rel(d.noiseless(), fft.noiseless()) < 1e-12
    assert np.array_equal(d.measurement(), fft.measurement())
    for p in (d, fft):
        p.iterate(25)
    assert max_rel(d.estimate(), fft.estimate()) < 1e-11
    o = orc.Deconvolver(psfs)
    o.create_data_from_object(obj[:1], noisy_measurement=[m[None] for m in d.measurement()[0]])
    for _ in range(25):
        o.iterate()
    assert max_rel(d.estimate()[0], o.estimate[0]) < 1e-10
    f32 = _direct_plan(lib, 2, psfs, B, ny, nx, 'f32')
    assert f32.strategy()['direct_stencil']
    f32.set_measurement(d.measurement())
    f32.iterate(25)
    assert max_rel(f32.estimate(), d.estimate()) < 1e-5


def test_direct_stencil_keeps_f32_plans_accurate_on_dark_backgrounds(lib):
    """What the direct stencil is for beyond speed: sparse emitters on a black background under a narrow, non-separable PSF
    (tests/test_gpu_parity.py::test_dark_background_narrow_psf_stays_finite).  The FFT path's f32 predictions of the dark region are
    rounding noise (finite, but 1e-5 ... 4e-5 of the maximum from the float64 plan, and counted by rl_deconv_unresolved); the
    stencil sums non-negative terms only, so every prediction keeps its relative accuracy: f32 within 3e-6 of float64."""
    rng = np.random.default_rng(77)
    ny = nx = 256
    obj = np.zeros((2, ny, nx))
    for b in range(2):
        obj[b, rng.integers(8, ny - 8, 30), rng.integers(8, nx - 8, 30)] = rng.random(30) + 0.5
    yy, xx = np.mgrid[-4:5, -4:5]
    u, w = 0.866 * xx + 0.5 * yy, -0.5 * xx + 0.866 * yy
    psf = [np.exp(-0.5 * ((u / 1.6) ** 2 + (w / 0.8) ** 2))[None]]
    p64 = _direct_plan(lib, 0, psf, 2, ny, nx, 'f64')
    p64.set_object(obj, 3e3)
    p64.simulate(seed=9)
    meas = p64.measurement()
    p64.iterate(12)
    ref = p64.estimate()
    err = {}
    for mode in (0, 2):
        p32 = _direct_plan(lib, mode, psf, 2, ny, nx, 'f32')
        assert p32.strategy()['direct_stencil'] == (mode == 2)
        p32.set_measurement(meas)
        p32.iterate(12)
        e = p32.estimate()
        assert np.isfinite(e).all() and e.min() >= 0
        err[mode] = max_rel(e, ref)
    print('f32 against float64, 12 iterations: FFT path %.2e, direct stencil %.2e' % (err[0], err[2]))
    assert err[2] < 3e-6 and err[2] < 0.3 * err[0]


# ------------------------------------------------------------------ per pixel, against the plain long-double reference (tests/sep_reference.py)
FORM_KNOBS = {'two': {'RLSTED_SEP': '2', 'RLSTED_SEP_ONE': '0'}, 'one': {'RLSTED_SEP': '2', 'RLSTED_SEP_ONE': '2'},
              'direct': {'RLSTED_SEP': '1', 'RLSTED_DIRECT': '2'}}


@pytest.fixture(scope='module')
def emu():
    e = sr.Emulator()
    yield e
    print()
    for line in sr.WORST.lines():
        print(line)


def forced_plan(lib, form, psfs, B, ny, nx, dtype, **more):
    """A plan made to run `form` of the stencils: RLSTED_SEP=2 with RLSTED_SEP_ONE=0 / 2, or RLSTED_DIRECT=2; more: further options."""
    plan = lib.DeconvPlan([p[None] for p in psfs], B, ny, nx, dtype=dtype, options=dict(FORM_KNOBS[form], **more))
    s = plan.strategy()
    assert (s['direct_stencil'] and not s['separable']) if form == 'direct' else s['separable'], (form, s)
    return plan


def plan_taps(c):
    """What a plan hands to a form: up to 128 taps a side here (the plan also builds its FFT strategy: lengths up to 4608); the direct
    stencil takes PSFs that are not rank 1 -- at least 2 x 2 -- of at most 1024 taps."""
    py, px = min(c.py, 128), min(c.px, 128)
    if c.form == 'direct':
        py, px = max(py, 2), max(px, 2)
        while py * px > 1024:
            py, px = (py // 2, px) if py >= px else (py, px // 2)
    return py, px


def plan_case(emu, seed, dtype):
    """Case `seed` of the CPU tests' generator at plan level: (case, the float64 PSFs the plan is given, the views as the plan uploads
    them in its element type).  Objects and taps are values of the element type, so the plan's upload conversion adds nothing; the
    rank-1 factors are the plan's own (sep_taps.hpp sep_rank1_factors, through the emulator library), converted as the upload converts."""
    T = np.float32 if dtype == 'f32' else np.float64
    c = sr.draw_data(sr.draw_geometry(seed, emu.fits_for, dtypes=(T,), allow_th64=False, max_taps=plan_taps))
    if c.form == 'direct':
        psfs = c.views.p.astype(np.float64)
        views = c.views
    else:
        psfs = np.stack([np.outer(c.views.u[w].astype(np.float64), c.views.v[w].astype(np.float64)) for w in range(c.V)])
        ok, fu, fv = emu.rank1(psfs)
        assert ok
        views = sr.Views(False, u=fu.astype(T), v=fv.astype(T))
    return c, psfs, views


def check_forward_and_adjoint(emu, plan, c, views, key):
    """forward / adjoint of `plan` on case c against the reference per pixel within the derived bounds, and against the emulator
    within twice the bound (both sides obey it).  NOT bit for bit, f64 STORE included: the device build contracts (every multiply-add
    of k_sep2d<double, STORE> is a v_fma_f64 in the ISA of HEAD), the emulator is built with -ffp-contract=off."""
    T, V, F, ny, nx = c.dtype, c.V, c.frames, c.ny, c.nx
    u = sr.unit(T)
    conv, e, A = sr.forward_ref(c.x, views, T)
    h = plan.forward(c.x)
    sr.check_store(h, conv, e, key, c)
    tab = emu.tables(views, T)
    dst, buf = sr.guarded((F, V, ny, nx), T)
    assert emu.run(c.form, 32, sr.STORE, c.x, tab, views, dst, F, ny, nx) == 0 and sr.guards_intact(buf)
    assert np.all(np.abs(h.astype(sr.LD) - dst.astype(sr.LD)) <= 2 * e), ('device against emulator, STORE', c)
    cv, ev, _ = sr.forward_views_ref(c.y, views, T)
    S = np.maximum(cv, 0).sum(axis=1)
    E = sr.sum_bound(S, ev.sum(axis=1), V, T)
    ht = plan.adjoint(c.y, False)
    sr.check_sum(ht, S, E, None, T, key, c)
    dst, buf = sr.guarded((F, ny, nx), T)
    assert emu.run(c.form, 32, sr.SUM, c.y.reshape(F * V, ny, nx), tab, views, dst, F, ny, nx) == 0 and sr.guards_intact(buf)
    assert np.all(np.abs(ht.astype(sr.LD) - dst.astype(sr.LD)) <= 2 * E), ('device against emulator, SUM', c)
    # with the normaliser (the plan's own: SUM of ones through the same stencil): its bound is added, S En / n^2
    n, cn, An = sr.norm_ref(views, ny, nx)
    En = sr.sum_bound(n, (sr.gamma(views.depth(), u) * An).sum(axis=0), V, T)
    sr.check_sum(plan.normalization()[None], n[None], En[None], None, T, key + ('normaliser',), c)
    ok = n > 2 * En
    # (signed taps: where every view's convolution of ones is negative beyond its bound the normaliser is exactly 0 in reference and
    # plan alike and the quotient is x / 0 in both -- nothing to bound; only pixels near the clamp's kink count against the cap)
    dead = np.all(cn < -sr.gamma(views.depth(), u) * An, axis=0)
    assert np.all(plan.normalization()[dead] == 0) and not (c.signed is False and dead.any())
    assert 1 - (ok | dead).mean() <= (sr.MAX_EXCLUDED if c.signed else 0.0), c
    ref = S[:, ok] / n[ok]
    b = E[:, ok] / n[ok] + S[:, ok] * En[ok] / n[ok] ** 2 + u * np.abs(ref)
    err = np.abs(plan.adjoint(c.y, True)[:, ok].astype(sr.LD) - ref)
    r = float(np.max(err[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0
    assert np.all(err[b == 0] == 0)
    sr.WORST.note(key + ('SUM/normaliser',), r)
    assert r <= 1, ('adjoint with the normaliser', c, r)


@pytest.mark.parametrize('seed', fuzz_seeds(24))
def test_random_forced_stencils_per_pixel_f64(lib, emu, seed):
    """The generator of tests/test_sep_cpu.py at plan level (two-pass, one-kernel, DIRECT by seed), float64: forward and adjoint with
    and without the normaliser per pixel within the derived bounds; three iterations against the oracle at 1e-11 normwise (cases
    with non-negative taps: Richardson-Lucy's domain)."""
    c, psfs, views = plan_case(emu, seed, 'f64')
    print(c)
    plan = forced_plan(lib, c.form, psfs, c.frames, c.ny, c.nx, 'f64')
    check_forward_and_adjoint(emu, plan, c, views, (c.form, 'f64', 'plan'))
    if not c.signed:
        plan.set_measurement(c.aux)
        plan.iterate(3)
        for f in range(c.frames):
            d = orc.Deconvolver([p[None] for p in psfs])
            d.create_data_from_object(np.ones((1, c.ny, c.nx)), noisy_measurement=[c.aux[f, v][None].astype(np.float64) for v in range(c.V)])
            for _ in range(3):
                d.iterate()
            assert max_rel(plan.estimate()[f], d.estimate[0]) < 1e-11, c


@pytest.mark.parametrize('seed', fuzz_seeds(24))
def test_random_forced_stencils_per_pixel_f32(lib, emu, seed):
    """... float32: the same per-pixel bounds with u = 2^-24 (a dark pixel as accurate as a bright one); three iterations within the
    f32 contract of 1e-5 normwise from the float64 plan of the same form."""
    c, psfs, views = plan_case(emu, seed, 'f32')
    print(c)
    plan = forced_plan(lib, c.form, psfs, c.frames, c.ny, c.nx, 'f32')
    check_forward_and_adjoint(emu, plan, c, views, (c.form, 'f32', 'plan'))
    if not c.signed:
        p64 = forced_plan(lib, c.form, psfs, c.frames, c.ny, c.nx, 'f64')
        for p in (plan, p64):
            p.set_measurement(c.aux)
            p.iterate(3)
        assert max_rel(plan.estimate(), p64.estimate()) < 1e-5, c


def _worst(out, ref, bound):
    """The largest error / bound of a pixel (inf: an error where the bound is 0)."""
    err = np.abs(np.asarray(out, dtype=sr.LD) - ref)
    if np.any(err[bound == 0] != 0):
        return float('inf')
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def test_tile_height_64_per_pixel_beside_the_default_height(lib, emu):
    """RLSTED_SEP_TH is a switch of the plan: f32 plans created with RLSTED_SEP_TH=64 run the one-kernel and DIRECT forms on cases of
    the shared generator -- the first ten that fit LDS at height 64 --, forward and adjoint against the long-double reference per
    pixel.  A plan of the same case at the default height, alive in the same process and called in between, stays within the same
    bounds: the two heights coexist."""
    rows = []
    for seed in range(40):
        if seed % 3 == 0:          # the two-pass form has one tile height
            continue
        c, psfs, views = plan_case(emu, seed, 'f32')
        if not emu.fits(c.form, 4, 64, c.V, views.py, views.px):
            continue
        tall = forced_plan(lib, c.form, psfs, c.frames, c.ny, c.nx, 'f32', RLSTED_SEP_TH='64')
        low = forced_plan(lib, c.form, psfs, c.frames, c.ny, c.nx, 'f32', RLSTED_SEP_TH='32')
        assert tall.options['RLSTED_SEP_TH'] == '64'
        conv, e, _ = sr.forward_ref(c.x, views, c.dtype)
        cv, ev, _ = sr.forward_views_ref(c.y, views, c.dtype)
        S = np.maximum(cv, 0).sum(axis=1)
        E = sr.sum_bound(S, ev.sum(axis=1), c.V, c.dtype)
        row = {'seed': seed, 'form': c.form, 'case': c}
        for name, plan in (('64', tall), ('32', low)):                 # (forward of both, then adjoint of both: the calls alternate)
            s = plan.strategy()
            assert s['separable'] or s['direct_stencil'], (name, c)     # every plan reports a stencil strategy
            row['h' + name] = plan.forward(c.x)
        for name, plan in (('64', tall), ('32', low)):
            row['ht' + name] = plan.adjoint(c.y, False)
        for name in ('64', '32'):
            h, ht = row.pop('h' + name), row.pop('ht' + name)
            assert not (np.isnan(h).any() or np.isnan(ht).any()), (name, c)
            row['forward' + name], row['adjoint' + name] = _worst(h, np.maximum(conv, 0), e), _worst(ht, S, E)
        print({k: v for k, v in row.items() if k != 'case'})
        rows.append(row)
        if len(rows) == 10:
            break
    assert {row['form'] for row in rows} == {'one', 'direct'} and len(rows) >= 8
    for row in rows:
        assert row['forward64'] <= 1 and row['adjoint64'] <= 1, row
        assert row['forward32'] <= 1 and row['adjoint32'] <= 1, row


def test_direct_stencil_dark_background_per_pixel(lib):
    """test_direct_stencil_keeps_f32_plans_accurate_on_dark_backgrounds per pixel, on `forward`: every pixel the PSF can reach from an
    emitter is within gamma(py * px + 2) RELATIVE of the reference (all terms are non-negative: A equals the value), every other pixel
    is exactly 0 -- which a normwise max_rel cannot see."""
    rng = np.random.default_rng(77)
    ny = nx = 256
    for dtype, T in (('f32', np.float32), ('f64', np.float64)):
        obj = np.zeros((2, ny, nx), T)
        for b in range(2):
            obj[b, rng.integers(8, ny - 8, 30), rng.integers(8, nx - 8, 30)] = (rng.random(30) + 0.5).astype(T)
        yy, xx = np.mgrid[-4:5, -4:5]
        u, w = 0.866 * xx + 0.5 * yy, -0.5 * xx + 0.866 * yy
        psf = np.exp(-0.5 * ((u / 1.6) ** 2 + (w / 0.8) ** 2)).astype(T)
        plan = _direct_plan(lib, 2, [psf[None].astype(np.float64)], 2, ny, nx, dtype)
        assert plan.strategy()['direct_stencil']
        views = sr.Views(True, p=psf[None])
        conv, e, A = sr.forward_ref(obj, views, T)
        h = plan.forward(obj)
        assert np.mean(A == 0) > 0.5 and np.all(h[A == 0] == 0)
        lit = A > 0
        rel = np.abs(h[lit].astype(sr.LD) - conv[lit]) / conv[lit]
        g = sr.gamma(9 * 9 + 2, sr.unit(T))
        print('%s: largest relative error of a lit pixel %.3g, bound %.3g; smallest lit value %.3g of the maximum' %
              (dtype, float(rel.max()), float(g), float(conv[lit].min() / conv.max())))
        assert rel.max() <= g
