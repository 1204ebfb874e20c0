"""The stencil kernels without a GPU: the workgroup bodies of rescan_line_sted_amd/csrc/sep_kernels.hpp (row pass, column pass with
four epilogues, the one-kernel form and its DIRECT variant at tile heights 32 and 64), their host side (sep_taps.hpp) and the box
normaliser (aux_kernels.hpp), emulated on the host (tests/emu/sep_emu.cpp: one OS thread per GPU thread, LDS of exactly the
launcher's byte count, poisoned with 0xff) and compared PER PIXEL with the plain long-double reference of tests/sep_reference.py.
Every tolerance is one of the derived bounds of that module's docstring or an existing project tolerance.  CPU only;
tools/asan_emu.sh runs this file under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sep_reference as sr
from conftest import fuzz_seeds, max_rel
from oracle import line_sted_oracle as orc
from sep_reference import LD, RATIO, STORE, SUM, UPDATE

F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def emu():
    e = sr.Emulator()
    yield e
    print()
    for line in sr.WORST.lines():
        print(line)


def tname(dtype):
    return 'f32' if np.dtype(dtype) == F32 else 'f64'


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('ny,nx,py,px', [(20, 23, 5, 7), (20, 23, 4, 6), (9, 31, 1, 1), (17, 12, 1, 8), (12, 17, 6, 1),
                                         (5, 6, 9, 11), (3, 40, 8, 3), (1, 1, 4, 5)])
def test_reference_is_the_oracles_convolution(ny, nx, py, px):
    """The centre convention: the plain sums against oracle.Deconvolver.H / H_t (odd, even and 1-tap sizes, PSFs larger than the image)
    at 1e-13 normwise (the FFT oracle's own rounding; the plain sums are long double).  H_t uses the same, UNFLIPPED PSF as H."""
    rng = np.random.default_rng(ny * 100 + py)
    V = 2
    psfs = rng.random((V, py, px)) + 0.05
    x, y = rng.random((ny, nx)) * 30, rng.random((V, ny, nx)) + 0.5
    o = orc.Deconvolver([p[None] for p in psfs])
    views = sr.Views(True, p=psfs)
    c, _, _ = sr.forward_ref(x[None], views, F64)
    h = o.H(x[None])
    for v in range(V):
        assert max_rel(np.maximum(c[0, v], 0).astype(F64), h[v][0]) < 1e-13
    S, _ = sr.adjoint_ref(y[None], views, F64)
    n, _, _ = sr.norm_ref(views, ny, nx)
    assert max_rel(S[0].astype(F64), o.H_t([y[v][None] for v in range(V)], normalize=False)[0]) < 1e-13
    assert max_rel((S[0] / n).astype(F64), o.H_t([y[v][None] for v in range(V)])[0]) < 1e-13
    if py * px > 1 and not np.allclose(psfs[0], psfs[0][::-1, ::-1]):
        flipped = sr.Views(True, p=psfs[:, ::-1, ::-1])
        Sf, _ = sr.adjoint_ref(y[None], flipped, F64)
        if ny > 1 and nx > 1:
            assert max_rel(Sf[0].astype(F64), o.H_t([y[v][None] for v in range(V)], normalize=False)[0]) > 1e-3      # a flipped PSF is another operation
    u, w = rng.random(py) - 0.3, rng.random(px) - 0.3
    s2, A2 = sr.conv_same(x, np.outer(u.astype(LD), w.astype(LD)))
    s1, A1 = sr.conv_same_rank1(x, u, w)
    assert np.max(np.abs(s1 - s2)) <= 1e-17 * np.max(A2) and np.max(np.abs(A1 - A2)) <= 1e-17 * np.max(A2)


# ------------------------------------------------------------------------------------------------ one case through all four epilogues
def run_case(emu, c, what=(STORE, RATIO, SUM, UPDATE)):
    """Case c (geometry + data) through the emulator, every epilogue against the reference per pixel.  Besides the bounds: no nan
    (a poisoned LDS byte that reached an output), guard bands of every destination intact, every output written, UPDATE confined to
    the frames it was launched on."""
    T, V, F, ny, nx = c.dtype, c.V, c.frames, c.ny, c.nx
    key = (c.form, tname(T), 'th%d' % c.th)
    tab = emu.tables(c.views, T)
    nonneg = not c.signed
    if STORE in what or RATIO in what:
        conv, e, A = sr.forward_ref(c.x, c.views, T)
    if STORE in what:
        dst, buf = sr.guarded((F, V, ny, nx), T)
        assert emu.run(c.form, c.th, STORE, c.x, tab, c.views, dst, F, ny, nx) == 0
        assert sr.guards_intact(buf), ('STORE wrote outside its images', c)
        sr.check_store(dst, conv, e, key, c)
        if nonneg:
            assert np.all(dst[A == 0] == 0)
    if RATIO in what:
        dst, buf = sr.guarded((F, V, ny, nx), T)
        assert emu.run(c.form, c.th, RATIO, c.x, tab, c.views, dst, F, ny, nx, aux=c.aux) == 0
        assert sr.guards_intact(buf), ('RATIO wrote outside its images', c)
        left_out = sr.check_ratio(dst, c.aux, conv, e, A, T, key, c)
        assert left_out <= (sr.MAX_EXCLUDED if c.signed else 0.0), (left_out, c)
    if SUM in what or UPDATE in what:
        cv, ev, _ = sr.forward_views_ref(c.y, c.views, T)
        S = np.maximum(cv, 0).sum(axis=1)
        E = sr.sum_bound(S, ev.sum(axis=1), V, T)
        ysrc = c.y.reshape(F * V, ny, nx)
    if SUM in what:
        for norm in (None, c.norm):
            dst, buf = sr.guarded((F, ny, nx), T)
            assert emu.run(c.form, c.th, SUM, ysrc, tab, c.views, dst, F, ny, nx, norm=norm) == 0
            assert sr.guards_intact(buf), ('SUM wrote outside its images', c)
            sr.check_sum(dst, S, E, norm, T, key, c)
    if UPDATE in what:
        # launched on frames [f0, F) only, as the plan's slices do: the frames before f0 must keep their bits
        f0 = c.seed % F
        dst, buf = sr.guarded((F, ny, nx), T, fill=c.est0)
        assert emu.run(c.form, c.th, UPDATE, ysrc[f0 * V:], tab, c.views, dst[f0:], F - f0, ny, nx, norm=c.norm) == 0
        assert sr.guards_intact(buf), ('UPDATE wrote outside its images', c)
        assert np.array_equal(dst[:f0], c.est0[:f0]), ('UPDATE touched a frame it was not launched on', c)
        sr.check_update(dst[f0:], c.est0[f0:], S[f0:], E[f0:], c.norm, T, key, c)


@pytest.mark.parametrize('seed', fuzz_seeds(36))
def test_random_stencil_cases_per_pixel(emu, seed):
    """Form {two-pass, one-kernel, DIRECT} x type x tile height {32, 64 (float)} x ny, nx from 1 up past two tiles in each direction x
    taps from 1 x 1 up to the largest the form's size rule accepts (a quarter of the seeds large) x V 1-4 x frames 1-3 x dense / 90 %
    sparse objects x non-negative / signed taps; all four epilogues (SUM with and without norm) against the long-double reference, per
    pixel, within the derived bounds of sep_reference's docstring.  The signed generator (taps random - 0.35, object 50 * random) must
    keep the share of pixels within their bound of the clamp's kink under 0.1 % (asserted for RATIO; STORE, SUM and UPDATE need no
    pixel left out: the clamp is 1-Lipschitz)."""
    c = sr.draw_data(sr.draw_geometry(seed, emu.fits_for))
    print(c)
    run_case(emu, c)


# ------------------------------------------------------------------------------------------------ the fixed edge table
def fixed_case(form, dtype, th, ny, nx, py, px, V=2, frames=1, seed=1, signed=False, sparse=False):
    c = sr.Case()
    c.form, c.dtype, c.th, c.ny, c.nx, c.py, c.px, c.V, c.frames = form, dtype, th, ny, nx, py, px, V, frames
    c.seed, c.signed, c.sparse, c.large = seed, signed, sparse, False
    return sr.draw_data(c)


# every template choice: the two-pass form has one tile height, the one-kernel forms run 64 in float only
COMBOS = [(form, dtype, th) for form in sr.FORMS for dtype, th in ((F32, 32), (F32, 64), (F64, 32)) if not (form == 'two' and th == 64)]

EDGE_SHAPES = [   # ny, nx, py, px
    (1, 1, 1, 1), (1, 1, 7, 9), (1, 70, 3, 8), (40, 1, 8, 3),                      # 1 x 1 image; 1-pixel rows and columns
    (31, 63, 7, 7), (32, 64, 8, 8), (33, 65, 9, 9), (63, 255, 2, 16), (64, 256, 16, 2), (65, 257, 17, 17),     # tile edges
    (5, 4, 16, 17), (3, 90, 17, 2), (70, 3, 1, 16),                                # PSF taller / wider than the image
    (20, 30, 2, 2), (20, 30, 8, 2), (21, 29, 6, 4),                                # even taps: the (p - 1) // 2 centre (random taps: asymmetric)
]


@pytest.mark.parametrize('form,dtype,th', COMBOS)
def test_edge_table(emu, form, dtype, th):
    """Image sizes on either side of every tile edge (row segment 256, tile 64 wide, 32 or 64 tall), tap counts on either side of
    the padding to multiples of 8, images smaller than the PSF, even asymmetric taps."""
    for i, (ny, nx, py, px) in enumerate(EDGE_SHAPES):
        run_case(emu, fixed_case(form, dtype, th, ny, nx, py, px, V=1 + i % 3, frames=1 + i % 2, seed=100 + i))


def limits(emu, form, esize, th, V):
    """(largest py beside px = 1, largest px beside py = 1, largest square) the form's size rule accepts."""
    fits = emu.fits_for(form, esize, th, V)
    return tuple(sr.largest_taps(f, limit=20000) for f in (lambda n: fits(n, 1), lambda n: fits(1, n), lambda n: fits(n, n)))


@pytest.mark.parametrize('form,dtype,th', COMBOS)
def test_largest_taps_each_size_rule_accepts(emu, form, dtype, th):
    """The largest py / px (and square) each *_fits rule accepts per type and tile height, one workgroup each, through STORE and
    SUM; one tap beyond, the rule says no and the launcher refuses.  The rule must also be what bounds the LDS: the byte count at the
    limit is within the 160 KB (64 KB for the row pass's default limit), beyond it is not."""
    es, V = np.dtype(dtype).itemsize, 2
    top_y, top_x, top_sq = limits(emu, form, es, th, V)
    print(form, tname(dtype), th, 'largest py %d, px %d, square %d' % (top_y, top_x, top_sq))
    lib = emu.lib
    if form == 'two':
        assert (top_y, top_x) == ((609, 16129) if dtype == F32 else (289, 7937))       # sep_kernels.hpp: "py up to 609 taps in f32, 289 in f64"
        assert lib.emu_sep_cols_lds(es, top_y) <= 160 * 1024 < lib.emu_sep_cols_lds(es, top_y + 1)
        assert lib.emu_sep_rows_lds(es, top_x) <= 65536 < lib.emu_sep_rows_lds(es, top_x + 1)
        shapes = [(top_y, 1), (1, top_x), (top_y, 9)]
    else:
        d = 1 if form == 'direct' else 0
        for py, px in ((top_y, 1), (1, top_x), (top_sq, top_sq)):
            assert lib.emu_sep2d_lds(es, th, py, px, V, d) <= lib.emu_sep_max_lds()
        assert lib.emu_sep2d_lds(es, th, top_y + 1, 1, V, d) > lib.emu_sep_max_lds() and lib.emu_sep2d_lds(es, th, 1, top_x + 1, V, d) > lib.emu_sep_max_lds()
        shapes = [(top_y, 1), (1, top_x), (top_sq, top_sq)]
    for i, (py, px) in enumerate(shapes):
        c = fixed_case(form, dtype, th, min(th, 24), 40, py, px, V=V, seed=300 + i)
        run_case(emu, c, what=(STORE, SUM))
    # one tap beyond: refused, nothing written
    for py, px in ((top_y + 1, 1),) + (((1, top_x + 1),) if form != 'two' else ()):
        assert not emu.fits(form, es, th, V, py, px)
        c = fixed_case(form, dtype, th, 8, 8, 1, 1, V=V)
        c.py, c.px = py, px
        c.views = sr.Views(form == 'direct', u=np.ones((V, py), dtype), v=np.ones((V, px), dtype), p=np.ones((V, py, px), dtype))
        dst, buf = sr.guarded((1, V, 8, 8), dtype)
        assert emu.run(form, th, STORE, c.x, emu.tables(c.views, dtype), c.views, dst, 1, 8, 8) == -1
        assert np.all(buf == buf.dtype.type(sr.CANARY))


@pytest.mark.parametrize('form,dtype,th', COMBOS)
def test_each_view_is_clamped_before_the_view_sum(emu, form, dtype, th):
    """SUM and UPDATE clamp every view's convolution at 0 BEFORE the views are added (ref:587).  Two views whose convolutions are
    negative over a whole region (all taps of view 1 negative; view 2 negative taps on one side): clamping the sum instead would be
    wrong by the size of the negative view there, thousands of bounds."""
    c = fixed_case(form, dtype, th, 45, 80, 5, 6, V=3, frames=2, seed=7)
    rng = np.random.default_rng(5)
    if form == 'direct':
        p = rng.random((3, 5, 6)) + 0.2
        p[1] = -p[1]                              # a view that is negative everywhere
        p[2, :, :3] = -p[2, :, :3]                # a view of mixed sign
        c.views = sr.Views(True, p=p.astype(dtype))
    else:
        u, v = rng.random((3, 5)) + 0.2, rng.random((3, 6)) + 0.2
        u[1] = -u[1]
        v[2, :3] = -v[2, :3]
        c.views = sr.Views(False, u=u.astype(dtype), v=v.astype(dtype))
    c.signed = True
    cv, _, _ = sr.forward_views_ref(c.y, c.views, dtype)
    assert np.all(cv[:, 1] < 0)                                                  # the case is what it says
    assert np.max(np.abs(np.maximum(cv.sum(axis=1), 0) - np.maximum(cv, 0).sum(axis=1))) > 1.0
    run_case(emu, c, what=(STORE, SUM, UPDATE))


def test_exactly_dark_regions_give_the_neutral_ratio(emu):
    """An object that is zero beyond the PSF's reach: the prediction there is exactly 0 and the ratio exactly 1, every form and type."""
    for form in sr.FORMS:
        for dtype, th in ((F32, 32), (F32, 64), (F64, 32)):
            if form == 'two' and th == 64:
                continue
            c = fixed_case(form, dtype, th, 70, 100, 7, 5, V=2, frames=1, seed=11)
            c.x[...] = 0
            c.x[0, 30:34, 40:45] = 3.5
            _, _, A = sr.forward_ref(c.x, c.views, dtype)
            assert np.mean(A == 0) > 0.9
            run_case(emu, c, what=(STORE, RATIO))


# ------------------------------------------------------------------------------------------------ the chain as the plan runs it
def emu_chain(emu, form, th, views, meas, dtype, iterations, step=None):
    """deconv_build's normaliser (SUM of ones) and sep_iterate (RATIO, then UPDATE) `iterations` times on meas [F][V][ny][nx], image
    order [frame * V + view], in_div as rlsted.cpp passes it.  step(name, out, inputs...) sees every kernel's output."""
    F, V, ny, nx = meas.shape
    tab = emu.tables(views, dtype)
    ones = np.ones((V, ny, nx), dtype)
    norm, nbuf = sr.guarded((1, ny, nx), dtype)
    assert emu.run(form, th, SUM, ones, tab, views, norm, 1, ny, nx) == 0 and sr.guards_intact(nbuf)
    norm = norm[0]
    if step:
        step('norm', norm, ones[None])
    est, ebuf = sr.guarded((F, ny, nx), dtype, fill=1.0)
    ratio, rbuf = sr.guarded((F, V, ny, nx), dtype)
    m = np.ascontiguousarray(meas.astype(dtype))
    for it in range(iterations):
        before = est.copy()
        assert emu.run(form, th, RATIO, est, tab, views, ratio, F, ny, nx, aux=m) == 0
        if step:
            step('ratio', ratio, before, m)
        assert emu.run(form, th, UPDATE, ratio.reshape(F * V, ny, nx), tab, views, est, F, ny, nx, norm=norm) == 0
        if step:
            step('update', est, before, ratio, norm)
        assert sr.guards_intact(ebuf) and sr.guards_intact(rbuf)
    return est.copy(), norm


@pytest.mark.parametrize('form', sr.FORMS)
def test_chain_of_three_iterations(emu, form):
    """Normaliser through SUM of ones, then RATIO / UPDATE three times.  f64 against oracle.Deconvolver at the project's 1e-11
    normwise.  f32 STEP BY STEP: each kernel's output against the long-double reference applied to the emulator's own previous
    outputs (every assertion a one-step derived bound; how an iteration amplifies earlier rounding is a property of the data, not
    of the kernel); the end result within the project's f32 contract of 1e-5 normwise from the f64 chain."""
    rng = np.random.default_rng(21)
    F, V, ny, nx, py, px = 2, 3, 50, 90, 6, 9
    if form == 'direct':
        views64 = sr.Views(True, p=(rng.random((V, py, px)) + 0.05).astype(F32).astype(F64))
    else:
        views64 = sr.Views(False, u=(rng.random((V, py)) + 0.05).astype(F32).astype(F64), v=(rng.random((V, px)) + 0.05).astype(F32).astype(F64))
    obj = (rng.random((F, ny, nx)) * 30).astype(F32).astype(F64)
    c, _, _ = sr.forward_ref(obj, views64, F64)
    meas = rng.poisson(np.maximum(c, 0).astype(F64)).astype(F64) + 0.5            # float-representable: both types see the same data
    est64, _ = emu_chain(emu, form, 32, views64, meas, F64, 3)
    for f in range(F):
        d = orc.Deconvolver([views64.psf(v)[None] for v in range(V)])
        d.create_data_from_object(obj[f][None], noisy_measurement=[meas[f, v][None] for v in range(V)])
        for _ in range(3):
            d.iterate()
        assert max_rel(est64[f], d.estimate[0]) < 1e-11
    for th in (32, 64):
        if form == 'two' and th == 64:
            continue
        views32 = sr.Views(views64.direct, u=None if views64.direct else views64.u.astype(F32), v=None if views64.direct else views64.v.astype(F32),
                           p=views64.p.astype(F32) if views64.direct else None)
        key = (form, 'f32', 'th%d' % th, 'chain')
        state = {}

        def step(name, out, *inp):
            if name == 'norm':
                cv, ev, _ = sr.forward_views_ref(inp[0], views32, F32)
                S = np.maximum(cv, 0).sum(axis=1)
                sr.check_sum(out[None], S, sr.sum_bound(S, ev.sum(axis=1), V, F32), None, F32, key)
            elif name == 'ratio':
                cc, e, A = sr.forward_ref(inp[0], views32, F32)
                assert sr.check_ratio(out, inp[1], cc, e, A, F32, key) == 0.0
            else:
                cv, ev, _ = sr.forward_views_ref(inp[1], views32, F32)
                S = np.maximum(cv, 0).sum(axis=1)
                sr.check_update(out, inp[0], S, sr.sum_bound(S, ev.sum(axis=1), V, F32), inp[2], F32, key)
            state[name] = state.get(name, 0) + 1
        est32, _ = emu_chain(emu, form, th, views32, meas, F32, 3, step=step)
        assert state == {'norm': 1, 'ratio': 3, 'update': 3}
        assert max_rel(est32, est64) < 1e-5                                       # BASELINE f32 contract


# ------------------------------------------------------------------------------------------------ the host side
@pytest.mark.parametrize('seed', fuzz_seeds(20))
def test_random_rank1_factors_and_tap_tables(emu, seed):
    """Outer products of random vectors (zeros inside, the maximum anywhere, negative entries) are accepted and the factors reproduce
    the PSF, element by element, within 4 ulp of the element; a perturbation of one tap by 1e-10 of the
    maximum and an all-zero view are rejected (the threshold is 1e-12 of the maximum).  The flipped tables: f[k] = taps[n - 1 - k],
    F[l][k] = p[py-1-k][px-1-l], zero in the padding."""
    rng = np.random.default_rng(400 + seed)
    V, py, px = int(rng.integers(1, 5)), int(rng.integers(1, 40)), int(rng.integers(1, 40))
    u, v = rng.random((V, py)) - 0.3, rng.random((V, px)) - 0.3
    u[rng.random((V, py)) < 0.2] = 0.0
    v[rng.random((V, px)) < 0.2] = 0.0
    for w in range(V):                                     # no view may be all zero
        u[w, rng.integers(0, py)] = 1.0 + rng.random()
        v[w, rng.integers(0, px)] = -1.0 - rng.random()
    psfs = np.stack([np.outer(u[w], v[w]) for w in range(V)])
    ok, fu, fv = emu.rank1(psfs)
    assert ok
    back = np.stack([np.outer(fu[w].astype(LD), fv[w].astype(LD)) for w in range(V)])
    assert np.all(np.abs(back - psfs) <= 4 * np.spacing(np.abs(psfs)))
    if py * px > 1:
        bad = psfs.copy()
        w, a, b = int(rng.integers(0, V)), int(rng.integers(0, py)), int(rng.integers(0, px))
        bad[w, a, b] += 1e-10 * np.abs(psfs[w]).max()
        if py > 1 and px > 1:
            assert not emu.rank1(bad)[0]
    zero = psfs.copy()
    zero[V - 1] = 0.0
    assert not emu.rank1(zero)[0]
    uf, vf = emu.flipped_taps(fu, fv)
    assert uf.shape == (V, (py + 7) // 8 * 8) and vf.shape == (V, (px + 7) // 8 * 8)
    assert np.array_equal(uf[:, :py], fu[:, ::-1]) and np.all(uf[:, py:] == 0)
    assert np.array_equal(vf[:, :px], fv[:, ::-1]) and np.all(vf[:, px:] == 0)
    f = emu.direct_taps(psfs)
    assert f.shape == (V, px, (py + 7) // 8 * 8)
    for l in range(px):
        for k in range(py):
            assert np.array_equal(f[:, l, k], psfs[:, py - 1 - k, px - 1 - l])
    assert np.all(f[:, :, py:] == 0)


def test_rank1_rejects_full_rank_and_accepts_lines(emu):
    g = np.exp(-np.linspace(-2, 2, 9) ** 2)
    assert emu.rank1(np.outer(g, g)[None])[0]
    assert not emu.rank1((np.outer(g, g) + np.eye(9) * 0.01)[None])[0]
    assert emu.rank1(np.array([[[1, 2, 3, 4, 3, 2, 1.0]]]))[0]
    assert not emu.rank1(np.stack([np.outer(g, g), np.outer(g, g) + np.eye(9) * 1e-9]))[0]      # every view must be


# ------------------------------------------------------------------------------------------------ the box normaliser
BOX_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 4), (1, 40, 3, 3), (40, 1, 6, 2), (30, 50, 7, 9), (30, 50, 8, 6), (4, 5, 9, 11), (3, 60, 12, 2),
              (64, 257, 17, 17), (9, 300, 2, 16)]


@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('dtype', [F32, F64])
def test_box_normaliser_per_pixel(emu, dtype, signed):
    """box_integral_images + box_norm_pixel against the reference's H_t(ones) per pixel.  Bound per view: every integral-image entry
    is a float64 sum of depth at most py + px (running row sum, then the entry above), four entries meet in three subtractions:
    4 * gamma_f64(py + px + 2) * (the view's absolute tap sum over the rectangle... bounded by the whole view's absolute tap sum);
    the view sum adds gamma_f64(V) * sum; one u of T on the value for the final conversion.  Images smaller and larger than the
    PSF, 1-pixel images, even sizes; signed taps with the interval form where a view's rectangle sum is within its bound of zero
    (the clamp is 1-Lipschitz: the bound on the sum holds as it stands)."""
    u64, uT = sr.unit(F64), sr.unit(dtype)
    for i, (ny, nx, py, px) in enumerate(BOX_SHAPES):
        rng = np.random.default_rng(50 + i)
        V = 1 + i % 4
        psfs = rng.random((V, py, px)) - (0.35 if signed else 0.0)
        out, integ = emu.box_norm(psfs, ny, nx, dtype)
        assert np.all(integ[:, 0, :] == 0) and np.all(integ[:, :, 0] == 0)
        cum = np.cumsum(np.cumsum(psfs.astype(LD), axis=1), axis=2)
        assert np.all(np.abs(integ[:, 1:, 1:] - cum) <= sr.gamma(py + px, u64) * np.cumsum(np.cumsum(np.abs(psfs).astype(LD), axis=1), axis=2))
        views = sr.Views(True, p=psfs)
        ref, _, _ = sr.norm_ref(views, ny, nx)
        tapsum = np.abs(psfs).astype(LD).sum(axis=(1, 2))
        b = (4 * sr.gamma(py + px + 2, u64) * tapsum).sum() + sr.gamma(V, u64) * ref
        b = b + uT * (ref + b) if dtype == F32 else b          # the conversion to T (none in f64)
        o = out.astype(LD)
        r = float(np.max(np.abs(o - ref) / b))
        sr.WORST.note(('box', tname(dtype), 'signed' if signed else 'nonneg'), r)
        assert not np.isnan(o).any() and r <= 1, (ny, nx, py, px, V, r)
        if not signed:
            assert np.all(o > 0)


# ------------------------------------------------------------------------------------------------ the device build of the same bodies
def test_stencil_kernels_do_not_spill(tmp_path):
    """The neighbour of test_host_logic.py::test_default_path_kernels_do_not_spill for the stencils: sep_kernels.hip and aux_kernels.hip
    compiled device-only with the flags of _build.py; all 34 stencil kernels (rows x 2 types, columns x 4 epilogues x 2, one-kernel
    4 epilogues x {separable, DIRECT} x {f64 32, f32 32, f32 64}) and k_box_norm have `.private_segment_fixed_size` 0."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')

    def scratch(name):
        out = str(tmp_path / (name + '.s'))
        subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE + ['--cuda-device-only', '-S', os.path.join(_build.CSRC, name + '.hip'), '-o', out],
                              stderr=subprocess.DEVNULL)
        txt = open(out).read()
        names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
        return dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    sep = scratch('sep_kernels')
    assert len(sep) == 34 and sum('k_sep_rows' in k for k in sep) == 2 and sum('k_sep_cols' in k for k in sep) == 8 and sum('k_sep2d' in k for k in sep) == 24
    assert all(v == 0 for v in sep.values()), {k: v for k, v in sep.items() if v}
    box = {k: v for k, v in scratch('aux_kernels').items() if 'k_box_norm' in k}
    assert len(box) == 2 and all(v == 0 for v in box.values())
