"""The stencil operations of rescan_line_sted_amd/csrc/sep_kernels.hpp written down plainly, in numpy.longdouble and without any FFT,
the derived error bounds of the kernels' own arithmetic, the random case generator the CPU tests (tests/test_sep_cpu.py) and the GPU
tests (tests/test_gpu_separable.py) share, and the ctypes wrapper of the host emulator (tests/emu/sep_emu.cpp).

The operation (the reference's fftconvolve(x, p, 'same'), pinned against oracle.line_sted_oracle in tests/test_sep_cpu.py):

    out[i][j] = sum_{a,b} x[i + cy - a][j + cx - b] * p[a][b],   cy = (py - 1) // 2,  cx = (px - 1) // 2,  zero outside the image

H_t convolves with the SAME, unflipped PSF as H.  Each view's convolution is clamped at 0 before anything else is done with it.

Error bounds.  Inputs and taps are generated in the kernel's element type T and the reference is computed from those very values,
so the only error is the kernel's arithmetic.  u = 2^-24 (float) / 2^-53 (double), gamma(k) = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: a sum of k products in any order errs by at most gamma(k) * sum |terms|; fused
multiply-adds only remove roundings).  Per pixel, to first order in u:

    a view's convolution, separable forms   gamma(px + py + 2) * A     row pass (px products summed), store, column pass (py)
    a view's convolution, DIRECT            gamma(py * px + 2) * A     zero-padded taps add exact zeros; any summation order
        A = sum of the absolute values of the terms u_a v_b x (p_ab x)
    clamp at 0                              1-Lipschitz: the clamped value errs by no more than the unclamped one
    SUM over V views                        the views' bounds added, plus gamma(V) * sum
    a division, the UPDATE product          one more u each, relative (IEEE division on the host; the v_div_scale / v_div_fmas /
                                            v_div_fixup sequence on gfx950, correctly rounded in both types)

For non-negative data A equals the reference value: the bounds are pixelwise RELATIVE, a dark pixel must be as accurate as a bright one.
"""
import ctypes
import os
import subprocess

import numpy as np

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')

STORE, RATIO, SUM, UPDATE = 0, 1, 2, 3
FORMS = ('two', 'one', 'direct')                 # two-pass (k_sep_rows + k_sep_cols), one kernel (k_sep2d), k_sep2d DIRECT
MAX_EXCLUDED = 1e-3                              # share of a case's pixels that may sit within their bound of the clamp's kink


def unit(dtype):
    return LD(2.0) ** (-24 if np.dtype(dtype) == np.float32 else -53)


def gamma(k, u):
    return k * u / (1 - k * u)


# ------------------------------------------------------------------------------------------------ the plain operation
def conv_same(x, p):
    """x [ny][nx], p [py][px] -> (sum, sum of the terms' absolute values), both longdouble: the definition, term by term."""
    x, p = np.asarray(x, dtype=LD), np.asarray(p, dtype=LD)
    (ny, nx), (py, px) = x.shape, p.shape
    cy, cx = (py - 1) // 2, (px - 1) // 2
    pad = np.zeros((ny + py - 1, nx + px - 1), dtype=LD)
    pad[py - 1 - cy:py - 1 - cy + ny, px - 1 - cx:px - 1 - cx + nx] = x          # x[i + cy - a] = pad[i + py - 1 - a]
    s, A = np.zeros((ny, nx), dtype=LD), np.zeros((ny, nx), dtype=LD)
    for a in range(py):
        for b in range(px):
            if p[a, b] == 0:
                continue
            t = pad[py - 1 - a:py - 1 - a + ny, px - 1 - b:px - 1 - b + nx] * p[a, b]
            s += t
            A += np.abs(t)
    return s, A


def conv_same_rank1(x, u, v):
    """conv_same(x, outer(u, v)) as two 1-D passes (the same sum of the same terms in another order; long-double rounding apart):
    what the long taps of the two-pass form are checked against.  Pinned against conv_same in tests/test_sep_cpu.py."""
    x = np.asarray(x, dtype=LD)
    s1, _ = conv_same(x, np.asarray(v, dtype=LD)[None, :])
    a1, _ = conv_same(np.abs(x), np.abs(np.asarray(v, dtype=LD))[None, :])
    s, _ = conv_same(s1, np.asarray(u, dtype=LD)[:, None])
    A, _ = conv_same(a1, np.abs(np.asarray(u, dtype=LD))[:, None])
    return s, A


class Views:
    """The PSFs of a case as the kernels get them: rank-1 factors u [V][py], v [V][px] (separable forms) or p [V][py][px] (DIRECT),
    already in the element type."""

    def __init__(self, direct, u=None, v=None, p=None):
        self.direct, self.u, self.v, self.p = direct, u, v, p
        self.V = len(p) if direct else len(u)
        self.py, self.px = (p.shape[1:] if direct else (u.shape[1], v.shape[1]))

    def conv(self, x, view):
        if self.direct:
            return conv_same(x, self.p[view])
        if self.py * self.px > 400:
            return conv_same_rank1(x, self.u[view], self.v[view])
        return conv_same(x, np.outer(self.u[view].astype(LD), self.v[view].astype(LD)))

    def depth(self):                       # k of gamma(k) for one view's convolution
        return self.py * self.px + 2 if self.direct else self.py + self.px + 2

    def psf(self, view):                   # float64 [py][px] (for the oracle and the box normaliser: not exact for rank-1 factors)
        return np.asarray(self.p[view], dtype=np.float64) if self.direct else np.outer(self.u[view].astype(np.float64), self.v[view].astype(np.float64))


def forward_ref(x, views, dtype):
    """H of frames x [F][ny][nx]: (conv [F][V][ny][nx] unclamped, bound e, A), longdouble."""
    g = gamma(views.depth(), unit(dtype))
    c = np.zeros((len(x), views.V) + x.shape[1:], dtype=LD)
    A = np.zeros_like(c)
    for f in range(len(x)):
        for w in range(views.V):
            c[f, w], A[f, w] = views.conv(x[f], w)
    return c, g * A, A


def adjoint_ref(y, views, dtype):
    """H_t of y [F][V][ny][nx] without the normaliser: (sum_v max(conv_v, 0) [F][ny][nx], its bound)."""
    u = unit(dtype)
    c, e, _ = forward_views_ref(y, views, dtype)
    S = np.maximum(c, 0).sum(axis=1)
    return S, e.sum(axis=1) + gamma(views.V, u) * S


def forward_views_ref(y, views, dtype):
    """view w of frame f convolved with PSF w (the inputs of SUM / UPDATE): conv [F][V][ny][nx], bound, A."""
    g = gamma(views.depth(), unit(dtype))
    c = np.zeros(y.shape, dtype=LD)
    A = np.zeros_like(c)
    for f in range(y.shape[0]):
        for w in range(views.V):
            c[f, w], A[f, w] = views.conv(y[f, w], w)
    return c, g * A, A


def norm_ref(views, ny, nx):
    """H_t(ones): sum_v max(conv(1, p_v), 0), and sum_v conv(1, |p_v|) (the absolute tap sums the normaliser's bound scales with)."""
    ones = np.ones((1, views.V, ny, nx))
    c, _, A = forward_views_ref(ones, views, np.float64)
    return np.maximum(c, 0).sum(axis=1)[0], c[0], A[0]


# ------------------------------------------------------------------------------------------------ assertions with derived bounds
class Worst:
    """The worst observed error / bound per key (form, type, epilogue), printed by the tests."""

    def __init__(self):
        self.r = {}

    def note(self, key, ratio):
        self.r[key] = max(self.r.get(key, 0.0), float(ratio))

    def lines(self):
        return ['worst error / bound  %-28s %.3f' % (' '.join(str(k) for k in key), v) for key, v in sorted(self.r.items())]


WORST = Worst()


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    exact = bound == 0
    assert not np.any(err[exact] != 0), 'a pixel whose every term is zero is not exact'
    return float(np.max(err[~exact] / bound[~exact])) if np.any(~exact) else 0.0


def check_store(out, c, e, key, ctx=''):
    """STORE: max(c - e, 0) <= out <= max(c + e, 0) (the clamp is monotone: valid with taps of either sign)."""
    o = np.asarray(out, dtype=LD)
    assert not np.isnan(o).any(), ('nan in STORE', key, ctx)
    r = _ratio(np.abs(o - np.maximum(c, 0)), e)
    WORST.note(key + ('STORE',), r)
    bad = (o < np.maximum(c - e, 0)) | (o > np.maximum(c + e, 0))
    assert not bad.any(), ('STORE', key, ctx, 'error / bound %.3f' % r, np.argwhere(bad)[:4])


def check_ratio(out, aux, c, e, A, dtype, key, ctx=''):
    """RATIO: aux / c within (e / c + u) relative where c > e; exactly 1 where every term is zero (A == 0) or c < -e; the pixels
    with |c| <= e (the clamp may legitimately go either way) are left out and counted.  Returns the share left out."""
    u = unit(dtype)
    o = np.asarray(out, dtype=LD)
    assert not np.isnan(o).any(), ('nan in RATIO', key, ctx)
    dark = (A == 0) | (c < -e)
    assert np.all(o[dark] == 1), ('RATIO: a prediction of exactly zero must give the neutral ratio', key, ctx)
    lit = (c > e) & ~dark
    ref = np.asarray(aux, dtype=LD)[lit] / c[lit]
    b = np.abs(ref) * (e[lit] / c[lit] + u)
    r = _ratio(np.abs(o[lit] - ref), b)
    WORST.note(key + ('RATIO',), r)
    assert r <= 1, ('RATIO', key, ctx, 'error / bound %.3f' % r)
    return 1.0 - (dark.sum() + lit.sum()) / o.size


def sum_bound(S, e_views, V, dtype):
    return e_views + gamma(V, unit(dtype)) * S


def check_sum(out, S, E, norm, dtype, key, ctx=''):
    """SUM: S within E; with a normaliser S / norm within E / norm + u |S / norm|."""
    u = unit(dtype)
    o = np.asarray(out, dtype=LD)
    assert not np.isnan(o).any(), ('nan in SUM', key, ctx)
    if norm is None:
        ref, b = S, E
    else:
        n = np.asarray(norm, dtype=LD)
        ref = S / n
        b = E / n + u * np.abs(ref)
    r = _ratio(np.abs(o - ref), b)
    WORST.note(key + ('SUM' if norm is None else 'SUM/norm',), r)
    assert r <= 1, ('SUM', key, ctx, 'error / bound %.3f' % r)


def check_update(out, est0, S, E, norm, dtype, key, ctx=''):
    """UPDATE: est0 * (S / norm): the quotient's bound times |est0|, one more u for the product."""
    u = unit(dtype)
    o, d0, n = np.asarray(out, dtype=LD), np.asarray(est0, dtype=LD), np.asarray(norm, dtype=LD)
    assert not np.isnan(o).any(), ('nan in UPDATE', key, ctx)
    q = S / n
    ref = d0 * q
    b = np.abs(d0) * (E / n + u * np.abs(q)) + u * np.abs(ref)
    r = _ratio(np.abs(o - ref), b)
    WORST.note(key + ('UPDATE',), r)
    assert r <= 1, ('UPDATE', key, ctx, 'error / bound %.3f' % r)


# ------------------------------------------------------------------------------------------------ the random case generator
class Case:
    def __repr__(self):
        return 'Case(%s)' % ', '.join('%s=%r' % kv for kv in sorted(self.__dict__.items()) if not isinstance(kv[1], np.ndarray) and kv[0] != 'views')


def largest_taps(fits, start=1, limit=4096):
    """The largest n in [start, limit] with fits(n), fits being monotone (an LDS size rule), or start - 1."""
    n = start - 1
    while n < limit and fits(n + 1):
        n += 1
    return n


def draw_geometry(seed, fits_for, forms=FORMS, dtypes=(np.float32, np.float64), allow_th64=True, max_taps=None):
    """Geometry of random case `seed`: form x type x tile height {32, 64 (float)} x ny, nx from 1 up past two tiles x taps from 1 x 1
    up to the largest the form's size rule accepts (a quarter of the seeds large) x V 1-4 x frames 1-3 x dense / 90 % sparse x
    non-negative / signed taps.  fits_for(form, esize, th, V) -> fits(py, px)."""
    rng = np.random.default_rng(7000 + seed)
    c = Case()
    c.seed = seed
    c.form = forms[seed % len(forms)]
    c.dtype = dtypes[(seed // len(forms)) % len(dtypes)]
    c.th = 64 if (allow_th64 and c.dtype == np.float32 and c.form != 'two' and rng.random() < 0.5) else 32
    c.V, c.frames = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    c.sparse, c.signed = bool(rng.random() < 0.5), bool(rng.random() < 0.25)
    c.large = bool(rng.random() < 0.25)
    c.ny = int(rng.integers(1, 2 * c.th + 8))
    c.nx = int(rng.integers(1, 530)) if (c.form == 'two' and rng.random() < 0.2) else int(rng.integers(1, 150))
    fits = fits_for(c.form, np.dtype(c.dtype).itemsize, c.th, c.V)
    if c.large:
        # one side up to the rule's limit beside a short other side, or both sides up to the largest square the rule accepts
        kind = int(rng.integers(0, 3))
        if kind == 2:
            top = largest_taps(lambda n: fits(n, n))
            c.py, c.px = int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))
        else:
            short = int(rng.integers(1, 9))
            top = largest_taps((lambda n: fits(n, short)) if kind == 0 else (lambda n: fits(short, n)))
            long_ = int(rng.integers(max(1, top // 2), top + 1))
            c.py, c.px = (long_, short) if kind == 0 else (short, long_)
    else:
        c.py, c.px = int(rng.integers(1, 18)), int(rng.integers(1, 18))
    if max_taps is not None:                       # (plan-level callers: the plan's own limits on what it hands to a form)
        c.py, c.px = max_taps(c)
    assert fits(c.py, c.px), c
    return c


def draw_data(c):
    """Inputs of case c in its element type: taps random (- 0.35 when signed), object 50 * random (90 % zeros when sparse)."""
    rng = np.random.default_rng(9000 + c.seed)
    T = c.dtype
    off = 0.35 if c.signed else 0.0

    def image(*shape, scale=1.0, lift=0.0, sparse=c.sparse):
        a = rng.random(shape) * scale + lift
        if sparse:
            a = a * (rng.random(shape) < 0.1)
        return np.ascontiguousarray(a.astype(T))
    if c.form == 'direct':
        c.views = Views(True, p=(rng.random((c.V, c.py, c.px)) - off).astype(T))
    else:
        c.views = Views(False, u=(rng.random((c.V, c.py)) - off).astype(T), v=(rng.random((c.V, c.px)) - off).astype(T))
    c.x = image(c.frames, c.ny, c.nx, scale=50.0)                        # STORE / RATIO input
    c.y = image(c.frames, c.V, c.ny, c.nx, scale=50.0)                   # SUM / UPDATE input, image order [frame * V + view]
    c.aux = image(c.frames, c.V, c.ny, c.nx, lift=0.5, sparse=False)     # the measurement of RATIO
    c.norm = image(c.ny, c.nx, lift=0.5, sparse=False)
    c.est0 = image(c.frames, c.ny, c.nx, scale=2.0, sparse=False)
    return c


# ------------------------------------------------------------------------------------------------ the emulator
def build_emulator():
    """tests/emu/libsep_emu.so, rebuilt when its sources are newer; RLSTED_SEP_EMU_LIB names a prebuilt (sanitized) one instead."""
    override = os.environ.get('RLSTED_SEP_EMU_LIB')
    if override:
        return override
    so, src = os.path.join(EMU_DIR, 'libsep_emu.so'), os.path.join(EMU_DIR, 'sep_emu.cpp')
    deps = [src] + [os.path.join(CSRC, f) for f in ('sep_kernels.hpp', 'sep_taps.hpp', 'aux_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', '-pthread',
                               src, '-o', so])
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


CANARY = 12345.678                      # what a destination holds where no kernel may write
GUARD = 256                             # elements of guard band on either side of a destination


def guarded(shape, dtype, fill=None):
    """(view of `shape`, whole buffer): a destination with a guard band of CANARY before and after it."""
    n = int(np.prod(shape))
    buf = np.full(n + 2 * GUARD, CANARY, dtype=dtype)
    view = buf[GUARD:GUARD + n].reshape(shape)
    if fill is not None:
        view[...] = fill
    return view, buf


def guards_intact(buf):
    return bool(np.all(buf[:GUARD] == buf.dtype.type(CANARY)) and np.all(buf[-GUARD:] == buf.dtype.type(CANARY)))


class Emulator:
    def __init__(self, path=None):
        self.lib = lib = ctypes.CDLL(path or build_emulator())
        vp, st, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.emu_sep_rows.argtypes = [i, vp, vp, vp, i, i, i, i, i, i]
        lib.emu_sep_cols.argtypes = [i, i, vp, vp, vp, vp, vp, i, i, i, i, i]
        lib.emu_sep2d.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i]
        for name, args in (('emu_sep_rows_lds', [st, i]), ('emu_sep_cols_lds', [st, i]), ('emu_sep2d_lds', [st, i, i, i, i, i]), ('emu_sep_max_lds', [])):
            getattr(lib, name).restype = st
            getattr(lib, name).argtypes = args
        lib.emu_sep2d_fits.argtypes = lib.emu_direct2d_fits.argtypes = [st, i, i, i, i]
        lib.emu_two_pass_fits.argtypes = [st, i, i]
        lib.emu_rank1.argtypes = [vp, i, i, i, vp, vp]
        lib.emu_flipped_taps.argtypes = [vp, vp, i, i, i, vp, vp]
        lib.emu_direct_taps.argtypes = [vp, i, i, i, vp]
        lib.emu_box_integral.argtypes = [vp, i, i, i, vp]
        lib.emu_box_norm.argtypes = [i, vp, vp, i, i, i, i, i]
        for f in ('emu_flipped_taps', 'emu_direct_taps', 'emu_box_integral', 'emu_box_norm'):
            getattr(lib, f).restype = None

    # ---- size rules
    def fits(self, form, esize, th, V, py, px):
        if form == 'two':
            return bool(self.lib.emu_two_pass_fits(esize, py, px))
        return bool((self.lib.emu_sep2d_fits if form == 'one' else self.lib.emu_direct2d_fits)(esize, th, py, px, V))

    def fits_for(self, form, esize, th, V):
        return lambda py, px: self.fits(form, esize, th, V, py, px)

    # ---- host side
    def rank1(self, psfs):
        psfs = np.ascontiguousarray(psfs, dtype=np.float64)
        V, py, px = psfs.shape
        u, v = np.full((V, py), np.nan), np.full((V, px), np.nan)
        ok = self.lib.emu_rank1(_p(psfs), V, py, px, _p(u), _p(v))
        return bool(ok), u, v

    def flipped_taps(self, u, v):
        u, v = np.ascontiguousarray(u, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
        (V, py), px = u.shape, v.shape[1]
        uf, vf = np.full((V, (py + 7) // 8 * 8), np.nan), np.full((V, (px + 7) // 8 * 8), np.nan)
        self.lib.emu_flipped_taps(_p(u), _p(v), V, py, px, _p(uf), _p(vf))
        return uf, vf

    def direct_taps(self, psfs):
        psfs = np.ascontiguousarray(psfs, dtype=np.float64)
        V, py, px = psfs.shape
        f = np.full((V, px, (py + 7) // 8 * 8), np.nan)
        self.lib.emu_direct_taps(_p(psfs), V, py, px, _p(f))
        return f

    def box_norm(self, psfs, ny, nx, dtype):
        psfs = np.ascontiguousarray(psfs, dtype=np.float64)
        V, py, px = psfs.shape
        integ = np.full((V, py + 1, px + 1), np.nan)
        self.lib.emu_box_integral(_p(psfs), V, py, px, _p(integ))
        out, buf = guarded((ny, nx), dtype)
        self.lib.emu_box_norm(0 if np.dtype(dtype) == np.float32 else 1, _p(integ), _p(out), V, py, px, ny, nx)
        assert guards_intact(buf)
        return out.copy(), integ

    # ---- the kernels, launched as rlsted.cpp launches them
    def tables(self, views, dtype):
        """The device tables of a plan in the element type: as deconv_build makes them (float64 tables converted on upload)."""
        if views.direct:
            return {'uf': np.ascontiguousarray(self.direct_taps(views.p).astype(dtype))}
        uf, vf = self.flipped_taps(views.u, views.v)
        return {'u': np.ascontiguousarray(views.u.astype(dtype)), 'v': np.ascontiguousarray(views.v.astype(dtype)),
                'uf': np.ascontiguousarray(uf.astype(dtype)), 'vf': np.ascontiguousarray(vf.astype(dtype))}

    def run(self, form, th, mode, src, tab, views, dst, frames, ny, nx, aux=None, norm=None):
        """One epilogue over `frames` frames.  STORE / RATIO: src [frames] -> dst [frames * V]; SUM / UPDATE: src [frames * V] ->
        dst [frames].  Returns the launcher's verdict (0, or -1 for a size it refuses)."""
        dt = 0 if src.dtype == np.float32 else 1
        V, py, px = views.V, views.py, views.px
        multi = mode in (SUM, UPDATE)
        if form == 'two':
            tmp, tbuf = guarded((frames * V, ny, nx), src.dtype)
            if not self.lib.emu_two_pass_fits(src.dtype.itemsize, py, px):
                return -1
            r = self.lib.emu_sep_rows(dt, _p(src), _p(tmp), _p(tab['v']), frames * V, ny, nx, px, V, 1 if multi else V)
            assert r == 0 and guards_intact(tbuf), 'row pass wrote outside its images'
            assert not np.any(tmp == tmp.dtype.type(CANARY)) or tmp.size == 0, 'row pass left an output unwritten'
            return self.lib.emu_sep_cols(dt, mode, _p(tmp), _p(tab['u']), _p(aux), _p(norm), _p(dst), frames if multi else frames * V, ny, nx, py, V)
        direct = 1 if form == 'direct' else 0
        return self.lib.emu_sep2d(dt, mode, th, direct, _p(src), _p(tab['uf']), None if direct else _p(tab['vf']), _p(aux), _p(norm), _p(dst),
                                  frames, ny, nx, py, px, V)
