"""The row kernels of the long, workgroup-synchronous lengths (L = 1152, 2304, 4608) on the CPU, element by element against an
exact DFT.  CPU only.

tests/emu/long_emu.cpp runs rowpass_body (every mode) and rowpair_body (the `Q == 1` branch of k_rowpair) of
rescan_line_sted_amd/csrc/conv_kernels.hpp exactly as fft_kernels.hip instantiates and dispatches them, one OS thread per GPU
thread, LDS poisoned; tests/emu/long_outer_emu.cpp the outer-decimation column kernels with every setting read from
OuterCol<L> and the LDS at the launcher's byte count.  tests/fft_reference.py is the reference (direct long-double DFT sums)
and derives the per-element bounds: no tolerance below is a literal.  The worst error / bound per body, type and length is
printed at the end of the module (pytest -s) and kept in profiles/r09/long_rows_emulation.log.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fft_reference as fr
from conftest import ROOT, fuzz_seeds
from test_emulated_kernels import emu  # noqa: F401  (the short lengths' emulator, a fixture)
from fft_reference import CLD, LD, ROW_ADJ, ROW_FWD, ROW_INV, ROW_RATIO, ROW_UPDATE

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
LENGTHS = (1152, 2304, 4608)
DTYPES = (np.float32, np.float64)
MODE_NAME = {ROW_FWD: 'FWD', ROW_INV: 'INV', ROW_RATIO: 'RATIO', ROW_UPDATE: 'UPDATE', ROW_ADJ: 'ADJ'}
CANARY = 12345.678
GUARD = 256


def tname(dtype):
    return 'f32' if np.dtype(dtype) == np.float32 else 'f64'


def ctype_of(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


# ------------------------------------------------------------------------------------------------ the libraries
def _build(names):
    """tests/emu/lib<name>.so for each name, rebuilt (side by side) when a source is newer; RLSTED_<NAME>_LIB names a prebuilt
    (sanitized) one instead."""
    out, procs = {}, []
    hdrs = [os.path.join(CSRC, f) for f in ('conv_kernels.hpp', 'fft_core.hpp', 'fft_configs.hpp', 'outer_lds.hpp', 'kernel_variants.hpp')] + \
        [os.path.join(EMU_DIR, 'emu_common.hpp')]
    for name in names:
        override = os.environ.get('RLSTED_%s_LIB' % name.upper())
        if override:
            out[name] = override
            continue
        so, src = os.path.join(EMU_DIR, 'lib%s.so' % name), os.path.join(EMU_DIR, name + '.cpp')
        out[name] = so
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [src] + hdrs):
            procs.append(subprocess.Popen(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas',
                                           '-pthread', src, '-o', so]))
    for p in procs:
        assert p.wait() == 0
    return out


@pytest.fixture(scope='module')
def libs():
    paths = _build(('long_emu', 'long_outer_emu'))
    rows, outer = ctypes.CDLL(paths['long_emu']), ctypes.CDLL(paths['long_outer_emu'])
    vp, i = ctypes.c_void_p, ctypes.c_int
    for sfx in ('f32', 'f64'):
        getattr(rows, 'emu_long_row_' + sfx).argtypes = [i, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp]
        getattr(rows, 'emu_long_row_pair_' + sfx).argtypes = [i, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, vp]
        getattr(outer, 'emu_outer_whole_' + sfx).argtypes = [i, vp, vp, vp, i, i, i, i, i, i, i, i]
    outer.emu_outer_split_f32.argtypes = [i, vp, vp, vp, i, i, i, i, i, i, i]
    yield rows, outer
    print()
    for line in fr.WORST.lines():
        print(line)


@pytest.fixture(scope='module')
def lib(libs):
    return libs[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def geometry(lib, L):
    T, np_, slots = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rad = (ctypes.c_int * 4)()
    assert lib.emu_long_geometry(L, ctypes.byref(T), rad, ctypes.byref(np_), ctypes.byref(slots)) == 0
    return T.value, tuple(rad[:np_.value]), slots.value


_ARITH = {}


def arith(lib, L, dtype, div=1):
    key = (L, tname(dtype), div)
    if key not in _ARITH:
        _ARITH[key] = fr.Arith(dtype, geometry(lib, L)[1], div)
    return _ARITH[key]


# ------------------------------------------------------------------------------------------------ the plan's size rules
def length_for(n):
    from rescan_line_sted_amd import _lib
    return _lib.lib.rl_fft_length_for(n)


def nx_limits(L):
    """(smallest, largest) padded row length the plan's size rule (rlsted.cpp rl_fft_length_for) maps to L"""
    hi = L
    assert length_for(hi) == L and length_for(hi + 1) != L
    lo = hi
    while lo > 1 and length_for(lo - 1) == L:
        lo -= 1
    return lo, hi


def pair_pitch(L):
    """Row pitch of a pair spectrum, from the line of rlsted.cpp that sets it"""
    m = re.search(r'pair_pitch = h->lx \+ \(h->lx >= (\d+) \? (\d+) : 0\);', open(os.path.join(CSRC, 'rlsted.cpp')).read())
    assert m, 'rlsted.cpp no longer sets pair_pitch this way: restate the rule here'
    return L + (int(m.group(2)) if L >= int(m.group(1)) else 0)


def half_pitch(L):
    return (L // 2 + 1 + 7) // 8 * 8      # conv_kernels.hpp: Kx = Lx/2 + 1 valid columns, pitch = Kx rounded up to 8


EDGES = fr.EDGES


def edge_table(L):
    """fft_reference.edge_rows at the limits the plan's size rule gives the length.  (Computed when a test runs: the size rule
    is the built library's.)"""
    return fr.edge_rows(*nx_limits(L))


def test_edge_table_follows_the_size_rule():
    for L in LENGTHS:
        lo, hi = nx_limits(L)
        assert hi == L and 0 < length_for(lo - 1) < L and length_for(lo) == L
        tab = list(edge_table(L).values())
        assert len(tab) == len(EDGES)
        nxs = {nx for _, nx, _ in tab}
        assert {lo, hi, 1} <= nxs and any(nx % 2 for nx in nxs if nx > 1) and any(nx % 4 and nx % 2 == 0 for nx in nxs)
        assert any(nx % 64 and nx % 16 == 0 for nx in nxs)
        assert all(nx == 1 or length_for(nx) == L for nx in nxs)
        assert 1 in {ny for ny, _, _ in tab} and any(ny % 2 and ny > 1 for ny, _, _ in tab)


# ------------------------------------------------------------------------------------------------ buffers
def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = np.full(n + 2 * GUARD, CANARY, dtype=dtype)
    view = buf[GUARD:GUARD + n].reshape(shape)
    view[...] = fill
    return view, buf


def guards_intact(buf):
    return bool(np.all(buf[:GUARD] == buf.dtype.type(CANARY)) and np.all(buf[-GUARD:] == buf.dtype.type(CANARY)))


def poisoned_spec(n, ny, pitch, dtype):
    return guarded((n, ny, pitch), ctype_of(dtype), np.nan + 1j * np.nan)


def spectrum_input(values, pitch, dtype):
    """[n][ny][cols] complex -> the buffer a kernel reads: element type, row pitch `pitch`, NaN in the pad columns"""
    n, ny, cols = values.shape
    s = np.full((n, ny, pitch), np.nan + 1j * np.nan, dtype=ctype_of(dtype))
    s[:, :, :cols] = values.astype(np.complex128)
    return s


def draw_image(rng, shape, dtype, kind, lo=0.5, hi=3.5):
    """Values in float32 (exact in both element types, so both types share a reference)."""
    a = rng.random(shape) * (hi - lo) + lo
    if kind == 'one_pixel':
        b = np.zeros(shape)
        b[..., shape[-2] // 2, (2 * shape[-1]) // 3] = 100.0 * a[..., 0, 0]
        a = b
    if kind == 'zero_row':
        a[..., :2, :] = 0            # a whole row pair (what shares a transform)
    return np.ascontiguousarray(a.astype(np.float32).astype(dtype))


def half_spectra_of(dft, imgs, dtype, scale=None):
    """Row half spectra / L of real images [n][ny][nx] in the element type: an input whose inverse row pass returns ~ the images.
    The bins 0 and L/2 of a real row are real; a kernel must not rely on that (the packing treats them as any other bin), so
    they get a small imaginary part (1e-2 of their modulus: it moves the partner row by that much of the mean)."""
    n, ny, nx = imgs.shape
    F = dft.forward_real(imgs.reshape(n * ny, nx).astype(LD)) / LD(dft.L if scale is None else scale)
    for k, sign in ((0, 1), (dft.H, -1)):
        F[:, k] = F[:, k] * (1 + sign * LD(1e-2) * 1j)
    return spectrum_input(F.reshape(n, ny, -1), half_pitch(dft.L), dtype)


# ------------------------------------------------------------------------------------------------ per-frame bodies
def prediction(rng, shape, dtype, kind):
    """What ROW_RATIO divides by: positive, with clearly negative pixels (neutral: ratio 1, residual 0) among them"""
    a = draw_image(rng, shape, dtype, 'random' if kind != 'zero_row' else 'zero_row')
    neg = rng.random(shape) < 0.1
    a[neg & (a != 0)] = -0.25
    return a


def run_frame_mode(lib, L, dtype, mode, ny, nx, kind, seed, V=1, frames=2, sub_one=0, with_norm=True, in_mod=0):
    """One launch of a per-frame row mode through the emulator against the reference.  Returns the worst error / bound."""
    rng = np.random.default_rng(1000 * seed + 17 * mode + V)
    dft, ar = fr.RowDFT.get(L), arith(lib, L, dtype)
    kx, pitch = L // 2 + 1, half_pitch(L)
    key = ('rowpass' + ('+PRESUM' if mode == ROW_UPDATE and V > 1 and sub_one else ''), tname(dtype), L, MODE_NAME[mode])
    ctx = dict(L=L, ny=ny, nx=nx, kind=kind, V=V, frames=frames, sub_one=sub_one, seed=seed)
    f = getattr(lib, 'emu_long_row_' + tname(dtype))
    n_img = frames * V if mode != ROW_FWD else frames
    unresolved = np.zeros(1, dtype=np.uint64)
    worst = 0.0

    def call(spec_in, spec_out, src, dst, norm, scale, gy):
        assert f(L, mode, _p(spec_in), _p(spec_out), _p(src), _p(dst), _p(norm), _p(scale), ny, nx, pitch, V, gy, sub_one, in_mod,
                 _p(unresolved)) == 0, ctx

    def spec_checks(out, buf):
        assert guards_intact(buf), ('wrote outside the spectra', ctx)
        assert np.isnan(out[:, :, kx:].real).all() and np.isnan(out[:, :, kx:].imag).all(), ('wrote past kx', ctx)

    if mode == ROW_FWD:
        src = draw_image(rng, (frames, ny, nx), dtype, kind)
        scale = np.array([2.5, 0.75, 1.0][:frames], dtype=dtype) if seed % 2 == 0 else None
        out, buf = poisoned_spec(frames, ny, pitch, dtype)
        call(None, out, src, None, None, scale, frames)
        spec_checks(out, buf)
        for i in range(frames):
            img = src[i].astype(LD) * (LD(scale[i]) if scale is not None else 1)
            F, B = fr.frame_forward(dft, ar, img, ar.u * np.abs(img) if scale is not None else None)
            worst = max(worst, fr.check(out[i, :, :kx], F, B, key, ctx))
        return worst

    # the modes that begin with an inverse transform: spectra whose inverse is a designed image
    n_spec = in_mod if in_mod > 0 else n_img
    if mode == ROW_RATIO:
        target = prediction(rng, (n_spec, ny, nx), dtype, kind)
    elif mode == ROW_UPDATE and sub_one:
        target = draw_image(rng, (n_spec, ny, nx), dtype, 'random', -1.5, 1.0) / max(V, 1)     # H_t(ratio - 1): both signs, 1 + f crosses 0
        if kind == 'zero_row':
            target[:, :2] = 0
    else:
        target = draw_image(rng, (n_spec, ny, nx), dtype, kind, -1.0, 3.0)                   # the clamp matters
    spec_in = half_spectra_of(dft, target, dtype)
    if mode == ROW_INV:
        dst, buf = guarded((n_img, ny, nx), dtype, np.nan)
        call(spec_in, None, None, dst, None, None, n_img)
        assert guards_intact(buf), ctx
        for i in range(n_img):
            rows, e = fr.frame_inverse(dft, ar, [spec_in[i]], ny, nx)
            worst = max(worst, fr.check(dst[i], np.maximum(rows, 0), e, key, ctx))
        return worst
    if mode == ROW_ADJ:
        norm = draw_image(rng, (ny, nx), dtype, 'random', 0.5, 1.5) if with_norm else None
        dst, buf = guarded((frames, ny, nx), dtype, np.nan)
        call(spec_in, None, None, dst, norm, None, frames)
        assert guards_intact(buf), ctx
        for i in range(frames):
            a, da = view_sum(dft, ar, spec_in[i * V:(i + 1) * V], ny, nx, raw=False)
            if norm is not None:
                q = a / norm.astype(LD)
                da = da / norm + ar.u * (np.abs(q) + da / norm)
                a = q
            worst = max(worst, fr.check(dst[i], a, da, key + ('/norm' if with_norm else '',), ctx))
        return worst
    if mode == ROW_RATIO:
        meas = draw_image(rng, (n_img, ny, nx), dtype, 'one_pixel' if kind == 'one_pixel' else 'random', 0.0, 5.0)
        if kind == 'negative':
            assert not sub_one
            meas[rng.random(meas.shape) < 0.2] *= -1
        out, buf = poisoned_spec(n_img, ny, pitch, dtype)
        if kind == 'nan_prediction':
            spec_in[0, :, :kx] = np.nan + 1j * np.nan              # every pixel of image 0's prediction is NaN
        call(spec_in, out, meas, None, None, None, n_img)
        spec_checks(out, buf)
        neutral = 0
        for i in range(n_img):
            if kind == 'nan_prediction' and i == 0:                # (no long-double sums over NaN: they are slow, and say nothing more)
                rows, e = np.full((ny, nx), np.nan, dtype=LD), np.zeros((ny, 1), dtype=LD)
            else:
                rows, e = fr.frame_inverse(dft, ar, [spec_in[i % in_mod if in_mod > 0 else i]], ny, nx)
            r, dr, undecided = ar.ratio(meas[i], rows, e, sub_one)
            assert not undecided.any(), ('the case generator must not produce a prediction within its bound of zero', ctx)
            neutral += int(((rows <= 0) | np.isnan(rows)).sum())
            F, B = fr.frame_forward(dft, ar, r, dr)
            worst = max(worst, fr.check(out[i, :, :kx], F, B, key + ('sub_one',) * sub_one, ctx))
        assert (int(unresolved[0]) > 0) == (neutral > 0) and int(unresolved[0]) <= neutral, ('lanes that met a neutral pixel', ctx)
        return worst
    assert mode == ROW_UPDATE
    est, ebuf = guarded((frames, ny, nx), dtype, draw_image(rng, (frames, ny, nx), dtype, kind if kind != 'zero_row' else 'random', 0.0, 2.0))
    est0 = est.astype(LD)
    norm = draw_image(rng, (ny, nx), dtype, 'random', 0.5, 1.5)
    out, buf = poisoned_spec(frames, ny, pitch, dtype)
    call(spec_in, out, None, est, norm, None, frames)
    spec_checks(out, buf)
    assert guards_intact(ebuf), ctx
    for i in range(frames):
        specs = spec_in[i * V:(i + 1) * V]
        if sub_one:
            a, da = fr.frame_inverse(dft, ar, list(specs), ny, nx)            # the views' spectra summed on the way in (V = 1: one)
        else:
            a, da = view_sum(dft, ar, specs, ny, nx, raw=False)
        fac, dfac = ar.factor(a, da, norm.astype(LD), sub_one)
        new, dnew = ar.product(est0[i], fac, dfac)
        k2 = key + ('sub_one',) * sub_one + ('V=%d' % V,)
        worst = max(worst, fr.check(est[i], new, dnew, k2 + ('estimate',), ctx))
        F, B = fr.frame_forward(dft, ar, new, dnew)
        worst = max(worst, fr.check(out[i, :, :kx], F, B, k2 + ('spectrum',), ctx))
    return worst


def view_sum(dft, ar, specs, ny, nx, raw):
    """sum over the views of their (clamped) inverse rows, accumulated one after the other from zero"""
    V = len(specs)
    a, da, mag = 0, 0, 0
    for s in specs:
        rows, e = fr.frame_inverse(dft, ar, [s], ny, nx)
        v = rows if raw else np.maximum(rows, 0)
        a, da, mag = a + v, da + e, mag + np.abs(v) + e
    return a, da + (fr.gamma(V - 1, ar.u) * mag if V > 1 else 0)


@pytest.mark.parametrize('dtype', DTYPES, ids=tname)
@pytest.mark.parametrize('edge', EDGES)
@pytest.mark.parametrize('L', LENGTHS)
def test_frame_modes_on_the_edge_table(lib, L, edge, dtype):
    """Every per-frame row mode at every edge of the table.  Spectra and outputs start as NaN: every element of the valid region
    is written and finite, nothing past kx or outside the buffers is written, pad columns of the input are never read."""
    ny, nx, kind = edge_table(L)[edge]
    seed = ny * 7 + nx
    if kind == 'negative':
        run_frame_mode(lib, L, dtype, ROW_RATIO, ny, nx, kind, seed, sub_one=0)
        return
    run_frame_mode(lib, L, dtype, ROW_FWD, ny, nx, kind, seed)
    run_frame_mode(lib, L, dtype, ROW_FWD, ny, nx, kind, seed + 1)                          # (with / without the per-frame scale)
    run_frame_mode(lib, L, dtype, ROW_INV, ny, nx, kind, seed)
    run_frame_mode(lib, L, dtype, ROW_ADJ, ny, nx, kind, seed, V=1, with_norm=True)
    for sub_one in (0, 1):
        run_frame_mode(lib, L, dtype, ROW_RATIO, ny, nx, kind, seed, sub_one=sub_one)
        run_frame_mode(lib, L, dtype, ROW_UPDATE, ny, nx, kind, seed, sub_one=sub_one)


@pytest.mark.parametrize('dtype', DTYPES, ids=tname)
@pytest.mark.parametrize('V', [2, 4])
@pytest.mark.parametrize('L', LENGTHS)
def test_frame_modes_with_views(lib, L, V, dtype):
    """The modes that have views, V = 2 and 4 (V = 1 is in the edge table): ROW_INV / ROW_RATIO per (frame, view) image, ROW_ADJ
    and the plain ROW_UPDATE accumulating clamped views, the `ratio - 1` update summing the views' spectra on the way in
    (PRESUM: three at a time, so 2 and 4), ROW_RATIO of the first iteration reading V shared spectra (in_mod)."""
    lo, hi = nx_limits(L)
    ny, nx = 3, lo + 5 * V
    run_frame_mode(lib, L, dtype, ROW_INV, ny, nx, 'random', V, V=V, frames=1)
    run_frame_mode(lib, L, dtype, ROW_ADJ, ny, nx, 'random', V, V=V, frames=1, with_norm=False)
    run_frame_mode(lib, L, dtype, ROW_ADJ, ny, nx, 'random', V, V=V, frames=1, with_norm=True)
    run_frame_mode(lib, L, dtype, ROW_RATIO, ny, nx, 'random', V, V=V, frames=2, sub_one=1, in_mod=V)
    run_frame_mode(lib, L, dtype, ROW_RATIO, ny, nx, 'random', V, V=V, frames=1, sub_one=0)
    run_frame_mode(lib, L, dtype, ROW_UPDATE, ny, nx, 'random', V, V=V, frames=1, sub_one=0)
    run_frame_mode(lib, L, dtype, ROW_UPDATE, ny, nx, 'random', V, V=V, frames=2, sub_one=1)
    run_frame_mode(lib, L, dtype, ROW_UPDATE, 2, hi, 'one_pixel', V, V=V, frames=1, sub_one=1)


# ------------------------------------------------------------------------------------------------ pair bodies
def pair_frames(a, p, frames):
    """frames 2p and 2p+1 of `a`; the missing partner of an odd batch's last frame is a phantom copy of it"""
    return a[2 * p], a[2 * p + 1] if 2 * p + 1 < frames else a[2 * p]


def run_pair_mode(lib, L, dtype, mode, ny, nx, kind, seed, frames=3, V=1, sub_one=0, in_mod=0, special=0, keep=None):
    rng = np.random.default_rng(5000 + 1000 * seed + 17 * mode + V)
    dft, ar = fr.RowDFT.get(L), arith(lib, L, dtype)
    pitch, pairs = pair_pitch(L), (frames + 1) // 2
    key = ('rowpair' + ('+NXC' if special else ''), tname(dtype), L, MODE_NAME[mode]) + ('sub_one',) * sub_one
    ctx = dict(L=L, ny=ny, nx=nx, kind=kind, V=V, frames=frames, sub_one=sub_one, seed=seed, special=special)
    f = getattr(lib, 'emu_long_row_pair_' + tname(dtype))
    unresolved = np.zeros(1, dtype=np.uint64)
    worst = 0.0

    def call(spec_in, spec_out, src, dst, norm):
        assert f(L, mode, _p(spec_in), _p(spec_out), _p(src), _p(dst), _p(norm), ny, nx, pitch, V, frames, in_mod, sub_one, special,
                 _p(unresolved)) == 0, ctx

    def spec_checks(out, buf):
        assert guards_intact(buf), ('wrote outside the spectra', ctx)
        assert np.isnan(out[:, :, L:].real).all() and np.isnan(out[:, :, L:].imag).all(), ('wrote past the row', ctx)

    def pair_spectra_of(target, n):
        """[n pairs][ny][L] / L of the complex images target[2i] + i target[2i+1]"""
        vals = np.empty((n, ny, L), dtype=CLD)
        for i in range(n):
            vals[i] = dft.forward_pair(target[2 * i].astype(LD), target[2 * i + 1].astype(LD)) / LD(L)
        return spectrum_input(vals, pitch, dtype)

    if mode == ROW_FWD:
        src = draw_image(rng, (frames, ny, nx), dtype, kind)
        out, buf = poisoned_spec(pairs, ny, pitch, dtype)
        call(None, out, src, None, None)
        spec_checks(out, buf)
        for p in range(pairs):
            a, b = pair_frames(src, p, frames)
            S, B = fr.pair_forward(dft, ar, a, b)
            worst = max(worst, fr.check(out[p, :, :L], S, B, key, ctx))
        return worst
    if mode == ROW_RATIO:
        n_img = pairs * V
        n_spec = in_mod if in_mod > 0 else n_img
        spec_in = pair_spectra_of(prediction(rng, (2 * n_spec, ny, nx), dtype, kind), n_spec)
        meas = draw_image(rng, (frames * V, ny, nx), dtype, 'one_pixel' if kind == 'one_pixel' else 'random', 0.0, 5.0)
        if kind == 'negative':
            meas[rng.random(meas.shape) < 0.2] *= -1
        out, buf = poisoned_spec(n_img, ny, pitch, dtype)
        if kind == 'nan_prediction':
            spec_in[0, :, :L] = np.nan + 1j * np.nan               # every pixel of pair 0's prediction is NaN, both frames
        call(spec_in, out, meas, None, None)
        spec_checks(out, buf)
        neutral = 0
        mv = meas.reshape(frames, V, ny, nx)
        for by in range(n_img):
            p, vw = by // V, by % V
            if kind == 'nan_prediction' and by == 0:
                re = im = np.full((ny, nx), np.nan, dtype=LD)
                e = np.zeros((ny, 1), dtype=LD)
            else:
                re, im, e = fr.pair_inverse(dft, ar, spec_in[by % in_mod if in_mod > 0 else by], nx)
            ma, mb = pair_frames(mv[:, vw], p, frames)
            ra, dra, ua = ar.ratio(ma, re, e, sub_one)
            rb, drb, ub = ar.ratio(mb, im, e, sub_one)
            assert not ua.any() and not ub.any(), ('the case generator must not produce a prediction within its bound of zero', ctx)
            neutral += int(((re <= 0) | np.isnan(re)).sum()) + (int(((im <= 0) | np.isnan(im)).sum()) if 2 * p + 1 < frames else 0)      # (a phantom is not a frame)
            S, B = fr.pair_forward(dft, ar, ra, rb, dra, drb)
            worst = max(worst, fr.check(out[by, :, :L], S, B, key, ctx))
        assert (int(unresolved[0]) > 0) == (neutral > 0) and int(unresolved[0]) <= neutral, ('lanes that met a neutral pixel', ctx)
        if keep is not None:
            keep.append(out.copy())
        return worst
    assert mode == ROW_UPDATE and V == 1
    if sub_one:
        target = draw_image(rng, (2 * pairs, ny, nx), dtype, 'random', -1.5, 1.0)
    else:
        target = draw_image(rng, (2 * pairs, ny, nx), dtype, kind, -1.0, 3.0)
    if kind == 'zero_row':
        target[:, :2] = 0
    spec_in = pair_spectra_of(target, pairs)
    est, ebuf = guarded((frames, ny, nx), dtype, draw_image(rng, (frames, ny, nx), dtype, kind if kind != 'zero_row' else 'random', 0.0, 2.0))
    est0 = est.astype(LD)
    norm = draw_image(rng, (ny, nx), dtype, 'random', 0.5, 1.5)
    out, buf = poisoned_spec(pairs, ny, pitch, dtype)
    call(spec_in, out, None, est, norm)
    spec_checks(out, buf)
    assert guards_intact(ebuf), ctx
    for p in range(pairs):
        re, im, e = fr.pair_inverse(dft, ar, spec_in[p], nx)
        ea, eb = pair_frames(est0, p, frames)
        new, dnew = [], []
        for v, x in ((re, ea), (im, eb)):
            fac, dfac = ar.factor(v if sub_one else np.maximum(v, 0), e, norm.astype(LD), sub_one)
            n_, d_ = ar.product(x, fac, dfac)
            new.append(n_)
            dnew.append(d_)
        worst = max(worst, fr.check(est[2 * p], new[0], dnew[0], key + ('estimate',), ctx))
        if 2 * p + 1 < frames:
            worst = max(worst, fr.check(est[2 * p + 1], new[1], dnew[1], key + ('estimate',), ctx))
        S, B = fr.pair_forward(dft, ar, new[0], new[1], dnew[0], dnew[1])
        worst = max(worst, fr.check(out[p, :, :L], S, B, key + ('spectrum',), ctx))
    if keep is not None:
        keep.append((est.copy(), out.copy()))
    return worst


@pytest.mark.parametrize('dtype', DTYPES, ids=tname)
@pytest.mark.parametrize('edge', EDGES)
@pytest.mark.parametrize('L', LENGTHS)
def test_pair_modes_on_the_edge_table(lib, L, edge, dtype):
    """rowpair_body on the workgroup-synchronous geometries (the `Q == 1` branch of k_rowpair), FWD / RATIO / UPDATE, with an odd
    frame count (the last frame's partner is a phantom), the plan's row pitch (pad columns beside the row: never read, never
    written), with and without `ratio - 1`."""
    ny, nx, kind = edge_table(L)[edge]
    seed = ny * 7 + nx
    frames = 3 if ny < 5 else 1
    if kind == 'negative':
        run_pair_mode(lib, L, dtype, ROW_RATIO, ny, nx, kind, seed, frames=frames, sub_one=0)
        return
    run_pair_mode(lib, L, dtype, ROW_FWD, ny, nx, kind, seed, frames=frames)
    for sub_one in (0, 1):
        run_pair_mode(lib, L, dtype, ROW_RATIO, ny, nx, kind, seed, frames=frames, sub_one=sub_one)
        run_pair_mode(lib, L, dtype, ROW_UPDATE, ny, nx, kind, seed, frames=frames, sub_one=sub_one)


@pytest.mark.parametrize('dtype', DTYPES, ids=tname)
@pytest.mark.parametrize('L', LENGTHS)
def test_a_nan_prediction_is_neutral(lib, L, dtype):
    """rl_ratio's rule for a prediction that is NaN (a spectrum that went non-finite): the pixel is neutral -- ratio 1, residual 0
    -- as for a prediction <= 0, so the image's ratio spectrum is the exact spectrum of ones (or zeros) and finite; the other
    image of the launch is untouched by it.  Per-frame and pair bodies, with and without `ratio - 1`."""
    lo, _ = nx_limits(L)
    for sub_one in (0, 1):
        run_frame_mode(lib, L, dtype, ROW_RATIO, 3, lo + 4, 'nan_prediction', L + sub_one, sub_one=sub_one)
        run_pair_mode(lib, L, dtype, ROW_RATIO, 2, lo + 4, 'nan_prediction', L + sub_one, frames=3, sub_one=sub_one)


@pytest.mark.parametrize('dtype', DTYPES, ids=tname)
@pytest.mark.parametrize('L', LENGTHS)
def test_pair_ratio_with_views_and_shared_first_spectra(lib, L, dtype):
    """ROW_RATIO of a multi-view plan runs per (pair, view) image; the first iteration's V spectra are shared by every pair
    (in_mod); even and odd frame counts."""
    lo, _ = nx_limits(L)
    for V, frames, in_mod in ((2, 3, 0), (4, 2, 4), (2, 4, 2)):
        run_pair_mode(lib, L, dtype, ROW_RATIO, 2, lo + 11, 'random', V, frames=frames, V=V, sub_one=1, in_mod=in_mod)


def test_pair_bodies_with_the_row_length_at_compile_time(lib):
    """rowpair_body<..., NXC = 2048, SUBC = 1> on the 2304 geometry (the device's 2048-pixel frame-pair kernels, DeviceSpecial::pair_nx, float): bit for bit the
    run-time-size body's result, and the reference's within the bound."""
    L, ny, nx, frames = 2304, 3, 2048, 3
    for mode in (ROW_RATIO, ROW_UPDATE):
        kept = []
        for special in (0, 1):
            run_pair_mode(lib, L, np.float32, mode, ny, nx, 'random', 3, frames=frames, sub_one=1, special=special, keep=kept)
        a, b = kept
        if mode == ROW_RATIO:
            assert np.array_equal(a, b, equal_nan=True)
        else:
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


# ------------------------------------------------------------------------------------------------ random cases
@pytest.mark.parametrize('seed', fuzz_seeds(18))
def test_random_cases(lib, seed):
    """Seeded random geometry: length x type x body x mode x ny 1-5 x nx anywhere in the length's range (a third of the seeds
    below it: short rows are legal) x V x frames x `ratio - 1`."""
    rng = np.random.default_rng(424200 + seed)
    L = LENGTHS[seed % 3]
    dtype = DTYPES[(seed // 3) % 2]
    lo, hi = nx_limits(L)
    nx = int(rng.integers(1, lo)) if rng.random() < 0.33 else int(rng.integers(lo, hi + 1))
    ny = int(rng.integers(1, 6))
    sub_one = int(rng.integers(0, 2))
    kind = ('random', 'one_pixel', 'zero_row')[int(rng.integers(0, 3))]
    if kind == 'zero_row' and ny < 3:
        kind = 'random'
    if seed % 2 == 0:
        mode = int(rng.integers(0, 5))
        V = int(rng.integers(1, 5)) if mode != ROW_FWD else 1
        in_mod = V if (mode == ROW_RATIO and rng.random() < 0.5) else 0
        if mode == ROW_ADJ:
            sub_one = 0
        run_frame_mode(lib, L, dtype, mode, ny, nx, kind, seed, V=V, frames=int(rng.integers(1, 3)), sub_one=sub_one if mode in (ROW_RATIO, ROW_UPDATE) else 0,
                       with_norm=bool(rng.integers(0, 2)), in_mod=in_mod)
    else:
        mode = (ROW_FWD, ROW_RATIO, ROW_UPDATE)[int(rng.integers(0, 3))]
        V = int(rng.integers(1, 4)) if mode == ROW_RATIO else 1
        run_pair_mode(lib, L, dtype, mode, ny, nx, kind, seed, frames=int(rng.integers(1, 5)), V=V, sub_one=sub_one if mode != ROW_FWD else 0)


# ------------------------------------------------------------------------------------------------ the row chain
class Layout:
    """How images ride through the complex row transforms.  Per-frame form: a transform row is (frame, row pair) = row 2p +
    i row 2p+1, and the missing partner of an odd row count is zero for ever.  Pair form: (frame pair, row) = frame 2q +
    i frame 2q+1, and the missing partner of an odd frame count is a PHANTOM: it reads frame 2q's images and is never stored."""

    def __init__(self, pairwise, frames, ny, nx):
        self.pairwise, self.frames, self.ny, self.nx = pairwise, frames, ny, nx

    def split(self, imgs):
        """images [frames][ny][nx] -> (A, B, exists) component rows [rows][nx]: B of a phantom is a copy of A, of a missing row zero"""
        a = np.asarray(imgs, dtype=LD)
        if self.pairwise:
            b = np.concatenate([a, a[-1:]]) if self.frames % 2 else a
            A, B = b[0::2].reshape(-1, self.nx), b[1::2].reshape(-1, self.nx)
            exists = np.repeat(np.arange(1, len(b), 2) < self.frames, self.ny)
        else:
            b = np.concatenate([a, np.zeros_like(a[:, :1])], axis=1) if self.ny % 2 else a
            A, B = b[:, 0::2].reshape(-1, self.nx), b[:, 1::2].reshape(-1, self.nx)
            exists = np.tile(np.arange(1, b.shape[1], 2) < self.ny, self.frames)
        return A, B, exists[:, None]


class ChainRef:
    """ROW_FWD -> [identity column pass -> ROW_RATIO -> identity column pass -> ROW_UPDATE] x K in long double, every quantity
    with the bound of what an emulated chain may differ from it by.  An identity column pass multiplies a spectrum by c = 1 / L
    rounded to the element type.  Forward -> c -> inverse is c L times the identity on the pixels, so a pixel's CARRIED error
    passes to the same pixel with weight c L; only the FRESH rounding errors of the three steps spread over the row (the bound
    of fft_reference.py's docstring, applied to them alone)."""

    def __init__(self, dft, ar, pairwise):
        self.dft, self.ar, self.pairwise = dft, ar, pairwise
        self.c = LD(ar.dtype.type(1.0 / dft.L))

    def round_trip(self, A, B, dA, dB):
        """component rows known to dA, dB -> forward, x c, inverse: (c L A, c L B, per-pixel bound of each).  c is real, so a
        pixel's carried error stays in its own component: the real part's does not pass to the imaginary part's pixel."""
        ar, u, G, L, c = self.ar, self.ar.u, self.ar.G, self.dft.L, self.c
        dz = np.hypot(dA, dB)
        zin = (np.hypot(A, B) + dz).sum(axis=1, keepdims=True)     # bounds sum |computed inputs| and any computed bin's modulus
        fresh = G * zin                                            # the forward passes
        if not self.pairwise:
            fresh = 2 * (fresh + u * (zin + fresh))                # the split's add per half spectrum; two half spectra make a bin again
        fresh = fresh + u * (zin + fresh)                          # the product with c, relative to the bin
        if not self.pairwise:
            fresh = fresh + u * (zin + fresh)                      # the packing's add
        fresh = fresh * (1 + 8 * u)                                # the second-order terms of the lines above
        S = self.dft.forward_pair(A, B) * c
        sumS = np.abs(S).sum(axis=1, keepdims=True) + L * c * (dz.sum(axis=1, keepdims=True) + fresh)
        spread = L * c * fresh + G * sumS                          # what every pixel of the row pair may get
        return A * (c * L), B * (c * L), c * L * dA + spread, c * L * dB + spread


def run_chain(lib, L, dtype, pairwise, ny, nx, frames, K, data):
    """The emulated chain, per-frame or pair form: the estimate after every iteration."""
    meas, norm, est0 = data
    c = dtype(1.0 / L)
    est = est0.copy()
    ests = []
    unres = np.zeros(1, dtype=np.uint64)
    if pairwise:
        f = getattr(lib, 'emu_long_row_pair_' + tname(dtype))
        pitch, n = pair_pitch(L), (frames + 1) // 2

        def launch(mode, si, so, src, dst, nrm, sub):
            assert f(L, mode, _p(si), _p(so), _p(src), _p(dst), _p(nrm), ny, nx, pitch, 1, frames, 0, sub, 1, _p(unres)) == 0
    else:
        f = getattr(lib, 'emu_long_row_' + tname(dtype))
        pitch, n = half_pitch(L), frames

        def launch(mode, si, so, src, dst, nrm, sub):
            assert f(L, mode, _p(si), _p(so), _p(src), _p(dst), _p(nrm), None, ny, nx, pitch, 1, frames, sub, 0, _p(unres)) == 0
    sa = np.full((n, ny, pitch), np.nan + 1j * np.nan, dtype=ctype_of(dtype))
    sb = sa.copy()
    launch(ROW_FWD, None, sa, est, None, None, 0)
    for _ in range(K):
        sa *= c                                            # identity column pass (H)
        launch(ROW_RATIO, sa, sb, meas, None, None, 1)
        sb *= c                                            # identity column pass (H_t)
        launch(ROW_UPDATE, sb, sa, None, est, norm, 1)
        ests.append(est.copy())
    assert int(unres[0]) == 0
    return ests


def _chain_cases():
    out = []
    for L in LENGTHS:
        out.append(pytest.param(L, 130, np.float32, 'random', id='%d-nx130-f32' % L))
        out.append(pytest.param(L, 130, np.float64, 'random', id='%d-nx130-f64' % L))
        out.append(pytest.param(L, 0, np.float64, 'random', id='%d-full-f64' % L))
        out.append(pytest.param(L, 130, np.float32, 'one_pixel', id='%d-nx130-one-pixel-lit-f32' % L))
        out.append(pytest.param(L, 0, np.float64, 'one_pixel', id='%d-full-one-pixel-lit-f64' % L))
    return out


def chain_images(rng, frames, ny, nx, dtype, kind):
    """(measurement, normaliser, first estimate).  'random': dense rows.  'one_pixel': what makes the chain's bound sharp -- the
    bound of a transform is G * sum |row|, met only where one pixel carries the row's sum.  Every prediction must stay clear of
    zero, so the rows are not dark but DIM (1e-2 / nx * 130 of the lit pixel: the dim pixels sum to about the lit one), and the
    measurement equals the estimate on the dim pixels, so that `ratio - 1` -- the input of the second transform -- is one lit
    pixel per row as well."""
    norm = draw_image(rng, (ny, nx), dtype, 'random', 0.9, 1.1)
    if kind == 'random':
        return draw_image(rng, (frames, ny, nx), dtype, 'random', 1.5, 2.5), norm, draw_image(rng, (frames, ny, nx), dtype, 'random', 1.5, 2.5)
    dim = 1e-2 * 130 / nx
    est0 = draw_image(rng, (frames, ny, nx), dtype, 'random', 1.5 * dim, 2.5 * dim)
    meas = est0.copy()
    for f in range(frames):
        for r in range(ny):
            j = int(rng.integers(0, nx))
            est0[f, r, j] = np.float32(rng.uniform(1.5, 2.5))
            meas[f, r, j] = np.float32(rng.uniform(1.5, 2.5))
    return meas, norm, est0


@pytest.mark.parametrize('L,nx,dtype,kind', _chain_cases())
def test_row_chain_three_iterations(lib, L, nx, dtype, kind):
    """ROW_FWD -> ROW_RATIO -> ROW_UPDATE (`ratio - 1`) with an identity column pass, 3 iterations, odd frame and row counts (a
    zero partner row in the per-frame form, a phantom partner frame in the pair form): both forms stay within the propagated
    bound of the reference, hence of each other.  The bound is a worst case over the row -- its fresh part grows with
    G * sum |row| per transform and is amplified by measurement / prediction^2 in every ratio -- so in float it still says
    something after three iterations on short rows (130 pixels: a few per cent of the estimate, 1e-9 in float64 on full rows);
    rows at the length's full range run in float64 (nx = 0: the smallest row that selects the length, + 2).  On dense rows the
    real error is a random walk far below that worst case (error / bound < 1e-3): those cases check the structure (phantom, zero
    partner, no prediction undecided).  The 'one pixel lit' cases (chain_images) are the sharp ones: there the bound after three
    iterations is ~1e-5 of the lit pixels in float, and the error / bound of the log is what a small error would have to stay
    under."""
    lo, _ = nx_limits(L)
    nx = nx or lo + 2
    ny, frames, K = 3, 3, 3
    rng = np.random.default_rng(L + nx)
    dft, ar = fr.RowDFT.get(L), arith(lib, L, dtype)
    meas, norm, est0 = chain_images(rng, frames, ny, nx, dtype, kind)
    got, final = {}, {}
    for pairwise in (False, True):
        got[pairwise] = run_chain(lib, L, dtype, pairwise, ny, nx, frames, K, (meas, norm, est0))
        lay, ref = Layout(pairwise, frames, ny, nx), ChainRef(dft, ar, pairwise)
        MA, MB, exists = lay.split(meas)
        NA, NB, _ = lay.split(np.broadcast_to(norm, meas.shape))
        NB = NA if pairwise else np.where(exists, NB, 1)                      # (pair form: both parts are the same row of the normaliser)
        EA, EB, _ = lay.split(est0)                                           # the stored estimate ...
        dEA, dEB = np.zeros_like(EA), np.zeros_like(EB)
        ZA, ZB, dZA, dZB = EA, EB, dEA, dEB                                   # ... and what the spectrum carries
        key = ('chain', 'pair' if pairwise else 'frame', tname(dtype), L) + (('one pixel lit',) if kind == 'one_pixel' else ())
        for it in range(K):
            PA, PB, dPA, dPB = ref.round_trip(ZA, ZB, dZA, dZB)               # the prediction
            RA, dRA, ua = ar.ratio(MA, PA, dPA, True)
            RB, dRB, ub = ar.ratio(MB, PB, dPB, True)
            if not pairwise:                                                  # a row that does not exist stays zero
                RB, dRB, ub = np.where(exists, RB, 0), np.where(exists, dRB, 0), ub & exists
            assert not ua.any() and not ub.any(), ('a prediction within its bound of zero', it, pairwise, float(np.max(dPA / np.abs(PA))))
            VA, VB, dVA, dVB = ref.round_trip(RA, RB, dRA, dRB)
            FA, dFA = ar.factor(VA, dVA, NA, True)
            FB, dFB = ar.factor(VB, dVB, NB, True)
            # the phantom multiplies the STORED estimate of its real partner
            XB, dXB = (np.where(exists, EB, EA), np.where(exists, dEB, dEA)) if pairwise else (EB, dEB)
            ZA, dZA = ar.product(EA, FA, dFA)
            dZA = dZA + np.abs(FA + dFA) * dEA * (1 + ar.u)
            ZB, dZB = ar.product(XB, FB, dFB)
            dZB = dZB + np.abs(FB + dFB) * dXB * (1 + ar.u)
            if not pairwise:
                ZB, dZB = np.where(exists, ZB, 0), np.where(exists, dZB, 0)
            EA, dEA = ZA, dZA
            EB, dEB = np.where(exists, ZB, EB), np.where(exists, dZB, dEB)
            GA, GB, _ = lay.split(got[pairwise][it])
            fr.check(GA, EA, dEA, key)
            fr.check(np.where(exists, GB, 0), np.where(exists, EB, 0), np.where(exists, dEB, 0), key)
        final[pairwise] = (EA, dEA)
        rel = float(np.max(dEA / np.abs(EA)))
        fr.WORST.note(key + ('bound / estimate after 3 iterations',), rel)
        lit = np.abs(EA) >= 1
        if kind == 'one_pixel':
            assert lit.sum() == EA.shape[0]
            fr.WORST.note(key + ('bound / lit pixel after 3 iterations, x 1e6',), 1e6 * float(np.max(dEA[lit] / np.abs(EA[lit]))))
        assert rel < 1          # (what the chain needs of its bound: every prediction stays decided; the figure goes to the log)
    diff = np.abs(got[False][-1].astype(LD) - got[True][-1].astype(LD))
    assert float(diff.max()) <= float(final[False][1].max() + final[True][1].max())


# ------------------------------------------------------------------------------------------------ the outer column pass
def _settings(outer, L):
    v = (ctypes.c_int * 9)()
    assert outer.emu_outer_settings(L, v) == 0
    return dict(zip(('M', 'C', 'CW', 'C64', 'PARK', 'PARK64', 'TWLDS', 'TWLDS_SPLIT', 'SPLIT'), v))


def _outer_growth(dtype, V=1):
    """G of a column transform pair of length L = M x 576 through colconv_outer_body, counted as in fft_reference.py's
    docstring: each transform the (9,8,8) core's stages (compact inter-pass twiddles assumed: the larger count), the outer
    twiddle from its table (1 + sqrt 5) and the outer radix (8 = 4 x 2 at most); between them the multiplier (sqrt 5) and the
    sum over V views (V - 1).  A forward bin errs by at most G_f sum |column| and is at most (1 + G_f) sum |column| in modulus;
    the product with the multiplier p_k adds sqrt(5) u of it; the inverse passes every bin's error on with weight 1 and adds
    G_i sum_k |its inputs|.  So an output errs by at most (prod (1 + e u) - 1) * sum |column| * sum_k |p_k| <= expm1(c u) of it:
    the L1 norm of the multiplier, not L max |p_k| -- sharp when the column has one lit row and the multiplier's inverse
    transform is concentrated (an OTF).  The reference is numpy's float64 FFT, itself a radix 2 / 3 / 4 transform pair with
    rounded twiddles and fewer stages than the kernel's: it is granted the same c at 2^-53 (nothing in float, as much again in
    float64)."""
    core = fr.c_of((9, 8, 8))
    outer = float(1 + fr.SQRT5) + float(fr.E_RADIX_PRIME[4] + fr.TWC + fr.E_RADIX_PRIME[2])
    c = 2 * (core + outer) + float(fr.SQRT5) + (V - 1)
    return float(np.expm1(c * float(fr.unit(dtype))) + np.expm1(c * 2.0 ** -53))


def _outer_inputs(rng, n, ny, kx, lit_from):
    """[n][ny][kx] complex columns: images < lit_from dense (Gaussian), the others dark except ONE row per column (its own row per
    column and image, modulus 1-2), kept clear of the end so that a shifted multiplier leaves the peak among the rows < ny."""
    x = rng.standard_normal((n, ny, kx)) + 1j * rng.standard_normal((n, ny, kx))
    margin = min(48, ny // 4)
    for i in range(lit_from, n):
        x[i] = 0
        for j in range(kx):
            x[i, int(rng.integers(0, ny - margin)), j] = rng.uniform(1, 2) * np.exp(2j * np.pi * rng.random())
    return x, margin


def _otf_like(rng, kx, L, real, margin):
    """[kx][L] multiplier whose inverse transform is concentrated: a periodic Gaussian in the bin index (width L / 16 .. L / 8 and
    amplitude per column), real as the spectrum of a symmetric PSF is, or with the phase of a shift by s < margin rows.  A column
    with one lit row then comes back as one peak of modulus |x| sum_k |p_k| -- the scale of the bound."""
    k = np.arange(L)
    d = np.minimum(k, L - k)[None, :]
    sigma = L / rng.uniform(8, 16, size=(kx, 1))
    g = rng.uniform(0.5, 2, size=(kx, 1)) * np.exp(-0.5 * (d / sigma) ** 2)
    if real:
        return g + 0j
    s = rng.integers(0, margin, size=(kx, 1))
    return g * np.exp(-2j * np.pi * s * k[None, :] / L)


def _outer_check(got, ref, scale, G, key):
    got = got.astype(np.complex128)
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    r = float(np.max(np.abs(got - ref) / (G * scale[None, :])))
    fr.WORST.note(key, r)
    assert r <= 1, (key, r)
    return float(np.max(G * scale[None, :] / np.maximum(np.abs(ref).max(axis=0), 1e-300)[None, :]))


@pytest.mark.parametrize('dtype', DTYPES, ids=tname)
@pytest.mark.parametrize('L,ny,kx,real_psf', [(1152, 1024, 9, 1), (1152, 901, 3, 0), (2304, 2048, 17, 1), (2304, 2001, 3, 0),
                                               (4608, 4096, 2, 1), (4608, 3900, 9, 0)])
def test_outer_whole_pass_as_the_device_runs_it(libs, L, ny, kx, real_psf, dtype):
    """The whole outer pass exactly as launch_col launches it: f32 on CW columns with PARK parked values and TWLDS twiddle
    copies (2304: 16-column tiles, both tables in LDS), float64 on C64 columns with PARK64 parked values, the kernel with the row
    count at compile time where select_outer picks it (ny = 512 M, bit for bit the generic kernel's result) -- at the launcher's
    LDS byte count.  Against numpy's float64 FFT: IFFT_y(FFT_y(x zero padded) * psf_hat), rows < ny, per element within
    _outer_growth * sum |column| * sum |multiplier|.  Frame 0 is dense and view 0's multiplier Gaussian noise (every row and
    every bin carries weight; the bound is 0.2-1 % of a typical output there in float); frame 1 has one lit row per column and
    view 1's multiplier is OTF-like: the bound is ~1e-5 of the peak in float, 1e-14 in float64, and the log's error / bound is
    what a wrong twiddle copy or parking slot would have to stay under."""
    _, outer = libs
    st = _settings(outer, L)
    C = st['CW'] if dtype == np.float32 else st['C64']
    V, frames = 2, 2
    pitch = (kx + C - 1) // C * C if ny == 512 * st['M'] else (kx + 7) // 8 * 8
    rng = np.random.default_rng(L + ny)
    ct = ctype_of(dtype)
    x = np.full((frames, ny, pitch), np.nan + 1j * np.nan, dtype=ct)
    xs, margin = _outer_inputs(rng, frames, ny, kx, 1)
    x[:, :, :kx] = xs
    if pitch % C == 0:
        x[:, :, kx:] = 0          # (pad columns travel with the tile in the compile-time-size kernel: loaded, never used)
    noise = rng.standard_normal((kx, L)) + (0 if real_psf else 1j) * rng.standard_normal((kx, L))
    ph = np.stack([noise, _otf_like(rng, kx, L, real_psf, margin)]).astype(ct)
    psf_arg = np.ascontiguousarray(ph.real.astype(dtype) if real_psf else ph)
    f = getattr(outer, 'emu_outer_whole_' + tname(dtype))
    outs = []
    for n512 in ((1, 0) if ny == 512 * st['M'] else (1,)):
        out, buf = guarded((frames * V, ny, pitch), ct, np.nan + 1j * np.nan)
        outer.emu_outer_set_n512(n512)
        try:
            assert f(L, _p(x), _p(out), _p(psf_arg), real_psf, ny, kx, pitch, V, frames, 1, 0) == 0
        finally:
            outer.emu_outer_set_n512(1)
        assert guards_intact(buf)
        outs.append(out[:, :, :kx].copy())
    if len(outs) == 2:
        assert np.array_equal(outs[0], outs[1])
    full = np.zeros((frames, L, kx), dtype=np.complex128)
    full[:, :ny] = x[:, :, :kx]
    spec = np.fft.fft(full, axis=1)
    G = _outer_growth(dtype)
    for fi in range(frames):
        for v in range(V):
            phd = ph[v].astype(np.complex128)
            ref = np.fft.ifft(spec[fi] * phd.T, axis=0)[:ny] * L
            scale = np.abs(full[fi]).sum(axis=0) * np.abs(phd).sum(axis=1)                 # L1 of the column x L1 of the multiplier
            what = ('dense' if fi == 0 else 'one row lit') + (', noise' if v == 0 else ', OTF')
            rel = _outer_check(outs[0][fi * V + v], ref, scale, G, ('outer whole', tname(dtype), L, what))
            if fi == 1 and v == 1:
                fr.WORST.note(('outer whole', tname(dtype), L, what, 'bound / peak x 1e6'), 1e6 * rel)


@pytest.mark.parametrize('L,ny,kx,real_psf,sum_views', [(2304, 2048, 9, 1, 1), (2304, 2001, 3, 0, 0), (4608, 3000, 5, 1, 1),
                                                         (1152, 1024, 8, 0, 1), (1152, 437, 8, 1, 0)])
def test_outer_split_pass_as_the_device_runs_it(libs, L, ny, kx, real_psf, sum_views):
    """COL_SPLIT_FWD then COL_SPLIT_INV / COL_SPLIT_INV_SUM in float on C columns with TWLDS_SPLIT twiddle copies (1152: 2 at
    M = 2), at the launcher's LDS byte count; the parked spectra start as NaN.  Frame 0 dense; frame 1 one lit row per column
    and the last view's multiplier OTF-like (where the views are summed, frame 1 is dark in the other views, so that the sum's
    bound is the lit view's alone): the sharp case, as in the whole pass."""
    _, outer = libs
    st = _settings(outer, L)
    V, frames, C = 3, 2, st['C']
    pitch = (kx + 7) // 8 * 8
    rng = np.random.default_rng(L + ny + sum_views)
    n_in = frames * V if sum_views else frames
    n_out = frames if sum_views else frames * V
    x = np.zeros((n_in, ny, pitch), dtype=np.complex64)
    xs, margin = _outer_inputs(rng, n_in, ny, kx, n_in // 2)
    if sum_views:
        xs[V:2 * V - 1] = 0
    x[:, :, :kx] = xs
    ph = np.stack([rng.standard_normal((kx, L)) + (0 if real_psf else 1j) * rng.standard_normal((kx, L)) for _ in range(V - 1)] +
                  [_otf_like(rng, kx, L, real_psf, margin)]).astype(np.complex64)
    psf_arg = np.ascontiguousarray(ph.real.astype(np.float32) if real_psf else ph)
    out, buf = guarded((n_out, ny, pitch), np.complex64, np.nan + 1j * np.nan)
    assert outer.emu_outer_split_f32(L, _p(x), _p(out), _p(psf_arg), real_psf, ny, kx, pitch, V, frames, sum_views) == 0
    assert guards_intact(buf)
    full = np.zeros((n_in, L, kx), dtype=np.complex128)
    full[:, :ny] = x[:, :, :kx]
    spec = np.fft.fft(full, axis=1)
    phd = ph.astype(np.complex128)
    l1 = np.abs(phd).sum(axis=2)                                                             # [V][kx]
    G = _outer_growth(np.float32, V if sum_views else 1)
    for fi in range(frames):
        name = 'dense' if fi == 0 else 'one row lit'
        if sum_views:
            ref = np.fft.ifft(sum(spec[fi * V + v] * phd[v].T for v in range(V)), axis=0)[:ny] * L
            scale = sum(np.abs(full[fi * V + v]).sum(axis=0) * l1[v] for v in range(V))
            triples = [(out[fi][:, :kx], ref, scale, name + ', summed')]
        else:
            triples = [(out[fi * V + v][:, :kx], np.fft.ifft(spec[fi] * phd[v].T, axis=0)[:ny] * L,
                        np.abs(full[fi]).sum(axis=0) * l1[v], name + (', OTF' if v == V - 1 else ', noise')) for v in range(V)]
        for got, ref, scale, what in triples:
            _outer_check(got, ref, scale, G, ('outer split', 'f32', L, what))


# ------------------------------------------------------------------------------------------------ guard against drift
SHORT_LENGTHS = (64, 192, 256, 576)
WALK_OF = {'k_colconv': 'for_each_colconv<', 'k_colconv_outer': 'for_each_outer<', 'k_rowpass': 'for_each_rowpass<', 'k_rowpair': 'for_each_rowpair<'}


def _table(fn, *args):
    buf = ctypes.create_string_buffer(1 << 16)
    n = fn(*args, buf, len(buf))
    assert 0 < n < len(buf)
    return set(buf.value.decode().split('\n')) - {''}


def launchable(rows, L, esize):
    """The device's variants for a length and element size: the rows of csrc/kernel_variants.hpp that exist with the device's
    compile-time sizes, in the column family launch_col takes -- printed by the walk the launchers and prepare() take."""
    return _table(rows.emu_device_table, L, esize)


def test_every_launchable_instantiation_has_an_emulated_counterpart(libs, emu):
    """What fft_kernels.hip can launch (the shared list with the device's sizes) against what the emulators can run (the same
    list with theirs): a launchable instantiation with no emulated counterpart fails.  At the long lengths the launchable set
    must be, name for name, tests/golden/launchable_long_kernels.txt -- what the launch ladders gave before the list replaced
    them (parsed from their rl_launch( sites at that commit; the allow_lds( sites gave the same set)."""
    rows, outer = libs
    can_run = _table(rows.emu_long_table)
    can_run_outer = {re.sub(r' LDS=\d+', '', s) for s in _table(outer.emu_outer_table)}
    golden = set(open(os.path.join(ROOT, 'tests', 'golden', 'launchable_long_kernels.txt')).read().split('\n')) - {''}
    got = set()
    for L in LENGTHS:
        want_outer = set()
        for esize in (4, 8):
            assert rows.emu_long_q(L, esize, 0) == 1 and rows.emu_long_q(L, esize, 1) == 1
            have = launchable(rows, L, esize)
            assert not [w for w in have if w.startswith('k_colconv ')], 'the long lengths launch the outer column kernels in both types'
            want = {w for w in have if w.startswith('k_row')}
            assert len([w for w in want if w.startswith('k_rowpass')]) == 8 and len(want) >= 11, sorted(want)
            missing = want - can_run
            assert not missing, 'launchable, not emulated: %s' % sorted(missing)
            want_outer |= have - want
            got |= have
        assert len(want_outer) == 18, sorted(want_outer)
        assert not (want_outer - can_run_outer), sorted(want_outer - can_run_outer)
    assert got == golden, (sorted(got - golden), sorted(golden - got))
    assert 'k_rowpair L=2304 T=f32 MODE=2 NXC=2048 SUBC=1' in can_run
    # The short lengths (tests/emu/emu.cpp).  A variant with a compile-time image size (NYC / NXC: on the device 512, at L = 576
    # in float) runs in the emulator at a size of its own, and with it at the length and in the types that host that size there
    # (192 at L = 256, float and double): for such a row the size and, with it, L and T may differ.  No other field may, and a
    # row without a compile-time size must match in every field.
    can_run_short = _table(emu.emu_table)
    sized = lambda s: re.sub(r'(NYC|NXC)=[1-9]\d*', r'\1=N', re.sub(r' L=\d+ T=f\d+', '', s))
    can_run_sized = {sized(s) for s in can_run_short if re.search(r'(NYC|NXC)=[1-9]', s)}
    for L in SHORT_LENGTHS:
        for esize in (4, 8):
            want = launchable(rows, L, esize)
            assert len([w for w in want if w.startswith('k_rowpass')]) >= 8 and not [w for w in want if 'outer' in w], sorted(want)
            missing = {w for w in want if not (sized(w) in can_run_sized if re.search(r'(NYC|NXC)=[1-9]', w) else w in can_run_short)}
            assert not missing, 'launchable, not emulated: %s' % sorted(missing)
    assert len(launchable(rows, 576, 4)) == 13 + 10 + 5 and len(launchable(rows, 576, 8)) == 6 + 8 + 3


def test_every_launchable_row_kernel_may_use_its_lds():
    """A row kernel of a long length needs more than the default 64 KB of dynamic LDS in float64 at 4608 (4626 slots x 16 bytes):
    every instantiation fft_kernels.hip can launch must be among those prepare() raises the limit of.  (The PRESUM update,
    launched for multi-view `ratio - 1` plans, was once missing from a hand-written prepare list: a float64 4096^2 multi-view
    plan with RLSTED_SUB_ONE=1 could not launch it.)  It holds by construction for every kernel of every length: a launch and
    prepare() walk the same list of csrc/kernel_variants.hpp, and no rl_launch( or allow_lds( of fft_kernels.hip names one of
    the four kernel templates outside such a walk, where the template arguments are the row's."""
    text = re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, 'fft_kernels.hip')).read())
    sites = {'rl_launch': [], 'allow_lds': []}
    for m in re.finditer(r'\b(rl_launch|allow_lds)\((k_\w+)<([^;]*?)>,', text):
        assert m.group(2) in WALK_OF, m.group(0)
        before = text[:m.start()]
        walk = before.rfind(WALK_OF[m.group(2)])
        assert walk >= 0 and '});' not in before[walk:] and re.match(r'for_each_\w+<[^(]*>\(\[&\]\(auto v\) \{', before[walk:]), \
            'outside a walk over the variant list: %s' % m.group(0)
        args = [a.strip() for a in m.group(3).split(',')]
        assert all(a in ('RL_CFG_L', 'C', 'Q', 'QP', 'T') or a.startswith('V::') for a in args), 'hand-written template arguments: %s' % m.group(0)
        sites[m.group(1)].append((m.group(2), tuple('Q' if a == 'QP' else a for a in args)))
    assert sorted(sites['rl_launch']) == sorted(sites['allow_lds']) and sorted(k for k, _ in sites['rl_launch']) == sorted(WALK_OF)
    assert len(re.findall(r'\b(?:rl_launch|allow_lds)\(', text)) == 8 + 2       # those, and the two definitions


def test_outer_lds_is_the_launchers(libs):
    """The emulated outer pass allocates what outer_lds.hpp computes -- the functions launch_col and prepare call -- and the
    launcher has no second copy of the arithmetic."""
    _, outer = libs
    text = open(os.path.join(CSRC, 'fft_kernels.hip')).read()
    assert '#include "outer_lds.hpp"' in text
    assert not re.search(r'constexpr size_t outer_\w+\(', text), 'fft_kernels.hip defines an LDS size function of its own again'
    assert 'LdsSlots<typename OC::Core>' not in text, 'fft_kernels.hip computes an outer LDS size inline again'
    for L in LENGTHS:
        st = _settings(outer, L)
        lds = {re.sub(r' LDS=\d+', '', s): int(re.search(r'LDS=(\d+)', s).group(1)) for s in _table(outer.emu_outer_table) if 'L=%d ' % L in s}
        assert max(lds.values()) <= 160 * 1024
        whole32 = [v for k, v in lds.items() if 'MODE=0 T=f32' in k]
        assert len(set(whole32)) == 1 and whole32[0] % 8 == 0
        assert st['TWLDS'] == 2 and (L != 1152 or st['TWLDS_SPLIT'] == 2)
