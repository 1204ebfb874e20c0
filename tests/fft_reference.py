"""What the row kernels of rescan_line_sted_amd/csrc/conv_kernels.hpp compute, written down plainly: direct DFT sums in
numpy.longdouble (no FFT, nothing shared with fft_core.hpp), the pointwise stages restated from rowpass_body / rowpair_body,
and DERIVED per-element error bounds of the kernels' own arithmetic.  Used by tests/test_long_rows_cpu.py (host emulation of
the long lengths) and by the plan-level GPU counterpart in tests/test_gpu_parity.py.

The operations.  w = exp(-2 pi i / L); all transforms unnormalised (the PSF spectrum carries the 1 / (Ly Lx)).

  per-frame bodies (rowpass_body): rows 2p, 2p+1 of an image ride through ONE complex transform, z = row(2p) + i row(2p+1),
  zero padded from nx to L (a missing row 2p+1 -- ny odd -- is zero).  Spectra are stored as half spectra [ny][pitch],
  columns 0 .. L/2 valid:
      forward   Z[k] = sum_j z[j] w^(jk);  row 2p gets (Z[k] + conj Z[L-k]) / 2, row 2p+1 gets (Z[k] - conj Z[L-k]) / 2i
      inverse   Z[k] = A[k] + i B[k] (k <= L/2),  Z[L-k] = conj A[k] + i conj B[k] (0 < k < L/2);  z[i] = sum_k Z[k] w^(-ik), i < nx
  ROW_FWD     spec_out[f] = forward(src[f] * scale[f])
  ROW_INV     dst = max(Re / Im z, 0)
  ROW_RATIO   v = inverse(spec_in[img % in_mod]);  r = meas / v  (sub_one: (meas - v) / v);  a pixel with v <= 0 (or NaN) is
              NEUTRAL: r = 1 (sub_one: 0);  spec_out = forward(r)
  ROW_UPDATE  plain:   est *= (sum_v max(v_v, 0)) / norm
              sub_one: est *= max(1 + (sum_v v_v) / norm, 0);  V > 1: the views' SPECTRA are summed, one inverse (PRESUM)
              spec_out = forward(new est)
  ROW_ADJ     dst = sum_v max(v_v, 0)  (/ norm when given)
  pair bodies (rowpair_body): frames 2p, 2p+1 are the real / imaginary part of one complex image, spectra are whole complex
  rows [ny][pitch >= L]:  S[k] = Fa[k] + i Fb[k], and on the mirrored bin S[L-k] = conj Fa[k] + i conj Fb[k].  An odd frame
  count: the last pair's imaginary part is a phantom copy of its real part's frame (read from that frame, never stored).

Error bounds.  u = 2^-24 / 2^-53.  Every computed intermediate of a transform is a linear combination of the inputs; following
one input x_j to one output bin through the passes, each operation on the way perturbs its coefficient (modulus 1 in exact
arithmetic) relatively:
    complex add / subtract                      u          (componentwise rounding)
    multiply by a real constant rounded to T    2 u        (the constant's rounding + the product's); by 1/2: exact
    complex x complex                           sqrt(5) u  (Brent, Percival, Zimmermann, Math. Comp. 76 (2007); fused forms less)
    rotation by +-i, negation                   exact
so a transform's output bin errs by at most  G * sum_j |x_j|,  G = prod (1 + e u) - 1 over the stages of the path, i.e.
G = c u to first order with c the sum of the stages' e.  Counted from fft_core.hpp dft<R> and pass_compute:
    radix 2   e = 1          one add
    radix 4   e = 2          two levels of adds
    radix 3   e = 4.964      output 1 from input 1: -1/2 through (v1+v2), (v0 - t/2), the final add: 3 roundings x 0.5;
                             +-i sqrt(3)/2 through (v1-v2), the rounded constant, the final add: 4 roundings x 0.866
    radix R1 x R2 (Cooley-Tukey inside a pass: 8 = 4x2, 16 = 4x4, 9 = 3x3):  e(R1) + TWC + e(R2), TWC = 1 + sqrt(5): the
              constant twiddle, both components rounded to T (modulus error u) and one complex multiply
    inter-pass twiddle, passes 1 .. NP-1, compact form (every radix of the long lists is > 4, every long length uses it):
              the entry is the product of two table entries (u each, the table's own rounding from the long-double value) --
              2 + sqrt(5) -- and multiplies the data -- + sqrt(5):  TWP = 2 + 2 sqrt(5)
    c = sum_p e(R_p) + (NP - 1) TWP:   (8,9,16) 39.6    (9,16,16) 40.6    (8,8,8,9) 51.3     -- the inverse runs the same stages
The epilogues propagate: packing / splitting a half spectrum one more add (u); clamps are 1-Lipschitz; a sum of V values
gamma(V - 1) on the absolute sum; quotient n / c with |dn| and |dc| <= e < c:  (dn + |n/c| e) / (c - e), then the division's own
rounding DIV u (1 on the host; 3 for the device's float a * rcp(b), rcp within 1 ulp); a product one more u.  A prediction whose
reference value lies within its bound of zero may go either way through the neutral-pixel rule: such a case decides nothing and
the case generators do not produce it (the checks assert that).  The error of a transform's INPUT pixels (the pointwise stage's
bound) passes to every bin with weight 1: + sum_j dz_j.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = LD('3.14159265358979323846264338327950288')
SQRT5 = np.sqrt(LD(5))
ROW_FWD, ROW_INV, ROW_RATIO, ROW_UPDATE, ROW_ADJ = range(5)

E_RADIX_PRIME = {2: LD(1), 4: LD(2), 3: LD(3) * LD(0.5) + LD(4) * np.sqrt(LD(3)) / 2}
TWC = 1 + SQRT5
TWP = 2 + 2 * SQRT5


def unit(dtype):
    return LD(2.0) ** (-24 if np.dtype(dtype) == np.float32 else -53)


def gamma(k, u):
    return k * u / (1 - k * u)


def _split(R):            # fft_core.hpp radix_split, restated
    R1 = 4 if (R % 4 == 0 and R > 4) else (2 if R % 2 == 0 else (3 if R % 3 == 0 else 5))
    return R1, R // R1


def stages(radices):
    """The e of every rounding stage on an input's way through a transform with this radix list (compact inter-pass twiddles)."""
    out = []

    def radix(R):
        if R in E_RADIX_PRIME:
            out.append(E_RADIX_PRIME[R])
            return
        R1, R2 = _split(R)
        radix(R1)
        out.append(TWC)
        radix(R2)
    for p, R in enumerate(radices):
        assert R > 4, 'the direct-table form of the twiddles is not counted here'
        if p > 0:
            out.append(TWP)
        radix(R)
    return out


def growth(radices, dtype):
    """G of the docstring: a bin errs by at most G * sum |inputs|."""
    u = unit(dtype)
    g = LD(1)
    for e in stages(radices):
        g = g * (1 + e * u)
    return g - 1


def c_of(radices):
    return float(sum(stages(radices)))


# ------------------------------------------------------------------------------------------------ the transforms
_POOL = ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1)))


def _sums(sub, a, b, axis):
    """np.einsum(sub, a, b) with b cut along `axis` (an axis of the OUTPUT: every output element is the same sum, term for term)
    into one piece per thread.  numpy's long-double loops run on one core and release the GIL; the sums are most of the time of
    the tests that use this module."""
    n, w = b.shape[axis], _POOL._max_workers
    cuts = [slice(i * n // w, (i + 1) * n // w) for i in range(w) if (i + 1) * n // w > i * n // w]
    pick = (lambda c: b[c]) if axis == 0 else (lambda c: b[:, c])
    return np.concatenate(list(_POOL.map(lambda c: np.einsum(sub, a, pick(c)), cuts)), axis=1)


class RowDFT:
    """cos / sin of 2 pi j k / L for k <= L/2, j < L, from long-double cos / sin of arguments reduced to [0, pi/4]."""
    _cache = {}

    @classmethod
    def get(cls, L):
        if L not in cls._cache:
            cls._cache[L] = cls(L)
        return cls._cache[L]

    def __init__(self, L):
        assert L % 8 == 0
        self.L, self.H = L, L // 2
        p = 8 * np.arange(L, dtype=np.int64)                 # angle = pi p / (4 L)
        ss = np.where(p > 4 * L, -1, 1)
        p = np.where(p > 4 * L, 8 * L - p, p)                # sin odd, cos even about pi
        sc = np.where(p > 2 * L, -1, 1)
        p = np.where(p > 2 * L, 4 * L - p, p)                # about pi / 2
        swap = p > L
        p = np.where(swap, 2 * L - p, p)                     # about pi / 4
        a = PI * p.astype(LD) / LD(4 * L)
        c, s = np.cos(a), np.sin(a)
        tc, ts = np.where(swap, s, c) * sc, np.where(swap, c, s) * ss
        m = (np.arange(self.H + 1, dtype=np.int64)[:, None] * np.arange(L, dtype=np.int64)[None, :]) % L
        self.C, self.S = tc[m], ts[m]                        # [H + 1][L]

    def forward_real(self, x):
        """x [rows][n <= L] real -> sum_j x_j w^(jk), k <= L/2, complex [rows][L/2 + 1]."""
        x = np.asarray(x, dtype=LD)
        n = x.shape[1]
        out = np.empty((x.shape[0], self.H + 1), dtype=CLD)
        out.real = _sums('rj,kj->rk', x, self.C[:, :n], 0)           # (einsum: numpy's matmul is slow on long doubles)
        out.imag = -_sums('rj,kj->rk', x, self.S[:, :n], 0)
        return out

    def forward_pair(self, a, b):
        """The whole complex spectrum [rows][L] of a + i b (a, b real [rows][n]): the split on mirrored bins."""
        Fa, Fb = self.forward_real(a), self.forward_real(b)
        S = np.empty((Fa.shape[0], self.L), dtype=CLD)
        S[:, :self.H + 1] = Fa + 1j * Fb
        S[:, self.H + 1:] = (np.conj(Fa) + 1j * np.conj(Fb))[:, self.H - 1:0:-1]
        return S

    def inverse(self, S, n):
        """S [rows][L] complex -> z_i = sum_k S_k w^(-ik), i < n, complex [rows][n]."""
        S = np.asarray(S, dtype=CLD)
        H = self.H
        lo, hi = S[:, 1:H], S[:, :H:-1]                                    # bins k and L - k, k = 1 .. H-1
        P, M = lo + hi, lo - hi
        Ck, Sk = self.C[1:H, :n], self.S[1:H, :n]
        z = np.empty((S.shape[0], n), dtype=CLD)
        alt = np.where(np.arange(n) % 2 == 0, LD(1), LD(-1))
        dot = lambda a, b: _sums('rk,kn->rn', np.ascontiguousarray(a), b, 1)
        z.real = S[:, :1].real + S[:, H:H + 1].real * alt + dot(P.real, Ck) - dot(M.imag, Sk)
        z.imag = S[:, :1].imag + S[:, H:H + 1].imag * alt + dot(P.imag, Ck) + dot(M.real, Sk)
        return z

    def pack_half(self, A, B):
        """The Hermitian-free row of two half spectra (columns 0 .. L/2 of A and B are read): [rows][L]."""
        H = self.H
        A = np.asarray(A, dtype=CLD)[:, :H + 1]
        B = np.zeros_like(A) if B is None else np.asarray(B, dtype=CLD)[:, :H + 1]
        Z = np.empty((A.shape[0], self.L), dtype=CLD)
        Z[:, :H + 1] = A + 1j * B
        Z[:, H + 1:] = (np.conj(A) + 1j * np.conj(B))[:, H - 1:0:-1]
        return Z


# ------------------------------------------------------------------------------------------------ bounds of the pieces
class Arith:
    """The arithmetic whose error is bounded: element type, radix list of the geometry, DIV (see the docstring)."""

    def __init__(self, dtype, radices, div=1):
        self.dtype, self.u, self.G, self.div = np.dtype(dtype), unit(dtype), growth(radices, dtype), LD(div)

    def transform(self, abs_in_sum, d_in_sum=0):
        """bound of every output of a transform whose inputs have absolute sum abs_in_sum and errors summing to d_in_sum"""
        return self.G * (abs_in_sum + d_in_sum) + d_in_sum

    def ratio(self, meas, c, e, sub_one):
        """rl_ratio: (reference, bound, undecided mask)."""
        u = self.u
        meas, c, e = np.asarray(meas, dtype=LD), np.asarray(c, dtype=LD), np.broadcast_to(np.asarray(e, dtype=LD), np.shape(c))
        nan = np.isnan(c)                                 # a NaN prediction is neutral whatever its bound (`!(c > 0)` on the device)
        e = np.where(nan, 0, e)
        pos = c > e
        neutral = (c < -e) | ((c == 0) & (e == 0)) | nan
        cs = np.where(pos, c, 1)
        n = meas - c if sub_one else meas
        dn = (e + u * (np.abs(n) + e)) if sub_one else np.zeros_like(c)
        q = n / cs
        dq = (dn + np.abs(q) * e) / np.where(pos, c - e, 1)
        dq = dq + self.div * u * (np.abs(q) + dq)
        r = np.where(pos, q, LD(0) if sub_one else LD(1))
        return r, np.where(pos, dq, 0), ~(pos | neutral)

    def factor(self, a, da, norm, sub_one):
        """rl_update_factor on a value a known to da."""
        u = self.u
        f = a / norm
        df = da / norm + self.div * u * (np.abs(f) + da / norm)
        if not sub_one:
            return f, df
        g = 1 + f
        return np.maximum(g, 0), df + u * (np.abs(g) + df)

    def product(self, x, f, df):
        r = x * f
        return r, np.abs(x) * df + self.u * (np.abs(x) * (np.abs(f) + df))


def rows_to_complex(img, nx):
    """image [ny][nx] -> z [pairs][nx] = row 2p + i row 2p+1 (a missing last partner is zero)"""
    img = np.asarray(img, dtype=LD)
    ny = img.shape[0]
    z = np.zeros(((ny + 1) // 2, nx), dtype=CLD)
    z.real = img[0::2]
    z.imag[:ny // 2] = img[1::2]
    return z


def complex_to_rows(z, ny):
    out = np.empty((ny, z.shape[1]), dtype=LD)
    out[0::2] = z.real
    out[1::2] = z.imag[:ny // 2]
    return out


def frame_forward(dft, ar, img, d_img=None):
    """Half spectra [ny][L/2 + 1] of an image's rows through the two-rows-per-transform forward pass, and their bound [ny][1].
    d_img: bound of the error the image's pixels already carry."""
    ny, nx = np.shape(img)
    z = rows_to_complex(img, nx)
    F = dft.forward_real(np.asarray(img, dtype=LD))
    dz = np.zeros(z.shape, dtype=LD) if d_img is None else np.abs(rows_to_complex(d_img, nx))
    B = ar.transform(np.abs(z).sum(axis=1), dz.sum(axis=1))
    B = B + ar.u * (np.abs(z).sum(axis=1) + B)                       # the split's add
    return F, np.repeat(B, 2)[:ny, None]


def frame_inverse(dft, ar, specs, ny, nx):
    """specs: list of V half-spectrum images [ny][>= L/2 + 1] that are SUMMED on their way in (V = 1: plain).  Returns the
    rows [ny][nx] of the inverse pass and their bound [ny][1]."""
    V = len(specs)
    pairs = (ny + 1) // 2
    Z = np.zeros((pairs, dft.L), dtype=CLD)
    absZ = np.zeros(pairs, dtype=LD)
    for s in specs:
        s = np.asarray(s)
        A, B = s[0::2], s[1::2]
        if ny % 2:
            B = np.concatenate([B, np.zeros_like(A[:1])])
        Zv = dft.pack_half(A, B)
        Z += Zv
        absZ += np.abs(Zv).sum(axis=1)
    z = dft.inverse(Z, nx)
    g = (1 + ar.G) * (1 + ar.u) ** V - 1                              # V - 1 adds of the view sum, the packing's add, the passes
    return complex_to_rows(z, ny), np.repeat(g * absZ, 2)[:ny, None]


def pair_forward(dft, ar, a, b, da=None, db=None):
    """Whole complex spectrum [ny][L] of frame a + i frame b and its bound [ny][1]."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    S = dft.forward_pair(a, b)
    dz = 0 if da is None else np.hypot(da, db).sum(axis=1)
    return S, ar.transform(np.hypot(a, b).sum(axis=1), dz)[:, None]


def pair_inverse(dft, ar, S, nx):
    """S [ny][>= L] complex -> (Re z, Im z) [ny][nx] and their bound [ny][1]."""
    S = np.asarray(S, dtype=CLD)[:, :dft.L]
    z = dft.inverse(S, nx)
    return z.real, z.imag, ar.transform(np.abs(S).sum(axis=1))[:, None]


# ------------------------------------------------------------------------------------------------ the edge table
EDGES = ('widest', 'narrowest', 'one pixel wide', 'one column', 'one odd row', 'odd', 'not a multiple of 4', 'a multiple of 16 only',
         'zero rows', 'one pixel lit', 'one pixel lit, widest', 'negative measurement')


def edge_rows(lo, hi):
    """name -> (ny, nx, kind) for row lengths lo .. hi that select one transform length (the caller takes lo and hi from the
    plan's size rule): nx at the largest and the smallest value, 1, odd, not a multiple of 64 / 16 / 4; ny = 1 and odd; a row
    pair of zeros; rows dark except one pixel; negative measurement pixels.  Shared by the CPU module (row bodies) and its
    plan-level GPU counterpart."""
    odd = lo + (hi - lo) // 2 | 1                      # odd, in the upper half
    rows = [(2, hi, 'random'), (3, lo, 'random'), (1, 1, 'random'), (3, 1, 'random'), (1, odd, 'random'), (3, odd - 36, 'random'),
            (2, hi - 66, 'random'),                    # even, not a multiple of 4
            (3, hi - 48, 'random'),                    # a multiple of 16, not of 64
            (5, lo + 3, 'zero_row'), (3, odd, 'one_pixel'), (2, hi, 'one_pixel'), (3, lo + 8, 'negative')]
    return dict(zip(EDGES, rows))


# ------------------------------------------------------------------------------------------------ worst ratios
class Worst:
    def __init__(self):
        self.r = {}

    def note(self, key, ratio):
        self.r[key] = max(self.r.get(key, 0.0), float(ratio))

    def lines(self):
        return ['worst error / bound  %-40s %.3f' % (' '.join(str(k) for k in key), v) for key, v in sorted(self.r.items())]


WORST = Worst()


def check(got, ref, bound, key, ctx=''):
    """|got - ref| <= bound elementwise (moduli for complex values); a zero bound demands the exact value."""
    got = np.asarray(got)
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), ('not finite', key, ctx)
    err = np.abs(got.astype(CLD if np.iscomplexobj(got) else LD) - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    exact = bound == 0
    assert not np.any(err[exact] != 0), ('a value whose every term is zero is not exact', key, ctx)
    r = float(np.max(err[~exact] / bound[~exact])) if np.any(~exact) else 0.0
    WORST.note(key, r)
    assert r <= 1, (key, ctx, 'error / bound %.3f' % r)
    return r


# ------------------------------------------------------------------------------------------------ plan level (the GPU counterpart)
def conv_same_x(x, taps):
    """'same' convolution of every row of x [..][nx] with a one-row PSF `taps` [px], zero outside the image (the reference's
    fftconvolve(x, p, 'same')): out[j] = sum_b x[j + cx - b] p[b], cx = (px - 1) // 2.  Term by term in long double."""
    x, taps = np.asarray(x, dtype=LD), np.asarray(taps, dtype=LD)
    nx, px = x.shape[-1], len(taps)
    cx = (px - 1) // 2
    pad = np.zeros(x.shape[:-1] + (nx + px - 1,), dtype=LD)
    pad[..., px - 1 - cx:px - 1 - cx + nx] = x
    out = np.zeros(x.shape, dtype=LD)
    for b in range(px):
        out += pad[..., px - 1 - b:px - 1 - b + nx] * taps[b]
    return out


def plan_conv_growth(row_radices, col_radices, dtype, ntaps):
    """K such that one FFT convolution of the plan (row forward, column forward, multiplier, column inverse, row inverse)
    errs per pixel by at most K * (L1 norm of everything that shares the transforms) * (sum |PSF|).  With A the growth of a
    2-D transform (row passes, the split's / packing's add, column passes) every forward bin is within A X1 of its value and at
    most (1 + A) X1 in modulus; the multiplier, |psf_hat| <= h1 / N per bin over N = Ly Lx bins, is known to mu = u (its rounding
    to the element type) + gamma(ntaps + 4) 2^-53 (its float64 direct sum) and the product adds sqrt(5) u; the inverse passes
    every bin's error to a pixel with weight 1 -- N bins of h1 / N each -- and adds A times the sum of the bins' moduli."""
    u = unit(dtype)
    A = (1 + growth(row_radices, dtype)) * (1 + u) * (1 + growth(col_radices, dtype)) - 1
    mu = u + gamma(ntaps + 4, LD(2.0) ** -53) + SQRT5 * u
    d_bins = A + mu * (1 + A)
    return d_bins + A * (1 + A + d_bins)
