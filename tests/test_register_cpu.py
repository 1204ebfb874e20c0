"""Registration without a GPU (include/rlsted.h rl_register_sums, rl_shift_images; rescan_line_sted_amd/registration.py): the bodies
of the kernels emulated thread by thread (tests/emu/register_emu.cpp) against the twin (tests/register_reference.py) -- the sums
within the derived bound and bit-identical across runs and pair orderings, the shift against scipy; the same bodies as a stand-alone
program under the address and undefined-behaviour sanitizers; the twin against the analytic truth, which fixes what "accurate"
means; at_limit, flat, ties; the argument checks; the device build's private segments; and the wrappers on a numpy stand-in for the
device.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ingest_reference as ir
import register_reference as rr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'register_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('register_kernels.hpp', 'ingest_kernels.hpp', 'tile_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
FLOATS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
# the twin's worst error on the committed scenes (SCENES x DISPLACEMENTS, R = 6, noise-free), measured; asserted at twice these
TWIN_ERROR = {('same', 0): 0.057, ('same', 1): 0.0096, ('blur', 0): 0.056, ('blur', 1): 0.0211}
BLUR = (1.5, 0.7)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libregister_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_register_sums.argtypes = [vp, i, vp, vp, i, vp, i, i, i, i, i, vp, vp, vp]
    lib.emu_shift_images.argtypes = [vp, i, i, i, i, vp, i, d, vp, i, vp]
    return lib


def emu_sums(emu, a, a_off, b, b_off, ny, nx, R, M):
    W = 2 * R + 1
    n = len(a_off)
    S, A, geom = np.full((n, W * W, 3), np.nan), np.full((n, 2), np.nan), np.zeros(6, dtype=np.intc)
    ao, bo = np.asarray(a_off, dtype=np.int64), np.asarray(b_off, dtype=np.int64)
    assert emu.emu_register_sums(_p(a), FLOATS[a.dtype], _p(ao), _p(b), FLOATS[b.dtype], _p(bo), n, ny, nx, R, M, _p(S), _p(A), _p(geom)) == 0
    return S, A, geom


def emu_shift(emu, src, shifts, order, floor, dst_dtype, guard=False):
    n, ny, nx = src.shape
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    whole = np.full(src.size + 16, 7, dtype=dst_dtype)
    dst = whole[8:8 + src.size]
    stats = np.full((n, 2), np.nan)
    assert emu.emu_shift_images(_p(src), FLOATS[src.dtype], n, ny, nx, _p(sh), order, -np.inf if floor is None else floor, _p(dst),
                                FLOATS[np.dtype(dst_dtype)], _p(stats)) == 0
    assert np.all(whole[:8] == 7) and np.all(whole[8 + src.size:] == 7)
    return dst.reshape(src.shape).copy(), stats


# ---- the sums ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ny,nx,R,M', [(37, 53, 2, 2), (40, 56, 1, 1), (40, 56, 3, 3), (40, 56, 6, 6), (72, 48, 6, 8), (41, 45, 9, 11),
                                       (73, 74, 32, 32)])
def test_emulated_sums_are_within_the_bound_of_the_twin(emu, ny, nx, R, M):
    """Five pairs over three f32 references and five f64 moving images at non-trivial offsets (shared references), and the dtypes
    the other way round: every sum within gamma_N sum |t| of the long double twin; a second run and a reversed pair order give the
    same bits; a pair computed alone gives the same bits as in the call of five."""
    rng = np.random.default_rng(ny * 100 + R)
    n_pix = ny * nx
    for ta, tb in ((np.float32, np.float64), (np.float64, np.float32)):
        a = (rng.random(3 * n_pix + 5) * 100.0).astype(ta)
        b = (rng.random(5 * n_pix + 3) * 100.0).astype(tb)
        a_off = [5, n_pix + 5, 5, 2 * n_pix + 5, n_pix + 5]
        b_off = [3 + k * n_pix for k in (4, 0, 2, 1, 3)]
        S, A, geom = emu_sums(emu, a, a_off, b, b_off, ny, nx, R, M)
        assert geom[0] == (16 if R <= 16 else 8) and geom[1] * geom[2] == geom[0] and geom[5] * 8 <= 65536
        worst = 0.0
        for i in range(5):
            want, ref, bound, ref_bound = rr.sums(a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), b[b_off[i]:b_off[i] + n_pix].reshape(ny, nx), R, M)
            err = np.abs(S[i].astype(np.longdouble) - want).astype(np.float64)
            assert np.all(err <= bound), (i, (err / bound).max())
            assert np.all(np.abs(A[i].astype(np.longdouble) - ref).astype(np.float64) <= ref_bound)
            worst = max(worst, (err / bound).max())
        print('%d x %d R %d M %d: worst error / bound %.3g' % (ny, nx, R, M, worst))
        S2, A2, _ = emu_sums(emu, a, a_off, b, b_off, ny, nx, R, M)
        assert S2.tobytes() == S.tobytes() and A2.tobytes() == A.tobytes()
        S3, A3, _ = emu_sums(emu, a, a_off[::-1], b, b_off[::-1], ny, nx, R, M)
        assert S3[::-1].tobytes() == S.tobytes() and A3[::-1].tobytes() == A.tobytes()
        S4, A4, _ = emu_sums(emu, a, a_off[3:4], b, b_off[3:4], ny, nx, R, M)
        assert S4[0].tobytes() == S[3].tobytes() and A4[0].tobytes() == A[3].tobytes()


def test_geometry_keeps_the_lds_tile_under_64_kib_and_all_threads_busy(emu):
    """Every radius: the strips divide the band, the lanes cover the displacements, the LDS tile fits twice into 160 KiB."""
    rng = np.random.default_rng(1)
    for R in (1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 32):
        ny = nx = 2 * R + 8
        a = rng.random(ny * nx)
        _, _, (TY, G, h, passes, bands, lds) = emu_sums(emu, a, [0], a, [0], ny, nx, R, R)
        nd = (2 * R + 1) ** 2
        assert G * h == TY and bands == 1 and lds * 8 * 2 <= 160 * 1024
        assert (G * nd <= 256 and (G == TY or 2 * G * nd > 256)) if nd < 256 else (G == 1 and passes == -(-nd // 256))


# ---- the shift -----------------------------------------------------------------------------------------------------------------------
SHIFTS = [(0.0, 0.0), (3.0, -2.0), (-1.5, 0.25), (0.37, -0.81), (40.0, -40.0), (-40.3, 17.7)]


@pytest.mark.parametrize('order', [1, 3])
def test_emulated_shift_is_scipy(emu, order):
    """37 x 53 (tiles cut on both axes) and 70 x 130 (more than one tile each way): shifts 0, integer, negative, fractional and
    beyond the image (|s| = 40 on 37 rows); f64 -> f64 within 1e-12 max|image|; an f32 destination at most 1 ulp from the rounded
    twin; guard values around the destination intact; the sum within gamma_N sum |v| of the twin's."""
    rng = np.random.default_rng(order)
    for ny, nx in ((37, 53), (70, 130)):
        for dt in (np.float32, np.float64):
            src = (rng.random((len(SHIFTS), ny, nx)) * 1000.0).astype(dt)
            want = np.stack([rr.shift(src[k], SHIFTS[k], order) for k in range(len(SHIFTS))])
            got, stats = emu_shift(emu, src, SHIFTS, order, None, np.float64)
            err = np.abs(got - want).max() / np.abs(src).max()
            print('order %d %s %d x %d: max error %.3g max|image|' % (order, np.dtype(dt).name, ny, nx, err))
            assert err <= 1e-12
            assert np.all(stats[:, 0] == 0)
            for k in range(len(SHIFTS)):
                assert abs(stats[k, 1] - want[k].sum()) <= rr.gamma(ny * nx) * np.abs(want[k]).sum() + 1e-12 * np.abs(src).max() * ny * nx
            got32, _ = emu_shift(emu, src, SHIFTS, order, None, np.float32)
            w32 = want.astype(np.float32)
            assert np.all(np.abs(got32.astype(np.float64) - w32) <= np.spacing(np.abs(w32)))


def test_order_one_with_integer_shifts_copies_the_displaced_pixels_bit_for_bit(emu):
    rng = np.random.default_rng(5)
    for dt in (np.float32, np.float64):
        src = ((rng.random((3, 37, 53)) - 0.5) * 1e6).astype(dt)
        src[0, 0, 0] = -0.0
        shifts = [(0.0, 0.0), (3.0, -2.0), (-40.0, 75.0)]
        got, _ = emu_shift(emu, src, shifts, 1, None, dt)
        for k, (sy, sx) in enumerate(shifts):
            iy = np.pad(np.arange(37), 120, mode='reflect')[120 + int(sy):120 + int(sy) + 37]
            ix = np.pad(np.arange(53), 120, mode='reflect')[120 + int(sx):120 + int(sx) + 53]
            assert got[k].tobytes() == src[k][iy][:, ix].tobytes()


def overshoot_scene():
    """A bright square on zero: the cubic spline rings below zero beside its edges."""
    a = np.zeros((1, 40, 56))
    a[0, 12:28, 20:40] = 1000.0
    return a


def test_floor_and_raised_count_are_exact(emu):
    """The twin itself produces negative overshoot at order 3 on the scene; the floor and the count of raised pixels are exact
    where the twin is not within 1e-9 of the floor."""
    src = overshoot_scene()
    s = [(0.4, -0.3)]
    want = rr.shift(src[0], s[0], 3)
    assert want.min() < -10.0                                                  # (verified: the twin overshoots)
    floor = 1e-9
    got, stats = emu_shift(emu, src, s, 3, floor, np.float64)
    sure = np.abs(want - floor) > 1e-9
    assert np.all(got >= floor) and np.all(got[0][sure & (want < floor)] == floor)
    assert np.allclose(got[0][want > floor], want[want > floor], rtol=0, atol=1e-9)
    low, high = int((want < floor - 1e-9).sum()), int((want < floor + 1e-9).sum())
    assert low <= stats[0, 0] <= high and low > 50, (low, stats, high)
    assert stats[0, 0] == (got == floor).sum()


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation as a program of its own under -fsanitize=address,undefined, run directly: the images, the destination and the
    outputs are heap blocks of exactly their byte counts, the staged tiles exactly the launches' LDS sizes."""
    exe = str(tmp_path / 'register_emu_san')
    subprocess.check_call(['g++', '-DREGISTER_EMU_MAIN', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 24 32', r.stdout


# ---- the twin against the truth --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('refine', [0, 1])
@pytest.mark.parametrize('case', ['same', 'blur'])
def test_twin_finds_the_analytic_displacement(case, refine):
    """48 x 64 and 96 x 80 scenes, R = 6, noise-free, six displacements.  Measured worst errors of the twin: same PSF 0.057 px
    (refine = 0) and 0.0096 px (refine = 1); moving image through a different anisotropic blur (1.5, 0.7): 0.056 px and 0.0211 px --
    a property of the finite scene, not of the arithmetic.  Asserted at twice the measured values.  None lies at the limit."""
    worst = 0.0
    for seed, ny, nx in rr.SCENES:
        p = rr.blobs(seed, ny, nx)
        ref = rr.scene(p)
        for d in rr.DISPLACEMENTS:
            s, info = rr.estimate(rr.scene(p, d, BLUR if case == 'blur' else (0.0, 0.0)), ref, 6, refine)
            assert not info['at_limit'] and not info['flat']
            worst = max(worst, float(np.abs(s - d).max()))
    print('%s refine %d: worst error %.4f px' % (case, refine, worst))
    assert worst <= 2.0 * TWIN_ERROR[(case, refine)]


def test_committed_scenes_have_a_clear_peak():
    """The condition of the device test of estimate_shifts: on every committed scene the twin's best NCC exceeds the second best by
    more than 1e-6 (in the search window and in the 3 x 3 window of the refinement).  None is excluded."""
    for seed, ny, nx in rr.SCENES:
        p = rr.blobs(seed, ny, nx)
        ref = rr.scene(p)
        for d in rr.DISPLACEMENTS:
            for blur in ((0.0, 0.0), BLUR):
                img = rr.scene(p, d, blur)
                s, info = rr.estimate(img, ref, 6, 0)
                assert rr.margin_of(info['surface']) > 1e-6
                S1, r1, _, _ = rr.sums(ref, rr.shift(img, s, 3), 1, 8)
                c1, _ = rr.ncc(S1.astype(np.float64), r1.astype(np.float64), (ny - 16) * (nx - 16))
                assert rr.margin_of(c1) > 1e-6


def test_benefit_case_on_the_cpu():
    """The oracle on the twin's registration of the benefit case (64 x 64, V = 2, true displacement (2.3, -3.7) on view 1, K = 20):
    relative error 0.557 unregistered, 0.0220 registered: a factor of 25.4.  The device test asserts half of it."""
    import tile_reference as tr
    psfs, obj, meas = rr.benefit_case()
    s, info = rr.estimate(meas[1], meas[0], 8, 1)
    assert np.abs(s - rr.BENEFIT_DISPLACEMENT).max() < 0.15 and not info['at_limit']
    reg = np.stack([meas[0], rr.shift(meas[1], s, 3, 1e-9)])
    e0 = rr.relative_error(tr.oracle_estimate(meas, psfs, 20), obj)
    e1 = rr.relative_error(tr.oracle_estimate(reg, psfs, 20), obj)
    print('unregistered %.4f registered %.4f factor %.1f' % (e0, e1, e0 / e1))
    assert e0 / e1 >= rr.BENEFIT_FACTOR * 0.98


# ---- host logic ------------------------------------------------------------------------------------------------------------------------

def test_peak_ties_limit_flat_and_parabola():
    from rescan_line_sted_amd import registration as reg
    c = np.zeros((5, 5))
    c[1, 3] = c[2, 2] = c[3, 1] = 0.9                                       # a tie: the first in row-major order wins
    s, v, lim = reg.surface_peak(c)
    assert tuple(s) == (-1.0, 1.0) and v == 0.9 and not lim
    c = np.zeros((5, 5))
    c[2, 4] = 1.0                                                           # on the border: no sub-pixel part
    c[2, 3] = 0.8
    s, v, lim = reg.surface_peak(c)
    assert tuple(s) == (0.0, 2.0) and lim
    c = np.zeros((5, 5))
    c[2, 2], c[1, 2], c[3, 2], c[2, 1], c[2, 3] = 1.0, 0.5, 0.7, 0.9, 0.9   # delta_y = (0.5 - 0.7) / (2 (0.5 - 2 + 0.7)) = 0.125
    s, v, lim = reg.surface_peak(c)
    assert abs(s[0] - 0.125) < 1e-15 and s[1] == 0.0 and not lim
    tw, _, _, tl = rr.peak(c)
    assert np.array_equal(tw, s) and not tl
    # zero variance: flat, a surface of zeros
    S = np.zeros((9, 3))
    S[:, 0], S[:, 1], S[:, 2] = 50.0, 25.0, 10.0                            # S_bb - S_b^2 / n = 0 with n = 100
    surf, flat = reg.ncc_surface(S, (30.0, 20.0), 100)
    assert flat and not surf.any()
    surf, flat = reg.ncc_surface(S + [0, 1, 0], (30.0, 9.0), 100)          # S_aa - S_a^2 / n = 0
    assert flat
    # the NCC of an image with itself is 1 at d = 0
    a = np.random.default_rng(0).random((30, 30))
    St, rt, _, _ = rr.sums(a, a, 2, 4)
    surf, flat = reg.ncc_surface(St.astype(np.float64), rt.astype(np.float64), 22 * 22)
    assert not flat and abs(surf[2, 2] - 1.0) < 1e-12 and np.argmax(surf) == 12
    assert np.array_equal(surf, rr.ncc(St.astype(np.float64), rt.astype(np.float64), 22 * 22)[0])


def test_the_library_declares_and_checks_its_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert len(_lib.PROTOTYPES['rl_register_sums'][1]) == 14 and len(_lib.PROTOTYPES['rl_shift_images'][1]) == 12
    header = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_register_sums(' in header and 'int rl_shift_images(' in header and '#define RL_REGISTER_FIELDS 3' in header
    ctx, a, b = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)          # (never dereferenced)
    off = (ctypes.c_int64 * 2)(0, 100)
    neg = (ctypes.c_int64 * 2)(0, -1)
    out, ref = (ctypes.c_double * (2 * 4225 * 3))(), (ctypes.c_double * 4)()
    good = dict(ctx=ctx, a=a, adt=0, aoff=off, b=b, bdt=1, boff=off, n=2, ny=40, nx=56, R=3, M=3, out=out, ref=ref)
    bad = [dict(ctx=None), dict(a=None), dict(b=None), dict(aoff=None), dict(boff=None), dict(out=None), dict(ref=None), dict(adt=2), dict(bdt=-1),
           dict(n=0), dict(R=0), dict(R=33, M=33), dict(M=2), dict(M=17), dict(ny=13), dict(nx=13), dict(aoff=neg), dict(boff=neg),
           dict(ny=96, nx=80, R=32, M=37), dict(ny=96, nx=80, R=32, M=40)]  # (96 x 80 at R = 32: from M = 37 on the interior is too small)
    for change in bad:
        g = {**good, **change}
        rc = L.rl_register_sums(g['ctx'], g['a'], g['adt'], g['aoff'], g['b'], g['bdt'], g['boff'], g['n'], g['ny'], g['nx'], g['R'], g['M'], g['out'], g['ref'])
        assert rc == -1 and L.rl_last_error() != b'', change
    sh = (ctypes.c_double * 4)(0.5, 1.0, -2.0, 3.0)
    good = dict(ctx=ctx, src=a, sdt=0, n=2, ny=8, nx=16, sh=sh, order=3, floor=0.0, dst=b, ddt=1, stats=None)
    bad = [dict(ctx=None), dict(src=None), dict(sh=None), dict(dst=None), dict(sdt=2), dict(ddt=-1), dict(n=0), dict(ny=0), dict(nx=0), dict(order=2),
           dict(order=0), dict(floor=float('nan')), dict(sh=(ctypes.c_double * 4)(0.0, float('nan'), 0.0, 0.0)),
           dict(sh=(ctypes.c_double * 4)(0.0, 0.0, float('inf'), 0.0)), dict(sh=(ctypes.c_double * 4)(2e9, 0.0, 0.0, 0.0)),
           dict(dst=ctypes.c_void_p(0x100000 + 64)), dict(dst=ctypes.c_void_p(0x100000 - 64))]
    for change in bad:
        g = {**good, **change}
        rc = L.rl_shift_images(g['ctx'], g['src'], g['sdt'], g['n'], g['ny'], g['nx'], g['sh'], g['order'], g['floor'], g['dst'], g['ddt'], g['stats'])
        assert rc == -1 and L.rl_last_error() != b'', change


def test_register_kernels_do_not_spill(tmp_path):
    """register_kernels.hip compiled device-only with the flags of _build.py: the ten kernels (the sums x 4 dtype pairs, the shift's
    passes x 4, the two totals) have `.private_segment_fixed_size` 0."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'register_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'register_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    assert len(priv) == 10 and sum('k_register_sums<' in k for k in priv) == 4 and sum('k_shift_pass<' in k for k in priv) == 4, priv
    assert sum('k_register_totals' in k for k in priv) == 1 and sum('k_shift_totals' in k for k in priv) == 1, priv
    assert all(v == 0 for v in priv.values()), priv


# ---- the wrappers on a numpy stand-in ---------------------------------------------------------------------------------------------------

class _Buf:
    def __init__(self, a, dtype):
        self.a, self.dtype = a, dtype


class _NumpyDevice:
    """Stands in for registration._Device: its steps in numpy -- the twin's ingest, the long double sums rounded to float64, scipy's
    shift, the oracle as the plan -- and a log of what the wrapper asked for."""
    log = None
    NP = {'f32': np.float32, 'f64': np.float64, None: np.uint8}

    def __init__(self, psfs=None, batch=0, shape=None, dtype='f32', device=0, acceleration=None, tv_lambda=None, tv_epsilon=0.1):
        self.psfs, self.batch, self.shape, self.dtype = psfs, batch, shape, dtype
        type(self).log = self.calls = [('plan', batch, shape, dtype)]
        if psfs is not None:
            self.meas = _Buf(np.zeros(batch * len(psfs) * shape[0] * shape[1], dtype=self.NP[dtype]), dtype)

    def alloc(self, elements, dtype):
        return _Buf(np.full(int(elements), 77 if dtype is None else np.nan, dtype=self.NP[dtype]), dtype)

    def upload(self, buf, array, byte_offset=0):
        raw = np.ascontiguousarray(array).view(np.uint8).ravel()
        buf.a.view(np.uint8)[byte_offset:byte_offset + raw.size] = raw
        self.calls.append(('upload', array.shape, byte_offset))

    def download(self, buf, elements, element_offset=0):
        return buf.a[element_offset:element_offset + elements].astype(np.float64)

    def copy(self, dst, dst_element, src, src_element, elements):
        dst.a[dst_element:dst_element + elements] = src.a[src_element:src_element + elements]

    def measurement(self):
        return self.meas

    def ingest(self, raw, code, images, sensor, origin, frame_stride, view_stride, n_slots, n_valid, V, shape, camera, dark, dst, stats):
        dt = [k for k, v in ir.RAW.items() if v == code][0]
        frames = raw.a[:images * sensor[0] * sensor[1] * dt.itemsize].view(dt).reshape(images, sensor[0], sensor[1])
        m, s = ir.ingest(frames, n_slots, n_valid, V, shape[0], shape[1], origin[0], origin[1], frame_stride, view_stride,
                         None if dark is None else dark.a.reshape(shape), camera.dark, camera.gain, camera.epsilon,
                         0.0 if camera.saturation is None else camera.saturation, self.NP[dst.dtype])
        dst.a[:] = m.ravel()
        stats.a[:] = s.ravel()
        self.calls.append(('ingest', n_valid, frame_stride, view_stride))

    def sums(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, M):
        S, A = [], []
        for ro, mo in zip(ref_offsets, mov_offsets):
            s, a, _, _ = rr.sums(ref.a[ro:ro + ny * nx].reshape(ny, nx), mov.a[mo:mo + ny * nx].reshape(ny, nx), R, M)
            S.append(s.astype(np.float64))
            A.append(a.astype(np.float64))
        self.calls.append(('sums', list(ref_offsets), list(mov_offsets), R, M))
        return np.stack(S), np.stack(A)

    def shift(self, src, src_element, n, ny, nx, shifts, order, floor, dst, dst_element=0):
        sh = np.asarray(shifts, dtype=np.float64).reshape(n, 2)
        stats = np.zeros((n, 2))
        for k in range(n):
            img = src.a[src_element + k * ny * nx:src_element + (k + 1) * ny * nx].reshape(ny, nx)
            raw = rr.shift(img, sh[k], order)
            out = raw if floor is None else np.maximum(raw, floor)
            stats[k] = [0 if floor is None else (raw < floor).sum(), out.sum()]
            dst.a[dst_element + k * ny * nx:dst_element + (k + 1) * ny * nx] = out.ravel()
        self.calls.append(('shift', n, order, floor, sh.copy()))
        return stats

    def gather_shift(self, src, offsets, ny, nx, shifts, dst):
        for k, o in enumerate(offsets):
            self.shift(src, o, 1, ny, nx, shifts[k:k + 1], 3, None, dst, k * ny * nx)

    def iterate(self, iterations):
        import tile_reference as tr
        V, (ny, nx) = len(self.psfs), self.shape
        m = self.meas.a.astype(np.float64).reshape(self.batch, V, ny, nx)
        self.calls.append(('iterate', iterations, m.copy()))
        return np.stack([np.asarray(tr.oracle_estimate(f, self.psfs, iterations)) for f in m])

    def unresolved(self):
        return 0

    def strategy(self):
        return {}

    def close(self):
        self.calls.append(('close',))


def _drifting_stack(F=5, V=2, ny=48, nx=64, pad=(3, 5)):
    """A u16 stack of one scene: view v displaced by VIEW[v], frame f by f * DRIFT on top, inside a larger sensor frame."""
    p = rr.blobs(3, ny, nx)
    view, drift = np.array([[0.0, 0.0], [1.6, -2.2]]), np.array([0.7, 0.45])
    truth = np.zeros((F, V, 2))
    raw = np.full((F, V, ny + pad[0] + 2, nx + pad[1] + 1), 100, dtype=np.uint16)
    for f in range(F):
        for v in range(V):
            truth[f, v] = view[v] + f * drift
            raw[f, v, pad[0]:pad[0] + ny, pad[1]:pad[1] + nx] = np.rint(rr.scene(p, truth[f, v], (0.0, 0.0) if v == 0 else (1.0, 0.4)) * 8.0 + 100.0)
    return raw, truth, (pad[0], pad[1], ny, nx)


@pytest.mark.parametrize('order', ['frame-view', 'view-frame'])
def test_wrapper_chunks_composes_and_applies_the_shifts(monkeypatch, order):
    """F = 5, V = 2, batch = 2 (it does not divide F), a window of a u16 sensor frame, both orders: three chunks, the short one
    filled; the view estimate runs once, on frame 0; frame f, view v is compared with frame 0, view v; the applied shift is their
    sum and is close to the truth; the measurement handed to the plan is the shifted ingest; the estimates are the oracle's."""
    from rescan_line_sted_amd import line_sted_tools, registration as reg, stack
    assert line_sted_tools.deconvolve_stack_registered is reg.deconvolve_stack_registered
    assert line_sted_tools.estimate_shifts is reg.estimate_shifts and line_sted_tools.shift_images is reg.shift_images
    monkeypatch.setattr(reg, '_Device', _NumpyDevice)
    frames, truth, roi = _drifting_stack()
    raw = frames if order == 'frame-view' else np.ascontiguousarray(frames.transpose(1, 0, 2, 3))
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    cam = stack.CameraModel(dark=100.0, gain=0.125)
    est, info = reg.deconvolve_stack_registered(raw, psfs, 2, camera=cam, order=order, roi=roi, batch=2, dtype='f64', max_shift=6)
    calls = _NumpyDevice.log
    assert calls[0] == ('plan', 2, (48, 64), 'f64') and calls[-1] == ('close',)
    assert [c[1:] for c in calls if c[0] == 'ingest'] == [(n, 2, 1) if order == 'frame-view' else (n, 1, n) for n in (2, 2, 1)]
    n_pix = 48 * 64
    big = [c for c in calls if c[0] == 'sums' and c[3] == 6]
    assert big[0][1:3] == ([0], [n_pix]) and big[0][4] == 8                                  # views: (0, 1) against (0, 0), once
    assert big[1][1:3] == ([0, n_pix], [2 * n_pix, 3 * n_pix])                               # chunk 0: frame 1, each view to its own
    assert big[2][1:3] == ([0, n_pix, 0, n_pix], [0, n_pix, 2 * n_pix, 3 * n_pix]) and big[3][1:3] == ([0, n_pix], [0, n_pix]) and len(big) == 4
    assert all(c[4] == 8 for c in calls if c[0] == 'sums' and c[3] == 1)                     # the refinement: R = 1, M = max_shift + 2
    assert info['chunks'] == 3 and info['batch'] == 2 and est.shape == (5, 48, 64) and est.dtype == np.float64
    assert np.abs(info['shifts'] - truth).max() < 0.12, np.abs(info['shifts'] - truth).max()
    assert np.all(info['shifts'][0, 0] == 0) and not info['at_limit'].any() and not info['flat'].any() and info['ncc'][1:].min() > 0.9
    assert info['view_ncc'][1] > 0.9 and info['view_ncc'][0] == 0 and info['raised'].shape == (5, 2)
    want_meas, want_stats = ir.measurement(frames, 2, 'frame-view', roi, 100.0, 0.125)
    assert np.array_equal(info['level'], want_stats[:, :, 0]) and info['clipped'].dtype == np.int64
    its = [c for c in calls if c[0] == 'iterate']
    assert len(its) == 3 and np.abs(its[2][2][1] - 1.0).max() < 1e-12                       # the filler of the short last chunk: ones, unshifted
    final = [c for c in calls if c[0] == 'shift' and c[1] == 4]
    assert len(final) == 3 and all(c[2] == 3 and c[3] == cam.epsilon for c in final) and np.all(final[2][4][2:] == 0)
    import tile_reference as tr
    for f in (0, 3):
        m = np.stack([np.maximum(rr.shift(want_meas[f, v], info['shifts'][f, v], 3), cam.epsilon) for v in range(2)])
        assert np.array_equal(its[f // 2][2][f % 2], m)
        assert np.array_equal(est[f], np.asarray(tr.oracle_estimate(m, psfs, 2)))


def test_wrapper_given_shifts_switches_and_argument_errors(monkeypatch):
    from rescan_line_sted_amd import registration as reg
    monkeypatch.setattr(reg, '_Device', _NumpyDevice)
    frames, truth, roi = _drifting_stack(F=3)
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    # shifts given: no estimate at all, applied as they are, with the order asked for
    given = np.round(truth)
    est, info = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, shifts=given, interp=1)
    calls = _NumpyDevice.log
    assert not [c for c in calls if c[0] == 'sums'] and np.array_equal(info['shifts'], given)
    assert [c[2] for c in calls if c[0] == 'shift'] == [1] and info['batch'] == 3
    # each entry of `register` switched off
    est, info = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, register=('frames',), max_shift=6, refine=0)
    assert np.all(info['shifts'][0] == 0) and np.abs(info['shifts'][1:] - (truth[1:] - truth[0])).max() < 0.15
    assert all(c[1] != [0] for c in _NumpyDevice.log if c[0] == 'sums')
    est, info = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, register=('views',), max_shift=6, refine=0)
    assert len([c for c in _NumpyDevice.log if c[0] == 'sums']) == 1 and np.all(info['shifts'][:, 0] == 0)
    assert np.all(info['shifts'][:, 1] == info['shifts'][0, 1]) and np.abs(info['shifts'][0, 1] - truth[0, 1]).max() < 0.15
    est, info = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, register=())
    assert not [c for c in _NumpyDevice.log if c[0] == 'sums'] and not info['shifts'].any()
    # a flat image: shift 0, flagged
    blank = frames.copy()
    blank[2, 1] = 300
    est, info = reg.deconvolve_stack_registered(blank, psfs, 1, roi=roi, max_shift=6)
    assert info['flat'][2, 1] and not info['flat'][2, 0] and np.array_equal(info['shifts'][2, 1], info['shifts'][0, 1])
    # a drift beyond the window: at the limit
    est, info = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, register=('views',), max_shift=2, refine=0)
    assert info['view_at_limit'][1]
    for kwargs in (dict(shifts=np.zeros((3, 2))), dict(shifts=np.zeros((3, 2, 3))), dict(shifts=np.full((3, 2, 2), np.nan)), dict(interp=2),
                   dict(register=('rotation',)), dict(max_shift=0), dict(max_shift=33), dict(max_shift=20), dict(refine=-1), dict(order='view'),
                   dict(dtype='f16'), dict(batch=0), dict(roi=(0, 0, 100, 64)), dict(acceleration='nesterov'), dict(tv_lambda=0.5)):
        with pytest.raises(ValueError):
            reg.deconvolve_stack_registered(frames, psfs, 1, **{**dict(roi=roi), **kwargs})
    for bad in (frames.astype(np.float64), frames.astype(np.int32)):
        with pytest.raises(ValueError):
            reg.deconvolve_stack_registered(bad, psfs, 1)
    with pytest.raises(ValueError):
        reg.deconvolve_stack_registered(frames, psfs, -1)
    a = np.zeros((2, 40, 40), dtype=np.float32)
    for args, kwargs in (((a.astype(np.int16), a[0]), {}), ((a, a[0].astype(np.float16)), {}), ((a, a[0, :30]), {}), ((a[:, :20], a[0, :20]), {}),
                         ((a, a[0]), dict(max_shift=0)), ((a, a[0]), dict(margin=5)), ((a, a[0]), dict(refine=-1))):
        with pytest.raises(ValueError):
            reg.estimate_shifts(*args, **kwargs)
    for args, kwargs in (((a.astype(np.int32), np.zeros((2, 2))), {}), ((a, np.zeros((3, 2))), {}), ((a, np.zeros(2)), {}), ((a, np.zeros((2, 2))), dict(order=2)),
                         ((a, np.full((2, 2), np.inf)), {})):
        with pytest.raises(ValueError):
            reg.shift_images(*args, **kwargs)


def test_estimate_shifts_on_the_stand_in_is_the_twin(monkeypatch):
    """estimate_shifts through the stand-in's sums and shift equals the twin's estimate (same stages, same order), f32 and f64
    images, a shared and a per-image reference; the surfaces on request."""
    from rescan_line_sted_amd import registration as reg
    monkeypatch.setattr(reg, '_Device', _NumpyDevice)
    p = rr.blobs(3, 48, 64)
    ref = rr.scene(p)
    imgs = np.stack([rr.scene(p, d) for d in rr.DISPLACEMENTS[:4]])
    for refine in (0, 1):
        s, info = reg.estimate_shifts(imgs, ref, max_shift=6, refine=refine, surfaces=True)
        for k in range(4):
            w, wi = rr.estimate(imgs[k], ref, 6, refine)
            assert np.array_equal(s[k], w) and info['ncc'][k] == wi['ncc'] and np.array_equal(info['surfaces'][k], wi['surface'])
    s32, _ = reg.estimate_shifts(imgs.astype(np.float32), np.stack([ref] * 4).astype(np.float32), max_shift=6)
    assert np.abs(s32 - np.array(rr.DISPLACEMENTS[:4])).max() < 0.02
    one, _ = reg.estimate_shifts(imgs[2], ref, max_shift=6)
    assert one.shape == (1, 2)
