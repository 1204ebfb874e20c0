"""The coarse registration stage without a GPU (include/rlsted.h rl_register_xcorr; rescan_line_sted_amd/registration.py
coarse_shifts, estimate_shifts(coarse=), deconvolve_stack_registered(coarse=)): the kernel bodies emulated thread by thread
(tests/emu/xcorr_emu.cpp) against the twin (tests/xcorr_reference.py) -- C(d) within the derived bound, the means, energies and
window sums bit for bit, identical across runs and pair orderings; the twin's two ways of computing C against each other; peak, tie
and flat rules; the same bodies as a stand-alone program under the address and undefined-behaviour sanitizers; the argument checks of
the library; the device build's private segments; and the two-stage estimate on a numpy stand-in for the device.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import register_reference as rr
import xcorr_reference as xr
from conftest import ROOT
from test_register_cpu import _NumpyDevice, _drifting_stack

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'xcorr_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('xcorr_kernels.hpp', 'kernel_variants.hpp', 'conv_kernels.hpp', 'fft_core.hpp', 'fft_configs.hpp',
                                        'accel_kernels.hpp', 'outer_lds.hpp')] + [os.path.join(EMU_DIR, 'emu_common.hpp')]
FLAGS = ['-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas', '-pthread']
FLOATS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libxcorr_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + [SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_register_xcorr.argtypes = [vp, i, vp, vp, i, vp, i, i, i, i, vp, vp, vp, vp, vp]
    lib.emu_xcorr_peak.argtypes = [vp, vp, i, i, i, vp, vp]
    lib.emu_xcorr_length.argtypes = [ctypes.c_longlong]
    return lib


def emu_xcorr(emu, a, a_off, b, b_off, ny, nx, R):
    """(fields [n][7], surface [n][W][W] f32, C [n][W][W] f64, stats [n][4], geom [8]); guard values around the outputs intact"""
    W, n = 2 * R + 1, len(a_off)
    whole_p, whole_s = np.full(n * 7 + 16, 7.0), np.full(n * W * W + 16, 7.0, dtype=np.float32)
    P, S = whole_p[8:8 + n * 7], whole_s[8:8 + n * W * W]
    C, stats, geom = np.full((n, W, W), np.nan), np.full((n, 4), np.nan), np.zeros(8, dtype=np.intc)
    ao, bo = np.asarray(a_off, dtype=np.int64), np.asarray(b_off, dtype=np.int64)
    assert emu.emu_register_xcorr(_p(a), FLOATS[a.dtype], _p(ao), _p(b), FLOATS[b.dtype], _p(bo), n, ny, nx, R, _p(P), _p(S), _p(C), _p(stats), _p(geom)) == 0
    assert np.all(whole_p[:8] == 7) and np.all(whole_p[8 + n * 7:] == 7) and np.all(whole_s[:8] == 7) and np.all(whole_s[8 + n * W * W:] == 7)
    return P.reshape(n, 7).copy(), S.reshape(n, W, W).copy(), C, stats, geom


def displaced(rng, ref, d, noise=0.05):
    """ref's content displaced by the integer d (B[y + d] = A[y]); what enters from outside is fresh noise"""
    ny, nx = ref.shape
    out = rng.random((ny, nx)) * ref.max()
    ys, xs = np.arange(ny) - d[0], np.arange(nx) - d[1]
    oky, okx = (ys >= 0) & (ys < ny), (xs >= 0) & (xs < nx)
    out[np.ix_(oky, okx)] = ref[np.ix_(ys[oky], xs[okx])]
    return out + noise * ref.max() * rng.random((ny, nx))


# (ny, nx, R, pairs): every length on either axis, non-square length pairs, equality ny + R = L, odd sizes
CASES = [(24, 40, 8, 4), (56, 48, 8, 4), (37, 51, 6, 4), (40, 150, 10, 3), (100, 40, 20, 3), (230, 60, 12, 2), (540, 230, 12, 2),
         (30, 1100, 10, 2), (600, 30, 10, 2)]


@pytest.mark.parametrize('ny,nx,R,pairs', CASES)
def test_emulated_bodies_are_within_the_bound_of_the_twin(emu, ny, nx, R, pairs):
    """Pairs over two references (shared) at odd element offsets, f32 reference with f64 moving images and the other way round (the
    small shapes: f32 / f32 and f64 / f64 too): C within the derived bound of the float64 twin; the integer peak the twin's, which
    leads its runner-up by more than twice the bound; means and energies, the window sums of the emulated surface and the peak value
    bit for bit the twin's fixed order; the float32 surface the rounded v; a second run, the reversed pair order and a pair alone
    give the same bits; the LDS blocks are the launcher's byte counts and fit 64 KiB."""
    rng = np.random.default_rng(ny * 1000 + nx)
    n_pix = ny * nx
    W = 2 * R + 1
    combos = [(np.float32, np.float64), (np.float64, np.float32)] + ([(np.float32, np.float32), (np.float64, np.float64)] if n_pix < 3000 else [])
    worst = 0.0
    for ta, tb in combos:
        a = (rng.random(2 * n_pix + 5) * 1000.0 + 100.0).astype(ta)
        b = np.zeros(pairs * n_pix + 3, dtype=tb)
        a_off = [5 + (k % 2) * n_pix for k in range(pairs)]
        b_off = [3 + k * n_pix for k in reversed(range(pairs))]
        true = [(-R, R), (R // 2, -1), (0, 0), (R, -R)][:pairs]
        for k in range(pairs):
            ref = a[a_off[k]:a_off[k] + n_pix].reshape(ny, nx).astype(np.float64)
            b[b_off[k]:b_off[k] + n_pix] = (displaced(rng, ref, true[k]) * (0.01 if k == 1 else 1.0)).ravel()       # (pair 1: a much weaker moving image)
        P, S, C, stats, geom = emu_xcorr(emu, a, a_off, b, b_off, ny, nx, R)
        assert (geom[0], geom[1]) == (xr.length(ny + R), xr.length(nx + R)) and all(0 < geom[3 + 2 * k] <= 65536 for k in range(3))
        assert all(geom[2 + 2 * k] in (256, 144) for k in range(3))
        for i in range(pairs):
            A_img, B_img = a[a_off[i]:a_off[i] + n_pix].reshape(ny, nx), b[b_off[i]:b_off[i] + n_pix].reshape(ny, nx)
            f, v, Ct, bound = xr.xcorr(A_img, B_img, R)
            _, ma, ea = xr.centred(A_img)
            _, mb, eb = xr.centred(B_img)
            assert stats[i].tobytes() == np.array([ma, mb, ea, eb]).tobytes()
            err = np.abs(C[i] - Ct).max()
            assert err <= bound, (i, err / bound)
            worst = max(worst, err / bound)
            assert (f[0], f[1]) == true[i] and np.sort(v.ravel())[-1] - np.sort(v.ravel())[-2] > 2 * bound / xr.counts(ny, nx, R).min()
            ve = xr.surface(C[i], ny, nx, R)                                # the emulated surface in float64, as PEAK forms it
            assert P[i].tobytes() == xr.fields(ve, ea, eb).tobytes(), (P[i], xr.fields(ve, ea, eb))
            assert (P[i][0], P[i][1]) == true[i]
            assert S[i].tobytes() == ve.astype(np.float32).tobytes()
        if (ta, tb) != combos[0]:
            continue
        P2, S2, C2, _, _ = emu_xcorr(emu, a, a_off, b, b_off, ny, nx, R)
        assert P2.tobytes() == P.tobytes() and S2.tobytes() == S.tobytes()
        P3, S3, _, _, _ = emu_xcorr(emu, a, a_off[::-1], b, b_off[::-1], ny, nx, R)
        assert P3[::-1].tobytes() == P.tobytes() and S3[::-1].tobytes() == S.tobytes()
        P4, S4, _, _, _ = emu_xcorr(emu, a, a_off[1:2], b, b_off[1:2], ny, nx, R)
        assert P4[0].tobytes() == P[1].tobytes() and S4[0].tobytes() == S[1].tobytes()
    print('%d x %d R %d: worst error / bound %.3g' % (ny, nx, R, worst))


def test_the_twin_computes_c_two_ways():
    """Direct long double sums and np.fft on the zero-extended arrays agree to 1e-12 ||a|| ||b|| on small shapes, equality
    ny + R = L included (no lag wraps around)."""
    rng = np.random.default_rng(2)
    for ny, nx, R in ((24, 40, 8), (56, 48, 8), (37, 51, 6), (100, 40, 20)):
        a, _, ea = xr.centred(rng.random((ny, nx)) * 100.0)
        b, _, eb = xr.centred(rng.random((ny, nx)) * 100.0)
        d = np.abs(xr.correlation_fft(a, b, R) - xr.correlation_direct(a, b, R).astype(np.float64)).max()
        assert d <= 1e-12 * np.sqrt(ea * eb), d / np.sqrt(ea * eb)


def test_lengths_and_the_bound():
    assert [xr.length(n) for n in (1, 64, 65, 192, 193, 256, 257, 576, 577, 1152, 1153)] == [64, 64, 192, 192, 256, 256, 576, 576, 1152, 1152, None]
    assert xr.KAPPA == 22.0 and abs(xr.bound(512, 512, 64, 4.0, 9.0) - 22.0 * 2.0 ** -23 * 2 * np.log2(576) * 6.0) < 1e-18


def test_lengths_of_the_variant_table_are_the_twins(emu):
    for n in (1, 64, 65, 192, 193, 256, 257, 576, 577, 1152, 1153, 4608):
        assert emu.emu_xcorr_length(n) == (xr.length(n) or 0)


def emu_peak(emu, corr, stats, ny, nx, R):
    P, S = np.full(7, np.nan), np.full(corr.shape, np.nan, dtype=np.float32)
    assert emu.emu_xcorr_peak(_p(np.ascontiguousarray(corr, dtype=np.float32)), _p(np.asarray(stats, dtype=np.float64)), ny, nx, R, _p(P), _p(S)) == 0
    return P, S


def test_peak_tie_flat_and_scale_rules(emu):
    """PEAK alone on given windows: a tie goes to the first maximum in row-major order (two displacements with the same overlap count
    and the same C); the overlap count decides between equal C; an energy that is zero, negative or nan: d = (0, 0), v = 0, the sums
    still those of the window; the power-of-two scale of the energies is applied exactly; a window wider than one round of threads
    (R = 140: 281 rows)."""
    R, ny, nx = 3, 40, 50
    W = 2 * R + 1
    c = np.zeros((W, W), dtype=np.float32)
    c[R + 2, R - 1] = c[R - 2, R + 1] = c[R + 2, R + 1] = 5.0               # counts (ny - 2)(nx - 1) each
    P, S = emu_peak(emu, c, [0.0, 0.0, 1.0, 1.0], ny, nx, R)
    assert tuple(P[:3]) == (-2.0, 1.0, 5.0 / (38 * 49))
    assert P.tobytes() == xr.fields(xr.surface(c.astype(np.float64), ny, nx, R), 1.0, 1.0).tobytes()
    c[R, R] = 5.0                                                           # the full overlap: a smaller v
    c[R + 3, R + 3] = 5.0                                                   # the least overlap: the largest v
    P, _ = emu_peak(emu, c, [0.0, 0.0, 1.0, 1.0], ny, nx, R)
    assert tuple(P[:2]) == (3.0, 3.0)
    for ea, eb in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, float('nan'))):
        P, _ = emu_peak(emu, c, [0.0, 0.0, ea, eb], ny, nx, R)
        assert tuple(P[:3]) == (0.0, 0.0, 0.0) and P[5] != 0.0
    P, _ = emu_peak(emu, c, [0.0, 0.0, 2.0 ** 21, 2.0 ** -8], ny, nx, R)    # sqrt: 2^10 (floor of 10.5), 2^-4
    assert P[2] == 5.0 * 2.0 ** 6 / (37 * 47)
    R, ny, nx = 140, 300, 290
    W = 2 * R + 1
    c = np.random.default_rng(4).random((W, W)).astype(np.float32)
    c[270, 5] = 40.0
    P, S = emu_peak(emu, c, [0.0, 0.0, 3.0, 5.0], ny, nx, R)
    v = xr.surface(c.astype(np.float64) * 2.0, ny, nx, R)                   # floor(log2 sqrt 3) = 0, floor(log2 sqrt 5) = 1
    assert P.tobytes() == xr.fields(v, 3.0, 5.0).tobytes() and tuple(P[:2]) == (130.0, -135.0) and S.tobytes() == v.astype(np.float32).tobytes()


def test_a_flat_image_through_the_whole_emulation(emu):
    rng = np.random.default_rng(6)
    a = rng.random(24 * 40).astype(np.float32)
    b = np.full(24 * 40, 3.25)
    P, S, C, stats, _ = emu_xcorr(emu, a, [0], b, [0], 24, 40, 8)
    assert tuple(P[0][:3]) == (0.0, 0.0, 0.0) and P[0][4] == 0.0 and P[0][3] > 0.0
    assert np.abs(S).max() < 1e-6 * np.sqrt(P[0][3])                       # (the rounding residue of the other image's transform)


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation as a program of its own under -fsanitize=address,undefined, run directly: the images and the outputs are heap
    blocks of exactly their byte counts at odd offsets, the LDS blocks exactly the launches' sizes; every length, f32 / f64 / mixed."""
    exe = str(tmp_path / 'xcorr_emu_san')
    subprocess.check_call(['g++', '-DXCORR_EMU_MAIN', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS + [SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 16', r.stdout


# ---- the library ---------------------------------------------------------------------------------------------------------------------

def test_the_library_declares_and_checks_its_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert len(_lib.PROTOTYPES['rl_register_xcorr'][1]) == 13
    header = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_register_xcorr(' in header and '#define RL_XCORR_FIELDS 7' in header
    ctx, a, b = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)          # (never dereferenced)
    off = (ctypes.c_int64 * 2)(0, 100)
    neg = (ctypes.c_int64 * 2)(0, -1)
    out = (ctypes.c_double * 14)()
    good = dict(ctx=ctx, a=a, adt=0, aoff=off, b=b, bdt=1, boff=off, n=2, ny=40, nx=56, R=8, out=out)
    bad = [dict(ctx=None), dict(a=None), dict(b=None), dict(aoff=None), dict(boff=None), dict(out=None), dict(adt=2), dict(bdt=-1), dict(n=0),
           dict(R=0), dict(R=21), dict(ny=0), dict(nx=0), dict(ny=15), dict(aoff=neg), dict(boff=neg),
           dict(ny=1100, nx=1100, R=53), dict(ny=60, nx=1145, R=8), dict(ny=2000, nx=2000, R=100)]
    for change in bad:
        g = {**good, **change}
        rc = L.rl_register_xcorr(g['ctx'], g['a'], g['adt'], g['aoff'], g['b'], g['bdt'], g['boff'], g['n'], g['ny'], g['nx'], g['R'], g['out'], None)
        assert rc == -1 and L.rl_last_error() != b'', change


def test_xcorr_kernels_do_not_spill(tmp_path):
    """xcorr_kernels.hip compiled device-only with the flags of _build.py: the seventeen kernels (three stages x five lengths, the
    statistics, the peak) have `.private_segment_fixed_size` 0."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'xcorr_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE + _build.FFT_FLAGS +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'xcorr_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    assert len(priv) == 17 and sum('k_xcorr<' in k for k in priv) == 15, priv
    assert sum('k_xcorr_stats' in k for k in priv) == 1 and sum('k_xcorr_peak' in k for k in priv) == 1, priv
    assert all(v == 0 for v in priv.values()), priv
    assert any(os.path.basename(j[1]) == 'xcorr_kernels.hip' for j in _build.jobs())


# ---- the two-stage estimate on a numpy stand-in ------------------------------------------------------------------------------------------

class _CoarseDevice(_NumpyDevice):
    """The stand-in of tests/test_register_cpu.py with the two steps the coarse stage adds: rl_register_xcorr as the twin, and the
    gathering shift at a given order."""

    def xcorr(self, ref, ref_offsets, mov, mov_offsets, ny, nx, R, surfaces=False):
        P, V = [], []
        for ro, mo in zip(ref_offsets, mov_offsets):
            f, v, _, _ = xr.xcorr(ref.a[ro:ro + ny * nx].reshape(ny, nx), mov.a[mo:mo + ny * nx].reshape(ny, nx), R)
            P.append(f)
            V.append(v.astype(np.float32))
        self.calls.append(('xcorr', list(ref_offsets), list(mov_offsets), R))
        return (np.stack(P), np.stack(V)) if surfaces else np.stack(P)

    def gather_shift(self, src, offsets, ny, nx, shifts, dst, order=3):
        for k, o in enumerate(offsets):
            self.shift(src, o, 1, ny, nx, shifts[k:k + 1], order, None, dst, k * ny * nx)


def _same_log(x, y):
    if len(x) != len(y):
        return False
    for cx, cy in zip(x, y):
        if len(cx) != len(cy) or any(not np.array_equal(u, v) for u, v in zip(cx, cy)):
            return False
    return True


def test_coarse_none_is_todays_path(monkeypatch):
    """coarse=None on the stand-in of tests/test_register_cpu.py, which has no xcorr step and no order argument: it runs, and on the
    new stand-in the log of device calls and the results are the same; max_shift = 33 still raises, with and without coarse."""
    from rescan_line_sted_amd import registration as reg
    p = rr.blobs(3, 48, 64)
    ref = rr.scene(p)
    imgs = np.stack([rr.scene(p, d) for d in rr.DISPLACEMENTS[:3]])
    frames, truth, roi = _drifting_stack(F=3)
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    got = []
    for dev in (_NumpyDevice, _CoarseDevice):
        monkeypatch.setattr(reg, '_Device', dev)
        s, info = reg.estimate_shifts(imgs, ref, max_shift=6, refine=1, coarse=None)
        log1 = dev.log
        est, dinfo = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, max_shift=6, batch=2)
        got.append((s, info, log1, est, dinfo, dev.log))
        assert not [c for c in log1 + dev.log if c[0] == 'xcorr'] and 'coarse' not in info and 'coarse' not in dinfo
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][3].tobytes() == got[1][3].tobytes()
    assert _same_log(got[0][2], got[1][2]) and _same_log(got[0][5], got[1][5])
    assert got[0][4]['shifts'].tobytes() == got[1][4]['shifts'].tobytes()
    for coarse in (None, 8):
        with pytest.raises(ValueError):
            reg.estimate_shifts(imgs, ref, max_shift=33, coarse=coarse)


@pytest.fixture(scope='module')
def grouped():
    """Six pairs on one 160 x 160 scene whose coarse displacements fall into four margin groups (Rc = 24, max_shift = 4)."""
    seed, ny, nx, count = xr.COARSE_SCENES[0]
    p = rr.blobs(seed, ny, nx, count)
    d = [(0.2, -0.3), (3.3, -2.1), (8.2, 7.9), (9.4, -1.2), (17.1, 5.3), (-23.8, 3.3)]
    return rr.scene(p), np.stack([rr.scene(p, x) for x in d]), np.array(d)


def test_margin_groups_calls_and_independence(monkeypatch, grouped):
    """The margin rule 8 ceil(|c| / 8) + max_shift + 2 groups the pairs: one order-1 copy and one window call per group -- at most
    Rc / 8 + 1 -- then the refinement per group with the same margin; the copies are displaced by the integers c, the refinement
    shifts the ORIGINAL images by the totals; every pair equals the twin of the whole method; a pair alone gives the same bits; a
    pair with c = 0 gives the bits of the plain path."""
    from rescan_line_sted_amd import registration as reg
    monkeypatch.setattr(reg, '_Device', _CoarseDevice)
    ref, imgs, d = grouped
    n_pix = 160 * 160
    s0, i0 = reg.estimate_shifts(imgs, ref, max_shift=4, refine=0, coarse=24)
    log = _CoarseDevice.log
    assert [c[1:] for c in log if c[0] == 'xcorr'] == [([0] * 6, [k * n_pix for k in range(6)], 24)]
    assert np.array_equal(i0['coarse'], np.rint(d).astype(np.int64)) and i0['coarse'].dtype == np.int64
    assert list(reg.coarse_margin(i0['coarse'], 4)) == [6, 14, 14, 22, 30, 30]
    sums = [c for c in log if c[0] == 'sums']
    assert [(c[2], c[3], c[4]) for c in sums] == [([0], 4, 6), ([0, n_pix], 4, 14), ([0], 4, 22), ([0, n_pix], 4, 30)] and len(sums) <= 24 // 8 + 1
    assert [c[1] for c in sums] == [[0], [0, 0], [0], [0, 0]]
    copies = [c for c in log if c[0] == 'shift']
    assert all(c[2] == 1 and c[3] is None for c in copies) and np.array_equal(np.concatenate([c[4] for c in copies]), i0['coarse'].astype(np.float64))
    assert not i0['at_limit'].any() and not i0['flat'].any() and not i0['coarse_flat'].any() and i0['coarse_snr'].min() > 5.0
    s1, i1 = reg.estimate_shifts(imgs, ref, max_shift=4, refine=1, coarse=24)
    log = _CoarseDevice.log
    fine = [c for c in log if c[0] == 'sums' and c[3] == 1]
    assert [c[4] for c in fine] == [6, 14, 22, 30] and len([c for c in log if c[0] == 'sums']) == 8
    cubic = [c for c in log if c[0] == 'shift' and c[2] == 3]
    assert np.array_equal(np.concatenate([c[4] for c in cubic]), s0)       # the original image by c + peak + parabola
    assert np.abs(s1 - d).max() < 0.01 and np.abs(s0 - d).max() < 0.06
    for k in range(6):
        for refine, s, info in ((0, s0, i0), (1, s1, i1)):
            w, wi = xr.estimate(imgs[k], ref, 24, 4, refine)
            assert np.array_equal(s[k], w) and info['ncc'][k] == wi['ncc'] and info['coarse_value'][k] == wi['coarse_value']
    alone, ia = reg.estimate_shifts(imgs[4], ref, max_shift=4, refine=1, coarse=24)
    assert alone[0].tobytes() == s1[4].tobytes() and ia['ncc'][0] == i1['ncc'][4] and ia['coarse_snr'][0] == i1['coarse_snr'][4]
    plain, ip = reg.estimate_shifts(imgs[:1], ref, max_shift=4, refine=1)
    assert plain[0].tobytes() == s1[0].tobytes() and ip['ncc'][0] == i1['ncc'][0]
    both, ib = reg.estimate_shifts(imgs, ref, max_shift=4, refine=0, coarse=24, surfaces=True)
    assert ib['surfaces'].shape == (6, 9, 9) and both.tobytes() == s0.tobytes()


@pytest.mark.parametrize('refine', [0, 1])
def test_two_stage_estimate_recovers_large_displacements(monkeypatch, refine):
    """The committed scenes displaced by up to 40 px, coarse = 48, max_shift = 4, through the wrapper on the stand-in: 0.06 px
    without refinement, 0.01 px with one pass -- what section 5i states for the plain method at small displacements.  The same call
    without coarse is wrong by more than a pixel for every displacement beyond its window, and reports at_limit for all of them but
    one, whose window holds a spurious interior maximum."""
    from rescan_line_sted_amd import registration as reg
    monkeypatch.setattr(reg, '_Device', _CoarseDevice)
    d = np.array(xr.COARSE_DISPLACEMENTS)
    for seed, ny, nx, count in xr.COARSE_SCENES:
        p = rr.blobs(seed, ny, nx, count)
        imgs = np.stack([rr.scene(p, x) for x in d])
        s, info = reg.estimate_shifts(imgs, rr.scene(p), max_shift=xr.COARSE_MAX_SHIFT, refine=refine, coarse=xr.COARSE_RADIUS)
        err = np.abs(s - d).max()
        print('scene %d refine %d: worst error %.4f px, least snr %.1f' % (seed, refine, err, info['coarse_snr'].min()))
        assert err <= (0.01 if refine else 0.06) and not info['at_limit'].any() and not info['flat'].any()
        assert np.abs(info['coarse'] - d).max() <= 0.5
        if refine == 0:
            ps, plain = reg.estimate_shifts(imgs, rr.scene(p), max_shift=xr.COARSE_MAX_SHIFT, refine=0)
            beyond = np.abs(d).max(axis=1) > xr.COARSE_MAX_SHIFT
            assert np.all(np.abs(ps - d).max(axis=1)[beyond] > 1.0) and not plain['at_limit'][~beyond].any()
            assert plain['at_limit'][beyond].sum() >= beyond.sum() - 1      # (39.6, 38.2): a spurious interior maximum, NOT flagged


def test_coarse_argument_errors_and_coarse_shifts(monkeypatch):
    from rescan_line_sted_amd import line_sted_tools, registration as reg
    assert line_sted_tools.coarse_shifts is reg.coarse_shifts
    monkeypatch.setattr(reg, '_Device', _CoarseDevice)
    a = np.zeros((2, 64, 64), dtype=np.float32)
    for kwargs in (dict(coarse=0), dict(coarse=-3), dict(coarse=2.5), dict(coarse=23),               # 64 - 2 (23 + 4 + 2) = 6 < 8
                   dict(coarse=8, margin=14), dict(coarse=8, max_shift=33), dict(coarse=8, max_shift=0), dict(coarse=8, refine=-1)):
        with pytest.raises(ValueError):
            reg.estimate_shifts(a, a[0], **{**dict(max_shift=4), **kwargs})
    reg._check_coarse(64, 64, 22, 4, None)
    big = np.zeros((1, 1140, 60), dtype=np.float32)
    with pytest.raises(ValueError, match='1152'):
        reg.estimate_shifts(big, big[0], max_shift=4, coarse=13)                                     # 1140 + 13 > 1152
    frames, truth, roi = _drifting_stack(F=2)
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    for kwargs in (dict(coarse=0), dict(coarse=30), dict(coarse=8, max_shift=33)):
        with pytest.raises(ValueError):
            reg.deconvolve_stack_registered(frames, psfs, 1, **{**dict(roi=roi, max_shift=2), **kwargs})
    for args in ((a, a[0], 0), (a, a[0], 33), (a, a[0], 2.5), (a.astype(np.int16), a[0], 4), (a, a[0, :30], 4), (big, big[0], 13)):
        with pytest.raises(ValueError):
            reg.coarse_shifts(*args)
    p = rr.blobs(3, 48, 64)
    c, info = reg.coarse_shifts(np.stack([rr.scene(p, (11.0, -14.0)), np.full((48, 64), 5.0)]), rr.scene(p), 20, surfaces=True)
    assert c.tolist() == [[11, -14], [0, 0]] and info['flat'].tolist() == [False, True] and info['snr'][0] > 5.0 and info['snr'][1] == 0.0
    assert info['surfaces'].shape == (2, 41, 41) and info['surfaces'].dtype == np.float32 and info['value'][1] == 0.0
    assert info['snr'][0] == xr.snr(xr.xcorr(rr.scene(p), rr.scene(p, (11.0, -14.0)), 20)[0], 20)


def test_registered_stack_takes_the_coarse_stage_for_views_and_frames(monkeypatch):
    """F = 3, V = 2, batch = 2 on the stand-in with coarse = 8, max_shift = 2: one xcorr call for the views (on frame 0) and one
    per chunk for the frames; the applied shift is the sum of the two and close to the truth although the view offset (1.6, -2.2)
    and the drift exceed what max_shift = 2 alone finds; given shifts=, no xcorr call is made."""
    from rescan_line_sted_amd import registration as reg
    monkeypatch.setattr(reg, '_Device', _CoarseDevice)
    frames, truth, roi = _drifting_stack(F=3)
    psfs = [rr.gaussian_psf(0.9, 1.5, 5), rr.gaussian_psf(1.5, 0.9, 5)]
    n_pix = 48 * 64
    est, info = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, batch=2, dtype='f64', max_shift=2, coarse=8)
    calls = _CoarseDevice.log
    xc = [c for c in calls if c[0] == 'xcorr']
    assert [c[1:3] for c in xc] == [([0], [n_pix]), ([0, n_pix], [2 * n_pix, 3 * n_pix]), ([0, n_pix], [0, n_pix])] and all(c[3] == 8 for c in xc)
    assert np.abs(info['shifts'] - truth).max() < 0.12 and not info['at_limit'].any() and not info['view_at_limit'].any()
    assert info['view_coarse'].tolist() == [[0, 0], [2, -2]] and info['coarse'].shape == (3, 2, 2) and info['coarse'].dtype == np.int64
    assert info['coarse_snr'][1:].min() > 2.0 and info['view_coarse_snr'][1] > 2.0      # (a 17 x 17 window inside the blobs' own width)
    final = [c for c in calls if c[0] == 'shift' and c[1] == 4]
    assert len(final) == 2 and np.array_equal(final[0][4].reshape(2, 2, 2), info['shifts'][:2])
    est2, info2 = reg.deconvolve_stack_registered(frames, psfs, 1, roi=roi, batch=2, dtype='f64', shifts=info['shifts'], coarse=8)
    assert not [c for c in _CoarseDevice.log if c[0] in ('xcorr', 'sums')] and est2.tobytes() == est.tobytes() and 'coarse' not in info2
