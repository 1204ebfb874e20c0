"""The bead measurement without a GPU (include/rlsted.h rl_find_peaks; rescan_line_sted_amd/beads.py): the peak finder's bodies
emulated phase by phase at the launcher's geometry (tests/emu/bead_emu.cpp) against the numpy twin (tests/beads_reference.py) bit
for bit on constructed images; the same bodies as a stand-alone program under the address and undefined-behaviour sanitizers; the
device build's private segments; the argument checks; the wrappers on a numpy stand-in for the device; the method against the
analytic truth.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import beads_reference as br
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'bead_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('bead_kernels.hpp', 'fft_core.hpp')]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libbead_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.emu_find_peaks.argtypes = [vp, i, vp, i, i, i, vp, i, i, i, d, d, i, vp, vp, vp, vp, vp]
    return lib


SENTINEL = -7


def emu_peaks(emu, images, w, r, b, rel, threshold, cap, offsets=None, buf=None):
    """images: list of (ny, nx) arrays of one dtype, laid out consecutively (or `buf` at `offsets`); returns per image the dict of
    beads_reference.find_peaks cut to cap, and checks that the entries past min(count, cap) kept their sentinels."""
    ny, nx = images[0].shape
    n = len(images)
    if buf is None:
        buf = np.concatenate([np.ravel(a) for a in images])
        offsets = [k * ny * nx for k in range(n)]
    off = np.asarray(offsets, dtype=np.int64)
    yx = np.full((n, cap, 2), SENTINEL, dtype=np.intc)
    sv, xv = np.full((n, cap), float(SENTINEL)), np.full((n, cap), float(SENTINEL))
    cnt, lev = np.full(n, SENTINEL, dtype=np.int64), np.full((n, 3), float(SENTINEL))
    h = (len(w) - 1) // 2
    w = np.ascontiguousarray(w, dtype=np.float64)
    assert emu.emu_find_peaks(_p(buf), int(buf.dtype == np.float64), _p(off), n, ny, nx, _p(w), h, r, b, rel, threshold, cap, _p(yx), _p(sv),
                              _p(xv), _p(cnt), _p(lev)) == 0
    out = []
    for i in range(n):
        k = min(int(cnt[i]), cap)
        assert np.all(yx[i, k:] == SENTINEL) and np.all(sv[i, k:] == SENTINEL) and np.all(xv[i, k:] == SENTINEL)
        out.append({'yx': yx[i, :k].astype(np.int64), 's': sv[i, :k].copy(), 'x': xv[i, :k].copy(), 'count': int(cnt[i]), 'levels': lev[i].copy()})
    return out


def same(got, want, cap):
    k = min(want['count'], cap)
    assert got['count'] == want['count'], (got['count'], want['count'])
    assert got['levels'].tobytes() == want['levels'].tobytes(), (got['levels'], want['levels'])
    assert np.array_equal(got['yx'], want['yx'][:k]), (got['yx'], want['yx'][:k])
    assert got['s'].tobytes() == want['s'][:k].tobytes()
    assert got['x'].tobytes() == want['x'][:k].tobytes()


def scene_cases():
    """(name, images, w, r, b, rel, threshold, cap): every case of the issue's list."""
    x, marks, b = br.seam_scene()
    w, h = br.taps(0.6)
    assert h == 2 and b == 5
    out = [('seam_scene', [x], w, 3, b, 0.2, 0.0, 64)]
    out.append(('cap_overflow', [x], w, 3, b, 0.2, 0.0, 3))
    # s == t exactly: the threshold is the s of the in-D border peak, which must stay a candidate
    t_exact = float(br.smooth(x, w)[marks['border_in']])
    out.append(('s_equals_t', [x], w, 3, b, 0.0, t_exact, 64))
    x0 = br.h0_scene()
    out.append(('h0', [x0], np.array([1.0]), 1, 1, 0.5, 0.0, 200))
    one = np.random.default_rng(1).integers(0, 9, size=(2 * 5 + 1, 2 * 5 + 1)).astype(np.float64)
    one[5, 5] = 30.0
    out.append(('one_pixel_domain', [one], w, 3, 5, 0.2, 0.0, 4))
    out.append(('flat', [np.full((br.TY + 13, br.TX + 11), 3.25)], w, 3, 5, 0.2, 0.0, 8))
    # more than one image with different levels, a candidate exactly at border distance b in each
    y = x.copy()
    y[np.isnan(y)] = 1.0
    out.append(('two_images', [x, 2.0 * y + 1.0], w, 3, b, 0.25, 0.0, 64))
    return out


CASES = scene_cases()


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_emulated_finder_is_the_twin_bit_for_bit(emu, case, dtype):
    """Candidates (row-major), s, x, the true count and (lo, hi, t) of the emulated kernels against the twin, f32 and f64 inputs
    holding the same values (every value here is exact in float32)."""
    name, images, w, r, b, rel, thr, cap = case
    imgs = [np.asarray(a, dtype=dtype) for a in images]
    assert all(np.array_equal(a.astype(np.float64), b_, equal_nan=True) for a, b_ in zip(imgs, images))
    got = emu_peaks(emu, imgs, w, r, b, rel, thr, cap)
    for g, a in zip(got, imgs):
        same(g, br.find_peaks(a, w, r, b, rel, thr), cap)


def test_constructed_cases_mean_what_they_say():
    """The twin's own answers: one candidate per plateau, at its first pixel, inside a tile and across the seam; ties resolve to the
    pixel that comes first; the peak at distance b is a candidate, the one at b - 1 is not; the nan peak is not; s == t is kept;
    h = 0 makes s the input bit for bit; a flat image has none; the cap case overflows."""
    x, marks, b = br.seam_scene()
    w, _ = br.taps(0.6)
    S = br.smooth(x, w)
    got = br.find_peaks(x, w, 3, b, 0.2, 0.0)
    pos = [tuple(p) for p in got['yx']]
    for name in ('plateau', 'plateau_seam'):
        y0, x0 = marks[name]
        assert S[y0, x0] == S[y0 + 2, x0 + 2] and marks[name] in pos, name
        assert not any(y0 <= p[0] <= y0 + 2 and x0 <= p[1] <= x0 + 2 and p != marks[name] for p in pos), name
    assert marks['plateau_seam'][1] < b + br.TX <= marks['plateau_seam'][1] + 2
    for win, lose in (('tie_after', 'tie_loser_after'), ('tie_before', 'tie_loser_before')):
        assert S[marks[win]] == S[marks[lose]] and marks[win] in pos and marks[lose] not in pos, win
    assert marks['border_in'] in pos and marks['border_last'] in pos and marks['border_out'] not in pos
    assert marks['nan_peak'] not in pos
    assert got['count'] > 3 and np.all(got['s'] >= got['levels'][2])
    t_exact = float(S[marks['border_in']])
    e = br.find_peaks(x, w, 3, b, 0.0, t_exact)
    assert e['levels'][2] == t_exact and marks['border_in'] in [tuple(p) for p in e['yx']] and e['s'].min() == t_exact
    x0 = br.h0_scene()
    assert br.smooth(x0, np.array([1.0])).tobytes() == x0.tobytes()
    assert br.find_peaks(np.full((br.TY + 13, br.TX + 11), 3.25), w, 3, 5, 0.2, 0.0)['count'] == 0


def test_layout_does_not_change_an_image(emu):
    """Non-contiguous offsets in any order, an image alone or among others: the same bits."""
    x, _, b = br.seam_scene()
    w, _ = br.taps(0.6)
    y = np.nan_to_num(x, nan=2.0)[::-1].copy()
    ny, nx = x.shape
    buf = np.full(5 * ny * nx + 37, 1e30)
    offs = [3 * ny * nx + 37, 11]
    buf[offs[0]:offs[0] + ny * nx] = x.ravel()
    buf[offs[1]:offs[1] + ny * nx] = y.ravel()
    both = emu_peaks(emu, [x, y], w, 3, b, 0.2, 0.0, 16, offsets=offs, buf=buf)
    for img, g in zip((x, y), both):
        same(g, br.find_peaks(img, w, 3, b, 0.2, 0.0), 16)
        alone = emu_peaks(emu, [img], w, 3, b, 0.2, 0.0, 16)[0]
        assert alone['yx'].tobytes() == g['yx'].tobytes() and alone['s'].tobytes() == g['s'].tobytes()


# ---- sanitizers -------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulated finder as a program of its own under -fsanitize=address,undefined, run directly: images, taps, outputs, tile
    partials and masks are heap blocks of exactly their byte counts and the LDS exactly the kernel's; f32 and f64, partial tiles,
    the largest LDS (h = r = 16) with a one-pixel domain, h = 0, cap overflow; candidates held to a plain loop."""
    exe = str(tmp_path / 'bead_emu_san')
    subprocess.check_call(['g++', '-DBEAD_EMU_MAIN', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 4', r.stdout


def test_lds_stays_within_64_kb(emu):
    assert emu.emu_lds_bytes(16, 16) == 65536 and emu.emu_lds_bytes(0, 0) >= 2 * 256 * 8
    assert (emu.emu_tile(0), emu.emu_tile(1)) == (br.TY, br.TX)


# ---- the device build -------------------------------------------------------------------------------------------------------------

def test_bead_kernels_do_not_spill(tmp_path):
    """bead_kernels.hip compiled device-only with the flags of _build.py: the four kernels have `.private_segment_fixed_size` 0."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'bead_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'bead_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = re.findall(r'\.name:\s+(\S+)', txt)
    priv = [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]
    kern = dict(zip(names, priv))
    assert sorted(kern) == sorted('_ZN2rl%d%sENS_6BpArgsE' % (len(k), k) for k in ('k_peaks_range', 'k_peaks_levels', 'k_peaks_mark',
                                                                                    'k_peaks_compact')), kern
    assert all(v == 0 for v in kern.values()), kern


# ---- argument checks --------------------------------------------------------------------------------------------------------------

def test_the_library_declares_and_checks_its_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert len(_lib.PROTOTYPES['rl_find_peaks'][1]) == 19
    header = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_find_peaks(' in header and '#define RL_PEAK_LEVELS 3' in header
    ctx, src = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)          # (never dereferenced)
    off, neg = (ctypes.c_int64 * 2)(0, 5000), (ctypes.c_int64 * 2)(0, -1)
    w = (ctypes.c_double * 33)(*([0.0] * 33))
    yx = (ctypes.c_int32 * 64)()
    sv, xv, lev = (ctypes.c_double * 32)(), (ctypes.c_double * 32)(), (ctypes.c_double * 6)()
    cnt = (ctypes.c_int64 * 2)()
    good = dict(ctx=ctx, src=src, dt=0, off=off, n=2, ny=40, nx=50, w=w, h=2, r=3, b=5, rel=0.2, thr=0.0, cap=16, yx=yx, sv=sv, xv=xv,
                cnt=cnt, lev=lev)
    for change in (dict(ctx=None), dict(src=None), dict(off=None), dict(w=None), dict(yx=None), dict(sv=None), dict(xv=None), dict(cnt=None),
                   dict(lev=None), dict(dt=2), dict(dt=-1), dict(n=0), dict(h=-1), dict(h=17, b=40, ny=90, nx=90), dict(r=0), dict(r=17, b=20),
                   dict(b=4), dict(ny=10), dict(nx=10), dict(off=neg), dict(cap=0)):
        g = {**good, **change}
        rc = L.rl_find_peaks(g['ctx'], g['src'], g['dt'], g['off'], g['n'], g['ny'], g['nx'], g['w'], g['h'], g['r'], g['b'], g['rel'], g['thr'],
                             g['cap'], g['yx'], g['sv'], g['xv'], g['cnt'], g['lev'])
        assert rc == -1 and L.rl_last_error() != b'', change


# ---- the wrappers on the numpy stand-in -----------------------------------------------------------------------------------------------

@pytest.fixture
def numpy_device(monkeypatch):
    from rescan_line_sted_amd import beads
    made = []

    def make(device=0):
        d = br.NumpyDevice(device)
        made.append(d)
        return d
    monkeypatch.setattr(beads, '_Device', make)
    return made


def _camera(**kw):
    from rescan_line_sted_amd.stack import CameraModel
    return CameraModel(dark=100.0, gain=1.0, **kw)


def test_find_beads_hands_the_twin_its_taps_and_border(numpy_device):
    from rescan_line_sted_amd import beads
    x, _, _ = br.seam_scene()
    x = np.nan_to_num(x, nan=0.0)
    got, info = beads.find_beads(np.stack([x, x[::-1].copy()]), sigma=0.6, radius=3, rel_threshold=0.2, max_beads=4)
    w, h = br.taps(0.6)
    assert numpy_device[0].calls[0][2:] == (x.shape[0], x.shape[1], 2 * h + 1, 3, h + 3, 0.2, 0.0, 4)
    for k, img in enumerate((x, x[::-1])):
        want = br.find_peaks(img, w, 3, h + 3, 0.2, 0.0)
        assert np.array_equal(got[k], want['yx'][:4]) and info['counts'][k] == want['count'] > 4
        assert info['levels'][k].tobytes() == want['levels'].tobytes() and info['values'][k].tobytes() == want['s'][:4].tobytes()
    assert beads.gaussian_taps(0.6)[0].tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        beads.find_beads(x, border=h + 2, sigma=0.6)
    with pytest.raises(ValueError):
        beads.find_beads(x.astype(np.int32))


def _stack(F=1, ny=160, nx=192, edge=24, seed=3):
    return br.bead_stack(F, ny, nx, 21, False, seed=seed, spacing=24, edge=edge)


def test_rejection_reasons_are_counted_and_kept_out(numpy_device):
    """cap (past max_beads), separation (both of a close pair), saturated (the raw window), ncc (a wide blob among point beads), and
    none of them in the positions."""
    from rescan_line_sted_amd import beads
    raw, _ = _stack(F=2)
    raw = raw.astype(np.float32)
    raw[1, 0] += br.gauss_bead(160, 192, 60.2, 95.7, 1.3, 2.0, 5000.0).astype(np.float32)       # 11 px from the bead at (~48, ~96)... a pair
    raw[0, 0] += br.gauss_bead(160, 192, 120.0, 180.0 - 12.0, 4.0, 4.0, 60000.0).astype(np.float32)   # a wide blob
    raw[0, 1] += br.gauss_bead(160, 192, 84.0, 84.0, 2.0, 1.3, 2e5).astype(np.float32)          # saturates at 2000 counts
    psfs, info = beads.measure_psfs(raw, 21, camera=_camera(saturation=2000.0), max_beads=40, min_ncc=0.99)
    r0, r1 = info['rejected']
    assert r0['separation'] >= 2 and r0['ncc'] >= 1 and r1['saturated'] >= 1, info['rejected']
    assert r0['cap'] == 0
    psfs_c, info_c = beads.measure_psfs(raw, 21, camera=_camera(saturation=2000.0), max_beads=12, min_ncc=0.99)
    assert info_c['rejected'][0]['cap'] > 0 and info_c['rejected'][1]['cap'] > 0
    for v in range(2):
        pos = info['positions'][v]
        assert len(pos) == info['n_beads'][v] == len(info['ncc'][v]) == len(info['flux'][v])
        assert np.all(info['ncc'][v] >= 0.99)
        assert not np.any((pos[:, 0] == 0) & (np.abs(pos[:, 1] - 120.0) < 3) & (np.abs(pos[:, 2] - 168.0) < 3)) if v == 0 else True
        assert not np.any((pos[:, 0] == 0) & (np.abs(pos[:, 1] - 84.0) < 3) & (np.abs(pos[:, 2] - 84.0) < 3)) if v == 1 else True


def test_orders_give_the_same_bits_and_the_right_strides(numpy_device):
    from rescan_line_sted_amd import beads
    raw, _ = _stack(F=2)
    a, ia = beads.measure_psfs(raw, 21, camera=_camera(), order='frame-view')
    b, ib = beads.measure_psfs(np.ascontiguousarray(raw.transpose(1, 0, 2, 3)), 21, camera=_camera(), order='view-frame')
    ing = [c for d in numpy_device for c in d.calls if c[0] == 'ingest']
    assert ing[0][:6] == ('ingest', 4, 2, 1, 2, 2) and ing[1][:6] == ('ingest', 4, 1, 2, 2, 2)
    for v in range(2):
        assert a[v].tobytes() == b[v].tobytes() and ia['positions'][v].tobytes() == ib['positions'][v].tobytes()
    one, i1 = beads.measure_psfs(np.ascontiguousarray(raw[:, 1]), 21, camera=_camera())
    assert len(one) == 1 and one[0].tobytes() == a[1].tobytes()


def test_roi_offsets_the_positions(numpy_device):
    from rescan_line_sted_amd import beads
    raw, _ = _stack(F=1, ny=176, nx=208, edge=36)
    full, fi = beads.measure_psfs(raw, 21, camera=_camera())
    cut, ci = beads.measure_psfs(raw, 21, camera=_camera(), roi=(8, 12, 160, 188))
    for v in range(2):
        assert fi['n_beads'][v] == ci['n_beads'][v] > 10
        assert np.allclose(ci['positions'][v] + np.array([0.0, 8.0, 12.0]), fi['positions'][v], rtol=0.0, atol=1e-12)
        assert full[v].tobytes() == cut[v].tobytes()
    assert [c for c in numpy_device[1].calls if c[0] == 'ingest'][0][6:] == ((8, 12), (160, 188))


def test_output_is_what_deconvolve_takes(numpy_device):
    from rescan_line_sted_amd import _lib, beads
    raw, _ = _stack(F=1)
    psfs, info = beads.measure_psfs(raw, 21, camera=_camera())
    assert len(psfs) == 2 and all(p.shape == (1, 21, 21) and p.dtype == np.float64 and abs(p.sum() - 1.0) < 1e-12 and p.min() >= 0 for p in psfs)
    assert np.stack(_lib.common_psf_shape(psfs)).shape == (2, 1, 21, 21)       # (the plan's (V, py, px) stack)
    assert info['std'][0].shape == (1, 21, 21) and info['width'].shape == (2, 2) and info['margin'] == 10 and info['border'] == 20
    assert set(info['rejected'][0]) == set(beads.REASONS)


def test_bad_arguments_raise(numpy_device):
    from rescan_line_sted_amd import beads
    raw, _ = _stack(F=1)
    for kw in (dict(size=20), dict(size=3), dict(passes=0), dict(order='fv'), dict(roi=(0, 0, 170, 10)), dict(margin=3), dict(sigma=5.0),
               dict(radius=0), dict(max_beads=0), dict(max_shift=0)):
        with pytest.raises(ValueError):
            beads.measure_psfs(raw, **{'size': 21, **kw})
    with pytest.raises(ValueError):
        beads.measure_psfs(raw.astype(np.float64), 21)
    blank = np.full_like(raw, 100)
    blank[0, 0] = raw[0, 0]
    with pytest.raises(ValueError, match='view 1'):
        beads.measure_psfs(blank, 21, camera=_camera())
    with pytest.raises(ValueError, match='view 0'):
        beads.measure_psfs(raw, 21, camera=_camera(), min_ncc=1.5)


# ---- the method against the truth ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('noise', [False, True])
def test_method_against_the_truth(numpy_device, noise):
    """Analytic point-sampled anisotropic Gaussian beads, sigma (1.3, 2.0) and (2.0, 1.3), two views, size 21, sub-pixel centres at
    least 23 pixels apart.  Noise-free: 2 frames of 160 x 192, 60 beads per view; Poisson: 6 frames of 256 x 256, 600 beads per view,
    uint16, dark 100, gain 1, 5000 photons per bead, background 20 per pixel.  Caps: max|P - P_true| <= 0.02 max P_true, centroid
    within 0.05 px of the centre pixel, get_width within 2 % of the true FWHM.
    The twin (this path, on the numpy device) measured: noise-free 0.0028 / 0.0026 max P_true, centroid < 1e-7 px, width 0.22 % /
    0.20 %; Poisson 0.0061 / 0.0082 max P_true, centroid < 1.4e-4 px, width 0.20 % / 0.31 % -- each within half its cap."""
    from rescan_line_sted_amd import beads
    raw, truths = (br.bead_stack(2, 160, 192, 21, False, spacing=24, edge=24) if not noise else
                   br.bead_stack(6, 256, 256, 21, True, spacing=23, edge=24))
    psfs, info = beads.measure_psfs(raw, 21, camera=_camera())
    k = np.arange(21) - 10
    for v, (sy, sx) in enumerate(br.SIGMAS):
        P, T = psfs[v][0], truths[v]
        err = np.abs(P - T).max() / T.max()
        cy, cx = (P.sum(axis=1) * k).sum() / P.sum(), (P.sum(axis=0) * k).sum() / P.sum()
        wr = info['width'][v] / np.array([br.fwhm(sx), br.fwhm(sy)]) - 1.0
        print('view %d beads %d: max error %.4g of max, centroid (%.3g, %.3g) px, width %.4g %.4g' % (v, info['n_beads'][v], err, cy, cx, wr[0], wr[1]))
        assert info['n_beads'][v] >= 30
        assert err <= 0.02
        assert abs(cy) <= 0.05 and abs(cx) <= 0.05
        assert np.all(np.abs(wr) <= 0.02)
