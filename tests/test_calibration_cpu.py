"""Camera calibration without a GPU (include/rlsted.h rl_calib_*, rl_repair_pixels, rl_stack_set_defects;
rescan_line_sted_amd/calibration.py): the bodies of the accumulate, finalize and repair kernels emulated thread by thread at the
launchers' geometry (tests/emu/calib_emu.cpp) against the twin (tests/calibration_reference.py) -- integer sums equal as integers,
the maps bit for bit the correctly rounded rationals, the repair bit for bit; the same bodies as a stand-alone program under the
address and undefined-behaviour sanitizers; the device build's private segments; the argument checks of the C ABI that need no
device; and the Python functions on a numpy stand-in for the device with a synthetic camera.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import calibration_reference as cr
import ingest_reference as ir
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'calib_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('calib_kernels.hpp', 'ingest_kernels.hpp', 'tile_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
SENSOR, PITCH, ROI = 17, 32, (3, 5, 13, 21)          # 17 x 29 pixels in rows of 32; a partial last vector, an unaligned origin


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libcalib_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.emu_calib_parts.argtypes = [i, i, i, i]
    lib.emu_calib_accumulate.argtypes = [vp, i, i, i, i, i, i, i, i, vp, vp, ll, i]
    lib.emu_calib_finalize.argtypes = [i, vp, vp, ll, ll, vp, vp]
    lib.emu_repair.argtypes = [vp, i, i, i, i, vp, i, vp]
    return lib


def frames_of(rng, dtype, F, sy=SENSOR, pitch=PITCH):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.integers(0, 256, (F, sy, pitch)).astype(dtype)
    if dtype == np.uint16:
        a = rng.integers(0, 65536, (F, sy, pitch)).astype(dtype)
        a[rng.random(a.shape) < 0.05] = 65535
        return a
    if dtype == np.int16:
        return rng.integers(-32768, 32768, (F, sy, pitch)).astype(dtype)       # negative values included
    return (rng.random((F, sy, pitch)) * 4000.0 - 200.0).astype(dtype)


def accumulate(emu, frames, roi, calls, parts=0):
    """The frames in `calls` consecutive runs through the emulated kernel: (S, Q, parts used per call)."""
    y0, x0, ny, nx = roi
    integer = frames.dtype != np.float32
    S, Q = np.zeros((ny, nx), dtype=np.int64 if integer else np.float64), np.zeros((ny, nx), dtype=np.uint64 if integer else np.float64)
    done, used = 0, []
    for n in calls:
        chunk = np.ascontiguousarray(frames[done:done + n])
        used.append(emu.emu_calib_accumulate(_p(chunk), cr.RAW[frames.dtype], frames.shape[1], frames.shape[2], y0, x0, ny, nx, n, _p(S), _p(Q), done, parts))
        assert used[-1] >= 1
        done += n
    return S, Q, used


# ---- accumulate --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int16])
def test_emulated_integer_sums_are_the_twins_integers(emu, dtype):
    """17 x 29 sensor, pitch 32, window 13 x 21 at (3, 5); F = 1, 2, 7 in one call and F = 7 as 3 + 4; the launcher's split (one
    part at these sizes) and a forced frame split of 2 and 3 parts: S and Q equal the Python-integer sums."""
    rng = np.random.default_rng(3)
    frames = frames_of(rng, dtype, 7)
    if np.dtype(dtype) == np.int16:
        assert (frames < 0).any()
    for F, calls in ((1, (1,)), (2, (2,)), (7, (7,)), (7, (3, 4))):
        S, Q = cr.sums_int(frames[:F], ROI)
        for parts in (0, 2, 3):
            gotS, gotQ, used = accumulate(emu, frames[:F], ROI, calls, parts)
            assert used == [parts or 1] * len(calls)
            assert np.array_equal(gotS, cr.as_int64(S)) and np.array_equal(gotQ, cr.as_uint64(Q)), (F, calls, parts)
            assert all(int(a) == b for a, b in zip(gotS.ravel(), S.ravel())) and all(int(a) == b for a, b in zip(gotQ.ravel(), Q.ravel()))


def test_frame_split_engages_where_the_window_is_small(emu):
    """The launcher's own parts: 8 x 8 with F = 300 is 37 parts (1024 workgroups wanted, at least 8 frames a part); 512 x 512 with
    4096 frames is 8; 2048 x 2048 and float32 are never split.  The 8 x 8 run equals the twin."""
    assert emu.emu_calib_parts(8, 8, 300, 1) == 37 and emu.emu_calib_parts(8, 8, 7, 1) == 1 and emu.emu_calib_parts(8, 8, 300, 0) == 1
    assert emu.emu_calib_parts(512, 512, 4096, 1) == 8 and emu.emu_calib_parts(2048, 2048, 4096, 1) == 1
    rng = np.random.default_rng(5)
    frames = frames_of(rng, np.uint16, 300, 9, 11)
    S, Q = cr.sums_int(frames, (1, 2, 8, 8))
    gotS, gotQ, used = accumulate(emu, frames, (1, 2, 8, 8), (300,))
    assert used == [37] and np.array_equal(gotS, cr.as_int64(S)) and np.array_equal(gotQ, cr.as_uint64(Q))


def test_largest_numerator_does_not_overflow_and_frame_65536_is_refused(emu):
    """1 x 8 window of uint16, F = 65535, every pixel 0 in 32767 or 32768 frames and 65535 in the others: N = F Q - S^2 is the largest
    there is, F^2 65535^2 / 4, just under 2^62, from F Q just under 2^63 -- and the variance is the correctly rounded rational.  One frame more is refused and
    nothing is touched."""
    F = 65535
    frames = np.zeros((F, 1, 8), dtype=np.uint16)
    frames[:F // 2, :, :4] = 65535
    frames[F // 2:, :, 4:] = 65535
    S, Q = cr.sums_int(frames, (0, 0, 1, 8))
    N = [F * int(q) - int(s) ** 2 for s, q in zip(S.ravel(), Q.ravel())]
    assert 2 ** 61 < max(N) < 2 ** 62 < F * int(Q.ravel()[0]) < 2 ** 64
    gotS, gotQ, _ = accumulate(emu, frames, (0, 0, 1, 8), (40000, 25535))
    assert np.array_equal(gotS, cr.as_int64(S)) and np.array_equal(gotQ, cr.as_uint64(Q))
    mean, var = np.zeros((1, 8)), np.zeros((1, 8))
    emu.emu_calib_finalize(1, _p(gotS), _p(gotQ), F, 8, _p(mean), _p(var))
    want_mean, want_var = cr.stats_int(S, Q, F)
    assert mean.tobytes() == want_mean.tobytes() and np.all(cr.ulps(var, want_var) <= 2) and np.all(var > 0)
    keepS, keepQ = gotS.copy(), gotQ.copy()
    one = np.full((1, 1, 8), 7, dtype=np.uint16)
    assert emu.emu_calib_accumulate(_p(one), 1, 1, 8, 0, 0, 1, 8, 1, _p(gotS), _p(gotQ), F, 0) == -1
    assert emu.emu_calib_accumulate(_p(one), 1, 1, 8, 0, 0, 1, 8, 2, _p(gotS), _p(gotQ), F - 1, 0) == -1
    assert np.array_equal(gotS, keepS) and np.array_equal(gotQ, keepQ)
    f = np.zeros((1, 1, 8), dtype=np.float32)                           # (float32 has no such limit)
    assert emu.emu_calib_accumulate(_p(f), 3, 1, 8, 0, 0, 1, 8, 1, _p(np.zeros(8)), _p(np.zeros(8)), F, 0) == 1


def test_emulated_float_sums_are_the_sequential_twin(emu):
    """float32: S and Q bit for bit the sequential float64 loop, in one call and as 3 + 4 (a forced split is ignored: the order is
    the definition); one nan and one inf poison their pixels only."""
    rng = np.random.default_rng(7)
    frames = frames_of(rng, np.float32, 7)
    frames[2, 3 + 4, 5 + 6] = np.nan
    frames[5, 3 + 9, 5 + 20] = np.inf
    S, Q = cr.sums_f32(frames, ROI)
    for calls in ((7,), (3, 4)):
        gotS, gotQ, used = accumulate(emu, frames, ROI, calls, 3)
        assert used == [1] * len(calls) and gotS.tobytes() == S.tobytes() and gotQ.tobytes() == Q.tobytes()
    bad = ~np.isfinite(S) | ~np.isfinite(Q)
    assert np.array_equal(np.argwhere(bad), [[4, 6], [9, 20]])
    mean, var = np.zeros(S.shape), np.zeros(S.shape)
    emu.emu_calib_finalize(3, _p(gotS), _p(gotQ), 7, S.size, _p(mean), _p(var))
    want_mean, want_var, _ = cr.stats_f32(S, Q, 7)
    assert mean.tobytes() == want_mean.tobytes() and var.tobytes() == want_var.tobytes()
    assert np.array_equal(~np.isfinite(mean) | ~np.isfinite(var), bad)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int16])
def test_emulated_finalize_is_correctly_rounded(emu, dtype):
    """mean and variance bit for bit the correctly rounded exact rationals (here N < 2^53, so that its conversion is exact and the
    one division rounds once); F = 1 gives variance 0; either map may be left out."""
    rng = np.random.default_rng(9)
    frames = frames_of(rng, dtype, 7)
    if np.dtype(dtype) == np.uint16:
        frames = (frames >> 4).astype(dtype)                             # (12-bit data: N stays below 2^53)
    for F in (1, 2, 7):
        S, Q = cr.sums_int(frames[:F], ROI)
        assert max(F * int(q) - int(s) ** 2 for s, q in zip(S.ravel(), Q.ravel())) < 2 ** 53
        S64, Q64 = cr.as_int64(S), cr.as_uint64(Q)
        mean, var = np.full(S.shape, np.nan), np.full(S.shape, np.nan)
        emu.emu_calib_finalize(cr.RAW[np.dtype(dtype)], _p(S64), _p(Q64), F, S64.size, _p(mean), _p(var))
        want_mean, want_var = cr.stats_int(S, Q, F)
        assert mean.tobytes() == want_mean.tobytes() and var.tobytes() == want_var.tobytes(), F
        if F == 1:
            assert np.all(var == 0.0)
        else:
            w = cr.window(frames[:F], ROI).astype(np.float64)
            assert np.allclose(var, w.var(axis=0, ddof=1), rtol=1e-12, atol=1e-9)
        only = np.full(S.shape, np.nan)
        emu.emu_calib_finalize(cr.RAW[np.dtype(dtype)], _p(S64), _p(Q64), F, S64.size, None, _p(only))
        assert only.tobytes() == want_var.tobytes()


# ---- repair ----------------------------------------------------------------------------------------------------------------------

def _sentinel(shape, dtype):
    whole = np.full(int(np.prod(shape)) + 32, 7777, dtype=dtype)
    return whole, whole[16:-16].reshape(shape)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_emulated_repair_is_the_twin(emu, dtype):
    """Every case of calibration_reference.repair_cases at 20 x 23, three images, in place, sentinels around the buffer: the images
    bit for bit the twin's, `unrepaired` its count, good pixels untouched; the 7 x 7 block's centre stays at radius 3, its inner
    3 x 3 at radius 2; a mask without defects writes nothing."""
    rng = np.random.default_rng(12)
    ny, nx = 20, 23
    images = (rng.random((3, ny, nx)) * 500.0).astype(dtype)
    images[1, 0, 1] = images[1, 1, 0]                                    # (equal candidates at a corner)
    for name, (mask, radius, left) in cr.repair_cases(ny, nx).items():
        want, want_left = cr.repair(images, mask, radius)
        assert want_left == left, name
        whole, buf = _sentinel(images.shape, dtype)
        buf[...] = images
        got_left = ctypes.c_longlong(-1)
        m8 = np.ascontiguousarray(mask).view(np.uint8)
        listed = emu.emu_repair(_p(buf), 0 if np.dtype(dtype) == np.float32 else 1, 3, ny, nx, _p(m8), radius, ctypes.byref(got_left))
        assert listed == mask.sum() - left and got_left.value == left, name
        assert buf.tobytes() == want.tobytes(), name
        assert np.all(whole[:16] == 7777) and np.all(whole[-16:] == 7777)
        assert np.array_equal(buf[:, ~mask], images[:, ~mask])
        if name.startswith('block7'):
            cy, cx = ny // 2, nx // 2
            assert np.array_equal(buf[:, cy, cx], images[:, cy, cx]) and not np.array_equal(buf[:, cy - 3, cx - 3], images[:, cy - 3, cx - 3])
        if name == 'none':
            assert listed == 0 and buf.tobytes() == images.tobytes()
        if name == 'even':
            a = np.sort(images[0, 0:2, nx // 2 - 1:nx // 2 + 2][~mask[0:2, nx // 2 - 1:nx // 2 + 2]])
            assert a.size == 4 and buf[0, 0, nx // 2] == dtype((np.float64(a[1]) + np.float64(a[2])) * 0.5)
    assert emu.emu_repair(_p(images), 0, 3, ny, nx, _p(np.zeros((ny, nx), dtype=np.uint8)), 4, None) == -1


# ---- sanitizers, the device build ------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation as a program of its own under -fsanitize=address,undefined, run directly: frames, accumulators, maps, images
    and masks are heap blocks of exactly their byte counts, the window ends with the sensor frame, the first and the last pixel of
    every image are defects."""
    exe = str(tmp_path / 'calib_emu_san')
    subprocess.check_call(['g++', '-DCALIB_EMU_MAIN', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 192 72', r.stdout


def test_calibration_kernels_do_not_spill(tmp_path):
    """calib_kernels.hip compiled device-only with the flags of _build.py: the eight kernels (ACCUMULATE x 4 raw types, FINALIZE x 2,
    REPAIR x 2) have `.private_segment_fixed_size` 0 and use no LDS."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'calib_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'calib_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    lds = [int(x) for x in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', txt)]
    assert len(priv) == 8 and sum('k_calib_accumulate<' in k for k in priv) == 4 and sum('k_calib_finalize<' in k for k in priv) == 2, priv
    assert sum('k_repair<' in k for k in priv) == 2 and all(v == 0 for v in priv.values()) and lds == [0] * 8, (priv, lds)


# ---- the C ABI's argument checks (no device is touched before them) ----------------------------------------------------------------

def test_the_library_refuses_bad_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert {'rl_calib_create', 'rl_calib_accumulate', 'rl_calib_frames', 'rl_calib_sums', 'rl_calib_finalize', 'rl_calib_reset',
            'rl_calib_destroy', 'rl_repair_pixels', 'rl_stack_set_defects'} <= set(_lib.PROTOTYPES)
    ctx, dev = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)                  # (never dereferenced)
    out = ctypes.c_void_p()
    good = dict(ctx=ctx, rdt=1, sny=17, pitch=32, y0=3, x0=5, ny=13, nx=21, out=ctypes.byref(out))
    for change in (dict(ctx=None), dict(out=None), dict(rdt=4), dict(rdt=-1), dict(sny=0), dict(pitch=0), dict(ny=0), dict(nx=0), dict(y0=-1),
                   dict(x0=-1), dict(y0=5), dict(x0=12), dict(ny=18), dict(nx=33)):
        a = {**good, **change}
        assert L.rl_calib_create(a['ctx'], a['rdt'], a['sny'], a['pitch'], a['y0'], a['x0'], a['ny'], a['nx'], a['out']) == -1, change
        assert L.rl_last_error() != b'' and not out.value
    frames = ctypes.c_longlong()
    assert L.rl_calib_accumulate(None, dev, 1) == -1 and L.rl_calib_frames(None, ctypes.byref(frames)) == -1
    assert L.rl_calib_sums(None, dev, dev) == -1 and L.rl_calib_finalize(None, dev, dev) == -1 and L.rl_calib_reset(None) == -1
    assert L.rl_calib_destroy(None) == 0
    mask = np.zeros((8, 16), dtype=np.uint8)
    mask[2, 3] = 1
    good = dict(ctx=ctx, img=dev, dt=0, n=2, ny=8, nx=16, mask=_p(mask), r=3)
    for change in (dict(ctx=None), dict(img=None), dict(mask=None), dict(dt=2), dict(dt=-1), dict(n=0), dict(ny=0), dict(nx=0), dict(r=0), dict(r=4),
                   dict(ny=1 << 16, nx=1 << 15)):
        a = {**good, **change}
        assert L.rl_repair_pixels(a['ctx'], a['img'], a['dt'], a['n'], a['ny'], a['nx'], a['mask'], a['r'], None) == -1, change
    # a mask without repairable defects: the count comes back and nothing is launched (the context is not even looked at)
    left = (ctypes.c_longlong * 2)(-1, -1)
    assert L.rl_repair_pixels(ctx, dev, 1, 2, 8, 16, _p(np.zeros((8, 16), dtype=np.uint8)), 3, left) == 0 and list(left) == [0, 0]
    assert L.rl_repair_pixels(ctx, dev, 1, 2, 8, 16, _p(np.ones((8, 16), dtype=np.uint8)), 3, left) == 0 and list(left) == [128, 128]
    assert L.rl_stack_set_defects(None, _p(mask), 3) == -1


# ---- the Python layer on a numpy stand-in ----------------------------------------------------------------------------------------

def test_camera_model_defects_checks():
    from rescan_line_sted_amd import calibration, line_sted_tools, stack
    for name in ('temporal_stats', 'find_defects', 'photon_transfer', 'calibrate_camera', 'repair_defects'):
        assert getattr(line_sted_tools, name) is getattr(calibration, name)
    cam = stack.CameraModel(dark=100.0)
    assert cam.defects is None and cam.repair_radius == 3 and cam.defect_info() == {'defects': 0, 'unrepaired': 0}
    cam.check_window(5, 7)
    mask = np.zeros((10, 13), dtype=bool)
    mask[1:8, 2:9] = True
    cam = stack.CameraModel(defects=mask, repair_radius=3)
    assert cam.defects.dtype == np.uint8 and cam.defects.shape == (10, 13) and cam.defect_info() == {'defects': 49, 'unrepaired': 1}
    assert stack.CameraModel(defects=mask, repair_radius=2).defect_info() == {'defects': 49, 'unrepaired': 9}
    cam.check_window(10, 13)
    with pytest.raises(ValueError):
        cam.check_window(13, 10)
    for bad in (mask.astype(np.uint8), mask.astype(np.float64), mask[0], mask[None], np.zeros((0, 4), dtype=bool)):
        with pytest.raises(ValueError):
            stack.CameraModel(defects=bad)
    for r in (0, 4, 1.5):
        with pytest.raises(ValueError):
            stack.CameraModel(defects=mask, repair_radius=r)
    for name, (m, radius, left) in cr.repair_cases(20, 23).items():
        assert calibration.unrepairable(m, radius).sum() == left, name


def _check_calibration(camera, report, cam):
    """The assertions of the synthetic camera (shared with the device test): gain within 2 % of 0.46 -- eight times the worst of the
    eight seeds of the numpy prototype (0.25 %); the estimate's own scatter from 4 levels x 3072 pixels x 96 frames is about 0.2 % --
    the dark map within 6 sigma_read / sqrt(F) of the truth on good pixels, the planted pixels found exactly."""
    from rescan_line_sted_amd import calibration
    print('gain %.5f (truth %.2f), read noise %.3f, residual %.4f' % (camera.gain, cam.GAIN, report['read_noise'], report['transfer']['residual']))
    assert abs(camera.gain - cam.GAIN) <= 0.02 * cam.GAIN
    assert np.array_equal(report['mask'], cam.planted) and np.array_equal(camera.defects != 0, cam.planted)
    for p in cam.hot:
        assert report['reasons'][p] & calibration.HOT
    for p in cam.dead:
        assert report['reasons'][p] == calibration.DEAD
    good = ~cam.planted
    err = np.abs(camera.dark_map.astype(np.float64) - cam.dark)[good].max()
    print('dark map: largest error on good pixels %.3f counts, bound %.3f' % (err, 6 * cam.READ / np.sqrt(cam.frames)))
    assert camera.dark_map.dtype == np.float32 and camera.dark_map.shape == cam.shape and err <= 6 * cam.READ / np.sqrt(cam.frames)
    assert abs(report['read_noise'] - cam.READ) < 0.15 * cam.READ and report['top'] == 3 and report['defects'] == 5
    assert camera.saturation == 65535.0 and camera.repair_radius == 3 and report['frames'] == [cam.frames] * 5


@pytest.mark.parametrize('seed', [0, 1])
def test_calibrate_camera_on_the_stand_in(monkeypatch, seed):
    from rescan_line_sted_amd import calibration
    monkeypatch.setattr(calibration, '_Device', cr.NumpyDevice)
    cam = cr.Camera(seed)
    dark, levels = cam.stacks()
    camera, report = calibration.calibrate_camera(dark, levels, saturation=65535)
    _check_calibration(camera, report, cam)
    assert cr.NumpyDevice.log == [('open', 1, cam.shape, (0, 0) + cam.shape), ('accumulate', cam.frames), ('close',)]
    # the pieces on their own, a window of the sensor, several chunks
    roi = (4, 8, 40, 48)
    mean, var, info = calibration.temporal_stats(dark.reshape(4, 24, 48, 64), roi=roi, chunk_frames=40)
    assert info['frames'] == 96 and info['chunks'] == 3 and info['nonfinite'] == 0 and set(info['times']) == {'wall_ms', 'upload_ms', 'kernel_ms'}
    assert cr.NumpyDevice.log == [('open', 1, (48, 64), roi), ('accumulate', 40), ('accumulate', 40), ('accumulate', 16), ('close',)]
    assert mean.tobytes() == np.ascontiguousarray(report['dark_mean'][4:44, 8:56]).tobytes() and mean.shape == (40, 48)
    mask, reasons = calibration.find_defects((report['dark_mean'], report['dark_var']))
    assert np.array_equal(np.argwhere(mask), sorted(cam.hot)) and np.all(reasons[mask] == calibration.HOT)       # (no top level: no dead pixels)
    tr = calibration.photon_transfer((report['dark_mean'], report['dark_var']), report['levels'], report['mask'], saturation=65535)
    # (a pixel's variance over 96 frames scatters by sqrt(2 / 95) = 14.5 %, a bin of at least 16 pairs by at most 3.7 %: four of
    # those standard deviations bound the largest of up to 32 bins; the camera itself is linear)
    assert tr['gain'] == report['gain'] and tr['residual'] < 4 * np.sqrt(2 / 95) / np.sqrt(16) and tr['count'].sum() <= tr['pairs'] == 4 * (48 * 64 - 5)
    bad_var = report['dark_var'].copy()
    bad_var[7, 7], bad_var[8, 8] = np.nan, 50.0
    mask, reasons = calibration.find_defects((report['dark_mean'], bad_var), report['levels'][3])
    assert reasons[7, 7] == calibration.INVALID and reasons[8, 8] == calibration.NOISY and mask.sum() == 7


def test_calibration_argument_errors(monkeypatch):
    from rescan_line_sted_amd import calibration
    monkeypatch.setattr(calibration, '_Device', cr.NumpyDevice)
    raw = np.zeros((4, 6, 8), dtype=np.uint16)
    for bad in (raw.astype(np.float64), raw.astype(np.int32), raw[0, 0]):
        with pytest.raises(ValueError):
            calibration.temporal_stats(bad)
    for kwargs in (dict(roi=(0, 0, 7, 8)), dict(roi=(-1, 0, 2, 2)), dict(chunk_frames=0)):
        with pytest.raises(ValueError):
            calibration.temporal_stats(raw, **kwargs)
    with pytest.raises(ValueError):
        calibration.temporal_stats(np.zeros((65536, 1, 1), dtype=np.uint8))
    mean, var, info = calibration.temporal_stats(raw[:1])
    assert np.all(var == 0) and info['chunks'] == 1
    with pytest.raises(ValueError):
        calibration.calibrate_camera(raw, [raw])
    with pytest.raises(TypeError):
        calibration.calibrate_camera(raw, [raw, raw], sigma=3)
    with pytest.raises(ValueError):
        calibration.repair_defects(np.zeros((2, 6, 8)), np.zeros((6, 8), dtype=np.uint8))
    with pytest.raises(ValueError):
        calibration.repair_defects(np.zeros((2, 6, 8)), np.zeros((6, 7), dtype=bool))
    with pytest.raises(ValueError):
        calibration.repair_defects(np.zeros((2, 6, 8)), np.zeros((6, 8), dtype=bool), radius=4)
    rng = np.random.default_rng(0)
    img = rng.random((2, 3, 6, 8)).astype(np.float32)
    mask = np.zeros((6, 8), dtype=bool)
    mask[2, 3] = True
    out = calibration.repair_defects(img, mask, radius=1)
    assert out.dtype == np.float32 and out.shape == img.shape and out is not img
    assert np.array_equal(out.reshape(6, 6, 8), cr.repair(img.reshape(6, 6, 8), mask, 1)[0])


# ---- deconvolve_stack on the stand-in ----------------------------------------------------------------------------------------------

from test_stack_cpu import _NumpyStack, _oracle, _psf, raw_frames, GAIN      # noqa: E402  (the stand-in of the stack tests)


class _NumpyStackWithDefects(_NumpyStack):
    """_NumpyStack plus rl_stack_set_defects: the twin's repair between the twin's ingest and the oracle."""
    defects = None

    def set_defects(self, mask, radius):
        self.defects = (mask.copy(), radius)
        self.calls.append(('set_defects', mask.dtype, mask.shape, radius))

    def run(self, raw, frames, iterations, out, ingest_stats, export_stats, times):
        if self.defects is None:
            return super().run(raw, frames, iterations, out, ingest_stats, export_stats, times)
        c, V, B, (ny, nx) = self.cfg, self.V, self.batch, self.shape
        images = raw.reshape((-1,) + tuple(c['sensor']))
        cam = c['camera']
        assert c['order'] == 0
        for first in range(0, frames, B):
            nt = min(B, frames - first)
            meas, stats = ir.ingest(images[first * V:(first + nt) * V], B, nt, V, ny, nx, c['origin'][0], c['origin'][1], V, 1, cam.dark_map, cam.dark,
                                    cam.gain, cam.epsilon, 0.0, np.float64)
            meas = cr.repair(meas.reshape(B * V, ny, nx), *self.defects)[0].reshape(B, V, ny, nx)
            self.calls.append(('chunk', first, nt, meas.copy()))
            out[first:first + nt] = np.stack([_oracle(m, self.psfs, iterations) for m in meas])[:nt]
            ingest_stats[first:first + nt] = stats.reshape(B, V, 4)[:nt]
        times[:] = [4.0, 1.0, 2.0, 0.5]


def test_deconvolve_stack_repairs_between_ingest_and_iterations(monkeypatch):
    """With defects the wrapper hands the map to the pipeline after open and before run, and the estimates are the oracle's on the
    ingested-then-repaired measurement; the statistics stay the ingest's.  With defects=None it makes the calls it made before."""
    from rescan_line_sted_amd import stack
    monkeypatch.setattr(stack, '_Device', _NumpyStackWithDefects)
    rng = np.random.default_rng(8)
    F, V, sy, sx = 3, 2, 14, 19
    psfs = [_psf(rng), _psf(rng)]
    raw = raw_frames(rng, np.uint16, (F, V, sy, sx))
    roi = (2, 3, 10, 13)
    mask = np.zeros((10, 13), dtype=bool)
    mask[4, 5] = mask[0, 0] = mask[9, 11] = mask[9, 12] = True
    raw[:, :, 2 + 4, 3 + 5] = 60000                                        # a hot pixel
    cam = stack.CameraModel(dark=100.0, gain=GAIN, defects=mask, repair_radius=2)
    est, info = stack.deconvolve_stack(raw, psfs, 2, camera=cam, roi=roi, batch=2, out_dtype='f64')
    calls = _NumpyStackWithDefects.log
    assert [c[0] for c in calls] == ['plan', 'open', 'set_defects', 'chunk', 'chunk', 'close'] and calls[2][1:] == (np.uint8, (10, 13), 2)
    meas, stats = ir.measurement(raw, V, 'frame-view', roi, 100.0, GAIN, 0.0)
    fixed = cr.repair(meas.reshape(F * V, 10, 13), mask, 2)[0].reshape(F, V, 10, 13)
    assert fixed[:, :, 4, 5].max() < 3000 and meas[:, :, 4, 5].min() > 20000
    assert np.array_equal(est, np.stack([_oracle(m, psfs, 2) for m in fixed]))
    assert np.array_equal(info['level'], stats[:, :, 0]) and info['defects'] == 4 and info['unrepaired'] == 0
    plain = stack.CameraModel(dark=100.0, gain=GAIN)
    est0, info0 = stack.deconvolve_stack(raw, psfs, 2, camera=plain, roi=roi, batch=2, out_dtype='f64')
    assert [c[0] for c in _NumpyStackWithDefects.log] == ['plan', 'open', 'chunk', 'chunk', 'close']
    assert np.array_equal(est0, np.stack([_oracle(m, psfs, 2) for m in meas])) and info0['defects'] == 0 and info0['unrepaired'] == 0
    with pytest.raises(ValueError):
        stack.deconvolve_stack(raw, psfs, 2, camera=cam, batch=2)             # the map is the window's, not the sensor's
