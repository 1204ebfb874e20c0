"""Acquired camera stacks without a GPU (include/rlsted.h rl_ingest, rl_export, rl_stack_*; rescan_line_sted_amd/stack.py): the bodies
of k_ingest and k_export emulated thread by thread (tests/emu/ingest_emu.cpp) against the numpy twin (tests/ingest_reference.py) bit
for bit; the statistics' sums against the twin's same-order sum and math.fsum; half-to-even in the u16 export; the same bodies as a
stand-alone program under the address and undefined-behaviour sanitizers; the device build's private segments; the argument checks
of the C ABI that need no device; and the Python wrappers on a numpy stand-in for the device.  CPU only."""
import ctypes
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ingest_reference as ir
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'ingest_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('ingest_kernels.hpp', 'tile_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
FLOATS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
SHAPES = [(5, 13), (7, 16), (3, 33)]
ORIGINS = [(0, 0), (2, 1), (1, 5)]
GAIN = 0.4587


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libingest_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i, d, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    lib.emu_ingest.argtypes = [vp, i, i, i, i, i, ll, ll, i, i, i, i, i, vp, d, d, d, d, vp, i, vp, i]
    lib.emu_export.argtypes = [vp, i, i, i, i, d, vp, i, vp, i]
    lib.emu_ingest_blocks.argtypes = [i, i]
    lib.emu_export_blocks.argtypes = [i, i]
    return lib


def raw_frames(rng, dtype, shape):
    """Sensor frames with saturated pixels, pixels below the dark level and, in float32, nan and both infinities."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        a = rng.integers(60, 256, shape).astype(dtype)
    elif dtype == np.uint16:
        a = rng.integers(60, 4000, shape).astype(dtype)
        a[rng.random(shape) < 0.05] = 65535
    elif dtype == np.int16:
        a = rng.integers(-300, 4000, shape).astype(dtype)
        a[rng.random(shape) < 0.05] = 32767
    else:
        a = (rng.random(shape) * 4000.0 - 200.0).astype(dtype)
        r = rng.random(shape)
        a[r < 0.04] = np.nan
        a[(r >= 0.04) & (r < 0.07)] = np.inf
        a[(r >= 0.07) & (r < 0.10)] = -np.inf
        a[(r >= 0.10) & (r < 0.14)] = 65535.0
    return a


def saturation_of(dtype):
    return {1: 250.0, 2: 32767.0 if np.dtype(dtype) == np.int16 else 65535.0, 4: 65535.0}[np.dtype(dtype).itemsize]


def _guarded(n, dtype, shift):
    """n values starting `shift` elements into a 64-byte aligned block, with guard values around them."""
    raw = np.zeros(n + 64 + shift, dtype=dtype)
    start = (-raw.ctypes.data // raw.itemsize) % (64 // raw.itemsize)
    whole = raw[start:start + shift + n + 8]
    whole[:] = 7
    view = whole[shift:shift + n]
    assert view.ctypes.data % 64 == (shift * raw.itemsize) % 64
    return whole, view


# ---- the bodies against the twin -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dst_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('raw_dtype', [np.uint8, np.uint16, np.int16, np.float32])
def test_emulated_ingest_is_the_numpy_twin(emu, raw_dtype, dst_dtype):
    """Every TR x TD; shapes (5, 13), (7, 16), (3, 33) -- element stores, 16-byte stores, a partial last vector; src_pitch nx and
    nx + 3; three window origins; both view orders with V = 1 and 3; dark as a level and as a map; gain 0.4587; saturated,
    below-dark and (f32) nan / inf pixels; n_valid < n_slots; the destination aligned and at an odd element offset; the launcher's
    work split and a two-workgroup one: stored values and statistics bit for bit, nothing written around the destination."""
    rng = np.random.default_rng(11)
    sat = saturation_of(raw_dtype)
    seen = np.zeros(3)
    cases, ran = 0, set()
    for (ny, nx), pad, (y0, x0), V, view_frame, dark_map in itertools.product(SHAPES, (0, 3), ORIGINS, (1, 3), (False, True), (False, True)):
        cases += 1                                               # (the full product: nothing is thinned out)
        ran.add((V, view_frame, dark_map))
        n_slots, n_valid = 3, 2
        src_ny, src_pitch = y0 + ny + (cases % 2), x0 + nx + pad
        raw = raw_frames(rng, raw_dtype, (n_valid * V, src_ny, src_pitch))
        dark = (90.0 + rng.random((ny, nx)) * 30.0).astype(np.float32) if dark_map else None
        fs, vs = (1, n_valid) if view_frame else (V, 1)
        for nb in (None, 2):
            want, want_stats = ir.ingest(raw, n_slots, n_valid, V, ny, nx, y0, x0, fs, vs, dark, 100.25, GAIN, 1e-9, sat, dst_dtype, nb)
            for shift in (0, 1):
                whole, dst = _guarded(want.size, dst_dtype, shift)
                stats = np.full((n_slots * V, 4), np.nan)
                vec = emu.emu_ingest(_p(raw), ir.RAW[raw.dtype], src_ny, src_pitch, y0, x0, fs, vs, n_slots, n_valid, V, ny, nx, _p(dark), 100.25,
                                     GAIN, 1e-9, sat, _p(dst), FLOATS[np.dtype(dst_dtype)], _p(stats), 0 if nb is None else nb)
                assert vec == (1 if nx % 8 == 0 and shift == 0 else 0)
                assert dst.tobytes() == want.tobytes(), (ny, nx, pad, y0, x0, V, view_frame, dark_map, shift)
                assert stats.tobytes() == want_stats.tobytes(), (ny, nx, V, nb, stats, want_stats)
                assert np.all(whole[:shift] == 7) and np.all(whole[shift + want.size:] == 7)
        assert np.all(want[n_valid:] == 1) and np.all(want_stats[n_valid * V:, 0] == ny * nx) and np.all(want_stats[n_valid * V:, 1:] == 0)
        assert np.all(want[:n_valid] >= 0) and np.all(np.isfinite(want))
        seen += want_stats[:, 1:].sum(axis=0)
    assert seen[0] > 0 and seen[1] > 0 and (seen[2] > 0) == (np.dtype(raw_dtype) == np.float32), seen      # clipped, saturated, invalid
    # both orders at V = 3 (where they are different addressing: strides (3, 1) and (1, 2)) and at V = 1, each with both dark forms
    assert ran == set(itertools.product((1, 3), (False, True), (False, True))) and cases == 3 * 2 * 3 * 8


def test_ingest_without_statistics_and_in_more_workgroups(emu):
    """stats = NULL writes the same pixels; a 70 x 260 image is three workgroups of the launcher's own split, its sum bit for bit the
    twin's and within n * 2^-53 * sum |v| of math.fsum."""
    rng = np.random.default_rng(2)
    ny, nx = 70, 260
    raw = raw_frames(rng, np.uint16, (1, ny + 1, nx + 5))
    assert emu.emu_ingest_blocks(ny, nx) == 3 == ir.blocks(ny * 33) and emu.emu_ingest_blocks(40, 48) == 1
    for dst_dtype in (np.float32, np.float64):
        want, want_stats = ir.ingest(raw, 1, 1, 1, ny, nx, 1, 2, 1, 1, None, 99.5, GAIN, 1e-9, 65535.0, dst_dtype)
        dst, stats = np.zeros((ny, nx), dtype=dst_dtype), np.zeros((1, 4))
        emu.emu_ingest(_p(raw), 1, ny + 1, nx + 5, 1, 2, 1, 1, 1, 1, 1, ny, nx, None, 99.5, GAIN, 1e-9, 65535.0, _p(dst), FLOATS[np.dtype(dst_dtype)], _p(stats), 0)
        assert dst.tobytes() == want.tobytes() and stats.tobytes() == want_stats.tobytes()
        again = np.zeros_like(dst)
        emu.emu_ingest(_p(raw), 1, ny + 1, nx + 5, 1, 2, 1, 1, 1, 1, 1, ny, nx, None, 99.5, GAIN, 1e-9, 65535.0, _p(again), FLOATS[np.dtype(dst_dtype)], None, 0)
        assert again.tobytes() == want.tobytes()
        values = want.astype(np.float64).ravel()
        exact = math.fsum(values)
        bound = values.size * 2.0 ** -53 * math.fsum(np.abs(values))
        print('ingest sum: device order %.17g, fsum %.17g, bound %.3e' % (stats[0, 0], exact, bound))
        assert abs(stats[0, 0] - exact) <= bound


@pytest.mark.parametrize('out_dtype', [np.float32, np.float64, np.uint16])
@pytest.mark.parametrize('est_dtype', [np.float32, np.float64])
def test_emulated_export_is_the_numpy_twin(emu, est_dtype, out_dtype):
    """Every est x TO at the three shapes, the output aligned and at an odd offset, nan, negative and overflowing estimates: values
    and statistics bit for bit; the sums within n * 2^-53 * sum |v| of math.fsum."""
    rng = np.random.default_rng(4)
    for (ny, nx), nb in itertools.product(SHAPES, (None, 2)):
        est = (rng.random((3, ny, nx)) * 900.0 - 50.0).astype(est_dtype)
        est[1, 0, :4] = [np.nan, -3.0, 70000.0, 65535.2]
        want, want_stats = ir.export(est, 80.5, out_dtype, nb)
        for shift in (0, 1):
            whole, out = _guarded(want.size, out_dtype, shift)
            stats = np.full((3, 2), np.nan)
            vec = emu.emu_export(_p(est), FLOATS[est.dtype], 3, ny, nx, 80.5, _p(out), ir.OUT[np.dtype(out_dtype)], _p(stats), 0 if nb is None else nb)
            assert vec == (1 if (ny * nx) % 8 == 0 and (shift * np.dtype(out_dtype).itemsize) % 16 == 0 else 0)
            assert out.tobytes() == want.tobytes(), (ny, nx, shift)
            assert stats.tobytes() == want_stats.tobytes()
            assert np.all(whole[:shift] == 7) and np.all(whole[shift + want.size:] == 7)
        if np.dtype(out_dtype) == np.uint16:
            y = est.astype(np.float64) * 80.5
            assert np.array_equal(want_stats[:, 1], (y > 65535.0).reshape(3, -1).sum(axis=1)) and want_stats[:, 1].sum() > 0
            assert want[1, 0, 0] == 0 and want[1, 0, 1] == 0 and want[1, 0, 2] == 65535
        for i in (0, 2):
            values = est[i].astype(np.float64).ravel()
            assert abs(want_stats[i, 0] - math.fsum(values)) <= values.size * 2.0 ** -53 * math.fsum(np.abs(values))
        assert np.isnan(want_stats[1, 0])


def test_u16_export_rounds_half_to_even(emu):
    """k + 0.5 for even and odd k: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ..., 65534.5 -> 65534; 65535.5 is above 65535: clamped, counted."""
    k = np.concatenate([np.arange(0, 40), np.arange(65500, 65536)]).astype(np.float64)
    for est_dtype in (np.float32, np.float64):
        est = (k + 0.5).astype(est_dtype).reshape(1, 4, 19)
        assert np.array_equal(est.astype(np.float64).ravel(), k + 0.5)            # (exact in float32 too)
        out, stats = np.zeros((1, 4, 19), dtype=np.uint16), np.zeros((1, 2))
        emu.emu_export(_p(est), FLOATS[est.dtype], 1, 4, 19, 1.0, _p(out), 2, _p(stats), 0)
        want = np.where(k % 2 == 0, k, k + 1)
        want[-1] = 65535
        assert np.array_equal(out.ravel(), want.astype(np.uint16)) and stats[0, 1] == 1
        assert np.array_equal(ir.export(est, 1.0, np.uint16)[0], out)


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation as a program of its own under -fsanitize=address,undefined, run directly: raw, dark, destination and output are
    heap blocks of exactly their byte counts, and the window ends with the sensor frame -- the unaligned last run of the last row
    of the last image ends at the buffer's last byte."""
    exe = str(tmp_path / 'ingest_emu_san')
    subprocess.check_call(['g++', '-DINGEST_EMU_MAIN', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok 576 18', r.stdout


# ---- the device build of the same bodies -----------------------------------------------------------------------------------------

def test_ingest_kernels_do_not_spill(tmp_path):
    """ingest_kernels.hip compiled device-only with the flags of _build.py: the fifteen kernels (INGEST x 4 raw types x 2, EXPORT x 2
    x 3, the totals) have `.private_segment_fixed_size` 0."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'ingest_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'ingest_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = subprocess.run(['c++filt'], input='\n'.join(re.findall(r'\.name:\s+(\S+)', txt)), capture_output=True, text=True).stdout.split('\n')
    priv = dict(zip(names, [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)]))
    assert len(priv) == 15 and sum('k_ingest<' in k for k in priv) == 8 and sum('k_export<' in k for k in priv) == 6, priv
    assert sum('k_ingest_totals' in k for k in priv) == 1 and all(v == 0 for v in priv.values()), priv


# ---- the C ABI's argument checks (no device is touched before them) ----------------------------------------------------------------

def test_the_library_refuses_bad_arguments_before_any_launch():
    from rescan_line_sted_amd import _lib
    L = _lib.lib
    assert set(['rl_ingest', 'rl_export', 'rl_stack_create', 'rl_stack_run', 'rl_stack_destroy']) <= set(_lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES['rl_ingest'][1]) == 23 and len(_lib.PROTOTYPES['rl_export'][1]) == 10
    ctx, raw, dst = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)      # (never dereferenced)
    good = dict(ctx=ctx, raw=raw, rdt=1, images=6, sny=10, pitch=20, y0=1, x0=2, fs=3, vs=1, slots=2, valid=2, V=3, ny=8, nx=16, dark=None,
                offset=100.0, gain=0.5, eps=1e-9, sat=0.0, dst=dst, ddt=0, stats=None)
    bad = [dict(ctx=None), dict(raw=None), dict(dst=None), dict(rdt=4), dict(rdt=-1), dict(ddt=2), dict(images=0), dict(slots=0), dict(V=0), dict(ny=0),
           dict(nx=0), dict(sny=0), dict(pitch=0), dict(valid=3), dict(valid=-1), dict(y0=3), dict(x0=5), dict(y0=-1), dict(x0=-1), dict(fs=4),
           dict(vs=2), dict(fs=-1), dict(images=5), dict(gain=0.0), dict(gain=-1.0), dict(gain=float('inf')), dict(gain=float('nan')),
           dict(eps=-1e-9), dict(eps=float('nan')), dict(offset=float('nan')), dict(dst=ctypes.c_void_p(0x100000 + 64)),
           dict(dst=ctypes.c_void_p(0x100000 - 64))]
    for change in bad:
        a = {**good, **change}
        rc = L.rl_ingest(a['ctx'], a['raw'], a['rdt'], a['images'], a['sny'], a['pitch'], a['y0'], a['x0'], a['fs'], a['vs'], a['slots'], a['valid'],
                         a['V'], a['ny'], a['nx'], a['dark'], a['offset'], a['gain'], a['eps'], a['sat'], a['dst'], a['ddt'], a['stats'])
        assert rc == -1 and L.rl_last_error() != b'', change
    est, out = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)
    for args in ((None, est, 0, 2, 8, 16, 1.0, out, 0, None), (ctx, None, 0, 2, 8, 16, 1.0, out, 0, None), (ctx, est, 0, 2, 8, 16, 1.0, None, 0, None),
                 (ctx, est, 2, 2, 8, 16, 1.0, out, 0, None), (ctx, est, 0, 2, 8, 16, 1.0, out, 3, None), (ctx, est, 0, 0, 8, 16, 1.0, out, 0, None),
                 (ctx, est, 0, 2, 0, 16, 1.0, out, 0, None), (ctx, est, 0, 2, 8, 0, 1.0, out, 0, None), (ctx, est, 0, 2, 8, 16, float('nan'), out, 0, None),
                 (ctx, est, 0, 2, 8, 16, 1.0, ctypes.c_void_p(0x100000 + 512), 2, None)):
        assert L.rl_export(*args) == -1, args
    assert L.rl_stack_create(None, None, None) == -1 and L.rl_stack_run(None, None, 1, 1, None, None, None, None) == -1
    assert L.rl_stack_destroy(None) == 0
    assert L.rl_device_upload_bytes(None, est, out, 8) == -1 and L.rl_device_upload_bytes(ctx, None, out, 8) == -1
    assert L.rl_device_upload_bytes(ctx, est, None, 8) == -1 and L.rl_device_upload_bytes(ctx, None, None, 0) == 0


# ---- wrapper logic ---------------------------------------------------------------------------------------------------------------

def _oracle(meas, psfs, iterations):
    import tile_reference as tr
    return np.asarray(tr.oracle_estimate(meas, psfs, iterations))


class _NumpyStack:
    """Stands in for stack._Device: rl_stack_run's contract in numpy -- chunks of the batch, a short last chunk filled with ones
    frames, the twin's ingest and export, the oracle as the plan; records what the wrapper asked for.  (Its chunk loop is its own:
    nothing asserted about it says anything about the C pipeline.)"""
    log = None

    def __init__(self, psfs, batch, shape, dtype, device, acceleration, tv_lambda, tv_epsilon):
        self.psfs, self.batch, self.shape, self.V = psfs, batch, tuple(shape), len(psfs)
        type(self).log = self.calls = [('plan', batch, tuple(shape), dtype)]

    def open(self, raw_dtype, order, sensor, origin, camera, out_dtype, out_scale):
        self.cfg = dict(raw_dtype=raw_dtype, order=order, sensor=sensor, origin=origin, camera=camera, out_dtype=out_dtype, out_scale=out_scale)
        self.calls.append(('open', dict(self.cfg)))

    def run(self, raw, frames, iterations, out, ingest_stats, export_stats, times):
        c, V, B, (ny, nx) = self.cfg, self.V, self.batch, self.shape
        assert raw.dtype in ir.RAW and ir.RAW[raw.dtype] == c['raw_dtype'] and raw.flags.c_contiguous
        images = raw.reshape((-1,) + tuple(c['sensor']))
        cam = c['camera']
        for first in range(0, frames, B):
            nt = min(B, frames - first)
            if c['order'] == 0:
                chunk, fs, vs = images[first * V:(first + nt) * V], V, 1
            else:
                chunk, fs, vs = np.concatenate([images[v * frames + first:v * frames + first + nt] for v in range(V)]), 1, nt
            meas, stats = ir.ingest(chunk, B, nt, V, ny, nx, c['origin'][0], c['origin'][1], fs, vs, cam.dark_map, cam.dark, cam.gain, cam.epsilon,
                                    0.0 if cam.saturation is None else cam.saturation, np.float64)
            self.calls.append(('chunk', first, nt, meas.copy()))
            est = np.stack([_oracle(m, self.psfs, iterations) for m in meas])
            got, estats = ir.export(est, c['out_scale'], out.dtype)
            out[first:first + nt] = got[:nt]
            ingest_stats[first:first + nt] = stats.reshape(B, V, 4)[:nt]
            export_stats[first:first + nt] = estats[:nt]
        times[:] = [4.0, 1.0, 2.0, 0.5]

    def unresolved(self):
        return 0

    def strategy(self):
        return {}

    def close(self):
        self.calls.append(('close',))


def _psf(rng, shape=(5, 5)):
    p = rng.random(shape) + 0.1
    return (p / p.sum())[None]


@pytest.mark.parametrize('order', ['frame-view', 'view-frame'])
def test_wrapper_chunks_orders_roi_and_statistics(monkeypatch, order):
    """What the WRAPPER does with F = 5, batch = 2, both orders and a window: the plan it asks for, the parameters it hands to the
    pipeline (dtype code, order code, sensor, origin, camera, output), the array it passes on untouched, `info['chunks']`, and the
    statistics taken apart per frame and view.  The chunk loop and the ones fillers are rl_stack_run's, in C: here they are the
    STAND-IN's own loop (written to that call's contract so that the wrapper's inputs and outputs can be checked against the twin
    and the oracle), so the assertions on the chunks (0, 2), (2, 2), (4, 1) and on the filler check the stand-in, not product code.
    The product's chunking, slot reuse and fillers are checked on the device (tests/test_gpu_stack.py, F = 5, batch = 2), the
    filler slots of the kernel body in test_emulated_ingest_is_the_numpy_twin (n_valid < n_slots)."""
    from rescan_line_sted_amd import line_sted_tools, stack
    assert line_sted_tools.deconvolve_stack is stack.deconvolve_stack and line_sted_tools.CameraModel is stack.CameraModel
    monkeypatch.setattr(stack, '_Device', _NumpyStack)
    rng = np.random.default_rng(8)
    F, V, sy, sx = 5, 2, 14, 19
    psfs = [_psf(rng), _psf(rng)]
    frames = raw_frames(rng, np.uint16, (F, V, sy, sx))
    frames[3, 1, 4, 5:9] = 20                                     # below the dark level
    raw = frames if order == 'frame-view' else np.ascontiguousarray(frames.transpose(1, 0, 2, 3))
    roi = (2, 3, 10, 13)
    dark = (95.0 + rng.random((10, 13)) * 10.0).astype(np.float32)
    cam = stack.CameraModel(dark=dark, gain=GAIN, saturation=65535)
    est, info = stack.deconvolve_stack(raw, psfs, 2, camera=cam, order=order, roi=roi, batch=2, out_dtype='f64')
    calls = _NumpyStack.log
    assert [c[0] for c in calls] == ['plan', 'open', 'chunk', 'chunk', 'chunk', 'close'] and calls[0][1:] == (2, (10, 13), 'f32')
    cfg = calls[1][1]
    assert cfg['raw_dtype'] == 1 and cfg['order'] == (0 if order == 'frame-view' else 1) and cfg['sensor'] == (sy, sx) and cfg['origin'] == (2, 3)
    assert cfg['out_dtype'] == 1 and cfg['camera'] is cam
    assert [(c[1], c[2]) for c in calls if c[0] == 'chunk'] == [(0, 2), (2, 2), (4, 1)]
    last = calls[4][3]
    assert last.shape == (2, V, 10, 13) and np.all(last[1] == 1.0)                      # the filler of the short last chunk
    want_meas, want_stats = ir.measurement(frames, V, 'frame-view', roi, dark, GAIN, 65535.0)
    assert np.array_equal(np.concatenate([c[3][:c[2]] for c in calls if c[0] == 'chunk']), want_meas)
    want = np.stack([_oracle(m, psfs, 2) for m in want_meas])
    assert est.shape == (F, 10, 13) and est.dtype == np.float64 and np.array_equal(est, want)
    assert info['chunks'] == 3 and info['batch'] == 2 and info['unresolved'] == 0 and info['times']['upload_ms'] == 1.0
    win = frames[:, :, 2:12, 3:16].astype(np.float64)
    assert np.array_equal(info['saturated'], (win >= 65535).sum(axis=(2, 3))) and info['saturated'].sum() > 0
    assert np.array_equal(info['clipped'], (win < dark.astype(np.float64)).sum(axis=(2, 3))) and info['clipped'][3, 1] >= 4
    assert info['invalid'].shape == (F, V) and not info['invalid'].any() and info['clipped'].dtype == np.int64
    assert np.array_equal(info['level'], want_stats[:, :, 0]) and info['flux'].shape == (F,) and not info['clamped'].any()
    for f in range(F):
        assert abs(info['flux'][f] - want[f].sum()) <= 1e-12 * want[f].sum()


def test_wrapper_single_view_u16_output_and_argument_errors(monkeypatch):
    from rescan_line_sted_amd import stack
    monkeypatch.setattr(stack, '_Device', _NumpyStack)
    rng = np.random.default_rng(9)
    psfs = [_psf(rng, (3, 3))]
    raw = raw_frames(rng, np.uint8, (3, 9, 12))                                      # (F, sy, sx): one view
    out = np.zeros((3, 9, 12), dtype=np.uint16)
    est, info = stack.deconvolve_stack(raw, psfs, 1, out_dtype='u16', out_scale=300.0, out=out, camera=stack.CameraModel(dark=50.0))
    assert est is out and info['chunks'] == 1 and info['batch'] == 3 and _NumpyStack.log[1][1]['raw_dtype'] == 0
    meas, _ = ir.measurement(raw, 1, dark=50.0)
    y = np.stack([_oracle(m, psfs, 1) for m in meas]) * 300.0
    assert np.array_equal(info['clamped'], (y > 65535.0).reshape(3, -1).sum(axis=1)) and info['clamped'].sum() > 0
    assert np.array_equal(out, np.where(y > 65535.0, 65535.0, np.rint(y)).astype(np.uint16))
    for bad in (raw.astype(np.float64), raw.astype(np.int32), raw.astype(np.uint32), raw.astype(np.int8), raw.astype(np.float16), raw.astype(bool)):
        with pytest.raises(ValueError):
            stack.deconvolve_stack(bad, psfs, 1)
    for kwargs in (dict(order='view'), dict(dtype='f16'), dict(out_dtype='u8'), dict(batch=0), dict(roi=(0, 0, 10, 12)), dict(roi=(-1, 0, 4, 4)),
                   dict(out=np.zeros((3, 9, 12))), dict(out=np.zeros((2, 9, 12), dtype=np.float32)), dict(acceleration='nesterov'),
                   dict(tv_lambda=0.5), dict(camera=stack.CameraModel(dark=np.zeros((4, 4))))):
        with pytest.raises(ValueError):
            stack.deconvolve_stack(raw, psfs, 1, **kwargs)
    with pytest.raises(ValueError):
        stack.deconvolve_stack(raw, psfs, -1)
    with pytest.raises(ValueError):
        stack.deconvolve_stack(raw[:, None].repeat(2, axis=1), psfs, 1)            # two views, one PSF
    for kwargs in (dict(gain=0.0), dict(gain=float('nan')), dict(epsilon=-1.0), dict(saturation=0.0), dict(dark=float('inf')), dict(dark=np.zeros(4))):
        with pytest.raises(ValueError):
            stack.CameraModel(**kwargs)


class _NumpyTiles:
    """tiling._Device's steps that come before the tiles, recorded; the run ends at the first gather."""

    class Done(Exception):
        pass
    log = None

    def __init__(self, *args):
        type(self).log = self.calls = []

    def alloc(self, elements):
        return ctypes.c_void_p(1)

    def upload(self, measurement):
        self.calls.append(('upload', measurement.dtype, measurement.shape))

    def upload_raw(self, raw, camera):
        self.calls.append(('upload_raw', raw.dtype, raw.shape, camera))

    def gather(self, slots):
        raise self.Done()

    def close(self):
        self.calls.append(('close',))


def test_tiled_wrapper_takes_raw_data_only_with_a_camera(monkeypatch):
    from rescan_line_sted_amd import stack, tiling
    monkeypatch.setattr(tiling, '_Device', _NumpyTiles)
    rng = np.random.default_rng(1)
    psfs = [_psf(rng, (3, 3))]
    raw = raw_frames(rng, np.uint16, (2, 1, 40, 30))
    cam = stack.CameraModel(dark=100.0, gain=GAIN)
    with pytest.raises(_NumpyTiles.Done):
        tiling.deconvolve_tiled(raw, psfs, 1, tile=16, overlap=8, margin=1, camera=cam)
    assert _NumpyTiles.log == [('upload_raw', np.dtype(np.uint16), (2, 1, 40, 30), cam), ('close',)]
    with pytest.raises(_NumpyTiles.Done):
        tiling.deconvolve_tiled(raw, psfs, 1, tile=16, overlap=8, margin=1)
    assert _NumpyTiles.log == [('upload', np.dtype(np.float64), (2, 1, 40, 30)), ('close',)]      # camera=None: the present path
    with pytest.raises(ValueError):
        tiling.deconvolve_tiled(raw.astype(np.float64), psfs, 1, tile=16, overlap=8, margin=1, camera=cam)
    with pytest.raises(ValueError):
        tiling.deconvolve_tiled(raw, psfs, 1, tile=16, overlap=8, margin=1, camera=stack.CameraModel(dark=np.zeros((4, 4))))
    import inspect
    assert list(inspect.signature(tiling.deconvolve_tiled).parameters)[-1] == 'camera'
