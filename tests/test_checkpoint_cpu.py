"""The iteration checkpoints without a GPU (include/rlsted.h rl_batch_submit_checkpoints): the bodies of k_checkpoint and
k_checkpoint_totals (rescan_line_sted_amd/csrc/checkpoint_kernels.hpp) emulated on the host thread by thread
(tests/emu/checkpoint_emu.cpp) against numpy long double under the derived bound (tests/checkpoint_reference.py); the same code as a
stand-alone program under the address and undefined-behaviour sanitizers; the compiled kernels' resources; and the arithmetic of the
Python readers on synthetic arrays.  CPU only."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import checkpoint_reference as cr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'checkpoint_emu.cpp')
DT = {'f32': 0, 'f64': 1}
NP = {'f32': np.float32, 'f64': np.float64}


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libcheckpoint_emu.so')
    deps = [SRC] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f) for f in ('checkpoint_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_checkpoint_blocks.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.emu_checkpoint.argtypes = [vp, vp, i, vp, i, ctypes.c_size_t, i, vp, vp]
    return lib


def _at(buf, shift):
    return ctypes.c_void_p(buf.ctypes.data + shift * buf.itemsize)


def _run(emu, est, obj, shift, n, frames, out_dtype=None, trace=True):
    """The emulated launch on `frames` frames of n pixels that start at element `shift` of the buffers est and obj.  Returns
    (dst [frames][n] or None, part [frames][nb][6] or None, out [frames][6] or None)."""
    dtype = 'f32' if est.dtype == np.float32 else 'f64'
    nb = emu.emu_checkpoint_blocks(n, est.itemsize)
    dst = np.full(shift + frames * n, -1.0, dtype=NP[out_dtype]) if out_dtype else None
    part = np.full((frames, nb, cr.FIELDS), np.nan) if trace else None
    out = np.full((frames, cr.FIELDS), np.nan) if trace else None
    got = emu.emu_checkpoint(_at(est, shift), _at(obj, shift), DT[dtype], _at(dst, shift) if out_dtype else None, DT[out_dtype or dtype], n, frames,
                             part.ctypes.data_as(ctypes.c_void_p) if trace else None, out.ctypes.data_as(ctypes.c_void_p) if trace else None)
    assert got == nb == cr.blocks(n, est.itemsize)
    if out_dtype:
        assert np.all(dst[:shift] == -1.0)
        dst = dst[shift:].reshape(frames, n)
    return dst, part, out


def _data(rng, dtype, n, frames, shift):
    obj = np.zeros(shift + frames * n, dtype=NP[dtype])
    est = np.zeros_like(obj)
    level = 200.0 * (0.2 + rng.random(frames * n))
    obj[shift:] = level
    est[shift:] = rng.poisson(level) + rng.random(frames * n)
    return est, obj


def test_the_work_split_is_the_accel_split(emu):
    """8192 f32 pixels (4096 f64 pixels) are one workgroup's run; one more vector opens a second workgroup."""
    assert emu.emu_checkpoint_threads() == 256 and emu.emu_checkpoint_fields() == cr.FIELDS == 6
    assert [emu.emu_checkpoint_blocks(n, 4) for n in (1, 8192, 8193, 2 * 8192 + 1)] == [1, 1, 2, 3]
    assert [emu.emu_checkpoint_blocks(n, 8) for n in (4096, 4097, 8193)] == [1, 2, 3]
    # the chain of the bound: a full workgroup's thread owns 8 vectors
    assert cr.chain_length(8192, 4) == 8 * 4 + 8 + 1 and cr.chain_length(4097, 8) == 5 * 2 + 8 + 2 and cr.chain_length(1, 4) == 4 + 8 + 1


CASES = [('f32', n) for n in (1, 8192, 8193, 2 * 8192 + 1, 40 * 48)] + [('f64', n) for n in (4096, 4097, 8193, 40 * 48)]


@pytest.mark.parametrize('dtype,n', CASES)
def test_emulated_kernels_match_long_double(emu, dtype, n):
    """Three frames at an odd and at an even element offset (both load paths) to a float32 and to a float64 destination: every
    field of every frame within gamma_(L + r) sum |terms| of long double, the cast output bit-exact, every pixel written."""
    rng = np.random.default_rng(1000 * n + DT[dtype])
    worst = 0.0
    for shift in (0, 1):
        est, obj = _data(rng, dtype, n, 3, shift)
        for out_dtype in ('f32', 'f64'):
            dst, part, out = _run(emu, est, obj, shift, n, 3, out_dtype)
            assert not np.isnan(out).any() and not np.isnan(part).any()
            assert np.array_equal(dst, est[shift:].reshape(3, n).astype(NP[out_dtype]))
            for f in range(3):
                x, t = est[shift + f * n:shift + (f + 1) * n], obj[shift + f * n:shift + (f + 1) * n]
                worst = max(worst, cr.check(out[f], x, t, est.itemsize, '%s -> %s n=%d shift=%d frame %d' % (dtype, out_dtype, n, shift, f)))
    print('%s n=%d: worst error / bound %.3g' % (dtype, n, worst))


def test_field_5_under_cancellation(emu):
    """x = T (1 + 1e-9) at T ~ 1e8, f64: the per-pixel difference keeps field 5 inside its bound where f2 - 2 f4 + f3, formed from
    the kernel's own fields 2 to 4, does not."""
    rng = np.random.default_rng(5)
    n = 40 * 48
    obj = 1e8 * (1.0 + rng.random(n))
    est = obj * (1.0 + 1e-9)
    _, _, out = _run(emu, est, obj, 0, n, 1)
    ref, bnd = cr.sums(est, obj), cr.bounds(est, obj, 8)
    direct = abs(float(cr.LD(out[0, 5]) - ref[5]))
    composite = abs(float(cr.LD(out[0, 2]) - 2 * cr.LD(out[0, 4]) + cr.LD(out[0, 3]) - ref[5]))
    print('field 5 = %.6g, bound %.3g: error of the direct form %.3g, of f2 - 2 f4 + f3 %.3g' % (float(ref[5]), bnd[5], direct, composite))
    cr.check(out[0], est, obj, 8, 'cancellation f64 n=%d' % n)
    assert direct <= bnd[5] < composite


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_partials_depend_on_the_frame_alone(emu, dtype):
    """A frame's partials and trace are the same bits alone, among other frames, and with or without a destination of either type;
    without a trace the destination is the same."""
    rng = np.random.default_rng(77)
    n = 2 * 8192 + 1 if dtype == 'f32' else 8193
    est, obj = _data(rng, dtype, n, 3, 1)
    dst, part, out = _run(emu, est, obj, 1, n, 3, 'f32')
    assert part.shape[1] == 3
    for f in range(3):
        _, p1, o1 = _run(emu, est, obj, 1 + f * n, n, 1)
        assert np.array_equal(p1[0], part[f]) and np.array_equal(o1[0], out[f]), f
    for out_dtype in (None, 'f64'):
        _, p2, o2 = _run(emu, est, obj, 1, n, 3, out_dtype)
        assert np.array_equal(p2, part) and np.array_equal(o2, out)
    d3, p3, o3 = _run(emu, est, obj, 1, n, 3, 'f32', trace=False)
    assert p3 is None and np.array_equal(d3, dst)


def test_emulation_under_sanitizers(tmp_path):
    """checkpoint_emu.cpp as a stand-alone program (its own main: exactly-sized buffers, frames at element offsets 0 to 3, all four
    type pairs, with and without destination and trace) built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / 'checkpoint_emu_main')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-ffp-contract=off',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DCHECKPOINT_EMU_MAIN', SRC, '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith('ok 288')


def test_kernels_do_not_spill_and_hold_only_the_tree(tmp_path):
    """checkpoint_kernels.hip compiled device-only with the flags of _build.py: the four instances of k_checkpoint and
    k_checkpoint_totals, no scratch, no spills, LDS = the tree's 6 x 256 doubles (none in the totals kernel)."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'checkpoint_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'checkpoint_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    assert len(re.findall(r'\.name:\s+\S*k_checkpointI\S*', txt)) == 4
    assert len(re.findall(r'\.name:\s+\S*k_checkpoint_totals\S*', txt)) == 1
    assert [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)] == [0] * 5
    assert [int(x) for x in re.findall(r'\.(?:sgpr|vgpr)_spill_count:\s+(\d+)', txt)] == [0] * 10
    assert sorted(int(x) for x in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', txt)) == [0] + [6 * 256 * 8] * 4
    assert 'global_load_dwordx4' in txt and 'global_store_dwordx4' in txt                 # 16-byte accesses


# ------------------------------------------------------------------ the Python layer
def test_trace_metrics_on_synthetic_arrays():
    from rescan_line_sted_amd import quality
    rng = np.random.default_rng(3)
    n = 500
    t = 10.0 + rng.random(n)
    trace = np.zeros((3, 2, 6))
    xs = {}
    for j in range(3):
        for k in range(2):
            x = (1.0 + 0.1 * j) * t + 0.01 * (k + 1) * rng.standard_normal(n)
            xs[j, k] = x
            trace[j, k] = [x.sum(), t.sum(), (x * x).sum(), (t * t).sum(), (x * t).sum(), ((x - t) ** 2).sum()]
    m = quality.trace_metrics(trace, n)
    assert set(m) == {'mse', 'nrmse', 'ncc', 'flux'} and all(v.shape == (3, 2) for v in m.values())
    for (j, k), x in xs.items():
        assert np.isclose(m['mse'][j, k], np.mean((x - t) ** 2), rtol=1e-12)
        assert np.isclose(m['nrmse'][j, k], np.sqrt(((x - t) ** 2).sum() / (t * t).sum()), rtol=1e-12)
        assert np.isclose(m['ncc'][j, k], np.corrcoef(x, t)[0, 1], rtol=1e-9)
        assert np.isclose(m['flux'][j, k], x.sum() / t.sum(), rtol=1e-12)
    # one pixel count per task broadcasts; an all-zero object has no nrmse, ncc or flux
    m2 = quality.trace_metrics(trace, np.array([n, n]))
    assert np.array_equal(m2['mse'], m['mse'])
    z = quality.trace_metrics(np.array([[4.0, 0, 8.0, 0, 0, 8.0]]), 2)
    assert z['mse'][0] == 4.0 and np.isnan(z['nrmse'][0]) and np.isnan(z['ncc'][0]) and np.isnan(z['flux'][0])
    with pytest.raises(ValueError):
        quality.trace_metrics(np.zeros((2, 5)), 4)


def test_best_iterations_on_synthetic_arrays():
    from rescan_line_sted_amd import sweep
    trace = np.zeros((4, 3, 6))
    trace[:, 0, 5] = [9, 4, 1, 3]          # an interior minimum
    trace[:, 1, 5] = [5, 4, 3, 2]          # still falling at the end
    trace[:, 2, 5] = [2, 2, 7, 7]          # a tie: the first
    best = sweep.best_iterations(trace, [1, 2, 5, 10])
    assert best.tolist() == [5, 10, 1]


def test_abi_and_signatures():
    from rescan_line_sted_amd import _lib, quality, sweep
    res, args = _lib.PROTOTYPES['rl_batch_submit_checkpoints']
    vpp = ctypes.POINTER(ctypes.c_void_p)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, vpp, ctypes.c_int, vpp]
    hdr = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    decl = re.search(r'int rl_batch_submit_checkpoints\(([^;]*)\);', hdr).group(1)
    assert len(decl.split(',')) == len(args) and '#define RL_TRACE_FIELDS 6' in hdr
    assert quality.TRACE_FIELDS == cr.FIELDS == 6
    sig = inspect.signature
    assert list(sig(_lib.DeconvPlan.batch_submit_checkpoints).parameters)[1:] == [
        'objects', 'total_brightness', 'seeds', 'image_ids', 'iterations_list', 'dev_outs', 'out_dtype', 'trace_devs', 'rng']
    p = sig(sweep.run_tasks_checkpoints_device).parameters
    assert list(p)[:4] == ['tasks', 'objects', 'psf_sets', 'iterations_list'] and p['estimates'].default is True and p['trace'].default is True
    assert list(sig(sweep.error_vs_iterations).parameters)[:4] == ['objects', 'psf_sets', 'seeds', 'iterations_list']
    assert list(sig(sweep.best_iterations).parameters) == ['trace', 'iterations_list']
    assert list(sig(quality.trace_metrics).parameters) == ['trace', 'n_pixels']
