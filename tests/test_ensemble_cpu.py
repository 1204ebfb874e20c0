"""The ensemble statistics without a GPU (include/rlsted.h rl_ensemble_stats): the bodies of k_ensemble_stats and k_ensemble_totals
(rescan_line_sted_amd/csrc/ensemble_kernels.hpp) emulated on the host thread by thread (tests/emu/ensemble_emu.cpp) against numpy
long double under the derived bound (tests/ensemble_reference.py); the same code as a stand-alone program under the address and
undefined-behaviour sanitizers; the compiled kernels' resources; and the arithmetic of the Python wrappers on synthetic arrays.
CPU only."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ensemble_reference as er
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'ensemble_emu.cpp')
DT = {'f32': 0, 'f64': 1}
SIZES = (1, 2, 3, 16, 17)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libensemble_emu.so')
    deps = [SRC] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f) for f in ('ensemble_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_ensemble_blocks.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lib.emu_ensemble_stats.argtypes = [vp, i, vp, vp, i, vp, i, vp, vp, ctypes.c_size_t, vp, vp, vp]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _run(emu, case, groups=None, truth=True, maps=True):
    """The emulated call on the groups `groups` (indices into the case's; None: all).  Returns (mean, var, out), maps None if not asked for."""
    gs = range(len(case.sizes)) if groups is None else groups
    offs = [case.offsets[g] for g in gs]
    gp = np.concatenate([[0], np.cumsum([len(o) for o in offs])]).astype(np.int32)
    off = np.concatenate(offs).astype(np.int64)
    G = len(offs)
    mean = np.full((G, case.N), np.nan) if maps else None
    var = np.full((G, case.N), np.nan) if maps else None
    out = np.full((G, er.FIELDS), np.nan)
    t_off = np.array([case.truth_off[g] for g in gs], dtype=np.int64)
    scale = np.array([case.scale[g] for g in gs], dtype=np.float64)
    nb = emu.emu_ensemble_stats(_p(case.buf), DT[case.dtype], _p(off), _p(gp), G, _p(case.truth_buf) if truth else None, DT[case.truth_dtype],
                                _p(t_off), _p(scale), case.N, _p(mean), _p(var), _p(out))
    assert nb == emu.emu_ensemble_blocks(case.N, 4 if case.dtype == 'f32' else 8)
    return mean, var, out


def test_the_work_split_is_the_accel_split(emu):
    """8192 f32 pixels (4096 f64 pixels) are one workgroup's run; one more vector opens a second workgroup."""
    assert emu.emu_ensemble_threads() == 256 and emu.emu_ensemble_sums() == 5
    assert [emu.emu_ensemble_blocks(n, 4) for n in (1, 8192, 8193, 8197, 2 * 8192 + 1)] == [1, 1, 2, 2, 3]
    assert [emu.emu_ensemble_blocks(n, 8) for n in (1, 4096, 4097, 8192, 8193)] == [1, 1, 2, 2, 3]


@pytest.mark.parametrize('N', [1, 3, 5, 1023, 8192, 8193, 8197])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_emulated_kernels_match_long_double(emu, dtype, N):
    """One call with groups of 1, 2, 3, 16 and 17 members at odd and even element offsets (both load paths), the first member of
    group 1 listed in group 0 as well; every group against the reference; then a group alone, the call without a truth and the call
    without maps."""
    rng = np.random.default_rng(1000 * N + DT[dtype])
    case = er.Case(rng, dtype, N, SIZES, shift=1, truth_dtype='f32' if N == 1023 else 'f64')
    assert any(o % 2 == 1 for offs in case.offsets for o in offs) and any(o % 4 == 0 for offs in case.offsets for o in offs)
    assert case.offsets[1][0] == case.offsets[0][0]
    mean, var, out = _run(emu, case)
    assert not np.isnan(mean).any() and not np.isnan(var).any() and not np.isnan(out).any()   # every pixel of every map was written
    for g, n in enumerate(SIZES):
        case.reference(g).check(out[g], mean[g], var[g], '%s N=%d n=%d' % (dtype, N, n))
    assert np.all(var[0] == 0.0) and out[0, 2] == 0.0                                # n = 1: exactly 0
    # a group alone gives the bits it gives among the others
    for g in (3, 1):
        m1, v1, o1 = _run(emu, case, [g])
        assert np.array_equal(o1[0], out[g]) and np.array_equal(m1[0], mean[g]) and np.array_equal(v1[0], var[g]), g
    rev = _run(emu, case, [4, 3, 2, 1, 0])[2]
    assert np.array_equal(rev[::-1], out)
    # no truth: fields 3..5 are 0, the rest unchanged
    m2, v2, o2 = _run(emu, case, truth=False)
    assert np.array_equal(o2[:, :3], out[:, :3]) and np.all(o2[:, 3:] == 0.0)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)
    case.reference(4, truth=False).check(o2[4], m2[4], v2[4], '%s N=%d n=17 no truth' % (dtype, N))
    # no maps: the same sums
    assert np.array_equal(_run(emu, case, maps=False)[2], out)


def test_cancellation_needs_the_second_pass(emu):
    """f64 values 1e8 + N(0, 1), n = 16: the two-pass sum of squares stays within 1e-9 of its value -- the derived bound itself is
    that tight -- where sum x^2 - n mean^2 is off by whole units."""
    rng = np.random.default_rng(16)
    case = er.Case(rng, 'f64', 1023, (16,), shift=1, cancel=True)
    mean, var, out = _run(emu, case)
    ref = case.reference(0)
    ss = ref.ss.astype(np.float64)
    assert np.all(ref.e_ss < 1e-9 * ss) and np.all(ref.e_var < 1e-9 * ref.var.astype(np.float64))   # the derivation is not too loose
    sums, bnd = ref.sums()
    assert bnd[2] < 1e-9 * float(sums[2])
    ref.check(out[0], mean[0], var[0], 'cancellation f64 N=1023 n=16')
    x = case.members(0)
    one_pass = (x * x).sum(axis=0) - 16 * x.mean(axis=0) ** 2
    worst = float(np.max(np.abs(one_pass - ss) / ss))
    two_pass = float(np.max(np.abs(var[0] * 15 - ss) / ss))
    print('relative error of ss: two passes (emulated kernel) %.3g, one pass %.3g' % (two_pass, worst))
    assert worst > 1e-3 and two_pass < 1e-12


def test_emulation_under_sanitizers(tmp_path):
    """ensemble_emu.cpp as a stand-alone program (its own main: exactly-sized buffers, groups of 1 to 17 at odd and even offsets,
    all four type pairs, with and without truth and maps) built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / 'ensemble_emu_main')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-ffp-contract=off',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DENSEMBLE_EMU_MAIN', SRC, '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith('ok 144 720')


def test_kernels_do_not_spill_and_hold_only_the_tree(tmp_path):
    """ensemble_kernels.hip compiled device-only with the flags of _build.py: the four instances of k_ensemble_stats and
    k_ensemble_totals, no scratch, LDS = the tree's 5 x 256 doubles (none in the totals kernel)."""
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'ensemble_kernels.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE +
                          ['--cuda-device-only', '-S', os.path.join(_build.CSRC, 'ensemble_kernels.hip'), '-o', out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    assert len(re.findall(r'\.name:\s+\S*k_ensemble_stats\S*', txt)) == 4
    assert len(re.findall(r'\.name:\s+\S*k_ensemble_totals\S*', txt)) == 1
    assert [int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt)] == [0] * 5
    assert sorted(int(x) for x in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', txt)) == [0] + [5 * 256 * 8] * 4


# ------------------------------------------------------------------ the Python layer
def test_readers_on_synthetic_arrays():
    from rescan_line_sted_amd import quality
    spec = np.zeros((2, 3))
    spec[0] = [4, 16.0, 64.0]                                                         # 4 bins, bias power 16, variance power 64
    b, v = quality.spectral_bias_variance_rms(spec, (2, 5))
    assert b.shape == (2,) and b[0] == 0.2 and v[0] == 0.4 and np.isnan(b[1]) and np.isnan(v[1])
    # the units of radial_error_from_stats: a ring of field 4 = 16 over 4 bins reads the same
    st = np.zeros((2, 5))
    st[0] = [4, 100.0, 0, 0, 16.0]
    assert quality.radial_error_from_stats(st, (2, 5))[0] == b[0]
    s = quality.ssnr_from(st, spec, 16)
    assert s.shape == (2,) and s[0] == 100.0 / (64.0 / 16) and np.isnan(s[1])
    zero_noise = spec.copy()
    zero_noise[0, 2] = 0.0
    assert np.isnan(quality.ssnr_from(st, zero_noise, 16)[0])
    cells = np.zeros((3, 2, 4, 3))                                                    # [key][R][S][3] works per cell
    cells[..., 0] = 2
    cells[..., 1] = 8.0
    bb, vv = quality.spectral_bias_variance_rms(cells, (4, 4))
    assert bb.shape == (3, 2, 4) and np.all(bb == 2.0 / 16) and np.all(vv == 0.0)


def test_ensemble_keys_and_layout_helpers():
    from rescan_line_sted_amd import sweep
    tasks = [('b', 'p', 0), ('a', 'p', 0), ('b', 'p', 1), ('a', 'q', 0), ('a', 'p', 1), ('b', 'p', 2)]
    keys, members = sweep.ensemble_keys(tasks)
    assert keys == [('b', 'p'), ('a', 'p'), ('a', 'q')] and members == [[0, 2, 5], [1, 4], [3]]
    assert sweep.ensemble_keys([]) == ([], [])


def test_abi_and_signatures():
    from rescan_line_sted_amd import _lib, quality, sweep
    res, args = _lib.PROTOTYPES['rl_ensemble_stats']
    assert res is ctypes.c_int and len(args) == 14
    assert args[3] == ctypes.POINTER(ctypes.c_int64) and args[4] == ctypes.POINTER(ctypes.c_int32) and args[10] is ctypes.c_size_t
    hdr = open(os.path.join(ROOT, 'include', 'rlsted.h')).read()
    assert 'int rl_ensemble_stats(' in hdr and '#define RL_ENSEMBLE_FIELDS 6' in hdr
    assert quality.ENSEMBLE_FIELDS == er.FIELDS == 6
    sig = inspect.signature
    assert sig(sweep.figure_2_sweep).parameters['ensemble'].default is False
    assert list(sig(sweep.figure_2_sweep).parameters)[-1] == 'ensemble'               # appended: positional callers are unaffected
    p = sig(sweep.DeviceResults.ensemble).parameters
    assert [p[k].default for k in ('truth', 'truth_index', 'scale', 'maps')] == [None, None, None, True]
    p = sig(sweep.ensemble_tasks).parameters
    assert p['total_brightness'].default == 5e10 and p['maps'].default is True
    p = sig(sweep.bias_variance_spectrum).parameters
    assert p['total_brightness'].default == 5e10 and p['n_rings'].default is None and p['n_sectors'].default is None
    assert list(sig(sweep.bias_variance_vs_iterations).parameters)[:4] == ['objects', 'psf_sets', 'seeds', 'iterations_list']
    assert 'sum(iterations_list)' in sweep.bias_variance_vs_iterations.__doc__
    p = sig(quality.ensemble_stats).parameters
    assert p['truth'].default is None and p['scale'].default is None
    assert list(sig(quality.ensemble_stats_device).parameters)[:6] == ['ctx', 'dev', 'dtype', 'groups_offsets', 'n_pixels', 'truth']
