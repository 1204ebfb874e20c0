"""The Poisson I-divergence and the stopping rules without a GPU: the kernel bodies of rescan_line_sted_amd/csrc/stop_kernels.hpp,
emulated on the host (tests/emu/stop_emu.cpp), against numpy, and the numpy reference (tests/stop_reference.py) against the study
that motivated the feature.  CPU only."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import stop_reference as sr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
RULES = {sr.DISCREPANCY: 1, sr.RELATIVE: 2}


class StopFrame(ctypes.Structure):      # StopFrame of stop_kernels.hpp
    _fields_ = [('d_latched', ctypes.c_double), ('d_last', ctypes.c_double), ('iterations', ctypes.c_int), ('stopped', ctypes.c_int)]


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libstop_emu.so')
    src = os.path.join(EMU_DIR, 'stop_emu.cpp')
    deps = [src] + [os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc', f) for f in ('stop_kernels.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas',
                               src, '-o', so])
    lib = ctypes.CDLL(so)
    vp, st, i, d = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    lib.emu_stop_blocks.argtypes = [st, st]
    lib.emu_stop_term.restype = d
    lib.emu_stop_term.argtypes = [d, d]
    lib.emu_stop_total.restype = d
    lib.emu_stop_total.argtypes = [vp, i]
    lib.emu_stop_rule_met.argtypes = [i, d, d, d, i, d]
    for sfx in ('f32', 'f64'):
        getattr(lib, 'emu_stop_divergence_' + sfx).argtypes = [vp, vp, vp, st, i]
        getattr(lib, 'emu_stop_latch_' + sfx).argtypes = [vp, vp, vp, vp, vp, st, st, i, i, d, i, i]
    assert lib.emu_stop_state_bytes() == ctypes.sizeof(StopFrame)
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _frame_data(rng, n, dtype):
    """A measurement with zeros and negatives, a prediction with zeros, negatives and nan."""
    m = rng.poisson(3.0, size=n).astype(np.float64) + 1e-9
    p = rng.gamma(3.0, 1.0, size=n) + 0.05
    k = max(1, n // 9)
    m[rng.integers(0, n, size=k)] = 0.0
    m[rng.integers(0, n, size=k)] = -rng.random(k)
    p[rng.integers(0, n, size=k)] = 0.0
    p[rng.integers(0, n, size=k)] = -rng.random(k)
    p[rng.integers(0, n, size=k)] = np.nan
    return m.astype(dtype), p.astype(dtype)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('views', [1, 4])
@pytest.mark.parametrize('n', [1, 7, 4096, 128 * 128, 300 * 301])
def test_emulated_divergence_matches_numpy(emu, dtype, views, n):
    """One block and many, aligned frames and (odd sizes) frames off 16-byte alignment, a partial last vector; the reference value
    is math.fsum of the float64 terms; bound stop_reference.summation_bound with L = stop_reference.chain_length(N): vectors per thread * W + log2(threads) + nb."""
    rng = np.random.default_rng(n * 10 + views)
    sfx = 'f64' if dtype == np.float64 else 'f32'
    N = views * n
    m0, p0 = _frame_data(rng, N, dtype)
    m1, p1 = _frame_data(rng, N, dtype)
    meas, pred = np.stack([m0, m1, m0]), np.stack([p0, p1, p0])      # frames 0 and 2 hold the same values
    nb = emu.emu_stop_blocks(N, np.dtype(dtype).itemsize)
    threads = emu.emu_stop_threads()
    assert threads == sr.THREADS and nb == sr.stop_blocks(N, np.dtype(dtype).itemsize)
    part = np.full((3, nb), np.nan)
    getattr(emu, 'emu_stop_divergence_' + sfx)(_p(meas), _p(pred), _p(part), N, 3)
    L = sr.chain_length(N, np.dtype(dtype).itemsize)
    for f in range(3):
        D = emu.emu_stop_total(_p(np.ascontiguousarray(part[f])), nb)
        want = sr.divergence(meas[f], pred[f])
        bound = sr.summation_bound(meas[f], pred[f], L)
        print('n %d views %d %s frame %d: D %.17g ref %.17g diff %.3g bound %.3g (L = %d)' % (n, views, sfx, f, D, want, abs(D - want), bound, L))
        assert abs(D - want) <= bound, (D, want, bound)
    assert np.array_equal(part[0], part[2])              # equal content, equal partials, whatever the frame's index (and alignment)


def test_pixel_term(emu):
    cases = [(3.0, 2.0), (0.0, 2.0), (-1.5, 2.0), (3.0, 0.0), (3.0, -1.0), (3.0, np.nan), (0.0, 0.0), (-2.0, 0.0), (-2.0, np.nan), (1e-9, 5.0)]
    for m, p in cases:
        got, want = emu.emu_stop_term(m, p), float(sr.pixel_terms(m, p))
        slack = 4 * np.spacing(abs(m * math.log(m / p)) + abs(m) + abs(p)) if m > 0 and p > 0 else 0.0      # (the two logs may differ in an ulp)
        assert abs(got - want) <= slack, (m, p, got, want)
    assert emu.emu_stop_term(3.0, 0.0) == 0.0 and emu.emu_stop_term(-2.0, np.nan) == 2.0 and emu.emu_stop_term(0.0, 2.0) == 2.0


def test_rule_table(emu):
    N = 1000.0
    table = [   # rule, t, D, D_prev (None: first check), met
        (sr.DISCREPANCY, 1.0, 500.0, None, True), (sr.DISCREPANCY, 1.0, 500.0000001, None, False), (sr.DISCREPANCY, 1.0, np.nan, None, False),
        (sr.DISCREPANCY, 1.0, np.inf, None, False), (sr.DISCREPANCY, np.inf, np.inf, None, False), (sr.DISCREPANCY, 1.0, -np.inf, 3.0, False),
        (sr.DISCREPANCY, 0.9, 460.0, 700.0, False), (sr.DISCREPANCY, 0.9, 440.0, 700.0, True),
        (sr.RELATIVE, 1e-3, 5.0, None, False), (sr.RELATIVE, 1e-3, 9.0, 10.0, False), (sr.RELATIVE, 1e-3, 9.995, 10.0, True),
        (sr.RELATIVE, 1e-3, 12.0, 10.0, True),                      # a D that rose
        (sr.RELATIVE, 1e-3, np.nan, 10.0, False), (sr.RELATIVE, 1e-3, 5.0, np.nan, False), (sr.RELATIVE, 1e-3, 5.0, np.inf, False),
        (sr.RELATIVE, 0.0, 10.0, 10.0, True), (sr.RELATIVE, 0.0, 9.999, 10.0, False),
    ]
    for rule, t, d, dp, met in table:
        got = emu.emu_stop_rule_met(RULES[rule], t, N, d, 0 if dp is None else 1, 0.0 if dp is None else dp)
        assert bool(got) == met, (rule, t, d, dp)
        assert sr.rule_met(rule, t, N, d, dp) == met, (rule, t, d, dp)
    assert emu.emu_stop_rule_met(3, 1.0, N, 0.0, 1, 1.0) == 0


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('rule', [sr.DISCREPANCY, sr.RELATIVE])
def test_emulated_latch_over_three_checks(emu, dtype, rule):
    """Four frames, three checks: the copy happens exactly for the frames that had not stopped before the check, the state is carried
    in the double buffer, and every workgroup of a frame reaches workgroup 0's decision."""
    sfx = 'f64' if dtype == np.float64 else 'f32'
    n = 70001                                            # several workgroups per frame; odd: frames 1 and 3 off alignment
    N = float(n)
    nbp = emu.emu_stop_blocks(n, np.dtype(dtype).itemsize)
    assert nbp > 1
    if rule == sr.DISCREPANCY:
        t = 1.0
        ds = [[0.6 * N, np.nan, 0.5 * N, 0.9 * N],       # check 1: frame 2 stops (2 D / N == 1)
              [0.4 * N, np.nan, 0.7 * N, 0.8 * N],       # check 2: frame 0 stops
              [0.3 * N, 0.45 * N, 0.2 * N, np.inf]]      # check 3: frame 1 stops; frame 3 never does
        want_iter, want_stop = [6, 9, 3, 9], [1, 1, 1, 0]
    else:
        t = 1e-3
        ds = [[10.0, np.nan, 1.0, 10.0],                 # check 1: no previous check, nothing stops
              [9.0, 5.0, 1.5, 9.9999],                   # check 2: frame 2 (D rose) and frame 3 stop; frame 1: D_prev is nan
              [8.9999, 4.0, 0.1, 1.0]]                   # check 3: frame 0 stops
        want_iter, want_stop = [9, 9, 6, 6], [1, 0, 1, 1]
    rng = np.random.default_rng(5)
    state = [(StopFrame * 4)(), (StopFrame * 4)()]
    for s in state:                                      # (stale memory: not read at the first check)
        for f in range(4):
            s[f].stopped, s[f].d_last, s[f].iterations = 1, -1.0, 77
    result = np.full((4, n), -1, dtype=dtype)
    kept = [None] * 4
    stopped_before = [False] * 4
    for c in range(3):
        est = rng.random((4, n)).astype(dtype)
        part = np.zeros((4, nbp))
        part[:, 0] = ds[c]
        part[:, 1] = 0.0
        before = result.copy()
        differ = getattr(emu, 'emu_stop_latch_' + sfx)(_p(est), _p(result), _p(part), ctypes.byref(state[c & 1]), ctypes.byref(state[(c + 1) & 1]),
                                                       n, n, 4, RULES[rule], t, 3 * (c + 1), 1 if c > 0 else 0)
        assert differ == 0
        now = state[(c + 1) & 1]
        for f in range(4):
            if stopped_before[f]:
                assert np.array_equal(result[f], before[f])              # untouched
            else:
                assert np.array_equal(result[f], est[f])
                kept[f] = (3 * (c + 1), ds[c][f])
            assert now[f].d_last == ds[c][f] or (np.isnan(ds[c][f]) and np.isnan(now[f].d_last))
            met = sr.rule_met(rule, t, N, ds[c][f], ds[c - 1][f] if c > 0 else None)
            stopped_before[f] = stopped_before[f] or met
            assert bool(now[f].stopped) == stopped_before[f], (c, f)
            assert now[f].iterations == kept[f][0]
            assert now[f].d_latched == kept[f][1] or np.isnan(kept[f][1])
    final = state[1]
    assert [final[f].iterations for f in range(4)] == want_iter
    assert [final[f].stopped for f in range(4)] == want_stop


@pytest.mark.parametrize('case', list(sr.TABLE), ids=lambda c: '%s-%s-%g' % (c[0], c[1].split('/')[1][:5], c[2]))
def test_reference_reproduces_the_study(case):
    """The stop iterations exactly; d within one unit of the last printed digit (the print is a rounding of d: half a unit -- for
    'lines, 2.0x line, 1e7' the recipe gives 1.5575 and 1.0795 where the study prints 1.558 and 1.080)."""
    printed, k_disc, k_rel = sr.TABLE[case]
    psfs, meas, trace = sr.case_trace(*case)
    N = len(psfs) * 128 * 128
    ks = [t[0] for t in trace]
    D = [t[1] for t in trace]
    assert ks == list(range(2, 61, 2))
    assert all(D[i] < D[i - 1] for i in range(1, len(D)))                  # plain RL is monotone in D
    for k, s in zip((2, 10, 20, 60), printed):
        d = 2.0 * D[ks.index(k)] / N
        unit = 10.0 ** -len(s.split('.')[1]) if float(s) < 10 or '.' in s else 1.0
        print(case, k, d, s)
        assert abs(d - float(s)) < unit, (case, k, d, s)
    i = sr.first_stop(D, sr.DISCREPANCY, 1.0, N)
    assert (None if i is None else ks[i]) == k_disc
    i = sr.first_stop(D, sr.RELATIVE, 1e-3, N)
    assert (None if i is None else ks[i]) == k_rel
