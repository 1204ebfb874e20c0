"""The sampler header in pieces and the frame-group Poisson kernel, without a GPU.

tests/emu/poisson_groups_emu.cpp compiles philox_poisson.hpp and the workgroup body of k_poisson_groups
(rescan_line_sted_amd/csrc/poisson_kernels.hpp) for the host.  It holds philox_poisson_fast / philox_ptrs_attempt /
philox_poisson word for word as they were before the header was split into ptrs_rate / ptrs_candidate / ptrs_accept; that copy
is the reference here, and every comparison is bit for bit.  The kernel body runs with one OS thread per GPU thread; its output
is also compared with the numpy twin (oracle/philox_poisson.py).  CPU only.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
_u, _ull, _vp, _i = ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_int
SEEDS = (5, (1 << 40) + 3)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libpoisson_groups_emu.so')
    src = os.path.join(EMU_DIR, 'poisson_groups_emu.cpp')
    deps = [src, os.path.join(EMU_DIR, 'emu_common.hpp')] + [os.path.join(CSRC, f) for f in ('philox_poisson.hpp', 'poisson_kernels.hpp', 'fft_core.hpp')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                               '-Wno-unknown-pragmas', '-pthread', src, '-o', so])
    lib = ctypes.CDLL(so)
    lib.pg_check_pieces.argtypes = [_vp, _i, _ull, _i, _vp, _vp]
    lib.pg_check_pieces.restype = None
    lib.pg_run.argtypes = [_i, _vp, _u, _vp, _vp, _u, _u, _u, _ull, _u, _vp, _vp, _vp, _i]
    lib.pg_run.restype = _i
    lib.pg_ref.argtypes = [_i, _vp, _vp, _u, _u, _u, _ull, _u, _vp, _vp, _vp]
    lib.pg_ref.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(_vp) if a is not None else None


# ---- the header's pieces

NAMED_RATES = [0.0, 1e-3, 9.99, 10.0, np.nextafter(10.0, 11.0), 12.25, 30.0, 1e3, 1e7, 1e12]


@pytest.mark.parametrize('seed', SEEDS)
def test_pieces_are_the_sampler_as_it_was(emu, seed):
    """The named rates and 1e5 random rates log-uniform in [10, 1e8], blocks 0 .. 63 of each: the re-expressed functions and
    the pieces with the rate-only values hoisted give the bits of the functions as they were."""
    rng = np.random.default_rng(2024)
    lams = np.concatenate([NAMED_RATES, np.exp(rng.uniform(np.log(10.0), np.log(1e8), 100000))])
    bad = np.zeros(4, dtype=np.int64)
    slow = np.zeros(1, dtype=np.int64)
    emu.pg_check_pieces(_p(lams), len(lams), seed, 64, _p(bad), _p(slow))
    assert bad.tolist() == [0, 0, 0, 0], dict(zip(('philox_poisson', 'philox_poisson_fast', 'philox_ptrs_attempt', 'pieces'), bad.tolist()))
    assert slow[0] > 0.02 * 64 * 100000      # the logarithm test was reached often enough to be tested


# ---- the kernel body

def rate_images(n_classes, V, n_pix, dtype, seed=7):
    """Rates on both sides of 10, exact zeros, the named rates, rates where most first attempts fail the squeeze."""
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(np.log(1e-3), np.log(3e3), (n_classes * V, n_pix)))
    lam[:, rng.random(n_pix) < 0.1] = 0.0
    lam[::2, rng.random(n_pix) < 0.2] = 10.5
    k = min(len(NAMED_RATES), n_pix)
    lam[0, :k] = NAMED_RATES[:k]
    return np.ascontiguousarray(lam.astype(dtype))


def pattern(kind, frames):
    """'runs': 3 + 5 + 8 and one more of the first class, which the kernel's sorting moves in front of the boundary between the
    groups, so that the run of 5 crosses it; 'crossing': the run of 8 crosses it in the launch's own order; 'interleaved': the
    order of a sweep's chunk, every frame a run of its own before sorting."""
    base = {'equal': 'A' * 17, 'alternating': 'AB' * 9, 'runs': 'AAA' + 'B' * 5 + 'C' * 8 + 'A', 'crossing': 'AAA' + 'B' * 8 + 'C' * 5 + 'A',
            'interleaved': 'ABC' * 16}[kind]
    assert frames <= len(base)
    return np.array([ord(c) - ord('A') for c in base[:frames]], dtype=np.uint32)


def run_case(emu, dtype, n_pix, frames, V, kind, grid, per_frame_keys=False, seed=SEEDS[1], image0=3):
    rate_frame = pattern(kind, frames)
    lam = rate_images(3, V, n_pix, dtype)
    seeds = ids = None
    if per_frame_keys:
        seeds = np.array([1000 + 7 * f + ((f % 3) << 33) for f in range(frames)], dtype=np.uint64)
        ids = np.array([50 - f for f in range(frames)], dtype=np.uint32)
    got = np.full((frames, V, n_pix), np.nan, dtype=dtype)
    want = np.full_like(got, np.nan)
    writes = np.zeros(got.shape, dtype=np.int32)
    f64 = int(np.dtype(dtype) == np.float64)
    items = emu.pg_run(f64, _p(lam), len(lam), _p(got), _p(writes), n_pix, frames, V, seed, image0, _p(seeds), _p(ids), _p(rate_frame), grid)
    assert items == -(-frames // 8) * V * -(-n_pix // 256)
    emu.pg_ref(f64, _p(lam), _p(want), n_pix, frames, V, seed, image0, _p(seeds), _p(ids), _p(rate_frame))
    assert (writes == 1).all(), 'written %d .. %d times' % (writes.min(), writes.max())
    assert not np.isnan(got).any()
    assert np.array_equal(got, want)
    return got, lam, rate_frame, seeds, ids


@pytest.mark.parametrize('kind', ['equal', 'alternating', 'runs', 'interleaved'])
@pytest.mark.parametrize('V', [1, 2])
@pytest.mark.parametrize('frames', [1, 7, 8, 9, 17])
@pytest.mark.parametrize('n_pix', [256, 300, 1536])
def test_body_draws_what_the_sampler_draws(emu, n_pix, frames, V, kind):
    """Every (frame, view, pixel) written exactly once with philox_poisson()'s value, whatever the grid's width; f32 at the
    ragged size and f64 at the others, so that both element types meet every frame count and pattern."""
    dtype = np.float32 if n_pix == 300 else np.float64
    first = None
    for grid in (1, 3, 0):      # 0: one workgroup per item
        got = run_case(emu, dtype, n_pix, frames, V, kind, grid)[0]
        assert first is None or np.array_equal(got, first)
        first = got


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('per_frame_keys', [False, True])
def test_body_against_the_numpy_twin(emu, dtype, per_frame_keys):
    from oracle import philox_poisson as pp
    n_pix, frames, V = 300, 17, 2
    got, lam, rate_frame, seeds, ids = run_case(emu, dtype, n_pix, frames, V, 'runs', 3, per_frame_keys=per_frame_keys)
    for f in range(frames):
        for v in range(V):
            seed, image = (int(seeds[f]), int(ids[f]) * V + v) if per_frame_keys else (SEEDS[1], 3 + f * V + v)
            want = (pp.poisson(lam[rate_frame[f] * V + v].astype(np.float64), seed, image) + 1e-9).astype(dtype)
            assert np.array_equal(got[f, v], want), (f, v)


def test_per_frame_keys_at_every_shape_class(emu):
    for n_pix, frames, V, kind in ((256, 9, 1, 'alternating'), (1536, 17, 2, 'equal'), (300, 8, 2, 'runs'), (300, 17, 1, 'crossing')):
        run_case(emu, np.float32, n_pix, frames, V, kind, 0, per_frame_keys=True)


def test_frames_are_grouped_by_rate_image(emu):
    """A sweep's chunk: 48 frames of three objects in turn, a key per frame.  Sorted by rate image they are six groups of one run
    each; the values and the single write per pixel do not depend on it."""
    run_case(emu, np.float32, 300, 48, 2, 'interleaved', 5, per_frame_keys=True)


def test_more_frames_than_threads_keep_their_order(emu):
    """A launch of more than 256 frames is not sorted (a workgroup sorts with one thread per frame): 257 frames of two rate images
    in turn, the last group a single frame."""
    frames, n_pix = 257, 256
    rate_frame = (np.arange(frames) % 2).astype(np.uint32)
    lam = rate_images(2, 1, n_pix, np.float32)
    got = np.full((frames, 1, n_pix), np.nan, dtype=np.float32)
    want = np.full_like(got, np.nan)
    writes = np.zeros(got.shape, dtype=np.int32)
    assert emu.pg_run(0, _p(lam), len(lam), _p(got), _p(writes), n_pix, frames, 1, SEEDS[0], 0, None, None, _p(rate_frame), 4) == 33
    emu.pg_ref(0, _p(lam), _p(want), n_pix, frames, 1, SEEDS[0], 0, None, None, _p(rate_frame))
    assert (writes == 1).all() and np.array_equal(got, want)


def test_scratch_of_the_draw_kernels(tmp_path):
    """aux_kernels.hip compiled device-only with the flags of _build.py: k_poisson keeps nothing in scratch; k_poisson_groups,
    held to five waves per SIMD (96 registers), keeps the 12 bytes per lane that its comment and DESIGN.md section 4 state."""
    import re
    import shutil
    from rescan_line_sted_amd import _build
    if not (shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC)):
        pytest.skip('no hipcc')
    out = str(tmp_path / 'aux.s')
    subprocess.check_call([_build.HIPCC] + _build.COMMON + _build.DEVICE + ['--cuda-device-only', '-S', os.path.join(CSRC, 'aux_kernels.hip'), '-o', out],
                          stderr=subprocess.DEVNULL)
    txt = open(out).read()
    priv = dict(zip(re.findall(r'\.name:\s+(\S+)', txt), (int(x) for x in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', txt))))
    groups = {k: v for k, v in priv.items() if 'k_poisson_groups' in k}
    plain = {k: v for k, v in priv.items() if 'k_poisson' in k and k not in groups}
    assert len(groups) == 2 and len(plain) == 4
    assert all(v == 0 for v in plain.values()), plain
    assert all(v <= 12 for v in groups.values()), groups


def test_lds_fits_beside_the_per_frame_kernel(emu):
    """Two lists of 2048 entries, the table and the counters: no more than k_poisson's 2 x 2048 x (4 + 4) + 12 bytes (f32)."""
    assert emu.pg_lds_bytes() <= 2 * 2048 * 8 + 12
