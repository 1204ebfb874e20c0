"""Frames that carry the same object are simulated once per slice (csrc/object_classes.hpp, rlsted.cpp run_slices;
include/rlsted.h rl_deconv_object_classes).  Needs an MI355X.

Every check compares a plan created with RLSTED_SHARE_OBJECTS=0 -- H(object) of every frame, as it always was -- with a plan
created with the default in the same process: np.array_equal, no tolerance.  The shared simulation runs the same kernels on the
same values (a member's scaled object is its representative's bit for bit, and the sampler keeps each frame's own Philox
counters), so there is nothing to round differently.

Shapes.  A small PSF that is not rank 1 (9 x 9, 81 taps: neither stencil strategy takes it) keeps the plans on the FFT path.
With it 128 x 128 frames transform at L = 192, whose transforms share a wavefront four at a time: no frame pairs, the general
row body.  The wave-private kernels of L = 256 with the frame-pair loop on single-view f32 plans need more than 192 samples:
200 x 200 frames.  Both sizes run every case.  512 x 512 with the 107 x 107 STED PSF: the kernels compiled for 512-pixel rows;
1153 x 40 with two views: the smallest image whose column transform (L = 2304) takes the split pass.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_cases import plans_per_value

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def small_psfs(V, seed=3):
    """9 x 9, positive, not rank 1, 81 taps: neither the separable nor the direct stencil takes it."""
    rng = np.random.default_rng(seed)
    return [rng.random((1, 9, 9)) + 0.05 for _ in range(V)]


def objects(pattern, ny, nx, seed=11):
    rng = np.random.default_rng(seed)
    kinds = {c: rng.random((ny, nx)) * 200 + 1 for c in sorted(set(pattern))}
    return np.stack([kinds[c] for c in pattern])


# (per-frame plan, sharing plan) = plans(lib, psfs, B, ny, nx, dtype, options=None)
plans = functools.partial(plans_per_value, switch='RLSTED_SHARE_OBJECTS', fft_only=True)


def same_cycle(off, on, objs, brightness, K, cycles=2, seed=5, shared=True):
    """bench.py's call on both plans: measurement, estimate and (read back last) noiseless agree bit for bit."""
    for p in (off, on):
        p.set_object(objs, brightness)
        p.bench_cycles(K, cycles, seed=seed)
    info = on.object_classes()
    assert off.object_classes()['shared_slices'] == 0
    assert (info['shared_slices'] > 0) == shared, info
    assert np.array_equal(off.measurement(), on.measurement())
    assert np.array_equal(off.estimate(), on.estimate())
    assert np.array_equal(off.noiseless(), on.noiseless())          # every frame's, expanded from the representatives'
    return info


@pytest.mark.parametrize('pattern', ['AABABC', 'AABABCA'])           # B = 7: an odd batch's phantom pair
@pytest.mark.parametrize('V', [1, 2])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('size', [128, 200])
def test_shared_cycle_is_the_per_frame_cycle(lib, size, dtype, V, pattern):
    B = len(pattern)
    off, on = plans(lib, small_psfs(V), B, size, size, dtype)
    assert on.info()['lx'] == on.info()['ly'] == {128: 192, 200: 256}[size]
    assert on.strategy()['frame_pairs'] == (size == 200 and dtype == 'f32' and V == 1)
    info = same_cycle(off, on, objects(pattern, size, size), 3e7 * (size / 128) ** 2, K=3)
    assert info == {'classes': 3, 'shared_slices': 1, 'slices': 1}


@pytest.mark.parametrize('size,dtype,V,mb', [(200, 'f32', 1, '0.001'), (128, 'f64', 2, '2.2')])
def test_a_class_spans_slices_and_lanes(lib, size, dtype, V, mb):
    """Slices of two frames on two streams (a pair plan's smallest slice; 2.2 MB hold two float64 frames of two views): class A has
    a representative in three slices, on both lanes, and the cycles follow each other without the lanes meeting."""
    off, on = plans(lib, small_psfs(V), 8, size, size, dtype, options={'RLSTED_CHUNK_MB': mb, 'RLSTED_LANES': '2'})
    info = same_cycle(off, on, objects('AAAAAABB', size, size), 3e7, K=3, cycles=3)
    assert info == {'classes': 2, 'shared_slices': 4, 'slices': 4}


def test_slices_with_many_classes_keep_the_per_frame_path(lib):
    """A B C D | A A A A in slices of four: the first simulates its four frames, the second one representative."""
    off, on = plans(lib, small_psfs(1), 8, 128, 128, 'f64', options={'RLSTED_CHUNK_MB': '2.0', 'RLSTED_LANES': '2'})
    info = same_cycle(off, on, objects('ABCDAAAA', 128, 128), 3e7, K=2)
    assert info == {'classes': 4, 'shared_slices': 1, 'slices': 2}
    # all frames distinct: nothing to share
    same_cycle(off, on, objects('ABCDEFGH', 128, 128), 3e7, K=1, shared=False)
    # equal pixels, another brightness: another object on the device
    for p in (off, on):
        p.set_object(objects('AAAAAAAA', 128, 128), [3e7, 3e7, 3e7, 4e7, 3e7, 3e7, 3e7, 3e7])
    assert on.object_classes()['classes'] == 2


def test_512_specialised_kernels(lib, golden):
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    off, on = plans(lib, psf, 4, 512, 512, 'f32')
    assert on.info()['lx'] == 576 and on.strategy()['frame_pairs']
    same_cycle(off, on, objects('AAAB', 512, 512), 8e11, K=2, cycles=1)


def test_split_column_pass(lib):
    off, on = plans(lib, small_psfs(2), 4, 1153, 40, 'f32')
    assert on.info()['ly'] == 2304 and on.strategy()['split_column_pass']
    same_cycle(off, on, objects('ABAA', 1153, 40), 1e8, K=3)


@pytest.mark.parametrize('size,dtype,V', [(200, 'f32', 1), (128, 'f64', 2)])
def test_batch_run_with_tasks_that_share_objects(lib, size, dtype, V):
    """rl_batch_run: tasks that point at the same object, each with its own seed and image id; ten tasks on a plan of six frames
    (the short second chunk repeats its last task)."""
    B, n_tasks, K = 6, 10, 3
    off, on = plans(lib, small_psfs(V), B, size, size, dtype)
    kinds = objects('ABC', size, size)
    which = [0, 0, 1, 0, 1, 2, 0, 0, 0, 1]
    tasks = (lib.DeconvPlan._Task * n_tasks)()
    for i, w in enumerate(which):
        tasks[i].object = kinds[w].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        tasks[i].total_brightness = 3e7
        tasks[i].seed = 1000 + 7 * i
        tasks[i].image_id = 50 - i
    got = []
    for p in (off, on):
        out = np.empty((n_tasks, size, size))
        lib.check(lib.lib.rl_batch_run(p.handle, ctypes.cast(tasks, ctypes.c_void_p), n_tasks, K, lib.RNG_PHILOX, lib.ptr(out)))
        got.append((out, p.measurement(), p.noiseless()))
    assert on.object_classes() == {'classes': 2, 'shared_slices': 1, 'slices': 1}          # the last chunk: A A A B B B
    assert off.object_classes()['shared_slices'] == 0
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    # a frame's draws are its key's, whatever it shares: tasks 0 and 1 carry the same object and differ
    assert not np.array_equal(got[1][0][0], got[1][0][1])


def test_iterate_continues_after_shared_cycles(lib):
    """K = 4 on the pair loop drops the last spectrum; the first iteration never read or filled the estimate: rl_deconv_iterate
    afterwards rebuilds the spectrum from an estimate that is all there, and K = 0 / K = 1 leave ones / one update."""
    off, on = plans(lib, small_psfs(1), 6, 200, 200, 'f32')
    assert on.strategy()['frame_pairs']
    objs = objects('AABABC', 200, 200)
    for p in (off, on):
        p.set_object(objs, 7e7)
    on.bench_cycles(4, 2, seed=8)
    on.iterate(2)
    off.simulate(seed=9)                     # the second cycle's seed
    off.iterate(4)
    off.iterate(2)
    assert np.array_equal(off.measurement(), on.measurement())
    assert np.array_equal(off.estimate(), on.estimate())
    on.bench_cycles(0, 1, seed=8)
    assert np.array_equal(on.estimate(), np.ones((6, 200, 200)))
    on.bench_cycles(1, 1, seed=8)
    off.simulate(seed=8)
    off.reset_estimate()
    off.iterate(1)
    assert np.array_equal(off.estimate(), on.estimate())
    # simulate after a shared cycle draws from every frame's rates (the noiseless buffer is filled first)
    on.bench_cycles(1, 1, seed=3)
    on.simulate(seed=21)
    off.simulate(seed=21)
    assert np.array_equal(off.measurement(), on.measurement())


def test_handing_out_the_object_buffer_ends_the_sharing(lib):
    off, on = plans(lib, small_psfs(1), 4, 128, 128, 'f64')
    same_cycle(off, on, objects('AAAA', 128, 128), 3e7, K=1)
    on.device_array('object')               # the caller may write it: the classes are no longer known
    on.bench_cycles(1, 1, seed=5)
    assert on.object_classes() == {'classes': 0, 'shared_slices': 0, 'slices': 1}
    off.bench_cycles(1, 1, seed=5)
    assert np.array_equal(off.estimate(), on.estimate()) and np.array_equal(off.noiseless(), on.noiseless())
