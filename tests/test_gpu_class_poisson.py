"""One simulation per object class and CYCLE (rlsted.cpp run_slices / forward_classes, csrc/object_classes.hpp class_layout;
include/rlsted.h rl_deconv_simulated_images).  Needs an MI355X.

A cycle computes H(object) once for every class that its sharing slices hold, in spectrum space of its own, and every sharing
slice on either lane draws from those rates.  The checks compare a plan created with RLSTED_SHARE_OBJECTS=0 -- H(object) of every
frame -- with a plan created with the default in the same process, np.array_equal, no tolerance: the class simulation runs the
launches a slice's simulation runs, on the same bits, and the sampler keeps each frame's own Philox counters.  The measurement is
also compared with the numpy twin of the sampler (oracle/philox_poisson.py) on the rates the plan reports.

(The file carries the name of the class-wise Poisson sampler these cases were also written for; that kernel was measured slower
than k_poisson and is not in the library -- DESIGN.md "One simulation per object class and cycle" -- so the sampler under test
is k_poisson reading each frame's rates through rate_of.)

Shapes as in test_gpu_shared_objects.py: a 9 x 9 PSF that is not rank 1 keeps the plans on the FFT path; 128 x 128 transforms at
L = 192 (general row body), 200 x 200 at L = 256 (wave-private kernels, frame pairs on single-view f32 plans); 512 x 512 with the
107 x 107 STED PSF runs the kernels compiled for 512-pixel rows.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_cases import plans_per_value

pytestmark = pytest.mark.gpu

SEEDS = (5, 77, (1 << 40) + 3)


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def small_psfs(V, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.random((1, 9, 9)) + 0.05 for _ in range(V)]


def objects(pattern, ny, nx, seed=11):
    rng = np.random.default_rng(seed)
    kinds = {c: rng.random((ny, nx)) * 200 + 1 for c in sorted(set(pattern))}
    return np.stack([kinds[c] for c in pattern])


# (per-frame plan, sharing plan) = plans(lib, psfs, B, ny, nx, dtype, options=None)
plans = functools.partial(plans_per_value, switch='RLSTED_SHARE_OBJECTS', fft_only=True)


def twin(plan, dtype, seed):
    """The numpy twin's draws from the rates the plan reports (image = frame * V + view, one seed for the batch)."""
    from oracle import philox_poisson as pp
    lam = plan.noiseless()
    want = pp.noisy_measurement(lam.reshape((-1,) + lam.shape[2:]), seed).reshape(lam.shape)
    return want.astype(np.float32).astype(np.float64) if dtype == 'f32' else want


def same_cycles(off, on, K, seeds=SEEDS, cycles=1):
    """Cycles with different seeds on both plans: measurement and estimate after each, the noiseless images at the end."""
    for seed in seeds:
        for p in (off, on):
            p.bench_cycles(K, cycles, seed=seed)
        assert np.array_equal(off.measurement(), on.measurement()), seed
        assert np.array_equal(off.estimate(), on.estimate()), seed
    assert np.array_equal(off.noiseless(), on.noiseless())


@pytest.mark.parametrize('V', [1, 2])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('size', [128, 200])
def test_class_cycle_is_the_per_frame_cycle(lib, size, dtype, V):
    pattern = 'AABABCA'
    off, on = plans(lib, small_psfs(V), len(pattern), size, size, dtype)
    assert on.info()['lx'] == on.info()['ly'] == {128: 192, 200: 256}[size]
    assert on.strategy()['frame_pairs'] == (size == 200 and dtype == 'f32' and V == 1)
    for p in (off, on):
        p.set_object(objects(pattern, size, size), 3e7 * (size / 128) ** 2)
    same_cycles(off, on, K=3)
    assert on.object_classes() == {'classes': 3, 'shared_slices': 1, 'slices': 1}
    assert on.simulated_images() == 3 * V and off.simulated_images() == 7 * V
    assert np.array_equal(on.measurement(), twin(on, dtype, SEEDS[-1]))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_zero_pixels_and_rates_on_both_sides_of_ten(lib, dtype):
    """One object with a dark block and a ramp whose rates cross 10 inside one image: PTRS, the multiplication method and the
    exact zero all meet in a tile."""
    size, V = 128, 2
    rng = np.random.default_rng(19)
    a = rng.random((size, size)) * np.linspace(0.02, 4.0, size)[None, :]
    a[40:90, 10:70] = 0.0
    b = rng.random((size, size)) * 200 + 1
    objs = np.stack([a, a, b, a, a, b, a])
    off, on = plans(lib, small_psfs(V), 7, size, size, dtype)
    for p in (off, on):
        p.set_object(objs, 7000.0)
    same_cycles(off, on, K=2)
    lam = on.noiseless()[0, 0]
    assert (objs[0] == 0).sum() == 50 * 60
    assert (lam >= 10.0).sum() > 1000 and ((lam > 0) & (lam < 10.0)).sum() > 1000 and (lam[50:80, 20:60] < 1e-3).all()
    assert on.simulated_images() == 2 * V
    assert np.array_equal(on.measurement(), twin(on, dtype, SEEDS[-1]))


@pytest.mark.parametrize('size,dtype,V,mb', [(200, 'f32', 1, '0.001'), (128, 'f64', 2, '2.2')])
def test_a_class_is_simulated_once_for_all_slices_and_lanes(lib, size, dtype, V, mb):
    """Slices of two frames on two streams: class A is drawn from in three slices, on both lanes, class B in one; H is computed
    for 2 V images per cycle, not for the 4 V of one representative per slice.  Three cycles follow each other without the
    lanes meeting.  What this can catch of the event order is the first cycle's wait for the class rates on lane 1; the order
    between a cycle's last draws and the NEXT cycle's class simulation holds by construction (run_slices), not by this test: within
    one call the object stays, so an overtaking simulation would write the bytes that are there, and the API joins the lanes
    before the object can change (rl_deconv_set_object, rl_batch_submit)."""
    off, on = plans(lib, small_psfs(V), 8, size, size, dtype, options={'RLSTED_CHUNK_MB': mb, 'RLSTED_LANES': '2'})
    for p in (off, on):
        p.set_object(objects('AAAAAABB', size, size), 3e7)
    same_cycles(off, on, K=3, seeds=(5, 900), cycles=3)
    assert on.object_classes() == {'classes': 2, 'shared_slices': 4, 'slices': 4}
    assert on.simulated_images() == 2 * V
    assert off.simulated_images() == 8 * V
    assert np.array_equal(on.measurement(), twin(on, dtype, 900 + 2))      # (cycle r of a call draws with seed + r)


def test_sharing_and_per_frame_slices_in_one_cycle(lib):
    """A B C D | A A A A | E E F F in slices of four on two lanes: the first slice simulates its four frames, the others draw from
    three classes simulated once."""
    off, on = plans(lib, small_psfs(1), 12, 128, 128, 'f64', options={'RLSTED_CHUNK_MB': '2.0', 'RLSTED_LANES': '2'})
    for p in (off, on):
        p.set_object(objects('ABCDAAAAEEFF', 128, 128), 3e7)
    same_cycles(off, on, K=2, seeds=(5, 6), cycles=2)
    assert on.object_classes() == {'classes': 6, 'shared_slices': 2, 'slices': 3}
    assert on.simulated_images() == 4 + 3


def test_a_second_object_between_cycles(lib):
    off, on = plans(lib, small_psfs(1), 6, 200, 200, 'f32')
    for seed, pattern in ((1, 'AABABC'), (2, 'CCCCAA')):
        for p in (off, on):
            p.set_object(objects(pattern, 200, 200, seed=40 + seed), 7e7)
        same_cycles(off, on, K=2, seeds=(seed,))
    assert on.simulated_images() == 2
    assert np.array_equal(on.measurement(), twin(on, 'f32', 2))


def test_handing_out_the_object_buffer_returns_to_the_per_frame_path(lib):
    off, on = plans(lib, small_psfs(1), 4, 128, 128, 'f64')
    for p in (off, on):
        p.set_object(objects('AAAA', 128, 128), 3e7)
    same_cycles(off, on, K=1, seeds=(5,))
    assert on.simulated_images() == 1
    on.device_array('object')
    same_cycles(off, on, K=1, seeds=(6,))
    assert on.object_classes() == {'classes': 0, 'shared_slices': 0, 'slices': 1}
    assert on.simulated_images() == 4


@pytest.mark.parametrize('size,dtype,V', [(200, 'f32', 1), (128, 'f64', 2)])
def test_batch_run_tasks_share_objects_with_their_own_seeds(lib, size, dtype, V):
    """rl_batch_run over chunks of two-frame slices on two lanes; every task has its own seed and image id."""
    from oracle import philox_poisson as pp
    B, n_tasks, K = 6, 10, 2
    mb = {200: '0.001', 128: '2.2'}[size]
    off, on = plans(lib, small_psfs(V), B, size, size, dtype, options={'RLSTED_CHUNK_MB': mb, 'RLSTED_LANES': '2'})
    kinds = objects('ABC', size, size)
    which = [0, 0, 0, 0, 1, 1, 2, 2, 0, 0]
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
    # the last chunk: C C A A A A (the short chunk repeats its last task) -- three sharing slices, two classes
    assert on.object_classes() == {'classes': 2, 'shared_slices': 3, 'slices': 3}
    assert on.simulated_images() == 2 * V and off.simulated_images() == 6 * V
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert not np.array_equal(got[1][0][0], got[1][0][1])      # same object, own key
    # the twin, frame by frame of the last chunk, with the frame's key: tasks 6 .. 9, the last one repeated
    meas, lam = got[1][1], got[1][2]
    for f, t in enumerate([6, 7, 8, 9, 9, 9]):
        for v in range(V):
            want = pp.poisson(lam[f, v].ravel(), 1000 + 7 * t, (50 - t) * V + v).reshape(size, size) + 1e-9
            if dtype == 'f32':
                want = want.astype(np.float32).astype(np.float64)
            assert np.array_equal(meas[f, v], want), (f, v)


def test_512_specialised_kernels(lib, golden):
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    off, on = plans(lib, psf, 4, 512, 512, 'f32')
    assert on.info()['lx'] == 576 and on.strategy()['frame_pairs']
    for p in (off, on):
        p.set_object(objects('AAAB', 512, 512), 8e11)
    same_cycles(off, on, K=2, seeds=(5,))
    assert on.simulated_images() == 2


def test_timing_a_cycle_counts_the_class_simulation(lib):
    """rl_deconv_time_cycle on a sharing plan: the simulation's launches are those of one class simulation per cycle, and a kernel
    kind without launches (K = 0: no RL kernels) reports an average of 0."""
    _, on = plans(lib, small_psfs(1), 8, 128, 128, 'f64', options={'RLSTED_CHUNK_MB': '2.0', 'RLSTED_LANES': '2'})
    on.set_object(objects('AAAAAAAA', 128, 128), 3e7)
    avg = (ctypes.c_double * 8)()
    launches = (ctypes.c_double * 8)()
    fpl = ctypes.c_double()
    lib.check(lib.lib.rl_deconv_time_cycle(on.handle, 0, lib.RNG_PHILOX, ctypes.c_uint64(3), avg, launches, ctypes.byref(fpl)))
    info = on.object_classes()
    assert info['slices'] > 1 and info['shared_slices'] == info['slices']
    assert on.simulated_images() == 1
    # column pass and ROW_INV of the one class simulation; its ROW_FWD beside the one K = 0 runs per slice for the estimate's
    # spectrum; the sampler once per slice
    assert launches[0] == 1 and launches[5] == 1 and launches[4] == 1 + info['slices'] and launches[6] == info['slices']
    assert all(np.isfinite(avg[i]) for i in range(8))
    assert avg[1] == 0.0 and launches[1] == 0 and avg[3] == 0.0 and launches[3] == 0     # no ROW_RATIO, no ROW_UPDATE
