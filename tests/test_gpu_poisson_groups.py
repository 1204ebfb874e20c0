"""The frame-group Poisson kernel on the device (aux_kernels.hip k_poisson_groups, csrc/poisson_kernels.hpp; include/rlsted.h
rl_deconv_grouped_draws).  Needs an MI355X.

A sharing slice's Philox draw runs in groups of 8 frames per 256-pixel tile, with the sampler's rate-only set-up evaluated once per
pixel and run of frames that read one rate image.  Every case builds the same plan twice in one process, with
RLSTED_POISSON_GROUPS=0 -- k_poisson everywhere -- and with the default, runs the same cycles on both and compares measurement and
estimate with np.array_equal, no tolerance: a draw is philox_poisson(rate, the frame's key, the frame's image id, pixel) in either
kernel.  The getter proves which kernel ran.  The measurement is also compared with the numpy twin (oracle/philox_poisson.py) on
the rates the plan reports.

Shapes as in test_gpu_class_poisson.py: a 9 x 9 PSF that is not rank 1 keeps the plans on the FFT path; 128 x 128 is a multiple
of the 256-pixel tile, 200 x 200 leaves a ragged last tile (40000 = 156 * 256 + 64).
"""
import functools

import numpy as np
import pytest

from plan_cases import plans_per_value

pytestmark = pytest.mark.gpu

SEEDS = (5, (1 << 40) + 3)


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def small_psfs(V, seed=3, unit_sum=False):
    rng = np.random.default_rng(seed)
    psfs = [rng.random((1, 9, 9)) + 0.05 for _ in range(V)]
    return [p / p.sum() for p in psfs] if unit_sum else psfs


def objects(pattern, ny, nx, seed=11):
    rng = np.random.default_rng(seed)
    kinds = {c: rng.random((ny, nx)) * 200 + 1 for c in sorted(set(pattern))}
    return np.stack([kinds[c] for c in pattern])


# (k_poisson plan, frame-group plan: the default) = plans(lib, psfs, B, ny, nx, dtype, options=None)
plans = functools.partial(plans_per_value, switch='RLSTED_POISSON_GROUPS', values=('0', None))


def twin(plan, dtype, seed):
    """The numpy twin's draws from the rates the plan reports (image = frame * V + view, one seed for the batch)."""
    from oracle import philox_poisson as pp
    lam = plan.noiseless()
    want = pp.noisy_measurement(lam.reshape((-1,) + lam.shape[2:]), seed).reshape(lam.shape)
    return want.astype(np.float32).astype(np.float64) if dtype == 'f32' else want


def same_cycles(off, on, K, seeds=SEEDS, cycles=1):
    for seed in seeds:
        for p in (off, on):
            p.bench_cycles(K, cycles, seed=seed)
        assert np.array_equal(off.measurement(), on.measurement()), seed
        assert np.array_equal(off.estimate(), on.estimate()), seed
    assert np.array_equal(off.noiseless(), on.noiseless())
    info = on.object_classes()
    assert off.grouped_draws() == 0
    assert on.grouped_draws() == info['shared_slices']
    return info


@pytest.mark.parametrize('pattern', ['AAAAAAAAA', 'AABABCA', 'ABABABAB'])
@pytest.mark.parametrize('V', [1, 2])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('size', [128, 200])
def test_grouped_draw_is_the_per_frame_draw(lib, size, dtype, V, pattern):
    """B = 9, 7 and 8: a short second group, a single short group, one full group; one run, runs of 2 + 1 + ..., eight runs."""
    off, on = plans(lib, small_psfs(V), len(pattern), size, size, dtype)
    for p in (off, on):
        p.set_object(objects(pattern, size, size), 3e7 * (size / 128) ** 2)
    info = same_cycles(off, on, K=2)
    assert info['shared_slices'] == info['slices'] == 1 and info['classes'] == len(set(pattern))
    assert np.array_equal(on.measurement(), twin(on, dtype, SEEDS[-1]))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_zero_pixels_and_a_ramp_across_ten(lib, dtype):
    """A dark block and a ramp whose rates cross 10 inside one image: PTRS, the multiplication method and the exact zero meet
    in a tile and in a run."""
    size, V = 128, 2
    rng = np.random.default_rng(19)
    a = rng.random((size, size)) * np.linspace(0.02, 4.0, size)[None, :]
    a[40:90, 10:70] = 0.0
    b = rng.random((size, size)) * 200 + 1
    objs = np.stack([a, a, b, a, a, b, a, a, a, a, a])
    off, on = plans(lib, small_psfs(V), len(objs), size, size, dtype)
    for p in (off, on):
        p.set_object(objs, 7000.0)
    same_cycles(off, on, K=2)
    lam = on.noiseless()[0, 0]
    assert (lam >= 10.0).sum() > 1000 and ((lam > 0) & (lam < 10.0)).sum() > 1000 and (lam[50:80, 20:60] < 1e-3).all()
    assert on.grouped_draws() == 1
    assert np.array_equal(on.measurement(), twin(on, dtype, SEEDS[-1]))


@pytest.mark.parametrize('size,dtype', [(200, 'f32'), (128, 'f64')])
def test_rates_between_ten_and_thirty(lib, size, dtype):
    """Where the squeeze rejects most often and every list is long: most draws go to the rounds."""
    B = 10
    rng = np.random.default_rng(23)
    obj = rng.random((size, size)) * 0.8 + 0.6
    off, on = plans(lib, small_psfs(1, unit_sum=True), B, size, size, dtype)
    for p in (off, on):
        p.set_object(np.broadcast_to(obj, (B, size, size)), 20.0 * size * size)
    same_cycles(off, on, K=2)
    lam = on.noiseless()
    share = ((lam >= 10.0) & (lam <= 30.0)).mean()
    print('rates in [10, 30]: %.3f of the pixels' % share)
    assert share > 0.8
    assert on.grouped_draws() == 1
    assert np.array_equal(on.measurement(), twin(on, dtype, SEEDS[-1]))


def test_slices_on_two_lanes_and_a_per_frame_slice(lib):
    """A B C D | A A A A | E E F F in slices of four on two lanes: the first slice does not share and draws through k_poisson,
    the others through the frame groups -- in one cycle."""
    off, on = plans(lib, small_psfs(1), 12, 128, 128, 'f64', options={'RLSTED_CHUNK_MB': '2.0', 'RLSTED_LANES': '2'})
    for p in (off, on):
        p.set_object(objects('ABCDAAAAEEFF', 128, 128), 3e7)
    info = same_cycles(off, on, K=2, seeds=(5, 6), cycles=2)
    assert info == {'classes': 6, 'shared_slices': 2, 'slices': 3}


def test_rng_none_keeps_the_per_frame_kernel(lib):
    off, on = plans(lib, small_psfs(1), 8, 128, 128, 'f32')
    for p in (off, on):
        p.set_object(objects('AAAAAAAA', 128, 128), 3e7)
        p.bench_cycles(2, 1, seed=1, rng=lib.RNG_NONE)
    assert np.array_equal(off.measurement(), on.measurement()) and np.array_equal(off.estimate(), on.estimate())
    assert on.object_classes()['shared_slices'] == 1 and on.grouped_draws() == 0


@pytest.mark.parametrize('size,dtype,V', [(200, 'f32', 1), (128, 'f64', 2)])
def test_batch_submit_with_per_frame_keys(lib, size, dtype, V):
    """rl_batch_submit: every task has its own seed and image id.  13 tasks in chunks of 9: the last chunk holds tasks 9 .. 12 and
    repeats the last one, C C A B B B B B B -- runs of 2 + 1 + 5 in the first group, a second group of one frame."""
    from oracle import philox_poisson as pp
    B, K = 9, 2
    kinds = objects('ABC', size, size)
    which = [0, 1, 2, 2, 0, 0, 0, 0, 0, 2, 2, 0, 1]
    seeds = [1000 + 7 * i + ((i % 3) << 34) for i in range(len(which))]
    ids = [50 - i for i in range(len(which))]
    off, on = plans(lib, small_psfs(V), B, size, size, dtype)
    got = []
    for p in (off, on):
        p.batch_submit([kinds[w] for w in which], 3e7, seeds, ids, K, None)
        p.ctx.synchronize()
        got.append((p.measurement(), p.estimate(), p.noiseless()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert off.grouped_draws() == 0 and on.grouped_draws() == on.object_classes()['shared_slices'] == 1
    meas, lam = got[1][0], got[1][2]
    tasks = [min(B + f, len(which) - 1) for f in range(B)]
    assert on.object_classes()['classes'] == 3 and not np.array_equal(meas[0], meas[1])      # same object, own key
    for f, t in enumerate(tasks):
        for v in range(V):
            want = pp.poisson(lam[f, v].ravel(), seeds[t], ids[t] * V + v).reshape(size, size) + 1e-9
            if dtype == 'f32':
                want = want.astype(np.float32).astype(np.float64)
            assert np.array_equal(meas[f, v], want), (f, v)


def test_512_with_the_sted_psf(lib, golden):
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    off, on = plans(lib, psf, 16, 512, 512, 'f32')
    assert on.info()['lx'] == 576 and on.strategy()['frame_pairs']
    for p in (off, on):
        p.set_object(objects('A' * 13 + 'BBA', 512, 512), 8e11)
    info = same_cycles(off, on, K=2, seeds=(5,))
    assert info['shared_slices'] == info['slices'] and on.grouped_draws() >= 1
