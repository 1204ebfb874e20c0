"""Parity of the HIP path (through the C ABI / ctypes) with the CPU oracle and
with the committed golden vectors of the reference.  Needs an MI355X.

Tolerances (stated once):
  f64 plans : agreement with the float64 reference to 1e-10 normwise, 1e-8
              pixelwise on RL estimates (same arithmetic, different FFT sizes)
  f32 plans : <= 1e-5 normwise (max|a-b| / max|b|) up to 20 RL iterations --
              the BASELINE.json tolerance; a single convolution <= 2e-6.
"""
import os

import numpy as np
import pytest

from conftest import max_rel, fuzz_seeds
from oracle import line_sted_oracle as orc

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5
F64_TOL = 1e-10


@pytest.fixture(scope='module')
def st():
    from rescan_line_sted_amd import line_sted_tools
    return line_sted_tools


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


def pixelwise(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---------------------------------------------------------------- H / H_t
@pytest.mark.parametrize('dtype,tol', [('f64', 1e-12), ('f32', 2e-6)])
def test_g4_conv_conventions(st, golden, dtype, tol, tmp_path):
    g = golden('g4_conv')
    for name in ('odd', 'even', 'row', 'big', 'two'):
        x, psfs, y = g[name + '/x'], g[name + '/psfs'], g[name + '/y']
        d = st.Deconvolver(list(psfs), output_prefix=str(tmp_path) + '/', verbose=False, dtype=dtype)
        H = d.H(x)
        for i in range(len(psfs)):
            assert max_rel(H[i], g[name + '/H'][i]) < tol, (name, i)
        assert max_rel(d.H_t(list(y), normalize=False), g[name + '/Ht_raw']) < tol, name
        assert max_rel(d.H_t(list(y)), g[name + '/Ht']) < 5 * tol, name
        assert max_rel(d.H_t_normalization, g[name + '/norm']) < tol, name


# ------------------------------------------------ simulate + RL vs goldens
@pytest.mark.parametrize('run,ks', [('rings_point_1p5x', (1, 2, 5, 20, 100)),
                                    ('rings_line4_2p0x', (1, 5, 20)),
                                    ('cat_line1_1p0x', (5,))])
def test_g5_rl_f64_matches_reference(lib, golden, run, ks):
    g, psfs, objs = golden('g5_rl'), golden('g8_fig2_psfs'), golden('objects')
    psf_set = [p[None] for p in psfs[str(g[run + '/psf_key'])][:, 0]]
    obj = objs[str(g[run + '/object'])].astype(np.float64)
    plan = lib.DeconvPlan(psf_set, 1, obj.shape[1], obj.shape[2], dtype='f64')
    plan.set_object(obj, 5e10)
    assert max_rel(plan.noiseless()[0], g[run + '/noiseless'][:, 0]) < 1e-12
    assert max_rel(plan.normalization(), g[run + '/norm'][0]) < 1e-12
    plan.set_measurement(g[run + '/noisy'][:, 0][None])
    done = 0
    for k in ks:
        plan.iterate(k - done)
        done = k
        ref = g[run + '/estimate_%d' % k][0]
        est = plan.estimate()[0]
        assert max_rel(est, ref) < F64_TOL, (run, k)
        assert pixelwise(est, ref) < 1e-8, (run, k)


@pytest.mark.parametrize('run,ks', [('rings_point_1p5x', (1, 5, 20)),
                                    ('rings_line4_2p0x', (1, 5, 20))])
def test_g5_rl_f32_within_baseline_tolerance(lib, golden, run, ks):
    g, psfs, objs = golden('g5_rl'), golden('g8_fig2_psfs'), golden('objects')
    psf_set = [p[None] for p in psfs[str(g[run + '/psf_key'])][:, 0]]
    obj = objs[str(g[run + '/object'])].astype(np.float64)
    plan = lib.DeconvPlan(psf_set, 1, obj.shape[1], obj.shape[2], dtype='f32')
    plan.set_object(obj, 5e10)
    assert max_rel(plan.noiseless()[0], g[run + '/noiseless'][:, 0]) < 2e-6
    plan.set_measurement(g[run + '/noisy'][:, 0][None])
    done = 0
    for k in ks:
        plan.iterate(k - done)
        done = k
        assert max_rel(plan.estimate()[0], g[run + '/estimate_%d' % k][0]) < F32_TOL, (run, k)


def test_drop_in_deconvolver_reproduces_reference_run(st, golden, tmp_path):
    """The reference's own call sequence (line_sted_figure_2.py:39-56) through
    the mirror class, numpy RNG on the host, f64 device arithmetic."""
    g, psfs, objs = golden('g5_rl'), golden('g8_fig2_psfs'), golden('objects')
    run = 'rings_point_1p5x'
    d = st.Deconvolver(list(psfs['1p5x_lr/point_sted_psf']), str(tmp_path) + '/x_', verbose=False)
    d.create_data_from_object(objs['rings'].astype(np.float64), total_brightness=5e10, random_seed=0)
    assert max_rel(d.noiseless_measurement[0], g[run + '/noiseless'][0]) < 1e-12
    # same lambda to 1e-13 and the same MT19937 stream -> the same Poisson draws
    assert (d.noisy_measurement[0] == g[run + '/noisy'][0]).mean() > 0.999
    d.noisy_measurement = [g[run + '/noisy'][0]]
    d._measurement_on_device = False
    for i, save in st.logarithmic_progress(range(5), verbose=False):
        d.iterate()
        if save:
            d.record_iteration(save_tifs=False)
    assert d.num_iterations == 5 and d.saved_iterations == [2, 3, 5]
    assert max_rel(d.estimate, g[run + '/estimate_5']) < F64_TOL
    assert d.estimate.shape == (1, 128, 128) and d.estimate.dtype == np.float64


def test_record_and_load_round_trip(st, golden, tmp_path):
    """record_data / record_iteration (ref:533-565) write ImageJ TIFs through the np_tif
    mirror; load_data_from_tif (ref:514-518) feeds a saved measurement back in."""
    from rescan_line_sted_amd import np_tif
    g, psfs, objs = golden('g5_rl'), golden('g8_fig2_psfs'), golden('objects')
    prefix = str(tmp_path / 'out') + '/rings_'
    d = st.Deconvolver(list(psfs['1p5x_lr/point_sted_psf']), prefix, verbose=False)
    d.create_data_from_object(objs['rings'].astype(np.float64), total_brightness=5e10, random_seed=0)
    d.record_data()
    for name, shape in (('psfs', (1, 107, 107)), ('object', (1, 128, 128)),
                        ('noiseless_measurement', (1, 128, 128)), ('noisy_measurement', (1, 128, 128))):
        a = np_tif.tif_to_array(prefix + name + '.tif')
        assert a.shape == shape and a.dtype == np.float32
    assert np.array_equal(np_tif.tif_to_array(prefix + 'object.tif'), d.true_object.astype(np.float32))
    for i, save in st.logarithmic_progress(range(3), verbose=False):
        d.iterate()
        if save:
            d.record_iteration()
    hist = np_tif.tif_to_array(prefix + 'estimate_history.tif')
    assert hist.shape == (2, 128, 128) and d.saved_iterations == [2, 3]
    assert np.array_equal(hist[-1], d.estimate[0].astype(np.float32))
    ft = np_tif.tif_to_array(prefix + 'estimate_FT_error_history.tif')
    want = np.log(1 + np.abs(np.fft.fftshift(np.fft.fftn(d.estimate - d.true_object, axes=(1, 2)), axes=(1, 2))))
    assert max_rel(ft[-1], want[0]) < 1e-6
    # a second deconvolver that only sees the saved measurement
    e = st.Deconvolver(list(psfs['1p5x_lr/point_sted_psf']), prefix, verbose=False)
    e.load_data_from_tif(prefix + 'noisy_measurement.tif')
    for _ in range(3):
        e.iterate()
    assert max_rel(e.estimate, d.estimate) < 1e-6            # the TIF stores float32


# ----------------------------------------- BASELINE size: 512 x 512, K = 20
@pytest.fixture(scope='module')
def astronaut512(golden):
    obj = golden('objects')['astronaut'].astype(np.float64)
    return np.kron(obj, np.ones((1, 4, 4)))


@pytest.mark.parametrize('dtype,tol', [('f32', F32_TOL), ('f64', F64_TOL)])
def test_512_point_sted_cycle_vs_oracle(lib, golden, astronaut512, dtype, tol):
    psf = golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf']
    K = 20
    d = orc.Deconvolver(list(psf))
    d.create_data_from_object(astronaut512, total_brightness=8e11, random_seed=1)
    plan = lib.DeconvPlan(list(psf), 1, 512, 512, dtype=dtype)
    assert plan.info()['ly'] == 576 and plan.info()['lx'] == 576
    plan.set_object(astronaut512, 8e11)
    assert max_rel(plan.noiseless()[0, 0], d.noiseless_measurement[0][0]) < (2e-6 if dtype == 'f32' else 1e-12)
    plan.set_measurement(np.array(d.noisy_measurement)[:, 0][None])
    plan.iterate(K)
    for _ in range(K):
        d.iterate()
    assert max_rel(plan.estimate()[0], d.estimate[0]) < tol


def test_batch_of_frames_equals_frames_run_alone(lib, golden, astronaut512):
    psfs = [p[None] for p in golden('g8_fig2_psfs')['2p0x_lr/line_sted_psfs'][:, 0]]
    rng = np.random.default_rng(7)
    objs = np.stack([astronaut512[0], np.flipud(astronaut512[0]), rng.random((512, 512)) * 255])
    plan = lib.DeconvPlan(psfs, 3, 512, 512, dtype='f32')
    plan.set_object(objs, [8e11, 4e11, 1e11])
    plan.simulate(seed=11)
    plan.iterate(3)
    est, noisy = plan.estimate(), plan.measurement()
    one = lib.DeconvPlan(psfs, 1, 512, 512, dtype='f32')
    for f, tb in enumerate([8e11, 4e11, 1e11]):
        one.set_object(objs[f:f + 1], tb)
        one.set_measurement(noisy[f:f + 1])
        one.iterate(3)
        assert np.array_equal(one.estimate()[0], est[f])      # bitwise: no cross-frame coupling


def test_many_frames_persistent_column_kernel_orders(lib, golden):
    """B = 16 (work items a multiple of 8: XCD-contiguous order) and B = 5 (fallback
    order) through the persistent column kernel equal frames computed one by one."""
    psf = list(golden('g8_fig2_psfs')['1p5x_lr/point_sted_psf'])
    rng = np.random.default_rng(21)
    one = lib.DeconvPlan(psf, 1, 128, 128, dtype='f32')
    for B in (16, 5):
        objs = rng.random((B, 128, 128)) * 100
        plan = lib.DeconvPlan(psf, B, 128, 128, dtype='f32')
        plan.set_object(objs, 1e9)
        plan.simulate(seed=B)
        plan.iterate(3)
        est, noisy = plan.estimate(), plan.measurement()
        for f in (0, B // 2, B - 1):
            one.set_object(objs[f:f + 1], 1e9)
            one.set_measurement(noisy[f:f + 1])
            one.iterate(3)
            assert np.array_equal(one.estimate()[0], est[f])


@pytest.mark.parametrize('dtype,tol', [('f32', F32_TOL), ('f64', F64_TOL)])
def test_kernel_flavours_agree(lib, golden, astronaut512, dtype, tol):
    """The RL loop has switchable schedules (options of a plan, read when it is made): in place = single-view
    iterations entirely in spec_a (RLSTED_INPLACE; 0 also means the per-frame loop instead of frame pairs), the batch
    cut into slices (RLSTED_CHUNK_MB) that are iterated on RLSTED_LANES concurrent streams, the column kernel's tile
    order (RLSTED_COL_ORDER), frame pairs on / off.  Every combination must give the default's result (same arithmetic,
    schedule and buffers differ; only the compiler's fma contraction may differ between two instantiations) and the
    oracle's.  B = 19 frames of 512x512: an item count that is not a multiple of 8 (fallback work order), an odd
    frame count (the last pair half empty)."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    rng = np.random.default_rng(5)
    B, K = 19, 6
    objs = np.concatenate([astronaut512, rng.random((B - 1, 512, 512)) * 200])
    d = orc.Deconvolver(psf)
    d.create_data_from_object(objs[:2], total_brightness=2 * 8e11, random_seed=3)
    for _ in range(K):
        d.iterate()
    results = {}
    noisy = None
    # (frame pairs, in place, concurrent slice streams, slice budget in MB: 10 MB = 3 frames)
    for stream, inplace, lanes, mb in (('0', '1', '2', '108'), ('1', '1', '2', '108'), ('0', '0', '1', '10'),
                                       ('1', '1', '4', '10'), ('0', '0', '3', '20'), ('1', '1', '1', '100000'),
                                       ('0', '1', '1', '100000')):
        # (the complex PSF-spectrum multiplier throughout: the real one is a separate compilation with its own fma contraction)
        options = {'RLSTED_REAL_PSF': '0',
                   'RLSTED_COL_ORDER': {'10': '3', '100000': '64'}.get(mb, '1'),   # image blocks of the tile order
                   'RLSTED_PAIR': stream, 'RLSTED_INPLACE': inplace, 'RLSTED_LANES': lanes, 'RLSTED_CHUNK_MB': mb}
        plan = lib.DeconvPlan(psf, B, 512, 512, dtype=dtype, options=options)
        plan.set_object(objs, 8e11)
        if noisy is None:
            plan.simulate(seed=9)
            noisy = plan.measurement()
            noisy[:2, 0] = np.array(d.noisy_measurement)[0]       # frames 0, 1: the oracle's draw
        plan.set_measurement(noisy)
        plan.iterate(K)
        results[(stream, inplace, lanes, mb)] = plan.estimate()
        del plan
    ref = results[('0', '1', '2', '108')]
    assert max_rel(ref[:2], d.estimate) < tol
    for key, est in results.items():
        assert max_rel(est, ref) < (2e-6 if dtype == 'f32' else 1e-13), key
    # default plans: real multiplier for the (point-symmetric) PSF spectrum, first iteration from the shared H(1)
    plan = lib.DeconvPlan(psf, B, 512, 512, dtype=dtype)
    plan.set_object(objs, 8e11)
    plan.set_measurement(noisy)
    plan.iterate(K)
    assert max_rel(plan.estimate()[:2], d.estimate) < tol
    assert max_rel(plan.estimate(), ref) < (4e-6 if dtype == 'f32' else 1e-12)


@pytest.mark.parametrize('B,K', [(11, 4), (12, 5)])
@pytest.mark.parametrize('lanes,mb', [('1', '100000'), ('2', '10'), ('3', '7')])
def test_bench_cycle_equals_simulate_then_iterate(lib, golden, astronaut512, lanes, mb, B, K):
    """bench.py's timed call (rl_deconv_bench_cycles: forward model, Poisson, est = 1 and K
    iterations per slice of the batch, slices on concurrent streams) leaves exactly what
    rl_deconv_simulate + rl_deconv_iterate over the whole batch leave.  Frame pairs (B = 11: the last pair half empty),
    the last iteration's spectrum dropped (K = 5), lane joins deferred between the cycles -- the path bench.py times."""
    options = {'RLSTED_LANES': lanes, 'RLSTED_CHUNK_MB': mb}
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    rng = np.random.default_rng(17)
    objs = np.concatenate([astronaut512, rng.random((B - 1, 512, 512)) * 200])
    a = lib.DeconvPlan(psf, B, 512, 512, dtype='f32', options=options)
    assert a.strategy()['frame_pairs']               # (an odd batch leaves its last pair half empty)
    a.set_object(objs, 8e11)
    a.bench_cycles(K, 3, seed=39)                      # three cycles back to back (no lane join in between): seeds 39, 40, 41; the last one stays
    b = lib.DeconvPlan(psf, B, 512, 512, dtype='f32', options=options)
    b.set_object(objs, 8e11)
    b.simulate(seed=41)
    b.iterate(K)
    assert np.array_equal(a.noiseless(), b.noiseless())
    assert np.array_equal(a.measurement(), b.measurement())
    assert np.array_equal(a.estimate(), b.estimate())


@pytest.mark.parametrize('seed', fuzz_seeds(6))
def test_random_schedules_bench_cycle_equals_stepwise_calls(lib, seed):
    """Soak test of the schedule (RLSTED_FUZZ_SEEDS): random batch sizes, iteration counts, slice sizes (RLSTED_CHUNK_MB down to
    one frame per slice), 1-4 slices in flight, 1-3 views, f32 / f64, pair loop or per-frame loop, dense or sparse objects -- the
    cycle bench.py times leaves bit for bit what simulate + iterate over the whole batch leave, back to back cycles included."""
    rng = np.random.default_rng(81000 + seed)
    ny, nx = int(rng.integers(20, 200)), int(rng.integers(20, 200))
    V, B, K = int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(0, 6))
    dtype = ('f32', 'f64')[int(rng.integers(0, 2))]
    psfs = [rng.random((1, int(rng.integers(1, 16)), int(rng.integers(1, 16)))) + 0.01 for _ in range(V)]
    objs = rng.random((B, ny, nx)) * 50
    if rng.integers(0, 3) == 0:
        objs *= rng.random((B, ny, nx)) < 0.05
        objs[:, 0, 0] += 1.0
    frame_mb = ny * nx * 4 * 8 / 1e6
    options = {'RLSTED_LANES': str(int(rng.integers(1, 5))),
               'RLSTED_CHUNK_MB': '%g' % max(frame_mb * float(rng.choice([0.5, 2, 5, 1000])), 1e-3),
               'RLSTED_PAIR': str(int(rng.integers(0, 2)))}
    brightness = float(rng.choice([50.0, 1e4, 1e8])) * ny * nx
    cycles = int(rng.integers(1, 4))
    a = lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype, options=options)
    a.set_object(objs, brightness)
    a.bench_cycles(K, cycles, seed=100 + seed)
    b = lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype, options=options)
    b.set_object(objs, brightness)
    b.simulate(seed=100 + seed + cycles - 1)
    if K > 0:
        b.iterate(K)
    case = (ny, nx, V, B, K, dtype, cycles, a.strategy())
    assert np.array_equal(a.noiseless(), b.noiseless()), case
    assert np.array_equal(a.measurement(), b.measurement()), case
    if K > 0:
        assert np.array_equal(a.estimate(), b.estimate()), case


# ------------------------------------- BASELINE configs 3 and 5: large images
def test_2048_line_rescan_batch_vs_oracle(lib, golden):
    """Config 3 shape: synthetic 2048x2048 random object, line-rescan (4 views), a
    batch of noise seeds; 2 RL iterations against the oracle (a 20-iteration
    oracle run at this size takes minutes), then flux/positivity at K = 20."""
    psfs = [p[None] for p in golden('g8_fig2_psfs')['2p0x_lr/line_sted_psfs'][:, 0]]
    obj = np.random.default_rng(1234).random((1, 2048, 2048)) * 255
    plan = lib.DeconvPlan(psfs, 2, 2048, 2048, dtype='f32')
    assert plan.info()['ly'] == 2304
    plan.set_object(np.concatenate([obj, obj]), 5e10 * 256)
    plan.simulate(seed=5)
    noisy = plan.measurement()
    assert not np.array_equal(noisy[0], noisy[1])                # frames draw different noise
    d = orc.Deconvolver(psfs)
    d.create_data_from_object(obj, 5e10 * 256, noisy_measurement=list(noisy[0][:, None]))
    for v in range(4):
        assert max_rel(plan.noiseless()[0, v], d.noiseless_measurement[v][0]) < 2e-6
    plan.iterate(2)
    d.iterate()
    d.iterate()
    assert max_rel(plan.estimate()[0], d.estimate[0]) < F32_TOL
    plan.iterate(18)
    est = plan.estimate()
    assert np.isfinite(est).all() and est.min() >= 0


@pytest.mark.parametrize('ny,nx,B', [(2048, 2048, 2), (1801, 300, 3), (1302, 2011, 1), (4000, 600, 1)])
def test_split_column_pass_against_whole_pass(lib, golden, ny, nx, B):
    """Multi-view f32 plans whose column length is 2304 / 4608 run the split column pass (COL_SPLIT_FWD parks the column
    spectra in register-slot order; COL_SPLIT_INV per view for H, COL_SPLIT_INV_SUM for H_t): against the route through
    the whole per-image kernel and the pre-summed update (RLSTED_COL_SPLIT=0).  H_t sums the views' products before the
    inverse column transform instead of the views' spectra before the inverse row transform: the estimates agree to f32
    rounding; H is the same arithmetic in the same order either way (bit-identical noiseless images)."""
    psfs = [p[None] for p in golden('g8_fig2_psfs')['2p0x_lr/line_sted_psfs'][:3, 0]]
    obj = np.random.default_rng(ny + nx).random((B, ny, nx)) * 255
    est, sim = {}, {}
    for flag in ('0', '1'):
        plan = lib.DeconvPlan(psfs, B, ny, nx, dtype='f32', options={'RLSTED_COL_SPLIT': flag})
        assert plan.info()['ly'] == (4608 if ny > 2048 else 2304)
        assert plan.strategy()['split_column_pass'] == (flag == '1')
        plan.set_object(obj, 5e10 * ny * nx / 128 ** 2)
        plan.simulate(seed=9)
        sim[flag] = plan.noiseless()
        plan.iterate(3)
        est[flag] = plan.estimate()
        del plan
    assert np.array_equal(sim['0'], sim['1'])
    assert np.isfinite(est['1']).all() and max_rel(est['1'], est['0']) < 2e-6


def test_4096_tile_runs(lib, golden):
    """Config 5 shape (4096x4096, L = 4608): H against the oracle, f32 and f64."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    x = np.random.default_rng(4321).random((1, 4096, 4096))
    ref = orc.Deconvolver(psf).H(x)[0][0]
    for dtype, tol in (('f32', 2e-6), ('f64', 1e-12)):
        plan = lib.DeconvPlan(psf, 1, 4096, 4096, dtype=dtype)
        assert plan.info()['lx'] == 4608
        assert max_rel(plan.forward(x)[0, 0], ref) < tol
        del plan


@pytest.mark.parametrize('ny,nx,V,B', [(4000, 37, 1, 2), (3001, 20, 2, 1), (2000, 41, 3, 2), (1500, 70, 1, 3), (4096, 24, 1, 1), (620, 3000, 1, 1)])
def test_long_transforms_odd_shapes_vs_oracle(lib, ny, nx, V, B):
    """The long transforms (L = 1152 / 2304 / 4608 along y, once along x) on images whose row count is not the compile-time one
    and whose spectra do not fill whole column tiles -- float64: the outer-decimation column kernels with 2 / 4 / 8 residue
    classes, 0 / 10 / 28 waiting values parked in LDS, rows tested one by one -- through H, H_t and two RL iterations against the
    oracle; f32 at its tolerance.  Narrow images keep the oracle cheap."""
    rng = np.random.default_rng(ny + nx)
    psfs = [rng.random((1, 9, 7)) + 0.01 for _ in range(V)]
    x = rng.random((B, ny, nx)) * 20
    d = orc.Deconvolver(psfs)
    Hx = d.H(x)
    y = [rng.random((B, ny, nx)) for _ in range(V)]
    Ht = d.H_t(y)
    d.create_data_from_object(x, random_seed=5)
    d.iterate()
    d.iterate()
    for dtype, tol in (('f64', 1e-11), ('f32', F32_TOL)):
        plan = lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype)
        assert max(plan.info()['ly'], plan.info()['lx']) >= 1152
        got = plan.forward(x)
        for v in range(V):
            assert max_rel(got[:, v], Hx[v]) < tol, (dtype, 'H', v)
        assert max_rel(plan.adjoint(np.stack(y, axis=1)), Ht) < 5 * tol, (dtype, 'Ht')
        plan.set_measurement(np.stack(d.noisy_measurement, axis=1))
        plan.iterate(2)
        assert max_rel(plan.estimate(), d.estimate) < 10 * tol, (dtype, 'RL')
        del plan


# ---------------------------------------------- size independent properties
@pytest.mark.parametrize('shape,views', [((512, 512), None), ((500, 317), None), ((129, 64), None), ((2, 3), None),
                                         ((2048, 2048), None), ((4096, 4096), 1)])
def test_operator_properties(lib, golden, shape, views):
    """Size-independent properties of H and H_t, up to BASELINE's full sizes (config 3: 2048 x 2048 line-rescan; config 5's
    4096 x 4096 tile with one view: linearity, the clamp, the adjoint identity, H_t(ones) = ones, the energy bound."""
    ny, nx = shape
    psf = golden('g8_fig2_psfs')['1p5x_lr/line_sted_psfs'][:views, 0]
    psfs = [p[None] for p in psf]
    rng = np.random.default_rng(ny * 1000 + nx)
    plan = lib.DeconvPlan(psfs, 2, ny, nx, dtype='f64')
    x, z = rng.random((2, ny, nx)), rng.random((2, ny, nx))
    y = rng.random((2, len(psfs), ny, nx))
    Hx, Hz = plan.forward(x), plan.forward(z)
    assert max_rel(plan.forward(2 * x + 3 * z), 2 * Hx + 3 * Hz) < 1e-12          # linearity
    assert Hx.min() >= 0                                                           # clamp
    # adjoint identity (PSFs are point symmetric to ~1e-3 only after rotation, so use the flipped PSF set)
    flipped = lib.DeconvPlan([p[:, ::-1, ::-1] for p in psfs], 2, ny, nx, dtype='f64')
    lhs = float((Hx * y).sum())
    rhs = float((x * flipped.adjoint(y, normalize=False)).sum())
    assert abs(lhs - rhs) < 1e-10 * abs(lhs)
    ones = np.ones((2, len(psfs), ny, nx))
    assert max_rel(plan.adjoint(ones, normalize=True), np.ones((2, ny, nx))) < 1e-12   # H_t(ones) == ones
    # energy: with zero padding, sum(H x) <= sum(psf) * sum(x)
    for v, p in enumerate(psfs):
        assert Hx[:, v].sum() <= p.sum() * x.sum() * (1 + 1e-12)


def test_rl_preserves_flux_and_positivity(lib, golden, astronaut512):
    psf = golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf']
    plan = lib.DeconvPlan(list(psf), 1, 512, 512, dtype='f32')
    plan.set_object(astronaut512, 8e11)
    plan.simulate(seed=3)
    plan.iterate(20)
    est = plan.estimate()[0]
    assert np.isfinite(est).all() and est.min() >= 0
    assert plan.unresolved() == 0                         # the BASELINE workload: every prediction is resolved by the f32 transforms
    # RL with H_t(ones)-normalisation conserves the measured counts through H
    again = plan.forward(est[None])[0, 0]
    meas = plan.measurement()[0, 0]
    assert abs(again.sum() - meas.sum()) < 1e-3 * meas.sum()


def test_dark_background_narrow_psf_stays_finite(lib):
    """Sparse emitters on a black background, a PSF much narrower than the gaps, a low dose: most pixels count zero photons, the
    estimate falls to ~1e-9 there after one iteration (ref:510) and the prediction H(est) in the dark is below what an f32 transform
    resolves -- rounding noise of either sign.  The reference's arithmetic then divides by the clamped zero (ref:575, 524); the
    kernels make such a pixel neutral (conv_kernels.hpp rl_ratio).  f32 plans (pair loop and per-frame loop) stay finite and
    inside the normwise contract against the float64 plan; the float64 plan follows the oracle."""
    rng = np.random.default_rng(77)
    ny = nx = 256
    obj = np.zeros((2, ny, nx))
    for b in range(2):
        obj[b, rng.integers(8, ny - 8, 30), rng.integers(8, nx - 8, 30)] = rng.random(30) + 0.5
    yy, xx = np.mgrid[-4:5, -4:5]                         # an elliptical Gaussian at 30 degrees: narrow, and not rank 1 (the FFT path)
    u, w = 0.866 * xx + 0.5 * yy, -0.5 * xx + 0.866 * yy
    psf = [np.exp(-0.5 * ((u / 1.6) ** 2 + (w / 0.8) ** 2))[None]]
    p64 = lib.DeconvPlan(psf, 2, ny, nx, dtype='f64')
    p64.set_object(obj, 3e3)
    p64.simulate(seed=9)
    meas = p64.measurement()
    assert (meas < 0.5).mean() > 0.8                      # mostly zero counts
    d = orc.Deconvolver(psf)
    d.noisy_measurement = [meas[:, 0].copy()]
    d.estimate = np.ones_like(obj)
    K = 12
    for _ in range(K):
        d.iterate()
    assert np.isfinite(d.estimate).all()
    p64.iterate(K)
    e64 = p64.estimate()
    assert np.isfinite(e64).all()
    assert p64.unresolved() == 0                          # float64 resolves these predictions (14 decades)
    print('f64 plan vs oracle: %.2e; smallest prediction / largest: %.1e' % (max_rel(e64, d.estimate), d.H(d.estimate)[0].min() / d.H(d.estimate)[0].max()))
    assert max_rel(e64, d.estimate) < 1e-8
    for pair in ('1', '0'):
        p32 = lib.DeconvPlan(psf, 2, ny, nx, dtype='f32', options={'RLSTED_PAIR': pair})
        assert not p32.strategy()['separable']            # (a rank-1 PSF would run direct stencils: no cancellation there)
        p32.set_measurement(meas)
        p32.iterate(K)
        e32 = p32.estimate()
        assert np.isfinite(e32).all() and e32.min() >= 0 and e32.max() > 0
        assert p32.unresolved() > 0                        # ... and the plan says so: rl_deconv_unresolved
        assert p32.unresolved(reset=True) > 0 and p32.unresolved() == 0
        for b in range(2):
            err = max_rel(e32[b], e64[b])
            print('f32 (pairs %s) frame %d vs f64 plan: %.2e' % (pair, b, err))
            assert err < 1e-4, (pair, b, err)
        del p32


# ------------------------------------------------------------ device Poisson
def test_device_poisson_bit_exact_vs_oracle_twin(lib, golden):
    from oracle import philox_poisson as pp
    psf = golden('g8_fig2_psfs')['1p5x_lr/line_sted_psfs'][:, 0]
    psfs = [p[None] for p in psf]
    obj = golden('objects')['rings'].astype(np.float64)
    objs = np.stack([obj[0], obj[0].T])
    for dtype in ('f64', 'f32'):
        plan = lib.DeconvPlan(psfs, 2, 128, 128, dtype=dtype)
        # tiny, moderate and huge rates: multiplication method, PTRS slow path, PTRS fast path
        for tb, seed in ((3e3, 1), (4e5, 2), (5e10, 0xDEADBEEFCAFE)):
            plan.set_object(objs, tb)
            plan.simulate(seed=seed)
            lam = plan.noiseless().reshape(-1, 128, 128)      # exactly the rates the device used
            want = pp.noisy_measurement(lam, seed)
            if dtype == 'f32':
                want = want.astype(np.float32).astype(np.float64)
            got = plan.measurement().reshape(-1, 128, 128)
            assert np.array_equal(got, want), (dtype, tb)


@pytest.mark.parametrize('seed', fuzz_seeds(6))
def test_random_rates_poisson_bit_exact_vs_twin(lib, seed):
    """The device sampler on arbitrary rates (a 1 x 1 PSF: the rates are the object): log-uniform from 1e-12 to 1e15, the
    lam = 10 switch of the two methods from both sides, exact zeros, whole dark or whole bright tiles of the kernel's 2048-pixel
    work lists, random shapes and batch sizes -- bit for bit the numpy twin on the rates the device reports."""
    from oracle import philox_poisson as pp
    rng = np.random.default_rng(31000 + seed)
    ny, nx, B = int(rng.integers(1, 200)), int(rng.integers(1, 200)), int(rng.integers(1, 5))
    lam = 10.0 ** rng.uniform(-12, 15, (B, ny, nx))
    pick = rng.random((B, ny, nx))
    lam[pick < 0.10] = 0.0
    lam[(pick >= 0.10) & (pick < 0.20)] = 10.0 * (1 + rng.choice([-1e-15, 0.0, 1e-15, -1e-7, 1e-7], int(((pick >= 0.10) & (pick < 0.20)).sum())))
    lam[(pick >= 0.20) & (pick < 0.45)] = rng.uniform(0.0, 40.0, int(((pick >= 0.20) & (pick < 0.45)).sum()))
    flat = lam.reshape(-1)
    if flat.size > 5000:                                  # whole tiles of one kind
        flat[:2048] = rng.uniform(0.01, 9.9, 2048)
        flat[2048:4096] = rng.uniform(1e3, 1e6, 2048)
    for dtype in ('f64', 'f32'):
        plan = lib.DeconvPlan([np.ones((1, 1, 1))], B, ny, nx, dtype=dtype)
        plan.set_object(lam, None)
        key = int(rng.integers(0, 2 ** 62))
        plan.simulate(seed=key)
        rates = plan.noiseless().reshape(-1, ny, nx)
        assert np.abs(rates - lam).max() <= 1e-6 * lam.max()          # (H with a 1 x 1 PSF: the object up to the plan's rounding)
        want = pp.noisy_measurement(rates, key)
        if dtype == 'f32':
            want = want.astype(np.float32).astype(np.float64)
        assert np.array_equal(plan.measurement().reshape(-1, ny, nx), want), (dtype, ny, nx, B)
        del plan


@pytest.mark.parametrize('seed', fuzz_seeds(12))     # (a soak run: RLSTED_FUZZ_SEEDS=300)
def test_random_shapes_vs_oracle(lib, seed):
    """Random image / PSF shapes (odd sizes, even PSFs, 1-10 views, every transform length
    up to 1152) through H, H_t and two RL iterations, f64 against the oracle at 1e-11 and
    f32 at the BASELINE tolerance."""
    rng = np.random.default_rng(1000 + seed)
    target = [64, 192, 256, 576, 1152, 192, 256, 576, 64, 192, 576, 256][seed % 12]
    lo = {64: 2, 192: 70, 256: 200, 576: 260, 1152: 600}[target]
    py, px = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    hy, hx = max((py - 1) // 2, py - 1 - (py - 1) // 2), max((px - 1) // 2, px - 1 - (px - 1) // 2)
    ny = int(rng.integers(max(lo - hy, 1), target - hy + 1))
    nx = int(rng.integers(max(lo - hx, 1), target - hx + 1))
    if target == 1152:
        nx = int(rng.integers(2, 60))                     # keep the oracle cheap: only Ly is large
    V = int(rng.integers(1, 11)) if ny * nx < 40000 else int(rng.integers(1, 4))
    B = int(rng.integers(1, 4))
    psfs = [rng.random((1, py, px)) + 0.01 for _ in range(V)]
    x = rng.random((B, ny, nx)) * 20
    d = orc.Deconvolver(psfs)
    signed = seed % 4 == 3                            # H / H_t of SIGNED images: the clamps of ref:575 / 587 act on real negative values
    xs = x - 10.0 if signed else x
    Hx = d.H(xs)
    y = [rng.random((B, ny, nx)) - (0.5 if signed else 0.0) for _ in range(V)]
    Ht = d.H_t(y)
    d.create_data_from_object(x, random_seed=seed)
    d.iterate()
    # An FFT convolution resolves the prediction H(est) to eps * max only, the reference's as ours: where the smallest prediction
    # of the second iteration is below 1e-4 of the largest (a tiny image with narrow PSFs and zero counts: 1 seed in ~2000 of a
    # soak run, RLSTED_FUZZ_SEEDS), ratio = measurement / prediction carries that rounding into the estimate and two correct
    # implementations differ by more than the tolerance.  Such seeds check H, H_t and a finite, non-negative estimate.
    pred = d.H(d.estimate)
    well_posed = min(float(p.min()) for p in pred) > 1e-4 * max(float(p.max()) for p in pred)
    d.iterate()
    for dtype, tol in (('f64', 1e-11), ('f32', F32_TOL)):
        plan = lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype)
        info = plan.info()
        assert info['ly'] == lib.lib.rl_fft_length_for(ny + hy) and info['lx'] == lib.lib.rl_fft_length_for(nx + hx)
        got = plan.forward(xs)
        scale = max(float(np.abs(h).max()) for h in Hx) or 1.0          # (signed inputs can clamp a whole view to zero)
        for v in range(V):
            assert np.abs(got[:, v] - Hx[v]).max() < tol * scale * (20 if signed else 1), (dtype, 'H', v, ny, nx, py, px, V, signed)
        assert np.abs(plan.adjoint(np.stack(y, axis=1)) - Ht).max() < 5 * tol * max(float(np.abs(Ht).max()), 1e-300) * (20 if signed else 1), (dtype, 'Ht', ny, nx, py, px, V, signed)
        plan.set_measurement(np.stack(d.noisy_measurement, axis=1))
        plan.iterate(2)
        est = plan.estimate()
        assert np.isfinite(est).all() and est.min() >= 0
        if well_posed:
            assert max_rel(est, d.estimate) < 10 * tol, (dtype, 'RL', ny, nx, py, px, V)
        del plan


@pytest.mark.parametrize('seed', fuzz_seeds(8))
def test_random_hard_cases_vs_oracle(lib, seed):
    """The soak test's second half (RLSTED_FUZZ_SEEDS): what test_random_shapes_vs_oracle does not draw -- the long transforms
    (L = 1152 / 2304 / 4608 along one axis, the other kept narrow for the oracle), SPARSE objects at a low dose (most pixels count
    zero photons: the neutral-pixel rule of conv_kernels.hpp rl_ratio in every row body), the frame-pair loop against the
    per-frame loop, odd batches, and rl_batch_run against set_object / simulate / iterate.  Well-posed seeds compare the iterates
    with the oracle; every seed must stay finite and non-negative."""
    rng = np.random.default_rng(50000 + seed)
    long_axis = int(rng.integers(0, 3))                   # 0: no long axis, 1: y, 2: x
    big = int(rng.choice([1152, 2304, 4608]))
    py, px = int(rng.integers(1, 24)), int(rng.integers(1, 24))
    hy, hx = max((py - 1) // 2, py - 1 - (py - 1) // 2), max((px - 1) // 2, px - 1 - (px - 1) // 2)
    small = lambda h: int(rng.integers(2, 150))
    ny = int(rng.integers(big // 2 + 1, big - hy + 1)) if long_axis == 1 else small(hy)
    nx = int(rng.integers(big // 2 + 1, big - hx + 1)) if long_axis == 2 else small(hx)
    if long_axis:                                         # keep the oracle (and the upload) cheap
        if long_axis == 1:
            nx = min(nx, 48)
        else:
            ny = min(ny, 48)
    V = int(rng.integers(1, 5))
    B = int(rng.integers(1, 6))
    psfs = [rng.random((1, py, px)) + 0.01 for _ in range(V)]
    sparse = bool(rng.integers(0, 2))
    x = rng.random((B, ny, nx)) * 20
    if sparse:
        x *= rng.random((B, ny, nx)) < 0.03
        x[:, ny // 2, nx // 2] += 5.0                     # (never an empty frame)
    brightness = float(rng.choice([30.0, 3e3, 3e6])) * ny * nx / 100
    d = orc.Deconvolver(psfs)
    d.create_data_from_object(x, brightness, random_seed=seed)
    meas = np.stack(d.noisy_measurement, axis=1)
    K = 3
    well_posed = True
    d.estimate = np.ones_like(x)                          # (what the first iterate() starts from, ref:521-522)
    with np.errstate(all='ignore'):
        for _ in range(K):
            pred = d.H(d.estimate)
            lo, hi = min(float(p.min()) for p in pred), max(float(p.max()) for p in pred)
            well_posed = well_posed and np.isfinite(lo) and lo > 1e-4 * hi
            d.iterate()
    results = {}
    for dtype, tol in (('f64', 1e-10), ('f32', 3e-5)):
        for pair in ('0', '1'):
            plan = lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype, options={'RLSTED_PAIR': pair})
            plan.set_measurement(meas)
            plan.iterate(K)
            est = plan.estimate()
            assert np.isfinite(est).all() and est.min() >= 0 and est.max() > 0, (dtype, pair, ny, nx, py, px, V, B, sparse)
            if well_posed:
                assert max_rel(est, d.estimate) < tol, (dtype, pair, 'RL', ny, nx, py, px, V, B, sparse, brightness)
            results[dtype, pair] = est
            del plan
        if well_posed:                                    # the two loops of one arithmetic type agree much closer than with the oracle
            assert max_rel(results[dtype, '1'], results[dtype, '0']) < (1e-11 if dtype == 'f64' else 2e-5)
    # the batch call: scale, H, keyed Poisson draws, K iterations in one enqueue -- the same frames as the stepwise calls with the same keys
    if ny * nx <= 200 * 200:
        plan = lib.DeconvPlan(psfs, B, ny, nx, dtype='f64')
        seeds, ids = [int(s) for s in rng.integers(0, 2 ** 40, B)], [int(i) for i in rng.integers(0, 1000, B)]
        got = plan.batch_run(list(x), brightness, seeds, ids, K)
        plan.set_object(x, brightness)
        plan.simulate_keyed(seeds, ids)
        plan.iterate(K)
        assert np.array_equal(got, plan.estimate()), ('batch', ny, nx, V, B)


def test_edge_cases(lib):
    rng = np.random.default_rng(0)
    # PSF larger than the image, 1-pixel image, single row / column
    for (ny, nx, py, px) in ((3, 4, 9, 11), (1, 1, 5, 5), (1, 37, 3, 7), (41, 1, 7, 3)):
        psfs = [rng.random((1, py, px))]
        x = rng.random((1, ny, nx))
        plan = lib.DeconvPlan(psfs, 1, ny, nx, dtype='f64')
        ref = orc.Deconvolver(psfs).H(x)[0]
        assert max_rel(plan.forward(x)[0, 0], ref[0]) < 1e-12
    # all-zero object: noiseless 0, Poisson(0) + 1e-9 = 1e-9, RL stays finite
    plan = lib.DeconvPlan([rng.random((1, 5, 5))], 1, 16, 16, dtype='f64')
    plan.set_object(np.zeros((1, 16, 16)))
    plan.simulate(seed=1)
    assert np.all(plan.measurement() == 1e-9)
    plan.iterate(2)
    assert np.isfinite(plan.estimate()).all()
    # errors are reported, not swallowed
    with pytest.raises(lib.RlstedError):
        lib.DeconvPlan([rng.random((1, 5, 5))], 1, 5000, 5000, dtype='f32')    # > largest built length
    fresh = lib.DeconvPlan([rng.random((1, 5, 5))], 1, 16, 16)
    with pytest.raises(lib.RlstedError):
        fresh.iterate(1)                                                          # no measurement yet


# ------------------------------------- frame pairs (two frames in one complex image) in the RL loop
@pytest.mark.parametrize('ny,nx,B', [(30, 41, 2), (128, 128, 4), (190, 203, 6), (245, 140, 2), (511, 300, 2), (200, 500, 4), (190, 203, 17), (190, 203, 3)])
def test_frame_pair_loop_equals_per_frame_loop(lib, ny, nx, B):
    """RLSTED_PAIR=1 (default for single-view plans with an even batch on the wave-private lengths 64 ... 576): the RL
    loop transforms frames 2p and 2p+1 as the real and imaginary part of one complex image.  Same estimates as the
    per-frame loop (f64: rounding level), also across set_estimate / forward calls that invalidate the spectra."""
    rng = np.random.default_rng(ny + nx)
    psf = [(rng.random((1, 9, 12)) + 0.02)]
    x = rng.random((B, ny, nx)) * 40
    out = {}
    for flag in ('1', '0'):
        plan = lib.DeconvPlan(psf, B, ny, nx, dtype='f64', options={'RLSTED_PAIR': flag})
        info = plan.info()                   # pairs exist where both transforms are one-per-wave: L = 256, 576
        assert plan.strategy()['frame_pairs'] == (flag == '1' and info['ly'] in (256, 576) and info['lx'] in (256, 576))
        plan.set_object(x, 1e7)
        plan.simulate(seed=3)
        plan.iterate(5)                      # a run of >= 4: its last iteration leaves no spectrum of the estimate behind ...
        plan.iterate(1)                      # ... and a continuation rebuilds it
        a = plan.estimate()
        plan.forward(x)                      # clobbers the spectra: the next iterate rebuilds them from the estimate
        plan.iterate(2)
        b = plan.estimate()
        plan.set_estimate(b * 1.5)
        plan.iterate(1)
        out[flag] = (a, b, plan.estimate(), plan.measurement())
    assert np.array_equal(out['1'][3], out['0'][3])
    for i in range(3):
        assert max_rel(out['1'][i], out['0'][i]) < 1e-12, i
    d = orc.Deconvolver(psf)
    d.create_data_from_object(x[:1], noisy_measurement=[out['1'][3][:1, 0]])
    for _ in range(6):
        d.iterate()
    assert max_rel(out['1'][0][0], d.estimate[0]) < 1e-11


def test_frame_pair_loop_f32_within_contract(lib, golden, astronaut512):
    """f32: the pair loop is as accurate as the per-frame loop (same transforms, the packing / splitting arithmetic
    gone), BASELINE object and white noise alike, a factor of three inside the contract after 20 iterations."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    noise = np.random.default_rng(5).random((2, 512, 512)) * 200
    objs = np.concatenate([astronaut512, astronaut512.transpose(0, 2, 1), noise])
    ref = lib.DeconvPlan(psf, 4, 512, 512, dtype='f64', options={'RLSTED_PAIR': '0'})
    ref.set_object(objs, 8e11)
    ref.simulate(seed=11)
    noisy = ref.measurement()
    ref.iterate(20)
    err = {}
    for flag in ('1', '0'):
        plan = lib.DeconvPlan(psf, 4, 512, 512, dtype='f32', options={'RLSTED_PAIR': flag})
        plan.set_object(objs, 8e11)
        plan.set_measurement(noisy)
        plan.iterate(20)
        err[flag] = [max_rel(plan.estimate()[f], ref.estimate()[f]) for f in range(4)]
    print('pairs / per frame:', err)
    assert max(err['1'] + err['0']) < 3e-6, err                         # measured 0.7 ... 0.9e-6 (round 2: 0.75 ... 1.0e-5)
    assert np.mean(err['1']) < 1.25 * np.mean(err['0']), err


def test_f32_plan_with_negative_psf_values_keeps_the_plain_iteration(lib):
    """`ratio - 1` (conv_kernels.hpp rl_ratio) needs H_t(ones) == the normaliser, i.e. PSF values >= 0; a PSF with negative
    lobes makes the plan fall back to the plain arithmetic (ref:527-530 literally), with the exact normaliser still
    clamped per view (ref:587).  Both against the oracle, two views, f32."""
    rng = np.random.default_rng(31)
    pos = [rng.random((1, 9, 11)) + 0.05, rng.random((1, 9, 11)) + 0.05]
    neg = [p.copy() for p in pos]
    neg[1][0, 0, :3] = -0.02                                  # a small negative lobe at the edge of one view
    x = rng.random((2, 60, 75)) * 50 + 5
    for psfs in (pos, neg):
        d = orc.Deconvolver(psfs)
        d.create_data_from_object(x, 1e8, random_seed=2)
        plan = lib.DeconvPlan(psfs, 2, 60, 75, dtype='f32')
        plan.set_object(x, [1e8 * x[0].sum() / x.sum(), 1e8 * x[1].sum() / x.sum()])
        plan.set_measurement(np.stack(d.noisy_measurement, axis=1))
        d.H_t(d.noisy_measurement)                              # creates the oracle's normaliser (ref:589-592)
        assert max_rel(plan.normalization(), d.H_t_normalization) < 1e-6
        for _ in range(10):
            d.iterate()
        plan.iterate(10)
        assert max_rel(plan.estimate(), d.estimate) < 5e-6


def test_512_point_sted_100_iterations_f32_inside_the_contract(lib, golden, astronaut512):
    """The BASELINE object (astronaut 512 x 512, point-descan STED) carried to 100 iterations -- five times what the 1e-5
    contract is quoted for: f32 plan (frame pairs, the default) against the f64 plan on the same measurement."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    objs = np.concatenate([astronaut512, astronaut512.transpose(0, 2, 1)])
    p64 = lib.DeconvPlan(psf, 2, 512, 512, dtype='f64')
    p64.set_object(objs, 8e11)
    p64.simulate(seed=4)
    p32 = lib.DeconvPlan(psf, 2, 512, 512, dtype='f32')
    assert p32.strategy()['frame_pairs']
    p32.set_object(objs, 8e11)
    p32.set_measurement(p64.measurement())
    errs, done = {}, 0
    for k in (20, 100):
        p64.iterate(k - done)
        p32.iterate(k - done)
        done = k
        errs[k] = max(max_rel(p32.estimate()[f], p64.estimate()[f]) for f in range(2))
    print('f32 vs f64, astronaut 512^2:', errs)
    assert errs[20] < 3e-6 and errs[100] < F32_TOL, errs


# ------------------------------------------------- the long row lengths, per pixel against a long-double reference
def _long_row_radices():
    """radix lists of the row kernels of 1152 / 2304 / 4608 and of the 64-row column kernel, read from fft_configs.hpp"""
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rescan_line_sted_amd', 'csrc', 'fft_configs.hpp')).read()
    out = {}
    for L in (64, 1152, 2304, 4608):
        m = re.search(r'struct CfgFor<%d> \{.*?using Cfg = FftCfg<%d, \d+, ([\d, ]+)>;' % (L, L), text, flags=re.S)
        out[L] = tuple(int(r) for r in m.group(1).split(','))
    return out


@pytest.mark.parametrize('L', [1152, 2304, 4608])
def test_long_rows_per_pixel_against_long_double(lib, L):
    """The edge table of tests/test_long_rows_cpu.py at plan level: a one-row PSF of 61 taps (no stencil strategy takes it, the
    column transforms stay at 64), so that H and one Richardson-Lucy iteration have an affordable long-double reference -- the
    convolution sums themselves.  f64 and f32 plans (frame pairs with a phantom partner, `ratio - 1`), every pixel within the
    bound propagated as tests/fft_reference.py derives it; no tolerance is a literal.  The bound is K x (L1 of what shares the
    transforms) x (L1 of the PSF), a worst case met only where one pixel and one tap carry those sums: the one-pixel edges under the
    PSF with 95 % in its centre tap are the sharp cases (H of the lit pixel: error / bound 0.011-0.020 on the device, the bound
    ~1e-5 of the peak in float, ~1e-14 in float64 -- finer than the plan tolerances of the other tests).  The dense edges and the
    iteration are structural at this level (error / bound < 1e-3): an iteration's prediction is dense whatever the estimate -- a
    dim floor under a lit pixel is known only to K x L1 absolutely, 1e-5 / floor relatively, and 60 such neighbours reach every
    pixel of `ratio` through the PSF -- so its sharp check is the CPU module's row chain."""
    import fft_reference as fr
    LD = fr.LD
    radices = _long_row_radices()
    px, hx = 61, 30
    rng = np.random.default_rng(L)
    taps_flat = (rng.random(px) + 0.05)
    taps_flat /= taps_flat.sum()
    hi = L - hx
    lo = hi
    while lib.lib.rl_fft_length_for(lo - 1 + hx) == L:
        lo -= 1
    table = fr.edge_rows(lo, hi)          # the CPU module's table, at the image widths that select L with this PSF
    assert lib.lib.rl_fft_length_for(1 + hx) != L
    for edge, (ny, nx, kind) in table.items():
        if nx == 1:             # a plan of one-pixel rows selects the shortest length (asserted above; test_edge_cases runs it): the
            assert edge in ('one pixel wide', 'one column')      # long row bodies meet nx = 1 in the CPU module alone
            continue
        B = 3
        obj = (rng.random((B, ny, nx)) * 3 + 0.5).astype(np.float32).astype(np.float64)
        meas = (rng.random((B, 1, ny, nx)) * 5).astype(np.float32).astype(np.float64)
        if kind == 'one_pixel':
            o2 = np.zeros_like(obj)
            o2[:, ny // 2, 2 * nx // 3] = 100.0
            obj = o2
            m2 = np.zeros_like(meas)
            m2[:, :, ny // 2, nx // 3] = 7.0
            meas = m2
        if kind == 'zero_row':
            obj[:, :2] = 0
            meas[:, :, :2] = 0
        if kind == 'negative':
            meas[rng.random(meas.shape) < 0.2] *= -1
        # The bound is (L1 of the frame) x (L1 of the PSF): met only where one pixel AND one tap carry the sums.  The one-pixel edges
        # therefore run a second PSF too, 95 % of it in the centre tap: H of the lit pixel is then the sharp case of this test.
        variants = [('', taps_flat)]
        if kind == 'one_pixel':
            peaked = 0.05 * taps_flat
            peaked[hx] += 0.95
            variants.append((', peaked PSF', peaked))
        for pname, taps in variants:
            psf = taps.reshape(1, 1, px)
            h1 = LD(np.abs(taps).sum())
            for dtype in ('f64', 'f32'):
                T = np.float32 if dtype == 'f32' else np.float64
                plan = lib.DeconvPlan([psf], B, ny, nx, dtype=dtype)
                st_ = plan.strategy()
                assert plan.info()['lx'] == L and plan.info()['ly'] == 64 and not st_['separable'] and not st_['direct_stencil'], (edge, st_)
                pairs = dtype == 'f32'        # (frame pairs are the f32 single-view loop; where a launch is per frame the partner's share only widens the bound)
                sub_one = dtype == 'f32'
                K = fr.plan_conv_growth(radices[L], radices[64], T, px) * h1
                ar = fr.Arith(T, radices[L], div=3 if dtype == 'f32' else 1)

                def shared_l1(x):          # L1 norm of what shares a frame's transforms: the frame, and its partner in a frame pair
                    s = np.abs(np.asarray(x, dtype=LD)).reshape(B, -1).sum(axis=1)
                    if not pairs:
                        return s
                    partner = [b + 1 if b % 2 == 0 else b - 1 for b in range(B)]
                    return s + np.array([s[p] if p < B else s[b] for b, p in enumerate(partner)], dtype=LD)
                key = ('plan', dtype, L, ('one pixel lit' if kind == 'one_pixel' else 'dense rows') + pname)
                ctx = (edge, ny, nx, kind, dtype, pname)
                # H (the sharp case: frame 0 alone carries its pair's sum -- its partner is dark)
                x = obj.copy()
                if pname:
                    x[1] = 0
                got = plan.forward(x)[:, 0]
                ref = fr.conv_same_x(x, taps)
                e = (K * shared_l1(x))[:, None, None]
                fr.check(got, np.maximum(ref, 0), np.broadcast_to(e, ref.shape), key + ('H',), ctx)
                # one iteration from estimate = 1
                plan.set_measurement(meas)
                plan.reset_estimate()
                plan.iterate(1)
                est = plan.estimate()
                norm = plan.normalization().astype(LD)
                ones = np.ones((B, ny, nx), dtype=LD)
                pred = fr.conv_same_x(ones, taps)
                e_pred = (K * shared_l1(ones))[:, None, None]
                r, dr, undecided = ar.ratio(meas[:, 0], pred, np.broadcast_to(e_pred, pred.shape), sub_one)
                assert not undecided.any(), ctx
                a = fr.conv_same_x(r, taps)
                da = fr.conv_same_x(dr, np.abs(taps)) + (K * (shared_l1(r) + shared_l1(dr)))[:, None, None]
                fac, dfac = ar.factor(a if sub_one else np.maximum(a, 0), da, norm, sub_one)
                new, dnew = ar.product(ones, fac, dfac)
                fr.check(est, new, dnew, key + ('iteration',), ctx)
                assert plan.unresolved() == 0
                del plan
    for line in fr.WORST.lines():
        if "plan" in line and str(L) in line:
            print(line)


def test_float64_multi_view_ratio_minus_one_on_the_longest_rows(lib):
    """A float64 row transform of 4608 needs more than the default 64 KB of dynamic LDS.  The multi-view `ratio - 1` update
    (rowpass_body PRESUM; float64 plans run it with RLSTED_SUB_ONE=1) was missing from the kernels prepare() raises the limit of
    (tests/test_long_rows_cpu.py::test_every_launchable_row_kernel_may_use_its_lds): the launch must succeed and agree with the
    plain float64 iteration, which is the same iteration in exact arithmetic."""
    rng = np.random.default_rng(4608)
    ny, nx, B, px = 4, 2400, 1, 61
    psfs = [(rng.random((1, 1, px)) + 0.05) for _ in range(2)]
    meas = rng.random((B, 2, ny, nx)) * 5 + 0.5
    est = []
    for sub in ('0', '1'):
        plan = lib.DeconvPlan(psfs, B, ny, nx, dtype='f64', options={'RLSTED_SUB_ONE': sub})
        assert plan.info()['lx'] == 4608 and not plan.strategy()['separable'] and not plan.strategy()['direct_stencil']
        plan.set_measurement(meas)
        plan.iterate(3)
        est.append(plan.estimate())
        del plan
    assert np.isfinite(est[1]).all()
    assert max_rel(est[1], est[0]) < F64_TOL
