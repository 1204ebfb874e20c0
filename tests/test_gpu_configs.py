"""BASELINE.json configs 2, 3 and 5 in the driver-run suite (they lived in builder-run tools).

config 2: astronaut 512x512, point-descan vs line-rescan at the four STED doses 1p5x / 2p0x / 2p5x / 3p0x
          (line_sted_figure_2.py:93-148: 3, 4, 6, 8 line orientations), K = 20, f32, against the oracle.
          The eight PSF sets are made here by the product on the device (tune_psf, psf_report, rotations).
config 3 / 5 sizes: 2048^2 and 4096^2 at K = 20, f32 against the f64 plan (which agrees with the oracle
          to 1e-10 wherever the oracle is affordable: test_gpu_parity.py).

Error measure (stated once, also printed by bench.py): normwise max|a-b| / max|b|; the pixelwise figure
(max over pixels above 1e-3 of the maximum of |a-b| / b) is asserted for f32 as well.
"""
import numpy as np
import pytest

from conftest import max_rel
from oracle import line_sted_oracle as orc

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5          # BASELINE.json: <= 1e-5 relative, 20 RL iterations
F32_MARGIN = 3e-6       # what the f32 plans are held to at K = 20 since round 3 (measured 0.7 ... 1.0e-6: exact normaliser +
                        # `ratio - 1` transforms, conv_kernels.hpp rl_ratio); the contract itself is asserted at K = 100
F32_PIXELWISE = 3e-4    # pixels above 1e-3 of the maximum.  H(estimate)'s f32 transform error is white and proportional to the
                        # frame's RMS, so `measurement / H(estimate)` is 1e3 times less exact in regions 1e-3 as bright; H_t blurs
                        # that over the PSF, 20 iterations add up: 0.8 ... 2.3e-4 over the eight config-2 cases (the same in
                        # rounds 1-2: the `ratio - 1` transforms cure H_t's own error, not H's)


def pixelwise(a, b):
    big = b > 1e-3 * b.max()
    return float((np.abs(a - b)[big] / b[big]).max())


@pytest.fixture(scope='module')
def lib():
    from rescan_line_sted_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    return _lib


@pytest.fixture(scope='module')
def dose_sets():
    from rescan_line_sted_amd import psf
    sets, _ = psf.figure_2_psfs([d + '_lr' for d in ('1p5x', '2p0x', '2p5x', '3p0x')])
    return {k: [np.asarray(p) for p in v] for k, v in sets.items()}


@pytest.fixture(scope='module')
def astronaut512(golden):
    return np.kron(golden('objects')['astronaut'].astype(np.float64), np.ones((1, 4, 4)))[0]


def test_config_2_psf_sets(dose_sets):
    views = sorted(len(v) for v in dose_sets.values())
    assert views == [1, 1, 1, 1, 3, 4, 6, 8]
    assert all(p.shape == (1, 107, 107) for v in dose_sets.values() for p in v)


@pytest.mark.parametrize('dose,views', [('1p5x', 3), ('2p0x', 4), ('2p5x', 6), ('3p0x', 8)])
@pytest.mark.parametrize('mode', ['point', 'line'])
def test_config_2_cycle_vs_oracle(lib, dose_sets, astronaut512, dose, views, mode):
    key = dose + '_lr_point_sted' if mode == 'point' else '%s_lr_line_%d_angles_sted' % (dose, views)
    psfs = dose_sets[key]
    V, K = len(psfs), 20
    plan = lib.DeconvPlan(psfs, 2, 512, 512, dtype='f32')
    plan.set_object(np.stack([astronaut512, astronaut512]), 5e10 * 16)
    plan.simulate(seed=17)
    plan.iterate(K)
    noisy = plan.measurement()[1]                     # frame 1's device-drawn (Philox) measurement
    d = orc.Deconvolver(psfs)
    d.noisy_measurement = [noisy[v][None] for v in range(V)]
    for _ in range(K):
        d.iterate()
    est, ref = plan.estimate()[1], d.estimate[0]
    assert max_rel(est, ref) < F32_MARGIN, (key, max_rel(est, ref))
    assert pixelwise(est, ref) < F32_PIXELWISE, (key, pixelwise(est, ref))


@pytest.mark.parametrize('size', [1024, 2048, 4096])
def test_large_tiles_f32_vs_f64_plan(lib, golden, size):
    """White-noise objects (every frequency carries weight: the hardest input for f32), f32 against the f64 plan on the
    same noisy measurement.  Rounds 1-2 drifted by ~4-5e-7 of the maximum per RL iteration (8.7e-6 ... 9.7e-6 at K = 20,
    4.5e-5 at K = 100): the f32 transform path's rounding noise in the normaliser H_t(ones) and in H_t(ratio) was
    multiplied into the estimate again every iteration.  With the normaliser from the PSFs' integral images and the
    second half of the iteration on `ratio - 1` (conv_kernels.hpp rl_ratio) the same runs give 0.9 ... 1.0e-6 at K = 20
    and 1.5 ... 1.7e-6 at K = 100 (profiles/r03/f32_error.json) -- the 1e-5 contract holds at BASELINE config 5's
    100 iterations, with margin.  f64 plans meet 1e-10 at every size."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    obj = np.random.default_rng(4321 if size == 4096 else 1234).random((1, size, size)) * 255
    p64 = lib.DeconvPlan(psf, 1, size, size, dtype='f64')
    p64.set_object(obj, 5e10 * (size // 128) ** 2)
    p64.simulate(seed=9)
    noisy = p64.measurement()
    p32 = lib.DeconvPlan(psf, 1, size, size, dtype='f32')
    p32.set_object(obj, 5e10 * (size // 128) ** 2)
    p32.set_measurement(noisy)
    errs, done = {}, 0
    for k in (20, 100) if size == 4096 else (20,):     # 4096^2, K = 100: BASELINE config 5's tile and iteration count
        p64.iterate(k - done)
        p32.iterate(k - done)
        done = k
        errs[k] = max_rel(p32.estimate()[0], p64.estimate()[0])
    print('f32 vs f64 at %d^2: %s' % (size, errs))
    assert errs[20] < F32_MARGIN, errs
    if 100 in errs:
        assert errs[100] < F32_TOL, errs                # the contract, at five times the iterations it is quoted for
        assert errs[100] < 4 * errs[20], errs           # growth is sub-linear now (was 5x for 5x the iterations)


@pytest.mark.parametrize('ny,nx,views', [(2048, 2048, 2), (1024, 1024, 4), (2048, 2048, 5), (600, 4096, 3), (4000, 600, 3)])
def test_multi_view_long_transforms_f32_vs_f64_plan(lib, golden, ny, nx, views):
    """Multi-view plans on the long transforms, f32 against the f64 plan (same noisy measurement, K = 20).  L = 1152 runs V
    per-image column launches (colconv_outer_body, M = 2) and the pre-summed update (rowpass_body PRESUM: the views'
    `ratio - 1` spectra are added on their way in, ONE inverse row transform, the sum clamped); L = 2304 / 4608 the split
    column pass (COL_SPLIT_FWD / COL_SPLIT_INV / COL_SPLIT_INV_SUM: the views' products summed before one inverse column
    transform)."""
    g = golden('g8_fig2_psfs')
    base = g['2p0x_lr/line_sted_psfs'][:, 0]
    psfs = [np.roll(base[v % len(base)], v // len(base), axis=1)[None] for v in range(views)]
    obj = np.random.default_rng(ny + views).random((1, ny, nx)) * 255
    p64 = lib.DeconvPlan(psfs, 1, ny, nx, dtype='f64')
    p64.set_object(obj, 5e10 * ny * nx / 128 ** 2)
    p64.simulate(seed=3)
    p32 = lib.DeconvPlan(psfs, 1, ny, nx, dtype='f32')
    p32.set_object(obj, 5e10 * ny * nx / 128 ** 2)
    p32.set_measurement(p64.measurement())
    p64.iterate(20)
    p32.iterate(20)
    err = max_rel(p32.estimate()[0], p64.estimate()[0])
    print('f32 vs f64, %d x %d, %d views: %.2e' % (ny, nx, views, err))
    assert err < F32_MARGIN, err


@pytest.mark.parametrize('ny,nx,B', [(2048, 100, 2), (1500, 33, 3), (4096, 40, 2), (1100, 1100, 1), (700, 2048, 2)])
def test_single_view_long_columns_odd_shapes(lib, golden, ny, nx, B):
    """The whole column pass of the long transforms (16-column tiles at L = 2304, twiddle copies and parked values in LDS, the next
    residue class prefetched) on shapes whose spectra do not fill whole tiles: tall and narrow images, a single frame (no pair),
    an odd batch (half-empty last pair); f32 against the f64 plan, pair loop and per-frame loop."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    obj = np.random.default_rng(ny + nx).random((B, ny, nx)) * 255
    p64 = lib.DeconvPlan(psf, B, ny, nx, dtype='f64')
    p64.set_object(obj, 5e10 * ny * nx / 128 ** 2)
    p64.simulate(seed=4)
    noisy = p64.measurement()
    p64.iterate(10)
    ref = p64.estimate()
    for flag in ('1', '0'):
        p32 = lib.DeconvPlan(psf, B, ny, nx, dtype='f32', options={'RLSTED_PAIR': flag})
        p32.set_object(obj, 5e10 * ny * nx / 128 ** 2)
        p32.set_measurement(noisy)
        p32.iterate(10)
        err = max(max_rel(p32.estimate()[b], ref[b]) for b in range(B))
        assert err < F32_MARGIN, (flag, err)
        del p32


@pytest.mark.parametrize('size', [2048, 4096])
def test_frame_pairs_on_the_long_transforms(lib, golden, size):
    """L = 2304 / 4608 (one workgroup-synchronous row transform per workgroup): the frame-pair loop (the default for f32
    single-view plans at every size since round 3) against the per-frame loop (RLSTED_PAIR=0) and against the f64 plan,
    two white-noise frames, K = 20.  Rounds 1-2 kept pairs opt-in here because f32 had no margin left (0.87 ... 1.11e-5);
    both loops now sit near 1e-6."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    obj = np.random.default_rng(size).random((2, size, size)) * 255
    p64 = lib.DeconvPlan(psf, 2, size, size, dtype='f64')
    p64.set_object(obj, 5e10 * (size // 128) ** 2)
    p64.simulate(seed=9)
    noisy = p64.measurement()
    p64.iterate(20)
    ref = p64.estimate()
    del p64
    est = {}
    for flag in ('1', '0'):
        p32 = lib.DeconvPlan(psf, 2, size, size, dtype='f32', options={'RLSTED_PAIR': flag})
        assert p32.strategy()['frame_pairs'] == (flag == '1')
        p32.set_object(obj, 5e10 * (size // 128) ** 2)
        p32.set_measurement(noisy)
        p32.iterate(20)
        est[flag] = p32.estimate()
        del p32
    errs = {f: [max_rel(est[f][i], ref[i]) for i in range(2)] for f in est}
    print('f32 vs f64 at %d^2, K = 20, pairs / per frame: %s' % (size, errs))
    assert max(errs['1']) < F32_MARGIN and max(errs['0']) < F32_MARGIN, errs
    assert max_rel(est['1'], est['0']) < F32_MARGIN                 # two f32 roundings of the same arithmetic
    assert lib.DeconvPlan(psf, 2, size, size, dtype='f32').strategy()['frame_pairs']   # default: pairs


def test_frame_pairs_need_partners_of_comparable_brightness(lib, golden, astronaut512):
    """A pair's two frames share one complex transform, so f32 rounding error scales with the BRIGHTER partner:
    the plan pairs frames only while every pair's levels are within a factor of 4 (RLSTED_PAIR_MAX_RATIO) and runs its
    per-frame loop otherwise.  Frame 1 is 1e4 times dimmer than frame 0 here; frames 2 / 3 differ by 2."""
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    objs = np.stack([astronaut512] * 4)
    levels = [8e11, 8e7, 8e11, 4e11]
    ref = lib.DeconvPlan(psf, 4, 512, 512, dtype='f64')
    ref.set_object(objs, levels)
    ref.simulate(seed=21)
    noisy = ref.measurement()
    ref.iterate(20)
    r = ref.estimate()
    errs = {}
    for force in (False, True):
        # forced: pair whatever the levels (what round 2 did)
        plan = lib.DeconvPlan(psf, 4, 512, 512, dtype='f32', options={'RLSTED_PAIR_MAX_RATIO': '1e30'} if force else None)
        assert plan.strategy()['frame_pairs']                       # the plan holds the pair loop ...
        plan.set_object(objs, levels)
        plan.set_measurement(noisy)
        assert plan.strategy()['frame_pairs'] == force              # ... and does not run it on this batch
        plan.iterate(20)
        errs[force] = [max_rel(plan.estimate()[f], r[f]) for f in range(4)]
    print('guarded / forced pairs, per frame:', errs)
    assert max(errs[False]) < F32_MARGIN, errs
    assert errs[True][1] > 10 * errs[False][1], errs                # the dim partner pays for the bright one when forced
    ok = lib.DeconvPlan(psf, 4, 512, 512, dtype='f32')              # comparable partners stay paired
    ok.set_object(objs, [8e11, 4e11, 2e11, 6e11])
    ok.simulate(seed=3)
    assert ok.strategy()['frame_pairs']


def test_measurement_written_through_the_device_pointer_is_not_paired_blindly(lib, golden, astronaut512):
    """rl_deconv_device_ptr(which = 1) hands out the measurement buffer (the zero-copy drop-in path); what the host
    knew about the frames' levels is void from then on, so the next run recomputes the per-frame sums on the device before it
    chooses between the pair loop and the per-frame loop."""
    import ctypes
    psf = list(golden('g8_fig2_psfs')['2p0x_lr/point_sted_psf'])
    plan = lib.DeconvPlan(psf, 4, 512, 512, dtype='f32')
    plan.set_object(np.stack([astronaut512] * 4), 8e11)
    plan.simulate(seed=5)
    assert plan.strategy()['frame_pairs']
    noisy = plan.measurement()

    def write_frame_1(values):      # straight into the plan's buffer (rl_device_upload at the address rl_deconv_device_ptr hands out)
        arr = plan.device_array('measurement')
        addr = arr.__cuda_array_interface__['data'][0] + 512 * 512 * 4      # frame 1 of the f32 buffer
        v = np.ascontiguousarray(values, dtype=np.float64)
        lib.check(lib.lib.rl_device_upload(plan.ctx.handle, ctypes.c_void_p(addr), lib.RL_F32, v.size, lib.ptr(v)))
    write_frame_1(noisy[1, 0] * 1e-4)                     # frame 1 now 1e4 times dimmer than its partner
    plan.reset_estimate()
    plan.iterate(2)
    assert not plan.strategy()['frame_pairs']             # the per-frame loop ran
    write_frame_1(noisy[1, 0])
    plan.reset_estimate()
    plan.iterate(2)
    assert plan.strategy()['frame_pairs']
    assert np.array_equal(plan.measurement(), noisy.astype(np.float32).astype(np.float64))


def test_multi_view_measurement_with_negative_pixels_keeps_the_per_view_clamp(lib, golden):
    """`ratio - 1` clamps the SUM of the views' back-projections, the reference each view's (ref:587); they agree
    unless a view's term is negative, which takes a negative measurement pixel.  A multi-view f32 plan whose uploaded
    measurement has negative pixels (background-subtracted data) therefore runs the plain arithmetic: bit for bit what
    RLSTED_SUB_ONE=0 gives, and the float64 plan's result within the f32 margin; so does RLSTED_FUSE_VIEWS=0."""
    psfs = [p[None] for p in golden('g8_fig2_psfs')['1p5x_lr/line_sted_psfs'][:, 0]]
    obj = golden('objects')['rings'].astype(np.float64)
    obj = obj + 0.25 * obj.max()                          # a pedestal: every pixel carries signal, the iteration stays well posed
    ref = lib.DeconvPlan(psfs, 2, 128, 128, dtype='f64')
    ref.set_object(np.stack([obj[0], 2 * obj[0]]), 2e7)
    ref.simulate(seed=9)
    noisy = ref.measurement() - 40.0                      # a background estimate subtracted ...
    rng = np.random.default_rng(5)
    dead = (rng.integers(0, 2, 60), rng.integers(0, len(psfs), 60), rng.integers(0, 128, 60), rng.integers(0, 128, 60))
    noisy[dead] = -rng.random(60) * 30 - 1                # ... and a few dead pixels below it: negative values
    assert (noisy < 0).sum() == len(set(zip(*[d.tolist() for d in dead]))) and noisy.mean() > 500
    ref.set_measurement(noisy)
    ref.iterate(6)
    # (not a vacuous comparison: the reference's arithmetic is finite here -- a measurement that is negative over whole dark regions
    # drives the estimate to zero there, the reference to nan and, until the end of round 4, both plans to equal all-zero frames)
    d = orc.Deconvolver(psfs)
    d.noisy_measurement = [noisy[:, v].copy() for v in range(len(psfs))]
    d.estimate = np.ones((2, 128, 128))
    for _ in range(6):
        d.iterate()
    assert np.isfinite(d.estimate).all() and d.estimate.min() > 0
    assert max_rel(ref.estimate(), d.estimate) < 1e-10
    out = {}
    for name, options in (('default', {}), ('plain', {'RLSTED_SUB_ONE': '0'}), ('per_view', {'RLSTED_FUSE_VIEWS': '0'})):
        plan = lib.DeconvPlan(psfs, 2, 128, 128, dtype='f32', options=options)
        plan.set_measurement(noisy)
        plan.iterate(6)
        out[name] = plan.estimate()
    assert np.array_equal(out['default'], out['plain'])
    assert max_rel(out['default'], ref.estimate()) < 2e-5 and max_rel(out['per_view'], ref.estimate()) < 2e-5
    clean = lib.DeconvPlan(psfs, 2, 128, 128, dtype='f32')      # without negative pixels the residual form runs (a different rounding path)
    clean.set_measurement(np.abs(noisy) + 1e-9)
    clean.iterate(6)
    plain = lib.DeconvPlan(psfs, 2, 128, 128, dtype='f32', options={'RLSTED_SUB_ONE': '0'})
    plain.set_measurement(np.abs(noisy) + 1e-9)
    plain.iterate(6)
    assert not np.array_equal(clean.estimate(), plain.estimate()) and max_rel(clean.estimate(), plain.estimate()) < 2e-5


# ---------------------------------------------------------------- BASELINE config 4: the full figure-2 sweep
def test_config_4_full_figure_2_sweep(lib, golden):
    """4 test objects x 6 doses x 3 scan modes (point-descan, line-descanned, line-rescanned) x 16 seeds = 1152 tasks
    (line_sted_figure_2.py:39-56,77-162), K = 20, f32, on one GPU through sweep.figure_2_sweep -- the 18 PSF sets are the
    product's own (tune_psf, psf_report, spline rotations on the device: 1 ... 10 views).  Three spot frames against
    the oracle on the device-drawn measurement; the sharded form of the same call is tests/test_sharding.py (gloo)."""
    from rescan_line_sted_amd import psf, sweep
    objs = golden('objects')
    objects = {n: objs[n][0].astype(np.float64) for n in ('astronaut', 'cat', 'lines', 'rings')}
    doses = ('1p0x', '1p5x', '2p0x', '2p5x', '3p0x', '4p0x')
    sets, _ = psf.figure_2_psfs([d + s for d in doses for s in ('_ld', '_lr')])
    psf_sets = {}
    for d in doses:
        psf_sets[d + '_point'] = [np.asarray(p) for p in sets[d + '_lr_point_sted']]
        for s in ('_ld', '_lr'):
            key = [k for k in sets if k.startswith(d + s + '_line_')]
            assert len(key) == 1
            psf_sets[d + s] = [np.asarray(p) for p in sets[key[0]]]
    assert sorted(len(v) for v in psf_sets.values()) == sorted([1] * 6 + [1, 3, 4, 6, 8, 10] + [2, 3, 4, 6, 8, 10])
    K = 20
    tasks, est = sweep.figure_2_sweep(objects, psf_sets, seeds=range(16), iterations=K, dtype='f32')
    assert len(tasks) == 1152 and len(est) == 1152
    assert all(np.isfinite(e).all() and e.min() >= 0 for e in est)
    ids = sweep.object_ids(objects)
    for i in (5, 700, 1151):                           # a point task, a mid-sweep line task, the last (10-view) one
        o, p, seed = tasks[i]
        ny, nx = objects[o].shape
        alone = lib.DeconvPlan(psf_sets[p], 1, ny, nx, dtype='f32')      # the task's measurement: its Philox key is (seed, object id),
        alone.set_object(objects[o][None], 5e10)                         # whatever it was batched with
        alone.simulate_keyed([seed], [ids[o]])
        noisy = alone.measurement()[0]
        d = orc.Deconvolver(psf_sets[p])
        d.noisy_measurement = [m[None] for m in noisy]
        for _ in range(K):
            d.iterate()
        assert est[i].shape == (ny, nx)
        assert max_rel(est[i], d.estimate[0]) < F32_MARGIN, (tasks[i], max_rel(est[i], d.estimate[0]))


# ---------------------------------------------------------------- BASELINE config 5: 4096^2, K = 100, fp32 vs 16-bit spectra
def test_config_5_tolerance_study(lib, tmp_path):
    """4096 x 4096 tile, 100 RL iterations, the f32 plan and the two 16-bit-spectrum study builds (`_build --variant
    q16 / qbf16`, built by __graft_entry__.build()) against the f64 plan: tools/gpu/gpu_tolerance_study.py, one process
    per library.  f32 stays inside the contract all the way; spectra rounded to fp16 / bf16 between the row and the
    column kernels leave it in the first iteration -- the study's finding, asserted here."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the study builds must be builds of HEAD (same C ABI as the product library): bring them up to date where a compiler is at
    # hand -- objects whose sources did not change are kept, so this costs nothing after __graft_entry__.build()
    import shutil
    from rescan_line_sted_amd import _build
    if shutil.which(_build.HIPCC) or os.path.exists(_build.HIPCC):
        for variant in ('q16', 'qbf16'):
            _build.build_variant(variant)
    out = str(tmp_path / 'study.json')
    subprocess.check_call([sys.executable, os.path.join(root, 'tools', 'gpu', 'gpu_tolerance_study.py'), '4096', '100', out])
    study = json.load(open(out))
    f32 = {r['iteration']: r['max_over_max'] for r in study['f32']}
    assert f32[20] < F32_MARGIN and f32[100] < F32_TOL, f32
    for mode in ('fp16_spectra', 'bf16_spectra'):
        assert isinstance(study[mode], list), 'study build missing: %r (run __graft_entry__.build())' % (study[mode],)
        q = {r['iteration']: r['max_over_max'] for r in study[mode]}
        assert q[1] > 10 * F32_TOL and q[20] > 100 * F32_TOL, (mode, q)   # three to four orders outside the contract
    keep = os.path.join(root, 'gpurun_out', 'r04')
    os.makedirs(keep, exist_ok=True)
    json.dump(study, open(os.path.join(keep, 'tolerance_study_4096.json'), 'w'), indent=1)
