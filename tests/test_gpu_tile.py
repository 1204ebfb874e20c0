"""Tiled Richardson-Lucy on the MI355X (include/rlsted.h rl_tile_gather, rl_tile_blend, rl_device_copy,
rl_deconv_measurement_written; rescan_line_sted_amd/tiling.py): the two kernels bit for bit against numpy (tests/tile_reference.py),
the device-written measurement against rl_deconv_set_measurement, deconvolve_tiled end to end against the tiled oracle on every
convolution strategy, the exactness condition against the oracle's WHOLE-image estimate, an image no single plan can hold, chunk
independence and the per-tile stopping rule."""
import ctypes

import numpy as np
import pytest

import tile_reference as tr

pytestmark = pytest.mark.gpu

RL_ERR_INVALID, RL_ERR_STATE = -1, -4
NP = {'f32': np.float32, 'f64': np.float64}
IP = ctypes.POINTER(ctypes.c_int)


def _lib():
    from rescan_line_sted_amd import _lib
    return _lib


class _Dev:
    """A device buffer of `dtype` holding a host array from element `shift` on (rl_device_alloc; shift 1: not 16-byte aligned)."""

    def __init__(self, host, dtype, shift=0):
        L = _lib()
        self.ctx = L.Context.get(0)
        self.dtype, self.code, self.esize = dtype, L.DTYPES[dtype], 4 if dtype == 'f32' else 8
        host = np.ascontiguousarray(host, dtype=np.float64)
        self.size = host.size
        self.base = ctypes.c_void_p()
        L.check(L.lib.rl_device_alloc(self.ctx.handle, (host.size + shift + 1) * self.esize, ctypes.byref(self.base)))
        self.dev = ctypes.c_void_p(self.base.value + shift * self.esize)
        L.check(L.lib.rl_device_upload(self.ctx.handle, self.dev, self.code, host.size, L.ptr(host)))

    def download(self):
        L = _lib()
        out = np.empty(self.size)
        L.check(L.lib.rl_device_download(self.ctx.handle, self.dev, self.code, self.size, L.ptr(out)))
        return out

    def __del__(self):
        L = _lib()
        if L.lib is not None and self.base.value:
            L.lib.rl_device_free(self.ctx.handle, self.base)
            self.base = ctypes.c_void_p()


def _ints(a):
    return a.ctypes.data_as(IP)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dst_dtype', ['f32', 'f64'])
@pytest.mark.parametrize('src_dtype', ['f32', 'f64'])
def test_gather_is_numpy_slicing(src_dtype, dst_dtype):
    L = _lib()
    rng = np.random.default_rng(11)
    F, V, NY, NX = 2, 2, 37, 53
    src = (rng.random((F, V, NY, NX)) + 0.25).astype(NP[src_dtype])
    lay = tr.Layout((NY, NX), (16, 24), (6, 8), 2)
    assert (len(lay.origins_y), len(lay.origins_x)) == (4, 3)
    slots = np.concatenate([[(-1, 0, 0)], lay.slots(F), [(-1, 3, 3), (-1, 0, 0)]]).astype(np.intc)
    want = tr.gather(src, slots, (16, 24), NP[dst_dtype])
    d_src = _Dev(src, src_dtype)
    for shift in (0, 1):                                            # 16-byte stores; element stores
        d_dst = _Dev(np.full(want.size, -7.0), dst_dtype, shift)
        L.check(L.lib.rl_tile_gather(d_src.ctx.handle, d_src.dev, d_src.code, F, V, NY, NX, _ints(slots), len(slots), 16, 24, d_dst.dev,
                                     d_dst.code))
        d_src.ctx.synchronize()
        got = d_dst.download().reshape(want.shape)
        assert np.array_equal(got, want.astype(np.float64)), shift
        assert np.all(got[0] == 1.0) and np.all(got[-1] == 1.0)


def test_gather_grows_its_workspace_behind_a_queued_call():
    """rl_tile_gather does not wait for its kernel.  A second call whose slot list outgrows the context's tile workspace (24 bytes,
    then 2400) finds the first still queued: the workspace waits for the stream before it frees the block the first call reads, and
    both destinations are numpy slicing bit for bit.  On a context of its own: the shared one's workspace has grown in other tests."""
    L = _lib()
    rng = np.random.default_rng(12)
    src = rng.random((1, 1, 16, 16)) + 0.25
    few = np.array([(0, 3, 5), (-1, 0, 0)], dtype=np.intc)
    real = [(0, int(ay), int(ax)) for ay, ax in rng.integers(0, 9, (197, 2))]
    many = np.array([(-1, 0, 0)] + real + [(-1, 3, 3), (-1, 0, 0)], dtype=np.intc)
    assert (few.nbytes, many.nbytes) == (24, 2400)
    d_src = _Dev(src, 'f64')
    dsts = [_Dev(np.full(len(s) * 64, -7.0), 'f64', 1) for s in (few, many)]
    ctx = L.Context(0)
    try:
        for s, d in zip((few, many), dsts):                             # at once: nothing waits between the two calls
            L.check(L.lib.rl_tile_gather(ctx.handle, d_src.dev, d_src.code, 1, 1, 16, 16, _ints(s), len(s), 8, 8, d.dev, d.code))
        ctx.synchronize()
        for s, d in zip((few, many), dsts):
            want = tr.gather(src, s, (8, 8), np.float64)
            got = d.download().reshape(want.shape)
            assert np.array_equal(got, want), len(s)
        assert np.all(got[0] == 1.0) and np.all(got[-1] == 1.0)
    finally:
        L.check(L.lib.rl_ctx_destroy(ctx.handle))


def test_gather_and_blend_reject_bad_geometry():
    L = _lib()
    d = _Dev(np.zeros(2 * 37 * 53), 'f32')
    o = _Dev(np.zeros(4 * 16 * 24), 'f32')

    def gather(slots, F=1, V=2, NY=37, NX=53, ty=16, tx=24, dst=None, dt=0):
        s = np.array(slots, dtype=np.intc)
        return L.lib.rl_tile_gather(d.ctx.handle, d.dev, 0, F, V, NY, NX, _ints(s), len(s), ty, tx, o.dev if dst is None else dst, dt)
    assert gather([(0, 0, 0), (-1, 0, 0)]) == 0
    for bad in ([(1, 0, 0)], [(-2, 0, 0)], [(0, 22, 0)], [(0, 0, 30)], [(0, -1, 0)]):
        assert gather(bad) == RL_ERR_INVALID, bad
    assert gather([(0, 0, 0)], ty=40) == RL_ERR_INVALID and gather([(0, 0, 0)], V=0) == RL_ERR_INVALID
    assert gather([(0, 0, 0)], dt=2) == RL_ERR_INVALID and gather([(0, 0, 0)], dst=d.dev) == RL_ERR_INVALID
    lay = tr.Layout((37, 53), (16, 24), (6, 8), 2)
    oy, ox = lay.origins_y.astype(np.intc), lay.origins_x.astype(np.intc)
    tiles = _Dev(np.zeros(12 * 16 * 24), 'f64')
    out = _Dev(np.zeros(37 * 53), 'f64')

    def blend(oy=oy, ox=ox, ty=16, out_dev=out.dev):
        return L.lib.rl_tile_blend(d.ctx.handle, tiles.dev, 1, 1, 37, 53, len(oy), len(ox), ty, 24, _ints(oy), _ints(ox), L.ptr(lay.weights_y),
                                   L.ptr(lay.weights_x), out_dev, 1)
    assert blend() == 0
    assert blend(oy=oy[::-1].copy()) == RL_ERR_INVALID                 # decreasing
    assert blend(oy=np.array([0, 7, 14, 22], dtype=np.intc)) == RL_ERR_INVALID      # overhangs
    assert blend(oy=np.array([0, 0, 0, 21], dtype=np.intc)) == RL_ERR_INVALID       # rows 16 .. 20 uncovered
    assert blend(ty=0) == RL_ERR_INVALID and blend(out_dev=tiles.dev) == RL_ERR_INVALID
    assert L.lib.rl_device_copy(d.ctx.handle, out.dev, out.dev, 64) == RL_ERR_INVALID
    assert L.lib.rl_device_copy(d.ctx.handle, None, out.dev, 64) == RL_ERR_INVALID
    d.ctx.synchronize()


@pytest.mark.parametrize('case', [((150, 131), 64, 24, 8), ((64, 128), 64, 24, 0), ((105, 128), 64, 24, 8)], ids=lambda c: '%dx%d' % c[0])
def test_blend_is_the_numpy_twin_and_repeats(case):
    """f32 and f64 stores and outputs, an aligned output (16-byte stores where NX allows) and one an element off; two runs, same bytes."""
    L = _lib()
    shape, tile, overlap, margin = case
    lay = tr.Layout(shape, tile, overlap, margin)
    oy, ox = lay.origins_y.astype(np.intc), lay.origins_x.astype(np.intc)
    F = 2
    rng = np.random.default_rng(shape[1])
    for store_dtype, out_dtype in (('f32', 'f32'), ('f64', 'f64'), ('f32', 'f64'), ('f64', 'f32')):
        tiles = (rng.random((F, len(oy), len(ox)) + lay.tile_shape) + 0.25).astype(NP[store_dtype])
        want = tr.blend(tiles, lay, NP[out_dtype]).astype(np.float64)
        d_tiles = _Dev(tiles, store_dtype)
        for shift in (0, 1):
            runs = []
            for _ in range(2):
                d_out = _Dev(np.full(want.size, -7.0), out_dtype, shift)
                L.check(L.lib.rl_tile_blend(d_tiles.ctx.handle, d_tiles.dev, d_tiles.code, F, shape[0], shape[1], len(oy), len(ox),
                                            lay.tile_shape[0], lay.tile_shape[1], _ints(oy), _ints(ox), L.ptr(lay.weights_y),
                                            L.ptr(lay.weights_x), d_out.dev, d_out.code))
                runs.append(d_out.download().reshape(want.shape))
            assert runs[0].tobytes() == runs[1].tobytes()
            assert np.array_equal(runs[0], want), (store_dtype, out_dtype, shift)


# ---- a measurement written on the device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_measurement_written_is_set_measurement_without_the_upload(dtype):
    L = _lib()
    rng = np.random.default_rng(48)
    psfs = [tr.psf((9, 9), False, rng), tr.psf((9, 9), False, rng)]
    meas = rng.random((2, 2, 48, 40)) * 30.0 + 5.0
    twin = L.DeconvPlan(psfs, 2, 48, 40, dtype=dtype)
    twin.set_measurement(meas)
    twin.iterate(3)
    plan = L.DeconvPlan(psfs, 2, 48, 40, dtype=dtype)
    arr = plan.device_array('measurement').__cuda_array_interface__
    assert arr['shape'] == (2, 2, 48, 40)
    L.check(L.lib.rl_device_upload(plan.ctx.handle, ctypes.c_void_p(arr['data'][0]), L.DTYPES[dtype], meas.size, L.ptr(meas)))
    assert L.lib.rl_deconv_iterate(plan.handle, 3) == RL_ERR_STATE         # a fresh plan: written, but nobody said so
    assert b'no measurement' in L.lib.rl_last_error()
    plan.measurement_written()
    plan.iterate(3)
    assert plan.estimate().tobytes() == twin.estimate().tobytes()
    # again on the used plan: a new run from ones, not three more iterations
    plan.measurement_written()
    plan.iterate(3)
    assert plan.estimate().tobytes() == twin.estimate().tobytes()
    assert L.lib.rl_deconv_measurement_written(None) == RL_ERR_INVALID


# ---- end to end ------------------------------------------------------------------------------------------------------------------

_E2E = {}


def _e2e_case(name):
    """(measurement (2, V, 150, 131), psfs, the tiled oracle at tile 64, overlap 24, margin 4, K = 5), computed once per PSF set."""
    if name not in _E2E:
        from oracle import line_sted_oracle as orc
        rng = np.random.default_rng(len(name))
        psfs = {'separable': [tr.psf((5, 5), True, rng)], 'direct': [tr.psf((5, 5), False, rng)],
                'fft': [tr.psf((9, 9), False, rng), tr.psf((9, 9), False, rng)]}[name]
        meas = []
        for f in range(2):
            obj = rng.random((1, 150, 131)) + 0.5                       # uniform random plus an offset: nothing unresolved
            d = orc.Deconvolver(psfs)
            d.create_data_from_object(obj, total_brightness=100.0 * obj.size, random_seed=f)
            meas.append(np.stack([m[0] for m in d.noisy_measurement]))
        meas = np.stack(meas)
        _E2E[name] = (meas, psfs, tr.tiled_oracle(meas, psfs, 5, 64, 24, 4)[0])
    return _E2E[name]


@pytest.mark.parametrize('name', ['separable', 'direct', 'fft'])
def test_end_to_end_f64_matches_the_tiled_oracle(name):
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    meas, psfs, want = _e2e_case(name)
    est, info = deconvolve_tiled(meas, psfs, 5, tile=64, overlap=24, margin=4, dtype='f64', batch=5)
    st = info['strategy']
    assert {'separable': st['separable'], 'direct': st['direct_stencil'], 'fft': not st['separable'] and not st['direct_stencil']}[name], st
    assert info['tiles'] == 24 and info['chunks'] == 5 and info['unresolved'] == 0
    nw, pw = tr.normwise(est, want), tr.pixelwise(est, want)
    print('%s f64: normwise %.3e pixelwise %.3e' % (name, nw, pw))
    assert nw <= 1e-10 and pw <= 1e-8


def test_end_to_end_f32_matches_the_tiled_oracle():
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    meas, psfs, want = _e2e_case('fft')
    est, info = deconvolve_tiled(meas, psfs, 5, tile=64, overlap=24, margin=4, dtype='f32', batch=6)
    assert info['chunks'] == 4 and info['unresolved'] == 0
    nw = tr.normwise(est, want)
    print('fft f32: normwise %.3e' % nw)
    assert nw <= 1e-5


@pytest.mark.parametrize('case', tr.EXACT_CASES, ids=['5x5-rank1-K2', '5x5-full-K2', '4x4-K2', '9x9-K1'])
def test_exact_margin_gives_the_whole_image_estimate(case):
    from rescan_line_sted_amd.tiling import deconvolve_tiled, exact_margin
    meas, psfs, K, tile, overlap = tr.exact_case(case, 8)
    whole = tr.oracle_estimate(meas[0], psfs, K)
    est, info = deconvolve_tiled(meas, psfs, K, tile=tile, overlap=overlap, margin=exact_margin(psfs, K), dtype='f64')
    assert info['tiles'] == 4
    nw, pw = tr.normwise(est[0], whole), tr.pixelwise(est[0], whole)
    print('exact margin: normwise %.3e pixelwise %.3e' % (nw, pw))
    assert nw <= 1e-10 and pw <= 1e-8


def test_an_image_too_large_for_one_plan():
    from rescan_line_sted_amd.line_sted_tools import deconvolve, deconvolve_tiled
    L = _lib()
    rng = np.random.default_rng(4700)
    psfs = [tr.psf((9, 9), False, rng)]
    meas = rng.poisson(rng.random((1, 1, 4700, 96)) * 80.0 + 40.0) + 1e-9
    with pytest.raises(L.RlstedError, match='exceeds the largest built transform length'):
        deconvolve(meas, psfs, 2, dtype='f32')
    est, info = deconvolve_tiled(meas, psfs, 2, tile=(512, 96), dtype='f32')
    assert info['layout'].tile_shape == (512, 96) and info['tiles'] == len(info['layout'].origins_y) >= 10
    want, lay = tr.tiled_oracle(meas, psfs, 2, (512, 96), info['layout'].overlap, info['layout'].margin)
    assert np.array_equal(lay.origins_y, info['layout'].origins_y)
    nw = tr.normwise(est, want)
    print('4700 x 96 f32: normwise %.3e' % nw)
    assert est.shape == (1, 4700, 96) and nw <= 1e-5


def test_chunks_do_not_change_a_bit():
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    meas, psfs, _ = _e2e_case('fft')
    a, ia = deconvolve_tiled(meas[:1], psfs, 5, tile=64, overlap=24, margin=4, dtype='f64', batch=3)
    b, ib = deconvolve_tiled(meas[:1], psfs, 5, tile=64, overlap=24, margin=4, dtype='f64', batch=12)
    assert (ia['chunks'], ib['chunks']) == (4, 1)
    assert a.tobytes() == b.tobytes()


def test_stopping_rule_counts_are_those_of_the_stacked_tiles():
    from rescan_line_sted_amd.line_sted_tools import deconvolve_until
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    meas, psfs, _ = _e2e_case('fft')
    until = dict(rule='relative', threshold=0.02, check_every=2)
    est, info = deconvolve_tiled(meas[:1], psfs, 12, tile=64, overlap=24, margin=4, dtype='f64', batch=5, until=until)
    lay = info['layout']
    stacked = tr.gather(meas[:1], lay.slots(1), lay.tile_shape, np.float64)
    tiles, ref = deconvolve_until(stacked, psfs, 12, dtype='f64', **until)
    assert info['iterations'].shape == (1, 4, 3) and np.array_equal(info['iterations'].ravel(), ref['iterations'])
    assert len(set(ref['iterations'])) > 1 or ref['iterations'][0] < 12        # the rule did something
    want = tr.blend(tiles, tr.Layout(lay.shape, lay.tile, lay.overlap, lay.margin))
    assert est.tobytes() == want.tobytes()


def test_result_kept_on_the_device_feeds_ring_stats():
    from rescan_line_sted_amd import quality
    from rescan_line_sted_amd.tiling import deconvolve_tiled
    meas, psfs, _ = _e2e_case('direct')
    res, info = deconvolve_tiled(meas, psfs, 5, tile=64, overlap=24, margin=4, dtype='f64', batch=12, keep_on_device=True)
    host = res.download()
    got = quality.ring_stats_device(res.ctx, res.dev, res.dtype, res.offsets[:1], res.dev, res.dtype, res.offsets[1:], res.shape)
    want = quality.ring_stats(host[0], host[1])
    assert np.allclose(got[0], want, rtol=1e-12, atol=0)
    res.free()
