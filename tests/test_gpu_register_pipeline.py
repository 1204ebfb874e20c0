"""The peak search on the device and the overlapped registered pipeline on the MI355X (include/rlsted.h rl_register_peaks,
rl_register_estimate, rl_stack_run_registered; rescan_line_sted_amd/registration.py estimate_shifts(device_peaks=True),
deconvolve_stack_registered(pipeline=True)): the peaks against the host's ncc_surface + surface_peak bit for bit on constructed rows
(tests/peaks_reference.py); the device estimate against the host estimate byte for byte; the pipeline against the host loop of
deconvolve_stack_registered -- shifts, fields and estimates --, with given shifts and narrow export, with zero shifts against
deconvolve_stack, from page-locked arrays, and the plan afterwards."""
import ctypes

import numpy as np
import pytest

import ingest_reference as ir
import peaks_reference as pr
import register_reference as rr
from conftest import max_rel

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
GAIN, DARK, K = 0.125, 100.0, 3
CASES = [('f64', 1), ('f64', 2), ('f32', 2), ('f32', 1)]
INFO_KEYS = ('shifts', 'ncc', 'at_limit', 'flat', 'view_ncc', 'view_at_limit', 'view_flat', 'raised', 'level', 'clipped')


def _reg():
    from rescan_line_sted_amd import registration
    return registration


@pytest.fixture()
def dev():
    d = _reg()._Device(device=0)
    yield d
    d.close()


# ---- rl_register_peaks -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('R', [1, 8, 32])
def test_device_peaks_are_the_host_bit_for_bit(dev, R):
    """Every constructed row (ties across threads, within a thread and against the thread order; each border and corner; va <= 0,
    one vb <= 0, one vb nan; a plateau whose den rounds to 0) alone and 70 rows in one call, outputs inside sentinels: flags, integer
    peak, value and sub-pixel part, and the surface, the bits of the host.  This rests on float64 division and square root being
    correctly rounded in the device code."""
    from rescan_line_sted_amd._lib import lib, check
    rows = [r for seed in range(5) for r in pr.rows(R, seed).values()][:70]
    assert len(rows) == 70
    want = [pr.expected(r, R) for r in rows]
    nd = (2 * R + 1) ** 2
    tot = np.stack(rows)
    buf = dev.alloc(tot.size, 'f64')
    dev.upload(buf, tot)
    dp = ctypes.POINTER(ctypes.c_double)
    for n in (1, 70):
        pk, sf = np.full(n * 5 + 16, 7.0), np.full(n * nd + 16, 7.0)
        check(lib.rl_register_peaks(dev.ctx.handle, buf.ptr, n, R, pr.N_TERMS, pk[8:].ctypes.data_as(dp), sf[8:].ctypes.data_as(dp)))
        assert np.all(pk[:8] == 7.0) and np.all(pk[8 + n * 5:] == 7.0), 'written outside the fields'
        assert np.all(sf[:8] == 7.0) and np.all(sf[8 + n * nd:] == 7.0), 'written outside the surfaces'
        got, surf = pk[8:8 + n * 5].reshape(n, 5), sf[8:8 + n * nd].reshape(n, nd)
        for k in range(n):
            assert got[k].tobytes() == want[k][0].tobytes(), (k, got[k], want[k][0])
            assert surf[k].tobytes() == want[k][1].tobytes(), k
    fields = dev.peaks(buf, 70, R, pr.N_TERMS)
    assert fields.tobytes() == np.stack([w[0] for w in want]).tobytes()


# ---- estimate_shifts(device_peaks=True) ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('refine', [0, 1, 2])
def test_device_estimate_is_the_host_estimate(refine):
    """40 x 48 images of f32 and f64, R = 4, one flat image and one displaced by 6 px (at the limit): the shifts and every info
    array, surfaces included, byte for byte those of the default path."""
    reg = _reg()
    for dt in (np.float32, np.float64):
        imgs, ref = pr.estimate_images(dt)
        want, winfo = reg.estimate_shifts(imgs, ref, max_shift=4, refine=refine, surfaces=True)
        got, info = reg.estimate_shifts(imgs, ref, max_shift=4, refine=refine, surfaces=True, device_peaks=True)
        assert winfo['flat'][5] and winfo['at_limit'][4]
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (got, want)
        assert sorted(info) == sorted(winfo)
        for k in winfo:
            assert info[k].dtype == winfo[k].dtype and info[k].tobytes() == winfo[k].tobytes(), k


# ---- deconvolve_stack_registered(pipeline=True) ---------------------------------------------------------------------------------

def _stack(F, V, seed, sensor=(46, 61), roi=(3, 5, 40, 48)):
    """uint16 frames of a drifting blob scene inside a larger sensor frame, with noise (as tests/test_gpu_register.py)."""
    rng = np.random.default_rng(seed)
    y0, x0, ny, nx = roi
    p = rr.blobs(seed, ny, nx, 10)
    raw = rng.integers(95, 106, (F, V) + sensor).astype(np.uint16)
    for f in range(F):
        for v in range(V):
            img = rr.scene(p, (0.4 * f + 0.8 * v, -0.3 * f + 0.5 * v)) * 8.0 + 100.0
            raw[f, v, y0:y0 + ny, x0:x0 + nx] = rng.poisson(img).astype(np.uint16)
    return raw, roi


def _psfs(V):
    return [rr.gaussian_psf(0.8 + 0.5 * v, 1.9 - 0.5 * v, 7) for v in range(V)]


def _camera():
    from rescan_line_sted_amd.stack import CameraModel
    return CameraModel(dark=DARK, gain=GAIN)


def _ordered(raw, order):
    return raw if order == 'frame-view' else np.ascontiguousarray(raw.transpose(1, 0, 2, 3))


def _same_estimates(dtype, V, got, want, what):
    if (dtype, V) == ('f32', 1):
        err = max(max_rel(got[f], want[f]) for f in range(len(want)))
        print('%s f32 single view: bits equal %s, normwise %.3e' % (what, got.tobytes() == want.tobytes(), err))
        assert err <= 1e-5
    else:
        assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize('dtype,V', CASES)
def test_pipeline_is_the_host_loop(dtype, V):
    """F = 5, batch = 2 (three chunks, a short last one, both slots reused), a window of a u16 sensor, both orders, max_shift = 4:
    the shifts, the fields, the raised counts and the ingest statistics byte-equal to the host loop; the estimates byte-equal to
    the host loop run with the pipeline's shifts given."""
    reg = _reg()
    raw, roi = _stack(5, V, 50 + V)
    psfs = _psfs(V)
    for order in ('frame-view', 'view-frame'):
        r = _ordered(raw, order)
        kw = dict(camera=_camera(), order=order, roi=roi, dtype=dtype, batch=2, max_shift=4)
        want, winfo = reg.deconvolve_stack_registered(r, psfs, K, **kw)
        got, info = reg.deconvolve_stack_registered(r, psfs, K, pipeline=True, out_dtype='f64', **kw)
        assert got.dtype == np.float64 and got.shape == (5, 40, 48) and info['chunks'] == 3
        for k in INFO_KEYS:
            assert info[k].dtype == winfo[k].dtype and info[k].tobytes() == winfo[k].tobytes(), (order, k)
        assert set(winfo) | {'clamped', 'times_ms'} == set(info) and len(info['times_ms']) == 5
        if V > 1:
            assert info['view_ncc'][1] > 0.5
        given, _ = reg.deconvolve_stack_registered(r, psfs, K, camera=_camera(), order=order, roi=roi, dtype=dtype, batch=2,
                                                   shifts=info['shifts'])
        _same_estimates(dtype, V, got, given, order)
        _same_estimates(dtype, V, got, want, order + ' estimated')


@pytest.mark.parametrize('dtype,V', [('f64', 2), ('f32', 1)])
def test_pipeline_with_given_shifts_and_narrow_export(dtype, V):
    """Random shifts in +-3 px at order 3: the pipeline's estimates are those of the host loop with the same shifts; u16 export with
    a scale is the export twin of tests/ingest_reference.py applied to those estimates, the clamped counts equal."""
    reg = _reg()
    raw, roi = _stack(5, V, 60 + V)
    psfs = _psfs(V)
    shifts = np.random.default_rng(4).uniform(-3.0, 3.0, (5, V, 2))
    kw = dict(camera=_camera(), roi=roi, dtype=dtype, batch=2, shifts=shifts)
    want, winfo = reg.deconvolve_stack_registered(raw, psfs, K, **kw)
    got, info = reg.deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='f64', **kw)
    _same_estimates(dtype, V, got, want, 'given')
    assert np.array_equal(info['shifts'], shifts) and np.array_equal(info['raised'], winfo['raised']) and not info['ncc'].any()
    scale = 3000.0
    u16, uinfo = reg.deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='u16', out_scale=scale, **kw)
    twin, tstats = ir.export(got.astype(NP[dtype]), scale, np.uint16)
    print('clamped %d pixels' % tstats[:, 1].sum())
    assert u16.dtype == np.uint16 and u16.tobytes() == twin.tobytes()
    assert np.array_equal(uinfo['clamped'], tstats[:, 1].astype(np.int64)) and tstats[:, 1].sum() > 0


@pytest.mark.parametrize('dtype,V', CASES)
def test_zero_shifts_are_deconvolve_stack(dtype, V):
    """interp = 1 and register = (): the pipeline is deconvolve_stack, bit for bit outside the single-view f32 plans."""
    from rescan_line_sted_amd.stack import deconvolve_stack
    raw, roi = _stack(5, V, 20 + V)
    psfs = _psfs(V)
    want, winfo = deconvolve_stack(raw, psfs, K, camera=_camera(), roi=roi, dtype=dtype, out_dtype='f64', batch=2)
    got, info = _reg().deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype=dtype, batch=2, register=(), interp=1,
                                                   pipeline=True, out_dtype='f64')
    _same_estimates(dtype, V, got, want, 'zero shifts')
    assert not info['shifts'].any() and not info['raised'].any() and info['level'].tobytes() == winfo['level'].tobytes()
    assert np.array_equal(info['clamped'], winfo['clamped'])


def test_page_locked_arrays_give_the_bytes_of_pageable_ones():
    from rescan_line_sted_amd import _lib
    reg = _reg()
    raw, roi = _stack(5, 2, 71)
    psfs = _psfs(2)
    kw = dict(camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=4, pipeline=True, out_dtype='u16', out_scale=50.0)
    want, winfo = reg.deconvolve_stack_registered(raw, psfs, K, **kw)
    praw = _lib.pinned_empty(raw.shape, np.uint16)
    praw[:] = raw
    pout = _lib.pinned_empty((5, 40, 48), np.uint16)
    got, info = reg.deconvolve_stack_registered(praw, psfs, K, out=pout, **kw)
    assert got is pout and got.tobytes() == want.tobytes() and info['shifts'].tobytes() == winfo['shifts'].tobytes()


def test_the_plan_of_a_pipeline_run_stays_fresh(monkeypatch):
    """The plan of a pipeline run with estimation, used afterwards in the ordinary way, gives the bits of a fresh plan."""
    from rescan_line_sted_amd import _lib as L, stack
    kept = []

    class Keep(stack._Device):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            kept.append(self)
    monkeypatch.setattr(stack, '_Device', Keep)
    raw, roi = _stack(5, 2, 44)
    psfs = _psfs(2)
    est, info = _reg().deconvolve_stack_registered(raw, psfs, K, camera=_camera(), roi=roi, dtype='f32', batch=2, max_shift=4, pipeline=True)
    assert len(kept) == 1 and np.all(np.isfinite(est)) and info['unresolved'] == 0
    meas, _ = ir.measurement(raw, 2, 'frame-view', roi, DARK, GAIN)
    fresh = L.DeconvPlan(psfs, 2, 40, 48, dtype='f32')
    for q in (kept[0].plan, fresh):
        q.set_measurement(meas[3:5])
        q.iterate(K)
    assert kept[0].plan.estimate().tobytes() == fresh.estimate().tobytes()


def test_single_frame_or_view_estimates_nothing_missing():
    """F = 1: no frame pairs (frame 0 is the reference), V = 2 still estimates its view; V = 1 with register=('views',): no pair at
    all.  The missing estimates leave zero shifts and zero fields, and the results are those of the host loop."""
    reg = _reg()
    for F, V, register in ((1, 2, ('views', 'frames')), (1, 1, ('views', 'frames')), (5, 1, ('views',))):
        raw, roi = _stack(F, V, 80 + F + V)
        psfs = _psfs(V)
        kw = dict(camera=_camera(), roi=roi, dtype='f64', batch=2, max_shift=4, register=register)
        want, winfo = reg.deconvolve_stack_registered(raw, psfs, K, **kw)
        got, info = reg.deconvolve_stack_registered(raw, psfs, K, pipeline=True, out_dtype='f64', **kw)
        assert not info['ncc'].any() and not info['at_limit'].any() and not info['flat'].any()
        if V == 1:
            assert not info['shifts'].any() and not info['view_ncc'].any()
        else:
            assert info['view_ncc'][1] > 0.5 and np.all(info['shifts'][0, 0] == 0.0)
        for k in INFO_KEYS:
            assert info[k].tobytes() == winfo[k].tobytes(), (F, V, k)
        assert got.tobytes() == want.tobytes()
