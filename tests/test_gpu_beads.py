"""The bead measurement on the MI355X (include/rlsted.h rl_find_peaks; rescan_line_sted_amd/beads.py): the peak finder against the
numpy twin (tests/beads_reference.py) bit for bit -- images of two whole tiles plus a partial tile on each axis plus 2 b with a
plateau across a tile seam, candidates at the border distance, cap overflow, non-contiguous offsets, f32 and f64 --, the same bits
across runs, alone and among other images and under a permuted order; measure_psfs against the twin of the whole method (the same
calls on the numpy device) on a noisy stack; the measured PSFs straight into deconvolve_stack.  Also the finder with its images
cut into chunks of one and of two (rl_find_peaks_chunk_bytes) and at the largest LDS a launch can ask for (h = r = 16: 64 KB)."""
import ctypes

import numpy as np
import pytest

import beads_reference as br

pytestmark = pytest.mark.gpu

SENTINEL = -7
I64P = ctypes.POINTER(ctypes.c_int64)
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture()
def dev():
    from rescan_line_sted_amd import beads
    d = beads._BeadDevice(device=0)
    yield d
    d.close()


def device_peaks(dev, buf, offsets, ny, nx, w, r, b, rel, threshold, cap):
    """rl_find_peaks straight through the library into sentinel-filled outputs; checks the sentinels past min(count, cap)."""
    from rescan_line_sted_amd._lib import check, lib
    n = len(offsets)
    off = np.asarray(offsets, dtype=np.int64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    yx = np.full((n, cap, 2), SENTINEL, dtype=np.int32)
    sv, xv = np.full((n, cap), float(SENTINEL)), np.full((n, cap), float(SENTINEL))
    cnt, lev = np.full(n, SENTINEL, dtype=np.int64), np.full((n, 3), float(SENTINEL))
    check(lib.rl_find_peaks(dev.ctx.handle, buf.ptr, 0 if buf.dtype == 'f32' else 1, off.ctypes.data_as(I64P), n, ny, nx, w.ctypes.data_as(DP),
                            (len(w) - 1) // 2, r, b, rel, threshold, cap, yx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), sv.ctypes.data_as(DP),
                            xv.ctypes.data_as(DP), cnt.ctypes.data_as(I64P), lev.ctypes.data_as(DP)))
    out = []
    for i in range(n):
        k = min(int(cnt[i]), cap)
        assert np.all(yx[i, k:] == SENTINEL) and np.all(sv[i, k:] == SENTINEL) and np.all(xv[i, k:] == SENTINEL), 'written past the count'
        out.append((yx[i, :k].astype(np.int64), sv[i, :k].copy(), xv[i, :k].copy(), int(cnt[i]), lev[i].copy()))
    return out


def assert_twin(got, img, w, r, b, rel, thr, cap):
    want = br.find_peaks(img, w, r, b, rel, thr)
    yx, s, x, count, lev = got
    k = min(want['count'], cap)
    assert count == want['count'] and lev.tobytes() == want['levels'].tobytes(), (count, want['count'], lev, want['levels'])
    assert np.array_equal(yx, want['yx'][:k]) and s.tobytes() == want['s'][:k].tobytes() and x.tobytes() == want['x'][:k].tobytes()


def _scenes():
    x, marks, b = br.seam_scene()
    y = np.nan_to_num(x, nan=1.0)
    z = 3.0 * y[::-1].copy() + 2.0
    return [x, y, z], marks, b


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_device_finder_is_the_twin_bit_for_bit(dev, dt):
    """Three images of the seam scene (a plateau inside a tile and across the seam, ties, candidates at distance b and b - 1 from the
    border, a nan) at non-contiguous offsets in a buffer with gaps, cap 64 and cap 3 (overflow), against the twin; then two calls of
    the same images, each image alone, and the images in a permuted order: the same bits."""
    imgs, marks, b = _scenes()
    w, _ = br.taps(0.6)
    ny, nx = imgs[0].shape
    npx = ny * nx
    gap = 29
    offsets = [2 * (npx + gap) + 5, 7, npx + gap + 3]
    host = np.full(3 * (npx + gap) + 16, 1e30, dtype=np.float32 if dt == 'f32' else np.float64)
    for img, o in zip(imgs, offsets):
        host[o:o + npx] = img.ravel()
    buf = dev.alloc(host.size, dt)
    dev.upload(buf, host)
    first = None
    for cap in (64, 3):
        got = device_peaks(dev, buf, offsets, ny, nx, w, 3, b, 0.2, 0.0, cap)
        for g, img in zip(got, imgs):
            assert_twin(g, img, w, 3, b, 0.2, 0.0, cap)
        assert cap > 3 or all(g[3] > 3 for g in got), 'the cap case must overflow'
        if cap == 64:
            first = got
            pos = [tuple(p) for p in got[0][0]]
            assert marks['plateau_seam'] in pos and marks['border_in'] in pos and marks['border_out'] not in pos
    again = device_peaks(dev, buf, offsets, ny, nx, w, 3, b, 0.2, 0.0, 64)
    perm = device_peaks(dev, buf, offsets[::-1], ny, nx, w, 3, b, 0.2, 0.0, 64)[::-1]
    for k in range(3):
        alone = device_peaks(dev, buf, [offsets[k]], ny, nx, w, 3, b, 0.2, 0.0, 64)[0]
        for other in (again[k], perm[k], alone):
            assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(first[k], other)), k


def test_device_finder_edge_cases(dev):
    """h = 0 (s is the input), a one-pixel domain, a flat image, s == t exactly; f64."""
    w, _ = br.taps(0.6)
    x, marks, b = br.seam_scene()
    cases = [(br.h0_scene(), np.array([1.0]), 1, 1, 0.5, 0.0, 200)]
    one = np.random.default_rng(1).integers(0, 9, size=(11, 11)).astype(np.float64)
    one[5, 5] = 30.0
    cases.append((one, w, 3, 5, 0.2, 0.0, 4))
    cases.append((np.full((br.TY + 13, br.TX + 11), 3.25), w, 3, 5, 0.2, 0.0, 8))
    cases.append((x, w, 3, b, 0.0, float(br.smooth(x, w)[marks['border_in']]), 64))
    for img, ww, r, bb, rel, thr, cap in cases:
        buf = dev.alloc(img.size, 'f64')
        dev.upload(buf, img)
        got = device_peaks(dev, buf, [0], img.shape[0], img.shape[1], ww, r, bb, rel, thr, cap)[0]
        assert_twin(got, img, ww, r, bb, rel, thr, cap)


def _round_up(v, a=256):
    return (v + a - 1) // a * a


def test_device_finder_in_chunks(dev):
    """Five images (the seam scene's three, two of them again) at non-contiguous offsets with the workspace cap lowered so that the
    call runs in chunks of one image (1 byte: five chunks) and of two (the share of two images, as bead_api.cpp counts it: chunks
    of 2, 2 and 1): the twin bit for bit, and the bits of the call with the default cap (one chunk)."""
    from rescan_line_sted_amd._lib import check, lib
    imgs, _, b = _scenes()
    imgs = imgs + [imgs[1], imgs[0]]
    w, _ = br.taps(0.6)
    ny, nx = imgs[0].shape
    npx, gap, cap = ny * nx, 17, 64
    offsets = [(k * 3 % 5) * (npx + gap) + k for k in range(5)]
    host = np.full(5 * (npx + gap) + 8, 1e30)
    for img, o in zip(imgs, offsets):
        host[o:o + npx] = img.ravel()
    buf = dev.alloc(host.size, 'f64')
    dev.upload(buf, host)
    whole = device_peaks(dev, buf, offsets, ny, nx, w, 3, b, 0.2, 0.0, cap)
    nty, ntx = -(-(ny - 2 * b) // br.TY), -(-(nx - 2 * b) // br.TX)
    per = _round_up(nty * ntx * 16) + _round_up((ny - 2 * b) * ntx * 4) + _round_up(cap * 8) + 2 * _round_up(cap * 8)
    for limit in (1, 2 * per):
        check(lib.rl_find_peaks_chunk_bytes(dev.ctx.handle, ctypes.c_size_t(limit)))
        got = device_peaks(dev, buf, offsets, ny, nx, w, 3, b, 0.2, 0.0, cap)
        for g, one, img in zip(got, whole, imgs):
            assert_twin(g, img, w, 3, b, 0.2, 0.0, cap)
            assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(g, one)), limit
    assert lib.rl_find_peaks_chunk_bytes(dev.ctx.handle, ctypes.c_size_t(0)) != 0


def test_device_finder_at_the_largest_lds(dev):
    """h = 16 (sigma 4), r = 16, b = 32, f64: k_peaks_mark asks for (80 + 48) 64 doubles = 65536 bytes of dynamic LDS, the most the
    launcher allows.  2 x 2 tiles, the last of each axis partial; small integers with isolated highs, one of them at the first pixel
    of the domain and one at its last; against the twin bit for bit."""
    w, h = br.taps(4.0)
    assert h == 16
    r, b = 16, 32
    ny, nx = 2 * b + br.TY + 5, 2 * b + br.TX + 7
    img = np.random.default_rng(4).integers(0, 4, size=(ny, nx)).astype(np.float64)
    for y, x, v in ((b, b, 900.0), (ny - 1 - b, nx - 1 - b, 800.0), (b + br.TY, b + br.TX - 1, 700.0), (b + 3, b + 30, 700.0)):
        img[y, x] = v
    buf = dev.alloc(img.size, 'f64')
    dev.upload(buf, img)
    got = device_peaks(dev, buf, [0], ny, nx, w, r, b, 0.2, 0.0, 16)[0]
    assert_twin(got, img, w, r, b, 0.2, 0.0, 16)
    assert got[3] >= 2 and (b, b) in [tuple(p) for p in got[0]]


def test_find_beads_on_the_device():
    from rescan_line_sted_amd import beads
    imgs, _, _ = _scenes()
    got, info = beads.find_beads(np.stack(imgs[1:]), sigma=0.6, radius=3, rel_threshold=0.2)
    w, h = br.taps(0.6)
    for k, img in enumerate(imgs[1:]):
        want = br.find_peaks(img, w, 3, h + 3, 0.2, 0.0)
        assert np.array_equal(got[k], want['yx']) and info['levels'][k].tobytes() == want['levels'].tobytes()


# ---- measure_psfs ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def noisy():
    """3 frames x 2 views of 160 x 192, uint16, Poisson, dark 100, gain 1; the twin of the whole method on it, computed once."""
    from rescan_line_sted_amd import beads
    from rescan_line_sted_amd.stack import CameraModel
    raw, truths = br.bead_stack(3, 160, 192, 21, True, seed=11, spacing=23, edge=24)
    cam = CameraModel(dark=100.0, gain=1.0)
    made = []

    class Logged(br.NumpyDevice):
        def __init__(self, device=0):
            br.NumpyDevice.__init__(self, device)
            made.append(self)
    keep = beads._Device
    beads._Device = Logged
    try:
        twin = beads.measure_psfs(raw, 21, camera=cam)
    finally:
        beads._Device = keep
    return raw, truths, cam, twin, made[0].fields


def test_measure_psfs_is_the_twin_of_the_method(noisy):
    """The same accepted beads (frames, positions to 1e-9 px, counts of every rejection reason) and PSFs within 1e-11 max of the
    twin; the twin's NCCs keep at least 1e-9 from min_ncc, so that a flip would be a bug and not rounding: the NCC of EVERY window
    that is neither flat nor at the limit in any pass (two estimates per view: the last one's values decide), accepted or not."""
    from rescan_line_sted_amd import beads
    raw, _, cam, (tpsfs, tinfo), fields = noisy
    psfs, info = beads.measure_psfs(raw, 21, camera=cam)
    assert len(fields) == 4
    for v in range(2):
        first, last = fields[2 * v], fields[2 * v + 1]
        live = (first[:, 1:] == 0.0).all(axis=1) & (last[:, 1:] == 0.0).all(axis=1)
        assert live.sum() == tinfo['n_beads'][v] + tinfo['rejected'][v]['ncc']
        assert np.all(np.abs(last[live, 0] - 0.9) >= 1e-9)
        assert info['n_beads'][v] == tinfo['n_beads'][v] >= 30 and info['rejected'][v] == tinfo['rejected'][v]
        assert np.array_equal(info['positions'][v][:, 0], tinfo['positions'][v][:, 0])
        assert np.abs(info['positions'][v] - tinfo['positions'][v]).max() <= 1e-9
        err = np.abs(psfs[v] - tpsfs[v]).max()
        print('view %d: %d beads, |P - P_twin| = %.3g of max' % (v, info['n_beads'][v], err / tpsfs[v].max()))
        assert err <= 1e-11 * tpsfs[v].max()


def test_measured_psfs_go_into_deconvolve_stack(noisy):
    """The measured PSFs as they come, straight into deconvolve_stack on the same stack: finite, positive estimates of the flux of the
    measurement (Richardson-Lucy keeps it)."""
    from rescan_line_sted_amd import beads
    from rescan_line_sted_amd.stack import deconvolve_stack
    raw, _, cam, _, _ = noisy
    psfs, _ = beads.measure_psfs(raw[:1], 21, camera=cam)
    est, info = deconvolve_stack(raw, psfs, 5, camera=cam, dtype='f64', out_dtype='f64')
    assert est.shape == (3, 160, 192) and np.all(np.isfinite(est)) and est.min() >= 0.0
    assert np.all(info['flux'] > 0.0)
