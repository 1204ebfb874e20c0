"""Tiled Richardson-Lucy without a GPU (include/rlsted.h rl_tile_*; rescan_line_sted_amd/tiling.py): the layout rule and the
weights (csrc/tile_layout.hpp through the emulator and through the library) against the numpy twin (tests/tile_reference.py) bit
for bit; the bodies of k_tile_gather and k_tile_blend emulated thread by thread (tests/emu/tile_emu.cpp) against numpy; the same
code as stand-alone programs under the address and undefined-behaviour sanitizers; the exactness condition on the oracle; and the
wrapper's chunking on a numpy stand-in for the device.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tile_reference as tr
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, 'tests', 'emu')
SRC = os.path.join(EMU_DIR, 'tile_emu.cpp')
CSRC = os.path.join(ROOT, 'rescan_line_sted_amd', 'csrc')
DEPS = [os.path.join(CSRC, f) for f in ('tile_kernels.hpp', 'tile_layout.hpp', 'accel_kernels.hpp', 'fft_core.hpp')]
DT = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
T = 64
I32P = ctypes.POINTER(ctypes.c_int32)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def emu():
    so = os.path.join(EMU_DIR, 'libtile_emu.so')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in [SRC] + DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-Wno-unknown-pragmas', SRC, '-o', so])
    lib = ctypes.CDLL(so)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_tile_count.argtypes = [i, i, i]
    lib.emu_tile_origins.argtypes = [i, i, i, vp]
    lib.emu_tile_weights.argtypes = [i, i, i, i, vp, vp, vp, vp]
    lib.emu_tile_gather.argtypes = [vp, i, i, i, i, vp, i, i, i, vp, i]
    lib.emu_tile_gather.restype = None
    lib.emu_tile_blend.argtypes = [vp, i, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, i]
    return lib


def _emu_axis(emu, n, tile, overlap, margin):
    count = emu.emu_tile_count(n, tile, overlap)
    assert count >= 1
    origins = np.zeros(count, dtype=np.int32)
    emu.emu_tile_origins(n, tile, count, _p(origins))
    t = min(n, tile)
    w = np.full((count, t), np.nan)
    first, cover = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    assert emu.emu_tile_weights(n, tile, margin, count, _p(origins), _p(w), _p(first), _p(cover)) == 0
    return origins, w, first, cover


def _lib_axis(n, tile, overlap, margin):
    from rescan_line_sted_amd import _lib
    count = ctypes.c_int()
    _lib.check(_lib.lib.rl_tile_axis(n, tile, overlap, ctypes.byref(count), None))
    origins = np.zeros(count.value, dtype=np.intc)
    _lib.check(_lib.lib.rl_tile_axis(n, tile, overlap, ctypes.byref(count), origins.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    w = np.full((count.value, min(n, tile)), np.nan)
    first, cover = np.zeros(n, dtype=np.intc), np.zeros(n, dtype=np.intc)
    ip = ctypes.POINTER(ctypes.c_int)
    _lib.check(_lib.lib.rl_tile_weights(n, tile, overlap, margin, count.value, origins.ctypes.data_as(ip), _lib.ptr(w),
                                        first.ctypes.data_as(ip), cover.ctypes.data_as(ip)))
    return origins, w, first, cover


# ---- layout ----------------------------------------------------------------------------------------------------------------------

def test_the_issue_example_origins(emu):
    """150 x 131, tile 64, overlap 24: the library, the Python layout, the emulated header and the twin."""
    from rescan_line_sted_amd.tiling import TileLayout
    lay = TileLayout((150, 131), 64, 24, 8)
    assert list(lay.origins_y) == [0, 28, 57, 86] and list(lay.origins_x) == [0, 33, 67] and lay.tile_shape == (64, 64)
    assert list(_lib_axis(150, 64, 24, 8)[0]) == [0, 28, 57, 86] and list(_emu_axis(emu, 131, 64, 24, 8)[0]) == [0, 33, 67]
    assert list(tr.axis_origins(150, 64, 24)[0]) == [0, 28, 57, 86]
    assert list(tr.axis_origins(131, 64, 24)[0]) == [0, 33, 67]


@pytest.mark.parametrize('margin', [0, 8])
@pytest.mark.parametrize('overlap', [17, 24, 32])
def test_layout_rule_and_weights(emu, overlap, margin):
    """First origin 0, last N - t, every consecutive overlap >= o, positive weight sums, normalised weights summing to 1 within 4
    ulp, a zero margin band at interior edges -- and the C++ tables (emulator and library) equal to the numpy twin bit for bit."""
    s = T - overlap
    three = 0
    for n in (T - 1, T, T + 1, 2 * T - overlap, 2 * T - overlap + 1, T + s + 1, 150, 131):
        origins, t = tr.axis_origins(n, T, overlap)
        assert t == min(n, T) and origins[0] == 0 and origins[-1] == n - t
        assert np.all(np.diff(origins) > 0) and np.all(origins[:-1] + t - origins[1:] >= overlap)
        assert len(origins) == (1 if n <= T else -(-(n - T) // s) + 1)
        w, first, cover = tr.axis_weights(n, t, margin, origins)
        raw = tr.raw_weights(t, margin, origins)
        total = np.zeros(n)
        wsum = np.zeros(n)
        for i, a in enumerate(origins):
            total[a:a + t] += raw[i]
            wsum[a:a + t] += w[i]
            assert np.all(first[a:a + t] <= i) and np.all(i < first[a:a + t] + cover[a:a + t])
            if i > 0:
                assert np.all(w[i][:margin] == 0.0)
            if i < len(origins) - 1:
                assert np.all(w[i][t - margin:] == 0.0)
        assert np.all(total > 0.0)
        assert np.all(np.abs(wsum - 1.0) <= 4 * np.finfo(np.float64).eps), (n, np.abs(wsum - 1.0).max())
        three += int(np.sum(cover >= 3))
        for got in (_emu_axis(emu, n, T, overlap, margin), _lib_axis(n, T, overlap, margin)):
            assert np.array_equal(got[0], origins)
            assert got[1].tobytes() == w.tobytes(), (n, overlap, margin)
            assert np.array_equal(got[2], first) and np.array_equal(got[3], cover)
    assert three > 0                                  # N = t + s + 1: a stretch under three tiles


@pytest.mark.parametrize('tile,overlap,margin', [(64, 64, 0), (64, 0, 0), (64, 70, 0), (0, 8, 0), (64, 24, 12), (64, 24, -1), (64, 17, 9)])
def test_invalid_parameters_are_rejected(emu, tile, overlap, margin):
    from rescan_line_sted_amd import _lib
    from rescan_line_sted_amd.tiling import TileLayout
    with pytest.raises(ValueError):
        tr.Layout((150, 131), tile, overlap, margin)
    with pytest.raises(ValueError):
        TileLayout((150, 131), tile, overlap, margin)
    count = ctypes.c_int(-5)
    origins = np.array([0, 43, 86], dtype=np.intc)
    ip = ctypes.POINTER(ctypes.c_int)
    rc_axis = _lib.lib.rl_tile_axis(150, tile, overlap, ctypes.byref(count), None)
    rc_w = _lib.lib.rl_tile_weights(150, tile, overlap, margin, 3, origins.ctypes.data_as(ip), None, None, None)
    assert rc_w == -1 and b'' != _lib.lib.rl_last_error()
    if not 0 < overlap < tile:
        assert rc_axis == -1 and count.value == -5 and emu.emu_tile_count(150, tile, overlap) < 0


def test_the_library_rejects_origins_that_do_not_span_the_axis():
    from rescan_line_sted_amd import _lib
    ip = ctypes.POINTER(ctypes.c_int)
    w = np.zeros((3, 64))
    for origins in ([0, 40, 80], [1, 43, 86], [0, 86, 43], [0, 10, 86]):       # short, late, decreasing, a gap
        o = np.array(origins, dtype=np.intc)
        assert _lib.lib.rl_tile_weights(150, 64, 24, 8, 3, o.ctypes.data_as(ip), _lib.ptr(w), None, None) == -1, origins


def test_the_python_layout_is_the_reference_layout():
    from rescan_line_sted_amd.tiling import TileLayout
    for shape, tile, overlap, margin in (((150, 131), 64, 24, 8), ((64, 128), 64, 24, 0), ((40, 300), (64, 96), (24, 40), 4)):
        a, b = TileLayout(shape, tile, overlap, margin), tr.Layout(shape, tile, overlap, margin)
        assert a.tile_shape == b.tile_shape and a.tiles_per_frame == b.tiles_per_frame
        assert np.array_equal(a.origins_y, b.origins_y) and np.array_equal(a.origins_x, b.origins_x)
        assert a.weights_y.tobytes() == b.weights_y.tobytes() and a.weights_x.tobytes() == b.weights_x.tobytes()
        assert np.array_equal(a.slots(2), b.slots(2)) and a.slots(2).dtype == np.int32
    s = TileLayout((150, 131), 64, 24, 8).slots(2)
    assert s.shape == (24, 3) and list(s[0]) == [0, 0, 0] and list(s[1]) == [0, 0, 33] and list(s[3]) == [0, 28, 0] and list(s[12]) == [1, 0, 0]


# ---- kernels ---------------------------------------------------------------------------------------------------------------------

def _offset_buffer(n, dtype, shift, fill=None):
    """n values of `dtype` starting `shift` elements into a 64-byte aligned allocation (shift 0: the 16-byte paths; odd: the element
    paths), and the guard values around them."""
    raw = np.zeros(n + 32 + shift, dtype=dtype)
    start = (-raw.ctypes.data // raw.itemsize) % (64 // raw.itemsize)
    whole = raw[start:start + shift + n + 8]
    whole[:] = -7.0
    view = whole[shift:shift + n]
    assert view.ctypes.data % 64 == shift * raw.itemsize
    if fill is not None:
        view[:] = fill
    return whole, view


@pytest.mark.parametrize('dst_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('src_dtype', [np.float32, np.float64])
def test_emulated_gather_is_numpy_slicing(emu, src_dtype, dst_dtype):
    """All four dtype pairs, tiles 16 x 24 (16-byte stores) and 16 x 21 (element stores), destination aligned and at an odd element
    offset, unaligned window origins, fillers first, in the middle and last; nothing is written around the destination."""
    rng = np.random.default_rng(5)
    F, V, NY, NX = 2, 2, 37, 53
    src = (rng.random((F, V, NY, NX)) + 0.25).astype(src_dtype)
    for ty, tx in ((16, 24), (16, 21)):
        slots = np.array([(-1, 0, 0), (0, 0, 0), (1, NY - ty, NX - tx), (-1, 5, 5), (1, 5, 7), (0, 21, 3), (0, 7, 29), (-1, 0, 0)], dtype=np.int32)
        want = tr.gather(src, slots, (ty, tx), dst_dtype)
        for shift in (0, 1):
            whole, dst = _offset_buffer(want.size, dst_dtype, shift)
            emu.emu_tile_gather(_p(src), DT[src.dtype], V, NY, NX, _p(slots), len(slots), ty, tx, _p(dst), DT[dst.dtype])
            assert dst.tobytes() == want.tobytes(), (ty, tx, shift)
            assert np.all(whole[:shift] == -7.0) and np.all(whole[shift + want.size:] == -7.0)
        assert np.all(want[0] == 1) and np.all(want[3] == 1) and np.all(want[-1] == 1)


BLEND_CASES = [((150, 131), 64, 24, 8), ((64, 128), 64, 24, 0), ((105, 128), 64, 24, 8), ((70, 131), 64, 32, 8)]


@pytest.mark.parametrize('out_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('store_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', BLEND_CASES, ids=lambda c: '%dx%d' % c[0])
def test_emulated_blend_is_the_numpy_twin(emu, case, store_dtype, out_dtype):
    """f32 and f64 stores, f32 and f64 outputs, NX = 128 (16-byte stores) and 131 (element stores), the output aligned and at an odd
    element offset (element stores whatever NX), one, two and -- 105 rows -- three tiles over a pixel: bit for bit the twin."""
    shape, tile, overlap, margin = case
    lay = tr.Layout(shape, tile, overlap, margin)
    rng = np.random.default_rng(shape[0])
    F, nyt, nxt = 2, len(lay.origins_y), len(lay.origins_x)
    tiles = (rng.random((F, nyt, nxt) + lay.tile_shape) + 0.25).astype(store_dtype)
    want = tr.blend(tiles, lay, out_dtype)
    covers = set(int(a) * int(b) for a in lay.cover_y for b in lay.cover_x)
    assert {1, 2} <= covers or shape == (64, 128)
    if shape[0] == 105:
        assert lay.cover_y.max() == 3
    oy, ox = lay.origins_y.astype(np.int32), lay.origins_x.astype(np.int32)
    W = 16 // np.dtype(out_dtype).itemsize
    for shift in (0, 1):
        whole, out = _offset_buffer(want.size, out_dtype, shift)
        vec = emu.emu_tile_blend(_p(tiles), DT[tiles.dtype], F, shape[0], shape[1], nyt, nxt, lay.tile_shape[0], lay.tile_shape[1], _p(oy), _p(ox),
                                 _p(lay.weights_y), _p(lay.weights_x), _p(out), DT[out.dtype])
        assert vec == (1 if shift == 0 and shape[1] % W == 0 else 0)
        assert out.tobytes() == want.tobytes(), (shape, shift)
        assert np.all(whole[:shift] == -7.0) and np.all(whole[shift + want.size:] == -7.0)
    # the weights sum to one: a constant store blends to the constant
    flat = tr.blend(np.full_like(tiles, 3.0), lay, np.float64)
    assert np.abs(flat - 3.0).max() <= 3.0 * 4 * np.finfo(np.float64).eps


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('source,define,expect', [('tile_emu.cpp', '-DTILE_EMU_MAIN', 'ok 16 40'), ('tile_layout_test.cpp', None, 'ok 72 8')])
def test_stand_alone_programs_under_the_sanitizers(tmp_path, source, define, expect):
    """The emulation and the layout code as programs of their own under -fsanitize=address,undefined, run directly."""
    exe = str(tmp_path / source.replace('.cpp', '_san'))
    cmd = ['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=all', os.path.join(EMU_DIR, source), '-o', exe]
    if define:
        cmd.insert(1, define)
    subprocess.check_call(cmd)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == expect, r.stdout


# ---- exactness on the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', tr.EXACT_CASES, ids=['5x5-rank1-K2', '5x5-full-K2', '4x4-K2', '9x9-K1'])
def test_tiled_oracle_is_whole_image_oracle_at_the_exact_margin(case):
    from rescan_line_sted_amd.tiling import exact_margin
    meas, psfs, K, tile, overlap = tr.exact_case(case, 8)
    assert exact_margin(psfs, K) == 8
    whole = tr.oracle_estimate(meas[0], psfs, K)
    tiled, lay = tr.tiled_oracle(meas, psfs, K, tile, overlap, 8)
    assert lay.tiles_per_frame >= 4
    err = tr.normwise(tiled[0], whole)
    print('normwise deviation at the exact margin: %.3e' % err)
    assert err <= 1e-12


def test_one_pixel_less_than_the_exact_margin_is_not_exact():
    """5 x 5 full PSF, K = 2: at margin 7 the blend uses pixels the tile border has reached."""
    from rescan_line_sted_amd.tiling import exact_margin
    meas, psfs, K, tile, _ = tr.exact_case(tr.EXACT_CASES[1], 8)
    assert exact_margin(psfs, K) - 1 == 7
    whole = tr.oracle_estimate(meas[0], psfs, K)
    tiled, _ = tr.tiled_oracle(meas, psfs, K, tile, 20, 7)     # (the overlap of the exact case: only the margin moves)
    err = tr.normwise(tiled[0], whole)
    print('normwise deviation one pixel short: %.3e' % err)
    assert err > 1e-8


# ---- wrapper logic ---------------------------------------------------------------------------------------------------------------

class _NumpyDevice:
    """Stands in for tiling._Device: the same steps in numpy, the oracle as the plan; records what the wrapper asked for."""
    log = None

    def __init__(self, psfs, batch, tile_shape, dtype, device, acceleration, tv_lambda, tv_epsilon):
        self.psfs, self.batch, self.tile_shape = psfs, batch, tuple(tile_shape)
        self.handles = {}
        type(self).log = self.calls = []

    def alloc(self, elements):
        h = ctypes.c_void_p(len(self.handles) + 1)
        self.handles[h.value] = np.full(int(elements), np.nan)
        return h

    def upload(self, measurement):
        self.src = measurement.copy()
        self.calls.append(('upload', measurement.shape))

    def gather(self, slots):
        assert slots.shape == (self.batch, 3) and slots.dtype == np.int32
        self.calls.append(('gather', slots.copy()))
        self.meas = tr.gather(self.src, slots, self.tile_shape, np.float64)

    def iterate(self, iterations, until):
        self.calls.append(('iterate', iterations, until))
        self.est = np.stack([tr.oracle_estimate(m, self.psfs, iterations) for m in self.meas])
        return None if until is None else np.arange(self.batch) + 1

    def store(self, store, first, count):
        self.calls.append(('store', first, count))
        n = self.tile_shape[0] * self.tile_shape[1]
        self.handles[store.value][first * n:(first + count) * n] = self.est[:count].ravel()

    def blend(self, store, layout, frames, out):
        self.calls.append(('blend', frames))
        lay = tr.Layout(layout.shape, layout.tile, layout.overlap, layout.margin)
        self.handles[out.value][:] = tr.blend(self.handles[store.value], lay).ravel()

    def result(self, out, frames, shape):
        data = self.handles[out.value].reshape((frames,) + tuple(shape))

        class R:
            def download(self):
                return data

            def free(self):
                pass
        return R()

    def unresolved(self):
        return 0

    def strategy(self):
        return {}

    def close(self):
        self.calls.append(('close',))


def test_wrapper_chunks_slots_and_fillers(monkeypatch):
    from rescan_line_sted_amd import tiling
    monkeypatch.setattr(tiling, '_Device', _NumpyDevice)
    rng = np.random.default_rng(3)
    psfs = [tr.psf((5, 5), False, rng)]
    meas = rng.random((2, 1, 70, 50)) * 20.0 + 5.0
    est, info = tiling.deconvolve_tiled(meas, psfs, 2, tile=(40, 32), overlap=12, margin=2, batch=5)
    lay = info['layout']
    assert lay.tile_shape == (40, 32) and (len(lay.origins_y), len(lay.origins_x)) == (3, 2)
    assert info['tiles'] == 12 and info['batch'] == 5 and info['chunks'] == 3 and info['unresolved'] == 0
    calls = _NumpyDevice.log
    assert [c[0] for c in calls] == ['upload'] + ['gather', 'iterate', 'store'] * 3 + ['blend', 'close']
    slots = lay.slots(2)
    gathers = [c[1] for c in calls if c[0] == 'gather']
    assert np.array_equal(gathers[0], slots[:5]) and np.array_equal(gathers[1], slots[5:10])
    assert np.array_equal(gathers[2][:2], slots[10:]) and np.all(gathers[2][2:, 0] == -1)      # the short last chunk: fillers
    assert [c[1:] for c in calls if c[0] == 'store'] == [(0, 5), (5, 5), (10, 2)]
    assert all(c[1:] == (2, None) for c in calls if c[0] == 'iterate')
    want, _ = tr.tiled_oracle(meas, psfs, 2, (40, 32), 12, 2)
    assert est.shape == (2, 70, 50) and np.array_equal(est, want)
    # (V, NY, NX) is one frame; the per-tile iteration counts of a stopping rule come back in tile order, fillers dropped
    est1, info1 = tiling.deconvolve_tiled(meas[0], psfs, 2, tile=(40, 32), overlap=12, margin=2, batch=4, until=dict(rule='relative', threshold=0.5))
    assert est1.shape == (1, 70, 50) and np.array_equal(est1[0], want[0])
    assert info1['iterations'].shape == (1, 3, 2) and list(info1['iterations'].ravel()) == [1, 2, 3, 4, 1, 2]
    assert [c[2] for c in _NumpyDevice.log if c[0] == 'iterate'] == [{'rule': 'relative', 'threshold': 0.5}] * 2


def test_wrapper_defaults_and_argument_errors(monkeypatch):
    from rescan_line_sted_amd import tiling
    from rescan_line_sted_amd import line_sted_tools
    assert line_sted_tools.deconvolve_tiled is tiling.deconvolve_tiled
    monkeypatch.setattr(tiling, '_Device', _NumpyDevice)
    big = [np.ones((1, 107, 107))]
    assert tiling.default_tile(big) == 512 and tiling.default_tile([np.ones((1, 129, 9))]) == 512
    assert tiling.default_tile([np.ones((1, 131, 131))]) == 1152 - 65            # 512 + 65 > 576: the next length, less hw
    assert tiling.exact_margin(big, 20) == 2 * 20 * 53 and tiling.exact_margin([np.ones((1, 4, 4))], 2) == 8
    assert tiling.DEFAULT_MARGIN % 8 == 0 and tiling.default_overlap(tiling.DEFAULT_MARGIN) == 2 * tiling.DEFAULT_MARGIN + 16
    psfs = [np.full((1, 3, 3), 1 / 9.0)]
    meas = np.ones((1, 1, 20, 20))
    for kwargs in (dict(tile=16, overlap=16), dict(tile=16, overlap=8, margin=4), dict(tile=16, overlap=8, margin=-1), dict(batch=0),
                   dict(dtype='f16'), dict(until=dict(rule='relative', limit=3)), dict(acceleration='nesterov'), dict(tv_lambda=0.5)):
        with pytest.raises(ValueError):
            tiling.deconvolve_tiled(meas, psfs, 1, **{**dict(tile=16, overlap=8, margin=1), **kwargs})
    for bad in (np.ones((20, 20)), np.ones((1, 2, 20, 20)), np.ones((1, 1, 0, 20))):
        with pytest.raises(ValueError):
            tiling.deconvolve_tiled(bad, psfs, 1, tile=16, overlap=8, margin=1)
    with pytest.raises(ValueError):
        tiling.deconvolve_tiled(meas, psfs, -1, tile=16, overlap=8, margin=1)
    # an image no larger than the tile is one tile of the image's shape, whatever the defaults
    est, info = tiling.deconvolve_tiled(meas, psfs, 1)
    assert info['tiles'] == 1 and info['layout'].tile_shape == (20, 20) and est.shape == (1, 20, 20)
