"""Numpy twin of the ingest / export kernels (rescan_line_sted_amd/csrc/ingest_kernels.hpp; include/rlsted.h rl_ingest, rl_export):
the per-pixel arithmetic in float64 and the statistics' sums in the kernels' fixed order -- thread, binary tree over 256 threads,
workgroups in increasing order.  Test infrastructure: tests/test_stack_cpu.py holds the emulated bodies to it bit for bit,
tests/test_gpu_stack.py the device."""
import numpy as np

W, THREADS, VECS_PER_THREAD = 8, 256, 4
INGEST_FIELDS, EXPORT_FIELDS = 4, 2
RAW = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2, np.dtype(np.float32): 3}
OUT = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint16): 2}


def blocks(nvec):
    per = THREADS * VECS_PER_THREAD
    return min(max(-(-int(nvec) // per), 1), 0x10000)


def ordered_sum(vectors, nb=None):
    """vectors: (nvec, W) float64, dead lanes 0 (adding +0.0 changes no bit of a sum that started from +0.0).  The kernels' order:
    thread t of workgroup b adds vectors b * vpb + t, + 256, ... lane by lane; the tree; the workgroups in increasing order."""
    vectors = np.asarray(vectors, dtype=np.float64)
    nvec = len(vectors)
    nb = blocks(nvec) if nb is None else int(nb)
    vpb = -(-nvec // nb)
    total = np.float64(0.0)
    with np.errstate(all='ignore'):
        for b in range(nb):
            run = vectors[b * vpb:min((b + 1) * vpb, nvec)]
            rounds = -(-len(run) // THREADS) if len(run) else 0
            padded = np.zeros((max(rounds, 1) * THREADS, W))
            padded[:len(run)] = run
            padded = padded.reshape(-1, THREADS, W)
            s = np.zeros(THREADS)
            for m in range(padded.shape[0]):
                for e in range(W):
                    s = s + padded[m, :, e]
            h = THREADS // 2
            while h > 0:
                s[:h] = s[:h] + s[h:2 * h]
                h //= 2
            total = total + s[0]
    return float(total)


def _row_vectors(image):
    """(ny, nx) -> (ny * ceil(nx / W), W): every row cut into vectors, the last one padded with zeros."""
    ny, nx = image.shape
    cpr = -(-nx // W)
    padded = np.zeros((ny, cpr * W))
    padded[:, :nx] = image
    return padded.reshape(ny * cpr, W)


def _flat_vectors(image):
    flat = np.asarray(image, dtype=np.float64).ravel()
    padded = np.zeros(-(-flat.size // W) * W)
    padded[:flat.size] = flat
    return padded.reshape(-1, W)


def ingest_pixels(window, dark, offset, gain, epsilon, saturation, dst_dtype):
    """window (..., ny, nx) raw values -> (stored values of dst_dtype, clipped, saturated, invalid masks)."""
    with np.errstate(all='ignore'):
        x = window.astype(np.float64)
        d = np.float64(offset) if dark is None else np.asarray(dark, dtype=np.float32).astype(np.float64)
        v = (x - d) * np.float64(gain)
        saturated = (x >= saturation) if saturation > 0 else np.zeros(x.shape, dtype=bool)
        invalid = ~np.isfinite(v)
        clipped = ~invalid & (v < 0)
        v = np.where(invalid | clipped, 0.0, v)
        out = (v + np.float64(epsilon)).astype(dst_dtype)
    return out, clipped, saturated, invalid


def ingest(raw, n_slots, n_valid, V, ny, nx, y0=0, x0=0, frame_stride=None, view_stride=1, dark=None, offset=0.0, gain=1.0,
           epsilon=1e-9, saturation=0.0, dst_dtype=np.float64, nb=None):
    """raw (src_images, src_ny, src_pitch) -> dst (n_slots, V, ny, nx) of dst_dtype and stats (n_slots * V, 4) float64."""
    frame_stride = V if frame_stride is None else frame_stride
    dst = np.ones((n_slots, V, ny, nx), dtype=dst_dtype)
    stats = np.zeros((n_slots * V, INGEST_FIELDS))
    for b in range(n_slots):
        for v in range(V):
            if b < n_valid:
                window = raw[b * frame_stride + v * view_stride, y0:y0 + ny, x0:x0 + nx]
                out, clipped, saturated, invalid = ingest_pixels(window, dark, offset, gain, epsilon, saturation, dst_dtype)
                dst[b, v] = out
                stats[b * V + v, 1:] = clipped.sum(), saturated.sum(), invalid.sum()
            stats[b * V + v, 0] = ordered_sum(_row_vectors(dst[b, v].astype(np.float64)), nb)
    return dst, stats


def measurement(raw, V, order='frame-view', roi=None, dark=0.0, gain=1.0, saturation=None, epsilon=1e-9, dtype=np.float64):
    """A raw stack ((F, V, sy, sx) in 'frame-view' order, (V, F, sy, sx) in 'view-frame' order; (F, sy, sx) with V = 1) -> the
    measurement (F, V, ny, nx) the device forms from it, and its statistics (F, V, 4).  roi: (y0, x0, ny, nx)."""
    raw = np.asarray(raw)
    if raw.ndim == 3:
        raw = raw[:, None] if order == 'frame-view' else raw[None]
    F = raw.shape[0] if order == 'frame-view' else raw.shape[1]
    sy, sx = raw.shape[-2:]
    y0, x0, ny, nx = (0, 0, sy, sx) if roi is None else roi
    fs, vs = (V, 1) if order == 'frame-view' else (1, F)
    dark_map = None if np.isscalar(dark) else dark
    dst, stats = ingest(raw.reshape(-1, sy, sx), F, F, V, ny, nx, y0, x0, fs, vs, dark_map, 0.0 if dark_map is not None else dark, gain,
                        epsilon, 0.0 if saturation is None else saturation, dtype)
    return dst, stats.reshape(F, V, INGEST_FIELDS)


def export(est, scale=1.0, out_dtype=np.float32, nb=None):
    """est (n, ny, nx) f32 / f64 -> out (n, ny, nx) of out_dtype and stats (n, 2): the ordered sum of (double)e, the clamped count."""
    est = np.asarray(est)
    with np.errstate(all='ignore'):
        e = est.astype(np.float64)
        y = e * np.float64(scale)
        stats = np.zeros((len(est), EXPORT_FIELDS))
        if np.dtype(out_dtype) == np.uint16:
            over = y > 65535.0
            r = np.where(y > 0.0, np.where(over, 65535.0, np.rint(y)), 0.0)      # (nan > 0 is False; rint: ties to even)
            out = r.astype(np.uint16)
            stats[:, 1] = over.reshape(len(est), -1).sum(axis=1)
        else:
            out = y.astype(out_dtype)
    for i in range(len(est)):
        stats[i, 0] = ordered_sum(_flat_vectors(e[i]), nb)
    return out, stats
