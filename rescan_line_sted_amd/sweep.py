"""Parameter sweeps over independent simulations (BASELINE config 4: "all test
objects x doses x scan modes x seeds"), the workload of the reference's figure-2
script (line_sted_figure_2.py:29-57: one Deconvolver per PSF set and test image,
create_data_from_object + N x iterate), batched and -- optionally -- sharded over
GPUs.

A task is (object name, PSF-set name, seed).  All tasks that share a PSF set and an image
shape -- a GROUP -- become the frames of one device plan, whatever their seeds: a frame draws its
noise with the Philox key (task seed, object id) -- `rl_deconv_simulate_keyed` -- where the object
id is the position of the object's name in the sorted object names, so a task's result does not
depend on how the sweep was batched or sharded.

How a sweep runs on one rank (round 4; `run_tasks_device`): plans are built once per (PSF set, image
shape, batch, dtype, device) and kept (`plan_for`); every group is ENQUEUED with `rl_batch_submit` --
objects staged in page-locked memory, uploaded on a copy stream, simulated and deconvolved on the
device, the estimates written straight into one device buffer of the rank (`DeviceResults`: fp32 or
fp64, unpadded, task order) -- on one of a few contexts of the GPU in turn, so that the small launches
of neighbouring groups overlap; the host synchronises once, at the end.  Across ranks: whole groups
are dealt to the ranks (`sharding.partition_groups`: a plan's set-up is then paid by one rank), and
ONE `rl_comm_gather_device` brings the device buffers to the root, which downloads once.
"""
import ctypes
import hashlib

import numpy as np

from . import quality, sharding
from ._lib import DTYPES, RL_F32, RNG_PHILOX, Context, DeconvPlan, accel_mode, check, lib, ptr, tv_params


def make_tasks(objects, psf_sets, seeds):
    """All (object, psf set, seed) combinations, in a deterministic order."""
    return [(o, p, int(s)) for p in sorted(psf_sets) for s in seeds for o in sorted(objects)]


def task_costs(tasks, objects, psf_sets, iterations):
    return [sharding.task_cost(objects[o].shape[-2] * objects[o].shape[-1], len(psf_sets[p]), iterations)
            for o, p, _ in tasks]


def task_groups(tasks, objects):
    """The plan a task runs in: (PSF set, image shape)."""
    return [(p, tuple(objects[o].shape[-2:])) for o, p, _ in tasks]


def object_ids(objects):
    """Stable image ids for the Philox counter: the rank of each object name."""
    return {name: i for i, name in enumerate(sorted(objects))}


# ------------------------------------------------------------------ plans are built once and kept
PLAN_CACHE_MAX = 128
_plans = {}


_set_keys = {}      # id(list of PSF arrays) -> (the list, its arrays, per-array (sum, sum of squares), (digest, views))


def _psf_set_key(psfs):
    """(sha1 of the PSF set, its views as (1, py, px) float64 arrays).  Hashing 18 sets of up to ten 107 x 107 float64 PSFs is milliseconds per sweep -- as much
    as the device needs for a quarter of it -- so a set that is the SAME list of the SAME arrays as last time, with unchanged sums and
    sums of squares (an in-place edit shows there), is not hashed again."""
    ent = _set_keys.get(id(psfs))
    probe = tuple((float(np.sum(p)), float(np.square(p).sum())) for p in psfs)     # (no BLAS call: its thread pool costs more than the sums)
    if ent is not None and ent[0] is psfs and len(ent[1]) == len(psfs) and all(a is b for a, b in zip(ent[1], psfs)) and ent[2] == probe:
        return ent[3]
    # (the views of a set may differ in shape -- DeconvPlan embeds them in a common one -- so the key covers shapes and values)
    views = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape((1,) + np.shape(p)[-2:])) for p in psfs]
    h = hashlib.sha1()
    for v in views:
        h.update(repr(v.shape).encode())
        h.update(v.tobytes())
    val = (h.hexdigest(), views)
    if len(_set_keys) > 4 * PLAN_CACHE_MAX:
        _set_keys.clear()
    _set_keys[id(psfs)] = (psfs, list(psfs), probe, val)
    return val


def plan_for(psfs, batch, shape, dtype='f32', device=0, stream=0, acceleration=None, tv_lambda=None, tv_epsilon=0.1):
    """The plan of a (PSF set, image shape, batch): built on first use, kept for the next sweep (the reference builds its
    Deconvolvers once per figure too, line_sted_figure_2.py:39-45).  `stream`: which of the device's contexts it lives on;
    `acceleration`: None or 'biggs-andrews' (DeconvPlan) -- part of the key, a plain and an accelerated sweep keep plans of their own;
    `tv_lambda`, `tv_epsilon`: the total-variation regulariser (DeconvPlan.set_tv; None: off) -- part of the key as well."""
    digest, views = _psf_set_key(psfs)
    tv = tv_params(tv_lambda, tv_epsilon)
    key = (digest, len(views), int(batch), tuple(shape), dtype, device, stream, accel_mode(acceleration), tv if tv[0] else None)
    plan = _plans.pop(key, None)
    if plan is None:
        plan = DeconvPlan(views, batch, shape[0], shape[1], dtype=dtype, device=device, stream=stream, acceleration=acceleration,
                          tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
        while len(_plans) >= PLAN_CACHE_MAX:
            _plans.pop(next(iter(_plans)))          # the least recently used one
    _plans[key] = plan
    return plan


def clear_plans():
    _plans.clear()
    _set_keys.clear()


def unresolved_total(reset=False):
    """Predictions H(est) <= 0 the kept plans met in their sweeps so far (DeconvPlan.unresolved, include/rlsted.h
    rl_deconv_unresolved): 0 on data the plans' arithmetic resolves.  Synchronises the plans' contexts."""
    return sum(plan.unresolved(reset=reset) for plan in _plans.values())


class DeviceResults:
    """The estimates of a list of tasks in ONE device buffer (rl_device_alloc): image i at element offsets[i], shape shapes[i],
    arithmetic type `dtype` -- unpadded, in task order.  What rl_batch_submit writes and rl_comm_gather_device sends."""

    def __init__(self, shapes, dtype='f32', device=0):
        self.ctx = Context.get(device)
        self.shapes = [tuple(s) for s in shapes]
        self.dtype = dtype
        sizes = [s[0] * s[1] for s in self.shapes]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n = int(self.offsets[-1])
        self.itemsize = 4 if DTYPES[dtype] == RL_F32 else 8
        self.dev = ctypes.c_void_p()
        check(lib.rl_device_alloc(self.ctx.handle, max(self.n, 1) * self.itemsize, ctypes.byref(self.dev)))

    def address(self, i):
        return ctypes.c_void_p(self.dev.value + int(self.offsets[i]) * self.itemsize)

    def download(self):
        """ONE device-to-host transfer; the list of (ny, nx) float64 estimates."""
        flat = np.empty(self.n, dtype=np.float64)
        check(lib.rl_device_download(self.ctx.handle, self.dev, DTYPES[self.dtype], self.n, ptr(flat)))
        return [flat[int(o):int(o) + sh[0] * sh[1]].reshape(sh) for o, sh in zip(self.offsets, self.shapes)]

    @classmethod
    def with_layout(cls, shapes, order, dtype='f64', device=0):
        """A buffer whose images lie in memory in the order `order` (a permutation of the indices) while image i keeps index i:
        what lets the images of one shape be neighbours (the [G][n_pixels] maps of one rl_ensemble_stats call) whatever their
        indices.  offsets[i] is still image i's element offset; there is no offsets[len(shapes)]."""
        shapes = [tuple(s) for s in shapes]
        out = cls([shapes[i] for i in order], dtype, device)
        offsets = np.zeros(len(shapes), dtype=np.int64)
        offsets[list(order)] = out.offsets[:-1]
        out.shapes, out.offsets = shapes, offsets
        return out

    @classmethod
    def from_host(cls, images, dtype='f64', device=0):
        """A buffer holding host images (true objects, say), uploaded once."""
        images = [np.asarray(im, dtype=np.float64) for im in images]
        out = cls([im.shape[-2:] for im in images], dtype, device)
        flat = np.concatenate([im.ravel() for im in images]) if images else np.zeros(0)
        check(lib.rl_device_upload(out.ctx.handle, out.dev, DTYPES[dtype], out.n, ptr(np.ascontiguousarray(flat))))
        return out

    def ring_stats(self, a_idx, b_idx=None, truth=None, truth_index=None, scale=None, n_rings=None, n_sectors=None):
        """Ring statistics (quality.ring_stats, include/rlsted.h rl_ring_stats) of image pairs without a download: images `a_idx`
        of this buffer against images `b_idx` of the same buffer (two seeds of a sweep), or against images `truth_index` (one
        index, or one per pair) of `truth`, another DeviceResults of this GPU (DeviceResults.from_host of the true objects).
        scale: None, a number or one per pair, multiplied into the b side.  All images of a call share one shape (ValueError
        otherwise).  n_sectors = S: per (ring, orientation sector) cell (quality.sector_stats, rl_ring_sector_stats).  Returns
        [len(a_idx)][R][5] float64, with sectors [len(a_idx)][R][S][5]; synchronises this buffer's context, so whatever wrote the images must have
        been synchronised (run_tasks_device has)."""
        a_idx = [int(i) for i in np.atleast_1d(a_idx)]
        if (b_idx is None) == (truth is None):
            raise ValueError('give either b_idx or truth')
        other = self if truth is None else truth
        if truth is not None:
            if truth.ctx.device != self.ctx.device:
                raise ValueError('truth lives on another device')
            b_idx = np.zeros(len(a_idx), dtype=np.int64) if truth_index is None else truth_index
        b_idx = [int(i) for i in np.broadcast_to(np.atleast_1d(b_idx), (len(a_idx),))]
        if not a_idx:
            raise ValueError('no pairs')
        shape = self.shapes[a_idx[0]]
        if any(self.shapes[i] != shape for i in a_idx) or any(other.shapes[i] != shape for i in b_idx):
            raise ValueError('the images of one ring_stats call must share one shape')
        if n_sectors is not None:
            return quality.sector_stats_device(self.ctx, self.dev, self.dtype, self.offsets[a_idx], other.dev, other.dtype,
                                               other.offsets[b_idx], shape, n_sectors, scale, n_rings)
        return quality.ring_stats_device(self.ctx, self.dev, self.dtype, self.offsets[a_idx], other.dev, other.dtype,
                                         other.offsets[b_idx], shape, scale, n_rings)

    def _ensemble_into(self, groups, truth, truth_index, scale, mean_ptr, var_ptr):
        """One rl_ensemble_stats call on the images `groups` (index lists) of this buffer; the maps go to the device addresses
        given (None: not written).  Returns [G][6]."""
        groups = [[int(i) for i in np.atleast_1d(g)] for g in groups]
        if not groups or any(not g for g in groups):
            raise ValueError('no groups, or an empty group')
        shape = self.shapes[groups[0][0]]
        if any(self.shapes[i] != shape for g in groups for i in g):
            raise ValueError('the images of one ensemble call must share one shape')
        t = None
        if truth is not None:
            if truth.ctx.device != self.ctx.device:
                raise ValueError('truth lives on another device')
            t_idx = np.zeros(len(groups), dtype=np.int64) if truth_index is None else truth_index
            t_idx = [int(i) for i in np.broadcast_to(np.atleast_1d(t_idx), (len(groups),))]
            if any(truth.shapes[i] != shape for i in t_idx):
                raise ValueError('the images of one ensemble call must share one shape')
            t = (truth.dev, truth.dtype, truth.offsets[t_idx], scale)
        return quality.ensemble_stats_device(self.ctx, self.dev, self.dtype, [self.offsets[g] for g in groups], shape[0] * shape[1],
                                             truth=t, mean_dev=mean_ptr, var_dev=var_ptr)

    def ensemble(self, groups, truth=None, truth_index=None, scale=None, maps=True):
        """Ensemble statistics (quality.ensemble_stats, include/rlsted.h rl_ensemble_stats) without a download: group g is the
        images `groups[g]` (a list of index lists; the groups may differ in size) of this buffer -- the seeds of one operating
        point of a sweep.  truth: None, or another DeviceResults of this GPU whose image `truth_index` (one index, or one per
        group), times `scale` (None, a number or one per group), is the group's true image.  All images of a call share one shape
        (ValueError otherwise).  Returns (means, variances, scalars): two float64 DeviceResults on this GPU holding one map per
        group (None, None with maps=False) and [G][6] -- n and the pixel sums of mean, variance, bias^2, mean squared error and
        (scaled truth)^2.  Synchronises this buffer's context, so whatever wrote the images must have been synchronised."""
        means = variances = None
        try:
            if maps:
                shape = self.shapes[int(np.atleast_1d(groups[0])[0])] if len(groups) and len(np.atleast_1d(groups[0])) else (0, 0)
                means = DeviceResults([shape] * len(groups), 'f64', self.ctx.device)
                variances = DeviceResults([shape] * len(groups), 'f64', self.ctx.device)
            sc = self._ensemble_into(groups, truth, truth_index, scale, means.dev if maps else None, variances.dev if maps else None)
        except Exception:
            for m in (means, variances):
                if m is not None:
                    m.free()
            raise
        return means, variances, sc

    def free(self):
        if getattr(self, 'dev', None) is not None and self.dev.value and lib is not None:    # (lib: gone at interpreter shutdown)
            lib.rl_device_free(self.ctx.handle, self.dev)
            self.dev = ctypes.c_void_p()

    __del__ = free


def _by_shape(shapes):
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(tuple(s), []).append(i)
    return groups


def _pack_stats(per_task):
    """An array [n][R][5] ([n][R][S][5] with sectors) when every task has the same number of rings, otherwise the list."""
    return np.stack(per_task) if per_task and len({s.shape for s in per_task}) == 1 else per_task


def score_tasks(res, tasks, objects, total_brightness=5e10, n_rings=None, n_sectors=None):
    """The ring statistics of every task's estimate in `res` (the DeviceResults of `tasks`) against its true object scaled to the
    simulated brightness, scale = total_brightness / object.sum() (create_data_from_object, line_sted_tools.py:505-506), on the
    device: each distinct object is uploaded once as float64, one rl_ring_stats call per image shape.  Returns [n_tasks][R][5]
    (fields: quality.ring_stats; quality.radial_error_from_stats turns field 4 into the ring RMS of the reference's fourier_error)
    -- a list of per-task arrays when shapes with different numbers of rings are mixed.  n_sectors = S: angle-resolved, a task's
    score is [R][S][5] (rl_ring_sector_stats; quality.rings_from_sectors sums it back to [R][5])."""
    names = sorted({o for o, _, _ in tasks})
    where = {n: i for i, n in enumerate(names)}
    imgs = [np.asarray(objects[n], dtype=np.float64).reshape(np.shape(objects[n])[-2:]) for n in names]
    scales = {n: float(total_brightness) / float(im.sum()) for n, im in zip(names, imgs)}
    truths = DeviceResults.from_host(imgs, 'f64', res.ctx.device)
    out = [None] * len(tasks)
    try:
        for shape, idxs in _by_shape([res.shapes[i] for i in range(len(tasks))]).items():
            st = res.ring_stats(idxs, truth=truths, truth_index=[where[tasks[i][0]] for i in idxs],
                                scale=[scales[tasks[i][0]] for i in idxs], n_rings=n_rings, n_sectors=n_sectors)
            for k, i in enumerate(idxs):
                out[i] = st[k]
    finally:
        truths.free()
    return _pack_stats(out)


def frc_between_seeds(res, tasks, seed_a, seed_b, n_rings=None, n_sectors=None):
    """Fourier ring statistics between the two noise realisations `seed_a`, `seed_b` of every (object, PSF set) of `tasks` that
    has both, straight from `res`: returns (keys, stats) -- keys the (object, PSF set) pairs in task order of seed_a, stats
    [len(keys)][R][5] (a list when ring counts differ); quality.frc_from_stats(stats) is the FRC curve.  n_sectors = S: stats
    [len(keys)][R][S][5], one curve per orientation (quality.frc_resolution_by_angle)."""
    at = {t: i for i, t in enumerate(tasks)}
    keys = [(o, p) for o, p, s in tasks if s == int(seed_a) and (o, p, int(seed_b)) in at]
    if not keys:
        raise ValueError('no (object, PSF set) has both seeds %r and %r' % (seed_a, seed_b))
    ia = [at[(o, p, int(seed_a))] for o, p in keys]
    ib = [at[(o, p, int(seed_b))] for o, p in keys]
    out = [None] * len(keys)
    for shape, ks in _by_shape([res.shapes[i] for i in ia]).items():
        st = res.ring_stats([ia[k] for k in ks], b_idx=[ib[k] for k in ks], n_rings=n_rings, n_sectors=n_sectors)
        for j, k in enumerate(ks):
            out[k] = st[j]
    return keys, _pack_stats(out)


def ensemble_keys(tasks):
    """(keys, members): the (object, PSF set) pairs of `tasks` in order of first appearance, and per key the indices of all its
    seeds in task order."""
    members = {}
    for i, (o, p, _) in enumerate(tasks):
        members.setdefault((o, p), []).append(i)
    keys = list(members)
    return keys, [members[k] for k in keys]


def _upload_truths(tasks, objects, total_brightness, device):
    """The distinct objects of `tasks` as one float64 device buffer: (buffer, index of a name, scale of a name)."""
    names = sorted({o for o, _, _ in tasks})
    where = {n: i for i, n in enumerate(names)}
    imgs = [np.asarray(objects[n], dtype=np.float64).reshape(np.shape(objects[n])[-2:]) for n in names]
    scales = {n: float(total_brightness) / float(im.sum()) for n, im in zip(names, imgs)}
    return DeviceResults.from_host(imgs, 'f64', device), where, scales


def ensemble_tasks(res, tasks, objects, total_brightness=5e10, maps=True):
    """The ensemble statistics of every (object, PSF set) operating point of `tasks` over its seeds, from `res` (the DeviceResults
    of `tasks`) on the device: the truth is the object scaled to the simulated brightness, scale = total_brightness / object.sum()
    as in score_tasks, each distinct object uploaded once as float64; one rl_ensemble_stats call per image shape.  Returns (keys,
    counts, means, variances, scalars): the keys in order of first appearance (ensemble_keys), the number of seeds of each, two
    float64 DeviceResults on res's GPU holding the per-pixel mean and unbiased variance map of key k as image k (None, None with
    maps=False) and scalars [n_keys][6] (DeviceResults.ensemble): sum bias^2 (field 3) is what the blur leaves, sum variance
    (field 2) what the noise adds, and field 4 = field 3 + (n - 1) / n field 2 up to rounding."""
    keys, members = ensemble_keys(tasks)
    counts = np.array([len(m) for m in members], dtype=np.int64)
    scalars = np.zeros((len(keys), quality.ENSEMBLE_FIELDS))
    if not keys:
        return keys, counts, None, None, scalars
    key_shapes = [res.shapes[m[0]] for m in members]
    by_shape = _by_shape(key_shapes)
    means = variances = None
    truths, where, scales = _upload_truths(tasks, objects, total_brightness, res.ctx.device)
    try:
        if maps:
            order = [k for ks in by_shape.values() for k in ks]          # the keys of one shape are neighbours in memory
            means = DeviceResults.with_layout(key_shapes, order, 'f64', res.ctx.device)
            variances = DeviceResults.with_layout(key_shapes, order, 'f64', res.ctx.device)
        for shape, ks in by_shape.items():
            sc = res._ensemble_into([members[k] for k in ks], truths, [where[keys[k][0]] for k in ks], [scales[keys[k][0]] for k in ks],
                                    means.address(ks[0]) if maps else None, variances.address(ks[0]) if maps else None)
            scalars[ks] = sc
    except Exception:
        for m in (means, variances):
            if m is not None:
                m.free()
        raise
    finally:
        truths.free()
    return keys, counts, means, variances, scalars


def bias_variance_spectrum(res, tasks, objects, total_brightness=5e10, n_rings=None, n_sectors=None):
    """The spectral form of ensemble_tasks' split, per ring (per (ring, orientation sector) cell with n_sectors = S), from the ring
    entry points alone -- the DFT is linear, so the spectrum of the mean image is the mean of the spectra:
        bias power      field 4 of the pair (mean image, truth, scale): sum |fft2(mean) - fft2(s t)|^2
        variance power  1 / (n - 1) sum_m field 4 of (member m, mean image, scale 1): the unbiased variance of the members' spectra
                        (0 for a key with one seed)
    Returns (keys, counts, spectrum, mean_stats): per key spectrum [R][3] ([R][S][3]) = bin count, bias power, variance power
    (quality.spectral_bias_variance_rms reads it), and mean_stats [R][5] ([R][S][5]), the ring statistics of (mean image, truth)
    whose field 1 quality.ssnr_from wants; lists when ring counts differ.  For every bin set,
        mean over seeds of field 4 (member, truth) = bias power + (n - 1) / n variance power   up to rounding."""
    keys, members = ensemble_keys(tasks)
    k_, counts, means, variances, _ = ensemble_tasks(res, tasks, objects, total_brightness, maps=True)
    spectrum, mean_stats = [None] * len(keys), [None] * len(keys)
    truths = None
    try:
        truths, where, scales = _upload_truths(tasks, objects, total_brightness, res.ctx.device)
        for shape, ks in _by_shape([res.shapes[m[0]] for m in members]).items():
            ms = means.ring_stats(ks, truth=truths, truth_index=[where[keys[k][0]] for k in ks], scale=[scales[keys[k][0]] for k in ks],
                                  n_rings=n_rings, n_sectors=n_sectors)
            flat = [i for k in ks for i in members[k]]
            vs = res.ring_stats(flat, truth=means, truth_index=[k for k in ks for _ in members[k]], n_rings=n_rings, n_sectors=n_sectors)
            at = 0
            for j, k in enumerate(ks):
                n = len(members[k])
                power = np.zeros(ms[j].shape[:-1])
                for m in range(n):                                       # (member order: one fixed float64 sum)
                    power = power + vs[at + m][..., 4]
                at += n
                sp = np.zeros(ms[j].shape[:-1] + (3,))
                sp[..., 0] = ms[j][..., 0]
                sp[..., 1] = ms[j][..., 4]
                sp[..., 2] = power / (n - 1) if n > 1 else 0.0
                spectrum[k], mean_stats[k] = sp, ms[j]
    finally:
        for b in (means, variances, truths):
            if b is not None:
                b.free()
    return keys, counts, _pack_stats(spectrum), _pack_stats(mean_stats)


def _increasing_from_one(iterations_list):
    ks = [int(k) for k in iterations_list]
    return len(ks) > 0 and ks[0] >= 1 and all(b > a for a, b in zip(ks, ks[1:])) and all(k == K for k, K in zip(ks, iterations_list))


def _bias_variance_one_sweep_per_k(tasks, keys, objects, psf_sets, iterations_list, total_brightness, dtype, device, acceleration,
                                   tv_lambda, tv_epsilon):
    """bias_variance_vs_iterations without checkpoints: run_tasks_device once per K, each time from ones on the same measurements
    -- sum(iterations_list) iterations per task.  What a list that is not strictly increasing from 1 gets, and what the tests
    hold the one-sweep form against."""
    out = np.zeros((len(iterations_list), len(keys), quality.ENSEMBLE_FIELDS))
    for j, K in enumerate(iterations_list):
        res = run_tasks_device(tasks, objects, psf_sets, int(K), total_brightness, dtype, device, acceleration=acceleration,
                               tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
        try:
            out[j] = ensemble_tasks(res, tasks, objects, total_brightness, maps=False)[4]
        finally:
            res.free()
    return out


def bias_variance_vs_iterations(objects, psf_sets, seeds, iterations_list, total_brightness=5e10, dtype='f32', device=0,
                                acceleration=None, tv_lambda=None, tv_epsilon=0.1):
    """The semi-convergence picture: the ensemble scalars of every (object, PSF set) over `seeds` after K iterations, for every K
    of `iterations_list`.  A strictly increasing list that starts at 1 or above runs ONE sweep of max(iterations_list) iterations
    on the group-sorted tasks that takes a checkpoint at every K (run_tasks_checkpoints_device) and reduces each checkpoint with
    ensemble_tasks(maps=False): a checkpoint is bit for bit the estimate of a sweep of K iterations, so the numbers are those of
    one sweep per K at max(iterations_list) iterations per task.  Any other list runs run_tasks_device once per K, each time from
    ones on the SAME measurements (a task's noise depends only on its Philox key (seed, object id)), at sum(iterations_list)
    iterations per task.  Returns (keys, out): out [len(iterations_list)][n_keys][6], row j what
    ensemble_tasks gives for a sweep of iterations_list[j] iterations -- sum bias^2 (field 3) against sum variance (field 2)."""
    tasks = make_tasks(objects, psf_sets, seeds)
    tasks = [tasks[i] for i in sort_by_group(tasks, objects)]
    keys = ensemble_keys(tasks)[0]
    if not _increasing_from_one(iterations_list):
        return keys, _bias_variance_one_sweep_per_k(tasks, keys, objects, psf_sets, iterations_list, total_brightness, dtype, device,
                                                    acceleration, tv_lambda, tv_epsilon)
    out = np.zeros((len(iterations_list), len(keys), quality.ENSEMBLE_FIELDS))
    results, _ = run_tasks_checkpoints_device(tasks, objects, psf_sets, iterations_list, total_brightness, dtype, device,
                                              acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon, trace=False)
    try:
        for j, res in enumerate(results):
            out[j] = ensemble_tasks(res, tasks, objects, total_brightness, maps=False)[4]
    finally:
        for res in results:
            res.free()
    return keys, out


def split_flat(flat, shapes):
    out, o = [], 0
    for s in shapes:
        out.append(flat[o:o + s[0] * s[1]].reshape(s))
        o += s[0] * s[1]
    return out


SWEEP_STREAMS = 4      # contexts of one GPU the groups of a sweep are dealt to in turn (their launches overlap); measured on
#                        config 4's 1152 tasks: 1 / 2 / 3 / 4 / 6 / 8 contexts 43.7 / 34.0 / 31.6 / 30.7 / 31.4 / 33.3 ms


def run_tasks_device(tasks, objects, psf_sets, iterations, total_brightness=5e10, dtype='f32', device=0,
                     max_frames_per_plan=256, streams=SWEEP_STREAMS, timing=None, acceleration=None, tv_lambda=None, tv_epsilon=0.1):
    """Enqueue the tasks on one GPU (group by group, `rl_batch_submit`), synchronise once; returns their DeviceResults.
    timing (dict, optional): receives 'enqueue_s', the host's share (staging + launches) before the one synchronisation.
    acceleration: None or 'biggs-andrews' (DeconvPlan): every task's iterations from ones, with a history of its own.
    tv_lambda, tv_epsilon: the total-variation regulariser of every task's iterations (DeconvPlan.set_tv; None: off)."""
    import time
    t_start = time.perf_counter()
    ids = object_ids(objects)
    res = DeviceResults([objects[o].shape[-2:] for o, _, _ in tasks], dtype, device)
    groups = {}
    for idx, key in enumerate(task_groups(tasks, objects)):
        groups.setdefault(key, []).append(idx)
    used = set()
    n_sub = 0
    for (p, shape), idxs in groups.items():
        for start in range(0, len(idxs), max_frames_per_plan):
            part = idxs[start:start + max_frames_per_plan]
            # (the tasks of a piece are consecutive in `res`: a piece is a run of one group's tasks in task order only if
            # the caller's tasks are grouped; in general every task is submitted to its own address)
            stream = n_sub % max(1, streams)
            n_sub += 1
            plan = plan_for(psf_sets[p], len(part), shape, dtype, device, stream, acceleration, tv_lambda, tv_epsilon)
            used.add(stream)
            frames = [np.ascontiguousarray(np.asarray(objects[tasks[i][0]], dtype=np.float64).reshape(shape)) for i in part]
            runs = _consecutive_runs(part, res)
            for a, b in runs:                         # maximal runs of tasks that are neighbours in the result buffer
                plan.batch_submit(frames[a:b], total_brightness, [tasks[i][2] for i in part[a:b]], [ids[tasks[i][0]] for i in part[a:b]],
                                  iterations, res.address(part[a]), dtype, rng=RNG_PHILOX)
    if timing is not None:
        timing['enqueue_s'] = time.perf_counter() - t_start
    for st in used:
        Context.get(device, st).synchronize()
    return res


def run_tasks_checkpoints_device(tasks, objects, psf_sets, iterations_list, total_brightness=5e10, dtype='f32', device=0,
                                 max_frames_per_plan=256, streams=SWEEP_STREAMS, timing=None, acceleration=None, tv_lambda=None,
                                 tv_epsilon=0.1, estimates=True, trace=True):
    """run_tasks_device with iterations_list[-1] iterations that takes every task's estimate out after each K of `iterations_list`
    (strictly increasing, from 1) inside the enqueued run (`rl_batch_submit_checkpoints`): the same grouping, plan cache and
    contexts, one synchronisation.  Returns (results, trace): `results` a list of len(iterations_list) DeviceResults, entry j bit for
    bit what run_tasks_device gives with iterations_list[j] (None with estimates=False); `trace` a host array
    [len(iterations_list)][n_tasks][quality.TRACE_FIELDS] in task order, the six sums of every checkpoint against the task's scaled
    object (quality.trace_metrics reads it; None with trace=False) -- one small download from a device buffer.  With
    estimates=False a sweep can trace every iteration, range(1, K + 1), without storing an image."""
    import time
    t_start = time.perf_counter()
    ks = [int(k) for k in iterations_list]
    n_k, n_tasks = len(ks), len(tasks)
    ids = object_ids(objects)
    shapes = [objects[o].shape[-2:] for o, _, _ in tasks]
    results = [DeviceResults(shapes, dtype, device) for _ in ks] if estimates else None
    ctx = Context.get(device)
    trace_dev = ctypes.c_void_p()
    row = n_tasks * quality.TRACE_FIELDS
    if trace:
        check(lib.rl_device_alloc(ctx.handle, max(n_k * row, 1) * 8, ctypes.byref(trace_dev)))
    try:
        groups = {}
        for idx, key in enumerate(task_groups(tasks, objects)):
            groups.setdefault(key, []).append(idx)
        used = set()
        n_sub = 0
        for (p, shape), idxs in groups.items():
            for start in range(0, len(idxs), max_frames_per_plan):
                part = idxs[start:start + max_frames_per_plan]
                stream = n_sub % max(1, streams)
                n_sub += 1
                plan = plan_for(psf_sets[p], len(part), shape, dtype, device, stream, acceleration, tv_lambda, tv_epsilon)
                used.add(stream)
                frames = [np.ascontiguousarray(np.asarray(objects[tasks[i][0]], dtype=np.float64).reshape(shape)) for i in part]
                for a, b in _consecutive_runs(part, None):
                    plan.batch_submit_checkpoints(
                        frames[a:b], total_brightness, [tasks[i][2] for i in part[a:b]], [ids[tasks[i][0]] for i in part[a:b]], ks,
                        [r.address(part[a]) for r in results] if estimates else None, dtype,
                        [trace_dev.value + (j * row + part[a] * quality.TRACE_FIELDS) * 8 for j in range(n_k)] if trace else None,
                        rng=RNG_PHILOX)
        if timing is not None:
            timing['enqueue_s'] = time.perf_counter() - t_start
        for st in used:
            Context.get(device, st).synchronize()
        out = None
        if trace:
            out = np.zeros((n_k, n_tasks, quality.TRACE_FIELDS))
            if n_k * row:
                check(lib.rl_device_download(ctx.handle, trace_dev, DTYPES['f64'], n_k * row, ptr(out)))
    except Exception:
        for r in results or ():
            r.free()
        raise
    finally:
        if trace_dev:
            check(lib.rl_device_free(ctx.handle, trace_dev))
    return results, out


def best_iterations(trace, iterations_list):
    """Per task, the K of `iterations_list` at which the squared error against the scaled object (field 5 of the trace
    [n_k][n_tasks][6] of run_tasks_checkpoints_device) is smallest; the first such K on a tie."""
    trace = np.asarray(trace, dtype=np.float64)
    return np.asarray([int(k) for k in iterations_list])[np.argmin(trace[..., 5], axis=0)]


def error_vs_iterations(objects, psf_sets, seeds, iterations_list, total_brightness=5e10, dtype='f32', device=0, acceleration=None,
                        tv_lambda=None, tv_epsilon=0.1):
    """The error curve of every (object, PSF set, seed) over `iterations_list` from ONE sweep of iterations_list[-1] iterations that
    stores no image: (tasks, metrics), the group-sorted tasks and quality.trace_metrics of their trace, each entry
    [len(iterations_list)][n_tasks]."""
    tasks = make_tasks(objects, psf_sets, seeds)
    tasks = [tasks[i] for i in sort_by_group(tasks, objects)]
    _, trace = run_tasks_checkpoints_device(tasks, objects, psf_sets, iterations_list, total_brightness, dtype, device,
                                            acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon, estimates=False)
    n_pixels = np.array([objects[o].shape[-2] * objects[o].shape[-1] for o, _, _ in tasks], dtype=np.float64)
    return tasks, quality.trace_metrics(trace, n_pixels)


def _consecutive_runs(part, res):
    """[(a, b)): maximal ranges of `part` whose task indices are consecutive (their images are neighbours in `res`)."""
    runs, a = [], 0
    for k in range(1, len(part) + 1):
        if k == len(part) or part[k] != part[k - 1] + 1:
            runs.append((a, k))
            a = k
    return runs


def sort_by_group(tasks, objects):
    """Task indices ordered so that the tasks of one (PSF set, shape) group are neighbours: one submit per piece."""
    keys = task_groups(tasks, objects)
    return sorted(range(len(tasks)), key=lambda i: (keys[i][0], keys[i][1], i))


def run_tasks(tasks, objects, psf_sets, iterations, total_brightness=5e10, dtype='f32', device=0,
              max_frames_per_plan=256, acceleration=None, tv_lambda=None, tv_epsilon=0.1):
    """Run tasks on one GPU.  Returns a list of (ny, nx) estimates in task order."""
    order = sort_by_group(tasks, objects)
    res = run_tasks_device([tasks[i] for i in order], objects, psf_sets, iterations, total_brightness, dtype, device,
                           max_frames_per_plan, acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
    est = res.download()
    res.free()
    out = [None] * len(tasks)
    for k, i in enumerate(order):
        out[i] = est[k]
    return out


def run_and_score_tasks(tasks, objects, psf_sets, iterations, total_brightness=5e10, dtype='f32', device=0, n_rings=None,
                        acceleration=None, tv_lambda=None, tv_epsilon=0.1, n_sectors=None):
    """run_tasks, with every estimate scored on the device before the one download (score_tasks).  Returns (estimates, scores):
    two lists in task order, scores[i] of shape (R_i, 5), with n_sectors = S (R_i, S, 5)."""
    order = sort_by_group(tasks, objects)
    sorted_tasks = [tasks[i] for i in order]
    res = run_tasks_device(sorted_tasks, objects, psf_sets, iterations, total_brightness, dtype, device,
                           acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
    sc = score_tasks(res, sorted_tasks, objects, total_brightness, n_rings, n_sectors)
    est = res.download()
    res.free()
    out, scores = [None] * len(tasks), [None] * len(tasks)
    for k, i in enumerate(order):
        out[i], scores[i] = est[k], np.asarray(sc[k])
    return out, scores


def run_score_reduce_tasks(tasks, objects, psf_sets, iterations, total_brightness=5e10, dtype='f32', device=0, scores=False, n_rings=None,
                           acceleration=None, tv_lambda=None, tv_epsilon=0.1, n_sectors=None):
    """run_tasks, with the ensemble of every (object, PSF set) of `tasks` reduced on the device before the one download
    (ensemble_tasks(maps=False)), and -- scores=True -- every estimate scored as well (score_tasks).  Returns (estimates, scores,
    keys, scalars): estimates and scores in task order (scores None with scores=False), the keys in order of first appearance in
    the group-sorted tasks and their scalars [n_keys][6]."""
    order = sort_by_group(tasks, objects)
    sorted_tasks = [tasks[i] for i in order]
    res = run_tasks_device(sorted_tasks, objects, psf_sets, iterations, total_brightness, dtype, device,
                           acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
    try:
        sc = score_tasks(res, sorted_tasks, objects, total_brightness, n_rings, n_sectors) if scores else None
        keys, _, _, _, scalars = ensemble_tasks(res, sorted_tasks, objects, total_brightness, maps=False)
        est = res.download()
    finally:
        res.free()
    out, out_scores = [None] * len(tasks), [None] * len(tasks) if scores else None
    for k, i in enumerate(order):
        out[i] = est[k]
        if scores:
            out_scores[i] = np.asarray(sc[k])
    return out, out_scores, keys, scalars


def pad_stack(images, shape):
    """Stack 2-D images of different sizes into one (n, shape[0], shape[1]) array, top-left aligned
    and zero filled."""
    out = np.zeros((len(images),) + tuple(shape), dtype=np.float64)
    for k, im in enumerate(images):
        out[k, :im.shape[0], :im.shape[1]] = im
    return out


PLAN_SETUP_FRAMES = 24     # what building a plan costs a rank, in frames of its group's task cost (sharding.partition_groups)


def shard_sweep(tasks, objects, psf_sets, iterations, world):
    """The sweep's partition: whole (PSF set, shape) groups per rank -- a plan is then built, and its set-up paid, on one rank
    only -- groups of 128 tasks and more in pieces of at least 64.  Returns (shards, costs): task indices per rank, group sorted."""
    costs = task_costs(tasks, objects, psf_sets, iterations)
    keys = task_groups(tasks, objects)
    shards = sharding.partition_groups(keys, costs, world, setup_frames=PLAN_SETUP_FRAMES)
    order = {i: k for k, i in enumerate(sort_by_group(tasks, objects))}
    return [sorted(s, key=lambda i: order[i]) for s in shards], costs


def figure_2_sweep(objects, psf_sets, seeds, iterations, total_brightness=5e10, dtype='f32',
                   device=0, comm=None, info=None, acceleration=None, tv_lambda=None, tv_epsilon=0.1, scores=False, n_rings=None,
                   n_sectors=None, ensemble=False):
    """The sweep, sharded over the ranks of `comm` (sharding.RcclComm, or anything with its
    interface) when given.  Returns (tasks, estimates) on rank 0 and (tasks, None) elsewhere;
    estimates is an array (n_tasks, ny, nx) when all objects share a shape, otherwise a list of
    (ny, nx) arrays in task order.  The one gather carries the ranks' estimates unpadded: from device buffer to device
    buffer in the plans' arithmetic type (`comm.gather_device`), or -- a stand-in communicator without it -- as flat host
    arrays.  info (dict, optional) receives the partition's statistics.  acceleration: None (the reference's iteration) or
    'biggs-andrews' (DeconvPlan.set_acceleration); tv_lambda, tv_epsilon: the total-variation regulariser (DeconvPlan.set_tv; None: off).
    scores=True: every rank also scores its own shard on the device (score_tasks, `n_rings` rings) before the gather, the small
    score arrays travel through `comm.gather`, and the function returns (tasks, estimates, scores) -- scores [n_tasks][R][5] in task
    order (a list when ring counts differ) on rank 0, None elsewhere.  The estimates are those of scores=False.  n_sectors = S:
    the scores are angle-resolved, [n_tasks][R][S][5] (score_tasks).
    ensemble=True: every rank also reduces the (object, PSF set) operating points of its own shard over their seeds on the device
    (ensemble_tasks(maps=False)); only the [6] scalars per key travel, through `comm.gather`, and the function returns one more
    element, (keys, scalars) on rank 0 -- the keys rank by rank, within a rank in order of first appearance in its shard, scalars
    [n_keys][6] -- and None elsewhere.  The estimates are those of ensemble=False.  A partition that puts the seeds of one key on
    different ranks raises ValueError naming the key: partial statistics are not merged."""
    tasks = make_tasks(objects, psf_sets, seeds)
    world = comm.world if comm is not None else 1
    rank = comm.rank if comm is not None else 0
    shards, costs = shard_sweep(tasks, objects, psf_sets, iterations, world)
    mine = [tasks[i] for i in shards[rank]]
    if ensemble:
        owner = {}
        for r, sh in enumerate(shards):
            for i in sh:
                if owner.setdefault(tasks[i][:2], r) != r:
                    raise ValueError('the partition put the seeds of %r on ranks %d and %d; an ensemble is reduced on one rank'
                                     % (tasks[i][:2], owner[tasks[i][:2]], r))
    mine_keys, mine_ens = [], np.zeros((0, quality.ENSEMBLE_FIELDS))
    shapes = [tuple(objects[o].shape[-2:]) for o, _, _ in tasks]
    pix = [sum(shapes[i][0] * shapes[i][1] for i in sh) for sh in shards]
    if info is not None:
        info.update(sharding.partition_stats(shards, costs, task_groups(tasks, objects)))
    mine_scores = None
    if comm is not None and hasattr(comm, 'gather_device'):
        res = run_tasks_device(mine, objects, psf_sets, iterations, total_brightness, dtype, device, acceleration=acceleration,
                               tv_lambda=tv_lambda, tv_epsilon=tv_epsilon)
        if info is not None:
            info['unresolved_predictions_this_rank'] = unresolved_total(reset=True)
        if scores and mine:
            mine_scores = score_tasks(res, mine, objects, total_brightness, n_rings, n_sectors)
        if ensemble and mine:
            mine_keys, _, _, _, mine_ens = ensemble_tasks(res, mine, objects, total_brightness, maps=False)
        flat = comm.gather_device(res, pix, 0)       # root: host float64, rank-major; others: None
        res.free()
    else:
        if ensemble:
            local, mine_scores, mine_keys, mine_ens = run_score_reduce_tasks(
                mine, objects, psf_sets, iterations, total_brightness, dtype, device, scores, n_rings, acceleration=acceleration,
                tv_lambda=tv_lambda, tv_epsilon=tv_epsilon, n_sectors=n_sectors) if mine else ([], [], mine_keys, mine_ens)
        elif scores:
            local, mine_scores = run_and_score_tasks(mine, objects, psf_sets, iterations, total_brightness, dtype, device, n_rings,
                                                     acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon,
                                                     n_sectors=n_sectors) if mine else ([], [])
        else:
            local = run_tasks(mine, objects, psf_sets, iterations, total_brightness, dtype, device,
                              acceleration=acceleration, tv_lambda=tv_lambda, tv_epsilon=tv_epsilon) if mine else []
        flat = np.concatenate([np.asarray(e, dtype=np.float64).ravel() for e in local]) if local else np.zeros(0)
        if comm is not None:
            flat = comm.gather(flat, pix, 0)
    order = [i for sh in shards for i in sh]
    all_scores = None
    if scores:
        rings = [quality.ring_count(*s) if n_rings is None else int(n_rings) for s in shapes]
        cell = (quality.RING_FIELDS,) if n_sectors is None else (int(n_sectors), quality.RING_FIELDS)    # what a ring holds
        per_ring = int(np.prod(cell))
        have = mine_scores is not None and len(mine_scores)
        sflat = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in mine_scores]) if have else np.zeros(0)
        if comm is not None:
            sflat = comm.gather(sflat, [sum(rings[i] for i in sh) * per_ring for sh in shards], 0)
        if sflat is not None:
            all_scores, o = [None] * len(tasks), 0
            for i in order:
                k = rings[i] * per_ring
                all_scores[i] = np.asarray(sflat[o:o + k]).reshape((rings[i],) + cell)
                o += k
            all_scores = _pack_stats(all_scores)
    ens = None
    if ensemble:
        per_rank = [ensemble_keys([tasks[i] for i in sh])[0] for sh in shards]       # what every rank reduces, known everywhere
        at = {k: j for j, k in enumerate(mine_keys)}
        mine_ens = np.asarray(mine_ens, dtype=np.float64).reshape(-1, quality.ENSEMBLE_FIELDS)[[at[k] for k in per_rank[rank]]]
        eflat = np.ascontiguousarray(mine_ens).ravel()
        if comm is not None:
            eflat = comm.gather(eflat, [len(k) * quality.ENSEMBLE_FIELDS for k in per_rank], 0)
        if eflat is not None:
            ens = ([k for ks in per_rank for k in ks], np.asarray(eflat).reshape(-1, quality.ENSEMBLE_FIELDS))
    if flat is None:
        return ((tasks, None, None) if scores else (tasks, None)) + ((None,) if ensemble else ())
    parts = split_flat(np.asarray(flat), [shapes[i] for i in order])
    est = [None] * len(tasks)
    for k, i in enumerate(order):
        est[i] = parts[k]
    if len(set(shapes)) == 1:
        est = np.stack(est) if est else np.zeros((0,) + (shapes[0] if shapes else (0, 0)))
    return ((tasks, est, all_scores) if scores else (tasks, est)) + ((ens,) if ensemble else ())
