"""The cases of the plan matrix (tests/test_gpu_plan_matrix.py) and their admission: a generator of PSF sets, smooth object stacks,
doses and numpy Poisson measurements, the committed list of cases with their admitted seeds and iterate_until thresholds, the
scripted call sequence every case runs, and the conditions under which a case says something about the kernels at all.
Pure numpy on the oracle and the reference modules; test infrastructure only.

Admission (admit): evaluated on the model (plan_model.PlanModel) alone, float64, over the case's whole sequence --
    (a) every estimate is finite;
    (b) in every frame and view the smallest prediction is at least MIN_PREDICTION_RATIO of the largest (below, the oracle divides
        by a vanishing prediction where the device treats the pixel as neutral: two definitions, nothing about the kernels);
    (c) the final estimate moves by at most F32_SENSITIVITY (conftest.max_rel) when the PSFs and the measurements are rounded to
        float32 and back: a tenth of the f32 contract, the device keeps nine tenths.
Seeds that fail are replaced when CASES is written (python tests/plan_cases.py prints every case's figures and thresholds), never
at run time; tests/test_plan_model_cpu.py asserts every committed case admitted.
"""
import functools

import numpy as np

from conftest import max_rel          # (first: puts the repository's root on the path for the oracle)
import stop_reference as sr
from plan_model import BA, PlanModel

MIN_PREDICTION_RATIO = 1e-4
F32_SENSITIVITY = 1e-6
THRESHOLD_MARGIN = 1e-6          # no iterate_until decision of the model is closer to its threshold than this, relatively
TV_LAMBDA, TV_EPSILON = 0.01, 0.1
MODES = {'plain': (None, None), 'ba': (BA, None), 'tv': (None, TV_LAMBDA), 'batv': (BA, TV_LAMBDA)}
TOGGLE = {'plain': 'tv', 'ba': 'plain', 'tv': 'batv', 'batv': 'tv'}      # the mode of the one step in the middle of a run
ROWS = ('per_frame', 'pair', 'pair_switch', 'multi_view', 'split', 'separable', 'direct', 'slices')
FFT_ONLY = {'RLSTED_SEP': '0'}   # (RLSTED_SEP=0 also keeps the direct stencil away: deconv_build)


def _case(name, row, B, ny, nx, psf, seed, env=None, env32=None, want32=None, want64=None, lengths=None, levels=None, written=False,
          twin=None, slices=False):
    """psf: (kind, V, py, px).  env: the options of both element types, env32: of the f32 plan in addition.  want32 / want64: what
    strategy() must report; lengths: info()'s (ly, lx).  levels: per measurement of the sequence the frames' relative doses
    (None: drawn once, partners within a factor of 3).  twin: the options of a second f64 plan on another strategy."""
    return {'name': name, 'row': row, 'B': B, 'ny': ny, 'nx': nx, 'psf': psf, 'seed': seed, 'env': dict(env or {}),
            'env32': dict(env32 or {}), 'want32': dict(want32 or {}), 'want64': dict(want64 or {}), 'lengths': lengths,
            'levels': levels, 'written': written, 'twin': twin, 'slices': slices}


def plans_per_value(lib, psfs, B, ny, nx, dtype, switch, values=('0', '1'), options=None, fft_only=False):
    """One plan per value of `switch`, alive side by side, each with `options` besides (DeconvPlan's options; a value of None: the
    switch is not given, the plan has its default).  fft_only: no stencil may have taken the PSF set."""
    out = [lib.DeconvPlan(psfs, B, ny, nx, dtype=dtype, options=dict(options or {}, **({} if v is None else {switch: v})))
           for v in values]
    for p in out if fft_only else []:
        s = p.strategy()
        assert not s['separable'] and not s['direct_stencil']
    return out


_NO_PAIR = {'RLSTED_PAIR': '0'}
_FFT = {'separable': False, 'direct_stencil': False}
_PF = dict(_FFT, frame_pairs=False)
CASES = [
    # ---- per-frame FFT loop, one view: every transform length up to 1152
    _case('pf_64', 'per_frame', 2, 41, 37, ('generic', 1, 7, 9), 1, FFT_ONLY, _NO_PAIR, _PF, _PF, (64, 64)),
    _case('pf_192', 'per_frame', 1, 100, 20, ('symmetric', 1, 5, 5), 2, FFT_ONLY, _NO_PAIR, _PF, _PF, (192, 64)),
    _case('pf_256_even', 'per_frame', 2, 200, 12, ('generic', 1, 6, 4), 3, FFT_ONLY, _NO_PAIR, _PF, _PF, (256, 64)),
    _case('pf_576', 'per_frame', 1, 300, 10, ('generic', 1, 5, 3), 4, FFT_ONLY, _NO_PAIR, _PF, _PF, (576, 64)),
    _case('pf_1152_row', 'per_frame', 1, 12, 1100, ('generic', 1, 3, 9), 5, FFT_ONLY, _NO_PAIR, _PF, _PF, (64, 1152)),
    # ---- pair loop (f32): even and odd batches, the last pair half empty
    _case('pair_b2', 'pair', 2, 200, 200, ('symmetric', 1, 9, 9), 6, FFT_ONLY, None, dict(_FFT, frame_pairs=True), _PF, (256, 256)),
    _case('pair_b3', 'pair', 3, 200, 200, ('generic', 1, 7, 9), 107, FFT_ONLY, None, dict(_FFT, frame_pairs=True), _PF, (256, 256)),
    _case('pair_b5', 'pair', 5, 200, 200, ('generic', 1, 6, 4), 8, FFT_ONLY, None, dict(_FFT, frame_pairs=True), _PF, (256, 256),
          written=True),
    # ---- the pair loop and the per-frame loop inside one sequence: partners within a factor of 4, beyond it, within it again
    _case('switch_b4', 'pair_switch', 4, 200, 200, ('generic', 1, 5, 7), 9, FFT_ONLY, None, _FFT, _PF, (256, 256),
          levels=[(1, 2, 3, 1), (1, 10, 12, 1), (2, 1, 1, 3)]),
    # ---- several views: per view (f64), fused (f32); asymmetric and even-sized PSFs
    _case('views2_even', 'multi_view', 2, 41, 50, ('generic', 2, 6, 8), 10, FFT_ONLY, None, _PF, _PF, (64, 64)),
    _case('views3', 'multi_view', 1, 180, 30, ('generic', 3, 7, 5), 11, FFT_ONLY, None, _PF, _PF, (192, 64)),
    _case('views4_576', 'multi_view', 2, 300, 24, ('generic', 4, 5, 6), 12, FFT_ONLY, None, _PF, _PF, (576, 64)),
    # ---- split column pass (f32, column length 2304)
    _case('split_v2', 'split', 2, 1153, 40, ('generic', 2, 5, 7), 113, FFT_ONLY, None, dict(_PF, split_column_pass=True), _PF, (2304, 64)),
    _case('split_v3', 'split', 1, 1153, 40, ('generic', 3, 4, 6), 115, FFT_ONLY, None, dict(_PF, split_column_pass=True), _PF, (2304, 64)),
    # ---- separable stencils, two passes and one kernel; the f64 twin runs the FFT strategy
    _case('sep_two_pass', 'separable', 2, 45, 61, ('separable', 2, 7, 5), 15, {'RLSTED_SEP_ONE': '0'}, None, {'separable': True},
          {'separable': True}, twin=FFT_ONLY),
    _case('sep_one_kernel', 'separable', 3, 33, 64, ('separable', 1, 4, 9), 16, {'RLSTED_SEP_ONE': '1'}, None, {'separable': True},
          {'separable': True}, twin=FFT_ONLY),
    # ---- direct stencil: dense PSFs of 2-7 taps a side
    _case('direct_2x2', 'direct', 2, 33, 47, ('dense', 1, 2, 2), 17, None, None, {'direct_stencil': True}, {'direct_stencil': True},
          twin={'RLSTED_DIRECT': '0'}),
    _case('direct_7x6', 'direct', 2, 50, 64, ('dense', 2, 7, 6), 18, None, None, {'direct_stencil': True}, {'direct_stencil': True},
          twin={'RLSTED_DIRECT': '0'}),
    # ---- slices and lanes: five frames in three slices, the last one short
    _case('slices_lane1', 'slices', 5, 40, 36, ('generic', 2, 7, 9), 19, dict(FFT_ONLY, RLSTED_LANES='1'), None, _PF, _PF, (64, 64),
          slices=True),
    _case('slices_lane2', 'slices', 5, 40, 36, ('generic', 2, 7, 9), 20, dict(FFT_ONLY, RLSTED_LANES='2'), None, _PF, _PF, (64, 64),
          slices=True),
]
BY_NAME = {c['name']: c for c in CASES}

# (case, mode) -> (threshold of the relative rule, check_every 1; threshold of the discrepancy rule, check_every 3): between the
# frames' values where there are several, so that some frames stop and others do not; written by `python tests/plan_cases.py`
THRESHOLDS = {
    ('pf_64', 'plain'): (0.226776, 3.94721),
    ('pf_64', 'ba'): (0.226776, 3.35907),
    ('pf_64', 'tv'): (0.238868, 3.90255),
    ('pf_64', 'batv'): (0.238868, 3.31716),
    ('pf_192', 'plain'): (0.899384, 23.1956),
    ('pf_192', 'ba'): (0.899384, 21.3693),
    ('pf_192', 'tv'): (0.920938, 29.067),
    ('pf_192', 'batv'): (0.920938, 27.1553),
    ('pf_256_even', 'plain'): (0.210426, 1.56524),
    ('pf_256_even', 'ba'): (0.210426, 1.5352),
    ('pf_256_even', 'tv'): (0.246047, 1.62435),
    ('pf_256_even', 'batv'): (0.246047, 1.59467),
    ('pf_576', 'plain'): (0.403697, 1.82223),
    ('pf_576', 'ba'): (0.403697, 1.81664),
    ('pf_576', 'tv'): (0.525277, 1.83072),
    ('pf_576', 'batv'): (0.525277, 1.82636),
    ('pf_1152_row', 'plain'): (0.651162, 66.615),
    ('pf_1152_row', 'ba'): (0.651162, 50.1748),
    ('pf_1152_row', 'tv'): (0.72378, 69.3084),
    ('pf_1152_row', 'batv'): (0.72378, 53.0231),
    ('pair_b2', 'plain'): (0.384456, 80.263),
    ('pair_b2', 'ba'): (0.384456, 63.3038),
    ('pair_b2', 'tv'): (0.401125, 90.517),
    ('pair_b2', 'batv'): (0.401125, 73.1666),
    ('pair_b3', 'plain'): (0.275009, 414.703),
    ('pair_b3', 'ba'): (0.275009, 319.003),
    ('pair_b3', 'tv'): (0.302098, 404.631),
    ('pair_b3', 'batv'): (0.302098, 312.432),
    ('pair_b5', 'plain'): (0.232204, 4.77365),
    ('pair_b5', 'ba'): (0.232204, 4.16668),
    ('pair_b5', 'tv'): (0.273341, 4.38964),
    ('pair_b5', 'batv'): (0.273341, 3.85703),
    ('switch_b4', 'plain'): (0.208978, 1.82291),
    ('switch_b4', 'ba'): (0.208978, 1.69926),
    ('switch_b4', 'tv'): (0.230487, 1.81599),
    ('switch_b4', 'batv'): (0.230487, 1.69808),
    ('views2_even', 'plain'): (0.220256, 9.91071),
    ('views2_even', 'ba'): (0.220256, 8.68152),
    ('views2_even', 'tv'): (0.253386, 10.0867),
    ('views2_even', 'batv'): (0.253386, 8.82526),
    ('views3', 'plain'): (0.365581, 2.79195),
    ('views3', 'ba'): (0.365581, 2.69012),
    ('views3', 'tv'): (0.419589, 2.83024),
    ('views3', 'batv'): (0.419589, 2.7277),
    ('views4_576', 'plain'): (0.148115, 7.00987),
    ('views4_576', 'ba'): (0.148115, 6.74595),
    ('views4_576', 'tv'): (0.175986, 6.6607),
    ('views4_576', 'batv'): (0.175986, 6.39918),
    ('split_v2', 'plain'): (0.235448, 1.01462),
    ('split_v2', 'ba'): (0.235448, 1.00583),
    ('split_v2', 'tv'): (0.268102, 1.04103),
    ('split_v2', 'batv'): (0.268102, 1.03159),
    ('split_v3', 'plain'): (0.199513, 161.68),
    ('split_v3', 'ba'): (0.199513, 132.606),
    ('split_v3', 'tv'): (0.296208, 151.216),
    ('split_v3', 'batv'): (0.296208, 123.581),
    ('sep_two_pass', 'plain'): (0.273162, 2.75449),
    ('sep_two_pass', 'ba'): (0.273162, 2.59867),
    ('sep_two_pass', 'tv'): (0.321278, 3.02281),
    ('sep_two_pass', 'batv'): (0.321278, 2.87302),
    ('sep_one_kernel', 'plain'): (0.147366, 1579.89),
    ('sep_one_kernel', 'ba'): (0.147366, 1620.86),
    ('sep_one_kernel', 'tv'): (0.214371, 1450.11),
    ('sep_one_kernel', 'batv'): (0.214371, 1484.4),
    ('direct_2x2', 'plain'): (-0.627355, 13.5083),
    ('direct_2x2', 'ba'): (-0.627355, 14.263),
    ('direct_2x2', 'tv'): (-0.492966, 12.601),
    ('direct_2x2', 'batv'): (-0.492966, 13.316),
    ('direct_7x6', 'plain'): (0.106052, 16.2054),
    ('direct_7x6', 'ba'): (0.106052, 14.3248),
    ('direct_7x6', 'tv'): (0.158764, 16.6236),
    ('direct_7x6', 'batv'): (0.158764, 14.7587),
    ('slices_lane1', 'plain'): (0.0345334, 3.01146),
    ('slices_lane1', 'ba'): (0.0345334, 2.81226),
    ('slices_lane1', 'tv'): (0.0546928, 3.01547),
    ('slices_lane1', 'batv'): (0.0546928, 2.81312),
    ('slices_lane2', 'plain'): (0.158147, 4.86784),
    ('slices_lane2', 'ba'): (0.158147, 4.66351),
    ('slices_lane2', 'tv'): (0.178153, 5.11248),
    ('slices_lane2', 'batv'): (0.178153, 4.90429),
}


# ---------------------------------------------------------------------------------------------- the generator
def _gauss(n, s, shift=0.0):
    x = np.arange(n) - (n - 1) / 2 - shift
    return np.exp(-x ** 2 / (2 * s * s))


def psf_set(rng, kind, V, py, px):
    """V non-negative (1, py, px) PSFs of sum 1 / V.  generic: a shifted Gaussian envelope times random weights (asymmetric, full
    rank); separable: an outer product of two such rows; symmetric: generic plus its point reflection; dense: random taps."""
    out = []
    for _ in range(V):
        u = _gauss(py, rng.uniform(0.6, 0.3 * py + 0.7), rng.uniform(-0.8, 0.8)) * rng.uniform(0.5, 1.0, size=py)
        v = _gauss(px, rng.uniform(0.6, 0.3 * px + 0.7), rng.uniform(-0.8, 0.8)) * rng.uniform(0.5, 1.0, size=px)
        if kind == 'separable':
            p = np.outer(u, v)
        elif kind == 'dense':
            p = rng.uniform(0.1, 1.0, size=(py, px))
        else:
            p = np.outer(u, v) * rng.uniform(0.5, 1.0, size=(py, px))
            if kind == 'symmetric':
                p = p + p[::-1, ::-1]
        out.append((p / (p.sum() * V))[None])
    return out


def objects(rng, B, ny, nx):
    """(B, ny, nx) of mean 1: 2-6 Gaussian blobs of width 1.5-6 px on a floor of a quarter of their mean."""
    yy, xx = np.mgrid[:ny, :nx]
    out = np.zeros((B, ny, nx))
    for f in range(B):
        for _ in range(int(rng.integers(2, 7))):
            s = rng.uniform(1.5, 6.0)
            out[f] += rng.uniform(0.3, 1.0) * np.exp(-((yy - rng.uniform(0, ny)) ** 2 + (xx - rng.uniform(0, nx)) ** 2) / (2 * s * s))
        out[f] += 0.25 * out[f].mean()
        out[f] /= out[f].mean()
    return out


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def data(name, round32=False):
    """The case's PSFs, object stack (photons), its three measurements (B, V, ny, nx) and the estimate of its set_estimate."""
    c = BY_NAME[name]
    rng = np.random.default_rng([c['seed'], len(name)])
    kind, V, py, px = c['psf']
    psfs = psf_set(rng, kind, V, py, px)
    B, ny, nx = c['B'], c['ny'], c['nx']
    obj = objects(rng, B, ny, nx)
    dose = 10 ** rng.uniform(2, 5)                             # photons per pixel
    levels = c['levels'] or [tuple(rng.uniform(1.0, 3.0, size=B))] * 3
    model = PlanModel(psfs, B, ny, nx)
    meas = []
    for lv in levels:
        scaled = obj * (dose * np.asarray(lv, dtype=np.float64))[:, None, None]
        meas.append(rng.poisson(model.forward(scaled)) + 1e-9)
    x = obj * dose * rng.uniform(0.5, 1.5, size=obj.shape)
    obj = obj * dose
    if round32:
        psfs, meas = [_f32(p) for p in psfs], [_f32(m) for m in meas]
    return {'psfs': psfs, 'obj': obj, 'meas': meas, 'x': x}


# ---------------------------------------------------------------------------------------------- the sequence
def script(case, mode, thresholds=None):
    """The calls of a case, at most 12 iterations: runs of 1 and of 4 (the pair loop drops its last spectrum, another step follows),
    the operators and D in between, one step in another mode, a set estimate, new data that keeps the estimate and new data that
    does not, iterate_until with check_every 1 (the relative rule decides at the second check: the frames it stops there keep that
    estimate, the others the third) and 3 (one check)."""
    t_rel, t_disc = thresholds if thresholds is not None else THRESHOLDS[(case['name'], mode)]
    return [
        ('set_measurement', 0), ('iterate', 1),
        ('forward',), ('adjoint',), ('divergence',),
        ('iterate', 4),
        ('mode', TOGGLE[mode]), ('iterate', 1),
        ('mode', mode), ('set_estimate',),
        ('keep_measurement', 1), ('until', 3, 1, sr.RELATIVE, t_rel),
        ('written' if case['written'] else 'set_measurement', 2), ('until', 3, 3, sr.DISCREPANCY, t_disc),
    ]


def set_mode(target, mode):
    acceleration, lam = MODES[mode]
    target.set_acceleration(acceleration)
    target.set_tv(lam, TV_EPSILON)


def run_model(model, d, op):
    """One call of the script on the model; returns what the call returns."""
    if op[0] == 'set_measurement':
        return model.set_measurement(d['meas'][op[1]])
    if op[0] == 'written':
        return model.measurement_written(d['meas'][op[1]])
    if op[0] == 'keep_measurement':
        keep = model.estimate()
        model.set_measurement(d['meas'][op[1]])
        return model.set_estimate(keep)
    if op[0] == 'iterate':
        return model.iterate(op[1])
    if op[0] == 'forward':
        return model.forward(d['obj'])
    if op[0] == 'adjoint':
        return model.adjoint(d['meas'][0])
    if op[0] == 'divergence':
        return model.divergence()
    if op[0] == 'mode':
        return set_mode(model, op[1])
    if op[0] == 'set_estimate':
        return model.set_estimate(d['x'])
    if op[0] == 'until':
        return model.iterate_until(op[1], rule=op[3], threshold=op[4], check_every=op[2])
    raise ValueError(op)


def margins(info, rule, threshold, count, k_max, check_every):
    """The smallest relative distance from the threshold of the decisions an iterate_until run of the model took: every frame's,
    at every check up to the one it stopped at."""
    out = []
    trace = info['trace']
    for i in range(trace.shape[0]):
        done = min((i + 1) * check_every, k_max)
        for f in range(trace.shape[1]):
            if done > info['iterations'][f]:
                continue
            if rule == sr.DISCREPANCY:
                out.append(abs(2.0 * trace[i, f] / count - threshold) / abs(threshold))
            elif i > 0:
                out.append(abs((trace[i - 1, f] - trace[i, f]) / trace[i - 1, f] - threshold) / abs(threshold))
    return min(out) if out else np.inf


def _between(values):
    """A threshold that separates the values where there are several (the widest gap's geometric middle), else twice the value."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    if v.size < 2 or v[0] <= 0:
        return float(2.0 * v[-1])
    gaps = v[1:] / v[:-1]
    i = int(np.argmax(gaps))
    return float(np.sqrt(v[i] * v[i + 1]))


def run_reference(name, mode, round32=False, thresholds=None):
    """The whole sequence on the model alone.  Returns the model, its final estimate, the smallest margin of its iterate_until
    decisions and -- thresholds='choose' -- the thresholds chosen from the model's own traces."""
    case, d = BY_NAME[name], data(name, round32)
    choose = thresholds == 'choose'
    model = PlanModel(d['psfs'], case['B'], case['ny'], case['nx'])
    set_mode(model, mode)
    count = len(d['psfs']) * case['ny'] * case['nx']
    margin, chosen, finite = np.inf, [], True
    for op in script(case, mode, (1.0, 1.0) if choose else thresholds):
        if op[0] == 'until' and choose:                    # a dry run on a copy of the state finds the values the rule will see
            import copy
            dry = copy.deepcopy(model).iterate_until(op[1], rule=op[3], threshold=-1.0, check_every=op[2])
            tr = dry['trace']
            vals = 2.0 * tr[-1] / count if op[3] == sr.DISCREPANCY else (tr[0] - tr[1]) / tr[0]
            op = op[:4] + (_between(vals),)
            chosen.append(op[4])
        out = run_model(model, d, op)
        if op[0] == 'until':
            margin = min(margin, margins(out, op[3], op[4], count, op[1], op[2]))
        if model.est is not None:
            finite = finite and bool(np.all(np.isfinite(model.est)))
    return {'model': model, 'estimate': model.estimate(), 'margin': margin, 'thresholds': tuple(chosen), 'finite': finite}


def admit(name, mode):
    """The figures of the admission conditions: {'finite', 'min_ratio', 'sensitivity', 'margin'}."""
    ref = run_reference(name, mode)
    ref32 = run_reference(name, mode, round32=True)
    return {'finite': ref['finite'] and ref['model'].d.finite, 'min_ratio': ref['model'].d.min_ratio,
            'sensitivity': max_rel(ref32['estimate'], ref['estimate']), 'margin': ref['margin']}


def admitted(fig):
    return (fig['finite'] and fig['min_ratio'] >= MIN_PREDICTION_RATIO and fig['sensitivity'] <= F32_SENSITIVITY and
            fig['margin'] >= THRESHOLD_MARGIN)


if __name__ == '__main__':      # writes THRESHOLDS and shows every case's admission figures
    table = {}
    for c in CASES:
        for mode in MODES:
            table[(c['name'], mode)] = run_reference(c['name'], mode, thresholds='choose')['thresholds']
    THRESHOLDS.update(table)
    print('THRESHOLDS = {')
    for k, v in table.items():
        print('    %r: (%r, %r),' % (k, float('%.6g' % v[0]), float('%.6g' % v[1])))
    print('}')
    THRESHOLDS.update({k: (float('%.6g' % v[0]), float('%.6g' % v[1])) for k, v in table.items()})
    for c in CASES:
        for mode in MODES:
            fig = admit(c['name'], mode)
            print('%-16s %-5s %s min_ratio %.2e sensitivity %.2e margin %.2e' % (
                c['name'], mode, 'ok  ' if admitted(fig) else 'FAIL', fig['min_ratio'], fig['sensitivity'], fig['margin']))
