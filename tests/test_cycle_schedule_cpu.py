"""The streams and events of a run over the batch's slices (csrc/cycle_schedule.hpp cycle_schedule) and the slice size
(chunk_frames), run on the CPU through a stand-alone program (tests/emu/cycle_schedule_test.cpp, built with the address and
undefined-behaviour sanitizers).  rlsted.cpp run_slices enqueues the operation list as it stands, so what holds for the list holds
for the device.

The list of a CHAIN of cycles -- all but the last with cycle_follows, each fed the state the one before returned -- is replayed
into a happens-before model: an operation comes after the one in front of it on its stream, and a WAIT comes after the RECORD its
event held when the WAIT was enqueued (the last one in front of it in the list: what hipStreamWaitEvent captures; a WAIT for an
event never recorded waits for nothing).  On that model, with no tolerance:

  * no data hazard: two WORK operations that touch the same region, one of them writing, are ordered (REGIONS below);
  * fork and join: a cycle that forks has every operation behind the fork point; when the chain ends, or a cycle does not keep its
    lanes open, everything enqueued so far is in front of the end of the context's stream;
  * throttle: a draw ahead for lane l waits for the begun event of the slice in front of it on lane l, so it is behind every
    earlier loop of that lane: never more than one draw per lane ahead of the lane's loops;
  * the counts tests/test_gpu_draw_ahead.py asserts on the device.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'emu', 'cycle_schedule_test.cpp')
CTX = -1


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('cycle_schedule') / 'cycle_schedule_test')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', SRC, '-o', exe])
    return exe


def run(prog, text):
    out = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout.split('\n')


# ---- chains
def chain_text(B, cf, lanes, nrep, cycles, V=1, draws=True, share=None, classes=None, ahead=True):
    """share / classes default to what a plan would hold for these nrep: a layout exists when any slice shares."""
    assert len(nrep) == -(-B // cf)
    share = any(nrep) if share is None else share
    classes = (max(nrep) if share else 0) if classes is None else classes
    return 'chain %d %d %d %d %d %d %d %d %d\n%s\n' % (B, cf, lanes, V, draws, share, classes, ahead, cycles, ' '.join(map(str, nrep)))


def parse_chains(lines):
    """[[cycle, ...], ...]: a chain per 'chain' case; cycle = dict(head fields, ops=[tuple], state=[9 flags])"""
    cycles, i = [], 0
    while i < len(lines):
        w = lines[i].split()
        i += 1
        if not w:
            continue
        assert w[0] == 'cycle', w
        slices, lanes, forks, joins, shared, ahead, sim, n = map(int, w[1:])
        ops = []
        for line in lines[i:i + n]:
            t = line.split()
            if t[0] == 'WORK':
                ops.append(('WORK', int(t[1]), t[2], int(t[3]), bool(int(t[4]))))            # stream, kind, slice, shared
            else:
                ops.append((t[0], int(t[1]), (t[2], int(t[3])), bool(int(t[4]))))            # stream, (event, lane), join
        i += n
        st = lines[i].split()
        assert st[0] == 'state' and len(st) == 10
        i += 1
        cycles.append(dict(slices=slices, lanes=lanes, forks=bool(forks), joins=bool(joins), shared_slices=shared, draws_ahead=ahead,
                           sim_images=sim, ops=ops, lanes_open=bool(int(st[1])), begun=[int(x) for x in st[2:6]],
                           drawn=[int(x) for x in st[6:10]]))
    return cycles


def one_chain(prog, *a, **kw):
    return parse_chains(run(prog, chain_text(*a, **kw)))


# What a WORK operation reads and writes (cycle_schedule.hpp WorkKind):
#   rates        the class rates and the class simulation's spectrum space
#   noiseless s  the slice's rates             spec s   the slice's spectrum space
#   meas s       the slice's measurement       est s    its estimate          ws s   its Poisson work list
def regions(kind, s, shared):
    if kind == 'CLASS_SIM':
        return [('rates', True)]
    if kind == 'SIMULATE_SLICE':
        return [(('noiseless', s), True), (('spec', s), True)]
    if kind == 'DRAW_IN_LANE':
        return [('rates' if shared else ('noiseless', s), False), (('meas', s), True), (('ws', s), True)]
    if kind == 'DRAW_AHEAD':
        assert shared
        return [('rates', False), (('meas', s), True)]
    assert kind == 'LOOP', kind
    return [(('meas', s), False), (('spec', s), True), (('est', s), True)]


class Replay:
    """Happens-before over the operations of a chain: before[i] = bit set of the operations that come before operation i."""

    def __init__(self):
        self.ops, self.before, self.cycle_of = [], [], []
        self.last_on, self.recorded, self.captured = {}, {}, {}

    def add(self, op, cycle):
        i, b = len(self.ops), 0
        stream = op[1]
        if stream in self.last_on:
            p = self.last_on[stream]
            b |= self.before[p] | 1 << p
        if op[0] == 'WAIT' and op[2] in self.recorded:
            p = self.recorded[op[2]]
            self.captured[i] = p
            b |= self.before[p] | 1 << p
        if op[0] == 'RECORD':
            self.recorded[op[2]] = i
        self.last_on[stream] = i
        self.ops.append(op)
        self.before.append(b)
        self.cycle_of.append(cycle)
        return i

    def ordered(self, i, j):
        return bool(self.before[j] >> i & 1)


def check_chain(cycles, B, cf, lanes, nrep, ahead_switch=True, draws=True):
    """Every assertion of the module's docstring on one chain; returns the replay."""
    r = Replay()
    slices = -(-B // cf)
    nl = min(slices, lanes)
    touched = {}
    lane_loops = {}         # lane -> [(node of the BEGUN record or None, node of the LOOP, slice)] in stream order
    for c, cyc in enumerate(cycles):
        assert cyc['slices'] == slices and cyc['lanes'] == nl
        first = len(r.ops)
        begun_node = {}
        for n, op in enumerate(cyc['ops']):
            i = r.add(op, c)
            if op[0] == 'RECORD' and op[2][0] == 'BEGUN':
                begun_node[op[1]] = i
            if op[0] != 'WORK':
                continue
            _, stream, kind, s, shared = op
            assert stream == CTX if kind == 'DRAW_AHEAD' else kind == 'CLASS_SIM' or stream == (s % nl if nl > 1 else CTX)
            if kind == 'LOOP':
                lane_loops.setdefault(stream, []).append((begun_node.pop(stream, None), i, s))
            if kind == 'DRAW_AHEAD':
                # ---- throttle
                lane = s % nl
                wait = i - 1
                assert r.ops[wait][:3] == ('WAIT', CTX, ('BEGUN', lane)) and wait in r.captured
                in_front = lane_loops[lane][-1]
                assert r.captured[wait] == in_front[0], 'the draw waits for the begun event of the slice in front'
                assert in_front[2] == (s - nl if s >= nl else slices - 1 - (slices - 1 - lane) % nl)
                for _, loop, _ in lane_loops[lane][:-1]:
                    assert r.ordered(loop, i), 'a draw more than one slice ahead of its lane'
                # (the lane takes the draw before it begins the slice)
                assert [o[:3] for o in cyc['ops'][n + 1:n + 3]] == [('RECORD', CTX, ('DRAWN_AHEAD', lane)), ('WAIT', lane, ('DRAWN_AHEAD', lane))]
            # ---- no data hazard
            for region, writes in regions(kind, s, shared):
                for j, other_writes in touched.setdefault(region, []):
                    if writes or other_writes:
                        assert r.ordered(j, i), 'hazard on %s: cycle %d %s against cycle %d %s' % (
                            region, r.cycle_of[j], r.ops[j], c, op)
                touched[region].append((i, writes))
        # ---- fork and join
        if cyc['forks']:
            assert cyc['ops'][0][:3] == ('RECORD', CTX, ('FORK', 0))
            for i in range(first + 1, len(r.ops)):
                assert r.ordered(first, i), 'operation %s is not behind the fork' % (r.ops[i],)
        assert cyc['forks'] == (nl > 1 and (c == 0 or not cycles[c - 1]['lanes_open']))
        assert cyc['joins'] == (nl > 1 and c + 1 == len(cycles)) and cyc['lanes_open'] == (nl > 1 and c + 1 < len(cycles))
        assert [op[3] for op in cyc['ops'] if op[0] != 'WORK'].count(True) == (2 * nl if cyc['joins'] else 0)
        if not cyc['lanes_open']:
            end = r.add(('END', CTX), c)
            assert r.before[end] == (1 << end) - 1, 'operations that the context\'s stream does not wait for'
        # ---- counts
        kinds = [op[2] for op in cyc['ops'] if op[0] == 'WORK']
        sharing = [s for s in range(slices) if nrep[s] > 0] if draws and any(nrep) else []
        assert kinds.count('LOOP') == slices and kinds.count('CLASS_SIM') == (1 if sharing else 0)
        assert kinds.count('DRAW_AHEAD') == cyc['draws_ahead'] and (ahead_switch or cyc['draws_ahead'] == 0)
        assert kinds.count('DRAW_AHEAD') + kinds.count('DRAW_IN_LANE') == (slices if draws else 0)
        assert cyc['shared_slices'] == len(sharing) and kinds.count('SIMULATE_SLICE') == (slices - len(sharing) if draws else 0)
    return r


def ahead_slices(cyc):
    return [op[3] for op in cyc['ops'] if op[0] == 'WORK' and op[2] == 'DRAW_AHEAD']


# lanes, B, cf, nrep per slice, draws ahead of a lone cycle, of a cycle that follows another: tests/test_gpu_draw_ahead.py
DEVICE_CASES = {
    'two lanes, six sharing slices': (2, 12, 2, [1] * 6, 4, 6),
    'three lanes, seven slices': (3, 14, 2, [1] * 7, 4, 7),
    'three lanes, four slices': (3, 8, 2, [1] * 4, 1, 2),
    'two lanes, two slices': (2, 4, 2, [1] * 2, 0, 0),
    'one lane, six slices': (1, 12, 2, [1] * 6, 0, 0),
    'sharing and per-frame slices alternate': (2, 24, 4, [1, 0, 1, 1, 0, 1], 3, 4),
}


@pytest.mark.parametrize('case', sorted(DEVICE_CASES))
def test_draws_ahead_as_the_device_tests_count_them(prog, case):
    lanes, B, cf, nrep, lone, chained = DEVICE_CASES[case]
    for cycles in (1, 2, 3):
        got = one_chain(prog, B, cf, lanes, nrep, cycles)
        check_chain(got, B, cf, lanes, nrep)
        assert [c['draws_ahead'] for c in got] == [lone] + [chained] * (cycles - 1)
        off = one_chain(prog, B, cf, lanes, nrep, cycles, ahead=False)
        check_chain(off, B, cf, lanes, nrep, ahead_switch=False)
        assert [c['draws_ahead'] for c in off] == [0] * cycles
        assert [c['shared_slices'] for c in off] == [c['shared_slices'] for c in got] == [sum(n > 0 for n in nrep)] * cycles
    if case == 'sharing and per-frame slices alternate':
        lone_cycle, = one_chain(prog, B, cf, lanes, nrep, 1)
        assert ahead_slices(lone_cycle) == [2, 3, 5]
        assert ahead_slices(one_chain(prog, B, cf, lanes, nrep, 2)[1]) == [0, 2, 3, 5]


def test_shared_slices_and_simulated_images(prog):
    """Six sharing two-frame slices, two classes, one view: 6 and 2 (test_two_lanes_three_slices_each); with slices that do not share
    the images are the classes' plus every frame's of those slices, times the views."""
    for ahead in (False, True):
        for cyc in one_chain(prog, 12, 2, 2, [1] * 6, 2, classes=2, ahead=ahead):
            assert (cyc['shared_slices'], cyc['sim_images']) == (6, 2)
        for cyc in one_chain(prog, 22, 4, 2, [1, 0, 1, 1, 0, 1], 2, V=3, classes=2, ahead=ahead):     # (a short last slice of two frames)
            assert (cyc['shared_slices'], cyc['sim_images']) == (4, (2 + 2 * 4) * 3)
    cyc, = one_chain(prog, 12, 2, 2, [0] * 6, 1, V=2)
    assert (cyc['shared_slices'], cyc['sim_images'], cyc['draws_ahead']) == (0, 24, 0)
    cyc, = one_chain(prog, 12, 2, 2, [1] * 6, 1, draws=False)          # rl_deconv_iterate: nothing is simulated or drawn
    assert (cyc['shared_slices'], cyc['sim_images'], cyc['draws_ahead']) == (0, 0, 0)
    assert [op[2] for op in cyc['ops'] if op[0] == 'WORK'] == ['LOOP'] * 6


def test_the_next_class_simulation_waits_for_every_lanes_last_shared_draw(prog):
    """The orderings that were comments: across cycles whose lanes stay open the class simulation comes after every draw from the
    rates it replaces, and a draw ahead of slice s after the loop that last read the measurement of s."""
    for ahead in (False, True):
        got = one_chain(prog, 12, 2, 2, [1] * 6, 3, ahead=ahead)
        r = check_chain(got, 12, 2, 2, [1] * 6, ahead_switch=ahead)
        work = [(i, op, r.cycle_of[i]) for i, op in enumerate(r.ops) if op[0] == 'WORK']
        for i, op, c in work:
            if op[2] == 'CLASS_SIM':
                assert all(r.ordered(j, i) for j, o, cj in work if cj < c and o[2].startswith('DRAW'))
            if op[2] == 'DRAW_AHEAD':
                assert all(r.ordered(j, i) for j, o, cj in work if cj < c and o[2] == 'LOOP' and o[3] == op[3])


def test_a_lane_that_holds_one_slice_keeps_its_in_lane_draw(prog):
    got = one_chain(prog, 8, 2, 3, [1] * 4, 3)                     # lanes of 2, 1 and 1 slices
    assert [ahead_slices(c) for c in got] == [[3], [0, 3], [0, 3]]


def test_random_chains(prog):
    rng = np.random.default_rng(20)
    cases = []
    for n in range(400):
        B = int(rng.integers(1, 49))
        cf = int(rng.integers(1, B + 1))
        slices = -(-B // cf)
        kind = n % 4                                                  # none sharing, all sharing, two random mixes
        nrep = [0] * slices if kind == 0 else [1] * slices if kind == 1 else [int(x) for x in rng.integers(0, 3, slices)]
        cases.append(dict(B=B, cf=cf, lanes=int(rng.integers(1, 5)), nrep=nrep, cycles=int(rng.integers(1, 5)),
                          V=int(rng.integers(1, 4)), draws=bool(rng.random() < 0.85), ahead=bool(rng.integers(0, 2))))
    text = ''.join(chain_text(c['B'], c['cf'], c['lanes'], c['nrep'], c['cycles'], V=c['V'], draws=c['draws'], ahead=c['ahead'])
                   for c in cases)
    got = parse_chains(run(prog, text))
    assert len(got) == sum(c['cycles'] for c in cases)
    seen_ahead = 0
    for c in cases:
        mine, got = got[:c['cycles']], got[c['cycles']:]
        check_chain(mine, c['B'], c['cf'], c['lanes'], c['nrep'], ahead_switch=c['ahead'], draws=c['draws'])
        seen_ahead += sum(cyc['draws_ahead'] for cyc in mine)
        for cyc in mine:
            classes = max(c['nrep']) if any(c['nrep']) else 0
            frames = sum(min(c['cf'], c['B'] - s * c['cf']) for s in range(cyc['slices']) if not (any(c['nrep']) and c['nrep'][s]))
            assert cyc['sim_images'] == ((classes + frames) * c['V'] if c['draws'] else 0)
    assert seen_ahead > 100                                           # (the sweep does reach the draws ahead)


# ---- chunk_frames
def ceil_div(a, b):
    return -(-a // b)


def chunk_ref(B, V, n_img, n_spec, esize, one_buffer, accel, tv, pair, mb, lanes, col_tile, kx):
    """The rule of cycle_schedule.hpp chunk_frames, restated.  mb: RLSTED_CHUNK_MB or None."""
    MB = 1048576.0
    per_frame = ((1 if one_buffer else 1 + V) * 2.0 * n_spec + (1 + V + 3 * accel + tv) * n_img) * esize
    if mb is not None:
        c = int(mb * MB / per_frame)
    else:
        budget = 1024.0 if per_frame >= 32 * MB else 108.0 if lanes > 1 else 288.0     # large frames only fill the chip
        c = int(budget * MB / per_frame)
        if c < 8 and per_frame * 8 <= 300 * MB:
            c = 8
        if V > 1:
            tiles = ceil_div(kx, col_tile)
            need = ceil_div(ceil_div(512, tiles), 8) * 8                                # 512 column tiles, in groups of 8 frames
            if c < need and per_frame * need <= 300 * MB:
                c = need
    c = max(c, 1)
    if c >= B:
        return B
    fit = c
    c = ceil_div(B, ceil_div(B, c))                                                     # equal slices
    if c > 8:
        up = ceil_div(c, 8) * 8
        c = up if up <= fit else max(8, fit // 8 * 8)
    if pair and c % 2:
        c += 1
    return min(c, B)


def chunk_text(B, V, n_img, n_spec, esize, one_buffer, accel, tv, pair, mb, lanes, col_tile, kx):
    return 'chunk %d %d %d %d %d %d %d %d %d %d %r %d %d %d\n' % (B, V, n_img, n_spec, esize, one_buffer, accel, tv, pair, mb is not None,
                                                                  float(mb or 0), lanes, col_tile, kx)


def chunk(prog, *a):
    line = run(prog, chunk_text(*a))[0].split()
    assert line[0] == 'chunk' and int(line[1]) == chunk_ref(*a)
    return int(line[1])


def plan_numbers(n, L, dtype, V):
    """n_img, n_spec, esize, one_buffer, kx of an n x n plan that transforms at length L (rlsted.cpp deconv_build)"""
    kx = L // 2 + 1
    pitch = -(-kx // 8) * 8
    return n * n, n * pitch, 4 if dtype == 'f32' else 8, V == 1, kx


def test_budgets_of_the_device_tests_give_two_frame_slices(prog):
    """SHAPES of tests/test_gpu_draw_ahead.py, twelve frames on two lanes: 128^2 with a 9 x 9 PSF transforms at L = 192, 200^2 at
    L = 256.  The budgets hold 2.65, 2.65 and 2.24 frames; the pair plan's holds none, and its slice of one frame becomes a pair."""
    for mb, n, L, dtype, V, pair, frames in (('0.6', 128, 192, 'f32', 1, False, 2.65), ('1.2', 128, 192, 'f64', 1, False, 2.65),
                                             ('2.2', 128, 192, 'f64', 2, False, 2.24), ('0.001', 200, 256, 'f32', 1, True, 0.0)):
        n_img, n_spec, esize, one_buffer, kx = plan_numbers(n, L, dtype, V)
        per_frame = ((1 if one_buffer else 1 + V) * 2 * n_spec + (1 + V) * n_img) * esize
        assert abs(float(mb) * 1048576 / per_frame - frames) < 0.01
        assert chunk(prog, 12, V, n_img, n_spec, esize, one_buffer, False, False, pair, float(mb), 2, 8, kx) == 2
    # test_sharing_and_per_frame_slices_alternate: '2.0' on the f64 single-view plan, 24 frames -> slices of four
    n_img, n_spec, esize, one_buffer, kx = plan_numbers(128, 192, 'f64', 1)
    assert chunk(prog, 24, 1, n_img, n_spec, esize, one_buffer, False, False, False, 2.0, 2, 8, kx) == 4


def test_rules_without_a_budget_at_the_headline_shape(prog):
    """512^2 (L = 576), one view, f32, 1024 frames.  A frame's working set is one spectrum and two images, 3.16 MB: 108 MB hold 34
    frames; 1024 frames are 31 slices of 34, cut back to whole groups of eight: 32 frames, an even count for the pair loop."""
    n_img, n_spec, esize, one_buffer, kx = plan_numbers(512, 576, 'f32', 1)
    assert (2 * n_spec + 2 * n_img) * esize == 3309568 and int(108 * 1048576 / 3309568) == 34
    assert chunk(prog, 1024, 1, n_img, n_spec, esize, one_buffer, False, False, True, None, 2, 8, kx) == 32
    # one lane: 288 MB hold 91 frames; 12 slices of 86 -> 88
    assert chunk(prog, 1024, 1, n_img, n_spec, esize, one_buffer, False, False, True, None, 1, 8, kx) == 88
    # the accelerated loop keeps three more images per frame, RL-TV one, 7.16 MB: 15 frames fit, and 69 slices of 15 are cut back to 8
    assert chunk(prog, 1024, 1, n_img, n_spec, esize, one_buffer, True, True, True, None, 2, 8, kx) == 8
    # four views, five spectra and five images per frame, 10.8 MB: the budget holds 10; the column launches ask for 512 tiles --
    # 37 per frame (kx = 289 in tiles of 8), so 14 -> 16 frames, 172 MB
    n_img, n_spec, esize, one_buffer, kx = plan_numbers(512, 576, 'f32', 4)
    assert -(-kx // 8) == 37
    assert chunk(prog, 1024, 4, n_img, n_spec, esize, one_buffer, False, False, False, None, 2, 8, kx) == 16
    # 2048^2 (L = 2304), 50.1 MB per frame: frames of 32 MB and more get ~1 GB slices, 20 frames, cut back to 16
    n_img, n_spec, esize, one_buffer, kx = plan_numbers(2048, 2304, 'f32', 1)
    assert (2 * n_spec + 2 * n_img) * esize >= 32 * 1048576
    assert chunk(prog, 1024, 1, n_img, n_spec, esize, one_buffer, False, False, False, None, 2, 8, kx) == 16
    # a batch that fits one slice
    assert chunk(prog, 16, 1, n_img, n_spec, esize, one_buffer, False, False, False, None, 2, 8, kx) == 16


def test_random_plans_match_the_rule(prog):
    rng = np.random.default_rng(3)
    cases = []
    for _ in range(300):
        n, V = int(rng.choice([64, 100, 128, 200, 512, 1000, 2048])), int(rng.integers(1, 9))
        L = next(x for x in (64, 192, 256, 576, 1152, 2304) if x >= n + 4)
        n_img, n_spec, esize, one_buffer, kx = plan_numbers(n, L, str(rng.choice(['f32', 'f64'])), V)
        mb = None if rng.random() < 0.5 else float(rng.choice([0.001, 0.6, 2.2, 20.0, 108.0, 500.0]))
        cases.append((int(rng.integers(1, 1500)), V, n_img, n_spec, esize, one_buffer and bool(rng.integers(0, 2)), bool(rng.integers(0, 2)),
                      bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), mb, int(rng.integers(1, 5)), int(rng.choice([4, 8, 16])), kx))
    lines = run(prog, ''.join(chunk_text(*c) for c in cases))
    assert [int(line.split()[1]) for line in lines[:len(cases)]] == [chunk_ref(*c) for c in cases]
