"""Which frames of a batch carry the same object (csrc/object_classes.hpp): the classifier and the slices' representative lists,
run on the CPU through a stand-alone program (tests/emu/object_classes_test.cpp, built with the address and undefined-behaviour
sanitizers) and compared with a few lines of Python that state the rule:

  * frames are compared, in order, with the first `max_reps` frames that started a class; a frame that matches none starts a
    class of its own, which later frames can join only while the list has room;
  * "the same" is the same pixel bits and the same brightness bits;
  * per slice of cf frames the first frame of each class within the slice simulates for the others, if those representatives are
    at most half the slice's frames.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'emu', 'object_classes_test.cpp')


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('object_classes') / 'object_classes_test')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', SRC, '-o', exe])
    return exe


def bits(x):
    return struct.pack('<d', float(x))


def classify_ref(keys, max_reps):
    """keys[f]: everything that must be the same bits for two frames to be one class."""
    cls, reps = [], []
    for f, key in enumerate(keys):
        c = next((cls[g] for g in reps if keys[g] == key), None)
        if c is None:
            c = max(cls, default=-1) + 1
            if len(reps) < max_reps:
                reps.append(f)
        cls.append(c)
    return cls


def layout_ref(cls, cf):
    slices, reps, rate = [], [], [0] * len(cls)
    for f0 in range(0, len(cls), cf):
        part = cls[f0:f0 + cf]
        first = {}
        for i, c in enumerate(part):
            first.setdefault(c, f0 + i)
        if 2 * len(first) <= len(part):
            c0 = len(reps)
            order = list(first)
            slices.append((c0, len(order)))
            reps += [first[c] for c in order]
            for i, c in enumerate(part):
                rate[f0 + i] = c0 + order.index(c)
        else:
            slices.append((0, 0))
    return slices, reps, rate


def run(prog, text):
    out = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [[int(x) for x in line.split()] for line in out.stdout.strip().split('\n')]
    assert len(rows) == 4
    cls, flat, reps, rate = (r[1:] for r in rows)
    assert rows[2][0] == len(reps) == rows[1][0] and rows[3][0] == len(rate)
    return rows[0][0], cls, list(zip(flat[0::2], flat[1::2])), reps, rate


def fmt(v):
    return ' '.join(repr(float(x)) for x in np.asarray(v, dtype=np.float64).ravel())


def by_pixels(prog, frames, brightness=None, max_reps=8, cf=None):
    frames = np.asarray(frames, dtype=np.float64)
    B, n = frames.shape
    cf = cf or B
    text = 'pixels %d %d %d %d %d\n%s\n' % (B, n, max_reps, cf, brightness is not None, fmt(frames))
    if brightness is not None:
        text += fmt(brightness) + '\n'
    got = run(prog, text)
    keys = [(frames[f].tobytes(), bits(brightness[f]) if brightness is not None else b'') for f in range(B)]
    cls = classify_ref(keys, max_reps)
    assert got[0] == max(cls) + 1 and got[1] == cls
    assert got[2:] == layout_ref(cls, cf)
    return got


A, B_, C = [1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [0.0, 2.0, 3.0]


def test_all_frames_equal(prog):
    classes, cls, slices, reps, rate = by_pixels(prog, [A] * 12, cf=4)
    assert classes == 1 and cls == [0] * 12
    assert slices == [(0, 1), (1, 1), (2, 1)] and reps == [0, 4, 8]       # one representative per slice: slices do not depend on each other
    assert rate == [0] * 4 + [1] * 4 + [2] * 4


def test_all_frames_distinct(prog):
    frames = np.arange(30, dtype=np.float64).reshape(10, 3)
    classes, cls, slices, reps, rate = by_pixels(prog, frames, cf=5)
    assert classes == 10 and cls == list(range(10))
    assert slices == [(0, 0), (0, 0)] and reps == [] and rate == [0] * 10   # nothing is shared


def test_pattern_a_a_b_a_b_c(prog):
    classes, cls, slices, reps, rate = by_pixels(prog, [A, A, B_, A, B_, C])
    assert classes == 3 and cls == [0, 0, 1, 0, 1, 2]
    assert slices == [(0, 3)] and reps == [0, 2, 5] and rate == [0, 0, 1, 0, 1, 2]          # 3 of 6: at most half, shared


def test_slice_rule_is_at_most_half(prog):
    assert by_pixels(prog, [A, A, B_, A, B_, C], cf=3)[2] == [(0, 0), (0, 0)]        # A A B: 2 of 3; A B C: 3 of 3
    # 2 representatives in 3 frames: not shared; 2 in 4: shared; a single frame: never
    assert by_pixels(prog, [A, A, B_], cf=3)[2] == [(0, 0)]
    assert by_pixels(prog, [A, A, B_, B_], cf=4)[2] == [(0, 2)]
    assert by_pixels(prog, [A], cf=1)[2] == [(0, 0)]
    # a class that spans two slices has a representative in each; a short last slice is judged on its own frames
    classes, cls, slices, reps, rate = by_pixels(prog, [A, A, A, B_, B_, B_, B_, A, A], cf=4)
    assert slices == [(0, 2), (2, 2), (0, 0)] and reps == [0, 3, 4, 7] and rate == [0, 0, 0, 1, 2, 2, 2, 3, 0]


def test_equal_pixels_differing_brightness(prog):
    classes, cls, _, _, _ = by_pixels(prog, [A] * 4, brightness=[5e10, 5e10, 6e10, 5e10])
    assert classes == 2 and cls == [0, 0, 1, 0]
    # the same BITS: +0 and -0 differ, two nans of one pattern do not; without a brightness only the pixels count
    assert by_pixels(prog, [A] * 3, brightness=[0.0, -0.0, 0.0])[1] == [0, 1, 0]
    assert by_pixels(prog, [A] * 2, brightness=[float('nan')] * 2)[1] == [0, 0]
    assert by_pixels(prog, [A] * 3)[1] == [0, 0, 0]
    # pixels: -0.0 is not 0.0 either (the classes are about bits, so that a member's scaled object IS its representative's)
    assert by_pixels(prog, [[0.0, 1.0], [-0.0, 1.0]])[1] == [0, 1]


def test_more_than_eight_classes(prog):
    frames = np.repeat(np.arange(12, dtype=np.float64), 2).reshape(12, 2)          # 12 distinct objects ...
    order = list(range(12)) + list(range(12))                                      # ... each twice
    classes, cls, _, _, _ = by_pixels(prog, frames[order])
    # the first 8 are representatives and find their second copy; objects 8..11 do not: each copy is a class of its own
    assert cls[:12] == list(range(12)) and cls[12:20] == list(range(8)) and cls[20:] == [12, 13, 14, 15] and classes == 16
    assert by_pixels(prog, frames[order], max_reps=2)[0] == 2 + 10 + 10


def test_single_frame(prog):
    classes, cls, slices, reps, rate = by_pixels(prog, [A])
    assert (classes, cls, slices, reps, rate) == (1, [0], [(0, 0)], [], [0])


def test_classes_by_object_index(prog):
    """rl_batch_submit's form: the staged object's index and the task's brightness."""
    idx, tb = [0, 0, 1, 0, 1, 2, 0, 0], [1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 2.0]
    for brightness in (tb, None):
        text = 'index %d %d %d %d\n%s\n' % (len(idx), 8, 4, brightness is not None, ' '.join(map(str, idx)))
        if brightness is not None:
            text += fmt(brightness) + '\n'
        got = run(prog, text)
        cls = classify_ref([(i, bits(t) if brightness is not None else b'') for i, t in zip(idx, tb)], 8)
        assert got[1] == cls and got[2:] == layout_ref(cls, 4)
    assert cls == [0, 0, 1, 0, 1, 2, 0, 0]


def test_random_batches_match_the_rule(prog):
    rng = np.random.default_rng(5)
    for _ in range(40):
        B, kinds = int(rng.integers(1, 40)), int(rng.integers(1, 14))
        pool = rng.integers(0, 3, (kinds, 4)).astype(np.float64)
        frames = pool[rng.integers(0, kinds, B)]
        tb = rng.choice([1.0, 2.0], B) if rng.random() < 0.5 else None
        by_pixels(prog, frames, brightness=tb, max_reps=int(rng.integers(1, 10)), cf=int(rng.integers(1, B + 1)))
