"""One compact image per object class and cycle (csrc/object_classes.hpp class_layout), run on the CPU through a stand-alone program
(tests/emu/class_layout_test.cpp, built with the address and undefined-behaviour sanitizers) and compared with a few lines of
Python that state the rule:

  * which slices share is share_layout's decision and stays: the distinct classes of a slice are at most half its frames;
  * the compact classes are the classes that a sharing slice holds, numbered in order of first appearance in such a slice, and
    the frame of that first appearance carries the class's object;
  * every frame of a sharing slice reads its class's compact image; frames of the other slices read nothing (0).
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'emu', 'class_layout_test.cpp')


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('class_layout') / 'class_layout_test')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', SRC, '-o', exe])
    return exe


def layout_ref(cls, cf):
    nrep, reps, rate, compact = [], [], [0] * len(cls), {}
    for f0 in range(0, len(cls), cf):
        part = cls[f0:f0 + cf]
        kinds = len(set(part))
        if 2 * kinds > len(part):
            nrep.append(0)
            continue
        nrep.append(kinds)
        for i, c in enumerate(part):
            if c not in compact:
                compact[c] = len(reps)
                reps.append(f0 + i)
            rate[f0 + i] = compact[c]
    return nrep, reps, rate


def run(prog, cls, cf):
    text = '%d %d\n%s\n' % (len(cls), cf, ' '.join(map(str, cls)))
    out = subprocess.run([prog], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [[int(x) for x in line.split()] for line in out.stdout.strip().split('\n')]
    assert len(rows) == 3
    nrep, reps, rate = (r[1:] for r in rows)
    assert rows[0][0] == rows[1][0] == len(reps) and rows[2][0] == len(rate) == len(cls)
    assert (nrep, reps, rate) == layout_ref(list(cls), cf)
    return nrep, reps, rate


def test_one_class_in_every_slice_is_one_image(prog):
    nrep, reps, rate = run(prog, [0] * 12, 4)
    assert nrep == [1, 1, 1] and reps == [0] and rate == [0] * 12       # (share_layout alone: a representative per slice)


def test_classes_that_span_slices(prog):
    # A A A B | B B B A | A : the short last slice is a single frame and does not share
    nrep, reps, rate = run(prog, [0, 0, 0, 1, 1, 1, 1, 0, 0], 4)
    assert nrep == [2, 2, 0] and reps == [0, 3] and rate == [0, 0, 0, 1, 1, 1, 1, 0, 0]
    # A A A A A A B B in slices of two
    nrep, reps, rate = run(prog, [0] * 6 + [1, 1], 2)
    assert nrep == [1, 1, 1, 1] and reps == [0, 6] and rate == [0] * 6 + [1, 1]


def test_slices_that_do_not_share_are_left_out(prog):
    # A B C D | A A A A | E E F F: class A's compact image comes from the second slice, B C D have none
    nrep, reps, rate = run(prog, [0, 1, 2, 3, 0, 0, 0, 0, 4, 4, 5, 5], 4)
    assert nrep == [0, 1, 2] and reps == [4, 8, 10] and rate == [0] * 8 + [1, 1, 2, 2]
    # nothing shares: no compact image at all
    assert run(prog, list(range(10)), 5) == ([0, 0], [], [0] * 10)
    assert run(prog, [0], 1) == ([0], [], [0])


def test_random_batches_match_the_rule(prog):
    rng = np.random.default_rng(7)
    for _ in range(60):
        B = int(rng.integers(1, 48))
        kinds = int(rng.integers(1, 10))
        raw = rng.integers(0, kinds, B)
        order = {}
        cls = [order.setdefault(int(c), len(order)) for c in raw]      # numbered in order of first appearance, as classify_frames does
        run(prog, cls, int(rng.integers(1, B + 1)))
