"""The workspace layout of the C-ABI host calls (csrc/work_layout.hpp: Region, WorkLayout) on the CPU, through a stand-alone program
(tests/emu/work_layout_test.cpp, built with the address and undefined-behaviour sanitizers).  Every call of the ABI takes the size
of its device workspace from WorkLayout::bytes() and every pointer into it from Region::at(), so what holds here holds for them:

  * every region starts on a 256-byte boundary, regions are disjoint and in declaration order, bytes() is the end of the last
    reservation, at() is null exactly for an empty region -- for element sizes 1, 4, 8 and 12, counts from 0 on, 1 and 3 copies;
  * a block of exactly bytes() holds every region over its full copies x count extent (the sanitizer watches every store);
  * a block one byte shorter does not: the sanitizer ends that run, which shows that it would have seen a region too many.
"""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'emu', 'work_layout_test.cpp')


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('work_layout') / 'work_layout_test')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', SRC, '-o', exe])
    return exe


def test_regions_are_aligned_disjoint_and_fit_the_block(prog):
    out = subprocess.run([prog], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    head, sequences, regions = out.stdout.split()
    assert head == 'ok' and int(sequences) == 6 and int(regions) == 25


def test_a_block_one_byte_short_is_reported(prog):
    out = subprocess.run([prog, 'short'], capture_output=True, text=True)
    assert out.returncode != 0, out.stdout
    assert 'heap-buffer-overflow' in out.stderr and 'unreported' not in out.stdout
