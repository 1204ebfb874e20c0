"""The switch table of a plan (csrc/plan_options.hpp: OptionLookup, PlanOptions, plan_options) on the CPU, through a stand-alone
program (tests/emu/plan_options_test.cpp, built with the address and undefined-behaviour sanitizers).  rl_deconv_create_with runs
the same three steps -- parse the text, fill the table, refuse a given name nobody asked for -- so what holds here holds for a plan.

  * the defaults INTEGRATION.md section 1 documents, for f32 and f64 plans of one and of several views;
  * the clamps: lanes 1 .. kMaxLanes (4), draw grid 1 .. kPoissonGrid (4096), column order >= 1, tile height 32 or 64 only;
  * precedence: the options text, then the environment, then the default;
  * what the text may not hold: an entry without '=', an empty name or value, a name twice, a name that is no switch of a plan --
    while the environment may hold any variable.
"""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'emu', 'plan_options_test.cpp')
KMAXLANES, KPOISSONGRID = 4, 4096


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('plan_options') / 'plan_options_test')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', SRC, '-o', exe])
    return exe


def plan(prog, dtype='f32', views=1, options='', env=None):
    """The table as {field: number}, or the error message as a str."""
    text = ''.join('env %s %s\n' % kv for kv in (env or {}).items()) + 'plan %s %d %s\n' % (dtype, views, options)
    clean = {k: v for k, v in os.environ.items() if not k.startswith('RLSTED_')}
    out = subprocess.run([prog], input=text, capture_output=True, text=True, env=clean)
    assert out.returncode == 0, out.stderr
    line, = out.stdout.splitlines()
    head, _, rest = line.partition(' ')
    if head == 'error':
        return rest
    assert head == 'ok'
    return {k: float(v) for k, v in (w.split('=') for w in rest.split())}


DEFAULTS = {'chunk_mb_set': 0, 'lanes': 2, 'draw_ahead': 0, 'draw_grid': 128, 'poisson_groups': 1, 'inplace': 1, 'col_order': 4,
            'pair_max_ratio': 4.0, 'fuse_views': -1, 'col_split': 1, 'real_psf': 1, 'ones_shortcut': 1, 'share_objects': 1, 'sep': 1,
            'sep_one': 1, 'direct': 1, 'sep_th': 32, 'q_exp_est_set': 0, 'q_exp_ratio_set': 0, 'q_exp_est': 14, 'q_exp_ratio': 14}


@pytest.mark.parametrize('dtype, views, pair, sub_one', [('f32', 1, 1, 1), ('f32', 4, 0, 1), ('f64', 1, 0, 0)])
def test_defaults_are_the_documented_ones(prog, dtype, views, pair, sub_one):
    """frame pairs on single-view f32 plans, `ratio - 1` on f32 plans, the view sum unset (-1: f32 on, f64
    off, decided in rl_deconv_create_with), the rest the same for every plan."""
    got = plan(prog, dtype, views)
    want = dict(DEFAULTS, pair=pair, sub_one=sub_one, chunk_mb=0)
    assert got == want


def test_clamps(prog):
    for given, want in (('0', 1), ('-3', 1), ('1', 1), ('3', 3), ('4', KMAXLANES), ('9', KMAXLANES)):
        assert plan(prog, options='RLSTED_LANES=' + given)['lanes'] == want
    for given, want in (('0', 1), ('-1', 1), ('7', 7), ('4096', KPOISSONGRID), ('100000', KPOISSONGRID)):
        assert plan(prog, options='RLSTED_DRAW_GRID=' + given)['draw_grid'] == want
    for given, want in (('0', 1), ('-5', 1), ('1', 1), ('64', 64)):
        assert plan(prog, options='RLSTED_COL_ORDER=' + given)['col_order'] == want
    for given, want in (('64', 64), ('32', 32), ('48', 32), ('128', 32), ('0', 32), ('640', 32)):
        assert plan(prog, options='RLSTED_SEP_TH=' + given)['sep_th'] == want
    assert plan(prog, 'f64', options='RLSTED_SEP_TH=64')['sep_th'] == 32            # f64 plans stay at 32
    assert plan(prog, 'f64', env={'RLSTED_SEP_TH': '64'})['sep_th'] == 32
    assert plan(prog, 'f32', 3, env={'RLSTED_SEP_TH': '64'})['sep_th'] == 64


def test_options_then_environment_then_default(prog):
    assert plan(prog)['lanes'] == 2
    assert plan(prog, env={'RLSTED_LANES': '3'})['lanes'] == 3
    assert plan(prog, options='RLSTED_LANES=1', env={'RLSTED_LANES': '3'})['lanes'] == 1
    got = plan(prog, options='RLSTED_PAIR=0\tRLSTED_CHUNK_MB=2.5  ', env={'RLSTED_PAIR': '1', 'RLSTED_SEP': '0', 'RLSTED_CHUNK_MB': '7'})
    assert (got['pair'], got['sep'], got['chunk_mb_set'], got['chunk_mb'], got['direct']) == (0, 0, 1, 2.5, 1)
    got = plan(prog, 'f64', 2, options='RLSTED_PAIR=1 RLSTED_SUB_ONE=1 RLSTED_FUSE_VIEWS=0 RLSTED_Q_EXP_EST=12 RLSTED_PAIR_MAX_RATIO=1e30')
    assert (got['pair'], got['sub_one'], got['fuse_views'], got['q_exp_est_set'], got['q_exp_est'], got['q_exp_ratio_set']) == (1, 1, 0, 1, 12, 0)
    assert got['pair_max_ratio'] == 1e30
    # every switch of the table at once, each away from its default: none is refused, each arrives
    every = {'RLSTED_CHUNK_MB': '3', 'RLSTED_LANES': '3', 'RLSTED_DRAW_AHEAD': '1', 'RLSTED_DRAW_GRID': '5', 'RLSTED_POISSON_GROUPS': '0',
             'RLSTED_INPLACE': '0', 'RLSTED_COL_ORDER': '2', 'RLSTED_PAIR': '0', 'RLSTED_PAIR_MAX_RATIO': '2', 'RLSTED_SUB_ONE': '0',
             'RLSTED_FUSE_VIEWS': '1', 'RLSTED_COL_SPLIT': '0', 'RLSTED_REAL_PSF': '0', 'RLSTED_ONES_SHORTCUT': '0',
             'RLSTED_SHARE_OBJECTS': '0', 'RLSTED_SEP': '2', 'RLSTED_SEP_ONE': '2', 'RLSTED_DIRECT': '2', 'RLSTED_SEP_TH': '64',
             'RLSTED_Q_EXP_EST': '10', 'RLSTED_Q_EXP_RATIO': '11'}
    want = {'chunk_mb_set': 1, 'chunk_mb': 3, 'lanes': 3, 'draw_ahead': 1, 'draw_grid': 5, 'poisson_groups': 0, 'inplace': 0, 'col_order': 2,
            'pair': 0, 'pair_max_ratio': 2, 'sub_one': 0, 'fuse_views': 1, 'col_split': 0, 'real_psf': 0, 'ones_shortcut': 0,
            'share_objects': 0, 'sep': 2, 'sep_one': 2, 'direct': 2, 'sep_th': 64, 'q_exp_est_set': 1, 'q_exp_ratio_set': 1, 'q_exp_est': 10,
            'q_exp_ratio': 11}
    assert plan(prog, options=' '.join('%s=%s' % kv for kv in every.items())) == want
    assert plan(prog, env=every) == want


@pytest.mark.parametrize('options, offender', [
    ('RLSTED_LANE=1', 'RLSTED_LANE'),                                   # a misspelt switch
    ('PAIR=0', 'PAIR'),
    ('RLSTED_LANES=1 RLSTED_DEBUG_SYNC=1', 'RLSTED_DEBUG_SYNC'),        # process wide: no switch of a plan
    ('RLSTED_PAIR', 'RLSTED_PAIR'),                                     # no '='
    ('RLSTED_LANES=1 RLSTED_PAIR 0', 'RLSTED_PAIR'),
    ('=1', '=1'),                                                       # no name
    ('RLSTED_PAIR=', 'RLSTED_PAIR='),                                   # no value
    ('RLSTED_PAIR=0 RLSTED_LANES=1 RLSTED_PAIR=0', 'RLSTED_PAIR'),      # twice
])
def test_what_the_text_may_not_hold(prog, options, offender):
    for dtype, views in (('f32', 1), ('f64', 3)):
        got = plan(prog, dtype, views, options)
        assert isinstance(got, str) and "'%s'" % offender in got, got


def test_the_environment_may_hold_anything(prog):
    got = plan(prog, env={'RLSTED_LANE': '1', 'PAIR': '0', 'RLSTED_DEBUG_SYNC': '1', 'RLSTED_FUZZ_SEEDS': '3'})
    assert got == dict(DEFAULTS, pair=1, sub_one=1, chunk_mb=0)
