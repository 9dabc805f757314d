"""CPU: every host query of the convolution launchers (plans, workspace and slab sizes, split counts, refusals) answers exactly
what tests/golden/conv_plans.npz recorded for the same launches with the library of the commit before the launch decisions of
conv.hip were last restructured (tests/golden/make_golden_plans.py: the parity cases of conv_cases.py, the frame-strided and
pooled members, the refused geometries and a channel x kernel x member-set grid; the environment tunables in one child process
each). Host arithmetic only, no GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_golden_plans as mg       # noqa: E402


def _assert_same(got, want, ls, what):
    assert got.shape == want.shape, '%s: %d launches x %d values here, %d x %d in the fixture' % ((what,) + got.shape + want.shape)
    rows = np.nonzero((got != want).any(axis=1))[0]
    for r in rows[:10]:
        cols = np.nonzero(got[r] != want[r])[0]
        print('%s, launch %d (%s): record[%s] = %s, fixture has %s' % (what, r, ls[r][0], cols.tolist(), got[r][cols].tolist(), want[r][cols].tolist()))
    assert len(rows) == 0, '%s: %d of %d launches differ from the fixture (the first ones are printed above)' % (what, len(rows), len(ls))


def test_every_host_query_answers_as_recorded(golden):
    want = golden('conv_plans')
    ls = mg.launches()
    got = mg.records(ls)
    assert len(ls) == len(want['default']) == got.shape[0]          # every case compared, none dropped
    _assert_same(got, want['default'], ls, 'default tunables')
    # the recorded launches do reach the decisions they are there to pin
    ok = got[got[:, 0] == 0]
    assert {0, 1, 2, 3, 4, 5, 12} <= set(ok[:, 1].tolist())                                   # every forward kernel family
    assert set(got[got[:, 56] == 0][:, 57].tolist()) == {0, 1, 2, 3, 4}                       # every weight-gradient kernel
    assert (got[:, 0] < 0).any() and (got[:, 56] < 0).any() and all((got[:, c] == 0).any() and (got[:, c] < 0).any() for c in (27, 67, 76, 85))


def test_every_host_query_answers_as_recorded_under_each_tunable(golden):
    want = golden('conv_plans')
    ls = mg.launches(reduced=True)
    keys = [mg.env_key(n, v) for n, v in mg.ENV_CASES]
    assert sorted(keys + ['default']) == sorted(want.files)
    got = mg.records_in_children(ls, mg.ENV_CASES)
    base = want['default'][:len(ls)]                 # (the reduced list is the head of the full one)
    for key in keys:
        assert len(ls) == len(want[key]) == got[key].shape[0]
        _assert_same(got[key], want[key], ls, key)
        assert (want[key] != base).any(), '%s moves no recorded plan' % key
