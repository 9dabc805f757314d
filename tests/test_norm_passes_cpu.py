"""CPU: the cuts `t2v_bn_plan` gives the shapes of tests/norm_pass_cases.py, and that between them they put every pass of the
unrolled slice walker (csrc/pointwise.hip) on every path it has. Host arithmetic only."""
import pytest

import norm_cases as nc
import norm_pass_cases as pc


@pytest.mark.parametrize('case', list(pc.CASES))
def test_plan_and_elements_per_thread(case):
    (N, Cc, H, W), split, slices = pc.CASES[case]
    assert nc.plan(N, Cc, H * W) == (0, split, slices)
    assert (pc.per_thread(N * H * W, split), pc.per_thread(N * H * W, slices)) == pc.PER_THREAD[case]


def test_every_path_of_the_walker_is_reached():
    stat = [v[0] for v in pc.PER_THREAD.values()]
    app = [v[1] for v in pc.PER_THREAD.values()]
    U, CAP = pc.UNROLL, pc.REG_CAP
    for side in (stat, app):
        assert any(hi < U for lo, hi in side)                              # a predicated tail alone
        assert any(lo >= U and hi % U for lo, hi in side)                  # full trips and a tail
        assert any(lo == U for lo, hi in side)                             # exactly one full trip, no tail
    assert any(U < lo and hi <= CAP and lo % U and hi % U for lo, hi in stat)      # registers, several trips, ragged
    assert any(lo > CAP for lo, hi in stat)                                # the re-read
    assert any(lo == CAP and hi == CAP + 1 for lo, hi in stat)             # both in one workgroup
    rows = {H * W for (N, Cc, H, W), _, _ in pc.CASES.values()}
    assert {1, 7, 64, 255, 258} <= rows
    # slices that start inside a sample
    assert any((-(-N * H * W // split)) % (H * W) for (N, Cc, H, W), split, _ in pc.CASES.values() if split > 1)
