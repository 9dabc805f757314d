"""GPU: the unrolled slice walker of the two-launch BatchNorm training passes (csrc/pointwise.hip: `BnWalk`, `bn_for_each`) at
the shapes of tests/norm_pass_cases.py — full trips, ragged tails, the statistics pass keeping its slice in registers, reading
it again, and doing both in one workgroup; rows of 1, 7, 64, 255 and 258 elements; slices that start inside a sample — against
the float64 reference and the tolerances of tests/norm_cases.py. The cuts themselves are asserted on the CPU
(tests/test_norm_passes_cpu.py)."""
import itertools

import pytest
import torch

import norm_cases as nc
import norm_pass_cases as pc
from test_norm_gpu import FIELDS, run_op

pytestmark = pytest.mark.gpu

# case by case (norm_pass_cases.inputs keeps the last two): relu x up x {no fork, the `add` operand}
VARIANTS = [(c, r, relu, up, fork) for (c, r) in pc.CASE_RECIPES
            for relu, up, fork in itertools.product((False, True), (False, True), ('off', 'both'))]
IDS = ['%s-%s-%s-%s-%s' % (c, r, 'relu' if relu else 'lin', 'up' if up else 'flat', fork) for c, r, relu, up, fork in VARIANTS]


@pytest.mark.parametrize('case,recipe,relu,up,fork', VARIANTS, ids=IDS)
def test_batch_norm_act(case, recipe, relu, up, fork):
    inp = pc.inputs(case, recipe)
    got = run_op(inp, pc.MOMENTUM, pc.EPS, relu, up, fork)
    nc.check('/'.join((case, recipe, str(int(relu)), str(int(up)), fork)), got, pc.case_reference(case, recipe, relu, up, fork), FIELDS)


@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('case', list(pc.CASES))
def test_two_runs_give_the_same_bits(case, up):
    inp = pc.inputs(case, 'offset' if (case, 'offset') in pc.CASE_RECIPES else 'plain')
    a = run_op(inp, pc.MOMENTUM, pc.EPS, True, up, 'both')
    b = run_op(inp, pc.MOMENTUM, pc.EPS, True, up, 'both')
    for f in FIELDS:
        assert torch.equal(a[f], b[f]), f
