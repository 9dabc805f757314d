"""CPU: which cut every BatchNorm parity case gets (`t2v_bn_plan`: host arithmetic, no launch), and the float64 reference of
tests/norm_cases.py against `torch.nn.BatchNorm2d` before it judges a kernel (tests/test_norm_gpu.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc


@pytest.mark.parametrize('case', list(nc.CASES))
def test_plan_of_every_case(case):
    (N, Cc, H, W), split, slices, _, _ = nc.CASES[case]
    assert nc.plan(N, Cc, H * W) == (0, split, slices)
    from txt2vid_amd._lib import lib
    assert lib().t2v_bn_ws_floats(N, Cc, H * W) == 3 * Cc * split + 2 * Cc


def test_the_cases_cut_where_their_names_say():
    """`straddle`: both cuts cross sample boundaries, the last statistics slice is short; `cap64`: the 64-slice cap binds."""
    (N, Cc, H, W), split, slices, _, _ = nc.CASES['straddle']
    S, total = H * W, N * H * W
    for parts in (split, slices):
        per = -(-total // parts)
        assert per % S != 0 and per * (parts - 1) < total <= per * parts
    assert total < -(-total // split) * split
    (N, Cc, H, W), split, slices, _, _ = nc.CASES['cap64']
    total = N * H * W
    assert split == 64 and total // 1024 >= 64 and (1024 + Cc - 1) // Cc > 64
    assert -(-total // 64) == 1036 and 0 < total - 63 * 1036 < 1036


def test_plan_rejects_bad_arguments():
    from txt2vid_amd._lib import lib
    out = (C.c_int32 * 2)()
    assert lib().t2v_bn_plan(0, 3, 5, out) < 0
    assert lib().t2v_bn_plan(2, 0, 5, out) < 0
    assert lib().t2v_bn_plan(2, 3, 0, out) < 0
    assert lib().t2v_bn_plan(2, 3, -7, out) < 0
    assert lib().t2v_bn_plan(2, 3, 5, None) < 0
    assert lib().t2v_bn_ws_floats(0, 3, 5) < 0


@pytest.mark.parametrize('relu,up', [(False, False), (True, True)])
def test_reference_agrees_with_the_torch_module(relu, up):
    """fp32 nn.BatchNorm2d (train mode: running statistics with the unbiased variance, num_batches_tracked) -> relu ->
    interpolate on `tiny`, then one eval-mode forward on the updated buffers."""
    inp = nc.inputs('tiny', 'plain')
    momentum, eps = nc.hparams('tiny')
    gy = nc.grad_out(inp, relu, up)
    m = torch.nn.BatchNorm2d(inp['x'].shape[1], eps=eps, momentum=momentum)
    with torch.no_grad():
        m.weight.copy_(inp['gamma'])
        m.bias.copy_(inp['beta'])
        m.running_mean.copy_(inp['rm'])
        m.running_var.copy_(inp['rv'])
        m.num_batches_tracked.fill_(41)

    def head(t):
        t = F.relu(t) if relu else t
        return F.interpolate(t, scale_factor=2) if up else t
    x = inp['x'].clone().requires_grad_(True)
    y = head(m(x))
    (y * gy).sum().backward()
    ref = nc.reference(inp['x'], inp['gamma'], inp['beta'], inp['rm'], inp['rv'], gy, momentum, eps, relu, up, counter=41)
    got = {'y': y, 'dx': x.grad, 'dgamma': m.weight.grad, 'dbeta': m.bias.grad, 'rm': m.running_mean, 'rv': m.running_var}
    nc.check('module/train', got, ref, list(got))
    assert int(m.num_batches_tracked) == ref['counter'] == 42
    assert ref['y'].dtype == ref['dx'].dtype == ref['rv'].dtype == torch.float64
    m.eval()
    ye = head(m(inp['x']))
    refe = nc.reference(inp['x'], inp['gamma'], inp['beta'], m.running_mean, m.running_var, None, momentum, eps, relu, up,
                        training=False, counter=42)
    nc.check('module/eval', {'y': ye}, refe, ['y'])
    assert refe['counter'] == 42 and torch.equal(refe['rm'], m.running_mean.double())


def test_reference_of_the_forked_input():
    """The second consumer `+ (x * w2).sum()` adds w2 to dL/dx and nothing else; alone, it leaves dgamma = dbeta = 0."""
    inp = nc.inputs('tiny', 'dead')
    off, both = nc.case_reference('tiny', 'dead', True, True, 'off'), nc.case_reference('tiny', 'dead', True, True, 'both')
    assert torch.allclose(both['dx'], off['dx'] + inp['w2'].double(), rtol=0, atol=1e-12)
    assert torch.equal(both['dgamma'], off['dgamma']) and torch.equal(nc.case_reference('tiny', 'dead', True, True, 'bn_only')['dx'], off['dx'])
    alias = nc.case_reference('tiny', 'dead', True, True, 'alias_only')
    assert torch.equal(alias['dx'], inp['w2'].double()) and not alias['dgamma'].any() and not alias['dbeta'].any()
    # the dead channels: variance 0, so 1/std = 1/sqrt(eps); channel 1 (x = 0, beta = 0) is an exact tie at 0 everywhere
    assert torch.allclose(off['istd'][1:3], torch.full((2,), 1e-3 ** -0.5, dtype=torch.float64), rtol=1e-9)
    assert not off['y'][:, 1].any()
