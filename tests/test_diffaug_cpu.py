"""CPU: the opt-in differentiable augmentation of the discriminator's inputs (--D_aug) — the flag, the shared
parameter definition `aug_params`, the host draw order of HostDraws / StaticDraws, and the properties of the restatement
(tests/diffaug_cases.py) the GPU tests compare the kernels against. No kernel is launched here."""
import argparse
import itertools

import numpy as np
import pytest
import torch

import diffaug_cases as DA
from txt2vid_amd import functional_aug as A


# ------------------------------------------------------------------------------------------------ flag
def _parser():
    from txt2vid_amd.gan.trainer import add_params_to_parser
    return add_params_to_parser(argparse.ArgumentParser())


def test_flag_parses_and_defaults_to_off():
    assert _parser().parse_args([]).D_aug == ''
    assert _parser().parse_args(['--D_aug', DA.FULL]).D_aug == DA.FULL
    assert _parser().parse_args(['--D_aug', 'cutout']).D_aug == 'cutout'
    assert A.parse_policy('') == 0 and A.parse_policy(None) == 0
    assert A.parse_policy(DA.FULL) == 7 and A.parse_policy('cutout,color') == 5
    assert (A.COLOR, A.TRANSLATION, A.CUTOUT) == (1, 2, 4)


@pytest.mark.parametrize('bad', ['colour', 'color,', 'color;cutout', 'translate'])
def test_unknown_name_is_an_argparse_error(bad, capsys):
    with pytest.raises(SystemExit):
        _parser().parse_args(['--D_aug', bad])
    assert '--D_aug' in capsys.readouterr().err
    with pytest.raises(ValueError):
        A.parse_policy(bad)


def test_trainer_reads_the_flag_and_tolerates_its_absence():
    from txt2vid_amd.gan.trainer import TrainStep
    import schedule_cases as S

    class Gan(object):
        gen = object()
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    assert not hasattr(prm, 'D_aug')
    assert TrainStep(Gan(), None, None, None, prm, 'cpu').aug == 0
    prm.D_aug = 'color,cutout'
    assert TrainStep(Gan(), None, None, None, prm, 'cpu').aug == 5
    prm.D_aug = 'nope'
    with pytest.raises(ValueError):
        TrainStep(Gan(), None, None, None, prm, 'cpu')


# ------------------------------------------------------------------------------------------------ aug_params
@pytest.mark.parametrize('S', [8, 16, 32, 64, 128])
def test_aug_params_ranges_and_reachability(S):
    """u = 0 and the largest fp32 below 1 stay in range; every integer of the range is reachable."""
    r, size = int(np.floor(S / 8 + 0.5)), int(np.floor(S / 2 + 0.5))
    n = S + 1 - size % 2
    top = float(np.nextafter(np.float32(1), np.float32(0)))
    u = torch.zeros(2, A.K)
    u[1] = top
    assert float(u[1, 0]) < 1.0
    P = A.aug_params(u, S)
    assert P['r'] == r and P['size'] == size
    assert P['tx'].tolist() == [-r, r] and P['ty'].tolist() == [-r, r]
    assert P['x0'].tolist() == [-(size // 2), n - 1 - size // 2] and P['y0'].tolist() == P['x0'].tolist()
    assert P['b'].tolist() == [-0.5, top - 0.5] and P['s'].tolist() == [0.0, 2 * top] and P['c'].tolist() == [0.5, top + 0.5]
    # a fine fp32 grid over [0, 1): every shift in [-r, r] and every centre in [0, n) occurs, and nothing else
    grid = torch.linspace(0, 1, 4097)[:-1].view(-1, 1).repeat(1, A.K)
    P = A.aug_params(grid, S)
    assert sorted(set(P['tx'].tolist())) == list(range(-r, r + 1)) == sorted(set(P['ty'].tolist()))
    assert sorted(set((P['x0'] + size // 2).tolist())) == list(range(n)) == sorted(set((P['y0'] + size // 2).tolist()))
    # the definition, from the issue's formulas in exact arithmetic
    g64 = grid[:, 0].double()
    assert torch.equal(P['tx'], torch.clamp(torch.floor(g64 * (2 * r + 1)), max=2 * r).long() - r)
    assert torch.equal(P['x0'], torch.clamp(torch.floor(g64 * n), max=n - 1).long() - size // 2)


def test_aug_params_refuses_other_block_widths():
    with pytest.raises(ValueError):
        A.aug_params(torch.zeros(3, 6), 16)


# ------------------------------------------------------------------------------------------------ draw order
def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


@pytest.mark.parametrize('N,M', [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize('gp', [True, False])
@pytest.mark.parametrize('cond,ca_dim', [(False, 0), (True, 0), (True, 3)])
def test_static_and_host_draws_consume_the_same_sequence(N, M, gp, cond, ca_dim):
    from txt2vid_amd.draws import HostDraws, StaticDraws
    B, L, nl, ng = 5, 7, 4, 3
    perms = (N + 1) if cond else 0
    kw = dict(n_gen_phases=ng, gp=gp, subsample_input=True, n_perms=perms, n_d_steps=N, n_g_steps=M, ca_dim=ca_dim)
    args = (B, L, nl, ng, N, M, gp, ca_dim)

    def perms_of(d):
        return [d.perm(B, 'cpu').clone() for _ in range(perms)]
    _seed(11)
    hd = HostDraws()
    want = DA.consume(hd, *args, n_perms=perms, aug=True)
    want_perms = perms_of(hd)
    host_state = torch.get_rng_state()
    _seed(11)
    sd = StaticDraws('cpu', B, L, nl, n_aug=2 * N + M + 1, **kw)
    sd.begin_step()
    assert torch.equal(torch.get_rng_state(), host_state)
    got = DA.consume(sd, *args, n_perms=perms, aug=True)
    got_perms = perms_of(sd)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert all(torch.equal(a.long(), b.long()) for a, b in zip(got_perms, want_perms))
    with pytest.raises(AssertionError):
        sd.aug(B, 'cpu')                               # 2N + M + 1 blocks per iteration, no more
    sd.rewind()
    assert DA.consume(sd, *args, n_perms=perms, aug=True)[0] == got[0]
    # policy empty: the sequence, the buffer and the generator state are today's
    _seed(11)
    off = StaticDraws('cpu', B, L, nl, n_aug=0, **kw)
    off.begin_step()
    state_off = torch.get_rng_state()
    _seed(11)
    plain = StaticDraws('cpu', B, L, nl, **kw)
    plain.begin_step()
    assert torch.equal(torch.get_rng_state(), state_off)
    assert torch.equal(off.d_all, plain.d_all) and off.d_u is None
    assert sd.d_all.numel() == plain.d_all.numel() + (2 * N + M + 1) * B * A.K
    _seed(11)
    want_off = DA.consume(HostDraws(), *args, n_perms=perms, aug=False)
    assert torch.equal(torch.get_rng_state(), state_off)
    for a, b in zip(DA.consume(off, *args, n_perms=perms, aug=False), want_off):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_static_draws_refuse_a_wrong_block_count():
    from txt2vid_amd.draws import StaticDraws
    with pytest.raises(ValueError):
        StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=4)


def test_host_draws_aug_block():
    from txt2vid_amd.draws import HostDraws
    torch.manual_seed(4)
    u = HostDraws().aug(3, 'cpu')
    torch.manual_seed(4)
    assert torch.equal(u, torch.rand(3, A.K)) and A.K == 8


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('policy', DA.SUBSETS)
@pytest.mark.parametrize('C', [1, 3])
def test_adjoint_identity_in_float64(policy, C):
    """<T(x) - T(0), g> = <x, T^T g>: the map is affine per clip, autograd supplies T^T."""
    g = torch.Generator()
    g.manual_seed(7)
    N, T, S = 5, 2, 16
    u = torch.rand(N, A.K, generator=g)
    x = (torch.rand(N, C, T, S, S, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    gy = torch.randn(N, C, T, S, S, generator=g, dtype=torch.float64)
    y = DA.augment(x, u, policy)
    gx, = torch.autograd.grad(y, x, gy)
    y0 = DA.augment(torch.zeros_like(x), u, policy)
    lhs, rhs = float(((y - y0).detach() * gy).sum()), float((x.detach() * gx).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
    # affine: T(a x1 + (1 - a) x2) = a T(x1) + (1 - a) T(x2)
    x2 = torch.rand(N, C, T, S, S, generator=g, dtype=torch.float64)
    mix = DA.augment(0.25 * x.detach() + 0.75 * x2, u, policy)
    assert torch.allclose(mix, 0.25 * y.detach() + 0.75 * DA.augment(x2, u, policy), rtol=0, atol=1e-13)


def test_restatement_against_hand_computed_cases():
    x = torch.arange(2 * 8 * 8, dtype=torch.float64).view(1, 2, 1, 8, 8) / 64 - 1
    u = torch.zeros(1, A.K)
    u[0, :3] = torch.tensor([0.75, 0.25, 1.0 - 2 ** -20])       # b = 0.25, s = 0.5, c ~ 1.5
    u[0, 3], u[0, 4] = 0.99, 0.0                                # r = 1: tx = +1, ty = -1
    u[0, 5], u[0, 6] = 0.5, 0.0                                 # size 4, n = 9: cx = 4 -> columns 2..5; cy = 0 -> rows -2..1
    y = DA.augment(x, u, 'translation')
    assert torch.equal(y[0, :, 0, :7, 1:], x[0, :, 0, 1:, :7]) and float(y[0, :, 0, 7].abs().sum()) == 0 and float(y[0, :, 0, :, 0].abs().sum()) == 0
    y = DA.augment(x, u, 'cutout')
    assert float(y[0, :, 0, :2, 2:6].abs().sum()) == 0
    keep = torch.ones(8, 8, dtype=torch.bool)
    keep[:2, 2:6] = False
    assert torch.equal(y[0, :, 0][:, keep], x[0, :, 0][:, keep])
    y = DA.augment(x, u, 'color')
    c = float(u[0, 2].double() + 0.5)
    m = x.mean(dim=1, keepdim=True)
    v = (x - m) * 0.5 + m + 0.25
    want = (v - v.mean()) * c + v.mean()
    assert torch.allclose(y, want, rtol=0, atol=1e-14)
    assert abs(float(v.mean()) - (float(x.mean()) + 0.25)) < 1e-14         # saturation keeps the mean: mu = mean(x) + b
    # C = 1: saturation is the identity
    x1 = x[:, :1]
    u2 = u.clone()
    u2[0, 1] = 0.9
    assert torch.equal(DA.augment(x1, u, 'color'), DA.augment(x1, u2, 'color'))


@pytest.mark.parametrize('policy', DA.SUBSETS)
def test_level_consistency(policy):
    """Augmenting a constant-per-2x2-block clip at S = 64 and then nearest-downsampling it equals downsampling first and
    augmenting at S = 32 with the parameters `aug_params` derives for that level from the same rows: exact, because the draws
    are chosen so that the shifts and cut boxes divide evenly (r: 8 vs 4, size: 32 vs 16) and the data and colour draws are
    dyadic (every sum and product is exact in float64). Level sample j reads base row 2 j."""
    g = torch.Generator()
    g.manual_seed(5)
    B, C, T = 4, 2, 2
    u = torch.zeros(B, A.K)
    u[:, 0] = torch.tensor([0.25, 0.5, 0.75, 0.125])
    u[:, 1] = torch.tensor([0.5, 0.25, 0.75, 0.375])
    u[:, 2] = torch.tensor([0.0, 0.5, 0.25, 0.75])
    u[:, 3] = torch.tensor([0.05, 0.5, 0.95, 0.3])              # tx at 64 / 32: -8/-4, 0/0, +8/+4, -3/-2 (row 3 is never read)
    u[:, 4] = torch.tensor([0.95, 0.5, 0.05, 0.3])
    u[:, 5] = torch.tensor([0.25, 0.0, 0.5, 0.3])               # cx at 64 / 32: 16/8, 0/0, 32/16
    u[:, 6] = torch.tensor([0.5, 0.0, 0.75, 0.3])               # cy: 32/16, 0/0, 48/24
    P64, P32 = A.aug_params(u, 64), A.aug_params(u, 32)
    for k in ('tx', 'ty', 'x0', 'y0'):
        assert (P64[k][::2] == 2 * P32[k][::2]).all(), k
    low = torch.randint(-8, 9, (B, C, T, 32, 32), generator=g).double() / 8
    full = low.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    a = DA.augment(full, u, policy)[::2, :, :, ::2, ::2]
    b = DA.augment(low[::2], u, policy, stride=2)
    assert torch.equal(a, b)
    assert not torch.equal(b, low[::2])
