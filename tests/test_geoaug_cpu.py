"""CPU: the geometric augmentation of the discriminator's inputs (the names flip, scale, rotate of --D_aug) — the
flag and the policy bits, the shared parameter definition `geo_params`, the host draw order of HostDraws / StaticDraws with the
geometric block, the properties of the restatement (tests/geoaug_cases.py) the GPU tests compare the kernels against, and the
refusals of the two entry points, which come before any launch. No kernel is launched here."""
import argparse
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ada_cases as AC
import diffaug_cases as DA
import geoaug_cases as GC
from txt2vid_amd import functional_aug as A

TOP = float(np.nextafter(np.float32(1), np.float32(0)))


# ------------------------------------------------------------------------------------------------ flag and policy
def _parser():
    from txt2vid_amd.gan.trainer import add_params_to_parser
    return add_params_to_parser(argparse.ArgumentParser())


def test_flag_and_policy_bits():
    assert (A.FLIP, A.SCALE, A.ROTATE, A.GEO) == (8, 16, 32, 56)
    assert A.parse_policy(DA.FULL) == 7                                   # the old names keep their bits
    assert A.parse_policy(GC.GEO) == 56 and A.parse_policy(GC.SIX) == 63
    assert A.parse_policy('flip') == 8 and A.parse_policy('scale') == 16 and A.parse_policy('rotate') == 32
    assert A.parse_policy('rotate,color') == 33
    assert A.NAMES[:3] == ('color', 'translation', 'cutout')
    assert _parser().parse_args([]).D_aug == ''
    assert _parser().parse_args(['--D_aug', GC.SIX]).D_aug == GC.SIX
    assert _parser().parse_args(['--D_aug', 'flip']).D_aug == 'flip'


@pytest.mark.parametrize('bad', ['colour', 'color,', 'color;cutout', 'translate', 'flip,', 'rotation', 'scale;flip', 'Flip'])
def test_unknown_name_is_still_refused(bad, capsys):
    with pytest.raises(SystemExit):
        _parser().parse_args(['--D_aug', bad])
    assert '--D_aug' in capsys.readouterr().err
    with pytest.raises(ValueError):
        A.parse_policy(bad)


def test_help_text_names_the_new_transformations_and_says_untuned():
    text = ' '.join(_parser().format_help().split())
    assert 'color,translation,cutout,flip,scale,rotate' in text
    assert 'nobody has tuned them for video' in text


def test_trainer_splits_the_policy():
    from txt2vid_amd.gan.trainer import TrainStep
    import schedule_cases as S

    class Gan(object):
        gen = object()
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    assert TrainStep(Gan(), None, None, None, prm, 'cpu').geo == 0
    prm.D_aug = DA.FULL
    ts = TrainStep(Gan(), None, None, None, prm, 'cpu')
    assert (ts.aug, ts.geo) == (7, 0)
    prm.D_aug = 'cutout,rotate'
    ts = TrainStep(Gan(), None, None, None, prm, 'cpu')
    assert (ts.aug, ts.geo) == (36, 32)


# ------------------------------------------------------------------------------------------------ geo_params
def test_geo_params_follow_the_definition():
    v = torch.zeros(5, A.K)
    v[:, 0] = torch.tensor([0.0, 0.49999997, 0.5, TOP, 0.25])
    v[:, 1] = torch.tensor([0.0, 0.5, TOP, 0.25, 0.5])
    v[:, 2] = torch.tensor([0.0, 0.5, TOP, 0.25, 0.5])
    P = A.geo_params(v)
    assert P['f'].tolist() == [-1.0, -1.0, 1.0, 1.0, -1.0]
    assert P['s'].dtype == torch.float64 and P['M'].dtype == torch.float32 and P['M'].shape == (5, 2, 2)
    for j in range(5):
        v1, v2 = float(v[j, 1]), float(v[j, 2])
        s, th, f = 2.0 ** ((2 * v1 - 1) * 0.4), (2 * v2 - 1) * math.pi / 6, float(P['f'][j])
        assert abs(float(P['s'][j]) - s) <= 4e-16 * s and abs(float(P['theta'][j]) - th) <= 2e-16
        want = torch.tensor([[f * math.cos(th) / s, f * math.sin(th) / s], [-math.sin(th) / s, math.cos(th) / s]], dtype=torch.float64)
        assert float((P['M'][j].double() - want).abs().max()) <= 2.0 ** -24 * 1.32 + 1e-15      # one rounding to fp32
    # the ranges: s in [2^-0.4, 2^0.4), |theta| <= pi / 6, and the adjoint's window: s (|cos| + |sin|) < 1.81
    assert abs(float(P['s'][0]) - 2.0 ** -0.4) < 1e-15 and float(P['s'][2]) < 2.0 ** 0.4
    assert float(P['theta'][0]) == -A.PI_6 and float(P['theta'][2]) < A.PI_6
    grid = torch.linspace(0, 1, 4097)[:-1]
    vv = torch.zeros(4096, A.K)
    vv[:, 1], vv[:, 2] = TOP, grid
    Pg = A.geo_params(vv)
    assert float((Pg['s'] * (Pg['theta'].cos().abs() + Pg['theta'].sin().abs())).max()) < 1.81
    # a row that is exactly the identity, and a pure flip; transformations outside the policy take f = 1, s = 1, theta = 0
    assert torch.equal(P['M'][4], torch.tensor([[-1.0, 0.0], [0.0, 1.0]]))
    assert torch.equal(A.geo_params(v, 0)['M'], torch.eye(2).expand(5, 2, 2))
    Pf = A.geo_params(v, A.FLIP)
    assert Pf['s'].tolist() == [1.0] * 5 and Pf['theta'].tolist() == [0.0] * 5 and Pf['f'].tolist() == P['f'].tolist()
    Ps = A.geo_params(v, torch.tensor([A.SCALE, A.ROTATE, A.GEO, 0, A.SCALE | A.ROTATE]))
    assert Ps['f'].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0]
    assert float(Ps['theta'][0]) == 0.0 and float(Ps['s'][0]) == float(P['s'][0]) and float(Ps['s'][1]) == 1.0
    assert torch.equal(Ps['M'][2], P['M'][2])
    with pytest.raises(ValueError):
        A.geo_params(torch.zeros(3, 6))


# ------------------------------------------------------------------------------------------------ draw order
def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


@pytest.mark.parametrize('N,M', [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('gp,ca_dim', [(True, 0), (False, 3)])
def test_static_and_host_draws_consume_the_same_sequence(N, M, gated, gp, ca_dim):
    """Value for value with a geometric policy, gated and ungated; u, [g], v next to one another in the staging buffer."""
    from txt2vid_amd.draws import HostDraws, StaticDraws
    B, L, nl, ng = 5, 7, 4, 3
    sites = 2 * N + M + 1
    kw = dict(n_gen_phases=ng, gp=gp, subsample_input=True, n_perms=0, n_d_steps=N, n_g_steps=M, ca_dim=ca_dim)
    args = (B, L, nl, ng, N, M, gp, ca_dim)
    _seed(11)
    want = GC.consume(HostDraws(), *args, gated=gated, geo=True)
    host_state = torch.get_rng_state()
    _seed(11)
    sd = StaticDraws('cpu', B, L, nl, n_aug=sites * (2 if gated else 1), n_geo=sites, **kw)
    assert sd.geo and sd.gated == gated and sd.n_geo == sites
    sd.begin_step()
    assert torch.equal(torch.get_rng_state(), host_state)
    got = GC.consume(sd, *args, gated=gated, geo=True)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    with pytest.raises(AssertionError):
        sd.aug(B, 'cpu', gated=gated, geo=True)           # 2N + M + 1 sites per iteration, no more
    sd.rewind()
    with pytest.raises(AssertionError):
        sd.aug(B, 'cpu', gated=gated)                     # a geometric layout is consumed with geo=True
    # one upload: the geometric blocks sit in the same buffer, behind their site's u (and g)
    _seed(11)
    plain = StaticDraws('cpu', B, L, nl, **kw)
    assert sd.d_all.numel() == plain.d_all.numel() + sites * (3 if gated else 2) * B * A.K
    w = 3 if gated else 2
    blocks = [t for t in want if torch.is_tensor(t) and t.shape == (B, A.K)]
    assert len(blocks) == sites * w
    assert all(torch.equal(sd.d_u[i], blocks[i]) for i in range(sites * w))


@pytest.mark.parametrize('gated', [False, True])
def test_n_geo_zero_is_todays_layout_and_sequence(gated):
    from txt2vid_amd.draws import HostDraws, StaticDraws
    B, L, nl, ng, N, M = 5, 7, 4, 3, 2, 2
    sites = 2 * N + M + 1
    kw = dict(n_gen_phases=ng, gp=True, subsample_input=True, n_perms=0, n_d_steps=N, n_g_steps=M, ca_dim=0)
    n_aug = sites * (2 if gated else 1)
    _seed(3)
    a = StaticDraws('cpu', B, L, nl, n_aug=n_aug, n_geo=0, **kw)
    a.begin_step()
    state_a = torch.get_rng_state()
    _seed(3)
    b = StaticDraws('cpu', B, L, nl, n_aug=n_aug, **kw)
    b.begin_step()
    assert torch.equal(torch.get_rng_state(), state_a)
    assert torch.equal(a.d_all, b.d_all) and a.d_u.shape == (n_aug, B, A.K) and not a.geo and a.n_geo == 0
    _seed(3)
    want = AC.consume(HostDraws(), B, L, nl, ng, N, M, True, 0, gated)
    assert torch.equal(torch.get_rng_state(), state_a)
    for x, y in zip(AC.consume(a, B, L, nl, ng, N, M, True, 0, gated), want):
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y
    # HostDraws without geo: the return types of today
    torch.manual_seed(4)
    u = HostDraws().aug(3, 'cpu')
    torch.manual_seed(4)
    assert torch.is_tensor(u) and torch.equal(u, torch.rand(3, A.K))
    torch.manual_seed(4)
    u, g, v = HostDraws().aug(3, 'cpu', gated=True, geo=True)
    torch.manual_seed(4)
    assert torch.equal(u, torch.rand(3, A.K)) and torch.equal(g, torch.rand(3, A.K)) and torch.equal(v, torch.rand(3, A.K))


def test_static_draws_refuse_a_wrong_geo_count():
    from txt2vid_amd.draws import StaticDraws
    with pytest.raises(ValueError):
        StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=6, n_geo=5)
    with pytest.raises(ValueError):
        StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=0, n_geo=6)       # u is drawn at every geometric site
    StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=6, n_geo=6)
    StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=12, n_geo=6)


# ------------------------------------------------------------------------------------------------ the restatement
def _clips(N, C, T, S, dtype, seed=0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(N, C, T, S, S, generator=g, dtype=dtype) * 2 - 1, torch.rand(2 * N, A.K, generator=g)


@pytest.mark.parametrize('S', [8, 9])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_identity_parameters_are_a_bitwise_copy(S, dtype):
    x, v = _clips(3, 2, 2, S, dtype)
    v[:, 0], v[:, 1], v[:, 2] = 0.75, 0.5, 0.5
    assert torch.equal(GC.augment_geo(x, v, GC.GEO), x)
    assert torch.equal(GC.augment_geo(x, v, GC.GEO, stride=2), x)
    v[:, 1], v[:, 2] = 0.3, 0.9                                                       # not in the policy: not applied
    assert torch.equal(GC.augment_geo(x, v, 'flip'), x)
    assert not torch.equal(GC.augment_geo(x, v, 'scale'), x) and not torch.equal(GC.augment_geo(x, v, 'rotate'), x)


@pytest.mark.parametrize('S', [8, 9])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_pure_flip_equals_torch_flip(S, dtype):
    x, v = _clips(4, 2, 2, S, dtype, 1)
    v[:, 0] = torch.tensor([0.1, 0.9, 0.49999997, 0.5, 0.0, 0.7, TOP, 0.2])
    y = GC.augment_geo(x, v, 'flip')
    for j in range(4):
        assert torch.equal(y[j], torch.flip(x[j], dims=[-1]) if float(v[j, 0]) < 0.5 else x[j])
    y = GC.augment_geo(x, v, 'flip', stride=2)                                        # clip j reads row 2 j
    for j in range(4):
        assert torch.equal(y[j], torch.flip(x[j], dims=[-1]) if float(v[2 * j, 0]) < 0.5 else x[j])


def test_dead_gate_is_a_copy():
    """g == p is not applied (strict <); each of the columns 3, 4, 5 gates its own transformation."""
    x, v = _clips(3, 1, 2, 8, torch.float64, 2)
    v[:, 0] = 0.1
    g = torch.full((6, A.K), 0.25)
    assert torch.equal(GC.augment_geo(x, v, GC.GEO, gates=g, p=0.25), x)
    assert torch.equal(GC.augment_geo(x, v, GC.GEO, gates=g, p=0.0), x)
    full = GC.augment_geo(x, v, GC.GEO)
    assert torch.equal(GC.augment_geo(x, v, GC.GEO, gates=g, p=1.0), full) and not torch.equal(full, x)
    g[:, :3] = 0.0                                                                    # the old columns gate nothing here
    assert torch.equal(GC.augment_geo(x, v, GC.GEO, gates=g, p=0.25), x)
    for col, name in ((3, 'flip'), (4, 'scale'), (5, 'rotate')):
        gg = torch.full((6, A.K), 0.25)
        gg[:, col] = 0.2
        assert torch.equal(GC.augment_geo(x, v, GC.GEO, gates=gg, p=0.25), GC.augment_geo(x, v, name))
    assert GC.effective_geo(torch.tensor([[0, 0, 0, 0.1, 0.3, 0.2, 0, 0]]), 0.25, GC.SIX, 1) == [8 | 32]


@pytest.mark.parametrize('policy', GC.GEO_SUBSETS)
def test_restatement_is_linear_and_has_an_adjoint(policy):
    x, v = _clips(3, 2, 2, 9, torch.float64, 3)
    x.requires_grad_(True)
    g = torch.Generator()
    g.manual_seed(8)
    gy = torch.randn(3, 2, 2, 9, 9, generator=g, dtype=torch.float64)
    y = GC.augment_geo(x, v, policy)
    gx, = torch.autograd.grad(y, x, gy)
    lhs, rhs = float((y.detach() * gy).sum()), float((x.detach() * gx).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    x2 = torch.rand(3, 2, 2, 9, 9, generator=g, dtype=torch.float64)
    mix = GC.augment_geo(0.25 * x.detach() + 0.75 * x2, v, policy)
    assert torch.allclose(mix, 0.25 * y.detach() + 0.75 * GC.augment_geo(x2, v, policy), rtol=0, atol=1e-13)


def test_restatement_against_hand_computed_cases():
    """A constant frame stays constant where all four taps are inside; linear data is resampled exactly, about the centre."""
    S = 8
    x = torch.ones(1, 1, 1, S, S, dtype=torch.float64)
    v = torch.zeros(1, A.K)
    v[0, 0], v[0, 1], v[0, 2] = 0.9, 0.0, 0.5                    # s = 2^-0.4: the frame shrinks, the border shows the zero fill
    y = GC.augment_geo(x, v, 'scale')
    assert torch.allclose(y[0, 0, 0, 1:7, 1:7], torch.ones(6, 6, dtype=torch.float64), rtol=0, atol=1e-15)
    assert float(y[0, 0, 0, 0].abs().sum()) == 0 and float(y[0, 0, 0, :, 7].abs().sum()) == 0       # |x_src| = 1.32 * 3.5 > 4.5
    v[0, 1] = TOP                                                # s ~ 2^0.4: the frame grows, every tap inside
    y = GC.augment_geo(x, v, 'scale')
    assert torch.allclose(y, x, rtol=0, atol=1e-15)
    ramp = torch.arange(S, dtype=torch.float64).view(1, 1, 1, 1, S).expand(1, 1, 1, S, S).contiguous()
    y = GC.augment_geo(ramp, v, 'scale')
    m = float(A.geo_params(v, A.SCALE)['M'][0, 0, 0])
    w = torch.arange(S, dtype=torch.float64)
    assert torch.allclose(y[0, 0, 0, 3], m * (w + 0.5 - S / 2) + S / 2 - 0.5, rtol=0, atol=1e-13)      # linear data: exact resampling
    # rotation by +pi/6 (v2 -> 1): the centre 2 x 2 block of a ramp in x picks up cos * xo + sin * yo
    v[0, 1], v[0, 2] = 0.5, TOP
    P = A.geo_params(v, A.ROTATE)
    y = GC.augment_geo(ramp, v, 'rotate')
    c, sn = float(P['M'][0, 0, 0]), float(P['M'][0, 0, 1])
    for h in (3, 4):
        for ww in (3, 4):
            want = c * (ww + 0.5 - S / 2) + sn * (h + 0.5 - S / 2) + S / 2 - 0.5
            assert abs(float(y[0, 0, 0, h, ww]) - want) < 1e-13


def test_level_consistency_of_flip():
    """Row j * 2^l at level l: a clip is mirrored at every pyramid level or at none."""
    g = torch.Generator()
    g.manual_seed(5)
    v = torch.rand(4, A.K, generator=g)
    v[:, 0] = torch.tensor([0.1, 0.9, 0.8, 0.2])
    low = torch.rand(4, 1, 2, 8, 8, generator=g, dtype=torch.float64)
    full = low.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    a = GC.augment_geo(full, v, 'flip')[::2, :, :, ::2, ::2]
    b = GC.augment_geo(low[::2], v, 'flip', stride=2)
    assert torch.equal(a, b) and not torch.equal(b, low[::2])


# ------------------------------------------------------------------------------------------------ before any launch
@pytest.fixture(scope='module')
def built():
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'txt2vid_amd', 'csrc', 'libt2v_hip.so')
    if not os.path.exists(so):
        subprocess.check_call(['make', '-C', os.path.dirname(so), '-j4'])
    return so


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    """Both entry points exist and answer T2V_EINVAL on the host side, without a GPU (the pattern of
    test_abi.py::test_argument_validation_without_gpu). The pointers are never dereferenced."""
    from txt2vid_amd._lib import lib, AugMember, MAX_GROUPS
    EINVAL = -1
    x = torch.zeros(2 * 2 * 64)
    y = torch.zeros(2 * 2 * 64)
    v = torch.zeros(2, A.K)
    p = torch.ones(1)

    def member(**kw):
        m = dict(x=x.data_ptr(), y=y.data_ptr(), u=v.data_ptr(), N=2, C=1, T=2, S=8, row_stride=1, rows=2, policy=A.GEO)
        m.update(kw)
        return m

    def call(fn, ms, n=None, gates=None, pp=None):
        arr = (AugMember * max(1, len(ms)))()
        for a, m in zip(arr, ms):
            for k, val in m.items():
                setattr(a, k, val)
        return fn(arr, gates, len(ms) if n is None else n, pp, None)
    l = lib()
    for fn in (l.t2v_geoaug_fwd, l.t2v_geoaug_bwd):
        assert fn(None, None, 1, None, None) == EINVAL
        assert call(fn, [member()], n=0) == EINVAL
        assert call(fn, [member()], n=-1) == EINVAL
        assert call(fn, [member()] * (MAX_GROUPS + 1)) == EINVAL                  # more than MAX_GROUPS members
        for bad in (dict(policy=0), dict(policy=7), dict(policy=1), dict(policy=9), dict(policy=63), dict(policy=64),
                    dict(policy=64 | 8), dict(policy=-1), dict(x=None), dict(y=None), dict(u=None), dict(y=x.data_ptr()),
                    dict(N=0), dict(C=0), dict(T=0), dict(S=0), dict(row_stride=0), dict(row_stride=-1), dict(rows=1),
                    dict(rows=0), dict(row_stride=2)):
            assert call(fn, [member(), member(**bad)]) == EINVAL, bad
        # exactly one of gates / p
        gates = (ctypes.c_void_p * 1)(v.data_ptr())
        assert call(fn, [member()], gates=gates, pp=None) == EINVAL
        assert call(fn, [member()], gates=None, pp=p.data_ptr()) == EINVAL
    assert float(y.abs().sum()) == 0.0
