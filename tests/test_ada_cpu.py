"""CPU: the adaptive strength of the discriminator's augmentation (--D_aug_p / --D_ada) — the flags and their rules,
the gated restatement and the controller restatement (tests/ada_cases.py) the GPU tests compare the kernels against, the host
draw order with gate blocks, the controller state in checkpoints, and the argument checks of the three new entry points.
No kernel is launched here."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import ada_cases as AC
import diffaug_cases as DA
from txt2vid_amd import functional_aug as A

F32 = np.float32


# ------------------------------------------------------------------------------------------------ flags
def _parse(argv):
    from txt2vid_amd.gan.trainer import add_params_to_parser
    from txt2vid_amd.gan.ada import check_args
    return check_args(add_params_to_parser(argparse.ArgumentParser()).parse_args(argv))


def test_flags_parse_and_default_to_off():
    a = _parse([])
    assert a.D_aug_p is None and a.D_ada is None and a.D_ada_interval == 4 and a.D_ada_kclips == 500
    a = _parse(['--D_aug', DA.FULL])
    assert a.D_aug_p is None and a.D_ada is None                    # --D_aug alone: nothing resolved, the ungated path
    a = _parse(['--D_aug', 'cutout', '--D_aug_p', '0.25'])
    assert a.D_aug_p == 0.25 and a.D_ada is None
    a = _parse(['--D_aug', DA.FULL, '--D_ada', '0.6'])
    assert a.D_ada == 0.6 and a.D_aug_p == 0.0                      # with the controller p starts at 0
    a = _parse(['--D_aug', DA.FULL, '--D_ada', '0.6', '--D_aug_p', '0.5', '--D_ada_interval', '1', '--D_ada_kclips', '0.016'])
    assert (a.D_ada, a.D_aug_p, a.D_ada_interval, a.D_ada_kclips) == (0.6, 0.5, 1, 0.016)
    for edge in ('0', '1', '0.0', '1.0'):
        assert _parse(['--D_aug', 'color', '--D_aug_p', edge]).D_aug_p == float(edge)


@pytest.mark.parametrize('argv', [['--D_aug_p', '0.5'], ['--D_ada', '0.6'], ['--D_aug', '', '--D_ada', '0.6'],
                                  ['--D_aug', '', '--D_aug_p', '1.0']])
def test_either_flag_needs_a_policy(argv):
    with pytest.raises(ValueError, match='D_aug'):
        _parse(argv)


@pytest.mark.parametrize('argv,flag', [(['--D_aug_p', '1.5'], '--D_aug_p'), (['--D_aug_p', '-0.1'], '--D_aug_p'),
                                       (['--D_ada', '0'], '--D_ada'), (['--D_ada', '1'], '--D_ada'), (['--D_ada', '1.2'], '--D_ada'),
                                       (['--D_ada_interval', '0'], '--D_ada_interval'), (['--D_ada_kclips', '0'], '--D_ada_kclips'),
                                       (['--D_ada_kclips', '-3'], '--D_ada_kclips')])
def test_out_of_range_values_are_argparse_errors(argv, flag, capsys):
    with pytest.raises(SystemExit):
        _parse(['--D_aug', DA.FULL] + argv)
    assert flag in capsys.readouterr().err


def test_data_parallel_refusal_and_help_text():
    from txt2vid_amd.gan.trainer import add_params_to_parser, TrainStep
    from txt2vid_amd.gan.ada import check_args, AdaState
    import schedule_cases as S
    parser = add_params_to_parser(argparse.ArgumentParser())
    args = parser.parse_args(['--D_aug', DA.FULL, '--D_ada', '0.6'])
    with pytest.raises(ValueError, match='data-parallel'):
        check_args(args, world=2)
    check_args(parser.parse_args(['--D_aug', DA.FULL, '--D_aug_p', '0.5']), world=2)       # a fixed p needs no exchange
    # the trainer refuses a gradient exchange next to a controller, whatever built it

    class Gan(object):
        gen = object()
    gan = Gan()
    gan.ada = AdaState(0.6)
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    prm.D_aug = DA.FULL
    with pytest.raises(ValueError, match='data-parallel'):
        TrainStep(gan, None, None, None, prm, 'cpu', grad_sync=lambda which: None)
    ts = TrainStep(gan, None, None, None, prm, 'cpu')
    assert ts.gated and ts.ada is gan.ada
    prm.D_aug = ''
    with pytest.raises(ValueError):
        TrainStep(gan, None, None, None, prm, 'cpu')                # a controller without a policy
    text = ' '.join(parser.format_help().split())
    assert 'untuned' in text or 'tuned' in text


def test_trainer_gating_rules():
    """--D_aug alone and --D_aug_p 1.0 are the ungated path; p < 1 or a controller turn the gates on."""
    from txt2vid_amd.gan.trainer import TrainStep
    import schedule_cases as S

    class Gan(object):
        gen = object()
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    assert not TrainStep(Gan(), None, None, None, prm, 'cpu').gated
    prm.D_aug = DA.FULL
    assert not TrainStep(Gan(), None, None, None, prm, 'cpu').gated
    prm.D_aug_p = 1.0
    assert not TrainStep(Gan(), None, None, None, prm, 'cpu').gated
    prm.D_aug_p = None
    assert not TrainStep(Gan(), None, None, None, prm, 'cpu').gated
    prm.D_aug_p = 0.5
    ts = TrainStep(Gan(), None, None, None, prm, 'cpu')
    assert ts.gated and ts.ada is None and ts._p.tolist() == [0.5]
    prm.D_aug = ''
    with pytest.raises(ValueError):
        TrainStep(Gan(), None, None, None, prm, 'cpu')


# ------------------------------------------------------------------------------------------------ the gated restatement
def _clips(C_=1, N=8, S_=16, seed=3):
    g = torch.Generator()
    g.manual_seed(seed)
    x = torch.rand(N, C_, 2, S_, S_, generator=g, dtype=torch.float64) * 2 - 1
    return x, torch.rand(N, A.K, generator=g), torch.rand(N, A.K, generator=g)


@pytest.mark.parametrize('policy', DA.SUBSETS)
@pytest.mark.parametrize('C_', [1, 3])
def test_restatement_at_p_one_and_p_zero(policy, C_):
    x, u, g = _clips(C_)
    assert torch.equal(AC.augment(x, u, g, 1.0, policy), DA.augment(x, u, policy))          # every gate in [0, 1) is < 1
    assert torch.equal(AC.augment(x, u, g, 0.0, policy), x)                                 # none is < 0
    xs = [x, x[::2, :, :, ::2, ::2].contiguous()]
    for a, b in zip(AC.augment_pyramid(xs, u, g, 1.0, policy), DA.augment_pyramid(xs, u, policy)):
        assert torch.equal(a, b)


def test_restatement_gates_per_clip_and_per_transformation():
    """All 8 subsets of the full policy, one per clip; a gate EQUAL to p does not apply; the gate row follows the stride."""
    x, u, g = _clips(3)
    p = 0.5
    for j in range(8):
        for k in range(3):
            g[j, k] = 0.25 if (j >> k) & 1 else 0.75
    g[7, 1] = p                                                     # equal: translation is off for clip 7
    want = [0, 1, 2, 3, 4, 5, 6, 5]
    assert AC.effective_policies(g, p, DA.FULL, 8) == want
    assert AC.effective_policies(g, p, 'color,cutout', 8) == [w & 5 for w in want]
    assert AC.effective_policies(g, p, DA.FULL, 4, stride=2) == want[::2]
    y = AC.augment(x, u, g, p, DA.FULL)
    for j, bits in enumerate(want):
        ref = x[j:j + 1] if bits == 0 else DA.augment(x[j:j + 1], u[j:j + 1], bits)
        assert torch.equal(y[j:j + 1], ref)
    # the adjoint of a copied clip is a copy; that of the others is diffaug_cases' adjoint
    xr = x.clone().requires_grad_(True)
    gy = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    gx, = torch.autograd.grad(AC.augment(xr, u, g, p, DA.FULL), xr, gy)
    assert torch.equal(gx[0], gy[0])
    x5 = x[5:6].clone().requires_grad_(True)
    g5, = torch.autograd.grad(DA.augment(x5, u[5:6], 5), x5, gy[5:6])
    assert torch.equal(gx[5:6], g5)
    # fp32 comparison: the largest float32 below p is < p, p itself is not
    below = float(np.nextafter(F32(p), F32(0)))
    g2 = torch.full((1, A.K), p)
    g2[0, 0] = below
    assert AC.effective_policies(g2, p, DA.FULL, 1) == [1]


# ------------------------------------------------------------------------------------------------ the controller restatement
def test_controller_clamps_holds_and_counts_ties_zero():
    step = AC.step_size(4, 1, 0.016)
    assert step == F32(0.25)
    ada = AC.controller_init(0.5)
    for want in (0.75, 1.0, 1.0, 1.0):                              # r_t = 1 > target: up, then clamped at 1
        AC.controller_step(ada, 8, 8, 0.6, step, 1)
        assert ada.tolist() == [want, 0, 0, 0, 0, 0, 0, 0]
    for want in (0.75, 0.5, 0.25, 0.0, 0.0):                        # r_t = -1: down, then clamped at 0
        AC.controller_step(ada, -8, 8, 0.6, step, 1)
        assert ada[0] == F32(want)
    # r_t == target leaves p where it is (and still clears the window): 4 / 8 = 0.5 exactly
    ada = AC.controller_init(0.5)
    AC.controller_step(ada, 4, 8, 0.5, step, 1)
    assert ada.tolist() == [0.5, 0, 0, 0, 0, 0, 0, 0]
    # a window of 4 steps: the sums accumulate, p moves on the 4th
    ada = AC.controller_init(0.25)
    for k in range(3):
        AC.controller_step(ada, 2, 8, 0.6, step, 4)
        assert ada[:4].tolist() == [0.25, 2 * (k + 1), 8 * (k + 1), k + 1]
    AC.controller_step(ada, 8, 8, 0.6, step, 4)                     # (6 + 8) / 32 < 0.6: down
    assert ada[:4].tolist() == [0.0, 0, 0, 0]
    # ties count 0, in the sum and towards the pairs
    s, n = AC.sign_sum([np.array([1.0, 2.0, 3.0, -1.0], dtype=F32), np.array([0.5], dtype=F32)],
                       [np.array([1.0, 1.0, 4.0, -1.0], dtype=F32), np.array([0.5], dtype=F32)])
    assert (s, n) == (0, 5)
    # a step that is no dyadic fraction: the update is ONE float32 addition
    step = AC.step_size(32, 4, 500)
    ada = AC.controller_init(0.1)
    AC.controller_step(ada, 5, 5, 0.6, step, 1)
    assert ada[0] == F32(F32(0.1) + step) and ada[1:4].tolist() == [0, 0, 0]
    from txt2vid_amd.gan.ada import step_size
    assert F32(step_size(32, 4, 500)) == step


# ------------------------------------------------------------------------------------------------ draw order
def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


@pytest.mark.parametrize('N,M', [(1, 1), (2, 2)])
@pytest.mark.parametrize('cond,ca_dim', [(False, 0), (True, 3)])
def test_gated_draw_order(N, M, cond, ca_dim):
    """With gating on the host RNG sequence is u, g, u, g, ... at the call sites of --D_aug; HostDraws and StaticDraws hand out
    the same values; each gate block sits directly behind its parameter block in the staging buffer. With gating off the
    sequence, the buffer and the generator state are those of --D_aug alone."""
    from txt2vid_amd.draws import HostDraws, StaticDraws
    B, L, nl, ng = 5, 7, 4, 3
    X = 2 * N + M + 1
    perms = (N + 1) if cond else 0
    kw = dict(n_gen_phases=ng, gp=True, subsample_input=True, n_perms=perms, n_d_steps=N, n_g_steps=M, ca_dim=ca_dim)
    args = (B, L, nl, ng, N, M, True, ca_dim)
    _seed(11)
    want = AC.consume(HostDraws(), *args, gated=True)
    host_state = torch.get_rng_state()
    # the sequence on the raw generator: every aug site is two consecutive torch.rand(B, K)
    _seed(11)
    sd = StaticDraws('cpu', B, L, nl, n_aug=2 * X, **kw)
    assert sd.gated and sd.n_aug == 2 * X
    sd.begin_step()
    assert torch.equal(torch.get_rng_state(), host_state)
    got = AC.consume(sd, *args, gated=True)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    with pytest.raises(AssertionError):
        sd.aug(B, 'cpu', gated=True)                                # 2N + M + 1 pairs per iteration, no more
    blocks = [t for t in got if torch.is_tensor(t) and tuple(t.shape) == (B, A.K)]
    assert len(blocks) == 2 * X
    for k, t in enumerate(blocks):                                  # u0 g0 u1 g1 ... in one staging buffer
        assert torch.equal(sd.d_u[k], t)
    assert sd.d_u.data_ptr() + B * A.K * 4 == sd.d_u[1].data_ptr()
    # against the ungated sequence: the same values at the non-aug sites as long as no block has been drawn, and the ungated
    # layout itself is today's
    _seed(11)
    plain_want = DA.consume(HostDraws(), *args, n_perms=perms, aug=True)
    state_plain = torch.get_rng_state()
    _seed(11)
    un = StaticDraws('cpu', B, L, nl, n_aug=X, **kw)
    assert not un.gated
    un.begin_step()
    assert torch.equal(torch.get_rng_state(), state_plain)
    for a, b in zip(DA.consume(un, *args, n_perms=perms, aug=True), plain_want):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert sd.d_all.numel() == un.d_all.numel() + X * B * A.K
    with pytest.raises(AssertionError):
        un.rewind() or un.aug(B, 'cpu', gated=True)                 # an ungated buffer hands out no gates
    # gating on: the first parameter block is the ungated one, its gate block is what the ungated run draws next
    first = [t for t in plain_want if torch.is_tensor(t) and tuple(t.shape) == (B, A.K)]
    assert torch.equal(blocks[0], first[0]) and torch.equal(blocks[1], first[1])


def test_ungated_draws_are_byte_identical_to_before():
    """The ungated sequence restated on the raw generator (the order of DESIGN §17): HostDraws.aug is one torch.rand(B, K)."""
    from txt2vid_amd.draws import HostDraws, StaticDraws
    torch.manual_seed(4)
    u = HostDraws().aug(3, 'cpu')
    state = torch.get_rng_state()
    torch.manual_seed(4)
    assert torch.equal(u, torch.rand(3, A.K)) and torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(4)
    u, g = HostDraws().aug(3, 'cpu', gated=True)
    torch.manual_seed(4)
    assert torch.equal(u, torch.rand(3, A.K)) and torch.equal(g, torch.rand(3, A.K))
    with pytest.raises(ValueError):
        StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=11)
    assert StaticDraws('cpu', 4, 8, 4, n_d_steps=2, n_g_steps=1, n_aug=12).gated


# ------------------------------------------------------------------------------------------------ checkpoints
class _Module(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))


def _gan(ada):
    from txt2vid_amd.gan.cond_gan import CondGan
    gan = CondGan(gen=_Module(), discrims=[_Module()], discrim_names=['video'])
    assert gan.ada is None
    gan.ada = ada
    return gan


def test_ada_state_round_trips_through_a_checkpoint():
    from txt2vid_amd.gan.ada import AdaState
    a = AdaState(0.6, interval=4, kclips=500, p0=0.125)
    assert a.ada.dtype == torch.float32 and a.ada.tolist() == [0.125, 0, 0, 0, 0, 0, 0, 0]
    assert (a.target, a.interval, a.kclips, a.p0) == (0.6, 4, 500.0, 0.125)
    a.ada.copy_(torch.tensor([0.375, -3, 14, 2, 0, 0, 0, 0]))
    assert a.p.tolist() == [0.375]                                  # p is a view of the state
    saved = _gan(a).save_dict()
    assert saved['ada']['ada'].dtype == torch.float32 and saved['ada']['ada'].device.type == 'cpu'
    assert saved['ada']['ada'].tolist() == [0.375, -3, 14, 2, 0, 0, 0, 0]
    # key and state: restored, in place
    b = AdaState(0.6, p0=0.5)
    view = b.p
    _gan(b).load_from_dict(saved)
    assert b.ada.tolist() == [0.375, -3, 14, 2, 0, 0, 0, 0] and view.tolist() == [0.375]
    # no key: p0 and an empty window, whatever the state held
    plain = _gan(None).save_dict()
    assert 'ada' not in plain
    b.ada[1] = 5
    _gan(b).load_from_dict(plain)
    assert b.ada.tolist() == [0.5, 0, 0, 0, 0, 0, 0, 0]
    # a key without a state: ignored
    g = _gan(None)
    g.load_from_dict(saved)
    assert g.ada is None
    with pytest.raises(ValueError):
        AdaState(1.0)
    with pytest.raises(ValueError):
        AdaState(0.6, interval=0)
    with pytest.raises(ValueError):
        b.load_state_dict({'ada': torch.zeros(4)})
    with pytest.raises(RuntimeError):
        b.observe([torch.zeros(4)], [torch.zeros(4)])               # no CPU fallback


# ------------------------------------------------------------------------------------------------ argument checks
def test_new_entry_points_validate_without_a_device():
    """Bad arguments are refused on the host side (negative status) before any launch; no device is touched. The pointers are
    never dereferenced on the refused paths, so host addresses stand in for device ones."""
    from txt2vid_amd._lib import lib, AugMember, AdaLevel, MAX_GROUPS
    l = lib()
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)

    def members(n=1, **kw):
        arr = (AugMember * max(1, n))()
        for a in arr:
            a.x, a.y, a.u = addr, addr + 128, addr
            a.N, a.C, a.T, a.S, a.row_stride, a.rows, a.policy = 1, 1, 1, 2, 1, 1, 7
            for k, v in kw.items():
                setattr(a, k, v)
        return arr
    gates = (C.c_void_p * MAX_GROUPS)(*([addr] * MAX_GROUPS))
    for fn in (l.t2v_diffaug_gated_fwd, l.t2v_diffaug_gated_bwd):
        assert fn(None, gates, 1, addr, None) < 0
        assert fn(members(), None, 1, addr, None) < 0               # gates == NULL
        assert fn(members(), gates, 1, None, None) < 0              # p == NULL
        assert fn(members(), gates, 0, addr, None) < 0
        assert fn(members(MAX_GROUPS + 1), gates, MAX_GROUPS + 1, addr, None) < 0
        for bad in (dict(policy=0), dict(policy=8), dict(x=None), dict(u=None), dict(y=addr), dict(N=0), dict(S=0),
                    dict(row_stride=0), dict(N=2)):
            assert fn(members(**bad), gates, 1, addr, None) < 0, bad

    def levels(n=1, **kw):
        arr = (AdaLevel * max(1, n))()
        for a in arr:
            a.real, a.fake, a.count = addr, addr, 4
            for k, v in kw.items():
                setattr(a, k, v)
        return arr
    f = l.t2v_ada_update
    assert f(None, levels(), 1, 0.6, 0.25, 1, None) < 0
    assert f(addr, None, 1, 0.6, 0.25, 1, None) < 0
    assert f(addr, levels(), 0, 0.6, 0.25, 1, None) < 0
    assert f(addr, levels(MAX_GROUPS + 1), MAX_GROUPS + 1, 0.6, 0.25, 1, None) < 0
    assert f(addr, levels(count=0), 1, 0.6, 0.25, 1, None) < 0
    assert f(addr, levels(real=None), 1, 0.6, 0.25, 1, None) < 0
    assert f(addr, levels(fake=None), 1, 0.6, 0.25, 1, None) < 0
    assert f(addr, levels(), 1, 0.6, 0.25, 0, None) < 0             # interval < 1
    assert f(addr, levels(), 1, 0.6, -0.25, 1, None) < 0
    assert f(addr, levels(), 1, 0.6, float('inf'), 1, None) < 0
    assert f(addr, levels(), 1, 0.6, float('nan'), 1, None) < 0
    assert all(v == 0 for v in buf)
