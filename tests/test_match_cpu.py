"""CPU: the opt-in contrastive clip-caption matching term (Resnet3D(match=True), --D_match / --G_match) — the
restatement's own rounding against the bound and the precondition that makes its counts exact, the flags' rules, the two JSON --D
specs, state-dict layout and refusals, the draws `init()` leaves alone, the log line, the read-out's widths, and the host-side
refusals of the entry points."""
import argparse
import os

import pytest
import torch

import match_cases as MC
from oracle import tganv2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = MC.PRE


def _discrim(**kw):
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    return MultiScaleDiscrim(num_channels=1, cond_dim=256, **kw)


def _shapes(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


# ------------------------------------------------------------------------------------------------ the restatement

def test_restatement_rounding_sits_well_inside_the_bound():
    """fp32 against float64 of the same restatement on every op case: the worst ratio to the bound is printed and must leave a
    factor of 4; the counts agree exactly."""
    worst = {}
    for v in MC.VARIANTS:
        ref, got = MC.case_reference(*v), MC.reference(*v, dtype=torch.float32)
        assert got['stats'] == ref['stats'], (v, got['stats'], ref['stats'])
        for f in MC.FIELDS:
            r = MC.NC.ratio(got[f], ref[f], MC.TOL)
            if r >= worst.get(f, (0.0,))[0]:
                worst[f] = (r, v)
    for f, w in sorted(worst.items()):
        print('match-restatement fp32/fp64 worst ratio %s %.4g at %s' % (f, w[0], w[1]))
    assert set(worst) == set(MC.FIELDS) and all(w[0] <= 0.25 for w in worst.values()), worst


@pytest.mark.parametrize('v', MC.VARIANTS, ids=MC.IDS)
def test_every_top1_margin_is_100x_the_score_error_bound(v):
    """No row or column of member 0 can flip, so the accuracies and the masked count are compared for equality. A zero-norm
    feature or caption row (the `zero` variant plants both at the last row) makes that row and that column exact zeros in every
    precision: S_ii > S_ij is a tie there, a miss on every implementation; those are the only margins below the bound."""
    case, tau, variant = v
    ref, inp = MC.case_reference(*v), MC.inputs(case, variant)
    Sd, M = ref['S'][0], inp['M'][0]
    mr, mc = MC.margins(Sd, M)
    b = Sd.shape[0]
    need = 100 * MC.s_bound(tau)
    for i in range(b):
        dead = variant == 'zero' and i == b - 1
        if dead:
            assert not Sd[i].any() and not Sd[:, i].any() and float(mr[i]) == 0.0 and float(mc[i]) == 0.0
        else:
            assert abs(float(mr[i])) > need and abs(float(mc[i])) > need, (i, float(mr[i]), float(mc[i]), need)
    # and the planted structure shows: some hits, and (from 3 rows on) some misses
    if variant == 'plain' and b >= 3:
        assert 0 < ref['stats'][0] < 1


def test_restatement_matches_its_definition():
    """Against loops written straight from the issue's formulas (no maximum subtraction, F.normalize), float64, tau = 1."""
    inp = MC.inputs('odd', 'dup')
    f, s, W = inp['f'][0].double(), inp['s'][0].double(), inp['W'].double()
    e = (f @ W).requires_grad_(True)
    eh, sh = torch.nn.functional.normalize(e, dim=1, eps=1e-12), torch.nn.functional.normalize(s, dim=1, eps=1e-12)
    S = eh @ sh.t()
    b = 3
    M = [[i == j or not torch.equal(s[i], s[j]) for j in range(b)] for i in range(b)]
    assert sum(not m for row in M for m in row) == 2
    L = sum(-S[i, i] + torch.log(sum(torch.exp(S[i, j]) for j in range(b) if M[i][j])) for i in range(b))
    Lc = sum(-S[j, j] + torch.log(sum(torch.exp(S[i, j]) for i in range(b) if M[i][j])) for j in range(b))
    want = (L + Lc) / (2 * b)
    gE, = torch.autograd.grad(want, e)
    e2 = e.detach().clone().requires_grad_(True)
    term, stats, C, _ = MC.parts(e2, s, 1.0)
    assert abs(float(term.detach()) - float(want.detach())) < 1e-12 and stats[2] == 2.0
    g2, = torch.autograd.grad(term, e2)
    assert torch.allclose(g2, gE, rtol=1e-10, atol=1e-12)
    # the adjoint as DESIGN states it: dE_i = (dEh_i - eh_i <eh_i, dEh_i>) / |e_i| with dEh = C Sh
    dEh = C @ sh
    ehd = eh.detach()
    want_g = (dEh - ehd * (ehd * dEh).sum(1, keepdim=True)) / e.detach().norm(dim=1, keepdim=True)
    assert torch.allclose(g2, want_g, rtol=1e-10, atol=1e-12)


def test_degenerate_cases_are_exact():
    for v in (('one', 0.1, 'plain'), ('odd', 0.1, 'same'), ('pyramid', 0.1, 'same')):
        ref = MC.case_reference(*v)
        assert float(ref['term']) == 0.0 and not ref['gE'].any() and not ref['gW'].any() and not ref['C'].any(), v
        b = MC.CASES[v[0]][0][0]
        assert ref['stats'] == (1.0, 1.0, float(b * (b - 1) if v[2] == 'same' else 0))
    # a zero feature row: finite everywhere, its adjoint exactly zero (the others' not)
    ref = MC.case_reference('odd', 0.1, 'zero')
    assert all(bool(torch.isfinite(ref[f]).all()) for f in MC.FIELDS)
    assert not ref['gE'][-1].any() and ref['gE'][:-1].any()


# ------------------------------------------------------------------------------------------------ flags

def _args(**kw):
    ns = argparse.Namespace(D_match=None, G_match=None, match_tau=None, D=['spec'], D_names=None, dont_use_sent=False, end2end=False)
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def test_check_args():
    from txt2vid_amd.gan.match import check_args, enabled
    a = check_args(_args())
    assert not enabled(a) and a.match_tau is None
    assert check_args(_args(D_match=1.0)).match_tau == 0.1
    assert check_args(_args(G_match=0.5, match_tau=0.05)).match_tau == 0.05
    assert enabled(check_args(_args(D_match=2.0, G_match=1.0), world=4))             # data-parallel runs are allowed
    assert check_args(argparse.Namespace()) is not None                               # no attributes: off
    for bad in (dict(match_tau=0.1), dict(D_match=0.0), dict(G_match=-1.0), dict(D_match=float('inf')), dict(G_match=float('nan')),
                dict(D_match=1.0, match_tau=0.0), dict(D_match=1.0, match_tau=float('inf')), dict(D_match=1.0, D=['a', 'b']),
                dict(G_match=1.0, D_names=['a', 'b']), dict(D_match=1.0, dont_use_sent=True)):
        with pytest.raises(ValueError):
            check_args(_args(**bad))
    with pytest.raises(NotImplementedError, match='end2end'):
        check_args(_args(D_match=1.0, end2end=True))


def test_parser_has_the_flags():
    from txt2vid_amd.train.gan import build_parser
    base = ['--data', 'd', '--G', 'g', '--D', 'd']
    a = build_parser().parse_args(base)
    assert a.D_match is None and a.G_match is None and a.match_tau is None
    a = build_parser().parse_args(base + ['--D_match', '1', '--G_match', '0.5', '--match_tau', '0.05'])
    assert (a.D_match, a.G_match, a.match_tau) == (1.0, 0.5, 0.05)
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ['--D_match', '0'])


def test_flags_need_the_head_and_the_head_needs_flags():
    from txt2vid_amd.gan.match import check_discrims
    on, off = _discrim(match=True), _discrim()
    check_discrims(_args(D_match=1.0), [on])
    check_discrims(_args(), [off])
    check_discrims(_args(), [on], training=False)                  # sampling and evaluation load such a checkpoint without flags
    with pytest.raises(ValueError, match='match=True'):
        check_discrims(_args(G_match=1.0), [off])
    with pytest.raises(ValueError, match='--D_match'):
        check_discrims(_args(), [on])


def test_train_step_refuses_end2end():
    from txt2vid_amd.gan.match import MatchState
    from txt2vid_amd.gan.trainer import TrainStep

    class Gan(object):
        gen, ada = torch.nn.Linear(1, 1), None
        match = MatchState(1.0, None, 0.1)

    class Prm(object):
        discrim_steps = gen_steps = 1
    with pytest.raises(NotImplementedError, match='end2end'):
        TrainStep(Gan(), None, None, None, Prm(), 'cpu', end2end=True)


# ------------------------------------------------------------------------------------------------ specs and modules

@pytest.mark.parametrize('name,proj', [('discrim_cond_match.json', False), ('discrim_cond_proj_match.json', True)])
def test_json_specs_build_the_model(name, proj):
    from txt2vid_amd.util.reflection import create_object
    d = create_object(os.path.join(ROOT, 'tools', 'cfg', name), cond_dim=256)
    assert type(d).__module__ == 'txt2vid_amd.models.tganv2_cond.discrim'
    assert d.match_on and d.proj_on == proj and tuple(d.match_head().weight.shape) == (1024, 256)
    assert list(d.state_dict())[-1] == PRE + 'match.weight'
    assert d.single_discrim.module.res_block.inner_module[0].weight.shape[1] == 1


def test_match_off_is_todays_module():
    want = O.resnet3d_shapes(PRE, 1, 64, 256)
    m = _discrim()
    assert not m.match_on and m.match_head() is None
    assert _shapes(_discrim(match=False)) == _shapes(m)
    assert {k: s for k, s in _shapes(m)} == {k: tuple(v) for k, v in want.items()}


def test_match_on_adds_one_trailing_key_behind_every_other_head():
    on, off = _shapes(_discrim(match=True)), _shapes(_discrim())
    assert on[:-1] == off and on[-1] == (PRE + 'match.weight', (1024, 256))
    full, rest = _shapes(_discrim(match=True, proj=True, mbstd=4)), _shapes(_discrim(proj=True, mbstd=4))
    assert full[:-1] == rest and full[-1][0] == PRE + 'match.weight'
    assert not any('ones' in k for k, _ in on)                     # the constant vector is no checkpoint entry


def test_w_is_drawn_from_its_own_generator():
    """N(0, 1/K) under a seed that is a constant of the code: the same W whatever the global generator holds, which does not move."""
    from txt2vid_amd.models.resnet3d import CondMatch
    torch.manual_seed(1)
    state = torch.get_rng_state()
    a = CondMatch(1024, 256).weight.detach()
    assert torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(2)
    assert torch.equal(CondMatch(1024, 256).weight.detach(), a)
    assert abs(float(a.std()) - 1024 ** -0.5) < 0.02 * 1024 ** -0.5 and abs(float(a.mean())) < 1e-3
    assert float(a.abs().min()) >= 0 and bool(a.any())


@pytest.mark.parametrize('method', ['xavier', 'ortho', 'normal'])
def test_init_walks_past_the_head_and_every_other_draw_is_unchanged(method):
    from txt2vid_amd.models.resnet3d import Resnet3D, CondMatch
    from txt2vid_amd.util.torch.init import init
    kw = dict(num_channels=1, mid_ch=8, cond_dim=6, num_down_blocks=2)
    torch.manual_seed(11)
    a = Resnet3D(**kw)
    init(a, method)
    torch.manual_seed(11)
    b = Resnet3D(match=True, **kw)
    w0 = b.match.weight.detach().clone()
    init(b, method)
    sa, sb = a.state_dict(), b.state_dict()
    assert torch.equal(sb['match.weight'], w0) and tuple(w0.shape) == (256, 6) and torch.equal(w0, CondMatch(256, 6).weight.detach())
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and set(sb) - set(sa) == {'match.weight'}
    assert not any(tag in type(b.match).__name__ for tag in ('Linear', 'Conv', 'Embedding', 'BatchNorm'))
    assert not isinstance(b.match, (torch.nn.Linear, torch.nn.Conv3d))         # --D_sn walks past it


def test_refusals_use_projs_rules():
    from txt2vid_amd.models.resnet3d import Resnet3D
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim as Uncond
    with pytest.raises(ValueError, match='dont_use_sent'):
        Resnet3D(num_channels=1, cond_dim=0, match=True)
    with pytest.raises(ValueError, match='dont_use_sent'):
        MultiScaleDiscrim(num_channels=1, cond_dim=0, match=True)
    with pytest.raises(ValueError, match='text-conditioned'):
        Uncond(num_channels=1, match=True)
    with pytest.raises(ValueError, match='text-conditioned'):
        Uncond(num_channels=1, cond_dim=256, match=True)
    with pytest.raises(ValueError, match='single_discrim'):
        MultiScaleDiscrim(num_channels=1, cond_dim=256, match=True, single_discrim=False)


@pytest.mark.parametrize('saved,built', [(True, False), (False, True)])
def test_checkpoint_match_mismatch_is_refused_everywhere(saved, built):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.models.resnet3d import Resnet3D
    sd = _discrim(match=saved).state_dict()
    with pytest.raises(ValueError, match='match=%s' % built):
        _discrim(match=built).load_state_dict(sd)
    kw = dict(num_channels=1, mid_ch=8, cond_dim=6, num_down_blocks=2)
    with pytest.raises(ValueError, match='match=%s' % built):
        Resnet3D(match=built, **kw).load_state_dict(Resnet3D(match=saved, **kw).state_dict())
    gan = CondGan(gen=torch.nn.Linear(1, 1), discrims=[_discrim(match=built)], discrim_names=['video'])
    with pytest.raises(ValueError, match='match=%s' % built):
        gan.load_from_dict({'gen': gan.gen.state_dict(), 'video': sd})


def test_checkpoint_round_trip_with_match():
    a, b = _discrim(match=True), _discrim(match=True)
    with torch.no_grad():
        a.match_head().weight.normal_()
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.match_head().weight, b.match_head().weight)
    from txt2vid_amd.gan.cond_gan import CondGan
    gan = CondGan(gen=torch.nn.Linear(1, 1), discrims=[_discrim(match=True)], discrim_names=['video'])
    assert gan.match is None
    gan.load_from_dict({'gen': gan.gen.state_dict(), 'video': a.state_dict()})
    assert torch.equal(gan.discrims[0].match_head().weight, a.match_head().weight)
    # the evaluation's feature network takes the trunk of such a checkpoint: the head's key is dropped with the other heads'
    from txt2vid_amd.gan.kid import HEAD_KEYS
    assert 'match.weight'.startswith(HEAD_KEYS)


# ------------------------------------------------------------------------------------------------ the extras seam

def test_log_lines():
    from txt2vid_amd.gan.match import MatchState
    both = MatchState(1.0, 0.5, 0.1)
    vals = {'match_d': [1.2345, 0.75, 0.6875, 2.0], 'match_g': [2.5, 0.3125, 0.28125, 2.0]}
    assert both.log_lines(7, vals) == ['Iter 7, Match (tau 0.1): D term 1.2345, real acc 0.750 / 0.688, G term 2.5000, '
                                       'fake acc 0.312 / 0.281, masked 2']
    d_only = MatchState(1.0, None, 0.05)
    assert d_only.log_lines(3, vals) == ['Iter 3, Match (tau 0.05): D term 1.2345, real acc 0.750 / 0.688, masked 2']
    g_only = MatchState(None, 2.0)
    assert g_only.log_lines(3, vals) == ['Iter 3, Match (tau 0.1): G term 2.5000, fake acc 0.312 / 0.281, masked 2']
    assert both.log_lines(1, {}) == [] and both.key is None
    assert [s[0] for s in both.slots] == ['match_d', 'match_g'] and [s[0] for s in d_only.slots] == ['match_d']
    assert [s[0] for s in g_only.slots] == ['match_g']
    for bad in (dict(lam_d=None, lam_g=None), dict(lam_d=0.0), dict(lam_g=float('nan')), dict(lam_d=1.0, tau=0.0)):
        with pytest.raises(ValueError):
            MatchState(**bad)


def test_readout_widths_and_extras_order():
    from txt2vid_amd.gan.extras import Readout, training_extras, LOSSES
    from txt2vid_amd.gan.match import MatchState
    from txt2vid_amd.gan.lecam import LeCamState

    class Opt(object):
        lr_sched = grad_guard = None

    class Gan(object):
        ada = None
        lecam = LeCamState(0.3)
        match = MatchState(1.0, 1.0, 0.1)
    ex = training_extras(Gan(), Opt(), Opt())
    assert ex == [Gan.lecam, Gan.match]
    r = Readout(ex, 'cpu')
    assert [s[0] for s in r.slots] == list(LOSSES) + ['lecam', 'match_d', 'match_g']
    assert [s[1] for s in r.slots][-2:] == [3 + 20, 3 + 20 + 4] and r.width == 32
    Gan.match = MatchState(None, 1.0)
    r = Readout(training_extras(Gan(), Opt(), Opt()), 'cpu')
    assert r.width == 28 and [s[0] for s in r.slots][-1] == 'match_g'
    Gan.match.stats_g.copy_(torch.tensor([1.5, 0.5, 0.25, 0.0]))
    r.push(0, lD=torch.tensor(1.0), lG=torch.tensor(2.0))
    r.push(1, lD=torch.tensor(1.0), lG=torch.tensor(2.0))
    assert r.pop()['match_g'] == [1.5, 0.5, 0.25, 0.0]
    Gan.match = None
    assert Readout(training_extras(Gan(), Opt(), Opt()), 'cpu').width == 24          # off: the width of before


# ------------------------------------------------------------------------------------------------ host-side refusals

def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-side checks only, through the library cross-compiled for gfx950: null pointers, n outside 1..T2V_MAX_GROUPS, b outside
    1..128, J outside 1..1024, a temperature that is not positive and finite."""
    import ctypes as C
    from txt2vid_amd._lib import lib, MatchMember, MAX_GROUPS, MATCH_MAX_ROWS, MATCH_MAX_COLS
    L = lib()
    p = 16                                                         # never dereferenced: every call below is refused first
    EINVAL = -1                                                    # T2V_EINVAL: a launch status would be -1000 or below
    assert (MATCH_MAX_ROWS, MATCH_MAX_COLS) == (128, 1024)
    header = open(os.path.join(ROOT, 'include', 't2v_hip.h')).read()
    assert '#define T2V_MATCH_MAX_ROWS 128' in header and '#define T2V_MATCH_MAX_COLS 1024' in header
    assert C.sizeof(MatchMember) == 5 * 8 + 2 * 4

    def members(n=1, b=2, **null):
        arr = (MatchMember * max(n, 1))()
        for a in arr:
            a.e, a.s, a.coef, a.norms, a.de, a.b = p, p, p, p, p, b
            for k in null:
                setattr(a, k, None)
        return arr
    P = C.c_void_p(p)
    fwd = lambda m, n, J=4, tau=0.1, stats=P, out=P: L.t2v_match_fwd(m, n, J, tau, stats, out, None)
    bwd = lambda m, n, J=4, g=P, scale=1.0: L.t2v_match_bwd(m, n, J, scale, g, None)
    for fn in (fwd, bwd):
        assert fn(None, 1) == EINVAL
        assert fn(members(), 0) == EINVAL and fn(members(MAX_GROUPS + 1), MAX_GROUPS + 1) == EINVAL
        assert fn(members(b=0), 1) == EINVAL and fn(members(b=129), 1) == EINVAL and fn(members(2, b=-1), 2) == EINVAL
        assert fn(members(), 1, 0) == EINVAL and fn(members(), 1, 1025) == EINVAL and fn(members(), 1, -3) == EINVAL
        for k in ('e', 's', 'coef', 'norms'):
            assert fn(members(**{k: None}), 1) == EINVAL, k
    assert bwd(members(de=None), 1) == EINVAL and bwd(members(), 1, g=None) == EINVAL
    for scale in (0.0, -1.0, 1.5, float('nan')):
        assert bwd(members(), 1, scale=scale) == EINVAL, scale
    assert fwd(members(), 1, stats=None) == EINVAL and fwd(members(), 1, out=None) == EINVAL
    for tau in (0.0, -0.1, float('inf'), float('nan')):
        assert fwd(members(), 1, tau=tau) == EINVAL, tau


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    from txt2vid_amd import functional as TF
    W, f, s, st = torch.zeros(8, 3), torch.zeros(2, 8), torch.zeros(2, 3), torch.zeros(4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        TF.match_group(W, [f], [s], 0.1, st)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        TF.match_embedded([s], [s], 0.1, st)
    with pytest.raises(ValueError):
        TF.match_group(W, [], [], 0.1, st)
    with pytest.raises(ValueError):
        TF.match_group(W, [f] * 9, [s] * 9, 0.1, st)
    with pytest.raises(ValueError):
        TF.match_group(W, [f], [s, s], 0.1, st)
    with pytest.raises(ValueError):
        TF.match_embedded([s], [s], 0.0, st)
