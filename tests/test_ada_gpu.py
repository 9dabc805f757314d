"""GPU: the adaptive strength of the discriminator's augmentation (--D_aug_p / --D_ada) on the HIP path, against the
CPU restatement composed with the oracle (tests/ada_cases.py) —
  (1) the gated kernels equal the ungated ones clip by clip, bit for bit; p is read when the launch runs; the controller's
      state follows the numpy float32 restatement bit for bit; the refusals;
  (2) three training iterations against the oracle loop, graph replay against eager;
  (3) off means off, and the launch budget with the controller on;
  (4) the command line: checkpoints carry the controller, the flags compose with the other opt-ins."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ada_cases as AC
import diffaug_cases as DA
import schedule_cases as S
import test_diffaug_gpu as TD              # (its set-up helpers: make, batches, seed, tokens_for, _counted)
from txt2vid_amd import functional_aug as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = S.B
F32 = np.float32
NEW = ('t2v_diffaug_gated_fwd', 't2v_diffaug_gated_bwd', 't2v_ada_update')
OLD = ('t2v_diffaug_fwd', 't2v_diffaug_bwd')
P = 0.5

# name -> (shape, row stride, effective policy per clip). The gates are built from the policies: bit k of clip j is on iff
# gate[row j, k] < p.  one_wg: one workgroup per clip; rgb: C = 3 saturation; strided: row_stride 2 on an 8-row block; split:
# 65 536 elements per clip, split over several workgroups (one clip with and one without live colour).
MEMBERS = {
    'one_wg': ((8, 1, 4, 16, 16), 1, [0, 1, 2, 3, 4, 5, 6, 7]),
    'rgb': ((8, 3, 2, 8, 8), 1, [0, 1, 2, 3, 4, 5, 6, 7]),
    'strided': ((4, 1, 4, 16, 16), 2, [0, 2, 4, 6]),
    'split': ((2, 1, 16, 64, 64), 4, [3, 6]),
}
ORDER = ['one_wg', 'rgb', 'strided', 'split']


def _gate_block(rows, policies, stride):
    """[rows, K] gates realising `policies` at rows j * stride for p = P: 0.25 (< p) where the bit is on, 0.75 where it is off;
    clip 0's colour gate is EXACTLY p where its colour bit is off (equal means not applied). Unread rows and columns 3-7: 0."""
    g = torch.zeros(rows, A.K)
    for j, bits in enumerate(policies):
        for k in range(3):
            g[j * stride, k] = 0.25 if (bits >> k) & 1 else 0.75
    if not policies[0] & 1:
        g[0, 0] = P
    return g


def _member(name, s=0):
    shape, stride, policies = MEMBERS[name]
    gen = torch.Generator()
    gen.manual_seed(4321 + s + sum(shape))
    x = torch.rand(*shape, generator=gen) * 2 - 1
    gy = torch.randn(*shape, generator=gen)
    u = torch.rand(8, A.K, generator=gen)
    return x, gy, u, _gate_block(8, policies, stride), stride, policies


def _run(xs, gys, us, strides, policy, gates=None, p=None):
    """Forward + backward through the kernels (every member requires a gradient). Returns (ys, gxs) on the host."""
    xd = [x.to(DEV).requires_grad_(True) for x in xs]
    ud = [u.to(DEV) for u in us]
    if gates is None:
        ys = A.diffaug(xd, ud, strides, policy)
    else:
        ys = A.diffaug(xd, ud, strides, policy, [None if g is None else g.to(DEV) for g in gates], p)
    gxs = torch.autograd.grad(ys, xd, [g.to(DEV) for g in gys])
    return [y.detach().cpu() for y in ys], [g.cpu() for g in gxs]


@pytest.fixture(scope='module')
def ungated():
    """The ungated entry points over the four members, once per policy 1..7: policy -> (ys, gxs). Shared and left unchanged."""
    ms = [_member(n) for n in ORDER]
    out = {}
    for policy in range(1, 8):
        out[policy] = _run([m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms], [m[4] for m in ms], policy)
    return ms, out


def _expect(ms, ungated_runs, i, want_y, want_g):
    """Clip by clip: the ungated output at the clip's effective policy; the input itself for policy 0."""
    x, gy, _, _, _, policies = ms[i]
    for j, bits in enumerate(policies):
        ry = x[j] if bits == 0 else ungated_runs[bits][0][i][j]
        rg = gy[j] if bits == 0 else ungated_runs[bits][1][i][j]
        assert torch.equal(want_y[j], ry), (ORDER[i], j, bits, 'forward')
        assert torch.equal(want_g[j], rg), (ORDER[i], j, bits, 'backward')


# ------------------------------------------------------------------------------------------------ 1. op level
def test_gating_is_exact(ungated):
    ms, runs = ungated
    xs, gys, us, gs, strides = ([m[k] for m in ms] for k in range(5))
    assert sorted(set(ms[0][5])) == list(range(8)) and float(ms[0][3][0, 0]) == P        # all 8 subsets; one gate equal to p
    assert xs[3][0].numel() == 65536
    p = torch.tensor([P], device=DEV)
    ys, gxs = _run(xs, gys, us, strides, DA.FULL, gs, p)
    for i in range(4):
        _expect(ms, runs, i, ys[i], gxs[i])
    # p = 1: the ungated launch, bit for bit; p = 0: the input (forward) and the incoming gradient (adjoint)
    ys, gxs = _run(xs, gys, us, strides, DA.FULL, gs, torch.ones(1, device=DEV))
    for i in range(4):
        assert torch.equal(ys[i], runs[7][0][i]) and torch.equal(gxs[i], runs[7][1][i]), ORDER[i]
    ys, gxs = _run(xs, gys, us, strides, DA.FULL, gs, torch.zeros(1, device=DEV))
    for i in range(4):
        assert torch.equal(ys[i], xs[i]) and torch.equal(gxs[i], gys[i]), ORDER[i]
    # a sub-policy is masked by the gates like the full one
    ys, gxs = _run(xs[:1], gys[:1], us[:1], strides[:1], 'color,cutout', gs[:1], p)
    for j, bits in enumerate(ms[0][5]):
        e = bits & 5
        assert torch.equal(ys[0][j], xs[0][j] if e == 0 else runs[e][0][0][j])
        assert torch.equal(gxs[0][j], gys[0][j] if e == 0 else runs[e][1][0][j])


def test_mixed_launch_with_ungated_members(ungated):
    """8 members in one launch, two of them with gates[i] == NULL: those get the full policy, the others their gates."""
    ms, runs = ungated
    idx = [0, 1, 2, 3, 0, 1, 2, 3]
    gated = [True, False, True, True, False, True, True, True]
    calls, _, (ys, gxs) = TD._counted(lambda: _run([ms[i][0] for i in idx], [ms[i][1] for i in idx], [ms[i][2] for i in idx],
                                                   [ms[i][4] for i in idx], DA.FULL,
                                                   [ms[i][3] if on else None for i, on in zip(idx, gated)],
                                                   torch.tensor([P], device=DEV)), NEW + OLD)
    assert calls == {'t2v_diffaug_gated_fwd': 1, 't2v_diffaug_gated_bwd': 1, 't2v_ada_update': 0, 't2v_diffaug_fwd': 0,
                     't2v_diffaug_bwd': 0}
    for k, (i, on) in enumerate(zip(idx, gated)):
        if on:
            _expect(ms, runs, i, ys[k], gxs[k])
        else:
            assert torch.equal(ys[k], runs[7][0][i]) and torch.equal(gxs[k], runs[7][1][i]), k


def test_p_is_read_at_run_time(ungated):
    """One gated forward captured in a graph; replayed with p = 0 and, after p is overwritten ON THE DEVICE, with p = 1: the
    copy, then the full transformation. No re-capture."""
    ms, runs = ungated
    x, _, u, g, stride, _ = ms[0]
    xd, ud, gd = x.to(DEV), u.to(DEV), g.to(DEV)
    p = torch.zeros(1, device=DEV)
    one = torch.ones(1, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.diffaug([xd], [ud], [stride], DA.FULL, [gd], p)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, = A.diffaug([xd], [ud], [stride], DA.FULL, [gd], p)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), x)
    p.copy_(one)                                                    # device to device
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), runs[7][0][0])
    p.copy_(torch.tensor([P], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = y.cpu()
    for j, bits in enumerate(ms[0][5]):
        assert torch.equal(got[j], x[j] if bits == 0 else runs[bits][0][0][j]), j


# pattern -> (pairs with u_r > u_f, pairs with u_r < u_f, ties) as fractions of a step's pairs (4 or 8)
PATTERNS = {'up': (1.0, 0.0, 0.0), 'down': (0.0, 1.0, 0.0), 'half': (0.75, 0.25, 0.0), 'tiehalf': (0.5, 0.0, 0.5), 'ties': (0.0, 0.0, 1.0)}
# interval 1, p0 0.5, step 0.25, target 0.5: up to the clamp at 1, a window with r_t == target, down to the clamp at 0, a window of
# ties and wins with r_t == target, up, and a window of ties alone (r_t = 0 < target)
SEQ_1 = ['up', 'up', 'up', 'half', 'down', 'down', 'down', 'down', 'down', 'tiehalf', 'up', 'ties']
# interval 4, p0 0.5, step 1.5 (not dyadic after rounding kclips): 2.0 -> clamp 1; r_t == target (with ties); -0.5 -> clamp 0
SEQ_4 = ['up'] * 4 + ['up', 'ties', 'up', 'ties'] + ['down'] * 4


def _logits(pattern, counts, gen):
    """Synthetic paired logits of one D step: per level (u_r, u_f), the pattern's wins / losses / ties spread over the pairs."""
    total = sum(counts)
    up, down, tie = (int(round(f * total)) for f in PATTERNS[pattern])
    assert up + down + tie == total
    kinds = [1] * up + [-1] * down + [0] * tie
    order = torch.randperm(total, generator=gen).tolist()
    kinds = [kinds[k] for k in order]
    base = torch.randn(total, generator=gen)
    gap = torch.rand(total, generator=gen) + 0.5
    real = base + torch.tensor(kinds, dtype=torch.float32) * gap
    assert all((real[k] == base[k]) == (kinds[k] == 0) for k in range(total))
    rs, fs, o = [], [], 0
    for c in counts:
        rs.append(real[o:o + c].clone().view(c, 1))
        fs.append(base[o:o + c].clone().view(c, 1))
        o += c
    return rs, fs


@pytest.mark.parametrize('counts', [(4,), (4, 2, 1, 1)])
@pytest.mark.parametrize('interval,seq,kclips', [(1, SEQ_1, 0.016), (4, SEQ_4, 16.0 / 1500.0)])
def test_controller_follows_the_restatement_bitwise(counts, interval, seq, kclips):
    from txt2vid_amd.gan.ada import AdaState
    target = 0.5
    gen = torch.Generator()
    gen.manual_seed(31 + interval + len(counts))
    state = AdaState(target, interval=interval, kclips=kclips, p0=0.5, device=DEV)
    ref = AC.controller_init(0.5)
    step = AC.step_size(counts[0], interval, kclips)
    assert len(seq) == 12 and (step == F32(0.25) if interval == 1 else abs(float(step) - 1.5) < 1e-6)
    ps, rts = [], []
    for pattern in seq:
        rs, fs = _logits(pattern, counts, gen)
        s, n = AC.sign_sum([r.numpy() for r in rs], [f.numpy() for f in fs])
        assert n == sum(counts) and s == int(round((PATTERNS[pattern][0] - PATTERNS[pattern][1]) * n))
        if ref[3] + 1 >= interval:
            rts.append((float(ref[1]) + s) / (float(ref[2]) + n))
        AC.controller_step(ref, s, n, target, step, interval)
        state.observe([r.to(DEV) for r in rs], [f.to(DEV) for f in fs])
        got = state.ada.cpu().numpy()
        assert got.dtype == F32 and got.tobytes() == ref.tobytes(), (pattern, got, ref)
        ps.append(float(ref[0]))
    print('interval %d, %d levels: p %s, r_t %s' % (interval, len(counts), ps, rts))
    assert 1.0 in ps and 0.0 in ps and target in rts                # both clamps and a window with r_t == target were reached
    if interval == 1:
        assert ps == [0.75, 1.0, 1.0, 1.0, 0.75, 0.5, 0.25, 0.0, 0.0, 0.0, 0.25, 0.0]
    else:
        assert ps == [0.5] * 3 + [1.0] * 8 + [0.0]


def test_new_entry_points_refuse_bad_arguments():
    import ctypes
    from txt2vid_amd import functional as TF
    from txt2vid_amd._lib import AugMember, AdaLevel, MAX_GROUPS
    from txt2vid_amd.gan.ada import AdaState
    l, st = TF.lib(), TF._stream()
    x = torch.ones(2, 1, 2, 8, 8, device=DEV)
    y = torch.full_like(x, 7.0)
    u = torch.rand(2, A.K, device=DEV)
    g = torch.rand(2, A.K, device=DEV)
    p = torch.ones(1, device=DEV)

    def member(**kw):
        m = dict(x=x.data_ptr(), y=y.data_ptr(), u=u.data_ptr(), N=2, C=1, T=2, S=8, row_stride=1, rows=2, policy=7)
        m.update(kw)
        return m

    def call(fn, ms, n=None, gates=True, pp=True):
        arr = (AugMember * max(1, len(ms)))()
        for a, m in zip(arr, ms):
            for k, v in m.items():
                setattr(a, k, v)
        gp = (ctypes.c_void_p * max(1, len(ms)))(*([g.data_ptr()] * max(1, len(ms)))) if gates else None
        return fn(arr, gp, len(ms) if n is None else n, p.data_ptr() if pp else None, st)
    for fn in (l.t2v_diffaug_gated_fwd, l.t2v_diffaug_gated_bwd):
        assert fn(None, None, 1, p.data_ptr(), st) < 0
        assert call(fn, [member()], gates=False) < 0                             # gates == NULL
        assert call(fn, [member()], pp=False) < 0                                # p == NULL
        assert call(fn, [member()], n=0) < 0
        assert call(fn, [member()] * (MAX_GROUPS + 1)) < 0
        for bad in (dict(policy=8), dict(policy=0), dict(policy=-1), dict(x=None), dict(y=None), dict(u=None), dict(y=x.data_ptr()),
                    dict(N=0), dict(C=0), dict(T=0), dict(S=0), dict(row_stride=0), dict(rows=1), dict(row_stride=2)):
            assert call(fn, [member(), member(**bad)]) < 0, bad
    ada = torch.full((8,), 7.0, device=DEV)
    lo = torch.zeros(4, device=DEV)

    def upd(n=1, count=4, real=True, fake=True, ada_ptr=True, levels=True, step=0.25, interval=1):
        arr = (AdaLevel * max(1, n))()
        for a in arr:
            a.real, a.fake, a.count = (lo.data_ptr() if real else None), (lo.data_ptr() if fake else None), count
        return l.t2v_ada_update(ada.data_ptr() if ada_ptr else None, arr if levels else None, n, 0.6, step, interval, st)
    for bad in (dict(n=0), dict(n=MAX_GROUPS + 1), dict(count=0), dict(count=-1), dict(real=False), dict(fake=False), dict(ada_ptr=False),
                dict(levels=False), dict(interval=0), dict(step=-0.25), dict(step=float('inf')), dict(step=float('nan'))):
        assert upd(**bad) < 0, bad
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((ada == 7).all())                       # nothing was launched
    assert call(l.t2v_diffaug_gated_fwd, [member()]) == 0 and upd() == 0
    torch.cuda.synchronize()
    # (the fill value read as a state: window 7 / 11 > 0.6 after the step, so p = 7.25 is clamped to 1 and the window cleared)
    assert not bool((y == 7).any()) and ada.tolist() == [1.0, 0.0, 0.0, 0.0, 7.0, 7.0, 7.0, 7.0]
    # the host layer: CPU tensors raise, gates and p come together, shapes are checked
    with pytest.raises(RuntimeError):
        A.diffaug([x.cpu()], [u], [1], 7, [g], p)
    with pytest.raises(RuntimeError):
        A.diffaug([x], [u], [1], 7, [g.cpu()], p)
    with pytest.raises(RuntimeError):
        A.diffaug([x], [u], [1], 7, [g], p.cpu())
    with pytest.raises(ValueError):
        A.diffaug([x], [u], [1], 7, [g], None)
    with pytest.raises(ValueError):
        A.diffaug([x], [u], [1], 7, [g[:1]], p)
    with pytest.raises(ValueError):
        A.diffaug([x, x], [u, u], [1, 1], 7, [g], p)
    with pytest.raises(RuntimeError):
        AdaState(0.6, device=DEV).observe([lo.cpu()], [lo.cpu()])
    with pytest.raises(ValueError):
        AdaState(0.6, device=DEV).observe([lo], [lo[:2]])


# ------------------------------------------------------------------------------------------------ helpers for the runs
def make(cond=False, N=1, M=1, p0=0.5, target=0.6, interval=1, kclips=0.016, ada=True, p_fixed=None):
    """test_diffaug_gpu.make (B = 4, 64x64x1, recipe weights, RSGAN + GP 0.5, full policy) with a controller on `gan.ada`
    (ada=True) and / or a fixed --D_aug_p."""
    from txt2vid_amd.gan.ada import AdaState
    gan, optD, optG, losses, prm = TD.make(cond, N, M)
    if ada:
        gan.ada = AdaState(target, interval=interval, kclips=kclips, p0=p0, device=DEV)
        prm.D_aug_p, prm.D_ada, prm.D_ada_interval, prm.D_ada_kclips = p0, target, interval, kclips
    elif p_fixed is not None:
        prm.D_aug_p = p_fixed
    return gan, optD, optG, losses, prm


def _record(gan):
    """Wrap gan.ada.observe: the state's first four entries after every D step (eager runs: one read per call)."""
    traj, orig = [], gan.ada.observe

    def observe(u_r, u_f):
        orig(u_r, u_f)
        traj.append(gan.ada.ada[:4].cpu().numpy().copy())
    gan.ada.observe = observe
    return traj


# The seed of test_iterations_vs_oracle_loop, chosen on the CPU so that the oracle loop satisfies the test's precondition in all
# four cases (its smallest |u_r - u_f| / max(1, max |logit|) there: 3.1e-3, 6.1e-3, 5.6e-3, 3.9e-3).
SEED = 145
# How far the HIP path's logits may be from the oracle's at this size, relative to max(1, max |logit|); from the oracle alone and
# the number format. The oracle's own float32 error on D's logits here — its float32 forward against its float64 forward on the
# same weights and augmented clips, measured on the CPU — is 2e-7 at a logit scale of 0.9, three units in the last place. The HIP
# path sums in another order, so each side may be that far from the exact value: 4e-7 while the weights are identical, which
# they are in the first iteration only. A factor 25 on top is for the later iterations, whose weights come out of optimiser
# steps on gradients that differ in their last bits.
LOGIT_AGREEMENT = 1e-5


# ------------------------------------------------------------------------------------------------ 2. iteration level
@pytest.mark.parametrize('cond', [False, True])
@pytest.mark.parametrize('N,M', [(1, 1), (2, 1)])
def test_iterations_vs_oracle_loop(cond, N, M):
    """Three iterations with the full policy, p0 = 0.5, interval 1 and step 0.25 against the oracle loop with the restatement at the
    same call sites and draw positions: lossD and lossG at the bounds of test_diffaug_gpu's loop test (1e-3, then 2e-2 in the third
    iteration), and the trajectory of the controller's state EQUAL after every D step.

    Precondition, asserted on the oracle side alone: in every D step every |u_r - u_f| exceeds 100 x LOGIT_AGREEMENT x
    max(1, max |logit|) — so no sign can differ between the two sides short of a real defect — and no window has
    r_t == target. The seed is chosen on the CPU so that the oracle satisfies it."""
    from txt2vid_amd.gan.trainer import TrainStep
    seed = SEED
    tokens = TD.tokens_for(B) if cond else None
    kclips = 0.016
    assert AC.step_size(B, 1, kclips) == F32(0.25)
    ref = AC.oracle_loop(cond, N, M, DA.FULL, tokens=tokens, iters=3, seed=seed, p0=0.5, target=0.6, interval=1, kclips=kclips)
    for k, (margin, scale) in enumerate(ref['steps']):
        print('oracle D step %d: min |u_r - u_f| %.4g, max |logit| %.4g, r_t %r, p -> %g' % (k, margin, scale, ref['rt'][k], ref['p'][k]))
        assert margin > 100 * LOGIT_AGREEMENT * max(1.0, scale), (k, margin, scale)
        assert ref['rt'][k] is not None and ref['rt'][k] != 0.6
    gan, optD, optG, losses, prm = make(cond, N, M, p0=0.5, target=0.6, interval=1, kclips=kclips)
    traj = _record(gan)
    TD.seed(seed)
    for it in range(3):
        x = S.batch().to(DEV)
        c = None
        if cond:
            with torch.no_grad():
                c = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        assert ts.aug == 7 and ts.gated
        lD, lG, _, _ = ts.run(x, c)
        lD, lG = float(lD), float(lG)
        tol = 1e-3 if it < 2 else 2e-2
        print('D_ada %s %d:%d it %d: lossD %.6f (%.6f) lossG %.6f (%.6f) p %s (%s)' % (
            'cond' if cond else 'uncond', N, M, it, lD, ref['lossD'][it], lG, ref['lossG'][it],
            [float(t[0]) for t in traj[it * N:(it + 1) * N]], ref['p'][it * N:(it + 1) * N]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))
    assert len(traj) == 3 * N == len(ref['ada'])
    for k, (a, b) in enumerate(zip(traj, ref['ada'])):
        assert a.tobytes() == b.tobytes(), (k, a, b)


def test_graph_replay_matches_eager():
    """GraphedTrainStep with the controller (gate blocks among the device-resident draws, the update launch inside the one
    captured graph) reproduces the eager iterations: 2 eager, then capture + replays; p moves between replays without a
    re-capture. Loss tolerances of test_diffaug_gpu.test_graph_replay_matches_eager."""
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    kw = dict(N=1, M=2, p0=0.5, target=0.6, interval=1, kclips=0.032)             # step 0.125: four moves stay inside [0, 1]
    assert AC.step_size(B, 1, 0.032) == F32(0.125)
    gan, optD, optG, losses, prm = make(**kw)
    TD.seed(6)
    eager = []
    for x in TD.batches():
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, None)
        eager.append((float(lD), float(lG), float(gan.ada.p)))
    gan, optD, optG, losses, prm = make(**kw)
    TD.seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2)
    assert gs.draws.gated and gs.draws.n_aug == 2 * (2 * 1 + 2 + 1)
    ps = []
    for i, x in enumerate(TD.batches()):
        lD, lG = gs.step(x)
        got = (float(lD), float(lG))
        ps.append(float(gan.ada.p))
        print('D_ada step %d (%s): %s p %g vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, ps[-1], eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i][:2])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1
    assert ps == [e[2] for e in eager]
    assert ps[2] != ps[3]                                                         # p differs between the two replays
    assert all(abs(abs(a - b) - 0.125) < 1e-7 for a, b in zip([0.5] + ps[:-1], ps))


# ------------------------------------------------------------------------------------------------ 3. off means off
def _eager_with_rng(parts):
    out = TD._one_eager_iteration(parts)
    return out, torch.get_rng_state().clone(), np.random.get_state()[1].copy()


def test_off_means_off():
    """With no new flag, and with --D_aug_p 1.0 alone, no new entry point is called, eagerly or while capturing; the losses, the
    host RNG sequence and the number of augmentation blocks are those of --D_aug alone."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    TD._one_eager_iteration(make(ada=False))                                      # burn-in
    calls, _, (plain, rng, nprng) = TD._counted(lambda: _eager_with_rng(make(ada=False)), NEW)
    assert calls == dict.fromkeys(NEW, 0)
    calls, _, (one, rng1, nprng1) = TD._counted(lambda: _eager_with_rng(make(ada=False, p_fixed=1.0)), NEW)
    assert calls == dict.fromkeys(NEW, 0)
    assert one == plain and torch.equal(rng, rng1) and np.array_equal(nprng, nprng1)
    for parts in (make(ada=False), make(ada=False, p_fixed=1.0)):
        calls, _, _ = TD._counted(lambda: TD._three_graphed_iterations(parts), NEW)
        assert calls == dict.fromkeys(NEW, 0)
        gs = GraphedTrainStep(*parts, DEV, (B, 1, 16, 64, 64), warmup=2)
        assert gs.draws.n_aug == 2 * 1 + 1 + 1 and not gs.draws.gated and not gs.ts.gated
    # on: a fixed p < 1 takes the gated launches (and no controller launch), and changes the iteration
    calls, _, (half, rng2, _) = TD._counted(lambda: _eager_with_rng(make(ada=False, p_fixed=0.5)), NEW + OLD)
    assert calls == {'t2v_diffaug_gated_fwd': 2, 't2v_diffaug_gated_bwd': 1, 't2v_ada_update': 0, 't2v_diffaug_fwd': 0,
                     't2v_diffaug_bwd': 0}
    assert half != plain and all(np.isfinite(half)) and not torch.equal(rng, rng2)


@pytest.mark.parametrize('N,M', [(1, 1), (2, 2)])
def test_launch_budget(N, M):
    """--D_ada adds exactly N launches per iteration, one t2v_ada_update per D step; gating adds none over --D_aug: the gated
    entry points are called as often as test_diffaug_gpu.test_launch_budget counts the ungated ones, which are not called at
    all. Counted per Python pass: one eager iteration, and the 2 eager + 1 captured pass of a graphed run."""
    calls, _, _ = TD._counted(lambda: TD._one_eager_iteration(make(N=N, M=M)), NEW + OLD)
    assert calls == {'t2v_diffaug_gated_fwd': N + M, 't2v_diffaug_gated_bwd': M, 't2v_ada_update': N, 't2v_diffaug_fwd': 0,
                     't2v_diffaug_bwd': 0}
    calls, _, _ = TD._counted(lambda: TD._three_graphed_iterations(make(N=N, M=M)), NEW + OLD)
    assert calls == {'t2v_diffaug_gated_fwd': 3 * (N + M), 't2v_diffaug_gated_bwd': 3 * M, 't2v_ada_update': 3 * N,
                     't2v_diffaug_fwd': 0, 't2v_diffaug_bwd': 0}
    # the same iteration with --D_aug alone: the old entry points, the same counts, no update
    calls, _, _ = TD._counted(lambda: TD._one_eager_iteration(make(N=N, M=M, ada=False)), NEW + OLD)
    assert calls == {'t2v_diffaug_gated_fwd': 0, 't2v_diffaug_gated_bwd': 0, 't2v_ada_update': 0, 't2v_diffaug_fwd': N + M,
                     't2v_diffaug_bwd': M}


# ------------------------------------------------------------------------------------------------ 4. command line
BASE = ['--data', os.path.join(ROOT, 'tools', 'cfg', 'synth.json'), '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16',
        '32', '64', '--D_names', 'video', '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999',
        '--G_beta1', '0.5', '--G_beta2', '.999', '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier',
        '--seed', '100', '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1',
        '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
        '--dont_use_sent', '--batch_size', '8', '--epochs', '1', '--save_example_period', '0']
FLAGS = ['--D_aug', DA.FULL, '--D_ada', '0.6', '--D_ada_interval', '1']
STATE = re.compile(r'Augmentation probability p = ([-0-9.e]+); window: sign sum ([-0-9.e+]+) over ([-0-9.e+]+) pairs in ([-0-9.e+]+) D steps')


def _cli(args, env=None, ok=True):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + BASE + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600, env=e)
    out = p.stdout.decode(errors='replace')
    assert (p.returncode == 0) == ok, out[-3000:]
    return out


def _out(tmp_path, name):
    return ['--out', str(tmp_path / name), '--out_samples', str(tmp_path / (name + '_s'))]


def test_cli_checkpoint_carries_the_controller(tmp_path):
    # p0 = 0.5 and 0.5 kclips (step 0.016 per update at B = 8): two iterations move p whichever way the statistic points
    flags = FLAGS + ['--D_aug_p', '0.5', '--D_ada_kclips', '0.5']
    log = _cli(_out(tmp_path, 'a') + flags + ['--max_iters', '2', '--save_model_period', '2'])
    assert 'Iter 2, Loss_D' in log
    assert float(STATE.search(log).group(1)) == 0.5
    m = re.search(r'Iter 2, augmentation probability p \(--D_ada, target 0.6\): ([0-9.]+)', log)
    assert m, log[-2000:]
    ck, = glob.glob(os.path.join(str(tmp_path / 'a'), 'iter_2_lossG_*'))
    saved = torch.load(ck, map_location='cpu', weights_only=False)['ada']['ada']
    assert saved.dtype == torch.float32 and saved.shape == (8,) and saved[1:].tolist() == [0.0] * 7
    assert abs(float(saved[0]) - 0.5) <= 2 * 0.016 + 1e-6                          # at most two moves of 0.016
    # resume with the flags: p and the window are the saved ones (p0 would be 0.25)
    log = _cli(_out(tmp_path, 'b') + flags[:-4] + ['--D_aug_p', '0.25', '--D_ada_kclips', '0.5', '--weights', ck, '--max_iters', '1',
                                                   '--save_model_period', '1000'])
    got = [float(v) for v in STATE.search(log).groups()]
    assert [F32(v) for v in got] == [F32(v) for v in saved[:4].tolist()], (got, saved)
    assert 'Iter 1, Loss_D' in log
    # the file loads into a run without the flags: the key is ignored
    log = _cli(_out(tmp_path, 'c') + ['--weights', ck, '--max_iters', '1', '--save_model_period', '1'])
    assert 'Iter 1, Loss_D' in log and not STATE.search(log) and 'augmentation probability' not in log
    ck_c, = glob.glob(os.path.join(str(tmp_path / 'c'), 'iter_1_lossG_*'))
    assert 'ada' not in torch.load(ck_c, map_location='cpu', weights_only=False)
    # a checkpoint written by the reference (no key) loads with the flags: p = p0
    log = _cli(_out(tmp_path, 'd') + FLAGS + ['--D_aug_p', '0.375', '--weights', os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint_uncond.pt'),
                                              '--max_iters', '1', '--save_model_period', '1000'])
    assert [float(v) for v in STATE.search(log).groups()] == [0.375, 0.0, 0.0, 0.0] and 'Iter 1, Loss_D' in log


@pytest.mark.parametrize('name,extra,env', [('bf16', [], {'T2V_CONV_PRECISION': 'bf16'}), ('D_sn', ['--D_sn'], {}),
                                            ('G_ema', ['--G_ema', '0.999'], {}), ('end2end', ['--end2end'], {})])
def test_cli_flags_compose(tmp_path, name, extra, env):
    """Two iterations (the losses and p are read one iteration late under graph replay) with bf16-compute convolutions
    (T2V_CONV_PRECISION=bf16), --D_sn, --G_ema and --end2end (eager launches) next to the flags."""
    log = _cli(_out(tmp_path, name) + FLAGS + extra + ['--max_iters', '2', '--save_model_period', '1000'], env=env)
    m = re.search(r'Iter 2, Loss_D: ([-0-9.naninf]+) Loss_G: ([-0-9.naninf]+)', log)
    assert m and all(np.isfinite(float(v)) for v in m.groups()), log[-1500:]
    assert re.search(r'Iter 2, augmentation probability p \(--D_ada, target 0.6\): 0.0000', log)      # p0 = 0 stays, or rises by 1.6e-5 a step


def test_cli_refusals(tmp_path):
    """A data-parallel start with --D_ada raises before a process group forms; either flag needs a policy."""
    log = _cli(_out(tmp_path, 'dp') + FLAGS + ['--max_iters', '1'], env={'WORLD_SIZE': '2', 'RANK': '0'}, ok=False)
    assert 'data-parallel' in log
    log = _cli(_out(tmp_path, 'np') + ['--D_ada', '0.6', '--max_iters', '1'], ok=False)
    assert '--D_aug' in log
    log = _cli(_out(tmp_path, 'np2') + ['--D_aug_p', '0.5', '--max_iters', '1'], ok=False)
    assert '--D_aug' in log
