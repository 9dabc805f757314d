"""GPU: the --discrim_steps N / --gen_steps M schedule (trainer.py:228-263) on the HIP hot path —
  (a) the eager loop against the REAL reference's fixture (tests/golden/steps_schedule.npz, make_golden_steps.py),
  (b) graph replay against the eager loop, the BatchNorm counters, the Adam step counters and a checkpoint round trip,
  (c) the data-parallel multi-graph capture (two ranks over gloo on one GPU), --end2end against the oracle, the command line."""
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import schedule_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pour(module):
    sd = module.state_dict()
    module.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in sd.items()})
    return module.to(DEV)


def make(case):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss, WassersteinGanLoss
    from txt2vid_amd.optim import Adam
    txt = None
    if case['cond']:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
        from txt2vid_amd.models.txt.basic import Seq2Seq
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256))
        dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256))
        txt = Seq2Seq(vocab_size=S.V)
        txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                             for k, v in txt.state_dict().items()})
        txt.to(DEV)
    else:
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1))
        dis = pour(MultiScaleDiscrim(num_channels=1))
    gen.train()
    dis.train()
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    lc = RSGANLoss if case['loss'] == 'rsgan' else WassersteinGanLoss
    losses = MixedGanLoss(g_loss=lc(), d_loss=lc())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    return gan, optD, optG, losses, S.params_for(case)


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def code(gan, tokens):
    if tokens is None:
        return None
    with torch.no_grad():
        return gan.cond_encoder.encode(tokens, [8] * S.B)[2].detach()


def adam_steps(opt):
    sd = opt.state_dict()
    return {int(st['step']) for st in sd['state'].values()}


def nbt(gen):
    return {int(v) for k, v in gen.state_dict().items() if k.endswith('num_batches_tracked')}


def norms_close(module, want, rtol):
    """Per-parameter gradient norms compared as one vector (relative L2 distance), not key by key: the biases in front of
    training-mode BatchNorms carry rounding noise on both sides."""
    got = {k: (float(p.grad.norm()) if p.grad is not None else 0.0) for k, p in module.named_parameters()}
    a = np.array([got[k] for k in want])
    b = np.array([max(v, 0.0) for v in want.values()])
    rel = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print('gradient norms: relative L2 distance %.3e' % rel)
    assert rel < rtol, rel


@pytest.mark.parametrize('tag', sorted(S.CASES))
def test_eager_schedule_vs_reference_fixture(golden, tag):
    """Three free-running N:M iterations against the losses the REAL reference logged (the per-iteration totals), bounds of the
    existing 3-iteration step tests (1e-3 / 1e-3 / 2e-2: the GAN dynamics are chaotic); then the last iteration's gradient
    norms, the parameter deltas, the Adam step counts (3N, 3M) and the generator's BatchNorm counters (3M)."""
    from txt2vid_amd.gan.trainer import TrainStep
    g = golden('steps_schedule')
    case = S.CASES[tag]
    N, M = case['N'], case['M']
    gan, optD, optG, losses, prm = make(case)
    init = {m: {k: p.detach().clone() for k, p in mod.named_parameters()} for m, mod in (('G', gan.gen), ('D', gan.discrims[0]))}
    tokens = torch.from_numpy(g[tag + '_tokens']).to(DEV) if case['cond'] else None
    seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        cond = code(gan, tokens)
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        for k in range(ts.n_parts):
            ts.part(k, x, cond)
            # the last D backward and the last G backward of iterations 0 and 2 (in iteration 2 the losses already part by up to
            # 2e-2 and, with two G steps per iteration, G's gradient norms by ~15 %: a loose sanity bound there)
            if it in (0, 2) and k == N - 1:
                norms_close(gan.discrims[0], S.fixture_norms(g, tag + ('_D_gn' if it else '_D_gn0')), rtol=1e-1 if it else 1e-2)
            if it in (0, 2) and k == N + M - 1:
                norms_close(gan.gen, S.fixture_norms(g, tag + ('_G_gn' if it else '_G_gn0')), rtol=3e-1 if it else 1e-2)
        lD, lG = float(ts.lD), float(ts.lG)
        tol = 1e-3 if it < 2 else 2e-2
        if tag == 'b' and it == 1:
            # the Wasserstein critic is unbounded (|lossG| ~ 8 here) and takes three Adam steps per iteration at GP weight 10: the
            # fp32 rounding differences of iteration 0 reach 1.5e-3 of the loss one iteration later
            tol = 3e-3
        print('%s it %d: lossD %.7f (ref %.7f)  lossG %.7f (ref %.7f)' % (tag, it, lD, g[tag + '_lossD'][it], lG, g[tag + '_lossG'][it]))
        assert abs(lD - g[tag + '_lossD'][it]) < tol * max(1.0, abs(g[tag + '_lossD'][it])), (it, lD)
        assert abs(lG - g[tag + '_lossG'][it]) < tol * max(1.0, abs(g[tag + '_lossG'][it])), (it, lG)
    assert adam_steps(optD) == {int(g[tag + '_steps'][0])} == {3 * N}
    assert adam_steps(optG) == {int(g[tag + '_steps'][1])} == {3 * M}
    assert nbt(gan.gen) == set(int(v) for v in g[tag + '_nbt']) == {3 * M}
    # parameters after iteration 2: early Adam updates are ~ lr * sign(g) per element, so the norms of the per-parameter deltas
    # are robust (compared as one vector, like the gradient norms)
    for m, mod in (('G', gan.gen), ('D', gan.discrims[0])):
        want = S.fixture_norms(g, tag + '_%s_dp' % m)
        got = {k: float((p.detach() - init[m][k]).norm()) for k, p in mod.named_parameters()}
        a, b = np.array([got[k] for k in want]), np.array(list(want.values()))
        rel = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print('%s parameter deltas: relative L2 distance %.3e' % (m, rel))
        assert rel < 5e-2, (m, rel)


@pytest.mark.parametrize('tag', ['a', 'c'], ids=['uncond_2to2', 'cond_2to1'])
def test_graph_replay_matches_eager_schedule(golden, tag, tmp_path):
    """GraphedTrainStep (2 eager iterations, capture, replays: the N + M + 1 parts as ONE graph) reproduces the eager N:M loop,
    tolerances of test_graph_replay_matches_eager_nolstm (the second replay of the 2:2 schedule, four Adam steps of G later, at
    the chaotic-iteration bound 2e-2 of the fixture tests: the replay's device-side Adam step counter rounds the bias corrections
    differently from the eager host count); the BatchNorm counters advance by M and the device-side Adam counters
    by N and M per iteration, and a checkpoint written after the replays carries (and reloads) 4N and 4M."""
    from txt2vid_amd.gan.trainer import train_iteration, GraphedTrainStep
    from txt2vid_amd.optim import Adam
    case = S.CASES[tag]
    N, M = case['N'], case['M']
    tokens = torch.from_numpy(golden('steps_schedule')[tag + '_tokens']).to(DEV) if case['cond'] else None

    def batches():
        gen = torch.Generator()
        gen.manual_seed(11)
        return [(torch.rand(4, 1, 16, 64, 64, generator=gen) * 2 - 1).to(DEV) for _ in range(4)]
    gan, optD, optG, losses, prm = make(case)
    train_iteration(gan, batches()[0], code(gan, tokens), optD, optG, losses, prm, DEV)          # burn-in
    gan, optD, optG, losses, prm = make(case)
    seed(5)
    eager = []
    for x in batches():
        lD, lG, _, _ = train_iteration(gan, x, code(gan, tokens), optD, optG, losses, prm, DEV)
        eager.append((float(lD), float(lG)))
    gan, optD, optG, losses, prm = make(case)
    seed(5)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2, cond_dim=256 if tokens is not None else 0)
    for i, x in enumerate(batches()):
        lD, lG = gs.step(x, code(gan, tokens))
        got = (float(lD), float(lG))
        print('step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = (2e-5 if i < 2 else 2e-3) if tokens is not None else (5e-6 if i < 2 else 5e-4 if i == 2 or M == 1 else 2e-2)
        assert abs(got[0] - eager[i][0]) < tol and abs(got[1] - eager[i][1]) < tol, (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1
    assert nbt(gan.gen) == {4 * M}
    assert adam_steps(optD) == {4 * N} and adam_steps(optG) == {4 * M}
    path = str(tmp_path / 'ck.pt')
    torch.save({'optD': optD.state_dict(), 'optG': optG.state_dict()}, path)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    for key, mod, n in (('optD', gan.discrims[0], 4 * N), ('optG', gan.gen, 4 * M)):
        opt = Adam([{'params': mod.parameters()}], lr=2e-4, betas=(0.5, 0.999))
        opt.load_state_dict(ck[key])
        assert adam_steps(opt) == {n}, key


def test_two_rank_replicas_stay_identical_under_the_schedule():
    """tools/dp_check.py with a 2:2 schedule: one graph per part (N + M + 1 = 5), N + M = 4 exchanges per replayed iteration
    ('D', 'D', 'G', 'G'), and both ranks end with identical weights that differ from a solo run."""
    env = dict(os.environ, T2V_DIST_BACKEND='gloo', T2V_SINGLE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29541', os.path.join(ROOT, 'tools', 'dp_check.py'), '--discrim_steps', '2', '--gen_steps', '2']
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith('DP_CHECK')]
    assert line and 'identical after 5 iterations: True' in line[0], out[-2000:]
    assert 'schedule 2:2, 5 graphs and exchanges DDGG per replayed iteration' in line[0], line[0]


def test_end2end_two_d_steps_vs_oracle():
    """--end2end with N = 2: the sentence code's graph is retained through both D backwards and the G backward, optD moves the
    text encoder twice and optG once (train/gan.py:82-85). The oracle composition: text_encode_grad, AdamOnData in both
    optimisers (see test_models_gpu.test_end2end_iteration_vs_oracle for the 1:1 case)."""
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    case = dict(S.CASES['c'])
    gan, _, _, losses, prm = make(case)
    txt = gan.cond_encoder.differentiable(True)
    dis, gen = gan.discrims[0], gan.gen
    optD = Adam([{'params': dis.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    PG, PD, PT, pre = S.oracle_states(case)
    before = {k: v.detach().clone() for k, v in PT.items()}
    g_keys = [k for k, v in PG.items() if v.dtype.is_floating_point and 'running_' not in k]
    d_keys = [k for k, v in PD.items() if v.dtype.is_floating_point]
    t_keys = [k for k in PT if 'to_vocab' not in k]
    for P, keys in ((PG, g_keys), (PD, d_keys), (PT, t_keys)):
        for k in keys:
            P[k].requires_grad_(True)
    oD = O.AdamOnData([PD[k] for k in d_keys] + [PT[k] for k in t_keys], 2e-4, (0.5, 0.999))
    oG = O.AdamOnData([PG[k] for k in g_keys] + [PT[k] for k in t_keys], 2e-4, (0.5, 0.999))
    tg = torch.Generator()
    tg.manual_seed(5)
    tokens = torch.randint(4, S.V, (S.B, 8), generator=tg)
    tokens[:, 0], tokens[:, -1] = 1, 2
    lengths = [8] * S.B
    seed(31)
    x = S.batch()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    _, _, cond = txt.encode(tokens.to(DEV), lengths)
    assert cond.requires_grad
    lD, lG, _, _ = train_iteration(gan, x.to(DEV), cond, optD, optG, losses, prm, DEV, end2end=True)
    lD, lG = float(lD), float(lG)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    # ---- oracle: trainer.py:211-263 with N = 2, M = 1
    c = O.text_encode_grad(PT, tokens, lengths)
    xs, conds, _ = O.multiscale_data(x, c, S.FS)
    z = torch.randn(S.B, 256)
    fake = O.multiscale_gen(PG, z, conds[0], training=True)
    lDo = 0.0
    for _ in range(2):
        for P, keys in ((PD, d_keys), (PT, t_keys)):
            for k in keys:
                P[k].grad = None
        fc0 = conds[0][O.gen_perm(S.B)]
        l = O.discrim_loss(PD, pre, xs, [f.detach() for f in fake], conds, [fc0[0:cc.size(0)] for cc in conds], 0.5)
        l.backward(retain_graph=True)
        oD.step()
        lDo += float(l.detach())
    O.gen_perm(S.B)
    real_pred = O.multiscale_discrim(PD, xs, conds, pre)
    for P, keys in ((PG, g_keys), (PT, t_keys)):
        for k in keys:
            P[k].grad = None
    l = O.gen_loss(PD, pre, fake, real_pred, conds)
    l.backward()
    oG.step()
    lGo = float(l.detach())
    print('end2end 2:1: HIP lossD %.6f lossG %.6f | oracle %.6f %.6f' % (lD, lG, lDo, lGo))
    assert abs(lD - lDo) < 1e-3 and abs(lG - lGo) < 1e-3
    assert adam_steps(optD) == {2} and adam_steps(optG) == {1}
    named = dict(txt.encoder.named_parameters())
    for k in ('encoder.embed.weight', 'encoder.lstm.weight_hh_l0', 'encoder.lstm.weight_ih_l3_reverse', 'encoder.lstm.bias_ih_l2'):
        d_o = PT[k].detach() - before[k]
        d_p = named[k[len('encoder.'):]].detach().cpu() - before[k]
        rel = float((d_p - d_o).abs().mean() / d_o.abs().mean().clamp_min(1e-12))
        assert float(d_o.abs().max()) > 0 and rel < 0.05, (k, rel)


def test_cli_wgan_gp_schedule_checkpoint_resume(tmp_path):
    """The reference's WGAN-GP recipe (scripts/run_tgan.sh: --D_loss ...WassersteinGanLoss --gp_lambda 10 --discrim_steps 5, here
    3) through the command line on the TGANv2 models: 3 iterations (2 eager, capture, replay), a checkpoint whose Adam counters
    are 3N and 3, and a resume from it."""
    import json
    cfg = str(tmp_path / 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    base = ['--data', cfg, '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
            '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0', '--D_beta2', '.9', '--G_beta1', '0', '--G_beta2', '.9',
            '--D_loss', 'txt2vid.gan.losses.WassersteinGanLoss', '--gp_lambda', '10', '--discrim_steps', '3',
            '--init_method', 'xavier', '--seed', '100', '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--epochs', '1', '--out', out_dir, '--out_samples', smp]

    def run(args):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert p.returncode == 0, out[-3000:]
        return out
    log = run(base + ['--max_iters', '3', '--save_model_period', '3', '--save_example_period', '0'])
    assert 'Iter 3, Loss_D' in log
    ck = glob.glob(os.path.join(out_dir, 'iter_3_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert {int(st['step']) for st in sd['optD']['state'].values()} == {9}
    assert {int(st['step']) for st in sd['optG']['state'].values()} == {3}
    log2 = run(base + ['--max_iters', '2', '--weights', ck[0], '--save_model_period', '1000', '--save_example_period', '0'])
    assert 'Iter 2, Loss_D' in log2
