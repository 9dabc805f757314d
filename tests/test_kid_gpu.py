"""GPU: the Kernel Inception Distance evaluation (`--eval_period`; DESIGN "KID evaluation") on the HIP path, against the float64
restatement of tests/kid_cases.py: `t2v_kid_sums` through the raw ABI on guarded buffers at the derived bound, its determinism,
the evaluator's isolation from the training loop (bitwise), its consistency with the restatement, the feature network against the
oracle's trunk, `--eval_net`, the checkpoint, the launch budget and the command line."""
import ctypes as C
import functools
import glob
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import kid_cases as K
import schedule_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B = S.V, S.B
CLIPS, BLOCK = 2 * B, B                              # --eval_clips = two batches, --eval_block = one batch
KINDS = ['cond', 'uncond']


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _trace(monkeypatch, fn):
    """Names of the C entry points `fn` calls, in order."""
    from txt2vid_amd import _lib
    L, calls = _lib.lib(), []

    def wrap(name, orig):
        def f(*a):
            calls.append(name)
            return orig(*a)
        return f
    with monkeypatch.context() as mp:
        for name in _lib.SIGNATURES:
            mp.setattr(L, name, wrap(name, getattr(L, name)))
        fn()
    torch.cuda.synchronize()
    return calls


# ------------------------------------------------------------------------------------------------ op level: the raw ABI, guarded

SENTINEL = -7777.25
GUARD = 64


class Guarded64(object):
    """`n` doubles carved out of a larger allocation, GUARD sentinel doubles on each side; the inside starts as NaN, so an
    element the kernel never wrote fails the comparison."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float64)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(float('nan'))
        self.p = C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


def _raw(case):
    """(out [nb, 3] float64 on the host, intact flags, X and Y unmodified) of one guarded call."""
    from txt2vid_amd._lib import lib
    from txt2vid_amd._ops import _stream
    L = lib()
    X, Y, alpha = K.inputs(case)
    s, d, nb = case[:3]
    Xd, Yd = torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(Y.copy()).to(DEV)
    need = L.t2v_kid_sums_ws_bytes(nb * s, d, s)
    assert need > 0 and need % 8 == 0
    out, ws = Guarded64(nb * 3), Guarded64(need // 8)
    st = L.t2v_kid_sums(C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr()), nb * s, d, s, alpha, out.p, ws.p, _stream())
    assert st == 0
    torch.cuda.synchronize()
    same = torch.equal(Xd.cpu(), torch.from_numpy(X.copy())) and torch.equal(Yd.cpu(), torch.from_numpy(Y.copy()))
    return out.t.cpu().numpy().reshape(nb, 3).copy(), out.intact() and ws.intact(), same


@pytest.mark.parametrize('case', K.CASES + [K.LARGE_ALPHA] + K.TILED, ids=K.case_id)
def test_sums_on_guarded_buffers_within_the_derived_bound(case):
    X, Y, alpha = K.inputs(case)
    s, d, nb = case[:3]
    got, intact, same = _raw(case)
    assert intact and same
    ref, mag = K.sums(X, Y, s, alpha), K.magnitudes(X, Y, s, alpha)
    ratio = np.abs(got - ref) / (K.op_bound(d, s) * mag)
    print('kid-ratio %s per block and sum: %s' % (K.case_id(case), np.array2string(ratio, precision=4)))
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), ratio
    again, _, _ = _raw(case)
    assert got.tobytes() == again.tobytes()                                  # two calls: the same bits


def test_wrapper_reuses_buffers_and_matches_the_raw_call():
    from txt2vid_amd.functional_kid import kid_sums_raw
    case = (33, 70, 2)
    X, Y, alpha = K.inputs(case)
    Xd, Yd = torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(Y.copy()).to(DEV)
    a = kid_sums_raw(Xd, Yd, 33, alpha)
    out = torch.zeros(2, 3, device=DEV, dtype=torch.float64)
    ws = torch.zeros(4096, device=DEV, dtype=torch.float64).view(torch.uint8)
    b = kid_sums_raw(Xd, Yd, 33, alpha, out=out, ws=ws)
    assert b is out and torch.equal(a, b) and a.cpu().numpy().tobytes() == _raw(case)[0].tobytes()
    with pytest.raises(ValueError, match='KID'):
        kid_sums_raw(Xd, Yd, 32, alpha)
    with pytest.raises(ValueError, match='workspace'):
        kid_sums_raw(Xd, Yd, 33, alpha, ws=ws[:8])


def test_entry_point_refuses_bad_arguments_and_launches_nothing():
    from txt2vid_amd._lib import lib
    L = lib()
    buf = torch.full((4096,), 3.5, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    for n, d, s, x, ws in ((8, 4, 3, p, p), (1, 4, 1, p, p), (8, 0, 4, p, p), (8, 4, 1, p, p), (8, 4, 4, None, p), (8, 4, 4, p, None)):
        assert L.t2v_kid_sums(x, p, n, d, s, 0.25, p, ws, None) == -1
    torch.cuda.synchronize()
    assert bool((buf == 3.5).all())


def test_symbols_are_exported_and_declared():
    from txt2vid_amd import _lib
    header = open(os.path.join(ROOT, 'include', 't2v_hip.h')).read()
    assert [k for k in _lib.SIGNATURES if k.startswith('t2v_kid_')] == ['t2v_kid_sums', 't2v_kid_sums_ws_bytes']
    assert 'int t2v_kid_sums(' in header and 'size_t t2v_kid_sums_ws_bytes(' in header and hasattr(_lib.lib(), 't2v_kid_sums')


# ------------------------------------------------------------------------------------------------ host layer

def pour(module):
    module.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()})
    return module.to(DEV)


def make(kind):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    txt = None
    if kind == 'uncond':
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
        dis = pour(MultiScaleDiscrim(num_channels=1)).train()
    else:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
        from txt2vid_amd.models.txt.basic import Seq2Seq
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256)).train()
        dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256)).train()
        txt = Seq2Seq(vocab_size=V)
        txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                             for k, v in txt.state_dict().items()})
        txt.to(DEV)
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), prm


def tokens_for(batch, s=77):
    tg = torch.Generator()
    tg.manual_seed(s)
    t = torch.randint(4, V, (batch, 8), generator=tg)
    t[:, 0], t[:, -1] = 1, 2
    return t


def code(gan, tokens):
    if gan.cond_encoder is None:
        return None
    with torch.no_grad():
        return gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()


def evaluator(gan, **kw):
    from txt2vid_amd.gan.kid import KidEvaluator
    kw = dict(dict(clips=CLIPS, block=BLOCK, num_channels=1, period=1, sample_batch=B), **kw)
    return KidEvaluator(gan, DEV, **kw)


@functools.lru_cache(maxsize=None)
def loop(kind, graph, on, ema=False, iters=3):
    """Three iterations the way train() runs them — observe in front of the step, the evaluation behind it — with or without the
    evaluator. Returns everything the isolation test compares, and the gan."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.ema import GenAverage
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    TF.set_grad_sink(None)
    gan, optD, optG, losses, prm = make(kind)
    if ema:
        gan.gen_ema = GenAverage(gan.gen, 0.9, start=0)
    if on:
        gan.kid = evaluator(gan)
    tokens = tokens_for(B)
    seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2,
                          cond_dim=256 if kind != 'uncond' else 0) if graph else None
    seen, recs, live = [], [], []
    for it in range(1, iters + 1):
        x = S.batch().to(DEV)
        cnd = code(gan, tokens)
        if on and not gan.kid.full:
            gan.kid.observe(x, cnd)
        if graph:
            lD, lG = gs.step(x, cnd)
        else:
            lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, cnd)
        seen.append((lD.detach().clone(), lG.detach().clone()))
        if on:
            before = [p.detach().clone() for p in gan.gen.parameters()]
            recs.append(gan.kid.step(it))
            live.append(all(torch.equal(a, b) for a, b in zip(before, gan.gen.parameters())) and gan.gen.training)
    torch.cuda.synchronize()
    if graph:
        assert gs.graphs is not None
        gs.release()
    TF.set_grad_sink(None)
    state = {'losses': seen,
             'G': {k: v.detach().clone() for k, v in gan.gen.state_dict().items()},
             'D': {k: v.detach().clone() for k, v in gan.discrims[0].state_dict().items()},
             'ema': None if gan.gen_ema is None else {k: v.clone() for k, v in gan.gen_ema.state_dict().items()},
             'rng': (torch.get_rng_state(), np.random.get_state()[1].copy(), random.getstate())}
    return state, recs, live, gan


CONFIGS = [('cond', True, False), ('cond', False, False), ('uncond', True, False), ('uncond', False, False), ('uncond', True, True)]


@pytest.mark.parametrize('kind,graph,ema', CONFIGS, ids=lambda v: str(v))
def test_isolation_the_loop_computes_the_same_bits_with_and_without_the_flag(kind, graph, ema):
    off, _, _, _ = loop(kind, graph, False, ema)
    on, recs, live, gan = loop(kind, graph, True, ema)
    assert recs[0] is None and recs[1] is not None and recs[2] is not None           # the bank fills in two iterations
    assert all(math.isfinite(r['kid']) and r['stderr'] is not None and r['alpha'] > 0 for r in recs[1:])
    for (a, b), (c, d) in zip(off['losses'], on['losses']):
        assert torch.equal(a, c) and torch.equal(b, d)
    for part in ('G', 'D'):                                                         # parameters and BatchNorm buffers
        assert list(off[part]) == list(on[part])
        assert all(torch.equal(off[part][k], on[part][k]) for k in off[part]), part
    assert any('running_mean' in k for k in off['G'])
    assert torch.equal(off['rng'][0], on['rng'][0]) and np.array_equal(off['rng'][1], on['rng'][1]) and off['rng'][2] == on['rng'][2]
    assert all(live)                                                                # live weights and train mode are back
    if ema:
        assert all(torch.equal(off['ema'][k], on['ema'][k]) for k in off['ema'])
    print('kid %s graph=%s ema=%s: %s' % (kind, graph, ema, [(r['iteration'], r['kid'], r['stderr']) for r in recs[1:]]))
    assert recs[1]['kid'] != recs[2]['kid']                                         # the generator moved in between


@pytest.mark.parametrize('kind', KINDS)
def test_consistency_the_logged_kid_is_the_restatement_on_the_banks(kind):
    _, recs, _, gan = loop(kind, True, True, False)
    ev, rec = gan.kid, recs[2]
    X, Y = ev.real_bank.cpu().numpy(), ev.fake_bank.cpu().numpy()
    assert X.shape == (CLIPS, 1024) and rec == ev.last and (rec['clips'], rec['block']) == (CLIPS, BLOCK)
    assert abs(rec['alpha'] - K.default_alpha(X)) <= 1e-6 * rec['alpha']             # (row norms in fp32, their mean on the host)
    kid, stderr = K.kid(X, Y, BLOCK, rec['alpha'])
    bound = K.estimate_bound(X, Y, BLOCK, rec['alpha'])
    print('kid consistency %s: %.12g vs %.12g, bound %.3g' % (kind, rec['kid'], kid, bound))
    assert abs(rec['kid'] - kid) <= bound and abs(rec['stderr'] - stderr) <= 2 * bound
    if kind == 'cond':
        assert ev.cond_bank is not None and tuple(ev.cond_bank.shape) == (CLIPS, 256) and bool(ev.cond_bank.any())
    else:
        assert ev.cond_bank is None
    # two evaluations without a training step in between: fixed latents, the same bits
    a = dict(ev.evaluate(7))
    fa, sa = ev.fake_bank.clone(), ev.sums.clone()
    b = dict(ev.evaluate(7))
    assert a == b and torch.equal(fa, ev.fake_bank) and torch.equal(sa, ev.sums) and a['kid'] == rec['kid']


def test_features_equal_the_oracle_trunk_on_the_same_weights():
    """Tolerance of tests/test_models_gpu.py for the discriminator's features (`close`: rtol 1e-3, atol 1e-4 x scale)."""
    from txt2vid_amd.gan.kid import feature_network
    net, _ = feature_network(1, DEV)
    seed(5)
    x = S.batch()[:2].contiguous()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(x.to(DEV))[2]
        _, _, want = O.resnet3d({k: v.cpu() for k, v in net.state_dict().items()}, x)
    assert tuple(got.shape) == (2, 1024)
    a, b = got.cpu().double().numpy(), want.double().numpy()
    np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4 * max(1.0, float(np.abs(b).max())))
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def test_eval_net_loads_the_golden_checkpoint_and_evaluates():
    gan = make('uncond')[0]
    ev = evaluator(gan, net=os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint_uncond.pt'))
    assert 'ref_checkpoint_uncond.pt' in ev.net_name
    seed(8)
    for _ in range(2):
        ev.observe(S.batch().to(DEV))
    rec = ev.evaluate(0)
    assert ev.full and math.isfinite(rec['kid']) and rec['net'] == ev.net_name and rec['stderr'] is not None


def test_launch_budget_a_non_evaluation_iteration_is_the_flag_off_iteration(monkeypatch):
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import TrainStep
    out = {}
    for on in (True, False):
        gan, optD, optG, losses, prm = make('uncond')
        if on:
            gan.kid = evaluator(gan, period=5)
        step = TrainStep(gan, optD, optG, losses, prm, DEV)
        seed(3)
        for it in (1, 2):                                            # fills the bank (and the packed-weight caches)
            x = S.batch().to(DEV)
            if on:
                gan.kid.observe(x, None)
            step.run(x, None)
            if on:
                assert gan.kid.step(it) is None
        assert not on or gan.kid.full
        x = S.batch().to(DEV)

        def iteration():
            if on and not gan.kid.full:
                gan.kid.observe(x, None)
            step.run(x, None)
            if on:
                assert gan.kid.step(3) is None
        out[on] = _trace(monkeypatch, iteration)
        TF.set_grad_sink(None)
    assert out[True] == out[False] and len(out[False]) > 100 and 't2v_kid_sums' not in out[True]


# ------------------------------------------------------------------------------------------------ command line

def _run(module, args, tmp, ok=True):
    cfg = os.path.join(str(tmp), 'synth.json')
    with open(os.path.join(ROOT, 'tools', 'cfg', 'synth.json')) as f:
        spec = json.load(f)
    with open(cfg, 'w') as f:
        json.dump(spec, f)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', module, '--data', cfg] + args
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=700)
    out = p.stdout.decode(errors='replace')
    assert (p.returncode == 0) == ok, out[-3000:]
    return out


def test_cli_train_writes_metrics_and_the_stand_alone_entry_reads_the_checkpoint(tmp_path):
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    base = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002',
            '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--gp_lambda', '.5',
            '--subsample_input', '--workers', '0', '--log_period', '1', '--dont_use_sent',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--batch_size', '8', '--epochs', '1', '--out', out_dir, '--out_samples', smp, '--save_example_period', '0']
    bad = _run('txt2vid_amd.train.gan', base + ['--eval_period', '2', '--eval_clips', '12', '--eval_block', '8'], tmp_path, ok=False)
    assert 'multiple of --eval_block' in bad
    ev = ['--eval_clips', '16', '--eval_block', '8']
    log = _run('txt2vid_amd.train.gan', base + ['--max_iters', '4', '--save_model_period', '4', '--eval_period', '2'] + ev, tmp_path)
    assert 'Iter 4, Loss_D' in log and 'Iter 2, KID: ' in log and 'Iter 4, KID: ' in log and 'features: random-init Resnet3D' in log
    with open(os.path.join(out_dir, 'metrics.jsonl')) as f:
        recs = [json.loads(l) for l in f]
    assert [r['iteration'] for r in recs] == [2, 4]
    for r in recs:
        assert set(r) == {'iteration', 'kid', 'stderr', 'clips', 'block', 'alpha', 'net'}
        assert math.isfinite(r['kid']) and math.isfinite(r['stderr']) and (r['clips'], r['block']) == (16, 8) and r['alpha'] > 0
    ck = glob.glob(os.path.join(out_dir, 'iter_4_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    plain = make('uncond')[0]
    assert set(sd) == {'optG', 'optD', 'iteration', 'rng_state', 'gen', 'video'}                # nothing of the evaluator
    assert list(sd['video']) == list(plain.discrims[0].state_dict()) and not any('kid' in k for k in sd)
    plain.load_from_dict(sd)                                                                    # loads without the flag
    alone = _run('txt2vid_amd.gan.kid', base + ['--weights', ck[0]] + ev, tmp_path)
    rec = json.loads([l for l in alone.splitlines() if l.startswith('{')][-1])
    assert set(rec) == set(recs[0]) and rec['iteration'] == 4 and math.isfinite(rec['kid']) and rec['net'] == recs[0]['net']
