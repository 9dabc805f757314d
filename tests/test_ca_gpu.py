"""GPU: the generator's opt-in conditioning augmentation (MultiScaleGen(ca_dim=D); DESIGN "Conditioning augmentation") on the
HIP path, against the CPU restatement composed with the oracle (tests/ca_cases.py): the two kernels against fp64 autograd, the
module, three training iterations (1:1 and 2:1), graph replay, --end2end, bf16 compute and the command line."""
import glob
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import ca_cases as CA
import schedule_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B = S.V, S.B


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def pour(module):
    module.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()})
    return module.to(DEV)


def tokens_for(batch, s=77):
    tg = torch.Generator()
    tg.manual_seed(s)
    t = torch.randint(4, V, (batch, 8), generator=tg)
    t[:, 0], t[:, -1] = 1, 2
    return t


def make(D, N=1, M=1, batch=B):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, ca_dim=D)).train()
    dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256)).train()
    txt = Seq2Seq(vocab_size=V)
    txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                         for k, v in txt.state_dict().items()})
    txt.to(DEV)
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    prm = S.params_for(dict(N=N, M=M, gp=0.5, mean_d=False, mean_g=False))
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), prm


# ------------------------------------------------------------------------------------------------ op level

@pytest.mark.parametrize('Bn', [1, 3, 32])
@pytest.mark.parametrize('D', [64, 100, 128])
def test_ca_kernels_vs_fp64_autograd(Bn, D):
    from txt2vid_amd.functional_ca import cond_aug
    L = 256
    g = torch.Generator()
    g.manual_seed(1000 * Bn + D)
    h = torch.randn(Bn, 4 * D, generator=g)
    z, eps = torch.randn(Bn, L, generator=g), torch.randn(Bn, D, generator=g)
    gout, gkl = torch.randn(Bn, L + D, generator=g), torch.randn((), generator=g)
    c_ref, kl_ref = CA.ca_ref(h.double(), eps.double())
    hd = h.to(DEV).requires_grad_(True)
    out, kl = cond_aug(hd, z.to(DEV), eps.to(DEV))
    assert torch.equal(out[:, :L].cpu(), z)                               # z passes through bit-exactly
    np.testing.assert_allclose(out[:, L:].detach().cpu().double().numpy(), c_ref.numpy(), rtol=1e-5,
                               atol=1e-6 * float(c_ref.abs().max()))
    assert abs(float(kl.detach()) - float(kl_ref)) <= 1e-5 * abs(float(kl_ref))
    _, kl2 = cond_aug(hd, z.to(DEV), eps.to(DEV))
    assert torch.equal(kl.detach().cpu(), kl2.detach().cpu())            # fixed-order reduction: the same bits every run
    for branch in ('both', 'c', 'kl', 'coeff0'):
        hr = h.double().requires_grad_(True)
        c, k = CA.ca_ref(hr, eps.double())
        gc = gout[:, L:].double()
        if branch == 'both':
            ref = (c * gc).sum() + 1.5 * float(gkl) * k
        elif branch == 'c' or branch == 'coeff0':
            ref = (c * gc).sum()
        else:
            ref = 1.5 * float(gkl) * k
        want, = torch.autograd.grad(ref, hr)
        hd = h.to(DEV).requires_grad_(True)
        out, kl = cond_aug(hd, z.to(DEV), eps.to(DEV), kl_coeff=0.0 if branch == 'coeff0' else 1.5)
        outs, grads = [], []
        if branch in ('both', 'c', 'coeff0'):
            outs.append(out)
            grads.append(gout.to(DEV))
        if branch in ('both', 'kl', 'coeff0'):
            outs.append(kl)
            grads.append(gkl.to(DEV))
        got, = torch.autograd.grad(outs, hd, grads)
        np.testing.assert_allclose(got.cpu().double().numpy(), want.numpy(), rtol=1e-5, atol=1e-6 * float(want.abs().max()),
                                   err_msg=branch)


def test_ca_kernels_refuse_bad_arguments():
    from txt2vid_amd._lib import lib
    assert lib().t2v_ca_fwd(None, None, None, None, None, 4, 256, 128, None) < 0
    assert lib().t2v_ca_bwd(None, None, 1.0, None, None, None, 0, 256, 128, None) < 0


# ------------------------------------------------------------------------------------------------ module level

def test_ca_generator_vs_cpu_composition():
    """Forward + backward of a CA-enabled conditional MultiScaleGen with fixed z / eps / phases against CA + oracle.multiscale_gen:
    the rendered pyramid, KL, every per-parameter gradient norm (ca.fc.* included) and dL/ds. Tolerances of test_models_gpu.test_gen."""
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    D, coeff = 128, 2.0
    m = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, ca_dim=D)).train()
    PG = CA.gen_state(D)
    keys = [k for k, _ in m.named_parameters()]
    for k in keys:
        PG[k].requires_grad_(True)
    g = torch.Generator()
    g.manual_seed(3)
    z, s = torch.randn(B, 256, generator=g), 0.5 * torch.randn(B, 256, generator=g)
    seed(5)
    sd = s.to(DEV).requires_grad_(True)
    fake, kl = m(z.to(DEV), cond=sd, return_kl=True)
    weights = [torch.randn(*f.shape, generator=g) for f in fake]
    loss = sum((f * w.to(DEV)).sum() for f, w in zip(fake, weights)) + coeff * kl
    loss.backward()
    seed(5)
    so = s.clone().requires_grad_(True)
    fo, klo = CA.gen_ca(PG, z, so)                            # eps drawn first, then the 3 phases: the module's order
    lo = sum((f * w).sum() for f, w in zip(fo, weights)) + coeff * klo
    lo.backward()
    for a, b in zip(fake, fo):
        scale = max(1.0, float(b.abs().max()))
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-3, atol=5e-4 * scale)
    assert abs(float(kl.detach()) - float(klo)) < 1e-5 * max(1.0, abs(float(klo)))
    got = np.array([float(p.grad.norm()) for _, p in m.named_parameters()])
    want = np.array([float(PG[k].grad.norm()) for k in keys])
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    assert rel < 3e-3, rel
    for k in ('ca.fc.weight', 'ca.fc.bias', 'fc.weight'):
        gk, wk = float(dict(m.named_parameters())[k].grad.norm()), float(PG[k].grad.norm())
        assert abs(gk - wk) < 3e-3 * wk, (k, gk, wk)
    # dL/ds sits behind the whole generator's backward (16 LSTM steps, 4 levels of training-mode BatchNorm) and two more GEMMs:
    # compared as one vector, like the gradient norms (single elements carry ~2e-3 of the tensor's scale in summation noise)
    ds = so.grad.double()
    rel = float((sd.grad.cpu().double() - ds).norm() / ds.norm())
    assert rel < 3e-3, rel
    # eval mode samples too (a fresh eps per call: one caption, several videos)
    m.eval()
    with torch.no_grad():
        seed(6)
        v1 = m(z[:2].to(DEV), cond=sd[:2].detach())
        v2 = m(z[:2].to(DEV), cond=sd[:2].detach())
        seed(6)
        e1 = CA.gen_ca(PG, z[:2], s[:2], training=False)[0]
    assert len(v1) == 1 and not torch.equal(v1[0], v2[0])
    np.testing.assert_allclose(v1[0].cpu().numpy(), e1[0].detach().numpy(), rtol=2e-3, atol=5e-4 * max(1.0, float(e1[0].abs().max())))


# ------------------------------------------------------------------------------------------------ iteration level

@pytest.mark.parametrize('N,M', [(1, 1), (2, 1)])
def test_ca_iterations_vs_cpu_composition(N, M):
    """Three text-conditioned iterations with CA against the oracle loop plus CA: lossD, lossG (with 2 * KL) and KL, bounds of the
    existing conditional step tests (1e-3, then 2e-2 in iteration 2: the GAN dynamics are chaotic)."""
    from txt2vid_amd.gan.trainer import TrainStep
    D = 128
    tokens = tokens_for(B)
    ref = CA.oracle_loop(N, M, D, tokens, iters=3)
    gan, optD, optG, losses, prm = make(D, N, M)
    seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        with torch.no_grad():
            cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        lD, lG, _, _ = ts.run(x, cond)
        lD, lG, lK = float(lD), float(lG), float(ts.lKL)
        tol = 1e-3 if it < 2 else 2e-2
        print('CA %d:%d it %d: lossD %.6f (%.6f) lossG %.6f (%.6f) KL %.6f (%.6f)' % (N, M, it, lD, ref['lossD'][it], lG,
                                                                                     ref['lossG'][it], lK, ref['KL'][it]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))
        assert abs(lK - ref['KL'][it]) < tol * max(1.0, abs(ref['KL'][it]))


def test_ca_graph_replay_matches_eager():
    """GraphedTrainStep with CA (eps among the device-resident draws, the CA launches inside the one captured graph) reproduces the
    eager iterations: 2 eager, then capture + replays."""
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    D, tokens = 128, tokens_for(B).to(DEV)

    def batches():
        g = torch.Generator()
        g.manual_seed(12)
        return [(torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]
    gan, optD, optG, losses, prm = make(D)
    seed(6)
    eager = []
    for x in batches():
        cond = gan.cond_encoder.encode(tokens, [8] * B)[2].detach()
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        lD, lG, _, _ = ts.run(x, cond)
        eager.append((float(lD), float(lG), float(ts.lKL)))
    gan, optD, optG, losses, prm = make(D)
    seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2, cond_dim=256)
    assert gs.draws.ca_dim == D
    for i, x in enumerate(batches()):
        cond = gan.cond_encoder.encode(tokens, [8] * B)[2].detach()
        lD, lG = gs.step(x, cond)
        got = (float(lD), float(lG), float(gs.ts.lKL))
        print('CA step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1


def test_ca_end2end_encoder_gradient_vs_cpu_composition():
    """--end2end with CA: the sentence code keeps its graph, so the G step's gradient reaches the text encoder through CA's fc
    (and D's conditional heads). One iteration: both losses and the encoder's gradient norms left by the G step."""
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    D, coeff = 128, 2.0
    gan, _, _, losses, prm = make(D)
    txt = gan.cond_encoder.differentiable(True)
    dis, gen = gan.discrims[0], gan.gen
    optD = Adam([{'params': dis.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    _, PD, PT, pre = S.oracle_states(dict(cond=True))
    PG = CA.gen_state(D)
    tr = O.OracleTrainer(PG, PD, d_prefix=pre, end2end_txt=PT)
    tokens, lengths = tokens_for(B, 5), [8] * B
    seed(31)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    cond = txt.encode(tokens.to(DEV), lengths)[2]
    assert cond.requires_grad
    lD, lG, _, _ = train_iteration(gan, x.to(DEV), cond, optD, optG, losses, prm, DEV, end2end=True)
    lD, lG = float(lD), float(lG)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    # the oracle's step_end2end with CA on the generator input
    c = O.text_encode_grad(PT, tokens, lengths)
    xs, conds, _ = O.multiscale_data(x, c, S.FS)
    z = torch.randn(B, 256)
    fake, kl = CA.gen_ca(PG, z, conds[0])
    tr.zero(PD, tr.d_params)
    tr.zero(PT, tr.t_params)
    fc0 = conds[0][O.gen_perm(B)]
    lDo = O.discrim_loss(PD, pre, xs, [f.detach() for f in fake], conds, [fc0[0:cc.size(0)] for cc in conds], 0.5)
    lDo.backward(retain_graph=True)
    tr.optD.step()
    O.gen_perm(B)
    real_pred = O.multiscale_discrim(PD, xs, conds, pre)
    tr.zero(PG, tr.g_params)
    tr.zero(PT, tr.t_params)
    lGo = O.gen_loss(PD, pre, fake, real_pred, conds) + coeff * kl
    lGo.backward()
    lDo, lGo = float(lDo), float(lGo)
    print('CA end2end: HIP lossD %.6f lossG %.6f | oracle %.6f %.6f' % (lD, lG, lDo, lGo))
    assert abs(lD - lDo) < 1e-3 and abs(lG - lGo) < 1e-3
    named = dict(txt.encoder.named_parameters())
    ref_max = max(float(PT[k].grad.norm()) for k in tr.t_params)
    for k in tr.t_params:
        got, want = float(named[k[len('encoder.'):]].grad.norm()), float(PT[k].grad.norm())
        assert abs(got - want) <= 1e-2 * want + 1e-5 * ref_max, (k, got, want)
    gk, wk = float(gen.ca.fc.weight.grad.norm()), float(PG['ca.fc.weight'].grad.norm())
    assert abs(gk - wk) < 1e-2 * wk, (gk, wk)


def test_ca_iteration_bf16_vs_fp32_composition():
    """One conditional CA iteration in bf16-compute mode against the fp32 CPU composition, within the existing bf16 bound
    (|dlossD| < 2e-2, |dlossG| < 5e-2). The CA kernels stay fp32 whatever the mode."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import TrainStep
    D, tokens = 128, tokens_for(B)
    ref = CA.oracle_loop(1, 1, D, tokens, iters=1)
    gan, optD, optG, losses, prm = make(D)
    seed(100)
    x = S.batch().to(DEV)
    old = TF.set_conv_precision('bf16')
    try:
        with torch.no_grad():
            cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        lD, lG, _, _ = ts.run(x, cond)
        lD, lG, lK = float(lD), float(lG), float(ts.lKL)
    finally:
        TF.set_conv_precision(old)
    print('CA bf16: lossD %.6f (%.6f) lossG %.6f (%.6f) KL %.6f (%.6f)' % (lD, ref['lossD'][0], lG, ref['lossG'][0], lK,
                                                                         ref['KL'][0]))
    assert abs(lD - ref['lossD'][0]) < 2e-2 and abs(lG - ref['lossG'][0]) < 5e-2 and abs(lK - ref['KL'][0]) < 5e-2


# ------------------------------------------------------------------------------------------------ data parallel, command line

def test_ca_two_rank_replicas_stay_identical():
    """tools/dp_check.py --cond --ca_dim 128: the CA parameters sit in G's gradient arena and are exchanged with it."""
    env = dict(os.environ, T2V_DIST_BACKEND='gloo', T2V_SINGLE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29547', os.path.join(ROOT, 'tools', 'dp_check.py'), '--cond', '--ca_dim', '128']
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith('DP_CHECK')]
    assert line and 'identical after 5 iterations: True' in line[0] and 'ca_dim 128' in line[0], out[-2000:]


def _cli(args, tmp):
    cfg = os.path.join(str(tmp), 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    cmd = [sys.executable, '-m', 'txt2vid_amd.train.gan', '--data', cfg] + args
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    return out


def test_ca_cli_train_checkpoint_resume_and_sample(tmp_path):
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    base = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002',
            '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--gp_lambda', '.5',
            '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', os.path.join(ROOT, 'tools', 'cfg', 'gen_cond_ca.json'), '--D', 'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim',
            '--sent', 'txt2vid.models.txt.basic.Seq2Seq', '--batch_size', '8', '--epochs', '1', '--out', out_dir]
    log = _cli(base + ['--out_samples', smp, '--max_iters', '4', '--save_model_period', '4', '--save_example_period', '4'], tmp_path)
    assert 'Iter 4, Loss_D' in log and 'Iter 4, KL (conditioning augmentation' in log
    ck = glob.glob(os.path.join(out_dir, 'iter_4_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert tuple(sd['gen']['ca.fc.weight'].shape) == (512, 256) and tuple(sd['gen']['fc.weight'].shape) == (1024, 384)
    assert len(glob.glob(os.path.join(smp, 'fake_samples_epoch_000_iter_000004_*.png'))) == 4
    log2 = _cli(base + ['--out_samples', smp, '--max_iters', '2', '--weights', ck[0], '--save_model_period', '1000',
                        '--save_example_period', '0'], tmp_path)
    assert 'Iter 2, Loss_D' in log2
    smp2 = str(tmp_path / 'samples_test')
    _cli(base + ['--out_samples', smp2, '--test', '--weights', ck[0], '--num_samples', '1'], tmp_path)
    assert os.path.exists(os.path.join(smp2, 'real_0.png')) and os.path.exists(os.path.join(smp2, '64x64_0_0.jpg'))
    # a CA checkpoint into the CA-off generator: refused with a message that names ca_dim
    cmd = [sys.executable, '-m', 'txt2vid_amd.train.gan', '--data', os.path.join(str(tmp_path), 'synth.json')] + \
        [a if a != os.path.join(ROOT, 'tools', 'cfg', 'gen_cond_ca.json') else 'txt2vid.models.tganv2_cond.gen.MultiScaleGen'
         for a in base] + ['--out_samples', smp2, '--test', '--weights', ck[0]]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode != 0 and b'ca_dim' in p.stdout
