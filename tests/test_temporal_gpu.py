"""GPU: the frame-seed generator of MultiScaleGen(no_lstm=True) (csrc/temporal.hip via functional_temporal) against
  (a) torch autograd on the CPU, layer by layer (F.conv_transpose1d / F.batch_norm / relu / tanh),
  (b) the golden vectors recorded from the REAL reference (tests/golden/*_nolstm.*),
  (c) the eager iteration (graph replay) and the command line."""
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rtol=1e-3, atol=1e-4):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale)


def pour(module, **kw):
    sd = module.state_dict()
    module.load_state_dict({k: O.recipe_tensor(k, v.shape, **kw) for k, v in sd.items()})
    return module.to(DEV)


def rnd(seed, *shape):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def norms_close(module, g, prefix, rtol=2e-3):
    """As tests/test_models_gpu.py: biases in front of a training-mode BatchNorm have an exactly-zero true gradient, so an
    absolute floor of 1e-7 * max-norm absorbs their rounding noise."""
    got = {k: (float(p.grad.norm()) if p.grad is not None else 0.0) for k, p in module.named_parameters()}
    vals = [max(float(v), 0.0) for v in g[prefix + '_vals']]
    floor = 1e-7 * max(vals) + 1e-6
    for k, v in zip([str(k) for k in g[prefix + '_keys']], vals):
        assert abs(got[k] - v) <= rtol * abs(v) + floor, (k, got[k], v)


# ---------------------------------------------------------------------------------------------------------------------
# op level: every layer shape the generator launches
def _cpu_reference(fsg, x, training):
    """The reference's FrameSeedGenerator.forward (temporal_gen.py:27-33) with torch ops on CPU copies of the parameters.
    Returns (z, params, buffers) — params in named_parameters order, buffers updated in place."""
    P = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in fsg.named_parameters()}
    Bf = {k: v.detach().cpu().clone() for k, v in fsg.named_buffers()}
    Bf = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in Bf.items()}
    h = x.double().reshape(x.size(0), -1, 1)                 # (x: a CPU tensor; its gradient is compared)
    for i in range(4):
        h = F.conv_transpose1d(h, P['dc%d.weight' % i], P['dc%d.bias' % i], stride=1 if i == 0 else 2, padding=0 if i == 0 else 1)
        h = F.relu(F.batch_norm(h, Bf['bn%d.running_mean' % i], Bf['bn%d.running_var' % i], P['bn%d.weight' % i], P['bn%d.bias' % i],
                                training, 0.1, 1e-5))
    z = torch.tanh(F.conv_transpose1d(h, P['dc4.weight'], P['dc4.bias'], stride=2, padding=1))
    return z, P, Bf


@pytest.mark.parametrize('fm', [1024, 4096])
@pytest.mark.parametrize('B', [2, 4, 5, 32])
def test_frame_seed_layers_vs_torch(fm, B):
    from txt2vid_amd.models.tgan.temporal_gen import FrameSeedGenerator
    fsg = FrameSeedGenerator(fm, fm)
    fsg.load_state_dict({k: O.recipe_tensor('frame_seed_gen.' + k, v.shape) for k, v in fsg.state_dict().items()})
    fsg.to(DEV).train()
    x = rnd(3, B, fm)
    xd = x.to(DEV).requires_grad_(True)
    proj = rnd(4, B, fm, 16)
    xc = x.double().requires_grad_(True)
    zr, P, Bf = _cpu_reference(fsg, xc, True)             # (first: from the buffers before this step's update)
    (zr * proj.double()).sum().backward()
    z = fsg(xd)
    assert z.shape == (B, fm, 16) and z.is_contiguous()
    (z * proj.to(DEV)).sum().backward()
    close(z, zr, rtol=1e-4, atol=1e-5)
    close(xd.grad, xc.grad, rtol=1e-3, atol=1e-4)
    for k, p in fsg.named_parameters():
        if k.startswith('dc') and k.endswith('bias') and k != 'dc4.bias':
            # in front of a training-mode BatchNorm: the true gradient is zero; both sides hold rounding noise
            assert float(p.grad.abs().max()) < 1e-3 * max(1.0, float(P['dc%s.weight' % k[2]].grad.abs().max())), k
            continue
        close(p.grad, P[k].grad, rtol=1e-3, atol=1e-4)
    for k, v in fsg.named_buffers():
        if v.dtype.is_floating_point:
            close(v, Bf[k], rtol=1e-5, atol=1e-6)
        else:
            assert int(v) == 1, k
    # eval mode: running statistics (a batch of one is legal)
    fsg.eval()
    with torch.no_grad():
        ze = fsg(xd[:1])
    zre, _, _ = _cpu_reference(fsg, x[:1], False)
    close(ze, zre, rtol=1e-4, atol=1e-5)


def test_frame_seed_backward_accumulates_into_the_gradient_sink():
    """Inside a training step the parameter gradients land in the generator's arena (GradSink), like every other layer's."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.dist import model_arena
    from txt2vid_amd.models.tgan.temporal_gen import FrameSeedGenerator
    fsg = FrameSeedGenerator(1024, 1024)
    fsg.load_state_dict({k: O.recipe_tensor('frame_seed_gen.' + k, v.shape) for k, v in fsg.state_dict().items()})
    fsg.to(DEV).train()
    x = rnd(3, 4, 1024).to(DEV).requires_grad_(True)
    proj = rnd(4, 4, 1024, 16).to(DEV)
    (fsg(x) * proj).sum().backward()
    ref = {k: p.grad.clone() for k, p in fsg.named_parameters()}
    for p in fsg.parameters():
        p.grad = None
    arena = model_arena(fsg, TF.copy_into)
    sink = TF.GradSink([arena])
    old = TF.set_grad_sink(sink)
    try:
        TF.grad_sink_reset()
        (fsg(x) * proj).sum().backward()
        TF.grad_sink_flush()
    finally:
        TF.set_grad_sink(old)
    for (k, p), off in zip(fsg.named_parameters(), arena.offsets):
        close(arena.flat[off:off + p.numel()].view(p.shape), ref[k], rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------------
# module level against the reference
@pytest.mark.parametrize('tag,cond_dim,size', [('u', 0, 64), ('c', 16, 64), ('u128', 0, 128)])
def test_gen_nolstm(golden, tag, cond_dim, size):
    if cond_dim:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    else:
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    g = golden('gen_nolstm')
    m = pour(MultiScaleGen(width=size, height=size, num_channels=1, cond_dim=cond_dim, no_lstm=True))
    m.train()
    z = T(g[tag + '_z']).to(DEV)
    cond = T(g[tag + '_cond']).to(DEV) if cond_dim else None
    torch.manual_seed(5)                                   # the reference drew its 3 phases after this seed
    fake = m(z, cond=cond)
    for i, f in enumerate(fake):
        sp = max(1, f.size(4) // 64)
        close(f[..., ::sp, ::sp], g[tag + '_fake%d' % i], rtol=2e-3, atol=5e-4)
    loss = sum((f * rnd(40 + i, *f.shape).to(DEV)).sum() for i, f in enumerate(fake))
    loss.backward()
    norms_close(m, g, tag + '_gn', rtol=3e-3)
    # the deepest gradients (through 4 blocks of training-mode BN): test_gen's bound for fc.bias
    if z.size(0) > 2:
        close(m.fc.bias.grad, g[tag + '_g_fc.bias'], rtol=3e-3, atol=1.5e-3)
    else:
        # bn0 over TWO samples: xhat = +-1, and its adjoint passes back exactly zero (up to eps); fc's gradients are rounding
        # noise on both sides (the reference's: multiples of 2^-17)
        assert float(m.fc.bias.grad.abs().max()) < 1e-2 and float(np.abs(g[tag + '_g_fc.bias']).max()) < 1e-2
    # 128x128 at B=2: dL/dz comes back through BatchNorms of the 2x2-state pyramid over two samples, and both fp32 sides
    # part by up to ~0.7% of the tensor's scale (the kernels themselves are pinned against fp64 by the op-level test above;
    # the per-parameter norms above hold at 3e-3)
    deep = 1.5e-3 if size == 64 else 1e-2
    close(m.frame_seed_gen.dc4.bias.grad, g[tag + '_g_frame_seed_gen.dc4.bias'], rtol=3e-3, atol=deep)
    close(m.frame_seed_gen.dc4.weight.grad[:, :8], g[tag + '_g_frame_seed_gen.dc4.weight'], rtol=3e-3, atol=deep)
    sd = m.state_dict()
    for k in g.keys():
        if k.startswith(tag + '_buf_'):
            name = k[len(tag + '_buf_'):]
            if name.endswith('num_batches_tracked'):
                assert int(sd[name]) == int(g[k]), name
            else:
                close(sd[name], g[k])
    m.eval()
    with torch.no_grad():
        vid = m(z[:2], cond=None if cond is None else cond[:2])
    assert len(vid) == 1 and vid[0].shape[2] == 16
    se = size // 32
    close(vid[0][:, :, ::4, ::se, ::se], g[tag + '_eval'], rtol=2e-3, atol=5e-4)


# ---------------------------------------------------------------------------------------------------------------------
# training iterations
class _Prm(object):
    frame_sizes = [8, 16, 32, 64]
    subsample_input = True
    discrim_steps = gen_steps = 1
    gp_lambda = 0.5
    no_mean_discrim_loss = no_mean_gen_loss = True


def _make(cond=False, V=21):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    txt = None
    if cond:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
        from txt2vid_amd.models.txt.basic import Seq2Seq
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, no_lstm=True))
        dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256))
        txt = Seq2Seq(vocab_size=V)
        sd = txt.state_dict()
        txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                             for k, v in sd.items()})
        txt.to(DEV)
    else:
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, no_lstm=True))
        dis = pour(MultiScaleDiscrim(num_channels=1))
    gen.train()
    dis.train()
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    return gan, optD, optG, losses, _Prm()


def test_train_steps_nolstm_vs_reference_golden(golden):
    """Three free-running G+D iterations against the REAL reference's losses (tests/golden/steps_nolstm.npz); bounds as in
    test_train_steps_uncond_vs_reference_golden (1e-3 on iterations 0-1, 2e-2 on iteration 2: the GAN dynamics are chaotic)."""
    from txt2vid_amd.gan.trainer import train_iteration
    g = golden('steps_nolstm')
    gan, optD, optG, losses, prm = _make()
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    for it in range(3):
        x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
        lD, lG, _, _ = train_iteration(gan, x, None, optD, optG, losses, prm, DEV)
        if it == 0:
            norms_close(gan.gen, g, 'it0_G_gn', rtol=3e-3)
        tol = 1e-3 if it < 2 else 2e-2
        print('no_lstm it %d: lossD %.7f (ref %.7f)  lossG %.7f (ref %.7f)' % (it, float(lD), g['lossD'][it], float(lG), g['lossG'][it]))
        assert abs(float(lD) - g['lossD'][it]) < tol, (it, float(lD), g['lossD'][it])
        assert abs(float(lG) - g['lossG'][it]) < tol, (it, float(lG), g['lossG'][it])


@pytest.mark.parametrize('cond', [False, True], ids=['uncond', 'cond'])
def test_graph_replay_matches_eager_nolstm(golden, cond):
    """GraphedTrainStep (capture after 2 eager iterations, then replays) reproduces the eager iteration with the no_lstm
    generator; tolerances as test_graph_replay_matches_eager(_cond)."""
    from txt2vid_amd.gan.trainer import train_iteration, GraphedTrainStep
    tokens = T(golden('steps_cond')['tokens']).to(DEV) if cond else None

    def batches():
        g = torch.Generator()
        g.manual_seed(11)
        return [(torch.rand(4, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]

    def seed():
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(5)

    def code(gan):
        return gan.cond_encoder.encode(tokens, [8] * 4)[2].detach() if cond else None
    gan, optD, optG, losses, prm = _make(cond)
    train_iteration(gan, batches()[0], code(gan), optD, optG, losses, prm, DEV)          # burn-in (see the ConvLSTM test)
    gan, optD, optG, losses, prm = _make(cond)
    seed()
    eager = []
    for x in batches():
        lD, lG, _, _ = train_iteration(gan, x, code(gan), optD, optG, losses, prm, DEV)
        eager.append((float(lD), float(lG)))
    gan, optD, optG, losses, prm = _make(cond)
    seed()
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2, cond_dim=256 if cond else 0)
    for i, x in enumerate(batches()):
        lD, lG = gs.step(x, code(gan)) if cond else gs.step(x)
        got = (float(lD), float(lG))
        print('step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = (2e-5 if i < 2 else 2e-3) if cond else (5e-6 if i < 2 else 5e-4)
        assert abs(got[0] - eager[i][0]) < tol and abs(got[1] - eager[i][1]) < tol, (i, got, eager[i])
    assert gs.graphs is not None
    assert int(gan.gen.frame_seed_gen.bn0.num_batches_tracked) == 4


# ---------------------------------------------------------------------------------------------------------------------
def test_cli_nolstm_train_checkpoint_resume_and_sample(tmp_path):
    """`--G tools/cfg/gen_nolstm.json` through the reference's command line: 2 iterations, a checkpoint, a resume from it and
    `--test` sampling."""
    import json
    cfg = str(tmp_path / 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    base = ['--data', cfg, '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
            '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
            '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', os.path.join(ROOT, 'tools', 'cfg', 'gen_nolstm.json'), '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--epochs', '1', '--out', out_dir, '--out_samples', smp]

    def run(args):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert p.returncode == 0, out[-3000:]
        return out
    log = run(base + ['--max_iters', '2', '--save_model_period', '2', '--save_example_period', '0'])
    assert 'Iter 2, Loss_D' in log
    ck = glob.glob(os.path.join(out_dir, 'iter_2_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)['gen']
    assert 'frame_seed_gen.dc0.weight' in sd and not any(k.startswith('clstm.') for k in sd)
    log2 = run(base + ['--max_iters', '2', '--weights', ck[0], '--save_model_period', '1000', '--save_example_period', '0'])
    assert 'Iter 2, Loss_D' in log2
    smp2 = str(tmp_path / 'samples_test')
    run(base[:-2] + ['--out_samples', smp2, '--test', '--weights', ck[0], '--num_samples', '1', '--max_iters', '1'])
    assert os.path.exists(os.path.join(smp2, 'real_0.png')) and os.path.exists(os.path.join(smp2, '64x64_0_0.jpg'))
