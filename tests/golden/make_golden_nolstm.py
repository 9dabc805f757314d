"""Golden vectors of MultiScaleGen(no_lstm=True) — the TGAN-v1 frame-seed generator in place of the ConvLSTM
(txt2vid/models/tganv2/gen.py:40-43,66-75, tganv2_cond/gen.py:41-44,71-80, tgan/temporal_gen.py:10-34) — recorded by running
the REAL reference, from the repository root with a checkout of the reference first on the module path:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nolstm.py

Same two runtime shims (plus an empty stand-in for an unused import), weight recipe and conventions as make_golden.py (imported from it, not restated).
"""
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

# temporal_gen.py:2 imports torchvision and never uses it; this build environment has none, so an empty module stands in
# (no torchvision code is emulated)
sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import (HERE, GenU, GenC, DisU, CondGan, MixedGanLoss, RSGANLoss, Subsample, ref_init,   # noqa: E402
                         pour, rnd, npy, grad_norms, save, pack_norms)


def _gen_case(out, tag, cls, cond_dim, B, size):
    g = pour(cls(width=size, height=size, num_channels=1, cond_dim=cond_dim, no_lstm=True))
    g.train()
    z = rnd(30, B, 256)
    cond = rnd(31, B, cond_dim) if cond_dim else None
    torch.manual_seed(5)
    bts = [int(torch.randint(2, (1,))) for _ in range(3)]
    torch.manual_seed(5)
    fake = g(z, cond=cond)
    loss = sum((f * rnd(40 + i, *f.shape)).sum() for i, f in enumerate(fake))
    loss.backward()
    out[tag + '_z'] = npy(z)
    if cond is not None:
        out[tag + '_cond'] = npy(cond)
    out[tag + '_bts'] = np.array(bts)
    # (fixture size: frames wider than 64 pixels keep every 2nd row / column; the eval video every 4th frame and rows /
    # columns at a stride of size / 32; the dc4 weight gradient its first 8 output channels. The tests slice alike.)
    for i, f in enumerate(fake):
        sp = max(1, f.size(4) // 64)
        out[tag + '_fake%d' % i] = npy(f[..., ::sp, ::sp])
    pack_norms(tag + '_gn', grad_norms(g), out)
    out[tag + '_g_fc.bias'] = npy(g.fc.bias.grad)
    out[tag + '_g_frame_seed_gen.dc4.bias'] = npy(g.frame_seed_gen.dc4.bias.grad)
    out[tag + '_g_frame_seed_gen.dc4.weight'] = npy(g.frame_seed_gen.dc4.weight.grad)[:, :8]
    for k, v in g.state_dict().items():
        if k.startswith('frame_seed_gen.bn') and (k.endswith('running_mean') or k.endswith('running_var')
                                                   or k.endswith('num_batches_tracked')):
            out[tag + '_buf_' + k] = npy(v)
    g.eval()
    with torch.no_grad():
        vid = g(z[:2], cond=None if cond is None else cond[:2])
    assert len(vid) == 1
    se = size // 32
    out[tag + '_eval'] = npy(vid[0][:, :, ::4, ::se, ::se])


def golden_gen_nolstm():
    """Train-mode pyramid, gradients of a fixed random projection, BN buffers, eval-mode video: unconditional and
    text-conditioned (cond_dim 16) at 64x64, B=4; unconditional at 128x128 (2x2 state, fm_size 4096), B=2."""
    out = {}
    _gen_case(out, 'u', GenU, 0, 4, 64)
    _gen_case(out, 'c', GenC, 16, 4, 64)
    _gen_case(out, 'u128', GenU, 0, 2, 128)
    save('gen_nolstm', **out)


def golden_steps_nolstm():
    """Losses of 3 free-running unconditional iterations; otherwise make_golden.golden_steps."""
    out = {}
    B = 4
    g = pour(GenU(width=64, height=64, num_channels=1, no_lstm=True))
    d = pour(DisU(num_channels=1))
    seed = 100
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    g.train()
    d.train()
    gan = CondGan(gen=g, discrims=[d], discrim_names=['video'])
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = torch.optim.Adam([{'params': d.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = torch.optim.Adam([{'params': g.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    ss = Subsample()
    fs = [8, 16, 32, 64]
    lD_all, lG_all = [], []
    for it in range(3):
        x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4)
        xs = []
        for i in range(4):
            xs.append(F.interpolate(x, size=(x.size(2), fs[i], fs[i])) if i != 3 else x)
            x, _ = ss(x)
        z = torch.randn(B, g.latent_size)
        fake = gan(z, cond=None)
        lD = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=None, loss=losses.discrim_loss, gp_lambda=0.5)
        lD.backward()
        optD.step()
        _, _, real_pred = gan.all_discrim_forward(real=xs, cond=None, fake=None, loss=None)
        g.zero_grad()
        fc = d(x=fake, cond=None, xbar=None)
        lG = torch.stack([losses.gen_loss(fake=ff[0], real=rr) for ff, rr in zip(fc, real_pred[0])]).mean()
        lG.backward()
        if it == 0:
            pack_norms('it0_G_gn', grad_norms(g), out)
        optG.step()
        lD_all.append(float(lD))
        lG_all.append(float(lG))
        print('no_lstm it', it, float(lD), float(lG))
    out['lossD'] = np.array(lD_all, dtype=np.float64)
    out['lossG'] = np.array(lG_all, dtype=np.float64)
    save('steps_nolstm', **out)


def golden_init_nolstm():
    """`init(gen, 'xavier')` after seeding 100 and constructing the no_lstm generator: the frame_seed_gen.* entries (sums,
    absolute sums and the first 64 values of each)."""
    out = {}
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    g = GenU(width=64, height=64, num_channels=1, no_lstm=True)
    ref_init(g, 'xavier')
    sd = g.state_dict()
    keys = sorted(k for k, v in sd.items() if k.startswith('frame_seed_gen.') and v.dtype.is_floating_point)
    out['keys'] = np.array(keys)
    out['sum'] = np.array([float(sd[k].double().sum()) for k in keys])
    out['abs'] = np.array([float(sd[k].double().abs().sum()) for k in keys])
    out['head'] = np.stack([sd[k].reshape(-1)[:64].numpy() for k in keys])
    save('init_nolstm', **out)


def golden_checkpoint_nolstm():
    """`{'optG', 'optD'}` + the reference's `CondGan.save_dict()` for the unconditional no_lstm model after one optimiser step
    each, tensor values compacted as in make_golden.golden_checkpoint (what is pinned is the file format)."""
    from make_golden import _compact
    g = pour(GenU(width=64, height=64, num_channels=1, no_lstm=True))
    d = pour(DisU(num_channels=1))
    gan = CondGan(gen=g, discrims=[d], discrim_names=['video'])
    optD = torch.optim.Adam([{'params': d.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = torch.optim.Adam([{'params': g.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    for m, opt in ((g, optG), (d, optD)):
        for i, p in enumerate(m.parameters()):
            p.grad = torch.full_like(p, 1e-3 * (1 + i % 7))
        opt.step()
    to_save = {'optG': optG.state_dict(), 'optD': optD.state_dict()}
    to_save.update(gan.save_dict())
    path = os.path.join(HERE, 'ref_checkpoint_nolstm.pt')
    torch.save(_compact(to_save), path)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    which = sys.argv[1:] or ['gen', 'steps', 'init', 'checkpoint']
    if 'gen' in which:
        golden_gen_nolstm()
    if 'init' in which:
        golden_init_nolstm()
    if 'steps' in which:
        golden_steps_nolstm()
    if 'checkpoint' in which:
        golden_checkpoint_nolstm()
