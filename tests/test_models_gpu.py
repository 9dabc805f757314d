"""GPU parity of the HIP-backed modules (txt2vid_amd.models / .gan) against
  (a) the golden vectors recorded from the REAL reference (tests/golden/*.npz), and
  (b) the CPU oracle on the same seeded inputs.
Tolerances (fp32 everywhere): outputs rtol 1e-3 / atol 1e-4 relative to the tensor's scale; per-key
gradient norms 2e-3; losses of the 3 free-running training steps 1e-3 (BASELINE.json north_star)."""
import random

import numpy as np
import pytest
import torch

from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rtol=1e-3, atol=1e-4):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale)


def pour(module, prefix='', **kw):
    sd = module.state_dict()
    module.load_state_dict({k: O.recipe_tensor(prefix + k, v.shape, **kw) for k, v in sd.items()})
    return module.to(DEV)


def rnd(seed, *shape):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def norms_close(module, g, prefix, rtol=2e-3):
    """Per-parameter gradient norms. A parameter a sweep never reaches has grad None on one side and an
    all-zero grad on the other (both recorded as 0). Biases that feed a training-mode BatchNorm have an
    exactly-zero true gradient, so their recorded norms (~1e-4 against a median of ~1e2) are pure
    rounding noise: an absolute floor of 1e-7 * max-norm absorbs them."""
    got = {k: (float(p.grad.norm()) if p.grad is not None else 0.0) for k, p in module.named_parameters()}
    vals = [max(float(v), 0.0) for v in g[prefix + '_vals']]
    floor = 1e-7 * max(vals) + 1e-6
    for k, v in zip([str(k) for k in g[prefix + '_keys']], vals):
        assert abs(got[k] - v) <= rtol * abs(v) + floor, (k, got[k], v)


def test_downsample_subsample(golden):
    from txt2vid_amd.models.layers import DownSample, Subsample
    g = golden('layers')
    for tag in 'abc':
        close(DownSample()(T(g['ds_%s_x' % tag]).to(DEV)), g['ds_%s_y' % tag])
    x = T(g['ss_x']).to(DEV)
    close(Subsample()(x, bt=0)[0], g['ss_y0'])
    close(Subsample()(x, bt=1)[0], g['ss_y1'])


def test_down_block(golden):
    from txt2vid_amd.models.layers import DownBlock
    g = golden('layers')
    m = pour(DownBlock(in_channels=16, out_channels=32, wide=False))
    x = T(g['db_x']).to(DEV).requires_grad_(True)
    y = m(x)
    close(y, g['db_y'])
    (y * T(g['db_gy']).to(DEV)).sum().backward()
    close(x.grad, g['db_gx'])
    for k, p in m.named_parameters():
        close(p.grad, g['db_g_' + k])


def test_attention3d_double_backward(golden):
    from txt2vid_amd.models.layers import Attention3d
    g = golden('layers')
    m = pour(Attention3d(32))
    x = T(g['at3_x']).to(DEV).requires_grad_(True)
    y = m(x)
    close(y, g['at3_y'])
    gx, = torch.autograd.grad((y * T(g['at3_gy']).to(DEV)).sum(), x, create_graph=True)
    close(gx, g['at3_gx'])
    r = (gx ** 2).sum()
    r.backward()
    close(r, g['at3_r'])
    close(x.grad, g['at3_ggx'])
    for k, p in m.named_parameters():
        close(p.grad, g['at3_gg_' + k], rtol=2e-3, atol=2e-4)


def test_attention2d(golden):
    from txt2vid_amd.models.layers import Attention
    g = golden('layers')
    m = pour(Attention(32))
    x = T(g['at2_x']).to(DEV).requires_grad_(True)
    y = m(x)
    close(y, g['at2_y'])
    (y * T(g['at2_gy']).to(DEV)).sum().backward()
    close(x.grad, g['at2_gx'])
    for k, p in m.named_parameters():
        close(p.grad, g['at2_g_' + k])


# ---- stand-alone blocks run as groups of one: each against the plain fp32 PyTorch restatement (the oracle) on the CPU ----------

def _seeded(module, seed, gamma=None):
    """(module on the device, its parameters as CPU leaves for the oracle): torch's default initialisation under `seed`."""
    torch.manual_seed(seed)
    m = module()
    if gamma is not None:
        with torch.no_grad():
            m.gamma.fill_(gamma)                                  # (initialised to 0: the block would be the identity)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    return m.to(DEV), P


def _grads_close(m, P, rtol, atol):
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, P[k].grad, rtol=rtol, atol=atol)


def _attention_first_order(cls, ref, shape, x_grad, fused=None):
    m, P = _seeded(lambda: cls(16), 31, gamma=0.7)                # ch // 8 = 2, ch // 2 = 8: heads narrower than any tile
    if fused is not None:
        m.fused_attend = fused
    x0, gy = rnd(32, *shape), rnd(33, *shape)
    x, xr = x0.to(DEV).requires_grad_(x_grad), x0.clone().requires_grad_(x_grad)
    y, yr = m(x), ref(P, '', xr)
    # bounds of the non-local op tests (test_ops_gpu.test_maxpool_softmax_bmm_double_backward / test_scale_add_rowsum_...)
    close(y, yr, rtol=1e-4, atol=1e-4)
    (y * gy.to(DEV)).sum().backward()
    (yr * gy).sum().backward()
    if x_grad:
        close(x.grad, xr.grad, rtol=1e-3, atol=1e-3)
    _grads_close(m, P, rtol=1e-3, atol=1e-3)


def test_attention3d_alone_is_a_group_of_one():
    """`Attention3d(16)(x)` = `nonlocal_levels(att, [x])[0]`: output, dL/dx and the five parameter gradients."""
    from txt2vid_amd.models.layers import Attention3d
    _attention_first_order(Attention3d, O.nonlocal3d, (2, 16, 2, 4, 4), True)


def test_attention3d_alone_through_the_gradient_penalty():
    """The recorded adjoints of the grouped soft-max / batched GEMM / gamma * o + x (`SoftmaxG`, `BmmG`, `ScaleAddG`) on a group of
    one: second-order gradients of x and of the five parameters, bounds of the recorded-backward convolution tests."""
    from txt2vid_amd.models.layers import Attention3d
    m, P = _seeded(lambda: Attention3d(16), 31, gamma=0.7)
    x0 = rnd(32, 2, 16, 2, 4, 4)
    x, xr = x0.to(DEV).requires_grad_(True), x0.clone().requires_grad_(True)
    for out, leaf in ((m(x), x), (O.nonlocal3d(P, '', xr), xr)):
        gx, = torch.autograd.grad(out.sum(), leaf, create_graph=True)
        (gx ** 2).sum().backward()
    close(x.grad, xr.grad, rtol=2e-4, atol=2e-4)
    _grads_close(m, P, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize('x_grad', [True, False])
def test_attention2d_unfused_runs_the_grouped_ops(x_grad):
    """The 2-D block with the fused attention kernel switched off: the `[b, C, 1, H, W]` view through the grouped ops, with an
    input that takes part in the backward (forked: projections + residual) and one that does not."""
    from txt2vid_amd.models.layers import Attention
    _attention_first_order(Attention, O.nonlocal2d, (2, 16, 4, 4), x_grad, fused=False)


@pytest.mark.parametrize('shape', [(2, 8, 2, 4, 4), (1, 8, 3, 5, 5)])             # the second: odd extents, padded pooling
def test_down_block_alone_is_a_group_of_one(shape):
    """`DownBlock(8, 16)(x)` is `down_block_levels(block, [x])[0]` bit for bit, and the block of the oracle (output, dL/dx, parameter
    gradients; bounds of the fp32 convolution cases)."""
    from txt2vid_amd.models.layers import DownBlock, down_block_levels
    m, P = _seeded(lambda: DownBlock(8, 16), 41)
    x0 = rnd(42, *shape)
    x, xr = x0.to(DEV).requires_grad_(True), x0.clone().requires_grad_(True)
    y, yr = m(x), O.down_block(P, '', xr)
    assert torch.equal(y, down_block_levels(m, [x])[0])
    close(y, yr, rtol=2e-4, atol=2e-4)
    gy = rnd(43, *yr.shape)
    (y * gy.to(DEV)).sum().backward()
    (yr * gy).sum().backward()
    close(x.grad, xr.grad, rtol=2e-4, atol=2e-4)
    _grads_close(m, P, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize('base', ['layers', 'nn'])
def test_resnet3d_with_a_subclassed_pool(base):
    """A one-block trunk whose `which_pool` is a trivial subclass: `(uncond, None, features)` and the input gradient against the
    oracle, bounds of `test_resnet3d_and_gp`. A subclass of this package's `AvgPool3d` passes `forward_levels`' isinstance checks
    (the fused stem); one of `torch.nn.AvgPool3d` is a foreign layer there and takes the plain arm, module by module."""
    from txt2vid_amd.models import layers
    from txt2vid_amd.models.resnet3d import Resnet3D

    class Pool(layers.AvgPool3d if base == 'layers' else torch.nn.AvgPool3d):
        pass
    net, P = _seeded(lambda: Resnet3D(num_channels=1, num_down_blocks=1, with_attn=False, which_pool=Pool), 51)
    x0 = rnd(52, 2, 1, 2, 8, 8)
    x, xr = x0.to(DEV).requires_grad_(True), x0.clone().requires_grad_(True)
    (u, c, feat), (ur, cr, featr) = net(x), O.resnet3d(P, xr, num_down_blocks=1, with_attn=False)
    assert c is None and cr is None
    close(u, ur)
    close(feat, featr)
    for a, b in ((u, feat), (ur, featr)):
        ((a * rnd(22, 2, 1).to(a.device)).sum() + (b * rnd(23, 2, 128).to(a.device)).sum() * 1e-2).backward()
    close(x.grad, xr.grad)


@pytest.mark.parametrize('tag,cin,cout', [('ub', 16, 8), ('ub_same', 8, 8)])
def test_up_block(golden, tag, cin, cout):
    from txt2vid_amd.models.layers import UpBlock
    g = golden('layers')
    m = pour(UpBlock(in_channels=cin, out_channels=cout))
    m.train()
    x = T(g[tag + '_x']).to(DEV).requires_grad_(True)
    y = m(x)
    close(y, g[tag + '_y'])
    (y * T(g[tag + '_gy']).to(DEV)).sum().backward()
    close(x.grad, g[tag + '_gx'])
    for k, p in m.named_parameters():
        close(p.grad, g[tag + '_g_' + k], rtol=2e-3, atol=2e-4)
    for k, v in m.state_dict().items():
        if 'running' in k:
            close(v, g[tag + '_buf_' + k])


def test_render_block(golden):
    from txt2vid_amd.models.layers import RenderBlock
    g = golden('layers')
    m = pour(RenderBlock(in_channels=8, out_channels=3))
    m.train()
    x = T(g['rb_x']).to(DEV).requires_grad_(True)
    y = m(x)
    close(y, g['rb_y'])
    (y * T(g['rb_gy']).to(DEV)).sum().backward()
    close(x.grad, g['rb_gx'])
    for k, p in m.named_parameters():
        close(p.grad, g['rb_g_' + k])


@pytest.mark.parametrize('tag,hw', [('cl1', 1), ('cl2', 2)])
def test_conv_lstm(golden, tag, hw):
    from txt2vid_amd.models.conv_lstm import ConvLSTM
    g = golden('layers')
    m = pour(ConvLSTM(input_channels=8, hidden_channels=[8], kernel_size=3, step=5, effective_step=range(5)), prefix='clstm.')
    x = T(g[tag + '_x']).to(DEV).requires_grad_(True)
    ys, _ = m(x)
    y = torch.stack(ys)
    close(y, g[tag + '_y'])
    (y * T(g[tag + '_gy']).to(DEV)).sum().backward()
    close(x.grad, g[tag + '_gx'])
    for k, p in m.named_parameters():
        close(p.grad, g[tag + '_g_' + k])


@pytest.mark.parametrize('tag,cond_dim', [('u', 0), ('c', 24)])
def test_resnet3d_and_gp(golden, tag, cond_dim):
    from txt2vid_amd.models.resnet3d import Resnet3D
    from txt2vid_amd.gan.losses import _gradient_penalty
    g = golden('resnet3d')
    net = pour(Resnet3D(num_channels=1, cond_dim=cond_dim))
    x = T(g[tag + '_x']).to(DEV).requires_grad_(True)
    cond = T(g[tag + '_cond']).to(DEV) if cond_dim else None
    u, c, feat = net(x, cond=cond)
    close(u, g[tag + '_u'])
    close(feat, g[tag + '_feat'])
    loss = (u * rnd(22, 2, 1).to(DEV)).sum() + (feat * rnd(23, 2, 1024).to(DEV)).sum() * 1e-2
    if c is not None:
        close(c, g[tag + '_c'])
        loss = loss + (c * rnd(24, 2, 1).to(DEV)).sum()
    loss.backward()
    close(x.grad, g[tag + '_gx'])
    norms_close(net, g, tag + '_gn')
    close(net.fc_uncond.weight.grad, g[tag + '_g_fc_uncond.weight'])
    close(net.res_block.inner_module[0].weight.grad, g[tag + '_g_res_block.inner_module.0.weight'], rtol=2e-3, atol=2e-4)
    net.zero_grad()
    torch.manual_seed(77)
    alpha = torch.rand(2, 1, 1, 1, 1)
    gp = _gradient_penalty(net, real_x=T(g[tag + '_gp_xr']).to(DEV), fake_x=T(g[tag + '_gp_xf']).to(DEV),
                           real_cond=T(g[tag + '_gp_cr']).to(DEV) if cond_dim else None,
                           fake_cond=T(g[tag + '_gp_cf']).to(DEV) if cond_dim else None,
                           zero_center=True, combine=torch.sum, alpha=alpha)
    close(gp, g[tag + '_gp'])
    gp.backward()
    norms_close(net, g, tag + '_gp_gn', rtol=3e-3)
    close(net.down[1].gamma.grad, g[tag + '_gp_g_down.1.gamma'], rtol=3e-3, atol=3e-4)
    close(net.down[1].theta.weight.grad, g[tag + '_gp_g_down.1.theta.weight'], rtol=3e-3, atol=3e-4)
    close(net.res_block.inner_module[0].weight.grad, g[tag + '_gp_g_res_block.inner_module.0.weight'], rtol=3e-3, atol=3e-4)
    close(net.fc_uncond.weight.grad, g[tag + '_gp_g_fc_uncond.weight'], rtol=3e-3, atol=3e-4)


def test_gp_world_scale_applies_to_the_sum_combined_form_only(golden):
    """Data parallelism scales the local gradient penalty by world_size so that gradient AVERAGING reproduces the global batch
    SUM of the multi-scale form (losses.py:203); the single-discriminator form is a batch MEAN (losses.py:185,209), whose
    rank average already is the global mean: there the scale must not apply."""
    from txt2vid_amd.models.resnet3d import Resnet3D
    from txt2vid_amd.gan.losses import _gradient_penalty
    g = golden('resnet3d')
    net = pour(Resnet3D(num_channels=1, cond_dim=0))
    xr, xf = T(g['u_gp_xr']).to(DEV), T(g['u_gp_xf']).to(DEV)
    alpha = torch.rand(2, 1, 1, 1, 1)
    vals = {}
    for combine, zc in ((torch.sum, True), (torch.mean, False)):
        for scale in (1.0, 4.0):
            vals[(combine, scale)] = float(_gradient_penalty(net, real_x=xr, fake_x=xf, zero_center=zc, combine=combine,
                                                             alpha=alpha, scale=scale))
    assert abs(vals[(torch.sum, 4.0)] - 4.0 * vals[(torch.sum, 1.0)]) < 1e-4 * abs(vals[(torch.sum, 4.0)])
    assert vals[(torch.mean, 4.0)] == vals[(torch.mean, 1.0)]


@pytest.mark.parametrize('tag,cond_dim', [('u', 0), ('c', 16)])
def test_gen(golden, tag, cond_dim):
    if tag == 'u':
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    else:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    g = golden('gen')
    m = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=cond_dim))
    m.train()
    z = T(g[tag + '_z']).to(DEV)
    cond = T(g[tag + '_cond']).to(DEV) if cond_dim else None
    torch.manual_seed(5)                                   # the reference drew its 3 phases after this seed
    fake = m(z, cond=cond)
    for i, f in enumerate(fake):
        close(f, g[tag + '_fake%d' % i], rtol=2e-3, atol=5e-4)
    loss = sum((f * rnd(40 + i, *f.shape).to(DEV)).sum() for i, f in enumerate(fake))
    loss.backward()
    norms_close(m, g, tag + '_gn', rtol=3e-3)
    # the deepest gradient of the generator (through 4 blocks of training-mode BN + 16 LSTM steps):
    # summation-order noise reaches ~7e-4 of the tensor's scale
    close(m.fc.bias.grad, g[tag + '_g_fc.bias'], rtol=3e-3, atol=1.5e-3)
    close(m.render_blocks[3].conv.weight.grad, g[tag + '_g_render_blocks.3.conv.weight'], rtol=3e-3, atol=3e-4)
    sd = m.state_dict()
    for k in g.keys():
        if k.startswith(tag + '_buf_'):
            close(sd[k[len(tag + '_buf_'):]], g[k])
    m.eval()
    with torch.no_grad():
        vid = m(z[:2], cond=None if cond is None else cond[:2])
    assert len(vid) == 1
    close(vid[0], g[tag + '_eval'], rtol=2e-3, atol=5e-4)


def _make_uncond(B=4):
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1))
    dis = pour(MultiScaleDiscrim(num_channels=1))
    gen.train()
    dis.train()
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'])
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))

    class Prm(object):
        frame_sizes = [8, 16, 32, 64]
        subsample_input = True
        discrim_steps = gen_steps = 1
        gp_lambda = 0.5
        no_mean_discrim_loss = no_mean_gen_loss = True
    return gan, optD, optG, losses, Prm()


def test_train_steps_uncond_vs_reference_golden(golden):
    """Three free-running G+D iterations (RSGAN + GP 0.5, Adam) against the losses the REAL reference
    produced (tests/golden/steps_uncond.npz), same seeds and recipe weights. GAN + Adam dynamics are
    chaotic (the reference's own fp32 and fp64 runs part by > 1e-3 after 3 steps), so the
    1e-3 bound of the north star is asserted on iterations 0-1 and 2e-2 on iteration 2; the pointwise
    per-step bound is asserted teacher-forced in `test_teacher_forced_steps_vs_oracle`."""
    from txt2vid_amd.gan.trainer import train_iteration
    g = golden('steps_uncond')
    gan, optD, optG, losses, prm = _make_uncond()
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    for it in range(3):
        x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
        lD, lG, _, _ = train_iteration(gan, x, None, optD, optG, losses, prm, DEV)
        tol = 1e-3 if it < 2 else 2e-2
        print('free-running it %d: lossD %.7f (ref %.7f)  lossG %.7f (ref %.7f)' % (it, float(lD), g['lossD'][it], float(lG), g['lossG'][it]))
        assert abs(float(lD) - g['lossD'][it]) < tol, (it, float(lD), g['lossD'][it])
        assert abs(float(lG) - g['lossG'][it]) < tol, (it, float(lG), g['lossG'][it])


def _sync_from_oracle(tr, gan, optD, optG):
    """product <- oracle: parameters, buffers and Adam state (teacher forcing)."""
    gen, dis = gan.gen, gan.discrims[0]
    gen.load_state_dict({k: v.detach().clone() for k, v in tr.PG.items()})
    dis.load_state_dict({k: v.detach().clone() for k, v in tr.PD.items()})
    for mod, P, keys, opt_o, opt_p in ((gen, tr.PG, tr.g_params, tr.optG, optG), (dis, tr.PD, tr.d_params, tr.optD, optD)):
        named = dict(mod.named_parameters())
        for k in keys:
            so = opt_o.state.get(P[k], {})
            if not so:
                continue
            pp = named[k]
            sp = opt_p.state[pp]
            sp['step'] = int(so['step'])
            for key in ('exp_avg', 'exp_avg_sq'):                     # in the PARAMETER's memory layout (tap-major ConvLSTM masters):
                sp[key] = torch.empty_strided(pp.shape, pp.stride(), dtype=pp.dtype, device=pp.device).copy_(so[key].detach())   # the fused
                #                                                        optimiser walks parameter, gradient and moments with one flat index
    from txt2vid_amd import functional as TF
    TF.bump_weight_epoch()


def test_teacher_forced_steps_vs_oracle():
    """North-star parity protocol: at every step the HIP model is loaded with the oracle's state
    (weights, BN buffers, Adam moments), both consume the identical batch / z / subsample phases / GP
    alphas, and the single-step lossD / lossG must agree to 2e-4 (fp32 summation-order noise; the
    bound BASELINE.json asks for is 1e-3). The oracle is pinned to the real reference by
    tests/test_oracle_golden.py."""
    from txt2vid_amd.gan.trainer import train_iteration
    gan, optD, optG, losses, prm = _make_uncond()
    PG = O.recipe_state(O.gen_shapes(num_channels=1))
    PD = O.recipe_state(O.resnet3d_shapes('single_discrim.', 1, 64, 0))
    tr = O.OracleTrainer(PG, PD)
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    for it in range(4):          # (from the second step on Adam moments and BN buffers come from the step before; 100 steps: tools/parity_steps.py)
        x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
        _sync_from_oracle(tr, gan, optD, optG)
        st_t, st_n, st_r = torch.get_rng_state(), np.random.get_state(), random.getstate()
        lD, lG, _, _ = train_iteration(gan, x.to(DEV), None, optD, optG, losses, prm, DEV)
        torch.set_rng_state(st_t)
        np.random.set_state(st_n)
        random.setstate(st_r)
        before = {k: PD[k].detach().clone() for k in ('single_discrim.fc_uncond.weight', 'single_discrim.res_block.inner_module.2.weight')}
        before_g = {k: PG[k].detach().clone() for k in ('fc.weight', 'render_blocks.3.conv.weight')}
        lDo, lGo = tr.step(x)
        print('teacher-forced it %d: lossD %.7f vs %.7f   lossG %.7f vs %.7f' % (it, float(lD), lDo, float(lG), lGo))
        assert abs(float(lD) - lDo) < 2e-4, (it, float(lD), lDo)
        assert abs(float(lG) - lGo) < 2e-4, (it, float(lG), lGo)
        # post-step weights: Adam's early updates are ~lr*sign(g); compare the applied deltas
        for P, bef, mod in ((PD, before, gan.discrims[0]), (PG, before_g, gan.gen)):
            sd = mod.state_dict()
            for k, b in bef.items():
                d_o = (P[k].detach() - b)
                d_p = (sd[k].detach().cpu() - b)
                rel = float((d_p - d_o).abs().mean() / d_o.abs().mean().clamp_min(1e-12))
                assert rel < 0.05, (it, k, rel)


def test_first_step_grad_norms_vs_reference_golden(golden):
    """Per-parameter gradient norms of iteration 0 (D step incl. GP double backward; G step)."""
    from txt2vid_amd.gan.trainer import multiscale_data
    g = golden('steps_uncond')
    gan, optD, optG, losses, prm = _make_uncond()
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    xs, _ = multiscale_data(x, None, prm.frame_sizes, True)
    z = torch.randn(4, 256).to(DEV)
    fake = gan(z, cond=None)
    lD = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=None, loss=losses.discrim_loss, gp_lambda=0.5)
    lD.backward()
    norms_close(gan.discrims[0], g, 'it0_D_gn', rtol=3e-3)
    optD.step()
    with torch.no_grad():
        _, _, real_pred = gan.all_discrim_forward(real=xs, cond=None, fake=None, loss=None)
    lG = gan.gen_step(fake=fake, real_pred=real_pred, cond=None, loss=losses.gen_loss)
    lG.backward()
    norms_close(gan.gen, g, 'it0_G_gn', rtol=3e-3)


def test_graph_replay_matches_eager():
    """HIP-graph replay (3 graphs per iteration, device-resident random draws and Adam step counter) must
    reproduce the eager iteration: same seeds -> same losses on every step, captured or replayed."""
    from txt2vid_amd.gan.trainer import train_iteration, GraphedTrainStep

    def batches():
        g = torch.Generator()
        g.manual_seed(11)
        return [(torch.rand(4, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]    # 2 eager + 2 replayed

    def seed():
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(5)
    # Burn-in: the first backward in a process runs with the autograd worker thread's node numbering at
    # zero, which orders the (independent) per-level gradient accumulations differently from every later
    # run: ~1e-7 relative differences in the summed weight gradients, amplified by the GAN dynamics.
    gan, optD, optG, losses, prm = _make_uncond()
    train_iteration(gan, batches()[0], None, optD, optG, losses, prm, DEV)
    gan, optD, optG, losses, prm = _make_uncond()
    seed()
    eager = []
    for x in batches():
        lD, lG, _, _ = train_iteration(gan, x, None, optD, optG, losses, prm, DEV)
        eager.append((float(lD), float(lG)))
    gan, optD, optG, losses, prm = _make_uncond()
    seed()
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    for i, x in enumerate(batches()):
        lD, lG = gs.step(x)
        got = (float(lD), float(lG))
        print('step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        # eager iterations agree to the autograd accumulation order (~1e-6); from the capture on, the order in which autograd
        # accumulates the per-level contributions into the shared D weights is the one frozen at capture
        # time (a different but equally valid fp32 summation order): ~1e-7 relative in the gradients,
        # amplified by the dynamics to ~1e-5 in the next loss.
        tol = 5e-6 if i < 2 else 5e-4                              # the dynamics amplify ~x5-30 per iteration
        assert abs(got[0] - eager[i][0]) < tol and abs(got[1] - eager[i][1]) < tol, (i, got, eager[i])
    assert gs.graphs is not None


def test_weight_gradients_on_a_second_stream_give_the_same_iteration(monkeypatch):
    """`T2V_WGRAD_SIDE` (functional._SideLane: the deferred weight-gradient launches forked onto a second stream after the producer
    of dL/dy and joined before the sink's reduce; fork / join become graph edges under capture): the same kernels on the same
    operands, so eager iterations and the captured / replayed ones must give the losses of the single-stream iteration."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import train_iteration, GraphedTrainStep

    def batches():
        g = torch.Generator()
        g.manual_seed(11)
        return [(torch.rand(4, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]

    def run(side, graphed):
        monkeypatch.setattr(TF._side, 'enabled', side)
        gan, optD, optG, losses, prm = _make_uncond()
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(5)
        out = []
        gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2) if graphed else None
        for x in batches():
            lD, lG = gs.step(x) if graphed else train_iteration(gan, x, None, optD, optG, losses, prm, DEV)[:2]
            out.append((float(lD), float(lG)))
        torch.cuda.synchronize()
        assert not TF._side.used and not TF._side.keep            # joined, operands released
        return out
    run(False, False)                                              # burn-in (see test_graph_replay_matches_eager)
    base = run(False, False)
    for graphed in (False, True):
        got = run(True, graphed)
        for i, (g, b) in enumerate(zip(got, base)):
            tol = 5e-6 if (i < 2 or not graphed) else 5e-4
            assert abs(g[0] - b[0]) < tol and abs(g[1] - b[1]) < tol, (graphed, i, g, b)


def test_adam_step_counter_survives_a_second_capture():
    """`GraphedTrainStep` is rebuilt when the batch shape changes (trainer.py). Replays advance Adam's step counter on the device
    only; the second capture must carry on from it instead of falling back to the host-side count: after
    2 eager + 1 capture/replay + 3 replays, then a new GraphedTrainStep with 2 eager + 1 capture/replay + 1 replay, both
    optimisers have taken 10 steps."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm = _make_uncond()
    g = torch.Generator()
    g.manual_seed(3)
    xs = [(torch.rand(2, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(2)]
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (2, 1, 16, 64, 64), warmup=2)
    for i in range(6):
        gs.step(xs[i % 2])
    torch.cuda.synchronize()
    assert int(optD.step_dev[0].item()) == 6 and int(optG.step_dev[0].item()) == 6
    gs2 = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (2, 1, 16, 64, 64), warmup=2)
    for i in range(4):
        gs2.step(xs[i % 2])
    torch.cuda.synchronize()
    assert gs2.graphs is not None
    for opt in (optD, optG):
        assert int(opt.step_dev[0].item()) == 10
        steps = {int(st['step']) for st in opt.state_dict()['state'].values()}
        assert steps == {10}, steps


def _make_cond(V=21):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256))
    dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256))
    txt = Seq2Seq(vocab_size=V)
    sd = txt.state_dict()
    txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                         for k, v in sd.items()})
    txt.to(DEV)
    gen.train()
    dis.train()
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))

    class Prm(object):
        frame_sizes = [8, 16, 32, 64]
        subsample_input = True
        discrim_steps = gen_steps = 1
        gp_lambda = 0.5
        no_mean_discrim_loss = no_mean_gen_loss = True
    return gan, optD, optG, losses, Prm()


def test_graph_replay_matches_eager_cond(golden):
    """The text-conditioned iteration under HIP-graph replay (sentence codes in a fixed buffer, caption permutations among
    the device-resident draws) reproduces the eager iteration: same seeds -> same losses, captured or replayed."""
    from txt2vid_amd.gan.trainer import train_iteration, GraphedTrainStep
    tokens = T(golden('steps_cond')['tokens']).to(DEV)

    def batches():
        g = torch.Generator()
        g.manual_seed(12)
        return [(torch.rand(4, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]

    def seed():
        random.seed(6)
        np.random.seed(6)
        torch.manual_seed(6)
    gan, optD, optG, losses, prm = _make_cond()
    seed()
    eager = []
    for x in batches():
        _, _, cond = gan.cond_encoder.encode(tokens, [8] * 4)
        lD, lG, _, _ = train_iteration(gan, x, cond.detach(), optD, optG, losses, prm, DEV)
        eager.append((float(lD), float(lG)))
    gan, optD, optG, losses, prm = _make_cond()
    seed()
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2, cond_dim=256)
    for i, x in enumerate(batches()):
        _, _, cond = gan.cond_encoder.encode(tokens, [8] * 4)
        lD, lG = gs.step(x, cond)
        got = (float(lD), float(lG))
        print('cond step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert abs(got[0] - eager[i][0]) < tol and abs(got[1] - eager[i][1]) < tol, (i, got, eager[i])
    assert gs.graphs is not None


def test_train_steps_cond_vs_reference_golden(golden):
    """Text-conditioned path (Bi-LSTM cond, cat(z,cond), 2-D + 3-D non-local blocks, second D head,
    mismatched-caption loss, GP with interpolated captions): 3 free-running iterations vs the reference's
    recorded losses + iteration-0 per-parameter gradient norms."""
    from txt2vid_amd.gan.trainer import train_iteration
    g = golden('steps_cond')
    gan, optD, optG, losses, prm = _make_cond()
    tokens = T(g['tokens']).to(DEV)
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    for it in range(3):
        x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
        with torch.no_grad():
            _, _, cond = gan.cond_encoder.encode(tokens, [8] * 4)
        if it == 0:
            close(cond, g['cond0'])
        lD, lG, _, _ = train_iteration(gan, x, cond.detach(), optD, optG, losses, prm, DEV)
        tol = 1e-3 if it < 2 else 2e-2
        print('cond free-running it %d: lossD %.7f (ref %.7f)  lossG %.7f (ref %.7f)' % (it, float(lD), g['lossD'][it], float(lG), g['lossG'][it]))
        assert abs(float(lD) - g['lossD'][it]) < tol, (it, float(lD), g['lossD'][it])
        assert abs(float(lG) - g['lossG'][it]) < tol, (it, float(lG), g['lossG'][it])


def test_cond_first_step_grad_norms_vs_reference_golden(golden):
    from txt2vid_amd.gan.trainer import multiscale_data
    from txt2vid_amd import functional as TF
    g = golden('steps_cond')
    gan, optD, optG, losses, prm = _make_cond()
    tokens = T(g['tokens']).to(DEV)
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    with torch.no_grad():
        _, _, cond = gan.cond_encoder.encode(tokens, [8] * 4)
    xs, conds = multiscale_data(x, cond, prm.frame_sizes, True)
    z = torch.randn(4, 256).to(DEV)
    fake = gan(z, cond=conds[0])
    lD = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=conds, loss=losses.discrim_loss, gp_lambda=0.5)
    lD.backward()
    norms_close(gan.discrims[0], g, 'it0_D_gn', rtol=3e-3)
    optD.step()
    with torch.no_grad():
        _, _, real_pred = gan.all_discrim_forward(real=xs, cond=conds, fake=None, loss=None)
    lG = gan.gen_step(fake=fake, real_pred=real_pred, cond=conds, loss=losses.gen_loss)
    lG.backward()
    norms_close(gan.gen, g, 'it0_G_gn', rtol=3e-3)


@pytest.mark.parametrize('bi', [True, False])
def test_sentence_encoder_matches_packed_nn_lstm(bi):
    """models/txt/basic.py:49-70 on the HIP kernels vs torch's packed-sequence nn.LSTM on the CPU (same parameters):
    ragged lengths (sorted desc, incl. length 1), padded outputs, final states of every layer / direction, sentence code."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    from txt2vid_amd.models.txt.basic import RecurrentModel
    torch.manual_seed(11)
    V, B = 23, 6
    m = RecurrentModel(vocab_size=V, embed_size=48, hidden_size=64, num_layers=3, bi=bi)
    lengths = [9, 7, 7, 4, 2, 1]
    tokens = torch.zeros(B, 9, dtype=torch.long)
    for i, n in enumerate(lengths):
        tokens[i, :n] = torch.randint(1, V, (n,))
    with torch.no_grad():
        packed = pack_padded_sequence(m.embed(tokens), lengths, batch_first=True)
        ref_out, (ref_h, ref_c) = m.lstm(packed)
        ref_out, _ = pad_packed_sequence(ref_out, batch_first=True, total_length=9)
    m = m.to(DEV)
    out, (h, c), hn = m(tokens.to(DEV), lengths)
    assert out.shape == ref_out.shape and h.shape == ref_h.shape
    np.testing.assert_allclose(out.cpu().numpy(), ref_out.numpy(), rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(h.cpu().numpy(), ref_h.numpy(), rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(c.cpu().numpy(), ref_c.numpy(), rtol=1e-4, atol=2e-6)
    want = torch.cat((ref_h[-2], ref_h[-1]), 1) if bi else ref_h.view(3, 1, B, -1)[-1]      # basic.py:58-64 (keeps the 1)
    np.testing.assert_allclose(hn.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize('channels,batch,frame_sizes,size', [(3, 2, [8, 16, 32, 64], 64), (1, 3, [8, 16, 32, 64], 64), (1, 2, [16, 32, 64, 128], 128),
                                                              (1, 1, [8, 16, 32, 64], 64)])
def test_iteration_vs_oracle_other_shapes(channels, batch, frame_sizes, size):
    """One full training iteration against the CPU oracle (identical weights / batch / draws) away from the benchmark shape:
    RGB clips (the reference's default `num_channels=3`: Cin = 3 stem, Cout = 3 render convs, 3-channel stem gradient),
    an odd batch (ragged sub-sampled pyramid: 3 -> 2 -> 1 -> 1 clips), 128x128 frames (`run_tganv2.sh`'s
    `--frame_sizes 16 32 64 128`, 2x2 ConvLSTM state), and the smallest batch (one clip on every level)."""
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    gen = MultiScaleGen(width=size, height=size, num_channels=channels)
    dis = MultiScaleDiscrim(num_channels=channels)
    for m in (gen, dis):
        m.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in m.state_dict().items()})
        m.to(DEV).train()
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'])
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))

    class Prm(object):
        subsample_input = True
        discrim_steps = gen_steps = 1
        gp_lambda = 0.5
        no_mean_discrim_loss = no_mean_gen_loss = True
    Prm.frame_sizes = frame_sizes
    tr = O.OracleTrainer(O.recipe_state(O.gen_shapes(num_channels=channels, width=size, height=size)),
                         O.recipe_state(O.resnet3d_shapes('single_discrim.', channels, 64, 0)), frame_sizes=frame_sizes)
    random.seed(4)
    np.random.seed(4)
    torch.manual_seed(4)
    x = (torch.rand(batch, 16, channels, size, size) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    st = torch.get_rng_state()
    lD, lG, _, _ = train_iteration(gan, x.to(DEV), None, optD, optG, losses, Prm(), DEV)
    torch.set_rng_state(st)
    lDo, lGo = tr.step(x)
    print('C=%d B=%d %dx%d: HIP lossD %.6f lossG %.6f | oracle %.6f %.6f' % (channels, batch, size, size, float(lD), float(lG), lDo, lGo))
    assert abs(float(lD) - lDo) < 1e-3 and abs(float(lG) - lGo) < 1e-3


def test_benchmark_iteration_B32_vs_oracle(tmp_path, monkeypatch):
    """BASELINE configs[1] AS BENCHMARKED — unconditional TGANv2, 16x64x64x1, per-GPU batch 32, fp32, RSGAN + GP 0.5 — one full
    iteration against the CPU oracle on identical weights / batch / draws: both losses and the per-parameter gradient norms of
    the D step (incl. the gradient-penalty double backward) and of the G step. This is the only place besides bench.py where
    the kernels run at the size the headline is measured at (256x64 strip GEMM, 171-way split weight gradient, ...); the
    launch plans of every convolution launch of the iteration are recorded (T2V_PROF_DUMP) and each instantiation must also
    be one that the op-level cases of tests/conv_cases.py check against torch."""
    import ctypes as C
    import conv_cases as cc
    from txt2vid_amd._lib import lib
    from txt2vid_amd.gan.trainer import train_iteration
    B = 32
    gan, optD, optG, losses, prm = _make_uncond()
    tr = O.OracleTrainer(O.recipe_state(O.gen_shapes(num_channels=1)), O.recipe_state(O.resnet3d_shapes('single_discrim.', 1, 64, 0)))
    random.seed(11)
    np.random.seed(11)
    torch.manual_seed(11)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    st = torch.get_rng_state()
    dump = tmp_path / 'launches.csv'
    monkeypatch.setenv('T2V_PROF_DUMP', str(dump))
    assert lib().t2v_prof_begin(8192) == 0
    lD, lG, _, _ = train_iteration(gan, x.to(DEV), None, optD, optG, losses, prm, DEV)
    torch.cuda.synchronize()
    out = (C.c_double * 18)()
    assert lib().t2v_prof_end(out, 6) == 0                       # 0: every launch recorded (pool not exhausted)
    monkeypatch.delenv('T2V_PROF_DUMP')
    d_norms = {k: float(p.grad.norm()) for k, p in gan.discrims[0].named_parameters() if p.grad is not None}
    g_norms = {k: float(p.grad.norm()) for k, p in gan.gen.named_parameters() if p.grad is not None}
    # ---- oracle, same draws; D gradients are snapshotted before its optimiser step (the reference's G step adds the
    # discriminator's wasted weight gradients on top afterwards, cond_gan.py:157-158)
    torch.set_rng_state(st)
    d_ref = {}
    step_d = tr.optD.step

    def snap(*a, **kw):
        d_ref.update({k: float(tr.PD[k].grad.norm()) for k in tr.d_params if tr.PD[k].grad is not None})
        return step_d(*a, **kw)
    tr.optD.step = snap
    lDo, lGo = tr.step(x)
    g_ref = {k: float(tr.PG[k].grad.norm()) for k in tr.g_params if tr.PG[k].grad is not None}
    print('B=32: HIP lossD %.7f lossG %.7f | oracle %.7f %.7f' % (float(lD), float(lG), lDo, lGo))
    assert abs(float(lD) - lDo) < 2e-4 and abs(float(lG) - lGo) < 2e-4
    worst = 0.0
    for got, ref, what in ((d_norms, d_ref, 'D'), (g_norms, g_ref, 'G')):
        floor = 1e-7 * max(ref.values()) + 1e-6
        for k, v in ref.items():
            e = abs(got.get(k, 0.0) - v)
            assert e <= 3e-3 * abs(v) + floor, (what, k, got.get(k), v)
            if abs(v) > 1e-4 * max(ref.values()):                 # (biases in front of a BatchNorm have a true gradient of zero)
                worst = max(worst, e / abs(v))
    print('B=32: worst relative per-parameter gradient-norm deviation %.2e over %d + %d parameters' % (worst, len(d_ref), len(g_ref)))
    # ---- every convolution instantiation this iteration launched is one an op-level parity case covers
    pool_fwd, pool_wg = cc.all_checked_pool_variants()
    checked_fwd = set(cc.all_checked_fwd_variants()) | set(pool_fwd)
    checked_wgrad = set(cc.all_checked_wgrad_variants()) | set(pool_wg)
    kinds = {0: 'igemm', 1: 'strip', 2: 'thin', 3: 'linear', 4: 'thin2', 5: 'strip3', 9: 'pool_fwd', 10: 'pool_dgrad', 12: 'stem'}
    launched = set()
    rows = dump.read_text().strip().splitlines()[1:]
    assert len(rows) > 150
    for line in rows:
        f = line.split(',')
        kind, plan = int(f[0]), [int(v) for v in f[9].split(':')]
        if plan[0] < 0:
            continue                                              # second pass of the two-pass thin kernel: no plan of its own
        if kind in (0, 3):                                         # implicit GEMM / thin kernels (forward or data gradient)
            key = (kinds[plan[0]],) + tuple(plan[1:7])
            launched.add(key)
            assert key in checked_fwd, ('launched at B=32 but in no op-level parity case', key, line)
        elif kind == 1:
            key = ({0: 'taps', 1: 'cols', 2: 'rows3', 3: 'gemm', 4: 'thin', 11: 'pool_rows3'}[plan[0]], ('reduce', 'reduce_small')[plan[4]])
            launched.add(key)
            assert key in checked_wgrad, key
    # the stem's second convolution runs in its pooled form (box-sum + stride-2 GEMMs), the other big layers on the strip kernels
    assert ('pool_fwd', 64, 64, 16, 1, 1, 2) in launched and ('pool_dgrad', 64, 64, 32, 1, 1, 1) in launched
    assert ('pool_rows3', 'reduce_small') in launched and ('rows3', 'reduce_small') in launched
    print('B=32: %d convolution launches on %d instantiations, all covered by op-level parity cases' % (len(rows), len(launched)))


def test_benchmark_iteration_B32_bf16_launch_plans_are_covered(tmp_path, monkeypatch):
    """BASELINE configs[1] shape at per-GPU batch 32 in bf16-compute mode (what `bench.py --bf16` and the configs[2] extra record
    run), against the fp32 CPU oracle with the bf16 bound; and every convolution launch of the iteration is recorded with its launch plan, and every bf16
    instantiation — forward / data gradient incl. the frame-strided stem forms, and the bf16 weight-gradient kernels incl. the
    even-frame one — must be one that an op-level case of conv_cases.BF16_CASES checks against the convolution of the
    bf16-rounded operands; launches the bf16 entry point refuses (Cin % 32, thin outputs) must be covered fp32 instantiations."""
    import ctypes as C
    import conv_cases as cc
    from txt2vid_amd import functional as TF
    from txt2vid_amd._lib import lib
    from txt2vid_amd.gan.trainer import train_iteration
    B = 32
    gan, optD, optG, losses, prm = _make_uncond()
    tr = O.OracleTrainer(O.recipe_state(O.gen_shapes(num_channels=1)), O.recipe_state(O.resnet3d_shapes('single_discrim.', 1, 64, 0)))
    random.seed(12)
    np.random.seed(12)
    torch.manual_seed(12)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    st = torch.get_rng_state()
    dump = tmp_path / 'launches_bf16.csv'
    monkeypatch.setenv('T2V_PROF_DUMP', str(dump))
    old = TF.set_conv_precision('bf16')
    try:
        assert lib().t2v_prof_begin(8192) == 0
        lD, lG, _, _ = train_iteration(gan, x.to(DEV), None, optD, optG, losses, prm, DEV)
        torch.cuda.synchronize()
        out = (C.c_double * 18)()
        assert lib().t2v_prof_end(out, 6) == 0
    finally:
        TF.set_conv_precision(old)
        monkeypatch.delenv('T2V_PROF_DUMP')
    assert np.isfinite(float(lD)) and np.isfinite(float(lG)) and 0.3 < float(lD) < 1.5
    # the same iteration on the fp32 CPU oracle (identical weights / batch / draws): the stated bf16 bound, at the benchmark's batch
    torch.set_rng_state(st)
    lDo, lGo = tr.step(x)
    print('B=32 bf16 compute: HIP lossD %.6f lossG %.6f | fp32 oracle %.6f %.6f' % (float(lD), float(lG), lDo, lGo))
    assert abs(float(lD) - lDo) < 2e-2 and abs(float(lG) - lGo) < 5e-2
    bf_fwd, bf_wg = cc.all_checked_bf16_variants()
    checked_fwd = set(cc.all_checked_fwd_variants())
    checked_wgrad = set(cc.all_checked_wgrad_variants())
    pool_fwd, pool_wg = cc.all_checked_pool_variants()
    checked_fwd |= set(pool_fwd)
    checked_wgrad |= set(pool_wg)
    kinds = {0: 'igemm', 1: 'strip', 2: 'thin', 3: 'linear', 4: 'thin2', 5: 'strip3', 9: 'pool_fwd', 10: 'pool_dgrad', 12: 'stem'}
    launched = set()
    rows = dump.read_text().strip().splitlines()[1:]
    assert len(rows) > 150
    for line in rows:
        f = line.split(',')
        kind, plan = int(f[0]), [int(v) for v in f[9].split(':')]
        if plan[0] < 0:
            continue
        if kind == 5:                                              # bf16 forward / data-gradient GEMM
            key = ({6: 'igemm_bf16', 8: 'strip3_bf16'}[plan[0]], plan[1], plan[4])
            assert key in bf_fwd, ('bf16 launch at B=32 covered by no BF16_CASES entry', key, line)
        elif kind in (0, 3):                                       # refused by the bf16 entry point: fp32 kernels
            key = (kinds[plan[0]],) + tuple(plan[1:7])
            assert key in checked_fwd, key
        elif kind == 1:
            name = {0: 'taps', 1: 'cols', 2: 'rows3', 3: 'gemm', 4: 'thin', 11: 'pool_rows3'}[plan[0]]
            if plan[6] == 1:
                key = (name, 1, plan[7])
                assert key in bf_wg, ('bf16 weight-gradient launch covered by no BF16_CASES entry', key, line)
            else:
                key = (name, ('reduce', 'reduce_small')[plan[4]])
                assert key in checked_wgrad, key
        else:
            continue
        launched.add(key)
    # bf16-compute mode keeps the un-pooled layers (the pooled form is fp32-only and measured slower than un-pooled bf16): the stem
    # conv2's frame-strided bf16 forms did run
    assert ('strip3_bf16', 128, 1) in launched and ('rows3', 1, 1) in launched and not any(k[0].startswith('pool') for k in launched)
    print('B=32 bf16: %d convolution launches on %d instantiations, all covered' % (len(rows), len(launched)))


def test_pooled_and_unpooled_forms_agree_at_benchmark_size(monkeypatch):
    """A size-independent cross-check at BASELINE configs[1]'s full size (B=32): the SAME iteration computed with the pooled
    second convolutions / the up-sampling form (box-sum + stride-2 GEMMs, functional_pool.py) and with the un-pooled layers
    (convolution, then pooling; up-sampling, then convolution) — two different algorithms for the same mathematics — must give the
    same losses and the same per-parameter gradient norms up to fp32 summation order."""
    from txt2vid_amd import functional_pool as FP
    from txt2vid_amd.gan.trainer import train_iteration
    B = 32
    random.seed(21)
    np.random.seed(21)
    torch.manual_seed(21)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    states = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    out = {}
    for mode in ('pooled', 'plain'):
        monkeypatch.setattr(FP, '_DISABLED', mode == 'plain')
        torch.set_rng_state(states[0])
        np.random.set_state(states[1])
        random.setstate(states[2])
        gan, optD, optG, losses, prm = _make_uncond()
        snap = {}
        step_d = optD.step

        def spy(*a, _snap=snap, _gan=gan, _step=step_d, **kw):      # D's gradients as its optimiser sees them (the G step zeroes them)
            _snap.update({k: float(p.grad.norm()) for k, p in _gan.discrims[0].named_parameters() if p.grad is not None})
            return _step(*a, **kw)
        optD.step = spy
        lD, lG, _, _ = train_iteration(gan, x, None, optD, optG, losses, prm, DEV)
        torch.cuda.synchronize()
        out[mode] = (float(lD), float(lG), snap, {k: float(p.grad.norm()) for k, p in gan.gen.named_parameters() if p.grad is not None})
    (lD0, lG0, d0, g0), (lD1, lG1, d1, g1) = out['pooled'], out['plain']
    print('pooled %.7f %.7f | plain %.7f %.7f' % (lD0, lG0, lD1, lG1))
    assert abs(lD0 - lD1) < 2e-5 and abs(lG0 - lG1) < 2e-5
    for a, b in ((d0, d1), (g0, g1)):
        assert set(a) == set(b) and len(a) > 20
        top = max(b.values())
        for k in b:
            assert abs(a[k] - b[k]) <= 1e-3 * abs(b[k]) + 1e-6 * top + 1e-7, (k, a[k], b[k])


def test_iteration_bf16_compute_mode_vs_oracle():
    """bf16-compute mode (forward / data-gradient GEMMs on bf16 MFMA; BASELINE configs 2-4 "bf16 compute / fp32 master"): one
    full iteration against the fp32 CPU oracle. bf16 operands carry 8 mantissa bits, so this is a LOOSER, separately stated
    bound: |dlossD| < 2e-2, |dlossG| < 5e-2 (fp32 mode: 1e-3)."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import train_iteration
    gan, optD, optG, losses, prm = _make_uncond()
    tr = O.OracleTrainer(O.recipe_state(O.gen_shapes(num_channels=1)), O.recipe_state(O.resnet3d_shapes('single_discrim.', 1, 64, 0)))
    random.seed(9)
    np.random.seed(9)
    torch.manual_seed(9)
    x = (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    st = torch.get_rng_state()
    old = TF.set_conv_precision('bf16')
    try:
        lD, lG, _, _ = train_iteration(gan, x.to(DEV), None, optD, optG, losses, prm, DEV)
        lD, lG = float(lD), float(lG)
    finally:
        TF.set_conv_precision(old)
    torch.set_rng_state(st)
    lDo, lGo = tr.step(x)
    print('bf16 compute: HIP lossD %.6f lossG %.6f | fp32 oracle %.6f %.6f' % (lD, lG, lDo, lGo))
    assert abs(lD - lDo) < 2e-2 and abs(lG - lGo) < 5e-2


@pytest.mark.parametrize('size,channels,batch,frame_sizes,tol', [
    (64, 1, 4, [8, 16, 32, 64], (2e-2, 5e-2)),              # BASELINE configs[2] at B=4: text-conditioned x bf16 compute
    (64, 1, 32, [8, 16, 32, 64], (2e-2, 5e-2)),             # BASELINE configs[2] AS BENCHMARKED (per-GPU batch 32; also configs[3]'s share)
    (128, 3, 2, [16, 32, 64, 128], (2e-2, 5e-2)),           # BASELINE configs[4] shape at B=2: 16x128x128x3, cond, bf16
    (128, 3, 16, [16, 32, 64, 128], (2e-2, 5e-2)),          # BASELINE configs[4] at ITS per-GPU batch (128 over 8 GPUs)
])
def test_cond_iteration_bf16_and_fp32_vs_oracle(size, channels, batch, frame_sizes, tol):
    """BASELINE configs[2] and the configs[4] shape (MSRVDC: 16x128x128x3, 2x2 ConvLSTM state, non-local blocks on 64x64 /
    32x32 maps) as ONE text-conditioned iteration against the fp32 CPU oracle on identical weights / batch / captions /
    draws — first in fp32 (bound 1e-3, the fp32 bound of every other shape), then in bf16-compute mode (operands rounded to
    8 mantissa bits, fp32 accumulation and storage: the separately stated, looser bound |dlossD| < 2e-2, |dlossG| < 5e-2)."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    V = 21

    class Prm(object):
        subsample_input = True
        discrim_steps = gen_steps = 1
        gp_lambda = 0.5
        no_mean_discrim_loss = no_mean_gen_loss = True
    Prm.frame_sizes = frame_sizes
    tg = torch.Generator()
    tg.manual_seed(77)
    tokens = torch.randint(4, V, (batch, 8), generator=tg)
    tokens[:, 0], tokens[:, -1] = 1, 2
    random.seed(21)
    np.random.seed(21)
    torch.manual_seed(21)
    x = (torch.rand(batch, 16, channels, size, size) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())

    def restore():
        torch.set_rng_state(state[0])
        np.random.set_state(state[1])
        random.setstate(state[2])
    # ---- oracle (fp32, CPU)
    PT = O.recipe_state(O.text_encoder_shapes(V))
    tr = O.OracleTrainer(O.recipe_state(O.gen_shapes(num_channels=channels, width=size, height=size, cond_dim=256, cond_variant=True)),
                         O.recipe_state(O.resnet3d_shapes('single_discrim.module.', channels, 64, 256)),
                         d_prefix='single_discrim.module.', frame_sizes=frame_sizes)
    with torch.no_grad():
        cond_o = O.text_encode(PT, tokens, [8] * batch)
    lDo, lGo = tr.step(x, cond=cond_o)
    # ---- HIP, fp32 then bf16 compute
    for mode, (tD, tG) in (('fp32', (1e-3, 1e-3)), ('bf16', tol)):
        gen = pour(MultiScaleGen(width=size, height=size, num_channels=channels, cond_dim=256))
        dis = pour(MultiScaleDiscrim(num_channels=channels, cond_dim=256))
        txt = Seq2Seq(vocab_size=V)
        txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                             for k, v in txt.state_dict().items()})
        txt.to(DEV)
        gen.train()
        dis.train()
        gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
        losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
        optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
        optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
        restore()
        old = TF.set_conv_precision(mode)
        try:
            with torch.no_grad():
                _, _, cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * batch)
            lD, lG, _, _ = train_iteration(gan, x.to(DEV), cond.detach(), optD, optG, losses, Prm(), DEV)
            lD, lG = float(lD), float(lG)
        finally:
            TF.set_conv_precision(old)
        print('cond %dx%dx%d B=%d %s: HIP lossD %.6f lossG %.6f | fp32 oracle %.6f %.6f' % (size, size, channels, batch, mode, lD, lG, lDo, lGo))
        assert abs(lD - lDo) < tD and abs(lG - lGo) < tG, (mode, lD, lDo, lG, lGo)
        del gan, gen, dis, optD, optG
        torch.cuda.empty_cache()


def test_end2end_iteration_vs_oracle():
    """`--end2end` (train/gan.py:82-85, trainer.py:211-263): the text encoder's parameters sit in BOTH optimisers, the sentence
    code keeps its graph through the D step (retain_graph) and the G backward runs through that graph again AFTER optD.step() has
    moved the encoder — the sequence the reference's pinned torch 0.4.1 executes (its optimiser writes through `.data`: no version
    bump) and stock torch >= 1.x rejects. Here Adam is a kernel writing through raw pointers, so it runs; the oracle's extension
    (`OracleTrainer(end2end_txt=...)`, `AdamOnData`) states the same semantics on the CPU. No fixture from the reference can
    exist for this path on torch 2.x: parity for this row is HIP vs oracle only (unpinned). One iteration: both losses, the
    encoder's gradient norms left by the G step, and the encoder's parameters after both updates."""
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    V, B = 21, 4
    gan, _, _, losses, prm = _make_cond(V)
    txt = gan.cond_encoder.differentiable(True)
    dis, gen = gan.discrims[0], gan.gen
    optD = Adam([{'params': dis.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    PT = O.recipe_state(O.text_encoder_shapes(V))
    before = {k: v.detach().clone() for k, v in PT.items()}
    tr = O.OracleTrainer(O.recipe_state(O.gen_shapes(num_channels=1, cond_dim=256, cond_variant=True)),
                         O.recipe_state(O.resnet3d_shapes('single_discrim.module.', 1, 64, 256)),
                         d_prefix='single_discrim.module.', end2end_txt=PT)
    tg = torch.Generator()
    tg.manual_seed(5)
    tokens = torch.randint(4, V, (B, 8), generator=tg)
    tokens[:, 0], tokens[:, -1] = 1, 2
    lengths = [8, 8, 6, 5]
    for b_, n in enumerate(lengths):
        tokens[b_, n:] = 0
        tokens[b_, n - 1] = 2
    random.seed(31)
    np.random.seed(31)
    torch.manual_seed(31)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    _, _, cond = txt.encode(tokens.to(DEV), lengths)                 # keeps its graph (trainer.py:213-214)
    assert cond.requires_grad
    lD, lG, _, _ = train_iteration(gan, x.to(DEV), cond, optD, optG, losses, prm, DEV, end2end=True)
    lD, lG = float(lD), float(lG)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    lDo, lGo = tr.step_end2end(x, tokens, lengths)
    print('end2end: HIP lossD %.6f lossG %.6f | oracle %.6f %.6f' % (lD, lG, lDo, lGo))
    assert abs(lD - lDo) < 1e-3 and abs(lG - lGo) < 1e-3
    named = dict(txt.encoder.named_parameters())
    ref_max = max(float(PT[k].grad.norm()) for k in tr.t_params)
    worst = 0.0
    for k in tr.t_params:                                            # gradients the G step left on the encoder
        got, want = float(named[k[len('encoder.'):]].grad.norm()), float(PT[k].grad.norm())
        assert abs(got - want) <= 1e-2 * want + 1e-5 * ref_max, (k, got, want)
        worst = max(worst, abs(got - want) / (want + 1e-5 * ref_max))
    # parameters after optD.step() and optG.step(): early Adam updates are ~ lr * sign(g), compare the applied deltas
    for k in ('encoder.embed.weight', 'encoder.lstm.weight_hh_l0', 'encoder.lstm.weight_ih_l3_reverse', 'encoder.lstm.bias_ih_l2'):
        d_o = PT[k].detach() - before[k]
        d_p = named[k[len('encoder.'):]].detach().cpu() - before[k]
        rel = float((d_p - d_o).abs().mean() / d_o.abs().mean().clamp_min(1e-12))
        assert float(d_o.abs().max()) > 0 and rel < 0.05, (k, rel)
    print('end2end: worst relative encoder gradient-norm deviation %.2e' % worst)


def test_graphed_sentence_encoder_matches_eager():
    """`GraphedSentenceEncoder`: first batch of a length eager, second captured, third replayed — all equal to the plain
    forward for ragged batches of two different longest lengths (the per-sample lengths live on the device)."""
    from txt2vid_amd.gan.trainer import GraphedSentenceEncoder
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.util.torch.init import init
    torch.manual_seed(3)
    m = Seq2Seq(vocab_size=41)
    init(m, 'xavier')
    m.to(DEV)
    ge = GraphedSentenceEncoder(m, torch.device(DEV))
    gen = torch.Generator()
    gen.manual_seed(8)
    for round_ in range(3):
        for lengths in ([9, 7, 7, 4, 2, 1], [6, 6, 5, 3, 3, 2]):
            tokens = torch.zeros(len(lengths), lengths[0], dtype=torch.long)
            for b, n in enumerate(lengths):
                tokens[b, :n] = torch.randint(1, 41, (n,), generator=gen)
            want = m.encode(tokens.to(DEV), lengths)[2].detach().cpu()
            got = ge.encode(tokens.to(DEV), lengths).cpu()
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=0)
    assert all(e[2] is not None for e in ge.entries.values()) and len(ge.entries) == 2


def test_static_draws_stage_through_a_ring_of_pinned_buffers():
    """`StaticDraws.begin_step` uploads an iteration's host draws asynchronously while the training loop runs the host ahead of
    the GPU: consecutive iterations must stage through DIFFERENT pinned buffers (a single one would be rewritten before its copy
    has executed), and a slot comes back only after the copy that read it is done."""
    from txt2vid_amd.draws import StaticDraws
    sd = StaticDraws(DEV, batch=4, latent=16, n_levels=4, n_gen_phases=3, gp=True, subsample_input=True, n_perms=2)
    torch.manual_seed(3)
    np.random.seed(3)
    seen = []
    for i in range(2 * sd.RING + 1):
        sd.begin_step()
        seen.append((sd.h_all, sd.h_all.clone()))
        if i:
            assert sd.h_all is not seen[i - 1][0]                       # the previous iteration's staging buffer is left alone
            assert torch.equal(seen[i - 1][0], seen[i - 1][1]) or i >= sd.RING
    torch.cuda.synchronize()
    assert torch.equal(sd.d_all.cpu(), seen[-1][1])                      # the device holds the LAST iteration's draws
    assert len({id(h) for h, _ in seen}) == sd.RING
    assert not torch.equal(seen[-1][1], seen[-2][1])                     # (fresh draws every iteration)
