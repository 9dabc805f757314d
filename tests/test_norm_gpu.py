"""GPU: every BatchNorm kernel path of csrc/pointwise.hip (nine C entry points, seven kernels) against the float64 reference of
tests/norm_cases.py, at shapes whose cut `t2v_bn_plan` pins (tests/test_norm_cpu.py): several statistics slices and their Chan
merge, slices that straddle samples, the short last slice, the 64-slice cap, and the "only slice 0 publishes" guards."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _tag(*parts):
    return '/'.join(str(p) for p in parts)


def run_op(inp, momentum, eps, relu, up, fork, x_dev=None, counter=None):
    """One training-mode `TF.batch_norm_act` forward + backward on fresh device copies of `inp`; results as a dict."""
    from txt2vid_amd import functional as TF
    x = inp['x'].to(DEV).requires_grad_(True) if x_dev is None else x_dev
    gamma, beta = torch.nn.Parameter(inp['gamma'].to(DEV)), torch.nn.Parameter(inp['beta'].to(DEV))
    rm, rv = inp['rm'].to(DEV).clone(), inp['rv'].to(DEV).clone()          # (updated in place: never the shared inputs)
    gy, w2 = nc.grad_out(inp, relu, up).to(DEV), inp['w2'].to(DEV)
    res = TF.batch_norm_act(x, gamma, beta, rm, rv, True, momentum, eps, relu, counter, up, fork != 'off')
    y, alias = res if fork != 'off' else (res, None)
    loss = 0.0
    if fork != 'alias_only':
        loss = loss + (y * gy.reshape(y.shape)).sum()
    if fork in ('both', 'alias_only'):
        loss = loss + (alias * w2.reshape(alias.shape)).sum()
    grads = torch.autograd.grad(loss, [x, gamma, beta], allow_unused=True)
    out = {'y': y.detach(), 'rm': rm, 'rv': rv, 'alias': alias}
    for name, g, like in zip(('dx', 'dgamma', 'dbeta'), grads, (x, gamma, beta)):
        out[name] = torch.zeros_like(like) if g is None else g
    return out


FIELDS = ['y', 'dx', 'dgamma', 'dbeta', 'rm', 'rv']


# ---------------------------------------------------------------- a. the autograd surface
@pytest.mark.parametrize('fork', nc.FORKS)
@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case,recipe', nc.CASE_RECIPES, ids=['%s-%s' % cr for cr in nc.CASE_RECIPES])
def test_batch_norm_act(case, recipe, relu, up, fork):
    inp = nc.inputs(case, recipe)
    momentum, eps = nc.hparams(case)
    got = run_op(inp, momentum, eps, relu, up, fork)
    nc.check(_tag(case, recipe, int(relu), int(up), fork), got, nc.case_reference(case, recipe, relu, up, fork), FIELDS)
    if fork != 'off':
        assert torch.equal(got['alias'].detach().cpu(), inp['x'])


@pytest.mark.parametrize('fork', nc.FORKS)
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
def test_batch_norm_act_3d_input(relu, fork):
    """[4,6,25] (BatchNorm over (N, L)): the `tiny` case flattened; `fork` hands back x itself."""
    inp = dict(nc.inputs('tiny', 'plain'))
    momentum, eps = nc.hparams('tiny')
    for k in ('x', 'gy', 'gy_relu', 'w2'):
        inp[k] = inp[k].reshape(4, 6, 25)
    x = inp['x'].to(DEV).requires_grad_(True)
    got = run_op(inp, momentum, eps, relu, False, fork, x_dev=x)
    ref = nc.case_reference('tiny', 'plain', relu, False, fork)
    ref = {k: (v.reshape(4, 6, 25) if v.dim() == 4 else v) for k, v in ref.items()}
    nc.check(_tag('tiny3d', int(relu), fork), got, ref, FIELDS)
    if fork != 'off':
        assert got['alias'] is x


@pytest.mark.parametrize('fork', nc.FORKS)
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case', ['tiny', 'straddle'])
def test_batch_norm_act_non_contiguous_input(case, relu, fork):
    """x = every second channel of a [N,2C,H,W] tensor: the op sees the same values, the gradient lands in the even channels.
    The alias that `fork` hands back is checked by VALUE here, not by identity: a strided 4-D input that requires a gradient
    runs `BatchNormActFork` on the dense copy the op makes first, and the alias is a view of that copy. Only the 3-D input
    (above) and eval mode get x itself back."""
    inp = nc.inputs(case, 'plain')
    momentum, eps = nc.hparams(case)
    N, Cc, H, W = nc.shape(case)
    big = torch.full((N, 2 * Cc, H, W), 1e6)
    big[:, ::2] = inp['x']
    big = big.to(DEV).requires_grad_(True)
    x = big[:, ::2]
    assert not x.is_contiguous()
    from txt2vid_amd import functional as TF
    gamma, beta = torch.nn.Parameter(inp['gamma'].to(DEV)), torch.nn.Parameter(inp['beta'].to(DEV))
    rm, rv = inp['rm'].to(DEV).clone(), inp['rv'].to(DEV).clone()          # (updated in place: never the shared inputs)
    res = TF.batch_norm_act(x, gamma, beta, rm, rv, True, momentum, eps, relu, None, False, fork != 'off')
    y, alias = res if fork != 'off' else (res, None)
    loss = 0.0
    if fork != 'alias_only':
        loss = loss + (y * nc.grad_out(inp, relu, False).to(DEV)).sum()
    if fork in ('both', 'alias_only'):
        loss = loss + (alias * inp['w2'].to(DEV)).sum()
        assert torch.equal(alias.detach().cpu(), inp['x'])
    loss.backward()
    zero = torch.zeros(Cc, device=DEV)
    got = {'y': y, 'dx': big.grad[:, ::2], 'dgamma': zero if gamma.grad is None else gamma.grad,
           'dbeta': zero if beta.grad is None else beta.grad, 'rm': rm, 'rv': rv}
    nc.check(_tag(case, 'strided', int(relu), fork), got, nc.case_reference(case, 'plain', relu, False, fork), FIELDS)
    assert not big.grad[:, 1::2].any()


# ---------------------------------------------------------------- b. the step counter
@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('case', ['straddle', 'cap64', 'wide_c'])
def test_counter_is_incremented_once_per_launch_in_int64(case, up):
    """`straddle` (8 x 3 workgroups) and `cap64` (3 x 65) hold the `blockIdx.y == 0` half of the guard to one increment;
    `wide_c` has one slice per channel, its 1030 workgroups come from C alone: it holds the `c == 0` half."""
    from txt2vid_amd import functional as TF
    inp = nc.inputs(case, 'plain')
    (N, Cc, H, W), _, slices, _, _ = nc.CASES[case]
    assert Cc * slices > 8 and (slices > 1 or case == 'wide_c')          # many workgroups, one increment
    x, gamma, beta = inp['x'].to(DEV), inp['gamma'].to(DEV), inp['beta'].to(DEV)
    rm, rv = inp['rm'].to(DEV).clone(), inp['rv'].to(DEV).clone()          # (updated in place: never the shared inputs)
    counter = torch.tensor(2 ** 31 + 5, dtype=torch.int64, device=DEV)
    TF.batch_norm_act(x, gamma, beta, rm, rv, True, 0.3, 1e-3, True, counter, up)
    assert int(counter) == 2 ** 31 + 6
    TF.batch_norm_act(x, gamma, beta, rm, rv, True, 0.3, 1e-3, True, counter, up)
    assert int(counter) == 2 ** 31 + 7
    TF.batch_norm_act(x, gamma, beta, rm, rv, False, 0.3, 1e-3, True, counter, up)          # eval mode: untouched
    assert int(counter) == 2 ** 31 + 7
    with pytest.raises(TypeError):
        TF.batch_norm_act(x, gamma, beta, rm, rv, True, 0.3, 1e-3, True, counter.int(), up)


# ---------------------------------------------------------------- c. eval mode
@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
def test_eval_mode(relu, up):
    """Running statistics, one channel with a running variance of exactly 0 (1/std = 1/sqrt(eps)); the buffers stay as they are."""
    from txt2vid_amd import functional as TF
    case = 'straddle'
    inp = nc.inputs(case, 'plain')
    momentum, eps = nc.hparams(case)
    rv = inp['rv'].clone()
    rv[3] = 0.0
    ref = nc.reference(inp['x'], inp['gamma'], inp['beta'], inp['rm'], rv, None, momentum, eps, relu, up, training=False)
    rmd, rvd = inp['rm'].to(DEV).clone(), rv.to(DEV).clone()
    for fork in (False, True):
        x = inp['x'].to(DEV)
        res = TF.batch_norm_act(x, inp['gamma'].to(DEV), inp['beta'].to(DEV), rmd, rvd, False, momentum, eps, relu, None, up, fork)
        if fork:
            assert res[1] is x
            res = res[0]
        nc.check(_tag(case, 'eval', int(relu), int(up), int(fork)), {'y': res}, ref, ['y'])
    assert torch.equal(rmd.cpu(), inp['rm']) and torch.equal(rvd.cpu(), rv)


# ---------------------------------------------------------------- d. bit-reproducibility
@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('case', ['cap64', 'straddle'])
def test_two_runs_give_the_same_bits(case, up):
    inp = nc.inputs(case, 'offset')
    momentum, eps = nc.hparams(case)
    a = run_op(inp, momentum, eps, True, up, 'both')
    b = run_op(inp, momentum, eps, True, up, 'both')
    for f in FIELDS:
        assert torch.equal(a[f], b[f]), f


# ---------------------------------------------------------------- e. the raw ABI, with guard bands
SENTINEL = -7777.25
GUARD = 256


class Guarded(object):
    """`n` elements carved out of a larger allocation, GUARD sentinel elements on each side; the inside starts as NaN, so
    an element the kernel never wrote fails the comparison."""

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
        self.t = self.buf[GUARD:GUARD + n]
        if init is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(init.reshape(-1))
        self.p = C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


class _Raw(object):
    """Device inputs and guarded outputs of one case / recipe for the C entry points."""

    def __init__(self, case, recipe, relu, up):
        from txt2vid_amd._lib import lib
        from txt2vid_amd._ops import _stream
        self.lib, self.stream = lib(), _stream()
        self.inp = inp = nc.inputs(case, recipe)
        self.N, self.C, self.H, self.W = nc.shape(case)
        self.S = self.H * self.W
        self.momentum, self.eps = nc.hparams(case)
        self.relu, self.up = int(relu), int(up)
        self.keep = [inp[k].to(DEV).contiguous() for k in ('x', 'gamma', 'beta', 'w2')] + [nc.grad_out(inp, relu, up).to(DEV).contiguous()]
        self.x, self.gamma, self.beta, self.w2, self.gy = [C.c_void_p(t.data_ptr()) for t in self.keep]
        self.n = self.N * self.C * self.S
        self.ws_floats = int(self.lib.t2v_bn_ws_floats(self.N, self.C, self.S))
        assert self.ws_floats == 3 * self.C * nc.CASES[case][1] + 2 * self.C
        self.guards = []

    def out(self, n, init=None):
        g = Guarded(n, init)
        self.guards.append(g)
        return g

    def ws(self):
        return self.out(self.ws_floats)                      # exactly t2v_bn_ws_floats elements

    def ok(self, status):
        assert status == 0, status

    def assert_guards(self):
        torch.cuda.synchronize()
        assert all(g.intact() for g in self.guards), [i for i, g in enumerate(self.guards) if not g.intact()]

    def shaped(self, g, up=False):
        m = 2 if up else 1
        return g.t.reshape(self.N, self.C, m * self.H, m * self.W)

    def stats(self, g):
        return {'mean': g.t[:self.C], 'istd': g.t[self.C:]}


RAW_CASES = [(c, r) for c in ('straddle', 'cap64') for r in nc.RECIPES]
RAW_IDS = ['%s-%s' % cr for cr in RAW_CASES]


@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case,recipe', RAW_CASES, ids=RAW_IDS)
def test_three_launch_abi(case, recipe, relu):
    """t2v_bn_stats -> t2v_bn_apply -> t2v_bn_bwd (no Python caller): same results as the reference, same statistics as the
    fused path, nothing written outside the buffers."""
    r = _Raw(case, recipe, relu, False)
    L, N, Cc, S = r.lib, r.N, r.C, r.S
    stats, stats_null, stats_fused = r.out(2 * Cc), r.out(2 * Cc), r.out(2 * Cc)
    rm, rv = r.out(Cc, r.inp['rm'].to(DEV)), r.out(Cc, r.inp['rv'].to(DEV))
    y, gx, dg, db = r.out(r.n), r.out(r.n), r.out(Cc), r.out(Cc)
    ws_f, ws_n, ws_b, ws_t = r.ws(), r.ws(), r.ws(), r.ws()
    r.ok(L.t2v_bn_stats(r.x, stats.p, rm.p, rv.p, ws_f.p, N, Cc, S, r.momentum, r.eps, r.stream))
    r.ok(L.t2v_bn_stats(r.x, stats_null.p, None, None, ws_n.p, N, Cc, S, r.momentum, r.eps, r.stream))       # rm = rv = NULL
    r.ok(L.t2v_bn_apply(r.x, stats.p, r.gamma, r.beta, y.p, N, Cc, S, r.relu, r.stream))
    r.ok(L.t2v_bn_bwd(r.gy, r.x, y.p, stats.p, r.gamma, gx.p, dg.p, db.p, ws_b.p, N, Cc, S, r.relu, r.stream))
    y_f, rm_f, rv_f = r.out(r.n), r.out(Cc, r.inp['rm'].to(DEV)), r.out(Cc, r.inp['rv'].to(DEV))
    r.ok(L.t2v_bn_train_fwd(r.x, r.gamma, r.beta, y_f.p, stats_fused.p, rm_f.p, rv_f.p, ws_t.p, N, Cc, S, r.momentum, r.eps, r.relu,
                            None, r.stream))
    r.assert_guards()
    ref = nc.case_reference(case, recipe, bool(relu), False, 'off')
    got = {'y': r.shaped(y), 'dx': r.shaped(gx), 'dgamma': dg.t, 'dbeta': db.t, 'rm': rm.t, 'rv': rv.t}
    got.update(r.stats(stats))
    nc.check(_tag(case, recipe, int(relu), 'abi3'), got, ref, FIELDS + ['mean', 'istd'])
    assert torch.equal(stats_null.t, stats.t)
    nc.check(_tag(case, recipe, int(relu), 'abi3-vs-fused'), r.stats(stats), r.stats(stats_fused), ['mean', 'istd'])
    nc.check(_tag(case, recipe, int(relu), 'abi3-vs-fused'), {'y': y.t, 'rm': rm.t, 'rv': rv.t}, {'y': y_f.t, 'rm': rm_f.t, 'rv': rv_f.t},
             ['y', 'rm', 'rv'])


@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case,recipe', RAW_CASES, ids=RAW_IDS)
def test_fused_abi(case, recipe, relu, up):
    """t2v_bn_train_fwd[_up] -> t2v_bn_train_bwd[_up] and t2v_bn_train_bwd_add on guarded buffers."""
    r = _Raw(case, recipe, relu, up)
    L, N, Cc, S, H, W = r.lib, r.N, r.C, r.S, r.H, r.W
    ny = r.n * (4 if up else 1)
    stats, rm, rv = r.out(2 * Cc), r.out(Cc, r.inp['rm'].to(DEV)), r.out(Cc, r.inp['rv'].to(DEV))
    y, gx, dg, db = r.out(ny), r.out(r.n), r.out(Cc), r.out(Cc)
    gx_a, dg_a, db_a = r.out(r.n), r.out(Cc), r.out(Cc)
    gx_0, dg_0, db_0 = r.out(r.n), r.out(Cc), r.out(Cc)
    ws_f, ws_b, ws_a, ws_0 = r.ws(), r.ws(), r.ws(), r.ws()
    counter = torch.tensor([-9, 2 ** 40 + 1, -9], dtype=torch.int64, device=DEV)
    cp = C.c_void_p(counter[1:].data_ptr())
    if up:
        r.ok(L.t2v_bn_train_fwd_up(r.x, r.gamma, r.beta, y.p, stats.p, rm.p, rv.p, ws_f.p, N, Cc, H, W, r.momentum, r.eps, r.relu, cp, r.stream))
        r.ok(L.t2v_bn_train_bwd_up(r.gy, r.x, y.p, stats.p, r.gamma, gx.p, dg.p, db.p, ws_b.p, N, Cc, H, W, r.relu, r.stream))
    else:
        r.ok(L.t2v_bn_train_fwd(r.x, r.gamma, r.beta, y.p, stats.p, rm.p, rv.p, ws_f.p, N, Cc, S, r.momentum, r.eps, r.relu, cp, r.stream))
        r.ok(L.t2v_bn_train_bwd(r.gy, r.x, y.p, stats.p, r.gamma, gx.p, dg.p, db.p, ws_b.p, N, Cc, S, r.relu, r.stream))
    r.ok(L.t2v_bn_train_bwd_add(r.gy, r.x, y.p, stats.p, r.gamma, r.w2, gx_a.p, dg_a.p, db_a.p, ws_a.p, N, Cc, H, W, r.up, r.relu, r.stream))
    r.ok(L.t2v_bn_train_bwd_add(r.gy, r.x, y.p, stats.p, r.gamma, None, gx_0.p, dg_0.p, db_0.p, ws_0.p, N, Cc, H, W, r.up, r.relu, r.stream))
    r.assert_guards()
    assert counter.tolist() == [-9, 2 ** 40 + 2, -9]
    ref = nc.case_reference(case, recipe, bool(relu), bool(up), 'off')
    got = {'y': r.shaped(y, up), 'dx': r.shaped(gx), 'dgamma': dg.t, 'dbeta': db.t, 'rm': rm.t, 'rv': rv.t}
    got.update(r.stats(stats))
    nc.check(_tag(case, recipe, int(relu), int(up), 'fused'), got, ref, FIELDS + ['mean', 'istd'])
    got_a = {'dx': r.shaped(gx_a), 'dgamma': dg_a.t, 'dbeta': db_a.t}
    nc.check(_tag(case, recipe, int(relu), int(up), 'bwd_add'), got_a, nc.case_reference(case, recipe, bool(relu), bool(up), 'both'),
             ['dx', 'dgamma', 'dbeta'])
    # without a second gradient the `add` entry point is the plain adjoint: the same kernels on the same inputs
    assert torch.equal(gx_0.t, gx.t) and torch.equal(dg_0.t, dg.t) and torch.equal(db_0.t, db.t)


def test_abi_rejects_bad_arguments():
    from txt2vid_amd._lib import lib
    one = torch.zeros(64, device=DEV)
    p = C.c_void_p(one.data_ptr())
    L = lib()
    assert L.t2v_bn_stats(None, p, None, None, p, 1, 1, 1, 0.1, 1e-5, None) < 0
    assert L.t2v_bn_stats(p, p, None, None, p, 0, 1, 1, 0.1, 1e-5, None) < 0
    assert L.t2v_bn_apply(p, p, p, p, None, 1, 1, 1, 0, None) < 0
    assert L.t2v_bn_bwd(p, p, None, p, p, p, p, p, p, 1, 1, 1, 1, None) < 0           # relu needs y
    assert L.t2v_bn_train_fwd(p, p, p, p, p, None, None, None, 1, 1, 1, 0.1, 1e-5, 0, None, None) < 0
    assert L.t2v_bn_train_fwd_up(p, p, p, p, p, None, None, p, 1, 1, 0, 1, 0.1, 1e-5, 0, None, None) < 0
    assert L.t2v_bn_train_bwd(p, p, None, p, p, p, p, p, p, 1, 1, 1, 1, None) < 0
    assert L.t2v_bn_train_bwd_up(p, p, p, p, p, p, p, p, p, 1, 1, 1, 0, 0, None) < 0
    assert L.t2v_bn_train_bwd_add(p, p, None, p, p, None, p, p, p, p, 1, 1, 1, 1, 0, 1, None) < 0
    assert L.t2v_bn_eval(p, p, p, p, p, p, 1, -1, 1, 1e-5, 0, None) < 0


# ---------------------------------------------------------------- f. the BatchNorm half of the former test_batchnorm_tanh_upsample
def test_tiny_default_hparams_against_fp32_torch():
    """`tiny` / `default_hparams` ([4,6,5,5], momentum 0.1, eps 1e-5, fused ReLU) against fp32 torch on the CPU, then eval
    mode on the updated buffers."""
    from txt2vid_amd import functional as TF

    def rnd(seed, *shape):
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randn(*shape, generator=g)

    def close(a, b, rtol=1e-4, atol=1e-4):
        a = a.detach().cpu().double().numpy()
        b = b.detach().cpu().double().numpy()
        scale = max(1.0, float(np.abs(b).max()))
        np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale)
    x = rnd(1, 4, 6, 5, 5)
    gamma, beta = 1 + 0.1 * rnd(2, 6), 0.1 * rnd(3, 6)
    rm, rv = 0.1 * rnd(4, 6), 1 + 0.1 * torch.rand(6, generator=torch.Generator().manual_seed(6))
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rmr, rvr = rm.clone(), rv.clone()
    yr = F.relu(F.batch_norm(xr, rmr, rvr, gr, br, True, 0.1, 1e-5))
    gy = rnd(5, *yr.shape)
    (yr * gy).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    gd, bd = torch.nn.Parameter(gamma.to(DEV)), torch.nn.Parameter(beta.to(DEV))
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    yd = TF.batch_norm_act(xd, gd, bd, rmd, rvd, True, 0.1, 1e-5, True)
    close(yd, yr)
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rtol=1e-3, atol=1e-4)
    close(gd.grad, gr.grad, rtol=1e-3, atol=1e-4)
    close(bd.grad, br.grad, rtol=1e-3, atol=1e-4)
    close(rmd, rmr)
    close(rvd, rvr)
    # eval mode
    ye = TF.batch_norm_act(x.to(DEV), gd, bd, rmd, rvd, False, 0.1, 1e-5, False)
    close(ye, F.batch_norm(x, rmr, rvr, gamma, beta, False, 0.1, 1e-5))
