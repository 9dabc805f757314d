"""BatchNorm parity cases shared by tests/test_norm_cpu.py (launch plans, the reference itself) and tests/test_norm_gpu.py
(every kernel path of the BatchNorm section of csrc/pointwise.hip), the input recipes, and the float64 reference.

How a launch is cut is size-dependent (`bn_split`: 1..64 statistics slices per channel, `bn_slices`: workgroups per channel
of the fused merge + apply passes), so each case names the cut it must get and the CPU test asserts it through `t2v_bn_plan`.

Tolerances. Metric: |got - ref| <= tol * max(1, |ref|max) + tol * |ref| against the float64 reference (the `close` of
tests/test_ops_gpu.py with rtol = atol = tol); tol = 1e-4 for y, dx, the running statistics and (mean, 1/std), 2e-4 for
dgamma / dbeta. On `straddle` / `offset`, fp32 `F.batch_norm` on the CPU is within 1.3e-5 of float64 on this metric (worst:
dgamma), a slice + Chan-merge variance within 4e-7, a one-pass E[x^2] - E[x]^2 variance off by 1.3e-2 (about 6e-3 in y): the
bound sits 8x above the reference's own rounding and 60x below the defect it has to catch.

Measured on an MI355X, worst error / bound per case / recipe over relu x up x fork and the raw ABI (1.0 would be the bound):
tiny plain 1.0e-3 (y), offset 0.056 (dgamma), dead 1.1e-3 (dx); one_pixel 1.5e-3 (dx); odd_row 9e-4 (dx); straddle plain
9e-4 (dx), offset 0.058 (dgamma), dead 1e-3 (dx); wide_c 9e-4 (dx); cap64 plain 1.3e-3 (dx), offset 0.26 (dgamma), dead
3.7e-3 (dgamma); default_hparams 7e-4 (dgamma). The three-launch ABI publishes bit-identical (mean, 1/std, running stats)
to the fused path. With the ReLU band below switched off, 9 `cap64` / `offset` / relu tests miss the dx bound (a flipped
mask element); none does with it. A scratch build with a one-pass slice variance fails 60 of the 284 GPU tests (every
`offset` one); one without the `blockIdx.y == 0` publish guard of `bn_apply_merge_k` fails 4 (running statistics at `cap64`) —
that one is a read-modify-write race, caught when workgroups of a channel interleave, which no test can force.
"""
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

# name -> (N, C, H, W), statistics slices, apply workgroups per channel, momentum, eps
CASES = {
    'tiny': ((4, 6, 5, 5), 1, 1, 0.3, 1e-3),
    'one_pixel': ((3, 5, 1, 1), 1, 1, 0.3, 1e-3),            # S = 1: `up` writes a 2x2 block per element
    'odd_row': ((2, 3, 1, 7), 1, 1, 0.3, 1e-3),              # H = 1, odd W (row pitch 2 * W of the up-sampled map)
    'straddle': ((5, 8, 21, 29), 2, 3, 0.3, 1e-3),           # 3045 per channel, S = 609: slices of 1523 / 1015 cut across samples, short tail
    'wide_c': ((2, 1030, 3, 3), 1, 1, 0.3, 1e-3),            # C > BN_STATS_WGS; final / publish over more than 256 * 4 channels
    'cap64': ((2, 3, 181, 183), 64, 65, 0.3, 1e-3),          # the BN_MAXSPLIT cap: 64-way Chan merge, slices of 1036 with a short tail
    'default_hparams': ((4, 6, 5, 5), 1, 1, 0.1, 1e-5),
}
RECIPES = ('plain', 'offset', 'dead')
# the recipes other than `plain` run where the slicing is interesting (and on `tiny`, for speed)
CASE_RECIPES = [(c, r) for c in CASES for r in (RECIPES if c in ('tiny', 'straddle', 'cap64') else ('plain',))]
FORKS = ('off', 'both', 'bn_only', 'alias_only')

TOL = {'y': 1e-4, 'dx': 1e-4, 'rm': 1e-4, 'rv': 1e-4, 'mean': 1e-4, 'istd': 1e-4, 'dgamma': 2e-4, 'dbeta': 2e-4}

# ReLU's derivative jumps at 0: where the float64 pre-activation lies inside (-RELU_BAND, RELU_BAND) but is not exactly 0, a
# correctly rounded fp32 kernel may sit on the other side and dL/dx there is not comparable. dL/dy is zeroed at those elements
# (under 0.1 % of them), so either side gives the same gradients. The band is wider than the y bound inside it at every case
# (1e-4 * (|y|max + |y|) < 1e-3 while |y|max < 10; `inputs` asserts it), so a kernel that passes the y check cannot flip the
# mask outside the band. Exact zeros (the `dead` recipe's channel 1: x = 0, beta = 0) keep their dL/dy: there the kernel's
# `y > 0` mask and torch's relu'(0) = 0 must agree.
# The band is needed, not only cautious: without it torch's own fp32 `F.batch_norm` on the CPU misses the dx bound against
# this reference on `cap64` / `offset` with ReLU (one flipped element of 198 738, dx off by 1.6e3 bounds), and passes with it.
RELU_BAND = 1e-3


def shape(case):
    return CASES[case][0]


def hparams(case):
    return CASES[case][3], CASES[case][4]


def plan(N, Cc, S):
    """(status, split, slices) of `t2v_bn_plan`: host arithmetic, no GPU."""
    from txt2vid_amd._lib import lib
    out = (C.c_int32 * 2)(-1, -1)
    st = lib().t2v_bn_plan(N, Cc, S, out)
    return st, out[0], out[1]


@functools.lru_cache(maxsize=None)
def inputs(case, recipe):
    """fp32 CPU tensors of one case / recipe (seeded; shared by every test, never modified)."""
    N, Cc, H, W = shape(case)
    _, eps = hparams(case)
    g = torch.Generator()
    g.manual_seed(1000 * list(CASES).index(case) + RECIPES.index(recipe) + 17)

    def randn(*s):
        return torch.randn(*s, generator=g)
    x = randn(N, Cc, H, W)
    gamma, beta = 1 + 0.1 * randn(Cc), 0.1 * randn(Cc)
    if recipe == 'offset':
        x = 300 + x
    elif recipe == 'dead':
        x[:, 1] = 0.0
        x[:, 2] = 0.1
        beta[1] = 0.0
    inp = {'x': x, 'gamma': gamma, 'beta': beta, 'rm': 0.1 * randn(Cc), 'rv': 1 + 0.1 * torch.rand(Cc, generator=g),
           'gy': randn(N, Cc, H, W), 'gy_up': randn(N, Cc, 2 * H, 2 * W), 'w2': randn(N, Cc, H, W)}
    pre = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, eps)
    near = (pre.abs() < RELU_BAND) & (pre != 0)
    inp['gy_relu'] = inp['gy'].masked_fill(near, 0.0)
    inp['gy_up_relu'] = inp['gy_up'].masked_fill(F.interpolate(near.double(), scale_factor=2) > 0, 0.0)
    assert TOL['y'] * (max(1.0, float(pre.abs().max())) + RELU_BAND) < RELU_BAND          # the band is wider than the y bound inside it
    return inp


def grad_out(inp, relu, up):
    return inp[('gy_up' if up else 'gy') + ('_relu' if relu else '')]


def reference(x, gamma, beta, rm, rv, gy, momentum, eps, relu, up, w2=None, fork='off', training=True, counter=None):
    """The whole op in float64 on the CPU: F.batch_norm -> [relu] -> [F.interpolate(x2)], autograd for the gradients of
    (y * gy).sum() [+ (x * w2).sum(): the input's second consumer, fork = 'both' / 'alias_only'; 'alias_only' and
    'bn_only' drop the other term / the second consumer]. Inputs are the fp32 tensors, cast up here."""
    xd = x.double().requires_grad_(training)
    gd, bd = gamma.double().requires_grad_(training), beta.double().requires_grad_(training)
    rmd, rvd = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xd, rmd, rvd, gd, bd, training, momentum, eps)
    if relu:
        y = F.relu(y)
    if up:
        y = F.interpolate(y, scale_factor=2)
    out = {'y': y.detach(), 'rm': rmd, 'rv': rvd}
    if counter is not None:
        out['counter'] = counter + (1 if training else 0)
    if not training:
        return out
    dims = [0] + list(range(2, x.dim()))
    out['mean'] = x.double().mean(dims)
    out['istd'] = 1.0 / torch.sqrt(x.double().var(dims, unbiased=False) + eps)
    loss = 0.0
    if fork != 'alias_only':
        loss = loss + (y * gy.double()).sum()
    if fork in ('both', 'alias_only'):
        loss = loss + (xd * w2.double()).sum()
    grads = torch.autograd.grad(loss, [xd, gd, bd], allow_unused=True)
    for name, g, like in zip(('dx', 'dgamma', 'dbeta'), grads, (xd, gd, bd)):
        out[name] = torch.zeros_like(like) if g is None else g
    return out


@functools.lru_cache(maxsize=None)
def case_reference(case, recipe, relu, up, fork='off'):
    inp = inputs(case, recipe)
    momentum, eps = hparams(case)
    return reference(inp['x'], inp['gamma'], inp['beta'], inp['rm'], inp['rv'], grad_out(inp, relu, up), momentum, eps, relu, up,
                     w2=inp['w2'], fork=fork)


def ratio(got, ref, tol):
    """worst |got - ref| / (tol * max(1, |ref|max) + tol * |ref|): <= 1 is what `close(got, ref, rtol=tol, atol=tol)` accepts."""
    a = got.detach().cpu().double().numpy()
    b = ref.detach().cpu().double().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    if not np.isfinite(a).all():
        return float('inf')
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    return float((np.abs(a - b) / (tol * scale + tol * np.abs(b))).max()) if b.size else 0.0


def check(tag, got, ref, fields):
    """Prints every field's ratio (`bn-ratio <tag> <field> <ratio>`), then asserts all of them."""
    rs = {f: ratio(got[f], ref[f], TOL[f]) for f in fields}
    for f in fields:
        print('bn-ratio %s %s %.4g' % (tag, f, rs[f]))
    bad = {f: r for f, r in rs.items() if not r <= 1.0}
    assert not bad, '%s: error / bound %s' % (tag, bad)
