"""BatchNorm shapes for the unrolled slice walker of the two-launch training passes (csrc/pointwise.hip: `BnWalk`, trips of
BN_UNROLL = 8 elements, BN_REG_CAP = 32 values a statistics thread keeps in registers), shared by
tests/test_norm_passes_cpu.py (the cuts, through `t2v_bn_plan`), tests/test_norm_passes_gpu.py and tools/bn_bits.py.

The cases of tests/norm_cases.py give a thread at most 6 elements: none of them runs a full trip. A thread of a slice of L
elements visits ceil((L - t) / 256) of them, so the counts below are (longest slice / 256) rounded down and up. The statistics
pass and the first adjoint pass are cut by `split`, the two apply passes by `slices`. PER_THREAD (asserted by the CPU test)
gives both counts per case; between them the cases put each pass below a trip (a predicated tail only), at one full trip plus a
tail, and the statistics pass also between a trip and the cap (not a multiple of 8), above the cap, and on the cap's edge.

An apply workgroup gets 2048 elements or more only when the tensor has about 2048 * 2048 of them (`bn_slices` aims at 2048
workgroups of at least 1024 elements), so the `wide_*` cases are 4.7 M elements (19 MB); the others stay near 1 M.
Row lengths: S = 1, 7, 64 (a thread's stride of 256 crosses four samples per step), 255 (odd, just below the stride), 258 (just
above it, odd rows of 43); every case but `wide_s1` cuts or strides through samples mid-row.
"""
import functools

import torch
import torch.nn.functional as F

import norm_cases as nc

UNROLL, REG_CAP = 8, 32

# name -> (N, C, H, W), statistics slices, apply workgroups per channel
CASES = {
    'wide_s1': ((2300, 2049, 1, 1), 1, 1),          # one workgroup per channel everywhere: 8 or 9 elements per thread, S = 1
    'wide_s7': ((330, 2049, 1, 7), 1, 1),           # 2310 per channel: 9 or 10 per thread, S = 7
    'wide_s64': ((36, 2049, 8, 8), 1, 1),           # 2304 per channel: 9 per thread, S = 64
    'wide_s255': ((9, 2049, 15, 17), 1, 1),         # 2295 per channel: 8 or 9 per thread, S = 255 (odd)
    'mid_s64': ((3000, 3, 8, 8), 64, 188),          # statistics slices of 3000 (11 or 12 per thread, start mid-sample), apply 1022
    'cap_s7': ((93700, 2, 7, 1), 64, 641),          # statistics slices of 10249: 40 or 41 per thread (above the cap); apply 1024
    'small_s7': ((300, 5, 7, 1), 2, 3),             # slices of 1050 / 700: tails only (4 or 5, 2 or 3 per thread)
    'edge_s258': ((2040, 2, 6, 43), 64, 514),       # statistics slices of 8224: 32 (registers) or 33 (re-read) in ONE workgroup
}
# name -> ((fewest, most) elements of a thread in the longest statistics slice, the same for the apply passes)
PER_THREAD = {
    'wide_s1': ((8, 9), (8, 9)),
    'wide_s7': ((9, 10), (9, 10)),
    'wide_s64': ((9, 9), (9, 9)),
    'wide_s255': ((8, 9), (8, 9)),
    'mid_s64': ((11, 12), (3, 4)),
    'cap_s7': ((40, 41), (4, 4)),
    'small_s7': ((4, 5), (2, 3)),
    'edge_s258': ((32, 33), (4, 4)),
}
MOMENTUM, EPS = 0.3, 1e-3
RECIPES = ('plain', 'offset')
# `offset` (x = 300 + noise: a second moment taken about a wrong mean is off by far more than the bound) where the statistics
# thread holds more than a trip, in registers (mid_s64), re-reading (cap_s7) and both side by side (edge_s258)
CASE_RECIPES = [(c, 'plain') for c in CASES] + [(c, 'offset') for c in ('mid_s64', 'cap_s7', 'edge_s258')]


def shape(case):
    return CASES[case][0]


def per_thread(total, cuts):
    """(fewest, most) elements a thread of the longest slice visits when `total` elements are cut `cuts` ways."""
    per = (total + cuts - 1) // cuts
    return per // 256, (per + 255) // 256


@functools.lru_cache(maxsize=2)
def inputs(case, recipe):
    """fp32 CPU tensors of one case / recipe, as tests/norm_cases.py makes them (seeded; shared, never modified). The tests go
    case by case, so only the last two are kept: a `wide_*` one is 230 MB with its up-sampled gradients."""
    N, Cc, H, W = shape(case)
    g = torch.Generator()
    g.manual_seed(7000 + 10 * list(CASES).index(case) + RECIPES.index(recipe))

    def randn(*s):
        return torch.randn(*s, generator=g)
    x = randn(N, Cc, H, W)
    gamma, beta = 1 + 0.1 * randn(Cc), 0.1 * randn(Cc)
    if recipe == 'offset':
        x = 300 + x
    inp = {'x': x, 'gamma': gamma, 'beta': beta, 'rm': 0.1 * randn(Cc), 'rv': 1 + 0.1 * torch.rand(Cc, generator=g),
           'gy': randn(N, Cc, H, W), 'gy_up': randn(N, Cc, 2 * H, 2 * W), 'w2': randn(N, Cc, H, W)}
    pre = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, EPS)
    near = (pre.abs() < nc.RELU_BAND) & (pre != 0)
    inp['gy_relu'] = inp['gy'].masked_fill(near, 0.0)
    inp['gy_up_relu'] = inp['gy_up'].masked_fill(F.interpolate(near.double(), scale_factor=2) > 0, 0.0)
    assert nc.TOL['y'] * (max(1.0, float(pre.abs().max())) + nc.RELU_BAND) < nc.RELU_BAND          # (norm_cases.RELU_BAND)
    return inp


def case_reference(case, recipe, relu, up, fork='off'):
    inp = inputs(case, recipe)
    return nc.reference(inp['x'], inp['gamma'], inp['beta'], inp['rm'], inp['rv'], nc.grad_out(inp, relu, up), MOMENTUM, EPS, relu, up,
                        w2=inp['w2'], fork=fork)
