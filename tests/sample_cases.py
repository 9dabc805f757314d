"""Shared inputs and numpy references of the sampling tool's tests (`python -m txt2vid_amd.gan.sample`; not in the
reference) — used by test_sample_cpu.py and test_sample_gpu.py. No reference exists to record a fixture from: numpy is the yardstick.

The export byte. q = rint(x * 127.5 + 127.5), product and sum two rounded float32 operations, rint half to even, clamped to
[0, 255], NaN -> 0 (`functional_sample.byte_map` is that expression). The kernel's arithmetic is pinned to the same operations, so
the comparison is EQUALITY. It inverts `data.unit_range` on all 256 bytes (test_sample_cpu).

The distance bound (derived, not measured). d2 = sum_k (g_k - r_k)^2 over fp32 inputs; the kernel forms each difference in fp32,
d_k = (g_k - r_k)(1 + a_k), |a_k| <= u = 2^-24, and accumulates acc <- fma(d_k, d_k, acc) = (d_k^2 + acc)(1 + b_k), |b_k| <= u, over a
slab of at most L = t2v_clip_nn_chain(D) elements. Term k of a slab is therefore multiplied by (1 + a_k)^2 and by at most L factors
(1 + b): every term is non-negative, so the slab's computed sum lies within ((1 + u)^(L+2) - 1) of its exact value RELATIVELY, and so
does the sum over slabs, which is added in float64 in a fixed order: one more relative 2^-53 per slab. Hence

    |d2_hat - d2| <= gamma * d2,   gamma = (1 + 2^-24)^(L+2) - 1 + slabs * 2^-53        (`functional_sample.nn_gamma`)

with d2 the float64 sum over the same fp32 inputs (differences of fp32 values are exact in float64; its own rounding, <= D * 2^-53
relative, is four orders below gamma). The test multiplies gamma by nothing.

Planted clips. The samples sit in a tight cluster, g_n = p + 1e-3 * noise_n; real clip j is g_(j mod N) + s_j * nu_j with |nu_j|^2 = D
and the scales s_j = 0.05 * 1.25^pi(j), pi a permutation: d2(n, j) = s_j^2 D (1 +- 0.06), consecutive scales differ by 1.5625 in d2, so
the ordering of every sample's candidates has relative gaps above 0.3 — `min_gap` measures them on the float64 reference and the
tests assert >= 0.1, far above 2 * gamma (1.6e-5 at the 16x64x64 clip, 1.9e-4 at the longest chain).

Standing statistics. The tolerance on the 16 sites' buffers is the one test_models_gpu.py::test_gen applies to buffers (rtol 1e-3,
atol 1e-4 of the tensor's scale)."""
import functools

import numpy as np

EXPORT_SHAPES = [(1, 1, 1, 8, 8), (3, 3, 2, 8, 8), (2, 1, 16, 64, 64), (2, 3, 2, 5, 6)]          # the last: H*W % 4 != 0, the scalar path
NN_N, NN_B, NN_K = (1, 3, 64), (1, 5, 64), (1, 8)
NN_BIG_D = 65536
MIN_GAP = 0.1
BUF_RTOL, BUF_ATOL = 1e-3, 1e-4


def unit_table():
    from txt2vid_amd.data import unit_range
    return unit_range(np.arange(256, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def halfway():
    """(x float32 [m], k int [m]): inputs whose x * 127.5 + 127.5 is EXACTLY k + 0.5 in the pinned float32 arithmetic, found by
    walking a few ulps around (k + 0.5 - 127.5) / 127.5. The byte must be the even one of k, k + 1."""
    xs, ks = [], []
    for k in range(255):
        x = np.float32((k + 0.5 - 127.5) / 127.5)
        cand = [x]
        lo = hi = x
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2))
            cand += [lo, hi]
        for c in cand:
            if np.float32(c) * np.float32(127.5) + np.float32(127.5) == np.float32(k + 0.5):
                xs.append(np.float32(c))
                ks.append(k)
                break
    return np.asarray(xs, np.float32), np.asarray(ks, np.int64)


def halfway_bytes():
    _, k = halfway()
    return np.where(k % 2 == 0, k, k + 1).astype(np.uint8)


SPECIAL = np.asarray([-2.0, 2.0, np.inf, -np.inf, np.nan, -1.0, 1.0, 0.0, -0.0, 1.0000001, -1.0000001, 1e30, -1e30, 1e-40],
                     dtype=np.float32)
SPECIAL_BYTES = np.asarray([0, 255, 255, 0, 0, 0, 255, 128, 128, 255, 0, 255, 0, 128], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def export_input(shape):
    """fp32 [B,C,T,H,W], read-only: the 256 table values, the half-way points, out-of-range values, NaN and +-inf, then uniform
    draws in [-1.2, 1.2], shuffled over the tensor (every special value is present when the tensor has room, cycled in otherwise)."""
    rng = np.random.default_rng(2900 + int(np.prod(shape)))
    n = int(np.prod(shape))
    head = np.concatenate([SPECIAL, halfway()[0], unit_table()])
    if n <= head.size:
        flat = head[rng.permutation(head.size)[:n]]
    else:
        flat = np.concatenate([head, rng.uniform(-1.2, 1.2, n - head.size).astype(np.float32)])
        flat = flat[rng.permutation(n)]
    x = np.ascontiguousarray(flat.reshape(shape), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def nn_inputs(N, B, D):
    """(g [N, D], r [B, D]) fp32, read-only: the planted clips of the module docstring."""
    rng = np.random.default_rng(7100 + 977 * N + 31 * B + D % 9973)
    p = rng.standard_normal(D)
    g = (p + 1e-3 * rng.standard_normal((N, D))).astype(np.float32)
    nu = rng.standard_normal((B, D))
    nu *= np.sqrt(D) / np.linalg.norm(nu, axis=1, keepdims=True)
    s = 0.05 * 1.25 ** rng.permutation(B)
    r = (g[np.arange(B) % N].astype(np.float64) + s[:, None] * nu).astype(np.float32)
    g.setflags(write=False)
    r.setflags(write=False)
    return g, r


def d2_ref(g, r):
    """float64 [N, B]: sum_k (g[n,k] - r[j,k])^2 over the fp32 inputs, the differences exact."""
    g, r = np.asarray(g), np.asarray(r)
    out = np.empty((g.shape[0], r.shape[0]), dtype=np.float64)
    r64 = r.astype(np.float64)
    for n in range(g.shape[0]):
        d = r64 - g[n].astype(np.float64)
        out[n] = np.einsum('jk,jk->j', d, d)
    return out


@functools.lru_cache(maxsize=None)
def nn_reference(N, B, D):
    d2 = d2_ref(*nn_inputs(N, B, D))
    d2.setflags(write=False)
    return d2


def min_gap(d2):
    """The smallest relative gap between neighbours of any row's sorted distances (inf for one candidate)."""
    s = np.sort(np.asarray(d2, np.float64), axis=1)
    if s.shape[1] < 2:
        return np.inf
    return float(((s[:, 1:] - s[:, :-1]) / s[:, 1:]).min())


def empty_lists(N, K):
    return np.full((N, K), np.inf), np.full((N, K), -1, dtype=np.int64)


# ---- standing statistics: the CPU oracle generator driven the same way -------------------------------------------------------------
def standing_latents(nb=3, b=2, latent=256, seed=2919):
    import torch
    g = torch.Generator()
    g.manual_seed(seed)
    return [torch.randn(b, latent, generator=g) for _ in range(nb)]


def oracle_standing(zs, dtype=None):
    """{buffer name: tensor} of the oracle generator (recipe weights, num_channels=1, 64x64) after the batches `zs`: eval generator
    (full clips, every level rendered), training-mode BatchNorm with momentum 1/(k+1) at batch k — torch's momentum=None, whose
    factor is 1/num_batches_tracked. `oracle/` stays as it is: its BatchNorm is swapped for the duration of the call."""
    import torch
    import torch.nn.functional as F
    from oracle import tganv2_oracle as O
    P = O.recipe_state(O.gen_shapes(num_channels=1))
    if dtype is not None:
        P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    state = {'k': 0}

    def bn(P, q, x, training=True):
        return F.batch_norm(x, P[q + 'running_mean'], P[q + 'running_var'], P[q + 'weight'], P[q + 'bias'], True,
                            1.0 / (state['k'] + 1), 1e-5)
    keep = O.batchnorm_train
    O.batchnorm_train = bn
    try:
        with torch.no_grad():
            for k, z in enumerate(zs):
                state['k'] = k
                O.multiscale_gen(P, z if dtype is None else z.to(dtype), training=False, output_blocks=range(4))
    finally:
        O.batchnorm_train = keep
    return {k: v for k, v in P.items() if k.endswith('running_mean') or k.endswith('running_var')}
