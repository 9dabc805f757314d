"""Float64 reference of the spectral normalisation (txt2vid_amd/gan/spectral.py), the op-level shapes and the error
bounds the GPU tests assert. Pure torch on the CPU; imported by test_sn_cpu.py and test_sn_gpu.py.

    refresh:  t = W^T u ; v = t / max(|t|, eps) ; s = W v ; u = s / max(|s|, eps) ; sigma = u . s ; What = W / sigma
    backward: c = <G, What> ; dL/dW = (G - c u v^T) / sigma

Error model (E = 2^-24, the unit roundoff of fp32): a sum of n products, in any order and with or without fused multiply-adds, is
within g(n) sum |a_i| |b_i| of the exact one, g(n) = n E / (1 - n E); a Euclidean norm of n numbers is within (n + 2) E relative;
every further multiply, subtract or divide adds one relative rounding E."""
import torch

EPS = 1e-12
E = 2.0 ** -24

# [M, K] of one job: the smallest that reach every path of the kernels (column pass: 1024-column tiles, 32-row slices, 16-byte
# path iff K % 4 == 0 and aligned; row pass: one workgroup per row from K = 512, else one wave per row; 4096-element chunks)
SHAPES = [(1, 1), (1, 1031), (64, 27), (8, 81), (67, 129), (96, 2600), (260, 6912)]


def g(n):
    return n * E / (1.0 - n * E)


def make_case(M, K, seed):
    """fp32 (W, u, G): W ~ N(0, 1) / sqrt(K), u a unit vector, G ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(M, K, generator=gen) / K ** 0.5).float()
    u = torch.randn(M, generator=gen).float()
    u = u / max(float(u.norm()), EPS)
    G = torch.randn(M, K, generator=gen).float()
    return W, u, G


def low_rank_case(M, K, seed):
    """W = 3 a b^T + noise with unit a, b: sigma_1 ~ 3 and sigma_2 <= sigma_1 / 2 (asserted by the tests that use it)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(M, generator=gen, dtype=torch.float64)
    b = torch.randn(K, generator=gen, dtype=torch.float64)
    a, b = a / a.norm(), b / b.norm()
    noise = torch.randn(M, K, generator=gen, dtype=torch.float64) * (0.5 / (M ** 0.5 + K ** 0.5))
    W = (3.0 * torch.outer(a, b) + noise).float()
    u = torch.randn(M, generator=gen).float()
    return W, u / max(float(u.norm()), EPS)


def refresh_ref(W, u, eps=EPS, n_iter=1):
    """(v, u, sigma, What) after `n_iter` power iterations, in float64 on the given values. sigma == 0 divides by 1."""
    W, u = W.double().reshape(W.shape[0], -1), u.double()
    for _ in range(n_iter):
        t = W.t() @ u
        v = t / max(float(t.norm()), eps)
        s = W @ v
        u = s / max(float(s.norm()), eps)
        sigma = float(u @ s)
    return v, u, sigma, W / (sigma if sigma != 0.0 else 1.0)


def project_ref(G, What, u, v, sigma):
    """dL/dW from G = dL/dWhat, float64."""
    G2, Wh = G.double().reshape(G.shape[0], -1), What.double().reshape(G.shape[0], -1)
    c = float((G2 * Wh).sum())
    return ((G2 - c * torch.outer(u.double(), v.double())) / (sigma if sigma != 0.0 else 1.0)).reshape(G.shape)


def sn_weight(W, u, v):
    """What as a differentiable function of W with u, v constants (torch.nn.utils.spectral_norm's forward): autograd through
    this gives the gradient `project_ref` states in closed form."""
    sigma = torch.dot(u, W.reshape(W.shape[0], -1) @ v)
    return W / sigma


# ---- per-phase references with bounds: every phase takes the kernel's own fp32 inputs of that phase -----------------------------
def _unit_bound(x, ex, n_norm):
    """y = x / |x| computed as fl(xh / dh), |xh - x| <= ex elementwise, dh = the fp32 norm of xh ((n_norm + 2) E relative):
    returns (y, elementwise bound on |yh - y|). |x| > 0."""
    nx = float(x.norm())
    e_x = float(ex.norm())                                   # | |xh| - |x| | <= |xh - x|_2 <= |ex|_2
    th = (n_norm + 2) * E
    dlo = (nx - e_x) * (1.0 - th)
    assert dlo > 0, 'the case is too ill-conditioned for a bound (|x| = %g, error %g)' % (nx, e_x)
    e_d = e_x + th * (nx + e_x)
    y = x / nx
    b0 = ex / dlo + x.abs() * e_d / (dlo * nx)
    return y, b0 + E * (y.abs() + b0)


def phase_v(W, u):
    """v from (W, u): t_k sums M products; then the norm over K and one division."""
    W, u = W.double(), u.double()
    t = W.t() @ u
    et = g(W.shape[0]) * (W.abs().t() @ u.abs())
    return _unit_bound(t, et, W.shape[1])


def phase_u_sigma(W, v):
    """(u, bound, sigma, bound) from (W, the kernel's v): s_m sums K products; the norm over M and one division; sigma = u . s
    sums M products of the computed u and s."""
    W, v = W.double(), v.double()
    M, K = W.shape
    s = W @ v
    es = g(K) * (W.abs() @ v.abs())
    u, bu = _unit_bound(s, es, M)
    sigma = float(s.norm())                                  # u . s = |s| exactly
    uh = u.abs() + bu
    bs = float((uh * es + s.abs() * bu).sum() + g(M) * (uh * (s.abs() + es)).sum())
    return u, bu, sigma, bs


def phase_scale(W, sigma):
    """What = W / sigma: one rounding."""
    ref = W.double() / (float(sigma) if float(sigma) != 0.0 else 1.0)
    return ref, E * ref.abs()


def phase_project(G, What, u, v, sigma):
    """(G - c u v^T) / sigma from the kernel's own fp32 What, u, v, sigma: c sums M K products; x = u_m v_k, c x, the subtraction
    and the division add one rounding each."""
    G, Wh, u, v = G.double(), What.double(), u.double(), v.double()
    n = G.numel()
    c = float((G * Wh).sum())
    ec = g(n) * float((G.abs() * Wh.abs()).sum())
    x = torch.outer(u, v).abs()
    ep = x * (ec * (1 + E) ** 2 + abs(c) * ((1 + E) ** 2 - 1))
    d = G - c * torch.outer(u, v)
    e_d = ep + E * (d.abs() + ep)
    sg = float(sigma) if float(sigma) != 0.0 else 1.0
    ref = d / sg
    return ref, e_d / sg + E * (ref.abs() + e_d / sg)


# ---- the whole discriminator step, for the model-level tests -------------------------------------------------------------------
def normalised_param_dict(params, state, names):
    """{key: tensor} for the oracle: every weight in `names` (keys of `params`) replaced by `sn_weight(W, u, v)` built from the
    leaves in `state` ({name: (W, u, v)}); the leaves' `.grad` then are dL/dW."""
    out = dict(params)
    for k in names:
        W, u, v = state[k]
        out[k] = sn_weight(W, u, v)
    return out
