"""Float64 numpy restatement of the Kernel Inception Distance estimator (`--eval_period`; DESIGN "KID evaluation"; Bińkowski et
al. 2018; not in the reference) and the op cases — shared by test_kid_cpu.py and test_kid_gpu.py. No reference exists to record a
fixture from, so this restatement is the yardstick.

One definition. X (real) and Y (generated) are [n, d] feature matrices, s a block size with n % s == 0, nb = n / s; rows
[b·s, (b+1)·s) of X and of Y form block b. With k(u, v) = (alpha · uᵀv + 1)³

    S[b][0] = Σ_{i≠j in block b} k(x_i, x_j)      S[b][1] = Σ_{i≠j in block b} k(y_i, y_j)      S[b][2] = Σ_{i,j in block b} k(x_i, y_j)
    KID_b = S[b][0]/(s(s−1)) + S[b][1]/(s(s−1)) − 2·S[b][2]/s²        (the unbiased MMD² of the block)
    kid = mean_b KID_b        stderr = sample standard deviation of KID_b / √nb        (None for nb = 1)

Bound of the op (derived, not measured). Every summation order of a float64 dot product of length d followed by a sum of s² terms
stays within (d + s²)·2⁻⁵³ relative to the sum of magnitudes, to first order, and the cube triples the dot's share:

    |S − S_ref| ≤ 8·(d + s²)·2⁻⁵³ · Σ (alpha·|u_i|ᵀ|v_j| + 1)³       over the index pairs of that sum

(8 = 3 for the cube plus headroom for the alpha multiply and the +1). A float64 evaluation in another order — 16x16 tiles, k in
chunks of 4, test_kid_cpu — lies a few per cent of the way to it; anything computed in fp32 misses it by orders of magnitude."""
import functools
import math

import numpy as np

# (s, d, nb): the smallest sizes at which a tile edge, the K-step remainder, the diagonal mask or a block boundary can go wrong
CASES = [(2, 1, 1), (3, 5, 2), (16, 4, 1), (17, 33, 3), (33, 70, 2), (64, 257, 1)]
# (s, d, nb, alpha): kernel arguments alpha·uᵀv + 1 from about −20 to +20 — cubes of both signs that cancel in the sums
LARGE_ALPHA = (17, 33, 3, 1.0)
# beyond one 64x64 tile of the kernel: 3x3 ragged tiles (the mirrored tiles of the symmetric Grams count twice, the ones below the
# diagonal not at all), and more tiles than the reduce kernel has threads (18x18 > 256)
TILED = [(130, 37, 2), (1100, 8, 1)]
SHIFT = 0.3


def case_id(case):
    return 's%d-d%d-nb%d' % tuple(case[:3]) + ('-alpha%g' % case[3] if len(case) > 3 else '')


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(X, Y, alpha) of one case: fp32 standard normals [nb·s, d], Y shifted by 0.3; alpha = 1/d unless the case names one.
    Seeded per case, shared by every test, never modified (read-only arrays)."""
    s, d, nb = case[:3]
    rng = np.random.default_rng(4100 + 131 * s + 7 * d + nb + (1 if len(case) > 3 else 0))
    X = rng.standard_normal((nb * s, d)).astype(np.float32)
    Y = (rng.standard_normal((nb * s, d)) + SHIFT).astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, (float(case[3]) if len(case) > 3 else 1.0 / d)


def gram(U, V, alpha):
    """k(u_i, v_j) for every pair, float64."""
    return (alpha * (U.astype(np.float64) @ V.astype(np.float64).T) + 1.0) ** 3


def _three(X, Y, s, alpha, absolute):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = X.shape[0]
    assert X.shape == Y.shape and s >= 2 and n % s == 0
    if absolute:
        X, Y, alpha = np.abs(X), np.abs(Y), abs(alpha)
    out = np.zeros((n // s, 3))
    for b in range(n // s):
        x, y = X[b * s:(b + 1) * s], Y[b * s:(b + 1) * s]
        kxx, kyy, kxy = gram(x, x, alpha), gram(y, y, alpha), gram(x, y, alpha)
        out[b] = (kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum())
    return out


def sums(X, Y, s, alpha):
    """S [nb, 3] as defined above."""
    return _three(X, Y, s, alpha, False)


def magnitudes(X, Y, s, alpha):
    """Σ (alpha·|u_i|ᵀ|v_j| + 1)³ over the index pairs of each of the three sums of each block: [nb, 3]."""
    return _three(X, Y, s, alpha, True)


def op_bound(d, s):
    return 8.0 * (d + s * s) * 2.0 ** -53


def block_kids(S, s):
    return [float(r[0]) / (s * (s - 1)) + float(r[1]) / (s * (s - 1)) - 2.0 * float(r[2]) / (s * s) for r in S]


def estimate(S, s):
    """(kid, stderr or None) from the sums of every block, in Python floats."""
    ks = block_kids(S, s)
    nb = len(ks)
    kid = sum(ks) / nb
    if nb < 2:
        return kid, None
    var = sum((k - kid) ** 2 for k in ks) / (nb - 1)
    return kid, math.sqrt(var) / math.sqrt(nb)


def estimate_bound(X, Y, s, alpha):
    """What the op bound allows `kid` to move by: the three sums' bounds through the three divisions, averaged over the blocks."""
    d = np.asarray(X).shape[1]
    M = magnitudes(X, Y, s, alpha)
    per = op_bound(d, s) * (M[:, 0] / (s * (s - 1)) + M[:, 1] / (s * (s - 1)) + 2.0 * M[:, 2] / (s * s))
    return float(per.mean())


def kid(X, Y, s, alpha):
    return estimate(sums(X, Y, s, alpha), s)


def default_alpha(X):
    """1 / mean_i ‖x_i‖² over the real features: the kernel's argument is O(1) whatever the feature network's scale."""
    X = np.asarray(X, dtype=np.float64)
    return 1.0 / float((X * X).sum(1).mean())


def tiled_sums(X, Y, s, alpha, tile=16, kc=4):
    """The same sums in float64 in ANOTHER order: tile x tile tiles, dot products accumulated over k in chunks of kc, tiles added
    row-major — what a blocked kernel does; against `sums` it shows how far inside the bound a reordering stays."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n, d = X.shape
    out = np.zeros((n // s, 3))
    for b in range(n // s):
        x, y = X[b * s:(b + 1) * s], Y[b * s:(b + 1) * s]
        for g, (u, v) in enumerate(((x, x), (y, y), (x, y))):
            tot = 0.0
            for i0 in range(0, s, tile):
                for j0 in range(0, s, tile):
                    ui, vj = u[i0:i0 + tile], v[j0:j0 + tile]
                    acc = np.zeros((ui.shape[0], vj.shape[0]))
                    for k0 in range(0, d, kc):
                        acc = acc + ui[:, k0:k0 + kc] @ vj[:, k0:k0 + kc].T
                    k3 = (alpha * acc + 1.0) ** 3
                    if g < 2 and i0 == j0:
                        k3 = k3 - np.diag(np.diag(k3))
                    tot += float(k3.sum())
            out[b, g] = tot
    return out
