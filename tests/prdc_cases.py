"""Float64 numpy restatement of improved precision/recall (Kynkäänniemi et al. 2019) and density/coverage (Naeem et al. 2020)
(`--eval_prdc`; DESIGN "Precision/recall and density/coverage"; not in the reference) and the op cases — shared by
test_prdc_cpu.py and test_prdc_gpu.py. No reference exists to record a fixture from, so this restatement is the yardstick.

One definition (include/t2v_hip.h). X (real) and Y (generated) are [n, d], 1 <= k <= 16, k < n. D2(u, v) = ‖u − v‖², here in the
DIRECT-DIFFERENCE form Σ_k (u_k − v_k)²: differences of fp32 values are exact in float64, so this D2 is exact to a few ulp.
rX[i] = the k-th smallest D2(x_i, x_l), l ≠ i (squared, self excluded by index), rY[j] likewise within Y, and

    c[0] = #{ j : ∃ i, D2(x_i, y_j) ≤ rX[i] }      c[1] = Σ_j #{ i : D2(x_i, y_j) ≤ rX[i] }
    c[2] = #{ i : ∃ j, D2(x_i, y_j) ≤ rY[j] }      c[3] = #{ i : min_j D2(x_i, y_j) ≤ rX[i] }
    precision = c0/n    density = c1/(k·n)    recall = c2/n    coverage = c3/n

Bound of the op (derived, not measured). A float64 GRAM-form D2 = max(0, ‖u‖² + ‖v‖² − 2 uᵀv) in any summation order stays within

    e(u, v) = 4·(d + 4)·2⁻⁵³·(‖u‖² + ‖v‖²)

of the exact value: three sums of d terms, each within d·2⁻⁵³ of its sum of magnitudes to first order, |uᵀv| ≤ Σ|u_k||v_k| ≤
(‖u‖² + ‖v‖²)/2, so the three shares add to 2·d·2⁻⁵³·(‖u‖² + ‖v‖²); the factor 2 and the +4 are headroom for the two additions,
the doubling and second-order terms; the clamp at 0 only moves towards the exact value, which is ≥ 0. A k-th order statistic is
1-Lipschitz in the sup norm, so a radius moves by at most the largest e of its row, and so does a row minimum.

A count can only be demanded EXACTLY if no decision sits inside the bound: `margin` is the smallest ratio of |D2 − r²| to the sum
of the two bounds over every compared pair of a case; test_prdc_cpu asserts it is ≥ 10⁴ on every case (it is ≥ 2·10⁶)."""
import functools

import numpy as np

MAX_K = 16
# (n, d, k): the smallest sizes at which a tile edge, the K-step remainder, the diagonal mask, k = n − 1, k at its maximum, a 3x3
# ragged tile grid or a row with more column tiles (18) than a small merge loop assumes can go wrong
SHIFT_CASES = [(2, 1, 1), (6, 5, 3), (17, 33, 5), (17, 9, 16), (64, 4, 1), (65, 70, 5), (130, 37, 5), (130, 37, 16), (1100, 8, 3)]
CASES = [c + ('shift',) for c in SHIFT_CASES] + [(130, 37, 5, 'memo'), (130, 37, 5, 'collapse')]
SHIFT = 0.3
NOISE = 1e-3
EPS = 2.0 ** -53


def case_id(case):
    return 'n%d-d%d-k%d-%s' % tuple(case)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(X, Y) of one case, fp32 [n, d]; X standard normal, drawn first; Y by the mode: `shift` an independent normal + 0.3, `memo`
    X + 1e-3·noise (a generator that memorised the data), `collapse` x_0 + 1e-3·noise (one mode). Seeded per (n, d, k), shared by
    every test, never modified (read-only arrays)."""
    n, d, k, mode = case
    rng = np.random.default_rng(5200 + 131 * n + 7 * d + k)
    X = rng.standard_normal((n, d)).astype(np.float32)
    if mode == 'shift':
        Y = rng.standard_normal((n, d)) + SHIFT
    elif mode == 'memo':
        Y = X + NOISE * rng.standard_normal((n, d))
    elif mode == 'collapse':
        Y = X[:1] + NOISE * rng.standard_normal((n, d))
    else:
        raise ValueError(mode)
    Y = Y.astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def d2(U, V):
    """‖u_i − v_j‖² for every pair, float64, direct differences (rows in slabs: no [n, n, d] array)."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    out = np.empty((U.shape[0], V.shape[0]))
    for i0 in range(0, U.shape[0], 128):
        diff = U[i0:i0 + 128, None, :] - V[None, :, :]
        out[i0:i0 + 128] = (diff * diff).sum(-1)
    return out


def radii_of(D, k):
    """The k-th smallest off-diagonal value of every row of a square distance matrix."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and 1 <= k <= MAX_K and k < n
    D[np.arange(n), np.arange(n)] = np.inf
    return np.sort(D, axis=1)[:, k - 1].copy()


def radii(U, k):
    return radii_of(d2(U, U), k)


def counts_of(Dxy, rX, rY):
    """The four integers from D2(X, Y) [n, n] and the two radius vectors."""
    inX = Dxy <= rX[:, None]                        # y_j inside the ball of x_i
    inY = Dxy <= rY[None, :]                        # x_i inside the ball of y_j
    return [int(inX.any(0).sum()), int(inX.sum()), int(inY.any(1).sum()), int((Dxy.min(1) <= rX).sum())]


def counts(X, Y, k, rX=None, rY=None):
    rX = radii(X, k) if rX is None else np.asarray(rX, dtype=np.float64)
    rY = radii(Y, k) if rY is None else np.asarray(rY, dtype=np.float64)
    return counts_of(d2(X, Y), rX, rY)


def estimate(c, n, k):
    """(precision, recall, density, coverage) in Python floats."""
    return int(c[0]) / n, int(c[2]) / n, int(c[1]) / (k * n), int(c[3]) / n


def prdc(X, Y, k):
    return estimate(counts(X, Y, k), np.asarray(X).shape[0], k)


def e_bound(U, V):
    """e(u_i, v_j) for every pair: what a float64 Gram-form D2 may differ by from the exact one."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    d = U.shape[1]
    return 4.0 * (d + 4) * EPS * ((U * U).sum(1)[:, None] + (V * V).sum(1)[None, :])


def radius_bound(U):
    """Per row, what a radius within U may move by: the largest e of the row (off the diagonal)."""
    E = e_bound(U, U)
    n = E.shape[0]
    E[np.arange(n), np.arange(n)] = 0.0
    return E.max(1)


def margin(X, Y, k):
    """The smallest |D2 − r²| / (bound of D2 + bound of r²) over every comparison the four counts make: each pair against rX[i],
    each pair against rY[j], each row minimum (bound: the largest e of the row) against rX[i]."""
    D, E = d2(X, Y), e_bound(X, Y)
    rX, rY, bX, bY = radii(X, k), radii(Y, k), radius_bound(X), radius_bound(Y)
    a = (np.abs(D - rX[:, None]) / (E + bX[:, None])).min()
    b = (np.abs(D - rY[None, :]) / (E + bY[None, :])).min()
    c = (np.abs(D.min(1) - rX) / (E.max(1) + bX)).min()
    return float(min(a, b, c))


def tiled_d2(U, V, tile=16, kc=4):
    """The Gram form in float64 in ANOTHER order — tile x tile tiles, dot products and norms accumulated over k in chunks of kc,
    clamped at 0: what a blocked kernel does."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    d = U.shape[1]
    nu, nv = np.zeros(U.shape[0]), np.zeros(V.shape[0])
    for k0 in range(0, d, kc):
        nu = nu + (U[:, k0:k0 + kc] ** 2).sum(1)
        nv = nv + (V[:, k0:k0 + kc] ** 2).sum(1)
    out = np.empty((U.shape[0], V.shape[0]))
    for i0 in range(0, U.shape[0], tile):
        for j0 in range(0, V.shape[0], tile):
            ui, vj = U[i0:i0 + tile], V[j0:j0 + tile]
            acc = np.zeros((ui.shape[0], vj.shape[0]))
            for k0 in range(0, d, kc):
                acc = acc + ui[:, k0:k0 + kc] @ vj[:, k0:k0 + kc].T
            out[i0:i0 + tile, j0:j0 + tile] = np.maximum(0.0, (nu[i0:i0 + tile, None] + nv[None, j0:j0 + tile]) - 2.0 * acc)
    return out


def tiled(X, Y, k):
    """(rX, rY, counts) from the reordered Gram-form evaluation, the counts with its own radii."""
    rX, rY = radii_of(tiled_d2(X, X), k), radii_of(tiled_d2(Y, Y), k)
    return rX, rY, counts_of(tiled_d2(X, Y), rX, rY)
