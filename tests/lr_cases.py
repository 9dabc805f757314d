"""Float64 references of the learning-rate schedule (--lr_decay), shared by test_lr_sched_cpu.py and
test_lr_sched_gpu.py. Restated here from the definition, not imported from the package:

    frac   = clamp((it - S) / (T - S), 0, 1)          it: 0-based training iteration
    linear : factor = 1 - (1 - F) * frac
    cosine : factor = F + (1 - F) * 0.5 * (1 + cos(pi * frac))
    factor == 1 exactly while frac == 0, == F exactly once frac == 1

and the device-side bookkeeping: the optimiser's update k belongs to iteration k // spi."""
import numpy as np

KINDS = ('linear', 'cosine')
# the case the issue fixes: decay over iterations 2..5 down to a tenth
T, S, F = 5, 2, 0.1


def factor(kind, it, start=S, end=T, final=F):
    frac = min(max((np.float64(it) - start) / np.float64(end - start), 0.0), 1.0)
    if frac == 0.0:
        return 1.0
    if frac == 1.0:
        return float(final)
    if kind == 'linear':
        return float(1.0 - (1.0 - np.float64(final)) * frac)
    assert kind == 'cosine', kind
    return float(final + (1.0 - np.float64(final)) * 0.5 * (1.0 + np.cos(np.pi * frac)))


def update_factors(kind, spi, n, start=S, end=T, final=F):
    """The factor of each of an optimiser's first n updates: update k uses iteration k // spi."""
    return [factor(kind, k // spi, start, end, final) for k in range(n)]


def within_one_ulp(got, want64):
    """`got` (a float32 value) against np.float32 of the float64 reference: equal, or a neighbour."""
    w = np.float32(want64)
    g = np.float32(got)
    return bool(g == w or g == np.nextafter(w, np.float32(np.inf)) or g == np.nextafter(w, np.float32(-np.inf)))
