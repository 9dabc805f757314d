"""CPU: precision/recall and density/coverage of the evaluation (`--eval_prdc`; DESIGN "Precision/recall and density/coverage") —
the float64 restatement the GPU tests compare against (its definition, the margin condition that lets counts be demanded exactly,
a reordered evaluation against the derived bound), the host estimate, the host-side refusals of the two entry points, the flag's
rules, and the evaluator's record and log with the flag off and on (kernels stubbed by the restatement)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import prdc_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement

def test_restatement_equals_the_textbook_loops():
    rng = np.random.default_rng(9)
    X, Y, k, n = rng.standard_normal((7, 3)), rng.standard_normal((7, 3)) + 0.3, 2, 7
    dist = lambda u, v: sum((float(a) - float(b)) ** 2 for a, b in zip(u, v))
    rX = [sorted(dist(X[i], X[l]) for l in range(n) if l != i)[k - 1] for i in range(n)]
    rY = [sorted(dist(Y[i], Y[l]) for l in range(n) if l != i)[k - 1] for i in range(n)]
    c0 = sum(any(dist(X[i], Y[j]) <= rX[i] for i in range(n)) for j in range(n))
    c1 = sum(dist(X[i], Y[j]) <= rX[i] for i in range(n) for j in range(n))
    c2 = sum(any(dist(X[i], Y[j]) <= rY[j] for j in range(n)) for i in range(n))
    c3 = sum(min(dist(X[i], Y[j]) for j in range(n)) <= rX[i] for i in range(n))
    assert np.allclose(P.radii(X, k), rX, rtol=1e-14, atol=0) and np.allclose(P.radii(Y, k), rY, rtol=1e-14, atol=0)
    assert P.counts(X, Y, k) == [c0, c1, c2, c3]
    assert P.prdc(X, Y, k) == (c0 / n, c2 / n, c1 / (k * n), c3 / n)


def test_self_is_excluded_by_index_not_by_value():
    U = np.array([[0.0], [0.0], [3.0]], dtype=np.float32)                    # a duplicate: its first neighbour is at distance 0
    assert P.radii(U, 1).tolist() == [0.0, 0.0, 9.0] and P.radii(U, 2).tolist() == [9.0, 9.0, 9.0]


@pytest.mark.parametrize('case', P.CASES, ids=P.case_id)
def test_no_decision_of_a_case_sits_inside_the_bound(case):
    """The condition under which the GPU test may demand the counts exactly: every compared pair is 10⁴ bounds from its radius."""
    X, Y = P.inputs(case)
    m = P.margin(X, Y, case[2])
    print('prdc-margin %s: %.3g' % (P.case_id(case), m))
    assert m >= 1e4


@pytest.mark.parametrize('case', P.CASES, ids=P.case_id)
def test_a_reordered_gram_form_evaluation_stays_inside_the_bound_and_counts_the_same(case):
    """16x16 tiles, k in chunks of 4, clamp at 0: radii within the largest e of their row, the four counts equal."""
    X, Y = P.inputs(case)
    k = case[2]
    rX, rY, c = P.tiled(X, Y, k)
    worst = max(float((np.abs(rX - P.radii(X, k)) / P.radius_bound(X)).max()), float((np.abs(rY - P.radii(Y, k)) / P.radius_bound(Y)).max()))
    print('prdc-restatement tiled/plain %s worst radius ratio %.4g' % (P.case_id(case), worst))
    assert worst <= 1.0 and c == P.counts(X, Y, k)


def test_an_fp32_gram_form_misses_the_radius_bound():
    X, _ = P.inputs((130, 37, 5, 'memo'))
    g = X @ X.T
    n32 = (X * X).sum(1)
    D32 = np.maximum(np.float32(0), n32[:, None] + n32[None, :] - np.float32(2) * g).astype(np.float64)
    assert (np.abs(P.radii_of(D32, 5) - P.radii(X, 5)) / P.radius_bound(X)).max() > 100


def test_the_orientation_values_of_the_three_modes():
    """(130, 37, 5): an independent shifted normal, a generator that memorised the data, a generator with one mode."""
    got = {m: P.prdc(*P.inputs((130, 37, 5, m)), 5) for m in ('shift', 'memo', 'collapse')}
    print('prdc-orientation %s' % got)
    p, r, d, c = got['shift']
    assert (round(p, 3), round(r, 3), round(d, 3), round(c, 3)) == (0.723, 0.738, 0.711, 0.877)
    p, r, d, c = got['memo']
    assert (p, r, c) == (1.0, 1.0, 1.0) and round(d, 3) == 1.088
    p, r, d, c = got['collapse']
    assert p == 1.0 and round(r, 3) == 0.008 and round(d, 3) == 0.200 and round(c, 3) == 0.008


def test_host_estimate_against_hand_computed_counts():
    from txt2vid_amd.functional_prdc import estimate
    out = estimate([94, 462, 96, 114], 130, 5)
    assert out == (94 / 130, 96 / 130, 462 / 650, 114 / 130) and all(type(v) is float for v in out)
    assert estimate(torch.tensor([8, 24, 0, 8]).tolist(), 8, 3) == (1.0, 0.0, 1.0, 1.0)
    assert estimate([130, 707, 130, 130], 130, 5) == P.estimate([130, 707, 130, 130], 130, 5)


# ------------------------------------------------------------------------------------------------ the entry points, host side

def test_symbols_are_exported_declared_and_bound():
    from txt2vid_amd import _lib
    names = ['t2v_knn_radii', 't2v_knn_radii_ws_bytes', 't2v_prdc_counts', 't2v_prdc_counts_ws_bytes']
    header = open(os.path.join(ROOT, 'include', 't2v_hip.h')).read()
    assert [k for k in _lib.SIGNATURES if k.startswith(('t2v_knn_', 't2v_prdc_'))] == names
    assert 'int t2v_knn_radii(' in header and 'size_t t2v_knn_radii_ws_bytes(' in header and 'int t2v_prdc_counts(' in header
    assert 'size_t t2v_prdc_counts_ws_bytes(' in header and re.search(r'#define T2V_KNN_MAX_K 16\b', header)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    assert L.t2v_knn_radii_ws_bytes.restype is C.c_size_t and L.t2v_prdc_counts_ws_bytes.restype is C.c_size_t


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-side checks only: null pointers, n < 2, d < 1, k < 1, k > 16, k >= n, a tile grid beyond the launch limits; the
    workspace queries are 0 there."""
    from txt2vid_amd._lib import lib
    L = lib()
    p = C.c_void_p(64)                                               # never dereferenced: every call below is refused first
    ok = dict(U=p, X=p, Y=p, n=40, d=4, k=5, rX=p, rY=p, out=p, ws=p)
    big = 65536 * 64                                                 # ceil(n / 64) = 65536 tiles a side

    def radii(**kw):
        a = dict(ok, **kw)
        return L.t2v_knn_radii(a['U'], a['n'], a['d'], a['k'], a['out'], a['ws'], None)

    def counts(**kw):
        a = dict(ok, **kw)
        return L.t2v_prdc_counts(a['X'], a['Y'], a['n'], a['d'], a['k'], a['rX'], a['rY'], a['out'], a['ws'], None)
    sizes = (dict(n=1, k=1), dict(n=0), dict(n=-40), dict(d=0), dict(d=-1), dict(k=0), dict(k=-1), dict(k=17), dict(n=5, k=5), dict(n=5, k=6),
             dict(n=big))
    for bad in (dict(U=None), dict(out=None), dict(ws=None)) + sizes:
        assert radii(**bad) == -1, bad
    for bad in (dict(X=None), dict(Y=None), dict(rX=None), dict(rY=None), dict(out=None), dict(ws=None)) + sizes:
        assert counts(**bad) == -1, bad
    for a in sizes:
        a = dict(ok, **a)
        assert L.t2v_knn_radii_ws_bytes(a['n'], a['d'], a['k']) == 0 and L.t2v_prdc_counts_ws_bytes(a['n'], a['d'], a['k']) == 0, a
    # O(n · ceil(n / 64) · k): the norms and T·k values per row; two norm vectors, then a double and two ints per (row, tile)
    assert L.t2v_knn_radii_ws_bytes(40, 4, 5) == (40 + 1 * 5 * 40) * 8 and L.t2v_knn_radii_ws_bytes(130, 37, 16) == (130 + 3 * 16 * 130) * 8
    assert L.t2v_prdc_counts_ws_bytes(40, 4, 5) == 2 * 40 * 8 + 40 * 16 and L.t2v_prdc_counts_ws_bytes(130, 37, 16) == 2 * 130 * 8 + 3 * 130 * 16
    assert L.t2v_knn_radii_ws_bytes(2048, 1024, 5) == (2048 + 32 * 5 * 2048) * 8
    assert L.t2v_knn_radii_ws_bytes(big - 64, 4, 16) == (big - 64 + 65535 * 16 * (big - 64)) * 8          # the largest grid, no overflow


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from txt2vid_amd.functional_prdc import knn_radii_raw, prdc_counts_raw, check_sizes
    with pytest.raises(RuntimeError):
        knn_radii_raw(torch.zeros(4, 3), 2)
    with pytest.raises(RuntimeError):
        prdc_counts_raw(torch.zeros(4, 3), torch.zeros(4, 3), 2, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        knn_radii_raw(torch.zeros(4, 3, dtype=torch.float64), 2)
    for n, d, k in ((1, 4, 1), (8, 0, 3), (8, 4, 0), (8, 4, 8), (40, 4, 17), (8, 4, -1)):
        with pytest.raises(ValueError, match='PRDC'):
            check_sizes(n, d, k)
    check_sizes(2, 1, 1)
    check_sizes(17, 9, 16)


# ------------------------------------------------------------------------------------------------ flags

def _args(*extra):
    from txt2vid_amd.train.gan import build_parser
    return build_parser().parse_args(['--data', 'x', '--G', 'g', '--D', 'd'] + list(extra))


def test_flag_defaults_to_off_and_check_args_rules():
    from txt2vid_amd.gan import kid
    assert _args().eval_prdc == 0
    kid.check_args(_args())
    kid.check_args(_args('--eval_period', '5'), epoch_clips=lambda: 4096)
    a = _args('--eval_period', '5', '--eval_prdc', '5')
    kid.check_args(a, epoch_clips=lambda: 4096)
    assert a.eval_prdc == 5 and a.eval_block == 1024
    kid.check_args(_args('--eval_period', '2', '--eval_clips', '8', '--eval_prdc', '7'))          # K = M − 1
    kid.check_args(_args('--eval_period', '2', '--eval_clips', '32', '--eval_prdc', '16'))
    with pytest.raises(ValueError, match='needs --eval_period'):
        kid.check_args(_args('--eval_prdc', '5'))
    with pytest.raises(ValueError, match='--eval_prdc 8 needs more than 8 clips'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '8', '--eval_prdc', '8'))
    with pytest.raises(ValueError, match='--eval_prdc 12 needs more than 8 clips'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '8', '--eval_prdc', '12'))
    with pytest.raises(ValueError, match='from 1 to 16'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '64', '--eval_prdc', '17'))
    with pytest.raises(ValueError, match='from 1 to 16'):
        kid.check_args(_args('--eval_period', '2', '--eval_prdc', '-1'))
    with pytest.raises(ValueError, match='from 1 to 16'):
        kid.check_args(_args('--eval_prdc', '-3'))


# ------------------------------------------------------------------------------------------------ the evaluator's record and log

class _Gen(torch.nn.Module):
    latent_size = 4


class _Gan(object):
    gen = _Gen()


def _evaluator(monkeypatch, prdc, calls):
    """A KidEvaluator on the host whose kernels are stubbed: the KID sums by constants, the PRDC entry points by the restatement."""
    from txt2vid_amd.gan import kid
    n, d, k = 17, 1024, 5
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((n, d)).astype(np.float32), (rng.standard_normal((n, d)) + 0.05).astype(np.float32)

    def sums(real, fake, s, alpha, out=None, ws=None):
        calls.append('kid_sums')
        out.copy_(torch.tensor([[3.0 * s * (s - 1), 3.0 * s * (s - 1), 2.5 * s * s]], dtype=torch.float64))

    def radii(U, kk, out=None, ws=None):
        calls.append('knn_radii')
        out.copy_(torch.from_numpy(P.radii(U.numpy(), kk)))
        return out

    def counts(A, B, kk, rX, rY, out=None, ws=None):
        calls.append('prdc_counts')
        out.copy_(torch.tensor(P.counts(A.numpy(), B.numpy(), kk, rX.numpy(), rY.numpy())))
        return out
    monkeypatch.setattr(kid, 'kid_sums_raw', sums)
    monkeypatch.setattr(kid.FP, 'knn_radii_raw', radii)
    monkeypatch.setattr(kid.FP, 'prdc_counts_raw', counts)
    kw = {} if prdc is None else {'prdc': prdc}
    ev = kid.KidEvaluator(_Gan(), 'cpu', clips=n, block=n, num_channels=1, period=1, **kw)
    ev.real_bank.copy_(torch.from_numpy(X))
    ev.fake_bank.copy_(torch.from_numpy(Y))
    monkeypatch.setattr(ev, '_render', lambda: calls.append('render'))
    return ev, X, Y, k


def test_flag_off_the_record_the_log_and_the_buffers_are_todays(monkeypatch, capsys):
    for prdc in (None, 0):
        calls = []
        ev, X, Y, _ = _evaluator(monkeypatch, prdc, calls)
        assert ev.prdc == 0 and not any(hasattr(ev, a) for a in ('rX', 'rY', 'counts', 'prdc_ws'))
        ev.filled, ev.alpha = ev.M, 0.5
        rec = ev.step(4)
        assert list(rec) == ['iteration', 'kid', 'stderr', 'clips', 'block', 'alpha', 'net'] and calls == ['render', 'kid_sums']
        assert rec['kid'] == 1.0 and rec['stderr'] is None
        assert ev.log_line(rec) == 'Iter 4, KID: 1.00000 (17 clips in blocks of 17; features: %s)' % ev.net_name
        out = capsys.readouterr()
        assert 'PRDC' not in out.out + out.err


def test_flag_on_the_record_gains_five_keys_and_a_second_log_line(monkeypatch, capsys):
    calls, lines = [], []
    ev, X, Y, k = _evaluator(monkeypatch, 5, calls)
    from txt2vid_amd.gan import kid
    monkeypatch.setattr(kid, 'status', lambda s: lines.append(s))
    assert ev.prdc == 5 and ev.rX.dtype == torch.float64 and tuple(ev.counts.shape) == (4,) and ev.counts.dtype == torch.int64
    # the real bank's radii are computed once, when the bank fills (next to alpha)
    ev.filled = ev.M - 1
    monkeypatch.setattr(kid.TF, 'copy_into', lambda src, dst: dst.copy_(src))
    monkeypatch.setattr(kid.TF, 'row_sqnorm', lambda t: (t.double() ** 2).sum(1))
    monkeypatch.setattr(ev, 'features', lambda x: torch.from_numpy(X[-1:].copy()))
    ev.observe(torch.zeros(1, 1, 2, 2, 2))
    assert ev.full and calls == ['knn_radii'] and np.array_equal(ev.rX.numpy(), P.radii(X, k))
    rec = ev.step(6)
    assert calls == ['knn_radii', 'render', 'kid_sums', 'knn_radii', 'prdc_counts']
    assert list(rec) == ['iteration', 'kid', 'stderr', 'clips', 'block', 'alpha', 'net', 'precision', 'recall', 'density', 'coverage', 'prdc_k']
    assert (rec['precision'], rec['recall'], rec['density'], rec['coverage']) == P.prdc(X, Y, k) and rec['prdc_k'] == 5
    assert len(lines) == 2 and lines[0] == ev.log_line(rec)
    assert lines[1] == 'Iter 6, PRDC (k=5): precision %.3f, recall %.3f, density %.3f, coverage %.3f' % P.prdc(X, Y, k)
    assert re.fullmatch(r'Iter 6, PRDC \(k=5\): precision \d\.\d{3}, recall \d\.\d{3}, density \d\.\d{3}, coverage \d\.\d{3}', lines[1])
    with pytest.raises(ValueError, match='PRDC'):
        kid.KidEvaluator(_Gan(), 'cpu', clips=4, block=4, prdc=4)
