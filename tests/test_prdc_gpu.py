"""GPU: precision/recall and density/coverage of the evaluation (`--eval_prdc`; DESIGN "Precision/recall and density/coverage") on
the HIP path, against the float64 restatement of tests/prdc_cases.py: `t2v_knn_radii` at the derived bound and `t2v_prdc_counts`
exactly (test_prdc_cpu.py asserts the margin that allows it), on guarded buffers, their determinism and their independence of the
workspace's contents, the refusals, the evaluator's record against the restatement on its own banks, its isolation from the
training loop (bitwise), and the command line. The model helpers are test_kid_gpu.py's."""
import ctypes as C
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import prdc_cases as P
import test_kid_gpu as KG

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS, BLOCK, NEIGHBOURS = KG.CLIPS, KG.BLOCK, 3
NEW_KEYS = ['precision', 'recall', 'density', 'coverage', 'prdc_k']
KID_KEYS = ['iteration', 'kid', 'stderr', 'clips', 'block', 'alpha', 'net']
GUARD = 64                                                         # 8-byte words on each side of a guarded buffer
SENTINEL = 0x5A


# ------------------------------------------------------------------------------------------------ op level: guarded buffers

class Guarded(object):
    """`words` 8-byte words carved out of a larger allocation with GUARD sentinel words on each side; the inside starts as 0xFF
    bytes (a NaN as a double, -1 as an integer), so an element the kernels read without having written it shows."""

    def __init__(self, words, dtype):
        self.buf = torch.full(((words + 2 * GUARD) * 8,), SENTINEL, device=DEV, dtype=torch.uint8)
        self.bytes = self.buf[GUARD * 8:(GUARD + words) * 8]
        self.bytes.fill_(0xFF)
        self.t = self.bytes.view(dtype)

    def intact(self):
        return bool((self.buf[:GUARD * 8] == SENTINEL).all()) and bool((self.buf[GUARD * 8 + self.bytes.numel():] == SENTINEL).all())


def _ws_words(n, d, k):
    from txt2vid_amd._lib import lib
    a, b = lib().t2v_knn_radii_ws_bytes(n, d, k), lib().t2v_prdc_counts_ws_bytes(n, d, k)
    assert a > 0 and b > 0 and a % 8 == 0 and b % 8 == 0
    return a // 8, b // 8


def _run(case, ws_radii=None, ws_counts=None):
    """(rX, rY, counts, intact) of one case through the wrappers; outputs and (unless one is passed in) workspaces guarded and
    pre-filled with 0xFF bytes. The counts are fed the kernel's own radii."""
    from txt2vid_amd.functional_prdc import knn_radii_raw, prdc_counts_raw
    X, Y = P.inputs(case)
    n, d, k, _ = case
    Xd, Yd = torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(Y.copy()).to(DEV)
    wr, wc = _ws_words(n, d, k)
    guards = [Guarded(n, torch.float64), Guarded(n, torch.float64), Guarded(4, torch.int64)]
    rX, rY, cnt = guards
    ws = []
    for given, words in ((ws_radii, wr), (ws_radii, wr), (ws_counts, wc)):
        if given is None:
            guards.append(Guarded(words, torch.uint8))
            given = guards[-1].t
        ws.append(given)
    assert knn_radii_raw(Xd, k, out=rX.t, ws=ws[0]) is rX.t
    assert knn_radii_raw(Yd, k, out=rY.t, ws=ws[1]) is rY.t
    assert prdc_counts_raw(Xd, Yd, k, rX.t, rY.t, out=cnt.t, ws=ws[2]) is cnt.t
    torch.cuda.synchronize()
    same = torch.equal(Xd.cpu(), torch.from_numpy(X.copy())) and torch.equal(Yd.cpu(), torch.from_numpy(Y.copy()))
    return rX.t.cpu().numpy().copy(), rY.t.cpu().numpy().copy(), cnt.t.cpu().numpy().copy(), all(g.intact() for g in guards) and same


@pytest.mark.parametrize('case', P.CASES, ids=P.case_id)
def test_radii_within_the_derived_bound_and_counts_exact_on_guarded_buffers(case):
    X, Y = P.inputs(case)
    n, d, k, mode = case
    rX, rY, cnt, intact = _run(case)
    assert intact
    for got, U in ((rX, X), (rY, Y)):
        ratio = np.abs(got - P.radii(U, k)) / P.radius_bound(U)
        print('prdc-radius-ratio %s worst %.4g' % (P.case_id(case), ratio.max()))
        assert np.isfinite(got).all() and (got >= 0).all() and (ratio <= 1.0).all(), ratio.max()
    want = P.counts(X, Y, k)
    print('prdc-counts %s: %s (restatement %s)' % (P.case_id(case), cnt.tolist(), want))
    assert cnt.tolist() == want                                               # exactly: no decision sits inside the bound
    # two calls: the same bits
    rX2, rY2, cnt2, _ = _run(case)
    assert rX.tobytes() == rX2.tobytes() and rY.tobytes() == rY2.tobytes() and cnt.tobytes() == cnt2.tobytes()
    # one oversize workspace, shared by the three calls and used twice: first full of 0xFF bytes, then of what the last call left
    wr, wc = _ws_words(n, d, k)
    big = torch.full(((max(wr, wc) + 1000) * 8,), 0xFF, device=DEV, dtype=torch.uint8)
    for _ in range(2):
        a, b, c, ok = _run(case, ws_radii=big, ws_counts=big)
        assert ok and a.tobytes() == rX.tobytes() and b.tobytes() == rY.tobytes() and c.tobytes() == cnt.tobytes()
    if mode != 'shift':
        from txt2vid_amd.functional_prdc import estimate
        assert estimate(cnt.tolist(), n, k) == P.prdc(X, Y, k)
        p, r, dn, cv = estimate(cnt.tolist(), n, k)
        if mode == 'memo':
            assert (p, r, cv) == (1.0, 1.0, 1.0) and round(dn, 3) == 1.088
        else:                                                                 # every generated clip is real, one real clip is reached
            assert p == 1.0 and r == 1 / 130 and dn == 0.2 and cv == 1 / 130


def test_radii_do_not_depend_on_what_else_is_in_the_bank_order():
    """The k smallest of a multiset have no order: the bank with its rows reversed gives the reversed radii, bit for bit."""
    from txt2vid_amd.functional_prdc import knn_radii_raw
    X, _ = P.inputs((130, 37, 5, 'shift'))
    a = knn_radii_raw(torch.from_numpy(X.copy()).to(DEV), 5)
    b = knn_radii_raw(torch.from_numpy(X[::-1].copy()).to(DEV), 5)
    assert torch.equal(a, b.flip(0))


def test_wrappers_check_their_buffers():
    from txt2vid_amd.functional_prdc import knn_radii_raw, prdc_counts_raw
    X, Y = P.inputs((17, 33, 5, 'shift'))
    Xd, Yd = torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(Y.copy()).to(DEV)
    rX, rY = knn_radii_raw(Xd, 5), knn_radii_raw(Yd, 5)
    c = prdc_counts_raw(Xd, Yd, 5, rX, rY)
    assert rX.dtype == torch.float64 and tuple(rX.shape) == (17,) and c.dtype == torch.int64 and c.tolist() == P.counts(X, Y, 5)
    ws = torch.zeros(4096, device=DEV, dtype=torch.float64).view(torch.uint8)
    with pytest.raises(ValueError, match='workspace'):
        knn_radii_raw(Xd, 5, ws=ws[:64])
    with pytest.raises(ValueError, match='workspace'):
        prdc_counts_raw(Xd, Yd, 5, rX, rY, ws=ws[4:])
    with pytest.raises(ValueError, match='float64'):
        prdc_counts_raw(Xd, Yd, 5, rX.float(), rY)
    with pytest.raises(ValueError, match='float64'):
        knn_radii_raw(Xd, 5, out=torch.zeros(16, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='int64'):
        prdc_counts_raw(Xd, Yd, 5, rX, rY, out=torch.zeros(4, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match='PRDC'):
        knn_radii_raw(Xd, 17)
    with pytest.raises(ValueError, match='one shape'):
        prdc_counts_raw(Xd, Yd[:16], 5, rX, rY)


def test_entry_points_refuse_bad_arguments_launch_nothing_and_leave_the_output():
    from txt2vid_amd._lib import lib
    L = lib()
    buf = torch.full((8192,), 3.5, device=DEV, dtype=torch.float64)
    p = C.c_void_p(buf.data_ptr())
    for n, d, k, u, out, ws in ((1, 4, 1, p, p, p), (40, 0, 5, p, p, p), (40, 4, 0, p, p, p), (40, 4, 17, p, p, p), (5, 4, 5, p, p, p),
                                (40, 4, 5, None, p, p), (40, 4, 5, p, None, p), (40, 4, 5, p, p, None), (65536 * 64, 4, 5, p, p, p)):
        assert L.t2v_knn_radii(u, n, d, k, out, ws, None) == -1
        assert L.t2v_prdc_counts(u, p, n, d, k, p, p, out, ws, None) == -1
    for y, rx, ry in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.t2v_prdc_counts(p, y, 40, 4, 5, rx, ry, p, p, None) == -1
    torch.cuda.synchronize()
    assert bool((buf == 3.5).all())


# ------------------------------------------------------------------------------------------------ the evaluator

def _filled(prdc):
    gan = KG.make('uncond')[0]
    ev = KG.evaluator(gan, prdc=prdc)
    KG.seed(8)
    for _ in range(CLIPS // KG.B):
        ev.observe(KG.S.batch().to(DEV))
    assert ev.full
    return ev


def test_record_with_the_flag_is_the_restatement_on_the_banks_and_without_it_todays(monkeypatch):
    from txt2vid_amd import functional as TF
    off, on = _filled(0), _filled(NEIGHBOURS)
    recs, calls = {}, {}
    for name, ev in (('off', off), ('on', on)):
        ev.evaluate(1)                                                        # (warm: the eval-mode forwards pack their weights once)
        calls[name] = KG._trace(monkeypatch, lambda: recs.__setitem__(name, dict(ev.evaluate(2))))
    TF.set_grad_sink(None)
    new = ('t2v_knn_radii_ws_bytes', 't2v_knn_radii', 't2v_prdc_counts_ws_bytes', 't2v_prdc_counts')
    assert not set(new) & set(calls['off']) and calls['off'][-2:] == ['t2v_kid_sums_ws_bytes', 't2v_kid_sums']
    assert list(recs['off']) == KID_KEYS and not hasattr(off, 'rX') and not hasattr(off, 'prdc_ws')
    assert [c for c in calls['on'] if c not in new] == calls['off']          # today's calls, and behind them the new ones
    assert calls['on'][-4:] == list(new) and [c for c in calls['on'] if c in new] == list(new)
    rec = recs['on']
    assert list(rec) == KID_KEYS + NEW_KEYS and {k: rec[k] for k in KID_KEYS} == recs['off'] and rec['prdc_k'] == NEIGHBOURS
    X, Y = on.real_bank.cpu().numpy(), on.fake_bank.cpu().numpy()
    assert torch.equal(on.real_bank, off.real_bank) and torch.equal(on.fake_bank, off.fake_bank)
    m = P.margin(X, Y, NEIGHBOURS)
    want = P.prdc(X, Y, NEIGHBOURS)
    print('prdc evaluator: %s, restatement %s, margin %.3g' % ([rec[k] for k in NEW_KEYS[:4]], want, m))
    assert m >= 1e4                                                           # the banks decide nothing inside the bound
    assert (rec['precision'], rec['recall'], rec['density'], rec['coverage']) == want
    assert (np.abs(on.rX.cpu().numpy() - P.radii(X, NEIGHBOURS)) <= P.radius_bound(X)).all()
    assert (np.abs(on.rY.cpu().numpy() - P.radii(Y, NEIGHBOURS)) <= P.radius_bound(Y)).all()
    assert on.prdc_line(rec) == 'Iter 2, PRDC (k=3): precision %.3f, recall %.3f, density %.3f, coverage %.3f' % want
    # an untrained generator is far from the data (all four are 0): the same path with half of the generated bank replaced by
    # near-copies of half of the real clips, the other half left where it is
    h = CLIPS // 2
    monkeypatch.setattr(on, '_render', lambda: on.fake_bank[:h].copy_(on.real_bank[:h].roll(1, 0).mul(1.01)))
    rec = on.evaluate(3)
    Y = on.fake_bank.cpu().numpy()
    want = P.prdc(X, Y, NEIGHBOURS)
    print('prdc evaluator, half-copied bank: %s, restatement %s, margin %.3g' % ([rec[k] for k in NEW_KEYS[:4]], want, P.margin(X, Y, NEIGHBOURS)))
    assert P.margin(X, Y, NEIGHBOURS) >= 1e4 and (rec['precision'], rec['recall'], rec['density'], rec['coverage']) == want
    assert rec['precision'] == 0.5 and all(0 < rec[k] <= 1 for k in ('recall', 'coverage')) and 0 < rec['density']


_LOOPS = {}


def _loop_with_prdc(monkeypatch, kind, graph):
    """test_kid_gpu.loop with the evaluator built with prdc=NEIGHBOURS (not through its cache, which holds the flag-off runs)."""
    if (kind, graph) not in _LOOPS:
        plain = KG.evaluator
        with monkeypatch.context() as mp:
            mp.setattr(KG, 'evaluator', lambda gan, **kw: plain(gan, prdc=NEIGHBOURS, **kw))
            _LOOPS[(kind, graph)] = KG.loop.__wrapped__(kind, graph, True)
    return _LOOPS[(kind, graph)]


@pytest.mark.parametrize('kind,graph', [('cond', True), ('uncond', False)], ids=['cond-replayed', 'uncond-eager'])
def test_isolation_the_loop_computes_the_same_bits_with_and_without_eval_prdc(monkeypatch, kind, graph):
    off, off_recs, _, _ = KG.loop(kind, graph, True)                         # --eval_period alone
    on, recs, live, gan = _loop_with_prdc(monkeypatch, kind, graph)
    assert gan.kid.prdc == NEIGHBOURS and recs[0] is None and off_recs[0] is None and all(live)
    for a, b in zip(off_recs[1:], recs[1:]):
        assert list(b) == KID_KEYS + NEW_KEYS and {k: b[k] for k in KID_KEYS} == a
        assert all(0.0 <= b[k] <= 1.0 for k in ('precision', 'recall', 'coverage')) and 0.0 <= b['density'] and b['prdc_k'] == NEIGHBOURS
    print('prdc %s graph=%s: %s' % (kind, graph, [[r[k] for k in NEW_KEYS[:4]] for r in recs[1:]]))
    for (a, b), (c, d) in zip(off['losses'], on['losses']):
        assert torch.equal(a, c) and torch.equal(b, d)
    for part in ('G', 'D'):                                                   # parameters and BatchNorm buffers
        assert list(off[part]) == list(on[part])
        assert all(torch.equal(off[part][k], on[part][k]) for k in off[part]), part
    assert any('running_mean' in k for k in off['G'])
    assert torch.equal(off['rng'][0], on['rng'][0]) and np.array_equal(off['rng'][1], on['rng'][1]) and off['rng'][2] == on['rng'][2]


# ------------------------------------------------------------------------------------------------ command line

def test_cli_train_writes_the_extended_record_and_the_stand_alone_entry_prints_the_same_values(tmp_path):
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    base = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002',
            '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--gp_lambda', '.5',
            '--subsample_input', '--workers', '0', '--log_period', '1', '--dont_use_sent',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--batch_size', '8', '--epochs', '1', '--out', out_dir, '--out_samples', smp, '--save_example_period', '0']
    ev = ['--eval_clips', '8', '--eval_block', '4', '--eval_prdc', '3']
    log = KG._run('txt2vid_amd.train.gan', base + ['--max_iters', '2', '--save_model_period', '2', '--eval_period', '2'] + ev, tmp_path)
    assert 'Iter 2, KID: ' in log and 'Iter 2, PRDC (k=3): precision ' in log and 'k = 3 nearest neighbours among all 8 clips' in log
    assert log.index('Iter 2, KID: ') < log.index('Iter 2, PRDC (k=3)')
    with open(os.path.join(out_dir, 'metrics.jsonl')) as f:
        recs = [json.loads(l) for l in f]
    assert [r['iteration'] for r in recs] == [2] and list(recs[0]) == KID_KEYS + NEW_KEYS and recs[0]['prdc_k'] == 3
    assert all(isinstance(recs[0][k], float) and math.isfinite(recs[0][k]) and recs[0][k] >= 0 for k in NEW_KEYS[:4])
    assert all(recs[0][k] * 8 == round(recs[0][k] * 8) for k in ('precision', 'recall', 'coverage'))      # counts over 8 clips
    line = [l for l in log.splitlines() if 'PRDC (k=3)' in l][-1]
    assert line.endswith('precision %.3f, recall %.3f, density %.3f, coverage %.3f' % tuple(recs[0][k] for k in NEW_KEYS[:4]))
    ck = glob.glob(os.path.join(out_dir, 'iter_2_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert set(sd) == {'optG', 'optD', 'iteration', 'rng_state', 'gen', 'video'}                # nothing of the evaluator
    alone = KG._run('txt2vid_amd.gan.kid', base + ['--weights', ck[0]] + ev, tmp_path)
    rec = json.loads([l for l in alone.splitlines() if l.startswith('{')][-1])
    print('prdc cli: run %s, stand-alone %s' % (recs[0], rec))
    assert list(rec) == KID_KEYS + NEW_KEYS and rec['iteration'] == 2 and 'PRDC (k=3)' in alone
    assert [rec[k] for k in NEW_KEYS] == [recs[0][k] for k in NEW_KEYS]                         # the same four values (and k)
