"""Cost of precision/recall and density/coverage in the KID evaluation (`--eval_prdc`), in one process and one session:
  1. median ms per graph-replayed training iteration (unconditional TGANv2 64x64x1, B clips, recipe weights, RSGAN + GP 0.5, Adam,
     fp32) with `--eval_period` off / on with `--eval_prdc K` / off, alternated block by block. `on` is what train() runs on an
     iteration that is not an evaluation iteration with a full real bank. The two `off` variants are the same program built twice,
     so their difference is the spread the added time has to be read against.
  2. `t2v_knn_radii` and `t2v_prdc_counts` alone at (n, d, k) = (M, 1024, K) on the evaluator's banks, and as the yardstick the same
     quantities in torch on the same tensors: the fp64 Gram form (`X.double() @ X.double().T`, norms, clamp), `kthvalue`, and the
     comparisons and reductions of the four counts. Their agreement: the largest relative difference of a radius, the counts.
  3. one evaluation with the flag: its wall time, and the new work in it (the generated bank's radii and the counts; the real
     bank's radii are computed once, when the bank fills) as a share of the evaluation `profiles/kid_bench.json` records, next to
     the KID kernel's own time from the same file.
  python tools/prdc_bench.py [--batch 32] [--clips 2048] [--k 5] [--iters 20] [--rounds 5] [--out profiles/prdc_bench.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from txt2vid_amd.util.misc import limit_host_threads  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kid_bench import DEV, Prm, make, events_ms, stats  # noqa: E402  (the same workload and timers as tools/kid_bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--clips', type=int, default=2048)
    ap.add_argument('--block', type=int, default=1024)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd import functional as TF
    from txt2vid_amd.functional_prdc import knn_radii_raw, prdc_counts_raw
    from txt2vid_amd.gan.kid import KidEvaluator
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B, M, S, K = a.batch, a.clips, a.block, a.k
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, RSGAN + GP 0.5, Adam, fp32; the whole iteration graph-replayed; KID with %d '
                       'clips in blocks of %d and precision/recall/density/coverage with k = %d on the random-init feature network'
                       % (B, M, S, K),
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds, 'clips': M, 'block': S, 'k': K}

    # ---- 1. the iteration, flag off / on / off ---------------------------------------------------------------------------------
    runs = {}
    for name in ('off_a', 'on', 'off_b'):
        gan, optD, optG, losses = make()
        kid = None
        if name == 'on':
            kid = gan.kid = KidEvaluator(gan, DEV, clips=M, block=S, num_channels=1, period=10 ** 9, sample_batch=B, prdc=K)
            t0 = time.perf_counter()
            while not kid.full:                              # distinct clips: a new draw per batch
                kid.observe((torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV))
            torch.cuda.synchronize()
            out['fill_real_bank_s'] = time.perf_counter() - t0
        gs = GraphedTrainStep(gan, optD, optG, losses, Prm(), DEV, (B, 1, 16, 64, 64), warmup=3, cond_dim=0)
        for _ in range(5):                                   # 3 eager + capture + replays: every shape warm
            gs.step(x, None)
        torch.cuda.synchronize()
        runs[name] = (gs, kid)

    def body(gs, kid):
        def f():
            if kid is not None and not kid.full:
                kid.observe(x, None)
            gs.step(x, None)
            if kid is not None:
                kid.step(1)
        return f
    res = {k: [] for k in runs}
    for _ in range(a.rounds):                                # alternate the variants: same machine state for all
        for k, (gs, kid) in runs.items():
            res[k].append(events_ms(body(gs, kid), a.iters))
    for k, v in res.items():
        out['iter_%s' % k] = {'iter_ms': stats(v), 'graph_replayed': runs[k][0].graphs is not None}
    med = {k: out['iter_%s' % k]['iter_ms']['median'] for k in res}
    out['off_spread_ms'] = abs(med['off_a'] - med['off_b'])
    out['flag_cost_ms'] = med['on'] - 0.5 * (med['off_a'] + med['off_b'])

    # ---- 2. the two entry points alone against torch ---------------------------------------------------------------------------
    gs, kid = runs['on']
    kid.evaluate(0)                                          # warm: every shape of the eval-mode forwards; fills the generated bank
    torch.cuda.synchronize()
    X, Y, ws = kid.real_bank, kid.fake_bank, kid.prdc_ws
    n, d = X.shape
    rX, rY, cnt = kid.rX.clone(), kid.rY.clone(), kid.counts.clone()
    inf = float('inf')

    def gram_d2(U, V):
        Ud, Vd = U.double(), V.double()
        return ((Ud * Ud).sum(1)[:, None] + (Vd * Vd).sum(1)[None, :] - 2.0 * (Ud @ Vd.T)).clamp_min_(0.0)

    def torch_radii(U):
        D = gram_d2(U, U)
        D.fill_diagonal_(inf)
        return D.kthvalue(K, dim=1).values

    def torch_counts_of(A, Bm, rx, ry):
        D = gram_d2(A, Bm)
        inX, inY = D <= rx[:, None], D <= ry[None, :]
        return torch.stack([inX.any(0).sum(), inX.sum(), inY.any(1).sum(), (D.min(1).values <= rx).sum()])

    def torch_counts(rx, ry):
        return torch_counts_of(X, Y, rx, ry)
    tX, tY = torch_radii(X), torch_radii(Y)
    tC = torch_counts(rX, rY)
    torch.cuda.synchronize()
    radii_ms = [events_ms(lambda: knn_radii_raw(Y, K, out=rY, ws=ws), 10) for _ in range(a.rounds)]
    counts_ms = [events_ms(lambda: prdc_counts_raw(X, Y, K, rX, rY, out=cnt, ws=ws), 10) for _ in range(a.rounds)]
    t_radii_ms = [events_ms(lambda: torch_radii(Y), 10) for _ in range(a.rounds)]
    t_counts_ms = [events_ms(lambda: torch_counts(rX, rY), 10) for _ in range(a.rounds)]
    r_ms, c_ms, tr_ms, tc_ms = (float(np.median(v)) for v in (radii_ms, counts_ms, t_radii_ms, t_counts_ms))
    flop = 2.0 * n * n * d                                   # one n x n x d product each
    out['knn_radii'] = {'n': n, 'd': d, 'k': K, 'ms': stats(radii_ms), 'nominal_tflops': flop / (r_ms * 1e-3) / 1e12,
                        'torch_fp64_ms': stats(t_radii_ms), 'kernel_over_torch': r_ms / tr_ms,
                        'max_rel_diff_to_torch': float(max(((rX - tX).abs() / tX).max(), ((rY - tY).abs() / tY).max())),
                        'ws_bytes': int(TF.lib().t2v_knn_radii_ws_bytes(n, d, K))}
    out['prdc_counts'] = {'n': n, 'd': d, 'k': K, 'ms': stats(counts_ms), 'nominal_tflops': flop / (c_ms * 1e-3) / 1e12,
                          'torch_fp64_ms': stats(t_counts_ms), 'kernel_over_torch': c_ms / tc_ms, 'counts': cnt.tolist(),
                          'torch_counts': tC.tolist(), 'counts_equal_torch': cnt.tolist() == tC.tolist(),
                          'ws_bytes': int(TF.lib().t2v_prdc_counts_ws_bytes(n, d, K))}

    # an untrained generator is far from the data (all counts 0): the agreement once more with half of the generated bank replaced by
    # near-copies of real clips, where every count is in play
    Ym = Y.clone()
    Ym[:n // 2] = X[:n // 2].roll(1, 0) * 1.01
    rYm = knn_radii_raw(Ym, K)
    out['prdc_counts'].update({'half_copied_counts': prdc_counts_raw(X, Ym, K, rX, rYm).tolist(),
                               'half_copied_torch_counts': torch_counts_of(X, Ym, rX, rYm).tolist()})
    out['prdc_counts']['half_copied_equal_torch'] = out['prdc_counts']['half_copied_counts'] == out['prdc_counts']['half_copied_torch_counts']

    # ---- 3. one evaluation with the flag ----------------------------------------------------------------------------------------
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        rec = kid.evaluate(0)
        walls.append((time.perf_counter() - t0) * 1e3)
    new_ms = r_ms + c_ms
    ev = {'wall_ms': stats(walls), 'new_work_ms': new_ms, 'real_radii_once_ms': r_ms,
          'record': {k: rec[k] for k in ('kid', 'stderr', 'precision', 'recall', 'density', 'coverage', 'prdc_k')}}
    kb = os.path.join(ROOT, 'profiles', 'kid_bench.json')
    if os.path.exists(kb):
        with open(kb) as f:
            ref = json.loads(f.readline())
        base, sums = ref['evaluation']['wall_ms']['median'], ref['kid_sums']['ms']['median']
        ev.update({'kid_bench_evaluation_ms': base, 'new_work_over_kid_bench_evaluation': new_ms / base, 'kid_bench_kid_sums_ms': sums,
                   'new_work_over_kid_sums': new_ms / sums, 'knn_radii_over_kid_sums': r_ms / sums, 'prdc_counts_over_kid_sums': c_ms / sums})
    out['evaluation'] = ev
    TF.set_grad_sink(None)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
