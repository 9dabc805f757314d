#!/usr/bin/env python
"""The CPU oracle's own rounding error on the LeCam state: `tests/lecam_cases.oracle_loop` in float32 against the same
loop in float64 on the same float32 weights and draws, over the four cases of
tests/test_lecam_gpu.py::test_iterations_vs_oracle_loop with that test's seed, lambda, decay and start. Needs no GPU.

Per D step it prints the largest gap of the anchors and the gap of R_last, absolute and relative to max(1, max |logit|) of the
step; then the largest relative gaps over all D steps behind the first. The anchors' figure is the test's ORACLE_GAP: run this
again when the seed or the recipe of that test changes.

  python tools/lecam_oracle_gap.py [--seed 145] [--iters 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))

import diffaug_cases as DA  # noqa: E402
import lecam_cases as LC  # noqa: E402
import schedule_cases as S  # noqa: E402

CASES = [(False, 1, 1), (False, 2, 1), (True, 1, 1), (True, 2, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=145)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--lam', type=float, default=0.3)
    ap.add_argument('--decay', type=float, default=0.5)
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    worst_a = worst_r = 0.0
    for cond, N, M in CASES:
        tokens = None
        if cond:
            tg = torch.Generator()                     # test_diffaug_gpu.tokens_for, restated
            tg.manual_seed(77)
            tokens = torch.randint(4, S.V, (S.B, 8), generator=tg)
            tokens[:, 0], tokens[:, -1] = 1, 2
        runs = [LC.oracle_loop(cond, N, M, DA.FULL, tokens=tokens, iters=args.iters, seed=args.seed, lam=args.lam,
                               decay=args.decay, start=0, dtype=dt) for dt in (torch.float32, torch.float64)]
        for k, (a, b) in enumerate(zip(runs[0]['state'], runs[1]['state'])):
            scale = max(1.0, runs[0]['scale'][k])
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            ga, gr = float(d[LC.A_R:].max()), float(d[1])
            print('%s %d:%d D step %d: max |logit| %.4g; anchors %.3g absolute, %.3g relative; R_last %.3g absolute, %.3g relative'
                  % ('cond' if cond else 'uncond', N, M, k, runs[0]['scale'][k], ga, ga / scale, gr, gr / scale))
            if k:
                worst_a, worst_r = max(worst_a, ga / scale), max(worst_r, gr / scale)
    print('behind the first D step, relative to max(1, max |logit|): anchors %.3g, R_last %.3g' % (worst_a, worst_r))


if __name__ == '__main__':
    main()
