"""Cost of the opt-in spectral normalisation of the discriminator (--D_sn): unconditional TGANv2 64x64x1, B frames,
recipe weights, Adam, RSGAN + GP 0.5 (bench.py's workload), the whole iteration graph-replayed —
  * median ms per iteration without and with `SpectralNorm`, the two alternated block by block, and the launches one
    discriminator update adds;
  * the refresh and the projection on their own (back-to-back calls) with the bytes each must move at least: refresh reads W for
    the column pass, the row pass and the scaling and writes W and What (20 B per weight element); the projection reads G and What
    for the inner product, then G and W, and writes G and the parameter (24 B per element).
Back-to-back launches over a working set near the 256 MB Infinity Cache flatter a streaming kernel; the in-iteration overhead is
the figure that counts.
  python tools/sn_bench.py [--batch 32] [--iters 20] [--rounds 5] [--out result.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from txt2vid_amd.util.misc import limit_host_threads  # noqa: E402
from steps_bench import make, events_ms  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd.gan.spectral import SpectralNorm, attach
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    runs, parts = {}, {}
    for name in ('off', 'on'):
        gan, optD, optG, losses, prm = make(1, 1, 'rsgan', 0.5)
        if name == 'on':
            attach(gan, optD, SpectralNorm(gan.discrims))
        gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=3)
        for _ in range(5):                                  # 3 eager + capture + replays: every shape warm
            gs.step(x)
        torch.cuda.synchronize()
        runs[name], parts[name] = gs, gan
    res = {n: [] for n in runs}
    for _ in range(a.rounds):                               # alternate: same machine state for both
        for n, gs in runs.items():
            res[n].append(events_ms(lambda: gs.step(x), a.iters))
    sn = parts['on'].discrim_sn
    elements = sum(int(p.numel()) for p in sn.params)

    def pair():                # project (weight <- W) then refresh (weight <- W / sigma): the state the graphs read stays valid
        sn.project_grads()
        sn.refresh()

    def project_alone():       # (restores W into the parameters; `pair` below puts What back before anything else runs)
        sn.project_grads()
    for _ in range(5):
        pair()
    torch.cuda.synchronize()
    both, proj = [], []
    for _ in range(a.rounds):
        both.append(events_ms(pair, 100))
        proj.append(events_ms(project_alone, 100))
        pair()
    torch.cuda.synchronize()
    med = {n: float(np.median(v)) for n, v in res.items()}
    both_ms, proj_ms = float(np.median(both)), float(np.median(proj))
    refresh_ms = both_ms - proj_ms
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam, RSGAN + GP 0.5; the whole iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds,
           'graph_replayed': all(gs.graphs is not None for gs in runs.values()),
           'iter_ms': {n: {'median': med[n], 'min': float(min(v)), 'max': float(max(v))} for n, v in res.items()},
           'sn_overhead_ms': med['on'] - med['off'], 'sn_overhead_pct': 100.0 * (med['on'] - med['off']) / med['off'],
           'layers': len(sn.params), 'weight_elements': elements, 'launches_added_per_d_update': sn.launches_per_update,
           'project': {'ms': proj_ms, 'bytes': 24 * elements, 'GBps': 24e-6 * elements / proj_ms, 'launches': 3,
                       'timing': '100 back-to-back calls per round'},
           'refresh': {'ms': refresh_ms, 'bytes': 20 * elements, 'GBps': 20e-6 * elements / max(refresh_ms, 1e-9),
                       'launches': 5 * sn.n_iter + 1, 'timing': '(project + refresh) minus project, 100 back-to-back calls per round'},
           'sigma_min_max': [min(sn.sigmas().values()), max(sn.sigmas().values())]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
