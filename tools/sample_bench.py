"""Cost of the sampling tool's device passes (`python -m txt2vid_amd.gan.sample`), in one process and one session:
  1. clips/s of render + export at B clips (unconditional TGANv2 64x64x1, recipe weights, eval mode): the generator's forward, then
     A. `t2v_clip_export` into a device buffer and the bytes copied to a pinned buffer (what `--export` does), against
     B. the float clips copied to a pinned buffer and numpy's byte map on the host (`functional_sample.byte_map` + `export_rows`),
     alternated round by round; and the export kernel alone, with the bytes it moves per second. A and B give the same bytes.
  2. `t2v_clip_nn` per call at N = 64 samples, B real clips, D = 65536, against reading r once: a device-to-device copy of r
     (read + write: half its time is the read at the measured copy bandwidth), and torch's `cdist` on the same tensors as an
     outside figure (it uses the Gram form the kernel avoids).
  python tools/sample_bench.py [--batch 32] [--iters 10] [--rounds 5] [--out profiles/sample_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from txt2vid_amd.util.misc import limit_host_threads  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kid_bench import DEV, make, events_ms, stats  # noqa: E402  (the same models and timers as tools/kid_bench.py)


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd import functional_sample as FS
    from txt2vid_amd.gan import sample as S
    torch.manual_seed(0)
    B = a.batch
    gan = make()[0]
    out = {'workload': 'unconditional TGANv2 64x64x1, recipe weights, eval mode, B=%d clips of 16 frames per forward' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds}

    # ---- 1. render + export -----------------------------------------------------------------------------------------------------
    g_dev, g_host = S.generators(0, DEV)
    z = S.draw_latents(B, gan.gen.latent_size, g_dev, g_host, None, DEV)
    with S.sampling(gan):
        fake = S.forward(gan, z)[-1]
        _, C, T, H, W = [int(v) for v in fake.shape]
        dev_bytes = torch.empty((B * T, C * H * W), device=DEV, dtype=torch.uint8)
        pin_bytes = torch.empty((B * T, C * H * W), dtype=torch.uint8).pin_memory()
        pin_float = torch.empty(tuple(fake.shape), dtype=torch.float32).pin_memory()

        def render():
            return S.forward(gan, z)[-1]

        def path_a():
            FS.clip_export(render(), out=dev_bytes)
            pin_bytes.copy_(dev_bytes)
            return pin_bytes.numpy()

        def path_b():
            pin_float.copy_(render())
            return FS.export_rows(FS.byte_map(pin_float.numpy()))
        same = bool(np.array_equal(path_a(), path_b()))
        for f in (render, path_a, path_b):
            f()
        r_ms, a_ms, b_ms = [], [], []
        for _ in range(a.rounds):                            # alternate the variants: same machine state for all
            r_ms.append(wall_ms(render, a.iters))
            a_ms.append(wall_ms(path_a, a.iters))
            b_ms.append(wall_ms(path_b, a.iters))
        k_ms = [events_ms(lambda: FS.clip_export(fake, out=dev_bytes), 50) for _ in range(a.rounds)]
    med = lambda v: float(np.median(v))  # noqa: E731
    moved = fake.numel() * 5                                  # 4 bytes read, 1 written per element
    out['render_export'] = {'clips': B, 'render_ms': stats(r_ms), 'kernel_path_ms': stats(a_ms), 'numpy_path_ms': stats(b_ms),
                            'kernel_path_clips_per_s': B / (med(a_ms) * 1e-3), 'numpy_path_clips_per_s': B / (med(b_ms) * 1e-3),
                            'kernel_path_over_numpy_path': med(a_ms) / med(b_ms), 'same_bytes': same,
                            'export_kernel_ms': stats(k_ms), 'export_kernel_gb_per_s': moved / (med(k_ms) * 1e-3) / 1e9}

    # ---- 2. nearest real clips ----------------------------------------------------------------------------------------------------
    N, D, K = 64, C * T * H * W, 8
    gen = torch.Generator()
    gen.manual_seed(2)
    g = (torch.rand(N, D, generator=gen) * 2 - 1).to(DEV)
    r = (torch.rand(B, D, generator=gen) * 2 - 1).to(DEV)
    r2 = torch.empty_like(r)
    bd, bi = FS.nn_init(N, K, DEV)
    ws = torch.empty((int(FS.lib().t2v_clip_nn_ws_bytes(N, B, D)),), device=DEV, dtype=torch.uint8)
    FS.clip_nn(g, r, 0, bd, bi, ws=ws)
    ref = torch.cdist(g.double(), r.double()) ** 2
    want = ref.sort(dim=1)
    nn_ms = [events_ms(lambda: FS.clip_nn(g, r, 0, bd, bi, ws=ws), 50) for _ in range(a.rounds)]
    cp_ms = [events_ms(lambda: r2.copy_(r), 50) for _ in range(a.rounds)]
    cd_ms = [events_ms(lambda: torch.cdist(g, r), 50) for _ in range(a.rounds)]
    bd0, bi0 = FS.nn_init(N, K, DEV)
    FS.clip_nn(g, r, 0, bd0, bi0, ws=ws)
    rbytes = r.numel() * 4
    copy_bw = 2 * rbytes / (med(cp_ms) * 1e-3)                # a copy reads and writes
    out['clip_nn'] = {'N': N, 'B': B, 'D': D, 'K': K, 'chain': FS.nn_chain(D), 'slabs': FS.nn_slabs(D), 'ms': stats(nn_ms),
                      'r_bytes': rbytes, 'copy_r_ms': stats(cp_ms), 'copy_gb_per_s': copy_bw / 1e9,
                      'read_r_once_ms': rbytes / copy_bw * 1e3, 'kernel_over_read_r_once': med(nn_ms) / (rbytes / copy_bw * 1e3),
                      'pair_elements_per_s': N * B * D / (med(nn_ms) * 1e-3), 'torch_cdist_fp32_ms': stats(cd_ms),
                      'indices_equal_fp64_cdist': bool(torch.equal(bi0, want.indices[:, :K])),
                      'max_rel_diff_to_fp64_cdist': float(((bd0 - want.values[:, :K]).abs() / want.values[:, :K]).max()),
                      'gamma': FS.nn_gamma(D)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
