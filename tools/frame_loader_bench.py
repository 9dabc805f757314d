"""What the HBM frame cache buys on real frame folders: on generated JPEG trees (quality 90, 16 frames per video, source frames
25 % larger than the crop) at 64x64x3 (B=32) and 128x128x3 (B=16), in one call,
  (a) clips/s of the host DataLoader (PIL decode + default_transform + collate + pinned copy + H2D) at --workers 0, 4 and 14;
  (b) clips/s of DeviceFrameLoader alone, and the t2v_clip_gather launch's time and GB/s (1 byte read + 4 written per sample);
  (c) iterations/s of the CLI's train() loop (unconditional TGANv2, RSGAN + GP, HIP-graph replay) fed by the host loader at its
      best worker count, by DeviceFrameLoader, and — the yardstick — by the on-device synthetic loader at the same shape, twice
      (run-to-run spread).
Every measurement is a child process of its own (one process on the GPU at a time, each under a time limit; the first failure
ends the run). Rates are host clocks around work that ends in a device synchronise; the train() rate skips the first iterations
(eager warm-up and graph capture).
  python tools/frame_loader_bench.py [--out profiles/frame_cache_loader.json] [--work DIR]"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [{'size': 64, 'batch': 32, 'videos': 512}, {'size': 128, 'batch': 16, 'videos': 256}]
WORKERS = (0, 4, 14)
TRAIN_ITERS, TRAIN_SKIP = 100, 20


def make_tree(root, size, videos):
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(size)
    src = size + size // 4
    yy, xx = np.mgrid[0:src, 0:src].astype(np.float32) / src
    caps = {}
    for v in range(videos):
        d = os.path.join(root, 'videos', 'v%04d' % v)
        os.makedirs(d)
        f0, ph = rng.uniform(1, 6, size=3), rng.uniform(0, 6.28, size=3)
        for n in range(16):                                  # smooth moving pattern + noise: JPEG sizes like natural frames'
            img = np.stack([127 + 100 * np.sin(6.28 * f0[c] * (xx if c != 1 else yy) + ph[c] + 0.3 * n) for c in range(3)], -1)
            img = np.clip(img + rng.normal(0, 8, size=img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, '%d.jpg' % n), quality=90)
        caps['v%04d' % v] = ['digit %d is left and right.' % (v % 10)]
    anno = os.path.join(root, 'sent.pickle')
    with open(anno, 'wb') as f:
        pickle.dump(caps, f)
    return os.path.join(root, 'videos'), anno


def child_loader_host(a):
    import torch
    from txt2vid_amd import data as D
    ds = D.my_dataset(data=a.data, vocab=D.Vocab(), anno=a.anno, transform=D.default_transform([a.size], 3))
    loader = D.get_loader(dset=ds, batch_size=a.batch, num_workers=a.workers, device='cuda:0')
    torch.zeros(1).to('cuda:0')
    n, t0 = 0, None
    for epoch in range(2):                                   # epoch 0 warms the page cache and the allocator
        if epoch == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        pre = D.DevicePrefetcher(loader, 'cuda:0')
        x, _ = pre.next()
        while x is not None:
            n += (epoch == 1) * x.shape[0]
            x, _ = pre.next()
    torch.cuda.synchronize()
    return {'clips_per_s': n / (time.perf_counter() - t0), 'clips': n}


def child_loader_device(a):
    import torch
    from txt2vid_amd import data as D
    ds = D.my_dataset(data=a.data, vocab=D.Vocab(), anno=a.anno, transform=D.default_transform([a.size], 3), on_device=True)
    loader = D.get_loader(dset=ds, batch_size=a.batch, device='cuda:0')
    n, t0 = 0, None
    for epoch in range(6):
        if epoch == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for x, _, _ in loader:
            n += (epoch >= 1) * x.shape[0]
    torch.cuda.synchronize()
    rate = n / (time.perf_counter() - t0)
    cache = loader.cache
    rows = torch.randint(0, cache.block.shape[0], (a.batch * 16,), dtype=torch.int64).to('cuda:0')
    shape = (a.batch, 16, 3, a.size, a.size)
    out = torch.empty(shape, device='cuda:0')
    for _ in range(10):
        D.clip_gather(cache.device_block, rows, cache.device_lut, shape, loader._err, out=out)
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        D.clip_gather(cache.device_block, rows, cache.device_lut, shape, loader._err, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    loader.check_rows()
    return {'gpu': torch.cuda.get_device_name(0), 'clips_per_s': rate, 'clips': n, 'cache_mb': cache.nbytes / 1e6, 'cache_build_s': cache.seconds,
            'gather_ms_back_to_back': ms, 'gather_gb_per_s': 5.0 * out.numel() / (ms * 1e-3) / 1e9, 'gather_bytes_moved': 5 * out.numel()}


def child_train(a):
    import torch
    from txt2vid_amd import data as D
    from txt2vid_amd.train import gan
    stamps = []

    class Timed(object):
        def __init__(self, inner):
            self.inner, self.sampler = inner, getattr(inner, 'sampler', None)

        def __len__(self):
            return len(self.inner)

        def __iter__(self):
            for b in self.inner:
                stamps.append(time.perf_counter())          # batch k handed to the prefetcher
                yield b
    keep = D.get_loader
    D.get_loader = lambda **kw: Timed(keep(**kw))
    s = a.size
    argv = ['--data', a.spec, '--num_channels', '3', '--cuda', '--frame_sizes', str(s // 8), str(s // 4), str(s // 2), str(s),
            '--D_names', 'video', '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5',
            '--G_beta2', '.999', '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
            '--gp_lambda', '.5', '--subsample_input', '--workers', str(a.workers), '--log_period', '0', '--dont_use_sent',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--batch_size', str(a.batch), '--epochs', '1000', '--max_iters', str(TRAIN_ITERS), '--save_model_period', '0',
            '--save_example_period', '0', '--out', os.path.join(a.work, 'out'), '--out_samples', os.path.join(a.work, 'samples')]
    if a.anno:
        argv += ['--anno', a.anno]
    gan.main(gan.build_parser().parse_args(argv))
    torch.cuda.synchronize()
    end = time.perf_counter()
    # stamp k is taken when batch k+1 (1-based) is fetched, i.e. before iteration k starts (the prefetcher runs one ahead)
    done = TRAIN_ITERS - TRAIN_SKIP
    return {'iters_per_s': done / (end - stamps[TRAIN_SKIP + 1]), 'iters_timed': done, 'batch': a.batch}


CHILDREN = {'loader-host': child_loader_host, 'loader-device': child_loader_device, 'train': child_train}


def run_child(kind, limit, **kw):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', kind]
    for k, v in kw.items():
        if v is not None:
            cmd += ['--' + k, str(v)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
    out = p.stdout.decode(errors='replace')
    lines = [ln for ln in out.splitlines() if ln.startswith('RESULT ')]
    if p.returncode != 0 or not lines:
        sys.stderr.write(out[-4000:])
        raise SystemExit('%s %s failed with status %d: stopping (nothing more is started on the GPU)' % (kind, kw, p.returncode))
    res = json.loads(lines[-1][7:])
    print('%s %s -> %s' % (kind, {k: v for k, v in kw.items() if k in ('size', 'workers', 'spec')}, res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--work', default=None)
    ap.add_argument('--child', choices=sorted(CHILDREN))
    for name, typ in (('data', str), ('anno', str), ('spec', str), ('size', int), ('batch', int), ('workers', int)):
        ap.add_argument('--' + name, type=typ, default=None)
    a = ap.parse_args()
    if a.child:
        from txt2vid_amd.util.misc import limit_host_threads
        limit_host_threads()
        print('RESULT ' + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    import tempfile
    work = a.work or tempfile.mkdtemp(prefix='frame_loader_bench_')
    out = {'what': 'frame folders served by the host DataLoader vs the HBM frame cache (DeviceFrameLoader); unconditional TGANv2, RSGAN + GP '
                   '0.5, HIP-graph replay, %d timed iterations after %d' % (TRAIN_ITERS - TRAIN_SKIP, TRAIN_SKIP),
           'host_cpus': len(os.sched_getaffinity(0)), 'shapes': []}
    for sh in SHAPES:
        size, batch = sh['size'], sh['batch']
        root = os.path.join(work, 'tree%d' % size)
        t0 = time.time()
        data, anno = make_tree(root, size, sh['videos'])
        rec = {'size': size, 'channels': 3, 'batch': batch, 'videos': sh['videos'], 'frames_per_video': 16, 'source_side': size + size // 4,
               'tree_s': time.time() - t0}
        print('tree %dx%d: %d videos in %.1f s' % (size, size, sh['videos'], rec['tree_s']), flush=True)
        common = {'data': data, 'anno': anno, 'size': size, 'batch': batch}
        rec['host_loader'] = {str(w): run_child('loader-host', 600, workers=w, **common) for w in WORKERS}
        rec['device_loader'] = run_child('loader-device', 600, **common)
        best = max(WORKERS, key=lambda w: rec['host_loader'][str(w)]['clips_per_s'])
        specs = {}
        for name, args in (('host', {'data': data, 'num_frames': 16}), ('device', {'data': data, 'num_frames': 16, 'on_device': True}),
                           ('synthetic', {'data': 'synthetic', 'num_frames': 16, 'length': sh['videos'], 'on_device': True})):
            specs[name] = os.path.join(root, name + '.json')
            with open(specs[name], 'w') as f:
                json.dump({'class': 'txt2vid.data.my_dataset', 'args': args}, f)
        tr = {'size': size, 'batch': batch, 'work': root}
        rec['train'] = {
            'synthetic_on_device_1': run_child('train', 900, spec=specs['synthetic'], workers=0, **tr),
            'device_frames': run_child('train', 900, spec=specs['device'], anno=anno, workers=0, **tr),
            'host_loader_workers_%d' % best: run_child('train', 900, spec=specs['host'], anno=anno, workers=best, **tr),
            'synthetic_on_device_2': run_child('train', 900, spec=specs['synthetic'], workers=0, **tr)}
        s1, s2 = rec['train']['synthetic_on_device_1']['iters_per_s'], rec['train']['synthetic_on_device_2']['iters_per_s']
        dv, hs = rec['train']['device_frames']['iters_per_s'], rec['train']['host_loader_workers_%d' % best]['iters_per_s']
        rec['summary'] = {'synthetic_spread_rel': abs(s1 - s2) / max(s1, s2), 'device_vs_synthetic': dv / (0.5 * (s1 + s2)),
                          'device_within_synthetic_spread': dv >= min(s1, s2),
                          'device_vs_host_train': dv / hs, 'best_host_workers': best,
                          'device_vs_host_loader_alone': rec['device_loader']['clips_per_s'] / rec['host_loader'][str(best)]['clips_per_s']}
        out['shapes'].append(rec)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
