"""What augmenting the real clips on the device costs: on generated JPEG trees (quality 90, 36 frames per video, source
frames 25 % larger than the crop), at B=32, T=16, 3x128x128 with crop_jitter 8 and at 1x64x64 with crop_jitter 4, in one session,
  (a) the plain gather (`t2v_clip_gather`, frames stored at the crop size) and the augmented gather (`t2v_clip_gather_aug`: random
      window of the frames stored with the margin, every second clip mirrored), alternated, two repeats each: ms per launch and GB/s
      (1 + 4 bytes per sample for the plain one; the augmented one is given both at those 5 bytes and at rho + 4, rho = Hc*Wc/(H*W),
      the whole stored frame read once);
  (b) the ratio of the two times next to the bound it is held against, (4 + rho) / 5 plus the spread of the two plain repeats;
  (c) clips/s of `DeviceFrameLoader` alone without the keys and with hflip + crop_jitter + window=2.
Both gathers read every-frame caches of the same row count (the plain one a `window` data set's, which the plain kernel serves).
One process, one GPU; rates are device events around back-to-back launches, and host clocks around epochs that end in a synchronise.
  python tools/frame_aug_bench.py [--out profiles/frame_aug_bench.json] [--work DIR]"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [{'size': 128, 'channels': 3, 'jitter': 8}, {'size': 64, 'channels': 1, 'jitter': 4}]
BATCH, FRAMES, VIDEOS, PER_VIDEO, WINDOW = 32, 16, 64, 36, 2
WARM, REPS = 10, 200


def make_tree(root, size, channels):
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(size)
    src = size + size // 4
    yy, xx = np.mgrid[0:src, 0:src].astype(np.float32) / src
    caps = {}
    for v in range(VIDEOS):
        d = os.path.join(root, 'videos', 'v%04d' % v)
        os.makedirs(d)
        f0, ph = rng.uniform(1, 6, size=3), rng.uniform(0, 6.28, size=3)
        for n in range(PER_VIDEO):
            img = np.stack([127 + 100 * np.sin(6.28 * f0[c] * (xx if c != 1 else yy) + ph[c] + 0.3 * n) for c in range(3)], -1)
            img = np.clip(img + rng.normal(0, 8, size=img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img if channels == 3 else img[..., 0]).save(os.path.join(d, '%d.jpg' % n), quality=90)
        caps['v%04d' % v] = ['digit %d is left and right.' % (v % 10)]
    anno = os.path.join(root, 'sent.pickle')
    with open(anno, 'wb') as f:
        pickle.dump(caps, f)
    return os.path.join(root, 'videos'), anno


def time_launch(fn):
    import torch
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def loader_rate(loader, epochs=30):
    import torch
    n, t0 = 0, None
    for epoch in range(epochs + 1):                          # epoch 0 uploads the cache and warms the allocator
        if epoch == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for x, _, _ in loader:
            n += (epoch >= 1) * x.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def measure(sh, work):
    import torch
    from txt2vid_amd import data as D
    S, C, J = sh['size'], sh['channels'], sh['jitter']
    data, anno = make_tree(os.path.join(work, 'tree%d' % S), S, C)

    def loader_for(**keys):
        ds = D.my_dataset(data=data, vocab=D.Vocab(), anno=anno, transform=D.default_transform([S], C), num_frames=FRAMES, on_device=True, **keys)
        return D.get_loader(dset=ds, batch_size=BATCH, device='cuda:0')
    off, rows_only, on = loader_for(), loader_for(window=WINDOW), loader_for(hflip=True, crop_jitter=J, window=WINDOW)
    rec = {'size': S, 'channels': C, 'batch': BATCH, 'frames': FRAMES, 'crop_jitter': J, 'window': WINDOW, 'videos': VIDEOS,
           'frames_per_video': PER_VIDEO, 'loader_clips_per_s': {'keys_off': loader_rate(off), 'hflip_jitter_window': loader_rate(on)}}
    loader_rate(rows_only, epochs=1)                         # (uploads its cache)
    plain_c, aug_c = rows_only.cache, on.cache
    assert plain_c.block.shape[0] == aug_c.block.shape[0] and plain_c.stored == (S, S) and aug_c.stored == (S + 2 * J, S + 2 * J)
    g = torch.Generator().manual_seed(0)
    rows = torch.randint(0, aug_c.block.shape[0], (BATCH * FRAMES,), dtype=torch.int64, generator=g).to('cuda:0')
    win = torch.zeros((BATCH, 4), dtype=torch.int32)
    win[:, :2] = torch.randint(0, 2 * J + 1, (BATCH, 2), generator=g).to(torch.int32)
    win[:, 2] = torch.arange(BATCH, dtype=torch.int32) % 2
    win = win.to('cuda:0')
    shape = (BATCH, FRAMES, C, S, S)
    out = torch.empty(shape, device='cuda:0')
    err = on._err

    def plain():
        D.clip_gather(plain_c.device_block, rows, plain_c.device_lut, shape, err, out=out)

    def aug():
        D.clip_gather_aug(aug_c.device_block, rows, win, aug_c.device_lut, shape, aug_c.stored, err, out=out)
    ms = {'plain': [], 'aug': []}
    for _ in range(2):                                       # alternated: plain, aug, plain, aug
        ms['plain'].append(time_launch(plain))
        ms['aug'].append(time_launch(aug))
    on.check_rows()
    rho = float(aug_c.stored[0] * aug_c.stored[1]) / (S * S)
    p, a = sum(ms['plain']) / 2, sum(ms['aug']) / 2
    spread = abs(ms['plain'][0] - ms['plain'][1]) / min(ms['plain'])
    rec.update({'gpu': torch.cuda.get_device_name(0), 'cache_mb': {'plain': plain_c.nbytes / 1e6, 'aug': aug_c.nbytes / 1e6},
                'gather_ms': ms, 'samples': out.numel(), 'rho': rho,
                'gb_per_s': {'plain_5_bytes': [5.0 * out.numel() / (t * 1e-3) / 1e9 for t in ms['plain']],
                             'aug_5_bytes': [5.0 * out.numel() / (t * 1e-3) / 1e9 for t in ms['aug']],
                             'aug_rho_plus_4_bytes': [(4.0 + rho) * out.numel() / (t * 1e-3) / 1e9 for t in ms['aug']]},
                'ratio_aug_over_plain': a / p, 'bound_4_plus_rho_over_5': (4.0 + rho) / 5.0, 'plain_spread_rel': spread,
                'within_bound_plus_spread': a / p <= (4.0 + rho) / 5.0 + spread})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--work', default=None)
    a = ap.parse_args()
    from txt2vid_amd.util.misc import limit_host_threads
    limit_host_threads()
    work = a.work or tempfile.mkdtemp(prefix='frame_aug_bench_')
    out = {'what': 'plain vs augmented gather from the HBM frame cache, alternated, %d launches each after %d; DeviceFrameLoader clips/s '
                   'with and without hflip + crop_jitter + window' % (REPS, WARM), 'shapes': []}
    for sh in SHAPES:
        rec = measure(sh, work)
        print(json.dumps(rec), flush=True)
        out['shapes'].append(rec)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
