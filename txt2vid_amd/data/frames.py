"""Real-data twin of the on-device synthetic clips: a frame-folder `Dataset` decoded ONCE into a uint8 frame cache that lives in
HBM, and a loader that builds every batch with one `t2v_clip_gather` launch (csrc/data.hip) — per batch only B*T row indices and
the caption tokens cross PCIe; no JPEG is decoded, no float is made and no pixel is copied on the host after the first epoch.

What is cached is the INTEGER part of `default_transform` (centre crop with zero fill, `convert('RGB' | 'L')`, done by PIL exactly
as the host path does it); the float part is a 256-entry table computed with the host path's own numpy expression (`unit_range`),
so `lut[cache]` equals the host item bit for bit whatever the device's arithmetic does.

A dataset that augments its clips (`hflip`, `crop_jitter`, `window`) is served from the same cache by a different read
pattern: the crop is stored with a margin, `plan` makes the host items' draws, and `t2v_clip_gather_aug` reads each clip's window,
mirrored where drawn.
"""
import json
import os
import time

import numpy as np
import torch

from . import DeviceSyntheticLoader, pick_frames, unit_range

CACHE_VERSION = 1


def _paths(path):
    npy = str(path) if str(path).endswith('.npy') else str(path) + '.npy'
    return npy, npy + '.json'


class FrameCache(object):
    """uint8 frames of a frame-folder `Dataset`, channel-planar, one row [C,h,w] per frame, all videos back to back:
    `block` [rows, C*h*w] uint8 (host; `to(device)` uploads it), `table` {video id -> (first row, row count)}. With
    `random_frames == 0` only the strided pick of every video is stored (its `num_frames` rows, in pick order); otherwise every
    frame, so that any random pick is a set of rows. Items that share a video (several captions) share its rows. A dataset with
    `crop_jitter=J` stores the crop enlarged by a margin of J pixels on every side (`stored` = (h + 2J, w + 2J), `crop` stays the
    output crop): a jittered crop is then a window of the stored frame; a `window` dataset stores every frame."""

    RESERVE_BYTES = 16 << 30          # HBM left to the training step when `to()` sizes the cache against the free memory

    def __init__(self, block, table, meta):
        self.block, self.table, self.meta = block, table, meta
        self.crop, self.channels, self.margin = tuple(meta['crop']), int(meta['channels']), int(meta.get('margin', 0))
        self.stored = (self.crop[0] + 2 * self.margin, self.crop[1] + 2 * self.margin)
        self.row_bytes = self.channels * self.stored[0] * self.stored[1]
        self.lut = np.ascontiguousarray(unit_range(np.arange(256, dtype=np.uint8)))       # lut[u] == what the host transform makes of byte u
        self.device_block = self.device_lut = None
        self.seconds, self.source = 0.0, 'built'

    @property
    def nbytes(self):
        return int(self.block.shape[0]) * self.row_bytes

    @staticmethod
    def _spec(dset):
        """(integer part, crop, channels) of the dataset's transform — only `default_transform`'s closures carry them."""
        tf = dset.transform
        part, crop, ch = getattr(tf, 'integer_part', None), getattr(tf, 'crop', None), getattr(tf, 'num_channels', None)
        if part is None or crop is None or ch is None:
            raise ValueError('the frame cache stores the integer part of data.default_transform (crop + convert) and applies its float '
                             'part as a table: a dataset with another transform (%r) cannot be served from it — use the host loader '
                             '(on_device=False)' % (tf,))
        return part, (int(crop[0]), int(crop[1])), int(ch)

    @staticmethod
    def _meta(dset):
        """What a cache must agree with to serve `dset`: crop, channels, which frames are kept, and the folder listing."""
        _, crop, ch = FrameCache._spec(dset)
        listing = {}
        for vid in dset.video_ids:
            if str(vid) not in listing:
                folder = os.path.join(dset.video_dir, str(vid))
                listing[str(vid)] = [[name, os.path.getsize(os.path.join(folder, name))] for _, name in dset.frame_files(vid)]
        meta = {'version': CACHE_VERSION, 'crop': list(crop), 'channels': ch,
                'all_frames': bool(dset.random_frames or getattr(dset, 'window', 0)), 'num_frames': int(dset.num_frames), 'listing': listing}
        if getattr(dset, 'crop_jitter', 0):
            meta['margin'] = int(dset.crop_jitter)          # (absent without jitter: such sidecars are what they always were)
        return meta

    @classmethod
    def build(cls, dset):
        from PIL import Image
        t0 = time.time()
        part, crop, ch = cls._spec(dset)
        meta = cls._meta(dset)
        margin = int(meta.get('margin', 0))
        table, chosen, first = {}, [], 0
        for vid, files in meta['listing'].items():
            names = [f[0] for f in files]
            if getattr(dset, 'window', 0):
                dset.check_span(vid, len(names))
            elif not dset.random_frames:
                names = pick_frames(names, num_frames=dset.num_frames, random=False)
            elif len(names) < dset.random_frames:
                raise ValueError('video %s has %d frames, random_frames=%d needs at least that many' % (vid, len(names), dset.random_frames))
            table[vid] = (first, len(names))
            chosen.extend((vid, n) for n in names)
            first += len(names)
        block = np.empty((first, ch * (crop[0] + 2 * margin) * (crop[1] + 2 * margin)), dtype=np.uint8)
        for r, (vid, name) in enumerate(chosen):
            with Image.open(os.path.join(dset.video_dir, vid, name)) as img:
                img.load()
                a = np.asarray(part(img, margin=margin) if margin else part(img), dtype=np.uint8)
            block[r] = (a[None] if a.ndim == 2 else a.transpose(2, 0, 1)).reshape(-1)
        meta['table'] = {vid: list(fc) for vid, fc in table.items()}
        cache = cls(block, table, meta)
        cache.seconds = time.time() - t0
        return cache

    def save(self, path):
        """`<path>.npy` (the uint8 block, memory-mappable) + `<path>.npy.json` (crop, channels, per-video table, folder listing)."""
        npy, side = _paths(path)
        np.save(npy, np.ascontiguousarray(self.block))
        with open(side, 'w') as f:
            json.dump(self.meta, f)
        return npy

    @classmethod
    def load(cls, path, dset):
        """The cache written by `save`, memory-mapped; refused (ValueError) unless its sidecar matches `dset`: same crop, channels,
        frame selection and folder listing (names and sizes of every frame file of every video the dataset serves), and a margin
        (absent = 0) at least the dataset's `crop_jitter` — a larger one serves too, the windows then start further in."""
        t0 = time.time()
        npy, side = _paths(path)
        with open(side) as f:
            meta = json.load(f)
        want = cls._meta(dset)
        for key in ('version', 'crop', 'channels', 'all_frames', 'num_frames', 'listing'):
            if key == 'num_frames' and want['all_frames'] and meta.get('all_frames'):
                continue                                   # every frame is stored: the pick length does not matter
            if meta.get(key) != want[key]:
                a, b = meta.get(key), want[key]
                if key == 'listing':
                    a, b = '%d videos' % len(a or {}), '%d videos (or other frame files)' % len(b)
                raise ValueError('frame cache %s was not built for this dataset: its %s is %s, the dataset needs %s — rebuild it '
                                 '(python -m txt2vid_amd.data.cache)' % (npy, key, a, b))
        margin = int(meta.get('margin', 0))
        if margin < int(want.get('margin', 0)):
            raise ValueError('frame cache %s was not built for this dataset: its margin is %s, the dataset needs %s — rebuild it '
                             '(python -m txt2vid_amd.data.cache)' % (npy, margin, want['margin']))
        block = np.load(npy, mmap_mode='r')
        table = {vid: (int(fc[0]), int(fc[1])) for vid, fc in meta['table'].items()}
        rows = sum(c for _, c in table.values())
        stored = meta['channels'] * (meta['crop'][0] + 2 * margin) * (meta['crop'][1] + 2 * margin)
        if block.dtype != np.uint8 or block.ndim != 2 or block.shape != (rows, stored):
            raise ValueError('frame cache %s: the block %s %s does not match its sidecar (%d rows)' % (npy, block.dtype, block.shape, rows))
        cache = cls(block, table, meta)
        cache.seconds, cache.source = time.time() - t0, 'loaded from %s' % npy
        return cache

    def rows_of(self, video_id):
        return self.table[str(video_id)]

    def to(self, device, max_bytes=None, reserve_bytes=None):
        """Upload the block (once) and the table. Refuses a block larger than `max_bytes`; default: the device's free memory
        (`torch.cuda.mem_get_info`) minus `reserve_bytes` (RESERVE_BYTES, 16 GiB: activations, workspaces and graphs of the step)."""
        dev = torch.device(device)
        if max_bytes is None:
            if dev.type != 'cuda':
                raise RuntimeError('FrameCache.to: the cache serves the HIP gather kernel; there is no CPU path (use the host loader)')
            free, _ = torch.cuda.mem_get_info(dev)
            max_bytes = free - (self.RESERVE_BYTES if reserve_bytes is None else int(reserve_bytes))
        if self.nbytes > max_bytes:
            raise RuntimeError('frame cache of %d bytes (%d frames of %d bytes) exceeds the %d bytes it may take on %s: store fewer '
                               'frames (random_frames=0 keeps only the strided pick) or use the host loader'
                               % (self.nbytes, self.block.shape[0], self.row_bytes, max_bytes, dev))
        if dev.type != 'cuda':
            raise RuntimeError('FrameCache.to: the cache serves the HIP gather kernel; there is no CPU path (use the host loader)')
        if self.device_block is None or self.device_block.device != dev:
            out = torch.empty((self.nbytes,), dtype=torch.uint8, device=dev)
            flat, step = self.block.reshape(-1), 1 << 30             # (a memory-mapped block goes up in 1 GiB pieces: no second host copy)
            for a in range(0, self.nbytes, step):
                out[a:a + step].copy_(torch.from_numpy(np.array(flat[a:a + step])))
            self.device_block, self.device_lut = out, torch.from_numpy(self.lut).to(dev)
        return self


def frame_cache_for(dset):
    """The dataset's cache: loaded from `dset.cache_file` when that exists, built (and written there, if named) otherwise."""
    cache = getattr(dset, '_frame_cache', None)
    if cache is None:
        path = getattr(dset, 'cache_file', None)
        if path and os.path.exists(_paths(path)[1]):
            cache = FrameCache.load(path, dset)
        else:
            cache = FrameCache.build(dset)
            if path:
                cache.save(path)
        dset._frame_cache = cache
    return cache


def clip_gather(cache_u8, rows, lut, shape, err, out=None):
    """out[b,t] = lut[cache_u8[rows[b,t]]] (`t2v_clip_gather`): cache_u8 uint8 [n_rows * C*H*W] on the device, rows int64 [B*T] on
    the device, lut float32 [256], shape (B,T,C,H,W), err int32 [1] (set to 1 when a row index had to be clamped)."""
    import ctypes as C
    from .._lib import lib, check
    from .._ops import _stream
    B, T, Cc, H, W = [int(v) for v in shape]
    n = Cc * H * W
    for t, dt, numel in ((cache_u8, torch.uint8, None), (rows, torch.int64, B * T), (lut, torch.float32, 256), (err, torch.int32, 1)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or (numel is not None and t.numel() != numel):
            raise RuntimeError('clip_gather: dense device tensors uint8 / int64 [B*T] / float32 [256] / int32 [1] expected (the HIP '
                               'path has no CPU fallback)')
    if cache_u8.numel() < n or cache_u8.numel() % n:
        raise ValueError('clip_gather: the cache holds %d bytes, not a whole number of %d-byte frames' % (cache_u8.numel(), n))
    if out is None:
        out = torch.empty((B, T, Cc, H, W), device=cache_u8.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, T, Cc, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('clip_gather: the output buffer must be dense [B,T,C,H,W] float32 on the device')
    check(lib().t2v_clip_gather(C.c_void_p(cache_u8.data_ptr()), cache_u8.numel() // n, C.c_void_p(rows.data_ptr()), B, T, Cc, H, W,
                                C.c_void_p(lut.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(err.data_ptr()), _stream()),
          't2v_clip_gather')
    return out


def clip_gather_aug(cache_u8, rows, win, lut, shape, stored, err, out=None):
    """out[b,t,c,y,x] = lut[frame(rows[b,t])[c, y0_b + y, x0_b + (flip_b ? W-1-x : x)]] (`t2v_clip_gather_aug`): `clip_gather`
    through a per-clip window of the stored frames. cache_u8 uint8 [n_rows * C*Hc*Wc], rows int64 [B*T], win int32 [B,4] =
    (y0, x0, flip, 0), lut float32 [256], all on the device; shape (B,T,C,H,W), stored (Hc, Wc); err int32 [1] (set to 1 when a
    row index, a window origin or a flip had to be clamped)."""
    import ctypes as C
    from .._lib import lib, check
    from .._ops import _stream
    B, T, Cc, H, W = [int(v) for v in shape]
    Hc, Wc = int(stored[0]), int(stored[1])
    n = Cc * Hc * Wc
    for t, dt, numel in ((cache_u8, torch.uint8, None), (rows, torch.int64, B * T), (win, torch.int32, B * 4), (lut, torch.float32, 256),
                         (err, torch.int32, 1)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or (numel is not None and t.numel() != numel):
            raise RuntimeError('clip_gather_aug: dense device tensors uint8 / int64 [B*T] / int32 [B,4] / float32 [256] / int32 [1] '
                               'expected (the HIP path has no CPU fallback)')
    if H > Hc or W > Wc:
        raise ValueError('clip_gather_aug: a %dx%d window does not fit the stored %dx%d frames' % (H, W, Hc, Wc))
    if cache_u8.numel() < n or cache_u8.numel() % n:
        raise ValueError('clip_gather_aug: the cache holds %d bytes, not a whole number of %d-byte frames' % (cache_u8.numel(), n))
    if out is None:
        out = torch.empty((B, T, Cc, H, W), device=cache_u8.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, T, Cc, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('clip_gather_aug: the output buffer must be dense [B,T,C,H,W] float32 on the device')
    check(lib().t2v_clip_gather_aug(C.c_void_p(cache_u8.data_ptr()), cache_u8.numel() // n, C.c_void_p(rows.data_ptr()),
                                    C.c_void_p(win.data_ptr()), B, T, Cc, Hc, Wc, H, W, C.c_void_p(lut.data_ptr()),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(err.data_ptr()), _stream()), 't2v_clip_gather_aug')
    return out


class DeviceFrameLoader(object):
    """Stands in for `DataLoader(Dataset, collate_fn=collate_fn, num_workers=0)` when the frames live in HBM: same protocol as
    `DeviceSyntheticLoader` (len, iter -> (videos [B,T,C,h,w] float32 on the device, tokens [B,L] int64, lengths), drop_last) and
    the same sample order — for one process an epoch consumes the global torch generator exactly as `DataLoader(shuffle=True)`
    does, for several it walks the `DistributedSampler` handed in (`.sampler`, so `set_epoch` keeps working); random frame picks
    come from global `np.random` in item order, as the host loader's do."""

    RING = 8

    def __init__(self, dset, cache, batch_size, device, shuffle=True, sampler=None, max_bytes=None):
        self.dataset, self.cache, self.batch_size, self.device = dset, cache, int(batch_size), torch.device(device)
        self.shuffle, self.sampler, self.max_bytes = shuffle, sampler, max_bytes
        self._ring, self._pos, self._err = [], 0, None
        from ..util.log import status
        status('frame cache %s in %.2f s: %d frames of %dx%dx%d uint8, %.1f MB on %s; batches are gathered on the device (--workers is '
               'not used on this path)' % (cache.source, cache.seconds, cache.block.shape[0], cache.channels, cache.stored[0], cache.stored[1],
                                           cache.nbytes / 1e6, self.device))

    def __len__(self):
        return (len(self.sampler) if self.sampler is not None else len(self.dataset)) // self.batch_size

    def epoch_order(self):
        """The item indices of one epoch, in the order (and with the generator draws) of the host `DataLoader`."""
        if self.sampler is None:
            return [int(i) for i in DeviceSyntheticLoader.epoch_order(self)]
        torch.empty((), dtype=torch.int64).random_()                 # (_BaseDataLoaderIter's base seed: drawn, unused here)
        return [int(i) for i in self.sampler]

    def plan(self, indices):
        """Host half of a batch (no pixels): for the items in sampler order draw the frame pick and tokenise, then apply `collate_fn`'s
        rule (stable sort by caption length, descending; zero-padded int64 tokens). -> (rows int64 [B,T], tokens [B,L], lengths);
        for a dataset that flips or jitters (or a cache with a margin), a fourth element: win int32 [B,4] = (y0, x0, flip, 0) per
        clip, sorted with the rows, the window `t2v_clip_gather_aug` reads. The augmentation draws are `Dataset.draw`'s, item by
        item, as the host items make them; `window` alone only changes rows."""
        ds, picked, toks, wins = self.dataset, [], [], []
        aug, margin = getattr(ds, 'augmented', False), self.cache.margin
        for i in indices:
            first, count = self.cache.rows_of(ds.video_ids[int(i)])
            if not aug:                                    # the keys are off: what this loop always did
                if ds.random_frames:
                    picked.append(pick_frames(range(first, first + count), num_frames=ds.random_frames, random=True))
                else:
                    picked.append(list(range(first, first + count)))
                toks.append(ds.tokens(int(i)))
                continue
            if ds.random_frames:                           # (drawn in the window start's place, as the host item does)
                picked.append(pick_frames(range(first, first + count), num_frames=ds.random_frames, random=True))
            start, dy, dx, flip = ds.draw(ds.video_ids[int(i)], count)
            if ds.window:
                picked.append([first + start + ds.window * t for t in range(ds.num_frames)])
            elif not ds.random_frames:
                picked.append(list(range(first, first + count)))
            wins.append([margin + dy, margin + dx, flip, 0])
            toks.append(ds.tokens(int(i), flip))
        order = sorted(range(len(toks)), key=lambda k: len(toks[k]), reverse=True)
        lengths = [len(toks[k]) for k in order]
        rows = torch.tensor([picked[k] for k in order], dtype=torch.int64)
        tokens = torch.zeros(len(order), max(lengths), dtype=torch.long)
        for j, k in enumerate(order):
            tokens[j, :lengths[j]] = torch.tensor(toks[k], dtype=torch.long)
        if not (margin or (aug and (ds.hflip or ds.crop_jitter))):
            return rows, tokens, lengths
        win = torch.tensor([wins[k] for k in order] if aug else [[margin, margin, 0, 0]] * len(order), dtype=torch.int32)
        return rows, tokens, lengths, win

    def _upload(self, rows, tokens, win=None):
        """rows, tokens (and the windows, two int32 pairs per int64 pair) through one pinned slot of a small ring and one
        non-blocking copy: the host never waits for the stream (a slot is reused only after the copy that read it has finished — an
        event per slot, normally long past)."""
        n_r, n_t = rows.numel(), tokens.numel()
        n_w = 0 if win is None else win.numel() // 2
        if not self._ring:
            self._ring = [[None, torch.cuda.Event()] for _ in range(self.RING)]
        slot = self._ring[self._pos % self.RING]
        self._pos += 1
        if slot[0] is None or slot[0].numel() < n_r + n_t + n_w:
            slot[0] = torch.empty((2 * (n_r + n_t + n_w),), dtype=torch.int64).pin_memory()
        else:
            slot[1].synchronize()
        slot[0][:n_r].copy_(rows.reshape(-1))
        slot[0][n_r:n_r + n_t].copy_(tokens.reshape(-1))
        if n_w:
            slot[0][n_r + n_t:n_r + n_t + n_w].copy_(win.reshape(-1).view(torch.int64))
        dev = torch.empty((n_r + n_t + n_w,), dtype=torch.int64, device=self.device)
        dev.copy_(slot[0][:n_r + n_t + n_w], non_blocking=True)
        slot[1].record()
        if n_w:
            return dev[:n_r], dev[n_r:n_r + n_t].view(tokens.shape), dev[n_r + n_t:].view(torch.int32).view(win.shape)
        return dev[:n_r], dev[n_r:].view(tokens.shape)

    def device_batch(self, indices):
        if self.device.type != 'cuda':
            raise RuntimeError('DeviceFrameLoader gathers on the GPU: the HIP path has no CPU fallback (use the host loader)')
        if self.cache.device_block is None or self.cache.device_block.device != self.device:
            self.cache.to(self.device, max_bytes=self.max_bytes)
        if self._err is None:
            self._err = torch.zeros((1,), dtype=torch.int32).to(self.device)            # (zero by copy: no fill kernel)
        rows, tokens, lengths, *win = self.plan(indices)
        B, T = rows.shape
        shape = (B, T, self.cache.channels, self.cache.crop[0], self.cache.crop[1])
        if win:                                                       # flip, jitter or a cache with a margin: the windowed gather
            rows_dev, tokens_dev, win_dev = self._upload(rows, tokens, win[0])
            vids = clip_gather_aug(self.cache.device_block, rows_dev, win_dev, self.cache.device_lut, shape, self.cache.stored, self._err)
        else:
            rows_dev, tokens_dev = self._upload(rows, tokens)
            vids = clip_gather(self.cache.device_block, rows_dev, self.cache.device_lut, shape, self._err)
        return vids, tokens_dev, lengths

    def check_rows(self):
        """Raise if a gather kernel had to clamp a row index (or the augmented one a window or a flip) since the last check
        (device flag; one 4-byte read-back)."""
        if self._err is not None and int(self._err.item()) != 0:
            self._err.zero_()
            raise RuntimeError('t2v_clip_gather: a row index (or, augmented, a window) lay outside the frame cache (device flag set): '
                               'the batch was built from clamped values and is not what the host loader would have produced')

    def __iter__(self):
        order = self.epoch_order()
        for k in range(len(self)):
            yield self.device_batch(order[k * self.batch_size:(k + 1) * self.batch_size])
        self.check_rows()                                             # (one read-back per epoch: flagged, not hidden)

