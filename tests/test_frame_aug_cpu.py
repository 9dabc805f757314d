"""CPU: per-clip augmentation of a frame-folder `Dataset` (hflip, crop_jitter, window) — the host items against an
independent numpy construction, the frame cache with its margin against the host items, `DeviceFrameLoader.plan` against the host
loader's draws, sidecars, refusals, the caption swap and `Dataset.plain`. Every comparison is exact: both sides move the same
bytes and share `unit_range`."""
import json
import os

import numpy as np
import pytest
import torch

from frame_cases import make_tree
from frame_aug_cases import ODD, aug_dataset, expected_clip, frame_names, replay_draws, source_window
from txt2vid_amd import data as D

T = 8           # frames per clip here: window=2 then spans 15 frames, and the shortest video has 20
SETTINGS = [{'hflip': True}, {'crop_jitter': 3}, {'window': 2}, {'hflip': True, 'crop_jitter': 3, 'window': 2}]


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('odd'), sizes=ODD)


def keys_of(s):
    return s.get('window', 0), s.get('crop_jitter', 0), s.get('hflip', False)


@pytest.mark.parametrize('setting', SETTINGS, ids=lambda s: '+'.join(sorted(s)))
@pytest.mark.parametrize('crop,channels', [(64, 3), (30, 1)])
def test_host_items_equal_an_independent_construction(tree, setting, crop, channels):
    ds = aug_dataset(tree, crop, channels, num_frames=T, **setting)
    window, jitter, hflip = keys_of(setting)
    assert (ds.window, ds.crop_jitter, ds.hflip) == (window, jitter, hflip)          # recorded, not swallowed
    seen = set()
    for i in range(len(ds)):
        vid = ds.video_ids[i]
        np.random.seed(40 + i)
        got = ds[i][0].numpy()
        after = np.random.get_state()[1].copy()
        np.random.seed(40 + i)
        start, dy, dx, flip = replay_draws(len(frame_names(tree[0], vid)), T, window, jitter, hflip)
        assert np.array_equal(np.random.get_state()[1], after), i                     # exactly these draws, no other
        want = expected_clip(tree[0], vid, (crop, crop), channels, T, window, start, dy, dx, flip)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), (i, start, dy, dx, flip)
        seen.add((start, dy, dx, flip))
    # not vacuous: every key that is on did vary over the six items
    assert not hflip or {s[3] for s in seen} == {0, 1}
    assert not jitter or len({s[1:3] for s in seen}) >= 3
    assert not window or len({s[0] for s in seen}) >= 3


@pytest.mark.parametrize('crop,channels,jitter', [(64, 3, 3), (64, 1, 1), (30, 1, 5)])
def test_cache_with_margin_equals_host_items(tree, crop, channels, jitter):
    """J odd on the tree whose (w - crop) is odd: a margin cut from a re-rounded enlarged crop would sit one pixel off."""
    ds = aug_dataset(tree, crop, channels, num_frames=T, hflip=True, crop_jitter=jitter, window=2)
    cache = D.FrameCache.build(ds)
    Hc = crop + 2 * jitter
    assert cache.margin == jitter and cache.crop == (crop, crop) and cache.stored == (Hc, Hc) and cache.meta['margin'] == jitter
    assert cache.block.shape == (40 + 33 + 40 + 20, channels * Hc * Hc) and cache.row_bytes == channels * Hc * Hc
    for vid in ('vid0', 'vid1', 'vid2', 'vid3'):                                     # the stored frame is the source window with the margin
        first, count = cache.rows_of(vid)
        names = frame_names(tree[0], vid)
        for f in (0, count - 1):
            want = source_window(os.path.join(tree[0], vid, names[f]), (crop, crop), channels, margin=jitter)
            assert np.array_equal(np.asarray(cache.block[first + f]).reshape(channels, Hc, Hc), want), (vid, f)
    flips = set()
    for i in range(len(ds)):
        first, count = cache.rows_of(ds.video_ids[i])
        np.random.seed(7 + i)
        host = ds[i][0].numpy()
        np.random.seed(7 + i)
        start, dy, dx, flip = replay_draws(count, T, 2, jitter, True)
        y0, x0 = jitter + dy, jitter + dx
        rows = [first + start + 2 * t for t in range(T)]
        got = cache.lut[np.asarray(cache.block)[rows]].reshape(T, channels, Hc, Hc)[:, :, y0:y0 + crop, x0:x0 + crop]
        got = got[..., ::-1] if flip else got
        assert np.array_equal(got, host), (i, start, dy, dx, flip)
        flips.add(flip)
    assert flips == {0, 1}


def host_epoch(loader):
    return [b for b in loader]


@pytest.mark.parametrize('setting', [{'hflip': True, 'crop_jitter': 3, 'window': 2}, {'hflip': True, 'crop_jitter': 2, 'random_frames': 5},
                                     {'window': 3}], ids=lambda s: '+'.join(sorted(s)))
def test_plan_makes_the_host_loaders_draws(tree, setting):
    """One walk of two epochs each: same generator states afterwards, and the planned rows / windows / tokens name the host batches
    (in `collate_fn`'s order: captions of equal length, so the stable sort decides)."""
    swap = [['left', 'right']] if setting.get('hflip') else None
    nf = 4 if setting.get('window') == 3 else T
    ds = aug_dataset(tree, 32, 3, num_frames=nf, hflip_swap=swap, **setting)
    torch.manual_seed(9)
    np.random.seed(9)
    host_loader = D.get_loader(dset=ds, batch_size=2, num_workers=0)
    host = [host_epoch(host_loader) for _ in range(2)]
    after = (torch.get_rng_state(), np.random.get_state()[1].copy(), np.random.get_state()[2])
    dev_ds = aug_dataset(tree, 32, 3, on_device=True, num_frames=nf, hflip_swap=swap, **setting)
    torch.manual_seed(9)
    np.random.seed(9)
    loader = D.get_loader(dset=dev_ds, batch_size=2, num_workers=0, device='cuda:0')          # (no GPU is touched before iteration)
    assert isinstance(loader, D.DeviceFrameLoader)
    cache, J = loader.cache, setting.get('crop_jitter', 0)
    Hc, Wc = cache.stored
    seen = set()
    for epoch in range(2):
        order = loader.epoch_order()
        for k in range(len(loader)):
            planned = loader.plan(order[2 * k:2 * k + 2])
            hv, ht, hl = host[epoch][k]
            rows, tokens, lengths = planned[:3]
            if setting.get('hflip') or J:
                win = planned[3]
                assert win.dtype == torch.int32 and win.shape == (2, 4) and int(win[:, 3].abs().sum()) == 0
            else:
                assert len(planned) == 3                           # window alone only changes rows: the plain gather serves
                win = torch.tensor([[0, 0, 0, 0]] * 2, dtype=torch.int32)
            assert rows.dtype == torch.int64 and tuple(rows.shape) == (2, setting.get('random_frames') or nf)
            full = cache.lut[np.asarray(cache.block)[rows.reshape(-1).tolist()]].reshape(2, -1, 3, Hc, Wc)
            for b in range(2):
                y0, x0, flip = [int(v) for v in win[b, :3]]
                assert 0 <= y0 - (cache.margin - J) <= 2 * J and 0 <= x0 - (cache.margin - J) <= 2 * J and flip in (0, 1)
                got = full[b, :, :, y0:y0 + 32, x0:x0 + 32]
                got = got[..., ::-1] if flip else got
                assert np.array_equal(got, hv[b].numpy()), (epoch, k, b)
                seen.add((y0, x0, flip))
            assert torch.equal(tokens, ht) and lengths == hl, (epoch, k)
    assert torch.equal(torch.get_rng_state(), after[0])
    assert np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    if setting.get('hflip'):                                       # not vacuous: both directions and several offsets were walked
        assert {s[2] for s in seen} == {0, 1} and len({s[:2] for s in seen}) >= 3


def test_sidecars_margin_and_frame_selection(tree, tmp_path):
    off = aug_dataset(tree, 32, 1, num_frames=T)
    meta = D.FrameCache._meta(off)
    assert sorted(meta) == ['all_frames', 'channels', 'crop', 'listing', 'num_frames', 'version']     # the parent's keys, no new one
    assert meta['all_frames'] is False and meta['crop'] == [32, 32] and meta['version'] == 1
    plain = D.FrameCache.build(off)
    assert 'margin' not in plain.meta and plain.margin == 0 and plain.stored == plain.crop == (32, 32)
    p0 = plain.save(str(tmp_path / 'plain'))
    assert D.FrameCache.load(p0, off).margin == 0                                    # a sidecar without `margin` loads
    jit = aug_dataset(tree, 32, 1, num_frames=T, crop_jitter=2, hflip=True)
    with pytest.raises(ValueError, match='margin is 0, the dataset needs 2'):
        D.FrameCache.load(p0, jit)                                                   # margin < jitter
    wide = D.FrameCache.build(aug_dataset(tree, 32, 1, num_frames=T, crop_jitter=5))
    p5 = wide.save(str(tmp_path / 'wide'))
    back = D.FrameCache.load(p5, jit)                                                # margin > jitter: serves, windows start further in
    assert back.margin == 5 and back.stored == (42, 42)
    loader = D.DeviceFrameLoader(jit, back, 2, 'cuda:0', shuffle=False)
    for i in range(len(jit)):
        np.random.seed(60 + i)
        host = jit[i][0].numpy()
        np.random.seed(60 + i)
        rows, _, _, win = loader.plan([i])
        y0, x0, flip = [int(v) for v in win[0, :3]]
        assert 3 <= y0 <= 7 and 3 <= x0 <= 7
        got = back.lut[np.asarray(back.block)[rows[0].tolist()]].reshape(T, 1, 42, 42)[:, :, y0:y0 + 32, x0:x0 + 32]
        assert np.array_equal(got[..., ::-1] if flip else got, host), i
    rows, _, _, win = D.DeviceFrameLoader(off, D.FrameCache.load(p5, off), 2, 'cuda:0', shuffle=False).plan([0])
    assert win.tolist() == [[5, 5, 0, 0]]                                            # keys off on a margin cache: the centred window
    win_ds = aug_dataset(tree, 32, 1, num_frames=T, window=2)
    with pytest.raises(ValueError, match='all_frames'):
        D.FrameCache.load(p0, win_ds)                                                # a window data set needs every frame
    every = D.FrameCache.build(aug_dataset(tree, 32, 1, num_frames=T, random_frames=4))
    assert D.FrameCache.load(every.save(str(tmp_path / 'every')), win_ds).block.shape[0] == 133


def test_command_line_writes_margin_and_every_frame(tree, tmp_path):
    from txt2vid_amd.data import cache as cache_cli
    out = str(tmp_path / 'c.npy')
    assert cache_cli.main(['--data', tree[0], '--anno', tree[1], '--frame_size', '32', '--num_channels', '1', '--num_frames', str(T),
                           '--crop_jitter', '3', '--window', '2', '--out', out]) == 0
    side = json.load(open(out + '.json'))
    assert side['margin'] == 3 and side['all_frames'] is True and np.load(out).shape == (133, 38 * 38)
    ds = aug_dataset(tree, 32, 1, on_device=True, cache_file=out, num_frames=T, crop_jitter=3, window=2, hflip=True)
    assert D.get_loader(dset=ds, batch_size=2, device='cuda:0').cache.source.startswith('loaded from')


def test_refusals(tree):
    with pytest.raises(ValueError, match='window=2 and random_frames=4'):
        aug_dataset(tree, 32, 1, window=2, random_frames=4)
    with pytest.raises(ValueError, match='crop_jitter'):
        aug_dataset(tree, 32, 1, crop_jitter=-1)
    short = aug_dataset(tree, 32, 1, num_frames=16, window=2)                        # spans 31 frames; vid1 has 33, vid3 has 20
    with pytest.raises(ValueError, match='video vid3 has 20 frames'):
        short[5]
    with pytest.raises(ValueError, match='video vid3 has 20 frames'):
        D.FrameCache.build(short)
    with pytest.raises(ValueError, match="'sideways' is not in the vocabulary"):
        aug_dataset(tree, 32, 1, hflip=True, hflip_swap=[['left', 'sideways']])
    with pytest.raises(ValueError, match='needs hflip'):
        aug_dataset(tree, 32, 1, hflip_swap=[['left', 'right']])
    for keys in ({'hflip': True}, {'crop_jitter': 2}, {'window': 2}):
        with pytest.raises(ValueError, match='synthetic'):
            D.my_dataset(data='synthetic', vocab=D.Vocab(), **keys)
        with pytest.raises(ValueError, match='default_transform'):
            D.my_dataset(data=tree[0], vocab=D.Vocab(), anno=tree[1], transform=lambda img: torch.zeros(1, 4, 4), **keys)
        with pytest.raises(ValueError, match='default_transform'):                   # ... on the device path too: at construction
            D.my_dataset(data=tree[0], vocab=D.Vocab(), anno=tree[1], transform=lambda img: torch.zeros(1, 4, 4), on_device=True, **keys)


def test_token_swap_on_exactly_the_flipped_clips(tree):
    ds = aug_dataset(tree, 32, 1, num_frames=T, hflip=True, hflip_swap=[['left', 'right'], ['top', 'bottom']])
    base = aug_dataset(tree, 32, 1, num_frames=T)
    v = ds.vocab
    pairs = {v('left'): v('right'), v('right'): v('left'), v('top'): v('bottom'), v('bottom'): v('top')}
    np.random.seed(3)
    flips = []
    for i in range(len(ds)):
        state = np.random.get_state()
        flip = int(np.random.randint(0, 2))
        np.random.set_state(state)
        frames, toks = ds[i]
        plain = base[i][1]
        want = torch.tensor([pairs.get(int(t), int(t)) for t in plain], dtype=torch.float32) if flip else plain
        assert toks.shape == plain.shape and torch.equal(toks, want), (i, flip)
        assert torch.equal(frames, base[i][0].flip(-1) if flip else base[i][0]), (i, flip)
        flips.append(flip)
    assert set(flips) == {0, 1}
    assert any(not torch.equal(ds.plain(i)[1], torch.tensor(ds.tokens(i, 1), dtype=torch.float32)) for i in range(len(ds)))   # a swap happened


def test_plain_items_draw_nothing(tree):
    off = aug_dataset(tree, 32, 3, num_frames=T)
    on = aug_dataset(tree, 32, 3, num_frames=T, hflip=True, crop_jitter=3, window=2, hflip_swap=[['left', 'right']])
    np.random.seed(5)
    torch.manual_seed(5)
    before = (np.random.get_state()[1].copy(), np.random.get_state()[2], torch.get_rng_state())
    for i in range(len(off)):
        a, b = off.plain(i), off[i]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), i                # keys off: plain is the item
        p = on.plain(i)
        count = len(frame_names(tree[0], on.video_ids[i]))
        want = expected_clip(tree[0], on.video_ids[i], (32, 32), 3, T, 2, (count - 15) // 2, 0, 0, 0)     # the centred window
        assert np.array_equal(p[0].numpy(), want) and torch.equal(p[1], b[1]), i
    assert np.array_equal(np.random.get_state()[1], before[0]) and np.random.get_state()[2] == before[1]
    assert torch.equal(torch.get_rng_state(), before[2])
