"""GPU: the windowed, mirrored gather (`t2v_clip_gather_aug`) against plain host indexing, and batches of an augmented frame-folder
data set (hflip, crop_jitter, window) gathered from the HBM frame cache against the host DataLoader's — `torch.equal`
throughout: the kernel only moves bytes through the host's own 256-entry table."""
import json

import numpy as np
import pytest
import torch

from frame_cases import make_tree
from frame_aug_cases import ODD, BIG_ODD, aug_dataset
from txt2vid_amd import data as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_ROWS = 11


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('odd'), sizes=ODD)


@pytest.fixture(scope='module')
def big_tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('big_odd'), sizes=BIG_ODD)


def host_gather(store, rows, win, lut, shape, stored):
    """out[b,t,c,y,x] = lut[frame(rows[b,t])[c, y0_b + y, x0_b + (flip_b ? W-1-x : x)]] by indexing, on the host."""
    B, T, C, H, W = shape
    Hc, Wc = stored
    frames = store.reshape(-1, C, Hc, Wc)
    out = torch.empty(shape, dtype=torch.float32)
    for b in range(B):
        y0, x0, flip = [int(v) for v in win[b][:3]]
        for t in range(T):
            w = frames[int(rows[b * T + t])][:, y0:y0 + H, x0:x0 + W]
            out[b, t] = lut[(w.flip(-1) if flip else w).long()]
    return out


def operands(shape, stored, offset, seed=3):
    B, T, C, H, W = shape
    n = C * stored[0] * stored[1]
    g = torch.Generator().manual_seed(seed)
    store = torch.randint(0, 256, (offset + N_ROWS * n,), dtype=torch.uint8, generator=g)
    rows = torch.randint(0, N_ROWS, (B * T,), dtype=torch.int64, generator=g)
    rows[0], rows[-1] = 0, N_ROWS - 1              # the first and the last frame of the cache are read
    lut = torch.from_numpy(D.unit_range(np.arange(256, dtype=np.uint8)))
    return store, rows, lut


@pytest.mark.parametrize('dims,offset', [((2, 3, 1, 17, 19, 15, 15), 0), ((2, 3, 3, 5, 7, 5, 7), 0), ((3, 2, 1, 12, 12, 8, 8), 5),
                                         ((1, 4, 2, 16, 16, 16, 16), 0), ((2, 2, 3, 40, 40, 30, 30), 0)])
def test_windowed_gather_equals_host_indexing(dims, offset):
    """Odd everything (scalar stores), no margin (flip only, odd planes), an unaligned cache base, the all-vector case flipped,
    W % 16 != 0 with a reversed tail. Every launch gives each clip another window: the four corners of the valid range (the first
    starts on byte 0 of frame 0, the last ends on the last byte of the last frame), an odd x0, both directions."""
    B, T, C, Hc, Wc, H, W = dims
    shape, stored = (B, T, C, H, W), (Hc, Wc)
    store, rows, lut = operands(shape, stored, offset)
    my, mx = Hc - H, Wc - W
    odd_x = 1 if mx >= 1 else 0
    places = [(0, 0), (0, mx), (my, 0), (my, mx), (my // 2, odd_x), (min(1, my), min(3, mx))]
    err = torch.zeros(1, dtype=torch.int32).to(DEV)
    store_dev, rows_dev, lut_dev = store.to(DEV)[offset:], rows.to(DEV), lut.to(DEV)
    for shift in range(len(places)):
        for flip0 in (0, 1):
            win = []
            for b in range(B):
                y0, x0 = places[(shift + 3 * b) % len(places)]
                win.append([y0, x0, (flip0 + b) % 2, 0])
            if shift == 0:
                win[-1][:2] = [my, mx]             # with rows[-1] = the last row: the window that ends on the cache's last byte
            win = torch.tensor(win, dtype=torch.int32)
            out = D.clip_gather_aug(store_dev, rows_dev, win.to(DEV), lut_dev, shape, stored, err)
            want = host_gather(store[offset:], rows, win, lut, shape, stored)
            assert torch.equal(out.cpu(), want), (shift, flip0, win.tolist())
    assert int(err.item()) == 0


@pytest.mark.parametrize('shape,offset', [((2, 3, 1, 15, 15), 0), ((3, 2, 1, 8, 8), 5), ((1, 4, 2, 16, 16), 0), ((2, 2, 3, 64, 64), 0)])
def test_identity_window_equals_the_plain_gather(shape, offset):
    store, rows, lut = operands(shape, shape[3:], offset)
    err = torch.zeros(1, dtype=torch.int32).to(DEV)
    store_dev, rows_dev, lut_dev = store.to(DEV)[offset:], rows.to(DEV), lut.to(DEV)
    win = torch.zeros((shape[0], 4), dtype=torch.int32).to(DEV)
    a = D.clip_gather_aug(store_dev, rows_dev, win, lut_dev, shape, shape[3:], err)
    b = D.clip_gather(store_dev, rows_dev, lut_dev, shape, err)
    assert torch.equal(a, b) and int(err.item()) == 0


def test_bad_rows_windows_and_flips_are_clamped_and_flagged(tree):
    """Never dereferenced as given: a row outside [0, n_rows), a window outside the stored frame and a flip outside {0, 1} are
    clamped, the device word is set and the loader's check raises (and clears it). Nothing is provoked: the kernel reads only
    through the clamped values."""
    ds = aug_dataset(tree, 32, 1, on_device=True, num_frames=8, hflip=True, crop_jitter=2)
    loader = D.get_loader(dset=ds, batch_size=2, device=DEV)
    loader.device_batch([0, 1])
    loader.check_rows()                                                  # nothing flagged by a good batch
    cache = loader.cache
    n_rows, (Hc, Wc) = cache.block.shape[0], cache.stored
    assert (Hc, Wc) == (36, 36)
    shape = (4, 2, 1, 32, 32)
    rows = torch.tensor([-7, 3, n_rows + 1000, 1, 1 << 40, 5, 2, n_rows - 1], dtype=torch.int64)
    win = torch.tensor([[Hc, 1, 0, 0], [1, -1, 1, 0], [0, 0, 2, 0], [4, 4, 0, 0]], dtype=torch.int32)
    store = torch.from_numpy(np.ascontiguousarray(cache.block)).reshape(-1)
    lut = torch.from_numpy(cache.lut)
    clamped_rows = torch.tensor([0, 3, n_rows - 1, 1, n_rows - 1, 5, 2, n_rows - 1])
    clamped_win = torch.tensor([[Hc - 32, 1, 0, 0], [1, 0, 1, 0], [0, 0, 1, 0], [4, 4, 0, 0]], dtype=torch.int32)
    want = host_gather(store, clamped_rows, clamped_win, lut, shape, (Hc, Wc))
    for bad in range(6):                                                 # each offender alone sets the flag ...
        r, w = clamped_rows.clone(), clamped_win.clone()
        if bad < 3:
            r[2 * bad] = rows[2 * bad]
        else:
            w[bad - 3] = win[bad - 3]
        out = D.clip_gather_aug(cache.device_block, r.to(DEV), w.to(DEV), cache.device_lut, shape, (Hc, Wc), loader._err)
        assert torch.equal(out.cpu(), want), bad
        with pytest.raises(RuntimeError, match='outside the frame cache'):
            loader.check_rows()
        loader.check_rows()                                              # the flag was cleared by the raise
    out = D.clip_gather_aug(cache.device_block, rows.to(DEV), win.to(DEV), cache.device_lut, shape, (Hc, Wc), loader._err)   # ... and all together
    assert torch.equal(out.cpu(), want) and int(loader._err.item()) == 1
    with pytest.raises(RuntimeError, match='outside the frame cache'):
        loader.check_rows()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.clip_gather_aug(store, rows, win, lut, shape, (Hc, Wc), torch.zeros(1, dtype=torch.int32))


def walk(pre):
    x, y = pre.next()
    while x is not None:
        yield x, y
        x, y = pre.next()


@pytest.mark.parametrize('crop,channels,jitter,hflip,window,random_frames',
                         [(64, 3, 3, True, 0, 0), (30, 1, 1, True, 2, 0), (64, 1, 0, True, 0, 0), (64, 3, 5, False, 0, 8), (128, 3, 8, True, 2, 0),
                          (64, 1, 0, False, 2, 0)])
def test_device_batches_equal_host_batches(tree, big_tree, crop, channels, jitter, hflip, window, random_frames):
    """Host DataLoader against DeviceFrameLoader through DevicePrefetcher, 2 epochs from the same generator states, batch 3."""
    where = big_tree if crop == 128 else tree
    args = {'num_frames': 8 if window else 16, 'hflip': hflip, 'crop_jitter': jitter, 'window': window, 'random_frames': random_frames}
    if hflip and jitter == 3:
        args['hflip_swap'] = [['left', 'right'], ['top', 'bottom']]
    args = json.loads(json.dumps(args))                                   # the spec's keys as a --data JSON file delivers them
    host_ds = aug_dataset(where, crop, channels, **args)
    dev_ds = aug_dataset(where, crop, channels, on_device=True, **args)
    torch.manual_seed(21)
    np.random.seed(21)
    host_loader = D.get_loader(dset=host_ds, batch_size=3, num_workers=0, device=DEV)
    host = [list(host_loader) for _ in range(2)]
    torch.manual_seed(21)
    np.random.seed(21)
    loader = D.get_loader(dset=dev_ds, batch_size=3, num_workers=0, device=DEV)
    assert isinstance(loader, D.DeviceFrameLoader) and isinstance(host_loader, torch.utils.data.DataLoader)
    assert loader.cache.stored == (crop + 2 * jitter, crop + 2 * jitter) and loader.cache.crop == (crop, crop)
    n = 0
    for epoch in range(2):
        for k, (x, y) in enumerate(walk(D.DevicePrefetcher(loader, DEV))):
            hv, ht, hl = host[epoch][k]
            assert x.is_cuda and x.dtype == torch.float32 and y[0].is_cuda and y[0].dtype == torch.int64
            assert torch.equal(x.cpu(), hv), (epoch, k, float((x.cpu() - hv).abs().max()))
            assert torch.equal(y[0].cpu(), ht) and list(y[1]) == list(hl), (epoch, k)
            n += 1
    assert n == 2 * len(host_loader) and n > 0
    # flip or jitter: the windowed gather built these batches; window alone only changes rows and the plain gather serves
    assert len(loader.plan([0, 1, 2])) == (4 if hflip or jitter else 3)


def test_nearest_search_reads_plain_items(tree):
    from txt2vid_amd.gan import sample
    ds = aug_dataset(tree, 32, 3, num_frames=8, hflip=True, crop_jitter=3, window=2)
    np.random.seed(1)
    state = np.random.get_state()[1].copy()
    a = sample._real_batch(ds, 0, 4, DEV)
    b = sample._real_batch(ds, 0, 4, DEV)
    want = torch.stack([ds.plain(i)[0] for i in range(4)]).permute(0, 2, 1, 3, 4)
    assert torch.equal(a, b) and torch.equal(a.cpu(), want) and a.is_contiguous()
    assert np.array_equal(np.random.get_state()[1], state)               # no draw was consumed
