"""GPU: batches gathered from the HBM frame cache (`t2v_clip_gather`) equal the host DataLoader's batches exactly — the cache
holds PIL's bytes and the 256-entry table holds the host transform's own floats, so the kernel adds no error and the bound is
`torch.equal`; a row index outside the cache is clamped and flagged, never dereferenced; the CLI trains on device batches."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from frame_cases import make_tree, make_golden_tree

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ((150, 160), (130, 140), (160, 170), (30, 30))          # source frames around a 128x128 crop (vid3 stays 30x30: zero fill)


def walk(pre):
    x, y = pre.next()
    while x is not None:
        yield x, y
        x, y = pre.next()


def assert_loaders_agree(host_ds, dev_ds, batch, epochs=2):
    from txt2vid_amd import data as D
    torch.manual_seed(21)
    np.random.seed(21)
    host_loader = D.get_loader(dset=host_ds, batch_size=batch, num_workers=0, device=DEV)
    host = [list(host_loader) for _ in range(epochs)]
    torch.manual_seed(21)
    np.random.seed(21)
    loader = D.get_loader(dset=dev_ds, batch_size=batch, num_workers=0, device=DEV)
    assert isinstance(loader, D.DeviceFrameLoader) and isinstance(host_loader, torch.utils.data.DataLoader)
    n = 0
    for epoch in range(epochs):
        for k, (x, y) in enumerate(walk(D.DevicePrefetcher(loader, DEV))):
            hv, ht, hl = host[epoch][k]
            assert x.is_cuda and x.dtype == torch.float32 and y[0].is_cuda and y[0].dtype == torch.int64
            assert torch.equal(x.cpu(), hv), (epoch, k, float((x.cpu() - hv).abs().max()))
            assert torch.equal(y[0].cpu(), ht) and list(y[1]) == list(hl), (epoch, k)
            n += 1
    assert n == epochs * len(host_loader) and n > 0
    return loader


@pytest.mark.parametrize('crop,channels,random_frames', [(64, 3, 0), (128, 3, 0), (64, 1, 0), (30, 1, 0), (64, 3, 8), (30, 1, 8)])
def test_device_batches_equal_host_batches(tmp_path, crop, channels, random_frames):
    from txt2vid_amd import data as D
    root, anno = make_tree(tmp_path, sizes=BIG) if crop == 128 else make_tree(tmp_path)
    tf = D.default_transform([crop], channels)
    host_ds = D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=tf, random_frames=random_frames)
    dev_ds = D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=tf, random_frames=random_frames, on_device=True)
    loader = assert_loaders_agree(host_ds, dev_ds, batch=3)
    assert loader.cache.row_bytes == channels * crop * crop and (crop != 30 or loader.cache.row_bytes % 16 == 4)   # 30x30: head / tail path


def test_reference_fixture_folders_from_the_cache(golden, tmp_path):
    """tests/golden/data_contract.npz: the device batch equals what the REAL reference's Dataset + collate_fn produced."""
    from txt2vid_amd import data as D
    g = golden('data_contract')
    root, anno, (h, w) = make_golden_tree(g, tmp_path)
    vocab = D.build_vocab([str(s) for s in g['sentences']])
    ds = D.my_dataset(data=root, vocab=vocab, anno=anno, transform=D.default_transform([h, w], 1), on_device=True)
    loader = D.get_loader(dset=ds, batch_size=len(ds), val=True, device=DEV)
    x, y = D.DevicePrefetcher(loader, DEV).next()
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), g['collate_vids'])
    assert np.array_equal(y[0].cpu().numpy(), g['collate_targets']) and list(y[1]) == list(g['collate_lengths'])


@pytest.mark.parametrize('shape,offset', [((2, 3, 1, 15, 15), 0), ((2, 3, 3, 5, 7), 0), ((3, 2, 1, 8, 8), 5), ((1, 4, 2, 16, 16), 0)])
def test_gather_any_row_size_and_alignment(shape, offset):
    """Op level: C*H*W odd (scalar stores: the output row is not 16-byte aligned), not a multiple of 16 (head / tail), a cache
    base that is not 16-byte aligned (a slice), and the all-vector case — against plain indexing on the host."""
    from txt2vid_amd import data as D
    B, T, C, H, W = shape
    n, n_rows = C * H * W, 11
    g = torch.Generator().manual_seed(3)
    store = torch.randint(0, 256, (offset + n_rows * n,), dtype=torch.uint8, generator=g)
    rows = torch.randint(0, n_rows, (B * T,), dtype=torch.int64, generator=g)
    lut = torch.from_numpy(D.unit_range(np.arange(256, dtype=np.uint8)))
    err = torch.zeros(1, dtype=torch.int32).to(DEV)
    out = D.clip_gather(store.to(DEV)[offset:], rows.to(DEV), lut.to(DEV), shape, err)
    torch.cuda.synchronize()
    want = lut[store[offset:].reshape(n_rows, n)[rows].long()].reshape(shape)
    assert torch.equal(out.cpu(), want) and int(err.item()) == 0


def test_out_of_range_rows_are_clamped_and_flagged(tmp_path):
    """A row index outside [0, n_rows) is never dereferenced: the kernel clamps it (negative -> row 0, too large -> the last row),
    sets the error word, and the loader's per-epoch check raises."""
    from txt2vid_amd import data as D
    root, anno = make_tree(tmp_path)
    ds = D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=D.default_transform([32], 1), on_device=True)
    loader = D.get_loader(dset=ds, batch_size=2, device=DEV)
    loader.device_batch([0, 1])
    loader.check_rows()                                                  # nothing flagged by a good batch
    cache = loader.cache
    n_rows = cache.block.shape[0]
    rows = torch.tensor([0, n_rows + 1000, -7, n_rows - 1, 1 << 40, 5], dtype=torch.int64)
    out = D.clip_gather(cache.device_block, rows.to(DEV), cache.device_lut, (1, 6, 1, 32, 32), loader._err)
    torch.cuda.synchronize()
    clamped = [0, n_rows - 1, 0, n_rows - 1, n_rows - 1, 5]
    want = torch.from_numpy(cache.lut[np.asarray(cache.block)[clamped]].reshape(1, 6, 1, 32, 32))
    assert torch.equal(out.cpu(), want)
    with pytest.raises(RuntimeError, match='outside the frame cache'):
        loader.check_rows()
    loader.check_rows()                                                  # the flag was cleared by the raise
    with pytest.raises(RuntimeError):
        D.clip_gather(cache.device_block.cpu(), rows, cache.device_lut.cpu(), (1, 6, 1, 32, 32), loader._err.cpu())   # no CPU fallback


DRIVER = '''
import os, sys, torch
dump = sys.argv[1]
from txt2vid_amd.gan import samples
keep = samples.save_frames
def spy(x, path=None, **kw):
    if path and path.endswith('real_samples.png') and not os.path.exists(dump):
        torch.save(x.detach().cpu(), dump)                 # the xs[0] of the iteration that saved its examples
    return keep(x, path=path, **kw)
samples.save_frames = spy
from txt2vid_amd.train import gan
gan.main(gan.build_parser().parse_args(sys.argv[2:]))
'''


def test_cli_trains_on_device_frame_batches(tmp_path):
    """`python -m txt2vid_amd.train.gan` (its `main`, with `save_frames` wrapped to keep the tensor) on a JSON spec with
    `on_device`: 4 iterations under HIP-graph replay (eager warm-up, capture, replay — all fed by device batches), finite losses,
    and the `xs[0]` of iteration 1 equals the one the same command trains on through the host loader."""
    import re
    from PIL import Image
    rng = np.random.RandomState(5)
    root = tmp_path / 'videos'
    caps = {}
    words = ['digit', '3', 'is', 'left', 'and', 'right', 'top', 'bottom', '7']
    for v in range(12):
        d = root / ('clip%02d' % v)
        d.mkdir(parents=True)
        for n in range(16):
            Image.fromarray(rng.randint(0, 256, size=(70, 76)).astype(np.uint8)).save(d / ('%d.png' % n))
        caps['clip%02d' % v] = [' '.join(rng.choice(words, size=rng.randint(2, 7))) + '.' for _ in range(3)]
    anno = tmp_path / 'sent.pickle'
    with open(anno, 'wb') as f:
        pickle.dump(caps, f)
    driver = tmp_path / 'driver.py'
    driver.write_text(DRIVER)
    dumps, logs = {}, {}
    for kind in ('device', 'host'):
        spec = tmp_path / ('frames_%s.json' % kind)
        spec.write_text(json.dumps({'class': 'txt2vid.data.my_dataset',
                                    'args': {'data': str(root), 'num_frames': 16, 'on_device': kind == 'device'}}))
        dumps[kind] = str(tmp_path / ('xs0_%s.pt' % kind))
        cmd = [sys.executable, str(driver), dumps[kind], '--data', str(spec), '--anno', str(anno), '--num_channels', '1', '--cuda',
               '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002', '--D_lr', '0.0002',
               '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
               '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1',
               '--G', 'txt2vid.models.tganv2_cond.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim',
               '--sent', 'txt2vid.models.txt.basic.Seq2Seq', '--batch_size', '8', '--epochs', '2',
               '--out', str(tmp_path / ('out_' + kind)), '--out_samples', str(tmp_path / ('samples_' + kind)),
               '--max_iters', '4' if kind == 'device' else '1', '--save_model_period', '0', '--save_example_period', '1000',
               '--save_initial_examples']
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        logs[kind] = p.stdout.decode(errors='replace')
        assert p.returncode == 0, logs[kind][-3000:]
    log = logs['device']
    assert 'frame cache built' in log and '--workers is not used' in log and 'HIP-graph replay' in log
    assert 'frame cache' not in logs['host']
    m = re.findall(r'Iter (\d+), Loss_D: ([-0-9.naninf]+) Loss_G: ([-0-9.naninf]+)', log)
    assert [int(t[0]) for t in m] == [1, 2, 3, 4], log[-2000:]
    assert all(np.isfinite(float(v)) for t in m for v in t[1:]), m
    dev_x, host_x = torch.load(dumps['device']), torch.load(dumps['host'])
    assert dev_x.shape == (8, 1, 16, 8, 8) and torch.equal(dev_x, host_x)
    # ... and that tensor is the host loader's first batch: level 0 of the pyramid keeps every clip and frame (nearest resize)
    from txt2vid_amd import data as D
    host_ds = D.my_dataset(data=str(root), vocab=D.Vocab(), anno=str(anno), transform=D.default_transform([64], 1))
    firsts = {tuple(host_ds[i][0].permute(1, 0, 2, 3)[:, :, ::8, ::8].reshape(-1).tolist()) for i in range(len(host_ds))}
    assert all(tuple(dev_x[b].reshape(-1).tolist()) in firsts for b in range(8))
