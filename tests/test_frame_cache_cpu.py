"""CPU: the HBM frame cache's host side — `FrameCache` (what is stored, the 256-entry table, save / load, refusals) and
`DeviceFrameLoader.plan` / `epoch_order` (order parity with the host DataLoader) — against the host `Dataset` path, which
tests/test_data_cpu.py pins to the reference. Every bound here is exact equality: the cache stores the bytes PIL produced and the
table is computed with the host transform's own expression, so there is no rounding to allow for."""
import json

import numpy as np
import pytest
import torch

from frame_cases import make_tree, make_golden_tree
from txt2vid_amd import data as D

CROPS = [([64], 3), ([48, 56], 3), ([64], 1), ([30], 1)]


def dataset(tree, crop, channels, random_frames=0, **kw):
    root, anno = tree
    return D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=D.default_transform(crop, channels),
                        random_frames=random_frames, num_frames=16, **kw)


def cached_frames(cache, rows):
    """lut[cache rows] as the [T,C,h,w] float32 clip the host item is."""
    return cache.lut[np.asarray(cache.block)[list(rows)]].reshape(len(rows), cache.channels, cache.crop[0], cache.crop[1])


@pytest.mark.parametrize('crop,channels', CROPS)
def test_cache_rows_equal_host_items_bit_for_bit(tmp_path, crop, channels):
    ds = dataset(make_tree(tmp_path), crop, channels)
    assert len(ds) == 6 and ds.missing == 1
    cache = D.FrameCache.build(ds)
    assert cache.lut.dtype == np.float32 and cache.lut.shape == (256,) and cache.block.dtype == np.uint8
    assert cache.block.shape == (4 * 16, channels * cache.crop[0] * cache.crop[1])         # only the strided pick is stored
    assert cache.rows_of('vid0') == (0, 16) and len(cache.table) == 4                       # two captions share vid0's rows
    for i in range(len(ds)):
        first, count = cache.rows_of(ds.video_ids[i])
        host = ds[i][0].numpy()
        got = cached_frames(cache, range(first, first + count))
        assert got.dtype == np.float32 and np.array_equal(got, host), i
    assert float(ds[5][0][0, 0, 0, 0]) == -1.0 or crop == [30]                              # vid3 is 30x30: zero fill outside


@pytest.mark.parametrize('crop,channels', [([64], 3), ([30], 1)])
def test_cache_keeps_every_frame_for_random_picks(tmp_path, crop, channels):
    ds = dataset(make_tree(tmp_path), crop, channels, random_frames=8)
    cache = D.FrameCache.build(ds)
    assert [cache.rows_of('vid%d' % v)[1] for v in range(4)] == [40, 33, 40, 20] and cache.block.shape[0] == 133
    for i in range(len(ds)):
        first, count = cache.rows_of(ds.video_ids[i])
        np.random.seed(100 + i)
        host = ds[i][0].numpy()
        np.random.seed(100 + i)
        rows = D.pick_frames(range(first, first + count), num_frames=8, random=True)
        assert np.array_equal(cached_frames(cache, rows), host), i


def test_cache_equals_the_reference_fixture(golden, tmp_path):
    """tests/golden/data_contract.npz: frames the REAL reference's data module produced (`ds_frames_<i>`), the bound
    test_input_pipeline_vs_reference_fixture holds the host path to — `np.array_equal`."""
    g = golden('data_contract')
    root, anno, (h, w) = make_golden_tree(g, tmp_path)
    vocab = D.build_vocab([str(s) for s in g['sentences']])
    ds = D.Dataset(video_dir=root, vocab=vocab, captions=anno, transform=D.default_transform([h, w], 1))
    assert len(ds) == int(g['ds_len'])
    cache = D.FrameCache.build(ds)
    for i in range(len(ds)):
        first, count = cache.rows_of(ds.video_ids[i])
        assert count == 16
        assert np.array_equal(cached_frames(cache, range(first, first + count)), g['ds_frames_%d' % i]), i
    loader = D.DeviceFrameLoader(ds, cache, len(ds), 'cuda:0', shuffle=False)
    rows, tokens, lengths = loader.plan(range(len(ds)))
    assert np.array_equal(cached_frames(cache, rows.reshape(-1).tolist()).reshape(g['collate_vids'].shape), g['collate_vids'])
    assert np.array_equal(tokens.numpy(), g['collate_targets']) and lengths == list(g['collate_lengths'])


@pytest.mark.parametrize('random_frames', [0, 8])
def test_plans_follow_the_host_dataloader_batch_by_batch(tmp_path, random_frames):
    """Two epochs from the same generator states: sampler draws (torch), frame picks (np.random) and the caption sort (captions of
    equal length: stable) — the device loader's plans name exactly the host loader's batches."""
    tree = make_tree(tmp_path)
    ds = dataset(tree, [32], 3, random_frames=random_frames)
    torch.manual_seed(7)
    np.random.seed(7)
    host_loader = D.get_loader(dset=ds, batch_size=2, num_workers=0)
    host = [[b for b in host_loader] for _ in range(2)]
    after = (torch.get_rng_state(), np.random.get_state()[1].copy())
    torch.manual_seed(7)
    np.random.seed(7)
    dev_ds = dataset(tree, [32], 3, random_frames=random_frames, on_device=True)
    loader = D.get_loader(dset=dev_ds, batch_size=2, num_workers=0, device='cuda:0')        # (no GPU is touched before iteration)
    assert isinstance(loader, D.DeviceFrameLoader) and len(loader) == len(host_loader) == 3
    cache = loader.cache
    orders = []
    for epoch in range(2):
        order = loader.epoch_order()
        orders.append(order)
        for k in range(len(loader)):
            rows, tokens, lengths = loader.plan(order[2 * k:2 * k + 2])
            hv, ht, hl = host[epoch][k]
            assert rows.dtype == torch.int64 and rows.shape == (2, random_frames or 16)
            got = cached_frames(cache, rows.reshape(-1).tolist()).reshape(hv.shape)
            assert np.array_equal(got, hv.numpy()), (epoch, k)
            assert tokens.dtype == torch.int64 and torch.equal(tokens, ht) and lengths == hl, (epoch, k)
    assert orders[0] != orders[1] and sorted(orders[0]) == list(range(6))
    assert torch.equal(torch.get_rng_state(), after[0]) and np.array_equal(np.random.get_state()[1], after[1])


def test_two_ranks_walk_the_distributed_sampler(tmp_path):
    tree = make_tree(tmp_path)
    seen = []
    for rank in range(2):
        ds = dataset(tree, [32], 1, on_device=True)
        loader = D.get_loader(dset=ds, batch_size=1, rank=rank, world=2, seed=5, device='cuda:0')
        host = D.get_loader(dset=dataset(tree, [32], 1), batch_size=1, num_workers=0, rank=rank, world=2, seed=5)
        assert isinstance(loader, D.DeviceFrameLoader) and len(loader) == 3
        epochs = []
        for epoch in range(2):
            loader.sampler.set_epoch(epoch)
            host.sampler.set_epoch(epoch)
            order = loader.epoch_order()
            assert order == [int(i) for i in host.sampler]
            epochs.append(order)
        assert epochs[0] != epochs[1]                          # set_epoch changes the order
        seen.append(epochs[0])
    assert not set(seen[0]) & set(seen[1]) and sorted(seen[0] + seen[1]) == list(range(6))


def test_save_load_round_trip_and_refusals(tmp_path):
    tree = make_tree(tmp_path)
    ds = dataset(tree, [48, 56], 3)
    cache = D.FrameCache.build(ds)
    path = cache.save(str(tmp_path / 'frames'))
    assert path.endswith('frames.npy')
    back = D.FrameCache.load(path, ds)
    assert isinstance(back.block, np.memmap) and np.array_equal(np.asarray(back.block), cache.block)
    assert back.table == cache.table and back.crop == cache.crop and back.channels == cache.channels
    assert np.array_equal(back.lut, cache.lut)
    side = json.load(open(path + '.json'))
    assert side['crop'] == [48, 56] and side['channels'] == 3 and set(side['listing']) == {'vid0', 'vid1', 'vid2', 'vid3'}
    with pytest.raises(ValueError, match='crop'):
        D.FrameCache.load(path, dataset(tree, [64], 3))                                      # another crop size
    with pytest.raises(ValueError, match='channels'):
        D.FrameCache.load(path, dataset(tree, [48, 56], 1))
    with pytest.raises(ValueError, match='all_frames'):
        D.FrameCache.load(path, dataset(tree, [48, 56], 3, random_frames=8))
    (tmp_path / 'other').mkdir()
    with pytest.raises(ValueError, match='listing'):
        D.FrameCache.load(path, dataset(make_tree(tmp_path / 'other', frames=(40, 33, 40, 21)), [48, 56], 3))   # another folder
    # a transform that is not default_transform's: refused, not served from the host behind the caller's back
    root, anno = tree
    other = D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=lambda img: torch.zeros(1, 4, 4), on_device=True)
    with pytest.raises(ValueError, match='default_transform'):
        D.FrameCache.build(other)
    with pytest.raises(ValueError, match='default_transform'):
        D.get_loader(dset=other, batch_size=2, device='cuda:0')
    with pytest.raises(RuntimeError) as e:
        cache.to('cuda:0', max_bytes=1000)                                                   # refused before anything is uploaded
    assert str(cache.nbytes) in str(e.value) and '1000' in str(e.value)
    with pytest.raises(RuntimeError) as e:
        cache.to('cuda:0', max_bytes=-(4 << 30))              # what "free - reserve" gives on a card that is already full
    assert str(cache.nbytes) in str(e.value)


def test_factory_cache_file_and_command_line(tmp_path):
    """`my_dataset(on_device=, cache_file=)` records both; `python -m txt2vid_amd.data.cache` writes the file a later run loads;
    without `on_device` or without a CUDA device every loader is what it was."""
    from txt2vid_amd.data import cache as cache_cli
    from txt2vid_amd.util.reflection import create_object
    root, anno = make_tree(tmp_path)
    out = str(tmp_path / 'cache' / 'c.npy')
    (tmp_path / 'cache').mkdir()
    assert cache_cli.main(['--data', root, '--anno', anno, '--frame_size', '32', '--num_channels', '1', '--out', out]) == 0
    spec = tmp_path / 'frames_on_device.json'
    spec.write_text(json.dumps({'class': 'txt2vid.data.my_dataset', 'args': {'data': root, 'on_device': True, 'cache_file': out}}))
    ds = create_object(str(spec), vocab=D.Vocab(), anno=anno, transform=D.default_transform([32], 1), size=32, channels=1, seed=0)
    assert isinstance(ds, D.Dataset) and ds.on_device is True and ds.cache_file == out
    loader = D.get_loader(dset=ds, batch_size=2, device='cuda:0')
    assert isinstance(loader, D.DeviceFrameLoader) and loader.cache.source.startswith('loaded from')
    assert np.array_equal(cached_frames(loader.cache, range(16)), ds[0][0].numpy())
    assert isinstance(D.get_loader(dset=ds, batch_size=2, device='cpu'), torch.utils.data.DataLoader)
    plain = D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=D.default_transform([32], 1))
    assert plain.on_device is False and isinstance(D.get_loader(dset=plain, batch_size=2, device='cuda:0'), torch.utils.data.DataLoader)
    # a cache_file that does not exist yet is written by the first run
    fresh = str(tmp_path / 'cache' / 'fresh.npy')
    ds2 = D.my_dataset(data=root, vocab=D.Vocab(), anno=anno, transform=D.default_transform([32], 1), on_device=True, cache_file=fresh)
    assert D.get_loader(dset=ds2, batch_size=2, device='cuda:0').cache.source == 'built'
    assert np.array_equal(np.load(fresh), np.load(out))
