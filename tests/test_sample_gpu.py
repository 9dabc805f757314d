"""GPU: the sampling tool's device passes and the tool itself (`python -m txt2vid_amd.gan.sample`).
`t2v_clip_export` is compared with numpy's float32 byte map for EQUALITY, `t2v_clip_nn` with the float64 distances within the
derived bound gamma (sample_cases.py) and for exact indices, the standing statistics with the CPU oracle generator driven the same
way, and the tool runs end to end on the reference's own checkpoints as tests/test_cli_gpu.py runs commands."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_cases as SC
from txt2vid_amd import functional_sample as FS
from txt2vid_amd.gan import sample as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'


# ---- export ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SC.EXPORT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_export_equals_the_numpy_byte_map(shape):
    x = SC.export_input(shape)
    want = FS.export_rows(FS.byte_map(x))
    got = FS.clip_export(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    # into a buffer of the caller's, twice: the same bytes
    out = torch.empty_like(got)
    assert FS.clip_export(torch.from_numpy(x).to(DEV), out=out) is out and torch.equal(out, got)


def test_export_takes_the_scalar_path_from_an_unaligned_base():
    x = SC.export_input((3, 3, 2, 8, 8))
    buf = torch.empty(x.size + 1, device=DEV, dtype=torch.float32)
    view = buf[1:].view(x.shape)                                                   # 4 bytes past a 16-byte boundary
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4
    assert np.array_equal(FS.clip_export(view).cpu().numpy(), FS.export_rows(FS.byte_map(x)))


@pytest.mark.parametrize('shape', [(2, 1, 16, 64, 64), (3, 3, 2, 8, 8), (2, 3, 2, 5, 6)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_gather_then_export_returns_the_block(shape):
    from txt2vid_amd import functional as TF
    from txt2vid_amd.data import clip_gather
    B, C, T, H, W = shape
    rng = np.random.default_rng(291)
    block = rng.integers(0, 256, size=(B * T, C * H * W), dtype=np.uint8)
    block.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                      # every byte value is there
    cache = torch.from_numpy(block).to(DEV).reshape(-1)
    lut = torch.from_numpy(SC.unit_table()).to(DEV)
    rows = torch.arange(B * T, dtype=torch.int64).to(DEV)
    err = torch.zeros(1, dtype=torch.int32).to(DEV)
    clips = clip_gather(cache, rows, lut, (B, T, C, H, W), err)                    # [B,T,C,H,W]
    back = FS.clip_export(TF.video_to_channel_first(clips))
    assert int(err.item()) == 0 and np.array_equal(back.cpu().numpy(), block)


# ---- nearest real clips ------------------------------------------------------------------------------------------------------------
def _slab():
    return FS.nn_chain(SC.NN_BIG_D)


def _run(g, r, K, base=0, lists=None):
    gd, rd = torch.from_numpy(np.ascontiguousarray(g)).to(DEV), torch.from_numpy(np.ascontiguousarray(r)).to(DEV)
    bd, bi = FS.nn_init(g.shape[0], K, DEV) if lists is None else lists
    FS.clip_nn(gd, rd, base, bd, bi)
    return bd, bi


def _check(bd, bi, want_d, want_i, D):
    bd, bi = bd.cpu().numpy(), bi.cpu().numpy()
    assert np.array_equal(bi, want_i)
    live = want_i >= 0
    assert np.isposinf(bd[~live]).all()
    gamma = FS.nn_gamma(D)
    err = np.abs(bd[live] - want_d[live])
    print('D = %d: gamma %.3e, largest relative error %.3e' % (D, gamma, float((err / np.maximum(want_d[live], 1e-300)).max()) if err.size else 0.0))
    assert (err <= gamma * want_d[live]).all()


def test_nn_plan_has_the_sizes_the_cases_assume():
    slab = _slab()
    assert slab >= 8 and FS.nn_slabs(slab - 4) == 1 and FS.nn_slabs(slab + 4) == 2 and FS.nn_slabs(SC.NN_BIG_D) > 1


@pytest.mark.parametrize('D', ['4', 'slab-4', 'slab+4', '65536'])
@pytest.mark.parametrize('B', SC.NN_B)
@pytest.mark.parametrize('N', SC.NN_N)
def test_nn_distances_within_gamma_and_indices_exact(N, B, D):
    D = {'4': 4, 'slab-4': _slab() - 4, 'slab+4': _slab() + 4, '65536': SC.NN_BIG_D}[D]
    g, r = SC.nn_inputs(N, B, D)
    d2 = SC.nn_reference(N, B, D)
    gap = SC.min_gap(d2)
    assert gap >= SC.MIN_GAP and gap > 1e3 * 2 * FS.nn_gamma(D)                   # the reference's ordering is not in question
    for K in SC.NN_K:
        want_d, want_i = FS.nn_merge(*SC.empty_lists(N, K), d2, 0)
        bd, bi = _run(g, r, K)
        _check(bd, bi, want_d, want_i, D)
        if K > B:
            assert (bi[:, B:] == -1).all().item() and torch.isinf(bd[:, B:]).all().item()
        bd2, bi2 = _run(g, r, K)                                                   # no atomics: the same bits
        assert torch.equal(bd, bd2) and torch.equal(bi, bi2)


def test_nn_duplicates_ties_and_streaming():
    """Three calls of 3 clips with consecutive bases into 8 slots: an exact duplicate of a sample, two identical clips inside one
    call and two across calls, against ONE numpy merge of the 9 candidates."""
    N, B, D, K = 3, 3, _slab() + 4, 8
    g, r9 = SC.nn_inputs(N, 3 * B, D)
    r = [np.array(r9[c * B:(c + 1) * B]) for c in range(3)]
    r[0][1] = g[2]                                                                 # an exact duplicate of sample 2 at index 1
    r[1][2] = r[1][1]                                                              # two identical real clips: indices 4 and 5
    r[2][0] = r[0][2]                                                              # and one equal to an earlier clip: indices 2 and 6
    d_all = np.concatenate([SC.d2_ref(g, rc) for rc in r], axis=1)
    assert (d_all[:, 4] == d_all[:, 5]).all() and (d_all[:, 2] == d_all[:, 6]).all() and d_all[2, 1] == 0.0
    for n in range(N):                                                             # apart from the planted ties the gaps stay wide
        assert SC.min_gap(np.unique(d_all[n])[None]) >= SC.MIN_GAP
    lists = FS.nn_init(N, K, DEV)
    want = SC.empty_lists(N, K)
    for c, rc in enumerate(r):
        lists = _run(g, rc, K, base=c * B, lists=lists)
        want = FS.nn_merge(*want, SC.d2_ref(g, rc), c * B)
        if c == 0:                                                                 # 3 candidates in 8 slots
            assert (lists[1][:, B:] == -1).all().item() and torch.isinf(lists[0][:, B:]).all().item()
            assert (lists[1][:, :B] >= 0).all().item()
    one = FS.nn_merge(*SC.empty_lists(N, K), d_all, 0)
    assert np.array_equal(want[0], one[0]) and np.array_equal(want[1], one[1])      # three merges = one merge
    bd, bi = lists[0].cpu().numpy(), lists[1].cpu().numpy()
    assert np.array_equal(bi, one[1])
    assert bi[2, 0] == 1 and bd[2, 0] == 0.0                                       # the duplicate: exactly zero
    assert (np.abs(bd - one[0]) <= FS.nn_gamma(D) * one[0]).all()
    pairs = 0
    for n in range(N):                                                             # equal distances: the lower index first, adjacent
        row = bi[n].tolist()
        for lo, hi in ((4, 5), (2, 6)):
            if hi in row:
                assert row.index(hi) == row.index(lo) + 1 and bd[n, row.index(lo)] == bd[n, row.index(hi)]
                pairs += 1
    assert pairs >= N                                                              # (8 of 9 candidates stay: at most one pair is cut per row)


def test_nn_refuses_what_the_header_refuses():
    g = torch.zeros(2, 8, device=DEV)
    with pytest.raises(ValueError):
        FS.clip_nn(g, torch.zeros(2, 12, device=DEV), 0, *FS.nn_init(2, 2, DEV))
    with pytest.raises(ValueError):
        FS.clip_nn(torch.zeros(2, 6, device=DEV), torch.zeros(2, 6, device=DEV), 0, *FS.nn_init(2, 2, DEV))
    with pytest.raises(ValueError):
        FS.clip_nn(g, g, 0, *FS.nn_init(2, 9, DEV))
    with pytest.raises(ValueError):
        FS.clip_nn(torch.zeros(65, 8, device=DEV), g, 0, *FS.nn_init(65, 2, DEV))


# ---- standing statistics -----------------------------------------------------------------------------------------------------------
class _Gan(object):
    """What the tool's forward needs of a CondGan: the generator and the call."""

    def __init__(self, gen):
        self.gen, self.gen_ema = gen, None

    def __call__(self, *a, **k):
        return self.gen(*a, **k)


def _gen():
    from oracle import tganv2_oracle as O
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    m = MultiScaleGen(width=64, height=64, num_channels=1)
    m.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.to(DEV)


def _buffers(gen):
    return {k: v.detach().clone() for k, v in gen.state_dict().items() if k.endswith('running_mean') or k.endswith('running_var')}


def test_standing_statistics_match_the_oracle_and_restore_the_modules():
    gen = _gen()
    gen.train()
    gan = _Gan(gen)
    sites = S.batchnorm_sites(gen)
    assert len(sites) == 16
    sites[3].momentum = 0.25
    before = _buffers(gen)
    zs = SC.standing_latents()
    # without the recomputation a sampling forward leaves the buffers as they are, bit for bit
    with S.sampling(gan):
        out = S.forward(gan, zs[0].to(DEV))
        assert len(out) == 1 and tuple(out[-1].shape) == (2, 1, 16, 64, 64)
    after = _buffers(gen)
    assert all(torch.equal(before[k], after[k]) for k in before)
    with S.sampling(gan):
        assert S.standing_stats(gan, [(z.to(DEV), None, None) for z in zs]) == 3
        assert not gen.training and not any(m.training for m in sites)
        assert [m.momentum for m in sites] == [0.1] * 3 + [0.25] + [0.1] * 12
    assert gen.training and all(m.training for m in sites)                          # sampling() gives the mode back
    want = SC.oracle_standing(zs)
    got = _buffers(gen)
    assert sorted(want) == sorted(got) and len(got) == 32
    worst = 0.0
    for k in sorted(want):
        a, b = got[k].cpu().double().numpy(), want[k].double().numpy()
        scale = max(1.0, float(np.abs(b).max()))
        worst = max(worst, float((np.abs(a - b) / (SC.BUF_ATOL * scale + SC.BUF_RTOL * np.abs(b))).max()))
        assert not torch.equal(got[k], before[k])
    print('standing statistics: largest error / tolerance over 32 buffers: %.3f' % worst)
    for k in sorted(want):
        b = want[k].double().numpy()
        np.testing.assert_allclose(got[k].cpu().double().numpy(), b, rtol=SC.BUF_RTOL, atol=SC.BUF_ATOL * max(1.0, float(np.abs(b).max())))


# ---- the tool, end to end ----------------------------------------------------------------------------------------------------------
COMMON = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
          '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--workers', '0', '--batch_size', '8']
UNCOND = COMMON + ['--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
                   '--dont_use_sent']
COND = COMMON + ['--G', 'txt2vid.models.tganv2_cond.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim',
                 '--sent_weights', os.path.join(GOLD, 'ref_seq2seq.pt')]
FULL = ['--sample_n', '4', '--truncation', '1.0', '--standing_stats', '2', '--gif', '--nearest', '2', '--nearest_clips', '16']


def _cfg(tmp):
    cfg = os.path.join(str(tmp), 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    return cfg


def _tool(module, args, tmp):
    p = subprocess.run([sys.executable, '-m', module, '--data', _cfg(tmp)] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    return out


def _sample(args, tmp, name):
    out = os.path.join(str(tmp), name)
    log = _tool('txt2vid_amd.gan.sample', args + ['--out_samples', out, '--export', os.path.join(out, 'clips')], tmp)
    with open(os.path.join(out, S.SAMPLES_FILE)) as f:
        rec = json.load(f)
    return out, log, rec


def _check_full(out, rec, C=1):
    for name in ['sample_0.png', 'clips.npy', 'clips.json', S.SAMPLES_FILE] + ['sample_%d.gif' % i for i in range(4)] + \
            ['nearest_%d.png' % i for i in range(4)]:
        assert os.path.exists(os.path.join(out, name)), name
    a = np.load(os.path.join(out, 'clips.npy'))
    assert a.dtype == np.uint8 and a.shape == (4 * 16, C * 64 * 64) and a.min() < a.max()
    with open(os.path.join(out, 'clips.json')) as f:
        meta = json.load(f)
    assert (meta['N'], meta['T'], meta['C'], meta['H'], meta['W']) == (4, 16, C, 64, 64)
    assert meta['seed'] == 0 and meta['truncation'] == 1.0 and meta['iteration'] == rec['iteration']
    assert rec['seed'] == 0 and rec['truncation'] == 1.0 and rec['standing_stats'] == 2 and rec['clips'] == 4
    assert len(rec['nearest']) == 4
    for row in rec['nearest']:
        assert len(row) == 2 and row[0]['d2'] <= row[1]['d2'] and all(0 <= e['index'] < 16 for e in row)
        assert all(abs(e['rms'] - (e['d2'] / (C * 16 * 64 * 64)) ** 0.5) < 1e-12 for e in row)
    return a


def test_tool_on_the_reference_unconditional_checkpoint(tmp_path):
    base = UNCOND + ['--weights', os.path.join(GOLD, 'ref_checkpoint_uncond.pt')]
    out, log, rec = _sample(base + FULL, tmp_path, 'a')
    assert 'sampling from the live weights' in log and rec['weights'] == 'gen' and rec['captions'] is None
    assert 'standing statistics: 16 BatchNorm sites' in log
    a = _check_full(out, rec)
    assert not os.path.exists(os.path.join(out, S.CAPTIONS_FILE))
    out2, _, rec2 = _sample(base + FULL, tmp_path, 'b')                             # the same seed: the same bytes
    assert np.array_equal(np.load(os.path.join(out2, 'clips.npy')), a) and rec2['nearest'] == rec['nearest']
    # --nearest only reads: with it and without it (no standing statistics either way) the export is the same
    plain = ['--sample_n', '4', '--truncation', '1.0']
    out3, _, rec3 = _sample(base + plain, tmp_path, 'c')
    out4, _, rec4 = _sample(base + plain + ['--nearest', '2', '--nearest_clips', '16'], tmp_path, 'd')
    c, d = np.load(os.path.join(out3, 'clips.npy')), np.load(os.path.join(out4, 'clips.npy'))
    assert np.array_equal(c, d) and rec3['nearest'] is None and len(rec4['nearest']) == 4
    assert not glob.glob(os.path.join(out3, 'nearest_*.png')) and not glob.glob(os.path.join(out3, '*.gif'))
    assert not np.array_equal(a, c)                                                # the recomputed buffers do change the clips


def test_tool_on_the_reference_conditional_checkpoint_with_typed_captions(tmp_path):
    caps = tmp_path / 'caps.txt'
    caps.write_text('digit 3 is left and right.\ndigit 7 is top and bottom\n')
    base = COND + ['--weights', os.path.join(GOLD, 'ref_checkpoint_cond.pt'), '--captions', str(caps)]
    out, log, rec = _sample(base + FULL, tmp_path, 'a')
    _check_full(out, rec)
    want = ['<start> digit 3 is left and right<end>', '<start> digit 7 is top and bottom<end>'] * 2
    assert rec['captions'] == want
    with open(os.path.join(out, S.CAPTIONS_FILE)) as f:
        assert f.read().splitlines() == want
    with open(os.path.join(out, 'clips.json')) as f:
        assert json.load(f)['captions'] == want


def test_tool_samples_the_averaged_generator_of_a_checkpoint_that_holds_one(tmp_path):
    out_dir = str(tmp_path / 'out')
    train = UNCOND + ['--G_lr', '0.0002', '--D_lr', '0.0002', '--discrim_steps', '1', '--gp_lambda', '.5', '--subsample_input',
                      '--log_period', '1', '--epochs', '1', '--out', out_dir, '--out_samples', str(tmp_path / 'smp'),
                      '--max_iters', '3', '--save_model_period', '3', '--save_example_period', '0', '--G_ema', '0.9']
    _tool('txt2vid_amd.train.gan', train, tmp_path)
    ck = glob.glob(os.path.join(out_dir, 'iter_3_lossG_*'))
    assert len(ck) == 1 and 'gen_ema' in torch.load(ck[0], map_location='cpu', weights_only=False)
    out, log, rec = _sample(UNCOND + ['--weights', ck[0], '--sample_n', '2'], tmp_path, 'e')
    assert 'sampling from the averaged generator (3 updates)' in log and rec['weights'] == 'gen_ema' and rec['iteration'] == 3
    out2, log2, rec2 = _sample(UNCOND + ['--weights', ck[0], '--sample_n', '2', '--no_ema'], tmp_path, 'f')
    assert 'sampling from the live weights (--no_ema)' in log2 and rec2['weights'] == 'gen'
    a, b = np.load(os.path.join(out, 'clips.npy')), np.load(os.path.join(out2, 'clips.npy'))
    assert a.shape == b.shape == (2 * 16, 64 * 64) and not np.array_equal(a, b)
