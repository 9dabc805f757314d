"""CPU: the host side of the sampling tool (`python -m txt2vid_amd.gan.sample`) — latents, captions, the numpy byte map
and top-K merge that the GPU tests compare the kernels with, the momentum recipe of the standing statistics, the flags' rules and
the argument validation of both entry points. No kernel is launched here."""
import argparse
import json
import math
import os

import numpy as np
import pytest
import torch

import sample_cases as SC
from txt2vid_amd import functional_sample as FS
from txt2vid_amd.gan import sample as S


# ---- latents ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tau', [0.05, 0.5, 1.0, 2.0])
def test_truncation_keeps_every_component_inside(tau):
    g, h = S.generators(3, 'cpu')
    z = S.draw_latents(16, 256, g, h, tau)
    assert z.shape == (16, 256) and z.dtype == torch.float32
    assert float(z.abs().max()) <= tau


def test_truncation_is_deterministic_and_inf_is_the_plain_draw():
    a = S.draw_latents(8, 64, *S.generators(11, 'cpu'), tau=0.7)
    b = S.draw_latents(8, 64, *S.generators(11, 'cpu'), tau=0.7)
    assert torch.equal(a, b)
    assert not torch.equal(a, S.draw_latents(8, 64, *S.generators(12, 'cpu'), tau=0.7))
    plain = S.draw_latents(8, 64, *S.generators(11, 'cpu'), tau=None)
    inf = S.draw_latents(8, 64, *S.generators(11, 'cpu'), tau=float('inf'))
    assert torch.equal(plain, inf)
    g = torch.Generator()
    g.manual_seed(11)
    assert torch.equal(plain, torch.randn(8, 64, generator=g))
    # components that were inside keep their value: only the outside ones are redrawn
    keep = plain.abs() <= 0.7
    assert torch.equal(a[keep], plain[keep])


def test_truncation_moves_no_global_generator():
    torch.manual_seed(5)
    before = torch.get_rng_state()
    S.draw_latents(4, 32, *S.generators(0, 'cpu'), tau=0.3)
    assert torch.equal(before, torch.get_rng_state())
    with pytest.raises(ValueError):
        S.draw_latents(4, 32, *S.generators(0, 'cpu'), tau=0.0)


@pytest.mark.parametrize('steps', [2, 3, 8])
def test_slerp_endpoints_and_norm(steps):
    g = torch.Generator()
    g.manual_seed(steps)
    a, b = torch.randn(256, generator=g), torch.randn(256, generator=g)
    z = S.slerp(a, b, steps)
    assert z.shape == (steps, 256) and z.dtype == torch.float32
    assert torch.equal(z[0], a) and torch.equal(z[-1], b)
    # equal-norm endpoints: the formula keeps the norm at every step
    b2 = b * (a.norm() / b.norm())
    z2 = S.slerp(a, b2, steps)
    rho = float(a.double().norm())
    for row in z2:
        assert abs(float(row.double().norm()) - rho) <= 1e-5 * rho
    # and the steps advance by equal angles
    if steps > 2:
        cos = [float((z2[i].double() * z2[i + 1].double()).sum()) / rho ** 2 for i in range(steps - 1)]
        assert max(cos) - min(cos) <= 1e-5
    with pytest.raises(ValueError):
        S.slerp(a, b, 1)


def test_slerp_of_parallel_endpoints_is_the_straight_line():
    a = torch.ones(8)
    z = S.slerp(a, 3 * a, 3)
    assert torch.equal(z[1], 2 * a)


# ---- captions --------------------------------------------------------------------------------------------------------------------
def test_captions_are_tokenised_cycled_and_sorted_for_the_encoder(tmp_path):
    from txt2vid_amd.data import Vocab
    vocab = Vocab()
    path = tmp_path / 'caps.txt'
    path.write_text('digit 3 is left and right.\n\ndigit 7 is top\n')
    args = argparse.Namespace(captions=str(path))
    toks = S.resolve_captions(args, True, None, vocab, 5)
    assert len(toks) == 5 and toks[0] == toks[2] == toks[4] and toks[1] == toks[3]
    assert toks[0] == [vocab(w) for w in ['<start>', 'digit', '3', 'is', 'left', 'and', 'right', '<end>']]
    assert toks[1] == [vocab(w) for w in ['<start>', 'digit', '7', 'is', 'top', '<end>']]            # <end> appended
    order, t, lengths = S.sorted_batch(toks)
    assert lengths == sorted(lengths, reverse=True) and t.shape == (5, 8) and t.dtype == torch.long
    for k, i in enumerate(order):
        assert t[k, :lengths[k]].tolist() == toks[i] and not t[k, lengths[k]:].any()
    assert sorted(order) == list(range(5))
    assert S.resolve_captions(argparse.Namespace(captions=None), False, None, vocab, 3) is None


def test_caption_defaults_come_from_the_dataset_by_index():
    from txt2vid_amd.data import SyntheticMovingDigits
    d = SyntheticMovingDigits(length=6, size=32)
    toks = S.resolve_captions(argparse.Namespace(captions=None), True, d, d.vocab, 4)
    assert toks == [[int(t) for t in d[i][1].tolist()] for i in range(4)]
    with pytest.raises(SystemExit):
        S.resolve_captions(argparse.Namespace(captions=None), True, None, d.vocab, 4)
    with pytest.raises(SystemExit):
        S.resolve_captions(argparse.Namespace(captions='x.txt'), False, d, d.vocab, 4)


# ---- the numpy byte map ------------------------------------------------------------------------------------------------------------
def test_byte_map_inverts_unit_range_on_all_256_bytes():
    assert np.array_equal(FS.byte_map(SC.unit_table()), np.arange(256, dtype=np.uint8))


def test_byte_map_rounds_half_to_even_and_clamps():
    x, k = SC.halfway()
    assert len(x) >= 100 and (k % 2 == 0).any() and (k % 2 == 1).any()
    got = FS.byte_map(x)
    assert np.array_equal(got, SC.halfway_bytes()) and (got % 2 == 0).all()
    assert FS.byte_map(np.float32(0.0)) == 128                                    # 127.5 exactly: the even neighbour
    assert FS.byte_map([-2, 2, np.inf, -np.inf, np.nan]).tolist() == [0, 255, 255, 0, 0]
    assert np.array_equal(FS.byte_map(SC.SPECIAL), SC.SPECIAL_BYTES)


def test_export_rows_is_the_frame_cache_layout():
    a = np.arange(2 * 3 * 2 * 2 * 2).reshape(2, 3, 2, 2, 2)
    rows = FS.export_rows(a)
    assert rows.shape == (4, 12)
    for b in range(2):
        for t in range(2):
            assert np.array_equal(rows[b * 2 + t], a[b, :, t].reshape(-1))


def test_export_inputs_hold_the_special_values():
    for shape in SC.EXPORT_SHAPES:
        x = SC.export_input(shape)
        assert x.shape == shape and x.dtype == np.float32
    big = SC.export_input((2, 1, 16, 64, 64)).reshape(-1)
    assert np.isnan(big).any() and np.isposinf(big).any() and np.isneginf(big).any() and (np.abs(big[np.isfinite(big)]) > 1).any()
    assert np.isin(SC.unit_table(), big).all() and np.isin(SC.halfway()[0], big).all()


# ---- the numpy top-K merge --------------------------------------------------------------------------------------------------------
def test_merge_orders_by_distance_then_index_across_three_merges():
    bd, bi = SC.empty_lists(2, 4)
    bd, bi = FS.nn_merge(bd, bi, [[5.0, 1.0], [2.0, 2.0]], 0)                     # more slots than candidates
    assert bd.tolist() == [[1.0, 5.0, np.inf, np.inf], [2.0, 2.0, np.inf, np.inf]]
    assert bi.tolist() == [[1, 0, -1, -1], [0, 1, -1, -1]]
    bd, bi = FS.nn_merge(bd, bi, [[1.0, 0.5, 7.0], [2.0, 9.0, 1.0]], 2)           # a tie with an earlier index: the lower index first
    assert bd.tolist() == [[0.5, 1.0, 1.0, 5.0], [1.0, 2.0, 2.0, 2.0]]
    assert bi.tolist() == [[3, 1, 2, 0], [4, 0, 1, 2]]
    bd, bi = FS.nn_merge(bd, bi, [[1.0, np.nan], [0.0, 2.0]], 5)                  # the list is full: the largest falls out; NaN never enters
    assert bd.tolist() == [[0.5, 1.0, 1.0, 1.0], [0.0, 1.0, 2.0, 2.0]]
    assert bi.tolist() == [[3, 1, 2, 5], [5, 4, 0, 1]]


def test_planted_clips_have_wide_gaps_and_the_bound_is_far_below_them():
    for (N, B, D) in [(3, 5, 4), (64, 64, 252), (64, 64, 260), (3, 64, 4)]:
        d2 = SC.nn_reference(N, B, D)
        assert d2.shape == (N, B) and SC.min_gap(d2) >= SC.MIN_GAP
    assert SC.min_gap(np.ones((3, 1))) == np.inf


# ---- the momentum recipe of the standing statistics ---------------------------------------------------------------------------------
def test_momentum_one_over_k_plus_one_is_torchs_cumulative_average():
    g = torch.Generator()
    g.manual_seed(29)
    xs = [torch.randn(4, 5, 6, 6, generator=g) * (k + 1) + k for k in range(4)]
    a = torch.nn.BatchNorm2d(5, momentum=None)
    b = torch.nn.BatchNorm2d(5)
    b.running_mean.fill_(3.0)                       # whatever the buffers held is gone after batch 0 (momentum 1)
    b.running_var.fill_(7.0)
    a.train()
    b.train()
    for k, x in enumerate(xs):
        a(x)
        b.momentum = 1.0 / (k + 1)
        b(x)
    means = torch.stack([x.mean(dim=(0, 2, 3)) for x in xs]).mean(0)
    vars_ = torch.stack([x.transpose(0, 1).reshape(5, -1).var(dim=1, unbiased=True) for x in xs]).mean(0)
    for got in (a, b):
        assert torch.allclose(got.running_mean, means, rtol=1e-5, atol=1e-6)
        assert torch.allclose(got.running_var, vars_, rtol=1e-5, atol=1e-6)
    assert torch.allclose(a.running_mean, b.running_mean, rtol=1e-6, atol=1e-7)
    assert torch.allclose(a.running_var, b.running_var, rtol=1e-6, atol=1e-7)


def test_standing_stats_sets_and_restores_modes_and_momenta_on_a_stub():
    """The driver alone, on a stand-in generator whose sites record what they saw (the kernels run in test_sample_gpu.py)."""
    from txt2vid_amd.models.layers import BatchNorm2d

    class Site(BatchNorm2d):
        def forward(self, x):
            self.seen.append((self.training, self.momentum))
            return x

    class Gen(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = Site(2), Site(2)
            self.render_blocks = [None, None]

        def forward(self, z, cond=None, output_blocks=None):
            assert not self.training and list(output_blocks) == [0, 1]
            return [self.b(self.a(z))]

    class Gan(object):
        def __init__(self):
            self.gen = Gen()

        def __call__(self, *a, **k):
            return self.gen(*a, **k)
    gan = Gan()
    gan.gen.eval()
    for m in (gan.gen.a, gan.gen.b):
        m.seen = []
    gan.gen.b.momentum = 0.25
    assert S.batchnorm_sites(gan.gen) == [gan.gen.a, gan.gen.b]
    from txt2vid_amd import functional as TF
    draws = TF.draws
    try:
        n = S.standing_stats(gan, [(torch.zeros(1), None, None)] * 3)
    finally:
        TF.set_draws(draws)
    assert n == 3
    assert gan.gen.a.seen == [(True, 1.0), (True, 0.5), (True, 1.0 / 3)] == gan.gen.b.seen
    assert (gan.gen.a.momentum, gan.gen.b.momentum) == (0.1, 0.25) and not gan.gen.a.training and not gan.gen.b.training


# ---- flags ------------------------------------------------------------------------------------------------------------------------
BASE = ['--data', 'd.json', '--G', 'g', '--D', 'd', '--weights', 'w.pt']


def parse(*extra):
    return S.build_parser().parse_args(BASE + list(extra))


def test_defaults_and_the_model_flags_of_train_gan():
    a = parse()
    assert (a.sample_n, a.sample_seed, a.captions, a.truncation, a.interp, a.standing_stats) == (16, 0, None, None, None, 0)
    assert (a.gif, a.export, a.nearest, a.nearest_clips, a.no_ema) == (False, None, 0, None, False)
    assert a.frame_sizes == [64] and a.G_ema == 0.0 and a.out_samples == 'out_samples'       # train.gan's flags, unchanged
    S.check_args(a)
    assert S.n_clips(parse('--sample_n', '6', '--interp', '5')) == 15


@pytest.mark.parametrize('extra, exc', [
    (['--sample_n', '0'], ValueError),
    (['--truncation', '0'], ValueError),
    (['--truncation', '-1'], ValueError),
    (['--interp', '1'], ValueError),
    (['--interp', '3', '--sample_n', '5'], ValueError),
    (['--standing_stats', '-1'], ValueError),
    (['--nearest', '9'], ValueError),
    (['--nearest', '-1'], ValueError),
    (['--nearest', '2', '--sample_n', '65'], ValueError),
    (['--nearest', '2', '--sample_n', '32', '--interp', '5'], ValueError),
    (['--nearest', '2', '--nearest_clips', '0'], ValueError),
    (['--captions', 'c.txt', '--dont_use_sent'], SystemExit),
])
def test_flag_rules(extra, exc):
    with pytest.raises(exc):
        S.check_args(parse(*extra))


def test_weights_are_required():
    a = S.build_parser().parse_args(BASE[:-2])
    with pytest.raises(SystemExit):
        S.check_args(a)
    with pytest.raises(SystemExit):
        S.main(BASE[:-2])


def test_records_round_trip_through_json(tmp_path):
    a = parse('--sample_seed', '7', '--truncation', '0.8', '--export', str(tmp_path / 'clips'))
    rec = S.export_record(a, (3, 16, 64, 64), 4, ['a b', 'c'], 12)
    S.write_json(a.export + '.json', rec)
    with open(a.export + '.json') as f:
        back = json.load(f)
    assert back == rec
    assert (back['N'], back['T'], back['C'], back['H'], back['W']) == (4, 16, 3, 64, 64)
    assert back['seed'] == 7 and back['truncation'] == 0.8 and back['iteration'] == 12 and back['captions'] == ['a b', 'c']
    assert '127.5' in back['byte_map'] and 'unit_range' in back['byte_map']
    rec2 = {'iteration': 3, 'weights': 'gen_ema', 'seed': 0, 'truncation': None, 'standing_stats': 2, 'captions': None,
            'files': ['sample_0.png'], 'nearest': [[{'index': 4, 'd2': 1.5, 'rms': math.sqrt(1.5 / 8)}]]}
    S.write_json(str(tmp_path / S.SAMPLES_FILE), rec2)
    with open(str(tmp_path / S.SAMPLES_FILE)) as f:
        assert json.load(f) == rec2


def test_gif_is_written_from_exported_rows(tmp_path):
    from PIL import Image
    rows = (np.arange(4 * 3 * 8 * 8) % 251).astype(np.uint8).reshape(4, 3 * 8 * 8)
    for C, name in ((1, 'g.gif'), (3, 'c.gif')):
        S.write_gif(str(tmp_path / name), rows[:, :C * 64], C, 8, 8)
        with Image.open(str(tmp_path / name)) as im:
            assert im.n_frames == 4 and im.size == (8, 8)


# ---- the entry points refuse bad arguments before any launch -----------------------------------------------------------------------
def test_entry_points_validate_without_gpu():
    import ctypes as C
    from txt2vid_amd._lib import lib
    L = lib()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert L.t2v_clip_export(None, 1, 1, 1, 8, 8, p, None) < 0
    assert L.t2v_clip_export(p, 1, 1, 1, 8, 8, None, None) < 0
    assert L.t2v_clip_export(p, 0, 1, 1, 8, 8, p, None) < 0
    assert L.t2v_clip_export(p, 1, 1, 1, 8, 0, p, None) < 0
    assert L.t2v_clip_export(p, 1, 1, 1, 65536, 65536, p, None) < 0                 # H*W above 2^31 - 1
    assert L.t2v_clip_export(p, 65536, 65536, 1, 1, 1, p, None) < 0                 # B*C*T above 2^31 - 1
    ok = dict(N=2, B=2, D=8, base=0, K=2)

    def nn(g=p, r=p, bd=p, bi=p, ws=p, **kw):
        a = dict(ok, **kw)
        return L.t2v_clip_nn(g, a['N'], r, a['B'], a['D'], a['base'], a['K'], bd, bi, ws, None)
    for kw in (dict(g=None), dict(r=None), dict(bd=None), dict(bi=None), dict(ws=None), dict(N=0), dict(N=65), dict(B=0), dict(B=65),
               dict(K=0), dict(K=9), dict(D=0), dict(D=6), dict(D=3 * 16 * 128 * 128 + 4), dict(base=-1)):
        assert nn(**kw) == -1, kw
    assert L.t2v_clip_nn_ws_bytes(65, 1, 8) < 1 and L.t2v_clip_nn_ws_bytes(1, 1, 6) < 1 and L.t2v_clip_nn_ws_bytes(1, 0, 8) < 1
    assert L.t2v_clip_nn_ws_bytes(64, 64, 3 * 16 * 128 * 128 + 4) < 1
    assert L.t2v_clip_nn_chain(6) < 1 and L.t2v_clip_nn_chain(0) < 1
    # the plan: one chain per slab, the same slab up to the benchmark clip, at most 512 slabs at the largest
    slab = FS.nn_chain(65536)
    assert slab % 4 == 0 and FS.nn_chain(4) == 4 and FS.nn_chain(slab - 4) == slab - 4 and FS.nn_chain(slab + 4) == slab
    assert FS.nn_slabs(slab - 4) == 1 and FS.nn_slabs(slab + 4) == 2 and FS.nn_slabs(65536) == 65536 // slab
    assert L.t2v_clip_nn_ws_bytes(3, 5, 65536) == FS.nn_slabs(65536) * 3 * 5 * 4
    big = 3 * 16 * 128 * 128
    assert FS.nn_slabs(big) <= 512 and FS.nn_chain(big) * FS.nn_slabs(big) >= big
    assert 0 < FS.nn_gamma(big) < 1e-4 and FS.nn_gamma(4) == (1 + 2.0 ** -24) ** 6 - 1 + 2.0 ** -53
    with pytest.raises(ValueError):
        FS.nn_chain(6)


def test_wrappers_refuse_host_tensors():
    with pytest.raises(RuntimeError):
        FS.clip_export(torch.zeros(1, 1, 1, 8, 8))
    with pytest.raises(RuntimeError):
        FS.clip_nn(torch.zeros(1, 8), torch.zeros(1, 8), 0, torch.zeros(1, 1, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.int64))
