"""CPU: the Kernel Inception Distance evaluation (`--eval_period`; DESIGN "KID evaluation") — the float64 restatement the GPU tests
compare against (its definition, a reordered evaluation against the derived bound, its power on a shifted Gaussian, the standard
error), the host-side refusals of `t2v_kid_sums`, the flags' rules, and the feature network's isolation from the host generators."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

import kid_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_textbook_double_loop():
    rng = np.random.default_rng(5)
    X, Y, alpha = rng.standard_normal((5, 3)), rng.standard_normal((5, 3)) + 0.3, 0.37
    k = lambda u, v: (alpha * sum(float(a) * float(b) for a, b in zip(u, v)) + 1.0) ** 3
    xx = sum(k(X[i], X[j]) for i in range(5) for j in range(5) if i != j)
    yy = sum(k(Y[i], Y[j]) for i in range(5) for j in range(5) if i != j)
    xy = sum(k(X[i], Y[j]) for i in range(5) for j in range(5))
    S = K.sums(X, Y, 5, alpha)
    assert S.shape == (1, 3) and np.allclose(S[0], [xx, yy, xy], rtol=1e-13, atol=0)
    kid, stderr = K.kid(X, Y, 5, alpha)
    assert stderr is None and abs(kid - (xx / 20 + yy / 20 - 2 * xy / 25)) < 1e-13 * (abs(xx) + abs(yy) + abs(xy))


@pytest.mark.parametrize('case', K.CASES + [K.LARGE_ALPHA] + K.TILED[:1], ids=K.case_id)
def test_a_reordered_float64_evaluation_sits_well_inside_the_bound(case):
    """16x16 tiles, k in chunks of 4: at most 5 % of the way to the bound, on every sum of every block."""
    X, Y, alpha = K.inputs(case)
    s, d = case[0], case[1]
    ratio = np.abs(K.tiled_sums(X, Y, s, alpha) - K.sums(X, Y, s, alpha)) / (K.op_bound(d, s) * K.magnitudes(X, Y, s, alpha))
    print('kid-restatement tiled/plain %s worst ratio %.4g' % (K.case_id(case), ratio.max()))
    assert ratio.max() <= 0.05


def test_fp32_anywhere_misses_the_bound_by_orders_of_magnitude():
    case = (64, 257, 1)
    X, Y, alpha = K.inputs(case)
    g32 = (np.float32(alpha) * (X @ Y.T) + np.float32(1)) ** 3                 # the x·y Gram in fp32
    err = abs(float(g32.astype(np.float64).sum()) - K.sums(X, Y, 64, alpha)[0, 2])
    assert err > 100 * K.op_bound(257, 64) * K.magnitudes(X, Y, 64, alpha)[0, 2]


def test_the_large_alpha_case_has_arguments_below_minus_one():
    X, Y, alpha = K.inputs(K.LARGE_ALPHA)
    arg = alpha * (X.astype(np.float64) @ Y.astype(np.float64).T) + 1.0
    assert alpha == 1.0 and arg.min() < -1 and arg.max() > 1
    S, M = K.sums(X, Y, 17, alpha), K.magnitudes(X, Y, 17, alpha)
    assert (np.abs(S) < 0.5 * M).all()                                      # terms of both signs cancel


def test_a_shifted_gaussian_is_told_apart_by_ten_standard_errors():
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((512, 64)), rng.standard_normal((512, 64))
    alpha = K.default_alpha(X)
    far, near = K.kid(X, Y + 0.5, 64, alpha), K.kid(X, Y, 64, alpha)
    print('kid shifted %.4f ± %.4f, same %.4f ± %.4f' % (far + near))
    assert far[0] - near[0] > 10 * max(far[1], near[1])
    assert abs(near[0]) < 3 * near[1]                                        # unbiased: zero within its error for one law


def test_one_block_has_no_standard_error_and_blocks_do_not_mix():
    X, Y, alpha = K.inputs((17, 33, 3))
    assert K.kid(X[:17], Y[:17], 17, alpha)[1] is None
    S = K.sums(X, Y, 17, alpha)
    for b in range(3):
        assert np.array_equal(S[b], K.sums(X[17 * b:17 * b + 17], Y[17 * b:17 * b + 17], 17, alpha)[0])
    ks = K.block_kids(S, 17)
    kid, stderr = K.estimate(S, 17)
    assert abs(kid - np.mean(ks)) < 1e-15 and abs(stderr - np.std(ks, ddof=1) / math.sqrt(3)) < 1e-15


def test_host_estimate_equals_the_restatement():
    from txt2vid_amd.functional_kid import estimate
    X, Y, alpha = K.inputs((3, 5, 2))
    S = K.sums(X, Y, 3, alpha)
    kid, stderr, ks = estimate(S.tolist(), 3)
    assert (kid, stderr) == K.estimate(S, 3) and ks == K.block_kids(S, 3)
    assert estimate(S[:1].tolist(), 3)[1] is None


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Host-side checks only: null pointers, n < 2, d < 1, s < 2, n % s != 0, s > n, a NaN alpha; the workspace query is 0 there."""
    from txt2vid_amd._lib import lib
    L = lib()
    p = C.c_void_p(64)                                               # never dereferenced: every call below is refused first
    ok = dict(X=p, Y=p, n=8, d=4, s=4, alpha=0.25, out=p, ws=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.t2v_kid_sums(a['X'], a['Y'], a['n'], a['d'], a['s'], a['alpha'], a['out'], a['ws'], None)
    for bad in (dict(X=None), dict(Y=None), dict(out=None), dict(ws=None), dict(n=1, s=1), dict(n=0), dict(n=-8), dict(d=0), dict(d=-1),
                dict(s=1), dict(s=0), dict(s=-4), dict(s=3), dict(s=16), dict(n=9, s=4), dict(alpha=float('nan'))):
        assert call(**bad) == -1, bad
    assert L.t2v_kid_sums_ws_bytes(8, 4, 4) == 2 * 3 * 8 and L.t2v_kid_sums_ws_bytes(2048, 1024, 1024) == 2 * 3 * 256 * 8
    assert L.t2v_kid_sums_ws_bytes(130, 7, 65) == 2 * 3 * 4 * 8
    for n, d, s in ((1, 4, 1), (8, 0, 4), (8, 4, 1), (8, 4, 3), (8, 4, 16), (0, 4, 2)):
        assert L.t2v_kid_sums_ws_bytes(n, d, s) == 0, (n, d, s)


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    from txt2vid_amd.functional_kid import kid_sums_raw, check_sizes
    with pytest.raises(RuntimeError):
        kid_sums_raw(torch.zeros(4, 3), torch.zeros(4, 3), 2, 1.0)
    for n, d, s in ((1, 4, 1), (8, 0, 4), (8, 4, 1), (8, 4, 3), (8, 4, 16)):
        with pytest.raises(ValueError, match='KID'):
            check_sizes(n, d, s)


# ------------------------------------------------------------------------------------------------ flags

def _args(*extra):
    from txt2vid_amd.train.gan import build_parser
    return build_parser().parse_args(['--data', 'x', '--G', 'g', '--D', 'd'] + list(extra))


def test_flags_default_to_off_and_the_block_defaults_to_min_m_1024():
    from txt2vid_amd.gan import kid
    a = _args()
    assert (a.eval_period, a.eval_clips, a.eval_block, a.eval_net) == (0, 2048, None, None)
    kid.check_args(a)                                                       # off: nothing is looked at
    assert a.eval_block is None
    a = _args('--eval_period', '5')
    kid.check_args(a, epoch_clips=lambda: 4096)
    assert a.eval_block == 1024
    a = _args('--eval_period', '5', '--eval_clips', '64')
    kid.check_args(a, epoch_clips=lambda: 64)
    assert a.eval_block == 64


def test_check_args_refusals():
    from txt2vid_amd.gan import kid
    with pytest.raises(ValueError, match='--eval_period'):
        kid.check_args(_args('--eval_period', '-1'))
    with pytest.raises(ValueError, match='multiple of --eval_block'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '10', '--eval_block', '4'))
    with pytest.raises(ValueError, match='exceeds the 8 clips of an epoch'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '16', '--eval_block', '8'), epoch_clips=lambda: 8)
    with pytest.raises(ValueError, match='at least 2'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '1', '--eval_block', '1'))
    with pytest.raises(ValueError, match='--end2end'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '8', '--end2end'))
    with pytest.raises(ValueError, match='no such file'):
        kid.check_args(_args('--eval_period', '2', '--eval_clips', '8', '--eval_net', '/nonexistent/ck'))
    # with the feature off none of the other flags is looked at
    kid.check_args(_args('--eval_clips', '10', '--eval_block', '4', '--end2end'))


def test_epoch_clips_counts_whole_batches_and_moves_no_generator():
    from txt2vid_amd.train.gan import _epoch_clips
    a = _args('--batch_size', '48')
    a.data = os.path.join(ROOT, 'tools', 'cfg', 'synth.json')
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    before = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state())
    assert _epoch_clips(a, 1) == 4096 // 48 * 48
    after = (random.getstate(), np.random.get_state()[1], torch.get_rng_state())
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and torch.equal(before[2], after[2])


# ------------------------------------------------------------------------------------------------ the feature network

def test_feature_network_is_a_constant_of_the_code_and_moves_no_generator():
    from txt2vid_amd.gan import kid
    from txt2vid_amd.models.resnet3d import Resnet3D
    from txt2vid_amd.util.torch.init import init
    torch.manual_seed(77)
    before = torch.get_rng_state()
    a, name = kid.feature_network(1, 'cpu')
    assert torch.equal(torch.get_rng_state(), before)
    torch.manual_seed(3)
    b, _ = kid.feature_network(1, 'cpu')
    torch.manual_seed(kid.FEATURE_SEED)
    c = Resnet3D(num_channels=1)
    init(c, init_method=kid.FEATURE_INIT)
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert list(sa) == list(sc) and all(torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sc[k]) for k in sa)
    assert not a.training and not any(p.requires_grad for p in a.parameters())
    assert not hasattr(a, 'fc') and not hasattr(a, 'proj') and not hasattr(a, 'mbstd')
    assert 'random-init' in name and str(kid.FEATURE_SEED) in name


def test_eval_net_takes_the_trunk_of_a_checkpoint_and_ignores_the_heads(tmp_path):
    from txt2vid_amd.gan import kid
    ref = os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint_uncond.pt')
    ck = torch.load(ref, map_location='cpu', weights_only=False)
    net, name = kid.feature_network(1, 'cpu', ref)
    sd = net.state_dict()
    for k, v in ck['video'].items():
        k = k[len('single_discrim.'):]
        if not k.startswith(kid.HEAD_KEYS):
            assert torch.equal(sd[k], v), k
    assert 'video' in name and 'ref_checkpoint_uncond.pt' in name
    # the text-conditioned key style, with head keys that the network does not have
    cond = {'single_discrim.module.' + k[len('single_discrim.'):]: v for k, v in ck['video'].items()}
    cond['single_discrim.module.fc.weight'] = torch.zeros(1, 1280)
    cond['single_discrim.module.proj.weight'] = torch.zeros(1024, 256)
    cond['single_discrim.module.mbstd.weight'] = torch.zeros(2)
    path = str(tmp_path / 'cond.pt')
    torch.save({'gen': {}, 'movie': cond}, path)
    net2, name2 = kid.feature_network(1, 'cpu', path)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values())) and 'movie' in name2
    with pytest.raises(ValueError, match='does not fit'):
        kid.feature_network(3, 'cpu', ref)
    torch.save({'gen': {}}, path)
    with pytest.raises(ValueError, match='no discriminator entry'):
        kid.feature_network(1, 'cpu', path)
