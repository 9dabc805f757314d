"""CPU: the LeCam regularisation of the discriminator (--D_lecam) — the flags' rules, the state's layout and its way
through a checkpoint, its place among the extras of a run and in the read-out, the log line, the float64 restatement
(tests/lecam_cases.py) against a hand-computed example, and the entry points' refusals (no device is touched)."""
import argparse
import ctypes as C
import re

import numpy as np
import pytest
import torch

import lecam_cases as LC

F32 = np.float32
# the line test_lecam_gpu parses: iteration, lambda, R, gate, the anchors of the real and of the generated logits
LINE = re.compile(r'Iter (\d+), LeCam \(--D_lecam (\S+)\): R (\S+), gate ([01]), real ((?:\S+ ?)+), fake ((?:\S+ ?)+)$')


# ------------------------------------------------------------------------------------------------ flags
def _parser():
    from txt2vid_amd.gan.trainer import add_params_to_parser
    p = add_params_to_parser(argparse.ArgumentParser())
    p.add_argument('--D_names', type=str, nargs='+', default=None)
    return p


def _parse(argv, world=1):
    from txt2vid_amd.gan.lecam import check_args
    return check_args(_parser().parse_args(argv), world=world)


def test_flags_parse_and_default_to_off():
    a = _parse([])
    assert a.D_lecam is None and a.D_lecam_decay is None and a.D_lecam_start is None
    a = _parse(['--D_lecam', '0.3'])
    assert (a.D_lecam, a.D_lecam_decay, a.D_lecam_start) == (0.3, 0.99, 0)
    a = _parse(['--D_lecam', '0.3', '--D_lecam_decay', '0', '--D_lecam_start', '1000', '--D_names', 'video'])
    assert (a.D_lecam, a.D_lecam_decay, a.D_lecam_start) == (0.3, 0.0, 1000)
    text = ' '.join(_parser().format_help().split())
    assert '--D_lecam LAMBDA' in text and 'tuned' in text and '0.3' in text

    class Bare(object):                                   # a parameter object without the attributes means "off"
        pass
    from txt2vid_amd.gan.lecam import check_args
    check_args(Bare(), world=2)


@pytest.mark.parametrize('argv', [['--D_lecam_decay', '0.9'], ['--D_lecam_start', '3'], ['--D_lecam_decay', '0.9', '--D_lecam_start', '0']])
def test_decay_and_start_need_the_weight(argv):
    with pytest.raises(ValueError, match='--D_lecam LAMBDA'):
        _parse(argv)


@pytest.mark.parametrize('argv', [['--D_lecam', '0.3', '--D_lecam_decay', '1'], ['--D_lecam', '0.3', '--D_lecam_decay', '-0.1'],
                                  ['--D_lecam', '0.3', '--D_lecam_decay', 'nan'], ['--D_lecam', '0.3', '--D_lecam_start', '-1'],
                                  ['--D_lecam', 'inf'], ['--D_lecam', '0.3', '--D_names', 'a', 'b']])
def test_out_of_range_values_raise(argv):
    with pytest.raises(ValueError):
        _parse(argv)


@pytest.mark.parametrize('bad', ['0', '-0.3', 'nan'])
def test_a_weight_that_is_not_positive_is_an_argparse_error(bad, capsys):
    with pytest.raises(SystemExit):
        _parse(['--D_lecam', bad])
    assert '--D_lecam' in capsys.readouterr().err


def test_data_parallel_refusal():
    with pytest.raises(ValueError, match='data-parallel'):
        _parse(['--D_lecam', '0.3'], world=2)
    _parse([], world=2)


# ------------------------------------------------------------------------------------------------ state and checkpoint
class _Module(torch.nn.Module):
    def __init__(self):
        super(_Module, self).__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))


def _gan(lecam):
    from txt2vid_amd.gan.cond_gan import CondGan
    gan = CondGan(gen=_Module(), discrims=[_Module()], discrim_names=['video'])
    assert gan.lecam is None
    gan.lecam = lecam
    return gan


def test_state_layout_and_round_trip_through_a_checkpoint():
    from txt2vid_amd.gan import lecam as M
    a = M.LeCamState(0.3, decay=0.9, start=5)
    assert (M.N_STATE, M.A_R, M.A_F) == (20, 4, 12) == (LC.N_STATE, LC.A_R, LC.A_F)
    assert a.lecam.dtype == torch.float32 and a.lecam.tolist() == [0.0] * 20
    assert (a.lam, a.decay, a.start, a.key) == (0.3, 0.9, 5, None)
    assert [(n, t is a.lecam, k) for n, t, k in a.slots] == [('lecam', True, 20)]
    vals = [7, 0.25, 1, 4] + [0.5, -0.5, 1.5, 2.5, 0, 0, 0, 0] + [-1, -2, -3, -4, 0, 0, 0, 0]
    a.lecam.copy_(torch.tensor(vals, dtype=torch.float32))
    saved = _gan(a).save_dict()
    assert saved['lecam']['lecam'].dtype == torch.float32 and saved['lecam']['lecam'].device.type == 'cpu'
    assert saved['lecam']['lecam'].tolist() == vals
    # key and state: restored, in place (a captured graph keeps the address)
    b = M.LeCamState(0.3)
    ptr = b.lecam.data_ptr()
    _gan(b).load_from_dict(saved)
    assert b.lecam.tolist() == vals and b.lecam.data_ptr() == ptr
    # no key: a fresh start, whatever the state held
    plain = _gan(None).save_dict()
    assert 'lecam' not in plain
    _gan(b).load_from_dict(plain)
    assert b.lecam.tolist() == [0.0] * 20 and b.lecam.data_ptr() == ptr
    # a key without the feature: ignored
    g = _gan(None)
    g.load_from_dict(saved)
    assert g.lecam is None
    for bad in (dict(lam=0.0), dict(lam=-1.0), dict(lam=float('nan')), dict(lam=0.3, decay=1.0), dict(lam=0.3, decay=-0.5),
                dict(lam=0.3, start=-1)):
        with pytest.raises(ValueError):
            M.LeCamState(**bad)
    with pytest.raises(ValueError):
        b.load_state_dict({'lecam': torch.zeros(8)})
    with pytest.raises(RuntimeError):
        b.term([torch.zeros(4, 1)], [torch.zeros(4, 1)])            # no CPU fallback
    with pytest.raises(ValueError):
        b.term([torch.zeros(4, 1)], [])
    with pytest.raises(ValueError):
        b.term([torch.zeros(1, 1)] * 9, [torch.zeros(1, 1)] * 9)


# ------------------------------------------------------------------------------------------------ the seam
class _Stub(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_extras_order_with_the_new_member():
    from txt2vid_amd.gan.extras import training_extras
    ada, lecam, guard = object(), object(), object()
    lr = _Stub(counters=lambda: {'D': 8, 'G': 4}, spi={'D': 2, 'G': 1}, it0=0)
    opts = [_Stub(lr_sched=_Stub(sched=lr), grad_guard=_Stub(guard=guard)) for _ in range(2)]
    none = [_Stub(lr_sched=None, grad_guard=None) for _ in range(2)]
    assert training_extras(_Stub(ada=ada, lecam=lecam), *opts) == [ada, lecam, lr, guard]
    assert training_extras(_Stub(ada=None, lecam=lecam), *opts) == [lecam, lr, guard]
    assert training_extras(_Stub(ada=ada, lecam=lecam), *none) == [ada, lecam]
    assert training_extras(_Stub(ada=ada, lecam=None), *opts) == [ada, lr, guard]
    assert training_extras(_Stub(ada=ada), *opts) == [ada, lr, guard]             # a gan without the attribute at all
    assert training_extras(_Stub(ada=None), *none) == []


def test_readout_offsets_and_width_with_the_new_slot():
    from txt2vid_amd.gan.ada import AdaState
    from txt2vid_amd.gan.extras import Readout
    from txt2vid_amd.gan.grad_guard import GradGuard
    from txt2vid_amd.gan.lecam import LeCamState
    lecam = LeCamState(0.3)
    r = Readout([lecam], 'cpu')
    assert [(name, off, n) for name, off, n, t in r.slots] == [('lD', 0, 1), ('lG', 1, 1), ('kl', 2, 1), ('lecam', 3, 20)]
    assert r.width == 24
    r = Readout([AdaState(0.6, p0=0.25), lecam, GradGuard(2.0, None)], 'cpu')
    assert [(name, off, n) for name, off, n, t in r.slots] == [('lD', 0, 1), ('lG', 1, 1), ('kl', 2, 1), ('ada.p', 3, 1),
                                                                ('lecam', 4, 20), ('guard.D', 24, 6), ('guard.G', 30, 6)]
    assert r.width == 36
    # the values travel by name, one push late
    lecam.lecam[1], lecam.lecam[3], lecam.lecam[4], lecam.lecam[12] = 0.5, 1.0, 0.25, -0.25
    for k in (1, 2):
        r.push(k, lD=torch.tensor(1.0), lG=torch.tensor(2.0))
    got = r.pop()
    assert got['lecam'] == lecam.lecam.tolist() and got['ada.p'] == [0.25]


def test_log_line_is_the_one_the_gpu_test_parses():
    from txt2vid_amd.gan.lecam import LeCamState
    s = LeCamState(0.3, decay=0.9)
    assert s.log_lines(2, {}) == []                                 # nothing read yet: nothing to say
    v = [5.0, 0.123456789, 1.0, 2.0] + [0.5, -0.25] + [0.0] * 6 + [-1.0, 2.0] + [0.0] * 6
    line, = s.log_lines(2, {'lecam': v})
    assert line == 'Iter 2, LeCam (--D_lecam 0.3): R 0.123457, gate 1, real 0.5000 -0.2500, fake -1.0000 2.0000'
    m = LINE.search(line)
    assert m and m.group(1, 2, 3, 4) == ('2', '0.3', '0.123457', '1')
    assert [float(t) for t in m.group(5).split()] == [0.5, -0.25] and [float(t) for t in m.group(6).split()] == [-1.0, 2.0]
    line, = s.log_lines(1, {'lecam': [0.0] * 20})                   # a state no step has written yet: no levels
    assert line.startswith('Iter 1, LeCam (--D_lecam 0.3): R 0, gate 0')


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_against_a_hand_computed_example():
    """L = 1, two pairs, decay 0.5. Step 1 (n = 0, anchors 0): R = mean(1, 9) + mean(1, 1) = 6, gate 0, anchors <- the means
    (2, 0). Step 2: R = mean(2^2, 4^2) + mean((0 - 2)^2, (2 - 2)^2) = 12, gate 1, anchors <- (0.5 * 2 + 0.5 * 3, 0.5 * 0 + 0.5 * 1);
    dR/du_r = 2 (u_r - 0) / 2 = (2, 4), dR/du_f = 2 (u_f - 2) / 2 = (-2, 0)."""
    s0 = LC.init_state()
    out, s1 = LC.step(s0, [np.array([1.0, 3.0])], [np.array([-1.0, 1.0])], 0.5, 0)
    assert out == 0.0 and s1[:4].tolist() == [1.0, 6.0, 0.0, 1.0] and (s1[LC.A_R], s1[LC.A_F]) == (2.0, 0.0)
    assert not s0.any()                                             # the input state is left as it was
    gr, gf = LC.grads(s0, [np.array([1.0, 3.0])], [np.array([-1.0, 1.0])], 0)
    assert gr[0].tolist() == [0.0, 0.0] and gf[0].tolist() == [0.0, 0.0]
    s1 = s1.astype(F32)
    u_r, u_f = [torch.tensor([[2.0], [4.0]])], [torch.tensor([[0.0], [2.0]])]
    out, s2 = LC.step(s1, u_r, u_f, 0.5, 0)
    assert out == 12.0 and s2[:4].tolist() == [2.0, 12.0, 1.0, 1.0] and (s2[LC.A_R], s2[LC.A_F]) == (2.5, 0.5)
    assert not s2[LC.A_R + 1:LC.A_F].any() and not s2[LC.A_F + 1:].any()
    gr, gf = LC.grads(s1, u_r, u_f, 0, g=1.0)
    assert gr[0].tolist() == [2.0, 4.0] and gf[0].tolist() == [-2.0, 0.0]
    assert LC.grads(s1, u_r, u_f, 0, g=0.5)[0][0].tolist() == [1.0, 2.0]
    # start = 2: the second step (n = 1) is still ungated; R_last holds the ungated value, the anchors move all the same
    out, s2b = LC.step(s1, u_r, u_f, 0.5, 2)
    assert out == 0.0 and s2b[:4].tolist() == [2.0, 12.0, 0.0, 1.0] and (s2b[LC.A_R], s2b[LC.A_F]) == (2.5, 0.5)
    assert LC.grads(s1, u_r, u_f, 2)[1][0].tolist() == [0.0, 0.0]
    # two levels: the mean over levels, every level against its own anchors
    s = LC.init_state()
    s[0], s[LC.A_R], s[LC.A_R + 1], s[LC.A_F], s[LC.A_F + 1] = 3, 1, 2, -1, -2
    out, t = LC.step(s, [np.array([1.0]), np.array([0.0, 2.0])], [np.array([0.0]), np.array([2.0, 4.0])], 0.0, 0)
    assert out == ((4 + 1) + ((4 + 16) / 2 + (0 + 4) / 2)) / 2 and t[3] == 2 and t[0] == 4
    assert (t[LC.A_R], t[LC.A_R + 1], t[LC.A_F], t[LC.A_F + 1]) == (1.0, 1.0, 0.0, 3.0)       # decay 0: the means themselves


# ------------------------------------------------------------------------------------------------ argument checks
def test_entry_points_validate_without_a_device():
    """Bad arguments are refused on the host side (negative status) before any launch; no device is touched. The pointers are
    never dereferenced on the refused paths, so host addresses stand in for device ones."""
    from txt2vid_amd._lib import lib, AdaLevel, LecamGrad, MAX_GROUPS
    l = lib()
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)

    def levels(kind, n=1, **kw):
        arr = (kind * max(1, n))()
        for a in arr:
            a.real, a.fake, a.count = addr, addr, 4
            for k, v in kw.items():
                setattr(a, k, v)
        return arr
    f = l.t2v_lecam_fwd
    ok = dict(state=addr, lv=levels(AdaLevel), n=1, decay=0.5, start=0, saved=addr, out=addr)
    for bad in (dict(state=None), dict(lv=None), dict(saved=None), dict(out=None), dict(n=0), dict(n=-1),
                dict(lv=levels(AdaLevel, MAX_GROUPS + 1), n=MAX_GROUPS + 1), dict(lv=levels(AdaLevel, count=0)),
                dict(lv=levels(AdaLevel, count=-4)), dict(lv=levels(AdaLevel, real=None)), dict(lv=levels(AdaLevel, fake=None)),
                dict(decay=1.0), dict(decay=-0.5), dict(decay=float('nan')), dict(decay=float('inf')), dict(start=-1)):
        a = dict(ok, **bad)
        assert f(a['state'], a['lv'], a['n'], a['decay'], a['start'], a['saved'], a['out'], None) < 0, bad
    b = l.t2v_lecam_bwd
    ok = dict(lv=levels(LecamGrad, d_real=addr, d_fake=addr), n=1, saved=addr, g=addr)
    for bad in (dict(lv=None), dict(saved=None), dict(g=None), dict(n=0), dict(lv=levels(LecamGrad, MAX_GROUPS + 1), n=MAX_GROUPS + 1),
                dict(lv=levels(LecamGrad, count=0, d_real=addr)), dict(lv=levels(LecamGrad, real=None, d_real=addr)),
                dict(lv=levels(LecamGrad, fake=None, d_fake=addr))):
        a = dict(ok, **bad)
        assert b(a['lv'], a['n'], a['saved'], a['g'], None) < 0, bad
    assert b(levels(LecamGrad), 1, addr, addr, None) == 0           # no side needs a gradient: accepted, nothing launched
    assert C.sizeof(LecamGrad) == 40 and C.sizeof(AdaLevel) == 24
