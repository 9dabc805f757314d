"""CPU: the opt-in averaged generator (--G_ema) — ABI declarations, the command line and the checkpoint key logic.
No kernel is launched here: `GenAverage`'s construction and `state_dict` / `load_state_dict` are host-only code."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 't2v_hip.h')
SO = os.path.join(ROOT, 'txt2vid_amd', 'csrc', 'libt2v_hip.so')
NEW = ('t2v_ema_multi', 't2v_ema_tick', 't2v_swap_multi')


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(SO):
        subprocess.check_call(['make', '-C', os.path.dirname(SO), '-j4'])
    return SO


def test_entry_points_declared_bound_and_exported(built):
    from txt2vid_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(', txt))
    exported = set(re.findall(r'\bT\s+(t2v_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', '--defined-only', built]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert name in exported, name
    assert _lib.SIGNATURES['t2v_ema_multi'] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                                ctypes.c_float, ctypes.c_void_p]


def test_job_struct_mirror_matches_header():
    """sizeof(t2v_ema_job) computed from the header's field list (pointers and int64_t only: no padding) == the ctypes mirror."""
    from txt2vid_amd._lib import EmaJob
    m = re.search(r'typedef\s+struct\s+t2v_ema_job\s*\{(.*?)\}\s*t2v_ema_job\s*;', open(HEADER).read(), flags=re.S)
    assert m
    fields = [f.strip() for f in m.group(1).split(';') if f.strip()]
    size = {'void*': ctypes.sizeof(ctypes.c_void_p), 'const void*': ctypes.sizeof(ctypes.c_void_p), 'int64_t': 8}
    parsed = [(f.rsplit(' ', 1)[0].strip(), f.rsplit(' ', 1)[1]) for f in fields]
    assert [n for _, n in parsed] == [n for n, _ in EmaJob._fields_] == ['e', 'p', 'n']
    assert sum(size[t] for t, _ in parsed) == ctypes.sizeof(EmaJob) == 24
    assert ctypes.sizeof(EmaJob) * 64 + 4 * (64 + 65 + 1) < 4096          # 64 jobs by value stay under the kernel-argument limit


def test_argument_validation_without_gpu(built):
    """T2V_EINVAL before any launch: null job list, no jobs, null pointers, n < 1, n > INT_MAX, null count."""
    from txt2vid_amd._lib import lib, EmaJob
    l = lib()
    buf = (ctypes.c_float * 8)()
    addr = ctypes.addressof(buf)

    def job(e, p, n):
        arr = (EmaJob * 1)()
        arr[0].e, arr[0].p, arr[0].n = e, p, n
        return arr
    bad = [job(None, addr, 8), job(addr, None, 8), job(addr, addr, 0), job(addr, addr, -1), job(addr, addr, 2 ** 31)]
    for arr in bad:
        assert l.t2v_ema_multi(arr, 1, 0.5, 0.0, None, 1.0, None) == -1
        assert l.t2v_swap_multi(arr, 1, None) == -1
    assert l.t2v_ema_multi(None, 1, 0.5, 0.0, None, 1.0, None) == -1
    assert l.t2v_ema_multi(job(addr, addr, 8), 0, 0.5, 0.0, None, 1.0, None) == -1
    assert l.t2v_swap_multi(None, 1, None) == -1
    assert l.t2v_swap_multi(job(addr, addr, 8), 0, None) == -1
    assert l.t2v_ema_tick(None, None) == -1


def test_command_line_flags():
    from txt2vid_amd.train.gan import build_parser
    need = ['--data', 'd.json', '--G', 'g', '--D', 'd']
    a = build_parser().parse_args(need)
    assert a.G_ema == 0 and a.G_ema_start == 0
    a = build_parser().parse_args(need + ['--G_ema', '0.999', '--G_ema_start', '100'])
    assert a.G_ema == 0.999 and a.G_ema_start == 100
    for bad in ('1.0', '-0.1'):
        with pytest.raises(SystemExit):
            build_parser().parse_args(need + ['--G_ema', bad])
    with pytest.raises(SystemExit):
        build_parser().parse_args(need + ['--G_ema=-0.1'])


def _gan(with_average, **kw):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    gen, dis = MultiScaleGen(width=64, height=64, num_channels=1), MultiScaleDiscrim(num_channels=1)
    if with_average:
        from txt2vid_amd.gan.ema import GenAverage
        kw['gen_ema'] = GenAverage(gen, 0.999)
    return CondGan(gen=gen, discrims=[dis], discrim_names=['video'], **kw)


def test_average_state_is_laid_out_like_the_parameters():
    gan = _gan(True)
    ema, gen = gan.gen_ema, gan.gen
    named = dict(gen.named_parameters())
    sd = ema.state_dict()
    assert list(sd) == [k for k, _ in gen.named_parameters()]                  # parameters by name, no BatchNorm buffers
    assert not any('running_' in k or 'num_batches' in k for k in sd)
    tap_major = 0
    for k, e in sd.items():
        p = named[k]
        assert e.shape == p.shape and e.stride() == p.stride() and e.dtype == torch.float32, k
        assert e.data_ptr() != p.data_ptr() and torch.equal(e, p.detach()), k
        tap_major += not p.is_contiguous()
    assert tap_major == 8                                                       # the ConvLSTM's tap-major master copies
    assert ema.updates == 0
    from txt2vid_amd.gan.ema import GenAverage
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            GenAverage(gen, bad)
    with pytest.raises(RuntimeError):
        ema.update()                             # host tensors: the kernels have no CPU fallback
    with pytest.raises(RuntimeError):
        with ema.swapped():
            pass


def test_checkpoint_keys_with_and_without_an_average():
    plain = _gan(False)
    assert plain.gen_ema is None
    assert set(plain.save_dict()) == {'gen', 'video'}
    gan = _gan(True)
    saved = gan.save_dict()
    assert set(saved) == {'gen', 'video', 'gen_ema', 'gen_ema_updates'}
    assert saved['gen_ema_updates'] == 0
    assert list(saved['gen_ema']) == [k for k, _ in gan.gen.named_parameters()]
    # round trip: averaged tensors and the count arrive; a run without an average ignores the keys
    for e in gan.gen_ema.avg:
        e.add_(1.0)
    gan.gen_ema.count.fill_(7.0)
    saved = {k: (dict((n, t.clone()) for n, t in v.items()) if isinstance(v, dict) else v) for k, v in gan.save_dict().items()}
    assert saved['gen_ema_updates'] == 7
    other = _gan(True)
    other.load_from_dict(saved)
    assert other.gen_ema.updates == 7
    for (k, e), p in zip(other.gen_ema.state_dict().items(), other.gen.parameters()):
        assert torch.equal(e, saved['gen_ema'][k]) and e.stride() == p.stride(), k
        assert torch.equal(e, p.detach() + 1.0), k
    plain.load_from_dict(saved)
    assert plain.gen_ema is None
    # missing keys fall back to the live parameter
    partial = dict(saved['gen_ema'])
    dropped = next(iter(partial))
    del partial[dropped]
    other.gen_ema.load_state_dict(partial, updates=3)
    assert torch.equal(other.gen_ema.state_dict()[dropped], dict(other.gen.named_parameters())[dropped].detach())
    assert other.gen_ema.updates == 3
    with pytest.raises(KeyError):
        other.gen_ema.load_state_dict({'no.such.weight': torch.zeros(1)})


def test_reference_checkpoint_without_the_key_leaves_a_copy_of_gen():
    """tests/golden/ref_checkpoint_uncond.pt was written by the reference: no `gen_ema`. The average becomes a copy of the LOADED
    generator (not of the weights it was constructed from)."""
    gan = _gan(True)
    for p in gan.gen.parameters():
        p.data.fill_(123.0)
    for e in gan.gen_ema.avg:
        e.fill_(-5.0)
    gan.gen_ema.count.fill_(9.0)
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint_uncond.pt'), weights_only=False, map_location='cpu')
    assert 'gen_ema' not in ck
    gan.load_from_dict(ck)
    named = dict(gan.gen.named_parameters())
    for k, e in gan.gen_ema.state_dict().items():
        assert torch.equal(e, named[k].detach()), k
        assert torch.equal(e, ck['gen'][k].contiguous()), k
    assert gan.gen_ema.updates == 0
