"""CPU: the opt-in spectral normalisation of the discriminator (--D_sn) — the float64 reference of tests/sn_cases.py
against `torch.nn.utils.spectral_norm`, ABI declarations and argument validation, the command line, key names and refusals.
No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

import sn_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 't2v_hip.h')
SO = os.path.join(ROOT, 'txt2vid_amd', 'csrc', 'libt2v_hip.so')
NEW = ('t2v_sn_ws_floats', 't2v_sn_refresh', 't2v_sn_project')


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(SO):
        subprocess.check_call(['make', '-C', os.path.dirname(SO), '-j4'])
    return SO


# ---- the reference math ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['conv3d', 'linear'])
def test_reference_matches_torch_spectral_norm(kind):
    """One training forward and backward of `torch.nn.utils.spectral_norm` in float64: its weight, u, v equal one `refresh_ref`
    from its state before the forward, and the gradient of `weight_orig` equals `project_ref` of dL/dWhat. The closed form and
    autograd through `sn_weight` agree too."""
    torch.manual_seed(5)
    if kind == 'conv3d':
        m = nn.utils.spectral_norm(nn.Conv3d(3, 5, 3, padding=1).double())
        x = torch.randn(2, 3, 4, 6, 6, dtype=torch.float64)
        fwd = lambda w: torch.nn.functional.conv3d(x, w, m.bias.detach(), padding=1)
    else:
        m = nn.utils.spectral_norm(nn.Linear(37, 11).double())
        x = torch.randn(4, 37, dtype=torch.float64)
        fwd = lambda w: torch.nn.functional.linear(x, w, m.bias.detach())
    m.train()
    W, u0 = m.weight_orig.detach().clone(), m.weight_u.detach().clone()
    y = m(x)
    r = torch.randn_like(y)
    (y * r).sum().backward()
    v, u, sigma, What = S.refresh_ref(W, u0)
    assert torch.allclose(u, m.weight_u, rtol=0, atol=1e-14)
    assert torch.allclose(v, m.weight_v, rtol=0, atol=1e-14)
    assert torch.allclose(What.reshape(W.shape), m.weight.detach(), rtol=0, atol=1e-13)
    leaf = What.reshape(W.shape).clone().requires_grad_(True)
    (fwd(leaf) * r).sum().backward()
    dW = S.project_ref(leaf.grad, What, u, v, sigma)
    err = float((dW - m.weight_orig.grad).abs().max())
    print('%s: max |dL/dW - torch| = %.3g' % (kind, err))
    assert err < 1e-12
    Wl = W.clone().requires_grad_(True)
    (fwd(S.sn_weight(Wl, u, v)) * r).sum().backward()
    assert float((Wl.grad - m.weight_orig.grad).abs().max()) < 1e-12


def test_reference_iteration_converges_to_the_largest_singular_value():
    """W = 3 a b^T + noise, sigma_2 <= sigma_1 / 2: 30 float64 refreshes are within 1e-6 relative of `torch.linalg.svdvals`."""
    for (M, K), seed in zip([(67, 129), (96, 2600)], (1, 2)):
        W, u = S.low_rank_case(M, K, seed)
        sv = torch.linalg.svdvals(W.double())
        assert float(sv[1]) <= 0.5 * float(sv[0])
        _, _, sigma, _ = S.refresh_ref(W, u, n_iter=30)
        rel = abs(sigma - float(sv[0])) / float(sv[0])
        print('[%d, %d]: sigma %.9f, svdvals %.9f, relative %.3g' % (M, K, sigma, float(sv[0]), rel))
        assert rel < 1e-6


def test_zero_matrix_reference_is_finite():
    v, u, sigma, What = S.refresh_ref(torch.zeros(5, 7), torch.ones(5) / 5 ** 0.5)
    assert sigma == 0.0 and not v.any() and not u.any() and not What.any()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported(built):
    from txt2vid_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(', txt))
    exported = set(re.findall(r'\bT\s+(t2v_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', '--defined-only', built]).decode()))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert int(re.search(r'#define\s+T2V_SN_MAX_JOBS\s+(\d+)', txt).group(1)) == _lib.SN_MAX_JOBS


def test_job_struct_mirror_matches_header():
    from txt2vid_amd._lib import SnJob, SN_MAX_JOBS
    m = re.search(r'typedef\s+struct\s+t2v_sn_job\s*\{(.*?)\}\s*t2v_sn_job\s*;', open(HEADER).read(), flags=re.S)
    assert m
    names = re.findall(r'(\w+)\s*[;,]', m.group(1))
    assert names == [n for n, _ in SnJob._fields_] == ['w', 'what', 'u', 'v', 'sigma', 'g', 'M', 'K']
    assert ctypes.sizeof(SnJob) == 6 * 8 + 2 * 4
    # by value in the kernel arguments: 6 pointers + M, K, workspace offset per job and four begin tables
    assert SN_MAX_JOBS * (6 * 8 + 3 * 4) + 4 * 4 * (SN_MAX_JOBS + 1) + 4 < 4096 - 64


def test_argument_validation_without_gpu(built):
    """T2V_EINVAL before any launch: null job list, no jobs, more jobs than a call holds, null pointers, M < 1, K < 1,
    M K > INT_MAX, no / too small a workspace, n_iter < 1, eps <= 0, a projection without a gradient."""
    from txt2vid_amd._lib import lib, SnJob, SN_MAX_JOBS
    l = lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def jobs(n=1, **kw):
        arr = (SnJob * n)()
        for j in arr:
            j.w, j.what, j.u, j.v, j.sigma, j.g, j.M, j.K = a, a, a, a, a, a, 2, 3
            for k, val in kw.items():
                setattr(j, k, val)
        return arr
    good = jobs()
    need = l.t2v_sn_ws_floats(good, 1)
    assert need >= 1 * 3 + 3 + 1 + 2 + 1 + 1            # slices K + K + tiles + M + chunks + 1
    assert l.t2v_sn_ws_floats(jobs(SN_MAX_JOBS), SN_MAX_JOBS) == SN_MAX_JOBS * need
    bad = [jobs(w=None), jobs(what=None), jobs(u=None), jobs(v=None), jobs(sigma=None), jobs(M=0), jobs(K=0), jobs(M=-1),
           jobs(M=65536, K=32768)]
    for arr in bad:
        assert l.t2v_sn_ws_floats(arr, 1) == -1
        assert l.t2v_sn_refresh(arr, 1, a, 1 << 40, 1, 1e-12, 0, None) == -1
        assert l.t2v_sn_project(arr, 1, a, 1 << 40, 0, None) == -1
    for fn_args in ((None, 1), (good, 0), (jobs(SN_MAX_JOBS + 1), SN_MAX_JOBS + 1)):
        assert l.t2v_sn_ws_floats(*fn_args) == -1
        assert l.t2v_sn_refresh(fn_args[0], fn_args[1], a, 1 << 40, 1, 1e-12, 0, None) == -1
        assert l.t2v_sn_project(fn_args[0], fn_args[1], a, 1 << 40, 0, None) == -1
    assert l.t2v_sn_refresh(good, 1, None, need, 1, 1e-12, 0, None) == -1
    assert l.t2v_sn_refresh(good, 1, a, need - 1, 1, 1e-12, 0, None) == -1
    assert l.t2v_sn_refresh(good, 1, a, need, 0, 1e-12, 0, None) == -1
    assert l.t2v_sn_refresh(good, 1, a, need, 1, 0.0, 0, None) == -1
    assert l.t2v_sn_project(good, 1, None, need, 0, None) == -1
    assert l.t2v_sn_project(good, 1, a, need - 1, 0, None) == -1
    assert l.t2v_sn_project(jobs(g=None), 1, a, need, 0, None) == -1


# ---- command line, key names, refusals --------------------------------------------------------------------------------------------
NEED = ['--data', 'd.json', '--G', 'g', '--D', 'd']


def test_command_line_flag():
    from txt2vid_amd.train.gan import build_parser
    assert build_parser().parse_args(NEED).D_sn is False
    assert build_parser().parse_args(NEED + ['--D_sn']).D_sn is True
    p = build_parser()
    action = [a for a in p._actions if a.dest == 'D_sn'][0]
    assert action.help.startswith('(new)')


def test_end2end_is_refused_before_anything_else_happens():
    from txt2vid_amd.train.gan import build_parser, main
    with pytest.raises(NotImplementedError, match='--D_sn'):
        main(build_parser().parse_args(NEED + ['--D_sn', '--end2end']))


def test_checkpoint_with_state_needs_the_flag():
    from txt2vid_amd.gan.spectral import check_checkpoint
    assert check_checkpoint({'gen': {}}, False) is None and check_checkpoint({'gen': {}}, True) is None
    state = {'0.x.weight_orig': torch.zeros(1)}
    assert check_checkpoint({'discrim_sn': state}, True, 'f.pt') is state
    with pytest.raises(ValueError, match='--D_sn'):
        check_checkpoint({'discrim_sn': state}, False, 'f.pt')


def _discrim(**kw):
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    return MultiScaleDiscrim(num_channels=1, **kw)


def test_normalised_layers_and_key_names():
    """Every Conv3d and Linear weight of the shared Resnet3D once: 3 stem + 4 x 3 DownBlock + 4 attention projections + the
    head(s). Biases and `gamma` are not in the list."""
    from txt2vid_amd.gan.spectral import normalised_layers, STATE_SUFFIXES
    layers = normalised_layers([_discrim()])
    keys = [k for k, _ in layers]
    assert len(keys) == len(set(keys)) == 3 + 12 + 4 + 1
    assert all(k.startswith('0.single_discrim.') and k.endswith('.weight') for k in keys)
    for must in ('0.single_discrim.res_block.inner_module.0.weight', '0.single_discrim.down.1.theta.weight',
                 '0.single_discrim.down.1.o.weight', '0.single_discrim.fc_uncond.weight'):
        assert must in keys, must
    assert not any('gamma' in k or 'bias' in k for k in keys)
    named = dict(_discrim().named_parameters())
    rest = set(named) - {k[2:] for k in keys}
    assert rest and all(k.endswith('.bias') or k.endswith('.gamma') for k in rest)
    cond = [k for k, _ in normalised_layers([_discrim(cond_dim=8)])]
    assert len(cond) == 21 and '0.single_discrim.fc.weight' in cond
    two = [k for k, _ in normalised_layers([_discrim(), _discrim()])]
    assert len(two) == 40 and two[20].startswith('1.')
    assert STATE_SUFFIXES == ('_orig', '_u', '_v', '_sigma')


def test_construction_refuses_what_the_kernels_cannot_take():
    from txt2vid_amd.gan.spectral import SpectralNorm
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        SpectralNorm([_discrim()])                                    # host tensors, as the other product ops
    with pytest.raises(TypeError, match='fp32'):
        SpectralNorm([_discrim().double()])
    d = _discrim()
    w = d.single_discrim.fc_uncond.weight
    w.data = w.data.t().contiguous().t() if w.shape[0] > 1 else torch.empty(1, 2 * w.shape[1])[:, ::2]
    assert not w.is_contiguous()
    with pytest.raises(ValueError, match='contiguous'):
        SpectralNorm([d])
    for bad in (dict(n_power_iterations=0), dict(n_init=0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            SpectralNorm([_discrim()], **bad)
    with pytest.raises(ValueError):
        SpectralNorm([nn.ReLU()])


def test_off_means_no_hook_and_no_checkpoint_key():
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.optim import Adam, SGD
    dis = _discrim()
    gan = CondGan(gen=MultiScaleGen(width=64, height=64, num_channels=1), discrims=[dis], discrim_names=['video'])
    assert gan.discrim_sn is None and set(gan.save_dict()) == {'gen', 'video'}
    assert Adam(dis.parameters()).weight_hook is None and SGD(dis.parameters()).weight_hook is None
