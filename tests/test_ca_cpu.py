"""CPU: the generator's opt-in conditioning augmentation (MultiScaleGen(ca_dim=D); DESIGN "Conditioning augmentation") — module
surface and state-dict layout, the refusals, checkpoint mismatches, the JSON --G spec, and the StaticDraws layout / draw order."""
import os

import numpy as np
import pytest
import torch

import ca_cases as CA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cond_gen(**kw):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    return MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, **kw)


def _shapes(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_ca_off_is_todays_module():
    from oracle import tganv2_oracle as O
    want = O.gen_shapes(num_channels=1, cond_dim=256, cond_variant=True)
    m = _cond_gen()
    assert m.ca_dim == 0 and not hasattr(m, 'ca')
    assert _shapes(_cond_gen(ca_dim=0)) == _shapes(m)
    params = {k: tuple(v.shape) for k, v in m.state_dict().items() if 'running_' not in k and 'num_batches' not in k}
    assert params == {k: tuple(v) for k, v in want.items() if 'running_' not in k and 'num_batches' not in k}


def test_ca_on_adds_its_fc_and_widens_the_generator_fc():
    m = _cond_gen(ca_dim=128, ca_kl_coeff=0.5)
    off = dict(_shapes(_cond_gen()))
    on = dict(_shapes(m))
    assert on.pop('ca.fc.weight') == (512, 256) and on.pop('ca.fc.bias') == (512,)
    assert on.pop('fc.weight') == (1024, 256 + 128) and off.pop('fc.weight') == (1024, 256 + 256)
    assert on == off
    assert m.ca_kl_coeff == 0.5 and _cond_gen(ca_dim=64).ca_kl_coeff == 2.0
    # init() draws the CA fc like every other Linear: xavier weight, zero bias
    from txt2vid_amd.util.torch.init import init
    torch.manual_seed(0)
    init(m, 'xavier')
    assert float(m.ca.fc.bias.detach().abs().max()) == 0.0 and 0.02 < float(m.ca.fc.weight.detach().std()) < 0.08


def test_ca_on_the_unconditional_generator_is_refused():
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    with pytest.raises(ValueError, match='text-conditioned'):
        MultiScaleGen(width=64, height=64, num_channels=1, ca_dim=128)


def test_ca_without_sentence_code_is_refused():
    """--dont_use_sent: the command line builds the generator with cond_dim = 0."""
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    with pytest.raises(ValueError, match='dont_use_sent'):
        MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=0, ca_dim=128)
    with pytest.raises(ValueError):
        _cond_gen(ca_dim=-1)


@pytest.mark.parametrize('saved,built', [(128, 0), (0, 128), (64, 128)])
def test_checkpoint_ca_mismatch_names_ca_dim(saved, built):
    sd = _cond_gen(ca_dim=saved).state_dict()
    m = _cond_gen(ca_dim=built)
    with pytest.raises(ValueError, match='ca_dim=%d' % built):
        m.load_state_dict(sd)


def test_checkpoint_round_trip_with_ca():
    a, b = _cond_gen(ca_dim=128), _cond_gen(ca_dim=128)
    with torch.no_grad():
        a.ca.fc.weight.normal_()
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.ca.fc.weight, b.ca.fc.weight)


def test_reference_checkpoint_loads_into_ca_off_generator():
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint_cond.pt'), map_location='cpu', weights_only=False)
    sd = ck['gen']
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    m = MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=sd['fc.weight'].shape[1] - 256)
    m.load_state_dict(sd)
    with pytest.raises(ValueError, match='ca_dim'):
        MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=sd['fc.weight'].shape[1] - 256, ca_dim=32).load_state_dict(sd)


def test_json_spec_parses():
    from txt2vid_amd.util.reflection import create_object
    g = create_object(os.path.join(ROOT, 'tools', 'cfg', 'gen_cond_ca.json'), cond_dim=256)
    assert type(g).__module__ == 'txt2vid_amd.models.tganv2_cond.gen'
    assert g.ca_dim == 128 and g.ca_kl_coeff == 2.0 and tuple(g.fc.weight.shape) == (1024, 384)


def test_trainer_reads_the_ca_settings():
    from txt2vid_amd.gan.trainer import TrainStep

    class G(object):
        ca_dim, ca_kl_coeff = 16, 0.75

    class Gan(object):
        gen = G()
    prm = CA.S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    ts = TrainStep(Gan(), None, None, None, prm, 'cpu')
    assert ts.ca and ts.kl_coeff == 0.75 and ts._kl_args() == {'kl': None, 'kl_coeff': 0.75}
    Gan.gen = object()
    ts = TrainStep(Gan(), None, None, None, prm, 'cpu')
    assert not ts.ca and ts._kl_args() == {}


@pytest.mark.parametrize('N,M', [(1, 1), (2, 2)])
def test_static_draws_with_ca_follow_the_documented_order(N, M):
    from txt2vid_amd.draws import StaticDraws
    Bt, L, D, nl, ng, perms = 5, 7, 3, 4, 3, N + 1
    sd = StaticDraws('cpu', Bt, L, nl, n_gen_phases=ng, gp=True, subsample_input=True, n_perms=perms, n_d_steps=N, n_g_steps=M,
                     ca_dim=D)
    base = StaticDraws('cpu', Bt, L, nl, n_gen_phases=ng, gp=True, subsample_input=True, n_perms=perms, n_d_steps=N, n_g_steps=M)
    assert sd.d_all.numel() == base.d_all.numel() + Bt * D * M
    torch.manual_seed(3)
    np.random.seed(3)
    sd.begin_step()
    torch.manual_seed(3)
    np.random.seed(3)
    want = CA.host_draw_sequence(Bt, L, D, nl, ng, N, M, perms)
    assert [int(t) for _, t in sd.multiscale_t0(nl)] == want['t0s']
    assert torch.equal(sd.z(Bt, L, 'cpu'), want['z'])
    # the consumers in the order one iteration calls them: G forward 0 (eps, phases), D steps (perm, alphas), real_pred's perm,
    # later G forwards (eps, phases)
    assert torch.equal(sd.ca_eps(Bt, D, 'cpu'), want['eps'][0])
    got_phases = [int(sd.phase()[1]) for _ in range(ng)]
    got_alphas = [sd.alpha(b, 5, 'cpu') for _ in range(N) for b in want['bs']]
    for j in range(1, M):
        assert torch.equal(sd.ca_eps(Bt, D, 'cpu'), want['eps'][j])
        got_phases += [int(sd.phase()[1]) for _ in range(ng)]
    assert got_phases == want['phases']
    assert all(torch.equal(a, b) for a, b in zip(got_alphas, want['alphas']))
    for p in want['perms']:
        assert np.array_equal(sd.perm(Bt, 'cpu').numpy(), p)
    with pytest.raises(AssertionError):
        sd.ca_eps(Bt, D, 'cpu')                        # M eps per iteration, no more
    sd.rewind()
    assert torch.equal(sd.ca_eps(Bt, D, 'cpu'), want['eps'][0])


@pytest.mark.parametrize('N,M', [(1, 1), (2, 2)])
def test_static_draws_without_ca_keep_todays_layout(N, M):
    """ca_dim = 0: the same buffer, byte for byte, as a StaticDraws built without the argument, and the same draws."""
    from txt2vid_amd.draws import StaticDraws
    kw = dict(n_gen_phases=3, gp=True, subsample_input=True, n_perms=N + 1, n_d_steps=N, n_g_steps=M)
    a, b = StaticDraws('cpu', 5, 7, 4, ca_dim=0, **kw), StaticDraws('cpu', 5, 7, 4, **kw)
    for sd in (a, b):
        torch.manual_seed(8)
        np.random.seed(8)
        sd.begin_step()
    assert a.d_all.numel() == 4 + 3 * M + 5 * 7 + (5 + 3 + 2 + 1) * N + (N + 1) * 5
    assert torch.equal(a.d_all, b.d_all) and a.d_eps is None


def test_host_draws_ca_eps():
    from txt2vid_amd.draws import HostDraws
    torch.manual_seed(4)
    e = HostDraws().ca_eps(3, 5, 'cpu')
    torch.manual_seed(4)
    assert torch.equal(e, torch.randn(3, 5))


def test_ca_ref_matches_its_definition():
    """The CPU restatement the GPU tests compare against: GLU split, reparameterisation, and the closed-form KL of N(mu, e^lv)."""
    torch.manual_seed(1)
    h, eps = torch.randn(3, 16, dtype=torch.float64), torch.randn(3, 4, dtype=torch.float64)
    c, kl = CA.ca_ref(h, eps)
    x = torch.nn.functional.glu(h, dim=1)
    mu, lv = x[:, :4], x[:, 4:]
    assert torch.allclose(c, mu + eps * lv.mul(0.5).exp())
    q = torch.distributions.Normal(mu, lv.mul(0.5).exp())
    p = torch.distributions.Normal(torch.zeros_like(mu), torch.ones_like(mu))
    assert torch.allclose(kl, torch.distributions.kl_divergence(q, p).mean())
