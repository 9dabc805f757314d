"""CPU: the generator's opt-in conditional BatchNorm (MultiScaleGen(cond_bn=True); DESIGN "Conditional BatchNorm") — state-dict
layout off and on, the zero projection that `init()` leaves alone, the site table, the refusals, checkpoint mismatches, the JSON
--G spec, and the float64 restatement the GPU tests compare against (its own fp32 rounding against the bounds)."""
import os

import pytest
import torch

import cbn_cases as CB
from oracle import tganv2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = [1024, 512, 512, 256, 256, 128, 128, 64, 64, 32, 32, 32, 128, 64, 32, 32]


def _cond_gen(**kw):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    return MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, **kw)


def _shapes(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_cond_bn_off_is_todays_module():
    want = O.gen_shapes(num_channels=1, cond_dim=256, cond_variant=True)
    m = _cond_gen()
    assert not m.cond_bn_on and not hasattr(m, 'cond_bn') and m.cond_bn_table() == []
    assert _shapes(_cond_gen(cond_bn=False)) == _shapes(m)
    assert [k for k, _ in _shapes(m)] == [k for k, _ in _shapes(_cond_gen(cond_bn=True))][:-2]
    params = {k: tuple(v.shape) for k, v in m.state_dict().items() if 'running_' not in k and 'num_batches' not in k}
    assert params == {k: tuple(v) for k, v in want.items() if 'running_' not in k and 'num_batches' not in k}


@pytest.mark.parametrize('ca_dim,d', [(0, 256), (128, 128)])
def test_cond_bn_on_adds_one_projection(ca_dim, d):
    on = _shapes(_cond_gen(cond_bn=True, ca_dim=ca_dim))
    off = _shapes(_cond_gen(ca_dim=ca_dim))
    assert on[:-2] == off                                          # the former keys, in the former order
    assert on[-2:] == [('cond_bn.weight', (2 * 3296, d)), ('cond_bn.bias', (2 * 3296,))]
    assert sum(CHANNELS) == 3296


def test_site_table():
    m = _cond_gen(cond_bn=True)
    tab = m.cond_bn_table()
    assert [k for k, _, _ in tab] == list(range(16))
    assert [c for _, c, _ in tab] == CHANNELS
    assert [o for _, _, o in tab] == [2 * sum(CHANNELS[:k]) for k in range(16)]
    assert [m_.num_features for m_ in m.cond_bn_sites()] == CHANNELS
    # the restatement derives the same table from the recipe state
    assert CB.site_table(CB.gen_state()) == tab
    names = dict((id(mod), name) for name, mod in m.named_modules())
    assert [names[id(s)] + '.' for s in m.cond_bn_sites()] == CB.site_prefixes()
    # other widths: two sites per later UpBlock, one per RenderBlock
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    m2 = MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=16, additional_blocks=[48, 24], cond_bn=True)
    assert [c for _, c, _ in m2.cond_bn_table()] == [1024, 512, 512, 256, 256, 128, 128, 48, 48, 24, 128, 48, 24]


@pytest.mark.parametrize('method', ['xavier', 'ortho', 'normal'])
def test_init_leaves_the_projection_zero_and_every_other_draw_unchanged(method):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.util.torch.init import init
    kw = dict(width=64, height=64, num_channels=1, cond_dim=8, fm_channels=1024)
    torch.manual_seed(11)
    a = MultiScaleGen(**kw)
    init(a, method)
    torch.manual_seed(11)
    b = MultiScaleGen(cond_bn=True, **kw)
    init(b, method)
    sa, sb = a.state_dict(), b.state_dict()
    assert float(sb['cond_bn.weight'].abs().max()) == 0.0 and float(sb['cond_bn.bias'].abs().max()) == 0.0
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and set(sb) - set(sa) == {'cond_bn.weight', 'cond_bn.bias'}
    assert not any(tag in type(b.cond_bn).__name__ for tag in ('Linear', 'Conv', 'Embedding', 'BatchNorm'))


def test_cond_bn_on_the_unconditional_generator_is_refused():
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    with pytest.raises(ValueError, match='text-conditioned'):
        MultiScaleGen(width=64, height=64, num_channels=1, cond_bn=True)


def test_cond_bn_without_sentence_code_is_refused():
    """--dont_use_sent: the command line builds the generator with cond_dim = 0."""
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    with pytest.raises(ValueError, match='dont_use_sent'):
        MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=0, cond_bn=True)
    with pytest.raises(ValueError, match='sentence code'):
        _cond_gen(cond_bn=True)(torch.zeros(2, 256))


@pytest.mark.parametrize('saved,built', [(True, False), (False, True)])
def test_checkpoint_cond_bn_mismatch_names_cond_bn(saved, built):
    sd = _cond_gen(cond_bn=saved).state_dict()
    with pytest.raises(ValueError, match='cond_bn=%s' % built):
        _cond_gen(cond_bn=built).load_state_dict(sd)


def test_checkpoint_round_trip_with_cond_bn():
    a, b = _cond_gen(cond_bn=True), _cond_gen(cond_bn=True)
    with torch.no_grad():
        a.cond_bn.weight.normal_()
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.cond_bn.weight, b.cond_bn.weight)


def test_json_spec_parses():
    from txt2vid_amd.util.reflection import create_object
    g = create_object(os.path.join(ROOT, 'tools', 'cfg', 'gen_cond_cbn.json'), cond_dim=256)
    assert type(g).__module__ == 'txt2vid_amd.models.tganv2_cond.gen'
    assert g.cond_bn_on and g.ca_dim == 0 and tuple(g.cond_bn.weight.shape) == (6592, 256)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-side checks only: null pointers, empty extents, N % T, the last base row, the column range."""
    import ctypes as C
    from txt2vid_amd._lib import lib
    p = C.c_void_p(16)                                             # never dereferenced: every call below is refused first
    EINVAL = -1                                                    # T2V_EINVAL: a launch status would be -1000 or below

    def fwd(N=6, Cc=6, H=5, W=5, ld=12, off=0, s=1, T=2, R=3, tab=p, x=p):
        return lib().t2v_cbn_train_fwd(x, p, p, tab, p, p, p, p, p, N, Cc, H, W, ld, off, s, T, R, 0.1, 1e-5, 0, None, None)

    def bwd(N=6, Cc=6, H=5, W=5, ld=12, off=0, s=1, T=2, R=3, gtab=p):
        return lib().t2v_cbn_train_bwd_add(p, p, p, p, p, p, None, p, p, p, gtab, p, N, Cc, H, W, ld, off, s, T, R, 0, 0, None)

    def ev(N=6, Cc=6, H=5, W=5, ld=12, off=0, s=1, T=2, R=3, tab=p):
        return lib().t2v_cbn_eval(p, p, p, p, p, tab, p, N, Cc, H, W, ld, off, s, T, R, 1e-5, 0, None)
    for f in (fwd, bwd, ev):
        assert f(T=4) == EINVAL                                          # N % T != 0
        assert f(R=2) == EINVAL                                          # (N/T - 1) * s + 1 > R
        assert f(s=2, R=4) == EINVAL
        assert f(ld=11) == EINVAL and f(off=1) == EINVAL and f(off=-1) == EINVAL     # the site's columns leave the leading dimension
        assert f(N=0) == EINVAL and f(Cc=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL and f(T=0) == EINVAL and f(s=0) == EINVAL
    assert fwd(tab=None) == EINVAL and fwd(x=None) == EINVAL and bwd(gtab=None) == EINVAL and ev(tab=None) == EINVAL
    assert lib().t2v_cbn_train_fwd_up(None, p, p, p, p, p, p, p, p, 6, 6, 5, 5, 12, 0, 1, 2, 3, 0.1, 1e-5, 0, None, None) == EINVAL
    assert lib().t2v_cbn_train_bwd(p, p, p, p, p, p, p, p, p, p, p, 6, 6, 5, 5, 12, 0, 1, 4, 3, 0, None) == EINVAL
    assert lib().t2v_cbn_train_bwd_up(p, p, None, p, p, p, p, p, p, p, p, 6, 6, 5, 5, 12, 0, 1, 2, 3, 1, None) == EINVAL     # relu needs y
    assert lib().t2v_cbn_ws_floats(0, 6, 25) == EINVAL
    # the workspace holds the statistics slices (forward) and the per-row sums (backward)
    assert lib().t2v_cbn_ws_floats(6, 6, 25) == max(lib().t2v_bn_ws_floats(6, 6, 25) - 2 * 6, 2 * 6 * 6)


def test_restatement_rounding_sits_well_inside_the_bounds():
    """fp32 against float64 of the same restatement on every op case: the worst ratio to the bound is printed and must leave a
    factor of 4 (the bounds come from tests/norm_cases.py; `one_pixel` only runs the `plain` recipe, as there)."""
    worst = {}
    for case, recipe in CB.CASE_RECIPES:
        for relu in (False, True):
            for up in (False, True):
                for fork in ('off', 'both'):
                    for wide in (False, True):
                        ref = CB.case_reference(case, recipe, relu, up, fork, wide)
                        got = CB.reference(case, recipe, relu, up, fork, wide, dtype=torch.float32)
                        for f in ('y', 'dx', 'dgamma', 'dbeta', 'dtab', 'rm', 'rv'):
                            r = CB.NC.ratio(got[f], ref[f], CB.TOL[f])
                            if r > worst.get(f, (0.0,))[0]:
                                worst[f] = (r, case, recipe, relu, up, fork, wide)
    for f, w in sorted(worst.items()):
        print('cbn-restatement fp32/fp64 worst ratio %s %.4g at %s' % (f, w[0], w[1:]))
    assert all(w[0] <= 0.25 for w in worst.values()), worst


def test_restatement_matches_its_definition():
    """Against a loop over samples written straight from the definition, and: the statistics ignore the table; rows the level
    does not hold get exactly zero gradient; a zero table is the plain BatchNorm."""
    import torch.nn.functional as F
    inp = CB.inputs('strided', 'plain', True)
    (N, Cc, H, W), T, s, R = CB.CASES['strided']
    ld, off = CB.geometry('strided', True)
    ref = CB.case_reference('strided', 'plain', False, False, 'off', True)
    x, tab = inp['x'].double(), inp['tab'].double()
    mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    y = torch.empty_like(x)
    for n in range(N):
        row = tab[(n // T) * s]
        for c in range(Cc):
            xh = (x[n, c] - mean[c]) / torch.sqrt(var[c] + CB.EPS)
            y[n, c] = xh * (inp['gamma'][c].double() + row[off + c]) + (inp['beta'][c].double() + row[off + Cc + c])
    assert torch.allclose(y, ref['y'], rtol=1e-12, atol=1e-12)
    assert float(ref['dtab'][1].abs().max()) == 0.0 and float(ref['dtab'][3].abs().max()) == 0.0
    assert float(ref['dtab'][:, :off].abs().max()) == 0.0 and float(ref['dtab'][:, off + 2 * Cc:].abs().max()) == 0.0
    assert float(ref['dtab'][0, off:off + 2 * Cc].abs().min()) > 0.0
    plain = F.batch_norm(x, inp['rm'].double().clone(), inp['rv'].double().clone(), inp['gamma'].double(), inp['beta'].double(),
                         True, CB.MOMENTUM, CB.EPS)
    zero = CB.reference('strided', 'plain', False, False, 'off', True, tab=torch.zeros(R, ld))
    assert torch.allclose(zero['y'], plain, rtol=1e-12, atol=1e-12)
    assert torch.equal(zero['rm'], ref['rm']) and torch.equal(zero['rv'], ref['rv'])
