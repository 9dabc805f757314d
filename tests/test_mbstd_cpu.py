"""CPU: the discriminator's opt-in minibatch standard deviation head (Resnet3D(mbstd=G) / MultiScaleDiscrim(mbstd=G); DESIGN
"Minibatch standard deviation") — state-dict layout off and on, the zero w that `init()` leaves alone, the refusals, checkpoint
mismatches, the JSON --D specs, the host-side refusals of the entry points, and the float64 restatement the GPU tests compare
against: its own fp32 rounding against the bound, its definition, and its segments."""
import os

import pytest
import torch

import mbstd_cases as MB
from oracle import tganv2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cond(**kw):
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    return MultiScaleDiscrim(num_channels=1, cond_dim=256, **kw)


def _uncond(**kw):
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    return MultiScaleDiscrim(num_channels=1, **kw)


def _shapes(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_mbstd_off_is_todays_module():
    for make, cond_dim in ((_cond, 256), (_uncond, 0)):
        want = O.resnet3d_shapes(MB.prefix(cond_dim > 0), 1, 64, cond_dim)
        m = make()
        trunk = getattr(m.single_discrim, 'module', m.single_discrim)
        assert m.mbstd_on == 0 and not hasattr(trunk, 'mbstd')
        assert _shapes(make(mbstd=0)) == _shapes(m)
        assert [k for k, _ in _shapes(m)] == list(want) and {k: s for k, s in _shapes(m)} == {k: tuple(v) for k, v in want.items()}


def test_mbstd_on_adds_one_trailing_key_per_sub_discriminator():
    on, off = _shapes(_cond(mbstd=4)), _shapes(_cond())
    assert on[:-1] == off and on[-1] == ('single_discrim.module.mbstd.weight', (2,))
    on, off = _shapes(_uncond(mbstd=4)), _shapes(_uncond())
    assert on[:-1] == off and on[-1] == ('single_discrim.mbstd.weight', (1,))
    # with a sentence-code-less text-conditioned class (--dont_use_sent builds cond_dim = 0): works, one weight
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    assert _shapes(MultiScaleDiscrim(num_channels=1, cond_dim=0, mbstd=2))[-1] == ('single_discrim.module.mbstd.weight', (1,))
    # together with proj: after it
    both = _shapes(_cond(proj=True, mbstd=16))
    assert both[:-1] == _shapes(_cond(proj=True)) and both[-1][0].endswith('mbstd.weight') and both[-2][0].endswith('proj.weight')
    multi = [(k, s) for k, s in _shapes(_cond(mbstd=4, single_discrim=False)) if 'mbstd' in k]
    assert multi == [('sub_discrims.%d.module.mbstd.weight' % i, (2,)) for i in range(4)]


@pytest.mark.parametrize('method', ['xavier', 'ortho', 'normal'])
def test_init_leaves_w_zero_and_every_other_draw_unchanged(method):
    from txt2vid_amd.models.resnet3d import Resnet3D
    from txt2vid_amd.util.torch.init import init
    for cond_dim in (6, 0):
        kw = dict(num_channels=1, mid_ch=8, cond_dim=cond_dim, num_down_blocks=2)
        torch.manual_seed(11)
        a = Resnet3D(**kw)
        init(a, method)
        torch.manual_seed(11)
        b = Resnet3D(mbstd=4, **kw)
        init(b, method)
        sa, sb = a.state_dict(), b.state_dict()
        assert tuple(sb['mbstd.weight'].shape) == ((2,) if cond_dim else (1,)) and float(sb['mbstd.weight'].abs().max()) == 0.0
        assert all(torch.equal(sa[k], sb[k]) for k in sa) and set(sb) - set(sa) == {'mbstd.weight'}
        assert not any(tag in type(b.mbstd).__name__ for tag in ('Linear', 'Conv', 'Embedding', 'BatchNorm'))
        assert not isinstance(b.mbstd, (torch.nn.Linear, torch.nn.Conv3d))          # --D_sn walks past it


@pytest.mark.parametrize('G', [1, 17, -1])
def test_group_sizes_outside_2_to_16_are_refused(G):
    from txt2vid_amd.models.resnet3d import Resnet3D
    with pytest.raises(ValueError, match='mbstd'):
        Resnet3D(num_channels=1, mbstd=G)
    with pytest.raises(ValueError, match='mbstd'):
        _cond(mbstd=G)
    with pytest.raises(ValueError, match='mbstd'):
        _uncond(mbstd=G)


def test_every_group_size_from_2_to_16_builds():
    from txt2vid_amd.models.resnet3d import Resnet3D
    for G in range(2, 17):
        assert Resnet3D(num_channels=1, mid_ch=8, num_down_blocks=1, mbstd=G).mbstd.group == G


@pytest.mark.parametrize('make', [_cond, _uncond])
@pytest.mark.parametrize('saved,built', [(4, 0), (0, 4)])
def test_checkpoint_mbstd_mismatch_names_mbstd(make, saved, built):
    sd = make(mbstd=saved).state_dict()
    with pytest.raises(ValueError, match='mbstd=%d' % built):
        make(mbstd=built).load_state_dict(sd)
    trunk = lambda m: getattr(m.single_discrim, 'module', m.single_discrim)
    with pytest.raises(ValueError, match='mbstd=%d' % built):
        trunk(make(mbstd=built)).load_state_dict(trunk(make(mbstd=saved)).state_dict())


def test_trainer_loader_refuses_the_mismatch_too():
    """`CondGan.load_from_dict` matches key styles and keeps the wanted keys only: the check runs in front of it."""
    from txt2vid_amd.gan.cond_gan import CondGan
    for saved, built in ((4, 0), (0, 4)):
        gan = CondGan(gen=torch.nn.Linear(1, 1), discrims=[_cond(mbstd=built)], discrim_names=['video'])
        with pytest.raises(ValueError, match='mbstd=%d' % built):
            gan.load_from_dict({'gen': gan.gen.state_dict(), 'video': _cond(mbstd=saved).state_dict()})


def test_checkpoint_round_trip_with_mbstd():
    a, b = _cond(mbstd=4, proj=True), _cond(mbstd=4, proj=True)
    with torch.no_grad():
        a.single_discrim.module.mbstd.weight.normal_()
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.single_discrim.module.mbstd.weight, b.single_discrim.module.mbstd.weight)


def test_json_specs_build_the_models():
    from txt2vid_amd.util.reflection import create_object
    d = create_object(os.path.join(ROOT, 'tools', 'cfg', 'discrim_mbstd.json'))
    assert type(d).__module__ == 'txt2vid_amd.models.tganv2.discrim'
    assert d.mbstd_on == 4 and tuple(d.single_discrim.mbstd.weight.shape) == (1,) and d.single_discrim.mbstd.group == 4
    assert d.single_discrim.res_block.inner_module[0].weight.shape[1] == 1
    d = create_object(os.path.join(ROOT, 'tools', 'cfg', 'discrim_cond_proj_mbstd.json'), cond_dim=256)
    assert type(d).__module__ == 'txt2vid_amd.models.tganv2_cond.discrim'
    assert d.mbstd_on == 4 and d.proj_on and tuple(d.single_discrim.module.mbstd.weight.shape) == (2,)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-side checks only: null pointers, n outside 1..T2V_MAX_GROUPS, b, K or seg < 1, b % seg != 0, G outside 2..16, H
    outside 1..2."""
    import ctypes as C
    from txt2vid_amd._lib import lib, MbstdMember, MAX_GROUPS
    L = lib()
    p = 16                                                         # never dereferenced: every call below is refused first
    EINVAL = -1                                                    # T2V_EINVAL: a launch status would be -1000 or below

    def members(n=1, b=4, seg=4, **null):
        arr = (MbstdMember * max(n, 1))()
        for a in arr:
            a.f, a.gam, a.stat, a.out, a.b, a.seg = p, p, p, p, b, seg
            for h in range(2):
                a.g[h], a.base[h], a.y[h] = p, p, p
            for k in null:
                if k in ('g', 'base', 'y'):
                    getattr(a, k)[0] = getattr(a, k)[1] = None
                else:
                    setattr(a, k, None)
        return arr
    w = C.c_void_p(p)
    roles = {'fwd': L.t2v_mbstd_fwd, 'feat': L.t2v_mbstd_feat, 'second': L.t2v_mbstd_second,
             'weight': lambda m, n, v, H, K, G, st: L.t2v_mbstd_weight(m, n, v, H, K, G, 0, st)}
    for name, fn in roles.items():
        assert fn(None, 1, w, 2, 8, 4, None) == EINVAL and fn(members(), 1, None, 2, 8, 4, None) == EINVAL, name
        assert fn(members(), 0, w, 2, 8, 4, None) == EINVAL and fn(members(MAX_GROUPS + 1), MAX_GROUPS + 1, w, 2, 8, 4, None) == EINVAL, name
        assert fn(members(), 1, w, 2, 0, 4, None) == EINVAL and fn(members(), 1, w, 2, -1, 4, None) == EINVAL, name
        assert fn(members(b=0, seg=1), 1, w, 2, 8, 4, None) == EINVAL and fn(members(2, b=-4), 2, w, 2, 8, 4, None) == EINVAL, name
        assert fn(members(seg=0), 1, w, 2, 8, 4, None) == EINVAL and fn(members(seg=-2), 1, w, 2, 8, 4, None) == EINVAL, name
        assert fn(members(b=4, seg=3), 1, w, 2, 8, 4, None) == EINVAL and fn(members(b=4, seg=8), 1, w, 2, 8, 4, None) == EINVAL, name
        for G in (1, 0, -1, 17):
            assert fn(members(), 1, w, 2, 8, G, None) == EINVAL, (name, G)
        for H in (0, 3, -1):
            assert fn(members(), 1, w, H, 8, 4, None) == EINVAL, (name, H)
    # the pointers each role uses (a role ignores the others)
    for name, reads in (('fwd', ('f', 'y')), ('feat', ('f', 'g', 'out')), ('second', ('f', 'gam')), ('weight', ('g', 'stat'))):
        for k in reads:
            assert roles[name](members(**{k: None}), 1, w, 2, 8, 4, None) == EINVAL, (name, k)
    assert roles['second'](members(g=None), 1, w, 2, 8, 4, None) == EINVAL              # dL/df needs a_q
    assert roles['second'](members(out=None, stat=None, y=None), 1, w, 2, 8, 4, None) == EINVAL   # nothing to write


def test_restatement_rounding_sits_well_inside_the_bound():
    """fp32 against float64 of the same restatement on every op case: the worst ratio to the bound is printed and must leave a
    factor of 4."""
    worst = {}
    for case in MB.CASES:
        ref, got = MB.case_reference(case), MB.reference(case, dtype=torch.float32)
        for f in MB.FIELDS:
            r = MB.ratio(got[f], ref[f])
            print('mbstd-restatement fp32/fp64 %s %s %.4g (max|ref| %.4g)' % (case, f, r, float(ref[f].abs().max())))
            if r >= worst.get(f, (-1.0,))[0]:
                worst[f] = (r, case)
    for f, w in sorted(worst.items()):
        print('mbstd-restatement fp32/fp64 worst ratio %s %.4g at %s' % (f, w[0], w[1]))
    assert set(worst) == set(MB.FIELDS) and all(w[0] <= 0.25 for w in worst.values()), worst


def test_restatement_matches_its_definition():
    """Against loops written straight from the definition and from the issue's adjoints, first and second order."""
    case = 'odd'
    inp, ref = MB.inputs(case), MB.case_reference(case)
    _, _, K, G, H = MB.CASES[case]
    f, base, r, t, w = (inp[k][0].double() if k != 'w' else inp[k].double() for k in ('f', 'base', 'r', 't', 'w'))
    b = f.shape[0]
    assert MB.groups(b, G) == [(0, 4), (4, 3)]
    y, gf, df, hf = torch.zeros(b, H).double(), torch.zeros(b, K).double(), torch.zeros(b, K).double(), torch.zeros(b, K).double()
    gw, hw = torch.zeros(H).double(), torch.zeros(H).double()
    for r0, n in MB.groups(b, G):
        rows = range(r0, r0 + n)
        mu = [sum(f[i, k] for i in rows) / n for k in range(K)]
        sig = [(sum((f[i, k] - mu[k]) ** 2 for i in rows) / n + 1e-8) ** 0.5 for k in range(K)]
        s = sum(sig) / K
        a1 = sum(r[i, h] * w[h] for i in rows for h in range(H))           # a_q of Σ y·r
        a0 = sum(w[h] for i in rows for h in range(H))                     # a_q of Σ y
        gam = K * t                                                        # Γ = ∂(K Σ df·t)/∂df
        tq = sum(gam[i, k] * (f[i, k] - mu[k]) / (n * K * sig[k]) for i in rows for k in range(K))
        for i in rows:
            for h in range(H):
                y[i, h] = base[i, h] + w[h] * s
                gw[h] += r[i, h] * s
                hw[h] += r[i, h] * s + 1.0 * tq                            # g_hb = 1 in ∂(Σ y)/∂f
            for k in range(K):
                gf[i, k] = a1 * (f[i, k] - mu[k]) / (n * K * sig[k])
                df[i, k] = a0 * (f[i, k] - mu[k]) / (n * K * sig[k])
                gbar = sum(gam[j, k] for j in rows) / n
                p = sum(gam[j, k] * (f[j, k] - mu[k]) for j in rows)
                hf[i, k] = gf[i, k] + (a0 / (n * K)) * ((gam[i, k] - gbar) / sig[k] - (f[i, k] - mu[k]) * p / (n * sig[k] ** 3))
    for name, mine in (('y', y), ('gf', gf), ('gw', gw), ('df', df), ('hf', hf), ('hw', hw)):
        assert torch.allclose(mine, ref[name], rtol=1e-9, atol=1e-12 * float(ref[name].abs().max())), name
    assert torch.equal(ref['gbase'], r)


def test_single_row_groups_have_exact_zero_gradients():
    ref = MB.case_reference('real')                                        # 33 rows, G = 4: row 32 is a group of its own
    assert not ref['gf'][32].any() and not ref['df'][32].any() and not ref['hf'][32].any() and ref['gf'][:32].abs().min() > 0
    one = MB.case_reference('one')
    assert abs(float(one['y'] - MB.inputs('one')['base'][0].double() - MB.inputs('one')['w'].double() * 1e-4)) < 1e-12
    assert not one['gf'].any() and not one['hf'].any() and float(one['gw'].abs()) > 0


def test_segments_restart_the_groups():
    """A real‖fake tensor with seg = b is two separate calls; with seg = 2b a group straddles the boundary and the values differ."""
    inp = MB.inputs('halves')
    G = MB.CASES['halves'][3]
    for f, seg in zip(inp['f'], MB.segs_of('halves')):
        f = f.double()
        b2 = f.shape[0]
        assert b2 == 2 * seg
        apart = torch.cat([MB.stat(f[:seg], G), MB.stat(f[seg:], G)], 0)
        assert torch.equal(MB.stat(f, G, seg), apart)
        whole = MB.stat(f, G, b2)
        assert MB.groups(b2, G, seg) != MB.groups(b2, G, b2) or seg % G == 0
        if seg % G:
            assert float((whole - apart).abs().max()) > 1e-3
    assert MB.groups(6, 2, 3) == [(0, 2), (2, 1), (3, 2), (5, 1)] and MB.groups(6, 2, 6) == [(0, 2), (2, 2), (4, 2)]
    assert MB.groups(4, 2, 2) == [(0, 2), (2, 2)] and MB.groups(33, 4)[-1] == (32, 1) and len(MB.groups(33, 4)) == 9


def test_wrapped_oracle_adds_the_term_and_leaves_the_rest(monkeypatch):
    for cond, proj in ((True, False), (True, True), (False, False)):
        PD, _ = MB.discrim_state(cond, proj)
        pre = MB.prefix(cond)
        g = torch.Generator()
        g.manual_seed(2)
        x = torch.rand(3, 1, 2, 16, 16, generator=g) * 2 - 1
        s = 0.1 * torch.randn(3, 256, generator=g) if cond else None
        with torch.no_grad():
            inner = MB.PJ.resnet3d_proj if proj else O.resnet3d
            u0, c0, f0 = inner(PD, x, s, prefix=pre)
            with monkeypatch.context() as mp:
                MB.patch(mp, 2, proj)
                (u1, c1, f1), = O.multiscale_discrim(PD, [x], [s] if cond else None, pre)
            assert O.resnet3d is MB._plain_resnet3d
        st = MB.stat(f0, 2)
        assert MB.groups(3, 2) == [(0, 2), (2, 1)] and abs(float(st[2]) - 1e-4) < 1e-9 and float(st[0]) == float(st[1]) > 1e-4
        w = PD[pre + 'mbstd.weight']
        assert torch.equal(f0, f1) and torch.equal(u1, u0 + w[0] * st)
        assert (c1 is None and not cond) or torch.equal(c1, c0 + w[1] * st)
