"""GPU: the weight repack (`t2v_pack_multi`, `t2v_pack_weight[_into]`, `t2v_pack_weight_bf16`, `functional.repack_params`) against
a host permutation of the source, and the batched weight-gradient reduce (`t2v_wgrad_reduce_multi`) bit for bit against the
float32 restatement of its documented summation order (tests/pack_reduce_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_reduce_cases as pc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -777.0


def _env():
    from txt2vid_amd import functional as TF
    from txt2vid_amd._lib import PackJob, WgradDest, WgradSrc
    return TF, TF.lib(), PackJob, WgradDest, WgradSrc


def _upload(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pack_cases(mode):
    """[(name, w (device), Cout, Cin, T, taps)] over every T, shape and tap list; mode | 8 sources are stored [T][Cout][Cin]."""
    g = torch.Generator()
    g.manual_seed(17 + mode)
    out = []
    for T in pc.PACK_T:
        for Cout, Cin in pc.PACK_SHAPES:
            shape = (T, Cout, Cin) if mode & 8 else (Cout, Cin, T)
            w = torch.randn(shape, generator=g).to(DEV)
            for name, taps in pc.tap_lists(T).items():
                out.append(('T%d %dx%d %s' % (T, Cout, Cin, name), w, Cout, Cin, T, taps))
    return out


def _dst_for(mode, ntaps, Cout, Cin, wide):
    """(sentinel-filled destination [ntaps][rows][cols], rows, cols, row_off, col_off): exact, or wider than the weight with offsets."""
    tr = (mode & 7) in (0, 3)
    r, c = (Cin, Cout) if tr else (Cout, Cin)
    ro, co = (3, 5) if wide else (0, 0)
    rows, cols = r + (ro + 2 if wide else 0), c + (co + 4 if wide else 0)
    dt = torch.bfloat16 if (mode & 7) >= 2 else torch.float32
    return torch.full((ntaps, rows, cols), SENTINEL, dtype=dt, device=DEV), rows, cols, ro, co


@pytest.mark.parametrize('mode', pc.PACK_MODES)
def test_pack_multi_one_table_per_mode(mode):
    """Every (T, shape, tap list) as one job of ONE table, each into a destination wider than the weight at non-zero offsets that is
    pre-filled with a sentinel: the job's rectangle holds the permuted source, everything else is untouched. Run twice."""
    TF, L, PackJob, _, _ = _env()
    cases = _pack_cases(mode)
    jobs, dsts = [], []
    for i, (name, w, Cout, Cin, T, taps) in enumerate(cases):
        dst, rows, cols, ro, co = _dst_for(mode, len(taps), Cout, Cin, wide=i % 2 == 0)
        dsts.append((dst, ro, co))
        jobs.append((w.data_ptr(), dst.data_ptr(), Cout, Cin, T, taps, mode, rows, cols, ro, co))
    assert len({j[4] for j in jobs}) >= 3
    arr, blocks = pc.pack_table(L, PackJob, jobs)
    tab = _upload(arr)
    for _ in range(2):
        TF.check(L.t2v_pack_multi(C.c_void_p(tab.data_ptr()), len(jobs), blocks, TF._stream()), 't2v_pack_multi')
    torch.cuda.synchronize()
    for (name, w, Cout, Cin, T, taps), (dst, ro, co) in zip(cases, dsts):
        want = pc.pack_expect(w, T, taps, mode, torch.full_like(dst, SENTINEL), ro, co)
        assert torch.equal(_bits(dst), _bits(want)), (mode, name)


@pytest.mark.parametrize('mode', pc.PACK_MODES)
def test_pack_single_tensor_entry_points(mode):
    """The same cases through t2v_pack_weight_into (wide destination, offsets), t2v_pack_weight (exact) and t2v_pack_weight_bf16."""
    TF, L, _, _, _ = _env()
    for name, w, Cout, Cin, T, taps in _pack_cases(mode):
        tc = (C.c_int32 * len(taps))(*taps)
        if (mode & 7) >= 2:
            dst, *_ = _dst_for(mode, len(taps), Cout, Cin, wide=False)
            TF.check(L.t2v_pack_weight_bf16(TF._p(w), TF._p(dst), Cout, Cin, T, tc, len(taps), (mode & 7) - 2, TF._stream()), 'bf16')
            want = pc.pack_expect(w, T, taps, mode, torch.full_like(dst, SENTINEL))
            assert torch.equal(_bits(dst), _bits(want)), (mode, name, 'bf16')
            continue
        dst, rows, cols, ro, co = _dst_for(mode, len(taps), Cout, Cin, wide=True)
        TF.check(L.t2v_pack_weight_into(TF._p(w), TF._p(dst), Cout, Cin, T, tc, len(taps), mode, rows, cols, ro, co, TF._stream()), 'into')
        want = pc.pack_expect(w, T, taps, mode, torch.full_like(dst, SENTINEL), ro, co)
        assert torch.equal(_bits(dst), _bits(want)), (mode, name, 'into')
        dst, *_ = _dst_for(mode, len(taps), Cout, Cin, wide=False)
        TF.check(L.t2v_pack_weight(TF._p(w), TF._p(dst), Cout, Cin, T, tc, len(taps), mode, TF._stream()), 'pack')
        want = pc.pack_expect(w, T, taps, mode, torch.full_like(dst, SENTINEL))
        assert torch.equal(_bits(dst), _bits(want)), (mode, name, 'exact')


def test_repack_params_three_kernel_extents_in_one_table():
    """`repack_params` on parameters with T = 27, 9 and 1 (one table, one launch): every cached variant (forward, mirrored, bf16, the
    9 live taps of a D == 1 member) equals the host permutation of the NEW values; a second call leaves the same bits."""
    TF = _env()[0]
    torch.manual_seed(5)
    shapes = [(33, 70, 3, 3, 3), (40, 48, 1, 3, 3), (64, 32, 1, 1, 1)]
    params = [torch.nn.Parameter(torch.randn(s).to(DEV)) for s in shapes]
    packed = []
    for w in params:
        cout, cin, kd, kh, kw = w.shape
        geoms = [TF.conv_geom(2, cin, 4, 6, 6, cout, kd, kh, kw)]
        if kd == 3:
            geoms.append(TF.conv_geom(2, cin, 1, 6, 6, cout, kd, kh, kw))
        for g in geoms:
            ts = TF._tapset(g.T, g.mask)
            for mode in (0, 1):
                packed.append((w, TF.packed_weight(w, g, mode), g.T, list(g.taps), mode))
                packed.append((w, TF.packed_weight_bf16(w, ts, mode), ts.T, list(ts.taps), 2 + mode))
    with torch.no_grad():
        for w in params:
            w.copy_(torch.randn(w.shape).to(DEV))
    for _ in range(2):
        TF.repack_params(params)
        torch.cuda.synchronize()
        for w, wp, T, taps, mode in packed:
            cout, cin = w.shape[0], w.shape[1]
            tr = (mode & 7) in (0, 3)
            want = pc.pack_expect(w.detach().reshape(cout, cin, T), T, taps, mode,
                                  torch.empty((len(taps), cin if tr else cout, cout if tr else cin), dtype=wp.dtype, device=DEV))
            assert torch.equal(_bits(wp.reshape(want.shape)), _bits(want)), (tuple(w.shape), mode, len(taps))
    assert len({p[2] for p in packed}) == 3


def test_fused_gate_packs_persist_across_repack(monkeypatch):
    """The ConvLSTM's fused gate matrices (`packed_fused`: four [8,8,3,3] parameters seen as [8,8,1,3,3] views, two stored tap-major
    and two dense; modes 0 / 1; the 9 taps and the single live tap of a 1x1 map) next to the plain fp32 / bf16 packs of one of the
    same parameters. After an in-place update + `bump_weight_epoch` + `repack_params` every buffer sits at the same address and
    equals, bit for bit, a fresh pack through the single-tensor entry points; a second lookup, through new `unsqueeze(2)` views,
    returns the same buffers without calling a pack entry point."""
    TF, L = _env()[:2]
    from txt2vid_amd import _lib
    Cc, n = 8, 4
    torch.manual_seed(11)
    params = [torch.nn.Parameter(TF.tap_major(torch.randn(Cc, Cc, 3, 3).to(DEV)) if i < 2 else torch.randn(Cc, Cc, 3, 3).to(DEV))
              for i in range(n)]
    assert [TF.is_tap_major(p) for p in params] == [True, True, False, False]
    tapsets = []
    for hw in (4, 1):
        g = TF.conv_geom(2, Cc, 1, hw, hw, n * Cc, 1, 3, 3)
        tapsets.append(TF._tapset(g.T, g.mask))
    assert [len(ts.taps) for ts in tapsets] == [9, 1]
    dense = params[2]

    def lookups():
        """[(buffer, fresh pack into a scratch buffer)] of every variant, through views made for this call."""
        out = []
        for ts in tapsets:
            for mode in (0, 1):
                def fresh_fused(dst, ts=ts, mode=mode):
                    rows, cols = (Cc, n * Cc) if mode == 0 else (n * Cc, Cc)
                    for i, p in enumerate(params):
                        ro, co = (0, i * Cc) if mode == 0 else (i * Cc, 0)
                        TF.check(L.t2v_pack_weight_into(TF._p(p), TF._p(dst), Cc, Cc, ts.T, ts.taps_c, len(ts.taps), mode | (8 if i < 2 else 0),
                                                        rows, cols, ro, co, TF._stream()), 'into')
                out.append((TF.packed_fused([p.unsqueeze(2) for p in params], ts, mode), fresh_fused))
        ts = tapsets[0]
        for mode in (0, 1):
            out.append((TF.packed_weight(dense.unsqueeze(2), ts, mode), lambda dst, mode=mode: TF.check(L.t2v_pack_weight(
                TF._p(dense), TF._p(dst), Cc, Cc, ts.T, ts.taps_c, len(ts.taps), mode, TF._stream()), 'pack')))
            out.append((TF.packed_weight_bf16(dense.unsqueeze(2), ts, mode), lambda dst, mode=mode: TF.check(L.t2v_pack_weight_bf16(
                TF._p(dense), TF._p(dst), Cc, Cc, ts.T, ts.taps_c, len(ts.taps), mode, TF._stream()), 'pack16')))
        return out
    first = lookups()
    assert len({wp.data_ptr() for wp, _ in first}) == len(first) == 8
    ptrs = [wp.data_ptr() for wp, _ in first]
    with torch.no_grad():
        for p in params:
            p.copy_(torch.randn(Cc, Cc, 3, 3).to(DEV))           # (keeps each parameter's memory layout)
    assert [TF.is_tap_major(p) for p in params] == [True, True, False, False]
    TF.bump_weight_epoch(params)
    TF.repack_params(params)
    torch.cuda.synchronize()
    for (wp, fresh), ptr in zip(first, ptrs):
        assert wp.data_ptr() == ptr
        ref = torch.full_like(wp, SENTINEL)
        fresh(ref)
        torch.cuda.synchronize()
        assert torch.equal(_bits(wp), _bits(ref)), (tuple(wp.shape), wp.dtype)
    calls = []

    def wrap(name, orig):
        def f(*a):
            calls.append(name)
            return orig(*a)
        return f
    with monkeypatch.context() as mp:
        for name in _lib.SIGNATURES:
            mp.setattr(L, name, wrap(name, getattr(L, name)))
        again = lookups()
    torch.cuda.synchronize()
    assert not {'t2v_pack_weight', 't2v_pack_weight_into', 't2v_pack_weight_bf16'} & set(calls), calls
    assert [wp.data_ptr() for wp, _ in again] == ptrs


# ---------------------------------------------------------------------------------------------- reduce
def _reduce_dests(kind, values):
    """Destinations of one table for `kind`: T x CoCi x S, with 1-3 sources whose maps have -1 entries, a tap no source touches,
    accumulate on / off for weight and bias, tap-major and dense, bias slabs with one source lacking them."""
    g = torch.Generator()
    g.manual_seed(100 * kind + (1 if values == 'int' else 2))

    def rnd(*shape):
        if values == 'int':
            return torch.randint(-8, 9, shape, generator=g).float()
        return torch.randn(*shape, generator=g)
    S_list = pc.REDUCE_S
    dests = []
    for T in pc.REDUCE_T:
        for CoCi in pc.REDUCE_COCI:
            if kind >= 2 and CoCi % 4:
                continue
            for idx, S in enumerate(S_list):
                nsrc, accum, tap_major = 1 + idx % 3, idx % 2, (idx // 2) % 2
                Cout = 4
                srcs = []
                for k in range(nsrc):
                    # source k skips the taps with (t + k) % 3 == 0; NO source touches the last tap (T > 1)
                    live = [t for t in range(T) if T == 1 or ((t + k) % 3 != 0 and t != T - 1)]
                    m = [-1] * T
                    for slot, t in enumerate(live):
                        m[t] = slot
                    Sk = S_list[(idx + k) % len(S_list)]
                    has_bias = idx % 3 != 1 and not (nsrc > 1 and k == 1)
                    srcs.append({'S': Sk, 'map': m, 'ntaps': max(len(live), 1), 'slab_h': rnd(Sk, max(len(live), 1), CoCi),
                                 'bias_h': rnd(Sk, Cout) if has_bias else None})
                dests.append({'T': T, 'CoCi': CoCi, 'Cout': Cout, 'accum': accum, 'accum_bias': (idx + 1) % 2, 'tap_major': tap_major,
                              'kind': kind, 'srcs': srcs, 'dw0_h': rnd(T, CoCi) if tap_major else rnd(CoCi, T),
                              'db0_h': rnd(Cout) if idx % 3 != 1 else None})
    return dests


@pytest.mark.parametrize('values', ('int', 'randn'))
@pytest.mark.parametrize('kind', (0, 1, 2, 3))
def test_wgrad_reduce_multi_bit_for_bit(kind, values):
    TF, L, _, WgradDest, WgradSrc = _env()
    dests = _reduce_dests(kind, values)
    assert {d['srcs'][0]['S'] for d in dests} == set(pc.REDUCE_S) and {len(d['srcs']) for d in dests} == {1, 2, 3}
    rows = []
    for d in dests:
        d['dw_d'] = d['dw0_h'].to(DEV)
        d['db_d'] = d['db0_h'].to(DEV) if d['db0_h'] is not None else None
        for s in d['srcs']:
            s['slab_d'] = s['slab_h'].to(DEV)
            s['bias_d'] = s['bias_h'].to(DEV) if s['bias_h'] is not None else None
        rows.append(dict(dw=d['dw_d'].data_ptr(), dbias=d['db_d'].data_ptr() if d['db_d'] is not None else None, CoCi=d['CoCi'], T=d['T'],
                         Cout=d['Cout'], accum=d['accum'], accum_bias=d['accum_bias'], kind=kind, tap_major=d['tap_major'],
                         srcs=[dict(slab=s['slab_d'].data_ptr(), bias_slab=s['bias_d'].data_ptr() if s['bias_d'] is not None else None,
                                    ntaps=s['ntaps'], S=s['S'], map=s['map'], tap_stride=d['CoCi'], split_stride=s['ntaps'] * d['CoCi'])
                               for s in d['srcs']]))
    arr, blocks = pc.reduce_table(WgradDest, WgradSrc, rows)
    assert C.sizeof(WgradDest) == L.t2v_wgrad_dest_bytes()
    tab = _upload(arr)
    TF.check(L.t2v_wgrad_reduce_multi(C.c_void_p(tab.data_ptr()), len(rows), blocks, TF._stream()), 't2v_wgrad_reduce_multi')
    torch.cuda.synchronize()
    for n, d in enumerate(dests):
        srcs = [{'slab': s['slab_h'].numpy(), 'map': s['map'], 'bias': s['bias_h'].numpy() if s['bias_h'] is not None else None}
                for s in d['srcs']]
        dw, db = pc.reduce_expect(kind, d['T'], d['CoCi'], d['Cout'], srcs, d['dw0_h'].numpy(), d['accum'], d['tap_major'],
                                  d['db0_h'].numpy() if d['db0_h'] is not None else None, d['accum_bias'])
        tag = (kind, values, n, d['T'], d['CoCi'], [s['S'] for s in d['srcs']], d['accum'], d['tap_major'])
        assert np.array_equal(d['dw_d'].cpu().numpy().view(np.int32), dw.view(np.int32)), tag
        if db is not None:
            assert np.array_equal(d['db_d'].cpu().numpy().view(np.int32), db.view(np.int32)), tag + ('bias',)


@pytest.mark.parametrize('case', ('many_splits', 'few_splits'))
def test_single_destination_reduce_agrees_with_multi(case):
    """`t2v_conv_wgrad_grouped` (weight-gradient kernel + its own single-destination reduce) against the same launch's partial
    sums reduced by `t2v_wgrad_reduce_multi` with one source, scalar and 16-byte kinds: the same bits. The two cases select
    wgrad_reduce_small_kernel (kinds 1 / 3) and wgrad_reduce_kernel (kinds 0 / 2)."""
    import conv_cases as cc
    TF, L, _, WgradDest, WgradSrc = _env()
    members, cin, cout, k, want = {'many_splits': ([(2, 4, 16, 16)], 16, 16, (3, 3, 3), 'reduce_small'),
                                   'few_splits': ([(2, 2, 8, 8)], 64, 128, (3, 3, 3), 'reduce')}[case]
    assert cc.wgrad_plan(members, cin, cout, k)[4] == want
    g = torch.Generator()
    g.manual_seed(9)
    xs = [torch.randn(n, cin, d, h, w, generator=g).to(DEV) for n, d, h, w in members]
    gys = [torch.randn(n, cout, d, h, w, generator=g).to(DEV) for n, d, h, w in members]
    wshape = (cout, cin) + k
    T, CoCi = k[0] * k[1] * k[2], cout * cin
    dw_full = TF.conv_group_wgrad_raw(xs, gys, wshape)
    src, slab = TF._wgrad_partial_launch(xs, gys, wshape, False, False)
    assert (src.S >= 16) == (want == 'reduce_small')
    torch.cuda.synchronize()
    for kind in ((1, 3) if want == 'reduce_small' else (0, 2)):
        dw = torch.full((CoCi * T,), float('nan'), device=DEV)
        arr = (WgradDest * 1)()
        a = arr[0]
        a.dw, a.dbias, a.CoCi, a.T, a.Cout, a.nsrc, a.accum, a.accum_bias, a.kind, a.tap_major = dw.data_ptr(), None, CoCi, T, cout, 1, 0, 0, kind, 0
        a.block_begin, a.nblocks = 0, pc.reduce_nblocks(kind, CoCi, T)
        C.memmove(C.byref(a.src[0]), C.byref(src), C.sizeof(WgradSrc))
        tab = _upload(arr)
        TF.check(L.t2v_wgrad_reduce_multi(C.c_void_p(tab.data_ptr()), 1, a.nblocks, TF._stream()), 't2v_wgrad_reduce_multi')
        torch.cuda.synchronize()
        assert torch.equal(_bits(dw), _bits(dw_full.reshape(-1))), (case, kind)
