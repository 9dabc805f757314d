"""Device-event timings of the two streaming passes that end an optimiser step, outside the training loop (developer tool).

    [T2V_LIB=<other build>] python tools/tail_stream_micro.py pack   [iters]    # t2v_pack_multi, one job per launch
    [T2V_LIB=<other build>] python tools/tail_stream_micro.py reduce [iters]    # t2v_wgrad_reduce_multi, one destination per launch

One JSON line per case: microseconds per launch (median of `iters` single-launch event pairs after a warm-up), the bytes the
pass has to move (source + destinations, from the shapes) and the rate that gives. `pack` has a T = 27 discriminator weight
in both orientations, a 2-D T = 9 weight and a T = 1 weight of the same byte count (the latter has no strided source
reads: the yardstick for what the strided ones cost); `reduce` has one 512 x 512 x 27 destination at S = 3, 4, 6, 7, 8, 12 so
that the eight-accumulator path (S = 8) can be set against the remainder path (S = 7).
Under `rocprofv3 --pmc ...` the same launches give per-dispatch counters (run with iters = 1)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_lib():
    """txt2vid_amd._lib.lib(), also for a build from before `t2v_pack_job_groups` existed (A/B against the parent commit)."""
    import torch  # noqa: F401  (first: one HIP runtime per process, see _lib.lib)
    from txt2vid_amd import _lib
    probe = C.CDLL(_lib.LIB_PATH)
    if not hasattr(probe, 't2v_pack_job_groups'):
        _lib.SIGNATURES.pop('t2v_pack_job_groups', None)
        import txt2vid_amd.functional as TF
        TF.pack_job_groups = lambda T, ntaps, mode: ntaps
    return _lib.lib()


def timed(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    return us[len(us) // 2], us[0]


def pack(iters):
    import torch
    import pack_reduce_cases as pc
    from txt2vid_amd._lib import PackJob, check
    from txt2vid_amd._ops import _stream
    L = load_lib()
    dev = 'cuda:0'
    cases = [('T27 512x256 mode0', 512, 256, 27, 0), ('T27 512x256 mode1', 512, 256, 27, 1), ('T27 512x512 mode0', 512, 512, 27, 0),
             ('T9 512x768 mode0', 512, 768, 9, 0), ('T9 512x768 mode1', 512, 768, 9, 1), ('T1 512x6912 mode0', 512, 6912, 1, 0),
             ('T27 512x256 mode3 bf16', 512, 256, 27, 3), ('T27 512x256 mode0 centre', 512, 256, 27, 0)]
    for name, Cout, Cin, T, mode in cases:
        taps = [T // 2] if name.endswith('centre') else list(range(T))
        w = torch.randn(Cout, Cin, T, device=dev)
        dst = torch.empty(len(taps) * Cout * Cin, device=dev, dtype=torch.bfloat16 if mode >= 2 else torch.float32)
        tr = (mode & 7) in (0, 3)
        arr, blocks = pc.pack_table(L, PackJob, [(w.data_ptr(), dst.data_ptr(), Cout, Cin, T, taps, mode, Cin if tr else Cout,
                                                  Cout if tr else Cin, 0, 0)])
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(dev)
        med, best = timed(lambda: check(L.t2v_pack_multi(C.c_void_p(tab.data_ptr()), 1, blocks, _stream()), 'pack'), iters)
        nbytes = len(taps) * Cout * Cin * (4 + dst.element_size())
        print(json.dumps({'pass': 'pack', 'case': name, 'blocks': blocks, 'us': round(med, 2), 'us_min': round(best, 2), 'bytes': nbytes,
                          'TBps': round(nbytes / med * 1e-6, 3)}), flush=True)


def reduce(iters):
    import torch
    import pack_reduce_cases as pc
    from txt2vid_amd._lib import WgradDest, WgradSrc, check
    from txt2vid_amd._ops import _stream
    L = load_lib()
    dev = 'cuda:0'
    CoCi, T = 512 * 512, 27
    slab = torch.randn(12 * T * CoCi, device=dev)
    dw = torch.empty(CoCi * T, device=dev)
    for kind in (2, 0):
        for S in (3, 4, 6, 7, 8, 12):
            d = dict(dw=dw.data_ptr(), CoCi=CoCi, T=T, Cout=512, accum=0, kind=kind, tap_major=0,
                     srcs=[dict(slab=slab.data_ptr(), ntaps=T, S=S, map=list(range(T)), tap_stride=CoCi, split_stride=T * CoCi)])
            arr, blocks = pc.reduce_table(WgradDest, WgradSrc, [d])
            tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(dev)
            med, best = timed(lambda: check(L.t2v_wgrad_reduce_multi(C.c_void_p(tab.data_ptr()), 1, blocks, _stream()), 'reduce'), iters)
            nbytes = (S + 1) * T * CoCi * 4
            print(json.dumps({'pass': 'reduce', 'kind': kind, 'S': S, 'blocks': blocks, 'us': round(med, 2), 'us_min': round(best, 2),
                              'bytes': nbytes, 'TBps': round(nbytes / med * 1e-6, 3)}), flush=True)


def flagship_tables(dev='cuda:0', batch=32, iters=3):
    """Run `iters` eager iterations of the benchmarked model and return what its LAST iteration handed to the two multi-tensor
    launches: {'reduce': [(table bytes, ndest, blocks)], 'pack': [...]} in call order (D step first), plus the objects that keep
    the memory those tables point to alive."""
    import torch
    import bench
    import txt2vid_amd.functional as TF
    from txt2vid_amd.gan.trainer import train_iteration
    L = load_lib()
    gen, dis, optD, optG, losses, CondGan = bench.build_models(dev)
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=None, discrim_names=['video'], gp_scale=1.0)
    prm = bench.Params()
    pool = bench.synthetic_batches(batch, 2, 100, dev)
    rec = {'reduce': [], 'pack': []}
    real = {n: getattr(L, n) for n in ('t2v_wgrad_reduce_multi', 't2v_pack_multi')}

    def dev_bytes(ptr, n):
        cands = [t[1] for t in TF._repack_tables.values()]
        for sink in (TF._grad_sink, (gan.__dict__.get('_t2v_grad_sink') or (None, None))[1]):
            if sink is not None and sink.tab_dev is not None:
                cands.append(sink.tab_dev)
        for t in cands:
            off = ptr - t.data_ptr()
            if 0 <= off and off + n <= t.numel():
                return bytes(t[off:off + n].cpu().numpy().tobytes())
        raise RuntimeError('table outside the known device buffers')

    def hook(name, rec_size):
        def f(table, n, blocks, stream):
            ptr = table.value if hasattr(table, 'value') else int(table)
            rec[name].append((dev_bytes(ptr, int(n) * rec_size), int(n), int(blocks)))
            return real['t2v_wgrad_reduce_multi' if name == 'reduce' else 't2v_pack_multi'](table, n, blocks, stream)
        return f
    from txt2vid_amd._lib import PackJob, WgradDest
    for i in range(iters):
        if i == iters - 1:
            L.t2v_wgrad_reduce_multi, L.t2v_pack_multi = hook('reduce', C.sizeof(WgradDest)), hook('pack', C.sizeof(PackJob))
        try:
            train_iteration(gan, pool[i % 2], None, optD, optG, losses, prm, dev)
            torch.cuda.synchronize()
        finally:
            L.t2v_wgrad_reduce_multi, L.t2v_pack_multi = real['t2v_wgrad_reduce_multi'], real['t2v_pack_multi']
    return rec, (gan, optD, optG, pool, L)


def _sub_launch(L, fn, Rec, recs, begin_of):
    """Device table + total workgroups of a sub-table (records copied, block_begin renumbered)."""
    import torch
    arr = (Rec * len(recs))()
    blocks = 0
    for a, r in zip(arr, recs):
        C.memmove(C.byref(a), C.byref(r), C.sizeof(Rec))
        a.block_begin = blocks
        blocks += begin_of(r)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to('cuda:0'), len(recs), blocks


def flagship(iters):
    """Bytes and time of the real tables, whole and by subset (kind x split count of the reduce; kernel extent x source layout of
    the pack). Replays run on whatever the buffers hold after the iteration: only the time is read."""
    import pack_reduce_cases as pc
    from txt2vid_amd._lib import PackJob, WgradDest, check
    from txt2vid_amd._ops import _stream
    tabs, keep = flagship_tables()
    L = keep[-1]

    def dest_bytes(d):
        rd = sum(sum(1 for t in range(d.T) if d.src[k].map[t] >= 0) * d.src[k].S for k in range(d.nsrc)) * d.CoCi * 4
        return rd + d.T * d.CoCi * 4 * (2 if d.accum else 1)

    def job_bytes(j):
        return j.ntaps * j.Cout * j.Cin * (4 + (2 if (j.mode & 7) >= 2 else 4))

    def bucket_d(d):
        smax = max(d.src[k].S for k in range(d.nsrc))
        return 'kind%d S%s nsrc%d' % (d.kind, '<8' if smax < 8 else ('8-15' if smax < 16 else '>=16'), d.nsrc)

    def bucket_j(j):
        return 'T%d %s ntaps%s' % (j.T, 'tap-major' if j.mode & 8 else 'dense', 'all' if j.ntaps == j.T else '<T')
    for name, Rec, fn, nbytes, bucket, nblk in (
            ('reduce', WgradDest, L.t2v_wgrad_reduce_multi, dest_bytes, bucket_d, lambda d: d.nblocks),
            ('pack', PackJob, L.t2v_pack_multi, job_bytes, bucket_j, lambda j: j.bx * j.by * pc.pack_groups(L, j.T, j.ntaps, j.mode))):
        for li, (raw, n, blocks) in enumerate(tabs[name]):
            recs = list((Rec * n).from_buffer_copy(raw))
            groups = {'all': recs}
            for r in recs:
                groups.setdefault(bucket(r), []).append(r)
            for g, rs in groups.items():
                tab, cnt, blk = _sub_launch(L, fn, Rec, rs, nblk)
                med, best = timed(lambda: check(fn(C.c_void_p(tab.data_ptr()), cnt, blk, _stream()), name), iters)
                b = sum(nbytes(r) for r in rs)
                print(json.dumps({'pass': name, 'launch': li, 'subset': g, 'records': cnt, 'blocks': blk, 'bytes': b, 'us': round(med, 2),
                                  'us_min': round(best, 2), 'TBps': round(b / med * 1e-6, 3)}), flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'pack'
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    {'pack': pack, 'reduce': reduce, 'flagship': flagship}[what](n)
