"""Bit-for-bit A/B of the weight repack and the batched weight-gradient reduce between two builds of the kernel library.

    python tools/tail_bits.py --ab LIB_A LIB_B [--json FILE]     # one child process per library, LIB_A twice (A against A), then A against B
    T2V_LIB=LIB python tools/tail_bits.py --out DIR              # what a child does: run everything, write DIR/<name>.npy

A child runs (1) every case of tests/test_pack_reduce_gpu.py — the pack tables of all six modes through t2v_pack_multi, the reduce
tables of kinds 0-3 on integer-valued and random slabs through t2v_wgrad_reduce_multi — and (2) one eager iteration (one D step,
one G step) of the benchmarked model at batch 32 on seeded weights and data, after which it writes every packed weight buffer
the step's two `repack_params` launches refreshed and both gradient arenas (what its two reduce launches summed). The parent
wants `np.array_equal` on every array; exit status 1 otherwise. A build from before `t2v_pack_job_groups` is given the
one-workgroup-per-tap count it expects (tools/tail_stream_micro.py: load_lib)."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def child(out_dir):
    import torch
    from tail_stream_micro import load_lib
    L = load_lib()
    import pack_reduce_cases as pc
    import test_pack_reduce_gpu as tp
    import txt2vid_amd.functional as TF
    from txt2vid_amd import _lib
    from txt2vid_amd._lib import PackJob, WgradDest, WgradSrc
    os.makedirs(out_dir, exist_ok=True)
    names = []

    def save(name, t):
        torch.cuda.synchronize()
        t = t.detach()
        a = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()
        np.save(os.path.join(out_dir, name + '.npy'), a)
        names.append(name)
    # ---- (1) the test cases
    for mode in pc.PACK_MODES:
        cases = tp._pack_cases(mode)
        jobs, dsts = [], []
        for i, (name, w, Cout, Cin, T, taps) in enumerate(cases):
            dst, rows, cols, ro, co = tp._dst_for(mode, len(taps), Cout, Cin, wide=i % 2 == 0)
            dsts.append(dst)
            jobs.append((w.data_ptr(), dst.data_ptr(), Cout, Cin, T, taps, mode, rows, cols, ro, co))
        arr, blocks = pc.pack_table(L, PackJob, jobs)
        tab = tp._upload(arr)
        TF.check(L.t2v_pack_multi(C.c_void_p(tab.data_ptr()), len(jobs), blocks, TF._stream()), 't2v_pack_multi')
        for i, dst in enumerate(dsts):
            save('pack-m%d-%03d' % (mode, i), dst)
    for kind in range(4):
        for values in ('int', 'randn'):
            dests = tp._reduce_dests(kind, values)
            rows, keep = [], []
            for d in dests:
                dw = d['dw0_h'].to(tp.DEV)
                db = d['db0_h'].to(tp.DEV) if d['db0_h'] is not None else None
                srcs = []
                for s in d['srcs']:
                    sl = s['slab_h'].to(tp.DEV)
                    bs = s['bias_h'].to(tp.DEV) if s['bias_h'] is not None else None
                    keep += [sl, bs]
                    srcs.append(dict(slab=sl.data_ptr(), bias_slab=bs.data_ptr() if bs is not None else None, ntaps=s['ntaps'], S=s['S'],
                                     map=s['map'], tap_stride=d['CoCi'], split_stride=s['ntaps'] * d['CoCi']))
                keep.append((dw, db))
                rows.append(dict(dw=dw.data_ptr(), dbias=db.data_ptr() if db is not None else None, CoCi=d['CoCi'], T=d['T'], Cout=d['Cout'],
                                 accum=d['accum'], accum_bias=d['accum_bias'], kind=kind, tap_major=d['tap_major'], srcs=srcs))
            arr, blocks = pc.reduce_table(WgradDest, WgradSrc, rows)
            tab = tp._upload(arr)
            TF.check(L.t2v_wgrad_reduce_multi(C.c_void_p(tab.data_ptr()), len(rows), blocks, TF._stream()), 't2v_wgrad_reduce_multi')
            for i, kd in enumerate(k for k in keep if isinstance(k, tuple)):
                save('reduce-k%d-%s-%03d-dw' % (kind, values, i), kd[0])
                if kd[1] is not None:
                    save('reduce-k%d-%s-%03d-db' % (kind, values, i), kd[1])
    # ---- (2) the benchmarked model's real tables: one D step + one G step
    import bench
    from txt2vid_amd.gan.trainer import train_iteration
    gen, dis, optD, optG, losses, CondGan = bench.build_models(tp.DEV)
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=None, discrim_names=['video'], gp_scale=1.0)
    pool = bench.synthetic_batches(32, 1, 100, tp.DEV)
    calls = {'t2v_pack_multi': 0, 't2v_wgrad_reduce_multi': 0}
    real = {n: getattr(L, n) for n in calls}

    def counted(n):
        def f(*a):
            calls[n] += 1
            return real[n](*a)
        return f
    for n in calls:
        setattr(L, n, counted(n))
    try:
        train_iteration(gan, pool[0], None, optD, optG, losses, bench.Params(), tp.DEV)
    finally:
        for n in calls:
            setattr(L, n, real[n])
    assert calls['t2v_pack_multi'] >= 2 and calls['t2v_wgrad_reduce_multi'] >= 2, calls
    seen = set()
    for tag, model in (('G', gen), ('D', dis)):
        for pname, p in model.named_parameters():
            for key, rec in (TF._pack_cache.get(id(p)) or {}).items():
                if rec.ref() is p and rec.buf.data_ptr() not in seen:
                    seen.add(rec.buf.data_ptr())
                    save('flagship-%s-%s-pack%02d' % (tag, pname, len([n for n in names if n.startswith('flagship-%s-%s-' % (tag, pname))])), rec.buf)
    sink = gan.__dict__['_t2v_grad_sink'][1]
    for i, arena in enumerate({id(s[0]): s[0] for s in sink.slots.values()}.values()):
        save('flagship-grad-arena%d' % i, arena.flat)
    json.dump({'lib': _lib.LIB_PATH, 'arrays': names, 'launches': calls}, open(os.path.join(out_dir, 'index.json'), 'w'))
    print('tail_bits: %d arrays from %s (%s)' % (len(names), _lib.LIB_PATH, calls))


def compare(dir_a, dir_b):
    ia, ib = (json.load(open(os.path.join(d, 'index.json'))) for d in (dir_a, dir_b))
    res = {'lib_a': ia['lib'], 'lib_b': ib['lib'], 'arrays': len(ia['arrays']), 'differing': [], 'same_set_of_arrays': ia['arrays'] == ib['arrays']}
    for name in ia['arrays']:
        f = os.path.join(dir_b, name + '.npy')
        if not os.path.exists(f) or not np.array_equal(np.load(os.path.join(dir_a, name + '.npy')), np.load(f)):
            res['differing'].append(name)
    res['bit_identical'] = res['same_set_of_arrays'] and not res['differing']
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', metavar='DIR')
    ap.add_argument('--ab', nargs=2, metavar='LIB')
    ap.add_argument('--json', metavar='FILE')
    args = ap.parse_args()
    if args.out:
        child(args.out)
        return 0
    if not args.ab:
        ap.error('one of --out, --ab')
    tmp = tempfile.mkdtemp(prefix='tail_bits_')
    try:
        dirs = [os.path.join(tmp, n) for n in ('a', 'a2', 'b')]
        for lib_path, d in zip((args.ab[0], args.ab[0], args.ab[1]), dirs):
            env = dict(os.environ, T2V_LIB=os.path.abspath(lib_path))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--out', d], env=env, cwd=ROOT)
        res = {'a_against_a': compare(dirs[0], dirs[1]), 'a_against_b': compare(dirs[0], dirs[2])}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res['bit_identical'] = res['a_against_a']['bit_identical'] and res['a_against_b']['bit_identical']
    print(json.dumps({k: (v if not isinstance(v, dict) else {x: y for x, y in v.items() if x != 'differing' or y}) for k, v in res.items()}))
    if args.json:
        json.dump(res, open(args.json, 'w'), indent=1)
    return 0 if res['bit_identical'] else 1


if __name__ == '__main__':
    sys.exit(main())
