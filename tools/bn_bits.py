"""Bit-for-bit A/B of the fused BatchNorm training entry points between two builds of the kernel library.

    python tools/bn_bits.py --ab LIB_A LIB_B [--json FILE]     # one child process per library, one after the other, then compare
    T2V_LIB=LIB python tools/bn_bits.py --out DIR                  # what a child does: run everything, write DIR/<name>.npy
    python tools/bn_bits.py --compare DIR_A DIR_B [--json FILE]

A child runs t2v_bn_train_fwd[_up], t2v_bn_train_bwd[_up], t2v_bn_train_bwd_add (with and without its second gradient) and the
conditional twins t2v_cbn_train_fwd[_up] / t2v_cbn_train_bwd[_up] / t2v_cbn_train_bwd_add through the C ABI, ReLU on and off,
on (1) the shapes of tests/norm_pass_cases.py and (2) the BatchNorm shapes of one flagship generator forward (unconditional
TGANv2, B = 32, recorded from the library calls of one train-mode forward), on seeded inputs, and writes every output: y,
(mean | 1/std), the running statistics, dx, dgamma, dbeta, dtab. `--compare` wants `np.array_equal` on every array (NaNs
would differ: there are none) and the same set of files; exit status 1 otherwise. `--ab` keeps the arrays in a temporary
directory and removes it."""
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

MOMENTUM, EPS = 0.1, 1e-5


def flagship_shapes(dev, batch=32):
    """[(N, C, H, W)] of the training-mode BatchNorm launches of one flagship generator forward, in first-seen order."""
    import torch
    import bench
    from txt2vid_amd._lib import lib
    L = lib()
    seen = []
    real = {n: getattr(L, n) for n in ('t2v_bn_train_fwd', 't2v_bn_train_fwd_up')}

    def flat(*a):
        seen.append((a[8], a[9], 1, int(a[10])))            # [N,C,S]: the plane as one row
        return real['t2v_bn_train_fwd'](*a)

    def up(*a):
        seen.append((a[8], a[9], a[10], a[11]))
        return real['t2v_bn_train_fwd_up'](*a)
    L.t2v_bn_train_fwd, L.t2v_bn_train_fwd_up = flat, up
    try:
        gen = bench.build_models(dev)[0]
        with torch.no_grad():
            gen(torch.randn(batch, gen.latent_size).to(dev))
        torch.cuda.synchronize()
    finally:
        L.t2v_bn_train_fwd, L.t2v_bn_train_fwd_up = real['t2v_bn_train_fwd'], real['t2v_bn_train_fwd_up']
    out = []
    for s in seen:
        if s not in out:
            out.append(s)
    assert out, 'the flagship generator ran no training-mode BatchNorm'
    return out


def run_shape(tag, N, Cc, H, W, seed, dev, out_dir, names):
    import torch
    from txt2vid_amd._lib import lib
    from txt2vid_amd._ops import _stream
    L, st = lib(), _stream()
    S = H * W
    g = torch.Generator()
    g.manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, generator=g).to(dev)
    x = randn(N, Cc, H, W)
    x += 3.0                                                       # a mean well off zero: M2 must be taken about the slice mean
    gamma, beta, rm0, rv0 = 1 + 0.1 * randn(Cc), 0.1 * randn(Cc), 0.1 * randn(Cc), 1 + 0.1 * randn(Cc).abs()
    gys = {0: randn(N, Cc, H, W), 1: randn(N, Cc, 2 * H, 2 * W)}
    w2 = randn(N, Cc, H, W)
    # the conditional twin: rows of T frames, base rows s apart, the site's 2C columns at `off` of a wider table
    T = max(t for t in (4, 3, 2, 1) if N % t == 0)
    s, off = 2, 3
    R, ld = (N // T - 1) * s + 1, 2 * Cc + off + 2
    tab = 0.1 * randn(R, ld)

    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def new(*shape):
        return torch.full(shape, float('nan'), device=dev, dtype=torch.float32)

    def save(name, t):
        torch.cuda.synchronize()
        a = t.detach().cpu().numpy()
        assert not np.isnan(a).any(), name                         # every element was written
        np.save(os.path.join(out_dir, name + '.npy'), a)
        names.append(name)

    def ok(status, what):
        if status != 0:
            raise RuntimeError('%s %s: status %d' % (tag, what, status))
    ws_n, cws_n = int(L.t2v_bn_ws_floats(N, Cc, S)), int(L.t2v_cbn_ws_floats(N, Cc, S))
    for relu in (0, 1):
        for up in (0, 1):
            v = '%s-r%du%d' % (tag, relu, up)
            m = 2 if up else 1
            gy = gys[up]
            # ---- the plain site
            y, stats, rm, rv = new(N, Cc, m * H, m * W), new(2 * Cc), rm0.clone(), rv0.clone()
            cnt = torch.tensor([5], dtype=torch.int64, device=dev)
            if up:
                ok(L.t2v_bn_train_fwd_up(p(x), p(gamma), p(beta), p(y), p(stats), p(rm), p(rv), p(new(ws_n)), N, Cc, H, W, MOMENTUM, EPS,
                                         relu, p(cnt), st), 'fwd_up')
            else:
                ok(L.t2v_bn_train_fwd(p(x), p(gamma), p(beta), p(y), p(stats), p(rm), p(rv), p(new(ws_n)), N, Cc, S, MOMENTUM, EPS, relu,
                                      p(cnt), st), 'fwd')
            for n_, t_ in (('y', y), ('stats', stats), ('rm', rm), ('rv', rv)):
                save('%s-%s' % (v, n_), t_)
            assert int(cnt) == 6
            gx, dg, db = new(N, Cc, H, W), new(Cc), new(Cc)
            if up:
                ok(L.t2v_bn_train_bwd_up(p(gy), p(x), p(y), p(stats), p(gamma), p(gx), p(dg), p(db), p(new(ws_n)), N, Cc, H, W, relu, st), 'bwd_up')
            else:
                ok(L.t2v_bn_train_bwd(p(gy), p(x), p(y), p(stats), p(gamma), p(gx), p(dg), p(db), p(new(ws_n)), N, Cc, S, relu, st), 'bwd')
            for n_, t_ in (('dx', gx), ('dgamma', dg), ('dbeta', db)):
                save('%s-%s' % (v, n_), t_)
            for add, a_ in ((w2, 'add'), (None, 'add0')):
                gx, dg, db = new(N, Cc, H, W), new(Cc), new(Cc)
                ok(L.t2v_bn_train_bwd_add(p(gy), p(x), p(y), p(stats), p(gamma), p(add), p(gx), p(dg), p(db), p(new(ws_n)), N, Cc, H, W, up,
                                          relu, st), 'bwd_add')
                for n_, t_ in (('dx', gx), ('dgamma', dg), ('dbeta', db)):
                    save('%s-%s-%s' % (v, a_, n_), t_)
            # ---- the conditional site
            y, stats, rm, rv = new(N, Cc, m * H, m * W), new(2 * Cc), rm0.clone(), rv0.clone()
            fwd = L.t2v_cbn_train_fwd_up if up else L.t2v_cbn_train_fwd
            ok(fwd(p(x), p(gamma), p(beta), p(tab), p(y), p(stats), p(rm), p(rv), p(new(cws_n)), N, Cc, H, W, ld, off, s, T, R, MOMENTUM, EPS,
                   relu, None, st), 'cbn_fwd')
            for n_, t_ in (('y', y), ('stats', stats), ('rm', rm), ('rv', rv)):
                save('%s-cbn-%s' % (v, n_), t_)
            for add, a_ in ((None, 'bwd'), (w2, 'add')):
                gx, dg, db, gtab = new(N, Cc, H, W), new(Cc), new(Cc), torch.zeros(R, ld, device=dev)
                if add is None:
                    bwd = L.t2v_cbn_train_bwd_up if up else L.t2v_cbn_train_bwd
                    ok(bwd(p(gy), p(x), p(y), p(stats), p(gamma), p(tab), p(gx), p(dg), p(db), p(gtab), p(new(cws_n)), N, Cc, H, W, ld, off, s,
                           T, R, relu, st), 'cbn_bwd')
                else:
                    ok(L.t2v_cbn_train_bwd_add(p(gy), p(x), p(y), p(stats), p(gamma), p(tab), p(add), p(gx), p(dg), p(db), p(gtab),
                                               p(new(cws_n)), N, Cc, H, W, ld, off, s, T, R, up, relu, st), 'cbn_bwd_add')
                for n_, t_ in (('dx', gx), ('dgamma', dg), ('dbeta', db), ('dtab', gtab)):
                    save('%s-cbn-%s-%s' % (v, a_, n_), t_)


def child(out_dir, flagship):
    import torch
    import norm_pass_cases as pc
    from txt2vid_amd import _lib
    dev = 'cuda:0'
    os.makedirs(out_dir, exist_ok=True)
    names = []
    shapes = [(name, ) + tuple(pc.shape(name)) for name in pc.CASES]
    if flagship:
        shapes += [('flagship%d' % i, ) + s for i, s in enumerate(flagship_shapes(dev))]
    for i, (tag, N, Cc, H, W) in enumerate(shapes):
        run_shape(tag, N, Cc, H, W, 4242 + i, dev, out_dir, names)
        torch.cuda.empty_cache()
    json.dump({'lib': _lib.LIB_PATH, 'shapes': [list(s) for s in shapes], 'arrays': names}, open(os.path.join(out_dir, 'index.json'), 'w'))
    print('bn_bits: %d arrays of %d shapes from %s' % (len(names), len(shapes), _lib.LIB_PATH))


def compare(dir_a, dir_b):
    ia, ib = (json.load(open(os.path.join(d, 'index.json'))) for d in (dir_a, dir_b))
    res = {'lib_a': ia['lib'], 'lib_b': ib['lib'], 'shapes': ia['shapes'], 'arrays': len(ia['arrays']), 'differing': [],
           'same_set_of_arrays': ia['arrays'] == ib['arrays'] and ia['shapes'] == ib['shapes']}
    for name in ia['arrays']:
        f = os.path.join(dir_b, name + '.npy')
        a = np.load(os.path.join(dir_a, name + '.npy'))
        if not os.path.exists(f) or not np.array_equal(a, np.load(f)):
            res['differing'].append(name)
    res['bit_identical'] = res['same_set_of_arrays'] and not res['differing']
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', metavar='DIR')
    ap.add_argument('--compare', nargs=2, metavar='DIR')
    ap.add_argument('--ab', nargs=2, metavar='LIB')
    ap.add_argument('--json', metavar='FILE')
    ap.add_argument('--no-flagship', action='store_true', help='only the shapes of tests/norm_pass_cases.py')
    args = ap.parse_args()
    if args.out:
        child(args.out, not args.no_flagship)
        return 0
    tmp = None
    if args.ab:
        tmp = tempfile.mkdtemp(prefix='bn_bits_')
        dirs = [os.path.join(tmp, 'a'), os.path.join(tmp, 'b')]
        for lib_path, d in zip(args.ab, dirs):
            env = dict(os.environ, T2V_LIB=os.path.abspath(lib_path))
            cmd = [sys.executable, os.path.abspath(__file__), '--out', d] + (['--no-flagship'] if args.no_flagship else [])
            subprocess.check_call(cmd, env=env, cwd=ROOT)
    elif args.compare:
        dirs = args.compare
    else:
        ap.error('one of --out, --compare, --ab')
    try:
        res = compare(*dirs)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({k: v for k, v in res.items() if k != 'shapes'}))
    if args.json:
        json.dump(res, open(args.json, 'w'), indent=1)
    return 0 if res['bit_identical'] else 1


if __name__ == '__main__':
    sys.exit(main())
