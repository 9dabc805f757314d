"""Golden launch plans of the convolution host code (txt2vid_amd/csrc/conv.hip): what EVERY host query of the C ABI answers for a
fixed list of launches, recorded with the library of the commit BEFORE a change to that code, from the repository root:

    T2V_LIB=<libt2v_hip.so of the parent commit> python tests/golden/make_golden_plans.py

(`T2V_LIB` selects the library txt2vid_amd._lib loads; without it the tree's own build is recorded.) The queries are host
arithmetic and never touch the device. tests/test_conv_plan_sweep.py regenerates the same records with the library under test
and asserts equality, so a refactor of the launch decisions cannot move a kernel choice, a grid, a split count or a workspace
size unnoticed.

One record per launch: RECORD_LEN int64 values, the return code and the whole `out[]` of every query (buffers are pre-filled
with SENTINEL, so entries a query leaves alone are pinned too):
  t2v_conv_fwd_plan and t2v_conv_fwd_bf16_plan for flags 0 / T2V_CONV_ACCUM / T2V_CONV_MASK_OUT, t2v_conv_fwd_grouped_ws_floats,
  t2v_conv_fwd_grouped_bf16_ok, t2v_conv_wgrad_plan, t2v_conv_wgrad_grouped_slab_floats, ..._bias_slab_floats,
  t2v_pool_conv_plan for what 0 / 1 / 2, t2v_pool_conv_fwd_ws_floats, t2v_pool_conv_dgrad_splits and
  t2v_pool_conv_wgrad_slab_floats for (kD, want_bias) = (3, 0) / (3, 1) / (1, 0).
Every query runs on every launch: most un-pooled members are refused by the pooled queries and the other way round, and the
refusals (T2V_EINVAL) are part of the record.

conv_plans.npz holds `default` [launches, RECORD_LEN] for the full list and, because the tunables are read once per process, one
array per entry of ENV_CASES for the reduced list (the named cases without the channel grid), each made in a process of its own
with that one variable set.
"""
import ctypes as C
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

SENTINEL = -7
RECORD_LEN = 6 * 9 + 2 + 9 + 2 + 3 * 9 + 5
FLAGS = (0, 4, 8)                       # none, T2V_CONV_ACCUM, T2V_CONV_MASK_OUT
GRID_CHANNELS = (1, 3, 4, 6, 16, 32, 40, 48, 64, 70, 128, 256, 512)
GRID_KERNELS = ((1, 1, 1), (1, 3, 3), (3, 3, 3))

# one non-default value of every plan-visible tunable (struct Tunables and the rest of the environment knobs of conv.hip)
ENV_CASES = [
    ('T2V_TILE128_MIN', '1'), ('T2V_TILE256_MIN', '1'), ('T2V_NOSPLIT_CHUNKS', '0'), ('T2V_FORCE_S', '3'), ('T2V_NO_STRIP', '1'),
    ('T2V_STRIP3_DB', '0'), ('T2V_STRIP3_DB', '32'), ('T2V_STRIP3_DB256', '0'), ('T2V_SPLIT_TARGET', '384'),
    ('T2V_WGRAD_SCAP', '64'), ('T2V_WGRAD_TARGET', '512'), ('T2V_WGRAD_NOQ', '1'), ('T2V_WGRAD_MINCPS', '8'),
    ('T2V_NO_WGRAD_THIN', '1'), ('T2V_POOL_FWD_DB', '0'), ('T2V_POOL_DGRAD_DB', '1'), ('T2V_POOL_DGRAD_SPLIT_BELOW', '1'),
    ('T2V_POOL_WGRAD_MINCPS', '8'),
]


def env_key(name, value):
    return 'env_%s_%s' % (name, value)


def _grid_member_sets():
    import conv_cases as cc
    sets = [
        [(1, 1, 1, 1)], [(6, 1, 1, 1)], [(3, 1, 5, 7)], [(2, 1, 6, 6)], [(2, 4, 1, 8)], [(2, 4, 8, 1)], [(2, 3, 6, 10)],
        [(2, 4, 16, 16)], [(12, 8, 16, 16)], [(8, 8, 64, 32)],
        [(4, 2, 16, 16), (2, 4, 8, 8), (1, 1, 5, 3)], [(2, 4, 8, 8), (3, 4, 6, 1), (5, 1, 1, 1)], [(7, 1, 1, 1), (3, 1, 1, 1), (1, 1, 1, 1)],
        [(8, 8, 64, 32), (2, 8, 8, 1), (3, 5, 12, 20)],
        cc.d_step_members(3, 0),
    ]
    return sets + [cc.d_step_members(32, s) for s in range(4)]


def _pool_array(members, stem, what):
    """The member table functional_pool.py hands to the pooled entry points (tests/conv_cases.py::pool_plan)."""
    from txt2vid_amd._lib import ConvGroup
    from txt2vid_amd.functional_pool import pool_tmode
    arr = (ConvGroup * len(members))()
    for a, (n, d, h, w) in zip(arr, members):
        tm = pool_tmode((n, 0, d, h, w), stem)
        a.N, a.D, a.H, a.W, a.dstride = n, d, h, w, tm
        j = 0
        for dz in ((-1, 0, 1) if tm else (0,)):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    a.dz[j], a.dy[j], a.dx[j], a.widx[j] = dz, dy, dx, j
                    j += 1
        a.ntaps = j
        if what == 1:
            for f in range(27):
                a.widx[f] = f
    return arr


def launches(reduced=False):
    """[(name, bytes of the t2v_conv_group array, ngroups, Cin, Cout, (kD, kH, kW))], deterministic."""
    import conv_cases as cc
    from txt2vid_amd._lib import ConvGroup
    out = []
    cache = {}

    def arr_of(members, k):
        key = (tuple(members), k)
        if key not in cache:
            cache[key] = bytes(cc._group_array(list(members), 1, 1, k))       # (the member table does not depend on the channels)
        return cache[key]

    def add(name, arr, n, cin, cout, k):
        out.append((name, arr if isinstance(arr, bytes) else bytes(arr), n, cin, cout, tuple(k)))

    def both(name, members, cin, cout, k):
        add(name + ' fwd', arr_of(members, k), len(members), cin, cout, k)
        add(name + ' dgrad', arr_of(members, k), len(members), cout, cin, k)

    for xs, cout, k in cc.SINGLE_CASES:
        both('single %s->%d' % (xs, cout), [cc.members_of_single(xs)], xs[1], cout, cc.k3(k))
    for name, cin, cout, k, members, _ in cc.GROUPED_CASES:
        both(name, members, cin, cout, cc.k3(k))
    # frame-strided members (tests/test_conv_plan.py::test_frame_strided_members_plan_on_the_host, conv_cases.BF16_CASES)
    k = (3, 3, 3)
    big = cc.d_step_members(32, 0)
    for cin in (64, 1):
        arr = cc._group_array(big, cin, 64, k)
        for a in arr:
            a.dstride = 2
        add('dstride2 Cin=%d' % cin, arr, len(big), cin, 64, k)
    half = [(n, (d + 1) // 2, h, w) for n, d, h, w in big]
    for yoff in (0, 1, 2):
        arr = cc._group_array(half, 64, 64, k)
        for a, (n, d, h, w) in zip(arr, big):
            a.ydstride, a.yoff, a.Dy = 2, yoff, d
        add('ydstride2 yoff=%d' % yoff, arr, len(big), 64, 64, k)
    for name, cin, cout, kk, members, _, even in cc.BF16_CASES:
        both(name, members, cin, cout, cc.k3(kk))
        if even:
            arr = cc._group_array(members, cin, cout, cc.k3(kk))
            for a in arr:
                a.dstride = 2
            add(name + ' even fwd', arr, len(members), cin, cout, cc.k3(kk))
            for i, (darr, n) in enumerate(cc._even_dgrad_arrays(members, cout, cin)):
                add(name + ' even dgrad %d' % i, darr, n, cout, cin, cc.k3(kk))
    # pooled members (test_pooled_convolution_plans), and the ones it expects refused
    for name, cin, cout, members, stem in cc.POOL_CASES:
        add(name + ' fwd/wgrad', _pool_array(members, stem, 0), len(members), cin, cout, k)
        add(name + ' dgrad', _pool_array(members, stem, 1), len(members), cout, cin, k)
    bad = (ConvGroup * 1)()
    bad[0].N, bad[0].D, bad[0].H, bad[0].W, bad[0].dstride, bad[0].ntaps = 2, 3, 8, 8, 1, 27
    add('pool odd frame count', bad, 1, 64, 64, k)
    bad[0].D, bad[0].W = 4, 1
    add('pool one voxel wide', bad, 1, 64, 64, k)
    bad[0].W = 8
    add('pool taps all zero', bad, 1, 64, 64, k)
    add('pool K % 32', bad, 1, 48, 64, k)
    # rejected geometries (test_plan_queries_reject_bad_geometry)
    zero = (ConvGroup * 1)()
    add('all-zero member', zero, 1, 64, 64, k)
    add('no members', zero, 0, 64, 64, k)
    add('too many members', bytes(zero) * 9, 9, 64, 64, k)
    add('Cin = 0', arr_of([(2, 4, 8, 8)], k), 1, 0, 64, k)
    add('kernel extent 2', arr_of([(2, 4, 8, 8)], k), 1, 64, 64, (2, 3, 3))
    if reduced:
        return out
    # the channel grid: un-pooled member sets under three kernels, pooled member sets as the pooled path builds them
    for members in _grid_member_sets():
        for kk in GRID_KERNELS:
            for cin in GRID_CHANNELS:
                for cout in GRID_CHANNELS:
                    add('grid %s k=%s %d->%d' % (members, kk, cin, cout), arr_of(members, kk), len(members), cin, cout, kk)
    for pname, _, _, members, stem in cc.POOL_CASES:
        for what in (0, 1):
            arr = bytes(_pool_array(members, stem, what))
            for cin in GRID_CHANNELS:
                for cout in GRID_CHANNELS:
                    add('grid %s what=%d %d->%d' % (pname, what, cin, cout), arr, len(members), cin, cout, k)
    return out


def record(launch):
    """The RECORD_LEN int64 values of one launch (module docstring)."""
    from txt2vid_amd._lib import lib, ConvGroup
    _, raw, n, cin, cout, (kd, kh, kw) = launch
    arr = (ConvGroup * max(1, len(raw) // C.sizeof(ConvGroup))).from_buffer_copy(raw)
    L = lib()
    rec = []

    def plan(fn, *args):
        out = (C.c_int32 * 8)(*([SENTINEL] * 8))
        rec.append(fn(*args, out))
        rec.extend(out)

    for f in FLAGS:
        plan(L.t2v_conv_fwd_plan, arr, n, cin, cout, f)
    for f in FLAGS:
        plan(L.t2v_conv_fwd_bf16_plan, arr, n, cin, cout, f)
    rec.append(L.t2v_conv_fwd_grouped_ws_floats(arr, n, cin, cout))
    rec.append(L.t2v_conv_fwd_grouped_bf16_ok(arr, n, cin, cout))
    plan(L.t2v_conv_wgrad_plan, arr, n, cin, cout, kd, kh, kw)
    rec.append(L.t2v_conv_wgrad_grouped_slab_floats(arr, n, cin, cout, kd, kh, kw))
    rec.append(L.t2v_conv_wgrad_grouped_bias_slab_floats(arr, n, cin, cout, kd, kh, kw))
    for what in (0, 1, 2):
        out = (C.c_int32 * 8)(*([SENTINEL] * 8))
        rec.append(L.t2v_pool_conv_plan(what, arr, n, cin, cout, out))
        rec.extend(out)
    rec.append(L.t2v_pool_conv_fwd_ws_floats(arr, n, cin, cout))
    rec.append(L.t2v_pool_conv_dgrad_splits(arr, n, cin, cout))
    for kD, want_bias in ((3, 0), (3, 1), (1, 0)):
        rec.append(L.t2v_pool_conv_wgrad_slab_floats(arr, n, cin, cout, kD, want_bias))
    assert len(rec) == RECORD_LEN
    return rec


def records(ls):
    return np.array([record(l) for l in ls], dtype=np.int64).reshape(len(ls), RECORD_LEN)


def records_in_children(ls, env_cases):
    """{env_key: records of `ls`}, each from a fresh process with that one variable set (and no other T2V_ tunable). The children
    run side by side; they get the launches as a file and import neither torch nor the test modules."""
    base = {k: v for k, v in os.environ.items() if not k.startswith('T2V_') or k == 'T2V_LIB'}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        spec = os.path.join(tmp, 'launches.pkl')
        with open(spec, 'wb') as f:
            pickle.dump(ls, f)
        procs = []
        for name, value in env_cases:
            dst = os.path.join(tmp, env_key(name, value) + '.npy')
            env = dict(base)
            env[name] = value
            procs.append((name, value, dst, subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child', spec, dst], env=env,
                                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        for name, value, dst, p in procs:
            log = p.communicate(timeout=300)[0]
            assert p.returncode == 0, '%s=%s: %s' % (name, value, log.decode()[-2000:])
            out[env_key(name, value)] = np.load(dst)
    return out


def main():
    if len(sys.argv) == 4 and sys.argv[1] == '--child':
        with open(sys.argv[2], 'rb') as f:
            np.save(sys.argv[3], records(pickle.load(f)))
        return
    data = {'default': records(launches())}
    data.update(records_in_children(launches(reduced=True), ENV_CASES))
    dst = os.path.join(HERE, 'conv_plans.npz')
    np.savez_compressed(dst, **data)
    print('%s: %d launches, %d environment cases of %d, %d bytes' % (dst, len(data['default']), len(ENV_CASES),
                                                                      len(launches(reduced=True)), os.path.getsize(dst)))


if __name__ == '__main__':
    main()
