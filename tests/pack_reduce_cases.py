"""Cases, table builders and host restatements for the weight repack (`t2v_pack_multi`, `t2v_pack_weight[_into]`,
`t2v_pack_weight_bf16`) and the batched weight-gradient reduce (`t2v_wgrad_reduce_multi` and its single-destination twins).

The restatements are the documented contracts of include/t2v_hip.h written out on the host:
  * a pack is a permutation / index of the source (compared with torch.equal; bf16 against `.to(torch.bfloat16)`);
  * a reduce is a float32 sum in a FIXED order (compared bit for bit, numpy float32 arithmetic in that order)."""
import ctypes as C

import numpy as np

PACK_T = (1, 3, 9, 27)
PACK_SHAPES = ((5, 3), (33, 70), (64, 32), (40, 48))          # (Cout, Cin): ragged both ways, one exact multiple of the 32 x 32 tile
PACK_MODES = (0, 1, 0 | 8, 1 | 8, 2, 3)


def tap_lists(T):
    """{name: [original tap indices]}: the full list, the centre, the dz = 0 plane of 27, a list that straddles the boundary
    between two groups of 9 source positions, and a list given out of order."""
    out = {'full': list(range(T)), 'centre': [T // 2]}
    if T == 27:
        out['dz0'] = list(range(9, 18))
        out['straddle'] = [7, 8, 9, 10, 17, 18]
        out['unordered'] = [26, 0, 13, 9, 8, 18, 4]
    elif T == 9:
        out['unordered'] = [8, 0, 4, 3]
    elif T == 3:
        out['unordered'] = [2, 0]
    return out


# ---------------------------------------------------------------------------------------------- repack
def pack_expect(w, T, taps, mode, dst, row_off=0, col_off=0):
    """What a pack job leaves in `dst` [ntaps][dst_rows][dst_cols] (a torch tensor, modified in place and returned).
    `w`: [Cout][Cin][T], or [T][Cout][Cin] for mode | 8."""
    jm = mode & 7
    mirror, transpose = jm in (1, 3), jm in (0, 3)
    for j, t in enumerate(taps):
        ts = T - 1 - t if mirror else t
        plane = w[ts] if mode & 8 else w[:, :, ts]                # [Cout][Cin]
        blk = plane.t() if transpose else plane
        dst[j, row_off:row_off + blk.shape[0], col_off:col_off + blk.shape[1]] = blk.to(dst.dtype)
    return dst


def pack_groups(lib, T, ntaps, mode):
    """Third factor of a job's workgroup count (bx * by * this). A build from before the library stated it owns one per listed tap."""
    if hasattr(lib, 't2v_pack_job_groups'):
        fn = lib.t2v_pack_job_groups
        fn.argtypes, fn.restype = [C.c_int, C.c_int, C.c_int], C.c_int
        return int(fn(T, ntaps, mode))
    return ntaps


def pack_table(lib, PackJob, jobs):
    """(ctypes array, total workgroups) for jobs = [(src_ptr, dst_ptr, Cout, Cin, T, taps, mode, rows, cols, row_off, col_off)]."""
    arr = (PackJob * len(jobs))()
    blocks = 0
    for a, (src, dst, Cout, Cin, T, taps, mode, rows, cols, ro, co) in zip(arr, jobs):
        a.src, a.dst = src, dst
        a.Cout, a.Cin, a.T, a.ntaps, a.mode = Cout, Cin, T, len(taps), mode
        a.dst_rows, a.dst_cols, a.row_off, a.col_off = rows, cols, ro, co
        a.bx, a.by = (Cin + 31) // 32, (Cout + 31) // 32
        a.block_begin = blocks
        for j, t in enumerate(taps):
            a.taps[j] = t
        blocks += a.bx * a.by * pack_groups(lib, T, len(taps), mode)
    return arr, blocks


# ---------------------------------------------------------------------------------------------- reduce
REDUCE_S = (1, 2, 3, 7, 8, 9, 17)
REDUCE_COCI = (132, 256 * 2 + 64, 64 * 3 + 1)                  # the last: scalar kinds only (the 16-byte kinds need CoCi % 4 == 0)
REDUCE_T = (1, 9, 27)
F = np.float32


def slab_sum(p):
    """The split sum of kinds 0 / 2, the bias path and wgrad_reduce_kernel. p: [S][...] float32.
    Eight accumulators over whole groups of eight splits, the remainder into the first, then ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7))."""
    S = p.shape[0]
    v = [np.zeros(p.shape[1:], F) for _ in range(8)]
    s = 0
    while s + 8 <= S:
        for u in range(8):
            v[u] = v[u] + p[s + u]
        s += 8
    while s < S:
        v[0] = v[0] + p[s]
        s += 1
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))


def wave_split_sum(p):
    """The split sum of kinds 1 / 3 and wgrad_reduce_small_kernel: wave w takes splits w, w+4, ... alternating between two
    accumulators, part_w = v0 + v1, then (part0 + part1) + (part2 + part3)."""
    S = p.shape[0]
    part = []
    for wv in range(4):
        v0, v1 = np.zeros(p.shape[1:], F), np.zeros(p.shape[1:], F)
        s = wv
        while s + 4 < S:
            v0 = v0 + p[s]
            v1 = v1 + p[s + 4]
            s += 8
        if s < S:
            v0 = v0 + p[s]
        part.append(v0 + v1)
    return (part[0] + part[1]) + (part[2] + part[3])


def reduce_expect(kind, T, CoCi, Cout, srcs, dw0, accum, tap_major, dbias0=None, accum_bias=0):
    """srcs: [{'slab': [S][ntaps][CoCi] float32, 'map': [T] slot or -1, 'bias': [S][Cout] or None}]. dw0: what the destination
    held ([CoCi][T], or [T][CoCi] tap-major). Returns (dw, dbias or None) as float32 arrays."""
    ssum = wave_split_sum if kind in (1, 3) else slab_sum
    dw = dw0.copy()
    for t in range(T):
        v, touched = None, False
        for k, sr in enumerate(srcs):
            j = sr['map'][t]
            vk = ssum(sr['slab'][:, j]) if j >= 0 else np.zeros(CoCi, F)
            touched = touched or j >= 0
            v = vk if k == 0 else v + vk
        if tap_major:
            if touched:
                dw[t] = dw[t] + v if accum else v
        else:
            dw[:, t] = dw[:, t] + v if accum else v
    db = None
    if dbias0 is not None:
        db = dbias0.copy()
        v = None
        for sr in srcs:
            if sr['bias'] is None:
                continue
            vk = slab_sum(sr['bias'])
            v = vk if v is None else v + vk
        if v is not None:
            db = db + v if accum_bias else v
    return dw, db


def reduce_nblocks(kind, CoCi, T):
    per = 256 if kind >= 2 else 64
    return ((CoCi + per - 1) // per) * (T if kind in (1, 3) else 1)


def reduce_table(WgradDest, WgradSrc, dests):
    """(ctypes array, total workgroups). dests = [dict(dw, dbias, CoCi, T, Cout, accum, accum_bias, kind, tap_major,
    srcs=[dict(slab, bias_slab, ntaps, S, map, tap_stride, split_stride)])] with device pointers as ints."""
    arr = (WgradDest * len(dests))()
    blocks = 0
    for a, d in zip(arr, dests):
        a.dw, a.dbias, a.CoCi, a.T, a.Cout = d['dw'], d.get('dbias') or None, d['CoCi'], d['T'], d['Cout']
        a.nsrc, a.accum, a.accum_bias, a.kind, a.tap_major = len(d['srcs']), d['accum'], d.get('accum_bias', 0), d['kind'], d['tap_major']
        a.block_begin, a.nblocks = blocks, reduce_nblocks(d['kind'], d['CoCi'], d['T'])
        blocks += a.nblocks
        for k, s in enumerate(d['srcs']):
            q = a.src[k]
            q.slab, q.bias_slab, q.ntaps, q.S = s['slab'], s.get('bias_slab') or None, s['ntaps'], s['S']
            for t in range(27):
                q.map[t] = s['map'][t] if t < len(s['map']) else -1
            q.tap_stride, q.split_stride = s['tap_stride'], s['split_stride']
    return arr, blocks
