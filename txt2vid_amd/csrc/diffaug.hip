// diffaug.hip — differentiable augmentation of the discriminator's inputs (DiffAugment, Zhao et al. 2020; opt-in through
// --D_aug, not in the reference), gfx950. One grouped launch per direction: every member tensor of a step (the real and the
// generated pyramid, up to T2V_MAX_GROUPS) is transformed per clip with the colour / translation / cutout map defined in
// include/t2v_hip.h and txt2vid_amd/functional_aug.py (`aug_params`). Launch-bound work (a pyramid level has 32 K elements at
// the benchmarked shapes): plain vector loads and stores, the clip reduction and the apply step in the same launch.
//
// Adaptive strength (ADA, Karras et al. 2020; opt-in through --D_aug_p / --D_ada). The GATED entry points
// t2v_diffaug_gated_fwd / _bwd are the same kernels with one more step in front: clip j of a member also reads row j * row_stride
// of the member's gate block g [rows, 8] (uniforms in [0, 1), drawn right behind u) and the probability p from DEVICE memory, and
// its effective policy is  policy & (1 [g0 < p] | 2 [g1 < p] | 4 [g2 < p])  (strict fp32 <; g == p: not applied). Everything
// behind that is the ungated code with that policy: p = 1 gives today's bits, an effective policy of 0 copies the clip (forward and
// adjoint), a clip without live colour sums nothing. Every part of a split clip reads the same gate row and the same p. The
// backward re-reads gates and p: p is written only by t2v_ada_update, which the trainer launches behind the D forward, never
// between an augmentation's forward and its backward. t2v_ada_update is the controller: one workgroup adds a D step's
// sum of sgn(u_real - u_fake) to the window kept in ada float32[8] = {p, sum, pairs, steps, 0...} and, every `interval` steps,
// moves p by +-step towards the target and clears the window (small integers: exact in fp32 in any order).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/t2v_hip.h"

#define T2V_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define S_(stream) ((hipStream_t)(stream))

static inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2V_OK : -(int)e - 1000;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block-wide sum for 256 threads in a fixed order; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* red /*4 floats*/) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

#define AUG_MAX_PARTS 16          // workgroups one clip is split over, at most
#define AUG_PART_ELEMS 8192       // elements of a clip per workgroup before it is split

struct AugBatch {
    t2v_aug_member m[T2V_MAX_GROUPS];
    int begin[T2V_MAX_GROUPS + 1];      // first workgroup of member g; a member owns N * parts[g] workgroups
    int parts[T2V_MAX_GROUPS];
    int n;
};

struct AugGate {
    const float* g[T2V_MAX_GROUPS];     // gate block of member g, or NULL: ungated
    const float* p;                     // the probability, one float in device memory
};

struct AugP {
    float b, s, c;            // brightness offset, saturation factor, contrast factor
    int tx, ty;               // out(h, w) = in(h - ty, w - tx)
    int x0, y0, size;         // zeroed box [x0, x0 + size) x [y0, y0 + size); size 0: none
};
// min(floor(u * n), n - 1) with the product exact (a 24-bit significand times a small integer fits a double)
__device__ __forceinline__ int aug_index(float u, int n) {
    int k = (int)floor((double)u * (double)n);
    k = k < 0 ? 0 : k;
    return k < n - 1 ? k : n - 1;
}
// the device mirror of functional_aug.aug_params
__device__ __forceinline__ AugP aug_params(const float* __restrict__ u, int S, int policy) {
    AugP p;
    p.b = 0.f; p.s = 1.f; p.c = 1.f; p.tx = p.ty = 0; p.x0 = p.y0 = 0; p.size = 0;
    if (policy & T2V_AUG_COLOR) { p.b = u[0] - 0.5f; p.s = 2.f * u[1]; p.c = u[2] + 0.5f; }
    if (policy & T2V_AUG_TRANSLATION) {
        const int r = (S + 4) / 8;
        p.tx = aug_index(u[3], 2 * r + 1) - r;
        p.ty = aug_index(u[4], 2 * r + 1) - r;
    }
    if (policy & T2V_AUG_CUTOUT) {
        p.size = (S + 1) / 2;
        const int n = S + 1 - (p.size & 1);
        p.x0 = aug_index(u[5], n) - p.size / 2;
        p.y0 = aug_index(u[6], n) - p.size / 2;
    }
    return p;
}
__device__ __forceinline__ bool aug_cut(const AugP& p, int h, int w) {
    return (unsigned)(w - p.x0) < (unsigned)p.size && (unsigned)(h - p.y0) < (unsigned)p.size;
}

// Which member, clip and part of the clip this workgroup serves.
#define AUG_LOCATE()                                                                       \
    int g = 0;                                                                             \
    while (g + 1 < tb.n && tb.begin[g + 1] <= (int)blockIdx.x) ++g;                        \
    const t2v_aug_member& m = tb.m[g];                                                     \
    const int parts = tb.parts[g];                                                         \
    const int local = (int)blockIdx.x - tb.begin[g];                                       \
    const int clip = local / parts, part = local - clip * parts;                           \
    const int S = m.S, C = m.C;                                                            \
    int policy = m.policy;                                                                 \
    if (GATED && tg.g[g]) {        /* uniform over the workgroup and over the parts of a clip */ \
        const float* __restrict__ gr = tg.g[g] + (long)clip * m.row_stride * T2V_AUG_K;    \
        const float pv = tg.p[0];                                                          \
        policy &= (gr[0] < pv ? T2V_AUG_COLOR : 0) | (gr[1] < pv ? T2V_AUG_TRANSLATION : 0) | (gr[2] < pv ? T2V_AUG_CUTOUT : 0); \
    }                                                                                      \
    const int V = m.T * S * S;                 /* voxels of one channel */                 \
    const int n = C * V;                       /* elements of the clip  */                 \
    const AugP p = aug_params(m.u + (long)clip * m.row_stride * T2V_AUG_K, S, policy);     \
    const int per = (V + parts - 1) / parts;                                               \
    const int v0 = part * per, v1 = min(V, v0 + per)

// (an effective policy of 0 falls through the same code: no sum, no shift, no box — a copy)
template <bool GATED>
__global__ __launch_bounds__(256) void diffaug_fwd_k(AugBatch tb, AugGate tg) {
    __shared__ float red[4];
    AUG_LOCATE();
    const float* __restrict__ x = m.x + (long)clip * n;
    float* __restrict__ y = m.y + (long)clip * n;
    float mu = 0.f;
    if (policy & T2V_AUG_COLOR) {
        // saturation keeps the channel mean: mu = mean(x) + b needs the clip sum of the input only. Every part of a clip sums the
        // whole clip (L2-resident) in the same order.
        float acc = 0.f;
        const int nv = (((uintptr_t)x & 15) == 0) ? (n >> 2) : 0;
        for (int q = threadIdx.x; q < nv; q += 256) {
            const float4 a = reinterpret_cast<const float4*>(x)[q];
            acc += (a.x + a.y) + (a.z + a.w);
        }
        for (int i = nv * 4 + threadIdx.x; i < n; i += 256) acc += x[i];
        mu = block_sum(acc, red) / (float)n + p.b;
    }
    const float invC = 1.f / (float)C;
    for (int v = v0 + threadIdx.x; v < v1; v += 256) {
        const int w = v % S, h = (v / S) % S;
        const int hs = h - p.ty, ws = w - p.tx;
        if (aug_cut(p, h, w) || (unsigned)hs >= (unsigned)S || (unsigned)ws >= (unsigned)S) {
            for (int c = 0; c < C; ++c) y[(long)c * V + v] = 0.f;
            continue;
        }
        const int src = v - (h * S + w) + hs * S + ws;
        if (!(policy & T2V_AUG_COLOR)) {
            for (int c = 0; c < C; ++c) y[(long)c * V + v] = x[(long)c * V + src];
            continue;
        }
        float mc = x[src];
        if (C > 1) {
            for (int c = 1; c < C; ++c) mc += x[(long)c * V + src];
            mc *= invC;
        }
        for (int c = 0; c < C; ++c) {
            const float xv = x[(long)c * V + src];
            const float t = (xv - mc) * p.s + (mc + p.b);
            y[(long)c * V + v] = (t - mu) * p.c + mu;
        }
    }
}

// dL/dx from dL/dy (m.x -> m.y). gcol = the gradient masked by the cutout and shifted back; then the colour map's adjoint.
template <bool GATED>
__global__ __launch_bounds__(256) void diffaug_bwd_k(AugBatch tb, AugGate tg) {
    __shared__ float red[4];
    AUG_LOCATE();
    const float* __restrict__ gy = m.x + (long)clip * n;
    float* __restrict__ gx = m.y + (long)clip * n;
    float gm = 0.f;
    if (policy & T2V_AUG_COLOR) {
        // clip sum of gcol = sum of dL/dy over the output voxels that are not cut and whose source lies inside the frame
        float acc = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int v = i % V, w = v % S, h = (v / S) % S;
            const bool keep = !aug_cut(p, h, w) && (unsigned)(h - p.ty) < (unsigned)S && (unsigned)(w - p.tx) < (unsigned)S;
            acc += keep ? gy[i] : 0.f;
        }
        gm = block_sum(acc, red) / (float)n;
    }
    const float invC = 1.f / (float)C;
    const float rest = (1.f - p.c) * gm;
    for (int v = v0 + threadIdx.x; v < v1; v += 256) {
        const int w = v % S, h = (v / S) % S;
        const int ho = h + p.ty, wo = w + p.tx;
        const bool valid = (unsigned)ho < (unsigned)S && (unsigned)wo < (unsigned)S && !aug_cut(p, ho, wo);
        const int dst = v - (h * S + w) + ho * S + wo;
        if (!(policy & T2V_AUG_COLOR)) {
            for (int c = 0; c < C; ++c) gx[(long)c * V + v] = valid ? gy[(long)c * V + dst] : 0.f;
            continue;
        }
        if (C == 1) {
            gx[v] = p.c * (valid ? gy[dst] : 0.f) + rest;
            continue;
        }
        float gc = 0.f;
        if (valid) for (int c = 0; c < C; ++c) gc += gy[(long)c * V + dst];
        const float pm = p.c * (gc * invC) + rest;                  // mean over channels of the contrast adjoint
        for (int c = 0; c < C; ++c) {
            const float g2 = p.c * (valid ? gy[(long)c * V + dst] : 0.f) + rest;
            gx[(long)c * V + v] = p.s * g2 + (1.f - p.s) * pm;
        }
    }
}

static int aug_batch(AugBatch& tb, const t2v_aug_member* ms, int n, long* blocks_out) {
    if (!ms || n < 1 || n > T2V_MAX_GROUPS) return T2V_EINVAL;
    long blocks = 0;
    for (int g = 0; g < T2V_MAX_GROUPS; ++g) {
        tb.begin[g] = (int)blocks;
        tb.parts[g] = 1;
        if (g >= n) { tb.m[g] = t2v_aug_member{}; continue; }
        const t2v_aug_member& q = ms[g];
        if (!q.x || !q.y || !q.u || q.x == q.y || q.N < 1 || q.C < 1 || q.T < 1 || q.S < 1) return T2V_EINVAL;
        if (q.policy < 1 || (q.policy & ~(T2V_AUG_COLOR | T2V_AUG_TRANSLATION | T2V_AUG_CUTOUT))) return T2V_EINVAL;
        if (q.row_stride < 1 || q.rows < 1 || (long)(q.N - 1) * q.row_stride >= (long)q.rows) return T2V_EINVAL;
        const long V = (long)q.T * q.S * q.S, elems = V * q.C;
        if (q.S > 32768 || elems > 0x40000000L) return T2V_EINVAL;
        long parts = (elems + AUG_PART_ELEMS - 1) / AUG_PART_ELEMS;
        parts = parts > AUG_MAX_PARTS ? AUG_MAX_PARTS : parts;
        parts = parts > V ? V : parts;
        tb.m[g] = q;
        tb.parts[g] = (int)parts;
        blocks += (long)q.N * parts;
        if (blocks > 0x7fffffffL) return T2V_EINVAL;
    }
    tb.begin[T2V_MAX_GROUPS] = (int)blocks;
    tb.n = n;
    *blocks_out = blocks;
    return T2V_OK;
}

extern "C" int t2v_diffaug_fwd(const t2v_aug_member* members, int n, void* st) {
    AugBatch tb;
    long blocks = 0;
    const int rc = aug_batch(tb, members, n, &blocks);
    if (rc != T2V_OK) return rc;
    T2V_LAUNCH(diffaug_fwd_k<false>, dim3((unsigned)blocks), dim3(256), 0, S_(st), tb, AugGate{});
    return launch_status();
}

extern "C" int t2v_diffaug_bwd(const t2v_aug_member* members, int n, void* st) {
    AugBatch tb;
    long blocks = 0;
    const int rc = aug_batch(tb, members, n, &blocks);
    if (rc != T2V_OK) return rc;
    T2V_LAUNCH(diffaug_bwd_k<false>, dim3((unsigned)blocks), dim3(256), 0, S_(st), tb, AugGate{});
    return launch_status();
}

static int aug_gate(AugGate& tg, const float* const* gates, int n, const float* p) {
    if (!gates || !p) return T2V_EINVAL;
    for (int g = 0; g < T2V_MAX_GROUPS; ++g) tg.g[g] = g < n ? gates[g] : nullptr;
    tg.p = p;
    return T2V_OK;
}

extern "C" int t2v_diffaug_gated_fwd(const t2v_aug_member* members, const float* const* gates, int n, const float* p, void* st) {
    AugBatch tb;
    AugGate tg;
    long blocks = 0;
    int rc = aug_batch(tb, members, n, &blocks);
    if (rc == T2V_OK) rc = aug_gate(tg, gates, n, p);
    if (rc != T2V_OK) return rc;
    T2V_LAUNCH(diffaug_fwd_k<true>, dim3((unsigned)blocks), dim3(256), 0, S_(st), tb, tg);
    return launch_status();
}

extern "C" int t2v_diffaug_gated_bwd(const t2v_aug_member* members, const float* const* gates, int n, const float* p, void* st) {
    AugBatch tb;
    AugGate tg;
    long blocks = 0;
    int rc = aug_batch(tb, members, n, &blocks);
    if (rc == T2V_OK) rc = aug_gate(tg, gates, n, p);
    if (rc != T2V_OK) return rc;
    T2V_LAUNCH(diffaug_bwd_k<true>, dim3((unsigned)blocks), dim3(256), 0, S_(st), tb, tg);
    return launch_status();
}

// ---- the controller of p ---------------------------------------------------------------------------------------------------
struct AdaBatch {
    t2v_ada_level l[T2V_MAX_GROUPS];
    int n;
};

// One workgroup. Every term is -1, 0 or +1 and there are at most a few thousand of them: the sums are exact in any order.
__global__ __launch_bounds__(256) void ada_update_k(float* __restrict__ ada, AdaBatch tb, float pairs, float target, float step,
                                                    float interval) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int g = 0; g < tb.n; ++g) {
        const float* __restrict__ r = tb.l[g].real;
        const float* __restrict__ f = tb.l[g].fake;
        for (int j = threadIdx.x; j < tb.l[g].count; j += 256) {
            const float a = r[j], b = f[j];
            acc += (a > b ? 1.f : 0.f) - (a < b ? 1.f : 0.f);             // sgn(a - b), 0 for a tie (and for a NaN)
        }
    }
    const float sum = block_sum(acc, red);
    if (threadIdx.x != 0) return;
    float p = ada[0], s = ada[1] + sum, c = ada[2] + pairs, k = ada[3] + 1.f;
    if (k >= interval) {
        const float rt = s / c;                                           // c >= 1
        const float dir = (rt > target ? 1.f : 0.f) - (rt < target ? 1.f : 0.f);
        p = p + dir * step;                                               // dir * step is exact: one rounding, in the add
        p = p < 0.f ? 0.f : p;
        p = p > 1.f ? 1.f : p;
        s = c = k = 0.f;
    }
    ada[0] = p; ada[1] = s; ada[2] = c; ada[3] = k;
}

extern "C" int t2v_ada_update(float* ada, const t2v_ada_level* levels, int n, float target, float step, int interval, void* st) {
    if (!ada || !levels || n < 1 || n > T2V_MAX_GROUPS || interval < 1) return T2V_EINVAL;
    if (!(step >= 0.f) || !(step <= 3.0e38f)) return T2V_EINVAL;          // negative, NaN or infinite
    AdaBatch tb;
    long pairs = 0;
    for (int g = 0; g < T2V_MAX_GROUPS; ++g) {
        tb.l[g] = g < n ? levels[g] : t2v_ada_level{};
        if (g >= n) continue;
        if (!levels[g].real || !levels[g].fake || levels[g].count < 1) return T2V_EINVAL;
        pairs += levels[g].count;
    }
    if (pairs > (1L << 24)) return T2V_EINVAL;                            // the window stays exact in fp32
    tb.n = n;
    T2V_LAUNCH(ada_update_k, dim3(1), dim3(256), 0, S_(st), ada, tb, (float)pairs, target, step, (float)interval);
    return launch_status();
}

// ---- LeCam regularisation of the discriminator (Tseng et al. 2021; opt-in through --D_lecam) ----------------------
// lecam float32[20] = {n, R_last, gate_last, L, alpha_R[0..7], alpha_F[0..7]}: the anchors are moving averages of D's own
// unconditional logits on real / generated clips, per pyramid level. The forward is ONE workgroup: per level the four sums
// (sum u_r, sum u_f, sum (u_r - alpha_F)^2, sum (u_f - alpha_R)^2) as per-thread strided partials, a 64-lane wave reduction and
// the four waves through LDS — a fixed order, no atomics — then thread 0 combines them in double (one rounding per stored
// float), stores the anchors IT USED and the gate into `saved` for the backward, moves the anchors and increments n.
#define LECAM_N 20
#define LECAM_AR 4
#define LECAM_AF 12

struct LecamBatch {
    t2v_ada_level l[T2V_MAX_GROUPS];
    int n;
};

struct LecamGradBatch {
    t2v_lecam_grad l[T2V_MAX_GROUPS];
    int n;
};

__global__ __launch_bounds__(256) void lecam_fwd_k(float* __restrict__ state, LecamBatch tb, float decay, float start,
                                                   float* __restrict__ saved, float* __restrict__ out) {
    __shared__ float red[4][4];
    __shared__ float sums[T2V_MAX_GROUPS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int g = 0; g < tb.n; ++g) {
        const float* __restrict__ r = tb.l[g].real;
        const float* __restrict__ f = tb.l[g].fake;
        const float aR = state[LECAM_AR + g], aF = state[LECAM_AF + g];      // (thread 0 writes them behind the last barrier)
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (long j = threadIdx.x; j < tb.l[g].count; j += 256) {
            const float a = r[j], b = f[j], da = a - aF, db = b - aR;
            v[0] += a;
            v[1] += b;
            v[2] += da * da;
            v[3] += db * db;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[wave][k] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 4) sums[g][threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float n = state[0];
    const float gate = n >= start ? 1.f : 0.f;                                // start >= 1: the first step has no anchors yet
    const double d = (double)decay;
    double R = 0.0;
    for (int g = 0; g < tb.n; ++g) {
        const double cnt = (double)tb.l[g].count;
        const float aR = state[LECAM_AR + g], aF = state[LECAM_AF + g];
        R += ((double)sums[g][2] + (double)sums[g][3]) / cnt;
        saved[g] = aR;
        saved[tb.n + g] = aF;
        const double mr = (double)sums[g][0] / cnt, mf = (double)sums[g][1] / cnt;
        state[LECAM_AR + g] = n == 0.f ? (float)mr : (float)(d * (double)aR + (1.0 - d) * mr);
        state[LECAM_AF + g] = n == 0.f ? (float)mf : (float)(d * (double)aF + (1.0 - d) * mf);
    }
    const float Rf = (float)(R / (double)tb.n);
    saved[2 * tb.n] = gate;
    out[0] = gate != 0.f ? Rf : 0.f;
    state[0] = n + 1.f;
    state[1] = Rf;
    state[2] = gate;
    state[3] = (float)tb.n;
}

// blockIdx.y: the level; its elements grid-strided over blockIdx.x. dL/du_r = gate * g * 2 (u_r - alpha_F) / (L * count), the
// anchors being constants of differentiation; exact zeros with the gate off.
__global__ __launch_bounds__(256) void lecam_bwd_k(LecamGradBatch tb, const float* __restrict__ saved, const float* __restrict__ gp) {
    const t2v_lecam_grad l = tb.l[blockIdx.y];
    const float aR = saved[blockIdx.y], aF = saved[tb.n + blockIdx.y], gate = saved[2 * tb.n];
    const float c = (gp[0] * 2.f) / ((float)tb.n * (float)l.count);
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < l.count; j += (long)gridDim.x * 256) {
        if (l.d_real) l.d_real[j] = gate != 0.f ? c * (l.real[j] - aF) : 0.f;
        if (l.d_fake) l.d_fake[j] = gate != 0.f ? c * (l.fake[j] - aR) : 0.f;
    }
}

extern "C" int t2v_lecam_fwd(float* state, const t2v_ada_level* levels, int n, float decay, int start, float* saved, float* out,
                             void* st) {
    if (!state || !levels || !saved || !out || n < 1 || n > T2V_MAX_GROUPS || start < 0) return T2V_EINVAL;
    if (!(decay >= 0.f) || !(decay < 1.f)) return T2V_EINVAL;                 // outside [0, 1), or NaN
    LecamBatch tb;
    for (int g = 0; g < T2V_MAX_GROUPS; ++g) {
        tb.l[g] = g < n ? levels[g] : t2v_ada_level{};
        if (g < n && (!levels[g].real || !levels[g].fake || levels[g].count < 1)) return T2V_EINVAL;
    }
    tb.n = n;
    T2V_LAUNCH(lecam_fwd_k, dim3(1), dim3(256), 0, S_(st), state, tb, decay, (float)(start < 1 ? 1 : start), saved, out);
    return launch_status();
}

extern "C" int t2v_lecam_bwd(const t2v_lecam_grad* levels, int n, const float* saved, const float* g, void* st) {
    if (!levels || !saved || !g || n < 1 || n > T2V_MAX_GROUPS) return T2V_EINVAL;
    LecamGradBatch tb;
    int most = 0;
    bool any = false;
    for (int k = 0; k < T2V_MAX_GROUPS; ++k) {
        tb.l[k] = k < n ? levels[k] : t2v_lecam_grad{};
        if (k >= n) continue;
        if (!levels[k].real || !levels[k].fake || levels[k].count < 1) return T2V_EINVAL;
        most = levels[k].count > most ? levels[k].count : most;
        any = any || levels[k].d_real || levels[k].d_fake;
    }
    if (!any) return T2V_OK;                                                  // no side needs a gradient: nothing to launch
    tb.n = n;
    long bx = ((long)most + 255) / 256;
    bx = bx > 1024 ? 1024 : bx;
    T2V_LAUNCH(lecam_bwd_k, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, S_(st), tb, saved, g);
    return launch_status();
}
