// mbstd.hip — the minibatch standard deviation head of the discriminator (opt-in, Resnet3D(mbstd=G); gfx950).
// One definition (include/t2v_hip.h, t2v_mbstd_*). Rows [i*seg, (i+1)*seg) of a member's features f [b, K] form a segment, runs of
// G consecutive rows inside a segment a group (the last one holds the remainder); per group q of n rows
//   mu_k = mean_b f_bk   v_k = mean_b (f_bk - mu_k)^2   sigma_k = sqrt(v_k + 1e-8)   s_q = mean_k sigma_k   y_h[b] = base_h[b] + w_h s_q(b)
// One workgroup per (member, group): a thread owns channels k, k + T, ... and holds the group's <= 16 rows of a channel in
// registers (row-contiguous loads, all of a channel's rows in flight at once); sums over K go through the wave, then through LDS
// in wave order. fp32, plain vector stores, no atomics, no workspace: the same bits run to run.
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

#define MB_T 256                          // threads per workgroup: 4 channels per thread at K = 1024
#define MB_W (MB_T / 64)
#define MB_G T2V_MBSTD_MAX_GROUP          // rows of a group at most
#define MB_EPS 1e-8f

// descriptors travel by value in the kernel arguments; begin[m] = first workgroup (= group) of member m
struct MbBatch { t2v_mbstd_member m[T2V_MAX_GROUPS]; int begin[T2V_MAX_GROUPS + 1]; int n; };

// the group a workgroup owns: its member, first row and row count
struct MbGroup { int mi, r0, n; };

__device__ __forceinline__ MbGroup mb_group_of(const MbBatch& tb, int wg, int G) {
    int mi = 0;
    while (mi + 1 < tb.n && wg >= tb.begin[mi + 1]) ++mi;
    const int seg = tb.m[mi].seg;
    const int per = (seg + G - 1) / G;                       // groups of one segment
    const int q = wg - tb.begin[mi];
    const int si = q / per, gi = q - si * per;
    MbGroup g;
    g.mi = mi;
    g.r0 = si * seg + gi * G;
    g.n = min(G, seg - gi * G);
    return g;
}

// the sum of `v` over the workgroup, in every thread: lanes in the wave's butterfly, then the waves in order
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < MB_W; ++i) t += red[i];
    return t;
}

// a_q = sum over the group's rows, then heads, of g_h[b] w_h (at most 32 terms, in every thread, in one order)
__device__ __forceinline__ float mb_aq(const t2v_mbstd_member& q, const float* __restrict__ w, int H, int r0, int n) {
    float a = 0.f;
    for (int j = 0; j < n; ++j)
        for (int h = 0; h < H; ++h)
            if (q.g[h]) a += q.g[h][r0 + j] * w[h];
    return a;
}

// the rows of channel k into registers (all loads issued before the first use), centred; ve = v_k + eps
__device__ __forceinline__ void mb_channel(const float* __restrict__ f, int K, int k, int n, float (&d)[MB_G], float& ve) {
#pragma unroll
    for (int j = 0; j < MB_G; ++j) d[j] = j < n ? f[(long)j * K + k] : 0.f;
    float mu = 0.f;
#pragma unroll
    for (int j = 0; j < MB_G; ++j) mu += d[j];
    mu /= (float)n;
    // centre twice: mu carries a rounding error of half an ulp of f, which is not small next to f - mu when the rows of a group
    // nearly coincide (the adjoints divide by sigma ~ |f - mu|); the mean of the residuals takes it out
    float res = 0.f;
#pragma unroll
    for (int j = 0; j < MB_G; ++j) {
        d[j] = j < n ? d[j] - mu : 0.f;
        res += d[j];
    }
    res /= (float)n;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < MB_G; ++j) {
        d[j] = j < n ? d[j] - res : 0.f;
        v += d[j] * d[j];
    }
    ve = v / (float)n + MB_EPS;
}

// fwd: stat[b] = s_q(b), y_h[b] = (base_h ? base_h[b] : 0) + w_h s_q(b)
__global__ __launch_bounds__(MB_T) void mbstd_fwd_k(const MbBatch tb, const float* __restrict__ w, int H, int K, int G) {
    __shared__ float red[MB_W];
    const MbGroup gr = mb_group_of(tb, blockIdx.x, G);
    const t2v_mbstd_member& q = tb.m[gr.mi];
    const float* __restrict__ f = q.f + (long)gr.r0 * K;
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += MB_T) {
        float d[MB_G], ve;
        mb_channel(f, K, k, gr.n, d, ve);
        acc += sqrtf(ve);
    }
    const float s = block_sum(acc, red) / (float)K;
    if ((int)threadIdx.x < gr.n) {
        const int r = gr.r0 + threadIdx.x;
        if (q.stat) q.stat[r] = s;
        for (int h = 0; h < H; ++h)
            if (q.y[h]) q.y[h][r] = (q.base[h] ? q.base[h][r] : 0.f) + w[h] * s;
    }
}

// feat: F[b,k] = a_q (f_bk - mu_k) / (n K sigma_k)
__global__ __launch_bounds__(MB_T) void mbstd_feat_k(const MbBatch tb, const float* __restrict__ w, int H, int K, int G) {
    const MbGroup gr = mb_group_of(tb, blockIdx.x, G);
    const t2v_mbstd_member& q = tb.m[gr.mi];
    const float* __restrict__ f = q.f + (long)gr.r0 * K;
    float* __restrict__ out = q.out + (long)gr.r0 * K;
    const float c = mb_aq(q, w, H, gr.r0, gr.n) / ((float)gr.n * (float)K);
    for (int k = threadIdx.x; k < K; k += MB_T) {
        float d[MB_G], ve;
        mb_channel(f, K, k, gr.n, d, ve);
        const float cs = c / sqrtf(ve);
#pragma unroll
        for (int j = 0; j < MB_G; ++j)
            if (j < gr.n) out[(long)j * K + k] = cs * d[j];
    }
}

// second: with Gam = dL/dF,  t_q = sum_bk Gam_bk (f_bk - mu_k) / (n K sigma_k)  ->  stat[b] = t_q(b), y_h[b] = w_h t_q(b);
//   out[b,k] = (a_q / (n K)) [ (Gam_bk - mean_b Gam_k) / sigma_k - (f_bk - mu_k) sum_b' Gam_b'k (f_b'k - mu_k) / (n sigma_k^3) ]
__global__ __launch_bounds__(MB_T) void mbstd_second_k(const MbBatch tb, const float* __restrict__ w, int H, int K, int G) {
    __shared__ float red[MB_W];
    const MbGroup gr = mb_group_of(tb, blockIdx.x, G);
    const t2v_mbstd_member& q = tb.m[gr.mi];
    const float* __restrict__ f = q.f + (long)gr.r0 * K;
    const float* __restrict__ gam = q.gam + (long)gr.r0 * K;
    float* __restrict__ out = q.out ? q.out + (long)gr.r0 * K : nullptr;
    const float fn = (float)gr.n;
    const float c = out ? mb_aq(q, w, H, gr.r0, gr.n) / (fn * (float)K) : 0.f;
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += MB_T) {
        float e[MB_G];
#pragma unroll
        for (int j = 0; j < MB_G; ++j) e[j] = j < gr.n ? gam[(long)j * K + k] : 0.f;
        float d[MB_G], ve;
        mb_channel(f, K, k, gr.n, d, ve);
        float em = 0.f, p = 0.f;
#pragma unroll
        for (int j = 0; j < MB_G; ++j) {
            em += e[j];
            p += e[j] * d[j];
        }
        em /= fn;
        float er = 0.f;                                          // (Gam centred twice, like f)
#pragma unroll
        for (int j = 0; j < MB_G; ++j) {
            e[j] = j < gr.n ? e[j] - em : 0.f;
            er += e[j];
        }
        er /= fn;
        const float is = 1.f / sqrtf(ve);
        acc += p * is;
        if (out) {
            const float pk = p / (fn * ve), cs = c * is;       // (sigma^2 as it was summed, not sqrt squared)
#pragma unroll
            for (int j = 0; j < MB_G; ++j)
                if (j < gr.n) out[(long)j * K + k] = cs * ((e[j] - er) - d[j] * pk);
        }
    }
    const float t = block_sum(acc, red) / (fn * (float)K);
    if ((int)threadIdx.x < gr.n) {
        const int r = gr.r0 + threadIdx.x;
        if (q.stat) q.stat[r] = t;
        for (int h = 0; h < H; ++h)
            if (q.y[h]) q.y[h][r] = w[h] * t;
    }
}

// weight: W[h] (+)= sum over members, then rows, of g_h[b] stat[b] (a head whose g is NULL adds nothing). One workgroup, wave h
// owns head h: lane l adds the rows l, l + 64, ... of the members' concatenation, then the wave's butterfly.
__global__ __launch_bounds__(64 * T2V_MBSTD_MAX_HEADS) void mbstd_weight_k(const MbBatch tb, float* __restrict__ W, int H, int accum) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    if (h >= H) return;
    float acc = 0.f;
    int at = 0;                                              // rows before member mi, modulo 64
    for (int mi = 0; mi < tb.n; ++mi) {
        const t2v_mbstd_member& q = tb.m[mi];
        if (q.g[h])
            for (int r = (lane - at + 64) & 63; r < q.b; r += 64) acc += q.g[h][r] * q.stat[r];
        at = (at + q.b) & 63;
    }
    acc = wave_sum(acc);
    if (lane == 0) W[h] = accum ? W[h] + acc : acc;
}

enum { MB_FWD, MB_FEAT, MB_SECOND, MB_WEIGHT };

// every refusal of the family, before any launch; fills the by-value table
static bool mb_table(int role, const t2v_mbstd_member* members, int n, const float* w, int H, int K, int G, MbBatch& tb) {
    if (!members || !w || n < 1 || n > T2V_MAX_GROUPS || K < 1 || H < 1 || H > T2V_MBSTD_MAX_HEADS || G < 2 || G > T2V_MBSTD_MAX_GROUP)
        return false;
    long groups = 0;
    for (int i = 0; i < n; ++i) {
        const t2v_mbstd_member& q = members[i];
        if (q.b < 1 || q.seg < 1 || q.b % q.seg != 0) return false;
        bool any_g = false, any_y = false;
        for (int h = 0; h < H; ++h) {
            any_g = any_g || q.g[h];
            any_y = any_y || q.y[h];
        }
        switch (role) {
        case MB_FWD: if (!q.f || !any_y) return false; break;
        case MB_FEAT: if (!q.f || !q.out || !any_g) return false; break;
        case MB_SECOND: if (!q.f || !q.gam || (q.out && !any_g) || (!q.out && !q.stat && !any_y)) return false; break;
        default: if (!q.stat || !any_g) return false; break;
        }
        tb.m[i] = q;
        for (int h = H; h < T2V_MBSTD_MAX_HEADS; ++h) tb.m[i].g[h] = tb.m[i].base[h] = nullptr, tb.m[i].y[h] = nullptr;
        tb.begin[i] = (int)groups;
        groups += (long)(q.b / q.seg) * ((q.seg + G - 1) / G);
        if (groups > 0x7fffffffL) return false;
    }
    tb.begin[n] = (int)groups;
    tb.n = n;
    return true;
}

extern "C" int t2v_mbstd_fwd(const t2v_mbstd_member* members, int n, const float* w, int H, int K, int G, void* st) {
    MbBatch tb;
    if (!mb_table(MB_FWD, members, n, w, H, K, G, tb)) return T2V_EINVAL;
    T2V_LAUNCH(mbstd_fwd_k, dim3(tb.begin[n]), dim3(MB_T), 0, S_(st), tb, w, H, K, G);
    return launch_status();
}

extern "C" int t2v_mbstd_feat(const t2v_mbstd_member* members, int n, const float* w, int H, int K, int G, void* st) {
    MbBatch tb;
    if (!mb_table(MB_FEAT, members, n, w, H, K, G, tb)) return T2V_EINVAL;
    T2V_LAUNCH(mbstd_feat_k, dim3(tb.begin[n]), dim3(MB_T), 0, S_(st), tb, w, H, K, G);
    return launch_status();
}

extern "C" int t2v_mbstd_second(const t2v_mbstd_member* members, int n, const float* w, int H, int K, int G, void* st) {
    MbBatch tb;
    if (!mb_table(MB_SECOND, members, n, w, H, K, G, tb)) return T2V_EINVAL;
    T2V_LAUNCH(mbstd_second_k, dim3(tb.begin[n]), dim3(MB_T), 0, S_(st), tb, w, H, K, G);
    return launch_status();
}

extern "C" int t2v_mbstd_weight(const t2v_mbstd_member* members, int n, float* W, int H, int K, int G, int accum, void* st) {
    MbBatch tb;
    if (!mb_table(MB_WEIGHT, members, n, W, H, K, G, tb)) return T2V_EINVAL;
    T2V_LAUNCH(mbstd_weight_k, dim3(1), dim3(64 * T2V_MBSTD_MAX_HEADS), 0, S_(st), tb, W, H, accum ? 1 : 0);
    return launch_status();
}
