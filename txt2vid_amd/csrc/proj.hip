// proj.hip — the projection head of the text-conditioned discriminator (opt-in, Resnet3D(proj=True); gfx950).
// One trilinear form T(g, f, s; V) = sum_b g[b] sum_kj f[b,k] V[k,j] s[b,j] and its four contractions (include/t2v_hip.h,
// t2v_proj_*). V [K, J] row-major is the only large operand (1 MB at 1024 x 256); rows are few (<= 64 per member), so every
// kernel streams V lane-contiguously from L2 and reduces in registers, then in-wave, then through LDS in a fixed order.
// fp32, plain vector stores, no atomics, no workspace: the same bits run to run.
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

// descriptors travel by value in the kernel arguments; begin[m] = first workgroup (= row) of member m
struct ProjBatch { t2v_proj_member m[T2V_MAX_GROUPS]; int begin[T2V_MAX_GROUPS + 1]; int n; };

__device__ __forceinline__ int proj_member_of(const ProjBatch& tb, int row) {
    int mi = 0;
    while (mi + 1 < tb.n && row >= tb.begin[mi + 1]) ++mi;
    return mi;
}

// The loops below are latency-bound (one workgroup per row, V from L2): every thread keeps PROJ_R independent loads of V in flight
// per step instead of one, and a workgroup is 16 waves so that a row's K x J walk is short.
#define PROJ_T 1024                       // threads per workgroup of the row kernels
#define PROJ_W (PROJ_T / 64)
#define PROJ_R 8                          // rows of V a wave takes per step

// rows: y[b] = base[b] + sum_kj f[b,k] V[k,j] s[b,j]. One workgroup per (member, row); a wave takes PROJ_R rows k of V per step,
// lanes along j; per-lane partial sums, one wave reduction at the end, the 16 waves through LDS in wave order.
__global__ __launch_bounds__(PROJ_T) void proj_rows_k(const ProjBatch tb, const float* __restrict__ V, int K, int J) {
    __shared__ float red[PROJ_W];
    const int mi = proj_member_of(tb, blockIdx.x);
    const t2v_proj_member& q = tb.m[mi];
    const int r = blockIdx.x - tb.begin[mi];
    const float* __restrict__ f = q.f + (long)r * K;
    const float* __restrict__ s = q.s + (long)r * J;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float acc = 0.f;
    for (int k0 = w * PROJ_R; k0 < K; k0 += PROJ_W * PROJ_R) {
        float fk[PROJ_R];
#pragma unroll
        for (int u = 0; u < PROJ_R; ++u) fk[u] = k0 + u < K ? f[k0 + u] : 0.f;
        for (int j = lane; j < J; j += 64) {
            float v[PROJ_R];
#pragma unroll
            for (int u = 0; u < PROJ_R; ++u) v[u] = k0 + u < K ? V[(long)(k0 + u) * J + j] : 0.f;
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < PROJ_R; ++u) a += fk[u] * v[u];
            acc += a * s[j];
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < PROJ_W; ++i) t += red[i];
        q.out[r] = q.base ? q.base[r] + t : t;
    }
}

// feat: F[b,k] = g[b] * sum_j V[k,j] s[b,j]. One workgroup per (member, row); a wave takes PROJ_R rows k of V per step, lanes
// along j, one wave reduction per row.
__global__ __launch_bounds__(PROJ_T) void proj_feat_k(const ProjBatch tb, const float* __restrict__ V, int K, int J) {
    const int mi = proj_member_of(tb, blockIdx.x);
    const t2v_proj_member& q = tb.m[mi];
    const int r = blockIdx.x - tb.begin[mi];
    const float* __restrict__ s = q.s + (long)r * J;
    float* __restrict__ out = q.out + (long)r * K;
    const float g = q.g[r];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k0 = w * PROJ_R; k0 < K; k0 += PROJ_W * PROJ_R) {
        float a[PROJ_R];
#pragma unroll
        for (int u = 0; u < PROJ_R; ++u) a[u] = 0.f;
        for (int j = lane; j < J; j += 64) {
            const float sj = s[j];
            float v[PROJ_R];
#pragma unroll
            for (int u = 0; u < PROJ_R; ++u) v[u] = k0 + u < K ? V[(long)(k0 + u) * J + j] : 0.f;
#pragma unroll
            for (int u = 0; u < PROJ_R; ++u) a[u] += v[u] * sj;
        }
        float mine = 0.f;
#pragma unroll
        for (int u = 0; u < PROJ_R; ++u) {
            const float t = wave_sum(a[u]);
            if (lane == u) mine = t;
        }
        if (lane < PROJ_R && k0 + lane < K) out[k0 + lane] = g * mine;
    }
}

// cond: C[b,j] = g[b] * sum_k f[b,k] V[k,j]. One workgroup per (member, row); 64 columns per pass (lanes), a wave takes PROJ_R
// rows k per step; the 16 waves' partial sums meet in LDS and are added in wave order.
__global__ __launch_bounds__(PROJ_T) void proj_cond_k(const ProjBatch tb, const float* __restrict__ V, int K, int J) {
    __shared__ float part[PROJ_W][64];
    const int mi = proj_member_of(tb, blockIdx.x);
    const t2v_proj_member& q = tb.m[mi];
    const int r = blockIdx.x - tb.begin[mi];
    const float* __restrict__ f = q.f + (long)r * K;
    float* __restrict__ out = q.out + (long)r * J;
    const float g = q.g[r];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        float acc = 0.f;
        if (j < J)
            for (int k0 = w * PROJ_R; k0 < K; k0 += PROJ_W * PROJ_R) {
                float v[PROJ_R];
#pragma unroll
                for (int u = 0; u < PROJ_R; ++u) v[u] = k0 + u < K ? V[(long)(k0 + u) * J + j] : 0.f;
#pragma unroll
                for (int u = 0; u < PROJ_R; ++u) acc += (k0 + u < K ? f[k0 + u] : 0.f) * v[u];
            }
        part[w][lane] = acc;
        __syncthreads();
        if (w == 0 && j < J) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < PROJ_W; ++i) t += part[i][lane];
            out[j] = g * t;
        }
        __syncthreads();
    }
}

// weight: W[k,j] (+)= sum over members, then rows, of g[b] f[b,k] s[b,j]. A workgroup owns a 16 x 64 tile of W (thread: 4 rows k,
// one column j) and walks every row of every member in order, PROJ_R rows per step.
#define PROJ_WK 16
__global__ __launch_bounds__(256) void proj_weight_k(const ProjBatch tb, float* __restrict__ W, int K, int J, int accum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    if (j >= J) return;
    for (long kt = blockIdx.y; kt * PROJ_WK + w * 4 < K; kt += gridDim.y) {
        const int k0 = (int)(kt * PROJ_WK) + w * 4;
        const int nk = min(4, K - k0);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int mi = 0; mi < tb.n; ++mi) {
            const t2v_proj_member& q = tb.m[mi];
            for (int r0 = 0; r0 < q.b; r0 += PROJ_R) {
                float gs[PROJ_R], fv[PROJ_R][4];
#pragma unroll
                for (int u = 0; u < PROJ_R; ++u) {
                    const bool in = r0 + u < q.b;
                    const int r = in ? r0 + u : r0;
                    gs[u] = in ? q.g[r] * q.s[(long)r * J + j] : 0.f;
                    const float* __restrict__ f = q.f + (long)r * K + k0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) fv[u][c] = c < nk ? f[c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < PROJ_R; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] += fv[u][c] * gs[u];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nk) {
                float* o = W + (long)(k0 + c) * J + j;
                *o = accum ? *o + acc[c] : acc[c];
            }
    }
}

enum { PROJ_ROWS, PROJ_FEAT, PROJ_COND, PROJ_WEIGHT };

// every refusal of the family, before any launch; fills the by-value table
static bool proj_table(int role, const t2v_proj_member* members, int n, const float* V, int K, int J, ProjBatch& tb) {
    if (!members || !V || n < 1 || n > T2V_MAX_GROUPS || K < 1 || J < 1) return false;
    long rows = 0;
    for (int i = 0; i < n; ++i) {
        const t2v_proj_member& q = members[i];
        if (q.b < 1) return false;
        const bool need_g = role != PROJ_ROWS, need_f = role != PROJ_FEAT, need_s = role != PROJ_COND;
        if ((need_g && !q.g) || (need_f && !q.f) || (need_s && !q.s) || (role != PROJ_WEIGHT && !q.out)) return false;
        tb.m[i] = q;
        tb.begin[i] = (int)rows;
        rows += q.b;
        if (rows > 0x7fffffffL) return false;
    }
    tb.begin[n] = (int)rows;
    tb.n = n;
    return true;
}

extern "C" int t2v_proj_rows(const t2v_proj_member* members, int n, const float* V, int K, int J, void* st) {
    ProjBatch tb;
    if (!proj_table(PROJ_ROWS, members, n, V, K, J, tb)) return T2V_EINVAL;
    T2V_LAUNCH(proj_rows_k, dim3(tb.begin[n]), dim3(PROJ_T), 0, S_(st), tb, V, K, J);
    return launch_status();
}

extern "C" int t2v_proj_feat(const t2v_proj_member* members, int n, const float* V, int K, int J, void* st) {
    ProjBatch tb;
    if (!proj_table(PROJ_FEAT, members, n, V, K, J, tb)) return T2V_EINVAL;
    T2V_LAUNCH(proj_feat_k, dim3(tb.begin[n]), dim3(PROJ_T), 0, S_(st), tb, V, K, J);
    return launch_status();
}

extern "C" int t2v_proj_cond(const t2v_proj_member* members, int n, const float* V, int K, int J, void* st) {
    ProjBatch tb;
    if (!proj_table(PROJ_COND, members, n, V, K, J, tb)) return T2V_EINVAL;
    T2V_LAUNCH(proj_cond_k, dim3(tb.begin[n]), dim3(PROJ_T), 0, S_(st), tb, V, K, J);
    return launch_status();
}

extern "C" int t2v_proj_weight(const t2v_proj_member* members, int n, float* W, int K, int J, int accum, void* st) {
    ProjBatch tb;
    if (!proj_table(PROJ_WEIGHT, members, n, W, K, J, tb)) return T2V_EINVAL;
    long gy = ((long)K + PROJ_WK - 1) / PROJ_WK;
    if (gy > 65535) gy = 65535;              // (the kernel strides over the tiles beyond)
    T2V_LAUNCH(proj_weight_k, dim3((J + 63) / 64, (unsigned)gy), dim3(256), 0, S_(st), tb, W, K, J, accum ? 1 : 0);
    return launch_status();
}
