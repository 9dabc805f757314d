// spectral.hip — spectral normalisation of the discriminator's weights (Miyato et al. 2018; opt-in through --D_sn, not in the
// reference), gfx950. Grouped like t2v_adam_multi / t2v_ema_multi: up to T2V_SN_MAX_JOBS weight matrices W [M, K] per call, the job
// table by value in the kernel arguments, every launch serving all jobs. One refresh is
//     t = W^T u ; v = t / max(|t|, eps) ; s = W v ; u = s / max(|s|, eps) ; sigma = u . s ; What = W / sigma
// and the gradient projection  c = <G, What> ; G <- (G - c u v^T) / sigma  (include/t2v_hip.h).
//
// Bandwidth- and latency-bound reductions, no MFMA. There are no floating-point atomics: a sum that spans workgroups leaves
// per-workgroup partial sums in the caller's workspace and a later launch adds them in a fixed order, so results are the same
// bits run to run and replay to eager. The column pass (W^T u) and the row pass (W v) split the matrix differently: columns are
// coalesced across lanes with the rows cut into slices of SN_ROWS; rows are reduced by one workgroup (long rows) or one wave
// (short rows) each.
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
    return (red[0] + red[1]) + (red[2] + red[3]);
}

#define SN_COLS 1024          // columns per workgroup of the column pass (4 per thread)
#define SN_ROWS 32            // rows per slice of the column pass
#define SN_ROW_WG_K 512       // rows at least this long are reduced by a whole workgroup, shorter ones by one wave
#define SN_CHUNK 4096         // elements per workgroup of the streaming passes

enum { SN_G_COL = 0, SN_G_TILE = 1, SN_G_ROW = 2, SN_G_CHUNK = 3, SN_GRIDS = 4 };

// Workspace of one job, in floats from ws + off: part [slices][K] | t [K] | tss [tiles] | s [M] | cpart [chunks] | c [1]
struct SnBatch {
    float* w[T2V_SN_MAX_JOBS]; float* what[T2V_SN_MAX_JOBS]; float* u[T2V_SN_MAX_JOBS]; float* v[T2V_SN_MAX_JOBS];
    float* sigma[T2V_SN_MAX_JOBS]; float* g[T2V_SN_MAX_JOBS];
    int M[T2V_SN_MAX_JOBS]; int K[T2V_SN_MAX_JOBS]; int off[T2V_SN_MAX_JOBS];
    int begin[SN_GRIDS][T2V_SN_MAX_JOBS + 1];      // first workgroup of job j in each of the four grid shapes
    int njobs;
};
static_assert(sizeof(SnBatch) < 4096 - 64, "SnBatch travels by value in the kernel arguments (4 KB limit)");

struct SnWs { float *part, *t, *tss, *s, *cpart, *c; };

__host__ __device__ __forceinline__ int sn_slices(int M) { return (M + SN_ROWS - 1) / SN_ROWS; }
__host__ __device__ __forceinline__ int sn_tiles(int K) { return (K + SN_COLS - 1) / SN_COLS; }
__host__ __device__ __forceinline__ int sn_chunks(int M, int K) { return (int)(((long)M * K + SN_CHUNK - 1) / SN_CHUNK); }
__host__ __device__ __forceinline__ long sn_job_floats(int M, int K) {
    const long n = (long)sn_slices(M) * K + K + sn_tiles(K) + M + sn_chunks(M, K) + 1;
    return (n + 3) & ~3L;                          // every job's block starts 16-byte aligned
}
__device__ __forceinline__ SnWs sn_ws(float* ws, int off, int M, int K) {
    SnWs r;
    r.part = ws + off;
    r.t = r.part + (long)sn_slices(M) * K;
    r.tss = r.t + K;
    r.s = r.tss + sn_tiles(K);
    r.cpart = r.s + M;
    r.c = r.cpart + sn_chunks(M, K);
    return r;
}

// largest j with begin[j] <= blockIdx.x
#define SN_LOCATE(grid)                                                                                                  \
    int lo = 0, hi = tb.njobs;                                                                                          \
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tb.begin[grid][mid] <= (int)blockIdx.x) lo = mid; else hi = mid; } \
    const int j = lo;                                                                                                   \
    const int local = (int)blockIdx.x - tb.begin[grid][j];                                                              \
    const int M = tb.M[j], K = tb.K[j];                                                                                 \
    const SnWs q = sn_ws(ws, tb.off[j], M, K)

// ---- column pass, stage 1: part[slice][k] = sum over the slice's rows (ascending) of W[m][k] u[m]
__global__ __launch_bounds__(256) void sn_col_partial_k(SnBatch tb, float* ws, int from_param) {
    SN_LOCATE(SN_G_COL);
    const int tiles = sn_tiles(K);
    const int slice = local / tiles, tile = local - slice * tiles;
    const float* __restrict__ W = from_param ? tb.what[j] : tb.w[j];
    const float* __restrict__ u = tb.u[j];
    const int m0 = slice * SN_ROWS, m1 = min(M, m0 + SN_ROWS);
    float* __restrict__ out = q.part + (long)slice * K;
    const int c0 = tile * SN_COLS;
    if ((K & 3) == 0 && (((uintptr_t)W | (uintptr_t)out) & 15) == 0) {
        // 16-byte loads: this thread owns four adjacent columns (K % 4 == 0, so it has all four or none)
        const int k = c0 + 4 * (int)threadIdx.x;
        if (k < K) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
            for (int m = m0; m < m1; ++m) {
                const float4 a = *reinterpret_cast<const float4*>(W + (long)m * K + k);
                const float um = u[m];
                acc.x += a.x * um; acc.y += a.y * um; acc.z += a.z * um; acc.w += a.w * um;
            }
            *reinterpret_cast<float4*>(out + k) = acc;
        }
        return;
    }
    // any K, any alignment: four columns 256 apart per thread (coalesced 4-byte loads); each column sums its rows in the same order
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int m = m0; m < m1; ++m) {
        const float um = u[m];
        const float* __restrict__ row = W + (long)m * K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = c0 + (int)threadIdx.x + 256 * i;
            if (k < K) acc[i] += row[k] * um;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = c0 + (int)threadIdx.x + 256 * i;
        if (k < K) out[k] = acc[i];
    }
}

// ---- column pass, stage 2: t[k] = sum over slices (ascending) of part[slice][k]; tss[tile] = sum of t[k]^2 over the tile
__global__ __launch_bounds__(256) void sn_col_finish_k(SnBatch tb, float* ws) {
    __shared__ float red[4];
    SN_LOCATE(SN_G_TILE);
    const int slices = sn_slices(M);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = local * SN_COLS + (int)threadIdx.x + 256 * i;
        if (k < K) {
            float t = q.part[k];
            for (int sl = 1; sl < slices; ++sl) t += q.part[(long)sl * K + k];
            q.t[k] = t;
            ss += t * t;
        }
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) q.tss[local] = ss;
}

// ---- v = t / max(|t|, eps); |t|^2 = the tiles' sums in ascending order (every workgroup of a job computes the same bits)
__global__ __launch_bounds__(256) void sn_v_k(SnBatch tb, float* ws, float eps) {
    SN_LOCATE(SN_G_TILE);
    const int tiles = sn_tiles(K);
    float ss = q.tss[0];
    for (int i = 1; i < tiles; ++i) ss += q.tss[i];
    const float d = fmaxf(sqrtf(ss), eps);
    float* __restrict__ v = tb.v[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = local * SN_COLS + (int)threadIdx.x + 256 * i;
        if (k < K) v[k] = q.t[k] / d;
    }
}

// ---- row pass: s[m] = sum_k W[m][k] v[k]. K >= SN_ROW_WG_K: one workgroup per row; else one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void sn_row_k(SnBatch tb, float* ws, int from_param) {
    __shared__ float red[4];
    SN_LOCATE(SN_G_ROW);
    const float* __restrict__ W = from_param ? tb.what[j] : tb.w[j];
    const float* __restrict__ v = tb.v[j];
    if (K >= SN_ROW_WG_K) {
        const float* __restrict__ row = W + (long)local * K;
        float acc = 0.f;
        const int nv = ((((uintptr_t)row | (uintptr_t)v) & 15) == 0) ? (K >> 2) : 0;
        for (int p = threadIdx.x; p < nv; p += 256) {
            const float4 a = reinterpret_cast<const float4*>(row)[p];
            const float4 b = reinterpret_cast<const float4*>(v)[p];
            acc += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
        }
        for (int k = nv * 4 + threadIdx.x; k < K; k += 256) acc += row[k] * v[k];
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) q.s[local] = acc;
        return;
    }
    const int m = local * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;                                   // (whole waves leave; no barrier follows)
    const float* __restrict__ row = W + (long)m * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc += row[k] * v[k];
    acc = wave_sum(acc);
    if (lane == 0) q.s[m] = acc;
}

// ---- one workgroup per job: u = s / max(|s|, eps) ; sigma = u . s
__global__ __launch_bounds__(256) void sn_u_sigma_k(SnBatch tb, float* ws, float eps) {
    __shared__ float red[4];
    const int j = blockIdx.x;
    const int M = tb.M[j], K = tb.K[j];
    const SnWs q = sn_ws(ws, tb.off[j], M, K);
    float* __restrict__ u = tb.u[j];
    float ss = 0.f;
    for (int m = threadIdx.x; m < M; m += 256) ss += q.s[m] * q.s[m];
    ss = block_sum(ss, red);
    const float d = fmaxf(sqrtf(ss), eps);
    float dot = 0.f;
    for (int m = threadIdx.x; m < M; m += 256) {
        const float um = q.s[m] / d;
        u[m] = um;
        dot += um * q.s[m];
    }
    dot = block_sum(dot, red);
    if (threadIdx.x == 0) tb.sigma[j][0] = dot;
}

// sigma == 0 (W v = 0: a zero matrix, or u starting orthogonal to the range) divides by 1 instead: What = W, no NaN
__device__ __forceinline__ float sn_divisor(float sigma) { return sigma != 0.f ? sigma : 1.f; }

// ---- What = W / sigma over 4096-element chunks; from_param: the parameter's storage holds W — save it to the master first
__global__ __launch_bounds__(256) void sn_scale_k(SnBatch tb, float* ws, int from_param) {
    SN_LOCATE(SN_G_CHUNK);
    (void)q;
    const long base = (long)local * SN_CHUNK;
    const int len = (int)min((long)SN_CHUNK, (long)M * K - base);
    float* __restrict__ w = tb.w[j] + base;
    float* __restrict__ p = tb.what[j] + base;
    const float d = sn_divisor(tb.sigma[j][0]);
    const int nv = ((((uintptr_t)w | (uintptr_t)p) & 15) == 0) ? (len >> 2) : 0;
    for (int i = threadIdx.x; i < nv; i += 256) {
        float4 a;
        if (from_param) { a = reinterpret_cast<float4*>(p)[i]; reinterpret_cast<float4*>(w)[i] = a; }
        else a = reinterpret_cast<const float4*>(w)[i];
        a.x /= d; a.y /= d; a.z /= d; a.w /= d;
        reinterpret_cast<float4*>(p)[i] = a;
    }
    for (int i = nv * 4 + threadIdx.x; i < len; i += 256) {
        float a;
        if (from_param) { a = p[i]; w[i] = a; } else a = w[i];
        p[i] = a / d;
    }
}

// ---- projection, stage 1: cpart[chunk] = sum over the chunk of G What
__global__ __launch_bounds__(256) void sn_dot_partial_k(SnBatch tb, float* ws) {
    __shared__ float red[4];
    SN_LOCATE(SN_G_CHUNK);
    const long base = (long)local * SN_CHUNK;
    const int len = (int)min((long)SN_CHUNK, (long)M * K - base);
    const float* __restrict__ g = tb.g[j] + base;
    const float* __restrict__ p = tb.what[j] + base;
    float acc = 0.f;
    const int nv = ((((uintptr_t)g | (uintptr_t)p) & 15) == 0) ? (len >> 2) : 0;
    for (int i = threadIdx.x; i < nv; i += 256) {
        const float4 a = reinterpret_cast<const float4*>(g)[i];
        const float4 b = reinterpret_cast<const float4*>(p)[i];
        acc += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
    }
    for (int i = nv * 4 + threadIdx.x; i < len; i += 256) acc += g[i] * p[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) q.cpart[local] = acc;
}

// ---- projection, stage 2 (one workgroup per job): c = sum of the chunks' partial sums
__global__ __launch_bounds__(256) void sn_dot_finish_k(SnBatch tb, float* ws) {
    __shared__ float red[4];
    const int j = blockIdx.x;
    const int M = tb.M[j], K = tb.K[j];
    const SnWs q = sn_ws(ws, tb.off[j], M, K);
    const int chunks = sn_chunks(M, K);
    float acc = 0.f;
    for (int i = threadIdx.x; i < chunks; i += 256) acc += q.cpart[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) q.c[0] = acc;
}

// ---- projection, stage 3: G = (G - c u[m] v[k]) / sigma ; restore: the parameter's storage gets the master W back
__global__ __launch_bounds__(256) void sn_project_k(SnBatch tb, float* ws, int restore) {
    SN_LOCATE(SN_G_CHUNK);
    const long base = (long)local * SN_CHUNK;
    const int len = (int)min((long)SN_CHUNK, (long)M * K - base);
    float* __restrict__ g = tb.g[j] + base;
    const float* __restrict__ w = tb.w[j] + base;
    float* __restrict__ p = tb.what[j] + base;
    const float* __restrict__ u = tb.u[j];
    const float* __restrict__ v = tb.v[j];
    const float c = q.c[0];
    const float d = sn_divisor(tb.sigma[j][0]);
    for (int i = threadIdx.x; i < len; i += 256) {
        const unsigned e = (unsigned)(base + i);           // M * K < 2^31 (host-checked)
        const unsigned m = e / (unsigned)K, k = e - m * (unsigned)K;
        const float uv = u[m] * v[k];
        g[i] = (g[i] - c * uv) / d;
        if (restore) p[i] = w[i];
    }
}

// Validates the jobs and fills `tb`; returns the floats of workspace the call needs, or < 0.
static long sn_batch(SnBatch& tb, const t2v_sn_job* jobs, int njobs, int need_g, long* grids /*SN_GRIDS*/) {
    if (!jobs || njobs < 1 || njobs > T2V_SN_MAX_JOBS) return T2V_EINVAL;
    long off = 0, blocks[SN_GRIDS] = {0, 0, 0, 0};
    for (int i = 0; i < T2V_SN_MAX_JOBS; ++i) {
        for (int gsh = 0; gsh < SN_GRIDS; ++gsh) tb.begin[gsh][i] = (int)blocks[gsh];
        if (i >= njobs) {
            tb.w[i] = tb.what[i] = tb.u[i] = tb.v[i] = tb.sigma[i] = tb.g[i] = nullptr;
            tb.M[i] = tb.K[i] = tb.off[i] = 0;
            continue;
        }
        const t2v_sn_job& jb = jobs[i];
        if (!jb.w || !jb.what || !jb.u || !jb.v || !jb.sigma || (need_g && !jb.g)) return T2V_EINVAL;
        if (jb.M < 1 || jb.K < 1 || (long)jb.M * jb.K > 0x7fffffffL) return T2V_EINVAL;
        tb.w[i] = jb.w; tb.what[i] = jb.what; tb.u[i] = jb.u; tb.v[i] = jb.v; tb.sigma[i] = jb.sigma; tb.g[i] = jb.g;
        tb.M[i] = jb.M; tb.K[i] = jb.K; tb.off[i] = (int)off;
        off += sn_job_floats(jb.M, jb.K);
        blocks[SN_G_COL] += (long)sn_slices(jb.M) * sn_tiles(jb.K);
        blocks[SN_G_TILE] += sn_tiles(jb.K);
        blocks[SN_G_ROW] += jb.K >= SN_ROW_WG_K ? jb.M : (jb.M + 3) / 4;
        blocks[SN_G_CHUNK] += sn_chunks(jb.M, jb.K);
        if (off > 0x7fffffffL) return T2V_EINVAL;
        for (int gsh = 0; gsh < SN_GRIDS; ++gsh) if (blocks[gsh] > 0x7fffffffL) return T2V_EINVAL;
    }
    for (int gsh = 0; gsh < SN_GRIDS; ++gsh) { tb.begin[gsh][T2V_SN_MAX_JOBS] = (int)blocks[gsh]; grids[gsh] = blocks[gsh]; }
    tb.njobs = njobs;
    return off;
}

extern "C" int64_t t2v_sn_ws_floats(const t2v_sn_job* jobs, int njobs) {
    SnBatch tb;
    long grids[SN_GRIDS];
    return sn_batch(tb, jobs, njobs, 0, grids);
}

extern "C" int t2v_sn_refresh(const t2v_sn_job* jobs, int njobs, float* ws, int64_t ws_floats, int n_iter, float eps, int from_param,
                              void* st) {
    SnBatch tb;
    long grids[SN_GRIDS];
    const long need = sn_batch(tb, jobs, njobs, 0, grids);
    if (need < 0) return (int)need;
    if (!ws || ws_floats < need || n_iter < 1 || !(eps > 0.f)) return T2V_EINVAL;
    for (int it = 0; it < n_iter; ++it) {
        T2V_LAUNCH(sn_col_partial_k, dim3((unsigned)grids[SN_G_COL]), dim3(256), 0, S_(st), tb, ws, from_param);
        T2V_LAUNCH(sn_col_finish_k, dim3((unsigned)grids[SN_G_TILE]), dim3(256), 0, S_(st), tb, ws);
        T2V_LAUNCH(sn_v_k, dim3((unsigned)grids[SN_G_TILE]), dim3(256), 0, S_(st), tb, ws, eps);
        T2V_LAUNCH(sn_row_k, dim3((unsigned)grids[SN_G_ROW]), dim3(256), 0, S_(st), tb, ws, from_param);
        T2V_LAUNCH(sn_u_sigma_k, dim3((unsigned)njobs), dim3(256), 0, S_(st), tb, ws, eps);
    }
    T2V_LAUNCH(sn_scale_k, dim3((unsigned)grids[SN_G_CHUNK]), dim3(256), 0, S_(st), tb, ws, from_param);
    return launch_status();
}

extern "C" int t2v_sn_project(const t2v_sn_job* jobs, int njobs, float* ws, int64_t ws_floats, int restore, void* st) {
    SnBatch tb;
    long grids[SN_GRIDS];
    const long need = sn_batch(tb, jobs, njobs, 1, grids);
    if (need < 0) return (int)need;
    if (!ws || ws_floats < need) return T2V_EINVAL;
    T2V_LAUNCH(sn_dot_partial_k, dim3((unsigned)grids[SN_G_CHUNK]), dim3(256), 0, S_(st), tb, ws);
    T2V_LAUNCH(sn_dot_finish_k, dim3((unsigned)njobs), dim3(256), 0, S_(st), tb, ws);
    T2V_LAUNCH(sn_project_k, dim3((unsigned)grids[SN_G_CHUNK]), dim3(256), 0, S_(st), tb, ws, restore);
    return launch_status();
}
