// match.hip — the contrastive clip-caption matching term of the text-conditioned discriminator (opt-in, Resnet3D(match=True),
// --D_match / --G_match; gfx950). A symmetric, masked InfoNCE loss between the embedded features e = f W [b, J] and
// the sentence codes s [b, J] of one member (include/t2v_hip.h, t2v_match_*):
//   S_ij = <e_i / max(|e_i|, 1e-12), s_j / max(|s_j|, 1e-12)> / tau,   M_ij = (i == j) or (row s_i differs from row s_j in a bit)
//   term = (1 / 2b) sum_i [ -2 S_ii + log sum_j M_ij exp(S_ij) + log sum_j M_ji exp(S_ji) ]
// Forward: ONE workgroup of 1024 threads walks the members in order (b <= 128 rows each; the mean of their terms needs them in one
// place and no atomics are used). The b x b x J product runs on the VALU from J-chunks of the normalised rows staged through
// LDS; every thread keeps a 4 x 4 tile of S in registers (rows ty + 32u, columns tx + 32v), so the row reductions are butterflies
// over the 32 lanes of a row group and the column reductions one cross-lane step plus sixteen per-wave partials summed in wave
// order: a fixed summation order, the same bits run to run. Backward: one workgroup per (member, row).
// fp32, plain vector stores, no atomics, no workspace.
#include <hip/hip_runtime.h>
#include <math.h>
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

#define MATCH_T 1024                      // threads of the forward workgroup: a 32 x 32 grid of 4 x 4 register tiles
#define MATCH_W (MATCH_T / 64)
#define MATCH_B T2V_MATCH_MAX_ROWS        // 128
#define MATCH_JC 32                       // columns of e and s staged per round
#define MATCH_LD (MATCH_B + 1)            // LDS row pitch of the transposed chunks: conflict-free both ways
#define MATCH_EPS 1e-12f

// descriptors travel by value in the kernel arguments
struct MatchBatch { t2v_match_member m[T2V_MAX_GROUPS]; int begin[T2V_MAX_GROUPS + 1]; int n; };

// max / sum over the 32 lanes that share a row (the tx bits of the lane index): every lane ends with the same bits
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(MATCH_T) void match_fwd_k(const MatchBatch tb, int J, float tau, float* __restrict__ stats,
                                                       float* __restrict__ out) {
    __shared__ float eT[MATCH_JC][MATCH_LD], sT[MATCH_JC][MATCH_LD];     // chunk, transposed: [column of the chunk][row]
    __shared__ float part[MATCH_W][MATCH_B];                             // per-wave column partials
    __shared__ float nrm_e[MATCH_B], nrm_s[MATCH_B], diag[MATCH_B], cmax[MATCH_B], csum[MATCH_B], coff[MATCH_B];
    __shared__ float lrow[MATCH_B], lcol[MATCH_B];
    __shared__ uint32_t first[MATCH_B];
    __shared__ int rep[MATCH_B], hit_r[MATCH_B], nmask[MATCH_B];
    __shared__ float terms[T2V_MAX_GROUPS], st0[3];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tx = tid & 31, ty = tid >> 5;
    const float ninf = -INFINITY;

    for (int mi = 0; mi < tb.n; ++mi) {
        const t2v_match_member& q = tb.m[mi];
        const int b = q.b;
        const float* __restrict__ e = q.e;
        const float* __restrict__ s = q.s;
        // ---- row norms: a wave per row, lanes along J
        for (int r = w; r < 2 * b; r += MATCH_W) {
            const float* __restrict__ x = r < b ? e + (long)r * J : s + (long)(r - b) * J;
            float a = 0.f;
            for (int j = lane; j < J; j += 64) a += x[j] * x[j];
            a = sqrtf(wave_sum(a));
            if (lane == 0) {
                if (r < b) {
                    nrm_e[r] = fmaxf(a, MATCH_EPS);                       // the clamped norm itself: the staging divides by it
                    q.norms[r] = a > MATCH_EPS ? 1.f / a : 0.f;          // backward: exactly 0 for a row without a direction
                } else {
                    nrm_s[r - b] = fmaxf(a, MATCH_EPS);
                    q.norms[r] = 1.f / fmaxf(a, MATCH_EPS);
                    first[r - b] = __float_as_uint(x[0]);
                }
            }
        }
        __syncthreads();
        // ---- classes of bitwise identical captions: rep[i] = the first row equal to row i
        if (tid < b) {
            const uint32_t* __restrict__ si = (const uint32_t*)(s + (long)tid * J);
            int r = tid;
            for (int j = 0; j < tid; ++j) {
                if (first[j] != first[tid]) continue;
                const uint32_t* __restrict__ sj = (const uint32_t*)(s + (long)j * J);
                bool same = true;
                for (int c = 1; c < J; ++c)
                    if (si[c] != sj[c]) { same = false; break; }
                if (same) { r = j; break; }
            }
            rep[tid] = r;
        }
        // ---- S = Ehat Shat^T / tau: 4 x 4 tiles in registers
        float acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
        for (int j0 = 0; j0 < J; j0 += MATCH_JC) {
            __syncthreads();
            // (consecutive lanes: consecutive columns of one row). x / max(norm, eps) as the definition has it; the backward
            // rebuilds eh and sh as x * (1 / norm) from the stored reciprocals, which may differ from these in the last bit
            for (int p = tid; p < 2 * b * MATCH_JC; p += MATCH_T) {
                const int c = p & (MATCH_JC - 1), r2 = p / MATCH_JC;
                const int r = r2 < b ? r2 : r2 - b;
                const int j = j0 + c;
                if (r2 < b) eT[c][r] = j < J ? e[(long)r * J + j] / nrm_e[r] : 0.f;
                else sT[c][r] = j < J ? s[(long)r * J + j] / nrm_s[r] : 0.f;
            }
            __syncthreads();
            if (ty < b && tx < b) {
#pragma unroll 4
                for (int c = 0; c < MATCH_JC; ++c) {
                    float a[4], bb[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = ty + 32 * u < b ? eT[c][ty + 32 * u] : 0.f;
#pragma unroll
                    for (int v = 0; v < 4; ++v) bb[v] = tx + 32 * v < b ? sT[c][tx + 32 * v] : 0.f;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * bb[v];
                }
            }
        }
        __syncthreads();
        // ---- S and the mask; entries outside b x b and masked entries are -inf
        bool msk[4][4];                                  // M_ij == 1
        bool dg[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = ty + 32 * u, j = tx + 32 * v;
                const bool in = i < b && j < b;
                dg[u][v] = in && i == j;
                msk[u][v] = in && (i == j || rep[i] != rep[j]);
                acc[u][v] = acc[u][v] / tau;
                if (dg[u][v]) diag[i] = acc[u][v];
            }
        // ---- rows: max, sum, off-diagonal max, masked count (butterflies over tx)
        float rmx[4], rsm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = ty + 32 * u;
            float m = ninf, mo = ninf, cnt = 0.f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (msk[u][v]) m = fmaxf(m, acc[u][v]);
                if (msk[u][v] && !dg[u][v]) mo = fmaxf(mo, acc[u][v]);
                if (!msk[u][v] && i < b && tx + 32 * v < b) cnt += 1.f;
            }
            m = row_max(m);
            mo = row_max(mo);
            cnt = row_sum(cnt);
            float sm = 0.f;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (msk[u][v]) sm += expf(acc[u][v] - m);
            sm = row_sum(sm);
            rmx[u] = m;
            rsm[u] = sm;
            if (tx == 0 && i < b) {
                lrow[i] = sm;                             // (finished below, once diag is visible)
                coff[i] = mo;
                nmask[i] = (int)cnt;
                cmax[i] = m;
            }
        }
        __syncthreads();
        if (tid < b) {
            // L_i = (max_i - S_ii) + log sum_i: exactly 0 when nothing but the diagonal is left
            hit_r[tid] = diag[tid] > coff[tid] ? 1 : 0;
            lrow[tid] = (cmax[tid] - diag[tid]) + logf(lrow[tid]);
        }
        __syncthreads();
        // ---- columns: max
        float cm[4], cmo[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float m = ninf, mo = ninf;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (msk[u][v]) m = fmaxf(m, acc[u][v]);
                if (msk[u][v] && !dg[u][v]) mo = fmaxf(mo, acc[u][v]);
            }
            cm[v] = fmaxf(m, __shfl_xor(m, 32, 64));
            cmo[v] = fmaxf(mo, __shfl_xor(mo, 32, 64));
        }
        if (lane < 32)
#pragma unroll
            for (int v = 0; v < 4; ++v) part[w][tx + 32 * v] = cm[v];
        __syncthreads();
        if (tid < MATCH_B) {
            float m = ninf;
#pragma unroll
            for (int k = 0; k < MATCH_W; ++k) m = fmaxf(m, part[k][tid]);
            cmax[tid] = m;
        }
        __syncthreads();
        if (lane < 32)
#pragma unroll
            for (int v = 0; v < 4; ++v) part[w][tx + 32 * v] = cmo[v];
        __syncthreads();
        if (tid < MATCH_B) {
            float m = ninf;
#pragma unroll
            for (int k = 0; k < MATCH_W; ++k) m = fmaxf(m, part[k][tid]);
            coff[tid] = m;
        }
        __syncthreads();
        // ---- columns: sum
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = tx + 32 * v;
            const float mx = j < b ? cmax[j] : 0.f;
            float sm = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (msk[u][v]) sm += expf(acc[u][v] - mx);
            sm += __shfl_xor(sm, 32, 64);
            if (lane < 32) part[w][j] = sm;
        }
        __syncthreads();
        if (tid < MATCH_B) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < MATCH_W; ++k) t += part[k][tid];
            csum[tid] = t;
            if (tid < b) lcol[tid] = (cmax[tid] - diag[tid]) + logf(t);
        }
        __syncthreads();
        // ---- the coefficients of the backward: C = (P_row + P_col - 2 I) / (2 b tau), masked
        const float scale = 1.f / (2.f * (float)b * tau);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = ty + 32 * u, j = tx + 32 * v;
                if (i < b && j < b) {
                    float c = 0.f;
                    if (msk[u][v]) {
                        const float pr = expf(acc[u][v] - rmx[u]) / rsm[u];
                        const float pc = expf(acc[u][v] - cmax[j]) / csum[j];
                        c = ((pr + pc) - (dg[u][v] ? 2.f : 0.f)) * scale;
                    }
                    q.coef[(long)i * b + j] = c;
                }
            }
        if (tid == 0) {
            float t = 0.f;
            int hr = 0, hc = 0, nm = 0;
            for (int i = 0; i < b; ++i) {
                t += lrow[i] + lcol[i];
                hr += hit_r[i];
                hc += diag[i] > coff[i] ? 1 : 0;
                nm += nmask[i];
            }
            terms[mi] = t / (2.f * (float)b);
            if (mi == 0) {
                st0[0] = (float)hr / (float)b;
                st0[1] = (float)hc / (float)b;
                st0[2] = (float)nm;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        float t = 0.f;
        for (int mi = 0; mi < tb.n; ++mi) t += terms[mi];
        t /= (float)tb.n;
        *out = t;
        stats[0] = t;
        stats[1] = st0[0];
        stats[2] = st0[1];
        stats[3] = st0[2];
    }
}

// backward: dE_i = (dEh_i - eh_i <eh_i, dEh_i>) / |e_i| with dEh_i = g scale sum_k C_ik sh_k (scale: the member's weight in out). One workgroup per (member, row), threads
// along J (up to 4 columns each); the row's dot product through a wave reduction and four waves in order.
#define MATCH_BT 256
__global__ __launch_bounds__(MATCH_BT) void match_bwd_k(const MatchBatch tb, int J, float scale, const float* __restrict__ g) {
    __shared__ float cs[MATCH_B];
    __shared__ float red[MATCH_BT / 64];
    int mi = 0;
    while (mi + 1 < tb.n && (int)blockIdx.x >= tb.begin[mi + 1]) ++mi;
    const t2v_match_member& q = tb.m[mi];
    const int b = q.b, i = blockIdx.x - tb.begin[mi];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < b) cs[tid] = q.coef[(long)i * b + tid] * q.norms[b + tid];
    __syncthreads();
    const float ie = q.norms[i], gg = *g * scale;
    const float* __restrict__ s = q.s;
    float d[4], eh[4];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = tid + MATCH_BT * c;
        d[c] = eh[c] = 0.f;
        if (j < J) {
            float a = 0.f;
            for (int k = 0; k < b; ++k) a += cs[k] * s[(long)k * J + j];
            d[c] = gg * a;
            eh[c] = q.e[(long)i * J + j] * ie;
            dot += eh[c] * d[c];
        }
    }
    dot = wave_sum(dot);
    if (lane == 0) red[w] = dot;
    __syncthreads();
    dot = (red[0] + red[1]) + (red[2] + red[3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = tid + MATCH_BT * c;
        if (j < J) q.de[(long)i * J + j] = ie > 0.f ? (d[c] - eh[c] * dot) * ie : 0.f;
    }
}

// every refusal of the family, before any launch; fills the by-value table
static bool match_table(bool bwd, const t2v_match_member* members, int n, int J, MatchBatch& tb) {
    if (!members || n < 1 || n > T2V_MAX_GROUPS || J < 1 || J > T2V_MATCH_MAX_COLS) return false;
    int rows = 0;
    for (int i = 0; i < n; ++i) {
        const t2v_match_member& q = members[i];
        if (q.b < 1 || q.b > T2V_MATCH_MAX_ROWS) return false;
        if (!q.e || !q.s || !q.coef || !q.norms || (bwd && !q.de)) return false;
        tb.m[i] = q;
        tb.begin[i] = rows;
        rows += q.b;
    }
    tb.begin[n] = rows;
    tb.n = n;
    return true;
}

extern "C" int t2v_match_fwd(const t2v_match_member* members, int n, int J, float tau, float* stats, float* out, void* st) {
    MatchBatch tb;
    if (!stats || !out || !(tau > 0.f) || !(tau < INFINITY)) return T2V_EINVAL;
    if (!match_table(false, members, n, J, tb)) return T2V_EINVAL;
    T2V_LAUNCH(match_fwd_k, dim3(1), dim3(MATCH_T), 0, S_(st), tb, J, tau, stats, out);
    return launch_status();
}

extern "C" int t2v_match_bwd(const t2v_match_member* members, int n, int J, float scale, const float* g, void* st) {
    MatchBatch tb;
    if (!g || !(scale > 0.f) || !(scale <= 1.f)) return T2V_EINVAL;
    if (!match_table(true, members, n, J, tb)) return T2V_EINVAL;
    T2V_LAUNCH(match_bwd_k, dim3(tb.begin[n]), dim3(MATCH_BT), 0, S_(st), tb, J, scale, g);
    return launch_status();
}
