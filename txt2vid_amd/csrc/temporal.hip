// temporal.hip — the TGAN-v1 frame-seed generator that MultiScaleGen(no_lstm=True) puts in place of the ConvLSTM
// (txt2vid/models/tgan/temporal_gen.py:10-34): dc0 = ConvTranspose1d(fm, 512, 1), dc1..dc4 = ConvTranspose1d(k=4, s=2, p=1),
// BatchNorm1d + ReLU after dc0..dc3, tanh after dc4. Activations are [B, C, L]; weights are torch's [Cin, Cout, k].
//
// The whole generator is well under a GFLOP at B = 32, so the design is for launch count:
//  * forward, one launch per layer. A dc0..dc3 launch gives each workgroup ONE output channel over the whole batch, so the
//    workgroup holds every value that channel's BatchNorm sees: its epilogue computes the exact batch mean / M2 (two passes
//    over its own outputs, no atomics, no accumulator to zero), updates the running buffers and publishes the per-channel
//    (scale, shift) the NEXT launch applies — with the ReLU — while it loads its operand. dc4 fuses the tanh and writes
//    the contiguous [B, fm, 16] buffer that is, reinterpreted, the [B*16, 1024, h, w] merged-frames tensor.
//  * backward, one launch per layer, two workgroup roles: data-gradient workgroups own a block of input channels over the
//    whole batch, so the BatchNorm adjoint of the layer in front (its sum(dy) / sum(dy * xhat) reductions) finishes in
//    the same workgroup; weight-gradient workgroups own a (Cout x Cin) tile and sum over the batch in registers (no split,
//    no partial slabs). The tanh adjoint is applied on load.
// fp32 VALU throughout (the bf16-compute switch does not reach these kernels).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/t2v_hip.h"

#define T2V_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define S_(stream) ((hipStream_t)(stream))

static inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2V_OK : -(int)e - 1000;
}

__device__ __forceinline__ float tw_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// N sums over a 256-thread workgroup; every thread gets the results. red: 4*N floats.
template <int N>
__device__ __forceinline__ void tblock_sum(float* v, float* red) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = tw_sum(v[j]);
    __syncthreads();                                     // (red may still be read by a previous call)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) red[(threadIdx.x >> 6) * N + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = red[j] + red[N + j] + red[2 * N + j] + red[3 * N + j];
}

// ---------------------------------------------------------------------------------------------------------------------
// forward of dc0..dc3 (+ the statistics of the BatchNorm behind it). grid = Cout, block = 256: groups of G lanes share one
// output (b, o) and split its sum over Cin. K = 1 (dc0, LIN = 1) or 4 (stride 2, pad 1: o = 2i - 1 + t).
// x: [B, Cin, LIN] raw; ss_in: (scale[Cin], shift[Cin]) of the BatchNorm in front (null for dc0); y: [B, Cout, LOUT] raw.
// st: [mean | 1/std | scale | shift] x Cout (training); eval mode writes only scale / shift, from the running buffers.
template <int K, int LIN>
__global__ __launch_bounds__(256) void tseed_fwd_bn_k(const float* __restrict__ x, const float* __restrict__ ss_in,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ y, float* __restrict__ st, float* rm, float* rv,
                                                      long long* counter, int B, int Cin, int Cout, int G, float momentum, float eps,
                                                      int training) {
    constexpr int LOUT = K == 4 ? 2 * LIN : LIN;
    extern __shared__ float wcol[];                       // w[:, co, :]: Cin * K floats
    __shared__ float red[8];
    const int co = blockIdx.x;
    for (int j = threadIdx.x; j < Cin * K; j += 256) {
        const int ci = j / K, t = j - ci * K;
        wcol[j] = w[((long)ci * Cout + co) * K + t];
    }
    __syncthreads();
    const int gi = threadIdx.x / G, gl = threadIdx.x - gi * G, ngroups = 256 / G;
    const int n_out = B * LOUT;
    const float bco = bias[co];
    float lsum = 0.f;
    for (int idx = gi; idx < n_out; idx += ngroups) {       // (all G lanes of a group run the same trip count)
        const int b = idx / LOUT, o = idx - b * LOUT;
        const float* xb = x + (long)b * Cin * LIN;
        float acc = 0.f;
        for (int ci = gl; ci < Cin; ci += G) {
            float sc = 1.f, sh = 0.f;
            if (ss_in) { sc = ss_in[ci]; sh = ss_in[Cin + ci]; }
            const float* xr = xb + (long)ci * LIN;
            auto ld = [&](int i) { const float v = xr[i]; return ss_in ? fmaxf(fmaf(v, sc, sh), 0.f) : v; };
            const float* wc = wcol + ci * K;
            if (K == 1) {
                acc = fmaf(ld(0), wc[0], acc);
            } else {
                const int m = o >> 1;
                if ((o & 1) == 0) {                          // o = 2m: tap 1 at i = m, tap 3 at i = m - 1
                    acc = fmaf(ld(m), wc[1], acc);
                    if (m >= 1) acc = fmaf(ld(m - 1), wc[3], acc);
                } else {                                     // o = 2m + 1: tap 0 at i = m + 1, tap 2 at i = m
                    if (m + 1 < LIN) acc = fmaf(ld(m + 1), wc[0], acc);
                    acc = fmaf(ld(m), wc[2], acc);
                }
            }
        }
        for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (gl == 0) {
            const float v = acc + bco;
            y[((long)b * Cout + co) * LOUT + o] = v;
            lsum += v;
        }
    }
    if (!training) {
        if (threadIdx.x == 0) {
            const float sc = gamma[co] / sqrtf(rv[co] + eps);
            st[2 * Cout + co] = sc;
            st[3 * Cout + co] = beta[co] - rm[co] * sc;
        }
        return;
    }
    const float n = (float)n_out;
    float s[1] = {lsum};
    tblock_sum<1>(s, red);
    const float mean = s[0] / n;
    float lm2 = 0.f;
    if (gl == 0) {
        for (int idx = gi; idx < n_out; idx += ngroups) {   // this thread's own outputs, written above
            const int b = idx / LOUT, o = idx - b * LOUT;
            const float d = y[((long)b * Cout + co) * LOUT + o] - mean;
            lm2 = fmaf(d, d, lm2);
        }
    }
    s[0] = lm2;
    tblock_sum<1>(s, red);
    if (threadIdx.x == 0) {
        const float m2 = s[0];
        const float var = m2 / n, istd = 1.f / sqrtf(var + eps);
        const float sc = gamma[co] * istd;
        st[co] = mean;
        st[Cout + co] = istd;
        st[2 * Cout + co] = sc;
        st[3 * Cout + co] = beta[co] - mean * sc;
        const float unb = n > 1.f ? m2 / (n - 1.f) : var;
        rm[co] = (1.f - momentum) * rm[co] + momentum * mean;
        rv[co] = (1.f - momentum) * rv[co] + momentum * unb;
        if (counter && co == 0) *counter += 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward of dc4 + tanh: grid (ceil(Cout / 256), B), one output channel (all 16 frames) per thread. The sample's input
// h = relu(bn3(x)) is staged in LDS once; each weight float4 w[ci, co, 0..3] feeds 4 * LIN FMAs.
template <int LIN>
__global__ __launch_bounds__(256) void tseed_fwd_tanh_k(const float* __restrict__ x, const float* __restrict__ ss_in,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ z, int Cin, int Cout) {
    constexpr int LOUT = 2 * LIN;
    extern __shared__ float h[];                           // Cin * LIN
    const int b = blockIdx.y;
    const float* xb = x + (long)b * Cin * LIN;
    for (int j = threadIdx.x; j < Cin * LIN; j += 256) {
        const int ci = j / LIN;
        h[j] = fmaxf(fmaf(xb[j], ss_in[ci], ss_in[Cin + ci]), 0.f);
    }
    __syncthreads();
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Cout) return;
    float acc[LOUT];
    const float bco = bias[co];
#pragma unroll
    for (int o = 0; o < LOUT; ++o) acc[o] = bco;
    for (int ci = 0; ci < Cin; ++ci) {
        const float4 wv = *reinterpret_cast<const float4*>(w + ((long)ci * Cout + co) * 4);
        const float* hc = h + ci * LIN;
#pragma unroll
        for (int i = 0; i < LIN; ++i) {                    // input position i reaches o = 2i - 1 + t
            const float hv = hc[i];
            if (i >= 1) acc[2 * i - 1] = fmaf(hv, wv.x, acc[2 * i - 1]);
            acc[2 * i] = fmaf(hv, wv.y, acc[2 * i]);
            acc[2 * i + 1] = fmaf(hv, wv.z, acc[2 * i + 1]);
            if (2 * i + 2 < LOUT) acc[2 * i + 2] = fmaf(hv, wv.w, acc[2 * i + 2]);
        }
    }
    float4* zo = reinterpret_cast<float4*>(z + ((long)b * Cout + co) * LOUT);
#pragma unroll
    for (int q = 0; q < LOUT / 4; ++q)
        zo[q] = make_float4(tanhf(acc[4 * q]), tanhf(acc[4 * q + 1]), tanhf(acc[4 * q + 2]), tanhf(acc[4 * q + 3]));
}

// ---------------------------------------------------------------------------------------------------------------------
// backward of one layer. g: dL/d(raw output) [B, Cout, LOUT] — or dL/dz of dc4 with z (TANH: g * (1 - z^2) on load).
// Workgroups [0, nd): data gradient. Each owns CIB input channels; rows of S lanes take one sample each, the S lanes split
// the sum over Cout and meet in a shuffle. With a BatchNorm in front (st_in != null) the workgroup then has every dL/dh of
// its channels and finishes that BatchNorm's adjoint (ReLU mask, sum(dy), sum(dy * xhat)) in place: gin = dL/d(raw input).
// Workgroups [nd, ...): weight gradient. 64 output channels x (4 waves x CIPT input channels); each thread sums its
// (ci, co, 0..K-1) over the batch in registers; the first ci tile also sums the bias gradient.
#define TSEED_TANH 1
#define TSEED_ACC_W 2
#define TSEED_ACC_B 4
#define TSEED_ACC_GAMMA 8
#define TSEED_ACC_BETA 16

__device__ __forceinline__ void tstore(float* p, float v, bool acc) { *p = acc ? *p + v : v; }

template <int K, int LIN>
__global__ __launch_bounds__(256) void tseed_bwd_k(const float* __restrict__ g, const float* __restrict__ z,
                                                   const float* __restrict__ w, const float* __restrict__ a_in,
                                                   const float* __restrict__ st_in, float* __restrict__ gin, float* __restrict__ dw,
                                                   float* __restrict__ db, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                   int B, int Cin, int Cout, int flags, int nd, int S) {
    constexpr int LOUT = K == 4 ? 2 * LIN : LIN;
    constexpr int CIB = LIN == 1 ? 8 : (LIN == 8 ? 2 : 32 / LIN);     // data gradient: input channels per workgroup
    constexpr int CIPT = 16 / K;                           // weight gradient: CIPT * K accumulators per thread
    const bool tanh_in = flags & TSEED_TANH;
    if ((int)blockIdx.x < nd) {
        __shared__ float red[4 * 2 * CIB];
        const int ci0 = blockIdx.x * CIB;
        const int R = 256 / S, row = threadIdx.x / S, sl = threadIdx.x - row * S;
        float lsg[CIB], lsgx[CIB];
#pragma unroll
        for (int c = 0; c < CIB; ++c) lsg[c] = lsgx[c] = 0.f;
        for (int b = row; b < B; b += R) {                  // (all S lanes of a row run the same trip count)
            float acc[CIB][LIN];
#pragma unroll
            for (int c = 0; c < CIB; ++c)
#pragma unroll
                for (int i = 0; i < LIN; ++i) acc[c][i] = 0.f;
#pragma unroll 2
            for (int co = sl; co < Cout; co += S) {          // (two iterations' loads in flight: the loop is latency-bound)
                const long go = ((long)b * Cout + co) * LOUT;
                float gv[LOUT];
#pragma unroll
                for (int o = 0; o < LOUT; ++o) {
                    gv[o] = g[go + o];
                    if (tanh_in) { const float zz = z[go + o]; gv[o] *= 1.f - zz * zz; }
                }
#pragma unroll
                for (int c = 0; c < CIB; ++c) {
                    const int ci = ci0 + c;
                    if (ci >= Cin) break;
                    const float* wp = w + ((long)ci * Cout + co) * K;
                    if (K == 1) {
                        acc[c][0] = fmaf(wp[0], gv[0], acc[c][0]);
                    } else {
                        const float4 wv = *reinterpret_cast<const float4*>(wp);
#pragma unroll
                        for (int i = 0; i < LIN; ++i) {     // dL/dx[i] = sum_t w[t] g[2i - 1 + t]
                            float s = acc[c][i];
                            if (i >= 1) s = fmaf(wv.x, gv[2 * i - 1], s);
                            s = fmaf(wv.y, gv[2 * i], s);
                            s = fmaf(wv.z, gv[2 * i + 1], s);
                            if (2 * i + 2 < LOUT) s = fmaf(wv.w, gv[2 * i + 2], s);
                            acc[c][i] = s;
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CIB; ++c)
#pragma unroll
                for (int i = 0; i < LIN; ++i)
                    for (int off = S >> 1; off > 0; off >>= 1) acc[c][i] += __shfl_xor(acc[c][i], off, 64);
            if (sl == 0) {
#pragma unroll
                for (int c = 0; c < CIB; ++c) {
                    const int ci = ci0 + c;
                    if (ci >= Cin) break;
#pragma unroll
                    for (int i = 0; i < LIN; ++i) {
                        const long idx = ((long)b * Cin + ci) * LIN + i;
                        float v = acc[c][i];
                        if (st_in) {
                            const float a = a_in[idx];
                            if (fmaf(a, st_in[2 * Cin + ci], st_in[3 * Cin + ci]) <= 0.f) v = 0.f;     // ReLU mask
                            const float xhat = (a - st_in[ci]) * st_in[Cin + ci];
                            lsg[c] += v;
                            lsgx[c] = fmaf(v, xhat, lsgx[c]);
                        }
                        gin[idx] = v;
                    }
                }
            }
        }
        if (!st_in) return;                                 // (uniform over the workgroup)
        float sums[2 * CIB];
#pragma unroll
        for (int c = 0; c < CIB; ++c) { sums[c] = lsg[c]; sums[CIB + c] = lsgx[c]; }
        tblock_sum<2 * CIB>(sums, red);
        const float inv_n = 1.f / (float)(B * LIN);
        if (sl == 0) {
            for (int b = row; b < B; b += R) {
#pragma unroll
                for (int c = 0; c < CIB; ++c) {
                    const int ci = ci0 + c;
                    if (ci >= Cin) break;
                    const float mg = sums[c] * inv_n, mgx = sums[CIB + c] * inv_n;
                    const float mean = st_in[ci], istd = st_in[Cin + ci], sc = st_in[2 * Cin + ci];
#pragma unroll
                    for (int i = 0; i < LIN; ++i) {
                        const long idx = ((long)b * Cin + ci) * LIN + i;
                        const float xhat = (a_in[idx] - mean) * istd;
                        gin[idx] = sc * (gin[idx] - mg - xhat * mgx);
                    }
                }
            }
        }
        if (threadIdx.x < CIB && ci0 + (int)threadIdx.x < Cin) {
            const int c = threadIdx.x;
            tstore(dbeta + ci0 + c, sums[c], flags & TSEED_ACC_BETA);
            tstore(dgamma + ci0 + c, sums[CIB + c], flags & TSEED_ACC_GAMMA);
        }
        return;
    }
    // ---- weight gradient
    const int wb = blockIdx.x - nd;
    const int nct = (Cout + 63) / 64;
    const int ct = wb % nct, cit = wb / nct;
    const int co = ct * 64 + (threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cib = cit * 4 * CIPT + wave * CIPT;
    if (co >= Cout) return;
    const bool want_db = cit == 0 && wave == 0;
    float acc[CIPT][K];
#pragma unroll
    for (int c = 0; c < CIPT; ++c)
#pragma unroll
        for (int t = 0; t < K; ++t) acc[c][t] = 0.f;
    float dbacc = 0.f;
#pragma unroll 2
    for (int b = 0; b < B; ++b) {
        const long go = ((long)b * Cout + co) * LOUT;
        float gv[LOUT];
#pragma unroll
        for (int o = 0; o < LOUT; ++o) {
            gv[o] = g[go + o];
            if (tanh_in) { const float zz = z[go + o]; gv[o] *= 1.f - zz * zz; }
            dbacc += gv[o];
        }
#pragma unroll
        for (int c = 0; c < CIPT; ++c) {
            const int ci = cib + c;
            if (ci >= Cin) break;
            const float* ar = a_in + ((long)b * Cin + ci) * LIN;
            float sc = 1.f, sh = 0.f;
            if (st_in) { sc = st_in[2 * Cin + ci]; sh = st_in[3 * Cin + ci]; }
#pragma unroll
            for (int i = 0; i < LIN; ++i) {
                const float hv = st_in ? fmaxf(fmaf(ar[i], sc, sh), 0.f) : ar[i];
                if (K == 1) {
                    acc[c][0] = fmaf(hv, gv[0], acc[c][0]);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int o = 2 * i - 1 + t;
                        if (o >= 0 && o < LOUT) acc[c][t] = fmaf(hv, gv[o], acc[c][t]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CIPT; ++c) {
        const int ci = cib + c;
        if (ci >= Cin) break;
#pragma unroll
        for (int t = 0; t < K; ++t) tstore(dw + ((long)ci * Cout + co) * K + t, acc[c][t], flags & TSEED_ACC_W);
    }
    if (want_db) tstore(db + co, dbacc, flags & TSEED_ACC_B);
}

// ---------------------------------------------------------------------------------------------------------------------
static bool tseed_shape_ok(int K, int Lin) {
    return (K == 1 && Lin == 1) || (K == 4 && (Lin == 1 || Lin == 2 || Lin == 4 || Lin == 8));
}

extern "C" int t2v_tseed_fwd_bn(const float* x, const float* ss_in, const float* w, const float* bias, const float* gamma,
                                const float* beta, float* y, float* st, float* running_mean, float* running_var,
                                int64_t* batches_tracked, int B, int Cin, int Cout, int Lin, int K, float momentum, float eps,
                                int training, void* stream) {
    if (!x || !w || !bias || !gamma || !beta || !y || !st || !running_mean || !running_var) return T2V_EINVAL;
    if (B < 1 || Cin < 1 || Cout < 1 || !tseed_shape_ok(K, Lin)) return T2V_EINVAL;
    if ((long)Cin * K > 16384) return T2V_EINVAL;                  // the staged weight column: at most 64 KB of LDS
    const int n_out = B * (K == 4 ? 2 * Lin : Lin);
    int G = 1;
    while (G < 64 && (long)n_out * G < 256) G <<= 1;
    const size_t lds = (size_t)Cin * K * sizeof(float);
    long long* cnt = (long long*)batches_tracked;
#define FWD_BN(KK, LL) T2V_LAUNCH((tseed_fwd_bn_k<KK, LL>), dim3(Cout), dim3(256), lds, S_(stream), x, ss_in, w, bias, gamma, beta, y, \
                                  st, running_mean, running_var, cnt, B, Cin, Cout, G, momentum, eps, training)
    if (K == 1) FWD_BN(1, 1);
    else if (Lin == 1) FWD_BN(4, 1);
    else if (Lin == 2) FWD_BN(4, 2);
    else if (Lin == 4) FWD_BN(4, 4);
    else FWD_BN(4, 8);
#undef FWD_BN
    return launch_status();
}

extern "C" int t2v_tseed_fwd_tanh(const float* x, const float* ss_in, const float* w, const float* bias, float* z, int B, int Cin,
                                  int Cout, int Lin, void* stream) {
    if (!x || !ss_in || !w || !bias || !z || B < 1 || Cin < 1 || Cout < 1 || Lin != 8) return T2V_EINVAL;
    if ((long)Cin * Lin > 16384) return T2V_EINVAL;
    T2V_LAUNCH(tseed_fwd_tanh_k<8>, dim3((Cout + 255) / 256, B), dim3(256), (size_t)Cin * Lin * sizeof(float), S_(stream), x, ss_in, w,
               bias, z, Cin, Cout);
    return launch_status();
}

extern "C" int t2v_tseed_bwd(const float* g, const float* z, const float* w, const float* a_in, const float* st_in, float* gin,
                             float* dw, float* db, float* dgamma, float* dbeta, int B, int Cin, int Cout, int Lin, int K, int flags,
                             void* stream) {
    if (!g || !w || !a_in || !dw || !db || B < 1 || Cin < 1 || Cout < 1 || !tseed_shape_ok(K, Lin)) return T2V_EINVAL;
    if ((flags & TSEED_TANH) && !z) return T2V_EINVAL;
    if (st_in && gin && (!dgamma || !dbeta)) return T2V_EINVAL;
    const int cib = Lin == 1 ? 8 : (Lin == 8 ? 2 : 32 / Lin), ci_tile = 4 * (16 / K);     // (= the kernel's CIB)
    const int nd = gin ? (Cin + cib - 1) / cib : 0;
    const int nw = ((Cout + 63) / 64) * ((Cin + ci_tile - 1) / ci_tile);
    int R = 4;                                                      // samples in flight per data-gradient workgroup
    while (R < 64 && R < B) R <<= 1;
    const int S = 256 / R;
#define BWD(KK, LL) T2V_LAUNCH((tseed_bwd_k<KK, LL>), dim3(nd + nw), dim3(256), 0, S_(stream), g, z, w, a_in, st_in, gin, dw, db, \
                               dgamma, dbeta, B, Cin, Cout, flags, nd, S)
    if (K == 1) BWD(1, 1);
    else if (Lin == 1) BWD(4, 1);
    else if (Lin == 2) BWD(4, 2);
    else if (Lin == 4) BWD(4, 4);
    else BWD(4, 8);
#undef BWD
    return launch_status();
}
