// Input row of the hot path: synthetic Moving-MNIST-shaped clips + captions generated straight in HBM.
//
// txt2vid/data/synthetic/generate.py:18-47,136-170 draws one 28x28 blob, a digit label, one of four bounce motions and a fixed
// coordinate per clip, then translates the blob linearly between two edge points and back. The host-side dataset of this build
// (`txt2vid_amd.data.SyntheticMovingDigits`) takes those draws from numpy's legacy RandomState seeded per (seed, index); this
// kernel reproduces that generator bit for bit — MT19937 seeding / twist / tempering, numpy's 53-bit `random_sample`, its
// masked-rejection `randint` — so that a clip generated on the GPU equals the host clip exactly (integer / geometry work; the one
// floating-point step, -1 + 2u in double rounded to float, is the same IEEE operation on both sides).
//
// One workgroup per clip: thread 0 seeds the 624-word state (a serial recurrence), the twist runs in parallel in its four
// dependency phases, every thread tempers and converts, then all 256 lanes write the T x C x S x S frames with 16-byte stores
// (HBM-write bound: 4 bytes per output element, nothing is read).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t2v_hip.h"

namespace {

constexpr int MT_N = 624, MT_M = 397, MT_BLOCKS = 4, BLOB = 28;

struct SynthVocab { int32_t id[T2V_SYNTH_VOCAB]; };

__device__ inline uint32_t mt_mix(uint32_t cur, uint32_t next, uint32_t far_) {
    const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
    return far_ ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__global__ __launch_bounds__(256) void synth_clips_k(const int64_t* __restrict__ index, int64_t seed, int T, int C, int S, SynthVocab voc,
                                                     float* __restrict__ vids, int64_t* __restrict__ tokens, int32_t* __restrict__ err) {
    __shared__ uint32_t mt[MT_N];
    __shared__ uint32_t draws[MT_BLOCKS * MT_N];
    __shared__ float blob[BLOB * BLOB];
    __shared__ int32_t meta[4];                       // digit, motion, fixed coordinate
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {                                   // numpy `_legacy_seeding(int)` == init_genrand
        uint32_t s = (uint32_t)(((uint64_t)seed * 1000003ull + (uint64_t)index[b]) & 0x7FFFFFFFull);
        for (int k = 0; k < MT_N; ++k) {
            mt[k] = s;
            s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)k + 1u;
        }
    }
    __syncthreads();
    for (int blk = 0; blk < MT_BLOCKS; ++blk) {
        // the twist's four dependency phases; inside a phase every element reads values no lane of the phase writes except its
        // own slot and its right neighbour's OLD value: read into registers, barrier, write
        uint32_t v = 0;
        if (tid < MT_N - MT_M) v = mt_mix(mt[tid], mt[tid + 1], mt[tid + MT_M]);                           // [0, 227)
        __syncthreads();
        if (tid < MT_N - MT_M) mt[tid] = v;
        __syncthreads();
        const int i2 = (MT_N - MT_M) + tid;                                                              // [227, 454)
        if (tid < MT_N - MT_M) v = mt_mix(mt[i2], mt[i2 + 1], mt[i2 - (MT_N - MT_M)]);
        __syncthreads();
        if (tid < MT_N - MT_M) mt[i2] = v;
        __syncthreads();
        const int i3 = 2 * (MT_N - MT_M) + tid;                                                          // [454, 623)
        if (i3 < MT_N - 1) v = mt_mix(mt[i3], mt[i3 + 1], mt[i3 - (MT_N - MT_M)]);
        __syncthreads();
        if (i3 < MT_N - 1) mt[i3] = v;
        __syncthreads();
        if (tid == 0) mt[MT_N - 1] = mt_mix(mt[MT_N - 1], mt[0], mt[MT_M - 1]);
        __syncthreads();
        for (int k = tid; k < MT_N; k += 256) {
            uint32_t y = mt[k];
            y ^= y >> 11;
            y ^= (y << 7) & 0x9d2c5680u;
            y ^= (y << 15) & 0xefc60000u;
            y ^= y >> 18;
            draws[blk * MT_N + k] = y;
        }
        __syncthreads();
    }
    // rs.uniform(-1, 1, (28, 28)).astype(float32): lower + range * random_sample(), random_sample = (a >> 5, b >> 6) / 2^53
    for (int e = tid; e < BLOB * BLOB; e += 256) {
        const double a = (double)(draws[2 * e] >> 5), c = (double)(draws[2 * e + 1] >> 6);
        const double u = (a * 67108864.0 + c) / 9007199254740992.0;
        blob[e] = (float)(-1.0 + 2.0 * u);
    }
    if (tid == 0) {                                   // rs.randint(10), rs.randint(4), rs.randint(S - 28 + 1): masked rejection on 32-bit draws
        int pos = 2 * BLOB * BLOB;
        const uint32_t rngs[3] = {9u, 3u, (uint32_t)(S - BLOB)};
        bool bad = false;
        for (int r = 0; r < 3; ++r) {
            uint32_t val = 0;
            if (rngs[r] != 0) {
                uint32_t mask = rngs[r];
                mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
                for (;;) {
                    if (pos >= MT_BLOCKS * MT_N) { bad = true; val = 0; break; }     // (> 900 rejections in a row: never; flagged, not hidden)
                    val = draws[pos++] & mask;
                    if (val <= rngs[r]) break;
                }
            }
            meta[r] = (int32_t)val;
        }
        if (bad && err) *err = 1;
        // caption: <start> digit N is A and B <end>   (MOTIONS: left-right, right-left, top-bottom, bottom-top)
        const int mot = meta[1];
        const int a_ = mot == 0 ? 13 : mot == 1 ? 15 : mot == 2 ? 16 : 17;
        const int b_ = mot == 0 ? 15 : mot == 1 ? 13 : mot == 2 ? 17 : 16;
        int64_t* tk = tokens + (int64_t)b * 8;
        tk[0] = voc.id[0]; tk[1] = voc.id[1]; tk[2] = voc.id[2 + meta[0]]; tk[3] = voc.id[12];
        tk[4] = voc.id[a_]; tk[5] = voc.id[14]; tk[6] = voc.id[b_]; tk[7] = voc.id[18];
    }
    __syncthreads();
    const int mot = meta[1], fixed = meta[2], lim = S - BLOB;
    const int64_t frame = (int64_t)S * S;
    float* out = vids + (int64_t)b * T * C * frame;
    const int rowq = S / 4;                            // S % 4 == 0 (host-checked): a float4 never straddles a row
    const int64_t nq = (int64_t)T * C * frame / 4;
    for (int64_t q = tid; q < nq; q += 256) {
        const int x0 = (int)(q % rowq) * 4;
        const int64_t r = q / rowq;
        const int y = (int)(r % S);
        const int t = (int)(r / ((int64_t)S * C));
        // pos = int(round((ph if ph <= 1 else 2 - ph) * lim)), ph = t / float(T - 1) * 2.0 — Python doubles, round half to even
        const double ph = (double)t / (double)(T - 1) * 2.0;
        int p = (int)rint((ph <= 1.0 ? ph : 2.0 - ph) * (double)lim);
        if (mot == 1 || mot == 3) p = lim - p;
        const int by = mot < 2 ? fixed : p, bx = mot < 2 ? p : fixed;
        float4 v4;
        float* pv = reinterpret_cast<float*>(&v4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            const bool in = y >= by && y < by + BLOB && x >= bx && x < bx + BLOB;
            pv[j] = in ? blob[(y - by) * BLOB + (x - bx)] : -1.0f;
        }
        reinterpret_cast<float4*>(out)[q] = v4;
    }
}

// Real-data twin of synth_clips_k: batch rows gathered from an HBM-resident uint8 frame cache (one [C,H,W] row of N bytes per
// decoded frame, rows back to back) and converted through a 256-entry table the host computed with default_transform's own
// float32 expression, so out == the host item bit for bit. One lane per 16 source bytes: a 16-byte load, 16 LDS look-ups, four
// 16-byte stores. A row of the cache starts at base + row * N, which is 16-byte aligned only when N is: unit 0 of a row is its
// scalar head (the bytes in front of the first aligned address), units 1..nbody the aligned body, the next one the scalar tail.
// Streaming, HBM bound: 1 byte read + 4 bytes written per sample.
__global__ __launch_bounds__(256) void clip_gather_k(const uint8_t* __restrict__ cache, int64_t n_rows, const int64_t* __restrict__ row_index,
                                                     int64_t n_slots, int64_t N, int upr, const float* __restrict__ lut,
                                                     float* __restrict__ out, int32_t* __restrict__ err) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = u / upr;
    if (slot >= n_slots) return;
    const int c = (int)(u - slot * upr);
    int64_t row = row_index[slot];
    if (row < 0 || row >= n_rows) {                   // never dereferenced: clamped and flagged (the loader raises at its next check)
        row = row < 0 ? 0 : n_rows - 1;
        if (c == 0 && err) *err = 1;
    }
    const uint8_t* src = cache + row * N;
    float* dst = out + slot * N;
    int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)src & 15u)) & 15u);
    if (head > N) head = N;
    const int64_t nbody = (N - head) / 16;
    if (c >= 1 && c <= nbody) {
        const int64_t off = head + (int64_t)(c - 1) * 16;
        const uint4 q = *reinterpret_cast<const uint4*>(src + off);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = s_lut[(w[j >> 2] >> (8 * (j & 3))) & 0xffu];
        float* o = dst + off;
        if (((uintptr_t)o & 15u) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) reinterpret_cast<float4*>(o)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
        } else {                                      // (N not a multiple of 4: the output row is not float4 aligned)
#pragma unroll
            for (int j = 0; j < 16; ++j) o[j] = v[j];
        }
        return;
    }
    int64_t lo, hi;
    if (c == 0) { lo = 0; hi = head; }
    else if (c == nbody + 1) { lo = head + nbody * 16; hi = N; }
    else return;
    for (int64_t e = lo; e < hi; ++e) dst[e] = s_lut[src[e]];
}

// clip_gather_k with a per-clip window and direction: out[b,t,c,y,x] = lut[frame(row)[c, y0 + y, x0 + (flip ? W-1-x : x)]], the
// stored frame being C x Hc x Wc bytes. One workgroup row per output frame (blockIdx.x = slot, so row, window and every clamp are
// uniform), one lane per 16 consecutive output floats, cut at 16-byte boundaries of the OUTPUT (a slot starts `mis` floats past
// one when C*H*W is not a multiple of 4, so unit 0 and the last unit may be partial). The 16 source bytes of a unit lie in one
// stored row whenever the unit does not cross an output row: they are read with one 16-byte load at whatever address they have
// (no widening to aligned words, so no byte that is not needed is ever touched), reversed in registers for a flipped clip. A
// unit that crosses an output row falls back to one 4-byte load per float4 that stays inside a row and to byte loads for the
// rest. Full float4s are stored wide, partial ones (slot edges) and unaligned output buffers by scalars.
struct AugPos { int c, y, x; };

__device__ inline void aug_step(AugPos& p, int n, int H, int W) {
    p.x += n;
    while (p.x >= W) {
        p.x -= W;
        if (++p.y == H) { p.y = 0; ++p.c; }
    }
}

__global__ __launch_bounds__(256) void clip_gather_aug_k(const uint8_t* __restrict__ cache, int64_t n_rows, const int64_t* __restrict__ row_index,
                                                         const int32_t* __restrict__ win, int T, int C, int Hc, int Wc, int H, int W, int upr,
                                                         const float* __restrict__ lut, float* __restrict__ out, int32_t* __restrict__ err) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int64_t slot = blockIdx.x;
    const int N = C * H * W;
    int64_t row = row_index[slot];
    const int32_t* wb = win + (slot / T) * 4;
    int y0 = wb[0], x0 = wb[1], flip = wb[2];
    bool bad = false;
    if (row < 0 || row >= n_rows) { row = row < 0 ? 0 : n_rows - 1; bad = true; }     // never dereferenced as given: clamped and flagged
    if (y0 < 0 || y0 > Hc - H) { y0 = y0 < 0 ? 0 : Hc - H; bad = true; }
    if (x0 < 0 || x0 > Wc - W) { x0 = x0 < 0 ? 0 : Wc - W; bad = true; }
    if (flip < 0 || flip > 1) { flip = flip < 0 ? 0 : 1; bad = true; }
    if (bad && err && threadIdx.x == 0 && blockIdx.y == 0) *err = 1;
    const uint8_t* src = cache + row * ((int64_t)C * Hc * Wc) + (int64_t)y0 * Wc + x0;    // byte [c, y0, x0] of the frame, c = 0
    const int64_t e0 = slot * N;                      // first output float of the slot
    const int mis = (int)(e0 & 3);
    float* dst = out + e0;
    const bool wide = ((uintptr_t)out & 15u) == 0;
    for (int k = blockIdx.y * 256 + threadIdx.x; k < upr; k += gridDim.y * 256) {
        int i = 16 * k - mis;                         // first float of the unit inside the slot (< 0: the part in front belongs to slot - 1)
        if (i >= N) break;
        const int first = i < 0 ? 0 : i;
        AugPos p;
        p.c = first / (H * W);
        const int r = first - p.c * (H * W);
        p.y = r / W;
        p.x = r - p.y * W;
        uint32_t w[4] = {0u, 0u, 0u, 0u};             // the unit's bytes in OUTPUT order, four per word
        if (i >= 0 && i + 16 <= N && p.x + 16 <= W) {
            const uint8_t* s = src + (p.c * Hc + p.y) * Wc + (flip ? W - 16 - p.x : p.x);
            uint32_t t[4];
            __builtin_memcpy(t, s, 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = flip ? __builtin_bswap32(t[3 - j]) : t[j];
        } else {
            int q = i;
#pragma unroll
            for (int j = 0; j < 4; ++j, q += 4) {
                if (q >= 0 && q + 4 <= N && p.x + 4 <= W) {
                    const uint8_t* s = src + (p.c * Hc + p.y) * Wc + (flip ? W - 4 - p.x : p.x);
                    uint32_t t;
                    __builtin_memcpy(&t, s, 4);
                    w[j] = flip ? __builtin_bswap32(t) : t;
                    aug_step(p, 4, H, W);
                } else {
                    for (int m = 0; m < 4; ++m) {
                        if (q + m < 0 || q + m >= N) continue;
                        w[j] |= (uint32_t)src[(p.c * Hc + p.y) * Wc + (flip ? W - 1 - p.x : p.x)] << (8 * m);
                        aug_step(p, 1, H, W);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = i + 4 * j;
            float v[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) v[m] = s_lut[(w[j] >> (8 * m)) & 0xffu];
            if (wide && q >= 0 && q + 4 <= N) {
                *reinterpret_cast<float4*>(dst + q) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (q + m >= 0 && q + m < N) dst[q + m] = v[m];
            }
        }
    }
}

}  // namespace

extern "C" int t2v_synth_clips(const int64_t* index_dev, int B, int64_t seed, int T, int C, int S, const int32_t* vocab_ids, float* vids,
                               int64_t* tokens, int32_t* err_dev, void* stream) {
    if (!index_dev || !vocab_ids || !vids || !tokens || B < 1 || T < 2 || C < 1 || S < BLOB || (S % 4) != 0) return T2V_EINVAL;
    if ((int64_t)B * T * C * S * S >= (1LL << 40)) return T2V_EINVAL;
    SynthVocab voc;
    for (int i = 0; i < T2V_SYNTH_VOCAB; ++i) voc.id[i] = vocab_ids[i];
    (void)hipGetLastError();
    hipLaunchKernelGGL(synth_clips_k, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, index_dev, seed, T, C, S, voc, vids, tokens, err_dev);
    return hipGetLastError() == hipSuccess ? T2V_OK : T2V_ELAUNCH;
}

extern "C" int t2v_clip_gather(const uint8_t* cache_u8, int64_t n_rows, const int64_t* row_index, int B, int T, int C, int H, int W,
                               const float* lut, float* out, int32_t* err_dev, void* stream) {
    if (!cache_u8 || !row_index || !lut || !out || n_rows < 1 || B < 1 || T < 1 || C < 1 || H < 1 || W < 1) return T2V_EINVAL;
    const int64_t N = (int64_t)C * H * W, n_slots = (int64_t)B * T;
    if (N >= (1LL << 30) || n_slots * N >= (1LL << 40) || n_rows >= (1LL << 40) / N) return T2V_EINVAL;
    const int upr = (int)(N / 16) + 2;                // units per row: head + aligned 16-byte chunks + tail
    const int64_t blocks = (n_slots * upr + 255) / 256;
    if (blocks >= (1LL << 31)) return T2V_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(clip_gather_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cache_u8, n_rows, row_index, n_slots, N, upr,
                       lut, out, err_dev);
    return hipGetLastError() == hipSuccess ? T2V_OK : T2V_ELAUNCH;
}

extern "C" int t2v_clip_gather_aug(const uint8_t* cache_u8, int64_t n_rows, const int64_t* row_index, const int32_t* win, int B, int T, int C,
                                   int Hc, int Wc, int H, int W, const float* lut, float* out, int32_t* err_dev, void* stream) {
    if (!cache_u8 || !row_index || !win || !lut || !out || n_rows < 1 || B < 1 || T < 1 || C < 1 || H < 1 || W < 1 || H > Hc || W > Wc)
        return T2V_EINVAL;
    const int64_t Nc = (int64_t)C * Hc * Wc, N = (int64_t)C * H * W, n_slots = (int64_t)B * T;
    if (Nc >= (1LL << 30) || n_slots * N >= (1LL << 40) || n_rows >= (1LL << 40) / Nc || n_slots >= (1LL << 31)) return T2V_EINVAL;
    if (((uintptr_t)out & 3u) != 0) return T2V_EINVAL;
    const int upr = (int)(N / 16) + 2;                // units per slot: 16 floats each, cut at the output's 16-byte boundaries
    const int by = (upr + 255) / 256;
    (void)hipGetLastError();
    hipLaunchKernelGGL(clip_gather_aug_k, dim3((unsigned)n_slots, (unsigned)(by < 65535 ? by : 65535)), dim3(256), 0, (hipStream_t)stream,
                       cache_u8, n_rows, row_index, win, T, C, Hc, Wc, H, W, upr, lut, out, err_dev);
    return hipGetLastError() == hipSuccess ? T2V_OK : T2V_ELAUNCH;
}
