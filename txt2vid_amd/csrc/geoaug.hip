// geoaug.hip — geometric augmentation of the discriminator's inputs (ADA's x-flip, isotropic scaling and rotation, Karras et al.
// 2020; opt-in through the names flip, scale, rotate of --D_aug, not in the reference), gfx950. One grouped launch per
// direction, in front of diffaug.hip's: every member tensor of a step (the real and the generated pyramid, up to T2V_MAX_GROUPS)
// is resampled per clip [C, T, S, S] with the bilinear map defined in include/t2v_hip.h and txt2vid_amd/functional_aug.py
// (`geo_params`): one sampling matrix per clip, formed once per workgroup in double from the clip's row of v and rounded to fp32,
// fp32 coordinates and weights per pixel, zero outside the frame. Launch-bound work (a pyramid is 0.5 MB): plain loads and stores.
//
// The adjoint is a GATHER, so that it is deterministic without atomics: input pixel i visits, in row-major order, the 5 x 5 output
// pixels around its pre-image — s (|cos| + |sin|) <= 1.32 * 1.37 < 1.81 bounds how far an output pixel whose taps reach i can lie
// from it, and rounding the pre-image to the nearest pixel adds 0.5: |w - centre| < 2.31, so <= 2 — and takes each one's weight
// for i from geo_src / geo_weight, the device functions the forward uses. The backward is therefore the forward's transpose
// weight by weight.
//
// Gating: clip j of a member also reads row j * row_stride of the member's gate block and p from DEVICE memory;
// effective policy = policy & (8 [g3 < p] | 16 [g4 < p] | 32 [g5 < p]) with a strict fp32 <. A clip whose effective policy is 0 is
// copied, forward and adjoint. The backward re-reads gates and p (the p-invariant of §19: nothing writes p between the two).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/t2v_hip.h"

#define T2V_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define S_(stream) ((hipStream_t)(stream))

static inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2V_OK : -(int)e - 1000;
}

#define GEO_BITS (T2V_AUG_FLIP | T2V_AUG_SCALE | T2V_AUG_ROTATE)
#define GEO_MAX_PARTS 64          // workgroups one clip is split over, at most
#define GEO_PART_ELEMS 1024       // elements of a clip per workgroup before it is split: a few dependent gathers per thread
#define GEO_R 2                   // the adjoint visits (2 GEO_R + 1)^2 output pixels
#define GEO_PI_6 0.5235987755982988    // pi / 6 as a double

struct GeoBatch {
    t2v_aug_member m[T2V_MAX_GROUPS];
    int begin[T2V_MAX_GROUPS + 1];      // first workgroup of member g; a member owns N * parts[g] workgroups
    int parts[T2V_MAX_GROUPS];
    int n;
};

struct GeoGate {
    const float* g[T2V_MAX_GROUPS];     // gate block of member g, or NULL: ungated
    const float* p;                     // the probability, one float in device memory; NULL: the ungated form
};

struct GeoM {
    float m00, m01, m10, m11;           // the sampling matrix: source = M * output, both relative to the frame centre
    float i00, i01, i10, i11;           // its inverse; it only centres the adjoint's window, so its rounding is immaterial
};

// the device mirror of functional_aug.geo_params: double from the fp32 draw, one rounding per entry
__device__ __forceinline__ GeoM geo_matrix(const float* __restrict__ v, int policy) {
    double f = 1.0, s = 1.0, c = 1.0, sn = 0.0;
    if ((policy & T2V_AUG_FLIP) && v[0] < 0.5f) f = -1.0;
    if (policy & T2V_AUG_SCALE) s = exp2((2.0 * (double)v[1] - 1.0) * 0.4);
    if (policy & T2V_AUG_ROTATE) {
        const double th = (2.0 * (double)v[2] - 1.0) * GEO_PI_6;
        c = cos(th);
        sn = sin(th);
    }
    GeoM g;
    g.m00 = (float)((f * c) / s);  g.m01 = (float)((f * sn) / s);
    g.m10 = (float)((-sn) / s);    g.m11 = (float)(c / s);
    g.i00 = (float)(s * (f * c));  g.i01 = (float)(s * (-sn));
    g.i10 = (float)(s * (f * sn)); g.i11 = (float)(s * c);
    return g;
}

struct GeoSrc {
    int x0, y0;                         // the top-left tap
    float wx, wy;                       // the weights of the taps at x0 + 1 / y0 + 1
};
// Where output pixel (h, w) samples. Explicit fmaf and separately rounded steps: the forward and the adjoint get the same bits.
__device__ __forceinline__ GeoSrc geo_src(const GeoM& g, float half, int h, int w) {
    const float xo = ((float)w + 0.5f) - half, yo = ((float)h + 0.5f) - half;
    const float xs = fmaf(g.m00, xo, g.m01 * yo), ys = fmaf(g.m10, xo, g.m11 * yo);
    const float px = (xs + half) - 0.5f, py = (ys + half) - 0.5f;
    const float fx = floorf(px), fy = floorf(py);
    GeoSrc r;
    r.x0 = (int)fx;  r.y0 = (int)fy;
    r.wx = px - fx;  r.wy = py - fy;
    return r;
}
// the weight of tap (y0 + dy, x0 + dx), dy, dx in {0, 1}
__device__ __forceinline__ float geo_weight(const GeoSrc& r, int dy, int dx) {
    return (dy ? r.wy : 1.f - r.wy) * (dx ? r.wx : 1.f - r.wx);
}

// Which member, clip and part of the clip this workgroup serves; the clip's effective policy.
#define GEO_LOCATE()                                                                       \
    int g = 0;                                                                             \
    while (g + 1 < tb.n && tb.begin[g + 1] <= (int)blockIdx.x) ++g;                        \
    const t2v_aug_member& m = tb.m[g];                                                     \
    const int parts = tb.parts[g];                                                         \
    const int local = (int)blockIdx.x - tb.begin[g];                                       \
    const int clip = local / parts, part = local - clip * parts;                           \
    const int S = m.S, C = m.C;                                                            \
    int policy = m.policy;                                                                 \
    if (tg.p && tg.g[g]) {         /* uniform over the workgroup and over the parts of a clip */ \
        const float* __restrict__ gr = tg.g[g] + (long)clip * m.row_stride * T2V_AUG_K;    \
        const float pv = tg.p[0];                                                          \
        policy &= (gr[3] < pv ? T2V_AUG_FLIP : 0) | (gr[4] < pv ? T2V_AUG_SCALE : 0) | (gr[5] < pv ? T2V_AUG_ROTATE : 0); \
    }                                                                                      \
    const int V = m.T * S * S;                 /* voxels of one channel */                 \
    const long n = (long)C * V;                /* elements of the clip  */                 \
    const int per = (V + parts - 1) / parts;                                               \
    const int v0 = part * per, v1 = min(V, v0 + per);                                      \
    const float* __restrict__ src = m.x + (long)clip * n;                                  \
    float* __restrict__ dst = m.y + (long)clip * n;                                        \
    if (!policy) {                             /* nothing live: a copy, both directions */ \
        for (int v = v0 + threadIdx.x; v < v1; v += 256)                                   \
            for (int c = 0; c < C; ++c) dst[(long)c * V + v] = src[(long)c * V + v];       \
        return;                                                                            \
    }                                                                                      \
    if (threadIdx.x == 0) gm = geo_matrix(m.u + (long)clip * m.row_stride * T2V_AUG_K, policy); \
    __syncthreads();                                                                       \
    const GeoM M = gm;                                                                     \
    const float half = 0.5f * (float)S

__global__ __launch_bounds__(256) void geoaug_fwd_k(GeoBatch tb, GeoGate tg) {
    __shared__ GeoM gm;
    GEO_LOCATE();
    for (int v = v0 + threadIdx.x; v < v1; v += 256) {
        const int w = v % S, h = (v / S) % S;
        const int frame = v - (h * S + w);
        const GeoSrc r = geo_src(M, half, h, w);
        float wt[4];
        int off[4];                                  // the tap's offset in its channel, -1 outside the frame
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dy = k >> 1, dx = k & 1;
            const int ys = r.y0 + dy, xs = r.x0 + dx;
            wt[k] = geo_weight(r, dy, dx);
            off[k] = ((unsigned)ys < (unsigned)S && (unsigned)xs < (unsigned)S) ? frame + ys * S + xs : -1;
        }
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ xc = src + (long)c * V;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (off[k] >= 0) acc = fmaf(wt[k], xc[off[k]], acc);
            dst[(long)c * V + v] = acc;
        }
    }
}

// dL/dx from dL/dy (m.x -> m.y): every input pixel gathers from the output pixels that sampled it.
__global__ __launch_bounds__(256) void geoaug_bwd_k(GeoBatch tb, GeoGate tg) {
    __shared__ GeoM gm;
    GEO_LOCATE();
    constexpr int W = 2 * GEO_R + 1;
    for (int v = v0 + threadIdx.x; v < v1; v += 256) {
        const int ix = v % S, iy = (v / S) % S;
        const int frame = v - (iy * S + ix);
        // the pre-image of the input pixel's centre, as an output pixel index
        const float xi = ((float)ix + 0.5f) - half, yi = ((float)iy + 0.5f) - half;
        const int cw = (int)rintf((fmaf(M.i00, xi, M.i01 * yi) + half) - 0.5f);
        const int ch = (int)rintf((fmaf(M.i10, xi, M.i11 * yi) + half) - 0.5f);
        float wt[W * W];
        int off[W * W];                              // the candidate's offset in its channel, -1: it does not sample this pixel
#pragma unroll
        for (int k = 0; k < W * W; ++k) {
            const int h = ch - GEO_R + k / W, w = cw - GEO_R + k % W;
            wt[k] = 0.f;
            off[k] = -1;
            if ((unsigned)h < (unsigned)S && (unsigned)w < (unsigned)S) {
                const GeoSrc r = geo_src(M, half, h, w);
                const int dy = iy - r.y0, dx = ix - r.x0;
                if ((unsigned)dy < 2u && (unsigned)dx < 2u) {
                    wt[k] = geo_weight(r, dy, dx);
                    off[k] = frame + h * S + w;
                }
            }
        }
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ gc = src + (long)c * V;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < W * W; ++k)
                if (off[k] >= 0) acc = fmaf(wt[k], gc[off[k]], acc);
            dst[(long)c * V + v] = acc;
        }
    }
}

static int geo_batch(GeoBatch& tb, GeoGate& tg, const t2v_aug_member* ms, const float* const* gates, int n, const float* p,
                     long* blocks_out) {
    if (!ms || n < 1 || n > T2V_MAX_GROUPS) return T2V_EINVAL;
    if ((gates == nullptr) != (p == nullptr)) return T2V_EINVAL;              // gates and p come together
    long blocks = 0;
    for (int g = 0; g < T2V_MAX_GROUPS; ++g) {
        tb.begin[g] = (int)blocks;
        tb.parts[g] = 1;
        tg.g[g] = (gates && g < n) ? gates[g] : nullptr;
        if (g >= n) { tb.m[g] = t2v_aug_member{}; continue; }
        const t2v_aug_member& q = ms[g];
        if (!q.x || !q.y || !q.u || q.x == q.y || q.N < 1 || q.C < 1 || q.T < 1 || q.S < 1) return T2V_EINVAL;
        if (!(q.policy & GEO_BITS) || (q.policy & ~GEO_BITS)) return T2V_EINVAL;
        if (q.row_stride < 1 || q.rows < 1 || (long)(q.N - 1) * q.row_stride >= (long)q.rows) return T2V_EINVAL;
        const long V = (long)q.T * q.S * q.S, elems = V * q.C;
        if (q.S > 32768 || elems > 0x40000000L) return T2V_EINVAL;
        long parts = (elems + GEO_PART_ELEMS - 1) / GEO_PART_ELEMS;
        parts = parts > GEO_MAX_PARTS ? GEO_MAX_PARTS : parts;
        parts = parts > V ? V : parts;
        tb.m[g] = q;
        tb.parts[g] = (int)parts;
        blocks += (long)q.N * parts;
        if (blocks > 0x7fffffffL) return T2V_EINVAL;
    }
    tb.begin[T2V_MAX_GROUPS] = (int)blocks;
    tb.n = n;
    tg.p = p;
    *blocks_out = blocks;
    return T2V_OK;
}

extern "C" int t2v_geoaug_fwd(const t2v_aug_member* members, const float* const* gates, int n, const float* p, void* st) {
    GeoBatch tb;
    GeoGate tg;
    long blocks = 0;
    const int rc = geo_batch(tb, tg, members, gates, n, p, &blocks);
    if (rc != T2V_OK) return rc;
    T2V_LAUNCH(geoaug_fwd_k, dim3((unsigned)blocks), dim3(256), 0, S_(st), tb, tg);
    return launch_status();
}

extern "C" int t2v_geoaug_bwd(const t2v_aug_member* members, const float* const* gates, int n, const float* p, void* st) {
    GeoBatch tb;
    GeoGate tg;
    long blocks = 0;
    const int rc = geo_batch(tb, tg, members, gates, n, p, &blocks);
    if (rc != T2V_OK) return rc;
    T2V_LAUNCH(geoaug_bwd_k, dim3((unsigned)blocks), dim3(256), 0, S_(st), tb, tg);
    return launch_status();
}
