// kid.hip — blocked Gram sums of the Kernel Inception Distance estimator (opt-in evaluation, --eval_period; gfx950).
// One definition (include/t2v_hip.h, t2v_kid_sums). X, Y [n, d] fp32, rows [b*s, (b+1)*s) of each form block b of nb = n / s, and
// with k(u, v) = (alpha u.v + 1)^3
//   out[b][0] = sum_{i != j} k(x_i, x_j)    out[b][1] = sum_{i != j} k(y_i, y_j)    out[b][2] = sum_{i, j} k(x_i, y_j)
// fp64 throughout: the features are widened on the way into LDS, the dot products run on v_mfma_f64_16x16x4_f64, the cube and
// every sum are double. One workgroup (4 waves) per 64x64 tile of one of the three Grams of one block: k-chunks of 32 columns go
// through LDS k-major, each wave owns a 32x32 quarter as 2x2 MFMA tiles. Operands outside the block or beyond d are zero-filled,
// and the epilogue masks by row and column index (a padded entry would be k = 1, not 0). The x.x and y.y Grams are symmetric:
// tiles below the diagonal are not computed, tiles above it count twice (an exact doubling). Every tile writes one partial to
// the workspace (lanes in the wave's butterfly, then the waves in order); a second kernel adds a Gram's partials in one fixed
// order. No atomics: the same bits run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/t2v_hip.h"

#define T2V_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define S_(stream) ((hipStream_t)(stream))

static inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2V_OK : -(int)e - 1000;
}

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define KD_T 256                          // threads per workgroup: 4 waves, a 32x32 quarter of the tile each
#define KD_TILE 64                        // rows and columns of a tile
#define KD_KC 32                          // k-columns per LDS chunk
#define KD_LD (KD_TILE + 1)               // row pitch of the k-major LDS image in doubles (odd: the transposing stores spread over the banks)
#define KD_R 256                          // threads of the reduce kernel

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rows [r0, r0 + 64) x columns [k0, k0 + 32) of a block's features into dst[k][row], widened; zero outside [0, s) x [0, d)
__device__ __forceinline__ void kd_stage(const float* __restrict__ src, int s, int d, int r0, int k0, double* __restrict__ dst) {
    const int k = threadIdx.x & (KD_KC - 1), rr = threadIdx.x >> 5;          // 8 rows per pass, a row's 32 columns on 32 lanes
    float v[KD_TILE / 8];
#pragma unroll
    for (int p = 0; p < KD_TILE / 8; ++p) {
        const int r = r0 + rr + 8 * p;
        v[p] = (r < s && k0 + k < d) ? src[(size_t)r * d + (k0 + k)] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < KD_TILE / 8; ++p) dst[k * KD_LD + rr + 8 * p] = (double)v[p];
}

// grid (T * T, 3, nb), T = ceil(s / 64): partial[(b * 3 + g) * T * T + tile] = this tile's share of out[b][g]
__global__ __launch_bounds__(KD_T) void kid_tile_k(const float* __restrict__ X, const float* __restrict__ Y, int d, int s, int T,
                                                   double alpha, double* __restrict__ partial) {
    __shared__ double As[KD_KC * KD_LD], Bs[KD_KC * KD_LD];
    __shared__ double red[KD_T / 64];
    const int g = blockIdx.y, b = blockIdx.z;
    const int ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
    double* __restrict__ slot = partial + ((size_t)b * 3 + g) * T * T + blockIdx.x;
    const bool sym = g < 2;
    if (sym && tj < ti) {                                                     // (the mirror tile counts twice)
        if (threadIdx.x == 0) *slot = 0.0;
        return;
    }
    const float* __restrict__ A = (g == 1 ? Y : X) + (size_t)b * s * d;
    const float* __restrict__ B = (g == 0 ? X : Y) + (size_t)b * s * d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;                    // this wave's quarter
    const int l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += KD_KC) {
        kd_stage(A, s, d, ti * KD_TILE, k0, As);
        kd_stage(B, s, d, tj * KD_TILE, k0, Bs);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KD_KC; kk += 4) {
            // A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]: one double per lane
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = As[(kk + l4) * KD_LD + wr + 16 * a + l15];
#pragma unroll
            for (int c = 0; c < 2; ++c) bv[c] = Bs[(kk + l4) * KD_LD + wc + 16 * c + l15];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[c], acc[a][c], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * KD_TILE + wr + 16 * a + l4 + 4 * r;
                const int j = tj * KD_TILE + wc + 16 * c + l15;
                const double t = alpha * acc[a][c][r] + 1.0;
                const bool in = i < s && j < s && !(sym && i == j);
                sum += in ? t * t * t : 0.0;
            }
    sum = wave_sum_f64(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < KD_T / 64; ++w) t += red[w];
        *slot = (sym && tj > ti) ? 2.0 * t : t;
    }
}

// one workgroup per (block, Gram): thread t adds partials t, t + 256, ... in order, then a tree over LDS in one fixed order
__global__ __launch_bounds__(KD_R) void kid_reduce_k(const double* __restrict__ partial, int count, double* __restrict__ out) {
    __shared__ double red[KD_R];
    const double* __restrict__ p = partial + (size_t)blockIdx.x * count;
    double t = 0.0;
    for (int i = threadIdx.x; i < count; i += KD_R) t += p[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = KD_R / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

static inline long kd_tiles(int s) { return (s + KD_TILE - 1) / KD_TILE; }

// every refusal that needs no pointer: the sizes, and a tile grid the launch can express
static bool kd_sizes_ok(int n, int d, int s) {
    if (n < 2 || d < 1 || s < 2 || s > n || n % s != 0) return false;
    const long T = kd_tiles(s);
    return T * T <= 0x7fffffffL && n / s <= 65535;
}

extern "C" size_t t2v_kid_sums_ws_bytes(int n, int d, int s) {
    if (!kd_sizes_ok(n, d, s)) return 0;
    const long T = kd_tiles(s);
    return (size_t)(n / s) * 3 * (size_t)(T * T) * sizeof(double);
}

extern "C" int t2v_kid_sums(const float* X, const float* Y, int n, int d, int s, double alpha, double* out, void* ws, void* st) {
    if (!X || !Y || !out || !ws || !kd_sizes_ok(n, d, s) || !(alpha == alpha)) return T2V_EINVAL;
    const int nb = n / s, T = (int)kd_tiles(s);
    T2V_LAUNCH(kid_tile_k, dim3(T * T, 3, nb), dim3(KD_T), 0, S_(st), X, Y, d, s, T, alpha, (double*)ws);
    int status = launch_status();
    if (status != T2V_OK) return status;
    T2V_LAUNCH(kid_reduce_k, dim3(nb * 3), dim3(KD_R), 0, S_(st), (const double*)ws, T * T, out);
    return launch_status();
}
