// prdc.hip — k-nearest-neighbour radii and membership counts of improved precision/recall (Kynkaanniemi et al. 2019) and
// density/coverage (Naeem et al. 2020) on the feature banks of the KID evaluation (opt-in, --eval_prdc; gfx950).
// One definition (include/t2v_hip.h, t2v_knn_radii / t2v_prdc_counts): D2(u, v) = max(0, |u|^2 + |v|^2 - 2 u.v), a radius is the
// k-th smallest D2 of a row to the other rows of its own bank, and the four counts compare D2(x_i, y_j) with those radii.
// fp64 throughout, as in kid.hip and for its reason: the features are widened on the way into LDS, the dot products run on
// v_mfma_f64_16x16x4_f64, the row norms are double. The k-major staging and the 2x2 MFMA core are kid.hip's, duplicated here
// (kid.hip stays untouched), with the next chunk's global loads issued in front of a chunk's MFMAs. The n x n distance
// matrices never reach memory: one workgroup (4 waves) per 64x64 tile puts the finished tile of D2 into the staging LDS (the same
// 33 KB) and selects there —
//   radii:  every row keeps its k smallest off-diagonal values of the tile (4 threads per row, 16 columns each, sorted insertion
//           in registers, then the row's first thread merges the four lists) and writes them as the (row, column-tile) partial; a
//           second launch merges a row's partials and writes the k-th smallest. The k smallest of a multiset do not depend on the
//           order of visiting: the same bits run to run.
//   counts: per column the number of tile rows with D2 <= rX[row], per row whether a tile column has D2 <= rY[col], per row the
//           tile's minimum, as partials; a second launch folds them per index and adds four integers (integer atomics: an
//           integer sum has no order).
// Rows and columns outside the bank and, in the radii, the diagonal are masked BY INDEX to +inf: a zero-filled padded operand
// would otherwise be a neighbour at distance |u|^2.
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

#define PR_T 256                          // threads per workgroup: 4 waves, a 32x32 quarter of the tile each
#define PR_TILE 64                        // rows and columns of a tile
#define PR_KC 32                          // k-columns per LDS chunk
#define PR_LD (PR_TILE + 1)               // pitch in doubles of the k-major staging image AND of the finished tile (odd: the transposing
                                          // stores spread over the banks; a wave's 64 rows of one column fall on 64 distinct 8-byte slots)
#define PR_K T2V_KNN_MAX_K                // length of the sorted list a thread keeps in registers
#define PR_INF __builtin_huge_val()

static_assert(2 * PR_KC * PR_LD == PR_TILE * PR_LD, "the finished tile reuses the staging LDS exactly");
static_assert(PR_K == 16 && PR_TILE == 4 * PR_K, "four threads per row select among 16 columns each");

// ---- row norms in double: one wave per row --------------------------------------------------------------------------------------
// grid (ceil(n / 4), 1 or 2): nrm[y][i] = |row i of (y ? V : U)|^2. `zero` (counts only): four integers cleared for the last launch
__global__ __launch_bounds__(PR_T) void pr_sqnorm_k(const float* __restrict__ U, const float* __restrict__ V, int n, int d,
                                                    double* __restrict__ nrm, unsigned long long* __restrict__ zero) {
    if (zero && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) zero[threadIdx.x] = 0ull;
    const int lane = threadIdx.x & 63, i = blockIdx.x * (PR_T / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                                                       // (whole waves: the butterfly below stays full)
    const float* __restrict__ row = (blockIdx.y ? V : U) + (size_t)i * d;
    double t = 0.0;
    for (int k = lane; k < d; k += 64) {
        const double v = (double)row[k];
        t += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) nrm[(size_t)blockIdx.y * n + i] = t;
}

// ---- the tile of D2 (kid.hip's staging layout and MFMA core)--------------------------------------------------------------------
// rows [r0, r0 + 64) x columns [k0, k0 + 32) of src [n, d]: a thread's 8 values into registers (zero outside [0, n) x [0, d)), and
// from there into dst[k][row], widened. Two halves, so that the next chunk's loads are in flight under this chunk's MFMAs
__device__ __forceinline__ void pr_fetch(const float* __restrict__ src, int n, int d, int r0, int k0, float (&v)[PR_TILE / 8]) {
    const int k = threadIdx.x & (PR_KC - 1), rr = threadIdx.x >> 5;          // 8 rows per pass, a row's 32 columns on 32 lanes
#pragma unroll
    for (int p = 0; p < PR_TILE / 8; ++p) {
        const int r = r0 + rr + 8 * p;
        v[p] = (r < n && k0 + k < d) ? src[(size_t)r * d + (k0 + k)] : 0.f;
    }
}

__device__ __forceinline__ void pr_put(const float (&v)[PR_TILE / 8], double* __restrict__ dst) {
    const int k = threadIdx.x & (PR_KC - 1), rr = threadIdx.x >> 5;
#pragma unroll
    for (int p = 0; p < PR_TILE / 8; ++p) dst[k * PR_LD + rr + 8 * p] = (double)v[p];
}

// D2(a_i, b_j) of tile (ti, tj) into sm[row * PR_LD + col]; +inf where i >= n, j >= n or (diag and i == j). nA, nB: the row norms.
// Ends behind a barrier: every thread may read the whole tile.
__device__ __forceinline__ void pr_tile(const float* __restrict__ A, const float* __restrict__ B, const double* __restrict__ nA,
                                        const double* __restrict__ nB, int n, int d, int ti, int tj, bool diag, double* __restrict__ sm,
                                        double* __restrict__ nAs, double* __restrict__ nBs) {
    double* __restrict__ As = sm;
    double* __restrict__ Bs = sm + PR_KC * PR_LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;                    // this wave's quarter
    const int l15 = lane & 15, l4 = lane >> 4;
    if (threadIdx.x < PR_TILE) {
        const int i = ti * PR_TILE + threadIdx.x;
        nAs[threadIdx.x] = i < n ? nA[i] : 0.0;
    } else if (threadIdx.x < 2 * PR_TILE) {
        const int j = tj * PR_TILE + threadIdx.x - PR_TILE;
        nBs[threadIdx.x - PR_TILE] = j < n ? nB[j] : 0.0;
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = (f64x4){0.0, 0.0, 0.0, 0.0};
    float va[PR_TILE / 8], vb[PR_TILE / 8];
    pr_fetch(A, n, d, ti * PR_TILE, 0, va);
    pr_fetch(B, n, d, tj * PR_TILE, 0, vb);
    for (int k0 = 0; k0 < d; k0 += PR_KC) {
        pr_put(va, As);
        pr_put(vb, Bs);
        __syncthreads();
        if (k0 + PR_KC < d) {
            pr_fetch(A, n, d, ti * PR_TILE, k0 + PR_KC, va);
            pr_fetch(B, n, d, tj * PR_TILE, k0 + PR_KC, vb);
        }
#pragma unroll
        for (int kk = 0; kk < PR_KC; kk += 4) {
            // A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]: one double per lane
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = As[(kk + l4) * PR_LD + wr + 16 * a + l15];
#pragma unroll
            for (int c = 0; c < 2; ++c) bv[c] = Bs[(kk + l4) * PR_LD + wc + 16 * c + l15];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[c], acc[a][c], 0, 0, 0);
        }
        __syncthreads();                                                      // (also: the staging image is free, the norms are in)
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr + 16 * a + l4 + 4 * r, col = wc + 16 * c + l15;
                const int i = ti * PR_TILE + row, j = tj * PR_TILE + col;
                const double d2 = fmax(0.0, (nAs[row] + nBs[col]) - 2.0 * acc[a][c][r]);
                sm[row * PR_LD + col] = (i < n && j < n && !(diag && i == j)) ? d2 : PR_INF;
            }
    __syncthreads();
}

// L ascending; v takes its place if it is among the PR_K smallest (a NaN is never smaller: it is dropped)
__device__ __forceinline__ void pr_insert(double (&L)[PR_K], double v) {
#pragma unroll
    for (int s = PR_K - 1; s > 0; --s) L[s] = v < L[s - 1] ? L[s - 1] : (v < L[s] ? v : L[s]);
    L[0] = v < L[0] ? v : L[0];
}

// ---- radii ----------------------------------------------------------------------------------------------------------------------
// grid (T, T), T = ceil(n / 64), block (tj = x, ti = y): part[(tj * k + s) * n + i] = the s-th smallest D2(u_i, u_j), j != i in tile tj
__global__ __launch_bounds__(PR_T) void pr_knn_tile_k(const float* __restrict__ U, const double* __restrict__ nrm, int n, int d, int k,
                                                      double* __restrict__ part) {
    __shared__ double sm[PR_TILE * PR_LD];
    __shared__ double nAs[PR_TILE], nBs[PR_TILE];
    const int tj = blockIdx.x, ti = blockIdx.y;
    pr_tile(U, U, nrm, nrm, n, d, ti, tj, true, sm, nAs, nBs);
    const int row = threadIdx.x & 63, q = threadIdx.x >> 6;                   // a wave = one quarter of the columns, a lane = one row
    double* __restrict__ mine = sm + row * PR_LD + PR_K * q;                  // read and written by this thread alone
    double L[PR_K];
#pragma unroll
    for (int s = 0; s < PR_K; ++s) L[s] = PR_INF;
#pragma unroll
    for (int c = 0; c < PR_K; ++c) pr_insert(L, mine[c]);
#pragma unroll
    for (int s = 0; s < PR_K; ++s) mine[s] = L[s];                            // the 16 columns, sorted in place
    __syncthreads();
    if (q != 0) return;
    for (int o = 1; o < 4; ++o)                                               // only a list's first k can be among the row's first k
        for (int s = 0; s < k; ++s) pr_insert(L, mine[PR_K * o + s]);
    const int i = ti * PR_TILE + row;
    if (i >= n) return;
#pragma unroll
    for (int s = 0; s < PR_K; ++s)
        if (s < k) part[((size_t)tj * k + s) * n + i] = L[s];
}

// one thread per row: the k-th smallest of its T * k partial values
__global__ __launch_bounds__(PR_T) void pr_knn_merge_k(const double* __restrict__ part, int n, int T, int k, double* __restrict__ r2) {
    const int i = blockIdx.x * PR_T + threadIdx.x;
    if (i >= n) return;
    double L[PR_K];
#pragma unroll
    for (int s = 0; s < PR_K; ++s) L[s] = PR_INF;
    for (int t = 0; t < T; ++t)
        for (int s = 0; s < k; ++s) pr_insert(L, part[((size_t)t * k + s) * n + i]);
    double out = PR_INF;
#pragma unroll
    for (int s = 0; s < PR_K; ++s)
        if (s == k - 1) out = L[s];
    r2[i] = out;
}

// ---- counts ---------------------------------------------------------------------------------------------------------------------
// grid (T, T), block (tj = x, ti = y), on D2(x_i, y_j):
//   colcnt[ti * n + j] = #{ i in tile ti : D2 <= rX[i] }    rowany[tj * n + i] = exists j in tile tj : D2 <= rY[j]    rowmin[tj * n + i] = min_j D2
__global__ __launch_bounds__(PR_T) void pr_counts_tile_k(const float* __restrict__ X, const float* __restrict__ Y,
                                                         const double* __restrict__ nX, const double* __restrict__ nY,
                                                         const double* __restrict__ rX, const double* __restrict__ rY, int n, int d,
                                                         int* __restrict__ colcnt, int* __restrict__ rowany, double* __restrict__ rowmin) {
    __shared__ double sm[PR_TILE * PR_LD];
    __shared__ double nAs[PR_TILE], nBs[PR_TILE], rXs[PR_TILE], rYs[PR_TILE];
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (threadIdx.x >= 2 * PR_TILE && threadIdx.x < 3 * PR_TILE) {            // (visible behind pr_tile's barriers; a padded radius
        const int i = ti * PR_TILE + threadIdx.x - 2 * PR_TILE;               //  is never met: its D2 is +inf)
        rXs[threadIdx.x - 2 * PR_TILE] = i < n ? rX[i] : -1.0;
    } else if (threadIdx.x >= 3 * PR_TILE) {
        const int j = tj * PR_TILE + threadIdx.x - 3 * PR_TILE;
        rYs[threadIdx.x - 3 * PR_TILE] = j < n ? rY[j] : -1.0;
    }
    pr_tile(X, Y, nX, nY, n, d, ti, tj, false, sm, nAs, nBs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {                                                          // a lane = one column, down the tile's rows
        const int j = tj * PR_TILE + lane;
        int cnt = 0;
#pragma unroll 8
        for (int r = 0; r < PR_TILE; ++r) cnt += sm[r * PR_LD + lane] <= rXs[r] ? 1 : 0;
        if (j < n) colcnt[(size_t)ti * n + j] = cnt;
    } else if (wave == 1) {                                                   // a lane = one row, along the tile's columns
        const int i = ti * PR_TILE + lane;
        int any = 0;
        double mn = PR_INF;
#pragma unroll 8
        for (int c = 0; c < PR_TILE; ++c) {
            const double v = sm[lane * PR_LD + c];
            any |= v <= rYs[c] ? 1 : 0;
            mn = fmin(mn, v);
        }
        if (i < n) {
            rowany[(size_t)tj * n + i] = any;
            rowmin[(size_t)tj * n + i] = mn;
        }
    }
}

// one thread per index: folds the T partials of column j = index and of row i = index, then the workgroup adds its four integers
__global__ __launch_bounds__(PR_T) void pr_counts_fold_k(const int* __restrict__ colcnt, const int* __restrict__ rowany,
                                                         const double* __restrict__ rowmin, const double* __restrict__ rX, int n, int T,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long red[PR_T / 64][4];
    const int x = blockIdx.x * PR_T + threadIdx.x;
    unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
    if (x < n) {
        long long cc = 0;
        int any = 0;
        double mn = PR_INF;
        for (int t = 0; t < T; ++t) {
            cc += colcnt[(size_t)t * n + x];
            any |= rowany[(size_t)t * n + x];
            mn = fmin(mn, rowmin[(size_t)t * n + x]);
        }
        c[0] = cc > 0 ? 1ull : 0ull;
        c[1] = (unsigned long long)cc;
        c[2] = any ? 1ull : 0ull;
        c[3] = mn <= rX[x] ? 1ull : 0ull;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[m] += __shfl_xor(c[m], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m) red[threadIdx.x >> 6][m] = c[m];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0ull;
#pragma unroll
        for (int w = 0; w < PR_T / 64; ++w) t += red[w][threadIdx.x];
        if (t) atomicAdd(counts + threadIdx.x, t);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static inline long pr_tiles(int n) { return ((long)n + PR_TILE - 1) / PR_TILE; }

// every refusal that needs no pointer: the sizes, and a tile grid the launch can express
static bool pr_sizes_ok(int n, int d, int k) {
    if (n < 2 || d < 1 || k < 1 || k > T2V_KNN_MAX_K || k >= n) return false;
    return pr_tiles(n) <= 65535;
}

extern "C" size_t t2v_knn_radii_ws_bytes(int n, int d, int k) {
    if (!pr_sizes_ok(n, d, k)) return 0;
    return ((size_t)n + (size_t)pr_tiles(n) * k * n) * sizeof(double);       // the norms, then the (column-tile, s, row) partials
}

extern "C" size_t t2v_prdc_counts_ws_bytes(int n, int d, int k) {
    if (!pr_sizes_ok(n, d, k)) return 0;
    const size_t Tn = (size_t)pr_tiles(n) * n;                                // norms of X and Y, row minima; then the two integer planes
    return (2 * (size_t)n + Tn) * sizeof(double) + 2 * Tn * sizeof(int);
}

extern "C" int t2v_knn_radii(const float* U, int n, int d, int k, double* r2_out, void* ws, void* st) {
    if (!U || !r2_out || !ws || !pr_sizes_ok(n, d, k)) return T2V_EINVAL;
    const int T = (int)pr_tiles(n);
    double* nrm = (double*)ws;
    double* part = nrm + n;
    T2V_LAUNCH(pr_sqnorm_k, dim3((n + 3) / 4, 1), dim3(PR_T), 0, S_(st), U, U, n, d, nrm, (unsigned long long*)nullptr);
    int status = launch_status();
    if (status != T2V_OK) return status;
    T2V_LAUNCH(pr_knn_tile_k, dim3(T, T), dim3(PR_T), 0, S_(st), U, (const double*)nrm, n, d, k, part);
    status = launch_status();
    if (status != T2V_OK) return status;
    T2V_LAUNCH(pr_knn_merge_k, dim3((n + PR_T - 1) / PR_T), dim3(PR_T), 0, S_(st), (const double*)part, n, T, k, r2_out);
    return launch_status();
}

extern "C" int t2v_prdc_counts(const float* X, const float* Y, int n, int d, int k, const double* rX, const double* rY,
                               int64_t* counts_out, void* ws, void* st) {
    if (!X || !Y || !rX || !rY || !counts_out || !ws || !pr_sizes_ok(n, d, k)) return T2V_EINVAL;
    const int T = (int)pr_tiles(n);
    const size_t Tn = (size_t)T * n;
    double* nrm = (double*)ws;                                                // [2][n]
    double* rowmin = nrm + 2 * (size_t)n;
    int* colcnt = (int*)(rowmin + Tn);
    int* rowany = colcnt + Tn;
    unsigned long long* counts = (unsigned long long*)counts_out;
    T2V_LAUNCH(pr_sqnorm_k, dim3((n + 3) / 4, 2), dim3(PR_T), 0, S_(st), X, Y, n, d, nrm, counts);
    int status = launch_status();
    if (status != T2V_OK) return status;
    T2V_LAUNCH(pr_counts_tile_k, dim3(T, T), dim3(PR_T), 0, S_(st), X, Y, (const double*)nrm, (const double*)(nrm + n), rX, rY, n, d,
               colcnt, rowany, rowmin);
    status = launch_status();
    if (status != T2V_OK) return status;
    T2V_LAUNCH(pr_counts_fold_k, dim3((n + PR_T - 1) / PR_T), dim3(PR_T), 0, S_(st), (const int*)colcnt, (const int*)rowany,
               (const double*)rowmin, rX, n, T, counts);
    return launch_status();
}
