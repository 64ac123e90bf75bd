// Embedding statistics, part 1 (acx_moments, acx_gram_f64, acx_pca_transform, acx_pca_inverse in include/acx.h, which states
// every sum order).
//
//   f64_tile_body           the float64 product tile on v_mfma_f64_16x16x4_f64: a wave owns 32 x 32 results as 2 x 2 instruction
//                           tiles, four waves a 64 x 64 tile.  Operands as the f32 16x16x4 form (lane l: A[l & 15][k = l >> 4],
//                           B[k = l >> 4][l & 15]); results at col = l & 15, row = (l >> 4) + 4 reg -- NOT the f32 C/D map.
//   moments_colsum / mean   float64 column sums per slice in a fixed order, then the mean; NaN / Inf detection.
//   moments_cov_kernel      (tile pair b >= a, slice): fp32 rows centred on load in float64, the slice's partial tile to the
//                           workspace.  One instruction takes 64 cycles of the matrix pipe and a wave needs one scalar load per
//                           instruction: the operands come straight from global memory (L2), clamped and predicated at the
//                           tails, the next trip's loads issued ahead of this trip's instructions.
//   moments_finish_kernel   the slices' partials in ascending slice order, / (n - ddof), written with the mirror image.
//   gram_f64_kernel         out = A^T B on the same tile body, one slice.
//   pca_transform / inverse fp32 projections on v_mfma_f32_32x32x2_f32, predicated for every dim.
//
// No float atomics; the only atomics are status bits.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kStTile = 64;                  // results per workgroup: 64 x 64
constexpr int kMomMaxSlices = 16;            // default slicing of acx_moments
constexpr int kMomMinSliceRows = 1024;
constexpr int kMomGridSlices = 65535;        // the slices are the launch's second grid dimension

// acc[u][v] = sum over the steps of the 16 x 16 products of four rows each: step k4 covers rows 4 k4 .. 4 k4 + 3, this lane
// holding row k = 4 k4 + (lane >> 4).  la(u, k) / lb(v, k) LOAD this lane's raw operand of instruction tile u / v (from a clamped
// address: any k is safe), fa(u, k, raw) / fb(v, k, raw) make the float64 operand of it (zero past the end).  Four steps per trip,
// and the next trip's sixteen loads are issued ahead of this trip's sixteen instructions, so they fly under 1 024 cycles of
// matrix pipe instead of in front of them.
template <class TA, class TB, class LA, class FA, class LB, class FB>
__device__ __forceinline__ void f64_tile_body(f64x4 (&acc)[2][2], int steps, int kq, LA la, FA fa, LB lb, FB fb) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4(0.0);
    TA ra[4][2];
    TB rb[4][2];
    auto fetch = [&](int k16) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u) { ra[j][u] = la(u, 4LL * (k16 + j) + kq); rb[j][u] = lb(u, 4LL * (k16 + j) + kq); }
    };
    fetch(0);
    for (int k16 = 0; k16 < steps; k16 += 4) {
        double a[4][2], b[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[j][u] = fa(u, 4LL * (k16 + j) + kq, ra[j][u]);
                b[j][u] = fb(u, 4LL * (k16 + j) + kq, rb[j][u]);
            }
        __builtin_amdgcn_sched_barrier(0);               // the operands of this trip are made: nothing below moves above
        fetch(k16 + 4);
        __builtin_amdgcn_sched_barrier(0);               // the loads are out before the first instruction of the trip
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j][u], b[j][v], acc[u][v], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// result register g of instruction tile (u, v) of wave (wa, wb): its place in the 64 x 64 tile
__device__ __forceinline__ int f64_tile_row(int wa, int u, int g, int lane) { return 32 * wa + 16 * u + (lane >> 4) + 4 * g; }
__device__ __forceinline__ int f64_tile_col(int wb, int v, int lane) { return 32 * wb + 16 * v + (lane & 15); }

// ---- moments ---------------------------------------------------------------------------------------------------------------
static long long mom_slice_rows(long long n) {
    long long r = tuning().moments_slice_rows.load(std::memory_order_relaxed);
    if (r <= 0) r = std::max<long long>(kMomMinSliceRows, cdiv(n, kMomMaxSlices));
    return (r + 3) & ~3LL;
}
static int st_tiles(int dim) { return (dim + kStTile - 1) / kStTile; }
struct MomWs { size_t psum, part, end; int slices, pairs; long long rows; };
static MomWs mom_carve(long long n, int dim) {
    MomWs w;
    w.rows = mom_slice_rows(n);
    w.slices = (int)cdiv(n, w.rows);
    const int t = st_tiles(dim);
    w.pairs = t * (t + 1) / 2;
    size_t off = 0;
    w.psum = off; off += align_up((size_t)w.slices * dim * sizeof(double));
    w.part = off; off += align_up((size_t)w.slices * w.pairs * kStTile * kStTile * sizeof(double));
    w.end = off;
    return w;
}

// psum[s][j] of slice s: row i of the slice on partial i mod 4, ((p0 + p1) + p2) + p3.  Block (slice, 64 columns).
__global__ __launch_bounds__(256) void moments_colsum_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                             long long rows, double* __restrict__ psum, int* status) {
    __shared__ double s_p[3][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int j = blockIdx.y * 64 + c;
    const long long lo = (long long)blockIdx.x * rows, hi = min(n, lo + rows);
    double a = 0.0;
    bool bad = false;
    if (j < dim)
        for (long long i = lo + q; i < hi; i += 4) {
            const float v = x[i * ld + j];
            bad |= acx_nonfinite(v);
            a += (double)v;
        }
    if (q) s_p[q - 1][c] = a;
    __syncthreads();
    if (q == 0 && j < dim) psum[(long long)blockIdx.x * dim + j] = ((a + s_p[0][c]) + s_p[1][c]) + s_p[2][c];
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, ACX_STATS_NONFINITE);
}

__global__ __launch_bounds__(256) void moments_mean_kernel(const double* __restrict__ psum, int slices, int dim, long long n,
                                                           double* __restrict__ mean) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= dim) return;
    double a = 0.0;
    for (int s = 0; s < slices; ++s) a += psum[(long long)s * dim + j];
    mean[j] = a / (double)n;
}

// pair index -> (ta, tb), ta <= tb, rows of the upper triangle in order
__device__ __forceinline__ void st_pair(int p, int tiles, int& ta, int& tb) {
    int a = 0;
    while (p >= tiles - a) { p -= tiles - a; ++a; }
    ta = a; tb = a + p;
}

__global__ __launch_bounds__(256) void moments_cov_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                          long long rows, const double* __restrict__ mean, int tiles,
                                                          double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wa = wave >> 1, wb = wave & 1;
    int ta, tb;
    st_pair(blockIdx.x, tiles, ta, tb);
    const long long lo = (long long)blockIdx.y * rows, hi = min(n, lo + rows);
    int ca[2], cb[2];
    double ma[2], mb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        ca[u] = ta * kStTile + 32 * wa + 16 * u + (lane & 15);
        cb[u] = tb * kStTile + 32 * wb + 16 * u + (lane & 15);
        ma[u] = ca[u] < dim ? mean[ca[u]] : 0.0;
        mb[u] = cb[u] < dim ? mean[cb[u]] : 0.0;
    }
    // loads never leave the buffer (row and column clamped); what lies past the slice or past dim enters as zero
    const float* pa[2];
    const float* pb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) { pa[u] = x + min(ca[u], dim - 1); pb[u] = x + min(cb[u], dim - 1); }
    f64x4 acc[2][2];
    f64_tile_body<float, float>(
        acc, (int)((hi - lo + 3) / 4), lane >> 4,
        [&](int u, long long k) { return pa[u][min(lo + k, hi - 1) * ld]; },
        [&](int u, long long k, float r) { return (lo + k < hi && ca[u] < dim) ? (double)r - ma[u] : 0.0; },
        [&](int v, long long k) { return pb[v][min(lo + k, hi - 1) * ld]; },
        [&](int v, long long k, float r) { return (lo + k < hi && cb[v] < dim) ? (double)r - mb[v] : 0.0; });
    double* out = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (kStTile * kStTile);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int g = 0; g < 4; ++g) out[f64_tile_row(wa, u, g, lane) * kStTile + f64_tile_col(wb, v, lane)] = acc[u][v][g];
}

// cov[a][b] = cov[b][a] = (the slices' partials in ascending slice order) / (n - ddof) for b >= a; zeros when n - ddof == 0
__global__ __launch_bounds__(256) void moments_finish_kernel(const double* __restrict__ part, int slices, int pairs, int tiles,
                                                             int dim, long long denom, double* __restrict__ cov, long long ld_c,
                                                             int* status) {
    int ta, tb;
    st_pair(blockIdx.x, tiles, ta, tb);
    if (denom == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, ACX_STATS_DEGENERATE);
    for (int e = threadIdx.x; e < kStTile * kStTile; e += 256) {
        const int a = ta * kStTile + e / kStTile, b = tb * kStTile + e % kStTile;
        if (a >= dim || b >= dim || b < a) continue;
        double s = 0.0;
        for (int sl = 0; sl < slices; ++sl) s += part[((long long)sl * pairs + blockIdx.x) * (kStTile * kStTile) + e];
        s = denom ? s / (double)denom : 0.0;
        cov[a * ld_c + b] = s;
        cov[b * ld_c + a] = s;
    }
}

// ---- A^T B in float64 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_f64_kernel(const double* __restrict__ A, long long ld_a, const double* __restrict__ B,
                                                       long long ld_b, long long rows, int m, int n, double* __restrict__ out,
                                                       long long ld_o) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wa = wave >> 1, wb = wave & 1;
    int ca[2], cb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        ca[u] = blockIdx.y * kStTile + 32 * wa + 16 * u + (lane & 15);
        cb[u] = blockIdx.x * kStTile + 32 * wb + 16 * u + (lane & 15);
    }
    f64x4 acc[2][2];
    f64_tile_body<double, double>(
        acc, (int)((rows + 3) / 4), lane >> 4,
        [&](int u, long long k) { return A[min(k, rows - 1) * ld_a + min(ca[u], m - 1)]; },
        [&](int u, long long k, double r) { return (k < rows && ca[u] < m) ? r : 0.0; },
        [&](int v, long long k) { return B[min(k, rows - 1) * ld_b + min(cb[v], n - 1)]; },
        [&](int v, long long k, double r) { return (k < rows && cb[v] < n) ? r : 0.0; });
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int a = blockIdx.y * kStTile + f64_tile_row(wa, u, g, lane), b = blockIdx.x * kStTile + f64_tile_col(wb, v, lane);
                if (a < m && b < n) out[a * ld_o + b] = acc[u][v][g];
            }
}

// ---- PCA projections (fp32) ------------------------------------------------------------------------------------------------
// A wave owns rows i0 .. i0 + 31 and components c0 .. c0 + 31; lane (r, h): A operand row i0 + r, B operand component c0 + r.
__global__ __launch_bounds__(256) void pca_transform_kernel(const float* __restrict__ x, long long ld_x, long long n, int dim,
                                                            const float* __restrict__ mean, const float* __restrict__ w,
                                                            long long ld_w, int k, const float* __restrict__ scale,
                                                            float* __restrict__ out, long long ld_o) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const long long i0 = (long long)blockIdx.x * 128 + 32 * (threadIdx.x >> 6);
    const int c0 = blockIdx.y * 32;
    if (i0 >= n) return;                                             // wave-uniform
    const float* xr = x + min(i0 + r, n - 1) * ld_x;
    const float* wr = w + (long long)min(c0 + r, k - 1) * ld_w;
    F32Tile<32>::acc_t acc = F32Tile<32>::acc_t(0.f);
    for (int g = 0; g < dim; g += 16) {
        float a[8], b[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = g + 8 * h + e;
            const bool on = j < dim;
            a[e] = on ? xr[j] - mean[j] : 0.f;
            b[e] = on ? wr[j] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = F32Tile<32>::mfma(a[e], b[e], acc);
    }
    const int c = c0 + r;
    if (c >= k) return;
    const float sc = scale ? scale[c] : 1.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long long row = i0 + F32Tile<32>::row(i, h);
        if (row < n) out[row * ld_o + c] = scale ? acc[i] * sc : acc[i];
    }
}

// lane (r, h): A operand row i0 + r (component 2 e + h), B operand column j0 + r of W row 2 e + h
__global__ __launch_bounds__(256) void pca_inverse_kernel(const float* __restrict__ z, long long ld_z, long long n, int k,
                                                          const float* __restrict__ scale, const float* __restrict__ w,
                                                          long long ld_w, int dim, const float* __restrict__ mean,
                                                          float* __restrict__ out, long long ld_o) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const long long i0 = (long long)blockIdx.x * 128 + 32 * (threadIdx.x >> 6);
    const int j0 = blockIdx.y * 32;
    if (i0 >= n) return;                                             // wave-uniform
    const float* zr = z + min(i0 + r, n - 1) * ld_z;
    const int j = j0 + r, jc = min(j, dim - 1);
    F32Tile<32>::acc_t acc = F32Tile<32>::acc_t(0.f);
    for (int c = h; c < k + h; c += 2) {
        const bool on = c < k;
        const float a = on ? (scale ? zr[c] * scale[c] : zr[c]) : 0.f;
        const float b = on ? w[c * ld_w + jc] : 0.f;
        acc = F32Tile<32>::mfma(a, b, acc);
    }
    if (j >= dim) return;
    const float mu = mean[j];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long long row = i0 + F32Tile<32>::row(i, h);
        if (row < n) out[row * ld_o + j] = acc[i] + mu;
    }
}

static int st_check_dim(const char* who, const char* name, int dim) {
    if (dim < 1 || dim > ACX_STATS_MAX_DIM) ACX_FAIL(ACX_ERR_ARG, "%s: %s = %d (expected 1 .. %d)", who, name, dim, ACX_STATS_MAX_DIM);
    return ACX_OK;
}
static int st_check_rows(const char* who, int64_t n) {
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    return ACX_OK;
}
static int st_check_ptr(const char* who, const char* name, const void* p, int64_t ld, int width, size_t elem) {
    if (!p) ACX_FAIL(ACX_ERR_ARG, "%s: %s is null", who, name);
    if (reinterpret_cast<uintptr_t>(p) & (elem - 1)) ACX_FAIL(ACX_ERR_ARG, "%s: %s is not %zu-byte aligned", who, name, elem);
    if (ld < width) ACX_FAIL(ACX_ERR_ARG, "%s: the row stride of %s is %lld, under its width %d", who, name, (long long)ld, width);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_moments_workspace_bytes(int64_t n, int dim, size_t* out_bytes) {
    static const char* who = "acx_moments_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(st_check_rows(who, n));
    ACX_TRY(st_check_dim(who, "dim", dim));
    const MomWs w = mom_carve(n, dim);
    if (w.slices > kMomGridSlices) ACX_FAIL(ACX_ERR_ARG, "%s: %d slices of %lld rows (at most %d)", who, w.slices, w.rows, kMomGridSlices);
    *out_bytes = w.end;
    return ACX_OK;
}

int acx_moments(const float* x, int64_t ld_x, int64_t n, int dim, int ddof, double* mean, double* cov, int64_t ld_c,
                int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_moments";
    ACX_TRY(st_check_rows(who, n));
    ACX_TRY(st_check_dim(who, "dim", dim));
    if (ddof != 0 && ddof != 1) ACX_FAIL(ACX_ERR_ARG, "%s: ddof = %d (expected 0 or 1)", who, ddof);
    ACX_TRY(st_check_ptr(who, "x", x, ld_x, dim, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "mean", mean, dim, dim, sizeof(double)));
    ACX_TRY(st_check_ptr(who, "cov", cov, ld_c, dim, sizeof(double)));
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const MomWs w = mom_carve(n, dim);
    if (w.slices > kMomGridSlices) ACX_FAIL(ACX_ERR_ARG, "%s: %d slices of %lld rows (at most %d)", who, w.slices, w.rows, kMomGridSlices);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    double* psum = reinterpret_cast<double*>(base + w.psum);
    double* part = reinterpret_cast<double*>(base + w.part);
    const int tiles = st_tiles(dim);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    launch_kernel(&moments_colsum_kernel, dim3(w.slices, (dim + 63) / 64), dim3(256), 0, s, x, (long long)ld_x, (long long)n, dim,
                  w.rows, psum, (int*)status);
    launch_kernel(&moments_mean_kernel, dim3((dim + 255) / 256), dim3(256), 0, s, (const double*)psum, w.slices, dim, (long long)n, mean);
    launch_kernel(&moments_cov_kernel, dim3(w.pairs, w.slices), dim3(256), 0, s, x, (long long)ld_x, (long long)n, dim, w.rows,
                  (const double*)mean, tiles, part);
    launch_kernel(&moments_finish_kernel, dim3(w.pairs), dim3(256), 0, s, (const double*)part, w.slices, w.pairs, tiles, dim,
                  (long long)(n - ddof), cov, (long long)ld_c, (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_gram_f64(const double* a, int64_t ld_a, const double* b, int64_t ld_b, int64_t rows, int m, int n, double* out,
                 int64_t ld_o, void* stream) {
    static const char* who = "acx_gram_f64";
    if (rows < 1) ACX_FAIL(ACX_ERR_ARG, "%s: rows = %lld (expected >= 1)", who, (long long)rows);
    if (rows > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: rows = %lld (at most 2^30 rows)", who, (long long)rows);
    ACX_TRY(st_check_dim(who, "m", m));
    ACX_TRY(st_check_dim(who, "n", n));
    ACX_TRY(st_check_ptr(who, "a", a, ld_a, m, sizeof(double)));
    ACX_TRY(st_check_ptr(who, "b", b, ld_b, n, sizeof(double)));
    ACX_TRY(st_check_ptr(who, "out", out, ld_o, n, sizeof(double)));
    launch_kernel(&gram_f64_kernel, dim3(st_tiles(n), st_tiles(m)), dim3(256), 0, (hipStream_t)stream, a, (long long)ld_a, b,
                  (long long)ld_b, (long long)rows, m, n, out, (long long)ld_o);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_pca_transform(const float* x, int64_t ld_x, int64_t n, int dim, const float* mean, const float* w, int64_t ld_w, int k,
                      const float* scale, float* out, int64_t ld_o, void* stream) {
    static const char* who = "acx_pca_transform";
    ACX_TRY(st_check_rows(who, n));
    ACX_TRY(st_check_dim(who, "dim", dim));
    if (k < 1 || k > dim) ACX_FAIL(ACX_ERR_ARG, "%s: k = %d (expected 1 .. dim = %d)", who, k, dim);
    ACX_TRY(st_check_ptr(who, "x", x, ld_x, dim, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "mean", mean, dim, dim, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "w", w, ld_w, dim, sizeof(float)));
    if (scale) ACX_TRY(st_check_ptr(who, "scale", scale, k, k, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "out", out, ld_o, k, sizeof(float)));
    launch_kernel(&pca_transform_kernel, dim3((unsigned)cdiv(n, 128), (k + 31) / 32), dim3(256), 0, (hipStream_t)stream, x,
                  (long long)ld_x, (long long)n, dim, mean, w, (long long)ld_w, k, scale, out, (long long)ld_o);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_pca_inverse(const float* z, int64_t ld_z, int64_t n, int k, const float* scale, const float* w, int64_t ld_w, int dim,
                    const float* mean, float* out, int64_t ld_o, void* stream) {
    static const char* who = "acx_pca_inverse";
    ACX_TRY(st_check_rows(who, n));
    ACX_TRY(st_check_dim(who, "dim", dim));
    if (k < 1 || k > dim) ACX_FAIL(ACX_ERR_ARG, "%s: k = %d (expected 1 .. dim = %d)", who, k, dim);
    ACX_TRY(st_check_ptr(who, "z", z, ld_z, k, sizeof(float)));
    if (scale) ACX_TRY(st_check_ptr(who, "scale", scale, k, k, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "w", w, ld_w, dim, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "mean", mean, dim, dim, sizeof(float)));
    ACX_TRY(st_check_ptr(who, "out", out, ld_o, dim, sizeof(float)));
    launch_kernel(&pca_inverse_kernel, dim3((unsigned)cdiv(n, 128), (dim + 31) / 32), dim3(256), 0, (hipStream_t)stream, z,
                  (long long)ld_z, (long long)n, k, scale, w, (long long)ld_w, dim, mean, out, (long long)ld_o);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
