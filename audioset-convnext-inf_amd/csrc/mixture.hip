// Gaussian mixtures over embeddings (acx_gmm_* in include/acx.h): EM for diagonal and spherical covariances, everything on the
// device.
//
//   gmm_rows_kernel      the E-step's A operand, once per call: row i -> [fp32(xc^2), fp32(xc)] with xc = (double)x - center, 2 dim
//                        floats.  A function of the row and `center` alone.
//   gmm_prepare_kernel   the B operand, the constant and the scale of component k from the float64 parameters, with mc = mean -
//                        center.  Diagonal: [fp32(1 / v), fp32(-2 mc / v)], scale -1/2.  Spherical: [1, fp32(-2 mc)], scale
//                        -1 / (2 v_k): one variance for every column, so its fp32 rounding would be the same relative error in every
//                        term.  cst_k = log w_k - (dim log 2 pi + sum log v + sum mc^2 / v) / 2, its sums in float64 in a fixed
//                        order.  Constant and scale stay float64: rounded to fp32 they would shift every row of a component the
//                        same way, an error of the lower bound that no number of rows averages out.
//   gmm_estep_kernel     a workgroup owns 64 rows and streams all K components, 256 per step, as kmeans_assign_kernel does: each
//                        wave forms the 64 x 64 tile of the 2 dim long contraction by dot_tile (device_common.h, which states the
//                        bit contract), lp = fp32(fma(scale_k, (double)dot, cst_k)): one rounding.  Sweep 1 keeps one running key
//                        knn_make_key(lp, k) per accumulator register: the row's maximum m and its label (highest lp, then lowest
//                        index, -0.0 as +0.0).
//                        Sweep 2 forms the same tiles again -- the same bits -- and sums e = expf(lp - m) per row: over the steps in
//                        a lane, over the 32 lanes by the xor butterfly, over the four waves in wave order, a function of K alone.
//                        log_prob_norm = m + logf(s); the lower bound sums (double)m + log((double)s), which is not rounded to
//                        fp32 (a row with log s below half an ulp of m would lose it every time: a bias, not noise).  With `resp`,
//                        sweep 2 writes e there and the workgroup divides its own 64 rows by s afterwards; the n x K
//                        log-densities never go to memory.
//   gmm_lsum_kernel      the sum of those terms in float64: thread t over rows t, t + 1024, ..., then a tree.
//   gmm_msum_kernel      the M-step's float64 sums of one chunk of rows: (chunk, 256 columns, 32 components) per workgroup, eight
//                        components per wave, rows in ascending order.  gmm_mfinal_kernel adds the chunks in ascending order and
//                        applies scikit-learn's formula.  The chunks are a function of (n, dim, K) alone.
//   gmm_colsum / colmean the float64 column means a fit centres by, in a fixed order.
//   gmm_decide_kernel    the device-side stop: iterations, lower_bound, change, converged, done.  Kernels of later iterations read
//                        `done` and return at once; the host queues max_iter iterations and never synchronises.
//
// No float atomics anywhere; the only atomics are the status bits.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kGmThreads = 256;
constexpr int kGmTileRows = 64;              // rows per workgroup of the E-step
constexpr int kGmStepComps = 256;            // components per step: four waves x 64
constexpr int kGmWaveComps = 8;              // components per wave of the M-step sums
constexpr int kGmMaxChunks = 64;             // row chunks of the M-step sums
constexpr int kGmChunkRows = 64;             // their least height
constexpr long long kGmPartCells = 1LL << 22;    // chunks * K * dim stays under this where more than one chunk is taken
constexpr int kGmMeanChunks = 256;           // row chunks of the column means
constexpr int kGmMeanChunkRows = 256;

enum { GM_ALWAYS = 0, GM_UNLESS_DONE = 1, GM_UNLESS_STOPPED = 2, GM_UNLESS_BAD = 3 };

__device__ __forceinline__ bool gm_skip(const acx_gmm_state* st, const int* status, int gate) {
    if (gate == GM_UNLESS_DONE) return st->done != 0;
    if (gate == GM_UNLESS_STOPPED) return st->done != 0 || (*status & ACX_GMM_NONFINITE) != 0;
    if (gate == GM_UNLESS_BAD) return (*status & ACX_GMM_NONFINITE) != 0;
    return false;
}

// ---- the E-step ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_rows_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                       const double* __restrict__ center, float* __restrict__ a) {
    const int q = dim >> 2;
    const long long total = n * q;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long i = e / q;
        const int c = (int)(e - i * q) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + i * ld + c);
        const double d0 = (double)v.x - (center ? center[c] : 0.0), d1 = (double)v.y - (center ? center[c + 1] : 0.0);
        const double d2 = (double)v.z - (center ? center[c + 2] : 0.0), d3 = (double)v.w - (center ? center[c + 3] : 0.0);
        float* row = a + i * 2 * dim;
        *reinterpret_cast<float4*>(row + c) = make_float4((float)(d0 * d0), (float)(d1 * d1), (float)(d2 * d2), (float)(d3 * d3));
        *reinterpret_cast<float4*>(row + dim + c) = make_float4((float)d0, (float)d1, (float)d2, (float)d3);
    }
}

__global__ __launch_bounds__(256) void gmm_prepare_kernel(const double* __restrict__ w, const double* __restrict__ mu,
                                                          const double* __restrict__ var, const double* __restrict__ center, int dim,
                                                          int spherical, float* __restrict__ b, double2* __restrict__ cst,
                                                          const acx_gmm_state* st, const int* status, int gate) {
    __shared__ double s_red[256];
    if (gm_skip(st, status, gate)) return;
    const int tid = threadIdx.x, k = blockIdx.x;
    float* row = b + (long long)k * 2 * dim;
    double sl = 0.0, sq = 0.0;
    for (int j = tid; j < dim; j += 256) {
        const double v = spherical ? var[k] : var[(long long)k * dim + j];
        const double m = mu[(long long)k * dim + j] - (center ? center[j] : 0.0);
        const double a = 1.0 / v, bb = m / v;
        row[j] = spherical ? 1.0f : (float)a;
        row[dim + j] = (float)(-2.0 * (spherical ? m : bb));
        sl += log(v);
        sq += (m * m) * a;
    }
    sl = km_block_sum<double, 256>(sl, s_red);
    sq = km_block_sum<double, 256>(sq, s_red);
    if (tid == 0)
        cst[k] = make_double2(log(w[k]) - 0.5 * ((double)dim * 1.8378770664093453 + sl + sq), spherical ? -0.5 / var[k] : -0.5);
}

struct GmEstepP {
    const float* a; long long n;             // [n][dim2]
    const float* b; const double2* cst; int K; // [K][dim2], [K] (constant, scale)
    int dim2;
    float* lpn; double* term; float* resp; long long ld_r; int* labels; int* status;
    const acx_gmm_state* st; int gate;
};

__global__ __launch_bounds__(kGmThreads, 2) void gmm_estep_kernel(GmEstepP p) {
    constexpr int QT = 2;
    __shared__ knn_key s_best[4][kGmTileRows];
    __shared__ float s_part[4][kGmTileRows];
    __shared__ float s_max[kGmTileRows];
    __shared__ float s_sum[kGmTileRows];
    if (gm_skip(p.st, p.status, p.gate)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const long long i0 = (long long)blockIdx.x * kGmTileRows;

    // rows past n / components past K repeat the last valid one: loads stay inside the buffers, results are dropped
    const float* xa[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) xa[t] = p.a + min(i0 + 32 * t + r32, p.n - 1) * p.dim2;

    // visit(t, i, u, k, lp) for every (row register, component) of this wave's share: the same bits on every sweep
    auto sweep = [&](auto visit) {
        for (int k0 = 0; k0 < p.K; k0 += kGmStepComps) {
            const int kw = k0 + wave * 64;
            if (kw >= p.K) break;                    // wave-uniform; no barrier inside the loop
            const float* cb[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) cb[u] = p.b + (long long)min(kw + 32 * u + r32, p.K - 1) * p.dim2;
            F32Tile<32>::acc_t acc[QT][2];
            dot_tile<QT>(acc, xa, cb, p.dim2, h, [](const float4 (&)[2], const float4 (&)[2]) {});
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k = kw + 32 * u + r32;
                const double2 c = p.cst[min(k, p.K - 1)];
                if (k < p.K) {
#pragma unroll
                    for (int t = 0; t < QT; ++t)
#pragma unroll
                        for (int i = 0; i < 16; ++i) visit(t, i, k, (float)fma(c.y, (double)acc[t][u][i], c.x));
                }
            }
        }
    };

    // sweep 1: the row's best key
    bool bad = false;
    {
        knn_key best[QT][16];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) best[t][i] = 0ull;
        sweep([&](int t, int i, int k, float lp) {
            if (i0 + 32 * t + F32Tile<32>::row(i, h) < p.n && acx_nonfinite(lp)) bad = true;
            const knn_key key = knn_make_key(lp, k);
            best[t][i] = key > best[t][i] ? key : best[t][i];
        });
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                knn_key v = best[t][i];
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) {
                    const knn_key w = __shfl_xor(v, o);
                    v = w > v ? w : v;
                }
                if (r32 == 0) s_best[wave][32 * t + F32Tile<32>::row(i, h)] = v;
            }
    }
    __syncthreads();
    if (tid < kGmTileRows) {
        knn_key v = s_best[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) v = s_best[w][tid] > v ? s_best[w][tid] : v;
        const float m = knn_key_score(v);
        s_max[tid] = m;
        if (p.labels && i0 + tid < p.n) p.labels[i0 + tid] = acx_nonfinite(m) ? -1 : knn_key_index(v);
    }
    __syncthreads();

    // sweep 2: s = sum_k expf(lp - m), and e to resp
    {
        float mrow[QT][16], sum[QT][16];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                mrow[t][i] = s_max[32 * t + F32Tile<32>::row(i, h)];
                sum[t][i] = 0.f;
            }
        sweep([&](int t, int i, int k, float lp) {
            const float e = expf(lp - mrow[t][i]);
            sum[t][i] += e;
            const long long row = i0 + 32 * t + F32Tile<32>::row(i, h);
            if (p.resp && row < p.n) p.resp[row * p.ld_r + k] = e;
        });
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float v = sum[t][i];
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
                if (r32 == 0) s_part[wave][32 * t + F32Tile<32>::row(i, h)] = v;
            }
    }
    __syncthreads();
    if (tid < kGmTileRows) {
        const float s = sum4(s_part[0][tid], s_part[1][tid], s_part[2][tid], s_part[3][tid]);
        s_sum[tid] = s;
        if (i0 + tid < p.n) {
            p.lpn[i0 + tid] = 0.f + (s_max[tid] + logf(s));      // -0.0 never leaves
            if (p.term) p.term[i0 + tid] = (double)s_max[tid] + log((double)s);    // what the lower bound sums: not rounded to fp32
        }
    }
    __syncthreads();                                 // also orders this workgroup's stores of e before its loads below
    if (p.resp) {
        const int rows = (int)min((long long)kGmTileRows, p.n - i0);
        for (int r = 0; r < rows; ++r) {
            float* out = p.resp + (i0 + r) * p.ld_r;
            const float s = s_sum[r];
            for (int k = tid; k < p.K; k += kGmThreads) out[k] = out[k] / s;
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(p.status, ACX_GMM_NONFINITE);
}

// *out = sum_i term[i], thread t over rows t, t + 1024, ..., then a tree
__global__ __launch_bounds__(1024) void gmm_lsum_kernel(const double* __restrict__ term, long long n, double* out,
                                                        const acx_gmm_state* st, const int* status, int gate) {
    __shared__ double s_red[1024];
    if (gm_skip(st, status, gate)) return;
    double a = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) a += term[i];
    a = km_block_sum<double, 1024>(a, s_red);
    if (threadIdx.x == 0) *out = a;
}

// ---- the M-step ------------------------------------------------------------------------------------------------------------
struct GmPart { int chunks; long long rows; };
// row chunks of the M-step sums: a function of (n, dim, K) alone
static GmPart gm_part(long long n, int dim, int K) {
    const long long cells = (long long)K * dim;
    const long long c = std::max(1LL, std::min(std::min<long long>(kGmMaxChunks, cdiv(n, kGmChunkRows)), kGmPartCells / cells));
    GmPart pt;
    pt.rows = cdiv(n, c);
    pt.chunks = (int)cdiv(n, pt.rows);
    return pt;
}
// an upper bound of chunks * K * dim, non-decreasing in each argument
static size_t gm_part_cells(long long n, int dim, int K) {
    const long long cells = (long long)K * dim;
    const long long cn = std::min<long long>(kGmMaxChunks, cdiv(n, kGmChunkRows));
    return (size_t)std::max(cells, std::min(cn * cells, kGmPartCells));
}
static GmPart gm_mean_part(long long n) {
    GmPart pt;
    pt.rows = cdiv(n, std::min<long long>(kGmMeanChunks, cdiv(n, kGmMeanChunkRows)));
    pt.chunks = (int)cdiv(n, pt.rows);
    return pt;
}

// The sums of chunk blockIdx.x over its rows in ascending order: p0[chunk][k] = sum r, p1 / p2[chunk][k][col] = sum r xc,
// sum r xc^2 with xc = (double)x - center.  Wave w of workgroup (., y, z) takes components 32 z + 8 w .. + 7, lane l columns
// 256 y + 4 l .. + 3.
__global__ __launch_bounds__(256) void gmm_msum_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                       const double* __restrict__ center, const float* __restrict__ resp,
                                                       long long ld_r, int K, long long rpc, double* __restrict__ p0,
                                                       double* __restrict__ p1, double* __restrict__ p2, const acx_gmm_state* st,
                                                       const int* status, int gate) {
    constexpr int W = kGmWaveComps;
    if (gm_skip(st, status, gate)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x, col = blockIdx.y * 256 + lane * 4;
    const int kb = (blockIdx.z * 4 + wave) * W;
    if (kb >= K) return;                             // no barrier in this kernel
    const bool on = col < dim;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    if (on && center) {
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = center[col + q];
    }
    double s0[W], s1[W][4], s2[W][4];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        s0[j] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) s1[j][q] = s2[j][q] = 0.0;
    }
    const long long lo = chunk * rpc, hi = min(n, lo + rpc);
    for (long long i = lo; i < hi; ++i) {
        const float4 v = on ? *reinterpret_cast<const float4*>(x + i * ld + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        double d[4] = {(double)v.x - c[0], (double)v.y - c[1], (double)v.z - c[2], (double)v.w - c[3]};
        double qq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) qq[q] = d[q] * d[q];
        const float* rr = resp + i * ld_r;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const double r = (double)rr[min(kb + j, K - 1)];
            s0[j] += r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s1[j][q] = fma(r, d[q], s1[j][q]);
                s2[j][q] = fma(r, qq[q], s2[j][q]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int k = kb + j;
        if (k < K) {
            const long long cell = (long long)chunk * K + k;
            if (on) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    p1[cell * dim + col + q] = s1[j][q];
                    p2[cell * dim + col + q] = s2[j][q];
                }
            }
            if (blockIdx.y == 0 && lane == 0) p0[cell] = s0[j];
        }
    }
}

// Component k from the chunks' sums in ascending chunk order: N = sum r + 10 eps, mean = S1 / N (+ center), v = S2 / N - mean^2 +
// reg_covar (spherical: their mean over the columns, by a fixed tree), w = N / n.  N < 1 sets ACX_GMM_DEGENERATE.
__global__ __launch_bounds__(256) void gmm_mfinal_kernel(const double* __restrict__ p0, const double* __restrict__ p1,
                                                         const double* __restrict__ p2, int chunks, int K, int dim, long long n,
                                                         const double* __restrict__ center, double reg, int spherical,
                                                         double* __restrict__ w, double* __restrict__ mu, double* __restrict__ var,
                                                         double* __restrict__ nk, int* status, const acx_gmm_state* st, int gate) {
    __shared__ double s_red[256];
    if (gm_skip(st, status, gate)) return;
    const int tid = threadIdx.x, k = blockIdx.x;
    double N = 0.0;
    for (int c = 0; c < chunks; ++c) N += p0[(long long)c * K + k];
    N += 10.0 * 2.220446049250313e-16;
    double vs = 0.0;
    for (int j = tid; j < dim; j += 256) {
        double a = 0.0, b = 0.0;
        for (int c = 0; c < chunks; ++c) {
            const long long e = ((long long)c * K + k) * dim + j;
            a += p1[e];
            b += p2[e];
        }
        const double m = a / N;
        const double v = (b / N - m * m) + reg;
        mu[(long long)k * dim + j] = m + (center ? center[j] : 0.0);
        if (spherical) vs += v;
        else var[(long long)k * dim + j] = v;
    }
    if (spherical) {                                 // uniform over the workgroup
        vs = km_block_sum<double, 256>(vs, s_red);
        if (tid == 0) var[k] = vs / (double)dim;
    }
    if (tid == 0) {
        w[k] = N / (double)n;
        nk[k] = N;
        if (N < 1.0) atomicOr(status, ACX_GMM_DEGENERATE);
    }
}

// ---- the fit ---------------------------------------------------------------------------------------------------------------
// part[chunk][col] = the float64 sum of the chunk's rows: row j of the chunk on wave j mod 4, the four waves joined in wave order
__global__ __launch_bounds__(256) void gmm_colsum_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                         long long rpc, double* __restrict__ part) {
    __shared__ double s_p[3][64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = blockIdx.y * 256 + lane * 4;
    const long long lo = blockIdx.x * rpc, hi = min(n, lo + rpc);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < dim) {
        for (long long i = lo + wave; i < hi; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + i * ld + col);
            a[0] += (double)v.x; a[1] += (double)v.y; a[2] += (double)v.z; a[3] += (double)v.w;
        }
    }
    if (wave) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s_p[wave - 1][lane][q] = a[q];
    }
    __syncthreads();
    if (wave == 0 && col < dim) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            part[(long long)blockIdx.x * dim + col + q] = ((a[q] + s_p[0][lane][q]) + s_p[1][lane][q]) + s_p[2][lane][q];
    }
}

__global__ __launch_bounds__(256) void gmm_colmean_kernel(const double* __restrict__ part, int chunks, int dim, long long n,
                                                          double* __restrict__ center) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= dim) return;
    double a = 0.0;
    for (int c = 0; c < chunks; ++c) a += part[(long long)c * dim + j];
    center[j] = a / (double)n;
}

__global__ void gmm_decide_kernel(acx_gmm_state* st, const double* lsum, long long n, const double* tol, const int* status) {
    if (st->done) return;
    const double lb = *lsum / (double)n;
    const double change = st->iterations == 0 ? (double)INFINITY : lb - st->lower_bound;
    const bool bad = (*status & ACX_GMM_NONFINITE) != 0;
    const bool conv = !bad && fabs(change) < *tol;
    st->iterations += 1;
    st->lower_bound = lb;
    st->change = change;
    st->converged = conv ? 1 : 0;
    st->done = (conv || bad) ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The workspace of every acx_gmm_* call, carved in this order (each piece 256-byte aligned)
struct GmWs { size_t a, b, cst, resp, term, p0, p1, p2, mean, lsum, nk, end; };
static GmWs gm_carve(long long n, int dim, int K) {
    GmWs w;
    size_t off = 0;
    w.a = off; off += align_up((size_t)n * 2 * dim * sizeof(float));
    w.b = off; off += align_up((size_t)K * 2 * dim * sizeof(float));
    w.cst = off; off += align_up((size_t)K * sizeof(double2));
    w.resp = off; off += align_up((size_t)n * K * sizeof(float));
    w.term = off; off += align_up((size_t)n * sizeof(double));
    w.p0 = off; off += align_up((size_t)kGmMaxChunks * K * sizeof(double));
    w.p1 = off; off += align_up(gm_part_cells(n, dim, K) * sizeof(double));
    w.p2 = off; off += align_up(gm_part_cells(n, dim, K) * sizeof(double));
    w.mean = off; off += align_up((size_t)kGmMeanChunks * dim * sizeof(double));
    w.lsum = off; off += align_up(sizeof(double));
    w.nk = off; off += align_up((size_t)K * sizeof(double));
    w.end = off;
    return w;
}

static int gm_check_shape(const char* who, int64_t n, int dim, int components, int covariance_type) {
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (components < 1 || components > ACX_KMEANS_MAX_CLUSTERS)
        ACX_FAIL(ACX_ERR_ARG, "%s: components = %d (expected 1 .. %d)", who, components, ACX_KMEANS_MAX_CLUSTERS);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    if (dim < 4 || dim > ACX_KNN_MAX_DIM || (dim & 3))
        ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected a multiple of 4 in 4 .. %d)", who, dim, ACX_KNN_MAX_DIM);
    if (covariance_type != ACX_GMM_DIAG && covariance_type != ACX_GMM_SPHERICAL)
        ACX_FAIL(ACX_ERR_ARG, "%s: covariance_type %d (expected ACX_GMM_DIAG or ACX_GMM_SPHERICAL)", who, covariance_type);
    return ACX_OK;
}

static int gm_check_f64(const char* who, const char* name, const void* p, bool may_be_null = false) {
    if (!p) {
        if (may_be_null) return ACX_OK;
        ACX_FAIL(ACX_ERR_ARG, "%s: %s is null", who, name);
    }
    if (reinterpret_cast<uintptr_t>(p) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: %s is not 8-byte aligned", who, name);
    return ACX_OK;
}

struct GmModel { const double* w; const double* mu; const double* var; const double* center; int K, dim, spherical; };

static void gm_launch_rows(const float* x, long long ld, long long n, int dim, const double* center, float* a, hipStream_t s) {
    const long long blocks = std::min<long long>(cdiv(n * (dim >> 2), 256), 4096);
    launch_kernel(&gmm_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, ld, n, dim, center, a);
}

// prepare + E-step + the sum of log_prob_norm, on the A operand in the workspace
static void gm_launch_estep(const GmModel& m, long long n, char* ws, const GmWs& w, float* lpn, float* resp, long long ld_r,
                            int* labels, double* lsum, int* status, const acx_gmm_state* st, int gate, hipStream_t s) {
    float* b = reinterpret_cast<float*>(ws + w.b);
    double2* cst = reinterpret_cast<double2*>(ws + w.cst);
    launch_kernel(&gmm_prepare_kernel, dim3(m.K), dim3(256), 0, s, m.w, m.mu, m.var, m.center, m.dim, m.spherical, b, cst, st,
                  (const int*)status, gate);
    GmEstepP p;
    p.a = reinterpret_cast<const float*>(ws + w.a); p.n = n; p.b = b; p.cst = cst; p.K = m.K; p.dim2 = 2 * m.dim;
    double* term = reinterpret_cast<double*>(ws + w.term);
    p.lpn = lpn; p.term = lsum ? term : nullptr; p.resp = resp; p.ld_r = ld_r; p.labels = labels; p.status = status; p.st = st; p.gate = gate;
    launch_kernel(&gmm_estep_kernel, dim3((unsigned)cdiv(n, kGmTileRows)), dim3(kGmThreads), 0, s, p);
    if (lsum) launch_kernel(&gmm_lsum_kernel, dim3(1), dim3(1024), 0, s, (const double*)term, n, lsum, st, (const int*)status, gate);
}

static void gm_launch_mstep(const float* x, long long ld, long long n, int dim, const double* center, const float* resp,
                            long long ld_r, int K, double reg, int spherical, double* wt, double* mu, double* var, double* nk,
                            char* ws, const GmWs& w, int* status, const acx_gmm_state* st, int gate, hipStream_t s) {
    const GmPart pt = gm_part(n, dim, K);
    double* p0 = reinterpret_cast<double*>(ws + w.p0);
    double* p1 = reinterpret_cast<double*>(ws + w.p1);
    double* p2 = reinterpret_cast<double*>(ws + w.p2);
    launch_kernel(&gmm_msum_kernel, dim3(pt.chunks, (dim + 255) / 256, (K + 4 * kGmWaveComps - 1) / (4 * kGmWaveComps)), dim3(256), 0, s,
                  x, ld, n, dim, center, resp, ld_r, K, pt.rows, p0, p1, p2, st, (const int*)status, gate);
    launch_kernel(&gmm_mfinal_kernel, dim3(K), dim3(256), 0, s, (const double*)p0, (const double*)p1, (const double*)p2, pt.chunks, K,
                  dim, n, center, reg, spherical, wt, mu, var, nk, status, st, gate);
}

static int gm_estep_call(const char* who, const float* x, int64_t ld_x, int64_t n, int dim, const double* center,
                         const double* weights, const double* means, const double* variances, int components, int covariance_type,
                         float* log_prob_norm, float* resp, int64_t ld_resp, int32_t* labels, double* log_prob_sum, int32_t* status,
                         void* ws, size_t ws_bytes, void* stream) {
    ACX_TRY(gm_check_shape(who, n, dim, components, covariance_type));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(gm_check_f64(who, "center", center, true));
    ACX_TRY(gm_check_f64(who, "weights", weights));
    ACX_TRY(gm_check_f64(who, "means", means));
    ACX_TRY(gm_check_f64(who, "variances", variances));
    ACX_TRY(gm_check_f64(who, "log_prob_sum", log_prob_sum));
    if (!log_prob_norm) ACX_FAIL(ACX_ERR_ARG, "%s: log_prob_norm is null", who);
    if (resp && ld_resp < components)
        ACX_FAIL(ACX_ERR_ARG, "%s: ld_resp = %lld is below the %d components", who, (long long)ld_resp, components);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const GmWs w = gm_carve(n, dim, components);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    gm_launch_rows(x, ld_x, n, dim, center, reinterpret_cast<float*>(base + w.a), s);
    GmModel m{weights, means, variances, center, components, dim, covariance_type == ACX_GMM_SPHERICAL};
    gm_launch_estep(m, n, base, w, log_prob_norm, resp, ld_resp, (int*)labels, log_prob_sum, (int*)status, nullptr, GM_ALWAYS, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_gmm_workspace_bytes(int64_t n, int dim, int components, size_t* out_bytes) {
    static const char* who = "acx_gmm_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(gm_check_shape(who, n, dim, components, ACX_GMM_DIAG));
    *out_bytes = gm_carve(n, dim, components).end;
    return ACX_OK;
}

int acx_gmm_estep(const float* x, int64_t ld_x, int64_t n, int dim, const double* center, const double* weights, const double* means,
                  const double* variances, int components, int covariance_type, float* log_prob_norm, float* resp, int64_t ld_resp,
                  int32_t* labels, double* log_prob_sum, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    return gm_estep_call("acx_gmm_estep", x, ld_x, n, dim, center, weights, means, variances, components, covariance_type,
                         log_prob_norm, resp, ld_resp, labels, log_prob_sum, status, ws, ws_bytes, stream);
}

int acx_gmm_score(const float* x, int64_t ld_x, int64_t n, int dim, const double* center, const double* weights, const double* means,
                  const double* variances, int components, int covariance_type, float* log_prob_norm, int32_t* labels,
                  double* log_prob_sum, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    return gm_estep_call("acx_gmm_score", x, ld_x, n, dim, center, weights, means, variances, components, covariance_type,
                         log_prob_norm, nullptr, 0, labels, log_prob_sum, status, ws, ws_bytes, stream);
}

int acx_gmm_mstep(const float* x, int64_t ld_x, int64_t n, int dim, const double* center, const float* resp, int64_t ld_resp,
                  int components, double reg_covar, int covariance_type, double* weights, double* means, double* variances,
                  double* nk, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_gmm_mstep";
    ACX_TRY(gm_check_shape(who, n, dim, components, covariance_type));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(gm_check_f64(who, "center", center, true));
    if (!resp) ACX_FAIL(ACX_ERR_ARG, "%s: resp is null", who);
    if (ld_resp < components) ACX_FAIL(ACX_ERR_ARG, "%s: ld_resp = %lld is below the %d components", who, (long long)ld_resp, components);
    if (!(reg_covar >= 0.0)) ACX_FAIL(ACX_ERR_ARG, "%s: reg_covar = %g (expected >= 0)", who, reg_covar);
    ACX_TRY(gm_check_f64(who, "weights", weights));
    ACX_TRY(gm_check_f64(who, "means", means));
    ACX_TRY(gm_check_f64(who, "variances", variances));
    ACX_TRY(gm_check_f64(who, "nk", nk));
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const GmWs w = gm_carve(n, dim, components);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    gm_launch_mstep(x, ld_x, n, dim, center, resp, ld_resp, components, reg_covar, covariance_type == ACX_GMM_SPHERICAL, weights, means,
                    variances, nk, static_cast<char*>(ws), w, (int*)status, nullptr, GM_ALWAYS, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_gmm_fit(const float* x, int64_t ld_x, int64_t n, int dim, double* weights, double* means, double* variances, int components,
                int covariance_type, int max_iter, const double* tol, double reg_covar, double* center, int32_t* labels,
                float* log_prob_norm, acx_gmm_state* state, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_gmm_fit";
    ACX_TRY(gm_check_shape(who, n, dim, components, covariance_type));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(gm_check_f64(who, "weights", weights));
    ACX_TRY(gm_check_f64(who, "means", means));
    ACX_TRY(gm_check_f64(who, "variances", variances));
    if (max_iter < 1 || max_iter > ACX_KMEANS_MAX_ITER)
        ACX_FAIL(ACX_ERR_ARG, "%s: max_iter = %d (expected 1 .. %d)", who, max_iter, ACX_KMEANS_MAX_ITER);
    ACX_TRY(gm_check_f64(who, "tol", tol));
    if (!(reg_covar >= 0.0)) ACX_FAIL(ACX_ERR_ARG, "%s: reg_covar = %g (expected >= 0)", who, reg_covar);
    ACX_TRY(gm_check_f64(who, "center", center));
    if (!labels || !log_prob_norm) ACX_FAIL(ACX_ERR_ARG, "%s: labels / log_prob_norm is null", who);
    ACX_TRY(gm_check_f64(who, "state", state));
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const GmWs w = gm_carve(n, dim, components);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    const int spherical = covariance_type == ACX_GMM_SPHERICAL;
    float* resp = reinterpret_cast<float*>(base + w.resp);
    double* lsum = reinterpret_cast<double*>(base + w.lsum);
    double* nk = reinterpret_cast<double*>(base + w.nk);
    double* mpart = reinterpret_cast<double*>(base + w.mean);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(state, 0, sizeof(acx_gmm_state), s));
    const GmPart mp = gm_mean_part(n);
    launch_kernel(&gmm_colsum_kernel, dim3(mp.chunks, (dim + 255) / 256), dim3(256), 0, s, x, (long long)ld_x, (long long)n, dim, mp.rows,
                  mpart);
    launch_kernel(&gmm_colmean_kernel, dim3((dim + 255) / 256), dim3(256), 0, s, (const double*)mpart, mp.chunks, dim, (long long)n,
                  center);
    gm_launch_rows(x, ld_x, n, dim, center, reinterpret_cast<float*>(base + w.a), s);
    GmModel m{weights, means, variances, center, components, dim, spherical};
    for (int it = 0; it < max_iter; ++it) {
        gm_launch_estep(m, n, base, w, log_prob_norm, resp, components, (int*)labels, lsum, (int*)status, state, GM_UNLESS_DONE, s);
        gm_launch_mstep(x, ld_x, n, dim, center, resp, components, components, reg_covar, spherical, weights, means, variances, nk, base,
                        w, (int*)status, state, GM_UNLESS_STOPPED, s);
        launch_kernel(&gmm_decide_kernel, dim3(1), dim3(1), 0, s, state, (const double*)lsum, (long long)n, tol, (const int*)status);
    }
    // labels and log_prob_norm belong to the returned parameters: the closing E-step, unless a non-finite density kept the last
    // M-step from running
    gm_launch_estep(m, n, base, w, log_prob_norm, nullptr, 0, (int*)labels, nullptr, (int*)status, state, GM_UNLESS_BAD, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
