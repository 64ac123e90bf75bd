// Cluster validation (acx_silhouette, acx_cluster_dispersion, acx_contingency in include/acx.h): what tells a good clustering from
// a bad one and picks k, computed where the embeddings and the labels already are.
//
//   the partition            kmeans_hist / scan / scatter (kmeans.hip): counts, start offsets and the row indices sorted stably by
//                            label.  Every sum below runs over PARTITION POSITIONS: cluster c owns positions start[c] ..
//                            start[c] + counts[c] - 1, ascending row index inside it.
//   cluster_rowsq_kernel     xx[i] = sum x_i^2 in fp32 (row_sumsq + wave_sum, device_common.h): one fixed order per row.
//   silhouette_tile_kernel   a WAVE owns 64 queried rows and streams a range of partition positions, 64 columns per step: the
//                            64 x 64 tile of dot products comes from dot_tile (device_common.h: a pair's dot product has the bits
//                            the search and the assignment give it), becomes distances in the accumulator registers and goes to
//                            LDS; then lane r walks row r's 64 columns in ascending position, adding into ONE running float64 and
//                            flushing it at each cluster boundary (the boundaries are wave-uniform: every row walks the same
//                            columns).  The four waves of a workgroup stream the same columns for four row tiles, so the column
//                            loads of three of them hit the cache.  The positions are cut into `ns` ranges (blockIdx.y) to fill
//                            the machine; a cluster that spans ranges leaves one partial per range, slot c + range of the
//                            workspace (c + range is unique along the staircase).  Neither the n x n distances nor the n x K sums
//                            of whole clusters exist anywhere else.
//   silhouette_row_kernel    one thread per queried row: S(i, c) = the range partials in ascending range, then a, b, nearest, s.
//   silhouette_mean_kernel   workgroup c: the mean of s over the queried rows of label c; workgroup K: over all of them.
//   cluster_disp_kernel      workgroup c: the float64 mean of cluster c, then sum (x - mean)^2 per row by direct float64
//                            differences (one wave per row), added over the cluster's rows in partition order.
//   contingency_kernel       table[a_i][b_i] += 1 (64-bit integer atomics: they commute).
//
// No float atomics; f32 / f64 arithmetic only (no packed FP32: the Makefile builds this file with -fno-slp-vectorize, and with
// -ffp-contract=off, so every fused multiply-add below is one that is spelled out).
#include <cfloat>
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

static_assert(ACX_CLUSTER_BAD_LABEL == ACX_KMEANS_BAD_LABEL, "the partition's histogram kernel sets the k-means bit");

constexpr int kSilRowsPerWave = 64;
constexpr int kSilRowsPerGroup = 256;        // four waves, four row tiles
constexpr int kSilStep = 64;                 // partition positions per step
constexpr int kSilPitch = 65;                // floats per LDS row of a wave's distance tile: lane r reads bank (r + col) % 64
constexpr int kSilMaxSplits = ACX_CLUSTER_MAX_SPLITS;
constexpr int kSilTargetGroups = 512;        // workgroups wanted: two per compute unit

// The ranges of partition positions: a function of (n, n_rows) alone (include/acx.h states it)
struct SilGeom { int ns; long long len; };
static SilGeom sil_geom(long long n, long long n_rows) {
    const long long chunks = cdiv(n, kSilStep), groups = cdiv(n_rows, kSilRowsPerGroup);
    long long ns = std::min<long long>(kSilMaxSplits, std::max<long long>(1, cdiv(kSilTargetGroups, groups)));
    ns = std::min(ns, chunks);
    SilGeom g;
    g.len = kSilStep * cdiv(chunks, ns);
    g.ns = (int)cdiv(n, g.len);
    return g;
}

__device__ __forceinline__ bool cs_nonfinite(double v) { return !(fabs(v) <= DBL_MAX); }

__global__ __launch_bounds__(256) void cluster_rowsq_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                            float* __restrict__ xx) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float s = wave_sum(row_sumsq(x + row * ld, dim, lane, [](const float4&) {}));
    if (lane == 0) xx[row] = s;
}

struct SilP {
    const float* x; long long ld; long long n; int dim, cosine;
    const float* rowc;                        // per row: xx (Euclidean) or the inverse norm (cosine)
    int K; const int* rows; long long n_rows;
    const int* perm; const int* start; const int* counts;
    double* sp; long long len;
};

__global__ __launch_bounds__(256, 2) void silhouette_tile_kernel(SilP p) {
    constexpr int QT = 2;
    __shared__ float s_d[4][kSilRowsPerWave * kSilPitch];
    __shared__ int s_q[4][kSilRowsPerWave];
    __shared__ float s_c[4][kSilRowsPerWave];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const int K = p.K, split = blockIdx.y;
    const long long npart = (long long)p.start[K - 1] + p.counts[K - 1];
    const long long lo = (long long)split * p.len, hi = min(npart, lo + p.len);
    if (lo >= hi) return;                            // uniform over the workgroup

    // this lane's queried row; a tile row past n_rows or with an index outside [0, n) computes on row 0 and is never written
    const long long q = (long long)blockIdx.x * kSilRowsPerGroup + wave * kSilRowsPerWave + lane;
    int qi = -1;
    if (q < p.n_rows) {
        qi = p.rows ? p.rows[q] : (int)q;
        if ((unsigned)qi >= (unsigned)p.n) qi = -1;
    }
    s_q[wave][lane] = qi;
    s_c[wave][lane] = p.rowc[max(qi, 0)];
    __syncthreads();
    const float* xa[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) xa[t] = p.x + (long long)max(s_q[wave][32 * t + r32], 0) * p.ld;

    // the cluster that holds position lo: the last one whose start is <= lo (an empty cluster shares its start with the next)
    int cur = 0;
    {
        int a = 0, b = K - 1;
        while (a < b) {
            const int m = (a + b + 1) >> 1;
            if (p.start[m] <= lo) a = m; else b = m - 1;
        }
        cur = a;
    }
    long long cend = (long long)p.start[cur] + p.counts[cur];
    double run = 0.0;
    float* tile = s_d[wave];

    for (long long p0 = lo; p0 < hi; p0 += kSilStep) {
        int j[2];
        const float* cb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            j[u] = p.perm[min(p0 + 32 * u + r32, hi - 1)];     // past the range: its last column again, never walked
            cb[u] = p.x + (long long)j[u] * p.ld;
        }
        F32Tile<32>::acc_t acc[QT][2];
        dot_tile<QT>(acc, xa, cb, p.dim, h, [](const float4 (&)[2], const float4 (&)[2]) {});
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float cj = p.rowc[j[u]];
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = 32 * t + F32Tile<32>::row(i, h);
                    const float ci = s_c[wave][row];
                    float d;
                    if (p.cosine) {
                        d = 1.f - cos_scale(acc[t][u][i], ci, cj);
                    } else {
                        const float v = __builtin_fmaf(-2.f, acc[t][u][i], ci + cj);
                        d = sqrtf(v < 0.f ? 0.f : v);                // a NaN stays a NaN
                    }
                    if (s_q[wave][row] == j[u]) d = 0.f;             // the pair (i, i), by position
                    tile[row * kSilPitch + 32 * u + r32] = d;
                }
        }
        __syncthreads();
        const int cn = (int)min((long long)kSilStep, hi - p0);
        int c0 = 0;
        while (c0 < cn) {                                            // wave-uniform: cur, cend, c0
            const int ce = (int)min((long long)cn, cend - p0);
            const float* tr = tile + lane * kSilPitch;
#ifdef ACX_SIL_LAB_NO_WALK                                           // tools/lab/build_silhouette_lab.sh: one column per segment
            run += (double)tr[c0];
#else
            for (int c = c0; c < ce; ++c) run += (double)tr[c];
#endif
            c0 = ce;
            if (p0 + ce == cend) {                                   // the cluster ends inside this range
                if (qi >= 0) p.sp[(long long)(cur + split) * p.n_rows + q] = run;
                run = 0.0;
                do { ++cur; } while (cur < K && p.counts[cur] == 0);
                cend = cur < K ? (long long)p.start[cur] + p.counts[cur] : (long long)1 << 62;
            }
        }
        __syncthreads();
    }
    // the cluster the range ends in, if it goes on in the next one
    if (cur < K && p.start[cur] < hi && qi >= 0) p.sp[(long long)(cur + split) * p.n_rows + q] = run;
}

struct SilRowP {
    const float* xx; const int* labels; long long n; int K;
    const int* rows; long long n_rows;
    const int* start; const int* counts; const double* sp; long long len;
    double* a; double* b; int* nearest; double* s; int* ql; int* status;
};

__global__ __launch_bounds__(256) void silhouette_row_kernel(SilRowP p) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.n_rows) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int flags = 0;
    int qi = p.rows ? p.rows[q] : (int)q;
    int L = -1;
    if ((unsigned)qi >= (unsigned)p.n) flags |= ACX_CLUSTER_BAD_ROW;
    else {
        L = p.labels[qi];
        if ((unsigned)L >= (unsigned)p.K) { L = -1; flags |= ACX_CLUSTER_BAD_LABEL; }
    }
    double a = nan, b = nan, s = nan;
    int nearest = -1;
    if (L >= 0) {
        bool bad = acx_nonfinite(p.xx[qi]);
        double own = 0.0, best = 0.0;
        int nonempty = 0;
        for (int c = 0; c < p.K; ++c) {
            const int cnt = p.counts[c];
            if (cnt == 0) continue;
            ++nonempty;
            const long long first = p.start[c];
            const int s_lo = (int)(first / p.len), s_hi = (int)((first + cnt - 1) / p.len);
            double S = p.sp[(long long)(c + s_lo) * p.n_rows + q];
            for (int r = s_lo + 1; r <= s_hi; ++r) S += p.sp[(long long)(c + r) * p.n_rows + q];
            if (cs_nonfinite(S)) bad = true;
            if (c == L) own = S;
            else {
                const double m = S / (double)cnt;
                if (nearest < 0 || m < best) { best = m; nearest = c; }     // the lowest c wins a tie
            }
        }
        const int cl = p.counts[L];
        if (bad) {
            flags |= ACX_CLUSTER_NONFINITE;
            nearest = -1;
        } else {
            a = cl > 1 ? own / (double)(cl - 1) : 0.0;
            if (nonempty < 2) {
                flags |= ACX_CLUSTER_DEGENERATE;
                s = 0.0;
            } else {
                b = best;
                const double mx = fmax(a, b);
                s = (cl == 1 || mx == 0.0) ? 0.0 : (b - a) / mx;
            }
        }
    }
    p.a[q] = a; p.b[q] = b; p.s[q] = s; p.nearest[q] = nearest;
    p.ql[q] = L;
    if (flags) atomicOr(p.status, flags);
}

// workgroup c < K: cluster_mean[c]; workgroup K: *mean.  Thread t adds rows t, t + 256, ... in ascending order, then the tree
__global__ __launch_bounds__(256) void silhouette_mean_kernel(const double* __restrict__ s, const int* __restrict__ ql, long long n_rows,
                                                              int K, double* cluster_mean, double* mean) {
    __shared__ double s_red[256];
    __shared__ long long s_cnt[256];
    const int c = blockIdx.x;
    if (c < K && !cluster_mean) return;
    double acc = 0.0;
    long long cnt = 0;
    for (long long q = threadIdx.x; q < n_rows; q += 256) {
        const int l = ql[q];
        if (c < K ? l == c : l >= 0) { acc += s[q]; ++cnt; }
    }
    acc = km_block_sum<double, 256>(acc, s_red);
    cnt = km_block_sum<long long, 256>(cnt, s_cnt);
    if (threadIdx.x == 0) (c < K ? cluster_mean[c] : *mean) = acc / (double)cnt;       // no rows: 0 / 0 = NaN
}

// ---- dispersion ------------------------------------------------------------------------------------------------------------
// Workgroup k.  means[k] = sums[k] / count; per row v = sum_j (x_j - mean_j)^2: lane l takes the columns 4 l .. 4 l + 3, + 256, ...
// in ascending order by v = v + d * d (two roundings), the lanes join by wave_sum; row j of the cluster runs on wave j mod 4, which
// adds v (within_sq) and sqrt(v) (within_dist) in ascending j; the waves join as ((w0 + w1) + w2) + w3.
__global__ __launch_bounds__(256) void cluster_disp_kernel(const float* __restrict__ x, long long ld, int dim, const int* __restrict__ perm,
                                                           const int* __restrict__ start, const int* __restrict__ counts,
                                                           const double* __restrict__ sums, long long* __restrict__ counts64,
                                                           double* means, double* __restrict__ within_sq,
                                                           double* __restrict__ within_dist, int* status) {
    __shared__ double s_p[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x;
    const int cnt = counts[k], s0 = start[k];
    double* mk = means + (long long)k * dim;
    for (int j = tid; j < dim; j += 256) mk[j] = cnt ? sums[(long long)k * dim + j] / (double)cnt : 0.0;
    if (tid == 0) counts64[k] = cnt;
    __syncthreads();
    double wsq = 0.0, wd = 0.0;
    bool bad = false;
    for (int j = wave; j < cnt; j += 4) {
        const float* xr = x + (long long)perm[s0 + j] * ld;
        double v = 0.0;
        for (int col = lane * 4; col < dim; col += 256) {
            const float4 f = *reinterpret_cast<const float4*>(xr + col);
            const double d0 = (double)f.x - mk[col], d1 = (double)f.y - mk[col + 1];
            const double d2 = (double)f.z - mk[col + 2], d3 = (double)f.w - mk[col + 3];
            v = v + d0 * d0; v = v + d1 * d1; v = v + d2 * d2; v = v + d3 * d3;
        }
        v = wave_sum(v);
        if (cs_nonfinite(v)) bad = true;
        wsq += v;
        wd += sqrt(v);
    }
    if (lane == 0) { s_p[wave][0] = wsq; s_p[wave][1] = wd; }
    __syncthreads();
    if (tid == 0) {
        within_sq[k] = ((s_p[0][0] + s_p[1][0]) + s_p[2][0]) + s_p[3][0];
        within_dist[k] = ((s_p[0][1] + s_p[1][1]) + s_p[2][1]) + s_p[3][1];
    }
    if (bad && lane == 0) atomicOr(status, ACX_CLUSTER_NONFINITE);
}

// grand_mean[j] = (sum_k sums[k][j], ascending k) / rows in a cluster; fewer than two non-empty clusters: ACX_CLUSTER_DEGENERATE
__global__ __launch_bounds__(256) void cluster_grand_kernel(const double* __restrict__ sums, const int* __restrict__ counts, int K, int dim,
                                                            double* __restrict__ grand, int* status) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    long long total = 0;
    int nonempty = 0;
    for (int k = 0; k < K; ++k) { total += counts[k]; nonempty += counts[k] != 0; }
    if (j == 0 && nonempty < 2) atomicOr(status, ACX_CLUSTER_DEGENERATE);
    if (j >= dim) return;
    double a = 0.0;
    for (int k = 0; k < K; ++k)
        if (counts[k]) a += sums[(long long)k * dim + j];
    grand[j] = a / (double)total;
}

// ---- contingency -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void contingency_kernel(const int* __restrict__ a, int ka, const int* __restrict__ b, int kb, long long n,
                                                          unsigned long long* table, int* status) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int la = a[i], lb = b[i];
        if ((unsigned)la < (unsigned)ka && (unsigned)lb < (unsigned)kb) atomicAdd(table + (long long)la * kb + lb, 1ull);
        else bad = true;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, ACX_CLUSTER_BAD_LABEL);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int cs_check_shape(const char* who, int64_t n, int clusters) {
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (clusters < 1 || clusters > ACX_KMEANS_MAX_CLUSTERS)
        ACX_FAIL(ACX_ERR_ARG, "%s: clusters = %d (expected 1 .. %d)", who, clusters, ACX_KMEANS_MAX_CLUSTERS);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    return ACX_OK;
}

// The workspace, carved in this order (each piece 256-byte aligned); sp holds (K + max splits) slots of n_rows <= n doubles
struct CsWs { size_t hist, start, counts, perm, xx, ql, sums, sp, end; };
static CsWs cs_carve(long long n, int dim, int K) {
    CsWs w;
    size_t off = 0;
    w.hist = off; off += km_hist_bytes(n, K);
    w.start = off; off += align_up((size_t)K * sizeof(int));
    w.counts = off; off += align_up((size_t)K * sizeof(int));
    w.perm = off; off += align_up((size_t)n * sizeof(int));
    w.xx = off; off += align_up((size_t)n * sizeof(float));
    w.ql = off; off += align_up((size_t)n * sizeof(int));
    w.sums = off; off += align_up((size_t)K * dim * sizeof(double));
    w.sp = off; off += align_up((size_t)(K + kSilMaxSplits) * (size_t)n * sizeof(double));
    w.end = off;
    return w;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_cluster_scores_workspace_bytes(int64_t n, int dim, int clusters, size_t* out_bytes) {
    static const char* who = "acx_cluster_scores_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(cs_check_shape(who, n, clusters));
    if (dim < 4 || dim > ACX_KNN_MAX_DIM || (dim & 3))
        ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected a multiple of 4 in 4 .. %d)", who, dim, ACX_KNN_MAX_DIM);
    *out_bytes = cs_carve(n, dim, clusters).end;
    return ACX_OK;
}

int acx_silhouette(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric, const int32_t* labels,
                   int clusters, const int32_t* rows, int64_t n_rows, double* a, double* b, int32_t* nearest, double* s,
                   double* cluster_mean, double* mean, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_silhouette";
    ACX_TRY(cs_check_shape(who, n, clusters));
    if (metric != ACX_KMEANS_EUCLIDEAN && metric != ACX_KMEANS_COSINE)
        ACX_FAIL(ACX_ERR_ARG, "%s: metric %d (expected ACX_KMEANS_EUCLIDEAN or ACX_KMEANS_COSINE)", who, metric);
    if (metric == ACX_KMEANS_COSINE && !x_inv_norm) ACX_FAIL(ACX_ERR_ARG, "%s: x_inv_norm is null with ACX_KMEANS_COSINE", who);
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!rows) n_rows = n;
    if (n_rows < 1 || n_rows > n) ACX_FAIL(ACX_ERR_ARG, "%s: n_rows = %lld (expected 1 .. n = %lld)", who, (long long)n_rows, (long long)n);
    if (!a || !b || !nearest || !s) ACX_FAIL(ACX_ERR_ARG, "%s: a / b / nearest / s is null", who);
    if (!mean) ACX_FAIL(ACX_ERR_ARG, "%s: mean is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const CsWs w = cs_carve(n, dim, clusters);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    int* start = reinterpret_cast<int*>(base + w.start);
    int* counts = reinterpret_cast<int*>(base + w.counts);
    int* perm = reinterpret_cast<int*>(base + w.perm);
    float* xx = reinterpret_cast<float*>(base + w.xx);
    int* ql = reinterpret_cast<int*>(base + w.ql);
    double* sp = reinterpret_cast<double*>(base + w.sp);
    const bool cosine = metric == ACX_KMEANS_COSINE;
    const SilGeom g = sil_geom(n, n_rows);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    km_launch_partition((const int*)labels, n, clusters, reinterpret_cast<int*>(base + w.hist), counts, start, perm, (int*)status, st);
    launch_kernel(&cluster_rowsq_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, x, (long long)ld_x, (long long)n, dim, xx);
    SilP p;
    p.x = x; p.ld = ld_x; p.n = n; p.dim = dim; p.cosine = cosine; p.rowc = cosine ? x_inv_norm : xx;
    p.K = clusters; p.rows = (const int*)rows; p.n_rows = n_rows; p.perm = perm; p.start = start; p.counts = counts;
    p.sp = sp; p.len = g.len;
    launch_kernel(&silhouette_tile_kernel, dim3((unsigned)cdiv(n_rows, kSilRowsPerGroup), g.ns), dim3(256), 0, st, p);
    SilRowP r;
    r.xx = xx; r.labels = (const int*)labels; r.n = n; r.K = clusters; r.rows = (const int*)rows; r.n_rows = n_rows;
    r.start = start; r.counts = counts; r.sp = sp; r.len = g.len;
    r.a = a; r.b = b; r.nearest = (int*)nearest; r.s = s; r.ql = ql; r.status = (int*)status;
    launch_kernel(&silhouette_row_kernel, dim3((unsigned)cdiv(n_rows, 256)), dim3(256), 0, st, r);
    launch_kernel(&silhouette_mean_kernel, dim3(clusters + 1), dim3(256), 0, st, (const double*)s, (const int*)ql, (long long)n_rows,
                  clusters, cluster_mean, mean);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_cluster_dispersion(const float* x, int64_t ld_x, int64_t n, int dim, const int32_t* labels, int clusters, int64_t* counts,
                           double* means, double* within_sq, double* within_dist, double* grand_mean, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream) {
    static const char* who = "acx_cluster_dispersion";
    ACX_TRY(cs_check_shape(who, n, clusters));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!counts || !means) ACX_FAIL(ACX_ERR_ARG, "%s: counts / means is null", who);
    if (!within_sq || !within_dist) ACX_FAIL(ACX_ERR_ARG, "%s: within_sq / within_dist is null", who);
    if (!grand_mean) ACX_FAIL(ACX_ERR_ARG, "%s: grand_mean is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const CsWs w = cs_carve(n, dim, clusters);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    int* start = reinterpret_cast<int*>(base + w.start);
    int* cnt = reinterpret_cast<int*>(base + w.counts);
    int* perm = reinterpret_cast<int*>(base + w.perm);
    double* sums = reinterpret_cast<double*>(base + w.sums);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    km_launch_partition((const int*)labels, n, clusters, reinterpret_cast<int*>(base + w.hist), cnt, start, perm, (int*)status, st);
    km_launch_sums(x, ld_x, dim, clusters, perm, start, cnt, sums, st);
    launch_kernel(&cluster_disp_kernel, dim3(clusters), dim3(256), 0, st, x, (long long)ld_x, dim, (const int*)perm, (const int*)start,
                  (const int*)cnt, (const double*)sums, (long long*)counts, means, within_sq, within_dist, (int*)status);
    launch_kernel(&cluster_grand_kernel, dim3((dim + 255) / 256), dim3(256), 0, st, (const double*)sums, (const int*)cnt, clusters, dim,
                  grand_mean, (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_contingency(const int32_t* a, int ka, const int32_t* b, int kb, int64_t n, int64_t* table, int32_t* status, void* stream) {
    static const char* who = "acx_contingency";
    if (!a || !b) ACX_FAIL(ACX_ERR_ARG, "%s: a / b is null", who);
    if (ka < 1 || kb < 1) ACX_FAIL(ACX_ERR_ARG, "%s: ka = %d, kb = %d (expected >= 1)", who, ka, kb);
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    if ((long long)ka * kb > ACX_CONTINGENCY_MAX_CELLS)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: ka * kb = %lld (at most 2^24 cells)", who, (long long)ka * kb);
    if (!table) ACX_FAIL(ACX_ERR_ARG, "%s: table is null", who);
    if (reinterpret_cast<uintptr_t>(table) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: table is not 8-byte aligned", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    hipStream_t st = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    ACX_HIP(hipMemsetAsync(table, 0, (size_t)ka * kb * sizeof(int64_t), st));
    launch_kernel(&contingency_kernel, dim3((unsigned)std::min<long long>(cdiv(n, 256), 4096)), dim3(256), 0, st, (const int*)a, ka,
                  (const int*)b, kb, (long long)n, reinterpret_cast<unsigned long long*>(table), (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
