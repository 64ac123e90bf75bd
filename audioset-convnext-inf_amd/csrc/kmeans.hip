// K-means over embeddings (acx_kmeans_* in include/acx.h): Lloyd iterations with k-means++ seeding, everything on the device.
//
//   kmeans_assign_kernel    a workgroup owns 64 rows and streams all K centres, 256 per step: each of the four waves forms the
//                           64 x 64 tile of dot products of its 64 centres on the f32 matrix cores by dot_tile
//                           (device_common.h, which states the bit contract: the function knn_search_kernel calls, so a
//                           pair's dot product has the search's bits) and sums c^2 of its centres from the same operand
//                           registers.  score = fma(-2, dot, cc) (cosine: -dot).  Every accumulator register keeps ONE running
//                           key knn_make_key(-score, k): lowest score, then lowest centre index, -0.0 as +0.0.  The keys of a
//                           row are joined by lane shuffles and through LDS by max -- a total order, so the label does not
//                           depend on how the centres arrived.  The n x K scores never go to memory.
//   kmeans_hist / scan / scatter   the stable partition of the row indices by label: histograms per block of rows, exclusive
//                           sums, and a scatter by one wave per block that keeps ascending row order inside a cluster.
//   kmeans_sum_kernel       (cluster, 256 columns): float64 sums over the cluster's rows in partition order, rows j = w mod 4
//                           on wave w, the four waves joined in wave order: a function of (n, dim, labels) alone.
//   kmeans_finalize_kernel  the new centre (mean, or the renormalised weighted mean), and the cluster's squared shift.
//   kmeans_decide_kernel    the device-side stop: iterations, changed, shift, done.  Kernels of later iterations read `done` and
//                           return at once; the host queues max_iter iterations and never synchronises.
//   kmeans_mindist / bsum / pick   k-means++: d_i <- min(d_i, dist(x_i, newest centre)) with the exact maximum, integer weights
//                           q_i = floor(d_i 2^(30 - e)), uint64 sums, and the smallest row whose inclusive prefix exceeds
//                           t = min(floor(u total), total - 1).  Integer arithmetic after the quantisation: order-independent.
//
// No float atomics anywhere; the integer atomics (changed count, LDS histograms, the maximum of non-negative floats through
// their bit patterns, status bits) commute.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kKmThreads = 256;
constexpr int kKmTileRows = 64;              // rows per workgroup of the assignment
constexpr int kKmStepCentres = 256;          // centres per step: four waves x 64
constexpr int kKmMaxBlocks = 1024;           // row blocks of the partition and of the sampler
constexpr int kKmBlockRows = 1024;           // their least height
constexpr int kKmDistRows = 16;              // rows per wave of the seeding distance pass

enum { KM_ALWAYS = 0, KM_UNLESS_DONE = 1, KM_IF_MOVED = 2 };

__device__ __forceinline__ bool km_skip(const acx_kmeans_state* st, int gate) {
    if (gate == KM_UNLESS_DONE) return st->done != 0;
    if (gate == KM_IF_MOVED) return !(st->shift != 0.0);
    return false;
}

// ---- assignment ------------------------------------------------------------------------------------------------------------
struct KmAssignP {
    const float* x; long long ld_x; long long n;
    const float* c; long long ld_c; int K;
    int dim, cosine;
    const int* prev; int* labels; float* scores; int* changed; int* status;
    const acx_kmeans_state* st; int gate;
};

__global__ __launch_bounds__(kKmThreads, 2) void kmeans_assign_kernel(KmAssignP p) {
    constexpr int QT = 2;
    __shared__ knn_key s_best[4][kKmTileRows];
    if (km_skip(p.st, p.gate)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const long long i0 = (long long)blockIdx.x * kKmTileRows;

    // rows past n / centres past K repeat the last valid one: loads stay inside the buffers, results are dropped
    const float* xa[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) xa[t] = p.x + min(i0 + 32 * t + r32, p.n - 1) * p.ld_x;
    bool bad = false;
    knn_key best[QT][16];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) best[t][i] = 0ull;

    for (int k0 = 0; k0 < p.K; k0 += kKmStepCentres) {
        const int kw = k0 + wave * 64;
        if (kw >= p.K) break;                        // wave-uniform; no barrier inside the loop
        const float* cb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) cb[u] = p.c + (long long)min(kw + 32 * u + r32, p.K - 1) * p.ld_c;
        F32Tile<32>::acc_t acc[QT][2];
        float cs[2] = {0.f, 0.f};                    // this lane half's share of sum c^2 of its two centres, in column order
        dot_tile<QT>(acc, xa, cb, p.dim, h, [&](const float4 (&b0)[2], const float4 (&b1)[2]) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int c = 0; c < 4; ++c) cs[u] = __builtin_fmaf(b0[u][c], b0[u][c], cs[u]);
#pragma unroll
                for (int c = 0; c < 4; ++c) cs[u] = __builtin_fmaf(b1[u][c], b1[u][c], cs[u]);
            }
        });
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float cc = cs[u] + __shfl_xor(cs[u], 32);           // the two halves of the centre's row: a + b = b + a
            const int k = kw + 32 * u + r32;
            if (k < p.K) {
#pragma unroll
                for (int t = 0; t < QT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float a = acc[t][u][i];
                        const float s = p.cosine ? -a : __builtin_fmaf(-2.f, a, cc);
                        if (i0 + 32 * t + F32Tile<32>::row(i, h) < p.n && acx_nonfinite(s)) bad = true;
                        const knn_key key = knn_make_key(-s, k);
                        best[t][i] = key > best[t][i] ? key : best[t][i];
                    }
            }
        }
    }

    // the row's best key: over the 32 lanes of its lane half, then over the four waves
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
    __syncthreads();
    if (tid < kKmTileRows) {
        const long long row = i0 + tid;
        int chg = 0;
        if (row < p.n) {
            knn_key v = s_best[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) v = s_best[w][tid] > v ? s_best[w][tid] : v;
            const float score = 0.f - knn_key_score(v);          // -0.0 never leaves
            const int label = acx_nonfinite(score) ? -1 : knn_key_index(v);
            chg = p.prev ? (p.prev[row] != label) : 1;
            p.labels[row] = label;
            p.scores[row] = score;
        }
        const int cnt = __popcll(__ballot(chg));
        if (lane == 0 && cnt) atomicAdd(p.changed, cnt);
    }
    if (__ballot(bad) && lane == 0) atomicOr(p.status, ACX_KMEANS_NONFINITE);
}

// xx[i] = sum x^2 of row i in float64 (one wave per row, fixed order)
__global__ __launch_bounds__(256) void kmeans_rowsq_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                           double* __restrict__ xx) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + row * ld;
    double s = 0.0;
    for (int k = lane * 4; k < dim; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + k);
        s = fma((double)v.x, (double)v.x, s);
        s = fma((double)v.y, (double)v.y, s);
        s = fma((double)v.z, (double)v.z, s);
        s = fma((double)v.w, (double)v.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) xx[row] = s;
}

// inertia = sum_i max(xx_i + score_i, 0) (cosine: 1 + score_i rx_i) in float64, thread t over rows t, t + 1024, ..., then a tree
__global__ __launch_bounds__(1024) void kmeans_inertia_kernel(const float* __restrict__ scores, const double* __restrict__ xx,
                                                              const float* __restrict__ rx, long long n, int cosine,
                                                              acx_kmeans_state* st) {
    __shared__ double s_red[1024];
    double a = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        const double s = (double)scores[i];
        a += cosine ? 1.0 + s * (double)rx[i] : fmax(xx[i] + s, 0.0);
    }
    a = km_block_sum<double, 1024>(a, s_red);
    if (threadIdx.x == 0) st->inertia = a;
}

__global__ __launch_bounds__(256) void kmeans_poison_kernel(int* labels, long long n, const int* status) {
    if (!(*status & ACX_KMEANS_NONFINITE)) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) labels[i] = -1;
}

// ---- the centre update -----------------------------------------------------------------------------------------------------
struct KmPart { int nb; long long rpb; };
static int km_max_blocks(long long n) { return (int)std::min<long long>(kKmMaxBlocks, cdiv(n, kKmBlockRows)); }
// row blocks of n rows: at most km_max_blocks(n) blocks of rpb rows
static KmPart km_part(long long n) {
    KmPart pt;
    pt.rpb = cdiv(n, km_max_blocks(n));
    pt.nb = (int)cdiv(n, pt.rpb);
    return pt;
}

__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int* __restrict__ labels, long long n, int K, long long rpb,
                                                          int* __restrict__ hist, int* status, int flag_bad,
                                                          const acx_kmeans_state* st, int gate) {
    __shared__ int s_h[ACX_KMEANS_MAX_CLUSTERS];
    if (km_skip(st, gate)) return;
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += 256) s_h[k] = 0;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * rpb, hi = min(n, lo + rpb);
    bool bad = false;
    for (long long i = lo + tid; i < hi; i += 256) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)K) atomicAdd(&s_h[l], 1);
        else bad = true;
    }
    __syncthreads();
    for (int k = tid; k < K; k += 256) hist[(long long)blockIdx.x * K + k] = s_h[k];
    if (flag_bad && __ballot(bad) && (tid & 63) == 0) atomicOr(status, ACX_KMEANS_BAD_LABEL);
}

// hist[b][k] <- rows of cluster k in the blocks before b; counts[k]; start[k] = rows of the clusters before k.  One workgroup.
__global__ __launch_bounds__(1024) void kmeans_scan_kernel(int* __restrict__ hist, int nb, int K, int* __restrict__ counts,
                                                           int* __restrict__ start, const acx_kmeans_state* st, int gate) {
    __shared__ int s_c[ACX_KMEANS_MAX_CLUSTERS];
    __shared__ int s_s[1024];
    if (km_skip(st, gate)) return;
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += 1024) {
        int run = 0;
        for (int b = 0; b < nb; ++b) {
            const int v = hist[(long long)b * K + k];
            hist[(long long)b * K + k] = run;
            run += v;
        }
        s_c[k] = run;
        counts[k] = run;
    }
    __syncthreads();
    int loc[4], sum = 0;                             // clusters 4 tid .. 4 tid + 3
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * tid + j;
        loc[j] = k < K ? s_c[k] : 0;
        sum += loc[j];
    }
    s_s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int t = tid >= o ? s_s[tid - o] : 0;
        __syncthreads();
        s_s[tid] += t;
        __syncthreads();
    }
    int run = s_s[tid] - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * tid + j;
        if (k < K) start[k] = run;
        run += loc[j];
    }
}

// One wave per block of rows, 64 rows at a time: a row's place is its cluster's cursor + the rows of the same label on the
// lanes below (ballots over the label's bits), so a cluster's rows stay in ascending order.
__global__ __launch_bounds__(64) void kmeans_scatter_kernel(const int* __restrict__ labels, long long n, int K, long long rpb,
                                                            const int* __restrict__ hist, const int* __restrict__ start,
                                                            int* __restrict__ perm, int nbits, const acx_kmeans_state* st,
                                                            int gate) {
    __shared__ int s_cur[ACX_KMEANS_MAX_CLUSTERS];
    if (km_skip(st, gate)) return;
    const int lane = threadIdx.x;
    for (int k = lane; k < K; k += 64) s_cur[k] = start[k] + hist[(long long)blockIdx.x * K + k];
    __syncthreads();
    const long long lo = (long long)blockIdx.x * rpb, hi = min(n, lo + rpb);
    for (long long base = lo; base < hi; base += 64) {
        const long long i = base + lane;
        const int l = i < hi ? labels[i] : -1;
        const bool ok = (unsigned)l < (unsigned)K;
        unsigned long long m = __ballot(ok);
        for (int bit = 0; bit < nbits; ++bit) {
            const bool one = (l >> bit) & 1;
            const unsigned long long b = __ballot(ok && one);
            m &= one ? b : ~b;
        }
        const int rank = __popcll(m & ((1ull << lane) - 1ull)), cnt = __popcll(m);
        if (ok) {
            const long long pos = (long long)s_cur[l] + rank;
            if (pos < n) perm[pos] = (int)i;
        }
        __syncthreads();
        if (ok && rank == cnt - 1) s_cur[l] += cnt;
        __syncthreads();
    }
}

// sums[k][col .. col + 3] of cluster k over its rows in partition order: row j of the cluster on wave j mod 4
__global__ __launch_bounds__(256) void kmeans_sum_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ rx,
                                                         const int* __restrict__ perm, const int* __restrict__ start,
                                                         const int* __restrict__ counts, int dim, double* __restrict__ sums,
                                                         const acx_kmeans_state* st, int gate) {
    __shared__ double s_p[3][64][4];
    if (km_skip(st, gate)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x, col = blockIdx.y * 256 + lane * 4;
    const int cnt = counts[k], s0 = start[k];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (col < dim) {
        for (int j = wave; j < cnt; j += 4) {
            const long long i = perm[s0 + j];
            const float4 v = *reinterpret_cast<const float4*>(x + i * ld + col);
            if (rx) {
                const double w = (double)rx[i];                  // float x float is exact in float64
                a0 += (double)v.x * w; a1 += (double)v.y * w; a2 += (double)v.z * w; a3 += (double)v.w * w;
            } else {
                a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
            }
        }
    }
    if (wave) { s_p[wave - 1][lane][0] = a0; s_p[wave - 1][lane][1] = a1; s_p[wave - 1][lane][2] = a2; s_p[wave - 1][lane][3] = a3; }
    __syncthreads();
    if (wave == 0 && col < dim) {
        double* out = sums + (long long)k * dim + col;
        out[0] = ((a0 + s_p[0][lane][0]) + s_p[1][lane][0]) + s_p[2][lane][0];
        out[1] = ((a1 + s_p[0][lane][1]) + s_p[1][lane][1]) + s_p[2][lane][1];
        out[2] = ((a2 + s_p[0][lane][2]) + s_p[1][lane][2]) + s_p[2][lane][2];
        out[3] = ((a3 + s_p[0][lane][3]) + s_p[1][lane][3]) + s_p[2][lane][3];
    }
}

// c_k <- (float)(sum / count), or (float)(sum / |sum|) for the cosine metric; shiftk[k] = |c_new - c_old|^2 in float64.  An
// empty cluster (or a weighted sum of length 0) keeps its centre.
__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const double* __restrict__ sums, const int* __restrict__ counts,
                                                              int dim, int cosine, float* __restrict__ c, long long ld_c,
                                                              double* __restrict__ shiftk, const acx_kmeans_state* st, int gate) {
    __shared__ double s_red[256];
    if (km_skip(st, gate)) return;
    const int tid = threadIdx.x, k = blockIdx.x;
    const int cnt = counts[k];
    const double* sk = sums + (long long)k * dim;
    double div = (double)cnt;
    if (cosine && cnt > 0) {
        double q = 0.0;
        for (int j = tid; j < dim; j += 256) q = fma(sk[j], sk[j], q);
        q = km_block_sum<double, 256>(q, s_red);
        div = sqrt(q);
    }
    if (cnt == 0 || !(div > 0.0)) {                  // uniform over the workgroup
        if (tid == 0) shiftk[k] = 0.0;
        return;
    }
    double sh = 0.0;
    for (int j = tid; j < dim; j += 256) {
        const float f = (float)(sk[j] / div);
        const double d = (double)f - (double)c[k * ld_c + j];
        sh = fma(d, d, sh);
        c[k * ld_c + j] = f;
    }
    sh = km_block_sum<double, 256>(sh, s_red);
    if (tid == 0) shiftk[k] = sh;
}

// *shift = sum_k shiftk[k] in a fixed order
__global__ __launch_bounds__(256) void kmeans_shift_kernel(const double* __restrict__ shiftk, int K, double* shift) {
    __shared__ double s_red[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) a += shiftk[k];
    a = km_block_sum<double, 256>(a, s_red);
    if (threadIdx.x == 0) *shift = a;
}

__global__ __launch_bounds__(256) void kmeans_decide_kernel(acx_kmeans_state* st, int* changed, const double* __restrict__ shiftk,
                                                            int K, const double* tol, const int* status) {
    __shared__ double s_red[256];
    if (st->done) return;                            // read by every thread before the first barrier below
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) a += shiftk[k];
    a = km_block_sum<double, 256>(a, s_red);
    if (threadIdx.x == 0) {
        const int ch = *changed;
        st->iterations += 1;
        st->changed = ch;
        st->shift = a;
        st->done = (ch == 0 || a <= *tol || (*status & ACX_KMEANS_NONFINITE)) ? 1 : 0;
        *changed = 0;
    }
}

// ---- seeding ---------------------------------------------------------------------------------------------------------------
// d_i <- min(d_i, dist(x_i, c)) (first: d_i <- dist), one wave per row, kKmDistRows rows per wave; *dmax <- max over the rows
// (bit patterns of non-negative floats order as the floats).  c = row *pick of x when pick is given.
__global__ __launch_bounds__(256) void kmeans_mindist_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ rx,
                                                             long long n, int dim, int cosine, const float* c, const int* pick,
                                                             int first, float* __restrict__ d, unsigned* dmax, int* status) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pick) c = x + (long long)min(max(*pick, 0), (int)(n - 1)) * ld;
    const float rc = cosine ? inv_norm_of(wave_sum(row_sumsq(c, dim, lane, [](const float4&) {}))) : 0.f;
    float mx = 0.f;
    bool bad = false;
    for (int r = 0; r < kKmDistRows; ++r) {
        const long long row = wv * kKmDistRows + r;
        if (row >= n) break;
        const float* xr = x + row * ld;
        float s = 0.f;
        for (int k = lane * 4; k < dim; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(xr + k);
            const float4 w = *reinterpret_cast<const float4*>(c + k);
            if (cosine) {
                s = __builtin_fmaf(v.x, w.x, s); s = __builtin_fmaf(v.y, w.y, s);
                s = __builtin_fmaf(v.z, w.z, s); s = __builtin_fmaf(v.w, w.w, s);
            } else {
                const float t0 = v.x - w.x, t1 = v.y - w.y, t2 = v.z - w.z, t3 = v.w - w.w;
                s = __builtin_fmaf(t0, t0, s); s = __builtin_fmaf(t1, t1, s);
                s = __builtin_fmaf(t2, t2, s); s = __builtin_fmaf(t3, t3, s);
            }
        }
        s = wave_sum(s);
        float dist = s;
        if (cosine) dist = fmaxf(__builtin_fmaf(-2.f, cos_scale(s, rx[row], rc), 2.f), 0.f);
        if (!(dist <= kF32Max)) bad = true;
        const float nd = first ? dist : fminf(d[row], dist);
        if (lane == 0) d[row] = nd;
        mx = fmaxf(mx, nd);
    }
    if (lane == 0 && mx > 0.f) atomicMax(dmax, __float_as_uint(mx));
    if (bad && lane == 0) atomicOr(status, ACX_KMEANS_NONFINITE);
}

// q = floor(d 2^sh) < 2^31 for 0 <= d <= the maximum the shift was taken from
__device__ __forceinline__ unsigned long long km_quant(float d, int sh) {
    const float v = ldexpf(d, sh);
    return v >= 1.f ? (unsigned long long)fminf(v, 2147483520.f) : 0ull;
}
__device__ __forceinline__ int km_shift_of(unsigned dmax_bits) {
    const float m = __uint_as_float(dmax_bits);
    return (m > 0.f && m <= kF32Max) ? 30 - ilogbf(m) : 0;
}

__global__ __launch_bounds__(256) void kmeans_bsum_kernel(const float* __restrict__ d, long long n, long long rpb,
                                                          const unsigned* dmax, unsigned long long* __restrict__ bsum) {
    __shared__ unsigned long long s_red[256];
    const unsigned mb = *dmax;
    const int sh = km_shift_of(mb);
    const long long lo = (long long)blockIdx.x * rpb, hi = min(n, lo + rpb);
    unsigned long long a = 0ull;
    if (mb) for (long long i = lo + threadIdx.x; i < hi; i += 256) a += km_quant(d[i], sh);
    a = km_block_sum<unsigned long long, 256>(a, s_red);
    if (threadIdx.x == 0) bsum[blockIdx.x] = a;
}

// The smallest row whose inclusive prefix sum of q exceeds t = min(floor(u total), total - 1): first the block of rows (a scan of
// the block sums), then the row inside it.  total == 0: the lowest row index not among chosen[0 .. nchosen) (-1 without
// `chosen`) and ACX_KMEANS_DEGENERATE.  One workgroup.
__global__ __launch_bounds__(1024) void kmeans_pick_kernel(const float* __restrict__ d, long long n, long long rpb, int nb,
                                                           const unsigned* dmax, const unsigned long long* __restrict__ bsum,
                                                           const double* u, int* picked, const int* chosen, int nchosen,
                                                           int* status) {
    __shared__ unsigned long long s_a[1024];
    __shared__ unsigned long long s_t;
    __shared__ int s_sel;
    const int tid = threadIdx.x;
    auto scan = [&](unsigned long long v) {          // inclusive, over the 1024 threads
        __syncthreads();
        s_a[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const unsigned long long t = tid >= o ? s_a[tid - o] : 0ull;
            __syncthreads();
            s_a[tid] += t;
            __syncthreads();
        }
        return s_a[tid];
    };
    const unsigned long long v = tid < nb ? bsum[tid] : 0ull;
    const unsigned long long incl = scan(v);
    const unsigned long long total = s_a[1023];
    if (total == 0ull) {
        int c = -1;
        if (chosen) {
            for (c = 0; c < nchosen; ++c) {
                int hit = 0;
                for (int j = tid; j < nchosen; j += 1024) hit |= chosen[j] == c;
                if (!__syncthreads_or(hit)) break;
            }
        }
        if (tid == 0) {
            *picked = c;
            atomicOr(status, ACX_KMEANS_DEGENERATE);
        }
        return;
    }
    unsigned long long t = (unsigned long long)floor(__dmul_rn(*u, (double)total));
    t = t < total - 1 ? t : total - 1;
    if (tid == 0) s_sel = -1;
    __syncthreads();
    if (tid < nb && incl - v <= t && t < incl) { s_sel = tid; s_t = t - (incl - v); }
    __syncthreads();
    const int b = s_sel;
    if (b < 0) return;                               // cannot happen: t < total
    const unsigned long long tr = s_t;
    const int sh = km_shift_of(*dmax);
    const long long lo = (long long)b * rpb, hi = min(n, lo + rpb);
    const long long seg = (hi - lo + 1023) / 1024;
    const long long a = min(hi, lo + tid * seg), e = min(hi, a + seg);
    unsigned long long loc = 0ull;
    for (long long i = a; i < e; ++i) loc += km_quant(d[i], sh);
    const unsigned long long inc2 = scan(loc);
    if (inc2 - loc <= tr && tr < inc2) {
        unsigned long long run = inc2 - loc;
        for (long long i = a; i < e; ++i) {
            run += km_quant(d[i], sh);
            if (run > tr) { *picked = (int)i; break; }
        }
    }
}

__global__ void kmeans_first_kernel(const double* u, long long n, int* picked) {
    const long long i = (long long)floor(__dmul_rn(*u, (double)n));
    *picked = (int)(i < 0 ? 0 : i < n - 1 ? i : n - 1);
}

// centres[k] = row picked[k] of x (cosine: times its inverse norm)
__global__ __launch_bounds__(256) void kmeans_gather_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ rx,
                                                            long long n, int dim, const int* __restrict__ picked,
                                                            float* __restrict__ c, long long ld_c) {
    const int k = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    if (j >= dim) return;
    const long long i = min(max(picked[k], 0), (int)(n - 1));
    const float v = x[i * ld + j];
    c[k * ld_c + j] = rx ? v * rx[i] : v;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int km_check_shape(const char* who, int64_t n, int clusters, bool need_k_le_n = true) {
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (clusters < 1 || clusters > ACX_KMEANS_MAX_CLUSTERS)
        ACX_FAIL(ACX_ERR_ARG, "%s: clusters = %d (expected 1 .. %d)", who, clusters, ACX_KMEANS_MAX_CLUSTERS);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    if (need_k_le_n && clusters > n) ACX_FAIL(ACX_ERR_ARG, "%s: clusters = %d exceeds the %lld rows", who, clusters, (long long)n);
    return ACX_OK;
}

static int km_check_metric(const char* who, int metric, const float* x_inv_norm) {
    if (metric != ACX_KMEANS_EUCLIDEAN && metric != ACX_KMEANS_COSINE)
        ACX_FAIL(ACX_ERR_ARG, "%s: metric %d (expected ACX_KMEANS_EUCLIDEAN or ACX_KMEANS_COSINE)", who, metric);
    if (metric == ACX_KMEANS_COSINE && !x_inv_norm) ACX_FAIL(ACX_ERR_ARG, "%s: x_inv_norm is null with ACX_KMEANS_COSINE", who);
    return ACX_OK;
}

// The workspace of a fit / an update / a seeding, carved in this order (each piece 256-byte aligned)
struct KmWs { size_t hist, start, perm, sums, shiftk, xx, scores, changed, d, dmax, bsum, end; };
static KmWs km_carve(long long n, int dim, int K) {
    KmWs w;
    size_t off = 0;
    w.hist = off; off += align_up((size_t)km_max_blocks(n) * K * sizeof(int));
    w.start = off; off += align_up((size_t)K * sizeof(int));
    w.perm = off; off += align_up((size_t)n * sizeof(int));
    w.sums = off; off += align_up((size_t)K * dim * sizeof(double));
    w.shiftk = off; off += align_up((size_t)K * sizeof(double));
    w.xx = off; off += align_up((size_t)n * sizeof(double));
    w.scores = off; off += align_up((size_t)n * sizeof(float));
    w.changed = off; off += align_up(2 * sizeof(int));
    w.d = off; off += align_up((size_t)n * sizeof(float));
    w.dmax = off; off += align_up((size_t)K * sizeof(unsigned));
    w.bsum = off; off += align_up((size_t)kKmMaxBlocks * sizeof(unsigned long long));
    w.end = off;
    return w;
}

struct KmData {
    const float* x; long long ld_x; const float* rx; long long n; int dim, K, cosine;
    float* c; long long ld_c;
};

static void km_launch_assign(const KmData& v, const int* prev, int* labels, float* scores, int* changed, int* status,
                             const acx_kmeans_state* st, int gate, hipStream_t s) {
    KmAssignP p;
    p.x = v.x; p.ld_x = v.ld_x; p.n = v.n; p.c = v.c; p.ld_c = v.ld_c; p.K = v.K; p.dim = v.dim; p.cosine = v.cosine;
    p.prev = prev; p.labels = labels; p.scores = scores; p.changed = changed; p.status = status; p.st = st; p.gate = gate;
    launch_kernel(&kmeans_assign_kernel, dim3((unsigned)cdiv(v.n, kKmTileRows)), dim3(kKmThreads), 0, s, p);
}

static int km_bits(int K) {
    int b = 0;
    while ((1 << b) < K) ++b;
    return b;
}

// counts (and, with `centres`, the mean step) from labels
static void km_launch_update(const KmData& v, const int* labels, int* counts, char* ws, const KmWs& w, int* status, int flag_bad,
                             bool centres, const acx_kmeans_state* st, int gate, hipStream_t s) {
    const KmPart pt = km_part(v.n);
    int* hist = reinterpret_cast<int*>(ws + w.hist);
    int* start = reinterpret_cast<int*>(ws + w.start);
    int* perm = reinterpret_cast<int*>(ws + w.perm);
    double* sums = reinterpret_cast<double*>(ws + w.sums);
    double* shiftk = reinterpret_cast<double*>(ws + w.shiftk);
    launch_kernel(&kmeans_hist_kernel, dim3(pt.nb), dim3(256), 0, s, labels, v.n, v.K, pt.rpb, hist, status, flag_bad, st, gate);
    launch_kernel(&kmeans_scan_kernel, dim3(1), dim3(1024), 0, s, hist, pt.nb, v.K, counts, start, st, gate);
    if (!centres) return;
    launch_kernel(&kmeans_scatter_kernel, dim3(pt.nb), dim3(64), 0, s, labels, v.n, v.K, pt.rpb, (const int*)hist, (const int*)start,
                  perm, km_bits(v.K), st, gate);
    launch_kernel(&kmeans_sum_kernel, dim3(v.K, (v.dim + 255) / 256), dim3(256), 0, s, v.x, v.ld_x, v.cosine ? v.rx : nullptr,
                  (const int*)perm, (const int*)start, (const int*)counts, v.dim, sums, st, gate);
    launch_kernel(&kmeans_finalize_kernel, dim3(v.K), dim3(256), 0, s, (const double*)sums, (const int*)counts, v.dim, v.cosine, v.c,
                  v.ld_c, shiftk, st, gate);
}

// The partition and the per-cluster sums for cluster_scores.hip (prototypes in acx_internal.h): the kernels above, ungated.
size_t km_hist_bytes(long long n, int K) { return align_up((size_t)km_max_blocks(n) * K * sizeof(int)); }

void km_launch_partition(const int* labels, long long n, int K, int* hist, int* counts, int* start, int* perm, int* status,
                         hipStream_t s) {
    const KmPart pt = km_part(n);
    launch_kernel(&kmeans_hist_kernel, dim3(pt.nb), dim3(256), 0, s, labels, n, K, pt.rpb, hist, status, 1, (const acx_kmeans_state*)nullptr,
                  (int)KM_ALWAYS);
    launch_kernel(&kmeans_scan_kernel, dim3(1), dim3(1024), 0, s, hist, pt.nb, K, counts, start, (const acx_kmeans_state*)nullptr,
                  (int)KM_ALWAYS);
    launch_kernel(&kmeans_scatter_kernel, dim3(pt.nb), dim3(64), 0, s, labels, n, K, pt.rpb, (const int*)hist, (const int*)start, perm,
                  km_bits(K), (const acx_kmeans_state*)nullptr, (int)KM_ALWAYS);
}

void km_launch_sums(const float* x, long long ld_x, int dim, int K, const int* perm, const int* start, const int* counts, double* sums,
                    hipStream_t s) {
    launch_kernel(&kmeans_sum_kernel, dim3(K, (dim + 255) / 256), dim3(256), 0, s, x, ld_x, (const float*)nullptr, perm, start, counts,
                  dim, sums, (const acx_kmeans_state*)nullptr, (int)KM_ALWAYS);
}

static void km_launch_mindist(const KmData& v, const float* c, const int* pick, int first, float* d, unsigned* dmax, int* status,
                              hipStream_t s) {
    launch_kernel(&kmeans_mindist_kernel, dim3((unsigned)cdiv(v.n, 4 * kKmDistRows)), dim3(256), 0, s, v.x, v.ld_x, v.rx, v.n, v.dim,
                  v.cosine, c, pick, first, d, dmax, status);
}

static void km_launch_sample(const float* d, long long n, const unsigned* dmax, const double* u, int* picked, const int* chosen,
                             int nchosen, unsigned long long* bsum, int* status, hipStream_t s) {
    const KmPart pt = km_part(n);
    launch_kernel(&kmeans_bsum_kernel, dim3(pt.nb), dim3(256), 0, s, d, n, pt.rpb, dmax, bsum);
    launch_kernel(&kmeans_pick_kernel, dim3(1), dim3(1024), 0, s, d, n, pt.rpb, pt.nb, dmax, (const unsigned long long*)bsum, u, picked,
                  chosen, nchosen, status);
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_kmeans_workspace_bytes(int64_t n, int dim, int clusters, size_t* out_bytes) {
    static const char* who = "acx_kmeans_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(km_check_shape(who, n, clusters, false));
    if (dim < 4 || dim > ACX_KNN_MAX_DIM || (dim & 3))
        ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected a multiple of 4 in 4 .. %d)", who, dim, ACX_KNN_MAX_DIM);
    *out_bytes = km_carve(n, dim, clusters).end;
    return ACX_OK;
}

int acx_kmeans_assign(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, const float* centers, int64_t ld_c,
                      int clusters, int dim, int metric, const int32_t* prev_labels, int32_t* labels, float* scores,
                      int32_t* changed, int32_t* status, void* stream) {
    static const char* who = "acx_kmeans_assign";
    ACX_TRY(km_check_shape(who, n, clusters, false));
    ACX_TRY(km_check_metric(who, metric, x_inv_norm));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(check_f32_rows(who, "centers", centers, ld_c, dim));
    if (!labels || !scores) ACX_FAIL(ACX_ERR_ARG, "%s: labels / scores is null", who);
    if (!changed) ACX_FAIL(ACX_ERR_ARG, "%s: changed is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t), s));
    KmData v{x, ld_x, x_inv_norm, n, dim, clusters, metric == ACX_KMEANS_COSINE, const_cast<float*>(centers), ld_c};
    km_launch_assign(v, (const int*)prev_labels, (int*)labels, scores, (int*)changed, (int*)status, nullptr, KM_ALWAYS, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_kmeans_update(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric, const int32_t* labels,
                      int clusters, float* centers, int64_t ld_c, int32_t* counts, double* shift, int32_t* status, void* ws,
                      size_t ws_bytes, void* stream) {
    static const char* who = "acx_kmeans_update";
    ACX_TRY(km_check_shape(who, n, clusters, false));
    ACX_TRY(km_check_metric(who, metric, x_inv_norm));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(check_f32_rows(who, "centers", centers, ld_c, dim));
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!counts || !shift) ACX_FAIL(ACX_ERR_ARG, "%s: counts / shift is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const KmWs w = km_carve(n, dim, clusters);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    KmData v{x, ld_x, x_inv_norm, n, dim, clusters, metric == ACX_KMEANS_COSINE, centers, ld_c};
    char* base = static_cast<char*>(ws);
    km_launch_update(v, (const int*)labels, (int*)counts, base, w, (int*)status, 1, true, nullptr, KM_ALWAYS, s);
    launch_kernel(&kmeans_shift_kernel, dim3(1), dim3(256), 0, s, (const double*)(base + w.shiftk), clusters, shift);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_kmeans_fit(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric, float* centers,
                   int64_t ld_c, int clusters, int max_iter, const double* tol_abs, int32_t* labels, int32_t* counts,
                   acx_kmeans_state* state, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_kmeans_fit";
    ACX_TRY(km_check_shape(who, n, clusters));
    ACX_TRY(km_check_metric(who, metric, x_inv_norm));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(check_f32_rows(who, "centers", centers, ld_c, dim));
    if (max_iter < 1 || max_iter > ACX_KMEANS_MAX_ITER)
        ACX_FAIL(ACX_ERR_ARG, "%s: max_iter = %d (expected 1 .. %d)", who, max_iter, ACX_KMEANS_MAX_ITER);
    if (!tol_abs) ACX_FAIL(ACX_ERR_ARG, "%s: tol_abs is null", who);
    if (!labels || !counts) ACX_FAIL(ACX_ERR_ARG, "%s: labels / counts is null", who);
    if (!state) ACX_FAIL(ACX_ERR_ARG, "%s: state is null", who);
    if (reinterpret_cast<uintptr_t>(state) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: state is not 8-byte aligned", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const KmWs w = km_carve(n, dim, clusters);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    const bool cosine = metric == ACX_KMEANS_COSINE;
    KmData v{x, ld_x, x_inv_norm, n, dim, clusters, cosine, centers, ld_c};
    float* scores = reinterpret_cast<float*>(base + w.scores);
    double* xx = reinterpret_cast<double*>(base + w.xx);
    int* changed = reinterpret_cast<int*>(base + w.changed);
    const double* shiftk = reinterpret_cast<const double*>(base + w.shiftk);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(state, 0, sizeof(acx_kmeans_state), s));
    ACX_HIP(hipMemsetAsync(changed, 0, 2 * sizeof(int), s));
    ACX_HIP(hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(int32_t), s));       // every row counts as changed in iteration 1
    if (!cosine) launch_kernel(&kmeans_rowsq_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, s, x, (long long)ld_x, (long long)n, dim, xx);
    for (int it = 0; it < max_iter; ++it) {
        km_launch_assign(v, (const int*)labels, (int*)labels, scores, changed, (int*)status, state, KM_UNLESS_DONE, s);
        km_launch_update(v, (const int*)labels, (int*)counts, base, w, (int*)status, 0, true, state, KM_UNLESS_DONE, s);
        launch_kernel(&kmeans_decide_kernel, dim3(1), dim3(256), 0, s, state, changed, shiftk, clusters, tol_abs, (const int*)status);
    }
    // labels, counts and inertia belong to the returned centres: one more assignment if the last update moved a centre
    km_launch_assign(v, (const int*)labels, (int*)labels, scores, changed + 1, (int*)status, state, KM_IF_MOVED, s);
    launch_kernel(&kmeans_poison_kernel, dim3((unsigned)std::min<long long>(cdiv(n, 256), 1024)), dim3(256), 0, s, (int*)labels,
                  (long long)n, (const int*)status);
    km_launch_update(v, (const int*)labels, (int*)counts, base, w, (int*)status, 0, false, nullptr, KM_ALWAYS, s);
    launch_kernel(&kmeans_inertia_kernel, dim3(1), dim3(1024), 0, s, (const float*)scores, (const double*)xx, x_inv_norm, (long long)n,
                  (int)cosine, state);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_kmeans_min_distance(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric,
                            const float* center, int first, float* d, float* d_max, int32_t* status, void* stream) {
    static const char* who = "acx_kmeans_min_distance";
    ACX_TRY(km_check_shape(who, n, 1));
    ACX_TRY(km_check_metric(who, metric, x_inv_norm));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(check_f32_rows(who, "center", center, dim, dim));
    if (!d || !d_max) ACX_FAIL(ACX_ERR_ARG, "%s: d / d_max is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(d_max, 0, sizeof(float), s));
    KmData v{x, ld_x, x_inv_norm, n, dim, 1, metric == ACX_KMEANS_COSINE, nullptr, 0};
    km_launch_mindist(v, center, nullptr, first ? 1 : 0, d, reinterpret_cast<unsigned*>(d_max), (int*)status, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_kmeans_sample(const float* d, int64_t n, const float* d_max, const double* u, int32_t* picked, int32_t* status, void* ws,
                      size_t ws_bytes, void* stream) {
    static const char* who = "acx_kmeans_sample";
    ACX_TRY(km_check_shape(who, n, 1));
    if (!d || !d_max) ACX_FAIL(ACX_ERR_ARG, "%s: d / d_max is null", who);
    if (!u) ACX_FAIL(ACX_ERR_ARG, "%s: u is null", who);
    if (reinterpret_cast<uintptr_t>(u) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: u is not 8-byte aligned", who);
    if (!picked) ACX_FAIL(ACX_ERR_ARG, "%s: picked is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    ACX_TRY(check_workspace(ws, ws_bytes, align_up((size_t)kKmMaxBlocks * sizeof(unsigned long long))));
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    km_launch_sample(d, n, reinterpret_cast<const unsigned*>(d_max), u, (int*)picked, nullptr, 0, static_cast<unsigned long long*>(ws),
                     (int*)status, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_kmeans_seed(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric, int clusters,
                    const double* u, int32_t* picked, float* centers, int64_t ld_c, int32_t* status, void* ws, size_t ws_bytes,
                    void* stream) {
    static const char* who = "acx_kmeans_seed";
    ACX_TRY(km_check_shape(who, n, clusters));
    ACX_TRY(km_check_metric(who, metric, x_inv_norm));
    ACX_TRY(check_f32_rows(who, "x", x, ld_x, dim));
    ACX_TRY(check_f32_rows(who, "centers", centers, ld_c, dim));
    if (!u) ACX_FAIL(ACX_ERR_ARG, "%s: u is null", who);
    if (reinterpret_cast<uintptr_t>(u) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: u is not 8-byte aligned", who);
    if (!picked) ACX_FAIL(ACX_ERR_ARG, "%s: picked is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const KmWs w = km_carve(n, dim, clusters);
    ACX_TRY(check_workspace(ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    float* d = reinterpret_cast<float*>(base + w.d);
    unsigned* dmax = reinterpret_cast<unsigned*>(base + w.dmax);
    unsigned long long* bsum = reinterpret_cast<unsigned long long*>(base + w.bsum);
    const bool cosine = metric == ACX_KMEANS_COSINE;
    KmData v{x, ld_x, x_inv_norm, n, dim, clusters, cosine, centers, ld_c};
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(dmax, 0, (size_t)clusters * sizeof(unsigned), s));
    launch_kernel(&kmeans_first_kernel, dim3(1), dim3(1), 0, s, u, (long long)n, (int*)picked);
    for (int r = 1; r < clusters; ++r) {
        km_launch_mindist(v, nullptr, (const int*)picked + (r - 1), r == 1, d, dmax + r, (int*)status, s);
        km_launch_sample(d, n, dmax + r, u + r, (int*)picked + r, (const int*)picked, r, bsum, (int*)status, s);
    }
    launch_kernel(&kmeans_gather_kernel, dim3(clusters, (dim + 255) / 256), dim3(256), 0, s, x, (long long)ld_x, cosine ? x_inv_norm : nullptr, (long long)n,
                  dim, (const int*)picked, centers, (long long)ld_c);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
