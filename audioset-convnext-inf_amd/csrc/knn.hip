// Nearest-neighbour search over embeddings (acx_knn_row_norms / acx_knn_search / acx_knn_vote, include/acx.h): the k best
// database rows per query by dot product or cosine, and kNN tagging from the neighbours' targets.
//
//   knn_norm_kernel    r[i] = 1 / sqrt(sum x^2) per row (one wave per row, fixed order), 0 for a zero row.
//   knn_search_kernel  grid (query tiles, slices).  A workgroup owns TQ = 32 or 64 queries and one slice of the database, which
//                      it streams once in steps of 256 rows: each of the four waves forms the TQ x 64 score tile of its 64 rows
//                      on the f32 matrix cores (v_mfma_f32_32x32x2_f32, operands straight from global memory: a lane reads
//                      32 contiguous bytes of its row per 16 columns of the contraction) and filters it against the queries'
//                      thresholds into per-query candidate buffers in LDS.  The scores never go to memory.
//   knn_merge_kernel   one wave per query: the k best out of the slices' lists, decoded to indices / scores.
//   knn_vote_kernel    out[q][c] = sum_j w_j y[idx[q][j]][c] / sum_j w_j, a gather.
//
// Order.  A candidate is ONE 64-bit key: the order-preserving image of its fp32 score (-0.0 taken as +0.0) in the high word,
// the complemented database index in the low word.  Larger key = better neighbour: score descending, then index ascending, and
// no two keys are equal.  Key 0 is "no candidate" (no finite score and index < 2^30 maps to it).  Everything below selects on
// keys, so the result is the first k of that one total order whatever the arrival order of the LDS atomics was.
//
// Keeping the top k.  Query q of the tile has CAP = 64 R slots (R = 1, 2, 4 for k <= 32, 64, 128: CAP >= 2 k), a count and a
// threshold key (the k-th best so far, 0 until k candidates were seen).  A score whose key beats the threshold takes a slot by
// an LDS atomic on the count.  When a query runs out of slots the workgroup stops (the block-wide OR of __syncthreads_or), one
// wave per full query sorts its CAP keys in registers (bitonic network over lane shuffles, no barrier inside), keeps the first
// k and raises the threshold, and the lanes whose candidates found no slot try again against the new threshold.  On random data
// the threshold soon rejects almost everything and trims are rare; on adversarial data (every score beats the last) there is
// one trim per CAP - k rows, and the result is the same.
//
// Bits.  The contraction of a (query, row) pair is dot_tile's (device_common.h, which states the contract): the whole of `dim`
// inside one wave, in an order that depends on `dim` alone, whatever the pair's position in its tile, the tile's in the grid,
// nq, n, k or the number of slices: the same pair has the same score bits everywhere, and in kmeans_assign_kernel too.  Cosine
// scores are cos_scale(acc, rq[i], rd[j]), two roundings.  A non-finite accumulator (a NaN or inf in Q or D always gives one,
// as every query meets every row) sets ACX_KNN_NONFINITE, and the merge then writes index -1 / score NaN everywhere.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"
#include "knn_common.h"

namespace acx {

// kKnn* constants, knn_sort_desc, knn_load_sorted and the launch plan: knn_common.h (knn_i8.hip searches with the same machinery;
// its kernel takes the slot / trim / slice-list steps below from there as functions)
// knn_key, knn_make_key, knn_key_score, knn_key_index: device_common.h (classify.hip orders classes by the same keys)

__global__ __launch_bounds__(256) void knn_norm_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                       float* __restrict__ inv_norm, int* status) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + row * ld;
    bool bad = false;
    const float s = wave_sum(row_sumsq(xr, dim, lane, [&](const float4& v) {
        bad |= acx_nonfinite(v.x) || acx_nonfinite(v.y) || acx_nonfinite(v.z) || acx_nonfinite(v.w);
    }));
    if (__ballot(bad) && lane == 0) atomicOr(status, ACX_KNN_NONFINITE);
    if (lane == 0) inv_norm[row] = inv_norm_of(s);
}

struct KnnSearchP {
    const float* q; long long ld_q; const float* rq; long long nq;
    const float* d; long long ld_d; const float* rd; long long n;
    int dim, k;
    const int* exclude;
    knn_key* ws;             // [nq][slices][k]
    int* status;
    int slices; long long slice_rows;
};

template <int QT, int R>
__global__ __launch_bounds__(kKnnThreads, 2) void knn_search_kernel(KnnSearchP p) {
    constexpr int TQ = 32 * QT, CAP = 64 * R;
    extern __shared__ knn_key s_buf[];           // [TQ][CAP]
    __shared__ knn_key s_thr[TQ];
    __shared__ int s_cnt[TQ];
    __shared__ int s_excl[TQ];
    __shared__ float s_rq[TQ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const long long q0 = (long long)blockIdx.x * TQ;
    const long long j_lo = (long long)blockIdx.y * p.slice_rows;
    const long long j_hi = min(p.n, j_lo + p.slice_rows);
    const bool cosine = p.rq != nullptr;

    if (tid < TQ) {
        const long long qi = q0 + tid;
        s_thr[tid] = 0ull;
        s_cnt[tid] = 0;
        s_excl[tid] = (p.exclude && qi < p.nq) ? p.exclude[qi] : -1;
        s_rq[tid] = cosine ? p.rq[min(qi, p.nq - 1)] : 1.f;
    }
    __syncthreads();

    // rows past nq / the slice repeat the last valid one: loads stay inside the buffers, results are dropped
    const float* qa[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) qa[t] = p.q + min(q0 + 32 * t + r32, p.nq - 1) * p.ld_q;
    bool bad = false;

    for (long long j0 = j_lo; j0 < j_hi; j0 += kKnnStepRows) {
        const long long jw = j0 + wave * 64;
        const bool active = jw < j_hi;               // wave-uniform
        F32Tile<32>::acc_t acc[QT][2];
        float rdv[2] = {1.f, 1.f};
        if (active) {
            const float* db[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long long j = min(jw + 32 * u + r32, j_hi - 1);
                db[u] = p.d + j * p.ld_d;
                if (cosine) rdv[u] = p.rd[j];
            }
            dot_tile<QT>(acc, qa, db, p.dim, h, [](const float4 (&)[2], const float4 (&)[2]) {});
        }

        // filter the tile into the candidate buffers; lanes left without a slot try again after the trim
        unsigned long long pend = active ? (QT == 2 ? ~0ull : 0xffffffffull) : 0ull;
        for (;;) {
            int over = 0;
            if (pend) {
#pragma unroll
                for (int t = 0; t < QT; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int bit = (t * 2 + u) * 16 + i;
                            if ((pend >> bit) & 1ull) {
                                const int ql = 32 * t + F32Tile<32>::row(i, h);
                                const long long j = jw + 32 * u + r32;
                                bool keep = false;
                                if (q0 + ql < p.nq && j < j_hi) {
                                    float s = acc[t][u][i];
                                    if (acx_nonfinite(s)) bad = true;
                                    if (j != (long long)s_excl[ql]) {
                                        if (cosine) s = cos_scale(s, s_rq[ql], rdv[u]);
                                        const knn_key key = knn_make_key(s, j);
                                        if (key > s_thr[ql]) {
                                            const int slot = atomicAdd(&s_cnt[ql], 1);
                                            if (slot < CAP) s_buf[ql * CAP + slot] = key;
                                            else { keep = true; over = 1; }
                                        }
                                    }
                                }
                                if (!keep) pend &= ~(1ull << bit);
                            }
                        }
            }
            if (!__syncthreads_or(over)) break;
            for (int ql = wave; ql < TQ; ql += 4) {
                const int cnt = s_cnt[ql];           // wave-uniform
                if (cnt >= CAP) {
                    knn_key v[R];
                    knn_load_sorted<R>(s_buf + ql * CAP, CAP, v, lane);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int e = lane + 64 * r;
                        s_buf[ql * CAP + e] = v[r];
                        if (e == p.k - 1) s_thr[ql] = v[r];
                    }
                    if (lane == 0) s_cnt[ql] = p.k;
                }
            }
            __syncthreads();
        }
    }

    // the slice's k best of each query, sorted, to the workspace (0 keys where the slice holds fewer than k candidates)
    for (int ql = wave; ql < TQ; ql += 4) {
        if (q0 + ql >= p.nq) break;
        knn_key v[R];
        knn_load_sorted<R>(s_buf + ql * CAP, min(s_cnt[ql], CAP), v, lane);
        knn_key* out = p.ws + ((q0 + ql) * p.slices + blockIdx.y) * p.k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            if (e < p.k) out[e] = v[r];
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(p.status, ACX_KNN_NONFINITE);
}

// One wave per query: the k best keys of its slices' lists (slices * k keys, contiguous), decoded.
template <int R>
__global__ __launch_bounds__(kKnnThreads) void knn_merge_kernel(const knn_key* __restrict__ ws, long long nq, int slices, int k,
                                                                int* __restrict__ indices, float* __restrict__ scores,
                                                                const int* status) {
    constexpr int CAP = 64 * R;
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const knn_key* flat = ws + q * slices * k;
    const long long total = (long long)slices * k;
    knn_key v[R];
    knn_load_sorted<R>(flat, (int)min(total, (long long)CAP), v, lane);
    for (long long pos = CAP; pos < total; pos += CAP - k) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            if (e >= k) v[r] = pos + (e - k) < total ? flat[pos + (e - k)] : 0ull;
        }
        knn_sort_desc<R>(v, lane);
    }
    const bool nonfinite = (*status & ACX_KNN_NONFINITE) != 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        if (e < k) {
            const bool none = nonfinite || v[r] == 0ull;
            indices[q * k + e] = none ? -1 : knn_key_index(v[r]);
            scores[q * k + e] = none ? __uint_as_float(0x7fc00000u) : knn_key_score(v[r]);
        }
    }
}

struct KnnVoteP {
    const int* indices; const float* scores; int k;
    const void* y; int y_u8; long long ld_y; long long n; int classes;
    int similarity; float temperature;
    float* out; long long ld_out; int* status;
};

__global__ __launch_bounds__(256) void knn_vote_kernel(KnnVoteP p) {
    __shared__ int s_idx[ACX_KNN_MAX_K];
    __shared__ float s_w[ACX_KNN_MAX_K];
    const long long q = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < p.k) {
        const int idx = p.indices[q * p.k + tid];
        const bool bad = idx < 0 || idx >= p.n;
        if (bad) atomicOr(p.status, ACX_KNN_BAD_INDEX);
        s_idx[tid] = bad ? -1 : idx;
        s_w[tid] = p.similarity ? expf((p.scores[q * p.k + tid] - p.scores[q * p.k]) / p.temperature) : 1.f;
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + tid;
    if (c >= p.classes) return;
    float res;
    if (!p.similarity && p.y_u8) {
        int count = 0;
        for (int j = 0; j < p.k; ++j)
            if (s_idx[j] >= 0) count += static_cast<const unsigned char*>(p.y)[s_idx[j] * p.ld_y + c] ? 1 : 0;
        res = (float)count / (float)p.k;
    } else {
        float num = 0.f, den = 0.f;
        for (int j = 0; j < p.k; ++j) {
            const float w = s_w[j];
            den += w;
            if (s_idx[j] >= 0) {
                const long long o = s_idx[j] * p.ld_y + c;
                const float y = p.y_u8 ? (static_cast<const unsigned char*>(p.y)[o] ? 1.f : 0.f) : static_cast<const float*>(p.y)[o];
                num = __builtin_fmaf(w, y, num);
            }
        }
        res = num / den;
    }
    p.out[q * p.ld_out + c] = res;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int check_f32_rows(const char* who, const char* name, const float* x, int64_t ld, int dim) {
    if (!x) ACX_FAIL(ACX_ERR_ARG, "%s: %s is null", who, name);
    if (dim < 4 || dim > ACX_KNN_MAX_DIM || (dim & 3))
        ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected a multiple of 4 in 4 .. %d)", who, dim, ACX_KNN_MAX_DIM);
    if (ld < dim || (ld & 3))
        ACX_FAIL(ACX_ERR_ARG, "%s: row stride of %s = %lld (expected a multiple of 4, at least dim = %d)", who, name, (long long)ld, dim);
    if (reinterpret_cast<uintptr_t>(x) & 15) ACX_FAIL(ACX_ERR_ARG, "%s: %s is not 16-byte aligned", who, name);
    return ACX_OK;
}

static DeviceOnce g_knn_lds[2][3];

template <int QT, int R>
static int knn_launch_search(const KnnSearchP& p, long long qtiles, DeviceOnce& once, hipStream_t s) {
    const size_t lds = (size_t)32 * QT * 64 * R * sizeof(knn_key);
    ACX_TRY(set_max_dynamic_lds(once, &knn_search_kernel<QT, R>, lds));
    launch_kernel(&knn_search_kernel<QT, R>, dim3((unsigned)qtiles, (unsigned)p.slices), dim3(kKnnThreads), lds, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int knn_launch_merge(const knn_key* ws, long long nq, int slices, int k, int r, int* indices, float* scores, const int* status,
                     hipStream_t s) {
    const dim3 mgrid((unsigned)((nq + 3) / 4));
    if (r == 1) launch_kernel(&knn_merge_kernel<1>, mgrid, dim3(kKnnThreads), 0, s, ws, nq, slices, k, indices, scores, status);
    else if (r == 2) launch_kernel(&knn_merge_kernel<2>, mgrid, dim3(kKnnThreads), 0, s, ws, nq, slices, k, indices, scores, status);
    else launch_kernel(&knn_merge_kernel<4>, mgrid, dim3(kKnnThreads), 0, s, ws, nq, slices, k, indices, scores, status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_knn_row_norms(const float* x, int64_t ld, int64_t n, int dim, float* inv_norm, int32_t* status, void* stream) {
    static const char* who = "acx_knn_row_norms";
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    ACX_TRY(check_f32_rows(who, "x", x, ld, dim));
    if (!inv_norm) ACX_FAIL(ACX_ERR_ARG, "%s: inv_norm is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    launch_kernel(&knn_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long long)ld, (long long)n,
                  dim, inv_norm, (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_knn_workspace_bytes(int64_t nq, int64_t n, int k, size_t* out_bytes) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_knn_workspace_bytes: out_bytes is null");
    ACX_TRY(knn_check_shape("acx_knn_workspace_bytes", nq, n, k));
    *out_bytes = knn_ws_bytes(nq, n, k);
    return ACX_OK;
}

int acx_knn_slices(int64_t nq, int64_t n, int k, int* out_slices) {
    if (!out_slices) ACX_FAIL(ACX_ERR_ARG, "acx_knn_slices: out_slices is null");
    ACX_TRY(knn_check_shape("acx_knn_slices", nq, n, k));
    *out_slices = knn_plan(nq, n, k).slices;
    return ACX_OK;
}

int acx_knn_search(const float* q, int64_t ld_q, const float* q_inv_norm, int64_t nq, const float* d, int64_t ld_d,
                   const float* d_inv_norm, int64_t n, int dim, int metric, int k, const int32_t* exclude, int32_t* indices,
                   float* scores, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_knn_search";
    ACX_TRY(knn_check_shape(who, nq, n, k));
    if (metric != ACX_KNN_DOT && metric != ACX_KNN_COSINE)
        ACX_FAIL(ACX_ERR_ARG, "%s: metric %d (expected ACX_KNN_DOT or ACX_KNN_COSINE)", who, metric);
    ACX_TRY(check_f32_rows(who, "q", q, ld_q, dim));
    ACX_TRY(check_f32_rows(who, "d", d, ld_d, dim));
    if (metric == ACX_KNN_COSINE && (!q_inv_norm || !d_inv_norm))
        ACX_FAIL(ACX_ERR_ARG, "%s: q_inv_norm / d_inv_norm is null with ACX_KNN_COSINE", who);
    if (!indices || !scores) ACX_FAIL(ACX_ERR_ARG, "%s: indices / scores is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    if (k > n - (exclude ? 1 : 0))
        ACX_FAIL(ACX_ERR_ARG, "%s: k = %d exceeds the %lld rows a query may return%s", who, k, (long long)(n - (exclude ? 1 : 0)),
                 exclude ? " (n - 1 with exclude)" : "");
    ACX_TRY(check_workspace(ws, ws_bytes, knn_ws_bytes(nq, n, k)));
    hipStream_t s = (hipStream_t)stream;
    const KnnPlan pl = knn_plan(nq, n, k);
    KnnSearchP p;
    p.q = q; p.ld_q = ld_q; p.rq = metric == ACX_KNN_COSINE ? q_inv_norm : nullptr; p.nq = nq;
    p.d = d; p.ld_d = ld_d; p.rd = metric == ACX_KNN_COSINE ? d_inv_norm : nullptr; p.n = n;
    p.dim = dim; p.k = k; p.exclude = exclude; p.ws = static_cast<knn_key*>(ws); p.status = (int*)status;
    p.slices = pl.slices; p.slice_rows = pl.slice_rows;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const long long qtiles = cdiv(nq, 32 * pl.qt);
    const int ri = pl.r == 1 ? 0 : pl.r == 2 ? 1 : 2;
    DeviceOnce& once = g_knn_lds[pl.qt - 1][ri];
    int rc;
    if (pl.qt == 1) rc = ri == 0 ? knn_launch_search<1, 1>(p, qtiles, once, s) : ri == 1 ? knn_launch_search<1, 2>(p, qtiles, once, s)
                                                                                         : knn_launch_search<1, 4>(p, qtiles, once, s);
    else rc = ri == 0 ? knn_launch_search<2, 1>(p, qtiles, once, s) : ri == 1 ? knn_launch_search<2, 2>(p, qtiles, once, s)
                                                                              : knn_launch_search<2, 4>(p, qtiles, once, s);
    ACX_TRY(rc);
    return knn_launch_merge(p.ws, nq, pl.slices, k, pl.r, (int*)indices, scores, (const int*)status, s);
}

int acx_knn_vote(const int32_t* indices, const float* scores, int64_t nq, int k, const void* target, int target_dtype,
                 int64_t ld_target, int64_t n, int classes, int weighting, float temperature, float* out, int64_t ld_out,
                 int32_t* status, void* stream) {
    static const char* who = "acx_knn_vote";
    ACX_TRY(knn_check_shape(who, nq, n, k));
    if (!indices) ACX_FAIL(ACX_ERR_ARG, "%s: indices is null", who);
    if (!target) ACX_FAIL(ACX_ERR_ARG, "%s: target is null", who);
    if (!out) ACX_FAIL(ACX_ERR_ARG, "%s: out is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (target_dtype != ACX_TARGET_F32 && target_dtype != ACX_TARGET_U8)
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, target_dtype);
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "%s: classes = %d (expected 1 .. %d)", who, classes, ACX_MAX_CLASSES);
    if (ld_target < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld_target = %lld is shorter than %d classes", who, (long long)ld_target, classes);
    if (ld_out < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld_out = %lld is shorter than %d classes", who, (long long)ld_out, classes);
    if (weighting != ACX_KNN_UNIFORM && weighting != ACX_KNN_SIMILARITY)
        ACX_FAIL(ACX_ERR_ARG, "%s: weighting %d (expected ACX_KNN_UNIFORM or ACX_KNN_SIMILARITY)", who, weighting);
    if (weighting == ACX_KNN_SIMILARITY) {
        if (!scores) ACX_FAIL(ACX_ERR_ARG, "%s: scores is null with ACX_KNN_SIMILARITY", who);
        if (!(temperature > 0.f) || !std::isfinite(temperature))
            ACX_FAIL(ACX_ERR_ARG, "%s: temperature = %g (expected > 0)", who, (double)temperature);
    }
    hipStream_t s = (hipStream_t)stream;
    KnnVoteP p;
    p.indices = (const int*)indices; p.scores = scores; p.k = k;
    p.y = target; p.y_u8 = target_dtype == ACX_TARGET_U8; p.ld_y = ld_target; p.n = n; p.classes = classes;
    p.similarity = weighting == ACX_KNN_SIMILARITY; p.temperature = temperature;
    p.out = out; p.ld_out = ld_out; p.status = (int*)status;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    launch_kernel(&knn_vote_kernel, dim3((unsigned)nq, (unsigned)((classes + 255) / 256)), dim3(256), 0, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
