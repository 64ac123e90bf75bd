// Reading and judging a single-label head (acx_softmax_topk / acx_classification_counts, include/acx.h): softmax
// probabilities, the k best classes of a row, and the counts behind accuracy, top-k accuracy, per-class precision / recall and
// the confusion matrix.
//
//   softmax_topk_kernel  one group per row (device_common.h, "softmax of one row": a wave for N <= 2048, four rows per
//                        workgroup; the whole workgroup for wider rows).  m, s and p_c = expf(z_c - m) / s are the functions
//                        fit_ce_row_kernel (head_fit.hip) calls, so the probabilities are the ones the head was trained with.
//                        The k best: k rounds of "the largest key below the last one taken" over the row's keys (knn_make_key:
//                        logit descending, class index ascending, -0.0 = +0.0; no two keys equal), each thread over its own
//                        elements, then the group maximum.  The rounds re-read the row from L1 / L2: k N / W loads per thread,
//                        45 for the AudioSet head at k = 5, but 8 192 for a 32 768-class row at k = 64 (64 rounds of 128
//                        loads): the cost grows as k N / W, and a wide head read at k = 64 pays for it
//                        (1 024 such rows: 0.39 ms at k = 5, 3.1 ms at k = 64; profiles/r20_a_classify_bench.txt, c').  top_prob is soft_prob of the chosen logit: the bits of probs.
//   class_counts_kernel  one group per run of rows; per row ONE pass gives the largest key (the prediction: the first index of
//                        the row maximum), the rank of the true class and the non-finite flag.  Counts go to memory with
//                        64-bit integer atomics (any order, same result); the two hit counters are kept in registers over
//                        the group's rows and added once.
// Nothing here sums floats across rows; a row's outputs depend on that row alone.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kClsThreads = 256;
constexpr long long kClsMaxRows = 1LL << 30;
constexpr int kClsMaxConfusion = 4096;

template <int W>
__device__ __forceinline__ knn_key group_max_key(knn_key v, knn_key* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const knn_key w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    if (W == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        const knn_key a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        v = a > b ? a : b;
    }
    return v;
}
template <int W>
__device__ __forceinline__ int group_sum_int(int v, int* red) {
    v = wave_sum(v);
    if (W == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = red[0] + red[1] + red[2] + red[3];
    }
    return v;
}

struct SoftTopkP {
    const float* z; long long ld; long long rows; int N; int k;
    float* probs; long long ld_p; int* top_index; float* top_prob; int* status;
};

template <int W>
__global__ __launch_bounds__(kClsThreads) void softmax_topk_kernel(SoftTopkP p) {
    __shared__ float red[4];
    __shared__ knn_key redk[4];
    const int t = soft_thread<W>();
    const long long row = W == 64 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
    if (row >= p.rows) return;                                     // W = 64 only: a whole wave, which meets no barrier
    const float* z = p.z + row * p.ld;
    float* pr = p.probs ? p.probs + row * p.ld_p : nullptr;
    int* ti = p.top_index + row * p.k;
    float* tp = p.top_prob + row * p.k;
    bool bad = false;
    for (int c = t; c < p.N; c += W) bad |= acx_nonfinite(z[c]);
    if (group_any<W>(bad)) {                                       // the same answer in every thread of the group
        const float nan = __uint_as_float(0x7fc00000u);
        if (pr)
            for (int c = t; c < p.N; c += W) pr[c] = nan;
        for (int j = t; j < p.k; j += W) { ti[j] = -1; tp[j] = nan; }
        if (t == 0) atomicOr(p.status, ACX_CLASSIFY_NONFINITE);
        return;
    }
    float m, s;
    soft_row_stats<W>(z, p.N, red, m, s);
    if (pr)
        for (int c = t; c < p.N; c += W) pr[c] = soft_prob(z[c], m, s);
    knn_key prev = ~0ull;
    for (int j = 0; j < p.k; ++j) {
        knn_key best = 0ull;
        for (int c = t; c < p.N; c += W) {
            const knn_key key = knn_make_key(z[c], c);
            if (key < prev && key > best) best = key;
        }
        best = group_max_key<W>(best, redk);                       // k <= N finite logits: never 0
        if (t == 0) {
            const int c = knn_key_index(best);
            ti[j] = c;
            tp[j] = soft_prob(z[c], m, s);
        }
        prev = best;
    }
}

struct ClassCountsP {
    const float* z; long long ld; const long long* labels; long long n; int N; int k;
    unsigned long long* per_class; unsigned long long* hits; unsigned long long* confusion; int* status;
    int rpg;            // rows per group
};

template <int W>
__global__ __launch_bounds__(kClsThreads) void class_counts_kernel(ClassCountsP p) {
    __shared__ knn_key redk[4];
    __shared__ int redi[4];
    const int t = soft_thread<W>();
    const long long g = W == 64 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
    const long long r_lo = g * p.rpg, r_hi = min(p.n, r_lo + p.rpg);
    unsigned long long h1 = 0, hk = 0;
    int flags = 0;
    for (long long row = r_lo; row < r_hi; ++row) {
        const float* z = p.z + row * p.ld;
        const long long y = p.labels[row];
        const bool ybad = y < 0 || y >= p.N;
        const float zy = ybad ? 0.f : z[y];
        bool bad = false;
        knn_key best = 0ull;
        int rank = 0;
        for (int c = t; c < p.N; c += W) {
            const float v = z[c];
            bad |= acx_nonfinite(v);
            const knn_key key = knn_make_key(v, c);
            best = key > best ? key : best;
            rank += (v > zy || (v == zy && c < y)) ? 1 : 0;
        }
        bad = group_any<W>(bad);
        if (bad || ybad) {                                         // uniform over the group
            flags |= (bad ? ACX_CLASSIFY_NONFINITE : 0) | (ybad ? ACX_CLASSIFY_BAD_LABEL : 0);
            continue;
        }
        best = group_max_key<W>(best, redk);
        rank = group_sum_int<W>(rank, redi);
        if (t == 0) {
            const int pred = knn_key_index(best);
            atomicAdd(p.per_class + 3 * y, 1ull);
            atomicAdd(p.per_class + 3 * (long long)pred + 1, 1ull);
            if (pred == y) { atomicAdd(p.per_class + 3 * y + 2, 1ull); ++h1; }
            if (rank < p.k) ++hk;
            if (p.confusion) atomicAdd(p.confusion + y * p.N + pred, 1ull);
        }
    }
    if (t == 0) {
        if (h1) atomicAdd(p.hits, h1);
        if (hk) atomicAdd(p.hits + 1, hk);
        if (flags) atomicOr(p.status, flags);
    }
}

static int cls_check_logits(const char* who, const float* logits, int64_t ld, int64_t rows, const char* rows_name, int classes,
                            int k, const int32_t* status) {
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (rows < 1) ACX_FAIL(ACX_ERR_ARG, "%s: %s = %lld (expected >= 1)", who, rows_name, (long long)rows);
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "%s: classes = %d (expected 1 .. %d)", who, classes, ACX_MAX_CLASSES);
    if (ld < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld = %lld is shorter than %d classes", who, (long long)ld, classes);
    const int kmax = classes < ACX_CLASSIFY_MAX_K ? classes : ACX_CLASSIFY_MAX_K;
    if (k < 1 || k > kmax) ACX_FAIL(ACX_ERR_ARG, "%s: k = %d (expected 1 .. %d)", who, k, kmax);
    if (rows > kClsMaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: %s = %lld (at most 2^30)", who, rows_name, (long long)rows);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_softmax_topk(const float* logits, int64_t ld, int64_t rows, int classes, int k, float* probs, int64_t ld_p,
                     int32_t* top_index, float* top_prob, int32_t* status, void* stream) {
    static const char* who = "acx_softmax_topk";
    ACX_TRY(cls_check_logits(who, logits, ld, rows, "rows", classes, k, status));
    if (!top_index) ACX_FAIL(ACX_ERR_ARG, "%s: top_index is null", who);
    if (!top_prob) ACX_FAIL(ACX_ERR_ARG, "%s: top_prob is null", who);
    if (probs && ld_p < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld_p = %lld is shorter than %d classes", who, (long long)ld_p, classes);
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, 4, s));
    const SoftTopkP p{logits, ld, rows, classes, k, probs, ld_p, (int*)top_index, top_prob, (int*)status};
    if (classes <= kSoftWaveMaxN)
        launch_kernel(&softmax_topk_kernel<64>, dim3((unsigned)((rows + 3) / 4)), dim3(kClsThreads), 0, s, p);
    else
        launch_kernel(&softmax_topk_kernel<256>, dim3((unsigned)rows), dim3(kClsThreads), 0, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_classification_counts(const float* logits, int64_t ld, const int64_t* labels, int64_t n, int classes, int k,
                              int64_t* per_class, int64_t* hits, int64_t* confusion, int32_t* status, void* stream) {
    static const char* who = "acx_classification_counts";
    ACX_TRY(cls_check_logits(who, logits, ld, n, "n", classes, k, status));
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!per_class) ACX_FAIL(ACX_ERR_ARG, "%s: per_class is null", who);
    if (!hits) ACX_FAIL(ACX_ERR_ARG, "%s: hits is null", who);
    if (confusion && classes > kClsMaxConfusion)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: confusion with classes = %d (at most %d: the matrix has classes^2 int64 cells)", who,
                 classes, kClsMaxConfusion);
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, 4, s));
    ACX_HIP(hipMemsetAsync(per_class, 0, (size_t)classes * 3 * 8, s));
    ACX_HIP(hipMemsetAsync(hits, 0, 16, s));
    if (confusion) ACX_HIP(hipMemsetAsync(confusion, 0, (size_t)classes * classes * 8, s));
    ClassCountsP p{logits, ld, reinterpret_cast<const long long*>(labels), n, classes, k,
                   reinterpret_cast<unsigned long long*>(per_class), reinterpret_cast<unsigned long long*>(hits),
                   reinterpret_cast<unsigned long long*>(confusion), (int*)status, 1};
    // about 8192 groups: enough to fill the device, few enough that the hit counters see one atomic per many rows
    const long long rpg = (n + 8191) / 8192;
    p.rpg = (int)(rpg > 256 ? 256 : rpg);
    const long long groups = (n + p.rpg - 1) / p.rpg;
    if (classes <= kSoftWaveMaxN)
        launch_kernel(&class_counts_kernel<64>, dim3((unsigned)((groups + 3) / 4)), dim3(kClsThreads), 0, s, p);
    else
        launch_kernel(&class_counts_kernel<256>, dim3((unsigned)groups), dim3(kClsThreads), 0, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
