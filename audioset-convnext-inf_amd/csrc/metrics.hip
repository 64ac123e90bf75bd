// Per-class AudioSet statistics on the device (acx_tagging_metrics, include/acx.h): average precision, ROC-AUC and d' of the
// reference's evaluate.py:44-58 (sklearn average_precision_score / roc_auc_score with average=None, scipy norm.ppf).
//
// A class's statistics depend only on the order of its scores, so they are computed exactly from two sorted runs:
//   key(s)  = the float32 bits mapped to an unsigned order (-0.0 canonicalised to +0.0 first: equal scores, equal keys)
//   for every positive i with key t:  TP(>= t) = P - #pos(< t),  FP(>= t) = Nn - #neg(< t)
//   AP  = (1/P) sum_i TP / (TP + FP)                      (float64; = sum over distinct positive thresholds of npos * precision)
//   AUC = sum_i (#neg(< t) + #neg(<= t)) / (2 P Nn)     (numerator in int64: Mann-Whitney with mid-ranks; one float64 division)
//   d'  = 2 erfinv(2 AUC - 1)                             (= sqrt(2) Phi^-1(AUC))
// P = 0: AP 0, AUC and d' NaN; Nn = 0: AP 1, AUC and d' NaN (sklearn 1.7.2 warns and returns these).
//
// Three launches on the caller's stream: the status word is cleared; metrics_prep_kernel transposes the (N, C) scores and
// targets into per-class keys / labels in the workspace and ORs invalid inputs into the status word; one workgroup per class
// then splits its keys into a positives run and a negatives run, sorts both (bitonic network, in LDS up to kMetLdsKeys keys,
// through the workspace beyond) and counts every positive against them by binary search.  Partial sums are reduced per wave and
// combined in a fixed order: the results are the same bits on every call.
//
// Operating points (acx_operating_points): the same prep, split and sorts, then one sweep over the distinct positive scores --
// the only thresholds worth choosing under the rule score >= threshold -- that keeps the best one under the criterion's total
// order (op_better below); an argmax over distinct candidates, so the result does not depend on the order of the reduction.
// acx_threshold_counts scores given thresholds on any split without a sort: integer sums per class, combined by integer atomics.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"
#include "metrics_common.h"

namespace acx {

// global-memory stores of one workgroup made visible to its other waves
__device__ __forceinline__ void met_gsync() {
    __threadfence();
    __syncthreads();
    __threadfence();
}

// the half-cleaners j = jtop .. 1 of a stage of block size k > kMetLdsKeys, over one chunk s[0, m) in LDS
__device__ void met_lds_tail(unsigned* s, int m, int k, int jtop) {
    const int half = met_pow2(m) >> 1;
    for (int j = jtop; j >= 1; j >>= 1) {
        for (int t = threadIdx.x; t < half; t += kMetThreads) {
            int lo, hi;
            met_pair(t, k, j, lo, hi);
            if (hi < m) met_cmpx(s, lo, hi);
        }
        __syncthreads();
    }
}

// sorts g[0, n) in global memory with the whole workgroup: stages whose comparators stay inside a chunk of kMetLdsKeys run on
// the chunk in LDS (s), the others over global memory
__device__ void met_global_sort(unsigned* g, int n, unsigned* s) {
    if (n <= 1) return;
    const int np = met_pow2(n);
    const int CH = kMetLdsKeys;
    const int chunks = (n + CH - 1) / CH;
    for (int q = 0; q < chunks; ++q) {            // every chunk sorted on its own: stages k = 2 .. min(np, CH)
        const int m = min(CH, n - q * CH);
        for (int e = threadIdx.x; e < m; e += kMetThreads) s[e] = g[(long long)q * CH + e];
        __syncthreads();
        met_lds_network(s, m, 2, min(np, CH));
        for (int e = threadIdx.x; e < m; e += kMetThreads) g[(long long)q * CH + e] = s[e];
        met_gsync();
    }
    for (int k = 2 * CH; k <= np; k <<= 1) {
        for (int j = k >> 1; j >= CH; j >>= 1) {
            for (int t = threadIdx.x; t < (np >> 1); t += kMetThreads) {
                int lo, hi;
                met_pair(t, k, j, lo, hi);
                if (hi < n) met_cmpx(g, lo, hi);
            }
            met_gsync();
        }
        for (int q = 0; q < chunks; ++q) {
            const int m = min(CH, n - q * CH);
            for (int e = threadIdx.x; e < m; e += kMetThreads) s[e] = g[(long long)q * CH + e];
            __syncthreads();
            met_lds_tail(s, m, k, CH >> 1);
            for (int e = threadIdx.x; e < m; e += kMetThreads) g[(long long)q * CH + e] = s[e];
            met_gsync();
        }
    }
}

// scores (N, C) row stride ld_s and targets (N, C) row stride ld_t -> keys[c][i] and labels[c][i] of the workspace, coalesced
// both ways through an LDS tile.  Any non-finite score sets ACX_METRICS_NONFINITE, any target other than 0 or 1
// ACX_METRICS_BAD_TARGET in *status (one atomic per wave that saw one).
__global__ __launch_bounds__(256) void metrics_prep_kernel(const float* __restrict__ scores, long long ld_s,
                                                           const void* __restrict__ target, int u8, long long ld_t, int n,
                                                           int C, unsigned* __restrict__ keys, unsigned char* __restrict__ labs,
                                                           int* status) {
    __shared__ unsigned s_key[kMetTile][kMetTile + 1];
    __shared__ unsigned char s_lab[kMetTile][kMetTile + 4];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * kMetTile;
    const int c0 = blockIdx.y * kMetTile;
    int bad = 0;
    for (int rr = ty; rr < kMetTile; rr += 4) {
        const long long r = r0 + rr;
        const int c = c0 + tx;
        if (r < n && c < C) {
            const float v = scores[r * ld_s + c];
            unsigned u = __float_as_uint(v);
            if ((u & 0x7f800000u) == 0x7f800000u) bad |= ACX_METRICS_NONFINITE;
            if (v == 0.0f) u = 0u;                                   // -0.0 == +0.0: one key
            s_key[rr][tx] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            unsigned char l;
            if (u8) {
                const unsigned char t = static_cast<const unsigned char*>(target)[r * ld_t + c];
                if (t > 1) bad |= ACX_METRICS_BAD_TARGET;
                l = t != 0;
            } else {
                const float t = static_cast<const float*>(target)[r * ld_t + c];
                if (!(t == 0.0f || t == 1.0f)) bad |= ACX_METRICS_BAD_TARGET;
                l = t == 1.0f;
            }
            s_lab[rr][tx] = l;
        }
    }
    __syncthreads();
    for (int cc = ty; cc < kMetTile; cc += 4) {
        const int c = c0 + cc;
        const long long r = r0 + tx;
        if (r < n && c < C) {
            keys[(long long)c * n + r] = s_key[tx][cc];
            labs[(long long)c * n + r] = s_lab[tx][cc];
        }
    }
    const unsigned long long b1 = __ballot(bad & ACX_METRICS_NONFINITE), b2 = __ballot(bad & ACX_METRICS_BAD_TARGET);
    const int bits = (b1 ? ACX_METRICS_NONFINITE : 0) | (b2 ? ACX_METRICS_BAD_TARGET : 0);
    if (__lane_id() == 0 && bits) atomicOr(status, bits);
}

// every positive against the sorted runs pos[0, P) and neg[0, Nn); the class's three results written by thread 0
template <typename T>
__device__ void met_count(const T* pos, int P, const T* neg, int Nn, double* s_ap, long long* s_auc, int c, double* ap,
                          double* auc, double* dprime) {
    double a = 0.0;
    long long u = 0;
    for (int j = threadIdx.x; j < P; j += kMetThreads) {
        const unsigned t = pos[j];
        const int lbp = met_bound(pos, P, t, false);
        const int lbn = met_bound(neg, Nn, t, false);
        const int ubn = met_bound(neg, Nn, t, true);
        const long long tp = P - lbp, fp = Nn - lbn;
        a += (double)tp / (double)(tp + fp);
        u += (long long)lbn + ubn;
    }
    a = wave_sum(a);
    u = wave_sum(u);
    const int w = threadIdx.x >> 6;
    if (__lane_id() == 0) { s_ap[w] = a; s_auc[w] = u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0;
        long long su = 0;
        for (int i = 0; i < kMetWaves; ++i) { sa += s_ap[i]; su += s_auc[i]; }
        const double au = (P > 0 && Nn > 0) ? (double)su / (double)(2LL * P * (long long)Nn) : __builtin_nan("");
        ap[c] = P > 0 ? sa / (double)P : 0.0;
        auc[c] = au;
        dprime[c] = 2.0 * erfinv(2.0 * au - 1.0);
    }
}

__device__ __forceinline__ bool met_failed(const int* status, int c, double* ap, double* auc, double* dprime) {
    if (*status == 0) return false;
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        ap[c] = nan; auc[c] = nan; dprime[c] = nan;
    }
    return true;
}

// N <= kMetLdsKeys: both runs in LDS (dynamic, n keys)
__global__ __launch_bounds__(kMetThreads) void metrics_lds_kernel(const unsigned* __restrict__ keys,
                                                                  const unsigned char* __restrict__ labs, int n,
                                                                  const int* status, double* ap, double* auc, double* dprime) {
    extern __shared__ unsigned s_k[];
    __shared__ int s_cnt[2];
    __shared__ double s_ap[kMetWaves];
    __shared__ long long s_auc[kMetWaves];
    const int c = blockIdx.x;
    if (met_failed(status, c, ap, auc, dprime)) return;
    const int P = met_split(keys + (long long)c * n, labs + (long long)c * n, n, s_k, s_cnt);
    const int Nn = n - P;
    // both runs through one network loop: comparators of the positives first, then those of the negatives
    const int npP = met_pow2(P), npN = met_pow2(Nn);
    const int kmax = max(npP, npN);
    for (int k = 2; k <= kmax; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const int hp = k <= npP ? npP >> 1 : 0, hn = k <= npN ? npN >> 1 : 0;
            for (int t = threadIdx.x; t < hp + hn; t += kMetThreads) {
                const bool inp = t < hp;
                unsigned* base = inp ? s_k : s_k + P;
                int lo, hi;
                met_pair(inp ? t : t - hp, k, j, lo, hi);
                if (hi < (inp ? P : Nn)) met_cmpx(base, lo, hi);
            }
            __syncthreads();
        }
    met_count(s_k, P, s_k + P, Nn, s_ap, s_auc, c, ap, auc, dprime);
}

// N > kMetLdsKeys: the runs of class c in runs[c][0, n) of the workspace, sorted chunk-wise in LDS and across chunks in place
__global__ __launch_bounds__(kMetThreads) void metrics_global_kernel(const unsigned* __restrict__ keys,
                                                                     const unsigned char* __restrict__ labs, int n,
                                                                     unsigned* runs, const int* status, double* ap,
                                                                     double* auc, double* dprime) {
    extern __shared__ unsigned s_k[];
    __shared__ int s_cnt[2];
    __shared__ double s_ap[kMetWaves];
    __shared__ long long s_auc[kMetWaves];
    const int c = blockIdx.x;
    if (met_failed(status, c, ap, auc, dprime)) return;
    unsigned* g = runs + (long long)c * n;
    const int P = met_split(keys + (long long)c * n, labs + (long long)c * n, n, g, s_cnt);
    const int Nn = n - P;
    met_gsync();
    met_global_sort(g, P, s_k);
    met_global_sort(g + P, Nn, s_k);
    met_count((const unsigned*)g, P, (const unsigned*)(g + P), Nn, s_ap, s_auc, c, ap, auc, dprime);
}

// ---- operating points -----------------------------------------------------------------------------------------------------

struct OpSpec {
    int crit;              // ACX_OP_*
    double param;          // precision / recall: the level to reach
    double b2, onepb2;     // F-beta: beta * beta and 1 + beta * beta, both rounded on the host
};

// A thread's best candidate.  The criterion's total order is (f, rank), larger is better: F-beta ranks by F, then by the key
// (the highest threshold among equal F); precision and recall give every qualifying candidate f = 0 and rank by ~key (the lowest
// threshold) and by the key (the highest).  f < 0: no candidate.  Keys of candidates are distinct, so the maximum is unique.
struct OpBest {
    double f;
    unsigned rank;
    int tp, fp;
};

__device__ __forceinline__ bool op_better(const OpBest& x, const OpBest& b) {
    return x.f >= 0.0 && (x.f > b.f || (x.f == b.f && x.rank > b.rank));
}

// F-beta of a candidate.  The selection has to equal the host statement (pytorch/metrics.py operating_points_host) bit for bit,
// and there every operation is rounded on its own: contraction into fused multiply-adds, which hipcc applies by default, is
// switched off for this function.
__device__ __forceinline__ double op_fbeta(const OpSpec& sp, int tp, int fn, int fp) {
#pragma clang fp contract(off)
    const double num = sp.onepb2 * (double)tp;
    const double den = (num + sp.b2 * (double)fn) + (double)fp;
    return num / den;
}

// every distinct positive score of the sorted runs pos[0, P) and neg[0, Nn) as a threshold; the class's threshold and its
// (TP, FP, FN, TN) written by thread 0
__device__ void met_operating(const unsigned* pos, int P, const unsigned* neg, int Nn, const OpSpec& sp, OpBest* s_best, int c,
                              float* thresholds, long long* counts) {
    OpBest b{-1.0, 0u, 0, 0};
    for (int j = threadIdx.x; j < P; j += kMetThreads) {
        const unsigned t = pos[j];
        if (j > 0 && pos[j - 1] == t) continue;            // the first of equal positives: met_bound(pos, P, t, false) == j
        OpBest x;
        x.tp = P - j;
        x.fp = Nn - met_bound(neg, Nn, t, false);
        if (sp.crit == ACX_OP_FBETA) {
            x.f = op_fbeta(sp, x.tp, P - x.tp, x.fp);
            x.rank = t;
        } else if (sp.crit == ACX_OP_PRECISION) {
            x.f = (double)x.tp / (double)(x.tp + x.fp) >= sp.param ? 0.0 : -1.0;
            x.rank = ~t;
        } else {
            x.f = (double)x.tp / (double)P >= sp.param ? 0.0 : -1.0;
            x.rank = t;
        }
        if (op_better(x, b)) b = x;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        OpBest o;
        o.f = __shfl_xor(b.f, d);
        o.rank = __shfl_xor(b.rank, d);
        o.tp = __shfl_xor(b.tp, d);
        o.fp = __shfl_xor(b.fp, d);
        if (op_better(o, b)) b = o;
    }
    if (__lane_id() == 0) s_best[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kMetWaves; ++i)
            if (op_better(s_best[i], b)) b = s_best[i];
        long long* o = counts + (long long)c * 4;
        if (b.f >= 0.0) {
            const unsigned key = sp.crit == ACX_OP_PRECISION ? ~b.rank : b.rank;
            thresholds[c] = __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);      // key 0x80000000 -> +0.0
            o[0] = b.tp; o[1] = b.fp; o[2] = P - b.tp; o[3] = Nn - b.fp;
        } else {                                            // no positives, or a precision no threshold reaches: never fires
            thresholds[c] = INFINITY;
            o[0] = 0; o[1] = 0; o[2] = P; o[3] = Nn;
        }
    }
}

__device__ __forceinline__ bool op_failed(const int* status, int c, float* thresholds, long long* counts) {
    if (*status == 0) return false;
    if (threadIdx.x < 4) counts[(long long)c * 4 + threadIdx.x] = -1;
    if (threadIdx.x == 0) thresholds[c] = __builtin_nanf("");
    return true;
}

// N <= kMetLdsKeys: both runs in LDS (dynamic, n keys)
__global__ __launch_bounds__(kMetThreads) void operating_lds_kernel(const unsigned* __restrict__ keys,
                                                                    const unsigned char* __restrict__ labs, int n,
                                                                    const int* status, OpSpec sp, float* thresholds,
                                                                    long long* counts) {
    extern __shared__ unsigned s_k[];
    __shared__ int s_cnt[2];
    __shared__ OpBest s_best[kMetWaves];
    const int c = blockIdx.x;
    if (op_failed(status, c, thresholds, counts)) return;
    const int P = met_split(keys + (long long)c * n, labs + (long long)c * n, n, s_k, s_cnt);
    const int Nn = n - P;
    // the positives, then the negatives, each through the network met_global_sort runs on a chunk (metrics_lds_kernel keeps its
    // own loop over both runs at once, and with it its code)
    if (P > 1) met_lds_network(s_k, P, 2, met_pow2(P));
    if (Nn > 1) met_lds_network(s_k + P, Nn, 2, met_pow2(Nn));
    met_operating(s_k, P, s_k + P, Nn, sp, s_best, c, thresholds, counts);
}

// N > kMetLdsKeys: the runs of class c in runs[c][0, n) of the workspace, as metrics_global_kernel sorts them
__global__ __launch_bounds__(kMetThreads) void operating_global_kernel(const unsigned* __restrict__ keys,
                                                                       const unsigned char* __restrict__ labs, int n,
                                                                       unsigned* runs, const int* status, OpSpec sp,
                                                                       float* thresholds, long long* counts) {
    extern __shared__ unsigned s_k[];
    __shared__ int s_cnt[2];
    __shared__ OpBest s_best[kMetWaves];
    const int c = blockIdx.x;
    if (op_failed(status, c, thresholds, counts)) return;
    unsigned* g = runs + (long long)c * n;
    const int P = met_split(keys + (long long)c * n, labs + (long long)c * n, n, g, s_cnt);
    const int Nn = n - P;
    met_gsync();
    met_global_sort(g, P, s_k);
    met_global_sort(g + P, Nn, s_k);
    met_operating(g, P, g + P, Nn, sp, s_best, c, thresholds, counts);
}

// ---- counts at given thresholds -------------------------------------------------------------------------------------------

constexpr int kThrRows = 256;                     // rows per workgroup: 64 classes x 4 rows per pass, 256 threads

// acc[c] = (TP, FP, P, -) of score >= thresholds[c] over the rows of this workgroup, added with integer atomics: any order gives
// the same sums.  Rows are read as coalesced lines of 64 classes.  Invalid inputs are ORed into *status.
__global__ __launch_bounds__(256) void threshold_counts_kernel(const float* __restrict__ scores, long long ld_s,
                                                               const void* __restrict__ target, int u8, long long ld_t, int n,
                                                               int C, const float* __restrict__ thresholds,
                                                               unsigned long long* acc, int* status) {
    __shared__ int s_part[4][3][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + tx;
    const long long r0 = (long long)blockIdx.x * kThrRows;
    const long long r1 = r0 + kThrRows < n ? r0 + kThrRows : n;
    int bad = 0, tp = 0, fp = 0, p = 0;
    if (c < C) {
        const float th = thresholds[c];
        if (th != th) bad |= ACX_METRICS_BAD_THRESHOLD;
        for (long long r = r0 + ty; r < r1; r += 4) {
            const float v = scores[r * ld_s + c];
            if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) bad |= ACX_METRICS_NONFINITE;
            bool l;
            if (u8) {
                const unsigned char t = static_cast<const unsigned char*>(target)[r * ld_t + c];
                if (t > 1) bad |= ACX_METRICS_BAD_TARGET;
                l = t != 0;
            } else {
                const float t = static_cast<const float*>(target)[r * ld_t + c];
                if (!(t == 0.0f || t == 1.0f)) bad |= ACX_METRICS_BAD_TARGET;
                l = t == 1.0f;
            }
            const bool fire = v >= th;                     // float32 order: -0.0 == +0.0, nothing finite reaches +inf
            tp += fire && l;
            fp += fire && !l;
            p += l;
        }
    }
    s_part[ty][0][tx] = tp; s_part[ty][1][tx] = fp; s_part[ty][2][tx] = p;
    __syncthreads();
    if (ty < 3 && c < C) {                                 // wave ty adds quantity ty of its 64 classes
        const int v = s_part[0][ty][tx] + s_part[1][ty][tx] + s_part[2][ty][tx] + s_part[3][ty][tx];
        if (v) atomicAdd(&acc[(long long)c * 4 + ty], (unsigned long long)v);
    }
    const int bits = (__ballot(bad & ACX_METRICS_NONFINITE) ? ACX_METRICS_NONFINITE : 0) |
                     (__ballot(bad & ACX_METRICS_BAD_TARGET) ? ACX_METRICS_BAD_TARGET : 0) |
                     (__ballot(bad & ACX_METRICS_BAD_THRESHOLD) ? ACX_METRICS_BAD_THRESHOLD : 0);
    if (__lane_id() == 0 && bits) atomicOr(status, bits);
}

// (TP, FP, P, -) -> (TP, FP, FN, TN), or four -1 on a data error
__global__ __launch_bounds__(256) void threshold_finish_kernel(long long* counts, int n, int C, const int* status) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    long long* o = counts + (long long)c * 4;
    if (*status) {
        o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1;
    } else {
        const long long tp = o[0], fp = o[1], p = o[2];
        o[2] = p - tp;
        o[3] = ((long long)n - p) - fp;
    }
}

// keys, labels and (N > kMetLdsKeys) the global runs, each 256-byte aligned
void met_layout(long long n, long long C, size_t* keys_off, size_t* labs_off, size_t* runs_off, size_t* total) {
    const size_t kb = align_up((size_t)n * C * 4), lb = align_up((size_t)n * C);
    *keys_off = 0;
    *labs_off = kb;
    *runs_off = kb + lb;
    *total = kb + lb + (n > kMetLdsKeys ? kb : 0);
}

int met_check_shape(int64_t n, int classes) {
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "tagging metrics: n = %lld (expected >= 1)", (long long)n);
    if (classes < 1) ACX_FAIL(ACX_ERR_ARG, "tagging metrics: %d classes (expected >= 1)", classes);
    if (n > kMetMaxN) ACX_FAIL(ACX_ERR_UNSUPPORTED, "tagging metrics: n = %lld (at most 2^30 rows)", (long long)n);
    return ACX_OK;
}

int met_check_inputs(const char* who, const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                            int64_t ld_target, int64_t n, int classes, const int32_t* status) {
    if (!scores || !target || !status) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (target_dtype != ACX_TARGET_F32 && target_dtype != ACX_TARGET_U8)
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, target_dtype);
    ACX_TRY(met_check_shape(n, classes));
    if (ld_scores < classes || ld_target < classes)
        ACX_FAIL(ACX_ERR_ARG, "%s: row strides %lld / %lld are shorter than %d classes", who, (long long)ld_scores,
                 (long long)ld_target, classes);
    return ACX_OK;
}

int met_prepare(const char* who, const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                       int64_t ld_target, int64_t n, int classes, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s,
                       MetPrep* m) {
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(met_check_inputs(who, scores, ld_scores, target, target_dtype, ld_target, n, classes, status));
    size_t koff, loff, roff, need;
    met_layout(n, classes, &koff, &loff, &roff, &need);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, need));
    char* w = static_cast<char*>(ws);
    m->keys = reinterpret_cast<unsigned*>(w + koff);
    m->labs = reinterpret_cast<unsigned char*>(w + loff);
    m->runs = reinterpret_cast<unsigned*>(w + roff);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const dim3 pgrid((unsigned)((n + kMetTile - 1) / kMetTile), (unsigned)((classes + kMetTile - 1) / kMetTile));
    launch_kernel(&metrics_prep_kernel, pgrid, dim3(256), 0, s, scores, (long long)ld_scores, target,
                  target_dtype == ACX_TARGET_U8 ? 1 : 0, (long long)ld_target, (int)n, classes, m->keys, m->labs, (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_metrics_workspace_bytes(int64_t n, int classes, size_t* out_bytes) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_metrics_workspace_bytes: out_bytes is null");
    ACX_TRY(met_check_shape(n, classes));
    size_t k, l, r;
    met_layout(n, classes, &k, &l, &r, out_bytes);
    return ACX_OK;
}

int acx_tagging_metrics(const float* scores, int64_t ld_scores, const void* target, int target_dtype, int64_t ld_target,
                        int64_t n, int classes, double* ap, double* auc, double* dprime, int32_t* status, void* ws,
                        size_t ws_bytes, void* stream) {
    if (!ap || !auc || !dprime) ACX_FAIL(ACX_ERR_ARG, "acx_tagging_metrics: null argument");
    MetPrep m;
    ACX_TRY(met_prepare("acx_tagging_metrics", scores, ld_scores, target, target_dtype, ld_target, n, classes, status, ws, ws_bytes,
                        (hipStream_t)stream, &m));
    const hipStream_t s = (hipStream_t)stream;
    unsigned* keys = m.keys;
    unsigned char* labs = m.labs;
    if (n <= kMetLdsKeys) {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &metrics_lds_kernel, (size_t)kMetLdsKeys * 4));
        launch_kernel(&metrics_lds_kernel, dim3(classes), dim3(kMetThreads), (size_t)n * 4, s, (const unsigned*)keys,
                      (const unsigned char*)labs, (int)n, (const int*)status, ap, auc, dprime);
    } else {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &metrics_global_kernel, (size_t)kMetLdsKeys * 4));
        launch_kernel(&metrics_global_kernel, dim3(classes), dim3(kMetThreads), (size_t)kMetLdsKeys * 4, s, (const unsigned*)keys,
                      (const unsigned char*)labs, (int)n, m.runs, (const int*)status, ap, auc, dprime);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_operating_points(const float* scores, int64_t ld_scores, const void* target, int target_dtype, int64_t ld_target,
                         int64_t n, int classes, const acx_operating_spec* spec, float* thresholds, int64_t* counts,
                         int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "acx_operating_points";
    if (!spec || !thresholds || !counts) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    const double v = spec->param;
    if (spec->criterion == ACX_OP_FBETA) {
        if (!(v > 0.0) || std::isinf(v)) ACX_FAIL(ACX_ERR_ARG, "%s: beta %g (expected a finite value > 0)", who, v);
    } else if (spec->criterion == ACX_OP_PRECISION || spec->criterion == ACX_OP_RECALL) {
        if (!(v > 0.0 && v <= 1.0)) ACX_FAIL(ACX_ERR_ARG, "%s: level %g (expected a value in (0, 1])", who, v);
    } else {
        ACX_FAIL(ACX_ERR_ARG, "%s: criterion %d (expected ACX_OP_FBETA, ACX_OP_PRECISION or ACX_OP_RECALL)", who, spec->criterion);
    }
    const hipStream_t s = (hipStream_t)stream;
    MetPrep m;
    ACX_TRY(met_prepare(who, scores, ld_scores, target, target_dtype, ld_target, n, classes, status, ws, ws_bytes, s, &m));
    OpSpec sp;
    sp.crit = spec->criterion;
    sp.param = v;
    {
#pragma clang fp contract(off)       // two roundings, as the host statement has them
        sp.b2 = v * v;
        sp.onepb2 = 1.0 + sp.b2;
    }
    if (n <= kMetLdsKeys) {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &operating_lds_kernel, (size_t)kMetLdsKeys * 4));
        launch_kernel(&operating_lds_kernel, dim3(classes), dim3(kMetThreads), (size_t)n * 4, s, (const unsigned*)m.keys,
                      (const unsigned char*)m.labs, (int)n, (const int*)status, sp, thresholds,
                      reinterpret_cast<long long*>(counts));
    } else {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &operating_global_kernel, (size_t)kMetLdsKeys * 4));
        launch_kernel(&operating_global_kernel, dim3(classes), dim3(kMetThreads), (size_t)kMetLdsKeys * 4, s,
                      (const unsigned*)m.keys, (const unsigned char*)m.labs, (int)n, m.runs, (const int*)status, sp, thresholds,
                      reinterpret_cast<long long*>(counts));
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_threshold_counts(const float* scores, int64_t ld_scores, const void* target, int target_dtype, int64_t ld_target,
                         int64_t n, int classes, const float* thresholds, int64_t* counts, int32_t* status, void* stream) {
    const char* who = "acx_threshold_counts";
    if (!thresholds || !counts) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(met_check_inputs(who, scores, ld_scores, target, target_dtype, ld_target, n, classes, status));
    if (classes > 65535 * 64) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: %d classes (at most %d)", who, classes, 65535 * 64);
    const hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(counts, 0, (size_t)classes * 4 * sizeof(int64_t), s));
    const dim3 grid((unsigned)((n + kThrRows - 1) / kThrRows), (unsigned)((classes + 63) / 64));
    launch_kernel(&threshold_counts_kernel, grid, dim3(256), 0, s, scores, (long long)ld_scores, target,
                  target_dtype == ACX_TARGET_U8 ? 1 : 0, (long long)ld_target, (int)n, classes, thresholds,
                  reinterpret_cast<unsigned long long*>(counts), (int*)status);
    ACX_HIP(hipGetLastError());
    launch_kernel(&threshold_finish_kernel, dim3((classes + 255) / 256), dim3(256), 0, s, reinterpret_cast<long long*>(counts),
                  (int)n, classes, (const int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
