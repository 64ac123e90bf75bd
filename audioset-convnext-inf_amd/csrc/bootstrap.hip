// Bootstrap weights and weighted per-class statistics on the device (acx_bootstrap_weights, acx_weighted_metrics, include/acx.h):
// confidence intervals for mAP, AUC and d' by resampling the clips.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"
#include "metrics_common.h"

namespace acx {

// ---- weighted statistics over an order computed once (acx_weighted_metrics), bootstrap weights ----------------------------------
// A non-negative integer weight per row -- a bootstrap resample is the count of each row's draws -- changes no score, so the
// order of a class is the same for every weight vector.  weighted_plan_kernel sorts each class once and keeps what depends on
// the order: per row the SLOT of its tie group (the first index of its key in its own sorted run; positives 0 .. P - 1, negatives
// P .. n - 1) and per positive tie group the bounds of its key among the negatives.  weighted_recount_kernel, one workgroup per
// (class, weight vector), adds the weights into one LDS bucket per slot (integer atomics: any order, the same sums), scans the
// buckets and evaluates every positive tie group of non-zero weight from the prefix sums.

// splitmix64's finaliser
__host__ __device__ __forceinline__ unsigned long long boot_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}

// weights[k][idx(first + k, j)] += 1 for draw j of this thread; base = boot_mix(seed).  The rows were cleared in front.
__global__ __launch_bounds__(256) void bootstrap_weights_kernel(unsigned long long base, unsigned first, int replicates, int n,
                                                                int* __restrict__ weights, long long ld_w) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    for (int k = blockIdx.y; k < replicates; k += gridDim.y) {
        const unsigned long long r = (unsigned long long)first + (unsigned long long)k;
        const unsigned long long x = boot_mix(base + 0x9E3779B97F4A7C15ULL * (((r << 32) | (unsigned long long)j) + 1ULL));
        const long long idx = (long long)(((x >> 32) * (unsigned long long)n) >> 32);          // < n
        atomicAdd(&weights[(long long)k * ld_w + idx], 1);
    }
}

// a negative weight, or a row of weights whose sum exceeds 2^30 (the int32 buckets and the int64 AUC numerator then hold),
// sets ACX_METRICS_BAD_WEIGHT
__global__ __launch_bounds__(256) void weights_check_kernel(const int* __restrict__ weights, long long ld_w, int n, int replicates,
                                                            int* status) {
    __shared__ long long s_sum[4];
    __shared__ int s_neg[4];
    for (int k = blockIdx.x; k < replicates; k += gridDim.x) {
        const int* w = weights + (long long)k * ld_w;
        long long sum = 0;
        int neg = 0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int v = w[i];
            neg |= v < 0;
            sum += v;
        }
        sum = wave_sum(sum);
        const unsigned long long bn = __ballot(neg);
        if (__lane_id() == 0) { s_sum[threadIdx.x >> 6] = sum; s_neg[threadIdx.x >> 6] = bn != 0; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long total = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
            if ((s_neg[0] | s_neg[1] | s_neg[2] | s_neg[3]) || total > (1LL << 30)) atomicOr(status, ACX_METRICS_BAD_WEIGHT);
        }
        __syncthreads();
    }
}

// one workgroup per class, n <= kMetLdsKeys: slots[c][i] of every row, nbounds[c][j] = lower | upper << 16 bound among the
// negatives of the positive tie group that starts at slot j (both <= Nn <= 32767 where a positive exists), npos[c] = P
__global__ __launch_bounds__(kMetThreads) void weighted_plan_kernel(const unsigned* __restrict__ keys,
                                                                    const unsigned char* __restrict__ labs, int n,
                                                                    const int* status, unsigned short* __restrict__ slots,
                                                                    unsigned* __restrict__ nbounds, int* __restrict__ npos) {
    extern __shared__ unsigned s_k[];
    __shared__ int s_cnt[2];
    const int c = blockIdx.x;
    if (*status != 0) return;                              // the recount writes the NaNs
    const unsigned* key = keys + (long long)c * n;
    const unsigned char* lab = labs + (long long)c * n;
    const int P = met_split(key, lab, n, s_k, s_cnt);
    const int Nn = n - P;
    if (P > 1) met_lds_network(s_k, P, 2, met_pow2(P));
    if (Nn > 1) met_lds_network(s_k + P, Nn, 2, met_pow2(Nn));
    for (int i = threadIdx.x; i < n; i += kMetThreads) {
        const unsigned k = key[i];
        const int slot = lab[i] ? met_bound(s_k, P, k, false) : P + met_bound(s_k + P, Nn, k, false);
        slots[(long long)c * n + i] = (unsigned short)slot;
    }
    for (int j = threadIdx.x; j < P; j += kMetThreads) {
        const unsigned t = s_k[j];
        if (j > 0 && s_k[j - 1] == t) continue;            // only a tie group's first slot ever holds weight
        const unsigned lbn = met_bound(s_k + P, Nn, t, false), ubn = met_bound(s_k + P, Nn, t, true);
        nbounds[(long long)c * n + j] = lbn | (ubn << 16);
    }
    if (threadIdx.x == 0) npos[c] = P;
}

// workgroup (c, r - r0): the class's three statistics under weight vector r, into ap / auc / dprime[r][c].  With I the inclusive
// scan of the buckets and E(q) = I[q - 1] (0 at q = 0): Pw = E(P), Nw = I[n - 1] - Pw, and for the positive group at slot j with
// weight g = I[j] - E(j) > 0 and bounds (lbn, ubn):  TPw = Pw - E(j),  Nw(< t) = E(P + lbn) - Pw,  Nw(<= t) = E(P + ubn) - Pw.
__global__ __launch_bounds__(kMetThreads) void weighted_recount_kernel(const unsigned short* __restrict__ slots,
                                                                       const unsigned* __restrict__ nbounds,
                                                                       const int* __restrict__ npos, int n, int C,
                                                                       const int* __restrict__ weights, long long ld_w,
                                                                       int r0, const int* status, double* ap, double* auc,
                                                                       double* dprime) {
    extern __shared__ int s_b[];
    __shared__ int s_wsum[kMetWaves];
    __shared__ double s_ap[kMetWaves];
    __shared__ long long s_auc[kMetWaves];
    const int c = blockIdx.x;
    const int lane = __lane_id(), wv = threadIdx.x >> 6;
    const double nan = __builtin_nan("");
    const int r = r0 + blockIdx.y;
    const long long o = (long long)r * C + c;
    if (*status != 0) {
        if (threadIdx.x == 0) { ap[o] = nan; auc[o] = nan; dprime[o] = nan; }
        return;
    }
    const int P = npos[c];
    const unsigned short* slot = slots + (long long)c * n;
    const unsigned* nb = nbounds + (long long)c * n;
    const int seg = (n + kMetThreads - 1) / kMetThreads * 64;        // buckets per wave in the scan, a multiple of 64
    const int b0 = wv * seg, b1 = min(n, b0 + seg);
    for (int i = threadIdx.x; i < n; i += kMetThreads) s_b[i] = 0;
    __syncthreads();
    const int* w = weights + (long long)r * ld_w;
    for (int i = threadIdx.x; i < n; i += kMetThreads) {
        const int wi = w[i];
        if (wi) atomicAdd(&s_b[slot[i]], wi);
    }
    __syncthreads();
    // inclusive scan in place: every wave over its own segment, then the sums of the waves in front added
    int carry = 0;
    for (int e = b0; e < b1; e += 64) {
        const int i = e + lane;
        int v = i < b1 ? s_b[i] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        v += carry;
        if (i < b1) s_b[i] = v;
        carry = __shfl(v, 63);
    }
    if (lane == 0) s_wsum[wv] = carry;
    __syncthreads();
    int off = 0;
    for (int q = 0; q < wv; ++q) off += s_wsum[q];
    if (off)
        for (int i = b0 + lane; i < b1; i += 64) s_b[i] += off;
    __syncthreads();
    const int Pw = P ? s_b[P - 1] : 0;
    const int Nw = s_b[n - 1] - Pw;
    double a = 0.0;
    long long u = 0;
    for (int j = threadIdx.x; j < P; j += kMetThreads) {
        const int before = j ? s_b[j - 1] : 0;
        const int g = s_b[j] - before;
        if (g == 0) continue;
        const unsigned b = nb[j];
        const int lbn = b & 0xffffu, ubn = b >> 16;
        const int nlt = (P + lbn ? s_b[P + lbn - 1] : 0) - Pw, nle = (P + ubn ? s_b[P + ubn - 1] : 0) - Pw;
        const int tpw = Pw - before, fpw = Nw - nlt;
        a += (double)g * ((double)tpw / (double)(tpw + fpw));
        u += (long long)g * (long long)(nlt + nle);              // g (2 Nw(< t) + Nw(= t))
    }
    a = wave_sum(a);
    u = wave_sum(u);
    if (lane == 0) { s_ap[wv] = a; s_auc[wv] = u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0;
        long long su = 0;
        for (int i = 0; i < kMetWaves; ++i) { sa += s_ap[i]; su += s_auc[i]; }
        const double au = (Pw > 0 && Nw > 0) ? (double)su / (double)(2LL * Pw * (long long)Nw) : nan;
        ap[o] = Pw > 0 ? sa / (double)Pw : nan;
        auc[o] = Pw > 0 ? au : nan;
        dprime[o] = Pw > 0 ? 2.0 * erfinv(2.0 * au - 1.0) : nan;
    }
}

// acx_weighted_metrics: the keys and labels of met_layout, then the plan -- slots (uint16), bounds (uint32) and P per class
static void weighted_layout(long long n, long long C, size_t* slots_off, size_t* nb_off, size_t* npos_off, size_t* total) {
    size_t k, l, r, base;
    met_layout(n, C, &k, &l, &r, &base);
    *slots_off = base;
    *nb_off = *slots_off + align_up((size_t)n * C * 2);
    *npos_off = *nb_off + align_up((size_t)n * C * 4);
    *total = *npos_off + align_up((size_t)C * 4);
}

static int weighted_check_shape(const char* who, int64_t n, int classes) {
    ACX_TRY(met_check_shape(n, classes));
    if (n > kMetLdsKeys)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most %d rows: the weight buckets of a class are kept in LDS)", who,
                 (long long)n, kMetLdsKeys);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_bootstrap_weights(uint64_t seed, uint32_t first_replicate, int replicates, int64_t n, int32_t* weights, int64_t ld_w,
                          void* stream) {
    const char* who = "acx_bootstrap_weights";
    if (!weights) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (replicates < 1) ACX_FAIL(ACX_ERR_ARG, "%s: %d replicates (expected >= 1)", who, replicates);
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kMetMaxN) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    if ((uint64_t)first_replicate + (uint64_t)replicates > (1ULL << 32))
        ACX_FAIL(ACX_ERR_ARG, "%s: replicates %u .. %llu (replicate numbers are below 2^32)", who, first_replicate,
                 (unsigned long long)first_replicate + (unsigned long long)replicates - 1);
    if (ld_w < n) ACX_FAIL(ACX_ERR_ARG, "%s: row stride %lld is shorter than n = %lld", who, (long long)ld_w, (long long)n);
    const hipStream_t s = (hipStream_t)stream;
    if (ld_w == n) ACX_HIP(hipMemsetAsync(weights, 0, (size_t)replicates * (size_t)n * 4, s));
    else ACX_HIP(hipMemset2DAsync(weights, (size_t)ld_w * 4, 0, (size_t)n * 4, (size_t)replicates, s));
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(replicates < 65535 ? replicates : 65535));
    launch_kernel(&bootstrap_weights_kernel, grid, dim3(256), 0, s, (unsigned long long)boot_mix(seed), (unsigned)first_replicate,
                  replicates, (int)n, (int*)weights, (long long)ld_w);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_weighted_metrics_workspace_bytes(int64_t n, int classes, size_t* out_bytes) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_weighted_metrics_workspace_bytes: out_bytes is null");
    ACX_TRY(weighted_check_shape("acx_weighted_metrics_workspace_bytes", n, classes));
    size_t a, b, c;
    weighted_layout(n, classes, &a, &b, &c, out_bytes);
    return ACX_OK;
}

int acx_weighted_metrics(const float* scores, int64_t ld_scores, const void* target, int target_dtype, int64_t ld_target,
                         int64_t n, int classes, const int32_t* weights, int64_t ld_w, int replicates, double* ap, double* auc,
                         double* dprime, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "acx_weighted_metrics";
    if (!weights || !ap || !auc || !dprime || !ws) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(met_check_inputs(who, scores, ld_scores, target, target_dtype, ld_target, n, classes, status));
    ACX_TRY(weighted_check_shape(who, n, classes));
    if (replicates < 1) ACX_FAIL(ACX_ERR_ARG, "%s: %d replicates (expected >= 1)", who, replicates);
    if (ld_w < n) ACX_FAIL(ACX_ERR_ARG, "%s: weight row stride %lld is shorter than n = %lld", who, (long long)ld_w, (long long)n);
    size_t soff, boff, poff, need;
    weighted_layout(n, classes, &soff, &boff, &poff, &need);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, need));
    const hipStream_t s = (hipStream_t)stream;
    MetPrep m;
    ACX_TRY(met_prepare(who, scores, ld_scores, target, target_dtype, ld_target, n, classes, status, ws, ws_bytes, s, &m));
    char* w = static_cast<char*>(ws);
    unsigned short* slots = reinterpret_cast<unsigned short*>(w + soff);
    unsigned* nbounds = reinterpret_cast<unsigned*>(w + boff);
    int* npos = reinterpret_cast<int*>(w + poff);
    launch_kernel(&weights_check_kernel, dim3(replicates < 4096 ? replicates : 4096), dim3(256), 0, s, (const int*)weights,
                  (long long)ld_w, (int)n, replicates, (int*)status);
    ACX_HIP(hipGetLastError());
    {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &weighted_plan_kernel, (size_t)kMetLdsKeys * 4));
    }
    launch_kernel(&weighted_plan_kernel, dim3(classes), dim3(kMetThreads), (size_t)n * 4, s, (const unsigned*)m.keys,
                  (const unsigned char*)m.labs, (int)n, (const int*)status, slots, nbounds, npos);
    ACX_HIP(hipGetLastError());
    {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &weighted_recount_kernel, (size_t)kMetLdsKeys * 4));
    }
    for (int r0 = 0; r0 < replicates; r0 += 65535) {         // (a grid's second dimension ends at 65535)
        const int rows = replicates - r0 < 65535 ? replicates - r0 : 65535;
        launch_kernel(&weighted_recount_kernel, dim3(classes, rows), dim3(kMetThreads), (size_t)n * 4, s,
                      (const unsigned short*)slots, (const unsigned*)nbounds, (const int*)npos, (int)n, classes,
                      (const int*)weights, (long long)ld_w, r0, (const int*)status, ap, auc, dprime);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
