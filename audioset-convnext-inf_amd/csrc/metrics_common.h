// What metrics.hip (acx_tagging_metrics, acx_operating_points) and bootstrap.hip (acx_weighted_metrics) share: the sizes, the key
// order's primitives -- bitonic comparators, bounds in a sorted run, the split of a class into its two runs -- and the host side
// that checks the arguments, lays out the workspace and launches metrics_prep_kernel.
#pragma once
#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kMetThreads = 1024;                 // one workgroup per class
constexpr int kMetWaves = kMetThreads / 64;
constexpr int kMetLdsKeys = 32768;                // N <= this: both runs sorted in LDS (128 KiB); beyond: LDS chunks of this size
constexpr int kMetTile = 64;                      // prep: 64 rows x 64 classes per workgroup of 256 threads
constexpr long long kMetMaxN = 1LL << 30;

__device__ __forceinline__ int met_pow2(int n) { return n <= 1 ? 1 : 1 << (32 - __clz(n - 1)); }

// comparator t of stage (k, j) of the bitonic network that sorts ascending with every comparator (lo < hi) putting the smaller
// key at lo: the first stage of each block of k pairs r with k - 1 - r, the others are half-cleaners of distance j.  Over a run
// of n keys padded to a power of two with +infinity, every comparator with hi >= n leaves both keys in place: it is skipped.
__device__ __forceinline__ void met_pair(int t, int k, int j, int& lo, int& hi) {
    lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    hi = (j == (k >> 1)) ? (lo ^ (k - 1)) : (lo + j);
}

template <typename T>
__device__ __forceinline__ void met_cmpx(T* a, int lo, int hi) {
    const unsigned x = a[lo], y = a[hi];
    if (x > y) { a[lo] = y; a[hi] = x; }
}

// first index of a[0, n) with a[i] >= t (upper = false) or a[i] > t (upper = true); a sorted ascending
template <typename T>
__device__ __forceinline__ int met_bound(const T* a, int n, unsigned t, bool upper) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned v = a[mid];
        if (v < t || (upper && v == t)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// stages k = k_first .. k_last (all their half-cleaners) over s[0, m), m <= kMetLdsKeys, in LDS
__device__ void met_lds_network(unsigned* s, int m, int k_first, int k_last) {
    const int half = met_pow2(m) >> 1;
    for (int k = k_first; k <= k_last; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += kMetThreads) {
                int lo, hi;
                met_pair(t, k, j, lo, hi);
                if (hi < m) met_cmpx(s, lo, hi);
            }
            __syncthreads();
        }
}


// the keys of class c split into positives (from dst[0] up) and negatives (from dst[n - 1] down); returns P (all threads)
template <typename T>
__device__ int met_split(const unsigned* __restrict__ key, const unsigned char* __restrict__ lab, int n, T* dst, int* s_cnt) {
    if (threadIdx.x == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    const int lane = __lane_id();
    const unsigned long long below = (1ULL << lane) - 1;
    for (int i0 = 0; i0 < n; i0 += kMetThreads) {
        const int i = i0 + threadIdx.x;
        const bool in = i < n;
        const unsigned k = in ? key[i] : 0u;
        const bool pos = in && lab[i];
        const unsigned long long bp = __ballot(pos), bn = __ballot(in && !pos);
        int bpos = 0, bneg = 0;
        if (lane == 0) {
            bpos = atomicAdd(&s_cnt[0], __popcll(bp));
            bneg = atomicAdd(&s_cnt[1], __popcll(bn));
        }
        bpos = __shfl(bpos, 0);
        bneg = __shfl(bneg, 0);
        if (pos) dst[bpos + __popcll(bp & below)] = k;
        else if (in) dst[n - 1 - (bneg + __popcll(bn & below))] = k;
    }
    __syncthreads();
    return s_cnt[0];
}

// what the sorting calls share: the argument checks, the cleared status word and the keys / labels of the workspace
struct MetPrep {
    unsigned* keys;
    unsigned char* labs;
    unsigned* runs;
};

// metrics.hip
void met_layout(long long n, long long C, size_t* keys_off, size_t* labs_off, size_t* runs_off, size_t* total);
int met_check_shape(int64_t n, int classes);
int met_check_inputs(const char* who, const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                     int64_t ld_target, int64_t n, int classes, const int32_t* status);
int met_prepare(const char* who, const float* scores, int64_t ld_scores, const void* target, int target_dtype, int64_t ld_target,
                int64_t n, int classes, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s, MetPrep* m);

}  // namespace acx
