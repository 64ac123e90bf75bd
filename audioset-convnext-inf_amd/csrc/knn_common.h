// What the fp32 search (knn.hip) and the int8 search (knn_i8.hip) share: the register sort of the 64-bit keys, the candidate
// buffers of a query tile in LDS (take a slot, trim a full buffer to its k best, write a slice's list), and the launch plan
// of a search with its workspace size.  The keys themselves are device_common.h's (knn_make_key: one total order).
#pragma once
#include <algorithm>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kKnnThreads = 256;
constexpr int kKnnStepRows = 256;            // database rows per step of a workgroup: four waves x 64
constexpr int kKnnTargetWgs = 512;           // the slice count aims at this many workgroups: two per CU of an MI355X
constexpr int kKnnMaxSlices = 1024;

// Element e = lane + 64 r of a wave's 64 R keys, sorted descending (bitonic network: strides under 64 by lane shuffles, the
// others between the lane's own registers).
template <int R>
__device__ __forceinline__ void knn_sort_desc(knn_key (&v)[R], int lane) {
#pragma unroll
    for (int size = 2; size <= 64 * R; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j >= 1; j >>= 1) {
            if (j >= 64) {
                const int jr = j >> 6;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if ((r & jr) == 0) {
                        const bool desc = ((r << 6) & size) == 0;
                        const knn_key a = v[r], b = v[r | jr];
                        const bool sw = desc ? (a < b) : (a > b);
                        v[r] = sw ? b : a;
                        v[r | jr] = sw ? a : b;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const bool desc = ((lane + (r << 6)) & size) == 0;
                    const bool lower = (lane & j) == 0;
                    const knn_key o = __shfl_xor(v[r], j);
                    const knn_key hi = v[r] > o ? v[r] : o, lo = v[r] > o ? o : v[r];
                    v[r] = (lower == desc) ? hi : lo;
                }
            }
        }
    }
}

// v[] <- the cnt keys of buf (the other elements 0), sorted descending.  One wave.
template <int R>
__device__ __forceinline__ void knn_load_sorted(const knn_key* buf, int cnt, knn_key (&v)[R], int lane) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        v[r] = e < cnt ? buf[e] : 0ull;
    }
    knn_sort_desc<R>(v, lane);
}

// ---- the candidate buffers of a query tile (LDS): per query CAP = 64 R slots, a count and a threshold key ----------------------
// A key that beats its query's threshold takes a slot by an LDS atomic on the count.  false: no slot was left -- the caller
// keeps the candidate, raises the workgroup's `over` flag and offers it again after the trim.
template <int CAP>
__device__ __forceinline__ bool knn_offer(knn_key key, int ql, const knn_key* s_thr, int* s_cnt, knn_key* s_buf) {
    if (key > s_thr[ql]) {
        const int slot = atomicAdd(&s_cnt[ql], 1);
        if (slot < CAP) s_buf[ql * CAP + slot] = key;
        else return false;
    }
    return true;
}

// Every query of the tile whose buffer ran full: one wave sorts its CAP keys, keeps the first k and raises the threshold to the
// k-th.  Called by the whole workgroup between two barriers.
template <int R>
__device__ __forceinline__ void knn_trim_full(int tq, int k, knn_key* s_thr, int* s_cnt, knn_key* s_buf, int wave, int lane) {
    constexpr int CAP = 64 * R;
    for (int ql = wave; ql < tq; ql += 4) {
        const int cnt = s_cnt[ql];           // wave-uniform
        if (cnt >= CAP) {
            knn_key v[R];
            knn_load_sorted<R>(s_buf + ql * CAP, CAP, v, lane);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int e = lane + 64 * r;
                s_buf[ql * CAP + e] = v[r];
                if (e == k - 1) s_thr[ql] = v[r];
            }
            if (lane == 0) s_cnt[ql] = k;
        }
    }
}

// The slice's k best of each query of the tile, sorted, to the workspace [nq][slices][k] (0 keys where the slice holds fewer
// than k candidates).
template <int R>
__device__ __forceinline__ void knn_store_slice(int tq, long long q0, long long nq, int k, int slices, int slice, knn_key* ws,
                                                const int* s_cnt, const knn_key* s_buf, int wave, int lane) {
    constexpr int CAP = 64 * R;
    for (int ql = wave; ql < tq; ql += 4) {
        if (q0 + ql >= nq) break;
        knn_key v[R];
        knn_load_sorted<R>(s_buf + ql * CAP, min(s_cnt[ql], CAP), v, lane);
        knn_key* out = ws + ((q0 + ql) * slices + slice) * k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            if (e < k) out[e] = v[r];
        }
    }
}

// ---- host: the launch shape of a search ---------------------------------------------------------------------------------------
struct KnnPlan { int qt, r, slices; long long slice_rows; };

// A function of (nq, n, k) and ACX_KNN_SLICE_ROWS alone.
inline KnnPlan knn_plan(long long nq, long long n, int k) {
    KnnPlan pl;
    pl.qt = nq <= 32 ? 1 : 2;
    pl.r = k <= 32 ? 1 : k <= 64 ? 2 : 4;
    const long long qtiles = cdiv(nq, 32 * pl.qt);
    const int forced = tuning().knn_slice_rows.load(std::memory_order_relaxed);
    long long rows, slices;
    if (forced > 0) {
        rows = forced;
        if (cdiv(n, rows) > kKnnMaxSlices) rows = cdiv(n, kKnnMaxSlices);
    } else {
        slices = std::min(std::max(cdiv(kKnnTargetWgs, qtiles), 1LL), cdiv(n, kKnnStepRows));
        rows = cdiv(cdiv(n, slices), kKnnStepRows) * kKnnStepRows;
    }
    slices = cdiv(n, rows);
    pl.slices = (int)slices;
    pl.slice_rows = rows;
    return pl;
}

// Workspace: nq * slices lists of k keys.  The bound below covers every plan and is non-decreasing in nq, n and k:
// nq * slices <= nq * ceil(n / 256), and <= 64 * 512 + nq because slices <= ceil(512 / qtiles) and nq <= 64 qtiles.
inline size_t knn_ws_bytes(long long nq, long long n, int k) {
    const int forced = tuning().knn_slice_rows.load(std::memory_order_relaxed);
    long long cells;
    if (forced > 0) cells = nq * std::min<long long>(kKnnMaxSlices, cdiv(n, forced));
    else cells = std::min(nq * cdiv(n, kKnnStepRows), 64LL * kKnnTargetWgs + nq);
    return align_up((size_t)cells * (size_t)k * sizeof(knn_key));
}

inline int knn_check_shape(const char* who, int64_t nq, int64_t n, int k) {
    if (nq < 1) ACX_FAIL(ACX_ERR_ARG, "%s: nq = %lld (expected >= 1)", who, (long long)nq);
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (k < 1 || k > ACX_KNN_MAX_K) ACX_FAIL(ACX_ERR_ARG, "%s: k = %d (expected 1 .. %d)", who, k, ACX_KNN_MAX_K);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    if (nq > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: nq = %lld (at most 2^30 queries per call)", who, (long long)nq);
    return ACX_OK;
}

// knn.hip: the merge of the slices' lists of nq queries (ws [nq][slices][k], r = 1 / 2 / 4 the plan's) into indices / scores;
// one launch on s.
int knn_launch_merge(const knn_key* ws, long long nq, int slices, int k, int r, int* indices, float* scores, const int* status,
                     hipStream_t s);

}  // namespace acx
