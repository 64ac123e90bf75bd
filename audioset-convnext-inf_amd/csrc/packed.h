// Packed batches: several clips, recordings or slots of different lengths lying back to back in one call (varlen, resample,
// windows, stream, segments, events, the log-mel frontend).  The indexing rules of such a call are defined here ONCE: the
// lengths by value, the prefix sums over per-entry counts, the search for the entry that owns a flat index, and the windows of a
// recording with the run of them that covers a timeline midpoint.  Kept free of HIP-only constructs, as fft_core.h is, so that
// tests/packed_check.cpp runs the very same functions on the CPU.
#pragma once
#include "../../include/acx.h"

#ifndef ACX_HD
#if defined(__HIPCC__)
#define ACX_HD __host__ __device__ __forceinline__
#else
#define ACX_HD inline
#endif
#endif

namespace acx {

constexpr int kVarMaxClips = ACX_MAX_VARLEN_CLIPS;

// The lengths (or per-entry counts) of a call's n <= kVarMaxClips entries, handed to a kernel BY VALUE (1 KiB of kernel
// argument): the call copies nothing from the host, allocates and synchronises nothing, and stays capturable.
struct PackedLens {
    int n;
    int len[kVarMaxClips];
};
// from a HOST array the caller has checked: 1 <= n <= kVarMaxClips, every length in [0, 2^31)
template <class I>
inline PackedLens packed_lens(const I* lengths, int n) {
    PackedLens a{};
    a.n = n;
    for (int i = 0; i < n; ++i) a.len[i] = (int)lengths[i];
    return a;
}

// The serial exclusive prefix of n per-entry counts: off[0] = 0, off[i + 1] = off[i] + count(i); returns the total off[n].
// No barrier inside: a kernel wraps its prefixes in `if (threadIdx.x == 0) { ... } __syncthreads();` (n <= 256: a few
// microseconds at most), and a launcher calls the same function with the same counts for its totals and grid sizes.
template <class T, class Count>
ACX_HD T packed_prefix(int n, T* off, Count count) {
    T t = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = t;
        t += count(i);
    }
    off[n] = t;
    return t;
}

// The entry that owns flat index v: the largest i in [0, n) with off[i] + gap * i <= v, for ascending off with off[0] = 0 <= v
// (int or long long offsets; gap: units between entries that belong to the entry before them, the zero rows of varlen.hip).
// Ties: with gap = 0, entries of count 0 share their offset with their successor and the LAST entry at that offset is returned,
// so for any v < off[n] the result i has off[i] <= v < off[i + 1]: the entry that really holds v, never an empty one.
template <class T>
ACX_HD int packed_find(const T* off, int n, long long v, int gap = 0) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] + (T)gap * mid <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the window definition (include/acx.h), shared by windows.hip and stream.hip ----------------------------------------------
// Windows of a recording of L samples, the start of window j, and the timeline steps.
ACX_HD long long win_count(long long L, long long W, long long H) { return L <= W ? 1 : 1 + (L - W + H - 1) / H; }
ACX_HD long long win_start(long long j, long long L, long long W, long long H) {
    const long long last = L > W ? L - W : 0;
    return j * H < last ? j * H : last;
}
ACX_HD long long win_steps(long long L, long long H) { return (L + H - 1) / H; }
// the midpoint of timeline row k at `step` samples per row: k step + step / 2, held inside the recording
ACX_HD long long win_mid(long long k, long long step, long long L) {
    const long long m = k * step + step / 2;
    return m > L - 1 ? L - 1 : m;
}
// The windows [j0, j1) that cover sample m, 0 <= m < L: those with s_j <= m < s_j + W are a run of consecutive j, from the
// first with j H > m - W (an earlier window ends at or before m) up to the last with s_j <= m (s_j does not decrease).  Never
// empty: j0 itself qualifies (j0 H <= m - W + H <= m).
ACX_HD void win_cover(long long m, long long L, long long W, long long H, long long* j0, long long* j1) {
    const long long n = win_count(L, W, H), first = m >= W ? (m - W) / H + 1 : 0;
    long long last = first;
    while (last < n && win_start(last, L, W, H) <= m) ++last;
    *j0 = first;
    *j1 = last;
}

}  // namespace acx
