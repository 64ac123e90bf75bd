// Sliding windows over long recordings (acx_forward_windows, acx_window_timeline).  R recordings of L_r samples lie back to
// back; window j of recording r covers [s_j, s_j + min(W, L_r)) with s_j = min(j H, max(0, L_r - W)), so the last window
// ends with the recording.  The windows are numbered recording by recording, then by j.
//
// The forward of a run of windows is the UNIFORM B = count, L = W pipeline; only the frontend differs: it reads window b's
// samples at the absolute offset the window table holds (frontend.hip, kFrontWin).  The table is written by one kernel that
// gets the lengths BY VALUE, so the call stays free of host -> device copies, allocations and synchronisation (capturable),
// as varlen_tables_kernel does for variable-length batches.
#include "acx_internal.h"
#include "device_common.h"

namespace acx {

struct WinArgs {
    int R;
    long long W, H;
    int len[kVarMaxClips];
};

// largest i in [0, R) with off[i] <= v (off ascending, off[0] = 0 <= v)
__device__ __forceinline__ int win_find(const long long* off, int R, long long v) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Per recording: first sample, first window and (timeline) first step -- a serial prefix over R <= 256 by one thread.
struct WinPrefix {
    long long soff[kVarMaxClips], woff[kVarMaxClips], toff[kVarMaxClips + 1];
};
__device__ void win_prefix(const WinArgs& a, WinPrefix& p) {
    if (threadIdx.x == 0) {
        long long s = 0, w = 0, t = 0;
        for (int r = 0; r < a.R; ++r) {
            p.soff[r] = s; p.woff[r] = w; p.toff[r] = t;
            s += a.len[r];
            w += win_count(a.len[r], a.W, a.H);
            t += win_steps(a.len[r], a.H);
        }
        p.toff[a.R] = t;
    }
    __syncthreads();
}

// wstart[i] = absolute sample offset of window first + i, i < count
__global__ __launch_bounds__(256) void window_table_kernel(WinArgs a, long long first, int count, long long* __restrict__ wstart) {
    __shared__ WinPrefix p;
    win_prefix(a, p);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const long long g = first + i;
        const int r = win_find(p.woff, a.R, g);
        wstart[i] = p.soff[r] + win_start(g - p.woff[r], a.len[r], a.W, a.H);
    }
}

// One workgroup per timeline row (grid-stride), threads striding over the row's N classes.  Row k of recording r has the
// midpoint m = min(k H + H / 2, L_r - 1); the windows with s_j <= m < s_j + W are a run of consecutive j: those with j H > m - W
// (an earlier window ends at or before m) up to the last with s_j <= m (s_j does not decrease).  mean: an fp32 sum in ascending
// j, then one division by the count; max: the largest value.
__global__ __launch_bounds__(256) void window_timeline_kernel(WinArgs a, const float* __restrict__ probs, int N, int reduce,
                                                              float* __restrict__ out) {
    __shared__ WinPrefix p;
    win_prefix(a, p);
    const long long rows = p.toff[a.R];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int r = win_find(p.toff, a.R, row);
        const long long L = a.len[r], k = row - p.toff[r], n = win_count(L, a.W, a.H);
        long long m = k * a.H + a.H / 2;
        if (m > L - 1) m = L - 1;
        const long long j0 = m >= a.W ? (m - a.W) / a.H + 1 : 0;
        long long j1 = j0;                                 // at least one window qualifies (j0 itself: j0 H <= m - W + H <= m)
        while (j1 < n && win_start(j1, L, a.W, a.H) <= m) ++j1;
        const float* pr = probs + p.woff[r] * N;
        for (int c = threadIdx.x; c < N; c += 256)
            out[row * N + c] = win_reduce([pr, N](long long j) { return pr + j * N; }, j0, j1 - j0, c, reduce);
    }
}

// The timeline at segment resolution (acx_segment_timeline).  Window j of recording r holds min(W, L_r) samples and
// S_r = seg_count(min(W, L_r)) segments of 10240 samples, the last one reaching to the window's end; probs holds the windows'
// (S_r, N) blocks in window order.  Row k of recording r has the midpoint m = min(10240 k + 5120, L_r - 1); the windows that
// cover it are the run of window_timeline_kernel, and each contributes the one segment min((m - s_j) / 10240, S_r - 1).
struct SegWinPrefix {
    long long poff[kVarMaxClips], toff[kVarMaxClips + 1];       // first probs row / first timeline row of recording r
};
__global__ __launch_bounds__(256) void segment_timeline_kernel(WinArgs a, const float* __restrict__ probs, int N, int reduce,
                                                               float* __restrict__ out) {
    __shared__ SegWinPrefix p;
    if (threadIdx.x == 0) {
        long long w = 0, t = 0;
        for (int r = 0; r < a.R; ++r) {
            const long long L = a.len[r];
            p.poff[r] = w; p.toff[r] = t;
            w += win_count(L, a.W, a.H) * seg_count(L < a.W ? L : a.W);
            t += (L + kSegSamples - 1) / kSegSamples;
        }
        p.toff[a.R] = t;
    }
    __syncthreads();
    const long long rows = p.toff[a.R];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int r = win_find(p.toff, a.R, row);
        const long long L = a.len[r], k = row - p.toff[r], n = win_count(L, a.W, a.H);
        const int Sr = seg_count(L < a.W ? L : a.W);
        long long m = k * kSegSamples + kSegSamples / 2;
        if (m > L - 1) m = L - 1;
        const long long j0 = m >= a.W ? (m - a.W) / a.H + 1 : 0;
        long long j1 = j0;
        while (j1 < n && win_start(j1, L, a.W, a.H) <= m) ++j1;
        const float* pr = probs + p.poff[r] * N;
        const long long W = a.W, H = a.H;
        auto seg_row = [pr, N, Sr, m, L, W, H](long long j) {
            long long i = (m - win_start(j, L, W, H)) / kSegSamples;
            if (i > Sr - 1) i = Sr - 1;
            return pr + (j * Sr + i) * N;
        };
        for (int c = threadIdx.x; c < N; c += 256) out[row * N + c] = win_reduce(seg_row, j0, j1 - j0, c, reduce);
    }
}

int window_check(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t* n_windows) {
    if (window < ACX_MIN_SAMPLES)
        ACX_FAIL(ACX_ERR_SHAPE,
                 "window of %lld samples is too short: the last 2x2 downsample needs at least %d samples "
                 "(kernel size can't be greater than actual input size)", (long long)window, ACX_MIN_SAMPLES);
    if (window > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "window of %lld samples is longer than 2^31 - 1", (long long)window);
    if (hop < 1 || hop > window)
        ACX_FAIL(ACX_ERR_ARG, "hop of %lld samples (expected 1 .. window = %lld: a longer hop leaves audio uncovered)",
                 (long long)hop, (long long)window);
    if (R <= 0 || R > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "%d recordings (expected 1 .. %d)", R, kVarMaxClips);
    if (!lengths) ACX_FAIL(ACX_ERR_ARG, "windows: lengths is null");
    int64_t n = 0;
    for (int r = 0; r < R; ++r) {
        if (lengths[r] < 0 || lengths[r] > 0x7fffffffLL)
            ACX_FAIL(ACX_ERR_ARG, "recording %d has %lld samples (expected 0 .. 2^31 - 1)", r, (long long)lengths[r]);
        n += win_count(lengths[r], window, hop);
    }
    if (n_windows) *n_windows = n;
    return ACX_OK;
}

static WinArgs win_args(const int64_t* lengths, int R, int64_t window, int64_t hop) {
    WinArgs a{};
    a.R = R; a.W = window; a.H = hop;
    for (int r = 0; r < R; ++r) a.len[r] = (int)lengths[r];
    return a;
}

int launch_window_table(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t first, int count, long long* wstart,
                        hipStream_t s) {
    const unsigned blocks = (unsigned)((count + 255) / 256);
    launch_kernel(&window_table_kernel, dim3(blocks), dim3(256), 0, s, win_args(lengths, R, window, hop), (long long)first,
                  count, wstart);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_window_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                           int reduce, float* out, hipStream_t s) {
    long long rows = 0;
    for (int r = 0; r < R; ++r) rows += win_steps(lengths[r], hop);
    if (rows == 0) return ACX_OK;
    const unsigned blocks = (unsigned)(rows < 4096 ? rows : 4096);
    launch_kernel(&window_timeline_kernel, dim3(blocks), dim3(256), 0, s, win_args(lengths, R, window, hop), probs, classes, reduce,
                  out);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_segment_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                            int reduce, float* out, hipStream_t s) {
    long long rows = 0;
    for (int r = 0; r < R; ++r) rows += (lengths[r] + kSegSamples - 1) / kSegSamples;
    if (rows == 0) return ACX_OK;
    const unsigned blocks = (unsigned)(rows < 4096 ? rows : 4096);
    launch_kernel(&segment_timeline_kernel, dim3(blocks), dim3(256), 0, s, win_args(lengths, R, window, hop), probs, classes,
                  reduce, out);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx
