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

// Per recording, each kernel takes the offsets it needs -- first sample, first window (or probs row), first timeline row -- as
// serial prefixes over R <= 256 by thread 0 (packed.h).

// wstart[i] = absolute sample offset of window first + i, i < count
__global__ __launch_bounds__(256) void window_table_kernel(PackedLens a, long long W, long long H, long long first, int count,
                                                           long long* __restrict__ wstart) {
    __shared__ long long soff[kVarMaxClips + 1], woff[kVarMaxClips + 1];
    if (threadIdx.x == 0) {
        packed_prefix(a.n, soff, [&a](int r) { return (long long)a.len[r]; });
        packed_prefix(a.n, woff, [&a, W, H](int r) { return win_count(a.len[r], W, H); });
    }
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const long long g = first + i;
        const int r = packed_find(woff, a.n, g);
        wstart[i] = soff[r] + win_start(g - woff[r], a.len[r], W, H);
    }
}

// One workgroup per timeline row (grid-stride), threads striding over the row's N classes.  Row k of recording r has the
// midpoint m = win_mid(k, H, L_r) and is reduced over the windows that cover it (win_cover).  mean: an fp32 sum in ascending
// j, then one division by the count; max: the largest value (win_reduce).
__global__ __launch_bounds__(256) void window_timeline_kernel(PackedLens a, long long W, long long H, const float* __restrict__ probs,
                                                              int N, int reduce, float* __restrict__ out) {
    __shared__ long long woff[kVarMaxClips + 1], toff[kVarMaxClips + 1];
    // every workgroup waits for its prefixes before its first row: the two run side by side, on the first lanes of two waves
    if (threadIdx.x == 0) packed_prefix(a.n, woff, [&a, W, H](int r) { return win_count(a.len[r], W, H); });
    if (threadIdx.x == 64) packed_prefix(a.n, toff, [&a, H](int r) { return win_steps(a.len[r], H); });
    __syncthreads();
    const long long rows = toff[a.n];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int r = packed_find(toff, a.n, row);
        const long long L = a.len[r];
        long long j0, j1;
        win_cover(win_mid(row - toff[r], H, L), L, W, H, &j0, &j1);
        const float* pr = probs + woff[r] * N;
        for (int c = threadIdx.x; c < N; c += 256)
            out[row * N + c] = win_reduce([pr, N](long long j) { return pr + j * N; }, j0, j1 - j0, c, reduce);
    }
}

// The timeline at segment resolution (acx_segment_timeline).  Window j of recording r holds min(W, L_r) samples and
// S_r = seg_count(min(W, L_r)) segments of 10240 samples, the last one reaching to the window's end; probs holds the windows'
// (S_r, N) blocks in window order.  Row k of recording r has the midpoint m = win_mid(k, 10240, L_r); each window that covers
// it contributes the one segment min((m - s_j) / 10240, S_r - 1).
__host__ __device__ __forceinline__ long long seg_steps(long long L) { return (L + kSegSamples - 1) / kSegSamples; }
__global__ __launch_bounds__(256) void segment_timeline_kernel(PackedLens a, long long W, long long H, const float* __restrict__ probs,
                                                               int N, int reduce, float* __restrict__ out) {
    __shared__ long long woff[kVarMaxClips + 1], toff[kVarMaxClips + 1];       // woff: the first probs row of recording r
    if (threadIdx.x == 0)                                       // side by side, as in window_timeline_kernel
        packed_prefix(a.n, woff, [&a, W, H](int r) {
            const long long L = a.len[r];
            return win_count(L, W, H) * seg_count(L < W ? L : W);
        });
    if (threadIdx.x == 64) packed_prefix(a.n, toff, [&a](int r) { return seg_steps(a.len[r]); });
    __syncthreads();
    const long long rows = toff[a.n];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int r = packed_find(toff, a.n, row);
        const long long L = a.len[r], m = win_mid(row - toff[r], kSegSamples, L);
        const int Sr = seg_count(L < W ? L : W);
        long long j0, j1;
        win_cover(m, L, W, H, &j0, &j1);
        const float* pr = probs + woff[r] * N;
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

int launch_window_table(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t first, int count, long long* wstart,
                        hipStream_t s) {
    const unsigned blocks = (unsigned)((count + 255) / 256);
    launch_kernel(&window_table_kernel, dim3(blocks), dim3(256), 0, s, packed_lens(lengths, R), (long long)window, (long long)hop,
                  (long long)first, count, wstart);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// one workgroup per timeline row, 4096 at most; `steps`: the rows of a recording of L samples
template <class Kernel, class Steps>
static int timeline_launch(Kernel kernel, Steps steps, const float* probs, int classes, const int64_t* lengths, int R,
                           int64_t window, int64_t hop, int reduce, float* out, hipStream_t s) {
    long long toff[kVarMaxClips + 1];
    const long long rows = packed_prefix(R, toff, [&](int r) { return steps(lengths[r]); });
    if (rows == 0) return ACX_OK;
    const unsigned blocks = (unsigned)(rows < 4096 ? rows : 4096);
    launch_kernel(kernel, dim3(blocks), dim3(256), 0, s, packed_lens(lengths, R), (long long)window, (long long)hop, probs, classes,
                  reduce, out);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_window_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                           int reduce, float* out, hipStream_t s) {
    return timeline_launch(&window_timeline_kernel, [hop](long long L) { return win_steps(L, hop); }, probs, classes, lengths, R,
                           window, hop, reduce, out, s);
}

int launch_segment_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                            int reduce, float* out, hipStream_t s) {
    return timeline_launch(&segment_timeline_kernel, [](long long L) { return seg_steps(L); }, probs, classes, lengths, R, window,
                           hop, reduce, out, s);
}

}  // namespace acx
