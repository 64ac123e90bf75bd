// Event decoding on the device (include/acx.h "sound event decoding"): probabilities over time -> one compact, ordered table of
// events, the batched form of pytorch/segments.py::decode_events.
//
// One WAVE per (clip, 64 classes), a lane per class, walking down time: every row read is one coalesced 256-byte line, and each
// lane runs the whole per-column state machine -- running median, hysteresis runs, merge, minimum duration -- in registers.
// Three launches on the caller's stream, no atomics that could order anything:
//   events_kernel<.., false>  counts the events of every column (counts[unit][lane]) and of every wave (unit_off[unit]);
//   events_scan_kernel        turns the wave totals into exclusive offsets, writes *count and the overflow bit;
//   events_kernel<.., true>   walks again and writes event i of a column at offset(unit) + prefix(lane) + i.
// The table is therefore ordered by (clip, class, begin) and has the same bits on every call.
//
// The median is a per-lane SORTED sliding window: stepping removes the value that leaves and inserts the value that enters in
// one pass over the window (one compare-select chain per slot, no sort).  Widths up to kEvRegMedian live in registers, wider
// ones in LDS as [slot][lane] (conflict-free: a lane only ever touches its own column of banks).  The value that leaves is
// re-read from memory (row t - median / 2, a line the wave read median rows earlier).  Both row streams are loaded kEvDepth
// rows ahead of their use.
//
// The window and the column state machine live in events_common.h, shared with the online decoder (events_online.hip).
//
// float64 appears only where decode_events has it: the boundaries (k * step_seconds), their differences against merge_gap /
// min_duration, and the sum behind an event's mean.  Built with -fno-slp-vectorize like segments.hip (csrc/Makefile).
#include "events_common.h"

namespace acx {

template <int WR, bool EMIT>
__global__ __launch_bounds__(64) void events_kernel(EvArgs a) {
    extern __shared__ float s_win[];
    const int lane = threadIdx.x;
    const long long unit = blockIdx.x;
    const int clip = (int)(unit / a.G), g = (int)(unit - (long long)clip * a.G);
    const int cls = g * 64 + lane;
    const bool live = cls < a.N;

    long long base = 0;
    if constexpr (EMIT) {
        if (*a.status & (ACX_EVENTS_NONFINITE | ACX_EVENTS_BAD_THRESHOLD)) return;
        // exclusive prefix of the lanes' counts; a unit without events has nothing to write
        const int mine = a.counts[unit * 64 + lane];
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (__shfl(incl, 63, 64) == 0) return;
        base = a.unit_off[unit] + (incl - mine);
        if (base >= a.capacity) base = a.capacity;     // nothing of this column fits; keeps base + n from wrapping
    }

    int steps = a.steps;
    long long row0 = (long long)clip * a.steps;
    double end = a.end;
    if (a.tab_steps) { steps = a.tab_steps[clip]; row0 = a.tab_row0[clip]; end = a.tab_end[clip]; }
    const int col_of = live ? cls : a.N - 1;                              // idle lanes re-read the last class: in bounds
    const float* x = a.probs + row0 * a.ld + col_of;
    // the lane's own two levels, loaded once
    const float thr = a.thr_c ? a.thr_c[col_of] : a.thr;
    const float low = a.low_c ? a.low_c[col_of] : a.thr_c ? thr : a.low;
    const int h = a.median / 2, last = steps - 1;
    auto row = [&](int r) { return x[(long long)(r < 0 ? 0 : r > last ? last : r) * a.ld]; };

    EvWindow<WR> win;
    win.l = s_win + lane;
    win.w = a.median;
    const float x0 = row(0);
    bool bad = ev_nonfinite(x0);
    if constexpr (WR != 1) {
        // the window of t = 0: rows -h .. h with the ends repeated
        win.fill(x0);
        for (int j = 1; j <= h; ++j) {
            const float v = row(j);
            bad = bad || ev_nonfinite(v);
            win.update(x0, v);
        }
    } else {
        win.r[0] = x0;
    }

    EvColumn<EMIT> col(a, steps, end, live, thr, low, clip, cls, base);
    // step t reads the window's median, then trades row t - h for row t + h + 1; both streams run kEvDepth rows ahead
    float cin[kEvDepth], cout[kEvDepth], nin[kEvDepth], nout[kEvDepth];
#pragma unroll
    for (int j = 0; j < kEvDepth; ++j) {
        cin[j] = row(j + h + 1);
        cout[j] = WR == 1 ? 0.f : row(j - h);
    }
    for (int t0 = 0; t0 < steps; t0 += kEvDepth) {
#pragma unroll
        for (int j = 0; j < kEvDepth; ++j) {      // (rows past the end clamp to the last one: in bounds, unused)
            nin[j] = row(t0 + kEvDepth + j + h + 1);
            nout[j] = WR == 1 ? 0.f : row(t0 + kEvDepth + j - h);
        }
#pragma unroll
        for (int j = 0; j < kEvDepth; ++j) {
            const int t = t0 + j;
            if (t < steps) {
                col.step(t, win.median());
                bad = bad || ev_nonfinite(cin[j]);
                if constexpr (WR == 1) win.r[0] = cin[j];
                else win.update(cout[j], cin[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kEvDepth; ++j) { cin[j] = nin[j]; cout[j] = nout[j]; }
    }
    col.finish();

    if constexpr (!EMIT) {
        a.counts[unit * 64 + lane] = col.n;
        const long long tot = wave_sum((long long)col.n);
        if (lane == 0) a.unit_off[unit] = tot;
        // per-class levels live on the device: checked here (the host has checked the scalar ones), NaN included
        const bool bad_level = !(low >= 0.f && low <= thr);
        const int bits = (__any(bad) ? ACX_EVENTS_NONFINITE : 0) | (__any(bad_level) ? ACX_EVENTS_BAD_THRESHOLD : 0);
        if (bits && lane == 0) atomicOr(a.status, bits);                           // an OR: no order to depend on
    }
}

// unit totals -> exclusive offsets (in place), *count, the overflow bit.  One workgroup: thread i owns a contiguous chunk.
__global__ __launch_bounds__(1024) void events_scan_kernel(long long* unit_off, long long units, long long capacity,
                                                           long long* count, int* status) {
    __shared__ long long s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long chunk = (units + 1023) / 1024;
    const long long lo = tid * chunk < units ? tid * chunk : units, hi = lo + chunk < units ? lo + chunk : units;
    long long mine = 0;
    for (long long i = lo; i < hi; ++i) mine += unit_off[i];
    long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    long long run = before + incl - mine;
    for (long long i = lo; i < hi; ++i) {
        const long long c = unit_off[i];
        unit_off[i] = run;
        run += c;
    }
    if (tid == 0) {
        const int st = *status;
        if (st & (ACX_EVENTS_NONFINITE | ACX_EVENTS_BAD_THRESHOLD)) {
            *count = 0;
        } else {
            *count = total;
            if (total > capacity) *status = st | ACX_EVENTS_OVERFLOW;
        }
    }
}

// varlen: the clips' first rows, step counts and last boundaries, from the values passed by value
struct EvTabArgs {
    PackedLens steps;
    double end[kVarMaxClips];      // <= 0: steps * step
    double step;
};
__global__ __launch_bounds__(kVarMaxClips) void events_table_kernel(EvTabArgs t, long long* row0, int* steps, double* end) {
    __shared__ long long s_row0[kVarMaxClips + 1];
    const int i = threadIdx.x;
    if (i == 0) packed_prefix(t.steps.n, s_row0, [&t](int j) { return (long long)t.steps.len[j]; });
    __syncthreads();
    if (i >= t.steps.n) return;
    row0[i] = s_row0[i];
    steps[i] = t.steps.len[i];
    end[i] = t.end[i] > 0.0 ? t.end[i] : (double)t.steps.len[i] * t.step;
}

// workspace: unit_off [units] int64 | counts [units][64] int32 | row0 [256] int64 | end [256] double | steps [256] int32
static void ev_layout(long long units, size_t* counts, size_t* row0, size_t* end, size_t* steps, size_t* total) {
    *counts = align_up((size_t)units * 8);
    *row0 = *counts + align_up((size_t)units * 64 * 4);
    *end = *row0 + align_up(kVarMaxClips * 8);
    *steps = *end + align_up(kVarMaxClips * 8);
    *total = *steps + align_up(kVarMaxClips * 4);
}

template <bool EMIT>
static void ev_launch(const EvArgs& a, long long units, hipStream_t s) {
    const dim3 grid((unsigned)units), block(64);
    switch (a.median) {
        case 1: launch_kernel(&events_kernel<1, EMIT>, grid, block, 0, s, a); break;
        case 3: launch_kernel(&events_kernel<3, EMIT>, grid, block, 0, s, a); break;
        case 5: launch_kernel(&events_kernel<5, EMIT>, grid, block, 0, s, a); break;
        case 7: launch_kernel(&events_kernel<7, EMIT>, grid, block, 0, s, a); break;
        default: launch_kernel(&events_kernel<0, EMIT>, grid, block, (size_t)a.median * 64 * 4, s, a); break;
    }
    static_assert(kEvRegMedian == 7, "one case per register width");
}

int ev_scan(long long* unit_off, long long units, long long capacity, long long* count, int* status, hipStream_t s) {
    launch_kernel(&events_scan_kernel, dim3(1), dim3(1024), 0, s, unit_off, units, capacity, count, status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// everything after the argument checks: clear the status, count, scan, emit
static int ev_run(EvArgs a, long long units, long long* count, hipStream_t s) {
    ACX_HIP(hipMemsetAsync(a.status, 0, sizeof(int), s));
    ev_launch<false>(a, units, s);
    ACX_HIP(hipGetLastError());
    ACX_TRY(ev_scan(a.unit_off, units, a.capacity, count, a.status, s));
    ev_launch<true>(a, units, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// the uniform and the varlen call, with every class's levels in *p or one per class behind threshold / low
static int ev_decode(const char* who, const float* probs, int64_t ld, int64_t B, int steps, int N, const acx_event_params* p,
                     double step_seconds, double end_seconds, acx_event* events, int64_t capacity, int64_t* count, int* status,
                     void* ws, size_t ws_bytes, void* stream, const float* threshold, const float* low) {
    if (!probs || !p || !events || !count || !status || !ws) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(ev_check_params(who, p, step_seconds, capacity, threshold, low));
    if (steps < 1 || steps > kEvMaxSteps) ACX_FAIL(ACX_ERR_SHAPE, "%s: %d steps (expected 1 .. 2^30)", who, steps);
    long long units;
    ACX_TRY(ev_units(who, B, N, &units));
    if (ld < N) ACX_FAIL(ACX_ERR_SHAPE, "%s: row stride %lld is shorter than %d classes", who, (long long)ld, N);
    size_t coff, roff, eoff, soff, need;
    ev_layout(units, &coff, &roff, &eoff, &soff, &need);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, need));
    char* w = static_cast<char*>(ws);
    EvArgs a{};
    a.probs = probs; a.ld = ld; a.steps = steps; a.N = N; a.G = (N + 63) / 64;
    a.thr = p->threshold; a.low = p->low; a.thr_c = threshold; a.low_c = low; a.median = p->median;
    a.min_dur = p->min_duration; a.gap = p->merge_gap; a.step = step_seconds;
    a.end = end_seconds > 0.0 ? end_seconds : (double)steps * step_seconds;
    a.counts = reinterpret_cast<int*>(w + coff);
    a.unit_off = reinterpret_cast<long long*>(w);
    a.status = status; a.events = events; a.capacity = capacity;
    return ev_run(a, units, reinterpret_cast<long long*>(count), (hipStream_t)stream);
}

static int ev_decode_varlen(const char* who, const float* probs, int64_t ld, const int* steps, const double* end_seconds, int B,
                            int N, const acx_event_params* p, double step_seconds, acx_event* events, int64_t capacity,
                            int64_t* count, int* status, void* ws, size_t ws_bytes, void* stream, const float* threshold,
                            const float* low) {
    if (!probs || !steps || !p || !events || !count || !status || !ws) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(ev_check_params(who, p, step_seconds, capacity, threshold, low));
    if (B < 1 || B > kVarMaxClips) ACX_FAIL(ACX_ERR_SHAPE, "%s: %d clips (expected 1 .. %d)", who, B, kVarMaxClips);
    for (int i = 0; i < B; ++i)
        if (steps[i] < 1 || steps[i] > kEvMaxSteps)
            ACX_FAIL(ACX_ERR_SHAPE, "%s: clip %d has %d steps (expected 1 .. 2^30)", who, i, steps[i]);
    long long units;
    ACX_TRY(ev_units(who, B, N, &units));
    if (ld < N) ACX_FAIL(ACX_ERR_SHAPE, "%s: row stride %lld is shorter than %d classes", who, (long long)ld, N);
    size_t coff, roff, eoff, soff, need;
    ev_layout(units, &coff, &roff, &eoff, &soff, &need);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, need));
    const hipStream_t s = (hipStream_t)stream;
    char* w = static_cast<char*>(ws);
    EvTabArgs t{};
    t.steps = packed_lens(steps, B);
    t.step = step_seconds;
    for (int i = 0; i < B; ++i) t.end[i] = end_seconds ? end_seconds[i] : 0.0;
    long long* row0 = reinterpret_cast<long long*>(w + roff);
    double* end = reinterpret_cast<double*>(w + eoff);
    int* stp = reinterpret_cast<int*>(w + soff);
    launch_kernel(&events_table_kernel, dim3(1), dim3(kVarMaxClips), 0, s, t, row0, stp, end);
    ACX_HIP(hipGetLastError());
    EvArgs a{};
    a.probs = probs; a.ld = ld; a.steps = 0; a.N = N; a.G = (N + 63) / 64;
    a.thr = p->threshold; a.low = p->low; a.thr_c = threshold; a.low_c = low; a.median = p->median;
    a.min_dur = p->min_duration; a.gap = p->merge_gap; a.step = step_seconds;
    a.tab_row0 = row0; a.tab_steps = stp; a.tab_end = end;
    a.counts = reinterpret_cast<int*>(w + coff);
    a.unit_off = reinterpret_cast<long long*>(w);
    a.status = status; a.events = events; a.capacity = capacity;
    return ev_run(a, units, reinterpret_cast<long long*>(count), s);
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_events_workspace_bytes(int64_t B, int N, size_t* bytes) {
    if (!bytes) ACX_FAIL(ACX_ERR_ARG, "acx_events_workspace_bytes: bytes is null");
    long long units;
    ACX_TRY(ev_units("acx_events_workspace_bytes", B, N, &units));
    size_t c, r, e, st;
    ev_layout(units, &c, &r, &e, &st, bytes);
    return ACX_OK;
}

int acx_decode_events(const float* probs, int64_t ld, int64_t B, int steps, int N, const acx_event_params* p, double step_seconds,
                      double end_seconds, acx_event* events, int64_t capacity, int64_t* count, int* status, void* ws,
                      size_t ws_bytes, void* stream) {
    return ev_decode("acx_decode_events", probs, ld, B, steps, N, p, step_seconds, end_seconds, events, capacity, count, status, ws,
                     ws_bytes, stream, nullptr, nullptr);
}

int acx_decode_events_classwise(const float* probs, int64_t ld, int64_t B, int steps, int N, const acx_event_params* p,
                                double step_seconds, double end_seconds, acx_event* events, int64_t capacity, int64_t* count,
                                int* status, void* ws, size_t ws_bytes, void* stream, const float* threshold, const float* low) {
    return ev_decode("acx_decode_events_classwise", probs, ld, B, steps, N, p, step_seconds, end_seconds, events, capacity, count,
                     status, ws, ws_bytes, stream, threshold, low);
}

int acx_decode_events_varlen(const float* probs, int64_t ld, const int* steps, const double* end_seconds, int B, int N,
                             const acx_event_params* p, double step_seconds, acx_event* events, int64_t capacity, int64_t* count,
                             int* status, void* ws, size_t ws_bytes, void* stream) {
    return ev_decode_varlen("acx_decode_events_varlen", probs, ld, steps, end_seconds, B, N, p, step_seconds, events, capacity,
                            count, status, ws, ws_bytes, stream, nullptr, nullptr);
}

int acx_decode_events_varlen_classwise(const float* probs, int64_t ld, const int* steps, const double* end_seconds, int B, int N,
                                       const acx_event_params* p, double step_seconds, acx_event* events, int64_t capacity,
                                       int64_t* count, int* status, void* ws, size_t ws_bytes, void* stream, const float* threshold,
                                       const float* low) {
    return ev_decode_varlen("acx_decode_events_varlen_classwise", probs, ld, steps, end_seconds, B, N, p, step_seconds, events,
                            capacity, count, status, ws, ws_bytes, stream, threshold, low);
}

}  // extern "C"
