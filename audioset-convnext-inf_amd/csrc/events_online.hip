// Online event decoding (include/acx.h "online event decoding"): acx_decode_events for recordings whose rows arrive chunk by
// chunk.  The definition is pytorch/segments.py::OnlineEventDecoderHost; the column state machine is the batch decoder's
// (events_common.h), started from the state the previous call stored instead of from nothing.
//
// The shape of events_kernel: one WAVE per (entry of the call, 64 classes), a lane per class, every row read one coalesced
// line; a count pass, the batch decoder's scan, an emit pass.  Both passes start from the saved state and only the emit pass
// stores it -- after reading the status the scan wrote, so a call whose table overflowed or whose rows held a NaN leaves every
// byte of the state as it was.  The table of one call is ordered (entry, cls, begin) and has the same bits on every call.
//
// State, struct-of-arrays over (slot, class padded to 64): the EvColumn fields, per (slot, 64 classes) the raw rows pushed so
// far, and the last `median` raw rows as a ring (raw row i at ring row i % median).  Filtered row t needs raw rows t - h ..
// t + h (h = median / 2), so a call that has s rows behind it and r new ones consumes filtered rows max(0, s - h) ..
// max(0, s + r - h) - 1 (close: .. s - 1, the last row repeated) and reads at most median - 1 rows of the ring.  The sorted
// window is rebuilt from those rows at entry: the median is a selection, so the values are the ones a kept window would give.
//
// Built with -fno-slp-vectorize like events.hip and with -ffp-contract=off: (double)k * step and the differences against
// merge_gap / min_duration are the host definition's two roundings, never one fused one.
#include "events_common.h"

#include <new>
#include <vector>

namespace acx {

constexpr int kEvMaxSlots = 1 << 20;
constexpr size_t kEvMaxState = (size_t)1 << 40;

struct EvOnArgs {
    const float* probs;        // the call's rows: rows[0] of slot[0], then rows[1] of slot[1], ...
    long long ld;
    int N, G, Np;              // classes, units per slot = ceil(N / 64), padded classes = 64 G
    int median;
    int far;                   // a step count no row number reaches: edge(k) = k * step while the recording is open
    double min_dur, gap, step;
    const float* thr_c;        // [Np]
    const float* low_c;        // [Np]
    EvState st;                // [slots][Np]
    float* hist;               // [slots][median][Np]
    int* steps;                // [slots][G] raw rows of the open recording, one copy per unit
    const double* end;         // close: [n] last boundaries, resolved by events_online_end_kernel; push: null
    int* counts;               // [n G][64]
    long long* unit_off;       // [n G]
    int* status;
    acx_event* events;
    long long capacity;
    int slot[kVarMaxClips];
    int rows[kVarMaxClips];    // close: 0
};

template <int WR, bool EMIT>
__global__ __launch_bounds__(64) void events_online_kernel(EvOnArgs o) {
    extern __shared__ float s_win[];
    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int e = unit / o.G, g = unit - e * o.G;
    const int cls = g * 64 + lane;
    const bool live = cls < o.N;

    long long base = 0;
    if constexpr (EMIT) {
        if (*o.status) return;                          // a void call: nothing is written, no state is stored
        const int mine = o.counts[unit * 64 + lane];
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        base = o.unit_off[unit] + (incl - mine);        // (no overflow here, so base + n stays below capacity)
    }

    const int slot = o.slot[e], r = o.rows[e];
    const bool closing = o.end != nullptr;
    long long row0 = 0;
    for (int j = 0; j < e; ++j) row0 += o.rows[j];
    int* const steps_at = o.steps + (long long)slot * o.G + g;
    const int s = __builtin_amdgcn_readfirstlane(*steps_at);
    if ((unsigned)s + (unsigned)r > (unsigned)kEvMaxSteps) {
        // past 2^30 rows: the host counters refuse this unless a void call was never undone; the call is void
        if constexpr (!EMIT) {
            o.counts[unit * 64 + lane] = 0;
            if (lane == 0) {
                o.unit_off[unit] = 0;
                atomicOr(o.status, ACX_EVENTS_NONFINITE);
            }
        }
        return;
    }
    const int h = o.median / 2;
    const int total = s + r, last = total - 1;
    const int c0 = s - h > 0 ? s - h : 0;                                   // filtered rows consumed before this call
    const int c1 = closing ? s : (total - h > 0 ? total - h : 0);           // ... and after it
    const int col_of = live ? cls : o.N - 1;                                // idle lanes re-read the last class: in bounds
    const float* x = o.probs + row0 * o.ld + col_of;
    const long long idx = (long long)slot * o.Np + cls;
    float* hs = o.hist + (long long)slot * o.median * o.Np + cls;
    // raw row i of the recording, the ends repeated: from the ring below s, from the call's rows from s on
    auto row = [&](int i) {
        i = i < 0 ? 0 : i > last ? last : i;
        if (i < s) return hs[(long long)(i % o.median) * o.Np];
        return x[(long long)(i - s) * o.ld];
    };

    EvArgs a{};
    a.step = o.step; a.min_dur = o.min_dur; a.gap = o.gap;
    a.events = o.events; a.capacity = o.capacity;
    EvColumn<EMIT> col(a, o.far, 0.0, live, o.thr_c[cls], o.low_c[cls], slot, cls, base);
    col.load(o.st, idx);

    bool bad = false;
    if (c1 > c0) {
        EvWindow<WR> win;
        win.l = s_win + lane;
        win.w = o.median;
        // the window of filtered row c0: raw rows c0 - h .. c0 + h
        const float x0 = row(c0 - h);
        bad = ev_nonfinite(x0);
        if constexpr (WR != 1) {
            win.fill(x0);
            for (int j = 1; j <= 2 * h; ++j) {
                const float v = row(c0 - h + j);
                bad = bad || ev_nonfinite(v);
                win.update(x0, v);
            }
        } else {
            win.r[0] = x0;
        }
        // step t reads the window's median, then trades row t - h for row t + h + 1; both streams run kEvDepth rows ahead
        float cin[kEvDepth], cout[kEvDepth], nin[kEvDepth], nout[kEvDepth];
#pragma unroll
        for (int j = 0; j < kEvDepth; ++j) {
            cin[j] = row(c0 + j + h + 1);
            cout[j] = WR == 1 ? 0.f : row(c0 + j - h);
        }
        for (int t0 = c0; t0 < c1; t0 += kEvDepth) {
#pragma unroll
            for (int j = 0; j < kEvDepth; ++j) {      // (rows past the end clamp to the last one: in bounds, unused)
                nin[j] = row(t0 + kEvDepth + j + h + 1);
                nout[j] = WR == 1 ? 0.f : row(t0 + kEvDepth + j - h);
            }
#pragma unroll
            for (int j = 0; j < kEvDepth; ++j) {
                const int t = t0 + j;
                if (t < c1) {
                    col.step(t, win.median());
                    col.early(t);
                    bad = bad || ev_nonfinite(cin[j]);
                    if constexpr (WR == 1) win.r[0] = cin[j];
                    else win.update(cout[j], cin[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < kEvDepth; ++j) { cin[j] = nin[j]; cout[j] = nout[j]; }
        }
    } else if constexpr (!EMIT) {
        for (int i = 0; i < r; ++i) bad = bad || ev_nonfinite(x[(long long)i * o.ld]);     // rows no filtered row reads yet
    }
    if (closing && s > 0) {
        col.steps = s;
        col.end = o.end[e];
        col.finish();
    }

    if constexpr (!EMIT) {
        o.counts[unit * 64 + lane] = col.n;
        const long long tot = wave_sum((long long)col.n);
        if (lane == 0) o.unit_off[unit] = tot;
        if (__any(bad) && lane == 0) atomicOr(o.status, ACX_EVENTS_NONFINITE);            // an OR: no order to depend on
    } else {
        if (closing) col.reset();
        col.store(o.st, idx);
        // the ring keeps the last `median` raw rows (every read of it above has been issued before these stores)
        const int from = total - o.median > s ? total - o.median : s;
        for (int i = from; i < total; ++i) hs[(long long)(i % o.median) * o.Np] = x[(long long)(i - s) * o.ld];
        if (lane == 0) *steps_at = closing ? 0 : total;
    }
}

// close: the last boundaries, passed by value, resolved against the rows each slot holds
struct EvEndArgs {
    double end[kVarMaxClips];      // <= 0: steps * step
    int slot[kVarMaxClips];
    int n, G;
    double step;
};
__global__ __launch_bounds__(kVarMaxClips) void events_online_end_kernel(EvEndArgs t, const int* steps, double* end) {
    const int i = threadIdx.x;
    if (i >= t.n) return;
    end[i] = t.end[i] > 0.0 ? t.end[i] : (double)steps[(long long)t.slot[i] * t.G] * t.step;
}

struct EvOpenArgs {
    int N, G, Np, far;
    double gap, step;
    EvState st;
    int* begin;                    // (n, N)
    int slot[kVarMaxClips];
};
__global__ __launch_bounds__(64) void events_online_open_kernel(EvOpenArgs o) {
    const int lane = threadIdx.x;
    const int e = blockIdx.x / o.G, g = blockIdx.x - e * o.G;
    const int cls = g * 64 + lane;
    if (cls >= o.N) return;
    EvArgs a{};
    a.step = o.step; a.gap = o.gap;
    EvColumn<false> col(a, o.far, 0.0, true, 0.f, 0.f, 0, cls, 0);
    col.load(o.st, (long long)o.slot[e] * o.Np + cls);
    o.begin[(long long)e * o.N + cls] = col.open_begin();
}

template <bool EMIT>
static void ev_online_launch(const EvOnArgs& o, int units, hipStream_t s) {
    const dim3 grid((unsigned)units), block(64);
    switch (o.median) {
        case 1: launch_kernel(&events_online_kernel<1, EMIT>, grid, block, 0, s, o); break;
        case 3: launch_kernel(&events_online_kernel<3, EMIT>, grid, block, 0, s, o); break;
        case 5: launch_kernel(&events_online_kernel<5, EMIT>, grid, block, 0, s, o); break;
        case 7: launch_kernel(&events_online_kernel<7, EMIT>, grid, block, 0, s, o); break;
        default: launch_kernel(&events_online_kernel<0, EMIT>, grid, block, (size_t)o.median * 64 * 4, s, o); break;
    }
    static_assert(kEvRegMedian == 7, "one case per register width");
}

// device state of a handle: the columns | ring | steps | thr | low | counts | unit_off | end
struct EvOnLayout {
    size_t flags, rb, eb, ee, rmax, emax, epeak, rsum, esum, esnap, hist, steps, thr, low, counts, unit_off, end, total;
};
static int ev_online_layout(const char* who, int slots, int N, int median, EvOnLayout* l) {
    if (slots < 1 || slots > kEvMaxSlots) ACX_FAIL(ACX_ERR_SHAPE, "%s: %d slots (expected 1 .. 2^20)", who, slots);
    if (N < 1 || N > ACX_MAX_CLASSES) ACX_FAIL(ACX_ERR_SHAPE, "%s: %d classes (expected 1 .. %d)", who, N, ACX_MAX_CLASSES);
    if (median < 1 || median > ACX_MAX_EVENT_MEDIAN || median % 2 == 0)
        ACX_FAIL(ACX_ERR_ARG, "%s: median %d (expected an odd width in 1 .. %d)", who, median, ACX_MAX_EVENT_MEDIAN);
    const size_t G = (size_t)(N + 63) / 64, Np = G * 64, cols = (size_t)slots * Np;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
    l->flags = take(cols * 4); l->rb = take(cols * 4); l->eb = take(cols * 4); l->ee = take(cols * 4);
    l->rmax = take(cols * 4); l->emax = take(cols * 4); l->epeak = take(cols * 4);
    l->rsum = take(cols * 8); l->esum = take(cols * 8); l->esnap = take(cols * 8);
    l->hist = take(cols * (size_t)median * 4);
    l->steps = take((size_t)slots * G * 4);
    l->thr = take(Np * 4); l->low = take(Np * 4);
    l->counts = take((size_t)kVarMaxClips * Np * 4);
    l->unit_off = take((size_t)kVarMaxClips * G * 8);
    l->end = take((size_t)kVarMaxClips * 8);
    l->total = off;
    if (off > kEvMaxState)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: %d slots of %d classes at median %d need %zu bytes of state (at most 2^40)", who, slots,
                 N, median, off);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

struct acx_event_stream {
    int slots = 0, N = 0, G = 0, Np = 0, device = 0;
    acx_event_params p{};
    double step = 0.0;
    char* mem = nullptr;
    EvOnLayout l{};
    std::vector<int64_t> rows;            // host: raw rows of each slot's open recording
    std::vector<int> mark;                // host: scratch of the distinct-slots check
    std::vector<int64_t> prev;            // host: each slot's counter before its last push / close (acx_event_stream_undo)
};

namespace acx {

static int ev_online_slots(const acx_event_stream* h, const char* who, const int* slot, int n, std::vector<int>* mark) {
    if (n < 1 || n > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "%s: %d slots in the call (expected 1 .. %d)", who, n, kVarMaxClips);
    for (int k = 0; k < n; ++k)
        if (slot[k] < 0 || slot[k] >= h->slots)
            ACX_FAIL(ACX_ERR_ARG, "%s: slot %d out of range (the handle has %d)", who, slot[k], h->slots);
    if (mark) {
        int twice = -1;
        for (int k = 0; k < n; ++k) {
            if ((*mark)[slot[k]]) twice = slot[k];
            (*mark)[slot[k]] = 1;
        }
        for (int k = 0; k < n; ++k) (*mark)[slot[k]] = 0;
        if (twice >= 0) ACX_FAIL(ACX_ERR_ARG, "%s: slot %d is listed twice", who, twice);
    }
    return ACX_OK;
}

static EvState ev_online_state(const acx_event_stream* h) {
    char* m = h->mem;
    const EvOnLayout& l = h->l;
    EvState st;
    st.flags = reinterpret_cast<int*>(m + l.flags);
    st.rb = reinterpret_cast<int*>(m + l.rb); st.eb = reinterpret_cast<int*>(m + l.eb); st.ee = reinterpret_cast<int*>(m + l.ee);
    st.rmax = reinterpret_cast<float*>(m + l.rmax); st.emax = reinterpret_cast<float*>(m + l.emax);
    st.epeak = reinterpret_cast<float*>(m + l.epeak);
    st.rsum = reinterpret_cast<double*>(m + l.rsum); st.esum = reinterpret_cast<double*>(m + l.esum);
    st.esnap = reinterpret_cast<double*>(m + l.esnap);
    return st;
}

// the launches of a push (end == null) or a close: clear the status, count, scan, emit
static int ev_online_run(acx_event_stream* h, const float* probs, int64_t ld, const int* slot, const int* rows, int n, bool closing,
                         acx_event* events, int64_t capacity, int64_t* count, int* status, hipStream_t s) {
    char* m = h->mem;
    EvOnArgs o{};
    o.probs = probs; o.ld = ld; o.N = h->N; o.G = h->G; o.Np = h->Np; o.median = h->p.median;
    o.far = 0x7fffffff;
    o.min_dur = h->p.min_duration; o.gap = h->p.merge_gap; o.step = h->step;
    o.thr_c = reinterpret_cast<const float*>(m + h->l.thr); o.low_c = reinterpret_cast<const float*>(m + h->l.low);
    o.st = ev_online_state(h);
    o.hist = reinterpret_cast<float*>(m + h->l.hist);
    o.steps = reinterpret_cast<int*>(m + h->l.steps);
    o.end = closing ? reinterpret_cast<const double*>(m + h->l.end) : nullptr;
    o.counts = reinterpret_cast<int*>(m + h->l.counts);
    o.unit_off = reinterpret_cast<long long*>(m + h->l.unit_off);
    o.status = status; o.events = events; o.capacity = capacity;
    for (int k = 0; k < n; ++k) { o.slot[k] = slot[k]; o.rows[k] = rows ? rows[k] : 0; }
    const int units = n * h->G;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    ev_online_launch<false>(o, units, s);
    ACX_HIP(hipGetLastError());
    ACX_TRY(ev_scan(o.unit_off, units, capacity, reinterpret_cast<long long*>(count), status, s));
    ev_online_launch<true>(o, units, s);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx

extern "C" {

int acx_event_stream_bytes(int slots, int N, int median, size_t* bytes) {
    if (!bytes) ACX_FAIL(ACX_ERR_ARG, "acx_event_stream_bytes: bytes is null");
    EvOnLayout l;
    ACX_TRY(ev_online_layout("acx_event_stream_bytes", slots, N, median, &l));
    *bytes = l.total;
    return ACX_OK;
}

int acx_event_stream_create(int slots, int N, const acx_event_params* p, double step_seconds, const float* threshold,
                            const float* low, acx_event_stream** out) {
    const char* who = "acx_event_stream_create";
    if (out) *out = nullptr;
    if (!p || !out) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(ev_check_params(who, p, step_seconds, 0, threshold, low));
    EvOnLayout l;
    ACX_TRY(ev_online_layout(who, slots, N, p->median, &l));
    acx_event_stream* h = new (std::nothrow) acx_event_stream();
    if (!h) ACX_FAIL(ACX_ERR_HIP, "%s: out of host memory", who);
    h->slots = slots; h->N = N; h->G = (N + 63) / 64; h->Np = h->G * 64;
    h->p = *p; h->step = step_seconds; h->l = l;
    h->rows.assign(slots, 0);
    h->prev.assign(slots, 0);
    h->mark.assign(slots, 0);
    auto fail = [&](int rc) { acx_event_stream_destroy(h); return rc; };
    if (hipGetDevice(&h->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&h->mem), l.total) != hipSuccess) {
        h->mem = nullptr;
        set_error("%s: cannot allocate %zu bytes of device state", who, l.total);
        return fail(ACX_ERR_HIP);
    }
    // the levels of every class, padded classes never on; a clean state is all zero
    std::vector<float> thr(h->Np, INFINITY), lo(h->Np, INFINITY);
    hipError_t e = hipMemset(h->mem, 0, l.total);
    if (e == hipSuccess && threshold) e = hipMemcpy(thr.data(), threshold, (size_t)N * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && low) e = hipMemcpy(lo.data(), low, (size_t)N * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        return fail(ACX_ERR_HIP);
    }
    for (int c = 0; c < N; ++c) {
        if (!threshold) thr[c] = p->threshold;
        if (!low) lo[c] = threshold ? thr[c] : p->low;
        if (!(lo[c] >= 0.f && lo[c] <= thr[c])) {
            set_error("%s: low %g must be in [0, threshold = %g] in class %d", who, (double)lo[c], (double)thr[c], c);
            return fail(ACX_ERR_ARG);
        }
    }
    e = hipMemcpy(h->mem + l.thr, thr.data(), (size_t)h->Np * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->mem + l.low, lo.data(), (size_t)h->Np * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        return fail(ACX_ERR_HIP);
    }
    *out = h;
    return ACX_OK;
}

void acx_event_stream_destroy(acx_event_stream* h) {
    if (!h) return;
    if (h->mem) (void)hipFree(h->mem);
    delete h;
}

int acx_event_stream_push(acx_event_stream* h, const float* probs, int64_t ld, const int* slot, const int* rows, int n,
                          acx_event* events, int64_t capacity, int64_t* count, int* status, void* stream) {
    const char* who = "acx_event_stream_push";
    if (!h || !slot || !rows || !events || !count || !status) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (capacity < 0) ACX_FAIL(ACX_ERR_ARG, "%s: capacity %lld (expected >= 0)", who, (long long)capacity);
    ACX_TRY(ev_online_slots(h, who, slot, n, &h->mark));
    long long total = 0;
    for (int k = 0; k < n; ++k) {
        if (rows[k] < 0) ACX_FAIL(ACX_ERR_ARG, "%s: %d rows for slot %d (expected >= 0)", who, rows[k], slot[k]);
        if (h->rows[slot[k]] + rows[k] > kEvMaxSteps)
            ACX_FAIL(ACX_ERR_SHAPE, "%s: slot %d holds %lld rows, %d more pass 2^30", who, slot[k], (long long)h->rows[slot[k]],
                     rows[k]);
        total += rows[k];
    }
    if (total > 0 && !probs) ACX_FAIL(ACX_ERR_ARG, "%s: probs is null", who);
    if (total > 0 && ld < h->N)
        ACX_FAIL(ACX_ERR_SHAPE, "%s: row stride %lld is shorter than %d classes", who, (long long)ld, h->N);
    ACX_TRY(ev_online_run(h, probs, ld, slot, rows, n, false, events, capacity, count, status, (hipStream_t)stream));
    for (int k = 0; k < n; ++k) {
        h->prev[slot[k]] = h->rows[slot[k]];
        h->rows[slot[k]] += rows[k];
    }
    return ACX_OK;
}

int acx_event_stream_close(acx_event_stream* h, const int* slot, const double* end_seconds, int n, acx_event* events,
                           int64_t capacity, int64_t* count, int* status, void* stream) {
    const char* who = "acx_event_stream_close";
    if (!h || !slot || !events || !count || !status) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (capacity < 0) ACX_FAIL(ACX_ERR_ARG, "%s: capacity %lld (expected >= 0)", who, (long long)capacity);
    ACX_TRY(ev_online_slots(h, who, slot, n, &h->mark));
    const hipStream_t s = (hipStream_t)stream;
    EvEndArgs t{};
    t.n = n; t.G = h->G; t.step = h->step;
    for (int k = 0; k < n; ++k) {
        t.slot[k] = slot[k];
        t.end[k] = end_seconds ? end_seconds[k] : 0.0;
    }
    launch_kernel(&events_online_end_kernel, dim3(1), dim3(kVarMaxClips), 0, s, t,
                  reinterpret_cast<const int*>(h->mem + h->l.steps), reinterpret_cast<double*>(h->mem + h->l.end));
    ACX_HIP(hipGetLastError());
    ACX_TRY(ev_online_run(h, nullptr, h->N, slot, nullptr, n, true, events, capacity, count, status, s));
    for (int k = 0; k < n; ++k) {
        h->prev[slot[k]] = h->rows[slot[k]];
        h->rows[slot[k]] = 0;
    }
    return ACX_OK;
}

int acx_event_stream_open(const acx_event_stream* h, const int* slot, int n, int32_t* begin, void* stream) {
    const char* who = "acx_event_stream_open";
    if (!h || !slot || !begin) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(ev_online_slots(h, who, slot, n, nullptr));
    EvOpenArgs o{};
    o.N = h->N; o.G = h->G; o.Np = h->Np; o.far = 0x7fffffff;
    o.gap = h->p.merge_gap; o.step = h->step;
    o.st = ev_online_state(h);
    o.begin = begin;
    for (int k = 0; k < n; ++k) o.slot[k] = slot[k];
    launch_kernel(&events_online_open_kernel, dim3((unsigned)(n * h->G)), dim3(64), 0, (hipStream_t)stream, o);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_event_stream_steps(const acx_event_stream* h, int slot, int64_t* steps) {
    if (!h || !steps) ACX_FAIL(ACX_ERR_ARG, "acx_event_stream_steps: null argument");
    if (slot < 0 || slot >= h->slots)
        ACX_FAIL(ACX_ERR_ARG, "acx_event_stream_steps: slot %d out of range (the handle has %d)", slot, h->slots);
    *steps = h->rows[slot];
    return ACX_OK;
}

int acx_event_stream_undo(acx_event_stream* h, const int* slot, int n) {
    if (!h || !slot) ACX_FAIL(ACX_ERR_ARG, "acx_event_stream_undo: null argument");
    ACX_TRY(ev_online_slots(h, "acx_event_stream_undo", slot, n, nullptr));
    for (int k = 0; k < n; ++k) h->rows[slot[k]] = h->prev[slot[k]];
    return ACX_OK;
}

}  // extern "C"
