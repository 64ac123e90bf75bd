// What the batch event decoder (events.hip) and the online one (events_online.hip) share (include/acx.h "sound event decoding",
// "online event decoding"): the arguments of a decoding, the sorted median window of one lane and the per-column state machine
// -- defined once, here -- plus the host-side checks of both C entry points.  The online decoder adds to the state machine
// only what makes it resumable: load / store of the state, the early-emission step and the open-event query.
#pragma once
#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kEvDepth = 8;          // rows of each stream in flight per wave
constexpr int kEvRegMedian = 7;      // widest median window kept in registers
constexpr long long kEvMaxUnits = 2147483647LL;   // one workgroup per unit: the grid's x limit
constexpr int kEvMaxSteps = 1 << 30;              // row numbers plus the look-ahead stay inside an int

struct EvArgs {
    const float* probs;
    long long ld;
    int steps;                 // uniform batches; varlen: tab_steps[clip]
    int N, G;                  // classes, units per clip = ceil(N / 64)
    float thr, low;            // every class's, unless thr_c / low_c give each class its own
    const float* thr_c;        // [N] per-class threshold (null: thr)
    const float* low_c;        // [N] per-class low (null: thr_c given ? the class's threshold : low)
    int median;
    double min_dur, gap, step, end;      // end: uniform batches (already resolved); varlen: tab_end[clip]
    const long long* tab_row0;           // varlen: first row of each clip (null: clip * steps)
    const int* tab_steps;
    const double* tab_end;
    int* counts;               // [units][64] events of each column
    long long* unit_off;       // [units] events of each unit, then (after the scan) their exclusive prefix
    int* status;
    acx_event* events;
    long long capacity;
};

// The columns' state between two calls of an online decoder: struct-of-arrays, one element per (slot, padded class).
struct EvState {
    int* flags;                // bit 0 in_run, bit 1 rvalid, bit 2 have
    int *rb, *eb, *ee;
    float *rmax, *emax, *epeak;
    double *rsum, *esum, *esnap;
};

// The sorted window of one lane.  WR > 0: WR registers; WR == 0: `w` LDS slots, slot k of this lane at l[k * 64].
template <int WR>
struct EvWindow {
    float r[WR > 0 ? WR : 1];
    float* l;
    int w;
    __device__ __forceinline__ void fill(float v) {
        if constexpr (WR > 0) {
#pragma unroll
            for (int k = 0; k < WR; ++k) r[k] = v;
        } else {
            for (int k = 0; k < w; ++k) l[k * 64] = v;
        }
    }
    __device__ __forceinline__ float median() const {
        if constexpr (WR > 0) return r[WR / 2];
        else return l[(w / 2) * 64];
    }
    // One slot of the update: a = the window as it was, rem[k] = (a[k] < o ? a[k] : a[k + 1]) = a without one `o`,
    // new[k] = rem[k - 1] if rem[k - 1] > n, else rem[k] if rem[k] <= n, else n.
    static __device__ __forceinline__ float slot(float ak, float ak1, float o, float n, float& rprev, bool first) {
        const float rk = ak < o ? ak : ak1;
        const float b = (!first && !(rprev <= n)) ? rprev : (rk <= n ? rk : n);
        rprev = rk;
        return b;
    }
    // remove one `o` (which the window holds), insert `n`; the window stays sorted
    __device__ __forceinline__ void update(float o, float n) {
        float rprev = 0.f;
        if constexpr (WR > 0) {
#pragma unroll
            for (int k = 0; k < WR; ++k) {
                const float ak1 = k + 1 < WR ? r[k + 1] : INFINITY;
                r[k] = slot(r[k], ak1, o, n, rprev, k == 0);
            }
        } else {
            float ak = l[0];
            for (int k = 0; k < w; ++k) {
                const float ak1 = k + 1 < w ? l[(k + 1) * 64] : INFINITY;
                l[k * 64] = slot(ak, ak1, o, n, rprev, k == 0);
                ak = ak1;
            }
        }
    }
};

__device__ __forceinline__ bool ev_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// The per-column state machine of decode_events, one step of time per call; [eb, ee) is the pending (possibly merged) event,
// emax / esum run from eb over EVERY row since (gap rows included) so that a merge can adopt them, epeak / esnap are their
// values at ee.
template <bool EMIT>
struct EvColumn {
    const EvArgs& a;
    int steps;
    double end;
    bool live;
    float thr, low;          // this lane's class
    int clip, cls;
    long long base;          // EMIT: table index of this column's first event
    int n = 0;               // events so far
    bool in_run = false, rvalid = false, have = false;
    int rb = 0, eb = 0, ee = 0;
    float rmax = 0.f, emax = 0.f, epeak = 0.f;
    double rsum = 0.0, esum = 0.0, esnap = 0.0;

    __device__ __forceinline__ EvColumn(const EvArgs& a_, int steps_, double end_, bool live_, float thr_, float low_, int clip_,
                                        int cls_, long long base_)
        : a(a_), steps(steps_), end(end_), live(live_), thr(thr_), low(low_), clip(clip_), cls(cls_), base(base_) {}
    __device__ __forceinline__ double edge(int k) const { return event_edge(k, steps, a.step, end); }
    __device__ __forceinline__ void finish_event() {
        if (!(edge(ee) - edge(eb) < a.min_dur)) {
            if constexpr (EMIT) {
                const long long i = base + n;
                if (i < a.capacity) {
                    acx_event e;
                    e.clip = clip; e.cls = cls; e.begin = eb; e.end = ee;
                    e.peak = epeak; e.reserved = 0.f;
                    e.mean = esnap / (double)(ee - eb);
                    a.events[i] = e;
                }
            }
            ++n;
        }
    }
    // the run [rb, t) has ended
    __device__ __forceinline__ void end_run(int t) {
        in_run = false;
        if (!rvalid) return;
        if (have && edge(rb) - edge(ee) < a.gap) {
            ee = t; epeak = emax; esnap = esum;
        } else {
            if (have) finish_event();
            have = true;
            eb = rb; ee = t;
            epeak = emax = rmax;
            esnap = esum = rsum;
        }
    }
    __device__ __forceinline__ void step(int t, float p) {
        const bool on = live && p >= low;
        if (!on && in_run) end_run(t);
        if (have) { emax = fmaxf(emax, p); esum += (double)p; }
        if (on) {
            if (!in_run) { in_run = true; rb = t; rvalid = false; rmax = p; rsum = 0.0; }
            rmax = fmaxf(rmax, p);
            rsum += (double)p;
            rvalid = rvalid || p >= thr;
        }
    }
    __device__ __forceinline__ void finish() {
        if (in_run) end_run(steps);
        if (have) finish_event();
    }
    // ---- the resumable form (events_online.hip) ----
    // After step(t): the pending event is final once no run still to come can merge with it -- k * step never decreases in
    // k -- and leaves now.  A later valid run then starts a fresh event through end_run's else branch.
    __device__ __forceinline__ void early(int t) {
        if (!have) return;
        const double from = in_run ? edge(rb) : edge(t + 1);
        if (!(from - edge(ee) < a.gap)) {
            finish_event();
            have = false;
        }
    }
    // the step at which the event this column is inside of began: a run that has reached thr is open; -1 otherwise
    __device__ __forceinline__ int open_begin() const {
        if (!(in_run && rvalid)) return -1;
        return have && edge(rb) - edge(ee) < a.gap ? eb : rb;
    }
    __device__ __forceinline__ void load(const EvState& s, long long i) {
        const int f = s.flags[i];
        in_run = f & 1; rvalid = f & 2; have = f & 4;
        rb = s.rb[i]; eb = s.eb[i]; ee = s.ee[i];
        rmax = s.rmax[i]; emax = s.emax[i]; epeak = s.epeak[i];
        rsum = s.rsum[i]; esum = s.esum[i]; esnap = s.esnap[i];
    }
    __device__ __forceinline__ void store(const EvState& s, long long i) const {
        s.flags[i] = (in_run ? 1 : 0) | (rvalid ? 2 : 0) | (have ? 4 : 0);
        s.rb[i] = rb; s.eb[i] = eb; s.ee[i] = ee;
        s.rmax[i] = rmax; s.emax[i] = emax; s.epeak[i] = epeak;
        s.rsum[i] = rsum; s.esum[i] = esum; s.esnap[i] = esnap;
    }
    // a closed recording leaves the column as a new handle has it: all zero
    __device__ __forceinline__ void reset() {
        n = 0;
        in_run = rvalid = have = false;
        rb = eb = ee = 0;
        rmax = emax = epeak = 0.f;
        rsum = esum = esnap = 0.0;
    }
};

// events.hip: unit totals -> exclusive offsets (in place), *count, the overflow bit; one launch on s
int ev_scan(long long* unit_off, long long units, long long capacity, long long* count, int* status, hipStream_t s);

inline int ev_units(const char* who, int64_t B, int N, long long* units) {
    if (B < 1) ACX_FAIL(ACX_ERR_SHAPE, "%s: B = %lld (expected >= 1)", who, (long long)B);
    if (N < 1 || N > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_SHAPE, "%s: %d classes (expected 1 .. %d)", who, N, ACX_MAX_CLASSES);
    const long long G = (N + 63) / 64;
    if (B > kEvMaxUnits / G)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: %lld clips of %d classes need more than %lld workgroups", who, (long long)B, N,
                 kEvMaxUnits);
    *units = B * G;
    return ACX_OK;
}

inline int ev_check_params(const char* who, const acx_event_params* p, double step_seconds, int64_t capacity,
                           const float* threshold = nullptr, const float* low = nullptr) {
    if (p->median < 1 || p->median > ACX_MAX_EVENT_MEDIAN || p->median % 2 == 0)
        ACX_FAIL(ACX_ERR_ARG, "%s: median %d (expected an odd width in 1 .. %d)", who, p->median, ACX_MAX_EVENT_MEDIAN);
    // a per-class pointer replaces its scalar; what is left of the scalars is checked here, the rest on the device
    if (!threshold && !low && !(p->low >= 0.f && p->low <= p->threshold))
        ACX_FAIL(ACX_ERR_ARG, "%s: low %g must be in [0, threshold = %g]", who, (double)p->low, (double)p->threshold);
    if (!threshold && low && !(p->threshold >= 0.f))
        ACX_FAIL(ACX_ERR_ARG, "%s: threshold %g must not be negative", who, (double)p->threshold);
    if (!(p->min_duration >= 0.0) || !(p->merge_gap >= 0.0))
        ACX_FAIL(ACX_ERR_ARG, "%s: min_duration %g and merge_gap %g must not be negative", who, p->min_duration, p->merge_gap);
    if (!(step_seconds > 0.0)) ACX_FAIL(ACX_ERR_ARG, "%s: step_seconds %g (expected > 0)", who, step_seconds);
    if (capacity < 0) ACX_FAIL(ACX_ERR_ARG, "%s: capacity %lld (expected >= 0)", who, (long long)capacity);
    return ACX_OK;
}

}  // namespace acx
