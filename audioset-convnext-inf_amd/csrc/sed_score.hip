// Scoring detected events against annotations on the device (include/acx.h "sound event scoring"): the event table of
// acx_decode_events and a table of reference events -> integer counts, the batched form of pytorch/sed_metrics.py's
// event_based_metrics_host and segment_based_metrics_host.
//
// Both tables are sorted by (clip, cls), so every (clip, class) column finds its rows in each by binary search on that key: no
// offset pass, no workspace.  The estimated table's valid length is min(*count, capacity) read on the device -- the scorers queue
// behind the decoder without a host round trip.  Everything produced is an integer; the counts of different columns meet only in
// 64-bit integer atomic adds, which are order-free, so every call gives the same bits.
//   sed_event_match_kernel  one WAVE per (clip, 64 classes), a lane per class, as in events.hip: the greedy collar matching.  A
//                           lane reads and writes only the rows of its own column.
//   sed_segment_kernel      one WORKGROUP per (clip, tile of kScTile segments), a thread per class: the unions of the reference
//                           and of the estimated intervals, intersected by two pointers; the runs of misses and false alarms are
//                           +1 / -1 interval adds into two per-segment LDS difference arrays, which the workgroup then scans for
//                           the substitutions, deletions and insertions of every segment.
//   sed_intersection_kernel one WAVE per (clip, 64 classes), a lane per class: the intersection criteria of PSDS (detection
//                           tolerance, ground-truth intersection, cross-trigger tolerance), all three by one walk, sc_cover_row.
//   cross_trigger_rate_kernel  a thread per detected class: its row of a cross-trigger matrix as one weighted mean, summed in
//                           ascending class order (the fixed order psds_host states).
//
// float64 throughout, as the host definitions: onsets and offsets come from event_edge (device_common.h), the decoder's own
// function.  The expressions compared -- |r_on - e_on| <= t_collar, |r_off - e_off| <= max(t_collar, pct * (r_off - r_on)),
// floor(t / res), ceil(t / res), cover >= rho * (b - a) -- hold subtractions, one product, one IEEE division, sums in a stated
// order and comparisons.  NOTHING here may be
// contracted into an FMA or reassociated, or a difference exactly on a collar would fall on the other side than on the host:
// this file is built with -ffp-contract=off and without fast-math (csrc/Makefile), and says so again below.  Like events.hip it
// may run beside a forward on another stream: -fno-slp-vectorize, no packed-FP32 instructions.
#include "acx_internal.h"
#include "device_common.h"

#pragma clang fp contract(off)

namespace acx {

constexpr long long kScMaxUnits = 2147483647LL;   // one workgroup per unit / per clip: the grid's x limit
// Segments per tile.  A workgroup keeps two int32 difference arrays of kScTile + 1 entries in LDS.  A CU holds 2048 threads:
// two workgroups of 1024 (N >= 1024) up to eight of 256 (N <= 256), and 160 KB / 8 = 20 KB each at eight.  2048 is the largest
// power of two whose two arrays (16392 bytes) fit that, so LDS does not limit residency for any N above 192.
constexpr int kScTile = ACX_SCORE_TILE_SEGMENTS;
static_assert(2 * (kScTile + 1) * 4 <= 20 * 1024, "the two difference arrays of a tile fit an eighth of the LDS");
constexpr int kScMaxTileWorkers = 16;             // workgroups that share the tiles of one clip (grid y)
constexpr int kScMaxSegments = 2147483646;        // a clip's segment count stays inside an int

struct ScArgs {
    const acx_ref_event* ref;
    long long n_ref;
    const acx_event* est;
    long long capacity;
    const long long* est_count;    // the decoder's *count and *status, still on the device
    const int* est_status;
    int N, G;                      // classes, units per clip = ceil(N / 64)
    const int* steps;              // [B]
    const double* end;             // [B] the clips' last boundaries
    double step;
    long long* counts;             // [N][3] TP, FP, FN
    int* status;
};

// the valid rows of the estimated table, or -1 when the decoder did not leave a usable one
__device__ __forceinline__ long long sc_est_rows(const ScArgs& a) {
    const long long n = *a.est_count;
    return (*a.est_status != 0 || n > a.capacity || n < 0) ? -1 : n;
}

__device__ __forceinline__ long long sc_key(int clip, int cls) { return ((long long)clip << 32) | (unsigned)cls; }

// One lower bound in flight: the first row of a table sorted by (clip, cls) whose key is >= key.  Rows of `stride` bytes begin
// with the int32 pair (clip, cls) -- acx_event and acx_ref_event both do.
struct ScBound {
    const char* t;
    long long stride, lo, hi, key;
    __device__ __forceinline__ bool open() const { return lo < hi; }
    __device__ __forceinline__ void step() {
        if (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            const int2 k = *reinterpret_cast<const int2*>(t + mid * stride);
            if (sc_key(k.x, k.y) < key) lo = mid + 1;
            else hi = mid;
        }
    }
};

// rows [rlo, rhi) of the reference table and [elo, ehi) of the estimated one that belong to (clip, cls): four independent
// searches stepped together, so their loads overlap
__device__ __forceinline__ void sc_ranges(const ScArgs& a, long long n_est, int clip, int cls, long long& rlo, long long& rhi,
                                          long long& elo, long long& ehi) {
    const long long k0 = sc_key(clip, cls), k1 = sc_key(clip, cls + 1);           // cls + 1 <= ACX_MAX_CLASSES: no overflow
    ScBound s[4] = {{reinterpret_cast<const char*>(a.ref), (long long)sizeof(acx_ref_event), 0, a.n_ref, k0},
                    {reinterpret_cast<const char*>(a.ref), (long long)sizeof(acx_ref_event), 0, a.n_ref, k1},
                    {reinterpret_cast<const char*>(a.est), (long long)sizeof(acx_event), 0, n_est, k0},
                    {reinterpret_cast<const char*>(a.est), (long long)sizeof(acx_event), 0, n_est, k1}};
    while (s[0].open() || s[1].open() || s[2].open() || s[3].open()) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i].step();
    }
    rlo = s[0].lo; rhi = s[1].lo; elo = s[2].lo; ehi = s[3].lo;
}

__device__ __forceinline__ void sc_add(long long* p, long long v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ---- event-based: greedy matching with onset / offset collars ----------------------------------------------------------------
// Reference events in table order; each takes the first estimated row of its column, in table order, that is not taken yet and
// passes both tests.  est_match doubles as the "taken" flag (-1: free); a lane re-reads only what it wrote itself.
// Both tables ascend in onset inside a column, and fl(r_on - e_on) is monotone in either argument, so with evaluate_onset a row
// in FRONT of a reference event's onset window is in front of every later one's (the pointer `low` never returns to it) and a row
// BEHIND the window ends the scan: neither changes which row is the first to pass.
__global__ __launch_bounds__(64) void sed_event_match_kernel(ScArgs a, acx_event_collar c, long long* ref_match,
                                                             long long* est_match) {
    const int lane = threadIdx.x;
    const long long unit = blockIdx.x;
    const int clip = (int)(unit / a.G), cls = (int)(unit - (long long)clip * a.G) * 64 + lane;
    const long long n_est = sc_est_rows(a);
    if (n_est < 0) {
        if (unit == 0 && lane == 0) atomicOr(a.status, ACX_SCORE_BAD_TABLE);
        return;
    }
    if (cls >= a.N) return;
    long long rlo, rhi, elo, ehi;
    sc_ranges(a, n_est, clip, cls, rlo, rhi, elo, ehi);
    const int steps = a.steps[clip];
    const double end = a.end[clip];
    const bool on = c.evaluate_onset != 0, off = c.evaluate_offset != 0;

    long long low = elo, tp = 0;
    for (long long r = rlo; r < rhi; ++r) {
        const double r_on = a.ref[r].onset, r_off = a.ref[r].offset;
        const double tol = fmax(c.t_collar, c.percentage_of_length * (r_off - r_on));      // one product, not contracted
        while (low < ehi) {                       // rows no reference event from here on can take
            if (est_match[low] < 0) {
                if (!on) break;
                const double e_on = event_edge(a.est[low].begin, steps, a.step, end);
                if (!(e_on < r_on) || fabs(r_on - e_on) <= c.t_collar) break;
            }
            ++low;
        }
        for (long long j = low; j < ehi; ++j) {
            const int2 be = *reinterpret_cast<const int2*>(&a.est[j].begin);
            if (on) {
                const double e_on = event_edge(be.x, steps, a.step, end);
                if (!(fabs(r_on - e_on) <= c.t_collar)) {
                    if (e_on > r_on) break;       // behind the window, and so is every later row
                    continue;
                }
            }
            if (est_match[j] >= 0) continue;
            if (off && !(fabs(r_off - event_edge(be.y, steps, a.step, end)) <= tol)) continue;
            ref_match[r] = j;
            est_match[j] = r;
            ++tp;
            break;
        }
    }
    sc_add(a.counts + (long long)cls * 3 + 0, tp);
    sc_add(a.counts + (long long)cls * 3 + 1, (ehi - elo) - tp);
    sc_add(a.counts + (long long)cls * 3 + 2, (rhi - rlo) - tp);
}

// ---- segment-based: activity on a fixed grid -----------------------------------------------------------------------------------
// floor(t / res) and ceil(t / res) as segment numbers clamped to [0, nseg]: IEEE division, exact floor / ceil
__device__ __forceinline__ int sc_clamp_seg(double f, int nseg) { return f >= (double)nseg ? nseg : f > 0.0 ? (int)f : 0; }
__device__ __forceinline__ int sc_seg_floor(double t, double res, int nseg) { return sc_clamp_seg(floor(t / res), nseg); }
__device__ __forceinline__ int sc_seg_ceil(double t, double res, int nseg) { return sc_clamp_seg(ceil(t / res), nseg); }

// The union of one column's intervals, one maximal run of active segments at a time, clipped to the tile [s0, s1).  row(i, a, b)
// gives the segments [a, b) of table row i, clamped to the clip; the rows ascend in a.  [a, b) is the current run; a == s1 when
// none is left.
template <class Row>
struct ScUnion {
    Row row;
    long long i, hi;
    int s0, s1;
    int a = 0, b = 0, na = 0, nb = 0;
    bool peeked = false;
    __device__ __forceinline__ ScUnion(Row row_, long long lo_, long long hi_, int s0_, int s1_)
        : row(row_), i(lo_), hi(hi_), s0(s0_), s1(s1_) { next(); }
    __device__ __forceinline__ bool done() const { return a >= s1; }
    __device__ __forceinline__ void next() {
        for (;;) {
            if (!peeked) {
                if (i >= hi) { a = b = s1; return; }
                row(i++, na, nb);
            }
            peeked = false;
            int ca = na, cb = nb;
            while (i < hi) {                      // rows that overlap or touch the run join it
                row(i++, na, nb);
                if (na > cb) { peeked = true; break; }
                cb = nb > cb ? nb : cb;
            }
            if (ca >= s1) { a = b = s1; i = hi; peeked = false; return; }       // behind the tile, and so is every later row
            if (cb <= s0 || ca >= cb) continue;                                     // in front of the tile, or empty
            a = ca > s0 ? ca : s0;
            b = cb < s1 ? cb : s1;
            return;
        }
    }
};
template <class Row>
__device__ __forceinline__ ScUnion<Row> sc_union(Row row, long long lo, long long hi, int s0, int s1) {
    return ScUnion<Row>(row, lo, hi, s0, s1);
}

__global__ __launch_bounds__(1024) void sed_segment_kernel(ScArgs a, double res, long long* overall) {
    __shared__ int s_fn[kScTile + 1], s_fp[kScTile + 1];       // difference arrays: misses and false alarms per segment
    __shared__ int s_wave[2][16];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int clip = blockIdx.x;
    const long long n_est = sc_est_rows(a);
    if (n_est < 0) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) atomicOr(a.status, ACX_SCORE_BAD_TABLE);
        return;
    }
    const int steps = a.steps[clip];
    const double end = a.end[clip], step = a.step;
    const int nseg = sc_clamp_seg(ceil(end / res), kScMaxSegments);

    for (long long t0 = (long long)blockIdx.y * kScTile; t0 < nseg; t0 += (long long)gridDim.y * kScTile) {
        const int s0 = (int)t0, s1 = (int)(t0 + kScTile < nseg ? t0 + kScTile : nseg), len = s1 - s0;
        for (int i = tid; i <= len; i += nt) { s_fn[i] = 0; s_fp[i] = 0; }
        __syncthreads();

        long long tp_all = 0, nref_all = 0, nsys_all = 0;
        for (int cls = tid; cls < a.N; cls += nt) {
            long long rlo, rhi, elo, ehi;
            sc_ranges(a, n_est, clip, cls, rlo, rhi, elo, ehi);
            auto R = sc_union([&](long long i, int& x, int& y) {
                x = sc_seg_floor(a.ref[i].onset, res, nseg);
                y = sc_seg_ceil(a.ref[i].offset, res, nseg);
            }, rlo, rhi, s0, s1);
            auto E = sc_union([&](long long i, int& x, int& y) {
                const int2 be = *reinterpret_cast<const int2*>(&a.est[i].begin);
                x = sc_seg_floor(event_edge(be.x, steps, step, end), res, nseg);
                y = sc_seg_ceil(event_edge(be.y, steps, step, end), res, nseg);
            }, elo, ehi, s0, s1);
            // walk the tile from change to change; a run [a, b) that is current has b > p
            int tp = 0, fp = 0, fn = 0;
            for (int p = s0; p < s1;) {
                const bool in_r = R.a <= p, in_e = E.a <= p;
                const int qr = in_r ? R.b : R.a, qe = in_e ? E.b : E.a;
                const int q = qr < qe ? qr : qe;                       // <= s1: a finished union stands at s1
                if (in_r && in_e) {
                    tp += q - p;
                } else if (in_r) {
                    fn += q - p;
                    atomicAdd(&s_fn[p - s0], 1);
                    atomicAdd(&s_fn[q - s0], -1);
                } else if (in_e) {
                    fp += q - p;
                    atomicAdd(&s_fp[p - s0], 1);
                    atomicAdd(&s_fp[q - s0], -1);
                }
                p = q;
                if (!R.done() && R.b <= p) R.next();
                if (!E.done() && E.b <= p) E.next();
            }
            sc_add(a.counts + (long long)cls * 3 + 0, tp);
            sc_add(a.counts + (long long)cls * 3 + 1, fp);
            sc_add(a.counts + (long long)cls * 3 + 2, fn);
            tp_all += tp; nref_all += tp + fn; nsys_all += tp + fp;
        }
        __syncthreads();

        // prefix sums of the two arrays: thread i owns a contiguous chunk of the tile
        const int chunk = (len + nt - 1) / nt;
        const int lo = tid * chunk < len ? tid * chunk : len, hi = lo + chunk < len ? lo + chunk : len;
        int dfn = 0, dfp = 0;
        for (int i = lo; i < hi; ++i) { dfn += s_fn[i]; dfp += s_fp[i]; }
        int ifn = dfn, ifp = dfp;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int un = __shfl_up(ifn, d, 64), up = __shfl_up(ifp, d, 64);
            if (lane >= d) { ifn += un; ifp += up; }
        }
        if (lane == 63) { s_wave[0][wave] = ifn; s_wave[1][wave] = ifp; }
        __syncthreads();
        int fn = ifn - dfn, fp = ifp - dfp;
        for (int w = 0; w < wave; ++w) { fn += s_wave[0][w]; fp += s_wave[1][w]; }
        long long S = 0, D = 0, I = 0;
        for (int i = lo; i < hi; ++i) {
            fn += s_fn[i]; fp += s_fp[i];
            S += fn < fp ? fn : fp;
            D += fn > fp ? fn - fp : 0;
            I += fp > fn ? fp - fn : 0;
        }
        const long long v[6] = {wave_sum(tp_all), wave_sum(S), wave_sum(D), wave_sum(I), wave_sum(nref_all), wave_sum(nsys_all)};
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) sc_add(overall + k, v[k]);
        }
        __syncthreads();                          // the next tile clears the arrays
    }
}

// ---- intersection-based: the criteria of PSDS ---------------------------------------------------------------------------------
// One row of the cover walk of pytorch/sed_metrics.py::_cover: [a, b) is the interval measured, `covered` starts at a and `total`
// at 0.0, the rows (on, off) come ascending in on.  false: this row begins at or behind b, and so does every later one.
__device__ __forceinline__ bool sc_cover_row(double on, double off, double b, double& covered, double& total) {
    if (on >= b) return false;
    const double lo = fmax(on, covered), hi = fmin(off, b);
    if (hi > lo) { total += hi - lo; covered = hi; }
    return true;
}

// rows [lo, hi) of the reference table that belong to `clip`, every class: two lower bounds stepped together
__device__ __forceinline__ void sc_clip_range(const ScArgs& a, int clip, long long& lo, long long& hi) {
    ScBound s[2] = {{reinterpret_cast<const char*>(a.ref), (long long)sizeof(acx_ref_event), 0, a.n_ref, (long long)clip << 32},
                    {reinterpret_cast<const char*>(a.ref), (long long)sizeof(acx_ref_event), 0, a.n_ref, ((long long)clip + 1) << 32}};
    while (s[0].open() || s[1].open()) {
        s[0].step();
        s[1].step();
    }
    lo = s[0].lo; hi = s[1].lo;
}

// A lane's three passes over its column.  Detections of a column ascend in onset and do not overlap; reference events ascend in
// onset and may overlap.  A row that ends at or before the interval's beginning adds nothing to its cover (hi <= a <= covered
// <= lo), nor to that of any later interval of the column, whose beginning is no smaller: `low` passes such rows once, from
// the front only, so that a long column costs its length and not its square.  est_rel is written in the first pass and read
// in the third by the lane that wrote it.
__global__ __launch_bounds__(64) void sed_intersection_kernel(ScArgs a, acx_intersection_criteria c, long long* ct,
                                                              long long* ref_hit, long long* est_rel) {
    const int lane = threadIdx.x;
    const long long unit = blockIdx.x;
    const int clip = (int)(unit / a.G), cls = (int)(unit - (long long)clip * a.G) * 64 + lane;
    const long long n_est = sc_est_rows(a);
    if (n_est < 0) {
        if (unit == 0 && lane == 0) atomicOr(a.status, ACX_SCORE_BAD_TABLE);
        return;
    }
    if (cls >= a.N) return;
    long long rlo, rhi, elo, ehi, clo = 0, chi = 0;
    sc_ranges(a, n_est, clip, cls, rlo, rhi, elo, ehi);
    const bool cross = c.cross_triggers != 0 && ct != nullptr;
    if (cross && ehi > elo) sc_clip_range(a, clip, clo, chi);
    const int steps = a.steps[clip];
    const double end = a.end[clip];

    // 1. detection tolerance: a detection is relevant when the annotations of its column cover dtc of its length
    long long low = rlo, fp = 0;
    for (long long j = elo; j < ehi; ++j) {
        const int2 be = *reinterpret_cast<const int2*>(&a.est[j].begin);
        const double d_on = event_edge(be.x, steps, a.step, end), d_off = event_edge(be.y, steps, a.step, end);
        while (low < rhi && a.ref[low].offset <= d_on) ++low;
        double covered = d_on, total = 0.0;
        for (long long r = low; r < rhi; ++r)
            if (!sc_cover_row(a.ref[r].onset, a.ref[r].offset, d_off, covered, total)) break;
        const bool relevant = total >= c.dtc * (d_off - d_on);                      // one product, not contracted
        est_rel[j] = relevant ? 1 : 0;
        if (relevant) continue;
        ++fp;
        if (!cross) continue;
        // 2. cross triggers of a false positive: the clip's annotations, class group by class group
        for (long long i = clo; i < chi;) {
            const int k = a.ref[i].cls;
            if (k == cls) { i = rhi; continue; }                                    // its own column is [rlo, rhi)
            double cov = d_on, sum = 0.0;
            bool more = true;
            for (; i < chi && a.ref[i].cls == k; ++i)
                if (more) more = sc_cover_row(a.ref[i].onset, a.ref[i].offset, d_off, cov, sum);
            if ((unsigned)k < (unsigned)a.N && sum >= c.cttc * (d_off - d_on)) sc_add(ct + (long long)cls * a.N + k, 1);
        }
    }

    // 3. ground-truth intersection: an annotation is found when the relevant detections of its column cover gtc of its length
    long long tp = 0;
    low = elo;
    for (long long r = rlo; r < rhi; ++r) {
        const double g_on = a.ref[r].onset, g_off = a.ref[r].offset;
        while (low < ehi && event_edge(a.est[low].end, steps, a.step, end) <= g_on) ++low;
        double covered = g_on, total = 0.0;
        for (long long j = low; j < ehi; ++j) {
            const int2 be = *reinterpret_cast<const int2*>(&a.est[j].begin);
            const double d_on = event_edge(be.x, steps, a.step, end);
            if (d_on >= g_off) break;                                               // what sc_cover_row would answer
            if (est_rel[j] == 0) continue;
            sc_cover_row(d_on, event_edge(be.y, steps, a.step, end), g_off, covered, total);
        }
        const bool hit = total >= c.gtc * (g_off - g_on);
        ref_hit[r] = hit ? 1 : 0;
        tp += hit ? 1 : 0;
    }
    sc_add(a.counts + (long long)cls * 3 + 0, tp);
    sc_add(a.counts + (long long)cls * 3 + 1, fp);
    sc_add(a.counts + (long long)cls * 3 + 2, (rhi - rlo) - tp);
}

// rate[c] = the mean over k != c with weight[k] > 0 of ct[c][k] * weight[k]: one thread's sum in ascending k, then one division
__global__ __launch_bounds__(256) void cross_trigger_rate_kernel(const long long* ct, const double* weight, int N, double* rate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const long long* row = ct + (long long)c * N;
    double acc = 0.0;
    int n = 0;
    for (int k = 0; k < N; ++k) {
        const double w = weight[k];
        if (k == c || !(w > 0.0)) continue;
        acc += (double)row[k] * w;                                                  // a product, then a sum: not contracted
        ++n;
    }
    rate[c] = n > 0 ? acc / (double)n : 0.0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int sc_check(const char* who, const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity,
                    const int64_t* est_count, const int* est_status, int64_t B, int N, const int* steps, const double* end_seconds,
                    double step_seconds, const int64_t* counts, const int* status) {
    if (!est_count || !est_status || !steps || !end_seconds || !counts || !status || (n_ref > 0 && !ref) || (capacity > 0 && !est))
        ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (n_ref < 0) ACX_FAIL(ACX_ERR_ARG, "%s: n_ref %lld (expected >= 0)", who, (long long)n_ref);
    if (capacity < 0) ACX_FAIL(ACX_ERR_ARG, "%s: capacity %lld (expected >= 0)", who, (long long)capacity);
    if (!(step_seconds > 0.0)) ACX_FAIL(ACX_ERR_ARG, "%s: step_seconds %g (expected > 0)", who, step_seconds);
    if (B < 1) ACX_FAIL(ACX_ERR_SHAPE, "%s: B = %lld (expected >= 1)", who, (long long)B);
    if (N < 1 || N > ACX_MAX_CLASSES) ACX_FAIL(ACX_ERR_SHAPE, "%s: %d classes (expected 1 .. %d)", who, N, ACX_MAX_CLASSES);
    if (B > kScMaxUnits / ((N + 63) / 64))
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: %lld clips of %d classes need more than %lld workgroups", who, (long long)B, N,
                 kScMaxUnits);
    return ACX_OK;
}

static ScArgs sc_args(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity, const int64_t* est_count,
                      const int* est_status, int N, const int* steps, const double* end_seconds, double step_seconds,
                      int64_t* counts, int* status) {
    ScArgs a{};
    a.ref = ref; a.n_ref = n_ref; a.est = est; a.capacity = capacity;
    a.est_count = reinterpret_cast<const long long*>(est_count); a.est_status = est_status;
    a.N = N; a.G = (N + 63) / 64;
    a.steps = steps; a.end = end_seconds; a.step = step_seconds;
    a.counts = reinterpret_cast<long long*>(counts); a.status = status;
    return a;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_score_events(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity, const int64_t* est_count,
                     const int* est_status, int64_t B, int N, const int* steps, const double* end_seconds, double step_seconds,
                     const acx_event_collar* c, int64_t* counts, int64_t* ref_match, int64_t* est_match, int* status,
                     void* stream) {
    const char* who = "acx_score_events";
    if (!c || (n_ref > 0 && !ref_match) || (capacity > 0 && !est_match)) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(sc_check(who, ref, n_ref, est, capacity, est_count, est_status, B, N, steps, end_seconds, step_seconds, counts, status));
    if (!(c->t_collar >= 0.0 && c->t_collar <= 1.7976931348623157e308) ||
        !(c->percentage_of_length >= 0.0 && c->percentage_of_length <= 1.7976931348623157e308))
        ACX_FAIL(ACX_ERR_ARG, "%s: t_collar %g and percentage_of_length %g must be finite and not negative", who, c->t_collar,
                 c->percentage_of_length);
    const hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    ACX_HIP(hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(int64_t), s));
    if (n_ref > 0) ACX_HIP(hipMemsetAsync(ref_match, 0xff, (size_t)n_ref * sizeof(int64_t), s));        // -1
    if (capacity > 0) ACX_HIP(hipMemsetAsync(est_match, 0xff, (size_t)capacity * sizeof(int64_t), s));
    const ScArgs a = sc_args(ref, n_ref, est, capacity, est_count, est_status, N, steps, end_seconds, step_seconds, counts, status);
    launch_kernel(&sed_event_match_kernel, dim3((unsigned)(B * a.G)), dim3(64), 0, s, a, *c, reinterpret_cast<long long*>(ref_match),
                  reinterpret_cast<long long*>(est_match));
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_score_segments(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity, const int64_t* est_count,
                       const int* est_status, int64_t B, int N, const int* steps, const double* end_seconds, double step_seconds,
                       double time_resolution, int64_t* counts, int64_t* overall, int* status, void* stream) {
    const char* who = "acx_score_segments";
    if (!overall) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(sc_check(who, ref, n_ref, est, capacity, est_count, est_status, B, N, steps, end_seconds, step_seconds, counts, status));
    if (!(time_resolution > 0.0 && time_resolution <= 1.7976931348623157e308))
        ACX_FAIL(ACX_ERR_ARG, "%s: time_resolution %g (expected a finite value > 0)", who, time_resolution);
    const hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    ACX_HIP(hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(int64_t), s));
    ACX_HIP(hipMemsetAsync(overall, 0, 6 * sizeof(int64_t), s));
    const ScArgs a = sc_args(ref, n_ref, est, capacity, est_count, est_status, N, steps, end_seconds, step_seconds, counts, status);
    // a thread per class, up to a full workgroup; few clips share their tiles among more workgroups
    const int threads = N >= 1024 ? 1024 : (N + 63) / 64 * 64;
    const long long workers = (1024 + B - 1) / B;
    const dim3 grid((unsigned)B, (unsigned)(workers < 1 ? 1 : workers > kScMaxTileWorkers ? kScMaxTileWorkers : workers));
    launch_kernel(&sed_segment_kernel, grid, dim3(threads), 0, s, a, time_resolution, reinterpret_cast<long long*>(overall));
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_score_intersection(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity, const int64_t* est_count,
                           const int* est_status, int64_t B, int N, const int* steps, const double* end_seconds, double step_seconds,
                           const acx_intersection_criteria* c, int64_t* counts, int64_t* cross_triggers, int64_t* ref_hit,
                           int64_t* est_relevant, int* status, void* stream) {
    const char* who = "acx_score_intersection";
    if (!c || (n_ref > 0 && !ref_hit) || (capacity > 0 && !est_relevant)) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    ACX_TRY(sc_check(who, ref, n_ref, est, capacity, est_count, est_status, B, N, steps, end_seconds, step_seconds, counts, status));
    const double rho[3] = {c->dtc, c->gtc, c->cttc};
    const char* const name[3] = {"dtc", "gtc", "cttc"};
    for (int i = 0; i < (c->cross_triggers ? 3 : 2); ++i)
        if (!(rho[i] > 0.0 && rho[i] <= 1.0))
            ACX_FAIL(ACX_ERR_ARG, "%s: %s %g (expected a threshold in (0, 1])", who, name[i], rho[i]);
    if (c->cross_triggers && !cross_triggers)
        ACX_FAIL(ACX_ERR_ARG, "%s: cross_triggers is set and the matrix is null", who);
    const hipStream_t s = (hipStream_t)stream;
    const bool cross = c->cross_triggers != 0;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    ACX_HIP(hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(int64_t), s));
    if (cross) ACX_HIP(hipMemsetAsync(cross_triggers, 0, (size_t)N * N * sizeof(int64_t), s));
    if (n_ref > 0) ACX_HIP(hipMemsetAsync(ref_hit, 0, (size_t)n_ref * sizeof(int64_t), s));
    if (capacity > 0) ACX_HIP(hipMemsetAsync(est_relevant, 0xff, (size_t)capacity * sizeof(int64_t), s));   // -1
    const ScArgs a = sc_args(ref, n_ref, est, capacity, est_count, est_status, N, steps, end_seconds, step_seconds, counts, status);
    launch_kernel(&sed_intersection_kernel, dim3((unsigned)(B * a.G)), dim3(64), 0, s, a, *c,
                  cross ? reinterpret_cast<long long*>(cross_triggers) : nullptr, reinterpret_cast<long long*>(ref_hit),
                  reinterpret_cast<long long*>(est_relevant));
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_cross_trigger_rate(const int64_t* cross_triggers, const double* weight, int N, double* rate, void* stream) {
    const char* who = "acx_cross_trigger_rate";
    if (!cross_triggers || !weight || !rate) ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (N < 1 || N > ACX_MAX_CLASSES) ACX_FAIL(ACX_ERR_SHAPE, "%s: %d classes (expected 1 .. %d)", who, N, ACX_MAX_CLASSES);
    launch_kernel(&cross_trigger_rate_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                  reinterpret_cast<const long long*>(cross_triggers), weight, N, rate);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
