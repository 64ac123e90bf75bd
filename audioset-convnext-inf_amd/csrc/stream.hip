// Live streams (acx_stream_*, include/acx.h): recordings that arrive chunk by chunk, tagged window by window as soon as a
// window is complete, with the bits of acx_forward_windows over the whole recording.
//
// Each slot owns a mirrored 32 kHz ring of C samples: sample p sits at both p mod C and C + (p mod C) of the slot's 2C
// region, so any span of up to C samples is contiguous at slot 2C + (s mod C) and a window goes through the unchanged uniform
// forward by its table offset (forward_uniform with wstart, the acx_forward_windows path).  At an input rate other than
// 32 kHz, pushes land in a per-slot input history and the outputs that became final are resampled into the ring by res_tile,
// the tile body resample_kernel calls.  With a timeline, the probabilities of each forwarded window are kept in a per-slot
// history of Hw windows, and the rows that became final are reduced from it by the calls window_timeline_kernel makes: win_mid,
// win_cover and win_reduce.
//
// The host owns every position and count (the schedule below).  Launches take them BY VALUE, in blocks of at most
// kStrBatch slots (about 1 KiB), so a call copies nothing from the host and allocates and synchronises nothing.
#include <algorithm>
#include <climits>
#include <vector>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kModelRate = 32000;
constexpr int kStrBatch = 32;            // slots per append / resample / timeline launch
constexpr int kStrTable = 128;           // windows per table / stash launch
constexpr int kStrThreads = 256;
constexpr long long kStrOpen = 1LL << 60;    // the length of a recording that is still open (no end-aligned window yet)

// ---- the schedule (host only) ---------------------------------------------------------------------------------------------
struct StrGeom {
    long long W = 0, H = 0;
    int orig = kModelRate, of = 1, nf = 1, width = 0;
    std::vector<long long> q;            // resampling: output j nf + i is final once j of + q[i] + 1 input samples are pushed
    long long qmax = 0;
};

static int str_geom(int64_t window, int64_t hop, int orig_hz, StrGeom* g) {
    if (window < ACX_MIN_SAMPLES)
        ACX_FAIL(ACX_ERR_SHAPE, "stream: window of %lld samples is too short: kernel size can't be greater than actual input size "
                 "(minimum is %d samples)", (long long)window, ACX_MIN_SAMPLES);
    if (window > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "stream: window of %lld samples is longer than 2^31 - 1", (long long)window);
    if (hop < 1 || hop > window)
        ACX_FAIL(ACX_ERR_ARG, "stream: hop of %lld samples (expected 1 .. window = %lld: a longer hop leaves audio uncovered)",
                 (long long)hop, (long long)window);
    g->W = window;
    g->H = hop;
    g->orig = orig_hz;
    if (orig_hz == kModelRate) {
        g->q.assign(1, 0);
        return ACX_OK;
    }
    int of = 0, nf = 0, width = 0, mb = 0;
    ACX_TRY(acx_resample_geometry(orig_hz, kModelRate, &of, &nf, &width, &mb));
    std::vector<int> st(nf), ct(nf);
    ACX_TRY(acx_resample_taps(orig_hz, kModelRate, st.data(), ct.data(), nullptr, 0));
    g->of = of; g->nf = nf; g->width = width;
    // the last input output j nf + i reads is j of + e_i (resample_kernel: band start - width + count - 1); prefix maxima make
    // the requirement non-decreasing in n, and one period back is the only earlier one that can exceed this period's
    std::vector<long long> pm(nf);
    long long m = LLONG_MIN / 4;
    for (int i = 0; i < nf; ++i) {
        if (ct[i] > 0) m = std::max(m, (long long)st[i] - width + ct[i] - 1);
        pm[i] = m;
    }
    g->q.resize(nf);
    for (int i = 0; i < nf; ++i) g->q[i] = std::max(pm[i], pm[nf - 1] - of);
    g->qmax = std::max(0LL, pm[nf - 1]);
    return ACX_OK;
}

// final 32 kHz samples of a recording of P input samples (closed: all ceil(nf P / of) of them)
static long long str_final(const StrGeom& g, long long P, bool closed) {
    if (g.orig == kModelRate) return P;
    const long long N = ((long long)g.nf * P + g.of - 1) / g.of;
    if (closed) return N;
    long long lo = 0, hi = N;               // the first output whose band is not all pushed
    while (lo < hi) {
        const long long n = lo + (hi - lo) / 2;
        if ((n / g.nf) * g.of + g.q[n % g.nf] + 1 <= P) lo = n + 1; else hi = n;
    }
    return lo;
}
// windows emitted so far by a recording with R final samples (closed: R = L, its whole length)
static long long str_windows(const StrGeom& g, long long R, bool closed) {
    if (closed) return R < ACX_MIN_SAMPLES ? 0 : win_count(R, g.W, g.H);
    return R >= g.W ? (R - g.W) / g.H + 1 : 0;
}
// timeline rows emitted so far: open, row k once k H + H / 2 < R - W; closed, all ceil(L / H)
static long long str_rows(const StrGeom& g, long long R, bool closed) {
    if (closed) return R < ACX_MIN_SAMPLES ? 0 : win_steps(R, g.H);
    const long long x = R - g.W - g.H / 2;
    return x > 0 ? (x + g.H - 1) / g.H : 0;
}

// The sizes of one slot's device state (host only; acx_stream_create allocates exactly these, acx_stream_geometry reports them):
//   adv  the largest 32 kHz advance of one push of max_push input samples, or of a close (the outputs that read past the end);
//   C    the mirrored ring: a window plus one advance, so no pending window is overwritten;
//   Ch   the input history (0 at 32 kHz): one push behind the oldest input the first output that is not final yet reads;
//   Hw   the probability history (0 without a timeline): every window under a row that is not final yet, plus one advance.
struct StrSizes {
    long long adv = 0, C = 0, Ch = 0, Hw = 0;
};
static int str_sizes(const StrGeom& g, int64_t max_push, bool timeline, const char* who, StrSizes* z) {
    if (max_push < 1 || max_push > 0x7fffffffLL)
        ACX_FAIL(ACX_ERR_ARG, "%s: max_push of %lld samples (expected 1 .. 2^31 - 1)", who, (long long)max_push);
    const bool res = g.orig != kModelRate;
    z->adv = res ? ((max_push + g.qmax + 1 + 2LL * g.of) * g.nf + g.of - 1) / g.of + 2 : max_push;
    z->C = (g.W + z->adv + 63) / 64 * 64;
    z->Ch = res ? (max_push + g.qmax + g.width + g.of + 64 + 63) / 64 * 64 : 0;
    z->Hw = timeline ? (g.W + z->adv) / g.H + 4 : 0;
    if (z->C > 0x7fffffffLL) ACX_FAIL(ACX_ERR_ARG, "%s: window + max_push exceed 2^31 samples at 32 kHz", who);
    return ACX_OK;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------
struct StrAppend {
    int n, mirror;
    long long cap;
    int slot[kStrBatch], len[kStrBatch];
    long long pos[kStrBatch], src[kStrBatch];
};

// Entry e = blockIdx.y: len samples from in + src to positions pos .. pos + len - 1 of its slot's ring (cap samples; mirrored:
// each also at cap + its offset).  len <= cap, so one wrap at most.  The 16-byte part is moved as float4 when source and
// destination line up.
__global__ __launch_bounds__(kStrThreads) void stream_append_kernel(StrAppend a, const float* __restrict__ in,
                                                                   float* __restrict__ dst) {
    const int e = blockIdx.y;
    const int len = a.len[e];
    const long long cap = a.cap;
    float* d = dst + (long long)a.slot[e] * (a.mirror ? 2 * cap : cap);
    const float* x = in + a.src[e];
    const long long p0 = a.pos[e] % cap;
    const bool wide = ((p0 | cap) & 3) == 0 && ((uintptr_t)x & 15) == 0;
    if (wide) {
        for (int k = (blockIdx.x * kStrThreads + threadIdx.x) * 4; k < len; k += gridDim.x * kStrThreads * 4) {
            long long q = p0 + k;
            if (q >= cap) q -= cap;                     // q, cap multiples of 4: the 4 samples never straddle the wrap
            if (k + 4 <= len) {
                const float4 v = *reinterpret_cast<const float4*>(x + k);
                *reinterpret_cast<float4*>(d + q) = v;
                if (a.mirror) *reinterpret_cast<float4*>(d + cap + q) = v;
            } else {
                for (int u = 0; k + u < len; ++u) {
                    const float v = x[k + u];
                    d[q + u] = v;
                    if (a.mirror) d[cap + q + u] = v;
                }
            }
        }
        return;
    }
    for (int k = blockIdx.x * kStrThreads + threadIdx.x; k < len; k += gridDim.x * kStrThreads) {
        long long q = p0 + k;
        if (q >= cap) q -= cap;
        const float v = x[k];
        d[q] = v;
        if (a.mirror) d[cap + q] = v;
    }
}

struct StrRes {
    int n;
    int slot[kStrBatch], nout[kStrBatch];
    long long out0[kStrBatch], in1[kStrBatch];
};
// Outputs out0 .. out0 + nout - 1 of each entry's slot, tile by tile through res_tile: the input comes from the slot's input
// history of Ch samples, zero below sample 0 and from in1 (the samples pushed) on, and every output is written mirrored into
// the slot's 32 kHz ring of C samples.
static_assert(kStrThreads == kResThreads, "res_tile strides by kResThreads");
__global__ __launch_bounds__(kStrThreads) void stream_resample_kernel(StrRes a, ResGeom g, long long C, long long Ch,
                                                                     const float* __restrict__ hin, float* __restrict__ ring,
                                                                     const int2* __restrict__ band, const float* __restrict__ taps) {
    extern __shared__ float s_in[];
    __shared__ long long s_toff[kStrBatch + 1];
    const int T = kStrThreads * g.per_thread;
    if (threadIdx.x == 0) packed_prefix(a.n, s_toff, [&a, T](int e) { return (long long)((a.nout[e] + T - 1) / T); });
    __syncthreads();
    const long long tiles = s_toff[a.n];
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int e = packed_find(s_toff, a.n, t);
        const long long nb = a.out0[e] + (t - s_toff[e]) * T;
        const float* x = hin + (long long)a.slot[e] * Ch;
        const long long in1 = a.in1[e];
        float* y = ring + (long long)a.slot[e] * 2 * C;
        res_tile(g, nb, (int)min((long long)T, a.out0[e] + a.nout[e] - nb), s_in, band, taps,
                 [x, in1, Ch](long long m) { return (m >= 0 && m < in1) ? x[m % Ch] : 0.0f; },
                 [y, nb, C](int d, float v) {
                     const long long p = (nb + d) % C;
                     y[p] = v;
                     y[C + p] = v;
                 });
    }
}

struct StrTable {
    int n;
    long long off[kStrTable];
};
__global__ __launch_bounds__(kStrTable) void stream_table_kernel(StrTable a, long long* __restrict__ wstart) {
    if ((int)threadIdx.x < a.n) wstart[threadIdx.x] = a.off[threadIdx.x];
}

struct StrStash {
    int n;
    long long row[kStrTable];
};
// window b's N probabilities -> history row a.row[b]
__global__ __launch_bounds__(kStrThreads) void stream_stash_kernel(StrStash a, const float* __restrict__ probs, int N,
                                                                  float* __restrict__ hist) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < N; c += kStrThreads)
        hist[a.row[b] * N + c] = probs[(long long)b * N + c];
}

struct StrRows {
    int n;
    long long W, H, Hw;
    int slot[kStrBatch], rows[kStrBatch];
    long long k0[kStrBatch], L[kStrBatch];
};
// One workgroup per row (grid-stride), threads striding over the N classes: row k of entry e's slot is reduced over the windows
// that win_cover names, read from the slot's window history (window j at row j mod Hw).  L = kStrOpen while the recording is open.
__global__ __launch_bounds__(kStrThreads) void stream_timeline_kernel(StrRows a, const float* __restrict__ hist, int N,
                                                                     int reduce, float* __restrict__ out) {
    __shared__ long long s_roff[kStrBatch + 1];
    if (threadIdx.x == 0) packed_prefix(a.n, s_roff, [&a](int e) { return (long long)a.rows[e]; });
    __syncthreads();
    const long long total = s_roff[a.n];
    for (long long row = blockIdx.x; row < total; row += gridDim.x) {
        const int e = packed_find(s_roff, a.n, row);
        const long long L = a.L[e];
        long long j0, j1;
        win_cover(win_mid(a.k0[e] + (row - s_roff[e]), a.H, L), L, a.W, a.H, &j0, &j1);
        const float* hs = hist + (long long)a.slot[e] * a.Hw * N;
        const long long Hw = a.Hw;
        for (int c = threadIdx.x; c < N; c += kStrThreads)
            out[row * N + c] = win_reduce([hs, Hw, N](long long j) { return hs + (j % Hw) * N; }, j0, j1 - j0, c, reduce);
    }
}

}  // namespace acx

using namespace acx;

struct acx_stream {
    acx_ctx* ctx = nullptr;
    int device = 0, slots = 0;
    int classes = 0;                        // N of the context at create: the width of the probability history and the rows
    bool timeline = false;
    StrGeom g;
    long long max_push = 0, adv_max = 0, C = 0, Ch = 0, Hw = 0;
    acx_resampler* rs = nullptr;
    float *ring = nullptr, *hin = nullptr, *hist = nullptr;
    struct Slot {
        long long in = 0, out = 0;          // input samples pushed, final 32 kHz samples
        bool closed = false;
        long long win_done = 0, row_done = 0;
    };
    std::vector<Slot> s;
    long long windows(const Slot& x) const { return str_windows(g, x.out, x.closed); }
    long long rows(const Slot& x) const { return timeline ? str_rows(g, x.out, x.closed) : 0; }
    bool busy(const Slot& x) const { return x.win_done < windows(x) || x.row_done < rows(x); }
    long long win_len(const Slot& x) const { return x.closed && x.out < g.W ? x.out : g.W; }
    long long win_at(const Slot& x, long long j) const { return x.closed ? win_start(j, x.out, g.W, g.H) : j * g.H; }
};

namespace {
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(d); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// the first `max` pending windows of one length, in slot order and then start order
int pending_run(const acx_stream* st, int max, int* slot_of, int64_t* start_of, int64_t* length, int* count) {
    int n = 0;
    long long len = 0;
    for (int i = 0; i < st->slots && n < max; ++i) {
        const acx_stream::Slot& x = st->s[i];
        const long long w = st->windows(x);
        if (x.win_done >= w) continue;
        const long long l = st->win_len(x);
        if (n > 0 && l != len) break;
        len = l;
        for (long long j = x.win_done; j < w && n < max; ++j, ++n) {
            if (slot_of) slot_of[n] = i;
            if (start_of) start_of[n] = st->win_at(x, j);
        }
    }
    *count = n;
    if (length) *length = n ? len : 0;
    return ACX_OK;
}

int check_slots(const acx_stream* st, const int* slot, int n, const char* who) {
    if (!slot) ACX_FAIL(ACX_ERR_ARG, "%s: slot is null", who);
    std::vector<char> seen(st->slots, 0);
    for (int k = 0; k < n; ++k) {
        if (slot[k] < 0 || slot[k] >= st->slots)
            ACX_FAIL(ACX_ERR_ARG, "%s: slot %d out of range (the handle has %d)", who, slot[k], st->slots);
        if (seen[slot[k]]) ACX_FAIL(ACX_ERR_ARG, "%s: slot %d is listed twice", who, slot[k]);
        seen[slot[k]] = 1;
        if (st->busy(st->s[slot[k]]))
            ACX_FAIL(ACX_ERR_STATE, "%s: slot %d has windows or timeline rows that are not fetched yet (acx_stream_forward, "
                     "acx_stream_timeline)", who, slot[k]);
    }
    return ACX_OK;
}

// resample outputs [out0[k], out1[k]) of the listed slots into the ring; in1 = samples pushed (zeros from there on)
int launch_stream_resample(acx_stream* st, const std::vector<int>& slot, const std::vector<long long>& out0,
                           const std::vector<long long>& out1, const std::vector<long long>& in1, hipStream_t s) {
    const StrGeom& g = st->g;
    const ResGeom rg{g.of, g.nf, g.width, st->rs->per_thread};
    const long long T = (long long)kStrThreads * st->rs->per_thread;
    StrRes a{};
    long long tiles = 0;
    auto flush = [&]() -> int {
        if (a.n == 0) return ACX_OK;
        launch_kernel(&stream_resample_kernel, dim3((unsigned)std::min(tiles, 4096LL)), dim3(kStrThreads), st->rs->lds_bytes, s,
                      a, rg, st->C, st->Ch, (const float*)st->hin, st->ring, (const int2*)st->rs->band, (const float*)st->rs->taps);
        ACX_HIP(hipGetLastError());
        a = StrRes{};
        tiles = 0;
        return ACX_OK;
    };
    for (size_t k = 0; k < slot.size(); ++k) {
        const long long n = out1[k] - out0[k];
        if (n <= 0) continue;
        // the oldest input the first tile stages must still be in the history
        if (out0[k] * g.of / g.nf - g.width - 1 < in1[k] - st->Ch)
            ACX_FAIL(ACX_ERR_STATE, "stream: slot %d: the input history of %lld samples does not reach back far enough",
                     slot[k], st->Ch);
        a.slot[a.n] = slot[k];
        a.nout[a.n] = (int)n;
        a.out0[a.n] = out0[k];
        a.in1[a.n] = in1[k];
        ++a.n;
        tiles += (n + T - 1) / T;
        if (a.n == kStrBatch) ACX_TRY(flush());
    }
    return flush();
}
}  // namespace

extern "C" {

int acx_stream_schedule(int64_t window, int64_t hop, int orig_hz, int64_t pushed, int closed, int64_t* samples,
                        int64_t* windows, int64_t* rows) {
    StrGeom g;
    ACX_TRY(str_geom(window, hop, orig_hz, &g));
    if (pushed < 0 || pushed > (1LL << 50))
        ACX_FAIL(ACX_ERR_ARG, "acx_stream_schedule: %lld samples pushed (expected 0 .. 2^50)", (long long)pushed);
    if (closed != 0 && closed != 1) ACX_FAIL(ACX_ERR_ARG, "acx_stream_schedule: closed must be 0 or 1 (got %d)", closed);
    const long long R = str_final(g, pushed, closed != 0);
    if (samples) *samples = R;
    if (windows) *windows = str_windows(g, R, closed != 0);
    if (rows) *rows = str_rows(g, R, closed != 0);
    return ACX_OK;
}

int acx_stream_geometry(int64_t window, int64_t hop, int orig_hz, int64_t max_push, int timeline, int64_t* adv, int64_t* ring,
                        int64_t* history, int64_t* rows) {
    if (timeline != 0 && timeline != 1) ACX_FAIL(ACX_ERR_ARG, "acx_stream_geometry: timeline must be 0 or 1 (got %d)", timeline);
    StrGeom g;
    ACX_TRY(str_geom(window, hop, orig_hz, &g));
    StrSizes z;
    ACX_TRY(str_sizes(g, max_push, timeline != 0, "acx_stream_geometry", &z));
    if (adv) *adv = z.adv;
    if (ring) *ring = z.C;
    if (history) *history = z.Ch;
    if (rows) *rows = z.Hw;
    return ACX_OK;
}

// the handle's rows are `classes` wide: a context finalized since with another N must not get them
static int check_classes(const acx_stream* st, const char* who) {
    if (st->ctx->num_classes != st->classes)
        ACX_FAIL(ACX_ERR_STATE, "%s: the context now has %d classes, the stream was created for %d: create a new stream", who,
                 st->ctx->num_classes, st->classes);
    return ACX_OK;
}

int acx_stream_create(acx_ctx* c, int slots, int64_t window, int64_t hop, int orig_hz, int64_t max_push, int timeline,
                      acx_stream** out) {
    if (!c || !out) ACX_FAIL(ACX_ERR_ARG, "acx_stream_create: null argument");
    *out = nullptr;
    ACX_TRY(need_ready(c));
    if (slots < 1 || slots > (1 << 20)) ACX_FAIL(ACX_ERR_ARG, "acx_stream_create: %d slots (expected 1 .. 2^20)", slots);
    if (timeline != 0 && timeline != 1) ACX_FAIL(ACX_ERR_ARG, "acx_stream_create: timeline must be 0 or 1 (got %d)", timeline);
    StrGeom g;
    ACX_TRY(str_geom(window, hop, orig_hz, &g));
    StrSizes z;
    ACX_TRY(str_sizes(g, max_push, timeline != 0, "acx_stream_create", &z));
    const bool res = orig_hz != kModelRate;
    const long long adv = z.adv, C = z.C, Ch = z.Ch, Hw = z.Hw;
    const size_t ring_b = sizeof(float) * 2 * (size_t)C * slots, hin_b = sizeof(float) * (size_t)Ch * slots;
    const size_t hist_b = sizeof(float) * (size_t)Hw * c->num_classes * slots;
    acx_stream* st = new acx_stream();
    st->ctx = c; st->device = c->device; st->slots = slots; st->timeline = timeline != 0; st->g = g;
    st->classes = c->num_classes;
    st->max_push = max_push; st->adv_max = adv; st->C = C; st->Ch = Ch; st->Hw = Hw;
    st->s.assign(slots, acx_stream::Slot{});
    if (res) {
        const int rc = acx_resampler_create(c->device, orig_hz, kModelRate, &st->rs);
        if (rc != ACX_OK) { delete st; return rc; }
    }
    hipError_t e;
    {
        DeviceGuard dg(c->device);
        e = hipMalloc(&st->ring, ring_b);
        if (e == hipSuccess && hin_b) e = hipMalloc(&st->hin, hin_b);
        if (e == hipSuccess && hist_b) e = hipMalloc(&st->hist, hist_b);
        // defined contents once (nothing reads an unwritten sample, but the memory is never left undefined)
        if (e == hipSuccess) e = hipMemset(st->ring, 0, ring_b);
        if (e == hipSuccess && hin_b) e = hipMemset(st->hin, 0, hin_b);
        if (e == hipSuccess && hist_b) e = hipMemset(st->hist, 0, hist_b);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) {
        acx_stream_destroy(st);
        ACX_FAIL(ACX_ERR_HIP, "acx_stream_create: allocating %zu bytes of stream state failed: %s", ring_b + hin_b + hist_b,
                 hipGetErrorString(e));
    }
    *out = st;
    return ACX_OK;
}

void acx_stream_destroy(acx_stream* st) {
    if (!st) return;
    {
        DeviceGuard dg(st->device);
        if (st->ring) (void)hipFree(st->ring);
        if (st->hin) (void)hipFree(st->hin);
        if (st->hist) (void)hipFree(st->hist);
    }
    if (st->rs) acx_resampler_destroy(st->rs);
    delete st;
}

int acx_test_stream_poison(acx_stream* st, int slot, void* stream) {
    if (!st) ACX_FAIL(ACX_ERR_ARG, "acx_test_stream_poison: null handle");
    if (slot < -1 || slot >= st->slots)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_stream_poison: slot %d out of range (-1, or 0 .. %d)", slot, st->slots - 1);
    const int first = slot < 0 ? 0 : slot, last = slot < 0 ? st->slots : slot + 1;
    for (int i = first; i < last; ++i) {
        const acx_stream::Slot& x = st->s[i];
        if (!x.closed && (x.in > 0 || x.out > 0))
            ACX_FAIL(ACX_ERR_STATE, "acx_test_stream_poison: slot %d has an open recording", i);
        if (st->busy(x))
            ACX_FAIL(ACX_ERR_STATE, "acx_test_stream_poison: slot %d has windows or timeline rows that are not fetched yet", i);
    }
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(st->device);
    const size_t n = (size_t)(last - first);
    ACX_HIP(hipMemsetAsync(st->ring + (size_t)first * 2 * st->C, 0xFF, sizeof(float) * 2 * (size_t)st->C * n, s));
    if (st->hin) ACX_HIP(hipMemsetAsync(st->hin + (size_t)first * st->Ch, 0xFF, sizeof(float) * (size_t)st->Ch * n, s));
    if (st->hist)
        ACX_HIP(hipMemsetAsync(st->hist + (size_t)first * st->Hw * st->classes, 0xFF,
                               sizeof(float) * (size_t)st->Hw * st->classes * n, s));
    return ACX_OK;
}

int acx_stream_push(acx_stream* st, const float* chunks, const int* slot, const int64_t* lengths, int n, void* stream) {
    if (!st || !lengths) ACX_FAIL(ACX_ERR_ARG, "acx_stream_push: null argument");
    if (n < 1 || n > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "acx_stream_push: %d chunks (expected 1 .. %d)", n, kVarMaxClips);
    ACX_TRY(check_slots(st, slot, n, "acx_stream_push"));
    long long total = 0;
    for (int k = 0; k < n; ++k) {
        if (lengths[k] < 0 || lengths[k] > st->max_push)
            ACX_FAIL(ACX_ERR_ARG, "acx_stream_push: chunk %d has %lld samples (expected 0 .. max_push = %lld)", k,
                     (long long)lengths[k], st->max_push);
        total += lengths[k];
    }
    if (total > 0 && !chunks) ACX_FAIL(ACX_ERR_ARG, "acx_stream_push: chunks is null");
    const bool res = st->rs != nullptr;
    std::vector<int> sl(n);
    std::vector<long long> in0(n), in1(n), out0(n), out1(n);
    for (int k = 0; k < n; ++k) {
        acx_stream::Slot x = st->s[slot[k]];
        if (x.closed) x = acx_stream::Slot{};             // a drained closed slot: this push starts its next recording
        sl[k] = slot[k];
        in0[k] = x.in;
        in1[k] = x.in + lengths[k];
        out0[k] = x.out;
        out1[k] = str_final(st->g, in1[k], false);
        if (out1[k] - out0[k] > st->C - st->g.W)
            ACX_FAIL(ACX_ERR_STATE, "acx_stream_push: slot %d advances by %lld samples, more than the ring holds", slot[k],
                     out1[k] - out0[k]);
    }
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(st->device);
    {
        StrAppend a{};
        a.mirror = res ? 0 : 1;
        a.cap = res ? st->Ch : st->C;
        long long off = 0, most = 0;
        for (int k = 0; k <= n; ++k) {
            if (k == n || (a.n == kStrBatch)) {
                if (a.n) {
                    const unsigned bx = (unsigned)std::min<long long>((most + 4 * kStrThreads - 1) / (4 * kStrThreads), 64);
                    launch_kernel(&stream_append_kernel, dim3(std::max(1u, bx), a.n), dim3(kStrThreads), 0, s, a, chunks,
                                  res ? st->hin : st->ring);
                    ACX_HIP(hipGetLastError());
                }
                a.n = 0;
                most = 0;
                if (k == n) break;
            }
            if (lengths[k] > 0) {
                a.slot[a.n] = slot[k];
                a.len[a.n] = (int)lengths[k];
                a.pos[a.n] = in0[k];
                a.src[a.n] = off;
                most = std::max(most, (long long)lengths[k]);
                ++a.n;
            }
            off += lengths[k];
        }
    }
    if (res) ACX_TRY(launch_stream_resample(st, sl, out0, out1, in1, s));
    for (int k = 0; k < n; ++k) {
        acx_stream::Slot& x = st->s[slot[k]];
        if (x.closed) x = acx_stream::Slot{};
        x.in = in1[k];
        x.out = out1[k];
    }
    return ACX_OK;
}

int acx_stream_close(acx_stream* st, const int* slot, int n, void* stream) {
    if (!st) ACX_FAIL(ACX_ERR_ARG, "acx_stream_close: null handle");
    if (n < 1 || n > st->slots) ACX_FAIL(ACX_ERR_ARG, "acx_stream_close: %d slots (expected 1 .. %d)", n, st->slots);
    ACX_TRY(check_slots(st, slot, n, "acx_stream_close"));
    for (int k = 0; k < n; ++k)
        if (st->s[slot[k]].closed) ACX_FAIL(ACX_ERR_STATE, "acx_stream_close: slot %d holds no open recording", slot[k]);
    std::vector<int> sl(slot, slot + n);
    std::vector<long long> in1(n), out0(n), out1(n);
    for (int k = 0; k < n; ++k) {
        const acx_stream::Slot& x = st->s[slot[k]];
        in1[k] = x.in;
        out0[k] = x.out;
        out1[k] = str_final(st->g, x.in, true);
        if (out1[k] - out0[k] > st->C - st->g.W)
            ACX_FAIL(ACX_ERR_STATE, "acx_stream_close: slot %d advances by %lld samples, more than the ring holds", slot[k],
                     out1[k] - out0[k]);
    }
    if (st->rs) {
        DeviceGuard dg(st->device);
        ACX_TRY(launch_stream_resample(st, sl, out0, out1, in1, (hipStream_t)stream));
    }
    for (int k = 0; k < n; ++k) {
        acx_stream::Slot& x = st->s[slot[k]];
        x.out = out1[k];
        x.closed = true;
    }
    return ACX_OK;
}

int acx_stream_pending(const acx_stream* st, int64_t* windows, int64_t* rows) {
    if (!st) ACX_FAIL(ACX_ERR_ARG, "acx_stream_pending: null handle");
    long long w = 0, r = 0;
    for (const acx_stream::Slot& x : st->s) {
        w += st->windows(x) - x.win_done;
        r += st->rows(x) - x.row_done;
    }
    if (windows) *windows = w;
    if (rows) *rows = r;
    return ACX_OK;
}

int acx_stream_next(const acx_stream* st, int max, int* slot_of, int64_t* start_of, int64_t* length, int* count) {
    if (!st || !count) ACX_FAIL(ACX_ERR_ARG, "acx_stream_next: null argument");
    if (max < 1 || max > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "acx_stream_next: max %d (expected 1 .. %d)", max, kVarMaxClips);
    return pending_run(st, max, slot_of, start_of, length, count);
}

int acx_stream_forward(acx_stream* st, int count, int mode, float* out0, float* out1, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (!st) ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: null handle");
    ACX_TRY(need_ready(st->ctx));
    ACX_TRY(check_classes(st, "acx_stream_forward"));
    if (!out0 || !workspace) ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: null pointer");
    if (mode < 0 || mode > 2) ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: bad mode %d", mode);
    if (mode == ACX_MODE_LOGITS && !out1) ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: logits mode needs out1 (probs)");
    if (st->timeline && mode != ACX_MODE_LOGITS)
        ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: a handle with a timeline forwards in logits mode only");
    if (count < 1 || count > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: count %d (expected 1 .. %d)", count, kVarMaxClips);
    std::vector<int> slot_of(count);
    std::vector<int64_t> start_of(count);
    int64_t L = 0;
    int got = 0;
    ACX_TRY(pending_run(st, count, slot_of.data(), start_of.data(), &L, &got));
    if (got < count)
        ACX_FAIL(ACX_ERR_ARG, "acx_stream_forward: %d windows asked, %d pending of one length (acx_stream_next)", count, got);
    size_t need = 0;
    ACX_TRY(acx_workspace_bytes_windows(st->ctx, count, L, mode, &need));
    ACX_TRY(check_workspace(workspace, workspace_bytes, need));
    ACX_TRY(check_uniform_plans(st->ctx, count, L, mode, nullptr, false));        // (before the table launches below)
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(st->device);
    long long* wstart = (long long*)workspace;
    // on the caller's stream, before forward_uniform records its fork event
    for (int b0 = 0; b0 < count; b0 += kStrTable) {
        StrTable t{};
        t.n = std::min(kStrTable, count - b0);
        for (int b = 0; b < t.n; ++b)
            t.off[b] = (long long)slot_of[b0 + b] * 2 * st->C + start_of[b0 + b] % st->C;
        launch_kernel(&stream_table_kernel, dim3(1), dim3(kStrTable), 0, s, t, wstart + b0);
        ACX_HIP(hipGetLastError());
    }
    const size_t head = align_up((size_t)count * 8);
    ACX_TRY(forward_uniform(st->ctx, st->ring, count, L, mode, out0, out1, (char*)workspace + head, s, wstart, nullptr, nullptr, true));
    if (st->timeline) {
        // window j of slot i -> history row i Hw + j mod Hw; slot i's windows are listed in order from its win_done on
        std::vector<long long> next(st->slots, -1), row(count);
        for (int k = 0; k < count; ++k) {
            const int i = slot_of[k];
            if (next[i] < 0) next[i] = st->s[i].win_done;
            row[k] = (long long)i * st->Hw + next[i] % st->Hw;
            next[i] += 1;
        }
        for (int b0 = 0; b0 < count; b0 += kStrTable) {
            StrStash a{};
            a.n = std::min(kStrTable, count - b0);
            for (int k = 0; k < a.n; ++k) a.row[k] = row[b0 + k];
            launch_kernel(&stream_stash_kernel, dim3(a.n), dim3(kStrThreads), 0, s, a,
                          (const float*)(out1 + (size_t)b0 * st->classes), st->classes, st->hist);
            ACX_HIP(hipGetLastError());
        }
    }
    for (int k = 0; k < count; ++k) st->s[slot_of[k]].win_done += 1;
    return ACX_OK;
}

int acx_stream_timeline(acx_stream* st, int reduce, int64_t max_rows, float* out, int* slot_of, int64_t* step_of,
                        int64_t* n_rows, void* stream) {
    if (!st || !n_rows) ACX_FAIL(ACX_ERR_ARG, "acx_stream_timeline: null argument");
    *n_rows = 0;
    if (!st->timeline) ACX_FAIL(ACX_ERR_STATE, "acx_stream_timeline: the handle was created without a timeline");
    ACX_TRY(check_classes(st, "acx_stream_timeline"));
    if (reduce != 0 && reduce != 1) ACX_FAIL(ACX_ERR_ARG, "acx_stream_timeline: bad reduce %d (0 mean, 1 max)", reduce);
    if (max_rows < 0) ACX_FAIL(ACX_ERR_ARG, "acx_stream_timeline: max_rows %lld", (long long)max_rows);
    long long want = 0;
    for (int i = 0; i < st->slots; ++i) {
        const acx_stream::Slot& x = st->s[i];
        const long long r = st->rows(x) - x.row_done;
        if (r > 0 && x.win_done < st->windows(x))
            ACX_FAIL(ACX_ERR_STATE, "acx_stream_timeline: slot %d has windows that are not forwarded yet", i);
        want += r;
    }
    want = std::min(want, (long long)max_rows);
    if (want == 0) return ACX_OK;
    if (!out || !slot_of || !step_of) ACX_FAIL(ACX_ERR_ARG, "acx_stream_timeline: null output");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(st->device);
    StrRows a{};
    a.W = st->g.W; a.H = st->g.H; a.Hw = st->Hw;
    long long done = 0, base = 0, in_launch = 0;
    auto flush = [&]() -> int {
        if (a.n == 0) return ACX_OK;
        launch_kernel(&stream_timeline_kernel, dim3((unsigned)std::min(in_launch, 4096LL)), dim3(kStrThreads), 0, s, a,
                      (const float*)st->hist, st->classes, reduce, out + (size_t)base * st->classes);
        ACX_HIP(hipGetLastError());
        base += in_launch;
        in_launch = 0;
        a.n = 0;
        return ACX_OK;
    };
    for (int i = 0; i < st->slots && done < want; ++i) {
        acx_stream::Slot& x = st->s[i];
        const long long r = std::min(st->rows(x) - x.row_done, want - done);
        if (r <= 0) continue;
        for (long long k = 0; k < r; ++k) {
            slot_of[done + k] = i;
            step_of[done + k] = x.row_done + k;
        }
        a.slot[a.n] = i;
        a.rows[a.n] = (int)r;
        a.k0[a.n] = x.row_done;
        a.L[a.n] = x.closed ? x.out : kStrOpen;
        ++a.n;
        in_launch += r;
        done += r;
        x.row_done += r;
        if (a.n == kStrBatch) ACX_TRY(flush());
    }
    ACX_TRY(flush());
    *n_rows = done;
    return ACX_OK;
}

}  // extern "C"
