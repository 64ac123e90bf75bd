// Band-limited resampling of input clips to the model rate (acx_resample*, include/acx.h): the interpolation of
// torchaudio.functional.resample with its defaults (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), which the
// reference's demo applies on the host (demo_convnext.py:53-59).  torchaudio evaluates it as a dense polyphase conv1d of
// 2 * width + of taps per output (459 at 44.1 kHz); all but the ~17 taps inside the window's support |t| < 6 are zero,
// and only those are stored and applied here.
//
// Output n = j * nf + i of a clip is the fp32 FMA chain, in ascending k, over phase i's band:
//     y[n] = sum_{r < count_i} h_i[start_i + r] * x[j * of + start_i + r - width]      (x = 0 outside the clip)
// The chain depends on (i, band) and the clip's own samples only: a clip's bits are the same alone or packed among others.
#include <cmath>
#include <numeric>
#include <vector>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kResMaxRate = 768000;
constexpr long long kResMaxTable = 1LL << 22;           // nf * max_band floats
constexpr size_t kResMaxLds = 56 * 1024;                // the staged input span (the prefix tables take 6 KiB more)
constexpr int kResMaxGrid = 4096;                       // workgroups per launch; each walks tiles t, t + grid, ...

struct ResPlan {
    int of, nf, width, max_band, per_thread;
    double base;
    size_t lds_bytes;
    std::vector<int> start, count;                       // per phase, start in tap coordinates k = 0 .. 2 * width + of - 1
};

// t of tap k of phase i, exactly as utils/resample.py forms it (in float64 here)
static inline double res_t(const ResPlan& p, int i, long long k) {
    return (-(double)i / p.nf + (double)(k - p.width) / p.of) * p.base;
}

static int res_plan(int orig, int target, ResPlan* p) {
    if (orig < 1 || orig > kResMaxRate || target < 1 || target > kResMaxRate)
        ACX_FAIL(ACX_ERR_ARG, "resample: sample rates must be integers in [1, %d] (got %d -> %d)", kResMaxRate, orig, target);
    const int g = std::gcd(orig, target);
    p->of = orig / g;
    p->nf = target / g;
    p->base = std::min(p->of, p->nf) * 0.99;
    p->width = (int)std::ceil(6.0 * p->of / p->base);
    // |t| < 6  <=>  |k - width - i * of / nf| < 6 * of / base: a contiguous band; find its ends near the centre
    const double R = 6.0 * p->of / p->base;
    const long long kmax = 2LL * p->width + p->of;        // dense kernel length
    p->start.assign(p->nf, 0);
    p->count.assign(p->nf, 0);
    long long mb = 0;
    for (int i = 0; i < p->nf; ++i) {
        const double centre = p->width + (double)i * p->of / p->nf;
        long long a = std::max(0LL, (long long)std::floor(centre - R) - 2);
        long long b = std::min(kmax - 1, (long long)std::ceil(centre + R) + 2);
        while (a <= b && !(std::fabs(res_t(*p, i, a)) < 6.0)) ++a;
        while (b >= a && !(std::fabs(res_t(*p, i, b)) < 6.0)) --b;
        p->start[i] = (int)a;
        p->count[i] = (int)(b - a + 1);
        mb = std::max(mb, b - a + 1);
        // the kernel indexes its staged span from floor(n * of / nf) - width - 1 (resample_kernel): every band lies inside
        const long long c = (long long)i * p->of / p->nf;
        if (p->count[i] > 0 && (a - p->width < c - p->width - 1 || b + 1 - p->width > c + p->width + 2))
            ACX_FAIL(ACX_ERR_UNSUPPORTED, "resample: band of phase %d of ratio %d/%d leaves the staged span", i, p->of, p->nf);
    }
    p->max_band = (int)mb;
    if ((long long)p->nf * mb > kResMaxTable)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "resample: ratio of/nf = %d/%d (%d -> %d Hz) needs %lld taps (%d phases x %lld); at most "
                 "%lld are supported", p->of, p->nf, orig, target, (long long)p->nf * mb, p->nf, mb, kResMaxTable);
    // outputs per workgroup: 4, 2 or 1 per thread, whichever lets the input span fit the LDS budget
    p->per_thread = 0;
    for (int q = 4; q >= 1; q /= 2) {
        const long long T = (long long)kResThreads * q;
        const long long span = (T - 1) * p->of / p->nf + 2LL * p->width + 4;
        if (span * 4 <= (long long)kResMaxLds) { p->per_thread = q; p->lds_bytes = (size_t)span * 4; break; }
    }
    if (!p->per_thread)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "resample: ratio of/nf = %d/%d (%d -> %d Hz): the input span of %d outputs exceeds "
                 "%zu bytes of LDS", p->of, p->nf, orig, target, kResThreads, kResMaxLds);
    return ACX_OK;
}

// h_i[k] = (base / of) * sinc(t) * cos^2(pi t / 12), float64, rounded to fp32 once
static float res_tap(const ResPlan& p, int i, long long k) {
    const double t = res_t(p, i, k);
    const double pt = M_PI * t;
    const double s = t == 0.0 ? 1.0 : std::sin(pt) / pt;
    const double w = std::cos(pt / 12.0);
    return (float)((p.base / p.of) * s * (w * w));
}

static long long res_out_len(const ResPlan& p, long long L) { return (p.nf * L + p.of - 1) / p.of; }

// One workgroup per tile of 256 * per_thread consecutive outputs of one clip (grid-strided over every tile of the call), each
// formed by res_tile from the clip's own samples.  Offsets of clips and tiles are prefix sums over the lengths passed by value.
__global__ __launch_bounds__(kResThreads) void resample_kernel(PackedLens a, ResGeom g, const float* __restrict__ in,
                                                              float* __restrict__ out, const int2* __restrict__ band,
                                                              const float* __restrict__ taps) {
    extern __shared__ float s_in[];
    __shared__ long long s_soff[kVarMaxClips + 1], s_ooff[kVarMaxClips + 1], s_toff[kVarMaxClips + 1];
    const int tid = threadIdx.x, B = a.n;
    const int T = kResThreads * g.per_thread;
    {   // inclusive scan of (samples, outputs, tiles) per clip; slot c + 1 ends clip c.  Every workgroup of a large launch runs
        // this prologue, so it stays a parallel scan where the other packed calls take packed_prefix
        long long L = 0, N = 0, nt = 0;
        if (tid < B) {
            L = a.len[tid];
            N = ((long long)g.nf * L + g.of - 1) / g.of;
            nt = (N + T - 1) / T;
        }
        if (tid == 0) { s_soff[0] = 0; s_ooff[0] = 0; s_toff[0] = 0; }
        s_soff[tid + 1] = L; s_ooff[tid + 1] = N; s_toff[tid + 1] = nt;
        __syncthreads();
        for (int d = 1; d < kVarMaxClips; d *= 2) {
            long long v0 = 0, v1 = 0, v2 = 0;
            if (tid >= d) { v0 = s_soff[tid + 1 - d]; v1 = s_ooff[tid + 1 - d]; v2 = s_toff[tid + 1 - d]; }
            __syncthreads();
            s_soff[tid + 1] += v0; s_ooff[tid + 1] += v1; s_toff[tid + 1] += v2;
            __syncthreads();
        }
    }
    const long long tiles = s_toff[B];
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int c = packed_find(s_toff, B, t);         // the clip whose tiles hold t
        const long long L = a.len[c];
        const long long N = s_ooff[c + 1] - s_ooff[c];
        const long long nb = (t - s_toff[c]) * T;
        const float* x = in + s_soff[c];
        float* y = out + s_ooff[c] + nb;
        res_tile(g, nb, (int)min((long long)T, N - nb), s_in, band, taps,
                 [x, L](long long m) { return (m >= 0 && m < L) ? x[m] : 0.0f; }, [y](int d, float v) { y[d] = v; });
    }
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_resample_geometry(int orig_hz, int new_hz, int* of, int* nf, int* width, int* max_band) {
    ResPlan p;
    ACX_TRY(res_plan(orig_hz, new_hz, &p));
    if (of) *of = p.of;
    if (nf) *nf = p.nf;
    if (width) *width = p.width;
    if (max_band) *max_band = p.max_band;
    return ACX_OK;
}

int acx_resample_taps(int orig_hz, int new_hz, int* band_start, int* band_count, float* taps, size_t n_taps) {
    ResPlan p;
    ACX_TRY(res_plan(orig_hz, new_hz, &p));
    size_t total = 0;
    for (int i = 0; i < p.nf; ++i) total += (size_t)p.count[i];
    if (taps && n_taps < total)
        ACX_FAIL(ACX_ERR_ARG, "acx_resample_taps: %zu taps do not fit a buffer of %zu", total, n_taps);
    size_t o = 0;
    for (int i = 0; i < p.nf; ++i) {
        if (band_start) band_start[i] = p.start[i];
        if (band_count) band_count[i] = p.count[i];
        if (taps)
            for (int r = 0; r < p.count[i]; ++r) taps[o + r] = res_tap(p, i, (long long)p.start[i] + r);
        o += (size_t)p.count[i];
    }
    return ACX_OK;
}

int acx_resampled_length(int orig_hz, int new_hz, int64_t L, int64_t* out) {
    if (!out || L < 0) ACX_FAIL(ACX_ERR_ARG, "acx_resampled_length: bad argument");
    if (orig_hz < 1 || orig_hz > kResMaxRate || new_hz < 1 || new_hz > kResMaxRate)
        ACX_FAIL(ACX_ERR_ARG, "resample: sample rates must be integers in [1, %d] (got %d -> %d)", kResMaxRate, orig_hz, new_hz);
    if (L > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "acx_resampled_length: clip of %lld samples is longer than 2^31 - 1", (long long)L);
    const int g = std::gcd(orig_hz, new_hz);
    const long long of = orig_hz / g, nf = new_hz / g;
    *out = (nf * L + of - 1) / of;
    return ACX_OK;
}

int acx_resampler_create(int hip_device, int orig_hz, int new_hz, acx_resampler** out) {
    if (!out) ACX_FAIL(ACX_ERR_ARG, "acx_resampler_create: out is null");
    ResPlan p;
    ACX_TRY(res_plan(orig_hz, new_hz, &p));
    int n = 0;
    ACX_HIP(hipGetDeviceCount(&n));
    if (hip_device < 0 || hip_device >= n)
        ACX_FAIL(ACX_ERR_ARG, "acx_resampler_create: device %d out of range (%d visible)", hip_device, n);
    std::vector<int2> band(p.nf);
    std::vector<float> taps((size_t)p.max_band * p.nf, 0.0f);
    for (int i = 0; i < p.nf; ++i) {
        band[i] = make_int2(p.start[i] - p.width, p.count[i]);
        for (int r = 0; r < p.count[i]; ++r) taps[(size_t)r * p.nf + i] = res_tap(p, i, (long long)p.start[i] + r);
    }
    int prev = 0;
    ACX_HIP(hipGetDevice(&prev));
    ACX_HIP(hipSetDevice(hip_device));
    acx_resampler* rs = new acx_resampler();
    *rs = acx_resampler{hip_device, orig_hz, new_hz, p.of, p.nf, p.width, p.max_band, p.per_thread, p.lds_bytes, nullptr, nullptr};
    hipError_t e = hipMalloc(&rs->band, sizeof(int2) * p.nf);
    if (e == hipSuccess) e = hipMalloc(&rs->taps, sizeof(float) * std::max<size_t>(1, taps.size()));
    if (e == hipSuccess) e = hipMemcpy(rs->band, band.data(), sizeof(int2) * p.nf, hipMemcpyHostToDevice);
    if (e == hipSuccess && !taps.empty()) e = hipMemcpy(rs->taps, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        acx_resampler_destroy(rs);
        ACX_FAIL(ACX_ERR_HIP, "acx_resampler_create: uploading the tables failed: %s", hipGetErrorString(e));
    }
    *out = rs;
    return ACX_OK;
}

void acx_resampler_destroy(acx_resampler* rs) {
    if (!rs) return;
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    (void)hipSetDevice(rs->device);
    if (rs->band) (void)hipFree(rs->band);
    if (rs->taps) (void)hipFree(rs->taps);
    if (have_prev) (void)hipSetDevice(prev);
    delete rs;
}

// acx_resample; max_blocks caps the grid (acx_test_resample: a workgroup then walks many tiles of a small call)
static int res_launch(const acx_resampler* rs, const float* in, const int64_t* lengths, int B, float* out, void* stream,
                      int max_blocks = kResMaxGrid) {
    if (!rs || !lengths || !out) ACX_FAIL(ACX_ERR_ARG, "acx_resample: null argument");
    if (max_blocks < 1 || max_blocks > kResMaxGrid)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_resample: max_blocks = %d (expected 1 .. %d)", max_blocks, kResMaxGrid);
    if (B <= 0 || B > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "acx_resample: %d clips (expected 1 .. %d)", B, kVarMaxClips);
    long long tiles = 0, samples = 0;
    const long long T = (long long)kResThreads * rs->per_thread;
    ResPlan p;
    p.of = rs->of;
    p.nf = rs->nf;
    for (int i = 0; i < B; ++i) {
        if (lengths[i] < 0 || lengths[i] > 0x7fffffffLL)
            ACX_FAIL(ACX_ERR_SHAPE, "acx_resample: clip %d has %lld samples (expected 0 .. 2^31 - 1)", i, (long long)lengths[i]);
        samples += lengths[i];
        tiles += (res_out_len(p, lengths[i]) + T - 1) / T;
    }
    if (samples > 0 && !in) ACX_FAIL(ACX_ERR_ARG, "acx_resample: in is null");
    if (tiles == 0) return ACX_OK;
    const ResGeom g{rs->of, rs->nf, rs->width, rs->per_thread};
    const unsigned grid = (unsigned)std::min(tiles, (long long)max_blocks);
    launch_kernel(&resample_kernel, dim3(grid), dim3(kResThreads), rs->lds_bytes, (hipStream_t)stream, packed_lens(lengths, B), g,
                  in, out, (const int2*)rs->band, (const float*)rs->taps);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_resample(const acx_resampler* rs, const float* in, const int64_t* lengths, int B, float* out, void* stream) {
    return res_launch(rs, in, lengths, B, out, stream);
}

int acx_test_resample(const acx_resampler* rs, const float* in, const int64_t* lengths, int B, float* out, int max_blocks,
                      void* stream) {
    return res_launch(rs, in, lengths, B, out, stream, max_blocks);
}

int acx_test_resample_plan(int orig_hz, int new_hz, acx_resample_plan_t* plan) {
    if (!plan) ACX_FAIL(ACX_ERR_ARG, "acx_test_resample_plan: plan is null");
    ResPlan p;
    ACX_TRY(res_plan(orig_hz, new_hz, &p));
    *plan = acx_resample_plan_t{p.of, p.nf, p.width, p.max_band, p.per_thread, (int32_t)p.lds_bytes, kResThreads * p.per_thread,
                                kResMaxGrid};
    return ACX_OK;
}

}  // extern "C"
