// The reference's training-mode input transforms as two bandwidth kernels, and the augmented forward that chains them with the
// frontend and the trunk (acx_augment_wave, acx_augment_spec, acx_forward_augmented; include/acx.h).  The definitions are the
// host functions of pytorch/augment.py (augment_wave_host, augment_spec_host); the kernels equal them bit for bit.
//
// Waveform (pydub_augment, roll_augment, SpeedPerturbation with nearest interpolation; augmentations.py:266-351): gain, roll,
// stretch and pad / crop compose into one gather per output sample,
//     out[i] = gain * in[(src(i + shift) - roll) mod L]    if 0 <= i + shift < n_out, else +0,
//     src(j) = min(L - 1, rint(j * step))                  in float64, ties to even.
// Log-mel (SpecAugmentation, do_mixup; convnext.py:308-313): stripes of frames and of mel bins become +0.0, then rows 2b and
// 2b + 1 mix as fl(a * l0) + fl(b * l1).
#include <cmath>

#include "acx_internal.h"

namespace acx {

constexpr int kAugWaveThreads = 256;
constexpr int kAugWaveVecPerThread = 4;             // float4 stores per thread: 4096 samples per workgroup
constexpr int kAugRowF4 = kMels / 4;                // 56 float4 per log-mel row
constexpr int kAugMixRows = 8;                      // rows per workgroup of the mixing form
constexpr int kAugMixThreads = kAugMixRows * kAugRowF4;    // 448 = 7 waves: a thread keeps one float4 column for all its rows
constexpr int kAugMaskThreads = 256;

// one output sample of clip `x` (L samples) under plan entry p
__device__ __forceinline__ float aug_wave_sample(const float* __restrict__ x, long long L, const acx_wave_aug& p, long long i) {
    const long long j = i + p.shift;
    if (j < 0 || j >= p.n_out) return 0.0f;
    // the position is formed in float64, one rounded product and a round-half-even, as the host definition forms it: a float32
    // shortcut misses it by one sample at long clips
    long long src = (long long)rint(__dmul_rn((double)j, p.step));
    src = src < L - 1 ? src : L - 1;
    src = src > 0 ? src : 0;                         // (a plan that skipped acx_augment_plan_check still reads inside the clip)
    long long k = src - p.roll;                      // 0 <= roll < L
    if (k < 0) k += L;
    return __fmul_rn(p.gain, x[k]);
}

// grid (tiles, B): workgroup (t, b) writes samples [t * 4096, (t + 1) * 4096) of clip b's output row, counted from the row's first
// 16-byte aligned sample; the samples in front of it (rows of an L that is no multiple of 4 start unaligned) and the tail behind
// the last whole float4 are scalar stores.  The plan entry is uniform over the workgroup (scalar loads).
__global__ __launch_bounds__(kAugWaveThreads) void augment_wave_kernel(const float* __restrict__ in, long long L,
                                                                       const acx_wave_aug* __restrict__ plan,
                                                                       float* __restrict__ out) {
    const int b = blockIdx.y;
    acx_wave_aug p = plan[b];
    p.roll = ((p.roll % L) + L) % L;                 // a checked plan has it in range already
    const float* x = in + (long long)b * L;
    float* y = out + (long long)b * L;
    long long head = (4 - (long long)((reinterpret_cast<uintptr_t>(y) >> 2) & 3)) & 3;
    if (head > L) head = L;
    if (blockIdx.x == 0 && threadIdx.x < head) y[threadIdx.x] = aug_wave_sample(x, L, p, threadIdx.x);
    const long long nvec = (L - head) / 4;
    const long long v0 = (long long)blockIdx.x * (kAugWaveThreads * kAugWaveVecPerThread) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kAugWaveVecPerThread; ++u) {
        const long long v = v0 + (long long)u * kAugWaveThreads;
        if (v < nvec) {
            const long long i = head + 4 * v;
            float4 r;
            r.x = aug_wave_sample(x, L, p, i);
            r.y = aug_wave_sample(x, L, p, i + 1);
            r.z = aug_wave_sample(x, L, p, i + 2);
            r.w = aug_wave_sample(x, L, p, i + 3);
            *reinterpret_cast<float4*>(y + i) = r;
        }
    }
    const long long tail0 = head + 4 * nvec;
    if (blockIdx.x == gridDim.x - 1 && tail0 + threadIdx.x < L) y[tail0 + threadIdx.x] = aug_wave_sample(x, L, p, tail0 + threadIdx.x);
}

__device__ __forceinline__ bool aug_in_stripe(const int32_t* bgn, const int32_t* len, int v) {
    bool m = false;
#pragma unroll
    for (int s = 0; s < ACX_AUG_MAX_STRIPES; ++s) m = m || (v >= bgn[s] && v < bgn[s] + len[s]);
    return m;
}

// In place, no lambdas: grid (G, B); only the masked elements of clip b are written.  Time stripes: whole rows, as float4 stores;
// frequency stripes: at most 27 bins per row, scalar stores.  Stripes may overlap (the same +0.0 is stored twice).
__global__ __launch_bounds__(kAugMaskThreads) void augment_spec_mask_kernel(float* __restrict__ feat, int T,
                                                                            const acx_spec_aug* __restrict__ plan) {
    const int b = blockIdx.y;
    const acx_spec_aug p = plan[b];
    float* f = feat + (long long)b * T * kMels;
    const int stride = gridDim.x * kAugMaskThreads;
    const int first = blockIdx.x * kAugMaskThreads + threadIdx.x;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < ACX_AUG_MAX_STRIPES; ++s) {
        // (clamped to the map, here and below: a checked plan is inside it already)
        const int t0 = max(p.t_bgn[s], 0), t1 = min(p.t_bgn[s] + p.t_len[s], T);
        const int n = (t1 - t0) * kAugRowF4;
        float4* rows = reinterpret_cast<float4*>(f + (long long)t0 * kMels);
        for (int i = first; i < n; i += stride) rows[i] = z;
    }
#pragma unroll
    for (int s = 0; s < ACX_AUG_MAX_STRIPES; ++s) {
        const int f0 = max(p.f_bgn[s], 0), len = min(p.f_bgn[s] + p.f_len[s], kMels) - f0;
        if (len <= 0) continue;
        const int n = T * len;
        for (int i = first; i < n; i += stride) {
            const int t = i / len;
            f[(long long)t * kMels + f0 + (i - t * len)] = 0.0f;
        }
    }
}

// With lambdas: grid (G, B / 2); output clip b = mask(in[2b]) * lam[2b] + mask(in[2b + 1]) * lam[2b + 1], two rounded products and
// one rounded sum (__fmul_rn / __fadd_rn: no contraction into an FMA).  plan == null: no masks.  A thread owns one float4 column
// of the row, so its frequency masks are formed once.
__global__ __launch_bounds__(kAugMixThreads) void augment_spec_mix_kernel(const float* __restrict__ feat, int T,
                                                                          const acx_spec_aug* __restrict__ plan,
                                                                          const float* __restrict__ lam, float* __restrict__ out) {
    const int b = blockIdx.y;
    acx_spec_aug pa = {}, pb = {};
    if (plan) { pa = plan[2 * b]; pb = plan[2 * b + 1]; }
    const float l0 = lam[2 * b], l1 = lam[2 * b + 1];
    const float4* A = reinterpret_cast<const float4*>(feat + (long long)(2 * b) * T * kMels);
    const float4* Bm = reinterpret_cast<const float4*>(feat + (long long)(2 * b + 1) * T * kMels);
    float4* O = reinterpret_cast<float4*>(out + (long long)b * T * kMels);
    const int col = threadIdx.x % kAugRowF4, r0 = threadIdx.x / kAugRowF4;
    bool fa[4], fb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        fa[e] = aug_in_stripe(pa.f_bgn, pa.f_len, 4 * col + e);
        fb[e] = aug_in_stripe(pb.f_bgn, pb.f_len, 4 * col + e);
    }
    for (int t = blockIdx.x * kAugMixRows + r0; t < T; t += gridDim.x * kAugMixRows) {
        const bool ta = aug_in_stripe(pa.t_bgn, pa.t_len, t), tb = aug_in_stripe(pb.t_bgn, pb.t_len, t);
        const float4 a = A[(long long)t * kAugRowF4 + col], c = Bm[(long long)t * kAugRowF4 + col];
        float4 o;
        o.x = __fadd_rn(__fmul_rn((ta || fa[0]) ? 0.0f : a.x, l0), __fmul_rn((tb || fb[0]) ? 0.0f : c.x, l1));
        o.y = __fadd_rn(__fmul_rn((ta || fa[1]) ? 0.0f : a.y, l0), __fmul_rn((tb || fb[1]) ? 0.0f : c.y, l1));
        o.z = __fadd_rn(__fmul_rn((ta || fa[2]) ? 0.0f : a.z, l0), __fmul_rn((tb || fb[2]) ? 0.0f : c.z, l1));
        o.w = __fadd_rn(__fmul_rn((ta || fa[3]) ? 0.0f : a.w, l0), __fmul_rn((tb || fb[3]) ? 0.0f : c.w, l1));
        O[(long long)t * kAugRowF4 + col] = o;
    }
}

static int launch_augment_wave(const float* wav, int B, int64_t L, const acx_wave_aug* plan, float* out, hipStream_t st) {
    const long long per_block = (long long)kAugWaveThreads * kAugWaveVecPerThread * 4;
    const unsigned tiles = (unsigned)((L + per_block - 1) / per_block);
    launch_kernel(&augment_wave_kernel, dim3(tiles, (unsigned)B), dim3(kAugWaveThreads), 0, st, wav, (long long)L, plan, out);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

static int launch_augment_spec(const float* feat, int B, int T, const acx_spec_aug* plan, const float* lam, float* out,
                               hipStream_t st) {
    if (lam) {
        const unsigned g = (unsigned)std::min((T + kAugMixRows - 1) / kAugMixRows, 256);
        launch_kernel(&augment_spec_mix_kernel, dim3(g, (unsigned)(B / 2)), dim3(kAugMixThreads), 0, st, feat, T, plan, lam, out);
    } else {
        // at most 4 x 63 rows x 56 float4 and 4 x 27 x T scalars per clip
        const unsigned g = (unsigned)std::min((T + 63) / 64 + 1, 64);
        launch_kernel(&augment_spec_mask_kernel, dim3(g, (unsigned)B), dim3(kAugMaskThreads), 0, st, out, T, plan);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

static int check_aug_shape(const char* who, int B, int64_t L) {
    if (B <= 0 || B > 65535) ACX_FAIL(ACX_ERR_ARG, "%s: %d clips (expected 1 .. 65535)", who, B);
    if (L < 1 || L > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "%s: clips of %lld samples (expected 1 .. 2^31 - 1)", who, (long long)L);
    return ACX_OK;
}

// (AugWs: acx_internal.h.  The frames and the spectrum own regions here, sized by the tenants' own definitions.)
int carve_augmented(bool dense, int B, int64_t L, bool wave, bool lam, int mode, AugWs* w) {
    const size_t T = (size_t)(L / kHop + 1);
    size_t off = 0;
    w->wave = off; if (wave) off += align_up((size_t)B * L * 4);
    w->feat = off; off += align_up((size_t)B * T * kMels * 4);
    w->mix = off; if (lam) off += align_up((size_t)(B / 2) * T * kMels * 4);
    w->frames = off; if (dense) off += align_up(need_dense_frames((size_t)B * T));
    w->spec = off; if (dense) off += align_up(need_dense_spec((size_t)B * T));
    size_t fwd = 0;
    ACX_TRY(acx_workspace_bytes(nullptr, lam ? B / 2 : B, L, mode, &fwd));       // (it reads no context)
    w->fwd = off;
    w->total = off + fwd;
    return ACX_OK;
}

// What acx_forward_augmented puts in front of the nested forward, as data: its five regions (wave, feat, mix, frames, spectrum) and
// the two tenants of its own frontend.  The driver takes the frames and spectrum pointers from here, acx_test_forward_plan reports it.
void augmented_front(const AugWs& w, bool dense, size_t frames, AugFront* f) {
    const size_t cut[6] = {w.wave, w.feat, w.mix, w.frames, w.spec, w.fwd};
    for (int i = 0; i < 5; ++i) f->regions[i] = acx_plan_region_t{cut[i], cut[i + 1] - cut[i]};
    f->n_tenants = 0;
    if (!dense) return;
    const uint32_t ops = (1u << ACX_PLAN_AUG_WAVE) | (1u << ACX_PLAN_AUG_FEAT);
    f->tenants[f->n_tenants++] = acx_plan_tenant_t{ACX_PLAN_DENSE_FRAMES, ACX_PLAN_AUG_FRAMES, ACX_PLAN_PHASE_FRONTEND, -1, -1, ops, 0,
                                                   need_dense_frames(frames)};
    f->tenants[f->n_tenants++] = acx_plan_tenant_t{ACX_PLAN_DENSE_SPEC, ACX_PLAN_AUG_SPEC, ACX_PLAN_PHASE_FRONTEND, -1, -1, ops, 0,
                                                   need_dense_spec(frames)};
}

static int check_augmented_shape(const char* who, int B, int64_t L, bool lam, int mode) {
    if (mode < 0 || mode > 2) ACX_FAIL(ACX_ERR_ARG, "%s: bad mode %d", who, mode);
    ACX_TRY(check_aug_shape(who, B, L));
    if (lam && (B & 1)) ACX_FAIL(ACX_ERR_ARG, "%s: mixup pairs clips 2b and 2b + 1: the batch must be even (got %d)", who, B);
    if (L < ACX_MIN_SAMPLES)
        ACX_FAIL(ACX_ERR_SHAPE, "%s: clip of %lld samples is too short: the last 2x2 downsample needs at least %d samples", who,
                 (long long)L, ACX_MIN_SAMPLES);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_augment_plan_check(int B, int64_t L, const acx_wave_aug* wave, const acx_spec_aug* spec) {
    ACX_TRY(check_aug_shape("acx_augment_plan_check", B, L));
    const int T = (int)(L / kHop + 1);
    for (int b = 0; wave && b < B; ++b) {
        const acx_wave_aug& p = wave[b];
        if (!(p.step > 0.0) || !std::isfinite(p.step) || !std::isfinite(p.gain))
            ACX_FAIL(ACX_ERR_ARG, "augment plan: clip %d has step %g and gain %g (expected a positive finite step, a finite gain)", b,
                     p.step, (double)p.gain);
        if (p.roll < 0 || p.roll >= L)
            ACX_FAIL(ACX_ERR_ARG, "augment plan: clip %d has roll %lld (expected 0 <= roll < L = %lld)", b, (long long)p.roll,
                     (long long)L);
        const double n = std::ceil((double)L / p.step);
        if (!(n >= 1.0 && n <= 2147483647.0) || p.n_out != (int64_t)n)
            ACX_FAIL(ACX_ERR_ARG, "augment plan: clip %d has n_out %lld (expected ceil(L / step) = %.0f, in 1 .. 2^31 - 1)", b,
                     (long long)p.n_out, n);
        const int64_t lo = p.n_out < L ? p.n_out - L : 0, hi = p.n_out > L ? p.n_out - L : 0;
        if (p.shift < lo || p.shift > hi)
            ACX_FAIL(ACX_ERR_ARG, "augment plan: clip %d has shift %lld (expected %lld .. %lld: the crop start or minus the left pad)",
                     b, (long long)p.shift, (long long)lo, (long long)hi);
    }
    for (int b = 0; spec && b < B; ++b) {
        const acx_spec_aug& p = spec[b];
        for (int s = 0; s < ACX_AUG_MAX_STRIPES; ++s) {
            if (p.t_bgn[s] < 0 || p.t_len[s] < 0 || (int64_t)p.t_bgn[s] + p.t_len[s] > T)
                ACX_FAIL(ACX_ERR_ARG, "augment plan: time stripe %d of clip %d, frames [%d, %d + %d), leaves the clip's T = %d frames", s,
                         b, p.t_bgn[s], p.t_bgn[s], p.t_len[s], T);
            if (p.f_bgn[s] < 0 || p.f_len[s] < 0 || (int64_t)p.f_bgn[s] + p.f_len[s] > kMels)
                ACX_FAIL(ACX_ERR_ARG, "augment plan: frequency stripe %d of clip %d, bins [%d, %d + %d), leaves the %d mel bins", s, b,
                         p.f_bgn[s], p.f_bgn[s], p.f_len[s], kMels);
        }
    }
    return ACX_OK;
}

int acx_augment_wave(const float* wav, int B, int64_t L, const acx_wave_aug* plan, float* out, void* stream) {
    if (!wav || !plan || !out) ACX_FAIL(ACX_ERR_ARG, "acx_augment_wave: null pointer");
    ACX_TRY(check_aug_shape("acx_augment_wave", B, L));
    if (wav == out) ACX_FAIL(ACX_ERR_ARG, "acx_augment_wave: out must not be wav (the kernel gathers)");
    return launch_augment_wave(wav, B, L, plan, out, (hipStream_t)stream);
}

int acx_augment_spec(float* feat, int B, int T, const acx_spec_aug* plan, const float* lambda, float* out, void* stream) {
    if (!feat || !out || (!plan && !lambda)) ACX_FAIL(ACX_ERR_ARG, "acx_augment_spec: null pointer");
    if (B <= 0 || B > 65535 || T <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_augment_spec: %d clips of %d frames", B, T);
    if (((uintptr_t)feat | (uintptr_t)out) & 15) ACX_FAIL(ACX_ERR_ARG, "acx_augment_spec: feat and out must be 16-byte aligned");
    if (lambda && (B & 1))
        ACX_FAIL(ACX_ERR_ARG, "acx_augment_spec: mixup pairs clips 2b and 2b + 1: the batch must be even (got %d)", B);
    if (lambda && out == feat) ACX_FAIL(ACX_ERR_ARG, "acx_augment_spec: with lambdas out must not be feat");
    if (!lambda && out != feat) ACX_FAIL(ACX_ERR_ARG, "acx_augment_spec: without lambdas the masks are written in place (out == feat)");
    return launch_augment_spec(feat, B, T, plan, lambda, out, (hipStream_t)stream);
}

int acx_workspace_bytes_augmented(const acx_ctx* c, int B, int64_t L, int has_wave_plan, int has_lambda, int mode,
                                  size_t* out_bytes) {
    // (the shapes first: they need no context)
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_workspace_bytes_augmented: out_bytes is null");
    ACX_TRY(check_augmented_shape("acx_workspace_bytes_augmented", B, L, has_lambda != 0, mode));
    ACX_TRY(need_ready(c));
    AugWs w;
    ACX_TRY(carve_augmented(c->dense_stft, B, L, has_wave_plan != 0, has_lambda != 0, mode, &w));
    *out_bytes = w.total;
    return ACX_OK;
}

int acx_forward_augmented(acx_ctx* c, const float* wav, int B, int64_t L, const acx_wave_aug* wave_plan,
                          const acx_spec_aug* spec_plan, const float* lambda, int mode, float* out0, float* out1, void* workspace,
                          size_t workspace_bytes, void* stream) {
    ACX_TRY(check_forward_args("acx_forward_augmented", wav, out0, out1, workspace, mode));
    ACX_TRY(check_augmented_shape("acx_forward_augmented", B, L, lambda != nullptr, mode));
    ACX_TRY(need_ready(c));
    AugWs w;
    ACX_TRY(carve_augmented(c->dense_stft, B, L, wave_plan != nullptr, lambda != nullptr, mode, &w));
    ACX_TRY(check_workspace(workspace, workspace_bytes, w.total));
    ACX_TRY(check_uniform_plans(c, lambda ? B / 2 : B, L, mode, nullptr, true));       // (before the first launch)
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int T = (int)(L / kHop + 1);
    const float* x = wav;
    if (wave_plan) {
        float* aug = (float*)(ws + w.wave);
        ACX_TRY(launch_augment_wave(wav, B, L, wave_plan, aug, st));
        x = aug;
    }
    float* feat = (float*)(ws + w.feat);
    AugFront front;
    augmented_front(w, c->dense_stft, (size_t)B * T, &front);
    auto lies = [&](int kind) -> float* {          // (null without the dense frontend: the FFT frontend needs no scratch)
        for (int i = 0; i < front.n_tenants; ++i) {
            const acx_plan_tenant_t& t = front.tenants[i];
            if (t.kind == kind) return (float*)(ws + front.regions[t.region - ACX_PLAN_AUG_WAVE].offset + t.offset);
        }
        return nullptr;
    };
    ACX_TRY(launch_logmel(c, x, B, L, T, feat, true, st, lies(ACX_PLAN_DENSE_FRAMES), lies(ACX_PLAN_DENSE_SPEC)));
    int Bf = B;
    if (lambda) {
        float* mix = (float*)(ws + w.mix);
        ACX_TRY(launch_augment_spec(feat, B, T, spec_plan, lambda, mix, st));
        feat = mix;
        Bf = B / 2;
    } else if (spec_plan) {
        ACX_TRY(launch_augment_spec(feat, B, T, spec_plan, nullptr, feat, st));
    }
    // everything above is queued on `st` in front of the fork event of the batch split: every sub-batch sees the finished rows
    return forward_uniform(c, nullptr, Bf, L, mode, out0, out1, ws + w.fwd, st, nullptr, nullptr, feat, true);
}

}  // extern "C"
