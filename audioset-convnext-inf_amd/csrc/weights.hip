// libacx weight intake: the state_dict key table, acx_set_weight, and acx_finalize's folding / repacking of the weights into
// the images the kernels read.  Host code only.
#include <cmath>
#include <cstring>

#include "acx_internal.h"

namespace acx {

struct KeySpec { std::string key; std::vector<int64_t> shape; };
constexpr int64_t kAnyClasses = -1;     // a KeySpec dim of the classifier head: N, 1 .. ACX_MAX_CLASSES

static std::vector<KeySpec> required_keys() {
    std::vector<KeySpec> v;
    v.push_back({"spectrogram_extractor.stft.conv_real.weight", {kBins, 1, kNFFT}});
    v.push_back({"spectrogram_extractor.stft.conv_imag.weight", {kBins, 1, kNFFT}});
    v.push_back({"logmel_extractor.melW", {kBins, kMels}});
    for (const char* k : {"bn0.weight", "bn0.bias", "bn0.running_mean", "bn0.running_var"}) v.push_back({k, {kMels}});
    v.push_back({"downsample_layers.0.0.weight", {kDims[0], 1, 4, 4}});
    v.push_back({"downsample_layers.0.0.bias", {kDims[0]}});
    v.push_back({"downsample_layers.0.1.weight", {kDims[0]}});
    v.push_back({"downsample_layers.0.1.bias", {kDims[0]}});
    char buf[96];
    for (int i = 1; i < 4; ++i) {
        snprintf(buf, sizeof buf, "downsample_layers.%d.0.weight", i); v.push_back({buf, {kDims[i - 1]}});
        snprintf(buf, sizeof buf, "downsample_layers.%d.0.bias", i); v.push_back({buf, {kDims[i - 1]}});
        snprintf(buf, sizeof buf, "downsample_layers.%d.1.weight", i); v.push_back({buf, {kDims[i], kDims[i - 1], 2, 2}});
        snprintf(buf, sizeof buf, "downsample_layers.%d.1.bias", i); v.push_back({buf, {kDims[i]}});
    }
    for (int s = 0; s < 4; ++s) {
        const int64_t C = kDims[s];
        for (int j = 0; j < kDepths[s]; ++j) {
            auto key = [&](const char* leaf) { snprintf(buf, sizeof buf, "stages.%d.%d.%s", s, j, leaf); return std::string(buf); };
            v.push_back({key("gamma"), {C}});
            v.push_back({key("dwconv.weight"), {C, 1, 7, 7}});
            v.push_back({key("dwconv.bias"), {C}});
            v.push_back({key("norm.weight"), {C}});
            v.push_back({key("norm.bias"), {C}});
            v.push_back({key("pwconv1.weight"), {4 * C, C}});
            v.push_back({key("pwconv1.bias"), {4 * C}});
            v.push_back({key("pwconv2.weight"), {C, 4 * C}});
            v.push_back({key("pwconv2.bias"), {C}});
        }
    }
    v.push_back({"norm.weight", {kDims[3]}});
    v.push_back({"norm.bias", {kDims[3]}});
    v.push_back({"head_audioset.weight", {kAnyClasses, kDims[3]}});
    v.push_back({"head_audioset.bias", {kAnyClasses}});
    return v;
}

static const std::vector<KeySpec>& key_table() {
    static const std::vector<KeySpec> t = required_keys();
    return t;
}

template <typename T>
static int upload(acx_ctx* c, const std::vector<T>& h, T** out) {
    void* d = nullptr;
    ACX_HIP(hipMalloc(&d, h.size() * sizeof(T)));
    c->allocs.push_back(d);
    ACX_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = static_cast<T*>(d);
    return ACX_OK;
}

// rows x K fp32 -> rows x Kp bf16, source column k of group q (K = groups * Kg) lands at q * Kgp + k
static std::vector<uint16_t> bf16_rows(const std::vector<float>& w, int rows, int groups, int Kg, int Kgp) {
    std::vector<uint16_t> h((size_t)rows * groups * Kgp, 0);
    for (int n = 0; n < rows; ++n)
        for (int q = 0; q < groups; ++q)
            for (int k = 0; k < Kg; ++k)
                h[((size_t)n * groups + q) * Kgp + k] = to_bf16(w[((size_t)n * groups + q) * Kg + k]);
    return h;
}

// power of two that brings max |w| into [2^14, 2^15): both fp16 halves of every weight within 2^13 of the largest
// stay normal numbers
static float s16_scale(const std::vector<float>& w) {
    float mx = 0.f;
    for (float v : w) mx = std::fmax(mx, std::fabs(v));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.f;
    return std::ldexp(1.0f, 14 - std::ilogb(mx));
}

// Power-of-two scale of the S16 hidden activation of one block.  The GEMM input is z = LayerNorm(y) without affine
// (the affine is folded into w1 / b1): ||z||_2 <= sqrt(C), so |h_n| = |w1_n . z + b1_n| <= ||w1_n||_2 sqrt(C) + |b1_n|
// (Cauchy-Schwarz) and |GELU(h)| <= |h|.  The scale puts that bound below the largest fp16 number: the GELU's
// fp32 -> fp16 conversion (split_math.h) cannot overflow, whatever the input (bounded below at 2^-24 -- weights of ~1e11).  Typical weights give 2^10..2^11; the absolute
// resolution of a stored value is 2^-25 / scale (fp16 subnormal spacing of the lo half).
static float hidden_scale_for(const std::vector<float>& w1, const std::vector<float>& b1, int N, int C) {
    double worst = 0.0;
    for (int n = 0; n < N; ++n) {
        double ss = 0.0;
        for (int k = 0; k < C; ++k) ss += (double)w1[(size_t)n * C + k] * w1[(size_t)n * C + k];
        worst = std::fmax(worst, std::sqrt(ss) * std::sqrt((double)C) + std::fabs((double)b1[n]));
    }
    if (!(worst > 0.0) || !std::isfinite(worst)) return 1.f;
    int e = (int)std::floor(std::log2(65000.0 / worst));
    e = e > 12 ? 12 : (e < -24 ? -24 : e);      // 2^-24: every scaled GELU coefficient stays a normal fp32 number (split_math.h, gelu_k3)
    return std::ldexp(1.0f, e);
}

void free_device(acx_ctx* c) {
    for (void* p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    for (int s = 0; s < 4; ++s) c->blocks[s].clear();
    c->d_dw_sink = nullptr;
    c->num_classes = 0;
    c->finalized = false;
}

static const std::vector<float>& W(const acx_ctx* c, const std::string& k) { return c->host.at(k).data; }

// max |stored - window x DFT| with the window read from bin 0 (cos = 1: that row IS the window)
static double stft_deviation_from_dft(const acx_ctx* c, std::vector<float>* hann_out) {
    const auto& re = W(c, "spectrogram_extractor.stft.conv_real.weight");
    const auto& im = W(c, "spectrogram_extractor.stft.conv_imag.weight");
    std::vector<float>& hann = *hann_out;
    hann.assign(re.begin(), re.begin() + kNFFT);      // bin 0: cos = 1, so the row IS the window
    double worst = 0.0;
    for (int k = 0; k < kBins; ++k) {
        for (int n = 0; n < kNFFT; ++n) {
            const double ang = 2.0 * M_PI * (double)(((long long)n * k) % kNFFT) / kNFFT;
            const double er = hann[n] * std::cos(ang), ei = -(double)hann[n] * std::sin(ang);
            worst = std::fmax(worst, std::fabs(er - re[(size_t)k * kNFFT + n]));
            worst = std::fmax(worst, std::fabs(ei - im[(size_t)k * kNFFT + n]));
        }
    }
    return worst;
}

static int finalize_impl(acx_ctx* c) {
    for (const auto& ks : key_table()) {
        auto it = c->host.find(ks.key);
        if (it == c->host.end()) ACX_FAIL(ACX_ERR_STATE, "missing weight '%s'", ks.key.c_str());
    }
    const int64_t n_w = c->host.at("head_audioset.weight").shape[0], n_b = c->host.at("head_audioset.bias").shape[0];
    if (n_w != n_b)
        ACX_FAIL(ACX_ERR_SHAPE, "'head_audioset.weight' has %lld rows but 'head_audioset.bias' has %lld entries: the classifier "
                 "head's weight and bias must have one row per class", (long long)n_w, (long long)n_b);
    ACX_HIP(hipSetDevice(c->device));
    free_device(c);

    // ---- frontend ---------------------------------------------------------------------------
    // The FFT stands in for the two Conv1d only if the stored buffers ARE window x DFT (any window; torchlibrosa's is the
    // periodic hann).  The reference applies whatever its state_dict holds (convnext.py:179-187, overwritten by
    // load_state_dict), so anything else -- a fine-tuned or hand-edited frontend -- runs as the dense contraction it is:
    // frames [B T, 1024] . [conv_real; conv_imag]^T on the f32 matrix cores (frontend.hip).
    std::vector<float> hann;
    const double dev = stft_deviation_from_dft(c, &hann);
    c->stft_deviation = (float)dev;
    c->dense_stft = c->force_dense_stft || !(dev <= 2e-6);
    c->d_stft_w = nullptr; c->d_stft_zero = nullptr;
    if (c->dense_stft) {
        std::vector<float> w((size_t)kDenseN * kNFFT, 0.f);
        const auto& re = W(c, "spectrogram_extractor.stft.conv_real.weight");
        const auto& im = W(c, "spectrogram_extractor.stft.conv_imag.weight");
        std::memcpy(w.data(), re.data(), (size_t)kBins * kNFFT * 4);
        std::memcpy(w.data() + (size_t)kBins * kNFFT, im.data(), (size_t)kBins * kNFFT * 4);
        ACX_TRY(upload(c, w, &c->d_stft_w));
        ACX_TRY(upload(c, std::vector<float>(kDenseN, 0.f), &c->d_stft_zero));
    }
    ACX_TRY(upload(c, hann, &c->d_hann));
    std::vector<float> tw(2 * kNFFT);
    for (int n = 0; n < kNFFT; ++n) {
        const double a = -2.0 * M_PI * n / kNFFT;
        tw[2 * n] = (float)std::cos(a);
        tw[2 * n + 1] = (float)std::sin(a);
    }
    ACX_TRY(upload(c, tw, &c->d_twiddle));
    {
        const auto& melW = W(c, "logmel_extractor.melW");     // [513][224]
        std::vector<int> start(kMels), len(kMels), off(kMels);
        std::vector<float> band;
        for (int m = 0; m < kMels; ++m) {
            int lo = -1, hi = -1;
            for (int k = 0; k < kBins; ++k)
                if (melW[(size_t)k * kMels + m] != 0.f) { if (lo < 0) lo = k; hi = k; }
            start[m] = lo < 0 ? 0 : lo;
            len[m] = lo < 0 ? 0 : hi - lo + 1;
            off[m] = (int)band.size();
            for (int k = 0; k < len[m]; ++k) band.push_back(melW[(size_t)(start[m] + k) * kMels + m]);
        }
        if (band.empty()) band.push_back(0.f);
        ACX_TRY(upload(c, start, &c->d_mel_start));
        ACX_TRY(upload(c, len, &c->d_mel_len));
        ACX_TRY(upload(c, off, &c->d_mel_off));
        ACX_TRY(upload(c, band, &c->d_mel_w));
        c->mel_w_len = (int)band.size();
    }
    {
        const auto &w = W(c, "bn0.weight"), &b = W(c, "bn0.bias"), &mu = W(c, "bn0.running_mean"),
                   &var = W(c, "bn0.running_var");
        std::vector<float> sc(kMels), sh(kMels);
        for (int m = 0; m < kMels; ++m) {
            const double s = (double)w[m] / std::sqrt((double)var[m] + 1e-5);   // BatchNorm2d eps default
            sc[m] = (float)s;
            sh[m] = (float)((double)b[m] - (double)mu[m] * s);
        }
        ACX_TRY(upload(c, sc, &c->d_bn_scale));
        ACX_TRY(upload(c, sh, &c->d_bn_shift));
        ACX_TRY(upload(c, std::vector<float>(kMels, 1.f), &c->d_bn_one));
        ACX_TRY(upload(c, std::vector<float>(kMels, 0.f), &c->d_bn_zero));
    }
    {   // where the column-streaming depthwise kernel parks the stores of rows that are not image rows (dwconv_col.hip)
        void* d = nullptr;
        ACX_HIP(hipMalloc(&d, kDwSinkBytes));
        c->allocs.push_back(d);
        c->d_dw_sink = d;
    }
    // ---- stem -------------------------------------------------------------------------------
    ACX_TRY(upload(c, W(c, "downsample_layers.0.0.weight"), &c->d_stem_w));
    ACX_TRY(upload(c, W(c, "downsample_layers.0.0.bias"), &c->d_stem_b));
    ACX_TRY(upload(c, W(c, "downsample_layers.0.1.weight"), &c->d_stem_lnw));
    ACX_TRY(upload(c, W(c, "downsample_layers.0.1.bias"), &c->d_stem_lnb));
    // ---- downsample convs: LayerNorm affine folded, K ordered (dy,dx,c) ------------------------
    char buf[96];
    for (int i = 1; i < 4; ++i) {
        const int Ci = kDims[i - 1], Co = kDims[i];
        auto key = [&](const char* leaf) { snprintf(buf, sizeof buf, "downsample_layers.%d.%s", i, leaf); return std::string(buf); };
        const auto &lnw = W(c, key("0.weight")), &lnb = W(c, key("0.bias")), &cw = W(c, key("1.weight")),
                   &cb = W(c, key("1.bias"));
        std::vector<float> w((size_t)Co * 4 * Ci), b(Co);
        for (int n = 0; n < Co; ++n) {
            double acc = cb[n];
            for (int ci = 0; ci < Ci; ++ci)
                for (int q = 0; q < 4; ++q) {
                    const float v = cw[(((size_t)n * Ci + ci) * 2 + (q >> 1)) * 2 + (q & 1)];
                    w[(size_t)n * 4 * Ci + (size_t)q * Ci + ci] = (float)((double)v * lnw[ci]);
                    acc += (double)v * lnb[ci];
                }
            b[n] = (float)acc;
        }
        DownW& d = c->down[i];
        d = DownW{};
        ACX_TRY(upload(c, b, &d.b));
        switch (c->precision) {
            case ACX_PREC_F32: ACX_TRY(upload(c, w, &d.w)); break;
            case ACX_PREC_F32_SPLIT:
                d.ws_scale = s16_scale(w);
                ACX_TRY(upload(c, s16_rows(w, Co, 4 * Ci, d.ws_scale), &d.ws));
                break;
            default: ACX_TRY(upload(c, bf16_rows(w, Co, 4, Ci, pad64(Ci)), &d.wh));      // bf16, bf16a
        }
    }
    // ---- blocks -----------------------------------------------------------------------------
    for (int s = 0; s < 4; ++s) {
        const int C = kDims[s];
        for (int j = 0; j < kDepths[s]; ++j) {
            auto key = [&](const char* leaf) { snprintf(buf, sizeof buf, "stages.%d.%d.%s", s, j, leaf); return std::string(buf); };
            const auto &gamma = W(c, key("gamma")), &dw = W(c, key("dwconv.weight")), &dwb = W(c, key("dwconv.bias")),
                       &lnw = W(c, key("norm.weight")), &lnb = W(c, key("norm.bias")), &w1 = W(c, key("pwconv1.weight")),
                       &b1 = W(c, key("pwconv1.bias")), &w2 = W(c, key("pwconv2.weight")), &b2 = W(c, key("pwconv2.bias"));
            BlockW bw;
            std::vector<float> t((size_t)49 * C);
            for (int ch = 0; ch < C; ++ch)
                for (int tap = 0; tap < 49; ++tap) t[(size_t)tap * C + ch] = dw[(size_t)ch * 49 + tap];
            ACX_TRY(upload(c, t, &bw.dw));
            ACX_TRY(upload(c, dwb, &bw.dwb));
            std::vector<float> f1((size_t)4 * C * C), fb1((size_t)4 * C), fs1((size_t)4 * C);
            for (int n = 0; n < 4 * C; ++n) {
                double acc = b1[n], csum = 0.0;
                for (int k = 0; k < C; ++k) {
                    const float v = w1[(size_t)n * C + k];
                    const float f = (float)((double)v * lnw[k]);
                    f1[(size_t)n * C + k] = f;
                    csum += (double)f;                      // of the fp32 values the GEMM really multiplies
                    acc += (double)v * lnb[k];
                }
                fb1[n] = (float)acc;
                fs1[n] = (float)csum;
            }
            ACX_TRY(upload(c, fb1, &bw.b1));
            std::vector<float> f2((size_t)C * 4 * C), fb2(C);
            for (int n = 0; n < C; ++n) {
                for (int k = 0; k < 4 * C; ++k) f2[(size_t)n * 4 * C + k] = (float)((double)gamma[n] * w2[(size_t)n * 4 * C + k]);
                fb2[n] = (float)((double)gamma[n] * b2[n]);
            }
            ACX_TRY(upload(c, fb2, &bw.b2));
            // the weight images the launches of this arithmetic read (run_block), nothing else
            switch (c->precision) {
                case ACX_PREC_F32:
                    if (mlp_fused_supported(C)) {
                        ACX_TRY(upload(c, mlp_fused_pack(f1, f2, C), &bw.wpack));
                    } else {
                        ACX_TRY(upload(c, f1, &bw.w1));
                        ACX_TRY(upload(c, fs1, &bw.w1sum));
                        ACX_TRY(upload(c, f2, &bw.w2));
                    }
                    break;
                case ACX_PREC_F32_SPLIT:
                    bw.w1s_scale = s16_scale(f1);
                    bw.w2s_scale = s16_scale(f2);
                    bw.hid_scale = hidden_scale_for(f1, fb1, 4 * C, C);
                    if (mlp_fused_split_supported(C)) {
                        ACX_TRY(upload(c, mlp_fused_split_pack(f1, f2, C, bw.w1s_scale, bw.w2s_scale), &bw.wpack_s));
                    } else if (mlp_fused_wide_supported(C)) {
                        ACX_TRY(upload(c, mlp_fused_wide_pack(f1, f2, C, bw.w1s_scale, bw.w2s_scale), &bw.wstream_s));
                    } else {
                        ACX_TRY(upload(c, s16_rows(f1, 4 * C, C, bw.w1s_scale), &bw.w1s));
                        ACX_TRY(upload(c, s16_rows(f2, C, 4 * C, bw.w2s_scale), &bw.w2s));
                    }
                    break;
                default:                                                    // bf16, bf16a
                    if (mlp_fused_wide_bf16_supported(C)) {
                        ACX_TRY(upload(c, mlp_fused_wide_bf16_pack(f1, f2, C), &bw.wstream_b));
                    } else {
                        ACX_TRY(upload(c, bf16_rows(f1, 4 * C, 1, C, pad64(C)), &bw.w1h));
                        ACX_TRY(upload(c, bf16_rows(f2, C, 1, 4 * C, 4 * C), &bw.w2h));
                    }
                    if (act_bf16(c, s)) ACX_TRY(upload(c, dwconv_mfma_pack(dw, C), &bw.dw_ops));
            }
            c->blocks[s].push_back(bw);
        }
    }
    // ---- tail -------------------------------------------------------------------------------
    ACX_TRY(upload(c, W(c, "norm.weight"), &c->d_norm_w));
    ACX_TRY(upload(c, W(c, "norm.bias"), &c->d_norm_b));
    ACX_TRY(upload(c, W(c, "head_audioset.weight"), &c->d_head_w));
    ACX_TRY(upload(c, W(c, "head_audioset.bias"), &c->d_head_b));
    c->num_classes = (int)n_w;
    c->finalized = true;
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_set_weight(acx_ctx* c, const char* key, const float* host_data, const int64_t* shape, int ndim) {
    if (!c || !key || (ndim > 0 && !shape)) ACX_FAIL(ACX_ERR_ARG, "acx_set_weight: null argument");
    for (const auto& ks : key_table()) {
        if (ks.key != key) continue;
        if ((int)ks.shape.size() != ndim) ACX_FAIL(ACX_ERR_SHAPE, "'%s': expected %d dims, got %d", key, (int)ks.shape.size(), ndim);
        size_t n = 1;
        for (int d = 0; d < ndim; ++d) {
            if (ks.shape[d] == kAnyClasses) {
                if (shape[d] < 1 || shape[d] > ACX_MAX_CLASSES)
                    ACX_FAIL(ACX_ERR_SHAPE, "'%s': dim %d is %lld classes, expected 1 .. %d", key, d, (long long)shape[d],
                             ACX_MAX_CLASSES);
            } else if (shape[d] != ks.shape[d]) {
                ACX_FAIL(ACX_ERR_SHAPE, "'%s': dim %d is %lld, expected %lld", key, d, (long long)shape[d], (long long)ks.shape[d]);
            }
            n *= (size_t)shape[d];
        }
        if (!host_data) ACX_FAIL(ACX_ERR_ARG, "acx_set_weight: null argument");     // (after the shape: a 0-row head has no data)
        HostTensor& t = c->host[key];
        t.shape.assign(shape, shape + ndim);
        t.data.assign(host_data, host_data + n);
        c->finalized = false;
        return ACX_OK;
    }
    ACX_FAIL(ACX_ERR_ARG, "acx_set_weight: unexpected key '%s'", key);
}

int acx_finalize(acx_ctx* c) {
    if (!c) ACX_FAIL(ACX_ERR_ARG, "null context");
    c->fail_sub.store(-1, std::memory_order_relaxed);       // an armed test hook never outlives the weights it was armed on
    int rc = finalize_impl(c);
    if (rc != ACX_OK) { free_device(c); }
    return rc;
}

}  // extern "C"
