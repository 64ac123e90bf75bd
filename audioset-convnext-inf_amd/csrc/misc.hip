// K6 -- tail of forward_features + head (convnext.py:279-285, :321-325), and the NHWC->NCHW
// transpose that gives forward_frame_embeddings its layout (convnext.py:276-277).
#include "acx_internal.h"
#include "device_common.h"

namespace acx {

// One workgroup of 768 threads per clip.  x NHWC (B,H3,7,768):
//   mean over the 7 frequency columns (torch.mean(x, dim=3)), then max over time + mean over time,
//   nn.LayerNorm(768, eps=1e-6) -> scene embedding; Linear 768->N -> logits; sigmoid -> probs.
// Thread = (float4 of channels, one of 4 time phases): every thread streams ~H3/4 rows x 7 columns of
// independent 16-B loads (the first version walked all H3 rows serially per thread: latency-bound, 143 us),
// partial (max, sum) meet in LDS.
// VAR: a variable-length batch -- clip b has H3 = roff3[b + 1] - roff3[b] rows from row roff3[b] on (same reduction order)
template <bool VAR>
__global__ __launch_bounds__(768) void pool_head_kernel(const float* __restrict__ x, int H3_,
                                                        const float* __restrict__ nw, const float* __restrict__ nb,
                                                        const float* __restrict__ hw, const float* __restrict__ hb,
                                                        float* __restrict__ scene, float* __restrict__ logits,
                                                        float* __restrict__ probs, const int* __restrict__ roff3, int N) {
    __shared__ __attribute__((aligned(16))) float pmax[4][768];
    __shared__ __attribute__((aligned(16))) float psum[4][768];
    __shared__ __attribute__((aligned(16))) float emb[768];
    __shared__ float red[12];
    const int tid = threadIdx.x;
    const int cg = tid % 192, ph = tid / 192;
    const long long b = blockIdx.x;
    const int H3 = VAR ? roff3[b + 1] - roff3[b] : H3_;
    const long long row0 = VAR ? (long long)roff3[b] : b * (long long)H3;
    const float* xb = x + row0 * 7 * 768 + 4 * cg;
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), sm = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h = ph; h < H3; h += 4) {
        const float4 s = freq_mean7(xb + (long long)h * 7 * 768);
        mx.x = fmaxf(mx.x, s.x); mx.y = fmaxf(mx.y, s.y); mx.z = fmaxf(mx.z, s.z); mx.w = fmaxf(mx.w, s.w);
        sm.x += s.x; sm.y += s.y; sm.z += s.z; sm.w += s.w;
    }
    *reinterpret_cast<float4*>(&pmax[ph][4 * cg]) = mx;
    *reinterpret_cast<float4*>(&psum[ph][4 * cg]) = sm;
    __syncthreads();
    // thread c: combine the 4 phases (time order of the sum is (h%4, h/4) -- fp32 re-association only)
    const int c = tid;
    const float m = fmaxf(fmaxf(pmax[0][c], pmax[1][c]), fmaxf(pmax[2][c], pmax[3][c]));
    const float su = (psum[0][c] + psum[1][c]) + (psum[2][c] + psum[3][c]);
    const float pooled = m + su / (float)H3;
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) t += red[i];
        return t;
    };
    const float mean = block_sum(pooled) * (1.0f / 768.0f);
    const float d = pooled - mean;
    const float var = block_sum(d * d) * (1.0f / 768.0f);
    const float rstd = 1.0f / sqrtf(var + 1e-6f);
    const float e0 = fmaf(d * rstd, nw[c], nb[c]);
    emb[c] = e0;
    if (scene) scene[b * 768 + c] = e0;
    __syncthreads();
    if (!logits && !probs) return;
    const int lane = tid & 63, wave = tid >> 6;
    float4 e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = *reinterpret_cast<const float4*>(&emb[4 * (lane + 64 * k)]);
    // four rows of the head per wave and pass: 12 independent 16-byte loads per lane in flight (one row at a time was a chain
    // of 44 L2 round trips per wave).  The per-class arithmetic is head_dot over lane l's chunks l, l + 64, l + 128, wave_sum,
    // + b[n], head_sigmoid (device_common.h), the calls head_tiled_kernel makes as well: both give the same bits.
    for (int n0 = wave; n0 < N; n0 += 48) {
        float4 w4[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 12 * r < N ? n0 + 12 * r : n0;
            const float4* wr = reinterpret_cast<const float4*>(hw + (long long)n * 768);
#pragma unroll
            for (int k = 0; k < 3; ++k) w4[r][k] = wr[lane + 64 * k];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = wave_sum(head_dot(e, w4[r]));
            const int n = n0 + 12 * r;
            if (lane == 0 && n < N) {
                const float z = s + hb[n];
                if (logits) logits[b * N + n] = z;
                if (probs) probs[b * N + n] = head_sigmoid(z);
            }
        }
    }
}

// Class-tiled head for wide heads (kHeadTiledMin): logits / probs (B, N) from the scene rows (B, 768) that pool_head_kernel wrote.
// pool_head_kernel reads the whole head once per clip (N = 16384: 48 MiB per clip, one busy CU per clip); here a workgroup holds
// kHeadBt scene rows in LDS and applies the kHeadNt rows of its class tile to all of them, so the head is read ceil(B / kHeadBt)
// times and the grid fills the chip.  Every (clip, class) value is pool_head_kernel's arithmetic, by the same calls: lane l holds
// chunks l, l + 64, l + 128 of the row and of the embedding, head_dot, wave_sum, + b[n], head_sigmoid (device_common.h).
// Plain fp32 VALU, no MFMA: the bits stay, and the kernel is not CU-exclusive.
// 4 waves; wave w takes classes w * 4 .. w * 4 + 3 of each group of 16, 4 rows in flight as in pool_head_kernel.  After the
// wave_sums every lane holds each sum; lane r * 16 + i keeps (class r, clip i) of a pass of 16 clips, so that all 64 lanes add
// the bias, take the sigmoid and store (64 values per store instruction instead of one from lane 0).
// Grid: one workgroup per (clip tile, class tile), numbered so that the clip tiles of a class tile share blockIdx.x % 8 -- one
// XCD under round-robin placement, so they read its rows through one L2 (speed only).
constexpr int kHeadBt = 16;     // clips per workgroup
constexpr int kHeadNt = 64;     // classes per workgroup
__global__ __launch_bounds__(256) void head_tiled_kernel(const float* __restrict__ scene, int B, int N,
                                                         const float* __restrict__ hw, const float* __restrict__ hb,
                                                         float* __restrict__ logits, float* __restrict__ probs, int ctiles) {
    __shared__ __attribute__((aligned(16))) float emb[kHeadBt][768];
    const int btiles = (B + kHeadBt - 1) / kHeadBt;
    const int g = blockIdx.x;
    const int q = g / (8 * btiles), rem = g - q * 8 * btiles;
    const int bt = rem / 8, ct = q * 8 + (rem & 7);
    if (ct >= ctiles) return;                       // (the class-tile count is padded to a multiple of 8)
    const int b0 = bt * kHeadBt, nb = B - b0 < kHeadBt ? B - b0 : kHeadBt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nb * 192; i += 256) {
        const int r = i / 192, c4 = i - r * 192;
        *reinterpret_cast<float4*>(&emb[r][4 * c4]) = reinterpret_cast<const float4*>(scene + (long long)(b0 + r) * 768)[c4];
    }
    __syncthreads();
    for (int n0 = ct * kHeadNt + wave * 4; n0 < (ct + 1) * kHeadNt && n0 < N; n0 += 16) {
        float4 w4[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + r < N ? n0 + r : n0;
            const float4* wr = reinterpret_cast<const float4*>(hw + (long long)n * 768);
#pragma unroll
            for (int k = 0; k < 3; ++k) w4[r][k] = wr[lane + 64 * k];
        }
        const int nr = lane >> 4;                  // the class this lane stores: n0 + nr
        const float bias = hb[n0 + nr < N ? n0 + nr : n0];
        for (int i0 = 0; i0 < nb; i0 += 16) {
            float mine = 0.f;
            for (int i = i0; i < i0 + 16 && i < nb; ++i) {
                float4 e[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) e[k] = *reinterpret_cast<const float4*>(&emb[i][4 * (lane + 64 * k)]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = wave_sum(head_dot(e, w4[r]));
                    if (lane == r * 16 + (i - i0)) mine = s;
                }
            }
            const int i = i0 + (lane & 15), n = n0 + nr;
            if (i < nb && n < N) {
                const float z = mine + bias;
                const long long o = (long long)(b0 + i) * N + n;
                if (logits) logits[o] = z;
                if (probs) probs[o] = head_sigmoid(z);
            }
        }
    }
}

bool head_tiled(const acx_ctx* c) {
    const int force = tuning().head_path.load(std::memory_order_relaxed);
    if (force == 1) return false;
    if (force == 2) return true;
    return c->num_classes >= kHeadTiledMin;
}

int launch_head_tiled(acx_ctx* c, const float* scene, int B, float* logits, float* probs, hipStream_t s) {
    const int N = c->num_classes;
    const int btiles = (B + kHeadBt - 1) / kHeadBt, ctiles = (N + kHeadNt - 1) / kHeadNt;
    const long long blocks = (long long)((ctiles + 7) / 8) * 8 * btiles;
    if (blocks > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "head: %d clips x %d classes is too large a grid", B, N);
    ProfScope ps(c, ACX_K_POOLHEAD, s);
    launch_kernel(&head_tiled_kernel, dim3((unsigned)blocks), dim3(256), 0, s, scene, B, N, c->d_head_w, c->d_head_b, logits,
                  probs, ctiles);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_pool_head(acx_ctx* c, const float* x, int B, int H3, float* scene, float* logits, float* probs,
                     hipStream_t s) {
    ProfScope ps(c, ACX_K_POOLHEAD, s);
    launch_kernel(&pool_head_kernel<false>, dim3(B), dim3(768), 0, s, x, H3, c->d_norm_w, c->d_norm_b, c->d_head_w, c->d_head_b,
                                                   scene, logits, probs, (const int*)nullptr, c->num_classes);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_pool_head_varlen(acx_ctx* c, const float* x, const VarGeom& vg, float* scene, float* logits, float* probs,
                            hipStream_t s) {
    ProfScope ps(c, ACX_K_POOLHEAD, s);
    launch_kernel(&pool_head_kernel<true>, dim3(vg.B), dim3(768), 0, s, x, 0, c->d_norm_w, c->d_norm_b, c->d_head_w, c->d_head_b,
                  scene, logits, probs, vg.roff[3], c->num_classes);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// out[b][c][p] = x[b][p][c], p = h*W + w.  32x32 tiles through LDS (+1 pad), coalesced both ways.
// VAR: a variable-length batch -- clip b is the block of P = (roff3[b + 1] - roff3[b]) x W pixels from pixel roff3[b] W on,
// in the input and in the output alike (the grid covers the tallest clip)
template <bool VAR>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                           int P_, int C, const int* __restrict__ roff3, int W) {
    __shared__ float t[32][33];
    const long long b = blockIdx.z;
    const int P = VAR ? (roff3[b + 1] - roff3[b]) * W : P_;
    const long long base = VAR ? (long long)roff3[b] * W * C : b * (long long)P * C;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    if (VAR && p0 >= P) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const float* xb = x + base;
    float* ob = out + base;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + 8 * i;
        if (p < P) t[ty + 8 * i][tx] = xb[(long long)p * C + c0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i;
        const int p = p0 + tx;
        if (p < P) ob[(long long)c * P + p] = t[tx][ty + 8 * i];
    }
}

int launch_nhwc_to_nchw(acx_ctx* c, const float* x, float* out, int B, int H, int W, int C, hipStream_t s) {
    if (C % 32 != 0) ACX_FAIL(ACX_ERR_SHAPE, "nhwc_to_nchw: C=%d is not a multiple of 32", C);
    const int P = H * W;
    ProfScope ps(c, ACX_K_TRANSPOSE, s);
    launch_kernel(&nhwc_to_nchw_kernel<false>, dim3((P + 31) / 32, C / 32, B), dim3(256), 0, s, x, out, P, C, (const int*)nullptr, W);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_nhwc_to_nchw_varlen(acx_ctx* c, const float* x, float* out, const VarGeom& vg, hipStream_t s) {
    const int W = kStemW >> 3, C = kDims[3];
    const int Pmax = vg.maxH[3] * W;
    ProfScope ps(c, ACX_K_TRANSPOSE, s);
    launch_kernel(&nhwc_to_nchw_kernel<true>, dim3((Pmax + 31) / 32, C / 32, vg.B), dim3(256), 0, s, x, out, 0, C, vg.roff[3], W);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// Stored clips -> model input: AudioSet shards hold int16 PCM and the reference scales by 1 / 32767 on the host
// (utilities.py:226-227 `int16_to_float32`: (x / 32767.0).astype(np.float32), numpy promotes to float64).  Here the clips cross
// PCIe as int16 and are widened on the GPU: float(double(x) / 32767.0) -- the same two roundings, so the same bits -- 8 samples
// (16 bytes in, 32 out) per thread and step; the tail of an odd-length buffer sample by sample.
__global__ __launch_bounds__(256) void pcm16_to_f32_kernel(const short* __restrict__ in, float* __restrict__ out, long long n) {
    const long long n8 = n >> 3;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const uint4 u = reinterpret_cast<const uint4*>(in)[i];
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
        float r[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            r[2 * q] = (float)((double)(short)(w[q] & 0xffffu) / 32767.0);
            r[2 * q + 1] = (float)((double)(short)(w[q] >> 16) / 32767.0);
        }
        reinterpret_cast<float4*>(out)[2 * i] = make_float4(r[0], r[1], r[2], r[3]);
        reinterpret_cast<float4*>(out)[2 * i + 1] = make_float4(r[4], r[5], r[6], r[7]);
    }
    for (long long i = (n8 << 3) + blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = (float)((double)in[i] / 32767.0);
}

int launch_pcm16_to_f32(const short* in, float* out, long long n, hipStream_t s) {
    if ((reinterpret_cast<uintptr_t>(in) & 15) || (reinterpret_cast<uintptr_t>(out) & 15))
        ACX_FAIL(ACX_ERR_ARG, "acx_pcm16_to_f32: buffers must be 16-byte aligned");
    long long blocks = (n / 8 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;
    launch_kernel(&pcm16_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, out, n);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// element-wise fp32 <-> bf16 (round to nearest even): the per-layer entry points of the C ABI keep fp32 tensors in every mode
// and convert at their boundary when the activations live in HBM as bf16 (ACX_PREC_BF16_ACT)
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ in, __bf16* __restrict__ out, long long n4) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(in)[i];
        reinterpret_cast<uint2*>(out)[i] = uint2{acx_pack_bf16x2(v.x, v.y), acx_pack_bf16x2(v.z, v.w)};
    }
}
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const __bf16* __restrict__ in, float* __restrict__ out, long long n4) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const uint2 u = reinterpret_cast<const uint2*>(in)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(acx_bf16_lo(u.x), acx_bf16_hi(u.x), acx_bf16_lo(u.y), acx_bf16_hi(u.y));
    }
}
int launch_convert_f32_to_bf16(const float* in, void* out, long long n, hipStream_t s) {
    if (n % 4 != 0) ACX_FAIL(ACX_ERR_SHAPE, "convert: %lld elements (not a multiple of 4)", n);
    const long long n4 = n / 4;
    if (n4 == 0) return ACX_OK;
    const long long blocks = (n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096;
    launch_kernel(&f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, reinterpret_cast<__bf16*>(out), n4);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}
int launch_convert_bf16_to_f32(const void* in, float* out, long long n, hipStream_t s) {
    if (n % 4 != 0) ACX_FAIL(ACX_ERR_SHAPE, "convert: %lld elements (not a multiple of 4)", n);
    const long long n4 = n / 4;
    if (n4 == 0) return ACX_OK;
    const long long blocks = (n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096;
    launch_kernel(&bf16_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const __bf16*>(in), out, n4);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx
