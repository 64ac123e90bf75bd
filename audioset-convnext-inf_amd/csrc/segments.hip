// Sound event detection: segment-wise and frame-wise outputs from the stage-3 map (include/acx.h, "sound event detection").
// The reference's decision-level recipe (pytorch/models.py:5757-5771, pytorch/pytorch_utils.py:140-176) on the ConvNeXt trunk:
//   segment_pool_kernel     NHWC x (rows of 7 x 768) -> mean over frequency, max + average over `pool` rows of time, the final
//                           LayerNorm (convnext.py:279-285 per segment instead of per clip) -> one embedding row per segment
//   segment_head_kernel     (segments) x N x 768 fp32 GEMM on the f32-input matrix cores + bias + sigmoid (convnext.py:321-325)
//   segment_clipmax_kernel  clip[n] = max over a clip's segments (models.py:5767)
//   segment_expand_kernel   frame[u] = segment[min(u / 32, S - 1)]  (interpolate + pad_framewise_output)
// Everything is fp32 whatever acx_set_precision says, as the head of the clip-level forward is.
//
// Bits.  A value (segment, class) is one fixed sequence of fp32 operations on that segment's rows of x and that head row.  The
// pooling adds the rows of a window in ascending time.  In the head each of a workgroup's four waves contracts a quarter of
// K = 768 and the four partial sums meet in wave order; inside a wave the contraction walks its 192 inputs in blocks of 16,
// block by block alternating between two accumulators that are added at the end, and inside a block in the order
// 0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15.  That order is what four v_mfma_f32_16x16x4_f32 make of one 16-byte load per lane
// (lane group h holds inputs 4 h .. 4 h + 3) and ALSO what eight v_mfma_f32_32x32x2_f32 make of two (lane group h holds
// 4 h .. 4 h + 3 and 8 + 4 h .. 8 + 4 h + 3, used alternately): the two tile shapes give the same bits, so the choice between
// them -- by the size of the launch -- never shows in a result.  No atomics anywhere.
#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kSegTs = 4;          // segments per workgroup of the pooling kernel

// One workgroup of 192 threads per (clip, kSegTs consecutive segments); a thread owns four channels.  It walks the rows
// t0 - pool / 2 .. t0 + kSegTs - 1 + pool / 2 that exist, one 7 x 16-byte load group per row, and folds each row's frequency
// mean (freq_mean7, device_common.h: pool_head_kernel's call) into the running (max, sum) of every segment of the tile whose
// window holds it: registers only.  The LayerNorm statistics of the tile's rows are reduced by wave_sum, then the three waves
// in order through LDS.
// VAR: clip b owns rows [roff3[b], roff3[b + 1]) of x and of emb.
template <bool VAR>
__global__ __launch_bounds__(192) void segment_pool_kernel(const float* __restrict__ x, int S_, int pool, int tiles,
                                                           const float* __restrict__ nw, const float* __restrict__ nb,
                                                           float* __restrict__ emb, const int* __restrict__ roff3) {
    __shared__ float red[2][3][kSegTs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x % tiles) * kSegTs;
    const int S = VAR ? roff3[b + 1] - roff3[b] : S_;
    if (t0 >= S) return;                                           // (VAR: the grid covers the tallest clip)
    const long long row0 = VAR ? (long long)roff3[b] : b * (long long)S;
    const int hp = pool >> 1;
    const int nt = S - t0 < kSegTs ? S - t0 : kSegTs;
    const int s_lo = t0 - hp > 0 ? t0 - hp : 0;
    const int s_hi = t0 + nt - 1 + hp < S - 1 ? t0 + nt - 1 + hp : S - 1;
    const float* xb = x + row0 * 7 * 768 + 4 * tid;
    float4 mx[kSegTs], sm[kSegTs];
#pragma unroll
    for (int i = 0; i < kSegTs; ++i) {
        mx[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        sm[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int s = s_lo; s <= s_hi; ++s) {
        const float4 z = freq_mean7(xb + (long long)s * 7 * 768);
#pragma unroll
        for (int i = 0; i < kSegTs; ++i) {
            const int t = t0 + i;
            if (s >= t - hp && s <= t + hp) {
                mx[i].x = fmaxf(mx[i].x, z.x); mx[i].y = fmaxf(mx[i].y, z.y);
                mx[i].z = fmaxf(mx[i].z, z.z); mx[i].w = fmaxf(mx[i].w, z.w);
                sm[i].x += z.x; sm[i].y += z.y; sm[i].z += z.z; sm[i].w += z.w;
            }
        }
    }
    const float fpool = (float)pool;
    float4 p[kSegTs];
    float part[kSegTs];
#pragma unroll
    for (int i = 0; i < kSegTs; ++i) {
        p[i] = make_float4(mx[i].x + sm[i].x / fpool, mx[i].y + sm[i].y / fpool, mx[i].z + sm[i].z / fpool,
                           mx[i].w + sm[i].w / fpool);
        part[i] = i < nt ? wave_sum((p[i].x + p[i].y) + (p[i].z + p[i].w)) : 0.f;
        if (lane == 0) red[0][wave][i] = part[i];
    }
    __syncthreads();
    float4 d[kSegTs];
#pragma unroll
    for (int i = 0; i < kSegTs; ++i) {
        const float mean = ((red[0][0][i] + red[0][1][i]) + red[0][2][i]) * (1.0f / 768.0f);
        d[i] = make_float4(p[i].x - mean, p[i].y - mean, p[i].z - mean, p[i].w - mean);
        part[i] = i < nt ? wave_sum((d[i].x * d[i].x + d[i].y * d[i].y) + (d[i].z * d[i].z + d[i].w * d[i].w)) : 0.f;
        if (lane == 0) red[1][wave][i] = part[i];
    }
    __syncthreads();
    const float4 w4 = *reinterpret_cast<const float4*>(nw + 4 * tid), b4 = *reinterpret_cast<const float4*>(nb + 4 * tid);
#pragma unroll
    for (int i = 0; i < kSegTs; ++i) {
        if (i >= nt) break;
        const float var = ((red[1][0][i] + red[1][1][i]) + red[1][2][i]) * (1.0f / 768.0f);
        const float rstd = 1.0f / sqrtf(var + 1e-6f);
        const float4 e = make_float4(fmaf(d[i].x * rstd, w4.x, b4.x), fmaf(d[i].y * rstd, w4.y, b4.y),
                                     fmaf(d[i].z * rstd, w4.z, b4.z), fmaf(d[i].w * rstd, w4.w, b4.w));
        *reinterpret_cast<float4*>(emb + (row0 + t0 + i) * 768 + 4 * tid) = e;
    }
}

int launch_segment_pool(acx_ctx* c, const float* x, int B, int S, int pool, float* emb, const int* roff3, int maxS, hipStream_t s) {
    const int tiles = ((roff3 ? maxS : S) + kSegTs - 1) / kSegTs;
    const long long blocks = (long long)B * tiles;
    if (blocks < 1 || blocks > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "segments: %d clips x %d segments is not a launchable grid", B, S);
    ProfScope ps(c, ACX_K_POOLHEAD, s);
    if (roff3) launch_kernel(&segment_pool_kernel<true>, dim3((unsigned)blocks), dim3(192), 0, s, x, 0, pool, tiles, c->d_norm_w, c->d_norm_b, emb, roff3);
    else launch_kernel(&segment_pool_kernel<false>, dim3((unsigned)blocks), dim3(192), 0, s, x, S, pool, tiles, c->d_norm_w, c->d_norm_b, emb, (const int*)nullptr);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// ---- the head ------------------------------------------------------------------------------------------------------------
// F32Tile (device_common.h) + block(): one block of 16 inputs of the contraction
template <int S> struct SegTile;
template <> struct SegTile<32> : F32Tile<32> {
    // lane group h (0, 1) holds 4 h .. 4 h + 3 and 8 + 4 h .. 8 + 4 h + 3
    static __device__ __forceinline__ acc_t block(const float* a, const float* b, int h, acc_t c) {
        const float4 ap = *reinterpret_cast<const float4*>(a + 4 * h), aq = *reinterpret_cast<const float4*>(a + 8 + 4 * h);
        const float4 bp = *reinterpret_cast<const float4*>(b + 4 * h), bq = *reinterpret_cast<const float4*>(b + 8 + 4 * h);
        c = mfma(ap.x, bp.x, c); c = mfma(aq.x, bq.x, c);
        c = mfma(ap.y, bp.y, c); c = mfma(aq.y, bq.y, c);
        c = mfma(ap.z, bp.z, c); c = mfma(aq.z, bq.z, c);
        c = mfma(ap.w, bp.w, c); c = mfma(aq.w, bq.w, c);
        return c;
    }
};
template <> struct SegTile<16> : F32Tile<16> {
    // lane group h (0 .. 3) holds 4 h .. 4 h + 3
    static __device__ __forceinline__ acc_t block(const float* a, const float* b, int h, acc_t c) {
        const float4 av = *reinterpret_cast<const float4*>(a + 4 * h), bv = *reinterpret_cast<const float4*>(b + 4 * h);
        c = mfma(av.x, bv.x, c); c = mfma(av.y, bv.y, c);
        c = mfma(av.z, bv.z, c); c = mfma(av.w, bv.w, c);
        return c;
    }
};

struct SegHeadP {
    const float* E; long long M; int N;
    const float* W; const float* b;
    float* logits; float* probs;
    int tiles_n;
};

constexpr int kSegK = 768;
constexpr int kSegThreads = 256;       // four waves: the contraction is split four ways

// Tiles of S segments x S classes.  Rows past M and classes past N repeat the last valid one: loads stay inside the buffers,
// their results are dropped.
template <int S>
__global__ __launch_bounds__(kSegThreads) void segment_head_kernel(SegHeadP p) {
    using T = SegTile<S>;
    constexpr int KW = kSegK / 4;                  // inputs per wave
    __shared__ float red[4][S * S];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane % S, h = lane / S;
    const int tile_c = blockIdx.x % p.tiles_n, tile_r = blockIdx.x / p.tiles_n;
    const long long row0 = (long long)tile_r * S;
    const int c0 = tile_c * S;
    const long long er = row0 + r < p.M ? row0 + r : p.M - 1;
    const int wc = c0 + r < p.N ? c0 + r : p.N - 1;
    const float* ea = p.E + er * kSegK + wave * KW;
    const float* wb = p.W + (long long)wc * kSegK + wave * KW;

    typename T::acc_t acc0, acc1;
#pragma unroll
    for (int i = 0; i < T::REGS; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll 2
    for (int kb = 0; kb < KW / 32; ++kb) {
        acc0 = T::block(ea + 32 * kb, wb + 32 * kb, h, acc0);
        acc1 = T::block(ea + 32 * kb + 16, wb + 32 * kb + 16, h, acc1);
    }
    tile_spill<S>([&](int i) { return acc0[i] + acc1[i]; }, red[wave], r, h);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < S * S / kSegThreads; ++q) {
        const int e = tid + kSegThreads * q;
        const int rr = e / S, cc = e % S;
        const long long row = row0 + rr;
        const int c = c0 + cc;
        if (row < p.M && c < p.N) {
            const float z = tile_sum4(red, e) + p.b[c];
            const long long o = row * p.N + c;
            p.logits[o] = z;
            p.probs[o] = head_sigmoid(z);
        }
    }
}

int launch_segment_head(acx_ctx* c, const float* emb, long long M, float* logits, float* probs, hipStream_t s) {
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));
    const int N = c->num_classes;
    if (M < 1) ACX_FAIL(ACX_ERR_SHAPE, "segment head: %lld rows", M);
    SegHeadP p;
    p.E = emb; p.M = M; p.N = N; p.W = c->d_head_w; p.b = c->d_head_b; p.logits = logits; p.probs = probs;
    // 32 x 32 tiles when there is at least one per CU (counting the other sub-batches of a split forward), 16 x 16 otherwise
    const bool big = ((M + 31) / 32) * ((N + 31) / 32) * inflight_ways() >= cus;
    const int ts = big ? 32 : 16;
    p.tiles_n = (N + ts - 1) / ts;
    const long long tiles = ((M + ts - 1) / ts) * p.tiles_n;
    if (tiles > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "segment head: %lld segments x %d classes is too large a grid", M, N);
    ProfScope ps(c, ACX_K_POOLHEAD, s);
    if (big) launch_kernel(&segment_head_kernel<32>, dim3((unsigned)tiles), dim3(kSegThreads), 0, s, p);
    else launch_kernel(&segment_head_kernel<16>, dim3((unsigned)tiles), dim3(kSegThreads), 0, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// ---- clip maximum ----------------------------------------------------------------------------------------------------------
template <bool VAR>
__global__ __launch_bounds__(256) void segment_clipmax_kernel(const float* __restrict__ probs, int S_, int N, int nblk,
                                                              float* __restrict__ clip, const int* __restrict__ roff3) {
    const long long b = blockIdx.x / nblk;
    const int n = (int)(blockIdx.x % nblk) * 256 + threadIdx.x;
    if (n >= N) return;
    const int S = VAR ? roff3[b + 1] - roff3[b] : S_;
    const long long row0 = VAR ? (long long)roff3[b] : b * (long long)S;
    const float* q = probs + row0 * N + n;
    float m = -INFINITY;
    for (int t = 0; t < S; ++t) m = fmaxf(m, q[(long long)t * N]);
    clip[b * N + n] = m;
}

int launch_segment_clipmax(const float* probs, int B, int S, int N, float* clip, const int* roff3, hipStream_t s) {
    const int nblk = (N + 255) / 256;
    const long long blocks = (long long)B * nblk;
    if (blocks < 1 || blocks > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "segments: %d clips x %d classes is not a launchable grid", B, N);
    if (roff3) launch_kernel(&segment_clipmax_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, probs, 0, N, nblk, clip, roff3);
    else launch_kernel(&segment_clipmax_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, probs, S, N, nblk, clip, (const int*)nullptr);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// ---- frame expansion -------------------------------------------------------------------------------------------------------
// The output is one flat array of (frames x N) floats; a thread writes four consecutive ones with one 16-byte store (the array
// starts 16-byte aligned; rows of N floats need not).  It finds (clip, frame, class) of its first element once and steps from
// there.  VAR: packed clips, lengths by value; the frame / segment offsets of the clips are a serial prefix by one thread.
struct SegOffs {
    long long foff[kVarMaxClips + 1];       // first frame of clip b
    long long roff[kVarMaxClips + 1];       // first segment of clip b
};

template <bool VAR>
__global__ __launch_bounds__(256) void segment_expand_kernel(PackedLens a, const float* __restrict__ probs, int S_, int N, int T_,
                                                             long long total, float* __restrict__ out) {
    __shared__ SegOffs o;
    if (VAR) {
        if (threadIdx.x == 0) {
            packed_prefix(a.n, o.foff, [&a](int b) { return (long long)(a.len[b] / kHop + 1); });
            packed_prefix(a.n, o.roff, [&a](int b) { return (long long)seg_count(a.len[b]); });
        }
        __syncthreads();
    }
    for (long long g = (blockIdx.x * 256ll + threadIdx.x) * 4; g < total; g += (long long)gridDim.x * 256 * 4) {
        const long long uf = g / N;                 // frame, counted over all clips
        int n = (int)(g - uf * N);
        long long b = VAR ? packed_find(o.foff, a.n, uf) : uf / T_;
        int T = VAR ? (int)(o.foff[b + 1] - o.foff[b]) : T_;
        int S = VAR ? (int)(o.roff[b + 1] - o.roff[b]) : S_;
        long long row0 = VAR ? o.roff[b] : b * (long long)S;
        int u = (int)(uf - (VAR ? o.foff[b] : b * (long long)T));
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0.f;
            if (g + j < total) {
                const int seg = (u >> 5) < S - 1 ? (u >> 5) : S - 1;
                v[j] = probs[(row0 + seg) * N + n];
                if (++n == N) {
                    n = 0;
                    if (++u == T) {
                        u = 0; ++b;
                        if (VAR) {
                            if (b < a.n) { T = (int)(o.foff[b + 1] - o.foff[b]); S = (int)(o.roff[b + 1] - o.roff[b]); row0 = o.roff[b]; }
                        } else {
                            row0 += S;
                        }
                    }
                }
            }
        }
        if (g + 3 < total) {
            *reinterpret_cast<float4*>(out + g) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; g + j < total; ++j) out[g + j] = v[j];
        }
    }
}

static int expand_launch(bool var, const PackedLens& a, const float* probs, int S, int N, int T, long long total, float* frame,
                         hipStream_t s) {
    if (reinterpret_cast<uintptr_t>(frame) & 15) ACX_FAIL(ACX_ERR_ARG, "acx_segment_expand: frame must be 16-byte aligned");
    long long blocks = (total / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 16384) blocks = 16384;
    if (var) launch_kernel(&segment_expand_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a, probs, S, N, T, total, frame);
    else launch_kernel(&segment_expand_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a, probs, S, N, T, total, frame);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int launch_segment_expand(const float* probs, int B, int S, int N, int T, float* frame, hipStream_t s) {
    return expand_launch(false, PackedLens{}, probs, S, N, T, (long long)B * T * N, frame, s);
}

int launch_segment_expand_varlen(const float* probs, const int64_t* lengths, int B, int N, float* frame, hipStream_t s) {
    long long foff[kVarMaxClips + 1];
    const long long frames = packed_prefix(B, foff, [lengths](int b) { return (long long)(lengths[b] / kHop + 1); });
    return expand_launch(true, packed_lens(lengths, B), probs, 0, N, 0, frames * N, frame, s);
}

}  // namespace acx
