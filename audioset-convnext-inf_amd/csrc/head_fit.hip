// Training a classifier head on frozen scene embeddings (acx_head_fit_step / acx_head_fit_grad / acx_adam_update, include/acx.h):
// what the reference's fine-tuning loop does to `head_audioset` with the base frozen (pytorch/finetune_audiocaps.py: BCELoss on
// clipwise_output, optim.Adam(amsgrad=True); pytorch/main.py:648 uses AdamW the same way), without autograd and without the
// backbone: the head reads norm(pool(x)) (convnext.py:285,321), which never changes while the backbone is frozen.
//
// One optimisation step on a mini-batch of `rows` embeddings E[idx[r]] (K = 768) for a head of N classes is two launches:
//   fit_grad_kernel   tiles of S rows x S classes: z = E[idx] W^T + b, p = sigmoid(z), G = (p - y) / (rows N) -> workspace,
//                     and the tile's partial of the loss  -[y max(log p, -100) + (1 - y) max(log(1 - p), -100)]
//                     (torch's binary_cross_entropy with its -100 clamp; the mean's 1 / (rows N) is applied once, to the sum).
//   fit_update_kernel tiles of S classes x S of the 768 inputs: dW = G^T E[idx] over K = rows.  Every element of dW has exactly
//                     one owner thread, which applies Adam / AdamW to W, m, v, vmax in place: dW never goes to memory.  The
//                     blocks behind the tiles reduce db = sum_rows G (64 classes each) and update b; the last block adds the
//                     loss partials in index order and writes the step's loss.  Stream order keeps these writes of W behind
//                     the gradient kernel's reads.
// The batch rows are gathered through idx in both kernels: no shuffled copy of the data set exists.
//
// Cross-entropy (acx_head_fit_step_ce / acx_head_fit_grad_ce: a single-label head, integer labels, F.cross_entropy with
// label_smoothing, reduction mean) is three launches:
//   fit_logits_kernel  the tile body of fit_grad_kernel with the loss taken out (fit_grad_tile<S, kLossCe>): z -> workspace.
//   fit_ce_row_kernel  per row: m = max z, s = sum expf(z - m), G = (expf(z - m) / s - q) / rows with q = (1 - eps) [c = y] +
//                      eps / N, and the row's loss log s + sum_c q_c (m - z_c) (= m + log s - sum_c q_c z_c, written so
//                      that every term is >= 0 and a one-class row gives 0 exactly) -> part[row].
//                      Which shape runs when: N <= 2048 (kSoftWaveMaxN): one WAVE per row, four rows per workgroup, so a
//                      50-class head with 64 rows is 16 full workgroups; wider rows: one WORKGROUP per row.  Either way a
//                      thread adds its elements in ascending order, then the lanes by the xor butterfly, then (workgroup
//                      shape) the four waves in order: depth D = ceil(N / 64) + 6, or ceil(N / 256) + 9, a function of N alone.
//                      The row is NOT staged in LDS: it is read three times (max, sum, G); the first pass brings it into
//                      the XCD's L2 (4 MiB; a 32 768-class row is 128 KiB, a 527-class one 2 KiB and stays in L1), the other
//                      two hit there.  Holding a wide row in LDS would cost 128 of a CU's 160 KiB -- one workgroup per CU and
//                      no latency hiding -- to save L2 hits.  No atomics on floats; a row's G (at equal rows) depends on that row's z
//                      and label alone, and so do the row's z bits: the logits launch picks its tile shape from N, not rows.
//   fit_update_kernel  exactly as for BCE: it consumes G, adds part[0 .. rows) in index order and scales by 1 / rows.
//
// Groups (acx_head_fit_group_step / _step_ce): up to ACX_FIT_MAX_JOBS independent fits over the same E advance per launch.  The
// bodies above are device functions that take the tile (or row) number as an argument; the single-call kernels pass blockIdx.x,
// the group kernels resolve (tile, job) = (blockIdx.x, blockIdx.y) first and build the same parameter struct from the job table
// and the step's plan row, so a job's bits are its single call's (see "groups" below).
//
// Arithmetic: fp32 products, fp32 accumulation on the f32-input matrix cores (v_mfma_f32_32x32x2_f32 when the launch has
// at least one 32 x 32 tile per CU, v_mfma_f32_16x16x4_f32 otherwise, so that a 50-class head with 64 rows still spreads over
// 16 + 192 workgroups) -- bit-equal to an fmaf chain.  The four waves of a workgroup split the contraction (K = 768 or the rows)
// four ways and their partial tiles are added in wave order through LDS; nothing is accumulated with atomics, so the same
// inputs give the same bits on every run.  model.set_precision() has no influence here: training state is fp32.
//
// The gradient of the logits is the exact (sigmoid(z) - y) / (rows N) -- the BCEWithLogitsLoss form.  The reference's
// sigmoid-then-BCELoss product form equals it except where the fp32 sigmoid saturates (|z| >~ 16.6: p rounds to 0 or 1,
// log(1 - p) hits the clamp and autograd returns 0 for that logit); this kernel keeps the exact gradient there.
//
// Optimiser: torch.optim.Adam / AdamW, single-tensor form, step t = 1, 2, ...:
//   g <- g + wd p (Adam)  or  p <- p (1 - lr wd) (AdamW);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;
//   amsgrad: vmax <- max(vmax, v), used for v below;  p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// eps sits outside the root, after the bias correction.  What depends only on the hyper-parameters and t is evaluated on the
// host in double and rounded to fp32 once (adam_scalars); the decay and the step are applied to p in ONE fused multiply-add.
#include <cmath>
#include <vector>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kFitK = 768;                        // inputs of the head (convnext.py:656, dims[-1])
constexpr int kFitThreads = 256;                  // four waves: the contraction is split four ways
constexpr int kFitDbCols = 64;                    // classes per db block
constexpr long long kFitMaxRows = 1LL << 22;

// The tile form of a matrix launch: 32 x 32 where that still leaves every CU a tile, 16 x 16 otherwise.  The BCE gradient pass
// asks fit_rows_wide, the cross-entropy logits and every update pass fit_classes_wide (fit_ce_launch says why).  The two forms add
// the products in different orders, so these are part of the bit contract: the single calls evaluate them on the host, the group
// kernels per job on the device.
__host__ __device__ inline bool fit_rows_wide(int rows, int N, int cus) { return (long long)((rows + 31) / 32) * ((N + 31) / 32) >= cus; }
__host__ __device__ inline bool fit_classes_wide(int N, int cus) { return ((N + 31) / 32) * (kFitK / 32) >= cus; }

struct AdamK {          // fp32 roundings of the host's double evaluations
    float beta1, omb1, beta2, omb2, eps, wd, decay, step_size, bc2_sqrt;
    int amsgrad;
};

// One element of the update.  Contraction is off and the fused operations are spelled out: the fused step and
// acx_adam_update run this function in different kernels and must produce the same bits.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float* vmax, const AdamK& a) {
#pragma clang fp contract(off)
    const float p0 = p;
    g = __builtin_fmaf(a.wd, p0, g);                              // Adam: wd p added to the gradient (a.wd = 0 for AdamW)
    const float mn = __builtin_fmaf(a.beta1, m, a.omb1 * g);
    const float vn = __builtin_fmaf(a.beta2, v, a.omb2 * (g * g));
    float vv = vn;
    if (a.amsgrad) {
        vv = fmaxf(*vmax, vn);
        *vmax = vv;
    }
    const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
    const float upd = a.step_size * (mn / denom);
    m = mn;
    v = vn;
    p = __builtin_fmaf(p0, a.decay, -upd);                        // AdamW: decay = 1 - lr wd; Adam: 1
}

// F32Tile (device_common.h) + the accumulators an S x S tile alternates between, MFMA by MFMA
template <int S> struct FitTile : F32Tile<S> {
    static constexpr int NACC = S == 16 ? 2 : 1;   // 16 x 16: the dependent latency (40) exceeds the issue interval (32)
};

// the wave's accumulators, added -> red (tile_spill)
template <int S>
__device__ __forceinline__ void fit_spill(const typename FitTile<S>::acc_t* acc, float* red, int lane) {
    using T = FitTile<S>;
    tile_spill<S>([&](int i) {
        float v = acc[0][i];
        if (T::NACC == 2) v += acc[T::NACC - 1][i];
        return v;
    }, red, lane % S, lane / S);
}

struct FitGradP {
    const float* E; long long ld_e; long long n_total;
    const void* Y; int y_u8; long long ld_y;
    const long long* idx; int rows; int N;
    const float* W; const float* b;
    float* z;            // optional (rows, N)
    float* G;            // (rows, N)
    float* part;         // [gridDim.x] loss partials
    int* status; float inv; int tiles_n;
};

enum { kLossBce = 0, kLossCe = 1 };

// sigmoid(z) from ex = exp(-|z|): 1 / (1 + ex) or ex / (1 + ex), never an overflow (the gradient pass and the bag pass)
__device__ __forceinline__ float fit_sigmoid(float zz, float ex) { return (zz >= 0.f ? 1.f : ex) / (1.f + ex); }

// The tile body of the gradient pass.  LOSS = kLossBce: the whole of fit_grad_kernel.  LOSS = kLossCe: the logits alone go
// to p.z (the softmax needs whole rows: fit_ce_row_kernel); Y, G, part and inv are not read.  bid: the tile's number in p's own
// tiling (blockIdx.x in a single call; a group's block resolves its job first).
template <int S, int LOSS>
__device__ __forceinline__ void fit_grad_tile(const FitGradP& p, unsigned bid) {
    using T = FitTile<S>;
    constexpr int KB = (64 / S) * 4;               // k per block of four MFMAs: lane group h holds k = 4 h .. 4 h + 3
    constexpr int KW = kFitK / 4;                  // k per wave
    __shared__ float red[4][S * S];
    __shared__ long long s_idx[S];
    __shared__ float s_loss[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane % S, h = lane / S;
    const int tile_c = bid % p.tiles_n, tile_r = bid / p.tiles_n;
    const int row0 = tile_r * S, c0 = tile_c * S;

    // rows past the batch and classes past N repeat the last valid one: loads stay inside the buffers, results are dropped
    long long src = p.idx[min(row0 + r, p.rows - 1)];
    const bool bad = src < 0 || src >= p.n_total;
    src = src < 0 ? 0 : src >= p.n_total ? p.n_total - 1 : src;
    if (wave == 0 && h == 0) {
        s_idx[r] = src;
        if (__ballot(bad) && lane == 0) atomicOr(p.status, ACX_FIT_BAD_INDEX);
    }
    const float* ea = p.E + src * p.ld_e + wave * KW + 4 * h;
    const float* wb = p.W + (long long)min(c0 + r, p.N - 1) * kFitK + wave * KW + 4 * h;

    typename T::acc_t acc[T::NACC];
#pragma unroll
    for (int a = 0; a < T::NACC; ++a)
#pragma unroll
        for (int i = 0; i < T::REGS; ++i) acc[a][i] = 0.f;
#pragma unroll 4
    for (int kb = 0; kb < KW / KB; ++kb) {
        const float4 av = *reinterpret_cast<const float4*>(ea + kb * KB);
        const float4 bv = *reinterpret_cast<const float4*>(wb + kb * KB);
        acc[0] = T::mfma(av.x, bv.x, acc[0]);
        acc[T::NACC - 1] = T::mfma(av.y, bv.y, acc[T::NACC - 1]);
        acc[0] = T::mfma(av.z, bv.z, acc[0]);
        acc[T::NACC - 1] = T::mfma(av.w, bv.w, acc[T::NACC - 1]);
    }
    fit_spill<S>(acc, red[wave], lane);
    __syncthreads();

    float lsum = 0.f;
#pragma unroll
    for (int q = 0; q < S * S / kFitThreads; ++q) {
        const int e = tid + kFitThreads * q;
        const int rr = e / S, cc = e % S;
        const int row = row0 + rr, c = c0 + cc;
        if (row < p.rows && c < p.N) {
            const float zz = tile_sum4(red, e) + p.b[c];
            if (LOSS == kLossCe) {
                p.z[(long long)row * p.N + c] = zz;
                continue;
            }
            const long long yo = s_idx[rr] * p.ld_y + c;
            const float y = p.y_u8 ? (static_cast<const unsigned char*>(p.Y)[yo] ? 1.f : 0.f) : static_cast<const float*>(p.Y)[yo];
            // sigmoid and both logarithms from e = exp(-|z|): log p = min(z, 0) - log1p(e), log(1 - p) = min(-z, 0) - log1p(e)
            const float ex = expf(-fabsf(zz));
            const float pr = fit_sigmoid(zz, ex);
            const float l1 = log1pf(ex);
            const float lp = fmaxf(fminf(zz, 0.f) - l1, -100.f), lq = fmaxf(fminf(-zz, 0.f) - l1, -100.f);
            lsum -= y * lp + (1.f - y) * lq;
            const long long o = (long long)row * p.N + c;
            p.G[o] = (pr - y) * p.inv;
            if (p.z) p.z[o] = zz;
        }
    }
    if (LOSS == kLossCe) return;
    lsum = wave_sum(lsum);
    if (lane == 0) s_loss[wave] = lsum;
    __syncthreads();
    if (tid == 0) p.part[bid] = sum4(s_loss[0], s_loss[1], s_loss[2], s_loss[3]);
}

template <int S>
__global__ __launch_bounds__(kFitThreads) void fit_grad_kernel(FitGradP p) { fit_grad_tile<S, kLossBce>(p, blockIdx.x); }
template <int S>
__global__ __launch_bounds__(kFitThreads) void fit_logits_kernel(FitGradP p) { fit_grad_tile<S, kLossCe>(p, blockIdx.x); }

// The row pass of the cross-entropy step: G and the row's loss from the logits z (rows, N), one group of W threads per row
// (device_common.h, "softmax of one row").  label = labels[idx[r]], both clamped into their ranges.
struct FitCeRowP {
    const float* z; const long long* labels; const long long* idx; long long n_total; int rows; int N;
    float q_hit, q_miss, ome;      // fp32 roundings of (1 - eps) + eps / N, eps / N and 1 - eps
    float inv;                     // 1 / rows
    float* G; float* part; int* status;
};

template <int W>
__device__ __forceinline__ void fit_ce_row_body(const FitCeRowP& p, int bid) {
    __shared__ float red[4];
    const int t = soft_thread<W>();
    const int row = W == 64 ? (int)(bid * 4 + (threadIdx.x >> 6)) : bid;
    if (row >= p.rows) return;                                     // W = 64 only: a whole wave, and no barrier follows
    long long src = p.idx[row];
    src = src < 0 ? 0 : src >= p.n_total ? p.n_total - 1 : src;    // flagged by the logits kernel
    long long y = p.labels[src];
    if (y < 0 || y >= p.N) {
        if (t == 0) atomicOr(p.status, ACX_FIT_BAD_LABEL);
        y = y < 0 ? 0 : p.N - 1;
    }
    const float* z = p.z + (long long)row * p.N;
    float* g = p.G + (long long)row * p.N;
    float m, s;
    soft_row_stats<W>(z, p.N, red, m, s);
    // sum_c q_c (m - z_c) = q_miss sum_c (m - z_c) + (1 - eps) (m - z_y): with sum_c q_c = 1 this is m - sum_c q_c z_c, every
    // term >= 0, and a one-class row gives 0 exactly
    float d = 0.f;
    for (int c = t; c < p.N; c += W) {
        const float zc = z[c];
        d += m - zc;
        g[c] = (soft_prob(zc, m, s) - (c == (int)y ? p.q_hit : p.q_miss)) * p.inv;
    }
    d = group_sum<W>(d, red);
    if (t == 0) p.part[row] = logf(s) + (p.q_miss * d + p.ome * (m - z[y]));
}

template <int W>
__global__ __launch_bounds__(kFitThreads) void fit_ce_row_kernel(FitCeRowP p) { fit_ce_row_body<W>(p, blockIdx.x); }

struct FitUpdP {
    const float* E; long long ld_e; long long n_total;
    const long long* idx; int rows; int N;
    const float* G;
    float *W, *mW, *vW, *vmaxW;        // APPLY
    float *b, *mb, *vb, *vmaxb;
    float *dW, *db;                    // !APPLY
    const float* part; int nparts; float* loss; float inv;
    AdamK a;
    int tiles;                         // ceil(N / S) * (768 / S); then ceil(N / 64) db blocks; then the loss block
};

template <int S, bool APPLY>
__device__ __forceinline__ void fit_update_body(const FitUpdP& p, int bid) {
    using T = FitTile<S>;
    constexpr int KB = (64 / S) * 4;               // batch rows per block of four MFMAs
    constexpr int TK = kFitK / S;
    __shared__ float red[4][S * S];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    if (bid < p.tiles) {
        const int r = lane % S, h = lane / S;
        const int c0 = (bid / TK) * S, k0 = (bid % TK) * S;
        const float* gcol = p.G + min(c0 + r, p.N - 1);       // A[m = class][k = row] = G[row][class]
        const float* ecol = p.E + k0 + r;                     // B[k = row][n = input] = E[idx[row]][input]
        const int nblk = (p.rows + KB - 1) / KB, per = (nblk + 3) / 4;
        const int b_lo = wave * per, b_hi = min(nblk, b_lo + per);
        typename T::acc_t acc[T::NACC];
#pragma unroll
        for (int a = 0; a < T::NACC; ++a)
#pragma unroll
            for (int i = 0; i < T::REGS; ++i) acc[a][i] = 0.f;
        for (int blk = b_lo; blk < b_hi; ++blk) {
            float gv[4], ev[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = blk * KB + 4 * h + j;
                const bool in = row < p.rows;
                long long src = p.idx[in ? row : p.rows - 1];
                src = src < 0 ? 0 : src >= p.n_total ? p.n_total - 1 : src;
                const float g = gcol[(long long)(in ? row : p.rows - 1) * p.N];
                const float e = ecol[src * p.ld_e];
                gv[j] = in ? g : 0.f;
                ev[j] = in ? e : 0.f;
            }
            acc[0] = T::mfma(gv[0], ev[0], acc[0]);
            acc[T::NACC - 1] = T::mfma(gv[1], ev[1], acc[T::NACC - 1]);
            acc[0] = T::mfma(gv[2], ev[2], acc[0]);
            acc[T::NACC - 1] = T::mfma(gv[3], ev[3], acc[T::NACC - 1]);
        }
        fit_spill<S>(acc, red[wave], lane);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < S * S / kFitThreads; ++q) {
            const int e = tid + kFitThreads * q;
            const int c = c0 + e / S, k = k0 + e % S;
            if (c < p.N) {
                const float dw = tile_sum4(red, e);
                const long long o = (long long)c * kFitK + k;
                if (APPLY) {
                    float w = p.W[o], m = p.mW[o], v = p.vW[o];
                    adam_elem(w, dw, m, v, p.a.amsgrad ? p.vmaxW + o : nullptr, p.a);
                    p.W[o] = w; p.mW[o] = m; p.vW[o] = v;
                } else {
                    p.dW[o] = dw;
                }
            }
        }
        return;
    }
    const int ndb = (p.N + kFitDbCols - 1) / kFitDbCols;
    if (bid < p.tiles + ndb) {                                     // db of 64 classes: four row quarters, added in order
        const int c = (bid - p.tiles) * kFitDbCols + lane;
        const int per = (p.rows + 3) / 4;
        const int r_lo = wave * per, r_hi = min(p.rows, r_lo + per);
        float s = 0.f;
        if (c < p.N)
            for (int row = r_lo; row < r_hi; ++row) s += p.G[(long long)row * p.N + c];
        red[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && c < p.N) {
            const float d = tile_sum4(red, lane);
            if (APPLY) {
                float w = p.b[c], m = p.mb[c], v = p.vb[c];
                adam_elem(w, d, m, v, p.a.amsgrad ? p.vmaxb + c : nullptr, p.a);
                p.b[c] = w; p.mb[c] = m; p.vb[c] = v;
            } else {
                p.db[c] = d;
            }
        }
        return;
    }
    // the loss: partials in index order per thread, threads by the shuffle tree, waves in order
    float s = 0.f;
    for (int i = tid; i < p.nparts; i += kFitThreads) s += p.part[i];
    s = wave_sum(s);
    if (lane == 0) red[0][wave] = s;
    __syncthreads();
    if (tid == 0) *p.loss = sum4(red[0][0], red[0][1], red[0][2], red[0][3]) * p.inv;
}

template <int S, bool APPLY>
__global__ __launch_bounds__(kFitThreads) void fit_update_kernel(FitUpdP p) { fit_update_body<S, APPLY>(p, blockIdx.x); }

__global__ __launch_bounds__(256) void adam_update_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                          float* __restrict__ m, float* __restrict__ v, float* vmax,
                                                          long long n, AdamK a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float w = param[i], mm = m[i], vv = v[i];
    adam_elem(w, grad[i], mm, vv, a.amsgrad ? vmax + i : nullptr, a);
    param[i] = w; m[i] = mm; v[i] = vv;
}

// ---- weak labels: the bag pass of acx_head_fit_step_mil / acx_head_fit_grad_mil, and acx_segment_pool ----------------------------
// A clip is a bag of S segments and only the clip has a label (include/acx.h, "sound event detection heads from clip-level
// labels").  Between the logits launch (fit_logits_kernel on idx = seg_idx) and the update launch (fit_update_kernel on the same
// rows) this pass turns z (seg_rows, N) into G (seg_rows, N), the pooled P (bags, N) and one loss partial per item.
// An item is (bag, chunk of 64 consecutive classes), owned by ONE WAVE, four items per workgroup: lane l walks the column of class
// 64 chunk + l over the bag's rows twice -- statistics, then G -- in ascending t.  A row's read is one coalesced 256-byte line per
// wave; a lane's sums depend on its own column alone: no LDS, no barrier, no atomics on floats, the same bits on every run.  The
// column is not staged in LDS, because S has no bound (an hour-long recording is 11 250 segments).  The second walk re-reads what
// the first one brought in: a 64-bag step of 31 segments and 527 classes is 4 MiB of z in all, an XCD's L2; the columns of an
// hour-long bag (2.8 MiB per chunk, eight chunks in flight) come back from the Infinity Cache instead.  With 576 waves for such a
// step occupancy is no concern (24 .. 32 VGPRs, no scratch); what hides the latency of the walks is kMilAhead independent row
// loads in flight per lane, while the arithmetic stays in t order.  "max" needs no second read: one row of a column has a gradient.
// GRAD = false is the forward alone (acx_segment_pool): the same functions, the same P.
constexpr int kMilAhead = 8;
enum { kMilMax = ACX_MIL_MAX, kMilMean = ACX_MIL_MEAN, kMilLinear = ACX_MIL_LINEAR, kMilExp = ACX_MIL_EXP };

struct FitMilP {
    const float* z; long long ld_z;                    // (seg_rows, classes) logits
    const int* bag_off; int bags; int seg_rows;        // bag i: rows [bag_off[i], bag_off[i + 1]); seg_rows: the bound of the clamp
    int N; int chunks;                                 // chunks = ceil(N / 64)
    float* P; long long ld_p;                          // (bags, classes)
    // GRAD only
    const void* Y; int y_u8; long long ld_y; long long n_bags; const long long* bag_idx;
    float* G; float* part; float inv;
    int* status;
};

// Row t of a lane's column joins its running statistics (a, b, ts): MAX: a = the maximum so far and ts the FIRST row that attains
// it; MEAN: a = sum q; LINEAR: a = sum q, b = sum q q; EXP: a = sum e^q, b = sum q e^q.  Every product is rounded before it is added.
template <int POOL>
__device__ __forceinline__ void mil_accumulate(float zt, int t, float& a, float& b, int& ts) {
#pragma clang fp contract(off)
    if (POOL == kMilMax) {
        if (zt > a) { a = zt; ts = t; }
        return;
    }
    const float q = fit_sigmoid(zt, expf(-fabsf(zt)));
    if (POOL == kMilMean) {
        a += q;
    } else if (POOL == kMilLinear) {
        a += q;
        b += q * q;
    } else {
        const float e = expf(q);
        a += e;
        b += q * e;
    }
}

// The pooled probability of a bag of S rows from its statistics.  Termwise q q <= q and q e^q <= e^q and both sums run in the
// same order, so b <= a and P <= 1 in fp32 as well.
template <int POOL>
__device__ __forceinline__ float mil_pooled(float a, float b, int S) {
    if (S == 0) return 0.f;
    if (POOL == kMilMax) return fit_sigmoid(a, expf(-fabsf(a)));
    if (POOL == kMilMean) return a / (float)S;
    return a == 0.f ? 0.f : b / a;                     // LINEAR: every q underflowed; EXP: a >= S
}

// G of row t: dL/dP dP/dq_t q_t (1 - q_t) inv, the products taken from the left.
template <int POOL>
__device__ __forceinline__ float mil_grad_elem(float zt, float a, float P, float dLdP, float invS, float inv) {
#pragma clang fp contract(off)
    const float q = fit_sigmoid(zt, expf(-fabsf(zt)));
    float d;
    if (POOL == kMilMax) {
        d = 1.f;
    } else if (POOL == kMilMean) {
        d = invS;
    } else if (POOL == kMilLinear) {
        d = a == 0.f ? 0.f : (2.f * q - P) / a;
    } else {
        d = expf(q) * ((1.f + q) - P) / a;
    }
    return ((dLdP * d) * (q * (1.f - q))) * inv;
}

template <int POOL, bool GRAD>
__global__ __launch_bounds__(kFitThreads) void fit_mil_bag_kernel(FitMilP p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long item = (long long)blockIdx.x * 4 + wave;
    if (item >= (long long)p.bags * p.chunks) return;              // a whole wave, and no barrier follows
    const int bag = (int)(item / p.chunks), chunk = (int)(item % p.chunks);
    const int c = chunk * 64 + lane;
    const bool live = c < p.N;
    const int cc = live ? c : p.N - 1;                             // lanes past N repeat the last class: loads stay inside z

    // the bag's rows, held inside [0, seg_rows] and in order; a gradient pass covers every row of G whatever bag_off holds: the
    // first bag starts at 0, the last one ends at seg_rows
    int lo = p.bag_off[bag], hi = p.bag_off[bag + 1];
    bool bad = lo < 0 || lo > p.seg_rows || hi < lo || hi > p.seg_rows;
    lo = min(max(lo, 0), p.seg_rows);
    hi = min(max(hi, lo), p.seg_rows);
    if (GRAD) {
        if (bag == 0 && lo != 0) { bad = true; lo = 0; }
        if (bag == p.bags - 1 && hi != p.seg_rows) { bad = true; hi = p.seg_rows; }
    }
    if (bad && chunk == 0 && lane == 0) atomicOr(p.status, ACX_FIT_BAD_BAG);
    const int S = hi - lo;

    const float* __restrict__ zc = p.z + cc;
    float a = POOL == kMilMax ? -__builtin_inff() : 0.f, b = 0.f;
    int ts = lo;
    int t = lo;
    // groups of kMilAhead rows: every load is issued (rows past the bag repeat its last one) before the first is used; the rows
    // past the bag are left out of the arithmetic by a wave-uniform test, so a short last group costs one round trip, not one per row
    for (; t < hi; t += kMilAhead) {
        float v[kMilAhead];
#pragma unroll
        for (int j = 0; j < kMilAhead; ++j) v[j] = zc[(long long)min(t + j, hi - 1) * p.ld_z];
#pragma unroll
        for (int j = 0; j < kMilAhead; ++j)
            if (t + j < hi) mil_accumulate<POOL>(v[j], t + j, a, b, ts);
    }
    const float P = mil_pooled<POOL>(a, b, S);
    if (live) p.P[(long long)bag * p.ld_p + c] = P;
    if (!GRAD) return;

    long long yb = p.bag_idx[bag];
    if (yb < 0 || yb >= p.n_bags) {
        if (chunk == 0 && lane == 0) atomicOr(p.status, ACX_FIT_BAD_INDEX);
        yb = yb < 0 ? 0 : p.n_bags - 1;
    }
    const long long yo = yb * p.ld_y + cc;
    const float y = p.y_u8 ? (static_cast<const unsigned char*>(p.Y)[yo] ? 1.f : 0.f) : static_cast<const float*>(p.Y)[yo];
    // torch's binary_cross_entropy on a probability, and its backward: both logarithms held at -100, P (1 - P) at 1e-12
    const float lp = fmaxf(logf(P), -100.f), lq = fmaxf(log1pf(-P), -100.f);
    float l = live ? -(y * lp + (1.f - y) * lq) : 0.f;
    l = wave_sum(l);
    if (lane == 0) p.part[item] = l;
    const float dLdP = (P - y) / fmaxf(P * (1.f - P), 1e-12f);
    const float invS = 1.f / (float)max(S, 1);

    float* __restrict__ gc = p.G + c;
    if (POOL == kMilMax) {                                         // one row of the column has a gradient: no second read
        const float g = S ? mil_grad_elem<POOL>(a, a, P, dLdP, invS, p.inv) : 0.f;
        if (live)
            for (t = lo; t < hi; ++t) gc[(long long)t * p.N] = t == ts ? g : 0.f;
        return;
    }
    t = lo;
    for (; t < hi; t += kMilAhead) {
        float v[kMilAhead];
#pragma unroll
        for (int j = 0; j < kMilAhead; ++j) v[j] = zc[(long long)min(t + j, hi - 1) * p.ld_z];
#pragma unroll
        for (int j = 0; j < kMilAhead; ++j) {
            const float g = mil_grad_elem<POOL>(v[j], a, P, dLdP, invS, p.inv);
            if (live && t + j < hi) gc[(long long)(t + j) * p.N] = g;
        }
    }
}

// ---- groups: J independent fits over the same embeddings, one launch per stage for all of them (acx_head_fit_group_step) -----
// A block is (tile, job) = (blockIdx.x, blockIdx.y): it reads the job's pointers (acx_fit_job) and its entry of the step's plan row
// (rows, idx offset, loss slot, 1 / count and the AdamK scalars, all evaluated on the host by acx_head_fit_plan_fill with the
// single call's own code), builds the single call's parameter struct and runs the single call's body.  The grid is sized for
// rows_max; blocks past the job's own tiling, blocks of a job that sits the step out (rows = 0) and -- BCE gradient pass, where the
// form depends on the job's rows -- blocks of the other tile form return before the first barrier.  Nothing of an idle job is
// written.  Each job owns a slice of the workspace laid out as the single call's.
struct FitPlanE {       // one (step, job) entry of the plan
    long long idx_off;  // the batch is idx[idx_off .. idx_off + rows) of the job's index array
    int rows;           // 0: the job sits this step out
    int loss_slot;      // the job's step count before this step (t - 1): loss[loss_slot] receives the step's loss
    float inv;          // 1 / (rows classes) (BCE) or 1 / rows (cross-entropy), from double
    int pad;
    AdamK a;
};
static_assert(sizeof(FitPlanE) == 64, "plan entries are 64 bytes: acx_head_fit_plan_bytes");

struct FitGroupP {
    const float* E; long long ld_e; long long n_total;
    const void* Y; int y_u8; long long ld_y;           // the targets (BCE) or the int64 labels (cross-entropy)
    const acx_fit_job* jobs; const FitPlanE* plan;     // plan: the step's row of J entries
    int N, rows_max, cus, loss;
    char* ws; size_t ws_job, z_off, part_off;          // job j's slice starts at ws + j ws_job: G, then z (CE), then the partials
    int* status;                                       // [J]
    float q_hit, q_miss, ome;                          // cross-entropy: FitCeRowP's
};

template <int S, int LOSS>
__global__ __launch_bounds__(kFitThreads) void fit_group_grad_kernel(FitGroupP q) {
    const int j = blockIdx.y;
    const FitPlanE e = q.plan[j];
    const int rows = min(e.rows, q.rows_max);
    if (rows <= 0) return;
    if (LOSS == kLossBce && fit_rows_wide(rows, q.N, q.cus) != (S == 32)) return;
    const int tiles_n = (q.N + S - 1) / S;
    if ((int)blockIdx.x >= ((rows + S - 1) / S) * tiles_n) return;
    const acx_fit_job jb = q.jobs[j];
    char* w = q.ws + j * q.ws_job;
    FitGradP p;
    p.E = q.E; p.ld_e = q.ld_e; p.n_total = q.n_total;
    p.Y = q.Y; p.y_u8 = q.y_u8; p.ld_y = q.ld_y;
    p.idx = reinterpret_cast<const long long*>(jb.idx) + e.idx_off; p.rows = rows; p.N = q.N;
    p.W = jb.W; p.b = jb.b;
    p.z = LOSS == kLossCe ? reinterpret_cast<float*>(w + q.z_off) : nullptr;
    p.G = reinterpret_cast<float*>(w);
    p.part = reinterpret_cast<float*>(w + q.part_off);
    p.status = q.status + j; p.inv = e.inv; p.tiles_n = tiles_n;
    fit_grad_tile<S, LOSS>(p, blockIdx.x);
}

template <int W>
__global__ __launch_bounds__(kFitThreads) void fit_group_ce_row_kernel(FitGroupP q) {
    const int j = blockIdx.y;
    const FitPlanE e = q.plan[j];
    const int rows = min(e.rows, q.rows_max);
    if ((int)blockIdx.x * (W == 64 ? 4 : 1) >= rows) return;
    const acx_fit_job jb = q.jobs[j];
    char* w = q.ws + j * q.ws_job;
    FitCeRowP p;
    p.z = reinterpret_cast<const float*>(w + q.z_off); p.labels = static_cast<const long long*>(q.Y);
    p.idx = reinterpret_cast<const long long*>(jb.idx) + e.idx_off; p.n_total = q.n_total; p.rows = rows; p.N = q.N;
    p.q_hit = q.q_hit; p.q_miss = q.q_miss; p.ome = q.ome; p.inv = e.inv;
    p.G = reinterpret_cast<float*>(w); p.part = reinterpret_cast<float*>(w + q.part_off); p.status = q.status + j;
    fit_ce_row_body<W>(p, blockIdx.x);
}

template <int S>
__global__ __launch_bounds__(kFitThreads) void fit_group_update_kernel(FitGroupP q) {
    const int j = blockIdx.y;
    const FitPlanE e = q.plan[j];
    const int rows = min(e.rows, q.rows_max);
    if (rows <= 0) return;
    const acx_fit_job jb = q.jobs[j];
    char* w = q.ws + j * q.ws_job;
    FitUpdP p;
    p.E = q.E; p.ld_e = q.ld_e; p.n_total = q.n_total;
    p.idx = reinterpret_cast<const long long*>(jb.idx) + e.idx_off; p.rows = rows; p.N = q.N;
    p.G = reinterpret_cast<const float*>(w);
    p.W = jb.W; p.mW = jb.mW; p.vW = jb.vW; p.vmaxW = jb.vmaxW;
    p.b = jb.b; p.mb = jb.mb; p.vb = jb.vb; p.vmaxb = jb.vmaxb;
    p.dW = nullptr; p.db = nullptr;
    p.part = reinterpret_cast<const float*>(w + q.part_off);
    if (q.loss == kLossCe) {
        p.nparts = rows;                               // one partial per row
    } else {                                           // one per tile of the form the job's gradient pass took
        const int gs = fit_rows_wide(rows, q.N, q.cus) ? 32 : 16;
        p.nparts = ((rows + gs - 1) / gs) * ((q.N + gs - 1) / gs);
    }
    p.loss = jb.loss + e.loss_slot; p.inv = e.inv; p.a = e.a;
    p.tiles = ((q.N + S - 1) / S) * (kFitK / S);
    fit_update_body<S, true>(p, blockIdx.x);
}

// workspace: G (rows_max, classes) fp32, then the loss partials of the finest tiling (16 x 16)
static void fit_layout(long long rows, long long N, size_t* part_off, size_t* total) {
    const size_t gb = align_up((size_t)rows * N * 4);
    const size_t pb = align_up((size_t)((rows + 15) / 16) * ((N + 15) / 16) * 4);
    *part_off = gb;
    *total = gb + pb;
}

// cross-entropy workspace: G, z (rows_max, classes) fp32 each, then one loss partial per row
static void fit_ce_layout(long long rows, long long N, size_t* z_off, size_t* part_off, size_t* total) {
    const size_t gb = align_up((size_t)rows * N * 4);
    *z_off = gb;
    *part_off = 2 * gb;
    *total = 2 * gb + align_up((size_t)rows * 4);
}

static int fit_check_shape(const char* who, int64_t rows, int classes) {
    if (rows < 1) ACX_FAIL(ACX_ERR_ARG, "%s: rows = %lld (expected >= 1)", who, (long long)rows);
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "%s: classes = %d (expected 1 .. %d)", who, classes, ACX_MAX_CLASSES);
    if (rows > kFitMaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: rows = %lld (at most 2^22 per step)", who, (long long)rows);
    return ACX_OK;
}

static int adam_scalars(const char* who, const acx_adam* hp, int64_t t, double lr, AdamK* a) {
    if (!hp) ACX_FAIL(ACX_ERR_ARG, "%s: hp is null", who);
    if (!(hp->beta1 >= 0.0 && hp->beta1 < 1.0)) ACX_FAIL(ACX_ERR_ARG, "%s: hp->beta1 = %g (expected 0 <= beta1 < 1)", who, hp->beta1);
    if (!(hp->beta2 >= 0.0 && hp->beta2 < 1.0)) ACX_FAIL(ACX_ERR_ARG, "%s: hp->beta2 = %g (expected 0 <= beta2 < 1)", who, hp->beta2);
    if (!(hp->eps > 0.0) || !std::isfinite(hp->eps)) ACX_FAIL(ACX_ERR_ARG, "%s: hp->eps = %g (expected > 0)", who, hp->eps);
    if (!(hp->weight_decay >= 0.0) || !std::isfinite(hp->weight_decay))
        ACX_FAIL(ACX_ERR_ARG, "%s: hp->weight_decay = %g (expected >= 0)", who, hp->weight_decay);
    if (t < 1) ACX_FAIL(ACX_ERR_ARG, "%s: step_t = %lld (steps count from 1)", who, (long long)t);
    if (!(lr >= 0.0) || !std::isfinite(lr)) ACX_FAIL(ACX_ERR_ARG, "%s: lr = %g (expected >= 0)", who, lr);
    a->beta1 = (float)hp->beta1;
    a->omb1 = (float)(1.0 - hp->beta1);
    a->beta2 = (float)hp->beta2;
    a->omb2 = (float)(1.0 - hp->beta2);
    a->eps = (float)hp->eps;
    a->wd = hp->decoupled ? 0.f : (float)hp->weight_decay;
    a->decay = hp->decoupled ? (float)(1.0 - lr * hp->weight_decay) : 1.f;
    a->step_size = (float)(lr / (1.0 - std::pow(hp->beta1, (double)t)));
    a->bc2_sqrt = (float)std::sqrt(1.0 - std::pow(hp->beta2, (double)t));
    a->amsgrad = hp->amsgrad ? 1 : 0;
    return ACX_OK;
}

struct FitCall {        // the arguments a step and its component form share, for either loss
    const float* E; int64_t ld_e; int64_t n_total;
    const void* Y; const char* y_name;      // target (BCE) or labels (cross-entropy), and the name its null message prints
    int y_dtype; int64_t ld_y;              // BCE only
    double eps;                             // cross-entropy only: label_smoothing
    const int64_t* idx; int64_t rows; int classes; const float* W; const float* b; int32_t* status; void* ws; size_t ws_bytes;
};

// The checks of both losses, in two pieces: a loss has checks of its own between them, and its workspace check after them.
static int fit_check_pointers(const char* who, const FitCall& c) {
    if (!c.E) ACX_FAIL(ACX_ERR_ARG, "%s: E is null", who);
    if (!c.Y) ACX_FAIL(ACX_ERR_ARG, "%s: %s is null", who, c.y_name);
    if (!c.idx) ACX_FAIL(ACX_ERR_ARG, "%s: idx is null", who);
    if (!c.W) ACX_FAIL(ACX_ERR_ARG, "%s: W is null", who);
    if (!c.b) ACX_FAIL(ACX_ERR_ARG, "%s: b is null", who);
    if (!c.status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!c.ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    return ACX_OK;
}

static int fit_check_rows(const char* who, const FitCall& c) {
    ACX_TRY(fit_check_shape(who, c.rows, c.classes));
    if (c.n_total < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n_rows_total = %lld (expected >= 1)", who, (long long)c.n_total);
    if (c.ld_e < kFitK) ACX_FAIL(ACX_ERR_ARG, "%s: ld_e = %lld is shorter than a row of %d", who, (long long)c.ld_e, kFitK);
    if ((c.ld_e & 3) || (reinterpret_cast<uintptr_t>(c.E) & 15) || (reinterpret_cast<uintptr_t>(c.W) & 15))
        ACX_FAIL(ACX_ERR_ARG, "%s: E and W must be 16-byte aligned and ld_e a multiple of 4 (ld_e = %lld)", who, (long long)c.ld_e);
    return ACX_OK;
}

static int fit_check_call(const char* who, const FitCall& c, size_t* part_off) {
    ACX_TRY(fit_check_pointers(who, c));
    if (c.y_dtype != ACX_TARGET_F32 && c.y_dtype != ACX_TARGET_U8)
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, c.y_dtype);
    ACX_TRY(fit_check_rows(who, c));
    if (c.ld_y < c.classes)
        ACX_FAIL(ACX_ERR_ARG, "%s: ld_target = %lld is shorter than %d classes", who, (long long)c.ld_y, c.classes);
    size_t need;
    fit_layout(c.rows, c.classes, part_off, &need);
    return check_workspace_for(who, c.ws, c.ws_bytes, need);
}

static int fit_ce_check_call(const char* who, const FitCall& c, size_t* z_off, size_t* part_off) {
    ACX_TRY(fit_check_pointers(who, c));
    if (!(c.eps >= 0.0 && c.eps < 1.0)) ACX_FAIL(ACX_ERR_ARG, "%s: label_smoothing = %g (expected 0 <= label_smoothing < 1)", who, c.eps);
    ACX_TRY(fit_check_rows(who, c));
    size_t need;
    fit_ce_layout(c.rows, c.classes, z_off, part_off, &need);
    return check_workspace_for(who, c.ws, c.ws_bytes, need);
}

// What the two _step entries check after the call itself, and the APPLY half of the update's arguments.
static int fit_step_args(const char* who, float* W, float* b, float* mW, float* vW, float* vmaxW, float* mb, float* vb, float* vmaxb,
                         const acx_adam* hp, int64_t step_t, double lr, const float* loss_out, FitUpdP* u) {
    if (!mW || !vW || !mb || !vb) ACX_FAIL(ACX_ERR_ARG, "%s: a moment buffer (mW, vW, mb, vb) is null", who);
    if (!loss_out) ACX_FAIL(ACX_ERR_ARG, "%s: loss_out is null", who);
    ACX_TRY(adam_scalars(who, hp, step_t, lr, &u->a));
    if (hp->amsgrad && (!vmaxW || !vmaxb)) ACX_FAIL(ACX_ERR_ARG, "%s: vmaxW / vmaxb is null with hp->amsgrad set", who);
    u->W = W; u->mW = mW; u->vW = vW; u->vmaxW = vmaxW;
    u->b = b; u->mb = mb; u->vb = vb; u->vmaxb = vmaxb;
    return ACX_OK;
}

// The same for the two _grad entries: the !APPLY half.
static int fit_grad_args(const char* who, const float* z, const float* G, float* dW, float* db, const float* loss, FitUpdP* u) {
    if (!z || !G || !dW || !db || !loss) ACX_FAIL(ACX_ERR_ARG, "%s: an output (z, G, dW, db, loss) is null", who);
    u->dW = dW; u->db = db;
    return ACX_OK;
}

// The arguments of the first matrix launch that both losses set; BCE adds its targets, G, part and inv.
static FitGradP fit_grad_params(const FitCall& c, float* z) {
    FitGradP g{};
    g.E = c.E; g.ld_e = c.ld_e; g.n_total = c.n_total;
    g.idx = reinterpret_cast<const long long*>(c.idx); g.rows = (int)c.rows; g.N = c.classes;
    g.W = c.W; g.b = c.b; g.z = z; g.status = (int*)c.status;
    return g;
}

// The update launch both losses share: u holds its APPLY or !APPLY half (fit_step_args / fit_grad_args).
static int fit_launch_update(FitUpdP u, const FitCall& c, const float* G, const float* part, int nparts, float* loss, float inv,
                             int cus, bool apply, hipStream_t s) {
    const int N = c.classes;
    u.E = c.E; u.ld_e = c.ld_e; u.n_total = c.n_total; u.idx = reinterpret_cast<const long long*>(c.idx); u.rows = (int)c.rows;
    u.N = N; u.G = G; u.part = part; u.nparts = nparts; u.loss = loss; u.inv = inv;
    const bool u32 = fit_classes_wide(N, cus);
    const int us = u32 ? 32 : 16;
    u.tiles = ((N + us - 1) / us) * (kFitK / us);
    const dim3 grid(u.tiles + (N + kFitDbCols - 1) / kFitDbCols + 1);
    if (apply) {
        if (u32) launch_kernel(&fit_update_kernel<32, true>, grid, dim3(kFitThreads), 0, s, u);
        else launch_kernel(&fit_update_kernel<16, true>, grid, dim3(kFitThreads), 0, s, u);
    } else {
        if (u32) launch_kernel(&fit_update_kernel<32, false>, grid, dim3(kFitThreads), 0, s, u);
        else launch_kernel(&fit_update_kernel<16, false>, grid, dim3(kFitThreads), 0, s, u);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// The two launches.  apply: W, b and the moments updated in place (u.a set); otherwise dW / db written.  The tile shape of each
// launch depends on (rows, classes, CUs) alone, so the step and its component form run the same kernels.
static int fit_launch(const FitCall& c, float* z, float* G, float* part, const FitUpdP& u, bool apply, float* loss, hipStream_t s) {
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));
    const int rows = (int)c.rows, N = c.classes;
    const float inv = (float)(1.0 / ((double)rows * (double)N));
    FitGradP g = fit_grad_params(c, z);
    g.Y = c.Y; g.y_u8 = c.y_dtype == ACX_TARGET_U8; g.ld_y = c.ld_y;
    g.G = G; g.part = part; g.inv = inv;
    const bool g32 = fit_rows_wide(rows, N, cus);
    const int gs = g32 ? 32 : 16;
    g.tiles_n = (N + gs - 1) / gs;
    const int gtiles = ((rows + gs - 1) / gs) * g.tiles_n;
    if (g32) launch_kernel(&fit_grad_kernel<32>, dim3(gtiles), dim3(kFitThreads), 0, s, g);
    else launch_kernel(&fit_grad_kernel<16>, dim3(gtiles), dim3(kFitThreads), 0, s, g);
    ACX_HIP(hipGetLastError());
    return fit_launch_update(u, c, G, part, gtiles, loss, inv, cus, apply, s);
}

// The three launches.  BOTH matrix launches take the update kernel's tile rule, a function of (classes, CUs) alone: the logits
// of a row then have the same bits in every batch, whatever `rows` is (the two tile shapes add the 768 products in different
// orders, so a rule that looked at `rows`, as fit_launch's does for BCE, would let the short last batch of an epoch change them).
static int fit_launch_logits(const FitCall& c, float* z, int cus, hipStream_t s) {
    const int rows = (int)c.rows, N = c.classes;
    FitGradP g = fit_grad_params(c, z);
    const bool g32 = fit_classes_wide(N, cus);
    const int gs = g32 ? 32 : 16;
    g.tiles_n = (N + gs - 1) / gs;
    const int gtiles = ((rows + gs - 1) / gs) * g.tiles_n;
    if (g32) launch_kernel(&fit_logits_kernel<32>, dim3(gtiles), dim3(kFitThreads), 0, s, g);
    else launch_kernel(&fit_logits_kernel<16>, dim3(gtiles), dim3(kFitThreads), 0, s, g);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

static int fit_ce_launch(const FitCall& c, float* z, float* G, float* part, const FitUpdP& u, bool apply, float* loss, hipStream_t s) {
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));
    const int rows = (int)c.rows, N = c.classes;
    const float inv = (float)(1.0 / (double)rows);
    ACX_TRY(fit_launch_logits(c, z, cus, s));

    FitCeRowP r;
    r.z = z; r.labels = static_cast<const long long*>(c.Y); r.idx = reinterpret_cast<const long long*>(c.idx); r.n_total = c.n_total; r.rows = rows; r.N = N;
    r.q_hit = (float)((1.0 - c.eps) + c.eps / N); r.q_miss = (float)(c.eps / N); r.ome = (float)(1.0 - c.eps);
    r.inv = inv; r.G = G; r.part = part; r.status = (int*)c.status;
    if (N <= kSoftWaveMaxN) launch_kernel(&fit_ce_row_kernel<64>, dim3((rows + 3) / 4), dim3(kFitThreads), 0, s, r);
    else launch_kernel(&fit_ce_row_kernel<256>, dim3(rows), dim3(kFitThreads), 0, s, r);
    ACX_HIP(hipGetLastError());
    return fit_launch_update(u, c, G, part, rows, loss, inv, cus, apply, s);
}

// ---- weak labels: host side -------------------------------------------------------------------------------------------------
// workspace: G, z (seg_rows_max, classes), P (bags_max, classes) fp32, then one loss partial per (bag, chunk of 64 classes)
struct MilLayout { size_t z, P, part, total; };
static MilLayout fit_mil_layout(long long seg_rows, long long bags, long long N) {
    MilLayout l;
    const size_t gb = align_up((size_t)seg_rows * N * 4);
    l.z = gb;
    l.P = 2 * gb;
    l.part = l.P + align_up((size_t)bags * N * 4);
    l.total = l.part + align_up((size_t)bags * ((N + 63) / 64) * 4);
    return l;
}

static int fit_mil_check_pool(const char* who, int pool) {
    if (pool != ACX_MIL_MAX && pool != ACX_MIL_MEAN && pool != ACX_MIL_LINEAR && pool != ACX_MIL_EXP)
        ACX_FAIL(ACX_ERR_ARG, "%s: pool %d (expected ACX_MIL_MAX, ACX_MIL_MEAN, ACX_MIL_LINEAR or ACX_MIL_EXP)", who, pool);
    return ACX_OK;
}

static int fit_mil_check_shape(const char* who, int64_t seg_rows, int64_t bags, int classes) {
    if (bags < 1) ACX_FAIL(ACX_ERR_ARG, "%s: bags = %lld (expected >= 1)", who, (long long)bags);
    if (seg_rows < 1) ACX_FAIL(ACX_ERR_ARG, "%s: seg_rows = %lld (expected >= 1)", who, (long long)seg_rows);
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "%s: classes = %d (expected 1 .. %d)", who, classes, ACX_MAX_CLASSES);
    if (seg_rows > kFitMaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: seg_rows = %lld (at most 2^22 per step)", who, (long long)seg_rows);
    if (bags > kFitMaxRows || bags * ((classes + 63) / 64) > (1LL << 30))
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: bags = %lld (at most 2^22 per step, and 2^30 chunks of 64 classes)", who, (long long)bags);
    return ACX_OK;
}

struct MilCall {        // what a weak-label step has beside FitCall (whose idx / rows are seg_idx / seg_rows)
    int64_t n_bags; const int32_t* bag_off; const int64_t* bag_idx; int64_t bags; int pool;
};

static int fit_mil_check_call(const char* who, const FitCall& c, const MilCall& m, MilLayout* lay) {
    if (!c.E) ACX_FAIL(ACX_ERR_ARG, "%s: E is null", who);
    if (!c.Y) ACX_FAIL(ACX_ERR_ARG, "%s: target is null", who);
    if (!c.idx) ACX_FAIL(ACX_ERR_ARG, "%s: seg_idx is null", who);
    if (!m.bag_off) ACX_FAIL(ACX_ERR_ARG, "%s: bag_off is null", who);
    if (!m.bag_idx) ACX_FAIL(ACX_ERR_ARG, "%s: bag_idx is null", who);
    if (!c.W) ACX_FAIL(ACX_ERR_ARG, "%s: W is null", who);
    if (!c.b) ACX_FAIL(ACX_ERR_ARG, "%s: b is null", who);
    if (!c.status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!c.ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    if (c.y_dtype != ACX_TARGET_F32 && c.y_dtype != ACX_TARGET_U8)
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, c.y_dtype);
    ACX_TRY(fit_mil_check_shape(who, c.rows, m.bags, c.classes));
    ACX_TRY(fit_mil_check_pool(who, m.pool));
    if (m.n_bags < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n_bags_total = %lld (expected >= 1)", who, (long long)m.n_bags);
    ACX_TRY(fit_check_rows(who, c));
    if (c.ld_y < c.classes)
        ACX_FAIL(ACX_ERR_ARG, "%s: ld_target = %lld is shorter than %d classes", who, (long long)c.ld_y, c.classes);
    *lay = fit_mil_layout(c.rows, m.bags, c.classes);
    return check_workspace_for(who, c.ws, c.ws_bytes, lay->total);
}

template <bool GRAD>
static int fit_mil_launch_bag(const FitMilP& p, int pool, hipStream_t s) {
    const dim3 grid((unsigned)(((long long)p.bags * p.chunks + 3) / 4)), block(kFitThreads);
    switch (pool) {
        case ACX_MIL_MAX: launch_kernel(&fit_mil_bag_kernel<kMilMax, GRAD>, grid, block, 0, s, p); break;
        case ACX_MIL_MEAN: launch_kernel(&fit_mil_bag_kernel<kMilMean, GRAD>, grid, block, 0, s, p); break;
        case ACX_MIL_LINEAR: launch_kernel(&fit_mil_bag_kernel<kMilLinear, GRAD>, grid, block, 0, s, p); break;
        default: launch_kernel(&fit_mil_bag_kernel<kMilExp, GRAD>, grid, block, 0, s, p); break;
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

// The three launches: the logits of the segment rows (the cross-entropy step's launch: a row's z bits are acx_head_fit_grad_ce's),
// the bag pass, and the update over the segment rows with 1 / (bags classes) on the loss.
static int fit_mil_launch(const FitCall& c, const MilCall& m, float* z, float* P, float* G, float* part, const FitUpdP& u, bool apply,
                          float* loss, hipStream_t s) {
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));
    const int N = c.classes, bags = (int)m.bags;
    const float inv = (float)(1.0 / ((double)bags * (double)N));
    ACX_TRY(fit_launch_logits(c, z, cus, s));
    FitMilP p{};
    p.z = z; p.ld_z = N; p.bag_off = m.bag_off; p.bags = bags; p.seg_rows = (int)c.rows; p.N = N; p.chunks = (N + 63) / 64;
    p.P = P; p.ld_p = N;
    p.Y = c.Y; p.y_u8 = c.y_dtype == ACX_TARGET_U8; p.ld_y = c.ld_y; p.n_bags = m.n_bags;
    p.bag_idx = reinterpret_cast<const long long*>(m.bag_idx);
    p.G = G; p.part = part; p.inv = inv; p.status = (int*)c.status;
    ACX_TRY(fit_mil_launch_bag<true>(p, m.pool, s));
    return fit_launch_update(u, c, G, part, bags * p.chunks, loss, inv, cus, apply, s);
}

// A job's slice of the group workspace: the single call's layout of its loss (z_off is unused for BCE).
static void fit_group_layout(int loss, long long rows, long long N, size_t* z_off, size_t* part_off, size_t* per_job) {
    *z_off = 0;
    if (loss == kLossCe) fit_ce_layout(rows, N, z_off, part_off, per_job);
    else fit_layout(rows, N, part_off, per_job);
}

static int fit_group_check_shape(const char* who, int jobs, int64_t rows_max, int classes, int loss) {
    if (jobs < 1 || jobs > ACX_FIT_MAX_JOBS) ACX_FAIL(ACX_ERR_ARG, "%s: jobs = %d (expected 1 .. %d)", who, jobs, ACX_FIT_MAX_JOBS);
    if (loss != ACX_FIT_LOSS_BCE && loss != ACX_FIT_LOSS_CE)
        ACX_FAIL(ACX_ERR_ARG, "%s: loss %d (expected ACX_FIT_LOSS_BCE or ACX_FIT_LOSS_CE)", who, loss);
    return fit_check_shape(who, rows_max, classes);
}

struct FitGroupCall {
    int loss; double eps; int jobs; const acx_fit_job* job_table; const void* plan; int64_t steps, step;
};

// One group step: each stage once for all jobs.  c holds the shared arguments as a single call's would (rows = rows_max, no W / b).
static int fit_group_step(const char* who, const FitCall& c, const FitGroupCall& gc, hipStream_t s) {
    if (!c.E) ACX_FAIL(ACX_ERR_ARG, "%s: E is null", who);
    if (!c.Y) ACX_FAIL(ACX_ERR_ARG, "%s: %s is null", who, c.y_name);
    if (!gc.job_table) ACX_FAIL(ACX_ERR_ARG, "%s: jobs is null", who);
    if (!gc.plan) ACX_FAIL(ACX_ERR_ARG, "%s: plan is null", who);
    if (!c.status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!c.ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    ACX_TRY(fit_group_check_shape(who, gc.jobs, c.rows, c.classes, gc.loss));
    if (gc.steps < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n_steps = %lld (expected >= 1)", who, (long long)gc.steps);
    if (gc.step < 0 || gc.step >= gc.steps)
        ACX_FAIL(ACX_ERR_ARG, "%s: step = %lld (expected 0 .. %lld)", who, (long long)gc.step, (long long)gc.steps - 1);
    if (gc.loss == kLossCe) {
        if (!(gc.eps >= 0.0 && gc.eps < 1.0))
            ACX_FAIL(ACX_ERR_ARG, "%s: label_smoothing = %g (expected 0 <= label_smoothing < 1)", who, gc.eps);
    } else if (c.y_dtype != ACX_TARGET_F32 && c.y_dtype != ACX_TARGET_U8) {
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, c.y_dtype);
    }
    ACX_TRY(fit_check_rows(who, c));                               // W and b live in the job table, on the device
    if (gc.loss == kLossBce && c.ld_y < c.classes)
        ACX_FAIL(ACX_ERR_ARG, "%s: ld_target = %lld is shorter than %d classes", who, (long long)c.ld_y, c.classes);
    FitGroupP q{};
    size_t per_job;
    fit_group_layout(gc.loss, c.rows, c.classes, &q.z_off, &q.part_off, &per_job);
    ACX_TRY(check_workspace_for(who, c.ws, c.ws_bytes, per_job * (size_t)gc.jobs));
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));

    const int J = gc.jobs, rows = (int)c.rows, N = c.classes;
    q.E = c.E; q.ld_e = c.ld_e; q.n_total = c.n_total;
    q.Y = c.Y; q.y_u8 = c.y_dtype == ACX_TARGET_U8; q.ld_y = c.ld_y;
    q.jobs = gc.job_table; q.plan = static_cast<const FitPlanE*>(gc.plan) + gc.step * J;
    q.N = N; q.rows_max = rows; q.cus = cus; q.loss = gc.loss;
    q.ws = static_cast<char*>(c.ws); q.ws_job = per_job; q.status = (int*)c.status;
    const auto tiles = [&](int S) { return (unsigned)(((rows + S - 1) / S) * ((N + S - 1) / S)); };
    const bool u32 = fit_classes_wide(N, cus);
    if (gc.loss == kLossCe) {
        q.q_hit = (float)((1.0 - gc.eps) + gc.eps / N); q.q_miss = (float)(gc.eps / N); q.ome = (float)(1.0 - gc.eps);
        if (u32) launch_kernel(&fit_group_grad_kernel<32, kLossCe>, dim3(tiles(32), J), dim3(kFitThreads), 0, s, q);
        else launch_kernel(&fit_group_grad_kernel<16, kLossCe>, dim3(tiles(16), J), dim3(kFitThreads), 0, s, q);
        ACX_HIP(hipGetLastError());
        if (N <= kSoftWaveMaxN) launch_kernel(&fit_group_ce_row_kernel<64>, dim3((rows + 3) / 4, J), dim3(kFitThreads), 0, s, q);
        else launch_kernel(&fit_group_ce_row_kernel<256>, dim3(rows, J), dim3(kFitThreads), 0, s, q);
        ACX_HIP(hipGetLastError());
    } else {
        // fit_rows_wide never falls as rows grow: a job of 1 .. rows_max rows can need the wide form only if rows_max does, the
        // narrow one only if a single row does.  One launch per form that can occur; a block of the other form returns at once.
        if (fit_rows_wide(rows, N, cus)) {
            launch_kernel(&fit_group_grad_kernel<32, kLossBce>, dim3(tiles(32), J), dim3(kFitThreads), 0, s, q);
            ACX_HIP(hipGetLastError());
        }
        if (!fit_rows_wide(1, N, cus)) {
            launch_kernel(&fit_group_grad_kernel<16, kLossBce>, dim3(tiles(16), J), dim3(kFitThreads), 0, s, q);
            ACX_HIP(hipGetLastError());
        }
    }
    const int us = u32 ? 32 : 16;
    const dim3 ugrid(((N + us - 1) / us) * (kFitK / us) + (N + kFitDbCols - 1) / kFitDbCols + 1, J);
    if (u32) launch_kernel(&fit_group_update_kernel<32>, ugrid, dim3(kFitThreads), 0, s, q);
    else launch_kernel(&fit_group_update_kernel<16>, ugrid, dim3(kFitThreads), 0, s, q);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_head_fit_workspace_bytes(int64_t rows_max, int classes, size_t* out_bytes) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_head_fit_workspace_bytes: out_bytes is null");
    ACX_TRY(fit_check_shape("acx_head_fit_workspace_bytes", rows_max, classes));
    size_t po;
    fit_layout(rows_max, classes, &po, out_bytes);
    return ACX_OK;
}

int acx_head_fit_step(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                      int64_t ld_target, const int64_t* idx, int64_t rows, int classes, float* W, float* b, float* mW, float* vW,
                      float* vmaxW, float* mb, float* vb, float* vmaxb, const acx_adam* hp, int64_t step_t, double lr,
                      float* loss_out, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_head_fit_step";
    const FitCall c{E, ld_e, n_rows_total, target, "target", target_dtype, ld_target, 0.0, idx, rows, classes, W, b, status, ws,
                    ws_bytes};
    size_t part_off;
    ACX_TRY(fit_check_call(who, c, &part_off));
    FitUpdP u{};
    ACX_TRY(fit_step_args(who, W, b, mW, vW, vmaxW, mb, vb, vmaxb, hp, step_t, lr, loss_out, &u));
    char* w = static_cast<char*>(ws);
    return fit_launch(c, nullptr, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + part_off), u, true, loss_out,
                      (hipStream_t)stream);
}

int acx_head_fit_grad(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                      int64_t ld_target, const int64_t* idx, int64_t rows, int classes, const float* W, const float* b, float* z,
                      float* G, float* dW, float* db, float* loss, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_head_fit_grad";
    const FitCall c{E, ld_e, n_rows_total, target, "target", target_dtype, ld_target, 0.0, idx, rows, classes, W, b, status, ws,
                    ws_bytes};
    size_t part_off;
    ACX_TRY(fit_check_call(who, c, &part_off));
    FitUpdP u{};
    ACX_TRY(fit_grad_args(who, z, G, dW, db, loss, &u));
    return fit_launch(c, z, G, reinterpret_cast<float*>(static_cast<char*>(ws) + part_off), u, false, loss, (hipStream_t)stream);
}

int acx_head_fit_ce_workspace_bytes(int64_t rows_max, int classes, size_t* out_bytes) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_head_fit_ce_workspace_bytes: out_bytes is null");
    ACX_TRY(fit_check_shape("acx_head_fit_ce_workspace_bytes", rows_max, classes));
    size_t zo, po;
    fit_ce_layout(rows_max, classes, &zo, &po, out_bytes);
    return ACX_OK;
}

int acx_head_fit_step_ce(const float* E, int64_t ld_e, int64_t n_rows_total, const int64_t* labels, const int64_t* idx,
                         int64_t rows, int classes, double label_smoothing, float* W, float* b, float* mW, float* vW, float* vmaxW,
                         float* mb, float* vb, float* vmaxb, const acx_adam* hp, int64_t step_t, double lr, float* loss_out,
                         int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_head_fit_step_ce";
    const FitCall c{E, ld_e, n_rows_total, labels, "labels", 0, 0, label_smoothing, idx, rows, classes, W, b, status, ws, ws_bytes};
    size_t z_off, part_off;
    ACX_TRY(fit_ce_check_call(who, c, &z_off, &part_off));
    FitUpdP u{};
    ACX_TRY(fit_step_args(who, W, b, mW, vW, vmaxW, mb, vb, vmaxb, hp, step_t, lr, loss_out, &u));
    char* w = static_cast<char*>(ws);
    return fit_ce_launch(c, reinterpret_cast<float*>(w + z_off), reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + part_off),
                         u, true, loss_out, (hipStream_t)stream);
}

int acx_head_fit_grad_ce(const float* E, int64_t ld_e, int64_t n_rows_total, const int64_t* labels, const int64_t* idx,
                         int64_t rows, int classes, double label_smoothing, const float* W, const float* b, float* z, float* G,
                         float* dW, float* db, float* loss, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_head_fit_grad_ce";
    const FitCall c{E, ld_e, n_rows_total, labels, "labels", 0, 0, label_smoothing, idx, rows, classes, W, b, status, ws, ws_bytes};
    size_t z_off, part_off;
    ACX_TRY(fit_ce_check_call(who, c, &z_off, &part_off));
    FitUpdP u{};
    ACX_TRY(fit_grad_args(who, z, G, dW, db, loss, &u));
    return fit_ce_launch(c, z, G, reinterpret_cast<float*>(static_cast<char*>(ws) + part_off), u, false, loss, (hipStream_t)stream);
}

int acx_head_fit_mil_workspace_bytes(int64_t seg_rows_max, int64_t bags_max, int classes, size_t* out_bytes) {
    static const char* who = "acx_head_fit_mil_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(fit_mil_check_shape(who, seg_rows_max, bags_max, classes));
    *out_bytes = fit_mil_layout(seg_rows_max, bags_max, classes).total;
    return ACX_OK;
}

int acx_head_fit_step_mil(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                          int64_t ld_target, int64_t n_bags_total, const int64_t* seg_idx, int64_t seg_rows, const int32_t* bag_off,
                          const int64_t* bag_idx, int64_t bags, int classes, int pool, float* W, float* b, float* mW, float* vW,
                          float* vmaxW, float* mb, float* vb, float* vmaxb, const acx_adam* hp, int64_t step_t, double lr,
                          float* loss_out, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_head_fit_step_mil";
    const FitCall c{E, ld_e, n_rows_total, target, "target", target_dtype, ld_target, 0.0, seg_idx, seg_rows, classes, W, b, status,
                    ws, ws_bytes};
    const MilCall m{n_bags_total, bag_off, bag_idx, bags, pool};
    MilLayout lay;
    ACX_TRY(fit_mil_check_call(who, c, m, &lay));
    FitUpdP u{};
    ACX_TRY(fit_step_args(who, W, b, mW, vW, vmaxW, mb, vb, vmaxb, hp, step_t, lr, loss_out, &u));
    char* w = static_cast<char*>(ws);
    return fit_mil_launch(c, m, reinterpret_cast<float*>(w + lay.z), reinterpret_cast<float*>(w + lay.P), reinterpret_cast<float*>(w),
                          reinterpret_cast<float*>(w + lay.part), u, true, loss_out, (hipStream_t)stream);
}

int acx_head_fit_grad_mil(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                          int64_t ld_target, int64_t n_bags_total, const int64_t* seg_idx, int64_t seg_rows, const int32_t* bag_off,
                          const int64_t* bag_idx, int64_t bags, int classes, int pool, const float* W, const float* b, float* z,
                          float* P, float* G, float* dW, float* db, float* loss, int32_t* status, void* ws, size_t ws_bytes,
                          void* stream) {
    static const char* who = "acx_head_fit_grad_mil";
    const FitCall c{E, ld_e, n_rows_total, target, "target", target_dtype, ld_target, 0.0, seg_idx, seg_rows, classes, W, b, status,
                    ws, ws_bytes};
    const MilCall m{n_bags_total, bag_off, bag_idx, bags, pool};
    MilLayout lay;
    ACX_TRY(fit_mil_check_call(who, c, m, &lay));
    if (!P) ACX_FAIL(ACX_ERR_ARG, "%s: an output (z, P, G, dW, db, loss) is null", who);
    FitUpdP u{};
    ACX_TRY(fit_grad_args(who, z, G, dW, db, loss, &u));
    return fit_mil_launch(c, m, z, P, G, reinterpret_cast<float*>(static_cast<char*>(ws) + lay.part), u, false, loss,
                          (hipStream_t)stream);
}

int acx_segment_pool(const float* logits, int64_t ld, const int32_t* bag_off, int64_t bags, int classes, int pool, float* out,
                     int32_t* status, void* stream) {
    static const char* who = "acx_segment_pool";
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!bag_off) ACX_FAIL(ACX_ERR_ARG, "%s: bag_off is null", who);
    if (!out) ACX_FAIL(ACX_ERR_ARG, "%s: out is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    ACX_TRY(fit_mil_check_shape(who, 1, bags, classes));
    ACX_TRY(fit_mil_check_pool(who, pool));
    if (ld < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld = %lld is shorter than %d classes", who, (long long)ld, classes);
    FitMilP p{};
    p.z = logits; p.ld_z = ld; p.bag_off = bag_off; p.bags = (int)bags; p.seg_rows = 0x7ffffff0;     // the caller owns the rows
    p.N = classes; p.chunks = (classes + 63) / 64; p.P = out; p.ld_p = classes; p.status = (int*)status;
    return fit_mil_launch_bag<false>(p, pool, (hipStream_t)stream);
}

int acx_adam_update(float* param, const float* grad, float* m, float* v, float* vmax, int64_t n, const acx_adam* hp,
                    int64_t step_t, double lr, void* stream) {
    static const char* who = "acx_adam_update";
    if (!param || !grad || !m || !v) ACX_FAIL(ACX_ERR_ARG, "%s: param, grad, m or v is null", who);
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    AdamK a;
    ACX_TRY(adam_scalars(who, hp, step_t, lr, &a));
    if (hp->amsgrad && !vmax) ACX_FAIL(ACX_ERR_ARG, "%s: vmax is null with hp->amsgrad set", who);
    launch_kernel(&adam_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, m, v,
                  vmax, (long long)n, a);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_head_fit_group_workspace_bytes(int jobs, int64_t rows_max, int classes, int loss, size_t* out_bytes) {
    static const char* who = "acx_head_fit_group_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(fit_group_check_shape(who, jobs, rows_max, classes, loss));
    size_t zo, po, per_job;
    fit_group_layout(loss, rows_max, classes, &zo, &po, &per_job);
    *out_bytes = per_job * (size_t)jobs;
    return ACX_OK;
}

int acx_head_fit_plan_bytes(int jobs, int64_t n_steps, size_t* out_bytes) {
    static const char* who = "acx_head_fit_plan_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    if (jobs < 1 || jobs > ACX_FIT_MAX_JOBS) ACX_FAIL(ACX_ERR_ARG, "%s: jobs = %d (expected 1 .. %d)", who, jobs, ACX_FIT_MAX_JOBS);
    if (n_steps < 1 || n_steps > (1LL << 40) / ACX_FIT_MAX_JOBS) ACX_FAIL(ACX_ERR_ARG, "%s: n_steps = %lld (expected >= 1)", who, (long long)n_steps);
    *out_bytes = sizeof(FitPlanE) * (size_t)jobs * (size_t)n_steps;
    return ACX_OK;
}

int acx_head_fit_plan_fill(int jobs, int64_t n_steps, int64_t rows_max, int classes, int loss, const int32_t* rows,
                           const int64_t* idx_offset, const acx_adam* hp, const double* lr, void* plan, size_t plan_bytes) {
    static const char* who = "acx_head_fit_plan_fill";
    size_t need;
    ACX_TRY(acx_head_fit_plan_bytes(jobs, n_steps, &need));
    ACX_TRY(fit_group_check_shape(who, jobs, rows_max, classes, loss));
    if (!rows || !idx_offset || !hp || !lr || !plan) ACX_FAIL(ACX_ERR_ARG, "%s: rows, idx_offset, hp, lr or plan is null", who);
    if (plan_bytes < need) ACX_FAIL(ACX_ERR_ARG, "%s: plan of %zu bytes, %zu needed", who, plan_bytes, need);
    for (int j = 1; j < jobs; ++j)
        if (!hp[j].amsgrad != !hp[0].amsgrad || !hp[j].decoupled != !hp[0].decoupled)
            ACX_FAIL(ACX_ERR_ARG, "%s: hp[%d] differs from hp[0] in amsgrad / decoupled (a group shares them)", who, j);
    FitPlanE* out = static_cast<FitPlanE*>(plan);
    std::vector<int64_t> t((size_t)jobs, 0);
    for (int64_t s = 0; s < n_steps; ++s)
        for (int j = 0; j < jobs; ++j) {
            const size_t i = (size_t)s * jobs + j;
            FitPlanE e{};
            if (rows[i] < 0 || rows[i] > rows_max)
                ACX_FAIL(ACX_ERR_ARG, "%s: rows[%lld][%d] = %d (expected 0 .. rows_max = %lld)", who, (long long)s, j, rows[i], (long long)rows_max);
            if (rows[i] > 0) {
                if (idx_offset[i] < 0) ACX_FAIL(ACX_ERR_ARG, "%s: idx_offset[%lld][%d] = %lld (expected >= 0)", who, (long long)s, j, (long long)idx_offset[i]);
                e.idx_off = idx_offset[i];
                e.rows = rows[i];
                e.loss_slot = (int)t[j];
                e.inv = loss == kLossCe ? (float)(1.0 / (double)rows[i]) : (float)(1.0 / ((double)rows[i] * (double)classes));
                ACX_TRY(adam_scalars(who, &hp[j], ++t[j], lr[i], &e.a));      // the job's own step count: idle steps do not advance it
            }
            out[i] = e;
        }
    return ACX_OK;
}

int acx_head_fit_group_step(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                            int64_t ld_target, int jobs, int64_t rows_max, int classes, const acx_fit_job* job_table,
                            const void* plan, int64_t n_steps, int64_t step, int32_t* status, void* ws, size_t ws_bytes,
                            void* stream) {
    const FitCall c{E, ld_e, n_rows_total, target, "target", target_dtype, ld_target, 0.0, nullptr, rows_max, classes, nullptr,
                    nullptr, status, ws, ws_bytes};
    return fit_group_step("acx_head_fit_group_step", c, FitGroupCall{kLossBce, 0.0, jobs, job_table, plan, n_steps, step},
                          (hipStream_t)stream);
}

int acx_head_fit_group_step_ce(const float* E, int64_t ld_e, int64_t n_rows_total, const int64_t* labels, int jobs, int64_t rows_max,
                               int classes, double label_smoothing, const acx_fit_job* job_table, const void* plan, int64_t n_steps,
                               int64_t step, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    const FitCall c{E, ld_e, n_rows_total, labels, "labels", 0, 0, label_smoothing, nullptr, rows_max, classes, nullptr, nullptr,
                    status, ws, ws_bytes};
    return fit_group_step("acx_head_fit_group_step_ce", c,
                          FitGroupCall{kLossCe, label_smoothing, jobs, job_table, plan, n_steps, step}, (hipStream_t)stream);
}

}  // extern "C"
