// Host-side declarations shared by the libacx translation units (gfx950 only): the context, the launcher prototypes and the
// host helpers.  What kernels share lives in device_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/acx.h"
#include "packed.h"

struct acx_resampler {
    int device, orig, target, of, nf, width, max_band, per_thread;
    size_t lds_bytes;
    int2* band;         // [nf] {start_i - width (input offset of the band's first sample from j * of), count_i}
    float* taps;        // [max_band][nf]: tap r of phase i at taps[r * nf + i] (lanes on consecutive phases read consecutively)
};

namespace acx {

constexpr int kDepths[4] = {3, 3, 9, 3};        // convnext.py:655
constexpr int kDims[4] = {96, 192, 384, 768};   // convnext.py:656
constexpr int kNFFT = 1024, kHop = 320, kBins = 513, kMels = 224;   // convnext.py:168-172
constexpr int kClasses = ACX_NUM_CLASSES;      // the AudioSet head; a context's own class count is acx_ctx::num_classes
// Heads of this many classes or more run as pooling (scene rows into the workspace) + the class-tiled head kernel (misc.hip,
// head_tiled_kernel); narrower ones, the AudioSet head included, as the fused pool_head_kernel.  Both give the same bits.  The
// first measured N past the crossover of the two at bs 64, where the fused kernel costs ~0.06 us per class and the tiled one
// ~0.046 ms flat (at bs 1 the tiled one is faster from N = 527 on); profiles/r12_a_heads_bench.txt, DESIGN.md 2.
constexpr int kHeadTiledMin = 640;
constexpr int kStemW = 56;                      // 224 mel bins / 4

void set_error(const char* fmt, ...);

#define ACX_FAIL(code, ...)          \
    do {                             \
        acx::set_error(__VA_ARGS__); \
        return (code);               \
    } while (0)

#define ACX_HIP(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            ACX_FAIL(ACX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                              \
    } while (0)

#define ACX_TRY(expr)             \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != ACX_OK) return rc_; \
    } while (0)

// hipFuncSetAttribute acts on the CURRENT device: remember, per kernel, which devices already have the attribute
// (one process may drive several GPUs; launches may come from several threads)
struct DeviceOnce {
    std::atomic<unsigned long long> mask{0};
};
template <typename K>
inline int set_max_dynamic_lds(DeviceOnce& once, K kernel, size_t bytes) {
    int dev = 0;
    ACX_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ULL << (dev & 63);
    if (once.mask.load(std::memory_order_acquire) & bit) return ACX_OK;
    ACX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    once.mask.fetch_or(bit, std::memory_order_release);
    return ACX_OK;
}

// CU-exclusive workgroups: a workgroup that holds ALL of a CU's LDS (kCuLdsBytes requested at launch)
// and all of its vector registers (512 threads x 256 or 256 threads x 512 registers) cannot share the CU with any other
// wave -- the hardware's own resource accounting enforces it.  Every kernel that runs dense 16-bit MFMA on live data
// is launched this way: next to such a kernel, packed-FP32 VALU instructions (v_pk_*_f32) of a co-resident foreign
// wave return wrong results on this platform (tools/race2/).
constexpr size_t kCuLdsBytes = 160 * 1024;

// ---- host-side weight image helpers (acx_finalize and the per-kernel packers) ----
inline uint16_t to_bf16(float f) {      // round to nearest even, as v_cvt_pk_bf16_f32 does
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// S16 form of gemm_split.hip: [rows][K/8][hi x8 | lo x8] fp16, values pre-multiplied by `scale` (a power of two)
inline std::vector<uint16_t> s16_rows(const std::vector<float>& w, int rows, int K, float scale) {
    std::vector<uint16_t> h((size_t)rows * K * 2);
    for (int n = 0; n < rows; ++n)
        for (int k = 0; k < K; ++k) {
            const float v = w[(size_t)n * K + k] * scale;
            const _Float16 hi = (_Float16)v;
            const _Float16 lo = (_Float16)(v - (float)hi);
            uint16_t* blk = h.data() + ((size_t)n * K + (size_t)(k & ~7)) * 2;
            std::memcpy(blk + (k & 7), &hi, 2);
            std::memcpy(blk + 8 + (k & 7), &lo, 2);
        }
    return h;
}

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct BlockW {          // one ConvNeXt Block (convnext.py:44-87), kernel layouts
    float* dw = nullptr;     // [49][C]   tap-major depthwise weights
    float* dwb = nullptr;    // [C]
    float* b1 = nullptr;     // [4C]      pwconv1 bias + W1 . ln_bias
    float* b2 = nullptr;     // [C]       gamma * pwconv2 bias
    // Weight images: acx_finalize uploads only those the launches of the context's arithmetic read; the rest stay null.
    // W1 = pwconv1 with the LayerNorm weight folded in [4C][C], W2 = gamma * pwconv2 [C][4C].
    float* w1 = nullptr;     // fp32, stages 2-3: W1
    float* w1sum = nullptr;  // fp32, stages 2-3: [4C] sum_k w1[n][k]  (LayerNorm applied in the GEMM epilogue)
    float* w2 = nullptr;     // fp32, stages 2-3: W2
    float* wpack = nullptr;  // fp32, stages 0-1: chunk-major image of mlp_fused.hip
    uint16_t* wpack_s = nullptr;   // fp32_split, stage 0: chunk-major S16 image of mlp_fused_split.hip
    uint16_t* wstream_s = nullptr; // fp32_split, stages 1-2: S16 segment stream of mlp_fused_wide.hip
    uint16_t* w1s = nullptr; // fp32_split, stage 3: W1 in S16 form (gemm_split.hip), scaled by w1s_scale
    uint16_t* w2s = nullptr; // fp32_split, stage 3: W2 in S16 form, scaled by w2s_scale
    uint16_t* wstream_b = nullptr; // bf16 / bf16a, stages 0-2: bf16 segment stream of mlp_fused_wide_bf16.hip
    uint16_t* w1h = nullptr; // bf16 / bf16a, stage 3: [4C][Cp]  W1 rounded to bf16, K zero-padded to Cp = pad64(C)
    uint16_t* w2h = nullptr; // bf16 / bf16a, stage 3: W2 rounded to bf16
    uint16_t* dw_ops = nullptr;    // bf16a, stages 0-2: the depthwise weights as the B operands of dwconv_mfma.hip
    float w1s_scale = 1.f, w2s_scale = 1.f;   // fp32_split: power-of-two scales of the S16 weight images
    float hid_scale = 1.f;   // fp32_split: power-of-two scale of the S16 hidden activation (GELU output)
};

struct DownW {           // downsample_layers[i], i>=1 (convnext.py:230-235)
    float* b = nullptr;      // [C']      bias + W . ln_bias
    // W = [C'][4C], k = (dy*2+dx)*C + c, LayerNorm weight folded in: one form per arithmetic
    float* w = nullptr;      // fp32
    uint16_t* ws = nullptr;  // fp32_split: in S16 form, scaled by ws_scale
    uint16_t* wh = nullptr;  // bf16 / bf16a: [C'][4*Cp]  k = (dy*2+dx)*Cp + c
    float ws_scale = 1.f;
};

struct Profile {
    bool on = false;
    struct Rec { int cls; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
};

}  // namespace acx

struct acx_ctx {
    int device = 0;
    bool finalized = false;
    std::map<std::string, acx::HostTensor> host;     // raw state_dict as handed in
    std::vector<void*> allocs;                       // every device allocation we own

    // frontend
    float* d_hann = nullptr;      // [1024]
    float* d_twiddle = nullptr;   // [1024][2]  exp(-2 pi i n / 1024)
    int* d_mel_start = nullptr;   // [224]
    int* d_mel_len = nullptr;     // [224]
    int* d_mel_off = nullptr;     // [224] offset into d_mel_w
    float* d_mel_w = nullptr;     // banded mel weights
    int mel_w_len = 0;            // number of floats in d_mel_w
    float* d_bn_scale = nullptr;  // [224]
    float* d_bn_shift = nullptr;  // [224]
    // dense-DFT fallback (STFT buffers that are not window x DFT: the two Conv1d are evaluated as one GEMM, convnext.py:179-187)
    bool dense_stft = false;
    bool force_dense_stft = false; // acx_set_frontend(ACX_FRONTEND_DENSE)
    float stft_deviation = 0.f;   // max |stored - hann x DFT| found at acx_finalize
    float* d_stft_w = nullptr;    // [kDenseN][1024]: rows 0..512 conv_real, 513..1025 conv_imag, the rest zero
    float* d_stft_zero = nullptr; // [kDenseN] zero bias
    // stem
    float* d_stem_w = nullptr;    // [96][16]
    float* d_stem_b = nullptr;    // [96]
    float* d_stem_lnw = nullptr;  // [96]
    float* d_stem_lnb = nullptr;  // [96]
    acx::DownW down[4];
    std::vector<acx::BlockW> blocks[4];
    // tail
    float* d_norm_w = nullptr;    // [768]
    float* d_norm_b = nullptr;
    float* d_head_w = nullptr;    // [N][768]
    float* d_head_b = nullptr;    // [N]
    int num_classes = 0;          // N of the finalized head (0 while not finalized)

    int precision = ACX_PREC_F32_SPLIT;   // acx_set_precision (include/acx.h): the default equals the Python host's
    // two-way batch split over two HIP streams (fork/join by events): kernels of the two halves co-run, so
    // an HBM-bound kernel of one half fills the matrix-pipe-bound phases of the other and vice versa
    bool split_streams = true;    // ACX_SPLIT_STREAMS=0 turns it off
    int split_ways = 0;           // ACX_SPLIT_WAYS=n forces n sub-batches (1 .. kMaxSplitWays); 0: the per-arithmetic default
    // fork/join resources per CALLER stream: forwards issued on different streams (or threads) never share an event.
    // Sub-batch 0 runs on the caller's stream, sub-batch i > 0 on streams[i - 1].  An entry is pinned (users > 0) while a
    // forward is queueing work on it; the map is bounded by dropping the least recently used UNPINNED entry.
    static constexpr int kMaxSplitWays = 4;
    struct Aux { hipStream_t streams[kMaxSplitWays - 1] = {}; hipEvent_t fork = nullptr, joins[kMaxSplitWays - 1] = {}; };
    struct AuxEntry { Aux a; unsigned long long stamp = 0; int users = 0; };
    std::map<hipStream_t, AuxEntry> aux;
    unsigned long long aux_clock = 0;
    std::vector<Aux> aux_retired;   // evicted fork / join sets, released by acx_destroy
    std::mutex aux_mutex;
    // identity affine for acx_logmel_bn0(apply_bn0 = 0) (tests): per context, i.e. per device
    float* d_bn_one = nullptr;
    float* d_bn_zero = nullptr;
    std::atomic<int> fail_sub{-1}; // acx_test_fail_sub(ctx, i): THIS context's acx_forward reports a failure after queueing sub-batch i (error-path tests); cleared by acx_finalize
    void* comm = nullptr;          // RCCL communicator (comm.hip), owned; null until acx_comm_init
    int comm_rank = 0, comm_world = 1;
    void* d_dw_sink = nullptr;     // kDwSinkBytes: where the column-streaming depthwise kernel stores rows that are not image rows
    acx::Profile prof;
};

namespace acx {

void comm_release(acx_ctx* c);     // comm.hip

// Sub-batches of the forward THIS THREAD is queueing (acx_forward): the tile-shape choice of a small launch counts the
// workgroups of the other sub-batches too.  Per thread, not per context: concurrent forwards on one context from several
// host threads are supported and must not race on it.
extern thread_local int tls_inflight_ways;
inline int inflight_ways() { return tls_inflight_ways > 0 ? tls_inflight_ways : 1; }

// Diagnostic A/B switches (tile shape overrides), read from the environment ONCE (first acx_create) and again only through
// acx_tuning_refresh() (tests): launches read these atomics, never the environment (an uncached getenv scan sat on the
// batch-1 latency path and is not safe beside a setenv in another thread).
struct Tuning {
    std::atomic<int> gemm_mi{0};       // ACX_GEMM_MI = 1 | 2 | 4: row blocks per wave of the split / bf16 GEMM tiles (0: by launch size)
    std::atomic<int> wide_npb{0};      // ACX_WIDE_NPB = 1 | 2: pixel blocks per wave of the wide fused MLP (0: by launch size)
    std::atomic<int> wide_pers{0};     // ACX_WIDE_PERSIST: 1 = persistent wide fused MLP wherever it exists, 2 = never; 0 = by launch size
    std::atomic<int> dwm_waves{0};     // ACX_DWM_WAVES = 2..9: the matrix-pipe depthwise launch asks for that many waves per CU of its share (0: 8 = two per SIMD)
    std::atomic<int> dw_stream{-1};    // ACX_DW_STREAM = 0 | 1: forces the tile / column-streaming depthwise kernels (-1: by launch size)
    std::atomic<int> head_path{0};     // ACX_HEAD_PATH = 1 | 2: forces the fused / class-tiled head in the forwards (0: by N, kHeadTiledMin)
    std::atomic<int> knn_slice_rows{0}; // ACX_KNN_SLICE_ROWS = 16 .. 2^30: database rows per slice of acx_knn_search (0: by launch size; tests run many slices on small inputs)
    std::atomic<int> moments_slice_rows{0}; // ACX_MOMENTS_SLICE_ROWS = 16 .. 2^30: rows per slice of acx_moments (0: by n; tests run many slices on small inputs)
};
Tuning& tuning();
void tuning_reload();

// Per-kernel-class device time (acx_profile_enable / acx_profile_read).  A ProfScope names the class of the launches made on
// this thread while it is alive; when profiling is on, every launch_kernel() inside it is dispatched with a start / stop event
// pair of its own (hipExtLaunchKernel: the events carry the dispatch's begin and end timestamps -- the kernel's duration as
// rocprofv3 reports it; a hipEventRecord pair AROUND a launch also times the dispatch gap in front of the kernel, 3.6 us per
// launch on this part, 10-16 % of a 25-40 us depthwise launch).  Off: a plain launch, nothing recorded.
struct ProfScope {
    acx_ctx* ctx; int cls; hipStream_t s; ProfScope* prev;
    ProfScope(acx_ctx* c, int k, hipStream_t st);
    ~ProfScope();
};
void prof_next_events(hipEvent_t* a, hipEvent_t* b);       // api.hip: null / null unless a profiling ProfScope is open on this thread

template <typename K, typename... Args>
inline void launch_kernel(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    hipEvent_t a = nullptr, b = nullptr;
    prof_next_events(&a, &b);
    if (a && b) hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, s, a, b, 0u, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

__host__ __device__ inline int stage_h0(int T) { return (T + 8 - 4) / 4 + 1; }

// ---- variable-length batches (acx_forward_varlen, varlen.hip) -------------------------------------------------------------
// Clip i of a packed batch owns samples [soff[i], soff[i+1]), frames [foff[i], foff[i+1]) and, at stage s, image rows
// [roff[s][i], roff[s][i+1]) (H_s,i = T_i ... as the uniform geometry).  The depthwise kernels see the stage as one tall image of
// VIRTUAL rows: clip i starts at virtual row roff[s][i] + 3 i, and the three virtual rows after each clip are zero rows that
// exist in no memory.  All tables live in the head of the forward's workspace and are written by one kernel per call.
struct VarGeom {
    const long long* soff;        // [B+1] sample offsets
    const int* foff;              // [B+1] frame offsets
    const int* roff[4];           // [B+1] row offsets per stage
    const int* vclip[4];          // [vrows[s]] clip of virtual row v (a zero row belongs to the clip above it)
    const unsigned* vbits[4];     // [vwords[s]] bit v + 32 of word (v + 32) / 32: virtual row v is an image row
    const int* rclip0;            // [rows[0]] clip of stage-0 image row r (stem)
    const int* irow[4];           // s = 1..3: [rows[s]] stage s-1 image row of the top-left input of stage-s row r (downsample)
    int B;
    // host copies of the sizes (launch geometry)
    long long samples;
    int frames, rows[4], vrows[4], vwords[4], maxT, maxH[4];
};

// ---- kernel launchers (each returns acx_status) ---------------------------------------------
// dense_frames / dense_spec: scratch of the dense-DFT fallback (B*T*1024 and B*T*kDenseN floats); null: the context's own
// scratch, grown on demand (per-kernel entry point only: not capturable)
constexpr int kDenseN = 1056;                    // 2 x 513 rows padded to a multiple of the GEMM's 96-column tile
// wstart: windows of acx_forward_windows -- clip b's L samples start at wav + wstart[b] (device table) instead of wav + b L;
// needs the forward's scratch
int launch_logmel(acx_ctx* c, const float* wav, int B, int64_t L, int T, float* out, bool bn, hipStream_t s,
                  float* dense_frames = nullptr, float* dense_spec = nullptr, const long long* wstart = nullptr);
// act_bf16: the activation tensors named void* are bf16 (ACX_PREC_BF16_ACT, stages 0-2) instead of fp32; launch_dwconv then
// takes the matrix-pipe kernel (dwconv_mfma.hip), which reads BlockW::dw_ops
// max_blocks: 0 = the launcher's own grid; 1 .. kStemMaxBlocks caps it (acx_test_stem: workgroups then walk more row pairs)
constexpr int kStemMaxBlocks = 2048;
int launch_stem(acx_ctx* c, const float* in, int B, int T, int H0, void* out, hipStream_t s, bool act_bf16 = false, int max_blocks = 0);
int launch_dwconv(acx_ctx* c, const BlockW& w, int C, const void* x, void* y, float* stats, int B, int H,
                  int W, hipStream_t s, bool act_bf16 = false, int dwm_target_waves = 0 /* bf16: 0 = ACX_DWM_WAVES per CU of the launch's share */);
// column-streaming form (dwconv_col.hip): same bits as the kernels of dwconv.hip; `sink` (kDwSinkBytes, device) takes the
// stores of rows that are not part of the image; target_waves = waves the launch should spread over (one per SIMD)
constexpr int kDwColMinRows = 16;            // output rows per wave segment below which the launch uses fewer waves
constexpr int kDwSinkWindows = 128;                   // waves get sink windows of their own, modulo this
constexpr size_t kDwSinkWindowBytes = 64 * 1024;      // >= a row's lane offsets + 6 pixel strides
constexpr size_t kDwSinkBytes = kDwSinkWindows * kDwSinkWindowBytes;
int launch_dwconv_col(const void* x, void* y, const float* wt, const float* bias, void* sink, int B, int H, int W,
                      int target_waves, hipStream_t s);
// What a column-kernel launch consists of: segments of n_out = 7 k7 - s0 output rows of the Vt stacked rows, n_seg of them, six
// wave columns each.  dw_col_segments is the ONE place that decides it (wps: waves per SIMD of the width's kernel; whole_groups:
// the variable-length kernel, n_out a multiple of seven); dw_col_too_tall: the batch is beyond the kernel's multiply-high
// division.  dwconv_col_plan / _varlen: the same for a stage's width, for the test-support entry points.
struct DwColPlan { int n_out, s0, k7, n_seg, n_items; };
DwColPlan dw_col_segments(long long Vt, int wps, int target_waves, bool whole_groups);
bool dw_col_too_tall(int B, int H);
int dwconv_col_plan(int W, int B, int H, int target_waves, DwColPlan* plan);
int dwconv_col_plan_varlen(int stage, int vrows, int target_waves, DwColPlan* plan);
// launch_dwconv's fp32 kernels with the form given: col = false the ring / tile kernel, true the column kernel at target_waves
int launch_dwconv_form(acx_ctx* c, const BlockW& w, int C, const void* x, void* y, float* stats, int B, int H, int W, bool col,
                       int target_waves, hipStream_t s);
// matrix-pipe form for bf16 activations (dwconv_mfma.hip): weights rounded to bf16, fp32 accumulation; every launch size.
// dwconv_mfma_pack: its weight operands (BlockW::dw_ops) from the depthwise weights as stored, [C][49]
std::vector<uint16_t> dwconv_mfma_pack(const std::vector<float>& dw, int C);
int launch_dwconv_mfma(const void* x, void* y, const void* dw_ops, const float* bias, void* sink, int B, int H, int W,
                       int target_waves, hipStream_t s);
// What a matrix-form launch consists of: n_seg segments of `rows` = 4 `steps` output rows of the Vt stacked rows, one (slice,
// segment) group each -> n_groups, packed into `grid` workgroups.  dw_mfma_segments is the ONE place that decides it, for both
// launchers; dw_mfma_too_tall: the batch is beyond the uniform kernel's multiply-high division.
struct DwMfmaPlan { int rows, steps, n_seg, n_groups, grid; };
int dw_mfma_segments(int W, long long Vt, int target_waves, DwMfmaPlan* plan);
bool dw_mfma_too_tall(int B, int H);
// element-wise fp32 <-> bf16 (the per-layer entry points of the C ABI keep fp32 tensors in every mode)
int launch_convert_f32_to_bf16(const float* in, void* out, long long n, hipStream_t s);
int launch_convert_bf16_to_f32(const void* in, float* out, long long n, hipStream_t s);
int launch_rowstats(acx_ctx* c, const float* x, float* stats, int64_t M, int C, hipStream_t s);
// out[row] = (x[row] - mean) * rstd (no affine), rows of C channels; out may alias x
int launch_layernorm_rows(acx_ctx* c, const float* x, float* out, int64_t M, int C, hipStream_t s);
// out[M,N] = epi( LN?(A)[M,K] . Wt[N,K]^T + bias ).
enum GemmEpi { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2 };
struct GemmArgs {
    const float* A; const float* Wt; const float* bias; float* out;
    const float* stats;      // EPI_GELU: (M,2) mean/rstd of the A rows -- LayerNorm applied in the epilogue
    const float* colsum;     // EPI_GELU: (N) sum_k Wt[n][k]
    const float* resid;      // EPI_RESID: added to the result (may alias out)
    int64_t M; int N; int K;
    // 2x2 gather (downsample): A is NHWC (B,H,W,C) and row m=(b,h',w'), k=(dy*2+dx)*C+c
    const int* irow;        // gather, variable-length batch: VarGeom::irow of the output stage (null: uniform)
    int gather; int H, W, C, Ho, Wo;
    int epi; int cls;
};
int launch_gemm(acx_ctx* c, const GemmArgs& a, hipStream_t s);
// bf16-precision variants (gemm_bf16.hip): A, Wt bf16; EPI_GELU writes bf16, the others fp32
inline int pad64(int v) { return (v + 63) / 64 * 64; }
int launch_layernorm_rows_bf16(acx_ctx* c, const float* x, void* out, int64_t M, int C, hipStream_t s);
struct GemmBf16Args {
    const void* A; const void* Wt; const float* bias; void* out; const float* resid;
    int64_t M; int N; int Kp; int lda;
    const int* irow;        // gather, variable-length batch: VarGeom::irow of the output stage (null: uniform)
    int gather; int H, W, Cp, Ho, Wo;
    int epi; int cls;
    int out_bf16;            // EPI_BIAS only: write the result as bf16 (the next stage's bf16 activations)
};
int launch_gemm_bf16(acx_ctx* c, const GemmBf16Args& a, hipStream_t s);
// fp32 operands as two fp16 halves (gemm_split.hip): A, Wt in S16 form; EPI_GELU writes S16, the others fp32
constexpr float kSplitLnScale = 2048.0f;      // LayerNorm rows: |LN(y)| <= sqrt(C-1) < 28 -> < 2^15.8
// The GELU output (hidden activation) is scaled per block by BlockW::hid_scale, a power of two chosen at acx_finalize
// from a rigorous bound on |pwconv1 output| (weights.hip, hidden_scale_for): the fp16 range cannot be exceeded.
int launch_layernorm_rows_split(acx_ctx* c, const float* x, void* out, int64_t M, int C, hipStream_t s);
struct GemmSplitArgs {
    const void* A; const void* Wt; const float* bias; void* out; const float* resid;
    int64_t M; int N; int K; float sinv;
    float hscale;            // EPI_GELU: power-of-two scale of the S16 output
    const int* irow;        // gather, variable-length batch: VarGeom::irow of the output stage (null: uniform)
    int gather; int H, W, C, Ho, Wo;
    int epi; int cls;
};
int launch_gemm_split(acx_ctx* c, const GemmSplitArgs& a, hipStream_t s);
// The fused block MLPs below read their weights as one image each, built on the host by the kernel's *_pack function from the
// folded W1 [4C][C] and W2 [C][4C] (the S16 forms scaled by w1_scale / w2_scale).
bool mlp_fused_supported(int C);
// x += MLP(LN(y)) for one block, hidden activation kept in registers (mlp_fused.hip)
std::vector<float> mlp_fused_pack(const std::vector<float>& w1, const std::vector<float>& w2, int C);
int launch_mlp_fused(acx_ctx* c, const BlockW& w, int C, const float* y, float* x, long long M, hipStream_t s);
// ln_out != nullptr: do not write x; write LayerNorm(x_new) as S16 rows (the downsample GEMM's operand) there instead
bool mlp_fused_split_supported(int C);
std::vector<uint16_t> mlp_fused_split_pack(const std::vector<float>& w1, const std::vector<float>& w2, int C, float w1_scale,
                                           float w2_scale);
int launch_mlp_fused_split(acx_ctx* c, const BlockW& w, int C, const float* y, float* x, long long M, hipStream_t s,
                           void* ln_out = nullptr);
// the same for wide stages (C = 384, mlp_fused_wide.hip): one wave per SIMD, weights as one stream of segments
bool mlp_fused_wide_supported(int C);
std::vector<uint16_t> mlp_fused_wide_pack(const std::vector<float>& w1, const std::vector<float>& w2, int C, float w1_scale,
                                          float w2_scale);
int launch_mlp_fused_wide(acx_ctx* c, const BlockW& w, int C, const float* y, float* x, long long M, hipStream_t s,
                          void* ln_out = nullptr);
// bf16 arithmetic (mlp_fused_wide_bf16.hip): the fused block MLP for C = 96 / 192 / 384; ln_out (with row stride ld_out
// bf16 elements) receives LayerNorm(x_new) as bf16 rows INSTEAD of x when non-null
bool mlp_fused_wide_bf16_supported(int C);
std::vector<uint16_t> mlp_fused_wide_bf16_pack(const std::vector<float>& w1, const std::vector<float>& w2, int C);
int launch_mlp_fused_wide_bf16(acx_ctx* c, const BlockW& w, int C, const void* y, void* x, long long M, hipStream_t s,
                               void* ln_out = nullptr, int ld_out = 0, bool act_bf16 = false);
int launch_pool_head(acx_ctx* c, const float* x, int B, int H3, float* scene, float* logits, float* probs,
                     hipStream_t s);
// logits / probs (B, N) of B scene rows (B, 768) with the context's head: the class-tiled kernel, same bits as pool_head_kernel
int launch_head_tiled(acx_ctx* c, const float* scene, int B, float* logits, float* probs, hipStream_t s);
// the head path of a forward: true = pooling into scene rows + launch_head_tiled
bool head_tiled(const acx_ctx* c);
int launch_nhwc_to_nchw(acx_ctx* c, const float* x, float* out, int B, int H, int W, int C, hipStream_t s);
int launch_pcm16_to_f32(const short* in, float* out, long long n, hipStream_t s);

// variable-length forms (vg: tables of acx_forward_varlen; same arithmetic per element as the uniform kernels)
int launch_logmel_varlen(acx_ctx* c, const float* wav, const VarGeom& vg, float* out, hipStream_t s, float* dense_frames,
                         float* dense_spec);
int launch_stem_varlen(acx_ctx* c, const float* in, const VarGeom& vg, void* out, hipStream_t s, bool act_bf16, int max_blocks = 0);
int launch_dwconv_col_varlen(const void* x, void* y, const float* wt, const float* bias, void* sink, const VarGeom& vg, int stage,
                             int target_waves, hipStream_t s);
int launch_dwconv_mfma_varlen(const void* x, void* y, const void* dw_ops, const float* bias, void* sink, const VarGeom& vg,
                              int stage, int target_waves, hipStream_t s);
int launch_dwconv_varlen(acx_ctx* c, const BlockW& w, int C, const void* x, void* y, float* stats, const VarGeom& vg, int stage,
                         hipStream_t s, bool act_bf16, int target_waves = 0 /* 0: one wave per SIMD (fp32), ACX_DWM_WAVES per CU (bf16) */);
int launch_pool_head_varlen(acx_ctx* c, const float* x, const VarGeom& vg, float* scene, float* logits, float* probs,
                            hipStream_t s);
int launch_nhwc_to_nchw_varlen(acx_ctx* c, const float* x, float* out, const VarGeom& vg, hipStream_t s);
// the tables of vg (device pointers into `ws`) from the host lengths; bytes: their size (256-byte aligned)
int varlen_geometry(const int64_t* lengths, int B, char* ws, VarGeom* vg, size_t* bytes);
int launch_varlen_tables(const int64_t* lengths, const VarGeom& vg, hipStream_t s);

// ---- sliding windows (acx_forward_windows / acx_window_timeline, windows.hip) --------------------------------------------------
// R recordings of lengths[r] samples back to back; window j of recording r starts at min(j hop, max(0, L_r - window)) and the
// windows are numbered recording by recording.  Checks window / hop / R / lengths; *n_windows (may be null): their total.
int window_check(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t* n_windows);
// wstart[i] = absolute sample offset (into the packed recordings) of window first + i, i < count
int launch_window_table(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t first, int count, long long* wstart,
                        hipStream_t s);
int launch_window_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                           int reduce, float* out, hipStream_t s);

// (the window definition itself -- win_count, win_start, win_steps, win_mid, win_cover -- is packed.h's)

// ---- sound event detection (segments.hip; the segment timeline in windows.hip) ---------------------------------------------
constexpr int kSegSamples = ACX_SEGMENT_SAMPLES;
// segments of a clip of L samples: the stage-3 height ((T + 4) / 4 + 1) / 8 = (T + 8) / 32, T = L / 320 + 1
__host__ __device__ inline int seg_count(long long L) { return (int)((L / kHop + 1 + 8) / 32); }
// x NHWC (rows of 7 x 768) -> segment embeddings, one row of 768 per segment.  Uniform: B clips of S rows; roff3 != null: a
// variable-length batch of B clips, clip b owning rows [roff3[b], roff3[b + 1]) of x and of emb (maxS: the tallest clip)
int launch_segment_pool(acx_ctx* c, const float* x, int B, int S, int pool, float* emb, const int* roff3, int maxS, hipStream_t s);
// logits / probs (M, N) of M embedding rows with the context's head, on the f32 matrix cores
int launch_segment_head(acx_ctx* c, const float* emb, long long M, float* logits, float* probs, hipStream_t s);
// clip[b][n] = max_t probs[b][t][n]; roff3 as above
int launch_segment_clipmax(const float* probs, int B, int S, int N, float* clip, const int* roff3, hipStream_t s);
int launch_segment_expand(const float* probs, int B, int S, int N, int T, float* frame, hipStream_t s);
int launch_segment_expand_varlen(const float* probs, const int64_t* lengths, int B, int N, float* frame, hipStream_t s);
int launch_segment_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                            int reduce, float* out, hipStream_t s);

// ---- rows of fp32 vectors: the search and the clustering (knn.hip, kmeans.hip) ---------------------------------------------
inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
// at most this many rows or queries per call
constexpr long long kF32MaxRows = 1LL << 30;
// x non-null and 16-byte aligned, dim a multiple of 4 in 4 .. ACX_KNN_MAX_DIM, ld a multiple of 4 and at least dim (knn.hip)
int check_f32_rows(const char* who, const char* name, const float* x, int64_t ld, int dim);
// The k-means partition for the cluster scores (kmeans.hip; cluster_scores.hip): counts[k] = rows of label k, start[k] = rows of
// the labels below k, perm = the row indices sorted stably by label (ascending row inside a cluster); a label outside [0, K) is
// in no cluster and sets ACX_KMEANS_BAD_LABEL in *status.  hist: km_hist_bytes(n, K) bytes of scratch.
size_t km_hist_bytes(long long n, int K);
void km_launch_partition(const int* labels, long long n, int K, int* hist, int* counts, int* start, int* perm, int* status,
                         hipStream_t s);
// sums (K, dim) float64: each cluster's rows summed as acx_kmeans_update sums them (unweighted)
void km_launch_sums(const float* x, long long ld_x, int dim, int K, const int* perm, const int* start, const int* counts, double* sums,
                    hipStream_t s);

// ---- host code shared by api.hip, weights.hip, forward.hip and stream.hip ------------------------------------------------
// bf16 activations in HBM for the stages that keep them (ACX_PREC_BF16_ACT, stages 0-2)
inline bool act_bf16(const acx_ctx* c, int stage) { return c->precision == ACX_PREC_BF16_ACT && stage >= 0 && stage < 3; }
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
int need_ready(const acx_ctx* c);                     // api.hip: a context with finalized weights
void free_device(acx_ctx* c);                         // weights.hip: every device allocation of the context
int make_aux(acx_ctx::Aux* a);                        // forward.hip: one fork/join set of the batch split
void destroy_aux(acx_ctx::Aux& a);
// "workspace of %zu bytes is smaller than the %zu needed" / "must be 256-byte aligned", in that order
int check_workspace(const void* ptr, size_t bytes, size_t need);
// the stand-alone modules (metrics.hip, head_fit.hip, events.hip), which name the entry point: "<who>: workspace of %zu bytes,
// %zu needed" / "<who>: workspace is not 256-byte aligned", in that order
int check_workspace_for(const char* who, const void* ptr, size_t bytes, size_t need);
// The scratch of one block over pix pixels of C channels, carved from `off` on: y [pix][C], hidden [pix][4C], stats [pix][2]
// (fp32 each, 256-byte aligned); end = the first byte after it.
struct BlockScratch { size_t y, hidden, stats, end; };
inline BlockScratch carve_block_scratch(size_t pix, int C, size_t off) {
    BlockScratch b;
    b.y = off; off += align_up(pix * C * 4);
    b.hidden = off; off += align_up(pix * 4 * C * 4);
    b.stats = off; off += align_up(pix * 2 * 4);
    b.end = off;
    return b;
}
// The capacity of the three regions in bytes.  The forward carves them once, for stage 0, and every later stage -- and every
// tenant below -- lives in them; a per-layer entry point carves them for its own stage.  kNoCap: a capacity the caller cannot
// state (acx_downsample takes its scratch as a bare pointer).
constexpr size_t kNoCap = ~(size_t)0;
struct ScratchCap { size_t y, hidden, stats; };
inline ScratchCap scratch_cap(const BlockScratch& b) { return ScratchCap{b.hidden - b.y, b.stats - b.hidden, b.end - b.stats}; }

// ---- the tenants of the forward's workspace: what each needs, in bytes -------------------------------------------------------
// ONE definition each.  The driver (run_forward, run_block, run_downsample, carve_augmented) checks them against the capacity of
// the region they are lent, on the host and before the first launch; acx_test_forward_plan reports the same numbers, and
// tests/test_forward_plan_cpu.py sweeps them over every shape ("The workspace plan").
// the dense-DFT frontend's frames [n][1024] and spectrum [n][kDenseN], fp32, of n mel frames
inline size_t need_dense_frames(size_t n) { return n * kNFFT * 4; }
inline size_t need_dense_spec(size_t n) { return n * kDenseN * 4; }
// the LayerNorm rows the last block of a stage hands the downsample GEMM: S16 (two fp16 halves per element) or bf16 rows padded
// to 64 channels, M pixels of C channels
inline size_t need_ln_rows(int precision, size_t M, int C) {
    return precision == ACX_PREC_F32_SPLIT ? M * C * 4 : M * (size_t)pad64(C) * 2;
}
// run_mlp_bf16: the bf16 hidden activation [M][4C] at offset 0, then the bf16 LayerNorm rows [M][Cp] behind it
inline size_t need_mlp_bf16_hidden(size_t M, int C) { return M * 4 * C * 2; }
inline size_t need_mlp_bf16_rows(size_t M, int C) { return M * (size_t)pad64(C) * 2; }
inline size_t mlp_bf16_rows_offset(size_t M, int C) { return align_up(need_mlp_bf16_hidden(M, C)); }
// the two-GEMM MLP of the fp32 arithmetics: the hidden activation [M][4C] (fp32, or S16 of the same size), the LayerNorm
// statistics [M][2] (fp32 only)
inline size_t need_hidden_act(size_t M, int C) { return M * 4 * C * 4; }
inline size_t need_row_stats(size_t M) { return M * 2 * 4; }
// the downsample's normalised input rows when no block wrote them: fp32 / S16 [M][C], bf16 [M][Cp]
inline size_t need_xnorm(int precision, size_t M, int C) {
    return precision == ACX_PREC_F32 || precision == ACX_PREC_F32_SPLIT ? M * C * 4 : M * (size_t)pad64(C) * 2;
}
// acx_block under ACX_PREC_BF16_ACT: the block's x as bf16 [pix][C], lent the `hidden` scratch of its own stage
inline size_t need_act_bf16(size_t pix, int C) { return pix * C * 2; }
// the segment tail's embeddings [rows][768] and the class-tiled head's scene rows [B][768], fp32
inline size_t need_segment_emb(size_t rows) { return rows * kDims[3] * 4; }
inline size_t need_scene_rows(size_t B) { return B * kDims[3] * 4; }
// one block / one downsample layer (forward.hip), shared by the forward and the per-layer entry points
// vg: a variable-length batch (acx_forward_varlen) -- B = 1 and H = the stage's total rows then, so that M counts every pixel;
// only the depthwise conv needs the per-clip tables
// cap: the bytes y, hidden and stats hold -- the block's tenants are checked against it before anything is launched
int run_block(acx_ctx* c, int s, int j, float* x, float* y, float* hidden, float* stats, const ScratchCap& cap, int B, int H, int Wd,
              hipStream_t st, void* ln_out = nullptr, const VarGeom* vg = nullptr);
// the last block of stage s can write the downsample conv's operand rows (ln_out) instead of x
bool block_can_emit_ln(const acx_ctx* c, int s);
// have_ln: xnorm already holds the normalised S16 rows (written by the last block of the previous stage)
// out_bf16: the result is the bf16 activation tensor of stage i (ACX_PREC_BF16_ACT inside acx_forward; the per-layer entry
// point keeps fp32)
// vg: a variable-length batch -- B = 1 and H = the input stage's total rows; the output rows and the gather come from the tables
// (a clip of odd height drops its last row, as the stride-2 conv does)
// xnorm_cap: the bytes xnorm holds (kNoCap: unknown to the caller)
int run_downsample(acx_ctx* c, int i, const float* x, float* out, float* xnorm, size_t xnorm_cap, int B, int H, int Wd,
                   hipStream_t st, bool have_ln = false, bool out_bf16 = false, const VarGeom* vg = nullptr);
// The carve-up of acx_forward_augmented's workspace (augment.hip): the augmented waveform (with a waveform plan), the feature map
// of all B clips, the mixed map of B / 2 clips (with lambdas), the dense-DFT frontend's frames and spectrum of B clips (dense: a
// context whose frontend is the dense contraction; need_dense_frames / need_dense_spec), then the workspace of the forward over
// the clips that remain (fwd bytes from `fwd` on).
struct AugWs { size_t wave, feat, mix, frames, spec, fwd, total; };
int carve_augmented(bool dense, int B, int64_t L, bool wave, bool lam, int mode, AugWs* w);
// its five regions (ACX_PLAN_AUG_WAVE ..) and the tenants of its own frontend (`frames` mel frames), shared by driver and hook
struct AugFront { acx_plan_region_t regions[5]; int n_tenants; acx_plan_tenant_t tenants[2]; };
void augmented_front(const AugWs& w, bool dense, size_t frames, AugFront* f);
// The uniform forward of B clips of L samples with the batch split (acx_forward; arguments checked by the caller).  wstart: the
// window table of acx_forward_windows / acx_stream_forward, written on `st` by the caller -- clip b's samples start at
// wav + wstart[b], sub-batch i gets its slice of the table and the whole of wav.  seg: the segment tail instead of `mode`'s.
// feat_in: the (B, T, 224) bn0'd log-mel rows of the batch, given by the caller (acx_forward_features; wav is null then): the
// frontend launch is skipped and sub-batch i's stem reads its slice of them.
struct SegTail;
int forward_uniform(acx_ctx* c, const float* wav, int B, int64_t L, int mode, float* out0, float* out1, char* ws, hipStream_t st,
                    const long long* wstart, const SegTail* seg = nullptr, const float* feat_in = nullptr, bool plans_checked = false);
// ACX_ERR_STATE when a tenant of the plans forward_uniform would run for this batch (unsplit and split) does not fit its region.
// Host arithmetic.  forward_uniform calls it first thing; a driver that launches something of its own in front of forward_uniform
// calls it before that and passes plans_checked = true, so that every plan is checked once and before anything is launched.
int check_uniform_plans(const acx_ctx* c, int B, int64_t L, int mode, const SegTail* seg, bool feat_in);
// null pointers / mode / logits-needs-out1, in the entry points' words (forward.hip)
int check_forward_args(const char* who, const void* wav, const float* out0, const float* out1, const void* ws, int mode);

// number of CUs of the current device (one persistent workgroup each), cached per device
inline int cu_count_of_current_device(int* out) {
    static std::atomic<int> cache[64];
    int dev = 0;
    ACX_HIP(hipGetDevice(&dev));
    int v = cache[dev & 63].load(std::memory_order_acquire);
    if (v == 0) {
        ACX_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        if (v <= 0) ACX_FAIL(ACX_ERR_HIP, "device %d reports %d compute units", dev, v);
        cache[dev & 63].store(v, std::memory_order_release);
    }
    *out = v;
    return ACX_OK;
}

}  // namespace acx
