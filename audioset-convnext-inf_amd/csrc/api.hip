// libacx C ABI: context lifetime, the setters, the per-layer entry points, tuning and event profiling.  Weight intake is in
// weights.hip, the forward driver in forward.hip.  See include/acx.h for the contract and the reference interfaces each entry
// point stands in for.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "acx_internal.h"

namespace acx {

static thread_local char g_err[512] = "";

Tuning& tuning() {
    static Tuning t;
    return t;
}
void tuning_reload() {
    auto digit = [](const char* name, const char* allowed, int none) {
        const char* e = std::getenv(name);
        if (!e || !e[0] || e[1] || !std::strchr(allowed, e[0])) return none;
        return e[0] - '0';
    };
    Tuning& t = tuning();
    t.gemm_mi.store(digit("ACX_GEMM_MI", "124", 0), std::memory_order_relaxed);
    t.wide_npb.store(digit("ACX_WIDE_NPB", "12", 0), std::memory_order_relaxed);
    t.wide_pers.store(digit("ACX_WIDE_PERSIST", "01", -1) < 0 ? 0 : (digit("ACX_WIDE_PERSIST", "01", 0) == 1 ? 1 : 2), std::memory_order_relaxed);
    t.dw_stream.store(digit("ACX_DW_STREAM", "01", -1), std::memory_order_relaxed);
    t.dwm_waves.store(digit("ACX_DWM_WAVES", "23456789", 0), std::memory_order_relaxed);
    t.head_path.store(digit("ACX_HEAD_PATH", "12", 0), std::memory_order_relaxed);
    const char* sr = std::getenv("ACX_KNN_SLICE_ROWS");
    const long srv = sr && sr[0] ? std::strtol(sr, nullptr, 10) : 0;
    t.knn_slice_rows.store(srv >= 16 && srv <= (1L << 30) ? (int)srv : 0, std::memory_order_relaxed);
    const char* mr = std::getenv("ACX_MOMENTS_SLICE_ROWS");
    const long mrv = mr && mr[0] ? std::strtol(mr, nullptr, 10) : 0;
    t.moments_slice_rows.store(mrv >= 16 && mrv <= (1L << 30) ? (int)mrv : 0, std::memory_order_relaxed);
}

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local ProfScope* g_prof_scope = nullptr;

ProfScope::ProfScope(acx_ctx* c, int k, hipStream_t st) : ctx(c), cls(k), s(st), prev(g_prof_scope) {
    if (!ctx || !ctx->prof.on || cls < 0) ctx = nullptr;      // (an inner scope without a class keeps the outer one's)
    if (ctx) g_prof_scope = this;
}
ProfScope::~ProfScope() {
    if (ctx) g_prof_scope = prev;
}

void prof_next_events(hipEvent_t* a, hipEvent_t* b) {
    ProfScope* sc = g_prof_scope;
    if (!sc) return;
    acx_ctx* ctx = sc->ctx;
    auto get = [&]() {
        hipEvent_t e;
        if (!ctx->prof.pool.empty()) { e = ctx->prof.pool.back(); ctx->prof.pool.pop_back(); }
        else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        return e;
    };
    *a = get(); *b = get();
    if (!*a || !*b) { if (*a) ctx->prof.pool.push_back(*a); if (*b) ctx->prof.pool.push_back(*b); *a = *b = nullptr; return; }
    ctx->prof.recs.push_back({sc->cls, *a, *b});
}

int need_ready(const acx_ctx* c) {
    if (!c) ACX_FAIL(ACX_ERR_ARG, "null context");
    if (!c->finalized) ACX_FAIL(ACX_ERR_STATE, "weights not finalized: call acx_set_weight for every key, then acx_finalize");
    return ACX_OK;
}

static int check_stage(int stage, int block) {
    if (stage < 0 || stage > 3 || block < 0 || block >= kDepths[stage])
        ACX_FAIL(ACX_ERR_ARG, "no block %d in stage %d", block, stage);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

const char* acx_last_error(void) { return g_err; }
int acx_version(void) { return 101; }

int acx_create(int hip_device, acx_ctx** out) {
    if (!out) ACX_FAIL(ACX_ERR_ARG, "acx_create: out is null");
    int n = 0;
    ACX_HIP(hipGetDeviceCount(&n));
    if (hip_device < 0 || hip_device >= n) ACX_FAIL(ACX_ERR_ARG, "acx_create: device %d out of range (%d visible)", hip_device, n);
    hipDeviceProp_t prop;
    ACX_HIP(hipGetDeviceProperties(&prop, hip_device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "acx_create: device %d is %s; this library is built for gfx950 (MI355X) only",
                 hip_device, prop.gcnArchName);
    acx_ctx* c = new acx_ctx();
    c->device = hip_device;
    ACX_HIP(hipSetDevice(hip_device));
    {
        const char* e = std::getenv("ACX_SPLIT_STREAMS");
        c->split_streams = !(e && e[0] == '0');
        const char* e2 = std::getenv("ACX_SPLIT_WAYS");
        if (e2 && e2[0] >= '1' && e2[0] <= '0' + acx_ctx::kMaxSplitWays && e2[1] == 0) c->split_ways = e2[0] - '0';
    }
    {   // the null stream's side stream + events exist from the start (nothing is created inside a capture)
        acx_ctx::AuxEntry e;
        int rc = make_aux(&e.a);
        if (rc != ACX_OK) { delete c; return rc; }
        c->aux.emplace((hipStream_t) nullptr, e);
    }
    {
        static std::once_flag env_once;
        std::call_once(env_once, tuning_reload);
    }
    *out = c;
    return ACX_OK;
}

void acx_destroy(acx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    free_device(c);
    for (auto& r : c->prof.recs) { if (r.a) (void)hipEventDestroy(r.a); if (r.b) (void)hipEventDestroy(r.b); }
    for (auto e : c->prof.pool) (void)hipEventDestroy(e);
    for (auto& kv : c->aux) destroy_aux(kv.second.a);
    for (auto& a : c->aux_retired) destroy_aux(a);
    comm_release(c);
    delete c;
}

int acx_num_classes(const acx_ctx* c, int* n) {
    ACX_TRY(need_ready(c));
    if (!n) ACX_FAIL(ACX_ERR_ARG, "acx_num_classes: n is null");
    *n = c->num_classes;
    return ACX_OK;
}

int acx_set_precision(acx_ctx* c, int precision) {
    if (!c) ACX_FAIL(ACX_ERR_ARG, "null context");
    if (precision != ACX_PREC_F32 && precision != ACX_PREC_BF16 && precision != ACX_PREC_F32_SPLIT && precision != ACX_PREC_BF16_ACT) ACX_FAIL(ACX_ERR_ARG, "acx_set_precision: unknown precision %d", precision);
    if (precision != c->precision) { c->precision = precision; c->finalized = false; }
    return ACX_OK;
}

int acx_set_frontend(acx_ctx* c, int mode) {
    if (!c) ACX_FAIL(ACX_ERR_ARG, "null context");
    if (mode != ACX_FRONTEND_AUTO && mode != ACX_FRONTEND_DENSE) ACX_FAIL(ACX_ERR_ARG, "acx_set_frontend: unknown mode %d", mode);
    const bool dense = mode == ACX_FRONTEND_DENSE;
    if (dense == c->force_dense_stft) return ACX_OK;
    c->force_dense_stft = dense;
    return c->finalized ? acx_finalize(c) : ACX_OK;
}

int acx_num_frames(int64_t L, int* T) {
    if (!T || L < 0) ACX_FAIL(ACX_ERR_ARG, "acx_num_frames: bad argument");
    *T = (int)(L / kHop + 1);
    return ACX_OK;
}

int acx_logmel_bn0(acx_ctx* c, const float* wav, int B, int64_t L, float* out, int apply_bn0, void* stream) {
    ACX_TRY(need_ready(c));
    if (!wav || !out || B <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_logmel_bn0: bad argument");
    if (L < kNFFT / 2 + 1) ACX_FAIL(ACX_ERR_SHAPE, "reflect padding needs at least %d samples (got %lld)", kNFFT / 2 + 1, (long long)L);
    return launch_logmel(c, wav, B, L, (int)(L / kHop + 1), out, apply_bn0 != 0, (hipStream_t)stream);
}

int acx_stem_ln(acx_ctx* c, const float* in, int B, int T, float* out, void* stream) {
    ACX_TRY(need_ready(c));
    if (!in || !out || B <= 0 || T <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_stem_ln: bad argument");
    return launch_stem(c, in, B, T, stage_h0(T), out, (hipStream_t)stream);
}

int acx_dwconv7(acx_ctx* c, int stage, int block, const float* x, float* y, float* stats, int B, int H, int Wd, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_stage(stage, block));
    if (!x || !y || B <= 0 || H <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_dwconv7: bad argument");
    if (Wd != (kStemW >> stage)) ACX_FAIL(ACX_ERR_SHAPE, "stage %d has width %d, got %d", stage, kStemW >> stage, Wd);
    return launch_dwconv(c, c->blocks[stage][block], kDims[stage], x, y, stats, B, H, Wd, (hipStream_t)stream);
}

int acx_dwconv7_bf16(acx_ctx* c, int stage, int block, const uint16_t* x, uint16_t* y, int B, int H, int Wd, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_stage(stage, block));
    if (!x || !y || B <= 0 || H <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_dwconv7_bf16: bad argument");
    if (!act_bf16(c, stage)) ACX_FAIL(ACX_ERR_STATE, "acx_dwconv7_bf16: stage %d does not store bf16 activations at this precision", stage);
    if (Wd != (kStemW >> stage)) ACX_FAIL(ACX_ERR_SHAPE, "stage %d has width %d, got %d", stage, kStemW >> stage, Wd);
    return launch_dwconv(c, c->blocks[stage][block], kDims[stage], x, y, nullptr, B, H, Wd, (hipStream_t)stream, true);
}

int acx_block_scratch_bytes(int stage, int B, int H, int Wd, size_t* out_bytes) {
    if (!out_bytes || stage < 0 || stage > 3 || B <= 0 || H <= 0 || Wd <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_block_scratch_bytes: bad argument");
    *out_bytes = carve_block_scratch((size_t)B * H * Wd, kDims[stage], 0).end;
    return ACX_OK;
}

int acx_block(acx_ctx* c, int stage, int block, float* x, int B, int H, int Wd, void* scratch, size_t scratch_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_stage(stage, block));
    if (!x || !scratch) ACX_FAIL(ACX_ERR_ARG, "acx_block: null pointer");
    if (Wd != (kStemW >> stage)) ACX_FAIL(ACX_ERR_SHAPE, "stage %d has width %d, got %d", stage, kStemW >> stage, Wd);
    size_t need = 0;
    ACX_TRY(acx_block_scratch_bytes(stage, B, H, Wd, &need));
    if (scratch_bytes < need || ((uintptr_t)scratch & 255)) ACX_FAIL(ACX_ERR_WORKSPACE, "acx_block: scratch too small (%zu < %zu) or misaligned", scratch_bytes, need);
    const size_t pix = (size_t)B * H * Wd;
    char* ws = (char*)scratch;
    const BlockScratch b = carve_block_scratch(pix, kDims[stage], 0);
    float* y = (float*)(ws + b.y);
    float* hidden = (float*)(ws + b.hidden);
    float* stats = (float*)(ws + b.stats);
    if (act_bf16(c, stage)) {
        // The ABI keeps fp32 tensors; the block itself runs on bf16 activations: x is rounded to bf16 into the hidden scratch
        // (need_act_bf16; the fused MLP of stages 0-2 puts nothing there: run_block has no tenant of `hidden` without ln_out),
        // dwconv + fused MLP read and write bf16 there, and the result is widened back into x.
        const long long n = (long long)pix * kDims[stage];
        if (need_act_bf16(pix, kDims[stage]) > scratch_cap(b).hidden)
            ACX_FAIL(ACX_ERR_STATE, "acx_block: the bf16 copy of x needs %zu bytes of `hidden`, which holds %zu", need_act_bf16(pix, kDims[stage]),
                     scratch_cap(b).hidden);
        ACX_TRY(launch_convert_f32_to_bf16(x, hidden, n, (hipStream_t)stream));
        ACX_TRY(run_block(c, stage, block, hidden, y, hidden, stats, scratch_cap(b), B, H, Wd, (hipStream_t)stream));
        return launch_convert_bf16_to_f32(hidden, x, n, (hipStream_t)stream);
    }
    return run_block(c, stage, block, x, y, hidden, stats, scratch_cap(b), B, H, Wd, (hipStream_t)stream);
}

int acx_downsample(acx_ctx* c, int i, const float* x, float* out, float* scratch, int B, int H, int Wd, void* stream) {
    ACX_TRY(need_ready(c));
    if (i < 1 || i > 3) ACX_FAIL(ACX_ERR_ARG, "acx_downsample: layer index %d (expected 1..3)", i);
    if (!x || !out || !scratch || B <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_downsample: bad argument");
    if (H < 2 || Wd < 2) ACX_FAIL(ACX_ERR_SHAPE, "acx_downsample: kernel size can't be greater than actual input size (%dx%d)", H, Wd);
    return run_downsample(c, i, x, out, scratch, kNoCap, B, H, Wd, (hipStream_t)stream);      // (the ABI passes no size)
}

int acx_pool_head(acx_ctx* c, const float* x, int B, int H3, float* scene, float* logits, float* probs, void* stream) {
    ACX_TRY(need_ready(c));
    if (!x || B <= 0 || H3 <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_pool_head: bad argument");
    return launch_pool_head(c, x, B, H3, scene, logits, probs, (hipStream_t)stream);
}

int acx_nhwc_to_nchw(const float* x, float* out, int B, int H, int Wd, int C, void* stream) {
    if (!x || !out || B <= 0 || H <= 0 || Wd <= 0 || C <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_nhwc_to_nchw: bad argument");
    return launch_nhwc_to_nchw(nullptr, x, out, B, H, Wd, C, (hipStream_t)stream);
}

int acx_pcm16_to_f32(const int16_t* pcm, float* out, int64_t n, void* stream) {
    if (!pcm || !out || n < 0) ACX_FAIL(ACX_ERR_ARG, "acx_pcm16_to_f32: bad argument");
    if (n == 0) return ACX_OK;
    return launch_pcm16_to_f32(pcm, out, n, (hipStream_t)stream);
}

int acx_frontend_info(const acx_ctx* c, int* dense_dft, float* stft_deviation, int* mel_taps) {
    ACX_TRY(need_ready(c));
    if (dense_dft) *dense_dft = c->dense_stft ? 1 : 0;
    if (stft_deviation) *stft_deviation = c->stft_deviation;
    if (mel_taps) *mel_taps = c->mel_w_len;
    return ACX_OK;
}

int acx_tuning_refresh(void) {
    tuning_reload();
    return ACX_OK;
}

int acx_test_fail_sub(acx_ctx* c, int sub) {
    if (!c) ACX_FAIL(ACX_ERR_ARG, "null context");
    if (sub < -1 || sub >= acx_ctx::kMaxSplitWays) ACX_FAIL(ACX_ERR_ARG, "acx_test_fail_sub: sub-batch index %d", sub);
    c->fail_sub.store(sub, std::memory_order_relaxed);
    return ACX_OK;
}

// Scratch of acx_test_stage_tail: the block scratch of the stage, then a bf16 image of x and one of the downsample's output (the
// storage types of ACX_PREC_BF16_ACT; sized whatever the precision: the size call has no context).
struct TailScratch { BlockScratch blk; size_t xb, outb, end; };
static TailScratch carve_tail_scratch(int stage, size_t B, size_t H, size_t Wd) {
    TailScratch t;
    const size_t pix = B * H * Wd;
    t.blk = carve_block_scratch(pix, kDims[stage], 0);
    size_t off = t.blk.end;
    t.xb = off; off += align_up(pix * kDims[stage] * 2);
    t.outb = off; off += align_up(B * (H / 2) * (Wd / 2) * kDims[stage + 1] * 2);
    t.end = off;
    return t;
}

int acx_test_stage_tail_scratch_bytes(int stage, int B, int H, int Wd, size_t* out_bytes) {
    if (!out_bytes || stage < 0 || stage > 2 || B <= 0 || H <= 0 || Wd <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_stage_tail_scratch_bytes: bad argument");
    *out_bytes = carve_tail_scratch(stage, (size_t)B, (size_t)H, (size_t)Wd).end;
    return ACX_OK;
}

int acx_test_stage_tail(acx_ctx* c, int stage, float* x, float* out, int B, int H, int Wd, void* scratch, size_t scratch_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    if (stage < 0 || stage > 2) ACX_FAIL(ACX_ERR_ARG, "acx_test_stage_tail: stage %d (expected 0..2)", stage);
    if (!x || !out || !scratch || B <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_stage_tail: bad argument");
    if (Wd != (kStemW >> stage)) ACX_FAIL(ACX_ERR_SHAPE, "stage %d has width %d, got %d", stage, kStemW >> stage, Wd);
    if (H < 2) ACX_FAIL(ACX_ERR_SHAPE, "acx_test_stage_tail: kernel size can't be greater than actual input size (%dx%d)", H, Wd);
    const TailScratch t = carve_tail_scratch(stage, (size_t)B, (size_t)H, (size_t)Wd);
    if (scratch_bytes < t.end || ((uintptr_t)scratch & 255)) ACX_FAIL(ACX_ERR_WORKSPACE, "acx_test_stage_tail: scratch too small (%zu < %zu) or misaligned", scratch_bytes, t.end);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)scratch;
    float* y = (float*)(ws + t.blk.y);
    float* hidden = (float*)(ws + t.blk.hidden);
    float* stats = (float*)(ws + t.blk.stats);
    const int last = kDepths[stage] - 1;
    // as run_forward: the LayerNorm rows go to `hidden`; without them the downsample normalises x into y
    const bool have_ln = block_can_emit_ln(c, stage);
    float* xs = x;
    if (act_bf16(c, stage)) {       // the stage's x as stored: bf16, in a region of its own (`hidden` takes the LayerNorm rows here)
        xs = (float*)(ws + t.xb);
        ACX_TRY(launch_convert_f32_to_bf16(x, xs, (long long)B * H * Wd * kDims[stage], st));
    }
    const ScratchCap cap = scratch_cap(t.blk);
    ACX_TRY(run_block(c, stage, last, xs, y, hidden, stats, cap, B, H, Wd, st, have_ln ? (void*)hidden : nullptr));
    const bool ob = act_bf16(c, stage + 1);
    float* os = ob ? (float*)(ws + t.outb) : out;
    ACX_TRY(run_downsample(c, stage + 1, xs, os, have_ln ? hidden : y, have_ln ? cap.hidden : cap.y, B, H, Wd, st, have_ln, ob));
    if (ob) return launch_convert_bf16_to_f32(os, out, (long long)B * (H / 2) * (Wd / 2) * kDims[stage + 1], st);
    return ACX_OK;
}

static void export_plan(const DwColPlan& p, acx_dwconv7_plan_t* out) {
    out->n_out = p.n_out; out->s0 = p.s0; out->k7 = p.k7; out->n_seg = p.n_seg; out->n_items = p.n_items;
}

int acx_test_dwconv7_plan(int stage, int B, int H, int target_waves, acx_dwconv7_plan_t* plan) {
    if (!plan || stage < 0 || stage > 3 || B <= 0 || H <= 0 || target_waves <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_plan: bad argument");
    DwColPlan p;
    ACX_TRY(dwconv_col_plan(kStemW >> stage, B, H, target_waves, &p));
    export_plan(p, plan);
    return ACX_OK;
}

int acx_test_dwconv7_varlen_plan(int stage, const int64_t* lengths, int n, int target_waves, acx_dwconv7_plan_t* plan) {
    if (!plan || stage < 0 || stage > 3 || target_waves <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_varlen_plan: bad argument");
    VarGeom vg;
    size_t bytes = 0;
    ACX_TRY(varlen_geometry(lengths, n, nullptr, &vg, &bytes));
    DwColPlan p;
    ACX_TRY(dwconv_col_plan_varlen(stage, vg.vrows[stage], target_waves, &p));
    export_plan(p, plan);
    return ACX_OK;
}

int acx_test_dwconv7_form(acx_ctx* c, int stage, int block, const float* x, float* y, float* stats, int B, int H, int Wd, int form,
                          int target_waves, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_stage(stage, block));
    if (!x || !y || B <= 0 || H <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_form: bad argument");
    if (Wd != (kStemW >> stage)) ACX_FAIL(ACX_ERR_SHAPE, "stage %d has width %d, got %d", stage, kStemW >> stage, Wd);
    if (form != 0 && form != 1) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_form: form %d (expected 0: ring / tile, 1: column)", form);
    if (form == 1) {
        int cus = 0;
        ACX_TRY(cu_count_of_current_device(&cus));
        if (target_waves < 1 || target_waves > 4 * cus)
            ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_form: target_waves %d (expected 1 .. %d)", target_waves, 4 * cus);
        if (dw_col_too_tall(B, H)) ACX_FAIL(ACX_ERR_SHAPE, "acx_test_dwconv7_form: batch too tall for the column kernel (%d clips of %d rows)", B, H);
    }
    return launch_dwconv_form(c, c->blocks[stage][block], kDims[stage], x, y, stats, B, H, Wd, form == 1, target_waves, (hipStream_t)stream);
}

static void export_plan(const DwMfmaPlan& p, bool too_tall, acx_dwconv7_bf16_plan_t* out) {
    out->rows = p.rows; out->steps = p.steps; out->n_seg = p.n_seg; out->n_groups = p.n_groups; out->grid = p.grid;
    out->too_tall = too_tall ? 1 : 0;
}

int acx_test_dwconv7_bf16_plan(int stage, int B, int H, int target_waves, acx_dwconv7_bf16_plan_t* plan) {
    if (!plan || stage < 0 || stage > 2 || B <= 0 || H <= 0 || target_waves <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_bf16_plan: bad argument");
    DwMfmaPlan p;
    ACX_TRY(dw_mfma_segments(kStemW >> stage, (long long)B * (H + 3) - 3, target_waves, &p));
    export_plan(p, dw_mfma_too_tall(B, H), plan);
    return ACX_OK;
}

int acx_test_dwconv7_bf16_varlen_plan(int stage, const int64_t* lengths, int n, int target_waves, acx_dwconv7_bf16_plan_t* plan) {
    if (!plan || stage < 0 || stage > 2 || target_waves <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_bf16_varlen_plan: bad argument");
    VarGeom vg;
    size_t bytes = 0;
    ACX_TRY(varlen_geometry(lengths, n, nullptr, &vg, &bytes));
    DwMfmaPlan p;
    ACX_TRY(dw_mfma_segments(kStemW >> stage, (long long)vg.vrows[stage] - 3, target_waves, &p));
    export_plan(p, false, plan);       // the packed kernel divides nothing: its cursors read the row tables
    return ACX_OK;
}

int acx_test_dwconv7_bf16_form(acx_ctx* c, int stage, int block, const uint16_t* x, uint16_t* y, int B, int H, int Wd, int target_waves,
                               void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_stage(stage, block));
    if (!x || !y || B <= 0 || H <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_bf16_form: bad argument");
    if (!act_bf16(c, stage)) ACX_FAIL(ACX_ERR_STATE, "acx_test_dwconv7_bf16_form: stage %d does not store bf16 activations at this precision", stage);
    if (Wd != (kStemW >> stage)) ACX_FAIL(ACX_ERR_SHAPE, "stage %d has width %d, got %d", stage, kStemW >> stage, Wd);
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));
    if (target_waves < 1 || target_waves > 9 * cus)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_bf16_form: target_waves %d (expected 1 .. %d)", target_waves, 9 * cus);
    return launch_dwconv(c, c->blocks[stage][block], kDims[stage], x, y, nullptr, B, H, Wd, (hipStream_t)stream, true, target_waves);
}

int acx_test_dwconv7_varlen_scratch_bytes(const int64_t* lengths, int n, size_t* out_bytes) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_varlen_scratch_bytes: bad argument");
    VarGeom vg;
    return varlen_geometry(lengths, n, nullptr, &vg, out_bytes);
}

int acx_test_dwconv7_varlen(acx_ctx* c, int stage, int block, const void* x, void* y, const int64_t* lengths, int n, int target_waves,
                            void* scratch, size_t scratch_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_stage(stage, block));
    if (!x || !y || !scratch) ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_varlen: null pointer");
    int cus = 0;
    ACX_TRY(cu_count_of_current_device(&cus));
    const bool ab = act_bf16(c, stage);
    const int max_waves = (ab ? 9 : 8) * cus;      // bf16 activations: the matrix-pipe kernel, up to ACX_DWM_WAVES = 9 per CU
    if (target_waves < 1 || target_waves > max_waves)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_dwconv7_varlen: target_waves %d (expected 1 .. %d)", target_waves, max_waves);
    VarGeom vg;
    size_t need = 0;
    ACX_TRY(varlen_geometry(lengths, n, (char*)scratch, &vg, &need));
    if (scratch_bytes < need || ((uintptr_t)scratch & 255))
        ACX_FAIL(ACX_ERR_WORKSPACE, "acx_test_dwconv7_varlen: scratch too small (%zu < %zu) or misaligned", scratch_bytes, need);
    if (ab && stage > 2) ACX_FAIL(ACX_ERR_STATE, "acx_test_dwconv7_varlen: no bf16 activations in stage %d", stage);
    ACX_TRY(launch_varlen_tables(lengths, vg, (hipStream_t)stream));
    return launch_dwconv_varlen(c, c->blocks[stage][block], kDims[stage], x, y, nullptr, vg, stage, (hipStream_t)stream, ab, target_waves);
}

int acx_test_stem_scratch_bytes(const int64_t* lengths, int n, size_t* out_bytes, int64_t* out_rows) {
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "acx_test_stem_scratch_bytes: bad argument");
    VarGeom vg;
    ACX_TRY(varlen_geometry(lengths, n, nullptr, &vg, out_bytes));
    if (out_rows) *out_rows = vg.rows[0];
    return ACX_OK;
}

int acx_test_stem(acx_ctx* c, const float* feat, void* out, int B, int T, const int64_t* lengths, int n, int max_blocks, void* scratch,
                  size_t scratch_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    if (!feat || !out) ACX_FAIL(ACX_ERR_ARG, "acx_test_stem: null pointer");
    if (max_blocks < 0 || max_blocks > kStemMaxBlocks)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_stem: max_blocks %d (expected 0: the launcher's grid, or 1 .. %d)", max_blocks, kStemMaxBlocks);
    const bool ab = act_bf16(c, 0);
    if (!lengths && n == 0) {
        if (B < 1 || T < 1) ACX_FAIL(ACX_ERR_ARG, "acx_test_stem: %d clips of %d frames", B, T);
        return launch_stem(c, feat, B, T, stage_h0(T), out, (hipStream_t)stream, ab, max_blocks);
    }
    if (!scratch) ACX_FAIL(ACX_ERR_ARG, "acx_test_stem: null pointer");
    VarGeom vg;
    size_t need = 0;
    ACX_TRY(varlen_geometry(lengths, n, (char*)scratch, &vg, &need));
    if (scratch_bytes < need || ((uintptr_t)scratch & 255))
        ACX_FAIL(ACX_ERR_WORKSPACE, "acx_test_stem: scratch too small (%zu < %zu) or misaligned", scratch_bytes, need);
    ACX_TRY(launch_varlen_tables(lengths, vg, (hipStream_t)stream));
    return launch_stem_varlen(c, feat, vg, out, (hipStream_t)stream, ab, max_blocks);
}

int acx_profile_enable(acx_ctx* c, int on) {
    if (!c) ACX_FAIL(ACX_ERR_ARG, "null context");
    c->prof.on = on != 0;
    return ACX_OK;
}

int acx_profile_read(acx_ctx* c, double* ms, int64_t* launches) {
    if (!c || !ms || !launches) ACX_FAIL(ACX_ERR_ARG, "acx_profile_read: null argument");
    for (int k = 0; k < ACX_K_COUNT; ++k) { ms[k] = 0.0; launches[k] = 0; }
    for (auto& r : c->prof.recs) {
        if (r.a && r.b) {
            ACX_HIP(hipEventSynchronize(r.b));
            float t = 0.f;
            ACX_HIP(hipEventElapsedTime(&t, r.a, r.b));
            if (r.cls >= 0 && r.cls < ACX_K_COUNT) { ms[r.cls] += t; launches[r.cls] += 1; }
        }
        if (r.a) c->prof.pool.push_back(r.a);
        if (r.b) c->prof.pool.push_back(r.b);
    }
    c->prof.recs.clear();
    return ACX_OK;
}

}  // extern "C"
