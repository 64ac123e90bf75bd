// libacx forward driver: workspace plans, the side-stream pool of the batch split, the trunk and tail of the forward, and the
// forward / varlen / windows / segments entry points.  Host code only.
#include <cstring>

#include "acx_internal.h"

namespace acx {

thread_local int tls_inflight_ways = 1;

// What the trunk runs over.  Uniform: B clips of L samples, T frames and Hs[s] rows at stage s each.  Variable-length (vg): the B
// packed clips of vg, T and Hs[s] the sums over the clips (vg->frames, vg->rows[s]).  wstart: windows (acx_forward_windows,
// uniform only) -- clip b's samples start at wav + wstart[b] (device table), not at wav + b L.
struct Geom {
    int B, T, Hs[4];
    int64_t L;
    const VarGeom* vg;
    const long long* wstart;
};

struct Plan {          // the geometry of one forward and its workspace carve-up: feat, x of the four stages, the block scratch
    Geom g;
    size_t off_feat, off_x[4];
    BlockScratch scr;
    size_t total;
};

// ---- the plan as data ------------------------------------------------------------------------------------------------------------
// What a plan depends on beside its geometry: the context's settings in a forward, the query's in acx_test_forward_plan.
struct PlanEnv { int precision; bool dense, tiled_head; };

// One tenant: `need` bytes from byte `offset` of region `region` (ACX_PLAN_*), used in one phase of the forward; operands: the
// regions (bit r = region r) that phase reads or writes in their own role while the tenant is live.
struct Tenant { int kind, region, phase, stage, block; unsigned operands; size_t offset, need; };
struct TenantList {
    int n = 0;
    Tenant t[ACX_PLAN_MAX_TENANTS];
    void add(int kind, int region, int phase, int stage, int block, unsigned operands, size_t offset, size_t need) {
        if (n < ACX_PLAN_MAX_TENANTS) t[n] = Tenant{kind, region, phase, stage, block, operands, offset, need};
        ++n;                            // (an overflow is reported by whoever reads the list)
    }
};

static const char* const kTenantNames[ACX_PLAN_TENANT_KINDS] = {
    "dense frames", "dense spectrum", "LayerNorm rows", "bf16 hidden activation", "bf16 LayerNorm rows of the MLP",
    "hidden activation", "LayerNorm statistics", "downsample xnorm", "segment embeddings", "scene rows"};
static const char* const kRegionNames[ACX_PLAN_REGIONS] = {
    "tables", "feat", "x0", "x1", "x2", "x3", "y", "hidden", "stats", "augmented wave", "augmented feat", "augmented mix",
    "augmented frames", "augmented spectrum"};

static constexpr unsigned region_bit(int r) { return 1u << r; }

// the tail of a forward as one number: enum acx_mode, then ACX_PLAN_TAIL_SEG_OUTPUT / _SEG_EMBED
static int tail_of(int mode, const SegTail* seg);

// Every tenant of the forward of geometry g, in launch order.  run_forward lends exactly these: the pointers it passes on are
// region start + offset of the entries here, and it refuses a plan in which one does not fit.
static void forward_tenants(const PlanEnv& e, const Geom& g, int tail, bool feat_in, TenantList* l) {
    l->n = 0;
    const unsigned tab = region_bit(ACX_PLAN_TABLES);
    const size_t Bp = g.vg ? 1 : (size_t)g.B;             // (a variable-length batch: T and Hs are the sums over its clips)
    if (e.dense && !feat_in) {
        const unsigned ops = tab | region_bit(ACX_PLAN_FEAT);
        l->add(ACX_PLAN_DENSE_FRAMES, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_FRONTEND, -1, -1, ops, 0, need_dense_frames(Bp * g.T));
        l->add(ACX_PLAN_DENSE_SPEC, ACX_PLAN_Y, ACX_PLAN_PHASE_FRONTEND, -1, -1, ops, 0, need_dense_spec(Bp * g.T));
    }
    for (int s = 0; s < 4; ++s) {
        const int C = kDims[s];
        const size_t M = Bp * g.Hs[s] * (kStemW >> s);
        if (s > 0) {
            const size_t Min = Bp * g.Hs[s - 1] * (kStemW >> (s - 1));
            const unsigned ops = tab | region_bit(ACX_PLAN_X0 + s - 1) | region_bit(ACX_PLAN_X0 + s);
            if (e.precision != ACX_PREC_F32)
                l->add(ACX_PLAN_LN_ROWS, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_DOWNSAMPLE, s, -1, ops, 0, need_ln_rows(e.precision, Min, kDims[s - 1]));
            else
                l->add(ACX_PLAN_XNORM, ACX_PLAN_Y, ACX_PLAN_PHASE_DOWNSAMPLE, s, -1, ops, 0, need_xnorm(e.precision, Min, kDims[s - 1]));
        }
        for (int j = 0; j < kDepths[s]; ++j) {
            const unsigned ops = tab | region_bit(ACX_PLAN_X0 + s) | region_bit(ACX_PLAN_Y);
            const bool last = j == kDepths[s] - 1 && s < 3;
            if (e.precision == ACX_PREC_F32) {
                if (mlp_fused_supported(C)) continue;
                l->add(ACX_PLAN_HIDDEN_ACT, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_BLOCK, s, j, ops, 0, need_hidden_act(M, C));
                l->add(ACX_PLAN_ROW_STATS, ACX_PLAN_STATS, ACX_PLAN_PHASE_BLOCK, s, j, ops, 0, need_row_stats(M));
            } else if (e.precision == ACX_PREC_F32_SPLIT) {
                if (mlp_fused_split_supported(C) || mlp_fused_wide_supported(C)) {
                    if (last) l->add(ACX_PLAN_LN_ROWS, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_BLOCK, s, j, ops, 0, need_ln_rows(e.precision, M, C));
                } else {
                    l->add(ACX_PLAN_HIDDEN_ACT, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_BLOCK, s, j, ops, 0, need_hidden_act(M, C));
                }
            } else if (mlp_fused_wide_bf16_supported(C)) {
                if (last) l->add(ACX_PLAN_LN_ROWS, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_BLOCK, s, j, ops, 0, need_ln_rows(e.precision, M, C));
            } else {
                l->add(ACX_PLAN_MLP_BF16_HIDDEN, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_BLOCK, s, j, ops, 0, need_mlp_bf16_hidden(M, C));
                l->add(ACX_PLAN_MLP_BF16_ROWS, ACX_PLAN_HIDDEN, ACX_PLAN_PHASE_BLOCK, s, j, ops, mlp_bf16_rows_offset(M, C),
                       need_mlp_bf16_rows(M, C));
            }
        }
    }
    const unsigned ops = tab | region_bit(ACX_PLAN_X0 + 3);
    if (tail == ACX_PLAN_TAIL_SEG_OUTPUT)
        l->add(ACX_PLAN_SEGMENT_EMB, ACX_PLAN_FEAT, ACX_PLAN_PHASE_TAIL, -1, -1, ops, 0, need_segment_emb(Bp * g.Hs[3]));
    else if (tail == ACX_MODE_LOGITS && e.tiled_head)
        l->add(ACX_PLAN_SCENE_ROWS, ACX_PLAN_FEAT, ACX_PLAN_PHASE_TAIL, -1, -1, ops, 0, need_scene_rows((size_t)g.B));
}

// The regions of plan p as (offset, bytes): a region holds everything up to the next one's first byte.  `base`: where the plan's
// byte 0 lies in what is reported; tables: the bytes in front of feat (the tables of a variable-length batch).
static void plan_regions(const Plan& p, size_t base, size_t tables, acx_plan_region_t* r) {
    for (int i = 0; i < ACX_PLAN_REGIONS; ++i) r[i] = acx_plan_region_t{0, 0};
    r[ACX_PLAN_TABLES] = acx_plan_region_t{base, tables};
    const size_t cut[8] = {p.off_feat, p.off_x[0], p.off_x[1], p.off_x[2], p.off_x[3], p.scr.y, p.scr.hidden, p.scr.stats};
    for (int i = 0; i < 8; ++i) r[ACX_PLAN_FEAT + i] = acx_plan_region_t{base + cut[i], (i < 7 ? cut[i + 1] : p.scr.end) - cut[i]};
}

// ACX_ERR_STATE when a tenant of plan p does not fit the region it is lent.  Host arithmetic, before the first launch.
static int check_tenants(const Plan& p, const TenantList& l) {
    if (l.n > ACX_PLAN_MAX_TENANTS) ACX_FAIL(ACX_ERR_STATE, "workspace plan: %d tenants (at most %d)", l.n, ACX_PLAN_MAX_TENANTS);
    acx_plan_region_t r[ACX_PLAN_REGIONS];
    plan_regions(p, 0, p.off_feat, r);
    for (int i = 0; i < l.n; ++i) {
        const Tenant& t = l.t[i];
        if (t.offset + t.need > r[t.region].bytes)
            ACX_FAIL(ACX_ERR_STATE,
                     "workspace plan: the %s (stage %d, block %d) need %zu bytes from byte %zu of `%s`, which holds %zu "
                     "(%d clips, %d frames, rows %d / %d / %d / %d)", kTenantNames[t.kind], t.stage, t.block, t.need, t.offset,
                     kRegionNames[t.region], (size_t)r[t.region].bytes, p.g.B, p.g.T, p.g.Hs[0], p.g.Hs[1], p.g.Hs[2], p.g.Hs[3]);
    }
    return ACX_OK;
}

// one tenant against the capacity its caller states (run_block, run_downsample: also reached from the per-layer entry points)
static int tenant_fits(int kind, const char* region, size_t offset, size_t need, size_t cap, int64_t M, int C) {
    if (cap != kNoCap && offset + need > cap)
        ACX_FAIL(ACX_ERR_STATE, "workspace plan: the %s need %zu bytes from byte %zu of `%s`, which holds %zu (%lld pixels of %d channels)",
                 kTenantNames[kind], need, offset, region, cap, (long long)M, C);
    return ACX_OK;
}

// frames mel frames and rows[s] image rows at stage s in all, from byte `off` of the workspace on; the block scratch is stage 0's
static void carve_workspace(size_t frames, const size_t rows[4], size_t off, Plan* p) {
    p->off_feat = off; off += align_up(frames * kMels * 4);
    for (int s = 0; s < 4; ++s) { p->off_x[s] = off; off += align_up(rows[s] * (kStemW >> s) * kDims[s] * 4); }
    p->scr = carve_block_scratch(rows[0] * kStemW, kDims[0], off);
    p->total = p->scr.end;
}

static int make_plan(int B, int64_t L, Plan* p) {
    if (B <= 0) ACX_FAIL(ACX_ERR_ARG, "batch size must be positive (got %d)", B);
    if (L < ACX_MIN_SAMPLES)
        ACX_FAIL(ACX_ERR_SHAPE,
                 "clip of %lld samples is too short: the last 2x2 downsample needs at least %d samples "
                 "(kernel size can't be greater than actual input size)", (long long)L, ACX_MIN_SAMPLES);
    Geom& g = p->g;
    g = Geom{};
    g.B = B; g.L = L;
    g.T = (int)(L / kHop + 1);
    g.Hs[0] = stage_h0(g.T);
    for (int s = 1; s < 4; ++s) g.Hs[s] = g.Hs[s - 1] / 2;
    size_t rows[4];
    for (int s = 0; s < 4; ++s) rows[s] = (size_t)B * g.Hs[s];
    carve_workspace((size_t)B * g.T, rows, 0, p);
    return ACX_OK;
}

// Variable-length batches.  Workspace: the geometry tables (varlen_geometry, device pointers into ws), then the tensors of
// make_plan sized by the sums over the clips.
static int make_plan_varlen(const int64_t* lengths, int B, char* ws, VarGeom* vg, Plan* p) {
    size_t off = 0;
    ACX_TRY(varlen_geometry(lengths, B, ws, vg, &off));
    Geom& g = p->g;
    g = Geom{};
    g.B = B; g.T = vg->frames; g.vg = vg;
    size_t rows[4];
    for (int s = 0; s < 4; ++s) { g.Hs[s] = vg->rows[s]; rows[s] = (size_t)vg->rows[s]; }
    carve_workspace((size_t)vg->frames, rows, off, p);
    return ACX_OK;
}

int check_workspace(const void* ptr, size_t bytes, size_t need) {
    if (bytes < need) ACX_FAIL(ACX_ERR_WORKSPACE, "workspace of %zu bytes is smaller than the %zu needed", bytes, need);
    if (((uintptr_t)ptr & 255) != 0) ACX_FAIL(ACX_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    return ACX_OK;
}

int check_workspace_for(const char* who, const void* ptr, size_t bytes, size_t need) {
    if (bytes < need) ACX_FAIL(ACX_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, bytes, need);
    if (reinterpret_cast<uintptr_t>(ptr) & 255) ACX_FAIL(ACX_ERR_WORKSPACE, "%s: workspace is not 256-byte aligned", who);
    return ACX_OK;
}

// bf16 precision: y -> fp32 LayerNorm -> bf16 rows; pwconv1 + GELU -> bf16 hidden; pwconv2 + residual -> fp32 x.
// Both bf16 arrays live in the `hidden` scratch: need_mlp_bf16_hidden at its head, need_mlp_bf16_rows from mlp_bf16_rows_offset on.
static int run_mlp_bf16(acx_ctx* c, const BlockW& bw, int C, const float* y, float* x, float* hidden, size_t hidden_cap, int64_t M,
                        hipStream_t st) {
    const int Cp = pad64(C);
    ACX_TRY(tenant_fits(ACX_PLAN_MLP_BF16_HIDDEN, "hidden", 0, need_mlp_bf16_hidden((size_t)M, C), hidden_cap, M, C));
    ACX_TRY(tenant_fits(ACX_PLAN_MLP_BF16_ROWS, "hidden", mlp_bf16_rows_offset((size_t)M, C), need_mlp_bf16_rows((size_t)M, C), hidden_cap, M, C));
    char* hb = reinterpret_cast<char*>(hidden);
    char* yb = hb + mlp_bf16_rows_offset((size_t)M, C);
    ACX_TRY(launch_layernorm_rows_bf16(c, y, yb, M, C, st));
    GemmBf16Args g1{};
    g1.A = yb; g1.Wt = bw.w1h; g1.bias = bw.b1; g1.out = hb; g1.M = M; g1.N = 4 * C; g1.Kp = Cp; g1.lda = Cp;
    g1.epi = EPI_GELU; g1.cls = ACX_K_PW1;
    ACX_TRY(launch_gemm_bf16(c, g1, st));
    GemmBf16Args g2{};
    g2.A = hb; g2.Wt = bw.w2h; g2.bias = bw.b2; g2.out = x; g2.resid = x; g2.M = M; g2.N = C; g2.Kp = 4 * C; g2.lda = 4 * C;
    g2.epi = EPI_RESID; g2.cls = ACX_K_PW2;
    return launch_gemm_bf16(c, g2, st);
}

// split precision: y -> fp32 LayerNorm -> S16 rows IN PLACE (row-local); pwconv1 + GELU -> S16 hidden;
// pwconv2 + residual -> fp32 x.  Same bytes per element as the fp32 path.
static int run_mlp_split(acx_ctx* c, const BlockW& bw, int C, float* y, float* x, float* hidden, size_t hidden_cap, int64_t M,
                         hipStream_t st) {
    ACX_TRY(tenant_fits(ACX_PLAN_HIDDEN_ACT, "hidden", 0, need_hidden_act((size_t)M, C), hidden_cap, M, C));
    ACX_TRY(launch_layernorm_rows_split(c, y, y, M, C, st));
    GemmSplitArgs g1{};
    g1.A = y; g1.Wt = bw.w1s; g1.bias = bw.b1; g1.out = hidden; g1.M = M; g1.N = 4 * C; g1.K = C;
    g1.sinv = 1.0f / (kSplitLnScale * bw.w1s_scale); g1.hscale = bw.hid_scale; g1.epi = EPI_GELU; g1.cls = ACX_K_PW1;
    ACX_TRY(launch_gemm_split(c, g1, st));
    GemmSplitArgs g2{};
    g2.A = hidden; g2.Wt = bw.w2s; g2.bias = bw.b2; g2.out = x; g2.resid = x; g2.M = M; g2.N = C; g2.K = 4 * C;
    g2.sinv = 1.0f / (bw.hid_scale * bw.w2s_scale); g2.epi = EPI_RESID; g2.cls = ACX_K_PW2;
    return launch_gemm_split(c, g2, st);
}

// True when the last block of stage s hands the downsample conv its LayerNorm'ed operand rows (S16 / bf16) directly: the fused
// MLP kernels of stages 0-2 in the 16-bit arithmetics (LNOUT epilogue).  x of that stage is then NOT updated by its last block.
bool block_can_emit_ln(const acx_ctx* c, int s) { return s < 3 && c->precision != ACX_PREC_F32; }

int run_block(acx_ctx* c, int s, int j, float* x, float* y, float* hidden, float* stats, const ScratchCap& cap, int B, int H, int Wd,
              hipStream_t st, void* ln_out, const VarGeom* vg) {
    const int C = kDims[s];
    const BlockW& bw = c->blocks[s][j];
    const int64_t M = (int64_t)B * H * Wd;
    // (ln_out is the head of `hidden` in every caller)
    if (ln_out) ACX_TRY(tenant_fits(ACX_PLAN_LN_ROWS, "hidden", 0, need_ln_rows(c->precision, (size_t)M, C), cap.hidden, M, C));
    auto launch_dw = [&](float* row_stats, bool ab) {
        if (vg) return launch_dwconv_varlen(c, bw, C, x, y, row_stats, *vg, s, st, ab);
        return launch_dwconv(c, bw, C, x, y, row_stats, B, H, Wd, st, ab);
    };
    switch (c->precision) {
        case ACX_PREC_F32: {
            if (mlp_fused_supported(C)) {
                ACX_TRY(launch_dw(nullptr, false));      // LN statistics are computed in-kernel
                return launch_mlp_fused(c, bw, C, y, x, M, st);
            }
            ACX_TRY(tenant_fits(ACX_PLAN_HIDDEN_ACT, "hidden", 0, need_hidden_act((size_t)M, C), cap.hidden, M, C));
            ACX_TRY(tenant_fits(ACX_PLAN_ROW_STATS, "stats", 0, need_row_stats((size_t)M), cap.stats, M, C));
            ACX_TRY(launch_dw(stats, false));
            GemmArgs g1{};
            g1.A = y; g1.Wt = bw.w1; g1.bias = bw.b1; g1.out = hidden; g1.stats = stats; g1.colsum = bw.w1sum; g1.M = M; g1.N = 4 * C; g1.K = C;
            g1.epi = EPI_GELU; g1.cls = ACX_K_PW1;
            ACX_TRY(launch_gemm(c, g1, st));
            GemmArgs g2{};
            g2.A = hidden; g2.Wt = bw.w2; g2.bias = bw.b2; g2.out = x; g2.resid = x; g2.M = M; g2.N = C; g2.K = 4 * C;
            g2.epi = EPI_RESID; g2.cls = ACX_K_PW2;
            return launch_gemm(c, g2, st);
        }
        case ACX_PREC_F32_SPLIT:
            ACX_TRY(launch_dw(nullptr, false));
            if (mlp_fused_split_supported(C)) return launch_mlp_fused_split(c, bw, C, y, x, M, st, ln_out);
            if (mlp_fused_wide_supported(C)) return launch_mlp_fused_wide(c, bw, C, y, x, M, st, ln_out);
            if (ln_out) ACX_FAIL(ACX_ERR_STATE, "run_block: LayerNorm output requested from a two-GEMM stage");
            return run_mlp_split(c, bw, C, y, x, hidden, cap.hidden, M, st);
        default: {                                                              // bf16, bf16a
            const bool ab = act_bf16(c, s);         // x and y of this stage are bf16 tensors in HBM
            ACX_TRY(launch_dw(nullptr, ab));
            if (mlp_fused_wide_bf16_supported(C)) return launch_mlp_fused_wide_bf16(c, bw, C, y, x, M, st, ln_out, pad64(C), ab);
            if (ln_out) ACX_FAIL(ACX_ERR_STATE, "run_block: LayerNorm output requested from a two-GEMM stage");
            return run_mlp_bf16(c, bw, C, y, x, hidden, cap.hidden, M, st);
        }
    }
}

int run_downsample(acx_ctx* c, int i, const float* x, float* out, float* xnorm, size_t xnorm_cap, int B, int H, int Wd,
                   hipStream_t st, bool have_ln, bool out_bf16, const VarGeom* vg) {
    const int Ci = kDims[i - 1], Co = kDims[i];
    const DownW& d = c->down[i];
    {
        const int64_t Min = (int64_t)B * H * Wd;
        if (have_ln) ACX_TRY(tenant_fits(ACX_PLAN_LN_ROWS, "hidden", 0, need_ln_rows(c->precision, (size_t)Min, Ci), xnorm_cap, Min, Ci));
        else ACX_TRY(tenant_fits(ACX_PLAN_XNORM, "y", 0, need_xnorm(c->precision, (size_t)Min, Ci), xnorm_cap, Min, Ci));
    }
    const int* irow = vg ? vg->irow[i] : nullptr;
    const int64_t Mout = vg ? (int64_t)vg->rows[i] * (Wd / 2) : (int64_t)B * (H / 2) * (Wd / 2);
    switch (c->precision) {
        case ACX_PREC_F32: {
            ACX_TRY(launch_layernorm_rows(c, x, xnorm, (int64_t)B * H * Wd, Ci, st));
            GemmArgs g{};
            g.A = xnorm; g.Wt = d.w; g.bias = d.b; g.out = out;
            g.gather = 1; g.H = H; g.W = Wd; g.C = Ci; g.Ho = H / 2; g.Wo = Wd / 2;
            g.M = Mout; g.N = Co; g.K = 4 * Ci; g.epi = EPI_BIAS; g.cls = ACX_K_DOWNSAMPLE; g.irow = irow;
            return launch_gemm(c, g, st);
        }
        case ACX_PREC_F32_SPLIT: {
            if (!have_ln) ACX_TRY(launch_layernorm_rows_split(c, x, xnorm, (int64_t)B * H * Wd, Ci, st));
            GemmSplitArgs g{};
            g.A = xnorm; g.Wt = d.ws; g.bias = d.b; g.out = out;
            g.gather = 1; g.H = H; g.W = Wd; g.C = Ci; g.Ho = H / 2; g.Wo = Wd / 2;
            g.M = Mout; g.N = Co; g.K = 4 * Ci; g.sinv = 1.0f / (kSplitLnScale * d.ws_scale);
            g.epi = EPI_BIAS; g.cls = ACX_K_DOWNSAMPLE; g.irow = irow;
            return launch_gemm_split(c, g, st);
        }
        default: {                                                              // bf16, bf16a
            const int Cp = pad64(Ci);
            if (!have_ln) ACX_TRY(launch_layernorm_rows_bf16(c, x, xnorm, (int64_t)B * H * Wd, Ci, st));
            GemmBf16Args g{};
            g.out_bf16 = out_bf16 ? 1 : 0;
            g.A = xnorm; g.Wt = d.wh; g.bias = d.b; g.out = out;
            g.gather = 1; g.H = H; g.W = Wd; g.Cp = Cp; g.Ho = H / 2; g.Wo = Wd / 2;
            g.M = Mout; g.N = Co; g.Kp = 4 * Cp; g.lda = Cp; g.epi = EPI_BIAS; g.cls = ACX_K_DOWNSAMPLE; g.irow = irow;
            return launch_gemm_bf16(c, g, st);
        }
    }
}

// side streams + fork/join events of the batch split (acx_forward), one set per caller stream.  The set of the null stream is
// created in acx_create; any other stream gets its set at its first split forward -- which must not be a stream capture
// (hipStreamCreate inside a capture region): warm up once on the stream before capturing, as the host wrapper does.
// A partial failure destroys what it created; the map is bounded (sets of the least recently added streams are dropped).
void destroy_aux(acx_ctx::Aux& a) {
    if (a.fork) (void)hipEventDestroy(a.fork);
    for (auto& j : a.joins) if (j) (void)hipEventDestroy(j);
    for (auto& s : a.streams) if (s) (void)hipStreamDestroy(s);
    a = acx_ctx::Aux{};
}
int make_aux(acx_ctx::Aux* a) {
    *a = acx_ctx::Aux{};
    hipError_t e = hipEventCreateWithFlags(&a->fork, hipEventDisableTiming);
    for (int i = 0; i < acx_ctx::kMaxSplitWays - 1 && e == hipSuccess; ++i) {
        e = hipStreamCreateWithFlags(&a->streams[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&a->joins[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        destroy_aux(*a);
        ACX_FAIL(ACX_ERR_HIP, "side streams / events of the batch split: %s", hipGetErrorString(e));
    }
    return ACX_OK;
}

// A batch is split into sub-batches that run side by side on separate streams when every sub-batch keeps at least this
// many clips.
static constexpr int kSplitMinClips = 8;

// number of sub-batches a forward of B clips runs as
static int split_ways_for(const acx_ctx* c, int B) {
    int ways = 1;
    if (c && c->split_streams && !c->prof.on) {
        // defaults measured at B = 64 (profiles/r03_j_batch_split.txt): sub-batches on separate streams fill each other's
        // tail rounds and kernel boundaries -- also between CU-exclusive kernels, whose workgroups never share a CU but do
        // share the chip
        ways = c->split_ways > 0 ? c->split_ways : 2;
    }
    while (ways > 1 && B < ways * kSplitMinClips) --ways;
    return ways;
}
// clips of sub-batch i of `ways`
static int split_part(int B, int ways, int i) { return B / ways + (i < B % ways ? 1 : 0); }

static constexpr size_t kMaxAuxStreams = 16;
// Is one of the set's side streams inside a stream capture?  A side stream joins the capture of its caller stream at the
// fork and stays in it until the capture ENDS, also between two captured forwards, when nobody is queueing on the set
// (users == 0).  Such a set must not serve another caller stream: its side streams would wait on a fork event that was
// not captured, and the other caller's kernels would be recorded into the open graph instead of running.
// A query that fails counts as capturing.
static bool aux_capturing(const acx_ctx::Aux& a) {
    for (hipStream_t s : a.streams) {
        if (!s) continue;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return true; }
        if (cap != hipStreamCaptureStatusNone) return true;
    }
    return false;
}
// The fork/join set of caller stream `st`, pinned until release_aux().  *found = false (and nothing pinned) when the stream
// has no set yet and one cannot be made now -- the first split forward on the stream happens inside a stream capture
// (hipStreamCreate is illegal there; `with torch.cuda.graph(g): model(x)` captures on a private stream nobody can warm
// up): the caller then runs the batch un-split, which gives the same bits.
static int get_aux(acx_ctx* c, hipStream_t st, acx_ctx::Aux* out, bool* found) {
    std::lock_guard<std::mutex> lock(c->aux_mutex);
    *found = false;
    auto it = c->aux.find(st);
    if (it == c->aux.end()) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return ACX_OK;
        acx_ctx::AuxEntry e;
        if (c->aux.size() >= kMaxAuxStreams) {          // drop the least recently used set nobody is queueing on or capturing with
            auto victim = c->aux.end();                 // (none eligible: the map grows past kMaxAuxStreams while captures are open)
            for (auto d = c->aux.begin(); d != c->aux.end(); ++d)
                if (d->first != nullptr && d->second.users == 0 && (victim == c->aux.end() || d->second.stamp < victim->second.stamp) &&
                    !aux_capturing(d->second.a))
                    victim = d;
            if (victim != c->aux.end()) {
                // retired, not destroyed: destroying a stream that still has work means synchronising it, which stalls every
                // forward waiting for aux_mutex and is an illegal call while ANY stream of the process captures in global
                // mode.  The retired sets are a FREE POOL: fork and join are ordered by events alone,
                // so a set whose old work is still draining can serve a new caller stream as it is -- a context called from
                // ever-new streams (per-request streams, private capture streams) recycles kMaxAuxStreams + pool sets for ever
                // instead of leaking two streams and three events per eviction.
                c->aux_retired.push_back(victim->second.a);
                c->aux.erase(victim);
            }
        }
        // the most recently retired set that is not inside a capture (victims are checked above, so none should be: the pool
        // is held to the same rule where a set is handed out, not only where it goes in); none eligible: a new set
        auto r = c->aux_retired.end();
        while (r != c->aux_retired.begin() && aux_capturing(*(r - 1))) --r;
        if (r != c->aux_retired.begin()) {
            e.a = *(r - 1);
            c->aux_retired.erase(r - 1);
        } else {
            ACX_TRY(make_aux(&e.a));
        }
        it = c->aux.emplace(st, e).first;
    }
    it->second.stamp = ++c->aux_clock;
    it->second.users += 1;
    *out = it->second.a;
    *found = true;
    return ACX_OK;
}
static void release_aux(acx_ctx* c, hipStream_t st) {
    std::lock_guard<std::mutex> lock(c->aux_mutex);
    auto it = c->aux.find(st);
    if (it != c->aux.end() && it->second.users > 0) it->second.users -= 1;
}

// The tail of the segment forwards (acx_forward_segments*): what to compute from the stage-3 map instead of `mode`'s output.
struct SegTail {
    int pool, what;
    float* clip;        // ACX_SEG_OUTPUT: (clips, N) maximum over segments, or null
};

static int tail_of(int mode, const SegTail* seg) {
    if (!seg) return mode;
    return seg->what == ACX_SEG_EMBED ? ACX_PLAN_TAIL_SEG_EMBED : ACX_PLAN_TAIL_SEG_OUTPUT;
}

// ACX_SEG_EMBED: the segment embeddings go straight to out0.  ACX_SEG_OUTPUT: they go to `feat` (idle since the stem; the tenant
// ACX_PLAN_SEGMENT_EMB, need_segment_emb), the head reads them there.  roff3 / maxS: a variable-length batch (B clips, rows rows).
static int run_segment_tail(acx_ctx* c, const SegTail& sg, const float* x3, int B, int S, long long rows, float* feat, float* out0,
                            float* out1, const int* roff3, int maxS, hipStream_t st) {
    if (sg.what == ACX_SEG_EMBED) return launch_segment_pool(c, x3, B, S, sg.pool, out0, roff3, maxS, st);
    ACX_TRY(launch_segment_pool(c, x3, B, S, sg.pool, feat, roff3, maxS, st));
    ACX_TRY(launch_segment_head(c, feat, rows, out0, out1, st));
    if (sg.clip) return launch_segment_clipmax(out1, B, S, c->num_classes, sg.clip, roff3, st);
    return ACX_OK;
}

// The tenants of plan p under context c against their regions (check_tenants).  Every plan is checked ONCE, by its driver and before
// that driver launches anything: forward_varlen_impl for its packed plan, forward_uniform for the unsplit and the split plans --
// unless its caller launches something of its own first (window table, stream table, the augmentations) and therefore has called
// check_uniform_plans already (plans_checked).  run_forward takes its pointers from the list and checks nothing again.
static int check_plan(const acx_ctx* c, const Plan& p, int mode, const SegTail* seg, bool feat_in) {
    const PlanEnv env{c->precision, c->dense_stft, head_tiled(c)};
    TenantList tl;
    forward_tenants(env, p.g, tail_of(mode, seg), feat_in, &tl);
    return check_tenants(p, tl);
}
int check_uniform_plans(const acx_ctx* c, int B, int64_t L, int mode, const SegTail* seg, bool feat_in) {
    Plan p;
    ACX_TRY(make_plan(B, L, &p));                   // (the unsplit plan too: a split falls back to it inside a stream capture)
    ACX_TRY(check_plan(c, p, mode, seg, feat_in));
    const int ways = split_ways_for(c, B);
    for (int i = 0; ways > 1 && i < ways; ++i) {
        ACX_TRY(make_plan(split_part(B, ways, i), L, &p));
        ACX_TRY(check_plan(c, p, mode, seg, feat_in));
    }
    return ACX_OK;
}

// The forward of one (sub-)batch on one stream: frontend, stem, the four stages, then the tail -- seg's, or `mode`'s.  Where the
// uniform and the variable-length kernels differ (frontend, stem, depthwise conv, downsample gather, pooling, transpose), p.g.vg
// picks the launcher; the pointwise stages of a variable-length batch run as B = 1, H = the stage's total rows.
// feat_in (uniform batches only): the batch's bn0'd log-mel rows, (B, T, 224), given by the caller (acx_forward_features) -- no
// frontend launch, the stem reads them where they lie; `feat` of the workspace stays the tail's scratch.
static int run_forward(acx_ctx* c, const float* wav, const Plan& p, int mode, float* out0, float* out1, char* ws, hipStream_t st,
                       const SegTail* seg, const float* feat_in = nullptr) {
    const Geom& g = p.g;
    const VarGeom* vg = g.vg;
    float* feat = (float*)(ws + p.off_feat);
    float* x[4];
    for (int s = 0; s < 4; ++s) x[s] = (float*)(ws + p.off_x[s]);
    float* y = (float*)(ws + p.scr.y);
    float* hidden = (float*)(ws + p.scr.hidden);
    float* stats = (float*)(ws + p.scr.stats);
    const int Bp = vg ? 1 : g.B;            // batch of the pointwise launches
    const ScratchCap cap = scratch_cap(p.scr);

    // feat, y, hidden and stats are carved for the stem and for stage 0 and then lent to tenants they were not sized for
    // (forward_tenants lists them; their needs are the need_* definitions of acx_internal.h).  Whether each fits was checked by the
    // driver before anything was launched (check_plan), and over every shape by tests/test_forward_plan_cpu.py through
    // acx_test_forward_plan; here the list says where each one lies.
    const PlanEnv env{c->precision, c->dense_stft, head_tiled(c)};
    TenantList tl;
    forward_tenants(env, g, tail_of(mode, seg), feat_in != nullptr, &tl);
    acx_plan_region_t reg[ACX_PLAN_REGIONS];
    plan_regions(p, 0, p.off_feat, reg);
    // where the plan puts a tenant (null: this forward has no such tenant) -- the pointers below come from the list that was checked
    auto at = [&](int kind, int phase, int stage, int block) -> float* {
        for (int i = 0; i < tl.n; ++i) {
            const Tenant& t = tl.t[i];
            if (t.kind == kind && t.phase == phase && t.stage == stage && t.block == block)
                return (float*)(ws + reg[t.region].offset + t.offset);
        }
        return nullptr;
    };
    float* dense_frames = at(ACX_PLAN_DENSE_FRAMES, ACX_PLAN_PHASE_FRONTEND, -1, -1);
    float* dense_spec = at(ACX_PLAN_DENSE_SPEC, ACX_PLAN_PHASE_FRONTEND, -1, -1);
    // (the launchers want scratch pointers whatever the frontend: they are read by the dense-DFT frontend only)
    if (!dense_frames) dense_frames = hidden;
    if (!dense_spec) dense_spec = y;
    // (dense-DFT fallback: frames in `hidden`, spectrum in `y`, both idle until the first block -- ACX_PLAN_DENSE_FRAMES / _SPEC)
    if (vg) {
        ACX_TRY(launch_logmel_varlen(c, wav, *vg, feat, st, dense_frames, dense_spec));
        ACX_TRY(launch_stem_varlen(c, feat, *vg, x[0], st, act_bf16(c, 0)));
    } else {
        if (!feat_in) ACX_TRY(launch_logmel(c, wav, g.B, g.L, g.T, feat, true, st, dense_frames, dense_spec, g.wstart));
        ACX_TRY(launch_stem(c, feat_in ? feat_in : feat, g.B, g.T, g.Hs[0], x[0], st, act_bf16(c, 0)));
    }
    for (int s = 0; s < 4; ++s) {
        const int Wd = kStemW >> s;
        // The last block of stages 0-2 writes LayerNorm(x) as GEMM operand rows (S16 / bf16) instead of x: nothing else
        // reads that x (convnext.py:270-273).  The rows go to the `hidden` scratch (idle in the fused stages; the tenant
        // ACX_PLAN_LN_ROWS, need_ln_rows), never to y: the block kernel reads y -- with a tile of look-ahead -- while it
        // writes them, and bf16 rows are shorter than the fp32 rows they would overwrite.  Without them (fp32) the
        // downsample normalises x into y (ACX_PLAN_XNORM, need_xnorm).
        if (s > 0) {
            const bool have_ln = block_can_emit_ln(c, s - 1);
            float* xnorm = at(have_ln ? ACX_PLAN_LN_ROWS : ACX_PLAN_XNORM, ACX_PLAN_PHASE_DOWNSAMPLE, s, -1);
            ACX_TRY(run_downsample(c, s, x[s - 1], x[s], xnorm, have_ln ? cap.hidden : cap.y, Bp, g.Hs[s - 1], Wd * 2, st, have_ln,
                                   act_bf16(c, s), vg));
        }
        for (int j = 0; j < kDepths[s]; ++j) {
            void* ln_out = (j == kDepths[s] - 1 && block_can_emit_ln(c, s)) ? (void*)at(ACX_PLAN_LN_ROWS, ACX_PLAN_PHASE_BLOCK, s, j) : nullptr;
            ACX_TRY(run_block(c, s, j, x[s], y, hidden, stats, cap, Bp, g.Hs[s], Wd, st, ln_out, vg));
        }
    }
    const int H3 = g.Hs[3];
    auto pool_head = [&](float* scene, float* logits, float* probs) {
        if (vg) return launch_pool_head_varlen(c, x[3], *vg, scene, logits, probs, st);
        return launch_pool_head(c, x[3], g.B, H3, scene, logits, probs, st);
    };
    if (seg) {
        float* emb = at(ACX_PLAN_SEGMENT_EMB, ACX_PLAN_PHASE_TAIL, -1, -1);           // (null with ACX_SEG_EMBED: not used then)
        if (vg) return run_segment_tail(c, *seg, x[3], g.B, 0, H3, emb, out0, out1, vg->roff[3], vg->maxH[3], st);
        return run_segment_tail(c, *seg, x[3], g.B, H3, (long long)g.B * H3, emb, out0, out1, nullptr, H3, st);
    }
    if (mode == ACX_MODE_FRAME) {
        if (vg) return launch_nhwc_to_nchw_varlen(c, x[3], out0, *vg, st);
        return launch_nhwc_to_nchw(c, x[3], out0, g.B, H3, kStemW >> 3, kDims[3], st);
    }
    if (mode == ACX_MODE_SCENE) return pool_head(out0, nullptr, nullptr);
    if (env.tiled_head) {       // wide head: scene rows into `feat` (idle since the stem; ACX_PLAN_SCENE_ROWS, need_scene_rows), then the head
        float* scene = at(ACX_PLAN_SCENE_ROWS, ACX_PLAN_PHASE_TAIL, -1, -1);
        ACX_TRY(pool_head(scene, nullptr, nullptr));
        return launch_head_tiled(c, scene, g.B, out0, out1, st);
    }
    return pool_head(nullptr, out0, out1);
}

int forward_uniform(acx_ctx* c, const float* wav, int B, int64_t L, int mode, float* out0, float* out1, char* ws, hipStream_t st,
                    const long long* wstart, const SegTail* seg, const float* feat_in, bool plans_checked) {
    // Clips are independent: a large batch runs as sub-batches on separate streams (fork/join with events, so the call
    // still looks like one unit of work on `stream` and stays graph-capturable).  Per-kernel event profiling runs
    // un-split to keep launch durations clean.  The kernels of the 16-bit arithmetics are CU-exclusive -- nothing
    // shares a CU with them -- but a second stream's workgroups take the CUs their tail rounds and launch boundaries
    // leave idle: +4 % (fp32_split) / +11 % (bf16a) at B = 64.
    if (!plans_checked) ACX_TRY(check_uniform_plans(c, B, L, mode, seg, feat_in != nullptr));
    const int ways = split_ways_for(c, B);
    acx_ctx::Aux aux;
    bool have_aux = false;
    if (ways > 1) ACX_TRY(get_aux(c, st, &aux, &have_aux));
    if (ways > 1 && have_aux) {
        // From here on every exit joins the side streams that were forked (an error in sub-batch i must not leave an
        // un-joined fork behind -- inside a stream capture that invalidates the capture, and the caller may free the
        // workspace the side streams still use) and unpins the set.
        int rc = ACX_OK;
        int forked = 0;                 // side streams that wait on the fork event so far
        hipError_t he = hipEventRecord(aux.fork, st);
        if (he != hipSuccess) { set_error("hipEventRecord(fork) failed: %s", hipGetErrorString(he)); rc = ACX_ERR_HIP; }
        size_t ws_off = 0;
        int b_off = 0;
        tls_inflight_ways = ways;
        for (int i = 0; i < ways && rc == ACX_OK; ++i) {
            const int Bi = split_part(B, ways, i);
            Plan pi;
            rc = make_plan(Bi, L, &pi);
            if (rc != ACX_OK) break;
            const size_t per_clip = seg ? (size_t)pi.g.Hs[3] * (seg->what == ACX_SEG_EMBED ? (size_t)kDims[3] : (size_t)c->num_classes)
                                  : mode == ACX_MODE_FRAME ? (size_t)kDims[3] * pi.g.Hs[3] * (kStemW >> 3)
                                                           : (mode == ACX_MODE_SCENE ? (size_t)kDims[3] : (size_t)c->num_classes);
            SegTail sgi{};
            if (seg) { sgi = *seg; if (sgi.clip) sgi.clip += (size_t)b_off * c->num_classes; }
            hipStream_t si = i == 0 ? st : aux.streams[i - 1];
            if (i > 0) {
                he = hipStreamWaitEvent(si, aux.fork, 0);
                if (he != hipSuccess) { set_error("hipStreamWaitEvent(fork) failed: %s", hipGetErrorString(he)); rc = ACX_ERR_HIP; break; }
                forked = i;
            }
            pi.g.wstart = wstart ? wstart + b_off : nullptr;
            rc = run_forward(c, (wstart || !wav) ? wav : wav + (size_t)b_off * L, pi, mode, out0 + b_off * per_clip,
                             out1 ? out1 + b_off * per_clip : nullptr, ws + ws_off, si, seg ? &sgi : nullptr,
                             feat_in ? feat_in + (size_t)b_off * pi.g.T * kMels : nullptr);
            ws_off += pi.total;
            b_off += Bi;
            if (rc == ACX_OK && c->fail_sub.load(std::memory_order_relaxed) == i) {
                set_error("test hook acx_test_fail_sub: failure injected after sub-batch %d", i);
                rc = ACX_ERR_STATE;
            }
        }
        tls_inflight_ways = 1;
        for (int i = 1; i <= forked; ++i) {            // join whatever was forked, also after an error
            hipError_t e1 = hipEventRecord(aux.joins[i - 1], aux.streams[i - 1]);
            if (e1 == hipSuccess) e1 = hipStreamWaitEvent(st, aux.joins[i - 1], 0);
            if (e1 != hipSuccess && rc == ACX_OK) { set_error("joining sub-batch %d failed: %s", i, hipGetErrorString(e1)); rc = ACX_ERR_HIP; }
        }
        release_aux(c, st);
        return rc;
    }
    Plan p;
    ACX_TRY(make_plan(B, L, &p));
    p.g.wstart = wstart;
    return run_forward(c, wav, p, mode, out0, out1, ws, st, seg, feat_in);
}

// ---- argument checks shared by the entry points (who: the entry point's name, which its messages start with) ---------------
int check_forward_args(const char* who, const void* wav, const float* out0, const float* out1, const void* ws, int mode) {
    if (!wav || !out0 || !ws) ACX_FAIL(ACX_ERR_ARG, "%s: null pointer", who);
    if (mode < 0 || mode > 2) ACX_FAIL(ACX_ERR_ARG, "%s: bad mode %d", who, mode);
    if (mode == ACX_MODE_LOGITS && !out1) ACX_FAIL(ACX_ERR_ARG, "%s: logits mode needs out1 (probs)", who);
    return ACX_OK;
}
static int check_seg_what(const char* who, int what) {
    if (what != ACX_SEG_OUTPUT && what != ACX_SEG_EMBED) ACX_FAIL(ACX_ERR_ARG, "%s: bad `what` %d", who, what);
    return ACX_OK;
}
static int check_pool(const char* who, int pool) {
    if (pool < 1 || pool > ACX_MAX_SEGMENT_POOL || !(pool & 1))
        ACX_FAIL(ACX_ERR_ARG, "%s: pool = %d (expected an odd number in 1 .. %d)", who, pool, ACX_MAX_SEGMENT_POOL);
    return ACX_OK;
}
static int check_segment_args(const char* who, int pool, int what, const void* wav, const float* out0, const float* out1,
                              const void* ws) {
    if (!wav || !out0 || !ws) ACX_FAIL(ACX_ERR_ARG, "%s: null pointer", who);
    ACX_TRY(check_seg_what(who, what));
    if (what == ACX_SEG_OUTPUT && !out1) ACX_FAIL(ACX_ERR_ARG, "%s: ACX_SEG_OUTPUT needs out1 (segment probabilities)", who);
    return check_pool(who, pool);
}

// seg == null: the windows / variable-length forward of `mode`; else the segment forward (the mode is ACX_MODE_LOGITS then)
static int forward_windows_impl(acx_ctx* c, const float* wav, const int64_t* lengths, int R, int64_t window, int64_t hop,
                                int64_t first, int count, int mode, float* out0, float* out1, void* workspace,
                                size_t workspace_bytes, void* stream, const SegTail* seg) {
    int64_t n = 0;
    ACX_TRY(window_check(lengths, R, window, hop, &n));
    for (int r = 0; r < R; ++r)
        if (lengths[r] < window)
            ACX_FAIL(ACX_ERR_SHAPE, "recording %d of %lld samples is shorter than the window of %lld: run it as one clip "
                     "(acx_forward_varlen)", r, (long long)lengths[r], (long long)window);
    if (count <= 0 || first < 0 || first + count > n)
        ACX_FAIL(ACX_ERR_ARG, "acx_forward_windows: windows [%lld, %lld) outside the %lld of these recordings", (long long)first,
                 (long long)first + count, (long long)n);
    size_t need = 0;
    ACX_TRY(acx_workspace_bytes_windows(c, count, window, mode, &need));
    ACX_TRY(check_workspace(workspace, workspace_bytes, need));
    ACX_TRY(check_uniform_plans(c, count, window, mode, seg, false));
    hipStream_t st = (hipStream_t)stream;
    long long* wstart = (long long*)workspace;
    // on the caller's stream, before forward_uniform records the fork event: every sub-batch reads its slice after it
    ACX_TRY(launch_window_table(lengths, R, window, hop, first, count, wstart, st));
    return forward_uniform(c, wav, count, window, mode, out0, out1, (char*)workspace + align_up((size_t)count * 8), st, wstart, seg,
                           nullptr, true);
}

static int forward_varlen_impl(acx_ctx* c, const float* wav, const int64_t* lengths, int B, int mode, float* out0, float* out1,
                               void* workspace, size_t workspace_bytes, void* stream, const SegTail* seg) {
    ACX_TRY(check_workspace(workspace, workspace_bytes, 0));       // the alignment first, as ever: the tables go to its head
    VarGeom vg;
    Plan p;
    ACX_TRY(make_plan_varlen(lengths, B, (char*)workspace, &vg, &p));
    ACX_TRY(check_workspace(workspace, workspace_bytes, p.total));
    ACX_TRY(check_plan(c, p, mode, seg, false));
    ACX_TRY(launch_varlen_tables(lengths, vg, (hipStream_t)stream));
    return run_forward(c, wav, p, mode, out0, out1, (char*)workspace, (hipStream_t)stream, seg);
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_stage_hw(int64_t L, int stage, int* H, int* Wd) {
    if (!H || !Wd || stage < 0 || stage > 3) ACX_FAIL(ACX_ERR_ARG, "acx_stage_hw: bad argument");
    Plan p;
    ACX_TRY(make_plan(1, L, &p));
    *H = p.g.Hs[stage]; *Wd = kStemW >> stage;
    return ACX_OK;
}

int acx_workspace_bytes(const acx_ctx* c, int B, int64_t L, int mode, size_t* out_bytes) {
    if (!out_bytes || mode < 0 || mode > 2) ACX_FAIL(ACX_ERR_ARG, "acx_workspace_bytes: bad argument");
    Plan p;
    ACX_TRY(make_plan(B, L, &p));
    *out_bytes = p.total;
    // room for every way the forward may run (the split can be switched by precision, profiling or the environment)
    for (int ways = 2; ways <= acx_ctx::kMaxSplitWays && B >= ways * kSplitMinClips; ++ways) {
        size_t tot = 0;
        for (int i = 0; i < ways; ++i) {
            Plan pi;
            ACX_TRY(make_plan(split_part(B, ways, i), L, &pi));
            tot += pi.total;
        }
        if (tot > *out_bytes) *out_bytes = tot;
    }
    return ACX_OK;
}

int acx_sub_batches(const acx_ctx* c, int B, int* out) {
    if (!c || !out || B <= 0) ACX_FAIL(ACX_ERR_ARG, "acx_sub_batches: bad argument");
    *out = split_ways_for(c, B);
    return ACX_OK;
}

int acx_forward(acx_ctx* c, const float* wav, int B, int64_t L, int mode, float* out0, float* out1, void* workspace,
                size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_forward_args("acx_forward", wav, out0, out1, workspace, mode));
    size_t need = 0;
    ACX_TRY(acx_workspace_bytes(c, B, L, mode, &need));
    ACX_TRY(check_workspace(workspace, workspace_bytes, need));
    return forward_uniform(c, wav, B, L, mode, out0, out1, (char*)workspace, (hipStream_t)stream, nullptr);
}

int acx_forward_features(acx_ctx* c, const float* feat, int B, int64_t L, int mode, float* out0, float* out1, void* workspace,
                         size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_forward_args("acx_forward_features", feat, out0, out1, workspace, mode));
    if ((uintptr_t)feat & 15) ACX_FAIL(ACX_ERR_ARG, "acx_forward_features: feat must be 16-byte aligned");
    size_t need = 0;
    ACX_TRY(acx_workspace_bytes(c, B, L, mode, &need));
    ACX_TRY(check_workspace(workspace, workspace_bytes, need));
    return forward_uniform(c, nullptr, B, L, mode, out0, out1, (char*)workspace, (hipStream_t)stream, nullptr, nullptr, feat);
}

// ---- sliding windows -----------------------------------------------------------------------------------------------------
// Workspace: the window table (count absolute sample offsets), then the uniform forward's workspace of count clips of W samples.
int acx_window_count(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t* n_windows) {
    if (!n_windows) ACX_FAIL(ACX_ERR_ARG, "acx_window_count: n_windows is null");
    return window_check(lengths, R, window, hop, n_windows);
}

int acx_workspace_bytes_windows(const acx_ctx* c, int count, int64_t window, int mode, size_t* out_bytes) {
    if (!out_bytes || mode < 0 || mode > 2) ACX_FAIL(ACX_ERR_ARG, "acx_workspace_bytes_windows: bad argument");
    size_t fwd = 0;
    ACX_TRY(acx_workspace_bytes(c, count, window, mode, &fwd));
    *out_bytes = align_up((size_t)count * 8) + fwd;
    return ACX_OK;
}

int acx_forward_windows(acx_ctx* c, const float* wav, const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t first,
                        int count, int mode, float* out0, float* out1, void* workspace, size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_forward_args("acx_forward_windows", wav, out0, out1, workspace, mode));
    return forward_windows_impl(c, wav, lengths, R, window, hop, first, count, mode, out0, out1, workspace, workspace_bytes, stream,
                                nullptr);
}

int acx_window_timeline_classes(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                                int reduce, float* out, void* stream) {
    if (!probs || !out) ACX_FAIL(ACX_ERR_ARG, "acx_window_timeline: null pointer");
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "acx_window_timeline: %d classes (expected 1 .. %d)", classes, ACX_MAX_CLASSES);
    if (reduce != 0 && reduce != 1) ACX_FAIL(ACX_ERR_ARG, "acx_window_timeline: bad reduce %d (0 mean, 1 max)", reduce);
    ACX_TRY(window_check(lengths, R, window, hop, nullptr));
    return launch_window_timeline(probs, classes, lengths, R, window, hop, reduce, out, (hipStream_t)stream);
}

int acx_window_timeline(const float* probs, const int64_t* lengths, int R, int64_t window, int64_t hop, int reduce, float* out,
                        void* stream) {
    return acx_window_timeline_classes(probs, kClasses, lengths, R, window, hop, reduce, out, stream);
}

// ---- variable-length batches -------------------------------------------------------------------------------------------
int acx_workspace_bytes_varlen(const acx_ctx* c, const int64_t* lengths, int B, int mode, size_t* out_bytes) {
    (void)c;
    if (!out_bytes || mode < 0 || mode > 2) ACX_FAIL(ACX_ERR_ARG, "acx_workspace_bytes_varlen: bad argument");
    VarGeom vg;
    Plan p;
    ACX_TRY(make_plan_varlen(lengths, B, nullptr, &vg, &p));
    *out_bytes = p.total;
    return ACX_OK;
}

int acx_forward_varlen(acx_ctx* c, const float* wav, const int64_t* lengths, int B, int mode, float* out0, float* out1,
                       void* workspace, size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_forward_args("acx_forward_varlen", wav, out0, out1, workspace, mode));
    return forward_varlen_impl(c, wav, lengths, B, mode, out0, out1, workspace, workspace_bytes, stream, nullptr);
}

// ---- sound event detection: segment-wise outputs (segments.hip) --------------------------------------------------------------
int acx_segment_count(int64_t L, int* S) {
    if (!S) ACX_FAIL(ACX_ERR_ARG, "acx_segment_count: S is null");
    Plan p;
    ACX_TRY(make_plan(1, L, &p));
    *S = p.g.Hs[3];
    return ACX_OK;
}

int acx_workspace_bytes_segments(const acx_ctx* c, int B, int64_t L, int what, size_t* out_bytes) {
    ACX_TRY(check_seg_what("acx_workspace_bytes_segments", what));
    return acx_workspace_bytes(c, B, L, ACX_MODE_LOGITS, out_bytes);
}

int acx_forward_segments(acx_ctx* c, const float* wav, int B, int64_t L, int pool, int what, float* out0, float* out1, float* clip,
                         void* workspace, size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_segment_args("acx_forward_segments", pool, what, wav, out0, out1, workspace));
    size_t need = 0;
    ACX_TRY(acx_workspace_bytes(c, B, L, ACX_MODE_LOGITS, &need));
    ACX_TRY(check_workspace(workspace, workspace_bytes, need));
    const SegTail sg{pool, what, what == ACX_SEG_OUTPUT ? clip : nullptr};
    return forward_uniform(c, wav, B, L, ACX_MODE_LOGITS, out0, out1, (char*)workspace, (hipStream_t)stream, nullptr, &sg);
}

int acx_workspace_bytes_segments_varlen(const acx_ctx* c, const int64_t* lengths, int B, int what, size_t* out_bytes) {
    ACX_TRY(check_seg_what("acx_workspace_bytes_segments_varlen", what));
    return acx_workspace_bytes_varlen(c, lengths, B, ACX_MODE_LOGITS, out_bytes);
}

int acx_forward_segments_varlen(acx_ctx* c, const float* wav, const int64_t* lengths, int B, int pool, int what, float* out0,
                                float* out1, float* clip, void* workspace, size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_segment_args("acx_forward_segments_varlen", pool, what, wav, out0, out1, workspace));
    const SegTail sg{pool, what, what == ACX_SEG_OUTPUT ? clip : nullptr};
    return forward_varlen_impl(c, wav, lengths, B, ACX_MODE_LOGITS, out0, out1, workspace, workspace_bytes, stream, &sg);
}

int acx_workspace_bytes_segments_windows(const acx_ctx* c, int count, int64_t window, int what, size_t* out_bytes) {
    ACX_TRY(check_seg_what("acx_workspace_bytes_segments_windows", what));
    return acx_workspace_bytes_windows(c, count, window, ACX_MODE_LOGITS, out_bytes);
}

int acx_forward_segments_windows(acx_ctx* c, const float* wav, const int64_t* lengths, int R, int64_t window, int64_t hop,
                                 int64_t first, int count, int pool, int what, float* out0, float* out1, float* clip,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    ACX_TRY(need_ready(c));
    ACX_TRY(check_segment_args("acx_forward_segments_windows", pool, what, wav, out0, out1, workspace));
    const SegTail sg{pool, what, what == ACX_SEG_OUTPUT ? clip : nullptr};
    return forward_windows_impl(c, wav, lengths, R, window, hop, first, count, ACX_MODE_LOGITS, out0, out1, workspace,
                                workspace_bytes, stream, &sg);
}

int acx_segment_head(acx_ctx* c, const float* x, int B, int S, int pool, float* emb, float* logits, float* probs, void* stream) {
    ACX_TRY(need_ready(c));
    if (!x || !emb) ACX_FAIL(ACX_ERR_ARG, "acx_segment_head: null pointer");
    if (!logits != !probs) ACX_FAIL(ACX_ERR_ARG, "acx_segment_head: logits and probs go together (both or neither)");
    ACX_TRY(check_pool("acx_segment_head", pool));
    if (B <= 0 || S <= 0) ACX_FAIL(ACX_ERR_SHAPE, "acx_segment_head: %d clips of %d segments", B, S);
    ACX_TRY(launch_segment_pool(c, x, B, S, pool, emb, nullptr, S, (hipStream_t)stream));
    if (!logits) return ACX_OK;
    return launch_segment_head(c, emb, (long long)B * S, logits, probs, (hipStream_t)stream);
}

int acx_segment_expand(const float* probs, int B, int S, int N, int T, float* frame, void* stream) {
    if (!probs || !frame) ACX_FAIL(ACX_ERR_ARG, "acx_segment_expand: null pointer");
    if (N < 1 || N > ACX_MAX_CLASSES) ACX_FAIL(ACX_ERR_ARG, "acx_segment_expand: %d classes (expected 1 .. %d)", N, ACX_MAX_CLASSES);
    if (B <= 0 || S <= 0 || T <= 0) ACX_FAIL(ACX_ERR_SHAPE, "acx_segment_expand: %d clips, %d segments, %d frames", B, S, T);
    return launch_segment_expand(probs, B, S, N, T, frame, (hipStream_t)stream);
}

int acx_segment_expand_varlen(const float* probs, const int64_t* lengths, int B, int N, float* frame, void* stream) {
    if (!probs || !frame || !lengths) ACX_FAIL(ACX_ERR_ARG, "acx_segment_expand_varlen: null pointer");
    if (N < 1 || N > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "acx_segment_expand_varlen: %d classes (expected 1 .. %d)", N, ACX_MAX_CLASSES);
    if (B <= 0 || B > kVarMaxClips) ACX_FAIL(ACX_ERR_ARG, "acx_segment_expand_varlen: %d clips (expected 1 .. %d)", B, kVarMaxClips);
    for (int b = 0; b < B; ++b)
        if (lengths[b] < ACX_MIN_SAMPLES || lengths[b] > 0x7fffffffLL)
            ACX_FAIL(ACX_ERR_SHAPE, "acx_segment_expand_varlen: clip %d has %lld samples (expected %d .. 2^31 - 1)", b,
                     (long long)lengths[b], ACX_MIN_SAMPLES);
    return launch_segment_expand_varlen(probs, lengths, B, N, frame, (hipStream_t)stream);
}

int acx_segment_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop, int reduce,
                         float* out, void* stream) {
    if (!probs || !out) ACX_FAIL(ACX_ERR_ARG, "acx_segment_timeline: null pointer");
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "acx_segment_timeline: %d classes (expected 1 .. %d)", classes, ACX_MAX_CLASSES);
    if (reduce != 0 && reduce != 1) ACX_FAIL(ACX_ERR_ARG, "acx_segment_timeline: bad reduce %d (0 mean, 1 max)", reduce);
    ACX_TRY(window_check(lengths, R, window, hop, nullptr));
    for (int r = 0; r < R; ++r)
        if (lengths[r] != 0 && lengths[r] < ACX_MIN_SAMPLES)
            ACX_FAIL(ACX_ERR_SHAPE, "acx_segment_timeline: recording %d of %lld samples is shorter than the %d a clip needs", r,
                     (long long)lengths[r], ACX_MIN_SAMPLES);
    return launch_segment_timeline(probs, classes, lengths, R, window, hop, reduce, out, (hipStream_t)stream);
}

// ---- test support: the plan as data ------------------------------------------------------------------------------------------
static void export_sub(const Plan& p, size_t base, size_t tables, const TenantList& l, acx_plan_sub_t* out) {
    out->clips = p.g.B;
    out->base = base;
    out->bytes = p.total;
    plan_regions(p, base, tables, out->regions);
    out->n_tenants = l.n;
    for (int i = 0; i < l.n; ++i) {
        const Tenant& t = l.t[i];
        out->tenants[i] = acx_plan_tenant_t{t.kind, t.region, t.phase, t.stage, t.block, t.operands, t.offset, t.need};
    }
}

int acx_test_forward_plan(const acx_forward_plan_query_t* q, acx_forward_plan_t* out) {
    if (!q || !out) ACX_FAIL(ACX_ERR_ARG, "acx_test_forward_plan: null pointer");
    if (q->precision < ACX_PREC_F32 || q->precision > ACX_PREC_BF16_ACT || q->classes < 1 || q->classes > ACX_MAX_CLASSES ||
        q->head_path < 0 || q->head_path > 2 || q->driver < ACX_PLAN_UNIFORM || q->driver > ACX_PLAN_AUGMENTED || q->tail < 0 ||
        q->tail > ACX_PLAN_TAIL_SEG_EMBED || q->ways < 1 || q->ways > acx_ctx::kMaxSplitWays)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_forward_plan: bad query");
    const bool pre = q->driver == ACX_PLAN_FEATURES || q->driver == ACX_PLAN_AUGMENTED;      // the trunk is handed its feature map
    if (pre && q->tail > ACX_MODE_FRAME) ACX_FAIL(ACX_ERR_ARG, "acx_test_forward_plan: the features and augmented drivers have no segment tail");
    const bool lam = q->driver == ACX_PLAN_AUGMENTED && q->has_lambda;
    if (lam && (q->B & 1)) ACX_FAIL(ACX_ERR_ARG, "acx_test_forward_plan: mixup needs an even batch");
    const int mode = q->tail <= ACX_MODE_FRAME ? q->tail : ACX_MODE_LOGITS;
    const PlanEnv env{q->precision, q->dense != 0, q->head_path == 2 || (q->head_path == 0 && q->classes >= kHeadTiledMin)};
    std::memset(out, 0, sizeof(*out));
    TenantList l;
    if (q->driver == ACX_PLAN_VARLEN) {
        if (q->ways != 1) ACX_FAIL(ACX_ERR_ARG, "acx_test_forward_plan: a variable-length batch runs unsplit");
        VarGeom vg;
        Plan p;
        ACX_TRY(make_plan_varlen(q->lengths, q->B, nullptr, &vg, &p));
        forward_tenants(env, p.g, q->tail, false, &l);
        if (l.n > ACX_PLAN_MAX_TENANTS) ACX_FAIL(ACX_ERR_STATE, "acx_test_forward_plan: %d tenants", l.n);
        export_sub(p, 0, p.off_feat, l, &out->subs[0]);
        out->n_subs = 1;
        out->total = p.total;
        size_t promised = 0;
        ACX_TRY(acx_workspace_bytes_varlen(nullptr, q->lengths, q->B, mode, &promised));
        out->promised = promised;
        return ACX_OK;
    }
    const int Bf = lam ? q->B / 2 : q->B;
    if (q->ways > 1 && Bf < q->ways * kSplitMinClips)
        ACX_FAIL(ACX_ERR_ARG, "acx_test_forward_plan: %d ways need %d clips (got %d)", q->ways, q->ways * kSplitMinClips, Bf);
    // what lies in front of the (sub-)batches of forward_uniform
    size_t front = 0, promised = 0;
    acx_plan_sub_t& s0 = out->subs[0];
    AugWs aw{};
    if (q->driver == ACX_PLAN_WINDOWS) {
        front = align_up((size_t)q->B * 8);
        ACX_TRY(acx_workspace_bytes_windows(nullptr, q->B, q->L, mode, &promised));
    } else if (q->driver == ACX_PLAN_AUGMENTED) {
        ACX_TRY(carve_augmented(env.dense, q->B, q->L, q->has_wave_plan != 0, lam, mode, &aw));
        front = aw.fwd;
        promised = aw.total;
    } else {
        ACX_TRY(acx_workspace_bytes(nullptr, q->B, q->L, mode, &promised));
    }
    size_t off = front;
    for (int i = 0; i < q->ways; ++i) {
        Plan p;
        ACX_TRY(make_plan(q->ways > 1 ? split_part(Bf, q->ways, i) : Bf, q->L, &p));
        forward_tenants(env, p.g, q->tail, pre, &l);
        if (l.n + 2 > ACX_PLAN_MAX_TENANTS) ACX_FAIL(ACX_ERR_STATE, "acx_test_forward_plan: %d tenants", l.n);
        export_sub(p, off, 0, l, &out->subs[i]);
        off += p.total;
    }
    out->n_subs = q->ways;
    out->total = off;
    out->promised = promised;
    if (front) {                      // sub-batch 0 also owns what the driver put in front
        s0.bytes += s0.base;
        s0.base = 0;
    }
    if (q->driver == ACX_PLAN_WINDOWS) s0.regions[ACX_PLAN_TABLES] = acx_plan_region_t{0, front};
    if (q->driver == ACX_PLAN_AUGMENTED) {
        AugFront af;
        augmented_front(aw, env.dense, (size_t)q->B * (size_t)(q->L / kHop + 1), &af);
        for (int i = 0; i < 5; ++i) s0.regions[ACX_PLAN_AUG_WAVE + i] = af.regions[i];
        for (int i = 0; i < af.n_tenants; ++i) s0.tenants[s0.n_tenants++] = af.tenants[i];
    }
    return ACX_OK;
}

}  // extern "C"
