/* acx.h -- C ABI of libacx.so: the MI355X-native (gfx950) audio-tagging inference path.
 *
 * The reference (topel/audioset-convnext-inf) has no FFI layer: its boundary for this path is
 * the Python nn.Module surface of `ConvNeXt` (src/audioset_convnext_inf/pytorch/convnext.py).
 * Each entry point below names the reference interface it stands in for (file:line relative to
 * the reference root).  The host-side mirror of that surface lives in
 * audioset-convnext-inf_amd/pytorch/convnext.py and binds these symbols with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in any signature
 *     (`stream` is a hipStream_t passed as void*; NULL = the null stream).
 *   - every function returns ACX_OK (0) or a negative acx_status; acx_last_error() gives the
 *     thread-local message of the last failure.
 *   - device pointers are fp32, 16-byte aligned, caller-owned (torch tensors); the context owns
 *     only the repacked weights.  Nothing in the launch path allocates or synchronises, so the
 *     forward can be captured into a hipGraph and `.cpu()` on the outputs synchronises exactly
 *     as it does in the reference.
 *   - activations inside the library are NHWC (channels-last); NCHW appears only in the
 *     frame-embedding output, as in the reference.
 */
#ifndef ACX_H
#define ACX_H

#include <stddef.h>
#include <stdint.h>

#if defined(ACX_BUILD)
#define ACX_API __attribute__((visibility("default")))
#else
#define ACX_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct acx_ctx acx_ctx;

enum acx_status {
    ACX_OK = 0,
    ACX_ERR_ARG = -1,         /* null pointer, bad enum, bad key */
    ACX_ERR_STATE = -2,       /* weights missing / not finalized */
    ACX_ERR_HIP = -3,         /* a HIP runtime call failed */
    ACX_ERR_SHAPE = -4,       /* tensor shape does not match the model, or clip too short */
    ACX_ERR_WORKSPACE = -5,   /* workspace too small or misaligned */
    ACX_ERR_UNSUPPORTED = -6  /* e.g. a device that is not gfx950 */
};

enum acx_mode {
    ACX_MODE_LOGITS = 0,      /* ConvNeXt.forward                  convnext.py:287-331 */
    ACX_MODE_SCENE = 1,       /* ConvNeXt.forward_scene_embeddings convnext.py:333-366 */
    ACX_MODE_FRAME = 2        /* ConvNeXt.forward_frame_embeddings convnext.py:369-402 */
};

/* Arithmetic of the dense contractions (pwconv1/pwconv2, convnext.py:60-62, and the 2x2 downsample convs,
 * convnext.py:230-235).  The reference runs everything in fp32; BASELINE configs[2] asks for "bf16 with fp32
 * LayerNorm": bf16 MFMA operands with fp32 accumulation, while LayerNorm statistics, the residual stream, the
 * depthwise conv, the frontend and the head stay fp32.  The 1e-3 parity bar applies to ACX_PREC_F32 only. */
enum acx_precision {
    ACX_PREC_F32 = 0,         /* v_mfma_f32_32x32x2_f32: fp32 operands on the matrix cores */
    ACX_PREC_BF16 = 1,        /* bf16 operands, fp32 accumulate (NOT within the 1e-3 bar) */
    ACX_PREC_F32_SPLIT = 2,   /* DEFAULT.  fp32 operands carried as fp16 hi + fp16 lo -- v = hi + lo + e with
                               * |e| <= 2^-23 |v| in the worst case (exact for ~40 % of random mantissas; 23 significant bits
                               * where fp32 has 24) -- three fp16 MFMAs per product (the lo*lo term, <= 2^-22 |ab|, is
                               * dropped), fp32 accumulate: fp32-grade results (same parity tests and
                               * tolerances as ACX_PREC_F32, plus tests/test_gpu_stress.py) at 16/3 of the f32-MFMA
                               * rate.  Its kernels launch CU-exclusive workgroups (whole LDS + whole register file of
                               * a CU): work of other streams or processes never shares a CU with them. */
    ACX_PREC_BF16_ACT = 3     /* ACX_PREC_BF16 with the ACTIVATIONS of stages 0-2 (residual stream and depthwise-conv
                               * output: 97 % of the activation bytes) stored in HBM as bf16 as well -- BASELINE configs[2]
                               * read as SURVEY 8d does (107.5 MB of activation traffic per clip).  LayerNorm statistics,
                               * accumulation, GELU, the residual add and the depthwise arithmetic stay fp32; a tensor is
                               * rounded to bf16 (nearest even) when it is written.  Stage 3, frontend and head as in
                               * ACX_PREC_BF16.  The per-layer entry points keep fp32 tensors at the ABI (acx_block converts
                               * at its boundary so that the block runs in this arithmetic). */
};

/* kernel classes for acx_profile_read() */
enum acx_kernel_class {
    ACX_K_FRONTEND = 0, ACX_K_STEM, ACX_K_DWCONV, ACX_K_PW1, ACX_K_PW2, ACX_K_ROWSTATS,
    ACX_K_DOWNSAMPLE, ACX_K_POOLHEAD, ACX_K_TRANSPOSE, ACX_K_MLP_FUSED, ACX_K_MLP_WIDE, ACX_K_COUNT
};

#define ACX_MIN_SAMPLES 7360  /* shortest clip the reference accepts (last 2x2 downsample needs H>=2) */
#define ACX_NUM_CLASSES 527   /* convnext.py:654: the AudioSet head */
#define ACX_MAX_CLASSES 32768 /* widest classifier head a context takes (convnext.py:145-158, num_classes) */
#define ACX_EMBED_DIM 768     /* convnext.py:656 */
#define ACX_MAX_VARLEN_CLIPS 256  /* clips per acx_forward_varlen call */

ACX_API const char* acx_last_error(void);
ACX_API int acx_version(void);

/* Lifetime.  One context per process per GPU (reference: one nn.Module placed by
 * `model.to(device)`, demo_convnext.py:44-45, evaluate_convnext_on_audioset.py:45-47). */
ACX_API int acx_create(int hip_device, acx_ctx** out);
ACX_API void acx_destroy(acx_ctx* ctx);

/* Weights enter under the reference's own state_dict keys (the 190-key contract of
 * `load_state_dict` / `safetensors.torch.load_model`, convnext.py:507,
 * evaluate_convnext_on_audioset.py:36-38).  `host_data` is fp32, C-contiguous, HOST memory,
 * borrowed for the duration of the call.  `bn0.num_batches_tracked` (int64) is not needed.
 * Classifier heads of any size (a fine-tuned `head_audioset = nn.Linear(768, N)`, convnext.py:257): `head_audioset.weight`
 * is (N, 768) and `head_audioset.bias` (N,) with 1 <= N <= ACX_MAX_CLASSES; every other key has its fixed shape.  The
 * context's class count N is the row count of the head it was finalized with (acx_finalize fails with ACX_ERR_SHAPE, naming
 * both keys, when weight and bias disagree).  Every output that is 527 wide with the AudioSet head is N wide: "(B, N)" below.
 * A class's logit depends only on the clip's scene embedding and that head row -- not on N, on the row's position, on the
 * batch or on which head kernel computed it -- bit for bit. */
ACX_API int acx_set_weight(acx_ctx* ctx, const char* state_dict_key, const float* host_data,
                   const int64_t* shape, int ndim);

/* *n = N, the class count of the finalized weights (ACX_NUM_CLASSES for the AudioSet head); ACX_ERR_STATE before
 * acx_finalize. */
ACX_API int acx_num_classes(const acx_ctx* ctx, int* n);

/* Folds and repacks for the kernels, uploads to the device:
 *   bn0 -> per-mel scale/shift (convnext.py:304-306); melW -> banded form (any matrix: a band may span all 513 bins);
 *   STFT buffers that are window x DFT (torchlibrosa's are hann x DFT) -> the FFT kernel stands in for the two Conv1d
 *   (convnext.py:179-187,298); any other stored buffers -> the dense contraction itself (acx_frontend_info);
 *   dwconv (C,1,7,7) -> [49][C]; LayerNorm affine of each block folded into pwconv1;
 *   gamma folded into pwconv2 (convnext.py:78-83); downsample conv (C',C,2,2) -> [C'][4C] with its
 *   LayerNorm affine folded in.
 * May be called again after weights change. */
ACX_API int acx_finalize(acx_ctx* ctx);

/* Selects enum acx_precision for every later call.  Default: ACX_PREC_F32_SPLIT -- the same default as the Python host
 * (pytorch/convnext.py, ACX_PRECISION overrides it there), so a C caller and a Python caller get the same arithmetic.
 * The reference has no such switch (its torch equivalent is `model.to(torch.bfloat16)` / autocast around the Linear
 * layers).  Changing it drops the finalized state: call acx_finalize again. */
ACX_API int acx_set_precision(acx_ctx* ctx, int precision);

/* Geometry helpers: frames T = L/320+1 (torchlibrosa STFT, hop 320, center) and the spatial size
 * after the stem / each downsample (convnext.py:688-691, 230-235). */
ACX_API int acx_num_frames(int64_t L, int* T);
ACX_API int acx_stage_hw(int64_t L, int stage, int* H, int* W);

/* Workspace of acx_forward.  It does not depend on N: the wide-head path keeps its scene rows in the frontend's feature
 * buffer, which is idle once the stem has run and holds at least 24 x 224 floats per clip ("Classifier heads of
 * any size"). */
ACX_API int acx_workspace_bytes(const acx_ctx* ctx, int B, int64_t L, int mode, size_t* out_bytes);

/* How acx_forward runs a batch of B clips: as *out sub-batches side by side on separate streams (clips are independent in
 * eval mode, convnext.py:219,305 -- BatchNorm uses running statistics; every clip's result is bit-identical however the
 * batch is composed or split).  1 for small batches, while per-kernel profiling is enabled, or with ACX_SPLIT_STREAMS=0;
 * ACX_SPLIT_WAYS=n (1..4) overrides the default of 2.  A forward whose FIRST use of a caller stream happens inside a
 * stream capture (`with torch.cuda.graph(g): model(x)` captures on a private stream) runs un-split -- the side streams
 * cannot be created there -- with the same bits.  No reference counterpart: torch runs one batch on one stream. */
ACX_API int acx_sub_batches(const acx_ctx* ctx, int B, int* out);

/* The hot path.  wav: device (B, L) fp32.
 *   ACX_MODE_LOGITS: out0 = logits (B,N), out1 = probs (B,N)   [dict keys
 *                    "clipwise_logits" / "clipwise_output", convnext.py:329]
 *   ACX_MODE_SCENE : out0 = (B,768), out1 ignored
 *   ACX_MODE_FRAME : out0 = NCHW (B,768,H3,7), out1 ignored */
ACX_API int acx_forward(acx_ctx* ctx, const float* wav, int B, int64_t L, int mode, float* out0,
                float* out1, void* workspace, size_t workspace_bytes, void* stream);

/* Variable-length batches: B clips of different lengths in one forward (reference extract_embeddings.py:64-99 feeds clips
 * un-padded, one at a time).  wav: the B clips back to back (sum(lengths) fp32 samples, device memory); lengths: HOST array of
 * the B clip lengths, each >= ACX_MIN_SAMPLES; 1 <= B <= ACX_MAX_VARLEN_CLIPS.
 *   ACX_MODE_LOGITS / ACX_MODE_SCENE: out0 / out1 as acx_forward, one row per clip
 *   ACX_MODE_FRAME : out0 = the clips' NCHW blocks (768, H3_i, 7) back to back in clip order
 * Every clip's result is bit-identical to acx_forward of that clip alone.  Same launch contract as acx_forward (all work on
 * `stream`, no allocation, no synchronisation, capturable): the per-clip geometry tables are written into the head of the
 * workspace by the first kernel of the call, from the lengths passed by value.  Runs on the caller's stream (no batch split). */
ACX_API int acx_workspace_bytes_varlen(const acx_ctx* ctx, const int64_t* lengths, int B, int mode, size_t* out_bytes);
ACX_API int acx_forward_varlen(acx_ctx* ctx, const float* wav, const int64_t* lengths, int B, int mode, float* out0,
                               float* out1, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sliding windows over long recordings: tagging over time ---------------------------------------------------------------
 * No reference counterpart: the reference tags a clip as a whole; PANNs-style harnesses reserve a "segmentwise_output" key
 * (pytorch/pytorch_utils.py:63-137).  All lengths in samples at 32 kHz.  R recordings of lengths[r] samples (HOST array,
 * 0 <= lengths[r] < 2^31, 1 <= R <= ACX_MAX_VARLEN_CLIPS) lie back to back in wav; window >= ACX_MIN_SAMPLES, 1 <= hop <= window.
 *   Recording r has n_r = 1 window if L_r <= window, else 1 + ceil((L_r - window) / hop).  Window j starts at
 *   s_j = min(j hop, max(0, L_r - window)) -- the last one ends with the recording -- and holds min(window, L_r) samples.
 *   Windows are numbered recording by recording, then by j.
 *   acx_window_count: *n_windows = sum of n_r (host only; checks the arguments as the calls below do).
 *   acx_forward_windows: windows [first, first + count) as a uniform batch of count clips of `window` samples: outputs as
 *   acx_forward with B = count, L = window, each row bit-identical to acx_forward of that window cut out and run alone.
 *   Every L_r must be >= window (a shorter recording is one clip: ACX_ERR_SHAPE, run it through acx_forward_varlen).
 *   acx_forward's launch contract: lengths by value, no allocation or synchronisation, capturable, the same sub-batch split;
 *   the window table (count absolute sample offsets) is written into the head of the workspace on `stream` first.
 *   acx_window_timeline_classes: probs = the (sum n_r, classes) probabilities of ALL windows of the R recordings, in window
 *   order (1 <= classes <= ACX_MAX_CLASSES: an N-class model's rows); out = sum_r ceil(L_r / hop) rows of `classes`.  Row k of
 *   recording r has the midpoint m_k = min(k hop + hop / 2, L_r - 1) (integer division) and reduces over the windows with
 *   s_j <= m_k < s_j + window: reduce 0 = mean (an fp32 sum in ascending j, then one fp32 division by their count), 1 = max.
 *   One kernel on `stream`, no allocation, capturable.  acx_window_timeline: the same with classes = 527 (the AudioSet head). */
ACX_API int acx_window_count(const int64_t* lengths, int R, int64_t window, int64_t hop, int64_t* n_windows);
ACX_API int acx_workspace_bytes_windows(const acx_ctx* ctx, int count, int64_t window, int mode, size_t* out_bytes);
ACX_API int acx_forward_windows(acx_ctx* ctx, const float* wav, const int64_t* lengths, int R, int64_t window, int64_t hop,
                                int64_t first, int count, int mode, float* out0, float* out1, void* workspace,
                                size_t workspace_bytes, void* stream);
ACX_API int acx_window_timeline(const float* probs, const int64_t* lengths, int R, int64_t window, int64_t hop,
                                int reduce /* 0 mean, 1 max */, float* out, void* stream);
ACX_API int acx_window_timeline_classes(const float* probs, int classes, const int64_t* lengths, int R, int64_t window,
                                        int64_t hop, int reduce, float* out, void* stream);

/* ---- sound event detection: segment-wise and frame-wise outputs ---------------------------------------------------------------
 * The reference's decision-level recipe (pytorch/models.py:5757-5771: mean over frequency, max_pool1d(3,1,1) + avg_pool1d(3,1,1)
 * over time, the head per segment, sigmoid, clipwise = max over segments, interpolate(.., 32) + pad_framewise_output,
 * pytorch/pytorch_utils.py:140-176) applied to the ConvNeXt trunk: the keys "segmentwise_output" / "framewise_output" that
 * pytorch/inference.py:96-200 (sound_event_detection, :156) and pytorch_utils.py:78,108-119 read, and that the reference's
 * ConvNeXt class never fills.  For a clip of L samples with stage-3 map x (768, S, 7), S = acx_stage_hw(L, 3).H (one segment
 * per 32 STFT frames = 10240 samples; *S of acx_segment_count), and odd pool, 1 <= pool <= ACX_MAX_SEGMENT_POOL:
 *   z[c, t] = mean_f x[c, t, f]                                                                        (convnext.py:279)
 *   p[c, t] = max_{|s-t| <= pool/2, 0 <= s < S} z[c, s] + (1 / pool) sum_{|s-t| <= pool/2, 0 <= s < S} z[c, s]
 *             (F.max_pool1d(z, pool, 1, pool / 2) + F.avg_pool1d(z, pool, 1, pool / 2): the average always divides by pool,
 *              rows beyond the clip count as zeros; the max ignores them; the sum runs in ascending s)
 *   e[t, :] = LayerNorm_768(p[:, t]; norm.weight, norm.bias, eps 1e-6)       segment embedding         (convnext.py:285)
 *   l[t, :] = head_audioset(e[t, :]);  q[t, :] = 1 / (1 + expf(-l[t, :]))    segment logits / output   (convnext.py:321-325)
 *   clip[n] = max_t q[t, n]                                                                            (models.py:5767)
 *   frame[u, :] = q[min(u / 32, S - 1), :],  0 <= u < T = L / 320 + 1        (interpolate + pad_framewise_output)
 * Everything after the trunk is fp32 in every precision mode.  The head runs on the f32-input matrix cores
 * (v_mfma_f32_32x32x2_f32, v_mfma_f32_16x16x4_f32 for small launches) with a fixed contraction order and no atomics: a value
 * (clip, segment, class) depends only on that segment's embedding row and that head row -- not on N, on the batch, on the
 * sub-batch split or on the tile shape -- bit for bit.  Not the arithmetic of acx_forward's head: "clip" is the maximum over
 * segments, NOT the clipwise_output of ACX_MODE_LOGITS.
 *
 * what = ACX_SEG_OUTPUT: out0 = segment logits, out1 = segment probabilities, one row of N per segment; clip (may be NULL) =
 *   (clips, N).  what = ACX_SEG_EMBED: out0 = segment embeddings, one row of 768 per segment; out1 and clip are ignored.
 * acx_forward_segments: acx_forward's arguments; rows (B, S, .).  acx_forward_segments_varlen: acx_forward_varlen's; clip i's
 *   S_i rows back to back in clip order.  acx_forward_segments_windows: acx_forward_windows's; rows (count, S_window, .), each
 *   window bit-identical to acx_forward_segments of that window cut out.  A clip's rows are the same bits through all three.
 * Launch contract of acx_forward: work on `stream` only, no allocation, no synchronisation, capturable, and for the uniform and
 * window forms the same sub-batch split.  The embeddings of the ACX_SEG_OUTPUT forms live in the frontend's feature buffer
 * (idle after the stem, 224 T >= 768 S floats per clip): the workspace equals the one of the corresponding acx_forward call.
 *
 * acx_segment_head (per-layer entry, in the style of acx_pool_head): x NHWC (B, S, 7, 768) -> emb (B S, 768), logits / probs
 *   (B S, N); logits and probs may be NULL (both or neither).
 * acx_segment_expand: frame (B, T, N) from probs (B, S, N), frame[b, u] = probs[b, min(u / 32, S - 1)]; 1 <= S, 1 <= T.
 * acx_segment_expand_varlen: the same for packed clips of lengths[i] samples (HOST array, B <= ACX_MAX_VARLEN_CLIPS): probs =
 *   the clips' (S_i, N) blocks back to back, frame = their (T_i, N) blocks back to back.
 * acx_segment_timeline: a timeline at segment resolution over the windows of R recordings, defined as
 *   acx_window_timeline_classes is.  probs = the segment probabilities of ALL windows in window order: n_r blocks of
 *   (S_window, classes) for a recording longer than the window, one block (S(L_r), classes) for any other (one clip, as
 *   acx_forward_windows treats it).  Recording r gets ceil(L_r / 10240) rows; row k has the midpoint
 *   m_k = min(10240 k + 5120, L_r - 1) and reduces over the (window j, segment i) pairs with
 *   s_j + 10240 i <= m_k < s_j + 10240 (i + 1), where the last segment of a window reaches to the window's end: at most one
 *   segment per window.  reduce 0 = mean (an fp32 sum in ascending j, then one fp32 division by the count), 1 = max.
 *   Every L_r must be >= ACX_MIN_SAMPLES or 0.  One kernel on `stream`, no allocation, capturable.
 * Argument errors (ACX_ERR_ARG: null pointer, pool even or out of range, bad `what`; ACX_ERR_SHAPE: a clip too short, S or T
 * not positive) are returned before any launch. */
enum acx_segment_what { ACX_SEG_OUTPUT = 0, ACX_SEG_EMBED = 1 };
#define ACX_SEGMENT_SAMPLES 10240   /* 32 STFT frames of 320 samples: the four 2x strides of the trunk along time */
#define ACX_MAX_SEGMENT_POOL 31
ACX_API int acx_segment_count(int64_t L, int* S);
ACX_API int acx_workspace_bytes_segments(const acx_ctx* ctx, int B, int64_t L, int what, size_t* out_bytes);
ACX_API int acx_forward_segments(acx_ctx* ctx, const float* wav, int B, int64_t L, int pool, int what, float* out0, float* out1,
                                 float* clip, void* workspace, size_t workspace_bytes, void* stream);
ACX_API int acx_workspace_bytes_segments_varlen(const acx_ctx* ctx, const int64_t* lengths, int B, int what, size_t* out_bytes);
ACX_API int acx_forward_segments_varlen(acx_ctx* ctx, const float* wav, const int64_t* lengths, int B, int pool, int what,
                                        float* out0, float* out1, float* clip, void* workspace, size_t workspace_bytes,
                                        void* stream);
ACX_API int acx_workspace_bytes_segments_windows(const acx_ctx* ctx, int count, int64_t window, int what, size_t* out_bytes);
ACX_API int acx_forward_segments_windows(acx_ctx* ctx, const float* wav, const int64_t* lengths, int R, int64_t window,
                                         int64_t hop, int64_t first, int count, int pool, int what, float* out0, float* out1,
                                         float* clip, void* workspace, size_t workspace_bytes, void* stream);
ACX_API int acx_segment_head(acx_ctx* ctx, const float* x, int B, int S, int pool, float* emb, float* logits, float* probs,
                             void* stream);
ACX_API int acx_segment_expand(const float* probs, int B, int S, int N, int T, float* frame, void* stream);
ACX_API int acx_segment_expand_varlen(const float* probs, const int64_t* lengths, int B, int N, float* frame, void* stream);
ACX_API int acx_segment_timeline(const float* probs, int classes, const int64_t* lengths, int R, int64_t window, int64_t hop,
                                 int reduce, float* out, void* stream);

/* ---- sound event decoding: probabilities over time -> a table of events --------------------------------------------------------
 * The reference leaves this step to its harness (pytorch/inference.py:156-200 thresholds "framewise_output" on the host).  The
 * definition here is pytorch/segments.py::decode_events, the host function of this project, restated for a batch; the device
 * table equals its output bit for bit except `mean`, which is float64 here (decode_events takes numpy's float32 mean).
 * probs: device fp32, rows of N classes with row stride ld >= N floats; clip i owns steps_i consecutive rows (acx_decode_events:
 * rows [i steps, (i + 1) steps); acx_decode_events_varlen: the clips back to back, steps[i] rows each, B <= ACX_MAX_VARLEN_CLIPS).
 * For every (clip, class) column, independently:
 *   1. median: an odd running median of width p->median over time, the ends repeating the first / last row (the width may
 *      exceed steps_i; 1 = identity).  A selection: the result is one of the input values.
 *   2. boundaries, float64: edges[k] = (double)k * step_seconds for k < steps_i, edges[steps_i] = the clip's end_seconds, or
 *      (double)steps_i * step_seconds when that is <= 0 (varlen: or end_seconds == NULL) -- segments.segment_edges().
 *   3. runs: a maximal stretch of filtered q >= p->low is a run; it is valid if it holds a q >= p->threshold (fp32 comparisons).
 *   4. merge, in time order: a valid run [b, e) joins the previous (possibly merged) event when edges[b] - edges[prev end] <
 *      p->merge_gap (float64); the event then reaches to e and contains the gap rows and any invalid runs between.
 *   5. minimum duration: an event with edges[end] - edges[begin] < p->min_duration (float64) is dropped, after merging.
 *   6. per event: begin, end (exclusive) in steps; peak = the fp32 maximum of q over [begin, end); mean = the float64 sum of
 *      those q in ascending time, divided by their count.
 * events: device table of `capacity` rows, written in the order (clip, cls, begin), the same bits on every call (offsets come
 * from a count pass and an exclusive scan; no atomic orders anything).  *count (device int64) = the TOTAL number of events; when
 * it exceeds capacity the first `capacity` rows in table order are written and ACX_EVENTS_OVERFLOW is set in *status (device
 * int): call again with capacity >= *count.  A NaN or +-inf in any probs row read sets ACX_EVENTS_NONFINITE, *count = 0, and
 * nothing is written.  *status is cleared first.  Rows past *count are left untouched.
 * acx_forward's launch contract: everything in order on `stream` (a 4-byte clear, three kernels, one more for the varlen
 * tables, whose steps / end_seconds travel by value), no allocation, no synchronisation, capturable.  Stateless: no acx_ctx.
 * ws: acx_events_workspace_bytes(B, N) bytes, 256-byte aligned (host only; non-decreasing in both arguments).
 * Argument errors are returned before anything touches the device.  ACX_ERR_ARG: a null pointer; median even, < 1 or >
 * ACX_MAX_EVENT_MEDIAN; low outside [0, threshold]; negative min_duration or merge_gap; step_seconds <= 0; capacity < 0.
 * ACX_ERR_SHAPE: steps < 1 (or > 2^30); N < 1 or N > ACX_MAX_CLASSES; ld < N; B < 1 (varlen: B > ACX_MAX_VARLEN_CLIPS).
 * ACX_ERR_WORKSPACE: ws too small or not 256-byte aligned.  ACX_ERR_UNSUPPORTED: B * ceil(N / 64) beyond a launchable grid
 * (2^31 - 1 workgroups). */
typedef struct acx_event { int32_t clip, cls, begin, end; float peak, reserved; double mean; } acx_event;   /* 32 bytes; reserved = 0 */
typedef struct acx_event_params { float threshold, low; int median; double min_duration, merge_gap; } acx_event_params;
#define ACX_MAX_EVENT_MEDIAN 101          /* ~1 s of frames, 32 s of segments */
#define ACX_EVENTS_NONFINITE 1
#define ACX_EVENTS_OVERFLOW  2
ACX_API int acx_events_workspace_bytes(int64_t B, int N, size_t* bytes);                                   /* host only */
ACX_API int acx_decode_events(const float* probs, int64_t ld, int64_t B, int steps, int N, const acx_event_params* p,
                              double step_seconds, double end_seconds /* <= 0: steps * step_seconds */, acx_event* events,
                              int64_t capacity, int64_t* count, int* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_decode_events_varlen(const float* probs, int64_t ld, const int* steps /* HOST, B */,
                                     const double* end_seconds /* HOST, B, or NULL */, int B /* <= ACX_MAX_VARLEN_CLIPS */, int N,
                                     const acx_event_params* p, double step_seconds, acx_event* events, int64_t capacity,
                                     int64_t* count, int* status, void* ws, size_t ws_bytes, void* stream);
/* The same two calls with one threshold and one low per class (the reference's pytorch/inference.py cuts every class at one
 * fixed 0.5-style constant): threshold / low are DEVICE fp32 [N], e.g. acx_operating_points' output.  A pointer that is given
 * replaces the field of the same name of *p, which is then ignored; low == NULL with threshold given means low = threshold per
 * class; with both NULL the calls are acx_decode_events / _varlen.  Values on the device cannot be checked on the host: the
 * count pass sets ACX_EVENTS_BAD_THRESHOLD in *status when any class has !(0 <= low <= threshold) (a NaN included; +inf is
 * legal: the class emits nothing), and then *count = 0 and nothing is written, as with ACX_EVENTS_NONFINITE.  The scalar fields
 * still in use are checked on the host as before. */
#define ACX_EVENTS_BAD_THRESHOLD 4
ACX_API int acx_decode_events_classwise(const float* probs, int64_t ld, int64_t B, int steps, int N, const acx_event_params* p,
                                        double step_seconds, double end_seconds, acx_event* events, int64_t capacity,
                                        int64_t* count, int* status, void* ws, size_t ws_bytes, void* stream,
                                        const float* threshold /* device [N] or NULL */, const float* low /* device [N] or NULL */);
ACX_API int acx_decode_events_varlen_classwise(const float* probs, int64_t ld, const int* steps, const double* end_seconds, int B,
                                               int N, const acx_event_params* p, double step_seconds, acx_event* events,
                                               int64_t capacity, int64_t* count, int* status, void* ws, size_t ws_bytes,
                                               void* stream, const float* threshold, const float* low);

/* ---- online event decoding: the same events from rows that arrive chunk by chunk ---------------------------------------------------
 * The reference decodes nothing, and acx_decode_events needs the whole (steps, N) matrix of a finished recording.  A handle
 * holds `slots` recordings at a time and carries each column's state machine across calls (csrc/events_common.h; the
 * definition is pytorch/segments.py::OnlineEventDecoderHost): every event is handed out exactly once, as soon as nothing still
 * to come can change it, and the rows of all calls of one recording, sorted by (cls, begin), are the rows of acx_decode_events
 * over the concatenated matrix BYTE FOR BYTE, `mean` included, for any chunking.  Rules 1-6 of "sound event decoding" hold
 * unchanged; edges[k] = (double)k * step_seconds for every k but the recording's last boundary, which is free and enters only
 * in acx_event_stream_close.
 *   filtered rows: filtered row t exists once raw row t + median / 2 has been pushed; the front repeats row 0, close supplies
 *     the tail by repeating the last raw row.  A recording of fewer rows than median / 2, or of none, is legal; an empty one
 *     emits nothing.
 *   early emission: after filtered row t a pending event [eb, ee) is final -- and is emitted by this call if it passes the
 *     minimum duration -- when a run is open that began at rb and !(edges[rb] - edges[ee] < merge_gap), or when no run is open
 *     and !(edges[t + 1] - edges[ee] < merge_gap): k * step never decreases in k, so no later run could have merged.  A run
 *     still open is part of no emitted event.
 * acx_event_stream_create allocates the device state on the current device (acx_event_stream_bytes of it: per (slot, class)
 * the state machine's fields and the last `median` raw rows), copies the per-class levels -- device fp32 [N] as in the
 * _classwise calls, NULL: the field of *p -- and CHECKS them: !(0 <= low <= threshold) in any class is ACX_ERR_ARG (a NaN
 * included; +inf is legal), so ACX_EVENTS_BAD_THRESHOLD never appears in a handle's status.  It synchronises the device.
 * After create there is no allocation and no synchronisation: push / close / open launch on `stream` only (a 4-byte clear,
 * a count pass, the scan of acx_decode_events and an emit pass; close one small kernel more) and are capturable.  Slots and
 * row counts travel by value.  The calls of one handle must reach the device in order (one stream, or an event between two).
 * acx_event_stream_push: probs holds rows[0] rows of slot[0], then rows[1] rows of slot[1], ... (row stride ld >= N; may be
 *   NULL when every rows[i] is 0).  The table is ordered by (position in slot[], cls, begin) with clip = the slot and begin /
 *   end in steps of the slot's recording, the same bits on every call.
 * acx_event_stream_close: ends the recordings (last boundary end_seconds[i], <= 0 or end_seconds == NULL: steps * step_seconds),
 *   emits what is left; the slots are clean for their next recordings.
 * A VOID CALL CHANGES NOTHING: when the events of a call exceed `capacity`, ACX_EVENTS_OVERFLOW is set and *count = the total;
 *   a NaN or +-inf in a pushed row sets ACX_EVENTS_NONFINITE and *count = 0.  In both cases the table is not to be used and
 *   the device state of every slot of the call is exactly as before (only the emit pass stores state, and it reads the status
 *   first): repeat the call with a larger table, or with other rows.  The host-side row counters cannot see the device's
 *   status: a caller that finds a call void tells the handle with acx_event_stream_undo (host only: takes back what the
 *   last push or close of each listed slot did to its counter) before the next call to those slots.  Should a recording pass
 *   2^30 rows unseen by the host counters all the same, the device voids the call with ACX_EVENTS_NONFINITE.
 * acx_event_stream_open: begin[i][c] = the step at which the event that class c of slot[i] is inside of began -- the pending
 *   event's begin when the open run will merge with it, else the run's -- once the open run has reached threshold; else -1.
 * acx_event_stream_steps (host only): the raw rows of the slot's open recording.
 * Argument errors are returned before anything touches the device, with acx_decode_events' codes; in addition ACX_ERR_ARG:
 * n outside 1 .. ACX_MAX_VARLEN_CLIPS, a slot out of range or listed twice, rows[i] < 0; ACX_ERR_SHAPE: slots outside
 * 1 .. 2^20, a push that would take a recording past 2^30 rows; ACX_ERR_UNSUPPORTED: a state beyond 2^40 bytes. */
typedef struct acx_event_stream acx_event_stream;
ACX_API int acx_event_stream_bytes(int slots, int N, int median, size_t* bytes);                            /* host only */
ACX_API int acx_event_stream_create(int slots, int N, const acx_event_params* p, double step_seconds,
                                    const float* threshold /* device [N] or NULL */, const float* low /* device [N] or NULL */,
                                    acx_event_stream** out);
ACX_API void acx_event_stream_destroy(acx_event_stream* s);
ACX_API int acx_event_stream_push(acx_event_stream* s, const float* probs, int64_t ld, const int* slot /* HOST, n, distinct */,
                                  const int* rows /* HOST, n, >= 0 */, int n, acx_event* events, int64_t capacity, int64_t* count,
                                  int* status, void* stream);
ACX_API int acx_event_stream_close(acx_event_stream* s, const int* slot /* HOST, n */, const double* end_seconds /* HOST, n, or NULL */,
                                   int n, acx_event* events, int64_t capacity, int64_t* count, int* status, void* stream);
ACX_API int acx_event_stream_open(const acx_event_stream* s, const int* slot /* HOST, n */, int n, int32_t* begin /* device (n, N) */,
                                  void* stream);
ACX_API int acx_event_stream_steps(const acx_event_stream* s, int slot, int64_t* steps);                    /* host only */
ACX_API int acx_event_stream_undo(acx_event_stream* s, const int* slot /* HOST, n */, int n);               /* host only */

/* ---- sound event scoring: an event table against annotated events -> integer counts ------------------------------------------------
 * The reference has no scoring of detected events at all (its pytorch/inference.py:156-200 stops at the thresholded plot); users
 * of acx_decode_events pulled the table to the host and looped.  The definitions are the two host functions of this project,
 * pytorch/sed_metrics.py::event_based_metrics_host and ::segment_based_metrics_host, written after sed_eval's published
 * EventBasedMetrics (greedy matching) and SegmentBasedMetrics; every output is an integer and EQUALS theirs.
 * ref: device table of n_ref reference events ordered by (clip, cls, onset, offset), 0 <= onset < offset finite, 0 <= clip < B,
 * 0 <= cls < N; events of one class may overlap.  est / capacity / est_count / est_status: the table, capacity, *count and
 * *status of acx_decode_events as they lie on the device -- the valid rows are the first min(*est_count, capacity), read on the
 * device, so the call queues behind the decoder without a host synchronisation.  *est_status != 0 or *est_count > capacity (a
 * table that overflowed, non-finite probabilities, bad per-class levels) sets ACX_SCORE_BAD_TABLE in *status and leaves every
 * count zero and every match -1.  steps / end_seconds: DEVICE arrays of B values, the clips' row counts and last boundaries (no
 * ACX_MAX_VARLEN_CLIPS limit: an evaluation set is one call).  An estimated event's onset / offset are edges[begin] / edges[end]
 * of "sound event decoding", 2.
 * acx_score_events (replaces: nothing in the reference; host loops over EventTable.to_lists()).  Per (clip, cls), the reference
 *   events in order: each takes the first estimated row, in table order, not taken yet, with
 *     |r_on - e_on| <= t_collar                                                  (unless evaluate_onset == 0) and
 *     |r_off - e_off| <= max(t_collar, percentage_of_length * (r_off - r_on))    (unless evaluate_offset == 0), all in float64.
 *   counts[cls] = TP (matched pairs), FP = rows - TP, FN = reference events - TP.  ref_match[i] = the estimated row matched to
 *   reference event i or -1; est_match[j] = the reference row matched to estimated row j or -1 (all `capacity` entries are
 *   written).  sed_eval's optimal (bipartite) matching and its cross-class substitutions are not offered.
 * acx_score_segments (replaces: the same).  Clip i has ceil(end_i / time_resolution) segments (at most 2^31 - 2); an event is
 *   active in segments [floor(onset / res), ceil(offset / res)) clipped to the clip, float64 with IEEE division.  Per segment and
 *   class, ref / est activity is the union of the events.  counts[cls] = TP = sum(ref & est), FP = sum(est & ~ref), FN =
 *   sum(ref & ~est) over all segments and clips.  Per segment, with fn / fp its totals over the classes: S = min(fn, fp),
 *   D = max(0, fn - fp), I = max(0, fp - fn).  overall = TP, S, D, I, Nref, Nsys summed over segments and clips (Nref, Nsys: the
 *   active (segment, class) cells).
 * Launch contract: everything in order on `stream` (the clears of the outputs, one kernel), no allocation, no workspace, no
 * synchronisation, capturable; counts meet only in 64-bit integer atomic adds, so every call gives the same bits.  n_ref == 0
 * (ref, ref_match may be NULL) and an empty estimated table (capacity == 0: est, est_match may be NULL) are legal.
 * Argument errors are returned before anything touches the device.  ACX_ERR_ARG: a null pointer; n_ref or capacity < 0;
 * step_seconds <= 0; time_resolution not finite or <= 0; t_collar or percentage_of_length negative or not finite.  ACX_ERR_SHAPE:
 * B < 1; N < 1 or N > ACX_MAX_CLASSES.  ACX_ERR_UNSUPPORTED: B * ceil(N / 64) beyond a launchable grid (2^31 - 1 workgroups). */
typedef struct acx_ref_event { int32_t clip, cls; double onset, offset; } acx_ref_event;   /* 24 bytes */
typedef struct acx_event_collar { double t_collar, percentage_of_length; int32_t evaluate_onset, evaluate_offset; } acx_event_collar;
#define ACX_SCORE_BAD_TABLE 1
#define ACX_SCORE_TILE_SEGMENTS 2048     /* segments one workgroup of acx_score_segments holds in LDS at a time */
ACX_API int acx_score_events(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity,
                             const int64_t* est_count, const int* est_status, int64_t B, int N, const int* steps /* device, B */,
                             const double* end_seconds /* device, B */, double step_seconds, const acx_event_collar* c,
                             int64_t* counts /* N*3 */, int64_t* ref_match /* n_ref */, int64_t* est_match /* capacity */,
                             int* status, void* stream);
ACX_API int acx_score_segments(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity,
                               const int64_t* est_count, const int* est_status, int64_t B, int N, const int* steps /* device, B */,
                               const double* end_seconds /* device, B */, double step_seconds, double time_resolution,
                               int64_t* counts /* N*3 */, int64_t* overall /* 6 */, int* status, void* stream);

/* ---- sound event scoring, intersection criteria: the counts that PSDS integrates ----------------------------------------------
 * The third scoring family (replaces: nothing in the reference; host loops over EventTable.to_lists() per threshold).  The
 * definitions are this project's own host functions, pytorch/sed_metrics.py::intersection_based_metrics_host and ::psds_host,
 * written after the polyphonic sound detection score of Bilen et al. (ICASSP 2020); psds_eval is not a dependency and nothing
 * claims equality with it.  Every output of acx_score_intersection is an integer and EQUALS the host definition's.
 * Tables, est_count / est_status, steps / end_seconds / step_seconds: as in "sound event scoring" above.
 * cover(a, b, rows) = the length of [a, b) that the union of rows (on, off), ascending in on, covers: with covered = a and
 *   total = 0.0, for each row until the first with on >= b:  lo = max(on, covered), hi = min(off, b);  if hi > lo: total += hi - lo,
 *   covered = hi.  A criterion with ratio rho holds when cover(...) >= rho * (b - a): float64, one product, not contracted.
 * Per (clip, class c) column:
 *   DTC   detection d is relevant when cover(d, the reference rows of (clip, c)) >= dtc * len(d); one that is not is an FP of c.
 *   GTC   reference event g is a TP when cover(g, the RELEVANT detections of (clip, c), in table order) >= gtc * len(g), else
 *         an FN.  A relevant detection whose annotation fails GTC is neither a TP nor an FP.
 *   CTTC  (cross_triggers != 0) for each FP d of class c and each class k != c with annotations in the clip:
 *         cover(d, the reference rows of (clip, k)) >= cttc * len(d) adds 1 to cross_triggers[c * N + k].  The diagonal stays 0.
 * counts[cls] = TP, FP, FN.  est_relevant[j] = 1 / 0 for the valid rows and -1 behind them (all `capacity` entries are
 * written); ref_hit[i] = 1 / 0.  An unusable estimated table sets ACX_SCORE_BAD_TABLE and leaves the outputs cleared: counts,
 * matrix and ref_hit 0, est_relevant -1.
 * Launch contract: the clears of the outputs, then one kernel (one wave per (clip, 64 classes), a lane per class), in order on
 * `stream`; no allocation, no workspace, no synchronisation, capturable; counts meet only in 64-bit integer atomic adds, so every
 * call gives the same bits.  n_ref == 0 (ref, ref_hit may be NULL) and capacity == 0 (est, est_relevant may be NULL) are legal;
 * cross_triggers (the matrix) may be NULL when c->cross_triggers == 0, and is not touched then.
 * Argument errors are returned before anything touches the device, with the codes of "sound event scoring"; in addition
 * ACX_ERR_ARG: dtc or gtc -- and cttc when c->cross_triggers != 0 -- not finite or outside (0, 1]; c->cross_triggers != 0 with a
 * NULL matrix.
 * acx_cross_trigger_rate: rate[c] = (sum over k != c with weight[k] > 0, ascending in k, of (double)cross_triggers[c * N + k] *
 *   weight[k]) / (the number of such k), 0 when there is none: one thread's sequential float64 sum per class, the order
 *   psds_host states, so a threshold sweep keeps one matrix and T rows of rates.  All three arrays on the device; one launch on
 *   `stream`, capturable.  ACX_ERR_ARG: a null pointer; ACX_ERR_SHAPE: N < 1 or N > ACX_MAX_CLASSES. */
typedef struct acx_intersection_criteria { double dtc, gtc, cttc; int32_t cross_triggers, reserved; } acx_intersection_criteria;
ACX_API int acx_score_intersection(const acx_ref_event* ref, int64_t n_ref, const acx_event* est, int64_t capacity,
                                   const int64_t* est_count, const int* est_status, int64_t B, int N,
                                   const int* steps /* device, B */, const double* end_seconds /* device, B */,
                                   double step_seconds, const acx_intersection_criteria* c, int64_t* counts /* N*3 */,
                                   int64_t* cross_triggers /* N*N or NULL */, int64_t* ref_hit /* n_ref */,
                                   int64_t* est_relevant /* capacity */, int* status, void* stream);
ACX_API int acx_cross_trigger_rate(const int64_t* cross_triggers /* N*N */, const double* weight /* N */, int N,
                                   double* rate /* N */, void* stream);

/* ---- live streams: tagging recordings that arrive chunk by chunk ----------------------------------------------------------
 * No reference counterpart.  A handle has `slots`; each slot holds one recording at a time.  Samples pushed to a slot are
 * appended to its open recording; acx_stream_close ends it and the slot's next push starts a new one.  Window W, hop H, the
 * input rate orig_hz and the timeline are fixed at create.  THE INVARIANT: everything a recording emits over all its pushes
 * and its close -- window starts, per-window outputs in the same order, timeline rows -- equals acx_forward_windows /
 * acx_window_timeline of the whole recording (after acx_resample of it at its rate), bit for bit, for any chunking.
 *
 * THE SCHEDULE (host only: acx_stream_schedule gives it for one slot from the geometry and its totals).  R = the final 32 kHz
 * samples of the open recording.  At 32 kHz a sample is final when pushed.  Resampling, output n = j nf + i is final once every
 * input sample its band reads has been pushed (and every earlier output is final); at close all ceil(nf L / of) outputs are,
 * reading zeros past the end as acx_resample does.  Then, cumulatively:
 *   - windows: while open, window j (start j H) once j H + W <= R.  At close, with L = the recording's 32 kHz length:
 *     L >= W: all n = 1 + ceil((L - W) / H), the last end-aligned at L - W;  ACX_MIN_SAMPLES <= L < W: one window, the clip
 *     itself;  L < ACX_MIN_SAMPLES: nothing (the recording is SHORT; no error, the other slots go on).
 *   - timeline rows: while open, row k once k H + H / 2 < R - W -- only then can no window still to come cover its midpoint,
 *     so the timeline trails the newest window by about one window length; at close, all ceil(L / H) rows (none if short).
 *   acx_stream_schedule: *samples = R, *windows / *rows = the windows / rows emitted so far by a recording with `pushed` input
 *   samples, open (closed = 0) or closed (closed = 1).  Any output pointer may be NULL.
 *
 * THE SIZES (host only: acx_stream_geometry gives them from the arguments of acx_stream_create, with the same argument checks;
 * acx_stream_create allocates what the same function computes).  Per slot: *adv = the largest 32 kHz advance of one push of
 * max_push input samples or of a close; *ring = C, the samples of the mirrored ring (2 C floats); *history = Ch, the samples of
 * the input history (0 at 32 kHz); *rows = Hw, the windows of the probability history (0 without a timeline).  Any output
 * pointer may be NULL.
 *
 * acx_stream_create: needs a finalized ctx; allocates the device state on ctx's device and synchronises (call it outside any
 * capture): per slot a
 * 32 kHz ring of 2 (W + the largest 32 kHz advance of one push) samples, an input history when orig_hz != 32000, and with
 * timeline = 1 the probabilities of about (W + max_push) / H + 4 windows, N floats each (N: the context's class count at
 * create).  max_push: the longest chunk, in input samples.  If the context is finalized again with a different N, the
 * handle's acx_stream_forward and acx_stream_timeline return ACX_ERR_STATE and write nothing.
 * Every other call allocates nothing and synchronises nothing; the launch calls run on `stream`, which must keep the handle's
 * work in order (one stream, or an event between two).  Slots, lengths and positions go to the kernels BY VALUE.
 *   acx_stream_push: n (1 .. ACX_MAX_VARLEN_CLIPS) chunks back to back in `chunks` (device fp32), chunk k of lengths[k]
 *   (0 .. max_push) input samples to slot[k]; the slots of one call are distinct.  acx_stream_close: end the recordings of
 *   the n listed slots (a slot never pushed to closes an empty recording).  Both return ACX_ERR_STATE for a slot with windows
 *   or rows that are not fetched yet: call acx_stream_forward until acx_stream_pending reports no window, then
 *   acx_stream_timeline, before the next push or close of that slot.
 *   acx_stream_pending: the windows and rows emitted and not fetched yet (host only).
 *   acx_stream_next: the next run of pending windows, in slot order and then start order, that share one length -- at most
 *   `max`: *count of them, *length (W, or a short clip's L), their slots and starts (32 kHz samples within the recording) in
 *   slot_of / start_of (host arrays of max, may be NULL).  Host only.
 *   acx_stream_forward: forwards the first `count` pending windows (a run of acx_stream_next) as acx_forward_windows does:
 *   outputs as acx_forward with B = count, L = length; workspace: acx_workspace_bytes_windows(ctx, count, length, mode).  With
 *   a timeline the mode must be ACX_MODE_LOGITS, and the probabilities are also kept for the rows.
 *   acx_stream_timeline: the pending rows (at most max_rows) of slots whose windows are all forwarded, in slot order and then
 *   step order: out = (rows, N) device fp32, slot_of / step_of host arrays, *n_rows their number.  reduce 0 = mean, 1 = max,
 *   the reduction of acx_window_timeline. */
typedef struct acx_stream acx_stream;
ACX_API int acx_stream_schedule(int64_t window, int64_t hop, int orig_hz, int64_t pushed, int closed, int64_t* samples,
                                int64_t* windows, int64_t* rows);
ACX_API int acx_stream_geometry(int64_t window, int64_t hop, int orig_hz, int64_t max_push, int timeline, int64_t* adv,
                                int64_t* ring, int64_t* history, int64_t* rows);
ACX_API int acx_stream_create(acx_ctx* ctx, int slots, int64_t window, int64_t hop, int orig_hz, int64_t max_push, int timeline,
                              acx_stream** out);
ACX_API void acx_stream_destroy(acx_stream* st);
ACX_API int acx_stream_push(acx_stream* st, const float* chunks, const int* slot, const int64_t* lengths, int n, void* stream);
ACX_API int acx_stream_close(acx_stream* st, const int* slot, int n, void* stream);
ACX_API int acx_stream_pending(const acx_stream* st, int64_t* windows, int64_t* rows);
ACX_API int acx_stream_next(const acx_stream* st, int max, int* slot_of, int64_t* start_of, int64_t* length, int* count);
ACX_API int acx_stream_forward(acx_stream* st, int count, int mode, float* out0, float* out1, void* workspace,
                               size_t workspace_bytes, void* stream);
ACX_API int acx_stream_timeline(acx_stream* st, int reduce, int64_t max_rows, float* out, int* slot_of, int64_t* step_of,
                                int64_t* n_rows, void* stream);

/* ---- input resampling: clips at any integer rate -> the model's 32 kHz ---------------------------------------------------
 * The reference resamples on the host before `.to(device)`: torchaudio.functional.resample with its defaults in the demo
 * (demo_convnext.py:53-59), librosa.load(sr=32000) in its extraction script (pytorch/extract_embeddings.py).  This is the
 * same band-limited interpolation as torchaudio 0.11's (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), on the
 * device.  With g = gcd(orig, new), of = orig / g, nf = new / g, base = min(of, nf) * 0.99, width = ceil(6 of / base):
 *   output n = j nf + i:  y[n] = sum_k h_i[k] x[j of + k - width]      (x = 0 outside the clip), ceil(nf L / of) outputs
 *   h_i[k] = (base / of) sinc(t) cos^2(pi t / 12),  t = (-i / nf + (k - width) / of) base
 * The taps are evaluated in float64 and rounded to fp32 once; a tap with |t| >= 6 is exactly zero and is not stored (~17 of
 * torchaudio's 459 per output remain at 44.1 kHz).  utils/resample.py, the host path, evaluates its taps in float32 (up to
 * 1.5e-5 from the formula at 44.1 kHz, ~3e-24 instead of 0 outside the band): the two agree to about that.
 * Each output is an fp32 FMA chain over its phase's stored band in ascending k, whatever the batch, the clip's position or
 * the tile: a clip's resampled bits are the same alone, in a uniform batch or packed among other clips.  fp32 in every
 * precision mode.  Non-finite input is out of scope: a NaN spreads over the ~17 outputs whose band holds it.
 * Rates are integers in [1, 768000]; a reduced ratio whose table exceeds nf * max_band = 2^22 taps (or whose input span per
 * 256 outputs exceeds the kernel's LDS budget) is ACX_ERR_UNSUPPORTED, the message naming of/nf.  44101 -> 32000 Hz
 * (32000 phases x 17 taps) fits.
 *
 * Host only (no device needed):
 *   acx_resample_geometry: of, nf, width and the longest band (any pointer may be NULL).
 *   acx_resample_taps: band_start[nf] (first stored k of each phase, 0 <= k < 2 width + of), band_count[nf], and the stored
 *     taps of phase 0, 1, ... back to back in taps[n_taps] (n_taps >= the sum of band_count; nf * max_band always suffices).
 *   acx_resampled_length: ceil(nf L / of), the output length of utils/resample.py.
 * Device:
 *   acx_resampler_create builds the tables and uploads them to `hip_device` (allocates and synchronises: call it outside a
 *   stream capture); acx_resample allocates nothing later.
 *   acx_resample: in = B clips back to back (sum(lengths) fp32 samples), out = their resampled clips back to back (the sum of
 *   acx_resampled_length), device memory; lengths = HOST array, 0 <= lengths[i] < 2^31, 1 <= B <= ACX_MAX_VARLEN_CLIPS (a
 *   uniform (B, L) batch is B equal lengths).  acx_forward's launch contract: one kernel on `stream`, the lengths passed by
 *   value, no allocation, no synchronisation, capturable.  Chain it with acx_forward / acx_forward_varlen on the same stream
 *   (INTEGRATION.md). */
typedef struct acx_resampler acx_resampler;
ACX_API int acx_resample_geometry(int orig_hz, int new_hz, int* of, int* nf, int* width, int* max_band);
ACX_API int acx_resample_taps(int orig_hz, int new_hz, int* band_start, int* band_count, float* taps, size_t n_taps);
ACX_API int acx_resampled_length(int orig_hz, int new_hz, int64_t L, int64_t* out);
ACX_API int acx_resampler_create(int hip_device, int orig_hz, int new_hz, acx_resampler** out);
ACX_API void acx_resampler_destroy(acx_resampler* rs);
ACX_API int acx_resample(const acx_resampler* rs, const float* in, const int64_t* lengths, int B, float* out, void* stream);

/* ---- augmented forwards: the reference's training-mode input transforms with the backbone frozen ---------------------------
 * The reference fine-tunes with the model in train mode (finetune_audiocaps.py): every forward then sees, in this order,
 * pydub_augment, roll_augment and SpeedPerturbation on the waveform (augmentations.py:266-351, convnext.py:288-295),
 * SpecAugmentation on the bn0'd log-mel (convnext.py:205-210, 308-309) and do_mixup (pytorch_utils.py:20-36, convnext.py:312-313).
 * Here they are two kernels driven by PLANS -- per-clip structs the caller draws on the host (pytorch/augment.py: draw_plan) and
 * keeps in device memory -- so that the calls allocate nothing, synchronise nothing and are capturable.  The definitions the
 * kernels equal bit for bit are augment_wave_host / augment_spec_host of pytorch/augment.py.
 *
 * acx_wave_aug (40 bytes), one per clip of L samples: the composite of gain, roll, nearest-neighbour stretch and pad / crop,
 *     out[i] = gain * in[(src(i + shift) - roll) mod L]   if 0 <= i + shift < n_out, else +0
 *     src(j) = min(L - 1, rint(j * step))                 evaluated in FLOAT64, ties to even
 *   step = 1 / rate; n_out = ceil(L / step), the stretched length (Resample.resample_nearest); shift = the crop's start
 *   (n_out > L: 0 .. n_out - L) or minus the left padding (n_out < L: n_out - L .. 0); roll reduced to 0 <= roll < L
 *   (x.roll(r): out[i] = in[(i - r) mod L]); gain = float32 of 10 ** (dB / 20).  The reference forms src with a float32
 *   torch.arange whose values depend on torch's CPU vectoriser and thread count; where the step is exact in binary every scheme
 *   agrees, and that is where this definition is pinned to it.
 * acx_spec_aug (64 bytes), one per clip of T = acx_num_frames(L) frames: up to ACX_AUG_MAX_STRIPES stripes per axis, frames
 *   [t_bgn, t_bgn + t_len) and mel bins [f_bgn, f_bgn + f_len) become +0.0 (DropStripes zeroes AFTER bn0); a stripe of length
 *   0 is legal and is how unused slots are filled.
 * lambda: B float32 values on the device; output row b = fl(mask(row 2b) * lambda[2b]) + fl(mask(row 2b + 1) * lambda[2b + 1]),
 *   two rounded products and one rounded sum, each row masked with its own stripes first.  B must be even.
 *
 * acx_augment_plan_check: HOST arrays (either may be null) -- stripe bounds, 0 <= roll < L, n_out == ceil(L / step) in
 *   1 .. 2^31 - 1, shift in its range; call it before uploading a plan.  No device is touched.
 * acx_augment_wave: wav, out (B, L) device, out != wav.  acx_augment_spec: feat (B, T, 224), 16-byte aligned; lambda == null: the
 *   masks are written IN PLACE (out == feat, only the masked elements are stored, plan non-null); lambda != null: out is a second
 *   (B / 2, T, 224) buffer, feat is left untouched, plan may be null.  One kernel each on `stream`.
 * acx_forward_features: acx_forward from the stem on -- feat = (B, T, 224) bn0'd log-mel rows (acx_logmel_bn0's output, or the
 *   caller's own features), 16-byte aligned, T = acx_num_frames(L).  Same sub-batch split, same workspace (acx_workspace_bytes),
 *   same outputs as acx_forward; acx_forward_features(acx_logmel_bn0(wav)) equals acx_forward(wav) bit for bit.
 * acx_forward_augmented: wave kernel (wave_plan non-null), the frontend over all B clips, spec kernel (spec_plan or lambda
 *   non-null), then acx_forward_features over B clips -- B / 2 with lambda, as the reference's output has.  Its extra buffers are
 *   carved from its own workspace, acx_workspace_bytes_augmented(ctx, B, L, wave_plan != null, lambda != null, mode);
 *   acx_workspace_bytes does not change.  With all three null it equals acx_forward bit for bit. */
#define ACX_AUG_MAX_STRIPES 4
typedef struct acx_wave_aug {
    double step;
    int64_t n_out, shift, roll;
    float gain;
    int32_t reserved;
} acx_wave_aug;
typedef struct acx_spec_aug {
    int32_t t_bgn[ACX_AUG_MAX_STRIPES], t_len[ACX_AUG_MAX_STRIPES], f_bgn[ACX_AUG_MAX_STRIPES], f_len[ACX_AUG_MAX_STRIPES];
} acx_spec_aug;
ACX_API int acx_augment_plan_check(int B, int64_t L, const acx_wave_aug* wave, const acx_spec_aug* spec);
ACX_API int acx_augment_wave(const float* wav, int B, int64_t L, const acx_wave_aug* plan, float* out, void* stream);
ACX_API int acx_augment_spec(float* feat, int B, int T, const acx_spec_aug* plan, const float* lambda, float* out, void* stream);
ACX_API int acx_forward_features(acx_ctx* ctx, const float* feat, int B, int64_t L, int mode, float* out0, float* out1,
                                 void* workspace, size_t workspace_bytes, void* stream);
ACX_API int acx_workspace_bytes_augmented(const acx_ctx* ctx, int B, int64_t L, int has_wave_plan, int has_lambda, int mode,
                                          size_t* out_bytes);
ACX_API int acx_forward_augmented(acx_ctx* ctx, const float* wav, int B, int64_t L, const acx_wave_aug* wave_plan,
                                  const acx_spec_aug* spec_plan, const float* lambda, int mode, float* out0, float* out1,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-GPU: the one collective of the path -----------------------------------------------------------------
 * One process per GPU, full weight replica, clips sharded; logits / probabilities / scene rows are all-gathered over xGMI by
 * RCCL (ncclAllGather), frame embeddings stay sharded.  The reference has no inference-time collective (training DDP only,
 * main.py:641,992-997); the Python host reaches the same collective through torch.distributed (parallel.py).  librccl.so is
 * opened on first use: a single-GPU process never loads it.
 *   rank 0: acx_comm_unique_id(id) -> share the ACX_COMM_ID_BYTES bytes with every rank (file, TCP store, MPI ...)
 *   all   : acx_comm_init(ctx, rank, world, id)         (collective: every rank must call it)
 *   step  : acx_allgather(ctx, send, recv, bytes_per_rank, stream)   recv = world * bytes_per_rank device bytes, rank order;
 *           enqueued on `stream` behind the forward that produced `send` -- no host synchronisation.
 * The communicator belongs to the context (released by acx_destroy). */
#define ACX_COMM_ID_BYTES 128
ACX_API int acx_comm_unique_id(void* id_out);
ACX_API int acx_comm_init(acx_ctx* ctx, int rank, int world, const void* unique_id);
ACX_API int acx_allgather(acx_ctx* ctx, const void* send, void* recv, size_t bytes_per_rank, void* stream);
ACX_API int acx_comm_info(const acx_ctx* ctx, int* rank, int* world);

/* ---- per-kernel entry points (golden-vector tests, rocprofv3 isolation, roofline bench) ---- */

/* K1: Spectrogram + LogmelFilterBank + bn0 (convnext.py:298-306). out (B,T,224). */
ACX_API int acx_logmel_bn0(acx_ctx* ctx, const float* wav, int B, int64_t L, float* out, int apply_bn0,
                   void* stream);
/* K2: stem Conv2d(1,96,4x4,s4,pad(4,0)) + LayerNorm (convnext.py:688-691,227).
 * in (B,T,224) -> out NHWC (B,H0,56,96). */
ACX_API int acx_stem_ln(acx_ctx* ctx, const float* in, int B, int T, float* out, void* stream);
/* K3: Block.dwconv 7x7 depthwise + bias (convnext.py:58-60,76), NHWC in/out, plus the per-pixel
 * LayerNorm statistics (mean, rstd) of the output (convnext.py:78) into stats (B*H*W, 2). */
ACX_API int acx_dwconv7(acx_ctx* ctx, int stage, int block, const float* x, float* y, float* stats, int B,
                int H, int W, void* stream);
/* K3 on bf16 activations -- the storage type of stages 0-2 under ACX_PREC_BF16_ACT (x, y: NHWC bf16, 2 bytes per element;
 * any other precision or stage 3: ACX_ERR_STATE).  Matrix-pipe form: weights rounded to bf16, products exact, fp32
 * accumulation from the bias, one rounding to bf16 at the end (convnext.py:58-60,76). */
ACX_API int acx_dwconv7_bf16(acx_ctx* ctx, int stage, int block, const uint16_t* x, uint16_t* y, int B, int H, int W,
                     void* stream);
/* K3 + K4: whole Block.forward (convnext.py:74-87) on NHWC x, in place: depthwise conv, then LayerNorm + pwconv1 + GELU +
 * pwconv2 + gamma + residual (convnext.py:78-86).  Stages 0-1 (ACX_PREC_F32) or 0-2 (the other precisions) run the
 * MLP as ONE fused kernel that keeps the hidden activation in registers; the remaining stages run two MFMA GEMMs through
 * the hidden scratch.
 * scratch >= acx_block_scratch_bytes, 256-byte aligned. */
ACX_API int acx_block(acx_ctx* ctx, int stage, int block, float* x, int B, int H, int W, void* scratch,
              size_t scratch_bytes, void* stream);
ACX_API int acx_block_scratch_bytes(int stage, int B, int H, int W, size_t* out_bytes);
/* K5: downsample_layers[i], i=1..3: LayerNorm + Conv2d 2x2 s2 (convnext.py:230-235).
 * x NHWC (B,H,W,C_{i-1}) -> out NHWC (B,H/2,W/2,C_i); scratch (B*H*W*C_{i-1}) fp32 receives the
 * normalised copy of x that the 2x2 gather GEMM reads. */
ACX_API int acx_downsample(acx_ctx* ctx, int i, const float* x, float* out, float* scratch, int B, int H,
                   int W, void* stream);
/* K6: pooling + final LayerNorm + head + sigmoid (convnext.py:279-285,321-325).
 * x NHWC (B,H3,7,768); scene (B,768), logits / probs (B,N). Any of scene/logits/probs may be NULL.  Always the fused
 * one-workgroup-per-clip kernel (the forwards take the class-tiled head kernel for wide heads; both give the same bits). */
ACX_API int acx_pool_head(acx_ctx* ctx, const float* x, int B, int H3, float* scene, float* logits,
                  float* probs, void* stream);
/* NHWC -> NCHW (the layout forward_frame_embeddings returns, convnext.py:276-277). */
ACX_API int acx_nhwc_to_nchw(const float* x, float* out, int B, int H, int W, int C, void* stream);

/* Stored clips -> model input, on the device: out[i] = float(double(pcm[i]) / 32767.0), the arithmetic (and therefore the
 * bits) of the reference's host-side `int16_to_float32` (utils/utilities.py:226-227; applied by the AudioSet dataset,
 * utils/data_generator.py:72).  The evaluation sweep copies the int16 clips over PCIe (half the bytes) and widens them here,
 * in stream order in front of acx_forward.  Both buffers on the device, 16-byte aligned; n samples. */
ACX_API int acx_pcm16_to_f32(const int16_t* pcm, float* out, int64_t n, void* stream);

/* ---- evaluation statistics: per-class AP, ROC-AUC and d' on the device ----------------------------------------------------
 * The reference scores its evaluation on the host (pytorch/evaluate.py:44-58): sklearn average_precision_score and
 * roc_auc_score with average=None, then sqrt(2) * scipy.stats.norm.ppf(auc).  These are the same statistics, exact up to
 * float64 rounding.  For class c with scores s (float32; -0.0 == +0.0, equal values are one threshold), labels y in {0, 1},
 * P positives and Nn negatives:
 *   ap[c]     = (1/P) sum over distinct positive scores t of npos(s == t) TP(>= t) / (TP(>= t) + FP(>= t));   P = 0: 0.0
 *   auc[c]    = sum over positives i of (2 #neg(s < s_i) + #neg(s == s_i)), an exact int64, divided once by 2 P Nn (float64);
 *               P = 0 or Nn = 0: NaN
 *   dprime[c] = 2 erfinv(2 auc - 1) = sqrt(2) Phi^-1(auc): +inf at auc = 1, -inf at auc = 0, NaN stays NaN
 * scores: device (n, classes) fp32 with row stride ld_scores; target: device (n, classes) of target_dtype (ACX_TARGET_F32 or
 * ACX_TARGET_U8, e.g. a bool tensor) with row stride ld_target; both may be column slices of wider rows.  ap / auc / dprime:
 * device float64 [classes]; status: one device int32.
 *   acx_metrics_workspace_bytes: workspace for (n, classes), non-decreasing in both (host only).
 *   acx_tagging_metrics: ARGUMENT errors return a negative status (null pointer, n < 1, classes < 1, a row stride shorter than
 *   classes, a workspace too small or not 256-byte aligned; n > 2^30 is ACX_ERR_UNSUPPORTED).  DATA errors are reported only
 *   through *status, which the call sets to the OR of ACX_METRICS_NONFINITE (a NaN or +-inf score) and ACX_METRICS_BAD_TARGET
 *   (a target other than 0 or 1), 0 when the data is valid; on a data error every output is NaN.  acx_forward's launch
 *   contract: every launch in order on `stream` (a 4-byte clear of *status and two kernels), no allocation, no synchronisation,
 *   capturable; the results are the same bits on every call whatever the workspace holds.  n <= 32768 sorts each class in LDS;
 *   larger n goes through the workspace. */
enum acx_target_dtype { ACX_TARGET_F32 = 0, ACX_TARGET_U8 = 1 };
#define ACX_METRICS_NONFINITE 1
#define ACX_METRICS_BAD_TARGET 2
ACX_API int acx_metrics_workspace_bytes(int64_t n, int classes, size_t* out_bytes);
ACX_API int acx_tagging_metrics(const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                                int64_t ld_target, int64_t n, int classes, double* ap, double* auc, double* dprime,
                                int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- operating points: one decision threshold per class, chosen and scored on the device ------------------------------------
 * The reference decides with fixed cut-offs (pytorch/inference.py thresholds its outputs with 0.5-style constants for every
 * class); choosing a threshold per class on a labelled set is otherwise sklearn.metrics.precision_recall_curve looped over the
 * classes on the host.  The decision rule everywhere is score >= threshold, float32, -0.0 == +0.0 (the decoder's p >= thr and
 * the convention of sklearn's PR curve).  For class c with P positives and Nn negatives the CANDIDATES are the distinct scores
 * of its positives -- any other threshold is dominated: raising it to the next positive score keeps TP and cannot raise FP --
 * and for a candidate t:  TP = P - #pos(< t),  FP = Nn - #neg(< t),  FN = P - TP,  TN = Nn - FP.
 *   ACX_OP_FBETA (param = beta > 0, finite): the candidate with the largest F, float64, every operation rounded on its own (no
 *     fused multiply-add):  b2 = beta * beta;  num = (1 + b2) * TP;  den = (num + b2 * FN) + FP;  F = num / den.  Among equal F
 *     the highest threshold.
 *   ACX_OP_PRECISION (param = p in (0, 1]): the lowest candidate with (double)TP / (double)(TP + FP) >= p: the most recall at
 *     that precision.
 *   ACX_OP_RECALL (param = r in (0, 1]): the highest candidate with (double)TP / (double)P >= r.
 *   No qualifying candidate (no positives, or a precision that no candidate reaches): threshold +inf, counts (0, 0, P, Nn) -- the
 *   class never fires.  A zero threshold is returned as +0.0.
 * pytorch/metrics.py::operating_points_host states the same in numpy float64; the device equals it bit for bit.
 *   acx_operating_points: inputs, workspace (acx_metrics_workspace_bytes), argument errors, status bits and launch contract of
 *     acx_tagging_metrics (a 4-byte clear and two kernels on `stream`, capturable, no context; the same bits on every call);
 *     spec is read on the host; ACX_ERR_ARG for an unknown criterion or a param outside its range.  thresholds: device fp32
 *     [classes]; counts: device int64 [classes][4] = TP, FP, FN, TN.  On a data error every threshold is NaN, every count -1.
 *   acx_threshold_counts: TP, FP, FN, TN of score >= thresholds[c] (device fp32 [classes], +-inf allowed) on any (n, classes)
 *     scores and targets -- thresholds picked on a validation split scored on a test split.  No workspace, no sort: two clears,
 *     one counting kernel (integer sums combined by integer atomics: the same result in any order) and one finishing kernel on
 *     `stream`, capturable.  A NaN threshold sets ACX_METRICS_BAD_THRESHOLD; on any data error every count is -1. */
enum acx_operating_criterion { ACX_OP_FBETA = 0, ACX_OP_PRECISION = 1, ACX_OP_RECALL = 2 };
typedef struct acx_operating_spec { int32_t criterion; double param; } acx_operating_spec;
#define ACX_METRICS_BAD_THRESHOLD 4
ACX_API int acx_operating_points(const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                                 int64_t ld_target, int64_t n, int classes, const acx_operating_spec* spec,
                                 float* thresholds /* [classes] */, int64_t* counts /* [classes][4] = TP, FP, FN, TN */,
                                 int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_threshold_counts(const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                                 int64_t ld_target, int64_t n, int classes, const float* thresholds /* device, [classes] */,
                                 int64_t* counts /* [classes][4] */, int32_t* status, void* stream);

/* ---- bootstrap resamples and weighted statistics: confidence intervals for mAP, AUC and d' ---------------------------------
 * A clip-level bootstrap resamples the n clips with replacement and recomputes the statistics.  A resample changes no score, so
 * it is a vector of integer weights (how often each clip was drawn) over an order that is computed once per class; the same
 * call gives sklearn's `sample_weight` statistics for any non-negative integer weights (stratified or block resampling).
 * DRAWS.  mix(z) is splitmix64's finaliser in uint64 wrap-around arithmetic:
 *     z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27; z *= 0x94D049BB133111EB;  z ^= z >> 31
 *   and draw j (0 <= j < n <= 2^30) of replicate r (0 <= r < 2^32) is
 *     x = mix(mix(seed) + 0x9E3779B97F4A7C15 * (((r << 32) | j) + 1));   idx = ((x >> 32) * n) >> 32
 *   Replicate r draws idx(r, 0 .. n-1); its weight vector is the count of each row among them, so it sums to n.  The
 *   multiply-shift maps 2^32 values onto n rows: a row's probability differs from 1/n by at most 2^-32, a relative bias of at
 *   most n / 2^32 (a contract, not a statistical claim).  pytorch/metrics.py::bootstrap_indices_host states the same in numpy.
 * WEIGHTED STATISTICS of class c under one weight vector w (int32, >= 0), scores and labels as acx_tagging_metrics takes them:
 *   Pw = sum of w over the positives, Nw = over the negatives; for each distinct positive score t whose positives have total
 *   weight g > 0:  TPw = weight of positives with score >= t,  FPw = weight of negatives with score >= t
 *   ap     = (1/Pw) sum_t g TPw / (TPw + FPw)                                   (float64)
 *   auc    = sum_t g (2 Nw(< t) + Nw(= t)), an exact int64, divided once by 2 Pw Nw   (float64)
 *   dprime = 2 erfinv(2 auc - 1)
 *   Pw = 0: ap, auc and dprime are all NaN -- a resample that drew no positive says nothing about the class.  (This differs on
 *   purpose from acx_tagging_metrics' ap = 0 for P = 0.)  Nw = 0 and Pw > 0: ap = 1, auc and dprime NaN.
 *   With every weight 1 these are acx_tagging_metrics' values; with w the counts of a resample they are the statistics of the
 *   resampled rows.  pytorch/metrics.py::weighted_metrics_host states them in numpy.
 *   acx_bootstrap_weights: weights[k][0 .. n-1] (device int32, row stride ld_w >= n) = the weight vector of replicate
 *     first_replicate + k, k < replicates -- a chunk computed alone equals the same rows of a larger call.  One clear and one
 *     kernel on `stream` (integer atomics: the same counts in any order), capturable.  ACX_ERR_ARG for a null pointer, n < 1,
 *     replicates < 1, ld_w < n or first_replicate + replicates > 2^32; n > 2^30 is ACX_ERR_UNSUPPORTED.
 *   acx_weighted_metrics_workspace_bytes: workspace of acx_weighted_metrics for (n, classes) (host only).
 *   acx_weighted_metrics: inputs, argument errors, status-word convention and launch contract of acx_tagging_metrics (a 4-byte
 *     clear and four kernels on `stream`: no context, no allocation, no synchronisation, capturable; argument errors return
 *     before anything touches the device; the same bits on every call whatever the workspace holds).  weights: device int32
 *     (replicates, n) with row stride ld_w >= n; ap / auc / dprime: device float64 [replicates][classes].  replicates < 1 and
 *     ld_w < n are ACX_ERR_ARG.  n > 32768 is ACX_ERR_UNSUPPORTED: the recount keeps one int32 weight bucket per row of a class
 *     in LDS (128 KiB).  A negative weight, or a weight vector that sums to more than 2^30 (the bound under which the int32
 *     buckets and the int64 AUC numerator cannot overflow), sets ACX_METRICS_BAD_WEIGHT; on any data error every output is NaN. */
#define ACX_METRICS_BAD_WEIGHT 8
ACX_API int acx_bootstrap_weights(uint64_t seed, uint32_t first_replicate, int replicates, int64_t n, int32_t* weights,
                                  int64_t ld_w, void* stream);
ACX_API int acx_weighted_metrics_workspace_bytes(int64_t n, int classes, size_t* out_bytes);
ACX_API int acx_weighted_metrics(const float* scores, int64_t ld_scores, const void* target, int target_dtype,
                                 int64_t ld_target, int64_t n, int classes, const int32_t* weights, int64_t ld_w, int replicates,
                                 double* ap /* [replicates][classes] */, double* auc, double* dprime, int32_t* status, void* ws,
                                 size_t ws_bytes, void* stream);

/* ---- fitting a classifier head on frozen scene embeddings -----------------------------------------------------------------
 * The reference fine-tunes with the whole model in train mode (pytorch/finetune_audiocaps.py: base frozen, BCELoss on
 * clipwise_output, optim.Adam(amsgrad=True); pytorch/main.py:648 AdamW).  With the backbone frozen the head's input -- the scene
 * embedding norm(pool(x)), convnext.py:285,321 -- never changes, so training is logits = E W^T + b, binary cross-entropy, Adam,
 * on embeddings computed once.  Stateless: the caller owns every buffer (all on the device, fp32 unless said otherwise):
 *   E (n_rows_total, 768) with row stride ld_e (16-byte aligned, ld_e a multiple of 4); target (n_rows_total, classes) of
 *   target_dtype (ACX_TARGET_U8: 0 / 1; ACX_TARGET_F32: any value in [0, 1], soft targets allowed) with row stride ld_target;
 *   idx: `rows` int64 row numbers into E / target, the mini-batch (repeats allowed; nothing is copied or shuffled in memory);
 *   W (classes, 768) 16-byte aligned, b (classes); the moments mW, vW, vmaxW like W and mb, vb, vmaxb like b, zero before step 1
 *   (vmax* may be NULL unless hp->amsgrad); status: one int32, which the calls OR into and never clear.
 * One step t = 1, 2, ... with G = (sigmoid(z) - y) / (rows classes), z = E[idx] W^T + b:
 *   g = G^T E[idx] (for W), sum_rows G (for b);   Adam: g += weight_decay p;   AdamW (hp->decoupled): p *= 1 - lr weight_decay;
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  amsgrad: vmax = max(vmax, v) replaces v below;
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)           -- torch.optim.Adam / AdamW, single-tensor form
 *   *loss_out = mean over (rows, classes) of -[y max(log p, -100) + (1 - y) max(log(1 - p), -100)]   (F.binary_cross_entropy)
 * The scalars that depend on hp, step_t and lr alone are evaluated in double and rounded to fp32 once.  G is the exact
 * BCE-with-logits gradient; the reference's sigmoid-then-BCELoss autograd equals it except where the fp32 sigmoid saturates
 * (|z| >~ 16.6), where autograd returns 0.  Products and sums are fp32 (f32 matrix instructions), combined in a fixed order: the
 * same inputs give the same bits on every call; acx_set_precision has no influence.
 *   acx_head_fit_workspace_bytes: workspace for steps of up to rows_max rows, non-decreasing in both arguments (host only).
 *   acx_head_fit_step: the step above, W / b / moments updated in place.  Two launches.
 *   acx_head_fit_grad: the same gradient pass without an update: z and G (rows, classes), dW (classes, 768), db (classes) and
 *     *loss to caller buffers.  acx_adam_update: the element-wise update of n parameters from a gradient buffer.
 *     acx_head_fit_grad, then acx_adam_update on (W, dW) and (b, db), leaves the bits of acx_head_fit_step.
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable; step_t and lr
 * travel by value.  ARGUMENT errors return a negative status before any launch, acx_last_error naming the argument: a null
 * pointer, rows < 1, classes outside 1 .. ACX_MAX_CLASSES, a row stride shorter than its row, E or W not 16-byte aligned or
 * ld_e not a multiple of 4, a workspace too small or not 256-byte aligned (ACX_ERR_WORKSPACE), beta outside [0, 1), eps <= 0, weight_decay < 0, lr < 0, step_t < 1; rows > 2^22 is
 * ACX_ERR_UNSUPPORTED.  An idx entry outside [0, n_rows_total) is a DATA error: it is clamped into the range (nothing outside E
 * or target is read) and ACX_FIT_BAD_INDEX is ORed into *status. */
typedef struct acx_adam {
    double beta1, beta2, eps, weight_decay;
    int amsgrad;     /* keep the running maximum of v and divide by it */
    int decoupled;   /* 0: Adam (weight decay added to the gradient), 1: AdamW */
} acx_adam;
#define ACX_FIT_BAD_INDEX 1
ACX_API int acx_head_fit_workspace_bytes(int64_t rows_max, int classes, size_t* out_bytes);
ACX_API int acx_head_fit_step(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                              int64_t ld_target, const int64_t* idx, int64_t rows, int classes, float* W, float* b, float* mW,
                              float* vW, float* vmaxW, float* mb, float* vb, float* vmaxb, const acx_adam* hp, int64_t step_t,
                              double lr, float* loss_out, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_head_fit_grad(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                              int64_t ld_target, const int64_t* idx, int64_t rows, int classes, const float* W, const float* b,
                              float* z, float* G, float* dW, float* db, float* loss, int32_t* status, void* ws, size_t ws_bytes,
                              void* stream);
ACX_API int acx_adam_update(float* param, const float* grad, float* m, float* v, float* vmax, int64_t n, const acx_adam* hp,
                            int64_t step_t, double lr, void* stream);

/* Single-label heads: softmax cross-entropy instead of BCE.  labels: n_rows_total int64 class numbers (the label of batch row r
 * is labels[idx[r]]); everything else as above.  One step with q_c = (1 - label_smoothing) [c = label] + label_smoothing /
 * classes, per row m = max_c z_c, s = sum_c expf(z_c - m), p_c = expf(z_c - m) / s:
 *   G = (p - q) / rows;   *loss_out = mean over rows of (m + log s) - sum_c q_c z_c
 * -- F.cross_entropy(z, labels, label_smoothing=...), reduction mean -- then the update above.  Three launches: the logits to
 * the workspace, the row pass, the update kernel of acx_head_fit_step.  Row sums run in a fixed order that depends on
 * `classes` alone (depth ceil(classes / 64) + 6 up to 2048 classes, ceil(classes / 256) + 9 beyond); a row's z bits depend
 * on that row alone -- not on `rows`, the other rows of the batch or the row's place in it (the logits launch picks its tile shape
 * from `classes`) -- and so does its G up to the one factor 1 / rows: equal G bits at equal `rows`.  classes = 1 gives G = 0 and loss = 0 exactly.
 *   acx_head_fit_ce_workspace_bytes: G + z + one loss partial per row.  acx_head_fit_step_ce / acx_head_fit_grad_ce: the
 *   counterparts of acx_head_fit_step / acx_head_fit_grad, with the same contract (acx_head_fit_grad_ce, then acx_adam_update on
 *   (W, dW) and (b, db), leaves the bits of acx_head_fit_step_ce).  label_smoothing outside [0, 1) is ACX_ERR_ARG.  A label
 *   outside [0, classes) is a DATA error: it is clamped into the range and ACX_FIT_BAD_LABEL is ORed into *status. */
#define ACX_FIT_BAD_LABEL 2
ACX_API int acx_head_fit_ce_workspace_bytes(int64_t rows_max, int classes, size_t* out_bytes);
ACX_API int acx_head_fit_step_ce(const float* E, int64_t ld_e, int64_t n_rows_total, const int64_t* labels, const int64_t* idx,
                                 int64_t rows, int classes, double label_smoothing, float* W, float* b, float* mW, float* vW,
                                 float* vmaxW, float* mb, float* vb, float* vmaxb, const acx_adam* hp, int64_t step_t, double lr,
                                 float* loss_out, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_head_fit_grad_ce(const float* E, int64_t ld_e, int64_t n_rows_total, const int64_t* labels, const int64_t* idx,
                                 int64_t rows, int classes, double label_smoothing, const float* W, const float* b, float* z,
                                 float* G, float* dW, float* db, float* loss, int32_t* status, void* ws, size_t ws_bytes,
                                 void* stream);

/* Sound event detection heads from clip-level labels: multiple-instance learning.  acx_head_fit_step trains on scene embeddings;
 * detection applies the head to every 0.32 s segment embedding and pools over time ("sound event detection" above).  These calls
 * train along that path -- the reference's decision-level recipe, pytorch/models.py:5757-5771 (head per segment, sigmoid, pooling
 * over time) with pytorch/losses.py clip_bce (F.binary_cross_entropy on the pooled clip probability): a clip is a BAG, its
 * segments are the instances, only the bag has a label.
 *   E (n_rows_total, 768): the segment embeddings of all clips back to back (acx_head_fit_step's layout rules);
 *   target (n_bags_total, classes): one row per clip, of target_dtype, row stride ld_target.
 * A step takes `bags` clips: bag_idx (`bags` int64 target rows; repeats allowed), bag_off (`bags` + 1 int32: bag i owns the rows
 * [bag_off[i], bag_off[i + 1]) of the step; bag_off[0] = 0, non-decreasing, bag_off[bags] = seg_rows) and seg_idx (seg_rows int64
 * rows of E, in bag order), all on the device; seg_rows and bags travel by value.  With z = E[seg_idx] W^T + b -- the bits
 * acx_head_fit_grad_ce writes for those rows -- and q_t = sigmoid(z_t) over the S rows of a bag, per class:
 *   ACX_MIL_MAX     P = sigmoid(z_t*), t* the LOWEST t that attains max_t z_t         dP/dq_t = [t = t*]
 *   ACX_MIL_MEAN    P = (sum q_t) / S                                                 dP/dq_t = 1 / S
 *   ACX_MIL_LINEAR  P = sum q_t^2 / sum q_t   (sum q_t = 0: P = 0, no gradient)       dP/dq_t = (2 q_t - P) / sum q_t
 *   ACX_MIL_EXP     P = sum q_t e^q_t / sum e^q_t                                     dP/dq_t = e^q_t (1 + q_t - P) / sum e^q_t
 *   loss term -[y max(log P, -100) + (1 - y) max(log1p(-P), -100)],  dL/dP = (P - y) / max(P (1 - P), 1e-12)
 *   G[t] = dL/dP dP/dq_t q_t (1 - q_t) / (bags classes);  *loss_out = the mean of the terms over (bags, classes)
 * -- torch's binary_cross_entropy on a probability and its backward -- then acx_head_fit_step's update with g = G^T E[seg_idx],
 * sum_rows G.  An empty bag has P = 0, no gradient, and its loss term.  All fp32, every sum in ascending t per (bag, class), the
 * loss terms added in a fixed order: the same inputs give the same bits on every call.  Three launches.
 *   acx_head_fit_mil_workspace_bytes: for steps of up to seg_rows_max rows and bags_max bags; non-decreasing (host only).
 *   acx_head_fit_step_mil: the step.  acx_head_fit_grad_mil: the same pass without the update -- z, G (seg_rows, classes), P
 *     (bags, classes), dW, db and *loss to caller buffers; followed by acx_adam_update on (W, dW) and (b, db) it leaves the bits
 *     of acx_head_fit_step_mil.
 *   acx_segment_pool: the forward half alone, the same device function and so the same bits as P: logits (rows, classes) with
 *     row stride ld, bag_off as above (bag_off[bags] rows are read), out (bags, classes).  How a head trained with MEAN / LINEAR /
 *     EXP gets its clip probability at inference; acx_forward_segments' clipwise output stays the maximum.
 * The launch contract and the ARGUMENT errors of acx_head_fit_step; also bags < 1, seg_rows < 1, a pool that is no acx_mil_pool
 * (ACX_ERR_ARG); seg_rows or bags > 2^22 (ACX_ERR_UNSUPPORTED).  DATA errors: a seg_idx or bag_idx entry out of range is clamped
 * and ORs ACX_FIT_BAD_INDEX into *status; a bag_off entry below its predecessor (the bag is then empty), below 0 or beyond
 * seg_rows, a first entry other than 0 or a last one other than seg_rows is clamped -- nothing outside the buffers is touched,
 * every row of G is written -- and ORs ACX_FIT_BAD_BAG.  acx_segment_pool knows no seg_rows: it flags negative and decreasing
 * entries only. */
#define ACX_FIT_BAD_BAG 4
enum acx_mil_pool { ACX_MIL_MAX = 0, ACX_MIL_MEAN = 1, ACX_MIL_LINEAR = 2, ACX_MIL_EXP = 3 };
ACX_API int acx_head_fit_mil_workspace_bytes(int64_t seg_rows_max, int64_t bags_max, int classes, size_t* out_bytes);
ACX_API int acx_head_fit_step_mil(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                                  int64_t ld_target, int64_t n_bags_total, const int64_t* seg_idx, int64_t seg_rows,
                                  const int32_t* bag_off, const int64_t* bag_idx, int64_t bags, int classes, int pool, float* W,
                                  float* b, float* mW, float* vW, float* vmaxW, float* mb, float* vb, float* vmaxb,
                                  const acx_adam* hp, int64_t step_t, double lr, float* loss_out, int32_t* status, void* ws,
                                  size_t ws_bytes, void* stream);
ACX_API int acx_head_fit_grad_mil(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                                  int64_t ld_target, int64_t n_bags_total, const int64_t* seg_idx, int64_t seg_rows,
                                  const int32_t* bag_off, const int64_t* bag_idx, int64_t bags, int classes, int pool,
                                  const float* W, const float* b, float* z, float* P, float* G, float* dW, float* db, float* loss,
                                  int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_segment_pool(const float* logits, int64_t ld, const int32_t* bag_off, int64_t bags, int classes, int pool,
                             float* out /* (bags, classes) */, int32_t* status, void* stream);

/* Groups: `jobs` independent fits (1 .. ACX_FIT_MAX_JOBS: the folds of a cross-validation, the settings of a grid) over the SAME
 * E and target / labels, advanced together: one group step launches each stage ONCE for all jobs (BCE: the gradient pass, once
 * per tile form that can occur, and the update; cross-entropy: logits, row pass, update).  The jobs share classes, the loss,
 * label_smoothing, rows_max (the batch size) and hp->amsgrad / hp->decoupled; each has its own batch (so its own training subset
 * and epoch order), its own row count per step -- 0: the job sits the step out and NOTHING of it is written -- and its own W, b,
 * moments, optimiser scalars, step count, loss outputs and status word.
 *   Every job's W, b, loss outputs and status have the bits of the acx_head_fit_step / _step_ce calls it replaces: each job runs
 *   the tile form its own single call would (decided per job on the device by the single call's rule) and the same orders of
 *   addition; its step count t advances only in the steps in which it has rows.
 * acx_fit_job: a job's DEVICE pointers; the table of `jobs` of them lives on the device.  idx: the job's batches of all steps
 * (int64 rows of E, as acx_head_fit_step's idx); loss: one float per step in which the job has rows, in order; the rest as
 * acx_head_fit_step's (W 16-byte aligned; vmaxW / vmaxb may be NULL unless amsgrad).  The host cannot check these.
 * The plan: what changes from step to step -- (row count, offset of the batch in the job's idx, 1 / count, the optimiser scalars
 * of the job's step t with that step's lr) per (step, job) -- evaluated on the HOST by the single calls' own code, once, before
 * the first step.  acx_head_fit_plan_bytes: 64 bytes per entry.  acx_head_fit_plan_fill (host only, no device needed): rows,
 * idx_offset and lr are [n_steps][jobs] (idx_offset and lr are not read where rows is 0), hp is [jobs]; writes plan_bytes of HOST
 * memory, which the caller copies to the device once.  Its layout is private.  ACX_ERR_ARG: what acx_head_fit_step refuses in hp
 * and lr, rows outside 0 .. rows_max, a negative offset, jobs that differ in amsgrad / decoupled, a plan buffer too small.
 * acx_head_fit_group_step / _step_ce: step `step` (0 .. n_steps - 1) of the plan at DEVICE pointer `plan`; status: `jobs`
 * int32 words (ACX_FIT_BAD_INDEX / ACX_FIT_BAD_LABEL, ORed into the offending job's word only).  Workspace:
 * acx_head_fit_group_workspace_bytes(jobs, rows_max, classes, loss) (host only).  The launch contract of acx_head_fit_step: in
 * order on `stream`, no copy, no allocation, no synchronisation, capturable (a captured step replays that step of the plan);
 * argument errors return before any launch. */
#define ACX_FIT_MAX_JOBS 256
enum acx_fit_loss { ACX_FIT_LOSS_BCE = 0, ACX_FIT_LOSS_CE = 1 };
typedef struct acx_fit_job {
    const int64_t* idx;
    float *W, *b, *mW, *vW, *vmaxW, *mb, *vb, *vmaxb;
    float* loss;
} acx_fit_job;
ACX_API int acx_head_fit_group_workspace_bytes(int jobs, int64_t rows_max, int classes, int loss, size_t* out_bytes);
ACX_API int acx_head_fit_plan_bytes(int jobs, int64_t n_steps, size_t* out_bytes);
ACX_API int acx_head_fit_plan_fill(int jobs, int64_t n_steps, int64_t rows_max, int classes, int loss, const int32_t* rows,
                                   const int64_t* idx_offset, const acx_adam* hp, const double* lr, void* plan, size_t plan_bytes);
ACX_API int acx_head_fit_group_step(const float* E, int64_t ld_e, int64_t n_rows_total, const void* target, int target_dtype,
                                    int64_t ld_target, int jobs, int64_t rows_max, int classes, const acx_fit_job* job_table,
                                    const void* plan, int64_t n_steps, int64_t step, int32_t* status, void* ws, size_t ws_bytes,
                                    void* stream);
ACX_API int acx_head_fit_group_step_ce(const float* E, int64_t ld_e, int64_t n_rows_total, const int64_t* labels, int jobs,
                                       int64_t rows_max, int classes, double label_smoothing, const acx_fit_job* job_table,
                                       const void* plan, int64_t n_steps, int64_t step, int32_t* status, void* ws,
                                       size_t ws_bytes, void* stream);

/* ---- reading and judging a single-label head: softmax top-k, accuracy, confusion matrix ---------------------------------------
 * Stateless, no workspace; logits (rows, classes) fp32 on the device with row stride ld >= classes.  Both calls clear *status
 * (4 bytes) on `stream` first, then run one kernel; capturable.
 *   acx_softmax_topk: probs[r][c] = expf(z_c - m) / s with m and s as above (probs may be NULL; row stride ld_p), and the k
 *     best classes of each row ordered by logit descending, then class index ascending, -0.0 equal to +0.0 (the order of
 *     acx_knn_search) -- decided on the logits, so exact.  top_prob[r][j] has the bits of probs[r][top_index[r][j]].  A row
 *     holding a NaN or an infinity gets NaN probabilities and -1 indices and sets ACX_CLASSIFY_NONFINITE.  A row's outputs do
 *     not depend on rows, its position or ld.  1 <= k <= min(classes, ACX_CLASSIFY_MAX_K), else ACX_ERR_ARG.
 *   acx_classification_counts: over n rows with int64 labels: per_class[c] = {support, predicted, correct}, hits = {top-1,
 *     top-k}, confusion[true][predicted] (may be NULL).  The prediction is the first index of the row maximum; the rank of the
 *     true class y is #{c : z_c > z_y, or z_c = z_y and c < y}; a top-k hit is rank < k.  The outputs are cleared on `stream`
 *     first and counted with integer atomics: the same counts in any order.  A row with a non-finite logit or a label outside
 *     [0, classes) is counted nowhere and flagged.  confusion != NULL with classes > 4096 is ACX_ERR_UNSUPPORTED.
 * ARGUMENT errors (before any launch, acx_last_error naming the argument): a null pointer, rows / n < 1, classes outside
 * 1 .. ACX_MAX_CLASSES, ld < classes, ld_p < classes, k out of range; rows / n > 2^30 is ACX_ERR_UNSUPPORTED. */
#define ACX_CLASSIFY_MAX_K 64
#define ACX_CLASSIFY_NONFINITE 1
#define ACX_CLASSIFY_BAD_LABEL 2
ACX_API int acx_softmax_topk(const float* logits, int64_t ld, int64_t rows, int classes, int k, float* probs, int64_t ld_p,
                             int32_t* top_index, float* top_prob, int32_t* status, void* stream);
ACX_API int acx_classification_counts(const float* logits, int64_t ld, const int64_t* labels, int64_t n, int classes, int k,
                                      int64_t* per_class, int64_t* hits, int64_t* confusion, int32_t* status, void* stream);

/* ---- calibration: reliability (ECE / MCE / Brier), per-class Platt scaling, temperature scaling ---------------------------------
 * What the probabilities of a head mean, measured and repaired on the device.  Stateless: no context, the caller owns every
 * buffer (all on the device), everything runs on `stream`, nothing allocates or synchronises; capturable.  Each call clears
 * *status (4 bytes) on `stream` first and writes every element of its outputs.  The definitions are the float64 numpy
 * functions of pytorch/calibration.py (reliability_host, reliability_toplabel_host, fit_platt_host, fit_temperature_host,
 * platt_apply_host): Platt 1999 with the Newton / backtracking solver of Lin, Lin & Weng 2007; temperature scaling and ECE as
 * in Guo et al. 2017.  With a non-zero status the outputs are not to be read.
 *   bin of a probability p with `bins` bins (1 .. ACX_CAL_MAX_BINS): min(bins - 1, (int)(p * (float)bins)), the product in
 *     float32: p = 1 falls into the last bin, an edge k / bins belongs to bin k.
 *   acx_reliability_counts: probs (n, classes) fp32 with row stride ld against targets as acx_threshold_counts takes them.
 *     count / positive [classes][bins] int64: rows per bin and the positives among them (exact); conf_sum [classes][bins]
 *     double: the sum of p per bin; brier_sum [classes] double: the sum of (p - y)^2.  The float64 sums have ONE order: a
 *     (class, bin) sum runs over ascending rows, brier_sum adds the bins' partials by a fixed tree -- the same call gives the
 *     same bits.  p outside [0, 1] sets ACX_CAL_BAD_PROBABILITY, a NaN or infinity ACX_CAL_NONFINITE, a target other than 0 / 1
 *     ACX_CAL_BAD_TARGET.
 *   acx_reliability_toplabel: logits (n, classes) fp32, int64 labels, *beta a DEVICE double (NULL: 1).  The scaled logit is
 *     (float)beta * z (one rounding); the confidence is the top-1 softmax probability of the scaled row with the bits of
 *     acx_softmax_topk's top_prob[:, 0] on the scaled logits; the prediction is the first index of the row maximum.  count /
 *     correct [bins] int64, conf_sum [bins] double, nll_sum [1] double = sum of log s + (m - z_y) over the counted rows, in one
 *     fixed order.  A row holding a NaN or an infinity, or a label outside [0, classes), is counted nowhere and sets
 *     ACX_CAL_NONFINITE / ACX_CAL_BAD_LABEL.  workspace: acx_temperature_workspace_bytes(n, classes) bytes.
 *   acx_platt_fit: per class c the minimiser (a, b) of F = - sum_i [t_i log p_i + (1 - t_i) log(1 - p_i)], p_i = sigmoid(a z_ic +
 *     b); smooth != 0: Platt's targets t+ = (P + 1) / (P + 2), t- = 1 / (Nn + 2), else t = y.  ab [classes][2] double; info
 *     [classes] int32: the Newton iterations used, ACX_CAL_DEGENERATE (no positive, no negative or a constant column: the
 *     identity a = 1, b = 0 is returned) or ACX_CAL_NOT_CONVERGED (100 iterations; e.g. smooth = 0 on a separable class).  One
 *     launch fits all classes, the whole iteration on the device.  Status bits as acx_reliability_counts.
 *   acx_platt_apply: probs[r][c] = sigmoid_f32(fmaf((float)a_c, z, (float)b_c)) with the forward's sigmoid: a = 1, b = 0 gives
 *     the bits of clipwise_output.  rows x classes, row strides ld / ld_p.
 *   acx_temperature_fit: the minimiser over beta = 1 / T in [1e-4, 1e4] of F = sum_i [logsumexp_c(beta z_ic) - beta z_i,y_i],
 *     Newton with step halving from beta = 1.  The call queues `evaluations` (1 .. ACX_CAL_MAX_EVALUATIONS) launches, one pass
 *     over the logits each; the decision stays in device memory and launches after the stop return at once.  beta [1] double
 *     and info [1] int32 ON THE DEVICE: info = the evaluations used, ACX_CAL_DEGENERATE (every row constant: beta = 1),
 *     ACX_CAL_NOT_CONVERGED (evaluations used up; beta = the last accepted value) or ACX_CAL_AT_BOUND (the iteration stopped
 *     against 1e-4 or 1e4).  Rows flagged as in acx_reliability_toplabel enter no sum.
 *   acx_temperature_apply: out[r][c] = (float)beta * z (the input of acx_softmax_topk); row strides ld / ld_o.
 * ARGUMENT errors (before any launch): a null pointer, n / rows < 1, classes outside 1 .. ACX_MAX_CLASSES, a row stride shorter
 * than its row, bins or evaluations out of range, a bad target_dtype; n > 2^30 is ACX_ERR_UNSUPPORTED; a workspace too small
 * or not 256-byte aligned is ACX_ERR_WORKSPACE. */
#define ACX_CAL_MAX_BINS 64
#define ACX_CAL_MAX_EVALUATIONS 64
#define ACX_CAL_NONFINITE 1
#define ACX_CAL_BAD_TARGET 2
#define ACX_CAL_BAD_PROBABILITY 4
#define ACX_CAL_BAD_LABEL 8
#define ACX_CAL_DEGENERATE (-1)
#define ACX_CAL_NOT_CONVERGED (-2)
#define ACX_CAL_AT_BOUND (-3)
ACX_API int acx_reliability_counts(const float* probs, int64_t ld, const void* target, int target_dtype, int64_t ld_t, int64_t n,
                                   int classes, int bins, int64_t* count, int64_t* positive, double* conf_sum, double* brier_sum,
                                   int32_t* status, void* stream);
ACX_API int acx_reliability_toplabel(const float* logits, int64_t ld, const int64_t* labels, int64_t n, int classes,
                                     const double* beta, int bins, int64_t* count, int64_t* correct, double* conf_sum,
                                     double* nll_sum, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
ACX_API int acx_platt_workspace_bytes(int64_t n, int classes, size_t* out_bytes);                              /* host only */
ACX_API int acx_platt_fit(const float* logits, int64_t ld, const void* target, int target_dtype, int64_t ld_t, int64_t n,
                          int classes, int smooth, double* ab, int32_t* info, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);
ACX_API int acx_platt_apply(const float* logits, int64_t ld, int64_t rows, int classes, const double* ab, float* probs,
                            int64_t ld_p, void* stream);
ACX_API int acx_temperature_workspace_bytes(int64_t n, int classes, size_t* out_bytes);                        /* host only */
ACX_API int acx_temperature_fit(const float* logits, int64_t ld, const int64_t* labels, int64_t n, int classes, int evaluations,
                                double* beta, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes,
                                void* stream);
ACX_API int acx_temperature_apply(const float* logits, int64_t ld, int64_t rows, int classes, const double* beta, float* out,
                                  int64_t ld_o, void* stream);

/* ---- nearest-neighbour search over embeddings: top-k by dot product or cosine, and kNN tagging ----------------------------------
 * The reference's checkpoint is "for audio tagging and embedding extraction"; this is what the embeddings are extracted for:
 * query by example, and the kNN probe of a frozen representation.  Stateless: the caller owns every buffer (all on the device).
 *   q (nq, dim) and d (n, dim) fp32 with row strides ld_q / ld_d (16-byte aligned, strides multiples of 4; column slices of
 *   wider rows are read in place); dim a multiple of 4 in 4 .. ACX_KNN_MAX_DIM (pad with zero columns: neither dots nor norms
 *   change); 1 <= k <= ACX_KNN_MAX_K.
 * Score of (query i, row j): the fp32 dot product over dim (f32 matrix instructions, one fixed order per pair); for
 * ACX_KNN_COSINE it is then (dot * q_inv_norm[i]) * d_inv_norm[j], with inv_norm = 1 / sqrt(sum x^2) from acx_knn_row_norms
 * (0 for a zero row: every cosine with it is 0, never NaN).  A pair's score has the SAME BITS however it is reached: any nq, n,
 * k, number of slices, position of the query or the row, a sub-range of the database.
 * ONE TOTAL ORDER: neighbours are ordered by score descending, then database index ascending; -0.0 counts as +0.0.  Row t of
 * `indices` (nq, k) int32 / `scores` (nq, k) fp32 holds the first k of that order over the computed fp32 scores, best first.
 * exclude: NULL or device int32[nq], per query one database index that is never returned (-1: none); a self-search passes 0, 1,
 * ..., n - 1.
 *   acx_knn_row_norms: inv_norm[i] for n rows; ORs ACX_KNN_NONFINITE into *status if a row holds a NaN or +-inf (never clears).
 *   acx_knn_workspace_bytes: workspace of a search, non-decreasing in nq, n and k (host only).
 *   acx_knn_slices: into how many slices of the database rows a search of this shape is cut, so that a small nq still fills
 *     the device (host only; a function of the three sizes and ACX_KNN_SLICE_ROWS alone).
 *   acx_knn_search: a 4-byte clear of *status, the search kernel over (query tiles) x (slices), which keeps a running top k per
 *     query on chip and never writes the (nq, n) score matrix, and the merge of the slices' lists.  DATA errors go through
 *     *status: ACX_KNN_NONFINITE for a NaN or +-inf in q or d (or a dot product that overflows); every index is then -1 and
 *     every score NaN.  0 when the data is valid.
 *   acx_knn_vote: out[q][c] = sum_j w_j y[indices[q][j]][c] / sum_j w_j over the k neighbours, y = target (n, classes) of
 *     target_dtype with row stride ld_target, out (nq, classes) fp32 with row stride ld_out.  ACX_KNN_UNIFORM: w_j = 1; with
 *     ACX_TARGET_U8 the count is an integer and the result exactly float(count) / float(k).  ACX_KNN_SIMILARITY: w_j =
 *     exp((s_j - s_0) / temperature) in fp32, s = scores, sums in neighbour order j = 0 .. k - 1.  Clears *status, then ORs
 *     ACX_KNN_BAD_INDEX for an index outside [0, n): that neighbour contributes nothing (nothing outside target is read).
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable; the same
 * inputs give the same bits on every call whatever the workspace holds.  No global atomics except on *status.  ARGUMENT errors
 * return a negative status before any launch: a null pointer (q_inv_norm / d_inv_norm may be NULL for ACX_KNN_DOT, scores for
 * ACX_KNN_UNIFORM), nq < 1, n < 1, k < 1, k > ACX_KNN_MAX_K, k > n (k > n - 1 with exclude), dim not a multiple of 4 or outside
 * 4 .. ACX_KNN_MAX_DIM, a row stride shorter than its row or not a multiple of 4, an unaligned pointer, temperature <= 0, a
 * workspace too small or not 256-byte aligned (ACX_ERR_WORKSPACE); n > 2^30 is ACX_ERR_UNSUPPORTED.  acx_set_precision has no
 * influence; the kernels use no 16-bit matrix instruction and may run beside a forward on another stream. */
enum acx_knn_metric { ACX_KNN_DOT = 0, ACX_KNN_COSINE = 1 };
enum acx_knn_weighting { ACX_KNN_UNIFORM = 0, ACX_KNN_SIMILARITY = 1 };
#define ACX_KNN_MAX_K 128      /* candidate buffers of 2 k keys for 64 queries: 128 KiB of the CU's 160 KiB of LDS */
#define ACX_KNN_MAX_DIM 4096
#define ACX_KNN_NONFINITE 1
#define ACX_KNN_BAD_INDEX 2
ACX_API int acx_knn_row_norms(const float* x, int64_t ld, int64_t n, int dim, float* inv_norm, int32_t* status, void* stream);
ACX_API int acx_knn_workspace_bytes(int64_t nq, int64_t n, int k, size_t* out_bytes);
ACX_API int acx_knn_slices(int64_t nq, int64_t n, int k, int* out_slices);
ACX_API int acx_knn_search(const float* q, int64_t ld_q, const float* q_inv_norm, int64_t nq, const float* d, int64_t ld_d,
                           const float* d_inv_norm, int64_t n, int dim, int metric, int k, const int32_t* exclude,
                           int32_t* indices, float* scores, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_knn_vote(const int32_t* indices, const float* scores, int64_t nq, int k, const void* target, int target_dtype,
                         int64_t ld_target, int64_t n, int classes, int weighting, float temperature, float* out,
                         int64_t ld_out, int32_t* status, void* stream);

/* ---- int8 embedding index: coarse search on int8 codes (i8 matrix instructions), exact fp32 rerank -----------------------------
 * The two-stage design of a retrieval library over the search above (no reference counterpart, as for the search itself): a
 * coarse search on per-row symmetric int8 codes, 1 byte per column instead of 4, then the exact fp32 scores of a short candidate
 * list.  Stateless; every buffer is the caller's, on the device.
 *   acx_knn_quantize_i8: per row i of x (n, dim) fp32 (the layout rules of acx_knn_search), all in fp32 and each operation
 *     rounded on its own: y = x * inv_norm[i] (inv_norm NULL, the dot metric: y = x), amax = max |y|, g = 127.0f / amax,
 *     code = (int8) clamp(rintf(y * g), -127, 127) (round half to even), scale[i] = amax / 127.0f.  A zero row gives zero
 *     codes and scale 0.  A row with a NaN or +-inf among its y gives zero codes and scale NaN and ORs ACX_KNN_NONFINITE into
 *     *status (never clears).  codes (n, ld_c) int8, 16-byte aligned, ld_c a multiple of 16 and >= dim rounded up to
 *     ACX_KNN_I8_K; the columns from dim up to that multiple are written as zeros.
 *   acx_knn_search_i8: cq (nq, dim) / cd (n, dim) int8 codes with row strides ld_cq / ld_cd (16-byte aligned, multiples of 16,
 *     >= dim) and their scales sq / sd; dim is the PADDED code width, a multiple of ACX_KNN_I8_K in ACX_KNN_I8_K ..
 *     ACX_KNN_MAX_DIM.  t = sum_c cq[i][c] cd[j][c] is exact in int32 (|t| <= 4096 * 127^2 = 66 064 384), and the score is
 *     ((float)t * sq[i]) * sd[j]: one int -> float conversion (round to nearest even) and two rounded products.  Order,
 *     exclude, output shapes, workspace (acx_knn_workspace_bytes), slicing (acx_knn_slices, ACX_KNN_SLICE_ROWS) and launch
 *     sequence (4-byte clear of *status, search kernel, merge) are acx_knn_search's; where ws_bytes leaves room behind the
 *     slices' lists (nq * slices * k keys), a search of 16 or more slices merges them in two levels -- the result is the same.  A NaN or infinite scale sets
 *     ACX_KNN_NONFINITE: every index is then -1 and every score NaN.  The search kernel runs dense i8 matrix instructions and
 *     is launched as workgroups that hold a whole compute unit, like the 16-bit kernels of a forward.
 *   acx_knn_rescore: for each query the exact fp32 scores of its kc <= ACX_KNN_MAX_K candidate rows cand (nq, kc) int32 with row
 *     stride ld_cand, with the SAME BITS acx_knn_search gives that (query, row) pair, and the first k <= kc of the one total
 *     order into indices (nq, k) / scores (nq, k).  A candidate -1 is skipped; an index outside [0, n) is skipped and sets
 *     ACX_KNN_BAD_INDEX; outputs beyond the valid candidates are -1 / NaN.  A non-finite exact dot product sets
 *     ACX_KNN_NONFINITE and makes that query's row -1 / NaN.  A row listed twice is returned twice.  Clears *status first.
 *     No workspace.
 * acx_forward's launch contract, as above.  ARGUMENT errors return a negative status before any launch: a null pointer
 * (inv_norm may be NULL; the inverse norms of acx_knn_rescore for ACX_KNN_DOT), a size < 1, k or kc > ACX_KNN_MAX_K, k > kc,
 * k > n (n - 1 with exclude), a code width that is no multiple of ACX_KNN_I8_K or outside its range, a code stride that is no
 * multiple of 16 or too short, ld_cand < kc, an unaligned pointer, the fp32 layout errors and workspace errors of acx_knn_search;
 * n > 2^30 is ACX_ERR_UNSUPPORTED. */
#define ACX_KNN_I8_K 32        /* contraction width of one i8 matrix instruction: code rows are padded to a multiple */
ACX_API int acx_knn_quantize_i8(const float* x, int64_t ld, const float* inv_norm, int64_t n, int dim, int8_t* codes, int64_t ld_c,
                                float* scale, int32_t* status, void* stream);
ACX_API int acx_knn_search_i8(const int8_t* cq, int64_t ld_cq, const float* sq, int64_t nq, const int8_t* cd, int64_t ld_cd,
                              const float* sd, int64_t n, int dim, int k, const int32_t* exclude, int32_t* indices, float* scores,
                              int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_knn_rescore(const float* q, int64_t ld_q, const float* q_inv_norm, int64_t nq, const float* d, int64_t ld_d,
                            const float* d_inv_norm, int64_t n, int dim, int metric, const int32_t* cand, int64_t ld_cand, int kc,
                            int k, int32_t* indices, float* scores, int32_t* status, void* stream);

/* ---- k-means over embeddings: Lloyd iterations with k-means++ seeding, all decisions on the device --------------------------------
 * Clustering for embeddings without labels (no reference counterpart).  Stateless; every buffer is the caller's, on the device.
 *   x (n, dim) and centers (clusters, dim) fp32 with row strides ld_x / ld_c, the layout rules of acx_knn_search: 16-byte
 *   aligned, strides multiples of 4, dim a multiple of 4 in 4 .. ACX_KNN_MAX_DIM (pad with zero columns);
 *   1 <= clusters <= ACX_KMEANS_MAX_CLUSTERS, n <= 2^30, and clusters <= n for acx_kmeans_fit / acx_kmeans_seed.
 * SCORE of (row i, centre k): fma(-2, dot(x_i, c_k), cc_k) in fp32 -- the squared distance less the row's own sum x_i^2, which
 * cannot change the arg-min -- with the dot product on the f32 matrix instructions in ONE fixed order per pair (that of
 * acx_knn_search) and cc_k = sum c_k^2 in one fixed order.  ACX_KMEANS_COSINE: -dot(x_i, c_k) with the RAW row (its positive
 * inverse norm cannot change the arg-min either); the centres are unit rows.  A pair's score has the SAME BITS whatever n,
 * clusters or the position of the row or the centre.  ONE TOTAL ORDER: the label of a row is the first centre by score
 * ascending, then centre index ascending, -0.0 counting as +0.0.  The (n, clusters) scores are never written.
 *   acx_kmeans_assign: clears *status and *changed; labels[i] int32, scores[i] = the winner's score, *changed = rows whose label
 *     differs from prev_labels[i] (prev_labels NULL: n; it may alias labels).  A row with a non-finite winner score (a NaN or
 *     +-inf in x or centers, or an overflow) gets label -1 and sets ACX_KMEANS_NONFINITE.
 *   acx_kmeans_update: one mean step from given labels.  The row indices are partitioned STABLY by label, each (cluster, column)
 *     is summed in float64 in an order that depends on (n, dim, labels) alone, and c_k = (float)(sum / count).  COSINE: the rows
 *     are weighted by x_inv_norm (acx_knn_row_norms) and c_k = (float)(sum / |sum|), the norm in float64.  AN EMPTY CLUSTER KEEPS
 *     ITS CENTRE and reports count 0 (scikit-learn moves it to a far row instead).  counts (clusters) int32; *shift =
 *     sum_k |c_new - c_old|^2 in float64.  Labels outside [0, clusters) are left out and set ACX_KMEANS_BAD_LABEL.  No float
 *     atomics: the same inputs give the same bits on every call.
 *   acx_kmeans_fit: centers holds the initial centres and receives the final ones.  max_iter iterations (assign, update,
 *     decide) are QUEUED; after each the device sets state->done when no label changed or shift <= *tol_abs (a float64 on the
 *     device), and every kernel of a later iteration returns at once.  One closing assignment runs only if the last update moved a
 *     centre, so labels, counts and state->inertia always belong to the returned centres.  inertia = sum_i max(sum x_i^2 +
 *     score_i, 0) in float64 in a fixed order (COSINE: sum_i 1 + score_i x_inv_norm[i]).  state->iterations counts the
 *     iterations that ran, state->changed / shift are those of the last one.  ACX_KMEANS_NONFINITE stops the fit and leaves every
 *     label -1.
 *   k-means++ (D^2 sampling):
 *   acx_kmeans_min_distance: d[i] <- min(d[i], dist(x_i, center)) (first != 0: d[i] <- dist), dist = sum (x - c)^2 in fp32 by one
 *     wave per row in a fixed order, COSINE: max(0, 2 - 2 cos) with cos = (dot * x_inv_norm[i]) / |center|; *d_max = max_i d[i].
 *   acx_kmeans_sample: integer weights q_i = floor(d_i 2^(30 - e)), e = floor(log2 *d_max), summed exactly in uint64;
 *     *picked = the smallest i whose inclusive prefix sum exceeds t = min(floor(*u total), total - 1), the product one rounded
 *     float64 multiply.  Integer arithmetic after the quantisation: the pick does not depend on any order of summation.
 *     total == 0: *picked = -1 and ACX_KMEANS_DEGENERATE.  ws: at least 8192 bytes.
 *   acx_kmeans_seed: picked[0] = floor(u[0] n); round r = 1 .. clusters - 1 runs min_distance against row picked[r - 1] and
 *     sample with u[r]; a round with total == 0 (fewer distinct rows than clusters) takes the lowest row index not yet picked and
 *     sets ACX_KMEANS_DEGENERATE.  centers[k] = row picked[k] (COSINE: times its inverse norm).  u: clusters doubles in [0, 1).
 *   acx_kmeans_workspace_bytes: the workspace of fit, update and seed; non-decreasing in each argument (host only).
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable.  ARGUMENT errors
 * return a negative status before any launch, as for acx_knn_search. */
enum acx_kmeans_metric { ACX_KMEANS_EUCLIDEAN = 0, ACX_KMEANS_COSINE = 1 };
#define ACX_KMEANS_MAX_CLUSTERS 4096
#define ACX_KMEANS_MAX_ITER 1000
#define ACX_KMEANS_NONFINITE 1
#define ACX_KMEANS_DEGENERATE 2
#define ACX_KMEANS_BAD_LABEL 4
typedef struct acx_kmeans_state {
    int32_t iterations, done, changed, reserved;
    double shift, inertia;
} acx_kmeans_state;
ACX_API int acx_kmeans_workspace_bytes(int64_t n, int dim, int clusters, size_t* out_bytes);
ACX_API int acx_kmeans_assign(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, const float* centers, int64_t ld_c,
                              int clusters, int dim, int metric, const int32_t* prev_labels, int32_t* labels, float* scores,
                              int32_t* changed, int32_t* status, void* stream);
ACX_API int acx_kmeans_update(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric,
                              const int32_t* labels, int clusters, float* centers, int64_t ld_c, int32_t* counts, double* shift,
                              int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_kmeans_fit(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric, float* centers,
                           int64_t ld_c, int clusters, int max_iter, const double* tol_abs, int32_t* labels, int32_t* counts,
                           acx_kmeans_state* state, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_kmeans_min_distance(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric,
                                    const float* center, int first, float* d, float* d_max, int32_t* status, void* stream);
ACX_API int acx_kmeans_sample(const float* d, int64_t n, const float* d_max, const double* u, int32_t* picked, int32_t* status,
                              void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_kmeans_seed(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric, int clusters,
                            const double* u, int32_t* picked, float* centers, int64_t ld_c, int32_t* status, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- Gaussian mixtures over embeddings: EM with diagonal or spherical covariances, all decisions on the device ---------------------
 * A density model with more than one mode (no reference counterpart; scikit-learn 1.7.2's GaussianMixture is the yardstick).
 * Stateless; every buffer is the caller's, on the device.
 *   x (n, dim) fp32 with row stride ld_x under the layout rules of acx_kmeans_assign: 16-byte aligned, strides multiples of 4, dim a
 *   multiple of 4 in 4 .. ACX_KNN_MAX_DIM; 1 <= components <= ACX_KMEANS_MAX_CLUSTERS, n <= 2^30.
 *   PARAMETERS, float64: weights (components), means (components, dim), variances (components, dim) for ACX_GMM_DIAG or
 *   (components) for ACX_GMM_SPHERICAL, all contiguous.  center (dim) float64 is subtracted from rows and means before anything is
 *   rounded to fp32 (NULL: zeros); a fit uses the column means.
 * LOG-DENSITY of (row i, component k): with xc = x_i - center, mc = mean_k - center, a = 1 / v_k, b = mc / v_k,
 *     lp = fp32(cst_k - D / 2),  D = sum_d [fp32(xc^2) fp32(a) + fp32(xc) fp32(-2 b)] in fp32,
 *     cst_k = log w_k - (dim log 2 pi + sum log v + sum mc^2 a) / 2 in float64 (its sums in one fixed order; kept in float64
 *     because its fp32 rounding would move every row of a component the same way), the last step one float64 fused multiply-add
 *     and one rounding.  ACX_GMM_SPHERICAL takes the one variance of a component out of the sum for the same reason:
 *     lp = fp32(cst_k - D / (2 v_k)) with D = sum_d [fp32(xc^2) + fp32(xc) fp32(-2 mc)] and v_k in float64;
 *   the 2 dim long contraction on the f32 matrix instructions in ONE fixed order per pair (that of acx_knn_search over rows of
 *   2 dim columns: the squares first).  A pair's log-density has the SAME BITS whatever n, components or the position of the row
 *   or the component, and a row's outputs are a function of that row, center and the parameters alone.  The (n, components)
 *   log-densities are never written.
 *   acx_gmm_estep: clears *status.  With m_i = max_k lp and s_i = sum_k expf(lp - m_i) (fp32, an order that depends on components
 *     alone): log_prob_norm[i] = m_i + logf(s_i) (never -0.0); resp[i * ld_resp + k] = expf(lp - m_i) / s_i (resp may be NULL);
 *     labels[i] int32 (may be NULL) = the first component by log-density descending, then index ascending, -0.0 counting as +0.0;
 *     *log_prob_sum = sum_i ((double)m_i + log((double)s_i)) in float64 in one fixed order: log_prob_norm before its rounding to
 *     fp32 (a row whose log s_i is below half an ulp of m_i loses it in fp32 every time, which would bias the mean).  A
 *     non-finite log-density (a NaN or +-inf in x, a zero weight or variance, an overflow) sets ACX_GMM_NONFINITE; a row whose
 *     maximum is non-finite gets label -1.
 *   acx_gmm_score: acx_gmm_estep without resp.
 *   acx_gmm_mstep: clears *status.  scikit-learn's M-step from resp (n, components) fp32: N_k = sum_i r_ik + 10 * 2^-52, mean_k =
 *     sum r xc / N_k + center, v_kd = sum r xc^2 / N_k - (sum r xc / N_k)^2 + reg_covar (SPHERICAL: the mean of v_kd over d),
 *     w_k = N_k / n; nk (components) float64 = N_k.  The sums are float64, in an order that depends on (n, dim, components)
 *     alone.  No float atomics: the same inputs give the same bits on every call.  N_k < 1 sets ACX_GMM_DEGENERATE; the
 *     component's parameters are still the formula's.
 *   acx_gmm_fit: the parameters hold the initial values and receive the result.  center (dim) <- the float64 column means of x in
 *     a fixed order; the rows are centred ONCE into the workspace.  max_iter iterations (E-step, M-step, decide) are QUEUED;
 *     after each the device writes *state: lower_bound = *log_prob_sum / n of the iteration's E-step, change = lower_bound
 *     less the previous one (+inf in iteration 1), and sets done and converged when |change| < *tol (a float64 on the device);
 *     every kernel of a later iteration returns at once.  ACX_GMM_NONFINITE stops the fit before the M-step.  One closing E-step
 *     runs only if the last M-step ran, so labels (n) and log_prob_norm (n) belong to the returned parameters.
 *     ACX_GMM_DEGENERATE may come from any iteration.
 *   acx_gmm_workspace_bytes: the workspace of every call above; non-decreasing in each argument (host only).
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable.  ARGUMENT errors
 * return a negative status before any launch, as for acx_kmeans_assign; max_iter in 1 .. ACX_KMEANS_MAX_ITER. */
enum acx_gmm_covariance { ACX_GMM_DIAG = 0, ACX_GMM_SPHERICAL = 1 };
#define ACX_GMM_NONFINITE 1
#define ACX_GMM_DEGENERATE 2
typedef struct acx_gmm_state {
    int32_t iterations, done, converged, reserved;
    double lower_bound, change;
} acx_gmm_state;
ACX_API int acx_gmm_workspace_bytes(int64_t n, int dim, int components, size_t* out_bytes);
ACX_API int acx_gmm_estep(const float* x, int64_t ld_x, int64_t n, int dim, const double* center, const double* weights,
                          const double* means, const double* variances, int components, int covariance_type, float* log_prob_norm,
                          float* resp, int64_t ld_resp, int32_t* labels, double* log_prob_sum, int32_t* status, void* ws,
                          size_t ws_bytes, void* stream);
ACX_API int acx_gmm_score(const float* x, int64_t ld_x, int64_t n, int dim, const double* center, const double* weights,
                          const double* means, const double* variances, int components, int covariance_type, float* log_prob_norm,
                          int32_t* labels, double* log_prob_sum, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_gmm_mstep(const float* x, int64_t ld_x, int64_t n, int dim, const double* center, const float* resp, int64_t ld_resp,
                          int components, double reg_covar, int covariance_type, double* weights, double* means, double* variances,
                          double* nk, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_gmm_fit(const float* x, int64_t ld_x, int64_t n, int dim, double* weights, double* means, double* variances,
                        int components, int covariance_type, int max_iter, const double* tol, double reg_covar, double* center,
                        int32_t* labels, float* log_prob_norm, acx_gmm_state* state, int32_t* status, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- cluster validation: silhouette, within-cluster dispersion, contingency tables ---------------------------------------------
 * What says whether a clustering is good and which k to take (no reference counterpart; scikit-learn 1.7.2's silhouette_samples,
 * calinski_harabasz_score, davies_bouldin_score and contingency-based scores are the yardsticks).  Stateless; every buffer is the
 * caller's, on the device.  x (n, dim) fp32 with row stride ld_x and x_inv_norm under the rules of acx_kmeans_assign; labels (n)
 * int32; 1 <= clusters <= ACX_KMEANS_MAX_CLUSTERS (clusters may exceed n), n <= 2^30; metric an acx_kmeans_metric.
 * THE PARTITION: the row indices sorted stably by label (acx_kmeans_update's): cluster c owns the partition positions
 * start_c .. start_c + count_c - 1, ascending row index inside it.  A label outside [0, clusters) puts its row in NO cluster and
 * sets ACX_CLUSTER_BAD_LABEL.  Every float64 sum below runs over partition positions in a stated order: no float atomics, the same
 * inputs give the same bits on every call.
 *   acx_silhouette: PAIR DISTANCE in fp32.  EUCLIDEAN: d(i, j) = sqrt(max(fma(-2, dot_ij, xx_i + xx_j), 0)), the square root
 *     correctly rounded, dot_ij the dot product of acx_knn_search / acx_kmeans_assign (one fixed order per pair) and xx_i = sum
 *     x_i^2 in one fixed order per row.  COSINE: d = 1 - (dot_ij * rx_i) * rx_j with rx = x_inv_norm (rx = 0: d = 1).  The pair
 *     (i, i) contributes exactly 0: it is left out by position, not by value.
 *     For the queried rows -- rows (n_rows) int32 row indices, n_rows <= n, in any order, repeats allowed; NULL: every row in
 *     order, n_rows ignored -- with L the row's label:  S(i, c) = sum over the positions of cluster c of (double)d(i, j);
 *     a = S(i, L) / (count_L - 1) (0 when count_L == 1);  b = min over the non-empty c != L of S(i, c) / count_c, the lowest c
 *     winning a tie, that c in nearest;  s = (b - a) / max(a, b), and s = 0 when count_L == 1 or max(a, b) == 0.  Empty clusters
 *     are skipped.  THE ORDER of S(i, c): the positions 0 .. n - 1 are cut into ranges of `len` positions, len = 64 ceil(ceil(n / 64)
 *     / ns) with ns = min(ACX_CLUSTER_MAX_SPLITS, ceil(n / 64), max(1, ceil(512 / ceil(n_rows / 256)))); inside a range the
 *     distances of cluster c are added one by one in ascending position into a float64 that starts at 0, and S(i, c) is the
 *     ranges' partial sums added in ascending range, starting from the first.  A function of (n, labels, n_rows) alone.
 *     *mean = the mean of s over the queried rows that have a cluster; cluster_mean[c] (NULL: not wanted) = the mean over the
 *     queried rows of label c, NaN when there are none.  Their order: with the queried rows numbered q = 0 .. n_rows - 1, partial t
 *     = rows q = t, t + 256, ... in ascending order (t = 0 .. 255), then partial[t] += partial[t + o] for o = 128, 64, .. 1, then
 *     one division by the count.
 *     *status (cleared first): ACX_CLUSTER_NONFINITE -- a NaN or an infinity (or an overflow) in a queried row or in a row of a
 *     cluster: the outputs of every row it reaches are NaN, nearest -1.  ACX_CLUSTER_BAD_LABEL -- some label is outside
 *     [0, clusters): a queried row with such a label gets NaN / -1 and stays out of *mean.  ACX_CLUSTER_BAD_ROW -- an entry of
 *     rows outside [0, n): the same.  ACX_CLUSTER_DEGENERATE -- fewer than two non-empty clusters: every s = 0, b = NaN,
 *     nearest = -1.  The (n, n) distances are never written; the workspace holds (clusters + ACX_CLUSTER_MAX_SPLITS) float64 per
 *     queried row.  a, b, s float64 (n_rows), nearest int32 (n_rows).
 *   acx_cluster_dispersion: what Calinski-Harabasz and Davies-Bouldin are made of.  counts (clusters) int64; means (clusters, dim)
 *     float64 = the cluster's float64 sums as acx_kmeans_update takes them (unweighted), divided by the count (an empty cluster: 0);
 *     per row v = sum_j ((double)x_j - mean_j)^2, every product and sum rounded: lane l = 0 .. 63 takes columns 4 l .. 4 l + 3,
 *     then + 256, ... in ascending order, the lanes join by the xor butterfly 32, 16, .. 1.  within_sq[c] = sum v, within_dist[c] =
 *     sum sqrt(v) over the cluster's rows: position j of the cluster goes to partial j mod 4, each partial in ascending j, joined
 *     as ((p0 + p1) + p2) + p3.  grand_mean (dim) = the clusters' sums added in ascending c, divided by the rows that have a
 *     cluster.  ACX_CLUSTER_NONFINITE, ACX_CLUSTER_BAD_LABEL as above; ACX_CLUSTER_DEGENERATE for fewer than two non-empty clusters
 *     (the outputs are written all the same).
 *   acx_contingency: table (ka, kb) int64, cleared on `stream`, table[a_i][b_i] += 1 by integer atomics.  A pair with either label
 *     out of range is counted nowhere and sets ACX_CLUSTER_BAD_LABEL.  ka * kb > ACX_CONTINGENCY_MAX_CELLS is ACX_ERR_UNSUPPORTED.
 *   acx_cluster_scores_workspace_bytes: the workspace of acx_silhouette and acx_cluster_dispersion; non-decreasing in each
 *     argument (host only).
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable.  ARGUMENT errors
 * return a negative status before any launch, as for acx_kmeans_assign; n_rows outside 1 .. n is ACX_ERR_ARG. */
#define ACX_CLUSTER_NONFINITE 1
#define ACX_CLUSTER_DEGENERATE 2
#define ACX_CLUSTER_BAD_LABEL 4
#define ACX_CLUSTER_BAD_ROW 8
#define ACX_CLUSTER_MAX_SPLITS 16
#define ACX_CONTINGENCY_MAX_CELLS (1 << 24)
ACX_API int acx_cluster_scores_workspace_bytes(int64_t n, int dim, int clusters, size_t* out_bytes);
ACX_API int acx_silhouette(const float* x, int64_t ld_x, const float* x_inv_norm, int64_t n, int dim, int metric,
                           const int32_t* labels, int clusters, const int32_t* rows, int64_t n_rows, double* a, double* b,
                           int32_t* nearest, double* s, double* cluster_mean, double* mean, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream);
ACX_API int acx_cluster_dispersion(const float* x, int64_t ld_x, int64_t n, int dim, const int32_t* labels, int clusters,
                                   int64_t* counts, double* means, double* within_sq, double* within_dist, double* grand_mean,
                                   int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_contingency(const int32_t* a, int ka, const int32_t* b, int kb, int64_t n, int64_t* table, int32_t* status,
                            void* stream);

/* ---- radius search, connected components, DBSCAN: which rows lie within a given distance of each other ---------------------------
 * Neighbour lists by a threshold instead of a k (no reference counterpart; scikit-learn 1.7.2's radius_neighbors and
 * DBSCAN(algorithm="brute") are the yardsticks).  Stateless; every buffer is the caller's, on the device.  q (nq, dim) and d (n, dim)
 * fp32 with row strides ld_q / ld_d under the layout rules of acx_knn_search; nq, n <= 2^30.
 * THE PAIR VALUE v(i, j) of query row i and database row j, in fp32:
 *   ACX_RADIUS_DOT, ACX_RADIUS_COSINE: acx_knn_search's score of that pair with the SAME BITS -- its dot product (one fixed order
 *     per pair, a function of dim alone), for COSINE then (dot * q_aux[i]) * d_aux[j] with aux = the inverse norms of
 *     acx_knn_row_norms.  The pair is kept iff v >= level.
 *   ACX_RADIUS_EUCLIDEAN: v = max(fma(-2, dot, q_aux[i] + d_aux[j]), 0) with aux = xx = sum x^2 in one fixed order per row
 *     (acx_radius_row_sumsq): the squared distance acx_silhouette forms before its square root.  The pair is kept iff v <= level;
 *     for a radius eps pass level = (float)(eps * eps), the product taken in double.
 *   A NaN is never kept.  A non-finite dot product of a pair sets ACX_RADIUS_NONFINITE.  aux is NULL (ignored) for ACX_RADIUS_DOT.
 * SELF-JOINS (self_mode != ACX_RADIUS_SELF_NONE; the queries are the database rows, nq == n): the pair (i, i) is decided by
 *   position, not by arithmetic: kept with ACX_RADIUS_SELF_INCLUDE, dropped with ACX_RADIUS_SELF_EXCLUDE.  DOT and EUCLIDEAN
 *   values are symmetric in their bits; COSINE is not ((dot * r_i) * r_j against (dot * r_j) * r_i), so everything built on a
 *   list treats an edge as UNDIRECTED: {i, j} is an edge iff (i -> j) or (j -> i) is listed.
 * THE LIST is CSR: offsets (nq + 1) int64, indices int32, values fp32 (NULL: not wanted); row i owns offsets[i] .. offsets[i + 1]
 *   - 1, in ASCENDING database index.  A pure function of the inputs: no atomically appended rows, the same bytes on every call
 *   and for every slicing.
 *   acx_radius_count: counts[i] int32 = the kept pairs of query i.  One fused kernel over (tiles of 256 queries) x (ranges of
 *     database rows): each 64 x 64 tile of dot products goes straight to keep bits; neither the (nq, n) values nor a mask are
 *     written.  The ranges: len = 64 ceil(ceil(n / 64) / ns) rows each, ns = min(slices, ACX_RADIUS_MAX_SLICES, ceil(n / 64)),
 *     slices = 0 standing for the ns in that span with the smallest ceil(ceil(nq / 256) ceil(n / len) / 256) len -- the rows the
 *     busiest of 256 compute units streams -- and the largest such ns among equals (acx_radius_slices returns the number of ranges).
 *   acx_radius_neighbors: the count pass per (query, range), an exclusive scan in (query, range) order that writes offsets and
 *     *total = offsets[nq], and the emit pass (the same kernel body).  total > capacity sets ACX_RADIUS_OVERFLOW: entries at
 *     positions >= capacity are not written (every store is guarded), offsets and *total stay valid, so the caller can size a
 *     second call.  capacity = 0 (indices may be NULL then) runs the count and the scan only.
 *   acx_radius_emit: the emit pass alone, with the arguments of an acx_radius_neighbors call that has run on the same workspace
 *     (its counts and their scan are read from there; offsets and *total are not written) and a capacity of its own: count with
 *     capacity 0, read *total, allocate, emit -- two tile passes in all.  The overflow bit is set or cleared against the new
 *     capacity; the other bits stay.
 *   acx_graph_components: labels[i] int32 = the smallest row index of i's connected component in the UNDIRECTED graph of a
 *     self-join list (n rows; offsets non-decreasing from 0, the caller's promise) -- unique, so every schedule gives the same
 *     bits.  Edge-parallel hooking by integer atomicMin plus pointer jumping, in rounds; max_rounds (1 .. ACX_GRAPH_MAX_ROUNDS)
 *     rounds are QUEUED, the stop is decided on the device and the launches after it return at once.  Labels not stable after
 *     max_rounds: ACX_GRAPH_NOT_CONVERGED; resume != 0 continues from the labels given (a forest with labels[i] <= i; any other
 *     entry restarts its node) instead of labels[i] = i.  An index outside [0, n) sets ACX_GRAPH_BAD_INDEX and that edge is
 *     skipped.  While the call is queued, bits 29 and 30 of *status are its own; its last kernel clears them.
 *   acx_dbscan_labels: DBSCAN from a self-join list made with ACX_RADIUS_SELF_INCLUDE.  core[i] = (offsets[i + 1] - offsets[i] >=
 *     min_samples); clusters = the components of the core-core edges, numbered 0, 1, .. in ascending order of their smallest core
 *     index; a row that is not core takes the SMALLEST cluster number among its core neighbours (undirected), -1 if it has none.
 *     These are scikit-learn's labels, border rows included (it expands cluster c completely before it starts c + 1).
 *     *clusters int32 = the number of clusters.  Status bits as acx_graph_components.
 *   acx_radius_row_sumsq: xx[i] = sum x_i^2 (fp32, one fixed order per row).
 *   acx_radius_workspace_bytes (acx_radius_count: slices = 0), acx_dbscan_workspace_bytes: host only, non-decreasing in nq / n.
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable; *status and
 * *total are cleared by a kernel of the call.  ARGUMENT errors return a negative status before any launch, as for acx_knn_search;
 * in addition ACX_ERR_ARG: a NaN level, a bad metric or self_mode, a self-join with nq != n, slices outside 0 ..
 * ACX_RADIUS_MAX_SLICES, capacity < 0, min_samples < 1, max_rounds outside 1 .. ACX_GRAPH_MAX_ROUNDS; nq or n > 2^30 is
 * ACX_ERR_UNSUPPORTED. */
enum acx_radius_metric { ACX_RADIUS_DOT = 0, ACX_RADIUS_COSINE = 1, ACX_RADIUS_EUCLIDEAN = 2 };
enum acx_radius_self { ACX_RADIUS_SELF_NONE = 0, ACX_RADIUS_SELF_EXCLUDE = 1, ACX_RADIUS_SELF_INCLUDE = 2 };
#define ACX_RADIUS_NONFINITE 1
#define ACX_RADIUS_OVERFLOW 2
#define ACX_GRAPH_BAD_INDEX 4
#define ACX_GRAPH_NOT_CONVERGED 8
#define ACX_RADIUS_MAX_SLICES 64
#define ACX_GRAPH_MAX_ROUNDS 4096
ACX_API int acx_radius_workspace_bytes(int64_t nq, int64_t n, int slices, size_t* out_bytes);
ACX_API int acx_radius_slices(int64_t nq, int64_t n, int slices, int* out_slices);
ACX_API int acx_radius_row_sumsq(const float* x, int64_t ld, int64_t n, int dim, float* xx, void* stream);
ACX_API int acx_radius_count(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d,
                             const float* d_aux, int64_t n, int dim, int metric, float level, int self_mode, int32_t* counts,
                             int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_radius_neighbors(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d,
                                 const float* d_aux, int64_t n, int dim, int metric, float level, int self_mode, int slices,
                                 int64_t* offsets, int32_t* indices, float* values, int64_t capacity, int64_t* total,
                                 int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_radius_emit(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d,
                            const float* d_aux, int64_t n, int dim, int metric, float level, int self_mode, int slices,
                            const int64_t* offsets, int32_t* indices, float* values, int64_t capacity, const int64_t* total,
                            int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_graph_components(const int64_t* offsets, const int32_t* indices, int64_t n, int32_t* labels, int32_t* status,
                                 int max_rounds, int resume, void* stream);
ACX_API int acx_dbscan_workspace_bytes(int64_t n, size_t* out_bytes);
ACX_API int acx_dbscan_labels(const int64_t* offsets, const int32_t* indices, int64_t n, int min_samples, int32_t* labels,
                              uint8_t* core, int32_t* clusters, int32_t* status, void* ws, size_t ws_bytes, int max_rounds,
                              void* stream);

/* ---- embedding statistics: float64 moments, Gram products, a symmetric eigensolver, PCA projection ------------------------------
 * Second-order statistics of a set of embeddings (no reference counterpart): what covariance, PCA / whitening, Mahalanobis
 * scores and the Frechet distance rest on.  Stateless; every buffer is the caller's, on the device.  1 <= dim <=
 * ACX_STATS_MAX_DIM; dim need NOT be a multiple of 4 and no pointer needs more than its element's alignment: tails are
 * predicated.  Row strides ld >= the row's width.  n <= 2^30 rows.
 *   acx_moments: x (n, dim) fp32 -> mean (dim) and cov (dim, dim) float64, ddof in {0, 1}.
 *     mean[j] = (sum_i (double)x[i][j]) / n: the n rows are cut into slices of R rows; inside a slice row i goes to partial
 *     i mod 4, each partial is summed in ascending i, the four are added as ((p0 + p1) + p2) + p3, the slices' sums are added
 *     in ascending slice order and the total is divided ONCE by n.
 *     cov[a][b] = (sum_i fl(x_ia - mean_a) fl(x_ib - mean_b)) / (n - ddof): the rows are centred ON LOAD in float64 (one
 *     rounded subtraction per element), the products and sums run on v_mfma_f64_16x16x4_f64, four rows per instruction in
 *     ascending row order inside a slice; the slices' partial tiles are summed in ascending slice order by a second pass and
 *     divided once.  Only the 64 x 64 tiles with b >= a are computed; the result is mirrored, so cov is exactly symmetric.
 *     No float atomics: the same input gives the same bits on every run.  R = ACX_MOMENTS_SLICE_ROWS (16 .. 2^30, rounded up
 *     to a multiple of 4; read at the first acx_create and by acx_tuning_refresh) or, without it, max(1024, ceil(n / 16))
 *     rounded up to a multiple of 4.  A NaN or infinite element sets ACX_STATS_NONFINITE (the outputs are written all the
 *     same, non-finite where the arithmetic makes them so); n - ddof == 0 sets ACX_STATS_DEGENERATE and writes a zero cov.
 *   acx_gram_f64: out (m, n) = A^T B for float64 A (rows, m) and B (rows, n), m, n <= ACX_STATS_MAX_DIM, on the same tile body:
 *     out[a][b] = sum_i A[i][a] B[i][b], four rows per instruction in ascending row order, ONE slice.  No workspace, no status.
 *   acx_eigh: a (dim, dim) float64 symmetric (the upper triangle is read) -> values (dim) descending (ties by the original
 *     column index) and vectors (dim, dim): ROW k is the k-th eigenvector, signed so that its entry of the largest magnitude
 *     (lowest index on ties) is positive.  Cyclic Jacobi with the round-robin ordering: with m = dim rounded up to even, a sweep
 *     is m - 1 rounds; in round r index m - 1 pairs with r and every other i with (2 r - i) mod (m - 1) (pairs with the padding
 *     index of an odd dim are idle).  A pair p < q is rotated where |a_pq| > 2^-53 max_i |a_ii| of the INPUT, by
 *     theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(1 + theta^2)), c = 1 / sqrt(1 + t^2), s = t c;
 *     a_pp <- a_pp - t a_pq, a_qq <- a_qq + t a_pq, a_pq <- 0, and every other new element from the four old ones
 *     A[{i, pi(i)}][{j, pi(j)}] (for i <= j, mirrored: the matrix stays exactly symmetric).  One launch per round reads one
 *     copy of the matrix (and of the accumulated vectors) and writes the other; every workgroup recomputes the rotations of
 *     its rows and columns from the old elements, so nothing inside a launch waits on another workgroup.  Each round adds the
 *     rotations it applied to a counter of its sweep; the first round of a sweep sets state->done when the sweep before applied
 *     none, and every later launch returns at once: max_sweeps (1 .. ACX_EIGH_MAX_SWEEPS) sweeps are QUEUED and the host reads
 *     nothing.  state->sweeps = sweeps that ran (the closing one that applied no rotation included), state->rotations = rotations
 *     applied.  ACX_STATS_NOT_CONVERGED when the last queued sweep still rotated; ACX_STATS_NONFINITE for a NaN or infinite
 *     input (nothing is rotated then).
 *   acx_pca_transform: out[i][c] = scale[c] * sum_j fl32(x[i][j] - mean[j]) W[c][j], x (n, dim), W (k, dim), mean (dim), scale (k)
 *     or NULL, all fp32, k <= dim, on the f32 matrix instructions (v_mfma_f32_32x32x2_f32).  The sum runs over groups of 16
 *     columns in ascending order; inside a group instruction e = 0 .. 7 adds columns e and 8 + e of the group, zeros past dim.
 *   acx_pca_inverse: out[i][j] = mean[j] + sum_c (z[i][c] * scale[c]) W[c][j], z (n, k); components in ascending pairs (2 e,
 *     2 e + 1), one instruction per pair, zero past k.  scale NULL: 1.
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable.  ARGUMENT errors
 * (a null pointer, a size < 1 or over its limit, ld too short, ddof outside {0, 1}, max_sweeps outside its range, an unaligned
 * state or float64 pointer, workspace errors) return a negative status before any launch; n > 2^30 is ACX_ERR_UNSUPPORTED.  The
 * data calls clear *status first. */
#define ACX_STATS_MAX_DIM 1024
#define ACX_EIGH_MAX_SWEEPS 64
#define ACX_STATS_NONFINITE 1
#define ACX_STATS_NOT_CONVERGED 2
#define ACX_STATS_DEGENERATE 4
typedef struct acx_eigh_state {
    int32_t sweeps, done;
    int64_t rotations;
} acx_eigh_state;
ACX_API int acx_moments_workspace_bytes(int64_t n, int dim, size_t* out_bytes);
ACX_API int acx_moments(const float* x, int64_t ld_x, int64_t n, int dim, int ddof, double* mean, double* cov, int64_t ld_c,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_gram_f64(const double* a, int64_t ld_a, const double* b, int64_t ld_b, int64_t rows, int m, int n, double* out,
                         int64_t ld_o, void* stream);
ACX_API int acx_eigh_workspace_bytes(int dim, size_t* out_bytes);
ACX_API int acx_eigh(const double* a, int64_t ld_a, int dim, int max_sweeps, double* values, double* vectors, int64_t ld_v,
                     acx_eigh_state* state, int32_t* status, void* ws, size_t ws_bytes, void* stream);
ACX_API int acx_pca_transform(const float* x, int64_t ld_x, int64_t n, int dim, const float* mean, const float* w, int64_t ld_w,
                              int k, const float* scale, float* out, int64_t ld_o, void* stream);
ACX_API int acx_pca_inverse(const float* z, int64_t ld_z, int64_t n, int k, const float* scale, const float* w, int64_t ld_w,
                            int dim, const float* mean, float* out, int64_t ld_o, void* stream);

/* ---- ranking metrics: the classes of one clip ranked against each other ------------------------------------------------------
 * What LRAP, lwlrap (DCASE 2019 Task 2), coverage error, label-ranking loss, one-error and precision / recall at k are made of
 * (no reference counterpart; sklearn 1.7.2's label_ranking_average_precision_score, coverage_error and label_ranking_loss are
 * the yardsticks): integer counts per (row, positive class).  For row i with scores s (classes) and a 0 / 1 target, and every
 * positive class j -- scores compared as float32 with -0.0 == +0.0, denormals in their own order:
 *   ge_j = #{c : s_c >= s_j}   pge_j = #{c positive : s_c >= s_j}   ord_j = #{c : s_c > s_j} + #{c < j : s_c == s_j}
 * (ge is the rank with ties at their worst, sklearn's rule; ord is the place in the total order score descending, then class
 * index ascending).  Per row: n_pos; psum = sum_j pge_j / ge_j, each quotient the correctly rounded float64 of the integer ratio,
 * added in ASCENDING j; coverage = max_j ge_j (0 without positives); bad_pairs = sum_j (ge_j - pge_j), the (positive, negative)
 * pairs not strictly ordered; hits_k = #{j : ord_j < k}.  Per class c: class_count[c] = rows in which c is positive, class_psum[c] =
 * the sum over those rows of pge / ge, added in ASCENDING row.  No float atomics: the same inputs give the same bits on every run.
 *   acx_ranking_metrics: scores (rows, classes) fp32 with row stride ld_s; target of target_dtype with row stride ld_t, as
 *     acx_tagging_metrics takes them, with its DATA errors: a NaN or infinite score sets ACX_METRICS_NONFINITE, a target other
 *     than 0 / 1 ACX_METRICS_BAD_TARGET in *status (cleared first); the outputs of such a row are unspecified, inside their
 *     buffers.  1 <= classes <= ACX_MAX_CLASSES, 1 <= rows <= 2^30, 1 <= k <= classes.  row_counts: (rows, 4) int64 = n_pos,
 *     coverage, bad_pairs, hits_k; row_psum (rows), class_count (classes), class_psum (classes).  The rows run in slices of
 *     slice_rows (0: the default, 2^26 / (8 classes) rows and at least 256; at most 2^22 slices): a row pass writes the slice's
 *     quotients to the workspace, 8 * classes bytes per slice row, and a column pass adds them onto class_psum / class_count; the
 *     slices follow each other on `stream`.  The results do not depend on slice_rows.  Up to 1 024 classes a wave ranks a row,
 *     four rows per workgroup; wider rows take a workgroup each.  The cost is O(n_pos * classes) per row: dense targets on very
 *     wide heads are quadratic.
 *   acx_ranking_workspace_bytes: 8 * classes * min(rows, slice rows), rounded up to 256 -- non-decreasing in slice_rows and
 *     independent of rows beyond one slice (host only).
 * acx_forward's launch contract: everything in order on `stream`, no allocation, no synchronisation, capturable.  ARGUMENT errors
 * return before any launch: ACX_ERR_ARG for a null pointer, a bad target_dtype, rows < 1, classes or k out of range, a row stride
 * shorter than `classes`, slice_rows < 0 or too many slices; rows > 2^30 is ACX_ERR_UNSUPPORTED; a workspace too small or not
 * 256-byte aligned is ACX_ERR_WORKSPACE. */
enum acx_ranking_count { ACX_RANK_N_POS = 0, ACX_RANK_COVERAGE = 1, ACX_RANK_BAD_PAIRS = 2, ACX_RANK_HITS = 3 };
#define ACX_RANK_COUNTS 4
#define ACX_RANK_WAVE_MAX_CLASSES 1024
ACX_API int acx_ranking_workspace_bytes(int64_t rows, int classes, int64_t slice_rows, size_t* out_bytes);
ACX_API int acx_ranking_metrics(const float* scores, int64_t ld_s, const void* target, int target_dtype, int64_t ld_t, int64_t rows,
                                int classes, int k, int64_t slice_rows, int64_t* row_counts, double* row_psum,
                                int64_t* class_count, double* class_psum, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* Which evaluation of the STFT the frontend uses (round 6).  ACX_FRONTEND_AUTO (default): the FFT kernel when the stored buffers are
 * window x DFT, the dense contraction otherwise (acx_finalize above).  ACX_FRONTEND_DENSE: ALWAYS the dense contraction with the
 * stored `conv_real` / `conv_imag` weights -- the reference's own formulation (two Conv1d, convnext.py:179-187,298) -- 2.1 GFLOP
 * per clip on the f32 matrix cores instead of 0.03.  It is the PARITY MODE for inputs whose spectrum has bins 90 dB and more under
 * the frame peak (pure tones off a bin centre, clean sweeps): such bins hold only the rounding noise of whichever formulation
 * computed them, and the reference's own outputs move by up to 1.4e-3 (frame embeddings) when its two Conv1d are merely
 * accumulated in float64.  Measured against the reference class on nine such probes (tests/test_gpu_frontend_edge.py,
 * profiles/r06_b_frontend_edge.txt): logits / probabilities / scene embeddings within 1e-3 with either frontend; frame embeddings
 * at the reference's own sensitivity with DENSE (<= 1.5e-3), at 2.4-2.7 x it with the FFT (<= 3.6e-3); every other input of the
 * suites is inside 1e-3 with the FFT.  Takes effect at once (re-finalizes a finalized context).  No reference counterpart: the
 * reference has one formulation. */
enum acx_frontend { ACX_FRONTEND_AUTO = 0, ACX_FRONTEND_DENSE = 1 };
ACX_API int acx_set_frontend(acx_ctx* ctx, int mode);

/* How acx_finalize decided to evaluate the frontend: *dense_dft = 0 when the stored STFT buffers are window x DFT (max
 * deviation *stft_deviation <= 2e-6) and the FFT kernel stands in for the two Conv1d, 1 when they are not and the
 * contraction runs as stored (GEMM on the f32 matrix cores) -- the reference applies whatever its state_dict holds
 * (convnext.py:179-187); *mel_taps = stored taps of the banded form of melW (884 for librosa's bank, up to 513 x 224 for a
 * dense matrix, which is applied as it is).  Any pointer may be NULL. */
ACX_API int acx_frontend_info(const acx_ctx* ctx, int* dense_dft, float* stft_deviation, int* mel_taps);

/* Diagnostics.  The tile-shape A/B switches ACX_GEMM_MI, ACX_WIDE_NPB, ACX_WIDE_PERSIST, ACX_DW_STREAM and ACX_DWM_WAVES, and
 * ACX_HEAD_PATH (1: the fused head kernel, 2: the class-tiled one, whatever N), and ACX_KNN_SLICE_ROWS (database rows per slice of
 * acx_knn_search, 16 .. 2^30: tests run many slices on a small database) and ACX_MOMENTS_SLICE_ROWS (rows per slice of
 * acx_moments, 16 .. 2^30, for the same purpose) are read from the
 * environment once, at the first acx_create; this re-reads them (tests force every tile shape through it and require
 * bit-identical results).  Launches never touch the environment.  No reference counterpart. */
ACX_API int acx_tuning_refresh(void);
/* Test support: make THIS CONTEXT's acx_forward report ACX_ERR_STATE after it has queued sub-batch `sub` (0 .. 3) of a split batch,
 * so that the error path -- joining the forked streams, ending a capture cleanly -- can be exercised; -1 switches it off (the
 * default; acx_finalize also resets it).  Per context (a process-global switch could poison every other user of the
 * library in the process), a call and not an environment variable.  No reference counterpart. */
ACX_API int acx_test_fail_sub(acx_ctx* ctx, int sub);
/* Test support: the tail of stage 0..2 exactly as the forwards queue it -- the stage's LAST block, which in the 16-bit arithmetics
 * writes LayerNorm(x_new) as the downsample conv's operand rows instead of x (x is then NOT updated: do not read it afterwards),
 * then downsample_layers[stage + 1] on those rows.  x NHWC (B,H,W,C_stage) fp32, out NHWC (B,H/2,W/2,C_{stage+1}) fp32 whatever
 * the precision (ACX_PREC_BF16_ACT converts at the boundary, as acx_block does).  scratch >= acx_test_stage_tail_scratch_bytes,
 * 256-byte aligned.  No other per-layer entry point reaches that epilogue.  No reference counterpart. */
ACX_API int acx_test_stage_tail(acx_ctx* ctx, int stage, float* x, float* out, int B, int H, int W, void* scratch,
                        size_t scratch_bytes, void* stream);
ACX_API int acx_test_stage_tail_scratch_bytes(int stage, int B, int H, int W, size_t* out_bytes);
/* Test support: the depthwise kernels per FORM.  The column-streaming kernel (dwconv_col.hip) cuts the stacked batch into segments
 * of n_out output rows and runs the instantiation for s0 = (7 - n_out % 7) % 7 on groups of seven rows (k7 of them), n_seg
 * segments x 6 wave columns = n_items waves; which one a launch gets depends on the batch, the clip length, the CU count and the
 * sub-batches in flight.  acx_test_dwconv7_plan reports what launch_dwconv_col would launch for B clips of H rows in `stage` at
 * `target_waves` (host arithmetic only: no context, no device; ACX_ERR_SHAPE where the kernel's multiply-high division refuses
 * the batch); acx_test_dwconv7_varlen_plan the same for the packed clips of `lengths` (samples), where n_out is a multiple of 7.
 * Both call the function the launchers call.  No reference counterpart. */
typedef struct acx_dwconv7_plan_t {
    int n_out, s0, k7, n_seg, n_items;
} acx_dwconv7_plan_t;
ACX_API int acx_test_dwconv7_plan(int stage, int B, int H, int target_waves, acx_dwconv7_plan_t* plan);
ACX_API int acx_test_dwconv7_varlen_plan(int stage, const int64_t* lengths, int n, int target_waves, acx_dwconv7_plan_t* plan);
/* acx_dwconv7 with the form chosen by the caller: form = 0 the ring / tile kernel of that width, form = 1 the column-streaming
 * kernel with `target_waves` (1 .. 4 x CUs) in place of 4 x CUs / sub-batches in flight (ignored by form 0).  stats as in
 * acx_dwconv7.  Everything is checked before the first launch. */
ACX_API int acx_test_dwconv7_form(acx_ctx* ctx, int stage, int block, const float* x, float* y, float* stats, int B, int H, int W,
                          int form, int target_waves, void* stream);
/* The depthwise conv of ONE stage of a packed batch as acx_forward_varlen queues it: builds the tables of `lengths` (n clips, in
 * samples, host) in `scratch` (>= acx_test_dwconv7_varlen_scratch_bytes, 256-byte aligned), then runs the variable-length launcher
 * at `target_waves` (1 .. 8 x CUs).  x, y: the clips' rows of that stage back to back, NHWC -- fp32, or bf16 in stages 0-2 under
 * ACX_PREC_BF16_ACT (the matrix-pipe kernel, `target_waves` 1 .. 9 x CUs: what ACX_DWM_WAVES can ask for). */
ACX_API int acx_test_dwconv7_varlen(acx_ctx* ctx, int stage, int block, const void* x, void* y, const int64_t* lengths, int n,
                            int target_waves, void* scratch, size_t scratch_bytes, void* stream);
ACX_API int acx_test_dwconv7_varlen_scratch_bytes(const int64_t* lengths, int n, size_t* out_bytes);
/* Test support: the matrix-pipe depthwise kernel of ACX_PREC_BF16_ACT (dwconv_mfma.hip, stages 0-2) per launch shape.  It cuts the
 * stacked batch into n_seg segments of `rows` = 4 `steps` output rows (a multiple of four, at least eight); every segment is
 * n_groups / n_seg (slice, segment) groups of waves, packed into `grid` workgroups.  acx_test_dwconv7_bf16_plan reports what the
 * launcher would launch for B clips of H rows in `stage` (0 .. 2) at `target_waves`, and in too_tall whether the launcher's guard
 * (the kernel's multiply-high division) refuses the batch -- host arithmetic only: no context, no device;
 * acx_test_dwconv7_bf16_varlen_plan the same for the packed clips of `lengths` (samples; too_tall is 0: the packed kernel divides
 * nothing).  Both call the functions the launchers call.  No reference counterpart. */
typedef struct acx_dwconv7_bf16_plan_t {
    int rows, steps, n_seg, n_groups, grid, too_tall;
} acx_dwconv7_bf16_plan_t;
ACX_API int acx_test_dwconv7_bf16_plan(int stage, int B, int H, int target_waves, acx_dwconv7_bf16_plan_t* plan);
ACX_API int acx_test_dwconv7_bf16_varlen_plan(int stage, const int64_t* lengths, int n, int target_waves, acx_dwconv7_bf16_plan_t* plan);
/* acx_dwconv7_bf16 with `target_waves` (1 .. 9 x CUs, the range ACX_DWM_WAVES = 2 .. 9 and the sub-batches in flight can produce)
 * in place of the shipped setting.  Refuses whatever acx_dwconv7_bf16 refuses; everything is checked before the launch. */
ACX_API int acx_test_dwconv7_bf16_form(acx_ctx* ctx, int stage, int block, const uint16_t* x, uint16_t* y, int B, int H, int W,
                               int target_waves, void* stream);
/* Test support: the stem kernel (K2) per FORM.  feat: the bn0'd log-mel rows, fp32; out: NHWC rows of 56 x 96 in the type the
 * context's precision stores at stage 0 -- fp32, or raw bf16 under ACX_PREC_BF16_ACT -- with no conversion at the boundary.
 *   uniform: lengths = NULL, n = 0: feat (B, T, 224) -> out (B, H0, 56, 96), H0 = (T + 4) / 4 + 1; scratch is not used.
 *   packed : lengths = n clip lengths in samples (HOST array, each >= ACX_MIN_SAMPLES, n <= ACX_MAX_VARLEN_CLIPS); B and T are
 *            ignored.  feat = the clips' frames back to back, out = their rows back to back.  The tables are built in `scratch`
 *            (>= acx_test_stem_scratch_bytes, 256-byte aligned) as acx_forward_varlen builds them.
 * max_blocks: 0 = the launcher's own grid (one workgroup per pair of output rows, at most 2048); 1 .. 2048 caps the grid below
 * that, so that a workgroup walks many row pairs on a small tensor.  The result does not depend on it.
 * Everything is checked before the first launch.  acx_test_stem_scratch_bytes needs no context; out_rows (may be NULL) receives
 * the number of stage-0 rows of the packed clips.  No reference counterpart. */
ACX_API int acx_test_stem(acx_ctx* ctx, const float* feat, void* out, int B, int T, const int64_t* lengths, int n, int max_blocks,
                          void* scratch, size_t scratch_bytes, void* stream);
ACX_API int acx_test_stem_scratch_bytes(const int64_t* lengths, int n, size_t* out_bytes, int64_t* out_rows);
/* Test support: the workspace plan of a forward as data -- host arithmetic only: no context, no device.  A forward carves its
 * workspace into REGIONS (the tables of a window / variable-length batch, feat, x of the four stages, and y, hidden, stats sized
 * for one block of stage 0; acx_forward_augmented puts five regions of its own in front) and then lends those regions to TENANTS
 * they were not sized for: the dense-DFT frontend's frames and spectrum, the LayerNorm rows the last block of a stage hands the
 * downsample, the arrays of the two-GEMM MLPs, the fp32 downsample's normalised rows, the segment embeddings, the scene rows of
 * the class-tiled head.  The forward computes every tenant's need with the definitions this call reports (need_* of
 * csrc/acx_internal.h) and refuses with ACX_ERR_STATE, before its first launch, a plan in which one does not fit.
 *   query : precision (enum acx_precision), dense (the dense-DFT frontend), classes, head_path (0: by class count, 1: fused, 2:
 *           class-tiled -- ACX_HEAD_PATH), driver, tail (enum acx_mode, or ACX_PLAN_TAIL_SEG_OUTPUT / _SEG_EMBED: the acx_forward_
 *           segments* calls; the features and augmented drivers take the three modes), ways (sub-batches, 1 .. 4; more than one
 *           needs 8 clips per sub-batch and a driver other than VARLEN), B clips of L samples (WINDOWS: B windows of L samples;
 *           VARLEN: the B entries of `lengths`; AUGMENTED: B clips going in, B / 2 into the trunk with has_lambda), and
 *           has_wave_plan / has_lambda of acx_forward_augmented.
 *   plan  : per sub-batch its clips, its first byte and size, every region as (offset, bytes) and every tenant as (kind, region,
 *           offset inside the region, bytes needed, phase: frontend / block `block` of `stage` / the downsample in front of `stage`
 *           / tail, operands: bit r set = the phase reads or writes region r in its own role).  All offsets count from the first
 *           byte of the workspace; a region that a plan does not have has 0 bytes; the regions in front of the nested forward
 *           (window table, acx_forward_augmented's five) are reported with sub-batch 0.  total: the last byte any sub-batch
 *           uses; promised: what the driver's acx_workspace_bytes* call returns for the batch.
 * No reference counterpart. */
enum { ACX_PLAN_UNIFORM = 0, ACX_PLAN_FEATURES = 1, ACX_PLAN_WINDOWS = 2, ACX_PLAN_VARLEN = 3, ACX_PLAN_AUGMENTED = 4 };
enum { ACX_PLAN_TAIL_SEG_OUTPUT = 3, ACX_PLAN_TAIL_SEG_EMBED = 4 };
enum {
    ACX_PLAN_TABLES = 0, ACX_PLAN_FEAT = 1, ACX_PLAN_X0 = 2, ACX_PLAN_Y = 6, ACX_PLAN_HIDDEN = 7, ACX_PLAN_STATS = 8,
    ACX_PLAN_AUG_WAVE = 9, ACX_PLAN_AUG_FEAT = 10, ACX_PLAN_AUG_MIX = 11, ACX_PLAN_AUG_FRAMES = 12, ACX_PLAN_AUG_SPEC = 13,
    ACX_PLAN_REGIONS = 14
};
enum {
    ACX_PLAN_DENSE_FRAMES = 0, ACX_PLAN_DENSE_SPEC = 1, ACX_PLAN_LN_ROWS = 2, ACX_PLAN_MLP_BF16_HIDDEN = 3, ACX_PLAN_MLP_BF16_ROWS = 4,
    ACX_PLAN_HIDDEN_ACT = 5, ACX_PLAN_ROW_STATS = 6, ACX_PLAN_XNORM = 7, ACX_PLAN_SEGMENT_EMB = 8, ACX_PLAN_SCENE_ROWS = 9,
    ACX_PLAN_TENANT_KINDS = 10
};
enum { ACX_PLAN_PHASE_FRONTEND = 0, ACX_PLAN_PHASE_BLOCK = 1, ACX_PLAN_PHASE_DOWNSAMPLE = 2, ACX_PLAN_PHASE_TAIL = 3 };
#define ACX_PLAN_MAX_TENANTS 40
#define ACX_PLAN_MAX_WAYS 4
typedef struct acx_plan_region_t { uint64_t offset, bytes; } acx_plan_region_t;
typedef struct acx_plan_tenant_t {
    int32_t kind, region, phase, stage, block;
    uint32_t operands;
    uint64_t offset, bytes;
} acx_plan_tenant_t;
typedef struct acx_plan_sub_t {
    int32_t clips, n_tenants;
    uint64_t base, bytes;
    acx_plan_region_t regions[ACX_PLAN_REGIONS];
    acx_plan_tenant_t tenants[ACX_PLAN_MAX_TENANTS];
} acx_plan_sub_t;
typedef struct acx_forward_plan_t {
    int32_t n_subs, reserved;
    uint64_t total, promised;
    acx_plan_sub_t subs[ACX_PLAN_MAX_WAYS];
} acx_forward_plan_t;
typedef struct acx_forward_plan_query_t {
    int32_t precision, dense, classes, head_path, driver, tail, ways, B, has_wave_plan, has_lambda;
    int64_t L;
    const int64_t* lengths;
} acx_forward_plan_query_t;
ACX_API int acx_test_forward_plan(const acx_forward_plan_query_t* query, acx_forward_plan_t* plan);
/* Test support: fill the device state of a live stream's slot -- its ring (2 C samples), its input history (Ch samples) and its
 * probability history (Hw x classes) -- with 0xFF bytes on `stream`, so that a window or timeline row that touches a sample or a
 * history row its own recording did not write comes out NaN instead of the zeros of acx_stream_create.  slot = -1: every slot.
 * ACX_ERR_STATE while a listed slot has an open recording, or windows or rows that are not fetched yet (nothing is written
 * then).  Changes nothing for callers who never call it.  No reference counterpart. */
ACX_API int acx_test_stream_poison(acx_stream* st, int slot, void* stream);
/* Test support: the resampler's launch plan as data, and its launch with the grid capped.  A workgroup forms tiles of
 * outputs_per_tile = 256 per_thread consecutive outputs of one clip from an input span staged in lds_bytes of LDS; per_thread is 4,
 * 2 or 1, the largest whose span  (outputs_per_tile - 1) of / nf + 2 width + 4  floats fits the kernel's LDS budget, and a call
 * launches min(tiles, max_grid) workgroups, each walking tiles t, t + grid, ...  acx_test_resample_plan reports what
 * acx_resampler_create would build for orig_hz -> new_hz, from the function it calls -- host arithmetic only, no device -- and
 * refuses what it refuses (ACX_ERR_UNSUPPORTED where no form fits).  acx_test_resample is acx_resample with at most max_blocks
 * (1 .. max_grid) workgroups, so that a workgroup walks many tiles of a small call; the result does not depend on it.  Everything
 * is checked before the launch.  No reference counterpart. */
typedef struct acx_resample_plan_t {
    int32_t of, nf, width, max_band, per_thread, lds_bytes, outputs_per_tile, max_grid;
} acx_resample_plan_t;
ACX_API int acx_test_resample_plan(int orig_hz, int new_hz, acx_resample_plan_t* plan);
ACX_API int acx_test_resample(const acx_resampler* rs, const float* in, const int64_t* lengths, int B, float* out, int max_blocks,
                              void* stream);

/* ---- measurement: per-kernel-class device time, HIP events on the launch stream ------------ */
ACX_API int acx_profile_enable(acx_ctx* ctx, int on);
/* Synchronises the recorded events; fills ms[ACX_K_COUNT], launches[ACX_K_COUNT]; resets. */
ACX_API int acx_profile_read(acx_ctx* ctx, double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* ACX_H */
