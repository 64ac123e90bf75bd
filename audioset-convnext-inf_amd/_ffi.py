"""ctypes binding of libacx.so (include/acx.h).  Plumbing only: torch tensors are handed over as raw
device pointers + sizes; the library never sees a torch type.

The library is built in-tree (`audioset-convnext-inf_amd/libacx.so`, see `__graft_entry__.build()`).
If it is missing, importing this module still works (CPU-only hosts can inspect the package), but
any attempt to *use* the product path raises -- there is no CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACX_LIB") or os.path.join(_HERE, "libacx.so")     # ACX_LIB: diagnostic builds (tools/)

OK = 0
MODE_LOGITS, MODE_SCENE, MODE_FRAME = 0, 1, 2
KERNEL_CLASSES = ("frontend", "stem", "dwconv", "pw1", "pw2", "rowstats", "downsample", "poolhead", "transpose",
                  "mlp_fused", "mlp_wide")
MIN_SAMPLES = 7360
MAX_VARLEN_CLIPS = 256
SEG_OUTPUT, SEG_EMBED = 0, 1         # enum acx_segment_what
SEGMENT_SAMPLES = 10240              # ACX_SEGMENT_SAMPLES: 32 STFT frames of 320 samples
MAX_SEGMENT_POOL = 31                # ACX_MAX_SEGMENT_POOL
NUM_CLASSES = 527          # the AudioSet head (ACX_NUM_CLASSES)
MAX_CLASSES = 32768        # widest classifier head a context takes (ACX_MAX_CLASSES)

_c_int, _c_i64, _c_sz, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
_pint = ctypes.POINTER(ctypes.c_int)



class AcxAdam(ctypes.Structure):
    """struct acx_adam: the optimiser settings of acx_head_fit_step / acx_adam_update."""
    _fields_ = [("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("amsgrad", ctypes.c_int), ("decoupled", ctypes.c_int)]


_padam, _c_dbl = ctypes.POINTER(AcxAdam), ctypes.c_double


class AcxFitJob(ctypes.Structure):
    """struct acx_fit_job: the device pointers of one job of acx_head_fit_group_step (80 bytes)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("idx", "W", "b", "mW", "vW", "vmaxW", "mb", "vb", "vmaxb", "loss")]


class AcxEvent(ctypes.Structure):
    """struct acx_event: one row of the event table of acx_decode_events (32 bytes)."""
    _fields_ = [("clip", ctypes.c_int32), ("cls", ctypes.c_int32), ("begin", ctypes.c_int32), ("end", ctypes.c_int32),
                ("peak", ctypes.c_float), ("reserved", ctypes.c_float), ("mean", ctypes.c_double)]


class AcxEventParams(ctypes.Structure):
    """struct acx_event_params: the decoding settings of acx_decode_events."""
    _fields_ = [("threshold", ctypes.c_float), ("low", ctypes.c_float), ("median", ctypes.c_int),
                ("min_duration", ctypes.c_double), ("merge_gap", ctypes.c_double)]


_pevp, _pdbl = ctypes.POINTER(AcxEventParams), ctypes.POINTER(ctypes.c_double)


class AcxOperatingSpec(ctypes.Structure):
    """struct acx_operating_spec: the criterion of acx_operating_points."""
    _fields_ = [("criterion", ctypes.c_int32), ("param", ctypes.c_double)]


_pops = ctypes.POINTER(AcxOperatingSpec)


class AcxRefEvent(ctypes.Structure):
    """struct acx_ref_event: one row of the reference table of acx_score_events / acx_score_segments / acx_score_intersection (24 bytes)."""
    _fields_ = [("clip", ctypes.c_int32), ("cls", ctypes.c_int32), ("onset", ctypes.c_double), ("offset", ctypes.c_double)]


class AcxEventCollar(ctypes.Structure):
    """struct acx_event_collar: the matching settings of acx_score_events."""
    _fields_ = [("t_collar", ctypes.c_double), ("percentage_of_length", ctypes.c_double), ("evaluate_onset", ctypes.c_int32),
                ("evaluate_offset", ctypes.c_int32)]


_pcol = ctypes.POINTER(AcxEventCollar)


class AcxIntersectionCriteria(ctypes.Structure):
    """struct acx_intersection_criteria: the three ratios of acx_score_intersection."""
    _fields_ = [("dtc", ctypes.c_double), ("gtc", ctypes.c_double), ("cttc", ctypes.c_double), ("cross_triggers", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


_pcrit = ctypes.POINTER(AcxIntersectionCriteria)

AUG_MAX_STRIPES = 4                  # ACX_AUG_MAX_STRIPES


class AcxWaveAug(ctypes.Structure):
    """struct acx_wave_aug: one clip's waveform plan of acx_augment_wave (40 bytes)."""
    _fields_ = [("step", ctypes.c_double), ("n_out", ctypes.c_int64), ("shift", ctypes.c_int64), ("roll", ctypes.c_int64),
                ("gain", ctypes.c_float), ("reserved", ctypes.c_int32)]


class AcxSpecAug(ctypes.Structure):
    """struct acx_spec_aug: one clip's stripes of acx_augment_spec (64 bytes)."""
    _fields_ = [(k, ctypes.c_int32 * AUG_MAX_STRIPES) for k in ("t_bgn", "t_len", "f_bgn", "f_len")]


class AcxDwconv7Plan(ctypes.Structure):
    """struct acx_dwconv7_plan_t: what a column-kernel launch consists of (acx_test_dwconv7_plan)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_out", "s0", "k7", "n_seg", "n_items")]


_pplan = ctypes.POINTER(AcxDwconv7Plan)


class AcxDwconv7Bf16Plan(ctypes.Structure):
    """struct acx_dwconv7_bf16_plan_t: what a launch of the matrix-pipe depthwise kernel consists of (acx_test_dwconv7_bf16_plan)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("rows", "steps", "n_seg", "n_groups", "grid", "too_tall")]


_pplan16 = ctypes.POINTER(AcxDwconv7Bf16Plan)


class AcxResamplePlan(ctypes.Structure):
    """struct acx_resample_plan_t: the tables and the tile form of a rate pair (acx_test_resample_plan)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("of", "nf", "width", "max_band", "per_thread", "lds_bytes", "outputs_per_tile",
                                              "max_grid")]

# acx_test_forward_plan: the workspace plan of a forward as data (include/acx.h, ACX_PLAN_*)
PLAN_DRIVERS = {"uniform": 0, "features": 1, "windows": 2, "varlen": 3, "augmented": 4}
PLAN_TAILS = {"logits": 0, "scene": 1, "frame": 2, "segment": 3, "segment_embeddings": 4}
PLAN_REGIONS = ("tables", "feat", "x0", "x1", "x2", "x3", "y", "hidden", "stats", "aug_wave", "aug_feat", "aug_mix", "aug_frames",
                "aug_spec")
PLAN_TENANTS = ("dense_frames", "dense_spec", "ln_rows", "mlp_bf16_hidden", "mlp_bf16_rows", "hidden_act", "row_stats", "xnorm",
                "segment_emb", "scene_rows")
PLAN_PHASES = ("frontend", "block", "downsample", "tail")
PLAN_MAX_TENANTS, PLAN_MAX_WAYS = 40, 4


class AcxPlanRegion(ctypes.Structure):
    """struct acx_plan_region_t"""
    _fields_ = [("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class AcxPlanTenant(ctypes.Structure):
    """struct acx_plan_tenant_t"""
    _fields_ = [(k, ctypes.c_int32) for k in ("kind", "region", "phase", "stage", "block")] + [
        ("operands", ctypes.c_uint32), ("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class AcxPlanSub(ctypes.Structure):
    """struct acx_plan_sub_t: one sub-batch of a forward's plan"""
    _fields_ = [("clips", ctypes.c_int32), ("n_tenants", ctypes.c_int32), ("base", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("regions", AcxPlanRegion * len(PLAN_REGIONS)), ("tenants", AcxPlanTenant * PLAN_MAX_TENANTS)]


class AcxForwardPlan(ctypes.Structure):
    """struct acx_forward_plan_t"""
    _fields_ = [("n_subs", ctypes.c_int32), ("reserved", ctypes.c_int32), ("total", ctypes.c_uint64), ("promised", ctypes.c_uint64),
                ("subs", AcxPlanSub * PLAN_MAX_WAYS)]


class AcxForwardPlanQuery(ctypes.Structure):
    """struct acx_forward_plan_query_t"""
    _fields_ = [(k, ctypes.c_int32) for k in ("precision", "dense", "classes", "head_path", "driver", "tail", "ways", "B",
                                              "has_wave_plan", "has_lambda")] + [
        ("L", ctypes.c_int64), ("lengths", ctypes.POINTER(ctypes.c_int64))]

# name -> (restype, argtypes); mirrors include/acx.h one to one
SIGNATURES = {
    "acx_last_error": (ctypes.c_char_p, []),
    "acx_version": (_c_int, []),
    "acx_create": (_c_int, [_c_int, ctypes.POINTER(_vp)]),
    "acx_destroy": (None, [_vp]),
    "acx_set_weight": (_c_int, [_vp, ctypes.c_char_p, _vp, ctypes.POINTER(_c_i64), _c_int]),
    "acx_finalize": (_c_int, [_vp]),
    "acx_set_precision": (_c_int, [_vp, _c_int]),
    "acx_num_classes": (_c_int, [_vp, _pint]),
    "acx_num_frames": (_c_int, [_c_i64, _pint]),
    "acx_stage_hw": (_c_int, [_c_i64, _c_int, _pint, _pint]),
    "acx_workspace_bytes": (_c_int, [_vp, _c_int, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_sub_batches": (_c_int, [_vp, _c_int, ctypes.POINTER(_c_int)]),
    "acx_forward": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_int, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_workspace_bytes_varlen": (_c_int, [_vp, ctypes.POINTER(_c_i64), _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_forward_varlen": (_c_int, [_vp, _vp, ctypes.POINTER(_c_i64), _c_int, _c_int, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_window_count": (_c_int, [ctypes.POINTER(_c_i64), _c_int, _c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    "acx_workspace_bytes_windows": (_c_int, [_vp, _c_int, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_forward_windows": (_c_int, [_vp, _vp, ctypes.POINTER(_c_i64), _c_int, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp,
                                     _vp, _c_sz, _vp]),
    "acx_window_timeline": (_c_int, [_vp, ctypes.POINTER(_c_i64), _c_int, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "acx_window_timeline_classes": (_c_int, [_vp, _c_int, ctypes.POINTER(_c_i64), _c_int, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "acx_segment_count": (_c_int, [_c_i64, _pint]),
    "acx_workspace_bytes_segments": (_c_int, [_vp, _c_int, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_forward_segments": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_workspace_bytes_segments_varlen": (_c_int, [_vp, ctypes.POINTER(_c_i64), _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_forward_segments_varlen": (_c_int, [_vp, _vp, ctypes.POINTER(_c_i64), _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_sz,
                                             _vp]),
    "acx_workspace_bytes_segments_windows": (_c_int, [_vp, _c_int, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_forward_segments_windows": (_c_int, [_vp, _vp, ctypes.POINTER(_c_i64), _c_int, _c_i64, _c_i64, _c_i64, _c_int, _c_int,
                                              _c_int, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_segment_head": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    "acx_segment_expand": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    "acx_segment_expand_varlen": (_c_int, [_vp, ctypes.POINTER(_c_i64), _c_int, _c_int, _vp, _vp]),
    "acx_segment_timeline": (_c_int, [_vp, _c_int, ctypes.POINTER(_c_i64), _c_int, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "acx_events_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_decode_events": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _pevp, _c_dbl, _c_dbl, _vp, _c_i64, _vp, _vp, _vp, _c_sz,
                                   _vp]),
    "acx_decode_events_varlen": (_c_int, [_vp, _c_i64, _pint, _pdbl, _c_int, _c_int, _pevp, _c_dbl, _vp, _c_i64, _vp, _vp, _vp,
                                          _c_sz, _vp]),
    "acx_decode_events_classwise": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _pevp, _c_dbl, _c_dbl, _vp, _c_i64, _vp, _vp, _vp,
                                             _c_sz, _vp, _vp, _vp]),
    "acx_decode_events_varlen_classwise": (_c_int, [_vp, _c_i64, _pint, _pdbl, _c_int, _c_int, _pevp, _c_dbl, _vp, _c_i64, _vp, _vp,
                                                    _vp, _c_sz, _vp, _vp, _vp]),
    "acx_event_stream_bytes": (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_event_stream_create": (_c_int, [_c_int, _c_int, _pevp, _c_dbl, _vp, _vp, ctypes.POINTER(_vp)]),
    "acx_event_stream_destroy": (None, [_vp]),
    "acx_event_stream_push": (_c_int, [_vp, _vp, _c_i64, _pint, _pint, _c_int, _vp, _c_i64, _vp, _vp, _vp]),
    "acx_event_stream_close": (_c_int, [_vp, _pint, _pdbl, _c_int, _vp, _c_i64, _vp, _vp, _vp]),
    "acx_event_stream_open": (_c_int, [_vp, _pint, _c_int, _vp, _vp]),
    "acx_event_stream_steps": (_c_int, [_vp, _c_int, ctypes.POINTER(_c_i64)]),
    "acx_event_stream_undo": (_c_int, [_vp, _pint, _c_int]),
    "acx_score_events": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _c_int, _vp, _vp, _c_dbl, _pcol, _vp, _vp, _vp, _vp,
                                  _vp]),
    "acx_score_segments": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _c_int, _vp, _vp, _c_dbl, _c_dbl, _vp, _vp, _vp,
                                    _vp]),
    "acx_score_intersection": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _c_int, _vp, _vp, _c_dbl, _pcrit, _vp, _vp, _vp,
                                        _vp, _vp, _vp]),
    "acx_cross_trigger_rate": (_c_int, [_vp, _vp, _c_int, _vp, _vp]),
    "acx_logmel_bn0": (_c_int, [_vp, _vp, _c_int, _c_i64, _vp, _c_int, _vp]),
    "acx_stem_ln": (_c_int, [_vp, _vp, _c_int, _c_int, _vp, _vp]),
    "acx_dwconv7": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int, _vp]),
    "acx_dwconv7_bf16": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _c_int, _vp]),
    "acx_block": (_c_int, [_vp, _c_int, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _c_sz, _vp]),
    "acx_block_scratch_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_downsample": (_c_int, [_vp, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int, _vp]),
    "acx_pool_head": (_c_int, [_vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    "acx_nhwc_to_nchw": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _vp]),
    "acx_comm_unique_id": (_c_int, [_vp]),
    "acx_comm_init": (_c_int, [_vp, _c_int, _c_int, _vp]),
    "acx_allgather": (_c_int, [_vp, _vp, _vp, _c_sz, _vp]),
    "acx_comm_info": (_c_int, [_vp, _pint, _pint]),
    "acx_pcm16_to_f32": (_c_int, [_vp, _vp, _c_i64, _vp]),
    "acx_stream_schedule": (_c_int, [_c_i64, _c_i64, _c_int, _c_i64, _c_int, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64),
                                     ctypes.POINTER(_c_i64)]),
    "acx_stream_geometry": (_c_int, [_c_i64, _c_i64, _c_int, _c_i64, _c_int] + [ctypes.POINTER(_c_i64)] * 4),
    "acx_test_stream_poison": (_c_int, [_vp, _c_int, _vp]),
    "acx_stream_create": (_c_int, [_vp, _c_int, _c_i64, _c_i64, _c_int, _c_i64, _c_int, ctypes.POINTER(_vp)]),
    "acx_stream_destroy": (None, [_vp]),
    "acx_stream_push": (_c_int, [_vp, _vp, _pint, ctypes.POINTER(_c_i64), _c_int, _vp]),
    "acx_stream_close": (_c_int, [_vp, _pint, _c_int, _vp]),
    "acx_stream_pending": (_c_int, [_vp, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "acx_stream_next": (_c_int, [_vp, _c_int, _pint, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _pint]),
    "acx_stream_forward": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_stream_timeline": (_c_int, [_vp, _c_int, _c_i64, _vp, _pint, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _vp]),
    "acx_resample_geometry": (_c_int, [_c_int, _c_int, _pint, _pint, _pint, _pint]),
    "acx_resample_taps": (_c_int, [_c_int, _c_int, _pint, _pint, ctypes.POINTER(ctypes.c_float), _c_sz]),
    "acx_resampled_length": (_c_int, [_c_int, _c_int, _c_i64, ctypes.POINTER(_c_i64)]),
    "acx_resampler_create": (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_vp)]),
    "acx_resampler_destroy": (None, [_vp]),
    "acx_resample": (_c_int, [_vp, _vp, ctypes.POINTER(_c_i64), _c_int, _vp, _vp]),
    "acx_augment_plan_check": (_c_int, [_c_int, _c_i64, _vp, _vp]),
    "acx_augment_wave": (_c_int, [_vp, _c_int, _c_i64, _vp, _vp, _vp]),
    "acx_augment_spec": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    "acx_forward_features": (_c_int, [_vp, _vp, _c_int, _c_i64, _c_int, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_workspace_bytes_augmented": (_c_int, [_vp, _c_int, _c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_forward_augmented": (_c_int, [_vp, _vp, _c_int, _c_i64, _vp, _vp, _vp, _c_int, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_metrics_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_tagging_metrics": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_operating_points": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _pops, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_threshold_counts": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _vp]),
    "acx_bootstrap_weights": (_c_int, [ctypes.c_uint64, ctypes.c_uint32, _c_int, _c_i64, _vp, _c_i64, _vp]),
    "acx_weighted_metrics_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_weighted_metrics": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _vp, _c_i64, _c_int, _vp, _vp, _vp, _vp, _vp,
                                      _c_sz, _vp]),
    "acx_head_fit_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_head_fit_step": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_int, _c_i64, _vp, _c_i64, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _padam, _c_i64, _c_dbl, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_head_fit_grad": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_int, _c_i64, _vp, _c_i64, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _c_sz, _vp]),
    "acx_adam_update": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _padam, _c_i64, _c_dbl, _vp]),
    "acx_head_fit_ce_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_head_fit_step_ce": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _c_i64, _c_int, _c_dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _padam, _c_i64, _c_dbl, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_head_fit_grad_ce": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _c_i64, _c_int, _c_dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _c_sz, _vp]),
    "acx_head_fit_mil_workspace_bytes": (_c_int, [_c_i64, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_head_fit_step_mil": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_int, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _c_int, _c_int,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _padam, _c_i64, _c_dbl, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_head_fit_grad_mil": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_int, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _c_int, _c_int,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_segment_pool": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _vp, _vp]),
    "acx_head_fit_group_workspace_bytes": (_c_int, [_c_int, _c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_head_fit_plan_bytes": (_c_int, [_c_int, _c_i64, ctypes.POINTER(_c_sz)]),
    "acx_head_fit_plan_fill": (_c_int, [_c_int, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _padam, _vp, _vp, _c_sz]),
    "acx_head_fit_group_step": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_int, _c_i64, _c_int, _c_i64, _c_int, _vp, _vp, _c_i64, _c_i64,
                                         _vp, _vp, _c_sz, _vp]),
    "acx_head_fit_group_step_ce": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_int, _c_i64, _c_int, _c_dbl, _vp, _vp, _c_i64, _c_i64, _vp,
                                            _vp, _c_sz, _vp]),
    "acx_softmax_topk": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _vp, _c_i64, _vp, _vp, _vp, _vp]),
    "acx_classification_counts": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp]),
    "acx_reliability_counts": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "acx_reliability_toplabel": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_platt_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_platt_fit": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_platt_apply": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _c_i64, _vp]),
    "acx_temperature_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_temperature_fit": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_temperature_apply": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _c_i64, _vp]),
    "acx_knn_row_norms": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _vp]),
    "acx_knn_workspace_bytes": (_c_int, [_c_i64, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_knn_slices": (_c_int, [_c_i64, _c_i64, _c_int, _pint]),
    "acx_knn_search": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp,
                                _c_sz, _vp]),
    "acx_knn_vote": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _c_int, _c_i64, _c_i64, _c_int, _c_int, ctypes.c_float, _vp, _c_i64,
                              _vp, _vp]),
    "acx_knn_quantize_i8": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _vp, _vp]),
    "acx_knn_search_i8": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_sz,
                                   _vp]),
    "acx_knn_rescore": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _c_i64, _c_int, _c_int, _vp,
                                 _vp, _vp, _vp]),
    "acx_kmeans_workspace_bytes": (_c_int, [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_kmeans_assign": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "acx_kmeans_update": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _c_int, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_sz,
                                   _vp]),
    "acx_kmeans_fit": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                _c_sz, _vp]),
    "acx_kmeans_min_distance": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "acx_kmeans_sample": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_kmeans_seed": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _c_int, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_sz, _vp]),
    "acx_gmm_workspace_bytes": (_c_int, [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_gmm_estep": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_sz,
                               _vp]),
    "acx_gmm_score": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_gmm_mstep": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _c_i64, _c_int, _c_dbl, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz,
                               _vp]),
    "acx_gmm_fit": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int, _vp, _c_dbl, _vp, _vp, _vp, _vp, _vp, _vp,
                             _c_sz, _vp]),
    "acx_cluster_scores_workspace_bytes": (_c_int, [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_silhouette": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _vp, _c_int, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _c_sz, _vp]),
    "acx_cluster_dispersion": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_contingency": (_c_int, [_vp, _c_int, _vp, _c_int, _c_i64, _vp, _vp, _vp]),
    "acx_radius_workspace_bytes": (_c_int, [_c_i64, _c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_radius_slices": (_c_int, [_c_i64, _c_i64, _c_int, _pint]),
    "acx_radius_row_sumsq": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "acx_radius_count": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, ctypes.c_float, _c_int, _vp, _vp,
                                  _vp, _c_sz, _vp]),
    "acx_radius_neighbors": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, ctypes.c_float, _c_int, _c_int,
                                      _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_radius_emit": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, ctypes.c_float, _c_int, _c_int,
                                 _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_graph_components": (_c_int, [_vp, _vp, _c_i64, _vp, _vp, _c_int, _c_int, _vp]),
    "acx_dbscan_workspace_bytes": (_c_int, [_c_i64, ctypes.POINTER(_c_sz)]),
    "acx_dbscan_labels": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _vp, _vp, _vp, _vp, _c_sz, _c_int, _vp]),
    "acx_moments_workspace_bytes": (_c_int, [_c_i64, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_moments": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _c_i64, _vp, _vp, _c_sz, _vp]),
    "acx_gram_f64": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_int, _c_int, _vp, _c_i64, _vp]),
    "acx_eigh_workspace_bytes": (_c_int, [_c_int, ctypes.POINTER(_c_sz)]),
    "acx_eigh": (_c_int, [_vp, _c_i64, _c_int, _c_int, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_sz, _vp]),
    "acx_pca_transform": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _c_i64, _c_int, _vp, _vp, _c_i64, _vp]),
    "acx_pca_inverse": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _vp, _vp, _c_i64, _c_int, _vp, _vp, _c_i64, _vp]),
    "acx_ranking_workspace_bytes": (_c_int, [_c_i64, _c_int, _c_i64, ctypes.POINTER(_c_sz)]),
    "acx_ranking_metrics": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _c_int, _c_int, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _c_sz, _vp]),
    "acx_frontend_info": (_c_int, [_vp, _pint, ctypes.POINTER(ctypes.c_float), _pint]),
    "acx_set_frontend": (_c_int, [_vp, _c_int]),
    "acx_tuning_refresh": (_c_int, []),
    "acx_test_fail_sub": (_c_int, [_vp, _c_int]),
    "acx_test_stage_tail": (_c_int, [_vp, _c_int, _vp, _vp, _c_int, _c_int, _c_int, _vp, _c_sz, _vp]),
    "acx_test_stage_tail_scratch_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "acx_test_dwconv7_plan": (_c_int, [_c_int, _c_int, _c_int, _c_int, _pplan]),
    "acx_test_dwconv7_varlen_plan": (_c_int, [_c_int, ctypes.POINTER(_c_i64), _c_int, _c_int, _pplan]),
    "acx_test_dwconv7_form": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "acx_test_dwconv7_varlen": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, ctypes.POINTER(_c_i64), _c_int, _c_int, _vp, _c_sz, _vp]),
    "acx_test_dwconv7_bf16_plan": (_c_int, [_c_int, _c_int, _c_int, _c_int, _pplan16]),
    "acx_test_dwconv7_bf16_varlen_plan": (_c_int, [_c_int, ctypes.POINTER(_c_i64), _c_int, _c_int, _pplan16]),
    "acx_test_dwconv7_bf16_form": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _vp]),
    "acx_test_dwconv7_varlen_scratch_bytes": (_c_int, [ctypes.POINTER(_c_i64), _c_int, ctypes.POINTER(_c_sz)]),
    "acx_test_stem": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, ctypes.POINTER(_c_i64), _c_int, _c_int, _vp, _c_sz, _vp]),
    "acx_test_stem_scratch_bytes": (_c_int, [ctypes.POINTER(_c_i64), _c_int, ctypes.POINTER(_c_sz), ctypes.POINTER(_c_i64)]),
    "acx_test_forward_plan": (_c_int, [ctypes.POINTER(AcxForwardPlanQuery), ctypes.POINTER(AcxForwardPlan)]),
    "acx_test_resample_plan": (_c_int, [_c_int, _c_int, ctypes.POINTER(AcxResamplePlan)]),
    "acx_test_resample": (_c_int, [_vp, _vp, ctypes.POINTER(_c_i64), _c_int, _vp, _c_int, _vp]),
    "acx_profile_enable": (_c_int, [_vp, _c_int]),
    "acx_profile_read": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64)]),
}

_lib = None


class AcxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libacx error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load libacx.so once.  Raises if the HIP library has not been built: no fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                "libacx.so not found at %s -- build it first (python -c 'import __graft_entry__ as g; g.build()' "
                "or make -C audioset-convnext-inf_amd/csrc). The HIP library IS the product path; "
                "there is no CPU fallback." % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc):
    if rc != OK:
        raise AcxError(rc, lib().acx_last_error().decode("utf-8", "replace"))


def ptr(t):
    """Raw pointer of a torch tensor (must be contiguous) or None."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor handed to libacx must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def vp(t):
    """Raw pointer of a torch tensor or None, whatever its strides.  ptr() is for calls that take no stride and so need a
    contiguous tensor; vp() is for the analysis calls, which pass the row stride along and read views where they lie."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _query(fn, ctype, *args):
    """The value a host-only query writes through its last parameter: fn(*args, &out) checked, -> out."""
    out = ctype()
    check(fn(*args, ctypes.byref(out)))
    return out.value


def forward_plan(precision, driver="uniform", tail="logits", B=1, L=MIN_SAMPLES, lengths=None, dense=False, classes=NUM_CLASSES,
                 head_path=0, ways=1, wave=False, lam=False, out=None):
    """acx_test_forward_plan -> AcxForwardPlan (filled into `out` when given: a sweep reuses one).  No context, no device."""
    q = AcxForwardPlanQuery(PRECISIONS[precision], int(dense), classes, head_path, PLAN_DRIVERS[driver], PLAN_TAILS[tail], ways,
                            len(lengths) if lengths is not None else B, int(wave), int(lam), L, None)
    if lengths is not None:
        keep = (ctypes.c_int64 * len(lengths))(*lengths)
        q.lengths = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int64))
    plan = out if out is not None else AcxForwardPlan()
    check(lib().acx_test_forward_plan(ctypes.byref(q), ctypes.byref(plan)))
    return plan


def stream_ptr(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


PRECISIONS = {"fp32": 0, "bf16": 1, "fp32_split": 2, "bf16a": 3}
FRONTENDS = {"auto": 0, "dense": 1}      # enum acx_frontend
# the five output kinds of the forwards (`what=`): enum acx_mode, and enum acx_segment_what of the acx_forward_segments* calls
MODES = {"logits": MODE_LOGITS, "scene": MODE_SCENE, "frame": MODE_FRAME}
SEG_WHAT = {"segment": SEG_OUTPUT, "segment_embeddings": SEG_EMBED}


class Context:
    """Owns one acx_ctx (repacked weights on one GPU)."""

    def __init__(self, device_index):
        self._h = _vp()
        check(lib().acx_create(int(device_index), ctypes.byref(self._h)))
        self.device_index = int(device_index)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().acx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        # at interpreter shutdown the module globals (lib, _vp) may already be gone: the process is about to
        # release the device anyway
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    @property
    def handle(self):
        return self._h

    def set_precision(self, precision):
        """"fp32" (default, the parity path) or "bf16" (bf16 MFMA operands, fp32 accumulate / LayerNorm / residual).
        Takes effect at the next load_state_dict()."""
        check(lib().acx_set_precision(self._h, PRECISIONS[precision]))

    def load_state_dict(self, sd):
        """sd: mapping key -> tensor (any device); fp32 tensors are staged through host memory."""
        import torch
        l = lib()
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                continue
            t = v.detach().to(device="cpu", dtype=torch.float32).contiguous()
            shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
            check(l.acx_set_weight(self._h, k.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()))
        check(l.acx_finalize(self._h))

    def num_classes(self):
        """N, the class count of the finalized head (acx_num_classes)."""
        return _query(lib().acx_num_classes, _c_int, self._h)

    def _workspace_bytes(self, geometry, kind, *args):
        """acx_workspace_bytes<geometry> for an output kind: a key of MODES (or the acx_mode value itself), or a key of
        SEG_WHAT, which goes to the _segments form of the call."""
        seg = kind in SEG_WHAT
        fn = getattr(lib(), "acx_workspace_bytes" + ("_segments" if seg else "") + geometry)
        return _query(fn, _c_sz, self._h, *args, SEG_WHAT[kind] if seg else int(MODES.get(kind, kind)))

    def workspace_bytes(self, B, L, kind):
        return self._workspace_bytes("", kind, int(B), int(L))

    def workspace_bytes_augmented(self, B, L, has_wave_plan, has_lambda, kind):
        return _query(lib().acx_workspace_bytes_augmented, _c_sz, self._h, int(B), int(L), 1 if has_wave_plan else 0,
                      1 if has_lambda else 0, int(MODES.get(kind, kind)))

    def workspace_bytes_varlen(self, lengths, kind):
        lens = (_c_i64 * max(1, len(lengths)))(*[int(n) for n in lengths])
        return self._workspace_bytes("_varlen", kind, lens, len(lengths))

    def workspace_bytes_windows(self, count, window, kind):
        return self._workspace_bytes("_windows", kind, int(count), int(window))

    def sub_batches(self, B):
        """How many sub-batches (on separate streams) a forward of B clips runs as (acx_sub_batches)."""
        return _query(lib().acx_sub_batches, _c_int, self._h, int(B))

    # ---- the C ABI's own collective (include/acx.h): RCCL all-gather without torch.distributed ----
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(128)
        check(lib().acx_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        check(lib().acx_comm_init(self._h, int(rank), int(world), ctypes.c_char_p(unique_id)))

    def allgather(self, local):
        """(n, ...) contiguous device tensor -> (world * n, ...) in rank order, on the current stream."""
        import torch
        r, w = _c_int(), _c_int()
        check(lib().acx_comm_info(self._h, ctypes.byref(r), ctypes.byref(w)))
        out = torch.empty((w.value * local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        check(lib().acx_allgather(self._h, ptr(local), ptr(out), local.numel() * local.element_size(), stream_ptr(local.device)))
        return out

    def set_frontend(self, mode):
        """"auto" (FFT kernel when the stored STFT buffers are window x DFT) or "dense" (always the reference's dense DFT
        contraction with the stored weights: the parity mode, acx.h acx_set_frontend)."""
        check(lib().acx_set_frontend(self._h, FRONTENDS[mode]))

    def frontend_info(self):
        """{"dense_dft": bool, "stft_deviation": float, "mel_taps": int} -- how acx_finalize evaluates the frontend."""
        d, dev, taps = _c_int(), ctypes.c_float(), _c_int()
        check(lib().acx_frontend_info(self._h, ctypes.byref(d), ctypes.byref(dev), ctypes.byref(taps)))
        return {"dense_dft": bool(d.value), "stft_deviation": dev.value, "mel_taps": taps.value}

    def profile(self, on):
        check(lib().acx_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        ms = (ctypes.c_double * len(KERNEL_CLASSES))()
        n = (ctypes.c_int64 * len(KERNEL_CLASSES))()
        check(lib().acx_profile_read(self._h, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(KERNEL_CLASSES)}


class Resampler:
    """Owns one acx_resampler: the band tables of orig_hz -> new_hz on one GPU (include/acx.h, acx_resample)."""

    def __init__(self, device_index, orig_hz, new_hz):
        self._h = _vp()
        check(lib().acx_resampler_create(int(device_index), int(orig_hz), int(new_hz), ctypes.byref(self._h)))
        self.device_index, self.orig_hz, self.new_hz = int(device_index), int(orig_hz), int(new_hz)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().acx_resampler_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def run(self, wav, lengths, out):
        """wav: packed fp32 device tensor of the clips, lengths: <= MAX_VARLEN_CLIPS ints, out: packed output tensor."""
        lens = (_c_i64 * len(lengths))(*[int(n) for n in lengths])
        check(lib().acx_resample(self._h, ptr(wav), lens, len(lengths), ptr(out), stream_ptr(wav.device)))


def resample_plan(orig_hz, new_hz):
    """acx_test_resample_plan -> AcxResamplePlan: geometry, tile form and grid cap of orig_hz -> new_hz (host only)."""
    plan = AcxResamplePlan()
    check(lib().acx_test_resample_plan(int(orig_hz), int(new_hz), ctypes.byref(plan)))
    return plan


def resample_geometry(orig_hz, new_hz):
    """(of, nf, width, max_band) of orig_hz -> new_hz (acx_resample_geometry; host only)."""
    v = [_c_int() for _ in range(4)]
    check(lib().acx_resample_geometry(int(orig_hz), int(new_hz), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def resample_taps(orig_hz, new_hz):
    """(band_start[nf], band_count[nf], taps) as lists: the stored taps of each phase, phase after phase (acx_resample_taps)."""
    _, nf, _, mb = resample_geometry(orig_hz, new_hz)
    start, count = (_c_int * nf)(), (_c_int * nf)()
    taps = (ctypes.c_float * max(1, nf * mb))()
    check(lib().acx_resample_taps(int(orig_hz), int(new_hz), start, count, taps, nf * mb))
    n = sum(count)
    return list(start), list(count), list(taps[:n])


def resampled_length(orig_hz, new_hz, L):
    return _query(lib().acx_resampled_length, _c_i64, int(orig_hz), int(new_hz), int(L))


def window_count(lengths, window, hop):
    """Windows of `window` samples every `hop` samples over recordings of `lengths` samples (acx_window_count; host only)."""
    lens = (_c_i64 * max(1, len(lengths)))(*[int(n) for n in lengths])
    return _query(lib().acx_window_count, _c_i64, lens, len(lengths), int(window), int(hop))


TARGET_F32, TARGET_U8 = 0, 1                 # enum acx_target_dtype
METRICS_NONFINITE, METRICS_BAD_TARGET = 1, 2  # bits of acx_tagging_metrics' status word
METRICS_BAD_THRESHOLD = 4                     # acx_threshold_counts: a NaN threshold
METRICS_BAD_WEIGHT = 8                        # acx_weighted_metrics: a negative weight, or a weight vector summing above 2^30
OP_FBETA, OP_PRECISION, OP_RECALL = 0, 1, 2   # enum acx_operating_criterion
WEIGHTED_MAX_N = 32768                        # acx_weighted_metrics: rows per class (one LDS bucket each)


def metrics_workspace_bytes(n, classes):
    """Workspace of acx_tagging_metrics for n rows of `classes` scores (host only)."""
    return _query(lib().acx_metrics_workspace_bytes, _c_sz, int(n), int(classes))


def tagging_metrics(scores, ld_scores, target, target_dtype, ld_target, n, classes, ap, auc, dprime, status, ws, stream):
    """acx_tagging_metrics on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_tagging_metrics(scores, int(ld_scores), target, int(target_dtype), int(ld_target), int(n), int(classes), ap,
                                    auc, dprime, status, ws[0], int(ws[1]), stream))


def operating_points(scores, ld_scores, target, target_dtype, ld_target, n, classes, criterion, param, thresholds, counts, status,
                     ws, stream):
    """acx_operating_points on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes) of metrics_workspace_bytes."""
    spec = AcxOperatingSpec(int(criterion), float(param))
    check(lib().acx_operating_points(scores, int(ld_scores), target, int(target_dtype), int(ld_target), int(n), int(classes),
                                     ctypes.byref(spec), thresholds, counts, status, ws[0], int(ws[1]), stream))


def threshold_counts(scores, ld_scores, target, target_dtype, ld_target, n, classes, thresholds, counts, status, stream):
    """acx_threshold_counts on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_threshold_counts(scores, int(ld_scores), target, int(target_dtype), int(ld_target), int(n), int(classes),
                                     thresholds, counts, status, stream))


def bootstrap_weights(seed, first_replicate, replicates, n, weights, ld_w, stream):
    """acx_bootstrap_weights on a raw device pointer (ctypes.c_void_p)."""
    check(lib().acx_bootstrap_weights(int(seed), int(first_replicate), int(replicates), int(n), weights, int(ld_w), stream))


def weighted_metrics_workspace_bytes(n, classes):
    """Workspace of acx_weighted_metrics for n rows of `classes` scores (host only)."""
    return _query(lib().acx_weighted_metrics_workspace_bytes, _c_sz, int(n), int(classes))


def weighted_metrics(scores, ld_scores, target, target_dtype, ld_target, n, classes, weights, ld_w, replicates, ap, auc, dprime,
                     status, ws, stream):
    """acx_weighted_metrics on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_weighted_metrics(scores, int(ld_scores), target, int(target_dtype), int(ld_target), int(n), int(classes),
                                     weights, int(ld_w), int(replicates), ap, auc, dprime, status, ws[0], int(ws[1]), stream))


RANK_N_POS, RANK_COVERAGE, RANK_BAD_PAIRS, RANK_HITS = 0, 1, 2, 3     # enum acx_ranking_count: the columns of row_counts
RANK_COUNTS = 4                               # ACX_RANK_COUNTS
RANK_WAVE_MAX_CLASSES = 1024                  # ACX_RANK_WAVE_MAX_CLASSES: up to here a wave ranks a row, beyond a workgroup


def ranking_workspace_bytes(rows, classes, slice_rows=0):
    """Workspace of acx_ranking_metrics for `rows` rows of `classes` scores in slices of slice_rows (0: the default; host only)."""
    return _query(lib().acx_ranking_workspace_bytes, _c_sz, int(rows), int(classes), int(slice_rows))


def ranking_metrics(scores, ld_s, target, target_dtype, ld_t, rows, classes, k, slice_rows, row_counts, row_psum, class_count,
                    class_psum, status, ws, stream):
    """acx_ranking_metrics on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes) of ranking_workspace_bytes."""
    check(lib().acx_ranking_metrics(scores, int(ld_s), target, int(target_dtype), int(ld_t), int(rows), int(classes), int(k),
                                    int(slice_rows), row_counts, row_psum, class_count, class_psum, status, ws[0], int(ws[1]),
                                    stream))


FIT_BAD_INDEX = 1                              # bit of the status word of acx_head_fit_step / acx_head_fit_grad


def adam(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, amsgrad=True, decoupled=False):
    """An acx_adam struct (the defaults are the reference's fine-tuning settings)."""
    return AcxAdam(float(beta1), float(beta2), float(eps), float(weight_decay), 1 if amsgrad else 0, 1 if decoupled else 0)


def head_fit_workspace_bytes(rows_max, classes):
    """Workspace of acx_head_fit_step / acx_head_fit_grad for steps of up to rows_max rows (host only)."""
    return _query(lib().acx_head_fit_workspace_bytes, _c_sz, int(rows_max), int(classes))


FIT_BAD_LABEL = 2                              # acx_head_fit_step_ce / acx_head_fit_grad_ce: a label outside [0, classes)


def head_fit_ce_workspace_bytes(rows_max, classes):
    """Workspace of acx_head_fit_step_ce / acx_head_fit_grad_ce for steps of up to rows_max rows (host only)."""
    return _query(lib().acx_head_fit_ce_workspace_bytes, _c_sz, int(rows_max), int(classes))


FIT_BAD_BAG = 4                                # acx_head_fit_step_mil / acx_head_fit_grad_mil / acx_segment_pool: a bad bag_off entry
FIT_MAX_ROWS = 1 << 22                         # rows (segment rows, bags) of one step
MIL_MAX, MIL_MEAN, MIL_LINEAR, MIL_EXP = 0, 1, 2, 3     # enum acx_mil_pool


def head_fit_mil_workspace_bytes(seg_rows_max, bags_max, classes):
    """Workspace of acx_head_fit_step_mil / acx_head_fit_grad_mil for steps of up to seg_rows_max rows in bags_max bags (host only)."""
    return _query(lib().acx_head_fit_mil_workspace_bytes, _c_sz, int(seg_rows_max), int(bags_max), int(classes))


def segment_pool(logits, ld, bag_off, bags, classes, pool, out, status, stream):
    """acx_segment_pool on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_segment_pool(logits, int(ld), bag_off, int(bags), int(classes), int(pool), out, status, stream))


FIT_MAX_JOBS = 256                             # ACX_FIT_MAX_JOBS: jobs of one acx_head_fit_group_step
FIT_LOSS_BCE, FIT_LOSS_CE = 0, 1               # enum acx_fit_loss


def head_fit_group_workspace_bytes(jobs, rows_max, classes, loss):
    """Workspace of acx_head_fit_group_step / _step_ce for `jobs` jobs of up to rows_max rows a step (host only)."""
    return _query(lib().acx_head_fit_group_workspace_bytes, _c_sz, int(jobs), int(rows_max), int(classes), int(loss))


def head_fit_plan(rows, idx_offset, lr, hps, rows_max, classes, loss):
    """The plan of a group fit (acx_head_fit_plan_fill, host only): rows / idx_offset / lr are (steps, jobs) arrays, hps one
    AcxAdam per job.  -> a uint8 numpy array to upload once."""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    steps, jobs = rows.shape
    idx_offset = np.ascontiguousarray(idx_offset, dtype=np.int64)
    lr = np.ascontiguousarray(lr, dtype=np.float64)
    if idx_offset.shape != rows.shape or lr.shape != rows.shape or len(hps) != jobs:
        raise ValueError("rows, idx_offset and lr must share one (steps, jobs) shape, with one hp per job")
    plan = np.zeros(_query(lib().acx_head_fit_plan_bytes, _c_sz, jobs, steps), dtype=np.uint8)
    check(lib().acx_head_fit_plan_fill(jobs, steps, int(rows_max), int(classes), int(loss), rows.ctypes.data, idx_offset.ctypes.data,
                                       (AcxAdam * jobs)(*hps), lr.ctypes.data, plan.ctypes.data, plan.nbytes))
    return plan


CLASSIFY_MAX_K = 64                            # ACX_CLASSIFY_MAX_K
CLASSIFY_NONFINITE, CLASSIFY_BAD_LABEL = 1, 2  # bits of the status words of acx_softmax_topk / acx_classification_counts
CLASSIFY_MAX_CONFUSION = 4096                  # widest head acx_classification_counts fills a confusion matrix for
SOFT_WAVE_MAX_N = 2048                         # rows up to this many classes are summed by one wave, wider ones by a workgroup


def softmax_depth(classes):
    """Depth of the fp32 row sum of the softmax kernels (include/acx.h): additions between an element and the sum."""
    classes = int(classes)
    return -(-classes // 64) + 6 if classes <= SOFT_WAVE_MAX_N else -(-classes // 256) + 9


def softmax_topk(logits, ld, rows, classes, k, probs, ld_p, top_index, top_prob, status, stream):
    """acx_softmax_topk on raw device pointers (ctypes.c_void_p); probs may be None."""
    check(lib().acx_softmax_topk(logits, int(ld), int(rows), int(classes), int(k), probs, int(ld_p), top_index, top_prob, status,
                                 stream))


def classification_counts(logits, ld, labels, n, classes, k, per_class, hits, confusion, status, stream):
    """acx_classification_counts on raw device pointers (ctypes.c_void_p); confusion may be None."""
    check(lib().acx_classification_counts(logits, int(ld), labels, int(n), int(classes), int(k), per_class, hits, confusion,
                                          status, stream))


CAL_MAX_BINS, CAL_MAX_EVALUATIONS = 64, 64     # ACX_CAL_MAX_BINS, ACX_CAL_MAX_EVALUATIONS
CAL_NONFINITE, CAL_BAD_TARGET, CAL_BAD_PROBABILITY, CAL_BAD_LABEL = 1, 2, 4, 8   # bits of the calibration calls' status words
CAL_DEGENERATE, CAL_NOT_CONVERGED, CAL_AT_BOUND = -1, -2, -3                     # negative values of their info words


def reliability_counts(probs, ld, target, target_dtype, ld_t, n, classes, bins, count, positive, conf_sum, brier_sum, status,
                       stream):
    """acx_reliability_counts on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_reliability_counts(probs, int(ld), target, int(target_dtype), int(ld_t), int(n), int(classes), int(bins),
                                       count, positive, conf_sum, brier_sum, status, stream))


def reliability_toplabel(logits, ld, labels, n, classes, beta, bins, count, correct, conf_sum, nll_sum, status, ws, stream):
    """acx_reliability_toplabel on raw device pointers; beta may be None; ws: (pointer, bytes) of temperature_workspace_bytes."""
    check(lib().acx_reliability_toplabel(logits, int(ld), labels, int(n), int(classes), beta, int(bins), count, correct, conf_sum,
                                         nll_sum, status, ws[0], int(ws[1]), stream))


def platt_workspace_bytes(n, classes):
    """Workspace of acx_platt_fit for n rows of `classes` logits (host only)."""
    return _query(lib().acx_platt_workspace_bytes, _c_sz, int(n), int(classes))


def platt_fit(logits, ld, target, target_dtype, ld_t, n, classes, smooth, ab, info, status, ws, stream):
    """acx_platt_fit on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_platt_fit(logits, int(ld), target, int(target_dtype), int(ld_t), int(n), int(classes), 1 if smooth else 0, ab,
                              info, status, ws[0], int(ws[1]), stream))


def platt_apply(logits, ld, rows, classes, ab, probs, ld_p, stream):
    """acx_platt_apply on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_platt_apply(logits, int(ld), int(rows), int(classes), ab, probs, int(ld_p), stream))


def temperature_workspace_bytes(n, classes):
    """Workspace of acx_temperature_fit and acx_reliability_toplabel for n rows of `classes` logits (host only)."""
    return _query(lib().acx_temperature_workspace_bytes, _c_sz, int(n), int(classes))


def temperature_fit(logits, ld, labels, n, classes, evaluations, beta, info, status, ws, stream):
    """acx_temperature_fit on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_temperature_fit(logits, int(ld), labels, int(n), int(classes), int(evaluations), beta, info, status, ws[0],
                                    int(ws[1]), stream))


def temperature_apply(logits, ld, rows, classes, beta, out, ld_o, stream):
    """acx_temperature_apply on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_temperature_apply(logits, int(ld), int(rows), int(classes), beta, out, int(ld_o), stream))


KNN_DOT, KNN_COSINE = 0, 1                    # enum acx_knn_metric
KNN_UNIFORM, KNN_SIMILARITY = 0, 1            # enum acx_knn_weighting
KNN_MAX_K, KNN_MAX_DIM = 128, 4096            # ACX_KNN_MAX_K, ACX_KNN_MAX_DIM
KNN_NONFINITE, KNN_BAD_INDEX = 1, 2           # bits of the status words of acx_knn_search / acx_knn_row_norms and acx_knn_vote
KNN_METRICS = {"dot": KNN_DOT, "cosine": KNN_COSINE}
KNN_WEIGHTS = {"uniform": KNN_UNIFORM, "similarity": KNN_SIMILARITY}


def knn_workspace_bytes(nq, n, k):
    """Workspace of acx_knn_search for nq queries, n database rows and k neighbours (host only)."""
    return _query(lib().acx_knn_workspace_bytes, _c_sz, int(nq), int(n), int(k))


def knn_slices(nq, n, k):
    """Slices of the database rows a search of this shape runs as (acx_knn_slices; host only)."""
    return _query(lib().acx_knn_slices, _c_int, int(nq), int(n), int(k))


def knn_row_norms(x, ld, n, dim, inv_norm, status, stream):
    """acx_knn_row_norms on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_knn_row_norms(x, int(ld), int(n), int(dim), inv_norm, status, stream))


def knn_search(q, ld_q, q_inv_norm, nq, d, ld_d, d_inv_norm, n, dim, metric, k, exclude, indices, scores, status, ws, stream):
    """acx_knn_search on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_knn_search(q, int(ld_q), q_inv_norm, int(nq), d, int(ld_d), d_inv_norm, int(n), int(dim), int(metric), int(k),
                               exclude, indices, scores, status, ws[0], int(ws[1]), stream))


def knn_vote(indices, scores, nq, k, target, target_dtype, ld_target, n, classes, weighting, temperature, out, ld_out, status,
             stream):
    """acx_knn_vote on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_knn_vote(indices, scores, int(nq), int(k), target, int(target_dtype), int(ld_target), int(n), int(classes),
                             int(weighting), float(temperature), out, int(ld_out), status, stream))


KNN_I8_K = 32                                 # ACX_KNN_I8_K: int8 code rows are padded to a multiple


def knn_quantize_i8(x, ld, inv_norm, n, dim, codes, ld_c, scale, status, stream):
    """acx_knn_quantize_i8 on raw device pointers (ctypes.c_void_p); inv_norm None: the dot metric."""
    check(lib().acx_knn_quantize_i8(x, int(ld), inv_norm, int(n), int(dim), codes, int(ld_c), scale, status, stream))


def knn_search_i8(cq, ld_cq, sq, nq, cd, ld_cd, sd, n, dim, k, exclude, indices, scores, status, ws, stream):
    """acx_knn_search_i8 on raw device pointers (ctypes.c_void_p); dim: the padded code width; ws: (pointer, bytes)."""
    check(lib().acx_knn_search_i8(cq, int(ld_cq), sq, int(nq), cd, int(ld_cd), sd, int(n), int(dim), int(k), exclude, indices, scores,
                                  status, ws[0], int(ws[1]), stream))


def knn_rescore(q, ld_q, q_inv_norm, nq, d, ld_d, d_inv_norm, n, dim, metric, cand, ld_cand, kc, k, indices, scores, status, stream):
    """acx_knn_rescore on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_knn_rescore(q, int(ld_q), q_inv_norm, int(nq), d, int(ld_d), d_inv_norm, int(n), int(dim), int(metric), cand,
                                int(ld_cand), int(kc), int(k), indices, scores, status, stream))


KMEANS_EUCLIDEAN, KMEANS_COSINE = 0, 1         # enum acx_kmeans_metric
KMEANS_METRICS = {"euclidean": KMEANS_EUCLIDEAN, "cosine": KMEANS_COSINE}
KMEANS_MAX_CLUSTERS, KMEANS_MAX_ITER = 4096, 1000      # ACX_KMEANS_MAX_CLUSTERS, ACX_KMEANS_MAX_ITER
KMEANS_NONFINITE, KMEANS_DEGENERATE, KMEANS_BAD_LABEL = 1, 2, 4    # bits of the status words of the acx_kmeans_* calls
KMEANS_SAMPLE_WORKSPACE = 8192                 # bytes of workspace acx_kmeans_sample needs


class AcxKmeansState(ctypes.Structure):
    """struct acx_kmeans_state: the device-side state of acx_kmeans_fit (32 bytes)."""
    _fields_ = [("iterations", ctypes.c_int32), ("done", ctypes.c_int32), ("changed", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("shift", ctypes.c_double), ("inertia", ctypes.c_double)]


KMEANS_STATE_BYTES = ctypes.sizeof(AcxKmeansState)     # 32


def kmeans_workspace_bytes(n, dim, clusters):
    """Workspace of acx_kmeans_fit / acx_kmeans_update / acx_kmeans_seed (host only)."""
    return _query(lib().acx_kmeans_workspace_bytes, _c_sz, int(n), int(dim), int(clusters))


def kmeans_assign(x, ld_x, x_inv_norm, n, centers, ld_c, clusters, dim, metric, prev_labels, labels, scores, changed, status,
                  stream):
    """acx_kmeans_assign on raw device pointers (ctypes.c_void_p); prev_labels may be None."""
    check(lib().acx_kmeans_assign(x, int(ld_x), x_inv_norm, int(n), centers, int(ld_c), int(clusters), int(dim), int(metric),
                                  prev_labels, labels, scores, changed, status, stream))


def kmeans_update(x, ld_x, x_inv_norm, n, dim, metric, labels, clusters, centers, ld_c, counts, shift, status, ws, stream):
    """acx_kmeans_update on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_kmeans_update(x, int(ld_x), x_inv_norm, int(n), int(dim), int(metric), labels, int(clusters), centers,
                                  int(ld_c), counts, shift, status, ws[0], int(ws[1]), stream))


def kmeans_fit(x, ld_x, x_inv_norm, n, dim, metric, centers, ld_c, clusters, max_iter, tol_abs, labels, counts, state, status, ws,
               stream):
    """acx_kmeans_fit on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_kmeans_fit(x, int(ld_x), x_inv_norm, int(n), int(dim), int(metric), centers, int(ld_c), int(clusters),
                               int(max_iter), tol_abs, labels, counts, state, status, ws[0], int(ws[1]), stream))


def kmeans_min_distance(x, ld_x, x_inv_norm, n, dim, metric, center, first, d, d_max, status, stream):
    """acx_kmeans_min_distance on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_kmeans_min_distance(x, int(ld_x), x_inv_norm, int(n), int(dim), int(metric), center, 1 if first else 0, d,
                                        d_max, status, stream))


def kmeans_sample(d, n, d_max, u, picked, status, ws, stream):
    """acx_kmeans_sample on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_kmeans_sample(d, int(n), d_max, u, picked, status, ws[0], int(ws[1]), stream))


def kmeans_seed(x, ld_x, x_inv_norm, n, dim, metric, clusters, u, picked, centers, ld_c, status, ws, stream):
    """acx_kmeans_seed on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_kmeans_seed(x, int(ld_x), x_inv_norm, int(n), int(dim), int(metric), int(clusters), u, picked, centers,
                                int(ld_c), status, ws[0], int(ws[1]), stream))


GMM_DIAG, GMM_SPHERICAL = 0, 1                 # enum acx_gmm_covariance
GMM_COVARIANCES = {"diag": GMM_DIAG, "spherical": GMM_SPHERICAL}
GMM_NONFINITE, GMM_DEGENERATE = 1, 2           # bits of the status words of the acx_gmm_* calls


class AcxGmmState(ctypes.Structure):
    """struct acx_gmm_state: the device-side state of acx_gmm_fit (32 bytes)."""
    _fields_ = [("iterations", ctypes.c_int32), ("done", ctypes.c_int32), ("converged", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("lower_bound", ctypes.c_double), ("change", ctypes.c_double)]


GMM_STATE_BYTES = ctypes.sizeof(AcxGmmState)           # 32


def gmm_workspace_bytes(n, dim, components):
    """Workspace of every acx_gmm_* call (host only)."""
    return _query(lib().acx_gmm_workspace_bytes, _c_sz, int(n), int(dim), int(components))


def gmm_estep(x, ld_x, n, dim, center, weights, means, variances, components, covariance_type, log_prob_norm, resp, ld_resp, labels,
              log_prob_sum, status, ws, stream):
    """acx_gmm_estep on raw device pointers (ctypes.c_void_p); center, resp and labels may be None; ws: (pointer, bytes)."""
    check(lib().acx_gmm_estep(x, int(ld_x), int(n), int(dim), center, weights, means, variances, int(components), int(covariance_type),
                              log_prob_norm, resp, int(ld_resp), labels, log_prob_sum, status, ws[0], int(ws[1]), stream))


def gmm_score(x, ld_x, n, dim, center, weights, means, variances, components, covariance_type, log_prob_norm, labels, log_prob_sum,
              status, ws, stream):
    """acx_gmm_score on raw device pointers (ctypes.c_void_p); center and labels may be None; ws: (pointer, bytes)."""
    check(lib().acx_gmm_score(x, int(ld_x), int(n), int(dim), center, weights, means, variances, int(components), int(covariance_type),
                              log_prob_norm, labels, log_prob_sum, status, ws[0], int(ws[1]), stream))


def gmm_mstep(x, ld_x, n, dim, center, resp, ld_resp, components, reg_covar, covariance_type, weights, means, variances, nk, status, ws,
              stream):
    """acx_gmm_mstep on raw device pointers (ctypes.c_void_p); center may be None; ws: (pointer, bytes)."""
    check(lib().acx_gmm_mstep(x, int(ld_x), int(n), int(dim), center, resp, int(ld_resp), int(components), float(reg_covar),
                              int(covariance_type), weights, means, variances, nk, status, ws[0], int(ws[1]), stream))


def gmm_fit(x, ld_x, n, dim, weights, means, variances, components, covariance_type, max_iter, tol, reg_covar, center, labels,
            log_prob_norm, state, status, ws, stream):
    """acx_gmm_fit on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_gmm_fit(x, int(ld_x), int(n), int(dim), weights, means, variances, int(components), int(covariance_type),
                            int(max_iter), tol, float(reg_covar), center, labels, log_prob_norm, state, status, ws[0], int(ws[1]),
                            stream))


# bits of the status words of acx_silhouette / acx_cluster_dispersion / acx_contingency
CLUSTER_NONFINITE, CLUSTER_DEGENERATE, CLUSTER_BAD_LABEL, CLUSTER_BAD_ROW = 1, 2, 4, 8
CLUSTER_MAX_SPLITS = 16                        # ACX_CLUSTER_MAX_SPLITS
CONTINGENCY_MAX_CELLS = 1 << 24                # ACX_CONTINGENCY_MAX_CELLS


def cluster_scores_workspace_bytes(n, dim, clusters):
    """Workspace of acx_silhouette / acx_cluster_dispersion (host only)."""
    return _query(lib().acx_cluster_scores_workspace_bytes, _c_sz, int(n), int(dim), int(clusters))


def silhouette(x, ld_x, x_inv_norm, n, dim, metric, labels, clusters, rows, n_rows, a, b, nearest, s, cluster_mean, mean, status, ws,
               stream):
    """acx_silhouette on raw device pointers (ctypes.c_void_p); rows and cluster_mean may be None; ws: (pointer, bytes)."""
    check(lib().acx_silhouette(x, int(ld_x), x_inv_norm, int(n), int(dim), int(metric), labels, int(clusters), rows, int(n_rows), a, b,
                               nearest, s, cluster_mean, mean, status, ws[0], int(ws[1]), stream))


def cluster_dispersion(x, ld_x, n, dim, labels, clusters, counts, means, within_sq, within_dist, grand_mean, status, ws, stream):
    """acx_cluster_dispersion on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_cluster_dispersion(x, int(ld_x), int(n), int(dim), labels, int(clusters), counts, means, within_sq, within_dist,
                                       grand_mean, status, ws[0], int(ws[1]), stream))


def contingency(a, ka, b, kb, n, table, status, stream):
    """acx_contingency on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_contingency(a, int(ka), b, int(kb), int(n), table, status, stream))


# ---- radius search, components, DBSCAN (acx_radius_*, acx_graph_components, acx_dbscan_labels) ---------------------------------
RADIUS_DOT, RADIUS_COSINE, RADIUS_EUCLIDEAN = 0, 1, 2          # enum acx_radius_metric
RADIUS_METRICS = {"dot": RADIUS_DOT, "cosine": RADIUS_COSINE, "euclidean": RADIUS_EUCLIDEAN}
RADIUS_SELF_NONE, RADIUS_SELF_EXCLUDE, RADIUS_SELF_INCLUDE = 0, 1, 2     # enum acx_radius_self
# bits of the status words of the acx_radius_* / acx_graph_components / acx_dbscan_labels calls
RADIUS_NONFINITE, RADIUS_OVERFLOW, GRAPH_BAD_INDEX, GRAPH_NOT_CONVERGED = 1, 2, 4, 8
RADIUS_MAX_SLICES = 64                         # ACX_RADIUS_MAX_SLICES
GRAPH_MAX_ROUNDS = 4096                        # ACX_GRAPH_MAX_ROUNDS


def radius_workspace_bytes(nq, n, slices=0):
    """Workspace of acx_radius_count (slices = 0) / acx_radius_neighbors (host only)."""
    return _query(lib().acx_radius_workspace_bytes, _c_sz, int(nq), int(n), int(slices))


def radius_slices(nq, n, slices=0):
    """The ranges of database rows acx_radius_count / acx_radius_neighbors cut (host only)."""
    return _query(lib().acx_radius_slices, _c_int, int(nq), int(n), int(slices))


def radius_row_sumsq(x, ld, n, dim, xx, stream):
    """acx_radius_row_sumsq on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_radius_row_sumsq(x, int(ld), int(n), int(dim), xx, stream))


def radius_count(q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, counts, status, ws, stream):
    """acx_radius_count on raw device pointers (ctypes.c_void_p); aux None for the dot metric; ws: (pointer, bytes)."""
    check(lib().acx_radius_count(q, int(ld_q), q_aux, int(nq), d, int(ld_d), d_aux, int(n), int(dim), int(metric), float(level),
                                 int(self_mode), counts, status, ws[0], int(ws[1]), stream))


def radius_neighbors(q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, slices, offsets, indices, values, capacity,
                     total, status, ws, stream):
    """acx_radius_neighbors on raw device pointers (ctypes.c_void_p); values may be None; ws: (pointer, bytes)."""
    check(lib().acx_radius_neighbors(q, int(ld_q), q_aux, int(nq), d, int(ld_d), d_aux, int(n), int(dim), int(metric), float(level),
                                     int(self_mode), int(slices), offsets, indices, values, int(capacity), total, status, ws[0],
                                     int(ws[1]), stream))


def radius_emit(q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, slices, offsets, indices, values, capacity, total,
                status, ws, stream):
    """acx_radius_emit on raw device pointers (ctypes.c_void_p): the emit pass on the workspace an acx_radius_neighbors call left."""
    check(lib().acx_radius_emit(q, int(ld_q), q_aux, int(nq), d, int(ld_d), d_aux, int(n), int(dim), int(metric), float(level),
                                int(self_mode), int(slices), offsets, indices, values, int(capacity), total, status, ws[0], int(ws[1]),
                                stream))


def graph_components(offsets, indices, n, labels, status, max_rounds, resume, stream):
    """acx_graph_components on raw device pointers (ctypes.c_void_p)."""
    check(lib().acx_graph_components(offsets, indices, int(n), labels, status, int(max_rounds), 1 if resume else 0, stream))


def dbscan_workspace_bytes(n):
    """Workspace of acx_dbscan_labels (host only)."""
    return _query(lib().acx_dbscan_workspace_bytes, _c_sz, int(n))


def dbscan_labels(offsets, indices, n, min_samples, labels, core, clusters, status, ws, max_rounds, stream):
    """acx_dbscan_labels on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_dbscan_labels(offsets, indices, int(n), int(min_samples), labels, core, clusters, status, ws[0], int(ws[1]),
                                  int(max_rounds), stream))


MAX_EVENT_MEDIAN = 101                        # ACX_MAX_EVENT_MEDIAN
EVENTS_NONFINITE, EVENTS_OVERFLOW = 1, 2      # bits of acx_decode_events' status word
EVENTS_BAD_THRESHOLD = 4                      # the _classwise calls: a class with !(0 <= low <= threshold)
EVENT_BYTES = ctypes.sizeof(AcxEvent)         # 32


# ---- embedding statistics (acx_moments, acx_gram_f64, acx_eigh, acx_pca_*) ---------------------------------------------------
STATS_MAX_DIM = 1024                           # ACX_STATS_MAX_DIM
EIGH_MAX_SWEEPS = 64                           # ACX_EIGH_MAX_SWEEPS
STATS_NONFINITE, STATS_NOT_CONVERGED, STATS_DEGENERATE = 1, 2, 4    # bits of the status words of acx_moments / acx_eigh


class AcxEighState(ctypes.Structure):
    """struct acx_eigh_state: the device-side state of acx_eigh (16 bytes)."""
    _fields_ = [("sweeps", ctypes.c_int32), ("done", ctypes.c_int32), ("rotations", ctypes.c_int64)]


def moments_workspace_bytes(n, dim):
    """Workspace of acx_moments (host only; a function of n, dim and ACX_MOMENTS_SLICE_ROWS)."""
    return _query(lib().acx_moments_workspace_bytes, _c_sz, int(n), int(dim))


def moments(x, ld_x, n, dim, ddof, mean, cov, ld_c, status, ws, stream):
    """acx_moments on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_moments(x, int(ld_x), int(n), int(dim), int(ddof), mean, cov, int(ld_c), status, ws[0], int(ws[1]), stream))


def gram_f64(a, ld_a, b, ld_b, rows, m, n, out, ld_o, stream):
    """acx_gram_f64 on raw device pointers (ctypes.c_void_p): out (m, n) = a^T b."""
    check(lib().acx_gram_f64(a, int(ld_a), b, int(ld_b), int(rows), int(m), int(n), out, int(ld_o), stream))


def eigh_workspace_bytes(dim):
    """Workspace of acx_eigh (host only)."""
    return _query(lib().acx_eigh_workspace_bytes, _c_sz, int(dim))


def eigh(a, ld_a, dim, max_sweeps, values, vectors, ld_v, state, status, ws, stream):
    """acx_eigh on raw device pointers (ctypes.c_void_p); ws: (pointer, bytes)."""
    check(lib().acx_eigh(a, int(ld_a), int(dim), int(max_sweeps), values, vectors, int(ld_v), state, status, ws[0], int(ws[1]),
                         stream))


def pca_transform(x, ld_x, n, dim, mean, w, ld_w, k, scale, out, ld_o, stream):
    """acx_pca_transform on raw device pointers (ctypes.c_void_p); scale may be None."""
    check(lib().acx_pca_transform(x, int(ld_x), int(n), int(dim), mean, w, int(ld_w), int(k), scale, out, int(ld_o), stream))


def pca_inverse(z, ld_z, n, k, scale, w, ld_w, dim, mean, out, ld_o, stream):
    """acx_pca_inverse on raw device pointers (ctypes.c_void_p); scale may be None."""
    check(lib().acx_pca_inverse(z, int(ld_z), int(n), int(k), scale, w, int(ld_w), int(dim), mean, out, int(ld_o), stream))


def event_params(threshold=0.5, low=None, median=1, min_duration=0.0, merge_gap=0.0):
    """An acx_event_params struct (decode_events' defaults: low=None means low = threshold).  threshold and low are rounded
    to fp32 here, as numpy rounds a Python float compared with a float32 array."""
    return AcxEventParams(float(threshold), float(threshold if low is None else low), int(median), float(min_duration),
                          float(merge_gap))


def events_workspace_bytes(B, N):
    """Workspace of acx_decode_events / acx_decode_events_varlen for B clips of N classes (host only)."""
    return _query(lib().acx_events_workspace_bytes, _c_sz, int(B), int(N))


def event_stream_bytes(slots, N, median):
    """Device state of an acx_event_stream handle of `slots` recordings of N classes (host only)."""
    return _query(lib().acx_event_stream_bytes, _c_sz, int(slots), int(N), int(median))


SCORE_BAD_TABLE = 1                           # bit of the status word of acx_score_events / acx_score_segments / acx_score_intersection
REF_EVENT_BYTES = ctypes.sizeof(AcxRefEvent)  # 24
SCORE_TILE_SEGMENTS = 2048                    # ACX_SCORE_TILE_SEGMENTS


def event_collar(t_collar=0.2, percentage_of_length=0.5, evaluate_onset=True, evaluate_offset=True):
    """An acx_event_collar struct (sed_eval's defaults)."""
    return AcxEventCollar(float(t_collar), float(percentage_of_length), 1 if evaluate_onset else 0, 1 if evaluate_offset else 0)


def intersection_criteria(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None):
    """An acx_intersection_criteria struct; cttc_threshold None: no cross-trigger matrix."""
    return AcxIntersectionCriteria(float(dtc_threshold), float(gtc_threshold), 0.0 if cttc_threshold is None else float(cttc_threshold),
                                   0 if cttc_threshold is None else 1, 0)


def segment_count(L):
    """S, the segments of a clip of L samples (acx_segment_count; host only)."""
    return _query(lib().acx_segment_count, _c_int, int(L))


def stage_hw(L, stage):
    h, w = _c_int(), _c_int()
    check(lib().acx_stage_hw(int(L), int(stage), ctypes.byref(h), ctypes.byref(w)))
    return h.value, w.value


def num_frames(L):
    return _query(lib().acx_num_frames, _c_int, int(L))


def stream_schedule(window, hop, orig_hz, pushed, closed):
    """(final 32 kHz samples, windows, timeline rows) emitted so far by one slot of a live stream (acx_stream_schedule; host
    only): `pushed` input samples at orig_hz, the recording open or closed."""
    v = [_c_i64(), _c_i64(), _c_i64()]
    check(lib().acx_stream_schedule(int(window), int(hop), int(orig_hz), int(pushed), 1 if closed else 0,
                                    *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def stream_geometry(window, hop, orig_hz, max_push, timeline):
    """(adv, C, Ch, Hw): the per-slot sizes acx_stream_create derives from its arguments (acx_stream_geometry; host only)."""
    v = [_c_i64() for _ in range(4)]
    check(lib().acx_stream_geometry(int(window), int(hop), int(orig_hz), int(max_push), 1 if timeline else 0,
                                    *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)
