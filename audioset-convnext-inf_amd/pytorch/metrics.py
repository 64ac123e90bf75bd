"""Per-class AudioSet statistics on the GPU (acx_tagging_metrics in include/acx.h): the average precision, ROC-AUC and d' of
`evaluate.calculate_statistics` -- sklearn 1.7.2 average_precision_score / roc_auc_score with average=None and
sqrt(2) * scipy.stats.norm.ppf(auc) -- up to float64 rounding, from scores taken as float32.

    from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics
    stats = tagging_metrics(target, clipwise_output)      # {"average_precision", "auc", "d_prime"}: float64 (C,) arrays

CUDA tensors are read where they are, on the current stream (a column slice of a wider tensor too); numpy arrays and CPU tensors
are checked on the host, then copied to `device` (default: the current CUDA device), the targets as uint8.  A class with no
positive or no negative target gets AP 0 / 1 and NaN AUC and d', with one UserWarning, as sklearn does."""
import ctypes
import warnings

import numpy as np
import torch

from .. import _ffi


def _shape_check(target, scores):
    ts, ss = tuple(target.shape), tuple(scores.shape)
    if len(ts) != 2 or len(ss) != 2:
        raise ValueError("target and clipwise_output must be 2-D (clips, classes); got shapes %s and %s" % (ts, ss))
    if ts != ss:
        raise ValueError("target shape %s differs from clipwise_output shape %s" % (ts, ss))
    if ss[0] == 0:
        raise ValueError("no clips to score (N = 0)")
    if ss[1] == 0:
        raise ValueError("no classes to score (C = 0)")


def _host_scores(x):
    s = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
    if s.dtype == object or not (np.issubdtype(s.dtype, np.floating) or np.issubdtype(s.dtype, np.integer)
                                 or s.dtype == np.bool_):
        raise ValueError("clipwise_output must hold numbers (got dtype %s)" % s.dtype)
    with np.errstate(over="ignore"):                 # a float64 score beyond the float32 range becomes inf: rejected below
        s = np.ascontiguousarray(s, dtype=np.float32)
    if not np.isfinite(s).all():
        raise ValueError("clipwise_output holds NaN or infinite scores")
    return s


def _host_target(x):
    t = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
    if t.dtype == np.bool_:
        return np.ascontiguousarray(t.view(np.uint8))
    if t.dtype == object or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
        raise ValueError("target must hold 0 / 1 labels (got dtype %s)" % t.dtype)
    if not ((t == 0) | (t == 1)).all():
        raise ValueError("target holds values other than 0 and 1")
    return np.ascontiguousarray(t.astype(np.uint8))


def _device_scores(s):
    if s.dtype != torch.float32:
        s = s.to(torch.float32)
    if s.stride(1) != 1 or s.stride(0) < s.shape[1]:
        s = s.contiguous()
    return s


def _device_target(t):
    """-> (tensor, ACX_TARGET_*): float32 and uint8 / bool are read as they are, anything else travels as float32."""
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype not in (torch.uint8, torch.float32):
        t = t.to(torch.float32)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, (_ffi.TARGET_U8 if t.dtype == torch.uint8 else _ffi.TARGET_F32)


def tagging_metrics(target, clipwise_output, device=None):
    """{"average_precision", "auc", "d_prime"} of (N, C) targets and scores, each a float64 numpy array of shape (C,), computed
    on the GPU.  ValueError for shapes that are not 2-D or differ, N = 0, a NaN or infinite score, or a target other than 0 or 1
    (host inputs are checked before they are copied, device inputs through the kernel's status word)."""
    _shape_check(target, clipwise_output)
    s_dev = isinstance(clipwise_output, torch.Tensor) and clipwise_output.is_cuda
    t_dev = isinstance(target, torch.Tensor) and target.is_cuda
    # host inputs: checked here, before any copy or device call
    scores = _host_scores(clipwise_output) if not s_dev else None
    tgt = _host_target(target) if not t_dev else None
    if device is None:
        device = clipwise_output.device if s_dev else target.device if t_dev else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("tagging_metrics runs on a CUDA (HIP) device, not %s" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    scores = _device_scores(clipwise_output.to(device)) if s_dev else torch.from_numpy(scores).to(device)
    if t_dev:
        tgt, dtype = _device_target(target.to(device))
    else:
        tgt, dtype = torch.from_numpy(tgt).to(device), _ffi.TARGET_U8
    n, C = scores.shape
    ws_bytes = _ffi.metrics_workspace_bytes(n, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    out = torch.empty((3, C), dtype=torch.float64, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _ffi.tagging_metrics(vp(scores), scores.stride(0), vp(tgt), dtype, tgt.stride(0), n, C, vp(out[0]), vp(out[1]), vp(out[2]),
                         vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(device))
    res = out.cpu().numpy()
    st = int(status.cpu()[0])
    if st & _ffi.METRICS_NONFINITE:
        raise ValueError("clipwise_output holds NaN or infinite scores")
    if st & _ffi.METRICS_BAD_TARGET:
        raise ValueError("target holds values other than 0 and 1")
    ap, auc, dp = res[0].copy(), res[1].copy(), res[2].copy()
    undefined = np.isnan(auc)
    if undefined.any():
        no_pos = int((undefined & (ap == 0.0)).sum())
        warnings.warn("%d class(es) have no positive and %d no negative target: their average precision is %s and their ROC-AUC and "
                      "d-prime are NaN (sklearn warns and returns the same)" % (no_pos, int(undefined.sum()) - no_pos,
                                                                                 "0 / 1" if no_pos else "1"),
                      UserWarning, stacklevel=2)
    return {"average_precision": ap, "auc": auc, "d_prime": dp}
