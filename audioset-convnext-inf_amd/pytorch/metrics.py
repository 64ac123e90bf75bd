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


def _to_device(target, clipwise_output, device, who):
    """The checks and copies every call here starts with -> (scores, targets, ACX_TARGET_*, device): host inputs are checked
    before any copy or device call, CUDA tensors are taken where they are."""
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
        raise ValueError("%s runs on a CUDA (HIP) device, not %s" % (who, device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    scores = _device_scores(clipwise_output.to(device)) if s_dev else torch.from_numpy(scores).to(device)
    if t_dev:
        tgt, dtype = _device_target(target.to(device))
    else:
        tgt, dtype = torch.from_numpy(tgt).to(device), _ffi.TARGET_U8
    return scores, tgt, dtype, device


def _raise_status(st):
    if st & _ffi.METRICS_NONFINITE:
        raise ValueError("clipwise_output holds NaN or infinite scores")
    if st & _ffi.METRICS_BAD_TARGET:
        raise ValueError("target holds values other than 0 and 1")
    if st & _ffi.METRICS_BAD_THRESHOLD:
        raise ValueError("thresholds hold a NaN")


def tagging_metrics(target, clipwise_output, device=None):
    """{"average_precision", "auc", "d_prime"} of (N, C) targets and scores, each a float64 numpy array of shape (C,), computed
    on the GPU.  ValueError for shapes that are not 2-D or differ, N = 0, a NaN or infinite score, or a target other than 0 or 1
    (host inputs are checked before they are copied, device inputs through the kernel's status word)."""
    scores, tgt, dtype, device = _to_device(target, clipwise_output, device, "tagging_metrics")
    n, C = scores.shape
    ws_bytes = _ffi.metrics_workspace_bytes(n, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    out = torch.empty((3, C), dtype=torch.float64, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _ffi.tagging_metrics(vp(scores), scores.stride(0), vp(tgt), dtype, tgt.stride(0), n, C, vp(out[0]), vp(out[1]), vp(out[2]),
                         vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(device))
    res = out.cpu().numpy()
    _raise_status(int(status.cpu()[0]))
    ap, auc, dp = res[0].copy(), res[1].copy(), res[2].copy()
    undefined = np.isnan(auc)
    if undefined.any():
        no_pos = int((undefined & (ap == 0.0)).sum())
        warnings.warn("%d class(es) have no positive and %d no negative target: their average precision is %s and their ROC-AUC and "
                      "d-prime are NaN (sklearn warns and returns the same)" % (no_pos, int(undefined.sum()) - no_pos,
                                                                                 "0 / 1" if no_pos else "1"),
                      UserWarning, stacklevel=2)
    return {"average_precision": ap, "auc": auc, "d_prime": dp}


# ---- operating points ------------------------------------------------------------------------------------------------------

_CRITERIA = {"fbeta": _ffi.OP_FBETA, "precision": _ffi.OP_PRECISION, "recall": _ffi.OP_RECALL}


def _criterion(criterion):
    """"f1" | ("fbeta", beta) | ("precision", p) | ("recall", r) -> (ACX_OP_*, float param); ValueError otherwise."""
    if isinstance(criterion, str) and criterion == "f1":
        return _ffi.OP_FBETA, 1.0
    try:
        name, value = criterion
        code, value = _CRITERIA[name], float(value)
    except (TypeError, ValueError, KeyError):
        raise ValueError('criterion must be "f1", ("fbeta", beta), ("precision", p) or ("recall", r) (got %r)' % (criterion,)) from None
    if code == _ffi.OP_FBETA:
        if not (value > 0.0 and np.isfinite(value)):
            raise ValueError("beta must be a finite number > 0 (got %r)" % (value,))
    elif not 0.0 < value <= 1.0:
        raise ValueError("the %s to reach must be in (0, 1] (got %r)" % (name, value))
    return code, value


def _ratio(num, den):
    """num / den in float64, 0.0 where den == 0 (sklearn's zero_division=0)."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


def _summary(tp, fp, fn, beta):
    b2 = float(beta) * float(beta)
    return {"precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
            "f": _ratio((1.0 + b2) * tp, (1.0 + b2) * tp + b2 * fn + fp)}


class OperatingPoints:
    """Per-class thresholds and the confusion counts they give.  threshold: (C,) float32, counts: (C, 4) int64 = TP, FP, FN, TN,
    both device tensors (operating_points_host: numpy arrays).  Everything else is float64 numpy computed from the counts (one
    copy to the host, kept); a ratio without a denominator is 0.0, sklearn's zero_division=0."""

    def __init__(self, threshold, counts):
        self.threshold, self.counts = threshold, counts
        self._host = None

    def counts_host(self):
        """counts as an int64 numpy array (C, 4)."""
        if self._host is None:
            self._host = self.counts.cpu().numpy() if isinstance(self.counts, torch.Tensor) else np.asarray(self.counts)
        return self._host

    @property
    def precision(self):
        tp, fp, fn, tn = self.counts_host().T
        return _ratio(tp, tp + fp)

    @property
    def recall(self):
        tp, fp, fn, tn = self.counts_host().T
        return _ratio(tp, tp + fn)

    def f(self, beta=1.0):
        """F-beta per class."""
        tp, fp, fn, tn = self.counts_host().T
        return _summary(tp, fp, fn, beta)["f"]

    def micro(self, beta=1.0):
        """{"precision", "recall", "f"} of the counts summed over the classes (floats)."""
        tp, fp, fn, tn = self.counts_host().sum(axis=0)
        return {k: float(v) for k, v in _summary(tp, fp, fn, beta).items()}

    def macro(self, beta=1.0):
        """{"precision", "recall", "f"}: the per-class values averaged over all classes (floats)."""
        tp, fp, fn, tn = self.counts_host().T
        return {k: float(v.mean()) for k, v in _summary(tp, fp, fn, beta).items()}


def operating_points_host(target, clipwise_output, criterion="f1"):
    """The definition of acx_operating_points (include/acx.h) in numpy float64: per class, the distinct scores of the positives
    are the candidate thresholds of the rule score >= threshold, and the criterion picks one.  Returns an OperatingPoints of
    numpy arrays.  Every float64 operation below is rounded on its own, in the order the header states."""
    _shape_check(target, clipwise_output)
    code, value = _criterion(criterion)
    s, y = _host_scores(clipwise_output), _host_target(target)
    s = np.where(s == 0, np.float32(0.0), s)                        # -0.0 == +0.0, returned as +0.0
    C = s.shape[1]
    thr = np.full(C, np.inf, np.float32)
    counts = np.zeros((C, 4), np.int64)
    for c in range(C):
        pos, neg = np.sort(s[y[:, c] == 1, c]), np.sort(s[y[:, c] == 0, c])
        P, Nn = len(pos), len(neg)
        counts[c] = (0, 0, P, Nn)
        if P == 0:
            continue
        cand = np.unique(pos)                                       # ascending
        tp = P - np.searchsorted(pos, cand, side="left")            # TP = P - #pos(< t)
        fp = Nn - np.searchsorted(neg, cand, side="left")           # FP = Nn - #neg(< t)
        fn = P - tp
        if code == _ffi.OP_FBETA:
            b2 = value * value
            num = (1.0 + b2) * tp.astype(np.float64)
            den = (num + b2 * fn.astype(np.float64)) + fp.astype(np.float64)
            f = num / den
            i = int(np.nonzero(f == f.max())[0][-1])                # among equal F the highest threshold
        elif code == _ffi.OP_PRECISION:
            ok = np.nonzero(tp.astype(np.float64) / (tp + fp).astype(np.float64) >= value)[0]
            if len(ok) == 0:
                continue                                            # unreachable: +inf, (0, 0, P, Nn)
            i = int(ok[0])                                          # the lowest: the most recall at that precision
        else:
            ok = np.nonzero(tp.astype(np.float64) / np.float64(P) >= value)[0]
            i = int(ok[-1])                                         # the highest (the lowest candidate always qualifies)
        thr[c] = cand[i]
        counts[c] = (tp[i], fp[i], fn[i], Nn - fp[i])
    return OperatingPoints(thr, counts)


def operating_points(target, clipwise_output, criterion="f1", device=None):
    """One threshold per class on the GPU (acx_operating_points): (N, C) targets and scores as tagging_metrics takes them, and a
    criterion: "f1", ("fbeta", beta) -- the largest F-beta, the highest threshold among equals --, ("precision", p) -- the
    lowest threshold whose precision reaches p -- or ("recall", r) -- the highest whose recall reaches r.  Returns an
    OperatingPoints on the device.  A class without positives (or whose precision never reaches p) gets +inf and never fires;
    one UserWarning names how many have no positives.  ValueErrors as tagging_metrics."""
    code, value = _criterion(criterion)
    scores, tgt, dtype, device = _to_device(target, clipwise_output, device, "operating_points")
    n, C = scores.shape
    ws_bytes = _ffi.metrics_workspace_bytes(n, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    thr = torch.empty(C, dtype=torch.float32, device=device)
    counts = torch.empty((C, 4), dtype=torch.int64, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(device):
        _ffi.operating_points(vp(scores), scores.stride(0), vp(tgt), dtype, tgt.stride(0), n, C, code, value, vp(thr), vp(counts),
                              vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(device))
    _raise_status(int(status.cpu()[0]))
    op = OperatingPoints(thr, counts)
    host = op.counts_host()
    empty = int(((host[:, 0] + host[:, 2]) == 0).sum())
    if empty:
        warnings.warn("%d class(es) have no positive target: their threshold is +inf and they never fire" % empty, UserWarning,
                      stacklevel=2)
    return op


def threshold_metrics(target, clipwise_output, threshold, device=None):
    """The counts of score >= threshold[c] on the GPU (acx_threshold_counts) -- thresholds chosen on one split scored on another.
    threshold: (C,) numbers, a CUDA tensor (read where it is; a NaN raises through the status word) or a host array (checked
    here); +-inf are allowed.  Returns an OperatingPoints whose threshold is the float32 device tensor used."""
    scores, tgt, dtype, device = _to_device(target, clipwise_output, device, "threshold_metrics")
    n, C = scores.shape
    if isinstance(threshold, torch.Tensor) and threshold.is_cuda:
        thr = threshold.detach().to(device=device, dtype=torch.float32).contiguous()
    else:
        host = np.asarray(threshold.detach().numpy() if isinstance(threshold, torch.Tensor) else threshold)
        if host.dtype == object or not (np.issubdtype(host.dtype, np.floating) or np.issubdtype(host.dtype, np.integer)):
            raise ValueError("threshold must hold numbers (got dtype %s)" % host.dtype)
        with np.errstate(over="ignore"):
            host = np.ascontiguousarray(host, dtype=np.float32)
        if np.isnan(host).any():
            raise ValueError("thresholds hold a NaN")
        thr = torch.from_numpy(host).to(device)
    if tuple(thr.shape) != (C,):
        raise ValueError("threshold has shape %s for %d classes (expected (%d,))" % (tuple(thr.shape), C, C))
    counts = torch.empty((C, 4), dtype=torch.int64, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(device):
        _ffi.threshold_counts(vp(scores), scores.stride(0), vp(tgt), dtype, tgt.stride(0), n, C, vp(thr), vp(counts), vp(status),
                              _ffi.stream_ptr(device))
    _raise_status(int(status.cpu()[0]))
    return OperatingPoints(thr, counts)
