"""Per-class AudioSet statistics on the GPU (acx_tagging_metrics in include/acx.h): the average precision, ROC-AUC and d' of
`evaluate.calculate_statistics` -- sklearn 1.7.2 average_precision_score / roc_auc_score with average=None and
sqrt(2) * scipy.stats.norm.ppf(auc) -- up to float64 rounding, from scores taken as float32.

    from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics
    stats = tagging_metrics(target, clipwise_output)      # {"average_precision", "auc", "d_prime"}: float64 (C,) arrays

CUDA tensors are read where they are, on the current stream (a column slice of a wider tensor too); numpy arrays and CPU tensors
are checked on the host, then copied to `device` (default: the current CUDA device), the targets as uint8.  A class with no
positive or no negative target gets AP 0 / 1 and NaN AUC and d', with one UserWarning, as sklearn does."""
import warnings

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs


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
        device = clipwise_output.device if s_dev else target.device if t_dev else None
    device = _inputs.cuda_device(device, who + " runs on")
    scores = _inputs.rows(clipwise_output.to(device=device, dtype=torch.float32)) if s_dev else torch.from_numpy(scores).to(device)
    tgt, dtype = _inputs.kernel_target(target.to(device) if t_dev else torch.from_numpy(tgt).to(device))
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
    with torch.cuda.device(device):
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
    with torch.cuda.device(device):
        _ffi.threshold_counts(vp(scores), scores.stride(0), vp(tgt), dtype, tgt.stride(0), n, C, vp(thr), vp(counts), vp(status),
                              _ffi.stream_ptr(device))
    _raise_status(int(status.cpu()[0]))
    return OperatingPoints(thr, counts)


# ---- bootstrap resamples and weighted statistics ---------------------------------------------------------------------------
# The definitions of acx_bootstrap_weights and acx_weighted_metrics (include/acx.h) in plain numpy, and the calls that run them
# on the GPU: a resample of the clips is a vector of integer weights over an order of each class's scores that never changes.

_MIX1, _MIX2, _GOLDEN = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)
_STATS = ("average_precision", "auc", "d_prime")
_SUMMARIES = (("mAP", "average_precision"), ("auc", "auc"), ("d_prime", "d_prime"))
MAX_WEIGHT_SUM = 1 << 30


def _mix(z):
    """splitmix64's finaliser over a uint64 array (wrap-around arithmetic)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    z = (z ^ (z >> np.uint64(30))) * _MIX1
    z = (z ^ (z >> np.uint64(27))) * _MIX2
    return z ^ (z >> np.uint64(31))


def _check_draw_args(seed, first, replicates, n):
    seed, first, replicates, n = int(seed), int(first), int(replicates), int(n)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64) (got %d)" % seed)
    if replicates < 1:
        raise ValueError("replicates must be >= 1 (got %d)" % replicates)
    if first < 0 or first + replicates > 1 << 32:
        raise ValueError("replicate numbers must be in [0, 2^32) (got %d .. %d)" % (first, first + replicates - 1))
    if not 1 <= n <= 1 << 30:
        raise ValueError("n must be in [1, 2^30] (got %d)" % n)
    return seed, first, replicates, n


def bootstrap_indices_host(seed, r, n, start=0, stop=None):
    """The rows replicate r draws from n clips -- draws start .. stop - 1 (default: all n) as an int64 array:
    x = mix(mix(seed) + 0x9E3779B97F4A7C15 * (((r << 32) | j) + 1)), idx = ((x >> 32) * n) >> 32, uint64 wrap-around arithmetic.
    The multiply-shift is biased by at most n / 2^32."""
    seed, r, _, n = _check_draw_args(seed, r, 1, n)
    stop = n if stop is None else int(stop)
    if not 0 <= int(start) <= stop <= n:
        raise ValueError("draws %d .. %d of %d" % (start, stop, n))
    j = np.arange(int(start), stop, dtype=np.uint64)
    counter = ((np.uint64(r) << np.uint64(32)) | j) + np.uint64(1)
    x = _mix(_mix(np.array([seed], dtype=np.uint64))[0] + _GOLDEN * counter)
    return (((x >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def bootstrap_weights_host(seed, replicates, n, first=0):
    """(replicates, n) int32: row k counts how often replicate first + k drew each clip; every row sums to n."""
    seed, first, replicates, n = _check_draw_args(seed, first, replicates, n)
    return np.stack([np.bincount(bootstrap_indices_host(seed, first + k, n), minlength=n) for k in range(replicates)]).astype(np.int32)


def _host_weights(weights, n):
    """-> (R, n) int64, checked: integers >= 0, every row summing to at most 2^30."""
    w = np.asarray(weights.numpy() if isinstance(weights, torch.Tensor) else weights)
    if w.dtype == np.bool_:
        w = w.astype(np.int64)
    if w.dtype == object or not np.issubdtype(w.dtype, np.integer):
        raise ValueError("weights must hold integers (got dtype %s)" % w.dtype)
    if w.ndim == 1:
        w = w[None, :]
    if w.ndim != 2 or w.shape[1] != n or w.shape[0] == 0:
        raise ValueError("weights must have shape (R, %d) or (%d,); got %s" % (n, n, tuple(np.shape(weights))))
    if w.dtype == np.uint64 and (w > np.uint64(MAX_WEIGHT_SUM)).any():
        raise ValueError("the weights of a replicate sum above 2^30")
    w = w.astype(np.int64)
    if (w < 0).any():
        raise ValueError("weights hold a negative value")
    if (w.sum(axis=1) > MAX_WEIGHT_SUM).any():
        raise ValueError("the weights of a replicate sum above 2^30")
    return w


def _erfinv(x):
    return torch.special.erfinv(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def weighted_metrics_host(target, clipwise_output, weights):
    """The definition of acx_weighted_metrics in numpy: {"average_precision", "auc", "d_prime"} as float64 (R, C) arrays for
    (N, C) targets and scores and integer weights (R, N) or (N,) (R = 1), w >= 0.  Per class and weight vector, with Pw / Nw the
    weight of the positives / negatives and, for each distinct positive score t whose positives weigh g > 0, TPw / FPw the weight
    of the positives / negatives with score >= t:
        AP = (1 / Pw) sum_t g * (TPw / (TPw + FPw));  AUC = sum_t g * (2 Nw(< t) + Nw(= t)) / (2 Pw Nw);  d' = 2 erfinv(2 AUC - 1)
    Pw = 0: all three NaN (tagging_metrics has AP = 0 for a class without positives; a resample without one says nothing about
    the class).  Nw = 0 < Pw: AP = 1, AUC and d' NaN.  These are sklearn's values on the rows repeated w times and with
    sample_weight=w."""
    _shape_check(target, clipwise_output)
    s, y = _host_scores(clipwise_output), _host_target(target)
    s = np.where(s == 0, np.float32(0.0), s)                        # -0.0 == +0.0
    n, C = s.shape
    w = _host_weights(weights, n)
    R = w.shape[0]
    ap, auc = np.full((R, C), np.nan), np.full((R, C), np.nan)
    for c in range(C):
        pos = y[:, c] == 1
        op, on = np.argsort(s[pos, c], kind="stable"), np.argsort(s[~pos, c], kind="stable")
        sp, sn = s[pos, c][op], s[~pos, c][on]
        t, first = np.unique(sp, return_index=True)                 # the distinct positive scores, ascending
        last = np.append(first[1:], len(sp))
        lb, ub = np.searchsorted(sn, t, side="left"), np.searchsorted(sn, t, side="right")
        for r in range(R):
            cp = np.concatenate([[0], np.cumsum(w[r][pos][op])])
            cn = np.concatenate([[0], np.cumsum(w[r][~pos][on])])
            Pw, Nw = int(cp[-1]), int(cn[-1])
            if Pw == 0:
                continue
            g = cp[last] - cp[first]
            tpw, nlt, neq = Pw - cp[first], cn[lb], cn[ub] - cn[lb]
            fpw = Nw - nlt
            keep = g > 0
            prec = tpw[keep].astype(np.float64) / (tpw[keep] + fpw[keep]).astype(np.float64)
            ap[r, c] = float(np.sum(g[keep].astype(np.float64) * prec)) / float(Pw)
            if Nw > 0:
                auc[r, c] = np.float64(int(np.sum(g * (2 * nlt + neq)))) / np.float64(2 * Pw * Nw)
    return {"average_precision": ap, "auc": auc, "d_prime": 2.0 * _erfinv(2.0 * auc - 1.0)}


def bootstrap_weights(replicates, n, seed=0, first=0, device=None):
    """bootstrap_weights_host on the GPU (acx_bootstrap_weights): an int32 device tensor (replicates, n), bit for bit the same."""
    seed, first, replicates, n = _check_draw_args(seed, first, replicates, n)
    device = _inputs.cuda_device(device, "bootstrap weights are drawn on")
    w = torch.empty((replicates, n), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _ffi.bootstrap_weights(seed, first, replicates, n, vp(w), n, _ffi.stream_ptr(device))
    return w


def _device_weights(weights, n, device):
    """-> int32 device tensor (R, n), rows at a stride >= n: host weights are checked here, device weights by the kernel."""
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        w = weights.detach()
        if w.dtype == torch.bool:
            w = w.to(torch.int32)
        if w.is_floating_point() or w.is_complex():
            raise ValueError("weights must hold integers (got dtype %s)" % w.dtype)
        if w.dim() == 1:
            w = w.unsqueeze(0)
        if w.dim() != 2 or w.shape[1] != n or w.shape[0] == 0:
            raise ValueError("weights must have shape (R, %d) or (%d,); got %s" % (n, n, tuple(weights.shape)))
        if w.dtype != torch.int32:
            w = w.clamp(-1, MAX_WEIGHT_SUM + 1).to(torch.int32)     # what is invalid stays invalid
        return _inputs.rows(w.to(device))
    return torch.from_numpy(_host_weights(weights, n).astype(np.int32)).to(device)


def _raise_weight_status(st):
    _raise_status(st)
    if st & _ffi.METRICS_BAD_WEIGHT:
        raise ValueError("weights hold a negative value, or the weights of a replicate sum above 2^30")


def _check_weighted_n(n, who):
    if n > _ffi.WEIGHTED_MAX_N:
        raise ValueError("%s: %d clips (at most %d: the weights of a class are recounted in LDS)" % (who, n, _ffi.WEIGHTED_MAX_N))


class _WeightedRunner:
    """acx_weighted_metrics on inputs that are already on the device, with one workspace for every call."""

    def __init__(self, scores, tgt, dtype, device):
        self.scores, self.tgt, self.dtype, self.device = scores, tgt, dtype, device
        self.n, self.C = scores.shape
        self.ws_bytes = _ffi.weighted_metrics_workspace_bytes(self.n, self.C)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.status = torch.empty(1, dtype=torch.int32, device=device)

    def __call__(self, w):
        """w: int32 device tensor (R, n) -> float64 numpy (3, R, C); ValueError through the status word."""
        R = w.shape[0]
        out = torch.empty((3, R, self.C), dtype=torch.float64, device=self.device)
        s, t = self.scores, self.tgt
        with torch.cuda.device(self.device):
            _ffi.weighted_metrics(vp(s), s.stride(0), vp(t), self.dtype, t.stride(0), self.n, self.C, vp(w), w.stride(0), R,
                                  vp(out[0]), vp(out[1]), vp(out[2]), vp(self.status), (vp(self.ws), self.ws_bytes),
                                  _ffi.stream_ptr(self.device))
        res = out.cpu().numpy()
        _raise_weight_status(int(self.status.cpu()[0]))
        return res


def weighted_metrics(target, clipwise_output, weights, device=None):
    """weighted_metrics_host on the GPU (acx_weighted_metrics): {"average_precision", "auc", "d_prime"} as float64 numpy arrays
    (R, C).  target and clipwise_output as tagging_metrics takes them (N <= 32768); weights: integers >= 0 of shape (R, N) or
    (N,) (R = 1), a host array or a device tensor, every row summing to at most 2^30.  A class whose positives all have weight
    0 gets NaN in all three (no warning: under a resample that is an outcome, not a defect of the data).  ValueErrors as
    tagging_metrics, and for weights that are not integers, negative or too large."""
    _shape_check(target, clipwise_output)
    _check_weighted_n(clipwise_output.shape[0], "weighted_metrics")
    scores, tgt, dtype, device = _to_device(target, clipwise_output, device, "weighted_metrics")
    res = _WeightedRunner(scores, tgt, dtype, device)(_device_weights(weights, scores.shape[0], device))
    return {k: res[i].copy() for i, k in enumerate(_STATS)}


def _mean_where(x, ok):
    """Row means of x over the entries where ok, and how many those are; NaN for a row with none."""
    count = ok.sum(axis=-1)
    total = np.where(ok, x, 0.0).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, total / count, np.nan), count


def summarize_classes(stats):
    """{"average_precision", "auc", "d_prime"} of shape (..., C) -> (values (..., 3), classes counted (..., 3)): mAP is the mean of
    AP over the classes where it is not NaN, AUC likewise, d' over the classes where it is finite."""
    ap, auc, dp = (np.asarray(stats[k], np.float64) for k in _STATS)
    m = [_mean_where(ap, ~np.isnan(ap)), _mean_where(auc, ~np.isnan(auc)), _mean_where(dp, np.isfinite(dp))]
    return np.stack([v for v, _ in m], axis=-1), np.stack([c for _, c in m], axis=-1).astype(np.int64)


def _check_confidence(confidence):
    confidence = float(confidence)
    if not 0.0 < confidence < 1.0:
        raise ValueError("confidence must be in (0, 1) (got %r)" % (confidence,))
    return confidence


def bootstrap_summary(estimate, replicates, confidence=0.95, per_class=False):
    """The host arithmetic of bootstrap_metrics.  estimate: the three statistics of the full data, (C,) each, NaN where a class
    is undefined (weighted_metrics' convention); replicates: the same per replicate, (R, C) each.  Percentile intervals:
    np.quantile(values, [alpha / 2, 1 - alpha / 2]) with alpha = 1 - confidence, numpy's default interpolation, float64."""
    confidence = _check_confidence(confidence)
    q = [(1.0 - confidence) / 2.0, 1.0 - (1.0 - confidence) / 2.0]
    point, _ = summarize_classes(estimate)
    values, counted = summarize_classes(replicates)
    out = {"confidence": confidence, "classes_counted": counted}
    for i, (name, _) in enumerate(_SUMMARIES):
        low, high = np.quantile(values[:, i], q)
        out[name] = {"estimate": float(point[i]), "low": float(low), "high": float(high), "replicates": values[:, i].copy()}
    if per_class:
        out["per_class"] = {}
        for k in _STATS:
            v = np.asarray(replicates[k], np.float64)
            ok = np.isfinite(v) if k == "d_prime" else ~np.isnan(v)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)      # a class no replicate defines: NaN bounds
                low, high = np.nanquantile(np.where(ok, v, np.nan), q, axis=0)
            out["per_class"][k] = {"estimate": np.asarray(estimate[k], np.float64).copy(), "low": low, "high": high,
                                   "defined": ok.mean(axis=0)}
    return out


def bootstrap_metrics(target, clipwise_output, replicates=1000, seed=0, confidence=0.95, per_class=False, chunk=256, device=None):
    """Clip-level bootstrap of mAP, macro AUC and macro d' on the GPU: `replicates` resamples of the N clips with replacement
    (bootstrap_weights, seed), the per-class statistics of each (weighted_metrics) and percentile intervals.  Returns
        {"mAP", "auc", "d_prime"}: each {"estimate", "low", "high", "replicates": (R,) float64},
        "classes_counted": (R, 3) -- the classes that entered each replicate's three means --, "confidence",
        and with per_class=True "per_class": {"average_precision", "auc", "d_prime"}: each {"estimate", "low", "high", "defined"}
        of shape (C,), the bounds over the replicates that define the class and `defined` their fraction.
    A replicate's mAP / AUC is the mean over the classes where the statistic is not NaN, its d' over those where it is finite;
    the estimates apply the same rule to the statistics of the full data (all weights 1: tagging_metrics' values, a class
    without positives left out instead of counted as AP = 0).  Replicates are processed `chunk` at a time -- the weights and
    statistics of one chunk are all that is resident -- and the results do not depend on `chunk`."""
    seed, _, replicates, _ = _check_draw_args(seed, 0, replicates, 1)
    _check_confidence(confidence)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1 (got %d)" % chunk)
    _shape_check(target, clipwise_output)
    _check_weighted_n(clipwise_output.shape[0], "bootstrap_metrics")
    scores, tgt, dtype, device = _to_device(target, clipwise_output, device, "bootstrap_metrics")
    n, C = scores.shape
    run = _WeightedRunner(scores, tgt, dtype, device)
    full = run(torch.ones((1, n), dtype=torch.int32, device=device))
    reps = np.empty((3, replicates, C), np.float64)
    for first in range(0, replicates, chunk):
        k = min(chunk, replicates - first)
        reps[:, first:first + k] = run(bootstrap_weights(k, n, seed=seed, first=first, device=device))
    out = bootstrap_summary({key: full[i, 0] for i, key in enumerate(_STATS)}, {key: reps[i] for i, key in enumerate(_STATS)},
                            confidence=confidence, per_class=per_class)
    out["seed"] = seed
    return out


def bootstrap_difference(target, scores_a, scores_b, replicates=1000, seed=0, confidence=0.95, chunk=256, device=None):
    """Two models on the same clips and the same resamples (one seed): the percentile interval of a - b for mAP, AUC and d'.
    Returns {"mAP", "auc", "d_prime"}: each {"estimate", "low", "high", "replicates": (R,) of a - b, "fraction_a_greater"}, and
    "a" / "b": bootstrap_metrics of each model."""
    a = bootstrap_metrics(target, scores_a, replicates, seed, confidence, False, chunk, device)
    b = bootstrap_metrics(target, scores_b, replicates, seed, confidence, False, chunk, device)
    alpha = 1.0 - a["confidence"]
    out = {"confidence": a["confidence"], "seed": a["seed"], "a": a, "b": b}
    for name, _ in _SUMMARIES:
        d = a[name]["replicates"] - b[name]["replicates"]
        low, high = np.quantile(d, [alpha / 2.0, 1.0 - alpha / 2.0])
        out[name] = {"estimate": a[name]["estimate"] - b[name]["estimate"], "low": float(low), "high": float(high), "replicates": d,
                     "fraction_a_greater": float(np.mean(d > 0))}
    return out
