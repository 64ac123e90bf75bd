"""Reading and judging a single-label head on the GPU (acx_softmax_topk / acx_classification_counts in include/acx.h): the
counterpart of sigmoid outputs, tagging_metrics and operating_points for heads trained with softmax cross-entropy
(fit_head(..., loss="ce")) -- ESC-50, UrbanSound8K, GTZAN, SpeechCommands, any "one folder per class" data set.

    from audioset_convnext_inf_amd.pytorch.classify import softmax_topk, classification_metrics
    probs, top_prob, top_index = softmax_topk(model(x)["clipwise_logits"], k=5)      # device tensors, nothing synchronises
    m = classification_metrics(labels, logits, k=5)                                  # counts on the device
    m.accuracy, m.topk_accuracy, m.macro_f1, m.confusion                            # the properties synchronise when read

Definitions (the *_host functions below are their float64 / exact evaluation in numpy, the reference of the tests):
  probabilities  p_c = exp(z_c - m) / sum_c exp(z_c - m), m = max_c z_c.
  top k          classes ordered by logit descending, then class index ascending, with -0.0 equal to +0.0; decided on the
                 logits, not on the rounded probabilities.
  prediction     the first index of the row maximum (the top 1 of that order).
  top-k hit      rank of the true class y < k, rank = #{c : z_c > z_y, or z_c = z_y and c < y}.
  per class      support (rows with that label), predicted (rows with that prediction), correct (both); recall = correct /
                 support, precision = correct / predicted (0 for a class never predicted), F1 = 2 correct / (support + predicted).
  balanced_accuracy, macro_f1   means of recall / F1 over the classes WITH support, as sklearn's balanced_accuracy_score.
A row holding a NaN or an infinity, or a label outside [0, N), is counted nowhere; check() raises for them."""
import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs
from .metrics import _ratio


def _check_logits(logits, name="logits"):
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError("%s must be a (rows, N) tensor (got %s)" % (name, getattr(logits, "shape", type(logits))))
    if logits.dtype != torch.float32:
        raise ValueError("%s must be float32 (got %s)" % (name, logits.dtype))
    if not logits.is_cuda:
        raise ValueError("%s must be a CUDA (HIP) tensor (got device %s)" % (name, logits.device))
    rows, N = int(logits.shape[0]), int(logits.shape[1])
    if rows < 1:
        raise ValueError("%s holds no rows" % name)
    if not 1 <= N <= _ffi.MAX_CLASSES:
        raise ValueError("%s has N = %d classes (expected 1 .. %d)" % (name, N, _ffi.MAX_CLASSES))
    return _inputs.rows(logits), rows, N


def _check_k(k, N):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(N, _ffi.CLASSIFY_MAX_K):
        raise ValueError("k must be an integer in 1 .. min(N, %d) = %d (got %r)" % (_ffi.CLASSIFY_MAX_K, min(N, _ffi.CLASSIFY_MAX_K), k))
    return int(k)


def softmax_topk(logits, k=5, probabilities=True, status=None):
    """(probs (rows, N) fp32, top_prob (rows, k) fp32, top_index (rows, k) int32) of (rows, N) fp32 CUDA logits -- any tensor
    with unit column stride, row strides are passed through (model(x)["clipwise_logits"], forward_windows / stream rows).
    top_prob[r, j] has the bits of probs[r, top_index[r, j]].  A row holding a NaN or an infinity gets NaN probabilities and -1
    indices.  probabilities=False: probs is None and is not written.  status: an int32 (1,) device tensor that receives the
    call's status word (_ffi.CLASSIFY_NONFINITE).  Everything runs on the current stream; nothing synchronises."""
    logits, rows, N = _check_logits(logits)
    k = _check_k(k, N)
    dev = logits.device
    with torch.cuda.device(dev):
        probs = torch.empty((rows, N), dtype=torch.float32, device=dev) if probabilities else None
        top_prob = torch.empty((rows, k), dtype=torch.float32, device=dev)
        top_index = torch.empty((rows, k), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(1, dtype=torch.int32, device=dev)
        _ffi.softmax_topk(vp(logits), logits.stride(0), rows, N, k, vp(probs), N, vp(top_index), vp(top_prob), vp(status),
                          _ffi.stream_ptr(dev))
    return probs, top_prob, top_index


class _Summary:
    """The float64 properties shared by the device object and the host definition; subclasses provide _counts() ->
    (per_class (N, 3), hits (2,), n) as numpy int64."""

    @property
    def counted(self):
        """Rows that were counted (n minus the rows check() complains about)."""
        return int(self._counts()[0][:, 0].sum())

    @property
    def accuracy(self):
        pc, hits, _ = self._counts()
        return float(hits[0]) / max(int(pc[:, 0].sum()), 1)

    @property
    def topk_accuracy(self):
        pc, hits, _ = self._counts()
        return float(hits[1]) / max(int(pc[:, 0].sum()), 1)

    @property
    def recall(self):
        pc = self._counts()[0]
        return _ratio(pc[:, 2], pc[:, 0])

    @property
    def precision(self):
        pc = self._counts()[0]
        return _ratio(pc[:, 2], pc[:, 1])

    @property
    def f1(self):
        pc = self._counts()[0]
        return _ratio(2 * pc[:, 2], pc[:, 0] + pc[:, 1])

    @property
    def macro_f1(self):
        pc = self._counts()[0]
        have = pc[:, 0] > 0
        return float(self.f1[have].mean()) if have.any() else 0.0

    @property
    def balanced_accuracy(self):
        pc = self._counts()[0]
        have = pc[:, 0] > 0
        return float(self.recall[have].mean()) if have.any() else 0.0


class ClassificationMetrics(_Summary):
    """Counts of classification_metrics on the device: per_class (N, 3) int64 [support, predicted, correct], hits (2,) int64
    [top-1, top-k], confusion (N, N) int64 true x predicted (or None), status (1,) int32; n and k are Python ints.  The
    float64 properties copy the counts to the host on first use (one synchronisation)."""

    def __init__(self, per_class, hits, confusion, status, n, k):
        self.per_class, self.hits, self.confusion, self.status, self.n, self.k = per_class, hits, confusion, status, n, k
        self._host = None

    def _counts(self):
        if self._host is None:
            self._host = (self.per_class.cpu().numpy(), self.hits.cpu().numpy(), self.n)
        return self._host

    def check(self):
        """Raises ValueError if a row was left out: a NaN or infinite logit, or a label outside [0, N).  Synchronises."""
        st = int(self.status.item())
        if st & _ffi.CLASSIFY_NONFINITE:
            raise ValueError("logits hold NaN or infinite values")
        if st & _ffi.CLASSIFY_BAD_LABEL:
            raise ValueError("labels hold values outside [0, %d)" % self.per_class.shape[0])
        return self


def _check_labels(labels, rows, device, name="labels"):
    if not isinstance(labels, torch.Tensor):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dim() != 1 or labels.shape[0] != rows:
        raise ValueError("%s must be (%d,) class numbers (got %s)" % (name, rows, tuple(labels.shape)))
    if labels.dtype == torch.bool or labels.dtype.is_floating_point or labels.dtype.is_complex:
        raise ValueError("%s must be an integer tensor (got %s)" % (name, labels.dtype))
    return labels.to(device=device, dtype=torch.int64).contiguous()


def classification_metrics(labels, logits, k=5, confusion=True):
    """Accuracy, top-k accuracy, per-class counts and the confusion matrix of (n, N) fp32 CUDA logits against (n,) integer
    labels, counted on the GPU on the current stream -> ClassificationMetrics.  k is cut to N.  confusion=True needs
    N <= 4096.  Nothing synchronises until a property is read."""
    logits, n, N = _check_logits(logits)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("k must be an integer >= 1 (got %r)" % (k,))
    k = _check_k(min(int(k), N), N)
    dev = logits.device
    lab = _check_labels(labels, n, dev)
    if confusion and N > _ffi.CLASSIFY_MAX_CONFUSION:
        raise ValueError("confusion=True with N = %d classes (at most %d)" % (N, _ffi.CLASSIFY_MAX_CONFUSION))
    with torch.cuda.device(dev):
        per_class = torch.empty((N, 3), dtype=torch.int64, device=dev)
        hits = torch.empty(2, dtype=torch.int64, device=dev)
        conf = torch.empty((N, N), dtype=torch.int64, device=dev) if confusion else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _ffi.classification_counts(vp(logits), logits.stride(0), vp(lab), n, N, k, vp(per_class), vp(hits), vp(conf),
                                   vp(status), _ffi.stream_ptr(dev))
    return ClassificationMetrics(per_class, hits, conf, status, n, k)


# ---- host definitions (numpy float64 / exact) --------------------------------------------------------------------------------
def _order(z_row):
    """Class indices of one row by logit descending, then index ascending; -0.0 equals +0.0 (a stable sort on -z)."""
    return np.argsort(-(z_row.astype(np.float64) + 0.0), kind="stable")


def softmax_topk_host(logits, k=5):
    """(probs (rows, N) float64, top_prob (rows, k) float64, top_index (rows, k) int64) of float logits, by the definitions
    of the module docstring.  A row holding a NaN or an infinity gets NaN probabilities and -1 indices."""
    z = np.asarray(logits, dtype=np.float64)
    rows, N = z.shape
    probs = np.full((rows, N), np.nan)
    top_prob = np.full((rows, k), np.nan)
    top_index = np.full((rows, k), -1, dtype=np.int64)
    for r in range(rows):
        if not np.isfinite(z[r]).all():
            continue
        e = np.exp(z[r] - z[r].max())
        probs[r] = e / e.sum()
        top_index[r] = _order(z[r])[:k]
        top_prob[r] = probs[r, top_index[r]]
    return probs, top_prob, top_index


class HostClassificationMetrics(_Summary):
    def __init__(self, per_class, hits, confusion, n, k, skipped):
        self.per_class, self.hits, self.confusion, self.n, self.k, self.skipped = per_class, hits, confusion, n, k, skipped

    def _counts(self):
        return self.per_class, self.hits, self.n


def prediction_and_rank_host(labels, logits, chunk=4096):
    """(counted (n,) bool, prediction (n,) int64, rank of the true class (n,) int64) by the definitions of the module docstring;
    prediction and rank are 0 where a row is not counted."""
    z = np.asarray(logits)
    y = np.asarray(labels, dtype=np.int64)
    n, N = z.shape
    ok, pred, rank = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    cols = np.arange(N)[None, :]
    for lo in range(0, n, chunk):
        zz, yy = z[lo:lo + chunk], y[lo:lo + chunk]
        good = np.isfinite(zz).all(axis=1) & (yy >= 0) & (yy < N)
        yc = np.where(good, yy, 0)
        zy = zz[np.arange(zz.shape[0]), yc][:, None]
        with np.errstate(invalid="ignore"):
            r = ((zz > zy) | ((zz == zy) & (cols < yc[:, None]))).sum(axis=1)
        ok[lo:lo + chunk] = good
        pred[lo:lo + chunk] = np.where(good, np.argmax(np.where(np.isnan(zz), -np.inf, zz), axis=1), 0)   # first index of the maximum; -0.0 == +0.0
        rank[lo:lo + chunk] = np.where(good, r, 0)
    return ok, pred, rank


def classification_metrics_host(labels, logits, k=5, ranks=None):
    """The counts of classification_metrics in numpy -> an object with per_class, hits, confusion (int64 arrays), skipped (rows
    left out) and the same float64 properties.  ranks: the result of prediction_and_rank_host for these inputs, to share it
    between several k."""
    y = np.asarray(labels, dtype=np.int64)
    n, N = np.asarray(logits).shape
    k = min(int(k), N)
    ok, pred, rank = prediction_and_rank_host(labels, logits) if ranks is None else ranks
    yy, pp, rr = y[ok], pred[ok], rank[ok]
    per_class = np.zeros((N, 3), dtype=np.int64)
    per_class[:, 0] = np.bincount(yy, minlength=N)
    per_class[:, 1] = np.bincount(pp, minlength=N)
    per_class[:, 2] = np.bincount(yy[pp == yy], minlength=N)
    hits = np.array([int((pp == yy).sum()), int((rr < k).sum())], dtype=np.int64)
    conf = np.bincount(yy * N + pp, minlength=N * N).reshape(N, N).astype(np.int64)
    return HostClassificationMetrics(per_class, hits, conf, n, k, int((~ok).sum()))


def cross_entropy_host(z, y, label_smoothing=0.0):
    """(mean loss, per-row loss (rows,), dloss/dz (rows, N)) of F.cross_entropy(z, y, label_smoothing=..., reduction="mean") in
    float64: l_r = (m + log s) - sum_c q_c z_c with q_c = (1 - eps) [c = y_r] + eps / N, gradient (p - q) / rows."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    rows, N = z.shape
    eps = float(label_smoothing)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    q = np.full((rows, N), eps / N)
    q[np.arange(rows), y] += 1.0 - eps
    per_row = (m[:, 0] + np.log(s[:, 0])) - (q * z).sum(axis=1)
    return float(per_row.mean()), per_row, (p - q) / rows
