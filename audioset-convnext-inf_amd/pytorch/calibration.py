"""Calibration of a head's probabilities on the GPU (the "calibration" section of include/acx.h): measure it (reliability
diagram, ECE / MCE, Brier score, NLL), fit a map on a validation split (per-class Platt scaling for multi-label heads,
temperature scaling for single-label heads) and apply the map.

    from audioset_convnext_inf_amd.pytorch.calibration import reliability, fit_platt, reliability_toplabel, fit_temperature
    r = reliability(target, probs, bins=15); r.classwise_ece, r.brier, r.curve(c)          # counts on the device
    cal = fit_platt(val_target, val_logits).check(); probs = cal.apply(model(x)["clipwise_logits"])
    t = fit_temperature(val_labels, val_logits).check(); probs, top_prob, top_index = t.softmax_topk(logits, k=5)

Definitions (the *_host functions below are their float64 evaluation in numpy, the reference of the tests; Platt 1999 with the
Newton / backtracking solver of Lin, Lin & Weng 2007; temperature scaling and ECE as in Guo et al. 2017):
  bin            of a probability p (float32) with B bins: min(B - 1, int(float32(p * float32(B)))): p = 1 falls into the last bin,
                 an edge k / B belongs to bin k.
  ECE_c          sum_b (count_b / n) |positive_b / count_b - conf_sum_b / count_b|; MCE_c the largest of the gaps; classwise_ece
                 the mean of ECE_c over the classes with at least one row; Brier_c = sum_i (p_i - y_i)^2 / n.
  top-label      confidence = the largest softmax probability of the row (scaled by beta = 1 / T first), correct = the first
                 index of the row maximum is the label; nll = mean of logsumexp(z) - z_y.
  Platt          per class the minimiser of F(a, b) = -sum_i [t_i log p_i + (1 - t_i) log(1 - p_i)], p_i = sigmoid(a z_i + b), with
                 t+ = (P + 1) / (P + 2), t- = 1 / (Nn + 2) (smooth) or t = y.
  temperature    the minimiser over beta in [1e-4, 1e4] of F(beta) = sum_i [logsumexp_c(beta z_ic) - beta z_i,y_i].
CUDA tensors are read where they lie (row strides are passed through); everything runs on the current stream of their device and
nothing synchronises until a derived number or check() is read."""
import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs
from .classify import _check_labels, _check_logits

DEGENERATE, NOT_CONVERGED, AT_BOUND = _ffi.CAL_DEGENERATE, _ffi.CAL_NOT_CONVERGED, _ffi.CAL_AT_BOUND
# "F does not increase" in both fits means F_new <= F + F_SLACK max(1, |F|): near the minimiser a Newton step changes F by less
# than the rounding of its float64 sum, and comparing two roundings would halve good steps for ever
F_SLACK = 2.0 ** -40


def _check_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= _ffi.CAL_MAX_BINS:
        raise ValueError("bins must be an integer in 1 .. %d (got %r)" % (_ffi.CAL_MAX_BINS, bins))
    return int(bins)


def _device_pair(target, scores, what):
    """(scores fp32 CUDA (n, C) readable in place, targets, ACX_TARGET_*) of a 2-D score tensor / array and its targets."""
    if not isinstance(scores, torch.Tensor):
        scores = torch.as_tensor(np.asarray(scores, dtype=np.float32))
    if not isinstance(target, torch.Tensor):
        target = torch.as_tensor(np.asarray(target))
    if scores.dim() != 2 or tuple(target.shape) != tuple(scores.shape):
        raise ValueError("%s and target must be 2-D of one shape (got %s and %s)" % (what, tuple(scores.shape), tuple(target.shape)))
    n, C = int(scores.shape[0]), int(scores.shape[1])
    if n < 1:
        raise ValueError("%s holds no rows" % what)
    if not 1 <= C <= _ffi.MAX_CLASSES:
        raise ValueError("%s has %d classes (expected 1 .. %d)" % (what, C, _ffi.MAX_CLASSES))
    dev = scores.device if scores.is_cuda else _inputs.cuda_device(None, what + " needs")
    scores = _inputs.rows(scores.to(device=dev, dtype=torch.float32))
    target, code = _inputs.kernel_target(target.to(dev))
    return scores, target, code, n, C


def _status_error(st, what):
    if st & _ffi.CAL_NONFINITE:
        raise ValueError("%s hold NaN or infinite values" % what)
    if st & _ffi.CAL_BAD_PROBABILITY:
        raise ValueError("probabilities lie outside [0, 1]")
    if st & _ffi.CAL_BAD_TARGET:
        raise ValueError("target holds values other than 0 and 1")
    if st & _ffi.CAL_BAD_LABEL:
        raise ValueError("labels hold values outside the classes of the logits")


# ---- measuring ------------------------------------------------------------------------------------------------------------------
def _gaps(count, hit, conf_sum):
    """(weights count / n_rows, |observed frequency - mean confidence|) per bin along the last axis; empty bins give 0."""
    count = np.asarray(count, dtype=np.float64)
    safe = np.maximum(count, 1.0)
    gap = np.where(count > 0, np.abs(np.asarray(hit, dtype=np.float64) / safe - np.asarray(conf_sum, dtype=np.float64) / safe), 0.0)
    total = np.maximum(count.sum(axis=-1, keepdims=True), 1.0)
    return count / total, gap


class _ReliabilitySummary:
    """The float64 numbers of reliability(); subclasses provide _arrays() -> (count (C, B), positive (C, B), conf_sum (C, B),
    brier_sum (C,)) as numpy."""

    @property
    def ece(self):
        count, pos, conf, _ = self._arrays()
        w, gap = _gaps(count, pos, conf)
        return (w * gap).sum(axis=1)

    @property
    def mce(self):
        count, pos, conf, _ = self._arrays()
        return _gaps(count, pos, conf)[1].max(axis=1)

    @property
    def classwise_ece(self):
        count = self._arrays()[0]
        have = count.sum(axis=1) > 0
        return float(self.ece[have].mean()) if have.any() else 0.0

    @property
    def brier(self):
        count, _, _, brier = self._arrays()
        return np.asarray(brier, dtype=np.float64) / np.maximum(count.sum(axis=1), 1)

    def curve(self, c):
        """(mean confidence, observed frequency, count) of class c, one entry per non-empty bin."""
        count, pos, conf, _ = self._arrays()
        keep = count[c] > 0
        k = count[c][keep].astype(np.float64)
        return conf[c][keep] / k, pos[c][keep] / k, count[c][keep]


class Reliability(_ReliabilitySummary):
    """reliability() on the device: count, positive (C, bins) int64, conf_sum (C, bins) float64, brier_sum (C,) float64, status
    (1,) int32.  The float64 properties copy them to the host on first use (one synchronisation)."""

    def __init__(self, count, positive, conf_sum, brier_sum, status, n, bins):
        self.count, self.positive, self.conf_sum, self.brier_sum, self.status = count, positive, conf_sum, brier_sum, status
        self.n, self.bins = n, bins
        self._host = None

    def _arrays(self):
        if self._host is None:
            self.check()
            self._host = tuple(t.cpu().numpy() for t in (self.count, self.positive, self.conf_sum, self.brier_sum))
        return self._host

    def check(self):
        """Raises ValueError for a NaN / infinite or out-of-range probability or a target other than 0 / 1.  Synchronises."""
        _status_error(int(self.status.item()), "probabilities")
        return self


class HostReliability(_ReliabilitySummary):
    def __init__(self, count, positive, conf_sum, brier_sum, bins):
        self.count, self.positive, self.conf_sum, self.brier_sum, self.bins = count, positive, conf_sum, brier_sum, bins

    def _arrays(self):
        return self.count, self.positive, self.conf_sum, self.brier_sum


def reliability(target, probs, bins=15):
    """Reliability counts of (n, C) probabilities against (n, C) 0 / 1 targets (bool, uint8 or float) -> Reliability."""
    bins = _check_bins(bins)
    probs, target, code, n, C = _device_pair(target, probs, "probs")
    dev = probs.device
    with torch.cuda.device(dev):
        count = torch.empty((C, bins), dtype=torch.int64, device=dev)
        positive = torch.empty((C, bins), dtype=torch.int64, device=dev)
        conf_sum = torch.empty((C, bins), dtype=torch.float64, device=dev)
        brier_sum = torch.empty(C, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _ffi.reliability_counts(vp(probs), probs.stride(0), vp(target), code, target.stride(0), n, C, bins, vp(count), vp(positive),
                                vp(conf_sum), vp(brier_sum), vp(status), _ffi.stream_ptr(dev))
    return Reliability(count, positive, conf_sum, brier_sum, status, n, bins)


class _TopLabelSummary:
    """Subclasses provide _arrays() -> (count (B,), correct (B,), conf_sum (B,), nll_sum float) as numpy."""

    @property
    def counted(self):
        return int(self._arrays()[0].sum())

    @property
    def ece(self):
        count, hit, conf, _ = self._arrays()
        w, gap = _gaps(count, hit, conf)
        return float((w * gap).sum())

    @property
    def mce(self):
        count, hit, conf, _ = self._arrays()
        return float(_gaps(count, hit, conf)[1].max())

    @property
    def nll(self):
        count, _, _, nll = self._arrays()
        return float(nll) / max(int(count.sum()), 1)

    @property
    def accuracy(self):
        count, hit, _, _ = self._arrays()
        return float(hit.sum()) / max(int(count.sum()), 1)

    def curve(self):
        """(mean confidence, accuracy, count) per non-empty bin."""
        count, hit, conf, _ = self._arrays()
        keep = count > 0
        k = count[keep].astype(np.float64)
        return conf[keep] / k, hit[keep] / k, count[keep]


class TopLabelReliability(_TopLabelSummary):
    """reliability_toplabel() on the device: count, correct (bins,) int64, conf_sum (bins,) float64, nll_sum (1,) float64, status
    (1,) int32.  Rows that check() complains about are counted nowhere."""

    def __init__(self, count, correct, conf_sum, nll_sum, status, n, bins):
        self.count, self.correct, self.conf_sum, self.nll_sum, self.status, self.n, self.bins = (count, correct, conf_sum, nll_sum,
                                                                                                 status, n, bins)
        self._host = None

    def _arrays(self):
        if self._host is None:
            self._host = (self.count.cpu().numpy(), self.correct.cpu().numpy(), self.conf_sum.cpu().numpy(),
                          float(self.nll_sum.item()))
        return self._host

    def check(self):
        """Raises ValueError if a row was left out: a NaN or infinite logit, or a label outside [0, N).  Synchronises."""
        _status_error(int(self.status.item()), "logits")
        return self


class HostTopLabelReliability(_TopLabelSummary):
    def __init__(self, count, correct, conf_sum, nll_sum, bins, skipped):
        self.count, self.correct, self.conf_sum, self.nll_sum, self.bins, self.skipped = count, correct, conf_sum, nll_sum, bins, skipped

    def _arrays(self):
        return self.count, self.correct, self.conf_sum, self.nll_sum


def _beta_of(calibration, device):
    if calibration is None:
        return None
    if not isinstance(calibration, TemperatureScaling):
        raise ValueError("calibration must be a TemperatureScaling or None (got %s)" % type(calibration).__name__)
    return calibration.beta.to(device)


def reliability_toplabel(labels, logits, bins=15, calibration=None):
    """Top-label reliability of (n, N) fp32 CUDA logits against (n,) integer labels -> TopLabelReliability.  calibration: a
    TemperatureScaling whose beta scales the logits first."""
    bins = _check_bins(bins)
    logits, n, N = _check_logits(logits)
    dev = logits.device
    lab = _check_labels(labels, n, dev)
    beta = _beta_of(calibration, dev)
    with torch.cuda.device(dev):
        count = torch.empty(bins, dtype=torch.int64, device=dev)
        correct = torch.empty(bins, dtype=torch.int64, device=dev)
        conf_sum = torch.empty(bins, dtype=torch.float64, device=dev)
        nll_sum = torch.empty(1, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = _ffi.temperature_workspace_bytes(n, N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ffi.reliability_toplabel(vp(logits), logits.stride(0), vp(lab), n, N, vp(beta), bins, vp(count), vp(correct), vp(conf_sum),
                                  vp(nll_sum), vp(status), (vp(ws), nbytes), _ffi.stream_ptr(dev))
    return TopLabelReliability(count, correct, conf_sum, nll_sum, status, n, bins)


# ---- Platt scaling ----------------------------------------------------------------------------------------------------------------
class PlattScaling:
    """One (a, b) per class: p = sigmoid(a z + b).  ab (C, 2) float64, info (C,) int32 and status (1,) int32 are device tensors;
    a and b are views of ab.  info[c]: the Newton iterations used, DEGENERATE (the identity is returned) or NOT_CONVERGED."""

    def __init__(self, ab, info=None, status=None):
        self.ab = ab
        self.info = info if info is not None else torch.zeros(ab.shape[0], dtype=torch.int32, device=ab.device)
        self.status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=ab.device)

    @property
    def a(self):
        return self.ab[:, 0]

    @property
    def b(self):
        return self.ab[:, 1]

    def check(self):
        """Raises ValueError for bad data (NaN / infinite logits, targets other than 0 / 1) and for classes whose iteration did
        not converge, which it names.  Degenerate classes keep the identity and are no error.  Synchronises."""
        _status_error(int(self.status.item()), "logits")
        bad = np.nonzero(self.info.cpu().numpy() == NOT_CONVERGED)[0]
        if bad.size:
            raise ValueError("Platt scaling did not converge for %d class(es): %s" % (bad.size, ", ".join(str(c) for c in bad[:16])
                                                                                      + (" ..." if bad.size > 16 else "")))
        return self

    def apply(self, logits):
        """(rows, C) fp32 CUDA logits -> calibrated probabilities (rows, C) fp32, on the current stream; nothing synchronises."""
        logits, rows, C = _check_logits(logits)
        if C != self.ab.shape[0]:
            raise ValueError("logits have %d classes, the calibration %d" % (C, self.ab.shape[0]))
        dev = logits.device
        ab = self.ab if self.ab.device == dev else self.ab.to(dev)
        with torch.cuda.device(dev):
            out = torch.empty((rows, C), dtype=torch.float32, device=dev)
            _ffi.platt_apply(vp(logits), logits.stride(0), rows, C, vp(ab), vp(out), C, _ffi.stream_ptr(dev))
        return out

    def save(self, path):
        np.savez(path, method="platt", ab=self.ab.cpu().numpy(), info=self.info.cpu().numpy())

    @classmethod
    def load(cls, path, device=None):
        dev = _inputs.cuda_device(device, "a calibration is applied on")
        with np.load(path) as f:
            if str(f["method"]) != "platt":
                raise ValueError("%s holds a %s calibration, not Platt scaling" % (path, f["method"]))
            ab, info = f["ab"], f["info"]
        if ab.ndim != 2 or ab.shape[1] != 2 or not np.isfinite(ab).all():
            raise ValueError("%s: ab must be a finite (C, 2) array" % path)
        return cls(torch.as_tensor(ab, dtype=torch.float64).contiguous().to(dev), torch.as_tensor(info, dtype=torch.int32).to(dev))


def fit_platt(target, logits, smooth=True):
    """Per-class Platt scaling of (n, C) logits against (n, C) 0 / 1 targets, fitted on the GPU in one launch -> PlattScaling."""
    logits, target, code, n, C = _device_pair(target, logits, "logits")
    dev = logits.device
    with torch.cuda.device(dev):
        ab = torch.empty((C, 2), dtype=torch.float64, device=dev)
        info = torch.empty(C, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = _ffi.platt_workspace_bytes(n, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ffi.platt_fit(vp(logits), logits.stride(0), vp(target), code, target.stride(0), n, C, bool(smooth), vp(ab), vp(info),
                       vp(status), (vp(ws), nbytes), _ffi.stream_ptr(dev))
    return PlattScaling(ab, info, status)


# ---- temperature scaling ----------------------------------------------------------------------------------------------------------
class TemperatureScaling:
    """One beta = 1 / T for a single-label head: probabilities = softmax(beta z).  beta (1,) float64, info (1,) int32 and status
    (1,) int32 are device tensors.  info: the evaluations used, DEGENERATE, NOT_CONVERGED or AT_BOUND."""

    def __init__(self, beta, info=None, status=None):
        self.beta = beta
        self.info = info if info is not None else torch.zeros(1, dtype=torch.int32, device=beta.device)
        self.status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=beta.device)

    @property
    def temperature(self):
        """T = 1 / beta as a Python float.  Synchronises."""
        return 1.0 / float(self.beta.item())

    def check(self):
        """Raises ValueError for rows left out (NaN / infinite logits, labels out of range), for an iteration that did not
        converge and for one that stopped against a bound of [1e-4, 1e4].  Synchronises."""
        _status_error(int(self.status.item()), "logits")
        info = int(self.info.item())
        if info == NOT_CONVERGED:
            raise ValueError("temperature scaling did not converge in the evaluations given")
        if info == AT_BOUND:
            raise ValueError("temperature scaling stopped at a bound: beta = %g" % float(self.beta.item()))
        return self

    def apply(self, logits):
        """(rows, N) fp32 CUDA logits -> float32(beta) * logits, the input of softmax_topk; nothing synchronises."""
        logits, rows, N = _check_logits(logits)
        dev = logits.device
        beta = self.beta if self.beta.device == dev else self.beta.to(dev)
        with torch.cuda.device(dev):
            out = torch.empty((rows, N), dtype=torch.float32, device=dev)
            _ffi.temperature_apply(vp(logits), logits.stride(0), rows, N, vp(beta), vp(out), N, _ffi.stream_ptr(dev))
        return out

    def softmax_topk(self, logits, k=5, probabilities=True):
        """classify.softmax_topk of the scaled logits -> (probs, top_prob, top_index)."""
        from .classify import softmax_topk
        return softmax_topk(self.apply(logits), k=k, probabilities=probabilities)

    def save(self, path):
        np.savez(path, method="temperature", beta=self.beta.cpu().numpy(), info=self.info.cpu().numpy())

    @classmethod
    def load(cls, path, device=None):
        dev = _inputs.cuda_device(device, "a calibration is applied on")
        with np.load(path) as f:
            if str(f["method"]) != "temperature":
                raise ValueError("%s holds a %s calibration, not temperature scaling" % (path, f["method"]))
            beta, info = f["beta"], f["info"]
        if beta.shape != (1,) or not np.isfinite(beta).all() or not beta[0] > 0:
            raise ValueError("%s: beta must be one finite value > 0" % path)
        return cls(torch.as_tensor(beta, dtype=torch.float64).to(dev), torch.as_tensor(info, dtype=torch.int32).to(dev))


def fit_temperature(labels, logits, evaluations=32):
    """Temperature scaling of (n, N) fp32 CUDA logits against (n,) integer labels: `evaluations` passes over the logits are
    queued on the current stream, the Newton decisions stay on the device -> TemperatureScaling."""
    if isinstance(evaluations, bool) or not isinstance(evaluations, (int, np.integer)) or \
            not 1 <= evaluations <= _ffi.CAL_MAX_EVALUATIONS:
        raise ValueError("evaluations must be an integer in 1 .. %d (got %r)" % (_ffi.CAL_MAX_EVALUATIONS, evaluations))
    logits, n, N = _check_logits(logits)
    dev = logits.device
    lab = _check_labels(labels, n, dev)
    with torch.cuda.device(dev):
        beta = torch.empty(1, dtype=torch.float64, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = _ffi.temperature_workspace_bytes(n, N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ffi.temperature_fit(vp(logits), logits.stride(0), vp(lab), n, N, int(evaluations), vp(beta), vp(info), vp(status),
                             (vp(ws), nbytes), _ffi.stream_ptr(dev))
    return TemperatureScaling(beta, info, status)


def load_calibration(path, device=None):
    """The PlattScaling or TemperatureScaling a .npz written by save() holds."""
    with np.load(path) as f:
        method = str(f["method"])
    if method == "platt":
        return PlattScaling.load(path, device)
    if method == "temperature":
        return TemperatureScaling.load(path, device)
    raise ValueError("%s: unknown calibration method %r" % (path, method))


# ---- host definitions (numpy float64) -----------------------------------------------------------------------------------------------
def bin_index_host(p, bins):
    """min(bins - 1, int(float32(p) * float32(bins))) with the product rounded to float32."""
    p = np.asarray(p, dtype=np.float32)
    return np.minimum(bins - 1, (p * np.float32(bins)).astype(np.float32).astype(np.int64))


def reliability_host(target, probs, bins=15):
    """reliability() in numpy: exact counts, float64 sums -> HostReliability.  Raises ValueError for bad data."""
    p = np.asarray(probs, dtype=np.float32)
    t = np.asarray(target)
    if not np.isfinite(p).all():
        raise ValueError("probabilities hold NaN or infinite values")
    if ((p < 0) | (p > 1)).any():
        raise ValueError("probabilities lie outside [0, 1]")
    if not ((t == 0) | (t == 1)).all():
        raise ValueError("target holds values other than 0 and 1")
    y = (t == 1)
    n, C = p.shape
    b = bin_index_host(p, bins)
    count, positive = np.zeros((C, bins), dtype=np.int64), np.zeros((C, bins), dtype=np.int64)
    conf = np.zeros((C, bins), dtype=np.float64)
    p64 = p.astype(np.float64)
    for c in range(C):
        count[c] = np.bincount(b[:, c], minlength=bins)
        positive[c] = np.bincount(b[:, c], weights=y[:, c], minlength=bins).astype(np.int64)
        conf[c] = np.bincount(b[:, c], weights=p64[:, c], minlength=bins)
    brier = ((p64 - y) ** 2).sum(axis=0)
    return HostReliability(count, positive, conf, brier, bins)


def reliability_toplabel_host(labels, logits=None, bins=15, beta=None, confidence=None, prediction=None):
    """reliability_toplabel() in numpy -> HostTopLabelReliability.  Either from logits alone (float64 softmax of float32(beta) *
    logits), or from given per-row `confidence` and `prediction` (e.g. the device's softmax_topk output: top_prob[:, 0] and
    top_index[:, 0], -1 for a flagged row), with the logits still giving the NLL."""
    y = np.asarray(labels, dtype=np.int64)
    z = np.asarray(logits, dtype=np.float32)
    if beta is not None:
        z = (np.float32(beta) * z).astype(np.float32)
    z64 = z.astype(np.float64)
    n, N = z.shape
    ok = np.isfinite(z).all(axis=1) & (y >= 0) & (y < N)
    zz, yy = z64[ok], y[ok]
    m = zz.max(axis=1) if zz.size else np.zeros(0)
    s = np.exp(zz - m[:, None]).sum(axis=1)
    if confidence is None:
        conf = (1.0 / s).astype(np.float32)                      # exp(m - m) / s
        pred = np.argmax(zz, axis=1) if zz.size else np.zeros(0, dtype=np.int64)
    else:
        conf = np.asarray(confidence, dtype=np.float32)[ok]
        pred = np.asarray(prediction, dtype=np.int64)[ok]
    b = bin_index_host(conf, bins)
    count = np.bincount(b, minlength=bins).astype(np.int64)
    correct = np.bincount(b, weights=(pred == yy), minlength=bins).astype(np.int64)
    conf_sum = np.bincount(b, weights=conf.astype(np.float64), minlength=bins)
    nll = float((np.log(s) + (m - zz[np.arange(zz.shape[0]), yy])).sum())
    return HostTopLabelReliability(count, correct, conf_sum, nll, bins, int((~ok).sum()))


def platt_sums_host(z, y, a, b, smooth=True):
    """(F, gradient (2,), Hessian (2, 2), targets) of one class at (a, b) in float64; log p and log(1 - p) from one exp(-|u|)."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y).astype(bool)
    P, Nn = float(y.sum()), float((~y).sum())
    t = np.where(y, (P + 1.0) / (P + 2.0), 1.0 / (Nn + 2.0)) if smooth else y.astype(np.float64)
    u = a * z + b
    e = np.exp(-np.abs(u))
    l1 = np.log1p(e)
    lp, lq = np.minimum(u, 0.0) - l1, np.minimum(-u, 0.0) - l1
    inv = 1.0 / (1.0 + e)
    p = np.where(u >= 0, inv, e * inv)
    F = -float((t * lp + (1.0 - t) * lq).sum())
    g = p - t
    h = e * inv * inv
    grad = np.array([float((g * z).sum()), float(g.sum())])
    H = np.array([[float((h * z * z).sum()), float((h * z).sum())], [float((h * z).sum()), float(h.sum())]])
    return F, grad, H, t


def platt_newton_step_host(z, y, a, b, smooth=True):
    """The Newton step (da, db) at (a, b) with the 1e-12 ridge, and the Hessian's smallest eigenvalue."""
    _, g, H, _ = platt_sums_host(z, y, a, b, smooth)
    haa, hbb, hab = H[0, 0] + 1e-12, H[1, 1] + 1e-12, H[0, 1]
    det = haa * hbb - hab * hab
    step = np.array([-(hbb * g[0] - hab * g[1]) / det, -(haa * g[1] - hab * g[0]) / det])
    return step, float(np.linalg.eigvalsh(H)[0])


def fit_platt_host(target, logits, smooth=True):
    """fit_platt() in numpy float64 -> (ab (C, 2), info (C,) int32): per class, from a = 0, b = log((P + 1) / (Nn + 1)), Newton
    steps delta on the 2 x 2 Hessian with a 1e-12 ridge, the step halved (50 times at the most) until F does not increase; it
    stops at an accepted point whose Newton step has |delta|_inf <= 1e-10 max(1, |a|, |b|), or after 100 iterations.  info: the
    steps taken."""
    z_all = np.asarray(logits, dtype=np.float32).astype(np.float64)
    t_all = np.asarray(target)
    if not np.isfinite(z_all).all():
        raise ValueError("logits hold NaN or infinite values")
    if not ((t_all == 0) | (t_all == 1)).all():
        raise ValueError("target holds values other than 0 and 1")
    n, C = z_all.shape
    ab, info = np.zeros((C, 2)), np.zeros(C, dtype=np.int32)
    for c in range(C):
        z, y = z_all[:, c], t_all[:, c] == 1
        P, Nn = int(y.sum()), int((~y).sum())
        if P == 0 or Nn == 0 or (z == z[0]).all():
            ab[c], info[c] = (1.0, 0.0), DEGENERATE
            continue
        a, b = 0.0, float(np.log((P + 1.0) / (Nn + 1.0)))
        ta, tb, da, db, step, Fa = a, b, 0.0, 0.0, 1.0, 0.0
        code, it, halvings, first = NOT_CONVERGED, 0, 0, True
        while True:
            F, g, H, _ = platt_sums_host(z, y, ta, tb, smooth)
            if first or F <= Fa + F_SLACK * max(1.0, abs(Fa)):
                first, a, b, Fa = False, ta, tb, F
                haa, hbb, hab = H[0, 0] + 1e-12, H[1, 1] + 1e-12, H[0, 1]
                det = haa * hbb - hab * hab
                da, db = -(hbb * g[0] - hab * g[1]) / det, -(haa * g[1] - hab * g[0]) / det
                if max(abs(da), abs(db)) <= 1e-10 * max(1.0, abs(a), abs(b)):
                    code = it
                    break
                if it == 100:
                    break
                it += 1
                step, halvings = 1.0, 0
            else:
                step *= 0.5
                halvings += 1
                if halvings == 50:
                    code = it
                    break
            with np.errstate(over="ignore", invalid="ignore"):
                ta, tb = a + step * da, b + step * db
        ab[c], info[c] = (a, b), code
    return ab, info


def platt_apply_host(logits, ab):
    """sigmoid(float32(a) z + float32(b)) in float64, a and b rounded to float32 as the kernel takes them."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    ab32 = np.asarray(ab, dtype=np.float64).astype(np.float32).astype(np.float64)
    u = ab32[None, :, 0] * z + ab32[None, :, 1]
    e = np.exp(-np.abs(u))
    return np.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def temperature_sums_host(labels, logits, beta):
    """(F, F', F'', rows that are not constant) at beta in float64 over the rows that are counted."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    y = np.asarray(labels, dtype=np.int64)
    ok = np.isfinite(z).all(axis=1) & (y >= 0) & (y < z.shape[1])
    z, y = z[ok], y[ok]
    zm = z.max(axis=1, keepdims=True)
    e = np.exp(beta * (z - zm))
    s = e.sum(axis=1, keepdims=True)
    E = (e * z).sum(axis=1, keepdims=True) / s
    var = (e * (z - E) ** 2).sum(axis=1, keepdims=True) / s
    zy = z[np.arange(z.shape[0]), y][:, None]
    F = float((np.log(s) + beta * (zm - zy)).sum())
    return F, float((E - zy).sum()), float(var.sum()), int((z.max(axis=1) != z.min(axis=1)).sum())


def fit_temperature_host(labels, logits, evaluations=32):
    """fit_temperature() in numpy float64 -> (beta, info): from beta = 1, Newton steps -F' / max(F'', 1e-12), the step halved
    until beta stays inside [1e-4, 1e4] and F does not increase; it stops at an accepted point whose Newton step has |delta| <=
    1e-10 max(1, beta) (info = the evaluations used), or against a bound, when a step the bound has cut moves beta by no more than
    that (AT_BOUND); one evaluation of (F, F', F'') per trial point, `evaluations` of them at the most."""
    base, Fb, d, step, cut, trial = 1.0, 0.0, 0.0, 1.0, False, 1.0
    for evals in range(1, int(evaluations) + 1):
        F, g, h, nonconst = temperature_sums_host(labels, logits, trial)
        accepted = False
        if evals == 1:
            if nonconst == 0:
                return 1.0, DEGENERATE
            Fb, accepted = F, True
        elif F <= Fb + F_SLACK * max(1.0, abs(Fb)):
            delta = step * d
            base, Fb = trial, F
            if cut and abs(delta) <= 1e-10 * max(1.0, base):
                return base, AT_BOUND
            accepted = True
        else:
            step *= 0.5
            if step < 2.0 ** -60:
                return base, (AT_BOUND if cut else evals)
            trial = base + step * d
        if accepted:
            d = -g / max(h, 1e-12)
            if not abs(d) <= 1.79e308:
                return base, NOT_CONVERGED
            if abs(d) <= 1e-10 * max(1.0, base):
                return base, evals
            step, cut = 1.0, False
            for _ in range(1200):
                if 1e-4 <= base + step * d <= 1e4:
                    break
                step *= 0.5
                cut = True
            trial = base + step * d
    return base, NOT_CONVERGED
