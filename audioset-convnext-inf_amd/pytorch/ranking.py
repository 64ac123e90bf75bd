"""Ranking metrics per clip on the GPU (acx_ranking_metrics in include/acx.h): the classes of one clip ranked against each other
-- LRAP, lwlrap (the label-weighted label-ranking average precision of DCASE 2019 Task 2 / FSDKaggle2019), coverage error,
label-ranking loss, one-error and precision / recall at k -- where metrics.py ranks the clips of one class.

    from audioset_convnext_inf_amd.pytorch.ranking import ranking_metrics, bootstrap_ranking
    r = ranking_metrics(target, clipwise_output, k=5)       # r.lwlrap, r.lrap, r.coverage_error, r.ranking_loss, r.precision_at_k
    ci = bootstrap_ranking(target, clipwise_output)         # {"lwlrap": {"estimate", "low", "high", "replicates"}, ...}

Everything rests on integer counts per (clip, positive class) -- ranking_metrics_host is the definition -- so LRAP, coverage error
and ranking loss are sklearn 1.7.2's label_ranking_average_precision_score, coverage_error and label_ranking_loss up to the order
of their float64 sums, tied scores included (a tie takes the worst rank).  lwlrap equals the DCASE reference code wherever a
clip has no tied scores; with ties that code depends on argsort's order, and this one keeps sklearn's rule."""
import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import metrics

_BOOT = ("lrap", "lwlrap", "ranking_loss", "coverage_error")


def _check_k(k, classes):
    k = int(k)
    if not 1 <= k <= classes:
        raise ValueError("k must be in 1 .. %d classes (got %d)" % (classes, k))
    return k


def _row_columns(n_pos, coverage, bad_pairs, psum, classes):
    """The per-row float64 columns every mean below is made of -> (lrap_i, loss_i, coverage_i, psum_i, n_pos_i); torch tensors
    of any device.  A row with no positive or no negative class counts 1.0 towards LRAP and 0 towards the ranking loss."""
    np_f = n_pos.to(torch.float64)
    full = (n_pos == 0) | (n_pos == classes)
    one = torch.ones_like(np_f)
    lrap = torch.where(full, one, psum / torch.where(full, one, np_f))
    loss = torch.where(full, torch.zeros_like(np_f), bad_pairs.to(torch.float64) / torch.where(full, one, np_f * (classes - np_f)))
    return lrap, loss, coverage.to(torch.float64), psum, np_f


def replicate_statistics(weights, n_pos, coverage, bad_pairs, psum, classes):
    """(R, 4) float64 = lrap, lwlrap, ranking_loss, coverage_error of R weightings of the rows: every one is a ratio of sums over
    rows, so a resample is its integer weight vector times the per-row columns.  weights: (R, rows) integers; torch tensors of
    one device.  lwlrap is NaN for a weighting that keeps no positive."""
    cols = torch.stack(_row_columns(n_pos, coverage, bad_pairs, psum, classes), dim=1)        # (rows, 5)
    w = weights.to(torch.float64)
    sums = w @ cols                                                                           # (R, 5)
    total = w.sum(dim=1)
    return torch.stack([sums[:, 0] / total, sums[:, 3] / sums[:, 4], sums[:, 1] / total, sums[:, 2] / total], dim=1)


class RankingMetrics:
    """The counts of acx_ranking_metrics and what follows from them.  Per row, on the device (ranking_metrics_host: numpy):
    n_pos, coverage, bad_pairs, hits (int64) and psum (float64); per class class_count (int64) and class_psum (float64).  The
    scalars and per-class arrays are float64 numpy computed on the host from one copy of the counts, made -- with the check of
    the status word -- when the first of them is read; nothing synchronises before that."""

    def __init__(self, row_counts, psum, class_count, class_psum, classes, k, status=None, hits1=None):
        self.row_counts, self.psum, self._class_count, self.class_psum = row_counts, psum, class_count, class_psum
        self.classes, self.k = int(classes), int(k)
        self._status, self._hits1, self._host, self._cols = status, hits1, None, None

    n_pos = property(lambda self: self.row_counts[:, _ffi.RANK_N_POS])
    coverage = property(lambda self: self.row_counts[:, _ffi.RANK_COVERAGE])
    bad_pairs = property(lambda self: self.row_counts[:, _ffi.RANK_BAD_PAIRS])
    hits = property(lambda self: self.row_counts[:, _ffi.RANK_HITS])

    def check(self):
        """Raise the ValueError of a NaN / infinite score or a target other than 0 / 1 found on the device (one synchronisation)."""
        if self._status is not None:
            st = int(self._status.cpu()[0])
            metrics._raise_status(st)
            self._status = None
        return self

    def host(self):
        """(row_counts (rows, 4) int64, psum (rows,), class_count (C,) int64, class_psum (C,)) as numpy arrays, checked."""
        if self._host is None:
            self.check()
            self._host = tuple(x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
                               for x in (self.row_counts, self.psum, self._class_count, self.class_psum))
        return self._host

    def _columns(self):
        """_row_columns of the host copy, as numpy arrays (computed once)."""
        if self._cols is None:
            rc, psum, _, _ = self.host()
            n_pos, coverage, bad = (torch.from_numpy(np.ascontiguousarray(rc[:, i])) for i in range(3))
            self._cols = tuple(c.numpy() for c in _row_columns(n_pos, coverage, bad, torch.from_numpy(psum), self.classes))
        return self._cols

    @property
    def lrap(self):
        return float(self._columns()[0].mean())

    @property
    def ranking_loss(self):
        return float(self._columns()[1].mean())

    @property
    def coverage_error(self):
        return float(self._columns()[2].mean())

    @property
    def lwlrap(self):
        rc, psum, _, _ = self.host()
        total = int(rc[:, 0].sum())
        return float(psum.sum()) / total if total else float("nan")

    @property
    def class_count(self):
        return self.host()[2]

    @property
    def per_class_lwlrap(self):
        _, _, count, csum = self.host()
        return np.divide(csum, count, out=np.full(count.shape, np.nan), where=count > 0)

    @property
    def class_weight(self):
        count = self.host()[2]
        total = int(count.sum())
        return count / total if total else np.full(count.shape, np.nan)

    @property
    def precision_at_k(self):
        return float((self.host()[0][:, 3] / float(self.k)).mean())

    @property
    def recall_at_k(self):
        rc = self.host()[0]
        has = rc[:, 0] > 0
        return float((rc[has, 3] / rc[has, 0]).mean()) if has.any() else float("nan")

    @property
    def one_error(self):
        """1 - the share of rows whose top class (score descending, then class index) is positive.  With k > 1 the top-1 hits
        come from a second call with k = 1 on the same device inputs, made when this is first read."""
        h1 = self.host()[0][:, 3] if self.k == 1 else self._hits1
        if callable(h1):
            h1 = self._hits1 = h1().host()[0][:, 3]
        return 1.0 - float((np.asarray(h1) > 0).mean())

    def summary(self):
        """The scalars as a dict of floats."""
        return {key: getattr(self, key) for key in ("lrap", "lwlrap", "coverage_error", "ranking_loss", "one_error",
                                                    "precision_at_k", "recall_at_k")}


def ranking_metrics_host(target, scores, k=1):
    """The definition of acx_ranking_metrics in plain numpy -> a RankingMetrics of numpy arrays.  For every positive class j of a
    row with float32 scores s (-0.0 == +0.0):
        ge_j = #{c : s_c >= s_j}    pge_j = #{c positive : s_c >= s_j}    ord_j = #{c : s_c > s_j} + #{c < j : s_c == s_j}
    n_pos; psum = sum_j pge_j / ge_j, each quotient one float64 division, added in ascending j; coverage = max_j ge_j (0 without
    positives); bad_pairs = sum_j (ge_j - pge_j); hits = #{j : ord_j < k}; class_count[c] = rows where c is positive and
    class_psum[c] = their pge / ge added in ascending row."""
    metrics._shape_check(target, scores)
    s, y = metrics._host_scores(scores), metrics._host_target(target)
    rows, C = s.shape
    k = _check_k(k, C)
    s = np.where(s == 0, np.float32(0.0), s)
    counts = np.zeros((rows, 4), np.int64)
    hits1 = np.zeros(rows, np.int64)
    psum = np.zeros(rows, np.float64)
    q = np.zeros((rows, C), np.float64)
    index = np.arange(C)
    for i in range(rows):
        pos = np.nonzero(y[i])[0]
        if len(pos) == 0:
            continue
        sj = s[i, pos][:, None]
        ge_m = s[i][None, :] >= sj                                                             # (P, C)
        ge = ge_m.sum(axis=1)
        pge = ge_m[:, pos].sum(axis=1)
        order = (s[i][None, :] > sj).sum(axis=1) + ((s[i][None, :] == sj) & (index[None, :] < pos[:, None])).sum(axis=1)
        quot = pge.astype(np.float64) / ge.astype(np.float64)
        q[i, pos] = quot
        psum[i] = np.cumsum(quot)[-1]                                                          # ascending j, one add each
        counts[i] = (len(pos), ge.max(), (ge - pge).sum(), (order < k).sum())
        hits1[i] = (order < 1).sum()
    class_psum = np.cumsum(q, axis=0)[-1]                                                      # ascending row; + 0.0 changes nothing
    return RankingMetrics(counts, psum, y.astype(np.int64).sum(axis=0), class_psum, C, k, hits1=hits1)


def _launch(scores, tgt, dtype, k, slice_rows, device):
    """acx_ranking_metrics on device tensors -> (row_counts, psum, class_count, class_psum, status), nothing read back."""
    rows, C = scores.shape
    ws_bytes = _ffi.ranking_workspace_bytes(rows, C, slice_rows)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    row_counts = torch.empty((rows, _ffi.RANK_COUNTS), dtype=torch.int64, device=device)
    psum = torch.empty(rows, dtype=torch.float64, device=device)
    class_count = torch.empty(C, dtype=torch.int64, device=device)
    class_psum = torch.empty(C, dtype=torch.float64, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _ffi.ranking_metrics(vp(scores), scores.stride(0), vp(tgt), dtype, tgt.stride(0), rows, C, k, slice_rows, vp(row_counts),
                             vp(psum), vp(class_count), vp(class_psum), vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(device))
    return row_counts, psum, class_count, class_psum, status


def ranking_metrics(target, scores, k=1, device=None, slice_rows=None):
    """ranking_metrics_host on the GPU (acx_ranking_metrics) -> a RankingMetrics whose counts stay on the device.  target and
    scores: (clips, classes) as tagging_metrics takes them, at most 32768 classes -- CUDA tensors are read where they are on the
    current stream and checked through the kernel's status word when a result is first read; host arrays are checked here,
    before any copy, with the same ValueErrors.  k: the cut of precision / recall at k.  slice_rows: rows per slice of the
    per-class sums (None: the library's default); the results do not depend on it.  The cost is O(positives x classes) per
    clip: made for tagging data with a few positives per clip, quadratic for dense targets on very wide heads."""
    metrics._shape_check(target, scores)
    C = scores.shape[1]
    k = _check_k(k, C)
    if C > _ffi.MAX_CLASSES:
        raise ValueError("ranking_metrics: %d classes (at most %d: a clip's scores are ranked in LDS)" % (C, _ffi.MAX_CLASSES))
    if slice_rows is not None and int(slice_rows) < 1:
        raise ValueError("slice_rows must be >= 1 (got %d)" % int(slice_rows))
    slice_rows = 0 if slice_rows is None else int(slice_rows)
    dev_scores, tgt, dtype, device = metrics._to_device(target, scores, device, "ranking_metrics")
    out = _launch(dev_scores, tgt, dtype, k, slice_rows, device)
    hits1 = None if k == 1 else (lambda: RankingMetrics(*_launch(dev_scores, tgt, dtype, 1, slice_rows, device)[:4], C, 1))
    return RankingMetrics(out[0], out[1], out[2], out[3], C, k, status=out[4], hits1=hits1)


def bootstrap_ranking(target, scores, replicates=1000, seed=0, confidence=0.95, k=1, chunk=256, device=None):
    """Clip-level bootstrap intervals of lrap, lwlrap, ranking_loss and coverage_error on the GPU: `replicates` resamples of the
    clips with replacement (metrics.bootstrap_weights, seed).  Each statistic is a ratio of sums over clips, so a replicate is its
    integer weight vector times the per-clip columns of ONE ranking_metrics call (float64 on the device, `chunk` replicates at
    a time).  Returns {"lrap", "lwlrap", "ranking_loss", "coverage_error"}: each {"estimate", "low", "high", "replicates": (R,)
    float64} -- the estimate is ranking_metrics' value, the bounds np.quantile(values, [alpha / 2, 1 - alpha / 2]) as
    metrics.bootstrap_summary takes them (a replicate without any positive leaves lwlrap NaN and out of its bounds) --, and
    "confidence", "seed", "metrics": the RankingMetrics."""
    seed, _, replicates, _ = metrics._check_draw_args(seed, 0, replicates, 1)
    confidence = metrics._check_confidence(confidence)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1 (got %d)" % chunk)
    full = ranking_metrics(target, scores, k=k, device=device).check()
    rows, device = full.psum.shape[0], full.psum.device
    values = np.empty((replicates, len(_BOOT)), np.float64)
    for first in range(0, replicates, chunk):
        n = min(chunk, replicates - first)
        w = metrics.bootstrap_weights(n, rows, seed=seed, first=first, device=device)
        values[first:first + n] = replicate_statistics(w, full.n_pos, full.coverage, full.bad_pairs, full.psum, full.classes).cpu().numpy()
    q = [(1.0 - confidence) / 2.0, 1.0 - (1.0 - confidence) / 2.0]
    out = {"confidence": confidence, "seed": seed, "metrics": full}
    for i, name in enumerate(_BOOT):
        v = values[:, i]
        low, high = np.nanquantile(v, q) if not np.isnan(v).all() else (np.nan, np.nan)
        out[name] = {"estimate": getattr(full, name), "low": float(low), "high": float(high), "replicates": v.copy()}
    return out
