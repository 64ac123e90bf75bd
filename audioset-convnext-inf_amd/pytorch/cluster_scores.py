"""Cluster validation on the GPU (acx_silhouette, acx_cluster_dispersion, acx_contingency in include/acx.h): whether a clustering
is good, and which k to take -- what `sklearn.metrics.silhouette_samples`, `calinski_harabasz_score`, `davies_bouldin_score`,
`adjusted_rand_score` and `normalized_mutual_info_score` answer on the host.

    from audioset_convnext_inf_amd.pytorch.cluster_scores import silhouette, dispersion_scores, agreement, select_clusters
    sil = silhouette(emb, km.labels, metric="euclidean", clusters=50, sample=None, seed=0)
    sil.values, sil.a, sil.b, sil.nearest     # per queried row: float64, float64, float64, int64 device tensors
    sil.mean, sil.cluster_mean, sil.rows      # 0-d float64, (K,) float64, the sampled row indices (None: every row)
    sil.check()                               # the one call that synchronises; raises on bad data
    d = dispersion_scores(emb, km.labels)     # d.calinski_harabasz, d.davies_bouldin, d.counts, d.means, d.within
    ag = agreement(labels_true, km.labels)    # ag.contingency (device int64), ag.ari, ag.nmi, ag.homogeneity, ...
    sel = select_clusters(emb, (10, 20, 50), criterion="silhouette")     # sel.scores, sel.best_k, sel.best, sel.fits

The silhouette needs all n^2 pair distances: one fused kernel forms them tile by tile on the f32 matrix cores and reduces each
tile at once to float64 sums per (row, cluster); the (n, n) matrix is never written.  Every float64 sum runs in an order that
depends on (n, labels, the number of queried rows) alone (include/acx.h states it): the same inputs give the same bits.
`sample=m` queries m rows drawn without replacement by a seeded torch generator against ALL n columns -- scikit-learn's
`sample_size`, except that `b` still sees every row.  Empty clusters (k-means here can leave one) are skipped.

`silhouette_host`, `dispersion_host` and `agreement_host` are the documented host definitions in numpy float64 (the tests'
reference)."""
import collections

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs
from . import clustering
from . import retrieval

METRICS = tuple(_ffi.KMEANS_METRICS)
CRITERIA = ("silhouette", "calinski_harabasz", "davies_bouldin")
MAX_CLUSTERS = _ffi.KMEANS_MAX_CLUSTERS


_check_metric = clustering._check_metric
_inv_norms = clustering._inv_norms


def _check_clusters(clusters):
    if isinstance(clusters, bool) or not isinstance(clusters, (int, np.integer)) or not 1 <= clusters <= MAX_CLUSTERS:
        raise ValueError("clusters = %r (expected an integer in 1 .. %d)" % (clusters, MAX_CLUSTERS))


def _check_labels_shape(labels, n, name="labels"):
    shape = tuple(getattr(labels, "shape", ()))
    if shape != (n,):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, shape))


def _check_sample(sample, n):
    if sample is None:
        return
    if isinstance(sample, bool) or not isinstance(sample, (int, np.integer)) or not 1 <= sample <= n:
        raise ValueError("sample = %r (expected an integer in 1 .. n = %d, or None)" % (sample, n))


# ---- the host definitions (numpy float64) ----------------------------------------------------------------------------------
def ordered_sum(v):
    """The float64 sum of v in the order of the device's workgroup sums: partial t = v[t] + v[t + 256] + ... in ascending order
    (t = 0 .. 255), then partial[t] += partial[t + o] for o = 128, 64, .. 1."""
    v = np.asarray(v, dtype=np.float64).ravel()
    m = max(1, -(-v.size // 256))
    pad = np.zeros(m * 256)
    pad[:v.size] = v
    part = np.zeros(256)
    for r in pad.reshape(m, 256):
        part = part + r
    o = 128
    while o >= 1:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return float(part[0])


HostSilhouette = collections.namedtuple("HostSilhouette", "values a b nearest mean cluster_mean")


def silhouette_host(x, labels, metric="euclidean", clusters=None, rows=None):
    """The silhouette in float64 -> HostSilhouette(values, a, b, nearest (int64), mean, cluster_mean (K,)), per queried row (`rows`:
    row indices, None = every row).  d(i, j) = |x_i - x_j| by direct differences (cosine: 1 - x_i . x_j / (|x_i| |x_j|), 1 for a zero
    row), d(i, i) = 0 by position; S(i, c) = the distances to the rows of label c added in ascending row; a = S(i, L) / (count_L -
    1) (0 for a singleton), b = min over the non-empty c != L of S(i, c) / count_c with the lowest c winning a tie (-> nearest),
    s = (b - a) / max(a, b), and 0 when count_L == 1 or max(a, b) == 0.  Empty clusters are skipped; fewer than two non-empty
    clusters: s = 0, b = NaN, nearest = -1.  A label outside [0, clusters) puts its row in no cluster: NaN / -1, and out of the
    mean.  A row that meets a NaN or an infinity: NaN / -1.  mean and cluster_mean by ordered_sum over the queried rows."""
    _check_metric(metric)
    x = np.asarray(x, dtype=np.float64)
    n = retrieval._check_2d(x, "x")[0]
    labels = np.asarray(labels).astype(np.int64)
    _check_labels_shape(labels, n)
    K = int(labels.max()) + 1 if clusters is None else int(clusters)
    _check_clusters(K)
    q = np.arange(n) if rows is None else np.asarray(rows).astype(np.int64)
    valid = (labels >= 0) & (labels < K)
    lab = np.where(valid, labels, K)                         # bin K collects the rows without a cluster
    counts = np.bincount(lab, minlength=K + 1)[:K]
    nonempty = counts > 0
    w = _inv_norms(x) if metric == "cosine" else None
    m = q.size
    a, b, s = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    nearest = np.full(m, -1, dtype=np.int64)
    ql = np.full(m, -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t, i in enumerate(q):
            if not (0 <= i < n) or not valid[i]:
                continue
            L = ql[t] = labels[i]
            if metric == "cosine":
                d = 1.0 - (x @ x[i]) * w * w[i]
            else:
                diff = x - x[i]
                d = np.sqrt((diff * diff).sum(axis=1))
            d[i] = 0.0
            S = np.bincount(lab, weights=d, minlength=K + 1)[:K]
            if not np.isfinite(S[nonempty]).all() or not np.isfinite(x[i]).all():
                continue
            a[t] = S[L] / (counts[L] - 1) if counts[L] > 1 else 0.0
            if nonempty.sum() < 2:
                s[t] = 0.0
                continue
            other = nonempty.copy()
            other[L] = False
            means = np.where(other, S / np.maximum(counts, 1), np.inf)
            nearest[t] = int(np.argmin(means))
            b[t] = means[nearest[t]]
            mx = max(a[t], b[t])
            s[t] = 0.0 if counts[L] == 1 or mx == 0.0 else (b[t] - a[t]) / mx
        cm = np.array([ordered_sum(np.where(ql == c, s, 0.0)) / (ql == c).sum() if (ql == c).any() else np.nan for c in range(K)])
        mean = ordered_sum(np.where(ql >= 0, s, 0.0)) / (ql >= 0).sum() if (ql >= 0).any() else np.nan
    return HostSilhouette(s, a, b, nearest, mean, cm)


HostDispersion = collections.namedtuple("HostDispersion",
                                        "counts means within_sq within_dist grand_mean calinski_harabasz davies_bouldin")


def _row_sq(diff):
    """sum_j diff_j^2 per row in the device's order: lane l = 0 .. 63 takes columns 4 l .. 4 l + 3, + 256, ... in ascending order
    (v = v + d * d, every operation rounded), the lanes join by the xor butterfly 32, 16, .. 1."""
    r, dim = diff.shape
    groups = -(-dim // 256)
    sq = np.zeros((r, groups * 256))
    sq[:, :dim] = diff * diff
    sq = sq.reshape(r, groups, 64, 4)
    v = np.zeros((r, 64))
    for g in range(groups):
        for c in range(4):
            v = v + sq[:, g, :, c]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def _sum4(rows):
    """Rows added as the device adds a cluster's rows: position j goes to partial j mod 4, each partial in ascending j, joined as
    ((p0 + p1) + p2) + p3."""
    rows = np.asarray(rows, dtype=np.float64)
    p = []
    for wv in range(4):
        part = rows[wv::4]
        p.append(np.cumsum(part, axis=0)[-1] if part.shape[0] else np.zeros(rows.shape[1:]))
    return ((p[0] + p[1]) + p[2]) + p[3]


def _dispersion_scores(counts, means, within_sq, within_dist, grand):
    """(calinski_harabasz, davies_bouldin) from the per-cluster quantities, as scikit-learn forms them; NaN with fewer than two
    non-empty clusters."""
    counts = np.asarray(counts, dtype=np.int64)
    ne = counts > 0
    k, n = int(ne.sum()), int(counts.sum())
    if k < 2:
        return float("nan"), float("nan")
    c, m = counts[ne].astype(np.float64), np.asarray(means, dtype=np.float64)[ne]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        extra = float((c * ((m - grand) ** 2).sum(axis=1)).sum())
        intra = float(np.asarray(within_sq, dtype=np.float64)[ne].sum())
        ch = 1.0 if intra == 0.0 else (float("nan") if n == k else extra * (n - k) / (intra * (k - 1.0)))
        spread = np.asarray(within_dist, dtype=np.float64)[ne] / c
        cd = np.zeros((k, k))
        for i in range(k):
            cd[i] = np.sqrt(((m - m[i]) ** 2).sum(axis=1))
        if np.allclose(spread, 0) or np.allclose(cd, 0):
            return ch, 0.0
        cd[cd == 0] = np.inf
        db = float(np.mean(np.max((spread[:, None] + spread[None, :]) / cd, axis=1)))
    return ch, db


def dispersion_host(x, labels, clusters=None):
    """The within-cluster dispersion in float64 -> HostDispersion(counts, means (K, dim), within_sq, within_dist, grand_mean,
    calinski_harabasz, davies_bouldin), in the device's documented order (include/acx.h): a cluster's rows are taken in ascending
    row index; its mean is their sum (position j in partial j mod 4, joined in order) over the count; per row sum (x - mean)^2 by
    direct differences; within_sq / within_dist add those and their square roots the same way.  An empty cluster has mean 0 and
    takes no part in the scores; labels outside [0, clusters) are in no cluster."""
    x = np.asarray(x, dtype=np.float64)
    n, dim = retrieval._check_2d(x, "x")
    labels = np.asarray(labels).astype(np.int64)
    _check_labels_shape(labels, n)
    K = int(labels.max()) + 1 if clusters is None else int(clusters)
    _check_clusters(K)
    counts = np.zeros(K, dtype=np.int64)
    means, sums = np.zeros((K, dim)), np.zeros((K, dim))
    wsq, wd = np.zeros(K), np.zeros(K)
    for c in range(K):
        rows = x[labels == c]
        counts[c] = rows.shape[0]
        if not counts[c]:
            continue
        sums[c] = _sum4(rows)
        means[c] = sums[c] / counts[c]
        v = _row_sq(rows - means[c])
        wsq[c], wd[c] = _sum4(v), _sum4(np.sqrt(v))
    total = int(counts.sum())
    grand = np.zeros(dim)
    for c in range(K):
        if counts[c]:
            grand = grand + sums[c]
    with np.errstate(invalid="ignore", divide="ignore"):
        grand = grand / total
    ch, db = _dispersion_scores(counts, means, wsq, wd, grand)
    return HostDispersion(counts, means, wsq, wd, grand, ch, db)


HostAgreement = collections.namedtuple("HostAgreement", "contingency ari nmi homogeneity completeness v_measure purity")


def _entropy(counts):
    pi = counts[counts > 0].astype(np.float64)
    if pi.size <= 1:
        return 0.0
    tot = pi.sum()
    return float(-np.sum((pi / tot) * (np.log(pi) - np.log(tot))))


def _agreement_scores(table):
    """ARI, NMI (arithmetic normalisation), homogeneity, completeness, V-measure and purity from an integer contingency table
    (rows: labels_a, columns: labels_b), as scikit-learn 1.7 forms them."""
    t = np.asarray(table, dtype=np.int64)
    n = int(t.sum())
    ra, cb = t.sum(axis=1), t.sum(axis=0)
    nzx, nzy = np.nonzero(t)
    cells = t[nzx, nzy]
    # adjusted Rand index from the pair confusion matrix: sums of squares fit int64 (n <= 2^30), the products are Python integers
    sq = int((cells * cells).sum())
    c11 = sq - n
    c01 = int((cb * cb).sum()) - sq
    c10 = int((ra * ra).sum()) - sq
    c00 = n * n - c01 - c10 - sq
    tn, fp, fn, tp = c00, c01, c10, c11
    ari = 1.0 if (fn == 0 and fp == 0) else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    # mutual information
    nz = cells.astype(np.float64)
    outer = ra[nzx].astype(np.int64) * cb[nzy].astype(np.int64)
    log_outer = -np.log(outer) + np.log(float(ra.sum())) + np.log(float(cb.sum()))
    mi = (nz / n) * (np.log(nz) - np.log(float(n))) + (nz / n) * log_outer
    mi = np.where(np.abs(mi) < np.finfo(mi.dtype).eps, 0.0, mi)
    mi = float(np.clip(mi.sum(), 0.0, None))
    ha, hb = _entropy(ra), _entropy(cb)
    ka, kb = int((ra > 0).sum()), int((cb > 0).sum())
    if ka == kb == 1 or ka == kb == 0:
        nmi = 1.0
    elif mi == 0.0:
        nmi = 0.0
    else:
        nmi = mi / ((ha + hb) / 2.0)
    hom = mi / ha if ha else 1.0
    com = mi / hb if hb else 1.0
    v = 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)
    purity = float(t.max(axis=0).sum()) / n if n else float("nan")
    return float(ari), float(nmi), float(hom), float(com), float(v), purity


def _label_pair(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 1 or a.shape != b.shape or a.size < 1:
        raise ValueError("labels_a and labels_b must be 1-D of one length >= 1, got shapes %s and %s" % (a.shape, b.shape))
    return a.astype(np.int64), b.astype(np.int64)


def agreement_host(labels_a, labels_b, clusters_a=None, clusters_b=None):
    """How two labellings of the same rows agree -> HostAgreement(contingency (ka, kb) int64, ari, nmi, homogeneity, completeness,
    v_measure, purity).  labels_a is the reference for homogeneity / completeness / purity (purity = sum over the clusters of b of
    their largest class of a, over n).  Pairs with a label outside its range are counted nowhere."""
    a, b = _label_pair(labels_a, labels_b)
    ka = int(a.max()) + 1 if clusters_a is None else int(clusters_a)
    kb = int(b.max()) + 1 if clusters_b is None else int(clusters_b)
    ok = (a >= 0) & (a < ka) & (b >= 0) & (b < kb)
    table = np.zeros((max(ka, 1), max(kb, 1)), dtype=np.int64)
    np.add.at(table, (a[ok], b[ok]), 1)
    return HostAgreement(table, *_agreement_scores(table))


# ---- the device path -------------------------------------------------------------------------------------------------------
def _status_error(st):
    if st & _ffi.CLUSTER_NONFINITE:
        return "the embeddings hold NaN or infinite values"
    if st & _ffi.CLUSTER_BAD_LABEL:
        return "a label lies outside [0, clusters)"
    if st & _ffi.CLUSTER_BAD_ROW:
        return "a sampled row index lies outside [0, n)"
    if st & _ffi.CLUSTER_DEGENERATE:
        return "fewer than two non-empty clusters"
    return None


def _labels32(labels, n, dev, name="labels"):
    """labels (n,) of any integer type, anywhere -> int32 on dev."""
    _check_labels_shape(labels, n, name)
    if not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("%s must be integers, got %s" % (name, labels.dtype))
    return labels.detach().to(device=dev, dtype=torch.int32).contiguous()


def _clusters_of(labels, clusters):
    """clusters, or max(labels) + 1 read back from the device (one synchronisation: pass clusters to avoid it)."""
    if clusters is None:
        clusters = max(int(labels.max().cpu()) + 1, 1)
    _check_clusters(clusters)
    return int(clusters)


class Silhouette:
    """The result of silhouette(): device tensors, nothing synchronised.  values, a, b (m,) float64 and nearest (m,) int64 per
    queried row; mean 0-d float64; cluster_mean (K,) float64 (NaN for a cluster without queried rows); rows: the (m,) int64 row
    indices of a sampled call, None when every row was queried."""

    def __init__(self, values, a, b, nearest, mean, cluster_mean, rows, metric, status):
        self.values, self.a, self.b, self.nearest = values, a, b, nearest
        self.mean, self.cluster_mean, self.rows, self.metric = mean, cluster_mean, rows, metric
        self.device = values.device
        self._status = status

    def check(self):
        """Synchronise: ValueError if the input held NaN or infinite values, a label outside [0, clusters), or fewer than two
        non-empty clusters."""
        msg = _status_error(int(self._status.cpu()[0]))
        if msg:
            raise ValueError(msg)
        return self

    def __float__(self):
        return float(self.mean.cpu())


def _silhouette_rows(x, rx, labels, K, metric, rows=None):
    """silhouette() on rows the kernels can read: x (n, padded dim) fp32 on the device, rx its inverse norms (cosine) or None,
    labels int32 (n,), rows int32 (m,) or None."""
    n, dp = x.shape
    dev = x.device
    m = n if rows is None else rows.shape[0]
    with torch.cuda.device(dev):
        out = torch.empty((3, m), dtype=torch.float64, device=dev)
        nearest = torch.empty(m, dtype=torch.int32, device=dev)
        means = torch.empty(K + 1, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.cluster_scores_workspace_bytes(n, dp, K)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _ffi.silhouette(vp(x), x.stride(0), vp(rx), n, dp, _ffi.KMEANS_METRICS[metric], vp(labels), K, vp(rows), m, vp(out[0]),
                        vp(out[1]), vp(nearest), vp(out[2]), vp(means), vp(means[K:]), vp(status), (vp(ws), ws_bytes),
                        _ffi.stream_ptr(dev))
    return Silhouette(out[2], out[0], out[1], nearest.to(torch.int64), means[K], means[:K],
                      None if rows is None else rows.to(torch.int64), metric, status)


def _sample_rows(n, sample, seed, dev):
    if sample is None:
        return None
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g)[:int(sample)].to(device=dev, dtype=torch.int32)


def silhouette(x, labels, metric="euclidean", clusters=None, sample=None, seed=0, device=None):
    """The silhouette of every row of x (n, dim) under `labels` (n,) on the GPU -> Silhouette.

    metric: "euclidean" or "cosine" (1 - cos).  clusters: labels lie in [0, clusters); None reads max(labels) + 1 back from the
    device (the one synchronisation of this call).  sample=m: only m rows, torch.randperm(n, generator seeded with `seed`)[:m], are
    queried -- against all n rows.  A CUDA tensor is read where it is when its layout allows; see Silhouette.check()."""
    _check_metric(metric)
    n = retrieval._check_2d(x, "x")[0]
    if n < 1:
        raise ValueError("x has no rows")
    _check_labels_shape(labels, n)
    _check_sample(sample, n)
    if clusters is not None:
        _check_clusters(clusters)
    if isinstance(x, torch.Tensor) and x.is_cuda and device is None:
        device = x.device
    dev = _inputs.cuda_device(device, "the cluster scores run on")
    xr = retrieval._rows(x, dev, name="x")
    lab = _labels32(labels, n, dev)
    K = _clusters_of(lab, clusters)
    with torch.cuda.device(dev):
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        rx = retrieval.row_norms(xr, st) if metric == "cosine" else None
    sil = _silhouette_rows(xr, rx, lab, K, metric, _sample_rows(n, sample, seed, dev))
    sil._status.bitwise_or_(((st & _ffi.KNN_NONFINITE) != 0).to(torch.int32) * _ffi.CLUSTER_NONFINITE)
    return sil


class ClusterDispersion:
    """The result of dispersion_scores(): calinski_harabasz and davies_bouldin (Python floats, from float64 host arithmetic on the
    K means), counts (K,) int64, means (K, dim) float64, within (K,) float64 -- each cluster's sum of squared distances to its mean
    -- and within_dist (K,) float64, the sum of the distances, on the device."""

    def __init__(self, calinski_harabasz, davies_bouldin, counts, means, within, within_dist, grand_mean, status):
        self.calinski_harabasz, self.davies_bouldin = calinski_harabasz, davies_bouldin
        self.counts, self.means, self.within, self.within_dist, self.grand_mean = counts, means, within, within_dist, grand_mean
        self.device = counts.device
        self._status = status

    def check(self):
        msg = _status_error(int(self._status.cpu()[0]))
        if msg:
            raise ValueError(msg)
        return self


def _dispersion_rows(x, dim, labels, K):
    n, dp = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        counts = torch.empty(K, dtype=torch.int64, device=dev)
        means = torch.empty((K, dp), dtype=torch.float64, device=dev)
        within = torch.empty((2, K), dtype=torch.float64, device=dev)
        grand = torch.empty(dp, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.cluster_scores_workspace_bytes(n, dp, K)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _ffi.cluster_dispersion(vp(x), x.stride(0), n, dp, vp(labels), K, vp(counts), vp(means), vp(within[0]), vp(within[1]),
                                vp(grand), vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(dev))
        # the K^2 centroid distances of Davies-Bouldin: float64 on the host, from one copy of the per-cluster results
        host = [t.cpu().numpy() for t in (counts, means[:, :dim], within[0], within[1], grand[:dim])]
    ch, db = _dispersion_scores(*host)
    return ClusterDispersion(ch, db, counts, means[:, :dim], within[0], within[1], grand[:dim], status)


def dispersion_scores(x, labels, clusters=None, device=None):
    """Calinski-Harabasz and Davies-Bouldin of x (n, dim) under `labels` on the GPU -> ClusterDispersion.  The per-cluster means
    and dispersions are float64 sums on the device in a fixed order; the two scores are formed from them on the host (one
    synchronisation).  Empty clusters take no part; NaN with fewer than two non-empty clusters."""
    n, dim = retrieval._check_2d(x, "x")
    if n < 1:
        raise ValueError("x has no rows")
    _check_labels_shape(labels, n)
    if clusters is not None:
        _check_clusters(clusters)
    if isinstance(x, torch.Tensor) and x.is_cuda and device is None:
        device = x.device
    dev = _inputs.cuda_device(device, "the cluster scores run on")
    xr = retrieval._rows(x, dev, name="x")
    lab = _labels32(labels, n, dev)
    return _dispersion_rows(xr, dim, lab, _clusters_of(lab, clusters))


class ClusterAgreement(collections.namedtuple("ClusterAgreement", "contingency ari nmi homogeneity completeness v_measure purity")):
    """agreement(): contingency (ka, kb) int64 on the device; ari, nmi (arithmetic normalisation), homogeneity, completeness,
    v_measure and purity as Python floats, float64 host arithmetic on the counts."""


def agreement(labels_a, labels_b, clusters_a=None, clusters_b=None, device=None):
    """How two labellings of the same rows agree, from their contingency table counted on the GPU -> ClusterAgreement.  labels_a is
    the reference for homogeneity / completeness / purity.  clusters_a / clusters_b: the label ranges; None reads max + 1 back from
    the device.  Raises ValueError for a label outside its range."""
    n = tuple(getattr(labels_a, "shape", ()))
    if len(n) != 1 or n[0] < 1:
        raise ValueError("labels_a must be 1-D with at least one entry, got shape %s" % (n,))
    n = n[0]
    if isinstance(labels_a, torch.Tensor) and labels_a.is_cuda and device is None:
        device = labels_a.device
    dev = _inputs.cuda_device(device, "the cluster scores run on")
    a, b = _labels32(labels_a, n, dev, "labels_a"), _labels32(labels_b, n, dev, "labels_b")
    ka, kb = _clusters_of(a, clusters_a), _clusters_of(b, clusters_b)
    if ka * kb > _ffi.CONTINGENCY_MAX_CELLS:
        raise ValueError("a contingency table of %d x %d cells (at most 2^24)" % (ka, kb))
    with torch.cuda.device(dev):
        table = torch.empty((ka, kb), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _ffi.contingency(vp(a), ka, vp(b), kb, n, vp(table), vp(status), _ffi.stream_ptr(dev))
        host, st = table.cpu().numpy(), int(status.cpu()[0])
    if st:
        raise ValueError(_status_error(st))
    return ClusterAgreement(table, *_agreement_scores(host))


ClusterScores = collections.namedtuple("ClusterScores", "silhouette dispersion")
ClusterSelection = collections.namedtuple("ClusterSelection", "ks scores best_k best fits criterion")


def _select(fit, score, ks, criterion):
    """fit(k) -> KMeans, score(km, k) -> a 0-d device tensor or a float; -> ClusterSelection (one synchronisation at the end)."""
    if criterion not in CRITERIA:
        raise ValueError("criterion must be one of %s, got %r" % (CRITERIA, criterion))
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 2:
        raise ValueError("ks = %r (expected one or more integers >= 2)" % (ks,))
    fits = [fit(k) for k in ks]
    dev = fits[0].device
    scores = torch.stack([torch.as_tensor(score(km, k), dtype=torch.float64, device=dev).reshape(()) for km, k in zip(fits, ks)])
    sign = -1.0 if criterion == "davies_bouldin" else 1.0                     # Davies-Bouldin: lower is better
    ranked = torch.where(torch.isnan(scores), torch.full_like(scores, -float("inf")), sign * scores)
    best = int(torch.argmax(ranked).cpu())                                     # the first k among equal scores
    return ClusterSelection(tuple(ks), scores, ks[best], fits[best], fits, criterion)


def select_clusters(emb, ks, criterion="silhouette", metric="euclidean", sample=None, seed=0, device=None, **kmeans_kwargs):
    """Fit kmeans(emb, k, metric, seed=seed, **kmeans_kwargs) for each k of `ks` and score each fit -> ClusterSelection(ks, scores
    (len(ks),) float64 on the device, best_k, best (the KMeans of best_k), fits, criterion).  criterion: "silhouette" (the mean
    silhouette, of `sample` rows when given; highest wins), "calinski_harabasz" (highest) or "davies_bouldin" (lowest); among
    equal scores the first k wins, a NaN score never does.  "silhouette" synchronises once, at the end; the other two once per k."""
    _check_metric(metric)
    n, dim = retrieval._check_2d(emb, "embeddings")
    _check_sample(sample, n)
    if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
        device = emb.device
    dev = _inputs.cuda_device(device, "the clustering runs on")
    x = retrieval._rows(emb, dev)
    with torch.cuda.device(dev):
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        rx = retrieval.row_norms(x, st) if metric == "cosine" else None
    rows = _sample_rows(n, sample, seed, dev)

    def fit(k):
        clustering._check_fit_args((n, dim), k, metric, kmeans_kwargs.get("init", "k-means++"), kmeans_kwargs.get("n_init", 1),
                                   kmeans_kwargs.get("max_iter", 100), kmeans_kwargs.get("tol", 1e-4))
        return clustering._fit_rows(x, dim, rx, k, metric, seed=seed, **kmeans_kwargs)

    def score(km, k):
        lab = km.labels.to(torch.int32)
        if criterion == "silhouette":
            return _silhouette_rows(x, rx, lab, k, metric, rows).mean
        d = _dispersion_rows(x, dim, lab, k)
        return d.calinski_harabasz if criterion == "calinski_harabasz" else d.davies_bouldin

    return _select(fit, score, ks, criterion)
