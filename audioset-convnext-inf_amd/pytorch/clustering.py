"""K-means over embeddings on the GPU (acx_kmeans_* in include/acx.h): Lloyd iterations with k-means++ seeding, for the
embeddings that have no labels -- what `sklearn.cluster.KMeans(...).fit(emb)` does on the host.

    from audioset_convnext_inf_amd.pytorch.clustering import kmeans, KMeans
    km = kmeans(emb, clusters=50, metric="euclidean", init="k-means++", n_init=1, max_iter=100, tol=1e-4, seed=0)
    km.centers, km.labels, km.counts          # (K, dim) fp32, (n,) int64, (K,) int64 device tensors
    km.inertia, km.n_iter, km.converged       # 0-d device tensors
    km.predict(x), km.distances(x)            # labels / winner distances of new rows
    km.silhouette(emb, sample=None)           # how good the clustering is (pytorch/cluster_scores.py)
    km.check()                                # the one call that synchronises
    km.save("km.npz"); KMeans.load("km.npz")

Order: a row goes to the centre of the lowest fp32 score, then the lowest centre index, -0.0 as +0.0 -- one total order, so a
label does not depend on how the kernel got there; the (n x K) score matrix is never written.  The centre update partitions the
rows stably by label and sums in float64 in a fixed order: no float atomics, the same inputs give the same bits.  The stop
(no label changed, or the squared centre shift <= tol * mean(var(x, axis=0)), scikit-learn's rule) is decided on the device: the
host queues max_iter iterations and nothing synchronises, so a whole fit can be captured in a torch.cuda.graph.

Differences from scikit-learn: an EMPTY cluster keeps its previous centre and reports count 0 (scikit-learn moves it to the row
farthest from its centre); `check()` warns about it.  metric="cosine" is spherical k-means: rows weighted by their inverse norm,
centres renormalised to unit length.

`kmeans_host`, `assign_host`, `sample_host` and `seed_host` are the documented host definitions in numpy float64 (the tests'
reference)."""
import collections
import warnings

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs
from . import retrieval

METRICS = tuple(_ffi.KMEANS_METRICS)
INITS = ("k-means++", "random")
MAX_CLUSTERS = _ffi.KMEANS_MAX_CLUSTERS
MAX_ITER = _ffi.KMEANS_MAX_ITER


def _check_metric(metric):
    if metric not in _ffi.KMEANS_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (METRICS, metric))


def _check_clusters(clusters, n):
    if isinstance(clusters, bool) or not isinstance(clusters, (int, np.integer)) or not 1 <= clusters <= MAX_CLUSTERS:
        raise ValueError("clusters = %r (expected an integer in 1 .. %d)" % (clusters, MAX_CLUSTERS))
    if clusters > n:
        raise ValueError("clusters = %d exceeds the %d rows" % (clusters, n))


def _check_max_iter(max_iter):
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 1 <= max_iter <= MAX_ITER:
        raise ValueError("max_iter = %r (expected an integer in 1 .. %d)" % (max_iter, MAX_ITER))


# ---- the host definitions (numpy float64) ----------------------------------------------------------------------------------
def _inv_norms(x):
    nrm = np.sqrt((x * x).sum(axis=1))
    return np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)


def assign_host(x, centers, metric="euclidean"):
    """(labels (n,) int64, scores (n,) float64): score[i, k] = sum c_k^2 - 2 x_i . c_k (cosine: -x_i . c_k with the raw row),
    the label the first arg-min (lowest centre index among equal scores, -0.0 as +0.0), scores[i] = score[i, labels[i]]."""
    _check_metric(metric)
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(centers, dtype=np.float64)
    xs, cs = retrieval._check_2d(x, "x"), retrieval._check_2d(c, "centers")
    if xs[1] != cs[1]:
        raise ValueError("x has dim %d, the centers dim %d" % (xs[1], cs[1]))
    s = -(x @ c.T) if metric == "cosine" else (c * c).sum(axis=1)[None, :] - 2.0 * (x @ c.T)
    s = s + 0.0
    labels = np.argmin(s, axis=1).astype(np.int64)
    return labels, s[np.arange(xs[0]), labels]


HostKMeans = collections.namedtuple("HostKMeans", "centers labels counts inertia n_iter converged")


def _update_host(x, w, labels, old, metric, round_centers):
    K = old.shape[0]
    onehot = np.zeros((K, x.shape[0]))
    onehot[labels, np.arange(x.shape[0])] = 1.0
    counts = onehot.sum(axis=1).astype(np.int64)
    sums = onehot @ (x * w[:, None] if metric == "cosine" else x)
    new = old.copy()
    if metric == "cosine":
        nrm = np.sqrt((sums * sums).sum(axis=1))
        ok = (counts > 0) & (nrm > 0)
        new[ok] = sums[ok] / nrm[ok, None]
    else:
        ok = counts > 0
        new[ok] = sums[ok] / counts[ok, None]
    if round_centers:
        new = new.astype(np.float32).astype(np.float64)
    return new, counts


def kmeans_host(x, init_centers, metric="euclidean", max_iter=100, tol_abs=0.0, round_centers=True):
    """Lloyd's algorithm as the device runs it -> HostKMeans(centers float32 (float64 with round_centers=False), labels, counts,
    inertia, n_iter, converged).  Per iteration: assign_host, the per-cluster mean (cosine: rows weighted by their inverse norm,
    the mean renormalised to unit length; an empty cluster keeps its centre), rounded to float32 as the device stores it; stop
    when no label changed or sum |c_new - c_old|^2 <= tol_abs.  Labels, counts and inertia belong to the returned centres."""
    _check_metric(metric)
    _check_max_iter(max_iter)
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(init_centers, dtype=np.float64)
    if round_centers:
        c = c.astype(np.float32).astype(np.float64)
    w = _inv_norms(x)
    if metric == "cosine":
        c = c * _inv_norms(c)[:, None]
        if round_centers:
            c = c.astype(np.float32).astype(np.float64)
    old_labels = np.full(x.shape[0], -1, dtype=np.int64)
    converged = strict = False
    n_iter = 0
    for it in range(max_iter):
        labels, scores = assign_host(x, c, metric)
        new, counts = _update_host(x, w, labels, c, metric, round_centers)
        shift = float(((new - c) ** 2).sum())
        c = new
        n_iter = it + 1
        if np.array_equal(labels, old_labels):
            converged = strict = True
            break
        if shift <= tol_abs:
            converged = True
            break
        old_labels = labels
    if not strict:
        labels, scores = assign_host(x, c, metric)
        counts = np.bincount(labels, minlength=c.shape[0]).astype(np.int64)
    if metric == "cosine":
        inertia = float((1.0 + scores * w).sum())
    else:
        inertia = float(np.maximum((x * x).sum(axis=1) + scores, 0.0).sum())
    return HostKMeans(c.astype(np.float32) if round_centers else c, labels, counts, inertia, n_iter, converged)


def sample_host(d, u):
    """The row D^2 sampling picks for the float32 weights d >= 0 and the uniform draw u in [0, 1): integer weights
    q_i = floor(d_i 2^(30 - e)) with e = floor(log2 max d), t = min(floor(u total), total - 1), and the smallest i whose inclusive
    prefix sum of q exceeds t.  -1 when every weight is zero."""
    d = np.asarray(d, dtype=np.float32)
    if d.ndim != 1 or d.size < 1:
        raise ValueError("d must be a non-empty 1-D array, got shape %s" % (d.shape,))
    m = d.max()
    if not m > 0:
        return -1
    e = int(np.frexp(m)[1]) - 1
    q = np.floor(np.ldexp(d, 30 - e)).astype(np.uint64)
    c = np.cumsum(q, dtype=np.uint64)
    total = int(c[-1])
    t = min(int(np.floor(np.float64(u) * np.float64(total))), total - 1)
    return int(np.searchsorted(c, np.uint64(t), side="right"))


def _distance_host(x, c, metric):
    if metric == "cosine":
        cn = np.sqrt((c * c).sum())
        cos = (x @ c) * _inv_norms(x) * (1.0 / cn if cn > 0 else 0.0)
        return np.maximum(2.0 - 2.0 * cos, 0.0)
    return ((x - c[None, :]) ** 2).sum(axis=1)


def seed_host(x, clusters, uniforms, metric="euclidean", d_rounds=None):
    """k-means++ as the device runs it -> (picked (clusters,) int64 row indices, degenerate bool).  picked[0] =
    floor(uniforms[0] n); round r = 1 .. clusters - 1 lowers d_i to the distance to row picked[r - 1] (squared Euclidean, or
    max(0, 2 - 2 cos), as float32) and picks sample_host(d, uniforms[r]); a round whose weights are all zero takes the lowest row
    index not yet picked and makes `degenerate` true.  d_rounds: optional callable (r, picked_so_far) -> the float32 d array of
    round r, used instead of the float64 distances (the tests feed the device's own arrays)."""
    _check_metric(metric)
    x = np.asarray(x, dtype=np.float64)
    n = retrieval._check_2d(x, "x")[0]
    _check_clusters(clusters, n)
    u = np.asarray(uniforms, dtype=np.float64)
    if u.ndim != 1 or u.size < clusters:
        raise ValueError("uniforms must hold at least %d draws, got shape %s" % (clusters, u.shape))
    picked = [min(int(np.floor(u[0] * np.float64(n))), n - 1)]
    degenerate = False
    d = None
    for r in range(1, clusters):
        if d_rounds is not None:
            d = np.asarray(d_rounds(r, list(picked)), dtype=np.float32)
        else:
            new = _distance_host(x, x[picked[-1]], metric).astype(np.float32)
            d = new if d is None else np.minimum(d, new)
        i = sample_host(d, u[r])
        if i < 0:
            degenerate = True
            taken = set(picked)
            i = next(j for j in range(n) if j not in taken)
        picked.append(i)
    return np.asarray(picked, dtype=np.int64), degenerate


# ---- the device path -------------------------------------------------------------------------------------------------------
class KMeans:
    """The result of kmeans(): device tensors, nothing synchronised.  centers (K, dim) fp32 (unit rows for "cosine"), labels
    (n,) int64 (-1 everywhere after non-finite input), counts (K,) int64, inertia (float64), n_iter (int32) and converged (bool)
    as 0-d tensors, metric."""

    def __init__(self, centers, labels, counts, inertia, n_iter, converged, metric, status=None):
        _check_metric(metric)
        self.centers, self.labels, self.counts = centers, labels, counts
        self.inertia, self.n_iter, self.converged = inertia, n_iter, converged
        self.metric = metric
        self.device = centers.device
        self._status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=self.device)
        self._padded = None

    def _centre_rows(self):
        if self._padded is None:
            self._padded = retrieval._rows(self.centers, self.device, name="centers")
        return self._padded

    def _assign(self, x):
        x = retrieval._rows(x, self.device, self.centers.shape[1], "x")
        c = self._centre_rows()
        n, dev = x.shape[0], self.device
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        scores = torch.empty(n, dtype=torch.float32, device=dev)
        rx = None
        if n:
            words = torch.empty(3, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                if self.metric == "cosine":
                    rx = retrieval.row_norms(x, self._status)
                _ffi.kmeans_assign(vp(x), x.stride(0), vp(rx), n, vp(c), c.stride(0), c.shape[0], x.shape[1],
                                   _ffi.KMEANS_METRICS[self.metric], None, vp(labels), vp(scores), vp(words[1:]), vp(words),
                                   _ffi.stream_ptr(dev))
            self._status.bitwise_or_(words[:1])
        return x, rx, labels, scores

    def predict(self, x):
        """(rows,) int64: the label of each row of x (rows, dim) -- the assignment kernel against the stored centres."""
        return self._assign(x)[2].to(torch.int64)

    def distances(self, x):
        """(rows,) fp32: each row's distance to its own centre -- squared Euclidean, or 1 - cos for "cosine"."""
        x, rx, _, scores = self._assign(x)
        if self.metric == "cosine":
            return 1.0 + scores * rx
        return ((x * x).sum(dim=1) + scores).clamp_min(0.0)

    def silhouette(self, x, sample=None, seed=0):
        """The silhouette of the rows x (n, dim) this clustering was fitted on, under its labels and metric
        (pytorch/cluster_scores.py: silhouette; sample, seed as there) -> cluster_scores.Silhouette."""
        from . import cluster_scores
        return cluster_scores.silhouette(x, self.labels, self.metric, clusters=self.centers.shape[0], sample=sample, seed=seed,
                                         device=self.device)

    def check(self):
        """Synchronise: ValueError if the input held NaN or infinite values; RuntimeWarning (warnings.warn) for degenerate
        seeding (fewer distinct rows than clusters) or empty clusters."""
        st = int(self._status.cpu()[0])
        if st & _ffi.KMEANS_NONFINITE:
            raise ValueError("the embeddings or the centers hold NaN or infinite values")
        if st & _ffi.KMEANS_DEGENERATE:
            warnings.warn("k-means++ ran out of distinct rows: fewer distinct rows than clusters", RuntimeWarning)
        empty = int((self.counts == 0).sum().cpu())
        if empty:
            warnings.warn("%d empty cluster(s) kept their previous centre" % empty, RuntimeWarning)
        return self

    def save(self, path):
        np.savez(path, method="kmeans", metric=self.metric, centers=self.centers.cpu().numpy(), labels=self.labels.cpu().numpy(),
                 counts=self.counts.cpu().numpy(), inertia=self.inertia.cpu().numpy(), n_iter=self.n_iter.cpu().numpy(),
                 converged=self.converged.cpu().numpy())

    @classmethod
    def load(cls, path, device=None):
        dev = _inputs.cuda_device(device, "a clustering is applied on")
        with np.load(path) as f:
            if str(f["method"]) != "kmeans":
                raise ValueError("%s holds %s, not a k-means clustering" % (path, f["method"]))
            metric = str(f["metric"])
            centers, labels, counts = f["centers"], f["labels"], f["counts"]
            inertia, n_iter, converged = f["inertia"], f["n_iter"], f["converged"]
        if centers.ndim != 2 or not np.isfinite(centers).all():
            raise ValueError("%s: centers must be a finite (K, dim) array" % path)
        t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(dev)
        return cls(t(centers, torch.float32).contiguous(), t(labels, torch.int64), t(counts, torch.int64), t(inertia, torch.float64),
                   t(n_iter, torch.int32), t(converged, torch.bool), metric)


def _tol_abs(x, dim, rx, tol):
    """tol * mean(var(x, axis=0)) as a float64 device tensor (1,), in float64 torch ops on the stream (cosine: of the unit rows)."""
    n = x.shape[0]
    s1 = torch.zeros(dim, dtype=torch.float64, device=x.device)
    s2 = torch.zeros(dim, dtype=torch.float64, device=x.device)
    for a in range(0, n, 16384):
        chunk = x[a:a + 16384, :dim].to(torch.float64)
        if rx is not None:
            chunk = chunk * rx[a:a + 16384, None].to(torch.float64)
        s1 += chunk.sum(dim=0)
        s2 += (chunk * chunk).sum(dim=0)
    var = (s2 / n - (s1 / n) ** 2).clamp_min(0.0)
    return (var.mean() * float(tol)).reshape(1)


def _fit_rows(x, dim, rx, clusters, metric, init="k-means++", n_init=1, max_iter=100, tol=1e-4, seed=0):
    """kmeans() on rows the kernels can read: x (n, padded dim) fp32 on the device, rx its inverse norms (cosine) or None."""
    n, dp = x.shape
    dev = x.device
    K = int(clusters)
    cosine = metric == "cosine"
    code = _ffi.KMEANS_METRICS[metric]
    init_rows = None
    if not isinstance(init, str):
        init_rows = retrieval._rows(init, dev, dim, "init")
    with torch.cuda.device(dev):
        stream = _ffi.stream_ptr(dev)
        tol_abs = _tol_abs(x, dim, rx, tol)
        ws_bytes = _ffi.kmeans_workspace_bytes(n, dp, K)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        best = None
        for run in range(int(n_init)):
            centers = torch.zeros((K, dp), dtype=torch.float32, device=dev)
            seed_status = torch.zeros(1, dtype=torch.int32, device=dev)
            if init_rows is not None:
                centers[:, :init_rows.shape[1]] = init_rows
                if cosine:
                    centers *= retrieval.row_norms(centers, seed_status)[:, None]
            elif init == "random":
                idx = np.random.default_rng(seed + run).choice(n, K, replace=False)
                centers.copy_(x.index_select(0, torch.from_numpy(idx).to(dev)))
                if cosine:
                    centers *= retrieval.row_norms(centers, seed_status)[:, None]
            else:
                u = torch.from_numpy(np.random.default_rng(seed + run).random(K + 1)).to(dev)
                picked = torch.empty(K, dtype=torch.int32, device=dev)
                _ffi.kmeans_seed(vp(x), x.stride(0), vp(rx), n, dp, code, K, vp(u), vp(picked), vp(centers), centers.stride(0),
                                 vp(seed_status), (vp(ws), ws_bytes), stream)
            labels = torch.empty(n, dtype=torch.int32, device=dev)
            counts = torch.empty(K, dtype=torch.int32, device=dev)
            state = torch.zeros(4, dtype=torch.float64, device=dev)          # struct acx_kmeans_state
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _ffi.kmeans_fit(vp(x), x.stride(0), vp(rx), n, dp, code, vp(centers), centers.stride(0), K, int(max_iter), vp(tol_abs),
                            vp(labels), vp(counts), vp(state), vp(status), (vp(ws), ws_bytes), stream)
            status = status | seed_status
            cur = [centers, labels, counts, state, status]
            if best is None:
                best = cur
            else:
                better = cur[3][3] < best[3][3]                              # a NaN inertia never wins
                best = [torch.where(better, c, b) for c, b in zip(cur, best)]
        centers, labels, counts, state, status = best
        words = state.view(torch.int32)
        finite = (status & _ffi.KMEANS_NONFINITE) == 0
        return KMeans(centers[:, :dim], labels.to(torch.int64), counts.to(torch.int64), state[3], words[0],
                      (words[1] != 0) & finite[0], metric, status)


def _check_fit_args(shape, clusters, metric, init, n_init, max_iter, tol):
    _check_metric(metric)
    _check_clusters(clusters, shape[0])
    _check_max_iter(max_iter)
    if isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or n_init < 1:
        raise ValueError("n_init = %r (expected an integer >= 1)" % (n_init,))
    if not tol >= 0:
        raise ValueError("tol = %r (expected >= 0)" % (tol,))
    if isinstance(init, str):
        if init not in INITS:
            raise ValueError("init must be one of %s or a (clusters, dim) array, got %r" % (INITS, init))
    else:
        ishape = retrieval._check_2d(init, "init")
        if ishape != (clusters, shape[1]):
            raise ValueError("init has shape %s (expected (clusters, dim) = %s)" % (ishape, (clusters, shape[1])))


def kmeans(emb, clusters, metric="euclidean", init="k-means++", n_init=1, max_iter=100, tol=1e-4, seed=0, device=None):
    """Cluster the rows of emb (n, dim) into `clusters` clusters on the GPU -> KMeans.

    metric: "euclidean" or "cosine" (spherical k-means).  init: "k-means++" (D^2 sampling on the device with the K + 1 uniforms
    of numpy.random.default_rng(seed).random(K + 1)), "random" (default_rng(seed).choice(n, K, replace=False), gathered on the
    device) or a (K, dim) array of initial centres.  n_init > 1 runs seeds seed, seed + 1, ... and keeps the lowest inertia
    (chosen on the device).  tol: relative to the mean variance of the columns, as in scikit-learn.  A CUDA tensor is read where
    it is when its layout allows; nothing synchronises with the host -- see KMeans.check()."""
    shape = retrieval._check_2d(emb, "embeddings")
    _check_fit_args(shape, clusters, metric, init, n_init, max_iter, tol)
    if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
        device = emb.device
    dev = _inputs.cuda_device(device, "the clustering runs on")
    x = retrieval._rows(emb, dev)
    with torch.cuda.device(dev):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rx = retrieval.row_norms(x, status) if metric == "cosine" else None
    km = _fit_rows(x, shape[1], rx, clusters, metric, init, n_init, max_iter, tol, seed)
    km._status.bitwise_or_(status)
    return km
