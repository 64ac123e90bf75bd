"""Radius search, near-duplicate groups and DBSCAN on the GPU (acx_radius_count, acx_radius_neighbors, acx_graph_components,
acx_dbscan_labels in include/acx.h): which rows lie within a given distance of each other -- what
`sklearn.neighbors.radius_neighbors`, a union-find over the pairs and `sklearn.cluster.DBSCAN(algorithm="brute")` answer on the host.

    from audioset_convnext_inf_amd.pytorch.neighbors import radius_neighbors, duplicate_groups, cross_duplicates, dbscan
    nb = radius_neighbors(None, emb, 0.9, metric="cosine")    # a self-join: every row against the others
    nb.offsets, nb.indices, nb.values, nb.counts, nb.total    # CSR: int64 (n + 1,), int64, fp32, int64 (n,), int
    dup = duplicate_groups(emb, threshold=0.95)               # dup.labels, dup.sizes, dup.keep, dup.pairs, dup.groups()
    leak = cross_duplicates(test_emb, train_emb, 0.95)        # leak.counts > 0: test rows with a near-duplicate in the training set
    db = dbscan(emb, eps=0.5, min_samples=5)                  # db.labels (-1: noise), db.core, db.counts, db.clusters, db.noise

One fused kernel forms the pair values tile by tile on the f32 matrix cores and turns each tile into keep bits at once; neither the
(nq, n) values nor a mask are ever written.  A list is CSR with each row in ascending database index and is a pure function of the
inputs: the same bytes on every run and for every slicing.  A cosine or dot value has the bits EmbeddingIndex.search gives that
pair; cosine bits are not symmetric in (i, j), so everything built on a list treats an edge as undirected.

`radius_host`, `components_host` and `dbscan_host` are the host definitions in numpy (the tests' reference)."""
import collections

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs
from . import retrieval

METRICS = tuple(_ffi.RADIUS_METRICS)
# Rounds of hooking + pointer jumping queued per call.  No bound on the rounds a graph needs is claimed (a hook can be lost to a race
# and is then found again a round later): a call that was not stable sets ACX_GRAPH_NOT_CONVERGED, check() raises, and
# components(labels=) resumes.  The duplicate graphs and a shuffled path of 4 097 nodes measured needed 2 to 8.
MAX_ROUNDS = 32


def _check_metric(metric):
    if metric not in _ffi.RADIUS_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (METRICS, metric))


def _check_threshold(threshold, metric):
    t = float(threshold)
    if t != t:
        raise ValueError("threshold is NaN")
    if metric == "euclidean" and t < 0:
        raise ValueError("eps = %r (expected >= 0)" % (threshold,))
    return t


def _check_min_samples(min_samples):
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or min_samples < 1:
        raise ValueError("min_samples = %r (expected an integer >= 1)" % (min_samples,))


def level_of(threshold, metric):
    """The fp32 level a pair value is compared with: the threshold itself (dot, cosine: kept iff v >= level), or eps * eps
    evaluated in double and rounded to fp32 (euclidean: kept iff the squared distance <= level)."""
    t = _check_threshold(threshold, metric)
    return np.float32(t * t) if metric == "euclidean" else np.float32(t)


# ---- the host definitions ------------------------------------------------------------------------------------------------------
HostRadius = collections.namedtuple("HostRadius", "offsets indices values counts")


def pair_values_host(queries, emb, metric="cosine"):
    """(nq, n) float64 pair values: the dot products, cosine: times 1 / norm of each side (0 for a zero row), euclidean: the squared
    distances by direct differences."""
    _check_metric(metric)
    q = np.asarray(queries, dtype=np.float64)
    d = np.asarray(emb, dtype=np.float64)
    qs, ds = retrieval._check_2d(q, "queries"), retrieval._check_2d(d, "emb")
    if qs[1] != ds[1]:
        raise ValueError("queries have dim %d, the embeddings dim %d" % (qs[1], ds[1]))
    if metric == "euclidean":
        v = np.empty((qs[0], ds[0]))
        for i in range(qs[0]):
            diff = d - q[i]
            v[i] = (diff * diff).sum(axis=1)
        return v
    v = q @ d.T
    if metric == "cosine":
        def inv(x):
            nrm = np.sqrt((x * x).sum(axis=1))
            return np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
        v = v * inv(q)[:, None] * inv(d)[None, :]
    return v


def radius_host(queries, emb, threshold, metric="cosine", include_self=False, values=None):
    """The neighbour lists in numpy -> HostRadius(offsets (nq + 1) int64, indices int64, values, counts (nq) int64), each row in
    ascending database index.  queries None: a self-join of emb, the pair (i, i) kept iff include_self, by position.  The pair
    (i, j) is kept iff v >= level (dot, cosine) or v <= level (euclidean), level = level_of(threshold, metric) -- inclusive: a value
    exactly at the level is kept; a NaN never is.  values None: v = pair_values_host in float64; values (nq, n): those instead (the
    device's own fp32 bits, to feed the graph definitions)."""
    level = np.float64(level_of(threshold, metric))
    self_join = queries is None
    if values is None:
        v = pair_values_host(emb if self_join else queries, emb, metric)
    else:
        v = np.asarray(values)
        level = level_of(threshold, metric).astype(v.dtype) if v.dtype == np.float32 else level
    with np.errstate(invalid="ignore"):
        keep = v <= level if metric == "euclidean" else v >= level
    if self_join:
        if v.shape[0] != v.shape[1]:
            raise ValueError("a self-join needs square values, got %s" % (v.shape,))
        np.fill_diagonal(keep, bool(include_self))
    counts = keep.sum(axis=1).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows, cols = np.nonzero(keep)                       # row-major: ascending row, then ascending column
    return HostRadius(offsets, cols.astype(np.int64), v[rows, cols], counts)


def _csr(offsets, indices, n=None):
    offsets = np.asarray(offsets).astype(np.int64)
    indices = np.asarray(indices).astype(np.int64)
    if offsets.ndim != 1 or offsets.size < 2:
        raise ValueError("offsets must be 1-D with n + 1 >= 2 entries, got shape %s" % (offsets.shape,))
    if n is not None and offsets.size != n + 1:
        raise ValueError("offsets has %d entries for n = %d rows" % (offsets.size, n))
    return offsets, indices, offsets.size - 1


def components_host(offsets, indices, n=None):
    """labels (n,) int64: the smallest row index of each row's connected component in the UNDIRECTED graph of a self-join list
    ({i, j} is an edge iff (i -> j) or (j -> i) is listed).  An index outside [0, n) is skipped.  Union-find by smallest root."""
    offsets, indices, n = _csr(offsets, indices, n)
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for i in range(n):
        for j in indices[offsets[i]:offsets[i + 1]]:
            if 0 <= j < n:
                a, b = find(i), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


HostDBSCAN = collections.namedtuple("HostDBSCAN", "labels core clusters")


def dbscan_host(offsets, indices, min_samples, n=None):
    """DBSCAN from a self-join list made with include_self=True -> HostDBSCAN(labels (n,) int64, core (n,) bool, clusters).
    core[i] = (row i lists at least min_samples rows, itself included); the clusters are the components of the graph restricted to
    core-core edges, numbered 0, 1, .. in ascending order of their smallest core index; a row that is not core takes the smallest
    cluster number among its core neighbours (undirected); every other row is -1.  scikit-learn's labels, border rows included: it
    expands cluster c completely before it starts c + 1."""
    _check_min_samples(min_samples)
    offsets, indices, n = _csr(offsets, indices, n)
    core = np.diff(offsets) >= min_samples
    rows = np.repeat(np.arange(n), np.diff(offsets))
    ok = (indices >= 0) & (indices < n)
    rows, cols = rows[ok], indices[ok]
    cc = core[rows] & core[cols]
    r2, c2 = rows[cc], cols[cc]
    order = np.argsort(r2, kind="stable")
    cnt = np.bincount(r2, minlength=n)
    comp = components_host(np.concatenate([[0], np.cumsum(cnt)]), c2[order], n)
    roots = np.nonzero(core & (comp == np.arange(n)))[0]
    number = np.full(n, -1, dtype=np.int64)
    number[roots] = np.arange(roots.size)
    labels = np.where(core, number[comp], -1)
    big = np.iinfo(np.int64).max
    border = np.full(n, big, dtype=np.int64)
    for a, b in ((rows, cols), (cols, rows)):               # both directions of every edge
        m = core[b] & ~core[a]
        np.minimum.at(border, a[m], labels[b[m]])
    labels = np.where(~core & (border != big), border, labels)
    return HostDBSCAN(labels.astype(np.int64), core, int(roots.size))


# ---- the device path -------------------------------------------------------------------------------------------------------------
def _status_error(st):
    if st & _ffi.RADIUS_NONFINITE:
        return "the embeddings hold NaN or infinite values"
    if st & _ffi.GRAPH_BAD_INDEX:
        return "a neighbour index lies outside [0, n)"
    if st & _ffi.GRAPH_NOT_CONVERGED:
        return "the components were not stable after max_rounds rounds (pass a larger max_rounds)"
    if st & _ffi.RADIUS_OVERFLOW:
        return "the neighbour list did not fit its capacity"
    return None


class _Checked:
    def check(self):
        """Synchronise: ValueError if the call met bad data (NaN or infinite values, a bad index, components not stable)."""
        msg = _status_error(int(self._status.cpu()[0]))
        if msg:
            raise ValueError(msg)
        return self


def row_sumsq(x):
    """sum x^2 per row of a readable (rows, dim) fp32 device tensor (acx_radius_row_sumsq), on the current stream."""
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _ffi.radius_row_sumsq(vp(x), x.stride(0), x.shape[0], x.shape[1], vp(out), _ffi.stream_ptr(x.device))
    return out


def _aux(x, metric, status):
    """What the radius kernels read per row beside the row: the inverse norms (cosine), sum x^2 (euclidean), nothing (dot)."""
    if metric == "cosine":
        return retrieval.row_norms(x, status)
    return row_sumsq(x) if metric == "euclidean" else None


def _self_mode(self_join, include_self):
    if not self_join:
        return _ffi.RADIUS_SELF_NONE
    return _ffi.RADIUS_SELF_INCLUDE if include_self else _ffi.RADIUS_SELF_EXCLUDE


class RadiusNeighbors(_Checked):
    """The result of radius_neighbors() / cross_duplicates(): a CSR list on the device.  offsets (nq + 1,) int64; indices (total,)
    int64 and values (total,) fp32 (None when not wanted), each row in ascending database index; counts (nq,) int64; total: the
    Python int that was read back to allocate the list (the call's one synchronisation)."""

    def __init__(self, offsets, indices32, values, total, n, metric, status):
        self.offsets, self.indices32, self.values, self.total = offsets, indices32, values, int(total)
        self.n, self.metric = int(n), metric
        self.device = offsets.device
        self._status = status

    @property
    def indices(self):
        return self.indices32.to(torch.int64)

    @property
    def counts(self):
        return self.offsets[1:] - self.offsets[:-1]

    def to_lists(self):
        """[(indices, values)] per query as numpy arrays (values None when not wanted); synchronises."""
        off = self.offsets.cpu().numpy()
        idx = self.indices.cpu().numpy()
        val = None if self.values is None else self.values.cpu().numpy()
        return [(idx[a:b], None if val is None else val[a:b]) for a, b in zip(off[:-1], off[1:])]


def _count_rows(q, q_aux, d, d_aux, metric, level, self_mode, status):
    nq, n, dev = q.shape[0], d.shape[0], d.device
    with torch.cuda.device(dev):
        counts = torch.empty(nq, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.radius_workspace_bytes(nq, n, 0)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _ffi.radius_count(vp(q), q.stride(0), vp(q_aux), nq, vp(d), d.stride(0), vp(d_aux), n, d.shape[1], _ffi.RADIUS_METRICS[metric],
                          level, self_mode, vp(counts), vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(dev))
    return counts


def _neighbors_rows(q, q_aux, d, d_aux, metric, level, self_mode, status, values=True, slices=0):
    """radius_neighbors() on rows the kernels can read: count and scan (acx_radius_neighbors with capacity 0), the total read back --
    the one synchronisation --, a list of exactly that size allocated, and the emit pass (acx_radius_emit): two tile passes.
    status: an int32 device word that receives the call's bits."""
    nq, n, dev = q.shape[0], d.shape[0], d.device
    with torch.cuda.device(dev):
        offsets = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        word = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.radius_workspace_bytes(nq, n, slices)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = _ffi.stream_ptr(dev)
        args = (vp(q), q.stride(0), vp(q_aux), nq, vp(d), d.stride(0), vp(d_aux), n, d.shape[1], _ffi.RADIUS_METRICS[metric], level,
                self_mode, slices, vp(offsets))
        _ffi.radius_neighbors(*args, None, None, 0, vp(total), vp(word), (vp(ws), ws_bytes), stream)
        found = int(total.cpu()[0])                       # the one synchronisation
        idx = torch.empty(found, dtype=torch.int32, device=dev)
        val = torch.empty(found, dtype=torch.float32, device=dev) if values else None
        if found:
            _ffi.radius_emit(*args, vp(idx), vp(val), found, vp(total), vp(word), (vp(ws), ws_bytes), stream)
        else:
            word.bitwise_and_(~_ffi.RADIUS_OVERFLOW)
        status.bitwise_or_(word)
    return RadiusNeighbors(offsets, idx, val, found, n, metric, status)


def _prepare(queries, emb, threshold, metric, device):
    """-> (q rows, q aux, d rows, d aux, level, self_join, status) on the device."""
    _check_metric(metric)
    level = float(level_of(threshold, metric))
    n, dim = retrieval._check_2d(emb, "embeddings")
    if n < 1:
        raise ValueError("the embeddings have no rows")
    if queries is not None:
        nq = retrieval._check_2d(queries, "queries")[0]
        if nq < 1:
            raise ValueError("the queries have no rows")
    if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
        device = emb.device
    dev = _inputs.cuda_device(device, "the radius search runs on")
    d = retrieval._rows(emb, dev)
    with torch.cuda.device(dev):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d_aux = _aux(d, metric, status)
        if queries is None:
            return d, d_aux, d, d_aux, level, True, status
        q = retrieval._rows(queries, dev, dim, "queries")
        return q, _aux(q, metric, status), d, d_aux, level, False, status


def radius_count(queries, emb, threshold, metric="cosine", include_self=False, device=None):
    """How many rows of emb (n, dim) lie within the threshold of each query -> (counts (nq,) int64 on the device, status word).
    queries None: a self-join (every row against the others; include_self counts the row itself).  threshold: the smallest cosine
    or dot product kept, or the radius eps for "euclidean".  Nothing synchronises; no list is written."""
    q, qa, d, da, level, self_join, status = _prepare(queries, emb, threshold, metric, device)
    return _count_rows(q, qa, d, da, metric, level, _self_mode(self_join, include_self), status).to(torch.int64), status


def radius_neighbors(queries, emb, threshold, metric="cosine", include_self=False, values=True, slices=0, device=None):
    """The rows of emb (n, dim) within the threshold of each query, as a CSR list on the GPU -> RadiusNeighbors.  queries None: a
    self-join.  threshold: the smallest cosine or dot product kept, or the radius eps for "euclidean" (values are then SQUARED
    distances); a value exactly at the level is kept.  slices: the ranges of database rows the kernels cut (0: by launch size); the
    list is the same bytes for every slicing.  One synchronisation: the total is read back to allocate the list."""
    q, qa, d, da, level, self_join, status = _prepare(queries, emb, threshold, metric, device)
    if isinstance(slices, bool) or not isinstance(slices, (int, np.integer)) or not 0 <= slices <= _ffi.RADIUS_MAX_SLICES:
        raise ValueError("slices = %r (expected an integer in 0 .. %d)" % (slices, _ffi.RADIUS_MAX_SLICES))
    return _neighbors_rows(q, qa, d, da, metric, level, _self_mode(self_join, include_self), status, values, int(slices))


def _check_rounds(max_rounds):
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or not 1 <= max_rounds <= _ffi.GRAPH_MAX_ROUNDS:
        raise ValueError("max_rounds = %r (expected an integer in 1 .. %d)" % (max_rounds, _ffi.GRAPH_MAX_ROUNDS))


def components(offsets, indices32, n, status=None, max_rounds=MAX_ROUNDS, labels=None):
    """labels (n,) int32 on the device: the smallest row index of each row's component in the undirected graph of a self-join list
    (offsets (n + 1,) int64, indices32 int32, device tensors) by acx_graph_components.  labels given: continue from them (resume).
    status: an int32 device word that receives ACX_GRAPH_NOT_CONVERGED / ACX_GRAPH_BAD_INDEX."""
    _check_rounds(max_rounds)
    dev = offsets.device
    with torch.cuda.device(dev):
        resume = labels is not None
        if labels is None:
            labels = torch.empty(n, dtype=torch.int32, device=dev)
        word = torch.empty(1, dtype=torch.int32, device=dev)
        idx = indices32 if indices32.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        _ffi.graph_components(vp(offsets), vp(idx), n, vp(labels), vp(word), max_rounds, resume, _ffi.stream_ptr(dev))
        if status is not None:
            status.bitwise_or_(word)
    return labels


class DuplicateGroups(_Checked):
    """The result of duplicate_groups(): device tensors.  labels (n,) int64 -- the smallest row index of each row's group; sizes
    (n,) int64 -- the size of each row's group; keep (n,) bool -- one representative per group, its smallest index (rows without a
    duplicate keep themselves); neighbors: the RadiusNeighbors list the groups were built from."""

    def __init__(self, labels, neighbors, status):
        self.labels, self.neighbors = labels, neighbors
        self.device = labels.device
        self._status = status
        n = labels.shape[0]
        self.sizes = torch.bincount(labels, minlength=n)[labels]
        self.keep = labels == torch.arange(n, device=labels.device)

    @property
    def pairs(self):
        """(m, 2) int64: every undirected near-duplicate pair once, i < j, in ascending (i, j)."""
        nb = self.neighbors
        rows = torch.repeat_interleave(torch.arange(nb.offsets.shape[0] - 1, device=self.device), nb.counts)
        cols = nb.indices
        a, b = torch.minimum(rows, cols), torch.maximum(rows, cols)
        key = torch.unique(a * nb.n + b)
        return torch.stack([key // nb.n, key % nb.n], dim=1)

    def groups(self):
        """The groups of two or more rows as lists of row indices, in ascending order of their smallest row; synchronises."""
        lab = self.labels.cpu().numpy()
        order = np.argsort(lab, kind="stable")
        cuts = np.nonzero(np.diff(lab[order]))[0] + 1
        return [g.tolist() for g in np.split(order, cuts) if g.size > 1]


def _groups_rows(x, aux, metric, level, max_rounds=MAX_ROUNDS):
    dev = x.device
    with torch.cuda.device(dev):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nb = _neighbors_rows(x, aux, x, aux, metric, level, _ffi.RADIUS_SELF_EXCLUDE, status, values=False)
        labels = components(nb.offsets, nb.indices32, x.shape[0], status, max_rounds)
        return DuplicateGroups(labels.to(torch.int64), nb, status)


def duplicate_groups(emb, threshold=0.95, metric="cosine", max_rounds=MAX_ROUNDS, device=None):
    """The groups of near-duplicate rows of emb (n, dim) on the GPU -> DuplicateGroups: the connected components of the graph whose
    edges are the pairs within the threshold (a cosine or dot product of at least `threshold`, or a distance of at most `threshold`
    for "euclidean").  A chain a ~ b ~ c is one group."""
    _check_rounds(max_rounds)
    x, aux, _, _, level, _, st = _prepare(None, emb, threshold, metric, device)
    dup = _groups_rows(x, aux, metric, level, max_rounds)
    dup._status.bitwise_or_(st)
    return dup


def cross_duplicates(queries, emb, threshold=0.95, metric="cosine", device=None):
    """The rows of emb within the threshold of each query -> RadiusNeighbors (counts: how many; the list: which, ascending).  The
    train / test leak check: queries = the test embeddings, emb = the training embeddings, leaked = counts > 0."""
    if queries is None:
        raise ValueError("cross_duplicates needs queries (duplicate_groups searches a set against itself)")
    return radius_neighbors(queries, emb, threshold, metric, values=True, device=device)


class DBSCANResult(_Checked):
    """The result of dbscan(): device tensors, nothing synchronised beyond the neighbour list's total.  labels (n,) int64 (-1:
    noise); core (n,) bool; counts (n,) int64 -- the rows within eps of each row, itself included; clusters: 0-d int32, the number
    of clusters; noise (n,) bool; neighbors: the RadiusNeighbors list."""

    def __init__(self, labels, core, clusters, neighbors, status):
        self.labels, self.core, self.clusters, self.neighbors = labels, core, clusters, neighbors
        self.counts = neighbors.counts
        self.noise = labels < 0
        self.device = labels.device
        self._status = status

    def clustered(self):
        """(rows (m,) int64: the indices of the rows that have a cluster, ascending; their labels (m,) int64) -- what the cluster
        scores take: silhouette(emb[rows], labels, clusters=int(db.clusters))."""
        rows = torch.nonzero(~self.noise)[:, 0]
        return rows, self.labels[rows]


def dbscan_labels(offsets, indices32, n, min_samples, status=None, max_rounds=MAX_ROUNDS):
    """(labels (n,) int32, core (n,) uint8, clusters (1,) int32) on the device from a self-join list made with include_self=True
    (acx_dbscan_labels).  status: an int32 device word that receives the call's bits."""
    _check_min_samples(min_samples)
    _check_rounds(max_rounds)
    dev = offsets.device
    with torch.cuda.device(dev):
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        core = torch.empty(n, dtype=torch.uint8, device=dev)
        clusters = torch.empty(1, dtype=torch.int32, device=dev)
        word = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.dbscan_workspace_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        idx = indices32 if indices32.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        _ffi.dbscan_labels(vp(offsets), vp(idx), n, min(int(min_samples), 2 ** 31 - 1), vp(labels), vp(core), vp(clusters), vp(word),
                           (vp(ws), ws_bytes), max_rounds, _ffi.stream_ptr(dev))
        if status is not None:
            status.bitwise_or_(word)
    return labels, core, clusters


def _dbscan_rows(x, aux, metric, level, min_samples, max_rounds=MAX_ROUNDS):
    dev = x.device
    with torch.cuda.device(dev):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nb = _neighbors_rows(x, aux, x, aux, metric, level, _ffi.RADIUS_SELF_INCLUDE, status, values=False)
        labels, core, clusters = dbscan_labels(nb.offsets, nb.indices32, x.shape[0], min_samples, status, max_rounds)
        return DBSCANResult(labels.to(torch.int64), core.to(torch.bool), clusters[0], nb, status)


def dbscan(emb, eps, min_samples=5, metric="euclidean", max_rounds=MAX_ROUNDS, device=None):
    """DBSCAN over emb (n, dim) on the GPU -> DBSCANResult, with scikit-learn's labels (DBSCAN(eps, min_samples, algorithm="brute"),
    border rows included).  metric "euclidean": rows within distance eps; "cosine" / "dot": rows whose cosine / dot product is at
    least `eps` (scikit-learn's cosine distance 1 - eps).  min_samples counts the row itself."""
    _check_min_samples(min_samples)
    _check_rounds(max_rounds)
    x, aux, _, _, level, _, st = _prepare(None, emb, eps, metric, device)
    res = _dbscan_rows(x, aux, metric, level, min_samples, max_rounds)
    res._status.bitwise_or_(st)
    return res
