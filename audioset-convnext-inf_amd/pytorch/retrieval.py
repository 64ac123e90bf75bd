"""Nearest-neighbour search over embeddings on the GPU (acx_knn_search / acx_knn_vote in include/acx.h): query by example and
the kNN probe of a frozen representation, next to the linear probe of `finetune.fit_head`.

    from audioset_convnext_inf_amd.pytorch.retrieval import EmbeddingIndex, search_host, vote_host
    idx = EmbeddingIndex(emb, metric="cosine", target=None)    # emb (n, dim); keeps the inverse norms
    idx.add(more_emb, target=None)                             # earlier rows keep their indices
    scores, indices = idx.search(queries, k=10, exclude=None)  # (q, k) fp32 / int64 device tensors, best first
    scores, indices = idx.search(None, k=10)                   # self-search: every row against the others
    probs = idx.classify(queries, k=10, weights="uniform")     # (q, C) fp32: kNN tagging, needs target=
    idx.check()                                                # synchronises; ValueError if a search met a NaN or inf
    km = idx.cluster(50)                                       # k-means over the stored rows (pytorch/clustering.py)

Order: score descending, then database index ascending, -0.0 as +0.0 -- one total order, so the result does not depend on how
the kernel got there.  A (query, row) pair has the same score bits whatever the batch, the index size, k or the chunking.
The (queries x database) score matrix is never written: a workgroup keeps the running top k of its queries on chip.

Nothing here synchronises with the host, and every call can be captured in a torch.cuda.graph.  Data errors therefore travel
in a status word on the device: a NaN or infinity in the queries or the index makes every index of that search -1 and every
score NaN, and `idx.check()` -- the one call that synchronises -- raises ValueError("... NaN or infinite ...") for any search
or classify since the last check.

`search_host` / `vote_host` are the documented host equivalents in numpy float64 (the tests' reference), as
`segments.decode_events` is for the event decoder.

The int8 index (acx_knn_quantize_i8 / acx_knn_search_i8 / acx_knn_rescore): a coarse search on per-row int8 codes on the i8
matrix cores, then the exact fp32 scores of a short candidate list.

    qidx = QuantizedIndex(emb, metric="cosine", rerank=True, oversample=4)     # or EmbeddingIndex.quantize(): shares the fp32 rows
    scores, indices = qidx.search(queries, k=10)      # coarse top min(MAX_K, 4 k), reranked: exact fp32 scores, the bits of
                                                      # EmbeddingIndex.search wherever the candidates hold the true neighbours
    qidx = QuantizedIndex(emb, rerank=False)          # codes, scales and targets only (dim_pad + 4 bytes a row): coarse scores

`quantize_host` / `search_i8_host` / `rescore_host` are its host definitions: the quantiser in numpy float32 operation by
operation, the coarse score ((float32)t * sq) * sd of the exact integer dot product t -- the device equals both bit for bit."""
import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs

METRICS = tuple(_ffi.KNN_METRICS)
WEIGHTS = tuple(_ffi.KNN_WEIGHTS)
MAX_K = _ffi.KNN_MAX_K
MAX_DIM = _ffi.KNN_MAX_DIM
WORKSPACE_LIMIT = 256 << 20          # bytes of search workspace per chunk of queries


def _check_metric(metric):
    if metric not in _ffi.KNN_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (METRICS, metric))


def _check_2d(x, name):
    shape = tuple(getattr(x, "shape", ()))
    if len(shape) != 2:
        raise ValueError("%s must be 2-D (rows, dim), got shape %s" % (name, shape))
    return shape


def _check_k(k, n, excluding):
    if int(k) != k or k < 1 or k > MAX_K:
        raise ValueError("k = %r (expected an integer in 1 .. %d)" % (k, MAX_K))
    if k > n - (1 if excluding else 0):
        raise ValueError("k = %d exceeds the %d rows a query may return%s" % (k, n - (1 if excluding else 0),
                                                                             " (the index size - 1 with exclude)" if excluding else ""))


# ---- the host equivalents (numpy float64) ---------------------------------------------------------------------------------
def search_host(queries, emb, k, metric="cosine", exclude=None):
    """(scores (q, k) float64, indices (q, k) int64) of the k nearest rows of `emb` per query: float64 dot products (cosine:
    times 1 / norm of each side, 0 for a zero row), ordered by score descending then index ascending (a stable sort);
    exclude: per query one index that is not returned (-1: none)."""
    _check_metric(metric)
    q = np.asarray(queries, dtype=np.float64)
    d = np.asarray(emb, dtype=np.float64)
    qs, ds = _check_2d(q, "queries"), _check_2d(d, "emb")
    if qs[1] != ds[1]:
        raise ValueError("queries have dim %d, the embeddings dim %d" % (qs[1], ds[1]))
    if ds[0] < 1:
        raise ValueError("the index is empty")
    _check_k(k, ds[0], exclude is not None)
    s = q @ d.T
    if metric == "cosine":
        def inv(x):
            nrm = np.sqrt((x * x).sum(axis=1))
            return np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
        s = s * inv(q)[:, None] * inv(d)[None, :]
    s = s + 0.0                                               # -0.0 -> +0.0
    key = -s
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64)
        if ex.shape != (qs[0],):
            raise ValueError("exclude must hold one index per query, got shape %s" % (ex.shape,))
        rows = np.nonzero((ex >= 0) & (ex < ds[0]))[0]
        key[rows, ex[rows]] = np.inf
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(s, order, axis=1), order.astype(np.int64)


def vote_host(indices, scores, target, weights="uniform", temperature=0.07):
    """(q, C) float64: sum_j w_j target[indices[q, j]] / sum_j w_j with w_j = 1 ("uniform") or exp((s_j - s_0) / temperature)
    ("similarity")."""
    if weights not in _ffi.KNN_WEIGHTS:
        raise ValueError("weights must be one of %s, got %r" % (WEIGHTS, weights))
    idx = np.asarray(indices, dtype=np.int64)
    y = np.asarray(target, dtype=np.float64)
    _check_2d(idx, "indices")
    _check_2d(y, "target")
    if weights == "uniform":
        w = np.ones(idx.shape, dtype=np.float64)
    else:
        if not temperature > 0:
            raise ValueError("temperature = %r (expected > 0)" % (temperature,))
        s = np.asarray(scores, dtype=np.float64)
        w = np.exp((s - s[:, :1]) / float(temperature))
    return (w[:, :, None] * y[idx]).sum(axis=1) / w.sum(axis=1)[:, None]


# ---- the host definitions of the int8 index ----------------------------------------------------------------------------------
I8_K = _ffi.KNN_I8_K


def quantize_host(x, metric="cosine", inv_norm=None):
    """(codes (n, dim rounded up to 32) int8, scales (n,) float32): the per-row symmetric quantiser of acx_knn_quantize_i8 in
    numpy float32, operation by operation: y = x * inv_norm[i] ("dot": y = x), amax = max |y|, g = 127 / amax,
    code = clip(rint(y * g), -127, 127), scale = amax / 127; a zero row -> zero codes, scale 0; a row with a NaN or infinity ->
    zero codes, scale NaN.  inv_norm: the float32 inverse norms to use for "cosine" (the device's, when its bits are to be
    met); by default 1 / sqrt(sum x^2) in float32, 0 for a zero row."""
    _check_metric(metric)
    x = np.asarray(x, dtype=np.float32)
    n, dim = _check_2d(x, "x")
    with np.errstate(all="ignore"):
        if metric == "cosine":
            if inv_norm is None:
                ss = (x * x).sum(axis=1, dtype=np.float32)
                inv_norm = np.where(ss > 0, np.float32(1) / np.sqrt(np.where(ss > 0, ss, np.float32(1))), np.float32(0))
            y = x * np.asarray(inv_norm, dtype=np.float32).reshape(n, 1)
        else:
            y = x
        bad = ~np.isfinite(y).all(axis=1) if dim else np.zeros(n, bool)
        y = np.where(bad[:, None], np.float32(0), y)
        amax = np.abs(y).max(axis=1) if dim else np.zeros(n, np.float32)
        zero = amax == 0
        g = np.float32(127) / np.where(zero, np.float32(1), amax)
        c = np.clip(np.rint(y * g[:, None]), np.float32(-127), np.float32(127))
        c = np.where(zero[:, None], np.float32(0), c).astype(np.int8)
        scale = (amax / np.float32(127)).astype(np.float32)
    scale[bad] = np.nan
    codes = np.zeros((n, -(-dim // I8_K) * I8_K), dtype=np.int8)
    codes[:, :dim] = c
    return codes, scale


def search_i8_host(cq, sq, cd, sd, k, exclude=None):
    """(scores (q, k) float32, indices (q, k) int64) of the coarse search: t = the integer dot product of two code rows
    (int64, exact), score = (float32(t) * sq[i]) * sd[j] in float32, the order of search_host (-0.0 as +0.0, stable)."""
    cq, cd = np.asarray(cq), np.asarray(cd)
    qs, ds = _check_2d(cq, "cq"), _check_2d(cd, "cd")
    if qs[1] != ds[1]:
        raise ValueError("query codes have dim %d, the database codes dim %d" % (qs[1], ds[1]))
    if ds[0] < 1:
        raise ValueError("the index is empty")
    _check_k(k, ds[0], exclude is not None)
    t = cq.astype(np.int64) @ cd.astype(np.int64).T
    with np.errstate(all="ignore"):
        s = (t.astype(np.float32) * np.asarray(sq, dtype=np.float32)[:, None]) * np.asarray(sd, dtype=np.float32)[None, :]
        s = s + np.float32(0)                                     # -0.0 -> +0.0
    key = -s
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64)
        if ex.shape != (qs[0],):
            raise ValueError("exclude must hold one index per query, got shape %s" % (ex.shape,))
        rows = np.nonzero((ex >= 0) & (ex < ds[0]))[0]
        key[rows, ex[rows]] = np.inf
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(s, order, axis=1), order.astype(np.int64)


def rescore_host(queries, emb, cand, k, metric="cosine"):
    """(scores (q, k) float64, indices (q, k) int64): search_host's float64 scores restricted to each query's candidate rows
    `cand` (q, kc) -- entries that are -1 or outside the rows are skipped -- in search_host's order; -1 / NaN where a query has
    fewer than k valid candidates."""
    _check_metric(metric)
    q = np.asarray(queries, dtype=np.float64)
    d = np.asarray(emb, dtype=np.float64)
    c = np.asarray(cand, dtype=np.int64)
    qs, ds, cs = _check_2d(q, "queries"), _check_2d(d, "emb"), _check_2d(c, "cand")
    if qs[1] != ds[1]:
        raise ValueError("queries have dim %d, the embeddings dim %d" % (qs[1], ds[1]))
    if cs[0] != qs[0]:
        raise ValueError("cand has %d rows, the queries %d" % (cs[0], qs[0]))
    if int(k) != k or k < 1 or k > cs[1]:
        raise ValueError("k = %r (expected an integer in 1 .. %d candidates)" % (k, cs[1]))
    valid = (c >= 0) & (c < ds[0])
    rows = d[np.where(valid, c, 0)]                                        # (q, kc, dim)
    s = np.einsum("qd,qcd->qc", q, rows)
    if metric == "cosine":
        def inv(x):
            nrm = np.sqrt((x * x).sum(axis=-1))
            return np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
        s = s * inv(q)[:, None] * inv(rows)
    s = s + 0.0
    order = np.lexsort((np.where(valid, c, ds[0]), np.where(valid, -s, np.inf)), axis=1)[:, :k]
    ok = np.take_along_axis(valid, order, axis=1)
    return (np.where(ok, np.take_along_axis(s, order, axis=1), np.nan),
            np.where(ok, np.take_along_axis(c, order, axis=1), -1).astype(np.int64))


def candidate_count(k, oversample, rows):
    """How many coarse candidates a reranked search of k neighbours keeps per query: min(MAX_K, k * oversample, the rows a
    query may return).  ValueError if k * oversample exceeds MAX_K."""
    if int(oversample) != oversample or oversample < 1:
        raise ValueError("oversample = %r (expected an integer >= 1)" % (oversample,))
    if k * oversample > MAX_K:
        raise ValueError("k * oversample = %d * %d exceeds MAX_K = %d candidates per query" % (k, oversample, MAX_K))
    return int(min(MAX_K, k * oversample, rows))


# ---- the device path -------------------------------------------------------------------------------------------------------
def _rows(x, device, dim=None, name="embeddings"):
    """x (rows, dim) -> an fp32 tensor on `device` the kernels can read (_inputs.rows with align4), zero-padded to a multiple
    of 4 columns.  A CUDA tensor that is already readable -- a column slice of a wider tensor too -- is returned as it is."""
    shape = _check_2d(x, name)
    if dim is not None and shape[1] != dim:
        raise ValueError("%s have dim %d, the index dim %d" % (name, shape[1], dim))
    if shape[1] < 1 or shape[1] > MAX_DIM:
        raise ValueError("dim = %d (expected 1 .. %d)" % (shape[1], MAX_DIM))
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = x.detach().to(device=device, dtype=torch.float32)
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))
    return _inputs.rows(x, align4=True) if x.shape[0] else x


def _target(t, rows, device):
    """-> (a (rows, C) uint8 or fp32 device tensor with unit column stride, ACX_TARGET_*)."""
    shape = _check_2d(t, "target")
    if shape[0] != rows:
        raise ValueError("target has %d rows, the embeddings %d" % (shape[0], rows))
    if shape[1] < 1 or shape[1] > _ffi.MAX_CLASSES:
        raise ValueError("target has %d classes (expected 1 .. %d)" % (shape[1], _ffi.MAX_CLASSES))
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return _inputs.kernel_target(t.detach().to(device))


def row_norms(x, status=None):
    """1 / sqrt(sum x^2) per row of a readable (rows, dim) device tensor (0 for a zero row), on the current stream."""
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _ffi.knn_row_norms(vp(x), x.stride(0), x.shape[0], x.shape[1], vp(out), vp(status), _ffi.stream_ptr(x.device))
    return out


def vote(indices, scores, target, weights="uniform", temperature=0.07, status=None):
    """(q, C) fp32 on the device: the kNN vote of acx_knn_vote over `indices` (q, k) int32 / int64 into `target` (n, C) uint8 /
    bool / fp32.  status: an int32 device word that receives ACX_KNN_BAD_INDEX for an index outside the target's rows."""
    if weights not in _ffi.KNN_WEIGHTS:
        raise ValueError("weights must be one of %s, got %r" % (WEIGHTS, weights))
    if weights == "similarity" and not temperature > 0:
        raise ValueError("temperature = %r (expected > 0)" % (temperature,))
    q, k = _check_2d(indices, "indices")
    if k < 1 or k > MAX_K:
        raise ValueError("k = %d (expected 1 .. %d)" % (k, MAX_K))
    dev = indices.device
    target, code = _target(target, target.shape[0], dev)
    idx32 = indices.to(torch.int32).contiguous()
    sc = None if scores is None else scores.to(torch.float32).contiguous()
    if weights == "similarity" and sc is None:
        raise ValueError("similarity weights need the scores")
    out = torch.empty((q, target.shape[1]), dtype=torch.float32, device=dev)
    word = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _ffi.knn_vote(vp(idx32), vp(sc), q, k, vp(target), code, target.stride(0), target.shape[0], target.shape[1],
                      _ffi.KNN_WEIGHTS[weights], temperature, vp(out), out.stride(0), vp(word), _ffi.stream_ptr(dev))
    if status is not None:
        status.bitwise_or_(word)
    return out


def quantize(x, inv_norm=None, status=None):
    """(codes (rows, dim rounded up to 32) int8, scales (rows,) fp32) of a readable (rows, dim) fp32 device tensor by
    acx_knn_quantize_i8, on the current stream; inv_norm: the rows' inverse norms (cosine) or None (dot).  status: an int32
    device word that receives ACX_KNN_NONFINITE for a row with a NaN or infinity."""
    n, dim = x.shape
    pad = -(-dim // I8_K) * I8_K
    codes = torch.empty((n, pad), dtype=torch.int8, device=x.device)
    scales = torch.empty(n, dtype=torch.float32, device=x.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _ffi.knn_quantize_i8(vp(x), x.stride(0), None if inv_norm is None else vp(inv_norm), n, dim, vp(codes), pad, vp(scales),
                                 vp(status), _ffi.stream_ptr(x.device))
    return codes, scales


def _append(buf, n0, new):
    """buf[:n0] followed by `new`, in place when the capacity allows (it at least doubles when it runs out)."""
    if buf is None:
        return new
    m = new.shape[0]
    if n0 + m > buf.shape[0]:
        grown = torch.empty((max(2 * buf.shape[0], n0 + m),) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
        grown[:n0] = buf[:n0]
        buf = grown
    buf[n0:n0 + m] = new
    return buf


class EmbeddingIndex:
    """A growing table of embeddings on one GPU with their inverse norms and, optionally, one target row each.

    emb: (n, dim) -- a CUDA tensor is read where it is when its layout allows (a column slice of a wider tensor too) and is
    then SHARED with the caller until the first add() that outgrows it; CPU tensors and numpy arrays are copied to `device`.
    A dim that is not a multiple of 4 is zero-padded, which changes neither dots nor norms.  workspace_limit: bytes of search
    workspace per chunk of queries; the chunking never changes a bit of the result."""

    def __init__(self, emb, metric="cosine", target=None, device=None, workspace_limit=WORKSPACE_LIMIT):
        _check_metric(metric)
        shape = _check_2d(emb, "embeddings")
        if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
            device = emb.device
        self.device = _inputs.cuda_device(device, "the search runs on")
        self.metric = metric
        self.dim = int(shape[1])
        self.workspace_limit = int(workspace_limit)
        self._n = 0
        self._buf = None
        self._inv = None
        self._tgt = None
        self._has_target = target is not None
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        if shape[0]:
            self.add(emb, target)
        elif target is not None:
            raise ValueError("target given with no embeddings")

    # ---- contents
    def __len__(self):
        return self._n

    @property
    def embeddings(self):
        """(n, dim) fp32 view of the stored rows."""
        if self._buf is None:
            return torch.empty((0, self.dim), dtype=torch.float32, device=self.device)
        return self._buf[:self._n, :self.dim]

    @property
    def target(self):
        return None if self._tgt is None else self._tgt[:self._n]

    @property
    def inverse_norms(self):
        return None if self._inv is None else self._inv[:self._n]

    def add(self, emb, target=None):
        """Append rows (amortised growth: the capacity at least doubles when it runs out); earlier rows keep their indices and
        their bits.  target: one row per new row if and only if the index was built with targets."""
        x = _rows(emb, self.device, self.dim)
        m = x.shape[0]
        if (target is not None) != self._has_target:
            raise ValueError("this index was built %s targets: add() must be called the same way"
                             % ("with" if self._has_target else "without"))
        if m == 0:
            return self
        t = _target(target, m, self.device)[0] if target is not None else None
        if t is not None and self._tgt is not None and (t.shape[1] != self._tgt.shape[1] or t.dtype != self._tgt.dtype):
            raise ValueError("target rows of %d classes (%s) added to an index of %d classes (%s)"
                             % (t.shape[1], t.dtype, self._tgt.shape[1], self._tgt.dtype))
        with torch.cuda.device(self.device):
            inv = row_norms(x, self._status) if self.metric == "cosine" else None
            if self._buf is None:
                self._buf, self._inv, self._tgt = x, inv, t
            else:
                n0, cap = self._n, self._buf.shape[0]
                if n0 + m > cap:
                    cap = max(2 * cap, n0 + m)
                    buf = torch.empty((cap, x.shape[1]), dtype=torch.float32, device=self.device)
                    buf[:n0] = self._buf[:n0]
                    self._buf = buf
                    if inv is not None:
                        nv = torch.empty(cap, dtype=torch.float32, device=self.device)
                        nv[:n0] = self._inv[:n0]
                        self._inv = nv
                    if t is not None:
                        nt = torch.empty((cap, t.shape[1]), dtype=t.dtype, device=self.device)
                        nt[:n0] = self._tgt[:n0]
                        self._tgt = nt
                self._buf[n0:n0 + m] = x
                if inv is not None:
                    self._inv[n0:n0 + m] = inv
                if t is not None:
                    self._tgt[n0:n0 + m] = t
            self._n += m
        return self

    # ---- search
    def _chunk(self, nq, k):
        """The most queries per call whose workspace fits workspace_limit (at least one)."""
        fits = lambda c: _ffi.knn_workspace_bytes(c, self._n, k) <= self.workspace_limit
        if fits(nq):
            return nq
        lo, hi = 1, nq                  # fits(lo) assumed, fits(hi) false: the size is non-decreasing in the query count
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        return lo

    def search(self, queries, k=10, exclude=None):
        """(scores (q, k) fp32, indices (q, k) int64), best first, on the device and the current stream; nothing synchronises.
        queries: (q, dim), or None for a self-search -- every row of the index against the others (exclude = its own row).
        exclude: None or one database index per query that is never returned (-1: none)."""
        if self._n == 0:
            raise ValueError("the index is empty")
        if queries is None:
            if exclude is not None:
                raise ValueError("a self-search excludes each row itself: exclude must be None")
            q, rq = self._buf[:self._n], self.inverse_norms
            exclude = torch.arange(self._n, dtype=torch.int32, device=self.device)
            _check_k(k, self._n, True)
        else:
            _check_2d(queries, "queries")
            _check_k(k, self._n, exclude is not None)
            q, rq = _rows(queries, self.device, self.dim, "queries"), None
            if exclude is not None:
                if not isinstance(exclude, torch.Tensor):
                    exclude = torch.from_numpy(np.ascontiguousarray(exclude))
                if tuple(exclude.shape) != (q.shape[0],):
                    raise ValueError("exclude must hold one index per query, got shape %s" % (tuple(exclude.shape),))
                exclude = exclude.to(device=self.device, dtype=torch.int32).contiguous()
        nq, k = q.shape[0], int(k)
        dev = self.device
        indices = torch.empty((nq, k), dtype=torch.int32, device=dev)
        scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if nq == 0:
            return scores, indices.to(torch.int64)
        d = self._buf[:self._n]
        cosine = self.metric == "cosine"
        with torch.cuda.device(dev):
            if cosine and rq is None:
                rq = row_norms(q)
            chunk = self._chunk(nq, k)
            ws_bytes = _ffi.knn_workspace_bytes(min(chunk, nq), self._n, k)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            words = torch.empty((nq + chunk - 1) // chunk, dtype=torch.int32, device=dev)
            stream = _ffi.stream_ptr(dev)
            for i, a in enumerate(range(0, nq, chunk)):
                b = min(nq, a + chunk)
                _ffi.knn_search(vp(q[a:b]), q.stride(0), vp(rq[a:b]) if cosine else None, b - a, vp(d), d.stride(0),
                                vp(self._inv) if cosine else None, self._n, q.shape[1], _ffi.KNN_METRICS[self.metric], k,
                                vp(exclude[a:b]) if exclude is not None else None, vp(indices[a:b]), vp(scores[a:b]),
                                vp(words[i:]), (vp(ws), ws_bytes), stream)
            self._status.bitwise_or_(words if words.numel() == 1 else words.amax())      # each word is 0 or ACX_KNN_NONFINITE
        return scores, indices.to(torch.int64)

    def classify(self, queries, k=10, weights="uniform", temperature=0.07):
        """(q, C) fp32 on the device: kNN tagging -- the mean of the k nearest rows' targets, uniform or weighted by
        exp((s_j - s_0) / temperature).  Equals search() followed by vote()."""
        if self._tgt is None:
            raise ValueError("classify needs an index built with target=")
        if weights not in _ffi.KNN_WEIGHTS:
            raise ValueError("weights must be one of %s, got %r" % (WEIGHTS, weights))
        scores, indices = self.search(queries, k)
        return vote(indices, scores, self.target, weights, temperature, status=self._status)

    def cluster(self, clusters, **kw):
        """K-means over the stored rows (pytorch/clustering.py: kmeans) with the index's own metric -- "cosine": cosine,
        "dot": euclidean -- reusing the index's inverse norms; kw: init, n_init, max_iter, tol, seed.  -> clustering.KMeans."""
        from . import clustering
        if self._n == 0:
            raise ValueError("the index is empty")
        metric = "cosine" if self.metric == "cosine" else "euclidean"
        clustering._check_fit_args((self._n, self.dim), clusters, metric, kw.get("init", "k-means++"), kw.get("n_init", 1),
                                   kw.get("max_iter", 100), kw.get("tol", 1e-4))
        return clustering._fit_rows(self._buf[:self._n], self.dim, self.inverse_norms if metric == "cosine" else None, clusters,
                                    metric, **kw)

    def cluster_scores(self, km, sample=None, seed=0):
        """How good a clustering of the stored rows is (pytorch/cluster_scores.py) with the index's own metric, as cluster()
        takes it, reusing the index's inverse norms: km is a clustering.KMeans over these rows (or a (n,) tensor of labels in
        [0, max + 1)).  -> cluster_scores.ClusterScores(silhouette, dispersion); sample, seed: as silhouette() takes them."""
        from . import cluster_scores as cs
        if self._n == 0:
            raise ValueError("the index is empty")
        metric = "cosine" if self.metric == "cosine" else "euclidean"
        labels = getattr(km, "labels", km)
        cs._check_sample(sample, self._n)
        lab = cs._labels32(labels, self._n, self.device)
        K = cs._clusters_of(lab, km.centers.shape[0] if hasattr(km, "centers") else None)
        x = self._buf[:self._n]
        sil = cs._silhouette_rows(x, self.inverse_norms if metric == "cosine" else None, lab, K, metric,
                                  cs._sample_rows(self._n, sample, seed, self.device))
        return cs.ClusterScores(sil, cs._dispersion_rows(x, self.dim, lab, K))

    # ---- radius search (pytorch/neighbors.py), with the index's own metric and inverse norms
    def _radius_self(self):
        if self._n == 0:
            raise ValueError("the index is empty")
        return self._buf[:self._n], self.inverse_norms

    def radius(self, queries=None, threshold=0.9, values=True, slices=0):
        """The stored rows whose score (the index's metric) with each query is at least `threshold`, as a CSR list in ascending row
        index -> neighbors.RadiusNeighbors.  queries None: a self-join, every row against the others.  The values have the bits
        search() gives the same pair."""
        from . import neighbors as nb
        d, rd = self._radius_self()
        level = float(nb.level_of(threshold, self.metric))
        with torch.cuda.device(self.device):
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            if queries is None:
                q, rq, mode = d, rd, _ffi.RADIUS_SELF_EXCLUDE
            else:
                _check_2d(queries, "queries")
                q, mode = _rows(queries, self.device, self.dim, "queries"), _ffi.RADIUS_SELF_NONE
                if q.shape[0] < 1:
                    raise ValueError("the queries have no rows")
                rq = row_norms(q, status) if self.metric == "cosine" else None
            return nb._neighbors_rows(q, rq, d, rd, self.metric, level, mode, status, values, slices)

    def duplicates(self, threshold=0.95, max_rounds=None):
        """The groups of near-duplicate stored rows (score of at least `threshold`) -> neighbors.DuplicateGroups."""
        from . import neighbors as nb
        d, rd = self._radius_self()
        return nb._groups_rows(d, rd, self.metric, float(nb.level_of(threshold, self.metric)), max_rounds or nb.MAX_ROUNDS)

    def dbscan(self, eps, min_samples=5, max_rounds=None):
        """DBSCAN over the stored rows with the index's metric: two rows are neighbours when their score is at least `eps`
        (cosine: scikit-learn's cosine distance 1 - eps) -> neighbors.DBSCANResult."""
        from . import neighbors as nb
        nb._check_min_samples(min_samples)
        d, rd = self._radius_self()
        return nb._dbscan_rows(d, rd, self.metric, float(nb.level_of(eps, self.metric)), min_samples, max_rounds or nb.MAX_ROUNDS)

    def moments(self, ddof=1):
        """Mean and covariance of the stored rows in float64 (pytorch/statistics.py: moments) -> statistics.Moments."""
        from . import statistics
        if self._n == 0:
            raise ValueError("the index is empty")
        return statistics.moments(self.embeddings, ddof, self.device)

    def pca(self, components=None, whiten=False, **kw):
        """PCA of the stored rows (pytorch/statistics.py: PCA.fit) -> (the fitted statistics.PCA, a new EmbeddingIndex over
        PCA.transform of the rows, with this index's metric and targets); kw: max_sweeps, eps."""
        from . import statistics
        if self._n == 0:
            raise ValueError("the index is empty")
        fit = statistics.PCA.fit(self.embeddings, components, whiten, device=self.device, **kw)
        reduced = EmbeddingIndex(fit.transform(self.embeddings), metric=self.metric, target=self.target, device=self.device,
                                 workspace_limit=self.workspace_limit)
        return fit, reduced

    def quantize(self, rerank=True, oversample=4):
        """-> a QuantizedIndex over the stored rows.  rerank=True: it SHARES this index (the fp32 rows are not copied; rows
        added to either later are seen by both); rerank=False: int8 codes, scales and a copy of the targets only."""
        return QuantizedIndex._of(self, rerank, oversample)

    def check(self):
        """Synchronise and raise ValueError if a search or classify since the last check met bad data."""
        _raise_status(self._status)
        return self


def _raise_status(word):
    st = int(word.cpu()[0])
    if st:
        word.zero_()
    if st & _ffi.KNN_NONFINITE:
        raise ValueError("the queries or the indexed embeddings hold NaN or infinite values")
    if st & _ffi.KNN_BAD_INDEX:
        raise ValueError("a neighbour index lies outside the target rows")


class QuantizedIndex:
    """An int8 index: per-row symmetric int8 codes with one fp32 scale each, searched on the i8 matrix cores.

    rerank=True keeps the fp32 rows and inverse norms on the device as well (an EmbeddingIndex, `exact`): a search is the coarse
    search for kc = min(MAX_K, k * oversample, the rows a query may return) candidates followed by their exact fp32 scores
    (acx_knn_rescore) -- the score bits of EmbeddingIndex.search, and its whole result wherever the candidates cover the true
    neighbours.  rerank=False stores codes, scales and targets only (dim rounded up to 32, + 4 bytes a row) and returns the
    coarse scores ((float)t * sq) * sd.  Queries are quantised per call.  emb, target, device, workspace_limit: as for
    EmbeddingIndex.  Nothing synchronises; data errors travel in the status word until check()."""

    def __init__(self, emb, metric="cosine", target=None, device=None, rerank=True, oversample=4, workspace_limit=WORKSPACE_LIMIT):
        _check_metric(metric)
        shape = _check_2d(emb, "embeddings")
        candidate_count(1, oversample, 1)
        if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
            device = emb.device
        self.device = _inputs.cuda_device(device, "the search runs on")
        self.metric = metric
        self.dim = int(shape[1])
        self.rerank = bool(rerank)
        self.oversample = int(oversample)
        self.workspace_limit = int(workspace_limit)
        self.exact = EmbeddingIndex(emb[:0], metric, None, self.device, workspace_limit) if rerank else None
        if rerank:
            self.exact._has_target = target is not None
        self._init_codes(target is not None)
        if shape[0]:
            self.add(emb, target)
        elif target is not None:
            raise ValueError("target given with no embeddings")

    def _init_codes(self, has_target):
        self._n = 0
        self._codes = None
        self._scales = None
        self._tgt = None                       # rerank=False only: with rerank the targets are exact's
        self._has_target = has_target
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    @classmethod
    def _of(cls, index, rerank, oversample):
        self = cls.__new__(cls)
        candidate_count(1, oversample, 1)
        self.device, self.metric, self.dim, self.workspace_limit = index.device, index.metric, index.dim, index.workspace_limit
        self.rerank, self.oversample = bool(rerank), int(oversample)
        self.exact = index if rerank else None
        self._init_codes(index._has_target)
        if rerank:
            self._sync()
        elif len(index):
            self._add_codes(index._buf[:len(index)], index.inverse_norms)
            self._tgt = None if index.target is None else index.target.clone()
        return self

    # ---- contents
    def _add_codes(self, x, inv):
        codes, scales = quantize(x, inv, self._status)
        self._codes = _append(self._codes, self._n, codes)
        self._scales = _append(self._scales, self._n, scales)
        self._n += x.shape[0]

    def _sync(self):
        """rerank: quantise the rows `exact` holds beyond the codes (rows added through it, or through a shared index)."""
        if self.exact is not None and len(self.exact) > self._n:
            e = self.exact
            with torch.cuda.device(self.device):
                self._add_codes(e._buf[self._n:len(e)], None if e._inv is None else e._inv[self._n:len(e)])

    def __len__(self):
        self._sync()
        return self._n

    @property
    def codes(self):
        """(n, dim rounded up to 32) int8 view of the stored codes."""
        if len(self) == 0:
            return torch.empty((0, -(-self.dim // I8_K) * I8_K), dtype=torch.int8, device=self.device)
        return self._codes[:self._n]

    @property
    def scales(self):
        """(n,) fp32: code * scale approximates the (cosine: normalised) row."""
        if len(self) == 0:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        return self._scales[:self._n]

    @property
    def target(self):
        if self.exact is not None:
            return self.exact.target
        return None if self._tgt is None else self._tgt[:self._n]

    def add(self, emb, target=None):
        """Append rows; earlier rows keep their indices, codes and scales.  target: as for EmbeddingIndex.add."""
        if self.exact is not None:
            self.exact.add(emb, target)
            self._sync()
            return self
        x = _rows(emb, self.device, self.dim)
        m = x.shape[0]
        if (target is not None) != self._has_target:
            raise ValueError("this index was built %s targets: add() must be called the same way"
                             % ("with" if self._has_target else "without"))
        if m == 0:
            return self
        t = _target(target, m, self.device)[0] if target is not None else None
        if t is not None and self._tgt is not None and (t.shape[1] != self._tgt.shape[1] or t.dtype != self._tgt.dtype):
            raise ValueError("target rows of %d classes (%s) added to an index of %d classes (%s)"
                             % (t.shape[1], t.dtype, self._tgt.shape[1], self._tgt.dtype))
        with torch.cuda.device(self.device):
            n0 = self._n
            self._add_codes(x, row_norms(x, self._status) if self.metric == "cosine" else None)
            if t is not None:
                self._tgt = _append(self._tgt, n0, t)
        return self

    # ---- search
    def search(self, queries, k=10, exclude=None):
        """(scores (q, k) fp32, indices (q, k) int64), best first, on the device and the current stream; nothing synchronises.
        queries, exclude: as for EmbeddingIndex.search (None: the self-search on the stored codes).  With rerank the scores are
        the exact fp32 scores of the best k of the coarse candidates; without, the coarse scores."""
        n = len(self)
        if n == 0:
            raise ValueError("the index is empty")
        dev, cosine = self.device, self.metric == "cosine"
        if queries is None:
            if exclude is not None:
                raise ValueError("a self-search excludes each row itself: exclude must be None")
            _check_k(k, n, True)
            exclude = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            _check_2d(queries, "queries")
            _check_k(k, n, exclude is not None)
        k = int(k)
        kc = candidate_count(k, self.oversample, n - (0 if exclude is None else 1)) if self.rerank else k
        with torch.cuda.device(dev):
            if queries is None:
                cq, sq = self._codes[:n], self._scales[:n]
                q, rq = (self.exact._buf[:n], self.exact.inverse_norms) if self.rerank else (None, None)
            else:
                q = _rows(queries, dev, self.dim, "queries")
                if exclude is not None:
                    if not isinstance(exclude, torch.Tensor):
                        exclude = torch.from_numpy(np.ascontiguousarray(exclude))
                    if tuple(exclude.shape) != (q.shape[0],):
                        raise ValueError("exclude must hold one index per query, got shape %s" % (tuple(exclude.shape),))
                    exclude = exclude.to(device=dev, dtype=torch.int32).contiguous()
                rq = row_norms(q) if cosine and q.shape[0] else None
                cq, sq = quantize(q, rq, self._status)
            nq = cq.shape[0]
            indices = torch.empty((nq, k), dtype=torch.int32, device=dev)
            scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
            if nq == 0:
                return scores, indices.to(torch.int64)
            cand, coarse = (torch.empty((nq, kc), dtype=torch.int32, device=dev), torch.empty((nq, kc), dtype=torch.float32,
                                                                                              device=dev)) if self.rerank else (indices, scores)
            fits = lambda c: _ffi.knn_workspace_bytes(c, n, kc) <= self.workspace_limit
            chunk = nq
            if not fits(nq):
                lo, hi = 1, nq          # fits(lo) assumed, fits(hi) false: the size is non-decreasing in the query count
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    lo, hi = (mid, hi) if fits(mid) else (lo, mid)
                chunk = lo
            # room for the first level of a two-level merge (about sqrt(slices) lists a query): a single query has ONE wave to merge
            slices = _ffi.knn_slices(chunk, n, kc)
            ws_bytes = _ffi.knn_workspace_bytes(chunk, n, kc) + (chunk * (int(slices ** 0.5) + 2) * kc * 8 if slices >= 16 else 0)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            chunks = (nq + chunk - 1) // chunk
            words = torch.empty(chunks + 1, dtype=torch.int32, device=dev)
            stream = _ffi.stream_ptr(dev)
            cd, sd = self._codes, self._scales
            for i, a in enumerate(range(0, nq, chunk)):
                b = min(nq, a + chunk)
                _ffi.knn_search_i8(vp(cq[a:b]), cq.stride(0), vp(sq[a:b]), b - a, vp(cd), cd.stride(0), vp(sd), n, cd.shape[1], kc,
                                   vp(exclude[a:b]) if exclude is not None else None, vp(cand[a:b]), vp(coarse[a:b]), vp(words[i:]),
                                   (vp(ws), ws_bytes), stream)
            if self.rerank:
                d = self.exact._buf
                _ffi.knn_rescore(vp(q), q.stride(0), vp(rq) if cosine else None, nq, vp(d), d.stride(0),
                                 vp(self.exact._inv) if cosine else None, n, q.shape[1], _ffi.KNN_METRICS[self.metric], vp(cand), kc,
                                 kc, k, vp(indices), vp(scores), vp(words[chunks:]), stream)
            else:
                words[chunks:].zero_()
            self._status.bitwise_or_(words.amax())           # each word is 0 or ACX_KNN_NONFINITE: the candidates are the search's own
        return scores, indices.to(torch.int64)

    def classify(self, queries, k=10, weights="uniform", temperature=0.07):
        """(q, C) fp32 on the device: kNN tagging, search() followed by vote()."""
        if self.target is None:
            raise ValueError("classify needs an index built with target=")
        if weights not in _ffi.KNN_WEIGHTS:
            raise ValueError("weights must be one of %s, got %r" % (WEIGHTS, weights))
        scores, indices = self.search(queries, k)
        return vote(indices, scores, self.target, weights, temperature, status=self._status)

    def cluster(self, clusters, **kw):
        """K-means over the stored fp32 rows (EmbeddingIndex.cluster); needs rerank=True."""
        if self.exact is None:
            raise ValueError("cluster needs the fp32 rows: build the index with rerank=True")
        return self.exact.cluster(clusters, **kw)

    def check(self):
        """Synchronise and raise ValueError if an add, a search or a classify since the last check met bad data."""
        if self.exact is not None:
            self._status.bitwise_or_(self.exact._status)
            self.exact._status.zero_()
        _raise_status(self._status)
        return self
