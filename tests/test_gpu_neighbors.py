"""GPU: radius search, components and DBSCAN (pytorch/neighbors.py; acx_radius_count, acx_radius_neighbors, acx_graph_components,
acx_dbscan_labels in include/acx.h; csrc/neighbors.hip) against the numpy host definitions: with `==` on integer rows whose every
pair value is exact, by decided pairs inside the fp32 rounding bound on Gaussian blobs, bit for bit against the search's scores,
between runs, between slicings and under a captured graph, and by flags and canaries on overflow and bad data."""
import numpy as np
import pytest
import torch

import neighbors_cases as cases
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import neighbors as nbm
from audioset_convnext_inf_amd.pytorch import retrieval
from audioset_convnext_inf_amd.pytorch.neighbors import components_host, dbscan_host, radius_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0x5a5a5a5a


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def rows_on_device(x, pad=0):
    """x (n, dim) on the device with a row stride of dim + pad floats (the padding filled with a value that must not be read)."""
    n, dim = x.shape
    buf = torch.full((n, dim + pad), 1e30, dtype=torch.float32, device=DEV)
    buf[:, :dim] = dev(x)
    return buf[:, :dim]


def aux_of(xv, metric):
    return nbm._aux(xv, metric, torch.zeros(1, dtype=torch.int32, device=DEV))


def run_neighbors(q, d, threshold, metric, mode=0, slices=0, pad=0, capacity=None, values=True):
    """acx_radius_neighbors through the raw binding -> dict(offsets, indices, values, total, status, tail: the canaries behind the
    capacity).  q None: a self-join of d.  capacity None: the host's total."""
    dv = rows_on_device(d, pad)
    qv = dv if q is None else rows_on_device(q, pad)
    da = aux_of(dv, metric)
    qa = da if q is None else aux_of(qv, metric)
    nq, n, dim = qv.shape[0], dv.shape[0], dv.shape[1]
    level = float(nbm.level_of(threshold, metric))
    if capacity is None:
        capacity = int(radius_host(q, d, threshold, metric, include_self=mode == 2).offsets[-1])
    guard = 64
    idx = torch.full((capacity + guard,), CANARY, dtype=torch.int32, device=DEV)
    val = torch.full((capacity + guard,), 7.0, dtype=torch.float32, device=DEV) if values else None
    off = torch.full((nq + 1 + guard,), -7, dtype=torch.int64, device=DEV)
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    st = torch.full((1,), 255, dtype=torch.int32, device=DEV)
    nb = _ffi.radius_workspace_bytes(nq, n, slices)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _ffi.radius_neighbors(vp(qv), qv.stride(0), vp(qa), nq, vp(dv), dv.stride(0), vp(da), n, dim, _ffi.RADIUS_METRICS[metric], level,
                          mode, slices, vp(off), vp(idx), vp(val), capacity, vp(total), vp(st), (vp(ws), nb),
                          _ffi.stream_ptr(torch.device(DEV)))
    assert (off[nq + 1:] == -7).all()
    return dict(offsets=off[:nq + 1].cpu().numpy(), indices=idx[:capacity].cpu().numpy(), tail=idx[capacity:].cpu().numpy(),
                values=None if val is None else val[:capacity].cpu().numpy(),
                vtail=None if val is None else val[capacity:].cpu().numpy(), total=int(total.cpu()[0]), status=int(st.cpu()[0]))


def run_count(q, d, threshold, metric, mode=0, pad=0):
    dv = rows_on_device(d, pad)
    qv = dv if q is None else rows_on_device(q, pad)
    da = aux_of(dv, metric)
    qa = da if q is None else aux_of(qv, metric)
    st = torch.full((1,), 255, dtype=torch.int32, device=DEV)
    counts = nbm._count_rows(qv, qa, dv, da, metric, float(nbm.level_of(threshold, metric)), mode, st)
    return counts.cpu().numpy(), int(st.cpu()[0])


def assert_list_equals_host(got, h, values=True):
    assert got["status"] == 0 and got["total"] == h.offsets[-1]
    np.testing.assert_array_equal(got["offsets"], h.offsets)
    np.testing.assert_array_equal(got["indices"], h.indices)
    if values:
        np.testing.assert_array_equal(got["values"], h.values)
    assert (got["tail"] == CANARY).all()


# ---- EQUAL: integer rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "euclidean"])
@pytest.mark.parametrize("shape", cases.EQUAL_SHAPES, ids=cases.EQUAL_IDS)
def test_integer_rows_equal_the_host_definition(shape, metric):
    nq, n, dim, pad = shape
    q, d = cases.int_rows(nq, dim, 1), cases.int_rows(n, dim, 2)
    v = nbm.pair_values_host(q, d, metric)
    thr = cases.attained_level(v, metric, 0.2 if metric == "euclidean" else 0.8)        # the level IS a value some pair has
    h = radius_host(q, d, thr, metric)
    assert (v == float(nbm.level_of(thr, metric))).any()
    by_slices = [run_neighbors(q, d, thr, metric, slices=s, pad=pad) for s in (0, 1, 2, 17)]
    for got in by_slices:
        assert_list_equals_host(got, h)
    counts, st = run_count(q, d, thr, metric, pad=pad)
    np.testing.assert_array_equal(counts, h.counts)
    assert st == 0


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
@pytest.mark.parametrize("shape", cases.SELF_SHAPES, ids=lambda s: "%d-d%d" % s)
def test_self_joins_decide_the_diagonal_by_position(shape, metric):
    n, dim = shape
    d = cases.int_rows(n, dim, 3)
    d[n // 2] = 0                                                        # a zero row: its dot products are all 0
    v = nbm.pair_values_host(d, d, metric)
    thr = cases.attained_level(v, metric, 0.3 if metric == "euclidean" else 0.7)
    for include in (False, True):
        h = radius_host(None, d, thr, metric, include_self=include)
        for s in (1, 2, 17):
            assert_list_equals_host(run_neighbors(None, d, thr, metric, mode=2 if include else 1, slices=s), h)
        counts, st = run_count(None, d, thr, metric, mode=2 if include else 1)
        np.testing.assert_array_equal(counts, h.counts)
        assert st == 0 and (np.diff(h.offsets) >= include).all()


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
def test_nothing_passes_and_everything_passes(metric):
    q, d = cases.int_rows(257, 12, 4), cases.int_rows(300, 12, 5)
    nothing, everything = (1e6, -1e6) if metric == "dot" else (0.0, 1e3)
    if metric == "euclidean":
        assert nbm.pair_values_host(q, d, metric).min() > 0
    # all-empty rows: without a buffer (count and scan only) and through the emit pass with a live buffer behind canaries
    for capacity, s in ((0, 0), (100, 0), (100, 1), (100, 2), (100, 17)):
        got = run_neighbors(q, d, nothing, metric, slices=s, capacity=capacity)
        assert got["total"] == 0 and got["status"] == 0 and (got["offsets"] == 0).all()
        assert (got["indices"] == CANARY).all() and (got["tail"] == CANARY).all() and (got["vtail"] == 7.0).all()
    h = radius_host(q, d, everything, metric)
    assert h.offsets[-1] == 257 * 300
    for s in (1, 2, 17):
        assert_list_equals_host(run_neighbors(q, d, everything, metric, slices=s), h)
    counts, _ = run_count(q, d, everything, metric)
    assert (counts == 300).all()


# ---- rounded: Gaussian blobs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", cases.LEVELS)
@pytest.mark.parametrize("case", cases.ROUNDED, ids=cases.ROUNDED_IDS)
def test_blobs_keep_every_decided_pair_and_no_other(case, which):
    n, metric = case[0], case[5]
    c = cases.rounded_case(case)
    thr, keep, undecided = cases.decided(case, which)
    share = undecided.sum() / keep.sum()
    assert share <= 0.01                                                  # a condition of the test, not a measurement
    x = dev(c["x"])
    nb = nbm.radius_neighbors(None, x, thr, metric).check()
    mask = cases.csr_mask(nb.offsets.cpu().numpy(), nb.indices.cpu().numpy(), n, n)
    assert nb.total == mask.sum() == int(nb.counts.sum().cpu())
    must, never = keep & ~undecided, ~keep & ~undecided
    differing = int((mask != keep).sum())
    print("%s: kept %d, undecided %d (%.3f %% of the kept), device differs from the host on %d pairs (%.3f %%)"
          % (which, keep.sum(), undecided.sum(), 100 * share, differing, 100 * differing / keep.sum()))
    assert not mask.diagonal().any()
    assert (mask[must]).all() and not (mask[never]).any()
    # the values are within the bound of the float64 values
    rows = np.repeat(np.arange(n), np.diff(nb.offsets.cpu().numpy()))
    cols = nb.indices.cpu().numpy()
    assert (np.abs(nb.values.cpu().numpy().astype(np.float64) - c["v"][rows, cols]) <= c["bound"][rows, cols]).all()
    # the graph stage is exact given the list: DBSCAN on the device's own list
    full = nbm.radius_neighbors(None, x, thr, metric, include_self=True, values=False).check()
    labels, core, clusters = nbm.dbscan_labels(full.offsets, full.indices32, n, 8)
    h = dbscan_host(full.offsets.cpu().numpy(), full.indices.cpu().numpy(), 8)
    np.testing.assert_array_equal(labels.cpu().numpy(), h.labels)
    np.testing.assert_array_equal(core.cpu().numpy().astype(bool), h.core)
    assert int(clusters.cpu()[0]) == h.clusters
    db = nbm.dbscan(x, thr, 8, metric).check()
    np.testing.assert_array_equal(db.labels.cpu().numpy(), h.labels)
    np.testing.assert_array_equal(db.counts.cpu().numpy(), np.diff(full.offsets.cpu().numpy()))


# ---- bits: the search's scores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [40, 768])
@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_values_are_the_scores_of_the_search(metric, dim):
    """A k = n search is out of reach (the search returns at most MAX_K = 128 neighbours): the best 128 and the best one of every
    query through the search, and every pair of the 257 x 300 through acx_knn_rescore, which gives a pair the search's bits."""
    rng = np.random.default_rng(8)
    q, d = rng.standard_normal((257, dim)).astype(np.float32), rng.standard_normal((300, dim)).astype(np.float32)
    d[7] = 0
    index = retrieval.EmbeddingIndex(dev(d), metric=metric)
    for k in (128, 1):                                                     # MAX_K = 128 < n: the best 128 of every row, and the best one
        scores, indices = index.search(dev(q), k=k)
        thr = float(scores[:, -1].min().cpu())                             # every returned pair passes this level
        nb = index.radius(dev(q), thr).check()
        table = torch.full((257, 300), float("nan"), device=DEV)
        rows = torch.repeat_interleave(torch.arange(257, device=DEV), nb.counts)
        table[rows, nb.indices] = nb.values
        listed = torch.gather(table, 1, indices)
        assert torch.equal(listed, scores)
        assert nb.total >= 257 * k
    # k = n is beyond the search's MAX_K: every pair of the 257 x 300 through the rescoring call instead, which gives any candidate
    # list the search's bits, 128 database rows at a time
    nb = index.radius(dev(q), -1e30).check()
    assert nb.total == 257 * 300
    vals = nb.values.reshape(257, 300)
    qv = retrieval._rows(dev(q), torch.device(DEV))
    rq = retrieval.row_norms(qv) if metric == "cosine" else None
    dv = index._buf[:300]
    for base in (0, 128, 256):
        cols = torch.arange(base, base + 128, dtype=torch.int32, device=DEV)
        cand = torch.where(cols < 300, cols, torch.full_like(cols, -1)).repeat(257, 1).contiguous()
        out_i = torch.empty((257, 128), dtype=torch.int32, device=DEV)
        out_s = torch.empty((257, 128), dtype=torch.float32, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        _ffi.knn_rescore(vp(qv), qv.stride(0), vp(rq), 257, vp(dv), dv.stride(0), vp(index.inverse_norms), 300, qv.shape[1],
                         _ffi.KNN_METRICS[metric], vp(cand), 128, 128, 128, vp(out_i), vp(out_s), vp(st),
                         _ffi.stream_ptr(torch.device(DEV)))
        valid = out_i >= 0
        assert int(st.cpu()[0]) == 0 and int(valid.sum().cpu()) == 257 * min(128, 300 - base)
        listed = torch.gather(vals, 1, out_i.clamp(min=0).to(torch.int64))
        assert torch.equal(listed[valid], out_s[valid])


# ---- planted duplicates -------------------------------------------------------------------------------------------------------------
def test_planted_duplicates_are_found_exactly():
    x, group, held, source_rows = cases.planted()
    lists = radius_host(None, x, 0.95, "cosine")
    want = components_host(lists.offsets, lists.indices)
    np.testing.assert_array_equal(want, group)                           # the groups are exactly the planted ones
    dup = nbm.duplicate_groups(dev(x), 0.95).check()
    np.testing.assert_array_equal(dup.labels.cpu().numpy(), want)
    np.testing.assert_array_equal(dup.sizes.cpu().numpy(), np.bincount(want, minlength=want.size)[want])
    np.testing.assert_array_equal(dup.keep.cpu().numpy(), want == np.arange(want.size))
    assert int(dup.keep.sum().cpu()) == 1500
    pairs = dup.pairs.cpu().numpy()
    assert (pairs[:, 0] < pairs[:, 1]).all() and (group[pairs[:, 0]] == group[pairs[:, 1]]).all()
    assert pairs.shape[0] == sum(len(s) * (len(s) - 1) // 2 for s in source_rows)
    groups = dup.groups()
    assert sorted(map(tuple, groups)) == sorted(tuple(s.tolist()) for s in source_rows)
    # the leak check: every held-out copy finds exactly its source and the source's copies
    leak = nbm.cross_duplicates(dev(held), dev(x), 0.95).check()
    found = leak.to_lists()
    assert len(found) == 200
    for (idx, val), rows in zip(found, source_rows):
        np.testing.assert_array_equal(idx, rows)
        assert (val > 0.99).all()
    np.testing.assert_array_equal(leak.counts.cpu().numpy(), [len(s) for s in source_rows])
    # through the index and its own inverse norms
    index = retrieval.EmbeddingIndex(dev(x))
    np.testing.assert_array_equal(index.duplicates(0.95).check().labels.cpu().numpy(), want)
    counts, _ = nbm.radius_count(dev(held), dev(x), 0.95)
    np.testing.assert_array_equal(counts.cpu().numpy(), [len(s) for s in source_rows])


# ---- components ---------------------------------------------------------------------------------------------------------------------
def run_components(offsets, indices, n, max_rounds=64, labels=None):
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    lab = nbm.components(dev(offsets, torch.int64), dev(indices, torch.int32), n, st, max_rounds, labels)
    return lab, int(st.cpu()[0])


@pytest.mark.parametrize("name", sorted(cases.graph_cases()))
def test_components_equal_the_host(name):
    offsets, indices, n, want = cases.graph_cases()[name]
    lab, st = run_components(offsets, indices, n)
    np.testing.assert_array_equal(lab.cpu().numpy(), want)
    assert st == 0


def test_long_shuffled_path_converges_and_resumes():
    n = 4097
    offsets, indices = cases.path_graph(n, seed=9)
    want = components_host(offsets, indices)
    assert (want == 0).all()
    lab, st = run_components(offsets, indices, n)
    np.testing.assert_array_equal(lab.cpu().numpy(), want)
    assert st == 0
    # two rounds are not enough; resumed calls then reach the same labels
    lab, st = run_components(offsets, indices, n, max_rounds=2)
    assert st == _ffi.GRAPH_NOT_CONVERGED
    part = lab.cpu().numpy()
    assert (part <= np.arange(n)).all() and (part != want).any()
    calls = 1
    while st:
        lab, st = run_components(offsets, indices, n, max_rounds=2, labels=lab)
        calls += 1
        assert st in (0, _ffi.GRAPH_NOT_CONVERGED) and calls <= 64
    print("calls of two rounds until stable: %d" % calls)
    np.testing.assert_array_equal(lab.cpu().numpy(), want)


# ---- DBSCAN -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 3, 5, 1000])
def test_dbscan_on_grid_points_equals_the_host_and_sklearn(min_samples):
    x = cases.grid_points()
    eps = 2.0                                                            # squared distances are integers: 4 is attained
    lists = radius_host(None, x, eps, "euclidean", include_self=True)
    h = dbscan_host(lists.offsets, lists.indices, min_samples)
    db = nbm.dbscan(dev(x), eps, min_samples).check()
    np.testing.assert_array_equal(db.labels.cpu().numpy(), h.labels)
    np.testing.assert_array_equal(db.core.cpu().numpy(), h.core)
    np.testing.assert_array_equal(db.counts.cpu().numpy(), lists.counts)
    np.testing.assert_array_equal(db.noise.cpu().numpy(), h.labels < 0)
    assert int(db.clusters.cpu()) == h.clusters
    try:                                                                 # scikit-learn, where it is installed
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    if DBSCAN is not None:
        sk = DBSCAN(eps=eps, min_samples=min_samples, algorithm="brute").fit(x.astype(np.float64))
        np.testing.assert_array_equal(h.labels, sk.labels_)
        np.testing.assert_array_equal(np.flatnonzero(h.core), sk.core_sample_indices_)
        assert h.clusters == sk.labels_.max() + 1
    if min_samples == 5:
        border = ~h.core & (h.labels >= 0)
        assert h.clusters == 3 and border.sum() >= 2 and (h.labels < 0).sum() >= 5       # bridge ends are border, its middle is noise


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes():
    c = cases.rounded_case(cases.ROUNDED[2])
    thr = c["thresholds"]["median"]
    runs = []
    for _ in range(2):
        nb = nbm.radius_neighbors(None, dev(c["x"]), thr, "euclidean", include_self=True)
        labels, core, clusters = nbm.dbscan_labels(nb.offsets, nb.indices32, c["x"].shape[0], 8)
        runs.append((nb.offsets, nb.indices32, nb.values, labels, core, clusters))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    sliced = nbm.radius_neighbors(None, dev(c["x"]), thr, "euclidean", include_self=True, slices=5)
    assert torch.equal(sliced.indices32, runs[0][1]) and torch.equal(sliced.values, runs[0][2])


def test_captured_graph_replays_the_eager_bytes():
    c = cases.rounded_case(cases.ROUNDED[2])
    thr, n = c["thresholds"]["median"], c["x"].shape[0]
    x = retrieval._rows(dev(c["x"]), torch.device(DEV))
    xx = nbm.row_sumsq(x)
    level = float(nbm.level_of(thr, "euclidean"))
    eager = nbm.radius_neighbors(None, x, thr, "euclidean", include_self=True)
    e_labels, e_core, e_clusters = nbm.dbscan_labels(eager.offsets, eager.indices32, n, 8)
    cap = eager.total
    off = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    idx = torch.empty(cap, dtype=torch.int32, device=DEV)
    val = torch.empty(cap, dtype=torch.float32, device=DEV)
    total = torch.empty(1, dtype=torch.int64, device=DEV)
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    core = torch.empty(n, dtype=torch.uint8, device=DEV)
    clusters = torch.empty(1, dtype=torch.int32, device=DEV)
    st = torch.empty(2, dtype=torch.int32, device=DEV)
    nb = _ffi.radius_workspace_bytes(n, n, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    nd = _ffi.dbscan_workspace_bytes(n)
    wd = torch.empty(nd, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = _ffi.stream_ptr(torch.device(DEV))
        _ffi.radius_neighbors(vp(x), x.stride(0), vp(xx), n, vp(x), x.stride(0), vp(xx), n, x.shape[1], _ffi.RADIUS_EUCLIDEAN, level,
                              _ffi.RADIUS_SELF_INCLUDE, 0, vp(off), vp(idx), vp(val), cap, vp(total), vp(st), (vp(ws), nb), s)
        _ffi.dbscan_labels(vp(off), vp(idx), n, 8, vp(labels), vp(core), vp(clusters), vp(st[1:]), (vp(wd), nd), 16, s)
    for _ in range(2):
        for t in (off, idx, total, labels, clusters, st):
            t.fill_(-3)
        val.fill_(-3.0)
        core.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        assert st.tolist() == [0, 0] and int(total) == cap
        assert torch.equal(off, eager.offsets) and torch.equal(idx, eager.indices32) and torch.equal(val, eager.values)
        assert torch.equal(labels, e_labels) and torch.equal(core, e_core) and torch.equal(clusters, e_clusters)


def test_overflow_leaves_the_total_the_offsets_and_the_canaries():
    q, d = cases.int_rows(257, 12, 4), cases.int_rows(300, 12, 5)
    v = nbm.pair_values_host(q, d, "dot")
    thr = cases.attained_level(v, "dot", 0.6)
    h = radius_host(q, d, thr, "dot")
    total = int(h.offsets[-1])
    for capacity in (total - 1, total // 2, 1):
        for s in (0, 17):
            got = run_neighbors(q, d, thr, "dot", slices=s, capacity=capacity)
            assert got["status"] == _ffi.RADIUS_OVERFLOW and got["total"] == total
            np.testing.assert_array_equal(got["offsets"], h.offsets)
            np.testing.assert_array_equal(got["indices"], h.indices[:capacity])
            np.testing.assert_array_equal(got["values"], h.values[:capacity])
            assert (got["tail"] == CANARY).all() and (got["vtail"] == 7.0).all()
    # the Python call counts, reads the total and emits once into a list of that size
    nb = nbm.radius_neighbors(dev(q), dev(d), thr, "dot").check()
    assert nb.total == total == nb.indices32.numel() == nb.values.numel()
    np.testing.assert_array_equal(nb.indices.cpu().numpy(), h.indices)
    np.testing.assert_array_equal(nb.values.cpu().numpy(), h.values)


@pytest.mark.parametrize("slices", [0, 17])
def test_emit_alone_completes_a_counting_call(slices):
    """acx_radius_neighbors with capacity 0 (count and scan), then acx_radius_emit on the same workspace: the host's list; with too
    small a capacity the overflow bit, the prefix and the canaries."""
    q, d = cases.int_rows(257, 12, 4), cases.int_rows(300, 12, 5)
    thr = cases.attained_level(nbm.pair_values_host(q, d, "euclidean"), "euclidean", 0.3)
    h = radius_host(q, d, thr, "euclidean")
    total = int(h.offsets[-1])
    qv, dv = rows_on_device(q), rows_on_device(d)
    qa, da = aux_of(qv, "euclidean"), aux_of(dv, "euclidean")
    off = torch.full((258,), -7, dtype=torch.int64, device=DEV)
    tot = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    st = torch.full((1,), 255, dtype=torch.int32, device=DEV)
    nb = _ffi.radius_workspace_bytes(257, 300, slices)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    args = (vp(qv), qv.stride(0), vp(qa), 257, vp(dv), dv.stride(0), vp(da), 300, 12, _ffi.RADIUS_EUCLIDEAN,
            float(nbm.level_of(thr, "euclidean")), 0, slices, vp(off))
    stream = _ffi.stream_ptr(torch.device(DEV))
    _ffi.radius_neighbors(*args, None, None, 0, vp(tot), vp(st), (vp(ws), nb), stream)
    assert int(tot.cpu()[0]) == total and int(st.cpu()[0]) == _ffi.RADIUS_OVERFLOW
    np.testing.assert_array_equal(off.cpu().numpy(), h.offsets)
    for capacity in (total, total - 1, total + 5):
        idx = torch.full((capacity + 64,), CANARY, dtype=torch.int32, device=DEV)
        val = torch.full((capacity + 64,), 7.0, dtype=torch.float32, device=DEV)
        _ffi.radius_emit(*args, vp(idx), vp(val), capacity, vp(tot), vp(st), (vp(ws), nb), stream)
        kept = min(capacity, total)
        assert int(st.cpu()[0]) == (_ffi.RADIUS_OVERFLOW if capacity < total else 0) and int(tot.cpu()[0]) == total
        np.testing.assert_array_equal(idx[:kept].cpu().numpy(), h.indices[:kept])
        np.testing.assert_array_equal(val[:kept].cpu().numpy(), h.values[:kept])
        assert (idx[kept:] == CANARY).all() and (val[kept:] == 7.0).all()
        np.testing.assert_array_equal(off.cpu().numpy(), h.offsets)


def test_nan_rows_set_nonfinite_and_are_never_kept():
    d = cases.int_rows(130, 12, 6)
    d[77, 3] = np.nan
    for metric, thr in (("dot", 1.0), ("cosine", 0.1), ("euclidean", 9.0)):
        got = run_neighbors(None, d, thr, metric, mode=1, capacity=130 * 130)
        assert got["status"] == _ffi.RADIUS_NONFINITE
        mask = cases.csr_mask(got["offsets"], got["indices"][:got["total"]], 130, 130)
        assert not mask[77].any() and not mask[:, 77].any() and mask.any()
        with pytest.raises(ValueError, match="NaN or infinite"):
            nbm.radius_neighbors(None, dev(d), 1.0, metric).check()
    with pytest.raises(ValueError, match="NaN or infinite"):
        nbm.dbscan(dev(d), 3.0).check()


def test_bad_indices_set_the_flag_and_touch_nothing_else():
    n = 9
    offsets, indices = cases.csr_of(n, cases.both([(0, 1), (1, 2), (4, 5), (7, 8)]))
    bad = indices.copy()
    bad[0] = n                                                           # (0 -> 9)
    bad[-1] = -1                                                         # (8 -> -1)
    want = components_host(offsets, bad)
    np.testing.assert_array_equal(want, [0, 0, 0, 3, 4, 4, 6, 7, 7])
    guard = 64
    lab = torch.full((n + guard,), CANARY, dtype=torch.int32, device=DEV)
    st = torch.full((2,), 255, dtype=torch.int32, device=DEV)
    off_d, bad_d = dev(offsets, torch.int64), dev(bad, torch.int32)
    _ffi.graph_components(vp(off_d), vp(bad_d), n, vp(lab), vp(st), 16, False, _ffi.stream_ptr(torch.device(DEV)))
    assert st.tolist() == [_ffi.GRAPH_BAD_INDEX, 255] and (lab[n:] == CANARY).all()
    np.testing.assert_array_equal(lab[:n].cpu().numpy(), want)
    labels = torch.full((n + guard,), CANARY, dtype=torch.int32, device=DEV)
    core = torch.full((n + guard,), 0x5a, dtype=torch.uint8, device=DEV)
    clusters = torch.full((1 + guard,), CANARY, dtype=torch.int32, device=DEV)
    nd = _ffi.dbscan_workspace_bytes(n)
    wd = torch.empty(nd, dtype=torch.uint8, device=DEV)
    _ffi.dbscan_labels(vp(off_d), vp(bad_d), n, 2, vp(labels), vp(core), vp(clusters), vp(st), (vp(wd), nd), 16,
                       _ffi.stream_ptr(torch.device(DEV)))
    h = dbscan_host(offsets, bad, 2)
    assert st.tolist() == [_ffi.GRAPH_BAD_INDEX, 255]
    assert (labels[n:] == CANARY).all() and (core[n:] == 0x5a).all() and (clusters[1:] == CANARY).all()
    np.testing.assert_array_equal(labels[:n].cpu().numpy(), h.labels)
    np.testing.assert_array_equal(core[:n].cpu().numpy().astype(bool), h.core)
    assert int(clusters[0].cpu()) == h.clusters
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbm.components(off_d, bad_d, n, word)
    assert "outside" in nbm._status_error(int(word.cpu()[0]))


def test_clustered_rows_feed_the_cluster_scores():
    """silhouette() and dispersion_scores() take labels in [0, clusters): a DBSCAN result goes in through its clustered rows."""
    from audioset_convnext_inf_amd.pytorch import cluster_scores as cs
    x = cases.grid_points()
    db = nbm.dbscan(dev(x), 2.0, 5).check()
    rows, labels = db.clustered()
    K = int(db.clusters.cpu())
    assert K == 3 and 0 < rows.numel() < x.shape[0] and int(labels.min().cpu()) == 0 and int(labels.max().cpu()) == K - 1
    np.testing.assert_array_equal(rows.cpu().numpy(), np.flatnonzero(db.labels.cpu().numpy() >= 0))
    sub = x[rows.cpu().numpy()]
    sil = cs.silhouette(dev(sub), labels, clusters=K).check()
    host = cs.silhouette_host(sub, labels.cpu().numpy(), "euclidean", K)
    assert np.abs(sil.values.cpu().numpy() - host.values).max() <= 1e-6 and float(sil) > 0.5
    disp = cs.dispersion_scores(dev(sub), labels, K).check()
    np.testing.assert_array_equal(disp.counts.cpu().numpy(), np.bincount(labels.cpu().numpy(), minlength=K))
    with pytest.raises(ValueError, match="label"):                     # the noise rows themselves are in no cluster
        cs.silhouette(dev(x), db.labels, clusters=K).check()


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def test_index_entry_points_agree_with_the_functions():
    c = cases.rounded_case(cases.ROUNDED[2])
    x = dev(c["x"])
    index = retrieval.EmbeddingIndex(x, metric="cosine")
    a = index.radius(None, 0.05).check()
    b = nbm.radius_neighbors(None, x, 0.05, "cosine").check()
    assert torch.equal(a.offsets, b.offsets) and torch.equal(a.indices32, b.indices32) and torch.equal(a.values, b.values)
    da, db = index.dbscan(0.05, 8).check(), nbm.dbscan(x, 0.05, 8, "cosine").check()
    assert torch.equal(da.labels, db.labels) and torch.equal(da.core, db.core)
    with pytest.raises(ValueError, match="empty"):
        retrieval.EmbeddingIndex(torch.empty((0, 8), device=DEV)).radius(None, 0.5)
