"""CPU: radius search, components and DBSCAN (pytorch/neighbors.py; acx_radius_count, acx_radius_neighbors, acx_graph_components,
acx_dbscan_labels in include/acx.h) -- the numpy host definitions against scikit-learn and hand-worked cases, a Python restatement
of the tile kernel's ballot and rank walk against the host definition, the premise of the GPU test's rounded cases, and the
host-only paths of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import neighbors_cases as cases
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import neighbors as nbm
from audioset_convnext_inf_amd.pytorch.neighbors import components_host, dbscan_host, radius_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acx_radius_workspace_bytes", "acx_radius_slices", "acx_radius_row_sumsq", "acx_radius_count", "acx_radius_neighbors",
         "acx_radius_emit", "acx_graph_components", "acx_dbscan_workspace_bytes", "acx_dbscan_labels")

# (n, dim, K, sep, seed, threshold, min_samples, metric): float64 blobs with at least 50 border points each
SKLEARN = [(400, 4, 6, 3.0, 1, 1.2, 6, "euclidean"), (600, 2, 8, 4.0, 2, 0.45, 6, "euclidean"), (500, 8, 5, 3.0, 3, 2.4, 6, "euclidean"),
           (500, 8, 5, 3.0, 4, 0.97, 8, "cosine")]


# ---- the host definitions against scikit-learn -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SKLEARN, ids=lambda c: "%dx%d-%s" % (c[0], c[1], c[7]))
def test_dbscan_host_equals_sklearn(case):
    skc = pytest.importorskip("sklearn.cluster")
    n, dim, K, sep, seed, thr, ms, metric = case
    x, _ = cases.blobs(n, dim, K, sep, seed, np.float64)
    lists = radius_host(None, x, thr, metric, include_self=True)
    got = dbscan_host(lists.offsets, lists.indices, ms)
    if metric == "cosine":                                    # scikit-learn's cosine distance: 1 - cos <= eps
        sk = skc.DBSCAN(eps=1.0 - thr, min_samples=ms, algorithm="brute", metric="cosine").fit(x)
    else:
        sk = skc.DBSCAN(eps=thr, min_samples=ms, algorithm="brute").fit(x)
    core = np.zeros(n, dtype=bool)
    core[sk.core_sample_indices_] = True
    border = ~core & (sk.labels_ >= 0)
    print("clusters %d, border points %d, noise %d" % (got.clusters, border.sum(), (sk.labels_ < 0).sum()))
    assert border.sum() >= 50
    np.testing.assert_array_equal(got.labels, sk.labels_)
    np.testing.assert_array_equal(got.core, core)
    np.testing.assert_array_equal(~got.core & (got.labels >= 0), border)
    assert got.clusters == sk.labels_.max() + 1


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.graph_cases()))
def test_components_host_hand_worked(name):
    offsets, indices, n, want = cases.graph_cases()[name]
    np.testing.assert_array_equal(components_host(offsets, indices), want)
    np.testing.assert_array_equal(components_host(offsets, indices, n), want)


def test_components_host_skips_bad_indices_and_checks_its_form():
    offsets, indices = cases.csr_of(4, [(0, 2), (3, 1)])
    indices = indices.copy()
    indices[0] = 9
    np.testing.assert_array_equal(components_host(offsets, indices), [0, 1, 2, 1])
    with pytest.raises(ValueError, match="offsets"):
        components_host(offsets, indices, 7)
    with pytest.raises(ValueError, match="offsets"):
        components_host([0], [])


def test_radius_host_thresholds_are_inclusive():
    x = np.array([[1.0, 0, 0, 0], [2, 0, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]])
    # dot products with row 1: 2, 4, 0, 8 -- a value exactly at the level is kept
    h = radius_host(x[1:2], x, 4.0, "dot")
    np.testing.assert_array_equal(h.indices, [1, 3])
    np.testing.assert_array_equal(h.values, [4, 8])
    np.testing.assert_array_equal(h.offsets, [0, 2])
    assert radius_host(x[1:2], x, np.nextafter(np.float32(4), np.float32(5)), "dot").indices.tolist() == [3]
    # squared distances from row 0: 0, 1, 10, 25; eps = 1 keeps the distance exactly 1
    e = radius_host(x[:1], x, 1.0, "euclidean")
    np.testing.assert_array_equal(e.indices, [0, 1])
    np.testing.assert_array_equal(e.values, [0, 1])
    assert radius_host(x[:1], x, 5.0, "euclidean").indices.tolist() == [0, 1, 2, 3]
    # cosine of row 3 with the rows: 1 / sqrt 2, 1 / sqrt 2, 1 / sqrt 2, 1
    c = radius_host(x[3:], x, 0.7, "cosine")
    np.testing.assert_array_equal(c.indices, [0, 1, 2, 3])
    # a self-join decides (i, i) by position
    s = radius_host(None, x, 100.0, "dot", include_self=True)
    np.testing.assert_array_equal(s.indices, [0, 1, 2, 3])
    assert radius_host(None, x, 100.0, "dot").indices.size == 0
    s0 = radius_host(None, x, -1.0, "dot")
    np.testing.assert_array_equal(s0.counts, [3, 3, 3, 3])
    np.testing.assert_array_equal(s0.indices[:3], [1, 2, 3])
    # a NaN is never kept; a zero row has cosine 0 with everything
    xn = x.copy()
    xn[2, 0] = np.nan
    assert radius_host(xn[:1], xn, -1e30, "dot").indices.tolist() == [0, 1, 3]
    z = radius_host(np.zeros((1, 4)), x, 0.0, "cosine")
    np.testing.assert_array_equal(z.counts, [4])
    # precomputed fp32 values against the fp32 level
    v = np.array([[0.1, 0.3, np.float32(0.3) - np.float32(1e-7)]], dtype=np.float32)
    assert radius_host(np.zeros((1, 4)), np.zeros((3, 4)), 0.3, "cosine", values=v).indices.tolist() == [1]
    assert float(nbm.level_of(3.0, "euclidean")) == 9.0 and nbm.level_of(0.1, "cosine") == np.float32(0.1)


def test_dbscan_host_hand_worked():
    # a line: 0 1 2 | 4 | 6 7 8 9, eps = 1, min_samples = 3: cores 1, 7, 8; 0, 2, 6, 9 border; 4 noise
    x = np.array([0, 1, 2, 4, 6, 7, 8, 9], dtype=np.float64)[:, None] * np.array([[1.0, 0, 0, 0]])
    lists = radius_host(None, x, 1.0, "euclidean", include_self=True)
    r = dbscan_host(lists.offsets, lists.indices, 3)
    np.testing.assert_array_equal(r.core, [0, 1, 0, 0, 0, 1, 1, 0])
    np.testing.assert_array_equal(r.labels, [0, 0, 0, -1, 1, 1, 1, 1])
    assert r.clusters == 2
    # a border row between two clusters takes the smaller number: 0 1 2 3 4 with cores 1 and 3 that do not see each other
    y = np.array([0, 1, 2, 3, 4, 0.5, 3.5], dtype=np.float64)[:, None] * np.array([[1.0, 0, 0, 0]])
    lists = radius_host(None, y, 1.0, "euclidean", include_self=True)
    r = dbscan_host(lists.offsets, lists.indices, 4)
    np.testing.assert_array_equal(r.core, [0, 1, 0, 1, 0, 0, 0])
    np.testing.assert_array_equal(r.labels, [0, 0, 0, 1, 1, 0, 1])
    # min_samples = 1: every row is core, the clusters are the components; larger than n: everything is noise
    r1 = dbscan_host(lists.offsets, lists.indices, 1)
    assert r1.core.all() and r1.clusters == 1 and (r1.labels == 0).all()
    rn = dbscan_host(lists.offsets, lists.indices, 100)
    assert not rn.core.any() and rn.clusters == 0 and (rn.labels == -1).all()
    with pytest.raises(ValueError, match="min_samples"):
        dbscan_host(lists.offsets, lists.indices, 0)


# ---- the kernel's walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,slices", [((1, 1), 0), ((65, 130), 1), ((130, 200), 2), ((70, 257), 17), ((64, 64), 0)])
def test_walk_equals_the_host_definition(shape, slices):
    """Ballots, popcounts below the lane's bit, running counts per tile row, the scan in (query, range) order: the list the kernel
    builds must be the host definition's, ascending inside each row, whatever the slicing."""
    nq, n = shape
    q, d = cases.int_rows(nq, 8, 1), cases.int_rows(n, 8, 2)
    v = nbm.pair_values_host(q, d, "dot")
    thr = cases.attained_level(v, "dot", 0.7)
    h = radius_host(q, d, thr, "dot")
    assert 0 < h.indices.size < nq * n or nq * n == 1
    offsets, indices = cases.walk_radius(v >= thr, slices)
    np.testing.assert_array_equal(offsets, h.offsets)
    np.testing.assert_array_equal(indices, h.indices)


def test_geometry_equals_the_library():
    for nq, n, s in ((1, 1, 0), (64, 64, 0), (300, 1025, 17), (300, 1025, 2), (20371, 20371, 0), (200000, 200000, 0), (5, 1 << 20, 0),
                     (257, 300, 1), (1025, 300, 17), (100, 100000, 64)):
        ns, length = cases.geometry(nq, n, s)
        assert _ffi.radius_slices(nq, n, s) == ns, (nq, n, s)
        assert ns <= _ffi.RADIUS_MAX_SLICES and length % 64 == 0 and (ns - 1) * length < n <= ns * length
    # 80 query tiles: 64 ranges of 320 rows are 5 120 workgroups, 20 per compute unit exactly; 7 ranges would leave 3 on some, 2 on most
    assert cases.geometry(20371, 20371) == (64, 320) and cases.geometry(300, 1025, 17) == (17, 64)
    assert cases.geometry(4097, 4097) == (13, 320) and cases.geometry(1, 1) == (1, 64)
    assert [cases.tile_row(i, 0) for i in range(16)] == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert sorted(cases.tile_row(i, h) for i in range(16) for h in range(2)) == list(range(32))


# ---- the premise of the GPU test's rounded cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.ROUNDED, ids=cases.ROUNDED_IDS)
def test_undecided_pairs_are_at_most_one_percent(case):
    """The pairs whose float64 value lies within the fp32 rounding bound of the level -- which the device may decide either way --
    are at most 1 % of the pairs the host keeps, at both levels of every case."""
    for which in cases.LEVELS:
        thr, keep, undecided = cases.decided(case, which)
        share = undecided.sum() / keep.sum()
        print("%s: threshold %.5f, kept %d (%.1f per row), undecided %d = %.3f %%" % (which, thr, keep.sum(), keep.sum() / case[0],
                                                                                     undecided.sum(), 100 * share))
        assert keep.sum() > case[0] and share <= 0.01


def test_fp32_formula_stays_inside_the_pair_bound():
    """The device's fp32 formulas emulated in numpy (numpy's own summation order): inside the bounds, which do not depend on order."""
    for case in cases.ROUNDED[:3]:
        c = cases.rounded_case(case)
        x = c["x"]
        dot = x @ x.T
        if c["metric"] == "euclidean":
            xx = (x * x).sum(axis=1, dtype=np.float32)
            v = np.maximum(np.float32(-2.0) * dot + (xx[:, None] + xx[None, :]), np.float32(0))
        else:
            r = (np.float32(1) / np.sqrt((x * x).sum(axis=1, dtype=np.float32))).astype(np.float32)
            v = (dot * r[:, None]) * r[None, :]
        assert v.dtype == np.float32
        ratio = float((np.abs(v.astype(np.float64) - c["v"])[c["off"]] / c["bound"][c["off"]]).max())
        print("%s: worst fp32 err / bound = %.3f" % (case, ratio))
        assert ratio <= 1.0


def test_planted_duplicates_have_no_undecided_pair():
    x, group, held, source_rows = cases.planted()
    x64 = x.astype(np.float64)
    r = 1.0 / np.sqrt((x64 * x64).sum(axis=1))
    v = (x64 @ x64.T) * r[:, None] * r[None, :]
    same = group[:, None] == group[None, :]
    assert v[same].min() > 0.99 and v[~same].max() < 0.5              # nothing near the threshold 0.95: far beyond any rounding
    lists = radius_host(None, x, 0.95, "cosine")
    np.testing.assert_array_equal(components_host(lists.offsets, lists.indices), group)
    sizes = np.bincount(group, minlength=group.size)[group]
    assert (sizes > 1).sum() == sum(len(s) for s in source_rows) and len(source_rows) == 200
    assert all(3 <= len(s) <= 6 for s in source_rows)


# ---- the C ABI: declarations and host-only paths ------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    for name in NAMES:
        assert re.search(r"ACX_API int %s\(" % name, header), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert _ffi.SIGNATURES[name][0] is ctypes.c_int
    assert [len(_ffi.SIGNATURES[k][1]) for k in NAMES] == [4, 4, 6, 17, 22, 22, 8, 2, 12]
    for name, value in (("ACX_RADIUS_NONFINITE", 1), ("ACX_RADIUS_OVERFLOW", 2), ("ACX_GRAPH_BAD_INDEX", 4), ("ACX_GRAPH_NOT_CONVERGED", 8),
                        ("ACX_RADIUS_MAX_SLICES", 64), ("ACX_GRAPH_MAX_ROUNDS", 4096)):
        assert re.search(r"#define %s %d\b" % (name, value), header) and getattr(_ffi, name[4:]) == value
    assert "enum acx_radius_metric { ACX_RADIUS_DOT = 0, ACX_RADIUS_COSINE = 1, ACX_RADIUS_EUCLIDEAN = 2 }" in header
    assert "enum acx_radius_self { ACX_RADIUS_SELF_NONE = 0, ACX_RADIUS_SELF_EXCLUDE = 1, ACX_RADIUS_SELF_INCLUDE = 2 }" in header
    assert _ffi.RADIUS_METRICS == {"dot": 0, "cosine": 1, "euclidean": 2}
    assert (_ffi.RADIUS_SELF_NONE, _ffi.RADIUS_SELF_EXCLUDE, _ffi.RADIUS_SELF_INCLUDE) == (0, 1, 2)
    # the search's metrics and its non-finite bit keep their values here: the inverse norms' status word is OR-ed in as it is
    assert _ffi.RADIUS_DOT == _ffi.KNN_DOT and _ffi.RADIUS_COSINE == _ffi.KNN_COSINE and _ffi.RADIUS_NONFINITE == _ffi.KNN_NONFINITE
    src = open(os.path.join(ROOT, "audioset-convnext-inf_amd", "csrc", "Makefile")).read()
    assert " neighbors.hip" in src and src.count("build/acx/neighbors.o") >= 2


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _nb_rc(fn="acx_radius_neighbors", q=64, ld_q=None, qa=64, nq=16, d=64, ld_d=None, da=64, n=16, dim=8, metric=1, level=0.5, mode=0, slices=0, off=64, idx=64,
           val=64, cap=100, total=64, st=64, ws=256, ws_bytes=1 << 40):
    return getattr(_ffi.lib(), fn)(_p(q), dim if ld_q is None else ld_q, _p(qa), nq, _p(d), dim if ld_d is None else ld_d, _p(da),
                                           n, dim, metric, level, mode, slices, _p(off), _p(idx), _p(val), cap, _p(total), _p(st), _p(ws),
                                           ws_bytes, None)


def _cnt_rc(q=64, ld_q=None, qa=64, nq=16, d=64, ld_d=None, da=64, n=16, dim=8, metric=1, level=0.5, mode=0, counts=64, st=64, ws=256,
            ws_bytes=1 << 40):
    return _ffi.lib().acx_radius_count(_p(q), dim if ld_q is None else ld_q, _p(qa), nq, _p(d), dim if ld_d is None else ld_d, _p(da), n,
                                       dim, metric, level, mode, _p(counts), _p(st), _p(ws), ws_bytes, None)


def _comp_rc(off=64, idx=64, n=16, labels=64, st=64, rounds=8, resume=0):
    return _ffi.lib().acx_graph_components(_p(off), _p(idx), n, _p(labels), _p(st), rounds, resume, None)


def _db_rc(off=64, idx=64, n=16, ms=5, labels=64, core=64, clusters=64, st=64, ws=256, ws_bytes=1 << 40, rounds=8):
    return _ffi.lib().acx_dbscan_labels(_p(off), _p(idx), n, ms, _p(labels), _p(core), _p(clusters), _p(st), _p(ws), ws_bytes, rounds, None)


PAIR_BAD = (dict(q=None), dict(d=None), dict(q=68), dict(d=72), dict(nq=0), dict(n=0), dict(dim=6), dict(dim=0),
            dict(dim=_ffi.KNN_MAX_DIM + 4), dict(ld_q=4), dict(ld_d=10), dict(qa=None), dict(da=None), dict(metric=3), dict(metric=-1),
            dict(level=float("nan")), dict(mode=3), dict(mode=-1), dict(mode=1, nq=15), dict(mode=2, n=17), dict(st=None), dict(ws=None))


def test_argument_errors_return_before_any_launch():
    lib = _ffi.lib()
    for kw in PAIR_BAD + (dict(off=None), dict(total=None), dict(off=68), dict(total=68), dict(idx=None), dict(cap=-1), dict(slices=-1),
                          dict(slices=_ffi.RADIUS_MAX_SLICES + 1)):
        assert _nb_rc(**kw) == -1, kw
        assert lib.acx_last_error()
        assert _nb_rc(fn="acx_radius_emit", **kw) == -1, kw
    assert b"acx_radius_emit" in (_nb_rc(fn="acx_radius_emit", cap=-1), lib.acx_last_error())[1]
    assert _nb_rc(fn="acx_radius_emit", ws_bytes=0) == -5 and _nb_rc(fn="acx_radius_emit", n=(1 << 30) + 1) == -6
    assert b"NaN" in (_nb_rc(level=float("nan")), lib.acx_last_error())[1]
    assert b"self-join" in (_nb_rc(mode=1, nq=15), lib.acx_last_error())[1]
    assert b"slices = 65" in (_nb_rc(slices=65), lib.acx_last_error())[1]
    assert _nb_rc(ws_bytes=0) == -5 and _nb_rc(ws=264) == -5 and _nb_rc(n=(1 << 30) + 1) == -6 and _nb_rc(nq=(1 << 30) + 1) == -6
    for kw in PAIR_BAD + (dict(counts=None),):
        assert _cnt_rc(**kw) == -1, kw
    assert _cnt_rc(ws_bytes=0) == -5 and _cnt_rc(ws=264) == -5 and _cnt_rc(n=(1 << 30) + 1) == -6
    assert lib.acx_radius_row_sumsq(_p(64), 8, 0, 8, _p(64), None) == -1 and lib.acx_radius_row_sumsq(_p(64), 8, 4, 8, None, None) == -1
    assert lib.acx_radius_row_sumsq(_p(64), 8, 4, 6, _p(64), None) == -1 and lib.acx_radius_row_sumsq(None, 8, 4, 8, _p(64), None) == -1
    for kw in (dict(off=None), dict(idx=None), dict(n=0), dict(labels=None), dict(st=None), dict(rounds=0), dict(off=68),
               dict(rounds=_ffi.GRAPH_MAX_ROUNDS + 1)):
        assert _comp_rc(**kw) == -1, kw
        assert _db_rc(**kw) == -1, kw
    assert _comp_rc(n=(1 << 30) + 1) == -6 and _db_rc(n=(1 << 30) + 1) == -6
    for kw in (dict(ms=0), dict(ms=-3), dict(core=None), dict(clusters=None), dict(ws=None)):
        assert _db_rc(**kw) == -1, kw
    assert b"min_samples = -3" in (_db_rc(ms=-3), lib.acx_last_error())[1]
    assert _db_rc(ws_bytes=0) == -5 and _db_rc(ws=264) == -5


def test_workspace_bytes_non_decreasing():
    size = ctypes.c_size_t()
    lib = _ffi.lib()
    assert lib.acx_radius_workspace_bytes(16, 16, 0, None) == -1 and lib.acx_dbscan_workspace_bytes(16, None) == -1
    assert lib.acx_radius_slices(16, 16, 0, None) == -1
    for nq, n, s in ((0, 8, 0), (8, 0, 0), (8, 8, -1), (8, 8, 65)):
        assert lib.acx_radius_workspace_bytes(nq, n, s, ctypes.byref(size)) == -1, (nq, n, s)
    assert lib.acx_radius_workspace_bytes((1 << 30) + 1, 8, 0, ctypes.byref(size)) == -6
    assert lib.acx_dbscan_workspace_bytes(0, ctypes.byref(size)) == -1 and lib.acx_dbscan_workspace_bytes((1 << 30) + 1, ctypes.byref(size)) == -6
    nqs = [1, 63, 64, 65, 255, 256, 257, 1025, 20371, 200000, 1 << 20, 1 << 30]
    for s in (1, 2, 17, 64):
        for n in (1, 64, 65, 20371, 1 << 30):
            sizes = np.array([_ffi.radius_workspace_bytes(nq, n, s) for nq in nqs], dtype=np.float64)
            assert (sizes > 0).all() and (sizes % 256 == 0).all() and (np.diff(sizes) >= 0).all()
    db = np.array([_ffi.dbscan_workspace_bytes(n) for n in nqs], dtype=np.float64)
    assert (db > 0).all() and (db % 256 == 0).all() and (np.diff(db) >= 0).all()
    # counts and positions per (query, range), far below the nq x n values (20 371^2 fp32 = 1.7 GB)
    assert _ffi.radius_workspace_bytes(20371, 20371) < 16 << 20


# ---- the Python API: errors raised before any device call ---------------------------------------------------------------------------
def test_python_value_errors_need_no_device():
    e = np.zeros((5, 8), np.float32)
    with pytest.raises(ValueError, match="metric"):
        nbm.radius_neighbors(None, e, 0.5, metric="l1")
    with pytest.raises(ValueError, match="2-D"):
        nbm.radius_neighbors(None, np.zeros(8, np.float32), 0.5)
    with pytest.raises(ValueError, match="NaN"):
        nbm.radius_count(None, e, float("nan"))
    with pytest.raises(ValueError, match="eps = -1"):
        nbm.dbscan(e, -1.0)
    with pytest.raises(ValueError, match="min_samples = 0"):
        nbm.dbscan(e, 1.0, min_samples=0)
    with pytest.raises(ValueError, match="max_rounds = 0"):
        nbm.dbscan(e, 1.0, max_rounds=0)
    with pytest.raises(ValueError, match="max_rounds"):
        nbm.duplicate_groups(e, max_rounds=_ffi.GRAPH_MAX_ROUNDS + 1)
    with pytest.raises(ValueError, match="no rows"):
        nbm.radius_neighbors(None, np.zeros((0, 8), np.float32), 0.5)
    with pytest.raises(ValueError, match="not cpu"):
        nbm.radius_neighbors(None, e, 0.5, device="cpu")
    with pytest.raises(ValueError, match="not cpu"):
        nbm.duplicate_groups(e, device="cpu")
    with pytest.raises(ValueError, match="not cpu"):
        nbm.dbscan(e, 1.0, device="cpu")
    with pytest.raises(ValueError, match="queries"):
        nbm.cross_duplicates(None, e)
    with pytest.raises(ValueError, match="metric"):
        radius_host(None, e, 0.5, "l1")
    assert nbm.METRICS == ("dot", "cosine", "euclidean") and nbm.MAX_ROUNDS <= _ffi.GRAPH_MAX_ROUNDS
