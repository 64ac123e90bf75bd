"""CPU: cluster validation (pytorch/cluster_scores.py; acx_silhouette, acx_cluster_dispersion, acx_contingency in include/acx.h)
-- the numpy host definitions against scikit-learn and hand-worked cases, a Python restatement of the silhouette kernel's walk
against the host definition, the premise of the GPU test's `nearest` check, and the host-only paths of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_scores_cases as cases
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import cluster_scores as cs
from audioset_convnext_inf_amd.pytorch.cluster_scores import agreement_host, dispersion_host, ordered_sum, silhouette_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acx_cluster_scores_workspace_bytes", "acx_silhouette", "acx_cluster_dispersion", "acx_contingency")


# ---- the host definitions against scikit-learn -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["geometric", "random"])
@pytest.mark.parametrize("case", cases.SKLEARN_SHAPES, ids=cases.GAUSS_IDS[:3])
def test_host_definitions_equal_sklearn(case, which):
    skm = pytest.importorskip("sklearn.metrics")
    x, geo, rand = cases.gauss(*case)
    labels = geo if which == "geometric" else rand
    x64 = x.astype(np.float64)
    h = silhouette_host(x, labels)
    ref = skm.silhouette_samples(x64, labels)
    err = np.abs(h.values - ref).max()
    d = dispersion_host(x, labels)
    e_ch = abs(d.calinski_harabasz - skm.calinski_harabasz_score(x64, labels))
    e_db = abs(d.davies_bouldin - skm.davies_bouldin_score(x64, labels))
    print("silhouette %.2e, calinski-harabasz %.2e, davies-bouldin %.2e" % (err, e_ch, e_db))
    assert err <= 1e-12 and abs(h.mean - ref.mean()) <= 1e-12
    for c in range(case[2]):
        assert abs(h.cluster_mean[c] - ref[labels == c].mean()) <= 1e-12
    assert e_ch <= 1e-12 and e_db <= 1e-12
    np.testing.assert_array_equal(d.counts, np.bincount(labels, minlength=case[2]))
    assert np.abs(d.means - np.stack([x64[labels == c].mean(axis=0) for c in range(case[2])])).max() <= 1e-12
    # cosine: scikit-learn's own metric
    hc = silhouette_host(x, labels, "cosine")
    assert np.abs(hc.values - skm.silhouette_samples(x64, labels, metric="cosine")).max() <= 1e-12


@pytest.mark.parametrize("case", cases.SKLEARN_SHAPES, ids=cases.GAUSS_IDS[:3])
def test_agreement_host_equals_sklearn(case):
    skm = pytest.importorskip("sklearn.metrics")
    _, geo, rand = cases.gauss(*case)
    noisy = np.where(np.random.default_rng(1).random(geo.size) < 0.2, rand, geo)
    for a, b in ((geo, rand), (geo, noisy), (geo, geo), (noisy % 3, geo)):
        g = agreement_host(a, b)
        hcv = skm.homogeneity_completeness_v_measure(a, b)
        got = np.array([g.ari, g.nmi, g.homogeneity, g.completeness, g.v_measure])
        want = np.array([skm.adjusted_rand_score(a, b), skm.normalized_mutual_info_score(a, b), *hcv])
        assert np.abs(got - want).max() <= 1e-12, (got, want)
        assert g.contingency.sum() == a.size
        assert abs(g.purity - sum(np.bincount(a[b == k]).max() for k in np.unique(b)) / a.size) <= 1e-15


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------------
def test_two_clusters_on_a_line():
    x = np.array([[0.0], [1], [10], [12]])
    h = silhouette_host(x, [0, 0, 1, 1])
    np.testing.assert_array_equal(h.a, [1, 1, 2, 2])
    np.testing.assert_array_equal(h.b, [11, 10, 9.5, 11.5])
    np.testing.assert_array_equal(h.values, [10 / 11, 9 / 10, 7.5 / 9.5, 9.5 / 11.5])
    np.testing.assert_array_equal(h.nearest, [1, 1, 0, 0])
    assert h.mean == ordered_sum(h.values) / 4 and abs(h.mean - h.values.mean()) < 1e-15
    np.testing.assert_array_equal(h.cluster_mean, [(h.values[0] + h.values[1]) / 2, (h.values[2] + h.values[3]) / 2])
    d = dispersion_host(x, [0, 0, 1, 1])
    np.testing.assert_array_equal(d.counts, [2, 2])
    np.testing.assert_array_equal(d.means[:, 0], [0.5, 11])
    np.testing.assert_array_equal(d.within_sq, [0.5, 2])
    np.testing.assert_array_equal(d.within_dist, [1, 2])
    assert d.grand_mean[0] == 5.75
    # between = 2 (5.25^2 + 5.25^2), within = 2.5, n - k = 2, k - 1 = 1; DB: (0.5 + 1) / 10.5 for both clusters
    assert d.calinski_harabasz == 2 * 2 * 5.25 ** 2 * 2 / 2.5 and d.davies_bouldin == 1.5 / 10.5


def test_singleton_empty_cluster_tie_and_duplicates():
    x = np.array([[0.0, 0], [3, 4], [0, 10], [6, 8], [0, 0]])
    # a singleton (row 1): s = 0, a = 0, b still defined; cluster id 1 is empty and is skipped
    h = silhouette_host(x, [0, 2, 3, 3, 0], clusters=5)
    assert h.values[1] == 0 and h.a[1] == 0 and h.b[1] == 5 and h.nearest[1] == 0
    assert h.nearest[0] == 2 and h.b[0] == 5 and h.a[0] == 0 and h.values[0] == 1
    assert np.isnan(h.cluster_mean[1]) and np.isnan(h.cluster_mean[4]) and h.cluster_mean[2] == 0
    # an exact tie for nearest: row 0 is 5 away from clusters 1 and 2 alike -> the lowest id
    t = silhouette_host(np.array([[0.0, 0], [3, 4], [-3, -4], [0, 1]]), [0, 2, 1, 0])
    assert t.nearest[0] == 1 and t.b[0] == 5
    # duplicate rows: a = b = 0 -> s = 0
    dup = silhouette_host(np.ones((4, 3)), [0, 1, 0, 1])
    np.testing.assert_array_equal(dup.values, 0)
    np.testing.assert_array_equal(dup.a, 0)
    np.testing.assert_array_equal(dup.b, 0)
    np.testing.assert_array_equal(dup.nearest, [1, 0, 1, 0])
    # fewer than two non-empty clusters: s = 0, b = NaN, nearest = -1
    one = silhouette_host(x, [1] * 5, clusters=3)
    assert (one.values == 0).all() and np.isnan(one.b).all() and (one.nearest == -1).all() and one.mean == 0
    # a label outside [0, clusters): in no cluster, NaN, and out of the mean; a NaN row reaches every row
    bad = silhouette_host(x, [0, 2, 3, 3, -1], clusters=4)
    assert np.isnan(bad.values[4]) and bad.nearest[4] == -1 and np.isfinite(bad.mean) and bad.a[0] == 0 and bad.values[0] == 0
    xn = x.copy()
    xn[2, 0] = np.nan
    assert np.isnan(silhouette_host(xn, [0, 2, 3, 3, 0], clusters=4).values).all()
    # cosine: a zero row is at distance 1 from everything
    c = silhouette_host(np.array([[0.0, 0], [1, 0], [0, 2], [0, 3]]), [0, 0, 1, 1], "cosine")
    assert c.a[0] == 1 and c.b[0] == 1 and c.values[0] == 0 and c.a[2] == 0 and c.b[2] == 1
    # rows: a subset, unsorted, with a repeat
    sub = silhouette_host(x, [0, 2, 3, 3, 0], clusters=5, rows=[3, 0, 3])
    np.testing.assert_array_equal(sub.values, h.values[[3, 0, 3]])
    assert sub.mean == ordered_sum(h.values[[3, 0, 3]]) / 3


def test_ordered_sum_is_the_documented_order():
    v = np.random.default_rng(0).standard_normal(1000)
    part = [0.0] * 256
    for i, e in enumerate(v):
        part[i % 256] += e
    o = 128
    while o:
        for t in range(o):
            part[t] += part[t + o]
        o //= 2
    assert ordered_sum(v) == part[0] and ordered_sum([]) == 0.0 and ordered_sum([1.5]) == 1.5


def test_agreement_hand_worked():
    g = agreement_host([0, 0, 1, 1, 2, 2], [1, 1, 0, 0, 0, 2])
    np.testing.assert_array_equal(g.contingency, [[0, 2, 0], [2, 0, 0], [1, 0, 1]])
    assert g.purity == 5 / 6
    # pairs: 15 in all; together in both: 2; together in a only: 1; in b only: 2
    assert g.ari == 2.0 * (2 * 10 - 1 * 2) / ((2 + 1) * (1 + 10) + (2 + 2) * (2 + 10))
    same = agreement_host([3, 3, 5], [0, 0, 1])
    assert same.ari == 1 and abs(same.nmi - 1) < 1e-15 and same.purity == 1 and same.contingency.shape == (6, 2)
    assert agreement_host([0, 0], [0, 0]).nmi == 1
    with pytest.raises(ValueError, match="1-D"):
        agreement_host([0, 1], [0])


# ---- the kernel's walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.equal_cases(), ids=lambda c: c["name"])
def test_walk_equals_the_host_definition_on_integer_rows(case):
    """Partition order, ranges, 64 columns per step, flushes at the cluster boundaries: on rows whose distances and sums are
    exact the kernel's accumulation must give the host definition's sums, whatever the order."""
    h = silhouette_host(case["x"], case["labels"], "euclidean", case["K"], case["rows"])
    a, b, nearest, s = cases.walk_silhouette(case["x"], case["labels"], case["K"], case["rows"])
    np.testing.assert_array_equal(a, h.a)
    np.testing.assert_array_equal(b, h.b)
    np.testing.assert_array_equal(nearest, h.nearest)
    np.testing.assert_array_equal(s, h.values)
    d = case["x"].astype(np.float64)
    assert np.array_equal(np.sqrt(((d[:, None] - d[None]) ** 2).sum(-1)) % 5, np.zeros((d.shape[0],) * 2))


def test_geometry():
    assert cases.geometry(1, 1) == (1, 64) and cases.geometry(64, 64) == (1, 64) and cases.geometry(65, 65) == (2, 64)
    assert cases.geometry(300, 300) == (5, 64) and cases.geometry(20371, 20371) == (7, 2944)
    assert cases.geometry(100000, 10000) == (13, 7744) and cases.geometry(1 << 20, 1 << 20) == (1, 1 << 20)
    for n, m in ((257, 8), (2000, 2000), (20371, 20371), (99999, 5)):
        ns, length = cases.geometry(n, m)
        assert ns <= _ffi.CLUSTER_MAX_SPLITS and length % 64 == 0 and (ns - 1) * length < n <= ns * length


@pytest.mark.parametrize("case", cases.GAUSS, ids=cases.GAUSS_IDS)
def test_margins_leave_few_rows_exempt(case):
    """The premise of the GPU test: on these seeds the host margin between the two nearest clusters exceeds the summed rounding
    bounds on all but 2 % of the rows, so `nearest` is checked on the rest."""
    x, geo, rand = cases.gauss(*case)
    for labels in (geo, rand):
        rb = cases.row_bounds(x, labels, case[2])
        exempt = int((~rb["safe"]).sum())
        print("exempt rows: %d of %d" % (exempt, x.shape[0]))
        assert exempt <= 0.02 * x.shape[0]
        assert (rb["s_lo"] <= rb["host"].values).all() and (rb["host"].values <= rb["s_hi"]).all()


def test_fp32_formula_stays_inside_the_pair_bound():
    """The device's fp32 formula emulated in numpy (its own summation order): inside the bound, which does not depend on order."""
    worst = 0.0
    for case in cases.GAUSS:
        x = cases.gauss(*case)[0]
        d, bound = cases.pair_bound(x)
        xx = (x * x).sum(axis=1, dtype=np.float32)
        v = (xx[:, None] + xx[None, :]) + np.float32(-2.0) * (x @ x.T)
        dh = np.sqrt(np.maximum(v, np.float32(0.0))).astype(np.float64)
        np.fill_diagonal(dh, 0.0)
        off = ~np.eye(x.shape[0], dtype=bool)
        ratio = float((np.abs(dh - d)[off] / bound[off]).max())
        worst = max(worst, ratio)
    print("worst fp32 err / bound = %.3f" % worst)
    assert worst <= 1.0


# ---- the C ABI: host-only paths -----------------------------------------------------------------------------------------------------
def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _sil_rc(x=64, ld_x=None, rx=None, n=16, dim=8, metric=0, lab=64, K=4, rows=None, n_rows=0, a=64, b=64, near=64, s=64, cm=64, mean=64,
            st=64, ws=256, ws_bytes=1 << 40):
    return _ffi.lib().acx_silhouette(_p(x), dim if ld_x is None else ld_x, _p(rx), n, dim, metric, _p(lab), K, _p(rows), n_rows, _p(a),
                                     _p(b), _p(near), _p(s), _p(cm), _p(mean), _p(st), _p(ws), ws_bytes, None)


def _disp_rc(x=64, ld_x=None, n=16, dim=8, lab=64, K=4, cnt=64, means=64, wsq=64, wd=64, grand=64, st=64, ws=256, ws_bytes=1 << 40):
    return _ffi.lib().acx_cluster_dispersion(_p(x), dim if ld_x is None else ld_x, n, dim, _p(lab), K, _p(cnt), _p(means), _p(wsq),
                                             _p(wd), _p(grand), _p(st), _p(ws), ws_bytes, None)


def _cont_rc(a=64, ka=3, b=64, kb=5, n=16, table=64, st=64):
    return _ffi.lib().acx_contingency(_p(a), ka, _p(b), kb, n, _p(table), _p(st), None)


ROWS_BAD = (dict(x=None), dict(x=68), dict(n=0), dict(dim=6), dict(dim=0), dict(dim=_ffi.KNN_MAX_DIM + 4), dict(ld_x=4), dict(ld_x=10),
            dict(lab=None), dict(K=0), dict(K=_ffi.KMEANS_MAX_CLUSTERS + 1), dict(st=None), dict(ws=None))


def test_declarations_exported():
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    for name in NAMES:
        assert re.search(r"ACX_API int %s\(" % name, header), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert _ffi.SIGNATURES[name][0] is ctypes.c_int
    assert [len(_ffi.SIGNATURES[k][1]) for k in NAMES] == [4, 20, 15, 8]
    for name, value in (("NONFINITE", 1), ("DEGENERATE", 2), ("BAD_LABEL", 4), ("BAD_ROW", 8), ("MAX_SPLITS", 16)):
        assert re.search(r"#define ACX_CLUSTER_%s %d\b" % (name, value), header) and getattr(_ffi, "CLUSTER_" + name) == value
    assert _ffi.CONTINGENCY_MAX_CELLS == 1 << 24 and "#define ACX_CONTINGENCY_MAX_CELLS (1 << 24)" in header


def test_argument_errors_return_before_any_launch():
    lib = _ffi.lib()
    for kw in ROWS_BAD + (dict(metric=2), dict(metric=-1), dict(metric=1), dict(a=None), dict(b=None), dict(near=None), dict(s=None),
                          dict(mean=None), dict(rows=64, n_rows=0), dict(rows=64, n_rows=17)):
        assert _sil_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert b"clusters = 0" in (_sil_rc(K=0), lib.acx_last_error())[1]
    assert b"x_inv_norm" in (_sil_rc(metric=1), lib.acx_last_error())[1]
    assert b"n_rows = 17" in (_sil_rc(rows=64, n_rows=17), lib.acx_last_error())[1]
    assert _sil_rc(ws_bytes=0) == -5 and _sil_rc(ws=264) == -5 and _sil_rc(n=(1 << 30) + 1) == -6
    for kw in ROWS_BAD + (dict(cnt=None), dict(means=None), dict(wsq=None), dict(wd=None), dict(grand=None)):
        assert _disp_rc(**kw) == -1, kw
    assert _disp_rc(ws_bytes=0) == -5 and _disp_rc(ws=264) == -5 and _disp_rc(n=(1 << 30) + 1) == -6
    for kw in (dict(a=None), dict(b=None), dict(ka=0), dict(kb=0), dict(n=0), dict(table=None), dict(table=68), dict(st=None)):
        assert _cont_rc(**kw) == -1, kw
    assert _cont_rc(ka=4097, kb=4096) == -6 and _cont_rc(n=(1 << 30) + 1) == -6
    assert b"2^24" in lib.acx_last_error() or b"2^30" in lib.acx_last_error()


def test_workspace_bytes_non_decreasing():
    size = ctypes.c_size_t()
    lib = _ffi.lib()
    assert lib.acx_cluster_scores_workspace_bytes(16, 8, 4, None) == -1
    for n, dim, K in ((0, 8, 4), (16, 6, 4), (16, 0, 4), (16, 8, 0), (16, 8, _ffi.KMEANS_MAX_CLUSTERS + 1), (16, _ffi.KNN_MAX_DIM + 4, 4)):
        assert lib.acx_cluster_scores_workspace_bytes(n, dim, K, ctypes.byref(size)) == -1, (n, dim, K)
    assert lib.acx_cluster_scores_workspace_bytes((1 << 30) + 1, 8, 4, ctypes.byref(size)) == -6
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 20371, 200000, 1048576, 1048577, 1 << 30]
    dims = [4, 8, 20, 768, 772, 4096]
    ks = [1, 2, 50, 256, 257, 4096]
    grid = np.array([[[_ffi.cluster_scores_workspace_bytes(a, b, c) for c in ks] for b in dims] for a in ns], dtype=np.float64)
    assert (grid > 0).all() and (grid % 256 == 0).all()
    for axis in range(3):
        assert (np.diff(grid, axis=axis) >= 0).all(), axis
    # (clusters + 16) float64 per row, far below the n x n distances (20 371^2 float64 = 3.3 GB)
    assert _ffi.cluster_scores_workspace_bytes(20371, 768, 50) < 16 << 20


# ---- the Python API: errors raised before any device call ---------------------------------------------------------------------------
def test_python_value_errors_need_no_device():
    e = np.zeros((5, 8), np.float32)
    lab = np.zeros(5, np.int64)
    with pytest.raises(ValueError, match="2-D"):
        cs.silhouette(np.zeros(8, np.float32), lab)
    with pytest.raises(ValueError, match="metric"):
        cs.silhouette(e, lab, metric="l1")
    with pytest.raises(ValueError, match="shape"):
        cs.silhouette(e, lab[:4])
    with pytest.raises(ValueError, match="sample = 6"):
        cs.silhouette(e, lab, sample=6)
    with pytest.raises(ValueError, match="sample = 0"):
        cs.silhouette(e, lab, sample=0)
    with pytest.raises(ValueError, match="clusters = 0"):
        cs.silhouette(e, lab, clusters=0)
    with pytest.raises(ValueError, match="not cpu"):
        cs.silhouette(e, lab, clusters=2, device="cpu")
    with pytest.raises(ValueError, match="shape"):
        cs.dispersion_scores(e, lab[:3])
    with pytest.raises(ValueError, match="not cpu"):
        cs.dispersion_scores(e, lab, clusters=2, device="cpu")
    with pytest.raises(ValueError, match="1-D"):
        cs.agreement(np.zeros((2, 2), np.int64), lab)
    with pytest.raises(ValueError, match="not cpu"):
        cs.agreement(lab, lab, 1, 1, device="cpu")
    with pytest.raises(ValueError, match="metric"):
        cs.select_clusters(e, (2, 3), metric="l1")
    with pytest.raises(ValueError, match="not cpu"):
        cs.select_clusters(e, (2, 3), device="cpu")
    with pytest.raises(ValueError, match="criterion"):
        cs._select(None, None, (2, 3), "gap")
    with pytest.raises(ValueError, match="ks"):
        cs._select(None, None, (1, 3), "silhouette")
    with pytest.raises(ValueError, match="metric"):
        silhouette_host(e, lab, "l1")
    assert cs.MAX_CLUSTERS == _ffi.KMEANS_MAX_CLUSTERS and cs.CRITERIA[0] == "silhouette"
