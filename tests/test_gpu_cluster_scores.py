"""GPU: cluster validation (pytorch/cluster_scores.py; acx_silhouette, acx_cluster_dispersion, acx_contingency in include/acx.h;
csrc/cluster_scores.hip) against the numpy host definitions: with `==` on integer rows whose every distance, sum and quotient
operand is exact, inside the rounding bound of the fp32 pair distance on Gaussian rows, bit for bit between runs and under a
captured graph, and by results and flags on bad data."""
import numpy as np
import pytest
import torch

import cluster_scores_cases as cases
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import cluster_scores as cs
from audioset_convnext_inf_amd.pytorch import retrieval
from audioset_convnext_inf_amd.pytorch.clustering import kmeans
from audioset_convnext_inf_amd.pytorch.cluster_scores import (agreement, agreement_host, dispersion_host, dispersion_scores,
                                                              select_clusters, silhouette, silhouette_host)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def run_silhouette(x, labels, K, rows=None, ld=None, metric="euclidean"):
    """acx_silhouette through the raw binding (row stride and row list as given) -> (dict of numpy arrays, status)."""
    n, dim = x.shape
    dp = (dim + 3) // 4 * 4                                                        # zero columns up to a multiple of 4
    buf = torch.zeros((n, ld or dp), dtype=torch.float32, device=DEV)
    buf[:, :dim] = dev(x)
    xv = buf[:, :dp]
    lab = dev(labels, torch.int32)
    r = None if rows is None else dev(rows, torch.int32)
    m = n if rows is None else len(rows)
    out = torch.full((3, m), 7.0, dtype=torch.float64, device=DEV)
    near = torch.full((m,), 7, dtype=torch.int32, device=DEV)
    means = torch.full((K + 1,), 7.0, dtype=torch.float64, device=DEV)
    st = torch.full((1,), 255, dtype=torch.int32, device=DEV)
    rx = retrieval.row_norms(xv) if metric == "cosine" else None
    nb = _ffi.cluster_scores_workspace_bytes(n, dp, K)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _ffi.silhouette(vp(xv), xv.stride(0), vp(rx), n, dp, _ffi.KMEANS_METRICS[metric], vp(lab), K, vp(r), m, vp(out[0]), vp(out[1]),
                    vp(near), vp(out[2]), vp(means), vp(means[K:]), vp(st), (vp(ws), nb), _ffi.stream_ptr(torch.device(DEV)))
    o = out.cpu().numpy()
    return dict(a=o[0], b=o[1], s=o[2], nearest=near.cpu().numpy(), cluster_mean=means[:K].cpu().numpy(),
                mean=float(means[K].cpu())), int(st.cpu()[0])


def assert_equals_host(got, h):
    np.testing.assert_array_equal(got["a"], h.a)
    np.testing.assert_array_equal(got["b"], h.b)
    np.testing.assert_array_equal(got["nearest"], h.nearest)
    np.testing.assert_array_equal(got["s"], h.values)
    np.testing.assert_array_equal(got["cluster_mean"], h.cluster_mean)
    np.testing.assert_array_equal(got["mean"], h.mean)


# ---- EQUAL: integer rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.equal_cases(), ids=lambda c: c["name"])
def test_integer_rows_equal_the_host_definitions(case):
    x, labels, K = case["x"], case["labels"], case["K"]
    got, st = run_silhouette(x, labels, K, case["rows"], case["ld"])
    h = silhouette_host(x, labels, "euclidean", K, case["rows"])
    assert_equals_host(got, h)
    few = np.unique(labels).size < 2
    assert st == (_ffi.CLUSTER_DEGENERATE if few else 0)
    # the dispersion: counts, means, within_sq (and the rest) with ==
    d = dispersion_scores(dev(x), dev(labels), K)
    hd = dispersion_host(x, labels, K)
    np.testing.assert_array_equal(d.counts.cpu().numpy(), hd.counts)
    np.testing.assert_array_equal(d.means.cpu().numpy(), hd.means)
    np.testing.assert_array_equal(d.within.cpu().numpy(), hd.within_sq)
    np.testing.assert_array_equal(d.within_dist.cpu().numpy(), hd.within_dist)
    np.testing.assert_array_equal(d.grand_mean.cpu().numpy(), hd.grand_mean)
    np.testing.assert_array_equal([d.calinski_harabasz, d.davies_bouldin], [hd.calinski_harabasz, hd.davies_bouldin])
    assert int(d._status.cpu()[0]) == (_ffi.CLUSTER_DEGENERATE if few else 0)


def test_cosine_is_exact_on_rows_of_equal_norm():
    x = cases.cosine_rows(300, 21)
    assert (np.linalg.norm(x, axis=1) == 0).sum() >= 3
    labels = np.random.default_rng(22).integers(0, 6, size=300)
    got, st = run_silhouette(x, labels, 7, metric="cosine")
    h = silhouette_host(x, labels, "cosine", 7)
    assert_equals_host(got, h)
    assert st == 0 and np.isnan(h.cluster_mean[6])
    zero = np.flatnonzero(np.linalg.norm(x, axis=1) == 0)[0]                       # rx = 0: d = 1 to every other row
    assert got["a"][zero] == 1.0 and got["b"][zero] == 1.0 and got["s"][zero] == 0.0
    sil = silhouette(dev(x), dev(labels), "cosine", clusters=7).check()
    np.testing.assert_array_equal(sil.values.cpu().numpy(), h.values)


# ---- rounded: Gaussian rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["geometric", "random"])
@pytest.mark.parametrize("case", cases.GAUSS, ids=cases.GAUSS_IDS)
def test_gaussian_rows_stay_inside_the_rounding_bound(case, which):
    x, geo, rand = cases.gauss(*case)
    labels = geo if which == "geometric" else rand
    K = case[2]
    rb = cases.row_bounds(x, labels, K)
    h = rb["host"]
    got, st = run_silhouette(x, labels, K)
    assert st == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ra = np.nanmax(np.where(rb["ea"] > 0, np.abs(got["a"] - h.a) / rb["ea"], 0.0))
        rbb = np.nanmax(np.abs(got["b"] - h.b) / rb["eb"])
    print("worst |a - host| / bound = %.3f, |b - host| / bound = %.3f, max |s - host| = %.2e" % (ra, rbb, np.abs(got["s"] - h.values).max()))
    assert (np.abs(got["a"] - h.a) <= rb["ea"]).all()
    assert (np.abs(got["b"] - h.b) <= rb["eb"]).all()
    tiny = 4 * np.finfo(np.float64).eps
    assert (got["s"] >= rb["s_lo"] - tiny).all() and (got["s"] <= rb["s_hi"] + tiny).all()
    safe = rb["safe"]
    assert (~safe).sum() <= 0.02 * x.shape[0]
    np.testing.assert_array_equal(got["nearest"][safe], h.nearest[safe])
    # the means follow from the rows' own values in the documented order
    assert got["mean"] == cs.ordered_sum(got["s"]) / x.shape[0]
    for c in range(K):
        assert got["cluster_mean"][c] == cs.ordered_sum(np.where(labels == c, got["s"], 0.0)) / (labels == c).sum()


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_runs_and_graph_replays_give_the_same_bits():
    x, geo, _ = cases.gauss(*cases.GAUSS[1])
    buf, lab = dev(x), dev(geo)
    fields = ("values", "a", "b", "nearest", "mean", "cluster_mean")
    first = silhouette(buf, lab, clusters=7)
    again = silhouette(buf, lab, clusters=7)
    for name in fields:
        assert torch.equal(getattr(first, name), getattr(again, name)), name
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        silhouette(buf, lab, clusters=7)                                           # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = silhouette(buf, lab, clusters=7)
    y, geo2, _ = cases.gauss(300, 20, 7, 2.0, 1.0, 44)
    buf.copy_(dev(y))
    lab.copy_(dev(geo2))
    g.replay()
    torch.cuda.synchronize()
    eager = silhouette(dev(y), dev(geo2), clusters=7).check()
    for name in fields:
        assert torch.equal(getattr(out, name), getattr(eager, name)), name
    assert not torch.equal(eager.values, first.values)


# ---- status -------------------------------------------------------------------------------------------------------------------------
def test_bad_data_is_reported_by_results_and_flags():
    x, geo, _ = cases.gauss(*cases.GAUSS[2])
    n, K = x.shape[0], 4
    for bad_value in (np.nan, np.inf):
        xb = x.copy()
        xb[40, 1] = bad_value
        got, st = run_silhouette(xb, geo, K)
        assert st == _ffi.CLUSTER_NONFINITE
        assert np.isnan(got["s"]).all() and np.isnan(got["a"]).all() and (got["nearest"] == -1).all() and np.isnan(got["mean"])
        with pytest.raises(ValueError, match="NaN or infinite"):
            silhouette(dev(xb), dev(geo), clusters=K).check()
        with pytest.raises(ValueError, match="NaN or infinite"):
            dispersion_scores(dev(xb), dev(geo), K).check()
    # a label of -1 and of `clusters`: the row is in no cluster -- NaN, out of the mean -- and the others do not see it.  Integer rows:
    # the host definition holds with ==
    xi = cases.integer_rows(np.random.default_rng(31).integers(-50, 51, size=n), 8)
    for bad_label in (-1, K):
        lab = geo.copy()
        lab[[5, 77]] = bad_label
        got, st = run_silhouette(xi, lab, K)
        assert st == _ffi.CLUSTER_BAD_LABEL
        assert np.isnan(got["s"][[5, 77]]).all() and (got["nearest"][[5, 77]] == -1).all() and np.isfinite(got["mean"])
        assert_equals_host(got, silhouette_host(xi, lab, "euclidean", K))
        with pytest.raises(ValueError, match="outside"):
            silhouette(dev(xi), dev(lab), clusters=K).check()
        d = dispersion_scores(dev(xi), dev(lab), K)
        np.testing.assert_array_equal(d.counts.cpu().numpy(), dispersion_host(xi, lab, K).counts)
        with pytest.raises(ValueError, match="outside"):
            d.check()
    # a single non-empty cluster: every s = 0
    got, st = run_silhouette(x, np.full(n, 2), K)
    assert st == _ffi.CLUSTER_DEGENERATE and (got["s"] == 0).all() and got["mean"] == 0 and np.isnan(got["b"]).all()
    assert (got["nearest"] == -1).all() and np.isnan(got["cluster_mean"][[0, 1, 3]]).all() and got["cluster_mean"][2] == 0
    with pytest.raises(ValueError, match="fewer than two"):
        silhouette(dev(x), dev(np.full(n, 2)), clusters=K).check()
    # a row index outside [0, n)
    got, st = run_silhouette(x, geo, K, rows=np.array([3, n, 9, -1]))
    assert st == _ffi.CLUSTER_BAD_ROW and np.isnan(got["s"][[1, 3]]).all() and np.isfinite(got["s"][[0, 2]]).all()


# ---- contingency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka,kb", [(1, 1), (3, 5), (527, 50), (4096, 4096)])
def test_contingency_equals_the_counts(ka, kb):
    rng = np.random.default_rng(ka + kb)
    n = 20000
    a, b = rng.integers(0, ka, size=n), rng.integers(0, kb, size=n)
    want = np.zeros((ka, kb), dtype=np.int64)
    np.add.at(want, (a, b), 1)
    ag = agreement(dev(a), dev(b), ka, kb)
    assert ag.contingency.dtype == torch.int64 and torch.equal(ag.contingency.cpu(), torch.from_numpy(want))
    if ka * kb < 1 << 20:
        h = agreement_host(a, b, ka, kb)
        assert ag[1:] == h[1:]
    # a pair with either label out of range is counted nowhere and flagged
    a2 = a.copy()
    a2[7], a2[9] = ka, -1
    table = torch.empty((ka, kb), dtype=torch.int64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    da, db = dev(a2, torch.int32), dev(b, torch.int32)
    _ffi.contingency(vp(da), ka, vp(db), kb, n, vp(table), vp(st), _ffi.stream_ptr(torch.device(DEV)))
    want[a[7], b[7]] -= 1
    want[a[9], b[9]] -= 1
    assert int(st.cpu()[0]) == _ffi.CLUSTER_BAD_LABEL and torch.equal(table.cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match="outside"):
        agreement(dev(a2), dev(b), ka, kb)


# ---- the Python-level scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.SKLEARN_SHAPES, ids=cases.GAUSS_IDS[:3])
def test_agreement_and_dispersion_scores(case):
    skm = pytest.importorskip("sklearn.metrics")
    x, geo, rand = cases.gauss(*case)
    noisy = np.where(np.random.default_rng(1).random(geo.size) < 0.2, rand, geo)
    ag = agreement(dev(geo), dev(noisy))
    hcv = skm.homogeneity_completeness_v_measure(geo, noisy)
    got = np.array([ag.ari, ag.nmi, ag.homogeneity, ag.completeness, ag.v_measure])
    want = np.array([skm.adjusted_rand_score(geo, noisy), skm.normalized_mutual_info_score(geo, noisy), *hcv])
    assert np.abs(got - want).max() <= 1e-12
    assert ag.purity == agreement_host(geo, noisy).purity
    for labels in (geo, rand):
        d = dispersion_scores(dev(x), dev(labels)).check()
        h = dispersion_host(x, labels)
        e = (abs(d.calinski_harabasz - h.calinski_harabasz), abs(d.davies_bouldin - h.davies_bouldin))
        print("calinski-harabasz %.2e, davies-bouldin %.2e" % e)
        assert max(e) <= 1e-12
        assert np.abs(d.means.cpu().numpy() - h.means).max() <= 1e-12
        assert np.abs(d.within.cpu().numpy() / h.within_sq - 1).max() <= 1e-12


def test_select_clusters_finds_the_planted_blobs():
    rng = np.random.default_rng(8)
    centres = np.array([[0.0] * 16, [8.0] * 16, [-8.0] * 8 + [8.0] * 8])
    x = dev((centres[np.arange(240) % 3] + rng.standard_normal((240, 16))).astype(np.float32))
    sel = select_clusters(x, (2, 3, 4, 6), seed=3)
    assert sel.best_k == 3 and sel.ks == (2, 3, 4, 6) and sel.best is sel.fits[1] and sel.scores.dtype == torch.float64
    for k, km, score in zip(sel.ks, sel.fits, sel.scores):
        assert km.centers.shape[0] == k
        assert torch.equal(silhouette(x, km.labels, clusters=k).check().mean, score)
        assert torch.equal(km.silhouette(x).mean, score)
    assert float(sel.scores[1]) > 0.6
    # the other criteria, a sample, and the wrappers
    assert select_clusters(x, (2, 3, 4, 6), criterion="calinski_harabasz", seed=3).best_k == 3
    assert select_clusters(x, (2, 3, 4, 6), criterion="davies_bouldin", seed=3).best_k == 3
    smp = select_clusters(x, (2, 3, 4), sample=100, seed=3)
    part = silhouette(x, smp.fits[1].labels, clusters=3, sample=100, seed=3)
    assert smp.best_k == 3 and torch.equal(part.mean, smp.scores[1]) and part.rows.shape == (100,)
    full = silhouette(x, smp.fits[1].labels, clusters=3)
    # (100 and 240 queried rows both fit one row group: the same ranges, so the same bits)
    assert torch.equal(part.values, full.values[part.rows]) and len(set(part.rows.tolist())) == 100
    index = retrieval.EmbeddingIndex(x, metric="dot")
    both = index.cluster_scores(sel.best)
    assert torch.equal(both.silhouette.values, silhouette(x, sel.best.labels, clusters=3).values)
    assert torch.equal(both.silhouette.mean, sel.scores[1])
    assert both.dispersion.calinski_harabasz == dispersion_scores(x, sel.best.labels, 3).calinski_harabasz
