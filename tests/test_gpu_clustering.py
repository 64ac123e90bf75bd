"""GPU: k-means over embeddings (pytorch/clustering.py, acx_kmeans_* in include/acx.h, csrc/kmeans.hip) against the numpy
float64 host definitions: (1) exact one-step assignment on integer inputs, (2) rounded assignment under the derived fp32 bound,
(3) the deterministic centre update, (4) whole trajectories, (5) k-means++ seeding, (6) the Python surface.  Shapes sit at the
tile and tail boundaries of the kernels (64-row tiles, 64 centres per wave, 256 per step, dim % 16), not at workload size."""
import warnings

import numpy as np
import pytest
import torch

import clustering_cases as cc
from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import clustering, retrieval
from audioset_convnext_inf_amd.pytorch.clustering import KMeans, assign_host, kmeans, kmeans_host, sample_host, seed_host
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev_rows(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def dev_assign(x, c, metric="euclidean", prev=None):
    """acx_kmeans_assign on device tensors -> (labels, scores, changed, status) as numpy / ints."""
    n, K = x.shape[0], c.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    scores = torch.empty(n, dtype=torch.float32, device=DEV)
    words = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    rx = retrieval.row_norms(x) if metric == "cosine" else None
    _ffi.kmeans_assign(vp(x), x.stride(0), vp(rx), n, vp(c), c.stride(0), K, x.shape[1], _ffi.KMEANS_METRICS[metric], vp(prev),
                       vp(labels), vp(scores), vp(words[1:]), vp(words), _ffi.stream_ptr(x.device))
    w = words.cpu().numpy()
    return labels.cpu().numpy(), scores.cpu().numpy(), int(w[1]), int(w[0])


# ---- (1) exact one-step assignment ---------------------------------------------------------------------------------------------
def exact_case(n, K, dim, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    if kind == "random":
        c = rng.integers(-8, 9, (K, dim)).astype(np.float32)
    elif kind == "identical":
        c = np.tile(rng.integers(-8, 9, (1, dim)).astype(np.float32), (K, 1))
    elif kind == "duplicated":
        base = rng.integers(-8, 9, (max(1, (K + 2) // 3), dim)).astype(np.float32)
        c = base[np.arange(K) % base.shape[0]]
    else:                                                  # rows equal to centres
        c = x[np.arange(K) % n]
    return x, c


EXACT = [(n, K, 768) for n in (1, 63, 64, 65, 257) for K in (1, 2, 63, 64, 65, 257, 4096)] + [(65, 65, d) for d in (4, 20, 772)]


@pytest.mark.parametrize("n,K,dim", EXACT)
def test_exact_assignment_equals_the_host(n, K, dim):
    """Entries -8 .. 8: every product, sum and the fma are exact in fp32 in any order, so labels and scores are EQUAL."""
    for metric in ("euclidean", "cosine"):
        for j, kind in enumerate(("random", "identical", "duplicated", "rows")):
            x, c = exact_case(n, K, dim, kind, 1000 * n + K + j)
            want_l, want_s = assign_host(x, c, metric)
            lab, sc, changed, status = dev_assign(dev_rows(x), dev_rows(c), metric)
            assert status == 0 and changed == n
            np.testing.assert_array_equal(lab, want_l, err_msg="%s %s" % (metric, kind))
            np.testing.assert_array_equal(sc.astype(np.float64), want_s, err_msg="%s %s" % (metric, kind))
            assert not np.signbit(sc[sc == 0]).any()
            if kind == "identical":
                assert (lab == 0).all()
            if kind == "duplicated":
                assert lab.max() < max(1, (K + 2) // 3)


def test_changed_counts_rows_that_moved():
    x, c = exact_case(257, 65, 20, "random", 3)
    xd, cd = dev_rows(x), dev_rows(c)
    lab, _, _, _ = dev_assign(xd, cd)
    prev = lab.copy()
    prev[[0, 63, 64, 200, 256]] += 1
    _, _, changed, _ = dev_assign(xd, cd, prev=torch.from_numpy(prev).to(DEV))
    assert changed == 5
    _, _, changed, _ = dev_assign(xd, cd, prev=torch.from_numpy(lab).to(DEV))
    assert changed == 0


# ---- (2) rounded one-step assignment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("case", cc.ROUNDED, ids=lambda c: "n%d-d%d-k%d" % c[:3])
def test_rounded_assignment_is_valid_under_the_fp32_bound(case, metric):
    x, c0 = cc.case_input(*case, "rand")
    xd = dev_rows(x)
    for it in range(3):
        c = c0 if it == 0 else cc.trajectory(case, metric, it).centers
        if it == 0 and metric == "cosine":                 # the unit rows the fit starts from
            c = (c0 / np.linalg.norm(c0.astype(np.float64), axis=1)[:, None]).astype(np.float32)
        s64 = cc.score_matrix(x, c, metric)
        b = cc.score_bound(x, c, metric)
        lab, sc, _, status = dev_assign(xd, dev_rows(c), metric)
        assert status == 0 and lab.min() >= 0 and lab.max() < c.shape[0]
        rows = np.arange(x.shape[0])
        # valid: no centre is better than the chosen one by more than the two rounding errors
        assert (s64[rows, lab] - b[rows, lab] <= (s64 + b).min(axis=1)).all()
        host, gap, bmax = cc.margins(x, c, metric)
        decided = gap > 2 * bmax
        exempt = 1.0 - decided.mean()
        print("%s it %d: %.2f %% of the rows exempt from equality" % (metric, it, 100 * exempt))
        assert exempt <= 0.02
        np.testing.assert_array_equal(lab[decided], host[decided])
        assert (np.abs(sc.astype(np.float64) - s64[rows, lab]) <= b[rows, lab]).all()


def test_score_bits_do_not_depend_on_the_shape():
    """A (row, centre) pair has the same score bits whatever n, K and its place in the tiles: one centre alone against rows in
    other positions gives the bits of the full call."""
    x, c0 = cc.case_input(*cc.ROUNDED[2], "rand")
    xd, cd = dev_rows(x), dev_rows(c0)
    lab, sc, _, _ = dev_assign(xd, cd)
    for k in (0, 17, 32):
        rows = np.nonzero(lab == k)[0]
        assert rows.size
        sub = dev_rows(x[rows[::-1]])
        l1, s1, _, _ = dev_assign(sub, dev_rows(c0[k:k + 1]))
        assert (l1 == 0).all()
        np.testing.assert_array_equal(s1.view(np.uint32), sc[rows[::-1]].view(np.uint32))


@pytest.mark.parametrize("dim", [4, 8, 12, 16, 20, 24, 28, 772])
def test_dot_products_are_the_search_s(dim):
    """kmeans_assign_kernel and knn_search_kernel form a (row, centre) dot product by ONE function (dot_tile, device_common.h).
    The cosine assignment scores a row as minus its largest raw dot product with a centre, and a k = 1 "dot" search over the
    centres returns that largest dot product: labels = indices and scores = -scores, no tolerance, on normal float32 data whose
    bits show the summation order.  dim: rem 4 / 8 / 12 / 0 of the 16-column groups without and with full groups; n: the search
    takes 32-query and 64-query tiles while the assignment always takes 64 rows; K: one centre, a partial second wave, a second
    step.  (Values are compared, not bit patterns: the search returns +0.0 where the assignment returns 0 - (+0.0).)"""
    rng = np.random.default_rng(7700 + dim)
    for n in (31, 65):
        for K in (1, 65, 257):
            xd = dev_rows(rng.standard_normal((n, dim)))
            cd = dev_rows(rng.standard_normal((K, dim)))
            lab, sc, _, status = dev_assign(xd, cd, "cosine")
            index = retrieval.EmbeddingIndex(cd, metric="dot")
            s, i = index.search(xd, k=1)
            assert status == 0 and int(index._status.cpu()[0]) == 0, (n, K)
            np.testing.assert_array_equal(lab, i.cpu().numpy()[:, 0], err_msg="n %d K %d" % (n, K))
            np.testing.assert_array_equal(sc, -s.cpu().numpy()[:, 0], err_msg="n %d K %d" % (n, K))


# ---- (3) the centre update -------------------------------------------------------------------------------------------------------
def dev_update(x, labels, c_old, metric="euclidean"):
    n, dim = x.shape
    K = c_old.shape[0]
    c = c_old.clone()
    counts = torch.empty(K, dtype=torch.int32, device=DEV)
    shift = torch.empty(1, dtype=torch.float64, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    ws_bytes = _ffi.kmeans_workspace_bytes(n, dim, K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    rx = retrieval.row_norms(x) if metric == "cosine" else None
    _ffi.kmeans_update(vp(x), x.stride(0), vp(rx), n, dim, _ffi.KMEANS_METRICS[metric], vp(labels), K, vp(c), c.stride(0), vp(counts),
                       vp(shift), vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(x.device))
    return c.cpu().numpy(), counts.cpu().numpy(), float(shift.cpu()[0]), int(status.cpu()[0]), rx


@pytest.mark.parametrize("n,dim,K", [(1, 4, 1), (1000, 20, 7), (2500, 772, 65), (70000, 8, 300)])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_update(n, dim, K, metric):
    rng = np.random.default_rng(n + K)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    labels = rng.integers(0, K, n)
    empty = K // 2 if K > 1 else None
    if empty is not None:
        labels[labels == empty] = 0                        # one empty cluster
    old = rng.standard_normal((K, dim)).astype(np.float32)
    xd, od = dev_rows(x), dev_rows(old)
    ld = torch.from_numpy(labels.astype(np.int32)).to(DEV)
    c, counts, shift, status, rx = dev_update(xd, ld, od, metric)
    assert status == 0
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=K))
    x64 = x.astype(np.float64)
    w = rx.cpu().numpy().astype(np.float64) if metric == "cosine" else np.ones(n)
    for k in range(K):
        rows = labels == k
        if not rows.any():
            np.testing.assert_array_equal(c[k].view(np.uint32), old[k].view(np.uint32))      # kept bit for bit
            continue
        xs = x64[rows] * w[rows, None]
        s = xs.sum(axis=0)
        # float64 summation of count terms: error <= count 2^-53 sum |x| <= n 2^-53 sum |x|; then one rounding to fp32
        serr = n * 2.0 ** -53 * np.abs(xs).sum(axis=0)
        if metric == "cosine":
            nrm = np.sqrt((s * s).sum())
            want, tol = s / nrm, 2.0 ** -24 * np.abs(s / nrm) + 2 * serr / nrm + 2.0 ** -50
            assert abs(np.sqrt((c[k].astype(np.float64) ** 2).sum()) - 1.0) <= 2.0 ** -23
        else:
            want, tol = s / rows.sum(), 2.0 ** -24 * np.abs(s / rows.sum()) + serr / rows.sum()
        assert (np.abs(c[k].astype(np.float64) - want) <= tol).all(), k
    moved = [k for k in range(K) if (labels == k).any()]
    want_shift = ((c[moved].astype(np.float64) - old[moved].astype(np.float64)) ** 2).sum()
    assert abs(shift - want_shift) <= 1e-12 * want_shift
    # the same bits on a second run, and under a renumbering of the clusters
    c2, counts2, shift2, _, _ = dev_update(xd, ld, od, metric)
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32)) and shift == shift2 and np.array_equal(counts, counts2)
    perm = rng.permutation(K)                              # cluster k becomes perm[k]
    inv = np.argsort(perm)
    c3, counts3, _, _, _ = dev_update(xd, torch.from_numpy(perm[labels].astype(np.int32)).to(DEV), dev_rows(old[inv]), metric)
    np.testing.assert_array_equal(c3[perm].view(np.uint32), c.view(np.uint32))
    np.testing.assert_array_equal(counts3[perm], counts)


def test_update_reports_labels_out_of_range():
    x = dev_rows(np.ones((10, 4)))
    lab = torch.tensor([0, 1, 2, -1, 3, 0, 1, 2, 0, 0], dtype=torch.int32, device=DEV)
    c, counts, _, status, _ = dev_update(x, lab, dev_rows(np.zeros((3, 4))))
    assert status == _ffi.KMEANS_BAD_LABEL
    np.testing.assert_array_equal(counts, [4, 2, 2])


# ---- (4) trajectories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.TRAJECTORIES, ids=lambda c: "n%d-d%d-k%d" % c[:3])
def test_trajectory_equals_the_host(case):
    x, c0 = cc.case_input(*case)
    want = cc.trajectory(case)
    km = kmeans(dev_rows(x), case[2], init=c0, tol=0.0).check()
    np.testing.assert_array_equal(km.labels.cpu().numpy(), want.labels)
    np.testing.assert_array_equal(km.counts.cpu().numpy(), want.counts)
    assert int(km.n_iter) == want.n_iter and bool(km.converged)
    assert km.labels.dtype == torch.int64 and km.counts.dtype == torch.int64 and km.centers.dtype == torch.float32
    c = km.centers.cpu().numpy()
    assert (np.abs(c.astype(np.float64) - want.centers.astype(np.float64)) <= np.spacing(np.abs(want.centers)).astype(np.float64)).all()
    b = cc.score_bound(x, want.centers)[np.arange(x.shape[0]), want.labels]
    print("inertia: device %.9g host %.9g bound %.3g" % (float(km.inertia), want.inertia, b.sum()))
    assert abs(float(km.inertia) - want.inertia) <= b.sum()
    # one iteration only: not converged, and the labels belong to the returned centres
    one = kmeans(dev_rows(x), case[2], init=c0, tol=0.0, max_iter=1).check()
    assert int(one.n_iter) == 1 and not bool(one.converged)
    np.testing.assert_array_equal(one.labels.cpu().numpy(), assign_host(x, one.centers.cpu().numpy())[0])
    np.testing.assert_array_equal(one.counts.cpu().numpy(), np.bincount(one.labels.cpu().numpy(), minlength=case[2]))


def test_tolerance_stops_early():
    case = cc.TRAJECTORIES[1]
    x, c0 = cc.case_input(*case)
    full = cc.trajectory(case)
    tol_abs = 1e-4 * float(np.var(x.astype(np.float64), axis=0).mean())
    want = kmeans_host(x, c0, "euclidean", 100, tol_abs)
    km = kmeans(dev_rows(x), case[2], init=c0, tol=1e-4).check()
    assert int(km.n_iter) == want.n_iter <= full.n_iter and bool(km.converged)
    np.testing.assert_array_equal(km.labels.cpu().numpy(), want.labels)


# ---- (5) seeding -----------------------------------------------------------------------------------------------------------------
def dev_sample(d, u):
    dd = torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(DEV)
    dmax = dd.max().reshape(1).clone()
    ud = torch.tensor([u], dtype=torch.float64, device=DEV)
    out = torch.full((2,), -9, dtype=torch.int32, device=DEV)
    ws = torch.empty(_ffi.KMEANS_SAMPLE_WORKSPACE, dtype=torch.uint8, device=DEV)
    _ffi.kmeans_sample(vp(dd), dd.shape[0], vp(dmax), vp(ud), vp(out), vp(out[1:]), (vp(ws), ws.numel()), _ffi.stream_ptr(dd.device))
    o = out.cpu().numpy()
    return int(o[0]), int(o[1])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_sample_equals_the_host(n):
    rng = np.random.default_rng(n)
    arrays = {"uniform": rng.random(n).astype(np.float32),
              "wide": (10.0 ** rng.uniform(-30, 5, n)).astype(np.float32),          # the small entries quantise to 0
              "sparse": np.where(rng.random(n) < 0.9, 0, rng.random(n)).astype(np.float32)}
    arrays["sparse"][n // 2] = 0.5
    for name, d in arrays.items():
        for u in (0.0, 0.5, 1 - 2.0 ** -53) + tuple(rng.random(3)):
            got, status = dev_sample(d, u)
            assert (got, status) == (sample_host(d, u), 0), (name, u)
    assert dev_sample(np.zeros(n, np.float32), 0.3) == (-1, _ffi.KMEANS_DEGENERATE)


def dev_min_distance(x, rx, c, first, d, metric):
    dmax = torch.empty(1, dtype=torch.float32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    _ffi.kmeans_min_distance(vp(x), x.stride(0), vp(rx), x.shape[0], x.shape[1], _ffi.KMEANS_METRICS[metric], vp(c), first, vp(d),
                             vp(dmax), vp(status), _ffi.stream_ptr(x.device))
    return dmax, status


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("n,dim", [(1, 4), (257, 20), (1100, 772)])
def test_min_distance(n, dim, metric):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    xd = dev_rows(x)
    rx = retrieval.row_norms(xd) if metric == "cosine" else None
    d = torch.empty(n, dtype=torch.float32, device=DEV)
    x64 = x.astype(np.float64)
    want = None
    for r, i in enumerate((0, n // 2, n - 1)):
        dmax, status = dev_min_distance(xd, rx, xd[i], r == 0, d, metric)
        new = clustering._distance_host(x64, x64[i], metric)
        want = new if want is None else np.minimum(want, new)
        got = d.cpu().numpy().astype(np.float64)
        assert int(status) == 0 and float(dmax) == got.max()
        if metric == "euclidean":
            # (x - c) rounds once, its square once, and a chain of at most dim additions: (dim + 8) 2^-24 relative
            tol = (dim + 8) * 2.0 ** -24 * want
        else:
            # cos is a dot product of unit-length operands (error (dim + 8) 2^-24) times two rounded inverse norms and two
            # products (5 roundings); 2 - 2 cos doubles the absolute error
            tol = np.full(n, 2 * (dim + 8 + 5) * 2.0 ** -24)
        assert (np.abs(got - want) <= tol).all()


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_seeding(metric):
    x, _ = cc.blobs(3000, 20, 12, 2.0, 9)
    K = 33
    xd = dev_rows(x)

    def run(seed):
        km_u = np.random.default_rng(seed).random(K + 1)
        rx = retrieval.row_norms(xd) if metric == "cosine" else None
        u = torch.from_numpy(km_u).to(DEV)
        picked = torch.empty(K, dtype=torch.int32, device=DEV)
        centers = torch.empty((K, 20), dtype=torch.float32, device=DEV)
        status = torch.empty(1, dtype=torch.int32, device=DEV)
        ws_bytes = _ffi.kmeans_workspace_bytes(3000, 20, K)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        _ffi.kmeans_seed(vp(xd), xd.stride(0), vp(rx), 3000, 20, _ffi.KMEANS_METRICS[metric], K, vp(u), vp(picked), vp(centers),
                         centers.stride(0), vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(xd.device))
        return km_u, rx, picked.cpu().numpy(), centers.cpu().numpy(), int(status.cpu()[0])

    u, rx, picked, centers, status = run(4)
    assert status == 0 and len(set(picked.tolist())) == K and picked.min() >= 0 and picked.max() < 3000
    _, _, again, _, _ = run(4)
    np.testing.assert_array_equal(picked, again)
    assert not np.array_equal(picked, run(5)[2])
    rows = x[picked] if metric == "euclidean" else (xd[torch.from_numpy(picked).to(DEV).long()] * rx[torch.from_numpy(picked).to(DEV).long(), None]).cpu().numpy()
    np.testing.assert_array_equal(centers, rows)
    # the host definition, fed the device's own distance arrays round by round, picks the same rows
    d = torch.empty(3000, dtype=torch.float32, device=DEV)

    def d_round(r, so_far):
        dev_min_distance(xd, rx, xd[so_far[-1]], r == 1, d, metric)
        return d.cpu().numpy()

    want, deg = seed_host(x, K, u, metric, d_rounds=d_round)
    assert not deg
    np.testing.assert_array_equal(picked, want)


def test_degenerate_seeding():
    tri = np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [-2, 0, 0, 0]], np.float32)[np.arange(12) % 3]
    for metric in ("euclidean", "cosine"):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            km = kmeans(dev_rows(tri), 5, metric=metric, seed=1, max_iter=2).check()
        assert any(issubclass(w.category, RuntimeWarning) for w in caught)
        assert int(km._status) & _ffi.KMEANS_DEGENERATE
    # through the C call: five distinct row indices, the first three of distinct rows
    xd = dev_rows(tri)
    u = torch.from_numpy(np.random.default_rng(1).random(6)).to(DEV)
    picked = torch.empty(5, dtype=torch.int32, device=DEV)
    centers = torch.empty((5, 4), dtype=torch.float32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    ws_bytes = _ffi.kmeans_workspace_bytes(12, 4, 5)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _ffi.kmeans_seed(vp(xd), 4, None, 12, 4, 0, 5, vp(u), vp(picked), vp(centers), 4, vp(status), (vp(ws), ws_bytes),
                     _ffi.stream_ptr(xd.device))
    p = picked.cpu().numpy()
    assert int(status.cpu()[0]) == _ffi.KMEANS_DEGENERATE and len(set(p.tolist())) == 5
    assert len({tuple(tri[i]) for i in p[:3]}) == 3
    want, deg = seed_host(tri, 5, u.cpu().numpy())
    assert deg
    np.testing.assert_array_equal(p, want)


# ---- (6) the surface -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    x, _ = cc.blobs(1500, 24, 6, 3.0, 21)
    xd = dev_rows(x)
    return x, xd, kmeans(xd, 6, seed=3).check()


def test_predict_distances_save_load(fitted, tmp_path):
    x, xd, km = fitted
    assert torch.equal(km.predict(xd), km.labels)
    assert torch.equal(km.predict(x), km.labels)                           # host rows travel to the device
    d = km.distances(xd).cpu().numpy().astype(np.float64)
    c = km.centers.cpu().numpy().astype(np.float64)
    want = ((x.astype(np.float64) - c[km.labels.cpu().numpy()]) ** 2).sum(axis=1)
    assert (np.abs(d - want) <= 2 * cc.score_bound(x, c).max(axis=1) + 1e-5 * want).all()
    assert abs(float(km.inertia) - want.sum()) <= 1e-5 * want.sum()
    assert int(km.counts.sum()) == 1500 and bool(km.converged)
    km.save(tmp_path / "km.npz")
    back = KMeans.load(tmp_path / "km.npz")
    for name in ("centers", "labels", "counts", "inertia", "n_iter", "converged"):
        assert torch.equal(getattr(back, name), getattr(km, name)), name
    assert back.metric == km.metric and torch.equal(back.predict(xd), km.labels)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_n_init_keeps_the_lowest_inertia(metric):
    x, _ = cc.blobs(900, 12, 9, 1.5, 33)
    xd = dev_rows(x)
    singles = [kmeans(xd, 9, metric=metric, init="random", seed=5 + j, max_iter=30) for j in range(3)]
    best = min(singles, key=lambda k: float(k.inertia))
    km = kmeans(xd, 9, metric=metric, init="random", n_init=3, seed=5, max_iter=30).check()
    assert float(km.inertia) == min(float(k.inertia) for k in singles)
    assert torch.equal(km.centers, best.centers) and torch.equal(km.labels, best.labels) and torch.equal(km.counts, best.counts)
    assert int(km.n_iter) == int(best.n_iter)


@pytest.mark.parametrize("metric,dim", [("cosine", 24), ("dot", 24), ("cosine", 22)])
def test_index_cluster_equals_kmeans(metric, dim):
    x, _ = cc.blobs(800, dim, 5, 2.0, 8)
    idx = retrieval.EmbeddingIndex(dev_rows(x), metric=metric)
    a = idx.cluster(5, seed=2).check()
    b = kmeans(dev_rows(x), 5, metric="cosine" if metric == "cosine" else "euclidean", seed=2).check()
    assert a.metric == b.metric and a.centers.shape == (5, dim)
    for name in ("centers", "labels", "counts", "inertia", "n_iter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    with pytest.raises(ValueError, match="clusters"):
        idx.cluster(801)


@pytest.fixture(scope="module")
def model(synth_sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    return m.to("cuda").eval()


def test_cluster_through_the_model(model):
    clips = [w for w in synth.synth_waveforms(8, 32000, seed=51).cuda()]
    a = model.cluster(clips, 3, seed=1).check()
    emb = torch.stack(extract(model, clips, what="scene", pack=True)).cuda()
    b = kmeans(emb, 3, seed=1).check()
    for name in ("centers", "labels", "counts", "inertia", "n_iter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.centers.shape == (3, 768) and torch.equal(model.cluster(emb, 3, seed=1).labels, b.labels)


def test_nonfinite_rows_are_reported():
    clean, _ = cc.blobs(300, 16, 4, 2.0, 5)
    x = clean.copy()
    x[77, 3] = np.nan
    for metric in ("euclidean", "cosine"):
        km = kmeans(dev_rows(x), 4, metric=metric, init=clean[:4])
        assert (km.labels == -1).all() and not bool(km.converged)
        with pytest.raises(ValueError, match="NaN or infinite"):
            km.check()


def test_whole_fit_in_a_graph():
    x, _ = cc.blobs(700, 20, 5, 2.0, 13)
    y, _ = cc.blobs(700, 20, 5, 2.0, 14)
    buf = dev_rows(x)
    c0 = dev_rows(x[:5])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kmeans(buf, 5, init=c0, max_iter=20)                      # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = kmeans(buf, 5, init=c0, max_iter=20)
    buf.copy_(dev_rows(y))
    g.replay()
    torch.cuda.synchronize()
    eager = kmeans(dev_rows(y), 5, init=c0, max_iter=20).check()
    for name in ("centers", "labels", "counts", "inertia", "n_iter", "converged"):
        assert torch.equal(getattr(out, name), getattr(eager, name)), name
    assert int(eager.n_iter) >= 2


def test_column_slices_are_read_in_place():
    x, _ = cc.blobs(500, 24, 4, 2.0, 17)
    wide = torch.zeros((500, 40), dtype=torch.float32, device=DEV)
    wide[:, 8:32] = dev_rows(x)
    view = wide[:, 8:32]
    assert retrieval._rows(view, view.device).data_ptr() == view.data_ptr()
    a = kmeans(view, 4, seed=6).check()
    b = kmeans(dev_rows(x), 4, seed=6).check()
    for name in ("centers", "labels", "counts", "inertia", "n_iter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.predict(view), a.labels)
