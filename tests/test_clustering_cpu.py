"""CPU: k-means over embeddings (pytorch/clustering.py, acx_kmeans_* in include/acx.h) -- the numpy host definitions against
scikit-learn and hand-worked cases, the argument errors and the workspace size of the C ABI (host-only paths), and the ValueErrors
of the Python API that need no device."""
import ctypes

import numpy as np
import pytest

import clustering_cases as cc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import clustering
from audioset_convnext_inf_amd.pytorch.clustering import assign_host, kmeans_host, sample_host, seed_host


# ---- kmeans_host against scikit-learn -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.TRAJECTORIES, ids=lambda c: "n%d-d%d-k%d" % c[:3])
def test_kmeans_host_equals_sklearn(case):
    sk = pytest.importorskip("sklearn.cluster")
    x, c0 = cc.case_input(*case)
    K = case[2]
    ref = sk.KMeans(K, init=np.asarray(c0, np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=100).fit(np.asarray(x, np.float64))
    # without the fp32 rounding of the centres: the same algorithm in the same precision
    plain = kmeans_host(x, c0, "euclidean", 100, 0.0, round_centers=False)
    np.testing.assert_array_equal(plain.labels, ref.labels_)
    assert np.abs(plain.centers - ref.cluster_centers_).max() <= 3e-15
    assert plain.n_iter == ref.n_iter_ and plain.converged
    # the host definition proper rounds the centres as the device stores them
    got = cc.trajectory(case)
    assert got.centers.dtype == np.float32 and got.converged and (got.counts > 0).all()
    np.testing.assert_array_equal(got.labels, ref.labels_)
    np.testing.assert_array_equal(got.counts, np.bincount(ref.labels_, minlength=K))
    assert (np.abs(got.centers.astype(np.float64) - ref.cluster_centers_) <= np.spacing(np.abs(got.centers)).astype(np.float64)).all()
    assert abs(got.inertia - ref.inertia_) <= 1e-6 * ref.inertia_


@pytest.mark.parametrize("case", cc.TRAJECTORIES, ids=lambda c: "n%d-d%d-k%d" % c[:3])
def test_trajectory_margins_exceed_the_rounding_bound(case):
    """The premise of the GPU trajectory test: at every iteration each row's float64 gap to the runner-up exceeds 2 max_k b_ik."""
    x, c0 = cc.case_input(*case)
    worst = np.inf
    for it in range(cc.trajectory(case).n_iter + 1):
        c = c0 if it == 0 else kmeans_host(x, c0, "euclidean", it, 0.0).centers
        _, gap, b = cc.margins(x, c)
        worst = min(worst, float((gap / (2 * b)).min()))
    print("min gap / (2 max b) = %.2f" % worst)
    assert worst > 1.0, worst


def test_kmeans_host_stops_and_keeps_empty_clusters():
    x = np.array([[0.0, 0], [0, 1], [10, 0], [10, 1]], np.float32)
    far = np.array([[0.0, 0.5], [10, 0.5], [100, 100]], np.float32)
    r = kmeans_host(x, far)
    np.testing.assert_array_equal(r.labels, [0, 0, 1, 1])
    np.testing.assert_array_equal(r.counts, [2, 2, 0])
    np.testing.assert_array_equal(r.centers[2], far[2])                 # the empty cluster keeps its centre
    assert r.converged and r.inertia == 1.0
    one = kmeans_host(x, np.array([[0.0, 0], [1, 0]], np.float32), max_iter=1)
    assert one.n_iter == 1 and not one.converged
    np.testing.assert_array_equal(one.labels, assign_host(x, one.centers)[0])
    loose = kmeans_host(x, np.array([[0.0, 0], [1, 0]], np.float32), tol_abs=1e9)
    assert loose.n_iter == 1 and loose.converged
    # cosine: unit centres, labels by direction
    r = kmeans_host(np.array([[1.0, 0], [5, 0.1], [0, 2], [0.1, 7]], np.float32), np.array([[1.0, 1], [0, 1]], np.float32), "cosine")
    np.testing.assert_array_equal(r.labels, [0, 0, 1, 1])
    np.testing.assert_allclose(np.linalg.norm(r.centers.astype(np.float64), axis=1), 1.0, atol=2.0 ** -23)


def test_assign_host_ties_go_to_the_lowest_index():
    x = np.array([[1.0, 2], [3, 4]])
    c = np.array([[3.0, 4], [1, 2], [1, 2], [3, 4]])
    lab, s = assign_host(x, c)
    np.testing.assert_array_equal(lab, [1, 0])
    np.testing.assert_array_equal(s, [-5.0, -25.0])
    lab, _ = assign_host(np.array([[0.0, 0]]), np.array([[-0.0, 0], [0.0, 0]]), "cosine")       # -0.0 ties with +0.0
    assert lab[0] == 0


# ---- sample_host ----------------------------------------------------------------------------------------------------------------
def test_sample_host_hand_worked():
    assert sample_host(np.zeros(7, np.float32), 0.4) == -1
    d = np.array([0, 0, 3, 0], np.float32)
    for u in (0.0, 0.5, 1 - 2.0 ** -53):
        assert sample_host(d, u) == 2
    d = np.ones(4, np.float32)                                              # ties: equal shares, boundaries go up
    assert [sample_host(d, u) for u in (0.0, 0.24999, 0.25, 0.5, 0.75, 1 - 2.0 ** -53)] == [0, 0, 1, 2, 3, 3]
    d = np.array([1, 0, 0, 1], np.float32)                                  # zero weights are never picked
    assert [sample_host(d, u) for u in (0.0, 0.49999, 0.5, 1 - 2.0 ** -53)] == [0, 0, 3, 3]
    d = np.array([1e-30, 1.0, 1e-30], np.float32)                           # the small entries quantise to 0
    assert [sample_host(d, u) for u in (0.0, 1 - 2.0 ** -53)] == [1, 1]
    # q = floor(d 2^(30 - e)): d = (3, 1) -> q = (3 * 2^29, 2^29), the boundary is u = 3/4 exactly
    d = np.array([3, 1], np.float32)
    assert [sample_host(d, u) for u in (0.75 - 2.0 ** -53, 0.75)] == [0, 1]
    with pytest.raises(ValueError, match="1-D"):
        sample_host(np.zeros((2, 2)), 0.1)


def test_sample_host_frequencies():
    rng = np.random.default_rng(0)
    d = (rng.random(1000) ** 2).astype(np.float32)
    p = d.astype(np.float64) / d.astype(np.float64).sum()
    draws = 200000
    # the quantised weights and their prefix sums once; every draw is then sample_host's own last two lines
    e = int(np.frexp(d.max())[1]) - 1
    c = np.cumsum(np.floor(np.ldexp(d, 30 - e)).astype(np.uint64), dtype=np.uint64)
    total = int(c[-1])
    u = rng.random(draws)
    t = np.minimum(np.floor(u * np.float64(total)).astype(np.uint64), np.uint64(total - 1))
    picks = np.searchsorted(c, t, side="right")
    for j in range(0, draws, 20000):
        assert picks[j] == sample_host(d, u[j])
    freq = np.bincount(picks, minlength=1000) / draws
    # a binomial share has standard deviation sqrt(p (1 - p) / draws) <= sqrt(max p / draws): five of them over 1000 weights
    assert np.abs(freq - p).max() <= 5 * np.sqrt(p.max() / draws)


# ---- seed_host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_seed_host(metric):
    x, _ = cc.blobs(400, 16, 6, 2.0, 11)
    u = np.random.default_rng(5).random(9)
    p, deg = seed_host(x, 8, u, metric)
    assert p.shape == (8,) and p.dtype == np.int64 and len(set(p.tolist())) == 8 and not deg
    assert p[0] == int(u[0] * 400)
    q, _ = seed_host(x, 8, u, metric)
    np.testing.assert_array_equal(p, q)
    r, _ = seed_host(x, 8, np.random.default_rng(6).random(9), metric)
    assert not np.array_equal(p, r)
    # three distinct rows, five clusters: the rounds that run dry take the lowest free index
    # (norms that are powers of two: a row's cosine with itself is exactly 1)
    tri = np.array([[1.0, 0], [0, 1], [-2, 0]], np.float32)[np.arange(12) % 3]
    p, deg = seed_host(tri, 5, u, metric)
    assert deg and len(set(p.tolist())) == 5
    assert len({tuple(tri[i]) for i in p[:3]}) == 3
    with pytest.raises(ValueError, match="uniforms"):
        seed_host(x, 8, u[:7], metric)


# ---- the C ABI: host-only paths -------------------------------------------------------------------------------------------------
def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _assign_rc(x=64, ld_x=None, rx=None, n=16, c=128, ld_c=None, K=4, dim=8, metric=0, prev=None, lab=64, sc=64, ch=64, st=64):
    return _ffi.lib().acx_kmeans_assign(_p(x), dim if ld_x is None else ld_x, _p(rx), n, _p(c), dim if ld_c is None else ld_c, K, dim,
                                        metric, _p(prev), _p(lab), _p(sc), _p(ch), _p(st), None)


def _update_rc(x=64, ld_x=None, rx=None, n=16, dim=8, metric=0, lab=64, K=4, c=128, ld_c=None, cnt=64, sh=64, st=64, ws=256,
               ws_bytes=1 << 30):
    return _ffi.lib().acx_kmeans_update(_p(x), dim if ld_x is None else ld_x, _p(rx), n, dim, metric, _p(lab), K, _p(c),
                                        dim if ld_c is None else ld_c, _p(cnt), _p(sh), _p(st), _p(ws), ws_bytes, None)


def _fit_rc(x=64, ld_x=None, rx=None, n=16, dim=8, metric=0, c=128, ld_c=None, K=4, max_iter=3, tol=64, lab=64, cnt=64, state=64,
            st=64, ws=256, ws_bytes=1 << 30):
    return _ffi.lib().acx_kmeans_fit(_p(x), dim if ld_x is None else ld_x, _p(rx), n, dim, metric, _p(c), dim if ld_c is None else ld_c,
                                     K, max_iter, _p(tol), _p(lab), _p(cnt), _p(state), _p(st), _p(ws), ws_bytes, None)


def _mind_rc(x=64, ld_x=None, rx=None, n=16, dim=8, metric=0, c=128, first=1, d=64, dmax=64, st=64):
    return _ffi.lib().acx_kmeans_min_distance(_p(x), dim if ld_x is None else ld_x, _p(rx), n, dim, metric, _p(c), first, _p(d),
                                              _p(dmax), _p(st), None)


def _sample_rc(d=64, n=16, dmax=64, u=64, picked=64, st=64, ws=256, ws_bytes=1 << 20):
    return _ffi.lib().acx_kmeans_sample(_p(d), n, _p(dmax), _p(u), _p(picked), _p(st), _p(ws), ws_bytes, None)


def _seed_rc(x=64, ld_x=None, rx=None, n=16, dim=8, metric=0, K=4, u=64, picked=64, c=128, ld_c=None, st=64, ws=256, ws_bytes=1 << 30):
    return _ffi.lib().acx_kmeans_seed(_p(x), dim if ld_x is None else ld_x, _p(rx), n, dim, metric, K, _p(u), _p(picked), _p(c),
                                      dim if ld_c is None else ld_c, _p(st), _p(ws), ws_bytes, None)


ROWS_BAD = (dict(x=None), dict(x=68), dict(n=0), dict(dim=6), dict(dim=0), dict(dim=_ffi.KNN_MAX_DIM + 4), dict(ld_x=4), dict(ld_x=10),
            dict(metric=2), dict(metric=-1), dict(metric=1), dict(st=None))
CENTRES_BAD = (dict(c=None), dict(c=72), dict(ld_c=4), dict(ld_c=10), dict(K=0), dict(K=_ffi.KMEANS_MAX_CLUSTERS + 1))


def test_declarations_exported():
    lib = _ffi.lib()
    for name in ("acx_kmeans_workspace_bytes", "acx_kmeans_assign", "acx_kmeans_update", "acx_kmeans_fit", "acx_kmeans_min_distance",
                 "acx_kmeans_sample", "acx_kmeans_seed"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert _ffi.SIGNATURES[name][0] is ctypes.c_int
    assert len(_ffi.SIGNATURES["acx_kmeans_assign"][1]) == 15 and len(_ffi.SIGNATURES["acx_kmeans_fit"][1]) == 18
    assert _ffi.KMEANS_STATE_BYTES == 32 and _ffi.KMEANS_MAX_CLUSTERS == 4096
    assert _ffi.KMEANS_METRICS == {"euclidean": 0, "cosine": 1}


def test_argument_errors_return_before_any_launch():
    lib = _ffi.lib()
    for kw in ROWS_BAD + CENTRES_BAD + (dict(lab=None), dict(sc=None), dict(ch=None)):
        assert _assign_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert _assign_rc(n=(1 << 30) + 1) == -6
    assert b"clusters = 0" in (_assign_rc(K=0), lib.acx_last_error())[1]
    for kw in ROWS_BAD + CENTRES_BAD + (dict(lab=None), dict(cnt=None), dict(sh=None), dict(ws=None)):
        assert _update_rc(**kw) == -1, kw
    assert _update_rc(ws_bytes=0) == -5 and _update_rc(ws=264) == -5 and _update_rc(n=(1 << 30) + 1) == -6
    for kw in ROWS_BAD + CENTRES_BAD + (dict(K=17), dict(max_iter=0), dict(max_iter=_ffi.KMEANS_MAX_ITER + 1), dict(tol=None),
                                        dict(lab=None), dict(cnt=None), dict(state=None), dict(state=68), dict(ws=None)):
        assert _fit_rc(**kw) == -1, kw
    assert _fit_rc(ws_bytes=0) == -5 and _fit_rc(ws=264) == -5 and _fit_rc(n=(1 << 30) + 1) == -6
    for kw in ROWS_BAD + (dict(c=None), dict(c=72), dict(d=None), dict(dmax=None)):
        assert _mind_rc(**kw) == -1, kw
    for kw in (dict(d=None), dict(n=0), dict(dmax=None), dict(u=None), dict(u=68), dict(picked=None), dict(st=None), dict(ws=None)):
        assert _sample_rc(**kw) == -1, kw
    assert _sample_rc(ws_bytes=_ffi.KMEANS_SAMPLE_WORKSPACE - 1) == -5 and _sample_rc(ws=264) == -5
    assert _sample_rc(n=(1 << 30) + 1) == -6
    for kw in ROWS_BAD + CENTRES_BAD + (dict(K=17), dict(u=None), dict(u=68), dict(picked=None), dict(ws=None)):
        assert _seed_rc(**kw) == -1, kw
    assert _seed_rc(ws_bytes=0) == -5 and _seed_rc(ws=264) == -5


def test_workspace_bytes_non_decreasing():
    size = ctypes.c_size_t()
    lib = _ffi.lib()
    assert lib.acx_kmeans_workspace_bytes(16, 8, 4, None) == -1
    for n, dim, K in ((0, 8, 4), (16, 6, 4), (16, 0, 4), (16, 8, 0), (16, 8, _ffi.KMEANS_MAX_CLUSTERS + 1), (16, _ffi.KNN_MAX_DIM + 4, 4)):
        assert lib.acx_kmeans_workspace_bytes(n, dim, K, ctypes.byref(size)) == -1, (n, dim, K)
    assert lib.acx_kmeans_workspace_bytes((1 << 30) + 1, 8, 4, ctypes.byref(size)) == -6
    ns = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 20371, 200000, 1048576, 1048577, 1 << 30]
    dims = [4, 8, 20, 768, 772, 4096]
    ks = [1, 2, 50, 256, 257, 4096]
    grid = np.array([[[_ffi.kmeans_workspace_bytes(a, b, c) for c in ks] for b in dims] for a in ns], dtype=np.float64)
    assert (grid > 0).all() and (grid % 256 == 0).all()
    for axis in range(3):
        assert (np.diff(grid, axis=axis) >= 0).all(), axis
    # far below the n x K score matrix the stock form writes (200 000 x 4 096 fp32 = 3.3 GB)
    assert _ffi.kmeans_workspace_bytes(200000, 768, 4096) < 64 << 20
    assert _ffi.KMEANS_SAMPLE_WORKSPACE <= _ffi.kmeans_workspace_bytes(1, 4, 1)


# ---- the Python API: errors raised before any device call ------------------------------------------------------------------------
def test_python_value_errors_need_no_device():
    e = np.zeros((5, 8), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        clustering.kmeans(np.zeros(8, np.float32), 2)
    with pytest.raises(ValueError, match="metric"):
        clustering.kmeans(e, 2, metric="l1")
    with pytest.raises(ValueError, match="clusters = 0"):
        clustering.kmeans(e, 0)
    with pytest.raises(ValueError, match="clusters = 6"):
        clustering.kmeans(e, 6)
    with pytest.raises(ValueError, match="clusters"):
        clustering.kmeans(e, _ffi.KMEANS_MAX_CLUSTERS + 1)
    with pytest.raises(ValueError, match="clusters"):
        clustering.kmeans(e, 2.5)
    with pytest.raises(ValueError, match="max_iter"):
        clustering.kmeans(e, 2, max_iter=0)
    with pytest.raises(ValueError, match="n_init"):
        clustering.kmeans(e, 2, n_init=0)
    with pytest.raises(ValueError, match="tol"):
        clustering.kmeans(e, 2, tol=-1.0)
    with pytest.raises(ValueError, match="init"):
        clustering.kmeans(e, 2, init="kmeans||")
    with pytest.raises(ValueError, match="init has shape"):
        clustering.kmeans(e, 2, init=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="not cpu"):
        clustering.kmeans(e, 2, device="cpu")
    with pytest.raises(ValueError, match="metric"):
        kmeans_host(e, e[:2], "l1")
    with pytest.raises(ValueError, match="dim"):
        assign_host(e, np.zeros((2, 4)))
    with pytest.raises(ValueError, match="clusters = 6"):
        seed_host(e, 6, np.zeros(7))
    assert clustering.MAX_CLUSTERS == _ffi.KMEANS_MAX_CLUSTERS
