"""CPU: nearest-neighbour search over embeddings (pytorch/retrieval.py, acx_knn_* in include/acx.h) -- the numpy host
equivalents against an independent brute force, the argument errors and the workspace size of the C ABI (host-only paths), and
the ValueErrors of the Python API that need no device."""
import ctypes

import numpy as np
import pytest

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import retrieval
from audioset_convnext_inf_amd.pytorch.retrieval import search_host, vote_host


def brute(q, d, k, metric, exclude=None):
    """A Python sort per query with the key (-score, index); scores by explicit float64 loops over numpy rows."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    out_s, out_i = [], []
    for i, qi in enumerate(q):
        rows = []
        for j, dj in enumerate(d):
            if exclude is not None and exclude[i] == j:
                continue
            s = float(np.dot(qi, dj))
            if metric == "cosine":
                nq, nd = np.sqrt(np.dot(qi, qi)), np.sqrt(np.dot(dj, dj))
                s = s * (1.0 / nq if nq > 0 else 0.0) * (1.0 / nd if nd > 0 else 0.0)
            rows.append((-(s + 0.0), j))
        rows.sort()
        out_s.append([-r[0] for r in rows[:k]])
        out_i.append([r[1] for r in rows[:k]])
    return np.array(out_s), np.array(out_i)


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("k", [1, 5, 23])
def test_search_host_matches_brute_force(metric, k):
    rng = np.random.default_rng(k)
    q = rng.standard_normal((7, 12))
    d = rng.standard_normal((23, 12))
    s, i = search_host(q, d, k, metric)
    bs, bi = brute(q, d, k, metric)
    assert i.dtype == np.int64 and i.shape == (7, k)
    np.testing.assert_array_equal(i, bi)
    np.testing.assert_allclose(s, bs, rtol=0, atol=1e-12)


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_search_host_ties_and_exclude(metric):
    rng = np.random.default_rng(3)
    base = rng.integers(-3, 4, size=(4, 8)).astype(np.float64)
    d = base[np.arange(20) % 4]                      # four distinct rows, five times each: ties everywhere
    q = np.concatenate([base[:3], rng.integers(-3, 4, size=(2, 8)).astype(np.float64)])
    for k in (1, 6, 19):
        ex = np.array([0, 5, -1, 19, 2])
        s, i = search_host(q, d, k, metric, exclude=ex)
        bs, bi = brute(q, d, k, metric, exclude=ex)
        np.testing.assert_array_equal(i, bi)
        np.testing.assert_allclose(s, bs, rtol=0, atol=1e-12)
        for r in range(5):
            assert ex[r] not in i[r]
    # all rows equal: the answer is the first k indices
    same = np.tile(base[:1], (9, 1))
    _, i = search_host(base[:2], same, 9, metric)
    np.testing.assert_array_equal(i, np.tile(np.arange(9), (2, 1)))


def test_search_host_zero_row_and_negative_zero():
    d = np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0]])
    s, i = search_host(np.array([[1.0, 0.0], [0.0, 0.0]]), d, 3, "cosine")
    np.testing.assert_array_equal(i, [[1, 0, 2], [0, 1, 2]])
    np.testing.assert_array_equal(s, [[1.0, 0.0, -1.0], [0.0, 0.0, 0.0]])
    assert not np.signbit(s).any() or (s[np.signbit(s)] != 0).all()      # no -0.0 among the scores
    # -0.0 ties with +0.0: the index decides
    s, i = search_host(np.array([[1.0, 0.0]]), np.array([[-0.0, 1.0], [0.0, 1.0]]), 2, "dot")
    np.testing.assert_array_equal(i, [[0, 1]])


def test_vote_host():
    rng = np.random.default_rng(0)
    y = (rng.random((30, 6)) < 0.3).astype(np.uint8)
    idx = np.stack([rng.permutation(30)[:5] for _ in range(4)])
    sc = -np.sort(-rng.random((4, 5)), axis=1)
    np.testing.assert_array_equal(vote_host(idx, None, y), np.stack([y[r].sum(0) / 5.0 for r in idx]))
    for T in (0.07, 1.0):
        got = vote_host(idx, sc, y, "similarity", T)
        for r in range(4):
            w = np.exp((sc[r] - sc[r, 0]) / T)
            w = w / w.sum()
            np.testing.assert_allclose(got[r], (w[:, None] * y[idx[r]]).sum(0), rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match="weights"):
        vote_host(idx, sc, y, "nearest")
    with pytest.raises(ValueError, match="temperature"):
        vote_host(idx, sc, y, "similarity", 0.0)


# ---- the C ABI: host-only paths ------------------------------------------------------------------------------------------------
def _search_rc(nq=4, n=16, k=2, dim=8, ld_q=None, ld_d=None, metric=0, q=64, d=64, rq=None, rd=None, exclude=None, ind=64, sc=64,
               st=64, ws=256, ws_bytes=1 << 30):
    """acx_knn_search with made-up (never dereferenced) pointers: argument errors return before anything is launched."""
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return _ffi.lib().acx_knn_search(p(q), dim if ld_q is None else ld_q, p(rq), nq, p(d), dim if ld_d is None else ld_d, p(rd), n,
                                     dim, metric, k, p(exclude), p(ind), p(sc), p(st), p(ws), ws_bytes, None)


def test_search_argument_errors():
    bad = dict(k=0), dict(k=_ffi.KNN_MAX_K + 1), dict(k=17), dict(k=16, exclude=64), dict(nq=0), dict(n=0), dict(dim=6), \
        dict(dim=0), dict(dim=_ffi.KNN_MAX_DIM + 4), dict(ld_q=4), dict(ld_d=10), dict(ld_d=4), dict(q=None), dict(d=None), \
        dict(ind=None), dict(sc=None), dict(st=None), dict(ws=None), dict(metric=2), dict(metric=1), dict(metric=1, rq=64), \
        dict(q=68), dict(d=72)
    for kw in bad:
        assert _search_rc(**kw) == -1, kw
        assert _ffi.lib().acx_last_error()
    assert _search_rc(ws_bytes=0) == -5
    assert _search_rc(ws=264) == -5
    assert _search_rc(n=(1 << 30) + 1) == -6
    assert b"k = 17" in (_search_rc(k=17), _ffi.lib().acx_last_error())[1]


def test_norms_and_vote_argument_errors():
    lib = _ffi.lib()
    p = ctypes.c_void_p
    assert lib.acx_knn_row_norms(None, 8, 4, 8, p(64), p(64), None) == -1
    assert lib.acx_knn_row_norms(p(64), 8, 0, 8, p(64), p(64), None) == -1
    assert lib.acx_knn_row_norms(p(64), 8, 4, 7, p(64), p(64), None) == -1
    assert lib.acx_knn_row_norms(p(64), 6, 4, 4, p(64), p(64), None) == -1
    assert lib.acx_knn_row_norms(p(64), 8, 4, 8, None, p(64), None) == -1
    assert lib.acx_knn_row_norms(p(64), 8, 4, 8, p(64), None, None) == -1

    def vote(idx=64, sc=64, nq=2, k=3, tgt=64, dt=1, ld_t=5, n=9, C=5, w=0, T=0.07, out=64, ld_o=5, st=64):
        q = lambda v: None if v is None else p(v)
        return lib.acx_knn_vote(q(idx), q(sc), nq, k, q(tgt), dt, ld_t, n, C, w, T, q(out), ld_o, q(st), None)
    for kw in (dict(idx=None), dict(tgt=None), dict(out=None), dict(st=None), dict(k=0), dict(k=_ffi.KNN_MAX_K + 1), dict(nq=0),
               dict(n=0), dict(C=0), dict(ld_t=4), dict(ld_o=4), dict(dt=2), dict(w=2), dict(w=1, sc=None), dict(w=1, T=0.0),
               dict(w=1, T=-1.0)):
        assert vote(**kw) == -1, kw


def test_workspace_bytes_non_decreasing():
    n = ctypes.c_size_t()
    lib = _ffi.lib()
    assert lib.acx_knn_workspace_bytes(4, 16, 2, None) == -1
    assert lib.acx_knn_workspace_bytes(0, 16, 2, ctypes.byref(n)) == -1
    assert lib.acx_knn_workspace_bytes(4, 0, 2, ctypes.byref(n)) == -1
    assert lib.acx_knn_workspace_bytes(4, 16, 0, ctypes.byref(n)) == -1
    assert lib.acx_knn_workspace_bytes(4, 16, _ffi.KNN_MAX_K + 1, ctypes.byref(n)) == -1
    assert lib.acx_knn_workspace_bytes(4, (1 << 30) + 1, 2, ctypes.byref(n)) == -6
    qs = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 4096, 4097, 20371, 100000, 1 << 20]
    ns = [1, 2, 255, 256, 257, 1000, 4097, 20371, 300001, 1000000, 1 << 30]
    ks = [1, 2, 10, 32, 33, 64, 65, 128]
    grid = np.array([[[_ffi.knn_workspace_bytes(a, b, c) for c in ks] for b in ns] for a in qs], dtype=np.float64)
    assert (grid > 0).all() and (grid % 256 == 0).all()
    for axis in range(3):
        assert (np.diff(grid, axis=axis) >= 0).all(), axis
    # every (query, slice) owns k keys of 8 bytes
    for a, b, c in ((1, 1, 1), (5, 1000, 10), (64, 4097, 128), (3, 300001, 5), (20371, 20371, 10), (64, 1000000, 10)):
        assert _ffi.knn_workspace_bytes(a, b, c) >= a * _ffi.knn_slices(a, b, c) * c * 8
    # the self-search of the evaluation set stays far below its 1.7 GB score matrix
    assert _ffi.knn_workspace_bytes(20371, 20371, 10) < 8 << 20


def test_slices_fill_the_device_for_few_queries():
    assert _ffi.knn_slices(3, 300001, 5) > 1
    assert _ffi.knn_slices(1, 100000, 10) > 64
    assert _ffi.knn_slices(1, 1, 1) == 1
    assert _ffi.knn_slices(100000, 300, 5) == 1


# ---- the Python API: errors raised before any device call --------------------------------------------------------------------
def test_python_value_errors_need_no_device():
    e = np.zeros((5, 8), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        search_host(np.zeros(8), e, 1)
    with pytest.raises(ValueError, match="2-D"):
        search_host(e, np.zeros((2, 3, 4)), 1)
    with pytest.raises(ValueError, match="dim"):
        search_host(np.zeros((2, 4)), e, 1)
    with pytest.raises(ValueError, match="k = 6"):
        search_host(e, e, 6)
    with pytest.raises(ValueError, match="k = 5"):
        search_host(e, e, 5, exclude=np.arange(5))
    with pytest.raises(ValueError, match="k = 0"):
        search_host(e, e, 0)
    with pytest.raises(ValueError, match="empty"):
        search_host(e, np.zeros((0, 8)), 1)
    with pytest.raises(ValueError, match="metric"):
        search_host(e, e, 1, metric="l2")
    with pytest.raises(ValueError, match="metric"):
        retrieval.EmbeddingIndex(e, metric="l2")
    with pytest.raises(ValueError, match="2-D"):
        retrieval.EmbeddingIndex(np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="not cpu"):
        retrieval.EmbeddingIndex(e, device="cpu")
    assert retrieval.MAX_K == _ffi.KNN_MAX_K >= 64
