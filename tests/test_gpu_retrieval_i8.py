"""GPU: the int8 embedding index -- acx_knn_quantize_i8 / acx_knn_search_i8 / acx_knn_rescore against their host definitions
(codes, scale bits, indices and score bits EQUAL), the operand map of the i8 matrix instruction derived with exact integer
data, and QuantizedIndex against EmbeddingIndex on the planted corpora."""
import numpy as np
import pytest
import torch

import retrieval_i8_cases as rc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import retrieval
from audioset_convnext_inf_amd.pytorch.retrieval import (EmbeddingIndex, QuantizedIndex, quantize_host, search_i8_host, vote)

pytestmark = pytest.mark.gpu
MAX_K = _ffi.KNN_MAX_K


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return _ffi.stream_ptr(torch.device("cuda", torch.cuda.current_device()))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def raw_quantize(x, inv=None):
    """acx_knn_quantize_i8 on a contiguous device tensor -> (codes int8 numpy, scales float32 numpy, status int); the code
    buffer is pre-filled, so the zeros of the pad columns are the kernel's."""
    n, dim = x.shape
    pad = -(-dim // 32) * 32
    codes = torch.full((n, pad), 0x55, dtype=torch.int8, device="cuda")
    scale = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.knn_quantize_i8(vp(x), x.stride(0), None if inv is None else vp(inv), n, dim, vp(codes), pad, vp(scale), vp(st), stream())
    return codes.cpu().numpy(), scale.cpu().numpy(), int(st.cpu()[0])


def raw_search_i8(cq, sq, cd, sd, k, exclude=None, ws_extra=0):
    """acx_knn_search_i8 on numpy codes / scales -> (indices int64 numpy, scores float32 numpy, status int)."""
    nq, n = cq.shape[0], cd.shape[0]
    tcq, tsq, tcd, tsd = dev(cq), dev(np.asarray(sq, np.float32)), dev(cd), dev(np.asarray(sd, np.float32))
    ex = None if exclude is None else dev(np.asarray(exclude, np.int32))
    ind = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    st = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    ws_bytes = _ffi.knn_workspace_bytes(nq, n, k) + ws_extra
    ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device="cuda")
    _ffi.knn_search_i8(vp(tcq), tcq.stride(0), vp(tsq), nq, vp(tcd), tcd.stride(0), vp(tsd), n, cq.shape[1], k,
                       None if ex is None else vp(ex), vp(ind), vp(sc), vp(st), (vp(ws), ws_bytes), stream())
    return ind.cpu().numpy().astype(np.int64), sc.cpu().numpy(), int(st.cpu()[0])


def assert_search_equal(cq, sq, cd, sd, k, exclude=None):
    ref_s, ref_i = search_i8_host(cq, sq, cd, sd, k, exclude)
    ind, sc, st = raw_search_i8(cq, sq, cd, sd, k, exclude)
    assert st == 0
    np.testing.assert_array_equal(ind, ref_i)
    np.testing.assert_array_equal(bits(sc), bits(ref_s))
    return ind, sc


# ---- the operand map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 64])
def test_operand_map_with_identity_queries_and_an_asymmetric_database(dim):
    """Query i selects column dim - 32 + i: score (i, j) must be cd[j][dim - 32 + i] -- a transposed or permuted row / column
    map of the A / B fragments or of the accumulator gives other numbers, as cd is not symmetric."""
    cq, cd = rc.operand_map_codes(dim)
    ones = np.ones(32, np.float32)
    ind, sc = assert_search_equal(cq, ones, cd, ones, 32)
    want = cd[:, dim - 32:].T.astype(np.float32)                       # [i][j]
    assert not np.array_equal(want, want.T)
    np.testing.assert_array_equal(sc, np.take_along_axis(want, ind, axis=1))
    np.testing.assert_array_equal(np.sort(ind, axis=1), np.tile(np.arange(32), (32, 1)))


# ---- the quantiser -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("dim", [4, 20, 30, 64, 100, 768, 4096])
def test_quantize_equals_the_host_definition(dim, n):
    rng = np.random.default_rng(dim + n)
    x = rc.quantize_rows(rng, n, dim)
    nonfinite = n > 7
    if nonfinite:
        x[5, dim // 2] = np.nan
        x[6, dim - 1] = np.inf
        x[7, 0] = -np.inf
    xp = np.pad(x, ((0, 0), (0, -dim % 4)))                              # the kernels read multiples of 4 columns (30 -> 32)
    dim4 = xp.shape[1]                                                   # 4, 20 and 100 leave pad columns to the kernel
    xt = dev(xp)
    inv = retrieval.row_norms(xt)
    for metric, inv_t in (("dot", None), ("cosine", inv)):
        ref_c, ref_s = quantize_host(xp, metric, None if inv_t is None else inv_t.cpu().numpy())
        codes, scale, st = raw_quantize(xt, inv_t)
        assert codes.shape == ref_c.shape == (n, -(-dim4 // 32) * 32)
        np.testing.assert_array_equal(codes, ref_c)
        np.testing.assert_array_equal(bits(scale), bits(ref_s))
        assert (codes[:, dim4:] == 0).all()
        assert st == (_ffi.KNN_NONFINITE if nonfinite else 0)
        if nonfinite:
            assert np.isnan(scale[5:8]).all() and (codes[5:8] == 0).all() and np.isfinite(np.delete(scale, [5, 6, 7])).all()
        if n > 4:
            assert scale[4] == 0 and (codes[4] == 0).all()
            if metric == "dot":                                          # the halves: round to even, and +-127 at the ends
                np.testing.assert_array_equal(codes[3, :dim], np.rint(x[3]).astype(np.int8))
                assert (np.abs(x[3, 1:] - np.trunc(x[3, 1:])) == 0.5).all()


# ---- the coarse search ---------------------------------------------------------------------------------------------------------------
def scales(rng, n):
    return (0.5 + rng.random(n)).astype(np.float32) * np.float32(1e-3)


GRID = [  # kind, dim, n, nq, k
    ("random", 32, 1, 1, 1), ("random", 96, 63, 31, 32), ("random", 768, 64, 33, 33), ("random", 768, 65, 65, 64),
    ("random", 96, 257, 65, 128), ("random", 768, 1000, 33, 32), ("random", 4096, 257, 33, 33), ("random", 768, 257, 65, 128),
    ("random", 4096, 64, 65, 1), ("random", 768, 257, 31, 128),
    ("tie", 96, 1000, 65, 64), ("tie", 32, 257, 33, 128), ("tie", 768, 1000, 31, 33), ("tie", 96, 65, 1, 32),
    ("extreme", 4096, 65, 33, 32), ("extreme", 4096, 257, 1, 64),
    ("ascending", 32, 1000, 33, 32), ("ascending", 96, 1000, 65, 1), ("ascending", 32, 1000, 1, 128), ("ascending", 32, 257, 65, 64),
]


def grid_codes(kind, dim, n, nq, seed):
    rng = np.random.default_rng(seed)
    if kind == "ascending":
        return rc.ascending_queries(nq, dim), np.ones(nq, np.float32), rc.ascending_codes(n, dim), np.ones(n, np.float32)
    gen = {"random": rc.random_codes, "tie": rc.tie_codes, "extreme": rc.extreme_codes}[kind]
    return gen(rng, nq, dim), scales(rng, nq), gen(rng, n, dim), scales(rng, n)


@pytest.mark.parametrize("kind,dim,n,nq,k", GRID)
def test_search_i8_equals_the_host_definition(kind, dim, n, nq, k):
    cq, sq, cd, sd = grid_codes(kind, dim, n, nq, seed=dim + 7 * n + nq)
    ind, sc = assert_search_equal(cq, sq, cd, sd, k)
    if kind == "extreme" and dim == 4096:
        assert np.abs(cq.astype(np.int64) @ cd.astype(np.int64).T).max() == 66064384
    if kind == "ascending":
        np.testing.assert_array_equal(ind[0], np.arange(n - 1, n - 1 - k, -1))


@pytest.mark.parametrize("kind,dim,n,nq,k", [("random", 96, 257, 33, 32), ("tie", 768, 300, 65, 33), ("tie", 32, 64, 31, 63)])
def test_search_i8_exclude_and_self_search(kind, dim, n, nq, k):
    cq, sq, cd, sd = grid_codes(kind, dim, n, nq, seed=3)
    rng = np.random.default_rng(5)
    ex = rng.integers(-1, n, size=nq)
    ind, _ = assert_search_equal(cq, sq, cd, sd, k, ex)
    assert all(ex[r] not in ind[r] for r in range(nq))
    ind, _ = assert_search_equal(cd, sd, cd, sd, k, np.arange(n))          # the self-search
    assert all(r not in ind[r] for r in range(n))


def test_search_i8_many_slices_equal_one_slice(monkeypatch):
    refresh = _ffi.lib().acx_tuning_refresh
    cases = [grid_codes(kind, dim, 1000, nq, seed=9) + (k,) for kind, dim, nq, k in
             (("random", 768, 33, 10), ("tie", 96, 65, 64), ("ascending", 32, 31, 128), ("tie", 4096, 1, 33))]
    monkeypatch.setenv("ACX_KNN_SLICE_ROWS", str(1 << 20))
    refresh()
    try:
        assert _ffi.knn_slices(33, 1000, 10) == 1
        one = [raw_search_i8(*c) for c in cases]
        monkeypatch.setenv("ACX_KNN_SLICE_ROWS", "64")
        refresh()
        assert _ffi.knn_slices(33, 1000, 10) == 16
        many = [raw_search_i8(*c) for c in cases]
    finally:
        monkeypatch.delenv("ACX_KNN_SLICE_ROWS", raising=False)
        refresh()
    for c, (i1, s1, st1), (i2, s2, st2) in zip(cases, one, many):
        ref_s, ref_i = search_i8_host(*c)
        assert st1 == 0 and st2 == 0
        np.testing.assert_array_equal(i1, ref_i)
        np.testing.assert_array_equal(i2, ref_i)
        np.testing.assert_array_equal(bits(s1), bits(ref_s))
        np.testing.assert_array_equal(bits(s2), bits(ref_s))


@pytest.mark.parametrize("kind,nq,k", [("random", 1, 40), ("tie", 3, 128), ("ascending", 2, 10)])
def test_search_i8_two_level_merge_equals_the_host_definition(kind, nq, k):
    """Room behind the slices' lists switches a search of 16 or more slices to the two-level merge: the same result."""
    n = 150000
    cq, sq, cd, sd = grid_codes(kind, 32, n, nq, seed=21)
    if kind == "ascending":                                                 # rows beyond 12 800 repeat: ties by index too
        cd = cd[np.arange(n) % 12800]
    slices = _ffi.knn_slices(nq, n, k)
    assert slices >= 16
    ref_s, ref_i = search_i8_host(cq, sq, cd, sd, k)
    for extra in (0, nq * (int(slices ** 0.5) + 2) * k * 8):
        ind, sc, st = raw_search_i8(cq, sq, cd, sd, k, ws_extra=extra)
        assert st == 0
        np.testing.assert_array_equal(ind, ref_i)
        np.testing.assert_array_equal(bits(sc), bits(ref_s))


def test_search_i8_zero_and_nan_scales():
    cq, sq, cd, sd = grid_codes("random", 96, 300, 33, seed=13)
    sq[3] = 0.0                                                              # a zero query: every score 0, the index decides
    sd[[0, 17, 299]] = 0.0                                                   # zero rows
    ind, sc = assert_search_equal(cq, sq, cd, sd, 40)
    np.testing.assert_array_equal(ind[3], np.arange(40))
    assert (sc[3] == 0).all() and not np.signbit(sc).any()
    sd[5] = np.nan
    ind, sc, st = raw_search_i8(cq, sq, cd, sd, 40)
    assert st == _ffi.KNN_NONFINITE and (ind == -1).all() and np.isnan(sc).all()
    sd[5] = 1.0
    sq[32] = np.nan
    ind, sc, st = raw_search_i8(cq, sq, cd, sd, 40)
    assert st == _ffi.KNN_NONFINITE and (ind == -1).all() and np.isnan(sc).all()


# ---- the rerank ----------------------------------------------------------------------------------------------------------------------
def raw_search(q, d, k, metric, rq=None, rd=None):
    nq, n = q.shape[0], d.shape[0]
    ind = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    sc = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = _ffi.knn_workspace_bytes(nq, n, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    _ffi.knn_search(vp(q), q.stride(0), None if rq is None else vp(rq), nq, vp(d), d.stride(0), None if rd is None else vp(rd), n,
                    q.shape[1], _ffi.KNN_METRICS[metric], k, None, vp(ind), vp(sc), vp(st), (vp(ws), ws_bytes), stream())
    return ind, sc, int(st.cpu()[0])


def raw_rescore(q, d, cand, k, metric, rq=None, rd=None):
    nq, kc = cand.shape
    ind = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    st = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    _ffi.knn_rescore(vp(q), q.stride(0), None if rq is None else vp(rq), nq, vp(d), d.stride(0), None if rd is None else vp(rd),
                     d.shape[0], q.shape[1], _ffi.KNN_METRICS[metric], vp(cand), cand.stride(0), kc, k, vp(ind), vp(sc), vp(st), stream())
    return ind, sc, int(st.cpu()[0])


@pytest.mark.parametrize("dim", [4, 20, 768])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128])
def test_rescore_of_all_rows_equals_the_exact_search(n, dim):
    rng = np.random.default_rng(n + dim)
    nq = 9
    q, d = dev(rng.standard_normal((nq, dim)).astype(np.float32)), dev(rng.standard_normal((n, dim)).astype(np.float32))
    d[n // 2] = d[0]                                                            # equal scores: the index decides
    cand = dev(np.stack([rng.permutation(n) for _ in range(nq)]).astype(np.int32))
    rq, rd = retrieval.row_norms(q), retrieval.row_norms(d)
    for metric, a, b in (("dot", None, None), ("cosine", rq, rd)):
        for k in sorted({n, (n + 1) // 2, 1}):
            ei, es, est = raw_search(q, d, k, metric, a, b)
            ri, rs, rst = raw_rescore(q, d, cand, k, metric, a, b)
            assert est == 0 and rst == 0
            assert torch.equal(ri, ei) and torch.equal(rs.view(torch.int32), es.view(torch.int32)), (metric, k)


def test_rescore_skips_missing_and_outside_candidates():
    rng = np.random.default_rng(2)
    q, d = dev(rng.standard_normal((5, 768)).astype(np.float32)), dev(rng.standard_normal((100, 768)).astype(np.float32))
    full_i, full_s, _ = raw_search(q, d, 100, "dot")
    c = np.stack([rng.permutation(100)[:70] for _ in range(5)]).astype(np.int32)
    c[:, 10:60] = -1                                                            # 20 valid candidates a query, in both passes
    ri, rs, st = raw_rescore(q, d, dev(c), 30, "dot")
    assert st == 0
    for r in range(5):
        keep = [j for j in full_i[r].tolist() if j in set(c[r].tolist())]
        assert ri[r, :20].tolist() == keep and (ri[r, 20:] == -1).all() and torch.isnan(rs[r, 20:]).all()
        pos = [full_i[r].tolist().index(j) for j in keep]
        assert torch.equal(rs[r, :20].view(torch.int32), full_s[r, pos].view(torch.int32))
    c[2, 3], c[4, 65] = 100, -5                                                 # outside [0, n): skipped, and reported
    ri, rs, st = raw_rescore(q, d, dev(c), 30, "dot")
    assert st == _ffi.KNN_BAD_INDEX
    assert (ri >= -1).all() and (ri < 100).all() and (ri[2] >= 0).sum() == 19 and (ri[4] >= 0).sum() == 19 and (ri[0] >= 0).sum() == 20
    q[1, 5] = float("nan")                                                      # a non-finite score: that query's row only
    ri, rs, st = raw_rescore(q, d, dev(c), 30, "dot")
    assert st == _ffi.KNN_BAD_INDEX | _ffi.KNN_NONFINITE
    assert (ri[1] == -1).all() and torch.isnan(rs[1]).all() and (ri[0] >= 0).sum() == 20


# ---- QuantizedIndex ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=range(len(rc.PLANTED)))
def corpus(request):
    rows, queries = rc.planted(*rc.PLANTED[request.param])
    exact = EmbeddingIndex(dev(rows), metric="cosine")
    return rows, queries, exact, exact.search(dev(queries), rc.K)


def test_two_stage_search_equals_the_exact_search_where_the_candidates_cover_it(corpus):
    rows, queries, exact, (es, ei) = corpus
    qidx = exact.quantize(rerank=True, oversample=4)
    assert qidx.exact is exact and qidx.exact.embeddings.data_ptr() == exact.embeddings.data_ptr()       # shared, not copied
    assert len(qidx) == len(rows) and qidx.codes.shape == (len(rows), -(-rows.shape[1] // 32) * 32)
    s, i = qidx.search(dev(queries), rc.K)
    _, coarse = exact.quantize(rerank=False).search(dev(queries), rc.KC)
    qidx.check()
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and i.shape == (len(queries), rc.K)
    covered = np.array([set(a) <= set(b) for a, b in zip(ei.cpu().numpy().tolist(), coarse.cpu().numpy().tolist())])
    print("queries not covered by the device candidates: %d of %d" % ((~covered).sum(), len(covered)))
    assert (~covered).sum() <= rc.EXEMPT_SHARE * len(covered)
    rows_ok = torch.from_numpy(covered).cuda()
    assert torch.equal(i[rows_ok], ei[rows_ok]) and torch.equal(s[rows_ok].view(torch.int32), es[rows_ok].view(torch.int32))


def test_coarse_index_equals_the_host_definitions(corpus):
    rows, queries, exact, _ = corpus
    qt = dev(queries)
    qidx = QuantizedIndex(dev(rows), metric="cosine", rerank=False)
    assert qidx.exact is None
    cd, sd = quantize_host(rows, "cosine", exact.inverse_norms.cpu().numpy())
    np.testing.assert_array_equal(qidx.codes.cpu().numpy(), cd)
    np.testing.assert_array_equal(bits(qidx.scales.cpu().numpy()), bits(sd))
    cq, sq = quantize_host(queries, "cosine", retrieval.row_norms(qt).cpu().numpy())
    ref_s, ref_i = search_i8_host(cq, sq, cd, sd, rc.KC)
    s, i = qidx.search(qt, rc.KC)
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(bits(s.cpu().numpy()), bits(ref_s))
    # the self-search on the stored codes
    ref_s, ref_i = search_i8_host(cd[:300], sd[:300], cd[:300], sd[:300], 5, np.arange(300))
    s, i = QuantizedIndex(dev(rows[:300]), rerank=False).search(None, 5)
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(bits(s.cpu().numpy()), bits(ref_s))


@pytest.mark.parametrize("rerank", [True, False])
def test_add_in_two_parts_equals_one_build(rerank):
    rows, queries = rc.planted(500, 64, 20, 1.0, 40, 3)
    y = (np.random.default_rng(4).random((500, 7)) < 0.3).astype(np.uint8)
    one = QuantizedIndex(dev(rows), target=dev(y), rerank=rerank)
    two = QuantizedIndex(dev(rows[:123]), target=dev(y[:123]), rerank=rerank).add(dev(rows[123:]), dev(y[123:]))
    assert len(one) == len(two) == 500
    assert torch.equal(one.codes, two.codes) and torch.equal(one.scales.view(torch.int32), two.scales.view(torch.int32))
    assert torch.equal(one.target, two.target)
    (s1, i1), (s2, i2) = one.search(dev(queries), 10), two.search(dev(queries), 10)
    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    # classify is the vote of its own search
    probs = two.classify(dev(queries), 10, weights="similarity")
    assert torch.equal(probs, vote(i2, s2, two.target, "similarity"))
    two.check()
    with pytest.raises(ValueError, match=r"k \* oversample = 33 \* 4"):
        QuantizedIndex(dev(rows), rerank=True).search(dev(queries), 33)


def test_rows_added_to_a_shared_index_are_seen():
    rows, queries = rc.planted(300, 64, 20, 1.0, 20, 5)
    exact = EmbeddingIndex(dev(rows[:200]))
    qidx = exact.quantize()
    exact.add(dev(rows[200:]))
    assert len(qidx) == 300
    whole = QuantizedIndex(dev(rows))
    (s1, i1), (s2, i2) = qidx.search(dev(queries), 10), whole.search(dev(queries), 10)
    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))


def test_search_captured_in_a_graph_replays_the_eager_bits():
    rows, queries = rc.planted(1000, 64, 20, 1.0, 70, 6)
    qidx = QuantizedIndex(dev(rows))
    qt = dev(queries)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = qidx.search(qt, 10)                                            # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s, i = qidx.search(qt, 10)
    fresh = dev(rc.planted(1000, 64, 20, 1.0, 70, 7)[1])
    qt.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    got = s.clone(), i.clone()
    want = qidx.search(fresh, 10)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert not torch.equal(got[1], eager[1])
    qidx.check()


@pytest.mark.parametrize("rerank", [True, False])
def test_check_raises_after_a_nan_query(rerank):
    rows, queries = rc.planted(300, 64, 20, 1.0, 5, 8)
    qidx = QuantizedIndex(dev(rows), rerank=rerank)
    qidx.search(dev(queries), 3)
    qidx.check()
    queries[2, 7] = np.nan
    s, i = qidx.search(dev(queries), 3)
    assert (i == -1).all() and torch.isnan(s).all()
    with pytest.raises(ValueError, match="NaN or infinite"):
        qidx.check()
    qidx.check()                                                               # the word was cleared
