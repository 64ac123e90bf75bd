"""GPU (`-m gpu`): nearest-neighbour search over embeddings (csrc/knn.hip, pytorch/retrieval.py).

Exact cases use integer-valued embeddings (entries in -8 .. 8, dim 768: every product and partial sum is an integer below 2^24,
so fp32 is exact in any order) and must EQUAL the float64 host reference `search_host`, indices and scores.  Rounded cases
(standard-normal data) are checked for validity under the derived rounding bound of an fp32 dot product,
b = (dim + 8) 2^-24 sum_i |q_i x_i| (divided by the norms for cosine): returned scores within b of the float64 score, rows
sorted by the one total order, and no row left out whose float64 score could not have lost to the k-th returned one."""

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import retrieval
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract
from audioset_convnext_inf_amd.pytorch.retrieval import EmbeddingIndex, search_host, vote_host

pytestmark = pytest.mark.gpu
MAX_K = _ffi.KNN_MAX_K
DIM = 768


def raw_search(q, d, k, metric="dot", exclude=None, ws=None):
    """acx_knn_search on contiguous device tensors -> (indices int32, scores, status int)."""
    nq, n = q.shape[0], d.shape[0]
    cos = metric == "cosine"
    rq = retrieval.row_norms(q) if cos else None
    rd = retrieval.row_norms(d) if cos else None
    ind = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    sc = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    if ws is None:
        ws = torch.empty(_ffi.knn_workspace_bytes(nq, n, k), dtype=torch.uint8, device="cuda")
    _ffi.knn_search(vp(q), q.stride(0), vp(rq), nq, vp(d), d.stride(0), vp(rd), n, q.shape[1], _ffi.KNN_METRICS[metric], k,
                    vp(exclude), vp(ind), vp(sc), vp(st), (vp(ws), ws.numel()), _ffi.stream_ptr(q.device))
    torch.cuda.synchronize()
    return ind, sc, int(st.cpu()[0])


def ints(rng, rows, dim=DIM):
    return rng.integers(-8, 9, size=(rows, dim)).astype(np.float32)


def one_hot(values, dim=DIM):
    x = np.zeros((len(values), dim), np.float32)
    x[:, 0] = values
    return x


def exact_inputs(kind, nq, n, seed):
    rng = np.random.default_rng(seed)
    q = ints(rng, nq)
    if kind == "random":
        d = ints(rng, n)
    elif kind == "four_rows":                   # only four distinct rows
        d = ints(rng, 4)[np.arange(n) % 4]
    elif kind == "one_row":                     # every score ties: the answer is 0 .. k-1
        d = np.tile(ints(rng, 1), (n, 1))
    elif kind == "dup_queries":                 # each query appears several times in the database
        d = ints(rng, n)
        for r in range(min(3 * nq, n)):
            d[(r * 7) % n] = q[r % nq]
    elif kind == "increasing":                  # every row beats the threshold
        q, d = one_hot(1 + np.arange(nq) % 8), one_hot(1 + np.arange(n))
    elif kind == "decreasing":
        q, d = one_hot(1 + np.arange(nq) % 8), one_hot(n - np.arange(n))
    return q, d


EXACT_SHAPES = [(1, 1, 1), (1, 31, 31), (33, 65, 1), (33, 65, 7), (33, 65, 64), (5, 1000, 10), (64, 4097, MAX_K)]
EXACT_KINDS = ["random", "four_rows", "one_row", "dup_queries", "increasing", "decreasing"]


@pytest.mark.parametrize("kind", EXACT_KINDS)
@pytest.mark.parametrize("nq,n,k", EXACT_SHAPES)
def test_exact_cases_equal_the_host_reference(nq, n, k, kind):
    q, d = exact_inputs(kind, nq, n, seed=nq * 131 + n)
    ref_s, ref_i = search_host(q, d, k, "dot")
    idx = EmbeddingIndex(torch.from_numpy(d).cuda(), metric="dot")
    s, i = idx.search(torch.from_numpy(q).cuda(), k)
    idx.check()
    assert i.dtype == torch.int64 and s.dtype == torch.float32 and i.shape == (nq, k)
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), ref_s)
    if kind == "one_row":
        np.testing.assert_array_equal(i.cpu().numpy(), np.tile(np.arange(k), (nq, 1)))


# ---- (b) rounded cases ---------------------------------------------------------------------------------------------------------
def normal_inputs(dim, nq, n, seed):
    """Standard-normal rows; a quarter of the database lies within 0.05 sigma of a query."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    d = rng.standard_normal((n, dim)).astype(np.float32)
    near = n // 4
    d[:near] = q[np.arange(near) % nq] + 0.05 * rng.standard_normal((near, dim)).astype(np.float32)
    return q, d


def check_valid(q, d, metric, scores, indices, exclude=None):
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    dim = q.shape[1]
    s64 = q64 @ d64.T
    b = (dim + 8) * 2.0 ** -24 * (np.abs(q64) @ np.abs(d64).T)
    if metric == "cosine":
        nn = np.sqrt((q64 * q64).sum(1))[:, None] * np.sqrt((d64 * d64).sum(1))[None, :]
        s64, b = s64 / nn, b / nn
    nq, k = indices.shape
    rows = np.arange(nq)[:, None]
    assert ((indices >= 0) & (indices < d.shape[0])).all()
    err = np.abs(scores.astype(np.float64) - s64[rows, indices])
    assert (err <= b[rows, indices]).all(), float((err / b[rows, indices]).max())          # 1
    for r in range(nq):                                                                    # 2
        keys = list(zip(-scores[r].astype(np.float64), indices[r]))
        assert keys == sorted(keys), r
        assert len(set(indices[r].tolist())) == k, r
        if exclude is not None:
            assert exclude[r] not in indices[r]
    out = np.ones(s64.shape, bool)                                                         # 3
    out[rows, indices] = False
    if exclude is not None:
        out[np.arange(nq), exclude] = False
    kth = indices[:, -1]
    limit = (s64[np.arange(nq), kth] + b[np.arange(nq), kth])[:, None]
    assert ((s64 - b <= limit) | ~out).all()


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("dim,nq,n", [(768, 33, 1001), (772, 5, 300), (4, 7, 65)])
def test_rounded_cases_are_valid_under_the_fp32_bound(dim, nq, n, pad, metric):
    q, d = normal_inputs(dim - pad, nq, n, seed=dim + n)
    idx = EmbeddingIndex(torch.from_numpy(d).cuda(), metric=metric)
    s, i = idx.search(torch.from_numpy(q).cuda(), 10)
    idx.check()
    assert idx.dim == dim - pad and idx.embeddings.shape == (n, dim - pad)
    check_valid(q, d, metric, s.cpu().numpy(), i.cpu().numpy())


# ---- (c) bits do not depend on the shape of the call --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_score_bits_are_shape_independent(metric):
    q, d = normal_inputs(DIM, 33, 128, seed=5)
    qt, dt = torch.from_numpy(q).cuda(), torch.from_numpy(d).cuda()
    s_all, i_all = EmbeddingIndex(dt, metric=metric).search(qt, 128)          # k = n: every pair's score
    full = torch.empty((33, 128), device="cuda").scatter_(1, i_all, s_all)
    # a sub-range of the database: the rows move inside their tile
    s_sub, i_sub = EmbeddingIndex(dt[37:101], metric=metric).search(qt, 64)
    assert torch.equal(s_sub, full[:, 37:101].gather(1, i_sub))
    # one query alone, and k = 1 against k = 64
    for r in (0, 17, 32):
        s1, i1 = EmbeddingIndex(dt, metric=metric).search(qt[r:r + 1], 64)
        assert torch.equal(s1, s_all[r:r + 1, :64]) and torch.equal(i1, i_all[r:r + 1, :64])
    s_k1, i_k1 = EmbeddingIndex(dt, metric=metric).search(qt, 1)
    assert torch.equal(s_k1, s_all[:, :1]) and torch.equal(i_k1, i_all[:, :1])

    # a larger database: whole against a sub-range, add() against cat, chunked against one call
    q, d = normal_inputs(DIM, 33, 1001, seed=6)
    d = np.roll(d, 300, axis=0)                                               # the rows near the queries: 300 .. 549
    qt, dt = torch.from_numpy(q).cuda(), torch.from_numpy(d).cuda()
    whole = EmbeddingIndex(dt, metric=metric)
    s_w, i_w = whole.search(qt, 64)
    s_sub, i_sub = EmbeddingIndex(dt[290:900], metric=metric).search(qt, 64)
    full = torch.full((33, 1001), float("nan"), device="cuda").scatter_(1, i_w, s_w)
    same = full[:, 290:900].gather(1, i_sub)                                  # the whole search's score of each row found here
    both = ~torch.isnan(same)
    assert bool(both[:, :5].all())                                            # the planted rows lead both lists
    assert torch.equal(same[both], s_sub[both]) and torch.equal(i_sub[:, :5] + 290, i_w[:, :5])
    grown = EmbeddingIndex(dt[:600].clone(), metric=metric)
    grown.add(dt[600:])
    assert len(grown) == 1001 and torch.equal(grown.embeddings, dt)
    s_g, i_g = grown.search(qt, 64)
    assert torch.equal(s_g, s_w) and torch.equal(i_g, i_w)
    small = EmbeddingIndex(dt, metric=metric, workspace_limit=_ffi.knn_workspace_bytes(5, 1001, 64))
    assert small._chunk(33, 64) < 33
    s_c, i_c = small.search(qt, 64)
    assert torch.equal(s_c, s_w) and torch.equal(i_c, i_w)
    check_valid(q, d, metric, s_w.cpu().numpy(), i_w.cpu().numpy())

    # the workspace's contents do not matter
    ws = torch.empty(_ffi.knn_workspace_bytes(33, 1001, 64), dtype=torch.uint8, device="cuda")
    res = []
    for fill in (0xFF, 0x00):
        ws.fill_(fill)
        ind, sc, st = raw_search(qt, dt, 64, metric, ws=ws)
        assert st == 0
        res.append((ind.clone(), sc.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0].long(), i_w) and torch.equal(res[0][1], s_w)


# ---- (d) many slices --------------------------------------------------------------------------------------------------------------
def test_many_slices_equal_one_slice(monkeypatch):
    refresh = _ffi.lib().acx_tuning_refresh
    monkeypatch.delenv("ACX_KNN_SLICE_ROWS", raising=False)
    refresh()
    rng = np.random.default_rng(11)
    qi, di = ints(rng, 64), ints(rng, 4097)
    di[1000:1040] = qi[:40]
    qn, dn = normal_inputs(DIM, 64, 4097, seed=12)
    cases = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), m, k)
             for a, b, m in ((qi, di, "dot"), (qn, dn, "dot"), (qn, dn, "cosine")) for k in (10, MAX_K)]
    monkeypatch.setenv("ACX_KNN_SLICE_ROWS", str(1 << 20))
    refresh()
    try:
        assert _ffi.knn_slices(64, 4097, 10) == 1
        one = [raw_search(a, b, k, m) for a, b, m, k in cases]
        monkeypatch.setenv("ACX_KNN_SLICE_ROWS", "64")
        refresh()
        assert _ffi.knn_slices(64, 4097, 10) == 65
        many = [raw_search(a, b, k, m) for a, b, m, k in cases]
    finally:
        monkeypatch.delenv("ACX_KNN_SLICE_ROWS", raising=False)
        refresh()
    for (i1, s1, st1), (i2, s2, st2) in zip(one, many):
        assert st1 == 0 and st2 == 0
        assert torch.equal(i1, i2) and torch.equal(s1, s2)
    for (ind, sc, _), k in zip(many[:2], (10, MAX_K)):
        ref_s, ref_i = search_host(qi, di, k, "dot")
        np.testing.assert_array_equal(ind.cpu().numpy(), ref_i)
        np.testing.assert_array_equal(sc.cpu().numpy().astype(np.float64), ref_s)


def test_natural_slicing_of_a_long_database():
    nq, n, k = 3, 300001, 10
    assert _ffi.knn_slices(nq, n, k) > 1
    rng = np.random.default_rng(13)
    q, d = ints(rng, nq, 8), ints(rng, n, 8)
    idx = EmbeddingIndex(torch.from_numpy(d).cuda(), metric="dot")
    s, i = idx.search(torch.from_numpy(q).cuda(), k)
    idx.check()
    ref_s, ref_i = search_host(q, d, k, "dot")
    np.testing.assert_array_equal(i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), ref_s)


# ---- (e) exclude, self-search, strides ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_self_search_excludes_only_the_row_itself(metric):
    rng = np.random.default_rng(17)
    d = ints(rng, 300)
    d[100:150] = d[:50]                                   # duplicated rows: the duplicate IS returned
    idx = EmbeddingIndex(torch.from_numpy(d).cuda(), metric=metric)
    s, i = idx.search(None, 7)
    idx.check()
    i_np = i.cpu().numpy()
    assert (i_np != np.arange(300)[:, None]).all()
    ref_s, ref_i = search_host(d, d, 7, metric, exclude=np.arange(300))
    if metric == "dot":
        np.testing.assert_array_equal(i_np, ref_i)
        np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), ref_s)
    else:
        check_valid(d, d, metric, s.cpu().numpy(), i_np, exclude=np.arange(300))
    assert (i_np[:50, 0] == np.arange(100, 150)).all() and (i_np[100:150, 0] == np.arange(50)).all()
    # an explicit exclude list with -1 entries
    ex = np.where(np.arange(300) % 2 == 0, np.arange(300), -1)
    s2, i2 = idx.search(torch.from_numpy(d).cuda(), 7, exclude=torch.from_numpy(ex))
    if metric == "dot":
        np.testing.assert_array_equal(i2.cpu().numpy(), search_host(d, d, 7, metric, exclude=ex)[1])
    with pytest.raises(ValueError, match="k = 5"):
        EmbeddingIndex(torch.from_numpy(d[:5]).cuda(), metric=metric).search(None, 5)


def test_column_slices_are_read_in_place():
    rng = np.random.default_rng(19)
    wide = torch.from_numpy(rng.standard_normal((200, 1024)).astype(np.float32)).cuda()
    qwide = torch.from_numpy(rng.standard_normal((9, 1024)).astype(np.float32)).cuda()
    view = wide[:, 4:772]
    idx = EmbeddingIndex(view, metric="cosine")
    assert idx.embeddings.data_ptr() == wide.data_ptr() + 16 and idx.embeddings.stride(0) == 1024
    s, i = idx.search(qwide[:, 4:772], 10)
    s2, i2 = EmbeddingIndex(view.contiguous(), metric="cosine").search(qwide[:, 4:772].contiguous(), 10)
    assert torch.equal(s, s2) and torch.equal(i, i2)
    # a slice the kernels cannot read in place (odd offset) is copied
    odd = EmbeddingIndex(wide[:, 3:771], metric="cosine")
    assert odd.embeddings.stride(0) == 768
    # numpy / CPU inputs are copied over
    host = EmbeddingIndex(view.cpu().numpy(), metric="cosine")
    s3, i3 = host.search(qwide[:, 4:772].cpu(), 10)
    assert torch.equal(s3, s) and torch.equal(i3, i)


# ---- (f) status ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_nonfinite_inputs_are_reported(metric):
    rng = np.random.default_rng(23)
    q = torch.from_numpy(ints(rng, 5)).cuda()
    d = torch.from_numpy(ints(rng, 70)).cuda()
    for where, value in (("q", float("nan")), ("d", float("nan")), ("d", float("inf")), ("q", float("-inf"))):
        qb, db = q.clone(), d.clone()
        (qb if where == "q" else db)[3, 100] = value
        idx = EmbeddingIndex(db, metric=metric)
        idx.search(qb, 4)
        with pytest.raises(ValueError, match="NaN or infinite"):
            idx.check()
        ind, sc, st = raw_search(qb, db, 4, metric)
        assert st == _ffi.KNN_NONFINITE
        assert (ind == -1).all() and torch.isnan(sc).all()
    ind, sc, st = raw_search(q, d, 4, metric)                  # the next valid call clears the word
    assert st == 0 and (ind >= 0).all() and torch.isfinite(sc).all()
    idx = EmbeddingIndex(d, metric=metric)
    idx.search(q, 4)
    idx.check()


def test_vote_reports_an_index_outside_the_targets():
    y = torch.ones((9, 5), dtype=torch.uint8, device="cuda")
    ind = torch.tensor([[0, 1, 2], [3, 9, 4]], dtype=torch.int32, device="cuda")
    out = torch.empty((2, 5), dtype=torch.float32, device="cuda")
    st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    _ffi.knn_vote(vp(ind), None, 2, 3, vp(y), _ffi.TARGET_U8, 5, 9, 5, _ffi.KNN_UNIFORM, 0.07, vp(out), 5, vp(st),
                  _ffi.stream_ptr(y.device))
    assert int(st.cpu()[0]) == _ffi.KNN_BAD_INDEX
    ind[1, 1] = 8
    _ffi.knn_vote(vp(ind), None, 2, 3, vp(y), _ffi.TARGET_U8, 5, 9, 5, _ffi.KNN_UNIFORM, 0.07, vp(out), 5, vp(st),
                  _ffi.stream_ptr(y.device))
    assert int(st.cpu()[0]) == 0 and bool((out == 1).all())


# ---- (g) vote -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vote_data():
    rng = np.random.default_rng(29)
    n, nq = 400, 21
    d = rng.standard_normal((n, 64)).astype(np.float32)
    q = rng.standard_normal((nq, 64)).astype(np.float32)
    idx = EmbeddingIndex(torch.from_numpy(d).cuda(), metric="cosine")
    found = {k: idx.search(torch.from_numpy(q).cuda(), k) for k in (1, 10, MAX_K)}
    return rng, n, q, d, found


@pytest.mark.parametrize("C", [1, 50, 527])
@pytest.mark.parametrize("k", [1, 10, MAX_K])
def test_vote(vote_data, C, k):
    rng, n, q, d, found = vote_data
    s, i = found[k]
    y8 = (np.random.default_rng(C).random((n, C)) < 0.3).astype(np.uint8)
    yf = np.random.default_rng(C + 1).random((n, C)).astype(np.float32)
    i_np, s_np = i.cpu().numpy(), s.cpu().numpy()
    got = retrieval.vote(i, s, torch.from_numpy(y8).cuda()).cpu().numpy()
    count = y8[i_np].astype(np.int64).sum(axis=1)
    np.testing.assert_array_equal(got, count.astype(np.float32) / np.float32(k))
    tol = (k + 16) * 2.0 ** -23
    for T in (0.07, 1.0):
        for y in (y8, yf):
            got = retrieval.vote(i, s, torch.from_numpy(y).cuda(), "similarity", T).cpu().numpy()
            ref = vote_host(i_np, s_np, y, "similarity", T)
            assert np.abs(got - ref).max() <= tol, (T, y.dtype, float(np.abs(got - ref).max()))
    got = retrieval.vote(i, s, torch.from_numpy(yf).cuda()).cpu().numpy()
    assert np.abs(got - vote_host(i_np, s_np, yf)).max() <= tol


def test_classify_equals_search_then_vote(vote_data):
    rng, n, q, d, found = vote_data
    y = (np.random.default_rng(31).random((n, 50)) < 0.2)
    idx = EmbeddingIndex(torch.from_numpy(d[:250]).cuda(), metric="cosine", target=torch.from_numpy(y[:250]).cuda())
    idx.add(d[250:], target=y[250:])
    assert len(idx) == n and idx.target.shape == (n, 50) and idx.target.dtype == torch.uint8
    qt = torch.from_numpy(q).cuda()
    for weights in ("uniform", "similarity"):
        probs = idx.classify(qt, 10, weights=weights, temperature=0.5)
        s, i = idx.search(qt, 10)
        assert torch.equal(probs, retrieval.vote(i, s, idx.target, weights, 0.5))
    idx.check()
    assert torch.equal(idx.search(qt, 10)[1], found[10][1])
    with pytest.raises(ValueError, match="target"):
        EmbeddingIndex(torch.from_numpy(d).cuda()).classify(qt, 3)
    with pytest.raises(ValueError, match="targets"):
        idx.add(d[:3])
    with pytest.raises(ValueError, match="dim"):
        idx.search(qt[:, :60], 3)
    with pytest.raises(ValueError, match="2-D"):
        idx.search(qt[0], 3)
    with pytest.raises(ValueError, match="k = "):
        idx.search(qt, MAX_K + 1)
    with pytest.raises(ValueError, match="empty"):
        EmbeddingIndex(torch.empty((0, 64), device="cuda")).search(qt, 1)


# ---- (h) through the model ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(synth_sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    return m.to("cuda").eval()


def test_index_and_search_through_the_model(model):
    wav = synth.synth_waveforms(6, 32000, seed=41).cuda()
    clips = [w for w in wav]
    idx = model.build_index(clips)
    assert len(idx) == 6 and idx.metric == "cosine"
    assert torch.equal(idx.embeddings, torch.stack(extract(model, clips, what="scene", pack=True)).cuda())
    hit = model.search(idx, clips[2][None], k=3)
    idx.check()
    assert hit["indices"].shape == (1, 3) and int(hit["indices"][0, 0]) == 2
    assert abs(float(hit["scores"][0, 0]) - 1.0) <= 1e-6
    assert torch.equal(hit["scene"], model.forward_scene_embeddings(clips[2][None]))

    # the whole call in a graph: replayed on fresh audio it gives the bits of the eager call
    x = wav[1:3].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.search(idx, x, k=3)                            # warm-up: workspace, side streams of this stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.search(idx, x, k=3)
    x.copy_(wav[4:6])
    g.replay()
    torch.cuda.synchronize()
    eager = model.search(idx, wav[4:6], k=3)
    for key in ("scores", "indices", "scene"):
        assert torch.equal(out[key], eager[key]), key
    assert out["indices"][:, 0].tolist() == [4, 5]


# ---- (i) beside a forward -----------------------------------------------------------------------------------------------------
def test_search_beside_a_forward(model):
    wav = synth.synth_waveforms(16, 32000, seed=43).cuda()
    q, d = normal_inputs(DIM, 33, 4097, seed=44)
    qt = torch.from_numpy(q).cuda()
    idx = EmbeddingIndex(torch.from_numpy(d).cuda(), metric="cosine")
    alone_fwd = model(wav)["clipwise_logits"].clone()
    alone_s, alone_i = idx.search(qt, 10)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s, i = idx.search(qt, 10)
    fwd = model(wav)["clipwise_logits"]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(fwd, alone_fwd)
    assert torch.equal(s, alone_s) and torch.equal(i, alone_i)
    idx.check()
