"""CPU: the int8 embedding index (pytorch/retrieval.py: quantize_host, search_i8_host, rescore_host, QuantizedIndex;
acx_knn_quantize_i8 / acx_knn_search_i8 / acx_knn_rescore in include/acx.h) -- the host definitions against their stated
properties and a plain Python loop, the coverage condition of the two-stage search on the planted corpora, the argument errors
of the C ABI (host-only paths) and the ValueErrors of the Python API that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import retrieval_i8_cases as rc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import retrieval
from audioset_convnext_inf_amd.pytorch.retrieval import quantize_host, rescore_host, search_host, search_i8_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- quantize_host -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("dim", [4, 30, 64, 768])
def test_quantize_host_properties(metric, dim):
    rng = np.random.default_rng(dim)
    x = rc.quantize_rows(rng, 9, dim)
    x[5] = np.nan if dim == 4 else x[5]
    x[6, dim - 1] = np.inf
    codes, scale = quantize_host(x, metric)
    pad = -(-dim // 32) * 32
    assert codes.dtype == np.int8 and codes.shape == (9, pad) and scale.dtype == np.float32 and scale.shape == (9,)
    assert codes.min() >= -127 and codes.max() <= 127
    assert (codes[:, dim:] == 0).all()
    bad = ~np.isfinite(x).all(axis=1)
    assert bad[6] and np.isnan(scale[bad]).all() and (codes[bad] == 0).all()
    assert scale[4] == 0 and (codes[4] == 0).all()                         # the zero row
    good = ~bad & (np.abs(x).max(axis=1) > 0)
    assert np.isfinite(scale[good]).all() and (scale[good] > 0).all()
    # the row's largest magnitude maps to +-127, with its sign
    for r in np.nonzero(good)[0]:
        top = np.argmax(np.abs(x[r]))
        assert codes[r, top] == (127 if x[r, top] > 0 else -127), r
    # |y - code * scale| <= scale / 2 (1 + 2^-22) -- wherever y g is not within 2^-14 of a tie k + 1/2.  At a tie the bound cannot
    # hold: rint may fall either way on the rounded product fl(y g) = y g (1 + 2^-24), and the code is scaled back by
    # scale = fl(amax / 127), not by 1 / g = 1 / fl(127 / amax), which differ by 2^-23 relative: with |code| <= 127,
    # |y - code scale| <= scale (1 + 2^-23) (1/2 + 127 2^-24) + 127 scale 2^-23 <= scale / 2 (1 + 382 2^-23) < scale / 2 (1 + 2^-14).
    # (Measured at the tie rows of quantize_rows under "cosine": up to scale / 2 (1 + 1.02e-5).)
    if metric == "cosine":
        ss = (x * x).sum(axis=1, dtype=np.float32)
        with np.errstate(all="ignore"):
            y = x * (np.float32(1) / np.sqrt(ss))[:, None]
    else:
        y = x
    y64, c64, s64 = y[good].astype(np.float64), codes[good, :dim].astype(np.float64), scale[good].astype(np.float64)[:, None]
    g64 = (np.float32(127) / np.abs(y[good]).max(axis=1)).astype(np.float64)[:, None]
    tie = np.abs(y64 * g64 - c64) > 0.5 - 2.0 ** -14
    err = np.abs(y64 - c64 * s64)
    print("largest |y - code scale| / (scale / 2): %.9f away from ties, %.9f at ties (%d elements)"
          % ((err / (s64 / 2))[~tie].max(), (err / (s64 / 2))[tie].max() if tie.any() else 0.0, tie.sum()))
    assert (err[~tie] <= np.broadcast_to(s64 / 2 * (1 + 2.0 ** -22), err.shape)[~tie]).all()
    assert (err[tie] <= np.broadcast_to(s64 / 2 * (1 + 2.0 ** -14), err.shape)[tie]).all()


def test_quantize_host_rounds_halves_to_even():
    x = np.array([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5]], dtype=np.float32)
    codes, scale = quantize_host(x, "dot")
    np.testing.assert_array_equal(codes[0, :8], [127, 0, 2, 2, 0, -2, -2, 126])
    assert scale[0] == np.float32(1.0)


def test_quantize_host_cosine_codes_are_those_of_the_normalised_rows():
    rng = np.random.default_rng(2)
    x = rc.quantize_rows(rng, 7, 96)
    ss = (x * x).sum(axis=1, dtype=np.float32)
    inv = np.where(ss > 0, np.float32(1) / np.sqrt(np.where(ss > 0, ss, np.float32(1))), np.float32(0)).astype(np.float32)
    a, sa = quantize_host(x, "cosine")
    b, sb = quantize_host(x * inv[:, None], "dot")
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(sa.view(np.uint32), sb.view(np.uint32))
    c, sc = quantize_host(x, "cosine", inv_norm=inv)
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(sa.view(np.uint32), sc.view(np.uint32))


# ---- search_i8_host ----------------------------------------------------------------------------------------------------------------
def loop_search(cq, sq, cd, sd, k, exclude=None):
    out_s, out_i = [], []
    for i in range(len(cq)):
        rows = []
        for j in range(len(cd)):
            if exclude is not None and exclude[i] == j:
                continue
            t = 0
            for c in range(cq.shape[1]):
                t += int(cq[i, c]) * int(cd[j, c])
            s = np.float32(np.float32(np.float32(t) * np.float32(sq[i])) * np.float32(sd[j]))
            rows.append((-(float(s) + 0.0), j, s))
        rows.sort(key=lambda r: (r[0], r[1]))
        out_s.append([r[2] + np.float32(0) for r in rows[:k]])
        out_i.append([r[1] for r in rows[:k]])
    return np.array(out_s, dtype=np.float32), np.array(out_i)


@pytest.mark.parametrize("gen", [rc.random_codes, rc.tie_codes])
def test_search_i8_host_equals_a_plain_loop(gen):
    rng = np.random.default_rng(4)
    cq, cd = gen(rng, 3, 8), gen(rng, 11, 8)
    sq, sd = rng.random(3).astype(np.float32), rng.random(11).astype(np.float32)
    sd[4] = 0.0
    for k, ex in ((1, None), (5, None), (11, None), (10, np.array([0, -1, 10]))):
        s, i = search_i8_host(cq, sq, cd, sd, k, exclude=ex)
        ls, li = loop_search(cq, sq, cd, sd, k, ex)
        assert s.dtype == np.float32 and i.dtype == np.int64 and i.shape == (3, k)
        np.testing.assert_array_equal(i, li)
        np.testing.assert_array_equal(s.view(np.uint32), ls.view(np.uint32))
        if ex is not None:
            assert all(ex[r] not in i[r] for r in range(3))


def test_search_i8_host_ties_by_index_and_negative_zero():
    cd = np.ones((9, 32), dtype=np.int8)
    _, i = search_i8_host(cd[:2], np.ones(2, np.float32), cd, np.ones(9, np.float32), 9)
    np.testing.assert_array_equal(i, np.tile(np.arange(9), (2, 1)))
    # t = 0 with a negative scale is -0.0: it ties with +0.0 and the index decides; the scores come back as +0.0
    cq = np.zeros((1, 32), dtype=np.int8)
    s, i = search_i8_host(cq, np.array([-1.0], np.float32), cd[:3], np.array([1.0, -1.0, 1.0], np.float32), 3)
    np.testing.assert_array_equal(i, [[0, 1, 2]])
    assert not np.signbit(s).any()


def test_rescore_host_is_search_host_on_the_candidates():
    rng = np.random.default_rng(6)
    q, d = rng.standard_normal((5, 12)), rng.standard_normal((20, 12))
    for metric in ("dot", "cosine"):
        full_s, full_i = search_host(q, d, 20, metric)
        cand = np.stack([rng.permutation(20) for _ in range(5)])
        s, i = rescore_host(q, d, cand, 7, metric)
        np.testing.assert_array_equal(i, full_i[:, :7])
        np.testing.assert_allclose(s, full_s[:, :7], rtol=0, atol=1e-12)
        cand[:, 3:] = -1
        cand[0, 1] = 20
        s, i = rescore_host(q, d, cand, 4, metric)
        assert (i[1:, 3] == -1).all() and np.isnan(s[1:, 3]).all() and (i[0, 2:] == -1).all()
        for r in range(1, 5):
            assert set(i[r, :3]) == set(cand[r, :3])


# ---- the coverage condition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.PLANTED)
def test_coarse_candidates_cover_the_exact_neighbours(case):
    """The share of queries whose float64 top 10 is not inside the host coarse top 40 (measured: 0 of 200 on all three)."""
    rows, queries = rc.planted(*case)
    _, exact = search_host(queries, rows, rc.K, "cosine")
    cd, sd = quantize_host(rows, "cosine")
    cq, sq = quantize_host(queries, "cosine")
    _, coarse = search_i8_host(cq, sq, cd, sd, rc.KC)
    missed = sum(1 for r in range(len(queries)) if not set(exact[r]) <= set(coarse[r]))
    print("queries not covered: %d of %d" % (missed, len(queries)))
    assert missed <= rc.EXEMPT_SHARE * len(queries)


# ---- the C ABI: host-only paths -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    for name in ("acx_knn_quantize_i8", "acx_knn_search_i8", "acx_knn_rescore"):
        assert re.search(r"ACX_API int %s\(" % name, header), name
        assert name in _ffi.SIGNATURES
        assert getattr(_ffi.lib(), name)
    assert re.search(r"#define ACX_KNN_I8_K 32\b", header) and _ffi.KNN_I8_K == 32


P = lambda v: None if v is None else ctypes.c_void_p(v)


def _quantize_rc(x=64, ld=8, inv=None, n=4, dim=8, codes=64, ld_c=32, scale=64, st=64):
    return _ffi.lib().acx_knn_quantize_i8(P(x), ld, P(inv), n, dim, P(codes), ld_c, P(scale), P(st), None)


def _search_rc(cq=64, ld_cq=None, sq=64, nq=4, cd=64, ld_cd=None, sd=64, n=16, dim=32, k=2, exclude=None, ind=64, sc=64, st=64, ws=256,
               ws_bytes=1 << 30):
    return _ffi.lib().acx_knn_search_i8(P(cq), dim if ld_cq is None else ld_cq, P(sq), nq, P(cd), dim if ld_cd is None else ld_cd, P(sd),
                                        n, dim, k, P(exclude), P(ind), P(sc), P(st), P(ws), ws_bytes, None)


def _rescore_rc(q=64, ld_q=8, rq=None, nq=4, d=64, ld_d=8, rd=None, n=16, dim=8, metric=0, cand=64, ld_cand=None, kc=8, k=2, ind=64,
                sc=64, st=64):
    return _ffi.lib().acx_knn_rescore(P(q), ld_q, P(rq), nq, P(d), ld_d, P(rd), n, dim, metric, P(cand), kc if ld_cand is None else ld_cand,
                                      kc, k, P(ind), P(sc), P(st), None)


def test_argument_errors_return_before_any_launch():
    """Made-up (never dereferenced) pointers: every argument error of the header's list is negative without a device."""
    lib = _ffi.lib()
    for kw in (dict(x=None), dict(codes=None), dict(scale=None), dict(st=None), dict(n=0), dict(dim=6), dict(dim=0),
               dict(dim=_ffi.KNN_MAX_DIM + 4), dict(ld=4), dict(ld=10), dict(x=68), dict(ld_c=16), dict(ld_c=40), dict(codes=72),
               dict(dim=36, ld=36, ld_c=48)):
        assert _quantize_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert _quantize_rc(n=(1 << 30) + 1) == -6
    for kw in (dict(dim=16), dict(dim=48), dict(dim=0), dict(dim=_ffi.KNN_MAX_DIM + 32), dict(ld_cq=16), dict(ld_cd=40), dict(ld_cd=16),
               dict(cq=None), dict(cd=None), dict(sq=None), dict(sd=None), dict(ind=None), dict(sc=None), dict(st=None), dict(ws=None),
               dict(cq=72), dict(cd=68), dict(k=0), dict(k=_ffi.KNN_MAX_K + 1), dict(k=17), dict(k=16, exclude=64), dict(nq=0),
               dict(n=0)):
        assert _search_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert _search_rc(ws_bytes=0) == -5
    assert _search_rc(ws=264) == -5
    assert _search_rc(n=(1 << 30) + 1) == -6
    assert b"dim = 48" in (_search_rc(dim=48), lib.acx_last_error())[1]
    for kw in (dict(k=9), dict(k=0), dict(kc=_ffi.KNN_MAX_K + 1, k=1), dict(kc=0), dict(q=None), dict(d=None), dict(cand=None),
               dict(ind=None), dict(sc=None), dict(st=None), dict(ld_cand=7), dict(metric=2), dict(metric=1), dict(metric=1, rq=64),
               dict(dim=6), dict(ld_q=4), dict(ld_d=10), dict(q=68), dict(nq=0), dict(n=0)):
        assert _rescore_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert _rescore_rc(n=(1 << 30) + 1) == -6
    assert b"k = 9" in (_rescore_rc(k=9), lib.acx_last_error())[1]


# ---- the Python API: errors raised before any device call --------------------------------------------------------------------------
def test_python_value_errors_need_no_device():
    e = np.zeros((5, 8), np.float32)
    with pytest.raises(ValueError, match="not cpu"):
        retrieval.QuantizedIndex(e, device="cpu")
    with pytest.raises(ValueError, match="metric"):
        retrieval.QuantizedIndex(e, metric="l2")
    with pytest.raises(ValueError, match="2-D"):
        retrieval.QuantizedIndex(np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="oversample"):
        retrieval.QuantizedIndex(e, oversample=0)
    # k * oversample > MAX_K is refused, and the message names both
    with pytest.raises(ValueError, match=r"k \* oversample = 33 \* 4 exceeds MAX_K = %d" % retrieval.MAX_K):
        retrieval.candidate_count(33, 4, 10 ** 6)
    assert retrieval.candidate_count(10, 4, 10 ** 6) == 40
    assert retrieval.candidate_count(32, 4, 10 ** 6) == retrieval.MAX_K
    assert retrieval.candidate_count(10, 4, 25) == 25
    with pytest.raises(ValueError, match="dim"):
        search_i8_host(np.zeros((2, 32), np.int8), np.ones(2), np.zeros((3, 64), np.int8), np.ones(3), 1)
    with pytest.raises(ValueError, match="k = 4"):
        search_i8_host(np.zeros((2, 32), np.int8), np.ones(2), np.zeros((3, 32), np.int8), np.ones(3), 4)
    with pytest.raises(ValueError, match="k = 3"):
        rescore_host(e, e, np.zeros((5, 2), np.int64), 3)
