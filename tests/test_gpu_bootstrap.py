"""GPU (`-m gpu`): bootstrap weights and weighted per-class statistics on the device (acx_bootstrap_weights, acx_weighted_metrics,
pytorch/metrics.py) against their numpy definitions and sklearn's sample_weight computed live -- on ties, degenerate classes and
resamples that draw no positive, at every size class of the kernels, as the loop over resampled rows they replace, at the
AudioSet eval set's shape, on strided and differently typed inputs, through the status word, captured into a graph, and through
bootstrap_metrics / bootstrap_difference and the evaluation script.  Tolerances as test_gpu_metrics.py: AP and AUC within 1e-12,
d' to rtol 1e-10 where finite, NaN and infinity patterns equal exactly."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from sklearn import metrics as skm

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import metrics as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("average_precision", "auc", "d_prime")


def assert_matches(got, ref, tol=1e-12):
    for k in ("average_precision", "auc"):
        a, b = got[k], ref[k]
        assert a.dtype == np.float64 and a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.nanmax(np.abs(a - b), initial=0.0) <= tol, (k, np.nanmax(np.abs(a - b)))
    a, b = got["d_prime"], ref["d_prime"]
    assert a.shape == b.shape
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True)
    np.testing.assert_allclose(a[fin], b[fin], rtol=1e-10, atol=1e-12)


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in KEYS)


def tagging(target, scores):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return M.tagging_metrics(target, scores)


def tie_family(kind, N, C):
    rs = np.random.RandomState(["levels8", "saturated", "denormal", "shared"].index(kind))
    if kind == "levels8":
        s = (rs.randint(0, 8, size=(N, C)) / 7.0).astype(np.float32)
    elif kind == "saturated":
        s = rs.choice(np.array([0.0, -0.0, 1.0, 0.25], np.float32), size=(N, C), p=[0.3, 0.3, 0.3, 0.1])
    elif kind == "denormal":
        s = (rs.randint(-4, 5, size=(N, C)).astype(np.float32) * np.float32(1.4e-45)).astype(np.float32)
    else:
        s = np.full((N, C), 0.5, np.float32)
        s[rs.uniform(size=(N, C)) < 0.2] = 0.75
    t = rs.uniform(size=(N, C)) < rs.uniform(0.01, 0.9, size=C)
    t[0] = True
    t[1] = False
    return t, s


# ---- weights ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1025])
def test_weights_equal_the_host_bit_for_bit(n):
    host = M.bootstrap_weights_host(7, 5, n)
    dev = M.bootstrap_weights(5, n, seed=7)
    assert dev.dtype == torch.int32 and dev.is_cuda and tuple(dev.shape) == (5, n)
    assert np.array_equal(dev.cpu().numpy(), host)
    assert np.array_equal(M.bootstrap_weights(2, n, seed=7, first=3).cpu().numpy(), host[3:])      # a chunk computed alone
    # raw ABI, rows at a stride: what lies between the rows is left alone
    wide = torch.full((5, n + 3), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    _ffi.bootstrap_weights(7, 0, 5, n, vp(wide), n + 3, _ffi.stream_ptr(wide.device))
    w = wide.cpu().numpy()
    assert np.array_equal(w[:, :n], host) and (w[:, n:] == 0x7f7f7f7f).all()


# ---- weighted statistics ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["levels8", "saturated", "denormal", "shared"])
def test_weighted_against_host_and_sklearn(kind):
    N, C = 3000, 24
    t, s = tie_family(kind, N, C)
    rs = np.random.RandomState(9)
    sparse = np.where(rs.uniform(size=N) < 0.9, 0, rs.randint(1, 4, size=N)).astype(np.int32)     # many zeros
    heavy = np.ones(N, np.int32)
    heavy[rs.choice(N, size=5, replace=False)] = 100000                                            # a few rows dominate
    w = np.concatenate([M.bootstrap_weights_host(7, 8, N), sparse[None], heavy[None]])
    got = M.weighted_metrics(t, s, w)
    assert_matches(got, M.weighted_metrics_host(t, s, w))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in range(len(w)):
            for c in range(C):
                if w[r][t[:, c]].sum() == 0:
                    assert np.isnan([got[k][r, c] for k in KEYS]).all()
                    continue
                ap = skm.average_precision_score(t[:, c], s[:, c], sample_weight=w[r])
                auc = skm.roc_auc_score(t[:, c], s[:, c], sample_weight=w[r])
                assert abs(got["average_precision"][r, c] - ap) <= 1e-12, (r, c, got["average_precision"][r, c], ap)
                assert abs(got["auc"][r, c] - auc) <= 1e-12, (r, c, got["auc"][r, c], auc)


def test_all_ones_weights_equal_tagging_metrics():
    rs = np.random.RandomState(2)
    N, C = 500, 5
    s = rs.uniform(size=(N, C)).astype(np.float32)
    s[:, 4] = np.round(s[:, 4] * 10) / 10
    t = rs.uniform(size=(N, C)) < 0.3
    t[:, 0] = False
    t[:, 1] = True
    got = M.weighted_metrics(t, s, np.ones(N, np.int32))
    assert all(got[k].shape == (1, C) for k in KEYS)
    ref = tagging(t, s)
    assert ref["average_precision"][0] == 0.0
    ref["average_precision"][0] = np.nan                 # the documented difference: no positive, no statement
    assert_matches({k: got[k][0] for k in KEYS}, ref)
    assert got["average_precision"][0, 1] == 1.0 and np.isnan(got["auc"][0, 1])


def test_degenerate_classes():
    # n = 1: one positive class, one negative class
    t1, s1 = np.array([[1, 0]]), np.array([[0.3, 0.7]], np.float32)
    w1 = np.array([[1], [3], [0]])
    got = M.weighted_metrics(t1, s1, w1)
    assert_matches(got, M.weighted_metrics_host(t1, s1, w1))
    assert got["average_precision"][:, 0].tolist()[:2] == [1.0, 1.0] and np.isnan(got["average_precision"][2, 0])
    assert np.isnan(got["average_precision"][:, 1]).all() and np.isnan(got["auc"]).all() and np.isnan(got["d_prime"]).all()
    # n = 2, one positive above / below one negative
    t2, s2 = np.array([[1, 1], [0, 0]]), np.array([[0.9, 0.1], [0.2, 0.8]], np.float32)
    w2 = np.array([[1, 1], [0, 2], [2, 0], [0, 0], [5, 7]])
    got = M.weighted_metrics(t2, s2, w2)
    assert_matches(got, M.weighted_metrics_host(t2, s2, w2))
    assert got["auc"][:, 0].tolist()[0] == 1.0 and got["d_prime"][0, 0] == np.inf and got["d_prime"][0, 1] == -np.inf
    assert np.isnan([got[k][1, 0] for k in KEYS]).all() and np.isnan([got[k][3, 1] for k in KEYS]).all()
    assert got["average_precision"][2].tolist() == [1.0, 1.0] and np.isnan(got["auc"][2]).all()
    assert got["auc"][4].tolist() == [1.0, 0.0] and abs(got["average_precision"][4, 1] - 5.0 / 12.0) <= 1e-15
    # all positive; none positive
    rs = np.random.RandomState(3)
    s = rs.uniform(size=(200, 3)).astype(np.float32)
    t = rs.uniform(size=(200, 3)) < 0.3
    t[:, 0], t[:, 1] = True, False
    w = M.bootstrap_weights_host(3, 4, 200)
    got = M.weighted_metrics(t, s, w)
    assert_matches(got, M.weighted_metrics_host(t, s, w))
    assert (got["average_precision"][:, 0] == 1.0).all() and np.isnan(got["auc"][:, :2]).all()
    assert np.isnan(got["average_precision"][:, 1]).all() and np.isfinite(got["auc"][:, 2]).all()


def test_single_positive_is_drawn_or_not():
    rs = np.random.RandomState(4)
    N, R = 200, 16
    s = rs.uniform(size=(N, 2)).astype(np.float32)
    t = rs.uniform(size=(N, 2)) < 0.4
    t[:, 0] = False
    t[57, 0] = True                                       # exactly one positive
    w = M.bootstrap_weights_host(7, R, N)
    drawn = w[:, 57] > 0
    assert drawn.any() and (~drawn).any(), "the 16 resamples must show both outcomes (each has probability 0.63 / 0.37)"
    got = M.weighted_metrics(t, s, M.bootstrap_weights(R, N, seed=7))
    for k in KEYS:
        assert np.array_equal(np.isnan(got[k][:, 0]), ~drawn), k
        assert not np.isnan(got[k][:, 1]).any()
    assert_matches(got, M.weighted_metrics_host(t, s, w))


@pytest.mark.parametrize("n", [64, 65, 1024, 1025, 4097, 32768])
def test_sizes(n):
    rs = np.random.RandomState(n)
    C, R = 3, 3
    t = rs.uniform(size=(n, C)) < [0.02, 0.5, 0.97]
    t[0], t[1] = True, False
    s = (1.0 / (1.0 + np.exp(-(rs.standard_normal((n, C)) * 2 + 1.5 * t)))).astype(np.float32)
    s[:, 1] = np.round(s[:, 1] * 100) / 100
    w = M.bootstrap_weights_host(n, R, n)
    assert_matches(M.weighted_metrics(t, s, w), M.weighted_metrics_host(t, s, w))


def test_more_rows_than_the_limit_raise():
    big = torch.zeros((32769, 1), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="32768"):
        M.weighted_metrics(big, big, torch.ones(32769, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="32768"):
        M.bootstrap_metrics(big, big, replicates=2)
    with pytest.raises(_ffi.AcxError, match="32768"):
        _ffi.weighted_metrics_workspace_bytes(32769, 1)


def test_equals_the_loop_over_resampled_rows():
    rs = np.random.RandomState(5)
    N, C, R = 2000, 50, 20
    prev = np.concatenate([[0.0005, 0.001], rs.uniform(0.005, 0.6, size=C - 2)])
    t = rs.uniform(size=(N, C)) < prev
    t[:, 0] = False
    t[11, 0] = True                                       # one positive: some resamples miss it
    t[1] = False
    s = (1.0 / (1.0 + np.exp(-(rs.standard_normal((N, C)) * 2 + 2.0 * t)))).astype(np.float32)
    s[:, 7] = np.round(s[:, 7] * 20) / 20
    td, sd = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()
    got = M.weighted_metrics(td, sd, M.bootstrap_weights(R, N, seed=3))
    missed = 0
    for r in range(R):
        idx = torch.from_numpy(M.bootstrap_indices_host(3, r, N)).cuda()
        ref = tagging(td[idx], sd[idx])
        no_pos = t[idx.cpu().numpy()].sum(axis=0) == 0
        missed += int(no_pos.sum())
        assert (ref["average_precision"][no_pos] == 0.0).all()
        ref["average_precision"][no_pos] = np.nan         # the documented convention for Pw = 0
        assert_matches({k: got[k][r] for k in KEYS}, ref)
    assert missed >= 1, "the case Pw = 0 must occur"


def test_eval_set_shape_against_the_host():
    rs = np.random.RandomState(0)
    N, C, R = 20371, 527, 32
    prev = np.concatenate([[1.0 / N, (N - 1.0) / N], np.geomspace(2.0 / N, 0.999, C - 2)])
    t = rs.uniform(size=(N, C)) < prev
    t[:, 0] = False
    t[123, 0] = True                                     # the rarest: one positive
    t[:, 1] = True
    t[77, 1] = False                                     # the densest: one negative
    s = (1.0 / (1.0 + np.exp(-(rs.standard_normal((N, C)).astype(np.float32) * 3 + 2.0 * t)))).astype(np.float32)
    s[:, 300] = np.round(s[:, 300] * 50) / 50            # a tied class
    classes = np.concatenate([[0, 1, 300], np.random.RandomState(1).choice(np.arange(2, C), size=9, replace=False)])
    w = M.bootstrap_weights(R, N, seed=11)
    got = M.weighted_metrics(torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda(), w)
    assert got["auc"].shape == (R, C)
    ref = M.weighted_metrics_host(t[:, classes], s[:, classes], w.cpu().numpy())
    assert_matches({k: got[k][:, classes] for k in KEYS}, ref)
    assert np.isnan(got["auc"][:, 0]).any() and np.isfinite(got["auc"][:, 0]).any()


def test_strided_dtypes_and_host_or_device_inputs():
    rs = np.random.RandomState(6)
    N, C, R = 4000, 40, 4
    big_s = torch.from_numpy(rs.uniform(size=(N, C + 13)).astype(np.float32)).cuda()
    big_t = torch.from_numpy(rs.uniform(size=(N, C + 7)) < 0.2).cuda()
    big_w = torch.full((R, N + 9), -5, dtype=torch.int32, device="cuda")
    s, t, w = big_s[:, 5:5 + C], big_t[:, 3:3 + C], big_w[:, 4:4 + N]
    w.copy_(M.bootstrap_weights(R, N, seed=1))
    assert s.stride(0) == C + 13 and w.stride(0) == N + 9 and not w.is_contiguous()
    a = M.weighted_metrics(t, s, w)                                     # bool, everything strided
    assert_matches(a, M.weighted_metrics_host(t.cpu().numpy(), s.cpu().numpy(), w.cpu().numpy()))
    others = [M.weighted_metrics(t.to(torch.uint8), s, w),
              M.weighted_metrics(t.to(torch.float32), s.contiguous(), w.contiguous()),
              M.weighted_metrics(t.cpu().numpy(), s.cpu().numpy(), w.cpu().numpy().astype(np.int64)),
              M.weighted_metrics(t.cpu(), s.cpu(), w.to(torch.int64))]
    for b in others:
        assert same_bits(a, b)
    one = M.weighted_metrics(t, s, w[2])                                # (N,): one replicate
    assert all(one[k].shape == (1, C) and one[k][0].tobytes() == a[k][2].tobytes() for k in KEYS)


def test_bad_data_raises_through_the_status_word():
    rs = np.random.RandomState(7)
    N, C = 300, 9
    s = torch.from_numpy(rs.uniform(size=(N, C)).astype(np.float32)).cuda()
    t = torch.from_numpy((rs.uniform(size=(N, C)) < 0.5).astype(np.uint8)).cuda()
    w = M.bootstrap_weights(3, N, seed=2)
    s2 = s.clone()
    s2[17, 4] = float("nan")
    with pytest.raises(ValueError, match="NaN or infinite"):
        M.weighted_metrics(t, s2, w)
    t2 = t.clone()
    t2[5, 2] = 2
    with pytest.raises(ValueError, match="other than 0 and 1"):
        M.weighted_metrics(t2, s, w)
    w2 = w.clone()
    w2[1, 40] = -1
    with pytest.raises(ValueError, match="negative"):
        M.weighted_metrics(t, s, w2)
    w3 = w.clone()
    w3[2, 7] = 2 ** 30
    with pytest.raises(ValueError, match=r"2\^30"):
        M.weighted_metrics(t, s, w3)
    with pytest.raises(ValueError, match="negative"):
        M.weighted_metrics(t, s, w2.cpu().numpy())                     # host weights: checked before any copy
    with pytest.raises(ValueError, match="integers"):
        M.weighted_metrics(t, s, w.to(torch.float32))
    # the raw outputs of a data error are all NaN, and the status word names it
    n_ws = _ffi.weighted_metrics_workspace_bytes(N, C)
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
    out = torch.zeros((3, 3, C), dtype=torch.float64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.weighted_metrics(vp(s), C, vp(t), _ffi.TARGET_U8, C, N, C, vp(w2), N, 3, vp(out[0]), vp(out[1]), vp(out[2]), vp(st),
                          (vp(ws), n_ws), _ffi.stream_ptr(s.device))
    assert int(st.cpu()[0]) == _ffi.METRICS_BAD_WEIGHT and torch.isnan(out).all()
    _ffi.weighted_metrics(vp(s2), C, vp(t2), _ffi.TARGET_U8, C, N, C, vp(w), N, 3, vp(out[0]), vp(out[1]), vp(out[2]), vp(st),
                          (vp(ws), n_ws), _ffi.stream_ptr(s.device))
    assert int(st.cpu()[0]) == _ffi.METRICS_NONFINITE | _ffi.METRICS_BAD_TARGET and torch.isnan(out).all()


@pytest.fixture(scope="module")
def small():
    rs = np.random.RandomState(8)
    N, C = 700, 6
    t = rs.uniform(size=(N, C)) < [0.003, 0.05, 0.2, 0.5, 0.8, 0.3]
    t[0], t[1] = True, False
    a = (1.0 / (1.0 + np.exp(-(rs.standard_normal((N, C)) * 2 + 2.0 * t)))).astype(np.float32)
    b = (1.0 / (1.0 + np.exp(-(rs.standard_normal((N, C)) * 2 + 1.0 * t)))).astype(np.float32)
    return t, a, b


def test_determinism_and_chunks(small):
    t, a, _ = small
    w = M.bootstrap_weights(6, len(t), seed=5)
    assert same_bits(M.weighted_metrics(t, a, w), M.weighted_metrics(t, a, w))
    runs = [M.bootstrap_metrics(t, a, replicates=20, seed=5, chunk=chunk, per_class=True) for chunk in (1, 7, 256, 256)]
    for other in runs[1:]:
        for k in ("mAP", "auc", "d_prime"):
            assert other[k]["replicates"].tobytes() == runs[0][k]["replicates"].tobytes()
            assert (other[k]["estimate"], other[k]["low"], other[k]["high"]) == (runs[0][k]["estimate"], runs[0][k]["low"], runs[0][k]["high"])
        assert np.array_equal(other["classes_counted"], runs[0]["classes_counted"])
        for k in KEYS:
            for f in ("estimate", "low", "high", "defined"):
                assert other["per_class"][k][f].tobytes() == runs[0]["per_class"][k][f].tobytes()


def test_bootstrap_metrics_is_the_summary_of_its_parts(small):
    t, a, _ = small
    R = 20
    out = M.bootstrap_metrics(t, a, replicates=R, seed=5, confidence=0.9, per_class=True)
    reps = M.weighted_metrics(t, a, M.bootstrap_weights(R, len(t), seed=5))
    full = M.weighted_metrics(t, a, np.ones(len(t), np.int32))
    want = M.bootstrap_summary({k: full[k][0] for k in KEYS}, reps, confidence=0.9, per_class=True)
    for k in ("mAP", "auc", "d_prime"):
        assert out[k]["replicates"].shape == (R,) and out[k]["replicates"].tobytes() == want[k]["replicates"].tobytes()
        assert out[k]["low"] == want[k]["low"] and out[k]["high"] == want[k]["high"] and out[k]["estimate"] == want[k]["estimate"]
        assert out[k]["low"] <= out[k]["high"]
    ref = tagging(t, a)                                   # every class here has both labels: the plain means
    assert abs(out["mAP"]["estimate"] - ref["average_precision"].mean()) <= 1e-12
    assert abs(out["auc"]["estimate"] - ref["auc"].mean()) <= 1e-12
    assert out["classes_counted"].shape == (R, 3) and out["classes_counted"].max() == 6
    assert out["classes_counted"][:, 0].min() < 6, "class 0 has four positives: some resamples draw none"
    assert out["per_class"]["auc"]["defined"][0] < 1.0 and (out["per_class"]["auc"]["defined"][1:] == 1.0).all()
    assert out["seed"] == 5 and out["confidence"] == 0.9


def test_capture_and_replay_equals_eager(small):
    t, a, _ = small
    N, C, R = len(t), t.shape[1], 5
    s = torch.from_numpy(a).cuda()
    tg = torch.from_numpy(t.view(np.uint8)).cuda()
    w = M.bootstrap_weights(R, N, seed=9)
    eager = M.weighted_metrics(tg, s, w)
    n_ws = _ffi.weighted_metrics_workspace_bytes(N, C)
    ws = torch.full((n_ws,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((3, R, C), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    wcap = torch.zeros_like(w)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):                             # a linear graph: two clears and five kernels in a row
        _ffi.bootstrap_weights(9, 0, R, N, vp(wcap), N, _ffi.stream_ptr(s.device))
        _ffi.weighted_metrics(vp(s), C, vp(tg), _ffi.TARGET_U8, C, N, C, vp(wcap), N, R, vp(out[0]), vp(out[1]), vp(out[2]),
                              vp(st), (vp(ws), n_ws), _ffi.stream_ptr(s.device))
    torch.cuda.synchronize()
    assert float(out[0, 0, 0].cpu()) == 7.0               # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert int(st.cpu()[0]) == 0 and torch.equal(wcap, w)
    o = out.cpu().numpy()
    assert all(o[i].tobytes() == eager[k].tobytes() for i, k in enumerate(KEYS))


def test_bootstrap_difference(small):
    t, a, b = small
    same = M.bootstrap_difference(t, a, a, replicates=20, seed=4)
    for k in ("mAP", "auc", "d_prime"):
        assert same[k]["estimate"] == 0.0 and same[k]["low"] == 0.0 and same[k]["high"] == 0.0
        assert (same[k]["replicates"] == 0.0).all() and same[k]["fraction_a_greater"] == 0.0
    d = M.bootstrap_difference(t, a, b, replicates=20, seed=4, chunk=8)
    ra, rb = M.bootstrap_metrics(t, a, replicates=20, seed=4), M.bootstrap_metrics(t, b, replicates=20, seed=4)
    for k in ("mAP", "auc", "d_prime"):
        assert d[k]["replicates"].tobytes() == (ra[k]["replicates"] - rb[k]["replicates"]).tobytes()
        assert d[k]["estimate"] == ra[k]["estimate"] - rb[k]["estimate"]
        assert d[k]["low"] <= d[k]["high"]
        assert d[k]["fraction_a_greater"] == float(np.mean(d[k]["replicates"] > 0))
    assert d["mAP"]["fraction_a_greater"] == 1.0 and d["mAP"]["low"] > 0.0, "model a separates the classes twice as far"


def test_evaluate_script_bootstrap_flag():
    script = os.path.join(ROOT, "evaluate_convnext_on_audioset.py")
    plain = r"^Validate synthetic (?:mAP|AUC|d-prime): [0-9.\-]+$"
    ci = r"^Validate synthetic (mAP|AUC|d-prime) 95% CI: \[([0-9.\-]+), ([0-9.\-]+)\] \(50 resamples\)$"
    out = {}
    for flags in ((), ("--bootstrap", "50")):
        r = subprocess.run([sys.executable, script, "--synthetic", "2048", *flags], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out[flags] = r.stdout
    before, after = out[()], out[("--bootstrap", "50")]
    assert len(re.findall(plain, before, flags=re.M)) == 3 and "CI" not in before
    assert re.findall(plain, after, flags=re.M) == re.findall(plain, before, flags=re.M)
    found = re.findall(ci, after, flags=re.M)
    assert [f[0] for f in found] == ["mAP", "AUC", "d-prime"], after
    for _, low, high in found:
        assert float(low) <= float(high)
    strip = lambda text: [l for l in text.splitlines() if " CI: " not in l and not l.startswith("(")]
    assert strip(after) == strip(before)
    r = subprocess.run([sys.executable, script, "--synthetic", "8", "--bootstrap", "5", "--metrics", "sklearn"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "no bootstrap" in r.stderr
