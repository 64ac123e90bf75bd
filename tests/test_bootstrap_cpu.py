"""CPU: the host side of the bootstrap -- the draws of acx_bootstrap_weights stated in numpy (known answers, chunks, a loose
uniformity check), weighted_metrics_host against sklearn on resampled rows and with sample_weight, its NaN conventions, the
percentile and summary arithmetic of bootstrap_metrics on injected replicate arrays, the ctypes declarations of the new symbols
and their argument checks.  No device needed."""
import ctypes
import warnings

import numpy as np
import pytest
from sklearn import metrics as skm

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import metrics as M


def test_known_answer_draws():
    assert int(M._mix(7)[0]) == 0x12ae30237b17df14
    assert M.bootstrap_indices_host(0, 0, 1000)[:6].tolist() == [883, 431, 26, 970, 106, 327]
    assert M.bootstrap_indices_host(7, 3, 20371)[:6].tolist() == [6767, 6944, 9236, 12193, 15944, 14073]
    n = 1 << 30
    assert M.bootstrap_indices_host(2 ** 64 - 1, 2 ** 32 - 1, n, start=n - 3).tolist() == [468486541, 308690130, 853489832]
    idx = M.bootstrap_indices_host(7, 3, 20371)
    assert idx.dtype == np.int64 and idx.shape == (20371,) and idx.min() >= 0 and idx.max() < 20371
    assert np.array_equal(M.bootstrap_indices_host(7, 3, 20371, start=100, stop=200), idx[100:200])


def test_weights_sum_to_n_and_chunks():
    for n in (1, 2, 63, 1000):
        w = M.bootstrap_weights_host(7, 6, n)
        assert w.dtype == np.int32 and w.shape == (6, n) and (w >= 0).all()
        assert (w.sum(axis=1) == n).all()
        assert np.array_equal(w[2], np.bincount(M.bootstrap_indices_host(7, 2, n), minlength=n))
        assert np.array_equal(M.bootstrap_weights_host(7, 3, n, first=3), w[3:])
    assert not np.array_equal(M.bootstrap_weights_host(7, 1, 1000), M.bootstrap_weights_host(8, 1, 1000))
    for bad in (dict(seed=-1), dict(seed=2 ** 64), dict(replicates=0), dict(n=0), dict(n=2 ** 30 + 1), dict(first=2 ** 32 - 1)):
        args = dict(seed=0, replicates=2, n=10, first=0)
        args.update(bad)
        with pytest.raises(ValueError):
            M.bootstrap_weights_host(**args)


def test_draws_are_roughly_uniform():
    idx = np.concatenate([M.bootstrap_indices_host(1, r, 1000) for r in range(200)])
    count = np.bincount(idx, minlength=1000)
    chi2_df = ((count - 200.0) ** 2 / 200.0).sum() / 999.0
    assert 0.8 <= chi2_df <= 1.2, chi2_df


def sk_pair(y, s, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return skm.average_precision_score(y, s, **kw), skm.roc_auc_score(y, s, **kw)


@pytest.mark.parametrize("kind", ["continuous", "levels8"])
def test_weighted_metrics_host_against_sklearn(kind):
    rs = np.random.RandomState(0 if kind == "continuous" else 1)
    n, C, R = 300, 3, 12
    y = rs.uniform(size=(n, C)) < [0.1, 0.5, 0.03]
    y[0], y[1] = True, False
    s = rs.uniform(size=(n, C)).astype(np.float32) if kind == "continuous" else (rs.randint(0, 8, size=(n, C)) / 7.0).astype(np.float32)
    w = M.bootstrap_weights_host(7, R, n)
    got = M.weighted_metrics_host(y, s, w)
    assert all(got[k].shape == (R, C) and got[k].dtype == np.float64 for k in ("average_precision", "auc", "d_prime"))
    seen = 0
    for r in range(R):
        idx = M.bootstrap_indices_host(7, r, n)
        for c in range(C):
            if y[idx, c].sum() == 0:
                assert np.isnan([got[k][r, c] for k in got]).all()
                continue
            seen += 1
            ap_rows, auc_rows = sk_pair(y[idx, c], s[idx, c])
            ap_w, auc_w = sk_pair(y[:, c], s[:, c], sample_weight=w[r])
            assert abs(got["average_precision"][r, c] - ap_rows) <= 1e-12 and abs(got["average_precision"][r, c] - ap_w) <= 1e-12
            assert abs(got["auc"][r, c] - auc_rows) <= 1e-12 and abs(got["auc"][r, c] - auc_w) <= 1e-12
    assert seen >= R * (C - 1)
    # a single weight vector is one replicate; all-ones weights are the unweighted statistics
    one = M.weighted_metrics_host(y, s, np.ones(n, np.int64))
    assert one["auc"].shape == (1, C)
    for c in range(C):
        ap, auc = sk_pair(y[:, c], s[:, c])
        assert abs(one["average_precision"][0, c] - ap) <= 1e-12 and abs(one["auc"][0, c] - auc) <= 1e-12


def test_nan_conventions():
    s = np.array([[0.9, 0.2], [0.1, 0.4], [0.5, 0.6], [-0.0, 0.0]], np.float32)
    y = np.array([[1, 1], [0, 1], [1, 1], [0, 1]])
    w = np.array([[1, 1, 1, 1],       # class 0 defined, class 1 has no negatives
                  [0, 3, 0, 1],       # class 0: no positive drawn
                  [2, 0, 2, 0]])      # class 0: no negative drawn
    got = M.weighted_metrics_host(y, s, w)
    assert got["average_precision"][0, 0] == 1.0 and got["auc"][0, 0] == 1.0 and got["d_prime"][0, 0] == np.inf
    assert got["average_precision"][:, 1].tolist() == [1.0, 1.0, 1.0] and np.isnan(got["auc"][:, 1]).all()
    assert np.isnan(got["d_prime"][:, 1]).all()
    assert np.isnan([got[k][1, 0] for k in got]).all()                       # Pw = 0: everything NaN
    assert got["average_precision"][2, 0] == 1.0 and np.isnan(got["auc"][2, 0]) and np.isnan(got["d_prime"][2, 0])
    # signed zeros tie: a positive at -0.0 against a negative at +0.0 is half a win
    t = M.weighted_metrics_host(np.array([[1], [0]]), np.array([[-0.0], [0.0]], np.float32), np.array([1, 1]))
    assert t["auc"][0, 0] == 0.5 and t["d_prime"][0, 0] == 0.0 and t["average_precision"][0, 0] == 0.5
    worst = M.weighted_metrics_host(np.array([[0], [1]]), np.array([[0.9], [0.1]], np.float32), np.array([5, 2]))
    assert worst["auc"][0, 0] == 0.0 and worst["d_prime"][0, 0] == -np.inf
    for bad, match in ((np.array([1.0, 1.0]), "integers"), (np.array([1, -1]), "negative"), (np.array([2 ** 30, 1]), "2\\^30"),
                       (np.array([1, 1, 1]), "shape")):
        with pytest.raises(ValueError, match=match):
            M.weighted_metrics_host(np.array([[0], [1]]), np.array([[0.9], [0.1]], np.float32), bad)


def test_summary_and_percentile_arithmetic():
    nan, inf = np.nan, np.inf
    est = {"average_precision": np.array([0.5, nan, 1.0]), "auc": np.array([0.75, nan, nan]), "d_prime": np.array([1.0, nan, nan])}
    R = 41
    ap = np.stack([np.linspace(0.0, 1.0, R), np.full(R, nan), np.linspace(1.0, 0.5, R)], axis=1)
    auc = np.stack([np.linspace(0.5, 1.0, R), np.linspace(0.0, 1.0, R), np.full(R, nan)], axis=1)
    auc[::2, 1] = nan                                               # class 1 defined in the odd replicates only
    dp = np.stack([np.linspace(0.0, 4.0, R), np.full(R, 2.0), np.full(R, nan)], axis=1)
    dp[0, 1], dp[1, 1], dp[2, 1] = inf, -inf, nan                  # not finite: left out of the mean
    out = M.bootstrap_summary(est, {"average_precision": ap, "auc": auc, "d_prime": dp}, confidence=0.9, per_class=True)
    assert out["confidence"] == 0.9
    assert out["mAP"]["estimate"] == 0.75 and out["auc"]["estimate"] == 0.75 and out["d_prime"]["estimate"] == 1.0
    want_map = (ap[:, 0] + ap[:, 2]) / 2
    want_auc = np.where(np.isnan(auc[:, 1]), auc[:, 0], (auc[:, 0] + auc[:, 1]) / 2)
    want_dp = (dp[:, 0] + 2.0) / 2
    want_dp[:3] = dp[:3, 0]
    for name, want in (("mAP", want_map), ("auc", want_auc), ("d_prime", want_dp)):
        assert out[name]["replicates"].shape == (R,)
        np.testing.assert_allclose(out[name]["replicates"], want, rtol=0, atol=1e-15)
        low, high = np.quantile(want, [0.05, 0.95])
        assert abs(out[name]["low"] - low) <= 1e-15 and abs(out[name]["high"] - high) <= 1e-15
        assert out[name]["low"] <= out[name]["high"]
    cc = out["classes_counted"]
    assert cc.shape == (R, 3) and cc.dtype == np.int64
    assert (cc[:, 0] == 2).all() and cc[::2, 1].tolist() == [1] * 21 and cc[1::2, 1].tolist() == [2] * 20
    assert cc[:3, 2].tolist() == [1, 1, 1] and (cc[3:, 2] == 2).all()
    pc = out["per_class"]
    assert pc["average_precision"]["defined"].tolist() == [1.0, 0.0, 1.0]
    assert abs(pc["auc"]["defined"][1] - 20 / 41) <= 1e-15 and abs(pc["d_prime"]["defined"][1] - 38 / 41) <= 1e-15
    assert np.isnan(pc["average_precision"]["low"][1]) and np.isnan(pc["auc"]["high"][2])
    lo, hi = np.quantile(auc[1::2, 1], [0.05, 0.95])
    assert abs(pc["auc"]["low"][1] - lo) <= 1e-15 and abs(pc["auc"]["high"][1] - hi) <= 1e-15
    assert abs(pc["average_precision"]["low"][0] - 0.05) <= 1e-15 and abs(pc["average_precision"]["high"][0] - 0.95) <= 1e-15
    assert pc["d_prime"]["low"][1] == 2.0 and np.array_equal(pc["auc"]["estimate"], est["auc"], equal_nan=True)
    assert "per_class" not in M.bootstrap_summary(est, {"average_precision": ap, "auc": auc, "d_prime": dp})
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError, match="confidence"):
            M.bootstrap_summary(est, {"average_precision": ap, "auc": auc, "d_prime": dp}, confidence=bad)


def test_python_argument_errors_come_before_the_device():
    t, s = np.zeros((4, 2)), np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError, match="replicates"):
        M.bootstrap_metrics(t, s, replicates=0)
    with pytest.raises(ValueError, match="confidence"):
        M.bootstrap_metrics(t, s, confidence=1.5)
    with pytest.raises(ValueError, match="chunk"):
        M.bootstrap_metrics(t, s, chunk=0)
    with pytest.raises(ValueError, match="differs"):
        M.bootstrap_metrics(np.zeros((4, 3)), s)
    big = np.zeros((32769, 1), np.float32)
    with pytest.raises(ValueError, match="32768"):
        M.weighted_metrics(big, big, np.ones(32769, np.int32))
    with pytest.raises(ValueError, match="32768"):
        M.bootstrap_metrics(big, big)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_ffi_declarations_and_argument_checks():
    lib = _ffi.lib()
    for name in ("acx_bootstrap_weights", "acx_weighted_metrics_workspace_bytes", "acx_weighted_metrics"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert len(_ffi.SIGNATURES["acx_weighted_metrics"][1]) == 17 and len(_ffi.SIGNATURES["acx_bootstrap_weights"][1]) == 7
    assert _ffi.SIGNATURES["acx_bootstrap_weights"][1][:2] == [ctypes.c_uint64, ctypes.c_uint32]
    assert _ffi.METRICS_BAD_WEIGHT == 8 and _ffi.WEIGHTED_MAX_N == 32768
    ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -5, -6
    # argument errors come back before anything touches a device: the pointers below are never read
    fake = ctypes.c_void_p(4096)
    n, classes, R = 100, 7, 3
    need = _ffi.weighted_metrics_workspace_bytes(n, classes)
    assert need > _ffi.metrics_workspace_bytes(n, classes) and need % 256 == 0
    assert _ffi.weighted_metrics_workspace_bytes(32768, 527) >= _ffi.weighted_metrics_workspace_bytes(20371, 527)
    out = ctypes.c_size_t()
    assert lib.acx_weighted_metrics_workspace_bytes(n, classes, None) == ERR_ARG
    assert lib.acx_weighted_metrics_workspace_bytes(0, classes, ctypes.byref(out)) == ERR_ARG
    assert lib.acx_weighted_metrics_workspace_bytes(n, 0, ctypes.byref(out)) == ERR_ARG
    assert lib.acx_weighted_metrics_workspace_bytes(32769, classes, ctypes.byref(out)) == ERR_UNSUPPORTED
    assert b"32768" in lib.acx_last_error()

    def wm(scores=fake, ld_s=classes, target=fake, dtype=_ffi.TARGET_U8, ld_t=classes, n_=n, c_=classes, w=fake, ld_w=n, r_=R,
           ap=fake, auc=fake, dp=fake, status=fake, ws=fake, ws_bytes=need):
        return lib.acx_weighted_metrics(scores, ld_s, target, dtype, ld_t, n_, c_, w, ld_w, r_, ap, auc, dp, status, ws, ws_bytes, None)

    for null in ("scores", "target", "w", "ap", "auc", "dp", "status", "ws"):
        assert wm(**{null: None}) == ERR_ARG, null
        assert b"acx_weighted_metrics" in lib.acx_last_error()
    assert wm(n_=0) == ERR_ARG and wm(n_=-5) == ERR_ARG
    assert wm(c_=0) == ERR_ARG
    assert wm(ld_s=classes - 1) == ERR_ARG and wm(ld_t=classes - 1) == ERR_ARG
    assert wm(ld_w=n - 1) == ERR_ARG and b"stride" in lib.acx_last_error()
    assert wm(r_=0) == ERR_ARG and b"replicates" in lib.acx_last_error()
    assert wm(dtype=5) == ERR_ARG
    assert wm(n_=32769, ld_w=32769) == ERR_UNSUPPORTED and b"32768" in lib.acx_last_error()
    assert wm(ws_bytes=need - 256) == ERR_WORKSPACE and b"workspace" in lib.acx_last_error()
    assert wm(ws=ctypes.c_void_p(4096 + 8)) == ERR_WORKSPACE

    def bw(first=0, r_=R, n_=n, w=fake, ld_w=n):
        return lib.acx_bootstrap_weights(7, first, r_, n_, w, ld_w, None)

    assert bw(w=None) == ERR_ARG and b"acx_bootstrap_weights" in lib.acx_last_error()
    assert bw(r_=0) == ERR_ARG and bw(n_=0) == ERR_ARG and bw(ld_w=n - 1) == ERR_ARG
    assert bw(first=2 ** 32 - 2) == ERR_ARG and b"2^32" in lib.acx_last_error()
    assert bw(n_=2 ** 30 + 1, ld_w=2 ** 30 + 1) == ERR_UNSUPPORTED
