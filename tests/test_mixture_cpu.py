"""CPU: Gaussian mixtures (pytorch/mixture.py; acx_gmm_* in include/acx.h) -- the numpy host definitions against scikit-learn's
GaussianMixture, the conditions the GPU tests rest on (the float32-E-step yardstick stops where float64 does, no stop decision is
close to tol, few rows have a label margin inside the rounding bound), and the host-only paths of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import mixture_cases as mc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import mixture
from audioset_convnext_inf_amd.pytorch.mixture import estep_host, gmm_host, log_prob_host, mstep_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acx_gmm_workspace_bytes", "acx_gmm_estep", "acx_gmm_score", "acx_gmm_mstep", "acx_gmm_fit")
COVS = ("diag", "spherical")
case_id = mc.case_name


def sk_model(weights, means, variances, cov):
    skm = pytest.importorskip("sklearn.mixture")
    g = skm.GaussianMixture(len(weights), covariance_type=cov)
    g.weights_, g.means_, g.covariances_ = weights, means, variances
    g.precisions_cholesky_ = 1.0 / np.sqrt(variances)
    return g


# ---- the host definitions against scikit-learn -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cov", COVS)
@pytest.mark.parametrize("case", mc.HARD + mc.SOFT + mc.SLOW, ids=case_id)
def test_gmm_host_equals_sklearn(case, cov):
    skm = pytest.importorskip("sklearn.mixture")
    x, w0, m0, v0 = mc.case_params(case)
    v = mc.variances_of(v0, cov)
    sk = skm.GaussianMixture(len(w0), covariance_type=cov, weights_init=w0, means_init=m0, precisions_init=1.0 / v, reg_covar=mc.REG,
                             tol=mc.TOL, max_iter=100).fit(np.float64(x))
    got = mc.host_fit(case, cov)
    assert got.n_iter == sk.n_iter_ and got.converged == sk.converged_
    for name, a, b in (("weights", got.weights, sk.weights_), ("means", got.means, sk.means_),
                       ("variances", got.variances, sk.covariances_), ("lower_bound", got.lower_bound, sk.lower_bound_)):
        rel = np.max(np.abs(a - b)) / np.max(np.abs(b))
        print("%s: %.2e" % (name, rel))
        assert rel <= 1e-9, name


@pytest.mark.parametrize("cov", COVS)
def test_scores_and_criteria_equal_sklearn(cov):
    case = mc.SOFT[1]
    x = mc.case_params(case)[0]
    f = mc.host_fit(case, cov)
    g = sk_model(f.weights, f.means, f.variances, cov)
    x64 = np.float64(x)
    lpn, resp, labels = estep_host(x, f.weights, f.means, f.variances)
    np.testing.assert_allclose(lpn, g.score_samples(x64), rtol=1e-10, atol=0)
    np.testing.assert_allclose(resp, g.predict_proba(x64), rtol=0, atol=1e-10)
    np.testing.assert_array_equal(labels, g.predict(x64))
    n, dim = x.shape
    p = mixture.n_parameters(len(f.weights), dim, cov)
    assert p == g._n_parameters()
    np.testing.assert_allclose(-2.0 * lpn.sum() + p * np.log(n), g.bic(x64), rtol=1e-12)
    np.testing.assert_allclose(-2.0 * lpn.sum() + 2.0 * p, g.aic(x64), rtol=1e-12)
    # the centre changes nothing but the rounding
    np.testing.assert_allclose(log_prob_host(x, f.weights, f.means, f.variances, x64.mean(axis=0)),
                               log_prob_host(x, f.weights, f.means, f.variances), rtol=1e-10)


def test_mstep_host_is_the_formula():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 8))
    r = rng.random((40, 3))
    r /= r.sum(axis=1)[:, None]
    w, mu, v, nk = mstep_host(x, r, 1e-3, "diag")
    for k in range(3):
        N = r[:, k].sum() + 10 * 2.0 ** -52
        assert abs(nk[k] - N) <= 40 * 2.0 ** -52 * N and w[k] == nk[k] / 40            # numpy's sum order along an axis differs
        m = (r[:, k, None] * x).sum(axis=0) / N
        np.testing.assert_allclose(mu[k], m, rtol=1e-13)
        np.testing.assert_allclose(v[k], (r[:, k, None] * (x - m) ** 2).sum(axis=0) / N + 1e-3, rtol=1e-11)
    ws, mus, vs, _ = mstep_host(x, r, 1e-3, "spherical")
    np.testing.assert_array_equal(vs, v.mean(axis=1))
    np.testing.assert_array_equal(mus, mu)


def test_first_argmax_and_ties():
    x = np.zeros((3, 4))
    mu = np.zeros((4, 4))
    _, resp, labels = estep_host(x, np.full(4, 0.25), mu, np.ones((4, 4)))
    assert (labels == 0).all() and (resp == resp[:, :1]).all() and np.abs(resp - 0.25).max() < 1e-15


# ---- the conditions the GPU tests rest on ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cov", mc.NITER_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else v)
def test_the_float32_yardstick_stops_where_float64_does(case, cov):
    f64, f32 = mc.host_fit(case, cov), mc.host_fit(case, cov, True)
    assert f64.converged and f32.converged and f64.n_iter == f32.n_iter
    for f in (False, True):
        ch = mc.host_changes(case, cov, f)
        gap = np.abs(ch - mc.TOL) / mc.TOL
        print("smallest ||change| - tol| / tol: %.3f" % gap.min())
        assert gap.min() >= 0.10


@pytest.mark.parametrize("case", mc.HARD + mc.SOFT, ids=case_id)
def test_few_rows_have_a_label_margin_inside_the_bound(case):
    x = mc.case_params(case)[0]
    center = np.float64(x).mean(axis=0)
    for it in range(3):
        w, m, v = mc.params_at(case, it)
        _, gap, bmax = mc.margins(x, w, m, v, center)
        share = float((gap <= 2 * bmax).mean())
        print("it %d: %.2f %% of the rows inside twice the bound" % (it, 100 * share))
        assert share <= 0.02


@pytest.mark.parametrize("n,K,dim", mc.EDGES)
def test_integer_cases_have_margins_outside_the_bound(n, K, dim):
    x, w, m, v = mc.integer_case(n, K, dim)
    _, gap, bmax = mc.margins(x, w, m, v)
    share = float((gap <= 2 * bmax).mean())
    print("%.2f %% of the rows inside twice the bound" % (100 * share))
    assert share <= 0.02


def test_the_float32_chain_stays_under_the_bound():
    """The numpy float32 chain (one order of the same roundings the device makes) against float64, under lp_bound."""
    for case in (mc.SOFT[0], mc.SOFT[2], mc.HARD[2]):
        x = mc.case_params(case)[0]
        center = np.float64(x).mean(axis=0)
        w, m, v = mc.params_at(case, 1)
        d = np.abs(log_prob_host(x, w, m, v, center, np.float32) - log_prob_host(x, w, m, v, center))
        ratio = float((d / mc.lp_bound(x, w, m, v, center)).max())
        print("%s: %.3f of the bound" % (case_id(case), ratio))
        assert ratio <= 1.0


# ---- the C ABI without a launch ----------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    for name in NAMES:
        assert re.search(r"ACX_API int %s\(" % name, header), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert _ffi.SIGNATURES[name][0] is ctypes.c_int
    assert [len(_ffi.SIGNATURES[k][1]) for k in NAMES] == [4, 19, 17, 18, 20]
    for name, value in (("ACX_GMM_NONFINITE", 1), ("ACX_GMM_DEGENERATE", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), header) and getattr(_ffi, name[4:]) == value
    assert "enum acx_gmm_covariance { ACX_GMM_DIAG = 0, ACX_GMM_SPHERICAL = 1 }" in header
    assert _ffi.GMM_COVARIANCES == {"diag": 0, "spherical": 1}
    assert re.search(r"int32_t iterations, done, converged, reserved;\s+double lower_bound, change;\s+} acx_gmm_state;", header)
    assert _ffi.GMM_STATE_BYTES == 32 and [f[0] for f in _ffi.AcxGmmState._fields_] == ["iterations", "done", "converged", "reserved",
                                                                                      "lower_bound", "change"]
    # the k-means status bit travels into a mixture's status word as it is
    assert _ffi.GMM_NONFINITE == _ffi.KMEANS_NONFINITE
    src = open(os.path.join(ROOT, "audioset-convnext-inf_amd", "csrc", "Makefile")).read()
    assert " mixture.hip" in src and src.count("build/acx/mixture.o") >= 1 and "and mixture.hip may run beside" in src
    flags = [l for l in src.splitlines() if "build/acx/mixture.o" in l]
    assert any(l.rstrip().endswith("CXXFLAGS += -fno-slp-vectorize") for l in flags)


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _estep_rc(x=64, ld_x=None, n=16, dim=8, center=64, w=64, mu=64, var=64, K=3, cov=0, lpn=64, resp=64, ld_r=None, labels=64, total=64,
              st=64, ws=256, ws_bytes=1 << 40):
    return _ffi.lib().acx_gmm_estep(_p(x), dim if ld_x is None else ld_x, n, dim, _p(center), _p(w), _p(mu), _p(var), K, cov, _p(lpn),
                                    _p(resp), K if ld_r is None else ld_r, _p(labels), _p(total), _p(st), _p(ws), ws_bytes, None)


def _score_rc(x=64, n=16, dim=8, center=64, w=64, mu=64, var=64, K=3, cov=0, lpn=64, labels=64, total=64, st=64, ws=256,
              ws_bytes=1 << 40):
    return _ffi.lib().acx_gmm_score(_p(x), dim, n, dim, _p(center), _p(w), _p(mu), _p(var), K, cov, _p(lpn), _p(labels), _p(total),
                                    _p(st), _p(ws), ws_bytes, None)


def _mstep_rc(x=64, ld_x=None, n=16, dim=8, center=64, resp=64, ld_r=None, K=3, reg=1e-6, cov=0, w=64, mu=64, var=64, nk=64, st=64,
              ws=256, ws_bytes=1 << 40):
    return _ffi.lib().acx_gmm_mstep(_p(x), dim if ld_x is None else ld_x, n, dim, _p(center), _p(resp), K if ld_r is None else ld_r, K,
                                    reg, cov, _p(w), _p(mu), _p(var), _p(nk), _p(st), _p(ws), ws_bytes, None)


def _fit_rc(x=64, ld_x=None, n=16, dim=8, w=64, mu=64, var=64, K=3, cov=0, max_iter=5, tol=64, reg=1e-6, center=64, labels=64, lpn=64,
            state=64, st=64, ws=256, ws_bytes=1 << 40):
    return _ffi.lib().acx_gmm_fit(_p(x), dim if ld_x is None else ld_x, n, dim, _p(w), _p(mu), _p(var), K, cov, max_iter, _p(tol), reg,
                                  _p(center), _p(labels), _p(lpn), _p(state), _p(st), _p(ws), ws_bytes, None)


BAD_COMMON = [dict(x=None), dict(x=68), dict(ld_x=6), dict(ld_x=4), dict(n=0), dict(n=(1 << 30) + 1), dict(dim=6), dict(dim=0),
              dict(dim=_ffi.KNN_MAX_DIM + 4), dict(K=0), dict(K=_ffi.KMEANS_MAX_CLUSTERS + 1), dict(cov=2), dict(cov=-1), dict(w=None),
              dict(mu=None), dict(var=None), dict(w=68), dict(st=None), dict(ws=None), dict(ws=260), dict(ws_bytes=64)]


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(center=68), dict(lpn=None), dict(total=None), dict(total=68), dict(ld_r=2)],
                         ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_estep_argument_errors_need_no_launch(bad):
    assert _estep_rc(**bad) < 0 and _ffi.lib().acx_last_error()
    if "ld_r" not in bad and "ld_x" not in bad:
        assert _score_rc(**bad) < 0


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(center=68), dict(resp=None), dict(ld_r=2), dict(reg=-1.0), dict(reg=float("nan")),
                                              dict(nk=None)], ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_mstep_argument_errors_need_no_launch(bad):
    assert _mstep_rc(**bad) < 0


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(max_iter=0), dict(max_iter=_ffi.KMEANS_MAX_ITER + 1), dict(tol=None), dict(tol=68),
                                              dict(reg=-1.0), dict(center=None), dict(labels=None), dict(lpn=None), dict(state=None),
                                              dict(state=68)], ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_fit_argument_errors_need_no_launch(bad):
    assert _fit_rc(**bad) < 0


def test_null_center_resp_and_labels_are_accepted_up_to_the_workspace():
    """NULL center / resp / labels pass the argument checks: the call fails only at the (too small) workspace."""
    rc = _estep_rc(center=None, resp=None, labels=None, ws_bytes=64)
    assert rc < 0 and b"workspace" in _ffi.lib().acx_last_error()


def test_workspace_bytes_is_monotone():
    f = _ffi.gmm_workspace_bytes
    ns = (1, 63, 64, 65, 4096, 4097, 100000, 1 << 20)
    dims = (4, 20, 768, 772, 1024, _ffi.KNN_MAX_DIM)
    ks = (1, 2, 63, 64, 65, 257, 1024, 4095, 4096)
    for dim in dims:
        for k in ks:
            vals = [f(n, dim, k) for n in ns]
            assert vals == sorted(vals), ("n", dim, k)
    for n in ns:
        for k in ks:
            vals = [f(n, dim, k) for dim in dims]
            assert vals == sorted(vals), ("dim", n, k)
        for dim in dims:
            vals = [f(n, dim, k) for k in ks]
            assert vals == sorted(vals), ("k", n, dim)
    assert f(1, 4, 1) % 256 == 0
    out = ctypes.c_size_t()
    for bad in ((0, 8, 3), (16, 6, 3), (16, 8, 0), (16, 8, _ffi.KMEANS_MAX_CLUSTERS + 1), ((1 << 30) + 1, 8, 3)):
        assert _ffi.lib().acx_gmm_workspace_bytes(*bad, ctypes.byref(out)) < 0
    assert _ffi.lib().acx_gmm_workspace_bytes(16, 8, 3, None) < 0


# ---- the Python surface's argument checks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(components=0), dict(components=2.0), dict(components=True), dict(components=41),
                                dict(covariance_type="full"), dict(covariance_type="tied"), dict(init="random"), dict(n_init=0),
                                dict(max_iter=0), dict(max_iter=_ffi.KMEANS_MAX_ITER + 1), dict(tol=-1.0), dict(tol=float("nan")),
                                dict(reg_covar=-1e-6)], ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_gmm_rejects_bad_arguments_before_touching_a_device(kw):
    args = dict(components=3)
    args.update(kw)
    with pytest.raises(ValueError):
        mixture.gmm(np.zeros((40, 8), np.float32), **args)


def test_gmm_rejects_bad_shapes():
    with pytest.raises(ValueError, match="2-D"):
        mixture.gmm(np.zeros(8, np.float32), 2)
    with pytest.raises(ValueError, match="multiple of 4"):
        mixture.gmm(np.zeros((40, 6), np.float32), 2)
    with pytest.raises(ValueError, match="criterion"):
        mixture.select_components(np.zeros((40, 8), np.float32), (2, 3), criterion="silhouette")
    with pytest.raises(ValueError, match="ks"):
        mixture.select_components(np.zeros((40, 8), np.float32), ())
    with pytest.raises(ValueError):
        log_prob_host(np.zeros((4, 8)), np.ones(2) / 2, np.zeros((2, 4)), np.ones((2, 4)))
    with pytest.raises(ValueError):
        gmm_host(np.zeros((4, 8)), np.ones(2) / 2, np.zeros((2, 8)), np.ones((2, 8)), "full")
