"""GPU: Gaussian mixtures over embeddings (pytorch/mixture.py, acx_gmm_* in include/acx.h, csrc/mixture.hip) against the numpy
float64 host definitions: (1) ties in the E-step on integer inputs, (2) the E-step under the derived fp32 bound, (3) log-density
bits that do not depend on the shape, (4) the deterministic M-step, (5) the exact stop logic, (6) fitted models against the
float32-E-step yardstick, (7) the Python surface.  Shapes sit at the tile and tail boundaries of the kernels (64-row tiles, 64
components per wave, 256 per step, eight components per M-step wave, dim % 16), not at workload size.  The measured error / bound
and device / yardstick ratios go to profiles/mixture_error_over_bound.txt."""
import os
import warnings

import numpy as np
import pytest
import torch

import clustering_cases as cc
import mixture_cases as mc
from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import clustering, mixture, retrieval
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.mixture import GaussianMixture, estep_host, gmm, log_prob_host, mstep_host

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
case_id = mc.case_name
RECORD = {}                    # line key -> text, written to profiles/ when the module is done


@pytest.fixture(scope="module", autouse=True)
def error_over_bound_table():
    yield
    if not any(k.startswith("estep") for k in RECORD) or not any(k.startswith("fit") for k in RECORD):
        return                 # a partial run keeps the table of the last whole one
    head = ("Mixture tests (tests/test_gpu_mixture.py) on an MI355X.  estep: worst |lp_dev - lp_host| / b over the (row, component) pairs,\n"
            "b = tests/mixture_cases.py: lp_bound (the numpy float32 chain of tests/test_mixture_cpu.py reaches 0.03 to 0.10 of it).  fit:\n"
            "deviation from gmm_host (float64) after 5 iterations, device / float32-E-step yardstick, per quantity (allowed: 4; x/0: the\n"
            "yardstick does not deviate and the floor of 64 float64 ulp applies).\n\n")
    try:
        with open(os.path.join(ROOT, "profiles", "mixture_error_over_bound.txt"), "w") as f:
            f.write(head + "".join(RECORD[k] + "\n" for k in sorted(RECORD)))
    except OSError:
        pass


def dev_rows(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def d64(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def workspace(n, dim, K):
    nbytes = _ffi.gmm_workspace_bytes(n, dim, K)
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def dev_estep(x, w, mu, v, center=None, cov="diag", resp=True, labels=True, score=False):
    """acx_gmm_estep (score: acx_gmm_score) on device rows x -> (log_prob_norm, resp, labels, sum, status) as numpy / numbers."""
    n, dim = x.shape
    K = len(w)
    lpn = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    r = torch.full((n, K), 7.0, dtype=torch.float32, device=DEV) if resp and not score else None
    lab = torch.full((n,), -7, dtype=torch.int32, device=DEV) if labels else None
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws, nbytes = workspace(n, dim, K)
    cd, wd, md, vd = d64(center), d64(w), d64(mu), d64(v)                     # kept alive until the results are read
    args = (vp(x), x.stride(0), n, dim, vp(cd), vp(wd), vp(md), vp(vd), K, _ffi.GMM_COVARIANCES[cov], vp(lpn))
    if score:
        _ffi.gmm_score(*args, vp(lab), vp(total), vp(status), (vp(ws), nbytes), _ffi.stream_ptr(x.device))
    else:
        _ffi.gmm_estep(*args, vp(r), K, vp(lab), vp(total), vp(status), (vp(ws), nbytes), _ffi.stream_ptr(x.device))
    return (lpn.cpu().numpy(), None if r is None else r.cpu().numpy(), None if lab is None else lab.cpu().numpy(),
            float(total.cpu()[0]), int(status.cpu()[0]))


def dev_lp(x, w, mu, v, center=None, cov="diag"):
    """The device's log-densities (n, K) fp32, read one component at a time: with K = 1 the row's maximum is the log-density,
    s = expf(0) = 1 and log_prob_norm = m + logf(1) = m, and a pair's bits do not depend on K (test (3))."""
    out = np.empty((x.shape[0], len(w)), np.float32)
    for k in range(len(w)):
        lpn, r, lab, _, status = dev_estep(x, w[k:k + 1], mu[k:k + 1], v[k:k + 1], center, cov)
        assert status == 0 and (lab == 0).all() and (r == 1.0).all()
        out[:, k] = lpn
    return out


def dev_mstep(x, resp, center=None, reg=1e-6, cov="diag"):
    """acx_gmm_mstep on device rows x and a device resp tensor -> (weights, means, variances, nk, status)."""
    n, dim = x.shape
    K = resp.shape[1]
    w = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
    mu = torch.full((K, dim), 7.0, dtype=torch.float64, device=DEV)
    v = torch.full((K, dim) if cov == "diag" else (K,), 7.0, dtype=torch.float64, device=DEV)
    nk = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws, nbytes = workspace(n, dim, K)
    cd = d64(center)
    _ffi.gmm_mstep(vp(x), x.stride(0), n, dim, vp(cd), vp(resp), resp.stride(0), K, reg, _ffi.GMM_COVARIANCES[cov], vp(w),
                   vp(mu), vp(v), vp(nk), vp(status), (vp(ws), nbytes), _ffi.stream_ptr(x.device))
    return w.cpu().numpy(), mu.cpu().numpy(), v.cpu().numpy(), nk.cpu().numpy(), int(status.cpu()[0])


def dev_fit(x, w0, m0, v0, cov="diag", max_iter=100, tol=mc.TOL, reg=mc.REG):
    """acx_gmm_fit on device rows x -> dict of numpy arrays / numbers."""
    n, dim = x.shape
    K = len(w0)
    w, mu, v = d64(w0).clone(), d64(m0).clone(), d64(v0).clone()
    center = torch.full((dim,), 7.0, dtype=torch.float64, device=DEV)
    labels = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lpn = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    state = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    tol_d = torch.full((1,), float(tol), dtype=torch.float64, device=DEV)
    ws, nbytes = workspace(n, dim, K)
    _ffi.gmm_fit(vp(x), x.stride(0), n, dim, vp(w), vp(mu), vp(v), K, _ffi.GMM_COVARIANCES[cov], max_iter, vp(tol_d), reg, vp(center),
                 vp(labels), vp(lpn), vp(state), vp(status), (vp(ws), nbytes), _ffi.stream_ptr(x.device))
    words = state.view(torch.int32).cpu().numpy()
    st = state.cpu().numpy()
    return dict(weights=w.cpu().numpy(), means=mu.cpu().numpy(), variances=v.cpu().numpy(), center=center.cpu().numpy(),
                labels=labels.cpu().numpy(), lpn=lpn.cpu().numpy(), iterations=int(words[0]), done=int(words[1]),
                converged=int(words[2]), lower_bound=float(st[2]), change=float(st[3]), status=int(status.cpu()[0]))


# ---- (1) ties ------------------------------------------------------------------------------------------------------------------------
def tie_case(n, K, dim, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (n, dim)).astype(np.float32)
    if kind == "identical":
        base = 1
    else:
        base = max(1, (K + 2) // 3)
    mu = rng.integers(-4, 5, (base, dim)).astype(np.float64)[np.arange(K) % base]
    return x, np.full(K, 1.0 / K), mu, np.ones((K, dim)), base


TIES = ([(n, K, 768) for n in (1, 63, 64, 65, 257) for K in (1, 2, 63, 64, 65, 257)] + [(65, 65, d) for d in (4, 20, 772)]
        + [(65, 4096, 20)])


@pytest.mark.parametrize("n,K,dim", TIES)
def test_ties_go_to_the_lowest_index_and_copies_share_their_bits(n, K, dim):
    """Integer rows and means in -4 .. 4, unit variances, no centre: every product and sum of the contraction is exact, so copies of
    a component have EQUAL log-densities whatever lane, wave or step holds them."""
    for j, kind in enumerate(("identical", "duplicated")):
        x, w, mu, v, base = tie_case(n, K, dim, kind, 1000 * n + K + j)
        lpn, resp, lab, total, status = dev_estep(dev_rows(x), w, mu, v)
        assert status == 0
        lp = log_prob_host(x, w, mu, v)
        b = mc.lp_bound(x, w, mu, v)
        rows = np.arange(n)
        assert lab.min() >= 0 and lab.max() < base, kind                     # the lowest index among the copies
        assert (lp[rows, lab] + b[rows, lab] >= (lp - b).max(axis=1)).all()
        np.testing.assert_array_equal(resp.view(np.uint32), resp[:, np.arange(K) % base].view(np.uint32), err_msg=kind)
        assert (np.abs(resp.astype(np.float64).sum(axis=1) - 1.0) <= (K + 8) * 2.0 ** -24).all()
        assert not np.signbit(lpn[lpn == 0]).any() and np.isfinite(lpn).all()
        want = estep_host(x, w, mu, v)[0]
        assert (np.abs(lpn - want) <= b.max(axis=1) + mc.lpn_slack(K, want)).all()
        if kind == "identical":
            assert (lab == 0).all() and np.abs(resp - 1.0 / K).max() <= (K + 8) * 2.0 ** -24 / K + 2.0 ** -24
        assert abs(total - lpn.astype(np.float64).sum()) <= mc.total_slack(K, lpn)


# ---- (2) the E-step under the derived bound ----------------------------------------------------------------------------------------
def check_estep(tag, x, w, mu, v, center, cov="diag", lp_dev=None):
    """Everything acx_gmm_estep returns for one input against the host, under mixture_cases' bounds; -> worst error / bound."""
    n, K = x.shape[0], len(w)
    xd = dev_rows(x)
    lp = log_prob_host(x, w, mu, v, center)
    b = mc.lp_bound(x, w, mu, v, center)
    bmax = b.max(axis=1)
    worst = 0.0
    if lp_dev is None:
        lp_dev = dev_lp(xd, w, mu, v, center, cov)
    ratio = np.abs(lp_dev.astype(np.float64) - lp) / b
    worst = float(ratio.max())
    assert worst <= 1.0, tag
    lpn, resp, lab, total, status = dev_estep(xd, w, mu, v, center, cov)
    assert status == 0, tag
    want_lpn, want_resp, _ = mixture._estep_of(lp)
    assert (np.abs(lpn - want_lpn) <= bmax + mc.lpn_slack(K, want_lpn)).all(), tag
    assert (np.abs(resp - want_resp) <= mc.resp_bound(K, bmax)[:, None]).all(), tag
    assert (np.abs(resp.astype(np.float64).sum(axis=1) - 1.0) <= (K + 8) * 2.0 ** -24).all(), tag
    host, gap, _ = mc.margins(x, w, mu, v, center)
    decided = gap > 2 * bmax
    exempt = 1.0 - decided.mean()
    print("%s: error / bound %.3f, %.2f %% of the rows exempt from label equality" % (tag, worst, 100 * exempt))
    assert exempt <= 0.02, tag
    np.testing.assert_array_equal(lab[decided], host[decided], err_msg=tag)
    # the label is the arg-max of the device's own log-densities: first by value, then by index
    np.testing.assert_array_equal(lab, np.argmax(lp_dev + np.float32(0.0), axis=1), err_msg=tag)
    assert abs(total - lpn.astype(np.float64).sum()) <= mc.total_slack(K, lpn), tag
    # acx_gmm_score is the same call without resp
    lpn2, _, lab2, total2, status2 = dev_estep(xd, w, mu, v, center, cov, score=True)
    assert status2 == 0 and total2 == total, tag
    np.testing.assert_array_equal(lpn2.view(np.uint32), lpn.view(np.uint32), err_msg=tag)
    np.testing.assert_array_equal(lab2, lab, err_msg=tag)
    return worst


@pytest.mark.parametrize("case", mc.HARD + mc.SOFT, ids=case_id)
def test_estep_is_within_the_fp32_bound(case):
    x = mc.case_params(case)[0]
    center = np.float64(x).mean(axis=0)
    worst = 0.0
    for it in range(3):
        w, mu, v = mc.params_at(case, it)
        worst = max(worst, check_estep("%s it %d" % (case_id(case), it), x, w, mu, v, center))
    RECORD["estep %s" % case_id(case)] = "estep %-21s diag       iterations 0-2   error/bound %.3f" % (case_id(case), worst)


def test_estep_spherical_is_within_the_fp32_bound():
    case = mc.SOFT[1]
    x = mc.case_params(case)[0]
    w, mu, v = mc.params_at(case, 2, "spherical")
    worst = check_estep("spherical", x, w, mu, v, np.float64(x).mean(axis=0), "spherical")
    RECORD["estep spherical"] = "estep %-21s spherical  iteration 2      error/bound %.3f" % (case_id(case), worst)


@pytest.mark.parametrize("n,K,dim", mc.EDGES)
def test_estep_on_integer_cases(n, K, dim):
    """Integer blobs, variances in {1/2, 1, 2, 4}, unequal weights, no centre (mixture_cases.integer_case)."""
    x, w, mu, v = mc.integer_case(n, K, dim)
    worst = check_estep("n%d K%d dim%d" % (n, K, dim), x, w, mu, v, None)
    RECORD["estep int %03d %03d %03d" % (n, K, dim)] = "estep %-21s integers, no centre          error/bound %.3f" % ("n%d-d%d-k%d" % (n, dim, K), worst)


# ---- (3) shape-independence ----------------------------------------------------------------------------------------------------------
def test_log_density_bits_do_not_depend_on_the_shape():
    """A (row, component) pair has the same log-density bits whatever n, K and its place in the tiles.  Blobs 20 apart: every
    other component is more than 2^-25 below the winner, s = 1 and log_prob_norm IS the winner's log-density; one component alone
    (K = 1, where log_prob_norm is the log-density too) against its rows in reverse order gives the bits of the full call."""
    n, dim, K = 1001, 772, 33
    rng = np.random.default_rng(44)
    mu = rng.standard_normal((K, dim)) * 20.0
    own = rng.integers(0, K, n)
    x = np.float32(mu[own] + rng.standard_normal((n, dim)))
    v = rng.random((K, dim)) + 0.5
    w = np.full(K, 1.0 / K)
    center = np.float64(x).mean(axis=0)
    lpn, resp, lab, _, status = dev_estep(dev_rows(x), w, mu, v, center)
    assert status == 0
    np.testing.assert_array_equal(lab, own)
    assert (resp[np.arange(n), lab] == 1.0).all()
    for k in (0, 17, 32):
        rows = np.nonzero(lab == k)[0][::-1]
        assert rows.size
        l1, _, lab1, _, _ = dev_estep(dev_rows(x[rows]), w[k:k + 1], mu[k:k + 1], v[k:k + 1], center)
        assert (lab1 == 0).all()
        np.testing.assert_array_equal(l1.view(np.uint32), lpn[rows].view(np.uint32))
    # a row's outputs are a function of the row: the same rows further down in a longer call
    tail = np.concatenate([x[:70], x])
    l2, r2, lab2, _, _ = dev_estep(dev_rows(tail), w, mu, v, center)
    np.testing.assert_array_equal(l2[70:].view(np.uint32), lpn.view(np.uint32))
    np.testing.assert_array_equal(r2[70:].view(np.uint32), resp.view(np.uint32))
    np.testing.assert_array_equal(lab2[70:], lab)


# ---- (4) the M-step -------------------------------------------------------------------------------------------------------------------
MSTEP = [(1, 1, 4), (63, 2, 20), (65, 9, 772), (257, 33, 260), (1000, 8, 768), (300, 65, 20)]


@pytest.mark.parametrize("n,K,dim", MSTEP)
def test_mstep_equals_the_host_on_the_device_s_responsibilities(n, K, dim):
    rng = np.random.default_rng(5 * n + K)
    x = cc.blobs(n, dim, K, 0.2, n + K)[0]
    mu0 = x[rng.integers(0, n, K)].astype(np.float64)
    w0 = np.full(K, 1.0 / K)
    v0 = np.ones((K, dim)) * 2.0
    center = np.float64(x).mean(axis=0)
    xd = dev_rows(x)
    for c in (None, center):
        nK = len(w0)
        r = torch.empty((n, nK), dtype=torch.float32, device=DEV)
        lpn = torch.empty(n, dtype=torch.float32, device=DEV)
        total = torch.zeros(1, dtype=torch.float64, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws, nbytes = workspace(n, dim, K)
        cd, wd, md, vd = d64(c), d64(w0), d64(mu0), d64(v0)
        _ffi.gmm_estep(vp(xd), xd.stride(0), n, dim, vp(cd), vp(wd), vp(md), vp(vd), K, 0, vp(lpn), vp(r), K, None,
                       vp(total), vp(st), (vp(ws), nbytes), _ffi.stream_ptr(xd.device))
        resp = r.cpu().numpy()
        want_w, want_mu, want_v, want_nk = mstep_host(x, resp, 1e-6, "diag")
        bw, bm, bv = mc.mstep_bounds(x, resp, c)
        w, mu, v, nk, status = dev_mstep(xd, r, c)
        assert (np.abs(nk - want_nk) <= bw * n).all() and (np.abs(w - want_w) <= bw).all()
        assert (np.abs(mu - want_mu) <= bm).all()
        assert (np.abs(v - want_v) <= bv).all()
        assert bool(status & _ffi.GMM_DEGENERATE) == bool((want_nk < 1).any())
        # the same bits on every call
        w2, mu2, v2, nk2, _ = dev_mstep(xd, r, c)
        for a, b2 in ((w, w2), (mu, mu2), (v, v2), (nk, nk2)):
            np.testing.assert_array_equal(a.view(np.uint64), b2.view(np.uint64))
        # spherical: the mean of the diagonal variances
        ws_, mus, vs, _, _ = dev_mstep(xd, r, c, cov="spherical")
        np.testing.assert_array_equal(mus.view(np.uint64), mu.view(np.uint64))
        np.testing.assert_array_equal(ws_.view(np.uint64), w.view(np.uint64))
        assert (np.abs(vs - v.mean(axis=1)) <= (dim + 4) * 2.0 ** -53 * np.abs(v).mean(axis=1)).all()


def test_mstep_reads_a_strided_resp_and_flags_an_empty_component():
    n, K, dim = 130, 5, 20
    x = cc.blobs(n, dim, K, 1.0, 9)[0]
    rng = np.random.default_rng(2)
    resp = rng.random((n, K)).astype(np.float32)
    resp[:, 3] = 0.0                                             # nobody's component
    wide = torch.zeros((n, 8), dtype=torch.float32, device=DEV)
    wide[:, :K] = torch.from_numpy(resp).to(DEV)
    w, mu, v, nk, status = dev_mstep(dev_rows(x), wide[:, :K], None, 1e-3)
    assert status == _ffi.GMM_DEGENERATE
    want_w, want_mu, want_v, want_nk = mstep_host(x, resp, 1e-3)
    assert nk[3] == 10 * 2.0 ** -52 == want_nk[3] and w[3] == nk[3] / n
    assert (mu[3] == 0).all() and (v[3] == 1e-3).all()           # the formula's values: 0 / N, 0 - 0 + reg_covar
    bw, bm, bv = mc.mstep_bounds(x, resp)
    assert (np.abs(mu - want_mu) <= bm).all() and (np.abs(v - want_v) <= bv).all()


# ---- (5) the stop logic ----------------------------------------------------------------------------------------------------------------
def test_the_stop_is_decided_as_defined():
    case = mc.SOFT[1]
    x, w0, m0, v0 = mc.case_params(case)
    xd = dev_rows(x)
    a = dev_fit(xd, w0, m0, v0, max_iter=9, tol=1e30)
    assert a["status"] == 0 and a["iterations"] == 2 and a["done"] == 1 and a["converged"] == 1
    b = dev_fit(xd, w0, m0, v0, max_iter=2, tol=0.0)
    assert b["iterations"] == 2 and b["done"] == 0 and b["converged"] == 0
    for name in ("weights", "means", "variances", "center", "labels", "lpn"):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert a["lower_bound"] == b["lower_bound"] and a["change"] == b["change"]
    one = dev_fit(xd, w0, m0, v0, max_iter=1, tol=1e30)
    assert one["iterations"] == 1 and one["done"] == 0 and one["converged"] == 0 and one["change"] == np.inf
    assert a["change"] == a["lower_bound"] - one["lower_bound"]
    c = dev_fit(xd, w0, m0, v0, max_iter=7, tol=0.0)
    assert c["iterations"] == 7 and c["converged"] == 0 and c["done"] == 0
    # lower_bound is the mean log_prob_norm of the last iteration's E-step; labels and log_prob_norm belong to the result
    six = dev_fit(xd, w0, m0, v0, max_iter=6, tol=0.0)
    lpn, _, lab, total, _ = dev_estep(xd, six["weights"], six["means"], six["variances"], six["center"])
    assert c["lower_bound"] == total / x.shape[0] and c["change"] == c["lower_bound"] - six["lower_bound"]
    lpn7, _, lab7, _, _ = dev_estep(xd, c["weights"], c["means"], c["variances"], c["center"])
    np.testing.assert_array_equal(c["lpn"].view(np.uint32), lpn7.view(np.uint32))
    np.testing.assert_array_equal(c["labels"], lab7)
    center = np.float64(x).mean(axis=0)
    assert (np.abs(c["center"] - center) <= x.shape[0] * 2.0 ** -52 * np.abs(np.float64(x)).mean(axis=0)).all()


def test_non_finite_rows_stop_the_fit():
    x, w0, m0, v0 = mc.case_params(mc.SOFT[2])
    bad = x.copy()
    bad[7, 1] = np.nan
    f = dev_fit(dev_rows(bad), w0, m0, v0, max_iter=5)
    assert f["status"] & _ffi.GMM_NONFINITE and f["done"] == 1 and f["converged"] == 0 and f["iterations"] == 1
    z = dev_fit(dev_rows(x), np.array([0.5, 0.5, 0.0]), m0, v0, max_iter=5)        # log 0
    assert z["status"] & _ffi.GMM_NONFINITE and z["iterations"] == 1
    np.testing.assert_array_equal(z["means"], m0)                                   # stopped before the M-step


# ---- (6) fitted models -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cov", mc.NITER_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else v)
def test_fits_stop_where_the_host_stops(case, cov):
    x, w0, m0, v0 = mc.case_params(case)
    host = mc.host_fit(case, cov)
    f = dev_fit(dev_rows(x), w0, m0, mc.variances_of(v0, cov), cov)
    assert f["status"] & _ffi.GMM_NONFINITE == 0
    assert f["iterations"] == host.n_iter and f["converged"] == 1 and f["done"] == 1
    assert abs(f["lower_bound"] - host.lower_bound) <= 1e-3 * abs(host.lower_bound)


@pytest.mark.parametrize("cov", ["diag", "spherical"])
@pytest.mark.parametrize("case", mc.HARD + mc.SOFT + mc.SLOW, ids=case_id)
def test_fitted_parameters_deviate_like_the_float32_yardstick(case, cov):
    """tol = 0, five iterations: the device's deviation from gmm_host (float64) is at most 4 x that of gmm_host(estep_dtype=
    float32) -- two orders of the same fp32 rounding, not the same draw -- with a floor of 64 ulp of float64."""
    x, w0, m0, v0 = mc.case_params(case)
    f64, f32 = mc.host_fit(case, cov, False, 5, 0.0), mc.host_fit(case, cov, True, 5, 0.0)
    f = dev_fit(dev_rows(x), w0, m0, mc.variances_of(v0, cov), cov, max_iter=5, tol=0.0)
    assert f["status"] & _ffi.GMM_NONFINITE == 0 and f["iterations"] == 5
    ratios = []
    for name in ("weights", "means", "variances", "lower_bound"):
        ref = np.asarray(getattr(f64, name), np.float64)
        yard = float(np.abs(np.asarray(getattr(f32, name)) - ref).max())
        got = float(np.abs(np.asarray(f[name]) - ref).max())
        floor = 64 * 2.0 ** -52 * float(np.abs(ref).max())
        print("%s: device %.3e, yardstick %.3e" % (name, got, yard))
        ratios.append("%.2f" % (got / yard) if yard > 0 else "%.0e/0" % got)
        assert got <= max(4.0 * yard, floor), name
    RECORD["fit %s %s" % (case_id(case), cov)] = ("fit   %-21s %-9s  device/yardstick  weights %s  means %s  variances %s  lower_bound %s"
                                                 % ((case_id(case), cov) + tuple(ratios)))


# ---- (7) the Python surface ------------------------------------------------------------------------------------------------------------
def sk_model(gm):
    skm = pytest.importorskip("sklearn.mixture")
    g = skm.GaussianMixture(gm.components, covariance_type=gm.covariance_type)
    g.weights_, g.means_, g.covariances_ = gm.weights.cpu().numpy(), gm.means.cpu().numpy(), gm.variances.cpu().numpy()
    g.precisions_cholesky_ = 1.0 / np.sqrt(g.covariances_)
    return g


@pytest.mark.parametrize("cov", ["diag", "spherical"])
def test_scores_and_criteria_equal_sklearn_on_the_device_s_parameters(cov):
    x = cc.blobs(500, 64, 5, 0.4, 21)[0]
    y = cc.blobs(300, 64, 5, 0.4, 22)[0]
    gm = gmm(dev_rows(x), 5, covariance_type=cov, seed=3).check()
    g = sk_model(gm)
    w, mu, v, c = g.weights_, g.means_, g.covariances_, gm.center.cpu().numpy()
    bmax = mc.lp_bound(y, w, mu, v, c).max(axis=1)
    y64 = np.float64(y)
    want = g.score_samples(y64)
    got = gm.score_samples(dev_rows(y)).cpu().numpy()
    slack = bmax + mc.lpn_slack(5, want)
    assert (np.abs(got - want) <= slack).all()
    assert (np.abs(gm.predict_proba(dev_rows(y)).cpu().numpy() - g.predict_proba(y64)) <= mc.resp_bound(5, bmax)[:, None]).all()
    _, gap, _ = mc.margins(y, w, mu, v, c)
    decided = gap > 2 * bmax
    np.testing.assert_array_equal(gm.predict(dev_rows(y)).cpu().numpy()[decided], g.predict(y64)[decided])
    n = y.shape[0]
    assert abs(float(gm.score(dev_rows(y))) - g.score(y64)) <= slack.mean()
    assert abs(float(gm.bic(dev_rows(y))) - g.bic(y64)) <= 2 * slack.sum() + 1e-9 * abs(g.bic(y64))
    assert abs(float(gm.aic(dev_rows(y))) - g.aic(y64)) <= 2 * slack.sum() + 1e-9 * abs(g.aic(y64))
    assert torch.equal(gm.predict(dev_rows(x)), gm.labels) and gm.labels.dtype == torch.int64
    assert gm.weights.dtype == gm.means.dtype == gm.variances.dtype == gm.center.dtype == torch.float64
    assert gm.lower_bound.ndim == gm.n_iter.ndim == gm.converged.ndim == 0 and gm.converged.dtype == torch.bool
    assert tuple(gm.variances.shape) == ((5, 64) if cov == "diag" else (5,))


def test_kmeans_init_is_one_mstep_on_the_kmeans_labels():
    x = cc.blobs(600, 20, 4, 1.0, 31)[0]
    xd = dev_rows(x)
    a = gmm(xd, 4, seed=5, max_iter=30).check()
    km = clustering.kmeans(xd, 4, seed=5).check()
    onehot = np.eye(4)[km.labels.cpu().numpy()]
    w0, m0, v0, _ = mstep_host(x, onehot, 1e-6)
    b = gmm(xd, 4, init="params", weights_init=w0, means_init=m0, variances_init=v0, max_iter=30).check()
    assert int(a.n_iter) == int(b.n_iter) and bool(a.converged) == bool(b.converged)
    # the initial parameters agree within the M-step's float64 bound; 30 EM iterations contract towards the same fixed point
    for name in ("weights", "means", "variances"):
        np.testing.assert_allclose(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy(), rtol=1e-6, atol=1e-9, err_msg=name)
    assert torch.equal(a.labels, b.labels)


def test_n_init_keeps_the_highest_lower_bound():
    x = cc.blobs(400, 20, 6, 0.8, 41)[0]
    xd = dev_rows(x)
    singles = [gmm(xd, 6, seed=7 + i, max_iter=40) for i in range(3)]
    best = gmm(xd, 6, seed=7, n_init=3, max_iter=40).check()
    lbs = [float(s.lower_bound) for s in singles]
    win = singles[int(np.argmax(lbs))]
    assert float(best.lower_bound) == max(lbs)
    for name in ("weights", "means", "variances", "labels", "n_iter", "converged", "center"):
        assert torch.equal(getattr(best, name), getattr(win, name)), name


def test_save_and_load_round_trip(tmp_path):
    x = cc.blobs(300, 20, 3, 1.0, 51)[0]
    for cov in ("diag", "spherical"):
        gm = gmm(dev_rows(x), 3, covariance_type=cov).check()
        path = str(tmp_path / ("gm_%s.npz" % cov))
        gm.save(path)
        back = GaussianMixture.load(path)
        for name in ("weights", "means", "variances", "center", "lower_bound", "n_iter", "converged"):
            assert torch.equal(getattr(gm, name), getattr(back, name)), name
        assert back.covariance_type == cov and back.labels is None
        assert torch.equal(back.score_samples(dev_rows(x)), gm.score_samples(dev_rows(x)))
        assert torch.equal(back.predict(dev_rows(x)), gm.labels)
    km = clustering.kmeans(dev_rows(x), 3)
    km.save(str(tmp_path / "km.npz"))
    with pytest.raises(ValueError, match="not a Gaussian mixture"):
        GaussianMixture.load(str(tmp_path / "km.npz"))


def test_non_finite_rows_are_reported():
    x = cc.blobs(200, 20, 3, 1.0, 61)[0]
    gm = gmm(dev_rows(x), 3).check()
    y = x[:70].copy()
    y[3, 2] = np.inf
    y[66, 0] = np.nan
    lab = gm.predict(dev_rows(y)).cpu().numpy()
    assert lab[3] == -1 and lab[66] == -1 and (np.delete(lab, [3, 66]) >= 0).all()
    with pytest.raises(ValueError, match="NaN or infinite"):
        gm.check()
    bad = x.copy()
    bad[150, 5] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        gmm(dev_rows(bad), 3).check()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        gmm(dev_rows(x), 3).check()                                           # a clean fit warns about nothing
    with pytest.warns(RuntimeWarning, match="did not converge"):
        gmm(dev_rows(x), 3, max_iter=1).check()


def test_column_slices_are_read_in_place():
    x = cc.blobs(500, 24, 4, 2.0, 17)[0]
    wide = torch.zeros((500, 40), dtype=torch.float32, device=DEV)
    wide[:, 8:32] = dev_rows(x)
    view = wide[:, 8:32]
    assert retrieval._rows(view, view.device).data_ptr() == view.data_ptr()
    a = gmm(view, 4, seed=6).check()
    b = gmm(dev_rows(x), 4, seed=6).check()
    for name in ("weights", "means", "variances", "labels", "lower_bound", "n_iter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.predict(view), a.labels)


def test_whole_fit_in_a_graph():
    x = cc.blobs(700, 20, 5, 2.0, 13)[0]
    y = cc.blobs(700, 20, 5, 2.0, 14)[0]
    buf = dev_rows(x)
    m0 = d64(x[:5])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gmm(buf, 5, init="params", means_init=m0, max_iter=20)                # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = gmm(buf, 5, init="params", means_init=m0, max_iter=20)
    buf.copy_(dev_rows(y))
    g.replay()
    torch.cuda.synchronize()
    eager = gmm(dev_rows(y), 5, init="params", means_init=m0, max_iter=20).check()
    for name in ("weights", "means", "variances", "center", "labels", "lower_bound", "n_iter", "converged"):
        assert torch.equal(getattr(out, name), getattr(eager, name)), name
    assert int(eager.n_iter) >= 2


def test_select_components_takes_the_lowest_criterion():
    x = cc.blobs(600, 8, 3, 4.0, 71)[0]
    xd = dev_rows(x)
    for criterion in ("bic", "aic"):
        sel = mixture.select_components(xd, (1, 2, 3, 5), criterion=criterion, seed=2)
        host = []
        for k, gm in zip(sel.ks, sel.fits):
            lpn = estep_host(x, gm.weights.cpu().numpy(), gm.means.cpu().numpy(), gm.variances.cpu().numpy())[0]
            p = mixture.n_parameters(k, 8, "diag")
            host.append(-2.0 * lpn.sum() + (p * np.log(600) if criterion == "bic" else 2.0 * p))
        assert sel.best_k == sel.ks[int(np.argmin(host))]
        assert sel.best is sel.fits[sel.ks.index(sel.best_k)] and sel.criterion == criterion
        np.testing.assert_allclose(sel.scores.cpu().numpy(), host, rtol=1e-5)


def test_model_fit_gmm_and_select_components():
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    model.load_state_dict(synth.synth_state_dict(0))
    model = model.to(DEV).eval()
    wav = synth.synth_waveforms(40, 16000, seed=8)
    clips = [w for w in wav]
    gm = model.fit_gmm(clips, 2, max_iter=10)
    assert tuple(gm.means.shape) == (2, 768) and tuple(gm.labels.shape) == (40,) and gm.labels.min() >= 0
    emb = model._scene_rows(clips, None)
    again = model.fit_gmm(emb, 2, max_iter=10)
    assert torch.equal(gm.means, again.means) and torch.equal(gm.labels, again.labels)
    scores = gm.score_samples(emb)
    assert tuple(scores.shape) == (40,) and bool(torch.isfinite(scores).all())
    sel = model.select_components(emb, (1, 2), max_iter=10)
    assert sel.best_k in (1, 2) and tuple(sel.scores.shape) == (2,) and bool(torch.isfinite(sel.scores).all())
