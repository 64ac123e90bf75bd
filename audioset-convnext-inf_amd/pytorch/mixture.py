"""Gaussian mixtures over embeddings on the GPU (acx_gmm_* in include/acx.h): EM with diagonal or spherical covariances -- what
`sklearn.mixture.GaussianMixture(covariance_type="diag" | "spherical").fit(emb)` does on the host: soft cluster memberships, a
density with more than one mode (the anomaly score of a clip), and a likelihood-based choice of the number of components.

    from audioset_convnext_inf_amd.pytorch.mixture import gmm, GaussianMixture, select_components
    gm = gmm(emb, components=16, covariance_type="diag", init="kmeans", n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0)
    gm.weights, gm.means, gm.variances        # (K,), (K, dim), (K, dim) or (K,) float64 device tensors
    gm.lower_bound, gm.n_iter, gm.converged   # 0-d device tensors
    gm.labels, gm.center                      # (n,) int64 of the fitted rows, (dim,) float64
    gm.predict(x), gm.predict_proba(x)        # labels / responsibilities of new rows
    gm.score_samples(x), gm.score(x)          # log-likelihood per row (the anomaly score) and its mean
    gm.bic(x), gm.aic(x)
    gm.check()                                # the one call that synchronises
    gm.save("gm.npz"); GaussianMixture.load("gm.npz")
    select_components(emb, ks=(2, 4, 8, 16), criterion="bic")

Full and tied covariances are not offered: reduce (and decorrelate) with `statistics.PCA(whiten=True)` first, then fit "diag".
The embedding dimension must be a multiple of 4 (a padded zero column would enter the density with variance reg_covar).

Arithmetic: the log-density of (row, component) is evaluated in the expanded form on rows centred by the column means,
sum xc^2 / v - 2 sum xc mc / v + sum mc^2 / v, the first two as ONE fp32 contraction of length 2 dim on the f32 matrix cores, the
last in float64 inside the per-component constant, which is added in float64 before the one rounding to fp32.  logsumexp and
the responsibilities are fp32; the M-step sums are float64 in a
fixed order with no float atomics, so the same inputs give the same bits.  The stop (|change of the mean log-likelihood| < tol,
scikit-learn's rule) is decided on the device: the host queues max_iter iterations and nothing synchronises, so a whole fit can
be captured in a torch.cuda.graph.

`log_prob_host`, `estep_host`, `mstep_host` and `gmm_host` are the documented host definitions in numpy float64 (the tests'
reference); `estep_dtype=np.float32` rounds the E-step's operands as the device does and is the yardstick of its rounding."""
import collections
import math
import warnings

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs
from . import retrieval

COVARIANCES = tuple(_ffi.GMM_COVARIANCES)
INITS = ("kmeans", "params")
CRITERIA = ("bic", "aic")
MAX_COMPONENTS = _ffi.KMEANS_MAX_CLUSTERS
MAX_ITER = _ffi.KMEANS_MAX_ITER
LOG_2PI = math.log(2.0 * math.pi)
NK_EPS = 10.0 * 2.0 ** -52


def _check_covariance(covariance_type):
    if covariance_type not in _ffi.GMM_COVARIANCES:
        raise ValueError("covariance_type must be one of %s, got %r" % (COVARIANCES, covariance_type))


def _check_components(components, n=None):
    if isinstance(components, bool) or not isinstance(components, (int, np.integer)) or not 1 <= components <= MAX_COMPONENTS:
        raise ValueError("components = %r (expected an integer in 1 .. %d)" % (components, MAX_COMPONENTS))
    if n is not None and components > n:
        raise ValueError("components = %d exceeds the %d rows" % (components, n))


def _check_max_iter(max_iter):
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 1 <= max_iter <= MAX_ITER:
        raise ValueError("max_iter = %r (expected an integer in 1 .. %d)" % (max_iter, MAX_ITER))


def _check_dim(dim):
    if dim < 4 or dim % 4 or dim > retrieval.MAX_DIM:
        raise ValueError("dim = %d (a mixture needs a multiple of 4 in 4 .. %d: drop or add real columns, or reduce with "
                         "statistics.PCA)" % (dim, retrieval.MAX_DIM))


def n_parameters(components, dim, covariance_type):
    """scikit-learn's count of free parameters: the covariances (K dim, or K), the means (K dim) and K - 1 weights."""
    _check_covariance(covariance_type)
    cov = components * dim if covariance_type == "diag" else components
    return int(cov + components * dim + components - 1)


# ---- the host definitions (numpy float64) ----------------------------------------------------------------------------------
def _operands(x, weights, means, variances, center):
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    mu = np.asarray(means, dtype=np.float64)
    v = np.asarray(variances, dtype=np.float64)
    n, dim = retrieval._check_2d(x, "x")
    if mu.ndim != 2 or mu.shape[1] != dim:
        raise ValueError("means have shape %s (expected (K, %d))" % (mu.shape, dim))
    K = mu.shape[0]
    if w.shape != (K,):
        raise ValueError("weights have shape %s (expected (%d,))" % (w.shape, K))
    if v.shape == (K,):
        v = np.repeat(v[:, None], dim, axis=1)
    if v.shape != (K, dim):
        raise ValueError("variances have shape %s (expected (%d, %d) or (%d,))" % (v.shape, K, dim, K))
    c = np.zeros(dim) if center is None else np.asarray(center, dtype=np.float64)
    xt, mt = x - c[None, :], mu - c[None, :]
    a, b = 1.0 / v, mt / v
    with np.errstate(divide="ignore"):
        cst = np.log(w) - 0.5 * (dim * LOG_2PI + np.log(v).sum(axis=1) + (mt * mt * a).sum(axis=1))
    return xt, a, b, cst


def log_prob_host(x, weights, means, variances, center=None, dtype=np.float64):
    """lp (n, K) float64: lp[i, k] = log w_k - (dim log 2 pi + sum_d log v_kd + sum_d (x_id - mu_kd)^2 / v_kd) / 2, in the expanded
    form on centred rows: with xc = x - center, mc = mu - center, a = 1 / v, b = mc / v the quadratic part is sum xc^2 a -
    2 sum xc b + sum mc^2 a, the last inside the per-component constant.  variances (K, dim), or (K,) for spherical.
    dtype=np.float32: xc^2, xc, a, -2 b and the constant are rounded to float32 and the 2 dim products are summed by one
    sequential float32 running sum (the yardstick of the device's rounding, not its bits; the device keeps the constant in
    float64 and rounds cst - D / 2 once)."""
    xt, a, b, cst = _operands(x, weights, means, variances, center)
    if np.dtype(dtype) == np.float64:
        return cst[None, :] - 0.5 * ((xt * xt) @ a.T - 2.0 * (xt @ b.T))
    if np.dtype(dtype) != np.float32:
        raise ValueError("dtype must be numpy float64 or float32, got %r" % (dtype,))
    A = np.concatenate([xt * xt, xt], axis=1).astype(np.float32)
    B = np.concatenate([a, -2.0 * b], axis=1).astype(np.float32)
    c32 = cst.astype(np.float32)
    lp = np.empty((A.shape[0], B.shape[0]))
    for k in range(B.shape[0]):
        q = np.cumsum(A * B[k][None, :], axis=1, dtype=np.float32)[:, -1]
        lp[:, k] = c32[k].astype(np.float64) - 0.5 * q.astype(np.float64)
    return lp


def _estep_of(lp):
    lp = lp + 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        m = lp.max(axis=1)
        lpn = m + np.log(np.exp(lp - m[:, None]).sum(axis=1))
        resp = np.exp(lp - lpn[:, None])
    return lpn, resp, np.argmax(lp, axis=1).astype(np.int64)


def estep_host(x, weights, means, variances, center=None, dtype=np.float64):
    """(log_prob_norm (n,), resp (n, K), labels (n,) int64): the logsumexp of log_prob_host over the components, the
    responsibilities exp(lp - log_prob_norm), and the first arg-max of lp (lowest component index among equal values, -0.0 as
    +0.0)."""
    return _estep_of(log_prob_host(x, weights, means, variances, center, dtype))


def mstep_host(x, resp, reg_covar=1e-6, covariance_type="diag"):
    """scikit-learn's M-step -> (weights (K,), means (K, dim), variances (K, dim) or (K,), N_k (K,)): N_k = sum_i r_ik + 10 * 2^-52,
    mu_k = sum r x / N_k, v_kd = sum r x^2 / N_k - mu_kd^2 + reg_covar (spherical: the mean over d), w_k = N_k / n."""
    _check_covariance(covariance_type)
    x = np.asarray(x, dtype=np.float64)
    r = np.asarray(resp, dtype=np.float64)
    n = retrieval._check_2d(x, "x")[0]
    if r.ndim != 2 or r.shape[0] != n:
        raise ValueError("resp has shape %s (expected (%d, K))" % (r.shape, n))
    nk = r.sum(axis=0) + NK_EPS
    mu = (r.T @ x) / nk[:, None]
    v = (r.T @ (x * x)) / nk[:, None] - mu * mu + reg_covar
    if covariance_type == "spherical":
        v = v.mean(axis=1)
    return nk / n, mu, v, nk


HostGMM = collections.namedtuple("HostGMM", "weights means variances lower_bound n_iter converged lower_bounds")


def gmm_host(x, weights0, means0, variances0, covariance_type="diag", max_iter=100, tol=1e-3, reg_covar=1e-6,
             estep_dtype=np.float64):
    """scikit-learn's EM loop -> HostGMM (lower_bounds: that of every iteration).  Each iteration is estep_host (on rows centred by the column means, in estep_dtype),
    then mstep_host; lower_bound is the mean log_prob_norm of that E-step, and the loop has converged when |lower_bound - the
    previous one| < tol (the first change is +inf)."""
    _check_covariance(covariance_type)
    _check_max_iter(max_iter)
    x = np.asarray(x, dtype=np.float64)
    w = np.array(weights0, dtype=np.float64)
    mu = np.array(means0, dtype=np.float64)
    v = np.array(variances0, dtype=np.float64)
    center = x.mean(axis=0)
    lower, converged, n_iter, history = -np.inf, False, 0, []
    for it in range(max_iter):
        prev = lower
        lpn, resp, _ = estep_host(x, w, mu, v, center, estep_dtype)
        w, mu, v, _ = mstep_host(x, resp, reg_covar, covariance_type)
        lower = float(lpn.mean())
        history.append(lower)
        n_iter = it + 1
        if abs(lower - prev) < tol:
            converged = True
            break
    return HostGMM(w, mu, v, lower, n_iter, converged, tuple(history))


# ---- the device path -------------------------------------------------------------------------------------------------------
class GaussianMixture:
    """The result of gmm(): device tensors, nothing synchronised.  weights (K,), means (K, dim), variances (K, dim) ("diag") or
    (K,) ("spherical") float64; center (dim,) float64, the column means of the fitted rows; lower_bound (float64), n_iter (int32)
    and converged (bool) as 0-d tensors; labels (n,) int64 of the fitted rows (None for a loaded model)."""

    def __init__(self, weights, means, variances, covariance_type, center, lower_bound, n_iter, converged, labels=None,
                 status=None):
        _check_covariance(covariance_type)
        self.weights, self.means, self.variances = weights, means, variances
        self.covariance_type, self.center = covariance_type, center
        self.lower_bound, self.n_iter, self.converged, self.labels = lower_bound, n_iter, converged, labels
        self.device = means.device
        self._status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=self.device)

    @property
    def components(self):
        return self.means.shape[0]

    def _estep(self, x, want_resp):
        K, dim = self.means.shape
        x = retrieval._rows(x, self.device, dim, "x")
        n, dev = x.shape[0], self.device
        lpn = torch.empty(n, dtype=torch.float32, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        resp = torch.empty((n, K), dtype=torch.float32, device=dev) if want_resp else None
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        if n:
            word = torch.empty(1, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                nbytes = _ffi.gmm_workspace_bytes(n, dim, K)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _ffi.gmm_estep(vp(x), x.stride(0), n, dim, vp(self.center), vp(self.weights), vp(self.means), vp(self.variances), K,
                               _ffi.GMM_COVARIANCES[self.covariance_type], vp(lpn), vp(resp), K, vp(labels), vp(total), vp(word),
                               (vp(ws), nbytes), _ffi.stream_ptr(dev))
            self._status.bitwise_or_(word & _ffi.GMM_NONFINITE)
        return n, lpn, resp, labels, total[0]

    def predict(self, x):
        """(rows,) int64: the component of the highest log-density of each row of x (rows, dim); -1 for a non-finite row."""
        return self._estep(x, False)[3].to(torch.int64)

    def predict_proba(self, x):
        """(rows, K) fp32: the responsibilities of each row."""
        return self._estep(x, True)[2]

    def score_samples(self, x):
        """(rows,) fp32: the log-likelihood of each row under the mixture -- low for an unusual row."""
        return self._estep(x, False)[1]

    def score(self, x):
        """0-d float64: the mean log-likelihood per row."""
        n, _, _, _, total = self._estep(x, False)
        return total / max(n, 1)

    def _criterion(self, x, penalty):
        n, _, _, _, total = self._estep(x, False)
        return -2.0 * total + penalty(max(n, 1)) * n_parameters(self.components, self.means.shape[1], self.covariance_type)

    def bic(self, x):
        """0-d float64: -2 log-likelihood + (free parameters) log(rows), scikit-learn's count for "diag" and "spherical"."""
        return self._criterion(x, math.log)

    def aic(self, x):
        """0-d float64: -2 log-likelihood + 2 (free parameters)."""
        return self._criterion(x, lambda n: 2.0)

    def check(self):
        """Synchronise: ValueError if a log-density was not finite (NaN or infinite values in the rows, a zero weight or
        variance); RuntimeWarning (warnings.warn) for a component that held less than one row's weight in some iteration, or a
        fit that used up max_iter."""
        st = int(self._status.cpu()[0])
        if st & _ffi.GMM_NONFINITE:
            raise ValueError("the embeddings or the parameters gave NaN or infinite log-densities")
        if st & _ffi.GMM_DEGENERATE:
            warnings.warn("a component collapsed (N_k < 1): fewer components, or a larger reg_covar", RuntimeWarning)
        if not bool(self.converged.cpu()):
            warnings.warn("EM did not converge in %d iterations" % int(self.n_iter.cpu()), RuntimeWarning)
        return self

    def save(self, path):
        np.savez(path, method="gmm", covariance_type=self.covariance_type, weights=self.weights.cpu().numpy(),
                 means=self.means.cpu().numpy(), variances=self.variances.cpu().numpy(), center=self.center.cpu().numpy(),
                 lower_bound=self.lower_bound.cpu().numpy(), n_iter=self.n_iter.cpu().numpy(),
                 converged=self.converged.cpu().numpy())

    @classmethod
    def load(cls, path, device=None):
        dev = _inputs.cuda_device(device, "a mixture is applied on")
        with np.load(path) as f:
            if str(f["method"]) != "gmm":
                raise ValueError("%s holds %s, not a Gaussian mixture" % (path, f["method"]))
            cov = str(f["covariance_type"])
            weights, means, variances, center = f["weights"], f["means"], f["variances"], f["center"]
            lower_bound, n_iter, converged = f["lower_bound"], f["n_iter"], f["converged"]
        _check_covariance(cov)
        if means.ndim != 2 or not np.isfinite(means).all():
            raise ValueError("%s: means must be a finite (K, dim) array" % path)
        K, dim = means.shape
        if weights.shape != (K,) or center.shape != (dim,) or variances.shape != ((K, dim) if cov == "diag" else (K,)):
            raise ValueError("%s: weights, variances or center do not fit the (%d, %d) means" % (path, K, dim))
        t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(dev).contiguous()
        return cls(t(weights, torch.float64), t(means, torch.float64), t(variances, torch.float64), cov, t(center, torch.float64),
                   t(lower_bound, torch.float64), t(n_iter, torch.int32), t(converged, torch.bool))


def _param(a, shape, name, dev):
    if tuple(getattr(a, "shape", ())) != shape:
        raise ValueError("%s has shape %s (expected %s)" % (name, tuple(getattr(a, "shape", ())), shape))
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return a.detach().to(device=dev, dtype=torch.float64).contiguous().clone()


def _column_variances(x, dim):
    n = x.shape[0]
    s1 = torch.zeros(dim, dtype=torch.float64, device=x.device)
    s2 = torch.zeros(dim, dtype=torch.float64, device=x.device)
    for a in range(0, n, 16384):
        chunk = x[a:a + 16384, :dim].to(torch.float64)
        s1 += chunk.sum(dim=0)
        s2 += (chunk * chunk).sum(dim=0)
    return (s2 / n - (s1 / n) ** 2).clamp_min(0.0)


def _check_fit_args(shape, components, covariance_type, init, n_init, max_iter, tol, reg_covar):
    _check_covariance(covariance_type)
    _check_components(components, shape[0])
    _check_dim(shape[1])
    _check_max_iter(max_iter)
    if init not in INITS:
        raise ValueError("init must be one of %s, got %r" % (INITS, init))
    if isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or n_init < 1:
        raise ValueError("n_init = %r (expected an integer >= 1)" % (n_init,))
    if not tol >= 0:
        raise ValueError("tol = %r (expected >= 0)" % (tol,))
    if not reg_covar >= 0:
        raise ValueError("reg_covar = %r (expected >= 0)" % (reg_covar,))


def _fit_rows(x, components, covariance_type="diag", init="kmeans", n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0,
              weights_init=None, means_init=None, variances_init=None):
    """gmm() on rows the kernels can read: x (n, dim) fp32 on the device, dim a multiple of 4."""
    from . import clustering
    n, dim = x.shape
    dev = x.device
    K = int(components)
    code = _ffi.GMM_COVARIANCES[covariance_type]
    vshape = (K, dim) if covariance_type == "diag" else (K,)
    if init == "params":
        if means_init is None:
            raise ValueError('init="params" needs means_init')
        n_init = 1
    elif weights_init is not None or means_init is not None or variances_init is not None:
        raise ValueError('weights_init, means_init and variances_init go with init="params"')
    with torch.cuda.device(dev):
        stream = _ffi.stream_ptr(dev)
        nbytes = _ffi.gmm_workspace_bytes(n, dim, K)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tol_dev = torch.full((1,), float(tol), dtype=torch.float64, device=dev)
        best = None
        for run in range(int(n_init)):
            init_status = torch.zeros(1, dtype=torch.int32, device=dev)
            if init == "params":
                means = _param(means_init, (K, dim), "means_init", dev)
                weights = (torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev) if weights_init is None
                           else _param(weights_init, (K,), "weights_init", dev))
                if variances_init is None:
                    cv = _column_variances(x, dim) + float(reg_covar)
                    variances = (cv[None, :].repeat(K, 1) if covariance_type == "diag" else cv.mean().repeat(K)).contiguous()
                else:
                    variances = _param(variances_init, vshape, "variances_init", dev)
            else:
                km = clustering.kmeans(x, K, seed=seed + run, device=dev)
                resp = (km.labels[:, None] == torch.arange(K, device=dev)[None, :]).to(torch.float32)
                weights = torch.empty(K, dtype=torch.float64, device=dev)
                means = torch.empty((K, dim), dtype=torch.float64, device=dev)
                variances = torch.empty(vshape, dtype=torch.float64, device=dev)
                nk = torch.empty(K, dtype=torch.float64, device=dev)
                _ffi.gmm_mstep(vp(x), x.stride(0), n, dim, None, vp(resp), K, K, reg_covar, code, vp(weights), vp(means),
                               vp(variances), vp(nk), vp(init_status), (vp(ws), nbytes), stream)
                init_status = init_status | (km._status & _ffi.KMEANS_NONFINITE)       # the same bit as GMM_NONFINITE
            center = torch.empty(dim, dtype=torch.float64, device=dev)
            labels = torch.empty(n, dtype=torch.int32, device=dev)
            lpn = torch.empty(n, dtype=torch.float32, device=dev)
            state = torch.zeros(4, dtype=torch.float64, device=dev)                  # struct acx_gmm_state
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _ffi.gmm_fit(vp(x), x.stride(0), n, dim, vp(weights), vp(means), vp(variances), K, code, int(max_iter), vp(tol_dev),
                         reg_covar, vp(center), vp(labels), vp(lpn), vp(state), vp(status), (vp(ws), nbytes), stream)
            status = status | init_status
            cur = [weights, means, variances, center, labels, state, status]
            if best is None:
                best = cur
            else:
                better = cur[5][2] > best[5][2]                                      # a NaN lower bound never wins
                best = [torch.where(better, c, b) for c, b in zip(cur, best)]
        weights, means, variances, center, labels, state, status = best
        words = state.view(torch.int32)
        return GaussianMixture(weights, means, variances, covariance_type, center, state[2], words[0], words[2] != 0,
                               labels.to(torch.int64), status)


def gmm(emb, components, covariance_type="diag", init="kmeans", n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0,
        weights_init=None, means_init=None, variances_init=None, device=None):
    """Fit a mixture of `components` Gaussians to the rows of emb (n, dim) on the GPU -> GaussianMixture.

    covariance_type: "diag" or "spherical".  init: "kmeans", as scikit-learn does -- clustering.kmeans(emb, components,
    seed=seed + i), one-hot responsibilities from its labels and one M-step on the device -- or "params" with means_init (K, dim)
    and optionally weights_init (K,) (default uniform) and variances_init ((K, dim) or (K,); default the column variances of emb,
    their mean for "spherical").  n_init > 1 runs seeds seed, seed + 1, ... and keeps the highest lower_bound (chosen on the
    device).  tol: on the change of the mean log-likelihood per row, as in scikit-learn; reg_covar is added to every variance.
    A CUDA tensor is read where it is when its layout allows; nothing synchronises with the host -- see GaussianMixture.check()."""
    shape = retrieval._check_2d(emb, "embeddings")
    _check_fit_args(shape, components, covariance_type, init, n_init, max_iter, tol, reg_covar)
    if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
        device = emb.device
    dev = _inputs.cuda_device(device, "the mixture is fitted on")
    x = retrieval._rows(emb, dev)
    return _fit_rows(x, components, covariance_type, init, n_init, max_iter, tol, reg_covar, seed, weights_init, means_init,
                     variances_init)


ComponentSelection = collections.namedtuple("ComponentSelection", "ks scores best_k best fits criterion")


def select_components(emb, ks, criterion="bic", device=None, **fit_args):
    """Fit gmm(emb, k, **fit_args) for each k of `ks` and score each fit on emb -> ComponentSelection(ks, scores (len(ks),)
    float64 on the device, best_k, best (the GaussianMixture of best_k), fits, criterion).  criterion: "bic" or "aic", lowest
    wins; among equal scores the first k wins, a NaN score never does.  Synchronises once, at the end."""
    if criterion not in CRITERIA:
        raise ValueError("criterion must be one of %s, got %r" % (CRITERIA, criterion))
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1:
        raise ValueError("ks = %r (expected one or more integers >= 1)" % (ks,))
    shape = retrieval._check_2d(emb, "embeddings")
    if isinstance(emb, torch.Tensor) and emb.is_cuda and device is None:
        device = emb.device
    dev = _inputs.cuda_device(device, "the mixture is fitted on")
    for k in ks:
        _check_fit_args(shape, k, fit_args.get("covariance_type", "diag"), fit_args.get("init", "kmeans"), fit_args.get("n_init", 1),
                        fit_args.get("max_iter", 100), fit_args.get("tol", 1e-3), fit_args.get("reg_covar", 1e-6))
    x = retrieval._rows(emb, dev)
    fits = [_fit_rows(x, k, **fit_args) for k in ks]
    scores = torch.stack([(gm.bic(x) if criterion == "bic" else gm.aic(x)).reshape(()) for gm in fits])
    ranked = torch.where(torch.isnan(scores), torch.full_like(scores, float("inf")), scores)
    best = int(torch.argmin(ranked).cpu())
    return ComponentSelection(tuple(ks), scores, ks[best], fits[best], fits, criterion)
