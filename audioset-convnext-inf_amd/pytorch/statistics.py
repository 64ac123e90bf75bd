"""Second-order statistics of embeddings on the GPU (acx_moments, acx_gram_f64, acx_eigh, acx_pca_* in include/acx.h): mean
and covariance in float64, a symmetric eigensolver, PCA / whitening, Mahalanobis distances and the Frechet distance between
two sets -- what numpy.cov, numpy.linalg.eigh, sklearn.decomposition.PCA and the usual scipy.linalg.sqrtm recipe do on the host.

    from audioset_convnext_inf_amd.pytorch.statistics import moments, eigh, PCA, frechet_distance, mahalanobis
    m = moments(emb, ddof=1)                      # Moments: m.mean (dim,), m.cov (dim, dim) float64 device tensors, m.n
    m.merge(moments(more))                        # the pooled moments of both sets
    values, vectors, state = eigh(m.cov)          # descending values, ROW k of vectors = the k-th eigenvector
    pca = PCA.fit(emb, components=64, whiten=True)
    z = pca.transform(emb); x = pca.inverse_transform(z)
    pca.components_, pca.explained_variance_, pca.explained_variance_ratio_, pca.mean_
    fd = frechet_distance(emb_a, emb_b)           # FrechetDistance: fd.value, fd.mean_term, fd.trace_term (0-d float64)
    d = mahalanobis(emb, m)                       # (n,) fp32 distances through the whitening transform
    pca.check(); fd.check(); float(fd)            # the calls that synchronise
    pca.save("pca.npz"); PCA.load("pca.npz")

Everything is queued on the current stream and nothing synchronises with the host (PCA.fit with a float `components`, which
has to read the spectrum to know its own output shape, is the one exception).  The covariance runs on the float64 matrix
instructions with the rows centred on load and all sums in a fixed order: no float atomics, the same input gives the same bits.
The eigensolver is cyclic Jacobi with the round-robin ordering, one launch per round, its stop decided on the device.

`moments_host`, `eigh_host`, `pca_host` and `frechet_distance_host` are the documented host definitions in numpy float64 (the
tests' reference); eigh_host states the device's algorithm step by step."""
import collections

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs

MAX_DIM = _ffi.STATS_MAX_DIM
MAX_SWEEPS = _ffi.EIGH_MAX_SWEEPS
DEFAULT_SWEEPS = 40
WHITEN_EPS = 1e-12            # whitening floors an eigenvalue at WHITEN_EPS * the largest one


def _check_2d(x, name):
    shape = tuple(getattr(x, "shape", ()))
    if len(shape) != 2:
        raise ValueError("%s must be 2-D (rows, dim), got shape %s" % (name, shape))
    if not 1 <= shape[1] <= MAX_DIM:
        raise ValueError("%s: dim = %d (expected 1 .. %d)" % (name, shape[1], MAX_DIM))
    return int(shape[0]), int(shape[1])


def _check_ddof(ddof):
    if isinstance(ddof, bool) or ddof not in (0, 1):
        raise ValueError("ddof = %r (expected 0 or 1)" % (ddof,))


def _check_sweeps(max_sweeps):
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or not 1 <= max_sweeps <= MAX_SWEEPS:
        raise ValueError("max_sweeps = %r (expected an integer in 1 .. %d)" % (max_sweeps, MAX_SWEEPS))


def _check_components(components, dim):
    """None (all), an integer in 1 .. dim, or a float in (0, 1): the share of the variance to keep."""
    if components is None:
        return
    if isinstance(components, bool):
        raise ValueError("components = %r" % (components,))
    if isinstance(components, (int, np.integer)):
        if not 1 <= components <= dim:
            raise ValueError("components = %d (expected 1 .. dim = %d)" % (components, dim))
    elif isinstance(components, (float, np.floating)):
        if not 0.0 < components < 1.0:
            raise ValueError("components = %r (a float must lie in (0, 1): the explained-variance share)" % (components,))
    else:
        raise ValueError("components = %r (expected None, an integer or a float in (0, 1))" % (components,))


def _count_for_share(values, share):
    """The smallest k whose leading eigenvalues (floored at 0) hold at least `share` of their total."""
    v = np.maximum(np.asarray(values, dtype=np.float64), 0.0)
    total = v.sum()
    if not total > 0:
        return 1
    return int(min(len(v), np.searchsorted(np.cumsum(v) / total, share, side="left") + 1))


# ---- the host definitions (numpy float64) ----------------------------------------------------------------------------------
HostMoments = collections.namedtuple("HostMoments", "mean cov n")
HostEigh = collections.namedtuple("HostEigh", "values vectors sweeps rotations converged")
HostPCA = collections.namedtuple("HostPCA", "components explained_variance explained_variance_ratio mean scale")
HostFrechet = collections.namedtuple("HostFrechet", "value mean_term trace_term")


def moments_host(x, ddof=1):
    """mean[j] = sum_i x[i][j] / n and cov[a][b] = sum_i (x_ia - mean_a)(x_ib - mean_b) / (n - ddof) in float64, the rows
    centred first (each difference rounded once); a zero cov when n - ddof == 0 -> HostMoments(mean, cov, n)."""
    _check_ddof(ddof)
    x = np.asarray(x, dtype=np.float64)
    n, dim = _check_2d(x, "x")
    if n < 1:
        raise ValueError("x has no rows")
    mean = x.sum(axis=0) / n
    xc = x - mean[None, :]
    cov = xc.T @ xc / (n - ddof) if n - ddof else np.zeros((dim, dim))
    cov = np.triu(cov) + np.triu(cov, 1).T
    return HostMoments(mean, cov, n)


def _sym_upper(a):
    return np.triu(a) + np.triu(a, 1).T


def eigh_host(a, max_sweeps=DEFAULT_SWEEPS):
    """The symmetric eigenproblem as the device solves it -> HostEigh(values descending, vectors with ROW k the k-th
    eigenvector, sweeps, rotations, converged).

    Cyclic Jacobi, round-robin ordering.  m = dim rounded up to even; a sweep is m - 1 rounds; in round r index m - 1 pairs with r
    and every other i with (2 r - i) mod (m - 1); a pair with the padding index of an odd dim is idle.  A pair p < q is rotated
    where |a_pq| > 2^-53 max_i |a_ii| of the INPUT: theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(1 +
    theta^2)) (sign(0) = 1), c = 1 / sqrt(1 + t^2), s = t c; a_pp - t a_pq, a_qq + t a_pq and a_pq = 0 replace the three, every
    other element (i <= j, mirrored) becomes c_j (c_i A[i][j] + g_i A[pi][j]) + g_j (c_i A[i][pj] + g_i A[pi][pj]) with g = -s at
    a pair's lower index and +s at its upper one -- all rotations of a round at once, from the OLD matrix.  The sweeps stop
    after one that applied no rotation (it counts); values are ordered descending, ties by the original index; a vector's entry
    of the largest magnitude (lowest index on ties) is made positive."""
    _check_sweeps(max_sweeps)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or not 1 <= a.shape[0] <= MAX_DIM:
        raise ValueError("a must be a square matrix of 1 .. %d rows, got shape %s" % (MAX_DIM, a.shape))
    d = a.shape[0]
    A = _sym_upper(a)
    V = np.eye(d)                                            # row j: the j-th accumulated vector
    idx = np.arange(d)
    sweeps = rotations = 0
    converged = False
    if not np.isfinite(A).all():
        return HostEigh(np.diag(A).copy(), V, 0, 0, False)
    m = d + (d & 1)
    thr = np.ldexp(np.abs(np.diag(A)).max(), -53)
    for sw in range(max_sweeps):
        applied = 0
        for r in range(m - 1):
            part = (2 * r - idx) % (m - 1)
            part[idx == r] = m - 1
            if m - 1 < d:
                part[m - 1] = r
            valid = part < d
            p = np.where(valid, part, idx)
            lo, hi = np.minimum(idx, p), np.maximum(idx, p)
            apq = A[lo, hi]
            on = valid & (np.abs(apq) > thr)
            app, aqq = A[lo, lo], A[hi, hi]
            with np.errstate(over="ignore"):                 # a pivot tiny against the diagonal gap: theta -> inf, t = 0, as on the device
                theta = np.divide(aqq - app, 2.0 * apq, out=np.zeros(d), where=on)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(1.0 + theta * theta))
            c1 = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c1
            lower = idx == lo
            c = np.where(on, c1, 1.0)
            g = np.where(on, np.where(lower, -s, s), 0.0)
            delta = np.where(on, np.where(lower, -(t * apq), t * apq), 0.0)
            U = c[:, None] * A + g[:, None] * A[p, :]
            N = c[None, :] * U + g[None, :] * U[:, p]
            N[idx, idx] = A[idx, idx] + delta
            N[idx[on], p[on]] = 0.0
            A = _sym_upper(N)
            V = c[:, None] * V + g[:, None] * V[p, :]
            applied += int((on & (idx < p)).sum())
        sweeps = sw + 1
        rotations += applied
        if applied == 0:
            converged = True
            break
    values = np.diag(A).copy()
    order = np.lexsort((idx, -values))
    vectors = V[order]
    top = np.argmax(np.abs(vectors), axis=1)
    flip = vectors[np.arange(d), top] < 0.0
    vectors[flip] = -vectors[flip]
    return HostEigh(values[order], vectors, sweeps, rotations, converged)


def _host_spectrum(cov, solver, max_sweeps=DEFAULT_SWEEPS):
    """(values descending, vectors as rows): eigh_host, or LAPACK for the sizes the host definition is too slow for."""
    if solver == "jacobi":
        e = eigh_host(cov, max_sweeps)
        return e.values, e.vectors
    if solver != "lapack":
        raise ValueError("solver must be \"jacobi\" or \"lapack\", got %r" % (solver,))
    w, v = np.linalg.eigh(cov)
    return w[::-1].copy(), v.T[::-1].copy()


def pca_host(x, components=None, whiten=False, solver="jacobi", eps=WHITEN_EPS):
    """PCA as PCA.fit computes it -> HostPCA(components (k, dim), explained_variance (k,), explained_variance_ratio (k,),
    mean (dim,), scale (k,) or None): moments_host(x, ddof=1), its spectrum (eigh_host), the leading k rows; variances floored at
    0, the ratio taken against the sum of all floored eigenvalues; whiten: scale = 1 / sqrt(max(lambda, eps * lambda_max))."""
    x = np.asarray(x, dtype=np.float64)
    n, dim = _check_2d(x, "x")
    _check_components(components, dim)
    mo = moments_host(x, 1)
    values, vectors = _host_spectrum(mo.cov, solver)
    var = np.maximum(values, 0.0)
    k = dim if components is None else components
    if isinstance(k, (float, np.floating)):
        k = _count_for_share(values, k)
    total = var.sum()
    ratio = var[:k] / total if total > 0 else np.zeros(k)
    scale = 1.0 / np.sqrt(np.maximum(values[:k], eps * max(var[0], np.finfo(np.float64).tiny))) if whiten else None
    return HostPCA(vectors[:k].copy(), var[:k].copy(), ratio, mo.mean, scale)


def frechet_from_moments_host(ma, mb, solver="lapack"):
    """|mu_a - mu_b|^2 + tr Sa + tr Sb - 2 sum_i sqrt(max(lambda_i, 0)), lambda the eigenvalues of Sa^1/2 Sb Sa^1/2 and
    Sa^1/2 = V diag(sqrt(max(lambda(Sa), 0))) V^T -> HostFrechet(value, mean_term, trace_term)."""
    if ma.mean.shape != mb.mean.shape:
        raise ValueError("the two sets have dims %d and %d" % (ma.mean.shape[0], mb.mean.shape[0]))
    wa, va = _host_spectrum(ma.cov, solver)
    q = np.sqrt(np.sqrt(np.maximum(wa, 0.0)))[:, None] * va
    h = q.T @ q
    inner = h.T @ (mb.cov.T @ h)
    w, _ = _host_spectrum(_sym_upper(inner), solver)
    diff = ma.mean - mb.mean
    mean_term = float(diff @ diff)
    trace_term = float(np.trace(ma.cov) + np.trace(mb.cov) - 2.0 * np.sqrt(np.maximum(w, 0.0)).sum())
    return HostFrechet(mean_term + trace_term, mean_term, trace_term)


def frechet_distance_host(x, y, solver="lapack"):
    """The Frechet distance of the Gaussians fitted to the rows of x and y (ddof = 1), frechet_from_moments_host's route.
    solver: "lapack" (numpy.linalg.eigh) or "jacobi" (eigh_host, the device's algorithm)."""
    return frechet_from_moments_host(moments_host(x, 1), moments_host(y, 1), solver)


# ---- the device path -------------------------------------------------------------------------------------------------------
def _f32_rows(x, device, name="x", dim=None):
    """x (rows, dim) -> an fp32 tensor on `device` with unit column stride; a CUDA fp32 tensor that is readable -- a column slice
    of a wider tensor too -- is returned as it is (the kernels need no padding and no alignment beyond the element's)."""
    shape = _check_2d(x, name)
    if dim is not None and shape[1] != dim:
        raise ValueError("%s has dim %d (expected %d)" % (name, shape[1], dim))
    if shape[0] < 1:
        raise ValueError("%s has no rows" % name)
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return _inputs.rows(x.detach().to(device=device, dtype=torch.float32))


def _f64_matrix(a, device, name):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if a.dim() != 2:
        raise ValueError("%s must be 2-D, got shape %s" % (name, tuple(a.shape)))
    return _inputs.rows(a.detach().to(device=device, dtype=torch.float64))


def _device_of(x, device, what):
    if isinstance(x, torch.Tensor) and x.is_cuda and device is None:
        device = x.device
    return _inputs.cuda_device(device, what)


def _raise_status(word):
    st = int(word.cpu().reshape(-1)[0])
    if st & _ffi.STATS_NONFINITE:
        raise ValueError("the input holds NaN or infinite values")
    if st & _ffi.STATS_DEGENERATE:
        raise ValueError("too few rows: n - ddof == 0, the covariance is undefined")
    if st & _ffi.STATS_NOT_CONVERGED:
        raise RuntimeError("the eigensolver still rotated in its last sweep: raise max_sweeps")


class Moments:
    """mean (dim,) and cov (dim, dim) float64 device tensors of n rows with `ddof`; nothing synchronised."""

    def __init__(self, mean, cov, n, ddof=1, status=None):
        self.mean, self.cov, self.n, self.ddof = mean, cov, int(n), int(ddof)
        self.device = mean.device
        self.status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=self.device)

    def merge(self, other):
        """The moments of the union of the two sets, from the two means and covariances alone (the pooled update)."""
        if other.mean.shape != self.mean.shape or other.ddof != self.ddof:
            raise ValueError("merge needs moments of the same dim and ddof")
        na, nb = self.n, other.n
        n = na + nb
        delta = other.mean.to(self.device) - self.mean
        mean = self.mean + delta * (nb / n)
        if n - self.ddof == 0:
            cov = torch.zeros_like(self.cov)
        else:
            cov = (self.cov * (na - self.ddof) + other.cov.to(self.device) * (nb - other.ddof)
                   + torch.outer(delta, delta) * (na * nb / n)) / (n - self.ddof)
        # a set of one row with ddof = 1 carries a zero covariance and DEGENERATE; the union of two sets is not degenerate
        status = (self.status | other.status.to(self.device)) & ~_ffi.STATS_DEGENERATE if n - self.ddof else self.status | other.status
        return Moments(mean, cov, n, self.ddof, status)

    def check(self):
        """Synchronise: ValueError for NaN / infinite input or n - ddof == 0."""
        _raise_status(self.status)
        return self


def moments(x, ddof=1, device=None):
    """Mean and covariance of the rows of x (n, dim) in float64 on the GPU (acx_moments) -> Moments."""
    _check_ddof(ddof)
    dev = _device_of(x, device, "the statistics run on")
    x = _f32_rows(x, dev)
    n, dim = x.shape
    with torch.cuda.device(dev):
        mean = torch.empty(dim, dtype=torch.float64, device=dev)
        cov = torch.empty((dim, dim), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.moments_workspace_bytes(n, dim)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _ffi.moments(vp(x), x.stride(0), n, dim, ddof, vp(mean), vp(cov), dim, vp(status), (vp(ws), ws_bytes), _ffi.stream_ptr(dev))
    return Moments(mean, cov, n, ddof, status)


def gram(a, b, device=None):
    """a^T b in float64 on the GPU (acx_gram_f64): a (rows, m), b (rows, n) -> (m, n), sums in a fixed order."""
    dev = _device_of(a, device, "the statistics run on")
    a, b = _f64_matrix(a, dev, "a"), _f64_matrix(b, dev, "b")
    if a.shape[0] != b.shape[0] or a.shape[0] < 1:
        raise ValueError("a and b must have the same, positive number of rows, got %d and %d" % (a.shape[0], b.shape[0]))
    for t, name in ((a, "a"), (b, "b")):
        if not 1 <= t.shape[1] <= MAX_DIM:
            raise ValueError("%s has %d columns (expected 1 .. %d)" % (name, t.shape[1], MAX_DIM))
    with torch.cuda.device(dev):
        out = torch.empty((a.shape[1], b.shape[1]), dtype=torch.float64, device=dev)
        _ffi.gram_f64(vp(a), a.stride(0), vp(b), b.stride(0), a.shape[0], a.shape[1], b.shape[1], vp(out), out.stride(0),
                      _ffi.stream_ptr(dev))
    return out


class EighState:
    """The device-side outcome of eigh(): sweeps (int32), rotations (int64), converged (bool) as 0-d device tensors and the
    status word; check() synchronises."""

    def __init__(self, words, status):
        self.sweeps = words[0]
        self.done = words[1]
        self.rotations = words.view(torch.int64)[1]
        self.status = status
        self.converged = (status[0] & (_ffi.STATS_NOT_CONVERGED | _ffi.STATS_NONFINITE)) == 0

    def check(self):
        _raise_status(self.status)
        return self


def eigh(a, max_sweeps=DEFAULT_SWEEPS, device=None):
    """Eigenvalues (descending) and eigenvectors (as ROWS) of the symmetric float64 matrix a on the GPU (acx_eigh) ->
    (values (dim,), vectors (dim, dim), EighState).  max_sweeps sweeps are queued and the device decides when to stop."""
    _check_sweeps(max_sweeps)
    dev = _device_of(a, device, "the statistics run on")
    a = _f64_matrix(a, dev, "a")
    dim = a.shape[0]
    if a.shape[1] != dim or not 1 <= dim <= MAX_DIM:
        raise ValueError("a must be a square matrix of 1 .. %d rows, got shape %s" % (MAX_DIM, tuple(a.shape)))
    with torch.cuda.device(dev):
        values = torch.empty(dim, dtype=torch.float64, device=dev)
        vectors = torch.empty((dim, dim), dtype=torch.float64, device=dev)
        words = torch.zeros(4, dtype=torch.int32, device=dev)              # struct acx_eigh_state
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws_bytes = _ffi.eigh_workspace_bytes(dim)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _ffi.eigh(vp(a), a.stride(0), dim, int(max_sweeps), vp(values), vp(vectors), dim, vp(words), vp(status), (vp(ws), ws_bytes),
                  _ffi.stream_ptr(dev))
    return values, vectors, EighState(words, status)


class PCA:
    """A fitted PCA: components_ (k, dim), explained_variance_ (k,), explained_variance_ratio_ (k,) and mean_ (dim,) as float64
    device tensors; transform / inverse_transform run in fp32 on the matrix cores with the rounded copies."""

    def __init__(self, components, explained_variance, explained_variance_ratio, mean, whiten=False, eps=WHITEN_EPS,
                 top_variance=None, n=0, status=None):
        self.components_, self.explained_variance_, self.explained_variance_ratio_, self.mean_ = (
            components, explained_variance, explained_variance_ratio, mean)
        self.whiten, self.eps, self.n_samples_ = bool(whiten), float(eps), int(n)
        self.device = components.device
        self.n_components_, self.dim = int(components.shape[0]), int(components.shape[1])
        self.status = status if status is not None else torch.zeros(1, dtype=torch.int32, device=self.device)
        self._top = explained_variance[:1].max() if top_variance is None else top_variance     # the largest eigenvalue of the fit
        self._w32 = components.to(torch.float32).contiguous()
        self._mean32 = mean.to(torch.float32).contiguous()
        self._scale = self._unscale = None
        if self.whiten:
            sd = torch.sqrt(torch.clamp_min(explained_variance, 0.0).clamp_min(self._top.clamp_min(0.0) * self.eps)
                            .clamp_min(torch.finfo(torch.float64).tiny))
            self._scale = (1.0 / sd).to(torch.float32).contiguous()
            self._unscale = sd.to(torch.float32).contiguous()

    @classmethod
    def from_moments(cls, mo, components=None, whiten=False, max_sweeps=DEFAULT_SWEEPS, eps=WHITEN_EPS):
        """The PCA of a set from its Moments (ddof as given there).  A float `components` reads the spectrum on the host to
        learn k, which synchronises; None and integers do not."""
        dim = mo.mean.shape[0]
        _check_components(components, dim)
        values, vectors, st = eigh(mo.cov, max_sweeps)
        var = values.clamp_min(0.0)
        k = dim if components is None else components
        if isinstance(k, (float, np.floating)):
            k = _count_for_share(values.cpu().numpy(), k)
        total = var.sum()
        ratio = torch.where(total > 0, var[:k] / total, torch.zeros_like(var[:k]))
        return cls(vectors[:k].contiguous(), var[:k].contiguous(), ratio, mo.mean, whiten, eps, var[0], mo.n, mo.status | st.status)

    @classmethod
    def fit(cls, x, components=None, whiten=False, max_sweeps=DEFAULT_SWEEPS, eps=WHITEN_EPS, device=None):
        """Fit on the rows of x (n, dim): moments(x, ddof=1), eigh of the covariance, the leading components.
        components: None (all dim), an integer k, or a float in (0, 1) = the explained-variance share to reach."""
        _check_components(components, _check_2d(x, "x")[1])
        return cls.from_moments(moments(x, 1, device), components, whiten, max_sweeps, eps)

    def transform(self, x):
        """(n, k) fp32: scale_c * sum_j fl32(x_ij - mean_j) W_cj (acx_pca_transform); whitened when the fit was."""
        x = _f32_rows(x, self.device, "x", self.dim)
        n, k = x.shape[0], self.n_components_
        with torch.cuda.device(self.device):
            out = torch.empty((n, k), dtype=torch.float32, device=self.device)
            _ffi.pca_transform(vp(x), x.stride(0), n, self.dim, vp(self._mean32), vp(self._w32), self.dim, k, vp(self._scale), vp(out),
                               k, _ffi.stream_ptr(self.device))
        return out

    def inverse_transform(self, z):
        """(n, dim) fp32: mean_j + sum_c (z_ic * unscale_c) W_cj (acx_pca_inverse)."""
        if tuple(getattr(z, "shape", ()))[1:] != (self.n_components_,):
            raise ValueError("z must be (rows, %d), got shape %s" % (self.n_components_, tuple(getattr(z, "shape", ()))))
        if not isinstance(z, torch.Tensor):
            z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
        z = _inputs.rows(z.detach().to(device=self.device, dtype=torch.float32))
        n, k = z.shape
        if n < 1:
            raise ValueError("z has no rows")
        with torch.cuda.device(self.device):
            out = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
            _ffi.pca_inverse(vp(z), z.stride(0), n, k, vp(self._unscale), vp(self._w32), self.dim, self.dim, vp(self._mean32), vp(out),
                             self.dim, _ffi.stream_ptr(self.device))
        return out

    def check(self):
        """Synchronise: ValueError for NaN / infinite input or fewer than two rows, RuntimeError if the eigensolver did not
        converge."""
        _raise_status(self.status)
        return self

    def save(self, path):
        np.savez(path, method="pca", components=self.components_.cpu().numpy(), explained_variance=self.explained_variance_.cpu().numpy(),
                 explained_variance_ratio=self.explained_variance_ratio_.cpu().numpy(), mean=self.mean_.cpu().numpy(),
                 whiten=self.whiten, eps=self.eps, top_variance=self._top.cpu().numpy(), n=self.n_samples_)

    @classmethod
    def load(cls, path, device=None):
        dev = _inputs.cuda_device(device, "a PCA is applied on")
        with np.load(path) as f:
            if str(f["method"]) != "pca":
                raise ValueError("%s holds %s, not a PCA" % (path, f["method"]))
            comp, var, ratio, mean = f["components"], f["explained_variance"], f["explained_variance_ratio"], f["mean"]
            whiten, eps, top, n = bool(f["whiten"]), float(f["eps"]), f["top_variance"], int(f["n"])
        if comp.ndim != 2 or mean.shape != (comp.shape[1],) or var.shape != (comp.shape[0],) or not np.isfinite(comp).all():
            raise ValueError("%s: components must be a finite (k, dim) array with (k,) variances and a (dim,) mean" % path)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).to(dev)
        return cls(t(comp).contiguous(), t(var), t(ratio), t(mean), whiten, eps, t(top), n)


class FrechetDistance:
    """value = mean_term + trace_term as 0-d float64 device tensors; float() and check() synchronise."""

    def __init__(self, value, mean_term, trace_term, status):
        self.value, self.mean_term, self.trace_term, self.status = value, mean_term, trace_term, status

    def __iter__(self):
        return iter((self.value, self.mean_term, self.trace_term))

    def __float__(self):
        return float(self.value.cpu())

    def check(self):
        _raise_status(self.status)
        return self


def frechet_distance_from_moments(ma, mb, max_sweeps=DEFAULT_SWEEPS):
    """The Frechet distance of two Gaussians from their Moments, all on the device -> FrechetDistance.
    |mu_a - mu_b|^2 + tr Sa + tr Sb - 2 sum_i sqrt(max(lambda_i, 0)) with lambda the eigenvalues of Sa^1/2 Sb Sa^1/2 and
    Sa^1/2 = V diag(sqrt(max(lambda(Sa), 0))) V^T: two eigh calls and three Gram products."""
    if ma.mean.shape != mb.mean.shape:
        raise ValueError("the two sets have dims %d and %d" % (ma.mean.shape[0], mb.mean.shape[0]))
    dev = ma.device
    sb, mub = mb.cov.to(dev), mb.mean.to(dev)
    wa, va, sta = eigh(ma.cov, max_sweeps)
    q = torch.sqrt(torch.sqrt(wa.clamp_min(0.0)))[:, None] * va
    h = gram(q, q)                                           # Sa^1/2, exactly symmetric
    inner = gram(h, gram(sb, h))                             # Sa^1/2 Sb Sa^1/2
    w, _, stb = eigh(inner, max_sweeps)
    diff = ma.mean - mub
    mean_term = (diff * diff).sum()
    trace_term = torch.diagonal(ma.cov).sum() + torch.diagonal(sb).sum() - 2.0 * torch.sqrt(w.clamp_min(0.0)).sum()
    status = ma.status | mb.status.to(dev) | sta.status | stb.status
    return FrechetDistance(mean_term + trace_term, mean_term, trace_term, status)


def frechet_distance(x, y, max_sweeps=DEFAULT_SWEEPS, device=None):
    """The Frechet distance between the Gaussians fitted to the rows of x (n, dim) and y (m, dim) (ddof = 1) -- the Frechet
    audio distance when the rows are embeddings of two sets of clips -> FrechetDistance."""
    dev = _device_of(x, device, "the statistics run on")
    return frechet_distance_from_moments(moments(x, 1, dev), moments(y, 1, dev), max_sweeps)


def mahalanobis(x, moments_or_pca, eps=WHITEN_EPS):
    """(n,) fp32: sqrt((x - mu)^T S^-1 (x - mu)) per row through the whitening transform -- |transform(x)| of a whitened PCA.  A
    Moments is whitened here with all its components (eigenvalues floored at eps * the largest); a PCA must have been fitted
    with whiten=True and measures the distance inside its subspace."""
    if isinstance(moments_or_pca, Moments):
        pca = PCA.from_moments(moments_or_pca, None, True, eps=eps)
    elif isinstance(moments_or_pca, PCA):
        pca = moments_or_pca
        if not pca.whiten:
            raise ValueError("mahalanobis needs a PCA fitted with whiten=True")
    else:
        raise ValueError("mahalanobis needs a Moments or a PCA, got %r" % type(moments_or_pca).__name__)
    z = pca.transform(x)
    return torch.sqrt((z * z).sum(dim=1))
