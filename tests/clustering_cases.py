"""Inputs and bounds shared by the clustering tests (test_clustering_cpu.py, test_gpu_clustering.py): Gaussian blobs, the two
inits, the rounding bound of an fp32 score, and the host trajectories, each computed once per session."""
import functools

import numpy as np

from audioset_convnext_inf_amd.pytorch.clustering import assign_host, kmeans_host


def blobs(n, dim, tk, sep, seed):
    """x (n, dim) float32: tk Gaussian blobs of unit variance whose means are sep * N(0, 1); lab (n,) the true blob of a row."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((tk, dim)) * sep
    lab = rng.integers(0, tk, n)
    x = np.float32(mu[lab] + rng.standard_normal((n, dim)))
    return x, lab


def blob_init(x, lab, K):
    """The first row of each true blob k < K."""
    return np.stack([x[np.nonzero(lab == k)[0][0]] for k in range(K)])


def rand_init(x, K, seed):
    return x[np.random.default_rng(seed + 100).choice(x.shape[0], K, replace=False)]


def score_bound(x, c, metric="euclidean"):
    """b (n, K): the rounding bound of the fp32 score of (row i, centre k).  The dot product is a chain of dim fused
    multiply-adds and a few additions in fp32, |error| <= (dim + 8) 2^-24 sum |x_i| |c_k|; the Euclidean score is
    fma(-2, dot, cc) with cc = sum c_k^2 from a chain of its own: b = (dim + 8) 2^-24 (2 sum |x_i| |c_k| + sum c_k^2).
    Cosine: the score is the raw -dot, b = (dim + 8) 2^-24 sum |x_i| |c_k|."""
    x, c = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(c, np.float64))
    eps = (x.shape[1] + 8) * 2.0 ** -24
    if metric == "cosine":
        return eps * (x @ c.T)
    return eps * (2.0 * (x @ c.T) + (c * c).sum(axis=1)[None, :])


def score_matrix(x, c, metric="euclidean"):
    """s64 (n, K): the float64 scores assign_host takes its arg-min of."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return -(x @ c.T) if metric == "cosine" else (c * c).sum(axis=1)[None, :] - 2.0 * (x @ c.T)


# (n, dim, K, sep, seed, init): assignment margins above the rounding bound at every iteration, no empty cluster
TRAJECTORIES = ((1000, 768, 8, 1.0, 1, "blob"), (2000, 768, 50, 0.5, 2, "blob"), (300, 64, 5, 1.0, 3, "rand"), (65, 4, 3, 3.0, 5, "rand"))
# (n, dim, K, sep, seed), "rand" init: margins of every size
ROUNDED = ((2000, 768, 50, 0.5, 2), (4097, 768, 256, 0.3, 4), (1001, 772, 33, 0.2, 7))


@functools.lru_cache(maxsize=None)
def case_input(n, dim, K, sep, seed, init):
    x, lab = blobs(n, dim, K, sep, seed)
    c0 = blob_init(x, lab, K) if init == "blob" else rand_init(x, K, seed)
    return x, c0


@functools.lru_cache(maxsize=None)
def trajectory(case, metric="euclidean", max_iter=100):
    """kmeans_host(tol_abs=0) of a TRAJECTORIES / ROUNDED case (the latter with the "rand" init)."""
    x, c0 = case_input(*case) if len(case) == 6 else case_input(*case, "rand")
    return kmeans_host(x, c0, metric, max_iter, 0.0)


def margins(x, c, metric="euclidean"):
    """(host labels, float64 gap of every row between its best and second-best centre (inf for K = 1), max_k b_ik)."""
    s = score_matrix(x, c, metric)
    lab, _ = assign_host(x, c, metric)
    b = score_bound(x, c, metric).max(axis=1)
    if s.shape[1] == 1:
        return lab, np.full(s.shape[0], np.inf), b
    part = np.partition(s, 1, axis=1)
    return lab, part[:, 1] - part[:, 0], b
