"""Inputs and bounds shared by the mixture tests (test_mixture_cpu.py, test_gpu_mixture.py): the cases with their initial
parameters, the rounding bound of an fp32 log-density derived from the kernel's stated arithmetic (include/acx.h), and the host
fits, each computed once per session."""
import functools

import numpy as np

from clustering_cases import TRAJECTORIES, blobs, case_input, rand_init

from audioset_convnext_inf_amd.pytorch import mixture

# well-separated blobs: the k-means trajectories with their own inits, unit variances, uniform weights (one-hot responsibilities)
HARD = TRAJECTORIES
# (n, dim, K, sep, seed): overlapping blobs, means = rand_init, variances = the column variances, uniform weights
SOFT = ((1000, 768, 8, 0.08, 12), (300, 64, 5, 0.3, 13), (65, 4, 3, 1.0, 14))
# the float32 E-step stops two iterations earlier than float64 here: fixed iteration counts only
SLOW = ((2000, 768, 8, 0.05, 11),)
TOL, REG = 1e-3, 1e-6
# (case, covariance type) whose n_iter the device must reproduce: every |change| of the host loops is at least 10 % of tol away
# from tol (test_mixture_cpu.py asserts it); the spherical fit of SOFT[2] passes tol by 1 % and stays out
NITER_CASES = tuple((c, "diag") for c in HARD + SOFT) + tuple((c, "spherical") for c in HARD + SOFT[:2])


@functools.lru_cache(maxsize=None)
def case_params(case):
    """(x float32 (n, dim), weights0 (K,), means0 (K, dim), variances0 (K, dim)) of a HARD (6 fields) or SOFT / SLOW case."""
    if len(case) == 6:
        x, c0 = case_input(*case)
        v0 = np.ones(c0.shape)
    else:
        n, dim, K, sep, seed = case
        x = blobs(n, dim, K, sep, seed)[0]
        c0 = rand_init(x, K, seed)
        v0 = np.tile(np.asarray(x, np.float64).var(axis=0)[None, :], (K, 1))
    K = c0.shape[0]
    return x, np.full(K, 1.0 / K), np.asarray(c0, np.float64), v0


def case_name(case):
    kind = "hard" if len(case) == 6 else "soft" if case in SOFT else "slow"
    return "%s-n%d-d%d-k%d" % ((kind,) + tuple(case[:3]))


def variances_of(v0, cov):
    return v0 if cov == "diag" else v0.mean(axis=1)


@functools.lru_cache(maxsize=None)
def host_fit(case, cov="diag", f32=False, max_iter=100, tol=TOL):
    x, w0, m0, v0 = case_params(case)
    return mixture.gmm_host(x, w0, m0, variances_of(v0, cov), cov, max_iter, tol, REG, np.float32 if f32 else np.float64)


@functools.lru_cache(maxsize=None)
def host_changes(case, cov="diag", f32=False):
    """|change| of every iteration after the first of the host loop (tol = TOL)."""
    lbs = host_fit(case, cov, f32).lower_bounds
    return np.abs(np.diff(lbs))


@functools.lru_cache(maxsize=None)
def params_at(case, it, cov="diag"):
    """The parameters the host holds after `it` iterations (0: the initial ones)."""
    x, w0, m0, v0 = case_params(case)
    if it == 0:
        return w0, m0, variances_of(v0, cov)
    f = host_fit(case, cov, False, it, 0.0)
    return f.weights, f.means, f.variances


# (n, K, dim) at the kernels' edges: one row, one component, a partial tile, a second wave, a second step, every dim % 16
EDGES = ((1, 1, 4), (63, 2, 20), (64, 63, 772), (65, 64, 20), (257, 65, 4), (65, 257, 20), (257, 257, 772))


def integer_case(n, K, dim):
    """(x float32, weights, means, variances): integer means in -4 .. 4, each row a mean plus integers in -1 .. 1, variances in
    {1/2, 1, 2, 4}, unequal weights.  Every product of the contraction is exact in fp32; blobs, so that a row's best component
    is ahead of the others by far more than the bound (random integer rows against random means are not, at dim 772)."""
    rng = np.random.default_rng(31 * n + 7 * K + dim)
    mu = rng.integers(-4, 5, (K, dim)).astype(np.float64)
    x = (mu[rng.integers(0, K, n)] + rng.integers(-1, 2, (n, dim))).astype(np.float32)
    v = 2.0 ** rng.integers(-1, 3, (K, dim))
    w = rng.random(K) + 0.5
    return x, w / w.sum(), mu, v


def total_slack(K, lpn):
    """|log_prob_sum - sum_i log_prob_norm[i]|: the sum takes every term before its rounding to fp32 (2^-24 |log_prob_norm|) and
    with log in float64 where log_prob_norm has logf (2 ulp of log s <= log K); the float64 sum itself adds n 2^-53 of it."""
    lpn = np.abs(np.asarray(lpn, np.float64))
    return float((2.0 ** -24 * lpn + 2.0 ** -22 * np.log(max(K, 2))).sum() + lpn.size * 2.0 ** -52 * lpn.sum())


def lp_bound(x, weights, means, variances, center=None):
    """b (n, K): the rounding bound of the device's fp32 log-density of (row i, component k) against log_prob_host in float64.
    lp = fp32(cst - D / 2) with D a chain of 2 dim fused multiply-adds over the fp32 operands fp32(xc^2) fp32(a) and
    fp32(xc) fp32(-2 b).  With T = sum xc^2 a + 2 sum |xc| |b| (the sum of the terms' magnitudes):
      the chain and its few additions    (2 dim + 8) 2^-24 T
      the operands' rounding             each factor 2^-24 relative, the product 2 2^-24 (+ second order): 3 2^-24 T
      the constant's rounding            2^-24 |cst| (the float32 yardstick of log_prob_host rounds it, and is held to this
                                         bound too; the device keeps it in float64)
      the final rounding                 2^-24 |lp|
    and D enters lp halved.  (Spherical on the device: the operands are fp32(xc^2), 1 and fp32(xc), fp32(-2 mc), and the float64
    1 / (2 v_k) scales D -- fewer roundings over terms of the same magnitudes, the same T.)"""
    xt, a, b, cst = mixture._operands(x, weights, means, variances, center)
    dim = xt.shape[1]
    T = (xt * xt) @ a.T + 2.0 * (np.abs(xt) @ np.abs(b).T)
    lp = cst[None, :] - 0.5 * ((xt * xt) @ a.T - 2.0 * (xt @ b.T))
    return 0.5 * (2 * dim + 8 + 3) * 2.0 ** -24 * T + 2.0 ** -24 * (np.abs(cst)[None, :] + np.abs(lp))


def lpn_slack(K, lpn):
    """What the fp32 logsumexp adds to max_k b_ik in log_prob_norm: s = sum_k expf(lp - m) has at most K terms, each with the
    rounding of its argument (|t| e^-t 2^-24 <= 2^-24 of s), of expf (2 ulp) and of the sum (depth <= K): (K + 16) 2^-24 relative,
    which is the absolute error of log s; logf adds 2 ulp of log s <= log K, the last addition 2^-24 |log_prob_norm|, and m itself
    carries none."""
    return (K + 16) * 2.0 ** -24 + 2.0 ** -22 * np.log(max(K, 1)) + 2.0 ** -23 * np.abs(lpn)


def resp_bound(K, bmax):
    """|resp_dev - resp_host| <= e^(2 bmax_i) - 1 + (K + 8) 2^-24: every log-density moves by at most bmax_i, so a ratio of two
    exponentials by e^(2 bmax_i); the fp32 quotient and sum add (K + 8) 2^-24."""
    return np.expm1(2.0 * bmax) + (K + 8) * 2.0 ** -24


def margins(x, weights, means, variances, center=None):
    """(host labels, float64 gap of every row between its best and second-best log-density (inf for K = 1), max_k b_ik)."""
    lp = mixture.log_prob_host(x, weights, means, variances, center)
    lab = np.argmax(lp + 0.0, axis=1)
    bmax = lp_bound(x, weights, means, variances, center).max(axis=1)
    if lp.shape[1] == 1:
        return lab, np.full(lp.shape[0], np.inf), bmax
    part = np.partition(lp, lp.shape[1] - 2, axis=1)
    return lab, part[:, -1] - part[:, -2], bmax


def mstep_bounds(x, resp, center=None):
    """(b_weights (K,), b_means (K, dim), b_variances (K, dim)): float64 sums of n terms on both sides, each within
    n 2^-53 sum |terms| of the exact sum.  With c = |center| (the device sums centred rows and adds the centre back),
    M = sum r (|x| + c) / N and Q = sum r (|x| + c)^2 / N, which dominate the sums of either side (M^2 <= Q):
      N_k, w_k     (n + 4) 2^-52 relative
      means        (n + 16) 2^-52 M
      variances    S2 / N within n 2^-53 Q, mean^2 within 2 |mean| n 2^-53 M <= 2 n 2^-53 Q, four roundings: (3 n + 4) 2^-52 Q
    (2^-52: one 2^-53 for each side)."""
    x = np.abs(np.asarray(x, np.float64))
    r = np.asarray(resp, np.float64)
    n = x.shape[0]
    c = np.zeros(x.shape[1]) if center is None else np.abs(np.asarray(center, np.float64))
    nk = r.sum(axis=0) + mixture.NK_EPS
    xa = x + c[None, :]
    M = (r.T @ xa) / nk[:, None]
    Q = (r.T @ (xa * xa)) / nk[:, None]
    return (n + 4) * 2.0 ** -52 * nk / n, (n + 16) * 2.0 ** -52 * M, (3 * n + 4) * 2.0 ** -52 * Q
