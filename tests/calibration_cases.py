"""Seeded inputs of the calibration tests (tests/test_calibration_cpu.py, tests/test_gpu_calibration.py) and the bounds both
hold the fits to.  Everything is numpy; a case is generated once per process and must be left unchanged.

Logits are class-conditional Gaussians with overlapping means (every Hessian well conditioned); the edge families: probabilities
on bin edges, classes with no positive / no negative / a constant column, rows with NaN / inf, a target of 2, labels of -1 and N,
strided layouts and the three target dtypes."""
import functools

import numpy as np

U53 = 2.0 ** -53

RELIABILITY_ROWS = (1, 63, 65, 1025)
RELIABILITY_CLASSES = (1, 3, 64, 65, 527)
RELIABILITY_BINS = (1, 10, 15, 64)
EDGE_BINS = (1, 2, 8, 64)
TOPLABEL_SHAPES = ((1, 2), (65, 5), (257, 50), (33, 2049))       # the last one is run with a row stride > N
TOPLABEL_BETAS = (None, 0.5, 2.0)
PLATT_ROWS = (2, 65, 1025, 4097)
PLATT_CLASSES = (1, 3, 65)
PLATT_STREAMED = (32769, 2)                                      # beyond the rows a workgroup keeps in LDS
PLANTED_BETAS = (0.25, 1.0, 3.0)
TEMPERATURE_EVALUATIONS = 64


@functools.lru_cache(maxsize=None)
def multilabel(n, C, seed=0):
    """(logits (n, C) float32, target (n, C) bool): y ~ Bernoulli(0.3) with row 0 positive and row 1 (if any) negative in every
    class, z = 0.8 (2 y - 1) + 1.5 randn."""
    rs = np.random.RandomState(1000 * seed + 7 * n + C)
    y = rs.rand(n, C) < 0.3
    y[0] = True
    if n > 1:
        y[1] = False
    z = (0.8 * (2.0 * y - 1.0) + 1.5 * rs.randn(n, C)).astype(np.float32)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


@functools.lru_cache(maxsize=None)
def probabilities(n, C, seed=0):
    """(probs (n, C) float32 in [0, 1], target (n, C) bool) -- the sigmoid of multilabel()'s logits, rounded to float32."""
    z, y = multilabel(n, C, seed)
    p = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    p.setflags(write=False)
    return p, y


def edge_probabilities(bins):
    """(probs (bins + 3, 1) float32, target, expected bin of every row): k / bins for k = 0 .. bins, then 0.0 and 1.0.  For the
    power-of-two bin counts of EDGE_BINS, k / bins and its product with bins are exact in float32."""
    p = np.array([k / bins for k in range(bins + 1)] + [0.0, 1.0], dtype=np.float32)[:, None]
    expect = np.array([min(k, bins - 1) for k in range(bins + 1)] + [0, bins - 1], dtype=np.int64)
    y = (np.arange(p.shape[0]) % 2 == 0)[:, None]
    return p, y, expect


@functools.lru_cache(maxsize=None)
def degenerate_multilabel(n=65):
    """(logits (n, 4), target): class 0 regular, class 1 without a positive, class 2 without a negative, class 3 a constant
    column."""
    z, y = multilabel(n, 4, seed=3)
    z, y = z.copy(), y.copy()
    y[:, 1] = False
    y[:, 2] = True
    z[:, 3] = 0.25
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


@functools.lru_cache(maxsize=None)
def separable(n=65):
    """(logits (n, 2), target): class 0 regular, class 1 separable (z > 0 exactly where y) -- smooth=False has no minimiser."""
    z, y = multilabel(n, 2, seed=4)
    z, y = z.copy(), y.copy()
    z[:, 1] = np.where(y[:, 1], np.abs(z[:, 1]) + 0.1, -np.abs(z[:, 1]) - 0.1)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


@functools.lru_cache(maxsize=None)
def singlelabel(n, N, beta_star=1.0, seed=0):
    """(logits (n, N) float32, labels (n,) int64): z = 2 randn, labels sampled from softmax(beta_star z)."""
    rs = np.random.RandomState(1000 * seed + 13 * n + N + int(100 * beta_star))
    z = (2.0 * rs.randn(n, N)).astype(np.float32)
    u = beta_star * z.astype(np.float64)
    q = np.exp(u - u.max(axis=1, keepdims=True))
    cdf = np.cumsum(q / q.sum(axis=1, keepdims=True), axis=1)
    y = np.minimum((cdf < rs.rand(n, 1)).sum(axis=1), N - 1).astype(np.int64)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


def constant_rows(n=5, N=7):
    """Every row constant: the temperature has no effect (ACX_CAL_DEGENERATE)."""
    z = np.repeat(np.linspace(-1.0, 1.0, n, dtype=np.float32)[:, None], N, axis=1)
    return z, (np.arange(n) % N).astype(np.int64)


def bound_cases():
    """{"high": (z, y), "low": (z, y)}: labels = argmax of small logits drive beta up against 1e4, labels = argmin drive it down
    against 1e-4."""
    z = (1e-3 * singlelabel(65, 5, 1.0, seed=9)[0]).astype(np.float32)
    return {"high": (z, z.argmax(axis=1).astype(np.int64)), "low": (z, z.argmin(axis=1).astype(np.int64))}


def strided(a, pad=3, fill=np.nan):
    """A copy of the 2-D array `a` as a column slice of a wider array (row stride = columns + pad) whose other columns hold
    `fill`."""
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


def sum_bound(n, total):
    """Two float64 summation orders of n non-negative terms differ by at most 2 n 2^-53 times the sum."""
    return 2.0 * n * U53 * abs(total)


def platt_bound(z, a, b, lam_min):
    """The stopping rule, plus the worst-case rounding of the float64 sums carried through the host's own Hessian (margin 8 for
    exp / log)."""
    n = z.shape[0]
    return 1e-10 * max(1.0, abs(a), abs(b)) + 8.0 * n * n * U53 * max(1.0, float(np.abs(z).max())) / lam_min


def temperature_bound(z, beta, h):
    """The same for F' / F'' over n N terms."""
    nN = float(z.shape[0] * z.shape[1])
    return 1e-10 * max(1.0, beta) + 8.0 * nN * nN * U53 * max(1.0, float(np.abs(z).max())) / h
