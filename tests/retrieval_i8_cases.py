"""Shared generators of the int8-index tests (test_retrieval_i8_cpu.py, test_gpu_retrieval_i8.py)."""
import numpy as np

# the planted corpora of the coverage condition: (n, dim, centres, sigma, nq, seed); k = 10, kc = 40, cosine
PLANTED = ((2000, 768, 50, 1.0, 200, 0), (2000, 768, 50, 0.3, 200, 0), (1000, 64, 20, 1.0, 200, 0))
K, KC = 10, 40
EXEMPT_SHARE = 0.02


def planted(n, dim, centres, sigma, nq, seed):
    """(rows (n, dim), queries (nq, dim)) float32: clusters around `centres` random centres, rows and queries drawn alike."""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((centres, dim))
    lab = rng.integers(0, centres, n)
    rows = cen[lab] + sigma * rng.standard_normal((n, dim))
    qlab = rng.integers(0, centres, nq)
    queries = cen[qlab] + sigma * rng.standard_normal((nq, dim))
    return rows.astype(np.float32), queries.astype(np.float32)


def random_codes(rng, rows, dim):
    return rng.integers(-127, 128, size=(rows, dim)).astype(np.int8)


def tie_codes(rng, rows, dim):
    """Codes from {-1, 0, 1}: few distinct dot products, so ties everywhere -- the order by index and the trim path."""
    return rng.integers(-1, 2, size=(rows, dim)).astype(np.int8)


def extreme_codes(rng, rows, dim):
    """All +-127, one sign per row: t = +-dim * 127^2 (+-66 064 384 at dim 4096)."""
    return (127 * rng.choice(np.array([-1, 1]), size=(rows, 1)) * np.ones((1, dim))).astype(np.int8)


def ascending_codes(n, dim):
    """Database row j scores j against the query codes of ascending_queries(): every row beats the last, one trim per
    CAP - k rows (the adversarial case of knn.hip's header)."""
    d = np.zeros((n, dim), dtype=np.int8)
    j = np.arange(n)
    d[:, 0] = j % 100                  # t = (j % 100) + 100 * (j // 100) = j with the query (1, 100, 0, ...)
    d[:, 1] = j // 100
    return d


def ascending_queries(nq, dim):
    q = np.zeros((nq, dim), dtype=np.int8)
    q[:, 0], q[:, 1] = 1, 100
    return q


def operand_map_codes(dim):
    """(cq (32, dim) the identity pattern in the LAST 32 columns, cd (32, dim) asymmetric): score (i, j) = cd[j][dim - 32 + i]."""
    cq = np.zeros((32, dim), dtype=np.int8)
    cq[np.arange(32), dim - 32 + np.arange(32)] = 1
    j, c = np.arange(32)[:, None], np.arange(dim)[None, :]
    cd = ((3 * j + 5 * c) % 11 - 5).astype(np.int8)
    return cq, cd


def quantize_rows(rng, n, dim):
    """Rows that exercise the quantiser: random ones, a repeated maximum, +amax and -amax, halves (y g = k + 0.5 exactly: amax
    127 makes g = 1), a zero row."""
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if n > 1:
        x[1] = np.clip(x[1], -1, 1)
        x[1, :2] = 1.0                                                 # a repeated maximum
    if n > 2:
        x[2] = np.clip(x[2], -1, 1)
        x[2, 0], x[2, dim - 1] = 2.0, -2.0                             # +amax and -amax
    if n > 3:
        half = (rng.integers(-126, 126, size=dim) + 0.5).astype(np.float32)
        half[0] = 127.0
        x[3] = half                                                    # round half to even: 0.5 -> 0, 1.5 -> 2, -2.5 -> -2
    if n > 4:
        x[4] = 0.0
    return x
