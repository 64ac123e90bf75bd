"""The cases of the ranking-metric tests (test_ranking_cpu.py, test_gpu_ranking.py): scores on grids that force ties, float32
edge values, and targets of every density a row can have.  A plain helper, not a conftest."""
import numpy as np

F32 = np.finfo(np.float32)
# -0.0 next to +0.0 (one level), the smallest denormals, the largest denormal, the smallest normal and the float32 extremes
EDGE = np.array([-0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, F32.max, -F32.max, 0.5], np.float32)
GRIDS = (1, 2, 4, None, "edge")            # g values only: all-equal rows, heavy ties; None: no ties; "edge": the values above
# positives of a row, cycled over the rows: about 3, none, one, about 3, N - 1, about 3, N, one
KINDS = ("few", "none", "one", "few", "all_but_one", "few", "all", "one")
SPARSE = ("few", "none", "one")           # at most 8 positives a row: what a very wide head is tested with


def scores(rows, n, grid, seed):
    """(rows, n) float32.  grid None: every row a permutation of n distinct values (no ties at all)."""
    rng = np.random.default_rng(seed)
    if grid is None:
        base = np.linspace(-3.0, 3.0, n, dtype=np.float64).astype(np.float32) if n > 1 else np.array([0.25], np.float32)
        assert len(np.unique(base)) == n
        return np.stack([rng.permutation(base) for _ in range(rows)])
    values = EDGE if isinstance(grid, str) else (np.arange(grid, dtype=np.float32) / np.float32(grid) - np.float32(0.25))
    return values[rng.integers(0, len(values), size=(rows, n))]


def targets(rows, n, seed, kinds=KINDS):
    """(rows, n) uint8: row i has the density kinds[i % len(kinds)]."""
    rng = np.random.default_rng(seed + 1000)
    y = np.zeros((rows, n), np.uint8)
    for i in range(rows):
        kind = kinds[i % len(kinds)]
        count = {"none": 0, "one": 1, "few": min(n, int(rng.integers(2, 9))), "all_but_one": n - 1, "all": n}[kind]
        y[i, rng.permutation(n)[:count]] = 1
    return y


def case(rows, n, grid, seed, kinds=KINDS):
    return targets(rows, n, seed, kinds), scores(rows, n, grid, seed)


def dcase_lwlrap(truth, score):
    """The DCASE 2019 Task 2 formula, written straight from its statement: per clip the classes sorted by score descending, the
    precision of each positive class = positives at or above its rank / its rank; per class the mean over its positive clips;
    the result weighted by each class's share of the positives.  -> (per_class, weight, lwlrap).  Depends on argsort's order
    where scores tie: call it on tie-free cases."""
    rows, C = truth.shape
    precision = np.zeros((rows, C), np.float64)
    for i in range(rows):
        pos = np.flatnonzero(truth[i] > 0)
        if len(pos) == 0:
            continue
        retrieved = np.argsort(score[i])[::-1]
        rank = np.zeros(C, np.int64)
        rank[retrieved] = np.arange(C)
        hit = np.zeros(C, bool)
        hit[rank[pos]] = True
        precision[i, pos] = np.cumsum(hit)[rank[pos]] / (1.0 + rank[pos])
    per_label = (truth > 0).sum(axis=0)
    per_class = precision.sum(axis=0) / np.maximum(1, per_label)
    weight = per_label / float(per_label.sum())
    return per_class, weight, float((per_class * weight).sum())
