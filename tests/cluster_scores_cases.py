"""Cases shared by test_cluster_scores_cpu.py and test_gpu_cluster_scores.py (pytorch/cluster_scores.py; acx_silhouette,
acx_cluster_dispersion, acx_contingency in include/acx.h): the generators, the rounding bound of a pair distance and what follows
from it per row, and a Python restatement of the silhouette kernel's walk."""
import functools

import numpy as np

from audioset_convnext_inf_amd.pytorch.cluster_scores import silhouette_host

# ---- Gaussian rows -----------------------------------------------------------------------------------------------------------
# (n, dim, K, centre scale, spread, seed): blobs with no duplicate rows; the last one has near-duplicate rows inside a cluster
GAUSS = ((257, 768, 5, 1.0, 1.0, 3), (300, 20, 7, 2.0, 1.0, 4), (131, 3, 4, 3.0, 1.0, 5), (200, 20, 4, 1.0, 1e-4, 6))
GAUSS_IDS = ["n%d-d%d-k%d%s" % (c[0], c[1], c[2], "-near" if c[4] < 1e-2 else "") for c in GAUSS]
SKLEARN_SHAPES = GAUSS[:3]


@functools.lru_cache(maxsize=None)
def gauss(n, dim, K, scale, spread, seed):
    """-> (x (n, dim) float32, geometric labels = the blob of each row, random labels), every label in use."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, dim)) * scale
    blob = np.arange(n) % K
    rng.shuffle(blob)
    x = (centres[blob] + spread * rng.standard_normal((n, dim))).astype(np.float32)
    assert len({r.tobytes() for r in x}) == n
    rand = np.arange(n) % K
    rng.shuffle(rand)
    return x, blob.astype(np.int64), rand.astype(np.int64)


# ---- integer rows: every distance an integer -----------------------------------------------------------------------------------
def integer_rows(m, dim, p0=0, p1=None):
    """Row i = 3 m_i at column p0 and 4 m_i at column p1, zero elsewhere: d(i, j) = 5 |m_i - m_j| exactly."""
    m = np.asarray(m, dtype=np.int64)
    p1 = dim - 1 if p1 is None else p1
    x = np.zeros((m.size, dim), dtype=np.float32)
    x[:, p0] = 3 * m
    x[:, p1] += 4 * m
    return x


def _sizes_to_labels(sizes, ids, seed):
    """Shuffled labels with sizes[k] rows of label ids[k]: the partition's boundaries sit at the cumulative sizes."""
    lab = np.repeat(np.asarray(ids), np.asarray(sizes))
    np.random.default_rng(seed).shuffle(lab)
    return lab.astype(np.int64)


def equal_cases():
    """-> list of dicts(name, x, labels, K, rows, ld): integer rows with |m| <= 50."""
    rng = np.random.default_rng(11)
    ms = lambda n: rng.integers(-50, 51, size=n)
    out = []

    def add(name, n, labels, K, dim=8, rows=None, ld=None, p0=0, p1=None):
        out.append(dict(name=name, x=integer_rows(ms(n), dim, p0, p1), labels=np.asarray(labels, dtype=np.int64), K=K, rows=rows, ld=ld))

    add("n1-k2", 1, [0], 2)
    add("n2-k2", 2, [0, 1], 2)
    add("n2-k3-one-cluster", 2, [2, 2], 3)
    add("n63-k3", 63, np.arange(63) % 3, 3)
    add("n64-k64-singletons", 64, rng.permutation(64), 64)
    add("n65-k64", 65, np.minimum(np.arange(65), 63), 64)
    add("n65-k65", 65, rng.permutation(65), 65)
    add("n257-k257-empties", 257, rng.permutation(257) % 200, 257)
    add("n257-k256", 257, np.minimum(rng.permutation(257), 255), 256)
    # cluster boundaries at partition positions 31 / 32 / 33, 63 / 64 / 65 and 255 / 256 / 257; ids 3 and 7 stay empty
    add("n300-boundaries", 300, _sizes_to_labels([31, 1, 1, 30, 1, 1, 190, 1, 1, 43], [0, 1, 2, 4, 5, 6, 8, 9, 10, 11], 12), 12)
    add("n300-k65", 300, rng.integers(0, 65, size=300), 65)
    add("n300-k299", 300, np.minimum(rng.permutation(300), 298), 299)
    add("n257-k2-dim4-ld", 257, rng.integers(0, 2, size=257), 2, dim=4, ld=12, p1=3)
    add("n300-k3-dim20", 300, rng.integers(0, 3, size=300), 3, dim=20, p0=17, p1=19)
    add("n300-k5-rows", 300, rng.integers(0, 5, size=300), 5, rows=np.array([7, 3, 299, 3, 150, 0, 64, 63]))
    add("n257-k3-rows65", 257, rng.integers(0, 3, size=257), 3, rows=rng.permutation(257)[:65])
    return out


def cosine_rows(n, seed):
    """Rows of norm 4 (or 0) with integer dot products: 1 / norm = 0.25 and every 1 - dot / 16 are exact in fp32."""
    pool = [np.eye(4)[i] * s for i in range(4) for s in (4, -4)]
    pool += [np.array([a, b, c, d]) for a in (2, -2) for b in (2, -2) for c in (2, -2) for d in (2, -2)]
    pool += [np.zeros(4)]
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 8), dtype=np.float32)
    x[:, 2:6] = np.asarray(pool)[rng.integers(0, len(pool), size=n)]
    return x


# ---- the rounding bound --------------------------------------------------------------------------------------------------------
def pair_bound(x):
    """(d, bound) (n, n) float64: the float64 distances by direct differences and, per pair, the most the fp32 distance
    sqrt(max(fma(-2, dot, xx_i + xx_j), 0)) may miss them by: min(sqrt(e), e / (2 d)) + 2^-23 d with
    e = (dim + 4) 2^-24 (2 sum |x_i| |x_j| + xx_i + xx_j) -- dim + 4 roundings of relative size 2^-24 on terms of that total size,
    whatever the order of summation -- carried through the square root, plus its own rounding."""
    x = np.asarray(x, dtype=np.float64)
    n, dim = x.shape
    d = np.zeros((n, n))
    for i in range(n):
        d[i] = np.sqrt(((x - x[i]) ** 2).sum(axis=1))
    xx = (x * x).sum(axis=1)
    ax = np.abs(x)
    e = (dim + 4) * 2.0 ** -24 * (2.0 * (ax @ ax.T) + xx[:, None] + xx[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        through = np.where(d > 0, np.minimum(np.sqrt(e), e / (2.0 * d)), np.sqrt(e))
    bound = through + 2.0 ** -23 * d
    np.fill_diagonal(bound, 0.0)
    return d, bound


def row_bounds(x, labels, K):
    """The host silhouette of every row and what the pair bound leaves of it -> dict: host (HostSilhouette), ea, eb (n,) the
    bounds on a and b, s_lo, s_hi (n,) the interval of s, safe (n,) bool: the host margin between the two nearest clusters
    exceeds the summed bounds, so `nearest` must agree."""
    x64 = np.asarray(x, dtype=np.float64)
    n = x64.shape[0]
    host = silhouette_host(x64, labels, "euclidean", K)
    d, bound = pair_bound(x64)
    onehot = np.zeros((n, K))
    onehot[np.arange(n), labels] = 1.0
    counts = onehot.sum(axis=0)
    S, E = d @ onehot, bound @ onehot
    E = E + n * 2.0 ** -52 * S                                  # the float64 additions themselves, any order
    own = labels
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(counts > 0, S / counts, np.inf)
        emean = np.where(counts > 0, E / counts, 0.0)
        ea = np.where(counts[own] > 1, E[np.arange(n), own] / (counts[own] - 1), 0.0)
    means[np.arange(n), own] = np.inf
    emean_other = emean.copy()
    emean_other[np.arange(n), own] = 0.0
    eb = emean_other.max(axis=1)
    order = np.sort(means, axis=1)
    safe = (order[:, 1] - order[:, 0]) > 2.0 * eb

    def sval(a, b):
        mx = np.maximum(a, b)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((counts[own] == 1) | (mx == 0), 0.0, (b - a) / mx)

    a_lo, a_hi = np.maximum(host.a - ea, 0.0), host.a + ea
    b_lo, b_hi = np.maximum(host.b - eb, 0.0), host.b + eb
    return dict(host=host, ea=ea, eb=eb, s_lo=sval(a_hi, b_lo), s_hi=sval(a_lo, b_hi), safe=safe)


# ---- the kernel's walk, restated -------------------------------------------------------------------------------------------------
def geometry(n, n_rows):
    """(ns, len): the ranges of partition positions acx_silhouette cuts (include/acx.h)."""
    cdiv = lambda a, b: -(-a // b)
    chunks, groups = cdiv(n, 64), cdiv(n_rows, 256)
    ns = min(16, chunks, max(1, cdiv(512, groups)))
    length = 64 * cdiv(chunks, ns)
    return cdiv(n, length), length


def walk_silhouette(x, labels, K, rows=None):
    """a, b, nearest, s as the device forms them on rows whose distances are exact in fp32: the stable partition by label, its
    positions cut into ranges, 64 columns per step, one running float64 per row flushed at each cluster boundary into slot
    (cluster + range), S(i, c) = the slots of c in ascending range; then the per-row arithmetic of silhouette_row_kernel."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    n = x.shape[0]
    q = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    m = q.size
    valid = (labels >= 0) & (labels < K)
    perm = np.concatenate([np.flatnonzero(labels == c) for c in range(K)]).astype(np.int64)
    counts = np.array([(labels == c).sum() for c in range(K)], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    npart = int(counts.sum())
    ns, length = geometry(n, m)
    d = np.zeros((m, n), dtype=np.float32)
    for t, i in enumerate(q):
        d[t] = np.sqrt(((x - x[i]) ** 2).sum(axis=1)).astype(np.float32)
        d[t, i] = 0.0
    sp = np.full((K + ns, m), np.nan)
    for split in range(ns):
        lo, hi = split * length, min(npart, (split + 1) * length)
        if lo >= hi:
            continue
        cur = max(c for c in range(K) if start[c] <= lo)
        cend = start[cur] + counts[cur]
        run = np.zeros(m)
        for p0 in range(lo, hi, 64):
            cn, c0 = min(64, hi - p0), 0
            while c0 < cn:
                ce = min(cn, cend - p0)
                for c in range(c0, ce):
                    run = run + d[:, perm[p0 + c]].astype(np.float64)
                c0 = ce
                if p0 + ce == cend:
                    sp[cur + split] = run
                    run = np.zeros(m)
                    cur += 1
                    while cur < K and counts[cur] == 0:
                        cur += 1
                    cend = start[cur] + counts[cur] if cur < K else 1 << 62
        if cur < K and start[cur] < hi:
            sp[cur + split] = run
    a, b, s = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    nearest = np.full(m, -1, dtype=np.int64)
    nonempty = int((counts > 0).sum())
    for t, i in enumerate(q):
        if not valid[i]:
            continue
        L, own, best = labels[i], 0.0, 0.0
        for c in range(K):
            if counts[c] == 0:
                continue
            s_lo, s_hi = start[c] // length, (start[c] + counts[c] - 1) // length
            S = sp[c + s_lo, t]
            for r in range(s_lo + 1, s_hi + 1):
                S = S + sp[c + r, t]
            assert np.isfinite(S)                            # every slot that is read was written
            if c == L:
                own = S
            else:
                mean = S / counts[c]
                if nearest[t] < 0 or mean < best:
                    best, nearest[t] = mean, c
        a[t] = own / (counts[L] - 1) if counts[L] > 1 else 0.0
        if nonempty < 2:
            s[t] = 0.0
            continue
        b[t] = best
        mx = max(a[t], b[t])
        s[t] = 0.0 if counts[L] == 1 or mx == 0.0 else (b[t] - a[t]) / mx
    return a, b, nearest, s
