"""Cases shared by test_neighbors_cpu.py and test_gpu_neighbors.py (pytorch/neighbors.py; acx_radius_count, acx_radius_neighbors,
acx_graph_components, acx_dbscan_labels in include/acx.h): the generators, the rounding bounds that say which pairs the fp32
kernel may decide either way, the hand-worked graphs and a Python restatement of the tile kernel's ballot and rank walk."""
import functools

import numpy as np

from audioset_convnext_inf_amd.pytorch import neighbors as nbm

U24 = 2.0 ** -24


# ---- integer rows: every dot product, sum of squares and squared distance is exact in fp32 ------------------------------------------
def int_rows(n, dim, seed):
    """(n, dim) float32 with entries in -3 .. 3."""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, dim)).astype(np.float32)


def attained_level(values, metric, fraction):
    """A level AT an attained value (so the threshold ties are exercised): the value of rank fraction * size of the sorted values;
    -> the threshold to pass (the value itself, or its square root for euclidean: integers, so sqrt(v)^2 rounds back to v in fp32)."""
    flat = np.sort(np.asarray(values, dtype=np.float64).ravel())
    v = float(flat[min(flat.size - 1, int(fraction * flat.size))])
    if metric == "euclidean":
        t = float(np.sqrt(v))
        assert float(np.float32(t * t)) == v
        return t
    return v


# (nq, n, dim, ld padding): the tile edges of both sides, every form of dot_tile's last group, a stride wider than the rows
EQUAL_SHAPES = [(1, 1, 4, 0), (63, 65, 12, 0), (64, 64, 16, 4), (65, 63, 20, 0), (255, 257, 28, 0), (256, 256, 12, 8), (257, 255, 16, 0),
                (1025, 300, 768, 0), (1, 257, 20, 0), (257, 1, 28, 4)]
EQUAL_IDS = ["%dx%d-d%d%s" % (a, b, c, "-ld" if p else "") for a, b, c, p in EQUAL_SHAPES]
SELF_SHAPES = [(1, 4), (63, 12), (64, 16), (65, 20), (255, 28), (256, 16), (257, 12), (300, 768)]


# ---- Gaussian blobs ---------------------------------------------------------------------------------------------------------------
def blobs(n, dim, K, sep, seed, dtype=np.float32):
    """x = center + N(0, 1) with center = sep * N(0, 1) per blob; -> (x (n, dim), blob (n,))."""
    rng = np.random.default_rng(seed)
    centers = sep * rng.standard_normal((K, dim))
    blob = rng.integers(0, K, size=n)
    x = centers[blob] + rng.standard_normal((n, dim))
    return x.astype(dtype), blob


# (n, dim, K, sep, seed, metric)
ROUNDED = [(2000, 768, 50, 0.5, 2, "cosine"), (2000, 768, 50, 0.5, 2, "euclidean"), (1001, 772, 33, 0.2, 7, "euclidean"),
           (4097, 768, 256, 0.3, 4, "cosine")]
ROUNDED_IDS = ["%d-d%d-%s" % (c[0], c[1], c[5]) for c in ROUNDED]
LEVELS = ("midway", "median")


@functools.lru_cache(maxsize=1)
def rounded_case(case):
    """-> dict(x, v (n, n) float64 pair values, bound (n, n), thresholds {"midway", "median"}) of a ROUNDED case: a self-join
    without the diagonal.  The bounds follow clustering_cases.score_bound: (dim + 8) 2^-24 times the sum of the magnitudes that
    enter the value, plus four roundings of the value itself for the two cosine scalings."""
    n, dim, K, sep, seed, metric = case
    x, blob = blobs(n, dim, K, sep, seed)
    x64 = x.astype(np.float64)
    a = np.abs(x64)
    mag = a @ a.T
    xx = (x64 * x64).sum(axis=1)
    if metric == "euclidean":
        v = np.maximum(xx[:, None] + xx[None, :] - 2.0 * (x64 @ x64.T), 0.0)
        bound = (dim + 8) * U24 * (2.0 * mag + xx[:, None] + xx[None, :])
    else:
        r = 1.0 / np.sqrt(xx)
        v = (x64 @ x64.T) * r[:, None] * r[None, :]
        bound = (dim + 8) * U24 * (mag * r[:, None] * r[None, :] + np.abs(v)) + 4 * U24 * np.abs(v)
    off = ~np.eye(n, dtype=bool)
    same = (blob[:, None] == blob[None, :]) & off
    within, across = v[same], v[~same & off]
    if metric == "euclidean":
        mid = 0.5 * (np.quantile(within, 0.999) + np.quantile(across, 0.001))
        thr = {"midway": float(np.sqrt(mid)), "median": float(np.sqrt(np.median(within)))}
    else:
        mid = 0.5 * (np.quantile(within, 0.001) + np.quantile(across, 0.999))
        thr = {"midway": float(mid), "median": float(np.median(within))}
    return dict(x=x, v=v, bound=bound, thresholds=thr, metric=metric, off=off)


def decided(case, which):
    """-> (threshold, keep (n, n) bool: the pairs the host keeps, undecided (n, n) bool) of a ROUNDED case at one of its levels."""
    c = rounded_case(case)
    thr = c["thresholds"][which]
    level = float(nbm.level_of(thr, c["metric"]))
    keep = (c["v"] <= level if c["metric"] == "euclidean" else c["v"] >= level) & c["off"]
    undecided = (np.abs(c["v"] - level) <= c["bound"]) & c["off"]
    return thr, keep, undecided


def csr_mask(offsets, indices, nq, n):
    """The (nq, n) bool mask of a CSR list (and a check of its form: ascending inside each row)."""
    offsets, indices = np.asarray(offsets), np.asarray(indices)
    assert offsets.shape == (nq + 1,) and offsets[0] == 0 and (np.diff(offsets) >= 0).all() and offsets[-1] == indices.size
    rows = np.repeat(np.arange(nq), np.diff(offsets))
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(indices)[same_row] > 0).all()
    mask = np.zeros((nq, n), dtype=bool)
    mask[rows, indices] = True
    return mask


# ---- planted duplicates -----------------------------------------------------------------------------------------------------------
def planted(n=1500, dim=768, sources=200, noise=1e-3, seed=11):
    """n random rows plus 2 .. 5 copies of `sources` of them with relative noise, shuffled; -> (x float32, group (rows,) int64: the
    smallest row index of each row's planted group, held-out (one more copy of every source, unshuffled), source_rows (where each
    held-out row's source and its copies sit after the shuffle, as a list of sorted arrays))."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, dim))
    src = rng.choice(n, size=sources, replace=False)
    rows, origin = [base], [np.arange(n)]
    for s in src:
        k = int(rng.integers(2, 6))
        rows.append(base[s] * (1.0 + noise * rng.standard_normal((k, dim))))
        origin.append(np.full(k, s))
    x, origin = np.concatenate(rows), np.concatenate(origin)
    perm = rng.permutation(x.shape[0])
    x, origin = x[perm], origin[perm]
    group = np.empty(x.shape[0], dtype=np.int64)
    for o in np.unique(origin):
        members = np.nonzero(origin == o)[0]
        group[members] = members.min()
    held = base[src] * (1.0 + noise * rng.standard_normal((sources, dim)))
    source_rows = [np.nonzero(origin == s)[0] for s in src]
    return x.astype(np.float32), group, held.astype(np.float32), source_rows


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
def csr_of(n, edges):
    """(offsets int64, indices int32) of directed entries (i -> j), each row ascending."""
    rows = [[] for _ in range(n)]
    for i, j in edges:
        rows[i].append(j)
    counts = [len(r) for r in rows]
    flat = [j for r in rows for j in sorted(r)]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(flat, dtype=np.int32)


def both(edges):
    return list(edges) + [(j, i) for i, j in edges]


def path_graph(n, seed=None):
    """A path over n nodes, in index order (seed None) or through a shuffled order; both directions listed."""
    order = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    return csr_of(n, both(list(zip(order[:-1].tolist(), order[1:].tolist()))))


def graph_cases():
    """name -> (offsets, indices, n, expected labels or None (then components_host is the reference))."""
    clique_a = [(i, j) for i in range(2, 6) for j in range(2, 6) if i < j]
    clique_b = [(i, j) for i in range(7, 11) for j in range(7, 11) if i < j]
    out = {
        "isolated": csr_of(5, []) + (5, np.arange(5)),
        "path": path_graph(9) + (9, np.zeros(9, dtype=np.int64)),
        "path-shuffled": path_graph(33, seed=3) + (33, np.zeros(33, dtype=np.int64)),
        "star": csr_of(8, both([(5, j) for j in range(8) if j != 5 and j != 0])) + (8, np.array([0, 1, 1, 1, 1, 1, 1, 1])),
        # nodes 0, 1, 6, 11 alone; cliques {2..5} and {7..10} joined by the bridge 5 - 7
        "cliques-bridge": csr_of(12, both(clique_a + clique_b + [(5, 7)])) + (12, np.array([0, 1, 2, 2, 2, 2, 6, 2, 2, 2, 2, 11])),
        # only (j -> i) is listed: still one edge
        "asymmetric": csr_of(6, [(4, 1), (5, 4), (3, 2)]) + (6, np.array([0, 1, 2, 2, 1, 1])),
    }
    return out


def grid_points():
    """Integer-grid points (exact distances): two dense 5 x 5 blocks, a bridge of border points between them (spacing 2, so each
    bridge point has fewer neighbours), a dense 3 x 3 block far away and isolated noise.  float32 (m, 4) with two zero columns."""
    pts = [(a, b) for a in range(5) for b in range(5)]
    pts += [(a + 12, b) for a in range(5) for b in range(5)]
    pts += [(6, 2), (8, 2), (10, 2)]
    pts += [(a + 30, b + 30) for a in range(3) for b in range(3)]
    pts += [(50, 0), (0, 50), (-20, -20), (60, 60)]
    rng = np.random.default_rng(5)
    p = np.asarray(pts, dtype=np.float32)[rng.permutation(len(pts))]
    return np.concatenate([p, np.zeros_like(p)], axis=1)


# ---- the tile kernel's walk ---------------------------------------------------------------------------------------------------------
def tile_row(i, h):
    """F32Tile<32>::row (device_common.h): the tile row of accumulator register i in lane half h."""
    return (i & 3) + 8 * (i >> 2) + 4 * h


def geometry(nq, n, slices=0):
    """(ns, len): the ranges of database rows (include/acx.h)."""
    chunks, groups = -(-n // 64), -(-nq // 256)
    most = min(64, chunks)
    if slices > 0:
        length = 64 * -(-chunks // min(slices, most))
    else:
        # the busiest of 256 compute units takes ceil(groups * ns / 256) workgroups of `length` rows: the smallest product wins,
        # the largest ns among equals
        best = None
        for ns in range(1, most + 1):
            cand = 64 * -(-chunks // ns)
            cost = -(-(groups * -(-n // cand)) // 256) * cand
            if best is None or cost <= best:
                best, length = cost, cand
    return -(-n // length), length


def walk_radius(keep, slices=0):
    """The count pass, the scan in (query, range) order and the emit pass of radius_tile_kernel on a given (nq, n) keep mask,
    ballot by ballot: a wave owns 64 queries and streams a range 64 columns per step; for accumulator register i of tile half t
    and column half u, the ballot's low word holds the 32 columns of tile row row(i, 0), its high word those of row(i, 1); a kept
    pair's place is its row's running count + the kept columns of the row's u = 0 word (for u = 1) + the popcount below its own
    bit.  -> (offsets, indices)."""
    nq, n = keep.shape
    ns, length = geometry(nq, n, slices)
    part = np.zeros((nq, ns), dtype=np.int64)
    indices = None
    for emit in (False, True):
        if emit:
            pos = np.concatenate([[0], np.cumsum(part.ravel())])
            offsets = np.append(pos[np.arange(nq) * ns], pos[-1])
            indices = np.full(int(pos[-1]), -1, dtype=np.int64)
        for q0 in range(0, nq, 64):
            for split in range(ns):
                lo, hi = split * length, min(n, (split + 1) * length)
                run = np.zeros(64, dtype=np.int64)                   # lane r carries tile row r
                if emit:
                    for r in range(64):
                        if q0 + r < nq:
                            run[r] = pos[(q0 + r) * ns + split]
                for j0 in range(lo, hi, 64):
                    for t in range(2):
                        for i in range(16):
                            words = np.zeros((2, 2), dtype=np.uint64)        # [u][h]
                            for u in range(2):
                                for h in range(2):
                                    qg = q0 + 32 * t + tile_row(i, h)
                                    for r32 in range(32):
                                        j = j0 + 32 * u + r32
                                        if qg < nq and j < hi and keep[qg, j]:
                                            words[u][h] |= np.uint64(1) << np.uint64(r32)
                            for h in range(2):
                                row = 32 * t + tile_row(i, h)
                                w0, w1 = int(words[0][h]), int(words[1][h])
                                if emit:
                                    base = run[row]
                                    for r32 in range(32):
                                        below = (1 << r32) - 1
                                        if (w0 >> r32) & 1:
                                            indices[base + bin(w0 & below).count("1")] = j0 + r32
                                        if (w1 >> r32) & 1:
                                            indices[base + bin(w0).count("1") + bin(w1 & below).count("1")] = j0 + 32 + r32
                                run[row] += bin(w0).count("1") + bin(w1).count("1")
                if not emit:
                    for r in range(64):
                        if q0 + r < nq:
                            part[q0 + r, split] = run[r]
    return offsets, indices
