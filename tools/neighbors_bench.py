#!/usr/bin/env python
"""Radius search, duplicate groups and DBSCAN on the GPU (pytorch/neighbors.py, csrc/neighbors.hip) against stock torch on the same
device and scikit-learn on the host: the measurements behind profiles/r32_a_neighbors_bench.txt.

    python tools/neighbors_bench.py [--out profiles/r32_a_neighbors_bench.txt] [--shapes 0,1] [--sklearn 1]

(a) acx_radius_count, a cosine self-join on resident rows, against the best stock-torch form of the same: (xn[a:b] @ xn.T >=
    t).sum(1) on normalised rows in chunks of 2 048 / 8 192 queries.  dim 768, n 20 371 and 200 000.  Every shape warmed up, the
    contenders alternate, medians of five windows between device events.  Only the first shape carries a requirement: ours >= 1.0x
    the best stock form.  Peak device memory above the inputs on both sides, and the call's share of the 157.3 TFLOP/s f32-matrix
    peak by its algorithmic flop (2 n n dim).
(b) acx_radius_neighbors at thresholds that keep about 1, 30 and 1 000 neighbours per row (n 20 371): the count pass
    (acx_radius_count) against the whole call (count, scan, emit) into a buffer of the list's size, and the Python call itself
    (count and scan, the total read back, the list allocated, acx_radius_emit).
(c) duplicate_groups and dbscan end to end from host arrays, copies included, against a host union-find over numpy's chunked
    products and sklearn.cluster.DBSCAN(algorithm="brute"), n 20 371 (recorded).
(d) acx_graph_components: rounds until stable and the time of a call of 32 queued rounds, on the duplicate graph of (c) and on a
    shuffled path of 4 097 nodes; rounds until stable on the tests' hand-worked graphs.
(f) the cases of tests/neighbors_cases.py: the undecided share of each and the pairs on which the device differs from the host.
bench.py against the parent and the kernels' register counts are taken beside this tool and kept in the same profile; this tool
rewrites only its own --out file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                    # noqa: E402
import torch                          # noqa: E402

from audioset_convnext_inf_amd import _ffi                                   # noqa: E402
from audioset_convnext_inf_amd._ffi import vp                                # noqa: E402
from audioset_convnext_inf_amd.pytorch import neighbors as nbm              # noqa: E402
from audioset_convnext_inf_amd.pytorch import retrieval                     # noqa: E402

SHAPES = [(20371, 50, "AudioSet eval-sized"), (200000, 256, "200 k clips")]
DIM = 768
F32_MATRIX_PEAK = 157.3e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, K):
    g = torch.Generator(device="cuda").manual_seed(n + K)
    mu = torch.randn(K, DIM, generator=g, device="cuda")
    lab = torch.randint(0, K, (n,), generator=g, device="cuda")
    return mu[lab] + torch.randn(n, DIM, generator=g, device="cuda")


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def medians(contenders, reps, repeats=5):
    """{name: median ms} with the contenders alternating inside each repeat; a contender slower than 200 ms / reps per call gets
    shorter windows of its own (at least one call)."""
    own = {}
    for k, fn in contenders.items():
        t = window(fn, 1)
        own[k] = max(1, min(reps, int(200.0 / max(t, 0.05))))
    got = {k: [] for k in contenders}
    for _ in range(repeats):
        for k, fn in contenders.items():
            got[k].append(window(fn, own[k]))
    return {k: statistics.median(v) for k, v in got.items()}


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


class Count:
    """acx_radius_count, a self-join on resident rows and inverse norms, preallocated outputs."""

    def __init__(self, x, rx, level):
        self.x, self.rx, self.level, self.n = x, rx, float(level), x.shape[0]
        dev = x.device
        self.counts = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.st = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws_bytes = _ffi.radius_workspace_bytes(self.n, self.n, 0)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.stream = _ffi.stream_ptr(dev)

    def run(self):
        _ffi.radius_count(vp(self.x), self.x.stride(0), vp(self.rx), self.n, vp(self.x), self.x.stride(0), vp(self.rx), self.n, DIM,
                          _ffi.RADIUS_COSINE, self.level, _ffi.RADIUS_SELF_EXCLUDE, vp(self.counts), vp(self.st),
                          (vp(self.ws), self.ws_bytes), self.stream)


class Lists(Count):
    """acx_radius_neighbors into a buffer of `capacity` entries."""

    def __init__(self, x, rx, level, capacity):
        super().__init__(x, rx, level)
        dev = x.device
        self.cap = int(capacity)
        self.off = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self.idx = torch.empty(max(self.cap, 1), dtype=torch.int32, device=dev)
        self.val = torch.empty(max(self.cap, 1), dtype=torch.float32, device=dev)
        self.total = torch.empty(1, dtype=torch.int64, device=dev)

    def run(self):
        _ffi.radius_neighbors(vp(self.x), self.x.stride(0), vp(self.rx), self.n, vp(self.x), self.x.stride(0), vp(self.rx), self.n, DIM,
                              _ffi.RADIUS_COSINE, self.level, _ffi.RADIUS_SELF_EXCLUDE, 0, vp(self.off), vp(self.idx), vp(self.val),
                              self.cap, vp(self.total), vp(self.st), (vp(self.ws), self.ws_bytes), self.stream)


def stock_count(xn, t, chunk):
    """The stock-torch count: chunks of normalised query rows against every row, the chunk of scores compared and summed."""
    n = xn.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=xn.device)
    for a in range(0, n, chunk):
        out[a:a + chunk] = (xn[a:a + chunk] @ xn.T >= t).sum(1)
    return out - 1                                       # the row itself


def level_for(xn, per_row):
    """A cosine level that keeps about per_row neighbours per row, from the scores of its first 512 rows (64 past 50 000 rows)."""
    n = xn.shape[0]
    s = (xn[:512 if n <= 50000 else 64] @ xn.T).flatten()
    k = max(1, int(round(s.numel() * (1.0 - (per_row + 1.0) / n))))
    return float(torch.kthvalue(s, min(k, s.numel())).values)


def rounds_until_stable(offsets, indices32, n):
    lab, rounds = None, 0
    while True:
        st = torch.zeros(1, dtype=torch.int32, device=offsets.device)
        lab = nbm.components(offsets, indices32, n, st, 1, lab)
        rounds += 1
        if not int(st.cpu()[0]) & _ffi.GRAPH_NOT_CONVERGED:
            return rounds, lab


def section_counts(si):
    n, K, what = SHAPES[si]
    say()
    say("== shape %d: n %d, dim %d, %d blobs (%s)" % (si, n, DIM, K, what))
    x = make_data(n, K)
    rx = retrieval.row_norms(x)
    xn = x * rx[:, None]
    t = level_for(xn, 30)
    ours = Count(x, rx, t)
    ours.run()
    ref = stock_count(xn, t, 2048)
    differ = int((ours.counts.long() != ref).sum())
    say("    cosine level %.6f: %.1f neighbours per row; rows whose count differs from stock torch's (other rounding): %d; status %d"
        % (t, float(ours.counts.float().mean()), differ, int(ours.st)))
    cont = {"ours": ours.run}
    for chunk in (2048, 8192):
        cont["torch (xn[a:b] @ xn.T >= t).sum(1), chunk %d" % chunk] = lambda c=chunk: stock_count(xn, t, c)
    med = medians(cont, 50)
    best = min((v, k) for k, v in med.items() if k != "ours")
    say("(a) radius_count self-join, median of 5 alternating windows:")
    for k, v in med.items():
        say("      %-52s %10.3f ms" % (k, v))
    say("    ours against the best stock form (%s): %.2fx%s" % (best[1], best[0] / med["ours"], "  [>= 1.0x]" if si == 0 else ""))
    mo = peak_above(ours.run)
    ms = peak_above(lambda: stock_count(xn, t, int(best[1].split("chunk ")[1])))
    say("    peak device memory above the inputs: ours %.1f MiB beside its %.1f MiB workspace, stock %.1f MiB (beside the normalised "
        "copy of the rows, %.1f MiB); the n x n fp32 scores would be %.0f MiB" % (mo, ours.ws_bytes / 2 ** 20, ms, n * DIM * 4 / 2 ** 20,
                                                                                  n * n * 4 / 2 ** 20))
    flop = 2.0 * n * n * DIM
    say("    the whole call: %.3f ms = %.1f %% of the 157.3 TFLOP/s f32-matrix peak (2 n n dim flop)"
        % (med["ours"], flop / (med["ours"] * 1e-3) / F32_MATRIX_PEAK * 100))
    if si == 0:
        say("(b) radius_neighbors, n %d: the count pass against the whole call (count, scan, emit)" % n)
        for per_row in (1, 30, 1000):
            lv = level_for(xn, per_row)
            c = Count(x, rx, lv)
            c.run()
            total = int(c.counts.sum().cpu())
            full = Lists(x, rx, lv, total)
            full.run()
            assert int(full.total.cpu()) == total and int(full.st.cpu()) == 0
            st = torch.zeros(1, dtype=torch.int32, device="cuda")

            def python_call():
                nbm._neighbors_rows(x, rx, x, rx, "cosine", lv, _ffi.RADIUS_SELF_EXCLUDE, st)
            m = medians({"count": c.run, "list": full.run, "python": python_call}, 50)
            say("      level %.6f, %8.1f per row, %10d entries: count %8.3f ms, whole call %8.3f ms (emit and scan: %.3f ms); "
                "radius_neighbors() itself (count, read the total, allocate, emit) %8.3f ms"
                % (lv, total / n, total, m["count"], m["list"], m["list"] - m["count"], m["python"]))
    del x, xn, rx, ours
    torch.cuda.empty_cache()


def section_end_to_end(use_sklearn):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import neighbors_cases as cases
    n = 20371
    say()
    say("(c) end to end from host arrays, copies included, n %d (planted duplicates: 2-5 copies of 2 000 rows, relative noise 1e-3)" % n)
    x, group, _, _ = cases.planted(n - 7000, DIM, 2000, 1e-3, 3)
    x = x[:n]
    nbm.duplicate_groups(x[:512], 0.95, device="cuda").check()          # warm-up
    t = time.perf_counter()
    dup = nbm.duplicate_groups(x, 0.95, device="cuda").check()
    labels = dup.labels.cpu().numpy()
    t_ours = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    rows, cols = [], []
    for a in range(0, x.shape[0], 2048):
        r, c = np.nonzero(xn[a:a + 2048] @ xn.T >= 0.95)
        rows.append(r + a)
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    keep = rows != cols
    cnt = np.bincount(rows[keep], minlength=x.shape[0])
    host = nbm.components_host(np.concatenate([[0], np.cumsum(cnt)]), cols[keep])
    t_host = (time.perf_counter() - t) * 1e3
    say("    duplicate_groups: ours %.1f ms, numpy chunked products + union-find %.1f ms: %.1fx; labels equal: %s; groups of two or "
        "more: %d" % (t_ours, t_host, t_host / t_ours, bool((labels == host).all()), len(dup.groups())))
    g = torch.Generator(device="cpu").manual_seed(5)
    mu = torch.randn(50, DIM, generator=g)
    xb = (mu[torch.randint(0, 50, (n,), generator=g)] + torch.randn(n, DIM, generator=g)).numpy()
    eps = 38.5
    nbm.dbscan(xb[:512], eps, 5, device="cuda").check()
    t = time.perf_counter()
    db = nbm.dbscan(xb, eps, 5, device="cuda").check()
    lab = db.labels.cpu().numpy()
    t_ours = (time.perf_counter() - t) * 1e3
    say("    dbscan(eps %.1f, min_samples 5): ours %.1f ms; clusters %d, noise %d, %.1f neighbours per row"
        % (eps, t_ours, int(db.clusters.cpu()), int((lab < 0).sum()), float(db.counts.float().mean())))
    if use_sklearn:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            say("    scikit-learn is not installed: not measured")
        else:
            t = time.perf_counter()
            sk = DBSCAN(eps=eps, min_samples=5, algorithm="brute").fit(xb)
            t_sk = (time.perf_counter() - t) * 1e3
            say("    sklearn DBSCAN(algorithm='brute') %.1f ms: %.1fx; rows whose label differs (pairs at the rounding of eps): %d"
                % (t_sk, t_sk / t_ours, int((sk.labels_ != lab).sum())))
    say("(d) acx_graph_components")
    nb = dup.neighbors
    rounds, _ = rounds_until_stable(nb.offsets, nb.indices32, x.shape[0])
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    m = medians({"call": lambda: nbm.components(nb.offsets, nb.indices32, x.shape[0], st)}, 20)
    say("      the duplicate graph (%d rows, %d entries): stable after %d rounds (the last one finds nothing to do); a call of %d "
        "queued rounds %.3f ms" % (x.shape[0], nb.total, rounds, nbm.MAX_ROUNDS, m["call"]))
    for name, (goff, gidx, gn, _) in sorted(cases.graph_cases().items()):
        goff, gidx = torch.as_tensor(goff).cuda(), torch.as_tensor(gidx).cuda()
        say("      hand-worked graph %-16s (%2d nodes): stable after %d rounds" % (name, gn, rounds_until_stable(goff, gidx, gn)[0]))
    off, idx = cases.path_graph(4097, seed=9)
    off, idx = torch.as_tensor(off).cuda(), torch.as_tensor(idx).cuda()
    rounds, _ = rounds_until_stable(off, idx, 4097)
    m = medians({"call": lambda: nbm.components(off, idx, 4097, st)}, 20)
    say("      a shuffled path of 4 097 nodes: stable after %d rounds; a call of %d queued rounds %.3f ms" % (rounds, nbm.MAX_ROUNDS,
                                                                                                               m["call"]))
    say("(f) the rounded cases of the tests: undecided pairs (host, by the fp32 rounding bound) and pairs where the device differs")
    worst = 0.0
    for case in cases.ROUNDED:
        for which in cases.LEVELS:
            thr, keep, undecided = cases.decided(case, which)
            got = nbm.radius_neighbors(None, torch.as_tensor(cases.rounded_case(case)["x"]).cuda(), thr, case[5]).check()
            mask = cases.csr_mask(got.offsets.cpu().numpy(), got.indices.cpu().numpy(), case[0], case[0])
            differ = mask != keep
            assert not (differ & ~undecided).any()
            worst = max(worst, undecided.sum() / keep.sum())
            say("      %-36s %-7s kept %8d, undecided %6d = %.3f %%, device differs on %d" % (case, which, keep.sum(), undecided.sum(),
                                                                                              100 * undecided.sum() / keep.sum(),
                                                                                              differ.sum()))
    say("    worst undecided share: %.3f %% (the tests require <= 1 %%)" % (100 * worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_a_neighbors_bench.txt"))
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--sklearn", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neighbors_bench needs a GPU: nothing is measured without one")
    say("neighbors_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for si in [int(v) for v in a.shapes.split(",") if v != ""]:
        section_counts(si)
    section_end_to_end(a.sklearn)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
