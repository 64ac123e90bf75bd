#!/usr/bin/env python
"""K-means on the GPU (pytorch/clustering.py, csrc/kmeans.hip) against stock torch on the same device and scikit-learn on the
host: the measurements behind profiles/r23_a_cluster_bench.txt.

    python tools/cluster_bench.py [--out profiles/r23_a_cluster_bench.txt] [--shapes 0,1,2] [--fit-iters 30]

(a) one Lloyd iteration (acx_kmeans_assign + acx_kmeans_update on resident data) and a whole fit (kmeans(init=c0)), against the
    best stock-torch form of the same: addmm / cdist + argmin + index_add_, eager and as a torch.cuda.graph replay of
    one captured iteration; the stock fit is the eager loop with its per-iteration convergence test on the host.  dim 768, shapes
    (20 371, 50), (200 000, 256), (200 000, 4 096).  Every shape warmed up, the contenders alternate, medians of five windows
    between device events.  Peak device memory above the inputs, both sides.
(b) against sklearn.cluster.KMeans(init=same centres, n_init=1, algorithm="lloyd") from host arrays, copies included (the first
    two shapes; recorded, no target).
(c) k-means++ seeding (acx_kmeans_seed) per shape and its share of seeding + fit (recorded, no target).
(d) the assignment kernel alone: 2 n K dim flop over its time against the 157.3 TFLOP/s f32-matrix peak (recorded).
bench.py against the parent is run beside this tool and kept in the same profile; this tool rewrites only its own --out file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                    # noqa: E402
import torch                          # noqa: E402

from audioset_convnext_inf_amd import _ffi                                   # noqa: E402
from audioset_convnext_inf_amd._ffi import vp                                # noqa: E402
from audioset_convnext_inf_amd.pytorch import clustering as cl               # noqa: E402

SHAPES = [(20371, 50, "AudioSet eval-sized, 50 clusters"), (200000, 256, "200 k clips, 256 clusters"),
          (200000, 4096, "200 k clips, a 4 096-entry codebook")]
DIM = 768
F32_MATRIX_PEAK = 157.3e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, K):
    """Blobs with as many true clusters as K / 2 (so that k-means has work to do), on the device."""
    g = torch.Generator(device="cuda").manual_seed(n + K)
    tk = max(2, K // 2)
    mu = torch.randn(tk, DIM, generator=g, device="cuda")
    lab = torch.randint(0, tk, (n,), generator=g, device="cuda")
    x = mu[lab] + torch.randn(n, DIM, generator=g, device="cuda")
    c0 = x[torch.randperm(n, generator=g, device="cuda")[:K]].clone()
    return x, c0


def window(fn, reps):
    """ms per call of fn over `reps` calls between device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def medians(contenders, reps, repeats=5):
    """{name: median ms} with the contenders alternating inside each repeat."""
    got = {k: [] for k in contenders}
    for _ in range(repeats):
        for k, fn in contenders.items():
            got[k].append(window(fn, reps))
    return {k: statistics.median(v) for k, v in got.items()}


class Ours:
    def __init__(self, x, c0):
        self.x, self.c = x, c0.clone()
        n, K = x.shape[0], c0.shape[0]
        self.n, self.K = n, K
        dev = x.device
        self.labels = torch.empty(n, dtype=torch.int32, device=dev)
        self.scores = torch.empty(n, dtype=torch.float32, device=dev)
        self.counts = torch.empty(K, dtype=torch.int32, device=dev)
        self.words = torch.zeros(4, dtype=torch.int32, device=dev)
        self.shift = torch.zeros(1, dtype=torch.float64, device=dev)
        self.ws_bytes = _ffi.kmeans_workspace_bytes(n, DIM, K)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.stream = _ffi.stream_ptr(dev)

    def assign(self):
        _ffi.kmeans_assign(vp(self.x), self.x.stride(0), None, self.n, vp(self.c), self.c.stride(0), self.K, DIM, 0, None,
                           vp(self.labels), vp(self.scores), vp(self.words[1:]), vp(self.words), self.stream)

    def iteration(self):
        self.assign()
        _ffi.kmeans_update(vp(self.x), self.x.stride(0), None, self.n, DIM, 0, vp(self.labels), self.K, vp(self.c), self.c.stride(0),
                           vp(self.counts), vp(self.shift), vp(self.words[2:]), (vp(self.ws), self.ws_bytes), self.stream)


class Stock:
    """The stock-torch Lloyd iteration: form = "addmm" (cc - 2 x c^T) or "cdist"."""

    def __init__(self, x, c0, form):
        self.x, self.c, self.form = x, c0.clone(), form
        self.K = c0.shape[0]
        self.ones = torch.ones(x.shape[0], device=x.device)
        self.graph = None

    def iteration(self):
        x, c = self.x, self.c
        if self.form == "addmm":
            d = torch.addmm((c * c).sum(1)[None, :], x, c.t(), alpha=-2.0)
        else:
            d = torch.cdist(x, c)
        lab = d.argmin(1)
        sums = torch.zeros_like(c).index_add_(0, lab, x)
        cnt = torch.zeros(self.K, device=x.device).index_add_(0, lab, self.ones)       # (bincount synchronises: not capturable)
        new = torch.where(cnt[:, None] > 0, sums / cnt.clamp_min(1)[:, None], c)
        self.shift = ((new - c) ** 2).sum()
        self.lab = lab
        c.copy_(new)

    def capture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self.iteration()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.iteration()

    def replay(self):
        self.graph.replay()


def stock_fit(x, c0, form, max_iter, tol_abs):
    s = Stock(x, c0, form)
    old = None
    it = 0
    for it in range(1, max_iter + 1):
        s.iteration()
        same = old is not None and bool((s.lab == old).all())           # the host decides: one synchronisation per iteration
        if same or float(s.shift) <= tol_abs:
            break
        old = s.lab
    return it


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_a_cluster_bench.txt"))
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--fit-iters", type=int, default=30)
    ap.add_argument("--sklearn", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_bench needs a GPU: nothing is measured without one")
    say("cluster_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for si in [int(v) for v in a.shapes.split(",")]:
        n, K, what = SHAPES[si]
        say()
        say("== shape %d: n %d, K %d, dim %d (%s)" % (si, n, K, DIM, what))
        x, c0 = make_data(n, K)
        ours = Ours(x, c0)
        stock = {f: Stock(x, c0, f) for f in ("addmm", "cdist")}
        graphs = {f: Stock(x, c0, f) for f in ("addmm", "cdist")}
        for s in graphs.values():
            s.capture()
        ours.iteration()
        for s in stock.values():
            s.iteration()
        torch.cuda.synchronize()
        t0 = window(ours.iteration, 2)
        reps = max(3, int(300.0 / max(t0, 0.05)))                       # windows of about 0.3 s of our iteration
        reps = min(reps, 2000)
        # (a) one iteration
        cont = {"ours": ours.iteration}
        for f in stock:
            cont["torch %s eager" % f] = stock[f].iteration
            cont["torch %s graph" % f] = graphs[f].replay
        med = medians(cont, reps)
        best = min((v, k) for k, v in med.items() if k != "ours")
        say("(a) one Lloyd iteration, median of 5 windows of %d iterations:" % reps)
        for k, v in med.items():
            say("      %-20s %9.3f ms" % (k, v))
        say("    ours against the best stock form (%s): %.2fx  [>= 1.0x]" % (best[1], best[0] / med["ours"]))
        # (d) the assignment alone
        ta = medians({"assign": ours.assign}, reps)["assign"]
        say("(d) assignment kernel alone: %.3f ms = %.1f %% of the 157.3 TFLOP/s f32-matrix peak (2 n K dim flop)"
            % (ta, 2.0 * n * K * DIM / (ta * 1e-3) / F32_MATRIX_PEAK * 100))
        # (a) a whole fit
        tol = 1e-4
        tol_abs = tol * float(x.double().var(dim=0, unbiased=False).mean())
        km = cl.kmeans(x, K, init=c0, max_iter=a.fit_iters, tol=tol)
        torch.cuda.synchronize()
        its_ours = int(km.n_iter)
        form = best[1].split()[1]
        its_stock = stock_fit(x, c0, form, a.fit_iters, tol_abs)
        fits = {"ours": [], "stock": []}
        for _ in range(5):
            t = time.perf_counter()
            km = cl.kmeans(x, K, init=c0, max_iter=a.fit_iters, tol=tol)
            int(km.n_iter)                                              # the first read synchronises
            fits["ours"].append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            stock_fit(x, c0, form, a.fit_iters, tol_abs)
            torch.cuda.synchronize()
            fits["stock"].append((time.perf_counter() - t) * 1e3)
        fo, fs = statistics.median(fits["ours"]), statistics.median(fits["stock"])
        say("(a) whole fit (init given, tol 1e-4, max_iter %d), host clock to the first synchronised read, median of 5:" % a.fit_iters)
        say("      ours %9.2f ms (%d iterations; all %d queued)   torch %s eager loop %9.2f ms (%d iterations)   %.2fx  [>= 1.0x]"
            % (fo, its_ours, a.fit_iters, form, fs, its_stock, fs / fo))
        mo = peak_above(lambda: cl.kmeans(x, K, init=c0, max_iter=a.fit_iters, tol=tol))
        ms = peak_above(lambda: stock_fit(x, c0, form, a.fit_iters, tol_abs))
        say("    peak device memory above the inputs: ours %.1f MiB, stock %.1f MiB (the n x K matrix is %.1f MiB)  [ours lower]"
            % (mo, ms, n * K * 4 / 2 ** 20))
        # (c) seeding
        u = torch.from_numpy(np.random.default_rng(0).random(K + 1)).cuda()
        picked = torch.empty(K, dtype=torch.int32, device="cuda")
        cs = torch.empty((K, DIM), dtype=torch.float32, device="cuda")

        def seed():
            _ffi.kmeans_seed(vp(x), x.stride(0), None, n, DIM, 0, K, vp(u), vp(picked), vp(cs), cs.stride(0), vp(ours.words[3:]),
                             (vp(ours.ws), ours.ws_bytes), ours.stream)
        seed()
        torch.cuda.synchronize()
        tsd = statistics.median([window(seed, 1) for _ in range(3)])
        say("(c) k-means++ seeding: %.2f ms for %d rounds = %.0f %% of seeding + fit" % (tsd, K, 100 * tsd / (tsd + fo)))
        # (b) scikit-learn from host arrays
        if a.sklearn and si < 2:
            try:
                from sklearn.cluster import KMeans as SK
            except ImportError:
                say("(b) scikit-learn is not installed: not measured")
            else:
                xh, ch = x.cpu().numpy(), c0.cpu().numpy()
                t = time.perf_counter()
                sk = SK(K, init=ch, n_init=1, algorithm="lloyd", max_iter=a.fit_iters, tol=tol).fit(xh)
                tsk = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                km = cl.kmeans(xh, K, init=ch, max_iter=a.fit_iters, tol=tol, device="cuda")
                lab = km.labels.cpu()
                tours = (time.perf_counter() - t) * 1e3
                agree = float((lab.numpy() == sk.labels_).mean())
                say("(b) from host arrays, copies included: sklearn %.1f ms (%d iterations), ours %.1f ms (%d iterations): %.1fx; "
                    "%.2f %% of the labels equal" % (tsk, sk.n_iter_, tours, int(km.n_iter), tsk / tours, 100 * agree))
        del ours, stock, graphs, x, c0
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
