#!/usr/bin/env python
"""Cluster validation on the GPU (pytorch/cluster_scores.py, csrc/cluster_scores.hip) against stock torch on the same device and
scikit-learn on the host: the measurements behind profiles/r31_a_cluster_scores_bench.txt.

    python tools/cluster_scores_bench.py [--out profiles/r31_a_cluster_scores_bench.txt] [--shapes 0,1,2] [--sklearn 1]

(a) the silhouette (acx_silhouette on resident rows and labels) against the best stock-torch form of the same: chunked
    torch.cdist in float64, the chunk reduced per cluster by index_add_ or by a product with the one-hot labels.  dim 768, shapes
    (n 20 371, K 50), (2 000, 10) and (100 000, 256) with 10 000 sampled rows.  Every shape warmed up, the contenders alternate,
    medians of five windows between device events.  Only the first shape carries a requirement: ours >= 1.0x the best stock form.
(b) peak device memory above the inputs, both sides.
(c) from host arrays, copies included, against sklearn.metrics.silhouette_score (recorded).
(d) the call's share of the 157.3 TFLOP/s f32-matrix peak by its algorithmic flop (2 rows n dim), and the share of its time spent in
    the LDS walk: the same call through build/lab/libacx_nowalk.so (tools/lab/build_silhouette_lab.sh), where the walk reads one
    column per cluster segment.
(e) acx_cluster_dispersion and acx_contingency per shape (recorded).
bench.py against the parent is run beside this tool and kept in the same profile; this tool rewrites only its own --out file."""
import argparse
import ctypes
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
from audioset_convnext_inf_amd.pytorch import cluster_scores as cs           # noqa: E402

SHAPES = [(20371, 50, None, "AudioSet eval-sized, 50 clusters"), (2000, 10, None, "2 000 clips, 10 clusters"),
          (100000, 256, 10000, "100 k clips, 256 clusters, 10 000 sampled rows")]
DIM = 768
F32_MATRIX_PEAK = 157.3e12
LAB_LIB = os.path.join(ROOT, "build", "lab", "libacx_nowalk.so")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, K):
    g = torch.Generator(device="cuda").manual_seed(n + K)
    mu = torch.randn(K, DIM, generator=g, device="cuda")
    lab = torch.randint(0, K, (n,), generator=g, device="cuda")
    return mu[lab] + torch.randn(n, DIM, generator=g, device="cuda"), lab.to(torch.int32)


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


class Ours:
    """acx_silhouette on resident inputs and preallocated outputs; lib: another build of the library (the ablation)."""

    def __init__(self, x, lab, K, rows, lib=None):
        self.x, self.lab, self.K, self.rows = x, lab, K, rows
        self.n = x.shape[0]
        self.m = self.n if rows is None else rows.shape[0]
        dev = x.device
        self.out = torch.empty((3, self.m), dtype=torch.float64, device=dev)
        self.near = torch.empty(self.m, dtype=torch.int32, device=dev)
        self.means = torch.empty(K + 1, dtype=torch.float64, device=dev)
        self.st = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws_bytes = _ffi.cluster_scores_workspace_bytes(self.n, DIM, K)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.stream = _ffi.stream_ptr(dev)
        self.fn = (lib or _ffi.lib()).acx_silhouette

    def run(self):
        _ffi.check(self.fn(vp(self.x), self.x.stride(0), None, self.n, DIM, 0, vp(self.lab), self.K, vp(self.rows), self.m,
                           vp(self.out[0]), vp(self.out[1]), vp(self.near), vp(self.out[2]), vp(self.means), vp(self.means[self.K:]),
                           vp(self.st), vp(self.ws), self.ws_bytes, self.stream))


def stock_silhouette(x, lab, K, rows, form, chunk=4096):
    """The stock-torch silhouette in float64: chunks of queried rows, torch.cdist against every row, the chunk's distances
    reduced per cluster by index_add_ ("index_add") or by a product with the one-hot labels ("onehot")."""
    n = x.shape[0]
    x64 = x.double()
    lab = lab.long()
    q = torch.arange(n, device=x.device) if rows is None else rows.long()
    ones = torch.ones(n, dtype=torch.float64, device=x.device)
    counts = torch.zeros(K, dtype=torch.float64, device=x.device).index_add_(0, lab, ones)
    onehot = torch.nn.functional.one_hot(lab, K).double() if form == "onehot" else None
    out = torch.empty(q.shape[0], dtype=torch.float64, device=x.device)
    for a in range(0, q.shape[0], chunk):
        qi = q[a:a + chunk]
        d = torch.cdist(x64[qi], x64)
        d[torch.arange(qi.shape[0], device=x.device), qi] = 0.0
        if form == "onehot":
            S = d @ onehot
        else:
            S = torch.zeros((qi.shape[0], K), dtype=torch.float64, device=x.device).index_add_(1, lab, d)
        own = lab[qi]
        cl = counts[own]
        a_ = S.gather(1, own[:, None])[:, 0] / (cl - 1).clamp_min(1)
        means = torch.where(counts[None, :] > 0, S / counts.clamp_min(1)[None, :], torch.full_like(S, float("inf")))
        means.scatter_(1, own[:, None], float("inf"))
        b_ = means.min(dim=1).values
        mx = torch.maximum(a_, b_)
        out[a:a + chunk] = torch.where((cl == 1) | (mx == 0), torch.zeros_like(mx), (b_ - a_) / mx)
    return out.mean()


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def load_lab():
    if not os.path.isfile(LAB_LIB):
        return None
    lib = ctypes.CDLL(LAB_LIB)
    res, args = _ffi.SIGNATURES["acx_silhouette"]
    lib.acx_silhouette.restype, lib.acx_silhouette.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_a_cluster_scores_bench.txt"))
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--sklearn", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_scores_bench needs a GPU: nothing is measured without one")
    say("cluster_scores_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    lab_lib = load_lab()
    for si in [int(v) for v in a.shapes.split(",")]:
        n, K, sample, what = SHAPES[si]
        say()
        say("== shape %d: n %d, K %d, dim %d (%s)" % (si, n, K, DIM, what))
        x, lab = make_data(n, K)
        rows = cs._sample_rows(n, sample, 0, x.device)
        m = n if rows is None else rows.shape[0]
        ours = Ours(x, lab, K, rows)
        ours.run()
        stock = {f: (lambda f=f: stock_silhouette(x, lab, K, rows, f)) for f in ("index_add", "onehot")}
        ref = {f: float(fn()) for f, fn in stock.items()}
        torch.cuda.synchronize()
        say("    mean silhouette: ours %.9f, stock index_add %.9f, stock onehot %.9f; status %d"
            % (float(ours.means[K]), ref["index_add"], ref["onehot"], int(ours.st)))
        reps = 200
        cont = {"ours": ours.run}
        for f, fn in stock.items():
            cont["torch cdist f64 + %s" % f] = fn
        med = medians(cont, reps)
        best = min((v, k) for k, v in med.items() if k != "ours")
        say("(a) silhouette of %d rows against %d, median of 5 alternating windows:" % (m, n))
        for k, v in med.items():
            say("      %-32s %10.3f ms" % (k, v))
        say("    ours against the best stock form (%s): %.2fx%s" % (best[1], best[0] / med["ours"], "  [>= 1.0x]" if si == 0 else ""))
        mo = peak_above(lambda: cs.silhouette(x, lab, clusters=K, sample=sample))
        ms = peak_above(stock[best[1].split("+ ")[1]])
        say("(b) peak device memory above the inputs: ours %.1f MiB (workspace %.1f MiB), stock %.1f MiB; the n x n float64 "
            "distances would be %.0f MiB" % (mo, ours.ws_bytes / 2 ** 20, ms, m * n * 8 / 2 ** 20))
        flop = 2.0 * m * n * DIM
        say("(d) the whole call: %.3f ms = %.1f %% of the 157.3 TFLOP/s f32-matrix peak (2 rows n dim flop)"
            % (med["ours"], flop / (med["ours"] * 1e-3) / F32_MATRIX_PEAK * 100))
        if lab_lib is not None:
            cut = Ours(x, lab, K, rows, lab_lib)
            cut.run()
            ab = medians({"full": ours.run, "one column per segment": cut.run}, reps)
            say("    LDS walk: full %.3f ms, ablation build (one column per segment) %.3f ms -> the walk is %.1f %% of the call"
                % (ab["full"], ab["one column per segment"], 100 * (1 - ab["one column per segment"] / ab["full"])))
        else:
            say("    LDS walk: build/lab/libacx_nowalk.so is not built (tools/lab/build_silhouette_lab.sh): not measured")
        # (e) dispersion and contingency
        dev = x.device
        cnt = torch.empty(K, dtype=torch.int64, device=dev)
        mean = torch.empty((K, DIM), dtype=torch.float64, device=dev)
        within = torch.empty((2, K), dtype=torch.float64, device=dev)
        grand = torch.empty(DIM, dtype=torch.float64, device=dev)
        table = torch.empty((K, K), dtype=torch.int64, device=dev)
        other = torch.roll(lab, 1)

        def disp():
            _ffi.cluster_dispersion(vp(x), x.stride(0), n, DIM, vp(lab), K, vp(cnt), vp(mean), vp(within[0]), vp(within[1]), vp(grand),
                                    vp(ours.st), (vp(ours.ws), ours.ws_bytes), ours.stream)

        def cont_():
            _ffi.contingency(vp(lab), K, vp(other), K, n, vp(table), vp(ours.st), ours.stream)
        disp()
        cont_()
        e = medians({"dispersion": disp, "contingency": cont_}, 20)
        say("(e) acx_cluster_dispersion %.3f ms, acx_contingency %.3f ms" % (e["dispersion"], e["contingency"]))
        # (c) scikit-learn from host arrays
        if a.sklearn and si < 2:
            try:
                from sklearn.metrics import silhouette_score
            except ImportError:
                say("(c) scikit-learn is not installed: not measured")
            else:
                xh, lh = x.cpu().numpy(), lab.cpu().numpy()
                t = time.perf_counter()
                sk = silhouette_score(xh, lh)
                tsk = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                val = float(cs.silhouette(xh, lh, clusters=K, device="cuda"))
                tours = (time.perf_counter() - t) * 1e3
                say("(c) from host arrays, copies included: sklearn silhouette_score %.1f ms, ours %.1f ms: %.1fx; |difference| %.2e"
                    % (tsk, tours, tsk / tours, abs(val - sk)))
        del ours, stock, x, lab
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
