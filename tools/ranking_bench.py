#!/usr/bin/env python
"""Ranking metrics per clip on the GPU (pytorch/ranking.py, csrc/ranking.hip) against a stock-torch formulation on the same device
and scikit-learn on the host: the measurements behind profiles/r30_a_ranking_bench.txt.

    python tools/ranking_bench.py [--out profiles/r30_a_ranking_bench.txt] [--shapes 20371x527x2,100000x80x1.2,4096x4096x5]

Per shape rows x classes x mean positives per row, on resident fp32 scores without ties and uint8 targets:
(a) device time of acx_ranking_metrics (every launch of the call, workspace preallocated) against the stock-torch form
    argsort(descending) + gather + cumsum, which yields the same per-row psum, coverage and bad pairs where no scores tie (it has
    no tie rule and no per-class sums); the contenders alternate, medians of five windows between device events.
    [>= 1.0x stock torch at the first shape]
(b) the share of 8 TB/s that the bytes the call MUST move (scores and targets once) make of its time, and the same with the
    quotient workspace it writes and reads back counted (8 bytes per cell each way) -- at the first shape.
(c) from host numpy arrays, copies included: ranking_metrics(...) to its synchronised scalars against sklearn's
    label_ranking_average_precision_score + coverage_error + label_ranking_loss.
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
from audioset_convnext_inf_amd.pytorch import ranking                        # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


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
    """acx_ranking_metrics on resident inputs with every buffer allocated once."""

    def __init__(self, y, s, k=1):
        self.y, self.s, self.k = y, s, k
        rows, C = s.shape
        dev = s.device
        self.counts = torch.empty((rows, 4), dtype=torch.int64, device=dev)
        self.psum = torch.empty(rows, dtype=torch.float64, device=dev)
        self.ccount = torch.empty(C, dtype=torch.int64, device=dev)
        self.cpsum = torch.empty(C, dtype=torch.float64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws_bytes = _ffi.ranking_workspace_bytes(rows, C, 0)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.stream = _ffi.stream_ptr(dev)

    def __call__(self):
        y, s = self.y, self.s
        _ffi.ranking_metrics(vp(s), s.stride(0), vp(y), _ffi.TARGET_U8, y.stride(0), s.shape[0], s.shape[1], self.k, 0, vp(self.counts),
                             vp(self.psum), vp(self.ccount), vp(self.cpsum), vp(self.status), (vp(self.ws), self.ws_bytes), self.stream)


def stock(y, s):
    """The sort-based form in stock torch ops -> (psum, coverage, bad_pairs, n_pos) per row; right where no scores tie."""
    order = torch.argsort(s, dim=1, descending=True)
    ys = torch.gather(y, 1, order).to(torch.float64)
    cum = torch.cumsum(ys, dim=1)
    rank = torch.arange(1, s.shape[1] + 1, device=s.device, dtype=torch.float64)
    return (ys * cum / rank).sum(dim=1), (ys * rank).amax(dim=1), (ys * (rank - cum)).sum(dim=1), cum[:, -1]


def bench(rows, C, mean_pos, first):
    say()
    say("== %d rows x %d classes, about %g positives per row" % (rows, C, mean_pos))
    g = torch.Generator(device="cuda").manual_seed(rows + C)
    s = torch.rand((rows, C), generator=g, device="cuda")
    y = (torch.rand((rows, C), generator=g, device="cuda") < mean_pos / C).to(torch.uint8)
    s = s + 0.3 * y                                                   # some signal: the positives rank higher than chance
    ours = Ours(y, s)
    ours()
    ref = stock(y, s)
    torch.cuda.synchronize()
    tied = int((torch.sort(s, dim=1).values.diff(dim=1) == 0).sum())
    say("    positives per row %.2f; adjacent equal scores in a row: %d; max |psum - stock| %.1e, coverage differs in %d rows, "
        "bad pairs in %d rows" % (float(ours.counts[:, 0].double().mean()), tied, float((ours.psum - ref[0]).abs().max()),
                                  int((ours.counts[:, 1] != ref[1]).sum()), int((ours.counts[:, 2] != ref[2]).sum())))
    t0 = window(ours, 2)
    reps = int(min(200, max(2, 100.0 / max(t0, 0.05))))
    med = medians({"ours": ours, "stock": lambda: stock(y, s)}, reps)
    say("    median of 5 windows of %d calls: acx_ranking_metrics %.3f ms, argsort + gather + cumsum %.3f ms: %.2fx%s"
        % (reps, med["ours"], med["stock"], med["stock"] / med["ours"], "  [>= 1.0x]" if first else ""))
    must, ws = rows * C * 5.0, rows * C * 16.0
    sec = med["ours"] * 1e-3
    say("    bytes that must move (fp32 scores + uint8 targets once): %.1f MB = %.1f %% of 8 TB/s over the call; with the quotient "
        "workspace written and read back: %.1f MB = %.1f %%" % (must / 1e6, 100 * must / sec / 8e12, (must + ws) / 1e6,
                                                                 100 * (must + ws) / sec / 8e12))
    from sklearn.metrics import coverage_error, label_ranking_average_precision_score, label_ranking_loss
    yh, sh = y.cpu().numpy(), s.cpu().numpy()
    t = time.perf_counter()
    want = (label_ranking_average_precision_score(yh, sh), coverage_error(yh, sh), label_ranking_loss(yh, sh))
    tsk = (time.perf_counter() - t) * 1e3
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        r = ranking.ranking_metrics(yh, sh, device="cuda")
        got = (r.lrap, r.coverage_error, r.ranking_loss)
        ts.append((time.perf_counter() - t) * 1e3)
    say("    from host arrays, copies included: sklearn's three functions %.1f ms, ranking_metrics to its scalars %.1f ms: %.0fx; "
        "max difference of the three values %.1e" % (tsk, statistics.median(ts), tsk / statistics.median(ts),
                                                     max(abs(a - b) for a, b in zip(got, want))))
    del s, y, ours, ref
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_a_ranking_bench.txt"))
    ap.add_argument("--shapes", default="20371x527x2,100000x80x1.2,4096x4096x5")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ranking_bench needs a GPU: nothing is measured without one")
    say("ranking_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for i, shape in enumerate(v for v in a.shapes.split(",") if v):
        rows, C, pos = shape.split("x")
        bench(int(rows), int(C), float(pos), i == 0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
