#!/usr/bin/env python
"""Weak-label SED fits (pytorch/finetune.py fit_sed_head, csrc/head_fit.hip fit_mil_bag_kernel) against stock torch on the same
device: the measurements behind profiles/r27_a_sed_fit_bench.txt.

    python tools/sed_fit_bench.py [--out profiles/r27_a_sed_fit_bench.txt] [--sizes 0,1] [--poolings max,linear]
    python tools/sed_fit_bench.py --only-ours 1 --pooling linear --steps 200      # a plain run, for a kernel trace around it

(a) steps/s of fit_sed_head against the best stock-torch form of the same loop: autograd through F.linear -> sigmoid -> pooling
    over the 31 segments -> F.binary_cross_entropy with optim.Adam(amsgrad=True, fused=True), eager, and torch.cuda.graph replay
    of one captured step of the same (capturable=True).  Shapes: (2 000 clips x 31 segments, N 50, batch 64) and (20 371 x 31,
    N 527, batch 64).  Same data resident on the device, same init and epoch orders, drop_last; every shape warmed up; a timing
    is a window of at least a second between device events; the contenders alternate; medians of five.  fit_sed_head's time
    includes building and uploading its index arrays for the window's epochs.
(b) the bag pass: its device time and share of a step come from a kernel trace around --only-ours (per-kernel durations); this
    tool prints the kernel's algorithmic traffic -- z read twice ("max": once), G written once, P and the targets once -- against
    8 TB/s, to set beside the traced duration (recorded with no target: the pass is latency-bound).
bench.py against the parent is run beside this tool and noted in the same profile by hand."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                          # noqa: E402
import torch.nn.functional as F       # noqa: E402

from audioset_convnext_inf_amd.pytorch import finetune as ft                # noqa: E402

SIZES = [(2000, 31, 50, 64, "ESC-50-sized weak set"), (20371, 31, 527, 64, "AudioSet eval-sized")]
HBM = 8.0e12
LR = 1e-3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, S, N):
    g = torch.Generator(device="cuda").manual_seed(n + N)
    E = F.layer_norm(torch.randn(n, S, 768, generator=g, device="cuda"), (768,))
    y = (torch.rand(n, N, generator=g, device="cuda") < 0.05).float()
    return E, y


def pooled(q, pooling):
    if pooling == "max":
        return q.max(dim=1).values
    if pooling == "mean":
        return q.mean(dim=1)
    if pooling == "linear":
        return (q * q).sum(dim=1) / q.sum(dim=1)
    e = torch.exp(q)
    return (q * e).sum(dim=1) / e.sum(dim=1)


class TorchLoop:
    """The reference's loop with fused Adam; mode: "fused" (eager) | "graph" (capturable=True, one captured step replayed)."""

    def __init__(self, E, y, N, batch, pooling, mode):
        self.E, self.y, self.batch, self.pooling = E, y, batch, pooling
        w0, b0 = ft.init_head(N, 0)
        self.W = w0.to("cuda").requires_grad_()
        self.b = b0.to("cuda").requires_grad_()
        self.opt = torch.optim.Adam([self.W, self.b], lr=LR, betas=(0.9, 0.999), eps=1e-8, amsgrad=True, fused=True,
                                    capturable=mode == "graph")
        self.graph = None
        if mode == "graph":
            self.x = torch.zeros((batch,) + tuple(E.shape[1:]), device="cuda")
            self.t = torch.zeros(batch, N, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    self._step(self.x, self.t)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._step(self.x, self.t)

    def _step(self, x, t):
        loss = F.binary_cross_entropy(pooled(torch.sigmoid(F.linear(x, self.W, self.b)), self.pooling), t)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()

    def run(self, orders):
        n, bs = orders.shape[1], self.batch
        for e in range(orders.shape[0]):
            perm = orders[e]
            for s in range(0, n - bs + 1, bs):
                i = perm[s:s + bs]
                if self.graph is not None:
                    torch.index_select(self.E, 0, i, out=self.x)
                    torch.index_select(self.y, 0, i, out=self.t)
                    self.graph.replay()
                else:
                    self._step(self.E[i], self.y[i])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1000.0


def windows(cont, unit=1):
    """Median-of-five rates of the contenders {name: fn(reps)}, alternating; a window is at least a second."""
    reps = {}
    for name, fn in cont.items():
        fn(1)
        t = timed(lambda: fn(1))
        reps[name] = max(1, int(1.2 / t) + 1)
    res = {name: [] for name in cont}
    for _ in range(5):
        for name, fn in cont.items():
            r = reps[name]
            res[name].append(r * unit / timed(lambda: fn(r)))
    return res, reps


def bench_fit(n, S, N, batch, label, pooling):
    E, y = make_data(n, S, N)
    spe = n // batch
    say("%d clips x %d segments, N %d, batch %d (%s), pooling %s: %d steps per epoch" % (n, S, N, batch, label, pooling, spe))
    loops = {}
    for mode in ("fused", "graph"):
        try:
            loops["torch " + mode] = TorchLoop(E, y, N, batch, pooling, mode)
        except Exception as ex:  # noqa: BLE001
            say("   torch %s: not available here (%s: %s)" % (mode, type(ex).__name__, str(ex).splitlines()[0][:120]))
    cont = {"fit_sed_head": lambda ep: ft.fit_sed_head(E, y, pooling, epochs=ep, batch_size=batch, lr=LR, seed=0, drop_last=True)}
    for name, loop in loops.items():
        cont[name] = (lambda ep, loop=loop: loop.run(ft.epoch_orders(n, ep, 0).cuda()))
    res, reps = windows(cont, unit=spe)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        say("   %-14s %9.0f steps/s (median of 5; %.0f .. %.0f; windows of %d steps)" % (k, med[k], min(v), max(v), reps[k] * spe))
    base = max((v, k) for k, v in med.items() if k != "fit_sed_head")
    ratio = med["fit_sed_head"] / base[0]
    say("   fit_sed_head / best torch form (%s): %.2f  [bar >= 1.0: %s]" % (base[1], ratio, "met" if ratio >= 1.0 else "MISSED"))
    rows = batch * S
    traffic = rows * N * 4 * ((1 if pooling == "max" else 2) + 1) + batch * N * 8
    say("   bag pass traffic model: %d x %d logits, %.2f MB per step -> %.2f us at 8 TB/s (no target: latency-bound)"
        % (rows, N, traffic / 1e6, traffic / HBM * 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_a_sed_fit_bench.txt"))
    ap.add_argument("--sizes", default="0,1")
    ap.add_argument("--poolings", default="max,linear")
    ap.add_argument("--only-ours", type=int, default=None, help="run fit_sed_head alone on this size (for a kernel trace)")
    ap.add_argument("--pooling", default="max")
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if a.only_ours is not None:
        n, S, N, batch, _ = SIZES[a.only_ours]
        n = min(n, batch * a.steps)
        E, y = make_data(n, S, N)
        epochs = max(1, a.steps // (n // batch))
        ft.fit_sed_head(E, y, a.pooling, epochs=epochs, batch_size=batch, lr=LR, drop_last=True)
        torch.cuda.synchronize()
        print("ran %d steps of %d clips x %d, N %d, batch %d, pooling %s" % (epochs * (n // batch), n, S, N, batch, a.pooling))
        return
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("(a) weak-label SED steps/s against stock torch")
    for i in (int(s) for s in a.sizes.split(",")):
        for pooling in a.poolings.split(","):
            bench_fit(*SIZES[i], pooling)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
