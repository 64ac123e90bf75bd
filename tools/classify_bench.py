#!/usr/bin/env python
"""Single-label heads (pytorch/classify.py, fit_head(loss="ce"), csrc/head_fit.hip, csrc/classify.hip) against stock torch on the
same device: the measurements behind profiles/r20_a_classify_bench.txt.

    python tools/classify_bench.py [--out profiles/r20_a_classify_bench.txt] [--sizes 0,1,2,3]
    python tools/classify_bench.py --only-ours 1 --steps 200      # a plain run of one size, for a kernel trace around it
    python tools/classify_bench.py --only-grad 1024,527           # 200 gradient passes of one shape, for a kernel trace

(a) cross-entropy steps/s: fit_head(loss="ce") against the best stock-torch form of the same loop (nn.Linear, F.cross_entropy,
    optim.Adam(amsgrad=True, fused=True), eager; and torch.cuda.graph replay of one captured step of the same, capturable=True),
    on round 13's four sizes.  Same data resident on the device, same init and epoch orders, drop_last; every shape warmed up; a timing is a window of
    at least a second between device events; the contenders alternate; medians of five.
(b) the row pass: its share of a step comes from a kernel trace around --only-grad (per-kernel durations of 200 steps of one
    shape); this tool prints the row kernel's traffic model, 16 bytes per logit (z read three times, G written once) against
    8 TB/s, to set beside the traced duration.
(c) softmax_topk against torch.softmax + torch.topk, classification_metrics against argmax + bincount, at (20 371, 527) and
    (100 000, 50); both sides leave their results on the device.  Then the widest case of softmax_topk, whose k rounds each
    re-read the row: (1 024, 32 768) at k = 64 beside k = 5, recorded without a target.
The kernel traces of (b), bench.py against the parent and the register figures are kept in profiles/r20_b_classify_traces.txt;
this tool rewrites only its own --out file."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                          # noqa: E402
import torch.nn.functional as F       # noqa: E402

from audioset_convnext_inf_amd.pytorch import classify as cl                # noqa: E402
from audioset_convnext_inf_amd.pytorch import finetune as ft                # noqa: E402

SIZES = [(2000, 50, 64, "ESC-50"), (20371, 527, 512, "AudioSet eval-sized"), (200000, 527, 1024, "200 k clips"),
         (20000, 4096, 256, "4 096 classes")]
HBM = 8.0e12
LR = 1e-3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, N):
    g = torch.Generator(device="cuda").manual_seed(n + N)
    E = F.layer_norm(torch.randn(n, 768, generator=g, device="cuda"), (768,))
    y = torch.randint(0, N, (n,), generator=g, device="cuda")
    return E, y


class TorchLoop:
    """The oracle's loop with fused Adam; mode: "fused" (eager) | "graph" (capturable=True, one captured step replayed)."""

    def __init__(self, E, y, N, batch, mode):
        self.E, self.y, self.batch = E, y, batch
        w0, b0 = ft.init_head(N, 0)
        self.W = w0.to("cuda").requires_grad_()
        self.b = b0.to("cuda").requires_grad_()
        kw = {"fused": True, "capturable": mode == "graph"}
        self.opt = torch.optim.Adam([self.W, self.b], lr=LR, betas=(0.9, 0.999), eps=1e-8, amsgrad=True, **kw)
        self.graph = None
        if mode == "graph":
            self.x = torch.zeros(batch, 768, device="cuda")
            self.t = torch.zeros(batch, dtype=torch.int64, device="cuda")
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
        loss = F.cross_entropy(F.linear(x, self.W, self.b), t)
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


def bench_fit(n, N, batch, label):
    E, y = make_data(n, N)
    spe = n // batch
    say("n %d, N %d, batch %d (%s): %d steps per epoch" % (n, N, batch, label, spe))
    loops = {}
    for mode in ("fused", "graph"):
        try:
            loops["torch " + mode] = TorchLoop(E, y, N, batch, mode)
        except Exception as ex:  # noqa: BLE001
            say("   torch %s: not available here (%s: %s)" % (mode, type(ex).__name__, str(ex).splitlines()[0][:120]))
    cont = {"fit_head ce": lambda ep: ft.fit_head(E, y, classes=N, loss="ce", epochs=ep, batch_size=batch, lr=LR, seed=0,
                                                  drop_last=True)}
    for name, loop in loops.items():
        cont[name] = (lambda ep, loop=loop: loop.run(ft.epoch_orders(n, ep, 0).cuda()))
    res, reps = windows(cont, unit=spe)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        say("   %-14s %9.0f steps/s (median of 5; %.0f .. %.0f; windows of %d steps)" % (k, med[k], min(v), max(v), reps[k] * spe))
    base = max((v, k) for k, v in med.items() if k != "fit_head ce")
    ratio = med["fit_head ce"] / base[0]
    say("   fit_head ce / best torch form (%s): %.2f  [expected >= 1.0: %s]" % (base[1], ratio, "met" if ratio >= 1.0 else "MISSED"))
    say("   row pass traffic model: %d x %d logits x 16 B = %.2f MB per step -> %.2f us at 8 TB/s"
        % (batch, N, batch * N * 16 / 1e6, batch * N * 16 / HBM * 1e6))


def bench_read(n, N, k=5):
    g = torch.Generator(device="cuda").manual_seed(n + N)
    z = torch.randn(n, N, generator=g, device="cuda") * 3
    y = torch.randint(0, N, (n,), generator=g, device="cuda")
    say("logits (%d, %d), k %d" % (n, N, k))

    def ours_topk(r):
        for _ in range(r):
            cl.softmax_topk(z, k=k)

    def ours_counts(r):
        for _ in range(r):
            cl.classification_metrics(y, z, k=k)

    def torch_topk(r):
        for _ in range(r):
            p = torch.softmax(z, dim=1)
            torch.topk(p, k, dim=1)

    def torch_counts(r):
        for _ in range(r):
            pred = z.argmax(dim=1)
            torch.bincount(y * N + pred, minlength=N * N)
            (pred == y).sum()
            (z.topk(k, dim=1).indices == y[:, None]).any(dim=1).sum()

    for title, cont in (("softmax + top-k", {"softmax_topk": ours_topk,
                                             "torch softmax + topk": torch_topk}),
                        ("accuracy, top-k accuracy, confusion", {"classification_metrics": ours_counts,
                                                                 "torch argmax + bincount + topk": torch_counts})):
        res, reps = windows(cont)
        med = {kk: statistics.median(v) for kk, v in res.items()}
        names = list(cont)
        for kk, v in res.items():
            say("   %-32s %9.1f us per call (median of 5 windows of %d calls; %.1f .. %.1f)"
                % (kk, 1e6 / med[kk], reps[kk], 1e6 / max(v), 1e6 / min(v)))
        say("   %s: ours / torch rate %.2f" % (title, med[names[0]] / med[names[1]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_a_classify_bench.txt"))
    ap.add_argument("--sizes", default="0,1,2,3")
    ap.add_argument("--only-ours", type=int, default=None, help="run fit_head(loss='ce') alone on this size (for a kernel trace)")
    ap.add_argument("--only-grad", default=None, help="rows,N: 200 calls of acx_head_fit_step_ce of that shape (for a kernel trace)")
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if a.only_ours is not None or a.only_grad is not None:
        if a.only_grad is not None:
            batch, N = (int(v) for v in a.only_grad.split(","))
            n = batch
        else:
            n, N, batch, _ = SIZES[a.only_ours]
        E, y = make_data(n, N)
        epochs = max(1, a.steps // (n // batch))
        ft.fit_head(E, y, classes=N, loss="ce", epochs=epochs, batch_size=batch, lr=LR, drop_last=True)
        torch.cuda.synchronize()
        print("ran %d steps of n %d N %d batch %d" % (epochs * (n // batch), n, N, batch))
        return
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("(a) cross-entropy steps/s against stock torch")
    for i in (int(s) for s in a.sizes.split(",")):
        bench_fit(*SIZES[i])
    say("(c) reading and judging a head against torch")
    bench_read(20371, 527)
    bench_read(100000, 50)
    say("(c') the widest head: k rounds over a 32 768-class row")
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn(1024, 32768, generator=g, device="cuda") * 3
    for k in (5, 64):
        def wide(r, k=k):
            for _ in range(r):
                cl.softmax_topk(z, k=k)

        res, reps = windows({"softmax_topk": wide})
        v = res["softmax_topk"]
        say("   softmax_topk (1024, 32768), k %2d  %9.1f us per call (median of 5 windows of %d calls)"
            % (k, 1e6 / statistics.median(v), reps["softmax_topk"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
