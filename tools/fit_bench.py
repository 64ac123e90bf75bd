#!/usr/bin/env python
"""Head fitting (pytorch/finetune.py, csrc/head_fit.hip) against stock torch on the same device: the measurements behind
profiles/r13_a_fit_bench.txt.

    python tools/fit_bench.py [--out profiles/r13_a_fit_bench.txt] [--sizes 0,1,2,3]
    python tools/fit_bench.py --only-ours 2 --steps 200        # a plain run of one size, for a kernel trace around it

Contenders, in one process, same data resident on the device, same init and epoch orders (drop_last, so every step has the
same shape): fit_head; the oracle's loop in torch (nn.Linear, sigmoid, F.binary_cross_entropy, optim.Adam(amsgrad=True)) with
foreach and with fused=True, eager; and torch.cuda.graph replay of one captured step (capturable=True), if it captures.  Every
shape is warmed up; a timing is a window of at least a second between device events; the contenders alternate; five repeats,
median and range.  Then the final weights of one epoch (at most 200 steps) of fit_head and of torch float32 against torch
float64 on the device, with the bound of tests/test_gpu_finetune.py (trajectories)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                          # noqa: E402
import torch.nn.functional as F       # noqa: E402

from audioset_convnext_inf_amd.pytorch import finetune as ft      # noqa: E402

SIZES = [(2000, 50, 64, "ESC-50"), (20371, 527, 512, "AudioSet eval-sized"), (200000, 527, 1024, "200 k clips"),
         (20000, 4096, 256, "4 096 classes")]
PEAK = 157.3e12
U = 2.0 ** -24
LR = 1e-3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, N):
    g = torch.Generator(device="cuda").manual_seed(n + N)
    E = F.layer_norm(torch.randn(n, 768, generator=g, device="cuda"), (768,))
    Y = (torch.rand(n, N, generator=g, device="cuda") < 0.05).float()
    return E, Y


class TorchLoop:
    """The oracle's loop; mode: "foreach" | "fused" | "graph"."""

    def __init__(self, E, Y, batch, mode, dtype=torch.float32):
        self.E, self.Y, self.batch, self.mode = E.to(dtype), Y.to(dtype), batch, mode
        N = Y.shape[1]
        w0, b0 = ft.init_head(N, 0)
        self.W = w0.to("cuda", dtype).requires_grad_()
        self.b = b0.to("cuda", dtype).requires_grad_()
        kw = {"fused": True} if mode == "fused" else {"foreach": True, "capturable": mode == "graph"}
        self.opt = torch.optim.Adam([self.W, self.b], lr=LR, betas=(0.9, 0.999), eps=1e-8, amsgrad=True, **kw)
        self.graph = None
        if mode == "graph":
            self.x, self.y = torch.zeros(batch, 768, device="cuda", dtype=dtype), torch.zeros(batch, N, device="cuda", dtype=dtype)
            side = torch.cuda.Stream()                  # the warm-up moves the state: this contender is timed, not compared
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    self._step(self.x, self.y)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._step(self.x, self.y)

    def _step(self, x, y):
        loss = F.binary_cross_entropy(torch.sigmoid(F.linear(x, self.W, self.b)), y)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()

    def run(self, orders):
        """orders: (epochs, n) device int64; drop_last."""
        n, bs = orders.shape[1], self.batch
        for e in range(orders.shape[0]):
            perm = orders[e]
            for s in range(0, n - bs + 1, bs):
                i = perm[s:s + bs]
                if self.graph is not None:
                    torch.index_select(self.E, 0, i, out=self.x)
                    torch.index_select(self.Y, 0, i, out=self.y)
                    self.graph.replay()
                else:
                    self._step(self.E[i], self.Y[i])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1000.0


def bench_size(n, N, batch, label):
    E, Y = make_data(n, N)
    spe = n // batch
    say("n %d, N %d, batch %d (%s): %d steps per epoch" % (n, N, batch, label, spe))
    cont = {"fit_head": None}
    for mode in ("foreach", "fused", "graph"):
        try:
            cont["torch " + mode] = TorchLoop(E, Y, batch, mode)
        except Exception as ex:  # noqa: BLE001
            say("   torch %s: not available here (%s: %s)" % (mode, type(ex).__name__, str(ex).splitlines()[0][:120]))
    torch.cuda.synchronize()

    def runner(name, epochs):
        if name == "fit_head":
            return lambda: ft.fit_head(E, Y, epochs=epochs, batch_size=batch, lr=LR, seed=0, drop_last=True)
        orders = ft.epoch_orders(n, epochs, 0).cuda()
        return lambda: cont[name].run(orders)

    epochs_of = {}
    for name in cont:                                  # warm-up and calibration: a window of at least a second
        runner(name, 1)()
        t = timed(runner(name, 1))
        epochs_of[name] = max(1, int(1.2 / t) + 1)
    res = {name: [] for name in cont}
    for _ in range(5):
        for name in cont:
            ep = epochs_of[name]
            res[name].append(ep * spe / timed(runner(name, ep)))
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        say("   %-14s %9.0f steps/s (median of 5; %.0f .. %.0f; windows of %d steps)" % (k, med[k], min(v), max(v), epochs_of[k] * spe))
    base = max((v, k) for k, v in med.items() if k != "fit_head")
    ratio = med["fit_head"] / base[0]
    say("   fit_head / best torch form (%s): %.2f  [target >= 1.0: %s]" % (base[1], ratio, "met" if ratio >= 1.0 else "MISSED"))
    flop = 2 * 2 * batch * 768 * N
    say("   (2 x 2 x rows x 768 x N = %.3g FLOP per step: %.2f %% of the f32 matrix peak at this rate, launch gaps included)"
        % (flop, 100 * flop * med["fit_head"] / PEAK))
    # agreement: one epoch (at most 200 steps)
    steps = min(spe, 200)
    m = steps * batch
    Es, Ys = E[:m], Y[:m]
    orders = ft.epoch_orders(m, 1, 0).cuda()
    ours = ft.fit_head(Es, Ys, epochs=1, batch_size=batch, lr=LR, seed=0, drop_last=True)
    t32, t64 = TorchLoop(Es, Ys, batch, "foreach"), TorchLoop(Es, Ys, batch, "foreach", torch.float64)
    t32.run(orders)
    t64.run(orders)
    torch.cuda.synchronize()
    w64 = t64.W.detach()
    floor = float((t32.W.detach().double() - w64).abs().max())
    bound = max(8 * floor, steps * U * float(w64.abs().max()))
    err = float((ours.weight.double() - w64).abs().max())
    say("   after %d steps: max|W fit_head - W torch f64| %.3g, torch f32's own %.3g, bound %.3g  [%s]"
        % (steps, err, floor, bound, "met" if err <= bound else "MISSED"))
    return ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_a_fit_bench.txt"))
    ap.add_argument("--sizes", default="0,1,2,3")
    ap.add_argument("--only-ours", type=int, default=None, help="run fit_head alone on this size (for a kernel trace)")
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if a.only_ours is not None:
        n, N, batch, _ = SIZES[a.only_ours]
        E, Y = make_data(n, N)
        epochs = max(1, a.steps // (n // batch))
        ft.fit_head(E, Y, epochs=epochs, batch_size=batch, lr=LR, drop_last=True)
        torch.cuda.synchronize()
        print("ran %d steps of n %d N %d batch %d" % (epochs * (n // batch), n, N, batch))
        return
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for i in (int(s) for s in a.sizes.split(",")):
        bench_size(*SIZES[i])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
