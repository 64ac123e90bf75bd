#!/usr/bin/env python
"""Calibration (pytorch/calibration.py, csrc/calibrate.hip) against stock torch on the same device: the measurements behind
profiles/r21_a_calibration_bench.txt.

    python tools/calibration_bench.py [--out profiles/r21_a_calibration_bench.txt] [--parent-lib path/to/parent/libacx.so]

Device times (events around `reps` calls after a warm-up, medians of five) at (20 371 x 527, 15 bins), (2 000 x 50) and
(100 000 x 50, single-label):
(a) reliability against torch ops on the device: bucketize by the same bin rule, then scatter_add of counts, positives and
    float64 confidences (the stock form has float atomics: its sums are not reproducible, which is noted beside the time);
(b) fit_platt against the best stock-torch form: a batched Newton over all classes in float64 -- the same sums as (C,) tensor
    reductions, the 2 x 2 solves batched, step halving by masks, run to the same stopping rule; the host reads one flag per
    iteration, as any torch loop must;
(c) fit_temperature against torch.optim.LBFGS (strong Wolfe, float64 parameter) on F.cross_entropy(beta * z, y, reduction="sum").
Both sides start from data resident on the device.  Then bench.py of this tree; with --parent-lib, bench.py again with ACX_LIB
pointing at the parent commit's library (expected ratio 1.00: no forward kernel changes).  Recorded, not asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                          # noqa: E402
import torch.nn.functional as F       # noqa: E402

from audioset_convnext_inf_amd.pytorch import calibration as cal            # noqa: E402

MULTI = [(20371, 527, "AudioSet eval-sized"), (2000, 50, "ESC-50-sized")]
SINGLE = [(100000, 50, "100 k clips, 50 classes"), (2000, 50, "ESC-50-sized")]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    """Median over five windows of the device time of one call, in ms."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def multilabel(n, C):
    g = torch.Generator(device="cuda").manual_seed(n + C)
    y = torch.rand(n, C, generator=g, device="cuda") < 0.3
    y[0], y[1] = True, False
    z = 0.8 * (2.0 * y.float() - 1.0) + 1.5 * torch.randn(n, C, generator=g, device="cuda")
    return z, y


def singlelabel(n, N, beta_star=2.0):
    g = torch.Generator(device="cuda").manual_seed(n + N)
    z = 2.0 * torch.randn(n, N, generator=g, device="cuda")
    y = torch.multinomial(torch.softmax(beta_star * z.double(), dim=1), 1, generator=g)[:, 0]
    return z, y


def torch_reliability(y, p, bins):
    n, C = p.shape
    b = torch.clamp((p * float(bins)).to(torch.int64), max=bins - 1) + torch.arange(C, device=p.device)[None, :] * bins
    flat = b.reshape(-1)
    count = torch.zeros(C * bins, dtype=torch.int64, device=p.device).scatter_add_(0, flat, torch.ones_like(flat))
    pos = torch.zeros(C * bins, dtype=torch.int64, device=p.device).scatter_add_(0, flat, y.reshape(-1).to(torch.int64))
    conf = torch.zeros(C * bins, dtype=torch.float64, device=p.device).scatter_add_(0, flat, p.reshape(-1).double())
    brier = ((p.double() - y.double()) ** 2).sum(dim=0)
    return count, pos, conf, brier


def torch_platt(y, z, smooth=True):
    """Batched float64 Newton over all classes with the stopping rule and the slack of fit_platt_host."""
    z = z.double()
    yb = y.bool()
    P, Nn = yb.sum(0).double(), (~yb).sum(0).double()
    t = torch.where(yb, ((P + 1) / (P + 2))[None, :], (1 / (Nn + 2))[None, :]) if smooth else yb.double()

    def sums(a, b):
        u = a[None, :] * z + b[None, :]
        e = torch.exp(-u.abs())
        l1 = torch.log1p(e)
        F_ = -(t * (torch.clamp(u, max=0) - l1) + (1 - t) * (torch.clamp(-u, max=0) - l1)).sum(0)
        inv = 1 / (1 + e)
        g = torch.where(u >= 0, inv, e * inv) - t
        h = e * inv * inv
        return F_, (g * z).sum(0), g.sum(0), (h * z * z).sum(0), (h * z).sum(0), h.sum(0)

    a, b = torch.zeros_like(P), torch.log((P + 1) / (Nn + 1))
    Fa, ga, gb, haa, hab, hbb = sums(a, b)
    live = torch.ones_like(P, dtype=torch.bool)
    for _ in range(100):
        haa2, hbb2 = haa + 1e-12, hbb + 1e-12
        det = haa2 * hbb2 - hab * hab
        da, db = -(hbb2 * ga - hab * gb) / det, -(haa2 * gb - hab * ga) / det
        live = live & (torch.maximum(da.abs(), db.abs()) > 1e-10 * torch.clamp(torch.maximum(a.abs(), b.abs()), min=1.0))
        if not bool(live.any()):                                   # the one host read per iteration
            break
        step = torch.where(live, 1.0, 0.0).double()
        for _ in range(50):
            Fn, *rest = sums(a + step * da, b + step * db)
            worse = live & ~(Fn <= Fa + cal.F_SLACK * torch.clamp(Fa.abs(), min=1.0))
            if not bool(worse.any()):
                break
            step = torch.where(worse, step * 0.5, step)
        a, b = a + step * da, b + step * db
        Fa, (ga, gb, haa, hab, hbb) = Fn, rest
    return a, b


def torch_temperature(y, z):
    beta = torch.ones(1, dtype=torch.float64, device=z.device, requires_grad=True)
    z64 = z.double()
    opt = torch.optim.LBFGS([beta], lr=1.0, max_iter=50, tolerance_grad=1e-10, tolerance_change=1e-14, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = F.cross_entropy(beta * z64, y, reduction="sum")
        loss.backward()
        return loss

    opt.step(closure)
    return beta.detach()


def bench_py(env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, env=env, timeout=1200)
    rows = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return json.loads(rows[-1]) if r.returncode == 0 and rows else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_a_calibration_bench.txt"))
    ap.add_argument("--parent-lib", help="libacx.so built from the parent commit: bench.py is run against it too (ACX_LIB)")
    ap.add_argument("--skip-bench", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this tool measures on an MI355X; no GPU is visible")
    say("calibration bench on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("\n(a) reliability, 15 bins: ours / torch scatter_add (device ms per call)")
    for n, C, name in MULTI:
        z, y = multilabel(n, C)
        p = torch.sigmoid(z)
        ours = timed(lambda: cal.reliability(y, p, bins=15), 20)
        ref = timed(lambda: torch_reliability(y, p, 15), 20)
        r = cal.reliability(y, p, bins=15)
        same = torch.equal(r.count.reshape(-1), torch_reliability(y, p, 15)[0])
        say("  %-24s (%6d x %3d): %8.3f ms / %8.3f ms = %.2fx   counts equal: %s (torch's float64 sums use atomics)"
            % (name, n, C, ours, ref, ref / ours, same))
    say("\n(b) fit_platt: ours (one launch) / batched float64 Newton in torch")
    for n, C, name in MULTI:
        z, y = multilabel(n, C)
        ours = timed(lambda: cal.fit_platt(y, z), 5)
        ref = timed(lambda: torch_platt(y, z), 2)
        fit = cal.fit_platt(y, z)
        ta, tb = torch_platt(y, z)
        d = max(float((fit.a - ta).abs().max()), float((fit.b - tb).abs().max()))
        say("  %-24s (%6d x %3d): %8.3f ms / %8.3f ms = %.2fx   max |(a, b) - torch| %.2e, iterations %d .. %d"
            % (name, n, C, ours, ref, ref / ours, d, int(fit.info.min()), int(fit.info.max())))
    say("\n(c) fit_temperature (32 evaluations queued): ours / torch.optim.LBFGS on F.cross_entropy")
    for n, N, name in SINGLE:
        z, y = singlelabel(n, N)
        ours = timed(lambda: cal.fit_temperature(y, z), 5)
        ref = timed(lambda: torch_temperature(y, z), 2)
        fit = cal.fit_temperature(y, z)
        say("  %-24s (%6d x %3d): %8.3f ms / %8.3f ms = %.2fx   beta %.9f against %.9f, %d evaluations"
            % (name, n, N, ours, ref, ref / ours, float(fit.beta), float(torch_temperature(y, z)), int(fit.info)))
        top = timed(lambda: cal.reliability_toplabel(y, z, calibration=fit), 20)
        say("  %-24s reliability_toplabel: %8.3f ms" % ("", top))
    if not a.skip_bench:
        say("\n(d) bench.py --gpus 1 --steps 20 --warmup 5")
        mine = bench_py()
        say("  this tree: %s" % (json.dumps(mine) if mine else "FAILED"))
        if a.parent_lib:
            parent = bench_py({"ACX_LIB": os.path.abspath(a.parent_lib)})
            say("  parent library: %s" % (json.dumps(parent) if parent else "FAILED"))
            if mine and parent and mine.get("value") and parent.get("value"):
                say("  ratio this / parent: %.3f (expected 1.00: no forward kernel changes)" % (mine["value"] / parent["value"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
