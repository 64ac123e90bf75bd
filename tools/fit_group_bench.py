#!/usr/bin/env python
"""Group fits (pytorch/finetune.py fit_heads / cross_validate_head, acx_head_fit_group_step) against the same fits as sequential
fit_head calls of this tree, in one process on one device: the measurements behind profiles/r24_a_fit_group_bench.txt.

    python tools/fit_group_bench.py [--out profiles/r24_a_fit_group_bench.txt] [--sizes 0,1,2]

Per shape: 5 folds x C settings as one fit_heads call against a loop of fit_head over the same (subset, setting) pairs -- the
subsets gathered BEFORE the clock starts, which favours the loop -- in aggregate job-steps per second; the same at J = 1; the
device time of one group step per kernel (torch.profiler).  Every contender is warmed up; a timing is a window of at least a
second between device events; the contenders alternate; five repeats, median and range.  Then cross_validate_head on the small
shape (5 folds x 4 learning rates) against the loop a user would write: fit_head per (setting, fold), validated once after its
last epoch."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                          # noqa: E402
import torch.nn.functional as F       # noqa: E402

from audioset_convnext_inf_amd.pytorch import finetune as ft      # noqa: E402

# (n, N, batch, loss, settings, label)
SIZES = [(2000, 50, 64, "ce", 8, "ESC-50-sized"), (20371, 527, 512, "bce", 4, "AudioSet eval-sized"),
         (20000, 4096, 256, "ce", 2, "4 096 classes")]
FOLDS = 5
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_data(n, N, loss):
    g = torch.Generator(device="cuda").manual_seed(n + N)
    E = F.layer_norm(torch.randn(n, 768, generator=g, device="cuda"), (768,))
    if loss == "ce":
        return E, torch.randint(0, N, (n,), generator=g, device="cuda"), dict(loss="ce", classes=N)
    return E, (torch.rand(n, N, generator=g, device="cuda") < 0.05).float(), dict(loss="bce")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1000.0


def compare(contenders, job_steps_per_epoch):
    """{name: fn(epochs)} -> {name: job-steps/s, five windows of at least a second each}"""
    epochs_of = {}
    for name, fn in contenders.items():
        fn(1)
        epochs_of[name] = max(1, int(1.2 / timed(lambda: fn(1))) + 1)
    res = {name: [] for name in contenders}
    for _ in range(5):
        for name, fn in contenders.items():
            ep = epochs_of[name]
            res[name].append(ep * job_steps_per_epoch / timed(lambda: fn(ep)))
    for k, v in res.items():
        say("   %-22s %9.0f job-steps/s (median of 5; %.0f .. %.0f; windows of %d epochs)"
            % (k, statistics.median(v), min(v), max(v), epochs_of[k]))
    return {k: statistics.median(v) for k, v in res.items()}


def stage_times(fn, steps):
    """Device time per kernel name over fn(), divided by the group steps it ran."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total, e.count)
                for e in prof.key_averages() if "fit_" in e.key]
        for key, us, count in sorted(rows):
            say("      %-64s %8.2f us per group step (%d launches)" % (key[:64], us / steps, count))
        say("      all fit kernels: %.2f us per group step" % (sum(r[1] for r in rows) / steps))
    except Exception as ex:  # noqa: BLE001
        say("      device time per stage: not recorded (%s: %s)" % (type(ex).__name__, str(ex).splitlines()[0][:100]))


def bench_size(n, N, batch, loss, settings, label):
    E, T, shared = make_data(n, N, loss)
    ids = ft.kfold_ids(n, FOLDS, 0)
    train = [torch.nonzero(ids != f).reshape(-1) for f in range(FOLDS)]
    subsets = [(E[r.cuda()], T[r.cuda()]) for r in train]
    lrs = [1e-4 * 2 ** c for c in range(settings)]
    jobs = [dict(rows=train[f], lr=lr, seed=c) for c, lr in enumerate(lrs) for f in range(FOLDS)]
    J = len(jobs)
    spe = sum(len(ft.epoch_batches(r.numel(), batch, True)) for r in train) * settings
    say("n %d, N %d, batch %d, %s (%s): %d folds x %d settings = %d jobs, %d job-steps per epoch"
        % (n, N, batch, loss, label, FOLDS, settings, J, spe))
    kw = dict(batch_size=batch, drop_last=True, **shared)

    def group(epochs):
        ft.fit_heads(E, T, jobs, epochs=epochs, **kw)

    def loop(epochs):
        for c, lr in enumerate(lrs):
            for f in range(FOLDS):
                ft.fit_head(subsets[f][0], subsets[f][1], epochs=epochs, lr=lr, seed=c, **kw)

    med = compare({"fit_heads (one group)": group, "fit_head x %d" % J: loop}, spe)
    ratio = med["fit_heads (one group)"] / med["fit_head x %d" % J]
    say("   group / sequential: %.2f  [requirement >= 1.0: %s]" % (ratio, "met" if ratio >= 1.0 else "MISSED"))
    one = spe // J
    med1 = compare({"fit_heads, J = 1": lambda ep: ft.fit_heads(E, T, jobs[:1], epochs=ep, **kw),
                    "fit_head": lambda ep: ft.fit_head(subsets[0][0], subsets[0][1], epochs=ep, lr=lrs[0], seed=0, **kw)}, one)
    say("   J = 1: group / fit_head: %.2f  [expected near 1]" % (med1["fit_heads, J = 1"] / med1["fit_head"]))
    say("   device time, one epoch of the group (%d group steps):" % one)
    stage_times(lambda: group(1), one)
    say("   device time, one epoch of one fit_head (%d steps):" % one)
    stage_times(lambda: ft.fit_head(subsets[0][0], subsets[0][1], epochs=1, lr=lrs[0], seed=0, **kw), one)
    return ratio


def bench_cross_validation():
    n, N, batch = 2000, 50, 64
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, N, (n,), generator=g)
    E = F.layer_norm(torch.randn(N, 768, generator=g)[lab] * 0.3 + torch.randn(n, 768, generator=g), (768,)).cuda()
    lab = lab.cuda()
    grid = {"lr": [1e-4, 3e-4, 1e-3, 3e-3]}
    kw = dict(loss="ce", classes=N, epochs=20, batch_size=batch)
    say("cross_validate_head: n %d, N %d, batch %d, ce, 20 epochs, 5 folds x 4 learning rates, no refit" % (n, N, batch))

    def ours():
        return ft.cross_validate_head(E, lab, folds=FOLDS, grid=grid, refit=False, keep_fits=False, **kw)

    def loop():
        ids = ft.kfold_ids(n, FOLDS, 0, lab)
        out = []
        for lr in grid["lr"]:
            for f in range(FOLDS):
                tr, te = (ids != f).cuda(), (ids == f).cuda()
                fit = ft.fit_head(E[tr], lab[tr], lr=lr, **kw)
                out.append(ft._validate_ce(fit.weight, fit.bias, E[te], lab[te])["accuracy"])
        return out

    cv, by_hand = ours(), loop()
    same = cv.scores.reshape(-1).tolist() == by_hand
    res = {"cross_validate_head": [], "loop of fit_head": []}
    for _ in range(5):
        res["cross_validate_head"].append(timed(ours))
        res["loop of fit_head"].append(timed(loop))
    for k, v in res.items():
        say("   %-24s %8.1f ms wall (median of 5; %.1f .. %.1f)" % (k, 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)))
    say("   both validate once per fit, after its last epoch; the 20 scores are %s; best lr %g, accuracy %.3f +- %.3f"
        % ("equal" if same else "NOT EQUAL", cv.configs[cv.best]["lr"], cv.mean[cv.best], cv.std[cv.best]))
    say("   loop / cross_validate_head: %.1fx"
        % (statistics.median(res["loop of fit_head"]) / statistics.median(res["cross_validate_head"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_a_fit_group_bench.txt"))
    ap.add_argument("--sizes", default="0,1,2")
    a = ap.parse_args()
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for i in (int(s) for s in a.sizes.split(",")):
        bench_size(*SIZES[i])
    bench_cross_validation()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
