#!/usr/bin/env python
"""Scoring events on the device ("Scoring events on the device"): the measurements behind
profiles/r19_a_sed_score_bench.txt.  Measured, not asserted; expectations in brackets, misses stated as misses.

    python tools/sed_score_bench.py [--base-tree DIR] [--out profiles/r19_a_sed_score_bench.txt]

The process started this way never opens the GPU.  Every measurement is a child process of its own under `timeout -k 10 N`
(the sections below; `rocprofv3 ... -- python tools/sed_score_bench.py --section trace-workload` for (a); `bench.py` for (d)),
run one after the other; the first child that does not exit with 0 -- a failure, a fault, an abort, a time limit -- ends the run
with exit code 1 and nothing more is started.  Every line goes to --out as soon as it exists.

0. Registers and scratch of the two kernels, from the code objects inside the built library [no scratch, as the decoder].
(a) Device time of acx_score_events and acx_score_segments on the events of detect_events(median=3, low=0.3) at bs 64 x 10 s,
    527 classes, against the device time of acx_decode_events (its three launches) on the same batch, from ONE
    `rocprofv3 --kernel-trace --stats` run [each scorer at or below the decoder: it reads tables that are a small fraction of
    the probabilities the decoder reads; the ratio is recorded either way].
(b) Both scorers against the host definitions on the same lists (wall clock, synchronised, best of 3), with and without the
    host needing the lists first.
(c) A 20-point sweep_event_thresholds on one hour of forward_windows(what="segment") timeline.
(d) (--base-tree: a checkout of the parent commit with its libacx.so built) bench.py headline of both trees, alternating
    [expected 1.00: nothing on its path changes; margin: the box-to-box spread of the README]."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np                      # noqa: E402
import torch                            # noqa: E402

from audioset_convnext_inf_amd import synth      # noqa: E402
from audioset_convnext_inf_amd.pytorch import sed_metrics as sm      # noqa: E402
from audioset_convnext_inf_amd.pytorch import segments as seg      # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny      # noqa: E402

SR = 32000
OUT = None          # the parent's output file, appended to line by line
DECODE = dict(median=3, low=0.3)
TRACE_CALLS = 13


def say(s=""):
    print(s, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(s + "\n")


def make_model():
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth.synth_state_dict(0))
    return m.to("cuda").eval().set_precision("fp32_split")


def annotations(estimated, ends, classes, step, seed=0):
    """Annotations for decoded events: onsets and offsets moved by up to two half steps, one event in seven dropped, one in seven
    doubled by an overlapping one, spurious ones added."""
    rng = np.random.default_rng(seed)
    half = step / 2
    out = []
    for events, end in zip(estimated, ends):
        ref = []
        for ev in events:
            u = rng.random()
            k_on, k_off = rng.integers(-2, 3, size=2)
            if u < 0.15:
                continue
            on, off = max(ev[1] + k_on * half, 0.0), ev[2] + k_off * half
            if not on < off:
                on, off = ev[1], ev[2]
            ref.append((ev[0], on, off))
            if u > 0.85:
                ref.append((ev[0], on + half, off + 3 * half))
        for _ in range(1 + len(events) // 6):
            on = half * int(rng.integers(0, max(int(end / half), 1)))
            ref.append((int(rng.integers(0, classes)), on, on + half * int(rng.integers(1, 5))))
        out.append(ref)
    return out


def batch_case():
    """(probabilities, table, reference, lists) of detect_events at bs 64 x 10 s, 527 classes, thresholds at the probabilities'
    upper quartile so that a synthetic checkpoint gives a realistic table"""
    m = make_model()
    x = synth.synth_waveforms(64, 10 * SR, seed=1).cuda()
    with torch.no_grad():
        out = m.forward_segments(x)
    probs = out["segmentwise_output"]
    thr = float(torch.quantile(probs.flatten()[:1 << 20], 0.75))
    args = dict(DECODE, threshold=thr, low=0.9 * thr, step=out["segment_edges"].numpy(), capacity=probs.numel() // 2 + 1)
    table = seg.decode_events_gpu(probs, **args)
    est = table.to_lists()
    ends = [float(e[-1]) for e in table.edges]
    ref = annotations(est, ends, probs.shape[2], seg.SEGMENT_SECONDS)
    return probs, args, table, sm.ReferenceEvents.from_lists(ref, probs.shape[2], device="cuda"), ref, est, ends


def section_trace_workload():
    """The workload of the rocprofv3 run: TRACE_CALLS x (decode, score events, score segments) on one batch."""
    probs, args, table, reference, ref, est, ends = batch_case()
    for _ in range(TRACE_CALLS):
        t = seg.decode_events_gpu(probs, **args)
        sm.event_based_metrics(reference, t)
        sm.segment_based_metrics(reference, t)
    torch.cuda.synchronize()


def best_of(fn, n=3):
    best = float("inf")
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def section_host():
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    probs, args, table, reference, ref, est, ends = batch_case()
    N = probs.shape[2]
    say("(b) against the host definitions on this machine's host (%d CPUs visible), bs 64 x 10 s, %d classes, %d events in the "
        "table, %d annotated, best of 3, synchronised:" % (os.cpu_count() or 0, N, len(table), len(reference)))
    for name, dev, host in (("event-based", lambda: sm.event_based_metrics(reference, table).check(),
                             lambda: sm.event_based_metrics_host(ref, est, N)),
                            ("segment-based (1 s)", lambda: sm.segment_based_metrics(reference, table).check(),
                             lambda: sm.segment_based_metrics_host(ref, est, ends, N))):
        dev()
        t_dev, t_host = best_of(dev), best_of(host, 2)
        t_lists = best_of(lambda: table.to_lists(), 2)
        same = np.array_equal(dev().counts_host(), host().counts)
        say("   %-20s device %.6f s (counts read back), host %.4f s: %.0f x; the host also needs to_lists() first, %.4f s: %.0f x;"
            " counts equal: %s" % (name, t_dev, t_host, t_host / t_dev, t_lists, (t_host + t_lists) / t_dev, same))


def section_sweep():
    m = make_model()
    hour = synth.synth_waveforms(1, 3600 * SR, seed=3)[0].cuda()
    with torch.no_grad():
        timeline = m.forward_windows(hour, window=10.0, hop=10.0, what="segment")["timeline"]
    thr0 = float(torch.quantile(timeline.flatten()[:1 << 20], 0.75))
    est = seg.decode_events_gpu(timeline, threshold=thr0, median=3).to_lists()
    ends = [timeline.shape[0] * seg.SEGMENT_SECONDS]
    ref = annotations(est, ends, timeline.shape[1], seg.SEGMENT_SECONDS)
    reference = sm.ReferenceEvents.from_lists(ref, timeline.shape[1], device="cuda")
    grid = np.linspace(0.5 * thr0, min(1.5 * thr0, 0.999), 20)
    say("(c) sweep_event_thresholds, 20 thresholds, one hour of forward_windows(what=\"segment\") timeline (%d rows x %d classes, "
        "%d annotated events), best of 3, synchronised:" % (timeline.shape[0], timeline.shape[1], len(reference)))
    for metric, kw in (("event", {}), ("segment", dict(time_resolution=1.0)), ("segment", dict(time_resolution=0.1))):
        run = lambda: sm.sweep_event_thresholds(timeline, reference, grid, metric=metric, capacity=1 << 20, median=3, **kw)   # noqa: E731
        run()
        t = best_of(run)
        thr, counts = run()
        say("   metric=%-8s %-22s %.4f s for 20 decodings and scorings (%.2f ms per point); %d classes got a finite threshold"
            % (metric, kw or "", t, 1e3 * t / 20, int(torch.isfinite(thr).sum())))


SECTIONS = {"trace-workload": section_trace_workload, "host": section_host, "sweep": section_sweep}


def run_child(cmd, limit, cwd=None, env=None):
    """One GPU step: `cmd` under its own time limit.  Returns its stdout; anything but exit code 0 ends the whole run."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd,
                       env=env)
    if r.returncode != 0:
        say("FAILED (exit %d), nothing more is started: %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-800:]))
        sys.exit(1)
    return r.stdout


def run_section(name, limit):
    for line in run_child([sys.executable, os.path.abspath(__file__), "--section", name], limit).splitlines():
        say(line)


def resources():
    import check_exclusive
    lib = os.path.join(ROOT, "audioset-convnext-inf_amd", "libacx.so")
    say("0. registers and scratch, from the code objects inside %s:" % os.path.relpath(lib, ROOT))
    for name, threads, vgpr, scratch in sorted(check_exclusive.kernels_of(lib)):
        if "sed_event_match_kernel" in name or "sed_segment_kernel" in name or "events_kernel" in name:
            say("   %-70s up to %4d threads, %3d vector registers, %d bytes of scratch  [no scratch: %s]"
                % (name[:70], threads, vgpr, scratch, "met" if scratch == 0 else "MISSED"))


def kernel_stats():
    with tempfile.TemporaryDirectory() as d:
        run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--section", "trace-workload"], 300, cwd=d)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            say("(a) FAILED: the rocprofv3 run left no kernel statistics")
            sys.exit(1)
        rows = list(csv.DictReader(open(files[0])))

    def per_call(key, exact_calls=None):
        mine = [r for r in rows if key in r["Name"]]
        ns = sum(float(r["TotalDurationNs"]) for r in mine)
        calls = sum(int(r["Calls"]) for r in mine)
        return ns / TRACE_CALLS / 1e3, calls / TRACE_CALLS

    say("(a) device time per call, rocprofv3 --kernel-trace --stats, bs 64 x 10 s, 527 classes, same run (the first decoding of "
        "the batch is in the decoder's average too):")
    dec = per_call("events_kernel")[0] + per_call("events_scan_kernel")[0]
    n_dec = per_call("events_kernel")[1] + per_call("events_scan_kernel")[1]
    say("   acx_decode_events     %8.1f us (%.1f launches per call)" % (dec * TRACE_CALLS / (TRACE_CALLS + 1), n_dec))
    dec = dec * TRACE_CALLS / (TRACE_CALLS + 1)
    for key, name in (("sed_event_match_kernel", "acx_score_events"), ("sed_segment_kernel", "acx_score_segments")):
        us, n = per_call(key)
        say("   %-20s  %8.1f us (%.1f launches per call): %.2f of the decoder  [at or below the decoder: %s]"
            % (name, us, n, us / dec, "met" if us <= dec else "MISSED"))


def tree_bench(tree, args):
    env = dict(os.environ)
    env.pop("ACX_LIB", None)
    out = run_child([sys.executable, os.path.join(tree, "bench.py")] + args, 300, cwd=tree, env=env)
    return json.loads(out.strip().splitlines()[-1])


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run one measurement in this process and print its lines")
    ap.add_argument("--base-tree", default=None, help="checkout of the parent commit, its library built (bench.py A/B)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_a_sed_score_bench.txt"))
    a = ap.parse_args()
    if a.section:
        return SECTIONS[a.section]()
    OUT = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    resources()
    if not a.skip_trace:
        kernel_stats()
    if not a.skip_host:
        run_section("host", 420)
    if not a.skip_sweep:
        run_section("sweep", 420)
    if a.base_tree:
        runs = {"base": [], "new": []}
        for _ in range(3):
            for which, tree in (("base", a.base_tree), ("new", ROOT)):
                runs[which].append(tree_bench(os.path.abspath(tree), ["--gpus", "1", "--steps", "50", "--warmup", "10"])["value"])
        r = max(runs["new"]) / max(runs["base"])
        say("(d) bench.py headline (fp32_split, bs 64), three alternating runs each: parent %s, this %s clips/s: best %.3f of the "
            "parent  [expected 1.00]" % (" ".join("%.0f" % v for v in runs["base"]), " ".join("%.0f" % v for v in runs["new"]), r))


if __name__ == "__main__":
    main()
