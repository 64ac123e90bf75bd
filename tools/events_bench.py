#!/usr/bin/env python
"""Event decoding on the device ("Decoding events on the device"): the measurements behind
profiles/r15_a_events_bench.txt.  Measured, not asserted; targets in brackets, misses stated as misses.

    python tools/events_bench.py [--base-tree DIR] [--out profiles/r15_a_events_bench.txt]

The process started this way never opens the GPU.  Every measurement is a child process of its own under `timeout -k 10 N`
(the sections below; `rocprofv3 ... -- python tools/events_bench.py --section trace-workload` for 2; `bench.py` for 4), run one
after the other; the first child that does not exit with 0 -- a failure, a fault, an abort, a time limit -- ends the run with
exit code 1 and nothing more is started.  Every line goes to --out as soon as it exists.

1. clips/s of detect_events(median=3, low=0.3) at bs 64 x 10 s, fp32_split, against forward_segments OF THE SAME TREE, same
   process, alternating rounds, the table left on the device [>= 0.97]; and with to_lists() per call.
2. Device time of the new kernels from one `rocprofv3 --kernel-trace --stats` run of that workload: share of the forward
   [<= 2 %], fraction of 8 TB/s (each of the two walks reads the probabilities once; with a median the row that leaves the
   window is read again, from cache).
3. Against decode_events on this machine's own host, same probabilities (sparse synthetic ones, about 0.03 % of the cells at
   or above 0.5): (64, 31, 527) median 3 low 0.3; (8 and 64, 1001, 527) framewise median 7; one (11 250, 527) one-hour
   timeline median 3 -- with and without the read-back -- and that hour's forward_windows(what="segment") beside it [the
   timeline decodes in less time than the forward that made it].
4. (--base-tree: a checkout of the parent commit with its libacx.so built) bench.py headline of both trees, alternating
   [expected 1.00: nothing on its path changes]."""
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

import numpy as np                      # noqa: E402
import torch                            # noqa: E402

from audioset_convnext_inf_amd import synth      # noqa: E402
from audioset_convnext_inf_amd.pytorch import segments as seg      # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny      # noqa: E402

SR = 32000
HBM_PEAK = 8.0e12
OUT = None          # the parent's output file, appended to line by line
DECODE = dict(median=3, low=0.3)


def say(s=""):
    print(s, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(s + "\n")


def make_model(precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth.synth_state_dict(0))
    return m.to("cuda").eval().set_precision(precision)


@torch.no_grad()
def clips_per_s(fn, x, steps=20, warmup=5):
    for _ in range(warmup):
        fn(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn(x)
    b.record()
    b.synchronize()
    return x.shape[0] * steps / (a.elapsed_time(b) / 1000.0)


def section_speed():
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    x = synth.synth_waveforms(64, 10 * SR, seed=1).cuda()
    m = make_model("fp32_split")
    runs = {"segments": [], "detect": [], "lists": []}
    for _ in range(3):
        runs["segments"].append(clips_per_s(lambda v: m.forward_segments(v), x))
        runs["detect"].append(clips_per_s(lambda v: m.detect_events(v, **DECODE), x))
        runs["lists"].append(clips_per_s(lambda v: m.detect_events(v, **DECODE)["events"].to_lists(), x))
    base = max(runs["segments"])
    r = max(runs["detect"]) / base
    n = len(m.detect_events(x, **DECODE)["events"])
    say("1. clips/s at bs 64 x 10 s, fp32_split, same process, best of 3 alternating rounds of 20 steps (%d events per batch):" % n)
    say("   forward_segments %.0f, detect_events(median=3, low=0.3) with the table left on the device %.0f: %.3f  "
        "[target >= 0.97: %s]" % (base, max(runs["detect"]), r, "met" if r >= 0.97 else "MISSED"))
    say("   with to_lists() after every call %.0f: %.3f of forward_segments" % (max(runs["lists"]), max(runs["lists"]) / base))


def section_trace_workload():
    """The workload of the rocprofv3 run: 3 warm-up + 10 calls of detect_events(median=3, low=0.3), bs 64 x 10 s."""
    m = make_model("fp32_split")
    x = synth.synth_waveforms(64, 10 * SR, seed=1).cuda()
    with torch.no_grad():
        for _ in range(13):
            m.detect_events(x, **DECODE)
    torch.cuda.synchronize()


def sparse_probs(shape, seed):
    """About 0.03 % of the cells at or above 0.5, in short bursts; everything else well under the low threshold."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g) * 0.2
    hot = torch.rand(shape, generator=g) < 0.0003
    p[hot] = 0.5 + 0.5 * torch.rand(int(hot.sum()), generator=g)
    return p


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
    say("3. against decode_events on this machine's host (%d CPUs visible), sparse synthetic probabilities, best of 3:"
        % (os.cpu_count() or 0))
    cases = (("64 clips of (31, 527), median 3, low 0.3", (64, 31, 527), dict(median=3, low=0.3), seg.SEGMENT_SECONDS),
             ("8 clips of framewise (1001, 527), median 7", (8, 1001, 527), dict(median=7), 0.01),
             ("64 clips of framewise (1001, 527), median 7", (64, 1001, 527), dict(median=7), 0.01),
             ("one one-hour timeline (11250, 527), median 3", (1, 11250, 527), dict(median=3), seg.SEGMENT_SECONDS))
    hour_decode = None
    for i, (name, shape, kw, step) in enumerate(cases):
        p = sparse_probs(shape, 7 + i)
        frac = float((p >= 0.5).float().mean())
        x = p.cuda()
        host_clips = min(shape[0], 8)                     # the host decodes clip by clip: a few clips give its rate
        pn = p.numpy()
        t_host = best_of(lambda: [seg.decode_events(pn[c], step=step, **kw) for c in range(host_clips)], 2) / host_clips * shape[0]
        for _ in range(2):
            len(seg.decode_events_gpu(x, step=step, **kw))
        t_dev = best_of(lambda: seg.decode_events_gpu(x, step=step, **kw))
        t_all = best_of(lambda: seg.decode_events_gpu(x, step=step, **kw).to_lists())
        t_pcie = best_of(lambda: x.cpu())
        n = len(seg.decode_events_gpu(x, step=step, **kw))
        waves = shape[0] * ((shape[2] + 63) // 64)
        say("   %s (%.3f %% of cells >= 0.5, %d events, %d waves):" % (name, 100 * frac, n, waves))
        say("     host %.4f s (%.1f clips/s%s); device %.6f s without the read-back: %.0f x; %.6f s with to_lists(): %.0f x; "
            "copying the probabilities to the host alone takes %.6f s"
            % (t_host, shape[0] / t_host, "" if host_clips == shape[0] else ", from %d clips" % host_clips, t_dev, t_host / t_dev,
               t_all, t_host / t_all, t_pcie))
        if shape[0] == 1:
            hour_decode = (t_dev, t_all, waves)
    m = make_model("fp32_split")
    hour = synth.synth_waveforms(1, 3600 * SR, seed=3)[0].cuda()
    kw = dict(window=10.0, hop=10.0, what="segment")
    with torch.no_grad():
        m.forward_windows(hour[:SR * 60], **kw)
        t_fw = best_of(lambda: m.forward_windows(hour, **kw), 2)
        rows = m.forward_windows(hour, **kw)["timeline"].shape[0]
    ok = hour_decode[1] < t_fw
    say("   the hour's forward_windows(window=10, hop=10, what=\"segment\") at 32 kHz, same run: %.3f s for %d timeline rows; its "
        "decoding %.6f s (%.6f s with to_lists())  [decode < forward: %s]%s"
        % (t_fw, rows, hour_decode[0], hour_decode[1], "met" if ok else "MISSED",
           "" if ok else "; only %d waves are busy on a single recording (a column is not split along time)" % hour_decode[2]))


SECTIONS = {"speed": section_speed, "trace-workload": section_trace_workload, "host": section_host}


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


def kernel_stats():
    with tempfile.TemporaryDirectory() as d:
        run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--section", "trace-workload"], 300, cwd=d)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            say("2. FAILED: the rocprofv3 run left no kernel statistics")
            sys.exit(1)
        rows = list(csv.DictReader(open(files[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    steps = 13
    say("2. device time of the new kernels, rocprofv3 --kernel-trace --stats, detect_events(median=3, low=0.3), bs 64 x 10 s, "
        "fp32_split (%.3f ms of kernels per call):" % (tot / steps / 1e6))
    B, S, N = 64, 31, 527
    share = 0.0
    for key, ideal_s in (("events_kernel", B * S * N * 4 / HBM_PEAK), ("events_scan_kernel", None)):
        mine = [r for r in rows if key in r["Name"]]
        if not mine:
            say("   %s: not in the trace" % key)
            continue
        calls = sum(int(r["Calls"]) for r in mine)
        ns = sum(float(r["TotalDurationNs"]) for r in mine)
        share += ns / tot
        say("   %-18s %.1f launches per call, %6.1f us each, %.3f %% of the call's device time%s"
            % (key, calls / steps, ns / calls / 1e3, 100 * ns / tot,
               "" if ideal_s is None else ", %.1f %% of 8 TB/s (one read of the probabilities per launch)" % (100 * ideal_s / (ns / calls * 1e-9))))
    say("   together %.3f %% of the device time of forward + decoding  [target <= 2 %%: %s]"
        % (100 * share, "met" if share <= 0.02 else "MISSED"))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_a_events_bench.txt"))
    a = ap.parse_args()
    if a.section:
        return SECTIONS[a.section]()
    OUT = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    run_section("speed", 300)
    if not a.skip_trace:
        kernel_stats()
    if not a.skip_host:
        run_section("host", 420)
    if a.base_tree:
        runs = {"base": [], "new": []}
        for _ in range(3):
            for which, tree in (("base", a.base_tree), ("new", ROOT)):
                runs[which].append(tree_bench(os.path.abspath(tree), ["--gpus", "1", "--steps", "50", "--warmup", "10"])["value"])
        r = max(runs["new"]) / max(runs["base"])
        say("4. bench.py headline (fp32_split, bs 64), three alternating runs each: parent %s, this %s clips/s: best %.3f of the "
            "parent  [expected 1.00]" % (" ".join("%.0f" % v for v in runs["base"]), " ".join("%.0f" % v for v in runs["new"]), r))


if __name__ == "__main__":
    main()
