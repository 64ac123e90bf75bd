#!/usr/bin/env python
"""Online event decoding ("Decoding events online"): the measurements behind profiles/r22_a_event_stream_bench.txt.
Measured, not asserted; expectations in brackets, misses stated as misses.

    python tools/event_stream_bench.py [--base-tree DIR] [--out profiles/r22_a_event_stream_bench.txt]

The process started this way never opens the GPU.  Every measurement is a child process of its own under `timeout -k 10 N`
(the sections below; `rocprofv3 ... -- python tools/event_stream_bench.py --section trace-workload` for the kernels' share;
`bench.py` for c), run one after the other; the first child that does not exit with 0 -- a failure, a fault, an abort, a time
limit -- ends the run with exit code 1 and nothing more is started.  Every line goes to --out as soon as it exists.

a. Stream.push at 256 slots, 10 s windows every 1 s, 1 s pushes, fp32_split: seconds per push in the steady state (every push
   completes one window per slot) with events= against events=None, same process, five alternating repeats each [the ratio
   lies inside the spread of the events=None repeats]; and from one `rocprofv3 --kernel-trace --stats` run of the events=
   workload the decoder kernels' share of the device time [< 2 %, the bracket of the stream's own helper kernels].
b. One recording's whole timeline, 11 250 x 527 (one hour of 0.32 s rows), median 3: a single push plus close against
   acx_decode_events on the same rows [about 1 x: both walk the rows twice; above 1.5 x is explained].
c. (--base-tree: a checkout of the parent commit with its libacx.so built) bench.py headline of both trees, alternating
   [expected 1.00: no forward kernel changes]."""
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

import torch                            # noqa: E402

from audioset_convnext_inf_amd import synth      # noqa: E402
from audioset_convnext_inf_amd.pytorch import segments as seg      # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny      # noqa: E402

SR = 32000
SLOTS = 256
OUT = None          # the parent's output file, appended to line by line
DECODE = dict(threshold=0.5, low=0.3, median=3, merge_gap=1.5)
FILL, MEASURED = 10, 8      # pushes that fill the first window, pushes timed after them


def say(s=""):
    print(s, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(s + "\n")


def make_model(precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth.synth_state_dict(0))
    return m.to("cuda").eval().set_precision(precision)


def push_seconds(m, audio, events, pushes=MEASURED):
    """seconds per 1 s push of all slots once every push completes a window per slot; the handle is made and closed here"""
    st = m.stream(slots=SLOTS, window=10.0, hop=1.0, max_push=1.0, events=events)
    with torch.no_grad():
        for k in range(FILL):
            st.push({s: audio[s, k * SR:(k + 1) * SR] for s in range(SLOTS)})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(FILL, FILL + pushes):
            st.push({s: audio[s, k * SR:(k + 1) * SR] for s in range(SLOTS)})
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / pushes
        st.close()
    st.close_handle()
    return dt


def section_push():
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    m = make_model("fp32_split")
    audio = synth.synth_waveforms(SLOTS, (FILL + MEASURED) * SR, seed=2).cuda()
    push_seconds(m, audio, None, 2)
    push_seconds(m, audio, DECODE, 2)
    runs = {"none": [], "events": []}
    for _ in range(5):
        runs["none"].append(push_seconds(m, audio, None))
        runs["events"].append(push_seconds(m, audio, DECODE))
    lo, hi = min(runs["none"]), max(runs["none"])
    med = lambda v: sorted(v)[len(v) // 2]
    r = med(runs["events"]) / med(runs["none"])
    inside = lo / med(runs["none"]) <= r <= hi / med(runs["none"])
    say("a. Stream.push, %d slots, 10 s windows every 1 s, 1 s pushes, fp32_split, %d steady pushes per repeat, five alternating "
        "repeats, ms per push:" % (SLOTS, MEASURED))
    say("   events=None  %s" % " ".join("%.2f" % (1e3 * v) for v in runs["none"]))
    say("   events=%r  %s" % (DECODE, " ".join("%.2f" % (1e3 * v) for v in runs["events"])))
    say("   median with events / median without: %.4f; the events=None repeats span %.4f .. %.4f of their median  "
        "[inside the spread: %s]" % (r, lo / med(runs["none"]), hi / med(runs["none"]), "met" if inside else "MISSED"))


def section_trace_workload():
    """The workload of the rocprofv3 run: the fill, then MEASURED steady pushes with events=, then the close."""
    m = make_model("fp32_split")
    audio = synth.synth_waveforms(SLOTS, (FILL + MEASURED) * SR, seed=2).cuda()
    push_seconds(m, audio, DECODE)


def best_of(fn, n=5):
    best = float("inf")
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def section_hour():
    g = torch.Generator().manual_seed(9)
    p = torch.rand((11250, 527), generator=g) * 0.2
    hot = torch.rand(p.shape, generator=g) < 0.0003
    p[hot] = 0.5 + 0.5 * torch.rand(int(hot.sum()), generator=g)
    x = p.cuda()
    kw = dict(median=3, low=0.3)
    es = seg.EventStream(1, 527, **kw)

    def online():
        return es.push(x, capacity=8192), es.close(capacity=8192)

    def batch():
        return seg.decode_events_gpu(x, capacity=8192, **kw)
    n_on = sum(len(t) for t in online())
    n_b = len(batch())
    t_on, t_b = best_of(online), best_of(batch)
    say("b. one recording's timeline (11250, 527), median 3, low 0.3, sparse synthetic rows (%d events online, %d from the batch "
        "call), best of 5, the tables left on the device:" % (n_on, n_b))
    say("   one push plus close %.6f s, acx_decode_events %.6f s: %.2f x  [about 1 x expected%s]"
        % (t_on, t_b, t_on / t_b, "" if t_on / t_b <= 1.5 else
           "; MISSED: beside the two walks the online form has the close's three launches and its end table, loads and stores "
           "the state of every column in both passes and writes the ring"))


SECTIONS = {"push": section_push, "trace-workload": section_trace_workload, "hour": section_hour}


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
            say("   FAILED: the rocprofv3 run left no kernel statistics")
            sys.exit(1)
        rows = list(csv.DictReader(open(files[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    say("   device time, rocprofv3 --kernel-trace --stats, the events= workload (fill, %d steady pushes, close; %.1f ms of kernels):"
        % (MEASURED, tot / 1e6))
    share = 0.0
    for key in ("events_online_kernel", "events_scan_kernel", "events_online_open_kernel", "events_online_end_kernel"):
        mine = [r for r in rows if key in r["Name"]]
        if not mine:
            say("   %s: not in the trace" % key)
            continue
        calls = sum(int(r["Calls"]) for r in mine)
        ns = sum(float(r["TotalDurationNs"]) for r in mine)
        share += ns / tot
        say("   %-26s %4d launches, %6.1f us each, %.3f %% of the device time" % (key, calls, ns / calls / 1e3, 100 * ns / tot))
    say("   the decoder's kernels together %.3f %% of the device time  [< 2 %%: %s]" % (100 * share, "met" if share < 0.02 else "MISSED"))


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
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_a_event_stream_bench.txt"))
    a = ap.parse_args()
    if a.section:
        return SECTIONS[a.section]()
    OUT = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    run_section("push", 420)
    if not a.skip_trace:
        kernel_stats()
    run_section("hour", 120)
    if a.base_tree:
        runs = {"base": [], "new": []}
        for _ in range(3):
            for which, tree in (("base", a.base_tree), ("new", ROOT)):
                runs[which].append(tree_bench(os.path.abspath(tree), ["--gpus", "1", "--steps", "50", "--warmup", "10"])["value"])
        r = max(runs["new"]) / max(runs["base"])
        say("c. bench.py headline (fp32_split, bs 64), three alternating runs each: parent %s, this %s clips/s: best %.3f of the "
            "parent  [expected 1.00]" % (" ".join("%.0f" % v for v in runs["base"]), " ".join("%.0f" % v for v in runs["new"]), r))


if __name__ == "__main__":
    main()
