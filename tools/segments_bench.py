#!/usr/bin/env python
"""Sound event detection ("Segment-wise and frame-wise outputs"): the measurements behind
profiles/r14_a_segments_bench.txt.  Measured, not asserted; targets in brackets, misses stated as misses.

    python tools/segments_bench.py [--base-tree DIR] [--out profiles/r14_a_segments_bench.txt]

The process started this way never opens the GPU.  Every measurement is a child process of its own under `timeout -k 10 N`
(the sections below; `rocprofv3 ... -- python tools/segments_bench.py --section trace-workload` for 3; `bench.py` for 5), run
one after the other; the first child that does not exit with 0 -- a failure, a fault, an abort, a time limit -- ends the run
with exit code 1 and nothing more is started.  Every line goes to --out as soon as it exists.

1. clips/s of forward_segments at bs 64 x 10 s against model(x) OF THE SAME TREE, same process, alternating rounds:
   resolution="segment" [>= 0.97 of model(x)], resolution="frame", fp32_split and bf16a.  model(x)'s own path is the parent
   commit's, byte for byte; 5 compares the two trees.
2. Against the only way to get these outputs before: stock torch ops on forward_frame_embeddings (mean, max_pool1d + avg_pool1d,
   layer_norm, linear, sigmoid, repeat_interleave) [>= 1.0 x], with the peak device memory of both.
3. Device time of the new kernels from one `rocprofv3 --kernel-trace --stats` run: share of the forward, fraction of the f32-matrix peak (head) and of 8 TB/s (pooling, expansion).
4. One hour at 44.1 kHz, forward_windows(window=10, hop=10, what="segment"): seconds and timeline rows; beside it
   what="logits", hop=1.0 -- the coarser timeline it replaces (the parent has that path, same code).
5. (--base-tree: a checkout of the parent commit with its libacx.so built) bench.py headline of both trees, alternating
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

import torch                            # noqa: E402
import torch.nn.functional as F         # noqa: E402

from audioset_convnext_inf_amd import synth      # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny      # noqa: E402

SR = 32000
F32_MATRIX_PEAK = 157.3e12
HBM_PEAK = 8.0e12
OUT = None          # the parent's output file, appended to line by line


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


def torch_ops_baseline(m):
    """forward_segments(resolution="frame") from stock torch ops on forward_frame_embeddings."""
    nw, nb = m.norm.weight.data, m.norm.bias.data
    hw, hb = m.head_audioset.weight.data, m.head_audioset.bias.data

    def run(x):
        z = m.forward_frame_embeddings(x).mean(dim=3)
        p = F.max_pool1d(z, 3, 1, 1) + F.avg_pool1d(z, 3, 1, 1)
        q = torch.sigmoid(F.linear(F.layer_norm(p.transpose(1, 2), (768,), nw, nb, 1e-6), hw, hb))
        T = x.shape[1] // 320 + 1
        fr = torch.repeat_interleave(q, 32, dim=1)
        if fr.shape[1] < T:
            fr = torch.cat((fr, fr[:, -1:].expand(-1, T - fr.shape[1], -1)), dim=1)
        return q, q.max(1).values, fr[:, :T].contiguous()
    return run


@torch.no_grad()
def peak_mib(fn, x):
    fn(x)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(x)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def section_speed():
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    x = synth.synth_waveforms(64, 10 * SR, seed=1).cuda()
    say("1. clips/s at bs 64 x 10 s against model(x) of the same tree, same process, best of 3 alternating rounds of 20 steps:")
    models = {}
    for prec in ("fp32_split", "bf16a"):
        m = models[prec] = make_model(prec)
        runs = {"model(x)": [], "segment": [], "frame": []}
        for _ in range(3):
            runs["model(x)"].append(clips_per_s(m, x))
            runs["segment"].append(clips_per_s(lambda v: m.forward_segments(v), x))
            runs["frame"].append(clips_per_s(lambda v: m.forward_segments(v, resolution="frame"), x))
        base = max(runs["model(x)"])
        for key in ("segment", "frame"):
            r = max(runs[key]) / base
            target = "  [target >= 0.97: %s]" % ("met" if r >= 0.97 else "MISSED") if (prec, key) == ("fp32_split", "segment") else ""
            say("   %-10s model(x) %.0f, forward_segments(resolution=\"%s\") %.0f: %.3f%s" % (prec, base, key, max(runs[key]), r, target))
    m = models["fp32_split"]
    tb = torch_ops_baseline(m)
    ours = lambda v: m.forward_segments(v, resolution="frame")
    r_t, r_o = [], []
    for _ in range(3):
        r_t.append(clips_per_s(tb, x))
        r_o.append(clips_per_s(ours, x))
    ratio = max(r_o) / max(r_t)
    say("2. against stock torch ops on forward_frame_embeddings (segment + clip + frame outputs, fp32_split): torch %.0f, "
        "forward_segments %.0f clips/s: %.3f x  [target >= 1.0 x: %s]" % (max(r_t), max(r_o), ratio, "met" if ratio >= 1.0 else "MISSED"))
    say("   peak device memory of one call beyond the inputs and the workspace held: torch ops %.0f MiB, forward_segments "
        "%.0f MiB" % (peak_mib(tb, x), peak_mib(ours, x)))


def section_trace_workload():
    """The workload of the rocprofv3 run: 3 warm-up + 10 forwards of forward_segments(resolution="frame"), bs 64 x 10 s."""
    m = make_model("fp32_split")
    x = synth.synth_waveforms(64, 10 * SR, seed=1).cuda()
    with torch.no_grad():
        for _ in range(13):
            m.forward_segments(x, resolution="frame")
    torch.cuda.synchronize()


def section_hour():
    m = make_model("fp32_split")
    hour = synth.synth_waveforms(1, 3600 * 44100, seed=3)[0].cuda()
    res = {}
    with torch.no_grad():
        for tag, kw in (("segment", dict(window=10.0, hop=10.0, what="segment")), ("logits", dict(window=10.0, hop=1.0, what="logits"))):
            m.forward_windows(hour[:44100 * 60], sample_rate=44100, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.forward_windows(hour, sample_rate=44100, **kw)
            torch.cuda.synchronize()
            res[tag] = (time.perf_counter() - t0, out["timeline"].shape[0], out["starts"].shape[0])
    say("4. one hour at 44.1 kHz, fp32_split: forward_windows(window=10, hop=10, what=\"segment\") %.2f s, %d forwards, %d timeline "
        "rows of 0.32 s; what=\"logits\", hop=1.0 (the 1 s timeline it replaces) %.2f s, %d forwards, %d rows"
        % (res["segment"][0], res["segment"][2], res["segment"][1], res["logits"][0], res["logits"][2], res["logits"][1]))


SECTIONS = {"speed": section_speed, "trace-workload": section_trace_workload, "hour": section_hour}


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
            say("3. FAILED: the rocprofv3 run left no kernel statistics")
            sys.exit(1)
        rows = list(csv.DictReader(open(files[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    steps = 13
    say("3. device time of the new kernels, rocprofv3 --kernel-trace --stats, bs 64 x 10 s, fp32_split, resolution=\"frame\" "
        "(%.3f ms of kernels per forward):" % (tot / steps / 1e6))
    B, S, N, T = 64, 31, 527, 1001
    work = {"segment_pool": ("of 8 TB/s", (B * S * 7 * 768 * 4 + B * S * 768 * 4) / HBM_PEAK),
            "segment_head": ("of the f32-matrix peak", 2.0 * B * S * N * 768 / F32_MATRIX_PEAK),
            "segment_clipmax": ("of 8 TB/s", (B * S * N * 4 + B * N * 4) / HBM_PEAK),
            "segment_expand": ("of 8 TB/s", (B * T * N * 4 + B * S * N * 4) / HBM_PEAK)}
    share = 0.0
    for key, (what, ideal_s) in work.items():
        mine = [r for r in rows if key in r["Name"]]
        if not mine:
            say("   %s: not in the trace" % key)
            continue
        ns = sum(float(r["TotalDurationNs"]) for r in mine) / sum(int(r["Calls"]) for r in mine)
        calls = sum(int(r["Calls"]) for r in mine) / steps
        share += ns * calls * steps / tot
        say("   %-16s %.1f launches per forward, %7.1f us each, %.2f %% of the forward, %.1f %% %s"
            % (key, calls, ns / 1e3, 100 * ns * calls * steps / tot, 100 * ideal_s / (ns * 1e-9) / max(1, round(calls)), what))
    say("   together %.2f %% of the forward's device time" % (100 * share))


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
    ap.add_argument("--skip-hour", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_a_segments_bench.txt"))
    a = ap.parse_args()
    if a.section:
        return SECTIONS[a.section]()
    OUT = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    run_section("speed", 300)
    if not a.skip_trace:
        kernel_stats()
    if not a.skip_hour:
        run_section("hour", 420)
    if a.base_tree:
        runs = {"base": [], "new": []}
        for _ in range(3):
            for which, tree in (("base", a.base_tree), ("new", ROOT)):
                runs[which].append(tree_bench(os.path.abspath(tree), ["--gpus", "1", "--steps", "50", "--warmup", "10"])["value"])
        r = max(runs["new"]) / max(runs["base"])
        say("5. bench.py headline (fp32_split, bs 64), three alternating runs each: parent %s, this %s clips/s: best %.3f of the "
            "parent  [expected 1.00]" % (" ".join("%.0f" % v for v in runs["base"]), " ".join("%.0f" % v for v in runs["new"]), r))


if __name__ == "__main__":
    main()
