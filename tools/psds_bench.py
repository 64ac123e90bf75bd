#!/usr/bin/env python
"""Intersection criteria and PSDS on the device ("Scoring events on the device"): the measurements behind
profiles/r25_a_psds_bench.txt.  Measured, not asserted; expectations in brackets, misses stated as misses.

    python tools/psds_bench.py [--base-tree DIR] [--out profiles/r25_a_psds_bench.txt]

The process started this way never opens the GPU.  Every measurement is a child process of its own under `timeout -k 10 N`
(`rocprofv3 ... -- python tools/psds_bench.py --section trace-...` for (a); `bench.py` for (c)), run one after the other; the
first child that does not exit with 0 -- a failure, a fault, an abort, a time limit -- ends the run with exit code 1 and nothing
more is started.  Every line goes to --out as soon as it exists.

0. Registers and scratch of the two new kernels, from the code objects inside the built library [no scratch, as the other scorers].
(a) Device time of acx_score_intersection, without and with the cross-trigger matrix (one `rocprofv3 --kernel-trace --stats` run
    each: the kernel has one name), against acx_score_events and acx_decode_events on the same table: detect_events(median=3) at
    bs 64 x 10 s, 527 classes [within the decoder's own time; the ratio is recorded either way].
(b) psds with 50 thresholds on (1168 clips x 156 steps x 10 classes) and on (2048 x 31 x 527), both scenarios, against the host
    loop of decode_events + intersection_based_metrics_host + psds_host on the same arrays.  The host loop is timed on
    --host-points of the 50 thresholds (evenly spread interior points; 1: the middle one) and scaled to 50; the line says so
    [the device path ahead: >= 1.0 x].
(c) (--base-tree: a checkout of the parent commit with its libacx.so built) bench.py headline of both trees, alternating
    [expected 1.00: no forward kernel changes]."""
import argparse
import csv
import glob
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np                      # noqa: E402
import torch                            # noqa: E402

import sed_score_bench as sb            # noqa: E402
from audioset_convnext_inf_amd.pytorch import sed_metrics as sm      # noqa: E402
from audioset_convnext_inf_amd.pytorch import segments as seg      # noqa: E402

say = sb.say
TRACE_CALLS = 13
CRITERIA = {name: {k: v for k, v in preset.items() if k.endswith("_threshold")} for name, preset in sm.PSDS_SCENARIOS.items()}


def trace_workload(criteria):
    probs, args, table, reference, ref, est, ends = sb.batch_case()
    for _ in range(TRACE_CALLS):
        t = seg.decode_events_gpu(probs, **args)
        sm.event_based_metrics(reference, t)
        sm.intersection_based_metrics(reference, t, **criteria)
    torch.cuda.synchronize()


def probabilities(B, S, N, active, seed=0):
    """smoothed noise through a sigmoid, shifted so that about `active` of the cells reach 0.5; fp32 CUDA (B, S, N)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(B, S + 4, N, generator=g, device="cuda")
    z = (z[:, :-4] + z[:, 1:-3] + z[:, 2:-2] + z[:, 3:-1] + z[:, 4:]) / 5 ** 0.5
    shift = float(torch.quantile(z.flatten()[:1 << 22], 1.0 - active))
    return torch.sigmoid(3.0 * (z - shift)).contiguous()


def section_psds(host_points):
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("(b) psds, 50 thresholds (the default grid), step 0.32 s, median=3, max_efpr 100 per hour; device: best of 3, synchronised; "
        "host loop: decode_events + intersection_based_metrics_host on %d of the 50 thresholds, scaled to 50, + psds_host, on "
        "this machine's host (%d CPUs visible):" % (host_points, os.cpu_count() or 0))
    thresholds = np.linspace(0.01, 0.99, 50).astype(np.float32)
    for B, S, N, active in ((1168, 156, 10, 0.2), (2048, 31, 527, 0.02)):
        p = probabilities(B, S, N, active)
        table = seg.decode_events_gpu(p, threshold=0.5, median=3, capacity=p.numel() // 2 + 1)
        est = table.to_lists()
        ends = [float(e[-1]) for e in table.edges]
        ref = sb.annotations(est, ends, N, seg.SEGMENT_SECONDS)
        reference = sm.ReferenceEvents.from_lists(ref, N, device="cuda")
        host_p = p.cpu().numpy()
        pick = thresholds[np.linspace(0, 49, host_points + 2)[1:-1].astype(int)]          # interior points, evenly spread
        for scenario in sorted(CRITERIA):
            run = lambda: sm.psds(p, reference, scenario=scenario, median=3, capacity=len(table) * 2 + 1024)   # noqa: E731
            run()
            t_dev = sb.best_of(run)
            got = run()
            t0 = time.perf_counter()
            scores = []
            for t in pick:
                lists = [seg.decode_events(host_p[i], threshold=float(t), median=3) for i in range(B)]
                scores.append(sm.intersection_based_metrics_host(ref, lists, N, **CRITERIA[scenario]))
            t_points = time.perf_counter() - t0
            same = all(np.array_equal(got.counts[int(np.nonzero(thresholds == t)[0][0])].cpu().numpy(), s.counts)
                       for t, s in zip(pick, scores))
            t_host = t_points * 50 / host_points
            say("   %4d x %3d x %3d (%d events at 0.5, %d annotated) %s: device %.3f s, value %.4f; host %.1f s for %d points -> "
                "%.0f s for 50: %.0f x  [>= 1.0 x: %s]; counts of those points equal: %s"
                % (B, S, N, len(table), len(reference), scenario, t_dev, got.value, t_points, host_points, t_host, t_host / t_dev,
                   "met" if t_host >= t_dev else "MISSED", same))


def resources():
    import check_exclusive
    lib = os.path.join(ROOT, "audioset-convnext-inf_amd", "libacx.so")
    say("0. registers and scratch, from the code objects inside %s:" % os.path.relpath(lib, ROOT))
    for name, threads, vgpr, scratch in sorted(check_exclusive.kernels_of(lib)):
        if "sed_intersection_kernel" in name or "cross_trigger_rate_kernel" in name or "sed_event_match_kernel" in name:
            say("   %-70s up to %4d threads, %3d vector registers, %d bytes of scratch  [no scratch: %s]"
                % (name[:70], threads, vgpr, scratch, "met" if scratch == 0 else "MISSED"))


def kernel_stats(section):
    with tempfile.TemporaryDirectory() as d:
        sb.run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                      os.path.abspath(__file__), "--section", section], 300, cwd=d)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            say("(a) FAILED: the rocprofv3 run left no kernel statistics")
            sys.exit(1)
        rows = list(csv.DictReader(open(files[0])))
    us = lambda key: sum(float(r["TotalDurationNs"]) for r in rows if key in r["Name"]) / 1e3      # noqa: E731
    dec = (us("events_kernel") + us("events_scan_kernel")) / (TRACE_CALLS + 1)       # batch_case decodes once more
    return dec, us("sed_event_match_kernel") / TRACE_CALLS, us("sed_intersection_kernel") / TRACE_CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=["trace-plain", "trace-matrix", "psds"], help="run one measurement in this process")
    ap.add_argument("--base-tree", default=None, help="checkout of the parent commit, its library built (bench.py A/B)")
    ap.add_argument("--host-points", type=int, default=2)
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--skip-psds", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_a_psds_bench.txt"))
    a = ap.parse_args()
    if a.section == "psds":
        return section_psds(a.host_points)
    if a.section:
        return trace_workload(CRITERIA["dcase_1" if a.section == "trace-plain" else "dcase_2"])
    sb.OUT = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(sb.OUT), exist_ok=True)
    open(sb.OUT, "w").close()
    resources()
    if not a.skip_trace:
        say("(a) device time per call, rocprofv3 --kernel-trace --stats, bs 64 x 10 s, 527 classes, one run per form:")
        for section, what in (("trace-plain", "dtc = gtc = 0.7, no matrix"), ("trace-matrix", "dtc = gtc = 0.1, cttc = 0.3, 527 x 527 matrix")):
            dec, ev, inter = kernel_stats(section)
            say("   %-46s acx_score_intersection %8.1f us; acx_score_events %8.1f us; acx_decode_events %8.1f us: %.2f of the "
                "decoder  [within the decoder's time: %s]" % (what, inter, ev, dec, inter / dec, "met" if inter <= dec else "MISSED"))
    if not a.skip_psds:
        for line in sb.run_child([sys.executable, os.path.abspath(__file__), "--section", "psds", "--host-points", str(a.host_points)],
                                 900).splitlines():
            say(line)
    if a.base_tree:
        runs = {"base": [], "new": []}
        for _ in range(3):
            for which, tree in (("base", a.base_tree), ("new", ROOT)):
                runs[which].append(sb.tree_bench(os.path.abspath(tree), ["--gpus", "1", "--steps", "50", "--warmup", "10"])["value"])
        say("(c) bench.py headline (bs 64), three alternating runs each: parent %s, this %s clips/s: best %.3f of the parent  "
            "[expected 1.00]" % (" ".join("%.0f" % v for v in runs["base"]), " ".join("%.0f" % v for v in runs["new"]),
                                 max(runs["new"]) / max(runs["base"])))


if __name__ == "__main__":
    main()
