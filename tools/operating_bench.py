#!/usr/bin/env python
"""Per-class operating points on the device (acx_operating_points / acx_threshold_counts, pytorch/metrics.py) and the event
decoder with per-class levels (acx_decode_events_classwise), measured -- nothing here is assumed:
  a. device time of acx_operating_points on GPU-resident (20 371, 527) scores and uint8 targets, per criterion, against
     acx_tagging_metrics on the same inputs in the same process (HIP events, best and median).  It runs the same prep and the
     same sorts plus one sweep of met_count's shape: the target is <= 1.5x the existing call.
  b. operating_points from host numpy arrays (checks, H2D, kernels, D2H) against sklearn.metrics.precision_recall_curve looped
     over the classes with the max-F1 pick, on the same host: wall time.
  c. acx_threshold_counts on the same inputs: device time, and the bytes it reads (scores fp32 + targets uint8) as a fraction of
     8 TB/s.
  d. detect_events at bs 64 x 10 s with a per-class threshold / low tensor against the same call with scalars, same process
     (medians of alternating timed windows): the kernel gains two loads per wave, target >= 0.99.
  e. bench.py against the parent commit's library (--parent-lib path/to/parent/libacx.so, loaded through ACX_LIB), alternating
     child processes: target 1.00.  Skipped without --parent-lib.

    python tools/operating_bench.py [--parent-lib PATH] [--skip-model] > profiles/rNN_operating_bench.txt"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audioset_convnext_inf_amd import _ffi                                                         # noqa: E402
from audioset_convnext_inf_amd.pytorch.metrics import operating_points, operating_points_host      # noqa: E402

N, C = 20371, 527
CRITERIA = [("f1", _ffi.OP_FBETA, 1.0), ("fbeta 2", _ffi.OP_FBETA, 2.0), ("precision 0.9", _ffi.OP_PRECISION, 0.9),
            ("recall 0.8", _ffi.OP_RECALL, 0.8)]
vp = _ffi.vp


def inputs(seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    prev = torch.linspace(0.0005, 0.3, C, device=device, dtype=torch.float64)
    t = (torch.rand((N, C), generator=g, device=device, dtype=torch.float64) < prev).to(torch.uint8)
    s = torch.sigmoid(torch.randn((N, C), generator=g, device=device) * 3 + 2.0 * t)
    return t, s


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return min(times), float(np.median(times))


def part_a_c():
    t, s = inputs()
    ws_bytes = _ffi.metrics_workspace_bytes(N, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((3, C), dtype=torch.float64, device="cuda")
    thr = torch.empty(C, dtype=torch.float32, device="cuda")
    cnt = torch.empty((C, 4), dtype=torch.int64, device="cuda")
    st = torch.empty(1, dtype=torch.int32, device="cuda")
    stream = _ffi.stream_ptr(s.device)
    base = timed(lambda: _ffi.tagging_metrics(vp(s), C, vp(t), _ffi.TARGET_U8, C, N, C, vp(out[0]), vp(out[1]), vp(out[2]), vp(st),
                                              (vp(ws), ws_bytes), stream), 50)
    print("a. device time, GPU-resident %d x %d, 50 calls each: acx_tagging_metrics best %.3f ms, median %.3f ms" % (N, C, *base))
    for name, crit, param in CRITERIA:
        got = timed(lambda: _ffi.operating_points(vp(s), C, vp(t), _ffi.TARGET_U8, C, N, C, crit, param, vp(thr), vp(cnt), vp(st),
                                                  (vp(ws), ws_bytes), stream), 50)
        assert int(st.cpu()[0]) == 0
        ratio = got[1] / base[1]
        print("   acx_operating_points %-14s best %.3f ms, median %.3f ms = %.2fx acx_tagging_metrics  [target <= 1.5x: %s]"
              % (name, got[0], got[1], ratio, "met" if ratio <= 1.5 else "MISSED"))
    got = timed(lambda: _ffi.threshold_counts(vp(s), C, vp(t), _ffi.TARGET_U8, C, N, C, vp(thr), vp(cnt), vp(st), stream), 50)
    assert int(st.cpu()[0]) == 0
    read = N * C * 5
    print("c. acx_threshold_counts, the same inputs (%.1f MB read): best %.1f us, median %.1f us (two clears and two kernels) = "
          "%.3f of 8 TB/s at the median" % (read / 1e6, got[0] * 1e3, got[1] * 1e3, read / (got[1] * 1e-3) / 8e12))
    return t, s


def part_b(t, s):
    from sklearn.metrics import precision_recall_curve
    tn, sn = t.cpu().numpy(), s.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        operating_points(tn, sn)
        gpu_s = []
        for _ in range(10):
            t0 = time.perf_counter()
            op = operating_points(tn, sn)
            thr = op.threshold.cpu().numpy()
            gpu_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sk = np.full(C, np.inf, np.float32)
        for c in range(C):
            if tn[:, c].any():
                p, r, th = precision_recall_curve(tn[:, c], sn[:, c])
                f = 2 * p * r / np.maximum(p + r, 1e-300)
                sk[c] = th[np.argmax(f[:-1])]
        sk_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = operating_points_host(tn, sn)
        host_s = time.perf_counter() - t0
    same = int((thr.view(np.uint32) == ref.threshold.view(np.uint32)).sum())
    print("b. from host numpy arrays, %d x %d, max F1: operating_points best %.2f ms, median %.2f ms (10 calls, incl. host checks, "
          "H2D and D2H); the sklearn precision_recall_curve loop %.0f ms on the same host (%d CPUs visible): %.0fx; "
          "operating_points_host %.0f ms; thresholds equal to operating_points_host bit for bit in %d of %d classes, to the sklearn "
          "pick (first maximum of its own F1) in %d" % (N, C, min(gpu_s) * 1e3, np.median(gpu_s) * 1e3, sk_s * 1e3,
                                                         len(os.sched_getaffinity(0)), sk_s / np.median(gpu_s), host_s * 1e3, same, C,
                                                         int((thr == sk).sum())))


def part_d():
    from audioset_convnext_inf_amd import synth
    from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    model.load_state_dict(synth.synth_state_dict(0))
    model = model.to("cuda").eval()
    wav = synth.synth_waveforms(64, 320000, seed=3).cuda()
    thr = torch.full((C,), 0.5, device="cuda")
    low = torch.full((C,), 0.3, device="cuda")
    calls = {"scalar": lambda: model.detect_events(wav, threshold=0.5, low=0.3, median=3),
             "per-class": lambda: model.detect_events(wav, threshold=thr, low=low, median=3)}
    rates = {k: [] for k in calls}
    with torch.no_grad():
        for k in calls:
            for _ in range(5):
                calls[k]()
        torch.cuda.synchronize()
        for _ in range(5):                                  # alternating windows of 20 calls
            for k in calls:
                t0 = time.perf_counter()
                for _ in range(20):
                    calls[k]()
                torch.cuda.synchronize()
                rates[k].append(20 * 64 / (time.perf_counter() - t0))
        n = (len(calls["scalar"]()["events"]), len(calls["per-class"]()["events"]))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    ratio = med["per-class"] / med["scalar"]
    print("d. detect_events, bs 64 x 10 s, median=3 (fp32_split), medians of 5 alternating windows of 20 calls: scalar levels %.0f "
          "clips/s, per-class tensors %.0f clips/s = %.3f  [target >= 0.99: %s]; %d / %d events"
          % (med["scalar"], med["per-class"], ratio, "met" if ratio >= 0.99 else "MISSED", n[0], n[1]))


def part_e(parent_lib, steps, warmup):
    def bench(lib):
        env = dict(os.environ)
        if lib:
            env["ACX_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                            str(warmup)], capture_output=True, text=True, env=env, timeout=900)
        if r.returncode != 0:
            print("e. bench.py failed (rc %d): %s" % (r.returncode, r.stderr[-800:]))
            sys.exit(1)
        return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])
    vals = {"parent": [], "this tree": []}
    for _ in range(2):
        vals["parent"].append(bench(parent_lib))
        vals["this tree"].append(bench(None))
    a, b = max(vals["parent"]), max(vals["this tree"])
    print("e. bench.py --gpus 1 --steps %d --warmup %d, two alternating child processes each, best: parent library %.1f clips/s "
          "%r, this tree %.1f clips/s %r = %.3f  [target 1.00]" % (steps, warmup, a, [round(v, 1) for v in vals["parent"]], b,
                                                                     [round(v, 1) for v in vals["this tree"]], b / a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libacx.so built from the parent commit: runs part e")
    ap.add_argument("--skip-model", action="store_true", help="skip parts d and e (no model forwards)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.parent_lib and not a.skip_model:                   # first: child processes, before this one opens the device
        part_e(os.path.abspath(a.parent_lib), a.steps, a.warmup)
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    t, s = part_a_c()
    part_b(t, s)
    del t, s
    torch.cuda.empty_cache()
    if a.skip_model:
        return
    part_d()
    if not a.parent_lib:
        print("e. bench.py against the parent: not run (no --parent-lib)")


if __name__ == "__main__":
    main()
