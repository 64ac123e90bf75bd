#!/usr/bin/env python
"""Per-class AP / ROC-AUC / d' on the device (acx_tagging_metrics, pytorch/metrics.tagging_metrics) against the reference's host
scoring (evaluate.calculate_statistics: sklearn + scipy):
  1. device time of one acx_tagging_metrics call on GPU-resident (20 371, 527) scores and uint8 targets -- the AudioSet eval
     set's shape -- HIP events on the stream, best and median of the repetitions;
  2. tagging_metrics from host numpy arrays (host checks, H2D copy, kernels, D2H of the results) against calculate_statistics on
     the same arrays and host: wall time;
  3. device time at N = 100 003 and N = 1 048 576 (the workspace path; no target);
  4. evaluate_convnext_on_audioset.py --synthetic 20371 wall time with --metrics gpu and --metrics sklearn (one GPU, from the
     script's own timing line, which covers the sweep and the scoring).
Targets (ISSUE, estimates set before measuring): 1. <= 2 ms; 2. >= 100x faster than sklearn on the same host.

    python tools/metrics_bench.py [--skip-script] [--script-n N] > profiles/rNN_metrics_bench.txt
(the script's synthetic set is generated in float64 on the host: 20 371 clips take about 100 GB of host memory at the peak)"""
import os
import re
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audioset_convnext_inf_amd import _ffi                                       # noqa: E402
from audioset_convnext_inf_amd.pytorch.evaluate import calculate_statistics      # noqa: E402
from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics            # noqa: E402

C = 527


def inputs(N, seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    prev = torch.linspace(0.0005, 0.3, C, device=device, dtype=torch.float64)
    t = (torch.rand((N, C), generator=g, device=device, dtype=torch.float64) < prev).to(torch.uint8)
    s = torch.sigmoid(torch.randn((N, C), generator=g, device=device) * 3 + 2.0 * t)
    return t, s


def device_ms(N, reps):
    t, s = inputs(N)
    ws_bytes = _ffi.metrics_workspace_bytes(N, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((3, C), dtype=torch.float64, device="cuda")
    st = torch.empty(1, dtype=torch.int32, device="cuda")
    vp = _ffi.vp
    stream = _ffi.stream_ptr(s.device)

    def call():
        _ffi.check(_ffi.lib().acx_tagging_metrics(vp(s), C, vp(t), _ffi.TARGET_U8, C, N, C, vp(out[0]), vp(out[1]), vp(out[2]),
                                                  vp(st), vp(ws), ws_bytes, stream))
    call()
    torch.cuda.synchronize()
    assert int(st.cpu()[0]) == 0
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return min(times), float(np.median(times)), ws_bytes


def main():
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    best, med, wsb = device_ms(20371, 50)
    print("1. device time, GPU-resident 20371 x 527: best %.3f ms, median %.3f ms (50 calls; workspace %.1f MB)  [target <= 2 ms]"
          % (best, med, wsb / 1e6))

    t, s = inputs(20371, seed=1)
    tn, sn = t.cpu().numpy(), s.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tagging_metrics(tn, sn)
        torch.cuda.synchronize()
        gpu_s = []
        for _ in range(10):
            t0 = time.perf_counter()
            g = tagging_metrics(tn, sn)
            gpu_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = calculate_statistics(tn, sn)
        sk_s = time.perf_counter() - t0
    dev = max(float(np.nanmax(np.abs(g[k] - ref[k]))) for k in ("average_precision", "auc"))
    print("2. from host numpy arrays, 20371 x 527: tagging_metrics best %.2f ms, median %.2f ms (10 calls, incl. host checks, "
          "H2D and D2H); calculate_statistics %.0f ms on the same host (%d CPUs visible): %.0fx  [target >= 100x]; "
          "max |AP, AUC diff| %.1e" % (min(gpu_s) * 1e3, np.median(gpu_s) * 1e3, sk_s * 1e3, len(os.sched_getaffinity(0)),
                                       sk_s / np.median(gpu_s), dev))
    del t, s
    for N, reps in ((100003, 5), (1048576, 2)):
        best, med, wsb = device_ms(N, reps)
        print("3. device time, GPU-resident %d x 527 (workspace path): best %.2f ms, median %.2f ms (%d calls; workspace %.2f GB)"
              % (N, best, med, reps, wsb / 1e9))
        torch.cuda.empty_cache()

    if "--skip-script" in sys.argv:
        return
    n_script = int(sys.argv[sys.argv.index("--script-n") + 1]) if "--script-n" in sys.argv else 20371
    script = os.path.join(ROOT, "evaluate_convnext_on_audioset.py")
    for m in ("gpu", "sklearn"):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, script, "--synthetic", str(n_script), "--metrics", m], capture_output=True, text=True,
                           timeout=1200)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print("4. --metrics %s failed (rc %d): %s" % (m, r.returncode, r.stderr[-800:]))
            sys.exit(1)
        line = re.search(r"^\((\d+) clips in ([0-9.]+) s on .*$", r.stdout, flags=re.M)
        vals = re.findall(r"^Validate .*$", r.stdout, flags=re.M)
        print("4. evaluate_convnext_on_audioset.py --synthetic %d --metrics %-7s: %s  (process wall %.1f s)  %s"
              % (n_script, m, line.group(0) if line else "?", wall, " | ".join(vals)))


if __name__ == "__main__":
    main()
