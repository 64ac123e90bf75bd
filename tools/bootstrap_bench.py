#!/usr/bin/env python
"""Bootstrap confidence intervals on the device (acx_bootstrap_weights / acx_weighted_metrics, pytorch/metrics.py), measured on
one GPU with the inputs resident, medians of five runs after a warm-up -- nothing here is assumed:
  a. device time (HIP events around everything bootstrap_metrics launches: per chunk of 256 replicates the weights and one
     acx_weighted_metrics call) for R = 1000 at (20 371, 527) and (2 000, 50), and the wall time of bootstrap_metrics itself on the
     same resident inputs (adds the D2H copies of the (R, C) statistics and the host percentiles).
  b. the same resamples as a loop over what the library offered before: for each r, scores[idx_r] and target[idx_r] gathered on
     the device, then acx_tagging_metrics with a workspace allocated once and no host synchronisation inside the loop (the index
     vectors are uploaded beforehand, outside the timed window).  Target: a at least 2x faster than b at the first shape.
     The values of the first replicates are compared, so that both sides time the same computation.
  c. where a's time goes: the weights alone, the once-per-call part of acx_weighted_metrics (prep, weight check, plan and ONE
     recount row, measured as a call with a single weight vector, times the number of chunks) and the rest, the recount.
  d. bench.py against the parent commit's library (--parent-lib path/to/parent/libacx.so, loaded through ACX_LIB), alternating
     child processes: target 1.00, nothing it runs changes.  Skipped without --parent-lib.

    python tools/bootstrap_bench.py [--parent-lib PATH] [--replicates 1000] > profiles/rNN_bootstrap_bench.txt"""
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
from audioset_convnext_inf_amd.pytorch import metrics as M                                         # noqa: E402

CHUNK = 256
vp = _ffi.vp


def inputs(N, C, seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    prev = torch.linspace(0.0005, 0.3, C, device=device, dtype=torch.float64)
    t = (torch.rand((N, C), generator=g, device=device, dtype=torch.float64) < prev).to(torch.uint8)
    s = torch.sigmoid(torch.randn((N, C), generator=g, device=device) * 3 + 2.0 * t)
    return t, s


def timed(call, reps=5):
    """median and best device time (ms) of `reps` calls after one warm-up call"""
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
    return float(np.median(times)), min(times)


def shape(N, C, R, seed, first_shape):
    t, s = inputs(N, C)
    stream = _ffi.stream_ptr(s.device)
    st = torch.empty(1, dtype=torch.int32, device="cuda")
    # ---- a: what bootstrap_metrics launches
    wws_bytes = _ffi.weighted_metrics_workspace_bytes(N, C)
    wws = torch.empty(wws_bytes, dtype=torch.uint8, device="cuda")
    w = torch.empty((CHUNK, N), dtype=torch.int32, device="cuda")
    out = torch.empty((3, R, C), dtype=torch.float64, device="cuda")
    chunks = [(f, min(CHUNK, R - f)) for f in range(0, R, CHUNK)]

    def draw(first, k):
        _ffi.bootstrap_weights(seed, first, k, N, vp(w), N, stream)

    def weighted(first, k):
        _ffi.weighted_metrics(vp(s), C, vp(t), _ffi.TARGET_U8, C, N, C, vp(w), N, k, vp(out[0, first]), vp(out[1, first]),
                              vp(out[2, first]), vp(st), (vp(wws), wws_bytes), stream)

    def ours():
        for first, k in chunks:
            draw(first, k)
            weighted(first, k)

    a_med, a_best = timed(ours)
    assert int(st.cpu()[0]) == 0
    mine = out[:, :4].cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        M.bootstrap_metrics(t, s, replicates=R, seed=seed, chunk=CHUNK)
        wall = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M.bootstrap_metrics(t, s, replicates=R, seed=seed, chunk=CHUNK)
            wall.append(time.perf_counter() - t0)
    print("a. (%d, %d), R = %d in chunks of %d: device time median %.2f ms, best %.2f ms (5 runs); bootstrap_metrics on the same "
          "resident inputs, wall: median %.1f ms, best %.1f ms" % (N, C, R, CHUNK, a_med, a_best, np.median(wall) * 1e3, min(wall) * 1e3))
    # ---- c: shares
    w_med, _ = timed(lambda: [draw(f, k) for f, k in chunks])
    draw(0, 1)
    once_med, _ = timed(lambda: weighted(0, 1))
    ours()                                                  # (out[:, 0] holds replicate 0 again)
    once = once_med * len(chunks)
    print("c. of a's %.2f ms: weights %.2f ms (%.0f %%); once per call -- prep, weight check, plan, one recount row -- %.3f ms x %d "
          "chunks = %.2f ms (%.0f %%); recount, the rest: %.2f ms (%.0f %%)"
          % (a_med, w_med, 100 * w_med / a_med, once_med, len(chunks), once, 100 * once / a_med, a_med - w_med - once,
             100 * (a_med - w_med - once) / a_med))
    # ---- b: the loop over gathered rows
    idx = torch.from_numpy(np.stack([M.bootstrap_indices_host(seed, r, N) for r in range(R)])).cuda()
    ws_bytes = _ffi.metrics_workspace_bytes(N, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    ref = torch.empty((3, R, C), dtype=torch.float64, device="cuda")

    def loop():
        for r in range(R):
            sr, tr = s.index_select(0, idx[r]), t.index_select(0, idx[r])
            _ffi.tagging_metrics(vp(sr), C, vp(tr), _ffi.TARGET_U8, C, N, C, vp(ref[0, r]), vp(ref[1, r]), vp(ref[2, r]), vp(st),
                                 (vp(ws), ws_bytes), stream)

    b_med, b_best = timed(loop)
    theirs = ref[:, :4].cpu().numpy()
    defined = ~np.isnan(mine[0])                            # (a class whose resample has no positive: NaN here, AP 0 there)
    worst = float(np.nanmax(np.abs(mine[:2] - theirs[:2])[:, defined], initial=0.0))
    ratio = b_med / a_med
    print("b. the loop over the same %d resamples -- gather scores[idx_r] / target[idx_r], acx_tagging_metrics, no synchronisation "
          "inside: median %.1f ms, best %.1f ms (5 runs) = %.2fx a%s; AP / AUC of the first 4 replicates agree to %.1e"
          % (R, b_med, b_best, ratio, ("  [target >= 2x: %s]" % ("met" if ratio >= 2.0 else "MISSED")) if first_shape else "", worst))
    return ratio


def part_d(parent_lib, steps, warmup):
    def bench(lib):
        env = dict(os.environ)
        if lib:
            env["ACX_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                            str(warmup)], capture_output=True, text=True, env=env, timeout=900)
        if r.returncode != 0:
            print("d. bench.py failed (rc %d): %s" % (r.returncode, r.stderr[-800:]))
            sys.exit(1)
        return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])
    vals = {"parent": [], "this tree": []}
    for _ in range(2):
        vals["parent"].append(bench(parent_lib))
        vals["this tree"].append(bench(None))
    a, b = max(vals["parent"]), max(vals["this tree"])
    print("d. bench.py --gpus 1 --steps %d --warmup %d, two alternating child processes each, best: parent library %.1f clips/s "
          "%r, this tree %.1f clips/s %r = %.3f  [target 1.00]" % (steps, warmup, a, [round(v, 1) for v in vals["parent"]], b,
                                                                     [round(v, 1) for v in vals["this tree"]], b / a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libacx.so built from the parent commit: runs part d")
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.parent_lib:                                        # first: child processes, before this one opens the device
        part_d(os.path.abspath(a.parent_lib), a.steps, a.warmup)
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    shape(20371, 527, a.replicates, a.seed, True)
    torch.cuda.empty_cache()
    shape(2000, 50, a.replicates, a.seed, False)
    if not a.parent_lib:
        print("d. bench.py against the parent: not run (no --parent-lib)")


if __name__ == "__main__":
    main()
