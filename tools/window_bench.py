#!/usr/bin/env python
"""Sliding windows over long recordings (ConvNeXt.forward_windows, acx_forward_windows / acx_window_timeline):
  1. non-overlapping windows (hop = window = 10 s) over one 640 s recording against model(x) of the same 64 windows pre-cut:
     clips/s;
  2. one hour at 44.1 kHz, window 10 s, hop 1 s (3 591 windows): forward_windows(sample_rate=44100, max_batch=64) against the
     do-it-yourself torch path (device resample -> unfold -> .contiguous() -> model(x) in 64-window chunks -> torch mean over
     the windows of each step): wall time and peak device memory;
  3. the timeline kernel alone on those 3 591 windows' probabilities (HIP events) against the forward time.
Targets (ISSUE, set before measuring): 1. >= 0.98 of model(x)'s clips/s; 2. no slower than the torch path, lower peak memory;
3. timeline < 1 % of the forward.

    python tools/window_bench.py [precision] > profiles/rNN_window_bench.txt"""
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audioset_convnext_inf_amd import _ffi, synth                                    # noqa: E402
from audioset_convnext_inf_amd.pytorch import windows as win                         # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny                 # noqa: E402
from audioset_convnext_inf_amd.pytorch.resample import resample                      # noqa: E402

precision = sys.argv[1] if len(sys.argv) > 1 else "fp32_split"
print("precision %s" % precision)
SR, W, H = 32000, 320000, 32000


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


m = convnext_tiny(after_stem_dim=[252, 56])
m.load_state_dict(synth.synth_state_dict(0))
m = m.cuda().eval().set_precision(precision)

# 1. hop = window over 640 s
rec = synth.synth_waveforms(1, 640 * SR, seed=1)[0].cuda()
cut = rec.view(64, W).contiguous()
t_win, t_uni = [], []
for _ in range(3):                       # alternated, same process
    t_uni.append(timed(lambda: m(cut), reps=5))
    t_win.append(timed(lambda: m.forward_windows(rec, window=10.0, timeline=None), reps=5))
c_uni, c_win = 64 / min(t_uni), 64 / min(t_win)
print("640 s, window = hop = 10 s (64 windows): model(x) of the pre-cut windows %.2f ms (%.0f clips/s) | forward_windows "
      "%.2f ms (%.0f clips/s) | ratio %.3f" % (min(t_uni) * 1e3, c_uni, min(t_win) * 1e3, c_win, c_win / c_uni))
del cut

# 2. one hour at 44.1 kHz, window 10 s, hop 1 s
hour = synth.synth_waveforms(1, 3600 * 44100, seed=2)[0].cuda()


def diy():
    x = resample(hour, 44100)
    L = x.numel()
    starts = win.window_starts([L], W, H)
    frames = x.unfold(0, W, H)                                  # full windows every hop
    if (L - W) % H:                                             # plus the end-aligned last one
        frames = torch.cat([frames, x[L - W:][None]])
    frames = frames.contiguous()
    probs = torch.cat([m(frames[i:i + 64])["clipwise_output"] for i in range(0, frames.shape[0], 64)])
    mids = torch.tensor(win.timeline_steps([L], W, H), device=probs.device)
    s = torch.tensor(starts, device=probs.device)
    cover = ((s[None, :] <= mids[:, None]) & (mids[:, None] < s[None, :] + W)).float()
    return probs, (cover @ probs) / cover.sum(1, keepdim=True)


def ours():
    out = m.forward_windows(hour, window=10.0, hop=1.0, sample_rate=44100)
    return out["clipwise_output"], out["timeline"]


n = ours()[0].shape[0]
peaks, times = {}, {}
for name, fn in (("torch", diy), ("forward_windows", ours), ("torch", diy), ("forward_windows", ours)):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = timed(fn, reps=1)
    times[name] = min(times.get(name, float("inf")), t)
    peaks[name] = torch.cuda.max_memory_allocated() - base
print("1 h at 44.1 kHz, window 10 s, hop 1 s (%d windows): forward_windows %.3f s (%.0f windows/s, peak +%.0f MiB) | torch "
      "unfold path %.3f s (%.0f windows/s, peak +%.0f MiB) | time ratio torch/ours %.3f | peak memory ratio ours/torch %.3f"
      % (n, times["forward_windows"], n / times["forward_windows"], peaks["forward_windows"] / 2**20, times["torch"],
         n / times["torch"], peaks["torch"] / 2**20, times["torch"] / times["forward_windows"],
         peaks["forward_windows"] / peaks["torch"]))

# 3. the timeline kernel alone
probs = ours()[0].contiguous()
L = _ffi.resampled_length(44100, 32000, hour.numel())
steps = len(win.timeline_steps([L], W, H))
tl = torch.empty((steps, 527), device="cuda")
lens = (ctypes.c_int64 * 1)(L)


def timeline():
    _ffi.check(_ffi.lib().acx_window_timeline(_ffi.ptr(probs), lens, 1, W, H, 0, _ffi.ptr(tl), _ffi.stream_ptr(probs.device)))


timeline()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(20):
    timeline()
b.record()
b.synchronize()
t_tl = a.elapsed_time(b) / 1e3 / 20
print("timeline kernel (mean, %d steps x 527 over %d windows): %.1f us = %.3f %% of the forward_windows call"
      % (steps, n, t_tl * 1e6, 100 * t_tl / times["forward_windows"]))
