#!/usr/bin/env python
"""Live streams (ConvNeXt.stream, acx_stream_*):
  1. steady state after a 10 s fill: 256 slots, 10 s windows, 1 s hop, 1 s pushes; push() windows/s, results included,
     against model(x) of the same 256 windows pre-cut; at 32 kHz and at 44.1 kHz;
  2. (`--prof`: only the 32 kHz and 44.1 kHz push loops, for a `rocprofv3 --kernel-trace --stats` run of its own: the append,
     resample and timeline kernels against the push's device time);
  3. one slot with 1 s pushes: push() to probabilities on the host, p50 / p99, against model(x) of one 10 s window;
  4. capacity: live 10 s / 1 s streams one GPU sustains (windows/s of 1., one window per stream per second).
Targets (ISSUE, set before measuring): 1. >= 0.97 of model(x) at 32 kHz, >= 0.95 at 44.1 kHz; 2. < 2 % of the device time;
3. p50 <= 1.25 x model(x) of one window.

    python tools/stream_bench.py [precision] [--prof] > profiles/rNN_stream_bench.txt"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audioset_convnext_inf_amd import synth                                          # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny                 # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
precision = args[0] if args else "fp32_split"
prof = "--prof" in sys.argv
SR, W, H, SLOTS = 32000, 320000, 32000, 256


def model_for(p):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth.synth_state_dict(0))
    return m.to("cuda").eval().set_precision(p)


def steady(model, rate, pushes):
    """windows/s of push() with 256 slots after a 10 s fill; every push emits one window per slot."""
    sec = rate
    audio = synth.synth_waveforms(1, sec * (10 + pushes + 2), seed=3)[0].cuda()
    st = model.stream(slots=SLOTS, window=10.0, hop=1.0, sample_rate=rate, max_push=1.0)
    for k in range(10):
        st.push([audio[k * sec:(k + 1) * sec]] * SLOTS)
    st.push([audio[10 * sec:11 * sec]] * SLOTS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for k in range(11, 11 + pushes):
        d = st.push([audio[k * sec:(k + 1) * sec]] * SLOTS)
        d["clipwise_output"].cpu()
        n += d["slot"].numel()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n


def direct(model, reps):
    x = synth.synth_waveforms(SLOTS, W, seed=4).cuda()
    model(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        model(x)["clipwise_output"].cpu()
    torch.cuda.synchronize()
    return SLOTS * reps / (time.perf_counter() - t0)


model = model_for(precision)
print("device %s, torch %s, precision %s" % (torch.cuda.get_device_name(0), torch.__version__, precision))
if prof:
    steady(model, 32000, 5)
    steady(model, 44100, 5)
    sys.exit(0)

ref = direct(model, 8)
for rate, target in ((32000, 0.97), (44100, 0.95)):
    wps, n = steady(model, rate, 8)
    print("1. %d Hz: push() %.0f windows/s (%d windows), model(x) pre-cut %.0f windows/s: %.3f  [target >= %.2f: %s]"
          % (rate, wps, n, ref, wps / ref, target, "met" if wps / ref >= target else "missed"))

one = synth.synth_waveforms(1, W, seed=5).cuda()
for _ in range(3):
    model(one)["clipwise_output"].cpu()
lat1 = []
for _ in range(50):
    t0 = time.perf_counter()
    model(one)["clipwise_output"].cpu()
    lat1.append(time.perf_counter() - t0)
audio = synth.synth_waveforms(1, SR * 80, seed=6)[0].cuda()
st = model.stream(slots=1, window=10.0, hop=1.0, max_push=1.0)
for k in range(10):
    st.push([audio[k * SR:(k + 1) * SR]])
lat = []
for k in range(10, 80):
    t0 = time.perf_counter()
    st.push([audio[k * SR:(k + 1) * SR]])["clipwise_output"].cpu()
    lat.append(time.perf_counter() - t0)
lat.sort()
lat1.sort()
p50, p99, m50 = lat[len(lat) // 2], lat[int(len(lat) * 0.99)], lat1[len(lat1) // 2]
print("3. one slot, 1 s pushes: push -> host probabilities p50 %.3f ms, p99 %.3f ms; model(x) of one 10 s window p50 %.3f ms: "
      "%.2fx  [target p50 <= 1.25x: %s]" % (p50 * 1e3, p99 * 1e3, m50 * 1e3, p50 / m50, "met" if p50 <= 1.25 * m50 else "missed"))
for p in ("fp32_split", "bf16a"):
    wps, _ = steady(model_for(p), 32000, 6)
    print("4. capacity %s: %.0f windows/s = %d live 10 s / 1 s streams" % (p, wps, int(wps)))
