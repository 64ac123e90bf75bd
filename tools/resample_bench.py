#!/usr/bin/env python
"""Input resampling on the device (acx_resample, include/acx.h):
  1. the kernel alone, 64 x 10 s clips at 44.1 and 48 kHz -> 32 kHz: device time per call (HIP events around back-to-back
     launches) and the algorithmic bytes (fp32 input read once + output written once) over it, as a share of 8 TB/s;
  2. model(x, sample_rate=44100) at bs 64 against model(x) of the same clips already at 32 kHz: clips/s;
  3. extraction of 256 ragged 44.1 kHz clips of 15-30 s: extract(pack=True, sample_rate=44100) against host resampling with
     utils/resample.py (the reference's order: resample on the CPU, then `.to(device)`) followed by extract(pack=True).
Targets (ISSUE): kernel >= 0.5 of 8 TB/s; sample_rate=44100 >= 0.97 of the 32 kHz clips/s; device path >= 10x the host path.

    python tools/resample_bench.py [precision] > profiles/rNN_resample_bench.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audioset_convnext_inf_amd import _ffi, synth                                    # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny                 # noqa: E402
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract             # noqa: E402
from audioset_convnext_inf_amd.utils.resample import resample as host_resample       # noqa: E402

HBM = 8.0e12
precision = sys.argv[1] if len(sys.argv) > 1 else "fp32_split"
print("precision %s, torch threads %d" % (precision, torch.get_num_threads()))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def event_timed(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


# 1. the kernel
dev = torch.cuda.current_device()
for rate in (44100, 48000):
    L = 10 * rate
    wav = torch.randn(64 * L, device="cuda")
    N = _ffi.resampled_length(rate, 32000, L)
    out = torch.empty(64 * N, device="cuda")
    rs = _ffi.Resampler(dev, rate, 32000)
    of, nf, width, mb = _ffi.resample_geometry(rate, 32000)
    dt = event_timed(lambda: rs.run(wav, [L] * 64, out), reps=100)
    nbytes = 4 * (64 * L + 64 * N)
    print("kernel %5d -> 32000 Hz, 64 x 10 s (of/nf %d/%d, <= %d taps): %7.1f us  %.2f TB/s  %.3f of 8 TB/s  (%.1f MB moved)"
          % (rate, of, nf, mb, dt * 1e6, nbytes / dt / 1e12, nbytes / dt / HBM, nbytes / 1e6))
    rs.close()

# 2. forward at bs 64
m = convnext_tiny(after_stem_dim=[252, 56])
m.load_state_dict(synth.synth_state_dict(0))
m = m.cuda().eval().set_precision(precision)
x44 = synth.synth_waveforms(64, 441000, seed=1).cuda()
x32 = synth.synth_waveforms(64, 320000, seed=1).cuda()
t44, t32 = [], []
for _ in range(3):                      # alternated, same process
    t32.append(timed(lambda: m(x32), reps=10))
    t44.append(timed(lambda: m(x44, sample_rate=44100), reps=10))
c32, c44 = 64 / min(t32), 64 / min(t44)
print("forward bs 64, 10 s clips: 32 kHz input %.2f ms (%.0f clips/s) | 44.1 kHz input, sample_rate=44100 %.2f ms (%.0f clips/s)"
      " | ratio %.3f" % (min(t32) * 1e3, c32, min(t44) * 1e3, c44, c44 / c32))

# 3. extraction of ragged 44.1 kHz clips
rng = np.random.RandomState(0)
lengths = rng.randint(15 * 44100, 30 * 44100 + 1, size=256)
wavs = [synth.synth_waveforms(1, int(n), seed=i)[0] for i, n in enumerate(lengths)]
audio = float(np.sum(lengths)) / 44100
extract(m, wavs[:8], what="scene", pack=True, sample_rate=44100)                   # warm-up
extract(m, [host_resample(w[None], 44100, 32000)[0] for w in wavs[:8]], what="scene", pack=True)


def host_path():
    return extract(m, [host_resample(w[None], 44100, 32000)[0] for w in wavs], what="scene", pack=True)


dt_d = timed(lambda: extract(m, wavs, what="scene", pack=True, sample_rate=44100), reps=1)
dt_h = timed(host_path, reps=1)
dt_d2 = timed(lambda: extract(m, wavs, what="scene", pack=True, sample_rate=44100), reps=1)
dt_d = min(dt_d, dt_d2)
print("extract(pack=True) 256 clips of 15-30 s at 44.1 kHz (%.0f s of audio): device resampling %.3f s (%.1f clips/s, "
      "%.0f audio-s/s) | host utils.resample + extract %.3f s (%.1f clips/s) | x%.1f"
      % (audio, dt_d, 256 / dt_d, audio / dt_d, dt_h, 256 / dt_h, dt_h / dt_d))
