#!/usr/bin/env python
"""The augmented forwards (csrc/augment.hip, acx_forward_augmented, acx_forward_features; include/acx.h) at bs 64 x 10 s, in
fp32_split and bf16a, every comparison in one process with alternating repeats:
  (a) forward_augmented(AugmentPolicy.reference()) against model(x): clips/s ratio (bar: >= 0.97);
  (b) the same with all three waveform augmentations on (gain 7 dB, roll 50, speed (0.5, 1.5) at p = 1) (bar: >= 0.97);
  (c) acx_logmel_bn0 over the whole batch + acx_forward_features against acx_forward: what running the frontend un-split costs
      (recorded, no target);
  (d) device time of the two kernels alone (HIP events around back-to-back launches): the gather and the mixing form as a
      share of 8 TB/s by their algorithmic traffic (gather: fp32 input read once + output written once; mix: two maps read,
      one written), the in-place mask against the bytes it writes (recorded, no target).
(a) and (b) draw the plan on the host inside the timed call, as a fine-tuning loop would.  The plans of (d) are drawn once.

    python tools/augment_bench.py > profiles/r26_a_augment_bench.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audioset_convnext_inf_amd import _ffi, synth                                    # noqa: E402
from audioset_convnext_inf_amd.pytorch import augment as A                           # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny                 # noqa: E402

HBM = 8.0e12
B, L = 64, 320000
T = L // 320 + 1
REPS, ROUNDS = 40, 3           # windows of 0.2 - 0.3 s: the first call's host work, which nothing overlaps, stays under 1 %
FULL = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=1.0)
assert torch.cuda.is_available(), "augment_bench needs a GPU"
dev = torch.device("cuda", torch.cuda.current_device())


def timed(fn, reps=REPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def alternate(fns):
    """Median seconds per call of each fn, ROUNDS rounds of REPS calls each, the fns taking turns."""
    for fn in fns:
        fn()                                             # warm every shape
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            times[i].append(timed(fn))
    return [float(np.median(t)) for t in times]


def event_timed(fn, reps=100):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


x = synth.synth_waveforms(B, L, seed=1).to(dev)
stream = _ffi.stream_ptr(dev)
lib = _ffi.lib()
for precision in ("fp32_split", "bf16a"):
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56])
    model.load_state_dict(synth.synth_state_dict(0))
    model = model.to(dev).eval().set_precision(precision)
    ctx = model.native_context(dev)
    g = torch.Generator().manual_seed(0)
    t_plain, t_ref, t_full = alternate([lambda: model(x), lambda: model.forward_augmented(x, generator=g),
                                        lambda: model.forward_augmented(x, policy=FULL, generator=g)])
    print("%s (a) model(x) %.1f clips/s, forward_augmented(reference()) %.1f clips/s: ratio %.3f (bar 0.97)"
          % (precision, B / t_plain, B / t_ref, t_plain / t_ref))
    print("%s (b) forward_augmented(gain + roll + speed + SpecAugment) %.1f clips/s: ratio %.3f (bar 0.97)"
          % (precision, B / t_full, t_plain / t_full))
    feat = torch.empty((B, T, 224), device=dev)
    ws = torch.empty(ctx.workspace_bytes(B, L, "logits"), dtype=torch.uint8, device=dev)
    o0, o1 = torch.empty((B, 527), device=dev), torch.empty((B, 527), device=dev)

    def staged():
        _ffi.check(lib.acx_logmel_bn0(ctx.handle, _ffi.ptr(x), B, L, _ffi.ptr(feat), 1, stream))
        _ffi.check(lib.acx_forward_features(ctx.handle, _ffi.ptr(feat), B, L, 0, _ffi.ptr(o0), _ffi.ptr(o1), _ffi.ptr(ws), ws.numel(),
                                            stream))

    def whole():
        _ffi.check(lib.acx_forward(ctx.handle, _ffi.ptr(x), B, L, 0, _ffi.ptr(o0), _ffi.ptr(o1), _ffi.ptr(ws), ws.numel(), stream))
    t_whole, t_staged = alternate([whole, staged])
    print("%s (c) acx_forward %.1f clips/s, acx_logmel_bn0 + acx_forward_features %.1f clips/s: ratio %.3f (no target)"
          % (precision, B / t_whole, B / t_staged, t_whole / t_staged))

# (d) the kernels alone
plan = A.draw_plan(A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=1.0), B, L, torch.Generator().manual_seed(1)).to(dev)
out = torch.empty_like(x)
dt = event_timed(lambda: _ffi.check(lib.acx_augment_wave(_ffi.ptr(x), B, L, _ffi.ptr(plan.wave_dev), _ffi.ptr(out), stream)))
nbytes = 2 * 4 * B * L
print("(d) augment_wave_kernel %d x %d: %.1f us, %.1f MB read + written once = %.2f TB/s = %.3f of 8 TB/s"
      % (B, L, dt * 1e6, nbytes / 1e6, nbytes / dt / 1e12, nbytes / dt / HBM))
feat = torch.randn((B, T, 224), device=dev)
mix = torch.empty((B // 2, T, 224), device=dev)
lam = torch.from_numpy(A.mixup_lambdas(B, 0.5).astype(np.float32)).to(dev)
dt = event_timed(lambda: _ffi.check(lib.acx_augment_spec(_ffi.ptr(feat), B, T, _ffi.ptr(plan.spec_dev), _ffi.ptr(lam), _ffi.ptr(mix),
                                                         stream)))
nbytes = 4 * T * 224 * (B + B // 2)
print("(d) augment_spec_mix_kernel %d x %d x 224: %.1f us, %.1f MB (two maps read, one written) = %.2f TB/s = %.3f of 8 TB/s"
      % (B, T, dt * 1e6, nbytes / 1e6, nbytes / dt / 1e12, nbytes / dt / HBM))
dt = event_timed(lambda: _ffi.check(lib.acx_augment_spec(_ffi.ptr(feat), B, T, _ffi.ptr(plan.spec_dev), None, _ffi.ptr(feat), stream)))
s = plan.spec
written = 4 * int((s["t_len"].astype(np.int64) * 224 + s["f_len"].astype(np.int64) * T).sum())
print("(d) augment_spec_mask_kernel %d x %d x 224 in place: %.1f us for %.2f MB written (stripes as drawn, overlaps counted "
      "twice) = %.3f TB/s; the whole map is %.1f MB" % (B, T, dt * 1e6, written / 1e6, written / dt / 1e12, 4 * B * T * 224 / 1e6))
