"""Cases for the host plumbing of the evaluation sweep (pytorch/evaluate.py: forward, _Stager), shared by tests/test_sweep_cpu.py
and tests/test_gpu_sweep_order.py.

The sweep moves every batch through a pinned ring, a per-slot int16 device buffer, three float32 buffers used in turn, a copy
stream, a fetch stream and events between them.  A missing wait changes nothing at the timing a machine happens to give, so the
timing is made adversarial on purpose: a model, a stager and a reader that each hold one party of the sweep back, while every
sample that was staged still reaches an output through arithmetic that is EXACT -- max, min and the library's widening
float(double(x) / 32767).  Every comparison is np.array_equal; a race shows as wrong numbers, nothing else."""
import time

import numpy as np
import torch
from torch import nn

from audioset_convnext_inf_amd.pytorch import evaluate as ev

CLASSES = 527
L = 4 * CLASSES                 # samples per clip: the echo model has no minimum length
# Eleven batches: more than two turns of the pinned ring (4) and more than three of the float32 buffers (3); the sizes grow at three
# different slots in mid-sweep, which takes every "buffer too small, replace it" branch of the stager; the last batch is short.
SIZES = [8, 8, 8, 8, 8, 24, 24, 8, 24, 40, 3]
kLagMs = 20.0                   # what every forced lag aims at (gpu_lag, LaggedStager, host_lag); at most kLagMaxMs per use
kLagMaxMs = 25.0


class EchoModel(nn.Module):
    """x (B, L) -> {"clipwise_output": max, "segmentwise_output": min} over the L / 527 segments of each clip: every sample of the
    staged batch reaches an output unchanged.  gpu_lag: cycles of torch.cuda._sleep on the current stream before x is read (the
    compute stream runs late); host_lag: seconds slept in forward (the consumer runs late, the reader its full depth ahead);
    fail_at: the n-th call (from 1) raises."""

    def __init__(self, gpu_lag=0, host_lag=0.0, fail_at=None):
        super().__init__()
        self.anchor = nn.Parameter(torch.zeros(1))      # evaluate.forward finds the device through model.parameters()
        self.gpu_lag, self.host_lag, self.fail_at = int(gpu_lag), float(host_lag), fail_at
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        if self.fail_at is not None and self.calls == self.fail_at:
            raise RuntimeError("EchoModel: call %d fails as asked" % self.calls)
        if self.host_lag:
            time.sleep(self.host_lag)
        if self.gpu_lag:
            torch.cuda._sleep(self.gpu_lag)
        x = x.view(x.shape[0], x.shape[1] // CLASSES, CLASSES)
        return {"clipwise_output": x.max(dim=1).values, "segmentwise_output": x.min(dim=1).values}


class LaggedStager(ev._Stager):
    """A stager whose copy stream runs late: every to_device first queues `cycles` of GPU sleep on the copy stream."""

    def __init__(self, device, cycles):
        super().__init__(device)
        self.cycles = int(cycles)
        self.copy_stream = torch.cuda.Stream(device, priority=-1)       # as _Stager.to_device makes it

    def to_device(self, staged):
        with torch.cuda.stream(self.copy_stream):
            torch.cuda._sleep(self.cycles)
        return super().to_device(staged)


def waveforms(sizes, L, seed, dtype):
    """One (B, L) array per batch: full-range int16, or float32 in [-1, 1)."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return [rng.integers(-32768, 32768, size=(b, L), dtype=np.int16) for b in sizes]
    return [rng.uniform(-1.0, 1.0, size=(b, L)).astype(np.float32) for b in sizes]


def batches(sizes, L, seed, dtype, reader_lag=0.0, pinned=False, fail_after=None):
    """The sweep's generator: {"waveform", "target"} per batch, the target carrying the batch index.  reader_lag: seconds slept
    before every batch; pinned: the waveform is a pinned torch tensor (the stager then copies straight out of it);
    fail_after: raise instead of yielding batch number `fail_after`."""
    for i, w in enumerate(waveforms(sizes, L, seed, dtype)):
        if fail_after is not None and i == fail_after:
            raise RuntimeError("reader: fails after %d batches as asked" % i)
        if reader_lag:
            time.sleep(reader_lag)
        yield {"waveform": torch.from_numpy(w).pin_memory() if pinned else w,
               "target": np.full((w.shape[0],), i, dtype=np.float32)}


def widen(w):
    """What the model must have been given: the library's float(double(x) / 32767) for int16, the samples themselves otherwise."""
    return (w / 32767.0).astype(np.float32) if w.dtype == np.int16 else w


def expected(sizes, L, seed, dtype):
    """The host fold of the same batches: what forward(EchoModel(), batches(...), return_target=True) must return, bit for bit."""
    f = [widen(w).reshape(w.shape[0], L // CLASSES, CLASSES) for w in waveforms(sizes, L, seed, dtype)]
    return {"clipwise_output": np.concatenate([x.max(axis=1) for x in f]),
            "segmentwise_output": np.concatenate([x.min(axis=1) for x in f]),
            "target": np.concatenate([np.full((b,), i, dtype=np.float32) for i, b in enumerate(sizes)])}


def assert_exact(out, want):
    for key in ("target", "clipwise_output", "segmentwise_output"):
        assert out[key].dtype == want[key].dtype and out[key].shape == want[key].shape, key
        bad = np.flatnonzero((out[key] != want[key]).reshape(out[key].shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s differs in %d rows, first at row %d" % (key, bad.size, bad[0])
        assert np.array_equal(out[key], want[key]), key


def walk(sizes, ring=ev._Stager.kRing, turns=3):
    """Where the stager puts each int16 batch of a fresh sweep, restated from _Stager.to_pinned / to_device: per batch
    (slot, turn, replaced), `replaced` being the buffers that existed and were too small ("pinned" and "dev16" per slot, "dev32"
    per turn).  A first allocation is not a replacement."""
    slot_rows, turn_rows, rows = [0] * ring, [0] * turns, []
    for i, b in enumerate(sizes):
        slot, turn = i % ring, i % turns
        replaced = []
        if 0 < slot_rows[slot] < b:
            replaced += ["pinned", "dev16"]
        if 0 < turn_rows[turn] < b:
            replaced += ["dev32"]
        slot_rows[slot], turn_rows[turn] = max(slot_rows[slot], b), max(turn_rows[turn], b)
        rows.append((slot, turn, tuple(replaced)))
    return rows


def calibrated_sleep(target_ms):
    """Cycles of torch.cuda._sleep that last target_ms on this device: what one cycle lasts depends on the build, so a probe is
    timed with events (the minimum of 3 runs).  -> (cycles, measured milliseconds of that count, again the minimum of 3)."""
    def timed(cycles):
        best = float("inf")
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            best = min(best, a.elapsed_time(b))
        return best
    probe = 2000000
    timed(probe)                                        # first launch
    ms = timed(probe)
    if ms < 0.5:                                        # too short to time well: a longer probe
        probe *= 20
        ms = timed(probe)
    cycles = max(1, int(probe * target_ms / ms))
    return cycles, timed(cycles)


def unlagged_batch_ms(device, rows=max(SIZES)):
    """One echo batch at natural timing -- staging, copy, widening, echo, fetch of both outputs -- the minimum of 3 after a warm-up."""
    stage, model = ev._Stager(device), EchoModel().to(device)
    w = waveforms([rows], L, 99, np.int16)[0]
    best = float("inf")
    for k in range(4):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        out = model(stage.to_device(stage.to_pinned(w)))
        got = [out[key].cpu() for key in ("clipwise_output", "segmentwise_output")]
        torch.cuda.synchronize(device)
        if k:
            best = min(best, (time.perf_counter() - t0) * 1e3)
    del got
    stage.close()
    return best
