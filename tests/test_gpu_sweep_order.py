"""GPU (`-m gpu`): the evaluation sweep (pytorch/evaluate.py: forward, _Stager) held to its stream order under forced lag.

The end-to-end sweep tests run both sides of their comparison through the same sweep at natural timing, where a missing wait is
invisible.  Here one party at a time is held back (tests/sweep_cases.py) -- the compute stream, the copy stream, the consumer, the
reader -- while an echo model carries every staged sample to an output through exact arithmetic: each ordering statement of the
sweep then has a test that returns wrong numbers without it.  All comparisons are np.array_equal.

The lag is a stimulus, not a pass criterion: `lag` calibrates torch.cuda._sleep to sweep_cases.kLagMs, checks that this is at
least ten times one un-lagged echo batch and at most kLagMaxMs, and prints both."""
import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd.pytorch import evaluate as ev
import sweep_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEY = ("cuda", 0)
INPUTS = {"int16": (np.int16, False), "float32": (np.float32, False),             # dev16 / dev32 path; host.to() path
          "pinned_int16": (np.int16, True), "pinned_float32": (np.float32, True)}   # `slot is None` path


@pytest.fixture(scope="module")
def lag():
    """-> cycles of torch.cuda._sleep for the forced lag."""
    cycles, lag_ms = sc.calibrated_sleep(sc.kLagMs)
    batch_ms = sc.unlagged_batch_ms(DEV)
    print("\nsweep order: forced lag %.2f ms (%d cycles of _sleep); one un-lagged echo batch of %d clips %.3f ms"
          % (lag_ms, cycles, max(sc.SIZES), batch_ms))
    assert lag_ms <= sc.kLagMaxMs, "the lag is longer than a test may spend per use"
    assert lag_ms >= 10 * batch_ms, "the lag does not dominate a batch: it would not reorder anything"
    return cycles


@pytest.fixture
def clean_cache():
    ev.drop_stagers()
    yield
    torch.cuda.synchronize()
    ev.drop_stagers()


def seed_stager(stage):
    ev.release_stager(stage)
    assert ev._stager_key(DEV) == KEY and ev._STAGERS[KEY] is stage
    return stage


def plain_stager():
    stage = ev._Stager(DEV)
    stage.copy_stream = torch.cuda.Stream(DEV, priority=-1)         # as to_device makes it
    return stage


def check_buffers(stage, sizes, dtype, pinned):
    """The real stager against the table of sweep_cases.walk (tests/test_sweep_cpu.py::test_slot_and_turn_table), after a first
    sweep: every buffer ended at the largest batch of its slot / turn -- the replacement branches were taken where the table says."""
    rows = sc.walk(sizes)
    per_slot = [max([b for b, r in zip(sizes, rows) if r[0] == s], default=0) * sc.L for s in range(stage.kRing)]
    per_turn = [max([b for b, r in zip(sizes, rows) if r[1] == t], default=0) * sc.L for t in range(3)]
    numel = lambda bufs: [0 if b is None else b.numel() for b in bufs]      # noqa: E731
    assert numel(stage.pinned) == ([0] * stage.kRing if pinned else per_slot)
    assert numel(stage.dev16) == (per_slot if dtype == np.int16 and not pinned else [0] * stage.kRing)
    assert numel(stage.dev32) == (per_turn if dtype == np.int16 and not pinned else [0, 0, 0])
    assert stage.turn == (0 if pinned else len(sizes) % stage.kRing)


@pytest.mark.parametrize("inp", sorted(INPUTS))
@pytest.mark.parametrize("how", ["none", "compute", "copy", "host_consumer", "reader"])
def test_sweep_under_lag(lag, clean_cache, how, inp):
    """Eleven batches with one party held back: the outputs equal the host fold, the targets are in order, and a second sweep
    (other data, so that a stale buffer cannot pass for a right one) on the same stager straight afterwards is exact as well."""
    dtype, pinned = INPUTS[inp]
    stage = seed_stager(sc.LaggedStager(DEV, lag) if how == "copy" else plain_stager())
    for seed in (31, 32):
        model = sc.EchoModel(gpu_lag=lag if how == "compute" else 0, host_lag=0.020 if how == "host_consumer" else 0.0).to(DEV)
        reader = sc.batches(sc.SIZES, sc.L, seed, dtype, reader_lag=0.005 if how == "reader" else 0.0, pinned=pinned)
        out = ev.forward(model, reader, return_target=True)
        sc.assert_exact(out, sc.expected(sc.SIZES, sc.L, seed, dtype))
        assert model.calls == len(sc.SIZES)
        assert ev._STAGERS[KEY] is stage
        if seed == 31:
            check_buffers(stage, sc.SIZES, dtype, pinned)


@pytest.mark.parametrize("late", ["compute", "copy"])
def test_ring_turn_without_a_host_wait(lag, late):
    """Directly on a stager, with no consumer that waits for outputs between batches (forward() does, which hides these two):
    kRing + 2 batches are staged while one stream is asleep.
    late = compute: the widening kernels of batches 0, 1 have not read their int16 buffers when batches kRing, kRing + 1 are
    copied into them -- the copy stream waits for dev16_read[slot].
    late = copy: the copies of batches 0, 1 have not read their pinned buffers when the reader stages batches kRing, kRing + 1
    there -- to_pinned waits for ready[slot]."""
    stage = sc.LaggedStager(DEV, lag) if late == "copy" else plain_stager()
    ws = sc.waveforms([8] * (stage.kRing + 2), sc.L, 41, np.int16)
    warm = sc.waveforms([8] * stage.kRing, sc.L, 42, np.int16)
    if late == "compute":
        for w in warm:                                  # buffers allocated: the host then queues the batches well inside one lag
            stage.to_device(stage.to_pinned(w))
        torch.cuda.synchronize()
        torch.cuda._sleep(lag)
    outs = [stage.to_device(stage.to_pinned(w)).clone() for w in ws]
    torch.cuda.synchronize()
    for i, (o, w) in enumerate(zip(outs, ws)):
        assert np.array_equal(o.cpu().numpy(), sc.widen(w)), "batch %d" % i
    stage.close()


@pytest.mark.parametrize("late", ["read", "write"])
def test_fresh_int16_buffer_waits_for_its_block(lag, late):
    """a fresh dev16 buffer comes from the caching allocator in the CALLER's stream order, and its first use is the
    copy on the copy stream.  Made deterministic: a victim of exactly the buffer's size is allocated on the compute stream and
    released while a kernel that reads it (late = read: a clone behind the sleep) or writes it (late = write: a fill behind the
    sleep) is still queued; the stager's allocation then gets the same block, and its copy must wait for that kernel.
    The reuse is made dependable with torch.cuda.empty_cache() before the victim is made: the victim is then carved from the
    front of the best-fitting free block, and when it is released that block (or, with the clone allocated behind it, a free block
    of exactly the victim's size) is again the best fit for the request of the same size that follows.  A run in which the
    allocator gave another block fails, saying so."""
    stage = plain_stager()
    w = sc.waveforms([8], sc.L, 51, np.int16)[0]
    staged = stage.to_pinned(w)
    slot = staged[1]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    victim = torch.full((w.size,), 7, dtype=torch.int16, device=DEV)
    ptr = victim.data_ptr()
    torch.cuda._sleep(lag)
    keep = victim.clone() if late == "read" else None
    if late == "write":
        victim.fill_(9)
    del victim
    out = stage.to_device(staged)
    assert stage.dev16[slot].data_ptr() == ptr, "the allocator gave dev16 another block than the victim's: hazard not set up"
    got = out.cpu().numpy()
    torch.cuda.synchronize()
    if keep is not None:
        assert bool((keep == 7).all()), "the copy overwrote a block that a queued kernel had yet to read"
    assert np.array_equal(got, sc.widen(w)), "the staged batch was overwritten by a kernel queued before the block was handed out"
    stage.close()


def test_fresh_float32_buffer_is_safe_by_stream_order(lag):
    """The same set-up for a fresh dev32: the victim's block becomes the float32 buffer while a clone of the victim is still
    queued behind the sleep.
    Why this needs no wait: dev32 is allocated on the compute stream and every use of it is on the compute stream -- first written
    by the widening kernel, then read by the model -- so whatever was queued on the block before the allocator handed it out runs
    before the first write, by stream order alone.  (The model's side streams fork from and join the compute stream inside each
    forward.)  The test passes with and without the dev16 fix; it is here so that a change that moves dev32's first use to another
    stream meets the hazard.  dev16[slot] is put in place beforehand so that dev32 is the first allocation behind the release."""
    stage = plain_stager()
    w = sc.waveforms([8], sc.L, 52, np.int16)[0]
    staged = stage.to_pinned(w)
    stage.dev16[staged[1]] = torch.empty(w.size, dtype=torch.int16, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    victim = torch.full((w.size,), 7.0, dtype=torch.float32, device=DEV)
    ptr = victim.data_ptr()
    torch.cuda._sleep(lag)
    keep = victim.clone()
    del victim
    out = stage.to_device(staged)
    assert stage.dev32[0].data_ptr() == ptr, "the allocator gave dev32 another block than the victim's: hazard not set up"
    got = out.cpu().numpy()
    torch.cuda.synchronize()
    assert bool((keep == 7).all())
    assert np.array_equal(got, sc.widen(w))
    stage.close()


def test_sweep_that_raises_in_mid_flight(lag, clean_cache):
    """The model raises at its third batch while the compute stream runs a lag behind: forward() hands the stager back, drained
    (nothing queued on the compute or the copy stream), and the next sweep on it is exact."""
    stage = seed_stager(plain_stager())
    with pytest.raises(RuntimeError, match="fails as asked"):
        ev.forward(sc.EchoModel(gpu_lag=lag, fail_at=3).to(DEV), sc.batches(sc.SIZES, sc.L, 61, np.int16), return_target=True)
    assert torch.cuda.current_stream(DEV).query() and stage.copy_stream.query()
    assert ev._STAGERS.get(KEY) is stage
    out = ev.forward(sc.EchoModel(gpu_lag=lag).to(DEV), sc.batches(sc.SIZES, sc.L, 62, np.int16), return_target=True)
    sc.assert_exact(out, sc.expected(sc.SIZES, sc.L, 62, np.int16))
    assert ev._STAGERS.get(KEY) is stage
