"""Cases and helpers of the live-stream tests, importable without a GPU: tests/test_stream_cpu.py holds the sizes that
acx_stream_geometry derives (adv, C, Ch, Hw; csrc/stream.hip str_sizes) to brute force over these geometries, and
tests/test_gpu_stream_geometry.py runs the same geometries on the device with the stream state poisoned.

Everything "expected" here comes from a definition, never from stream.hip's own arithmetic: the band tables of
_ffi.resample_taps / resample_geometry (final_table), windows.window_starts / timeline_steps, and a plain restatement of "the
windows that cover a midpoint" (cover).  Sim replays the host bookkeeping of a handle call by call -- what pytorch/stream.py and
acx_stream_push / _forward / _timeline do with positions and counts -- from those definitions and stream.schedule(), so that a
test can say which appends wrap, which windows read across the ring's mirror, which forward call a window was part of and
which rows' covers wrap the probability history."""
import functools
import random

import numpy as np
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import stream as stm
from audioset_convnext_inf_amd.pytorch import windows as win

SR = 32000
KEY = {"logits": "clipwise_logits", "scene": "scene", "frame": "frame"}

# ---- the geometries (samples at 32 kHz) ---------------------------------------------------------------------------------------
# name -> W, H, max_push values, recordings (slot i = recording i).  What each is for:
#   A  max_batch = 256: over 128 windows per forward (the second kStrTable launch) and over 256 pending after one push; about
#      254 windows under every row; H odd, no divisor of W or of the frame hop 320
#   B  odd W and H; max_push < H: pushes that emit nothing; a single-window short clip (W - 1) in the same handle
#   C  H = W, max_push > 3 W, Hw at its minimum
#   D  H = W - 1: the cover of a row switches between one and two windows
#   E  H = the frame hop; a handle whose every push is one sample (the smallest C)
#   R  the geometry of the other input rates
#   T  the geometry every earlier stream test runs (10 s every 1 s); CPU sweep only
# Recordings other than the issue's table (A 3W + 11, C 4W + 1 and 7W, D 3W + 5, E 2W + 161): at those lengths no recording
# has more than Hw windows (A 509 of 568, C 7 of 8, D 4 of 6, E 32 of 34), so no row's cover wraps the probability history.
# C and D have one window under every row but the last, whose cover is the last regular window and the end-aligned one: 8W + 1
# (windows 7, 8 at Hw = 8) and 6W + 5 (windows 5, 6 at Hw = 6) put that pair across the wrap.  check_reach holds every length.
GEOMETRIES = {
    "A": dict(W=_ffi.MIN_SAMPLES, H=29, max_push=(9000,), recs=(4 * 7360 + 11, 7360 + 1)),
    "B": dict(W=48001, H=7001, max_push=(5000,), recs=(5 * 48001 + 3, 48001, 48001 - 1)),
    "C": dict(W=32000, H=32000, max_push=(100000,), recs=(4 * 32000 + 1, 8 * 32000 + 1)),
    "D": dict(W=64000, H=63999, max_push=(64000,), recs=(6 * 64000 + 5,)),
    "E": dict(W=9600, H=320, max_push=(1, 700), recs=(3 * 9600 + 161,)),
    "R": dict(W=16000, H=5000, max_push=(), recs=()),
    "T": dict(W=320000, H=32000, max_push=(64000, 128000), recs=()),
}
# rate -> max_push (input samples), recordings (input samples) at geometry R.  44101 Hz: Ch and adv are dominated by of = 44101
# whatever max_push is (C = 114240, Ch = 91328, Hw = 26 at max_push 3000), so its recordings are as long as it takes to wrap
# all three: 29 and 18 windows.  At the issue's max_push of 50000 (C = 148288, Ch = 138304, Hw = 33) that would be 40 windows.
RATE_CASES = {
    8000: dict(max_push=37, recs=(4 * 4000 + 3, 3 * 4000 + 1251)),
    11025: dict(max_push=3000, recs=(5 * 5513 + 7, 3 * 5513)),
    96000: dict(max_push=1, recs=(48000 + 601,), lead=48000),
    44101: dict(max_push=3000, recs=(215003, 130000)),
    44100: dict(max_push=441, recs=(4 * 22050 + 11, 3 * 22050)),
}
RATES = (32000, 8000, 11025, 16000, 44100, 48000, 96000, 44101)
# The resampler's per_thread = 2 tile form (of / nf = 24: tests/resample_cases.py) under a live stream: 768 kHz, the API's
# maximum, windows of 0.5 s every 0.25 s, odd push sizes.  Kept beside RATE_CASES and out of RATES: the CPU sweeps over RATES
# build a table of every pushed count, which at 24 input samples per output would multiply their runtime; form_sim holds this
# case's ring, input history, guard and covers at every call instead (tests/test_stream_cpu.py).
FORM_CASE = dict(rate=768000, W=16000, H=8000, max_push=49999, recs=(7 * 384000 + 4801, 3 * 384000 + 77))


def sweep_max_push(W, H, rate):
    """The sweep's max_push values in input samples: 1, one below H, one between H and W, one above W (as far as H and W
    leave room), each from its 32 kHz value."""
    at32 = {1, max(1, H // 2), (H + W) // 2, W + W // 3 + 5}
    return sorted({max(1, v * rate // SR) for v in at32})


# ---- expected sides, from the definitions ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bands(rate):
    """(of, nf, width, start[nf], count[nf]) of rate -> 32 kHz as int64 arrays."""
    of, nf, width, _ = _ffi.resample_geometry(rate, SR)
    start, count, _ = _ffi.resample_taps(rate, SR)
    return of, nf, width, np.array(start, dtype=np.int64), np.array(count, dtype=np.int64)


def final_table(rate, L):
    """need[n] = input samples output n needs pushed (itself and every earlier output), n < ceil(nf L / of); brute force
    over the band tables."""
    if rate == SR:
        return np.arange(1, L + 1, dtype=np.int64)
    of, nf, width, start, count = bands(rate)
    N = (nf * L + of - 1) // of
    n = np.arange(N, dtype=np.int64)
    j, i = n // nf, n % nf
    last = j * of + start[i] - width + count[i] - 1
    last[count[i] == 0] = -1
    return np.maximum.accumulate(last + 1)


def oldest_table(rate, L):
    """oldest[n] = the oldest input sample any output n' >= n reads (n' < ceil(nf L / of)): j of + start[i] - width of the
    band tables, as a suffix minimum.  May be negative: the zeros in front of the recording."""
    of, nf, width, start, count = bands(rate)
    N = (nf * L + of - 1) // of
    n = np.arange(N, dtype=np.int64)
    first = (n // nf) * of + start[n % nf] - width
    return np.minimum.accumulate(first[::-1])[::-1]


def closed_length(rate, P):
    if rate == SR:
        return P
    of, nf = bands(rate)[:2]
    return (nf * P + of - 1) // of


_NEED = {}


def final_open(rate, P):
    """R: the final 32 kHz samples of an open recording of P input samples, from final_table (grown on demand)"""
    if rate == SR:
        return P
    t = _NEED.get(rate)
    if t is None or t[0] < P:
        L = max(2 * P, 1 << 16)
        t = _NEED[rate] = (L, final_table(rate, L))
    return int(np.searchsorted(t[1], P, side="right"))


def schedule_def(W, H, rate, P, closed):
    """(R, windows, rows) of include/acx.h's schedule, restated: what stream.schedule() is held to by test_stream_cpu.py"""
    if closed:
        R = closed_length(rate, P)
        if R < _ffi.MIN_SAMPLES:
            return R, 0, 0
        return R, win.window_count(R, W, H), (R + H - 1) // H
    R = final_open(rate, P)
    x = R - W - H // 2
    return R, ((R - W) // H + 1 if R >= W else 0), ((x + H - 1) // H if x > 0 else 0)


def open_windows(R, W, H):
    """windows j H + W <= R"""
    return np.where(R >= W, (R - W) // H + 1, 0)


def start_of(j, L, W, H):
    """window j of a recording of L samples (L = None: still open), windows.window_starts' definition for one j"""
    return j * H if L is None else min(j * H, max(0, L - W))


def cover(m, starts, W):
    """[j0, j1): the windows with s_j <= m < s_j + W.  starts ascends, so they are the run from the first window that ends
    behind m to the last that starts at or before it."""
    starts = np.asarray(starts, dtype=np.int64)
    j0 = int(np.searchsorted(starts + W, m, side="right"))
    j1 = int(np.searchsorted(starts, m, side="right"))
    assert j0 < j1 and all(s <= m < s + W for s in (starts[j0], starts[j1 - 1]))
    assert (j0 == 0 or starts[j0 - 1] + W <= m) and (j1 == len(starts) or starts[j1] > m)
    return j0, j1


# ---- the host bookkeeping of one handle, replayed ------------------------------------------------------------------------------------
class Sim:
    """One handle: push(chunks) / close() mirror Stream.push / Stream.close call by call and record
      appends   (slot, pos, len, wide)      each launch entry of stream_append_kernel: the float4 path or the scalar one
      forwards  [(slot, j, start, len)]     the windows of each acx_stream_forward call, in order
      rows      (slot, k, j0, j1, newest)   each timeline row with its cover and the newest window stashed when it is reduced
    and check, at every step, what the sizes have to guarantee (the assertion messages name the geometry)."""

    def __init__(self, W, H, rate, max_push, timeline=True, max_batch=64, name=""):
        self.W, self.H, self.rate, self.max_push, self.timeline, self.max_batch = W, H, rate, max_push, timeline, max_batch
        self.adv, self.C, self.Ch, self.Hw = stm.geometry(W, H, rate, max_push, timeline)
        self.cap = self.C if rate == SR else self.Ch
        self.tag = "%s W=%d H=%d rate=%d max_push=%d (adv=%d C=%d Ch=%d Hw=%d)" % (
            name, W, H, rate, max_push, self.adv, self.C, self.Ch, self.Hw)
        self.slots = {}
        self.hist = {}
        self.appends, self.forwards, self.rows = [], [], []

    def _slot(self, s):
        return self.slots.setdefault(s, dict(inp=0, out=0, closed=False, win_done=0, row_done=0))

    def push(self, chunks):
        """chunks: {slot: (samples, element offset of the chunk in its recording's 16-byte aligned storage)}"""
        mp = self.max_push
        pieces = []
        for s in sorted(chunks):
            n, off = chunks[s]
            pieces.append((s, [(min(mp, n - i), off + i) for i in range(0, n, mp)] or [(0, off)]))
        for r in range(max(len(p) for _, p in pieces)):
            ent = [(s, p[r]) for s, p in pieces if r < len(p)]
            assert len(ent) <= _ffi.MAX_VARLEN_CLIPS
            parts = [e for e in ent if e[1][0]]
            src = 0
            for s, (n, off) in ent:
                x = self._slot(s)
                if x["closed"]:
                    x.update(inp=0, out=0, closed=False, win_done=0, row_done=0)
                    self.hist.pop(s, None)
                if n:
                    at = off if len(parts) == 1 else src       # one part: the chunk itself; more: a fresh concatenation
                    p0 = x["inp"] % self.cap
                    self.appends.append((s, x["inp"], n, ((p0 | self.cap) & 3) == 0 and at % 4 == 0))
                src += n
                x["inp"] += n
                new = schedule_def(self.W, self.H, self.rate, x["inp"], False)[0]
                assert new - x["out"] <= self.C - self.W, "%s: a push advances by %d, more than the ring holds" % (
                    self.tag, new - x["out"])
                self._history(x, new)
                x["out"] = new
            self._drain()

    def close(self, slots=None):
        for s in sorted(self.slots if slots is None else slots):
            x = self._slot(s)
            assert not x["closed"]
            new = schedule_def(self.W, self.H, self.rate, x["inp"], True)[0]
            assert new - x["out"] <= self.C - self.W, "%s: a close advances by %d, more than the ring holds" % (
                self.tag, new - x["out"])
            self._history(x, new)
            x["out"], x["closed"] = new, True
        self._drain()

    def _history(self, x, new):
        """the oldest input the outputs x["out"] .. new - 1 read (band tables) is still in the input history, and the launcher's
        guard lets the call through"""
        if self.rate == SR or new <= x["out"]:
            return
        of, nf, width, start, _ = bands(self.rate)
        n = x["out"]
        oldest = (n // nf) * of + int(start[n % nf]) - width
        assert max(oldest, 0) >= x["inp"] - self.Ch, "%s: output %d reads input %d, overwritten at %d pushed" % (
            self.tag, n, oldest, x["inp"])
        assert n * of // nf - width - 1 >= x["inp"] - self.Ch, "%s: the history guard refuses a legal call" % self.tag

    def _counts(self, x):
        _, nw, nr = schedule_def(self.W, self.H, self.rate, x["inp"], x["closed"])
        return nw, (nr if self.timeline else 0)

    def _drain(self):
        while True:
            call, length = [], None
            for s in sorted(self.slots):
                x = self.slots[s]
                nw, _ = self._counts(x)
                if x["win_done"] >= nw:
                    continue
                ln = x["out"] if x["closed"] and x["out"] < self.W else self.W
                if call and ln != length:
                    break
                length = ln
                L = x["out"] if x["closed"] else None
                for j in range(x["win_done"], min(nw, x["win_done"] + self.max_batch - len(call))):
                    start = start_of(j, L, self.W, self.H)
                    assert start >= x["out"] - self.C and start + ln <= x["out"], "%s: window %d at %d is not in the ring" % (
                        self.tag, j, start)
                    call.append((s, j, start, ln))
                if len(call) == self.max_batch:
                    break
            if not call:
                break
            self.forwards.append(call)
            for s, j, _, _ in call:
                self.slots[s]["win_done"] = j + 1
                if self.timeline:
                    self.hist.setdefault(s, np.full(self.Hw, -1, dtype=np.int64))[j % self.Hw] = j
        if not self.timeline:
            return
        for s in sorted(self.slots):
            x = self.slots[s]
            nw, nr = self._counts(x)
            if nr <= x["row_done"]:
                continue
            L = x["out"] if x["closed"] else None
            starts = np.array([start_of(j, L, self.W, self.H) for j in range(nw)], dtype=np.int64)
            for k in range(x["row_done"], nr):
                m = k * self.H + self.H // 2 if L is None else min(k * self.H + self.H // 2, L - 1)
                j0, j1 = cover(m, starts, self.W)
                js = np.arange(j0, j1)
                assert nw - 1 - j0 < self.Hw, "%s: row %d covers windows from %d, the newest stashed is %d" % (self.tag, k, j0, nw - 1)
                assert np.array_equal(self.hist[s][js % self.Hw], js), "%s: row %d: a window of its cover %d..%d is overwritten" % (
                    self.tag, k, j0, j1 - 1)
                self.rows.append((s, k, j0, j1, nw - 1))
            x["row_done"] = nr

    # what a case is there for
    def reach(self):
        C, cap, Hw = self.C, self.cap, self.Hw
        return dict(
            mirror=sum(1 for call in self.forwards for _, _, st, ln in call if st % C + ln > C),
            wrap=sum(1 for _, p, n, _ in self.appends if p % cap + n > cap),
            wide=sum(1 for a in self.appends if a[3]),
            scalar=sum(1 for a in self.appends if not a[3]),
            cover_wrap=sum(1 for _, _, j0, j1, _ in self.rows if j0 % Hw > (j1 - 1) % Hw) if self.timeline else 0,
            count=max((len(c) for c in self.forwards), default=0))


# ---- chunkings ----------------------------------------------------------------------------------------------------------------------
def chunk_sizes(L, rng, max_push):
    """Seeded random chunking: empty and one-sample chunks, primes, ordinary sizes and chunks longer than max_push."""
    out, pos = [], 0
    while pos < L:
        c = rng.choice([0, 1, 7, 4099, 31991, 65537, rng.randrange(1, 3 * max_push), 2 * max_push + 13])
        c = min(c, L - pos)
        out.append(c)
        pos += c
    return out


def scaled_chunk_sizes(L, rng, max_push):
    """chunk_sizes with its fixed sizes scaled to max_push (they were chosen for max_push = 64000): empty and one-sample chunks,
    small odd ones, a size below max_push, max_push itself, and chunks longer than max_push, which the wrapper splits."""
    out, pos = [], 0
    while pos < L:
        c = rng.choice([0, 1, 7, max(1, max_push // 15 + 1), max_push // 2 + 1, max_push, rng.randrange(1, 3 * max_push + 1),
                        2 * max_push + 13])
        c = min(c, L - pos)
        out.append(c)
        pos += c
    return out


def even_chunks(L, c):
    return [c] * (L // c) + ([L % c] if L % c else [])


def steps_of(plans):
    """per-slot chunk lists -> the calls: [{slot: (samples, offset in the recording)}], all slots interleaved as run_stream does"""
    offs = [0] * len(plans)
    calls = []
    for step in range(max(len(p) for p in plans)):
        call = {}
        for i, p in enumerate(plans):
            if step < len(p):
                call[i] = (p[step], offs[i])
                offs[i] += p[step]
        calls.append(call)
    return calls


def simulate(sim, plans, slots=None):
    """one recording per slot through sim: the calls of steps_of(plans), then one close"""
    for call in steps_of(plans):
        sim.push({(i if slots is None else slots[i]): v for i, v in call.items()})
    sim.close(None if slots is None else slots)
    return sim


# ---- GPU helpers (moved from tests/test_gpu_stream.py; check_equal takes W and H) -------------------------------------------------
def run_stream(st, recs, rng, max_push, close=True, lead=()):
    """Push every recording (slot i = recording i) in random chunks, all slots interleaved, then close; returns the calls'
    dicts.  lead: chunk sizes per slot of the first calls, ahead of the random ones."""
    heads = [[step[i] for step in lead] for i in range(len(recs))]
    plans = [h + chunk_sizes(r.numel() - sum(h), rng, max_push) for h, r in zip(heads, recs)]
    offs = [0] * len(recs)
    results = []
    for step in range(max(len(p) for p in plans)):
        chunks = {}
        for i, p in enumerate(plans):
            if step < len(p):
                chunks[i] = recs[i][offs[i]:offs[i] + p[step]]
                offs[i] += p[step]
        results.append(st.push(chunks))
    if close:
        results.append(st.close())
    return results


def run_plans(st, recs, plans, slots=None):
    """run_stream with the chunk lists given (the ones Sim was fed): the calls' dicts, the close last"""
    results = []
    for call in steps_of(plans):
        results.append(st.push({(i if slots is None else slots[i]): recs[i][off:off + n] for i, (n, off) in call.items()}))
    results.append(st.close(slots))
    return results


def gather(results, slot, what, timeline):
    starts, rows, probs, tl, steps = [], [], [], [], []
    for d in results:
        m = (d["slot"] == slot).nonzero().flatten().tolist()
        starts += d["starts"][m].tolist()
        key = KEY[what]
        if isinstance(d[key], list):
            rows += [d[key][i] for i in m]
        else:
            rows += list(d[key][m])
        if what == "logits":
            probs += list(d["clipwise_output"][m])
            if timeline:
                t = (d["timeline_slot"] == slot).nonzero().flatten().tolist()
                steps += d["timeline_step"][t].tolist()
                tl += list(d["timeline"][t])
    return starts, rows, probs, tl, steps


def check_equal(model, recs, results, W, H, what="logits", timeline="mean", rate=None, slots=None):
    for i, rec in enumerate(recs):
        s = i if slots is None else slots[i]
        ref = model.forward_windows(rec, window=W / SR, hop=H / SR, what=what, sample_rate=rate, timeline=timeline)
        starts, rows, probs, tl, steps = gather(results, s, what, timeline)
        assert torch.equal(torch.tensor(starts, dtype=torch.float64), ref["starts"]), (i, starts[:4], ref["starts"][:4])
        assert torch.equal(torch.stack(rows), ref[KEY[what]]), i
        if what == "logits":
            assert torch.equal(torch.stack(probs), ref["clipwise_output"]), i
            if timeline:
                assert steps == list(range(ref["timeline"].shape[0])), i
                assert torch.equal(torch.stack(tl), ref["timeline"]), i


# ---- the GPU cases: their chunk lists, and what each has to reach ---------------------------------------------------------------------
def case_plans(name, max_push, even):
    """the chunk lists of geometry `name` (one recording per slot): all max_push, or the seeded mix scaled to max_push"""
    recs = GEOMETRIES[name]["recs"]
    if even:
        return [even_chunks(L, max_push) for L in recs]
    rng = random.Random(sum(map(ord, name)) * 1000 + max_push)
    return [scaled_chunk_sizes(L, rng, max_push) for L in recs]


def case_batch(name):
    return 256 if name == "A" else 64


def check_reach(sim, even=False, timeline=True, one_sample=False, many=False):
    """What a case is there for.  Exceptions, each where the edge is impossible: a one-sample append cannot wrap, nor can
    chunks of exactly max_push when they tile the ring (D: max_push = C / 2), and such chunks stay on one append path when
    max_push is a multiple of four -- the seeded mix of the same case has to show all of these."""
    r = sim.reach()
    assert r["mirror"] >= 1, (sim.tag, r)
    assert r["wrap"] >= 1 or one_sample or (even and sim.cap % sim.max_push == 0), (sim.tag, r)
    assert (r["wide"] >= 1 and r["scalar"] >= 1) if not even else r["wide"] + r["scalar"] >= 1, (sim.tag, r)
    assert not timeline or r["cover_wrap"] >= 1, (sim.tag, r)
    assert not many or r["count"] > 128, (sim.tag, r)
    return sim


def case_sim(name, max_push, even, timeline=True):
    g = GEOMETRIES[name]
    sim = simulate(Sim(g["W"], g["H"], SR, max_push, timeline, case_batch(name), name), case_plans(name, max_push, even))
    return check_reach(sim, even, timeline, max_push == 1, name == "A")


def rate_plans(rate):
    """the chunk lists of a rate case: the seeded mix; at 96 kHz the lead-in as one chunk, which the wrapper splits into
    one-sample pushes like everything else (a second handle could not hand its slot's state over)"""
    case = RATE_CASES[rate]
    rng = random.Random(rate)
    lead = case.get("lead", 0)
    return [([lead] if lead else []) + scaled_chunk_sizes(L - lead, rng, case["max_push"]) for L in case["recs"]]


def form_plans():
    """the chunk lists of FORM_CASE: the seeded mix scaled to its odd max_push"""
    rng = random.Random(FORM_CASE["rate"])
    return [scaled_chunk_sizes(L, rng, FORM_CASE["max_push"]) for L in FORM_CASE["recs"]]


def form_sim():
    """FORM_CASE through Sim: the ring's mirror, a wrapped append, both append paths and a wrapped cover are all reached"""
    c = FORM_CASE
    return check_reach(simulate(Sim(c["W"], c["H"], c["rate"], c["max_push"], True, 64, "form"), form_plans()))


def rate_sim(rate):
    """At 96 kHz (max_push = 1) no append can wrap, and a wrapped cover would take more than Hw = 7 windows, over 150000
    one-sample calls: the recording is about one window, as the case is defined, and reaches the ring's mirror only."""
    g, case = GEOMETRIES["R"], RATE_CASES[rate]
    sim = simulate(Sim(g["W"], g["H"], rate, case["max_push"], True, 64, "R"), rate_plans(rate))
    return check_reach(sim, timeline=case["max_push"] > 1, one_sample=case["max_push"] == 1)
