"""Live streams (ConvNeXt.stream, acx_stream_* in include/acx.h): recordings that arrive chunk by chunk, tagged window by window
as soon as a window is complete.

A handle has `slots`; each holds one recording at a time.  push() appends chunks to the slots' open recordings; close() ends
recordings, and a slot's next push starts a new one.  Whatever a recording emits over all its pushes and its close equals
ConvNeXt.forward_windows of the whole recording -- window starts, per-window outputs in the same order, timeline rows -- bit
for bit, for any chunking.  When things are emitted is the schedule of include/acx.h (schedule() below gives it for one slot):
window j once its last sample is final; timeline row k once no window still to come can cover its midpoint, which trails the
newest window by about one window length; the rest at close.  A recording shorter than the model's minimum emits nothing and is
listed under "short" instead of raising, so one short stream does not cost the results of the others.

With events= the handle also says what started and stopped when: the rows it emits -- one per window, or the timeline rows --
go through an online event decoder (pytorch/segments.py EventStream, acx_event_stream_*) that carries its state across calls
and hands out each event once, as soon as nothing still to come can change it; over a recording's calls the events are those
of decode_events_gpu over forward_windows' rows of the whole recording, byte for byte."""
import ctypes

import torch

from .. import _ffi
from . import resample as _rs
from . import segments as _seg
from . import windows as _win


def schedule(window, hop, sample_rate, pushed, closed):
    """(final 32 kHz samples, windows, timeline rows) emitted so far by one slot after `pushed` input samples at sample_rate,
    the recording open or closed.  Window / hop in samples at 32 kHz.  Host only (acx_stream_schedule)."""
    rate = _rs.MODEL_RATE if sample_rate is None else _rs.check_rate(sample_rate)
    return _ffi.stream_schedule(window, hop, rate, pushed, closed)


def geometry(window, hop, sample_rate, max_push, timeline=True):
    """(adv, C, Ch, Hw) of one slot of a handle with these arguments: the largest 32 kHz advance of one call, the samples of the
    ring and of the input history, the windows of the probability history.  Window / hop in samples at 32 kHz, max_push in
    input samples.  Host only (acx_stream_geometry)."""
    rate = _rs.MODEL_RATE if sample_rate is None else _rs.check_rate(sample_rate)
    return _ffi.stream_geometry(window, hop, rate, max_push, bool(timeline))


class Stream:
    """One acx_stream handle on the model's device (see ConvNeXt.stream).  Clip-level outputs per window only: the segment-wise /
    frame-wise outputs of ConvNeXt.forward_segments are not part of live streams (run forward_windows(what="segment") on the
    finished recording).  events=dict(threshold=..., low=..., median=..., min_duration=..., merge_gap=...) decodes events
    live from the clip-level rows, one step per hop: event_source="windows" takes row j from window j's "clipwise_output"
    (detection lags the audio by one window plus median // 2 hops plus merge_gap), "timeline" takes the handle's timeline
    rows (and inherits their trail)."""

    def __init__(self, model, slots=256, window=10.0, hop=1.0, what="logits", sample_rate=None, timeline="mean", max_push=2.0,
                 max_batch=64, events=None, event_source="windows"):
        if what not in _ffi.MODES:
            raise ValueError("what must be 'logits', 'scene' or 'frame' (got %r)" % (what,))
        if timeline not in ("mean", "max", None):
            raise ValueError("timeline must be 'mean', 'max' or None (got %r)" % (timeline,))
        if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= (1 << 20):
            raise ValueError("slots must be an integer in [1, 2^20] (got %r)" % (slots,))
        if isinstance(max_batch, bool) or not isinstance(max_batch, int) or not 1 <= max_batch <= _ffi.MAX_VARLEN_CLIPS:
            raise ValueError("max_batch must be an integer in [1, %d] (got %r)" % (_ffi.MAX_VARLEN_CLIPS, max_batch))
        self.window = _win.seconds_to_samples(window, "window")
        self.hop = self.window if hop is None else _win.seconds_to_samples(hop, "hop")
        _win.check_window(self.window, self.hop)
        self.rate = _rs.MODEL_RATE if sample_rate is None else _rs.check_rate(sample_rate)
        self.max_push = _win.seconds_to_samples(max_push, "max_push", self.rate)
        if self.max_push < 1:
            raise ValueError("max_push must be positive (got %r)" % (max_push,))
        self.slots, self.what, self.max_batch = slots, what, max_batch
        self.timeline = timeline if what == "logits" else None
        self.model = model
        self.device = model.head_audioset.weight.device
        model._check_run(self.device)
        self._h = None
        with torch.cuda.device(self.device):
            ctx = model.native_context(self.device)
            h = ctypes.c_void_p()
            _ffi.check(_ffi.lib().acx_stream_create(ctx.handle, slots, self.window, self.hop, self.rate, self.max_push,
                                                    1 if self.timeline else 0, ctypes.byref(h)))
        self._h = h
        self.classes = ctx.classes  # N of the model's head at create: the handle's rows are this wide
        self._pushed = {}           # slot -> input samples of its open recording
        self._last = None           # the torch stream of the previous call
        self._ev = None             # the online event decoder over the rows this handle emits
        if events is not None:
            if what != "logits":
                raise ValueError("events= needs what='logits' (got %r)" % (what,))
            if event_source not in ("windows", "timeline"):
                raise ValueError("event_source must be 'windows' or 'timeline' (got %r)" % (event_source,))
            if event_source == "timeline" and not self.timeline:
                raise ValueError("event_source='timeline' needs a timeline (got timeline=None)")
            extra = set(events) - {"threshold", "low", "median", "min_duration", "merge_gap"}
            if extra:
                raise TypeError("events= takes decode_events' threshold, low, median, min_duration and merge_gap (got %s)"
                                % sorted(extra))
            self.event_source = event_source
            self._ev = _seg.EventStream(slots, self.classes, step=self.hop / _rs.MODEL_RATE, device=self.device, **events)

    def close_handle(self):
        if self._h is not None and self._h.value:
            _ffi.lib().acx_stream_destroy(self._h)
        self._h = None

    def poison(self, slot=-1):
        """Test support (acx_test_stream_poison): fill the device state of `slot` (-1: every slot) with 0xFF bytes."""
        with torch.cuda.device(self.device):
            _ffi.check(_ffi.lib().acx_test_stream_poison(self._h, int(slot), _ffi.stream_ptr(self.device)))

    def __del__(self):
        try:
            self.close_handle()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------- calls
    def push(self, chunks):
        """chunks: a list of `slots` 1-D CUDA tensors or None, or {slot: tensor}.  Returns what this call emits (result())."""
        entries = self._entries(chunks)
        out = _Result(self)
        self._enter()
        pieces = []
        for s, t in entries:
            n = t.numel()
            pieces.append((s, [t[i:i + self.max_push] for i in range(0, n, self.max_push)] or [t]))
        rounds = max((len(p) for _, p in pieces), default=0)
        for r in range(rounds):
            ent = [(s, p[r]) for s, p in pieces if r < len(p)]
            for b0 in range(0, len(ent), _ffi.MAX_VARLEN_CLIPS):
                batch = ent[b0:b0 + _ffi.MAX_VARLEN_CLIPS]
                lens = [int(t.numel()) for _, t in batch]
                parts = [t for _, t in batch if t.numel()]
                packed = None
                if parts:
                    packed = parts[0] if len(parts) == 1 else torch.cat(parts)
                    packed = packed.to(torch.float32).contiguous()
                slot = (ctypes.c_int * len(batch))(*[s for s, _ in batch])
                ln = (ctypes.c_int64 * len(batch))(*lens)
                with torch.cuda.device(self.device):
                    _ffi.check(_ffi.lib().acx_stream_push(self._h, _ffi.ptr(packed), slot, ln, len(batch),
                                                          _ffi.stream_ptr(self.device)))
                for (s, _), n in zip(batch, lens):
                    self._pushed[s] = self._pushed.get(s, 0) + n
                self._drain(out)
        d = out.result()
        if self._ev is not None:
            touched = [s for s, _ in entries]
            d["events"] = self._decode(d, touched)
            d["events_open"] = self._ev.open_begin(touched)
        return d

    def close(self, slots=None):
        """End the recordings of `slots` (default: every slot pushed to since its last close); emits what the ends make final.
        A slot never pushed to closes an empty recording, which is short."""
        if slots is None:
            slots = sorted(self._pushed)
        else:
            slots = sorted(self._slot(s) for s in slots)
            if len(set(slots)) != len(slots):
                raise ValueError("a slot is listed twice")
        out = _Result(self)
        self._enter()
        seconds = {s: self._pushed.get(s, 0) / self.rate for s in slots}       # of the original audio
        for b0 in range(0, len(slots), _ffi.MAX_VARLEN_CLIPS):
            batch = slots[b0:b0 + _ffi.MAX_VARLEN_CLIPS]
            arr = (ctypes.c_int * len(batch))(*batch)
            with torch.cuda.device(self.device):
                _ffi.check(_ffi.lib().acx_stream_close(self._h, arr, len(batch), _ffi.stream_ptr(self.device)))
            for s in batch:
                L = _rs.resampled_length(self._pushed.pop(s, 0), self.rate)
                if L < _ffi.MIN_SAMPLES:
                    out.short.append(s)
            self._drain(out)
        d = out.result()
        if self._ev is not None:
            # the rows the ends made final, then the recordings' ends: the timeline's last boundary is the end of the audio,
            # the windows' the last hop's (a short recording closes an empty event recording)
            last = self._decode(d, slots).check()
            ends = seconds if self.event_source == "timeline" else None
            d["events"] = _seg.join_event_tables([last, self._ev.close(slots, ends)])
            d["events_open"] = self._ev.open_begin(slots)
        return d

    # ------------------------------------------------------------------------------------------------------------- helpers
    def _slot(self, s):
        if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.slots:
            raise ValueError("slot %r out of range (the stream has %d slots)" % (s, self.slots))
        return s

    def _entries(self, chunks):
        if isinstance(chunks, dict):
            items = [(self._slot(s), t) for s, t in chunks.items()]
        else:
            chunks = list(chunks)
            if len(chunks) != self.slots:
                raise ValueError("expected a list of %d chunks (one per slot, None to skip), got %d" % (self.slots, len(chunks)))
            items = list(enumerate(chunks))
        out = []
        for s, t in sorted(items, key=lambda e: e[0]):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dim() != 1:
                raise ValueError("expected 1-D waveform tensors, got %r" % (getattr(t, "shape", type(t)),))
            if not t.is_floating_point():
                raise ValueError("expected float waveform tensors, got %s" % (t.dtype,))
            if t.device != self.device:
                raise RuntimeError("chunk for slot %d on %s but the model is on %s" % (s, t.device, self.device))
            out.append((s, t.detach()))
        return out

    def _decode(self, d, touched):
        """The event table of one call's rows: d's window rows or timeline rows, which lie in (slot, step) order; the slots
        touched without a row push zero rows."""
        rows, of = (d["clipwise_output"], d["slot"]) if self.event_source == "windows" else (d["timeline"], d["timeline_slot"])
        count = {s: 0 for s in touched}
        for s in of.tolist():
            count[s] = count.get(s, 0) + 1
        slots = sorted(count)
        if not slots:
            return self._ev.close([])
        return self._ev.push(rows, slots=slots, steps=[count[s] for s in slots])

    def _enter(self):
        """All work of the handle runs in order: a new current stream first waits for the previous one (no synchronisation)."""
        self.model._check_run(self.device)
        cur = torch.cuda.current_stream(self.device)
        if self._last is not None and self._last != cur:
            ev = torch.cuda.Event()
            ev.record(self._last)
            cur.wait_event(ev)
        self._last = cur

    def _drain(self, out):
        """Forward every pending window (max_batch at a time), then fetch the timeline rows that became final."""
        lib, dev, mode, mb = _ffi.lib(), self.device, _ffi.MODES[self.what], self.max_batch
        slot_of, start_of = (ctypes.c_int * mb)(), (ctypes.c_int64 * mb)()
        length, count = ctypes.c_int64(), ctypes.c_int()
        with torch.cuda.device(dev):
            while True:
                _ffi.check(lib.acx_stream_next(self._h, mb, slot_of, start_of, ctypes.byref(length), ctypes.byref(count)))
                n, L = count.value, length.value
                if n == 0:
                    break
                ctx = self.model.native_context(dev)
                ws = self.model._workspace(dev, ctx.workspace_bytes_windows(n, L, mode))
                o0, o1, _ = self.model._outputs(self.what, (n,), self.classes, L, dev)
                _ffi.check(lib.acx_stream_forward(self._h, n, mode, _ffi.ptr(o0), _ffi.ptr(o1), _ffi.ptr(ws), ws.numel(),
                                                  _ffi.stream_ptr(dev)))
                out.add(list(slot_of[:n]), list(start_of[:n]), o0, o1)
            if self.timeline:
                rows = ctypes.c_int64()
                _ffi.check(lib.acx_stream_pending(self._h, None, ctypes.byref(rows)))
                r = rows.value
                if r:
                    tl = torch.empty((r, self.classes), dtype=torch.float32, device=dev)
                    ts, tk, got = (ctypes.c_int * r)(), (ctypes.c_int64 * r)(), ctypes.c_int64()
                    _ffi.check(lib.acx_stream_timeline(self._h, 1 if self.timeline == "max" else 0, r, _ffi.ptr(tl), ts, tk,
                                                       ctypes.byref(got), _ffi.stream_ptr(dev)))
                    out.add_rows(list(ts[:got.value]), list(tk[:got.value]), tl[:got.value])


class _Result:
    """The flat dict of one call: one row per window emitted, in slot order and then start order."""

    def __init__(self, st):
        self.st = st
        self.slot, self.start, self.o0, self.o1 = [], [], [], []
        self.tslot, self.tstep, self.tl = [], [], []
        self.short = []

    def add(self, slots, starts, o0, o1):
        self.slot += slots
        self.start += starts
        self.o0.append(o0)
        self.o1.append(o1)

    def add_rows(self, slots, steps, tl):
        self.tslot += slots
        self.tstep += steps
        self.tl.append(tl)

    @staticmethod
    def _order(keys):
        idx = sorted(range(len(keys)), key=lambda i: keys[i])
        return None if idx == list(range(len(keys))) else idx

    def result(self):
        st, dev = self.st, self.st.device
        order = self._order(list(zip(self.slot, self.start)))
        slot = [self.slot[i] for i in order] if order else self.slot
        start = [self.start[i] for i in order] if order else self.start
        d = {"slot": torch.tensor(slot, dtype=torch.int64),
             "starts": torch.tensor(start, dtype=torch.float64) / _rs.MODEL_RATE,
             "short": sorted(self.short)}

        def rows(parts, empty_shape):
            if not parts:
                return torch.empty(empty_shape, dtype=torch.float32, device=dev)
            t = parts[0] if len(parts) == 1 else torch.cat(parts)
            return t if order is None else t[torch.tensor(order, device=dev)]

        if st.what == "logits":
            d["clipwise_logits"] = rows(self.o0, (0, st.classes))
            d["clipwise_output"] = rows(self.o1, (0, st.classes))
        elif st.what == "scene":
            d["scene"] = rows(self.o0, (0, 768))
        else:
            shapes = {tuple(p.shape[1:]) for p in self.o0}
            if len(shapes) <= 1:
                d["frame"] = rows(self.o0, (0, 768) + _ffi.stage_hw(st.window, 3))
            else:                 # a short clip's frames are shorter than a window's: one (768, T', 7) tensor per window
                each = [t for p in self.o0 for t in p]
                d["frame"] = [each[i] for i in order] if order else each
        if st.timeline:
            torder = self._order(list(zip(self.tslot, self.tstep)))
            tl = torch.empty((0, st.classes), dtype=torch.float32, device=dev) if not self.tl else (
                self.tl[0] if len(self.tl) == 1 else torch.cat(self.tl))
            if torder is not None:
                tl = tl[torch.tensor(torder, device=dev)]
            d["timeline"] = tl
            d["timeline_slot"] = torch.tensor([self.tslot[i] for i in torder] if torder else self.tslot, dtype=torch.int64)
            d["timeline_step"] = torch.tensor([self.tstep[i] for i in torder] if torder else self.tstep, dtype=torch.int64)
        return d
