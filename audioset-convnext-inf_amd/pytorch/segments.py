"""Sound event detection on the host side (ConvNeXt.forward_segments / forward_segment_embeddings, include/acx.h "sound event
detection"): the geometry of segments, frames and the segment timeline -- one definition shared with the C ABI -- and the
decoding of probabilities over time into events: decode_events on the host -- nothing down to it touches the GPU -- and
decode_events_gpu / EventTable, the same decoding for whole batches on the device (acx_decode_events), and for rows that arrive
chunk by chunk OnlineEventDecoderHost, the definition, and EventStream, its device form (acx_event_stream_*).

The trunk halves time four times after a stride-4 stem on hop-320 frames, so one row of the stage-3 map -- one SEGMENT -- stands
for 32 STFT frames = 10240 samples = 0.32 s at 32 kHz.  A clip of L samples has T = L // 320 + 1 frames and
S = ((T + 4) // 4 + 1) // 8 = (T + 8) // 32 segments (acx_stage_hw(L, 3)); segment t covers samples [10240 t, 10240 (t + 1)) and the
last one reaches to the clip's end.  Frame u belongs to segment min(u // 32, S - 1): the reference's interpolate(x, 32) followed
by pad_framewise_output (pytorch/pytorch_utils.py:140-176)."""
import ctypes

import numpy as np

from .. import _ffi
from . import windows as _win

MODEL_RATE = 32000
HOP = 320
FRAMES_PER_SEGMENT = 32
SEGMENT_SAMPLES = _ffi.SEGMENT_SAMPLES          # 10240
SEGMENT_SECONDS = SEGMENT_SAMPLES / MODEL_RATE  # 0.32


def check_pool(pool):
    """The pooling widths of the recipe: odd, 1 .. 31 (ValueError otherwise)."""
    if isinstance(pool, bool) or not isinstance(pool, int) or not 1 <= pool <= _ffi.MAX_SEGMENT_POOL or pool % 2 == 0:
        raise ValueError("pool must be an odd integer in [1, %d] (got %r)" % (_ffi.MAX_SEGMENT_POOL, pool))
    return pool


def _check_length(L):
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < _ffi.MIN_SAMPLES:
        raise ValueError("a clip needs at least %d samples at 32 kHz (got %r)" % (_ffi.MIN_SAMPLES, L))
    return int(L)


def segment_count(L):
    """S of a clip of L samples at 32 kHz: the height of the stage-3 map, (T + 8) // 32 with T = L // 320 + 1."""
    return (_check_length(L) // HOP + 1 + 8) // FRAMES_PER_SEGMENT


def segment_edges(L, duration=None):
    """The S + 1 segment boundaries of a clip of L samples at 32 kHz, in seconds (float64 numpy): 0, 0.32, 0.64, ... and the
    clip's end -- `duration` seconds when given (the length of the audio before resampling), else L / 32000."""
    S = segment_count(L)
    edges = np.arange(S + 1, dtype=np.float64) * SEGMENT_SECONDS
    edges[S] = L / MODEL_RATE if duration is None else float(duration)
    return edges


def frame_to_segment(T, S):
    """The segment of each of T frames (int64 numpy): min(u // 32, S - 1)."""
    if T < 1 or S < 1:
        raise ValueError("frame_to_segment needs T >= 1 and S >= 1 (got %r, %r)" % (T, S))
    return np.minimum(np.arange(T, dtype=np.int64) // FRAMES_PER_SEGMENT, S - 1)


def window_segments(L, window):
    """Segments of one window of a recording of L samples: the window holds min(window, L) samples."""
    return segment_count(min(L, window))


def segment_timeline_cover(lengths, window, hop):
    """The segment timeline of forward_windows(what="segment") / acx_segment_timeline, spelled out.  Recording r of L samples has
    ceil(L / 10240) rows; row k has the midpoint m = min(10240 k + 5120, L - 1) and takes, from every window j with
    s_j <= m < s_j + min(window, L), the segment i = min((m - s_j) // 10240, S_w - 1).  Returns one list per row, in row order,
    of (recording, j, i, probs_row) in ascending j; probs_row indexes the windows' (S_w, N) blocks laid back to back in window
    order."""
    _win.check_window(window, hop)
    out, base = [], 0
    for r, L in enumerate(lengths):
        L = int(L)
        if L == 0:
            continue
        Sw = window_segments(L, window)
        span = min(window, L)
        starts = _win.window_starts([L], window, hop)
        for k in range((L + SEGMENT_SAMPLES - 1) // SEGMENT_SAMPLES):
            m = min(k * SEGMENT_SAMPLES + SEGMENT_SAMPLES // 2, L - 1)
            row = []
            for j, s in enumerate(starts):
                if s <= m < s + span:
                    i = min((m - s) // SEGMENT_SAMPLES, Sw - 1)
                    row.append((r, j, i, base + j * Sw + i))
            out.append(row)
        base += len(starts) * Sw
    return out


def median_filter(p, width):
    """Odd-width running median over axis 0; the ends repeat the first / last row."""
    if width == 1:
        return p
    h = width // 2
    padded = np.concatenate([np.repeat(p[:1], h, axis=0), p, np.repeat(p[-1:], h, axis=0)])
    return np.median(np.stack([padded[i:i + p.shape[0]] for i in range(width)]), axis=0).astype(p.dtype)


def _is_number(v):
    return np.ndim(v) == 0 and not hasattr(v, "detach")


def _host_level(v, p=None):
    """A threshold / low argument on the host: None and numbers pass as they are; per-class values (array, list, tensor)
    become a 1-D array in the precision of the probabilities p (float32 without p) -- what the device compares in."""
    if v is None or _is_number(v):
        return v
    a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("per-class threshold / low must hold numbers (got dtype %s)" % a.dtype)
    if a.ndim != 1:
        raise ValueError("per-class threshold / low must be one-dimensional (got shape %r)" % (a.shape,))
    kind = p.dtype if p is not None and np.issubdtype(p.dtype, np.floating) else np.float32
    return a.astype(kind)


def _check_levels(threshold, low, classes=None):
    """0 <= low <= threshold for numbers and host arrays (low already resolved), class by class, with decode_events' message;
    an array must hold one value per class."""
    for v in (threshold, low):
        if np.ndim(v) == 1 and classes is not None and v.shape[0] != classes:
            raise ValueError("%d per-class values for %d classes" % (v.shape[0], classes))
    if np.ndim(threshold) == 0 and np.ndim(low) == 0:
        if not 0.0 <= low <= threshold:
            raise ValueError("low must be in [0, threshold] (got low=%r, threshold=%r)" % (low, threshold))
        return
    if np.ndim(threshold) == 1 and np.ndim(low) == 1 and threshold.shape != low.shape:
        raise ValueError("%d thresholds and %d lows" % (threshold.shape[0], low.shape[0]))
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(low) >= 0.0) & (np.asarray(low) <= np.asarray(threshold))           # a NaN fails both
    if not np.all(ok):
        c = int(np.nonzero(~np.broadcast_to(ok, np.broadcast(threshold, low).shape))[0][0])
        raise ValueError("low must be in [0, threshold] (got low=%r, threshold=%r) in class %d"
                         % (float(low if np.ndim(low) == 0 else low[c]), float(threshold if np.ndim(threshold) == 0 else threshold[c]), c))


def decode_events(probs, threshold=0.5, low=None, median=1, min_duration=0.0, merge_gap=0.0, step=SEGMENT_SECONDS, labels=None):
    """Probabilities over time -> events.  probs: (steps, classes), a torch tensor or array -- "segmentwise_output" /
    "framewise_output" of one clip, or a forward_windows timeline.  Per class, after an optional odd `median` filter over time:
    an event is a maximal run of steps with p >= low that holds a value >= threshold (hysteresis; low=None: low = threshold);
    events of a class closer than `merge_gap` seconds are merged, then events shorter than `min_duration` seconds are dropped.
    threshold / low: one number for every class, or one per class (an array or tensor of `classes` values, e.g.
    metrics.operating_points(...).threshold; +inf: the class emits nothing), compared in the probabilities' own precision.
    step: seconds per row (0.32 for segments, 0.01 for frames), or the steps + 1 boundaries in seconds ("segment_edges").
    Returns [(class, onset_s, offset_s, peak, mean), ...] sorted by onset; class is labels[c] when labels are given, else c;
    peak / mean are taken over the event's rows of the filtered probabilities."""
    if hasattr(probs, "detach"):
        probs = probs.detach().cpu().numpy()
    p = np.asarray(probs)
    if p.ndim != 2:
        raise ValueError("decode_events expects (steps, classes) probabilities, got shape %r" % (p.shape,))
    threshold, low = _host_level(threshold, p), _host_level(low, p)
    low = threshold if low is None else low
    _check_levels(threshold, low, p.shape[1])
    if isinstance(median, bool) or not isinstance(median, int) or median < 1 or median % 2 == 0:
        raise ValueError("median must be an odd positive integer (got %r)" % (median,))
    if min_duration < 0 or merge_gap < 0:
        raise ValueError("min_duration and merge_gap must not be negative")
    if labels is not None and len(labels) != p.shape[1]:
        raise ValueError("%d labels for %d classes" % (len(labels), p.shape[1]))
    n = p.shape[0]
    if np.ndim(step) == 0:
        if not step > 0:
            raise ValueError("step must be positive (got %r)" % (step,))
        edges = np.arange(n + 1, dtype=np.float64) * float(step)
    else:
        edges = np.asarray(step, dtype=np.float64)
        if edges.shape != (n + 1,):
            raise ValueError("%d boundaries for %d steps (expected steps + 1)" % (edges.size, n))
    if n == 0:
        return []
    p = median_filter(p, median)
    events = []
    for c in np.nonzero((p >= threshold).any(axis=0))[0]:
        col = p[:, c]
        thr_c, low_c = (v if np.ndim(v) == 0 else v[c] for v in (threshold, low))
        on = np.concatenate([[False], col >= low_c, [False]])
        begins = np.nonzero(on[1:] & ~on[:-1])[0]
        ends = np.nonzero(~on[1:] & on[:-1])[0]                 # exclusive
        runs = [[b, e] for b, e in zip(begins, ends) if col[b:e].max() >= thr_c]
        merged = []
        for b, e in runs:
            if merged and edges[b] - edges[merged[-1][1]] < merge_gap:
                merged[-1][1] = e
            else:
                merged.append([b, e])
        for b, e in merged:
            if edges[e] - edges[b] < min_duration:
                continue
            events.append((labels[c] if labels is not None else int(c), float(edges[b]), float(edges[e]),
                           float(col[b:e].max()), float(col[b:e].mean())))
    events.sort(key=lambda ev: (ev[1], ev[2], str(ev[0])))
    return events


class OnlineEventDecoderHost:
    """decode_events for ONE recording whose rows arrive chunk by chunk: the definition of the online decoder (include/acx.h
    "online event decoding", csrc/events_online.hip), the per-column state machine of csrc/events_common.h restated step by
    step on the host, every class at once.  push(rows) takes (r, classes) rows, r >= 0, and returns the events this call makes
    final; close(end_seconds=None) flushes and returns the rest (the decoder then stands ready for a new recording).  Events
    are rows (cls, begin, end, peak, mean) in (cls, begin) order, begin / end in absolute steps of the recording; over all
    calls they are decode_events of the concatenated rows, each exactly once, for any chunking (mean: the float64 sum in
    ascending time over [begin, end) divided by the count; decode_events takes numpy's float32 mean).

    Filtered row t exists once raw row t + median // 2 has been pushed (the front repeats row 0; close repeats the last row).
    After filtered row t a pending event [eb, ee) is final -- and emitted, if edge(ee) - edge(eb) is no shorter than
    min_duration -- when a run is open that began at rb and not edge(rb) - edge(ee) < merge_gap, or when no run is open and
    not edge(t + 1) - edge(ee) < merge_gap, with edge(k) = float64(k) * step: k * step never decreases in k, so no later run
    could have merged.  A run still open is part of no emitted event.  The free last boundary enters only in close().
    open_begin()[c]: the step at which the event that class c is inside of began -- the pending event's begin when the open
    run will merge with it, else the run's -- once the open run has reached `threshold`; -1 otherwise."""

    def __init__(self, classes, threshold=0.5, low=None, median=1, min_duration=0.0, merge_gap=0.0, step=SEGMENT_SECONDS):
        if isinstance(classes, bool) or not isinstance(classes, (int, np.integer)) or classes < 1:
            raise ValueError("classes must be a positive integer (got %r)" % (classes,))
        threshold, low = _host_level(threshold), _host_level(low)
        low = threshold if low is None else low
        _check_levels(threshold, low, classes)
        if isinstance(median, bool) or not isinstance(median, int) or median < 1 or median % 2 == 0:
            raise ValueError("median must be an odd positive integer (got %r)" % (median,))
        if min_duration < 0 or merge_gap < 0:
            raise ValueError("min_duration and merge_gap must not be negative")
        if np.ndim(step) != 0 or not step > 0:
            raise ValueError("step must be a positive number of seconds (got %r)" % (step,))
        N = self.classes = int(classes)
        self.thr = np.broadcast_to(np.asarray(threshold, dtype=np.float32), (N,))
        self.low = np.broadcast_to(np.asarray(low, dtype=np.float32), (N,))
        self.median, self.h = median, median // 2
        self.min_duration, self.merge_gap, self.step = float(min_duration), float(merge_gap), float(step)
        self._reset()

    def _reset(self):
        N = self.classes
        self.steps = 0                       # raw rows of the open recording
        self.t = 0                           # filtered rows consumed
        self._raw = {}                       # raw row i, for the rows a filtered row still to come reads
        self._end = None                     # close(): (steps, end_seconds) of edge()
        self.in_run, self.rvalid, self.have = (np.zeros(N, dtype=bool) for _ in range(3))
        self.rb, self.eb, self.ee = (np.zeros(N, dtype=np.int64) for _ in range(3))
        self.rmax, self.emax, self.epeak = (np.zeros(N, dtype=np.float32) for _ in range(3))
        self.rsum, self.esum, self.esnap = (np.zeros(N, dtype=np.float64) for _ in range(3))

    def _edge(self, k):
        e = np.asarray(k, dtype=np.float64) * self.step
        if self._end is not None:
            e = np.where(np.asarray(k) < self._end[0], e, self._end[1])
        return e

    def _finish_event(self, m, out):
        keep = m & ~(self._edge(self.ee) - self._edge(self.eb) < self.min_duration)
        for c in np.nonzero(keep)[0]:
            b, e = int(self.eb[c]), int(self.ee[c])
            out.append((int(c), b, e, float(self.epeak[c]), float(self.esnap[c] / np.float64(e - b))))

    def _end_run(self, t, m, out):
        self.in_run[m] = False
        m = m & self.rvalid
        merge = m & self.have & (self._edge(self.rb) - self._edge(self.ee) < self.merge_gap)
        self.ee[merge] = t
        self.epeak[merge] = self.emax[merge]
        self.esnap[merge] = self.esum[merge]
        new = m & ~merge
        self._finish_event(new & self.have, out)
        self.have[new] = True
        self.eb[new] = self.rb[new]
        self.ee[new] = t
        self.epeak[new] = self.emax[new] = self.rmax[new]
        self.esnap[new] = self.esum[new] = self.rsum[new]

    def _step(self, t, p, out):
        on = p >= self.low
        self._end_run(t, ~on & self.in_run, out)
        hv = self.have
        self.emax[hv] = np.maximum(self.emax[hv], p[hv])
        self.esum[hv] += p[hv].astype(np.float64)
        start = on & ~self.in_run
        self.in_run[start] = True
        self.rb[start] = t
        self.rvalid[start] = False
        self.rmax[start] = p[start]
        self.rsum[start] = 0.0
        self.rmax[on] = np.maximum(self.rmax[on], p[on])
        self.rsum[on] += p[on].astype(np.float64)
        self.rvalid[on] |= p[on] >= self.thr[on]
        # early emission: the pending event is final once nothing still to come can merge with it
        since = np.where(self.in_run, self.rb, t + 1)
        final = self.have & ~(self._edge(since) - self._edge(self.ee) < self.merge_gap)
        self._finish_event(final, out)
        self.have[final] = False

    def _consume(self, upto, last, out):
        """filtered rows t .. upto - 1; raw rows past `last` repeat row `last`"""
        h = self.h
        while self.t < upto:
            t = self.t
            win = np.stack([self._raw[min(max(t + j, 0), last)] for j in range(-h, h + 1)])
            self._step(t, np.median(win, axis=0).astype(np.float32), out)
            self.t = t + 1

    def push(self, rows):
        rows = np.asarray(rows.detach().cpu().numpy() if hasattr(rows, "detach") else rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.classes:
            raise ValueError("push expects (rows, %d) probabilities, got shape %r" % (self.classes, rows.shape))
        if not np.isfinite(rows).all():
            raise ValueError("the probabilities hold a NaN or an infinity")
        for r in rows:
            self._raw[self.steps] = r
            self.steps += 1
        out = []
        self._consume(self.steps - self.h, self.steps - 1, out)
        for i in [i for i in self._raw if i < self.t - self.h]:     # what no filtered row still to come reads
            del self._raw[i]
        return sorted(out, key=lambda e: (e[0], e[1]))

    def close(self, end_seconds=None):
        out = []
        n = self.steps
        if n:
            self._consume(n, n - 1, out)
            self._end = (n, float(end_seconds) if end_seconds is not None and end_seconds > 0 else float(n) * self.step)
            self._end_run(n, self.in_run.copy(), out)
            self._finish_event(self.have, out)
        self._reset()
        return sorted(out, key=lambda e: (e[0], e[1]))

    def open_begin(self):
        merges = self.have & (self._edge(self.rb) - self._edge(self.ee) < self.merge_gap)
        return np.where(self.in_run & self.rvalid, np.where(merges, self.eb, self.rb), -1).astype(np.int64)


# ---- the same decoding on the device (include/acx.h "sound event decoding", csrc/events.hip) ---------------------------------

_GPU_EDGES = "only uniform steps with a free last boundary run on the GPU (edges k * step for k < steps, then the clip's end)"


def _on_device(v):
    return hasattr(v, "is_cuda") and v.is_cuda


def check_event_args(threshold, low, median, min_duration, merge_gap, classes=None):
    """decode_events' argument checks and messages, plus the device's cap on `median`.  Returns (threshold, low) with None
    resolved and per-class host values as float32 arrays.  Per-class CUDA tensors pass unread: their values are checked on the
    device (ACX_EVENTS_BAD_THRESHOLD, raised when the table is first read), only their length here."""
    threshold = threshold if _on_device(threshold) else _host_level(threshold)
    low = low if _on_device(low) else _host_level(low)
    low = threshold if low is None else low
    for v in (threshold, low):
        if _on_device(v) and (v.dim() != 1 or (classes is not None and v.shape[0] != classes)):
            raise ValueError("per-class threshold / low of shape %r for %s classes" % (tuple(v.shape), classes))
    if not (_on_device(threshold) or _on_device(low)):
        _check_levels(threshold, low, classes)
    elif not _on_device(threshold):
        _check_levels(threshold, 0.0, classes)                      # of a mixed pair, what the host can see: threshold >= 0
    elif not _on_device(low):
        _check_levels(low, low, classes)                            # low >= 0
    if isinstance(median, bool) or not isinstance(median, int) or median < 1 or median % 2 == 0:
        raise ValueError("median must be an odd positive integer (got %r)" % (median,))
    if median > _ffi.MAX_EVENT_MEDIAN:
        raise ValueError("median must be at most %d on the GPU (got %r)" % (_ffi.MAX_EVENT_MEDIAN, median))
    if min_duration < 0 or merge_gap < 0:
        raise ValueError("min_duration and merge_gap must not be negative")
    return threshold, low


def _uniform_edges(edges, n):
    """(step or None, end) of one clip's n + 1 boundaries when they are k * step for k < n plus a free, positive last one;
    ValueError otherwise.  step is None for a single step (any step fits)."""
    e = np.asarray(edges, dtype=np.float64)
    if e.shape != (n + 1,):
        raise ValueError("%d boundaries for %d steps (expected steps + 1)" % (e.size, n))
    if e[0] != 0.0 or not e[n] > 0.0:
        raise ValueError(_GPU_EDGES)
    if n == 1:
        return None, float(e[1])
    step = float(e[1])
    if not step > 0.0 or not np.array_equal(e[:n], np.arange(n, dtype=np.float64) * step):
        raise ValueError(_GPU_EDGES)
    return step, float(e[n])


class EventTable:
    """The events of a batch, on the device: one (capacity, 32-byte) buffer of acx_event rows ordered by (clip, cls, begin),
    of which the first `count` are valid.  clip / cls / begin / end (int32), peak (fp32) and mean (fp64) are views of it;
    count (int64) and status (int32) are device tensors of one element; edges: per clip the float64 boundaries in seconds
    (host).  Creating a table does not synchronise; len(), to_lists() and check() do."""

    def __init__(self, table, count, status, edges, classes, rerun=None):
        self._set(table, count, status)
        self.edges = edges
        self.classes = classes
        self._rerun = rerun          # capacity -> (table, count, status): decodes again into a larger table
        self._n = None

    def _set(self, table, count, status):
        self.table, self.count, self.status = table, count, status
        self.clip, self.cls, self.begin, self.end = (table[:, i] for i in range(4))
        self.peak = table.view(_torch().float32)[:, 4]
        self.mean = table.view(_torch().float64)[:, 3]

    @property
    def capacity(self):
        return self.table.shape[0]

    def check(self):
        """Waits for the decoding.  ValueError when the probabilities held a NaN or an infinity, or a per-class threshold / low
        on the device was not 0 <= low <= threshold; a table that was too small is decoded once more at the exact size (with
        the same per-class values).  Returns self."""
        if self._n is None:
            n, st = int(self.count.cpu()), int(self.status.cpu())
            if st & _ffi.EVENTS_NONFINITE:
                raise ValueError("the probabilities hold a NaN or an infinity")
            if st & _ffi.EVENTS_BAD_THRESHOLD:
                raise ValueError("low must be in [0, threshold] in every class (a per-class value on the device is out of "
                                 "order, negative or NaN)")
            if st & _ffi.EVENTS_OVERFLOW or n > self.capacity:
                if self._rerun is None:
                    raise ValueError("%d events for a table of %d rows" % (n, self.capacity))
                self._set(*self._rerun(n))
                n, st = int(self.count.cpu()), int(self.status.cpu())
                if st or n > self.capacity:
                    raise RuntimeError("event table: status %d, %d events for %d rows after the second pass" % (st, n, self.capacity))
            self._n = n
        return self

    def __len__(self):
        return self.check()._n

    def to_lists(self, labels=None):
        """One list per clip of (class, onset_s, offset_s, peak, mean), sorted like decode_events' output, by
        (onset, offset, str(class)); class is labels[c] when labels are given, else c."""
        if labels is not None and len(labels) != self.classes:
            raise ValueError("%d labels for %d classes" % (len(labels), self.classes))
        n = len(self)
        rows = self.table[:n].cpu().contiguous().numpy()
        clip, cls, begin, end = (rows[:, i].tolist() for i in range(4))
        peak = rows.view(np.float32)[:, 4].tolist()
        mean = rows.view(np.float64)[:, 3].tolist()
        out = [[] for _ in self.edges]
        for i in range(n):
            e = self.edges[clip[i]]
            c = cls[i]
            out[clip[i]].append((labels[c] if labels is not None else c, float(e[begin[i]]), float(e[end[i]]), peak[i], mean[i]))
        for events in out:
            events.sort(key=lambda ev: (ev[1], ev[2], str(ev[0])))
        return out


def _torch():
    import torch
    return torch


def decode_events_gpu(probs, threshold=0.5, low=None, median=1, min_duration=0.0, merge_gap=0.0, step=SEGMENT_SECONDS,
                      capacity=None, steps=None):
    """decode_events for whole batches on the GPU (acx_decode_events): the same events, bit for bit, except that `mean` is the
    float64 mean of the event's rows (decode_events takes numpy's float32 one).  probs: a fp32 CUDA tensor (steps, N) or
    (B, steps, N) -- the last stride must be 1; a row stride is passed on where the layout allows it, else a contiguous copy is
    made -- or up to 256 clips of different lengths: a list of (steps_i, N) tensors, or one packed (sum(steps), N) tensor with
    steps=[...].  step: seconds per row, or boundaries as segment_edges gives them ((steps + 1,), or one such array per clip):
    k * step for k < steps and any positive last one; other boundaries raise ValueError.  capacity: rows of the table
    (default max(1024, 16 * clips)); a table that turns out too small is decoded again at the exact size when it is first
    read.  threshold / low: numbers, or one value per class -- a host array (checked here, then copied) or a CUDA tensor (used
    where it is, e.g. metrics.operating_points(...).threshold; checked on the device, ValueError when the table is first read).
    Runs on the current stream without synchronising.  Returns an EventTable."""
    torch = _torch()
    scalar_levels = _is_number(threshold) and (low is None or _is_number(low))
    threshold, low = check_event_args(threshold, low, median, min_duration, merge_gap)
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0):
        raise ValueError("capacity must be a non-negative integer (got %r)" % (capacity,))
    # ---- the clips: uniform (B, S, N) or ragged (steps per clip over packed rows)
    ragged = None
    if isinstance(probs, (list, tuple)):
        if steps is not None:
            raise ValueError("steps= goes with one packed tensor, not with a list of clips")
        if not probs:
            raise ValueError("decode_events_gpu expects at least one clip")
        if len(probs) > _ffi.MAX_VARLEN_CLIPS:
            raise ValueError("at most %d clips of different lengths per call (got %d)" % (_ffi.MAX_VARLEN_CLIPS, len(probs)))
        for t in probs:
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != probs[0].shape[1]:
                raise ValueError("decode_events_gpu expects a list of (steps, classes) tensors of one class count")
        ragged = [int(t.shape[0]) for t in probs]
        first = probs[0]
    else:
        if not isinstance(probs, torch.Tensor):
            raise ValueError("decode_events_gpu expects CUDA tensors (got %s); decode_events takes arrays" % type(probs).__name__)
        first = probs
        if steps is not None:
            ragged = [int(n) for n in steps]
            if len(ragged) > _ffi.MAX_VARLEN_CLIPS:
                raise ValueError("at most %d clips of different lengths per call (got %d)" % (_ffi.MAX_VARLEN_CLIPS, len(ragged)))
            if probs.dim() != 2 or not ragged or sum(ragged) != probs.shape[0]:
                raise ValueError("steps=%r do not add up to the %r packed rows" % (ragged, tuple(probs.shape)))
        elif probs.dim() not in (2, 3):
            raise ValueError("decode_events_gpu expects (steps, classes) or (batch, steps, classes) probabilities, got shape %r"
                             % (tuple(probs.shape),))
    if ragged is not None:
        clip_steps = ragged
    elif probs.dim() == 2:
        clip_steps = [int(probs.shape[0])]
    else:
        clip_steps = [int(probs.shape[1])] * int(probs.shape[0])
    N = int(first.shape[-1])
    if not clip_steps or min(clip_steps) < 1 or N < 1:
        raise ValueError("decode_events_gpu needs at least one step and one class per clip (steps %r, %d classes)"
                         % (clip_steps if len(clip_steps) <= 8 else clip_steps[:8] + ["..."], N))
    B = len(clip_steps)
    for v in (threshold, low):
        if not _is_number(v) and tuple(v.shape) != (N,):
            raise ValueError("%d per-class values for %d classes" % (v.shape[0], N))
    # ---- the boundaries: one step and a last boundary per clip
    ends = None
    per_clip = isinstance(step, (list, tuple)) and len(step) > 0 and np.ndim(step[0]) == 1
    if not per_clip and np.ndim(step) == 0:
        if not step > 0:
            raise ValueError("step must be positive (got %r)" % (step,))
        step_s = float(step)
    else:
        if per_clip and len(step) != B:
            raise ValueError("%d boundary arrays for %d clips" % (len(step), B))
        if not per_clip and len(set(clip_steps)) != 1:
            raise ValueError("clips of different lengths need one boundary array each")
        found = [_uniform_edges(step[i] if per_clip else step, clip_steps[i]) for i in range(B if per_clip else 1)]
        known = {s for s, _ in found if s is not None}
        if len(known) > 1:
            raise ValueError(_GPU_EDGES + "; the clips' boundaries have different steps: %r" % (sorted(known),))
        step_s = known.pop() if known else found[0][1]
        ends = [e for _, e in found] * (1 if per_clip else B)
    edges = []
    memo = {}
    for i, n in enumerate(clip_steps):
        key = (n, None if ends is None else ends[i])
        if key not in memo:
            e = np.arange(n + 1, dtype=np.float64) * step_s
            if ends is not None:
                e[n] = ends[i]
            memo[key] = e
        edges.append(memo[key])
    # ---- device, dtype, layout
    tensors = list(probs) if isinstance(probs, (list, tuple)) else [probs]
    for t in tensors:
        if not t.is_cuda:
            raise ValueError("decode_events_gpu expects CUDA tensors (got a %s tensor); decode_events decodes on the host"
                             % t.device.type)
        if t.dtype != torch.float32:
            raise ValueError("decode_events_gpu expects float32 probabilities (got %s)" % (t.dtype,))
        if t.device != first.device:
            raise ValueError("the clips lie on different devices")
    dev = first.device
    if isinstance(probs, (list, tuple)):
        x = torch.cat([t.detach() for t in probs]) if len(probs) > 1 else probs[0].detach().contiguous()
    else:
        x = probs.detach()
    rows_of = x.shape[-2]
    if x.stride(-1) != 1 and N > 1:
        x = x.contiguous()
    ld = x.stride(-2) if rows_of > 1 else (x.stride(0) if x.dim() == 3 and x.shape[0] > 1 else N)
    if ld < N or (x.dim() == 3 and x.shape[0] > 1 and x.stride(0) != rows_of * ld):
        x = x.contiguous()
        ld = N
    uniform_end = None
    if ragged is None and (ends is None or len(set(ends)) == 1):
        uniform_end = 0.0 if ends is None else ends[0]
    elif B > _ffi.MAX_VARLEN_CLIPS:
        raise ValueError("at most %d clips with boundaries of their own per call (got %d)" % (_ffi.MAX_VARLEN_CLIPS, B))
    if scalar_levels:
        params = _ffi.event_params(threshold, low, median, min_duration, merge_gap)
        thr_t = low_t = None
    else:
        # per class (acx_decode_events_classwise): a device pointer replaces the field of the same name
        def level(v):
            if _is_number(v):
                return None
            t = v.detach().to(device=dev, dtype=torch.float32).contiguous() if _on_device(v) else torch.from_numpy(v).to(dev)
            if tuple(t.shape) != (N,):
                raise ValueError("%d per-class values for %d classes" % (t.numel(), N))
            return t
        thr_t = level(threshold)
        low_t = None if low is threshold else level(low)            # low=None: the class's own threshold
        if low_t is None and thr_t is not None and low is not threshold:      # a number beside per-class thresholds
            low_t = torch.full((N,), float(low), dtype=torch.float32, device=dev)
        params = _ffi.event_params(threshold if thr_t is None else 0.0, low if _is_number(low) else 0.0, median, min_duration,
                                   merge_gap)
    cap0 = max(1024, 16 * B) if capacity is None else capacity

    def run(cap):
        with torch.cuda.device(dev):
            table = torch.zeros((max(cap, 1), _ffi.EVENT_BYTES // 4), dtype=torch.int32, device=dev)
            meta = torch.zeros(4, dtype=torch.int32, device=dev)
            count, status = meta[:2].view(torch.int64), meta[2:3]
            ws = torch.empty(_ffi.events_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
            tail = (table.data_ptr(), cap, count.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _ffi.stream_ptr(dev))
            if not scalar_levels:               # (this closure keeps thr_t / low_t alive: the re-run reads them again)
                tail += (None if thr_t is None else thr_t.data_ptr(), None if low_t is None else low_t.data_ptr())
            which = "" if scalar_levels else "_classwise"
            if uniform_end is not None:
                _ffi.check(getattr(_ffi.lib(), "acx_decode_events" + which)(x.data_ptr(), ld, B, clip_steps[0], N,
                                                                            ctypes.byref(params), step_s, uniform_end, *tail))
            else:
                c_steps = (ctypes.c_int * B)(*clip_steps)
                c_ends = None if ends is None else (ctypes.c_double * B)(*ends)
                _ffi.check(getattr(_ffi.lib(), "acx_decode_events_varlen" + which)(x.data_ptr(), ld, c_steps, c_ends, B, N,
                                                                                   ctypes.byref(params), step_s, *tail))
        return table, count, status

    return EventTable(*run(cap0), edges=edges, classes=N, rerun=run)


# ---- the online decoder on the device (include/acx.h "online event decoding", csrc/events_online.hip) -------------------------

class _StreamEvents(EventTable):
    """The EventTable of one EventStream call: `clip` is the slot, begin / end are steps of the slot's recording.  A call over
    more than 256 slots (and a ConvNeXt.stream call that pushes and closes) is several device calls: their tables are joined
    -- in call order, each ordered (slot, cls, begin) -- when the table is first read, so `table`, `count`, `status` and the
    column views then wait for the decoding like len() does.  to_lists() returns {slot: events} over the slots of the call."""

    def __init__(self, owner, parts):
        self._owner, self._parts = owner, parts
        self.classes = owner.classes
        self.edges = None
        self._rerun = None
        self._n = None
        if len(parts) == 1:
            self._set(parts[0]["table"], parts[0]["count"], parts[0]["status"])

    def __getattr__(self, name):
        # a joined table exists once its parts have been read
        if name in ("table", "count", "status", "clip", "cls", "begin", "end", "peak", "mean") and self._n is None:
            self.check()
            return getattr(self, name)
        raise AttributeError(name)

    def check(self):
        """Waits for the decoding.  A part whose table was too small is issued once more at the exact size -- the device state
        is untouched by a void call -- and a part whose rows held a NaN or an infinity raises ValueError: its slots have
        consumed nothing (reading again gives the events of the other parts)."""
        if self._n is not None:
            return self
        own = self._owner
        if own is not None and own._pending is self:
            own._pending = None
        torch = _torch()
        parts = self._parts
        refused = []
        for p in parts:
            p["done"].synchronize()
            m = p["seen"]
            n, st = int(m[:2].view(torch.int64)), int(m[2])
            if st & _ffi.EVENTS_NONFINITE:
                own._undo(p["slots"])
                refused.append(p)
                continue
            if st & _ffi.EVENTS_OVERFLOW or n > p["table"].shape[0]:
                own._undo(p["slots"])
                p.update(p["issue"](n))
                p["done"].synchronize()
                m = p["seen"]
                n2, st = int(m[:2].view(torch.int64)), int(m[2])
                if st or n2 != n:
                    raise RuntimeError("event stream: status %d, %d events for %d rows after the second pass" % (st, n2, n))
            p["n"] = n
        if refused:
            self._parts = [p for p in parts if p not in refused]
            raise ValueError("the probabilities hold a NaN or an infinity (slots %s: their rows were not consumed)"
                             % sorted(s for p in refused for s in p["slots"]))
        if len(parts) == 1:
            self._set(parts[0]["table"], parts[0]["count"], parts[0]["status"])
        else:
            dev = own.device
            rows = [p["table"][:p["n"]] for p in parts if p["n"]]
            total = sum(p["n"] for p in parts)
            self._set(torch.cat(rows) if rows else torch.zeros((1, _ffi.EVENT_BYTES // 4), dtype=torch.int32, device=dev),
                      torch.tensor([total], dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        self._n = sum(p["n"] for p in parts)
        return self

    def to_lists(self, labels=None):
        """{slot: [(class, onset_s, offset_s, peak, mean), ...]} over the slots of the call, each list sorted like
        decode_events' output; onset / offset are k * step, and the recording's own last boundary where close() gave one."""
        if labels is not None and len(labels) != self.classes:
            raise ValueError("%d labels for %d classes" % (len(labels), self.classes))
        n = len(self)
        step = self._owner.step
        ends = {}
        out = {}
        for p in self._parts:
            for s in p["slots"]:
                out.setdefault(s, [])
            ends.update(p.get("ends") or {})
        rows = self.table[:n].cpu().contiguous().numpy()
        clip, cls, begin, end = (rows[:, i].tolist() for i in range(4))
        peak = rows.view(np.float32)[:, 4].tolist()
        mean = rows.view(np.float64)[:, 3].tolist()
        for i in range(n):
            last = ends.get(clip[i])
            off = last[1] if last is not None and end[i] >= last[0] else float(np.float64(end[i]) * step)
            c = cls[i]
            out[clip[i]].append((labels[c] if labels is not None else c, float(np.float64(begin[i]) * step), off, peak[i], mean[i]))
        for events in out.values():
            events.sort(key=lambda ev: (ev[1], ev[2], str(ev[0])))
        return out


class EventStream:
    """decode_events_gpu for recordings whose rows arrive chunk by chunk (acx_event_stream_*): `slots` recordings at a time,
    each column's state carried across calls on the device.  Every event is handed out exactly once, as soon as nothing still
    to come can change it (OnlineEventDecoderHost is the definition), and the rows of all calls of a recording, sorted by
    (cls, begin), are the rows of decode_events_gpu over the whole matrix byte for byte, for any chunking.  Arguments as
    decode_events_gpu's; step is the seconds per row (the recording's last boundary is close()'s end_seconds).  Per-class
    threshold / low (host arrays or CUDA tensors) are copied and checked here: a bad level raises ValueError at once.

    push() and close() run on the current stream without synchronising and return an EventTable with clip = slot.  A table
    that turns out too small is decoded again at the exact size when it is first read: a void call leaves the device state
    untouched.  For that to hold, while a table of the handle is unchecked a further push() or close() on the handle checks
    it first -- one read of its count / status, which waits for that earlier call alone (the two words were copied to pinned
    memory behind it), not for work queued since."""

    def __init__(self, slots, classes, threshold=0.5, low=None, median=1, min_duration=0.0, merge_gap=0.0, step=SEGMENT_SECONDS,
                 device=None):
        torch = _torch()
        if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= (1 << 20):
            raise ValueError("slots must be an integer in [1, 2^20] (got %r)" % (slots,))
        if isinstance(classes, bool) or not isinstance(classes, int) or not 1 <= classes <= _ffi.MAX_CLASSES:
            raise ValueError("classes must be an integer in [1, %d] (got %r)" % (_ffi.MAX_CLASSES, classes))
        scalar_levels = _is_number(threshold) and (low is None or _is_number(low))
        threshold, low = check_event_args(threshold, low, median, min_duration, merge_gap, classes)
        if np.ndim(step) != 0 or not step > 0:
            raise ValueError("step must be a positive number of seconds (got %r)" % (step,))
        self._h = None
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("an EventStream lives on a CUDA device (got %s)" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.slots, self.classes, self.step, self.median = slots, classes, float(step), median
        dev = self.device

        def level(v):
            if v is None or _is_number(v):
                return None
            return (v.detach().to(device=dev, dtype=torch.float32) if _on_device(v) else torch.from_numpy(v).to(dev)).contiguous()
        thr_t = None if scalar_levels else level(threshold)
        low_t = None if scalar_levels or low is threshold else level(low)
        if not scalar_levels and low_t is None and thr_t is not None and low is not threshold:
            low_t = torch.full((classes,), float(low), dtype=torch.float32, device=dev)
        params = _ffi.event_params(threshold if thr_t is None else 0.0, low if _is_number(low) else 0.0, median, min_duration,
                                   merge_gap)
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            torch.cuda.current_stream(dev).synchronize()               # the levels are read now
            try:
                _ffi.check(_ffi.lib().acx_event_stream_create(slots, classes, ctypes.byref(params), self.step, _ffi.vp(thr_t),
                                                              _ffi.vp(low_t), ctypes.byref(h)))
            except _ffi.AcxError as e:
                if "must be in [0, threshold" in str(e):
                    raise ValueError("low must be in [0, threshold] in every class (%s)" % e) from None
                raise
        self._h = h
        self._pending = None
        self._last = None
        self._open = set()              # slots pushed to since their last close

    def close_handle(self):
        if self._h is not None and self._h.value:
            _ffi.lib().acx_event_stream_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close_handle()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------- helpers
    def _slot(self, s):
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < self.slots:
            raise ValueError("slot %r out of range (the stream has %d slots)" % (s, self.slots))
        return int(s)

    def _enter(self):
        """The handle's calls run in order: the table still unchecked is checked, a new current stream waits for the last."""
        torch = _torch()
        if self._pending is not None:
            self._pending.check()
        cur = torch.cuda.current_stream(self.device)
        if self._last is not None and self._last != cur:
            ev = torch.cuda.Event()
            ev.record(self._last)
            cur.wait_event(ev)
        self._last = cur

    def _undo(self, slots):
        arr = (ctypes.c_int * len(slots))(*slots)
        _ffi.check(_ffi.lib().acx_event_stream_undo(self._h, arr, len(slots)))

    def _part(self, slots, cap, call, ends=None):
        """One device call -> a part of a _StreamEvents; call(table, cap, count, status) issues it."""
        torch = _torch()
        dev = self.device

        def issue(c):
            with torch.cuda.device(dev):
                table = torch.zeros((max(c, 1), _ffi.EVENT_BYTES // 4), dtype=torch.int32, device=dev)
                meta = torch.zeros(4, dtype=torch.int32, device=dev)
                count, status = meta[:2].view(torch.int64), meta[2:3]
                call(table.data_ptr(), c, count.data_ptr(), status.data_ptr(), _ffi.stream_ptr(dev))
                # count / status travel to pinned memory behind the call: reading them later waits for this call alone,
                # not for whatever the stream has been given since
                seen = torch.empty(4, dtype=torch.int32, pin_memory=True)
                seen.copy_(meta, non_blocking=True)
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(dev))
            return dict(table=table, meta=meta, count=count, status=status, seen=seen, done=done)
        p = dict(slots=slots, issue=issue, ends=ends)
        p.update(issue(cap))
        return p

    def _capacity(self, capacity, n):
        if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0):
            raise ValueError("capacity must be a non-negative integer (got %r)" % (capacity,))
        return max(1024, 16 * n) if capacity is None else capacity

    def _result(self, parts):
        t = _StreamEvents(self, parts)
        self._pending = t
        return t

    # ------------------------------------------------------------------------------------------------------------- calls
    def push(self, probs, slots=None, steps=None, capacity=None):
        """probs: a (r, N) fp32 CUDA tensor for one slot (slots=the slot, default 0), a {slot: (r_i, N)} dict, or one packed
        (sum(steps), N) tensor with slots=[...] and steps=[...] (r_i >= 0).  More than 256 slots are split into several device
        calls; capacity (default max(1024, 16 * slots of the call)) is each call's.  Returns the events this call makes final."""
        torch = _torch()
        packed = None
        if isinstance(probs, dict):
            if slots is not None or steps is not None:
                raise ValueError("slots= / steps= go with a tensor, not with a dict")
            items = [(self._slot(s), t) for s, t in probs.items()]
        elif steps is not None:
            if slots is None or not isinstance(probs, torch.Tensor) or probs.dim() != 2:
                raise ValueError("steps= goes with one packed (rows, classes) tensor and slots=")
            slots, steps = [self._slot(s) for s in slots], [int(n) for n in steps]
            if len(slots) != len(steps) or min(steps, default=0) < 0 or sum(steps) != probs.shape[0]:
                raise ValueError("steps=%r of %d slots do not add up to the %d packed rows" % (steps[:8], len(slots), probs.shape[0]))
            at, items = 0, []
            for s, n in zip(slots, steps):
                items.append((s, probs[at:at + n]))
                at += n
            if all(a < b for a, b in zip(slots, slots[1:])):
                packed = probs
        else:
            items = [(self._slot(0 if slots is None else slots), probs)]
        if not items:
            raise ValueError("push expects at least one slot")
        if len({s for s, _ in items}) != len(items):
            raise ValueError("a slot is listed twice")
        for _, t in items:
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != self.classes:
                raise ValueError("push expects (rows, %d) probabilities, got %r" % (self.classes, getattr(t, "shape", type(t))))
            if not t.is_cuda or t.device != self.device:
                raise ValueError("push expects CUDA tensors on %s (got a tensor on %s)" % (self.device, t.device))
            if t.dtype != torch.float32:
                raise ValueError("push expects float32 probabilities (got %s)" % (t.dtype,))
        items.sort(key=lambda e: e[0])
        cap = self._capacity(capacity, min(len(items), _ffi.MAX_VARLEN_CLIPS))
        self._enter()
        if packed is not None and packed.stride(1) != 1 and self.classes > 1:
            packed = None
        parts, at = [], 0
        for b0 in range(0, len(items), _ffi.MAX_VARLEN_CLIPS):
            batch = items[b0:b0 + _ffi.MAX_VARLEN_CLIPS]
            rows = [int(t.shape[0]) for _, t in batch]
            total = sum(rows)
            if packed is not None:
                x = packed[at:at + total].detach()
                at += total
            else:
                full = [t.detach() for _, t in batch if t.shape[0]]
                x = None if not full else full[0] if len(full) == 1 else torch.cat(full)
            ld = self.classes
            if x is not None and total:
                if (x.stride(1) != 1 and self.classes > 1) or (total > 1 and x.stride(0) < self.classes):
                    x = x.contiguous()
                ld = x.stride(0) if total > 1 else self.classes
            c_slot = (ctypes.c_int * len(batch))(*[s for s, _ in batch])
            c_rows = (ctypes.c_int * len(batch))(*rows)

            def call(table, c, count, status, stream, x=x, ld=ld, c_slot=c_slot, c_rows=c_rows, n=len(batch)):
                _ffi.check(_ffi.lib().acx_event_stream_push(self._h, None if x is None else x.data_ptr(), ld, c_slot, c_rows, n,
                                                            table, c, count, status, stream))
            parts.append(self._part([s for s, _ in batch], cap, call))
            self._open.update(s for s, _ in batch)
        return self._result(parts)

    def close(self, slots=None, end_seconds=None, capacity=None):
        """Ends the recordings of `slots` (default: every slot pushed to since its last close) and returns what is left of their events.
        end_seconds: the recordings' last boundaries -- a number, a list beside slots, or {slot: seconds}; None or <= 0: rows
        * step.  The slots are clean for their next recordings."""
        torch = _torch()
        self._enter()
        if slots is None:
            slots = sorted(self._open)
        elif isinstance(slots, (int, np.integer)) and not isinstance(slots, bool):
            slots = [slots]
        slots = [self._slot(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise ValueError("a slot is listed twice")
        if isinstance(end_seconds, dict):
            end_of = {self._slot(s): float(v) for s, v in end_seconds.items()}
        elif end_seconds is None or np.ndim(end_seconds) == 0:
            end_of = {s: 0.0 if end_seconds is None else float(end_seconds) for s in slots}
        else:
            if len(end_seconds) != len(slots):
                raise ValueError("%d end_seconds for %d slots" % (len(end_seconds), len(slots)))
            end_of = {s: float(v) for s, v in zip(slots, end_seconds)}
        slots = sorted(slots)
        cap = self._capacity(capacity, min(max(len(slots), 1), _ffi.MAX_VARLEN_CLIPS))
        parts = []
        for b0 in range(0, len(slots), _ffi.MAX_VARLEN_CLIPS):
            batch = slots[b0:b0 + _ffi.MAX_VARLEN_CLIPS]
            c_slot = (ctypes.c_int * len(batch))(*batch)
            c_end = (ctypes.c_double * len(batch))(*[end_of.get(s, 0.0) for s in batch])
            ends = {}
            for s in batch:
                n = self.steps(s)
                e = end_of.get(s, 0.0)
                ends[s] = (n, e if e > 0.0 else float(np.float64(n) * self.step))

            def call(table, c, count, status, stream, c_slot=c_slot, c_end=c_end, n=len(batch)):
                _ffi.check(_ffi.lib().acx_event_stream_close(self._h, c_slot, c_end, n, table, c, count, status, stream))
            parts.append(self._part(batch, cap, call, ends))
            self._open.difference_update(batch)
        if not parts:
            dev = self.device
            meta = torch.zeros(4, dtype=torch.int32, device=dev)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            parts = [dict(slots=[], issue=None, ends=None, table=torch.zeros((1, _ffi.EVENT_BYTES // 4), dtype=torch.int32, device=dev),
                          meta=meta, count=meta[:2].view(torch.int64), status=meta[2:3], seen=torch.zeros(4, dtype=torch.int32),
                          done=done)]
        return self._result(parts)

    def open_begin(self, slots=None):
        """(n, N) int32 on the device: per slot (default: all) and class the step at which the event the class is inside of
        began -- an open run that has reached `threshold` -- or -1.  Runs on the current stream without synchronising."""
        torch = _torch()
        slots = list(range(self.slots)) if slots is None else [self._slot(s) for s in slots]
        self._enter()
        out = torch.empty((len(slots), self.classes), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for b0 in range(0, len(slots), _ffi.MAX_VARLEN_CLIPS):
                batch = slots[b0:b0 + _ffi.MAX_VARLEN_CLIPS]
                arr = (ctypes.c_int * len(batch))(*batch)
                _ffi.check(_ffi.lib().acx_event_stream_open(self._h, arr, len(batch), out[b0:b0 + len(batch)].data_ptr(),
                                                            _ffi.stream_ptr(self.device)))
        return out

    def steps(self, slot):
        """Raw rows of the slot's open recording (host only)."""
        n = ctypes.c_int64()
        _ffi.check(_ffi.lib().acx_event_stream_steps(self._h, self._slot(slot), ctypes.byref(n)))
        return n.value


def join_event_tables(tables):
    """One table of several calls of one EventStream, in the order given (each part stays ordered (slot, cls, begin))."""
    tables = list(tables)
    owner = tables[0]._owner
    joined = _StreamEvents(owner, [p for t in tables for p in t._parts])
    if owner._pending in tables:
        owner._pending = joined
    return joined


# ---- pooling segment logits into clip probabilities (acx_segment_pool) ---------------------------------------------------------
def _pool_clips(logits, steps):
    """The (rows, N) view of segment logits and the rows per clip: logits (B, S, N) or (S, N) with steps=None, or packed
    (sum(steps), N) rows with one count per clip."""
    torch = _torch()
    if not isinstance(logits, torch.Tensor) or logits.dim() not in (2, 3) or logits.shape[-1] < 1:
        raise ValueError("pool_segments expects (B, S, N) or (rows, N) logits (got %s)" % (getattr(logits, "shape", type(logits)),))
    if steps is None:
        if logits.dim() == 2:
            logits = logits[None]
        lens = [int(logits.shape[1])] * int(logits.shape[0])
        logits = logits.reshape(-1, logits.shape[-1])
    else:
        lens = [int(n) for n in (steps.tolist() if hasattr(steps, "tolist") else steps)]
        if logits.dim() != 2 or not lens or min(lens) < 0 or sum(lens) != logits.shape[0]:
            raise ValueError("steps=%r do not add up to the %r packed rows" % (lens, tuple(logits.shape)))
    if not lens or not 1 <= logits.shape[1] <= _ffi.MAX_CLASSES:
        raise ValueError("pool_segments needs at least one clip and 1 .. %d classes" % _ffi.MAX_CLASSES)
    return logits, lens


def pool_segments(logits, pooling="max", steps=None):
    """Segment logits -> clip probabilities (clips, N) on the GPU, as finetune.fit_sed_head pools them while it trains
    (acx_segment_pool: the bits of the training pass): sigmoid per segment, then over a clip's segments "max", "mean", "linear"
    (sum q^2 / sum q) or "exp" (sum q e^q / sum e^q).  logits: fp32 CUDA, (B, S, N) / (S, N), or packed (rows, N) with steps=
    the segments per clip (forward_varlen's and forward_windows' outputs); a clip without segments gives 0.  "max" equals
    forward_segments' "clipwise_output".  Runs on the current stream without synchronising."""
    torch = _torch()
    from . import _inputs
    from .finetune import check_pooling
    pool = check_pooling(pooling)
    logits, lens = _pool_clips(logits, steps)
    if not logits.is_cuda or logits.dtype != torch.float32:
        raise ValueError("pool_segments runs on fp32 CUDA (HIP) tensors (got %s on %s); pool_segments_host takes any"
                         % (logits.dtype, logits.device))
    logits = _inputs.rows(logits)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(logits.device)
    out = torch.empty((len(lens), logits.shape[1]), dtype=torch.float32, device=logits.device)
    status = torch.zeros(1, dtype=torch.int32, device=logits.device)
    with torch.cuda.device(logits.device):
        _ffi.segment_pool(_ffi.vp(logits), logits.stride(0), _ffi.vp(off), len(lens), logits.shape[1], pool, _ffi.vp(out),
                          _ffi.vp(status), _ffi.stream_ptr(logits.device))
    return out


def pool_segments_host(logits, pooling="max", steps=None):
    """pool_segments' definition in float64 torch on the CPU (finetune.mil_forward_host) -> (clips, N) float64."""
    torch = _torch()
    from .finetune import mil_forward_host
    logits, lens = _pool_clips(torch.as_tensor(logits), steps)
    return mil_forward_host(logits.detach().cpu().to(torch.float64), np.concatenate([[0], np.cumsum(lens)]), pooling)[0]
