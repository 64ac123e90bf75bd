"""Scoring detected sound events against annotated onsets and offsets (include/acx.h "sound event scoring", csrc/sed_score.hip):
the two standard families of sound-event-detection scores, as integer counts.

  segment-based   activity of every class on a fixed time grid (time_resolution seconds per segment);
  event-based     events matched one to one, greedily, with an onset collar and an offset collar.

event_based_metrics_host / segment_based_metrics_host are the DEFINITIONS: plain float64 on per-clip lists, written after
sed_eval's published EventBasedMetrics and SegmentBasedMetrics.  sed_eval is not a dependency and nothing here claims equality
with it; the known departures: matching is greedy only (sed_eval's default is an optimal bipartite matching), and the overall
event-based error rate is (FP + FN) / Nref without sed_eval's cross-class substitution pass.  event_based_metrics /
segment_based_metrics compute the same counts on the GPU from a ReferenceEvents and an EventTable that never leave the device; every
output is an integer and equals the host definition's.  SedScores turns counts into precision, recall, F1 and error rates, in
one place for both.  sweep_event_thresholds decodes and scores a grid of thresholds on the device and picks each class's best."""
import ctypes
import math

import numpy as np

from .. import _ffi
from . import segments as _seg
from .metrics import _ratio

_REF_DTYPE = np.dtype([("clip", "<i4"), ("cls", "<i4"), ("onset", "<f8"), ("offset", "<f8")])
_SCORE_ARGS = {"event": ("t_collar", "percentage_of_length", "evaluate_onset", "evaluate_offset"), "segment": ("time_resolution",)}


def _torch():
    import torch
    return torch


def _check_classes(classes, labels):
    if isinstance(classes, bool) or not isinstance(classes, (int, np.integer)) or not 1 <= classes <= _ffi.MAX_CLASSES:
        raise ValueError("classes must be an integer in [1, %d] (got %r)" % (_ffi.MAX_CLASSES, classes))
    if labels is not None and len(labels) != classes:
        raise ValueError("%d labels for %d classes" % (len(labels), classes))
    return int(classes)


def _rows(per_clip, classes, labels=None, what="reference"):
    """per_clip[i]: [(class, onset_s, offset_s, ...), ...] -> [(clip, cls, onset, offset), ...] sorted by that tuple, the order of
    the device tables.  class: an index in [0, classes) or one of `labels`; fields after the third are ignored.  A bad entry
    raises a ValueError that names the clip and the entry."""
    index = {} if labels is None else {l: c for c, l in enumerate(labels)}
    rows = []
    for i, events in enumerate(per_clip):
        for k, ev in enumerate(events):
            where = "%s clip %d, entry %d (%r)" % (what, i, k, ev)
            try:
                name, on, off = ev[0], float(ev[1]), float(ev[2])
            except (TypeError, ValueError, IndexError):
                raise ValueError("%s: expected (class, onset_s, offset_s, ...)" % where) from None
            if not isinstance(name, (bool, np.bool_)) and isinstance(name, (int, np.integer)) and name not in index:
                cls = int(name)
                if not 0 <= cls < classes:
                    raise ValueError("%s: class %d is outside [0, %d)" % (where, cls, classes))
            elif name in index:
                cls = index[name]
            else:
                raise ValueError("%s: class %r is neither an index nor one of the labels" % (where, name))
            if not (math.isfinite(on) and math.isfinite(off)):
                raise ValueError("%s: onset and offset must be finite" % where)
            if not 0.0 <= on < off:
                raise ValueError("%s: expected 0 <= onset < offset" % where)
            rows.append((i, cls, on, off))
    rows.sort()
    return rows


def _lists(rows, clips, labels):
    """rows (clip, cls, onset, offset) -> one list per clip of (class, onset_s, offset_s) sorted like decode_events' output."""
    out = [[] for _ in range(clips)]
    for clip, cls, on, off in rows:
        out[clip].append((labels[cls] if labels is not None else cls, on, off))
    for events in out:
        events.sort(key=lambda ev: (ev[1], ev[2], str(ev[0])))
    return out


class ReferenceEvents:
    """The annotated events of a batch: rows (clip, cls, onset_s, offset_s) ordered by that tuple, float64 seconds -- on the host
    (`rows`) and, when a device is given, as one (n, 24-byte) table of acx_ref_event rows there (`table`, uploaded once)."""

    def __init__(self, rows, clips, classes, labels=None, device=None):
        self.rows, self.clips, self.classes, self.labels = rows, clips, classes, labels
        self.table = None
        if device is not None:
            torch = _torch()
            host = np.zeros(max(len(rows), 1), dtype=_REF_DTYPE)
            if rows:
                host[:len(rows)] = rows
            self.table = torch.from_numpy(host.view(np.uint8).reshape(-1, _ffi.REF_EVENT_BYTES)).to(device)

    @classmethod
    def from_lists(cls, per_clip, classes, labels=None, device=None):
        """per_clip[i]: the events of clip i as (class, onset_s, offset_s, ...) -- class an index or one of `labels`; further
        fields are ignored, so EventTable.to_lists() and decode_events output pass as they are.  Events of one class may overlap.
        Validated on the host (ValueError naming the clip and the entry: non-finite values, onset >= offset, an unknown class),
        sorted, and uploaded once when `device` is given."""
        classes = _check_classes(classes, labels)
        return cls(_rows(per_clip, classes, labels), len(per_clip), classes, labels, device)

    def __len__(self):
        return len(self.rows)

    def to_lists(self):
        """One list per clip of (class, onset_s, offset_s), sorted by (onset, offset, str(class)); class is labels[c] when the
        table was made with labels, else c."""
        return _lists(self.rows, self.clips, self.labels)


class SedScores:
    """Counts of one scoring and what follows from them.  counts: (N, 3) int64 = TP, FP, FN per class; segment-based scores add
    overall (6,) int64 = TP, S, D, I, Nref, Nsys; event-based ones ref_match (n_ref,) and est_match (rows of the table,) int64:
    the row matched in the other table, or -1.  They are device tensors from the GPU functions (nothing has synchronised yet) and
    numpy arrays from the host definitions.  Everything derived is float64 numpy computed on the host from the counts: a
    precision, recall or F1 without a denominator is 0.0 (metrics._ratio, sklearn's zero_division=0); an error rate is
    (FN + FP) / Nref and NaN where Nref == 0."""

    def __init__(self, kind, counts, overall=None, ref_match=None, est_match=None, status=None, events=None, reference=None):
        self.kind, self.counts, self.overall, self.ref_match, self.est_match = kind, counts, overall, ref_match, est_match
        self.status, self.events, self.reference = status, events, reference
        self._host = None

    def check(self):
        """Waits for the scoring.  ValueError when the event table was not usable as it was scored: decoded from non-finite
        probabilities or bad per-class levels, or too small for its events (events.check() decodes such a table again; score it
        after that).  Returns self."""
        if self._host is None:
            if self.status is not None and int(self.status.cpu()) & _ffi.SCORE_BAD_TABLE:
                raise ValueError("the event table was not usable when it was scored (it overflowed, or the decoder rejected its "
                                 "input): call events.check() before scoring")
            host = lambda v: None if v is None else v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)   # noqa: E731
            self._host = (host(self.counts), host(self.overall))
        return self

    def counts_host(self):
        """counts as an int64 numpy array (N, 3)."""
        return self.check()._host[0]

    def overall_host(self):
        """overall as an int64 numpy array (6,) (segment-based scores only)."""
        if self.overall is None:
            raise ValueError("only segment-based scores have overall counts")
        return self.check()._host[1]

    @staticmethod
    def _derive(tp, fp, fn):
        tp, fp, fn = (np.asarray(v, np.float64) for v in (tp, fp, fn))
        nref = tp + fn
        with np.errstate(invalid="ignore", divide="ignore"):
            er = np.where(nref > 0, (fn + fp) / nref, np.nan)
        return {"precision": _ratio(tp, tp + fp), "recall": _ratio(tp, nref), "f1": _ratio(2.0 * tp, 2.0 * tp + fp + fn),
                "error_rate": er}

    def classwise(self):
        """{"precision", "recall", "f1", "error_rate"}: float64 arrays of one value per class."""
        return self._derive(*self.counts_host().T)

    precision = property(lambda self: self.classwise()["precision"])
    recall = property(lambda self: self.classwise()["recall"])
    f1 = property(lambda self: self.classwise()["f1"])
    error_rate = property(lambda self: self.classwise()["error_rate"])

    def micro(self):
        """The four numbers from the counts summed over the classes (floats)."""
        return {k: float(v) for k, v in self._derive(*self.counts_host().sum(axis=0)).items()}

    def macro(self):
        """Their means over the classes with Nref > 0 (NaN when there is none)."""
        c = self.counts_host()
        seen = (c[:, 0] + c[:, 2]) > 0
        return {k: float(v[seen].mean()) if seen.any() else float("nan") for k, v in self.classwise().items()}

    @property
    def overall_error_rate(self):
        """Segment-based: (S + D + I) / Nref over all segments; event-based: (FP + FN) / Nref (no substitutions)."""
        if self.overall is None:
            return self.micro()["error_rate"]
        tp, s, d, i, nref, nsys = (float(v) for v in self.overall_host())
        return (s + d + i) / nref if nref > 0 else float("nan")


# ---- the definitions ---------------------------------------------------------------------------------------------------------

def _check_collar(t_collar, percentage_of_length):
    for name, v in (("t_collar", t_collar), ("percentage_of_length", percentage_of_length)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (math.isfinite(v) and v >= 0):
            raise ValueError("%s must be a finite number >= 0 (got %r)" % (name, v))
    return float(t_collar), float(percentage_of_length)


def _check_resolution(time_resolution):
    v = time_resolution
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (math.isfinite(v) and v > 0):
        raise ValueError("time_resolution must be a finite number > 0 (got %r)" % (v,))
    return float(v)


def event_based_metrics_host(reference, estimated, classes, t_collar=0.2, percentage_of_length=0.5, evaluate_onset=True,
                             evaluate_offset=True, labels=None):
    """The definition of the event-based counts.  reference / estimated: one list per clip of (class, onset_s, offset_s, ...).
    Both are put in table order, (clip, cls, onset, offset).  Per (clip, cls), the reference events in that order: each takes
    the first estimated event, in that order, that no earlier one took and that passes
        abs(r_on - e_on) <= t_collar                                                    (unless evaluate_onset is off) and
        abs(r_off - e_off) <= max(t_collar, percentage_of_length * (r_off - r_on))      (unless evaluate_offset is off),
    in float64.  Per class TP = the pairs, FP = estimated - TP, FN = reference - TP.  Returns SedScores with numpy counts (N, 3),
    ref_match and est_match (row numbers in table order, -1: unmatched).
    After sed_eval's EventBasedMetrics with greedy matching; NOT offered: its optimal bipartite matching (its default), and the
    cross-class substitutions of its overall error rate -- overall_error_rate here is (FP + FN) / Nref."""
    classes = _check_classes(classes, labels)
    t_collar, pct = _check_collar(t_collar, percentage_of_length)
    if len(reference) != len(estimated):
        raise ValueError("%d reference clips and %d estimated ones" % (len(reference), len(estimated)))
    ref = _rows(reference, classes, labels)
    est = _rows(estimated, classes, labels, "estimated")
    ref_match = np.full(len(ref), -1, np.int64)
    est_match = np.full(len(est), -1, np.int64)
    columns = {}
    for j, row in enumerate(est):
        columns.setdefault(row[:2], []).append(j)
    for i, (clip, cls, r_on, r_off) in enumerate(ref):
        tol = max(t_collar, pct * (r_off - r_on))
        for j in columns.get((clip, cls), ()):
            if est_match[j] >= 0:
                continue
            if evaluate_onset and not abs(r_on - est[j][2]) <= t_collar:
                continue
            if evaluate_offset and not abs(r_off - est[j][3]) <= tol:
                continue
            ref_match[i], est_match[j] = j, i
            break
    n_ref = np.bincount([r[1] for r in ref], minlength=classes).astype(np.int64)
    n_est = np.bincount([e[1] for e in est], minlength=classes).astype(np.int64)
    tp = np.bincount([r[1] for r, m in zip(ref, ref_match) if m >= 0], minlength=classes).astype(np.int64)
    return SedScores("event", np.stack([tp, n_est - tp, n_ref - tp], axis=1), ref_match=ref_match, est_match=est_match)


def segment_based_metrics_host(reference, estimated, ends, classes, time_resolution=1.0, labels=None):
    """The definition of the segment-based counts.  reference / estimated: one list per clip of (class, onset_s, offset_s, ...);
    ends: the clips' ends in seconds (one number: every clip's).  Clip i has ceil(end_i / time_resolution) segments; an event is
    active in segments [floor(onset / res), ceil(offset / res)) clipped to the clip (float64); per segment and class, reference
    and estimated activity are the unions of the events.  Per class over all segments and clips TP = sum(ref & est),
    FP = sum(est & ~ref), FN = sum(ref & ~est); per segment, with fn / fp its totals over the classes, S = min(fn, fp),
    D = max(0, fn - fp), I = max(0, fp - fn).  Returns SedScores with numpy counts (N, 3) and overall (6,) = TP, S, D, I, Nref, Nsys
    summed over segments and clips.  After sed_eval's SegmentBasedMetrics."""
    classes = _check_classes(classes, labels)
    res = _check_resolution(time_resolution)
    if len(reference) != len(estimated):
        raise ValueError("%d reference clips and %d estimated ones" % (len(reference), len(estimated)))
    B = len(reference)
    ends = [float(ends)] * B if np.ndim(ends) == 0 else [float(e) for e in ends]
    if len(ends) != B:
        raise ValueError("%d ends for %d clips" % (len(ends), B))
    tables = []
    for rows in (_rows(reference, classes, labels), _rows(estimated, classes, labels, "estimated")):
        by_clip = [{} for _ in range(B)]
        for clip, cls, on, off in rows:
            by_clip[clip].setdefault(cls, []).append((on, off))
        tables.append(by_clip)
    counts = np.zeros((classes, 3), np.int64)
    overall = np.zeros(6, np.int64)
    for i in range(B):
        nseg = max(int(math.ceil(ends[i] / res)), 0)
        fn_seg, fp_seg = np.zeros(nseg, np.int64), np.zeros(nseg, np.int64)
        for cls in sorted(set(tables[0][i]) | set(tables[1][i])):
            act = []
            for t in tables:
                a = np.zeros(nseg, bool)
                for on, off in t[i].get(cls, ()):
                    a[min(max(int(math.floor(on / res)), 0), nseg):min(max(int(math.ceil(off / res)), 0), nseg)] = True
                act.append(a)
            r, e = act
            tp, fp, fn = r & e, e & ~r, r & ~e
            counts[cls] += (tp.sum(), fp.sum(), fn.sum())
            fn_seg += fn
            fp_seg += fp
            overall[0] += tp.sum()
            overall[4] += r.sum()
            overall[5] += e.sum()
        overall[1] += np.minimum(fn_seg, fp_seg).sum()
        overall[2] += np.maximum(fn_seg - fp_seg, 0).sum()
        overall[3] += np.maximum(fp_seg - fn_seg, 0).sum()
    return SedScores("segment", counts, overall=overall)


# ---- the same counts on the device --------------------------------------------------------------------------------------------

def _clip_arrays(events):
    """(steps int32 (B,), end_seconds float64 (B,), step_seconds) of an EventTable, the arrays on its device: uploaded once per
    table from pinned memory, without waiting for the stream."""
    cached = getattr(events, "_score_clips", None)
    dev = events.table.device
    if cached is None or cached[0].device != dev:
        torch = _torch()
        steps = [len(e) - 1 for e in events.edges]
        step_s = next((float(e[1]) for e in events.edges if len(e) > 2), 1.0)      # one-step clips: no boundary reads it
        put = lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)   # noqa: E731
        cached = (put(np.asarray(steps, np.int32)), put(np.asarray([float(e[-1]) for e in events.edges], np.float64)), step_s)
        events._score_clips = cached
    return cached


def _check_pair(reference, events):
    if not isinstance(reference, ReferenceEvents) or not isinstance(events, _seg.EventTable):
        raise ValueError("expected a ReferenceEvents and an EventTable (got %s, %s); the *_host functions take lists"
                         % (type(reference).__name__, type(events).__name__))
    if reference.table is None:
        raise ValueError("the reference events are on the host: make them with ReferenceEvents.from_lists(..., device=...)")
    if reference.table.device != events.table.device:
        raise ValueError("the reference events lie on %s, the event table on %s" % (reference.table.device, events.table.device))
    if reference.clips != len(events.edges) or reference.classes != events.classes:
        raise ValueError("reference events of %d clips and %d classes for a table of %d clips and %d classes"
                         % (reference.clips, reference.classes, len(events.edges), events.classes))


def _table_args(reference, events):
    steps, ends, step_s = _clip_arrays(events)
    return (reference.table.data_ptr(), len(reference), events.table.data_ptr(), events.capacity, events.count.data_ptr(),
            events.status.data_ptr(), len(events.edges), events.classes, steps.data_ptr(), ends.data_ptr(), step_s)


def event_based_metrics(reference, events, t_collar=0.2, percentage_of_length=0.5, evaluate_onset=True, evaluate_offset=True):
    """event_based_metrics_host on the GPU (acx_score_events): reference, a ReferenceEvents on the table's device; events, an
    EventTable as decode_events_gpu / detect_events left it -- its valid length is read on the device.  Runs on the current
    stream without synchronising.  Returns SedScores with device counts (N, 3), ref_match (n_ref,) and est_match (capacity,),
    all int64 and equal to the host definition's; its derived numbers and check() wait, and raise when the table was unusable."""
    _check_pair(reference, events)
    t_collar, pct = _check_collar(t_collar, percentage_of_length)
    torch = _torch()
    dev = events.table.device
    collar = _ffi.event_collar(t_collar, pct, evaluate_onset, evaluate_offset)
    with torch.cuda.device(dev):
        counts = torch.empty((events.classes, 3), dtype=torch.int64, device=dev)
        ref_match = torch.empty(len(reference), dtype=torch.int64, device=dev)
        est_match = torch.empty(events.capacity, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _ffi.check(_ffi.lib().acx_score_events(*_table_args(reference, events), ctypes.byref(collar), counts.data_ptr(),
                                               ref_match.data_ptr() if len(reference) else None, est_match.data_ptr(),
                                               status.data_ptr(), _ffi.stream_ptr(dev)))
    return SedScores("event", counts, ref_match=ref_match, est_match=est_match, status=status, events=events, reference=reference)


def segment_based_metrics(reference, events, time_resolution=1.0):
    """segment_based_metrics_host on the GPU (acx_score_segments), the clips' ends taken from events.edges.  Runs on the current
    stream without synchronising.  Returns SedScores with device counts (N, 3) and overall (6,), int64, equal to the host
    definition's."""
    _check_pair(reference, events)
    res = _check_resolution(time_resolution)
    torch = _torch()
    dev = events.table.device
    with torch.cuda.device(dev):
        counts = torch.empty((events.classes, 3), dtype=torch.int64, device=dev)
        overall = torch.empty(6, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _ffi.check(_ffi.lib().acx_score_segments(*_table_args(reference, events), res, counts.data_ptr(), overall.data_ptr(),
                                                 status.data_ptr(), _ffi.stream_ptr(dev)))
    return SedScores("segment", counts, overall=overall, status=status, events=events, reference=reference)


def _scorer(metric, args):
    """(function, its arguments taken out of args) for metric "event" / "segment"."""
    if metric not in _SCORE_ARGS:
        raise ValueError('metric must be "event" or "segment" (got %r)' % (metric,))
    own = {k: args.pop(k) for k in _SCORE_ARGS[metric] if k in args}
    other = [k for k in args if k in _SCORE_ARGS["segment" if metric == "event" else "event"]]
    if other:
        raise TypeError("%s belongs to the other metric, not to metric=%r" % (", ".join(other), metric))
    return (event_based_metrics if metric == "event" else segment_based_metrics), own


def best_f1_thresholds(thresholds, counts):
    """thresholds (T,) float32 and counts (T, N, 3) = TP, FP, FN, device tensors -> (N,) float32: per class the threshold of the
    best F1 = 2 TP / (2 TP + FP + FN) (float64; 0 without a denominator), ties to the smallest threshold, +inf for a class
    without reference events (TP + FN == 0)."""
    torch = _torch()
    c = counts.to(torch.float64)
    den = 2.0 * c[..., 0] + c[..., 1] + c[..., 2]
    f1 = torch.where(den > 0, 2.0 * c[..., 0] / den.clamp(min=1.0), torch.zeros_like(den))
    best = f1.max(dim=0, keepdim=True).values
    inf = torch.full_like(f1, float("inf"), dtype=torch.float32)
    pick = torch.where(f1 == best, thresholds.to(torch.float32)[:, None].expand_as(f1), inf).min(dim=0).values
    seen = (counts[0, :, 0] + counts[0, :, 2]) > 0
    return torch.where(seen, pick, inf[0])


def sweep_event_thresholds(probs, reference, thresholds, metric="event", **decode_and_score_args):
    """Per-class thresholds by event-level F1.  For every value of the 1-D `thresholds` (rounded to float32, what the decoder
    compares in): decode_events_gpu(probs, threshold=value, ...) and the scorer of `metric`, everything queued on the current
    stream; then per class the threshold of the best F1, ties to the smallest, +inf for a class without reference events (the
    decoder reads it as "emit nothing").  decode_and_score_args: decode_events_gpu's (low, median, min_duration, merge_gap,
    step, steps, capacity) and the scorer's (t_collar, ... / time_resolution).  A table that overflowed is decoded again through
    EventTable.check() and scored again; that is the only synchronisation.  Returns (threshold (N,) float32 device tensor --
    an argument for detect_events(threshold=...) --, counts (T, N, 3) int64 device tensor in the order of `thresholds`)."""
    torch = _torch()
    args = dict(decode_and_score_args)
    if "threshold" in args:
        raise TypeError("the sweep sets threshold itself")
    score, score_args = _scorer(metric, args)
    thr = np.asarray(thresholds, dtype=np.float32)
    if thr.ndim != 1 or thr.size == 0 or not np.all(np.isfinite(thr)):
        raise ValueError("thresholds must be a non-empty 1-D array of finite numbers")
    tables = [_seg.decode_events_gpu(probs, threshold=float(t), **args) for t in thr]
    _check_pair(reference, tables[0])
    clips = _clip_arrays(tables[0])
    for t in tables[1:]:
        t._score_clips = clips                           # one geometry: one upload
    scores = [score(reference, t, **score_args) for t in tables]
    bad = torch.stack([s.status for s in scores]).cpu().numpy().ravel()
    for i in np.nonzero(bad & _ffi.SCORE_BAD_TABLE)[0]:
        tables[i].check()                                # decodes an overflowed table again; raises for unusable input
        scores[i] = score(reference, tables[i], **score_args)
    counts = torch.stack([s.counts for s in scores])
    return best_f1_thresholds(torch.from_numpy(thr).to(counts.device), counts), counts
