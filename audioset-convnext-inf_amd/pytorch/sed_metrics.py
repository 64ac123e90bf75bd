"""Scoring detected sound events against annotated onsets and offsets (include/acx.h "sound event scoring", csrc/sed_score.hip):
the three standard families of sound-event-detection scores, as integer counts, and the PSDS built on the third.

  segment-based   activity of every class on a fixed time grid (time_resolution seconds per segment);
  event-based     events matched one to one, greedily, with an onset collar and an offset collar;
  intersection    events judged by how much of their length intersects the other side, without collars: a detection by the
                  annotations of its class (DTC), an annotation by the relevant detections (GTC), a false positive by the
                  annotations of other classes (CTTC, the cross-trigger matrix).

event_based_metrics_host / segment_based_metrics_host / intersection_based_metrics_host are the DEFINITIONS: plain float64 on
per-clip lists.  The first two are written after sed_eval's published EventBasedMetrics and SegmentBasedMetrics, the third and
psds_host / psd_roc_host after the polyphonic sound detection score of Bilen et al. (ICASSP 2020).  Neither sed_eval nor
psds_eval is a dependency and nothing here claims equality with them; the known departures: matching is greedy only
(sed_eval's default is an optimal bipartite matching), the overall event-based error rate is (FP + FN) / Nref without sed_eval's
cross-class substitution pass, and the choices of the intersection family and of PSDS are listed in their docstrings as this
project's own.  event_based_metrics / segment_based_metrics / intersection_based_metrics compute the same counts on the GPU from
a ReferenceEvents and an EventTable that never leave the device; every output is an integer and equals the host definition's.
SedScores turns counts into precision, recall, F1 and error rates, in one place for all three.  sweep_event_thresholds decodes
and scores a grid of thresholds on the device and picks each class's best; psds decodes and scores a grid the same way and
integrates the PSD-ROC over it."""
import ctypes
import math

import numpy as np

from .. import _ffi
from . import segments as _seg
from .metrics import _ratio

_REF_DTYPE = np.dtype([("clip", "<i4"), ("cls", "<i4"), ("onset", "<f8"), ("offset", "<f8")])
_SCORE_ARGS = {"event": ("t_collar", "percentage_of_length", "evaluate_onset", "evaluate_offset"), "segment": ("time_resolution",),
               "intersection": ("dtc_threshold", "gtc_threshold", "cttc_threshold")}
# the two evaluation scenarios of DCASE task 4, per hour of audio
PSDS_SCENARIOS = {"dcase_1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0.0, alpha_st=1.0, max_efpr=100.0),
                  "dcase_2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1.0, max_efpr=100.0)}
MAX_CROSS_TRIGGER_CLASSES = 4096      # an (N, N) int64 matrix: 134 MB at this size


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
    """Counts of one scoring and what follows from them.  kind: "event", "segment" or "intersection".  counts: (N, 3) int64 =
    TP, FP, FN per class; segment-based scores add overall (6,) int64 = TP, S, D, I, Nref, Nsys; event-based ones ref_match
    (n_ref,) and est_match (rows of the table,) int64: the row matched in the other table, or -1; intersection-based ones
    est_relevant (rows of the table,) and ref_hit (n_ref,) int64, 1 or 0 (-1 behind the valid rows of a device table), and with a
    cttc_threshold cross_triggers (N, N) int64, row = the detected class.  In that family a relevant detection whose annotation
    fails GTC is neither a TP nor an FP: TP + FP is not the number of detections, and precision and F1 inherit that.  They are
    device tensors from the GPU functions (nothing has synchronised yet) and
    numpy arrays from the host definitions.  Everything derived is float64 numpy computed on the host from the counts: a
    precision, recall or F1 without a denominator is 0.0 (metrics._ratio, sklearn's zero_division=0); an error rate is
    (FN + FP) / Nref and NaN where Nref == 0."""

    def __init__(self, kind, counts, overall=None, ref_match=None, est_match=None, status=None, events=None, reference=None,
                 cross_triggers=None, est_relevant=None, ref_hit=None):
        self.kind, self.counts, self.overall, self.ref_match, self.est_match = kind, counts, overall, ref_match, est_match
        self.status, self.events, self.reference = status, events, reference
        self.cross_triggers, self.est_relevant, self.ref_hit = cross_triggers, est_relevant, ref_hit
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
        """Segment-based: (S + D + I) / Nref over all segments; event- and intersection-based: (FP + FN) / Nref (no
        substitutions)."""
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


def _check_ratio(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (math.isfinite(v) and 0 < v <= 1):
        raise ValueError("%s must be a finite number in (0, 1] (got %r)" % (name, v))
    return float(v)


def _check_criteria(dtc_threshold, gtc_threshold, cttc_threshold):
    return (_check_ratio("dtc_threshold", dtc_threshold), _check_ratio("gtc_threshold", gtc_threshold),
            None if cttc_threshold is None else _check_ratio("cttc_threshold", cttc_threshold))


def _cover(a, b, rows):
    """The length of [a, b) that the union of rows (onset, offset), ascending in onset, covers: a float64 sum in row order.
    csrc/sed_score.hip::sc_cover_row holds the same three lines."""
    covered, total = a, 0.0
    for on, off in rows:
        if on >= b:
            break
        lo, hi = max(on, covered), min(off, b)
        if hi > lo:
            total += hi - lo
            covered = hi
    return total


def intersection_based_metrics_host(reference, estimated, classes, dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None,
                                    labels=None):
    """The definition of the intersection-based counts, the operating point that PSDS integrates.  reference / estimated: one
    list per clip of (class, onset_s, offset_s, ...), put in table order (clip, cls, onset, offset).  All in float64;
    cover(a, b, rows) is the length of [a, b) that the union of the rows covers (_cover), and a criterion with ratio rho holds
    when cover >= rho * (b - a): one product, no division.  Per (clip, class c):
      DTC   a detection d is relevant when cover(d, the annotations of (clip, c)) >= dtc_threshold * len(d);
      FP    a detection that is not relevant is a false positive of class c;
      GTC   an annotation g is a TP when cover(g, the relevant detections of (clip, c)) >= gtc_threshold * len(g), else an FN;
      CTTC  (with cttc_threshold) for each FP d of class c and each class k != c with annotations in the clip,
            cover(d, the annotations of (clip, k)) >= cttc_threshold * len(d) adds 1 to cross_triggers[c, k].
    Returns SedScores of kind "intersection" with numpy counts (N, 3) = TP, FP, FN, est_relevant (rows,) and ref_hit (n_ref,)
    (1 / 0, rows in table order), and cross_triggers (N, N), row = the detected class, or None.
    This project's own choices, after Bilen et al. (ICASSP 2020), not psds_eval's code: annotations of one class may overlap and
    count by their UNION, never twice; a relevant detection whose annotation fails GTC is NEITHER a TP nor an FP (so TP + FP is
    not the number of detections, and precision and F1 of these counts inherit that); relevant detections never cross-trigger;
    the diagonal of cross_triggers stays 0; a tie cover == rho * length passes."""
    classes = _check_classes(classes, labels)
    dtc, gtc, cttc = _check_criteria(dtc_threshold, gtc_threshold, cttc_threshold)
    if len(reference) != len(estimated):
        raise ValueError("%d reference clips and %d estimated ones" % (len(reference), len(estimated)))
    ref = _rows(reference, classes, labels)
    est = _rows(estimated, classes, labels, "estimated")
    ref_cols, est_cols, clip_classes = {}, {}, {}
    for i, row in enumerate(ref):
        ref_cols.setdefault(row[:2], []).append(i)
        if row[1] not in clip_classes.setdefault(row[0], []):
            clip_classes[row[0]].append(row[1])                 # ascending: the rows are sorted
    for j, row in enumerate(est):
        est_cols.setdefault(row[:2], []).append(j)
    counts = np.zeros((classes, 3), np.int64)
    cross = None if cttc is None else np.zeros((classes, classes), np.int64)
    est_relevant = np.zeros(len(est), np.int64)
    ref_hit = np.zeros(len(ref), np.int64)
    for j, (clip, cls, on, off) in enumerate(est):
        if _cover(on, off, [ref[i][2:] for i in ref_cols.get((clip, cls), ())]) >= dtc * (off - on):
            est_relevant[j] = 1
            continue
        counts[cls, 1] += 1
        if cross is not None:
            for k in clip_classes.get(clip, ()):
                if k != cls and _cover(on, off, [ref[i][2:] for i in ref_cols[clip, k]]) >= cttc * (off - on):
                    cross[cls, k] += 1
    for i, (clip, cls, on, off) in enumerate(ref):
        relevant = [est[j][2:] for j in est_cols.get((clip, cls), ()) if est_relevant[j]]
        ref_hit[i] = 1 if _cover(on, off, relevant) >= gtc * (off - on) else 0
        counts[cls, 0 if ref_hit[i] else 2] += 1
    return SedScores("intersection", counts, cross_triggers=cross, est_relevant=est_relevant, ref_hit=ref_hit)


# ---- PSDS: the area under the PSD-ROC of a threshold sweep ----------------------------------------------------------------

def psds_durations(reference, ends, classes=None, labels=None):
    """(total_seconds, class_seconds (N,)) for psds_host: math.fsum of the clips' ends, and per class math.fsum(offset - onset)
    over its annotations.  reference: a ReferenceEvents, or per-clip lists with `classes` (and labels)."""
    rows = reference.rows if isinstance(reference, ReferenceEvents) else _rows(reference, _check_classes(classes, labels), labels)
    n = reference.classes if isinstance(reference, ReferenceEvents) else classes
    per_class = [[] for _ in range(n)]
    for _, cls, on, off in rows:
        per_class[cls].append(off - on)
    return math.fsum(float(e) for e in ends), np.array([math.fsum(v) for v in per_class], np.float64)


def cross_trigger_weights(class_seconds, unit_seconds=3600.0):
    """weight[k] = unit_seconds / class_seconds[k], 0 where class k has no annotated time: cross triggers per unit of class k's
    annotated time, the weights of cross_trigger_rate_host and acx_cross_trigger_rate."""
    cs = np.asarray(class_seconds, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cs > 0, float(unit_seconds) / cs, 0.0)


def cross_trigger_rate_host(cross_triggers, weight):
    """(..., N, N) int64 and (N,) float64 -> (..., N) float64: rate[c] = the mean over k != c with weight[k] > 0 of
    cross_triggers[c, k] * weight[k], summed in ascending k as ONE sequential float64 sum (a loop, not np.sum, which adds in
    pairs), 0 when no such k exists.  acx_cross_trigger_rate computes the same bits."""
    ct = np.asarray(cross_triggers)
    w = np.asarray(weight, np.float64)
    N = w.shape[0]
    if ct.shape[-2:] != (N, N):
        raise ValueError("cross_triggers of shape %r for %d weights" % (ct.shape, N))
    acc = np.zeros(ct.shape[:-1], np.float64)
    used = np.zeros(N, np.int64)
    for k in range(N):
        if not w[k] > 0:
            continue
        term = ct[..., k].astype(np.float64) * w[k]
        term[..., k] = 0.0                                      # k == c is left out; acc + 0.0 is acc
        acc = acc + term
        used += np.arange(N) != k
    return np.where(used > 0, acc / np.maximum(used, 1), 0.0)


def _psd_roc(counts, rates, total_seconds, alpha_ct, alpha_st, max_efpr, unit_seconds):
    """The PSD-ROC from counts (T, N, 3) and cross-trigger rates (T, N) or None -> (value, efpr axis, etpr, class curves (N, A),
    seen (N,) bool)."""
    counts = np.asarray(counts)
    if counts.ndim != 3 or counts.shape[2] != 3 or counts.shape[0] < 1:
        raise ValueError("counts must be (T, N, 3) with T >= 1 (got %r)" % (counts.shape,))
    for name, v, low in (("total_seconds", total_seconds, False), ("max_efpr", max_efpr, False), ("unit_seconds", unit_seconds, False),
                         ("alpha_ct", alpha_ct, True), ("alpha_st", alpha_st, True)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) \
                or not (v >= 0 if low else v > 0):
            raise ValueError("%s must be a finite number %s 0 (got %r)" % (name, ">=" if low else ">", v))
    T, N = counts.shape[:2]
    nref = counts[:, :, 0] + counts[:, :, 2]
    if not (nref == nref[0]).all():
        raise ValueError("TP + FN differs between the operating points: they were not scored against one reference")
    seen = nref[0] > 0
    curves = np.full((N, 0), np.nan)
    if not seen.any():
        return float("nan"), np.zeros(0), np.zeros(0), curves, seen
    tpr = counts[:, seen, 0].astype(np.float64) / nref[0, seen].astype(np.float64)
    efpr = counts[:, seen, 1].astype(np.float64) * float(unit_seconds) / float(total_seconds)
    if alpha_ct != 0:
        if rates is None:
            raise ValueError("alpha_ct = %r needs the cross triggers (score with a cttc_threshold)" % (alpha_ct,))
        efpr = efpr + float(alpha_ct) * np.asarray(rates, np.float64)[:, seen]
    axis = np.unique(efpr[efpr <= max_efpr])
    seen_curves = np.zeros((tpr.shape[1], axis.size))
    for c in range(tpr.shape[1]):
        order = np.argsort(efpr[:, c], kind="stable")
        best = np.maximum.accumulate(tpr[order, c])             # the largest tpr among the points with efpr <= x
        at = np.searchsorted(efpr[order, c], axis, side="right") - 1
        seen_curves[c] = np.where(at >= 0, best[np.maximum(at, 0)], 0.0)
    curves = np.full((N, axis.size), np.nan)
    curves[seen] = seen_curves
    etpr = np.maximum(seen_curves.mean(axis=0) - float(alpha_st) * seen_curves.std(axis=0), 0.0)
    widths = np.diff(np.append(axis, float(max_efpr)))
    return math.fsum(etpr * widths) / float(max_efpr), axis, etpr, curves, seen


def psd_roc_host(counts, cross_triggers, total_seconds, class_seconds, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0,
                 unit_seconds=3600.0):
    """The PSD-ROC that psds_host integrates: (efpr (A,), etpr (A,), class_curves (N, A)) -- the axis, the effective true
    positive rate on it, and every class's curve (NaN rows for classes without annotations), so that a plot needs no second
    implementation.  Arguments and definitions: psds_host."""
    rates = None
    if alpha_ct != 0 and cross_triggers is not None:
        rates = cross_trigger_rate_host(cross_triggers, cross_trigger_weights(class_seconds, unit_seconds))
    return _psd_roc(counts, rates, total_seconds, alpha_ct, alpha_st, max_efpr, unit_seconds)[1:4]


def psds_host(counts, cross_triggers, total_seconds, class_seconds, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0, unit_seconds=3600.0):
    """The polyphonic sound detection score of a sweep of operating points.  counts (T, N, 3) = TP, FP, FN of
    intersection_based_metrics_host at T operating points; cross_triggers (T, N, N) or None; total_seconds: math.fsum of the
    clips' ends; class_seconds (N,): per class math.fsum(offset - onset) over its annotations (psds_durations gives both).
      nref_c = TP + FN, the same at every operating point; classes with nref_c == 0 are left out, and without any class the
      result is NaN;
      tpr[o, c] = TP / nref_c;  fpr[o, c] = FP * unit_seconds / total_seconds;
      efpr[o, c] = fpr + alpha_ct * mean_k(cross_triggers[o, c, k] * weight[k]), weight[k] = unit_seconds / class_seconds[k],
      the mean over k != c with class_seconds[k] > 0, accumulated in ascending k as one fixed-order float64 sum
      (cross_trigger_rate_host), 0 when no such k exists;
      a class's curve at x = the largest tpr among the operating points with efpr <= x, 0 when there is none;
      the axis = the sorted unique efpr values <= max_efpr over all classes and operating points (points beyond are dropped);
      etpr(x) = max(0, mean_c - alpha_st * std_c) of the curves, population std (ddof = 0);
      PSDS = sum etpr(x_i) * (x_{i+1} - x_i) / max_efpr, with max_efpr behind the last point; an empty axis gives 0.
    This project's own choices, after Bilen et al. (ICASSP 2020), not psds_eval's code: the curves are staircases (no
    interpolation between operating points), the operating points are the given thresholds and not every distinct score, and
    the cross-trigger term divides each count by the annotated time of the class it was mistaken for."""
    rates = None
    if alpha_ct != 0 and cross_triggers is not None:
        rates = cross_trigger_rate_host(cross_triggers, cross_trigger_weights(class_seconds, unit_seconds))
    return _psd_roc(counts, rates, total_seconds, alpha_ct, alpha_st, max_efpr, unit_seconds)[0]


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


def _score_intersection(reference, events, criteria, matrix=None, counts=None):
    """One acx_score_intersection call on the current stream; matrix: the (N, N) buffer of a call with criteria.cross_triggers;
    counts: a contiguous (N, 3) int64 buffer to write into."""
    torch = _torch()
    dev = events.table.device
    with torch.cuda.device(dev):
        if counts is None:
            counts = torch.empty((events.classes, 3), dtype=torch.int64, device=dev)
        ref_hit = torch.empty(len(reference), dtype=torch.int64, device=dev)
        est_relevant = torch.empty(events.capacity, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _ffi.check(_ffi.lib().acx_score_intersection(*_table_args(reference, events), ctypes.byref(criteria), counts.data_ptr(),
                                                     None if matrix is None else matrix.data_ptr(),
                                                     ref_hit.data_ptr() if len(reference) else None, est_relevant.data_ptr(),
                                                     status.data_ptr(), _ffi.stream_ptr(dev)))
    return SedScores("intersection", counts, status=status, events=events, reference=reference, cross_triggers=matrix,
                     est_relevant=est_relevant, ref_hit=ref_hit)


def _check_matrix_size(classes):
    if classes > MAX_CROSS_TRIGGER_CLASSES:
        raise ValueError("cttc_threshold with %d classes: the cross-trigger matrix is (N, N) int64, 134 MB per table at N = %d, "
                         "and is refused beyond that" % (classes, MAX_CROSS_TRIGGER_CLASSES))


def intersection_based_metrics(reference, events, dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None):
    """intersection_based_metrics_host on the GPU (acx_score_intersection), event_based_metrics' twin: runs on the current
    stream without synchronising.  Returns SedScores of kind "intersection" with device counts (N, 3), est_relevant (capacity,;
    -1 behind the valid rows), ref_hit (n_ref,) and, with a cttc_threshold, cross_triggers (N, N) -- all int64 and equal to the
    host definition's.  With a cttc_threshold N may not exceed 4096 (the matrix would pass 134 MB per table): ValueError."""
    _check_pair(reference, events)
    dtc, gtc, cttc = _check_criteria(dtc_threshold, gtc_threshold, cttc_threshold)
    matrix = None
    if cttc is not None:
        _check_matrix_size(events.classes)
        matrix = _torch().empty((events.classes, events.classes), dtype=_torch().int64, device=events.table.device)
    return _score_intersection(reference, events, _ffi.intersection_criteria(dtc, gtc, cttc), matrix)


def cross_trigger_rate(cross_triggers, weight, out=None):
    """cross_trigger_rate_host on the GPU (acx_cross_trigger_rate): cross_triggers (N, N) int64 and weight (N,) float64, CUDA
    tensors -> (N,) float64 (written into `out` when given), the same bits.  Runs on the current stream without synchronising."""
    torch = _torch()
    N = weight.shape[0]
    if cross_triggers.dtype != torch.int64 or weight.dtype != torch.float64 or tuple(cross_triggers.shape) != (N, N) \
            or not cross_triggers.is_cuda or weight.device != cross_triggers.device \
            or not (cross_triggers.is_contiguous() and weight.is_contiguous()):
        raise ValueError("expected contiguous CUDA tensors: cross_triggers (N, N) int64 and weight (N,) float64")
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=weight.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (N,) or out.device != weight.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous (N,) float64 tensor on the matrix's device")
    with torch.cuda.device(weight.device):
        _ffi.check(_ffi.lib().acx_cross_trigger_rate(cross_triggers.data_ptr(), weight.data_ptr(), N, out.data_ptr(),
                                                     _ffi.stream_ptr(weight.device)))
    return out


def _scorer(metric, args):
    """(function, its arguments taken out of args) for metric "event" / "segment" / "intersection"."""
    if metric not in _SCORE_ARGS:
        raise ValueError('metric must be "event", "segment" or "intersection" (got %r)' % (metric,))
    own = {k: args.pop(k) for k in _SCORE_ARGS[metric] if k in args}
    other = [k for k in args if any(k in names for m, names in _SCORE_ARGS.items() if m != metric)]
    if other:
        raise TypeError("%s belongs to the other metric, not to metric=%r" % (", ".join(other), metric))
    return {"event": event_based_metrics, "segment": segment_based_metrics, "intersection": intersection_based_metrics}[metric], own


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
    step, steps, capacity) and the scorer's (t_collar, ... / time_resolution / dtc_threshold, ...).  A table that overflowed is
    decoded again through EventTable.check() and scored again; that is the only synchronisation.  Returns (threshold (N,) float32 device tensor --
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


# ---- PSDS on the device ---------------------------------------------------------------------------------------------------------

class PsdsResult:
    """What psds returns.  value: the PSDS (a float; NaN when no class has annotations); efpr (A,), etpr (A,) and class_curves
    (N, A): the PSD-ROC of psd_roc_host (numpy float64); counts: (T, N, 3) int64 device tensor = TP, FP, FN per threshold;
    thresholds: (T,) float32 numpy, as decoded; seen: (N,) bool numpy, the classes with annotations."""

    def __init__(self, value, efpr, etpr, class_curves, counts, thresholds, seen):
        self.value, self.efpr, self.etpr, self.class_curves = value, efpr, etpr, class_curves
        self.counts, self.thresholds, self.seen = counts, thresholds, seen

    def __float__(self):
        return self.value

    def __repr__(self):
        return "PsdsResult(value=%r, thresholds=%d, classes=%d)" % (self.value, len(self.thresholds), len(self.seen))


_UNSET = object()
_PSDS_DEFAULTS = dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0.0, alpha_st=0.0, max_efpr=100.0)


def check_psds_args(thresholds=None, scenario=None, dtc_threshold=_UNSET, gtc_threshold=_UNSET, cttc_threshold=_UNSET,
                    alpha_ct=_UNSET, alpha_st=_UNSET, max_efpr=_UNSET, unit_seconds=3600.0):
    """psds' own arguments, checked and with the scenario filled in, before anything touches the GPU -> (thresholds (T,) float32,
    dict of the seven settings).  Explicit arguments override the scenario's."""
    if scenario is not None and scenario not in PSDS_SCENARIOS:
        raise ValueError("scenario must be one of %s (got %r)" % (", ".join(sorted(PSDS_SCENARIOS)), scenario))
    cfg = dict(_PSDS_DEFAULTS)
    cfg.update(PSDS_SCENARIOS.get(scenario, {}))
    given = dict(dtc_threshold=dtc_threshold, gtc_threshold=gtc_threshold, cttc_threshold=cttc_threshold, alpha_ct=alpha_ct,
                 alpha_st=alpha_st, max_efpr=max_efpr)
    cfg.update({k: v for k, v in given.items() if v is not _UNSET})
    cfg["unit_seconds"] = unit_seconds
    cfg["dtc_threshold"], cfg["gtc_threshold"], cfg["cttc_threshold"] = _check_criteria(cfg["dtc_threshold"], cfg["gtc_threshold"],
                                                                                         cfg["cttc_threshold"])
    for name, low in (("alpha_ct", True), ("alpha_st", True), ("max_efpr", False), ("unit_seconds", False)):
        v = cfg[name]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) \
                or not (v >= 0 if low else v > 0):
            raise ValueError("%s must be a finite number %s 0 (got %r)" % (name, ">=" if low else ">", v))
        cfg[name] = float(v)
    if cfg["alpha_ct"] != 0 and cfg["cttc_threshold"] is None:
        raise ValueError("alpha_ct = %r weighs cross triggers: it needs a cttc_threshold" % (cfg["alpha_ct"],))
    thr = np.linspace(0.01, 0.99, 50).astype(np.float32) if thresholds is None else np.asarray(thresholds, dtype=np.float32)
    if thr.ndim != 1 or thr.size == 0 or not np.all(np.isfinite(thr)):
        raise ValueError("thresholds must be a non-empty 1-D array of finite numbers")
    return thr, cfg


def psds(probs, reference, thresholds=None, scenario=None, dtc_threshold=_UNSET, gtc_threshold=_UNSET, cttc_threshold=_UNSET,
         alpha_ct=_UNSET, alpha_st=_UNSET, max_efpr=_UNSET, unit_seconds=3600.0, **decode_args):
    """The polyphonic sound detection score of probabilities against annotations, decoded and scored on the GPU.  For every value
    of `thresholds` (default np.linspace(0.01, 0.99, 50); rounded to float32, what the decoder compares in):
    decode_events_gpu(probs, threshold=value, **decode_args) and acx_score_intersection, queued on the current stream with the
    geometry uploaded once.  scenario: "dcase_1" or "dcase_2" (PSDS_SCENARIOS), overridden by explicit arguments; without one:
    dtc_threshold = gtc_threshold = 0.7, no cttc_threshold, alpha_ct = alpha_st = 0, max_efpr = 100 per unit_seconds = 3600.
    With alpha_ct != 0 (which needs a cttc_threshold: ValueError) each table's cross-trigger matrix is reduced to its (N,) rates by
    acx_cross_trigger_rate at once and the one matrix buffer serves the next threshold.  A table that overflowed is decoded again
    through EventTable.check() and scored again; reading the statuses is the first synchronisation, the one copy of the (T, N, 3)
    counts and (T, N) rates the second.  The curve and the value are psd_roc_host's code on those numbers.  decode_args:
    decode_events_gpu's (low, median, min_duration, merge_gap, step, steps, capacity).  Returns a PsdsResult."""
    torch = _torch()
    if "threshold" in decode_args:
        raise TypeError("psds sets threshold itself")
    thr, cfg = check_psds_args(thresholds, scenario, dtc_threshold, gtc_threshold, cttc_threshold, alpha_ct, alpha_st, max_efpr,
                               unit_seconds)
    need = cfg["alpha_ct"] != 0
    criteria = _ffi.intersection_criteria(cfg["dtc_threshold"], cfg["gtc_threshold"], cfg["cttc_threshold"] if need else None)
    tables = [_seg.decode_events_gpu(probs, threshold=float(t), **decode_args) for t in thr]
    _check_pair(reference, tables[0])
    clips = _clip_arrays(tables[0])
    for t in tables[1:]:
        t._score_clips = clips                           # one geometry: one upload
    dev, N, T = tables[0].table.device, reference.classes, len(thr)
    total_seconds, class_seconds = psds_durations(reference, [e[-1] for e in tables[0].edges])
    matrix = weight = None
    if need:
        _check_matrix_size(N)
        matrix = torch.empty((N, N), dtype=torch.int64, device=dev)
        weight = torch.from_numpy(cross_trigger_weights(class_seconds, cfg["unit_seconds"])).to(dev)
    packed = torch.zeros((T, 4 * N), dtype=torch.int64, device=dev)       # per threshold: (N, 3) counts, then N rates (float64 bits)

    def score(i):
        s = _score_intersection(reference, tables[i], criteria, matrix, packed[i, :3 * N].view(N, 3))
        if need:
            cross_trigger_rate(matrix, weight, out=packed[i, 3 * N:].view(torch.float64))
        return s.status

    bad = torch.stack([score(i) for i in range(T)]).cpu().numpy().ravel()
    for i in np.nonzero(bad & _ffi.SCORE_BAD_TABLE)[0]:
        tables[i].check()                                # decodes an overflowed table again; raises for unusable input
        score(i)
    host = packed.cpu().numpy()
    rates = np.ascontiguousarray(host[:, 3 * N:]).view(np.float64) if need else None
    value, efpr, etpr, curves, seen = _psd_roc(host[:, :3 * N].reshape(T, N, 3), rates, total_seconds, cfg["alpha_ct"], cfg["alpha_st"],
                                               cfg["max_efpr"], cfg["unit_seconds"])
    return PsdsResult(value, efpr, etpr, curves, packed[:, :3 * N].reshape(T, N, 3), thr, seen)
