"""CPU: the definitions of the sound-event-detection scores (pytorch/sed_metrics.py: event_based_metrics_host,
segment_based_metrics_host, SedScores, ReferenceEvents) on hand-worked cases with known counts (tests/sed_cases.py) and against an
independent brute-force rasterisation; the ctypes declarations and the host-side argument checks of acx_score_events /
acx_score_segments.  No device needed."""
import ctypes
import math
import os

import numpy as np
import pytest

import sed_cases as sc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import sed_metrics as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, SHAPE = -1, -4


@pytest.mark.parametrize("case", sc.EVENT_CASES, ids=lambda c: c["name"])
def test_event_cases_by_hand(case):
    s = sm.event_based_metrics_host([case["ref"]], [sc.est_list(case)], case["classes"], **case["args"])
    assert s.counts.dtype == np.int64 and s.ref_match.dtype == np.int64 and s.est_match.dtype == np.int64
    assert s.counts.tolist() == case["counts"]
    assert s.ref_match.tolist() == case["ref_match"]
    assert s.est_match.tolist() == case["est_match"]


def test_the_collar_is_hit_exactly():
    """the two cases around the collar differ by one ulp of the reference onset, and only that"""
    on, over = (c for c in sc.EVENT_CASES if c["name"] in ("onset_on_collar", "onset_one_ulp_over"))
    assert abs(on["ref"][0][1] - 1.25) == 0.25 and abs(over["ref"][0][1] - 1.25) > 0.25
    assert on["ref"][0][1] - over["ref"][0][1] == 2.0 ** -53


def test_event_cases_as_one_batch():
    """all cases as the clips of one call: the counts add up and the match rows shift by the clips before"""
    cases = [c for c in sc.EVENT_CASES if c["args"] == sc.COLLAR]
    assert len(cases) >= 8
    s = sm.event_based_metrics_host([c["ref"] for c in cases], [sc.est_list(c) for c in cases], 2, **sc.COLLAR)
    assert s.counts.tolist() == np.sum([c["counts"] for c in cases], axis=0).tolist()
    ref_match, est_match, r0, e0 = [], [], 0, 0
    for c in cases:
        ref_match += [m + e0 if m >= 0 else -1 for m in c["ref_match"]]
        est_match += [m + r0 if m >= 0 else -1 for m in c["est_match"]]
        r0 += len(c["ref"])
        e0 += len(c["est"])
    assert s.ref_match.tolist() == ref_match and s.est_match.tolist() == est_match


@pytest.mark.parametrize("case", sc.SEGMENT_CASES, ids=lambda c: c["name"])
def test_segment_cases_by_hand(case):
    s = sm.segment_based_metrics_host([case["ref"]], [sc.est_list(case)], [case["end"]], case["classes"], **case["args"])
    assert s.counts.dtype == np.int64 and s.overall.dtype == np.int64
    assert s.counts.tolist() == case["counts"]
    assert s.overall.tolist() == case["overall"]


def test_s_d_i_case_has_all_three():
    case = next(c for c in sc.SEGMENT_CASES if c["name"] == "s_d_i")
    assert min(case["overall"][1:4]) > 0


def brute_force_segments(reference, estimated, ends, classes, res):
    """the segment-based counts restated: rasterise into a dense (segments, classes) bool array per clip and count"""
    counts, overall = np.zeros((classes, 3), np.int64), np.zeros(6, np.int64)
    for ref, est, end in zip(reference, estimated, ends):
        nseg = int(np.ceil(end / res))
        grid = np.zeros((2, nseg, classes), bool)
        for k, events in enumerate((ref, est)):
            for ev in events:
                lo, hi = int(np.floor(ev[1] / res)), int(np.ceil(ev[2] / res))
                for seg in range(lo, min(hi, nseg)):
                    grid[k, seg, ev[0]] = True
        r, e = grid
        counts += np.stack([(r & e).sum(0), (e & ~r).sum(0), (r & ~e).sum(0)], axis=1)
        fn, fp = (r & ~e).sum(1), (e & ~r).sum(1)
        overall += [(r & e).sum(), np.minimum(fn, fp).sum(), np.maximum(fn - fp, 0).sum(), np.maximum(fp - fn, 0).sum(), r.sum(),
                    e.sum()]
    return counts, overall


def random_lists(rng, clips, classes, ends, n, quantum):
    out = []
    for i in range(clips):
        events = []
        for _ in range(n):
            on = quantum * rng.integers(0, int(ends[i] / quantum))
            off = on + quantum * rng.integers(1, 24)
            events.append((int(rng.integers(0, classes)), float(on), float(off)))       # may overlap, may pass the clip's end
        out.append(events)
    return out


@pytest.mark.parametrize("res", [1.0, 0.3, 0.1, 0.32])
def test_segments_against_brute_force(res):
    rng = np.random.default_rng(5)
    ends = [10.0, 7.3, 3.21]                          # not multiples of any of the resolutions
    ref = random_lists(rng, 3, 5, ends, 12, 0.16)
    est = random_lists(rng, 3, 5, ends, 12, 0.32)
    s = sm.segment_based_metrics_host(ref, est, ends, 5, time_resolution=res)
    counts, overall = brute_force_segments(ref, est, ends, 5, res)
    assert np.array_equal(s.counts, counts) and np.array_equal(s.overall, overall)
    assert counts.sum(axis=0).min() > 0 and overall.min() > 0, "the draw holds hits, false alarms, misses, S, D and I"
    assert overall[4] == counts[:, [0, 2]].sum() and overall[5] == counts[:, [0, 1]].sum() and overall[0] == counts[:, 0].sum()


def test_sed_scores_arithmetic():
    counts = np.array([[2, 1, 1], [0, 0, 0], [0, 3, 0], [0, 0, 2]], np.int64)
    s = sm.SedScores("event", counts)
    assert np.array_equal(s.precision, [2 / 3, 0.0, 0.0, 0.0])
    assert np.array_equal(s.recall, [2 / 3, 0.0, 0.0, 0.0])
    assert np.array_equal(s.f1, [4 / 6, 0.0, 0.0, 0.0])
    er = s.error_rate
    assert er[0] == 2 / 3 and er[3] == 1.0 and np.isnan(er[1]) and np.isnan(er[2])        # NaN where Nref == 0
    assert s.micro() == {"precision": 2 / 6, "recall": 2 / 5, "f1": 4 / 11, "error_rate": 7 / 5}
    assert s.macro() == {"precision": (2 / 3) / 2, "recall": (2 / 3) / 2, "f1": (4 / 6) / 2, "error_rate": (2 / 3 + 1.0) / 2}
    assert s.overall_error_rate == 7 / 5                                                # event-based: no substitutions
    empty = sm.SedScores("event", np.zeros((3, 3), np.int64))
    assert all(math.isnan(v) for v in empty.macro().values()) and math.isnan(empty.micro()["error_rate"])
    assert empty.micro()["f1"] == 0.0
    seg = sm.SedScores("segment", counts, overall=np.array([2, 1, 2, 3, 5, 6], np.int64))
    assert seg.overall_error_rate == (1 + 2 + 3) / 5
    assert math.isnan(sm.SedScores("segment", counts, overall=np.zeros(6, np.int64)).overall_error_rate)
    with pytest.raises(ValueError, match="segment-based"):
        s.overall_host()


def test_host_definitions_share_sed_scores():
    case = next(c for c in sc.SEGMENT_CASES if c["name"] == "s_d_i")
    s = sm.segment_based_metrics_host([case["ref"]], [sc.est_list(case)], case["end"], 3)       # one end for every clip
    assert isinstance(s, sm.SedScores) and s.overall_error_rate == 1.0
    assert np.array_equal(s.f1, [0.0, 2 / 3, 0.0])
    e = sm.event_based_metrics_host([case["ref"]], [sc.est_list(case)], 3)
    assert isinstance(e, sm.SedScores) and e.micro()["recall"] == 1 / 3


def test_reference_events_validation():
    ok = [[(0, 0.0, 1.0)], []]
    for bad, msg in ((("x", 0.0, 1.0), "neither an index nor one of the labels"), ((2, 0.0, 1.0), r"class 2 is outside \[0, 2\)"),
                     ((-1, 0.0, 1.0), "outside"), ((0, 1.0, 1.0), "0 <= onset < offset"), ((0, -0.5, 1.0), "0 <= onset < offset"),
                     ((0, 0.0, float("inf")), "finite"), ((0, float("nan"), 1.0), "finite"), ((0, 0.0), "expected"),
                     ((True, 0.0, 1.0), "neither")):
        with pytest.raises(ValueError, match=msg) as e:
            sm.ReferenceEvents.from_lists([ok[0], [ok[0][0], bad]], 2)
        assert "clip 1, entry 1" in str(e.value)
    with pytest.raises(ValueError, match="3 labels for 2 classes"):
        sm.ReferenceEvents.from_lists(ok, 2, labels=["a", "b", "c"])
    with pytest.raises(ValueError, match="classes must be"):
        sm.ReferenceEvents.from_lists(ok, 0)
    with pytest.raises(ValueError, match="estimated clip 0, entry 0"):
        sm.event_based_metrics_host([[]], [[(0, 2.0, 1.0)]], 1)
    with pytest.raises(ValueError, match="1 reference clips and 2 estimated"):
        sm.event_based_metrics_host([[]], [[], []], 1)
    with pytest.raises(ValueError, match="t_collar"):
        sm.event_based_metrics_host([[]], [[]], 1, t_collar=-0.1)
    with pytest.raises(ValueError, match="time_resolution"):
        sm.segment_based_metrics_host([[]], [[]], [1.0], 1, time_resolution=0.0)
    with pytest.raises(ValueError, match="2 ends for 1 clips"):
        sm.segment_based_metrics_host([[]], [[]], [1.0, 2.0], 1)


def test_reference_events_sorting_and_round_trip():
    labels = ["dog", "cat", "car"]
    per_clip = [[("car", 2.0, 3.0, 0.9, 0.8), ("dog", 2.0, 2.5), ("dog", 0.5, 4.0), (1, 0.5, 1.0)], [], [("cat", 1.0, 2.0)]]
    r = sm.ReferenceEvents.from_lists(per_clip, 3, labels=labels)
    assert r.table is None and len(r) == 5 and r.clips == 3 and r.classes == 3
    assert r.rows == [(0, 0, 0.5, 4.0), (0, 0, 2.0, 2.5), (0, 1, 0.5, 1.0), (0, 2, 2.0, 3.0), (2, 1, 1.0, 2.0)]   # (clip, cls, on, off)
    lists = r.to_lists()
    assert lists == [[("cat", 0.5, 1.0), ("dog", 0.5, 4.0), ("dog", 2.0, 2.5), ("car", 2.0, 3.0)], [], [("cat", 1.0, 2.0)]]
    again = sm.ReferenceEvents.from_lists(lists, 3, labels=labels)
    assert again.rows == r.rows and again.to_lists() == lists
    plain = sm.ReferenceEvents.from_lists(per_clip[2:], 3, labels=labels)
    assert sm.ReferenceEvents.from_lists([[(1, 1.0, 2.0)]], 3).to_lists() == [[(1, 1.0, 2.0)]] and plain.rows == [(0, 1, 1.0, 2.0)]


def test_ctypes_declarations():
    assert ctypes.sizeof(_ffi.AcxRefEvent) == 24 == _ffi.REF_EVENT_BYTES
    assert [(_ffi.AcxRefEvent.clip.offset, _ffi.AcxRefEvent.cls.offset, _ffi.AcxRefEvent.onset.offset,
             _ffi.AcxRefEvent.offset.offset)] == [(0, 4, 8, 16)]
    assert sm._REF_DTYPE.itemsize == 24 and [sm._REF_DTYPE.fields[k][1] for k in ("clip", "cls", "onset", "offset")] == [0, 4, 8, 16]
    assert ctypes.sizeof(_ffi.AcxEventCollar) == 24
    c = _ffi.event_collar()
    assert (c.t_collar, c.percentage_of_length, c.evaluate_onset, c.evaluate_offset) == (0.2, 0.5, 1, 1)
    assert _ffi.SCORE_BAD_TABLE == 1
    res, args = _ffi.SIGNATURES["acx_score_events"]
    assert res is ctypes.c_int and len(args) == 17 and args[11] is ctypes.POINTER(_ffi.AcxEventCollar)
    assert args[1] is args[3] is args[6] is ctypes.c_int64 and args[7] is ctypes.c_int and args[10] is ctypes.c_double
    res, args = _ffi.SIGNATURES["acx_score_segments"]
    assert res is ctypes.c_int and len(args) == 16 and args[10] is args[11] is ctypes.c_double
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert "typedef struct acx_ref_event { int32_t clip, cls; double onset, offset; } acx_ref_event;" in hdr
    assert "#define ACX_SCORE_BAD_TABLE 1" in hdr
    lib = _ffi.lib()
    assert hasattr(lib, "acx_score_events") and hasattr(lib, "acx_score_segments")


def _abi(which, **change):
    """one call with dummy HOST buffers in every pointer -- the checks under test return before anything reads them"""
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    a = dict(ref=p, n_ref=1, est=p, capacity=1, est_count=p, est_status=p, B=1, N=2, steps=p, end=p, step=0.25,
             collar=_ffi.event_collar(0.25, 0.5), res=1.0, counts=p, ref_match=p, est_match=p, overall=p, status=p)
    a.update(change)
    head = (a["ref"], a["n_ref"], a["est"], a["capacity"], a["est_count"], a["est_status"], a["B"], a["N"], a["steps"], a["end"],
            a["step"])
    l = _ffi.lib()
    if which == "events":
        rc = l.acx_score_events(*head, None if a["collar"] is None else ctypes.byref(a["collar"]), a["counts"], a["ref_match"],
                                a["est_match"], a["status"], None)
    else:
        rc = l.acx_score_segments(*head, a["res"], a["counts"], a["overall"], a["status"], None)
    return rc, l.acx_last_error().decode()


def test_abi_argument_checks_return_before_the_device():
    for which, own in (("events", ("collar", "ref_match", "est_match")), ("segments", ("overall",))):
        who = "acx_score_" + which
        for name in ("ref", "est", "est_count", "est_status", "steps", "end", "counts", "status") + own:
            rc, msg = _abi(which, **{name: None})
            assert rc == ARG and msg == who + ": null argument", (which, name, rc, msg)
        assert _abi(which, n_ref=-1)[0] == ARG and _abi(which, capacity=-1)[0] == ARG
        rc, msg = _abi(which, step=0.0)
        assert rc == ARG and "step_seconds 0 (expected > 0)" in msg
        assert _abi(which, step=float("nan"))[0] == ARG
        rc, msg = _abi(which, B=0)
        assert rc == SHAPE and "B = 0" in msg
        rc, msg = _abi(which, N=0)
        assert rc == SHAPE and "0 classes" in msg
        assert _abi(which, N=_ffi.MAX_CLASSES + 1)[0] == SHAPE
    for res in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = _abi("segments", res=res)
        assert rc == ARG and "time_resolution" in msg, (res, rc, msg)
    for t, pct in ((-0.25, 0.5), (0.25, -0.5), (float("nan"), 0.5), (0.25, float("inf"))):
        rc, msg = _abi("events", collar=_ffi.event_collar(t, pct))
        assert rc == ARG and "t_collar" in msg and "must be finite and not negative" in msg, (t, pct, rc, msg)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_generated_cases_hold_every_count(shape):
    """the seeds of the generated GPU cases (tests/test_gpu_sed_metrics.py), checked where no device is needed: decode_events gives
    the table's events, and the draw must hold hits, false alarms and misses -- and S, D, I on the 0.1 s grid; with one class
    a segment cannot hold a miss and a false alarm at once, so S is 0 there"""
    from audioset_convnext_inf_amd.pytorch import segments as seg
    B, S, N = shape
    p = sc.probabilities(B, S, N)
    est = [seg.decode_events(p[i], low=0.3) for i in range(B)]
    ends = [S * seg.SEGMENT_SECONDS] * B
    ref = sc.make_reference(est, ends, N, seg.SEGMENT_SECONDS)
    for args in (dict(t_collar=seg.SEGMENT_SECONDS), dict(), dict(t_collar=seg.SEGMENT_SECONDS, evaluate_offset=False),
                 dict(t_collar=seg.SEGMENT_SECONDS / 2, percentage_of_length=0.0, evaluate_onset=False)):
        s = sm.event_based_metrics_host(ref, est, N, **args)
        assert s.counts.sum(axis=0).min() > 0, (args, s.counts.sum(axis=0))
        hit = np.nonzero(s.ref_match >= 0)[0]
        assert np.array_equal(s.est_match[s.ref_match[hit]], hit) and len(hit) == s.counts[:, 0].sum()
    s = sm.segment_based_metrics_host(ref, est, ends, N, time_resolution=0.1)
    assert s.counts.sum(axis=0).min() > 0 and s.overall[2:4].min() > 0 and (s.overall[1] > 0) == (N > 1), s.overall
