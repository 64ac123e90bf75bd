"""CPU: the definitions of the intersection-based counts and of PSDS (pytorch/sed_metrics.py: intersection_based_metrics_host,
psds_host, psd_roc_host, cross_trigger_rate_host) on hand-worked cases (tests/psds_cases.py), against an independent integer
rasterisation, and against a Python restatement of the walk of csrc/sed_score.hip::sed_intersection_kernel; the ctypes
declarations and the argument checks of acx_score_intersection / acx_cross_trigger_rate that need no launch.  No device needed."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import psds_cases as pc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import sed_metrics as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, SHAPE = -1, -4
IDS = lambda s: "x".join(map(str, s))          # noqa: E731


# ---- the counts ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c["name"])
def test_cases_by_hand(case):
    s = sm.intersection_based_metrics_host(case["ref"], pc.est_lists(case), case["classes"], **case["args"])
    assert s.kind == "intersection" and s.counts.dtype == s.est_relevant.dtype == s.ref_hit.dtype == np.int64
    assert s.counts.tolist() == case["counts"]
    assert s.est_relevant.tolist() == case["est_relevant"] and s.ref_hit.tolist() == case["ref_hit"]
    assert (s.cross_triggers is None) == (case["cross"] is None)
    if case["cross"] is not None:
        assert s.cross_triggers.dtype == np.int64 and s.cross_triggers.tolist() == case["cross"]


def test_cover():
    assert sm._cover(1.0, 3.0, []) == 0.0
    assert sm._cover(1.0, 3.0, [(0.0, 1.0), (3.0, 4.0)]) == 0.0                       # touching on either side
    assert sm._cover(1.0, 3.0, [(0.5, 1.5), (1.25, 2.0), (1.25, 1.5), (2.5, 9.0)]) == 1.5   # overlapping and nested rows once
    assert sm._cover(1.0, 3.0, [(0.0, 9.0), (1.0, 2.0)]) == 2.0


def test_neither_tp_nor_fp_shows_in_the_derived_numbers():
    case = next(c for c in pc.CASES if c["name"] == "relevant_but_gtc_fails")
    s = sm.intersection_based_metrics_host(case["ref"], pc.est_lists(case), 2, **case["args"])
    assert s.counts[0].tolist() == [0, 0, 1] and s.est_relevant.tolist() == [1]           # one detection, TP + FP == 0
    assert s.overall_error_rate == 1.0 and s.micro()["precision"] == 0.0                 # (FP + FN) / Nref


def raster(reference, estimated, classes, dtc, gtc, cttc, q=64):
    """the three criteria on a grid of 1 / q seconds in integers: every time is a multiple of 1 / q and every ratio a Fraction"""
    cells = lambda on, off: set(range(int(round(on * q)), int(round(off * q))))      # noqa: E731
    counts = np.zeros((classes, 3), np.int64)
    cross = None if cttc is None else np.zeros((classes, classes), np.int64)
    for ref, est in zip(reference, estimated):
        active = {}
        for c, on, off in ref:
            active.setdefault(c, set()).update(cells(on, off))
        relevant = {}
        for c, on, off in est:
            d = cells(on, off)
            if len(d & active.get(c, set())) >= dtc * len(d):
                relevant.setdefault(c, set()).update(d)
                continue
            counts[c, 1] += 1
            if cross is not None:
                for k, a in active.items():
                    if k != c and len(d & a) >= cttc * len(d):
                        cross[c, k] += 1
        for c, on, off in ref:
            g = cells(on, off)
            counts[c, 0 if len(g & relevant.get(c, set())) >= gtc * len(g) else 2] += 1
    return counts, cross


def grid_lists(rng, clips, classes, n, overlap):
    out = []
    for _ in range(clips):
        events, free = [], {}
        for _ in range(n):
            c = int(rng.integers(0, classes))
            on = int(rng.integers(0, 600)) if overlap else free.get(c, 0) + int(rng.integers(1, 160))
            off = on + int(rng.integers(1, 200))
            free[c] = off
            events.append((c, on / 64.0, off / 64.0))
        out.append(events)
    return out


@pytest.mark.parametrize("ratios", [(0.5, 0.5, 0.25), (0.75, 0.25, 0.5), (0.25, 0.75, 0.125), (0.125, 0.5, 0.75), (0.5, 0.5, None)], ids=str)
def test_against_the_integer_rasterisation(ratios):
    rng = np.random.default_rng(11)
    ref = grid_lists(rng, 4, 6, 14, overlap=True)               # annotations of one class may overlap
    est = grid_lists(rng, 4, 6, 14, overlap=False)
    dtc, gtc, cttc = ratios
    s = sm.intersection_based_metrics_host(ref, est, 6, dtc, gtc, cttc)
    counts, cross = raster(ref, est, 6, Fraction(dtc), Fraction(gtc), None if cttc is None else Fraction(cttc))
    assert np.array_equal(s.counts, counts), (s.counts.tolist(), counts.tolist())
    assert counts.sum(axis=0).min() > 0
    if cttc is not None:
        assert np.array_equal(s.cross_triggers, cross) and cross.sum() > 0 and np.all(np.diag(cross) == 0)
    assert s.counts[:, 1].sum() == (s.est_relevant == 0).sum() and s.counts[:, 0].sum() == s.ref_hit.sum()


@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_generated_cases_hold_every_count(shape):
    """the draws of the GPU cases (tests/test_gpu_psds.py), checked where no device is needed"""
    ref, est, ends = pc.host_case(*shape)
    for name, criteria in pc.CRITERIA.items():
        pc.needs_every_count(shape, name, sm.intersection_based_metrics_host(ref, est, shape[2], **criteria))


# ---- the kernel's walk ---------------------------------------------------------------------------------------------------------

def lower_bound(rows, key):
    lo, hi = 0, len(rows)
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if rows[mid][:2] < key:
            lo = mid + 1
        else:
            hi = mid
    return lo


def cover_row(on, off, b, state):
    """sc_cover_row; state = [covered, total]"""
    if on >= b:
        return False
    lo, hi = max(on, state[0]), min(off, b)
    if hi > lo:
        state[1] += hi - lo
        state[0] = hi
    return True


def walk(ref, est, clips, N, dtc, gtc, cttc):
    """sed_intersection_kernel, lane by lane: ref / est are the sorted tables of (clip, cls, onset, offset)"""
    counts = np.zeros((N, 3), np.int64)
    ct = None if cttc is None else np.zeros((N, N), np.int64)
    ref_hit, est_rel = [0] * len(ref), [-1] * len(est)
    for clip in range(clips):
        for cls in range(N):
            rlo, rhi = lower_bound(ref, (clip, cls)), lower_bound(ref, (clip, cls + 1))
            elo, ehi = lower_bound(est, (clip, cls)), lower_bound(est, (clip, cls + 1))
            clo = chi = 0
            if ct is not None and ehi > elo:
                clo, chi = lower_bound(ref, (clip, 0)), lower_bound(ref, (clip + 1, 0))
            low, fp = rlo, 0
            for j in range(elo, ehi):
                d_on, d_off = est[j][2:]
                while low < rhi and ref[low][3] <= d_on:
                    low += 1
                st = [d_on, 0.0]
                for r in range(low, rhi):
                    if not cover_row(ref[r][2], ref[r][3], d_off, st):
                        break
                est_rel[j] = 1 if st[1] >= dtc * (d_off - d_on) else 0
                if est_rel[j]:
                    continue
                fp += 1
                if ct is None:
                    continue
                i = clo
                while i < chi:
                    k = ref[i][1]
                    if k == cls:
                        i = rhi
                        continue
                    st, more = [d_on, 0.0], True
                    while i < chi and ref[i][1] == k:
                        if more:
                            more = cover_row(ref[i][2], ref[i][3], d_off, st)
                        i += 1
                    if st[1] >= cttc * (d_off - d_on):
                        ct[cls, k] += 1
            tp, low = 0, elo
            for r in range(rlo, rhi):
                g_on, g_off = ref[r][2:]
                while low < ehi and est[low][3] <= g_on:
                    low += 1
                st = [g_on, 0.0]
                for j in range(low, ehi):
                    if est[j][2] >= g_off:
                        break
                    if est_rel[j] == 0:
                        continue
                    cover_row(est[j][2], est[j][3], g_off, st)
                ref_hit[r] = 1 if st[1] >= gtc * (g_off - g_on) else 0
                tp += ref_hit[r]
            counts[cls] += (tp, fp, (rhi - rlo) - tp)
    return counts, ct, ref_hit, est_rel


def check_walk(ref, est, N, criteria):
    host = sm.intersection_based_metrics_host(ref, est, N, **criteria)
    counts, ct, ref_hit, est_rel = walk(sm._rows(ref, N), sm._rows(est, N, what="estimated"), len(ref), N, criteria["dtc_threshold"],
                                        criteria["gtc_threshold"], criteria["cttc_threshold"])
    assert np.array_equal(counts, host.counts)
    assert ref_hit == host.ref_hit.tolist() and est_rel == host.est_relevant.tolist()
    assert (ct is None) == (host.cross_triggers is None) and (ct is None or np.array_equal(ct, host.cross_triggers))


@pytest.mark.parametrize("shape", [s for s in pc.SHAPES if s[2] <= 130], ids=IDS)
def test_kernel_walk_equals_the_definition(shape):
    ref, est, ends = pc.host_case(*shape)
    for criteria in pc.CRITERIA.values():
        check_walk(ref, est, shape[2], criteria)


def test_kernel_walk_on_overlapping_rows_and_by_hand():
    rng = np.random.default_rng(3)
    ref, est = grid_lists(rng, 3, 5, 40, overlap=True), grid_lists(rng, 3, 5, 40, overlap=True)     # long, nested, overlapping
    for dtc, gtc, cttc in ((0.5, 0.5, 0.25), (0.125, 0.125, 0.125), (1.0, 0.25, None)):
        check_walk(ref, est, 5, dict(dtc_threshold=dtc, gtc_threshold=gtc, cttc_threshold=cttc))
    for case in pc.CASES:
        check_walk(case["ref"], pc.est_lists(case), case["classes"], case["args"])


# ---- PSDS ----------------------------------------------------------------------------------------------------------------------

PAIR = [[(0, 1.0, 2.0), (1, 3.0, 4.5)]]


def sweep(ref, estimated, N, ends, **criteria):
    """(counts (T, N, 3), cross triggers (T, N, N) or None, total_seconds, class_seconds) of a list of estimates"""
    scores = [sm.intersection_based_metrics_host(ref, est, N, **criteria) for est in estimated]
    ct = None if scores[0].cross_triggers is None else np.stack([s.cross_triggers for s in scores])
    return (np.stack([s.counts for s in scores]), ct) + sm.psds_durations(ref, ends, N)


def test_perfect_and_silent_detectors():
    for est, want in ((PAIR, 1.0), ([[]], 0.0)):
        args = sweep(PAIR, [est], 2, [10.0], dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=0.3)
        assert args[2] == 10.0 and args[3].tolist() == [1.0, 1.5]
        assert sm.psds_host(*args, alpha_ct=0.5, alpha_st=1.0) == want
        assert sm.psds_host(*args) == want


def hand_counts():
    """Two classes with 2 and 4 annotations, three operating points, one hour of audio, so fpr = FP per hour.
              class 0 (TP, FP)   class 1 (TP, FP)
        op 0      1, 0               1, 1          tpr 0.5 at 0        0.25 at 1
        op 1      2, 2               2, 1              1.0 at 2        0.5  at 1
        op 2      2, 3               4, 8              1.0 at 3        1.0  at 8, beyond max_efpr = 4: dropped
    axis 0, 1, 2, 3;  class 0's curve 0.5, 0.5, 1.0, 1.0;  class 1's 0, 0.5, 0.5, 0.5 (no point at or below 0: 0)."""
    tp_fp = [[(1, 0), (1, 1)], [(2, 2), (2, 1)], [(2, 3), (4, 8)]]
    nref = (2, 4)
    return np.array([[(tp, fp, nref[c] - tp) for c, (tp, fp) in enumerate(op)] for op in tp_fp], np.int64)


def test_psds_by_hand():
    counts = hand_counts()
    efpr, etpr, curves = sm.psd_roc_host(counts, None, 3600.0, [1800.0, 3600.0], max_efpr=4.0)
    assert efpr.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert curves.tolist() == [[0.5, 0.5, 1.0, 1.0], [0.0, 0.5, 0.5, 0.5]]
    assert etpr.tolist() == [0.25, 0.5, 0.75, 0.75]                                       # the means
    # widths 1, 1, 1 and 4 - 3: (0.25 + 0.5 + 0.75 + 0.75) / 4
    assert sm.psds_host(counts, None, 3600.0, [1800.0, 3600.0], max_efpr=4.0) == 0.5625
    # alpha_st = 1: the population std of two values is half their distance: 0.25, 0, 0.25, 0.25 -> etpr 0, 0.5, 0.5, 0.5
    efpr, etpr, _ = sm.psd_roc_host(counts, None, 3600.0, [1800.0, 3600.0], alpha_st=1.0, max_efpr=4.0)
    assert etpr.tolist() == [0.0, 0.5, 0.5, 0.5]
    assert sm.psds_host(counts, None, 3600.0, [1800.0, 3600.0], alpha_st=1.0, max_efpr=4.0) == 0.375
    # one cross trigger of class 0 on class 1 at op 1: weight[1] = 3600 / 3600 = 1, one other class, rate 1; alpha_ct = 1 moves
    # class 0's op 1 from 2 to 3.  axis 0, 1, 3; curves 0.5, 0.5, 1.0 and 0, 0.5, 0.5; means 0.25, 0.5, 0.75 over widths 1, 2, 1
    ct = np.zeros((3, 2, 2), np.int64)
    ct[1, 0, 1] = 1
    efpr, etpr, curves = sm.psd_roc_host(counts, ct, 3600.0, [1800.0, 3600.0], alpha_ct=1.0, max_efpr=4.0)
    assert efpr.tolist() == [0.0, 1.0, 3.0] and etpr.tolist() == [0.25, 0.5, 0.75]
    assert sm.psds_host(counts, ct, 3600.0, [1800.0, 3600.0], alpha_ct=1.0, max_efpr=4.0) == 0.5
    # the same trigger seen from class 1's side weighs 3600 / 1800 = 2
    assert sm.cross_trigger_rate_host(ct[1].T, sm.cross_trigger_weights([1800.0, 3600.0])).tolist() == [0.0, 2.0]


def test_a_point_beyond_max_efpr_adds_nothing():
    counts = hand_counts()
    far = counts[2:3].copy()
    far[0, :, 1] = 1000                                                                    # every class beyond the axis
    base = sm.psds_host(counts, None, 3600.0, [1800.0, 3600.0], max_efpr=4.0)
    assert sm.psds_host(np.concatenate([counts, far]), None, 3600.0, [1800.0, 3600.0], max_efpr=4.0) == base
    assert sm.psds_host(far, None, 3600.0, [1800.0, 3600.0], max_efpr=4.0) == 0.0            # an empty axis
    assert sm.psd_roc_host(far, None, 3600.0, [1800.0, 3600.0], max_efpr=4.0)[0].size == 0


def test_unseen_classes():
    counts = hand_counts()
    counts[:, 1] = (0, 3, 0)                                                               # class 1: detections, no annotation
    efpr, etpr, curves = sm.psd_roc_host(counts, None, 3600.0, [1800.0, 0.0], alpha_st=1.0, max_efpr=4.0)
    assert efpr.tolist() == [0.0, 2.0, 3.0] and etpr.tolist() == [0.5, 1.0, 1.0] and np.isnan(curves[1]).all()
    counts[:, 0] = (0, 1, 0)
    assert math.isnan(sm.psds_host(counts, None, 3600.0, [0.0, 0.0]))
    with pytest.raises(ValueError, match="differs between the operating points"):
        sm.psds_host(np.array([[[1, 0, 1]], [[1, 0, 2]]]), None, 10.0, [1.0])


def test_value_does_not_increase_with_the_alphas():
    B, S, N = 3, 31, 64
    ref = pc.host_case(B, S, N)[0]
    estimated = [pc.host_case(B, S, N, t)[1] for t in (0.3, 0.4, 0.5, 0.6, 0.7)]
    args = sweep(ref, estimated, N, [S * pc.STEP] * B, **pc.CRITERIA["dcase_2"])
    assert args[1].sum() > 0
    value = lambda **a: sm.psds_host(*args, max_efpr=3000.0, **a)          # noqa: E731
    st = [value(alpha_st=a) for a in (0.0, 0.5, 1.0, 2.0)]
    ct = [value(alpha_ct=a) for a in (0.0, 0.5, 1.0, 4.0)]
    assert all(a >= b for a, b in zip(st, st[1:])) and st[0] > st[-1] and 0 < st[0] < 1
    assert all(a >= b for a, b in zip(ct, ct[1:])) and ct[0] > ct[-1]


def test_cross_trigger_rate_is_one_sequential_sum():
    rng = np.random.default_rng(4)
    N = 130
    ct = rng.integers(0, 1000, size=(3, N, N)).astype(np.int64)                            # the diagonal is not zero here
    w = rng.random(N) * 1e3
    w[[0, 7, 64, 129]] = 0.0
    got = sm.cross_trigger_rate_host(ct, w)
    assert got.shape == (3, N) and all(np.array_equal(got[i], pc.sequential_rate(ct[i], w)) for i in range(3))
    assert not np.array_equal(got[0], (ct[0] * w * (1 - np.eye(N))).sum(axis=1) / (N - 5 + np.isin(np.arange(N), [0, 7, 64, 129])))
    assert sm.cross_trigger_rate_host(np.ones((2, 2), np.int64), np.zeros(2)).tolist() == [0.0, 0.0]


def test_scenarios():
    assert sm.PSDS_SCENARIOS == {
        "dcase_1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0.0, alpha_st=1.0, max_efpr=100.0),
        "dcase_2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1.0, max_efpr=100.0)}
    thr, cfg = sm.check_psds_args(scenario="dcase_2", alpha_st=0.0)                        # explicit arguments win
    assert thr.dtype == np.float32 and np.array_equal(thr, np.linspace(0.01, 0.99, 50).astype(np.float32))
    assert cfg == dict(sm.PSDS_SCENARIOS["dcase_2"], alpha_st=0.0, unit_seconds=3600.0)
    assert sm.check_psds_args()[1] == dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0.0, alpha_st=0.0,
                                           max_efpr=100.0, unit_seconds=3600.0)


# ---- declarations and argument checks --------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported():
    assert ctypes.sizeof(_ffi.AcxIntersectionCriteria) == 32
    f = _ffi.AcxIntersectionCriteria
    assert (f.dtc.offset, f.gtc.offset, f.cttc.offset, f.cross_triggers.offset, f.reserved.offset) == (0, 8, 16, 24, 28)
    c = _ffi.intersection_criteria()
    assert (c.dtc, c.gtc, c.cttc, c.cross_triggers) == (0.7, 0.7, 0.0, 0)
    c = _ffi.intersection_criteria(0.1, 0.2, 0.3)
    assert (c.dtc, c.gtc, c.cttc, c.cross_triggers, c.reserved) == (0.1, 0.2, 0.3, 1, 0)
    res, args = _ffi.SIGNATURES["acx_score_intersection"]
    assert res is ctypes.c_int and len(args) == 18 and args[11] is ctypes.POINTER(_ffi.AcxIntersectionCriteria)
    assert args[:11] == _ffi.SIGNATURES["acx_score_events"][1][:11]                        # the same leading arguments
    res, args = _ffi.SIGNATURES["acx_cross_trigger_rate"]
    assert res is ctypes.c_int and len(args) == 5 and args[2] is ctypes.c_int
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert ("typedef struct acx_intersection_criteria { double dtc, gtc, cttc; int32_t cross_triggers, reserved; } "
            "acx_intersection_criteria;") in hdr
    assert "ACX_API int acx_score_intersection(" in hdr and "ACX_API int acx_cross_trigger_rate(" in hdr
    lib = _ffi.lib()
    assert hasattr(lib, "acx_score_intersection") and hasattr(lib, "acx_cross_trigger_rate")


def _abi(**change):
    """one acx_score_intersection call with dummy HOST buffers in every pointer: the checks under test return before anything
    reads them"""
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    a = dict(ref=p, n_ref=1, est=p, capacity=1, est_count=p, est_status=p, B=1, N=2, steps=p, end=p, step=0.25,
             criteria=_ffi.intersection_criteria(0.5, 0.5, 0.5), counts=p, matrix=p, ref_hit=p, est_relevant=p, status=p)
    a.update(change)
    l = _ffi.lib()
    rc = l.acx_score_intersection(a["ref"], a["n_ref"], a["est"], a["capacity"], a["est_count"], a["est_status"], a["B"], a["N"],
                                  a["steps"], a["end"], a["step"], None if a["criteria"] is None else ctypes.byref(a["criteria"]),
                                  a["counts"], a["matrix"], a["ref_hit"], a["est_relevant"], a["status"], None)
    return rc, l.acx_last_error().decode()


def test_abi_argument_checks_return_before_the_device():
    who = "acx_score_intersection"
    for name in ("ref", "est", "est_count", "est_status", "steps", "end", "counts", "status", "criteria", "ref_hit", "est_relevant"):
        rc, msg = _abi(**{name: None})
        assert rc == ARG and msg == who + ": null argument", (name, rc, msg)
    rc, msg = _abi(matrix=None)
    assert rc == ARG and "cross_triggers is set and the matrix is null" in msg
    assert _abi(n_ref=-1)[0] == ARG and _abi(capacity=-1)[0] == ARG
    assert _abi(step=0.0)[0] == ARG and _abi(step=float("nan"))[0] == ARG
    assert _abi(B=0)[0] == SHAPE and _abi(N=0)[0] == SHAPE and _abi(N=_ffi.MAX_CLASSES + 1)[0] == SHAPE
    for bad in (0.0, -0.5, 1.0000000000000002, float("nan"), float("inf")):
        for i, name in enumerate(("dtc", "gtc", "cttc")):
            ratios = [0.5, 0.5, 0.5]
            ratios[i] = bad
            rc, msg = _abi(criteria=_ffi.intersection_criteria(*ratios))
            assert rc == ARG and who + ": " + name in msg and "(0, 1]" in msg, (bad, name, rc, msg)
    l = _ffi.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    for args in ((None, p, 2, p), (p, None, 2, p), (p, p, 2, None)):
        assert l.acx_cross_trigger_rate(*args, None) == ARG and l.acx_last_error().decode() == "acx_cross_trigger_rate: null argument"
    assert l.acx_cross_trigger_rate(p, p, 0, p, None) == SHAPE and l.acx_cross_trigger_rate(p, p, _ffi.MAX_CLASSES + 1, p, None) == SHAPE


def test_python_argument_errors():
    for name in ("dtc_threshold", "gtc_threshold", "cttc_threshold"):
        for bad in (0.0, 1.5, -0.1, float("nan"), float("inf"), True, "0.5"):
            with pytest.raises(ValueError, match=name + r" must be a finite number in \(0, 1\]"):
                sm.intersection_based_metrics_host([[]], [[]], 1, **{name: bad})
            with pytest.raises(ValueError, match=name):
                sm.check_psds_args(**{name: bad})
    with pytest.raises(ValueError, match="1 reference clips and 2 estimated"):
        sm.intersection_based_metrics_host([[]], [[], []], 1)
    with pytest.raises(ValueError, match="estimated clip 0, entry 0"):
        sm.intersection_based_metrics_host([[]], [[(0, 2.0, 1.0)]], 1)
    with pytest.raises(ValueError, match="needs a cttc_threshold"):
        sm.check_psds_args(alpha_ct=0.5)
    with pytest.raises(ValueError, match="needs a cttc_threshold"):
        sm.check_psds_args(scenario="dcase_2", cttc_threshold=None)
    with pytest.raises(ValueError, match="scenario must be one of dcase_1, dcase_2"):
        sm.check_psds_args(scenario="dcase_3")
    for name, bad in (("alpha_ct", -1.0), ("alpha_st", float("nan")), ("max_efpr", 0.0), ("unit_seconds", float("inf"))):
        with pytest.raises(ValueError, match=name + " must be a finite number"):
            sm.check_psds_args(cttc_threshold=0.3, **{name: bad})
    for bad in ([], [[0.5]], [0.5, float("nan")]):
        with pytest.raises(ValueError, match="thresholds must be a non-empty 1-D array"):
            sm.check_psds_args(thresholds=bad)
    with pytest.raises(TypeError, match="psds sets threshold itself"):
        sm.psds(None, None, threshold=0.5)
    with pytest.raises(ValueError, match="needs the cross triggers"):
        sm.psds_host(hand_counts(), None, 3600.0, [1800.0, 3600.0], alpha_ct=1.0)
    with pytest.raises(ValueError, match="134 MB"):
        sm._check_matrix_size(4097)
    sm._check_matrix_size(4096)
    with pytest.raises(ValueError, match="expected a ReferenceEvents and an EventTable"):
        sm.intersection_based_metrics([[]], [[]])


def test_scorer_families():
    f, own = sm._scorer("intersection", dict(dtc_threshold=0.5, cttc_threshold=0.3, capacity=7))
    assert f is sm.intersection_based_metrics and own == dict(dtc_threshold=0.5, cttc_threshold=0.3)
    with pytest.raises(ValueError, match="metric must be"):
        sm._scorer("psds", {})
    for metric, stray in (("intersection", "t_collar"), ("intersection", "time_resolution"), ("event", "dtc_threshold"),
                          ("segment", "cttc_threshold"), ("segment", "t_collar")):
        with pytest.raises(TypeError, match="other metric"):
            sm._scorer(metric, {stray: 0.5})
