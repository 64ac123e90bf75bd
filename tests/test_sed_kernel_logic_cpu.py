"""CPU: the two walks of csrc/sed_score.hip restated in Python, against the host definitions (pytorch/sed_metrics.py).

The kernels do not run the definitions literally.  The matching kernel keeps a pointer into a column's estimated rows that only
moves forward and ends a scan at the first row behind the onset window; the segment kernel merges intervals into unions on the
fly, walks a tile from change to change and books misses and false alarms as +1 / -1 into per-segment difference arrays that it
scans afterwards, tile by tile.  That these shortcuts change no count and no match is an argument about sorted tables and
monotone rounding (the comments in sed_score.hip); this file tests the argument itself, statement by statement the same walks,
where no device is needed.  The GPU tests then check the kernels."""
import math

import numpy as np
import pytest

import sed_cases as sc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import sed_metrics as sm
from audioset_convnext_inf_amd.pytorch import segments as seg

TILE = _ffi.SCORE_TILE_SEGMENTS
STEP = seg.SEGMENT_SECONDS


def columns(rows):
    d = {}
    for i, r in enumerate(rows):
        d.setdefault(r[:2], []).append(i)
    return d


def walk_events(ref, est, N, t_collar, pct, on, off):
    rm, em = [-1] * len(ref), [-1] * len(est)
    counts = np.zeros((N, 3), np.int64)
    rc, ec = columns(ref), columns(est)
    for key in set(rc) | set(ec):
        rr, ee = rc.get(key, []), ec.get(key, [])
        rlo, rhi = (rr[0], rr[-1] + 1) if rr else (0, 0)
        elo, ehi = (ee[0], ee[-1] + 1) if ee else (0, 0)
        low, tp = elo, 0
        for r in range(rlo, rhi):
            r_on, r_off = ref[r][2], ref[r][3]
            tol = max(t_collar, pct * (r_off - r_on))
            while low < ehi:
                if em[low] < 0:
                    if not on:
                        break
                    e_on = est[low][2]
                    if not (e_on < r_on) or abs(r_on - e_on) <= t_collar:
                        break
                low += 1
            j = low
            while j < ehi:
                e_on, e_off = est[j][2], est[j][3]
                if on:
                    if not (abs(r_on - e_on) <= t_collar):
                        if e_on > r_on:
                            break
                        j += 1
                        continue
                if em[j] >= 0:
                    j += 1
                    continue
                if off and not (abs(r_off - e_off) <= tol):
                    j += 1
                    continue
                rm[r] = j; em[j] = r; tp += 1
                break
        counts[key[1]] += (tp, (ehi - elo) - tp, (rhi - rlo) - tp)
    return counts, rm, em


class Union:
    def __init__(self, rows, idx, res, nseg, s0, s1):
        self.rows, self.idx, self.i, self.res, self.nseg, self.s0, self.s1 = rows, idx, 0, res, nseg, s0, s1
        self.peeked = False
        self.na = self.nb = 0
        self.next()

    def clamp(self, f):
        return self.nseg if f >= self.nseg else int(f) if f > 0 else 0

    def row(self, k):
        r = self.rows[self.idx[k]]
        return self.clamp(math.floor(r[2] / self.res)), self.clamp(math.ceil(r[3] / self.res))

    def done(self):
        return self.a >= self.s1

    def next(self):
        hi = len(self.idx)
        while True:
            if not self.peeked:
                if self.i >= hi:
                    self.a = self.b = self.s1
                    return
                self.na, self.nb = self.row(self.i); self.i += 1
            self.peeked = False
            ca, cb = self.na, self.nb
            while self.i < hi:
                self.na, self.nb = self.row(self.i); self.i += 1
                if self.na > cb:
                    self.peeked = True
                    break
                cb = max(cb, self.nb)
            if ca >= self.s1:
                self.a = self.b = self.s1; self.i = hi; self.peeked = False
                return
            if cb <= self.s0 or ca >= cb:
                continue
            self.a, self.b = max(ca, self.s0), min(cb, self.s1)
            return


def walk_segments(ref, est, ends, N, res):
    counts = np.zeros((N, 3), np.int64)
    overall = np.zeros(6, np.int64)
    rc, ec = columns(ref), columns(est)
    for clip, end in enumerate(ends):
        f = math.ceil(end / res)
        nseg = int(f) if f > 0 else 0
        for s0 in range(0, nseg, TILE):
            s1 = min(s0 + TILE, nseg)
            ln = s1 - s0
            dfn, dfp = [0] * (TILE + 1), [0] * (TILE + 1)
            for cls in range(N):
                R = Union(ref, rc.get((clip, cls), []), res, nseg, s0, s1)
                E = Union(est, ec.get((clip, cls), []), res, nseg, s0, s1)
                tp = fp = fn = 0
                p = s0
                while p < s1:
                    in_r, in_e = R.a <= p, E.a <= p
                    qr = R.b if in_r else R.a
                    qe = E.b if in_e else E.a
                    q = min(qr, qe)
                    assert q > p and q <= s1
                    if in_r and in_e:
                        tp += q - p
                    elif in_r:
                        fn += q - p; dfn[p - s0] += 1; dfn[q - s0] -= 1
                    elif in_e:
                        fp += q - p; dfp[p - s0] += 1; dfp[q - s0] -= 1
                    p = q
                    if not R.done() and R.b <= p:
                        R.next()
                    if not E.done() and E.b <= p:
                        E.next()
                counts[cls] += (tp, fp, fn)
                overall[0] += tp; overall[4] += tp + fn; overall[5] += tp + fp
            a = b = 0
            for i in range(ln):
                a += dfn[i]; b += dfp[i]
                overall[1] += min(a, b); overall[2] += max(a - b, 0); overall[3] += max(b - a, 0)
    return counts, overall


def generated(B, S, N):
    p = sc.probabilities(B, S, N)
    est = [[e[:3] for e in seg.decode_events(p[i], low=0.3)] for i in range(B)]
    ends = [S * STEP] * B
    return sc.make_reference(est, ends, N, STEP), est, ends


EVENT_ARGS = [dict(t_collar=STEP), dict(), dict(t_collar=STEP, evaluate_offset=False),
              dict(t_collar=STEP / 2, percentage_of_length=0.0, evaluate_onset=False), dict(evaluate_onset=False, evaluate_offset=False)]


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matching_walk_equals_the_definition(shape):
    ref, est, ends = generated(*shape)
    N = shape[2]
    rows, erows = sm._rows(ref, N), sm._rows(est, N, what="estimated")
    for a in EVENT_ARGS:
        host = sm.event_based_metrics_host(ref, est, N, **a)
        counts, ref_match, est_match = walk_events(rows, erows, N, a.get("t_collar", 0.2), a.get("percentage_of_length", 0.5),
                                                   a.get("evaluate_onset", True), a.get("evaluate_offset", True))
        assert np.array_equal(counts, host.counts) and ref_match == host.ref_match.tolist() and est_match == host.est_match.tolist(), a


@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s[2] <= 65], ids=lambda s: "x".join(map(str, s)))
def test_segment_walk_equals_the_definition(shape):
    ref, est, ends = generated(*shape)
    N = shape[2]
    rows, erows = sm._rows(ref, N), sm._rows(est, N, what="estimated")
    grids = [0.1, STEP, 1.0]
    if shape == (1, 313, 65):                    # around one tile, and three tiles
        grids += [ends[0] / (n - 0.5) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
    for res in grids:
        host = sm.segment_based_metrics_host(ref, est, ends, N, time_resolution=res)
        counts, overall = walk_segments(rows, erows, ends, N, res)
        assert np.array_equal(counts, host.counts) and np.array_equal(overall, host.overall), (res, overall, host.overall)


def test_walks_on_the_hand_worked_cases():
    for case in sc.EVENT_CASES:
        a = case["args"]
        counts, ref_match, est_match = walk_events(sm._rows([case["ref"]], 2), sm._rows([sc.est_list(case)], 2), 2, a["t_collar"],
                                                   a["percentage_of_length"], a.get("evaluate_onset", True), a.get("evaluate_offset", True))
        assert counts.tolist() == case["counts"] and ref_match == case["ref_match"] and est_match == case["est_match"], case["name"]
    for case in sc.SEGMENT_CASES:
        counts, overall = walk_segments(sm._rows([case["ref"]], 3), sm._rows([sc.est_list(case)], 3), [case["end"]], 3,
                                        case["args"]["time_resolution"])
        assert counts.tolist() == case["counts"] and overall.tolist() == case["overall"], case["name"]
