"""Cases shared by tests/test_psds_cpu.py and tests/test_gpu_psds.py (not a test module): hand-worked counts of the
intersection criteria, and the generators of the larger cases.

Every hand-worked number is exactly representable: steps of 0.25 s, ratios of 0.25 / 0.5 / 0.75 / 1.0, so a cover exactly on
ratio * length is a tie that must pass.  A case is a dict:
  steps, ends  rows of every clip and the clips' last boundaries (edges k * 0.25 for k < steps, then the end)
  classes      N
  ref          per clip [(cls, onset_s, offset_s), ...]
  est          per clip [(cls, begin, end), ...] in steps, in table order (cls, begin)
  args         dtc_threshold, gtc_threshold, cttc_threshold
  counts       (N, 3) TP, FP, FN;  cross: (N, N) or None;  est_relevant / ref_hit: 1 / 0 per row in table order."""
import numpy as np

import sed_cases as sc
from audioset_convnext_inf_amd.pytorch import segments as seg

STEP = sc.STEP


def edges(case, clip=0):
    e = np.arange(case["steps"] + 1, dtype=np.float64) * STEP
    e[-1] = case["ends"][clip]
    return e


def est_lists(case):
    """the estimated events of every clip as (cls, onset_s, offset_s)"""
    return [[(c, float(edges(case, i)[b]), float(edges(case, i)[x])) for c, b, x in events] for i, events in enumerate(case["est"])]


def _case(name, ref, est, counts, est_relevant, ref_hit, dtc, gtc, cttc=None, cross=None, classes=2, steps=40, end=10.0):
    if ref and not isinstance(ref[0], list):
        ref, est = [ref], [est]
    return dict(name=name, steps=steps, ends=[end] * len(ref), classes=classes, ref=ref, est=est,
                args=dict(dtc_threshold=dtc, gtc_threshold=gtc, cttc_threshold=cttc), counts=counts, cross=cross,
                est_relevant=est_relevant, ref_hit=ref_hit)


Z2 = [[0, 0], [0, 0]]
CASES = [
    # the detection [1.0, 2.0) has 0.75 s of its 1.0 s annotated: 0.75 >= 0.75 * 1.0, a tie, passes; the annotation is then
    # covered entirely
    _case("dtc_on_the_ratio", [(0, 1.0, 1.75)], [(0, 4, 8)], [[1, 0, 0], [0, 0, 0]], [1], [1], 0.75, 0.25),
    # a quarter step (0.0625 s) less: 0.6875 < 0.75.  The detection is a false positive and nothing relevant covers the annotation
    _case("dtc_quarter_step_short", [(0, 1.0, 1.6875)], [(0, 4, 8)], [[0, 1, 1], [0, 0, 0]], [0], [0], 0.75, 0.25),
    # [1.0, 2.0) and [1.5, 2.5) overlap: their union covers 1.5 s of the detection [1.0, 3.0), their sum would be 2.0 s.
    # With dtc = 1.0 the sum would pass (2.0 >= 2.0) and the union does not: a ratio cannot exceed 1
    _case("overlap_is_a_union_fails", [(0, 1.0, 2.0), (0, 1.5, 2.5)], [(0, 4, 12)], [[0, 1, 2], [0, 0, 0]], [0], [0, 0], 1.0, 1.0),
    # ... and 1.5 >= 0.75 * 2.0 is a tie; both annotations lie inside the relevant detection
    _case("overlap_is_a_union_tie", [(0, 1.0, 2.0), (0, 1.5, 2.5)], [(0, 4, 12)], [[2, 0, 0], [0, 0, 0]], [1], [1, 1], 0.75, 1.0),
    # [1.0, 2.5) holds 0.5 s of each annotation: 1.0 >= 0.5 * 1.5 only through both (0.5 < 0.75 through one)
    _case("relevant_through_two_annotations", [(0, 1.0, 1.5), (0, 2.0, 2.5)], [(0, 4, 10)], [[2, 0, 0], [0, 0, 0]], [1], [1, 1], 0.5, 1.0),
    # two detections of 0.75 s inside a 2 s annotation: 1.5 >= 0.75 * 2.0 through both, a tie (0.75 < 1.5 through one)
    _case("annotation_covered_by_two_detections", [(0, 1.0, 3.0)], [(0, 4, 7), (0, 9, 12)], [[1, 0, 0], [0, 0, 0]], [1, 1], [1], 1.0, 0.75),
    # the detection lies inside a 4 s annotation (relevant) and covers 1 s of it: 1.0 < 0.5 * 4.0.  Neither a TP nor an FP
    _case("relevant_but_gtc_fails", [(0, 1.0, 5.0)], [(0, 4, 8)], [[0, 0, 1], [0, 0, 0]], [1], [0], 0.75, 0.5),
    # class 0 is not annotated: [1.0, 3.0) is an FP.  Class 1 covers 1.0 s of it (a tie with 0.5 * 2.0), class 2 covers 0.5 + 0.5
    # through two annotations, class 3 only 0.75
    _case("fp_cross_triggers_two_classes", [(1, 1.0, 2.0), (2, 0.5, 1.5), (2, 2.5, 3.5), (3, 2.5, 3.25)], [(0, 4, 12)],
          [[0, 1, 0], [0, 0, 1], [0, 0, 2], [0, 0, 1]], [0], [0, 0, 0, 0], 0.5, 0.5, 0.5,
          [[0, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], classes=4),
    # a relevant detection lies on class 1's annotation too: no cross trigger
    _case("relevant_makes_no_cross_trigger", [(0, 1.0, 2.0), (1, 1.0, 2.0)], [(0, 4, 8)], [[1, 0, 0], [0, 0, 1]], [1], [1, 0],
          0.75, 0.75, 0.25, Z2),
    # the annotations lie in clip 1, the detection in clip 0: a false positive there without a cross trigger, two misses here
    _case("annotations_in_another_clip", [[], [(0, 1.0, 2.0), (1, 1.0, 2.0)]], [[(0, 4, 8)], []], [[0, 1, 1], [0, 0, 1]], [0], [0, 0],
          0.25, 0.25, 0.25, Z2),
]

# ---- generated cases ---------------------------------------------------------------------------------------------------------
# (clips, steps, classes): one lane, a full wave, two units per clip, three units, the real class count with its 527 x 527
# matrix, and one-step clips
SHAPES = [(1, 31, 1), (3, 31, 64), (1, 313, 65), (3, 31, 130), (3, 31, 527), (3, 1, 65)]
DEGENERATE = [(1, 31, 1), (3, 1, 65)]             # too small to promise hits, false alarms, misses and cross triggers
CRITERIA = {"dcase_1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None),
            "dcase_2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3)}


def decode_args(threshold=0.5):
    return dict(threshold=threshold, low=0.6 * threshold, median=3, step=STEP)


def host_case(B, S, N, threshold=0.5):
    """(reference lists, estimated lists, ends) of a generated case, decoded on the host"""
    p = sc.probabilities(B, S, N)
    est = [[e[:3] for e in seg.decode_events(p[i], **decode_args(threshold))] for i in range(B)]
    ends = [S * STEP] * B
    return sc.make_reference(est, ends, N, STEP), est, ends


def needs_every_count(shape, scenario, host):
    """a generated case must hold hits, false alarms and misses, and cross triggers when they are asked for"""
    if tuple(shape) in DEGENERATE:
        return
    assert host.counts.sum(axis=0).min() > 0, "the case needs TP, FP and FN: %r" % (host.counts.sum(axis=0),)
    if host.cross_triggers is not None:
        assert host.cross_triggers.sum() > 0 and np.all(np.diag(host.cross_triggers) == 0), scenario


def sequential_rate(ct, weight):
    """acx_cross_trigger_rate said in plain Python: one float64 accumulator per class, ascending k"""
    N = len(weight)
    out = np.zeros(N, np.float64)
    for c in range(N):
        acc, n = 0.0, 0
        for k in range(N):
            if k != c and weight[k] > 0:
                acc += float(int(ct[c, k])) * float(weight[k])
                n += 1
        out[c] = acc / n if n else 0.0
    return out
