"""Hand-worked scoring cases shared by tests/test_sed_metrics_cpu.py and tests/test_gpu_sed_metrics.py (not a test module).

Every number is exactly representable: steps of 0.25 s, a collar of 0.25 s.  A case is a dict:
  steps, end   rows of the one clip and its last boundary (edges k * 0.25 for k < steps, then `end`)
  classes      N
  ref          [(cls, onset_s, offset_s), ...]
  est          [(cls, begin, end), ...] in steps, in table order (cls, begin)
  args         the scorer's arguments
  counts       (N, 3) TP, FP, FN worked out by hand; event cases add ref_match / est_match (rows in table order), segment
               cases add overall = TP, S, D, I, Nref, Nsys."""
import numpy as np

STEP = 0.25
COLLAR = dict(t_collar=0.25, percentage_of_length=0.0)
UP = lambda v: float(np.nextafter(v, np.inf))          # noqa: E731
DOWN = lambda v: float(np.nextafter(v, -np.inf))       # noqa: E731


def edges(case):
    e = np.arange(case["steps"] + 1, dtype=np.float64) * STEP
    e[-1] = case["end"]
    return e


def est_list(case):
    """the estimated events of the case's clip as (cls, onset_s, offset_s)"""
    e = edges(case)
    return [(c, float(e[b]), float(e[x])) for c, b, x in case["est"]]


def _ev(name, ref, est, counts, ref_match, est_match, steps=40, end=10.0, classes=2, **args):
    a = dict(COLLAR)
    a.update(args)
    return dict(name=name, steps=steps, end=end, classes=classes, ref=ref, est=est, args=a, counts=counts, ref_match=ref_match,
                est_match=est_match)


EVENT_CASES = [
    # |1.0 - 1.25| = 0.25 <= 0.25: a difference exactly on the collar matches
    _ev("onset_on_collar", [(0, 1.0, 2.0)], [(0, 5, 8)], [[1, 0, 0], [0, 0, 0]], [0], [0]),
    # one ulp more does not: (1 - 2^-53) - 1.25 = -(0.25 + 2^-53), which float64 holds exactly
    _ev("onset_one_ulp_over", [(0, DOWN(1.0), 2.0)], [(0, 5, 8)], [[0, 1, 1], [0, 0, 0]], [-1], [-1]),
    _ev("offset_on_collar", [(0, 1.25, 2.25)], [(0, 5, 8)], [[1, 0, 0], [0, 0, 0]], [0], [0]),
    _ev("offset_one_ulp_over", [(0, 1.25, UP(2.25))], [(0, 5, 8)], [[0, 1, 1], [0, 0, 0]], [-1], [-1]),
    # two estimated events inside the first reference event's onset collar (0.75 and 1.25 around 1.0): it takes the first,
    # the second then serves the next reference event
    _ev("first_of_two_then_next", [(0, 1.0, 3.0), (0, 1.25, 3.0)], [(0, 3, 4), (0, 5, 6)], [[2, 0, 0], [0, 0, 0]], [0, 1], [0, 1],
        evaluate_offset=False),
    # ... or counts as a false positive
    _ev("first_of_two_then_fp", [(0, 1.0, 3.0)], [(0, 3, 4), (0, 5, 6)], [[1, 1, 0], [0, 0, 0]], [0], [0, -1], evaluate_offset=False),
    # two (overlapping) reference events compete for one estimated event: the earlier one gets it
    _ev("two_refs_one_est", [(0, 1.0, 2.0), (0, 1.25, 2.0)], [(0, 5, 8)], [[1, 0, 1], [0, 0, 0]], [0, -1], [0]),
    # an 8 s event: the offset may be 0.5 * 8 = 4 s off, far beyond the collar; 4.25 s is too much
    _ev("length_dominates", [(1, 1.0, 9.0)], [(1, 4, 20)], [[0, 0, 0], [1, 0, 0]], [0], [0], percentage_of_length=0.5),
    _ev("length_exceeded", [(1, 1.0, 9.0)], [(1, 4, 19)], [[0, 0, 0], [0, 1, 1]], [-1], [-1], percentage_of_length=0.5),
    _ev("onset_only", [(0, 1.0, 2.0)], [(0, 4, 30)], [[1, 0, 0], [0, 0, 0]], [0], [0], evaluate_offset=False),
    _ev("onset_only_needs_it", [(0, 1.0, 2.0)], [(0, 4, 30)], [[0, 1, 1], [0, 0, 0]], [-1], [-1]),
    _ev("offset_only", [(0, 1.0, 2.0)], [(0, 0, 8)], [[1, 0, 0], [0, 0, 0]], [0], [0], evaluate_onset=False),
    _ev("offset_only_needs_it", [(0, 1.0, 2.0)], [(0, 0, 8)], [[0, 1, 1], [0, 0, 0]], [-1], [-1]),
    # overlapping reference events of one class, each with an estimated event of its own; class 1 has a miss
    _ev("overlapping_refs", [(0, 1.0, 3.0), (0, 2.0, 4.0), (1, 5.0, 6.0)], [(0, 4, 6), (0, 8, 10)], [[2, 0, 0], [0, 0, 1]], [0, 1, -1],
        [0, 1], evaluate_offset=False),
    # the clip's last boundary is 9.9 s, not 40 * 0.25: an event that ends there ends at 9.9.  |9.7 - 9.9| matches (10.0 would
    # not); |10.2 - 9.9| does not (10.0 would)
    _ev("moved_last_boundary_hit", [(0, 9.0, 9.7)], [(0, 36, 40)], [[1, 0, 0], [0, 0, 0]], [0], [0], end=9.9),
    _ev("moved_last_boundary_miss", [(0, 9.0, 10.2)], [(0, 36, 40)], [[0, 1, 1], [0, 0, 0]], [-1], [-1], end=9.9),
    _ev("empty_reference", [], [(0, 4, 8), (1, 2, 3)], [[0, 1, 0], [0, 1, 0]], [], [-1, -1]),
    _ev("empty_estimate", [(0, 1.0, 2.0), (1, 1.0, 2.0), (1, 3.0, 4.0)], [], [[0, 0, 1], [0, 0, 2]], [-1, -1, -1], []),
    _ev("both_empty", [], [], [[0, 0, 0], [0, 0, 0]], [], []),
]


def _sg(name, ref, est, counts, overall, steps=40, end=10.0, classes=3, time_resolution=1.0):
    return dict(name=name, steps=steps, end=end, classes=classes, ref=ref, est=est, args=dict(time_resolution=time_resolution),
                counts=counts, overall=overall)


SEGMENT_CASES = [
    # [1.0, 3.0) ends exactly on a segment boundary: segments 1 and 2, no third
    _sg("ends_on_boundary", [(0, 1.0, 3.0)], [(0, 4, 12)], [[2, 0, 0], [0, 0, 0], [0, 0, 0]], [2, 0, 0, 0, 2, 2]),
    # 2.5 s at 1 s resolution: three segments, the last one short
    _sg("short_last_segment", [(0, 0.5, 2.4)], [(0, 0, 10)], [[3, 0, 0], [0, 0, 0], [0, 0, 0]], [3, 0, 0, 0, 3, 3], steps=10, end=2.5),
    # a reference offset beyond the clip's end is clipped: one missed segment, not five
    _sg("offset_beyond_end", [(1, 2.0, 7.0)], [], [[0, 0, 0], [0, 0, 1], [0, 0, 0]], [0, 0, 1, 0, 1, 0], steps=10, end=2.5),
    # segment 0: class 0 missed, class 1 a false alarm -> one substitution; segment 2: a miss alone -> a deletion; segment 4: a
    # false alarm alone -> an insertion; segment 6: a hit
    _sg("s_d_i", [(0, 0.0, 1.0), (0, 2.0, 3.0), (1, 6.0, 7.0)], [(1, 0, 4), (1, 24, 28), (2, 16, 20)],
        [[0, 0, 2], [1, 1, 0], [0, 1, 0]], [1, 1, 1, 1, 3, 3]),
    # 0.5 s resolution: [1.25, 2.25) touches segments 2, 3, 4; the estimate [1.0, 2.0) covers 2, 3
    _sg("half_second_grid", [(2, 1.25, 2.25)], [(2, 4, 8)], [[0, 0, 0], [0, 0, 0], [2, 0, 1]], [2, 0, 1, 0, 3, 2], time_resolution=0.5),
    _sg("both_empty", [], [], [[0, 0, 0]] * 3, [0] * 6),
]


# ---- generated cases ---------------------------------------------------------------------------------------------------------
# (clips, steps, classes): the lane and unit edges of the kernels (1, 64, 65, 527 classes), one and several clips, one step, a
# few, and more than one tile of 0.1 s segments
SHAPES = [(1, 31, 1), (3, 31, 64), (1, 313, 65), (3, 31, 527), (3, 1, 65)]


def probabilities(B, S, N, seed=0):
    """The recipe of tests/test_gpu_events.py: the sigmoid of temporally smoothed Gaussian noise, shifted so that about 30 % of
    the cells are >= 0.5, with values exactly on 0.5 and 0.3 and exact ties planted.  float32 numpy (B, S, N)."""
    import torch
    g = torch.Generator().manual_seed(1234 + seed)
    z = torch.randn(B, S + 4, N, generator=g, dtype=torch.float64)
    z = (z[:, :-4] + z[:, 1:-3] + z[:, 2:-2] + z[:, 3:-1] + z[:, 4:]) / 5 ** 0.5
    p = torch.sigmoid(3.0 * (z - 0.52)).to(torch.float32)
    u = torch.rand(B, S, N, generator=g)
    p[u < 0.03] = 0.5
    p[(u >= 0.03) & (u < 0.06)] = 0.3
    tie = (u >= 0.06) & (u < 0.12)
    tie[:, 0] = False
    p[tie] = torch.roll(p, 1, dims=1)[tie]
    return p.numpy()


def make_reference(estimated, ends, classes, step, seed=0):
    """Annotations for decoded events: the events of `estimated` (per clip (cls, onset_s, offset_s, ...)) with onset and offset
    moved by -2 .. 2 half steps, about one in seven dropped, one in seven doubled by an overlapping event of the same class, and
    spurious events added."""
    rng = np.random.default_rng(100 + seed)
    half = step / 2
    out = []
    for events, end in zip(estimated, ends):
        ref = []
        for ev in events:
            u = rng.random()
            k_on, k_off = rng.integers(-2, 3, size=2)
            if u < 0.15:
                continue
            on, off = max(ev[1] + k_on * half, 0.0), ev[2] + k_off * half
            if not on < off:
                on, off = ev[1], ev[2]
            ref.append((ev[0], on, off))
            if u > 0.85:
                ref.append((ev[0], on + half, off + 3 * half))
        for _ in range(1 + len(events) // 6):
            on = half * int(rng.integers(0, max(int(end / half), 1)))
            ref.append((int(rng.integers(0, classes)), on, on + half * int(rng.integers(1, 5))))
        out.append(ref)
    return out
