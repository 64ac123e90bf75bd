"""CPU: what the depthwise-form cases (tests/dwconv_cases.py) reach, asked from the launcher's own planning function
(acx_test_dwconv7_plan: no context, no device), the guard and the division of the column kernel, and that the bound of
tests/test_gpu_dwconv_forms.py tells a kernel with one kernel row lost at a segment head from a correct one."""
import ctypes

import numpy as np
import pytest

from audioset_convnext_inf_amd import _ffi
import dwconv_cases as dc
import layer_ref as lr


def _plans():
    out = []
    for s, B, H, tw, tw2 in dc.UNIFORM_CASES:
        p = dc.plan(s, B, H, tw)
        assert p is not None, (s, B, H, tw)
        out.append(((s, B, H, tw, tw2), p))
    return out


def test_plan_matches_the_documented_arithmetic():
    """n_out = max(nmin, ceil(Vt / segs)), segs = target_waves * WPS / 6, S0 = (7 - n_out % 7) % 7 -- the figures DESIGN.md quotes
    for the cases the suite ran before (256 CUs: target_waves = 1024), and the plan's own consistency on every case."""
    assert dc.plan(0, 3, 3, 1024) == (16, 5, 3, 1, 6) and dc.plan(1, 3, 3, 1024) == (16, 5, 3, 1, 6)
    assert dc.plan(2, 3, 3, 1024)[:3] == (7, 0, 1) and dc.plan(3, 3, 31, 1024)[:3] == (7, 0, 1) and dc.plan(3, 70, 31, 1024)[:3] == (7, 0, 1)
    assert dc.plan(0, 2, 15, 12)[:2] == (17, 4) and dc.plan(0, 2, 20, 12)[:2] == (22, 6) and dc.plan(0, 2, 7, 12)[1] == 5
    assert [dc.plan(2, 2, H, 12)[1:3] for H in range(13, 24, 2)] == [(s0, 2) for s0 in (6, 5, 4, 3, 2, 1)]
    for (s, B, H, tw, _), (n_out, s0, k7, n_seg, n_items) in _plans():
        Vt = B * (H + 3) - 3
        assert n_out == 7 * k7 - s0 and 0 <= s0 < 7 and n_out >= (16 if s < 2 else 7)
        assert (n_seg - 1) * n_out < Vt <= n_seg * n_out and n_items == n_seg * dc.UNITS


def test_plan_refuses_bad_arguments():
    p = _ffi.AcxDwconv7Plan()
    lib = _ffi.lib()
    assert lib.acx_test_dwconv7_plan(0, 2, 7, 12, ctypes.byref(p)) == 0
    for bad in ((4, 2, 7, 12), (-1, 2, 7, 12), (0, 0, 7, 12), (0, 2, 0, 12), (0, 2, 7, 0)):
        assert lib.acx_test_dwconv7_plan(*bad, ctypes.byref(p)) != 0, bad
    assert lib.acx_test_dwconv7_plan(0, 2, 7, 12, None) != 0
    one = (ctypes.c_int64 * 1)(dc.MIN_SAMPLES - 1)
    assert lib.acx_test_dwconv7_varlen_plan(0, one, 1, 12, ctypes.byref(p)) != 0          # too short a clip


def test_every_instantiation_has_a_case_with_a_segment_boundary():
    """All 28 (stage, S0) pairs, each with at least 2 clips and at least 2 segments."""
    seen = {(c[0], p[1]) for c, p in _plans() if c[1] >= 2 and p[3] >= 2}
    missing = [(s, s0) for s in range(4) for s0 in range(7) if (s, s0) not in seen]
    print("uniform (stage, S0) pairs reached: %d of 28" % (28 - len(missing)))
    assert not missing, missing


def test_group_counts():
    """Stages 2-3: k7 = 1, k7 = 2 with S0 >= 2 (no main-loop trip), k7 >= 4.  Stages 0-1: k7 = 3 and k7 >= 5."""
    for s in range(4):
        k7s = [(p[2], p[1]) for c, p in _plans() if c[0] == s]
        if s >= 2:
            assert any(k == 1 for k, _ in k7s) and any(k == 2 and s0 >= 2 for k, s0 in k7s) and any(k >= 4 for k, _ in k7s), (s, k7s)
        else:
            assert any(k == 3 for k, _ in k7s) and any(k >= 5 for k, _ in k7s), (s, k7s)


def test_segment_counts_and_ends():
    """Odd and even n_seg (odd: n_items % 4 = 2, the trailing waves of the last workgroup repeat the last item); a last segment
    that reaches past the last clip and one that ends exactly on it -- per stage."""
    for s in range(4):
        ps = [(c, p) for c, p in _plans() if c[0] == s]
        assert any(p[3] % 2 == 1 and p[3] > 1 and p[4] % 4 == 2 for _, p in ps), s
        assert any(p[3] % 2 == 0 for _, p in ps), s
        ends = [p[3] * p[0] - (c[1] * (c[2] + 3) - 3) for c, p in ps]
        assert any(e > 0 for e in ends) and any(e == 0 for e in ends), (s, ends)


def test_segment_boundaries_fall_everywhere():
    """Per stage: a segment (beyond the first) starts on a clip's first row, on its last row, and inside the three zero rows."""
    for s in range(4):
        kinds = set()
        for (cs, B, H, _, _), p in _plans():
            if cs == s:
                kinds |= {dc.row_kind(v, B, H) for v in dc.segment_starts(p, B, H)[1:]}
        assert {"first", "last", "zero", "inner"} <= kinds, (s, kinds)


def test_short_clips_and_whole_clip_segments():
    """H = 1, 2 and 3 per stage; with H <= 2 seven consecutive stacked rows (a group of steps) span three clips.  One case per stage has H + 3
    dividing n_out."""
    for s in range(4):
        cs = [(c, p) for c, p in _plans() if c[0] == s]
        assert {1, 2, 3} <= {c[2] for c, _ in cs}
        for H in (1, 2):
            Hp = H + 3
            assert any(len({(v0 + i) // Hp for i in range(7)}) >= 3 for v0 in range(Hp))
        assert any(p[0] % (c[2] + 3) == 0 and p[3] >= 2 for c, p in cs), s


def test_second_target_waves_moves_the_boundaries():
    for (s, B, H, tw, tw2), p in _plans():
        q = dc.plan(s, B, H, tw2)
        assert q is not None and q[0] != p[0], (s, B, H, tw, tw2, p, q)


def test_case_tensors_are_small():
    for s, B, H, _, _ in dc.UNIFORM_CASES:
        assert B * H * dc.width(s) * dc.DIMS[s] * 4 <= dc.MAX_TENSOR_BYTES
    for s, lengths, _ in dc.PACKED_CASES:
        assert sum(dc.stage_height(L, s) for L in lengths) * dc.width(s) * dc.DIMS[s] * 4 <= dc.MAX_TENSOR_BYTES
    assert len(dc.STATS_CASES) == 12 and all(sum(c[0] == s for c in dc.STATS_CASES) == 3 for s in range(4))


def test_packed_cases():
    """Mixed heights with the shortest clip the model takes, odd heights in every stage, at least three k7 per stage, several
    segments, all four VAR kernels (one per stage)."""
    stages = set()
    for s in range(4):
        cases = [c for c in dc.PACKED_CASES if c[0] == s]
        k7s, nsegs = set(), set()
        for _, lengths, tw in cases:
            hs = [dc.stage_height(L, s) for L in lengths]
            assert dc.MIN_SAMPLES in lengths and min(lengths) == dc.MIN_SAMPLES
            assert len(set(hs)) >= 4 and any(h % 2 for h in hs) and any(h % 2 == 0 for h in hs) and min(hs) == 8 >> s
            n_out, s0, k7, n_seg, n_items = dc.plan_varlen(s, list(lengths), tw)
            Vt = sum(hs) + 3 * len(hs) - 3
            assert s0 == 0 and n_out == 7 * k7 and (n_seg - 1) * n_out < Vt <= n_seg * n_out and n_items == 6 * n_seg
            k7s.add(k7)
            nsegs.add(n_seg)
            stages.add(s)
        assert len(k7s) >= 3 and min(nsegs) >= 2 and any(n % 2 for n in nsegs), (s, k7s, nsegs)
    print("VAR kernels reached: %d of 4" % len(stages))
    assert stages == {0, 1, 2, 3}


# ---- the guard and the division ------------------------------------------------------------------------------------------------------
GUARD_HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 13, 29, 31, 61, 126, 251, 1000, 4093, 20000, 65530)


def test_guard_sits_at_two_to_the_32():
    """(Vt + 16 Hp + 64) Hp: the largest accepted batch stays below 2^32, one clip more is at or above it (the launcher refuses
    from 2^32 - 1 on)."""
    for H in GUARD_HEIGHTS:
        Hp = H + 3

        def prod(B):
            return (B * Hp - 3 + 16 * Hp + 64) * Hp
        if prod(1) >= 2 ** 32 - 1:
            assert dc.plan(0, 1, H, 12) is None
            continue
        B = dc.largest_batch(H)
        assert prod(B) < 2 ** 32 - 1 <= prod(B + 1), (H, B)
        for s in range(4):
            assert dc.plan(s, B, H, 1024) is not None and dc.plan(s, B + 1, H, 1024) is None
    # Hp = 4: the product is 16 B + 500
    B4 = (2 ** 32 - 1 - 500) // 16
    assert dc.plan(0, B4, 1, 12) is not None and dc.plan(0, B4 + 1, 1, 12) is None


def test_division_by_multiply_high_is_exact_under_the_guard():
    """RESTATEMENT (dc.umulhi_div): umulhi(v + 9 Hp, floor(2^32 / Hp) + 1) == (v + 9 Hp) // Hp for every row index the guard speaks
    for -- v + 9 Hp < Vt + 16 Hp + 64 -- at the top of the range of the largest accepted batch: near every multiple of Hp there
    (where a too-large magic number fails first), and a dense run at the very top.

    The LAST segment of a launch cut into many segments looks further down than that: its flags ask about rows up to
    n_seg n_out + 8, and n_seg n_out exceeds Vt by up to the segment count.  Those rows lie past the last clip; there the quotient
    may be one too large (it is, from Vt + 16 Hp + 70 on at H = 1), the remainder v - n Hp then wraps to a huge unsigned number and
    the row counts as outside every image -- which it is.  Checked too: exact, or past the last clip and one too large."""
    checked = 0
    for H in GUARD_HEIGHTS:
        Hp = H + 3
        if dc.plan(0, 1, H, 12) is None:
            continue
        B = dc.largest_batch(H)
        Vt = B * Hp - 3
        top = Vt + 16 * Hp + 64                                # vv < top
        assert top * Hp < 2 ** 32
        m = np.arange(max(top // Hp - 40000, 0), top // Hp + 1, dtype=np.int64) * Hp
        near = (m[:, None] + np.arange(-3, 3, dtype=np.int64)[None, :]).reshape(-1)
        dense = np.arange(max(top - 200000, 0), top, dtype=np.int64)
        for vv in (near[(near >= 0) & (near < top)], dense):
            assert vv.max() < 2 ** 32
            assert np.array_equal(dc.umulhi_div(vv, Hp), (vv // Hp).astype(np.uint64)), H
            checked += vv.size
        reach = top
        for s in (0, 3):
            for tw in (1, 12, 100, 500, 1000, 1024, 2047, 2048):
                n_out, _, _, n_seg, _ = dc.plan(s, B, H, tw)
                reach = max(reach, n_seg * n_out + 8 + 9 * Hp + 1)
        assert reach < 2 ** 32
        vv = np.arange(top, reach, dtype=np.int64)
        if vv.size:
            q, want = dc.umulhi_div(vv, Hp), (vv // Hp).astype(np.uint64)
            assert top - 9 * Hp >= B * Hp                       # all of them past the last clip
            assert bool(((q == want) | (q == want + np.uint64(1))).all()), H
            wrapped = (vv.astype(np.uint64) - q * np.uint64(Hp)) & np.uint64(0xffffffff)
            assert bool(((q == want) | (wrapped >= np.uint64(H))).all()), H
            checked += vv.size
    print("multiply-high division: %d values checked" % checked)


# ---- the bound notices -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,B,H,tw", [(0, 2, 17, 12), (2, 2, 21, 12)])
def test_bound_passes_fp32_conv_and_notices_a_lost_kernel_row(synth_sd, s, B, H, tw):
    """torch's fp32 conv2d (49 products, its own order) stays inside g49 (|b| + sum |x||w|); the same conv with kernel row 6 left
    out on the first six rows of the second segment lands orders of magnitude outside."""
    x = lr.seeded_input(s, B, H, seed=77 + s)
    ref, bound = dc.conv_ref(synth_sd, s, x)
    assert float(bound.min()) > 0.0
    good = dc.worst_ratio(dc.conv_fp32(synth_sd, s, x), ref, bound)
    p = dc.plan(s, B, H, tw)
    assert p[3] >= 2
    bad = dc.worst_ratio(dc.conv_head_row_lost(synth_sd, s, x, p, 1), ref, bound)
    print("stage %d (%d, %d): fp32 conv2d error / bound %.3f; one kernel row lost at a segment head: %.3g" % (s, B, H, good, bad))
    assert good <= 1.0
    assert bad > 1000.0
