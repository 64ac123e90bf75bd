"""CPU: what the bf16 depthwise-form cases (tests/dwconv_bf16_cases.py) reach, asked from the launcher's own planning function
(acx_test_dwconv7_bf16_plan: no context, no device), the guard and the division of the matrix-pipe kernel, and that the interval
check of tests/test_gpu_dwconv_bf16_forms.py passes a correct fp32 accumulation and notices a lost kernel row and a truncating store."""
import ctypes

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
import dwconv_bf16_cases as bc
import dwconv_cases as dc


def _plans(s):
    """[((B, H, tw), Plan)] of every launch of the stage's cases."""
    out = []
    for cs, B, H, tws in bc.CASES:
        if cs == s:
            for tw in tws:
                p = bc.plan(s, B, H, tw)
                assert not p.too_tall, (s, B, H, tw)
                out.append(((B, H, tw), p))
    return out


def test_plan_matches_the_documented_arithmetic():
    """rows = max(8, ceil4(ceil(Vt / segs))), segs = target_waves / 12, steps = rows / 4, n_seg = ceil(Vt / rows), one group per
    (slice, segment), kGroups groups per workgroup -- on every case; and the production launches DESIGN.md quotes."""
    for s in bc.STAGES:
        for (B, H, tw), p in _plans(s):
            Vt = B * (H + 3) - 3
            segs = max(1, tw // 12)
            rows = max(8, (-(-Vt // segs) + 3) // 4 * 4)
            assert (p.rows, p.steps, p.n_seg) == (rows, rows // 4, -(-Vt // rows)), (s, B, H, tw, p)
            assert p.n_groups == p.n_seg * bc.KSLICES[s] and p.grid == -(-p.n_groups // bc.KGROUPS[s]), (s, B, H, tw, p)
    got = [bc.plan(s, 64, 252 >> s, 8 * 256) for s in bc.STAGES]
    assert [(p.steps, p.n_seg, p.grid) for p in got] == [(24, 170, 255), (13, 159, 239), (7, 151, 227)], got
    # every direct test of the uniform kernel before this one: 2 steps at the shipped setting (256 CUs)
    for s in bc.STAGES:
        for B, H in ((1, 5), (3, 9), (2, 31), (7, 50), (5, 63), (3, 252 >> s)):
            assert bc.plan(s, B, H, 8 * 256).steps == 2
    assert len({(p.rows, p.n_seg) for p in (bc.plan(2, 5, 63, v * 256) for v in (2, 5, 9, 8))}) == 1


def test_plan_refuses_bad_arguments():
    p = _ffi.AcxDwconv7Bf16Plan()
    lib = _ffi.lib()
    assert lib.acx_test_dwconv7_bf16_plan(0, 2, 7, 12, ctypes.byref(p)) == 0
    for bad in ((3, 2, 7, 12), (-1, 2, 7, 12), (0, 0, 7, 12), (0, 2, 0, 12), (0, 2, 7, 0), (0, 2, 7, -5)):
        assert lib.acx_test_dwconv7_bf16_plan(*bad, ctypes.byref(p)) != 0, bad
    assert lib.acx_test_dwconv7_bf16_plan(0, 2, 7, 12, None) != 0
    one = (ctypes.c_int64 * 1)(dc.MIN_SAMPLES - 1)
    assert lib.acx_test_dwconv7_bf16_varlen_plan(0, one, 1, 12, ctypes.byref(p)) != 0          # too short a clip
    ok = (ctypes.c_int64 * 1)(dc.MIN_SAMPLES)
    assert lib.acx_test_dwconv7_bf16_varlen_plan(0, ok, 1, 12, ctypes.byref(p)) == 0 and p.too_tall == 0
    assert lib.acx_test_dwconv7_bf16_varlen_plan(3, ok, 1, 12, ctypes.byref(p)) != 0
    assert lib.acx_test_dwconv7_bf16_varlen_plan(0, ok, 1, 12, None) != 0


@pytest.mark.parametrize("s", bc.STAGES)
def test_step_counts(s):
    """2, 3, 4 and 5 steps (the ring of 16 rows wraps from 3 on: 4 steps + 6 = 18 rows; both parities of steps + 1), one case of at
    least 9 (two wraps or more), and the step count of the stage's B = 64, 10 s launch at 8 waves per CU on 256 CUs."""
    steps = {p.steps for _, p in _plans(s)}
    assert {2, 3, 4, 5} <= steps, (s, steps)
    assert any(4 * n + 6 > 2 * 16 for n in steps) and max(steps) >= 9
    product = bc.plan(s, bc.PRODUCT["B"], 252 >> s, bc.PRODUCT["target_waves"])
    assert product.steps == bc.PRODUCT_STEPS[s] and product.steps in steps, (s, product, steps)
    print("stage %d: step counts %s" % (s, sorted(steps)))


@pytest.mark.parametrize("s", bc.STAGES)
def test_segment_counts_and_grids(s):
    """1, 2 and at least 3 segments; a last workgroup with and without surplus groups (they repeat the last group); grids below 8
    (XCDs without a workgroup), of exactly 8, and of 17 or more with a remainder modulo 8 (the XCD-major renumbering)."""
    ps = [p for _, p in _plans(s)]
    assert {1, 2} <= {p.n_seg for p in ps} and any(p.n_seg >= 3 for p in ps)
    k = bc.KGROUPS[s]
    assert any(p.n_groups % k == 0 for p in ps) and any(p.n_groups % k != 0 for p in ps)
    assert any(p.grid < 8 for p in ps) and any(p.grid == 8 for p in ps) and any(p.grid >= 17 and p.grid % 8 != 0 for p in ps)


@pytest.mark.parametrize("s", bc.STAGES)
def test_segment_starts_fall_everywhere(s):
    """A segment beyond the first starts on a clip's first row, on its last row, on each of the three zero rows and on an interior
    row (clips of at least two rows, so that first and last are different rows)."""
    kinds = set()
    for (B, H, _), p in _plans(s):
        if H >= 2:
            for k in range(1, p.n_seg):
                kinds |= bc.row_kinds(k * p.rows, B, H)
    assert {"first", "last", "zero0", "zero1", "zero2", "inner"} <= kinds, (s, kinds)


@pytest.mark.parametrize("s", bc.STAGES)
def test_last_segments(s):
    """One ends exactly on Vt, one 1 to 3 rows past it, one a whole step or more past it."""
    over = {p.n_seg * p.rows - (B * (H + 3) - 3) for (B, H, _), p in _plans(s)}
    assert min(over) == 0 and over & {1, 2, 3} and max(over) >= 4, (s, over)


@pytest.mark.parametrize("s", bc.STAGES)
def test_clip_shapes(s):
    """Clips of 1, 2 and 3 rows with four clips or more (several clips inside one four-row step; H = 1: H + 3 is the step), H = 5
    (H + 3 = the minimum rows of a segment), B = 1 -- and every tensor small."""
    shapes = {(B, H) for cs, B, H, _ in bc.CASES if cs == s}
    for H in (1, 2, 3):
        assert any(h == H and B >= 4 for B, h in shapes), (s, H)
    assert any(H == 5 and bc.plan(s, B, H, 12).rows == 8 for B, H in shapes)
    assert any(B == 1 for B, _ in shapes)
    for B, H in shapes:
        assert B * H * bc.width(s) * bc.DIMS[s] * 2 <= bc.MAX_TENSOR_BYTES
    # every shape with more than one launch moves its segment boundaries between them
    for cs, B, H, tws in bc.CASES:
        if cs == s:
            assert len({bc.plan(s, B, H, tw).rows for tw in tws}) == len(tws), (s, B, H, tws)


def test_packed_cases():
    """The lengths of dwconv_cases.PACKED_CASES in stages 0-2, each at target_waves that give 2 steps, an odd count, and 9 or more."""
    assert [c[0] for c in bc.PACKED] == list(bc.STAGES)
    for s, lengths, tws in bc.PACKED:
        assert any(c[0] == s and c[1] == lengths for c in dc.PACKED_CASES)
        hs = [dc.stage_height(L, s) for L in lengths]
        Vt = sum(hs) + 3 * len(hs) - 3
        assert sum(hs) * bc.width(s) * bc.DIMS[s] * 2 <= bc.MAX_TENSOR_BYTES
        ps = [bc.plan_varlen(s, list(lengths), tw) for tw in tws]
        for p in ps:
            assert not p.too_tall and p.rows == 4 * p.steps and (p.n_seg - 1) * p.rows < Vt <= p.n_seg * p.rows, (s, p)
            assert p.n_groups == p.n_seg * bc.KSLICES[s] and p.grid == -(-p.n_groups // bc.KGROUPS[s])
        steps = [p.steps for p in ps]
        assert 2 in steps and any(n % 2 == 1 and n > 2 for n in steps) and any(n >= 9 for n in steps), (s, steps)
        assert any(p.n_seg >= 2 for p in ps)
        print("packed stage %d heights %s: steps %s segments %s" % (s, hs, steps, [p.n_seg for p in ps]))


# ---- the guard and the division ------------------------------------------------------------------------------------------------------
GUARD_HEIGHTS = (1, 2, 3, 5, 13, 29, 61, 251, 1000, 4093, 20000, 65530)


def test_guard_sits_at_two_to_the_32():
    """(2 Vt + 16 Hp + 64) Hp: the largest accepted batch stays below 2^32 - 1, one clip more is at or above it."""
    some = 0
    for H in GUARD_HEIGHTS:
        if bc.guard_product(1, H) >= 2 ** 32 - 1:
            assert bc.plan(0, 1, H, 12).too_tall
            continue
        B = bc.largest_batch(H)
        assert bc.guard_product(B, H) < 2 ** 32 - 1 <= bc.guard_product(B + 1, H), (H, B)
        for s in bc.STAGES:
            assert not bc.plan(s, B, H, 2048).too_tall and bc.plan(s, B + 1, H, 2048).too_tall
        some += 1
    assert some >= 8
    # Hp = 4: the product is 32 B + 488
    B4 = (2 ** 32 - 2 - 488) // 32
    assert not bc.plan(0, B4, 1, 12).too_tall and bc.plan(0, B4 + 1, 1, 12).too_tall


def test_division_by_multiply_high_is_exact_under_the_guard():
    """RESTATEMENT (bc.umulhi_div): the kernel divides the first output row of a segment, vb = seg * rows < Vt, and the first row it
    requests shifted into the positive, vb - 3 + Hp < Vt + Hp.  umulhi(v, floor(2^32 / Hp) + 1) == v // Hp for those v at the
    largest accepted batch of each height: every multiple of Hp with its two neighbours -- all of them up to 2^23 clips, above
    that the bottom 2^20, the top 2^22 and every 61st in between -- and a dense run at the very top, where the excess
    v (magic Hp - 2^32) / 2^32 of the multiply-high, which grows with v, is largest."""
    checked = 0
    for H in GUARD_HEIGHTS:
        Hp = H + 3
        if bc.plan(0, 1, H, 12).too_tall:
            continue
        B = bc.largest_batch(H)
        top = B * Hp - 3 + Hp                                  # v < top
        assert top < 2 ** 32
        n = top // Hp + 1
        if n <= 1 << 23:
            m = np.arange(n, dtype=np.int64)
        else:
            m = np.unique(np.concatenate([np.arange(1 << 20, dtype=np.int64), np.arange(1 << 20, n - (1 << 22), 61, dtype=np.int64),
                                          np.arange(n - (1 << 22), n, dtype=np.int64)]))
        dense = np.arange(max(top - 200000, 0), top, dtype=np.int64)
        for off in (-1, 0, 1):
            v = m * Hp + off
            v = v[(v >= 0) & (v < top)]
            assert np.array_equal(bc.umulhi_div(v, Hp), (v // Hp).astype(np.uint64)), (H, off)
            checked += v.size
        assert np.array_equal(bc.umulhi_div(dense, Hp), (dense // Hp).astype(np.uint64)), H
        checked += dense.size
    print("multiply-high division: %d values checked" % checked)


# ---- the cases pin the result, and the check notices ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s,B,H,tws", bc.CASES)
def test_interval_pins_the_cases_and_passes_an_fp32_conv(synth_sd, s, B, H, tws):
    """From the reference alone: at least 95 % of a case's elements have bf16(ref - E) == bf16(ref + E), so that the check is an
    equality with the rounded exact sum there; and torch's fp32 conv2d (exact products, its own order of sums), rounded to bf16,
    lies inside every interval."""
    x, R = bc.case_reference(synth_sd, s, B, H)
    assert float(R.E.min()) > 0.0 and bool((R.lo <= R.exact).all()) and bool((R.exact <= R.hi).all())
    share = R.pinned_share()
    y = bc.conv_fp32(synth_sd, s, x).to(torch.bfloat16)
    print("stage %d (%d, %d): %.2f %% of the elements pinned to one bf16 value; fp32 conv2d: %.2f %% the rounded exact sum"
          % (s, B, H, 100 * share, 100 * R.exact_share(y)))
    assert share >= bc.MIN_EXACT_SHARE, (s, B, H, share)
    assert not bool(R.outside(y).any()), (s, B, H, int(R.outside(y).sum()))


def test_packed_intervals_pin_too(synth_sd):
    for s, lengths, _ in bc.PACKED:
        x, hs, R = bc.packed_reference(synth_sd, s, lengths)
        assert x.shape[0] == sum(hs) and R.pinned_share() >= bc.MIN_EXACT_SHARE, (s, R.pinned_share())
        r0, parts = 0, []
        for h in hs:
            parts.append(bc.conv_fp32(synth_sd, s, x[r0:r0 + h][None])[0])
            r0 += h
        assert not bool(R.outside(torch.cat(parts).to(torch.bfloat16)).any())


@pytest.mark.parametrize("s", bc.STAGES)
def test_check_notices_a_lost_kernel_row_and_a_truncating_store(synth_sd, s):
    """The rounded exact sum with kernel row 6 dropped on ONE output row: more than 99 % of that row lies outside.  A store that
    truncates instead of rounding to nearest: more than 45 % of all elements (every element whose dropped bits are above half a
    step, less those whose interval spans both neighbours)."""
    B, H = 5, 18
    x, R = bc.case_reference(synth_sd, s, B, H)
    n, r = 2, 7
    bad = bc.conv_row_lost(synth_sd, s, x, n, r)
    out = R.outside(bad)
    row = out[n, r]
    assert int(out.sum()) == int(row.sum()), "only that row was changed"
    trunc = R.outside(bc.bf16_trunc(bc.conv_fp32(synth_sd, s, x)))
    print("stage %d: kernel row 6 lost on one output row: %d of %d elements of the row outside; truncating store: %.1f %% of all outside"
          % (s, int(row.sum()), row.numel(), 100 * float(trunc.double().mean())))
    assert float(row.double().mean()) > 0.99
    assert float(trunc.double().mean()) > 0.45
