"""What tests/test_gpu_stem_forms.py rests on, shown on the CPU from the references alone (tests/stem_cases.py): bars below
LAYER_TOL, probes that discriminate, row pairs that straddle clips, workgroups that walk a third row pair."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
import layer_ref as lr
import stem_cases as sc


def _all_cases(synth_sd):
    for B, T in sc.UNIFORM:
        yield (B, T, "randn3"), sc.case(synth_sd, B, T)
    for kind in ("offset", "eps"):
        yield sc.PROBE_SHAPE + (kind,), sc.case(synth_sd, *sc.PROBE_SHAPE, kind)


def test_bars_come_from_the_reference_and_sit_below_the_cap(synth_sd):
    """Every case: noise32 > 0 and 8 noise32 < LAYER_TOL, so the cap is never the bar; the shapes are the stem's."""
    for key, (x, case, _) in _all_cases(synth_sd):
        B, T = key[:2]
        assert case.ref.shape == (B, sc.h0(T), sc.W0, sc.C0) and case.ref.dtype == torch.float64 and case.G == {}
        bar = case.bar("fp32_split")
        print("stem case %s: noise32 %.3g, bar %.3g, max |ref| %.3g" % (key, case.noise32, bar, float(case.ref.abs().max())))
        assert case.noise32 > 0.0 and lr.SPLIT_FACTOR * case.noise32 < lr.LAYER_TOL, (key, case.noise32)
        assert bar == lr.SPLIT_FACTOR * case.noise32 == case.bar("fp32") == case.bar("bf16a")
        if key[2] == "randn3":
            assert 1e-7 < bar < lr.LAYER_TOL / 3.0, (key, bar)           # (about 6e-6 .. 9e-6: a tenth of the fixed bar)


def test_reference_equals_unfold_and_matmul(synth_sd):
    """oracle/ref_cpu.py's stem in float64 against a restatement that shares neither conv2d nor the LayerNorm with it; the fp32
    chain restatement is an fp32 statement of the same layer."""
    sd64 = lr.to64(synth_sd)
    for B, T in sc.UNIFORM:
        x, case, _ = sc.case(synth_sd, B, T)
        assert float((sc.stem_unfold(sd64, x.double()) - case.ref).abs().max()) < 1e-12, (B, T)
        y = sc.conv(sd64, x.double())
        assert float((sc.layer_norm(y, sd64["downsample_layers.0.1.weight"], sd64["downsample_layers.0.1.bias"]) - case.ref).abs().max()) < 1e-12
        chain = sc.chain32(synth_sd, x)
        assert chain.dtype == torch.float32 and float((chain.double() - case.ref).abs().max()) <= case.noise32
    # a row wholly in the zero padding is the LayerNorm of the bias at every pixel: row 0 always (frames -4 .. -1), and at T = 4 the
    # last row (frames 4 .. 7) too
    x, case, _ = sc.case(synth_sd, 1, 4)
    for h, flat in ((0, True), (1, False), (2, True)):
        d = float((case.ref[0, h] - case.ref[0, h, :1]).abs().max())
        assert d < 1e-12 if flat else d > 0.1, (h, d)


def test_offset_probe_separates_the_two_variance_forms(synth_sd):
    """randn + 50 on the variance probe's weights: the kernel's chain in fp32 with a two-pass variance stays inside the bar (by
    construction of noise32: at most an eighth of it); the same chain with var = E[y^2] - mean^2 is several bars outside.  On the
    plain case both are inside LAYER_TOL -- test_stem_kernel_shapes cannot tell them apart.  (On the synthetic weights themselves
    randn + 50 leaves the per-pixel mean small: hence the probe's weights.)"""
    x, case, sd = sc.case(synth_sd, *sc.PROBE_SHAPE, "offset")
    bar = case.bar("fp32")
    y = sc.conv(lr.to64(sd), x.double())
    ratio = (y.mean(-1).abs() / y.std(-1, unbiased=False))[:, 1:-1]        # rows whose four frames all exist
    plain = sc.conv(lr.to64(synth_sd), x.double())
    two = float((sc.chain32(sd, x).double() - case.ref).abs().max())
    one = float((sc.chain32(sd, x, "one_pass").double() - case.ref).abs().max())
    print("offset probe: |mean| / std in [%.3g, %.3g]; two-pass %.3g, one-pass %.3g, bar %.3g"
          % (float(ratio.min()), float(ratio.max()), two, one, bar))
    assert float(ratio.min()) > 25.0
    assert float((plain.mean(-1).abs() / plain.std(-1, unbiased=False)).max()) < 1.0
    assert two <= bar / 8.0 and one > 4.0 * bar
    xp, cp, _ = sc.case(synth_sd, *sc.PROBE_SHAPE)
    assert float((sc.chain32(synth_sd, xp, "one_pass").double() - cp.ref).abs().max()) < lr.LAYER_TOL


def test_eps_probe_moves_the_reference_by_a_hundred_bars(synth_sd):
    """The eps probe's float64 reference without eps, and with eps outside the square root, is more than 100 bars away from the
    reference (it moves by 0.7) -- while on the synthetic weights themselves (var(y) >= 9e-3, reached in the rows of padding) either
    moves it by no more than twice LAYER_TOL, the bar of test_stem_kernel_shapes."""
    x, case, sd = sc.case(synth_sd, *sc.PROBE_SHAPE, "eps")
    sd64 = lr.to64(sd)
    y = sc.conv(sd64, x.double())
    lw, lb = sd64["downsample_layers.0.1.weight"], sd64["downsample_layers.0.1.bias"]
    var = y.var(-1, unbiased=False)
    bar = case.bar("fp32")
    live = var > 0.0            # (a row wholly in the padding is the constant bias: var = 0, and without eps 0 / 0)
    assert bool((~live[:, 0]).all()) and bool(live[:, 1:].all())
    assert bool(sc.layer_norm(y, lw, lb, "no_eps")[~live].isnan().all())
    moved = {f: float((sc.layer_norm(y, lw, lb, f) - case.ref)[live].abs().max()) for f in ("no_eps", "eps_outside")}
    print("eps probe: var(y) in [%.3g, %.3g], bar %.3g, no eps moves %.3g, eps outside the root %.3g"
          % (float(var.min()), float(var.max()), bar, moved["no_eps"], moved["eps_outside"]))
    assert float(var.min()) < 1e-5 and float(var.max()) > 1e-8
    assert min(moved.values()) > 100.0 * bar, (moved, bar)
    xp, cp, _ = sc.case(synth_sd, *sc.PROBE_SHAPE)
    s64 = lr.to64(synth_sd)
    yp = sc.conv(s64, xp.double())
    assert float(yp.var(-1, unbiased=False).min()) >= 9e-3
    for f in ("no_eps", "eps_outside"):
        assert float((sc.layer_norm(yp, lw, lb, f) - cp.ref).abs().max()) < 2.0 * lr.LAYER_TOL


def test_uniform_shapes_cover_the_row_pair_edges():
    rows = {bt: bt[0] * sc.h0(bt[1]) for bt in sc.UNIFORM}
    # row h reads frames 4 h - 4 .. 4 h - 1: row 0 lies wholly in the padding in front; the last row has 1, 2, 3 frames (T = 1, 2, 3),
    # none (T = 4: wholly in the padding behind) or 1 (T = 5)
    assert [sc.h0(T) for T in (1, 2, 3, 4, 5)] == [2, 2, 2, 3, 3]
    assert [T - (4 * sc.h0(T) - 8) for T in (1, 2, 3, 4, 5)] == [1, 2, 3, 0, 1]
    assert rows[(3, 23)] == 21 and sc.h0(23) == 7                   # odd H0: the pair of rows 6, 7 straddles clips 0 and 1
    assert rows[(1, 101)] == 27 and rows[(2, 100)] == 54
    assert any(r % 2 for r in rows.values()) and any(r % 2 == 0 for r in rows.values())
    assert sc.h0(23) * 4 - 4 > 23 - 4 and (23 + 4) % 4 != 0           # the last row is partly padding


def test_packed_case_geometry_from_the_library():
    """The facts the packed case is chosen for, from varlen_geometry's own row counts (acx_test_stem_scratch_bytes on every prefix
    of the batch) and from the restated H0 alike."""
    off = sc.row_offsets(sc.PACKED)
    hs = [b - a for a, b in zip(off, off[1:])]
    assert tuple(hs) == sc.PACKED_H0 == tuple(sc.h0(sc.frames(L)) for L in sc.PACKED)
    assert off[-1] == 143 and off[-1] % 2 == 1
    # odd boundaries: behind clips 0, 1 and 3 the parity changes; clips 4 and 5 have even heights and keep it odd up to the end
    assert off == [0, 15, 23, 62, 101, 115, 135, 143]
    assert [k for k in range(len(hs)) if off[k + 1] % 2 == 1] == [0, 1, 3, 4, 5, 6]
    assert sc.PACKED[2] == sc.PACKED[3] and min(sc.PACKED) == sc.MIN_SAMPLES and sc.PACKED[-1] == sc.MIN_SAMPLES + 1
    x, clips = sc.packed_input(sc.PACKED, 7)
    assert x.shape == (sum(sc.frames(L) for L in sc.PACKED), sc.MELS) and len(clips) == 7
    assert not torch.equal(clips[2], clips[3])                      # equal lengths, different frames


def test_walk_counts():
    """(1, 101) under max_blocks 1, 2, 3 and (33, 1005) at the launcher's grid: pairs per workgroup, and the rule the walk tests rest
    on -- some workgroup makes a second trip of the loop unrolled by two, so a refilled pa* is consumed."""
    B, T = sc.WALK_SHAPE
    npairs = sc.pairs(B * sc.h0(T))
    assert npairs == 14
    want = {1: [14], 2: [7, 7], 3: [5, 5, 4]}
    for cap in sc.WALK_CAPS:
        g = sc.grid(npairs, cap)
        assert sc.walk(npairs, g) == want[cap] and sum(want[cap]) == npairs
        assert max(sc.loop_trips(npairs, g)) >= 2
    assert sc.grid(npairs) == 14 and max(sc.loop_trips(npairs, 14)) == 1        # uncapped: one pair each, the loop's first trip only
    B, T = sc.BIG_SHAPE
    assert sc.h0(T) == 253 and B * sc.h0(T) == 8349 and B % sc.BIG_DISTINCT == 0
    npairs = sc.pairs(8349)
    g = sc.grid(npairs)
    assert npairs == 4175 > 2 * sc.MAX_BLOCKS and g == sc.MAX_BLOCKS
    w = sc.walk(npairs, g)
    assert sum(w) == npairs and w.count(3) == 4175 - 2 * 2048 == 79 and w.count(2) == 2048 - 79
    assert max(sc.loop_trips(npairs, g)) == 2
    # the largest case of test_stem_kernel_shapes, (64, 311), does not get there
    assert max(sc.loop_trips(sc.pairs(64 * sc.h0(311)), sc.grid(sc.pairs(64 * sc.h0(311))))) == 1


def test_stem_scratch_size_and_refusals():
    """acx_test_stem_scratch_bytes needs no context: the geometry tables of the packed forwards, in 256-byte pieces."""
    lib = _ffi.lib()
    arr, need, rows = sc.scratch_bytes(sc.PACKED)
    dw = ctypes.c_size_t()
    assert lib.acx_test_dwconv7_varlen_scratch_bytes(arr, len(sc.PACKED), ctypes.byref(dw)) == 0
    assert need == dw.value and need % 256 == 0 and need >= 4 * rows and rows == 143
    out, r = ctypes.c_size_t(), ctypes.c_int64()
    assert lib.acx_test_stem_scratch_bytes(arr, len(sc.PACKED), ctypes.byref(out), None) == 0 and out.value == need
    assert lib.acx_test_stem_scratch_bytes(arr, len(sc.PACKED), None, ctypes.byref(r)) != 0
    assert lib.acx_test_stem_scratch_bytes(None, len(sc.PACKED), ctypes.byref(out), ctypes.byref(r)) != 0
    assert lib.acx_test_stem_scratch_bytes(arr, 0, ctypes.byref(out), ctypes.byref(r)) != 0
    assert lib.acx_test_stem_scratch_bytes(arr, 257, ctypes.byref(out), ctypes.byref(r)) != 0
    short = (ctypes.c_int64 * 2)(sc.MIN_SAMPLES, sc.MIN_SAMPLES - 1)
    assert lib.acx_test_stem_scratch_bytes(short, 2, ctypes.byref(out), ctypes.byref(r)) != 0
    assert "too short" in lib.acx_last_error().decode()


def test_guarded_takes_a_dtype():
    """layer_ref.Guarded with bf16 payloads: the values, the canaries on both sides, an overrun of one element."""
    t = torch.arange(2 * 3 * 96, dtype=torch.float32).view(2, 3, 96).to(torch.bfloat16)
    g, v = lr.Guarded.tensor(t, device="cpu")
    assert v.dtype == torch.bfloat16 and torch.equal(v, t) and g.intact() and v.data_ptr() - g.buf.data_ptr() == 256
    go, out = lr.Guarded.filled((5, 96), device="cpu", dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.shape == (5, 96) and bool(out.float().isnan().all()) and go.intact()
    with pytest.raises(AssertionError):
        lr.assert_clean(out, go)
    out.fill_(1.0)
    lr.assert_clean(out, go)
    go.buf.view(torch.bfloat16)[2 * lr.GUARD_WORDS + out.numel()] = 0.0          # the half-word behind the last element
    assert not go.intact()
    h = sc.half_step_bf16(torch.tensor([1.0, 1.99, -3.0, 0.3], dtype=torch.float64), 0.0)
    assert h.tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -10]
