"""The helper behind the bf16 GPU tests (tests/bf16_ref.py), checked on the CPU: pins of the device GELUs' coefficients, the error
of the restated forms, the emulations against the float64 oracle, the exclusion caps of the GELU probe on its own inputs -- and
that the bars notice a wrong kernel, shown by perturbing the restatement that stands in for the device."""
import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import synth
import bf16_ref as br
import layer_ref as lr

PRECISIONS = ("bf16", "bf16a")


def _erf_gelu(v):
    from scipy.special import erf
    return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))


# ---- pins ------------------------------------------------------------------------------------------------------------------------
def test_shipped_gelu2h_coefficients_are_the_pinned_ones():
    """gelu_k2h carries the helper's three literals with the factors 2, 4, 8 of the unit z = 0.5 v, and the packers' halving of W1
    that this unit depends on is switched on."""
    coeff, half_w1 = br._gelu2h_constants_in_source()
    assert tuple(c for c, _ in coeff) == br.GELU2H_C
    assert tuple(s for _, s in coeff) == br.GELU2H_SCALE == (2.0, 4.0, 8.0)
    assert half_w1 == "true"
    assert all(lr._f32c(c) == c for c in br.GELU2H_C)             # fp32 values: the literal is the coefficient


def test_shipped_gelu3_unit_coefficients_are_gelu3s():
    """gelu3_unit is a second literal copy of gelu_k3's coefficients, pre-multiplied by 1 / 0.5^(j+1)."""
    coeff = br._gelu3_unit_constants_in_source()
    assert tuple(c for c, _ in coeff) == lr.GELU3_K
    assert tuple(s for _, s in coeff) == br.GELU3_UNIT_SCALE == tuple(2.0 ** (j + 1) for j in range(5))


def test_registry_names_a_form_per_stage_and_leaves_layer_ref_alone():
    assert set(lr.DEVICE_GELU) == {"fp32", "fp32_split"}
    for prec in PRECISIONS:
        assert [br.device_gelu(prec, s) for s in range(4)] == [br._gelu2h_fp32] * 3 + [br._gelu3_unit_fp32]


# ---- form error --------------------------------------------------------------------------------------------------------------------
V_GRID = np.linspace(-20.0, 20.0, 800001)


def test_gelu2h_form_error():
    """The header's own claim, |error| <= 8.6e-5 (worst near v = 2.9); at most half a bf16 step of the result wherever
    |gelu| > 0.044; far out v itself, or exactly 0, with no NaN on the way (asserted inside the restatement)."""
    ref = _erf_gelu(V_GRID)
    err = np.abs(br._gelu2h_fp32(V_GRID) - ref)
    print("gelu2h: max error %.3g at v = %.3f" % (err.max(), V_GRID[err.argmax()]))
    assert err.max() <= br.GELU2H_CLAIM, (err.max(), V_GRID[err.argmax()])
    big = np.abs(ref) > 0.044
    rel = err[big] / (2.0 ** -9 * np.abs(ref[big]))
    print("gelu2h: worst error %.3f of 2^-9 |gelu| where |gelu| > 0.044" % rel.max())
    assert rel.max() <= 1.0
    far = np.array([1e3, 1e4])
    assert np.array_equal(br._gelu2h_fp32(far), far)
    assert (br._gelu2h_fp32(-far) == 0.0).all()


def test_gelu3_unit_form_error():
    """The bound tests/test_split_arithmetic_cpu.py::test_gelu_third_form_error_bound gives the third form; and gelu3_unit IS that
    form at kh = 1."""
    ref = _erf_gelu(V_GRID)
    g = br._gelu3_unit_fp32(V_GRID)
    err = np.abs(g - ref)
    assert err.max() <= 1.1e-6, (err.max(), V_GRID[err.argmax()])
    small = np.abs(V_GRID) < 0.25
    assert (err[small] <= 6e-6 * np.abs(ref[small]) + 1e-12).all()
    assert np.array_equal(g, lr._gelu3_fp32(V_GRID, 1.0))
    far = np.array([20.0, 1e3, 1e4])
    assert np.array_equal(br._gelu3_unit_fp32(far), far)
    assert (br._gelu3_unit_fp32(-far) == 0.0).all()


def test_a_moved_gelu2h_coefficient_fails_the_form_error():
    """Any of the three coefficients moved by 1 % breaks the header's claim."""
    ref = _erf_gelu(V_GRID)
    for j in range(3):
        for f in (0.99, 1.01):
            c = list(br.GELU2H_C)
            c[j] *= f
            assert np.abs(br._gelu2h_fp32(V_GRID, c=c) - ref).max() > br.GELU2H_CLAIM, (j, f)


def test_restatements_take_torch_and_numpy_and_leave_their_input_alone():
    v = torch.linspace(-9.0, 9.0, 1001, dtype=torch.float64)
    keep = v.clone()
    for form in (br._gelu2h_fp32, br._gelu3_unit_fp32):
        a = form(v)
        assert torch.equal(v, keep) and a.dtype == torch.float64
        assert np.array_equal(form(v.numpy()), a.numpy())
        assert torch.equal(form(v.float()), form(v.float().double()))     # fp32 in: float64 out, of the same values


# ---- the emulation is an emulation of the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_emulations_stay_within_the_drift_bars_of_the_float64_oracle(precision):
    """With the exact GELU: one small shape per stage against layer_ref.block_case / downsample_case at the drift bar of
    tests/test_gpu_bf16.py (plus one bf16 step per element where the result is stored as bf16); the device forms move the block by
    far less than that."""
    sd = synth.synth_state_dict(0)
    sd64 = lr.to64(sd)
    for s, (B, H) in enumerate(((1, 5), (1, 5), (1, 5), (1, 9))):
        x = lr.seeded_input(s, B, H, seed=40 + s)
        case = lr.block_case(sd, sd64, s, 1, lr.nchw(x))
        emu = br._block_emulation(precision, sd, s, 1, lr.nchw(x))
        err = (emu - case.ref).abs()
        print("block s%d %s: emulation vs float64 %.3g" % (s, precision, float(err.max())))
        assert bool((err < br.DRIFT_LAYER_TOL + br.store_step(case.ref, br.act_bf16(precision, s))).all())
        assert float(err.max()) > 1e-5                                     # (it does round its operands)
        dev64, dev32 = br.block_pair(precision, sd, s, 1, x)
        bar = br.store_step(emu, br.act_bf16(precision, s)).clamp_min(br.EMU_TOL)
        assert bool(((dev64 - emu).abs() <= bar).all()) and bool(((dev32 - dev64).abs() <= bar).all())
    for i in (1, 2, 3):
        x = lr.seeded_input(i - 1, 1, 7, seed=50 + i)
        case = lr.downsample_case(sd, sd64, i, lr.nchw(x))
        emu64, emu32 = br.downsample_pair(sd, i, x)
        plain = br._downsample_emulation(sd, i, x).permute(0, 2, 3, 1)           # (LayerNorm by torch in fp32: the odd row rounds the other way)
        assert float((emu64 - plain).abs().max()) < br.EMU_TOL and float((emu64 - plain).abs().median()) == 0.0
        err = float((emu64 - case.ref).abs().max())
        print("downsample %d: emulation vs float64 %.3g" % (i, err))
        assert 1e-5 < err < br.DRIFT_LAYER_TOL and float((emu32 - emu64).abs().max()) < br.EMU_TOL


def test_running_fp32_layernorm():
    """The stand-in's LayerNorm is a LayerNorm -- within half of the GELU probe's exclusion zone of float64 (64 fp32 steps of the
    value or 16 of the row's scale: a small output keeps the rounding of the mean) -- and further from float64 than torch's
    blocked sums, which is why it is the stand-in."""
    for C in (96, 768):
        x = torch.randn(500, C, generator=torch.Generator().manual_seed(C)) * 1.5 + 0.3
        ref = br.ln_plain(x.double(), C)
        run, blocked = br.ln_running_fp32(x, C), br.ln_plain(x, C).double()
        zone = (br.BOUNDARY_REL * ref.abs()).clamp_min(br.BOUNDARY_ABS)
        print("C = %d: running fp32 LayerNorm at most %.3f of the exclusion zone from float64" % (C, float(((run - ref).abs() / zone).max())))
        assert bool(((run - ref).abs() < 0.5 * zone).all())
        assert float((run - ref).abs().mean()) > 1.5 * float((blocked - ref).abs().mean())


def test_tail_pair_is_the_chain_of_the_two_emulations():
    sd = synth.synth_state_dict(0)
    x = lr.seeded_input(1, 1, 10, seed=3)
    for precision in PRECISIONS:
        x_new = br._block_emulation(precision, sd, 1, 2, lr.nchw(x), store=False, gelu=br._gelu2h_fp32, ln_acc=True)
        emu = br._downsample_emulation(sd, 2, x_new, ln_acc=True).permute(0, 2, 3, 1)
        if precision == "bf16a":
            emu = emu.float().to(torch.bfloat16).double()
        emu64, emu32 = br.tail_pair(precision, sd, 1, x)
        assert torch.equal(emu64, emu) and emu64.shape == (1, 5, 14, 384)
        b64, b32 = br.block_pair(precision, sd, 1, 1, x)
        assert torch.equal(b64, br._block_emulation(precision, sd, 1, 1, lr.nchw(x), gelu=br._gelu2h_fp32, ln_acc=True))
        assert not torch.equal(b32, b64)
        assert 0.0 < float((emu32 - emu64).abs().max()) < 2 * br.EMU_TOL + 2.0 ** -7 * float(emu.abs().max())


def _third_draw(precision, sd, s, x):
    """A third draw of the process, in the device's place: accumulated in fp32 like the stand-in, but with torch's LayerNorm."""
    return br._block_emulation(precision, sd, s, 1, lr.nchw(x), acc=torch.float32, gelu=br.device_gelu(precision, s))


# (stage, (B, H)): 280 and 2 072 rows at C = 192 (the shapes of the two-pixel-tile form), 651 rows at stage 3, 7 rows, 10 080 rows
SMALL_AND_LARGE = [(1, (1, 10)), (1, (2, 37)), (3, (3, 31)), (3, (1, 1)), (0, (4, 45))]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("s,shape", SMALL_AND_LARGE)
def test_check_emulation_passes_another_draw_and_sees_a_wrong_result(s, shape, precision):
    """An independent draw of the same arithmetic passes every bar at every size.  A result with an error added before the store
    does not, while still under the ceiling: every output off by 2e-3, one element in ten off by 3e-3, three in ten off by 3e-3,
    one row in four off by 1e-3.  (7 rows: the counts cannot tell three rows from chance; the errors on every row are seen.)"""
    sd = synth.synth_state_dict(0)
    x = lr.seeded_input(s, *shape, seed=8)
    emu64, emu32 = br.block_pair(precision, sd, s, 1, x)
    stored = br.act_bf16(precision, s)
    rows = emu64.numel() // emu64.shape[-1]

    def store(t):
        return t.float().to(torch.bfloat16).double() if stored else t.float().double()
    clean = _third_draw(precision, sd, s, x)
    assert br.check_emulation("a third draw", clean, emu64, emu32, stored) <= 2.0
    pre = br._block_emulation(precision, sd, s, 1, lr.nchw(x), store=False, acc=torch.float32, gelu=br.device_gelu(precision, s))
    n = pre.numel()
    every_tenth = (torch.arange(n) % 10 == 0).view(pre.shape)
    three_in_ten = (torch.arange(n) % 10 < 3).view(pre.shape)
    row_in_four = (torch.arange(rows) % 4 == 0).view(pre.shape[:-1])[..., None].expand_as(pre)
    wrong = {"all 2e-3": pre + 2e-3, "tenth 3e-3": pre + 3e-3 * every_tenth, "three tenths 3e-3": pre + 3e-3 * three_in_ten}
    if rows >= 64:
        wrong["row in four 1e-3"] = pre + 1e-3 * row_in_four
    for what, bad in wrong.items():
        with pytest.raises(AssertionError, match="median|rows|share"):
            br.check_emulation(what, store(bad), emu64, emu32, stored)
    bad = clean.clone()
    bad[0, 0, 1, 3] += 2 * br.EMU_TOL + 2.0 ** -6 * float(bad[0, 0, 1, 3].abs())
    with pytest.raises(AssertionError, match="ceiling"):
        br.check_emulation("one element", bad, emu64, emu32, stored)


def test_count_allowance():
    assert br._count_allowed(7, 0.04) == 3 and br._count_allowed(7, 0.4) == 7 and br._count_allowed(2072, 0.04) < 130
    assert br._count_allowed(100, 1.0) == 100 and br._count_allowed(73640, 4.0 / 73641) <= 16


# ---- the GELU probe of the GPU tests, with the restatement in the device's place -----------------------------------------------------
def test_boundary_mask():
    one = 1.0 + 2.0 ** -8                                                  # the midpoint of the bf16 neighbours 1 and 1 + 2^-7
    t = torch.tensor([one, one * (1 + 2.0 ** -19), one * (1 - 2.0 ** -19), one * (1 + 2.0 ** -17), 1.0, -one,
                      2.0 ** -6 * one, 2.0 ** -6 * one + 2.0 ** -21, 2.0 ** -6 * one - 2.0 ** -19, 2.0 ** -6],
                     dtype=torch.float64)         # (the last four: a small value, where the zone is the absolute one)
    assert br.near_bf16_boundary(t).tolist() == [True, True, True, False, False, True, True, True, False, False]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_probe_exclusions_and_form_error_on_its_own_inputs(s, precision):
    """What the GPU test assumes of its inputs, computed from them: at most 0.5 % of the elements sit at a rounding boundary of
    LN(x), the arguments cover the range, and the restated form's error over them (G of the bound) is within the header's claim."""
    import test_gpu_bf16_shapes as T
    sd = synth.synth_state_dict(0)
    form = br.device_gelu(precision, s)
    excluded = total = 0
    seen = []
    for _, j, k, x, v, excl, far in T._probe_cases(sd, precision, s):
        keep = ~excl[..., ~far]
        vk = v[..., ~far][keep]
        G = float((form(vk) - lr.gelu_exact(vk)).abs().max())
        assert G <= (br.GELU2H_CLAIM if s < 3 else 1.1e-6), (s, k, G)
        excluded, total = excluded + int((~keep).sum()), total + keep.numel()
        seen.append(vk)
        if br.act_bf16(precision, s):
            assert torch.equal(x, x.to(torch.bfloat16).float()) and 0.03 < float(x.std()) < 0.1
    print("probe s%d %s: %.3f %% of %d elements left out" % (s, precision, 100.0 * excluded / total, total))
    assert 0 < excluded <= br.EXCLUDED_CAP * total
    T._check_coverage(torch.cat(seen))


class _Stub:
    """The block emulation accumulated in fp32, with the given GELU, in the device's place."""

    def __init__(self, sd, precision):
        self.sd, self.precision = sd, precision

    def native_context(self, device):
        return self


def _stand_in(monkeypatch, T, gelu):
    monkeypatch.setattr(T, "_make_model", _Stub)
    monkeypatch.setattr(T, "_run_block", lambda c, s, j, x: br._block_emulation(
        c.precision, c.sd, s, j, lr.nchw(x), acc=torch.float32, gelu=gelu(s)).float())


@pytest.mark.parametrize("precision,s", [("bf16", 0), ("bf16a", 1), ("bf16", 3)])
def test_probe_passes_with_the_restated_form(monkeypatch, precision, s):
    import test_gpu_bf16_shapes as T
    _stand_in(monkeypatch, T, lambda st: br.device_gelu(precision, st))
    T._check_device_gelu(synth.synth_state_dict(0), precision, s)


@pytest.mark.parametrize("j", [0, 1, 2])
def test_probe_sees_a_gelu2h_coefficient_moved_by_one_percent(monkeypatch, j):
    """On the "device" side only -- what a kernel built from an edited header computes: the per-element bound of the probe fails,
    and without it the binned means fail on their own."""
    import test_gpu_bf16_shapes as T
    c = list(br.GELU2H_C)
    c[j] *= 1.01
    _stand_in(monkeypatch, T, lambda st: (lambda v: br._gelu2h_fp32(v, c=c)))
    with pytest.raises(AssertionError, match="per element"):
        T._check_device_gelu(synth.synth_state_dict(0), "bf16", 0)
    with pytest.raises(AssertionError, match="binned"):
        T._check_device_gelu(synth.synth_state_dict(0), "bf16", 0, per_element=False)


def test_probe_sees_a_kernel_that_does_not_halve_b1(monkeypatch):
    """The packers store 0.5 W1; a kernel that staged b1 instead of 0.5 b1 would evaluate the form at z = 0.5 W1 x + b1."""
    import test_gpu_bf16_shapes as T
    sd = synth.synth_state_dict(0)

    def device(c, s, j, x):
        b1 = c.sd["stages.%d.%d.pwconv1.bias" % (s, j)].double()
        return br._block_emulation(c.precision, c.sd, s, j, lr.nchw(x), acc=torch.float32,
                                   gelu=lambda v: br._gelu2h_fp32(0.5 * v.double() + 0.5 * b1, v_is_z=True)).float()
    monkeypatch.setattr(T, "_make_model", _Stub)
    monkeypatch.setattr(T, "_run_block", device)
    with pytest.raises(AssertionError, match="per element"):
        T._check_device_gelu(sd, "bf16", 0)
    monkeypatch.setattr(T, "_probe_check_far", lambda *a: None)
    with pytest.raises(AssertionError, match="binned"):
        T._check_device_gelu(sd, "bf16", 0, per_element=False)
