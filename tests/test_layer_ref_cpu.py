"""The helper behind the GPU layer tests (tests/layer_ref.py), checked on the CPU: a reference that is wrong, a bar that is slack or a
guard that does not see an overrun would make those tests pass for nothing."""
import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import synth
import layer_ref as lr


def test_restated_gelu_erf_error_bound():
    """gelu_erf (A&S 7.1.26, device_common.h) restated: |erf error| <= 1.5e-7 gives |gelu error| <= 0.75e-7 |v|, plus the fp32
    rounding of the result and of exp(-v^2 / 2)'s argument; far out it is v, or 0."""
    from scipy.special import erf
    v = np.linspace(-12.0, 12.0, 480001)
    ref = 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))
    err = np.abs(lr._gelu_erf_fp32(v) - ref)
    assert err.max() <= 1.1e-6, (err.max(), v[err.argmax()])
    assert (err <= 0.75e-7 * np.abs(v) + 2.0 ** -23 * np.abs(ref) + 4e-7).all()
    far = np.array([20.0, 1e3, 1e10, 1e30])
    assert np.array_equal(lr._gelu_erf_fp32(far), far.astype(np.float32).astype(np.float64))
    assert (lr._gelu_erf_fp32(-far) == 0.0).all()


def test_restatements_take_torch_and_numpy_and_leave_their_input_alone():
    v = torch.linspace(-9.0, 9.0, 1001, dtype=torch.float64)
    keep = v.clone()
    for form in lr.DEVICE_GELU.values():
        a = form(v)
        assert torch.equal(v, keep) and a.dtype == torch.float64
        assert np.array_equal(form(v.numpy()), a.numpy())
        assert float((a - lr.gelu_exact(v)).abs().max()) <= 1.1e-6


def test_block_case_is_the_oracle_and_its_bar_is_tight():
    """The float64 block of the helper is oracle/ref_cpu.py's block in float64; G computed through the linear tail equals a second
    full pass with the restated GELU; and the bar lands a factor 3 or more under LAYER_TOL (a bar at LAYER_TOL would say nothing
    the old per-layer tests do not say)."""
    from oracle import ref_cpu
    sd = synth.synth_state_dict(0)
    sd64 = lr.to64(sd)
    for s, j, B, H in ((0, 1, 1, 5), (2, 8, 1, 5), (3, 2, 1, 9)):
        x = lr.seeded_input(s, B, H, seed=s)
        case = lr.block_case(sd, sd64, s, j, lr.nchw(x))
        ref = ref_cpu.block(sd64, s, j, lr.nchw(x).double()).permute(0, 2, 3, 1)
        assert float((case.ref - ref).abs().max()) < 1e-12
        for prec, form in lr.DEVICE_GELU.items():
            full = lr.block(sd64, s, j, lr.nchw(x).double(), gelu=form)
            assert abs(float((full - ref).abs().max()) - case.G[prec]) < 1e-12
            assert 1e-7 < case.bar(prec) < lr.LAYER_TOL / 3.0, (s, prec, case.bar(prec))
        assert 1e-8 < case.noise32 < 5e-6


def test_stage_tail_and_downsample_cases():
    from oracle import ref_cpu
    sd = synth.synth_state_dict(0)
    sd64 = lr.to64(sd)
    x = lr.seeded_input(1, 1, 10, seed=3)
    case = lr.stage_tail_case(sd, sd64, 1, lr.nchw(x))
    ref = ref_cpu.downsample(sd64, 2, ref_cpu.block(sd64, 1, 2, lr.nchw(x).double())).permute(0, 2, 3, 1)
    assert case.ref.shape == (1, 5, 14, 384) and float((case.ref - ref).abs().max()) < 1e-12
    assert 0.0 < case.G["fp32"] < case.G["fp32_split"] < 5e-6 and case.bar("fp32_split") < lr.LAYER_TOL / 3.0
    d = lr.downsample_case(sd, sd64, 3, lr.nchw(lr.seeded_input(2, 1, 3, seed=4)))
    assert d.ref.shape == (1, 1, 7, 768) and d.G == {} and d.bar("fp32_split") == lr.SPLIT_FACTOR * d.noise32


def test_guards_see_an_overrun_and_unwritten_scratch():
    t = torch.arange(30, dtype=torch.float32).view(2, 3, 5)
    g, v = lr.Guarded.tensor(t, device="cpu")
    assert torch.equal(v, t) and g.intact() and v.data_ptr() - g.buf.data_ptr() == 256
    lr.assert_clean(v, g)
    for off in (-1, t.numel(), lr.GUARD_WORDS + 63):          # the word in front, the first padding word behind, the very last word
        g, v = lr.Guarded.tensor(t, device="cpu")
        g.buf[lr.GUARD_WORDS + off] = 0
        assert not g.intact()
    gs, scr = lr.Guarded.scratch(1000, device="cpu")
    assert scr.numel() == 1000 and bool((scr == 255).all()) and gs.intact()
    assert bool(torch.isnan(scr[:1000].view(torch.float32)).all()) and bool(torch.isnan(scr.view(torch.bfloat16).float()).all())
    go, out = lr.Guarded.filled((3, 4), device="cpu")
    with pytest.raises(AssertionError):
        lr.assert_clean(out, go)                               # an output nobody wrote is NaN


def test_stage_tail_scratch_size():
    """acx_test_stage_tail_scratch_bytes needs no context: the block scratch of the stage plus room for the bf16 images of x and of
    the downsample's output (ACX_PREC_BF16_ACT), in 256-byte pieces; stages 0-2 only."""
    import ctypes
    from audioset_convnext_inf_amd import _ffi
    lib = _ffi.lib()
    for s, B, H in ((0, 1, 10), (1, 3, 6), (2, 2, 37)):
        W, C = 56 >> s, lr.DIMS[s]
        blk, tail = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.acx_block_scratch_bytes(s, B, H, W, ctypes.byref(blk)) == 0
        assert lib.acx_test_stage_tail_scratch_bytes(s, B, H, W, ctypes.byref(tail)) == 0
        extra = tail.value - blk.value
        assert tail.value % 256 == 0 and extra >= B * H * W * C * 2 + B * (H // 2) * (W // 2) * 2 * C * 2
        assert extra < B * H * W * C * 3 + 512
    assert lib.acx_test_stage_tail_scratch_bytes(3, 1, 4, 7, ctypes.byref(tail)) != 0
    assert lib.acx_test_stage_tail_scratch_bytes(0, 1, 4, 56, None) != 0


# ---- would the bars notice?  The arithmetic errors the GPU tests exist for, made on the CPU -------------------------------------
def test_bar_sees_a_lost_split_product():
    """The downsample conv in the documented split arithmetic stays well inside the per-layer bar; with any one of its three
    products left out it is far outside -- a lost lo-half term is about 2^-12 of every product, a hundred times the bar."""
    sd = synth.synth_state_dict(0)
    sd64 = lr.to64(sd)
    for i, (B, H) in ((1, (2, 19)), (2, (3, 7)), (3, (1, 75))):
        x = lr.nchw(lr.seeded_input(i - 1, B, H, seed=i))
        case = lr.downsample_case(sd, sd64, i, x)
        bar = case.bar("fp32_split")
        err = [float((lr.split_downsample(sd64, i, x, drop).double() - case.ref).abs().max()) for drop in (None, 0, 1, 2)]
        print("downsample %d: intact %.3g, a term dropped %.3g / %.3g / %.3g, bar %.3g" % (i, *err, bar))
        assert err[0] < 0.6 * bar
        assert min(err[1:3]) > 20.0 * bar and err[3] > 1e3 * bar


def test_binned_means_see_a_sixth_digit_of_a_gelu_coefficient(monkeypatch):
    """The device GELU check of tests/test_gpu_layer_shapes.py with the restated form standing in for the device: it passes; with
    k0 moved in its sixth digit on the "device" side only (what a kernel built from an edited header computes) its maximum
    still passes and its binned means do not."""
    import test_gpu_layer_shapes as T

    class Stub:
        def __init__(self, sd, precision):
            self.sd = sd

        def native_context(self, device):
            return self
    k = {"k": lr.GELU3_K}

    def device(c, s, j, x):
        return lr.block(c.sd, s, j, lr.nchw(x), gelu=lambda h: _gelu3_with(k["k"], h).float())

    def _gelu3_with(coeff, h):
        with monkeypatch.context() as m:
            m.setattr(lr, "GELU3_K", coeff)
            return lr._gelu3_fp32(h)
    monkeypatch.setattr(T, "_make_model", Stub)
    monkeypatch.setattr(T, "_run_block", device)
    sd = synth.synth_state_dict(0)
    T._check_device_gelu(sd, "fp32_split", 3)
    k["k"] = (lr.GELU3_K[0] - 1e-5,) + lr.GELU3_K[1:]
    with pytest.raises(AssertionError, match="binned"):
        T._check_device_gelu(sd, "fp32_split", 3)
