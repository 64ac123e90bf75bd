"""GPU (`-m gpu`): the block, downsample and stage-tail kernels per TILE FORM against float64, at the shapes where tiles end.

The matrix kernels of the trunk choose their tile form from the launch size and the CU count (mlp_fused_split_kernel: persistent
256-pixel tiles; mlp_fused_wide_kernel: 64- / 128-pixel tiles or the persistent form; gemm_split16_kernel: 64- / 128- / 256-row
tiles, with the 2x2 gather for the downsample convs; the native-fp32 kernels).  tests/test_gpu_parity.py holds them against a
reference at launches of at most a few tiles; here every form meets a per-layer float64 reference at sizes just below, at and
just above its tiles, with more tiles than CUs, in block 1 and in the stage's last block, and through the in-kernel LayerNorm-rows
epilogue that only the forwards reach otherwise (acx_test_stage_tail).  The forms of one case must also agree bit for bit.

The bar of every case is computed on the CPU from the reference alone (tests/layer_ref.py):
    bar = min(LAYER_TOL, 8 * noise32 + 2 * G).
Tensors live between canary words and scratch starts as 0xFF bytes: a store outside a tensor, or scratch read before it is
written, fails the case whatever the values."""
import ctypes
import functools

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
import layer_ref as lr

pytestmark = pytest.mark.gpu

DIMS, DEPTHS = lr.DIMS, lr.DEPTHS
TUNING = ("ACX_WIDE_NPB", "ACX_WIDE_PERSIST", "ACX_GEMM_MI", "ACX_DW_STREAM")

BLOCK_SHAPES = lr.BLOCK_SHAPES
# more tiles than CUs: 73 640 pixels = 287.66 tiles of 256 (stage 0), 36 820 = 287.66 tiles of 128 (stage 1): workgroups of the
# persistent forms walk a second tile and the last tile ends inside a 16-pixel block
BIG_SHAPE = (5, 263)
BIG_TILE = {0: 256, 1: 128}

WIDE_FORMS = [{}, {"ACX_WIDE_NPB": "1"}, {"ACX_WIDE_NPB": "2"}]
PERS_FORMS = [{"ACX_WIDE_NPB": "2", "ACX_WIDE_PERSIST": "1"}, {"ACX_WIDE_NPB": "2", "ACX_WIDE_PERSIST": "0"}]
GEMM_FORMS = [{"ACX_GEMM_MI": "1"}, {"ACX_GEMM_MI": "2"}, {"ACX_GEMM_MI": "4"}]
BLOCK_FORMS = {0: [{}], 1: WIDE_FORMS + PERS_FORMS, 2: WIDE_FORMS, 3: [{}] + GEMM_FORMS}
BIG_FORMS = {0: [{}], 1: [{}] + PERS_FORMS}
DW_FORMS = [{"ACX_DW_STREAM": "0"}, {"ACX_DW_STREAM": "1"}]
DW_SHAPE = {0: (3, 3), 1: (3, 3), 2: (3, 3), 3: (3, 31)}


@pytest.fixture(scope="module", params=["fp32", "fp32_split"])
def model(synth_sd, request):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _make_model(synth_sd, request.param)


@pytest.fixture(scope="module")
def ctx(model):
    return model.native_context(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def sd64(synth_sd):
    return lr.to64(synth_sd)


def _make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


def sp():
    return _ffi.stream_ptr(torch.device("cuda", 0))


def _forms_for(precision, forms):
    # the switches select tile forms of the split kernels; the native-fp32 kernels have one form each
    return forms if precision == "fp32_split" else [{}]


def _run_forms(monkeypatch, forms, run):
    """run() under every form: {env} -> result.  The environment is restored and re-read whatever happens."""
    refresh = _ffi.lib().acx_tuning_refresh
    outs = []
    for var in TUNING:
        monkeypatch.delenv(var, raising=False)
    try:
        for form in forms:
            for var in TUNING:
                monkeypatch.delenv(var, raising=False)
            for var, v in form.items():
                monkeypatch.setenv(var, v)
            refresh()
            outs.append(run())
    finally:
        for var in TUNING:
            monkeypatch.delenv(var, raising=False)
        refresh()
    return outs


def _name(form):
    return ",".join("%s=%s" % (k[4:], v) for k, v in form.items()) or "default"


def _all_forms_agree(forms, outs):
    for form, out in zip(forms[1:], outs[1:]):
        assert torch.equal(out, outs[0]), "form %s differs from form %s in bits" % (_name(form), _name(forms[0]))


# ---- blocks ----------------------------------------------------------------------------------------------------------------------
_block_cases = {}


def _block_case(synth_sd, sd64, s, j, B, H):
    """One float64 reference per (stage, block, shape), shared by the precisions and the forms, never modified."""
    key = (s, j, B, H)
    if key not in _block_cases:
        x = lr.seeded_input(s, B, H, seed=1000 * s + 100 * j + 7 * B + H)
        _block_cases[key] = (x, lr.block_case(synth_sd, sd64, s, j, lr.nchw(x)))
    return _block_cases[key]


def _run_block(ctx, s, j, x):
    B, H, W, _ = x.shape
    need = ctypes.c_size_t()
    _ffi.check(_ffi.lib().acx_block_scratch_bytes(s, B, H, W, ctypes.byref(need)))
    gx, xd = lr.Guarded.tensor(x)
    gs, scratch = lr.Guarded.scratch(need.value)
    _ffi.check(_ffi.lib().acx_block(ctx.handle, s, j, _ffi.ptr(xd), B, H, W, _ffi.ptr(scratch), need.value, sp()))
    torch.cuda.synchronize()
    lr.assert_clean(xd, gx, gs)
    return xd.clone()


def _check_block(ctx, model, synth_sd, sd64, monkeypatch, s, j, B, H, forms):
    x, case = _block_case(synth_sd, sd64, s, j, B, H)
    forms = _forms_for(model.precision, forms)
    outs = _run_forms(monkeypatch, forms, lambda: _run_block(ctx, s, j, x))
    for form, out in zip(forms, outs):
        case.check("block s%d b%d (%d,%d) M=%d %s" % (s, j, B, H, B * H * (56 >> s), _name(form)), out, model.precision)
    _all_forms_agree(forms, outs)


@pytest.mark.parametrize("last", [False, True], ids=["b1", "blast"])
@pytest.mark.parametrize("s,B,H", [(s, B, H) for s in range(4) for B, H in BLOCK_SHAPES[s]])
def test_block_tile_shapes(ctx, model, synth_sd, sd64, monkeypatch, s, B, H, last):
    """acx_block, block 1 and the stage's last block, every tile form of the stage's MLP kernels, against the float64 block."""
    _check_block(ctx, model, synth_sd, sd64, monkeypatch, s, DEPTHS[s] - 1 if last else 1, B, H, BLOCK_FORMS[s])


@pytest.mark.parametrize("last", [False, True], ids=["b1", "blast"])
@pytest.mark.parametrize("s", [0, 1])
def test_block_more_tiles_than_cus(ctx, model, synth_sd, sd64, monkeypatch, s, last):
    """(5, 263): workgroups of the persistent kernels walk a second tile (stage 0 always, stage 1 in its default form at this size);
    stage 1 also in the forced persistent and the forced one-tile-per-workgroup form."""
    B, H = BIG_SHAPE
    M = B * H * (56 >> s)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (M + BIG_TILE[s] - 1) // BIG_TILE[s]
    assert tiles > cus, "the case no longer walks a second tile: %d tiles on %d CUs" % (tiles, cus)
    assert M % 16 != 0 and M % BIG_TILE[s] != 0
    _check_block(ctx, model, synth_sd, sd64, monkeypatch, s, DEPTHS[s] - 1 if last else 1, B, H, BIG_FORMS[s])


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_block_both_depthwise_forms(ctx, model, synth_sd, sd64, monkeypatch, s):
    """The tile and the column-streaming depthwise kernels in front of the same MLP (ACX_DW_STREAM = 0 | 1)."""
    B, H = DW_SHAPE[s]
    x, case = _block_case(synth_sd, sd64, s, 1, B, H)
    outs = _run_forms(monkeypatch, DW_FORMS, lambda: _run_block(ctx, s, 1, x))
    for form, out in zip(DW_FORMS, outs):
        case.check("block s%d b1 (%d,%d) %s" % (s, B, H, _name(form)), out, model.precision)
    _all_forms_agree(DW_FORMS, outs)


# ---- downsamples -----------------------------------------------------------------------------------------------------------------
DOWN_SHAPES = lr.DOWN_SHAPES
_down_cases = {}


def _down_case(synth_sd, sd64, i, B, H):
    key = (i, B, H)
    if key not in _down_cases:
        x = lr.seeded_input(i - 1, B, H, seed=5000 + 100 * i + 7 * B + H)
        _down_cases[key] = (x, lr.downsample_case(synth_sd, sd64, i, lr.nchw(x)))
    return _down_cases[key]


def _run_downsample(ctx, i, x):
    B, H, W, C = x.shape
    gx, xd = lr.Guarded.tensor(x)
    go, out = lr.Guarded.filled((B, H // 2, W // 2, DIMS[i]))
    gs, scratch = lr.Guarded.scratch(x.numel() * 4)
    _ffi.check(_ffi.lib().acx_downsample(ctx.handle, i, _ffi.ptr(xd), _ffi.ptr(out), _ffi.ptr(scratch), B, H, W, sp()))
    torch.cuda.synchronize()
    lr.assert_clean(out, gx, go, gs)
    assert torch.equal(xd.cpu(), x)                        # the input is read, never written
    return out.clone()


@pytest.mark.parametrize("B,H", DOWN_SHAPES)
@pytest.mark.parametrize("i", [1, 2, 3])
def test_downsample_tile_shapes(ctx, model, synth_sd, sd64, monkeypatch, i, B, H):
    """acx_downsample under every row tile of the gather GEMM against ref_cpu.downsample in float64 (no GELU: G = 0)."""
    x, case = _down_case(synth_sd, sd64, i, B, H)
    forms = _forms_for(model.precision, [{}] + GEMM_FORMS)
    outs = _run_forms(monkeypatch, forms, lambda: _run_downsample(ctx, i, x))
    rows = B * (H // 2) * (28 >> (i - 1))
    for form, out in zip(forms, outs):
        case.check("downsample %d (%d,%d) rows=%d %s" % (i, B, H, rows, _name(form)), out, model.precision)
    _all_forms_agree(forms, outs)


# ---- stage tail: the LayerNorm-rows epilogue of a stage's last block and the gather GEMM that reads those rows -------------------
TAIL_SHAPES = {0: [(1, 10), (3, 6), (2, 37)], 1: [(1, 10), (3, 6), (2, 37)], 2: [(1, 10), (3, 6), (2, 37)]}
_tail_cases = {}


def _tail_case(synth_sd, sd64, s, B, H):
    key = (s, B, H)
    if key not in _tail_cases:
        x = lr.seeded_input(s, B, H, seed=9000 + 100 * s + 7 * B + H)
        _tail_cases[key] = (x, lr.stage_tail_case(synth_sd, sd64, s, lr.nchw(x)))
    return _tail_cases[key]


def _run_tail(ctx, s, x):
    B, H, W, _ = x.shape
    need = ctypes.c_size_t()
    _ffi.check(_ffi.lib().acx_test_stage_tail_scratch_bytes(s, B, H, W, ctypes.byref(need)))
    gx, xd = lr.Guarded.tensor(x)
    go, out = lr.Guarded.filled((B, H // 2, W // 2, DIMS[s + 1]))
    gs, scratch = lr.Guarded.scratch(need.value)
    _ffi.check(_ffi.lib().acx_test_stage_tail(ctx.handle, s, _ffi.ptr(xd), _ffi.ptr(out), B, H, W, _ffi.ptr(scratch), need.value, sp()))
    torch.cuda.synchronize()
    lr.assert_clean(out, gx, go, gs)          # (x is not read back: the last block does not update it in the 16-bit arithmetics)
    return out.clone()


@pytest.mark.parametrize("s,B,H", [(s, B, H) for s in range(3) for B, H in TAIL_SHAPES[s]])
def test_stage_tail(ctx, model, synth_sd, sd64, monkeypatch, s, B, H):
    """The calls the forwards make at the end of stages 0-2: the last block with the LayerNorm-rows epilogue, then the downsample
    conv on those rows -- against float64 downsample(block(x)), under the block forms and the GEMM forms."""
    x, case = _tail_case(synth_sd, sd64, s, B, H)
    forms = _forms_for(model.precision, BLOCK_FORMS[s] + GEMM_FORMS)
    outs = _run_forms(monkeypatch, forms, lambda: _run_tail(ctx, s, x))
    for form, out in zip(forms, outs):
        case.check("stage tail %d (%d,%d) %s" % (s, B, H, _name(form)), out, model.precision)
    _all_forms_agree(forms, outs)


def test_stage_tail_refuses_what_it_cannot_run(ctx):
    """Stage 3 has no tail, the width belongs to the stage, a 2x2 conv needs two rows, the scratch has a size and an alignment."""
    lib = _ffi.lib()
    need = ctypes.c_size_t()
    _ffi.check(lib.acx_test_stage_tail_scratch_bytes(1, 1, 4, 28, ctypes.byref(need)))
    x = torch.zeros(1, 4, 28, 192, device="cuda")
    out = torch.zeros(1, 2, 14, 384, device="cuda")
    scratch = torch.zeros(need.value + 256, dtype=torch.uint8, device="cuda")

    def call(stage=1, xp=x, op=out, H=4, W=28, sc=scratch, nbytes=need.value):
        return lib.acx_test_stage_tail(ctx.handle, stage, _ffi.ptr(xp), _ffi.ptr(op), 1, H, W, _ffi.ptr(sc), nbytes, sp())
    assert call() == 0
    for bad in (dict(stage=3), dict(stage=-1), dict(W=14), dict(H=1), dict(xp=None), dict(op=None), dict(nbytes=need.value - 256),
                dict(sc=scratch[4:])):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert not bool(out.isnan().any())


# ---- the device GELU over its whole argument range -------------------------------------------------------------------------------
# 8 064 / 4 032 / 1 512 / 1 008 pixels: 4C arguments per pixel, about three million at every width -- no gap of 1e-3 in [-12, 12],
# and thousands of arguments in every bin of the mean-error check below
GELU_SHAPE = {0: (6, 24), 1: (4, 36), 2: (3, 36), 3: (3, 48)}
FAR = (1e3, -1e3, 1e4, -1e4)


def _gelu_state_dict(synth_sd, s, k0):
    """Blocks 0 and 1 of stage s as a GELU probe: identity depthwise tap, plain LayerNorm, pwconv1 = 4 x one input channel per unit
    plus a bias ramp over [-8, 8] (eight units far out), pwconv2 picks unit 4c + k for channel c (k = k0 in block 0, k0 + 1 in block
    1), gamma = 0.5: out - x = 0.5 gelu(v) at v = 4 LN(x)[u mod C] + bias[u]."""
    C = DIMS[s]
    sd = {k: v.clone() for k, v in synth_sd.items()}
    b1 = torch.linspace(-8.0, 8.0, 4 * C)
    far_units = []
    for n, v in enumerate(FAR):
        for u in (4 * (5 + 11 * n) + n, 4 * (C - 7 - 13 * n) + n):        # units 4c + k with k = n: every k meets one value near both ends
            b1[u] = v
            far_units.append(u)
    for j in (0, 1):
        p = "stages.%d.%d." % (s, j)
        dw = torch.zeros(C, 1, 7, 7)
        dw[:, 0, 3, 3] = 1.0
        sd[p + "dwconv.weight"] = dw
        sd[p + "dwconv.bias"] = torch.zeros(C)
        sd[p + "norm.weight"] = torch.ones(C)
        sd[p + "norm.bias"] = torch.zeros(C)
        w1 = torch.zeros(4 * C, C)
        w1[torch.arange(4 * C), torch.arange(4 * C) % C] = 4.0
        sd[p + "pwconv1.weight"] = w1
        sd[p + "pwconv1.bias"] = b1.clone()
        w2 = torch.zeros(C, 4 * C)
        w2[torch.arange(C), 4 * torch.arange(C) + k0 + j] = 1.0
        sd[p + "pwconv2.weight"] = w2
        sd[p + "pwconv2.bias"] = torch.zeros(C)
        sd[p + "gamma"] = torch.full((C,), 0.5)
    return sd, far_units


@functools.lru_cache(maxsize=None)
def _gelu_input(s):
    B, H = GELU_SHAPE[s]
    return torch.randn(B, H, 56 >> s, DIMS[s], generator=torch.Generator().manual_seed(300 + s))


def _check_far_units(out, x, v, far):
    """Far out gelu(v) = v, and exactly 0 for negative v.  v: the float64 arguments behind the far channels."""
    pos = v.reshape(-1, 2).min(dim=0).values > 0
    assert float(v.abs().min()) > 900.0
    of, xf = out[..., far], x[..., far]
    assert torch.equal(of[..., ~pos], xf[..., ~pos]), "gelu(v) is not exactly 0 far below zero"
    if bool(pos.any()):
        # out = fl(x + 0.5 v): the split products of v (8 x 2^-24 relative, layer_ref.py) and one rounding of the sum
        want = (xf.double() + 0.5 * v)[..., pos]
        assert float(((of.double()[..., pos] - want).abs() / want.abs()).max()) <= 9.0 * 2.0 ** -24


def _check_coverage(allv):
    """The run means something only if the arguments cover [-12, 12] without holes."""
    assert float(allv.min()) < -12.0 and float(allv.max()) > 12.0
    v = torch.sort(allv).values
    v = v[(v >= -12.0) & (v <= 12.0)]
    assert float((v[1:] - v[:-1]).max()) <= 1e-3 and float(v[0]) <= -12.0 + 1e-3 and float(v[-1]) >= 12.0 - 1e-3


def _check_binned_means(name, allv, dev_err, form_err, mag, bar):
    """A maximum cannot tell a SYSTEMATIC error of the form from rounding noise eight times its size; a mean over thousands of
    arguments can.  Per bin of 0.5 in v: the device's mean error must equal the mean error of the restated form (pinned
    coefficients, evaluated at the float64 arguments) within 4 bar / sqrt n -- every sample deviates by less than the case's bar,
    asserted before, so the mean of n independent roundings stays inside four such standard deviations -- plus 2^-24 of the bin's
    mean magnitude for what is not zero-mean (the dropped lo x lo products, the last bit of the hardware exp2)."""
    edges = torch.arange(-12.0, 12.0 + 1e-9, 0.5, dtype=torch.float64)
    idx = torch.bucketize(allv, edges)
    nb = edges.numel() + 1
    n = torch.bincount(idx, minlength=nb).double()
    keep = n >= 2000
    keep[0] = keep[-1] = False
    assert int(keep.sum()) >= 40                                           # [-10, 10] at least
    mean = [torch.bincount(idx, weights=t, minlength=nb) / n.clamp_min(1.0) for t in (dev_err, form_err, mag)]
    gap = (mean[0] - mean[1]).abs()
    tol = 4.0 * bar / n.clamp_min(1.0).sqrt() + 2.0 ** -24 * mean[2]
    ratio = (gap / tol)[keep]
    print("%s: binned mean error vs the restated form: worst %.3g of its bound (gap %.3g) in the bin from v = %.2f"
          % (name, float(ratio.max()), float(gap[keep][ratio.argmax()]), float(edges[keep[1:]][ratio.argmax()])))
    assert float(ratio.max()) <= 1.0, "binned mean error of %s: %.3g of its bound" % (name, float(ratio.max()))


def _check_device_gelu(synth_sd, precision, s):
    C = DIMS[s]
    x = _gelu_input(s)
    xn = lr.nchw(x)
    form = lr.DEVICE_GELU[precision]
    seen, dev_err, form_err, mag = [], [], [], []
    worst = bar = 0.0
    for k0 in (0, 2):
        sd, far_units = _gelu_state_dict(synth_sd, s, k0)
        sd64 = lr.to64(sd)
        c = _make_model(sd, precision).native_context(torch.device("cuda", 0))
        for j in (0, 1):
            k = k0 + j
            h = lr.block_preact(sd64, s, j, xn.double())                   # (B, H, W, 4C) float64 pre-activations
            picked = h[..., 4 * torch.arange(C) + k]                       # the argument behind output channel c
            far = torch.tensor([4 * ch + k in far_units for ch in range(C)])
            assert int(far.sum()) == 2
            v = picked[..., ~far].reshape(-1)
            ref = lr.block_finish(sd64, s, j, xn.double(), lr.gelu_exact(h))
            assert float((ref - (x.double() + 0.5 * lr.gelu_exact(picked))).abs().max()) < 1e-9       # the probe measures what it says
            fe = 0.5 * (form(v) - lr.gelu_exact(v))
            G = float(fe.abs().max())
            assert G <= 0.5 * 1.1e-6                                       # the restated form's own error (tests/test_split_arithmetic_cpu.py)
            noise32 = float((lr.block(sd, s, j, xn).double() - ref)[..., ~far].abs().max())
            case = lr.Case(ref[..., ~far], noise32, {precision: G})
            out = _run_block(c, s, j, x).cpu()
            worst = max(worst, case.check("device GELU s%d k=%d" % (s, k), out[..., ~far], precision))
            bar = max(bar, case.bar(precision))
            _check_far_units(out, x, picked[..., far], far)
            seen.append(v)
            dev_err.append((out.double() - ref)[..., ~far].reshape(-1))
            form_err.append(fe)
            mag.append(ref[..., ~far].abs().reshape(-1))
    allv = torch.cat(seen)
    _check_coverage(allv)
    name = "device GELU stage %d %s" % (s, precision)
    _check_binned_means(name, allv, torch.cat(dev_err), torch.cat(form_err), torch.cat(mag), bar)
    print("%s: %d arguments, worst error / bar %.3f" % (name, allv.numel(), worst))


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_device_gelu_split(synth_sd, s):
    """gelu3 as it ships (split_math.h, hardware exp2 included) in every kernel that owns one: mlp_fused_split_kernel (stage 0),
    mlp_fused_wide_kernel<192 / 384> (stages 1, 2), gemm_split16_kernel's epilogue (stage 3) -- against float64 erf at hundreds of
    thousands of arguments over about [-20, 20]."""
    _check_device_gelu(synth_sd, "fp32_split", s)


@pytest.mark.parametrize("s", [0, 3])
def test_device_gelu_native_fp32(synth_sd, s):
    """gelu_erf (device_common.h) in mlp_fused_kernel (stage 0) and in gemm_f32_kernel's epilogue (stage 3)."""
    _check_device_gelu(synth_sd, "fp32", s)
