"""GPU (`-m gpu`): the bf16 block kernels ("bf16", "bf16a") per form, tile walk and GELU, against their emulation.

What tests/test_gpu_layer_shapes.py does for the fp32 arithmetics, for mlp_fused_wide_bf16.hip (mlp_fused_stat_bf16_kernel at
C = 96, mlp_fused_wide_bf16_kernel<192 | 384, PT>) and gemm_bf16.hip (stage 3):
  a. the persistent walk of the stage-0 kernel: more 32-pixel tiles than 8 x CUs, so that waves prefetch and compute a second
     tile, the last one of 8 rows -- block 1, and the LayerNorm-rows epilogue through acx_test_stage_tail;
  b. C = 192 at 256 + 24 and 8 x 256 + 24 pixels: a partial last workgroup of the two-pixel-tile form ("bf16a", block) and of the
     one-tile forms (the tail, and everything under "bf16");
  c. the stage-3 block under both row tiles of gemm_bf16_kernel (ACX_GEMM_MI = 2 | 4), which must agree bit for bit;
  d. the device GELUs -- gelu2h_micro in the fused kernels, gelu3_unit in the GEMM epilogue -- over their argument range against
     float64 erf, per element and in binned means.
References and bars: tests/bf16_ref.py; every bar is computed on the CPU from the emulation alone.  Tensors live
between canary words and scratch starts as 0xFF bytes (layer_ref.Guarded)."""
import functools

import pytest
import torch

import bf16_ref as br
import layer_ref as lr
import test_gpu_layer_shapes as L

pytestmark = pytest.mark.gpu

DIMS = lr.DIMS
WALK_SHAPE = (5, 263)                   # stage 0: 73 640 pixels = 2 302 tiles of 32, the last one of 8 rows
C192_SHAPES = [(1, 10), (2, 37)]        # stage 1: 280 = 256 + 24 and 2 072 = 8 x 256 + 24 pixels
MI_FORMS = [{"ACX_GEMM_MI": "2"}, {"ACX_GEMM_MI": "4"}]


@pytest.fixture(scope="module", params=["bf16", "bf16a"])
def model16(synth_sd, request):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _make_model(synth_sd, request.param)


@pytest.fixture(scope="module")
def ctx16(model16):
    return model16.native_context(torch.device("cuda", 0))


def _make_model(sd, precision):
    return L._make_model(sd, precision)


def _run_block(ctx, s, j, x):
    return L._run_block(ctx, s, j, x)


# ---- one emulation pair per case, shared by the tests that need it, never modified -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _input(s, B, H, tag):
    return lr.seeded_input(s, B, H, seed={"block": 1700, "tail": 1900}[tag] + 100 * s + 7 * B + H)


_pairs = {}


def _pair(synth_sd, precision, tag, s, B, H):
    # "bf16" and "bf16a" share the arithmetic where no activation is stored as bf16 (stage 3)
    key = (tag, s, B, H, precision if s < 3 else "bf16")
    if key not in _pairs:
        x = _input(s, B, H, tag)
        _pairs[key] = br.block_pair(precision, synth_sd, s, 1, x) if tag == "block" else br.tail_pair(precision, synth_sd, s, x)
    return _pairs[key]


def _check_block(ctx16, model16, synth_sd, s, B, H, name):
    prec = model16.precision
    emu64, emu32 = _pair(synth_sd, prec, "block", s, B, H)
    out = _run_block(ctx16, s, 1, _input(s, B, H, "block"))
    br.check_emulation("%s block s%d b1 (%d,%d) %s" % (name, s, B, H, prec), out, emu64, emu32, br.act_bf16(prec, s))
    return out


def _check_tail(ctx16, model16, synth_sd, s, B, H, name):
    prec = model16.precision
    emu64, emu32 = _pair(synth_sd, prec, "tail", s, B, H)
    out = L._run_tail(ctx16, s, _input(s, B, H, "tail"))
    stored = br.act_bf16(prec, s + 1)
    br.check_emulation("%s tail s%d (%d,%d) %s" % (name, s, B, H, prec), out, emu64, emu32, stored, layers=2)
    if stored:
        assert torch.equal(out, out.to(torch.bfloat16).float())            # what came back are bf16 values


# ---- a. the persistent walk of the stage-0 kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["b1", "tail"])
def test_stage0_persistent_walk(ctx16, model16, synth_sd, what):
    """mlp_fused_stat_bf16_kernel: one workgroup per CU, 8 waves, each walking 32-pixel tiles with stride 8 x workgroups and
    requesting the y rows of its next tile while the current one computes.  (5, 263): every wave's second tile exists or not
    depending on the wave, the last tile has 8 rows (clamped row loads, masked stores) and lies in a second round."""
    B, H = WALK_SHAPE
    M = B * H * 56
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (M + 31) // 32
    assert tiles > 8 * cus, "the case no longer walks a second tile: %d tiles on %d CUs of 8 waves" % (tiles, cus)
    assert M % 32 == 8
    if what == "b1":
        _check_block(ctx16, model16, synth_sd, 0, B, H, "walk")
    else:
        _check_tail(ctx16, model16, synth_sd, 0, B, H, "walk")             # the LNOUT epilogue in a second tile


# ---- b. C = 192: a partial last workgroup of both pixel-tile forms -------------------------------------------------------------------
@pytest.mark.parametrize("what", ["b1", "tail"])
@pytest.mark.parametrize("B,H", C192_SHAPES)
def test_c192_partial_last_workgroup(ctx16, model16, synth_sd, B, H, what):
    """"bf16a": the block takes WideBfCfg<192, 2> (256 pixels per workgroup), the tail <192, 1> with the LayerNorm-rows epilogue;
    "bf16": <192, 1> (128 pixels) in both."""
    assert (B * H * 28) % 256 == 24
    if what == "b1":
        _check_block(ctx16, model16, synth_sd, 1, B, H, "C=192")
    else:
        _check_tail(ctx16, model16, synth_sd, 1, B, H, "C=192")


# ---- c. stage 3 under both row tiles of gemm_bf16_kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", lr.BLOCK_SHAPES[3])
def test_stage3_block_both_gemm_tiles(ctx16, model16, synth_sd, monkeypatch, B, H):
    """run_mlp_bf16: two gemm_bf16_kernel launches (GELU epilogue, residual epilogue) under the 128- and the 256-row tile: each
    against the emulation, and the same bits from both (an output element sees the same MFMAs in the same order)."""
    prec = model16.precision
    emu64, emu32 = _pair(synth_sd, prec, "block", 3, B, H)
    x = _input(3, B, H, "block")
    outs = L._run_forms(monkeypatch, MI_FORMS, lambda: _run_block(ctx16, 3, 1, x))
    for form, out in zip(MI_FORMS, outs):
        br.check_emulation("block s3 b1 (%d,%d) %s %s" % (B, H, L._name(form), prec), out, emu64, emu32, False)
    L._all_forms_agree(MI_FORMS, outs)


# ---- d. the device GELU of the bf16 arithmetics ---------------------------------------------------------------------------------------
def _probe_input(precision, s):
    """The probe's x.  Where the block's result is stored as bf16 the input is scaled to about 2^-4 -- the store's step then is small
    beside gelu, and the LayerNorm still sees a variance far above its 1e-6 -- and is itself a bf16 tensor (what the block reads)."""
    x = L._gelu_input(s)
    if br.act_bf16(precision, s):
        x = (x * 2.0 ** -4).to(torch.bfloat16).float()
    return x


def _probe_arguments(x, s, k, b1):
    """-> (v, excluded), float64 / bool per output element: output channel c of the probe shows unit u = 4 c + k, whose argument is
    v = 4 bf16(LN(x)[u mod C]) + b1[u] -- exact products of bf16 values and one sum, known here to the device's one fp32 rounding
    except where LN(x) sits at a bf16 rounding boundary."""
    C = DIMS[s]
    u = 4 * torch.arange(C) + k
    ln = br.ln_plain(x.double(), C)[..., u % C]
    return 4.0 * br.bf(ln) + b1[u].double(), br.near_bf16_boundary(ln)


def _probe_bound(v, ref, G, stored):
    """|got - x - 0.5 gelu(v)| <= 0.5 (G + 2^-24 |v| + half a bf16 step of the hidden value) + 2^-24 |ref| (+ half a bf16 step of the
    result where it is stored as bf16): the restated form's error over the case's own arguments; the one ulp the hardware exp2 may
    differ from the restatement's correctly rounded one (g = z + |z| (1 - E), E <= 1, |z| = 0.5 |v|); the rounding of the hidden
    value; one fp32 rounding of the sum; the rounding of the store.  The steps are those of the binade the unrounded value can
    lie in."""
    G = G + 2.0 ** -24 * v.abs()
    b = 0.5 * (G + 0.5 * br.bf16_ulp(lr.gelu_exact(v).abs() + G)) + 2.0 ** -24 * ref.abs()
    return b + 0.5 * br.bf16_ulp(ref.abs() + b) if stored else b


def _probe_restated(x, v, form, stored):
    """The whole chain restated: fl32(x + 0.5 bf16(form(fl32(v)))), rounded to bf16 where the result is stored so.  The hidden values
    of one unit repeat with bf16(LN), so their roundings are not independent draws: the binned means compare the device with THIS,
    roundings included, and what is left between the two is the last bit of the hardware exp2."""
    r = (x.double() + 0.5 * br.bf(form(v).float())).float()
    return (r.to(torch.bfloat16) if stored else r).double()


def _probe_check_far(out, x, v, excl, stored):
    """Far out (|v| about 1e3, 1e4) the form returns v itself, or exactly 0: out = x below zero, x + 0.5 bf16(fl32(v)) within one
    fp32 rounding (and half a step of the store) above."""
    assert float(v.abs().min()) > 900.0
    pos = v.reshape(-1, v.shape[-1]).min(dim=0).values > 0
    assert int(pos.sum()) + int((v.reshape(-1, v.shape[-1]).max(dim=0).values < 0).sum()) == v.shape[-1]
    assert torch.equal(out[..., ~pos], x[..., ~pos]), "gelu(v) is not exactly 0 far below zero"
    if bool(pos.any()):
        want = (x.double() + 0.5 * br.bf(v.float()))[..., pos]
        tol = 2.0 ** -24 * want.abs()
        tol = tol + 0.5 * br.bf16_ulp(want.abs() + tol) if stored else tol
        ok = ((out.double()[..., pos] - want).abs() <= tol) | excl[..., pos]
        assert bool(ok.all()), "gelu(v) is not v far above zero"


def _check_coverage(allv):
    """The run means something only if the arguments cover [-12, 12] without holes.  What this arithmetic leaves: v = 4 bf16(LN) +
    b1[u] is the bias ramp over [-8, 8] plus a bf16 grid that is fine near zero and coarsens with |LN| -- no gap of 1e-3 inside the
    ramp, none of 2^-7 (the grid of 4 LN at 0.5 <= |LN| < 1) up to +-12; the forms do not change on that scale (|gelu'| <= 1.13)."""
    assert float(allv.min()) < -12.0 and float(allv.max()) > 12.0
    v = torch.sort(allv).values
    for r, gap in ((8.0, 1e-3), (12.0, 2.0 ** -7)):
        w = v[(v >= -r) & (v <= r)]
        assert float((w[1:] - w[:-1]).max()) <= gap and float(w[0]) <= -r + gap and float(w[-1]) >= r - gap, (r, gap)


def _bin_max(allv, t):
    """max of t per bin of L._check_binned_means."""
    edges = torch.arange(-12.0, 12.0 + 1e-9, 0.5, dtype=torch.float64)
    return torch.zeros(edges.numel() + 1, dtype=torch.float64).scatter_reduce_(0, torch.bucketize(allv, edges), t, "amax")


def _probe_cases(synth_sd, precision, s):
    """The CPU side of the probe, one entry per (k0, j): weights, input, arguments, exclusions."""
    x = _probe_input(precision, s)
    for k0 in (0, 2):
        sd, far_units = L._gelu_state_dict(synth_sd, s, k0)
        for j in (0, 1):
            k = k0 + j
            v, excl = _probe_arguments(x, s, k, sd["stages.%d.%d.pwconv1.bias" % (s, j)])
            far = torch.tensor([4 * ch + k in far_units for ch in range(DIMS[s])])
            assert int(far.sum()) == 2
            yield sd, j, k, x, v, excl, far


def _check_device_gelu(synth_sd, precision, s, per_element=True):
    """per_element=False: only the binned means and the far units are asserted (tests/test_bf16_ref_cpu.py shows that each of the
    two notices a wrong coefficient on its own)."""
    form = br.device_gelu(precision, s)
    stored = br.act_bf16(precision, s)
    seen, dev_err, form_err, mag, bound = [], [], [], [], []
    worst, excluded, total, ctx = 0.0, 0, 0, None
    for sd, j, k, x, v, excl, far in _probe_cases(synth_sd, precision, s):
        if j == 0:
            ctx = _make_model(sd, precision).native_context(torch.device("cuda", 0))
        keep = ~excl[..., ~far]
        vk = v[..., ~far]
        ref = x.double()[..., ~far] + 0.5 * lr.gelu_exact(vk)
        fe = form(vk[keep]) - lr.gelu_exact(vk[keep])
        G = float(fe.abs().max())
        bnd = _probe_bound(vk, ref, G, stored)
        out = _run_block(ctx, s, j, x).cpu()
        err = (out.double()[..., ~far] - ref)
        ratio = float((err.abs() / bnd)[keep].max())
        print("device GELU s%d k=%d %s: G %.3g, worst error / bound %.3f, %d of %d elements left out"
              % (s, k, precision, G, ratio, int((~keep).sum()), keep.numel()))
        assert ratio <= 1.0 or not per_element, ("device GELU per element", s, k, precision, ratio)
        worst = max(worst, ratio)
        _probe_check_far(out[..., far], x[..., far], v[..., far], excl[..., far], stored)
        excluded, total = excluded + int((~keep).sum()), total + keep.numel()
        seen.append(vk[keep])
        dev_err.append(err[keep])
        form_err.append((_probe_restated(x[..., ~far], vk, form, stored) - ref)[keep])
        mag.append(ref[keep].abs())
        bound.append(bnd[keep])
    assert excluded <= br.EXCLUDED_CAP * total, "%d of %d elements at a bf16 rounding boundary of LN(x)" % (excluded, total)
    allv = torch.cat(seen)
    _check_coverage(allv)
    name = "device GELU stage %d %s" % (s, precision)
    L._check_binned_means(name, allv, torch.cat(dev_err), torch.cat(form_err), torch.cat(mag), _bin_max(allv, torch.cat(bound)))
    print("%s: %d arguments, worst error / bound %.3f, %.3f %% left out" % (name, allv.numel(), worst, 100.0 * excluded / total))


@pytest.mark.parametrize("precision", ["bf16", "bf16a"])
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_device_gelu_bf16(synth_sd, s, precision):
    """gelu2h_micro as it ships (split_math.h: gelu_k2h, 0.5 W1 packed, 0.5 b1 staged, hardware exp2) in
    mlp_fused_stat_bf16_kernel (stage 0), mlp_fused_wide_bf16_kernel<192, 1 | 2> (stage 1: "bf16" | "bf16a", the interleaved
    schedule of two pixel tiles) and <384, 1> (stage 2), and gelu3_unit in gemm_bf16_kernel's epilogue (stage 3) -- against float64
    erf at about three million arguments over [-20, 20]."""
    _check_device_gelu(synth_sd, precision, s)
