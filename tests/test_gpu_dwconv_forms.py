"""GPU (`-m gpu`): every FORM of the fp32 depthwise 7x7 convolution against float64, at segment and clip edges.

The fp32 depthwise conv is the ring kernel (W = 56 / 28) and the tile kernel (W = 14 / 7) of dwconv.hip, and the column-streaming
kernel of dwconv_col.hip -- which is 28 instantiations (4 widths x S0 = 0 .. 6: the phase of a segment's head and tail in the
seven-row rotation) plus four for packed batches, picked by the launcher from the batch, the clip height, the CU count and the
sub-batches in flight.  tests/dwconv_cases.py fixes cases that reach every one of them with several segments per launch
(tests/test_dwconv_plan_cpu.py asserts what they reach); here each case runs through acx_test_dwconv7_form / _varlen:

  * the column form at the case's target_waves and the ring / tile form stay within the bound;
  * the two are equal bit for bit (the documented contract that lets the launcher pick by launch size), and so are the column
    form at a second target_waves, which moves every segment boundary, and acx_dwconv7 run clip by clip;
  * packed batches: within the bound and bit-equal to the ring / tile form run clip by clip; under bf16a the matrix-pipe kernel
    is bit-equal to acx_dwconv7_bf16 clip by clip (its arithmetic must not depend on the batch);
  * `stats` of both forms against the float64 LayerNorm of the float64 conv.

Reference and bound come from the reference alone (dwconv_cases.py): float64 conv2d of the same fp32 x and the stored fp32 weights
of stages.s.1;  |y - ref| <= g49 (|b| + sum |x||w|),  g49 = 49 u / (1 - 49 u),  u = 2^-24  -- the bias plus 49 sequential fused
multiply-adds -- per element.  x and y sit between canaries, y starts as NaN, x must come back unchanged."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
import dwconv_cases as dc
import layer_ref as lr

pytestmark = pytest.mark.gpu

DIMS = lr.DIMS
RING, COL = 0, 1


def _make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


@pytest.fixture(scope="module", params=["fp32", "fp32_split"])
def model(synth_sd, request):
    """Both fp32 arithmetics: they carry the same depthwise weights and must run the same depthwise kernels."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _make_model(synth_sd, request.param)


@pytest.fixture(scope="module")
def ctx(model):
    return model.native_context(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def ctx16a(synth_sd):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    m = _make_model(synth_sd, "bf16a")
    return m, m.native_context(torch.device("cuda", 0))


def sp():
    return _ffi.stream_ptr(torch.device("cuda", 0))


# ---- one float64 reference per case, shared by the precisions and the forms, never modified -------------------------------------
_cases = {}


def _case(synth_sd, s, B, H):
    key = (s, B, H)
    if key not in _cases:
        x = lr.seeded_input(s, B, H, seed=31000 + 1000 * s + 13 * B + H)
        _cases[key] = (x,) + dc.conv_ref(synth_sd, s, x)
    return _cases[key]


def _run_form(ctx, s, x, form, tw, want_stats=False):
    """acx_test_dwconv7_form on a guarded copy of x -> y (and stats), on the device."""
    B, H, W, C = x.shape
    gx, xd = lr.Guarded.tensor(x)
    gy, y = lr.Guarded.filled(x.shape)
    guards = [gx, gy]
    stats = None
    if want_stats:
        gs, stats = lr.Guarded.filled((B * H * W, 2))
        guards.append(gs)
    _ffi.check(_ffi.lib().acx_test_dwconv7_form(ctx.handle, s, dc.BLOCK, _ffi.ptr(xd), _ffi.ptr(y), _ffi.ptr(stats) if want_stats else None,
                                                B, H, W, form, tw, sp()))
    torch.cuda.synchronize()
    lr.assert_clean(y, *guards)
    assert torch.equal(xd.cpu(), x), "the input is read, never written"
    if want_stats:
        assert bool(torch.isfinite(stats).all())
        return y.clone(), stats.clone()
    return y.clone()


def _run_clip_by_clip(ctx, s, clips, form=None):
    """Every clip as a batch of one: acx_dwconv7 (the launcher's own choice), or the given form -> one (1, h, W, C) result per clip."""
    outs = []
    for x1 in clips:
        _, H, W, _ = x1.shape
        if form is not None:
            outs.append(_run_form(ctx, s, x1.contiguous(), form, 1))
            continue
        gx, xd = lr.Guarded.tensor(x1)
        gy, y = lr.Guarded.filled(x1.shape)
        _ffi.check(_ffi.lib().acx_dwconv7(ctx.handle, s, dc.BLOCK, _ffi.ptr(xd), _ffi.ptr(y), None, 1, H, W, sp()))
        torch.cuda.synchronize()
        lr.assert_clean(y, gx, gy)
        outs.append(y.clone())
    return outs


def _where(a, b):
    d = (a != b).nonzero()
    return "%d elements differ, the first at index %s" % (d.shape[0], tuple(d[0].tolist()))


# ---- uniform batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,B,H,tw,tw2", dc.UNIFORM_CASES)
def test_forms_against_float64(ctx, model, synth_sd, s, B, H, tw, tw2):
    """Column form at the case's target_waves and ring / tile form within the bound; both, the column form at a second
    target_waves and acx_dwconv7 clip by clip equal bit for bit."""
    x, ref, bound = _case(synth_sd, s, B, H)
    p = dc.plan(s, B, H, tw)
    col = _run_form(ctx, s, x, COL, tw)
    ring = _run_form(ctx, s, x, RING, 0)
    r_col, r_ring = dc.worst_ratio(col, ref, bound), dc.worst_ratio(ring, ref, bound)
    print("dwconv forms s%d (%d,%d) [%s] tw=%d: n_out %d S0 %d k7 %d segments %d: column error/bound %.3f, %s error/bound %.3f"
          % (s, B, H, model.precision, tw, p[0], p[1], p[2], p[3], r_col, "ring" if s < 2 else "tile", r_ring))
    assert r_col <= 1.0, ("column form", s, B, H, tw, r_col)
    assert r_ring <= 1.0, ("ring / tile form", s, B, H, r_ring)
    assert torch.equal(col, ring), "column form (S0 = %d) differs from the %s form: %s" % (p[1], "ring" if s < 2 else "tile", _where(col, ring))
    col2 = _run_form(ctx, s, x, COL, tw2)
    assert torch.equal(col2, col), "column form at target_waves %d differs from %d: %s" % (tw2, tw, _where(col2, col))
    solo = torch.cat(_run_clip_by_clip(ctx, s, [x[b:b + 1] for b in range(B)]))
    assert torch.equal(solo, col), "acx_dwconv7 clip by clip differs from the batch: %s" % _where(solo, col)


@pytest.mark.parametrize("s,B,H,tw,tw2", dc.STATS_CASES)
def test_stats_of_both_forms(ctx, model, synth_sd, s, B, H, tw, tw2):
    """(y - mean) rstd from the emitted statistics against the float64 LayerNorm (no affine, eps 1e-6) of the float64 conv, at
    min(1e-4, 8 noise32): the bar of the pool / head tail (noise32: the same statement in torch fp32 against float64)."""
    x, ref, _ = _case(synth_sd, s, B, H)
    C = DIMS[s]
    ln64 = F.layer_norm(ref, (C,), None, None, 1e-6)
    noise32 = float((F.layer_norm(dc.conv_fp32(synth_sd, s, x), (C,), None, None, 1e-6).double() - ln64).abs().max())
    case = lr.Case(ln64, noise32, {})
    outs = []
    for form in (COL, RING):
        y, stats = _run_form(ctx, s, x, form, tw, want_stats=True)
        st64 = stats.cpu().double()                          # (the reconstruction itself in float64: the error is the kernels')
        ln = ((y.cpu().double().view(-1, C) - st64[:, :1]) * st64[:, 1:]).view(B, H, dc.width(s), C)
        case.check("dwconv stats s%d (%d,%d) form %d" % (s, B, H, form), ln, model.precision)
        outs.append((y, stats))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- packed batches ----------------------------------------------------------------------------------------------------------------
_packed = {}


def _packed_case(synth_sd, s, lengths):
    key = (s, lengths)
    if key not in _packed:
        hs = [dc.stage_height(L, s) for L in lengths]
        x, clips = dc.packed_input(s, hs, seed=52000 + 100 * s + len(hs))
        refs = [dc.conv_ref(synth_sd, s, c) for c in clips]
        _packed[key] = (x, clips, torch.cat([r[0][0] for r in refs]), torch.cat([r[1][0] for r in refs]))
    return _packed[key]


def _scratch_for(lengths):
    arr = (ctypes.c_int64 * len(lengths))(*lengths)
    need = ctypes.c_size_t()
    _ffi.check(_ffi.lib().acx_test_dwconv7_varlen_scratch_bytes(arr, len(lengths), ctypes.byref(need)))
    return arr, need.value


def _run_varlen(ctx, s, xd, y, lengths, tw):
    arr, need = _scratch_for(lengths)
    gs, scratch = lr.Guarded.scratch(need)
    _ffi.check(_ffi.lib().acx_test_dwconv7_varlen(ctx.handle, s, dc.BLOCK, _ffi.ptr(xd), _ffi.ptr(y), arr, len(lengths), tw,
                                                  _ffi.ptr(scratch), need, sp()))
    torch.cuda.synchronize()
    assert gs.intact()


@pytest.mark.parametrize("s,lengths,tw", dc.PACKED_CASES)
def test_packed_batch_against_float64(ctx, model, synth_sd, s, lengths, tw):
    """launch_dwconv_col_varlen on clips of mixed heights: within the bound, and bit-equal to the ring / tile form clip by clip."""
    x, clips, ref, bound = _packed_case(synth_sd, s, lengths)
    gx, xd = lr.Guarded.tensor(x)
    gy, y = lr.Guarded.filled(x.shape)
    _run_varlen(ctx, s, xd, y, lengths, tw)
    lr.assert_clean(y, gx, gy)
    assert torch.equal(xd.cpu(), x)
    p = dc.plan_varlen(s, list(lengths), tw)
    r = dc.worst_ratio(y, ref, bound)
    print("dwconv packed s%d heights %s [%s] tw=%d: k7 %d segments %d: error/bound %.3f"
          % (s, [c.shape[1] for c in clips], model.precision, tw, p[2], p[3], r))
    assert r <= 1.0, (s, lengths, tw, r)
    solo = torch.cat([o[0] for o in _run_clip_by_clip(ctx, s, clips, form=RING)])
    assert torch.equal(solo, y), "packed batch differs from the clips run alone: %s" % _where(solo, y)


def _guarded_bf16(t=None, shape=None):
    n = t.numel() if t is not None else int(torch.tensor(shape).prod())
    g = lr.Guarded(n * 2)
    v = g.payload.view(torch.bfloat16)[:n].view(t.shape if t is not None else shape)
    if t is not None:
        v.copy_(t)
    else:
        v.fill_(float("nan"))
    return g, v


@pytest.mark.parametrize("s,lengths,tw", [c for c in dc.PACKED_CASES if c[0] < 3])
def test_packed_batch_bf16a_equals_clip_by_clip(ctx16a, synth_sd, s, lengths, tw):
    """launch_dwconv_mfma_varlen (bf16 activations, stages 0-2) against acx_dwconv7_bf16 on every clip alone, bit for bit."""
    model16, c16 = ctx16a
    x, clips, _, _ = _packed_case(synth_sd, s, lengths)
    xb = x.to(torch.bfloat16)
    gx, xd = _guarded_bf16(xb)
    gy, y = _guarded_bf16(shape=tuple(x.shape))
    _run_varlen(c16, s, xd, y, lengths, tw)
    assert gx.intact() and gy.intact() and bool(torch.isfinite(y.float()).all())
    assert torch.equal(xd.cpu(), xb)
    r0 = 0
    for clip in clips:
        h = clip.shape[1]
        g1, x1 = _guarded_bf16(xb[r0:r0 + h][None].contiguous())
        g2, y1 = _guarded_bf16(shape=(1, h) + tuple(x.shape[1:]))
        _ffi.check(_ffi.lib().acx_dwconv7_bf16(c16.handle, s, dc.BLOCK, _ffi.ptr(x1), _ffi.ptr(y1), 1, h, dc.width(s), sp()))
        torch.cuda.synchronize()
        assert g1.intact() and g2.intact()
        assert torch.equal(y1[0], y[r0:r0 + h]), "clip of %d rows at row %d differs from the packed batch" % (h, r0)
        r0 += h


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_y_untouched(ctx, model):
    """A wrong width for the stage, target_waves = 0 (and beyond 4 x CUs), an unknown form, a null pointer, a short scratch: non-zero,
    and nothing was launched -- y is still NaN."""
    lib = _ffi.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = torch.zeros(2, 7, 28, 192, device="cuda")
    y = torch.full_like(x, float("nan"))

    def form(stage=1, xp=x, yp=y, B=2, H=7, W=28, f=COL, tw=12):
        return lib.acx_test_dwconv7_form(ctx.handle, stage, dc.BLOCK, _ffi.ptr(xp) if xp is not None else None,
                                         _ffi.ptr(yp) if yp is not None else None, None, B, H, W, f, tw, sp())
    for bad in (dict(W=14), dict(W=56), dict(tw=0), dict(tw=4 * cus + 1), dict(tw=-1), dict(f=2), dict(f=-1), dict(xp=None), dict(yp=None),
                dict(stage=4), dict(B=0), dict(H=0), dict(f=RING, W=14)):
        assert form(**bad) != 0, bad
    torch.cuda.synchronize()
    assert bool(y.isnan().all())

    lengths = (dc.MIN_SAMPLES, dc.samples_for_h0(22))
    rows = sum(dc.stage_height(L, 1) for L in lengths)
    xv = torch.zeros(rows, 28, 192, device="cuda")
    yv = torch.full_like(xv, float("nan"))
    arr, need = _scratch_for(lengths)
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")

    def var(stage=1, xp=xv, yp=yv, ln=arr, n=2, tw=12, sc=scratch, nbytes=need):
        return lib.acx_test_dwconv7_varlen(ctx.handle, stage, dc.BLOCK, _ffi.ptr(xp) if xp is not None else None,
                                           _ffi.ptr(yp) if yp is not None else None, ln, n, tw, _ffi.ptr(sc) if sc is not None else None,
                                           nbytes, sp())
    short = (ctypes.c_int64 * 2)(dc.MIN_SAMPLES - 1, dc.MIN_SAMPLES)
    for bad in (dict(nbytes=need - 256), dict(nbytes=0), dict(sc=scratch[4:]), dict(sc=None), dict(tw=0), dict(tw=8 * cus + 1), dict(xp=None),
                dict(yp=None), dict(ln=None), dict(n=0), dict(stage=4), dict(ln=short)):
        assert var(**bad) != 0, bad
    torch.cuda.synchronize()
    assert bool(yv.isnan().all())
    assert var() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(yv).all())
