"""GPU (`-m gpu`): the matrix-pipe depthwise kernel of `bf16a` (dwconv_mfma.hip) against float64 at every step count and edge.

Which paths of dwconv7_mfma_kernel a launch takes -- whether the 16-row ring wraps, after which copy of the step the loop leaves,
how far the scalar cursors walk over clips and zero rows, whether surplus groups repeat the last one, how the workgroups are
renumbered over the XCDs -- follows from `steps` and the segment count, and at the shipped setting every tensor a quick test can
afford gets 2 steps.  tests/dwconv_bf16_cases.py fixes small cases with small `target_waves` (tests/test_dwconv_bf16_plan_cpu.py
asserts what they reach); here each runs through acx_test_dwconv7_bf16_form / acx_test_dwconv7_varlen:

  * every output lies in [bf16(ref - E), bf16(ref + E)] of the float64 conv (dwconv_bf16_cases.py: E bounds the fp32 accumulation
    in any order, the store is monotone; no tolerance on top) -- an equality with the rounded exact sum on 97 % of the elements;
  * every target_waves of a shape gives the same bits, and so does acx_dwconv7_bf16 at the shipped setting, on the batch and on
    every clip alone; a second run gives the same bits;
  * packed batches at each target_waves: inside the intervals, and bit-equal clip by clip to the uniform form;
  * x sits between guard regions of bf16 NaNs (a row taken from outside the tensor and multiplied into a sum shows), y between
    canaries and starts as NaN, x comes back bit-identical;
  * refusals are non-zero and launch nothing."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
import dwconv_bf16_cases as bc
import dwconv_cases as dc
import layer_ref as lr

pytestmark = pytest.mark.gpu

NAN_PAIR = 0x7FC17FC1        # two bf16 NaNs
GUARD_ROWS = 8               # image rows of NaNs on each side of x: the kernel reads whole rows, up to 3 above and below an output row


def _make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


@pytest.fixture(scope="module")
def ctx(synth_sd):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    m = _make_model(synth_sd, "bf16a")
    return m, m.native_context(torch.device("cuda", 0))


def sp():
    return _ffi.stream_ptr(torch.device("cuda", 0))


class NanGuardedInput:
    """x (bf16, rows x W x C) on the device between GUARD_ROWS image rows of bf16 NaNs on each side."""

    def __init__(self, xb):
        row = xb.shape[-2] * xb.shape[-1] // 2               # int32 words of an image row
        self.words, self.pad = xb.numel() // 2, GUARD_ROWS * row
        self.buf = torch.full((2 * self.pad + self.words,), NAN_PAIR, dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 256 == 0 and (self.pad * 4) % 256 == 0
        self.x = self.buf[self.pad:self.pad + self.words].view(torch.bfloat16).view(xb.shape)
        self.x.copy_(xb)
        self.host = xb
        assert bool(self.buf[:self.pad].view(torch.bfloat16).isnan().all())

    def unchanged(self):
        return (bool((self.buf[:self.pad] == NAN_PAIR).all()) and bool((self.buf[self.pad + self.words:] == NAN_PAIR).all())
                and torch.equal(self.x.cpu().view(torch.int16), self.host.view(torch.int16)))


def _nan_output(shape):
    g, y = lr.Guarded.filled(shape, dtype=torch.bfloat16)
    assert bool(y.isnan().all())
    return g, y


def _bits(y):
    return y.detach().cpu().contiguous().view(torch.int16)


def _run(c, s, gx, B, H, tw):
    """tw = None: acx_dwconv7_bf16 at the shipped setting; else acx_test_dwconv7_bf16_form.  -> y (bf16, device)."""
    gy, y = _nan_output((B, H, bc.width(s), bc.DIMS[s]))
    lib = _ffi.lib()
    if tw is None:
        _ffi.check(lib.acx_dwconv7_bf16(c.handle, s, bc.BLOCK, _ffi.ptr(gx.x), _ffi.ptr(y), B, H, bc.width(s), sp()))
    else:
        _ffi.check(lib.acx_test_dwconv7_bf16_form(c.handle, s, bc.BLOCK, _ffi.ptr(gx.x), _ffi.ptr(y), B, H, bc.width(s), tw, sp()))
    torch.cuda.synchronize()
    assert gy.intact(), "canary of y overwritten (target_waves %s)" % tw
    assert gx.unchanged(), "the input or its guard rows were written (target_waves %s)" % tw
    return y


def _where(a, b):
    d = (_bits(a) != _bits(b)).nonzero()
    return "%d elements differ, the first at index %s" % (d.shape[0], tuple(d[0].tolist()))


def _assert_inside(R, y, what):
    out = R.outside(y)
    if bool(out.any()):
        idx = tuple(out.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d outputs outside [bf16(ref - E), bf16(ref + E)], the first at %s: got %r, interval [%r, %r]"
                             % (what, int(out.sum()), out.numel(), idx, float(y.cpu()[idx]), float(R.lo[idx]), float(R.hi[idx])))


# ---- uniform batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,B,H,tws", bc.CASES)
def test_every_step_count_against_float64(ctx, synth_sd, s, B, H, tws):
    _, c = ctx
    x, R = bc.case_reference(synth_sd, s, B, H)
    gx = NanGuardedInput(x)
    first = None
    for tw in tws:
        p = bc.plan(s, B, H, tw)
        y = _run(c, s, gx, B, H, tw)
        print("dwconv bf16 forms s%d (%d,%d) tw=%d: %r: %.3f %% of the outputs are the rounded exact sum"
              % (s, B, H, tw, p, 100 * R.exact_share(y)))
        _assert_inside(R, y, "stage %d (%d, %d) target_waves %d (%r)" % (s, B, H, tw, p))
        again = _run(c, s, gx, B, H, tw)
        assert torch.equal(_bits(again), _bits(y)), "a second run differs: %s" % _where(again, y)
        if first is None:
            first = y
        else:
            assert torch.equal(_bits(y), _bits(first)), "target_waves %d differs from %d: %s" % (tw, tws[0], _where(y, first))
    shipped = _run(c, s, gx, B, H, None)
    assert torch.equal(_bits(shipped), _bits(first)), "acx_dwconv7_bf16 differs from target_waves %d: %s" % (tws[0], _where(shipped, first))
    for b in range(B):
        g1 = NanGuardedInput(x[b:b + 1].contiguous())
        solo = _run(c, s, g1, 1, H, None)
        assert torch.equal(_bits(solo[0]), _bits(first[b])), "clip %d alone differs from its rows of the batch: %s" % (b, _where(solo[0], first[b]))


# ---- packed batches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,lengths,tws", bc.PACKED)
def test_packed_batches_against_float64_and_the_uniform_form(ctx, synth_sd, s, lengths, tws):
    _, c = ctx
    x, hs, R = bc.packed_reference(synth_sd, s, lengths)
    gx = NanGuardedInput(x)
    arr = (ctypes.c_int64 * len(lengths))(*lengths)
    need = ctypes.c_size_t()
    _ffi.check(_ffi.lib().acx_test_dwconv7_varlen_scratch_bytes(arr, len(lengths), ctypes.byref(need)))
    solo, r0 = [], 0
    for h in hs:                                             # the uniform form on every clip alone, as one segment
        g1 = NanGuardedInput(x[r0:r0 + h][None].contiguous())
        solo.append(_run(c, s, g1, 1, h, 12)[0])
        r0 += h
    solo = torch.cat(solo)
    _assert_inside(R, solo, "stage %d clips alone" % s)
    for tw in tws:
        p = bc.plan_varlen(s, list(lengths), tw)
        gy, y = _nan_output(tuple(x.shape))
        gs, scratch = lr.Guarded.scratch(need.value)
        _ffi.check(_ffi.lib().acx_test_dwconv7_varlen(c.handle, s, bc.BLOCK, _ffi.ptr(gx.x), _ffi.ptr(y), arr, len(lengths), tw,
                                                      _ffi.ptr(scratch), need.value, sp()))
        torch.cuda.synchronize()
        assert gy.intact() and gs.intact() and gx.unchanged()
        print("dwconv bf16 packed s%d heights %s tw=%d: %r: %.3f %% of the outputs are the rounded exact sum" % (s, hs, tw, p, 100 * R.exact_share(y)))
        _assert_inside(R, y, "stage %d packed target_waves %d (%r)" % (s, tw, p))
        assert torch.equal(_bits(y), _bits(solo)), "packed batch at target_waves %d differs from the clips run alone: %s" % (tw, _where(y, solo))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_y_untouched(ctx, synth_sd):
    """Wrong width, stage 3, a null pointer, target_waves of 0 or above 9 x CUs, a batch over the guard (its size from the plan, never
    allocated), a context without bf16 activations: non-zero, and nothing was launched -- y is still NaN."""
    _, c = ctx
    lib = _ffi.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s, B, H = 1, 3, 7
    x = torch.zeros(B, H, bc.width(s), bc.DIMS[s], dtype=torch.bfloat16, device="cuda")
    gy, y = _nan_output(tuple(x.shape))
    tall = bc.largest_batch(H) + 1
    assert bc.plan(s, tall, H, 12).too_tall and not bc.plan(s, tall - 1, H, 12).too_tall

    def form(h=c.handle, stage=s, xp=x, yp=y, B=B, H=H, W=bc.width(s), tw=12):
        return lib.acx_test_dwconv7_bf16_form(h, stage, bc.BLOCK, _ffi.ptr(xp) if xp is not None else None,
                                              _ffi.ptr(yp) if yp is not None else None, B, H, W, tw, sp())
    for bad in (dict(W=14), dict(W=56), dict(stage=3, W=7), dict(stage=3), dict(stage=-1), dict(xp=None), dict(yp=None), dict(tw=0),
                dict(tw=-1), dict(tw=9 * cus + 1), dict(B=0), dict(H=0), dict(B=tall)):
        assert form(**bad) != 0, bad
    other = _make_model(synth_sd, "bf16")                    # bf16 operands, fp32 activations: no bf16 tensor to convolve
    assert form(h=other.native_context(torch.device("cuda", 0)).handle) != 0
    # the packed entry takes the same range of target_waves under bf16a
    lengths = (dc.MIN_SAMPLES, dc.samples_for_h0(22))
    rows = sum(dc.stage_height(L, s) for L in lengths)
    assert rows <= B * H
    arr = (ctypes.c_int64 * 2)(*lengths)
    need = ctypes.c_size_t()
    _ffi.check(lib.acx_test_dwconv7_varlen_scratch_bytes(arr, 2, ctypes.byref(need)))
    scratch = torch.zeros(need.value, dtype=torch.uint8, device="cuda")

    def var(tw):
        return lib.acx_test_dwconv7_varlen(c.handle, s, bc.BLOCK, _ffi.ptr(x), _ffi.ptr(y), arr, 2, tw, _ffi.ptr(scratch), need.value, sp())
    assert var(0) != 0 and var(9 * cus + 1) != 0
    torch.cuda.synchronize()
    assert gy.intact() and bool(y.isnan().all())
    assert var(9 * cus) == 0
    torch.cuda.synchronize()
    assert gy.intact() and bool(torch.isfinite(y.float().view(B * H, -1)[:rows]).all())
    y.fill_(float("nan"))
    assert form(tw=9 * cus) == 0 and form() == 0
    torch.cuda.synchronize()
    assert gy.intact() and bool((y.float() == y.float()[0, 0, 0]).all()), "zeros in: the bias out"
