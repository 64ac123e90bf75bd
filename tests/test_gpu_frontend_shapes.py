"""GPU (`-m gpu`): the two ends of the forward, kernel by kernel, against float64 at the shapes where they can go wrong.

logmel_kernel (the FFT frontend) and frames_kernel -> GEMM -> spec_to_logmel_kernel (the dense frontend), through acx_logmel_bn0:
clips of 513 samples upwards, the lengths at which a third frame and the first interior frames appear, odd lengths at B > 1 (the
8-byte loads of interior frames then start on 4-byte boundaries), fewer frames than waves, more frames than one grid sweep, one
long clip; every filter loop of logmel_kernel (unrolled, general over the LDS, general over global memory), a band that ends at
the Nyquist bin, a band of length 0, a window whose sample 0 is not 0.  pool_head_kernel through acx_pool_head at H3 = 1 .. 31,
where its four time phases run empty or unevenly, with each output pointer null in turn.

The bar of every case is computed on the CPU from the reference alone (tests/frontend_ref.py): an interval in dB
around float64, K = 4 x what fp32 references reach on the case, and for the tail layer_ref.Case = min(1e-4, 8 x noise32).
tests/test_frontend_ref_cpu.py holds the bar: it asserts K <= 64 and that no case has a cell with mel64 <= 2 b, and shows that
six mistakes fail by ten bars or more.  Tensors live between canary words, outputs start as NaN, inputs must come back unchanged,
and a second call must give the same bits."""
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
import frontend_ref as fr
import layer_ref as lr

pytestmark = pytest.mark.gpu

FRONTENDS = ["auto", "dense"]
_contexts = {}


def sp():
    return _ffi.stream_ptr(torch.device("cuda", 0))


def context(which, frontend):
    """The context of a bank / window variant on a frontend (one per pair and module); the frontend the stored buffers get is
    asserted: all variants are window x DFT, so "auto" is the FFT kernel."""
    key = (which, frontend)
    if key not in _contexts:
        assert torch.cuda.is_available(), "gpu tests need a GPU"
        c = _ffi.Context(0)
        c.set_precision("fp32")                             # (the frontend and the tail are fp32 in every mode)
        c.set_frontend(frontend)
        c.load_state_dict(fr.variant(which))
        _contexts[key] = c
    c = _contexts[key]
    info = c.frontend_info()
    assert info["dense_dft"] is (frontend == "dense"), info
    return c, info


def logmel(ctx, wav, bn):
    """acx_logmel_bn0 between canaries, into a NaN-filled output; the input must come back unchanged."""
    B, L = wav.shape
    gw, wd = lr.Guarded.tensor(wav)
    go, out = lr.Guarded.filled((B, L // fr.HOP + 1, fr.MELS))
    _ffi.check(_ffi.lib().acx_logmel_bn0(ctx.handle, _ffi.ptr(wd), B, L, _ffi.ptr(out), 1 if bn else 0, sp()))
    torch.cuda.synchronize()
    lr.assert_clean(out, gw, go)
    assert torch.equal(wd.cpu(), wav), "the waveform was modified"
    return out.clone()


def run_case(which, shape, frontend, bn=False):
    """One case on one frontend: the interval, and the same bits from a second call.  -> context info, output (on the CPU)."""
    case = fr.case(which, shape)
    ctx, info = context(which, frontend)
    out = logmel(ctx, case.wav, bn)
    case.check(case.name, out, frontend, bn)
    assert torch.equal(logmel(ctx, case.wav, bn), out), "a second call gave other bits"
    return info, out.cpu()


# ---- acx_logmel_bn0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,frontend", [(s, f) for s in fr.SHAPES for f in FRONTENDS if f == "auto" or s not in fr.FFT_ONLY],
                         ids=lambda v: fr.shape_id(v))
def test_logmel_edge_shapes(shape, frontend):
    """(1, 513): the API's minimum, T = 2, every tap of both frames reflected, fewer frames than waves.  (3, 639 .. 641): T goes
    2 -> 3, odd L puts clips 1 and 2 on odd offsets, 9 frames leave a wave idle.  (3, 1151 .. 1153): the first interior frame
    (t = 2, p0 + 512 <= L) appears at exactly 1 152; at 1 153 its 8-byte loads are 4-byte aligned.  (2, 1472): interior frame
    t = 3 at exactly its length.  (5, 7360): ACX_MIN_SAMPLES, interior, head and tail frames in every clip.  (1370, 1601): 8 220
    frames -- the FFT kernel's second sweep with 2 076 valid frames and every other wave invalid, three strides of frames_kernel,
    a second loop of spec_to_logmel_kernel over a 28-frame tail.  (1, 1984001): 6 201 frames of one clip, a wave's second frame
    far from its first (FFT frontend only: the dense scratch is not worth the time)."""
    run_case("shipped", shape, frontend)


@pytest.mark.parametrize("bn", [False, True], ids=["dB", "bn0"])
@pytest.mark.parametrize("frontend", FRONTENDS)
def test_logmel_tones_over_noise(frontend, bn):
    """(2, 4000): a 1 kHz tone and a tone halfway between two bins, each over noise at -40 dB -- strong and weak bins in one
    frame, every cell still above twice its bar; in dB and through the bn0 affine."""
    run_case("shipped", fr.SIGNAL, frontend, bn)


@pytest.mark.parametrize("frontend", FRONTENDS)
@pytest.mark.parametrize("shape", fr.BANK_SHAPES, ids=fr.shape_id)
@pytest.mark.parametrize("bank", fr.BANKS)
def test_logmel_mel_banks(bank, shape, frontend):
    """The shipped bank (unrolled loop); one band of lane group 0 widened to 2 taps (the general loop over the LDS table, which
    nothing else runs); mel 223 as a triangle over bins 500 .. 512 (start + 14 > 513: the unrolled form must be refused, it would
    read past the 513 power bins); one column all zero (length 0: the clamp value in every cell, and bn0 of it); a dense melW
    (513 x 224 taps, the loop over global memory).  The dense frontend has one loop for all of them."""
    info, out = run_case(bank, shape, frontend)
    loop, taps = fr.mel_loop(fr.case(bank, shape).sd[fr.KM])
    assert loop == fr.BANK_LOOP[bank] and info["mel_taps"] == taps
    assert (taps <= fr.MEL_LDS) == (loop != "global")
    if bank == "zero_col":
        case = fr.case(bank, shape)
        col = out[:, :, fr.ZERO_COL]
        assert bool((col == col[0, 0]).all()) and abs(float(col[0, 0]) + 100.0) <= case.d, "a band of length 0 is the clamp value"
        _, outbn = run_case(bank, shape, frontend, bn=True)
        s, t = fr.bn_affine64(case.sd)
        want = (col[0, 0].double() * s.float().double()[fr.ZERO_COL] + t.float().double()[fr.ZERO_COL]).float()   # the fma
        assert bool((outbn[:, :, fr.ZERO_COL] == want).all()), "bn0 of the clamp value"


@pytest.mark.parametrize("frontend", FRONTENDS)
def test_logmel_hamming_window(frontend):
    """Stored buffers of another window (hamming: sample 0 is 0.08, not 0) at (3, 1153): still window x DFT, the FFT kernel with
    the window read from the buffers; the reference applies the stored weights."""
    info, _ = run_case("hamming", (3, 1153), frontend)
    assert info["stft_deviation"] <= 2e-6


@pytest.mark.parametrize("shape", [(1, 513), (3, 641)], ids=fr.shape_id)
def test_frontends_pick_the_same_samples(shape):
    """Where the edge is pure indexing -- every tap reflected, clips on odd offsets -- frames_kernel and the FFT kernel's reflect
    path must read the same samples: each output inside its own interval, and the two within the sum of the two bars."""
    case = fr.case("shipped", shape)
    out = {}
    for f in FRONTENDS:
        out[f] = logmel(context("shipped", f)[0], case.wav, False).cpu().double()
        case.check(case.name, out[f], f)
    (lo_a, hi_a), (lo_d, hi_d) = case.interval("auto"), case.interval("dense")
    diff = out["auto"] - out["dense"]
    print("%s: max |auto - dense| = %.3g dB, sum of the bars >= %.3g dB" % (case.name, float(diff.abs().max()), float((hi_a - lo_d).min())))
    assert bool((diff <= hi_a - lo_d).all()) and bool((-diff <= hi_d - lo_a).all())


@pytest.mark.parametrize("frontend", FRONTENDS)
def test_logmel_refusals_leave_the_output_alone(frontend):
    """L = 512 (one sample short of the reflect padding), B = 0, null pointers: a non-zero return code, and the NaN-filled output
    is untouched."""
    ctx, _ = context("shipped", frontend)
    lib = _ffi.lib()
    wav = fr.edge_wav(2, 640, seed=3)
    gw, wd = lr.Guarded.tensor(wav)
    go, out = lr.Guarded.filled((2, 3, fr.MELS))
    calls = {"L = 512": (wd, 2, 512, out), "B = 0": (wd, 0, 640, out), "B < 0": (wd, -1, 640, out), "wav null": (None, 2, 640, out),
             "out null": (wd, 2, 640, None)}
    for name, (w, B, L, o) in calls.items():
        for bn in (0, 1):
            assert lib.acx_logmel_bn0(ctx.handle, _ffi.ptr(w), B, L, _ffi.ptr(o), bn, sp()) != 0, name
    assert lib.acx_logmel_bn0(None, _ffi.ptr(wd), 2, 640, _ffi.ptr(out), 0, sp()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and gw.intact() and go.intact() and torch.equal(wd.cpu(), wav)
    _ffi.check(lib.acx_logmel_bn0(ctx.handle, _ffi.ptr(wd), 2, 640, _ffi.ptr(out), 0, sp()))      # the same buffers are fine
    torch.cuda.synchronize()
    lr.assert_clean(out, gw, go)


# ---- acx_pool_head ----------------------------------------------------------------------------------------------------------------
def pool_head(ctx, x, want=("scene", "logits", "probs")):
    """acx_pool_head between canaries; outputs not in `want` are passed as null and their buffers must stay NaN."""
    B, H3 = x.shape[:2]
    N = ctx.num_classes()
    gx, xd = lr.Guarded.tensor(x)
    bufs = {k: lr.Guarded.filled((B, 768 if k == "scene" else N)) for k in ("scene", "logits", "probs")}
    ptrs = [_ffi.ptr(bufs[k][1]) if k in want else None for k in ("scene", "logits", "probs")]
    _ffi.check(_ffi.lib().acx_pool_head(ctx.handle, _ffi.ptr(xd), B, H3, *ptrs, sp()))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x), "the input was modified"
    for k, (g, v) in bufs.items():
        assert g.intact() and gx.intact(), "canary overwritten"
        if k in want:
            assert bool(torch.isfinite(v).all()), "NaN / inf in " + k
        else:
            assert bool(torch.isnan(v).all()), k + " was written though its pointer was null"
    return {k: bufs[k][1].clone() for k in want}


@pytest.mark.parametrize("B,H3", fr.POOL_SHAPES)
def test_pool_head_time_phases(B, H3):
    """H3 = 1, 2, 3 leave time phases of pool_head_kernel empty (they hold -inf and 0), 5 and 7 fill them unevenly, 31 is the
    10 s clip; B = 70 is more clips than workgroups that run at once on an XCD's share of one wave.  Seeded randn with one row
    raised by 4.0 in half of the channels, in the last phase that holds a row: the maximum comes from there.  Against mean over
    the 7 columns, max + mean over time, LayerNorm(768, 1e-6), Linear, sigmoid in float64 at min(1e-4, 8 x noise32), scene, logits
    and probs each; with each pointer null in turn the others receive the same bits."""
    ctx, _ = context("shipped", "auto")
    x, cases = fr.pool_case(B, H3)
    full = pool_head(ctx, x)
    for k in ("scene", "logits", "probs"):
        cases[k].check("pool_head (%d, %d) %s" % (B, H3, k), full[k], "fp32")
    again = pool_head(ctx, x)
    for drop in ("scene", "logits", "probs"):
        part = pool_head(ctx, x, want=tuple(k for k in ("scene", "logits", "probs") if k != drop))
        for k, v in part.items():
            assert torch.equal(v, full[k]) and torch.equal(again[k], full[k]), "%s differs with %s null" % (k, drop)
    only = pool_head(ctx, x, want=("scene",))                # (the kernel returns before the head)
    assert torch.equal(only["scene"], full["scene"])
