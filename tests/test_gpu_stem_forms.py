"""GPU (`-m gpu`): every FORM of the stem kernel against float64, at its row-pair edges.

stem_kernel<OBF, VAR> (csrc/stem.hip) has four instantiations -- fp32 or bf16 output, uniform or packed batch -- and a persistent
walk: a workgroup takes row pairs g, g + G, g + 2 G, ... with the next pair's rows prefetched into a register ping-pong.
acx_test_stem runs each form on its own and can cap the grid G.  tests/stem_cases.py fixes the cases, references and bars;
tests/test_stem_cases_cpu.py shows from the references alone what the cases rest on.  Here:

  a. the fp32 form within  min(LAYER_TOL, 8 noise32)  of float64 (about 6e-6, not 1e-4) at every shape, the same bits under fp32 and
     fp32_split, and on two probes: one whose variance a one-pass form loses, one where eps decides the result;
  b. the bf16 store: the bits of the fp32 form's output rounded to nearest even, element by element, and within the bar plus half
     a bf16 step of float64;
  c. the packed forms: every clip bit-equal to the uniform form run on that clip alone, and within the bar of float64;
  d. the walk: a capped grid (14, 7 + 7, 5 + 5 + 4 pairs per workgroup) bit-equal to the uncapped launch, and a batch of 4175 row
     pairs at the shipped grid, where workgroups consume a staging register that was refilled inside the loop;
  e. the refusals of the test entry.

Input and output sit between canary words, the output starts as NaN, the input must come back bit-identical."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
import layer_ref as lr
import stem_cases as sc

pytestmark = pytest.mark.gpu

F32_PRECISIONS = ("fp32", "fp32_split")     # one stem arithmetic: both must give the same bits
_models = {}


def _ctx(synth_sd, precision, kind="randn3"):
    """The native context of a model with the case kind's state dict at `precision`, built once per module run."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    key = (precision, kind if kind in ("eps", "offset") else "randn3")
    if key not in _models:
        sd = {"eps": sc.eps_state_dict, "offset": sc.offset_state_dict}.get(kind, lambda d: d)(synth_sd)
        m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
        m.load_state_dict(sd)
        m = m.to("cuda").eval().set_precision(precision)
        _models[key] = (m, m.native_context(torch.device("cuda", 0)))
    return _models[key][1]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _models.clear()


def sp():
    return _ffi.stream_ptr(torch.device("cuda", 0))


def _dtype(precision):
    return torch.bfloat16 if precision == "bf16a" else torch.float32


def _run(ctx, precision, x, B=0, T=0, lengths=None, max_blocks=0):
    """acx_test_stem on a guarded copy of x (host or device tensor) -> the guarded output (rows, 56, 96), still on the device, in the
    type the precision stores.  Canaries, NaN and the input's bits are checked."""
    if lengths is None:
        rows, arr, n, need, gs, scratch = B * sc.h0(T), None, 0, 0, None, None
        assert x.shape == (B, T, sc.MELS)
    else:
        arr, need, rows = sc.scratch_bytes(lengths)
        n = len(lengths)
        gs, scratch = lr.Guarded.scratch(need)
        assert x.shape == (sum(sc.frames(L) for L in lengths), sc.MELS)
    gx, xd = lr.Guarded.tensor(x)
    go, out = lr.Guarded.filled((rows, sc.W0, sc.C0), dtype=_dtype(precision))
    _ffi.check(_ffi.lib().acx_test_stem(ctx.handle, _ffi.ptr(xd), _ffi.ptr(out), B, T, arr, n, max_blocks, _ffi.ptr(scratch), need, sp()))
    torch.cuda.synchronize()
    lr.assert_clean(out, gx, go, *([gs] if gs is not None else []))
    assert torch.equal(sc.bits(xd), sc.bits(x.to(xd.device))), "the input is read, never written"
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(sc.bits(a), sc.bits(b))


def _where(a, b):
    d = (sc.bits(a) != sc.bits(b)).nonzero()
    return "%d elements differ, the first at index %s" % (d.shape[0], tuple(d[0].tolist()))


def _check_bf16(name, got, case):
    """A bf16 tensor against float64: |error| <= bar + half a bf16 step of the binade the unrounded value can lie in, per element
    (the rule of test_block_bf16).  Prints and returns the worst error / bound."""
    bar = case.bar("bf16a")
    err = (got.detach().cpu().double() - case.ref).abs()
    ratio = float((err / (bar + sc.half_step_bf16(case.ref, bar))).max())
    print("%s [bf16a]: worst |hip - fp64| / (bar %.3g + half step) = %.3f, max error %.3g" % (name, bar, ratio, float(err.max())))
    assert ratio <= 1.0, (name, ratio)
    return ratio


# ---- a. the fp32 form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,kind", [(B, T, "randn3") for B, T in sc.UNIFORM] + [sc.PROBE_SHAPE + ("offset",), sc.PROBE_SHAPE + ("eps",)])
def test_fp32_form_against_float64(synth_sd, B, T, kind):
    """stem_kernel<false, false> within the case's bar under both fp32 precisions, and the same bits under both."""
    x, case, _ = sc.case(synth_sd, B, T, kind)
    outs = []
    for prec in F32_PRECISIONS:
        out = _run(_ctx(synth_sd, prec, kind), prec, x, B, T).view(case.ref.shape)
        case.check("a. stem fp32 form (%d,%d) %s" % (B, T, kind), out, prec)
        outs.append(out)
    assert _same_bits(outs[0], outs[1]), "fp32 and fp32_split differ: %s" % _where(outs[0], outs[1])


# ---- b. the bf16 store --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", sc.UNIFORM)
def test_bf16_store_is_the_fp32_form_rounded(synth_sd, B, T):
    """stem_kernel<true, false>: the template changes the store alone, so every element carries the bits of the fp32 form's value
    rounded to nearest even (acx_pack_bf16x2) -- a swapped channel, a wrong half-word, a truncating conversion or a skipped pixel
    all show; and the stored tensor is within bar + half a step of float64."""
    x, case, _ = sc.case(synth_sd, B, T)
    o32 = _run(_ctx(synth_sd, "fp32_split"), "fp32_split", x, B, T).view(case.ref.shape)
    o16 = _run(_ctx(synth_sd, "bf16a"), "bf16a", x, B, T).view(case.ref.shape)
    assert o16.dtype == torch.bfloat16
    _check_bf16("b. stem bf16 store (%d,%d)" % (B, T), o16, case)
    want = o32.to(torch.bfloat16)
    assert _same_bits(o16, want), "bf16 store differs from the rounded fp32 form: %s" % _where(o16, want)


# ---- c. the packed forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_packed_forms_equal_the_clips_alone(synth_sd, precision):
    """stem_kernel<*, true> on seven clips of mixed lengths (clip boundaries on odd rows, two equal neighbours, the minimum length,
    143 rows): every clip's rows carry the bits of the uniform form run on that clip alone, and are within the bar of float64."""
    ctx = _ctx(synth_sd, precision)
    x, clips = sc.packed_input(sc.PACKED, seed=62000)
    off = sc.row_offsets(sc.PACKED)
    out = _run(ctx, precision, x, lengths=sc.PACKED)
    assert out.shape[0] == off[-1] == 143
    sd64 = lr.to64(synth_sd)
    for i, clip in enumerate(clips):
        T = clip.shape[1]
        got = out[off[i]:off[i + 1]]
        solo = _run(ctx, precision, clip, 1, T)
        assert _same_bits(got, solo), "clip %d (%d rows at row %d) differs from the clip alone: %s" % (i, solo.shape[0], off[i], _where(got, solo))
        case = sc.stem_case(synth_sd, sd64, clip)
        name = "c. stem packed clip %d (T = %d, rows %d .. %d)" % (i, T, off[i], off[i + 1] - 1)
        if precision == "bf16a":
            _check_bf16(name, got.view(case.ref.shape), case)
        else:
            case.check(name, got.view(case.ref.shape), precision)


# ---- d. the walk --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_capped_grid_equals_the_uncapped_launch(synth_sd, precision):
    """(1, 101), 14 row pairs: one, two and three workgroups walk 14, 7 + 7 and 5 + 5 + 4 pairs -- up to seven trips of the loop
    unrolled by two, both staging pairs refilled and consumed many times, an odd and an even count per workgroup -- and give the
    bits of the launch with one workgroup per pair, in both output types."""
    B, T = sc.WALK_SHAPE
    x, case, _ = sc.case(synth_sd, B, T)
    ctx = _ctx(synth_sd, precision)
    full = _run(ctx, precision, x, B, T)
    for cap in sc.WALK_CAPS:
        out = _run(ctx, precision, x, B, T, max_blocks=cap)
        if precision == "bf16a":
            _check_bf16("d. stem walk (%d,%d) max_blocks %d" % (B, T, cap), out.view(case.ref.shape), case)
        else:
            case.check("d. stem walk (%d,%d) max_blocks %d" % (B, T, cap), out.view(case.ref.shape), precision)
        assert _same_bits(out, full), "max_blocks = %d differs from the uncapped launch: %s" % (cap, _where(out, full))


@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_third_pair_at_the_shipped_grid(synth_sd, precision):
    """(33, 1005) at the launcher's own grid: 4175 row pairs on 2048 workgroups, so 79 of them walk a third pair, read from a staging
    register that was refilled inside the loop.  The batch is three distinct clips eleven times over: clip b must carry the bits of
    clip b % 3 of a B = 3 launch (compared on the device), which is held to float64."""
    B, T = sc.BIG_SHAPE
    H = sc.h0(T)
    npairs = sc.pairs(B * H)
    assert npairs > 2 * sc.MAX_BLOCKS, "this case no longer walks a third row pair: %d pairs" % npairs
    assert max(sc.loop_trips(npairs, sc.grid(npairs))) >= 2
    n3 = sc.BIG_DISTINCT
    x3, case, _ = sc.case(synth_sd, n3, T)
    ctx = _ctx(synth_sd, precision)
    out3 = _run(ctx, precision, x3, n3, T)
    if precision == "bf16a":
        _check_bf16("d. stem (%d,%d), the distinct clips of the long walk" % (n3, T), out3.view(case.ref.shape), case)
    else:
        case.check("d. stem (%d,%d), the distinct clips of the long walk" % (n3, T), out3.view(case.ref.shape), precision)
    xbig = x3.cuda().repeat(B // n3, 1, 1)                           # clip b = clip b % 3
    out = _run(ctx, precision, xbig, B, T)
    same = sc.bits(out).view(B // n3, n3 * H, sc.W0, sc.C0) == sc.bits(out3)[None]
    if not bool(same.all()):
        bad = (~same).nonzero()
        raise AssertionError("%d elements of the long walk differ from the B = 3 launch, the first at (repeat, row, pixel, channel) %s"
                             % (bad.shape[0], tuple(bad[0].tolist())))


# ---- e. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(synth_sd):
    """Null pointers, B or T < 1, max_blocks out of range, a short or misaligned scratch, a clip under the minimum, no clips: non-zero
    and nothing launched -- the guarded output is still NaN; then one good call of each kind."""
    lib = _ffi.lib()
    ctx = _ctx(synth_sd, "fp32_split")
    B, T = 2, 9
    gx, x = lr.Guarded.tensor(sc.stem_input(B, T, 5))
    go, out = lr.Guarded.filled((B * sc.h0(T), sc.W0, sc.C0))

    def uni(h=ctx.handle, xp=x, op=out, B=B, T=T, mb=0):
        return lib.acx_test_stem(h, _ffi.ptr(xp), _ffi.ptr(op), B, T, None, 0, mb, None, 0, sp())
    for bad in (dict(h=None), dict(xp=None), dict(op=None), dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(mb=-1), dict(mb=sc.MAX_BLOCKS + 1)):
        assert uni(**bad) != 0, bad
    lengths = (sc.MIN_SAMPLES, 9000)
    arr, need, rows = sc.scratch_bytes(lengths)
    gxv, xv = lr.Guarded.tensor(sc.packed_input(lengths, 6)[0])
    gov, outv = lr.Guarded.filled((rows, sc.W0, sc.C0))
    gs, scratch = lr.Guarded.scratch(need + 256)
    short = (ctypes.c_int64 * 2)(sc.MIN_SAMPLES, sc.MIN_SAMPLES - 1)

    def var(xp=xv, op=outv, ln=arr, n=2, mb=0, scr=scratch, nbytes=need):
        return lib.acx_test_stem(ctx.handle, _ffi.ptr(xp), _ffi.ptr(op), 0, 0, ln, n, mb, _ffi.ptr(scr) if scr is not None else None, nbytes, sp())
    for bad in (dict(xp=None), dict(op=None), dict(ln=None), dict(n=0), dict(n=-1), dict(n=257), dict(mb=-1), dict(mb=sc.MAX_BLOCKS + 1),
                dict(scr=None), dict(nbytes=need - 256), dict(nbytes=0), dict(scr=scratch[4:]), dict(ln=short)):
        assert var(**bad) != 0, bad
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(outv.isnan().all()) and bool((scratch == 255).all())
    assert uni(mb=sc.MAX_BLOCKS) == 0 and var(mb=1) == 0
    torch.cuda.synchronize()
    lr.assert_clean(out, gx, go)
    lr.assert_clean(outv, gxv, gov, gs)
