"""GPU (`-m gpu`): the resampler at every plan form, rate pair and tile edge, against float64.

resample_kernel and stream_resample_kernel form every output in res_tile (csrc/device_common.h), from an input span staged in LDS;
res_plan (csrc/resample.hip) gives a thread 4, 2 or 1 outputs, whichever span fits.  tests/resample_cases.py fixes the pairs,
lengths, the float64 reference (with its own bands: nothing here reads acx_resample_taps) and the derived bound
|y_dev - y| <= gamma_{c+1} sum |h_k x_k|; tests/test_resample_cases_cpu.py shows what they rest on.  Here:

  a. accuracy: every case of the table inside the bound (the worst error / bound per pair is printed: pytest -s);
  b. fences: input and output between canaries, NaN on both sides of the used samples, the output NaN before the call;
  c. zero-length clips in a packed batch;
  d. the walk: a capped grid bit-equal to the uncapped launch, and over 4096 tiles at the shipped grid;
  e. the same bits alone, packed, as a (B, L) batch and in a second run;
  f. the two-outputs-per-thread form under the model: sample_rate = 768000 in forwards, windows and a live stream;
  g. the refusals, which launch nothing.

Measured on an MI355X (worst error / bound per pair): profiles/resample_forms_error_over_bound.txt."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.resample import resample
import layer_ref as lr
import resample_cases as rc
import stream_cases as sc

pytestmark = pytest.mark.gpu
PAD = 64                                  # NaN words on each side of the used samples, inside the canaries
_resamplers = {}


def _rs(pair):
    if pair not in _resamplers:
        _resamplers[pair] = _ffi.Resampler(torch.cuda.current_device(), *pair)
    return _resamplers[pair]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for r in _resamplers.values():
        r.close()
    _resamplers.clear()


def bits(t):
    return t.contiguous().view(torch.int32)


def out_lengths(pair, lengths):
    of, nf = rc.reduced(*pair)
    return [rc.out_len(of, nf, n) for n in lengths]


def run_fenced(pair, clips, max_blocks=None, spare=0):
    """acx_resample (max_blocks None) or acx_test_resample on the packed clips (numpy fp32 arrays) inside fences: the input
    between canaries with PAD NaN words on both sides of the used samples, the output between canaries, NaN before the call and
    with `spare` more NaN words behind the total.  Afterwards the canaries are intact, every output is finite, the spare words
    are still NaN and the input is bit-identical.  -> the per-clip outputs, on the device."""
    lengths = [len(c) for c in clips]
    outs = out_lengths(pair, lengths)
    S, N = sum(lengths), sum(outs)
    host = np.full(S + 2 * PAD, np.nan, dtype=np.float32)
    host[PAD:PAD + S] = np.concatenate(clips) if S else []
    gx, xd = lr.Guarded.tensor(torch.from_numpy(host))
    before = bits(xd).clone()
    go, od = lr.Guarded.filled((N + spare,))
    lens = (ctypes.c_int64 * len(lengths))(*lengths)
    args = (_rs(pair)._h, _ffi.ptr(xd[PAD:]), lens, len(lengths), _ffi.ptr(od))
    sp = _ffi.stream_ptr(xd.device)
    if max_blocks is None:
        _ffi.check(_ffi.lib().acx_resample(*args, sp))
    else:
        _ffi.check(_ffi.lib().acx_test_resample(*args, max_blocks, sp))
    torch.cuda.synchronize()
    lr.assert_clean(od[:N], gx, go)
    assert bool(od[N:].isnan().all()), "a word of out beyond the total was written"
    assert torch.equal(bits(xd), before), "the input is read, never written"
    return list(torch.split(od[:N].clone(), outs))


def hold(name, got, x, pair):
    """got (device tensor) inside the bound of the float64 reference of clip x; -> the worst error / bound"""
    ref = rc.reference(x, *pair)
    got = got.cpu().numpy()
    assert got.shape == ref[0].shape, (name, got.shape, ref[0].shape)
    ratio, at = rc.worst_ratio(got, ref)
    assert ratio <= 1.0, "%s: output %d is %.3g bounds from float64 (%r, expected %r)" % (name, at, ratio, float(got[at]), float(ref[0][at]))
    return ratio


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- a. accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(rc.PAIRS), ids=rc.pair_id)
def test_every_case_inside_the_bound(pair):
    """Every length and input kind of the pair through pytorch.resample.resample(x, orig, new_freq=new)."""
    plan = _ffi.resample_plan(*pair)
    assert plan.per_thread == rc.PAIRS[pair]
    worst, n = 0.0, 0
    for L, kind, x in rc.cases(pair):
        y = resample(torch.from_numpy(x).cuda(), pair[0], new_freq=pair[1])
        worst = max(worst, hold("%d -> %d, %d samples of %s" % (pair + (L, kind)), y, x, pair))
        n += 1
    print("a. resample %6d -> %6d (per_thread %d): %d cases, worst |hip - fp64| / bound = %.3f" % (pair + (plan.per_thread, n, worst)))


# ---- b. fences --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(rc.FORM_PAIRS), ids=lambda q: "per_thread%d" % q)
def test_fenced_buffers(form):
    """One pair of each form: every case length packed into one call, noise and the loud kind alternating, between fences.  A read
    outside the packed input meets NaN, a store outside the output meets a canary; every clip is inside the bound and carries the
    bits of resample() on the clip alone."""
    pair = rc.FORM_PAIRS[form]
    clips = [rc.inputs(pair[0], L, seed=L % 89)["loud" if k % 2 else "noise"] for k, L in enumerate(rc.case_lengths(pair))]
    for k, (x, y) in enumerate(zip(clips, run_fenced(pair, clips))):
        hold("fenced %d -> %d, clip %d of %d samples" % (pair + (k, len(x))), y, x, pair)
        assert same(y, resample(torch.from_numpy(x).cuda(), pair[0], new_freq=pair[1])), (pair, k)


# ---- c. zero-length clips -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(rc.FORM_PAIRS), ids=lambda q: "per_thread%d" % q)
def test_zero_length_clips_in_a_packed_batch(form):
    """Lengths [0, L, 0, 0, L', 0] (tile offsets repeat: packed_find has to skip the empty clips) and [0] alone: each non-empty
    clip carries the bits of the same clip alone, and no word of out beyond the total is written."""
    pair = rc.FORM_PAIRS[form]
    p = rc.pair_plan(pair)
    T = p["outputs_per_tile"]
    La, Lb = rc.length_for(2 * T + 3, p["of"], p["nf"]), p["width"] + 1
    a, b = rc.inputs(pair[0], La, seed=11)["noise"], rc.inputs(pair[0], Lb, seed=12)["loud"]
    empty = np.zeros(0, dtype=np.float32)
    got = run_fenced(pair, [empty, a, empty, empty, b, empty], spare=2 * T)
    assert [g.numel() for g in got] == out_lengths(pair, [0, La, 0, 0, Lb, 0])
    alone_a, alone_b = run_fenced(pair, [a])[0], run_fenced(pair, [b])[0]
    assert same(got[1], alone_a) and same(got[4], alone_b)
    hold("packed among empty clips, %d samples" % La, got[1], a, pair)
    hold("packed among empty clips, %d samples" % Lb, got[4], b, pair)
    assert run_fenced(pair, [empty], spare=T)[0].numel() == 0           # nothing to do: nothing launched, out still NaN
    for cap in rc.WALK_CAPS:
        capped = run_fenced(pair, [empty, a, empty, empty, b, empty], max_blocks=cap, spare=2 * T)
        assert same(capped[1], alone_a) and same(capped[4], alone_b), cap


# ---- d. the walk --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(rc.FORM_PAIRS), ids=lambda q: "per_thread%d" % q)
def test_capped_grid_equals_the_uncapped_launch(form):
    """A clip of seven tiles (the last one short) and a short clip: one, two and three workgroups walk 8, 4 + 4 and 3 + 3 + 2 tiles,
    restaging s_in for every tile, crossing from one clip to the next inside a walk -- the bits of the launch with one workgroup
    per tile, and inside the bound."""
    pair = rc.FORM_PAIRS[form]
    p = rc.pair_plan(pair)
    T = p["outputs_per_tile"]
    La, Lb = rc.length_for(6 * T + T // 2 + 3, p["of"], p["nf"]), p["width"] + 1
    clips = [rc.inputs(pair[0], La, seed=21)["noise"], rc.inputs(pair[0], Lb, seed=22)["tone"]]
    assert sum(-(-n // T) for n in out_lengths(pair, [La, Lb])) == 8
    full = run_fenced(pair, clips)
    for x, y in zip(clips, full):
        hold("walk %d -> %d, %d samples" % (pair + (len(x),)), y, x, pair)
    for cap in rc.WALK_CAPS:
        capped = run_fenced(pair, clips, max_blocks=cap)
        assert all(same(c, f) for c, f in zip(capped, full)), "max_blocks = %d differs from the uncapped launch" % cap
    assert all(same(c, f) for c, f in zip(run_fenced(pair, clips, max_blocks=rc.MAX_GRID), full))


def test_second_sweep_at_the_shipped_grid():
    """8000 -> 32000 Hz (of / nf = 1 / 4, tiles of 1024) on 1048834 samples: 4195336 outputs in 4098 tiles on 4096 workgroups, so
    workgroups 0 and 1 restage s_in for a second tile -- one full, one of eight outputs.  The whole output is held to float64."""
    pair, L = rc.BIG_PAIR, rc.BIG_LENGTH
    plan = _ffi.resample_plan(*pair)
    N = rc.out_len(plan.of, plan.nf, L)
    tiles = -(-N // plan.outputs_per_tile)
    assert tiles > plan.max_grid == rc.MAX_GRID, "this case no longer walks a second tile: %d tiles" % tiles
    x = rc.inputs(pair[0], L, seed=4098)["noise"]
    y = run_fenced(pair, [x])[0]
    print("d. resample %d -> %d, %d tiles on %d workgroups: worst |hip - fp64| / bound = %.3f"
          % (pair + (tiles, plan.max_grid, hold("the second sweep", y, x, pair))))


# ---- e. bits across batchings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(rc.FORM_PAIRS), ids=lambda q: "per_thread%d" % q)
def test_same_bits_alone_packed_batched_and_again(form):
    pair = rc.FORM_PAIRS[form]
    p = rc.pair_plan(pair)
    T = p["outputs_per_tile"]
    L = rc.length_for(2 * T + 7, p["of"], p["nf"])
    x = torch.from_numpy(np.stack([rc.inputs(pair[0], L, seed=31 + b)["loud" if b == 1 else "noise"] for b in range(3)])).cuda()
    batch = resample(x, pair[0], new_freq=pair[1])
    assert batch.shape == (3, rc.out_len(p["of"], p["nf"], L))
    alone = [resample(x[b], pair[0], new_freq=pair[1]) for b in range(3)]
    lengths = [L, p["width"] - 1, L, 1, L]
    short = [torch.from_numpy(rc.inputs(pair[0], n, seed=41)["noise"]).cuda() for n in (p["width"] - 1, 1)]
    wav = torch.cat([x[0], short[0], x[1], short[1], x[2]])
    packed, lens = resample(wav, pair[0], new_freq=pair[1], lengths=lengths)
    assert lens == out_lengths(pair, lengths)
    parts = torch.split(packed, lens)
    again, _ = resample(wav, pair[0], new_freq=pair[1], lengths=lengths)
    assert same(again, packed)
    for b in range(3):
        assert same(batch[b], alone[b]) and same(parts[2 * b], alone[b]), (pair, b)
    for k, s in zip((1, 3), short):
        assert same(parts[k], resample(s, pair[0], new_freq=pair[1])), (pair, k)


# ---- f. the form reaches the model ---------------------------------------------------------------------------------------------------
def make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_model_rate_768k_equals_the_forward_of_the_resampled_clips(synth_sd, precision):
    """sample_rate = 768000 (per_thread = 2): 0.5 s is 384000 samples in and 16000 out.  model(x, sample_rate=), forward_varlen and
    forward_windows are bit-equal to the same call on resample(x, 768000), which is inside the bound of float64."""
    rate = rc.MODEL_FORM_RATE
    assert _ffi.resample_plan(rate, 32000).per_thread == 2
    model = make_model(synth_sd, precision)
    x = synth.synth_waveforms(2, rate // 2, seed=77).cuda()
    r = resample(x, rate)
    assert r.shape == (2, 16000)
    hold("768 kHz clip", r[1], x[1].cpu().numpy(), (rate, 32000))
    out, ref = model(x, sample_rate=rate), model(r)
    assert torch.equal(out["clipwise_logits"], ref["clipwise_logits"]) and torch.equal(out["clipwise_output"], ref["clipwise_output"])
    clips = [x[0], x[1, :rate // 4 + 1001]]
    v = model.forward_varlen(clips, sample_rate=rate)
    w = model.forward_varlen([resample(c, rate) for c in clips])
    assert torch.equal(v["clipwise_logits"], w["clipwise_logits"]) and torch.equal(v["clipwise_output"], w["clipwise_output"])
    a = model.forward_windows(x[0], window=0.25, hop=0.1, sample_rate=rate)
    b = model.forward_windows(r[0], window=0.25, hop=0.1)
    for k in ("starts", "clipwise_logits", "clipwise_output", "timeline"):
        assert torch.equal(a[k], b[k]), k
    assert a["clipwise_logits"].shape[0] == 4


def test_stream_at_768k_equals_forward_windows(synth_sd):
    """stream_resample_kernel in the same form: the 768 kHz case of tests/stream_cases.py (W = 0.5 s, H = 0.25 s, odd push
    sizes, the stream state poisoned) emits what forward_windows gives on each whole recording, bit for bit."""
    c = sc.FORM_CASE
    model = make_model(synth_sd, "fp32_split")
    sc.form_sim()                                         # asserts the reach: ring mirror, wrapped append, both paths, wrapped cover
    recs = [synth.synth_waveforms(1, L, seed=760 + i)[0].cuda() for i, L in enumerate(c["recs"])]
    st = model.stream(slots=len(recs), window=c["W"] / sc.SR, hop=c["H"] / sc.SR, sample_rate=c["rate"],
                      max_push=Fraction(c["max_push"], c["rate"]))
    st.poison()
    results = sc.run_plans(st, recs, sc.form_plans())
    sc.check_equal(model, recs, results, c["W"], c["H"], rate=c["rate"])


# ---- g. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """A ratio no form fits, max_blocks 0 and 4097, a null `in` with samples to read: each returns its error and launches nothing --
    the guarded output is still NaN; then one good call."""
    lib = _ffi.lib()
    h = _ffi._vp()
    assert lib.acx_resampler_create(torch.cuda.current_device(), *rc.REFUSED, ctypes.byref(h)) == rc.ERR_UNSUPPORTED and not h.value
    assert b"54/1" in lib.acx_last_error()
    with pytest.raises(_ffi.AcxError, match="54/1") as e:
        resample(torch.zeros(5400, device="cuda"), rc.REFUSED[0], new_freq=rc.REFUSED[1])
    assert e.value.code == rc.ERR_UNSUPPORTED
    pair = rc.FORM_PAIRS[2]
    L = 5000
    gx, x = lr.Guarded.tensor(torch.from_numpy(rc.inputs(pair[0], L, seed=3)["noise"]))
    N = out_lengths(pair, [L])[0]
    go, out = lr.Guarded.filled((N,))
    lens, sp = (ctypes.c_int64 * 1)(L), _ffi.stream_ptr(x.device)
    rs = _rs(pair)._h
    for cap in (0, rc.MAX_GRID + 1, -1):
        assert lib.acx_test_resample(rs, _ffi.ptr(x), lens, 1, _ffi.ptr(out), cap, sp) == rc.ERR_ARG, cap
        assert b"max_blocks" in lib.acx_last_error()
    assert lib.acx_test_resample(rs, None, lens, 1, _ffi.ptr(out), 1, sp) == rc.ERR_ARG
    assert lib.acx_resample(rs, None, lens, 1, _ffi.ptr(out), sp) == rc.ERR_ARG
    assert lib.acx_test_resample(None, _ffi.ptr(x), lens, 1, _ffi.ptr(out), 1, sp) == rc.ERR_ARG
    assert lib.acx_test_resample(rs, _ffi.ptr(x), lens, 1, None, 1, sp) == rc.ERR_ARG
    assert lib.acx_test_resample(rs, _ffi.ptr(x), lens, rc.MAX_CLIPS + 1, _ffi.ptr(out), 1, sp) == rc.ERR_ARG
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and gx.intact() and go.intact()
    assert lib.acx_test_resample(rs, _ffi.ptr(x), lens, 1, _ffi.ptr(out), rc.MAX_GRID, sp) == 0
    torch.cuda.synchronize()
    lr.assert_clean(out, gx, go)
