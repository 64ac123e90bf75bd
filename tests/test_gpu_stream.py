"""GPU (`-m gpu`): live streams (ConvNeXt.stream, acx_stream_*).

Correct means the stream invariant: gather everything a slot's recording emits over all its pushes and its close, and it equals
forward_windows of the whole recording -- starts, per-window outputs and timeline rows -- bit for bit, for any chunking."""
import random
import zlib

import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

from stream_cases import check_equal, run_stream

pytestmark = pytest.mark.gpu
SR = 32000
W, H = 320000, 32000


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(0)


def make_model(sd, precision="fp32_split"):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


LENGTHS = [W - 1, W, W + 7, 3 * W + H // 2, 65 * SR]


@pytest.mark.parametrize("precision,what,timeline,frontend", [
    ("fp32_split", "logits", "mean", "auto"),
    ("fp32_split", "scene", None, "auto"),
    ("bf16a", "logits", "max", "auto"),
    ("bf16a", "frame", None, "auto"),
    ("fp32", "logits", "mean", "auto"),
    ("bf16", "logits", "max", "auto"),
    ("fp32_split", "logits", "mean", "dense"),
])
def test_stream_equals_forward_windows(sd, precision, what, timeline, frontend):
    model = make_model(sd, precision).set_frontend(frontend)
    recs = [synth.synth_waveforms(1, L, seed=11 + i)[0].cuda() for i, L in enumerate(LENGTHS)]
    st = model.stream(slots=len(recs), window=W / SR, hop=H / SR, what=what, timeline=timeline, max_push=2.0)
    results = run_stream(st, recs, random.Random(zlib.crc32((precision + what + frontend).encode())), 2 * SR)
    assert all(d["short"] == [] for d in results)
    check_equal(model, recs, results, W, H, what, timeline)


@pytest.mark.parametrize("rate,lengths", [
    (44100, [441000 - 1, 441000 * 3 + 17, 44100 * 301 + 5]),     # the last one takes n * of past 2^31
    (48000, [480000 + 3, 48000 * 25]),
    (16000, [160000 - 5, 16000 * 27 + 1]),
])
def test_stream_resampled(sd, rate, lengths):
    model = make_model(sd)
    recs = [synth.synth_waveforms(1, L, seed=31 + i)[0].cuda() for i, L in enumerate(lengths)]
    st = model.stream(slots=len(recs), window=W / SR, hop=H / SR, sample_rate=rate, max_push=4.0)
    # after one second everywhere, slot 0 is pushed a single sample while the others get a normal chunk in the same call
    lead = [[rate] * len(recs), [1] + [rate // 2 + 7] * (len(recs) - 1)]
    results = run_stream(st, recs, random.Random(rate), 4 * rate, lead=lead)
    check_equal(model, recs, results, W, H, rate=rate)


def test_stream_slot_reuse(sd):
    model = make_model(sd)
    a, b = (synth.synth_waveforms(1, L, seed=s)[0].cuda() for L, s in ((W + 5 * H + 3, 51), (2 * W + 11, 52)))
    st = model.stream(slots=2, window=W / SR, hop=H / SR)
    first = run_stream(st, [a], random.Random(1), 2 * SR)
    second = run_stream(st, [b], random.Random(2), 2 * SR)
    check_equal(model, [a], first, W, H)
    check_equal(model, [b], second, W, H)
    fresh = run_stream(model.stream(slots=2, window=W / SR, hop=H / SR), [b], random.Random(2), 2 * SR)
    for x, y in zip(second, fresh):
        assert torch.equal(x["clipwise_logits"], y["clipwise_logits"]) and torch.equal(x["timeline"], y["timeline"])


def test_stream_many_slots(sd):
    model = make_model(sd, "bf16a")
    n = 300
    recs = [synth.synth_waveforms(1, W + (i % 3) * H + i, seed=100 + i)[0].cuda() for i in range(n)]
    st = model.stream(slots=n, window=W / SR, hop=H / SR, max_push=4.0)
    results = [st.push(list(r[:W // 2] for r in recs)), st.push(list(r[W // 2:] for r in recs)), st.close()]
    for d in results:
        assert d["slot"].tolist() == sorted(d["slot"].tolist())
    for i in (0, 1, 255, 256, 299):
        check_equal(model, [recs[i]], results, W, H, slots=[i])


def test_stream_short(sd):
    model = make_model(sd)
    tiny = synth.synth_waveforms(1, _ffi.MIN_SAMPLES - 1, seed=7)[0].cuda()
    clip = synth.synth_waveforms(1, W // 2, seed=8)[0].cuda()
    st = model.stream(slots=3, window=W / SR, hop=H / SR)
    d0 = st.push({0: tiny, 2: clip})
    assert d0["slot"].numel() == 0
    d1 = st.close()
    assert d1["short"] == [0]
    assert d1["slot"].tolist() == [2] and d1["starts"].tolist() == [0.0]
    ref = model(clip[None])
    assert torch.equal(d1["clipwise_logits"], ref["clipwise_logits"])
    assert torch.equal(d1["clipwise_output"], ref["clipwise_output"])
    assert (d1["timeline_slot"] == 0).sum() == 0
    check_equal(model, [clip], [d0, d1], W, H, slots=[2])


def test_stream_two_handles_two_streams(sd):
    model = make_model(sd)
    recs = [synth.synth_waveforms(1, 3 * W + 7 * i, seed=200 + i)[0].cuda() for i in range(4)]
    sa = model.stream(slots=2, window=W / SR, hop=H / SR)
    sb = model.stream(slots=2, window=W / SR, hop=H / SR)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ra, rb = [], []
    step = 48000
    for p in range(0, 3 * W + 21, step):
        with torch.cuda.stream(s1):
            ra.append(sa.push({0: recs[0][p:p + step], 1: recs[1][p:p + step]}))
        with torch.cuda.stream(s2):
            rb.append(sb.push({0: recs[2][p:p + step], 1: recs[3][p:p + step]}))
    with torch.cuda.stream(s1):
        ra.append(sa.close())
    with torch.cuda.stream(s2):
        rb.append(sb.close())
    torch.cuda.synchronize()
    check_equal(model, recs[:2], ra, W, H)
    check_equal(model, recs[2:], rb, W, H)


def test_stream_past_2_31_samples(sd):
    model = make_model(sd, "bf16a")
    clip = synth.synth_waveforms(1, W, seed=77)[0].cuda()
    per = 64
    block = clip.repeat(per)                       # 64 windows of hop = window per push
    st = model.stream(slots=1, window=W / SR, hop=W / SR, timeline=None, max_push=per * W / SR)
    ref = model(clip[None])
    total = (1 << 31) // W + 2 * per               # windows: the recording runs past 2^31 samples
    pushes = -(-total // per)
    n_after = 0
    for k in range(pushes):
        d = st.push({0: block})
        starts = (d["starts"] * SR).round().to(torch.int64).tolist()
        first = k * per
        assert starts == [j * W for j in range(first, first + len(starts))]
        big = [i for i, s in enumerate(starts) if s + W > (1 << 31)]
        if big:
            assert torch.equal(d["clipwise_logits"][big], ref["clipwise_logits"].expand(len(big), -1))
            assert torch.equal(d["clipwise_output"][big], ref["clipwise_output"].expand(len(big), -1))
            n_after += len(big)
    d = st.close()
    assert n_after > per
    assert torch.equal(d["clipwise_logits"], ref["clipwise_logits"].expand(d["slot"].numel(), -1))
