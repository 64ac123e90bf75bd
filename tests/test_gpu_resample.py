"""GPU (`-m gpu`): input resampling on the device (acx_resample, pytorch.resample.resample, forward(..., sample_rate=),
forward_varlen(..., sample_rate=), extract(..., sample_rate=)).

Correct means: every output sample within the error bound of an fp32 FMA chain of the float64 formula; every clip's bits the
same however it is batched or packed; every forward with sample_rate= bit-identical to the forward of the resampled clips."""
import ctypes

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract
from audioset_convnext_inf_amd.pytorch.resample import resample
from audioset_convnext_inf_amd.utils.resample import resample as host_resample
import resample_cases as rc

pytestmark = pytest.mark.gpu
RATES = (8000, 11025, 16000, 22050, 24000, 44100, 48000, 88200, 96000, 44101)


def formula(x, orig):
    """float64 y, sum |h_k x_k| over each output's band, and the band length: the independent reference of
    tests/resample_cases.py, whose bands come from the definition and never from acx_resample_taps (the two are held equal at
    these rates by tests/test_resample_cases_cpu.py)."""
    return rc.reference(x, orig, 32000)


def inputs(orig, L, seed):
    rs = np.random.RandomState(seed)
    noise = rs.standard_normal(L).astype(np.float32)
    tone = np.sin(2 * np.pi * 997.0 * np.arange(L) / orig).astype(np.float32)
    loud = (1e4 * rs.uniform(-1, 1, L)).astype(np.float32)
    return {"noise": noise, "tone": tone, "loud": loud}


@pytest.mark.parametrize("orig", RATES)
def test_accuracy_against_the_float64_formula(orig):
    for L in (1000, 12345, 10 * orig):
        for name, x in inputs(orig, L, seed=L % 97).items():
            y = resample(torch.from_numpy(x).cuda(), orig).cpu().numpy().astype(np.float64)
            ref, mag, band = formula(x.astype(np.float64), orig)
            assert y.shape == ref.shape
            bound = (band + 1) * 2.0 ** -24 * mag * 1.001 + 1e-30
            bad = np.abs(y - ref) > bound
            assert not bad.any(), (orig, L, name, int(np.argmax(bad)), float(np.abs(y - ref).max()))
            if name == "noise" and orig != 44101:          # (the restatement's dense bank at 44101 Hz: 1.4e9 taps)
                # 2e-5 of full scale: the bar utils/resample.py meets against the formula at 8 / 16 / 44.1 / 48 kHz
                # (tests/test_next_rows_cpu.py).  At 11.025 / 22.05 kHz its float32 taps are 3.1e-5 off and it misses that
                # bar itself: there the bound is its own distance from the formula plus the kernel's.
                h = host_resample(torch.from_numpy(x)[None], orig, 32000)[0].numpy()
                own = np.abs(h - ref).max()
                assert np.abs(y - h).max() < max(2e-5 * max(1.0, np.abs(x).max()), own + bound.max()), (orig, L, own)


@pytest.mark.parametrize("orig", (44100, 48000, 16000, 88200))
def test_packed_equals_alone_bit_for_bit(orig):
    rs = np.random.RandomState(orig % 1000)
    lengths = [int(n) for n in rs.randint(1, 30000, size=30)] + [1, 2, orig // 100 + 1]
    clips = [torch.from_numpy(rs.standard_normal(n).astype(np.float32) * (1e4 if c % 2 else 1.0)).cuda()
             for c, n in enumerate(lengths)]
    out, out_len = resample(torch.cat(clips), orig, lengths=lengths)
    assert out_len == [_ffi.resampled_length(orig, 32000, n) for n in lengths] and out.numel() == sum(out_len)
    o = 0
    for c, n in zip(clips, out_len):
        assert torch.equal(out[o:o + n], resample(c, orig)), (orig, c.numel())
        o += n
    # more than 256 clips: several launches, same bits
    many = [int(n) for n in rs.randint(100, 3000, size=300)]
    clips = [torch.from_numpy(rs.standard_normal(n).astype(np.float32)).cuda() for n in many]
    out, out_len = resample(torch.cat(clips), orig, lengths=many)
    o = 0
    for c, n in zip(clips, out_len):
        assert torch.equal(out[o:o + n], resample(c[None], orig)[0])
        o += n
    # a uniform (B, L) batch
    x = torch.randn(5, 3, 20011, device="cuda")
    y = resample(x, orig)
    assert y.shape == (5, 3, _ffi.resampled_length(orig, 32000, 20011))
    for a in range(5):
        for b in range(3):
            assert torch.equal(y[a, b], resample(x[a, b], orig))


@pytest.mark.parametrize("orig", (44100, 48000, 8000, 44101))
def test_every_output_written_and_nothing_past_the_end(orig):
    lengths = [7, 44100, 1, 30001, 441]
    wav = torch.randn(sum(lengths), device="cuda")
    N = sum(_ffi.resampled_length(orig, 32000, n) for n in lengths)
    rs = _ffi.Resampler(torch.cuda.current_device(), orig, 32000)
    runs = []
    for _ in range(2):
        out = torch.full((N + 4096,), float("nan"), device="cuda")
        rs.run(wav, lengths, out[:N])
        torch.cuda.synchronize()
        assert torch.isfinite(out[:N]).all() and torch.isnan(out[N:]).all()
        runs.append(out[:N].clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    rs.close()


def make_model(sd, precision="fp32_split"):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


@pytest.mark.parametrize("precision", ["fp32_split", "fp32", "bf16", "bf16a"])
def test_forwards_equal_the_forward_of_the_resampled_clips(synth_sd, precision):
    model = make_model(synth_sd, precision)
    for rate in (44100, 48000):
        x = synth.synth_waveforms(2, rate * 3 // 2 + 7, seed=rate % 13).cuda()
        r = resample(x, rate)
        out, ref = model(x, sample_rate=rate), model(r)
        assert torch.equal(out["clipwise_logits"], ref["clipwise_logits"])
        assert torch.equal(out["clipwise_output"], ref["clipwise_output"])
        assert torch.equal(model.forward_scene_embeddings(x, sample_rate=rate), model.forward_scene_embeddings(r))
        assert torch.equal(model.forward_frame_embeddings(x, sample_rate=rate), model.forward_frame_embeddings(r))
        clips = [synth.synth_waveforms(1, n, seed=n)[0].cuda() for n in (rate, rate // 4 + 3, 2 * rate + 11)]
        v = model.forward_varlen(clips, sample_rate=rate)
        scene = model.forward_varlen(clips, what="scene", sample_rate=rate)
        frames = model.forward_varlen(clips, what="frame", sample_rate=rate)
        for i, c in enumerate(clips):
            one = model(c[None], sample_rate=rate)
            assert torch.equal(v["clipwise_logits"][i], one["clipwise_logits"][0])
            assert torch.equal(v["clipwise_output"][i], one["clipwise_output"][0])
            assert torch.equal(scene[i], model.forward_scene_embeddings(c[None], sample_rate=rate)[0])
            assert torch.equal(frames[i], model.forward_frame_embeddings(c[None], sample_rate=rate)[0])
    x = synth.synth_waveforms(2, 40000, seed=3).cuda()
    base = model(x)["clipwise_logits"]
    assert torch.equal(model(x, sample_rate=32000)["clipwise_logits"], base)
    assert torch.equal(model(x, sample_rate=None)["clipwise_logits"], base)
    assert torch.equal(model.forward_varlen([x[0], x[1]], what="scene", sample_rate=32000), model.forward_scene_embeddings(x))


@pytest.mark.parametrize("rate", (44100, 48000))
def test_parity_with_the_oracle_on_host_resampled_clips(synth_sd, rate):
    from oracle import ref_cpu
    model = make_model(synth_sd)
    x = synth.synth_waveforms(2, rate * 2, seed=7)
    out = model(x.cuda(), sample_rate=rate)
    scene = model.forward_scene_embeddings(x.cuda(), sample_rate=rate)
    h = host_resample(x, rate, 32000)
    ref = ref_cpu.forward(synth_sd, h)
    assert float((out["clipwise_logits"].cpu() - ref["clipwise_logits"]).abs().max()) < 1e-3
    assert float((out["clipwise_output"].cpu() - ref["clipwise_output"]).abs().max()) < 1e-3
    assert float((scene.cpu() - ref_cpu.forward_scene_embeddings(synth_sd, h)).abs().max()) < 1e-3


@pytest.mark.parametrize("pack", [False, True])
def test_extract_equals_resample_then_extract(synth_sd, pack):
    model = make_model(synth_sd)
    rs = np.random.RandomState(5)
    lens = [int(n) for n in rs.randint(11000, 100000, size=9)] + [44100, 44100, 44101]
    wavs = [synth.synth_waveforms(1, n, seed=i)[0] for i, n in enumerate(lens)]
    first = [resample(w.cuda(), 44100).cpu() for w in wavs]
    for what in ("logits", "scene", "frame"):
        got = extract(model, wavs, what=what, max_batch=4, pack=pack, sample_rate=44100)
        ref = extract(model, first, what=what, max_batch=4, pack=pack)
        for a, b in zip(got, ref):
            assert torch.equal(a, b), what


def test_graph_capture_replays_the_eager_bits(synth_sd):
    model = make_model(synth_sd)
    x = synth.synth_waveforms(3, 66150, seed=11).cuda()
    eager = model(x, sample_rate=44100)["clipwise_logits"].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(x, sample_rate=44100)                    # warm-up on the capture stream (workspace, resampler tables)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model(x, sample_rate=44100)
    x.copy_(synth.synth_waveforms(3, 66150, seed=12).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["clipwise_logits"], model(x, sample_rate=44100)["clipwise_logits"])
    x.copy_(synth.synth_waveforms(3, 66150, seed=11).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["clipwise_logits"], eager)


def test_error_paths(synth_sd):
    model = make_model(synth_sd)
    with pytest.raises(RuntimeError, match=r"10000 samples at 44100 Hz \(7257 samples at 32000 Hz\) is too short"):
        model(torch.zeros(1, 10000, device="cuda"), sample_rate=44100)
    with pytest.raises(RuntimeError, match=r"clip 1 of 10000 samples at 44100 Hz"):
        model.forward_varlen([torch.zeros(20000, device="cuda"), torch.zeros(10000, device="cuda")], sample_rate=44100)
    with pytest.raises(RuntimeError, match="too short"):
        extract(model, [np.zeros(20000, np.float32), np.zeros(10000, np.float32)], sample_rate=44100)
    with pytest.raises(ValueError, match="integer"):
        model(torch.zeros(1, 20000, device="cuda"), sample_rate=44100.5)
    with pytest.raises(_ffi.AcxError, match="767999/32000") as e:
        model(torch.zeros(1, 800000, device="cuda"), sample_rate=767999)
    assert e.value.code == -6
    rs = _ffi.Resampler(torch.cuda.current_device(), 44100, 32000)
    wav, out = torch.zeros(257 * 10, device="cuda"), torch.zeros(257 * 10, device="cuda")
    lens = (ctypes.c_int64 * 257)(*([10] * 257))
    lib = _ffi.lib()
    assert lib.acx_resample(rs._h, _ffi.ptr(wav), lens, 257, _ffi.ptr(out), None) == -1
    assert b"257" in lib.acx_last_error()
    assert lib.acx_resample(rs._h, _ffi.ptr(wav), lens, 0, _ffi.ptr(out), None) == -1
    neg = (ctypes.c_int64 * 1)(-1)
    assert lib.acx_resample(rs._h, _ffi.ptr(wav), neg, 1, _ffi.ptr(out), None) != 0
    rs.close()
