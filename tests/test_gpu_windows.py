"""GPU (`-m gpu`): sliding windows over long recordings (acx_forward_windows, acx_window_timeline, ConvNeXt.forward_windows).

Correct means the project's invariant: every window's outputs are bit-identical to the uniform forward of that window cut out
and run alone, in every precision and with either frontend; the timeline equals a torch restatement of its definition."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.resample import resample

pytestmark = pytest.mark.gpu
SR = 32000
W10, H1 = 320000, 32000


def make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


def recordings(lengths, seed):
    return [synth.synth_waveforms(1, L, seed=seed + i)[0].cuda() for i, L in enumerate(lengths)]


def timeline_ref(probs, L, W, H, reduce):
    """Torch restatement of the definition: ascending-j fp32 sum then one division, or max."""
    starts = win.window_starts([L], W, H)
    rows = []
    for m in win.timeline_steps([L], W, H):
        js = [j for j, s in enumerate(starts) if s <= m < s + W]
        if reduce == "max":
            rows.append(probs[js].max(dim=0).values)
        else:
            acc = torch.zeros(probs.shape[1], dtype=torch.float32, device=probs.device)
            for j in js:
                acc = acc + probs[j]
            rows.append(acc / torch.tensor(float(len(js)), dtype=torch.float32, device=probs.device))
    return torch.stack(rows)


def check_windows(model, recs, W=W10, H=H1):
    out = model.forward_windows(recs, window=W / SR, hop=H / SR)
    scene = model.forward_windows(recs, window=W / SR, hop=H / SR, what="scene")
    frame = model.forward_windows(recs, window=W / SR, hop=H / SR, what="frame")
    assert len(out) == len(scene) == len(frame) == len(recs)
    for r, rec in enumerate(recs):
        L = rec.numel()
        starts = win.window_starts([L], W, H)
        assert torch.equal(out[r]["starts"], torch.tensor(starts, dtype=torch.float64) / SR)
        assert out[r]["clipwise_logits"].shape == (len(starts), 527) and scene[r]["scene"].shape == (len(starts), 768)
        assert out[r]["timeline"].shape == (-(-L // H), 527)
        for j, s in enumerate(starts):
            cut = rec[s:s + W][None]
            ref = model(cut)
            assert torch.equal(out[r]["clipwise_logits"][j], ref["clipwise_logits"][0]), (r, j)
            assert torch.equal(out[r]["clipwise_output"][j], ref["clipwise_output"][0]), (r, j)
            assert torch.equal(scene[r]["scene"][j], model.forward_scene_embeddings(cut)[0]), (r, j)
            assert torch.equal(frame[r]["frame"][j], model.forward_frame_embeddings(cut)[0]), (r, j)
    return out


LENGTHS = [1193600, 10 * SR, 61 * SR]             # 29, 1 and 52 windows of 10 s every 1 s


@pytest.mark.parametrize("precision", ["fp32_split", "fp32", "bf16", "bf16a"])
def test_every_window_bit_identical_to_its_cut(synth_sd, precision):
    check_windows(make_model(synth_sd, precision), recordings(LENGTHS, seed=100))


def test_dense_frontend(synth_sd):
    model = make_model(synth_sd, "fp32_split").set_frontend("dense")
    check_windows(model, recordings(LENGTHS[:2], seed=150))


def raw_windows(model, wav, lengths, W, H, first, count, mode, out0, out1, ws):
    ctx = model.native_context(wav.device)
    lens = (ctypes.c_int64 * len(lengths))(*lengths)
    return _ffi.lib().acx_forward_windows(ctx.handle, _ffi.ptr(wav), lens, len(lengths), W, H, first, count, mode,
                                          _ffi.ptr(out0), _ffi.ptr(out1), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(wav.device))


def raw_timeline(probs, lengths, W, H, reduce, out):
    lens = (ctypes.c_int64 * len(lengths))(*lengths)
    return _ffi.lib().acx_window_timeline(_ffi.ptr(probs), lens, len(lengths), W, H, reduce, _ffi.ptr(out),
                                          _ffi.stream_ptr(probs.device))


def test_nan_tail_and_ff_workspace(synth_sd):
    """No window reads past its own samples (the packed buffer ends in NaN, and in canary words behind them), no unwritten workspace
    is read (it starts as 0xFF bytes: every fp32 word a NaN; then as 0x7F bytes: 3.4e38, which no fmaxf drops --
    tests/forward_guard.py), nothing is written outside the acx_workspace_bytes_windows bytes or outside the outputs."""
    import forward_guard as fg
    model = make_model(synth_sd, "bf16a")
    W, H = 48000, 17000
    lengths = [130001, 48000, 97777]
    recs = recordings(lengths, seed=200)
    tail = 4096
    packed = torch.cat(recs + [torch.full((tail,), float("nan"), device="cuda")])
    n = _ffi.window_count(lengths, W, H)
    ctx = model.native_context(packed.device)
    need = ctx.workspace_bytes_windows(n, W, _ffi.MODE_LOGITS)
    seen = []

    def call(ws, ins, outs):
        assert ws.numel() == need
        seen.append(ins[0])
        return raw_windows(model, ins[0], lengths, W, H, 0, n, _ffi.MODE_LOGITS, outs[0], outs[1], ws)
    logits, probs = fg.run_guarded(need, [packed], [(n, 527), (n, 527)], call)
    for buf in seen:
        assert bool(torch.isnan(buf[sum(lengths):]).all())
    g = 0
    for r, rec in enumerate(recs):
        for s in win.window_starts([lengths[r]], W, H):
            assert torch.equal(logits[g], model(rec[s:s + W][None])["clipwise_logits"][0]), (r, s)
            g += 1
    assert g == n


def test_first_count_splits_equal_one_call(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    W, H = 64000, 9000
    lengths = [200000, 64000, 151234]
    packed = torch.cat(recordings(lengths, seed=300))
    n = _ffi.window_count(lengths, W, H)
    ctx = model.native_context(packed.device)
    ws = torch.empty(ctx.workspace_bytes_windows(n, W, _ffi.MODE_SCENE), dtype=torch.uint8, device="cuda")
    whole = torch.empty((n, 768), device="cuda")
    _ffi.check(raw_windows(model, packed, lengths, W, H, 0, n, _ffi.MODE_SCENE, whole, None, ws))
    parts = torch.empty((n, 768), device="cuda")
    for first, count in ((0, 5), (5, 1), (6, 17), (23, n - 23)):
        _ffi.check(raw_windows(model, packed, lengths, W, H, first, count, _ffi.MODE_SCENE, parts[first:first + count], None, ws))
    torch.cuda.synchronize()
    assert torch.equal(parts, whole)
    recs = recordings([int(23.5 * SR), 12 * SR], seed=310)
    a = model.forward_windows(recs, window=2.0, hop=0.5, max_batch=7)
    b = model.forward_windows(recs, window=2.0, hop=0.5, max_batch=64)
    for x, y in zip(a, b):
        for k in ("starts", "clipwise_logits", "clipwise_output", "timeline"):
            assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_timeline_matches_definition(synth_sd, reduce):
    model = make_model(synth_sd, "fp32_split")
    for W, H, lengths in ((W10, H1, LENGTHS[:2]), (48000, 7000, [100001, 30000, 48000]), (16000, 16000, [64321])):
        recs = recordings(lengths, seed=400)
        out = model.forward_windows(recs, window=W / SR, hop=H / SR, timeline=reduce)
        for r, L in enumerate(lengths):
            ref = timeline_ref(out[r]["clipwise_output"], L, W, H, reduce)
            assert torch.equal(out[r]["timeline"], ref), (W, H, L)
    assert "timeline" not in model.forward_windows(recs, window=0.5, timeline=None)[0]
    # the C call on its own, over random probabilities: a zero-length recording (one window, no row: it shares its row offset
    # with its successor), lengths around the window, and R = 256, the most recordings one call takes
    W, cycle = 7360, (0, 1, 7359, 7360, 7361, 11040, 22097)
    for N in (3, 527):
        for H in (3680, 7360):
            for R in (1, 256):
                lengths = [cycle[r % len(cycle)] for r in range(R)]
                counts = [len(win.window_starts([L], W, H)) for L in lengths]
                probs = torch.rand((sum(counts), N), generator=torch.Generator().manual_seed(N + H + R))
                rows = len(win.timeline_steps(lengths, W, H))
                out = torch.full((max(rows, 1), N), -1.0, device="cuda")
                lens = (ctypes.c_int64 * R)(*lengths)
                _ffi.check(_ffi.lib().acx_window_timeline_classes(_ffi.ptr(probs.cuda()), N, lens, R, W, H, int(reduce == "max"),
                                                                  _ffi.ptr(out), _ffi.stream_ptr(out.device)))
                blocks = probs.split(counts)
                ref = [timeline_ref(blocks[r], L, W, H, reduce) for r, L in enumerate(lengths) if L > 0]
                ref = torch.cat(ref) if ref else torch.empty((0, N))
                assert ref.shape == (rows, N) and torch.equal(out[:rows].cpu(), ref), (N, H, R)


def test_sample_rate_equals_resample_then_windows(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    recs = [synth.synth_waveforms(1, n, seed=500 + i)[0].cuda() for i, n in enumerate([int(25.3 * 44100), 6 * 44100])]
    a = model.forward_windows(recs, window=4.0, hop=1.5, sample_rate=44100)
    b = model.forward_windows([resample(r, 44100) for r in recs], window=4.0, hop=1.5)
    for x, y in zip(a, b):
        for k in ("starts", "clipwise_logits", "clipwise_output", "timeline"):
            assert torch.equal(x[k], y[k]), k


def test_short_recording_is_one_window(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    rec = recordings([123457], seed=600)[0]
    out = model.forward_windows(rec)                    # one dict for one tensor
    assert out["clipwise_logits"].shape == (1, 527) and torch.equal(out["starts"], torch.zeros(1, dtype=torch.float64))
    assert torch.equal(out["clipwise_logits"], model(rec[None])["clipwise_logits"])
    assert torch.equal(out["clipwise_output"], model(rec[None])["clipwise_output"])
    assert out["timeline"].shape == (1, 527) and torch.equal(out["timeline"][0], out["clipwise_output"][0])
    fr = model.forward_windows(rec, what="frame")["frame"]
    assert torch.equal(fr, model.forward_frame_embeddings(rec[None]))


def test_graph_capture_replay(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    W, H = 48000, 16000
    lengths = [150000, 60001]
    packed = torch.cat(recordings(lengths, seed=700))
    n = _ffi.window_count(lengths, W, H)
    steps = len(win.timeline_steps(lengths, W, H))
    ctx = model.native_context(packed.device)
    ws = torch.empty(ctx.workspace_bytes_windows(n, W, _ffi.MODE_LOGITS), dtype=torch.uint8, device="cuda")
    logits, probs = torch.empty((n, 527), device="cuda"), torch.empty((n, 527), device="cuda")
    tl = torch.empty((steps, 527), device="cuda")

    def run():
        _ffi.check(raw_windows(model, packed, lengths, W, H, 0, n, _ffi.MODE_LOGITS, logits, probs, ws))
        _ffi.check(raw_timeline(probs, lengths, W, H, 0, tl))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                            # warm-up: side streams of this stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    fresh = torch.cat(recordings(lengths, seed=710))
    packed.copy_(fresh)
    g.replay()
    torch.cuda.synchronize()
    got = (logits.clone(), probs.clone(), tl.clone())
    run()
    torch.cuda.synchronize()
    assert torch.equal(got[0], logits) and torch.equal(got[1], probs) and torch.equal(got[2], tl)
    ref = model.forward_windows([fresh[:lengths[0]], fresh[lengths[0]:]], window=W / SR, hop=H / SR)
    assert torch.equal(got[1], torch.cat([ref[0]["clipwise_output"], ref[1]["clipwise_output"]]))
    assert torch.equal(got[2], torch.cat([ref[0]["timeline"], ref[1]["timeline"]]))


def test_error_paths(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    W, H = 48000, 16000
    lengths = [150000, 40000]
    packed = torch.cat(recordings(lengths, seed=800))
    ctx = model.native_context(packed.device)
    ws = torch.empty(ctx.workspace_bytes_windows(8, W, _ffi.MODE_LOGITS), dtype=torch.uint8, device="cuda")
    o0, o1 = torch.empty((8, 527), device="cuda"), torch.empty((8, 527), device="cuda")
    rc = raw_windows(model, packed, lengths, W, H, 0, 8, _ffi.MODE_LOGITS, o0, o1, ws)
    msg = _ffi.lib().acx_last_error().decode()
    assert rc == -4 and "recording 1" in msg and "acx_forward_varlen" in msg
    lengths, packed = lengths[:1], packed[:lengths[0]]
    n = _ffi.window_count(lengths, W, H)
    assert raw_windows(model, packed, lengths, W, H, 0, n, 3, o0, o1, ws) == -1
    assert raw_windows(model, packed, lengths, W, H, 0, n, _ffi.MODE_LOGITS, o0, None, ws) == -1
    assert raw_windows(model, packed, lengths, W, H, 0, n, _ffi.MODE_LOGITS, o0, o1, ws[:4096]) == -5
    assert raw_windows(model, packed, lengths, W, H, 0, n + 1, _ffi.MODE_LOGITS, o0, o1, ws) == -1
    assert raw_windows(model, packed, lengths, W, H, 3, n - 2, _ffi.MODE_LOGITS, o0, o1, ws) == -1
    assert raw_windows(model, packed, lengths, W, W + 1, 0, n, _ffi.MODE_LOGITS, o0, o1, ws) == -1
    assert raw_timeline(o1, lengths, W, H, 2, o0) == -1
    assert _ffi.lib().acx_window_timeline(None, (ctypes.c_int64 * 1)(*lengths), 1, W, H, 0, _ffi.ptr(o0), None) == -1
    with pytest.raises(RuntimeError, match="model.eval"):
        model.train().forward_windows(packed)
    model.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        model.forward_windows(packed.cpu())
    with pytest.raises(RuntimeError, match="too short"):
        model.forward_windows([packed, packed[:7000]], window=1.0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="but model on"):
            model.forward_windows(packed.to("cuda:1"))
