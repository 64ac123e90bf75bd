"""GPU (`-m gpu`): variable-length batches (acx_forward_varlen, ConvNeXt.forward_varlen, extract(pack=True)).

Correct means the project's invariant: every clip of a packed batch gives exactly the bits of the uniform forward of that clip
alone, in every precision and with either frontend."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract

pytestmark = pytest.mark.gpu
L10 = 320000


def stage_h(L):
    h = [((L // 320 + 1) + 4) // 4 + 1]
    for _ in range(3):
        h.append(h[-1] // 2)
    return h


# the minimum, one past it, an odd height at stages 0 / 1 / 2, 10 s, 10 s + 319, 30 s, and two equal lengths side by side
EDGE_LENGTHS = [7360, 7361, 17000, 16000, 23000, L10, L10 + 319, 960000, 48000, 48000]


def test_edge_lengths_cover_the_odd_heights():
    assert stage_h(17000)[0] % 2 == 1 and stage_h(16000)[1] % 2 == 1 and stage_h(23000)[2] % 2 == 1


def make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to("cuda").eval().set_precision(precision)


def clips_of(lengths, seed):
    return [synth.synth_waveforms(1, L, seed=seed + i)[0].cuda() for i, L in enumerate(lengths)]


def check_all_outputs(model, clips):
    from oracle import ref_cpu
    out = model.forward_varlen(clips)
    scene = model.forward_varlen(clips, what="scene")
    frames = model.forward_varlen(clips, what="frame")
    assert out["clipwise_logits"].shape == (len(clips), 527) and scene.shape == (len(clips), 768)
    for i, c in enumerate(clips):
        ref = model(c[None])
        assert torch.equal(out["clipwise_logits"][i], ref["clipwise_logits"][0]), (i, c.numel())
        assert torch.equal(out["clipwise_output"][i], ref["clipwise_output"][0]), (i, c.numel())
        assert torch.equal(scene[i], model.forward_scene_embeddings(c[None])[0]), (i, c.numel())
        h3, w3 = ref_cpu.out_hw(c.numel())[3]
        assert tuple(frames[i].shape) == (768, h3, w3), (i, c.numel())
        assert torch.equal(frames[i], model.forward_frame_embeddings(c[None])[0]), (i, c.numel())


@pytest.mark.parametrize("precision", ["fp32_split", "fp32", "bf16", "bf16a"])
def test_ragged_batch_bit_identical_per_clip(synth_sd, precision):
    model = make_model(synth_sd, precision)
    check_all_outputs(model, clips_of(EDGE_LENGTHS, seed=100))


def test_ragged_batch_dense_frontend(synth_sd):
    model = make_model(synth_sd, "fp32_split").set_frontend("dense")
    check_all_outputs(model, clips_of([7360, 17000, 23000, L10 + 319, 48000, 48000], seed=200))


def test_equal_lengths_match_uniform_and_permutation(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    x = synth.synth_waveforms(5, 48000, seed=300).cuda()
    ref = model(x)["clipwise_logits"]
    out = model.forward_varlen(list(x))["clipwise_logits"]
    assert torch.equal(out, ref)
    clips = clips_of([23000, 7360, L10, 17000], seed=310)
    base = model.forward_varlen(clips, what="scene")
    perm = [2, 0, 3, 1]
    permuted = model.forward_varlen([clips[p] for p in perm], what="scene")
    assert torch.equal(permuted, base[perm])


def test_one_clip_against_oracle(synth_sd):
    from oracle import ref_cpu
    model = make_model(synth_sd, "fp32_split")
    clips = clips_of([7360, 40000, 17000], seed=400)
    out = model.forward_varlen(clips)
    ref = ref_cpu.forward(synth_sd, clips[1][None].cpu())
    assert float((out["clipwise_logits"][1].cpu() - ref["clipwise_logits"][0]).abs().max()) < 1e-3


def raw_forward(model, packed, lengths, mode, ws, out0, out1):
    ctx = model.native_context(packed.device)
    lens = (ctypes.c_int64 * len(lengths))(*lengths)
    return _ffi.lib().acx_forward_varlen(ctx.handle, _ffi.ptr(packed), lens, len(lengths), mode, _ffi.ptr(out0),
                                         _ffi.ptr(out1), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(packed.device))


def test_nan_workspace_and_canary_tail(synth_sd):
    """Nothing reads unwritten workspace (it starts as 0xFF bytes -- NaN -- and again as 0x7F bytes -- 3.4e38, which no fmaxf drops:
    tests/forward_guard.py), nothing writes outside the acx_workspace_bytes_varlen bytes, the packed input or the outputs: canaries
    lie directly at both ends of each."""
    import forward_guard as fg
    model = make_model(synth_sd, "bf16a")
    lengths = [7361, 23000, L10 + 319, 16000]
    clips = clips_of(lengths, seed=500)
    packed = torch.cat(clips)
    ctx = model.native_context(packed.device)
    need = ctx.workspace_bytes_varlen(lengths, _ffi.MODE_LOGITS)

    def call(ws, ins, outs):
        assert ws.numel() == need
        return raw_forward(model, ins[0], lengths, _ffi.MODE_LOGITS, ws, outs[0], outs[1])
    logits, probs = fg.run_guarded(need, [packed], [(4, 527), (4, 527)], call)
    for i, c in enumerate(clips):
        assert torch.equal(logits[i], model(c[None])["clipwise_logits"][0]), i
        assert torch.equal(probs[i], model(c[None])["clipwise_output"][0]), i


def test_graph_capture_replay(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    lengths = [17000, 7360, 48000]
    packed = torch.cat(clips_of(lengths, seed=600))
    model.forward_varlen(packed, lengths, what="scene")                       # warm-up: workspace, context
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.forward_varlen(packed, lengths, what="scene")
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.forward_varlen(packed, lengths, what="scene")
    fresh = torch.cat(clips_of(lengths, seed=700))
    packed.copy_(fresh)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model.forward_varlen(fresh, lengths, what="scene"))


def test_error_paths(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    with pytest.raises(RuntimeError, match=r"clip 1 .*kernel size can't be greater than actual input size"):
        model.forward_varlen(clips_of([8000, 7359], seed=800))
    with pytest.raises(ValueError):
        model.forward_varlen([])
    with pytest.raises(ValueError, match="lengths sum"):
        model.forward_varlen(torch.zeros(20000, device="cuda"), [8000, 8000])
    with pytest.raises(RuntimeError, match="GPU only"):
        model.forward_varlen([torch.zeros(8000)])
    packed = torch.zeros(8000 * 257, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    o0, o1 = torch.empty((257, 527), device="cuda"), torch.empty((257, 527), device="cuda")
    rc = raw_forward(model, packed, [8000] * 257, _ffi.MODE_LOGITS, ws, o0, o1)
    assert rc != _ffi.OK and b"257" in _ffi.lib().acx_last_error()
    rc = raw_forward(model, packed, [], _ffi.MODE_LOGITS, ws, o0, o1)
    assert rc != _ffi.OK
    rc = raw_forward(model, packed, [8000, 7000], _ffi.MODE_LOGITS, ws, o0, o1)
    assert rc != _ffi.OK and b"clip 1" in _ffi.lib().acx_last_error()


def test_wrapper_chunks_past_256_clips(synth_sd):
    model = make_model(synth_sd, "fp32_split")
    lengths = [7360 + 37 * (i % 11) for i in range(300)]
    clips = clips_of(lengths, seed=900)
    out = model.forward_varlen(clips, what="scene")
    assert out.shape == (300, 768)
    for i in (0, 255, 256, 299):
        assert torch.equal(out[i], model.forward_scene_embeddings(clips[i][None])[0]), i


@pytest.mark.parametrize("what", ["logits", "scene", "frame"])
def test_extract_pack_equals_bucketed(synth_sd, what):
    model = make_model(synth_sd, "fp32_split")
    lengths = [7360, 17000, 48000, 23000, 48000, 7361, 40000]
    clips = [synth.synth_waveforms(1, L, seed=1000 + i)[0] for i, L in enumerate(lengths)]
    a = extract(model, clips, what)
    b = extract(model, clips, what, pack=True, max_batch=3)
    assert len(a) == len(b) == len(clips)
    for i in range(len(clips)):
        assert a[i].shape == b[i].shape and torch.equal(a[i], b[i]), i
