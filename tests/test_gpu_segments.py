"""GPU (`-m gpu`): sound event detection -- segment-wise and frame-wise outputs (ConvNeXt.forward_segments,
forward_segment_embeddings, forward_varlen / forward_windows with what="segment", include/acx.h "sound event detection").

The references: recipe64 of tests/test_segments_cpu.py (the recipe in float64 torch, tied to the reference-made fixture
g6_segments.npz there), the fixture itself, and oracle/ref_cpu.py for the trunk."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import resample as rs
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from oracle import ref_cpu

_spec = importlib.util.spec_from_file_location("_segments_cpu_tests", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "test_segments_cpu.py"))
_cpu_tests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu_tests)
recipe64 = _cpu_tests.recipe64

pytestmark = pytest.mark.gpu
SR = 32000
LAYER_TOL = 1e-4         # tests/test_gpu_parity.py:19
E2E_TOL = 1e-3
PRECISIONS = ["fp32", "fp32_split", "bf16", "bf16a"]
KEYS = ("segmentwise_logits", "segmentwise_output", "clipwise_output")


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(0)


def head(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 768, generator=g) * 0.05, torch.randn(n, generator=g) * 0.1


def with_head(sd, w, b):
    out = dict(sd)
    out["head_audioset.weight"], out["head_audioset.bias"] = w, b
    return out


def make_model(state, precision="fp32_split"):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    n = state["head_audioset.weight"].shape[0]
    if n != 527:
        m.head_audioset = nn.Linear(768, n)
    m.load_state_dict(state)
    return m.to("cuda").eval().set_precision(precision)


@pytest.fixture(scope="module")
def model(sd):
    return make_model(sd)


def clips(B, L=SR, seed=11):
    return synth.synth_waveforms(B, L, seed=seed).cuda()


def maxdiff(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def check_against_recipe(out, emb, ref, tol, tag):
    """Prints each figure, then asserts."""
    figs = {"emb": maxdiff(emb, ref["emb"]), "logits": maxdiff(out["segmentwise_logits"], ref["logits"]),
            "probs": maxdiff(out["segmentwise_output"], ref["probs"]), "clip": maxdiff(out["clipwise_output"], ref["clip"])}
    print("segments %s: %s" % (tag, " ".join("%s=%.3e" % kv for kv in figs.items())))
    assert max(figs.values()) <= tol, (tag, figs)


# ---- 1. layer ---------------------------------------------------------------------------------------------------------------
def raw_segment_head(model, x, pool, with_head=True):
    """acx_segment_head on NHWC x (B, S, 7, 768) -> (emb, logits, probs)."""
    B, S = x.shape[:2]
    ctx = model.native_context(x.device)
    emb = torch.empty((B, S, 768), device="cuda")
    logits = torch.empty((B, S, ctx.classes), device="cuda") if with_head else None
    probs = torch.empty((B, S, ctx.classes), device="cuda") if with_head else None
    _ffi.check(_ffi.lib().acx_segment_head(ctx.handle, _ffi.ptr(x), B, S, pool, _ffi.ptr(emb), _ffi.ptr(logits), _ffi.ptr(probs),
                                           _ffi.stream_ptr(x.device)))
    return emb, logits, probs


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 10, 31, 94])
def test_layer_against_float64_recipe(model, sd, B, S):
    g = torch.Generator().manual_seed(1000 * B + S)
    x = torch.randn(B, S, 7, 768, generator=g)
    for pool in (1, 3, 5):
        emb, logits, probs = raw_segment_head(model, x.cuda(), pool)
        ref = recipe64(x.permute(0, 3, 1, 2), sd, pool)
        figs = (maxdiff(emb, ref["emb"]), maxdiff(logits, ref["logits"]), maxdiff(probs, ref["probs"]))
        print("layer B=%d S=%d pool=%d: emb=%.3e logits=%.3e probs=%.3e" % ((B, S, pool) + figs))
        assert max(figs) <= LAYER_TOL, (B, S, pool, figs)
        only_emb = raw_segment_head(model, x.cuda(), pool, with_head=False)[0]
        assert torch.equal(only_emb, emb)


def test_wide_pools_against_float64_recipe(model, sd):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 37, 7, 768, generator=g)
    for pool in (7, 31):
        emb, logits, _ = raw_segment_head(model, x.cuda(), pool)
        ref = recipe64(x.permute(0, 3, 1, 2), sd, pool)
        assert maxdiff(emb, ref["emb"]) <= LAYER_TOL and maxdiff(logits, ref["logits"]) <= LAYER_TOL, pool


# ---- 2. head bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 50, 527, 4096, 16384])
def test_head_bound(sd, N):
    w, b = (sd["head_audioset.weight"], sd["head_audioset.bias"]) if N == 527 else head(N, seed=300 + N)
    m = make_model(with_head(sd, w, b))
    wav = clips(3, 3 * SR, seed=41)
    with torch.no_grad():
        out = m.forward_segments(wav)
        emb = m.forward_segment_embeddings(wav)
    S = seg.segment_count(3 * SR)
    assert out["segmentwise_logits"].shape == (3, S, N) and out["clipwise_output"].shape == (3, N) and emb.shape == (3, S, 768)
    e = emb.double().cpu()
    w64, b64 = w.double(), b.double()
    ref = e @ w64.T + b64
    bound = 768 * 2.0 ** -24 * (e.abs() @ w64.abs().T) + 2.0 ** -24 * b64.abs()
    err = (out["segmentwise_logits"].double().cpu() - ref).abs()
    print("head bound N=%d: max err %.3e, max err / bound %.3f" % (N, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all()), (N, float((err - bound).max()))
    p_err = maxdiff(out["segmentwise_output"], torch.sigmoid(out["segmentwise_logits"].double()))
    assert p_err <= 1e-6, (N, p_err)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp32_split"])
def test_end_to_end_against_reference_fixture(sd, golden_dir, precision):
    g1 = np.load(os.path.join(golden_dir, "g1_demo.npz"))
    g6 = np.load(os.path.join(golden_dir, "g6_segments.npz"))
    wav = torch.from_numpy(g1["pcm16"].astype(np.float32) / 32768.0)[None, :].cuda()
    m = make_model(sd, precision)
    fc = torch.from_numpy(g6["frame_classes"])
    for pool in (1, 3, 5):
        with torch.no_grad():
            out = m.forward_segments(wav, pool=pool, resolution="frame")
            emb = m.forward_segment_embeddings(wav, pool=pool)
        ref = {k: torch.from_numpy(g6["%s_p%d" % (k, pool)])[None] for k in ("emb", "logits", "probs", "clip")}
        check_against_recipe(out, emb, ref, E2E_TOL, "g6 %s pool=%d" % (precision, pool))
        d = maxdiff(out["framewise_output"][0][:, fc.cuda()], torch.from_numpy(g6["frame_p%d" % pool]))
        print("segments g6 %s pool=%d: frame=%.3e" % (precision, pool, d))
        assert d <= E2E_TOL, (precision, pool, d)


@pytest.mark.parametrize("precision", ["fp32", "fp32_split"])
@pytest.mark.parametrize("L", [SR, 102400, 10 * SR])
def test_end_to_end_against_oracle(sd, precision, L):
    wav = synth.synth_waveforms(1, L, seed=500 + L % 97)
    m = make_model(sd, precision)
    frame = ref_cpu.forward_frame_embeddings(sd, wav)
    with torch.no_grad():
        out = m.forward_segments(wav.cuda())
        emb = m.forward_segment_embeddings(wav.cuda())
    check_against_recipe(out, emb, recipe64(frame, sd, 3), E2E_TOL, "oracle %s L=%d" % (precision, L))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tail_is_fp32_in_every_precision(sd, precision):
    """The segment outputs equal the float64 recipe on the SAME model's frame embeddings within the per-layer bar."""
    m = make_model(sd, precision)
    wav = clips(2, 5 * SR, seed=61)
    with torch.no_grad():
        frame = m.forward_frame_embeddings(wav)
        out = m.forward_segments(wav, pool=5)
        emb = m.forward_segment_embeddings(wav, pool=5)
    check_against_recipe(out, emb, recipe64(frame, sd, 5), LAYER_TOL, "own trunk %s" % precision)


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------
L_BITS = 102400 + 640        # 3.2 s and two frames: 10 segments


def embedded_head(sd, n=4096, at=1000):
    w, b = head(n, seed=7)
    w[at:at + 527], b[at:at + 527] = sd["head_audioset.weight"], sd["head_audioset.bias"]
    return with_head(sd, w, b)


def assert_same(a, b, tag):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (tag, k)


def test_bits_alone_vs_batch_of_64(model, sd, monkeypatch):
    wav = clips(64, L_BITS, seed=71)
    with torch.no_grad():
        whole = model.forward_segments(wav)
        whole_e = model.forward_segment_embeddings(wav)
        again = model.forward_segments(wav)
    assert_same(whole, again, "second run")
    assert model.native_context(wav.device).sub_batches(64) > 1
    for b in range(64):
        with torch.no_grad():
            one = model.forward_segments(wav[b:b + 1])
            one_e = model.forward_segment_embeddings(wav[b:b + 1])
        assert_same({k: whole[k][b:b + 1] for k in KEYS}, one, "position %d" % b)
        assert torch.equal(whole_e[b:b + 1], one_e), b
    monkeypatch.setenv("ACX_SPLIT_STREAMS", "0")              # read at acx_create: a fresh module = a fresh context
    unsplit = make_model(sd)
    assert unsplit.native_context(wav.device).sub_batches(64) == 1
    with torch.no_grad():
        assert_same(whole, unsplit.forward_segments(wav), "ACX_SPLIT_STREAMS=0")
        assert torch.equal(whole_e, unsplit.forward_segment_embeddings(wav))


def test_bits_through_varlen_windows_and_a_wide_head(model, sd):
    lengths = [SR, L_BITS, 5 * SR + 123, L_BITS, 7360]
    cl = [clips(1, n, seed=80 + i)[0] for i, n in enumerate(lengths)]
    with torch.no_grad():
        res = model.forward_varlen(cl, what="segment")
        res_e = model.forward_varlen(cl, what="segment_embeddings")
    for i, c in enumerate(cl):
        with torch.no_grad():
            one = model.forward_segments(c[None])
            one_e = model.forward_segment_embeddings(c[None])
        assert res[i]["segmentwise_logits"].shape == (seg.segment_count(lengths[i]), 527)
        assert_same({"segmentwise_logits": res[i]["segmentwise_logits"][None], "segmentwise_output": res[i]["segmentwise_output"][None],
                     "clipwise_output": res[i]["clipwise_output"][None]}, one, "varlen clip %d" % i)
        assert torch.equal(res_e[i][None], one_e), i
    # windows: every window against the window cut out
    rec = clips(1, 3 * L_BITS + 5000, seed=90)[0]
    W, H = L_BITS, 70000
    with torch.no_grad():
        r = model.forward_windows(rec, window=W / SR, hop=H / SR, what="segment")
        r_e = model.forward_windows(rec, window=W / SR, hop=H / SR, what="segment_embeddings")
    starts = win.window_starts([rec.numel()], W, H)
    assert r["segmentwise_output"].shape == (len(starts), seg.segment_count(W), 527) and len(starts) >= 4
    for j, s in enumerate(starts):
        with torch.no_grad():
            one = model.forward_segments(rec[s:s + W][None])
            one_e = model.forward_segment_embeddings(rec[s:s + W][None])
        assert_same({k: r[k][j:j + 1] for k in KEYS}, one, "window %d" % j)
        assert torch.equal(r_e["segment_embeddings"][j:j + 1], one_e), j
    # the AudioSet rows inside a 4096-row head
    wide = make_model(embedded_head(sd))
    for B in (1, 17):
        wav = clips(B, L_BITS, seed=95 + B)
        with torch.no_grad():
            a, z = model.forward_segments(wav), wide.forward_segments(wav)
        for k in KEYS:
            assert z[k].shape[-1] == 4096 and torch.equal(z[k][..., 1000:1527], a[k]), (B, k)


def test_existing_outputs_keep_their_bits(model):
    wav = clips(3, 2 * SR, seed=99)
    with torch.no_grad():
        before = (model(wav), model.forward_scene_embeddings(wav), model.forward_frame_embeddings(wav))
        model.forward_segments(wav, resolution="frame")
        model.forward_segment_embeddings(wav, pool=5)
        after = (model(wav), model.forward_scene_embeddings(wav), model.forward_frame_embeddings(wav))
    assert torch.equal(before[0]["clipwise_logits"], after[0]["clipwise_logits"])
    assert torch.equal(before[0]["clipwise_output"], after[0]["clipwise_output"])
    assert torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])


# ---- 5. derived outputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [102080, 104960, 112000])           # T % 32 = 0, 9, 31
def test_derived_outputs(model, L):
    T = L // 320 + 1
    assert T % 32 in (0, 9, 31)
    wav = clips(3, L, seed=L % 89)
    with torch.no_grad():
        out = model.forward_segments(wav, resolution="frame")
    S = seg.segment_count(L)
    assert out["segmentwise_output"].shape == (3, S, 527) and out["framewise_output"].shape == (3, T, 527)
    assert torch.equal(out["clipwise_output"], out["segmentwise_output"].max(1).values)
    idx = torch.from_numpy(seg.frame_to_segment(T, S)).cuda()
    assert torch.equal(out["framewise_output"], out["segmentwise_output"][:, idx])
    edges = out["segment_edges"]
    assert edges.dtype == torch.float64 and edges.device.type == "cpu" and edges.shape == (S + 1,)
    assert float(edges[-1]) == L / SR and float(edges[1]) == 0.32


def test_expand_varlen_through_the_c_abi(model):
    # the second case: a full table of 256 clips of the smallest legal lengths and one of 102080, rows that are no multiple of
    # the 16-byte store
    for lengths, N in (([SR, 112000, 7360, 104960], 37), ([102080 if b == 100 else 7360 + 319 * (b % 3) for b in range(256)], 3)):
        g = torch.Generator().manual_seed(5)
        blocks = [torch.rand(seg.segment_count(n), N, generator=g) for n in lengths]
        probs = torch.cat(blocks).cuda()
        frames = sum(n // 320 + 1 for n in lengths)
        out = torch.full((frames, N), -1.0, device="cuda")
        lens = (ctypes.c_int64 * len(lengths))(*lengths)
        _ffi.check(_ffi.lib().acx_segment_expand_varlen(_ffi.ptr(probs), lens, len(lengths), N, _ffi.ptr(out),
                                                        _ffi.stream_ptr(out.device)))
        want = torch.cat([b[torch.from_numpy(seg.frame_to_segment(n // 320 + 1, b.shape[0]))] for b, n in zip(blocks, lengths)])
        assert torch.equal(out.cpu(), want), (len(lengths), N)


def test_sample_rate_equals_resampled_input(model):
    x = synth.synth_waveforms(2, 3 * 44100 + 17, seed=33).cuda()
    with torch.no_grad():
        a = model.forward_segments(x, sample_rate=44100, resolution="frame")
        a_e = model.forward_segment_embeddings(x, sample_rate=44100)
        y = rs.resample(x, 44100)
        b = model.forward_segments(y, resolution="frame")
        b_e = model.forward_segment_embeddings(y)
    assert_same(a, b, "44100")
    assert torch.equal(a["framewise_output"], b["framewise_output"]) and torch.equal(a_e, b_e)
    assert float(a["segment_edges"][-1]) == x.shape[1] / 44100            # seconds of the input audio
    assert torch.equal(a["segment_edges"][:-1], b["segment_edges"][:-1])


# ---- 6. timeline ------------------------------------------------------------------------------------------------------------
def timeline_want(probs, cover, reduce):
    """The rows of seg.segment_timeline_cover reduced over probs (numpy, rows of N) as the definition says."""
    want = np.empty((len(cover), probs.shape[1]), dtype=np.float32)
    for k, row in enumerate(cover):
        rows = [probs[pr] for _, _, _, pr in row]
        if reduce == "max":
            want[k] = np.max(np.stack(rows), axis=0)
        else:
            acc = np.zeros(probs.shape[1], dtype=np.float32)
            for v in rows:                                    # fp32 sum in ascending window order
                acc = (acc + v).astype(np.float32)
            want[k] = acc / np.float32(len(rows))             # one fp32 division by the count
    return want


@pytest.mark.parametrize("hop", [L_BITS, 70000, 30720])
def test_segment_timeline(model, hop):
    W = L_BITS
    lengths = [3 * L_BITS + 5000, 40000, 2 * L_BITS, L_BITS]           # ragged; one shorter than the window, one equal to it
    recs = [clips(1, n, seed=120 + i)[0] for i, n in enumerate(lengths)]
    cover = seg.segment_timeline_cover(lengths, W, hop)
    for reduce in ("max", "mean"):
        with torch.no_grad():
            res = model.forward_windows(recs, window=W / SR, hop=hop / SR, what="segment", timeline=reduce)
        probs = torch.cat([r["segmentwise_output"].reshape(-1, 527) for r in res]).cpu().numpy()
        got = torch.cat([r["timeline"] for r in res]).cpu().numpy()
        assert got.shape == (len(cover), 527) == (sum(-(-n // 10240) for n in lengths), 527)
        assert np.array_equal(got, timeline_want(probs, cover, reduce)), (hop, reduce)
    with torch.no_grad():
        none = model.forward_windows(recs, window=W / SR, hop=hop / SR, what="segment", timeline=None)
    assert all("timeline" not in r for r in none)
    assert res[1]["segmentwise_output"].shape == (1, seg.segment_count(40000), 527)
    if hop != L_BITS:
        return
    # the C call on its own, over random probabilities: lengths around the window, a zero-length recording (no segment and no
    # row: it shares both offsets with its successor) and R = 256, the most recordings one call takes.  Recordings of 1 and
    # 7359 samples are shorter than a clip: the call refuses them, so they leave the cycle of lengths.
    lib, W, cycle = _ffi.lib(), 7360, (0, 7360, 7361, 11040, 22097)
    one = torch.zeros((1, 3), device="cuda")
    for short in (1, 7359):
        rc = lib.acx_segment_timeline(_ffi.ptr(one), 3, (ctypes.c_int64 * 2)(7360, short), 2, W, W, 0, _ffi.ptr(one), None)
        assert rc == -4 and "recording 1" in lib.acx_last_error().decode()
    for N in (3, 527):
        for H in (3680, 7360):
            for R in (1, 256):
                lengths = [cycle[r % len(cycle)] for r in range(R)]
                cover = seg.segment_timeline_cover(lengths, W, H)
                blocks = sum(len(win.window_starts([n], W, H)) * seg.window_segments(n, W) for n in lengths if n)
                probs = torch.rand((max(blocks, 1), N), generator=torch.Generator().manual_seed(N + H + R))
                out = torch.full((max(len(cover), 1), N), -1.0, device="cuda")
                lens = (ctypes.c_int64 * R)(*lengths)
                for reduce in ("max", "mean"):
                    _ffi.check(lib.acx_segment_timeline(_ffi.ptr(probs.cuda()), N, lens, R, W, H, int(reduce == "max"),
                                                        _ffi.ptr(out), _ffi.stream_ptr(out.device)))
                    assert np.array_equal(out[:len(cover)].cpu().numpy(), timeline_want(probs.numpy(), cover, reduce)), (N, H, R)


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------
def test_forward_segments_under_graph_capture(model):
    wav = clips(17, L_BITS, seed=140)             # a split batch
    with torch.no_grad():
        eager = {k: v.clone() for k, v in model.forward_segments(wav, resolution="frame").items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.no_grad():
            model.forward_segments(wav, resolution="frame")          # warm-up: workspace and side streams of this stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            with torch.no_grad():
                out = model.forward_segments(wav, resolution="frame")
    torch.cuda.synchronize()
    for _ in range(2):
        for k in KEYS + ("framewise_output",):
            out[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in KEYS + ("framewise_output",):
            assert torch.equal(out[k], eager[k]), k


# ---- 8. errors --------------------------------------------------------------------------------------------------------------
def test_c_abi_errors(model):
    lib = _ffi.lib()
    ctx = model.native_context(torch.device("cuda", torch.cuda.current_device()))
    L, B = SR, 2
    S = seg.segment_count(L)
    wav = clips(B, L)
    ws = torch.empty(ctx.workspace_bytes(B, L, _ffi.MODE_LOGITS), dtype=torch.uint8, device="cuda")
    o0, o1 = torch.zeros((B, S, 527), device="cuda"), torch.zeros((B, S, 527), device="cuda")
    clip = torch.zeros((B, 527), device="cuda")
    st = _ffi.stream_ptr(wav.device)
    ARG, SHAPE, WS = -1, -4, -5

    def fwd(pool=3, what=_ffi.SEG_OUTPUT, wav_=wav, out0=o0, out1=o1, L_=L, nbytes=None):
        return lib.acx_forward_segments(ctx.handle, _ffi.ptr(wav_), B, L_, pool, what, _ffi.ptr(out0), _ffi.ptr(out1), _ffi.ptr(clip),
                                        _ffi.ptr(ws), ws.numel() if nbytes is None else nbytes, st)

    def failed(rc, code):
        return rc == code and len(lib.acx_last_error()) > 0

    for pool in (0, 2, 32, 33, -3):
        assert failed(fwd(pool=pool), ARG), pool
    assert failed(fwd(what=2), ARG)
    assert failed(fwd(wav_=None), ARG) and failed(fwd(out0=None), ARG) and failed(fwd(out1=None), ARG)
    assert failed(fwd(L_=7359), SHAPE)
    assert failed(fwd(nbytes=1024), WS)
    lens = (ctypes.c_int64 * 2)(L, L)
    assert failed(lib.acx_forward_segments_varlen(ctx.handle, _ffi.ptr(wav), lens, 2, 4, 0, _ffi.ptr(o0), _ffi.ptr(o1), None,
                                                  _ffi.ptr(ws), ws.numel(), st), ARG)
    assert failed(lib.acx_forward_segments_windows(ctx.handle, _ffi.ptr(wav), lens, 2, 16000, 16000, 0, 2, 6, 0, _ffi.ptr(o0),
                                                   _ffi.ptr(o1), None, _ffi.ptr(ws), ws.numel(), st), ARG)
    x = torch.zeros((B, S, 7, 768), device="cuda")
    emb = torch.zeros((B, S, 768), device="cuda")
    assert failed(lib.acx_segment_head(ctx.handle, _ffi.ptr(x), B, 0, 3, _ffi.ptr(emb), None, None, st), SHAPE)
    assert failed(lib.acx_segment_head(ctx.handle, _ffi.ptr(x), B, S, 2, _ffi.ptr(emb), None, None, st), ARG)
    assert failed(lib.acx_segment_head(ctx.handle, _ffi.ptr(x), B, S, 3, None, None, None, st), ARG)
    assert failed(lib.acx_segment_head(ctx.handle, _ffi.ptr(x), B, S, 3, _ffi.ptr(emb), _ffi.ptr(o0), None, st), ARG)
    fr = torch.zeros((B, 101, 527), device="cuda")
    assert failed(lib.acx_segment_expand(_ffi.ptr(o1), B, S, 527, 0, _ffi.ptr(fr), st), SHAPE)
    assert failed(lib.acx_segment_expand(_ffi.ptr(o1), B, 0, 527, 101, _ffi.ptr(fr), st), SHAPE)
    assert failed(lib.acx_segment_expand(_ffi.ptr(o1), B, S, 0, 101, _ffi.ptr(fr), st), ARG)
    assert failed(lib.acx_segment_expand(None, B, S, 527, 101, _ffi.ptr(fr), st), ARG)
    short = (ctypes.c_int64 * 2)(L, 100)
    assert failed(lib.acx_segment_expand_varlen(_ffi.ptr(o1), short, 2, 527, _ffi.ptr(fr), st), SHAPE)
    assert failed(lib.acx_segment_timeline(_ffi.ptr(o1), 527, short, 2, 16000, 16000, 0, _ffi.ptr(fr), st), SHAPE)
    assert failed(lib.acx_segment_timeline(_ffi.ptr(o1), 527, lens, 2, 16000, 16000, 2, _ffi.ptr(fr), st), ARG)
    assert failed(lib.acx_segment_timeline(_ffi.ptr(o1), 527, lens, 2, 16000, 20000, 0, _ffi.ptr(fr), st), ARG)
    # the workspace queries: the sizes of the clip-level forwards (the embeddings live in the frontend's feature buffer)
    nb = ctypes.c_size_t()
    for what in ("segment", "segment_embeddings"):       # the acx_workspace_bytes_segments* calls
        assert ctx.workspace_bytes(B, L, what) == ctx.workspace_bytes(B, L, _ffi.MODE_LOGITS)
        assert ctx.workspace_bytes_varlen([L, 7360], what) == ctx.workspace_bytes_varlen([L, 7360], _ffi.MODE_LOGITS)
        assert ctx.workspace_bytes_windows(5, L, what) == ctx.workspace_bytes_windows(5, L, _ffi.MODE_LOGITS)
    assert failed(lib.acx_workspace_bytes_segments(ctx.handle, B, L, 2, ctypes.byref(nb)), ARG)
    assert failed(lib.acx_workspace_bytes_segments_varlen(ctx.handle, lens, 2, -1, ctypes.byref(nb)), ARG)
    assert failed(lib.acx_workspace_bytes_segments_windows(ctx.handle, 5, L, 7, ctypes.byref(nb)), ARG)
    assert failed(lib.acx_workspace_bytes_segments(ctx.handle, B, L, 0, None), ARG)
    assert failed(lib.acx_workspace_bytes_segments(ctx.handle, B, 7359, 0, ctypes.byref(nb)), SHAPE)
    n = ctypes.c_int()
    assert failed(lib.acx_segment_count(7359, ctypes.byref(n)), SHAPE) and failed(lib.acx_segment_count(L, None), ARG)
    torch.cuda.synchronize()
    assert float(o0.abs().max()) == 0.0 and float(fr.abs().max()) == 0.0          # nothing ran
    assert fwd() == 0                                                              # and the same call with good arguments does
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(o1, model.forward_segments(wav)["segmentwise_output"])
