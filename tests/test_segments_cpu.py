"""CPU: the host side of sound event detection (pytorch/segments.py, ConvNeXt.forward_segments' argument checks) and the tie
between the float64 recipe the GPU tests compare with (recipe64 below; tests/test_gpu_segments.py loads it from this file) and
the reference-made fixture tests/golden/g6_segments.npz (tests/golden/make_segment_golden.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

SR = 32000


def recipe64(frame, sd, pool, head=None):
    """The segment recipe in float64 torch: the decision-level head (mean over frequency, max + average pooling over time,
    LayerNorm, linear, sigmoid, max over segments) on a stage-3 map, with torch's own pooling and LayerNorm ops.
    frame: (B, 768, S, 7) frame embeddings (any float dtype); sd: state dict with norm.* and head_audioset.*; head: (w, b) to
    use instead of sd's.  Returns float64 {"emb" (B, S, 768), "logits", "probs" (B, S, N), "clip" (B, N)}."""
    x = frame.double().cpu()
    w, b = head if head is not None else (sd["head_audioset.weight"], sd["head_audioset.bias"])
    z = x.mean(dim=3)                                                                   # (B, 768, S)
    p = F.max_pool1d(z, pool, 1, pool // 2) + F.avg_pool1d(z, pool, 1, pool // 2)       # count_include_pad=True
    emb = F.layer_norm(p.transpose(1, 2), (768,), sd["norm.weight"].double().cpu(), sd["norm.bias"].double().cpu(), 1e-6)
    logits = emb @ w.double().cpu().T + b.double().cpu()
    probs = torch.sigmoid(logits)
    return {"emb": emb, "logits": logits, "probs": probs, "clip": probs.max(dim=1).values}


def test_segment_count_is_the_stage3_height():
    """S = acx_stage_hw(L, 3).H for every L.  The closed form is ((T + 4) // 4 + 1) // 8 = (T + 8) // 32 with T = L // 320 + 1:
    the stem pads four frames on each side.  The shorter form (L // 320 + 1) // 32 equals it exactly where T % 32 < 24 -- a
    10 s clip (T = 1001) among them -- and is one short elsewhere (a 7360-sample clip has T = 24 and one segment, not none), so
    it is asserted on those lengths and the stage height on all of them."""
    n_short_form = 0
    for L in range(_ffi.MIN_SAMPLES, 12 * SR + 1, 997):
        T = L // 320 + 1
        S = seg.segment_count(L)
        assert S == _ffi.stage_hw(L, 3)[0] == _ffi.segment_count(L) == (T + 8) // 32, L
        assert S >= 1
        if T % 32 < 24:
            assert S == (L // 320 + 1) // 32, L
            n_short_form += 1
    assert n_short_form > 200
    assert seg.segment_count(320000) == 31
    with pytest.raises(ValueError):
        seg.segment_count(_ffi.MIN_SAMPLES - 1)


def test_segment_edges():
    e = seg.segment_edges(320000)
    assert e.dtype == np.float64 and e.shape == (32,)
    assert np.array_equal(e[:31], np.arange(31) * 0.32) and e[31] == 10.0
    assert seg.segment_edges(7360)[-1] == 7360 / SR and seg.segment_edges(7360).shape == (2,)
    assert seg.segment_edges(320000, duration=9.99)[-1] == 9.99          # seconds of the audio before resampling


@pytest.mark.parametrize("L", [7360, 32000, 102080, 104960, 112000, 320000, 383999])
def test_frame_to_segment_repeats_32_and_pads_with_the_last(L):
    T, S = L // 320 + 1, seg.segment_count(L)
    got = seg.frame_to_segment(T, S)
    assert got.shape == (T,) and got.dtype == np.int64
    # every segment shown for 32 frames, then the last one to the clip's end (or the clip's frames end first)
    shown = np.repeat(np.arange(S), 32)
    shown = np.concatenate([shown, np.full(max(0, T - shown.size), S - 1)])[:T]
    assert np.array_equal(got, shown)
    assert got[0] == 0 and got[-1] == S - 1


def brute_cover(lengths, W, H):
    """Sample by sample: which (window, segment) pairs hold each row's midpoint."""
    rows, base = [], 0
    for r, L in enumerate(lengths):
        starts = win.window_starts([L], W, H)
        span = min(W, L)
        Sw = seg.segment_count(span)
        owner = np.full((len(starts), L), -1, dtype=np.int64)           # segment of sample x in window j, -1 outside
        for j, s in enumerate(starts):
            for x in range(s, s + span):
                owner[j, x] = min((x - s) // seg.SEGMENT_SAMPLES, Sw - 1)
        k = 0
        while k * seg.SEGMENT_SAMPLES < L:
            m = min(k * seg.SEGMENT_SAMPLES + seg.SEGMENT_SAMPLES // 2, L - 1)
            rows.append([(r, j, int(owner[j, m]), base + j * Sw + int(owner[j, m])) for j in range(len(starts)) if owner[j, m] >= 0])
            k += 1
        base += len(starts) * Sw
    return rows


@pytest.mark.parametrize("lengths,W,H", [
    ([40960, 81920], 20480, 20480),                 # even lengths, hop = window
    ([40960, 81920], 20480, 10240),                 # overlap, hop a multiple of the segment
    ([50001, 23456, 77777], 20480, 7000),           # ragged, hop not a multiple of 10240
    ([9000, 20480, 61440], 20480, 20480),           # L <= window: one clip with its own segments
    ([33333], 30000, 12345),
])
def test_segment_timeline_cover_against_brute_force(lengths, W, H):
    got = seg.segment_timeline_cover(lengths, W, H)
    assert got == brute_cover(lengths, W, H)
    assert len(got) == sum(-(-L // seg.SEGMENT_SAMPLES) for L in lengths)
    assert all(len(row) >= 1 for row in got)                                        # gap-free
    assert all(len({j for _, j, _, _ in row}) == len(row) for row in got)           # one segment per window at most


def test_decode_events_hysteresis_merge_duration_median():
    p = np.zeros((12, 3), dtype=np.float32)
    p[1:3, 0] = [0.6, 0.9]
    p[3, 0] = 0.4
    p[5, 0] = 0.45
    p[8:10, 1] = 0.7
    assert seg.decode_events(np.zeros((5, 2))) == []                                # empty result
    assert seg.decode_events(np.zeros((0, 2))) == []
    ev = seg.decode_events(p)
    assert [(c, round(a, 2), round(b, 2)) for c, a, b, _, _ in ev] == [(0, 0.32, 0.96), (1, 2.56, 3.2)]
    assert ev[0][3] == pytest.approx(0.9) and ev[0][4] == pytest.approx(0.75)
    # hysteresis: the run with p >= 0.4 around the peak; the 0.45 island never reaches the threshold
    ev = seg.decode_events(p, threshold=0.8, low=0.4)
    assert [(c, round(a, 2), round(b, 2)) for c, a, b, _, _ in ev] == [(0, 0.32, 1.28)]
    ev = seg.decode_events(p, threshold=0.45, low=0.4)
    assert [(round(a, 2), round(b, 2)) for c, a, b, _, _ in ev if c == 0] == [(0.32, 1.28), (1.6, 1.92)]
    # merge: the gap between them is 0.32 s
    ev = seg.decode_events(p, threshold=0.45, low=0.4, merge_gap=0.33)
    assert [(round(a, 2), round(b, 2)) for c, a, b, _, _ in ev if c == 0] == [(0.32, 1.92)]
    assert seg.decode_events(p, threshold=0.45, low=0.4, merge_gap=0.32) == seg.decode_events(p, threshold=0.45, low=0.4)
    # minimum duration: the one-step island goes
    ev = seg.decode_events(p, threshold=0.45, low=0.4, min_duration=0.5)
    assert [(c, round(a, 2), round(b, 2)) for c, a, b, _, _ in ev] == [(0, 0.32, 1.28), (1, 2.56, 3.2)]
    # median filter: a one-step spike disappears, a two-step event stays
    q = np.zeros((9, 1), dtype=np.float32)
    q[1, 0] = 0.9
    q[5:7, 0] = 0.9
    assert [(round(a, 2), round(b, 2)) for _, a, b, _, _ in seg.decode_events(q)] == [(0.32, 0.64), (1.6, 2.24)]
    assert [(round(a, 2), round(b, 2)) for _, a, b, _, _ in seg.decode_events(q, median=3)] == [(1.6, 2.24)]
    # labels, torch input, frame step, explicit edges; sorted by onset
    ev = seg.decode_events(torch.from_numpy(p), labels=["dog", "cat", "car"], step=0.01)
    assert [(c, round(a, 4)) for c, a, _, _, _ in ev] == [("dog", 0.01), ("cat", 0.08)]
    edges = np.arange(13) * 0.32
    edges[-1] = 3.7
    assert seg.decode_events(p, step=edges)[:2] == seg.decode_events(p)[:2]
    r = np.zeros((12, 1), dtype=np.float32)
    r[10:, 0] = 0.8
    assert seg.decode_events(r, step=edges)[0][2] == 3.7                            # the last segment reaches to the clip's end


def test_decode_events_value_errors():
    p = np.zeros((4, 2))
    for kw in ({"median": 2}, {"median": 0}, {"low": 0.9}, {"min_duration": -1.0}, {"merge_gap": -0.1}, {"step": 0.0},
               {"labels": ["a"]}, {"step": [0.0, 1.0]}):
        with pytest.raises(ValueError):
            seg.decode_events(p, **kw)
    with pytest.raises(ValueError):
        seg.decode_events(np.zeros(4))


def test_value_errors_before_anything_touches_the_gpu():
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False).eval()
    x = torch.zeros(1, SR)
    for pool in (0, 2, 4, 33, -1, 3.0, True, None):
        with pytest.raises(ValueError, match="pool"):
            m.forward_segments(x, pool=pool)
        with pytest.raises(ValueError, match="pool"):
            m.forward_segment_embeddings(x, pool=pool)
        with pytest.raises(ValueError, match="pool"):
            m.forward_varlen([x[0]], what="segment", pool=pool)
        with pytest.raises(ValueError, match="pool"):
            m.forward_windows(x[0], window=0.5, what="segment_embeddings", pool=pool)
    with pytest.raises(ValueError, match="resolution"):
        m.forward_segments(x, resolution="clip")
    with pytest.raises(ValueError, match="what"):
        m.forward_varlen([x[0]], what="segments")
    with pytest.raises(ValueError, match="what"):
        m.forward_windows(x[0], what="segments")
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.forward_segments(x)
    with pytest.raises(ValueError, match="eval"):
        m.forward_segment_embeddings(x)
    with pytest.raises(ValueError, match="eval"):
        m.forward_varlen([x[0]], what="segment")
    for bad in ((5, 0), (0, 3)):
        with pytest.raises(ValueError):
            seg.frame_to_segment(*bad)
    with pytest.raises(ValueError):
        seg.segment_timeline_cover([40000], 20480, 30000)                           # hop > window


def test_recipe_restatement_reproduces_the_reference_fixture(golden_dir, synth_sd):
    """The float64 restatement the GPU tests compare with, applied to the reference's own frame embeddings of the demo clip,
    against what the reference's modules gave (g6_segments.npz): within 1e-5 (fp32 vs fp64 of this recipe: ~1e-6 on embeddings,
    ~2e-6 on logits)."""
    g1 = np.load(os.path.join(golden_dir, "g1_demo.npz"))
    g6 = np.load(os.path.join(golden_dir, "g6_segments.npz"))
    assert list(g6["pools"]) == [1, 3, 5] and g6["frame_classes"].shape == (16,)
    frame = torch.from_numpy(g1["frame"])
    T, S = g1["pcm16"].shape[0] // 320 + 1, frame.shape[2]
    assert S == seg.segment_count(g1["pcm16"].shape[0]) == 31
    f2s = seg.frame_to_segment(T, S)
    for pool in (1, 3, 5):
        r = recipe64(frame, synth_sd, pool)
        for key, name in (("emb", "emb"), ("logits", "logits"), ("probs", "probs"), ("clip", "clip")):
            want = torch.from_numpy(g6["%s_p%d" % (name, pool)]).double()
            assert tuple(want.shape) == tuple(r[key][0].shape)
            assert float((r[key][0] - want).abs().max()) <= 1e-5, (pool, key)
        fr = r["probs"][0][torch.from_numpy(f2s)][:, torch.from_numpy(g6["frame_classes"])]
        want = torch.from_numpy(g6["frame_p%d" % pool]).double()
        assert want.shape == (T, 16)
        assert float((fr - want).abs().max()) <= 1e-5, pool
    assert not np.array_equal(g6["emb_p1"], g6["emb_p3"])
