"""GPU (`-m gpu`): every forward entry point of the C ABI inside guards (tests/forward_guard.py), in a workspace of exactly the
promised bytes that starts as a poison -- once as 0xFF bytes, once as 0x7F bytes.

tests/test_forward_plan_cpu.py shows on the CPU that the plan of every shape holds its tenants; here the kernels run in such plans at
the smallest shapes at which a carve-up can go wrong: 7360 samples (T = 24, heights 8 / 4 / 2 / 1, one segment) and the lengths with
an odd height at stage 0, 1 and 2 (17 000, 16 000, 23 000; test_gpu_varlen.py asserts that), batches of 1, of 3 and of 17 (two
sub-batches, 9 + 8), 25 and 33 clips under a 3- and 4-way split.  Each call must leave every canary intact, write every output
element with a finite value, leave its input alone, give the same bits under both poisons, the bits of the host wrapper for the
same batch, and for one clip the bits of the wrapper's forward of that clip alone.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import forward_guard as fg
from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import augment as A
from audioset_convnext_inf_amd.pytorch import segments as _seg
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny, varlen_frame_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["fp32", "fp32_split", "bf16", "bf16a"]
FRONTENDS = ["auto", "dense"]
MODES = ("logits", "scene", "frame")
SEGS = ("segment", "segment_embeddings")
ODD = (17000, 16000, 23000)          # an odd height at stage 0, 1, 2
POOL = 3


def make_model(sd, precision, frontend="auto", classes=527):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    state = sd
    if classes != 527:
        g = torch.Generator().manual_seed(classes)
        state = dict(sd)
        state["head_audioset.weight"] = torch.randn(classes, 768, generator=g) * 0.05
        state["head_audioset.bias"] = torch.randn(classes, generator=g) * 0.1
        m.head_audioset = nn.Linear(768, classes)
    m.load_state_dict(state)
    return m.to(DEV).eval().set_precision(precision).set_frontend(frontend)


@pytest.fixture(scope="module")
def models(synth_sd):
    cache = {}

    def get(precision, frontend="auto", classes=527):
        key = (precision, frontend, classes)
        if key not in cache:
            cache[key] = make_model(synth_sd, precision, frontend, classes)
        return cache[key]
    return get


def set_head_path(v):
    if v is None:
        os.environ.pop("ACX_HEAD_PATH", None)
    else:
        os.environ["ACX_HEAD_PATH"] = str(v)
    _ffi.check(_ffi.lib().acx_tuning_refresh())


@pytest.fixture
def head_path():
    yield set_head_path
    set_head_path(None)


def shapes_of(model, kind, lead, L, clips=None):
    ctx = model.native_context(torch.device(DEV))
    return [None if t is None else tuple(t.shape) for t in model._outputs(kind, lead, ctx.classes, L, torch.device(DEV), clips=clips)]


def compare(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, k)
        assert g is None or fg.same_bits(g, w), (what, "output %d differs from the wrapper's" % k)


def stream():
    return _ffi.stream_ptr(torch.device(DEV))


# ---- the entry points: each runs the raw call inside guards, then holds it to the wrapper and to one clip alone ---------------------
def run_uniform(model, x, kind, alone=0):
    """acx_forward (the three modes) and acx_forward_segments (the two kinds)."""
    ctx, (B, L), seg = model.native_context(x.device), x.shape, _ffi.SEG_WHAT.get(kind)
    need = ctx.workspace_bytes(B, L, kind)

    def call(ws, ins, outs):
        if seg is None:
            return _ffi.lib().acx_forward(ctx.handle, _ffi.ptr(ins[0]), B, L, _ffi.MODES[kind], _ffi.ptr(outs[0]), _ffi.ptr(outs[1]),
                                          _ffi.ptr(ws), ws.numel(), stream())
        return _ffi.lib().acx_forward_segments(ctx.handle, _ffi.ptr(ins[0]), B, L, POOL, seg, _ffi.ptr(outs[0]), _ffi.ptr(outs[1]),
                                               _ffi.ptr(outs[2]), _ffi.ptr(ws), ws.numel(), stream())
    got = fg.run_guarded(need, [x], shapes_of(model, kind, (B,), L), call)
    compare(got, model._run(x, kind, POOL), ("uniform", kind, B, L))
    one = model._run(x[alone:alone + 1], kind, POOL)
    compare([None if g is None else g[alone:alone + 1] for g in got], one, ("uniform alone", kind, B, L))
    return got


def logmel(model, x):
    B, L = x.shape
    ctx = model.native_context(x.device)
    feat = torch.empty((B, _ffi.num_frames(L), 224), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.lib().acx_logmel_bn0(ctx.handle, _ffi.ptr(x), B, L, _ffi.ptr(feat), 1, stream()))
    return feat


def run_features(model, x, kind, alone=0):
    ctx, (B, L) = model.native_context(x.device), x.shape
    feat = logmel(model, x)
    need = ctx.workspace_bytes(B, L, kind)

    def call(ws, ins, outs):
        return _ffi.lib().acx_forward_features(ctx.handle, _ffi.ptr(ins[0]), B, L, _ffi.MODES[kind], _ffi.ptr(outs[0]), _ffi.ptr(outs[1]),
                                               _ffi.ptr(ws), ws.numel(), stream())
    got = fg.run_guarded(need, [feat], shapes_of(model, kind, (B,), L)[:2], call)
    compare(got, model._run(x, kind)[:2], ("features", kind, B, L))
    compare([None if g is None else g[alone:alone + 1] for g in got], model._run(x[alone:alone + 1], kind)[:2], ("features alone", kind, B, L))


def run_varlen(model, clips, kind, alone=0):
    """acx_forward_varlen (modes) and acx_forward_segments_varlen (kinds)."""
    lengths = [int(c.numel()) for c in clips]
    packed = torch.cat(clips)
    ctx, B, seg = model.native_context(packed.device), len(clips), _ffi.SEG_WHAT.get(kind)
    need = ctx.workspace_bytes_varlen(lengths, kind)
    lens = (ctypes.c_int64 * B)(*lengths)
    if kind == "frame":
        offs = varlen_frame_layout(lengths)
    elif seg is not None:
        offs = [0] + list(np.cumsum([_seg.segment_count(n) for n in lengths]))
    else:
        offs = list(range(B + 1))
    shapes = shapes_of(model, kind, (offs[-1],), None, clips=B)

    def call(ws, ins, outs):
        if seg is None:
            return _ffi.lib().acx_forward_varlen(ctx.handle, _ffi.ptr(ins[0]), lens, B, _ffi.MODES[kind], _ffi.ptr(outs[0]),
                                                 _ffi.ptr(outs[1]), _ffi.ptr(ws), ws.numel(), stream())
        return _ffi.lib().acx_forward_segments_varlen(ctx.handle, _ffi.ptr(ins[0]), lens, B, POOL, seg, _ffi.ptr(outs[0]),
                                                      _ffi.ptr(outs[1]), _ffi.ptr(outs[2]), _ffi.ptr(ws), ws.numel(), stream())
    got = fg.run_guarded(need, [packed], shapes, call)
    compare(got, model._run_varlen(packed, lengths, kind, POOL), ("varlen", kind, lengths))
    # one clip alone, through the UNIFORM forward: its rows of the packed outputs
    one = model._run(clips[alone][None], kind, POOL)
    lo, hi = int(offs[alone]), int(offs[alone + 1])
    for k in (0, 1):
        if got[k] is not None:
            assert fg.same_bits(got[k][lo:hi].reshape(-1), one[k].reshape(-1)), ("varlen alone", kind, lengths, k)
    if got[2] is not None:
        assert fg.same_bits(got[2][alone], one[2][0]), ("varlen alone, clip maxima", kind, lengths)


def window_case(W, hop, counts):
    """Recordings whose window counts are `counts`; the last one ends with a window that ends exactly at its (and the buffer's)
    last sample, the others with a window pulled back to their end."""
    lengths = [W + (n - 2) * hop + hop // 3 if n > 1 else W for n in counts[:-1]] + [W + (counts[-1] - 1) * hop]
    assert [_ffi.window_count([n], W, hop) for n in lengths] == list(counts), lengths
    return lengths


def run_windows(model, W, hop, counts, kind, seed, alone=1):
    """acx_forward_windows (logits) and acx_forward_segments_windows (kinds).  W is no multiple of hop."""
    assert W % hop != 0
    lengths = window_case(W, hop, counts)
    packed = torch.cat([synth.synth_waveforms(1, n, seed=seed + i)[0] for i, n in enumerate(lengths)]).to(DEV)
    ctx, n, seg = model.native_context(packed.device), sum(counts), _ffi.SEG_WHAT.get(kind)
    need = ctx.workspace_bytes_windows(n, W, kind)
    lens = (ctypes.c_int64 * len(lengths))(*lengths)

    def call(ws, ins, outs):
        if seg is None:
            return _ffi.lib().acx_forward_windows(ctx.handle, _ffi.ptr(ins[0]), lens, len(lengths), W, hop, 0, n, _ffi.MODES[kind],
                                                  _ffi.ptr(outs[0]), _ffi.ptr(outs[1]), _ffi.ptr(ws), ws.numel(), stream())
        return _ffi.lib().acx_forward_segments_windows(ctx.handle, _ffi.ptr(ins[0]), lens, len(lengths), W, hop, 0, n, POOL, seg,
                                                       _ffi.ptr(outs[0]), _ffi.ptr(outs[1]), _ffi.ptr(outs[2]), _ffi.ptr(ws), ws.numel(),
                                                       stream())
    got = fg.run_guarded(need, [packed], shapes_of(model, kind, (n,), W), call)
    compare(got, model._run_windows(packed, lengths, W, hop, kind, n, POOL), ("windows", kind, W, hop, counts))
    # the last window of all -- the one that ends at the buffer's end -- and window `alone`, each as a clip of its own
    for g, start in ((n - 1, sum(lengths) - W), (alone, min(alone * hop, lengths[0] - W))):
        one = model._run(packed[start:start + W][None], kind, POOL)
        compare([None if t is None else t[g:g + 1] for t in got], one, ("window alone", kind, W, hop, g))


def run_augmented(model, x, seed, row=1):
    """acx_forward_augmented with a waveform plan, stripes and lambdas: 2 B clips in, B rows out; `row`: the output row held to the
    wrapper's forward of its two clips alone."""
    ctx, (B, L) = model.native_context(x.device), x.shape
    T = _ffi.num_frames(L)
    policy = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=1.0, time_width=min(40, T // 3), freq_width=28)
    plan = A.draw_plan(policy, B, L, torch.Generator().manual_seed(seed))
    lam = A.mixup_lambdas(B, 0.5, seed=seed)
    dplan = plan.to(x.device)
    lam_d = torch.from_numpy(np.asarray(lam, dtype=np.float32)).to(DEV)
    assert dplan.wave_dev is not None and dplan.spec_dev is not None
    need = ctx.workspace_bytes_augmented(B, L, True, True, "logits")

    def call(ws, ins, outs):
        return _ffi.lib().acx_forward_augmented(ctx.handle, _ffi.ptr(ins[0]), B, L, _ffi.ptr(ins[1]), _ffi.ptr(ins[2]), _ffi.ptr(ins[3]),
                                                _ffi.MODE_LOGITS, _ffi.ptr(outs[0]), _ffi.ptr(outs[1]), _ffi.ptr(ws), ws.numel(),
                                                stream())
    got = fg.run_guarded(need, [x, dplan.wave_dev, dplan.spec_dev, lam_d], [(B // 2, ctx.classes)] * 2, call)
    out = model.forward_augmented(x, plan=plan, mixup_lambda=lam)
    compare(got, [out["clipwise_logits"], out["clipwise_output"]], ("augmented", B, L))
    lo = 2 * row                                                         # clips 2 row and 2 row + 1 mix into row `row`
    pair = A.AugmentPlan(2, L, plan.wave[lo:lo + 2], plan.spec[lo:lo + 2])
    one = model.forward_augmented(x[lo:lo + 2], plan=pair, mixup_lambda=lam[lo:lo + 2])
    compare([g[row:row + 1] for g in got], [one["clipwise_logits"], one["clipwise_output"]], ("augmented alone", B, L))


def mixed_clips(B, seed):
    """The four lengths mixed, two equal clips side by side."""
    order = [7360, 23000, 23000, 17000, 16000, 7360, 16000, 17000]
    lengths = [order[i % len(order)] for i in range(B)]
    return [synth.synth_waveforms(1, n, seed=seed + i)[0].to(DEV) for i, n in enumerate(lengths)]


def profiled_poolhead_launches(model, x):
    """How many launches of the pool / head class one logits forward of x queues: 1 = the fused head, 2 = pooling into scene rows +
    the class-tiled head (the runtime's own choice, read from its per-kernel profile)."""
    ctx = model.native_context(x.device)
    ctx.profile(True)
    try:
        model._run(x, "logits")
        torch.cuda.synchronize()
        return ctx.profile_read()["poolhead"][1]
    finally:
        ctx.profile(False)


# ---- every entry point, every arithmetic, both frontends, at the small and at one odd-height shape ---------------------------------
@pytest.mark.parametrize("frontend", FRONTENDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_entry_point_single_clip(models, precision, frontend, head_path):
    """B = 1: the smallest plan there is at L = 7360 -- where the bf16 MLP arrays, the two-GEMM hidden activation and statistics, the
    segment embeddings and the scene rows are tightest -- and one clip of an odd-height length; one window, one packed clip, two
    clips mixed into one row.  The logits forwards run on both head paths: the tiled head's scene rows are a tenant of `feat`."""
    model = models(precision, frontend)
    odd = ODD[(PRECISIONS.index(precision) + 2 * FRONTENDS.index(frontend)) % 3]
    for L in (7360, odd):
        x = synth.synth_waveforms(1, L, seed=141 + L).to(DEV)
        assert model.native_context(x.device).sub_batches(1) == 1
        for kind in MODES + SEGS:
            run_uniform(model, x, kind)
            run_varlen(model, [x[0]], kind)
        for kind in MODES:
            run_features(model, x, kind)
        for kind in ("logits",) + SEGS:
            run_windows(model, L, 3000 if L == 7360 else 5000, (1,), kind, seed=151, alone=0)
        run_augmented(model, synth.synth_waveforms(2, L, seed=161).to(DEV), seed=7, row=0)
        head_path(2)
        assert profiled_poolhead_launches(model, x) == 2
        run_uniform(model, x, "logits")
        run_varlen(model, [x[0]], "logits")
        run_features(model, x, "logits")
        run_windows(model, L, 3000 if L == 7360 else 5000, (1,), "logits", seed=171, alone=0)
        head_path(None)
        assert profiled_poolhead_launches(model, x) == 1



@pytest.mark.parametrize("frontend", FRONTENDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_entry_point_smallest_shape(models, precision, frontend):
    """L = 7360 (T = 24, heights 8 / 4 / 2 / 1, one segment), 3 clips: the smallest feat and block scratch there is."""
    model = models(precision, frontend)
    L, B = 7360, 3
    x = synth.synth_waveforms(B, L, seed=11).to(DEV)
    for kind in MODES + SEGS:
        run_uniform(model, x, kind, alone=1)
        run_varlen(model, list(x), kind, alone=2)
    for kind in MODES:
        run_features(model, x, kind, alone=1)
    for kind in ("logits",) + SEGS:
        run_windows(model, L, 3000, (2, 1), kind, seed=21)
    run_augmented(model, synth.synth_waveforms(2 * B, L, seed=31).to(DEV), seed=5)


@pytest.mark.parametrize("frontend", FRONTENDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_entry_point_odd_heights_two_sub_batches(models, precision, frontend):
    """17 clips (9 + 8 on two streams) of a length with an odd stage height -- which length depends on the case, so that every one
    of the three runs in every arithmetic or frontend -- and the mixed variable-length batch of 17."""
    model = models(precision, frontend)
    B = 17
    L = ODD[(PRECISIONS.index(precision) + FRONTENDS.index(frontend)) % 3]
    assert model.native_context(torch.device(DEV)).sub_batches(B) == 2
    x = synth.synth_waveforms(B, L, seed=41).to(DEV)
    clips = mixed_clips(B, seed=51)
    for kind in MODES + SEGS:
        run_uniform(model, x, kind, alone=9)            # (the first clip of the second sub-batch)
        run_varlen(model, clips, kind, alone=2)         # (the second of two equal clips)
    for kind in MODES:
        run_features(model, x, kind, alone=16)
    for kind in ("logits",) + SEGS:
        run_windows(model, L, 5000, (9, 1, 7), kind, seed=61, alone=8)
    run_augmented(model, synth.synth_waveforms(2 * B, L, seed=71).to(DEV), seed=6)


# ---- the other ways a batch can run ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ways,B", [(3, 25), (4, 33)])
@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_three_and_four_way_split(synth_sd, precision, ways, B, monkeypatch):
    """ACX_SPLIT_WAYS is read at acx_create: a fresh module is a fresh context.  The promise covers every number of ways."""
    monkeypatch.setenv("ACX_SPLIT_WAYS", str(ways))
    L = 7360
    x = synth.synth_waveforms(B, L, seed=81).to(DEV)
    for frontend in FRONTENDS:
        model = make_model(synth_sd, precision, frontend)
        assert model.native_context(x.device).sub_batches(B) == ways
        for kind in ("logits", "frame", "segment"):
            run_uniform(model, x, kind, alone=B - 1)
        run_features(model, x, "scene", alone=B // 2)
        run_windows(model, L, 3000, (B - 1, 1), "logits", seed=91, alone=B - 3)
        del model


@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_unsplit_plan_in_the_split_promise(synth_sd, precision, monkeypatch):
    """ACX_SPLIT_STREAMS=0: 17 clips run as one plan in a workspace whose promise is the two-way split's."""
    monkeypatch.setenv("ACX_SPLIT_STREAMS", "0")
    model = make_model(synth_sd, precision, "dense")
    x = synth.synth_waveforms(17, 16000, seed=101).to(DEV)
    assert model.native_context(x.device).sub_batches(17) == 1
    for kind in ("logits", "segment"):
        run_uniform(model, x, kind, alone=16)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_both_head_paths_at_527_classes(models, precision, path, head_path):
    """ACX_HEAD_PATH = 1: the fused head; 2: the class-tiled one, whose scene rows are a tenant of `feat`."""
    model = models(precision, "auto")
    head_path(path)
    # the path is in effect: the plan of the tiled head lists the scene rows, and the runtime queues two launches for it, not one
    kinds = [_ffi.PLAN_TENANTS[t.kind] for p in [_ffi.forward_plan(precision, "uniform", "logits", 3, 7360, head_path=path)]
             for t in p.subs[0].tenants[:p.subs[0].n_tenants]]
    assert ("scene_rows" in kinds) == (path == 2)
    assert profiled_poolhead_launches(model, synth.synth_waveforms(3, 7360, seed=110).to(DEV)) == path
    for B, L in ((3, 7360), (17, 23000)):
        x = synth.synth_waveforms(B, L, seed=111).to(DEV)
        run_uniform(model, x, "logits", alone=B - 1)
        run_varlen(model, mixed_clips(B, seed=121), "logits", alone=1)


@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_wide_head(models, precision):
    """4096 classes (class-tiled by default) in logits mode and through the segment head."""
    model = models(precision, "auto", 4096)
    for B, L in ((3, 7360), (17, 17000)):
        x = synth.synth_waveforms(B, L, seed=131).to(DEV)
        run_uniform(model, x, "logits", alone=1)
        run_uniform(model, x, "segment", alone=1)
