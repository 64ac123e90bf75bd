"""GPU (`-m gpu`): classifier heads of any size (ConvNeXt(num_classes=N), a replaced head_audioset, acx_num_classes).

The contract (include/acx.h, acx_set_weight): a class's logit depends only on the clip's scene embedding and that head row --
not on N, on the row's position in the head, on the batch or on which of the two head kernels (the fused pool_head_kernel, the
class-tiled head_tiled_kernel) computed it -- bit for bit; every forward path writes N-wide rows."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import evaluate as ev
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract
from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics

pytestmark = pytest.mark.gpu
SR = 32000
E2E_TOL = 1e-3           # tests/test_gpu_parity.py
PRECISIONS = ["fp32", "fp32_split", "bf16", "bf16a"]
WIDE = 4096              # above the class-tiled threshold (kHeadTiledMin)


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


def clips(B, L=SR, seed=11):
    return synth.synth_waveforms(B, L, seed=seed).cuda()


def set_head_path(v):
    """ACX_HEAD_PATH: 1 forces the fused head, 2 the class-tiled one, None = by N (re-read through acx_tuning_refresh)."""
    if v is None:
        os.environ.pop("ACX_HEAD_PATH", None)
    else:
        os.environ["ACX_HEAD_PATH"] = str(v)
    _ffi.check(_ffi.lib().acx_tuning_refresh())


@pytest.fixture
def head_path():
    yield set_head_path
    set_head_path(None)


# ---- 1. head independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_independence(sd, precision):
    wav = clips(3)
    m = make_model(sd, precision)
    with torch.no_grad():
        scene527 = m.forward_scene_embeddings(wav)
    for i, n in enumerate([1, 10, 50, 200, 4096, 16384]):
        w, b = head(n, seed=100 + i)
        m.head_audioset = nn.Linear(768, n).cuda()
        m.load_state_dict(with_head(sd, w, b))
        with torch.no_grad():
            scene = m.forward_scene_embeddings(wav)
            out = m(wav)
        assert torch.equal(scene, scene527), (precision, n)
        assert out["clipwise_logits"].shape == (3, n) and out["clipwise_output"].shape == (3, n)
        e = scene.double().cpu()
        w64, b64 = w.double(), b.double()
        ref = e @ w64.T + b64
        bound = 768 * 2.0 ** -24 * (e.abs() @ w64.abs().T) + 2.0 ** -24 * b64.abs()
        err = (out["clipwise_logits"].double().cpu() - ref).abs()
        assert bool((err <= bound).all()), (precision, n, float((err - bound).max()))
        p_err = (out["clipwise_output"].double().cpu() - torch.sigmoid(out["clipwise_logits"].double().cpu())).abs().max()
        assert float(p_err) <= 1e-6, (precision, n, float(p_err))


# ---- 2. row position and tiling ---------------------------------------------------------------------------------------------
def embedded_head(sd, n=WIDE, at=1000):
    """An n-row head whose rows [at, at + 527) are the AudioSet head of sd."""
    w, b = head(n, seed=7)
    w[at:at + 527], b[at:at + 527] = sd["head_audioset.weight"], sd["head_audioset.bias"]
    return with_head(sd, w, b)


def test_row_position_and_tiling_keep_bits(sd):
    m527, mw = make_model(sd), make_model(embedded_head(sd))
    for B in (1, 3, 17, 64):
        wav = clips(B, seed=20 + B)
        with torch.no_grad():
            a, z = m527(wav), mw(wav)
        for k in ("clipwise_logits", "clipwise_output"):
            assert z[k].shape == (B, WIDE)
            assert torch.equal(z[k][:, 1000:1527], a[k]), (B, k)


def test_both_head_kernels_give_the_same_bits(sd, head_path):
    wav = clips(19, seed=3)
    for state in (with_head(sd, *head(50, seed=5)), embedded_head(sd)):
        m = make_model(state)
        got = []
        for path in (1, 2):
            head_path(path)
            with torch.no_grad():
                got.append(m(wav))
                got.append({"v": m.forward_varlen([wav[i, :SR - 97 * i] for i in range(19)])["clipwise_logits"]})
        for k in got[0]:
            assert torch.equal(got[0][k], got[2][k]), k
        assert torch.equal(got[1]["v"], got[3]["v"])


# ---- 3. end to end against the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp32_split"])
def test_oracle_parity_n50(sd, precision):
    from oracle import ref_cpu
    state = with_head(sd, *head(50, seed=9))
    m = make_model(state, precision)
    wav = synth.synth_waveforms(2, SR, seed=5)
    with torch.no_grad():
        out = m(wav.cuda())
    ref = ref_cpu.forward(state, wav)
    for k in ("clipwise_logits", "clipwise_output"):
        assert out[k].shape == ref[k].shape == (2, 50)
        d = float((out[k].cpu() - ref[k]).abs().max())
        assert d < E2E_TOL, (precision, k, d)


# ---- 4. every path ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[50, WIDE])
def model_n(request, sd):
    n = request.param
    return n, make_model(with_head(sd, *head(n, seed=n)))


def test_varlen_rows_equal_alone(model_n):
    n, m = model_n
    lens = [SR, 7360, 45001, 12345]
    cl = [synth.synth_waveforms(1, L, seed=40 + i)[0].cuda() for i, L in enumerate(lens)]
    with torch.no_grad():
        v = m.forward_varlen(cl)
        for i, c in enumerate(cl):
            one = m(c[None])
            for k in ("clipwise_logits", "clipwise_output"):
                assert v[k].shape == (len(lens), n)
                assert torch.equal(v[k][i], one[k][0]), (n, i, k)


def timeline_ref(probs, L, W, H, reduce):
    starts = win.window_starts([L], W, H)
    rows = []
    for mid in win.timeline_steps([L], W, H):
        js = [j for j, s in enumerate(starts) if s <= mid < s + W]
        if reduce == "max":
            rows.append(probs[js].max(dim=0).values)
        else:
            acc = torch.zeros(probs.shape[1], dtype=torch.float32, device=probs.device)
            for j in js:
                acc = acc + probs[j]
            rows.append(acc / torch.tensor(float(len(js)), dtype=torch.float32, device=probs.device))
    return torch.stack(rows)


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_windows_rows_and_timeline(model_n, reduce):
    n, m = model_n
    W, H = SR, 12000
    recs = [synth.synth_waveforms(1, L, seed=60 + i)[0].cuda() for i, L in enumerate([3 * SR + 777, 50000])]
    with torch.no_grad():
        out = m.forward_windows(recs, window=W / SR, hop=H / SR, timeline=reduce)
        for r, rec in zip(out, recs):
            L = rec.numel()
            starts = win.window_starts([L], W, H)
            assert r["clipwise_logits"].shape == (len(starts), n)
            cut = torch.stack([rec[s:s + W] for s in starts])
            ref = m(cut)
            assert torch.equal(r["clipwise_logits"], ref["clipwise_logits"])
            assert torch.equal(r["clipwise_output"], ref["clipwise_output"])
            assert r["timeline"].shape == (-(-L // H), n)
            assert torch.equal(r["timeline"], timeline_ref(r["clipwise_output"], L, W, H, reduce))


def test_stream_equals_forward_windows(model_n):
    n, m = model_n
    W, H = SR, 16000
    recs = [synth.synth_waveforms(1, L, seed=80 + i)[0].cuda() for i, L in enumerate([3 * SR + 5, 2 * SR + 1234])]
    with torch.no_grad():
        ref = m.forward_windows(recs, window=W / SR, hop=H / SR)
        for chunk in (4099, 31991):
            st = m.stream(slots=2, window=W / SR, hop=H / SR, max_push=1.0)
            res = []
            pos = 0
            while pos < max(r.numel() for r in recs):
                res.append(st.push({i: r[pos:pos + chunk] for i, r in enumerate(recs) if pos < r.numel()}))
                pos += chunk
            res.append(st.close())
            for i, r in enumerate(ref):
                rows = torch.cat([d["clipwise_logits"][d["slot"] == i] for d in res])
                probs = torch.cat([d["clipwise_output"][d["slot"] == i] for d in res])
                tl = torch.cat([d["timeline"][d["timeline_slot"] == i] for d in res])
                assert rows.shape[1] == n and tl.shape[1] == n
                assert torch.equal(rows, r["clipwise_logits"]), (n, chunk, i)
                assert torch.equal(probs, r["clipwise_output"])
                assert torch.equal(tl, r["timeline"])
            st.close_handle()


def test_extract_equals_forward(model_n):
    n, m = model_n
    lens = [SR, 20000, SR, 9000]
    waves = [synth.synth_waveforms(1, L, seed=90 + i)[0] for i, L in enumerate(lens)]
    with torch.no_grad():
        ref = [m(w[None].cuda())["clipwise_logits"][0].cpu() for w in waves]
        for pack in (False, True):
            got = extract(m, waves, what="logits", pack=pack)
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                assert g.shape == (n,) and torch.equal(g, r), (n, pack)


def test_metrics_on_n_columns(model_n):
    n, m = model_n
    from audioset_convnext_inf_amd.utils.data_generator import ClipShard, evaluate_batches
    rs = np.random.RandomState(7)
    wav = (rs.standard_normal((24, 16000)) * 0.1 * 32767).astype(np.int16)
    tgt = rs.uniform(size=(24, n)) < 0.3
    tgt[0], tgt[1] = True, False
    shard = ClipShard(wav, tgt)
    a = ev.Evaluator(m, metrics="gpu").evaluate(evaluate_batches(shard, batch_size=8))
    b = ev.Evaluator(m, metrics="sklearn").evaluate(evaluate_batches(shard, batch_size=8))
    for k in b:
        assert a[k].shape == (n,)
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-12)
    with torch.no_grad():
        probs = m(torch.from_numpy(wav[:8] / 32767.0).float().cuda())["clipwise_output"]
    t = torch.from_numpy(tgt[:8]).cuda()
    assert tagging_metrics(t, probs)["average_precision"].shape == (n,)


# ---- 5. C ABI -------------------------------------------------------------------------------------------------------------------
def set_weight(ctx, key, t):
    t = t.contiguous().float()
    shape = (ctypes.c_int64 * t.dim())(*t.shape)
    return _ffi.lib().acx_set_weight(ctx.handle, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())


def test_c_abi_num_classes_and_shape_errors(sd):
    lib = _ffi.lib()
    ctx = _ffi.Context(0)
    n = ctypes.c_int()
    assert lib.acx_num_classes(ctx.handle, ctypes.byref(n)) == -2            # ACX_ERR_STATE before finalize
    ctx.load_state_dict(with_head(sd, *head(50, seed=1)))
    assert ctx.num_classes() == 50
    w, b = head(51, seed=2)
    assert set_weight(ctx, "head_audioset.weight", w) == 0
    assert set_weight(ctx, "head_audioset.bias", b[:50]) == 0
    assert lib.acx_finalize(ctx.handle) == -4                                # ACX_ERR_SHAPE: rows disagree
    msg = lib.acx_last_error().decode()
    assert "head_audioset.weight" in msg and "head_audioset.bias" in msg
    for bad in (0, 32769):
        assert set_weight(ctx, "head_audioset.weight", torch.zeros(bad, 768)) == -4
        assert set_weight(ctx, "head_audioset.bias", torch.zeros(bad)) == -4
    assert set_weight(ctx, "head_audioset.weight", torch.zeros(50, 767)) == -4
    assert set_weight(ctx, "head_audioset.bias", b) == 0
    assert lib.acx_finalize(ctx.handle) == 0 and ctx.num_classes() == 51
    assert set_weight(ctx, "norm.weight", torch.zeros(50)) == -4              # every other key keeps its shape
    ctx.load_state_dict(sd)
    assert ctx.num_classes() == 527
    ctx.close()


def test_timeline_classes_527_equals_timeline():
    g = torch.Generator().manual_seed(4)
    lengths, W, H = [3 * SR + 11, 40000], SR, 9000
    nwin = _ffi.window_count(lengths, W, H)
    probs = torch.rand(nwin, 527, generator=g).cuda()
    rows = len(win.timeline_steps(lengths, W, H))
    lens = (ctypes.c_int64 * 2)(*lengths)
    for reduce in (0, 1):
        a = torch.full((rows, 527), float("nan"), device="cuda")
        b = torch.full((rows, 527), float("nan"), device="cuda")
        _ffi.check(_ffi.lib().acx_window_timeline(_ffi.ptr(probs), lens, 2, W, H, reduce, _ffi.ptr(a), None))
        _ffi.check(_ffi.lib().acx_window_timeline_classes(_ffi.ptr(probs), 527, lens, 2, W, H, reduce, _ffi.ptr(b), None))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
    out = torch.empty(rows, 10, device="cuda")
    for bad in (0, 32769):
        assert _ffi.lib().acx_window_timeline_classes(_ffi.ptr(probs), bad, lens, 2, W, H, 0, _ffi.ptr(out), None) == -1


def test_stream_handle_refuses_a_changed_class_count(sd):
    m = make_model(with_head(sd, *head(50, seed=1)))
    st = m.stream(slots=1, window=1.0, hop=0.5, max_push=1.0)
    assert st.classes == 50
    with torch.no_grad():
        d = st.push({0: clips(1, 2 * SR)[0]})
    assert d["clipwise_logits"].shape[1] == 50
    m.head_audioset = nn.Linear(768, 60).cuda()
    m.load_state_dict(with_head(sd, *head(60, seed=2)))
    with pytest.raises(_ffi.AcxError) as e:
        st.push({0: clips(1, SR)[0]})
    assert e.value.code == -2                                                 # ACX_ERR_STATE
    lib = _ffi.lib()
    rows, got = ctypes.c_int64(), ctypes.c_int64()
    ts, tk = (ctypes.c_int * 4)(), (ctypes.c_int64 * 4)()
    out = torch.empty(4, 60, device="cuda")
    assert lib.acx_stream_timeline(st._h, 0, 4, _ffi.ptr(out), ts, tk, ctypes.byref(got), None) == -2
    st.close_handle()


# ---- 6. head swap ---------------------------------------------------------------------------------------------------------------
def test_head_swap_and_back(sd):
    wav = clips(5, seed=31)
    fresh = make_model(sd)
    m = make_model(sd)
    m.head_audioset = nn.Linear(768, 50).cuda()
    m.load_state_dict(with_head(sd, *head(50, seed=8)))
    with torch.no_grad():
        out = m(wav)
    assert out["clipwise_logits"].shape == (5, 50) and out["clipwise_output"].shape == (5, 50)
    m.head_audioset = nn.Linear(768, 527).cuda()
    m.load_state_dict(sd)
    with torch.no_grad():
        a, b = m(wav), fresh(wav)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    m.head_audioset = nn.Linear(768, 50, bias=False).cuda()
    with pytest.raises(ValueError, match="head_audioset.bias"):
        m(wav)
