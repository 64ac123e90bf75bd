"""GPU (`-m gpu`): the augmented forwards (csrc/augment.hip, acx_forward_features, acx_forward_augmented,
ConvNeXt.forward_augmented, fit_head(augment=...)).

Correct means equal, bit for bit: the two kernels to their host definitions (pytorch/augment.py, themselves pinned to the
reference in test_augment_cpu.py), the forward from features to the forward from audio, the augmented forward to the staged
composition of its parts, and the augmented fit to the fit on the augmented rows."""
import ctypes

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import augment as A
from audioset_convnext_inf_amd.pytorch import finetune
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = (0.5, 0.9, 1.0, 1.1, 1.4999, 1.5)
FULL = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=1.0)


def make_model(sd, precision):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to(DEV).eval().set_precision(precision)


@pytest.fixture(scope="module")
def models(synth_sd):
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = make_model(synth_sd, precision)
        return cache[precision]
    return get


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def finite_bits(shape, seed):
    """float32 values over forty decades, both signs (finite: a product with a NaN would depend on payload rules)."""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(shape) * 10.0 ** rs.randint(-20, 18, shape)).astype(np.float32)


def stream():
    return _ffi.stream_ptr(torch.device(DEV))


# ---- acx_augment_wave -------------------------------------------------------------------------------------------------------
def wave_entries(L):
    """Every rate with its extreme offsets (crop start 0 and diff - 1, left padding 0 and `missing`), crossed with the rolls
    and the gains."""
    out = []
    for rate in RATES:
        n_out = A.stretched_length(L, 1.0 / rate)
        shifts = (0, n_out - L - 1) if n_out > L else ((0, n_out - L) if n_out < L else (0,))
        for shift in shifts:
            for roll in (0, 1, L - 1):
                for gain_db in (0, -5):
                    out.append(dict(rate=rate, shift=shift, roll=roll, gain_db=gain_db))
    return out


@pytest.mark.parametrize("L", [7360, 32000, 32001])
def test_wave_kernel_equals_its_host_definition(L):
    entries = wave_entries(L)
    assert len(entries) == 66
    for B in (1, 3, 65):
        x = finite_bits((B, L), 10 + B)
        xd = torch.from_numpy(x).to(DEV)
        # B = 65: one call holds 65 different plans; B = 1 and 3: a stride through the list that still visits every rate
        starts = [0, 1] if B == 65 else range(0, len(entries), 7 if B == 1 else 9)
        for s in starts:
            w = np.zeros(B, dtype=A.WAVE_DTYPE)
            for b in range(B):
                w[b] = A.wave_entry(L, **entries[(s + b) % len(entries)])
            plan = A.AugmentPlan(B, L, w, None).to(DEV)
            out = torch.full((B, L), float("nan"), device=DEV)
            _ffi.check(_ffi.lib().acx_augment_wave(_ffi.ptr(xd), B, L, _ffi.ptr(plan.wave_dev), _ffi.ptr(out), stream()))
            want = torch.from_numpy(A.augment_wave_host(x, plan))
            assert same_bits(out.cpu(), want), (B, L, s)
        assert same_bits(xd.cpu(), torch.from_numpy(x))


def test_wave_kernel_with_drawn_plans_and_an_unaligned_output():
    B, L = 5, 20803
    x = finite_bits((B, L), 3)
    plan = A.draw_plan(FULL, B, L, torch.Generator().manual_seed(1)).to(DEV)
    buf = torch.full((B * L + 3,), float("nan"), device=DEV)
    for off in (0, 1, 2, 3):                              # every alignment of the first row
        out = buf[off:off + B * L].view(B, L)
        _ffi.check(_ffi.lib().acx_augment_wave(_ffi.ptr(torch.from_numpy(x).to(DEV)), B, L, _ffi.ptr(plan.wave_dev),
                                               ctypes.c_void_p(out.data_ptr()), stream()))
        assert same_bits(out.cpu(), torch.from_numpy(A.augment_wave_host(x, plan))), off


# ---- acx_augment_spec -------------------------------------------------------------------------------------------------------
def stripe_plan(T, seed):
    """Eight clips: the hand-worked cases (length 0, bgn 0, ending at T, ending at bin 223, overlapping, none), a full house of
    widest stripes and a drawn one."""
    L = (T - 1) * 320
    s = np.zeros(8, dtype=A.SPEC_DTYPE)

    def put(b, t=(), f=()):
        for k, (bgn, n) in enumerate(t):
            s["t_bgn"][b, k], s["t_len"][b, k] = bgn, n
        for k, (bgn, n) in enumerate(f):
            s["f_bgn"][b, k], s["f_len"][b, k] = bgn, n
    put(0, [(5, 0)], [(7, 0)])
    put(1, [(0, 3)], [(0, 2)])
    put(2, [(T - 4, 4)])
    put(3, (), [(200, 24)])
    put(4, [(4, 6), (8, 5)], [(10, 20), (25, 27)])
    put(6, [(0, 63), (1, 63), (T - 63, 63), (T // 2 - 30, 63)], [(0, 27), (197, 27), (100, 27), (110, 27)])
    drawn = A.draw_plan(A.AugmentPolicy(time_stripes=4, freq_stripes=4), 1, L, torch.Generator().manual_seed(seed))
    s[7] = drawn.spec[0]
    return A.AugmentPlan(8, L, None, s)


@pytest.mark.parametrize("T", [65, 101, 1001])
def test_spec_kernel_in_place_writes_the_masked_elements_only(T):
    plan = stripe_plan(T, T).to(DEV)
    rs = np.random.RandomState(T)
    x = rs.randint(-2 ** 31, 2 ** 31, (8, T, 224), dtype=np.int64).astype(np.int32).view(np.float32)      # any bits, NaNs included
    feat = torch.from_numpy(x).to(DEV)
    _ffi.check(_ffi.lib().acx_augment_spec(_ffi.ptr(feat), 8, T, _ffi.ptr(plan.spec_dev), None, _ffi.ptr(feat), stream()))
    want = torch.from_numpy(A.augment_spec_host(x, plan))
    assert same_bits(feat.cpu(), want)
    assert same_bits(feat.cpu()[5], torch.from_numpy(x)[5])           # the clip without stripes keeps every bit


@pytest.mark.parametrize("T", [65, 101, 1001])
def test_spec_kernel_mixing_form(T):
    plan = stripe_plan(T, T + 1).to(DEV)
    x = finite_bits((8, T, 224), T)
    drawn = A.mixup_lambdas(2, 0.5, seed=T)
    lam = np.array([0.0, 1.0, 1.0, 0.0, 0.5, 0.5, drawn[0], drawn[1]])
    feat = torch.from_numpy(x).to(DEV)
    lam_d = torch.from_numpy(lam.astype(np.float32)).to(DEV)
    for p, pd in ((plan, plan.spec_dev), (None, None)):                # with each clip's own stripes, and the mix alone
        out = torch.full((4, T, 224), float("nan"), device=DEV)
        _ffi.check(_ffi.lib().acx_augment_spec(_ffi.ptr(feat), 8, T, _ffi.ptr(pd), _ffi.ptr(lam_d), _ffi.ptr(out), stream()))
        assert same_bits(out.cpu(), torch.from_numpy(A.augment_spec_host(x, p, lam)))
        assert same_bits(feat.cpu(), torch.from_numpy(x))              # the input map is untouched


# ---- acx_forward_features ---------------------------------------------------------------------------------------------------
def logmel(model, x):
    B, L = x.shape
    dev = x.device
    ctx = model.native_context(dev)
    feat = torch.empty((B, _ffi.num_frames(L), 224), dtype=torch.float32, device=dev)
    _ffi.check(_ffi.lib().acx_logmel_bn0(ctx.handle, _ffi.ptr(x), B, L, _ffi.ptr(feat), 1, _ffi.stream_ptr(dev)))
    return feat


def forward_features(model, feat, L, kind):
    B, dev = feat.shape[0], feat.device
    ctx = model.native_context(dev)
    ws = torch.empty(ctx.workspace_bytes(B, L, kind), dtype=torch.uint8, device=dev)
    out0, out1, _ = model._outputs(kind, (B,), ctx.classes, L, dev)
    _ffi.check(_ffi.lib().acx_forward_features(ctx.handle, _ffi.ptr(feat), B, L, _ffi.MODES[kind], _ffi.ptr(out0), _ffi.ptr(out1),
                                               _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
    return out0, out1


@pytest.mark.parametrize("precision", ["fp32_split", "fp32", "bf16", "bf16a"])
def test_forward_from_features_equals_the_forward_from_audio(models, precision):
    model = models(precision)
    assert model.native_context(torch.device(DEV)).sub_batches(64) > 1          # 64 clips take the split path
    for B, L in ((1, 32000), (5, 32000), (64, 32000), (5, 320000)):
        x = synth.synth_waveforms(B, L, seed=B).to(DEV)
        feat = logmel(model, x)
        keep = feat.clone()
        for kind in ("logits", "scene", "frame"):
            want0, want1, _ = model._run(x, kind)
            got0, got1 = forward_features(model, feat, L, kind)
            assert torch.equal(got0, want0), (precision, B, L, kind)
            assert kind != "logits" or torch.equal(got1, want1), (precision, B, L, kind)
        assert torch.equal(feat, keep)                                           # the caller's rows are read only


# ---- forward_augmented ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_identity_policy_equals_the_plain_forwards(models, precision):
    model = models(precision)
    for B in (4, 17):
        x = synth.synth_waveforms(B, 32000, seed=2).to(DEV)
        out = model.forward_augmented(x, policy=A.AugmentPolicy.identity())
        ref = model(x)
        assert torch.equal(out["clipwise_logits"], ref["clipwise_logits"]) and torch.equal(out["clipwise_output"], ref["clipwise_output"])
        assert out["plan"].wave is None and out["plan"].spec is None
        assert torch.equal(model.forward_augmented(x, policy=A.AugmentPolicy.identity(), what="scene")["scene"],
                           model.forward_scene_embeddings(x))
        assert torch.equal(model.forward_augmented(x, policy=A.AugmentPolicy.identity(), what="frame")["frame"],
                           model.forward_frame_embeddings(x))


@pytest.mark.parametrize("precision", ["fp32_split", "bf16a"])
def test_augmented_forward_equals_the_staged_composition(models, precision):
    model = models(precision)
    B, L = 4, 32000
    x = synth.synth_waveforms(B, L, seed=7)
    policy = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=1.0, time_width=40)
    plan = A.draw_plan(policy, B, L, torch.Generator().manual_seed(21))
    lam = A.mixup_lambdas(B, 0.5, seed=3)
    # the parts, one after the other: host gather, the library's frontend, host mask and mix, the forward from features
    wav = torch.from_numpy(A.augment_wave_host(x.numpy(), plan)).to(DEV)
    feat = logmel(model, wav)
    for lam_i, rows in ((lam, B // 2), (None, B)):
        staged = torch.from_numpy(A.augment_spec_host(feat.cpu().numpy(), plan, lam_i)).to(DEV)
        for kind in ("logits", "scene", "frame"):
            want0, want1 = forward_features(model, staged, L, kind)
            out = model.forward_augmented(x.to(DEV), plan=plan, mixup_lambda=lam_i, what=kind)
            got0 = out["clipwise_logits"] if kind == "logits" else out[kind]
            assert got0.shape[0] == rows and torch.equal(got0, want0), (precision, kind, rows)
            assert kind != "logits" or torch.equal(out["clipwise_output"], want1)
            assert out["plan"] is plan


def test_dense_frontend_takes_its_scratch_from_the_call(synth_sd):
    """The dense-DFT frontend's frames and spectrum for all B clips are carved from acx_forward_augmented's own workspace."""
    model = make_model(synth_sd, "fp32_split").set_frontend("dense")
    B, L = 6, 32000
    x = synth.synth_waveforms(B, L, seed=12).to(DEV)
    ctx = model.native_context(torch.device(DEV))
    assert ctx.frontend_info()["dense_dft"]
    assert ctx.workspace_bytes_augmented(B, L, True, True, "logits") >= ctx.workspace_bytes(B // 2, L, "logits") + B * 101 * (1024 + 1056) * 4
    out = model.forward_augmented(x, policy=A.AugmentPolicy.identity())
    assert torch.equal(out["clipwise_logits"], model(x)["clipwise_logits"])
    plan = A.draw_plan(A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), time_width=40), B, L, torch.Generator().manual_seed(2))
    lam = A.mixup_lambdas(B, 0.5)
    feat = logmel(model, torch.from_numpy(A.augment_wave_host(x.cpu().numpy(), plan)).to(DEV))
    staged = torch.from_numpy(A.augment_spec_host(feat.cpu().numpy(), plan, lam)).to(DEV)
    out = model.forward_augmented(x, plan=plan, mixup_lambda=lam)
    assert torch.equal(out["clipwise_logits"], forward_features(model, staged, L, "logits")[0])


def test_augmented_forward_is_capturable(models):
    """The plans live in device memory and the call neither allocates nor synchronises: captured into a hipGraph, the replay
    equals the eager call bit for bit."""
    model = models("fp32_split")
    B, L = 4, 32000
    dev = torch.device(DEV)
    x = synth.synth_waveforms(B, L, seed=3).to(DEV)
    plan = A.draw_plan(FULL, B, L, torch.Generator().manual_seed(4))
    lam = A.mixup_lambdas(B, 0.5)
    eager = model.forward_augmented(x, plan=plan, mixup_lambda=lam)["clipwise_logits"].clone()
    dplan = plan.to(dev)
    lam_d = torch.from_numpy(lam.astype(np.float32)).to(DEV)
    ctx = model.native_context(dev)
    ws = torch.empty(ctx.workspace_bytes_augmented(B, L, True, True, "logits"), dtype=torch.uint8, device=DEV)
    logits, probs = torch.zeros((B // 2, 527), device=DEV), torch.zeros((B // 2, 527), device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc = _ffi.lib().acx_forward_augmented(ctx.handle, _ffi.ptr(x), B, L, _ffi.ptr(dplan.wave_dev), _ffi.ptr(dplan.spec_dev),
                                                  _ffi.ptr(lam_d), 0, _ffi.ptr(logits), _ffi.ptr(probs), _ffi.ptr(ws), ws.numel(),
                                                  ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    logits.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(logits, eager)


def test_seeds(models):
    model = models("fp32_split")
    x = synth.synth_waveforms(4, 32000, seed=1).to(DEV)
    lam = A.mixup_lambdas(4, 1.0)
    a = model.forward_augmented(x, policy=FULL, mixup_lambda=lam, generator=torch.Generator().manual_seed(5))
    b = model.forward_augmented(x, policy=FULL, mixup_lambda=lam, generator=torch.Generator().manual_seed(5))
    c = model.forward_augmented(x, policy=FULL, mixup_lambda=lam, generator=torch.Generator().manual_seed(6))
    assert a["plan"] == b["plan"] and torch.equal(a["clipwise_logits"], b["clipwise_logits"])
    assert a["plan"] != c["plan"] and not torch.equal(a["clipwise_logits"], c["clipwise_logits"])
    assert a["clipwise_logits"].shape == (2, 527)
    torch.manual_seed(8)
    d = model.forward_augmented(x)                       # policy=None: the reference's SpecAugment, from the global generator
    torch.manual_seed(8)
    assert d["plan"] == A.draw_plan(A.AugmentPolicy.reference(), 4, 32000) and d["plan"].wave is None


def test_time_stripes_are_counted_in_frames(models):
    """A clip whose time stripes are given by hand equals its forward with those frames' features zeroed by torch."""
    model = models("fp32_split")
    L = 32000
    x = synth.synth_waveforms(2, L, seed=4).to(DEV)
    s = np.zeros(2, dtype=A.SPEC_DTYPE)
    s["t_bgn"][0, :2], s["t_len"][0, :2] = (10, 90), (7, 11)
    s["t_bgn"][1, 0], s["t_len"][1, 0] = 0, 30
    plan = A.AugmentPlan(2, L, None, s)
    feat = logmel(model, x)
    assert feat.shape == (2, 101, 224)
    feat[0, 10:17] = 0.0
    feat[0, 90:101] = 0.0
    feat[1, 0:30] = 0.0
    want0, want1 = forward_features(model, feat, L, "logits")
    out = model.forward_augmented(x, plan=plan)
    assert torch.equal(out["clipwise_logits"], want0) and torch.equal(out["clipwise_output"], want1)
    assert not torch.equal(want0, model(x)["clipwise_logits"])


# ---- fits ---------------------------------------------------------------------------------------------------------------------
def test_augmented_fit_equals_the_fit_on_the_augmented_rows(models):
    model = models("fp32_split")
    n, N, seed = 8, 5, 13
    waves = synth.synth_waveforms(n, 32000, seed=9).to(DEV)
    g = torch.Generator().manual_seed(0)
    target = (torch.rand(n, N, generator=g) < 0.4).float().to(DEV)
    policy = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), time_width=40)
    emb, soft = A.augmented_embeddings(model, waves, target, policy, views=2, mixup_alpha=0.5, seed=seed)
    assert emb.shape == (n, 768) and soft.shape == (n, N) and soft.dtype == torch.float32        # 2 views x n / 2 mixed rows
    assert bool(((soft > 0) & (soft < 1)).any())                                                    # mixed label rows
    want = finetune.fit_head(emb, soft, epochs=2, seed=seed)
    import copy
    m2 = copy.deepcopy(model)
    got = m2.fit_head(list(waves), target, augment=policy, views=2, mixup_alpha=0.5, epochs=2, seed=seed)
    assert torch.equal(got.weight, want.weight) and torch.equal(got.bias, want.bias) and torch.equal(got.loss, want.loss)
    assert m2.head_audioset.out_features == N and torch.equal(m2.head_audioset.weight.detach(), want.weight)
    # nothing on: the plain fit
    m3, m4 = copy.deepcopy(model), copy.deepcopy(model)
    a = m3.fit_head(waves, target, augment=A.AugmentPolicy.identity(), views=1, epochs=2, seed=seed)
    b = m4.fit_head(list(waves), target, epochs=2, seed=seed)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias) and torch.equal(a.loss, b.loss)
    cv = copy.deepcopy(model).cross_validate_head(waves, target, augment=policy, views=2, folds=2, epochs=1, seed=seed, install=False)
    assert len(cv.fold_ids) == 2 * n
