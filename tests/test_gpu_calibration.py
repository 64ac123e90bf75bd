"""GPU (`-m gpu`): calibration -- acx_reliability_counts / acx_reliability_toplabel, acx_platt_fit / acx_platt_apply,
acx_temperature_fit / acx_temperature_apply and the calls of pytorch/calibration.py up to ConvNeXt.tag / classify / calibrate.

The oracles are the float64 host definitions of pytorch/calibration.py on the inputs of tests/calibration_cases.py.  Counts are
compared exactly; float64 sums of non-negative terms within 2 n 2^-53 of the sum (two summation orders cannot differ by more);
the fits by the Newton step that the HOST computes at the point the DEVICE returned (cc.platt_bound / cc.temperature_bound)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import calibration_cases as cc
from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import calibration as cal
from audioset_convnext_inf_amd.pytorch import classify as cl
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.as_tensor(np.array(a)).to(DEV)                 # a copy: the cases are read-only


def dev_strided(a, pad=3):
    """`a` on the device as a column slice of a wider tensor whose other columns hold NaN (floats) or 7 (integers)."""
    t = dev(a)
    fill = float("nan") if t.dtype.is_floating_point else 7
    wide = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


# ---- reliability -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reliability_ref(n, C, bins):
    p, y = cc.probabilities(n, C)
    return cal.reliability_host(y, p, bins=bins)


@pytest.mark.parametrize("bins", cc.RELIABILITY_BINS)
@pytest.mark.parametrize("C", cc.RELIABILITY_CLASSES)
@pytest.mark.parametrize("n", cc.RELIABILITY_ROWS)
def test_reliability_counts_against_the_host(n, C, bins):
    p, y = cc.probabilities(n, C)
    ref = _reliability_ref(n, C, bins)
    kind = (n + C + bins) % 3                                      # bool, uint8 and float32 targets; strided inputs every other case
    target = dev(y) if kind == 0 else dev(y.astype(np.uint8)) if kind == 1 else dev(y.astype(np.float32))
    probs = dev(p)
    if (n + C) % 2:
        probs, target = dev_strided(p), dev_strided(target.cpu().numpy())
        assert probs.stride(0) == C + 3
    r = cal.reliability(target, probs, bins=bins).check()
    assert torch.equal(r.count.cpu(), torch.as_tensor(ref.count))
    assert torch.equal(r.positive.cpu(), torch.as_tensor(ref.positive))
    conf, brier = r.conf_sum.cpu().numpy(), r.brier_sum.cpu().numpy()
    assert (np.abs(conf - ref.conf_sum) <= cc.sum_bound(n, ref.conf_sum)).all()
    assert (np.abs(brier - ref.brier_sum) <= cc.sum_bound(n, ref.brier_sum)).all()
    assert np.allclose(r.ece, ref.ece, rtol=0, atol=1e-12) and abs(r.classwise_ece - ref.classwise_ece) <= 1e-12
    assert np.allclose(r.mce, ref.mce, rtol=0, atol=1e-12) and np.allclose(r.brier, ref.brier, rtol=1e-12, atol=0)
    again = cal.reliability(target, probs, bins=bins)              # the same call: the same bits
    assert torch.equal(again.conf_sum.view(torch.int64), r.conf_sum.view(torch.int64))
    assert torch.equal(again.brier_sum.view(torch.int64), r.brier_sum.view(torch.int64))
    assert torch.equal(again.count, r.count) and torch.equal(again.positive, r.positive)


@pytest.mark.parametrize("bins", cc.EDGE_BINS)
def test_reliability_edge_values_land_in_their_bins(bins):
    p, y, expect = cc.edge_probabilities(bins)
    r = cal.reliability(dev(y), dev(p), bins=bins).check()
    assert r.count.cpu().numpy()[0].tolist() == np.bincount(expect, minlength=bins).tolist()
    assert r.positive.cpu().numpy()[0].tolist() == np.bincount(expect, weights=y[:, 0], minlength=bins).astype(int).tolist()
    c, f, k = r.curve(0)
    assert k.sum() == p.shape[0] and len(c) == len(f) == len(k) == int((np.bincount(expect, minlength=bins) > 0).sum())


@pytest.mark.parametrize("what,match", [("nan", "NaN"), ("inf", "NaN"), ("above", "outside"), ("below", "outside"),
                                        ("target2", "other than 0 and 1"), ("target_half", "other than 0 and 1")])
def test_reliability_flags_bad_data(what, match):
    p, y = cc.probabilities(65, 3)
    p, t = p.copy(), y.astype(np.uint8 if what == "target2" else np.float32)
    if what == "nan":
        p[64, 2] = np.nan
    elif what == "inf":
        p[0, 0] = np.inf
    elif what == "above":
        p[33, 1] = np.nextafter(np.float32(1), np.float32(2))
    elif what == "below":
        p[33, 1] = -1e-30
    elif what == "target2":
        t[5, 1] = 2
    else:
        t[5, 1] = 0.5
    r = cal.reliability(dev(t), dev(p), bins=10)
    with pytest.raises(ValueError, match=match):
        r.check()
    with pytest.raises(ValueError, match=match):
        r.ece                                                      # the numbers are not handed out either


# ---- top-label reliability ---------------------------------------------------------------------------------------------------------
def _scaling(beta):
    return None if beta is None else cal.TemperatureScaling(torch.tensor([beta], dtype=torch.float64, device=DEV))


def _toplabel_inputs(n, N):
    z, y = cc.singlelabel(n, N, 1.0)
    return (dev_strided(z) if N == 2049 else dev(z)), dev(y), z, y


def _nll_bound(n, N, value):
    """nll_sum against the float64 value: two summation orders, 2 n 2^-53 of the sum, plus each row's own evaluation on the
    device -- s a float64 sum of depth D = softmax_depth(N) of exponentials, one log: (D + 4) 2^-53 (1 + term) per row."""
    D = _ffi.softmax_depth(N)
    return cc.U53 * (2.0 * n * value + (D + 4) * (n + value))


@pytest.mark.parametrize("beta", cc.TOPLABEL_BETAS)
@pytest.mark.parametrize("n,N", cc.TOPLABEL_SHAPES)
def test_toplabel_counts_follow_softmax_topk(n, N, beta):
    logits, labels, z, y = _toplabel_inputs(n, N)
    sc = _scaling(beta)
    for bins in (1, 15, 64):
        r = cal.reliability_toplabel(labels, logits, bins=bins, calibration=sc).check()
        scaled = logits if sc is None else sc.apply(logits)
        if sc is not None:                                         # (float)beta * z, one rounding
            assert torch.equal(scaled.cpu(), torch.as_tensor((np.float32(beta) * z).astype(np.float32)))
        _, top_prob, top_index = cl.softmax_topk(scaled, k=1, probabilities=False)
        ref = cal.reliability_toplabel_host(y, z, bins=bins, beta=beta, confidence=top_prob[:, 0].cpu().numpy(),
                                            prediction=top_index[:, 0].cpu().numpy())
        assert r.count.cpu().numpy().tolist() == ref.count.tolist()         # the confidences carry top_prob's bits: same bins
        assert r.correct.cpu().numpy().tolist() == ref.correct.tolist()
        assert (np.abs(r.conf_sum.cpu().numpy() - ref.conf_sum) <= cc.sum_bound(n, ref.conf_sum)).all()
        assert abs(float(r.nll_sum.item()) - ref.nll_sum) <= _nll_bound(n, N, ref.nll_sum)
        assert r.counted == n and abs(r.accuracy - ref.accuracy) < 1e-15 and abs(r.ece - ref.ece) < 1e-12
        assert abs(r.mce - ref.mce) < 1e-12 and len(r.curve()[0]) == int((ref.count > 0).sum())
        again = cal.reliability_toplabel(labels, logits, bins=bins, calibration=sc)
        assert torch.equal(again.conf_sum.view(torch.int64), r.conf_sum.view(torch.int64))
        assert torch.equal(again.nll_sum.view(torch.int64), r.nll_sum.view(torch.int64))


@pytest.mark.parametrize("n,N", [(65, 5), (33, 2049)])
def test_toplabel_flagged_rows_are_counted_nowhere(n, N):
    z, y = cc.singlelabel(n, N, 1.0)
    z, y = z.copy(), y.copy()
    z[3, N - 1] = np.nan
    z[7, 0] = np.inf
    y[11], y[12] = -1, N
    r = cal.reliability_toplabel(dev(y), dev(z), bins=15)
    assert int(r.status.item()) == _ffi.CAL_NONFINITE | _ffi.CAL_BAD_LABEL
    with pytest.raises(ValueError, match="NaN"):
        r.check()
    keep = np.ones(n, dtype=bool)
    keep[[3, 7, 11, 12]] = False
    ref = cal.reliability_toplabel_host(y[keep], z[keep], bins=15)
    full = cal.reliability_toplabel_host(y, z, bins=15)
    assert full.skipped == 4 and full.count.tolist() == ref.count.tolist()
    assert int(r.count.sum().item()) == n - 4
    assert r.correct.cpu().numpy().tolist() == ref.correct.tolist()
    assert abs(float(r.nll_sum.item()) - ref.nll_sum) <= _nll_bound(n, N, ref.nll_sum)
    only_label = cal.reliability_toplabel(dev(np.full(n, N, dtype=np.int64)), dev(cc.singlelabel(n, N, 1.0)[0]), bins=15)
    with pytest.raises(ValueError, match="labels"):
        only_label.check()
    assert int(only_label.count.sum().item()) == 0 and float(only_label.nll_sum.item()) == 0.0


# ---- Platt scaling -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _platt_ref(n, C, smooth):
    z, y = cc.multilabel(n, C)
    return cal.fit_platt_host(y, z, smooth=smooth)


def _check_platt(n, C, smooth, strided):
    z, y = cc.multilabel(n, C)
    ref_ab, ref_info = _platt_ref(n, C, smooth)
    logits, target = (dev_strided(z), dev_strided(y.astype(np.uint8))) if strided else (dev(z), dev(y))
    fit = cal.fit_platt(target, logits, smooth=smooth).check()
    ab, info = fit.ab.cpu().numpy(), fit.info.cpu().numpy()
    assert (info >= 0).all() and (ref_info >= 0).all()
    worst = 0.0
    for c in range(C):
        step, lam = cal.platt_newton_step_host(z[:, c], y[:, c], ab[c, 0], ab[c, 1], smooth)
        bound = cc.platt_bound(z[:, c], ab[c, 0], ab[c, 1], lam)
        worst = max(worst, float(np.abs(step).max()) / bound)
        assert np.abs(step).max() <= bound, (c, step, bound)
        assert np.abs(ab[c] - ref_ab[c]).max() <= 2 * bound, (c, ab[c], ref_ab[c], bound)
    print("platt n=%d C=%d smooth=%s: worst |newton step| / bound = %.3g" % (n, C, smooth, worst))
    again = cal.fit_platt(target, logits, smooth=smooth)
    assert torch.equal(again.ab.view(torch.int64), fit.ab.view(torch.int64)) and torch.equal(again.info, fit.info)
    assert torch.equal(fit.a, fit.ab[:, 0]) and torch.equal(fit.b, fit.ab[:, 1])


@pytest.mark.parametrize("C", cc.PLATT_CLASSES)
@pytest.mark.parametrize("n", cc.PLATT_ROWS)
def test_platt_fit_reaches_the_minimiser(n, C):
    _check_platt(n, C, True, strided=(n + C) % 2 == 1)
    if n > 2:
        _check_platt(n, C, False, strided=False)


def test_platt_fit_beyond_the_lds_column():
    _check_platt(*cc.PLATT_STREAMED, True, strided=False)


def test_platt_degenerate_separable_and_bad_data():
    z, y = cc.degenerate_multilabel()
    fit = cal.fit_platt(dev(y), dev(z)).check()
    assert fit.info.cpu().numpy()[1:].tolist() == [cal.DEGENERATE] * 3 and int(fit.info[0].item()) >= 0
    assert fit.ab.cpu().numpy()[1:].tolist() == [[1.0, 0.0]] * 3
    z, y = cc.separable()
    fit = cal.fit_platt(dev(y), dev(z), smooth=False)              # the iteration cap ends it
    info = fit.info.cpu().numpy()
    assert info[0] >= 0 and info[1] == cal.NOT_CONVERGED
    with pytest.raises(ValueError, match=r"did not converge for 1 class\(es\): 1"):
        fit.check()
    assert bool(torch.isfinite(fit.ab[0]).all())
    z2 = z.copy()
    z2[9, 0] = np.inf
    with pytest.raises(ValueError, match="NaN"):
        cal.fit_platt(dev(y), dev(z2)).check()
    with pytest.raises(ValueError, match="other than 0 and 1"):
        cal.fit_platt(dev(y.astype(np.uint8) * 2), dev(z)).check()


def test_platt_apply_general_and_file_round_trip(tmp_path):
    """General (a, b) within 8 * 2^-24 relative of the float64 sigmoid(fl32(a) z + fl32(b)): one expf, one add and one division
    at about 2 ulp each, with margin.  That count leaves out the fp32 rounding of u = fmaf(a, z, b) itself, which moves the
    sigmoid by (1 - p) |u| 2^-25 relative: inside the margin while |u| <= 8 (4 of the 8 units), so the inputs keep |u| <= 2 * 3.5 + 1
    = 8 by construction."""
    rs = np.random.RandomState(5)
    ab = np.stack([rs.uniform(0.5, 2.0, 65), rs.uniform(-1.0, 1.0, 65)], axis=1)
    z = rs.uniform(-3.5, 3.5, (257, 65)).astype(np.float32)
    ps = cal.PlattScaling(dev(ab))
    out = ps.apply(dev_strided(z)).cpu().numpy().astype(np.float64)
    ref = cal.platt_apply_host(z, ab)
    print("platt apply, |u| <= 8: worst relative error %.3g units of 2^-24" % (np.abs(out / ref - 1).max() * 2.0 ** 24))
    assert (np.abs(out - ref) <= 8 * 2.0 ** -24 * ref).all()
    path = str(tmp_path / "cal.npz")
    ps.save(path)
    back = cal.load_calibration(path, DEV)
    assert isinstance(back, cal.PlattScaling) and torch.equal(back.ab, ps.ab) and back.ab.is_cuda
    assert torch.equal(back.apply(dev(z)), ps.apply(dev(z)))
    with pytest.raises(ValueError, match="classes"):
        ps.apply(dev(z[:, :5]))


# ---- temperature scaling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta_star", cc.PLANTED_BETAS)
@pytest.mark.parametrize("n,N", cc.TOPLABEL_SHAPES)
def test_temperature_fit_reaches_the_minimiser(n, N, beta_star):
    z, y = cc.singlelabel(n, N, beta_star)
    ref_beta, ref_info = cal.fit_temperature_host(y, z, evaluations=cc.TEMPERATURE_EVALUATIONS)
    logits = dev_strided(z) if N == 2049 else dev(z)
    fit = cal.fit_temperature(dev(y), logits, evaluations=cc.TEMPERATURE_EVALUATIONS)
    beta, info = float(fit.beta.item()), int(fit.info.item())
    if ref_info < 0:                                               # n = 1: no finite minimiser (tests/test_calibration_cpu.py)
        assert info == ref_info == cal.NOT_CONVERGED and abs(beta - ref_beta) <= 1e-9 * ref_beta
        with pytest.raises(ValueError, match="did not converge"):
            fit.check()
        return
    fit.check()
    assert info > 0
    _, g, h, _ = cal.temperature_sums_host(y, z, beta)
    bound = cc.temperature_bound(z, beta, max(h, 1e-12))
    print("temperature n=%d N=%d beta*=%g: beta %.12g (host %.12g) in %d evaluations, |F'/F''| / bound = %.3g"
          % (n, N, beta_star, beta, ref_beta, info, abs(g / h) / bound))
    assert abs(g / max(h, 1e-12)) <= bound
    assert abs(beta - ref_beta) <= 2 * bound
    assert abs(fit.temperature - 1.0 / beta) < 1e-15
    again = cal.fit_temperature(dev(y), logits, evaluations=cc.TEMPERATURE_EVALUATIONS)
    assert torch.equal(again.beta.view(torch.int64), fit.beta.view(torch.int64)) and torch.equal(again.info, fit.info)


def test_temperature_codes():
    z, y = cc.constant_rows()
    fit = cal.fit_temperature(dev(y), dev(z)).check()
    assert float(fit.beta.item()) == 1.0 and int(fit.info.item()) == cal.DEGENERATE
    z, y = cc.singlelabel(65, 5, 1.0)
    fit = cal.fit_temperature(dev(y), dev(z), evaluations=1)
    assert float(fit.beta.item()) == 1.0 and int(fit.info.item()) == cal.NOT_CONVERGED
    for name, (z, y) in cc.bound_cases().items():
        fit = cal.fit_temperature(dev(y), dev(z), evaluations=cc.TEMPERATURE_EVALUATIONS)
        beta = float(fit.beta.item())
        assert int(fit.info.item()) == cal.AT_BOUND, (name, beta)
        assert (9.99e3 < beta <= 1e4) if name == "high" else (1e-4 <= beta < 1.001e-4), (name, beta)
        with pytest.raises(ValueError, match="bound"):
            fit.check()
    z, y = cc.singlelabel(65, 5, 1.0)
    y = y.copy()
    y[4] = 5
    fit = cal.fit_temperature(dev(y), dev(z))
    with pytest.raises(ValueError, match="labels"):
        fit.check()
    keep = np.arange(65) != 4                                      # the flagged row enters no sum
    ref_beta, ref_info = cal.fit_temperature_host(y[keep], z[keep])
    assert ref_info > 0 and abs(float(fit.beta.item()) - ref_beta) <= 1e-9


def test_temperature_fit_under_graph_capture_gives_the_eager_bits():
    z, y = cc.singlelabel(257, 50, 3.0)
    logits, labels = dev(z), dev(y)
    eager = cal.fit_temperature(labels, logits)
    eager_scaled = eager.apply(logits)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cal.fit_temperature(labels, logits)                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fit = cal.fit_temperature(labels, logits)
        scaled = fit.apply(logits)
    for _ in range(2):
        fit.beta.zero_()
        fit.info.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(fit.beta.view(torch.int64), eager.beta.view(torch.int64))
        assert torch.equal(fit.info, eager.info) and int(fit.info.item()) > 0
        assert torch.equal(scaled, eager_scaled)


def test_temperature_apply_softmax_and_file_round_trip(tmp_path):
    z, _ = cc.singlelabel(65, 5, 1.0)
    t = cal.TemperatureScaling(torch.tensor([0.7], dtype=torch.float64, device=DEV))
    scaled = t.apply(dev_strided(z))
    assert torch.equal(scaled.cpu(), torch.as_tensor((np.float32(0.7) * z).astype(np.float32)))
    got = t.softmax_topk(dev(z), k=3)
    want = cl.softmax_topk(scaled, k=3)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    path = str(tmp_path / "t.npz")
    t.save(path)
    back = cal.load_calibration(path, DEV)
    assert isinstance(back, cal.TemperatureScaling) and torch.equal(back.beta, t.beta) and back.beta.is_cuda
    with pytest.raises(ValueError, match="not Platt"):
        cal.PlattScaling.load(path, DEV)


# ---- the model surface -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(synth_sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    return m.to(DEV).eval()


def test_model_surface(model):
    x = synth.synth_waveforms(3, 32000, seed=11).to(DEV)
    with torch.no_grad():
        out = model(x)
        logits, probs = out["clipwise_logits"], out["clipwise_output"]
        N = logits.shape[1]
        # a = 1, b = 0 is the forward's sigmoid, bit for bit
        ident = cal.PlattScaling(torch.tensor([[1.0, 0.0]] * N, dtype=torch.float64, device=DEV))
        assert torch.equal(ident.apply(logits), probs)
        # calibration=None changes nothing
        a, b = model.tag(x, 0.5), model.tag(x, 0.5, calibration=None)
        assert all(torch.equal(a[k], b[k]) for k in a)
        a, b = model.classify(x, k=5), model.classify(x, k=5, calibration=None)
        assert all(torch.equal(a[k], b[k]) for k in a)
        # with a calibration: apply + the existing call
        rs = np.random.RandomState(2)
        ps = cal.PlattScaling(dev(np.stack([np.exp(0.3 * rs.randn(N)), rs.randn(N)], axis=1)))
        t = model.tag(x, 0.4, calibration=ps)
        assert torch.equal(t["clipwise_output"], ps.apply(logits)) and torch.equal(t["labels"], ps.apply(logits) >= 0.4)
        assert torch.equal(t["clipwise_logits"], logits)
        ts = cal.TemperatureScaling(torch.tensor([1.7], dtype=torch.float64, device=DEV))
        c = model.classify(x, k=5, calibration=ts)
        pr, tp, ti = cl.softmax_topk(ts.apply(logits), k=5)
        assert torch.equal(c["probabilities"], pr) and torch.equal(c["top_probabilities"], tp) and torch.equal(c["top_indices"], ti)
        assert torch.equal(c["clipwise_logits"], logits)
        with pytest.raises(ValueError, match="PlattScaling"):
            model.tag(x, 0.5, calibration=ts)
        with pytest.raises(ValueError, match="TemperatureScaling"):
            model.classify(x, calibration=ps)
        # calibrate(): from logits, and from waveforms whose logits are extracted first
        z, y = cc.multilabel(65, N)
        fit = model.calibrate(dev(z), dev(y), method="platt")
        assert torch.equal(fit.ab, cal.fit_platt(dev(y), dev(z)).ab)
        waves = [w for w in synth.synth_waveforms(4, 32000, seed=12)]
        labels = torch.tensor([1, 0, 3, 2])
        fit = model.calibrate(waves, labels, method="temperature", evaluations=8)
        wl = torch.stack([model(w[None].to(DEV))["clipwise_logits"][0] for w in waves])
        assert torch.equal(fit.beta, cal.fit_temperature(labels.to(DEV), wl, evaluations=8).beta)
        with pytest.raises(ValueError, match="method"):
            model.calibrate(dev(z), dev(y), method="isotonic")


@pytest.mark.parametrize("loss", ["bce", "ce"])
def test_demo_scripts_write_and_load_a_calibration(tmp_path, loss):
    out = str(tmp_path / "tagger")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo_finetune.py"), "--synthetic", "--clips", "120", "--classes", "4",
                        "--epochs", "2", "--val-fraction", "0.5", "--loss", loss, "--out", out], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ECE" in r.stdout and "before" in r.stdout and "after" in r.stdout, r.stdout[-1500:]
    path = out + ".calibration.npz"
    assert os.path.isfile(path)
    with np.load(path) as f:
        assert str(f["method"]) == ("platt" if loss == "bce" else "temperature")
    import wave
    wav = str(tmp_path / "clip.wav")
    pcm = (0.3 * np.sin(2 * np.pi * 350.0 * np.arange(32000) / 32000.0) * 32767).astype("<i2")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(32000)
        w.writeframes(pcm.tobytes())
    args = [sys.executable, os.path.join(ROOT, "demo_convnext.py"), "--ckpt", os.path.join(out, "model.safetensors"), "--wav", wav,
            "--calibration", path] + (["--softmax", "--top", "3"] if loss == "ce" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "calibration" in r.stdout.lower(), r.stdout[-1500:]
