"""GPU (`-m gpu`): per-class AP / ROC-AUC / d' on the device (acx_tagging_metrics, pytorch/metrics.py) against sklearn 1.7.2 and
scipy computed live -- at the AudioSet eval set's shape, on ties, signed zeros, denormals and degenerate classes, through the
global-memory path (N > 32768), on strided and differently typed inputs, through the status word, on the model's own output and
through the evaluation harness and script."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from scipy.stats import norm
from sklearn import metrics as skm

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import evaluate as ev
from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sk(target, scores):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap = np.atleast_1d(skm.average_precision_score(target, scores, average=None))
        auc = np.atleast_1d(skm.roc_auc_score(target, scores, average=None))
        return {"average_precision": ap, "auc": auc, "d_prime": np.sqrt(2) * norm.ppf(auc)}


def gpu(target, scores, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tagging_metrics(target, scores, **kw)


def assert_matches(got, ref, tol=1e-12):
    for k in ("average_precision", "auc"):
        a, b = got[k], ref[k]
        assert a.dtype == np.float64 and a.shape == b.shape
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.nanmax(np.abs(a - b), initial=0.0) <= tol, (k, np.nanmax(np.abs(a - b)))
    a, b = got["d_prime"], ref["d_prime"]
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True)
    np.testing.assert_allclose(a[fin], b[fin], rtol=1e-10, atol=1e-12)


def test_eval_set_shape_against_sklearn():
    rs = np.random.RandomState(0)
    N, C = 20371, 527
    prev = np.concatenate([[1.0 / N, (N - 1.0) / N], np.geomspace(2.0 / N, 0.999, C - 2)])
    t = rs.uniform(size=(N, C)) < prev
    t[:, 0] = False                                      # exactly one positive in class 0
    t[123, 0] = True
    t[:, 1] = True                                       # N - 1 positives in class 1
    t[77, 1] = False
    logits = rs.standard_normal((N, C)) * 3 + 2.0 * t
    s = (1.0 / (1.0 + np.exp(-logits))).astype(np.float32)
    got = gpu(t, s)
    assert_matches(got, sk(t, s))
    dev = gpu(torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda())
    for k in got:
        assert np.array_equal(got[k], dev[k], equal_nan=True)


@pytest.mark.parametrize("kind", ["levels8", "saturated", "denormal", "shared"])
def test_ties(kind):
    rs = np.random.RandomState(["levels8", "saturated", "denormal", "shared"].index(kind))
    N, C = 3000, 24
    if kind == "levels8":
        s = (rs.randint(0, 8, size=(N, C)) / 7.0).astype(np.float32)
    elif kind == "saturated":
        s = rs.choice(np.array([0.0, -0.0, 1.0, 0.25], np.float32), size=(N, C), p=[0.3, 0.3, 0.3, 0.1])
    elif kind == "denormal":
        s = (rs.randint(-4, 5, size=(N, C)).astype(np.float32) * np.float32(1.4e-45)).astype(np.float32)
    else:
        s = np.full((N, C), 0.5, np.float32)
        s[rs.uniform(size=(N, C)) < 0.2] = 0.75
    t = rs.uniform(size=(N, C)) < rs.uniform(0.01, 0.9, size=C)
    t[0] = True
    t[1] = False
    assert_matches(gpu(t, s), sk(t, s))


def test_degenerate_classes():
    rs = np.random.RandomState(2)
    N, C = 500, 4
    s = rs.uniform(size=(N, C)).astype(np.float32)
    t = rs.uniform(size=(N, C)) < 0.3
    t[:, 0] = False
    t[:, 1] = True
    with pytest.warns(UserWarning, match="1 class"):
        got = tagging_metrics(t, s)
    assert got["average_precision"][0] == 0.0 and got["average_precision"][1] == 1.0
    assert np.isnan(got["auc"][:2]).all() and np.isnan(got["d_prime"][:2]).all()
    assert_matches(got, sk(t, s))
    one = gpu(np.array([[1.0, 0.0]]), np.array([[0.3, 0.7]], np.float32))      # N = 1
    assert one["average_precision"].tolist() == [1.0, 0.0] and np.isnan(one["auc"]).all()
    t1 = (rs.uniform(size=(N, 1)) < 0.4)
    s1 = rs.uniform(size=(N, 1)).astype(np.float32)
    assert_matches(gpu(t1, s1), sk(t1, s1))                                     # C = 1
    perfect = gpu(np.array([[1], [0], [1]]), np.array([[0.9], [0.1], [0.8]], np.float32))
    assert perfect["auc"][0] == 1.0 and perfect["d_prime"][0] == np.inf
    worst = gpu(np.array([[0], [1]]), np.array([[0.9], [0.1]], np.float32))
    assert worst["auc"][0] == 0.0 and worst["d_prime"][0] == -np.inf


def test_global_path_large_n():
    rs = np.random.RandomState(3)
    N, C = 100003, 16
    t = rs.uniform(size=(N, C)) < np.linspace(0.001, 0.999, C)
    s = rs.uniform(size=(N, C)).astype(np.float32)
    s[:, 3] = np.round(s[:, 3] * 50) / 50                                      # ties across chunks
    s[:, 4] = s[:, 4] * t[:, 4] + 0.5 * (1 - t[:, 4]) * s[:, 4]
    assert N > 32768
    assert_matches(gpu(t, s), sk(t, s))


def test_strided_dtypes_workspace_and_repeat():
    rs = np.random.RandomState(4)
    N, C = 4000, 40
    big_s = torch.from_numpy(rs.uniform(size=(N, C + 13)).astype(np.float32)).cuda()
    big_t = torch.from_numpy(rs.uniform(size=(N, C + 7)) < 0.2).cuda()
    s, t = big_s[:, 5:5 + C], big_t[:, 3:3 + C]
    assert s.stride(0) == C + 13 and not s.is_contiguous()
    ref = sk(t.cpu().numpy(), s.cpu().numpy())
    a = gpu(t, s)                                   # bool, strided
    assert_matches(a, ref)
    b = gpu(t.to(torch.uint8), s)
    c = gpu(t.to(torch.float32), s.contiguous())
    d = gpu(t, s)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], c[k], equal_nan=True)
        assert a[k].tobytes() == d[k].tobytes()
    # raw ABI: a workspace full of 0xFF gives the same bits; a short one is rejected
    sc, tg = s.contiguous(), t.contiguous().view(torch.uint8)
    n_ws = _ffi.metrics_workspace_bytes(N, C)
    ws = torch.full((n_ws,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((3, C), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    args = [vp(sc), C, vp(tg), _ffi.TARGET_U8, C, N, C, vp(out[0]), vp(out[1]), vp(out[2]), vp(st)]
    _ffi.check(_ffi.lib().acx_tagging_metrics(*args, vp(ws), n_ws, _ffi.stream_ptr(sc.device)))
    assert int(st.cpu()[0]) == 0
    o = out.cpu().numpy()
    assert o[0].tobytes() == a["average_precision"].tobytes() and o[1].tobytes() == a["auc"].tobytes()
    assert o[2].tobytes() == a["d_prime"].tobytes()
    rc = _ffi.lib().acx_tagging_metrics(*args, vp(ws), n_ws - 256, _ffi.stream_ptr(sc.device))
    assert rc == -5 and b"workspace" in _ffi.lib().acx_last_error()


def test_bad_device_data_raises_through_status():
    rs = np.random.RandomState(5)
    s = torch.from_numpy(rs.uniform(size=(300, 9)).astype(np.float32)).cuda()
    t = torch.from_numpy((rs.uniform(size=(300, 9)) < 0.5).astype(np.float32)).cuda()
    for bad in (float("nan"), float("inf"), float("-inf")):
        s2 = s.clone()
        s2[17, 4] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            tagging_metrics(t, s2)
    t2 = t.clone()
    t2[3, 8] = 0.5
    with pytest.raises(ValueError, match="other than 0 and 1"):
        tagging_metrics(t2, s)
    t3 = t.to(torch.uint8)
    t3[5, 2] = 3
    with pytest.raises(ValueError, match="other than 0 and 1"):
        tagging_metrics(t3, s)
    # the raw outputs of a data error are all NaN
    n_ws = _ffi.metrics_workspace_bytes(300, 9)
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
    out = torch.zeros((3, 9), dtype=torch.float64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    s2 = s.clone()
    s2[0, 0] = float("nan")
    _ffi.check(_ffi.lib().acx_tagging_metrics(vp(s2), 9, vp(t2), _ffi.TARGET_F32, 9, 300, 9, vp(out[0]), vp(out[1]), vp(out[2]),
                                              vp(st), vp(ws), n_ws, _ffi.stream_ptr(s.device)))
    assert int(st.cpu()[0]) == _ffi.METRICS_NONFINITE | _ffi.METRICS_BAD_TARGET
    assert torch.isnan(out).all()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="a call on a device that is not the current one needs two GPUs")
def test_runs_on_the_device_it_is_given_while_another_is_current():
    rs = np.random.RandomState(11)
    N, C = 64, 3
    s = rs.uniform(size=(N, C)).astype(np.float32)
    t = rs.uniform(size=(N, C)) < 0.4
    t[0], t[1] = True, False
    with torch.cuda.device(0):
        host_in = gpu(t, s, device="cuda:1")
        dev_in = gpu(torch.from_numpy(t).to("cuda:1"), torch.from_numpy(s).to("cuda:1"))
        assert torch.cuda.current_device() == 0
    assert_matches(host_in, sk(t, s))
    assert_matches(dev_in, sk(t, s))


@pytest.fixture(scope="module")
def model(synth_sd):
    from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    return m.to("cuda").eval()


def test_model_output_directly(model):
    from audioset_convnext_inf_amd import synth
    wav = synth.synth_waveforms(48, 32000, seed=9).cuda()
    with torch.no_grad():
        probs = model(wav)["clipwise_output"]
    rs = np.random.RandomState(6)
    t = rs.uniform(size=probs.shape) < 0.3
    t[0], t[1] = True, False
    assert_matches(gpu(torch.from_numpy(t).cuda(), probs), sk(t, probs.cpu().numpy()))


def test_harness_gpu_equals_sklearn(model):
    from audioset_convnext_inf_amd.utils.data_generator import ClipShard, evaluate_batches
    rs = np.random.RandomState(7)
    wav = (rs.standard_normal((40, 32000)) * 0.1 * 32767).astype(np.int16)
    tgt = rs.uniform(size=(40, 527)) < 0.3
    tgt[0], tgt[1] = True, False
    shard = ClipShard(wav, tgt)
    a = ev.evaluate_sharded(model, shard, batch_size=16, metrics="gpu")
    b = ev.evaluate_sharded(model, shard, batch_size=16, metrics="sklearn")
    assert_matches(a, b)
    c = ev.Evaluator(model, metrics="gpu").evaluate(evaluate_batches(shard, batch_size=16))
    assert_matches(c, b)
    with pytest.raises(ValueError):
        ev.Evaluator(model, metrics="cpu")


def test_evaluate_script_metrics_flag():
    script = os.path.join(ROOT, "evaluate_convnext_on_audioset.py")
    lines = {}
    for m in ("gpu", "sklearn"):
        r = subprocess.run([sys.executable, script, "--synthetic", "300", "--batch_size", "64", "--metrics", m],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[m] = re.findall(r"^Validate synthetic (?:mAP|AUC|d-prime): [0-9.\-]+$", r.stdout, flags=re.M)
        assert len(lines[m]) == 3 and re.search(r"^\(300 clips in [0-9.]+ s on 1 GPU\(s\): ", r.stdout, flags=re.M), r.stdout
    assert lines["gpu"] == lines["sklearn"]
