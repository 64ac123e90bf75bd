"""GPU (`-m gpu`): per-class operating points on the device (acx_operating_points / acx_threshold_counts, pytorch/metrics.py), the
event decoder with one threshold / low per class (acx_decode_events_classwise, pytorch/segments.py) and ConvNeXt.tag /
detect_events with them.  Everything is held to operating_points_host (the numpy float64 definition), numpy, or the host
decode_events: thresholds are compared as float32 bit patterns, counts and events as exact values; an event's `mean` within the
2.5e-6 of test_gpu_events.py (numpy's float32 pairwise mean on the host against the float64 mean on the device)."""
import ctypes
import functools
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch.metrics import (operating_points, operating_points_host, tagging_metrics,
                                                       threshold_metrics)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN_ABS = 2.5e-6
KINDS = ["levels8", "saturated", "denormal", "shared"]
CRITERIA = [("fbeta", 0.5), "f1", ("fbeta", 2.0), ("precision", 0.5), ("precision", 0.9), ("precision", 1.0), ("recall", 0.5),
            ("recall", 1.0)]


def bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def assert_equals_host(t, s, criterion, got=None):
    """operating_points on the device (or `got`) against the host definition: the same bits, the same integers"""
    got = quiet(operating_points, t, s, criterion) if got is None else got
    t_h, s_h = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (t, s))
    ref = operating_points_host(t_h, s_h, criterion)
    assert got.threshold.dtype == torch.float32 and got.counts.dtype == torch.int64 and got.threshold.is_cuda
    gb, rb = bits(got.threshold), bits(ref.threshold)
    assert np.array_equal(gb, rb), (criterion, np.nonzero(gb != rb)[0][:5], got.threshold.cpu().numpy()[gb != rb][:5],
                                    ref.threshold[gb != rb][:5])
    assert np.array_equal(got.counts.cpu().numpy(), ref.counts), criterion
    return got, ref


@functools.lru_cache(maxsize=None)
def tie_family(kind):
    """the four tie families of test_gpu_metrics.py::test_ties -> (bool targets, float32 scores), read-only"""
    rs = np.random.RandomState(KINDS.index(kind))
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
    t.setflags(write=False)
    s.setflags(write=False)
    return t, s


@functools.lru_cache(maxsize=None)
def continuous():
    """3000 x 24 scores without planted ties, priors 0.01 .. 0.9"""
    rs = np.random.RandomState(21)
    t = rs.uniform(size=(3000, 24)) < rs.uniform(0.01, 0.9, size=24)
    t[0], t[1] = True, False
    s = (1.0 / (1.0 + np.exp(-(rs.standard_normal((3000, 24)) * 1.5 + 1.5 * t)))).astype(np.float32)
    t.setflags(write=False)
    s.setflags(write=False)
    return t, s


@pytest.mark.parametrize("criterion", CRITERIA, ids=lambda c: c if isinstance(c, str) else "%s%g" % c)
@pytest.mark.parametrize("kind", KINDS + ["continuous"])
def test_criteria_on_ties(kind, criterion):
    t, s = continuous() if kind == "continuous" else tie_family(kind)
    got, ref = assert_equals_host(t, s, criterion)
    if kind == "saturated":
        z = got.threshold.cpu().numpy()
        assert not np.signbit(z[z == 0]).any(), "a zero threshold is +0.0"


def test_degenerate_shapes():
    one_t, one_s = np.array([[1.0, 0.0]]), np.array([[0.3, 0.7]], np.float32)           # N = 1: one class without positives
    with pytest.warns(UserWarning, match="1 class"):
        got = operating_points(one_t, one_s)
    assert bits(got.threshold).tolist() == bits([0.3, np.inf]).tolist() and got.counts.tolist() == [[1, 0, 0, 0], [0, 0, 0, 1]]
    rs = np.random.RandomState(2)
    s1 = rs.uniform(size=(500, 1)).astype(np.float32)                                    # C = 1
    t1 = rs.uniform(size=(500, 1)) < 0.4
    for crit in CRITERIA:
        assert_equals_host(t1, s1, crit)
    s = rs.uniform(size=(500, 5)).astype(np.float32)
    t = rs.uniform(size=(500, 5)) < 0.3
    t[:, 0] = False                                                                      # no positives
    t[:, 1] = True                                                                       # no negatives
    t[:, 3] = False                                                                      # no positives either
    s[:, 2] = np.where(t[:, 2], 0.5 * s[:, 2], s[:, 2])
    s[np.nonzero(~t[:, 2])[0][0], 2] = 0.99                                              # precision 1 out of reach in class 2
    with pytest.warns(UserWarning, match="2 class"):
        got = operating_points(t, s, ("precision", 1.0))
    assert_equals_host(t, s, ("precision", 1.0), got)
    thr, cnt = got.threshold.cpu().numpy(), got.counts.cpu().numpy()
    P2 = int(t[:, 2].sum())
    assert np.isposinf(thr[[0, 2, 3]]).all() and cnt[0].tolist() == [0, 0, 0, 500] and cnt[2].tolist() == [0, 0, P2, 500 - P2]
    assert cnt[1].tolist() == [500, 0, 0, 0] and thr[1] == s[:, 1].min()                 # no negatives: the lowest score will do
    for crit in ("f1", ("recall", 1.0)):
        got, _ = assert_equals_host(t, s, crit)
        assert got.counts[1].tolist() == [500, 0, 0, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                   # every class has positives: no warning
        operating_points(t1, s1)


@pytest.mark.parametrize("n", [32768, 32769])
def test_lds_global_boundary(n):
    rs = np.random.RandomState(n)
    t = rs.uniform(size=(n, 3)) < np.array([0.02, 0.5, 0.97])
    s = rs.uniform(size=(n, 3)).astype(np.float32)
    s[:, 1] = np.round(s[:, 1] * 1000) / 1000
    for crit in ("f1", ("precision", 0.9), ("recall", 0.5)):
        assert_equals_host(torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda(), crit)


def test_global_path_ties_across_chunks():
    rs = np.random.RandomState(40)
    n = 40000
    t = rs.uniform(size=(n, 3)) < np.array([0.1, 0.5, 0.9])
    s = (np.round((rs.uniform(size=(n, 3)) * 0.6 + 0.3 * t) * 50) / 50).astype(np.float32)      # 1/50 steps: ties straddle chunks
    td, sd = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()
    for crit in CRITERIA:
        assert_equals_host(td, sd, crit)


def test_strided_dtypes_workspace_and_repeat():
    rs = np.random.RandomState(4)
    N, C = 4000, 40
    big_s = torch.from_numpy(rs.uniform(size=(N, C + 13)).astype(np.float32)).cuda()
    big_t = torch.from_numpy(rs.uniform(size=(N, C + 7)) < 0.2).cuda()
    s, t = big_s[:, 5:5 + C], big_t[:, 3:3 + C]
    assert s.stride(0) == C + 13 and not s.is_contiguous()
    a, _ = assert_equals_host(t, s, "f1")                                                # bool, strided
    b = operating_points(t.to(torch.uint8), s)
    c = operating_points(t.to(torch.float32), s.contiguous())
    d = operating_points(t, s)
    e = operating_points(t.cpu().numpy(), s.cpu().numpy())                               # host arrays
    for o in (b, c, d, e):
        assert bits(o.threshold).tobytes() == bits(a.threshold).tobytes() and torch.equal(o.counts, a.counts)
    held = threshold_metrics(t, s, a.threshold)                                          # the same slices, no sort
    assert torch.equal(held.counts, a.counts)
    assert torch.equal(threshold_metrics(t.to(torch.float32), s.contiguous(), a.threshold.cpu().numpy()).counts, a.counts)
    # raw ABI: a workspace full of 0xFF gives the same bits; a short one is refused
    sc, tg = s.contiguous(), t.contiguous().view(torch.uint8)
    n_ws = _ffi.metrics_workspace_bytes(N, C)
    ws = torch.full((n_ws,), 0xFF, dtype=torch.uint8, device="cuda")
    thr = torch.full((C,), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((C, 4), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    spec = _ffi.AcxOperatingSpec(_ffi.OP_FBETA, 1.0)
    args = [vp(sc), C, vp(tg), _ffi.TARGET_U8, C, N, C, ctypes.byref(spec), vp(thr), vp(cnt), vp(st)]
    _ffi.check(_ffi.lib().acx_operating_points(*args, vp(ws), n_ws, _ffi.stream_ptr(sc.device)))
    assert int(st.cpu()[0]) == 0
    assert bits(thr).tobytes() == bits(a.threshold).tobytes() and torch.equal(cnt, a.counts)
    rc = _ffi.lib().acx_operating_points(*args, vp(ws), n_ws - 256, _ffi.stream_ptr(sc.device))
    assert rc == -5 and b"workspace" in _ffi.lib().acx_last_error()


def test_bad_device_data_raises_through_status():
    rs = np.random.RandomState(5)
    s = torch.from_numpy(rs.uniform(size=(300, 9)).astype(np.float32)).cuda()
    t = torch.from_numpy((rs.uniform(size=(300, 9)) < 0.5).astype(np.float32)).cuda()
    thr = torch.full((9,), 0.5, device="cuda")
    s2 = s.clone()
    s2[17, 4] = float("nan")
    t2 = t.to(torch.uint8)
    t2[5, 2] = 2
    for fn, extra in ((operating_points, ()), (threshold_metrics, (thr,))):
        with pytest.raises(ValueError, match="NaN or infinite"):
            fn(t, s2, *extra)
        with pytest.raises(ValueError, match="other than 0 and 1"):
            fn(t2, s, *extra)
    bad = thr.clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError, match="thresholds hold a NaN"):
        threshold_metrics(t, s, bad)
    with pytest.raises(ValueError, match="thresholds hold a NaN"):
        threshold_metrics(t, s, bad.cpu().numpy())
    with pytest.raises(ValueError, match="for 9 classes"):
        threshold_metrics(t, s, thr[:8])
    # the raw outputs of a data error: NaN thresholds, -1 counts
    n_ws = _ffi.metrics_workspace_bytes(300, 9)
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
    out = torch.zeros(9, dtype=torch.float32, device="cuda")
    cnt = torch.zeros((9, 4), dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.operating_points(vp(s2), 9, vp(t2), _ffi.TARGET_U8, 9, 300, 9, _ffi.OP_RECALL, 0.5, vp(out), vp(cnt), vp(st), (vp(ws), n_ws),
                          _ffi.stream_ptr(s.device))
    assert int(st.cpu()[0]) == _ffi.METRICS_NONFINITE | _ffi.METRICS_BAD_TARGET
    assert torch.isnan(out).all() and bool((cnt == -1).all())
    cnt.zero_()
    _ffi.threshold_counts(vp(s), 9, vp(t), _ffi.TARGET_F32, 9, 300, 9, vp(bad), vp(cnt), vp(st), _ffi.stream_ptr(s.device))
    assert int(st.cpu()[0]) == _ffi.METRICS_BAD_THRESHOLD and bool((cnt == -1).all())


def numpy_counts(t, s, thr):
    fire = s >= thr[None, :]
    return np.stack([(fire & t).sum(0), (fire & ~t).sum(0), (~fire & t).sum(0), (~fire & ~t).sum(0)], axis=1).astype(np.int64)


def test_threshold_metrics_against_numpy():
    rs = np.random.RandomState(6)
    N, C = 1037, 70                                                                      # several row chunks, two class tiles
    s = rs.uniform(size=(N, C)).astype(np.float32)
    s[:, 1] = rs.choice(np.array([0.0, -0.0, 0.5], np.float32), size=N)
    s[:, 2] = -s[:, 2]
    t = rs.uniform(size=(N, C)) < rs.uniform(0.05, 0.9, size=C)
    thr = rs.uniform(size=C).astype(np.float32)
    thr[0] = np.inf
    thr[1] = -0.0                                                                        # against +0.0 and -0.0 scores: all >= it
    thr[2] = -np.inf
    thr[3:40] = s[rs.randint(0, N, size=37), np.arange(3, 40)]                           # exactly a score of the column
    thr[69] = 2.0
    got = threshold_metrics(t, s, thr)
    want = numpy_counts(t, s, thr)
    assert np.array_equal(got.counts.cpu().numpy(), want)
    assert want[0, :2].tolist() == [0, 0] and want[1, 2:].tolist() == [0, 0] and want[2, 2:].tolist() == [0, 0]
    assert bits(got.threshold).tobytes() == bits(thr).tobytes()
    again = threshold_metrics(torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(thr).cuda())
    assert torch.equal(again.counts, got.counts)
    np.testing.assert_allclose(got.precision[3:40], want[3:40, 0] / (want[3:40, 0] + want[3:40, 1]), rtol=0, atol=0)
    assert got.micro()["f"] == 2 * want[:, 0].sum() / (2 * want[:, 0].sum() + want[:, 2].sum() + want[:, 1].sum())


@pytest.mark.parametrize("kind", ["levels8", "denormal", "continuous"])
def test_round_trip(kind):
    t, s = continuous() if kind == "continuous" else tie_family(kind)
    td, sd = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()
    for crit in ("f1", ("precision", 0.9), ("recall", 0.5)):
        op = quiet(operating_points, td, sd, crit)
        assert torch.equal(threshold_metrics(td, sd, op.threshold).counts, op.counts)


def test_tagging_metrics_unchanged_by_operating_points():
    t, s = continuous()
    td, sd = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()
    first = quiet(tagging_metrics, td, sd)
    quiet(operating_points, td, sd, ("fbeta", 2.0))                                      # the same workspace size, just freed
    second = quiet(tagging_metrics, td, sd)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes()
    big_t = torch.from_numpy(np.random.RandomState(8).uniform(size=(33000, 2)) < 0.3).cuda()              # the global kernels
    big_s = torch.from_numpy(np.random.RandomState(9).uniform(size=(33000, 2)).astype(np.float32)).cuda()
    first = quiet(tagging_metrics, big_t, big_s)
    quiet(operating_points, big_t, big_s)
    second = quiet(tagging_metrics, big_t, big_s)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes()


# ---- the decoder with one threshold / low per class -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def probabilities(B, S, N, seed=0):
    """test_gpu_events.py's recipe: sigmoid of smoothed noise with planted ties and values exactly on 0.5 and 0.3"""
    g = torch.Generator().manual_seed(4321 + seed)
    z = torch.randn(B, S + 4, N, generator=g, dtype=torch.float64)
    z = (z[:, :-4] + z[:, 1:-3] + z[:, 2:-2] + z[:, 3:-1] + z[:, 4:]) / 5 ** 0.5
    p = torch.sigmoid(3.0 * (z - 0.52)).to(torch.float32)
    u = torch.rand(B, S, N, generator=g)
    p[u < 0.03] = 0.5
    p[(u >= 0.03) & (u < 0.06)] = 0.3
    p = p.numpy()
    p.setflags(write=False)
    return p


def levels(N, p=None, seed=0):
    """per-class (threshold, low): spread over (0.2, 0.8), some exactly 0.5 / 0.3 (planted values), one +inf, one equal pair"""
    rs = np.random.RandomState(100 + seed)
    thr = rs.uniform(0.2, 0.8, size=N).astype(np.float32)
    low = (thr * rs.uniform(0.3, 1.0, size=N)).astype(np.float32)
    thr[::5], low[::5] = 0.5, 0.3
    if N > 2:
        thr[2], low[2] = np.inf, 0.25
        thr[1] = low[1]
    if N > 66:
        thr[66], low[66] = np.inf, np.inf
    return thr, low


def compare(table, clips, edges=None, min_events=0, **args):
    """every event of the device table against decode_events on the host with the same arguments"""
    host = [seg.decode_events(p, step=seg.SEGMENT_SECONDS if edges is None else edges[i], **args) for i, p in enumerate(clips)]
    total = sum(len(h) for h in host)
    assert total >= min_events, "the case holds %d events, %d wanted" % (total, min_events)
    got = table.to_lists()
    assert len(got) == len(host) and len(table) == total
    for i, (g, h) in enumerate(zip(got, host)):
        assert len(g) == len(h), "clip %d: %d events on the device, %d on the host" % (i, len(g), len(h))
        for a, b in zip(g, h):
            assert a[:4] == b[:4], "clip %d: %r on the device, %r on the host" % (i, a, b)
            assert abs(a[4] - b[4]) <= MEAN_ABS, "clip %d: mean %r on the device, %r on the host" % (i, a[4], b[4])
    return host


@pytest.mark.parametrize("median", [1, 3, 9])
@pytest.mark.parametrize("N", [1, 64, 70])
def test_decoder_per_class(N, median):
    p = probabilities(3, 40, N)
    thr, low = levels(N)
    x = torch.from_numpy(p).cuda()
    thr_d, low_d = torch.from_numpy(thr).cuda(), torch.from_numpy(low).cuda()
    args = dict(median=median, merge_gap=0.33 if median == 3 else 0.0, min_duration=0.65 if median == 9 else 0.0)
    host = compare(seg.decode_events_gpu(x, threshold=thr_d, low=low_d, **args), list(p), threshold=thr, low=low,
                   min_events=3 * N // 2, **args)
    if N > 2:
        assert not [e for clip in host for e in clip if e[0] in (2, 66)], "+inf: the class emits nothing"
    # host arrays are taken like tensors; low=None is the class's own threshold; a number stands for every class
    a = seg.decode_events_gpu(x, threshold=thr, low=low, **args)
    b = seg.decode_events_gpu(x, threshold=thr_d, low=low_d, **args)
    assert len(a) == len(b) and torch.equal(a.table[:len(a)], b.table[:len(b)])
    compare(seg.decode_events_gpu(x, threshold=thr_d, **args), list(p), threshold=thr, **args)
    compare(seg.decode_events_gpu(x, threshold=thr_d, low=0.1, **args), list(p), threshold=thr, low=0.1, **args)
    compare(seg.decode_events_gpu(x, threshold=0.9, low=torch.clamp(low_d, max=0.9), **args), list(p), threshold=0.9,
            low=np.minimum(low, np.float32(0.9)), **args)
    # a constant tensor gives the scalar call's table, byte for byte
    for kw in (dict(), dict(low=0.3)):
        scalar = seg.decode_events_gpu(x, threshold=0.5, **kw, **args)
        const = seg.decode_events_gpu(x, threshold=torch.full((N,), 0.5, device="cuda"),
                                      **{k: torch.full((N,), v, device="cuda") for k, v in kw.items()}, **args)
        assert len(scalar) == len(const) > 0
        assert torch.equal(scalar.table[:len(scalar)], const.table[:len(const)])


def test_decoder_bad_levels_raise_at_first_read():
    p = probabilities(3, 40, 70)
    x = torch.from_numpy(p).cuda()
    thr, low = levels(70)
    for cls, (tv, lv) in ((69, (0.4, 0.5)), (0, (float("nan"), 0.1)), (65, (0.5, float("nan"))), (7, (0.5, -0.1))):
        t2, l2 = torch.from_numpy(thr).cuda(), torch.from_numpy(low).cuda()
        t2[cls], l2[cls] = tv, lv
        table = seg.decode_events_gpu(x, threshold=t2, low=l2)                           # nothing raises yet
        with pytest.raises(ValueError, match=r"low must be in \[0, threshold\]"):
            len(table)
        assert int(table.status.cpu()) == _ffi.EVENTS_BAD_THRESHOLD and int(table.count.cpu()) == 0
    t2 = torch.from_numpy(thr).cuda()
    t2[3] = float("nan")
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\]"):
        seg.decode_events_gpu(x, threshold=t2).to_lists()
    with pytest.raises(ValueError, match="69 per-class values for 70 classes"):
        seg.decode_events_gpu(x, threshold=t2[:69])
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\] .* in class 4"):
        seg.decode_events_gpu(x, threshold=0.5, low=np.where(np.arange(70) == 4, 0.6, 0.2))      # host arrays: before the launch


def test_decoder_varlen_and_overflow_rerun():
    N = 70
    thr, low = levels(N, seed=1)
    thr_d, low_d = torch.from_numpy(thr).cuda(), torch.from_numpy(low).cuda()
    clips = [probabilities(1, S, N, seed=S)[0] for S in (40, 7, 23)]
    args = dict(median=3, merge_gap=0.33)
    packed = torch.from_numpy(np.concatenate(clips)).cuda()
    t = seg.decode_events_gpu(packed, steps=[40, 7, 23], threshold=thr_d, low=low_d, **args)
    compare(t, clips, threshold=thr, low=low, min_events=50, **args)
    t2 = seg.decode_events_gpu([torch.from_numpy(c).cuda() for c in clips], threshold=thr_d, low=low_d, **args)
    assert torch.equal(t.table[:len(t)], t2.table[:len(t2)])
    edges = [np.concatenate([np.arange(S) * 0.32, [S * 0.32 - 0.1]]) for S in (40, 7, 23)]
    t3 = seg.decode_events_gpu(packed, steps=[40, 7, 23], step=edges, threshold=thr_d, low=low_d, **args)
    compare(t3, clips, edges=edges, threshold=thr, low=low, **args)
    # a table of one row: decoded again at the exact size, with the same per-class values
    x = torch.from_numpy(probabilities(3, 40, N)).cuda()
    full = seg.decode_events_gpu(x, threshold=thr_d, low=low_d, **args)
    small = seg.decode_events_gpu(x, threshold=thr_d, low=low_d, capacity=1, **args)
    assert small.capacity == 1 and len(small) == len(full) > 100 and small.capacity == len(full)
    assert torch.equal(small.table, full.table[:len(full)])
    small_v = seg.decode_events_gpu(packed, steps=[40, 7, 23], threshold=thr_d, low=low_d, capacity=1, **args)
    assert len(small_v) == len(t) and torch.equal(small_v.table, t.table[:len(t)])


# ---- the model -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(synth_sd):
    from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    return m.to("cuda").eval()


def test_model_tag_and_detect_events(model):
    wav = synth.synth_waveforms(3, 2 * 32000, seed=12).cuda()
    with torch.no_grad():
        probs = model(wav)["clipwise_output"]
        segs = model.forward_segments(wav)
    # thresholds from the model's own scores: the per-class median of 3 clips, so that labels of both kinds occur
    thr = probs.median(dim=0).values
    thr[5] = float("inf")
    with torch.no_grad():
        out = model.tag(wav, thr)
    assert out["labels"].dtype == torch.bool and out["labels"].shape == probs.shape
    assert torch.equal(out["labels"], probs >= thr) and torch.equal(out["clipwise_output"], probs)
    assert 0 < int(out["labels"].sum()) < out["labels"].numel() and not bool(out["labels"][:, 5].any())
    assert torch.equal(model.tag(wav, thr.cpu().numpy())["labels"], out["labels"])
    assert torch.equal(model.tag(wav, 0.5)["labels"], probs >= 0.5)
    with pytest.raises(ValueError, match="for 527 classes"):
        model.tag(wav, thr[:100])
    # detect_events with per-class tensors = the decoder on forward_segments' output
    so = segs["segmentwise_output"]
    thr_e = so.amax(dim=(0, 1)) * 0.98
    low_e = thr_e * 0.9
    with torch.no_grad():
        det = model.detect_events(wav, threshold=thr_e, low=low_e, median=3)
    assert torch.equal(det["segmentwise_output"], so)
    want = seg.decode_events_gpu(so, threshold=thr_e, low=low_e, median=3, step=segs["segment_edges"].numpy())
    assert len(det["events"]) == len(want) >= 527 and torch.equal(det["events"].table[:len(want)], want.table[:len(want)])
    compare(det["events"], list(so.cpu().numpy()), edges=[segs["segment_edges"].numpy()] * 3, threshold=thr_e.cpu().numpy(),
            low=low_e.cpu().numpy(), median=3)
    with pytest.raises(ValueError, match="per-class"):
        model.detect_events(wav, threshold=thr_e[:10])                                   # before the forward runs
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\]"):
        model.detect_events(wav, threshold=thr_e.cpu().numpy(), low=(thr_e * 1.1).cpu().numpy())


def test_demo_finetune_writes_thresholds(tmp_path):
    out = str(tmp_path / "tagger")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo_finetune.py"), "--synthetic", "--clips", "200", "--classes", "5",
                        "--epochs", "3", "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^val F1 at per-class thresholds: macro ([0-9.]+)  micro ([0-9.]+)  \(mAP [0-9.]+;", r.stdout, flags=re.M)
    assert m, r.stdout[-1500:]
    assert 0.0 <= float(m.group(1)) <= 1.0 and 0.0 <= float(m.group(2)) <= 1.0
    thr = np.load(out + ".thresholds.npy")
    assert thr.dtype == np.float32 and thr.shape == (5,) and not np.isnan(thr).any()
    assert os.path.isfile(os.path.join(out, "model.safetensors"))
