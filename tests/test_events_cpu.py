"""Host-side parts of the event decoder on the device (include/acx.h "sound event decoding", pytorch/segments.py
decode_events_gpu / EventTable): the C ABI's argument checks, which run before anything touches a device, the table -> lists
conversion on hand-made CPU tensors, and the Python argument checks.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import segments as seg

ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -4, -5, -6
FAKE = ctypes.c_void_p(1 << 20)         # non-null, 256-byte aligned, never dereferenced: every call below fails its checks


def ws_bytes(B, N):
    out = ctypes.c_size_t()
    assert _ffi.lib().acx_events_workspace_bytes(B, N, ctypes.byref(out)) == 0
    return out.value


def test_struct_layouts():
    assert ctypes.sizeof(_ffi.AcxEvent) == 32 == _ffi.EVENT_BYTES
    assert _ffi.AcxEvent.peak.offset == 16 and _ffi.AcxEvent.mean.offset == 24
    assert ctypes.sizeof(_ffi.AcxEventParams) == 32 and _ffi.AcxEventParams.min_duration.offset == 16
    p = _ffi.event_params(0.5, None, 3, 0.1, 0.2)
    assert (p.threshold, p.low, p.median, p.min_duration, p.merge_gap) == (0.5, 0.5, 3, 0.1, 0.2)
    assert _ffi.event_params(0.7, 0.3).low == np.float32(0.3)       # rounded to fp32, as numpy compares


def test_workspace_bytes():
    l = _ffi.lib()
    out = ctypes.c_size_t()
    assert l.acx_events_workspace_bytes(1, 527, None) == ARG and "bytes" in l.acx_last_error().decode()
    assert l.acx_events_workspace_bytes(0, 527, ctypes.byref(out)) == SHAPE
    assert l.acx_events_workspace_bytes(1, 0, ctypes.byref(out)) == SHAPE
    assert l.acx_events_workspace_bytes(1, _ffi.MAX_CLASSES + 1, ctypes.byref(out)) == SHAPE
    assert l.acx_events_workspace_bytes(1 << 31, 1, ctypes.byref(out)) == UNSUPPORTED
    assert l.acx_events_workspace_bytes((1 << 31) // 9 + 1, 527, ctypes.byref(out)) == UNSUPPORTED
    assert l.acx_events_workspace_bytes((1 << 31) - 1, 64, ctypes.byref(out)) == 0
    sizes = [ws_bytes(B, N) for B in (1, 2, 64, 256) for N in (1, 64, 65, 527, 32768)]
    assert all(s % 256 == 0 and s > 0 for s in sizes)
    for B in (1, 7, 64):
        for N in (1, 64, 65, 527):
            assert ws_bytes(B, N) <= ws_bytes(B + 1, N) and ws_bytes(B, N) <= ws_bytes(B, N + 64)
    # per column one int32 count, per wave one int64 offset
    assert ws_bytes(64, 527) >= 64 * 9 * (64 * 4 + 8)


def call(varlen=False, **kw):
    """One entry point with valid arguments except those given; returns (rc, message)."""
    a = dict(probs=FAKE, ld=527, B=2, steps=31, N=527, p=_ffi.event_params(0.5, 0.3, 3), step=0.32, end=0.0, events=FAKE,
             capacity=16, count=FAKE, status=FAKE, ws=FAKE, ws_bytes=None, steps_v=[31, 7], ends_v=None)
    a.update(kw)
    l = _ffi.lib()
    params = a["p"] if a["p"] is None else ctypes.byref(a["p"])
    if varlen:
        sv = a["steps_v"]
        steps = None if sv is None else (ctypes.c_int * max(1, len(sv)))(*sv)
        ends = None if a["ends_v"] is None else (ctypes.c_double * len(a["ends_v"]))(*a["ends_v"])
        B = a["B"] if "B" in kw else (len(sv) if sv is not None else 2)
        nb = ws_bytes(max(1, min(B, 256)), 527) if a["ws_bytes"] is None else a["ws_bytes"]
        rc = l.acx_decode_events_varlen(a["probs"], a["ld"], steps, ends, B, a["N"], params, a["step"], a["events"], a["capacity"],
                                        a["count"], a["status"], a["ws"], nb, None)
    else:
        nb = ws_bytes(2, 527) if a["ws_bytes"] is None else a["ws_bytes"]
        rc = l.acx_decode_events(a["probs"], a["ld"], a["B"], a["steps"], a["N"], params, a["step"], a["end"], a["events"],
                                 a["capacity"], a["count"], a["status"], a["ws"], nb, None)
    return rc, l.acx_last_error().decode()


BAD_PARAMS = [_ffi.event_params(0.5, 0.3, 2), _ffi.event_params(0.5, 0.3, 0), _ffi.event_params(0.5, 0.3, -3),
              _ffi.event_params(0.5, 0.3, _ffi.MAX_EVENT_MEDIAN + 2), _ffi.event_params(0.5, 0.6, 1),
              _ffi.event_params(0.5, -0.1, 1), _ffi.event_params(0.5, float("nan"), 1),
              _ffi.event_params(0.5, 0.3, 1, min_duration=-1e-9), _ffi.event_params(0.5, 0.3, 1, merge_gap=-1.0)]


@pytest.mark.parametrize("varlen", [False, True])
def test_argument_errors(varlen):
    for name in ("probs", "p", "events", "count", "status", "ws"):
        rc, msg = call(varlen, **{name: None})
        assert rc == ARG and "null" in msg, name
    for p in BAD_PARAMS:
        assert call(varlen, p=p)[0] == ARG
    assert call(varlen, p=_ffi.event_params(0.5, 0.5, _ffi.MAX_EVENT_MEDIAN), ws_bytes=0)[0] == WORKSPACE   # the widest passes
    for step in (0.0, -0.32, float("nan")):
        assert call(varlen, step=step)[0] == ARG
    assert call(varlen, capacity=-1)[0] == ARG
    assert call(varlen, N=0)[0] == SHAPE and call(varlen, N=_ffi.MAX_CLASSES + 1)[0] == SHAPE
    assert call(varlen, ld=526)[0] == SHAPE
    # reaching the workspace checks means every argument check has passed
    rc, msg = call(varlen, ws_bytes=ws_bytes(2, 527) - 256)
    assert rc == WORKSPACE and "needed" in msg
    rc, msg = call(varlen, ws=ctypes.c_void_p((1 << 20) + 64))
    assert rc == WORKSPACE and "aligned" in msg
    # an argument error outranks a shape error, a shape error the workspace
    assert call(varlen, p=BAD_PARAMS[0], N=0, ws_bytes=0)[0] == ARG
    assert call(varlen, N=0, ws_bytes=0)[0] == SHAPE


def test_uniform_shape_errors():
    assert call(steps=0)[0] == SHAPE and call(steps=-5)[0] == SHAPE
    assert call(B=0)[0] == SHAPE and call(B=-1)[0] == SHAPE
    rc, msg = call(B=1 << 31, N=64, ld=64, ws_bytes=1 << 40)
    assert rc == UNSUPPORTED and "workgroups" in msg


def test_varlen_shape_errors():
    assert call(True, steps_v=None)[0] == ARG
    assert call(True, steps_v=[31, 0])[0] == SHAPE and call(True, steps_v=[-1, 3])[0] == SHAPE
    assert call(True, steps_v=[3], B=0)[0] == SHAPE
    assert call(True, steps_v=[3] * 257)[0] == SHAPE
    assert call(True, steps_v=[3] * 256, ws_bytes=0)[0] == WORKSPACE


# ---- EventTable on hand-made CPU tensors ------------------------------------------------------------------------------------

def make_table(rows, capacity=None, count=None, status=0, edges=None, classes=5):
    """rows: (clip, cls, begin, end, peak, mean)"""
    cap = len(rows) if capacity is None else capacity
    buf = np.zeros((max(cap, 1), 8), dtype=np.int32)
    for i, (clip, cls, b, e, peak, mean) in enumerate(rows[:cap]):
        buf[i, :4] = (clip, cls, b, e)
        buf[i:i + 1].view(np.float32)[0, 4] = peak
        buf[i:i + 1].view(np.float64)[0, 3] = mean
    return seg.EventTable(torch.from_numpy(buf), torch.tensor([len(rows) if count is None else count]),
                          torch.tensor([status], dtype=torch.int32), edges, classes)


def test_event_table_views_and_lists():
    e0 = seg.segment_edges(90000)               # 9 segments, the last boundary at 2.8125 s instead of 2.88
    e1 = np.arange(4, dtype=np.float64) * 0.01
    assert e0.shape == (10,) and e0[9] == 2.8125
    rows = [(0, 1, 0, 2, 0.9, 0.8), (0, 1, 5, 9, 0.75, 0.7), (0, 3, 0, 2, 0.6, 0.55), (0, 4, 0, 1, 0.99, 0.99),
            (1, 0, 1, 3, 0.5, 0.5), (1, 2, 0, 3, 0.625, 0.6)]
    t = make_table(rows, edges=[e0, e1])
    assert len(t) == 6 and t.capacity == 6
    assert t.clip.tolist() == [0, 0, 0, 0, 1, 1] and t.cls.tolist() == [1, 1, 3, 4, 0, 2]
    assert t.begin.tolist() == [0, 5, 0, 0, 1, 0] and t.end.tolist() == [2, 9, 2, 1, 3, 3]
    assert t.peak.dtype == torch.float32 and t.peak.tolist() == [np.float32(r[4]) for r in rows]
    assert t.mean.dtype == torch.float64 and t.mean.tolist() == [r[5] for r in rows]
    got = t.to_lists()
    # decode_events' key: (onset, offset, str(class)); the free last boundary is the offset of an event that ends with the clip
    assert got[0] == [(4, 0.0, float(e0[1]), float(np.float32(0.99)), 0.99), (1, 0.0, float(e0[2]), float(np.float32(0.9)), 0.8),
                      (3, 0.0, float(e0[2]), float(np.float32(0.6)), 0.55), (1, float(e0[5]), 2.8125, 0.75, 0.7)]
    assert got[1] == [(2, 0.0, float(e1[3]), 0.625, 0.6), (0, float(e1[1]), float(e1[3]), 0.5, 0.5)]
    labels = ["b", "a", "10", "9", "c"]
    named = t.to_lists(labels)
    assert [ev[0] for ev in named[0]] == ["c", "9", "a", "a"]        # "9" < "a": the key sorts the label's string
    assert [ev[0] for ev in named[1]] == ["10", "b"]
    with pytest.raises(ValueError, match="4 labels for 5 classes"):
        t.to_lists(labels[:4])


def test_event_table_status():
    edges = [np.arange(4, dtype=np.float64) * 0.32]
    with pytest.raises(ValueError, match="NaN"):
        make_table([], status=_ffi.EVENTS_NONFINITE, edges=edges).to_lists()
    with pytest.raises(ValueError, match="NaN"):
        len(make_table([], status=_ffi.EVENTS_NONFINITE, edges=edges))
    # an overflowed table without a way to decode again says so; with one, it is decoded once at the exact size
    rows = [(0, c, 0, 1, 0.5, 0.5) for c in range(4)]
    with pytest.raises(ValueError, match="4 events for a table of 2 rows"):
        make_table(rows, capacity=2, status=_ffi.EVENTS_OVERFLOW, edges=edges).check()
    t = make_table(rows, capacity=2, status=_ffi.EVENTS_OVERFLOW, edges=edges)
    asked = []

    def rerun(cap):
        asked.append(cap)
        full = make_table(rows, edges=edges)
        return full.table, full.count, full.status
    t._rerun = rerun
    assert len(t) == 4 and asked == [4] and t.capacity == 4 and t.cls.tolist() == [0, 1, 2, 3]
    assert len(t.to_lists()[0]) == 4 and asked == [4]
    assert make_table([], edges=edges).to_lists() == [[]]


# ---- decode_events_gpu: what it refuses before it touches a device -------------------------------------------------------------

def test_decode_events_gpu_refusals():
    p = torch.rand(31, 7)
    with pytest.raises(ValueError, match="CUDA"):
        seg.decode_events_gpu(p)
    with pytest.raises(ValueError, match="CUDA"):
        seg.decode_events_gpu(p.numpy())
    with pytest.raises(ValueError, match="CUDA"):
        seg.decode_events_gpu([p, p[:4]])
    with pytest.raises(ValueError, match="CUDA|float32"):
        seg.decode_events_gpu(p.double())
    with pytest.raises(ValueError, match="odd positive integer"):
        seg.decode_events_gpu(p, median=4)
    with pytest.raises(ValueError, match="odd positive integer"):
        seg.decode_events_gpu(p, median=3.0)
    with pytest.raises(ValueError, match="at most 101"):
        seg.decode_events_gpu(p, median=103)
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\]"):
        seg.decode_events_gpu(p, threshold=0.5, low=0.6)
    with pytest.raises(ValueError, match="must not be negative"):
        seg.decode_events_gpu(p, merge_gap=-0.1)
    with pytest.raises(ValueError, match="step must be positive"):
        seg.decode_events_gpu(p, step=0.0)
    with pytest.raises(ValueError, match="capacity"):
        seg.decode_events_gpu(p, capacity=-1)
    with pytest.raises(ValueError, match="shape"):
        seg.decode_events_gpu(torch.rand(7))
    # boundaries: the count, then the form
    with pytest.raises(ValueError, match="31 boundaries for 31 steps"):
        seg.decode_events_gpu(p, step=np.arange(31) * 0.32)
    uneven = np.arange(32) * 0.32
    uneven[5] += 0.01
    for edges in (uneven, np.arange(32) * 0.32 + 1.0, np.linspace(0.0, 1.0, 32) ** 2):
        with pytest.raises(ValueError, match="only uniform steps with a free last boundary run on the GPU"):
            seg.decode_events_gpu(p, step=edges)
    with pytest.raises(ValueError, match="only uniform steps"):
        seg.decode_events_gpu([p, p], step=[np.arange(32) * 0.32, np.arange(32) * 0.01])
    # ... while the boundaries of segment_edges pass these checks and fail on the device check only
    with pytest.raises(ValueError, match="CUDA"):
        seg.decode_events_gpu(p, step=seg.segment_edges(31 * 10240 + 4000))
    with pytest.raises(ValueError, match="at most 256 clips"):
        seg.decode_events_gpu([p] * 257)
    with pytest.raises(ValueError, match="at most 256 clips"):
        seg.decode_events_gpu(torch.rand(257, 7), steps=[1] * 257)
    with pytest.raises(ValueError, match="do not add up"):
        seg.decode_events_gpu(p, steps=[30, 2])
    with pytest.raises(ValueError, match="one class count"):
        seg.decode_events_gpu([p, torch.rand(4, 8)])


def test_check_event_args_is_decode_events_own():
    """the same messages as decode_events for the same mistakes"""
    p = np.random.default_rng(0).random((5, 3)).astype(np.float32)
    for kw in (dict(low=0.6), dict(median=2), dict(median=True), dict(min_duration=-1.0), dict(merge_gap=-1.0)):
        with pytest.raises(ValueError) as host:
            seg.decode_events(p, **kw)
        with pytest.raises(ValueError) as dev:
            seg.decode_events_gpu(torch.from_numpy(p), **kw)
        assert str(host.value) == str(dev.value)
