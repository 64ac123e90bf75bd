"""GPU (`-m gpu`): the online event decoder (pytorch/segments.py EventStream, acx_event_stream_* in include/acx.h, ConvNeXt.stream
with events=).

Correct means two things.  The rows of all calls of a recording, sorted by (clip, cls, begin), are the rows of decode_events_gpu
over the whole matrix BYTE FOR BYTE (`mean` included), for any chunking; and every call's table equals the events that the host
definition, OnlineEventDecoderHost, emits in the same call, with open_begin equal after every call."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

pytestmark = pytest.mark.gpu
STEP = seg.SEGMENT_SECONDS
SHAPES = [(3, 31, 527), (2, 97, 70), (1, 1, 1), (2, 2, 65), (1, 300, 64)]
MAIN = SHAPES[0]
ROW = np.dtype([("clip", "<i4"), ("cls", "<i4"), ("begin", "<i4"), ("end", "<i4"), ("peak", "<f4"), ("reserved", "<f4"),
                ("mean", "<f8")])
PARAMS = [dict(median=1),
          dict(median=3, low=0.3),
          dict(median=5, low=0.3, merge_gap=0.33),
          dict(median=7, low=0.0, merge_gap=0.32),
          dict(median=9, low=0.3, min_duration=0.65),
          dict(median=31, low=0.3, merge_gap=0.7, min_duration=1.0),
          dict(median=101, low=0.3, merge_gap=1.0, min_duration=0.33)]


@functools.lru_cache(maxsize=None)
def probabilities(B, S, N, seed=0):
    """tests/test_gpu_events.py's recipe.  float32 numpy, read-only."""
    g = torch.Generator().manual_seed(1234 + seed)
    z = torch.randn(B, S + 4, N, generator=g, dtype=torch.float64)
    z = (z[:, :-4] + z[:, 1:-3] + z[:, 2:-2] + z[:, 3:-1] + z[:, 4:]) / 5 ** 0.5
    p = torch.sigmoid(3.0 * (z - 0.52)).to(torch.float32)
    u = torch.rand(B, S, N, generator=g)
    p[u < 0.03] = 0.5
    p[(u >= 0.03) & (u < 0.06)] = 0.3
    tie = (u >= 0.06) & (u < 0.12)
    tie[:, 0] = False
    p[tie] = torch.roll(p, 1, dims=1)[tie]
    p = p.numpy()
    p.setflags(write=False)
    return p


def random_cuts(steps, median, seed):
    """seeded chunks of one recording: empty pushes, chunks shorter than median // 2, ordinary and long ones"""
    h = median // 2
    rng = np.random.default_rng(seed)
    cuts, left = [], steps
    while left:
        kind = rng.integers(4)
        n = 0 if kind == 0 else int(rng.integers(1, max(h, 1) + 1)) if kind == 1 else int(rng.integers(1, 2 * median + 8))
        n = min(n, left)
        cuts.append(n)
        left -= n
    if h >= 2 and steps >= 2 and not any(0 < n < h for n in cuts):
        i = max(range(len(cuts)), key=lambda k: cuts[k])
        cuts[i:i + 1] = [1, cuts[i] - 1]
    cuts.insert(int(rng.integers(len(cuts) + 1)), 0)
    return cuts


def plans_of(B, S, median, name):
    if name == "one":
        return [[S]] * B
    if name == "rows":
        return [[1] * S] * B
    return [random_cuts(S, median, 100 * S + i) for i in range(B)]           # the slots advance at different rates


def rows_of(table):
    """the valid rows of a table as (n, 8) int32"""
    n = len(table)
    return table.table[:n].cpu().numpy().reshape(n, 8)


def pack(slot, events):
    """the host definition's events of one slot as table rows"""
    a = np.zeros(len(events), dtype=ROW)
    for i, (c, b, e, peak, mean) in enumerate(events):
        a[i] = (slot, c, b, e, peak, 0.0, mean)
    return a.view("<i4").reshape(len(events), 8)


def sort_rows(rows):
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def drive(es, hosts, data, plans, ends=None, slots=None, capacity=None):
    """Push data[i] to slot slots[i] along plans[i], all slots in the same calls, then close.  Every call's table must equal
    the host definition's events of that call and open_begin must agree after it.  Returns all rows in call order."""
    B = len(plans)
    slots = list(range(B)) if slots is None else slots
    at = [0] * B
    got = []
    for k in range(max(len(p) for p in plans)):
        chunk, want = {}, []
        for i in range(B):
            if k < len(plans[i]):
                n = plans[i][k]
                chunk[slots[i]] = data[i][at[i]:at[i] + n]
                want.append(pack(slots[i], hosts[i].push(chunk[slots[i]].cpu().numpy())))
                at[i] += n
        rows = rows_of(es.push(chunk, capacity=capacity))
        assert np.array_equal(rows, np.concatenate(want)), "call %d: the table is not the host definition's" % k
        got.append(rows)
        assert np.array_equal(es.open_begin(slots).cpu().numpy(), np.stack([h.open_begin() for h in hosts])), k
        assert [es.steps(s) for s in slots] == at
    t = es.close(slots, None if ends is None else list(ends), capacity=capacity)
    rows = rows_of(t)
    want = [pack(slots[i], hosts[i].close(None if ends is None else ends[i])) for i in range(B)]
    assert np.array_equal(rows, np.concatenate(want)), "close: the table is not the host definition's"
    got.append(rows)
    assert bool((es.open_begin(slots) == -1).all()) and [es.steps(s) for s in slots] == [0] * B
    return np.concatenate(got), t


@pytest.mark.parametrize("args", PARAMS, ids=lambda a: "median%d" % a["median"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bytes_of_the_batch_call_and_the_host_definition_per_call(shape, args):
    B, S, N = shape
    p = probabilities(*shape)
    x = torch.tensor(p).cuda()
    want = rows_of(seg.decode_events_gpu(x, **args))
    es = seg.EventStream(B, N, step=STEP, **args)
    for name in ("one", "rows", "random"):
        hosts = [seg.OnlineEventDecoderHost(N, step=STEP, **args) for _ in range(B)]
        got, _ = drive(es, hosts, x, plans_of(B, S, args["median"], name))          # the handle is reused: close left it clean
        assert np.array_equal(sort_rows(got), want), name
    # a free last boundary in slot 0, the recordings' own given explicitly in the others
    ends = [(S - 1) * STEP + 0.05] + [S * STEP] * (B - 1)
    edges = []
    for e in ends:
        edges.append(np.arange(S + 1, dtype=np.float64) * STEP)
        edges[-1][S] = e
    hosts = [seg.OnlineEventDecoderHost(N, step=STEP, **args) for _ in range(B)]
    got, last = drive(es, hosts, x, plans_of(B, S, args["median"], "random"), ends=ends)
    assert np.array_equal(sort_rows(got), rows_of(seg.decode_events_gpu(x, step=edges, **args)))
    listed = last.to_lists()
    assert sorted(listed) == list(range(B))
    assert all(ev[2] in (ends[s], float(np.float64(round(ev[2] / STEP)) * STEP)) for s in listed for ev in listed[s])


@pytest.mark.parametrize("median", [1, 5, 9, 31])
def test_recordings_shorter_than_half_the_median_and_empty_ones(median):
    N, h = 70, median // 2
    es = seg.EventStream(2, N, median=median, low=0.3, merge_gap=0.33)
    assert len(es.close([0, 1])) == 0 and len(es.close()) == 0                      # empty recordings emit nothing
    n = max(h - 1, 0)
    x = torch.tensor(probabilities(2, 97, 70)[:, :max(n, 1)]).cuda()
    tables = [es.push({0: x[0, i:i + 1], 1: x[1, :0]}) for i in range(n)]
    assert all(len(t) == 0 for t in tables)                                        # no filtered row exists yet
    got = rows_of(es.close([0, 1]))
    if n:
        want = rows_of(seg.decode_events_gpu(x[0, :n], median=median, low=0.3, merge_gap=0.33))
        assert np.array_equal(got, want)
    else:
        assert len(got) == 0


def test_per_class_levels_on_the_device():
    B, S, N = MAIN
    p = probabilities(*MAIN)
    x = torch.tensor(p).cuda()
    g = torch.Generator().manual_seed(3)
    thr = (0.35 + 0.4 * torch.rand(N, generator=g)).to(torch.float32)
    thr[::17] = float("inf")                                                        # these classes emit nothing
    low = (thr * (0.5 + 0.5 * torch.rand(N, generator=g))).to(torch.float32)
    low[::17] = 0.2
    low[5] = float("inf")
    thr[5] = float("inf")
    args = dict(median=3, merge_gap=0.33, min_duration=0.33)
    want = rows_of(seg.decode_events_gpu(x, threshold=thr.cuda(), low=low.cuda(), **args))
    assert len(want) >= 200 and not np.isin(want[:, 1], np.arange(0, N, 17)).any()
    es = seg.EventStream(B, N, threshold=thr.cuda(), low=low.cuda(), step=STEP, **args)
    hosts = [seg.OnlineEventDecoderHost(N, threshold=thr.numpy(), low=low.numpy(), step=STEP, **args) for _ in range(B)]
    got, _ = drive(es, hosts, x, plans_of(B, S, 3, "random"))
    assert np.array_equal(sort_rows(got), want)
    # thresholds alone: low = each class's threshold; host arrays are copied
    es = seg.EventStream(B, N, threshold=thr.numpy(), step=STEP, **args)
    hosts = [seg.OnlineEventDecoderHost(N, threshold=thr.numpy(), step=STEP, **args) for _ in range(B)]
    got, _ = drive(es, hosts, x, plans_of(B, S, 3, "random"))
    assert np.array_equal(sort_rows(got), rows_of(seg.decode_events_gpu(x, threshold=thr.cuda(), **args)))
    # a bad level is refused at create
    for bad_thr, bad_low in ((0.5, 0.6), (float("nan"), 0.1), (0.5, -0.1)):
        t, l = thr.clone(), low.clone()
        t[100], l[100] = bad_thr, bad_low
        with pytest.raises(ValueError, match="low must be in"):
            seg.EventStream(B, N, threshold=t.cuda(), low=l.cuda(), **args)
    h = ctypes.c_void_p(5)
    t = thr.clone()
    t[3] = float("nan")
    dev = t.cuda()
    params = _ffi.event_params(median=3)
    rc = _ffi.lib().acx_event_stream_create(B, N, ctypes.byref(params), STEP, dev.data_ptr(), None, ctypes.byref(h))
    assert rc == -1 and h.value is None and "class 3" in _ffi.lib().acx_last_error().decode()


class Raw:
    """the C calls on a handle of their own, with tables the test owns"""

    def __init__(self, slots, N, step=STEP, **kw):
        self.lib, self.N = _ffi.lib(), N
        self.h = ctypes.c_void_p()
        params = _ffi.event_params(**kw)
        _ffi.check(self.lib.acx_event_stream_create(slots, N, ctypes.byref(params), step, None, None, ctypes.byref(self.h)))

    def __del__(self):
        self.lib.acx_event_stream_destroy(self.h)

    def call(self, slot, x=None, rows=None, ends=None, capacity=4096, fill=0):
        table = torch.full((max(capacity, 1), 8), fill, dtype=torch.int32, device="cuda")
        count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        n = len(slot)
        c_slot = (ctypes.c_int * n)(*slot)
        stream = _ffi.stream_ptr(table.device)
        if rows is not None:
            rc = self.lib.acx_event_stream_push(self.h, None if x is None else x.data_ptr(), self.N, c_slot,
                                                (ctypes.c_int * n)(*rows), n, table.data_ptr(), capacity, count.data_ptr(),
                                                status.data_ptr(), stream)
        else:
            rc = self.lib.acx_event_stream_close(self.h, c_slot, None if ends is None else (ctypes.c_double * n)(*ends), n,
                                                 table.data_ptr(), capacity, count.data_ptr(), status.data_ptr(), stream)
        torch.cuda.synchronize()
        return rc, int(count.cpu()), int(status.cpu()), table.cpu().numpy()

    def steps(self, slot):
        n = ctypes.c_int64()
        _ffi.check(self.lib.acx_event_stream_steps(self.h, slot, ctypes.byref(n)))
        return n.value

    def undo(self, slot):
        _ffi.check(self.lib.acx_event_stream_undo(self.h, (ctypes.c_int * len(slot))(*slot), len(slot)))


def test_void_calls_change_nothing():
    B, S, N = MAIN
    args = dict(median=3, low=0.3, merge_gap=0.33)
    p = probabilities(*MAIN)
    x = torch.tensor(p).cuda().contiguous()
    hosts = [seg.OnlineEventDecoderHost(N, step=STEP, **args) for _ in range(B)]
    first = np.concatenate([pack(i, hosts[i].push(p[i, :20])) for i in range(B)])
    assert len(first) > 1
    a, b = Raw(B, N, **args), Raw(B, N, **args)                     # b never sees a void call
    head, tail = x[:, :20].contiguous(), x[:, 20:].contiguous()
    rc, count, status, table = a.call([0, 1, 2], head, [20] * B, capacity=1, fill=-3)
    assert rc == 0 and status == _ffi.EVENTS_OVERFLOW and count == len(first)
    assert (table == -3).all(), "a void call writes no row"
    assert [a.steps(s) for s in range(B)] == [20] * B
    a.undo([0, 1, 2])
    assert [a.steps(s) for s in range(B)] == [0] * B
    # a NaN row: void as well
    bad = head.clone()
    bad[1, 7, 300] = float("nan")
    rc, count, status, table = a.call([0, 1, 2], bad, [20] * B, fill=-3)
    assert rc == 0 and status == _ffi.EVENTS_NONFINITE and count == 0 and (table == -3).all()
    a.undo([0, 1, 2])
    # a row of the rows that no filtered row reads yet holds an infinity
    one = head[:, :1].clone()
    one[2, 0, 526] = float("-inf")
    rc, count, status, table = a.call([0, 1, 2], one, [1] * B)
    assert rc == 0 and status == _ffi.EVENTS_NONFINITE and count == 0
    a.undo([0, 1, 2])
    # the same push with room, and everything after it, is the run that never saw a void call
    for h in (a, b):
        h.out = [h.call([0, 1, 2], head, [20] * B), h.call([0, 1, 2], tail, [S - 20] * B), h.call([0, 1, 2])]
    for ra, rb in zip(a.out, b.out):
        assert ra[:3] == rb[:3] and ra[2] == 0 and np.array_equal(ra[3], rb[3])
    assert np.array_equal(a.out[0][3][:len(first)], first)
    got = np.concatenate([r[3][:r[1]] for r in a.out])
    assert np.array_equal(sort_rows(got), rows_of(seg.decode_events_gpu(x, **args)))
    # a void close leaves the recordings open
    rc, count, status, _ = a.call([0, 1, 2], head, [20] * B)
    want = a.call([0, 1, 2], head, [0] * B)[1:3]
    assert want == (0, 0)
    rc, count, status, table = a.call([0, 1, 2], capacity=0, fill=-3)
    assert status == _ffi.EVENTS_OVERFLOW and count > 0 and (table == -3).all()
    a.undo([0, 1, 2])
    assert [a.steps(s) for s in range(B)] == [20] * B
    rc, count2, status, table = a.call([0, 1, 2])
    b.call([0, 1, 2], head, [20] * B)
    assert status == 0 and count2 == count and np.array_equal(table, b.call([0, 1, 2])[3])


def test_event_stream_reissues_a_small_table_and_survives_a_nan():
    B, S, N = MAIN
    args = dict(median=3, low=0.3, merge_gap=0.33)
    p = probabilities(*MAIN)
    x = torch.tensor(p).cuda()
    want = rows_of(seg.decode_events_gpu(x, **args))
    es = seg.EventStream(B, N, step=STEP, **args)
    hosts = [seg.OnlineEventDecoderHost(N, step=STEP, **args) for _ in range(B)]
    got, _ = drive(es, hosts, x, [[7, 13, 11]] * B, capacity=1)                    # every call overflows and is issued again
    assert np.array_equal(sort_rows(got), want)
    # an unchecked table is checked by the next call on the handle
    t1 = es.push({0: x[0, :20]}, capacity=1)
    t2 = es.push({0: x[0, 20:]})
    assert t1._n is not None and t1.capacity == len(t1) > 1 and es.steps(0) == S
    rest = es.close()
    assert np.array_equal(sort_rows(np.concatenate([rows_of(t) for t in (t1, t2, rest)])), want[want[:, 0] == 0])
    # a NaN: ValueError when the table is read, and the push has not happened
    bad = x[1, :20].clone()
    bad[3, 64] = float("nan")
    start = es.push({1: x[1, :5]})
    t = es.push({1: bad})
    with pytest.raises(ValueError, match="NaN or an infinity"):
        len(t)
    assert es.steps(1) == 5
    more = [start, es.push({1: x[1, 5:]}), es.close([1])]
    rows = np.concatenate([rows_of(m) for m in more])
    assert np.array_equal(sort_rows(rows), want[want[:, 0] == 1])


def test_slot_reuse_equals_a_fresh_handle():
    B, S, N = 2, 97, 70
    args = dict(median=5, low=0.3, merge_gap=0.33, min_duration=0.33)
    x = torch.tensor(probabilities(B, S, N)).cuda()
    es = seg.EventStream(4, N, step=STEP, **args)
    es.push({3: x[0, :50]})
    es.close([3])                                                                   # recording 0 ends early in slot 3
    es.push({1: x[0, :9]})                                                          # slot 1 stays open beside it
    again = [es.push({3: x[1, :40]}), es.push({3: x[1, 40:]}), es.close([3])]
    fresh = seg.EventStream(1, N, step=STEP, **args)
    ref = [fresh.push(x[1, :40]), fresh.push(x[1, 40:]), fresh.close()]
    for a, b in zip(again, ref):
        ra, rb = rows_of(a), rows_of(b)
        assert (ra[:, 0] == 3).all() and np.array_equal(ra[:, 1:], rb[:, 1:])
    assert sum(len(t) for t in ref) > 20 and es.steps(1) == 9 and es.steps(3) == 0


def test_300_slots_in_one_push():
    n, N, S = 300, 5, 12
    args = dict(median=3, low=0.3)
    p = probabilities(n, S, N)
    x = torch.tensor(p).cuda()
    es = seg.EventStream(n, N, step=STEP, **args)
    packed = x[:, :8].reshape(n * 8, N)
    t1 = es.push(packed, slots=list(range(n)), steps=[8] * n)                        # two device calls: 256 + 44 slots
    assert len(t1._parts) == 2
    t2 = es.push({s: x[s, 8:] for s in reversed(range(n))}, capacity=3)              # both parts overflow and run again
    t3 = es.close()
    got = np.concatenate([rows_of(t) for t in (t1, t2, t3)])
    want = rows_of(seg.decode_events_gpu(x, **args))
    assert len(want) > n and np.array_equal(sort_rows(got), want)
    assert sorted(t3.to_lists()) == list(range(n))


def test_two_handles_on_two_torch_streams():
    B, S, N = MAIN
    args = dict(median=5, low=0.3, merge_gap=0.33)
    x = torch.tensor(probabilities(*MAIN)).cuda()
    y = torch.tensor(probabilities(*MAIN, seed=1)).cuda()
    torch.cuda.synchronize()
    handles = [seg.EventStream(B, N, step=STEP, **args) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    tables = [[], []]
    for lo, hi in ((0, 9), (9, 10), (10, 31)):
        for k, data in enumerate((x, y)):
            with torch.cuda.stream(streams[k]):
                tables[k].append(handles[k].push({i: data[i, lo:hi] for i in range(B)}))
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            tables[k].append(handles[k].close())
    torch.cuda.synchronize()
    for k, data in enumerate((x, y)):
        got = np.concatenate([rows_of(t) for t in tables[k]])
        assert np.array_equal(sort_rows(got), rows_of(seg.decode_events_gpu(data, **args)))


def test_capturable():
    """the launch contract: no allocation, no synchronisation after create -- a push replays from a graph with the same bits"""
    B, S, N = MAIN
    args = dict(median=3, low=0.3)
    x = torch.tensor(probabilities(*MAIN)).cuda().contiguous()
    eager = Raw(B, N, **args).call([0, 1, 2], x, [S] * B)
    h = Raw(B, N, **args)
    table = torch.zeros((4096, 8), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    c_slot, c_rows = (ctypes.c_int * B)(0, 1, 2), (ctypes.c_int * B)(*[S] * B)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        rc = h.lib.acx_event_stream_push(h.h, x.data_ptr(), N, c_slot, c_rows, B, table.data_ptr(), 4096, count.data_ptr(),
                                         status.data_ptr(), _ffi.stream_ptr(x.device))
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert int(count.cpu()) == eager[1] > 100 and int(status.cpu()) == 0 and np.array_equal(table.cpu().numpy(), eager[3])


def test_argument_errors_on_a_handle():
    h = Raw(2, 8, median=3)
    lib, err = h.lib, lambda: _ffi.lib().acx_last_error().decode()
    x = torch.zeros((4, 8), device="cuda")
    assert h.call([0, 0], x, [2, 2])[0] == -1 and "twice" in err()
    assert h.call([2], x, [4])[0] == -1 and "out of range" in err()
    assert h.call([0], x, [-1])[0] == -1 and "rows" in err()
    assert h.call([0], None, [4])[0] == -1 and "probs" in err()
    assert h.call([0], x, [4], capacity=-1)[0] == -1 and "capacity" in err()
    assert h.call([], x, [])[0] == -1 and "expected 1 .." in err()
    assert h.call([1, 1])[0] == -1 and "twice" in err()
    one = (ctypes.c_int * 1)(0)
    t = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    rc = lib.acx_event_stream_push(h.h, x.data_ptr(), 7, one, (ctypes.c_int * 1)(4), 1, t.data_ptr(), 1, t.data_ptr(),
                                   t.data_ptr(), None)
    assert rc == -4 and "stride" in err()
    assert h.steps(0) == 0 and h.call([0, 1])[1:3] == (0, 0), "no refused call touched the handle"
    es = seg.EventStream(2, 8)
    with pytest.raises(ValueError, match="listed twice"):
        es.close([1, 1])
    with pytest.raises(ValueError, match="out of range"):
        es.push({2: x})
    with pytest.raises(ValueError, match="add up"):
        es.push(x, slots=[0, 1], steps=[1, 2])
    with pytest.raises(ValueError, match="float32"):
        es.push(x.double())
    with pytest.raises(ValueError, match="CUDA"):
        es.push(x.cpu())


# ---- ConvNeXt.stream(events=...) ----------------------------------------------------------------------------------------------

SR = 32000
W, H = 320000, 32000


@pytest.fixture(scope="module")
def model():
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth.synth_state_dict(0))
    return m.to("cuda").eval()


def run_stream(st, recs, rng, max_push):
    """test_gpu_stream.py's driver: every recording in seeded random chunks, all slots interleaved, then one close"""
    plans = []
    for r in recs:
        out, pos = [], 0
        while pos < r.numel():
            c = min(rng.choice([0, 1, 4099, 31991, 65537, rng.randrange(1, 3 * max_push), 2 * max_push + 13]), r.numel() - pos)
            out.append(c)
            pos += c
        plans.append(out)
    offs = [0] * len(recs)
    results = []
    for step in range(max(len(p) for p in plans)):
        chunks = {}
        for i, p in enumerate(plans):
            if step < len(p):
                chunks[i] = recs[i][offs[i]:offs[i] + p[step]]
                offs[i] += p[step]
        results.append(st.push(chunks))
    results.append(st.close())
    return results


@pytest.mark.parametrize("source,rate", [("windows", None), ("timeline", None), ("timeline", 44100), ("windows", 16000)])
def test_model_stream_events(model, source, rate):
    in_rate = SR if rate is None else rate
    lengths = [int(sec * in_rate) + extra for sec, extra in ((25, 7), (31.5, 0), (40, 1234))]
    recs = [synth.synth_waveforms(1, L, seed=61 + i)[0].cuda() for i, L in enumerate(lengths)]
    refs = [model.forward_windows(r, window=W / SR, hop=H / SR, sample_rate=rate) for r in recs]
    key = "timeline" if source == "timeline" else "clipwise_output"
    every = torch.cat([r[key] for r in refs])
    N = every.shape[1]
    thr, low = torch.quantile(every, 0.6, dim=0), torch.quantile(every, 0.4, dim=0)       # seeded weights still give events
    args = dict(threshold=thr, low=low, median=3)
    st = model.stream(slots=len(recs), window=W / SR, hop=H / SR, sample_rate=rate, max_push=4.0, events=args,
                      event_source=source)
    results = run_stream(st, recs, random.Random(in_rate + len(source)), 4 * in_rate)
    assert all("events" in d and d["events_open"].dtype == torch.int32 for d in results)
    assert bool((results[-1]["events_open"] == -1).all())
    got = sort_rows(np.concatenate([rows_of(d["events"]) for d in results]))
    inside = set()
    for i, ref in enumerate(refs):
        n = ref[key].shape[0]
        if source == "timeline":
            edges = np.arange(n + 1, dtype=np.float64) * (H / SR)
            edges[n] = lengths[i] / in_rate                          # the end of the original audio
            want = rows_of(seg.decode_events_gpu(ref[key], step=edges, **args))
        else:
            want = rows_of(seg.decode_events_gpu(ref[key], step=H / SR, **args))
        mine = got[got[:, 0] == i]
        assert len(want) > 0 and np.array_equal(mine[:, 1:], want[:, 1:]), (source, rate, i)
        inside |= set(want[(want[:, 2] > 0) & (want[:, 3] < n), 1].tolist())
    assert len(inside) >= N / 4, "%d of %d classes hold an event with both ends inside a recording" % (len(inside), N)
    listed = results[-1]["events"].to_lists()
    assert sorted(listed) == list(range(len(recs)))
    if source == "timeline":                                         # an event still open at the end reaches to the audio's end
        assert any(ev[2] == lengths[s] / in_rate for s in listed for ev in listed[s])


def test_model_stream_without_events_is_unchanged(model):
    recs = [synth.synth_waveforms(1, L, seed=71 + i)[0].cuda() for i, L in enumerate((25 * SR + 5, W - 3))]
    plain = run_stream(model.stream(slots=2, window=W / SR, hop=H / SR), recs, random.Random(5), 2 * SR)
    none = run_stream(model.stream(slots=2, window=W / SR, hop=H / SR, events=None), recs, random.Random(5), 2 * SR)
    keys = {"slot", "starts", "short", "clipwise_logits", "clipwise_output", "timeline", "timeline_slot", "timeline_step"}
    for a, b in zip(plain, none):
        assert set(a) == set(b) == keys
        assert all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in keys)
    with pytest.raises(ValueError, match="what='logits'"):
        model.stream(slots=1, what="scene", events={})
    with pytest.raises(ValueError, match="needs a timeline"):
        model.stream(slots=1, timeline=None, events={}, event_source="timeline")
    with pytest.raises(TypeError, match="decode_events'"):
        model.stream(slots=1, events={"step": 0.5})
    # a short recording closes an empty event recording, and the slot is clean afterwards
    st = model.stream(slots=1, window=W / SR, hop=H / SR, events=dict(threshold=0.0))
    st.push({0: recs[0][:_ffi.MIN_SAMPLES - 1]})
    d = st.close()
    assert d["short"] == [0] and len(d["events"]) == 0
    d = [st.push({0: recs[1]}), st.close()]
    assert sum(len(x["events"]) for x in d) == d[1]["clipwise_output"].shape[1]           # threshold 0: one event per class
