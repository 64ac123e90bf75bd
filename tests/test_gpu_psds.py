"""GPU (`-m gpu`): the intersection criteria and PSDS on the device (pytorch/sed_metrics.py intersection_based_metrics /
cross_trigger_rate / psds, ConvNeXt.score_events(metric="intersection") / ConvNeXt.psds, include/acx.h "sound event scoring,
intersection criteria") against the host definitions intersection_based_metrics_host / psds_host / psd_roc_host.

Counts, cross-trigger matrix, est_relevant and ref_hit are integers and must be EQUAL.  The PSDS value and its curve come from the
same host code on equal integers and on rates summed in one stated order, so they must be equal too (==, no tolerance).  The
generated cases (tests/psds_cases.py) are asserted to hold hits, false alarms, misses and cross triggers."""
import functools

import numpy as np
import pytest
import torch

import psds_cases as pc
import sed_cases as sc
from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import sed_metrics as sm
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

pytestmark = pytest.mark.gpu
IDS = lambda s: "x".join(map(str, s))          # noqa: E731


def full_capacity(B, S, N):
    return B * N * ((S + 1) // 2) + 1


@functools.lru_cache(maxsize=None)
def generated(B, S, N):
    """(table, reference on the device, reference lists, estimated lists) of one generated case; the table has spare rows"""
    p = sc.probabilities(B, S, N)
    table = seg.decode_events_gpu(torch.tensor(p).cuda(), capacity=full_capacity(B, S, N), **pc.decode_args())
    est = table.to_lists()
    ref = sc.make_reference(est, [float(e[-1]) for e in table.edges], N, pc.STEP)
    return table, sm.ReferenceEvents.from_lists(ref, N, device="cuda"), ref, est


def check(table, reference, ref, est, N, **criteria):
    """the device scores of a table that is ready (or not yet read) against the host definition on the lists"""
    got = sm.intersection_based_metrics(reference, table, **criteria)
    host = sm.intersection_based_metrics_host(ref, est, N, **criteria)
    n = len(table)
    assert got.kind == "intersection" and got.counts.dtype == got.est_relevant.dtype == got.ref_hit.dtype == torch.int64
    assert np.array_equal(got.counts.cpu().numpy(), host.counts), (got.counts.sum(0).tolist(), host.counts.sum(0).tolist())
    rel = got.est_relevant.cpu().numpy()
    assert rel.shape == (table.capacity,) and np.array_equal(rel[:n], host.est_relevant) and np.all(rel[n:] == -1)
    assert np.array_equal(got.ref_hit.cpu().numpy(), host.ref_hit)
    assert (got.cross_triggers is None) == (host.cross_triggers is None)
    if host.cross_triggers is not None:
        assert got.cross_triggers.dtype == torch.int64 and np.array_equal(got.cross_triggers.cpu().numpy(), host.cross_triggers)
    assert np.array_equal(got.counts_host(), host.counts) and np.array_equal(got.f1, host.f1)
    return host


@pytest.mark.parametrize("scenario", sorted(pc.CRITERIA))
@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_generated_cases(shape, scenario):
    table, reference, ref, est = generated(*shape)
    assert len(table) < table.capacity
    host = sm.intersection_based_metrics_host(ref, est, shape[2], **pc.CRITERIA[scenario])
    pc.needs_every_count(shape, scenario, host)
    check(table, reference, ref, est, shape[2], **pc.CRITERIA[scenario])


def hand_table(case):
    """the EventTable of a hand-worked case, built row by row, with two spare rows"""
    rows = [(i, c, b, e) for i, events in enumerate(case["est"]) for c, b, e in events]
    table = torch.zeros((len(rows) + 2, _ffi.EVENT_BYTES // 4), dtype=torch.int32)
    if rows:
        table[:len(rows), :4] = torch.tensor(rows, dtype=torch.int32)
    table[len(rows):] = -1
    meta = torch.zeros(4, dtype=torch.int32).cuda()
    count, status = meta[:2].view(torch.int64), meta[2:3]
    count.fill_(len(rows))
    return seg.EventTable(table.cuda(), count, status, [pc.edges(case, i) for i in range(len(case["est"]))], case["classes"])


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c["name"])
def test_cases_by_hand(case):
    table = hand_table(case)
    reference = sm.ReferenceEvents.from_lists(case["ref"], case["classes"], device="cuda")
    got = sm.intersection_based_metrics(reference, table, **case["args"])
    assert got.counts.cpu().tolist() == case["counts"]
    assert got.est_relevant.cpu().tolist() == case["est_relevant"] + [-1] * 2 and got.ref_hit.cpu().tolist() == case["ref_hit"]
    assert (got.cross_triggers is None) == (case["cross"] is None)
    if case["cross"] is not None:
        assert got.cross_triggers.cpu().tolist() == case["cross"]


def test_varlen_table_with_clip_ends():
    N, steps = 65, [31, 1, 97]
    p = sc.probabilities(1, sum(steps), N, seed=3)[0]
    clips = list(np.split(p, np.cumsum(steps)[:-1]))
    edges = [seg.segment_edges(10240 * s + 4000) for s in steps]                 # the last boundary past s * 0.32
    step = seg.SEGMENT_SECONDS
    assert all(len(e) == s + 1 and e[-1] != s * step for e, s in zip(edges, steps))
    table = seg.decode_events_gpu([torch.tensor(c).cuda() for c in clips], step=edges, capacity=full_capacity(1, sum(steps), N),
                                  threshold=0.5, low=0.3, median=3)
    est = table.to_lists()
    ends = [float(e[-1]) for e in edges]
    assert any(ev[2] == ends[i] for i, events in enumerate(est) for ev in events), "an event ends on a moved last boundary"
    ref = sc.make_reference(est, ends, N, step, seed=3)
    reference = sm.ReferenceEvents.from_lists(ref, N, device="cuda")
    for criteria in pc.CRITERIA.values():
        host = check(table, reference, ref, est, N, **criteria)
        assert host.counts.sum(axis=0).min() > 0


def test_one_side_empty():
    B, S, N = 3, 31, 64
    table, reference, ref, est = generated(B, S, N)
    none = sm.ReferenceEvents.from_lists([[]] * B, N, device="cuda")
    host = check(table, none, [[]] * B, est, N, **pc.CRITERIA["dcase_2"])
    assert host.counts[:, 1].sum() == len(table) and host.counts[:, [0, 2]].sum() == 0 and host.cross_triggers.sum() == 0
    silent = seg.decode_events_gpu(torch.tensor(sc.probabilities(B, S, N)).cuda(), **pc.decode_args(2.0))
    assert len(silent) == 0
    host = check(silent, reference, ref, [[]] * B, N, **pc.CRITERIA["dcase_2"])
    assert host.counts[:, 2].sum() == len(reference) and host.counts[:, :2].sum() == 0
    check(silent, none, [[]] * B, [[]] * B, N, **pc.CRITERIA["dcase_1"])


def test_overflowed_table():
    B, S, N = 3, 31, 64
    _, reference, ref, est = generated(B, S, N)
    table = seg.decode_events_gpu(torch.tensor(sc.probabilities(B, S, N)).cuda(), capacity=16, **pc.decode_args())
    s = sm.intersection_based_metrics(reference, table, **pc.CRITERIA["dcase_2"])            # before check()
    assert int(s.status.cpu()) == _ffi.SCORE_BAD_TABLE
    assert int(s.counts.abs().sum()) == 0 and int(s.cross_triggers.abs().sum()) == 0 and int(s.ref_hit.abs().sum()) == 0
    assert bool((s.est_relevant == -1).all())
    with pytest.raises(ValueError, match="not usable when it was scored"):
        s.check()
    table.check()                                                # decodes again at the exact size
    check(table, reference, ref, est, N, **pc.CRITERIA["dcase_2"])


def test_two_calls_give_the_same_bits():
    table, reference, ref, est = generated(3, 31, 527)
    a, b = (sm.intersection_based_metrics(reference, table, **pc.CRITERIA["dcase_2"]) for _ in range(2))
    for k in ("counts", "cross_triggers", "est_relevant", "ref_hit"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int(a.cross_triggers.sum()) > 0


def test_capturable_in_a_graph():
    table, reference, ref, est = generated(3, 31, 64)
    want = sm.intersection_based_metrics(reference, table, **pc.CRITERIA["dcase_2"])
    weight = torch.linspace(0.0, 2.0, 64, dtype=torch.float64).cuda()
    want_rate = sm.cross_trigger_rate(want.cross_triggers, weight)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = sm.intersection_based_metrics(reference, table, **pc.CRITERIA["dcase_2"])
        got_rate = sm.cross_trigger_rate(got.cross_triggers, weight)
    g.replay()
    torch.cuda.synchronize()
    assert int(want.counts.sum()) > 0 and float(want_rate.sum()) > 0
    for k in ("counts", "cross_triggers", "est_relevant", "ref_hit"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert torch.equal(got_rate, want_rate)


def test_queued_behind_the_decoder():
    B, S, N = 3, 31, 130
    _, reference, ref, est = generated(B, S, N)
    p = torch.tensor(sc.probabilities(B, S, N)).cuda()
    torch.cuda.synchronize()
    table = seg.decode_events_gpu(p, capacity=full_capacity(B, S, N), **pc.decode_args())
    got = sm.intersection_based_metrics(reference, table, **pc.CRITERIA["dcase_2"])          # nothing has read the table yet
    assert table._n is None
    host = sm.intersection_based_metrics_host(ref, est, N, **pc.CRITERIA["dcase_2"])
    assert np.array_equal(got.counts.cpu().numpy(), host.counts) and np.array_equal(got.cross_triggers.cpu().numpy(), host.cross_triggers)
    assert np.array_equal(got.ref_hit.cpu().numpy(), host.ref_hit)


def test_cross_trigger_rate():
    rng = np.random.default_rng(4)
    N = 130
    ct = rng.integers(0, 1000, size=(N, N)).astype(np.int64)                               # the diagonal is not zero here
    w = rng.random(N) * 1e3
    w[[0, 7, 64, 129]] = 0.0
    got = sm.cross_trigger_rate(torch.tensor(ct).cuda(), torch.tensor(w).cuda())
    assert got.dtype == torch.float64 and got.shape == (N,)
    want = pc.sequential_rate(ct, w)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(sm.cross_trigger_rate_host(ct, w), want)
    none = sm.cross_trigger_rate(torch.tensor(ct).cuda(), torch.zeros(N, dtype=torch.float64).cuda())
    assert none.cpu().tolist() == [0.0] * N
    with pytest.raises(ValueError, match="contiguous CUDA tensors"):
        sm.cross_trigger_rate(torch.tensor(ct).cuda(), torch.tensor(w, dtype=torch.float32).cuda())


THRESHOLDS = np.linspace(0.1, 0.9, 10)
SWEEP = dict(median=3, step=pc.STEP, capacity=64)             # small tables: some thresholds overflow and are decoded again


@pytest.mark.parametrize("scenario", sorted(pc.CRITERIA))
@pytest.mark.parametrize("shape", [(3, 31, 64), (3, 31, 130)], ids=IDS)
def test_psds(shape, scenario):
    B, S, N = shape
    _, reference, ref, _ = generated(B, S, N)
    p = torch.tensor(sc.probabilities(B, S, N)).cuda()
    preset = sm.PSDS_SCENARIOS[scenario]
    got = sm.psds(p, reference, THRESHOLDS, scenario=scenario, max_efpr=3000.0, unit_seconds=3600.0, **SWEEP)
    thr = THRESHOLDS.astype(np.float32)
    hosts = []
    for t in thr:
        est = seg.decode_events_gpu(p, threshold=float(t), median=3, step=pc.STEP, capacity=full_capacity(B, S, N)).to_lists()
        hosts.append(sm.intersection_based_metrics_host(ref, est, N, **pc.CRITERIA[scenario]))
    counts = np.stack([h.counts for h in hosts])
    ct = None if scenario == "dcase_1" else np.stack([h.cross_triggers for h in hosts])
    assert ct is None or ct.sum() > 0
    total, class_seconds = sm.psds_durations(ref, [S * pc.STEP] * B, N)
    args = dict(alpha_ct=preset["alpha_ct"], alpha_st=preset["alpha_st"], max_efpr=3000.0, unit_seconds=3600.0)
    want = sm.psds_host(counts, ct, total, class_seconds, **args)
    efpr, etpr, curves = sm.psd_roc_host(counts, ct, total, class_seconds, **args)
    assert isinstance(got, sm.PsdsResult) and got.counts.is_cuda and np.array_equal(got.counts.cpu().numpy(), counts)
    assert np.array_equal(got.thresholds, thr) and np.array_equal(got.seen, counts[0, :, 0] + counts[0, :, 2] > 0)
    assert got.value == want and float(got) == want and 0 < got.value < 1, (got.value, want)
    assert np.array_equal(got.efpr, efpr) and np.array_equal(got.etpr, etpr) and np.array_equal(got.class_curves, curves, equal_nan=True)
    assert len(efpr) > 5 and np.all(np.diff(efpr) > 0)


def test_sweep_event_thresholds_with_the_intersection_metric():
    B, S, N = 3, 31, 64
    _, reference, ref, _ = generated(B, S, N)
    p = torch.tensor(sc.probabilities(B, S, N)).cuda()
    thresholds = [0.5, 0.3, 0.7]
    thr, counts = sm.sweep_event_thresholds(p, reference, thresholds, metric="intersection", dtc_threshold=0.5, gtc_threshold=0.5,
                                            median=3, step=pc.STEP, capacity=64)
    assert thr.shape == (N,) and counts.shape == (3, N, 3)
    for i, t in enumerate(np.asarray(thresholds, np.float32)):
        table = seg.decode_events_gpu(p, threshold=float(t), median=3, step=pc.STEP)
        one = sm.intersection_based_metrics(reference, table, dtc_threshold=0.5, gtc_threshold=0.5)
        host = sm.intersection_based_metrics_host(ref, table.to_lists(), N, dtc_threshold=0.5, gtc_threshold=0.5)
        assert torch.equal(counts[i], one.counts) and np.array_equal(one.counts.cpu().numpy(), host.counts)
    assert int(counts.sum(dim=(0, 1)).min()) > 0


@pytest.fixture(scope="module")
def model():
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth.synth_state_dict(0))
    return m.to("cuda").eval()


def test_model_entry_points(model):
    x = synth.synth_waveforms(2, 5 * 32000, seed=11).cuda()
    N = model.num_classes
    segments = model.forward_segments(x)
    probs, step = segments["segmentwise_output"], segments["segment_edges"].numpy()
    q = np.quantile(probs.cpu().numpy(), [0.5, 0.6, 0.7, 0.8, 0.9])
    decode = dict(median=3, merge_gap=0.33)
    mid = dict(threshold=float(q[2]), capacity=full_capacity(*probs.shape), **decode)
    first = model.detect_events(x, **mid)
    est = first["events"].to_lists()
    ends = [float(e[-1]) for e in first["events"].edges]
    ref = sc.make_reference(est, ends, N, seg.SEGMENT_SECONDS, seed=2)
    reference = sm.ReferenceEvents.from_lists(ref, N, device="cuda")
    criteria = dict(dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3)

    out = model.score_events(x, reference, metric="intersection", **criteria, **mid)
    assert set(out) == set(first) | {"scores"} and out["events"].to_lists() == est
    host = sm.intersection_based_metrics_host(ref, est, N, **criteria)
    assert host.counts.sum(axis=0).min() > 0 and host.cross_triggers.sum() > 0
    assert np.array_equal(out["scores"].counts.cpu().numpy(), host.counts)
    assert np.array_equal(out["scores"].cross_triggers.cpu().numpy(), host.cross_triggers)
    assert np.array_equal(out["scores"].ref_hit.cpu().numpy(), host.ref_hit)
    assert out["scores"].micro() == host.micro()
    with pytest.raises(TypeError, match="other metric"):
        model.score_events(x, reference, metric="intersection", t_collar=0.2)
    with pytest.raises(ValueError, match="metric must be"):
        model.score_events(x, reference, metric="psds")

    psds_args = dict(alpha_ct=0.5, max_efpr=1e5, **criteria)            # alpha_st = 0: the mean curve, > 0 with any hit
    out = model.psds(x, reference, thresholds=q, **psds_args, **decode)
    assert set(out) == set(segments) | {"psds"} and torch.equal(out["segmentwise_output"], probs)
    hosts = [sm.intersection_based_metrics_host(ref, seg.decode_events_gpu(probs, threshold=float(t), step=step, **decode).to_lists(),
                                                N, **criteria) for t in q.astype(np.float32)]
    counts, ct = np.stack([h.counts for h in hosts]), np.stack([h.cross_triggers for h in hosts])
    total, class_seconds = sm.psds_durations(ref, ends, N)
    want = sm.psds_host(counts, ct, total, class_seconds, alpha_ct=0.5, max_efpr=1e5)
    assert np.array_equal(out["psds"].counts.cpu().numpy(), counts)
    assert out["psds"].value == want and 0 < want < 1, (out["psds"].value, want)
    with pytest.raises(ValueError, match="needs a cttc_threshold"):
        model.psds(x, reference, alpha_ct=0.5)
    with pytest.raises(TypeError, match="step / steps"):
        model.psds(x, reference, step=0.32)
