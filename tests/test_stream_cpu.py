"""CPU: the schedule of live streams (acx_stream_schedule, include/acx.h) against a brute-force restatement of its definition,
the sizes of a handle's device state (acx_stream_geometry: adv, C, Ch, Hw) against brute force over the geometries of
tests/stream_cases.py, and the argument checks of the C entry points and of the Python wrapper.  No device needed."""
import ctypes
import random

import numpy as np
import pytest

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import stream as stm
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

import stream_cases as sc
from stream_cases import final_table

W = 320000


def brute(rate, W, H, L, pushed, closed):
    need = final_table(rate, L)
    if closed:
        R = len(need)
        if R < _ffi.MIN_SAMPLES:
            return R, 0, 0
        return R, len(win.window_starts([R], W, H)), len(win.timeline_steps([R], W, H))
    R = int(np.searchsorted(need, pushed, side="right"))
    wins = len([j for j in range(R // H + 2) if j * H + W <= R])
    rows = len([k for k in range(R // H + 2) if k * H + H // 2 < R - W])
    return R, wins, rows


def chunking(L, rng, max_push):
    out, pos = [], 0
    while pos < L:
        c = min(L - pos, rng.choice([0, 1, 7, 997, 31991, rng.randrange(1, 3 * max_push), 2 * max_push + 13]))
        out.append(c)
        pos += c
    return out


def schedule_matches_definition(rate, W, H):
    rng = random.Random(rate * 7 + H + (W if W != 320000 else 0))
    max_push = 2 * rate
    for L32 in (W - 1, W, W + 1, W + H - 1, W + H, 10 * W + 7):
        L = L32 * rate // 32000                        # input samples
        need = final_table(rate, L)
        pushed, seen_w, seen_r = 0, 0, 0
        for c in chunking(L, rng, max_push) + [None]:
            closed = c is None
            if not closed:
                pushed += c
            R, nw, nr = stm.schedule(W, H, rate, pushed, closed)
            if closed:
                assert (R, nw, nr) == brute(rate, W, H, L, pushed, True)
                R_all = R
            else:
                assert R == int(np.searchsorted(need, pushed, side="right")), (L, pushed)
                assert nw == (R - W) // H + 1 if R >= W else nw == 0
                assert nr == len([k for k in range(max(0, R // H + 2)) if k * H + H // 2 < R - W])
            # each window and row is reported once, a row only after every window that covers its midpoint
            assert nw >= seen_w and nr >= seen_r
            for k in range(seen_r, nr):
                m = k * H + H // 2 if not closed else min(k * H + H // 2, R_all - 1)
                if not closed:
                    assert (m // H) < nw                # the last window with j H <= m is out
            seen_w, seen_r = nw, nr
        if R_all < _ffi.MIN_SAMPLES:                  # W - 1 at W = MIN_SAMPLES: the recording is short and emits nothing
            assert (seen_w, seen_r) == (0, 0)
            continue
        assert seen_w == len(win.window_starts([R_all], W, H))
        assert seen_r == len(win.timeline_steps([R_all], W, H))


@pytest.mark.parametrize("rate", [32000, 44100, 16000])
@pytest.mark.parametrize("H", [320, 32000, W])
def test_schedule_matches_definition(rate, H):
    schedule_matches_definition(rate, W, H)


@pytest.mark.parametrize("rate", [32000, 44100, 16000, 8000, 96000])
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "R"])
def test_schedule_matches_definition_geometries(name, rate):
    g = sc.GEOMETRIES[name]
    schedule_matches_definition(rate, g["W"], g["H"])


def test_schedule_open_starts_are_final_windows():
    # while open, the starts are j H; they are exactly the windows of the whole recording that lie inside R
    for H in (320, 32000, W):
        for L in (W + 5 * H + 3, 3 * W + 1):
            _, nw, _ = stm.schedule(W, H, None, L - 1, False)
            starts = win.window_starts([L], W, H)
            assert [j * H for j in range(nw)] == starts[:nw]


def test_schedule_short_and_clip():
    assert stm.schedule(W, 32000, None, _ffi.MIN_SAMPLES - 1, True) == (_ffi.MIN_SAMPLES - 1, 0, 0)
    assert stm.schedule(W, 32000, None, _ffi.MIN_SAMPLES, True) == (_ffi.MIN_SAMPLES, 1, 1)
    assert stm.schedule(W, 32000, None, W - 1, False) == (W - 1, 0, 0)
    assert stm.schedule(W, 32000, None, W - 1, True) == (W - 1, 1, 10)


def test_schedule_argument_errors():
    with pytest.raises(_ffi.AcxError):
        _ffi.stream_schedule(_ffi.MIN_SAMPLES - 1, 1, 32000, 0, False)
    with pytest.raises(_ffi.AcxError):
        _ffi.stream_schedule(W, W + 1, 32000, 0, False)
    with pytest.raises(_ffi.AcxError):
        _ffi.stream_schedule(W, 0, 32000, 0, False)
    with pytest.raises(_ffi.AcxError):
        _ffi.stream_schedule(W, 320, 0, 0, False)
    with pytest.raises(_ffi.AcxError):
        _ffi.stream_schedule(W, 320, 32000, -1, False)
    with pytest.raises(ValueError):
        stm.schedule(W, 320, 44100.5, 0, False)


def test_c_entry_points_reject_bad_arguments():
    lib = _ffi.lib()
    h = ctypes.c_void_p()
    assert lib.acx_stream_create(None, 4, W, 32000, 32000, 64000, 1, ctypes.byref(h)) == -1
    assert lib.acx_stream_push(None, None, None, None, 1, None) == -1
    assert lib.acx_stream_close(None, None, 1, None) == -1
    assert lib.acx_stream_pending(None, None, None) == -1
    n = ctypes.c_int()
    assert lib.acx_stream_next(None, 4, None, None, None, ctypes.byref(n)) == -1
    assert lib.acx_stream_forward(None, 1, 0, None, None, None, 0, None) == -1
    got = ctypes.c_int64()
    assert lib.acx_stream_timeline(None, 0, 1, None, None, None, ctypes.byref(got), None) == -1
    lib.acx_stream_destroy(None)


def test_python_wrapper_rejects_bad_arguments():
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56],
                          use_speed_perturb=False).eval()
    for kw in ({"what": "probs"}, {"timeline": "median"}, {"slots": 0}, {"slots": True}, {"max_batch": 0},
               {"max_batch": 257}, {"window": 10.00001}, {"hop": 11.0}, {"window": 0.1}, {"sample_rate": 44100.5},
               {"max_push": 1e-6}):
        with pytest.raises(ValueError):
            model.stream(**kw)
    with pytest.raises(RuntimeError):            # valid arguments, but the model is on the CPU: there is no CPU path
        model.stream(slots=2)


# ---- the sizes of a handle's device state (acx_stream_geometry) ----------------------------------------------------------------------
def test_geometry_pins_the_sizes_of_the_existing_tests():
    """W = 10 s, H = 1 s, the geometry of tests/test_gpu_stream.py: the numbers acx_stream_create computed before the sizes
    moved into one function.  32 kHz: adv = max_push, C = ceil64(W + adv), Ch = 0, Hw = (W + adv) / H + 4.  44.1 kHz: of = 441,
    nf = 320, width = 9, qmax = 447, so adv = ceil((max_push + 447 + 1 + 882) 320 / 441) + 2 and
    Ch = ceil64(max_push + 447 + 9 + 441 + 64)."""
    H = 32000
    assert _ffi.resample_geometry(44100, 32000)[:3] == (441, 320, 9)
    assert stm.geometry(W, H, None, 64000) == (64000, 384000, 0, 16)
    assert stm.geometry(W, H, 32000, 128000) == (128000, 448000, 0, 18)
    assert stm.geometry(W, H, 44100, 88200) == (64968, 385024, 89216, 16)
    assert stm.geometry(W, H, 44100, 176400) == (128968, 449024, 177408, 18)
    assert stm.geometry(W, H, 44100, 176400, timeline=False) == (128968, 449024, 177408, 0)
    assert -(-(88200 + 447 + 1 + 882) * 320 // 441) + 2 == 64968 and -(-(88200 + 447 + 9 + 441 + 64) // 64) * 64 == 89216


def test_geometry_argument_errors():
    for bad in ((_ffi.MIN_SAMPLES - 1, 1, 32000, 1, 1), (W, W + 1, 32000, 1, 1), (W, 0, 32000, 1, 1), (W, 320, 0, 1, 1),
                (W, 320, 32000, 0, 1), (W, 320, 32000, 1 << 31, 1), (W, 320, 32000, (1 << 31) - 1, 0), (W, 320, 32000, 1, 2)):
        assert _ffi.lib().acx_stream_geometry(*bad, None, None, None, None) != 0, bad
    assert _ffi.lib().acx_stream_geometry(W, 320, 32000, 1, 1, None, None, None, None) == 0
    with pytest.raises(ValueError):
        stm.geometry(W, 320, 44100.5, 1)


# The headroom the formulas carry on purpose, and how much of it this sweep can see.  Ch = ceil64(max_push + qmax + width + of + 64):
# the need is max_push + qmax + width (the oldest input of the first output that is not final), `of` covers the guard's own
# reach (it looks one period's phase and one sample further back than the band), and the + 64 is margin: the sweep's smallest
# distance between the guard and a refusal is of + 64 (65 at 8 kHz), and it is held to at least 64, so a Ch that is 64 short
# fails.  adv = ceil((max_push + qmax + 1 + 2 of) nf / of) + 2 resampling: the 2 of inputs are about 2 nf outputs of headroom,
# and the sweep's largest advance stays at least 6 below adv at every rate (96 kHz, nf = 1), so it is held to the + 2 but CANNOT
# see an adv that is short by less than that spare.  At 32 kHz adv = max_push exactly, with no headroom.
HEADROOM_CH, HEADROOM_ADV = 64, 2


def sweep_cases():
    for name, g in sc.GEOMETRIES.items():
        for rate in sc.RATES:
            yield pytest.param(name, rate, id="%s-%d" % (name, rate))


def sweep_pushes(name, rate):
    g = sc.GEOMETRIES[name]
    mps = set(sc.sweep_max_push(g["W"], g["H"], rate)) | {max(1, v * rate // 32000) for v in g["max_push"]}
    if name == "R" and rate in sc.RATE_CASES:
        mps.add(sc.RATE_CASES[rate]["max_push"])
    return sorted(mps)


@pytest.mark.parametrize("name,rate", sweep_cases())
def test_ring_and_input_history_hold_every_legal_call(name, rate):
    """adv bounds the advance of every push and every close; C holds every window pending after the call; Ch holds the oldest
    input the next output reads, and the launcher's guard lies between the two.  Every pushed count P of the first periods and a
    seeded sample of later ones (the phase of P against the period `of` and against H); chunks c: R is non-decreasing in the
    samples pushed, so c = max_push is the worst chunk for every bound, and a few smaller ones are run as well."""
    g = sc.GEOMETRIES[name]
    Wn, H = g["W"], g["H"]
    of, nf, width = (1, 1, 0) if rate == 32000 else sc.bands(rate)[:3]
    pushes = sweep_pushes(name, rate)
    rng = np.random.default_rng(rate + Wn)
    span = (2 * Wn + 3 * H) * rate // 32000 + 4 * of
    P = np.unique(np.concatenate([np.arange(0, min(span, 2 * of + 4096)), rng.integers(0, span, 3000)])).astype(np.int64)
    Ltab = int(P.max()) + max(pushes) + 1
    need = final_table(rate, Ltab)
    if rate != 32000:
        first = sc.oldest_table(rate, Ltab)
        assert np.array_equal(first, (np.arange(len(first)) // nf) * of + sc.bands(rate)[3][np.arange(len(first)) % nf] - width)

    def final(p):
        return np.searchsorted(need, p, side="right").astype(np.int64)

    R0 = final(P)
    Rc = sc.closed_length(rate, P)
    j = sc.open_windows(R0, Wn, H)                                       # the first window still to come
    for mp in pushes:
        adv, C, Ch, _ = stm.geometry(Wn, H, rate, mp)
        tag = "%s W=%d H=%d rate=%d max_push=%d (adv=%d C=%d Ch=%d)" % (name, Wn, H, rate, mp, adv, C, Ch)
        assert C >= Wn + adv, tag                                     # the launcher's "more than the ring holds" is adv > C - W
        for c in sorted({1, mp, mp // 2 + 1, max(1, mp - 1), int(rng.integers(1, mp + 1))}):
            R1 = final(P + c)
            worst = int((R1 - R0).max())
            assert worst <= adv - HEADROOM_ADV * (rate != 32000), "%s: a push of %d advances by %d" % (tag, c, worst)
            has = sc.open_windows(R1, Wn, H) > j
            short = int((j * H - (R1 - C))[has].min()) if has.any() else 0
            assert short >= 0, "%s: a window pending after a push of %d starts %d samples behind the ring" % (tag, c, -short)
            if rate != 32000:
                out = R1 > R0
                old = np.maximum(first[R0[out]], 0)
                room = int((old - (P[out] + c - Ch)).min())
                assert room >= 0, "%s: a push of %d overwrites the oldest input of the next output by %d" % (tag, c, -room)
                guard = R0[out] * of // nf - width - 1
                assert np.all(guard <= first[R0[out]]), tag
                groom = int((guard - (P[out] + c - Ch)).min())
                assert groom >= HEADROOM_CH, "%s: the history guard is %d samples from refusing a legal push of %d" % (tag, groom, c)
        worst = int((Rc - R0).max())
        assert worst <= adv - HEADROOM_ADV * (rate != 32000), "%s: a close advances by %d" % (tag, worst)
        n_closed = np.where(Rc < _ffi.MIN_SAMPLES, 0, np.where(Rc <= Wn, 1, 1 + (Rc - Wn + H - 1) // H))
        has = n_closed > j
        start = np.minimum(j * H, np.maximum(0, Rc - Wn))
        short = int((start - (Rc - C))[has].min()) if has.any() else 0
        assert short >= 0, "%s: a window pending after a close starts %d samples behind the ring" % (tag, -short)
        if rate != 32000:
            out = Rc > R0
            old = np.maximum(first[R0[out]], 0)
            assert int((old - (P[out] - Ch)).min()) >= 0, "%s: a close reads an overwritten input" % tag
            guard = R0[out] * of // nf - width - 1
            assert np.all(guard <= first[R0[out]]) and int((guard - (P[out] - Ch)).min()) >= 0, "%s: the guard refuses a close" % tag


def recordings_for(name, rate):
    """input lengths of the simulated recordings: the case's own, else a little over one and over two windows"""
    g = sc.GEOMETRIES[name]
    if name == "R" and rate in sc.RATE_CASES:
        return list(sc.RATE_CASES[rate]["recs"])
    recs = g["recs"] or (g["W"] + 5 * g["H"] + 3, 2 * g["W"] + 11)
    return [L * rate // 32000 for L in recs]


@pytest.mark.parametrize("name,rate", sweep_cases())
def test_probability_history_holds_every_cover(name, rate):
    """Whole recordings through Sim (stream_cases.py), which asserts at every call and at the close that the newest stashed window
    minus a newly final row's first covering window is below Hw and that every window of the cover is still in its history row
    (the end-aligned window included).  Chunkings: all max_push, seeded random, and all one-sample where affordable (recordings of more than 60000 pushes are left out).  What a
    chunking emits does not depend on max_push, and Hw grows with it, so the one-sample chunking runs at max_push = 1 only."""
    g = sc.GEOMETRIES[name]
    Wn, H = g["W"], g["H"]
    rng = random.Random(rate * 3 + Wn)
    for mp in sweep_pushes(name, rate):
        for L in recordings_for(name, rate):
            if L // mp > 60000:
                continue
            for plan in (sc.even_chunks(L, mp), sc.scaled_chunk_sizes(L, rng, mp)):
                sim = sc.simulate(sc.Sim(Wn, H, rate, mp, True, 256, name), [plan])
                nw, nr = stm.schedule(Wn, H, rate, L, True)[1:]          # Sim counts by stream_cases.schedule_def
                assert sum(len(c) for c in sim.forwards) == nw and len(sim.rows) == nr, sim.tag
    L = (Wn + min(3 * H, Wn) + 5) * rate // 32000
    if L <= 70000:
        sim = sc.simulate(sc.Sim(Wn, H, rate, 1, True, 256, name), [[1] * L])
        assert len(sim.rows) == stm.schedule(Wn, H, rate, L, True)[2], sim.tag


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_cases_reach_their_edges(name):
    """What tests/test_gpu_stream_geometry.py runs reaches what it is there for (stream_cases.check_reach asserts it): a window
    across the ring's mirror, a wrapped append, both append paths, a row whose cover wraps the probability history, and for A a
    forward of more than 128 windows."""
    for mp in sc.GEOMETRIES[name]["max_push"]:
        for even in (False, True):
            sc.case_sim(name, mp, even)


@pytest.mark.parametrize("rate", sorted(sc.RATE_CASES))
def test_rate_cases_reach_their_edges(rate):
    """The same for the other input rates: the ring, the input history and the probability history all wrap, and Sim's checks of
    the ring, the input history, the guard and the covers hold at every call (the 96 kHz one-sample case: see rate_sim)."""
    sc.rate_sim(rate)


def test_form_case_reaches_its_edges():
    """The 768 kHz case (the resampler's two-outputs-per-thread form, stream_cases.FORM_CASE): the same reach and the same checks
    at every call, and schedule_def agrees with acx_stream_schedule at that rate wherever sampled."""
    c = sc.FORM_CASE
    sim = sc.form_sim()
    assert all(n % 2 for n in (c["max_push"],) + c["recs"]) and any(n % 2 for plan in sc.form_plans() for n in plan)
    nw = sum(stm.schedule(c["W"], c["H"], c["rate"], L, True)[1] for L in c["recs"])
    assert sum(len(call) for call in sim.forwards) == nw
    rng = random.Random(768)
    for _ in range(12):
        P = rng.randrange(0, max(c["recs"]))
        for closed in (False, True):
            assert sc.schedule_def(c["W"], c["H"], c["rate"], P, closed) == stm.schedule(c["W"], c["H"], c["rate"], P, closed)


def test_schedule_def_is_the_schedule():
    """Sim counts with stream_cases.schedule_def, the restatement; it agrees with acx_stream_schedule wherever sampled."""
    rng = random.Random(5)
    for name, g in sc.GEOMETRIES.items():
        for rate in sc.RATES:
            for _ in range(12 if rate == 44101 else 200):
                P = rng.randrange(0, (3 * g["W"] + 7) * rate // 32000)
                for closed in (False, True):
                    assert sc.schedule_def(g["W"], g["H"], rate, P, closed) == stm.schedule(g["W"], g["H"], rate, P, closed)
