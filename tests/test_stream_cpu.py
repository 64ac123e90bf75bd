"""CPU: the schedule of live streams (acx_stream_schedule, include/acx.h) against a brute-force restatement of its definition,
and the argument checks of the C entry points and of the Python wrapper.  No device needed."""
import ctypes
import random

import numpy as np
import pytest

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import stream as stm
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

W = 320000


def final_table(rate, L):
    """need[n] = input samples output n needs pushed (itself and every earlier output), n < ceil(nf L / of); brute force
    over the band tables."""
    if rate == 32000:
        return np.arange(1, L + 1, dtype=np.int64)
    of, nf, width, _ = _ffi.resample_geometry(rate, 32000)
    start, count, _ = _ffi.resample_taps(rate, 32000)
    N = (nf * L + of - 1) // of
    n = np.arange(N, dtype=np.int64)
    j, i = n // nf, n % nf
    last = j * of + np.array(start, dtype=np.int64)[i] - width + np.array(count, dtype=np.int64)[i] - 1
    last[np.array(count)[i] == 0] = -1
    return np.maximum.accumulate(last + 1)


def brute(rate, H, L, pushed, closed):
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


@pytest.mark.parametrize("rate", [32000, 44100, 16000])
@pytest.mark.parametrize("H", [320, 32000, W])
def test_schedule_matches_definition(rate, H):
    rng = random.Random(rate * 7 + H)
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
                assert (R, nw, nr) == brute(rate, H, L, pushed, True)
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
        assert seen_w == len(win.window_starts([R_all], W, H))
        assert seen_r == len(win.timeline_steps([R_all], W, H))


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
