"""CPU: the host side of sliding windows -- acx_window_count against the pure-Python enumeration (pytorch/windows.py), the
enumeration against the definition, argument checks of the C ABI and of the wrapper (no device needed)."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import windows as win
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny


def count(lengths, window, hop):
    lens = (ctypes.c_int64 * max(1, len(lengths)))(*lengths)
    out = ctypes.c_int64(-1)
    rc = _ffi.lib().acx_window_count(lens, len(lengths), window, hop, ctypes.byref(out))
    return rc, out.value, _ffi.lib().acx_last_error().decode()


def test_version():
    assert _ffi.lib().acx_version() == 101


# H in {320, 32000, W} for W in {7360, 320000}, a hop longer than the window left out
@pytest.mark.parametrize("W,H", [(7360, 320), (7360, 7360), (320000, 320), (320000, 32000), (320000, 320000)])
def test_count_matches_enumeration(W, H):
    grid = [W - 1, W, W + 1, W + H - 1, W + H, 10 * W + 7]
    for L in grid:
        rc, n, msg = count([L], W, H)
        assert rc == _ffi.OK, msg
        assert n == len(win.window_starts([L], W, H)), (L, W, H)
    rc, n, _ = count(grid, W, H)
    assert rc == _ffi.OK and n == len(win.window_starts(grid, W, H)) == _ffi.window_count(grid, W, H)


def covering(starts, L, W, m):
    return [j for j, s in enumerate(starts) if s <= m < s + W]


@pytest.mark.parametrize("L,W,H", [(37, 10, 3), (10, 10, 10), (9, 10, 4), (61, 10, 10), (23, 10, 1), (1193600, 320000, 32000)])
def test_starts_and_steps_follow_the_definition(L, W, H, monkeypatch):
    monkeypatch.setattr(_ffi, "MIN_SAMPLES", 1)                       # small numbers keep the definition readable
    starts = win.window_starts([L], W, H)
    n = 1 if L <= W else 1 + -(-(L - W) // H)
    assert len(starts) == n
    assert starts == [min(j * H, max(0, L - W)) for j in range(n)]
    assert starts[0] == 0 and starts == sorted(starts)
    if L >= W:
        assert starts[-1] + W == L                                     # the last window ends with the recording
        assert all(b - a <= H for a, b in zip(starts, starts[1:]))     # no sample is left uncovered
    mids = win.timeline_steps([L], W, H)
    assert len(mids) == -(-L // H)
    for k, m in enumerate(mids):
        assert m == min(k * H + H // 2, L - 1)
        assert covering(starts, L, W, m), (k, m)                       # at least one window qualifies


def test_enumeration_is_per_recording(monkeypatch):
    monkeypatch.setattr(_ffi, "MIN_SAMPLES", 1)
    assert win.window_starts([25, 7, 10], 10, 5) == [0, 5, 10, 15, 0, 0]
    assert win.timeline_steps([25, 7], 10, 5) == [2, 7, 12, 17, 22, 2, 6]


def test_short_recordings_are_one_window():
    for L in (0, 1, 7359, 319999, 320000):
        assert win.window_starts([L], 320000, 32000) == [0]
        assert count([L], 320000, 32000)[:2] == (_ffi.OK, 1)


def test_error_codes():
    rc, _, msg = count([400000], 320000, 0)
    assert rc == -1 and "hop" in msg
    assert count([400000], 320000, -5)[0] == -1
    rc, _, msg = count([400000], 320000, 320001)
    assert rc == -1 and "hop" in msg
    rc, _, msg = count([400000], 7359, 320)
    assert rc == -4 and "kernel size can't be greater than actual input size" in msg
    assert count([400000], 7360, 320)[0] == _ffi.OK
    rc, _, msg = count([8000] * 257, 7360, 320)
    assert rc == -1 and "257" in msg
    assert count([8000] * 256, 7360, 320)[0] == _ffi.OK
    assert count([], 7360, 320)[0] == -1
    rc, _, msg = count([8000, -1], 7360, 320)
    assert rc == -1 and "recording 1" in msg
    out = ctypes.c_int64()
    assert _ffi.lib().acx_window_count(None, 1, 7360, 320, ctypes.byref(out)) == -1
    # the forward and the timeline check the same arguments before touching a device
    lens = (ctypes.c_int64 * 1)(400000)
    assert _ffi.lib().acx_window_timeline(None, lens, 1, 320000, 32000, 0, None, None) == -1
    buf = ctypes.c_void_p(16)
    assert _ffi.lib().acx_window_timeline(buf, lens, 1, 320000, 32000, 2, buf, None) == -1
    assert _ffi.lib().acx_window_timeline(buf, lens, 1, 320000, 320001, 0, buf, None) == -1
    assert _ffi.lib().acx_forward_windows(None, buf, lens, 1, 320000, 32000, 0, 1, 0, buf, buf, buf, 1 << 30, None) == -1
    size = ctypes.c_size_t()
    assert _ffi.lib().acx_workspace_bytes_windows(None, 8, 320000, 0, ctypes.byref(size)) == _ffi.OK
    uni = ctypes.c_size_t()
    assert _ffi.lib().acx_workspace_bytes(None, 8, 320000, 0, ctypes.byref(uni)) == _ffi.OK
    assert size.value >= uni.value + 64
    assert _ffi.lib().acx_workspace_bytes_windows(None, 8, 7359, 0, ctypes.byref(size)) == -4
    assert _ffi.lib().acx_workspace_bytes_windows(None, 8, 320000, 3, ctypes.byref(size)) == -1


def test_python_checks_mirror_the_abi():
    with pytest.raises(ValueError, match="hop"):
        win.window_starts([400000], 320000, 0)
    with pytest.raises(ValueError, match="hop"):
        win.window_starts([400000], 320000, 320001)
    with pytest.raises(ValueError, match="too short"):
        win.timeline_steps([400000], 7359, 320)


@pytest.mark.parametrize("seconds,samples", [(10.0, 320000), (10, 320000), (1.0, 32000), (0.23, 7360), (37.3, 1193600),
                                             (0.01, 320), (3.125e-05, 1)])
def test_seconds_to_samples(seconds, samples):
    assert win.seconds_to_samples(seconds) == samples


@pytest.mark.parametrize("seconds", [1e-5, 0.0001, 10.00001, 1 / 3])
def test_non_integral_seconds_raise(seconds):
    with pytest.raises(ValueError, match="whole number of samples"):
        win.seconds_to_samples(seconds)


def make_model():
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    return m.eval()


def test_forward_windows_cpu_input_is_refused():
    model = make_model()
    with pytest.raises(RuntimeError, match="GPU only"):
        model.forward_windows(torch.zeros(400000))
    with pytest.raises(RuntimeError, match="GPU only"):
        model.forward_windows([torch.zeros(400000), torch.zeros(9000)], window=1.0, hop=0.5)


def test_forward_windows_argument_checks():
    model = make_model()
    x = torch.zeros(400000)
    with pytest.raises(ValueError, match="whole number of samples"):
        model.forward_windows(x, window=10.00001)
    with pytest.raises(ValueError, match="hop"):
        model.forward_windows(x, window=1.0, hop=2.0)
    with pytest.raises(ValueError, match="too short"):
        model.forward_windows(x, window=0.2)
    with pytest.raises(ValueError, match="what"):
        model.forward_windows(x, what="segments")
    with pytest.raises(ValueError, match="timeline"):
        model.forward_windows(x, timeline="median")
    with pytest.raises(ValueError, match="max_batch"):
        model.forward_windows(x, max_batch=0)
    with pytest.raises(ValueError):
        model.forward_windows([])
    with pytest.raises(RuntimeError, match="model.eval"):
        model.train().forward_windows(x)
