"""CPU: the host side of input resampling (acx_resample_geometry / acx_resample_taps / acx_resampled_length, include/acx.h) --
geometry and output lengths against utils/resample.py, the stored taps against a float64 evaluation of the formula and
against the restatement's dense filter bank, and the argument checks of the C ABI and of the Python surface."""
import ctypes
import math

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import resample as gpu_resample
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.utils.resample import resample as host_resample, sinc_resample_kernel

RATES = (8000, 11025, 16000, 22050, 24000, 44100, 48000, 88200, 96000, 44101)


def reduced(orig, new=32000):
    g = math.gcd(orig, new)
    return orig // g, new // g


def exact_taps(orig, i, k):
    """float64 h_i[k] and t, formed as utils/resample.py forms t (k may be an array)."""
    of, nf = reduced(orig)
    base = min(of, nf) * 0.99
    width = math.ceil(6 * of / base)
    t = (-i / nf + (np.asarray(k) - width) / of) * base
    s = np.where(t == 0, 1.0, np.sin(np.pi * t) / np.where(t == 0, 1.0, np.pi * t))
    return (base / of) * s * np.cos(np.pi * t / 12) ** 2, t


@pytest.mark.parametrize("orig", RATES)
def test_geometry_and_lengths_match_the_host_restatement(orig):
    of, nf, width, max_band = _ffi.resample_geometry(orig, 32000)
    assert (of, nf) == reduced(orig)
    assert width == math.ceil(6 * of / (min(of, nf) * 0.99))
    if orig != 44101:                                  # (its dense bank would have 32000 x 44119 taps)
        assert width == sinc_resample_kernel(orig, 32000, math.gcd(orig, 32000))[1]
    assert 13 <= max_band <= 40
    for L in (1, of - 1, of, of + 1, 320000, 441000):
        if L < 0:
            continue
        n = _ffi.resampled_length(orig, 32000, L)
        assert n == gpu_resample.resampled_length(L, orig)
        assert n == int(math.ceil(nf * L / of)), (orig, L)        # utils/resample.py's target_length
        if orig != 44101 and L in (1, of - 1, of, of + 1) and L > 0:
            assert host_resample(torch.zeros(1, L), orig, 32000).shape[-1] == n
    if orig != 44101:
        assert host_resample(torch.zeros(1, 441000), orig, 32000).shape[-1] == _ffi.resampled_length(orig, 32000, 441000)


@pytest.mark.parametrize("orig", RATES)
def test_taps_are_the_rounded_formula_on_the_band(orig):
    of, nf, width, max_band = _ffi.resample_geometry(orig, 32000)
    start, count, taps = _ffi.resample_taps(orig, 32000)
    start, count, taps = np.array(start), np.array(count), np.array(taps, dtype=np.float32)
    assert len(start) == nf and count.sum() == len(taps) and count.max() == max_band and count.min() >= 1
    phase = np.repeat(np.arange(nf), count)
    k = np.repeat(start, count) + (np.arange(len(taps)) - np.repeat(np.cumsum(count) - count, count))
    h, t = exact_taps(orig, phase, k)
    assert np.all(np.abs(t) < 6)
    # within half an ulp of the float64 value: rounded once
    ulp = np.spacing(np.abs(taps).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(taps.astype(np.float64) - h) <= 0.5 * ulp * (1 + 1e-9)), orig
    # the band holds exactly the k with |t| < 6: its neighbours are outside
    i = np.arange(nf)
    assert np.all(np.abs(exact_taps(orig, i, start - 1)[1]) >= 6) and np.all(np.abs(exact_taps(orig, i, start + count)[1]) >= 6)
    assert np.all(start >= 0) and np.all(start + count <= 2 * width + of)
    if orig == 44101:
        return
    dense = np.zeros((nf, 2 * width + of))
    dense[phase, k] = taps
    ref32 = sinc_resample_kernel(orig, 32000, math.gcd(orig, 32000))[0][:, 0].double().numpy()
    ref64 = sinc_resample_kernel(orig, 32000, math.gcd(orig, 32000), dtype=torch.float64)[0][:, 0].numpy()
    assert np.abs(dense - ref64).max() < 1e-7
    # the restatement evaluates its taps in float32 (1.5e-5 off at 44.1 kHz; 3.1e-5 at 11.025 / 22.05 kHz, where the
    # bound is its own error against the float64 bank)
    own = np.abs(ref32 - ref64).max()
    assert np.abs(dense - ref32).max() < max(2e-5, 1.05 * own), (orig, own)


def test_rate_errors():
    lib = _ffi.lib()
    for orig, new in ((0, 32000), (-44100, 32000), (768001, 32000), (44100, 0), (44100, 800000)):
        assert lib.acx_resample_geometry(orig, new, None, None, None, None) == -1          # ACX_ERR_ARG
        assert b"768000" in lib.acx_last_error()
        out = ctypes.c_int64()
        assert lib.acx_resampled_length(orig, new, 100, ctypes.byref(out)) == -1
    assert lib.acx_resampled_length(44100, 32000, -1, ctypes.byref(ctypes.c_int64())) == -1
    # over the table cap: ACX_ERR_UNSUPPORTED naming the reduced ratio
    for orig, new, ratio in ((767999, 32000, b"767999/32000"), (1, 768000, b"1/768000"), (768000, 1, b"768000/1")):
        assert lib.acx_resample_geometry(orig, new, None, None, None, None) == -6          # ACX_ERR_UNSUPPORTED
        assert ratio in lib.acx_last_error()
        assert lib.acx_resample_taps(orig, new, None, None, None, 0) == -6
    # a taps buffer too small for the bands
    buf = (ctypes.c_float * 4)()
    assert lib.acx_resample_taps(44100, 32000, None, None, buf, 4) == -1
    # 44101 Hz (of = 44101, nf = 32000) fits the cap
    assert _ffi.resample_geometry(44101, 32000)[:2] == (44101, 32000)


def test_python_surface_errors_without_a_gpu():
    with pytest.raises(RuntimeError, match="GPU"):
        gpu_resample.resample(torch.zeros(2, 1000), 44100)
    with pytest.raises(ValueError, match="integer"):
        gpu_resample.resample(torch.zeros(2, 1000), 44100.5)
    with pytest.raises(ValueError, match="768000"):
        gpu_resample.resample(torch.zeros(2, 1000), 0)
    with pytest.raises(RuntimeError, match=r"10000 samples at 44100 Hz \(7257 samples at 32000 Hz\) is too short"):
        gpu_resample.check_min_length(10000, 44100)
    assert gpu_resample.check_min_length(10142, 44100) == 7360
    m = convnext_tiny(after_stem_dim=[252, 56]).eval()
    with pytest.raises(ValueError, match="integer"):
        m(torch.zeros(1, 20000), sample_rate=22050.5)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 20000), sample_rate=22050)
    with pytest.raises(RuntimeError, match="GPU"):
        m.forward_varlen([torch.zeros(20000)], sample_rate=48000)
