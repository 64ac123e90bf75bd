"""Resampling of input clips on the GPU (acx_resample, include/acx.h): the band-limited interpolation that the reference's demo
applies on the host with torchaudio.functional.resample (demo_convnext.py:53-59) and its extraction script with
librosa.load(sr=32000) (pytorch/extract_embeddings.py), computed by a HIP kernel on the caller's stream.

Same interpolation and output length as utils/resample.py (the host path, unchanged); the taps are evaluated in float64 and
rounded to fp32 once, where the host restatement evaluates them in float32, so the two agree to ~1.5e-5 of full scale.
Every clip's output bits are the same whether it is resampled alone, in a uniform batch or packed among other clips.
Non-finite input is out of scope (a NaN spreads over the ~17 outputs whose band holds it)."""
import math

import torch

from .. import _ffi

MODEL_RATE = 32000
_CACHE = {}        # (device index, orig, new) -> _ffi.Resampler, for calls without a module of their own


def check_rate(rate, name="sample_rate"):
    """An integer rate in [1, 768000] (an integral float is accepted, as torchaudio does)."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or int(rate) != rate:
        raise ValueError("%s must be an integer number of Hz (got %r): resampling needs integer rates" % (name, rate))
    rate = int(rate)
    if not 1 <= rate <= 768000:
        raise ValueError("%s must be in [1, 768000] Hz (got %d)" % (name, rate))
    return rate


def resampled_length(L, orig_freq, new_freq=MODEL_RATE):
    """ceil(nf * L / of): the output length of utils/resample.py (exact integer arithmetic)."""
    g = math.gcd(orig_freq, new_freq)
    of, nf = orig_freq // g, new_freq // g
    return (nf * int(L) + of - 1) // of


def check_min_length(L, orig_freq, index=None):
    """The model's "too short" error for a clip of L samples at orig_freq Hz, stated in input and in model-rate samples."""
    n = resampled_length(L, orig_freq)
    if n < _ffi.MIN_SAMPLES:
        raise RuntimeError("%sof %d samples at %d Hz (%d samples at %d Hz) is too short: kernel size can't be greater than "
                           "actual input size (minimum is %d samples at %d Hz)"
                           % ("clip " if index is None else "clip %d " % index, L, orig_freq, n, MODEL_RATE,
                              _ffi.MIN_SAMPLES, MODEL_RATE))
    return n


def resampler(device, orig_freq, new_freq, cache=None):
    """The acx_resampler of (device, orig_freq -> new_freq), built once per cache."""
    cache = _CACHE if cache is None else cache
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, orig_freq, new_freq)
    rs = cache.get(key)
    if rs is None:
        rs = cache[key] = _ffi.Resampler(idx, orig_freq, new_freq)
    return rs


def _run_packed(wav, lengths, orig_freq, new_freq, cache):
    out_lengths = [resampled_length(n, orig_freq, new_freq) for n in lengths]
    out = torch.empty(sum(out_lengths), dtype=torch.float32, device=wav.device)
    with torch.cuda.device(wav.device):
        rs = resampler(wav.device, orig_freq, new_freq, cache)
        cap, s0, o0 = _ffi.MAX_VARLEN_CLIPS, 0, 0
        for c0 in range(0, len(lengths), cap):
            chunk, ochunk = lengths[c0:c0 + cap], out_lengths[c0:c0 + cap]
            n, m = sum(chunk), sum(ochunk)
            if m:
                rs.run(wav[s0:s0 + n], chunk, out[o0:o0 + m])
            s0, o0 = s0 + n, o0 + m
    return out, out_lengths


def resample(waveform, orig_freq, new_freq=MODEL_RATE, lengths=None, _cache=None):
    """Resample CUDA clips on the device, on the current stream.

    waveform (..., time) -> (..., ceil(nf * time / of)) fp32; or, with `lengths`, a packed 1-D tensor of clips back to back ->
    (packed output, list of output lengths).  orig_freq == new_freq returns the input unchanged (nothing is launched).  More
    than 256 clips run as several launches.  CPU tensors are refused: the host path is utils/resample.py."""
    orig_freq, new_freq = check_rate(orig_freq, "orig_freq"), check_rate(new_freq, "new_freq")
    if not isinstance(waveform, torch.Tensor):
        raise TypeError("expected a torch tensor, got %r" % type(waveform))
    if waveform.device.type != "cuda":
        raise RuntimeError("resample runs on the GPU: move the waveform with .to('cuda'); the host path is "
                           "audioset_convnext_inf_amd.utils.resample")
    if lengths is not None:
        if waveform.dim() != 1:
            raise ValueError("a packed waveform is 1-D (got shape %r)" % (tuple(waveform.shape),))
        lengths = [int(n) for n in lengths]
        if any(n < 0 for n in lengths) or sum(lengths) != waveform.numel():
            raise ValueError("lengths sum to %d samples but the packed tensor holds %d" % (sum(lengths), waveform.numel()))
        if orig_freq == new_freq:
            return waveform, lengths
        wav = waveform.detach().to(torch.float32).contiguous()
        return _run_packed(wav, lengths, orig_freq, new_freq, _cache)
    if waveform.dim() < 1:
        raise ValueError("expected a (..., time) waveform")
    if orig_freq == new_freq:
        return waveform
    shape = waveform.shape
    L = shape[-1]
    x = waveform.detach().to(torch.float32).contiguous().reshape(-1, L)
    out, out_lengths = _run_packed(x.reshape(-1), [L] * x.shape[0], orig_freq, new_freq, _cache)
    return out.view(tuple(shape[:-1]) + (resampled_length(L, orig_freq, new_freq),))
