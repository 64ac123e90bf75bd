"""The helper behind the GPU frontend shape tests (tests/frontend_ref.py), checked on the CPU: the kernel's documented arithmetic
passes its interval, six mistakes a kernel could make fail it by ten bars or more, and every case the GPU file runs meets the
conditions on its bar -- K <= 64 and no cell with mel64 <= 2 b -- before a GPU sees it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import frontend_ref as fr
import layer_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_CASES = [(3, 641), (3, 1153), fr.SIGNAL]


@pytest.fixture(scope="module")
def hostfft():
    """libhostfft.so as tests/test_host_cpu.py builds it (rebuilt when the source is newer: the batched entry point is recent)."""
    so = os.path.join(ROOT, "build", "libhostfft.so")
    src = os.path.join(ROOT, "tests", "host_fft_check.cpp")
    if not os.path.isfile(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.acx_host_power_spectrum_tw.restype = None
    lib.acx_host_power_spectrum_tw.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    return lib


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product is exact in float64, one rounding of the sum to fp32 follows."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(hostfft, sd, wav, bn=False, pad="reflect", window=None, shift=0, drop_last_tap=False, drop_nyquist=False,
            tw_bits=None, mel_out=None):
    """logmel_kernel's arithmetic on the CPU, from three pieces: the fp32 window product, the radix-8 schedule of fft_core.h
    (acx_host_power_spectrum_tw with the kernel's twiddle table), the fp32 fma loop over the banded mel table and 10 log10f in
    numpy fp32 (+ the bn0 fma).  The keyword arguments make one mistake each."""
    x = wav.numpy()
    B, L = x.shape
    T = L // fr.HOP + 1
    xp = np.pad(x, ((0, 0), (512, 512 + shift)), mode=pad)
    win = (fr.stored_window(sd).numpy() if window is None else window).astype(np.float32)
    fw = np.stack([xp[:, fr.HOP * t + shift:fr.HOP * t + shift + fr.N_FFT] for t in range(T)], axis=1) * win
    fw = np.ascontiguousarray(fw.reshape(B * T, fr.N_FFT), dtype=np.float32)
    ang = -2.0 * np.pi * np.arange(fr.N_FFT) / fr.N_FFT
    tw = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    if tw_bits is not None:
        m, e = np.frexp(tw.astype(np.float64))
        tw = np.ldexp(np.round(m * 2.0 ** tw_bits) / 2.0 ** tw_bits, e).astype(np.float32)
    tw = np.ascontiguousarray(tw)
    P = np.zeros((B * T, fr.BINS), np.float32)
    hostfft.acx_host_power_spectrum_tw(fw.ctypes.data, P.ctypes.data, B * T, tw.ctypes.data)
    melW = sd[fr.KM].numpy()
    start, length = fr.band_table(sd[fr.KM])
    db = np.empty((B * T, fr.MELS), np.float32)
    for m in range(fr.MELS):
        n = length[m]
        if drop_last_tap or (drop_nyquist and start[m] + n == fr.BINS):
            n = max(n - 1, 0)
        acc = np.zeros(B * T, np.float32)
        for q in range(n):
            acc = _fma32(P[:, start[m] + q], np.full(B * T, melW[start[m] + q, m], np.float32), acc)
        if mel_out is not None:
            mel_out.append(acc)
        db[:, m] = np.float32(10.0) * np.log10(np.maximum(acc, np.float32(1e-10)))
    if bn:
        s, t = fr.bn_affine64(sd)
        db = _fma32(db, np.broadcast_to(s.float().numpy(), db.shape), np.broadcast_to(t.float().numpy(), db.shape))
    return torch.from_numpy(db.reshape(B, T, fr.MELS))


def test_reference_is_the_oracle_in_float64(synth_sd):
    """ref64 is oracle/ref_cpu.py's spectrogram and mel product on float64 weights; the stored window is torchlibrosa's periodic
    hann; frames() picks what F.pad + the stride-320 conv see."""
    from oracle import ref_cpu
    wav = fr.edge_wav(3, 641, seed=1)
    P64, mel64 = fr.ref64(synth_sd, wav)
    P = ref_cpu.spectrogram(lr.to64(synth_sd), wav.double())[:, 0]
    assert P64.shape == (3, 3, 513) and float((P64 - P).abs().max()) <= 1e-12 * float(P.max())
    assert float((mel64 - P @ synth_sd[fr.KM].double()).abs().max()) <= 1e-12 * float(mel64.max())
    n = np.arange(1024)
    assert np.abs(fr.stored_window(synth_sd).numpy() - (0.5 - 0.5 * np.cos(2 * np.pi * n / 1024))).max() < 1e-7
    f = fr.frames(wav)
    assert f.shape == (3, 3, 1024) and float(f[1, 0, 512]) == float(np.float32(0.9)) and float(f[1, 0, 511]) == float(f[1, 0, 513])
    assert float(f[2, 2, 512]) == float(np.float32(-0.9)) and float(f[2, 2, 513]) == float(f[2, 2, 511])       # 640 = L - 1: the mirror sits on it


def test_banks_take_the_loops_they_are_meant_for(synth_sd):
    """The shipped bank has 1 / 3 / 8 / 14 taps at most per lane group and ends at bin 447; bank by bank, the restated choice of
    logmel_kernel's filter loop is the one the GPU file wants to run."""
    start, length = fr.band_table(synth_sd[fr.KM])
    assert [int(length[64 * g:64 * g + 64].max()) for g in range(4)] == [1, 3, 8, 14]
    assert int(length.sum()) == 884 and int((start + length).max()) == 448
    for bank in fr.BANKS:
        loop, taps = fr.mel_loop(fr.variant_sd(synth_sd, bank)[fr.KM])
        print("bank %-10s -> %s loop, %d taps" % (bank, loop, taps))
        assert loop == fr.BANK_LOOP[bank], (bank, loop)
    s, n = fr.band_table(fr.variant_sd(synth_sd, "nyquist")[fr.KM])
    assert (s[223], n[223]) == (500, 13) and s[223] + 14 > fr.BINS
    s, n = fr.band_table(fr.variant_sd(synth_sd, "wide0")[fr.KM])
    assert n[5] == 2 and int(n.sum()) <= fr.MEL_LDS
    assert fr.band_table(fr.variant_sd(synth_sd, "zero_col")[fr.KM])[1][fr.ZERO_COL] == 0
    assert fr.mel_loop(fr.variant_sd(synth_sd, "dense_melW")[fr.KM])[1] == 513 * 224


@pytest.mark.parametrize("which,shape,frontends", fr.all_gpu_cases(), ids=lambda v: fr.shape_id(v) if isinstance(v, tuple) and
                         len(v) == 2 and isinstance(v[0], int) else (v if isinstance(v, str) else None))
def test_gpu_cases_are_not_vacuous(which, shape, frontends):
    """Every case of tests/test_gpu_frontend_shapes.py, from the reference alone: K <= 64, and no cell whose lower bound says
    little (mel64 <= 2 b)."""
    c = fr.case(which, shape)
    for f in frontends:
        print("%-26s %-5s K %.2f (formula %.2f)  n_fft %.3f  n_dense %s  d0 %.3g  min mel64 / b %.1f  cells <= 2 b: %d"
              % (c.name, f, c.K(f), c.K_formula(f), c.n_fft, "%.3f" % c.n_dense if c.n_dense is not None else "-", c.d0,
                 c.min_mel_over_bar(f), c.vacuous(f)))
        assert c.K(f) <= fr.K_MAX
        assert c.vacuous(f) == 0
        assert c.d0 < 2e-5                                    # a few ulp of |dB| < 40
    dead = int((~c.live).sum())
    assert dead == (c.mel64.shape[0] * c.mel64.shape[1] if which == "zero_col" else 0)


@pytest.mark.parametrize("shape", EMU_CASES, ids=fr.shape_id)
def test_emulation_passes_and_mistakes_fail(hostfft, synth_sd, shape):
    """The kernel's documented arithmetic passes the interval of the FFT frontend (dB, and bn0 of it); one mistake at a time
    lands ten bars or more outside."""
    c = fr.case("shipped", shape)
    mel = []
    c.check("emulation " + c.name, emulate(hostfft, c.sd, c.wav, mel_out=mel), "auto")
    ratio = c.ratio(torch.from_numpy(np.stack(mel, axis=1)).view(c.mel64.shape))         # before the dB: the arithmetic alone
    print("emulation %s: ratio %.3f = %.2f x n_fft" % (c.name, ratio, ratio / c.n_fft))
    assert ratio <= 2.0 * c.n_fft                            # (the schedule reaches 0.9 - 1.4 x n_fft: half the margin of 4)
    c.check("emulation " + c.name, emulate(hostfft, c.sd, c.wav, bn=True), "auto", bn=True)
    n = np.arange(1024)
    mistakes = {
        "reflect with edge repeat": dict(pad="symmetric"),
        "symmetric hann": dict(window=0.5 - 0.5 * np.cos(2 * np.pi * n / 1023)),
        "frame start off by one": dict(shift=1),
        "last mel tap dropped": dict(drop_last_tap=True),
        "twiddles of 12 bits": dict(tw_bits=12),
    }
    for name, kw in mistakes.items():
        by = c.fails_by(emulate(hostfft, c.sd, c.wav, **kw), "auto")
        print("%-26s on %-10s: %.3g x bar" % (name, fr.shape_id(shape), by))
        assert by >= 10.0, (name, by)
        with pytest.raises(AssertionError):
            c.check(name, emulate(hostfft, c.sd, c.wav, **kw), "auto")
    # bank (c): the bands that reach the Nyquist bin lose it
    cn = fr.case("nyquist", shape) if shape in fr.BANK_SHAPES else fr.FrontCase("nyquist " + fr.shape_id(shape),
                                                                                fr.variant_sd(synth_sd, "nyquist"), c.wav)
    cn.check("emulation " + cn.name, emulate(hostfft, cn.sd, cn.wav), "auto")
    by = cn.fails_by(emulate(hostfft, cn.sd, cn.wav, drop_nyquist=True), "auto")
    print("%-26s on %-10s: %.3g x bar" % ("Nyquist bin dropped", fr.shape_id(shape), by))
    assert by >= 10.0


def test_interval_handles_the_clamp_and_an_empty_band(hostfft, synth_sd):
    """A band of length 0 is the clamp value in every cell, -100 dB to the last bits of the fp32 log10 (S = 0: no slack but d);
    the same cell at -99.99 is outside."""
    c = fr.case("zero_col", (3, 1153))
    out = emulate(hostfft, c.sd, c.wav)
    col = out[:, :, fr.ZERO_COL]
    assert bool((col == col[0, 0]).all()) and abs(float(col[0, 0]) + 100.0) <= c.d < 2e-5
    c.check("emulation " + c.name, out, "auto")
    bad = out.clone()
    bad[0, 0, fr.ZERO_COL] = -99.99
    with pytest.raises(AssertionError):
        c.check("clamp missed", bad, "auto")


def test_pool_cases_have_tight_bars():
    """The float64 pool / head statement is the oracle's tail; every bar is 8 x noise32, far under 1e-4; the raised row is the
    last one of the last phase that holds a row."""
    assert [fr.pool_raised_row(h) for h in (1, 2, 3, 4, 5, 7, 31)] == [0, 1, 2, 3, 3, 3, 27]
    assert len(fr.POOL_SHAPES) == 15 and (70, 7) in fr.POOL_SHAPES
    for B, H3 in ((1, 1), (3, 5), (3, 31)):
        x, cases = fr.pool_case(B, H3)
        r = fr.pool_raised_row(H3)
        y = x.double().mean(dim=2)
        assert bool((y.argmax(dim=1)[:, ::2] == r).all())     # the maximum of the raised channels lives in that row
        for k, case in cases.items():
            assert 0.0 < case.noise32 and case.bar("fp32") == 8.0 * case.noise32 < lr.LAYER_TOL / 3.0, (k, case.noise32)
