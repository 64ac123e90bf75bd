"""The float64 reference and the bar of the frontend shape tests (tests/test_gpu_frontend_shapes.py), a plain helper imported like
layer_ref.py; tests/test_frontend_ref_cpu.py shows on the CPU that the bar notices a mistake.

Reference.  ref64: reflect-pad 512 | 512, the two Conv1d with the STORED conv_real / conv_imag weights in float64 (the stored
buffers define the transform, not an ideal DFT), P64 = re^2 + im^2, mel64 = P64 @ melW in float64.

Error scale.  What an fp32 transform does to a power bin grows with the bin AND with the frame's strongest bin.  With u = 2^-24:

    dX[f, k] = u (|X[f, k]| + max_j |X[f, j]|),   S_P = 2 |X| dX + dX^2,   S = S_P @ |melW|,   ratio(impl) = max |mel_impl - mel64| / S.

Bar, per case, from the reference alone.  n_fft = ratio(fp32 torch.fft.rfft of frame x stored window), n_dense = ratio(the fp32
oracle's two Conv1d), both through the same fp32 `@ melW`:

    K(case, "auto") = 4 n_fft,   K(case, "dense") = 4 max(n_fft, n_dense),   b = K S,   K <= 64 asserted.

4: the kernel's radix-8 schedule reaches 0.9 - 1.4 x n_fft on the CPU, the device contracts to FMAs, sums the mel taps in another
order, and the GEMM sums its 1 024 products in another order than the CPU conv.  Nothing a kernel (or the emulation of its
schedule, which is built from fft_core.h) produced enters a bar.

Check: an interval in dB, the unit the device writes:

    10 log10(max(mel64 - b, 1e-10)) - d  <=  o  <=  10 log10(max(mel64 + b, 1e-10)) + d,

d = 4 d0, d0 = max |fp32 torch 10 log10(clamp) - float64| over the case's mel64.float(): the fp32 log10f, the product by 10 and the
rounding of the output (1 ulp for glibc, a few for the device).  With bn0 the ends go through the float64 affine and the slack is
d |scale| plus one fp32 rounding of the result.  The clamp and weak bins are handled by the interval itself; a case must have no
cell with mel64 <= 2 b (vacuous()), so that no test hides behind them.  A column of melW that is all zero has S = 0: its cells
must be exactly the clamp value."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu

U = 2.0 ** -24
MARGIN = 4.0                # K = MARGIN x the fp32 references' own ratio
K_MAX = 64.0
D_MARGIN = 4.0              # d = D_MARGIN x d0
AMIN = 1e-10
N_FFT, HOP, BINS, MELS = 1024, 320, 513, 224
KR, KI, KM = ("spectrogram_extractor.stft.conv_real.weight", "spectrogram_extractor.stft.conv_imag.weight",
              "logmel_extractor.melW")
MEL_LDS = 1664              # taps the log-mel kernel keeps in the LDS (frontend.hip, kMelLds)
MEL_FAST_TAPS = (1, 3, 8, 14)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def padded(wav):
    return F.pad(wav[:, None, :], (N_FFT // 2, N_FFT // 2), mode="reflect")


def frames(wav):
    """(B, L) -> (B, T, 1024): frame t = padded[320 t, 320 t + 1024), in wav's precision."""
    return padded(wav)[:, 0].unfold(1, N_FFT, HOP)


@torch.no_grad()
def ref64(sd, wav):
    """-> P64 (B, T, 513), mel64 (B, T, 224)."""
    x = padded(wav.double())
    re = F.conv1d(x, sd[KR].double(), stride=HOP)
    im = F.conv1d(x, sd[KI].double(), stride=HOP)
    P = (re * re + im * im).transpose(1, 2).contiguous()
    return P, P @ sd[KM].double()


def scale(P64, melW):
    X = P64.sqrt()
    dX = U * (X + X.amax(dim=-1, keepdim=True))
    return (2.0 * X * dX + dX * dX) @ melW.double().abs()


def stored_window(sd):
    return sd[KR][0, 0]                                      # bin 0: cos = 1, the row IS the window (weights.hip reads it there)


@torch.no_grad()
def mel_fft32(sd, wav):
    """fp32: frame x stored window -> torch.fft.rfft -> power -> @ melW."""
    Z = torch.fft.rfft(frames(wav) * stored_window(sd))
    return (Z.real * Z.real + Z.imag * Z.imag) @ sd[KM]


@torch.no_grad()
def mel_dense32(sd, wav):
    """fp32: the oracle's two Conv1d (oracle/ref_cpu.py spectrogram) -> @ melW."""
    return ref_cpu.spectrogram(sd, wav)[:, 0] @ sd[KM]


def db64(mel):
    return 10.0 * torch.log10(mel.clamp_min(AMIN))


def bn_affine64(sd):
    s = sd["bn0.weight"].double() / torch.sqrt(sd["bn0.running_var"].double() + 1e-5)
    return s, sd["bn0.bias"].double() - sd["bn0.running_mean"].double() * s


class FrontCase:
    """One (state dict, waveform): the float64 reference, the scale, the fp32 references' ratios and d0.  Never modified."""

    def __init__(self, name, sd, wav, dense=True):
        self.name, self.sd, self.wav = name, sd, wav
        P64, self.mel64 = ref64(sd, wav)
        self.S = scale(P64, sd[KM])
        self.live = self.S > 0.0                             # (an all-zero column of melW: S = 0, mel64 = 0, exact)
        self.n_fft = self.ratio(mel_fft32(sd, wav))
        self.n_dense = self.ratio(mel_dense32(sd, wav)) if dense else None
        m32 = self.mel64.float()
        self.d0 = float(((10.0 * torch.log10(m32.clamp_min(AMIN))).double() - db64(m32.double())).abs().max())
        self.d = D_MARGIN * self.d0

    def ratio(self, mel):
        """max |mel - mel64| / S; where S = 0 the value must be exactly mel64 (0)."""
        e = (mel.double() - self.mel64).abs()
        assert not bool((e[~self.live] != 0.0).any())
        return float((e[self.live] / self.S[self.live]).max())

    def K_formula(self, frontend):
        if frontend == "auto":
            return MARGIN * self.n_fft
        assert self.n_dense is not None, "case %s has no dense reference" % self.name
        return MARGIN * max(self.n_fft, self.n_dense)

    def K(self, frontend):
        """min(the formula, K_MAX): the fp32 oracle's Conv1d sums its 1 024 products one after the other and its worst cell grows
        with the number of cells -- 8 220 frames give 4 x 16.8 = 67 -- so the bar of such a case is held at 64, tighter than the
        formula asks; no case's K exceeds K_MAX on any machine's conv."""
        k = min(self.K_formula(frontend), K_MAX)
        assert 0.0 < k <= K_MAX, (self.name, frontend, k)
        return k

    def vacuous(self, frontend):
        """Cells whose lower bound says little: mel64 <= 2 b (cells of an all-zero column are exact and do not count)."""
        return int(((self.mel64 <= 2.0 * self.K(frontend) * self.S) & self.live).sum())

    def min_mel_over_bar(self, frontend):
        return float((self.mel64[self.live] / (self.K(frontend) * self.S[self.live])).min())

    def mel_interval_db(self, frontend):
        b = self.K(frontend) * self.S
        return db64(self.mel64 - b), db64(self.mel64 + b)

    def interval(self, frontend, bn=False):
        """-> lo, hi (float64) for the device's output, dB or bn0 of it."""
        lo, hi = self.mel_interval_db(frontend)
        if not bn:
            return lo - self.d, hi + self.d
        s, t = bn_affine64(self.sd)
        a, c = lo * s + t, hi * s + t
        slack = self.d * s.abs() + U * torch.maximum(a.abs(), c.abs())
        return torch.minimum(a, c) - slack, torch.maximum(a, c) + slack

    def figures(self, out, frontend, bn=False):
        """-> worst |10^(o / 10) - mel64| / b (the output rounded to dB included), worst distance outside the mel interval in dB
        (the part d has to cover), worst violation of the whole interval (<= 0: inside)."""
        o = out.detach().cpu().double()
        lo, hi = self.interval(frontend, bn)
        viol = float(torch.maximum(lo - o, o - hi).max())
        if bn:
            s, t = bn_affine64(self.sd)
            o = (o - t) / s
        mlo, mhi = self.mel_interval_db(frontend)
        over = float(torch.maximum(mlo - o, o - mhi).clamp_min(0.0).max())
        e = (torch.pow(10.0, o / 10.0) - self.mel64).abs()
        excess = float((e[self.live] / (self.K(frontend) * self.S[self.live])).max())
        return excess, over, viol

    def check(self, what, out, frontend, bn=False):
        """Prints the figures, then asserts the interval; returns excess / bar."""
        excess, over, viol = self.figures(out, frontend, bn)
        print("%-34s %-5s %s excess/bar %.3f  K %.2f  n_fft %.3f  n_dense %s  d0 %.3g  d %.3g  over mel interval %.3g dB"
              % (what or self.name, frontend, "bn0" if bn else "dB ", excess, self.K(frontend), self.n_fft,
                 "%.3f" % self.n_dense if self.n_dense is not None else "-", self.d0, self.d, over))
        assert viol <= 0.0, (self.name, frontend, bn, viol, excess)
        return excess

    def fails_by(self, out, frontend):
        """How far a (wrong) output in dB lies outside: worst |10^(o / 10) - mel64| / b."""
        return self.figures(out, frontend)[0]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def edge_wav(B, L, seed):
    """Seeded randn at amplitude 0.5; the first and the last sample of every clip +0.9 / -0.9: a shifted or edge-repeating
    reflect shows."""
    w = 0.5 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))
    w[:, 0] = 0.9
    w[:, -1] = -0.9
    return w


def signal_wav(seed=4000):
    """(2, 4000): a 1 kHz tone (bin 32) and a tone halfway between bins 100 and 101, amplitude 0.5, each over white noise 40 dB
    below it."""
    n = torch.arange(4000, dtype=torch.float64)
    f = torch.tensor([1000.0, 100.5 * 32000.0 / N_FFT], dtype=torch.float64)[:, None]
    tone = 0.5 * torch.sin(2.0 * np.pi * f * n / 32000.0)
    return (tone + 0.005 * torch.randn(2, 4000, generator=torch.Generator().manual_seed(seed)).double()).float()


# (B, L) -> what the shape reaches (test_gpu_frontend_shapes.py)
SHAPES = [(1, 513), (3, 639), (3, 640), (3, 641), (3, 1151), (3, 1152), (3, 1153), (2, 1472), (5, 7360), (1370, 1601),
          (1, 1984001)]
FFT_ONLY = {(1, 1984001)}                                    # the dense scratch of 6 201 frames is not worth the time
SIGNAL = "signal"


def band_table(melW):
    """start, len per mel bin as acx_finalize builds them: first to last non-zero weight."""
    nz = (melW != 0).numpy()
    start, length = np.zeros(MELS, int), np.zeros(MELS, int)
    for m in range(MELS):
        k = np.flatnonzero(nz[:, m])
        if k.size:
            start[m], length[m] = k[0], k[-1] - k[0] + 1
    return start, length


def mel_loop(melW):
    """Which filter loop logmel_kernel takes for this bank: "fast" (unrolled, zero-padded), "lds" (general loop over the LDS copy
    of the banded table) or "global"; and the tap count frontend_info reports."""
    start, length = band_table(melW)
    taps = max(1, int(length.sum()))
    g = np.arange(MELS) // 64
    cap = np.array(MEL_FAST_TAPS)[g]
    if bool((length <= cap).all()) and bool((start + cap <= BINS).all()):
        return "fast", taps
    return ("lds" if taps <= MEL_LDS else "global"), taps


def _fallback_variants(sd):
    import test_gpu_frontend_fallback as fb                 # the dense melW and the hamming buffers are that file's constructions
    return fb.variants(sd)


def variant_sd(sd, which):
    """The state dict of a bank / window variant (shares every other tensor with sd)."""
    if which == "shipped":
        return sd
    out = dict(sd)
    if which == "dense_melW":
        out[KM] = _fallback_variants(sd)["dense_melW"][0][KM]
        return out
    if which == "hamming":
        hv = _fallback_variants(sd)["hamming_window"][0]
        out[KR], out[KI] = hv[KR], hv[KI]
        return out
    W = sd[KM].clone()
    start, length = band_table(W)
    if which == "wide0":                                     # one band of lane group 0 (mel < 64) widened from 1 to 2 taps
        m = 5
        assert length[m] == 1 and W[start[m] + 1, m] == 0
        W[start[m] + 1, m] = 0.5 * W[start[m], m]
    elif which == "nyquist":                                 # mel 223: a triangle over bins 500 .. 512 (13 taps, start + 14 > 513)
        k = torch.arange(500, 513)
        W[:, 223] = 0.0
        W[500:513, 223] = (1.0 - (k - 506).abs().float() / 7.0) * sd[KM][:, 223].max()
    elif which == "zero_col":                                # a band of length 0: exactly the clamp value
        W[:, ZERO_COL] = 0.0
    else:
        raise KeyError(which)
    out[KM] = W
    return out


ZERO_COL = 100
BANKS = ["shipped", "wide0", "nyquist", "zero_col", "dense_melW"]
BANK_LOOP = {"shipped": "fast", "wide0": "lds", "nyquist": "lds", "zero_col": "fast", "dense_melW": "global"}
BANK_SHAPES = [(3, 1153), SIGNAL]


# Frame 0 of every clip is mirror-symmetric about sample 0 (reflect padding), and so is the last frame when L - 1 is a multiple of
# 320, as at L = 1 601: their spectra are real, |X| is a real Gaussian, and a one-tap mel band falls under 2 b with a chance of
# about 1e-5 per cell.  1 370 clips hold 175 000 such cells, so most seeds leave a few cells under 2 b at K = 64.  The seed of
# that case is the first of 1 .. 2 000 whose weakest cell keeps mel64 > 3 x 64 S -- found from the reference alone (float64 rfft
# of the two symmetric frames of every clip), before any kernel ran on it.
SEEDS = {(1370, 1601): 941}


def wav_for(shape):
    if shape == SIGNAL:
        return signal_wav()
    B, L = shape
    return edge_wav(B, L, seed=SEEDS.get(shape, 7 * L + B))


def shape_id(shape):
    return shape if isinstance(shape, str) else "%dx%d" % shape


@functools.lru_cache(maxsize=None)
def _synth_sd():
    from audioset_convnext_inf_amd import synth
    return synth.synth_state_dict(0)


@functools.lru_cache(maxsize=None)
def variant(which):
    return variant_sd(_synth_sd(), which)


@functools.lru_cache(maxsize=None)
def case(which, shape):
    """The case of (variant, shape) on the synthetic weights: computed once per process, shared by every test that needs it."""
    return FrontCase("%s %s" % (which, shape_id(shape)), variant(which), wav_for(shape), dense=shape not in FFT_ONLY)


def all_gpu_cases():
    """Every (variant, shape, frontends) the GPU file runs."""
    out = [("shipped", s, ("auto",) if s in FFT_ONLY else ("auto", "dense")) for s in SHAPES]
    out += [(b, s, ("auto", "dense")) for b in BANKS for s in BANK_SHAPES if (b, s) != ("shipped", (3, 1153))]
    out.append(("hamming", (3, 1153), ("auto", "dense")))
    return out


# ---- the pool / head tail --------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(B, H3) for H3 in (1, 2, 3, 4, 5, 7, 31) for B in (1, 3)] + [(70, 7)]


def pool_input(B, H3, seed):
    """Seeded randn (B, H3, 7, 768); one time row per clip raised by 4.0 in half of the channels.  The kernel's time phase p holds
    the rows p, p + 4, ...: the raised row is the last row of phase min(H3, 4) - 1, the last phase that holds a row and (with
    phase 3 whenever H3 is no multiple of 4) a shortest one -- the maximum comes from there."""
    x = torch.randn(B, H3, 7, 768, generator=torch.Generator().manual_seed(seed))
    x[:, pool_raised_row(H3), :, ::2] += 4.0
    return x


def pool_raised_row(H3):
    ph = min(H3, 4) - 1
    return ph + 4 * ((H3 - 1 - ph) // 4)


def pool_head(sd, x):
    """x NHWC (B, H3, 7, 768), in x's precision -> scene, logits, probs (oracle/ref_cpu.py forward_features' tail + head)."""
    cast = (lambda t: t.double()) if x.dtype == torch.float64 else (lambda t: t)
    y = x.mean(dim=2)
    y = y.max(dim=1).values + y.mean(dim=1)
    scene = F.layer_norm(y, (768,), cast(sd["norm.weight"]), cast(sd["norm.bias"]), 1e-6)
    logits = F.linear(scene, cast(sd["head_audioset.weight"]), cast(sd["head_audioset.bias"]))
    return {"scene": scene, "logits": logits, "probs": torch.sigmoid(logits)}


@functools.lru_cache(maxsize=None)
def pool_case(B, H3):
    """x and, per output, layer_ref.Case(float64 reference, noise32 of the same statement in fp32, {})."""
    import layer_ref as lr
    sd = _synth_sd()
    x = pool_input(B, H3, seed=100 * H3 + B)
    r64, r32 = pool_head(sd, x.double()), pool_head(sd, x)
    return x, {k: lr.Case(r64[k], float((r32[k].double() - r64[k]).abs().max()), {}) for k in r64}
