"""Augmented forwards: the reference's training-mode input transforms, applied on the GPU with the backbone frozen.

The reference fine-tunes with the model in train mode (finetune_audiocaps.py), so every forward sees, in this order:
  pydub_augment (augmentations.py:336-341), roll_augment (:344-351) and SpeedPerturbation (:278-329) on the waveform
  (convnext.py:288-295), SpecAugmentation on the bn0'd log-mel (convnext.py:205-210, 308-309) and do_mixup
  (pytorch_utils.py:20-36, convnext.py:312-313).
This module is the single statement of what the kernels of csrc/augment.hip compute.  Everything here runs on the host (numpy /
torch CPU, no GPU): the policy, the random draws (a PLAN: one small struct per clip, uploaded once and read by the kernels), and
the two host definitions augment_wave_host / augment_spec_host, which the kernels equal bit for bit.

The waveform composite.  Gain, roll, nearest-neighbour stretch and pad / crop (the reference's order) compose into one gather:
    out[i] = gain * in[(src(i + shift) - roll) mod L]   if 0 <= i + shift < n_out, else +0
    src(j) = min(L - 1, rint(j * step))                 evaluated in FLOAT64, ties to even
with step = 1 / rate, n_out = ceil(L / step) the stretched length, shift the crop's start (n_out > L) or minus the left padding
(n_out < L), roll reduced to 0 <= roll < L and gain the float32 of 10 ** (dB / 20).
The float64 positions are deliberate.  The reference forms them with a float32 `torch.arange(0, L, step)`, whose values are an
artefact of torch's CPU vectoriser: they follow an 8-lane "base + lane * step" scheme except for a handful of elements, and for
L = 32000 at rate 1.4999, 10636 of the 47997 values change when torch's thread count goes from 1 to 8 -- there is no single
reference result to equal.  At steps that are exact in binary (rate 0.5, 0.8, 1.0, 1.6, 2.0: step 2, 1.25, 1, 0.625, 0.5) every
scheme agrees, the ties at x.5 included (both round half to even); those rates are where this definition is pinned to the
reference (tests/golden/g7_augment.npz).

The draws.  draw_plan takes every random number from ONE torch CPU generator (None: the global one), in this order:
  1. clip by clip, the waveform draws of the clip, each only when its transform is on:
       gain   g = randint(0, 2 * gain_db) - gain_db                              (pydub_augment)
       roll   r = randint(-roll, roll)                                           (roll_augment)
       speed  u = rand() when speed_p < 1: the clip is stretched when u <= speed_p;
              rate = lo, or lo + rand() * (hi - lo) in float32 when lo < hi      (torch.distributions.Uniform.sample)
              "random" alignment: left padding = randint(0, missing + 1) -- drawn also when nothing is missing, as
              Pad.pad_align_random does -- and then, when the stretched clip is longer, crop start = randint(0, diff)
     (the reference draws gain and roll once per BATCH and the speed decision from Python's `random`; here every clip has its
     own, from the one generator)
  2. the time stripes of every clip, then the frequency stripes of every clip; per stripe distance = randint(0, width), then
     bgn = randint(0, total - distance).  This is torchlibrosa's DropStripes order (SpecAugmentation: the time dropper over the
     batch, then the frequency dropper), so with the waveform transforms off -- AugmentPolicy.reference() -- the same
     torch.manual_seed gives the stripes torchlibrosa would draw.  torchlibrosa is not installed where this was developed:
     that equality is stated here and NOT tested.
A stripe of length 0 is legal.  Masked elements become +0.0: the reference zeroes after bn0, not to the mean.
"""
import ctypes
import dataclasses
import math

import numpy as np
import torch

from .. import _ffi

MAX_STRIPES = _ffi.AUG_MAX_STRIPES
N_MELS = 224
HOP = 320
ALIGNS = ("left", "right", "center", "random")

WAVE_DTYPE = np.dtype([("step", "<f8"), ("n_out", "<i8"), ("shift", "<i8"), ("roll", "<i8"), ("gain", "<f4"),
                       ("reserved", "<i4")])                     # struct acx_wave_aug, 40 bytes
SPEC_DTYPE = np.dtype([("t_bgn", "<i4", (MAX_STRIPES,)), ("t_len", "<i4", (MAX_STRIPES,)), ("f_bgn", "<i4", (MAX_STRIPES,)),
                       ("f_len", "<i4", (MAX_STRIPES,))])        # struct acx_spec_aug, 64 bytes
assert WAVE_DTYPE.itemsize == ctypes.sizeof(_ffi.AcxWaveAug) and SPEC_DTYPE.itemsize == ctypes.sizeof(_ffi.AcxSpecAug)


def num_frames(L):
    """T, the log-mel frames of a clip of L samples (acx_num_frames)."""
    return int(L) // HOP + 1


@dataclasses.dataclass(frozen=True)
class AugmentPolicy:
    """What to draw.  The fields carry the reference's names; the defaults are "off" for the waveform transforms (the
    reference's constructor defaults) and the reference's SpecAugmentation (convnext.py:205-210).
    gain_db: pydub_augment's gain_augment (reference call: 7); roll: roll_augment's shift_range (50 samples);
    speed: None or (lo, hi) rates, with speed_p and speed_align (reference: SpeedPerturbation(rates=(0.5, 1.5), p=0.5), align
    "random"); time_stripes / time_width / freq_stripes / freq_width: SpecAugmentation's."""
    gain_db: int = 0
    roll: int = 0
    speed: tuple = None
    speed_p: float = 0.5
    speed_align: str = "random"
    speed_interpolation: str = "nearest"
    time_stripes: int = 2
    time_width: int = 64
    freq_stripes: int = 2
    freq_width: int = 28
    drop_path: float = 0.0

    @classmethod
    def reference(cls):
        """What the reference's default constructor does in train mode: SpecAugment only."""
        return cls()

    @classmethod
    def identity(cls):
        """Nothing: no waveform transform, no stripes."""
        return cls(time_stripes=0, freq_stripes=0)

    @property
    def has_wave(self):
        return bool(self.gain_db) or bool(self.roll) or self.speed is not None

    @property
    def has_spec(self):
        return self.time_stripes > 0 or self.freq_stripes > 0

    def check(self, L=None):
        """ValueError for a policy the kernels do not take; with L, also for a time_width the clip is too short for."""
        for name in ("gain_db", "roll", "time_stripes", "time_width", "freq_stripes", "freq_width"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError("%s must be an integer >= 0 (got %r)" % (name, v))
        if self.drop_path != 0.0:
            raise ValueError("DropPath (stochastic depth) is not part of the augmented forwards: the backbone is frozen")
        if self.speed_interpolation != "nearest":
            raise ValueError("speed_interpolation=%r: only the reference's default, \"nearest\", is built (the \"linear\" stretch "
                             "is torchaudio's Resample)" % (self.speed_interpolation,))
        if self.speed_align not in ALIGNS:
            raise ValueError("speed_align must be one of %s (got %r)" % (list(ALIGNS), self.speed_align))
        if self.speed is not None:
            if len(self.speed) != 2 or not 0.0 < float(self.speed[0]) <= float(self.speed[1]) or not math.isfinite(self.speed[1]):
                raise ValueError("speed must be None or (lo, hi) with 0 < lo <= hi (got %r)" % (self.speed,))
            if not 0.0 <= float(self.speed_p) <= 1.0:
                raise ValueError("speed_p must lie in [0, 1] (got %r)" % (self.speed_p,))
        for axis, n, w in (("time", self.time_stripes, self.time_width), ("freq", self.freq_stripes, self.freq_width)):
            if n > MAX_STRIPES:
                raise ValueError("%s_stripes = %d: at most %d stripes per axis (ACX_AUG_MAX_STRIPES)" % (axis, n, MAX_STRIPES))
            if n > 0 and w < 1:
                raise ValueError("%s_width must be at least 1 (got %d)" % (axis, w))
        if self.freq_stripes > 0 and self.freq_width > N_MELS:
            raise ValueError("freq_width = %d exceeds the %d mel bins" % (self.freq_width, N_MELS))
        if L is not None and self.time_stripes > 0 and self.time_width >= num_frames(L):
            raise ValueError("time_width = %d needs a clip of more than %d frames; this one has T = %d (%d samples)"
                             % (self.time_width, self.time_width, num_frames(L), int(L)))
        return self


class AugmentPlan:
    """The draws of one batch: host struct arrays `wave` (WAVE_DTYPE, (B,)) and `spec` (SPEC_DTYPE, (B,)), either None when
    the policy has no such transform, for B clips of L samples (T frames).  to(device) uploads them."""

    def __init__(self, B, L, wave=None, spec=None):
        self.B, self.L, self.T = int(B), int(L), num_frames(L)
        self.wave = None if wave is None else np.ascontiguousarray(wave, dtype=WAVE_DTYPE).reshape(self.B)
        self.spec = None if spec is None else np.ascontiguousarray(spec, dtype=SPEC_DTYPE).reshape(self.B)
        self.wave_dev = self.spec_dev = None

    def check(self):
        """acx_augment_plan_check on the host arrays (stripe bounds, roll, n_out and shift ranges); raises _ffi.AcxError."""
        _ffi.check(_ffi.lib().acx_augment_plan_check(self.B, self.L, None if self.wave is None else self.wave.ctypes.data,
                                                     None if self.spec is None else self.spec.ctypes.data))
        return self

    def to(self, device):
        """A copy whose wave_dev / spec_dev are uint8 tensors on `device` holding the structs (checked first)."""
        self.check()
        out = AugmentPlan(self.B, self.L, self.wave, self.spec)
        for name in ("wave", "spec"):
            a = getattr(self, name)
            if a is not None:       # from pinned memory, without blocking: a loop draws its next plan while the GPU works
                setattr(out, name + "_dev", torch.from_numpy(a.view(np.uint8).copy()).pin_memory().to(device, non_blocking=True))
        return out

    def __eq__(self, other):
        def same(a, b):
            return (a is None and b is None) or (a is not None and b is not None and a.tobytes() == b.tobytes())
        return isinstance(other, AugmentPlan) and (self.B, self.L) == (other.B, other.L) and same(self.wave, other.wave) \
            and same(self.spec, other.spec)

    __hash__ = None


def stretched_length(L, step):
    """n_out = ceil(L / step): the element count of the reference's torch.arange(0, L, step)."""
    return int(math.ceil(int(L) / float(step)))


def wave_entry(L, gain_db=0, roll=0, rate=1.0, shift=0):
    """One WAVE_DTYPE record from the reference's parameters: gain in dB, roll as x.roll takes it (any integer), the stretch rate
    and the offset (crop start, or minus the left padding)."""
    step = 1.0 / float(rate)
    return (step, stretched_length(L, step), int(shift), int(roll) % int(L), np.float32(10 ** (gain_db / 20)), 0)


_DRAW = torch.empty((1,), dtype=torch.int64)          # (the one-element results of the integer and the uniform draws)
_DRAW_F = torch.empty((1,), dtype=torch.float32)


def _randint(lo, hi, g):
    """torch.randint(lo, hi, (1,), generator=g) -- the same kernel, and so the same value, at half the call's overhead"""
    return _DRAW.random_(int(lo), int(hi), generator=g).item()


def _rand(g):
    """torch.rand((), generator=g) as a float32 scalar, likewise"""
    return np.float32(_DRAW_F.uniform_(0.0, 1.0, generator=g).item())


def draw_plan(policy, B, L, generator=None):
    """The AugmentPlan of B clips of L samples under `policy`; every draw comes from `generator` (a torch CPU generator; None:
    the global one) in the order of the module docstring.  identity() draws nothing and leaves the generator untouched."""
    policy.check(L)
    B, L, g = int(B), int(L), generator
    T = num_frames(L)
    wave = spec = None
    if policy.has_wave:
        entries = []
        if policy.speed is not None:
            lo, hi = np.float32(policy.speed[0]), np.float32(policy.speed[1])       # Uniform(lo, hi) holds float32 tensors
        for b in range(B):
            gain_db = roll = shift = 0
            rate = 1.0
            if policy.gain_db:
                gain_db = _randint(0, 2 * policy.gain_db, g) - policy.gain_db
            if policy.roll:
                roll = _randint(-policy.roll, policy.roll, g)
            if policy.speed is not None:
                apply = policy.speed_p >= 1.0 or float(_rand(g)) <= policy.speed_p
                if apply:       # (float32 scalars: a rounded difference, a rounded product, a rounded sum, as the tensor ops round)
                    rate = float(lo) if lo == hi else float(lo + _rand(g) * (hi - lo))
                    n_out = stretched_length(L, 1.0 / rate)
                    missing, diff = max(L - n_out, 0), max(n_out - L, 0)
                    if policy.speed_align == "random":
                        shift = -_randint(0, missing + 1, g)
                        if diff > 0:
                            shift = _randint(0, diff, g)
                    elif policy.speed_align == "right":
                        shift = diff - missing
                    elif policy.speed_align == "center":
                        shift = (diff // 2 + diff % 2) - (missing // 2 + missing % 2)
            entries.append(wave_entry(L, gain_db, roll, rate, shift))
        wave = np.array(entries, dtype=WAVE_DTYPE)
    if policy.has_spec:
        spec = np.zeros(B, dtype=SPEC_DTYPE)
        for bgn, length, n, width, total in (("t_bgn", "t_len", policy.time_stripes, policy.time_width, T),
                                             ("f_bgn", "f_len", policy.freq_stripes, policy.freq_width, N_MELS)):
            drawn = []
            for _ in range(B * n):
                distance = _randint(0, width, g)
                drawn.append((_randint(0, total - distance, g), distance))
            if n:
                drawn = np.array(drawn, dtype=np.int32).reshape(B, n, 2)
                spec[bgn][:, :n], spec[length][:, :n] = drawn[:, :, 0], drawn[:, :, 1]
    return AugmentPlan(B, L, wave, spec)


def mixup_lambdas(B, alpha, seed=1234, random_state=None):
    """The reference's Mixup(alpha, seed).get_lambda(B) (utils/utilities.py:251-270): float64 (B,), pairs lam, 1 - lam with lam
    from numpy's RandomState.beta.  random_state: a RandomState to continue instead of a fresh one (the reference keeps one
    for the whole run)."""
    if B < 0 or B % 2:
        raise ValueError("mixup pairs clips 2b and 2b + 1: the batch must be even (got %d)" % B)
    rs = np.random.RandomState(seed) if random_state is None else random_state
    out = []
    for _ in range(0, B, 2):
        lam = rs.beta(alpha, alpha, 1)[0]
        out += [lam, 1.0 - lam]
    return np.array(out)


def augment_wave_host(wave, plan):
    """The definition of augment_wave_kernel: (B, L) float32 -> (B, L) float32 under plan.wave (None: a copy)."""
    wave = np.ascontiguousarray(wave, dtype=np.float32)
    B, L = wave.shape
    if plan.wave is None:
        return wave.copy()
    if (B, L) != (plan.B, plan.L):
        raise ValueError("plan of %d clips of %d samples for a batch of shape %r" % (plan.B, plan.L, wave.shape))
    out = np.zeros_like(wave)
    i = np.arange(L, dtype=np.int64)
    for b in range(B):
        p = plan.wave[b]
        j = i + int(p["shift"])
        ok = (j >= 0) & (j < int(p["n_out"]))
        src = np.minimum(L - 1, np.rint(j.astype(np.float64) * np.float64(p["step"]))).astype(np.int64)
        k = (np.maximum(src, 0) - int(p["roll"])) % L
        out[b] = np.where(ok, np.float32(p["gain"]) * wave[b][k], np.float32(0.0))
    return out


def _masks(plan_spec, b, T):
    t, f = np.zeros(T, dtype=bool), np.zeros(N_MELS, dtype=bool)
    if plan_spec is not None:
        p = plan_spec[b]
        for s in range(MAX_STRIPES):
            t[int(p["t_bgn"][s]):int(p["t_bgn"][s]) + int(p["t_len"][s])] = True
            f[int(p["f_bgn"][s]):int(p["f_bgn"][s]) + int(p["f_len"][s])] = True
    return t, f


def augment_spec_host(feat, plan, lam=None):
    """The definition of augment_spec_kernel: (B, T, 224) float32 bn0'd log-mel -> the masked map (lam None), or the (B / 2, T,
    224) mix fl32(a * l0) + fl32(b * l1) of rows 2b and 2b + 1, each masked with its own stripes first.  plan: an AugmentPlan
    or None (no stripes); lam: (B,) values, rounded to float32 as the reference's device tensor holds them."""
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    if feat.ndim != 3 or feat.shape[2] != N_MELS:
        raise ValueError("expected (B, T, %d) features, got %r" % (N_MELS, feat.shape))
    B, T, _ = feat.shape
    spec = None if plan is None else plan.spec
    if spec is not None and (plan.B != B or plan.T != T):
        raise ValueError("plan of %d clips of %d frames for features of shape %r" % (plan.B, plan.T, feat.shape))
    masked = feat.copy()
    for b in range(B):
        t, f = _masks(spec, b, T)
        masked[b][t, :] = np.float32(0.0)
        masked[b][:, f] = np.float32(0.0)
    if lam is None:
        return masked
    lam = np.asarray(lam, dtype=np.float32).reshape(-1)
    if B % 2 or lam.shape[0] != B:
        raise ValueError("mixup pairs clips 2b and 2b + 1: %d clips with %d lambdas (expected an even batch, one lambda per clip)"
                         % (B, lam.shape[0]))
    return masked[0::2] * lam[0::2, None, None] + masked[1::2] * lam[1::2, None, None]


def _as_batch(clips):
    if isinstance(clips, torch.Tensor):
        if clips.dim() != 2:
            raise ValueError("expected a (n, samples) waveform tensor or a list of equal-length clips, got shape %r"
                             % (tuple(clips.shape),))
        return clips
    clips = list(clips)
    if not clips or any(not isinstance(c, torch.Tensor) or c.dim() != 1 for c in clips):
        raise ValueError("augmented fits take waveforms: a (n, samples) tensor or a list of 1-D tensors")
    if len({int(c.numel()) for c in clips}) != 1:
        raise ValueError("augmented forwards take clips of one length (variable-length batches are not augmented): got lengths "
                         "%s" % sorted({int(c.numel()) for c in clips}))
    return torch.stack(clips)


def augmented_embeddings(model, clips, target, policy, views=1, mixup_alpha=None, seed=0, batch_size=64, sample_rate=None):
    """`views` augmented passes over uniform-length clips -> (emb (rows, 768), soft_target (rows, N)): the rows fit_head takes.
    Every batch of every view gets its own plan from one generator seeded with `seed`; with mixup_alpha, its own lambdas from
    one RandomState(seed) (rows = views * n / 2; n and batch_size even), and the targets are mixed with the same lambdas in
    float32.  Without mixup the targets are repeated (rows = views * n)."""
    x = _as_batch(clips)
    n = int(x.shape[0])
    if isinstance(views, bool) or not isinstance(views, int) or views < 1:
        raise ValueError("views must be a positive integer (got %r)" % (views,))
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError("batch_size must be a positive integer (got %r)" % (batch_size,))
    if not isinstance(target, torch.Tensor) or target.shape[0] != n:
        raise ValueError("target must be a tensor with one row per clip (%d)" % n)
    if mixup_alpha is not None:
        if not float(mixup_alpha) > 0.0:
            raise ValueError("mixup_alpha must be positive (got %r)" % (mixup_alpha,))
        if n % 2 or batch_size % 2:
            raise ValueError("mixup pairs clips 2b and 2b + 1: the clip count and batch_size must be even (got %d, %d)"
                             % (n, batch_size))
        if target.dim() != 2:
            raise ValueError("mixup mixes (n, N) label rows; got a target of shape %r" % (tuple(target.shape),))
    g = torch.Generator().manual_seed(int(seed))
    rs = np.random.RandomState(int(seed))
    embs, tgts = [], []
    for _ in range(views):
        for b0 in range(0, n, batch_size):
            xb, tb = x[b0:b0 + batch_size], target[b0:b0 + batch_size]
            lam = None if mixup_alpha is None else mixup_lambdas(int(xb.shape[0]), mixup_alpha, random_state=rs)
            out = model.forward_augmented(xb, policy=policy, mixup_lambda=lam, what="scene", generator=g, sample_rate=sample_rate)
            embs.append(out["scene"])
            if lam is None:
                tgts.append(tb)
            else:
                l32 = torch.from_numpy(lam.astype(np.float32)).to(tb.device)
                tf = tb.to(torch.float32)
                tgts.append(tf[0::2] * l32[0::2, None] + tf[1::2] * l32[1::2, None])
    return torch.cat(embs), torch.cat(tgts)


def policy_of(name):
    """An AugmentPolicy from a command-line word: "reference", "identity" or "full" (the reference with all three waveform
    switches on: gain 7 dB, roll 50, speed (0.5, 1.5) at p = 0.5)."""
    if name == "reference":
        return AugmentPolicy.reference()
    if name == "identity":
        return AugmentPolicy.identity()
    if name == "full":
        return AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5))
    raise ValueError("unknown augmentation policy %r (expected reference, identity or full)" % (name,))
