"""Per-layer references for the GPU layer tests (tests/test_gpu_layer_shapes.py), a plain helper imported like parity_floor.py.

  * float64 restatements of one block, one downsample layer and the tail of a stage, built from oracle/ref_cpu.py, with a
    pluggable GELU: exact erf, or a step-by-step restatement of a device form (every instruction's result rounded to fp32);
  * the bar of a case, computed on the CPU from the references alone ("Parity bars"):

        bar = min(LAYER_TOL, 8 * noise32 + 2 * G)

    noise32 = max |fp32 oracle - fp64 oracle| on the same tensor: what the reference's own arithmetic does to this case.
    8: a split product carries two operand representation errors of 2^-23 and drops a lo * lo term of up to 2^-22 -- together
       2^-21 = 8 x the 2^-24 of one fp32 rounding (test_split_representation_error_bound).
    G = max |fp64 oracle with the exact GELU - fp64 oracle with the device form's restatement| on the same input.
    2: the polynomial's error oscillates, and the device evaluates it at pre-activations that differ from the oracle's in the
       last bits.
    Nothing in the bar comes from what a kernel produced;
  * a guarded device allocator: tensors inside larger buffers with canary words in front and behind, scratch prefilled with
    0xFF bytes (a NaN pattern), so that a store outside the tensor or a read of scratch nobody wrote is seen.
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

LAYER_TOL = 1e-4        # single layer, O(1) activations (tests/test_gpu_parity.py)
SPLIT_FACTOR = 8.0
GELU_FACTOR = 2.0
DIMS = (96, 192, 384, 768)
DEPTHS = (3, 3, 9, 3)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audioset-convnext-inf_amd", "csrc")


# ---- GELU forms ------------------------------------------------------------------------------------------------------------------
# The five coefficients of gelu3 (gelu_k3 in split_math.h) and the constants of gelu_erf (device_common.h: Abramowitz-Stegun 7.1.26,
# p, a1 .. a5 as published; 1 / sqrt 2 and log2(e) / 2 as the kernel writes them), PINNED here as literals: the restatements must not
# move with the sources they check.  tests/test_split_arithmetic_cpu.py holds the shipped header against GELU3_K.
GELU3_K = (-1.1510010957717896, -0.4595935642719269, -0.05214935168623924, 0.00719997426494956, -0.0004882981302216649)
AS_P, RSQRT2 = 0.3275911, 0.70710678
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
HALF_LOG2E = 0.72134752


def _gelu3_constants_in_source():
    """The coefficients as split_math.h carries them, for the pin test."""
    src = open(os.path.join(CSRC, "split_math.h")).read()
    body = src[src.index("GeluK3 gelu_k3("):]
    body = body[:body.index("return k;")]
    return tuple(float(m) for m in re.findall(r"k\.k[0-4] = (-?[0-9.]+)f \* s;", body))


def _t64(v):
    return v.double() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, np.float64))


class _Round32:
    """Rounds a float64 tensor to fp32 in place, through one fp32 buffer (a far-out polynomial value overflows to inf, as it does
    on the GPU).  The restatements below work in place: they run on tens of millions of pre-activations."""

    def __init__(self, like):
        self.buf = torch.empty(like.shape, dtype=torch.float32)

    def __call__(self, t):
        self.buf.copy_(t)
        return t.copy_(self.buf)


def _back(out, like):
    return out if isinstance(like, torch.Tensor) else out.numpy()


def _f32c(c):
    return float(np.float32(c))


def _gelu3_fp32(v, kh=1.0):
    """gelu3_nano step by step, every instruction's result rounded to fp32 (an FMA = one rounding), in the unit z = 0.5 kh v.
    numpy in, numpy out; torch in, torch (float64) out."""
    h = 0.5 * kh
    k = [c / h ** (j + 1) for j, c in enumerate(GELU3_K)]       # exact: h is a power of two
    assert all(abs(x) > 2.0 ** -126 and abs(x) < 2.0 ** 127 for x in k)
    z = _t64(v) * h
    r32 = _Round32(z)
    r32(z)
    a = z.abs()
    q = r32(a.mul(k[4]).add_(k[3]))
    for j in (2, 1, 0):
        r32(q.mul_(a).add_(k[j]))
    r32(q.mul_(a))
    r32(q.exp2_())                                  # E
    assert not bool(torch.isnan(q).any())          # no inf * 0, no inf - inf on the way
    r32(q.neg_().add_(1.0))                         # 1 - E
    r32(q.mul_(a).add_(z))
    return _back(q.div_(kh), v)


def _gelu_erf_fp32(v):
    """gelu_erf (device_common.h: A&S 7.1.26) step by step, every instruction's result rounded to fp32."""
    c = AS_A[::-1]                                  # a5 first: the Horner order of the kernel
    x = _t64(v).clone()
    r32 = _Round32(x)
    r32(x)
    av = x.abs()
    t = r32(av.mul(_f32c(np.float32(AS_P) * np.float32(RSQRT2))).add_(1.0))
    r32(t.reciprocal_())
    pl = r32(t.mul(_f32c(c[0])).add_(_f32c(c[1])))
    for cj in c[2:]:
        r32(pl.mul_(t).add_(_f32c(cj)))
    r32(pl.mul_(t))                                 # pl * t
    e = r32(x.mul(x))
    r32(e.mul_(-_f32c(HALF_LOG2E)))
    r32(e.exp2_())                                  # exp(-v^2 / 2)
    r32(pl.mul_(e))                                 # q
    return _back(r32(pl.mul_(av.mul_(-0.5)).add_(x.clamp_min_(0.0))), v)


def gelu_exact(v):
    return F.gelu(v)                                # 0.5 v (1 + erf(v / sqrt 2)) in the tensor's own precision


# which restatement belongs to which arithmetic
DEVICE_GELU = {"fp32": _gelu_erf_fp32, "fp32_split": _gelu3_fp32}


# ---- float64 restatements --------------------------------------------------------------------------------------------------------
def to64(sd):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}


def block_preact(sd, s, j, x):
    """x NCHW -> pwconv1's output, NHWC: Block.forward up to the GELU (oracle/ref_cpu.py block)."""
    from oracle import ref_cpu
    p = "stages.%d.%d." % (s, j)
    C = x.shape[1]
    y = ref_cpu.block_dwconv(sd, s, j, x).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (C,), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)
    return F.linear(y, sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"])


def block_finish(sd, s, j, x, g):
    """x NCHW, g = GELU(pre-activation) NHWC -> block output, NHWC."""
    p = "stages.%d.%d." % (s, j)
    return x.permute(0, 2, 3, 1) + sd[p + "gamma"] * F.linear(g, sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"])


def block(sd, s, j, x, gelu=gelu_exact):
    """One block, NCHW in, NHWC out, in the precision of sd / x, with the given GELU."""
    return block_finish(sd, s, j, x, gelu(block_preact(sd, s, j, x)))


class Case:
    """ref: float64 reference (NHWC); noise32; G per arithmetic."""

    def __init__(self, ref, noise32, G):
        self.ref, self.noise32, self.G = ref, noise32, G

    def bar(self, precision):
        return min(LAYER_TOL, SPLIT_FACTOR * self.noise32 + GELU_FACTOR * self.G.get(precision, 0.0))

    def check(self, name, got, precision):
        """got: the device result (NHWC).  Prints the figures, then asserts; returns error / bar."""
        err = float((got.detach().cpu().double() - self.ref).abs().max())
        bar = self.bar(precision)
        print("%s [%s]: |hip - fp64| = %.3g, noise32 %.3g, G %.3g, bar %.3g, ratio %.3f, max |ref| %.3g"
              % (name, precision, err, self.noise32, self.G.get(precision, 0.0), bar, err / bar, float(self.ref.abs().max())))
        assert err <= bar, (name, precision, err, bar)
        return err / bar


@torch.no_grad()
def block_case(sd, sd64, s, j, x32):
    """x32: NCHW fp32.  The exact-GELU float64 block, the fp32 oracle's deviation from it, and G for both device forms (the block
    is linear behind the GELU: G = max |gamma W2 (gelu - form)(h)|, one product per form and no second pass)."""
    from oracle import ref_cpu
    p = "stages.%d.%d." % (s, j)
    x64 = x32.double()
    h = block_preact(sd64, s, j, x64)
    g = gelu_exact(h)
    ref = block_finish(sd64, s, j, x64, g)
    noise32 = float((ref_cpu.block(sd, s, j, x32).permute(0, 2, 3, 1).double() - ref).abs().max())
    G = {}
    for prec, form in DEVICE_GELU.items():
        d = F.linear(form(h) - g, sd64[p + "pwconv2.weight"]) * sd64[p + "gamma"]
        G[prec] = float(d.abs().max())
    return Case(ref, noise32, G)


@torch.no_grad()
def downsample_case(sd, sd64, i, x32):
    from oracle import ref_cpu
    ref = ref_cpu.downsample(sd64, i, x32.double()).permute(0, 2, 3, 1)
    noise32 = float((ref_cpu.downsample(sd, i, x32).permute(0, 2, 3, 1).double() - ref).abs().max())
    return Case(ref, noise32, {})


@torch.no_grad()
def stage_tail_case(sd, sd64, s, x32):
    """downsample_layers[s + 1](last block of stage s (x)).  G through the same chain with the restated GELU: how the
    approximation propagates through the LayerNorm and the conv is measured on the reference."""
    from oracle import ref_cpu
    j = DEPTHS[s] - 1
    x64 = x32.double()

    def chain(sdx, x, gelu):
        return ref_cpu.downsample(sdx, s + 1, block(sdx, s, j, x, gelu).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    ref = chain(sd64, x64, gelu_exact)
    noise32 = float((chain(sd, x32, gelu_exact).double() - ref).abs().max())
    G = {prec: float((chain(sd64, x64, form) - ref).abs().max()) for prec, form in DEVICE_GELU.items()}
    return Case(ref, noise32, G)


def seeded_input(s, B, H, seed):
    """Seeded randn, NHWC fp32 at the stage's own width; first and last pixel constant (a shifted or wrapped window shows)."""
    C, W = DIMS[s], 56 >> s
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(seed))
    x[0, 0, 0, :] = 3.0
    x[-1, -1, -1, :] = -2.0
    return x


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- the documented split arithmetic, emulated ---------------------------------------------------------------------
def _split16(v):
    hi = v.to(torch.float16).float()
    return hi, (v - hi).to(torch.float16).float()


def _pow2_scale(w):
    return 2.0 ** (14 - int(np.floor(np.log2(float(w.abs().max())))))


def split_downsample(sd64, i, x32, drop=None):
    """downsample_layers[i] as fp32_split computes it, on the CPU: fp32 LayerNorm rows x 2^11 and the folded weights at their
    power-of-two scale as fp16 hi + lo, the three products W lo x A hi, W hi x A lo, W hi x A hi accumulated in fp32 (the order
    inside a product is torch's, not the kernel's).  x32 NCHW -> NHWC fp32.  drop = 0 | 1 | 2 leaves that product out: what a
    kernel that lost a term would compute -- for sizing bars and for showing that they notice."""
    p = "downsample_layers.%d." % i
    Ci = x32.shape[1]
    xn = F.layer_norm(x32.permute(0, 2, 3, 1), (Ci,), None, None, 1e-6)
    B, H, W, _ = xn.shape
    Ho, Wo = H // 2, W // 2
    a = xn[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, Ci).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * Ci)      # K order (kh, kw, c)
    cw = sd64[p + "1.weight"] * sd64[p + "0.weight"][None, :, None, None]
    w = cw.permute(0, 2, 3, 1).reshape(cw.shape[0], -1).float()
    b = (sd64[p + "1.bias"] + (sd64[p + "1.weight"] * sd64[p + "0.bias"][None, :, None, None]).sum(dim=(1, 2, 3))).float()
    ws = _pow2_scale(w)
    ah, al = _split16(a * 2048.0)
    wh, wl = _split16(w * ws)
    acc = torch.zeros(a.shape[0], w.shape[0])
    for t, (u, v) in enumerate(((ah, wl), (al, wh), (ah, wh))):
        if t != drop:
            acc = acc + u @ v.T
    return (acc * (1.0 / (2048.0 * ws)) + b).view(B, Ho, Wo, -1)


# ---- shapes (shared with tests/test_gpu_bf16.py) -------------------------------------------------------------------------------------
# (B, H) at the stage's own width 56 / 28 / 14 / 7 -> M pixels, around the tiles of the stage's kernels
BLOCK_SHAPES = {
    0: [(1, 1), (1, 5), (3, 3)],                 # 56: under one 16-pixel block group; 280 = 256 + 24; 504 = 2 x 256 - 8
    1: [(1, 1), (1, 5), (3, 3)],                 # 28: under one tile; 140 = 128 + 12; 252 = 4 x 64 - 4
    2: [(1, 1), (1, 5), (3, 3), (2, 37)],        # 14; 70 = 64 + 6; 126 = 128 - 2; 1 036 = 8 x 128 + 12
    3: [(1, 1), (1, 9), (1, 10), (1, 19), (1, 37), (3, 31)],     # 7; 63; 70; 133 = 128 + 5; 259 = 256 + 3; 651 = 2 x 256 + 139
}
# downsample inputs (B, H): odd H drops the last row; 7 .. 1 036 output rows, across 64 / 128 / 256
DOWN_SHAPES = [(1, 2), (1, 3), (3, 7), (2, 19), (1, 75)]


# ---- guarded device memory -------------------------------------------------------------------------------------------------------
CANARY = 0x5AC3A55A         # as a float: 2.75e16 -- a kernel that reads it does not get away with it either
GUARD_WORDS = 64            # 256 bytes on each side: the payload keeps the 256-byte alignment the ABI asks for


class Guarded:
    """nbytes of device memory inside a larger buffer: [256 B canary][payload, padded to 256 B with canary][256 B canary]."""

    def __init__(self, nbytes, device="cuda"):
        assert nbytes % 4 == 0
        self.words = nbytes // 4
        pad = (self.words + 63) // 64 * 64
        self.buf = torch.full((GUARD_WORDS + pad + GUARD_WORDS,), CANARY, dtype=torch.int32, device=device)
        assert not self.buf.is_cuda or self.buf.data_ptr() % 256 == 0          # (a device allocation: the ABI's alignment)
        self.payload = self.buf[GUARD_WORDS:GUARD_WORDS + self.words]

    @classmethod
    def tensor(cls, t, device="cuda"):
        """A tensor of t's type (float32, or a 16-bit payload such as bf16) with t's values inside a guarded buffer -> (guard, view)."""
        g = cls(t.numel() * t.element_size(), device)
        v = g.payload.view(t.dtype).view(t.shape)
        v.copy_(t)
        return g, v

    @classmethod
    def filled(cls, shape, value=float("nan"), device="cuda", dtype=torch.float32):
        g = cls(int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(), device)
        v = g.payload.view(dtype).view(shape)
        v.fill_(value)
        return g, v

    @classmethod
    def scratch(cls, nbytes, device="cuda", fill=0xFF):
        """Scratch prefilled with `fill` bytes -- 0xFF: NaN as fp32, fp16 and bf16; 0x7F: 3.4e38 as fp32 and bf16, NaN as fp16, a
        value no fmaxf drops -> (guard, uint8 view)."""
        g = cls((nbytes + 3) // 4 * 4, device)
        view = g.payload.view(torch.uint8)
        view.fill_(fill)
        return g, view

    def intact(self):
        front = self.buf[:GUARD_WORDS]
        back = self.buf[GUARD_WORDS + self.words:]
        return bool((front == CANARY).all()) and bool((back == CANARY).all())


def assert_clean(out, *guards):
    """After the call: every canary intact, no NaN / inf in the output."""
    for k, g in enumerate(guards):
        assert g.intact(), "canary of buffer %d overwritten" % k
    assert bool(torch.isfinite(out).all()), "NaN / inf in the output"
