"""References for the bf16 arithmetics ("bf16", "bf16a"), a plain helper imported like layer_ref.py.

  * emulations of one block and one downsample layer in the arithmetic of the bf16 kernels (mlp_fused_wide_bf16.hip, gemm_bf16.hip,
    dwconv_mfma.hip), built from oracle/ref_cpu.py: operands rounded to bf16 exactly where the kernels round them, wide
    accumulation, and a pluggable GELU -- exact erf, or a step-by-step restatement of the device form of the stage;
  * restatements of the two device GELUs of these arithmetics, every instruction's result rounded to fp32, with coefficients PINNED
    here as literals (tests/test_bf16_ref_cpu.py holds split_math.h against them):
        gelu2h      gelu2h_micro with gelu_k2h, degree 2, stages 0-2 (the fused kernels: the accumulator is z = 0.5 v)
        gelu3_unit  the degree-4 third form in the epilogue of gemm_bf16_kernel, stage 3
  * the bars of a case against its emulation ("Parity bars"), nothing of which comes from what a kernel produced:
      - a hard ceiling per element, EMU_TOL per layer, or ONE bf16 step of that element where the result is stored as bf16 and
        that is more (bf16 keeps 8 significant bits: the step of r is 2^(floor(log2 |r|) - 7), between 2^-8 |r| and 2^-7 |r|);
      - under it, a bar that follows the case (check_emulation): d_ref = |emulation(float32) - emulation(float64)|, what the
        reference's own choice of accumulation does to this case -- the two products in float32 or float64, and the LayerNorm's
        statistics as running fp32 sums or in float64 -- rounding-boundary flips of LayerNorm outputs and hidden values included.
        The device's accumulation order differs from both, a second independent draw of the same process.  Held with a margin
        of 4: the median over the elements; per row (a flip moves a whole row) the number of rows whose RMS deviation exceeds
        4 x the 90th / 99th percentile / maximum of d_ref's rows; and, where the result is stored as bf16, the number of stored
        values that differ at all.
"""
import numpy as np
import torch
import torch.nn.functional as F

import layer_ref as lr

DIMS, DEPTHS = lr.DIMS, lr.DEPTHS
EMU_TOL = 4e-3          # vs the bf16 emulation: activations O(1), one bf16 ulp of a hidden value is 2^-8 relative
DRIFT_LAYER_TOL = 6e-2  # one block / one downsample layer vs float64 (tests/test_gpu_bf16.py)
MARGIN = 4.0
ROW_LEVELS = (0.9, 0.99, 1.0)
ALPHA = 1e-4            # a correct kernel fails a count by chance once in 10 000 cases


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def ln_plain(x, C):
    return F.layer_norm(x, (C,), None, None, 1e-6)


def ln_running_fp32(x, C):
    """A plain fp32 LayerNorm (no weight, eps 1e-6) with RUNNING sums over the channels, every operation rounded to fp32: mean,
    then the sum of squared differences, then (a - mean) * (1 / sqrt(var + eps)) -- the formulation of the kernels' in-register
    LayerNorm.  torch's fp32 layer_norm sums in blocks and lands closer to float64; the running sums carry about sqrt(C) 2^-24
    and send about that many more values to the other bf16 neighbour.  float64 out."""
    a = x.float().numpy()
    f = np.float32
    s = np.zeros(a.shape[:-1], f)
    for c in range(C):
        s = s + a[..., c]
    mean = s * f(1.0 / C)
    d = np.zeros_like(s)
    for c in range(C):
        t = a[..., c] - mean
        d = (t.astype(np.float64) * t + d).astype(f)          # an FMA: one rounding
    rstd = f(1.0) / np.sqrt(d * f(1.0 / C) + f(1e-6))
    return torch.from_numpy((a - mean[..., None]) * rstd[..., None]).double()


def _ln_in(x, C, acc, ln_acc):
    """The LayerNorm of the emulations: in the precision of its input (the arithmetic of the emulation as tests/test_gpu_bf16.py
    always had it), or -- ln_acc -- with its statistics in the accumulation type of the pair: float64, or running fp32 sums."""
    if not ln_acc:
        return ln_plain(x, C)
    return ln_plain(x.double(), C) if acc == torch.float64 else ln_running_fp32(x, C)


def act_bf16(precision, s):
    """Stage s stores its activations (x in, depthwise output, x out) as bf16."""
    return precision == "bf16a" and s < 3


# ---- GELU forms ------------------------------------------------------------------------------------------------------------------
# c0, c1, c2 of gelu_k2h (split_math.h: degree-2 minimax fit, tools/lab/fit_gelu.py 2); the header multiplies them by 2, 4, 8 (the
# unit is z = 0.5 v).  PINNED: the restatement must not move with the source it checks.
GELU2H_C = (-1.140932559967041, -0.4882272183895111, -0.027643846347928047)
GELU2H_SCALE = (2.0, 4.0, 8.0)
GELU2H_CLAIM = 8.6e-5       # split_math.h: |gelu2h - gelu| <= 8.6e-5
GELU3_UNIT_SCALE = (2.0, 4.0, 8.0, 16.0, 32.0)


def _gelu2h_fp32(v, c=None, v_is_z=False):
    """gelu2h_micro step by step in the unit z = 0.5 v, every instruction's result rounded to fp32 (an FMA = one rounding).
    numpy in, numpy out; torch in, torch (float64) out.  c: other coefficients than the pinned ones, v_is_z: the argument taken as z
    itself (what a kernel that forgot to halve b1 or W1 would evaluate) -- both only for showing that the bars notice."""
    k = [lr._f32c(cj) * sj for cj, sj in zip(GELU2H_C if c is None else c, GELU2H_SCALE)]      # exact: powers of two
    z = lr._t64(v) * (1.0 if v_is_z else 0.5)
    r32 = lr._Round32(z)
    r32(z)
    a = z.abs()
    q = r32(a.mul(k[2]).add_(k[1]))                 # step 0
    r32(q.mul_(a).add_(k[0]))                       # step 1
    r32(q.mul_(a))                                  # step 2
    r32(q.exp2_())                                  # E
    assert not bool(torch.isnan(q).any())          # no inf * 0, no inf - inf on the way
    r32(q.neg_().add_(1.0))                         # step 3: 1 - E
    return lr._back(r32(q.mul_(a).add_(z)), v)


def _gelu3_unit_fp32(v):
    """gelu3_unit step by step: the steps of layer_ref._gelu3_fp32 at kh = 1, coefficients pre-multiplied by 2 .. 32 as the source
    writes them."""
    k = [lr._f32c(cj) * sj for cj, sj in zip(lr.GELU3_K, GELU3_UNIT_SCALE)]
    z = lr._t64(v) * 0.5
    r32 = lr._Round32(z)
    r32(z)
    a = z.abs()
    q = r32(a.mul(k[4]).add_(k[3]))
    for j in (2, 1, 0):
        r32(q.mul_(a).add_(k[j]))
    r32(q.mul_(a))
    r32(q.exp2_())
    assert not bool(torch.isnan(q).any())
    r32(q.neg_().add_(1.0))
    return lr._back(r32(q.mul_(a).add_(z)), v)


def _constants_in_source(start, pattern):
    import os
    import re
    src = open(os.path.join(lr.CSRC, "split_math.h")).read()
    body = src[src.index(start):]
    body = body[:body.index("\n}")]
    return body, re.findall(pattern, body)


def _gelu2h_constants_in_source():
    """((c0, 2), (c1, 4), (c2, 8)) as gelu_k2h carries them, and the value of kBf16FusedHalfW1, for the pin test."""
    _, m = _constants_in_source("GeluK3 gelu_k2h()", r"k\.k([0-2]) = (-?[0-9.]+)f \* ([0-9.]+)f;")
    assert [int(j) for j, _, _ in m] == [0, 1, 2]
    _, half = _constants_in_source("constexpr bool kBf16FusedHalfW1", r"kBf16FusedHalfW1 = (\w+);")
    return tuple((float(c), float(s)) for _, c, s in m), half[0]


def _gelu3_unit_constants_in_source():
    """The five (coefficient, factor) pairs of gelu3_unit in the order k0 .. k4."""
    body, m = _constants_in_source("float gelu3_unit(", r"(-?[0-9.]+)f \* ([0-9.]+)f")
    assert len(m) == 5 and "z = 0.5f * v" in body     # the Horner order of the source: k4, k3, k2, k1, k0
    return tuple((float(c), float(s)) for c, s in reversed(m))


# which restatement belongs to which arithmetic, per stage (layer_ref.DEVICE_GELU keeps the fp32 arithmetics)
DEVICE_GELU = {p: (_gelu2h_fp32, _gelu2h_fp32, _gelu2h_fp32, _gelu3_unit_fp32) for p in ("bf16", "bf16a")}


def device_gelu(precision, s):
    return DEVICE_GELU[precision][s]


# ---- emulations ------------------------------------------------------------------------------------------------------------------
def _out(ref, acc, bf16_out):
    """What leaves the layer: the float64-accumulated emulation keeps its sum; the float32 one rounds it as the device's
    registers do; a bf16 store rounds either."""
    if acc == torch.float32:
        ref = ref.float()
    if bf16_out:
        ref = ref.float().to(torch.bfloat16)
    return ref.double()


@torch.no_grad()
def _block_emulation(precision, synth_sd, s, j, x0, store=True, acc=torch.float64, gelu=None, ln_acc=False):
    """Block j of stage s on x0 (NCHW fp32) in the arithmetic of the bf16 block kernels -> NHWC float64.  store=False: the block's
    result BEFORE it is stored (the last block of a stage hands it to the LayerNorm-rows epilogue in registers).  acc: the type the
    two matrix products accumulate in; float32 is the stand-in for the device, its result rounded to fp32 as the device's is.
    gelu: None = exact erf in fp32, or a restatement of a device form.  ln_acc: the LayerNorm's statistics follow acc (_ln_in)."""
    from oracle import ref_cpu
    C = DIMS[s]
    p = "stages.%d.%d." % (s, j)
    act = act_bf16(precision, s)                           # stored tensors of this stage are bf16: x in, y, x out
    if act:
        x0 = x0.to(torch.bfloat16).float()                 # what the block reads
    sd_dw = synth_sd
    if act:                                                # the matrix-pipe depthwise kernel multiplies bf16 weights (dwconv_mfma.hip)
        sd_dw = dict(synth_sd)
        sd_dw[p + "dwconv.weight"] = synth_sd[p + "dwconv.weight"].to(torch.bfloat16).float()
    y = ref_cpu.block_dwconv(sd_dw, s, j, x0).permute(0, 2, 3, 1)
    if act:
        y = y.to(torch.bfloat16).float()                   # the depthwise conv's output as stored
    # the arithmetic of the bf16 block kernels (mlp_fused_wide_bf16.hip; stage 3: run_mlp_bf16 in forward.hip): folds in
    # fp32/fp64, operands rounded to bf16, wide accumulation
    yn = bf(_ln_in(y, C, acc, ln_acc))
    w1 = bf((synth_sd[p + "pwconv1.weight"].double() * synth_sd[p + "norm.weight"].double()[None, :]).float())
    b1 = synth_sd[p + "pwconv1.bias"].double() + synth_sd[p + "pwconv1.weight"].double() @ synth_sd[p + "norm.bias"].double()
    v = ((yn.to(acc) @ w1.T.to(acc)).double() + b1).float()
    h = bf(F.gelu(v) if gelu is None else gelu(v))
    g = synth_sd[p + "gamma"].double()
    w2 = bf((g[:, None] * synth_sd[p + "pwconv2.weight"].double()).float())
    ref = x0.permute(0, 2, 3, 1).double() + (h.to(acc) @ w2.T.to(acc)).double() + g * synth_sd[p + "pwconv2.bias"].double()
    return _out(ref, acc, act and store)                   # ... and what it writes


@torch.no_grad()
def _downsample_emulation(synth_sd, i, x, acc=torch.float64, ln_acc=False):
    """downsample_layers[i] on x (NHWC) in the arithmetic of the bf16 kernels -> NCHW float64: LayerNorm in full precision, rows
    and folded weights rounded to bf16, wide accumulation (acc and ln_acc as in _block_emulation)."""
    Ci = DIMS[i - 1]
    p = "downsample_layers.%d." % i
    xn = bf(_ln_in(x, Ci, acc, ln_acc)).permute(0, 3, 1, 2)
    cw = synth_sd[p + "1.weight"].double()
    w = bf((cw * synth_sd[p + "0.weight"].double()[None, :, None, None]).float())
    b = synth_sd[p + "1.bias"].double() + (cw * synth_sd[p + "0.bias"].double()[None, :, None, None]).sum(dim=(1, 2, 3))
    return _out(F.conv2d(xn.to(acc), w.to(acc), None, stride=2).double() + b[None, :, None, None], acc, False)


# The pairs behind the bars: the same call accumulated in float64 and in float32, LayerNorm statistics included, with the device
# GELU of the stage restated.  x NHWC fp32 -> [emu64, emu32], NHWC.
ACCS = (torch.float64, torch.float32)


def block_pair(precision, synth_sd, s, j, x):
    return [_block_emulation(precision, synth_sd, s, j, lr.nchw(x), acc=a, gelu=device_gelu(precision, s), ln_acc=True) for a in ACCS]


def downsample_pair(synth_sd, i, x):
    return [_downsample_emulation(synth_sd, i, x, acc=a, ln_acc=True).permute(0, 2, 3, 1) for a in ACCS]


def tail_pair(precision, synth_sd, s, x):
    """The chain of acx_test_stage_tail -- the stage's last block without its final store, then the downsample conv; the result
    rounded to bf16 where the next stage stores bf16 activations."""
    outs = []
    for a in ACCS:
        x_new = _block_emulation(precision, synth_sd, s, DEPTHS[s] - 1, lr.nchw(x), store=False, acc=a,
                                 gelu=device_gelu(precision, s), ln_acc=True)
        e = _downsample_emulation(synth_sd, s + 1, x_new, acc=a, ln_acc=True).permute(0, 2, 3, 1)
        outs.append(_out(e, a, act_bf16(precision, s + 1)))
    return outs


# ---- bars ------------------------------------------------------------------------------------------------------------------------
def bf16_ulp(t):
    """The distance between neighbouring bf16 values at each element of t (float64): 2^(floor(log2 |t|) - 7)."""
    _, e = torch.frexp(t.abs())                             # |t| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t), e - 8)


def store_step(ref, stored):
    """One bf16 step of each element where the result is stored as bf16 (a stored value may round the other way when the fp32 sum
    sits at a rounding boundary), nothing elsewhere."""
    return bf16_ulp(ref) if stored else torch.zeros_like(ref)


def _quantile(t, q):
    t = t.reshape(-1)
    k = min(t.numel(), max(1, int(np.ceil(q * t.numel()))))
    return float(torch.kthvalue(t, k).values)


def _deviations(got, emu64, emu32, stored):
    """-> (|device - emu64|, the store's step, the device's deviation beyond that step, d_ref beyond that step), per element."""
    got = got.detach().cpu().double()
    step = store_step(emu64, stored)
    err = (got - emu64).abs()
    return err, step, (err - step).clamp_min_(0.0), ((emu32 - emu64).abs() - step).clamp_min_(0.0)


def _row_rms(t):
    return t.reshape(-1, t.shape[-1]).pow(2).mean(dim=1).sqrt()


def _count_allowed(n, p):
    """The largest count among n independent rows, each with probability p, that chance still explains: P(more) <= ALPHA."""
    from scipy.stats import binom
    return n if p >= 1.0 else int(binom.isf(ALPHA, n, p))


def check_emulation(name, got, emu64, emu32, stored, layers=1):
    """got: the device result; emu64 / emu32: the emulation of the same call accumulated in float64 / float32; stored: the result
    is stored as bf16; layers: EMU_TOL counts once per layer of the call.  Prints the figures, then asserts:
      ceiling   per element, layers x EMU_TOL or the element's bf16 step;
      median    of the deviation over the elements <= MARGIN x that of d_ref;
      rows      a rounding-boundary flip moves every channel of its pixel, so rows are what is drawn independently, and the tail of
                the deviation is held per row: r = RMS over the row's channels.  For each level of ROW_LEVELS, T = MARGIN x that
                quantile of r(d_ref) (1.0: its maximum); the device's rows with r > T are counted, and chance must explain the
                count if a row exceeds with probability MARGIN x (1 - level) (the maximum: MARGIN / (rows + 1), the chance that a
                further draw tops all rows of the first) -- a margin on the size and on the rate of what d_ref shows;
      share     stored results: most flips stay inside the store's step, so the number of stored values that differ at all is held
                to MARGIN x the reference's number, plus four standard deviations of a count that arrives in clusters of up to
                one row, plus one row.
    Returns the median ratio."""
    err, step, dev, dref = _deviations(got, emu64, emu32, stored)
    C, rows = emu64.shape[-1], emu64.numel() // emu64.shape[-1]
    worst = float((err / step.clamp_min(layers * EMU_TOL)).max())
    qd, qr = _quantile(dev, 0.5), _quantile(dref, 0.5)
    ratio = 0.0 if qd == 0.0 else (qd / qr if qr > 0.0 else float("inf"))
    fig = ["max |hip - emulation| / ceiling %.3f (max %.3g)" % (worst, float(err.max())),
           "median device %.3g / reference %.3g = %.2f" % (qd, qr, ratio)]
    rd, rr = _row_rms(dev), _row_rms(dref)
    over = []
    for level in ROW_LEVELS:
        t = MARGIN * _quantile(rr, level)
        k = int((rd > t).sum())
        allowed = _count_allowed(rows, MARGIN * (1.0 - level) if level < 1.0 else MARGIN / (rows + 1.0))
        fig.append("rows above %g x reference q%g (%.3g): %d of %d, allowed %d" % (MARGIN, 100 * level, t, k, rows, allowed))
        over.append(k > allowed)
    n_dev = n_ref = n_allowed = 0
    if stored:
        n_dev, n_ref = int((err > 0).sum()), int((emu32 != emu64).sum())
        n_allowed = int(MARGIN * n_ref + 4.0 * np.sqrt(MARGIN * max(n_ref, 1) * C) + C)
        fig.append("stored values that differ: device %d, reference %d, allowed %d of %d" % (n_dev, n_ref, n_allowed, err.numel()))
    print("%s: %s" % (name, "; ".join(fig)))
    failed = [what for what, bad in (("ceiling", worst > 1.0),    # (a stored value that rounds the other way is off by exactly its step)
                                     ("median", ratio > MARGIN), ("rows", any(over)), ("share", n_dev > n_allowed)) if bad]
    assert not failed, (name, failed, fig)
    return ratio


# ---- the GELU probe of tests/test_gpu_bf16_shapes.py, its CPU side ------------------------------------------------------------------
BOUNDARY_REL = 2.0 ** -18       # 64 fp32 steps of the value, and
BOUNDARY_ABS = 2.0 ** -20       # 16 fp32 steps of the row's scale (LN outputs are O(1)): the mean's rounding does not shrink with a small
EXCLUDED_CAP = 0.005            # output.  Both far above what an fp32 LayerNorm moves a value by (test_running_fp32_layernorm: under half of it, with running sums over 768 channels)


def near_bf16_boundary(t):
    """True where a float64 value lies within BOUNDARY_REL of itself, or BOUNDARY_ABS, of the midpoint of two neighbouring bf16
    values: there the device's fp32 LayerNorm may round the other way."""
    a = t.abs()
    step = bf16_ulp(a)
    frac = torch.remainder(a / step, 1.0)
    return (frac - 0.5).abs() * step < (BOUNDARY_REL * a).clamp_min(BOUNDARY_ABS)
