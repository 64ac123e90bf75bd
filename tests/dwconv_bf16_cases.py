"""Cases, plans, the float64 reference and the check of the bf16 depthwise-form tests (tests/test_dwconv_bf16_plan_cpu.py,
tests/test_gpu_dwconv_bf16_forms.py); a plain helper imported like dwconv_cases.py.  Nothing in here comes from a kernel.

dwconv7_mfma_kernel (dwconv_mfma.hip), the depthwise conv of `bf16a`, cuts the stacked batch into segments of `rows` = 4 `steps`
output rows.  `steps` decides which of the kernel's paths a launch takes: whether its 16-row ring wraps (from 3 steps on), after
which copy of the step its loop leaves (the parity of steps + 1), how far the scalar cursors walk.  On a 256-CU device the shipped
setting gives 2 steps on every tensor a quick test can afford, so the tables below fix (B, H, target_waves) with SMALL target_waves;
what each case reaches is asked from the launcher's own arithmetic (acx_test_dwconv7_bf16_plan) and asserted on the CPU.  The
arithmetic is the same in stages 0-2 (12 waves per segment, three groups per two workgroups), so one table serves all three.

Reference: conv2d in float64 of the bf16 input, the weights rounded to bf16 and the fp32 bias.  Check: the kernel's products are
exact (8 x 8 significand bits), its fp32 accumulation adds 50 terms -- the bias and 49 products -- in some order, so whatever the
order (Higham, Accuracy and Stability, 4.2)

    |s32 - ref| <= E,    E = g50 * (|b| + sum |x||w|),    g50 = 50 u / (1 - 50 u),  u = 2^-24,

and the store rounds to nearest even, which is monotone:  bf16(ref - E) <= y <= bf16(ref + E)  element by element, nothing on top.
u = 2^-24 takes v_mfma_f32_4x4x4_16b_bf16 to round the sums it forms to nearest.  The alternative, u = 2^-23, is for an ISA text that
says it does not; none was found that does, so the tighter value stands.  It was fixed before the first device run."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi
import dwconv_cases as dc
import layer_ref as lr

DIMS = lr.DIMS
STAGES = (0, 1, 2)
BLOCK = dc.BLOCK                         # the weights of stages.s.1
U = 2.0 ** -24
G50 = 50 * U / (1 - 50 * U)
MAX_TENSOR_BYTES = 4 << 20
KGROUPS = {0: 2, 1: 4, 2: 8}             # RESTATEMENT of DwmGeom::kGroups, (slice, segment) groups per workgroup; checked against `grid`
KSLICES = {0: 3, 1: 6, 2: 12}            # RESTATEMENT of DwmGeom::kSlices; checked against `n_groups`
# the stage's B = 64, 10 s launch at 8 waves per CU on 256 CUs
PRODUCT = dict(B=64, target_waves=8 * 256)
PRODUCT_STEPS = {0: 24, 1: 13, 2: 7}
MIN_EXACT_SHARE = 0.95


def width(s):
    return 56 >> s


# ---- plans -------------------------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, p):
        self.rows, self.steps, self.n_seg, self.n_groups, self.grid, self.too_tall = p.rows, p.steps, p.n_seg, p.n_groups, p.grid, bool(p.too_tall)

    def __repr__(self):
        return "rows %d steps %d segments %d groups %d grid %d%s" % (self.rows, self.steps, self.n_seg, self.n_groups, self.grid,
                                                                      " REFUSED" if self.too_tall else "")


def plan(s, B, H, tw):
    """What launch_dwconv_mfma would launch, and whether its guard refuses the batch."""
    p = _ffi.AcxDwconv7Bf16Plan()
    _ffi.check(_ffi.lib().acx_test_dwconv7_bf16_plan(s, B, H, tw, ctypes.byref(p)))
    return Plan(p)


def plan_varlen(s, lengths, tw):
    p = _ffi.AcxDwconv7Bf16Plan()
    arr = (ctypes.c_int64 * len(lengths))(*lengths)
    _ffi.check(_ffi.lib().acx_test_dwconv7_bf16_varlen_plan(s, arr, len(lengths), tw, ctypes.byref(p)))
    return Plan(p)


# ---- uniform cases: (B, H, target_waves ...), the same in every stage ---------------------------------------------------------------
# steps / segments per target_waves in the comments; tests/test_dwconv_bf16_plan_cpu.py asserts what the list reaches
SHAPES = [
    (1, 5, (12,)),                       # B = 1, H + 3 = 8 = the minimum rows: 2 steps, one segment ending one row past Vt
    (1, 16, (12, 24)),                   # 4 / 1 ending exactly on Vt; 2 / 2 ending exactly on Vt, the second starting inside the clip
    (8, 2, (12, 24, 36, 48, 60)),        # H = 2: 10 / 1, 5 / 2, 4 / 3, 3 / 4, 2 / 5 (a grid of 8); starts on first, last and all three zero rows
    (7, 1, (12, 24, 36)),                # H = 1, H + 3 = one step: 7 / 1, 4 / 2, 3 / 3 ending 11 rows past Vt
    (4, 3, (12, 24)),                    # H = 3: 6 / 1, 3 / 2
    (7, 9, (12, 24, 36, 132)),           # 21 / 1, 11 / 2, 7 / 3, 2 / 11: a grid of 17 = 2 x 8 + 1
    (5, 18, (24, 60, 96)),               # 13 / 2, 6 / 5 (a grid of 8), 4 / 7
    (7, 24, (12, 24, 144)),              # 47 / 1, 24 / 2, 4 / 12: a grid of 18 = 2 x 8 + 2
]
CASES = [(s, B, H, tws) for s in STAGES for B, H, tws in SHAPES]

# ---- packed cases: the lengths of dwconv_cases.PACKED_CASES, target_waves for 2 steps, an odd count, at least 9 ---------------------
_PACKED_TW = {0: (144, 96, 24), 1: (144, 96, 24), 2: (72, 48, 12)}
PACKED = [(s, next(c[1] for c in dc.PACKED_CASES if c[0] == s), _PACKED_TW[s]) for s in STAGES]


# ---- geometry of a plan (restated for the coverage assertions only) --------------------------------------------------------------
def row_kinds(v, B, H):
    """What stacked row v is: {'first'}, {'last'}, {'inner'} (or first and last at H = 1), {'zero0' | 'zero1' | 'zero2'}, {'past'}."""
    Hp = H + 3
    if v >= B * Hp - 3:
        return {"past"}
    r = v % Hp
    if r >= H:
        return {"zero%d" % (r - H)}
    k = set()
    if r == 0:
        k.add("first")
    if r == H - 1:
        k.add("last")
    return k or {"inner"}


# ---- rounding ------------------------------------------------------------------------------------------------------------------------
def bf16_rne(v):
    """float64 -> the nearest bf16 (ties to even), as float64, in ONE rounding (v.to(bfloat16) rounds to fp32 first).  Normal range
    only: the sums here are far from bf16's subnormals and its overflow."""
    m, e = torch.frexp(v)                                # v = m 2^e, |m| in [0.5, 1)
    return torch.ldexp(torch.round(m * 256.0), e - 8)    # 8 significand bits; torch.round: half to even


def bf16_trunc(v32):
    """fp32 -> bf16 by dropping the low 16 bits: what a store without rounding would write."""
    return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def weights(sd, s):
    """(weights rounded to bf16, fp32 bias), both as stored types widened to fp32."""
    w, b = dc.weights(sd, s)
    return w.to(torch.bfloat16).float(), b


def seeded_input(s, B, H, seed):
    """randn * 2 rounded to bf16, NHWC; first and last pixel constant (layer_ref.seeded_input)."""
    return (lr.seeded_input(s, B, H, seed) * 2.0).to(torch.bfloat16)


@torch.no_grad()
def conv_ref(sd, s, xb, w=None):
    """xb NHWC bf16 -> (float64 conv NHWC, E NHWC)."""
    wt, b = weights(sd, s)
    wt = wt if w is None else w
    C = DIMS[s]
    xn = xb.double().permute(0, 3, 1, 2)
    ref = F.conv2d(xn, wt.double(), b.double(), padding=3, groups=C)
    mag = F.conv2d(xn.abs(), wt.double().abs(), b.double().abs(), padding=3, groups=C)
    return ref.permute(0, 2, 3, 1).contiguous(), (G50 * mag).permute(0, 2, 3, 1).contiguous()


class Reference:
    """ref, E and the interval [lo, hi] = [bf16(ref - E), bf16(ref + E)] of one input; `pinned`: where lo == hi, the check is an
    equality with the rounded exact sum."""

    def __init__(self, ref, E):
        self.ref, self.E = ref, E
        self.lo, self.hi = bf16_rne(ref - E), bf16_rne(ref + E)
        self.exact = bf16_rne(ref)
        self.pinned = self.lo == self.hi

    def pinned_share(self):
        return float(self.pinned.double().mean())

    def outside(self, y):
        """Mask of the elements of y (bf16, or fp32 holding bf16 values) outside their interval; NaN counts as outside."""
        v = y.detach().cpu().double()
        return ~((v >= self.lo) & (v <= self.hi))

    def exact_share(self, y):
        return float((y.detach().cpu().double() == self.exact).double().mean())


_refs = {}


def case_reference(sd, s, B, H):
    """(x bf16 NHWC, Reference) of a uniform case: computed once, shared, never modified."""
    key = (s, B, H)
    if key not in _refs:
        x = seeded_input(s, B, H, seed=61000 + 1000 * s + 17 * B + H)
        _refs[key] = (x, Reference(*conv_ref(sd, s, x)))
    return _refs[key]


_packed_refs = {}


def packed_reference(sd, s, lengths):
    """(x bf16 (rows, W, C), heights, Reference over the packed rows): every clip convolved on its own."""
    key = (s, lengths)
    if key not in _packed_refs:
        hs = [dc.stage_height(L, s) for L in lengths]
        x32, clips = dc.packed_input(s, hs, seed=62000 + 100 * s + len(hs))
        xb = (x32 * 2.0).to(torch.bfloat16)
        parts, r0 = [], 0
        for h in hs:
            parts.append(conv_ref(sd, s, xb[r0:r0 + h][None]))
            r0 += h
        _packed_refs[key] = (xb, hs, Reference(torch.cat([p[0][0] for p in parts]), torch.cat([p[1][0] for p in parts])))
    return _packed_refs[key]


@torch.no_grad()
def conv_fp32(sd, s, xb, w=None):
    """torch's fp32 conv2d of the same operands (exact products, fp32 sums in torch's order), NHWC fp32, not yet rounded."""
    wt, b = weights(sd, s)
    return F.conv2d(xb.float().permute(0, 3, 1, 2), wt if w is None else w, b, padding=3, groups=DIMS[s]).permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def conv_row_lost(sd, s, xb, n, r):
    """The rounded exact sum, except that kernel row 6 is left out on output row r of clip n."""
    wt, _ = weights(sd, s)
    w6 = wt.clone()
    w6[:, :, 6, :] = 0.0
    out = bf16_rne(conv_ref(sd, s, xb)[0])
    out[n, r] = bf16_rne(conv_ref(sd, s, xb[n:n + 1], w6)[0])[0, r]
    return out


# ---- the kernel's division, restated -------------------------------------------------------------------------------------------------
def umulhi_div(v, Hp):
    """RESTATEMENT of dwm_run's row -> clip division: umulhi(v, floor(2^32 / Hp) + 1), v as uint32."""
    magic = np.uint64((1 << 32) // Hp + 1)
    return (v.astype(np.uint64) * magic) >> np.uint64(32)


def guard_product(B, H):
    """RESTATEMENT of dw_mfma_too_tall's left side; the launcher refuses from 2^32 - 1 on."""
    Hp = H + 3
    return (2 * (B * Hp - 3) + 16 * Hp + 64) * Hp


def largest_batch(H):
    """The largest B that launch_dwconv_mfma accepts at this height, by bisection on the plan's refusal."""
    lo, hi = 1, (1 << 32) // ((H + 3) * (H + 3)) + 2
    assert not plan(2, lo, H, 12).too_tall and plan(2, hi, H, 12).too_tall
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(2, mid, H, 12).too_tall:
            hi = mid
        else:
            lo = mid
    return lo
