"""Cases, plans and the float64 reference of the depthwise-form tests (tests/test_dwconv_plan_cpu.py, tests/test_gpu_dwconv_forms.py);
a plain helper imported like layer_ref.py.

The column-streaming depthwise kernel (dwconv_col.hip) is 28 instantiations (4 widths x S0 = 0 .. 6) plus four for packed batches;
which one a launch gets follows from the batch, the clip height and `target_waves`.  The tables below fix (stage, B, H, target_waves)
with SMALL target_waves, so that tensors of a few hundred KB are cut into several segments; what each case reaches is asked from
the launcher's own arithmetic (acx_test_dwconv7_plan) and asserted on the CPU, not assumed here.

Reference and bound come from the reference alone: conv2d in float64 of the fp32 input and the stored fp32 weights, and -- an output
being the bias plus 49 sequential fused multiply-adds, one rounding each --

    |y - ref| <= g49 * (|b| + sum |x| |w|),    g49 = 49 u / (1 - 49 u),  u = 2^-24     (Higham, Accuracy and Stability, 3.1),

per element, by a second conv on absolute values."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi
import layer_ref as lr

DIMS = lr.DIMS
HOP = 320
MIN_SAMPLES = 7360                       # ACX_MIN_SAMPLES: 8 / 4 / 2 / 1 rows in stages 0 .. 3
UNITS = 6                                # wave columns per image row
U = 2.0 ** -24
G49 = 49 * U / (1 - 49 * U)
MAX_TENSOR_BYTES = 4 << 20
BLOCK = 1                                # the weights of stages.s.1


def width(s):
    return 56 >> s


# ---- plans -------------------------------------------------------------------------------------------------------------------------
def plan(s, B, H, tw):
    """(n_out, s0, k7, n_seg, n_items) of launch_dwconv_col, or None where it refuses the batch."""
    p = _ffi.AcxDwconv7Plan()
    if _ffi.lib().acx_test_dwconv7_plan(s, B, H, tw, ctypes.byref(p)) != 0:
        return None
    return (p.n_out, p.s0, p.k7, p.n_seg, p.n_items)


def plan_varlen(s, lengths, tw):
    p = _ffi.AcxDwconv7Plan()
    arr = (ctypes.c_int64 * len(lengths))(*lengths)
    _ffi.check(_ffi.lib().acx_test_dwconv7_varlen_plan(s, arr, len(lengths), tw, ctypes.byref(p)))
    return (p.n_out, p.s0, p.k7, p.n_seg, p.n_items)


def stage_height(L, s):
    T = L // HOP + 1
    return ((T + 4) // 4 + 1) >> s


def samples_for_h0(h0):
    """The shortest clip with h0 rows in stage 0 (h0 >= 8)."""
    return HOP * (4 * h0 - 9)


# ---- uniform cases: (stage, B, H, target_waves, second target_waves) ---------------------------------------------------------------
# target_waves = 12: 2 segments at W >= 28 (one wave per SIMD, at least 16 rows), 4 at W <= 14 (two per SIMD, at least 7 rows)
def _wide(s):
    return [
        (s, 2, 7, 12, 6),        # S0 = 5, k7 = 3 at the minimum of 16 rows
        (s, 2, 15, 12, 18),      # S0 = 4
        (s, 2, 16, 12, 18),      # S0 = 3
        (s, 2, 17, 12, 18),      # S0 = 2
        (s, 2, 18, 12, 18),      # S0 = 1
        (s, 2, 19, 12, 18),      # S0 = 0; the second segment reaches one row past the last clip
        (s, 2, 20, 12, 18),      # S0 = 6, k7 = 4
        (s, 3, 12, 12, 18),      # S0 = 0, n_out = 21: the last segment ends exactly on the last clip
        (s, 3, 19, 12, 24),      # S0 = 3, k7 = 5
        (s, 3, 27, 18, 12),      # three segments (n_items % 4 = 2), S0 = 5, k7 = 5
        (s, 8, 1, 12, 6),        # H = 1: n_out = 16 = 4 (H + 3); a group of seven steps spans three clips
        (s, 10, 2, 12, 18),      # H = 2
        (s, 8, 3, 12, 18),       # H = 3
        (s, 12, 4, 24, 12),      # H + 3 = 7 divides n_out = 21: every segment starts on a clip's first row
    ]


def _narrow(s):
    return [
        (s, 2, 6, 12, 6),        # S0 = 0, k7 = 1, three segments (n_items % 4 = 2)
        (s, 2, 13, 12, 6),       # S0 = 6, k7 = 2: the main loop runs zero times from here ...
        (s, 2, 15, 12, 6),       # S0 = 5
        (s, 2, 17, 12, 6),       # S0 = 4
        (s, 2, 19, 12, 6),       # S0 = 3
        (s, 2, 21, 12, 6),       # S0 = 2 ... to here
        (s, 2, 23, 12, 6),       # S0 = 1, k7 = 2
        (s, 2, 25, 12, 6),       # S0 = 0, k7 = 2
        (s, 3, 10, 12, 6),       # 36 stacked rows = 4 x 9: the last segment ends exactly on the last clip
        (s, 3, 27, 12, 24),      # S0 = 6, k7 = 4
        (s, 3, 37, 12, 24),      # k7 = 5
        (s, 8, 1, 12, 6),        # H = 1
        (s, 10, 2, 12, 6),       # H = 2
        (s, 8, 3, 12, 6),        # H = 3
        (s, 4, 4, 12, 6),        # H + 3 = 7 = n_out
    ]


UNIFORM_CASES = _wide(0) + _wide(1) + _narrow(2) + _narrow(3)
# `stats`: three shapes per stage (a subset of the above), both forms
STATS_CASES = [c for c in UNIFORM_CASES if (c[1], c[2]) in ((2, 17), (3, 27), (8, 1))]

# ---- packed cases: (stage, lengths in samples, target_waves) -------------------------------------------------------------------------
# heights in the case's own stage; the clip of MIN_SAMPLES has 8 >> stage rows
_PACKED_H = {
    0: [8, 11, 9, 13, 8, 15, 10],
    1: [4, 11, 9, 13, 5, 15, 10],
    2: [2, 5, 3, 7, 4, 9],
    3: [1, 5, 3, 7, 4, 9],
}
_PACKED_TW = {0: (12, 18, 24, 36), 1: (12, 18, 24, 36), 2: (6, 12, 24), 3: (6, 12, 24)}


def _packed_lengths(s):
    out = []
    for k, h in enumerate(_PACKED_H[s]):
        if h == 8 >> s:
            out.append(MIN_SAMPLES)
        else:
            # h rows in stage s: h0 in [h << s, (h << s) + (1 << s) - 1]; alternate the ends, a few samples past the shortest
            h0 = (h << s) + (((1 << s) - 1) if k % 2 else 0)
            out.append(samples_for_h0(h0) + 37 * k)
    return out


PACKED_CASES = [(s, tuple(_packed_lengths(s)), tw) for s in range(4) for tw in _PACKED_TW[s]]


# ---- geometry of a plan (restated for the coverage assertions only) --------------------------------------------------------------
def segment_starts(p, B, H):
    """First output row (stacked: clip * (H + 3) + row) of every segment."""
    n_out, _, _, n_seg, _ = p
    return [k * n_out for k in range(n_seg)]


def row_kind(v, B, H):
    """'first' / 'last' / 'inner' row of a clip, 'zero' between clips, 'past' the last clip."""
    Hp = H + 3
    if v >= B * Hp - 3:
        return "past"
    r = v % Hp
    if r >= H:
        return "zero"
    return "first" if r == 0 else ("last" if r == H - 1 else "inner")


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def weights(sd, s):
    return sd["stages.%d.%d.dwconv.weight" % (s, BLOCK)], sd["stages.%d.%d.dwconv.bias" % (s, BLOCK)]


@torch.no_grad()
def conv_ref(sd, s, x):
    """x NHWC fp32 -> (float64 conv NHWC, per-element bound NHWC)."""
    w, b = weights(sd, s)
    C = DIMS[s]
    xn = x.permute(0, 3, 1, 2).double()
    ref = F.conv2d(xn, w.double(), b.double(), padding=3, groups=C)
    mag = F.conv2d(xn.abs(), w.double().abs(), b.double().abs(), padding=3, groups=C)
    return ref.permute(0, 2, 3, 1).contiguous(), (G49 * mag).permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def conv_fp32(sd, s, x, w=None):
    wt, b = weights(sd, s)
    return F.conv2d(x.permute(0, 3, 1, 2), wt if w is None else w, b, padding=3, groups=DIMS[s]).permute(0, 2, 3, 1).contiguous()


def worst_ratio(y, ref, bound):
    """max over elements of |y - ref| / bound."""
    return float(((y.detach().cpu().double() - ref).abs() / bound).max())


@torch.no_grad()
def conv_head_row_lost(sd, s, x, p, seg):
    """fp32 conv2d, except that kernel row 6 is left out on the first six output rows of segment `seg`: what a kernel whose head
    steps took a kernel-row range one short would give."""
    B, H = x.shape[0], x.shape[1]
    wt, _ = weights(sd, s)
    w6 = wt.clone()
    w6[:, :, 6, :] = 0.0
    good, bad = conv_fp32(sd, s, x), conv_fp32(sd, s, x, w6)
    out = good.clone()
    hit = 0
    for v in range(seg * p[0], seg * p[0] + 6):
        n, r = divmod(v, H + 3)
        if n < B and r < H:
            out[n, r] = bad[n, r]
            hit += 1
    assert hit > 0
    return out


def packed_input(s, heights, seed):
    """The clips' rows of stage s back to back, (rows, W, C) fp32, and each clip as its own (1, h, W, C) view."""
    rows = sum(heights)
    x = torch.randn(rows, width(s), DIMS[s], generator=torch.Generator().manual_seed(seed))
    x[0, 0, :] = 3.0
    x[-1, -1, :] = -2.0
    clips, r0 = [], 0
    for h in heights:
        clips.append(x[r0:r0 + h][None])
        r0 += h
    return x, clips


# ---- the kernel's division, restated -------------------------------------------------------------------------------------------------
def umulhi_div(vv, Hp):
    """RESTATEMENT of dwconv7_col_kernel's row -> clip division: umulhi(vv, floor(2^32 / Hp) + 1), vv = v + 9 Hp as uint32."""
    magic = np.uint64((1 << 32) // Hp + 1)
    return (vv.astype(np.uint64) * magic) >> np.uint64(32)


def largest_batch(H):
    """The largest B that launch_dwconv_col accepts at this height, by bisection on the plan's refusal."""
    lo, hi = 1, (1 << 32) // ((H + 3) * (H + 3)) + 2
    assert plan(3, lo, H, 12) is not None and plan(3, hi, H, 12) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(3, mid, H, 12) is None:
            hi = mid
        else:
            lo = mid
    return lo
