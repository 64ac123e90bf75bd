"""Cases, references and bars of the stem tests (tests/test_gpu_stem_forms.py), importable without a GPU like dwconv_cases.py;
tests/test_stem_cases_cpu.py asserts, from the references alone, what the GPU cases rest on.

stem_kernel<OBF, VAR> (csrc/stem.hip) is four instantiations: fp32 or bf16 output, uniform or packed batch.  One arithmetic: per
channel the bias, then ky, kx ascending, one fused multiply-add per tap; a two-pass LayerNorm over the 96 channels (eps 1e-6 under
the square root); the affine as one fused multiply-add.  The forms differ in where a row's frames lie and in how a pixel is stored.

Reference: oracle/ref_cpu.py's stem in float64 on the float64 image of the state dict.  Bar: through layer_ref.Case
with G = {},  min(LAYER_TOL, 8 noise32),  noise32 = the larger of the distances from that reference of the fp32 oracle and of
chain32() below, the kernel's own chain restated with every instruction's result rounded to fp32.  Nothing comes from a kernel."""
import ctypes

import torch
import torch.nn.functional as F

import layer_ref as lr

MELS, W0, C0 = 224, 56, 96
HOP = 320
MIN_SAMPLES = 7360
MAX_BLOCKS = 2048                # launch_stem's grid cap (kStemMaxBlocks)
EPS = 1e-6

# (B, T).  T = 1 .. 5: H0 = 2, 2, 2, 3, 3 -- row 0 wholly in the zero padding in front, the last row partly (T = 1, 2, 3, 5) or
# wholly (T = 4) in the padding behind; (3, 23): 3 x 7 = 21 rows, pairs straddle clips; (1, 101): 27 rows, the last pair has one
# row; (2, 100): 2 x 27 = 54 rows, an even count
UNIFORM = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (3, 23), (1, 101), (2, 100)]
PROBE_SHAPE = (3, 23)            # the `offset` and `eps` inputs
# packed, in samples: H0 = 15, 8, 39, 39, 14, 20, 8 -- clip boundaries on odd rows after clips 0, 1 and 3, two equal neighbours, the
# minimum length, 143 rows in all (odd)
PACKED = (17000, 7360, 48000, 48000, 16000, 23000, 7361)
PACKED_H0 = (15, 8, 39, 39, 14, 20, 8)
# the walk: (1, 101) has 14 row pairs -- 14, 7 + 7 and 5 + 5 + 4 per workgroup under these caps; (33, 1005) at the launcher's own
# grid has 4175 > 2 x 2048 pairs
WALK_SHAPE, WALK_CAPS = (1, 101), (1, 2, 3)
BIG_SHAPE, BIG_DISTINCT = (33, 1005), 3


def frames(L):
    return L // HOP + 1


def h0(T):
    return (T + 4) // 4 + 1


def pairs(rows):
    return (rows + 1) // 2


def grid(npairs, max_blocks=0):
    cap = max_blocks if 0 < max_blocks < MAX_BLOCKS else MAX_BLOCKS
    return min(npairs, cap)


def walk(npairs, g):
    """Row pairs per workgroup: workgroup i of g takes pairs i, i + g, i + 2 g, ..."""
    return [(npairs - i + g - 1) // g for i in range(g)]


def loop_trips(npairs, g):
    """Trips of the kernel's outer loop (two pairs per trip) per workgroup.  From the second trip on, the first staging pair (pa*)
    is consumed after having been refilled inside the loop."""
    return [(n + 1) // 2 for n in walk(npairs, g)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def stem_input(B, T, seed, kind="randn3"):
    """(B, T, 224) fp32.  randn3: 3 randn, first and last frame constant (layer_ref.seeded_input's marks: a shifted or wrapped
    window shows); offset: randn + 50 -- with offset_state_dict() the mean of a pixel's 96 channels is far larger than their spread."""
    x = torch.randn(B, T, MELS, generator=torch.Generator().manual_seed(seed))
    if kind == "offset":
        return x + 50.0
    assert kind == "randn3"
    x = x * 3.0
    x[0, 0, :] = 3.0
    x[-1, -1, :] = -2.0
    return x


def seed_of(B, T):
    return 61000 + 1009 * B + T


EPS_SCALE, EPS_BIAS = 1e-3, 0.01


def eps_state_dict(synth_sd, scale=EPS_SCALE):
    """The eps probe: the stem conv's weight x `scale`, its bias constant -- var(y) over the channels is comparable to eps = 1e-6,
    so where eps enters (under the root, outside it, not at all) moves the output by tens of percent."""
    sd = {k: v.clone() for k, v in synth_sd.items()}
    sd["downsample_layers.0.0.weight"] = sd["downsample_layers.0.0.weight"] * scale
    sd["downsample_layers.0.0.bias"] = torch.full_like(sd["downsample_layers.0.0.bias"], EPS_BIAS)
    return sd


OFFSET_TAP = 28.0


def offset_state_dict(synth_sd, tap=OFFSET_TAP):
    """The variance probe.  The synthetic conv weights sum to about zero over the channels, so on them an input of randn + 50 moves
    the channels apart and leaves their mean near zero.  With `tap` added to every channel's LAST tap (ky = kx = 3) the same input
    puts 50 x tap on every channel of a pixel: its mean is some 30 times its spread, E[y^2] - mean^2 cancels ten bits, and only the
    final multiply-add of the chain works at that magnitude (a constant on all sixteen taps would round sixteen times there and
    push noise32 against the cap)."""
    sd = {k: v.clone() for k, v in synth_sd.items()}
    sd["downsample_layers.0.0.weight"][:, 0, 3, 3] += tap
    return sd


def packed_input(lengths, seed):
    """The clips' (T_i, 224) frames, each seeded on its own -> (all frames back to back, the list of (1, T_i, 224) clips)."""
    clips = [stem_input(1, frames(L), seed + 17 * i) for i, L in enumerate(lengths)]
    return torch.cat([c[0] for c in clips]), clips


# ---- references ----------------------------------------------------------------------------------------------------------------------
def _p(sd):
    return (sd["downsample_layers.0.0.weight"], sd["downsample_layers.0.0.bias"], sd["downsample_layers.0.1.weight"],
            sd["downsample_layers.0.1.bias"])


def conv(sd, x):
    """The stem's conv alone in the precision of sd / x: (B, T, 224) -> NHWC (B, H0, 56, 96)."""
    w, b, _, _ = _p(sd)
    return F.conv2d(x[:, None], w, b, stride=(4, 4), padding=(4, 0)).permute(0, 2, 3, 1)


def stem(sd, x):
    """oracle/ref_cpu.py's stem in the precision of sd / x, (B, T, 224) -> NHWC (B, H0, 56, 96)."""
    from oracle import ref_cpu
    return ref_cpu.stem(sd, x[:, None]).permute(0, 2, 3, 1).contiguous()


def patches(x):
    """(B, T, 224) -> (B, H0, 56, 16): output row h reads frames 4 h - 4 .. 4 h - 1 (zeros outside the clip), K order (ky, kx)."""
    B, T, _ = x.shape
    H = h0(T)
    xp = torch.zeros(B, 4 * H, MELS, dtype=x.dtype)
    n = min(T, 4 * H - 4)
    xp[:, 4:4 + n] = x[:, :n]
    return xp.view(B, H, 4, W0, 4).permute(0, 1, 3, 2, 4).reshape(B, H, W0, 16)


def stem_unfold(sd, x):
    """The same layer restated without conv2d: unfold, one matrix product, torch's layer_norm."""
    w, b, lw, lb = _p(sd)
    y = patches(x) @ w.reshape(C0, 16).T + b
    return F.layer_norm(y, (C0,), lw, lb, EPS)


def layer_norm(y, lw, lb, form="ref"):
    """LayerNorm over the last axis in the precision of y, in the form given: `ref` two passes, eps under the root; `no_eps`;
    `eps_outside`: sqrt(var) + eps; `one_pass`: var = E[y^2] - mean^2."""
    u = y.mean(-1, keepdim=True)
    if form == "one_pass":
        var = (y * y).mean(-1, keepdim=True) - u * u
    else:
        var = (y - u).pow(2).mean(-1, keepdim=True)
    den = {"ref": lambda: torch.sqrt(var + EPS), "one_pass": lambda: torch.sqrt(var + EPS), "no_eps": lambda: torch.sqrt(var),
           "eps_outside": lambda: torch.sqrt(var) + EPS}[form]()
    return (y - u) / den * lw + lb


def chain32(sd, x, form="ref"):
    """The kernel's chain in fp32, every instruction's result rounded to fp32 (layer_ref._Round32): per channel the bias, then
    ky, kx ascending, one fused multiply-add per tap (the product of two fp32 values is exact in float64); mean and variance in two
    passes, sums in fp32 (torch's order, not the kernel's butterfly), x 1/96; 1 / sqrt(var + eps); (a rstd) gw + gb as one fused
    multiply-add.  form as layer_norm's.  fp32 state dict and input -> NHWC fp32."""
    w, b, lw, lb = _p(sd)
    p = patches(x).double()
    w16 = w.reshape(C0, 16).double()
    acc = b.double().expand(p.shape[:3] + (C0,)).contiguous()
    r32 = lr._Round32(acc)
    for k in range(16):
        r32(acc.addcmul_(p[..., k:k + 1], w16[:, k]))
    a = acc.float()
    inv = torch.tensor(1.0 / 96.0, dtype=torch.float32)
    mean = a.sum(-1, keepdim=True) * inv
    if form == "one_pass":
        var = (a * a).sum(-1, keepdim=True) * inv - mean * mean
        a = a - mean
    else:
        a = a - mean
        var = (a * a).sum(-1, keepdim=True) * inv
    eps = torch.tensor(EPS, dtype=torch.float32)
    if form == "no_eps":
        rstd = 1.0 / torch.sqrt(var)
    elif form == "eps_outside":
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    t = (a * rstd).double()
    return r32(t.mul_(lw.double()).add_(lb.double())).float()


@torch.no_grad()
def stem_case(sd, sd64, x):
    """x (B, T, 224) fp32 -> layer_ref.Case: the float64 reference and noise32 = the larger of the fp32 oracle's and the restated
    chain's distance from it."""
    ref = stem(sd64, x.double())
    n_oracle = float((stem(sd, x).double() - ref).abs().max())
    n_chain = float((chain32(sd, x).double() - ref).abs().max())
    return lr.Case(ref, max(n_oracle, n_chain), {})


_cases = {}


def case(synth_sd, B, T, kind="randn3"):
    """(x, Case, state dict) of a uniform case, computed once per process, shared between the tests and never modified."""
    key = (B, T, kind)
    if key not in _cases:
        sd = {"eps": eps_state_dict, "offset": offset_state_dict}.get(kind, lambda d: d)(synth_sd)
        x = stem_input(B, T, seed_of(B, T), "offset" if kind == "offset" else "randn3")
        _cases[key] = (x, stem_case(sd, lr.to64(sd), x), sd)
    return _cases[key]


# ---- the packed geometry, from the library ---------------------------------------------------------------------------------------
def scratch_bytes(lengths):
    """(lengths as a C array, scratch bytes, stage-0 rows) from acx_test_stem_scratch_bytes: host arithmetic, no context."""
    from audioset_convnext_inf_amd import _ffi
    arr = (ctypes.c_int64 * len(lengths))(*lengths)
    need, rows = ctypes.c_size_t(), ctypes.c_int64()
    _ffi.check(_ffi.lib().acx_test_stem_scratch_bytes(arr, len(lengths), ctypes.byref(need), ctypes.byref(rows)))
    return arr, need.value, rows.value


def row_offsets(lengths):
    """First stage-0 row of every clip (and the total), as varlen_geometry counts the rows of each prefix of the batch."""
    return [0] + [scratch_bytes(lengths[:k])[2] for k in range(1, len(lengths) + 1)]


def half_step_bf16(ref, bar):
    """Half the distance between neighbouring bf16 values in the binade that a value within `bar` of ref can lie in."""
    _, e = torch.frexp(ref.abs() + bar)
    return 0.5 * torch.ldexp(torch.ones_like(ref), e - 8)


def bits(t):
    """The tensor's storage as integers: equality of bits, not of values (-0.0 and 0.0 differ, NaN equals itself)."""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

