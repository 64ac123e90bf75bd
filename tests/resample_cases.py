"""Cases, float64 reference and error bound of the resampler's per-form tests, importable without a GPU.

The resampler (csrc/resample.hip, res_tile of csrc/device_common.h) forms output n = j nf + i of a clip as an fp32 FMA chain over
phase i's band of taps; a workgroup forms tiles of T = 256 per_thread consecutive outputs from an input span staged in LDS, and
res_plan picks per_thread = 4, 2 or 1 from the LDS budget.  tests/test_resample_cases_cpu.py holds this file to the library's host
side and shows that the bound has teeth; tests/test_gpu_resample_forms.py runs the cases on the device.

Nothing here calls acx_resample_taps or acx_resample_geometry: the band of a phase is found from the definition (include/acx.h),
every tap k of the dense kernel [0, 2 width + of) with |t_k| < 6, searched from the band's centre outwards.

The bound is derived, not measured.  The device evaluates  acc <- fma(h32_k, x_k, acc)  over the c taps of the band in ascending
k, with h32_k = the float64 tap rounded to fp32 once: |h32_k - h_k| <= u |h_k|, u = 2^-24, and every fma rounds once.  By the
standard analysis of a recursive sum of c products (Higham, Accuracy and Stability of Numerical Algorithms, 3.1) with one more
factor (1 + delta) for the tap's own rounding,
    |y_dev - y| <= gamma_{c+1} sum_k |h_k x_k|,      gamma_m = m u / (1 - m u).
Nothing in it comes from device output."""
import functools
import math

import numpy as np

U = 2.0 ** -24
MAX_RATE = 768000
MAX_TABLE = 1 << 22            # nf * max_band floats (kResMaxTable)
MAX_LDS = 56 * 1024            # bytes of staged input span (kResMaxLds)
THREADS = 256                  # kResThreads
MAX_GRID = 4096                # kResMaxGrid
MAX_CLIPS = 256                # ACX_MAX_VARLEN_CLIPS
ERR_ARG, ERR_UNSUPPORTED = -1, -6

# ---- the case table ---------------------------------------------------------------------------------------------------------------
# (orig, new) -> per_thread the pair has to reach.  The literal small rates sit on both sides of each form boundary (of / nf = 13 |
# 14 and 27 | 28, and 53, the last ratio before the refusal); the realistic pairs reach per_thread 2 through the model rate
# (sample_rate 448000 .. 768000) and 1 through new_freq=, upsample to targets other than 32000 Hz (nf = 441, 160, 96), and at
# 44101 -> 32000 a tile never spans a phase period (nf = 32000 > T).
BOUNDARY_PAIRS = {(13, 1): 4, (14, 1): 2, (27, 1): 2, (28, 1): 1, (53, 1): 1}
REALISTIC_PAIRS = {(768000, 32000): 2, (448000, 32000): 2, (48000, 1000): 1, (32000, 44100): 4, (44100, 48000): 4,
                   (44101, 32000): 4, (8000, 768000): 4}
PAIRS = {**BOUNDARY_PAIRS, **REALISTIC_PAIRS}
REFUSED = (54, 1)
FORM_PAIRS = {4: (13, 1), 2: (768000, 32000), 1: (48000, 1000)}      # one pair per form: fences, walk, batchings
WALK_CAPS = (1, 2, 3)
# the shipped grid's second sweep: 1 -> 4, N = 4 L outputs (always a multiple of four) in tiles of 1024: 4096 full tiles, one more
# full tile and one of eight outputs
BIG_PAIR, BIG_LENGTH = (8000, 32000), (4096 * 1024 + 1029 + 3) // 4
MODEL_FORM_RATE = 768000        # the per_thread = 2 form through sample_rate=: 0.5 s = 384000 samples in, 16000 out


def pair_id(pair):
    return "%d-%d" % pair


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def out_len(of, nf, L):
    return (nf * L + of - 1) // of


# ---- res_plan restated -----------------------------------------------------------------------------------------------------------
def geometry(of, nf):
    base = min(of, nf) * 0.99
    return base, int(math.ceil(6.0 * of / base))


def bands(of, nf, phases):
    """The band of each phase in `phases` from the definition: (first k of the searched grid, on[P, K], t[P, K], start, count).
    The grid is the centre of the band, k - width = i of / nf, and ceil(6 of / base) + 3 taps to either side; on = |t| < 6 inside
    the dense kernel.  The band is contiguous (asserted)."""
    phases = np.asarray(phases, dtype=np.int64)
    base, width = geometry(of, nf)
    reach = int(math.ceil(6.0 * of / base)) + 3
    kmax = 2 * width + of
    first = width + phases * of // nf - reach
    k = first[:, None] + np.arange(2 * reach + 2, dtype=np.int64)[None, :]
    t = (-phases[:, None] / nf + (k - width) / of) * base
    on = (np.abs(t) < 6.0) & (k >= 0) & (k < kmax)
    count = on.sum(axis=1)
    lead = np.argmax(on, axis=1)
    last = on.shape[1] - 1 - np.argmax(on[:, ::-1], axis=1)
    assert np.all(count >= 1) and np.all(last - lead + 1 == count), "a band is not one run of taps"
    assert np.all(lead >= 1) and np.all(last <= on.shape[1] - 2), "the searched grid is too narrow"
    return first, on, t, first + lead, count


def tap_values(of, nf, t, on):
    """h = (base / of) sinc(t) cos^2(pi t / 12) in float64, zero off the band"""
    base, _ = geometry(of, nf)
    pt = np.pi * t
    s = np.where(t == 0, 1.0, np.sin(pt) / np.where(t == 0, 1.0, pt))
    w = np.cos(pt / 12.0)
    return np.where(on, (base / of) * s * (w * w), 0.0)


def max_band(of, nf, chunk=1 << 16):
    return max(int(bands(of, nf, np.arange(p, min(nf, p + chunk)))[4].max()) for p in range(0, nf, chunk))


def plan(orig, new):
    """res_plan restated: dict(of, nf, width, max_band, per_thread, lds_bytes, outputs_per_tile, max_grid), or None where the
    library refuses the pair with ACX_ERR_UNSUPPORTED (the table of nf * max_band taps over 2^22, or no form whose span fits)."""
    of, nf = reduced(orig, new)
    base, width = geometry(of, nf)
    # a band is the integers of an open interval of length 12 of / base: at least ceil(12 of / base) - 1 of them
    if nf * (math.ceil(12.0 * of / base) - 1) > MAX_TABLE:
        return None
    mb = max_band(of, nf)
    if nf * mb > MAX_TABLE:
        return None
    for q in (4, 2, 1):
        span = (THREADS * q - 1) * of // nf + 2 * width + 4
        if span * 4 <= MAX_LDS:
            return dict(of=of, nf=nf, width=width, max_band=mb, per_thread=q, lds_bytes=span * 4, outputs_per_tile=THREADS * q,
                        max_grid=MAX_GRID)
    return None


@functools.lru_cache(maxsize=None)
def pair_plan(pair):
    return plan(*pair)


# ---- lengths and inputs ------------------------------------------------------------------------------------------------------------
def length_for(count, of, nf):
    """the shortest clip with at least `count` outputs"""
    return (count - 1) * of // nf + 1


def case_lengths(pair):
    """Input lengths of a pair, from its plan: output counts 1, 2, T - 1, T, T + 1 and 3 T + 5 -- where the ratio skips a count
    (upsampling: 8000 -> 768000 has multiples of 96 only), the reachable counts on both sides of it -- and input lengths 1,
    width - 1 and width + 1.  Sorted, without repeats."""
    p = pair_plan(pair)
    of, nf, T = p["of"], p["nf"], p["outputs_per_tile"]
    lengths = {1, p["width"] - 1, p["width"] + 1}
    for count in (1, 2, T - 1, T, T + 1, 3 * T + 5):
        L = length_for(count, of, nf)
        lengths.add(L)
        if out_len(of, nf, L) != count and L > 1:
            lengths.add(L - 1)
    return sorted(lengths)


def inputs(orig, L, seed):
    """the three kinds of tests/test_gpu_resample.py: noise, a 997 Hz tone, uniform noise scaled by 1e4"""
    rs = np.random.RandomState(seed)
    noise = rs.standard_normal(L).astype(np.float32)
    tone = np.sin(2 * np.pi * 997.0 * np.arange(L) / orig).astype(np.float32)
    loud = (1e4 * rs.uniform(-1, 1, L)).astype(np.float32)
    return {"noise": noise, "tone": tone, "loud": loud}


def cases(pair):
    """[(L, kind, x)] of a pair"""
    return [(L, kind, x) for L in case_lengths(pair) for kind, x in inputs(pair[0], L, seed=(L * 31 + pair[0]) % 9973).items()]


# ---- the float64 reference and the bound ----------------------------------------------------------------------------------------------
def reference(x, orig, new):
    """(y, mag, c): the float64 formula of include/acx.h over the reference's own band, sum |h_k x_k|, and the band length of
    each output."""
    x = np.asarray(x, dtype=np.float64)
    of, nf = reduced(orig, new)
    _, width = geometry(of, nf)
    L = len(x)
    N = out_len(of, nf, L)
    n = np.arange(N, dtype=np.int64)
    j, i = n // nf, n % nf
    phases, inv = np.unique(i, return_inverse=True)
    first, on, t, _, count = bands(of, nf, phases)
    h = tap_values(of, nf, t, on)
    y, mag = np.zeros(N), np.zeros(N)
    m0 = j * of + first[inv] - width
    xp = np.concatenate([x, [0.0]])                                  # slot L: the zero outside the clip
    for r in np.flatnonzero(on.any(axis=0)):
        m = m0 + r
        p = h[inv, r] * xp[np.where((m >= 0) & (m < L), m, L)]
        y += p
        mag += np.abs(p)
    return y, mag, count[inv]


def bound(mag, c):
    """gamma_{c+1} mag"""
    m = (c + 1) * U
    return m / (1.0 - m) * mag


def worst_ratio(got, ref):
    """max |got - y| / bound, with 0 / 0 = 0 (an output whose band holds no sample must be exactly zero); the index of the worst"""
    y, mag, c = ref
    err, b = np.abs(np.asarray(got, dtype=np.float64) - y), bound(mag, c)
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(ratio)) if len(ratio) else 0
    return (float(ratio[k]) if len(ratio) else 0.0), k


# ---- res_tile restated: the kernel's tile arithmetic on the CPU -------------------------------------------------------------------------
def tile_indices(p, nb, nt, start, count):
    """res_tile's index arithmetic for the tile of outputs nb .. nb + nt - 1 under plan p, with the bands (start, count) of the
    tile's phases i (tap coordinates): (lo, span, i, j, first staged index of each output)."""
    of, nf, width = p["of"], p["nf"], p["width"]
    jb = nb // nf
    ib = nb - jb * nf
    lo = nb * of // nf - width - 1
    span = (nb + nt - 1) * of // nf - lo + width + 2
    base_off = jb * of - lo
    ii = ib + np.arange(nt, dtype=np.int64)
    jj = ii // nf
    i = ii - jj * nf
    return lo, span, i, jb + jj, jj * of + (start - width) + base_off


def tile_phases(p, nb, nt):
    return (nb % p["nf"] + np.arange(nt, dtype=np.int64)) % p["nf"]


MUTATIONS = ("band_shift", "next_phase", "lo_off_by_one", "neighbour")


def emulate(x, pair, mutation=None, neighbour=None):
    """The kernel's computation of one clip on the CPU, tile by tile as res_tile forms it: the span staged from lo, every output
    an fp32 chain in ascending k -- per tap the float64 product-sum (exact products: 24 x 24 bits) rounded to fp32 -- over the
    reference's own band with its taps rounded to fp32 once.  mutation: one of MUTATIONS, none of which reads outside the
    staged span or the clip's neighbourhood:
      band_shift     every band applied one input sample late (x[m + 1] for x[m])
      next_phase     phase (i + 1) mod nf's band and taps used for phase i (the identity where nf = 1)
      lo_off_by_one  the span staged from lo - 1 and indexed as if from lo
      neighbour      `neighbour`'s samples where zeros belong, on both sides of the clip (a packed batch's other clips)"""
    assert mutation is None or mutation in MUTATIONS
    p = pair_plan(pair)
    of, nf, width, T = p["of"], p["nf"], p["width"], p["outputs_per_tile"]
    x = np.asarray(x, dtype=np.float32)
    L = len(x)
    N = out_len(of, nf, L)
    out = np.zeros(N, dtype=np.float32)
    pad = p["lds_bytes"] // 4 + 2
    if mutation == "neighbour":
        left, right = np.resize(neighbour, pad).astype(np.float64), np.resize(neighbour[::-1], pad).astype(np.float64)
    else:
        left = right = np.zeros(pad)
    line = np.concatenate([left, x.astype(np.float64), right])       # sample m of the clip at line[pad + m]
    for nb in range(0, N, T):
        nt = min(T, N - nb)
        ph = tile_phases(p, nb, nt)
        if mutation == "next_phase":
            ph = (ph + 1) % nf
        uniq, inv = np.unique(ph, return_inverse=True)
        first, on, t, start, count = bands(of, nf, uniq)
        h32 = tap_values(of, nf, t, on).astype(np.float32).astype(np.float64)
        lo, span, _, _, at = tile_indices(p, nb, nt, start[inv], count[inv])
        assert span * 4 <= p["lds_bytes"]
        if mutation != "next_phase":
            assert at.min() >= 0 and (at + count[inv]).max() <= span
        at = np.clip(at, 0, span - 1)                                 # (a mutated phase stays inside the span)
        src =lo - (1 if mutation == "lo_off_by_one" else 0) + (1 if mutation == "band_shift" else 0)
        s_in = line[pad + src:pad + src + span]
        assert len(s_in) == span
        acc = np.zeros(nt, dtype=np.float32)
        lead = start - first                                          # the band's first column of the grid, per unique phase
        for r in range(int(count.max())):
            live = r < count[inv]
            col = np.minimum(lead[inv] + r, on.shape[1] - 1)
            hv = np.where(live, h32[inv, col], 0.0)
            xv = s_in[np.minimum(at + r, span - 1)]
            acc = np.where(live, (acc.astype(np.float64) + hv * xv).astype(np.float32), acc)
        out[nb:nb + nt] = acc
    return out
