"""CPU: what tests/test_gpu_resample_forms.py rests on, shown without a device.

  1. res_plan restated in Python (resample_cases.plan) equals acx_test_resample_plan field by field -- on the case table, which
     reaches per_thread 4, 2 and 1 on both sides of each boundary and the refusal, and on a sweep of every of, nf <= 64 plus
     seeded coprime pairs up to 768000;
  2. res_tile's index arithmetic restated in numpy keeps every staged index of every output inside [0, span), at first outputs
     0, T, 7 T, tiles that begin inside a phase period, and the last tile of each case length;
  3. the bands and taps of acx_resample_taps equal the reference's own, which never reads them;
  4. the bound has teeth: the kernel's chain emulated on the CPU passes every case, and four mutations fail on every pair."""
import ctypes
import math
import random

import numpy as np
import pytest

from audioset_convnext_inf_amd import _ffi
import resample_cases as rc

FIELDS = ("of", "nf", "width", "max_band", "per_thread", "lds_bytes", "outputs_per_tile", "max_grid")


def lib_plan(orig, new):
    """acx_test_resample_plan -> (dict or None where refused, return code, message)"""
    out = _ffi.AcxResamplePlan()
    rc_ = _ffi.lib().acx_test_resample_plan(orig, new, ctypes.byref(out))
    if rc_ != 0:
        return None, rc_, _ffi.lib().acx_last_error().decode()
    return {k: getattr(out, k) for k in FIELDS}, 0, ""


def sweep_pairs():
    """every of, nf <= 64 (as rates: reduced by the plan), and 300 seeded coprime pairs up to 768000, half of them with both
    sides below 4096 so that most are supported"""
    pairs = [(a, b) for a in range(1, 65) for b in range(1, 65)]
    rng = random.Random(20240)
    while len(pairs) < 64 * 64 + 300:
        top = 4096 if len(pairs) % 2 else rc.MAX_RATE
        a, b = rng.randint(1, top), rng.randint(1, top)
        if math.gcd(a, b) == 1:
            pairs.append((a, b))
    return pairs


@pytest.fixture(scope="module")
def supported():
    """the sweep's supported reduced pairs with their plans, checked against the library on the way"""
    seen, reached = {}, {4: 0, 2: 0, 1: 0, None: 0}
    for orig, new in sweep_pairs():
        key = rc.reduced(orig, new)
        if key in seen:
            continue
        mine = rc.plan(orig, new)
        theirs, code, msg = lib_plan(orig, new)
        assert mine == theirs, (orig, new, mine, theirs, msg)
        if theirs is None:
            assert code == rc.ERR_UNSUPPORTED and "leaves the staged span" not in msg, (orig, new, code, msg)
            assert ("%d/%d" % key) in msg
        seen[key] = mine
        reached[mine and mine["per_thread"]] += 1
    assert all(reached.values()), reached
    print("plan sweep: %d reduced pairs; per_thread 4 / 2 / 1 / refused: %d / %d / %d / %d"
          % (len(seen), reached[4], reached[2], reached[1], reached[None]))
    return {k: v for k, v in seen.items() if v is not None}


# ---- 1. the plan -----------------------------------------------------------------------------------------------------------------
def test_plan_restated_equals_the_library_on_the_table():
    """Every pair of the table: the restated plan equals the library's field by field and has the form the table says; the forms
    4, 2 and 1, both sides of 13 | 14 and 27 | 28, 53, and the refusal of 54 are each reached."""
    forms = {}
    for pair, want in rc.PAIRS.items():
        mine = rc.plan(*pair)
        theirs, code, msg = lib_plan(*pair)
        assert code == 0 and mine == theirs, (pair, mine, theirs, msg)
        assert mine["per_thread"] == want and mine["outputs_per_tile"] == rc.THREADS * want and mine["max_grid"] == rc.MAX_GRID
        assert mine["lds_bytes"] <= rc.MAX_LDS
        forms.setdefault(want, []).append(pair)
        print("plan %6d -> %6d: of/nf = %d/%d width %d max_band %d per_thread %d lds %d B"
              % (pair + tuple(mine[k] for k in ("of", "nf", "width", "max_band", "per_thread", "lds_bytes"))))
    assert sorted(forms) == [1, 2, 4] and all(rc.FORM_PAIRS[q] in forms[q] for q in forms)
    assert [rc.PAIRS[(r, 1)] for r in (13, 14, 27, 28, 53)] == [4, 2, 2, 1, 1]
    theirs, code, msg = lib_plan(*rc.REFUSED)
    assert rc.plan(*rc.REFUSED) is None and theirs is None and code == rc.ERR_UNSUPPORTED and "54/1" in msg and "LDS" in msg
    print("plan %6d -> %6d: refused (%d): %s" % (rc.REFUSED + (code, msg)))
    # the statement of the forms: 4 up to 13, 2 from 14 to 27, 1 from 28 to 53, none from 54, at any integer ratio of / 1
    for r in range(1, 80):
        q = rc.plan(r, 1)
        assert (q and q["per_thread"]) == (4 if r <= 13 else 2 if r <= 27 else 1 if r <= 53 else None), r
    # the model rate reaches per_thread 2: 13 x 32 kHz is the last whole ratio of form 4, 14 x 32 kHz up to the API's maximum is 2
    assert rc.plan(416000, 32000)["per_thread"] == 4 and rc.plan(448000, 32000)["per_thread"] == 2
    assert rc.plan(rc.MAX_RATE, 32000)["per_thread"] == 2
    assert _ffi.lib().acx_test_resample_plan(44100, 32000, None) == rc.ERR_ARG
    assert lib_plan(0, 32000)[1] == rc.ERR_ARG and lib_plan(44100, 768001)[1] == rc.ERR_ARG


def test_plan_restated_equals_the_library_on_the_sweep(supported):
    assert len(supported) > 2000


def test_case_lengths_reach_the_tile_edges():
    """Every pair's lengths give the output counts 1, 2, T - 1, T, T + 1, 3 T + 5 (or, where the ratio skips one, the reachable
    counts on both sides) and hold the input lengths 1, width - 1 and width + 1."""
    for pair in rc.PAIRS:
        p = rc.pair_plan(pair)
        of, nf, T = p["of"], p["nf"], p["outputs_per_tile"]
        lengths = rc.case_lengths(pair)
        counts = sorted({rc.out_len(of, nf, L) for L in lengths})
        assert {1, p["width"] - 1, p["width"] + 1} <= set(lengths) and min(lengths) >= 1
        for want in (1, 2, T - 1, T, T + 1, 3 * T + 5):
            below, above = [c for c in counts if c <= want], [c for c in counts if c >= want]
            assert above, (pair, want)
            if of >= nf:
                assert want in counts, (pair, want)                       # downsampling reaches every count
            elif want >= rc.out_len(of, nf, 1):                           # (one sample in is ceil(nf / of) out: no clip has fewer)
                assert below, (pair, want)
                assert above[0] - below[-1] <= -(-nf // of), (pair, want, below[-1], above[0])
        print("lengths %6d -> %6d (T = %4d): inputs %s -> outputs %s" % (pair + (T, lengths, [rc.out_len(of, nf, L) for L in lengths])))
    of, nf = rc.reduced(*rc.BIG_PAIR)
    big = rc.plan(*rc.BIG_PAIR)
    N = rc.out_len(of, nf, rc.BIG_LENGTH)
    assert (of, nf) == (1, 4) and N >= 4096 * 1024 + 1029 and -(-N // big["outputs_per_tile"]) > big["max_grid"]


# ---- 2. res_tile's indices ---------------------------------------------------------------------------------------------------------
def check_tile(key, p, nb, nt):
    of, nf, width = p["of"], p["nf"], p["width"]
    ph = rc.tile_phases(p, nb, nt)
    uniq, inv = np.unique(ph, return_inverse=True)
    _, _, _, start, count = rc.bands(of, nf, uniq)
    lo, span, i, j, at = rc.tile_indices(p, nb, nt, start[inv], count[inv])
    n = nb + np.arange(nt, dtype=np.int64)
    assert np.array_equal(i, n % nf) and np.array_equal(j, n // nf), (key, nb)
    assert span * 4 <= p["lds_bytes"] <= rc.MAX_LDS, (key, nb, nt, span)
    assert at.min() >= 0 and (at + count[inv]).max() <= span, (key, nb, nt, int(at.min()), int((at + count[inv]).max()), span)
    # the staged index of tap r of output n holds input sample j of + k - width (s_in[e] = x[lo + e])
    assert np.array_equal(lo + at, j * of + start[inv] - width), (key, nb)
    # and the span is no wider than the samples the tile's bands can name: one spare word on each side at the most
    return int(at.min()), int(span - (at + count[inv]).max())


def test_tile_indices_stay_inside_the_staged_span(supported):
    """For every supported pair of the sweep and of the table: first outputs 0, T, 7 T, first outputs inside a phase period
    (ib != 0, which base_off exists for: nb = T when nf does not divide it, and the tile that holds output nf + 1 for nf > T), a
    full tile and short last tiles of 1, 2, T - 1 outputs, and the last tile of each case length of the table."""
    plans = dict(supported)
    plans.update({rc.reduced(*pair): rc.pair_plan(pair) for pair in rc.PAIRS})
    slack_lo, slack_hi, with_ib = 1 << 30, 1 << 30, 0
    for key, p in plans.items():
        T, nf = p["outputs_per_tile"], p["nf"]
        firsts = {0, T, 7 * T, (nf // T + 1) * T, (3 * nf + 1) // T * T}
        with_ib += any(nb % nf for nb in firsts)
        for nb in sorted(firsts):
            for nt in (T, 1, 2, T - 1):
                a, b = check_tile(key, p, nb, nt)
                slack_lo, slack_hi = min(slack_lo, a), min(slack_hi, b)
    for pair in rc.PAIRS:
        p = rc.pair_plan(pair)
        T = p["outputs_per_tile"]
        for L in rc.case_lengths(pair):
            N = rc.out_len(p["of"], p["nf"], L)
            nb = (N - 1) // T * T
            check_tile(pair, p, nb, N - nb)
    assert with_ib > len(plans) // 2
    print("tile indices: %d plans, %d with a tile that begins inside a phase period; least spare words in front of / behind the "
          "bands: %d / %d" % (len(plans), with_ib, slack_lo, slack_hi))


# ---- 3. the library's bands and taps against the reference's own ------------------------------------------------------------------------
# the rates of tests/test_gpu_resample.py, whose formula() is the reference of this file: its band lengths enter that test's bound
LEGACY_PAIRS = [(r, 32000) for r in (8000, 11025, 16000, 22050, 24000, 44100, 48000, 88200, 96000)]


@pytest.mark.parametrize("pair", sorted(set(rc.PAIRS) | set(LEGACY_PAIRS)), ids=rc.pair_id)
def test_library_bands_equal_the_reference_bands(pair):
    """acx_resample_taps' band of every phase is the reference's own, except taps the reference holds at |h| <= 2^-40 base / of
    (the window's zero at |t| = 6, where the two evaluations of |t| < 6 may fall on either side); every stored tap is within
    2^-24 |h| plus one float64 ulp of h of the float64 value (one rounding, and the last bit of two float64 evaluations)."""
    of, nf = rc.reduced(*pair)
    base, width = rc.geometry(of, nf)
    start, count, taps = _ffi.resample_taps(*pair)
    start, count, taps = np.array(start, dtype=np.int64), np.array(count, dtype=np.int64), np.array(taps, dtype=np.float32)
    first, on, t, rstart, rcount = rc.bands(of, nf, np.arange(nf))
    h = rc.tap_values(of, nf, t, on)
    k = first[:, None] + np.arange(on.shape[1])[None, :]
    theirs = (k >= start[:, None]) & (k < (start + count)[:, None])
    assert theirs.sum() == count.sum() == len(taps), "a stored band lies outside the reference's search grid"
    extra, missing = on & ~theirs, theirs & ~on
    assert not missing.any(), (pair, "the library stores a tap outside |t| < 6", int(missing.sum()))
    assert np.all(np.abs(h[extra]) <= 2.0 ** -40 * base / of), (pair, float(np.abs(h[extra]).max()))
    stored = np.zeros(on.shape)
    stored[theirs] = taps                                              # row-major: phase after phase, ascending k
    err = np.abs(stored - h)[theirs]
    assert np.all(err <= rc.U * np.abs(h[theirs]) + np.spacing(np.abs(h[theirs]))), (pair, float(err.max()))
    print("bands %6d -> %6d: %d phases, %d taps, %d held by the reference alone" % (pair + (nf, len(taps), int(extra.sum()))))


# ---- 4. the bound has teeth -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(pair, L, kind, x):
        if (pair, L, kind) not in made:
            made[(pair, L, kind)] = rc.reference(x, *pair)
        return made[(pair, L, kind)]
    return get


@pytest.mark.parametrize("pair", sorted(rc.PAIRS), ids=rc.pair_id)
def test_the_emulated_chain_is_inside_the_bound(refs, pair):
    worst = 0.0
    for L, kind, x in rc.cases(pair):
        ref = refs(pair, L, kind, x)
        got = rc.emulate(x, pair)
        assert got.shape == ref[0].shape
        ratio, at = rc.worst_ratio(got, ref)
        assert ratio <= 1.0, (pair, L, kind, at, ratio)
        worst = max(worst, ratio)
    print("emulation %6d -> %6d: worst error / bound %.3f" % (pair + (worst,)))


@pytest.mark.parametrize("mutation", rc.MUTATIONS)
def test_mutations_leave_the_bound_on_every_pair(refs, mutation):
    """Each mutation of the emulated kernel is outside the bound on every pair (next_phase on every pair with nf > 1: at nf = 1
    there is no other phase).  "Last tap dropped" is not among them: at these widths the edge tap of the cos^2 window lies below
    the rounding bound, and this test does not claim to see it."""
    for pair in sorted(rc.PAIRS):
        nf = rc.pair_plan(pair)["nf"]
        if mutation == "next_phase" and nf == 1:
            continue
        ratios = []
        for L, kind, x in rc.cases(pair):
            other = rc.inputs(pair[0], 4099, seed=L + 1)[kind]
            ratios.append(rc.worst_ratio(rc.emulate(x, pair, mutation, neighbour=other), refs(pair, L, kind, x))[0])
        failing = sum(r > 1.0 for r in ratios)
        finite = [r for r in ratios if r > 1.0 and np.isfinite(r)]
        print("mutation %-13s %6d -> %6d: outside the bound in %3d of %3d cases, error / bound from %.3g to %.3g there"
              % ((mutation,) + pair + (failing, len(ratios), min(finite), max(finite))))
        assert max(ratios) > 1.0, (mutation, pair)
        # every clip of a full tile or more shows it, whatever the input kind
        T = rc.pair_plan(pair)["outputs_per_tile"]
        big = [r for (L, _, _), r in zip(rc.cases(pair), ratios) if rc.out_len(*rc.reduced(*pair), L) >= T - 1]
        assert big and min(big) > 1.0, (mutation, pair, min(big))
