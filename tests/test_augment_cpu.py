"""CPU: the host side of the augmented forwards (pytorch/augment.py, acx_augment_plan_check and the argument checks of the
acx_augment_* / acx_forward_augmented calls, include/acx.h).

The host definitions augment_wave_host / augment_spec_host / mixup_lambdas against the outputs of the reference's own
augmentations.py, do_mixup and Mixup recorded in tests/golden/g7_augment.npz (bit for bit), hand-worked stripe cases, the draws,
and the refusals -- which need no GPU: every check comes before anything touches a device.  That draw_plan's stripes are
torchlibrosa's for the same seed is stated in augment.py's docstring and not tested: torchlibrosa is not a dependency."""
import ctypes
import os

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import augment as A
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_augment.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def wave_plan(L, entries):
    w = np.zeros(len(entries), dtype=A.WAVE_DTYPE)
    for b, e in enumerate(entries):
        w[b] = A.wave_entry(L, **e)
    return A.AugmentPlan(len(entries), L, w, None)


def spec_plan(B, L, stripes):
    """stripes: per clip {"t": [(bgn, len), ...], "f": [...]}"""
    s = np.zeros(B, dtype=A.SPEC_DTYPE)
    for b, d in enumerate(stripes):
        for axis in "tf":
            for k, (bgn, n) in enumerate(d.get(axis, ())):
                s[axis + "_bgn"][b, k], s[axis + "_len"][b, k] = bgn, n
    return A.AugmentPlan(B, L, None, s)


# ---- the host definitions against the reference's recorded outputs ---------------------------------------------------------
def test_fixture_covers_what_it_should(golden):
    rates, shifts, rolls, gains = golden["wave_rate"], golden["wave_shift"], golden["wave_roll"], golden["wave_gain_db"]
    assert set(rates.tolist()) == {0.5, 0.8, 1.0, 1.6, 2.0}
    assert {-50, 0, 49} <= set(rolls.tolist()) and any(abs(r) > 7360 for r in rolls.tolist())
    assert {-7, 0, 6} <= set(gains.tolist())
    assert (shifts > 0).any() and (shifts < 0).any()
    assert {golden[str(k)].shape[1] for k in golden["wave_input"]} == {64, 7360}
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_wave_host_equals_the_reference_bit_for_bit(golden):
    for i in range(len(golden["wave_input"])):
        x = golden[str(golden["wave_input"][i])]
        plan = wave_plan(x.shape[1], [dict(gain_db=int(golden["wave_gain_db"][i]), roll=int(golden["wave_roll"][i]),
                                           rate=float(golden["wave_rate"][i]), shift=int(golden["wave_shift"][i]))]).check()
        got, ref = A.augment_wave_host(x, plan), golden[str(golden["wave_output"][i])]
        assert got.dtype == np.float32 and got.tobytes() == ref.tobytes(), "case %d" % i


def test_mixup_host_and_lambdas_equal_the_reference(golden):
    got = A.augment_spec_host(golden["mix_in"][:, 0], None, golden["mix_lambda"])
    assert got.dtype == np.float32 and got.tobytes() == golden["mix_out"][:, 0].tobytes()
    for alpha in (0.5, 1.0):
        lam = A.mixup_lambdas(8, alpha)
        assert lam.dtype == np.float64 and np.array_equal(lam, golden["lambda_alpha_%s" % alpha])
        assert np.array_equal(lam[0::2] + lam[1::2], np.ones(4))
    with pytest.raises(ValueError, match="even"):
        A.mixup_lambdas(3, 0.5)


def test_wave_definition_by_hand():
    # L = 8, rate 2 (step 0.5, 16 stretched samples, ties at x.5 to even), crop from 3; then roll 2 and gain
    x = (np.arange(8, dtype=np.float32) + 1)[None]
    src = [0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 5, 6, 6, 6, 7, 7]           # rint(j / 2) clamped to 7
    got = A.augment_wave_host(x, wave_plan(8, [dict(rate=2.0, shift=3)]))[0]
    assert got.tolist() == [x[0][src[i + 3]] for i in range(8)]
    got = A.augment_wave_host(x, wave_plan(8, [dict(rate=2.0, shift=3, roll=2, gain_db=6)]))[0]
    g = np.float32(10 ** (6 / 20))
    assert got.tolist() == [g * x[0][(src[i + 3] - 2) % 8] for i in range(8)]
    # rate 0.5: 4 stretched samples 0, 2, 4, 6, padded by 3 on the left
    got = A.augment_wave_host(x, wave_plan(8, [dict(rate=0.5, shift=-3)]))[0]
    assert got.tolist() == [0, 0, 0, 1, 3, 5, 7, 0]


# ---- stripes by hand -------------------------------------------------------------------------------------------------------
def bits(T, seed=3):
    """A (1, T, 224) map of arbitrary float32 bit patterns (no NaNs: 0 * NaN would hide a mask)."""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((1, T, 224)) * 10.0 ** rs.randint(-20, 20, (1, T, 224))).astype(np.float32)


STRIPE_CASES = {
    "length_0": {"t": [(5, 0)], "f": [(7, 0)]},
    "bgn_0": {"t": [(0, 3)], "f": [(0, 2)]},
    "ends_at_T": {"t": [(29, 4)]},
    "ends_at_bin_223": {"f": [(200, 24)]},
    "overlapping": {"t": [(4, 6), (8, 5)], "f": [(10, 20), (25, 27)]},
    "none": {},
}


@pytest.mark.parametrize("name", sorted(STRIPE_CASES))
def test_stripes_by_hand(name):
    T, L = 33, 32 * 320
    d = STRIPE_CASES[name]
    x = bits(T)
    got = A.augment_spec_host(x, spec_plan(1, L, [d]).check())
    want = x.copy()
    for bgn, n in d.get("t", ()):
        want[0, bgn:bgn + n, :] = 0.0
    for bgn, n in d.get("f", ()):
        want[0, :, bgn:bgn + n] = 0.0
    assert got.tobytes() == want.tobytes()
    masked = sum(n for _, n in d.get("t", ())) + sum(n for _, n in d.get("f", ()))
    assert (got.tobytes() == x.tobytes()) == (masked == 0)
    assert not np.signbit(got[want == 0]).any()                       # +0.0, never -0.0


def test_masks_come_before_the_mix_and_each_clip_has_its_own():
    T, L = 33, 32 * 320
    x = np.concatenate([bits(T, 1), bits(T, 2)])
    plan = spec_plan(2, L, [{"t": [(0, 2)]}, {"f": [(100, 5)]}])
    lam = np.array([0.25, 0.75])
    got = A.augment_spec_host(x, plan, lam)
    a, b = x[0].copy(), x[1].copy()
    a[0:2] = 0.0
    b[:, 100:105] = 0.0
    assert got.shape == (1, T, 224) and got.tobytes() == (a * np.float32(0.25) + b * np.float32(0.75))[None].tobytes()
    with pytest.raises(ValueError, match="even"):
        A.augment_spec_host(x[:1], None, lam[:1])


# ---- draws -------------------------------------------------------------------------------------------------------------------
FULL = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5))


def test_draw_plan_is_a_function_of_the_generator_state():
    for policy in (A.AugmentPolicy.reference(), FULL, A.AugmentPolicy(speed=(0.9, 1.1), speed_p=1.0, speed_align="center")):
        p1 = A.draw_plan(policy, 6, 32000, torch.Generator().manual_seed(11))
        p2 = A.draw_plan(policy, 6, 32000, torch.Generator().manual_seed(11))
        p3 = A.draw_plan(policy, 6, 32000, torch.Generator().manual_seed(12))
        assert p1 == p2 and p1 != p3
        p1.check()
    torch.manual_seed(5)
    a = A.draw_plan(FULL, 3, 32000)
    torch.manual_seed(5)
    assert A.draw_plan(FULL, 3, 32000) == a              # generator=None: the global one


def test_drawn_stripes_and_offsets_stay_inside():
    g = torch.Generator().manual_seed(0)
    for L in (7360, 32000, 20801):                        # T = 24, 101, 66
        T = A.num_frames(L)
        policy = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=1.0, time_stripes=4, time_width=min(64, T - 1),
                                 freq_stripes=4, freq_width=28)
        for _ in range(20):
            p = A.draw_plan(policy, 8, L, g).check()
            s, w = p.spec, p.wave
            assert (s["t_bgn"] >= 0).all() and (s["t_len"] >= 0).all() and (s["t_bgn"] + s["t_len"] <= T).all()
            assert (s["t_len"] < policy.time_width).all() and (s["f_len"] < 28).all()
            assert (s["f_bgn"] >= 0).all() and (s["f_bgn"] + s["f_len"] <= 224).all()
            assert ((w["roll"] >= 0) & (w["roll"] < L)).all() and (w["step"] >= 1 / 1.5).all() and (w["step"] <= 2.0).all()
            assert (w["n_out"] == np.ceil(L / w["step"])).all()
            assert (np.minimum(w["n_out"] - L, 0) <= w["shift"]).all() and (w["shift"] <= np.maximum(w["n_out"] - L, 0)).all()


def test_reference_policy_draws_in_dropstripes_order():
    """time axis for every clip, then frequency for every clip; per stripe distance = randint(0, width), bgn = randint(0, total
    - distance) -- replayed here from the same seed."""
    B, L = 3, 32000
    T = A.num_frames(L)
    p = A.draw_plan(A.AugmentPolicy.reference(), B, L, torch.Generator().manual_seed(4))
    g = torch.Generator().manual_seed(4)
    for axis, width, total in (("t", 64, T), ("f", 28, 224)):
        for b in range(B):
            for s in range(2):
                distance = int(torch.randint(0, width, (1,), generator=g))
                bgn = int(torch.randint(0, total - distance, (1,), generator=g))
                assert (p.spec[axis + "_bgn"][b, s], p.spec[axis + "_len"][b, s]) == (bgn, distance)
    assert p.wave is None and (p.spec["t_len"][:, 2:] == 0).all()


def test_full_policy_draws_in_the_documented_order():
    """clip by clip gain, roll, the speed decision, the rate as Uniform(lo, hi).sample() forms it, the offsets as Pad / Crop draw
    them; then the stripes -- replayed with plain torch.randint / torch.rand from the same seed."""
    B, L = 5, 32000
    policy = A.AugmentPolicy(gain_db=7, roll=50, speed=(0.5, 1.5), speed_p=0.5, time_stripes=1, freq_stripes=0)
    p = A.draw_plan(policy, B, L, torch.Generator().manual_seed(17))
    g = torch.Generator().manual_seed(17)
    stretched = 0
    for b in range(B):
        gain = int(torch.randint(14, (1,), generator=g)) - 7
        roll = int(torch.randint(-50, 50, (1,), generator=g))
        rate, shift = 1.0, 0
        if float(torch.rand((), generator=g)) <= 0.5:
            rate = (torch.tensor(0.5) + torch.rand((), generator=g) * (torch.tensor(1.5) - torch.tensor(0.5))).item()
            n_out = len(torch.arange(0, L, 1.0 / rate, dtype=torch.float64))
            shift = -int(torch.randint(0, max(L - n_out, 0) + 1, (), generator=g))
            if n_out > L:
                shift = int(torch.randint(0, n_out - L, (), generator=g))
            stretched += 1
        want = np.array([A.wave_entry(L, gain, roll, rate, shift)], dtype=A.WAVE_DTYPE)
        assert p.wave[b:b + 1].tobytes() == want.tobytes(), b
    assert 0 < stretched < B
    for b in range(B):
        distance = int(torch.randint(0, 64, (1,), generator=g))
        assert (p.spec["t_len"][b, 0], p.spec["t_bgn"][b, 0]) == (distance, int(torch.randint(0, 101 - distance, (1,), generator=g)))


def test_identity_draws_nothing():
    g = torch.Generator().manual_seed(9)
    before = g.get_state().clone()
    p = A.draw_plan(A.AugmentPolicy.identity(), 4, 32000, g)
    assert p.wave is None and p.spec is None and torch.equal(g.get_state(), before)
    x = np.random.RandomState(0).randn(4, 32000).astype(np.float32)
    assert A.augment_wave_host(x, p).tobytes() == x.tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_policy_refusals():
    with pytest.raises(ValueError, match="T = 24"):
        A.draw_plan(A.AugmentPolicy.reference(), 2, 7360)                     # time_width 64 >= T
    with pytest.raises(ValueError, match="T = 65"):
        A.AugmentPolicy(time_width=65).check(64 * 320)
    A.AugmentPolicy(time_width=64).check(64 * 320)
    with pytest.raises(ValueError, match="at most 4"):
        A.AugmentPolicy(time_stripes=5).check()
    with pytest.raises(ValueError, match="linear"):
        A.AugmentPolicy(speed=(0.5, 1.5), speed_interpolation="linear").check()
    with pytest.raises(ValueError, match="DropPath"):
        A.AugmentPolicy(drop_path=0.1).check()
    with pytest.raises(ValueError, match="speed_align"):
        A.AugmentPolicy(speed=(0.5, 1.5), speed_align="middle").check()


def test_plan_check_refuses_through_the_c_abi():
    L, T = 32000, 101
    spec_plan(1, L, [{"t": [(T - 4, 4)], "f": [(196, 28)]}]).check()
    for d, msg in (({"t": [(T - 3, 4)]}, "time stripe 0 of clip 0"), ({"f": [(200, 25)]}, "frequency stripe 0"),
                   ({"t": [(-1, 2)]}, "time stripe")):
        with pytest.raises(_ffi.AcxError, match=msg):
            spec_plan(1, L, [d]).check()
    good = wave_plan(L, [dict(rate=1.6, shift=100)]).check()
    for field, value, msg in (("roll", L, "roll"), ("roll", -1, "roll"), ("n_out", 51201, "n_out"), ("shift", -1, "shift"),
                              ("shift", 19201, "shift"), ("step", 0.0, "step"), ("step", float("nan"), "step")):
        w = good.wave.copy()
        w[field][0] = value
        with pytest.raises(_ffi.AcxError, match=msg):
            A.AugmentPlan(1, L, w, None).check()
    with pytest.raises(_ffi.AcxError, match="shift"):
        wave_plan(L, [dict(rate=0.8, shift=1)]).check()                        # a padded clip shifts left only


def test_entry_points_refuse_before_touching_a_device():
    lib = _ffi.lib()
    fake = ctypes.c_void_p(4096)                # never dereferenced: every check below comes first
    with pytest.raises(_ffi.AcxError, match="must be even"):
        _ffi.check(lib.acx_augment_spec(fake, 3, 101, fake, fake, ctypes.c_void_p(8192), None))
    with pytest.raises(_ffi.AcxError, match="must be even"):
        _ffi.check(lib.acx_forward_augmented(None, fake, 3, 32000, None, None, fake, 0, fake, fake, fake, 1 << 20, None))
    with pytest.raises(_ffi.AcxError, match="too short"):
        _ffi.check(lib.acx_forward_augmented(None, fake, 2, 7359, None, None, None, 0, fake, fake, fake, 1 << 20, None))
    n = ctypes.c_size_t()
    with pytest.raises(_ffi.AcxError, match="too short"):
        _ffi.check(lib.acx_workspace_bytes_augmented(None, 2, 7359, 0, 0, 0, ctypes.byref(n)))
    with pytest.raises(_ffi.AcxError, match="bad mode"):
        _ffi.check(lib.acx_forward_augmented(None, fake, 2, 32000, None, None, None, 3, fake, fake, fake, 1 << 20, None))
    with pytest.raises(_ffi.AcxError, match="null pointer"):
        _ffi.check(lib.acx_forward_augmented(None, None, 2, 32000, None, None, None, 0, fake, fake, fake, 1 << 20, None))
    with pytest.raises(_ffi.AcxError, match="null context"):
        _ffi.check(lib.acx_forward_augmented(None, fake, 2, 32000, None, None, None, 0, fake, fake, fake, 1 << 20, None))
    with pytest.raises(_ffi.AcxError, match="null context"):
        _ffi.check(lib.acx_forward_features(None, fake, 2, 32000, 0, fake, fake, fake, 1 << 20, None))
    with pytest.raises(_ffi.AcxError, match="in place"):
        _ffi.check(lib.acx_augment_spec(fake, 2, 101, fake, None, ctypes.c_void_p(8192), None))
    with pytest.raises(_ffi.AcxError, match="out must not be feat"):
        _ffi.check(lib.acx_augment_spec(fake, 2, 101, fake, fake, fake, None))
    with pytest.raises(_ffi.AcxError, match="out must not be wav"):
        _ffi.check(lib.acx_augment_wave(fake, 2, 32000, fake, fake, None))


def test_struct_layouts():
    assert ctypes.sizeof(_ffi.AcxWaveAug) == 40 and ctypes.sizeof(_ffi.AcxSpecAug) == 64 and _ffi.AUG_MAX_STRIPES == 4
    for dt, st in ((A.WAVE_DTYPE, _ffi.AcxWaveAug), (A.SPEC_DTYPE, _ffi.AcxSpecAug)):
        for name in dt.names:
            assert dt.fields[name][1] == getattr(st, name).offset


def test_python_surface_refusals():
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56]).eval()
    target = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="waveform"):
        model.fit_head(torch.zeros(4, 768), target, augment=A.AugmentPolicy.reference())
    with pytest.raises(ValueError, match="waveform"):
        model.cross_validate_head(torch.zeros(4, 768), target, augment=A.AugmentPolicy.reference())
    with pytest.raises(ValueError, match="augment="):
        model.fit_head(torch.zeros(4, 768), target, views=2)
    with pytest.raises(ValueError, match="one length"):
        model.fit_head([torch.zeros(32000), torch.zeros(32001)], target[:2], augment=A.AugmentPolicy.reference())
    with pytest.raises(ValueError, match="segment"):
        model.forward_augmented(torch.zeros(2, 32000), what="segment")
    model.train()
    with pytest.raises(RuntimeError, match="model.eval"):
        model.forward_augmented(torch.zeros(2, 32000))
