#!/usr/bin/env python
"""Generate tests/golden/g7_augment.npz by running the REFERENCE's own augmentation code on the CPU.

Runs only where the reference checkout is present.  Nothing of the reference is copied: the script loads its
pytorch/augmentations.py, pytorch/pytorch_utils.py (do_mixup) and utils/utilities.py (Mixup) from their files -- after registering a
stand-in for torchaudio.transforms.Resample, which augmentations.py imports for the "linear" stretch this project does not build
and which the image lacks (as make_goldens.py stubs its imports) -- calls them, and stores DATA only: small inputs, the parameters as
plan fields (gain in dB, roll, rate, shift) and the reference's outputs.

Waveform cases (L = 64 and L = 7360): SpeedPerturbation at the rates whose step is exact in binary (0.5, 0.8, 1.0, 1.6, 2.0) with
every alignment -- "random" with the offset recovered by re-seeding and replaying Pad.pad_align_random / Crop.crop_align_random's
draws; roll_augment at -50, 0, 49 and |roll| > L; pydub_augment at -7, 0 and 6 dB (the seed that draws the gain is searched);
composites in the reference's order.  The stretch and roll inputs are the ramp i + 0.25, so an output names the sample it was
gathered from (and the file compresses); the gain inputs are noise.  Then do_mixup on a (4, 1, 9, 224) map and get_lambda(8) at
alpha 0.5 and 1.0.

usage: python tests/golden/make_augment_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/audioset_convnext_inf"
RATES = (0.5, 0.8, 1.0, 1.6, 2.0)
ALIGNS = ("left", "right", "center", "random")


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _install_shims():
    ta, tr = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.transforms")

    class Resample:                                    # only the "linear" stretch constructs it
        def __init__(self, *a, **k):
            raise NotImplementedError("torchaudio stand-in")
    tr.Resample = Resample
    ta.transforms = tr
    sys.modules.setdefault("torchaudio", ta)
    sys.modules.setdefault("torchaudio.transforms", tr)


def _random_shift(L, n_out, seed):
    """Replays the draws of Pad.pad_align_random then Crop.crop_align_random after torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    missing = max(L - n_out, 0)
    left = torch.randint(low=0, high=missing + 1, size=()).item()
    if n_out > L:
        return torch.randint(low=0, high=n_out - L, size=()).item()
    return -left


def _fixed_shift(L, n_out, align):
    missing, diff = max(L - n_out, 0), max(n_out - L, 0)
    if align == "left":
        return 0
    if align == "right":
        return diff - missing
    return (diff // 2 + diff % 2) - (missing // 2 + missing % 2)


def _gain_seed(want, gain_augment=7):
    for seed in range(10000):
        torch.manual_seed(seed)
        if torch.randint(gain_augment * 2, (1,)).item() - gain_augment == want:
            return seed
    raise RuntimeError("no seed draws a gain of %d dB" % want)


def main():
    _install_shims()
    aug = _load("ref_augmentations", "pytorch/augmentations.py")
    pu = _load("ref_pytorch_utils", "pytorch/pytorch_utils.py")
    ut = _load("ref_utilities", "utils/utilities.py")
    rng = np.random.RandomState(7)
    out = {}
    cases = []          # (input key, gain_db, roll, rate, shift, output key)
    for L in (64, 7360):
        out["ramp_%d" % L] = (np.arange(L, dtype=np.float32) + np.float32(0.25))[None, :]
        out["noise_%d" % L] = rng.randn(1, L).astype(np.float32)

    def add(inp, gain_db, roll, rate, shift, y):
        key = "wave_out_%d" % len(cases)
        out[key] = y.numpy().astype(np.float32)
        cases.append((inp, gain_db, roll, rate, shift, key))

    for L in (64, 7360):
        ramp, noise = torch.from_numpy(out["ramp_%d" % L]), torch.from_numpy(out["noise_%d" % L])
        for rate in RATES:
            n_out = len(torch.arange(0, L, 1.0 / rate))
            for k, align in enumerate(ALIGNS):
                sp = aug.SpeedPerturbation(rates=(rate, rate), align=align, p=1.0)
                seed = 100 + k + int(rate * 10)
                torch.manual_seed(seed)
                y = sp(ramp)
                shift = _random_shift(L, n_out, seed) if align == "random" else _fixed_shift(L, n_out, align)
                add("ramp_%d" % L, 0, 0, rate, shift, y)
        for roll in (-50, 0, 49, L + 3, -(2 * L + 5)):
            add("ramp_%d" % L, 0, roll, 1.0, 0, aug.roll_augment(ramp, shift=roll))
        for gain in (-7, 0, 6):
            torch.manual_seed(_gain_seed(gain))
            add("noise_%d" % L, gain, 0, 1.0, 0, aug.pydub_augment(noise))
        # the composite, in the reference's order (convnext.py:288-295): gain, roll, speed
        for gain, roll, rate, align in ((-7, 49, 1.6, "right"), (6, -50, 0.8, "center")):
            torch.manual_seed(_gain_seed(gain))
            y = aug.pydub_augment(noise)
            y = aug.roll_augment(y, shift=roll)
            y = aug.SpeedPerturbation(rates=(rate, rate), align=align, p=1.0)(y)
            add("noise_%d" % L, gain, roll, rate, _fixed_shift(L, len(torch.arange(0, L, 1.0 / rate)), align), y)

    out["wave_input"] = np.array([c[0] for c in cases])
    out["wave_output"] = np.array([c[5] for c in cases])
    out["wave_gain_db"] = np.array([c[1] for c in cases], dtype=np.int64)
    out["wave_roll"] = np.array([c[2] for c in cases], dtype=np.int64)
    out["wave_rate"] = np.array([c[3] for c in cases], dtype=np.float64)
    out["wave_shift"] = np.array([c[4] for c in cases], dtype=np.int64)

    for alpha in (0.5, 1.0):
        out["lambda_alpha_%s" % alpha] = ut.Mixup(alpha).get_lambda(8)
    x = torch.from_numpy(rng.randn(4, 1, 9, 224).astype(np.float32))
    lam = ut.Mixup(0.5).get_lambda(4)
    out["mix_in"] = x.numpy()
    out["mix_lambda"] = lam
    out["mix_out"] = pu.do_mixup(x, torch.Tensor(lam)).numpy()        # (move_data_to_device: a float array becomes torch.Tensor)
    path = os.path.join(HERE, "g7_augment.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d waveform cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
