#!/usr/bin/env python
"""Classifier heads of any size: the measurements behind profiles/r12_a_heads_bench.txt.

    python tools/heads_bench.py [--base-tree DIR] [--out profiles/r12_a_heads_bench.txt]

1. (--base-tree: a checkout of the parent commit with its libacx.so built) N = 527 bits: bench.py --dump-outputs of every
   precision and mode, run by the parent tree and by this one, compared byte for byte.  (ACX_LIB cannot select the parent's
   library here: this package binds acx_num_classes, which it lacks.)  Speed of the same pair: --speed-ab, the headline bench.py
   of each tree, alternating.
2. model(x) clips/s at bs 64, fp32_split, N in {50, 200, 4096, 16384} against the 527-class model (same backbone; the runs
   alternate, best of three rounds each).
3. The head at N = 16384: device time of the head kernels (class poolhead: pooling + head) as a share of the forward's, per-kernel
   event profile, and the weight bytes the class-tiled kernel reads (ceil(B / 16) x the head; estimated from its tiling).
4. The threshold between the two head paths: poolhead device time with the fused kernel (ACX_HEAD_PATH=1) and with pooling + the
   class-tiled kernel (ACX_HEAD_PATH=2) over N, at bs 1 and bs 64."""
import argparse
import filecmp
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                  # noqa: E402
import torch.nn as nn         # noqa: E402

from audioset_convnext_inf_amd import _ffi, synth      # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny      # noqa: E402

SR = 32000
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def tree_bench(tree, args):
    """bench.py of `tree` (its own package and libacx.so) in a fresh process; returns its JSON line."""
    env = dict(os.environ)
    env.pop("ACX_LIB", None)
    out = subprocess.check_output([sys.executable, os.path.join(tree, "bench.py")] + args, env=env, cwd=tree, timeout=300)
    return json.loads(out.decode().strip().splitlines()[-1])


def bits_ab(base_tree):
    ok_all = True
    for prec in ("fp32_split", "fp32", "bf16", "bf16a"):
        for mode in ("logits", "scene", "frame"):
            with tempfile.TemporaryDirectory() as d:
                dirs = {}
                for which, tree in (("base", base_tree), ("new", ROOT)):
                    out = os.path.join(d, which)
                    tree_bench(os.path.abspath(tree), ["--steps", "3", "--warmup", "1", "--mode", mode, "--precision", prec,
                                                       "--dump-outputs", out])
                    dirs[which] = out
                names = sorted(os.listdir(dirs["new"]))
                same = names == sorted(os.listdir(dirs["base"])) and all(
                    filecmp.cmp(os.path.join(dirs["base"], n), os.path.join(dirs["new"], n), shallow=False) for n in names)
                ok_all &= same
                say("   %-10s %-6s %s: %s" % (prec, mode, ", ".join(names), "byte-identical" if same else "DIFFERENT"))
    return ok_all


def model_n(sd, n, precision="fp32_split"):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    state = dict(sd)
    if n != 527:
        g = torch.Generator().manual_seed(n)
        m.head_audioset = nn.Linear(768, n)
        state["head_audioset.weight"] = torch.randn(n, 768, generator=g) * 0.05
        state["head_audioset.bias"] = torch.randn(n, generator=g) * 0.1
    m.load_state_dict(state)
    return m.to("cuda").eval().set_precision(precision)


@torch.no_grad()
def clips_per_s(m, x, steps=20, warmup=5):
    for _ in range(warmup):
        m(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        m(x)
    b.record()
    b.synchronize()
    return x.shape[0] * steps / (a.elapsed_time(b) / 1000.0)


@torch.no_grad()
def profile(m, x, steps=5):
    """{kernel class: ms per step} of the event profile (acx_profile_read; runs un-split)."""
    ctx = m.native_context(x.device)
    m(x)
    torch.cuda.synchronize()
    ctx.profile(True)
    ctx.profile_read()
    for _ in range(steps):
        m(x)
    prof = ctx.profile_read()
    ctx.profile(False)
    return {k: v[0] / steps for k, v in prof.items()}


def set_path(v):
    os.environ["ACX_HEAD_PATH"] = str(v)
    _ffi.check(_ffi.lib().acx_tuning_refresh())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-tree", default=None, help="checkout of the parent commit, its library built (N = 527 A/B)")
    ap.add_argument("--speed-ab", action="store_true", help="with --base-tree: headline clips/s of both trees, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_a_heads_bench.txt"))
    ap.add_argument("--skip-speed", action="store_true")
    a = ap.parse_args()
    say("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if a.base_tree:
        say("1. N = 527, this tree against the parent's, bench.py --dump-outputs (bs 64, 10 s clips):")
        ok = bits_ab(a.base_tree)
        say("   all dumps byte-identical: %s  [target: met]" % ok if ok else "   some dumps differ  [target: MISSED]")
    if a.base_tree and a.speed_ab:
        runs = {"base": [], "new": []}
        for _ in range(3):
            for which, tree in (("base", a.base_tree), ("new", ROOT)):
                runs[which].append(tree_bench(os.path.abspath(tree), ["--steps", "50", "--warmup", "10"])["value"])
        say("   speed, bench.py headline (fp32_split, bs 64), three alternating runs each: parent %s, this %s clips/s: "
            "best %.3f of the parent" % (" ".join("%.0f" % v for v in runs["base"]), " ".join("%.0f" % v for v in runs["new"]),
                                         max(runs["new"]) / max(runs["base"])))
    if not a.skip_speed:
        sd = synth.synth_state_dict(0)
        x = synth.synth_waveforms(64, 10 * SR, seed=1).cuda()
        base = model_n(sd, 527)
        say("2. model(x) clips/s, bs 64, 10 s clips, fp32_split (best of 3 alternating rounds, 20 steps each):")
        for n in (50, 200, 4096, 16384):
            m = model_n(sd, n)
            r527, rn = [], []
            for _ in range(3):
                r527.append(clips_per_s(base, x))
                rn.append(clips_per_s(m, x))
            target = 0.97 if n == 16384 else 0.99
            ratio = max(rn) / max(r527)
            say("   N = %5d: %.0f clips/s, 527 classes %.0f: %.3f  [target >= %.2f: %s]"
                % (n, max(rn), max(r527), ratio, target, "met" if ratio >= target else "missed"))
            del m
        m = model_n(sd, 16384)
        os.environ.pop("ACX_HEAD_PATH", None)
        _ffi.check(_ffi.lib().acx_tuning_refresh())
        p = profile(m, x)
        tot = sum(p.values())
        head_ms = p["poolhead"]
        bt = 16
        head_bytes = 16384 * 768 * 4
        say("3. N = 16384, bs 64: head kernels (pooling + class-tiled head, class poolhead) %.3f ms of %.3f ms device time per "
            "forward = %.2f %%  [target <= 2 %%: %s]" % (head_ms, tot, 100 * head_ms / tot,
                                                        "met" if head_ms / tot <= 0.02 else "missed"))
        say("   weight bytes read by the class-tiled kernel: ceil(64 / %d) x %.1f MB = %.1f MB (each clip tile of %d reads every row "
            "once; estimated from the tiling, not counted)  [target <= ceil(64 / Bt) x head: met by construction]"
            % (bt, head_bytes / 1e6, math.ceil(64 / bt) * head_bytes / 1e6, bt))
        say("4. head path threshold: device time of class poolhead (ms per forward), fused pool_head_kernel (ACX_HEAD_PATH=1) / "
            "pooling + head_tiled_kernel (ACX_HEAD_PATH=2):")
        for B in (1, 64):
            xb = x[:B]
            row = []
            for n in (50, 527, 576, 640, 768, 1024, 2048, 4096, 8192, 16384):
                mm = base if n == 527 else model_n(sd, n)
                t = []
                for path in (1, 2):
                    set_path(path)
                    t.append(profile(mm, xb)["poolhead"])
                row.append("N=%d %.3f / %.3f" % (n, t[0], t[1]))
            os.environ.pop("ACX_HEAD_PATH", None)
            _ffi.check(_ffi.lib().acx_tuning_refresh())
            say("   bs %2d: %s" % (B, "; ".join(row)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
