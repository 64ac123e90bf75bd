#!/usr/bin/env python
"""Variable-length batches (acx_forward_varlen): extract(pack=True) against the length-bucketed extract() on the scenarios of
tools/extract_bench.py, and a resident 64-clip ragged batch (1 .. 30 s) through forward_varlen against a uniform 64 x 10 s
model(x) -- audio-seconds per second, same process, same precision (scene embeddings).

    python tools/varlen_bench.py [precision] > profiles/rNN_varlen.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audioset_convnext_inf_amd import synth                                          # noqa: E402
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny                 # noqa: E402
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract             # noqa: E402

precision = sys.argv[1] if len(sys.argv) > 1 else "fp32_split"
m = convnext_tiny(after_stem_dim=[252, 56])
m.load_state_dict(synth.synth_state_dict(0))
m = m.cuda().eval().set_precision(precision)
print("precision %s" % precision)


def timed(fn, reps=1):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


rs = np.random.RandomState(0)
for name, lengths in (("300 clips, every length different (1 .. 30 s)", rs.randint(32000, 960000, size=300)),
                      ("300 clips of 40 distinct lengths (1 .. 30 s)", rs.choice(rs.randint(32000, 960000, size=40), size=300)),
                      ("300 clips of 10 s", np.full(300, 320000))):
    wavs = [synth.synth_waveforms(1, int(n), seed=int(n) % 1000)[0] for n in lengths]
    audio = float(np.sum(lengths)) / 32000
    extract(m, wavs[:8], what="scene")
    extract(m, wavs[:8], what="scene", pack=True)                                   # warm-up
    dt_b = timed(lambda: extract(m, wavs, what="scene"))
    dt_p = timed(lambda: extract(m, wavs, what="scene", pack=True))
    print("%-48s bucketed %7.1f clips/s %8.0f audio-s/s | packed %7.1f clips/s %8.0f audio-s/s | x%.2f"
          % (name, len(wavs) / dt_b, audio / dt_b, len(wavs) / dt_p, audio / dt_p, dt_b / dt_p))

# resident batches: the forward alone
ragged = [int(n) for n in rs.randint(32000, 960001, size=64)]
packed = torch.cat([synth.synth_waveforms(1, n, seed=i)[0] for i, n in enumerate(ragged)]).cuda()
uniform = synth.synth_waveforms(64, 320000, seed=1).cuda()
dt_r = timed(lambda: m.forward_varlen(packed, ragged, what="scene"), reps=20)
dt_u = timed(lambda: m.forward_scene_embeddings(uniform), reps=20)
a_r, a_u = sum(ragged) / 32000 / dt_r, 64 * 10 / dt_u
print("resident ragged 64 clips (1 .. 30 s, %.0f s of audio) forward_varlen: %.2f ms  %8.0f audio-s/s" % (sum(ragged) / 32000, dt_r * 1e3, a_r))
print("resident uniform 64 x 10 s model(x):                             %.2f ms  %8.0f audio-s/s" % (dt_u * 1e3, a_u))
print("ragged / uniform audio-s/s: %.3f" % (a_r / a_u))
