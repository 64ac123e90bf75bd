#!/usr/bin/env python
"""Generate tests/golden/g6_segments.npz: segment-wise and frame-wise outputs made WITH THE REFERENCE'S OWN PARTS.

Runs only where the reference checkout exists (see make_goldens.py, whose reference import and torchlibrosa stand-ins this
script reuses).  Nothing of the reference is copied.  The script
  - imports the reference `convnext_tiny` and the reference's own `interpolate` / `pad_framewise_output`
    (pytorch/pytorch_utils.py:140-176),
  - installs the seeded weights of `audioset_convnext_inf_amd.synth`,
  - runs the reference class's `forward_frame_embeddings` on the demo clip already stored in g1_demo.npz (`pcm16`; the wav is
    not stored again),
  - applies the decision-level recipe of pytorch/models.py:5757-5771 -- mean over frequency, max_pool1d(pool, 1, pool // 2) +
    avg_pool1d(pool, 1, pool // 2) over time, then the class's own `norm` and `head_audioset` modules per segment, sigmoid,
    clipwise = max over segments, interpolate(.., 32) + pad_framewise_output -- for pool 1, 3 and 5,
  - stores segment embeddings, logits, probabilities, the clip maximum and the framewise output of FRAME_CLASSES.

MANIFEST.json and every other fixture stay untouched.

usage: python tests/golden/make_segment_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_goldens as mg                              # noqa: E402
from audioset_convnext_inf_amd import synth           # noqa: E402

POOLS = (1, 3, 5)
FRAME_CLASSES = np.arange(0, 527, 33)[:16]             # 16 classes spread over the head


def main():
    mg._install_shims()
    sys.path.insert(0, os.path.join(mg.REF, "src"))
    from audioset_convnext_inf.pytorch.convnext import convnext_tiny                       # the reference itself
    from audioset_convnext_inf.pytorch.pytorch_utils import interpolate, pad_framewise_output

    torch.manual_seed(0)
    torch.set_num_threads(8)
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56],
                          use_speed_perturb=False)
    model.load_state_dict(synth.synth_state_dict(0), strict=True)
    model.eval()

    g1 = np.load(os.path.join(HERE, "g1_demo.npz"))
    wav = torch.from_numpy(g1["pcm16"].astype(np.float32) / 32768.0)[None, :]
    frames_num = wav.shape[1] // 320 + 1
    out = {"pools": np.array(POOLS), "frame_classes": FRAME_CLASSES}
    with torch.no_grad():
        x = model.forward_frame_embeddings(wav)                    # (1, 768, S, 7)
        assert np.array_equal(x.numpy(), g1["frame"])
        z = torch.mean(x, dim=3)                                   # (1, 768, S)
        for pool in POOLS:
            p = F.max_pool1d(z, kernel_size=pool, stride=1, padding=pool // 2) + \
                F.avg_pool1d(z, kernel_size=pool, stride=1, padding=pool // 2)
            emb = model.norm(p.transpose(1, 2))                    # (1, S, 768)
            logits = model.head_audioset(emb)
            probs = torch.sigmoid(logits)
            clip = torch.max(probs, dim=1)[0]
            frame = pad_framewise_output(interpolate(probs, 32), frames_num)
            assert frame.shape[1] == frames_num
            out["emb_p%d" % pool] = emb[0].numpy()
            out["logits_p%d" % pool] = logits[0].numpy()
            out["probs_p%d" % pool] = probs[0].numpy()
            out["clip_p%d" % pool] = clip[0].numpy()
            out["frame_p%d" % pool] = frame[0][:, torch.from_numpy(FRAME_CLASSES)].numpy()
    path = os.path.join(HERE, "g6_segments.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
