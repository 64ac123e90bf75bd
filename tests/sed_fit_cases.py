"""What the CPU and GPU tests of the weak-label SED fit (test_sed_fit_cpu.py, test_gpu_sed_fit.py) share: the planted-event case,
random segment embeddings with clip labels, and the localisation score.  A plain helper module, not a conftest."""
import numpy as np
import torch
import torch.nn.functional as F

POOLINGS = ("max", "mean", "linear", "exp")

# The planted-event case: bags of 31 segments; a positive clip of class k carries AMP * d_k (d_k a unit direction) on 3 consecutive
# segments.  In the clip's mean row the event is 3 / 31 of that beside noise of 1 / sqrt(31) per direction; a fit that pools the
# segment probabilities learns from the event at full size once its pooling has found the segment.  Sizes chosen on the host
# definition (float64, fit seed 3): the clip-level fit on mean rows localises 45 % of the held-out clips, "max" 90 %, "linear" 88 %
# (chance: 3 / 31 = 10 %).
PLANT = dict(train=1024, test=128, S=31, span=3, N=4, amp=3.0, seed=11, epochs=20, batch=64, lr=3e-3, fit_seed=3,
             train_seed=100, test_seed=200)


def planted(n, seed, S=PLANT["S"], span=PLANT["span"], N=PLANT["N"], amp=PLANT["amp"], proto_seed=PLANT["seed"]):
    """-> (segments (n, S, 768) float32, target (n, N) float32, start (n,) int64: the first planted segment, klass (n,) int64).
    Every clip is positive for exactly one class."""
    gp = torch.Generator().manual_seed(proto_seed)
    proto = F.normalize(torch.randn(N, 768, generator=gp), dim=1)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S, 768, generator=g)
    klass = torch.randint(0, N, (n,), generator=g)
    start = torch.randint(0, S - span + 1, (n,), generator=g)
    for i in range(n):
        x[i, start[i]:start[i] + span] += amp * proto[klass[i]]
    y = torch.zeros(n, N)
    y[torch.arange(n), klass] = 1.0
    return x, y, start, klass


def localisation(weight, bias, segments, start, klass, span=PLANT["span"]):
    """The share of clips whose arg-max segment (of the clip's own class) falls inside the planted span."""
    z = segments.double() @ weight.double().cpu().T + bias.double().cpu()
    top = z[torch.arange(z.shape[0]), :, klass].argmax(dim=1)
    return float(((top >= start) & (top < start + span)).double().mean())


def random_bags(lengths, N, seed, n_total=None, scale=0.05, soft=False):
    """Segment embeddings for bags of the given lengths, laid back to back in a pool of n_total rows and read through a shuffled
    seg_idx; a head whose logits stay within |z| < 10; targets for 1.5 x as many clips as bags, bag_idx with a repeat.
    -> dict of CPU tensors: E, W, b, Y (float32, hard unless soft), seg_idx, bag_off, bag_idx."""
    g = torch.Generator().manual_seed(seed)
    rows = int(sum(lengths))
    n_total = max(rows + 5, 8) if n_total is None else n_total
    E = F.layer_norm(torch.randn(n_total, 768, generator=g), (768,))
    W, b = torch.randn(N, 768, generator=g) * scale, torch.randn(N, generator=g) * 0.3
    bags = len(lengths)
    n_bags = bags + bags // 2 + 1
    Y = torch.rand(n_bags, N, generator=g) if soft else (torch.rand(n_bags, N, generator=g) < 0.4).float()
    seg_idx = torch.randint(0, n_total, (max(rows, 1),), generator=g)[:rows]
    bag_idx = torch.randint(0, n_bags, (bags,), generator=g)
    if bags > 1:
        bag_idx[-1] = bag_idx[0]                                                   # a repeated bag in one batch
    bag_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
    return dict(E=E, W=W, b=b, Y=Y, seg_idx=seg_idx, bag_off=bag_off, bag_idx=bag_idx)
