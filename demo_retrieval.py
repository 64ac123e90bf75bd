#!/usr/bin/env python
"""Query by example and the kNN probe on this backbone's scene embeddings: build an index over a set of clips, print each
query's nearest neighbours, and score kNN tagging with the device metrics (pytorch/retrieval.py, ConvNeXt.build_index /
ConvNeXt.search).

    python demo_retrieval.py --ckpt checkpoints/model.safetensors --data sounds/ --query dog.wav      # sounds/<class>/*.wav
    python demo_retrieval.py --synthetic                       # seeded weights and clips, no files needed
    python demo_retrieval.py --synthetic --clusters 8          # also k-means over the corpus: sizes, the clip nearest each centre
    python demo_retrieval.py --synthetic --select-clusters 4,8,16     # choose k by the mean silhouette (--cluster-criterion ...)
    python demo_retrieval.py --synthetic --duplicates 0.95     # groups of near-duplicate clips (radius search + components)
    python demo_retrieval.py --synthetic --dbscan 0.6,5        # density clustering: no k, an explicit noise set (EPS,MIN_SAMPLES)
    python demo_retrieval.py --synthetic --pca 16 [--whiten]   # also search a PCA-reduced copy of the index, against the full one
    python demo_retrieval.py --synthetic --int8 [--oversample 4] [--no-rerank]     # int8 index: coarse search, exact fp32 rerank

16-bit PCM WAV files at any rate (resampled on the device)."""
import argparse
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from audioset_convnext_inf_amd.pytorch.convnext import ConvNeXt, convnext_tiny      # noqa: E402
from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics               # noqa: E402
from audioset_convnext_inf_amd.utils.utilities import read_wav_pcm16                # noqa: E402


def synthetic_items(clips, classes, seconds, seed=0):
    """Seeded clips in classes that differ in spectrum: band-limited noise around a class frequency plus its tone, on the
    seeded noise of synth.synth_waveforms -> (waveforms, (clips, classes) bool targets, names)"""
    from audioset_convnext_inf_amd import synth
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, classes, (clips,), generator=g)
    L = int(seconds * 32000)
    noise = synth.synth_waveforms(clips, L, seed=seed)
    t = torch.arange(L) / 32000.0
    waves = []
    for i, c in enumerate(label):
        f0 = 180.0 * (1.35 ** int(c))
        tone = torch.sin(2 * torch.pi * f0 * t) + 0.5 * torch.sin(2 * torch.pi * 2 * f0 * t + float(i))
        waves.append(0.3 * noise[i] + 0.3 * tone)
    target = torch.zeros(clips, classes, dtype=torch.bool)
    target[torch.arange(clips), label] = True
    return waves, target, ["band_%d" % c for c in range(classes)]


def folder_items(root):
    items = []
    for cls in sorted(os.listdir(root)):
        d = os.path.join(root, cls)
        if os.path.isdir(d):
            items += [(os.path.join(d, f), cls) for f in sorted(os.listdir(d)) if f.lower().endswith(".wav")]
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default="topel/ConvNeXt-Tiny-AT", help="local .safetensors/.pth, Zenodo URL or HF model id")
    ap.add_argument("--data", help="folder with one sub-folder of .wav files per class: the corpus")
    ap.add_argument("--query", nargs="*", default=[], help=".wav files to look up (default: the first clips of the corpus)")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights and clips (300 x 1 s, 8 classes)")
    ap.add_argument("--clips", type=int, default=300)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("-k", type=int, default=5)
    ap.add_argument("--metric", default="cosine", choices=("cosine", "dot"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--int8", action="store_true", help="an int8 index: coarse search on int8 codes, then the exact fp32 rerank")
    ap.add_argument("--oversample", type=int, default=4, help="--int8: coarse candidates per neighbour asked for")
    ap.add_argument("--no-rerank", action="store_true", help="--int8: keep codes only and return the coarse scores")
    ap.add_argument("--clusters", type=int, default=0, help="also cluster the corpus into this many clusters (k-means on the GPU)")
    ap.add_argument("--select-clusters", default="", help="choose the number of clusters among these, e.g. 10,20,50: one k-means fit "
                    "per k, each scored on the GPU")
    ap.add_argument("--cluster-criterion", default="silhouette", choices=("silhouette", "calinski_harabasz", "davies_bouldin"))
    ap.add_argument("--duplicates", type=float, default=None, metavar="THRESHOLD",
                    help="also list the groups of clips whose score (--metric) with each other is at least THRESHOLD")
    ap.add_argument("--dbscan", default="", metavar="EPS,MIN_SAMPLES",
                    help="also cluster the corpus by density: neighbours are the clips with a score (--metric) of at least EPS")
    ap.add_argument("--pca", type=int, default=0, help="also reduce the index to this many principal components (PCA on the GPU)")
    ap.add_argument("--whiten", action="store_true", help="--pca: whiten the reduced rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this build runs on an MI355X; no GPU is visible")

    rate = None
    if a.synthetic:
        from audioset_convnext_inf_amd import synth
        model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
        model.load_state_dict(synth.synth_state_dict(0))
        waves, target, names = synthetic_items(a.clips, a.classes, 1.0, a.seed)
        paths = ["clip_%03d" % i for i in range(len(waves))]
    else:
        if not a.data:
            sys.exit("give --data or --synthetic")
        model = ConvNeXt.from_pretrained(a.ckpt, map_location="cpu")
        if model is None:
            sys.exit(1)
        items = folder_items(a.data)
        if not items:
            sys.exit("no .wav files found")
        names = sorted({c for _, c in items})
        waves, paths, target = [], [], torch.zeros(len(items), len(names), dtype=torch.bool)
        for i, (path, cls) in enumerate(items):
            wav, sr = read_wav_pcm16(path)
            if rate is None:
                rate = sr
            elif sr != rate:
                sys.exit("%s is at %d Hz, the clips before it at %d Hz: one rate per run" % (path, sr, rate))
            waves.append(torch.from_numpy(wav[0]))
            paths.append(path)
            target[i, names.index(cls)] = True
    model = model.to("cuda").eval()
    print("%d clips, %d classes" % (len(waves), len(names)))

    t0 = time.perf_counter()
    index = model.build_index(waves, target=target, sample_rate=rate, metric=a.metric, quantize="int8" if a.int8 else None,
                              rerank=not a.no_rerank, oversample=a.oversample)
    torch.cuda.synchronize()
    print("%sindex of %d x %d built in %.2f s" % ("int8 " + ("" if index.rerank else "codes-only ") if a.int8 else "", len(index),
                                                  index.dim, time.perf_counter() - t0))
    label = target.float().argmax(1)
    k = min(a.k, len(index) - 1)

    if a.query:
        for path in a.query:
            wav, sr = read_wav_pcm16(path)
            hit = model.search(index, torch.from_numpy(wav[0])[None].cuda(), k=k, sample_rate=sr)
            print("%s:" % path)
            for s, j in zip(hit["scores"][0].tolist(), hit["indices"][0].tolist()):
                print("    %.4f  %s  (%s)" % (s, paths[j], names[int(label[j])]))
    else:
        scores, indices = index.search(None, k)             # every clip against the others
        for r in range(min(8, len(index))):
            print("%s (%s): %s" % (paths[r], names[int(label[r])],
                                   ", ".join("%s %.3f (%s)" % (paths[j], s, names[int(label[j])])
                                             for s, j in zip(scores[r].tolist(), indices[r].tolist()))))

    if a.clusters and a.int8 and a.no_rerank:
        print("--clusters needs the fp32 rows: skipped with --no-rerank")
    elif a.clusters:
        # no labels needed: k-means over the stored rows with the index's metric, and the stored clip nearest to each centre
        km = index.cluster(a.clusters, seed=a.seed)
        _, nearest = index.search(km.centers, 1)
        sil = (getattr(index, "exact", None) or index).cluster_scores(km).silhouette
        km.check()
        index.check()
        print("k-means, %d clusters, %d iterations, inertia %.4g, mean silhouette %.4f; sizes %s" % (
            a.clusters, int(km.n_iter), float(km.inertia), float(sil), km.counts.tolist()))
        for c, j in enumerate(nearest[:, 0].tolist()):
            print("    cluster %d (%d clips): nearest %s (%s)" % (c, int(km.counts[c]), paths[j], names[int(label[j])]))

    if a.select_clusters and a.int8 and a.no_rerank:
        print("--select-clusters needs the fp32 rows: skipped with --no-rerank")
    elif a.select_clusters:
        # which k: one fit per candidate, scored where the rows are; the silhouette decides unless told otherwise
        from audioset_convnext_inf_amd.pytorch.cluster_scores import select_clusters
        rows = getattr(index, "exact", None) or index
        sel = select_clusters(rows.embeddings, [int(k) for k in a.select_clusters.split(",")], criterion=a.cluster_criterion,
                              metric="cosine" if a.metric == "cosine" else "euclidean", seed=a.seed)
        print("%s per k: %s -> k = %d" % (a.cluster_criterion, ", ".join("%d: %.4f" % kv for kv in zip(sel.ks, sel.scores.tolist())),
                                          sel.best_k))

    if (a.duplicates is not None or a.dbscan) and a.int8 and a.no_rerank:
        print("--duplicates / --dbscan need the fp32 rows: skipped with --no-rerank")
    elif a.duplicates is not None or a.dbscan:
        rows = index if getattr(index, "exact", None) is None else index.exact
        if a.duplicates is not None:
            # which clips are (nearly) the same recording: a radius self-join, then the components of its graph
            dup = rows.duplicates(a.duplicates).check()
            groups = dup.groups()
            print("near-duplicates at %s >= %g: %d groups, %d of %d clips to keep" % (a.metric, a.duplicates, len(groups),
                                                                                   int(dup.keep.sum()), len(rows)))
            for g in groups[:8]:
                print("    " + ", ".join("%s (%s)" % (paths[j], names[int(label[j])]) for j in g))
        if a.dbscan:
            eps, min_samples = a.dbscan.split(",")
            db = rows.dbscan(float(eps), int(min_samples)).check()
            sizes = torch.bincount(db.labels[~db.noise], minlength=int(db.clusters)).tolist()
            print("DBSCAN at %s >= %s, min_samples %s: %d clusters, %d noise clips, %d core clips; sizes %s"
                  % (a.metric, eps, min_samples, int(db.clusters), int(db.noise.sum()), int(db.core.sum()), sizes))

    if a.pca and a.int8:
        print("--pca reduces the fp32 index: skipped with --int8")
    elif a.pca:
        # covariance, eigenvectors and projection on the device; the reduced index keeps the metric and the targets
        pca, small = index.pca(min(a.pca, index.dim, len(index)), whiten=a.whiten)
        pca.check()
        _, full_nn = index.search(None, 1)
        _, small_nn = small.search(None, 1)
        same = float((full_nn[:, 0] == small_nn[:, 0]).float().mean())
        print("PCA %d -> %d%s: %.1f %% of the variance kept; the nearest neighbour is the full index's for %.1f %% of the clips"
              % (index.dim, small.dim, " (whitened)" if a.whiten else "", 100 * float(pca.explained_variance_ratio_.sum()), 100 * same))

    # the kNN probe: each clip labelled by its neighbours (itself left out), scored like any tagger
    from audioset_convnext_inf_amd.pytorch.retrieval import vote
    scores, indices = index.search(None, k)
    probs = vote(indices, scores, index.target, "similarity", 0.07)
    index.check()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stats = tagging_metrics(index.target, probs)
    top1 = float((probs.argmax(1).cpu() == label).float().mean())
    print("kNN probe (k = %d, leave-one-out): mAP %.3f, top-1 %.3f" % (k, float(stats["average_precision"].mean()), top1))


if __name__ == "__main__":
    main()
