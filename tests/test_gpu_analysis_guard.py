"""GPU (`-m gpu`): every analysis call in poisoned, exactly sized, fenced buffers (tests/analysis_guard.py).

Each case makes one public wrapper call three times: as it is, and with every torch.empty of the wrapper -- workspace, outputs,
status words -- replaced by the payload of a layer_ref.Guarded buffer prefilled with 0xFF and with 0x7F.  Every canary must be
intact and the three documented results must have the same bits.  The values themselves are held to the host definitions by each
module's own GPU test; this file asks what those cannot see: a write past the promised end, an output element nobody wrote,
scratch read before it was written or relied on to be zero.

The shapes sit next to the constants at which a carve or a launch changes form; the case id names the constant.

The second test gives every *_workspace_bytes function of _ffi an answer 256 bytes short: the call must raise AcxError naming the
workspace before anything is launched (everything allocated after the size query is still poison) with every canary intact.

Two more: the harness must fail two toy wrappers on the device, and the calls whose workspace serves a second launch sequence
(n_init = 2, a chunked bootstrap) must equal the same work done in workspaces of its own -- leftovers of a first sequence are the
same in all three runs, so no poison shows them."""
import functools

import numpy as np
import pytest
import torch

import analysis_guard as ag
import sed_cases
import statistics_cases as stc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import (calibration, classify, cluster_scores, clustering, finetune, metrics, mixture,
                                               neighbors, ranking, retrieval, sed_metrics, segments, statistics)

pytestmark = pytest.mark.gpu

SKIP = {"_host", "_cols", "_padded", "device"}          # host caches of a result object, and its torch.device


def flat(obj):
    """A result as the flat tuple run_guarded compares: tensors, arrays and numbers as they are; tuples, lists, dicts (by key) and
    the result objects of the package (by attribute; host caches and callables left out) taken apart."""
    out = []

    def walk(v):
        if isinstance(v, (torch.Tensor, np.ndarray, float, int, bool, str, type(None), np.floating, np.integer, np.bool_)):
            out.append(v)
        elif isinstance(v, dict):
            for k in sorted(v, key=str):
                walk(v[k])
        elif isinstance(v, (tuple, list)):
            for e in v:
                walk(e)
        elif type(v).__module__.startswith("audioset_convnext_inf_amd"):
            for k in sorted(vars(v)):
                if k not in SKIP and not callable(vars(v)[k]):
                    walk(vars(v)[k])
        elif isinstance(v, torch.device):
            out.append(str(v))
        else:
            raise TypeError("flat() met a %s" % type(v).__name__)

    walk(obj)
    return tuple(out)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- seeded inputs (numpy; nothing here touches the GPU) -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scores_targets(n, C, seed=0):
    """(scores fp32 (n, C), targets uint8 (n, C)): about 30 % positives that score higher on average, every class with both."""
    rng = np.random.default_rng(1000 * seed + 7 * n + C)
    y = (rng.random((n, C)) < 0.3).astype(np.uint8)
    y[0], y[1 % n] = 1, 0
    s = (rng.random((n, C)) * 0.8 + 0.2 * y).astype(np.float32)
    return s, y


@functools.lru_cache(maxsize=None)
def logits_labels(n, N, seed=0):
    """(logits fp32 (n, N), labels int64 (n,)): every class present, the label's logit raised so that accuracy is neither 0 nor 1."""
    rng = np.random.default_rng(2000 * seed + 11 * n + N)
    lab = (np.arange(n) % N).astype(np.int64)
    rng.shuffle(lab)
    z = rng.standard_normal((n, N)).astype(np.float32)
    z[np.arange(n), lab] += 1.5
    return z, lab


@functools.lru_cache(maxsize=None)
def blobs(n, dim, k, seed=0, spread=0.15):
    """(rows fp32 (n, dim), labels int64 (n,)): k Gaussian blobs around random centres, the rows dealt round-robin."""
    rng = np.random.default_rng(3000 * seed + 13 * n + 17 * dim + k)
    c = rng.standard_normal((k, dim))
    lab = (np.arange(n) % k).astype(np.int64)
    return (c[lab] + spread * rng.standard_normal((n, dim))).astype(np.float32), lab


@functools.lru_cache(maxsize=None)
def embeddings(n, seed=0):
    return np.random.default_rng(4000 + seed).standard_normal((n, finetune.EMBED_DIM)).astype(np.float32)


# ---- metrics and scores ---------------------------------------------------------------------------------------------------------------

def metrics_cases():
    out = []
    for n, C, why in ((65, 2, "small"), (130, 65, "kMetTile+1"), (32768, 3, "kMetLdsKeys"), (32769, 3, "kMetLdsKeys+1")):
        s, y = scores_targets(n, C)
        out.append(("tagging_metrics-%dx%d-%s" % (n, C, why), lambda s=s, y=y: metrics.tagging_metrics(y, s)))
        for name, crit in (("f1", "f1"), ("precision", ("precision", 0.6)), ("recall", ("recall", 0.7))):
            out.append(("operating_points-%s-%dx%d-%s" % (name, n, C, why),
                        lambda s=s, y=y, crit=crit: metrics.operating_points(y, s, criterion=crit)))
    s, y = scores_targets(257, 65)
    thr = np.linspace(0.2, 0.8, 65).astype(np.float32)
    out.append(("threshold_metrics-257x65-rows256-classes64", lambda: metrics.threshold_metrics(y, s, thr)))
    return out


def bootstrap_cases():
    out = []
    for n, C in ((1025, 3), (32768, 1)):
        s, y = scores_targets(n, C, seed=1)
        s2 = scores_targets(n, C, seed=2)[0]
        tag = "%dx%d" % (n, C)
        out.append(("weighted_metrics-" + tag, lambda s=s, y=y, n=n: metrics.weighted_metrics(y, s, metrics.bootstrap_weights(3, n, seed=4))))
        out.append(("bootstrap_metrics-chunk2-" + tag,
                    lambda s=s, y=y: metrics.bootstrap_metrics(y, s, replicates=5, chunk=2, seed=3, per_class=True)))
        out.append(("bootstrap_difference-chunk2-" + tag,
                    lambda s=s, s2=s2, y=y: metrics.bootstrap_difference(y, s, s2, replicates=5, chunk=2, seed=3)))
    return out


def ranking_cases():
    out = []
    for rows, C, slice_rows, why in ((5, 527, None, "wave"), (3, 1025, None, "workgroup-form-above-1024"), (257, 16, 256, "two-slices")):
        s, y = scores_targets(rows, C, seed=5)
        tag = "%dx%d-%s" % (rows, C, why)
        out.append(("ranking_metrics-" + tag, lambda s=s, y=y, sr=slice_rows: ranking.ranking_metrics(y, s, k=3, slice_rows=sr)))
        out.append(("bootstrap_ranking-" + tag, lambda s=s, y=y: ranking.bootstrap_ranking(y, s, replicates=3, seed=2, k=3)))
    return out


def calibration_cases():
    out = []
    for n, C, why in ((300, 3, "small"), (70, 65, "kCalTile+1"), (32769, 2, "kCalLdsRows+1")):
        s, y = scores_targets(n, C, seed=6)
        z = (6.0 * s - 3.0).astype(np.float32)
        out.append(("fit_platt-%dx%d-%s" % (n, C, why), lambda z=z, y=y: calibration.fit_platt(cu(y), cu(z))))
    z, lab = logits_labels(300, 10, seed=1)
    out.append(("fit_temperature-300x10", lambda: calibration.fit_temperature(cu(lab), cu(3.0 * z))))
    s, y = scores_targets(300, 3, seed=6)
    out.append(("reliability-300x3", lambda: calibration.reliability(cu(y), cu(s))))

    def toplabel(n, N):
        z, lab = logits_labels(n, N, seed=1)
        cal = calibration.fit_temperature(cu(lab), cu(3.0 * z))
        return cal, calibration.reliability_toplabel(cu(lab), cu(3.0 * z), calibration=cal)

    out.append(("reliability_toplabel-fitted-300x10", lambda: toplabel(300, 10)))
    # acx_temperature_fit sums groups of ceil(n / 4096) rows: two rows a group from 4097 rows on
    out.append(("fit_temperature-reliability_toplabel-4097x10-rows-per-group2", lambda: toplabel(4097, 10)))
    # a workgroup instead of a wave per row, and another dynamic LDS size, above kSoftWaveMaxN = 2048 classes
    out.append(("fit_temperature-reliability_toplabel-70x2049-kSoftWaveMaxN+1", lambda: toplabel(70, 2049)))
    return out


def classify_cases():
    out = []
    for N, why in ((64, "one-wave"), (65, "one-wave+1"), (2049, "softmax_depth-2048+1")):
        z, lab = logits_labels(7, N, seed=2)
        k = min(5, N)
        out.append(("softmax_topk-7x%d-%s" % (N, why), lambda z=z, k=k: classify.softmax_topk(cu(z), k=k)))
        out.append(("classification_metrics-7x%d-%s" % (N, why), lambda z=z, lab=lab, k=k: classify.classification_metrics(cu(lab), cu(z), k=k)))
    return out


# ---- clustering and mixtures --------------------------------------------------------------------------------------------------------------

def clustering_cases():
    def fit_and_predict(n, dim, K, **kw):
        x = blobs(n, dim, min(K, 16))[0]
        km = clustering.kmeans(cu(x), K, **kw)
        return km, km.predict(cu(x[: n // 2 + 1]))

    return [("kmeans-1025x8x3-euclidean-kKmBlockRows+1", lambda: fit_and_predict(1025, 8, 3, metric="euclidean", init="k-means++", seed=1)),
            ("kmeans-200x12x5-cosine-n_init2", lambda: fit_and_predict(200, 12, 5, metric="cosine", n_init=2, seed=2)),
            ("kmeans-300x4x257-kKmStepCentres+1", lambda: fit_and_predict(300, 4, 257, seed=3, max_iter=10))]


def mixture_cases():
    def fit(n, dim, K, cov, max_iter=20):
        x = cu(blobs(n, dim, min(K, 16), seed=1, spread=0.4)[0])
        gm = mixture.gmm(x, K, covariance_type=cov, seed=1, max_iter=max_iter)
        return gm, gm.predict_proba(x), gm.score_samples(x), gm.score(x)

    def select():
        x = cu(blobs(65, 4, 2, seed=1, spread=0.4)[0])
        sel = mixture.select_components(x, (1, 2), max_iter=20)
        return sel.ks, sel.scores, sel.best_k, sel.fits, sel.criterion

    return [("gmm-65x4x2-diag-kGmChunkRows+1", lambda: fit(65, 4, 2, "diag")),
            ("gmm-300x8x3-spherical", lambda: fit(300, 8, 3, "spherical")),
            ("gmm-257x4x9-kGmWaveComps+1-kGmMeanChunkRows+1", lambda: fit(257, 4, 9, "diag")),
            ("gmm-300x4x257-kGmStepComps+1", lambda: fit(300, 4, 257, "diag", 3)),
            ("gmm-4097x4x2-kGmMaxChunks*kGmChunkRows+1", lambda: fit(4097, 4, 2, "diag", 3)),
            ("gmm-65537x4x2-kGmMeanChunks*kGmMeanChunkRows+1", lambda: fit(65537, 4, 2, "spherical", 2)),
            ("select_components-65x4-ks1,2", select)]


def cluster_score_cases():
    x, lab = blobs(257, 8, 3, seed=2, spread=0.5)
    other = (lab + (np.arange(257) % 7 == 0)) % 3
    return [("silhouette-257x8x3-euclidean", lambda: cluster_scores.silhouette(cu(x), cu(lab), metric="euclidean", clusters=3)),
            ("silhouette-257x8x3-cosine", lambda: cluster_scores.silhouette(cu(x), cu(lab), metric="cosine", clusters=3)),
            ("silhouette-257x8x3-sample100", lambda: cluster_scores.silhouette(cu(x), cu(lab), clusters=3, sample=100, seed=1)),
            ("dispersion_scores-257x8x3", lambda: cluster_scores.dispersion_scores(cu(x), cu(lab), clusters=3)),
            ("agreement-257", lambda: cluster_scores.agreement(cu(lab), cu(other), 3, 3))]


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------------

def statistics_cases():
    out = [("moments-1025x65-two-kMomMinSliceRows-slices-three-kStTile-pairs", lambda: statistics.moments(cu(stc.gaussian_rows(1025, 65, 1)))),
           ("moments-16389x5-kMomMaxSlices*kMomMinSliceRows+5", lambda: statistics.moments(cu(stc.gaussian_rows(16389, 5, 7)))),
           ("gram-70x70-rows33", lambda: statistics.gram(cu(stc.gaussian_rows(33, 70, 2).astype(np.float64)),
                                                         cu(stc.gaussian_rows(33, 70, 3).astype(np.float64))))]
    for d in (1, 33, 64):
        out.append(("eigh-d%d-32x32-tiles" % d, lambda d=d: statistics.eigh(cu(stc._cov(200, d, 20 + d)))))

    def pca():
        x = cu(stc.gaussian_rows(200, 50, 4))
        p = statistics.PCA.fit(x, components=2)
        return p, p.transform(x)

    out.append(("PCA-fit-transform-dim50-k2", pca))
    out.append(("frechet_distance-dim33", lambda: statistics.frechet_distance(cu(stc.gaussian_rows(120, 33, 5)),
                                                                               cu(stc.gaussian_rows(90, 33, 6, offset=0.25)))))
    return out


# ---- retrieval and neighbours -------------------------------------------------------------------------------------------------------------

def retrieval_cases():
    def queries(x, nq):
        return cu(x[np.arange(nq) % x.shape[0]] + 0.01 * (1 + np.arange(nq)[:, None] // x.shape[0]).astype(np.float32))

    def exact(exclude, n=257, nq=3, k=5):
        x = blobs(n, 8, 5, seed=3, spread=0.5)[0]
        index = retrieval.EmbeddingIndex(cu(x))
        scores, idx = index.search(queries(x, nq), k=k, exclude=np.arange(nq) if exclude else None)
        return scores, idx, index._status

    def exact_capped_cells():
        # knn_ws_bytes takes min(nq * ceil(n / kKnnStepRows), 64 * kKnnTargetWgs + nq) cells: 2100 * 17 against 32768 + 2100
        nq, n, k = 2100, 4097, 5
        assert nq * -(-n // 256) > 64 * 512 + nq and _ffi.knn_workspace_bytes(nq, n, k) == -(-(64 * 512 + nq) * k * 8 // 256) * 256
        return exact(False, n, nq, k)

    def i8(n, dim, nq=3, k=5):
        x = blobs(n, dim, 7, seed=4, spread=0.5)[0]
        index = retrieval.QuantizedIndex(cu(x))
        scores, idx = index.search(queries(x, nq), k=k)
        return scores, idx, index._status, index.codes, index.scales

    def i8_two_level():
        # the smallest database the plan cuts into kKnnTwoLevelSlices = 16 slices of kKnnStepRows = 256 rows: 15 * 256 + 1 rows;
        # with rerank the coarse search asks for kc = k * oversample = 20 candidates
        nq, n, kc = 3, 3841, retrieval.candidate_count(5, 4, 3841)
        assert kc == 20 and _ffi.knn_slices(nq, n - 1, kc) == 15 and _ffi.knn_slices(nq, n, kc) == 16
        # acx_knn_search_i8 merges in two levels only where the lists of the slices and of the ceil(16 / ceil(sqrt 16)) = 4 groups
        # fit the workspace it is given, and otherwise falls back to one level with the same bits: the size QuantizedIndex.search
        # allocates (restated here) must hold both, or this case runs the one-level form and shows nothing
        lists, mids = nq * 16 * kc * 8, nq * 4 * kc * 8
        given = _ffi.knn_workspace_bytes(nq, n, kc) + nq * (int(16 ** 0.5) + 2) * kc * 8
        assert lists + mids <= given and lists + mids > _ffi.knn_workspace_bytes(nq, n, kc)
        return i8(n, 32)

    return [("EmbeddingIndex.search-3x257x8-k5-kKnnStepRows+1", lambda: exact(False)),
            ("EmbeddingIndex.search-3x257x8-k5-exclude", lambda: exact(True)),
            ("EmbeddingIndex.search-3x257x8-k33-knn_plan-r2", lambda: exact(False, k=33)),
            ("EmbeddingIndex.search-3x257x8-k65-knn_plan-r4", lambda: exact(True, k=65)),
            ("EmbeddingIndex.search-33x257x8-k5-knn_plan-qt2", lambda: exact(False, nq=33)),
            ("EmbeddingIndex.search-2100x4097x8-k5-knn_ws_bytes-capped-cells", exact_capped_cells),
            ("QuantizedIndex.search-3x300x40-k5", lambda: i8(300, 40)),
            ("QuantizedIndex.search-3x300x40-k9-kc36-knn_plan-r2", lambda: i8(300, 40, k=9)),
            ("QuantizedIndex.search-3x300x40-k17-kc68-knn_plan-r4-knn_rescore_kernel2", lambda: i8(300, 40, k=17)),
            ("QuantizedIndex.search-33x300x40-k5-knn_plan-qt2", lambda: i8(300, 40, nq=33)),
            ("QuantizedIndex.search-3x3841x32-kKnnTwoLevelSlices", i8_two_level)]


def neighbor_cases():
    x = blobs(300, 8, 6, seed=5, spread=0.2)[0]

    def lists():
        assert _ffi.radius_slices(300, 300, 0) * 300 > 1024      # the self-join's cells fill two blocks of the scan (kScanBlock)
        nb = neighbors.radius_neighbors(None, cu(x), 0.9, metric="cosine")
        cross = neighbors.radius_neighbors(cu(x[:40] + 0.01), cu(x), 1.0, metric="euclidean", slices=3)
        assert nb.total > 0 and cross.total > 0
        return nb, cross

    def groups():
        dup = neighbors.duplicate_groups(cu(x), threshold=0.97)
        return dup, dup.pairs

    x2 = blobs(1025, 8, 6, seed=6, spread=0.2)[0]
    return [("radius_neighbors-300-kRadRowsPerGroup+44-kScanBlock+", lists),
            ("dbscan-1025-kScanBlock+1", lambda: neighbors.dbscan(cu(x2), eps=1.0, min_samples=5)),
            ("radius_count-300", lambda: neighbors.radius_count(None, cu(x), 0.9, metric="cosine", include_self=True)),
            ("duplicate_groups-300", groups),
            ("dbscan-300", lambda: neighbors.dbscan(cu(x), eps=1.0, min_samples=5))]


# ---- head fitting and sound event detection ---------------------------------------------------------------------------------------------

def wide_fit_cases():
    """The fits pick 16- or 32-wide tiles, and with them the number of partial sums the update reads from the workspace, from the
    part's compute units (head_fit.hip): fit_classes_wide(N) = ceil(N / 32) * 24 >= CUs for the updates and the cross-entropy
    logits, fit_rows_wide(rows, N) = ceil(rows / 32) * ceil(N / 32) >= CUs for the bce logits.  The class counts are read off the
    device in the case: the first N that is classes-wide (321 on 256 CUs), and 2049 = kSoftWaveMaxN + 1 classes (a workgroup per
    row in the cross-entropy row kernels), where batches of 128 rows are rows-wide too and the last batch of 2 rows is not."""
    def cus():
        return torch.cuda.get_device_properties(0).multi_processor_count

    def first_wide():
        N = 32 * (-(-cus() // 24) - 1) + 1
        assert -(-N // 32) * 24 >= cus() > -(-(N - 1) // 32) * 24
        return N

    def one(loss, N, n, batch):
        if N is None:
            N = first_wide()
        else:
            tiles = -(-N // 32)                      # classes-wide; the full batches rows-wide, the short last batch not
            assert tiles * 24 >= cus() and -(-batch // 32) * tiles >= cus() > tiles
        emb = cu(embeddings(n))
        if loss == "ce":
            return finetune.fit_head(emb, cu(logits_labels(n, N, seed=3)[1]), epochs=2, batch_size=batch, lr=1e-3, loss="ce", classes=N)
        return finetune.fit_head(emb, cu(scores_targets(n, N, seed=7)[1]), epochs=2, batch_size=batch, lr=1e-3)

    def group(loss, N, n, batch):
        N = first_wide() if N is None else N
        emb = cu(embeddings(n))
        jobs = [dict(lr=1e-3, seed=1), dict(lr=1e-2, seed=2, rows=torch.arange(0, n, 2))]
        if loss == "ce":
            return finetune.fit_heads(emb, cu(logits_labels(n, N, seed=3)[1]), jobs, epochs=2, batch_size=batch, loss="ce", classes=N)
        return finetune.fit_heads(emb, cu(scores_targets(n, N, seed=7)[1]), jobs, epochs=2, batch_size=batch)

    def sed():
        lens = [1 + i % 5 for i in range(10)]
        return finetune.fit_sed_head((cu(embeddings(sum(lens), seed=1)), lens), cu(scores_targets(10, first_wide(), seed=8)[1]),
                                     epochs=2, batch_size=4, lr=1e-3)

    out = []
    for loss in ("bce", "ce"):
        out.append(("fit_head-%s-70-first-fit_classes_wide" % loss, lambda loss=loss: one(loss, None, 70, 32)))
        out.append(("fit_heads-%s-70-first-fit_classes_wide" % loss, lambda loss=loss: group(loss, None, 70, 32)))
        out.append(("fit_head-%s-130x2049-kSoftWaveMaxN+1-fit_rows_wide-batch128" % loss, lambda loss=loss: one(loss, 2049, 130, 128)))
        out.append(("fit_heads-%s-130x2049-kSoftWaveMaxN+1-fit_rows_wide-batch128" % loss, lambda loss=loss: group(loss, 2049, 130, 128)))
    out.append(("fit_sed_head-max-first-fit_classes_wide", sed))
    return out


def finetune_cases():
    emb = embeddings(70)
    out = []
    for N, why in ((3, "small"), (65, "kFitDbCols+1")):
        y = scores_targets(70, N, seed=7)[1]
        lab = logits_labels(70, N, seed=3)[1]
        out.append(("fit_head-bce-70x%d-%s-short-last-batch" % (N, why),
                    lambda y=y: finetune.fit_head(cu(emb), cu(y), epochs=2, batch_size=32, lr=1e-3)))
        out.append(("fit_head-ce-70x%d-%s-short-last-batch" % (N, why),
                    lambda lab=lab, N=N: finetune.fit_head(cu(emb), cu(lab), epochs=2, batch_size=32, lr=1e-3, loss="ce", classes=N)))
    y, lab = scores_targets(70, 3, seed=7)[1], logits_labels(70, 3, seed=3)[1]
    jobs = [dict(lr=1e-3, seed=1), dict(lr=1e-2, seed=2, rows=torch.arange(0, 70, 2))]
    out.append(("fit_heads-bce-two-jobs", lambda: finetune.fit_heads(cu(emb), cu(y), jobs, epochs=2, batch_size=32)))
    out.append(("fit_heads-ce-two-jobs", lambda: finetune.fit_heads(cu(emb), cu(lab), jobs, epochs=2, batch_size=32, loss="ce", classes=3)))
    out += wide_fit_cases()
    lens = [1 + i % 5 for i in range(10)]
    seg, ybag = embeddings(sum(lens), seed=1), scores_targets(10, 3, seed=8)[1]
    for pooling in finetune.MIL_POOLS:
        out.append(("fit_sed_head-%s-bags1..5" % pooling,
                    lambda pooling=pooling: finetune.fit_sed_head((cu(seg), lens), cu(ybag), pooling=pooling, epochs=2, batch_size=4, lr=1e-3)))
    out.append(("cross_validate_head-folds2-grid2",
                lambda: finetune.cross_validate_head(cu(emb), cu(y), folds=2, grid={"lr": [1e-3, 1e-2]}, epochs=2, batch_size=32)))
    return out


def event_table(ev):
    """The valid rows of an EventTable, its count and its status (the capacity tail is not a result)."""
    n = len(ev)
    return ev.table[:n], n, ev.count, ev.status


def event_cases():
    p = sed_cases.probabilities(2, 40, 65)
    return [("decode_events-2x40x65-median%d-%s" % (m, why), lambda m=m: event_table(segments.decode_events_gpu(cu(p), low=0.3, median=m)))
            for m, why in ((1, "none"), (3, "registers"), (5, "registers"), (7, "kEvRegMedian-last-register-form"),
                           (9, "kEvRegMedian+2-dynamic-LDS"))]


SED = (3, 31, 4)                                           # three files, 31 steps, four classes


@functools.lru_cache(maxsize=None)
def sed_setup():
    """(probabilities, annotations as lists) of the scoring cases: the annotations are made from one decoding outside the guards."""
    B, S, N = SED
    p = sed_cases.probabilities(B, S, N)
    table = segments.decode_events_gpu(cu(p), step=sed_cases.STEP, low=0.3)
    ends = [float(e[-1]) for e in table.edges]
    return p, sed_cases.make_reference(table.to_lists(), ends, N, sed_cases.STEP)


def sed_scores(s):
    return (s.kind, s.counts, s.overall, s.ref_match, s.est_match, s.status, s.cross_triggers, s.est_relevant, s.ref_hit)


def sed_cases_list():
    def score(fn, **args):
        p, ref = sed_setup()
        table = segments.decode_events_gpu(cu(p), step=sed_cases.STEP, low=0.3)
        return sed_scores(fn(sed_metrics.ReferenceEvents.from_lists(ref, SED[2], device="cuda"), table, **args))

    def psds(**args):
        p, ref = sed_setup()
        reference = sed_metrics.ReferenceEvents.from_lists(ref, SED[2], device="cuda")
        return sed_metrics.psds(cu(p), reference, thresholds=(0.3, 0.5, 0.7), step=sed_cases.STEP, **args)

    return [("event_based_metrics-3files-4classes", lambda: score(sed_metrics.event_based_metrics, t_collar=sed_cases.STEP)),
            ("segment_based_metrics-3files-4classes", lambda: score(sed_metrics.segment_based_metrics, time_resolution=1.0)),
            ("intersection_based_metrics-3files-4classes", lambda: score(sed_metrics.intersection_based_metrics)),
            ("intersection_based_metrics-cttc-3files-4classes", lambda: score(sed_metrics.intersection_based_metrics, cttc_threshold=0.3)),
            ("psds-3files-4classes", psds),
            ("psds-cross-triggers-3files-4classes", lambda: psds(cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1.0))]


CASES = (metrics_cases() + bootstrap_cases() + ranking_cases() + calibration_cases() + classify_cases() + clustering_cases()
         + mixture_cases() + cluster_score_cases() + statistics_cases() + retrieval_cases() + neighbor_cases() + finetune_cases()
         + event_cases() + sed_cases_list())


@pytest.mark.parametrize("call", [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_guarded_call(monkeypatch, call):
    ag.run_guarded(call, flat, monkeypatch)


# ---- the size functions -------------------------------------------------------------------------------------------------------------------

def _sized_calls():
    s, y = scores_targets(65, 2)
    z, lab = logits_labels(300, 10, seed=1)
    x8, lab8 = blobs(257, 8, 3, seed=2, spread=0.5)
    emb, y3, lab3 = embeddings(70), scores_targets(70, 3, seed=7)[1], logits_labels(70, 3, seed=3)[1]
    lens = [1 + i % 5 for i in range(10)]
    seg, ybag = embeddings(sum(lens), seed=1), scores_targets(10, 3, seed=8)[1]

    def mixture_scores():
        # the fit outside the guards: its k-means initialisation launches kernels of its own before the mixture's first call
        gm = _fitted_mixture()
        return lambda: gm.score_samples(cu(blobs(65, 4, 2, seed=1, spread=0.4)[0]))

    return [
        ("metrics_workspace_bytes", lambda: lambda: metrics.tagging_metrics(y, s)),
        ("weighted_metrics_workspace_bytes", lambda: lambda: metrics.weighted_metrics(y, s, np.ones(65, np.int64))),
        ("ranking_workspace_bytes", lambda: lambda: ranking.ranking_metrics(y, s)),
        ("head_fit_workspace_bytes", lambda: lambda: finetune.fit_head(cu(emb), cu(y3), epochs=1, batch_size=32)),
        ("head_fit_ce_workspace_bytes", lambda: lambda: finetune.fit_head(cu(emb), cu(lab3), epochs=1, batch_size=32, loss="ce", classes=3)),
        ("head_fit_mil_workspace_bytes", lambda: lambda: finetune.fit_sed_head((cu(seg), lens), cu(ybag), epochs=1, batch_size=4)),
        ("head_fit_group_workspace_bytes", lambda: lambda: finetune.fit_heads(cu(emb), cu(y3), [dict(seed=1), dict(seed=2)], epochs=1,
                                                                              batch_size=32)),
        ("platt_workspace_bytes", lambda: lambda: calibration.fit_platt(cu(scores_targets(300, 3, seed=6)[1]),
                                                                         cu(scores_targets(300, 3, seed=6)[0]))),
        ("temperature_workspace_bytes", lambda: lambda: calibration.fit_temperature(cu(lab), cu(z))),
        ("knn_workspace_bytes", lambda: lambda: retrieval.EmbeddingIndex(cu(blobs(1025, 8, 5, seed=3)[0])).search(cu(x8[:3]), k=10)),
        ("kmeans_workspace_bytes", lambda: lambda: clustering.kmeans(cu(x8), 3)),
        ("gmm_workspace_bytes", mixture_scores),
        ("cluster_scores_workspace_bytes", lambda: lambda: cluster_scores.silhouette(cu(x8), cu(lab8), clusters=3)),
        ("radius_workspace_bytes", lambda: lambda: neighbors.radius_count(None, cu(x8), 0.9)),
        ("dbscan_workspace_bytes", lambda: lambda: neighbors.dbscan(cu(x8), eps=1.0)),
        ("moments_workspace_bytes", lambda: lambda: statistics.moments(cu(stc.gaussian_rows(40, 8, 1)))),
        ("eigh_workspace_bytes", lambda: lambda: statistics.eigh(cu(stc._cov(50, 16, 1)))),
        ("events_workspace_bytes", lambda: lambda: segments.decode_events_gpu(cu(sed_cases.probabilities(2, 40, 65)), low=0.3)),
    ]


@functools.lru_cache(maxsize=None)
def _fitted_mixture():
    return mixture.gmm(cu(blobs(65, 4, 2, seed=1, spread=0.4)[0]), 2, max_iter=5)


SIZED = _sized_calls()


def test_every_size_function_is_covered():
    names = sorted(k for k in vars(_ffi) if k.endswith("_workspace_bytes") and callable(getattr(_ffi, k)))
    assert names == sorted(n for n, _ in SIZED)


@pytest.mark.parametrize("name, prepare", SIZED, ids=[n for n, _ in SIZED])
def test_undersized_workspace_is_refused(monkeypatch, name, prepare):
    text = ag.undersized(monkeypatch, _ffi, name, prepare(), _ffi.AcxError)
    assert "workspace" in text


# ---- the harness on the device, and workspaces that serve more than one launch sequence ---------------------------------------------------

def test_harness_sees_poison_on_the_device(monkeypatch):
    """The interceptor engages for CUDA devices however the device is named, hands out 256-byte aligned poisoned payloads, and
    run_guarded fails two toys with the defects it is there to find: scratch summed without a clear, an output element left out."""
    x = torch.arange(1.0, 8.0, dtype=torch.float64, device="cuda")
    with ag.guarded_allocations(monkeypatch, 0x7F) as allocs:
        for device in ("cuda", "cuda:0", torch.device("cuda", 0), x.device, 0):
            t = torch.empty((3, 5), dtype=torch.float32, device=device)
            assert t.is_cuda and t.shape == (3, 5) and t.data_ptr() % 256 == 0
            assert bool((t.view(torch.int32) == 0x7F7F7F7F).all())
        assert len(allocs) == 5 and torch.empty(3).device.type == "cpu" and len(allocs) == 5
        allocs.check()

    def uncleared():
        part = torch.empty(4, dtype=torch.float64, device="cuda")
        part[:3] += x[:3]
        return 2.0 * x, part.sum()

    def unwritten():
        out = torch.empty(7, dtype=torch.float64, device="cuda")
        out[:6] = 2.0 * x[:6]
        return out, x.sum()

    def clean():
        out = torch.empty(7, dtype=torch.float64, device="cuda")
        out.copy_(2.0 * x)
        return out, x.sum()

    ag.run_guarded(clean, flat, monkeypatch)
    for toy, entry in ((uncleared, 1), (unwritten, 0)):
        with pytest.raises(AssertionError, match="result entry %d .*differs between poison 0xFF and 0x7F" % entry):
            ag.run_guarded(toy, flat, monkeypatch)


def _same_bits(a, b):
    a, b = [ag._bits(v) for v in flat(a)], [ag._bits(v) for v in flat(b)]
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, "result entry %d (%s) differs" % (k, ag._describe(x))


def test_reused_workspaces_match_fresh_ones(monkeypatch):
    """A workspace that serves a second launch sequence holds the leftovers of the first in every run alike, which no poison
    shows.  The documents promise the remedy: n_init = 2 is the better of the two single fits (each in a workspace of its own), and
    the bootstrap does not depend on how its replicates are chunked."""
    x = cu(blobs(200, 12, 5)[0])
    with ag.guarded_allocations(monkeypatch, 0xFF) as allocs:
        both = clustering.kmeans(x, 5, metric="cosine", n_init=2, seed=2)
        a, b = (clustering.kmeans(x, 5, metric="cosine", seed=s) for s in (2, 3))
        _same_bits(both, b if float(b.inertia) < float(a.inertia) else a)
        xm = cu(blobs(300, 8, 3, seed=1, spread=0.4)[0])
        both = mixture.gmm(xm, 3, n_init=2, seed=1, max_iter=20)
        a, b = (mixture.gmm(xm, 3, seed=s, max_iter=20) for s in (1, 2))
        _same_bits(both, b if float(b.lower_bound) > float(a.lower_bound) else a)
        s, y = scores_targets(1025, 3, seed=1)
        _same_bits(metrics.bootstrap_metrics(y, s, replicates=5, chunk=2, seed=3, per_class=True),
                   metrics.bootstrap_metrics(y, s, replicates=5, chunk=5, seed=3, per_class=True))
        torch.cuda.synchronize()
        assert len(allocs)
        allocs.check()
