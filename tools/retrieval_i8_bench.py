#!/usr/bin/env python
"""The int8 index (pytorch/retrieval.QuantizedIndex: acx_knn_quantize_i8 / acx_knn_search_i8 / acx_knn_rescore) against the exact
fp32 search (EmbeddingIndex.search, acx_knn_search) on the same device, in the same process, on the same inputs.  Cosine,
dim 768, k 10:
  1. one live query, nq = 1, n = 200 000;
  2. a batch, nq = 1 024, n = 200 000;
  3. the self-search of the evaluation set, nq = n = 20 371;
  4. nq = 4 096, n = 2 000 000 (only with --shapes 4: 6 GB of rows; one warm call, two windows of one call).
Three arms a shape: fp32 / two-stage (oversample 4, reranked: exact fp32 scores) / coarse only (rerank=False).  Device time by
HIP events around the whole Python call, warmed, in ALTERNATING windows (arm A, B, C, A, B, C, ...): per arm the median of the
window medians and their spread (min .. max).  Requirement: two-stage >= 1.0x the fp32 search at every shape; a ratio inside
the fp32 arm's own spread is marked.  Also, without bars: the quantise and rerank shares of a two-stage call (from whole-call
times of the parts), the coarse call's share of the i8 matrix rate (2 nq n dim operations against 5.03 POP/s = 2 048
op/clk/SIMD at 2.4 GHz) and of 8 TB/s (every query tile reads the codes once), recall@10 of both int8 arms against the exact
search on each shape's data, on the planted corpora of the tests and on scene embeddings of synthetic clips.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/retrieval_i8_bench.py --shapes 2 --quick` in a run of its own.

    python tools/retrieval_i8_bench.py --shapes 1,2,3,4 [--skip-model] [--quick] > profiles/r28_a_retrieval_i8_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from audioset_convnext_inf_amd import _ffi                                                        # noqa: E402
from audioset_convnext_inf_amd.pytorch import retrieval                                           # noqa: E402
from audioset_convnext_inf_amd.pytorch.retrieval import EmbeddingIndex, QuantizedIndex           # noqa: E402

DIM, K, OVERSAMPLE = 768, 10, 4
I8_PEAK, HBM_PEAK = 2048 * 4 * 256 * 2.4e9, 8e12
SHAPES = {"1": (1, 200000, False), "2": (1024, 200000, False), "3": (20371, 20371, True), "4": (4096, 2000000, False)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(arms, windows, reps, warm=2):
    """{name: [window medians, ms]}: every arm warmed, then `windows` rounds of `reps` calls of each arm in turn."""
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(windows):
        for name, fn in arms.items():
            out[name].append(float(np.median([timed(fn) for _ in range(reps)])))
    return out


def clustered(nq, n, seed, centres=500, sigma=1.0):
    """Rows and queries around `centres` random centres (the tests' planted generator, on the device)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cen = torch.randn((centres, DIM), generator=g, device="cuda")
    d = cen[torch.randint(0, centres, (n,), generator=g, device="cuda")] + sigma * torch.randn((n, DIM), generator=g, device="cuda")
    q = cen[torch.randint(0, centres, (nq,), generator=g, device="cuda")] + sigma * torch.randn((nq, DIM), generator=g, device="cuda")
    return q, d


def recall(found, exact):
    """Mean share of the exact neighbours among the found ones, row by row."""
    hit = (found[:, :, None] == exact[:, None, :]).any(dim=1).float().sum(dim=1)
    return float((hit / exact.shape[1]).mean())


def fmt(ts):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(ts)), min(ts), max(ts))


def shape_row(name, nq, n, self_search, windows, reps, warm):
    q, d = clustered(nq, n, seed=n % 1000 + nq)
    if self_search:
        q = None
    exact = EmbeddingIndex(d, metric="cosine")
    two = exact.quantize(rerank=True, oversample=OVERSAMPLE)
    coarse = exact.quantize(rerank=False)
    stage = exact.quantize(rerank=False)                       # the coarse stage of the two-stage call: kc candidates
    kc = retrieval.candidate_count(K, OVERSAMPLE, n - (1 if self_search else 0))
    last = {}                                                  # every arm's latest result: the recall below needs no further call
    arms = {"fp32": lambda: last.__setitem__("fp32", exact.search(q, K)), "two-stage": lambda: last.__setitem__("two", two.search(q, K)),
            "coarse": lambda: last.__setitem__("coarse", coarse.search(q, K))}
    t = alternating(arms, windows, reps, warm)
    m = {a: float(np.median(v)) for a, v in t.items()}
    lo, hi = min(t["fp32"]), max(t["fp32"])
    for arm in ("two-stage", "coarse"):
        ratio = m["fp32"] / m[arm]
        inside = lo / m["fp32"] <= 1.0 / ratio <= hi / m["fp32"]
        t[arm + " ratio"] = "%.2fx%s" % (ratio, "  (inside the fp32 arm's own spread)" if inside else "")
    print("%s. nq %d, n %d, k %d, %d slice(s), kc %d: fp32 %s; two-stage %s = %s  [required >= 1.0x]; coarse only %s = %s"
          % (name, nq if not self_search else n, n, K, _ffi.knn_slices(n if self_search else nq, n, K), kc, fmt(t["fp32"]),
             fmt(t["two-stage"]), t["two-stage ratio"], fmt(t["coarse"]), t["coarse ratio"]))
    # the parts of a two-stage call
    parts = {"coarse stage (k = kc)": lambda: stage.search(q, kc)}
    if not self_search:
        parts["norms + quantise of the queries"] = lambda: retrieval.quantize(q, retrieval.row_norms(q))
    tp = {a: float(np.median(v)) for a, v in alternating(parts, max(2, windows // 2), reps, 1).items()}
    t_stage = tp["coarse stage (k = kc)"]
    t_quant = tp.get("norms + quantise of the queries", 0.0)
    print("   of the two-stage call: quantise %.3f ms (%.1f %%), rerank (call - coarse stage at kc) %.3f ms (%.1f %%)"
          % (t_quant, 100 * t_quant / m["two-stage"], m["two-stage"] - t_stage, 100 * (m["two-stage"] - t_stage) / m["two-stage"]))
    rows_q = n if self_search else nq
    pad = two.codes.shape[1]
    ops, qtiles = 2.0 * rows_q * n * pad, -(-rows_q // (32 if rows_q <= 32 else 64))
    share_ops, share_bw = ops / (t_stage * 1e-3) / I8_PEAK, float(qtiles) * n * (pad + 4) / (t_stage * 1e-3) / HBM_PEAK
    share_hbm = n * (pad + 4) / (t_stage * 1e-3) / HBM_PEAK
    print("   coarse stage (whole call, an upper bound on the kernel's time): %.1f %% of the i8 matrix rate, %.1f %% of 8 TB/s with every "
          "query tile reading the codes (%.1f %% for one pass over them): the %s bound is the nearer one"
          % (100 * share_ops, 100 * share_bw, 100 * share_hbm, "arithmetic" if share_ops > share_hbm else "byte"))
    r_two, r_coarse = recall(last["two"][1], last["fp32"][1]), recall(last["coarse"][1], last["fp32"][1])
    two.check()
    coarse.check()
    print("   recall@%d against the exact search: two-stage %.4f, coarse only %.4f" % (K, r_two, r_coarse))
    del exact, two, coarse, stage, q, d
    torch.cuda.empty_cache()


def recall_rows(name, rows, queries):
    exact = EmbeddingIndex(rows, metric="cosine")
    ei = exact.search(queries, K)[1]
    two, coarse = exact.quantize(rerank=True, oversample=OVERSAMPLE), exact.quantize(rerank=False)
    print("   %s: %d rows x %d, %d queries: recall@%d two-stage %.4f, coarse only %.4f"
          % (name, rows.shape[0], rows.shape[1], queries.shape[0], K, recall(two.search(queries, K)[1], ei),
             recall(coarse.search(queries, K)[1], ei)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,2,3")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--quick", action="store_true", help="two windows of two calls (for a profiler run)")
    a = ap.parse_args()
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for s in a.shapes.split(","):
        if not s:
            continue
        nq, n, self_search = SHAPES[s]
        big = s == "4"
        shape_row(s, nq, n, self_search, 2 if (a.quick or big) else 3, 1 if big else 2 if a.quick else 3, 1)
    print("recall without bars:")
    import retrieval_i8_cases as rc
    for case in rc.PLANTED:
        rows, queries = rc.planted(*case)
        recall_rows("planted%s" % (case,), torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda())
    if not a.skip_model:
        from audioset_convnext_inf_amd import synth
        from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
        from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract
        m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
        m.load_state_dict(synth.synth_state_dict(0))
        m = m.to("cuda").eval()
        wav = synth.synth_waveforms(264, 32000, seed=3).cuda()
        emb = torch.stack(extract(m, [w for w in wav], what="scene", pack=True)).cuda()
        recall_rows("scene embeddings of synthetic 1 s clips (synthetic weights)", emb[:200], emb[200:])


if __name__ == "__main__":
    main()
