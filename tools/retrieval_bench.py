#!/usr/bin/env python
"""Nearest-neighbour search over embeddings (acx_knn_search, pytorch/retrieval.EmbeddingIndex) against the best stock-torch form
on the same device, in the same process, on the same inputs: torch.topk(Q @ D.T, k) in fp32 (D normalised outside the timed
region for cosine; queries chunked at the largest chunk whose score matrix fits in 4 GiB), eager and as a torch.cuda.graph
replay, the better of the two.  Cosine, dim 768, k 10 unless said otherwise:
  1. self-search of the evaluation set, nq = n = 20 371;
  2. a batch of queries against a large corpus, nq = 64, n = 1 000 000;
  3. one query, nq = 1, n = 100 000: p50 / p99 wall latency to host-visible indices;
  4. shape 2 with k = 128.
Per shape: device time (HIP events around the call; warm-up, then the median of the medians of repeated timed windows), the
ratio to the baseline [target >= 1.0x], and the peak device memory above the inputs (torch.cuda.max_memory_allocated around one
call) [target on shapes 1 and 2: lower than the baseline's].  Also, without targets: the search's share of the 157.3 TFLOP/s
f32-matrix peak on shape 1 (2 nq n dim flop) and of 8 TB/s on shape 2 (both from the whole call's time, an upper bound on the
search kernel's; `rocprofv3 --kernel-trace --stats -- python tools/retrieval_bench.py --shapes 1` splits it into
knn_search_kernel and knn_merge_kernel), model.search against forward_scene_embeddings alone at bs 64 over the index of shape 2,
and the wall time of the kNN probe (classify, 527 classes) on shape 1.

    python tools/retrieval_bench.py [--shapes 1,2,3,4] [--skip-model] > profiles/r16_a_retrieval_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audioset_convnext_inf_amd import _ffi                                        # noqa: E402
from audioset_convnext_inf_amd.pytorch.retrieval import EmbeddingIndex            # noqa: E402

DIM = 768
SCORE_BYTES = 4 << 30


def device_ms(fn, windows=5, reps=5):
    """Median over `windows` timed windows of the median device time of `reps` calls each."""
    fn()
    fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(windows):
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        meds.append(float(np.median(times)))
    return float(np.median(meds))


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def baseline_fn(q, dn, k, cosine):
    """torch.topk(Q @ D.T, k), D already normalised for cosine; the queries are normalised inside (they are the call's input)."""
    chunk = max(1, min(q.shape[0], SCORE_BYTES // (4 * dn.shape[0])))

    def run():
        s_out, i_out = [], []
        for a in range(0, q.shape[0], chunk):
            qq = q[a:a + chunk]
            if cosine:
                qq = torch.nn.functional.normalize(qq, dim=1)
            s, i = torch.topk(qq @ dn.T, k)
            s_out.append(s)
            i_out.append(i)
        return (s_out[0], i_out[0]) if len(s_out) == 1 else (torch.cat(s_out), torch.cat(i_out))
    return run


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def data(nq, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.randn((n, DIM), generator=g, device="cuda")
    q = d[:nq] if nq == n else torch.randn((nq, DIM), generator=g, device="cuda")
    return q, d


def shape_row(name, nq, n, k, self_search=False, windows=5, reps=5):
    q, d = data(nq, n, seed=n % 1000)
    idx = EmbeddingIndex(d, metric="cosine")
    ours = (lambda: idx.search(None, k)) if self_search else (lambda: idx.search(q, k))
    dn = torch.nn.functional.normalize(d, dim=1)
    base = baseline_fn(q, dn, k, True)
    t_ours = device_ms(ours, windows, reps)
    t_eager = device_ms(base, windows, reps)
    try:
        g, keep = graphed(base)
        t_graph = device_ms(g.replay, windows, reps)
        del g, keep
    except Exception as e:      # noqa: BLE001
        t_graph = float("nan")
        print("   (baseline graph capture failed: %s)" % str(e).splitlines()[0])
    t_base = np.nanmin([t_eager, t_graph])
    m_ours, m_base = peak_above_inputs(ours), peak_above_inputs(base)
    idx.check()
    s_o, i_o = ours()
    s_b, i_b = base()
    agree = float((i_o[:, 0] == i_b[:, 0]).float().mean()) if not self_search else float("nan")
    print("%s nq %d, n %d, k %d, %d slice(s): search %.3f ms; baseline eager %.3f ms, graph %.3f ms; %.2fx  [target >= 1.0x]; "
          "peak memory above the inputs %.1f MB against %.1f MB%s; top-1 agreement %.4f"
          % (name, nq, n, k, _ffi.knn_slices(nq, n, k), t_ours, t_eager, t_graph, t_base / t_ours, m_ours / 1e6, m_base / 1e6,
             "  [target: lower]" if name[0] in "12" else "", agree))
    return t_ours, idx, q


def latency(nq, n, k, calls=300):
    q, d = data(nq, n, seed=7)
    idx = EmbeddingIndex(d, metric="cosine")
    dn = torch.nn.functional.normalize(d, dim=1)
    base = baseline_fn(q, dn, k, True)
    res = {}
    for name, fn in (("search", lambda: idx.search(q, k)[1].cpu()), ("baseline", lambda: base()[1].cpu())):
        for _ in range(20):
            fn()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        res[name] = (np.percentile(ts, 50) * 1e3, np.percentile(ts, 99) * 1e3)
    print("3. nq %d, n %d, k %d, %d slices, wall to host-visible indices over %d calls: search p50 %.3f ms, p99 %.3f ms; baseline "
          "(eager) p50 %.3f ms, p99 %.3f ms; %.2fx at p50  [target >= 1.0x]"
          % (nq, n, k, _ffi.knn_slices(nq, n, k), calls, *res["search"], *res["baseline"], res["baseline"][0] / res["search"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,2,3,4")
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    shapes = set(a.shapes.split(","))
    print("device %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if "1" in shapes:
        n = 20371
        t, idx, _ = shape_row("1.", n, n, 10, self_search=True, windows=3, reps=3)
        print("   share of the 157.3 TFLOP/s f32-matrix peak (whole call): %.1f %%" % (2.0 * n * n * DIM / (t * 1e-3) / 157.3e12 * 100))
        tgt = (torch.rand((n, 527), device="cuda") < 0.02)
        probe = EmbeddingIndex(idx.embeddings, metric="cosine", target=tgt)
        probe.classify(idx.embeddings[:64], 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probs = probe.classify(idx.embeddings, 10)
        torch.cuda.synchronize()
        print("   kNN probe (classify, 527 classes, k 10) of the %d rows against themselves: %.1f ms wall" % (n, (time.perf_counter() - t0) * 1e3))
        del idx, probe, probs, tgt
        torch.cuda.empty_cache()
    if "2" in shapes or "4" in shapes:
        idx = None
        if "2" in shapes:
            t, idx, q = shape_row("2.", 64, 1000000, 10)
            print("   share of 8 TB/s (whole call, one pass over the index): %.1f %%" % (1000000 * DIM * 4 / (t * 1e-3) / 8e12 * 100))
            if not a.skip_model:
                from audioset_convnext_inf_amd import synth
                from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
                m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
                m.load_state_dict(synth.synth_state_dict(0))
                m = m.to("cuda").eval()
                wav = synth.synth_waveforms(64, 320000, seed=3).cuda()
                t_f = device_ms(lambda: m.forward_scene_embeddings(wav), 3, 3)
                t_s = device_ms(lambda: m.search(idx, wav, k=10), 3, 3)
                print("   model.search, bs 64 x 10 s over this index: %.3f ms against forward_scene_embeddings alone %.3f ms" % (t_s, t_f))
                del m, wav
            del idx, q
            torch.cuda.empty_cache()
        if "4" in shapes:
            shape_row("4.", 64, 1000000, 128)
            torch.cuda.empty_cache()
    if "3" in shapes:
        latency(1, 100000, 10)


if __name__ == "__main__":
    main()
