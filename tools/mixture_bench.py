#!/usr/bin/env python
"""Gaussian mixtures on the GPU (pytorch/mixture.py, csrc/mixture.hip): the measurements behind profiles/mixture_bench.txt.

    python tools/mixture_bench.py [--out profiles/mixture_bench.txt] [--n 100000] [--components 64] [--dim 768] [--sklearn 1]

(a) ms per EM iteration of acx_gmm_fit (E-step, M-step, decide; tol = 0 so every queued iteration runs) on resident rows: the
    difference of a 12-iteration and a 2-iteration fit divided by 10, which leaves out the centring and the closing E-step; medians
    of five windows between device events, after a warm-up.
(b) acx_gmm_estep alone (resp written), acx_gmm_score alone and acx_gmm_mstep alone, and the E-step's share of the 157.3 TFLOP/s
    f32-matrix peak by its algorithmic flop: two sweeps of 2 n K (2 dim) multiply-adds.
(c) the same fit (same initial parameters, 10 iterations, tol = 0) in sklearn.mixture.GaussianMixture on the host (recorded).
No figure is a requirement: nothing comparable exists in the parent commit."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                    # noqa: E402
import torch                          # noqa: E402

from audioset_convnext_inf_amd import _ffi                                   # noqa: E402
from audioset_convnext_inf_amd._ffi import vp                                # noqa: E402

F32_MATRIX_PEAK = 157.3e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def median_ms(fn, reps=3, windows=5):
    fn()
    torch.cuda.synchronize()
    return statistics.median(window(fn, reps) for _ in range(windows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_bench.txt"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--components", type=int, default=64)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--sklearn", type=int, default=1)
    args = ap.parse_args()
    n, K, dim = args.n, args.components, args.dim
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cuda").manual_seed(n + K)
    mu = torch.randn(K, dim, generator=g, device="cuda") * 0.3
    lab = torch.randint(0, K, (n,), generator=g, device="cuda")
    x = (mu[lab] + torch.randn(n, dim, generator=g, device="cuda")).contiguous()
    w0 = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
    m0 = x[torch.randperm(n, generator=g, device="cuda")[:K]].to(torch.float64).contiguous()
    v0 = x.to(torch.float64).var(dim=0, unbiased=False)[None, :].repeat(K, 1).contiguous()
    stream = _ffi.stream_ptr(dev)
    nbytes = _ffi.gmm_workspace_bytes(n, dim, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tol = torch.zeros(1, dtype=torch.float64, device=dev)
    center = torch.empty(dim, dtype=torch.float64, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    lpn = torch.empty(n, dtype=torch.float32, device=dev)
    resp = torch.empty((n, K), dtype=torch.float32, device=dev)
    state = torch.zeros(4, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    nk = torch.empty(K, dtype=torch.float64, device=dev)
    w, m, v = w0.clone(), m0.clone(), v0.clone()

    def fit(iters):
        w.copy_(w0); m.copy_(m0); v.copy_(v0)
        _ffi.gmm_fit(vp(x), x.stride(0), n, dim, vp(w), vp(m), vp(v), K, _ffi.GMM_DIAG, iters, vp(tol), 1e-6, vp(center), vp(labels),
                     vp(lpn), vp(state), vp(status), (vp(ws), nbytes), stream)

    say("Gaussian mixture, diag, n %d, K %d, dim %d on %s; workspace %.0f MiB" % (n, K, dim, torch.cuda.get_device_name(dev),
                                                                                 nbytes / 2 ** 20))
    t2, t12 = median_ms(lambda: fit(2)), median_ms(lambda: fit(12))
    words = state.view(torch.int32).cpu()
    say("(a) fit of 2 iterations %.2f ms, of 12 iterations %.2f ms: %.2f ms per EM iteration (iterations run: %d, status %d)"
        % (t2, t12, (t12 - t2) / 10, int(words[0]), int(status.cpu()[0])))

    def estep(r):
        _ffi.gmm_estep(vp(x), x.stride(0), n, dim, vp(center), vp(w), vp(m), vp(v), K, _ffi.GMM_DIAG, vp(lpn), vp(r), K, vp(labels),
                       vp(total), vp(status), (vp(ws), nbytes), stream)

    def mstep():
        _ffi.gmm_mstep(vp(x), x.stride(0), n, dim, vp(center), vp(resp), K, K, 1e-6, _ffi.GMM_DIAG, vp(w), vp(m), vp(v), vp(nk),
                       vp(status), (vp(ws), nbytes), stream)

    te, ts = median_ms(lambda: estep(resp)), median_ms(lambda: estep(None))
    tm = median_ms(mstep)
    flop = 2 * 2.0 * n * K * (2 * dim)
    say("(b) acx_gmm_estep %.2f ms (with the centring pass; %.1f %% of the f32-matrix peak by 2 sweeps x 2 n K 2 dim flop), "
        "acx_gmm_score %.2f ms, acx_gmm_mstep %.2f ms" % (te, 100 * flop / (te * 1e-3) / F32_MATRIX_PEAK, ts, tm))
    per_iter = (t12 - t2) / 10
    say("    inside a fit the rows are centred once: the E-step's share of an iteration is at most %.1f %% of the f32-matrix peak "
        "by the same flop over the whole iteration" % (100 * flop / (per_iter * 1e-3) / F32_MATRIX_PEAK))
    if args.sklearn:
        from sklearn.mixture import GaussianMixture
        import warnings
        xh = x.cpu().numpy().astype(np.float64)
        sk = GaussianMixture(K, covariance_type="diag", weights_init=w0.cpu().numpy(), means_init=m0.cpu().numpy(),
                             precisions_init=1.0 / v0.cpu().numpy(), reg_covar=1e-6, tol=0.0, max_iter=10)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk.fit(xh)
        th = time.perf_counter() - t0
        t10 = median_ms(lambda: fit(10), reps=1, windows=3)
        say("(c) 10 iterations from the same parameters: scikit-learn %s on the host %.1f s (%d threads), acx_gmm_fit %.1f ms (%.0fx); "
            "lower bound %.6f against %.6f" % (__import__("sklearn").__version__, th, os.cpu_count() if "OMP_NUM_THREADS" not in os.environ
                                              else int(os.environ["OMP_NUM_THREADS"]), t10, th * 1e3 / t10, sk.lower_bound_,
                                              float(state[2].cpu())))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
