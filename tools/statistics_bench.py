#!/usr/bin/env python
"""Embedding statistics on the GPU (pytorch/statistics.py, csrc/moments.hip, csrc/eigh.hip) against stock torch on the same
device and numpy on the host: the measurements behind profiles/r29_a_statistics_bench.txt.

    python tools/statistics_bench.py [--out profiles/r29_a_statistics_bench.txt] [--rows 20371,200000,1000000] [--dims 192,384,768]

(a) acx_moments on resident fp32 rows of dim 768 against torch.cov(x.double().T) on the same device (eager; it has no
    capturable single call) and against numpy.cov from host arrays, the copy of the result included.  Every size warmed up,
    the contenders alternate, medians of five windows between device events.  Achieved float64 TFLOP/s counts the n dim^2 flop
    of the upper triangle the kernel computes AND the 2 n dim^2 of the full product, both stated; no share of a peak is claimed
    (no bare f64-MFMA loop is measured here).  Peak device memory above the input, both sides.  [>= 1.0x torch at every size]
(b) acx_eigh at dim 192 / 384 / 768 on a covariance of 4 dim rows: device time, sweeps, against numpy.linalg.eigh from a host
    array, copies included.  Recorded, no bar.
(c) frechet_distance of two (20 371, 768) sets, the whole call to the synchronised value, against the host route
    (frechet_distance_host: numpy moments + LAPACK) from host arrays.  Recorded, no bar.
bench.py against the parent is run beside this tool and kept in the same profile; this tool rewrites only its own --out file."""
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
from audioset_convnext_inf_amd.pytorch import statistics as st               # noqa: E402

DIM = 768
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps):
    """ms per call of fn over `reps` calls between device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def medians(contenders, reps, repeats=5):
    """{name: median ms} with the contenders alternating inside each repeat."""
    got = {k: [] for k in contenders}
    for _ in range(repeats):
        for k, fn in contenders.items():
            got[k].append(window(fn, reps))
    return {k: statistics.median(v) for k, v in got.items()}


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def rows_on_device(n, seed):
    """Correlated rows with an offset mean, generated in chunks on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mix = torch.randn(DIM, DIM, generator=g, device="cuda") / DIM ** 0.5
    x = torch.empty((n, DIM), dtype=torch.float32, device="cuda")
    for a in range(0, n, 65536):
        b = min(n, a + 65536)
        x[a:b] = torch.randn(b - a, DIM, generator=g, device="cuda") @ mix + 3.0
    return x


class OurMoments:
    def __init__(self, x):
        self.x = x
        n, dim = x.shape
        self.mean = torch.empty(dim, dtype=torch.float64, device=x.device)
        self.cov = torch.empty((dim, dim), dtype=torch.float64, device=x.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=x.device)
        self.ws_bytes = _ffi.moments_workspace_bytes(n, dim)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=x.device)
        self.stream = _ffi.stream_ptr(x.device)

    def __call__(self):
        x = self.x
        _ffi.moments(vp(x), x.stride(0), x.shape[0], x.shape[1], 1, vp(self.mean), vp(self.cov), x.shape[1], vp(self.status),
                     (vp(self.ws), self.ws_bytes), self.stream)


def bench_moments(n, host_rows_limit):
    say()
    say("== (a) moments: n %d, dim %d" % (n, DIM))
    x = rows_on_device(n, n)
    ours = OurMoments(x)
    stock = lambda: torch.cov(x.double().T)
    ours()
    ref = stock()
    torch.cuda.synchronize()
    err = float((ours.cov - ref).abs().max() / ref.abs().max())
    t0 = window(ours, 2)
    reps = int(min(200, max(2, 300.0 / max(t0, 0.05))))
    med = medians({"ours": ours, "torch.cov(x.double().T)": stock}, reps)
    say("    median of 5 windows of %d calls:" % reps)
    for k, v in med.items():
        say("      %-26s %9.3f ms" % (k, v))
    say("    ours against torch: %.2fx  [>= 1.0x]   max |cov - torch| / max |cov| = %.1e" % (med["torch.cov(x.double().T)"] / med["ours"], err))
    sec = med["ours"] * 1e-3
    say("    achieved float64 rate: %.2f TFLOP/s of the full product (2 n dim^2), %.2f TFLOP/s of the tiles computed (upper triangle, "
        "78 of 144)" % (2.0 * n * DIM * DIM / sec / 1e12, 2.0 * n * 78 * 64 * 64 / sec / 1e12))
    say("    peak device memory above the input: ours %.1f MiB (workspace included), torch %.1f MiB"
        % (peak_above(lambda: st.moments(x)), peak_above(stock)))
    if n <= host_rows_limit:
        xh = x.cpu().numpy()
        t = time.perf_counter()
        np.cov(xh.astype(np.float64), rowvar=False)
        tn = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        st.moments(torch.from_numpy(xh), device="cuda").cov.cpu()
        to = (time.perf_counter() - t) * 1e3
        say("    from host arrays, copies included: numpy.cov %.1f ms, ours %.1f ms: %.1fx" % (tn, to, tn / to))
    else:
        say("    from host arrays: not measured at this size (numpy.cov of %d rows takes the host tens of seconds)" % n)
    del x, ours, ref
    torch.cuda.empty_cache()


def bench_eigh(dim):
    x = rows_on_device(4 * dim, dim)[:, :dim].contiguous()
    cov = st.moments(x).cov
    values, vectors, state = st.eigh(cov)
    torch.cuda.synchronize()
    sweeps = int(state.sweeps)
    ref = np.linalg.eigvalsh(cov.cpu().numpy())[::-1]
    err = float(np.abs(values.cpu().numpy() - ref).max() / np.abs(ref).max())
    td = statistics.median([window(lambda: st.eigh(cov), 1) for _ in range(3)])
    hosts = []
    for _ in range(3):
        t = time.perf_counter()
        c = cov.cpu().numpy()
        w, v = np.linalg.eigh(c)
        torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        hosts.append((time.perf_counter() - t) * 1e3)
    say("    dim %4d: ours %9.2f ms (%d sweeps of %d rounds ran, 40 queued)   numpy.linalg.eigh with copies %8.2f ms   ours / host %.2f   "
        "max |w - w_LAPACK| / max |w| = %.1e" % (dim, td, sweeps, dim - 1 + (dim & 1), statistics.median(hosts), td / statistics.median(hosts), err))


def bench_frechet(n):
    say()
    say("== (c) frechet_distance of two (%d, %d) sets" % (n, DIM))
    x, y = rows_on_device(n, 1), rows_on_device(n, 2) * 1.1
    float(st.frechet_distance(x, y))
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        v = float(st.frechet_distance(x, y))
        ts.append((time.perf_counter() - t) * 1e3)
    xh, yh = x.cpu().numpy(), y.cpu().numpy()
    t = time.perf_counter()
    h = st.frechet_distance_host(xh, yh)
    th = (time.perf_counter() - t) * 1e3
    say("    ours %.1f ms (resident rows, host clock to the synchronised value), host route from host arrays %.1f ms: %.2fx; "
        "values %.9g / %.9g" % (statistics.median(ts), th, th / statistics.median(ts), v, h.value))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_a_statistics_bench.txt"))
    ap.add_argument("--rows", default="20371,200000,1000000")
    ap.add_argument("--dims", default="192,384,768")
    ap.add_argument("--host-rows-limit", type=int, default=200000)
    ap.add_argument("--frechet-rows", type=int, default=20371)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("statistics_bench needs a GPU: nothing is measured without one")
    say("statistics_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for n in [int(v) for v in a.rows.split(",") if v]:
        bench_moments(n, a.host_rows_limit)
    say()
    say("== (b) eigh of a covariance of 4 dim rows (device time between events; the host side from and to device tensors)")
    for dim in [int(v) for v in a.dims.split(",") if v]:
        bench_eigh(dim)
    if a.frechet_rows:
        bench_frechet(a.frechet_rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
