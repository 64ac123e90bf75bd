"""GPU: ranking metrics per clip (pytorch/ranking.py; acx_ranking_metrics in include/acx.h; csrc/ranking.hip) against the numpy
host definition.  The counts are integers and the float64 sums are the same additions in the same order, so every output is
compared with ==.  Shapes sit at the boundaries of the kernels -- 64-class ballot words, the switch from a wave per row to a
workgroup per row between 1 024 and 1 025 classes, 4 rows per workgroup, slices of 16 rows, the widest head -- not at workload size."""
import numpy as np
import pytest
import torch

import ranking_cases as rc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import ranking

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWITCH = _ffi.RANK_WAVE_MAX_CLASSES                      # 1 024: the last wave-per-row width; 1 025 takes a workgroup per row
WIDTHS = (1, 2, 63, 64, 65, 527, SWITCH, SWITCH + 1)
ROWS = (1, 3, 4, 5, 257)
_HOST = {}


def host(key, y, s, k):
    """ranking_metrics_host of a case, computed once and shared."""
    if key + (k,) not in _HOST:
        _HOST[key + (k,)] = ranking.ranking_metrics_host(y, s, k=k)
    return _HOST[key + (k,)]


def padded(a, pad, dtype):
    """a on the device as a column slice of rows `pad` elements wider (ld > N), starting one element in."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)
    if not pad:
        return t
    wide = torch.full((a.shape[0], a.shape[1] + pad), 7, dtype=dtype, device=DEV)
    wide[:, 1:1 + a.shape[1]] = t
    return wide[:, 1:1 + a.shape[1]]


def assert_equal(got, want):
    rc_, psum, count, csum = got.host()
    np.testing.assert_array_equal(rc_, want.row_counts)
    np.testing.assert_array_equal(psum, want.psum)
    np.testing.assert_array_equal(count, want.class_count)
    np.testing.assert_array_equal(csum, want.class_psum)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", WIDTHS)
def test_counts_and_sums_equal_the_host_definition(n, rows):
    """Every width x every row count; the grid, k, the target dtype and the row strides rotate over the cases."""
    i = WIDTHS.index(n) + ROWS.index(rows)
    grid = rc.GRIDS[i % len(rc.GRIDS)]
    k = (1, min(5, n), n)[i % 3]
    y, s = rc.case(rows, n, grid, 100 * n + rows)
    pad_s, pad_t = (0, 3)[i % 2], (0, 5)[(i // 2) % 2]
    tdtype = (torch.uint8, torch.float32, torch.bool)[i % 3]
    got = ranking.ranking_metrics(padded(y, pad_t, tdtype), padded(s, pad_s, torch.float32), k=k)
    assert_equal(got, host((rows, n, grid), y, s, k))


@pytest.mark.parametrize("n", (65, SWITCH + 1))
def test_every_grid_density_and_k(n):
    """Both row kernels on all-equal rows, heavy ties, no ties and the float32 edge values, rows of 0, 1, a few, N - 1 and N
    positives, k = 1, 5 and N; the derived values agree with the host's to the last bit as well."""
    for grid in rc.GRIDS:
        y, s = rc.case(8, n, grid, n + 17)
        for k in (1, 5, n):
            got = ranking.ranking_metrics(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV), k=k)
            want = host((8, n, grid), y, s, k)
            assert_equal(got, want)
            assert got.summary() == want.summary()
            np.testing.assert_array_equal(got.per_class_lwlrap, want.per_class_lwlrap)
            np.testing.assert_array_equal(got.class_weight, want.class_weight)


def test_the_widest_head():
    """32 768 classes -- 128 KiB of keys in LDS -- on a handful of rows of at most 8 positives, with row strides."""
    n = _ffi.MAX_CLASSES
    for grid, k in ((None, 5), (4, n), ("edge", 1)):
        y, s = rc.case(5, n, grid, 9, kinds=rc.SPARSE)
        assert y.sum(axis=1).max() <= 8
        y[4, n - 1] = 1                                                  # the last bit of the last ballot word
        got = ranking.ranking_metrics(padded(y, 64, torch.uint8), padded(s, 1, torch.float32), k=k)
        assert_equal(got, ranking.ranking_metrics_host(y, s, k=k))


@pytest.mark.parametrize("n", (527, SWITCH + 1))
def test_slices_and_repeats_leave_the_bits(n):
    """257 rows as 17 slices of 16 (a short last one), as 2 slices, and as one: the same bits; and the same bits again."""
    y, s = rc.case(257, n, 4, 100 * n + 257)
    yd, sd = torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV)
    one = ranking.ranking_metrics(yd, sd, k=5)
    assert_equal(one, host((257, n, 4), y, s, 5))
    for slice_rows in (16, 129, 257, None):
        other = ranking.ranking_metrics(yd, sd, k=5, slice_rows=slice_rows)
        for a, b in zip(one.host(), other.host()):
            assert a.tobytes() == b.tobytes(), slice_rows


def test_derived_scalars_against_sklearn():
    from sklearn.metrics import coverage_error, label_ranking_average_precision_score, label_ranking_loss
    rng = np.random.default_rng(5)
    rows, n = 2000, 527
    y = (rng.random((rows, n)) < 2.5 / n).astype(np.uint8)
    y[0], y[1] = 0, 1
    s = (rng.random((rows, n)) * 64).astype(np.int32).astype(np.float32) / 64.0 + 0.5 * y            # a 1/64 grid: ties, and signal
    got = ranking.ranking_metrics(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV), k=3)
    n_pos = y.sum(axis=1)
    has = n_pos > 0
    diffs = {"lrap": got.lrap - label_ranking_average_precision_score(y, s),
             "coverage_error": got.coverage_error - coverage_error(y, s),
             "ranking_loss": got.ranking_loss - label_ranking_loss(y, s),
             "lwlrap": got.lwlrap - label_ranking_average_precision_score(y[has], s[has], sample_weight=n_pos[has])}
    print("device vs sklearn (2000, 527):", {k: "%.2e" % abs(v) for k, v in diffs.items()})
    for name, d in diffs.items():
        assert abs(d) <= 1e-12, (name, d)
    assert 0.0 <= got.one_error <= 1.0 and got.one_error == ranking.ranking_metrics_host(y, s, k=3).one_error      # k > 1: a second call


@pytest.mark.parametrize("n", (65, SWITCH + 1))
def test_device_data_errors_raise_on_read(n):
    y, s = rc.case(6, n, None, 3)
    for message, bad_y, bad_s in (("NaN or infinite", None, np.nan), ("NaN or infinite", None, -np.inf), ("other than 0 and 1", 2, None)):
        yy, ss = y.copy(), s.copy()
        if bad_y is not None:
            yy[3, n - 1] = bad_y
        else:
            ss[5, n // 2] = bad_s
        for tdtype in (torch.uint8, torch.float32):
            got = ranking.ranking_metrics(torch.from_numpy(yy).to(DEV).to(tdtype), torch.from_numpy(ss).to(DEV))      # not yet
            assert tuple(got.psum.shape) == (6,) and got.psum.is_cuda
            with pytest.raises(ValueError, match=message):
                got.lrap
    with pytest.raises(ValueError, match="NaN or infinite"):                                  # host inputs: before any copy
        ranking.ranking_metrics(y, np.where(s == s[0, 0], np.inf, s))
    with pytest.raises(ValueError, match="other than 0 and 1"):
        ranking.ranking_metrics(y * 3, s)
    assert_equal(ranking.ranking_metrics(y, s), ranking.ranking_metrics_host(y, s))           # and host inputs as such


def test_captured_call_replays_the_eager_bits():
    y, s = rc.case(21, 527, 2, 77)
    yd, sd = torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV)
    eager = ranking.ranking_metrics(yd, sd, k=5, slice_rows=8).host()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ranking.ranking_metrics(yd, sd, k=5, slice_rows=8)                                    # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ranking.ranking_metrics(yd, sd, k=5, slice_rows=8)
    for t in (captured.row_counts, captured.psum, captured._class_count, captured.class_psum):
        t.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured.host()):
        assert a.tobytes() == b.tobytes()


def test_bootstrap_intervals():
    y, s = rc.case(120, 33, 4, 5)
    out = ranking.bootstrap_ranking(y, s, replicates=64, seed=3, chunk=24)
    full = ranking.ranking_metrics(y, s)
    for name in ("lrap", "lwlrap", "ranking_loss", "coverage_error"):
        v = out[name]
        assert v["estimate"] == getattr(full, name) and v["replicates"].shape == (64,)
        assert v["low"] <= v["estimate"] <= v["high"], (name, v["low"], v["estimate"], v["high"])
        assert v["low"] < v["high"]
    again = ranking.bootstrap_ranking(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV), replicates=64, seed=3)
    np.testing.assert_array_equal(again["lwlrap"]["replicates"], out["lwlrap"]["replicates"])
    assert out["confidence"] == 0.95 and out["seed"] == 3
