"""CPU: the host definition of the ranking metrics (pytorch/ranking.py) against scikit-learn's three functions and the DCASE
lwlrap formula, hand-worked rows, the replicate arithmetic of bootstrap_ranking, and the host-only paths of the C ABI
(declarations, argument errors, the workspace query)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ranking_cases as rc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import metrics, ranking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12          # sklearn adds the same float64 terms in another order: a few units of 2^-53 on values of order 1 .. N


# ---- ranking_metrics_host against sklearn ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n,grid", [(50, 7, 3), (40, 65, 4), (30, 527, None), (20, 5, 1), (25, 2, 2), (24, 33, "edge"),
                                         (16, 64, 2), (16, 63, None)])
def test_host_definition_equals_sklearn(rows, n, grid):
    from sklearn.metrics import coverage_error, label_ranking_average_precision_score, label_ranking_loss
    y, s = rc.case(rows, n, grid, 7 * rows + n)
    assert (y.sum(axis=1) == 0).any() and (y.sum(axis=1) == n).any()                  # one all-zero and one all-one row at least
    r = ranking.ranking_metrics_host(y, s, k=min(3, n))
    n_pos = y.sum(axis=1)
    has = n_pos > 0
    with np.errstate(invalid="ignore", over="ignore"):              # sklearn's finiteness check sums the float32 extremes
        diffs = {"lrap": r.lrap - label_ranking_average_precision_score(y, s),
                 "coverage_error": r.coverage_error - coverage_error(y, s),
                 "ranking_loss": r.ranking_loss - label_ranking_loss(y, s),
                 "lwlrap": r.lwlrap - label_ranking_average_precision_score(y[has], s[has], sample_weight=n_pos[has])}
    print("host vs sklearn (%d, %d, %s): %s" % (rows, n, grid, {k: "%.2e" % abs(v) for k, v in diffs.items()}))
    for name, d in diffs.items():
        assert abs(d) <= BAR, (name, d)
    # the two ways to lwlrap the definition states
    w, pc = r.class_weight, r.per_class_lwlrap
    assert abs(np.nansum(w * pc) - r.lwlrap) <= BAR
    assert (np.isnan(pc) == (r.class_count == 0)).all() and abs(w.sum() - 1.0) <= BAR


@pytest.mark.parametrize("rows,n", [(30, 7), (20, 65), (12, 527), (9, 2)])
def test_lwlrap_equals_the_dcase_formula_without_ties(rows, n):
    y, s = rc.case(rows, n, None, 3 * rows + n)
    r = ranking.ranking_metrics_host(y, s)
    per_class, weight, lwlrap = rc.dcase_lwlrap(y, s)
    seen = r.class_count > 0
    worst = max(abs(r.lwlrap - lwlrap), np.abs(r.per_class_lwlrap[seen] - per_class[seen]).max(), np.abs(r.class_weight - weight).max())
    print("host vs DCASE formula (%d, %d): %.2e" % (rows, n, worst))
    assert worst <= BAR


def test_hand_worked_rows():
    host = lambda y, s, **kw: ranking.ranking_metrics_host(np.array(y, np.uint8), np.array(s, np.float32), **kw)
    one = host([[1], [0]], [[0.3], [0.3]])                                            # N = 1: sklearn refuses it
    assert one.row_counts.tolist() == [[1, 1, 0, 1], [0, 0, 0, 0]] and one.psum.tolist() == [1.0, 0.0]
    assert (one.lrap, one.ranking_loss, one.coverage_error, one.lwlrap, one.one_error) == (1.0, 0.0, 0.5, 1.0, 0.5)
    tied = host([[0, 1, 0, 1]], [[0.5, 0.5, 0.5, 0.5]], k=2)                          # ge = 4, pge = 2 twice; ord = 1 and 3
    assert tied.row_counts.tolist() == [[2, 4, 4, 1]] and tied.psum.tolist() == [1.0]
    assert (tied.lrap, tied.ranking_loss, tied.one_error, tied.precision_at_k, tied.recall_at_k) == (0.5, 1.0, 1.0, 0.5, 0.5)
    assert host([[0, 1, 0, 1]], [[0.5, 0.5, 0.5, 0.5]], k=1).row_counts.tolist() == [[2, 4, 4, 0]]
    last = host([[0, 0, 0, 1]], [[3.0, 2.0, 1.0, 0.0]])
    assert last.row_counts.tolist() == [[1, 4, 3, 0]] and last.psum.tolist() == [0.25] and last.ranking_loss == 1.0
    assert host([[0, 0, 0, 1]], [[3.0, 2.0, 1.0, 0.0]], k=4).row_counts.tolist() == [[1, 4, 3, 1]]
    mixed = host([[0, 1, 0, 0], [0, 0, 1, 0]], [[0.9, 0.5, 0.5, 0.1]] * 2, k=2)       # a positive tied with a negative
    assert mixed.row_counts.tolist() == [[1, 3, 2, 1], [1, 3, 2, 0]]                  # the lower class index goes first
    assert mixed.psum.tolist() == [1.0 / 3.0, 1.0 / 3.0] and mixed.class_count.tolist() == [0, 1, 1, 0]
    assert mixed.class_psum.tolist() == [0.0, 1.0 / 3.0, 1.0 / 3.0, 0.0]
    zeros = host([[0, 1, 0]], [[-0.0, 0.0, 1e-45]], k=2)                              # -0.0 == +0.0; a denormal is above both
    assert zeros.row_counts.tolist() == [[1, 3, 2, 0]] and zeros.psum.tolist() == [1.0 / 3.0]
    assert host([[0, 1, 0]], [[-0.0, 0.0, 1e-45]], k=3).row_counts.tolist() == [[1, 3, 2, 1]]


def test_class_sums_run_in_ascending_row():
    y, s = rc.case(40, 5, 4, 11)
    r = ranking.ranking_metrics_host(y, s)
    for c in range(5):
        acc = 0.0
        for i in range(40):
            if y[i, c]:
                pos = np.flatnonzero(y[i])
                acc += float((s[i, pos] >= s[i, c]).sum()) / float((s[i] >= s[i, c]).sum())
        assert r.class_psum[c] == acc and r.class_count[c] == y[:, c].sum()


def test_value_errors_need_no_device():
    y, s = rc.case(6, 5, 4, 1)
    for call in (ranking.ranking_metrics_host, ranking.ranking_metrics):
        with pytest.raises(ValueError, match="k must be"):
            call(y, s, k=0)
        with pytest.raises(ValueError, match="k must be"):
            call(y, s, k=6)
        with pytest.raises(ValueError, match="differs"):
            call(y[:, :4], s)
        bad = s.copy()
        bad[2, 3] = np.nan
        with pytest.raises(ValueError, match="NaN or infinite"):
            call(y, bad)
        two = y.copy()
        two[1, 1] = 2
        with pytest.raises(ValueError, match="other than 0 and 1"):
            call(two, s)
    with pytest.raises(ValueError, match="slice_rows"):
        ranking.ranking_metrics(y, s, slice_rows=0)
    with pytest.raises(ValueError, match="not cpu"):
        ranking.ranking_metrics(y, s, device="cpu")
    with pytest.raises(ValueError, match="replicates"):
        ranking.bootstrap_ranking(y, s, replicates=0)
    with pytest.raises(ValueError, match="confidence"):
        ranking.bootstrap_ranking(y, s, confidence=1.0)


# ---- bootstrap_ranking's replicate arithmetic ----------------------------------------------------------------------------------
def test_replicates_are_weights_times_row_columns():
    rows, C, R, seed = 37, 9, 12, 5
    rng = np.random.default_rng(3)
    n_pos = rng.integers(0, C + 1, rows)
    n_pos[:2] = (0, C)
    coverage = np.where(n_pos > 0, rng.integers(1, C + 1, rows), 0)
    bad = rng.integers(0, 20, rows)
    psum = rng.random(rows) * n_pos
    got = ranking.replicate_statistics(torch.from_numpy(metrics.bootstrap_weights_host(seed, R, rows)), torch.from_numpy(n_pos),
                                       torch.from_numpy(coverage), torch.from_numpy(bad), torch.from_numpy(psum), C).numpy()
    full = (n_pos == 0) | (n_pos == C)
    lrap_i = np.where(full, 1.0, psum / np.where(full, 1, n_pos))
    loss_i = np.where(full, 0.0, bad / np.where(full, 1, n_pos * (C - n_pos)))
    for r in range(R):
        idx = metrics.bootstrap_indices_host(seed, r, rows)
        want = [lrap_i[idx].mean(), psum[idx].sum() / n_pos[idx].sum(), loss_i[idx].mean(), coverage[idx].mean()]
        np.testing.assert_allclose(got[r], want, rtol=1e-12, atol=0)


# ---- the C ABI: host-only paths ------------------------------------------------------------------------------------------------
NAMES = ("acx_ranking_workspace_bytes", "acx_ranking_metrics")


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    lib = _ffi.lib()
    for name in NAMES:
        assert re.search(r"ACX_API int %s\(" % name, header), name
        assert name in _ffi.SIGNATURES and _ffi.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(lib, name)
    assert [len(_ffi.SIGNATURES[k][1]) for k in NAMES] == [4, 17]
    for name, value in (("ACX_RANK_COUNTS", _ffi.RANK_COUNTS), ("ACX_RANK_WAVE_MAX_CLASSES", _ffi.RANK_WAVE_MAX_CLASSES)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    for name, value in (("N_POS", _ffi.RANK_N_POS), ("COVERAGE", _ffi.RANK_COVERAGE), ("BAD_PAIRS", _ffi.RANK_BAD_PAIRS),
                        ("HITS", _ffi.RANK_HITS)):
        assert re.search(r"ACX_RANK_%s = %d\b" % (name, value), header), name


def test_workspace_query_follows_the_slice():
    ws = _ffi.ranking_workspace_bytes
    assert ws(1000, 527, 16) == 16 * 527 * 8 + 128 == ws(16, 527, 16) == ws(1 << 20, 527, 16)      # 67456 -> 67584: 256-aligned
    assert ws(8, 527, 16) == 8 * 527 * 8 + 64                                                     # fewer rows than a slice
    sizes = [ws(5000, 80, s) for s in (1, 2, 15, 16, 17, 1000, 4999, 5000, 5001, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[-1] == sizes[-3] == 5000 * 80 * 8
    default = (1 << 26) // (8 * 527)                                                              # 15 917 rows of 527 classes
    assert ws(1 << 30, 527, 0) == ws(default, 527, 0) == (default * 527 * 8 + 255) // 256 * 256 > ws(default - 1, 527, 0)
    assert ws(1 << 20, 32768, 0) == 256 * 32768 * 8                                               # never under 256 rows
    for args in ((0, 8, 0), ((1 << 30) + 1, 8, 0), (8, 0, 0), (8, _ffi.MAX_CLASSES + 1, 0), (8, 8, -1), (1 << 23, 8, 1)):
        with pytest.raises(_ffi.AcxError, match="acx_ranking_workspace_bytes"):
            ws(*args)


P = lambda v: None if v is None else ctypes.c_void_p(v)


def _rank_rc(scores=64, ld_s=8, target=64, dtype=_ffi.TARGET_U8, ld_t=8, rows=4, classes=8, k=1, slice_rows=0, counts=64, psum=64,
             ccount=64, cpsum=64, st=64, ws=256, ws_bytes=1 << 30):
    return _ffi.lib().acx_ranking_metrics(P(scores), ld_s, P(target), dtype, ld_t, rows, classes, k, slice_rows, P(counts), P(psum),
                                          P(ccount), P(cpsum), P(st), P(ws), ws_bytes, None)


def test_argument_errors_return_before_any_launch():
    """Made-up (never dereferenced) pointers: every argument error of the header's list is negative without a device."""
    lib = _ffi.lib()
    for kw in (dict(scores=None), dict(target=None), dict(counts=None), dict(psum=None), dict(ccount=None), dict(cpsum=None),
               dict(st=None), dict(ws=None), dict(rows=0), dict(classes=0), dict(classes=_ffi.MAX_CLASSES + 1, ld_s=1 << 20, ld_t=1 << 20),
               dict(k=0), dict(k=9), dict(ld_s=7), dict(ld_t=7), dict(dtype=2), dict(slice_rows=-1)):
        assert _rank_rc(**kw) == -1, kw
        assert b"acx_ranking_metrics" in lib.acx_last_error(), kw
    assert _rank_rc(rows=(1 << 30) + 1) == -6
    assert _rank_rc(ws_bytes=4 * 8 * 8 - 1) == -5 and _rank_rc(ws=264) == -5
    assert b"acx_ranking_metrics" in lib.acx_last_error()
    assert b"k = 9" in (_rank_rc(k=9), lib.acx_last_error())[1]
