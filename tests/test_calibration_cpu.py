"""CPU: calibration (pytorch/calibration.py, the "calibration" section of include/acx.h) without a device -- the float64 host
definitions on hand-worked cases, their own optimality on every generated case the GPU tests use, the ctypes declarations and the
argument errors that need no launch, and the save / load formats."""
import ctypes

import numpy as np
import pytest
import torch

import calibration_cases as cc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import calibration as cal


# ---- the host definitions on hand-worked cases -----------------------------------------------------------------------------------
def test_four_scores_in_two_bins():
    """p = (0.1, 0.4 | 0.6, 0.9), y = (0, 1 | 1, 1): bin 0 holds two rows, one positive, confidence 0.25; bin 1 two rows, two
    positives, confidence 0.75.  ECE = 0.5 |0.5 - 0.25| + 0.5 |1 - 0.75| = 0.25, MCE = 0.25, Brier = (0.01 + 0.36 + 0.16 +
    0.01) / 4."""
    p = np.array([[0.1], [0.4], [0.6], [0.9]], dtype=np.float32)
    y = np.array([[0], [1], [1], [1]])
    r = cal.reliability_host(y, p, bins=2)
    assert r.count.tolist() == [[2, 2]] and r.positive.tolist() == [[1, 2]]
    p64 = p.astype(np.float64)[:, 0]
    assert r.conf_sum[0].tolist() == [p64[0] + p64[1], p64[2] + p64[3]]
    assert abs(r.ece[0] - 0.25) < 1e-7 and abs(r.mce[0] - 0.25) < 1e-7 and abs(r.classwise_ece - 0.25) < 1e-7
    assert abs(r.brier[0] - 0.135) < 1e-7
    conf, freq, count = r.curve(0)
    assert np.allclose(conf, [0.25, 0.75], atol=1e-7) and freq.tolist() == [0.5, 1.0] and count.tolist() == [2, 2]


@pytest.mark.parametrize("bins", cc.EDGE_BINS)
def test_edges_belong_to_the_bin_they_open(bins):
    p, y, expect = cc.edge_probabilities(bins)
    assert cal.bin_index_host(p[:, 0], bins).tolist() == expect.tolist()
    r = cal.reliability_host(y, p, bins=bins)
    assert r.count[0].tolist() == np.bincount(expect, minlength=bins).tolist()


def test_two_point_platt_problem_has_its_closed_form():
    """One positive at z = 1, one negative at z = -1, Platt's targets 2/3 and 1/3: the minimiser interpolates them, sigmoid(a + b)
    = 2/3 and sigmoid(b - a) = 1/3, i.e. b = 0 and a = log 2."""
    ab, info = cal.fit_platt_host(np.array([[1], [0]]), np.array([[1.0], [-1.0]], dtype=np.float32))
    assert info[0] > 0
    assert abs(ab[0, 0] - np.log(2.0)) < 1e-9 and abs(ab[0, 1]) < 1e-9
    # without smoothing the two points are separable: no minimiser, the iteration cap reports it
    ab, info = cal.fit_platt_host(np.array([[1], [0]]), np.array([[1.0], [-1.0]], dtype=np.float32), smooth=False)
    assert info[0] == cal.NOT_CONVERGED


def test_top_label_host_on_a_worked_case():
    z = np.log(np.array([[0.7, 0.2, 0.1], [0.3, 0.6, 0.1], [0.5, 0.25, 0.25]], dtype=np.float64)).astype(np.float32)
    r = cal.reliability_toplabel_host([0, 0, 2], z, bins=10)
    assert r.count.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 0, 0] or r.count.sum() == 3      # 0.7 / 0.6 / 0.5 up to float32 rounding
    assert r.correct.sum() == 1 and abs(r.accuracy - 1 / 3) < 1e-12
    assert abs(r.nll - (-np.log(0.7) - np.log(0.3) - np.log(0.25)) / 3) < 1e-6
    assert r.skipped == 0
    r = cal.reliability_toplabel_host([0, -1, 3], z, bins=10)
    assert r.skipped == 2 and r.count.sum() == 1


def test_platt_apply_host_identity_is_the_sigmoid():
    z = np.linspace(-30, 30, 13, dtype=np.float32)[:, None]
    p = cal.platt_apply_host(z, np.array([[1.0, 0.0]]))
    assert np.allclose(p[:, 0], 1.0 / (1.0 + np.exp(-z[:, 0].astype(np.float64))), rtol=1e-14, atol=0)


# ---- the host fits keep themselves inside the bound the GPU tests use -------------------------------------------------------------
def _platt_shapes():
    return [(n, C) for n in cc.PLATT_ROWS for C in cc.PLATT_CLASSES] + [cc.PLATT_STREAMED]


@pytest.mark.parametrize("n,C,smooth", [(n, C, s) for n, C in _platt_shapes() for s in (True, False)
                                        if s or n > 2])          # two points without smoothing are separable
def test_fit_platt_host_is_optimal_on_every_gpu_case(n, C, smooth):
    z, y = cc.multilabel(n, C)
    ab, info = cal.fit_platt_host(y, z, smooth=smooth)
    for c in range(C):
        assert info[c] >= 0, (c, info[c])
        step, lam = cal.platt_newton_step_host(z[:, c], y[:, c], ab[c, 0], ab[c, 1], smooth)
        assert lam > 0
        assert np.abs(step).max() <= cc.platt_bound(z[:, c], ab[c, 0], ab[c, 1], lam), (c, step)


def test_fit_platt_host_degenerate_families():
    z, y = cc.degenerate_multilabel()
    ab, info = cal.fit_platt_host(y, z)
    assert info[0] > 0 and info[1:].tolist() == [cal.DEGENERATE] * 3
    assert ab[1:].tolist() == [[1.0, 0.0]] * 3
    z, y = cc.separable()
    ab, info = cal.fit_platt_host(y, z, smooth=False)
    assert info[0] > 0 and info[1] == cal.NOT_CONVERGED
    with pytest.raises(ValueError, match="NaN"):
        cal.fit_platt_host(y, np.where(np.arange(z.size).reshape(z.shape) == 3, np.nan, z))
    with pytest.raises(ValueError, match="other than 0 and 1"):
        cal.fit_platt_host(y.astype(np.int64) * 2, z)


@pytest.mark.parametrize("n,N", cc.TOPLABEL_SHAPES)
@pytest.mark.parametrize("beta_star", cc.PLANTED_BETAS)
def test_fit_temperature_host_is_optimal_on_every_gpu_case(n, N, beta_star):
    z, y = cc.singlelabel(n, N, beta_star)
    beta, info = cal.fit_temperature_host(y, z, evaluations=cc.TEMPERATURE_EVALUATIONS)
    if n == 1:                                                     # one row whose label is its maximum: F falls for ever, beta
        assert z[0].argmax() == y[0] and info == cal.NOT_CONVERGED  # grows by about 1 / gap per evaluation
    else:
        assert info > 0, info
    if info > 0:
        _, g, h, _ = cal.temperature_sums_host(y, z, beta)
        assert abs(g / max(h, 1e-12)) <= cc.temperature_bound(z, beta, max(h, 1e-12)), (beta, g, h)
    if n >= 257:                                                   # enough rows to see the planted value
        assert info > 0 and abs(np.log(beta / beta_star)) < 0.3, beta


def test_fit_temperature_host_codes():
    z, y = cc.constant_rows()
    assert cal.fit_temperature_host(y, z) == (1.0, cal.DEGENERATE)
    z, y = cc.singlelabel(65, 5, 1.0)
    beta, info = cal.fit_temperature_host(y, z, evaluations=1)
    assert (beta, info) == (1.0, cal.NOT_CONVERGED)
    for name, (z, y) in cc.bound_cases().items():
        beta, info = cal.fit_temperature_host(y, z, evaluations=cc.TEMPERATURE_EVALUATIONS)
        assert info == cal.AT_BOUND, (name, beta, info)
        assert (beta > 9.99e3) if name == "high" else (beta < 1.001e-4), (name, beta)


def test_fit_platt_host_against_sklearn():
    """fit_platt_host(smooth=False) against LogisticRegression(C=1e12) on the regular cases.  Tolerance: the larger of the two
    solvers' own gradient norms at their answers, mapped through the host Hessian (|H^-1 g|_inf), doubled; lbfgs at tol=1e-10
    leaves |g| near 1e-8 on these inputs, the host Newton near 1e-13, so the bound is a few 1e-9 -- measured, printed below."""
    lm = pytest.importorskip("sklearn.linear_model")
    z, y = cc.multilabel(1025, 3)
    ab, info = cal.fit_platt_host(y, z, smooth=False)
    for c in range(3):
        lr = lm.LogisticRegression(C=1e12, tol=1e-10, max_iter=1000).fit(z[:, c:c + 1].astype(np.float64), y[:, c])
        sk = np.array([lr.coef_[0, 0], lr.intercept_[0]])
        tol = 0.0
        for point in (ab[c], sk):
            _, g, H, _ = cal.platt_sums_host(z[:, c], y[:, c], point[0], point[1], smooth=False)
            tol = max(tol, float(np.abs(np.linalg.solve(H, g)).max()))
        print("class %d: host %s sklearn %s tolerance %.3e" % (c, ab[c], sk, 2 * tol))
        assert np.abs(ab[c] - sk).max() <= 2 * tol + 1e-12


# ---- the C ABI without a launch -------------------------------------------------------------------------------------------------
def test_declarations_and_constants():
    names = ["acx_reliability_counts", "acx_reliability_toplabel", "acx_platt_workspace_bytes", "acx_platt_fit", "acx_platt_apply",
             "acx_temperature_workspace_bytes", "acx_temperature_fit", "acx_temperature_apply"]
    lib = _ffi.lib()
    for name in names:
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert _ffi.SIGNATURES[name][0] is ctypes.c_int
    hdr = open(cc.__file__.replace("tests/calibration_cases.py", "include/acx.h")).read()
    for macro, value in (("ACX_CAL_MAX_BINS", _ffi.CAL_MAX_BINS), ("ACX_CAL_MAX_EVALUATIONS", _ffi.CAL_MAX_EVALUATIONS),
                         ("ACX_CAL_NONFINITE", _ffi.CAL_NONFINITE), ("ACX_CAL_BAD_TARGET", _ffi.CAL_BAD_TARGET),
                         ("ACX_CAL_BAD_PROBABILITY", _ffi.CAL_BAD_PROBABILITY), ("ACX_CAL_BAD_LABEL", _ffi.CAL_BAD_LABEL)):
        assert "#define %s %d\n" % (macro, value) in hdr, macro
    for macro, value in (("ACX_CAL_DEGENERATE", -1), ("ACX_CAL_NOT_CONVERGED", -2), ("ACX_CAL_AT_BOUND", -3)):
        assert "#define %s (%d)\n" % (macro, value) in hdr, macro
    assert (_ffi.CAL_DEGENERATE, _ffi.CAL_NOT_CONVERGED, _ffi.CAL_AT_BOUND) == (-1, -2, -3)


def test_workspace_sizes():
    assert _ffi.platt_workspace_bytes(1, 1) >= 5 and _ffi.platt_workspace_bytes(1, 1) % 256 == 0
    assert _ffi.platt_workspace_bytes(20371, 527) >= 20371 * 527 * 5
    assert _ffi.temperature_workspace_bytes(1, 2) % 256 == 0
    assert _ffi.temperature_workspace_bytes(100000, 50) >= 256 + 32 * 100000
    for fn in (_ffi.platt_workspace_bytes, _ffi.temperature_workspace_bytes):
        for n, C in ((0, 1), (1, 0), (1, _ffi.MAX_CLASSES + 1), (2 ** 30 + 1, 1)):
            with pytest.raises(_ffi.AcxError):
                fn(n, C)


def test_argument_errors_need_no_launch():
    """Every call checks its arguments before it touches the device: with a fake non-null pointer nothing may be read."""
    lib = _ffi.lib()
    P = ctypes.c_void_p(256)                                       # never dereferenced: each call below fails its checks first
    err = lambda: lib.acx_last_error().decode()
    for bins in (0, 65):
        assert lib.acx_reliability_counts(P, 4, P, _ffi.TARGET_U8, 4, 8, 4, bins, P, P, P, P, P, None) == -1 and "bins" in err()
        assert lib.acx_reliability_toplabel(P, 4, P, 8, 4, None, bins, P, P, P, P, P, P, 1 << 20, None) == -1 and "bins" in err()
    assert lib.acx_reliability_counts(P, 4, P, _ffi.TARGET_U8, 4, 8, _ffi.MAX_CLASSES + 1, 15, P, P, P, P, P, None) == -1
    assert "classes" in err()
    assert lib.acx_reliability_counts(P, 3, P, _ffi.TARGET_U8, 4, 8, 4, 15, P, P, P, P, P, None) == -1 and "ld" in err()
    assert lib.acx_reliability_counts(P, 4, P, 7, 4, 8, 4, 15, P, P, P, P, P, None) == -1 and "target_dtype" in err()
    for k in range(4):                                             # each NULL output in turn
        outs = [None if i == k else P for i in range(4)]
        assert lib.acx_reliability_counts(P, 4, P, _ffi.TARGET_U8, 4, 8, 4, 15, *outs, P, None) == -1 and "null" in err()
        assert lib.acx_reliability_toplabel(P, 4, P, 8, 4, None, 15, *outs, P, P, 1 << 20, None) == -1 and "null" in err()
    assert lib.acx_reliability_counts(P, 4, P, _ffi.TARGET_U8, 4, 8, 4, 15, P, P, P, P, None, None) == -1 and "status" in err()
    for ev in (0, 65):
        assert lib.acx_temperature_fit(P, 4, P, 8, 4, ev, P, P, P, P, 1 << 20, None) == -1 and "evaluations" in err()
    assert lib.acx_temperature_fit(P, 4, P, 8, 4, 8, None, P, P, P, 1 << 20, None) == -1 and "null" in err()
    assert lib.acx_temperature_fit(P, 4, P, 8, 4, 8, P, P, P, P, 16, None) == -5                  # workspace too small
    assert lib.acx_temperature_fit(P, 4, P, 8, 4, 8, P, P, P, ctypes.c_void_p(8), 1 << 20, None) == -5   # not 256-byte aligned
    assert lib.acx_platt_fit(P, 4, P, _ffi.TARGET_U8, 4, 8, _ffi.MAX_CLASSES + 1, 1, P, P, P, P, 1 << 20, None) == -1
    assert lib.acx_platt_fit(P, 4, P, _ffi.TARGET_U8, 4, 8, 4, 1, None, P, P, P, 1 << 20, None) == -1 and "null" in err()
    assert lib.acx_platt_fit(P, 4, P, _ffi.TARGET_U8, 4, 8, 4, 1, P, P, P, P, 16, None) == -5
    assert lib.acx_platt_apply(P, 4, 8, 4, None, P, 4, None) == -1 and "ab" in err()
    assert lib.acx_platt_apply(P, 4, 8, 4, P, P, 3, None) == -1 and "ld_p" in err()
    assert lib.acx_temperature_apply(P, 4, 8, 4, None, P, 4, None) == -1 and "beta" in err()
    assert lib.acx_temperature_apply(P, 4, 0, 4, P, P, 4, None) == -1


def test_python_argument_errors():
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="bins"):
        cal.reliability(z > 0, z, bins=0)
    with pytest.raises(ValueError, match="bins"):
        cal.reliability(z > 0, z, bins=65)
    with pytest.raises(ValueError, match="one shape"):
        cal.reliability(torch.zeros(4, 2), z)
    with pytest.raises(ValueError, match="CUDA"):
        cal.fit_temperature(torch.zeros(4, dtype=torch.int64), z)
    with pytest.raises(ValueError, match="evaluations"):
        cal.fit_temperature(torch.zeros(4, dtype=torch.int64), z, evaluations=0)


# ---- save / load -------------------------------------------------------------------------------------------------------------------
def test_saved_files_round_trip(tmp_path):
    """The .npz formats, written through the classes on CPU tensors and read back with numpy (load() itself places the tensors on
    a CUDA device: tests/test_gpu_calibration.py)."""
    ab = torch.tensor([[1.25, -0.5], [1.0, 0.0]], dtype=torch.float64)
    p = cal.PlattScaling(ab, torch.tensor([7, cal.DEGENERATE], dtype=torch.int32))
    path = str(tmp_path / "platt.npz")
    p.save(path)
    with np.load(path) as f:
        assert str(f["method"]) == "platt" and f["ab"].dtype == np.float64 and f["ab"].tolist() == ab.tolist()
        assert f["info"].tolist() == [7, -1]
    t = cal.TemperatureScaling(torch.tensor([0.8], dtype=torch.float64), torch.tensor([9], dtype=torch.int32))
    assert t.temperature == 1.25
    path2 = str(tmp_path / "temperature.npz")
    t.save(path2)
    with np.load(path2) as f:
        assert str(f["method"]) == "temperature" and f["beta"].tolist() == [0.8] and f["info"].tolist() == [9]
    if not torch.cuda.is_available():
        with pytest.raises((ValueError, RuntimeError, AssertionError)):
            cal.load_calibration(path)                             # no device to place it on
    np.savez(str(tmp_path / "other.npz"), method="isotonic")
    with pytest.raises(ValueError, match="unknown calibration method"):
        cal.load_calibration(str(tmp_path / "other.npz"))
    with pytest.raises(ValueError, match="not temperature"):
        cal.TemperatureScaling.load(path, device="cuda:0")
