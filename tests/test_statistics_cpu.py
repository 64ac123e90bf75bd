"""CPU: the host definitions of the embedding statistics (pytorch/statistics.py) against numpy, LAPACK, scikit-learn and scipy,
the recorded bars of statistics_cases.py, and the host-only paths of the C ABI (declarations, argument errors)."""
import ctypes
import os
import re

import numpy as np
import pytest

import statistics_cases as sc
from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import statistics as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- moments_host --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(2, 1), (5, 3), (64, 17), (257, 50), (300, 192)])
def test_moments_host_equals_numpy(n, dim):
    x = sc.gaussian_rows(n, dim, n + dim, offset=100.0)
    for ddof in (0, 1):
        mo = st.moments_host(x, ddof)
        x64 = x.astype(np.float64)
        assert (np.abs(mo.cov - np.cov(x64, rowvar=False, ddof=ddof).reshape(dim, dim)) <= sc.moments_bound(x, ddof)).all()
        assert (np.abs(mo.mean - np.mean(x64, axis=0)) <= 2 * n * sc.U * np.abs(x64).mean(axis=0)).all()
        np.testing.assert_array_equal(mo.cov, mo.cov.T)
    # integer rows with integer means: the scatter is an exact integer matrix, so cov is that matrix divided once -- EQUAL to
    # numpy.mean always, and to numpy.cov wherever its own scaling is exact too (numpy.cov multiplies by 1 / (n - ddof), which
    # is one more rounding unless n - ddof is a power of two)
    e = sc.exact_rows(n, dim, 5 * n + dim)
    i64 = e.astype(np.int64)
    centred = i64 - i64.sum(axis=0) // n
    for ddof in (0, 1):
        mo = st.moments_host(e, ddof)
        np.testing.assert_array_equal(mo.mean, np.mean(e.astype(np.float64), axis=0))
        np.testing.assert_array_equal(mo.cov, (centred.T @ centred).astype(np.float64) / (n - ddof))
        if (n - ddof) & (n - ddof - 1) == 0:
            np.testing.assert_array_equal(mo.cov, np.cov(e.astype(np.float64), rowvar=False, ddof=ddof).reshape(dim, dim))


def test_moments_host_edges():
    one = st.moments_host(np.array([[1.0, 2.0]], np.float32), 1)
    assert not one.cov.any() and one.n == 1 and one.mean.tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="ddof"):
        st.moments_host(np.zeros((3, 2)), 2)
    with pytest.raises(ValueError, match="2-D"):
        st.moments_host(np.zeros(3))
    with pytest.raises(ValueError, match="dim"):
        st.moments_host(np.zeros((3, st.MAX_DIM + 1)))


# ---- eigh_host -----------------------------------------------------------------------------------------------------------------
CASES = sc.eigh_cases()


def test_recorded_bars_are_the_measured_ones():
    """The header of statistics_cases.py records eigh_host's worst ratio per measure on the committed case list; the bar is 4 x
    that, never under one unit.  Recomputed here: the record may not understate what the definition does."""
    worst = {k: 0.0 for k in sc.EIGH_RECORDED}
    for name, a, _ in CASES:
        e = sc.host_solutions()[name]
        for k, v in sc.eigh_measures(a, e.values, e.vectors).items():
            worst[k] = max(worst[k], float(v))
    print("eigh_host worst ratios:", {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= sc.EIGH_RECORDED[k] * 1.5 + 0.25, (k, v)          # another BLAS moves the reference a little, not the record
        assert sc.EIGH_BAR[k] == max(1.0, 4.0 * sc.EIGH_RECORDED[k])


@pytest.mark.parametrize("name,a,repeated", CASES, ids=[c[0] for c in CASES])
def test_eigh_host_on_the_case_list(name, a, repeated):
    e = sc.host_solutions()[name]
    d = a.shape[0]
    m = sc.eigh_measures(a, e.values, e.vectors)
    for k, bar in sc.EIGH_BAR.items():
        assert m[k] <= bar, (k, m[k], bar)
    assert e.converged and 1 <= e.sweeps <= 30
    assert (np.diff(e.values) <= 0).all()
    top = np.argmax(np.abs(e.vectors), axis=1)
    assert (e.vectors[np.arange(d), top] > 0).all()
    if repeated:
        ref = np.linalg.eigh(a)[1].T[::-1]
        for lo, hi in repeated:
            assert np.abs(sc.projector(e.vectors, lo, hi) - sc.projector(ref, lo, hi)).max() <= sc.projector_bar(d, 3.0, 1.0)


def test_eigh_host_trivial_inputs_and_limits():
    e = st.eigh_host(np.diag([1.0, 3.0, 3.0, 2.0]))
    assert e.sweeps == 1 and e.rotations == 0 and e.converged
    np.testing.assert_array_equal(e.values, [3.0, 3.0, 2.0, 1.0])
    np.testing.assert_array_equal(e.vectors, np.eye(4)[[1, 2, 3, 0]])                  # ties by the original index
    e = st.eigh_host(np.array([[2.0, -1.0], [-1.0, 2.0]]))
    np.testing.assert_allclose(e.values, [3.0, 1.0], rtol=0, atol=8 * sc.U)
    assert e.vectors[0, 0] > 0 and e.vectors[0, 1] < 0                                 # the first of two equal magnitudes is made positive
    one = st.eigh_host(CASES[0][1], max_sweeps=1)
    assert not one.converged and one.sweeps == 1 and one.rotations > 0
    junk = np.triu(CASES[0][1]) + np.tril(np.full((16, 16), 9.0), -1)                  # only the upper triangle is read
    np.testing.assert_array_equal(st.eigh_host(junk).values, sc.host_solutions()["full_n50_d16"].values)
    bad = CASES[0][1].copy()
    bad[1, 2] = np.nan
    assert not st.eigh_host(bad).converged and st.eigh_host(bad).rotations == 0
    for kw in (dict(max_sweeps=0), dict(max_sweeps=st.MAX_SWEEPS + 1), dict(max_sweeps=True)):
        with pytest.raises(ValueError, match="max_sweeps"):
            st.eigh_host(np.eye(2), **kw)
    with pytest.raises(ValueError, match="square"):
        st.eigh_host(np.zeros((2, 3)))


# ---- pca_host against scikit-learn ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,k,whiten", [(200, 16, None, False), (300, 33, 5, True), (400, 64, 8, False)])
def test_pca_host_against_sklearn(n, dim, k, whiten):
    from sklearn.decomposition import PCA as SkPCA
    x = sc.gaussian_rows(n, dim, 100 + dim, offset=1.5, spread=1.6 ** -np.arange(dim))       # a separated spectrum
    ours = st.pca_host(x, k, whiten)
    kk = dim if k is None else k
    sk = SkPCA(n_components=kk, svd_solver="full", whiten=whiten).fit(x.astype(np.float64))
    top = sk.explained_variance_[0]
    bar = sc.EIGH_BAR["values"] * dim * sc.U * top
    assert (np.abs(ours.explained_variance - sk.explained_variance_) <= bar).all()
    assert (np.abs(ours.explained_variance_ratio - sk.explained_variance_ratio_) <= 2 * bar / sk.explained_variance_.sum() + 4 * sc.U).all()
    lead = min(kk, 8)                                       # where the gaps are far above the bar
    dots = np.abs((ours.components[:lead] * sk.components_[:lead]).sum(axis=1))
    assert (dots >= 1.0 - sc.EIGH_BAR["orthogonality"] * dim * sc.U).all(), dots
    z = (x.astype(np.float64) - ours.mean) @ ours.components.T
    if whiten:
        z = z * ours.scale[None, :]
    zs = sk.transform(x.astype(np.float64))
    sign = np.sign((ours.components * sk.components_).sum(axis=1))
    # a component with |dot| >= 1 - b is within sqrt(2 b) of sklearn's in length, so a projection within that times |x - mean|
    turn = np.sqrt(2.0 * sc.EIGH_BAR["orthogonality"] * dim * sc.U)
    reach = np.sqrt(((x.astype(np.float64) - ours.mean) ** 2).sum(axis=1)).max() * (ours.scale[:lead].max() if whiten else 1.0)
    assert np.abs(z[:, :lead] - (zs * sign[None, :])[:, :lead]).max() <= turn * reach


def test_pca_host_components_argument():
    x = sc.gaussian_rows(120, 12, 3)
    full = st.pca_host(x)
    assert full.components.shape == (12, 12) and abs(full.explained_variance_ratio.sum() - 1.0) <= 12 * sc.U * 4
    share = st.pca_host(x, 0.8)
    k = share.components.shape[0]
    assert full.explained_variance_ratio[:k].sum() >= 0.8 > full.explained_variance_ratio[:k - 1].sum()
    for bad in (0, 13, 0.0, 1.0, 1.5, True, "3"):
        with pytest.raises(ValueError, match="components"):
            st.pca_host(x, bad)


# ---- frechet_distance_host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(64, 16), (200, 16), (256, 64), (1000, 64)])
def test_frechet_host_against_the_textbook_route(n, d):
    """tr Sa + tr Sb - 2 tr sqrtm(Sa Sb) on full-rank cases (n >= 4 d): scipy's sqrtm is unreliable on singular products."""
    import scipy.linalg
    x, y = sc.gaussian_rows(n, d, 10 + d), sc.gaussian_rows(n + 7, d, 20 + d, offset=0.1)
    ours = st.frechet_distance_host(x, y)
    ma, mb = st.moments_host(x), st.moments_host(y)
    text = np.trace(ma.cov) + np.trace(mb.cov) - 2.0 * np.trace(scipy.linalg.sqrtm(ma.cov @ mb.cov)).real
    rel = abs(text - ours.trace_term) / (np.trace(ma.cov) + np.trace(mb.cov))
    print("frechet host vs sqrtm (%d, %d): relative difference %.3e" % (n, d, rel))
    assert rel <= sc.FRECHET_BAR_REL
    diff = ma.mean - mb.mean
    assert ours.mean_term == float(diff @ diff) and ours.value == ours.mean_term + ours.trace_term
    jac = st.frechet_distance_host(x, y, "jacobi") if d == 16 else ours
    assert abs(jac.value - ours.value) <= sc.FRECHET_BAR_REL * (np.trace(ma.cov) + np.trace(mb.cov))


def test_frechet_host_closed_forms():
    x = sc.gaussian_rows(80, 16, 1)
    x = (np.round(x * 256.0) / 256.0).astype(np.float32)
    ma = st.moments_host(x)
    tr = 2 * np.trace(ma.cov)
    same = st.frechet_distance_host(x, x)
    # identical sets: lambda_i = lambda_i(Sa)^2 up to the eigen bar e of the inner matrix; each term of the sum within sqrt of it
    e = sc.EIGH_BAR["values"] * 16 * sc.U * np.linalg.eigvalsh(ma.cov).max() ** 2
    assert same.mean_term == 0.0 and abs(same.value) <= 2 * 16 * np.sqrt(e) + 4 * 16 * sc.U * tr
    t = (np.arange(16, dtype=np.float32) % 3 - 1.0) * np.float32(0.75)
    moved = st.frechet_distance_host(x, x + t)                                        # exact in fp32: both on the 2^-8 grid
    assert abs(moved.mean_term - float(t.astype(np.float64) @ t)) <= 84 * 2 * sc.U * 16 * np.abs(x).max() * np.abs(t).max()
    assert abs(moved.trace_term) <= 2 * 16 * np.sqrt(e) + 4 * 16 * sc.U * tr + 2 * np.trace(sc.moments_bound(x, 1))
    a, b = np.array([4.0, 1.0, 0.25, 9.0, 0.0]), np.array([1.0, 1.0, 4.0, 0.0, 2.25])
    fd = st.frechet_from_moments_host(st.HostMoments(np.zeros(5), np.diag(a), 10), st.HostMoments(np.ones(5), np.diag(b), 10))
    assert abs(fd.trace_term - ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()) <= 16 * sc.U * (a.sum() + b.sum()) and fd.mean_term == 5.0
    with pytest.raises(ValueError, match="dims"):
        st.frechet_distance_host(x, x[:, :5])


# ---- the C ABI: host-only paths ------------------------------------------------------------------------------------------------
NAMES = ("acx_moments_workspace_bytes", "acx_moments", "acx_gram_f64", "acx_eigh_workspace_bytes", "acx_eigh", "acx_pca_transform",
         "acx_pca_inverse")


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    lib = _ffi.lib()
    for name in NAMES:
        assert re.search(r"ACX_API int %s\(" % name, header), name
        assert name in _ffi.SIGNATURES and _ffi.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(lib, name)
    for name, value in (("ACX_STATS_MAX_DIM", _ffi.STATS_MAX_DIM), ("ACX_EIGH_MAX_SWEEPS", _ffi.EIGH_MAX_SWEEPS),
                        ("ACX_STATS_NONFINITE", _ffi.STATS_NONFINITE), ("ACX_STATS_NOT_CONVERGED", _ffi.STATS_NOT_CONVERGED),
                        ("ACX_STATS_DEGENERATE", _ffi.STATS_DEGENERATE)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert ctypes.sizeof(_ffi.AcxEighState) == 16
    assert [len(_ffi.SIGNATURES[k][1]) for k in NAMES] == [3, 12, 10, 2, 12, 12, 12]


def test_workspace_queries_follow_the_slicing(monkeypatch):
    refresh = _ffi.lib().acx_tuning_refresh
    monkeypatch.delenv("ACX_MOMENTS_SLICE_ROWS", raising=False)
    refresh()
    try:
        tile = 64 * 64 * 8
        assert _ffi.moments_workspace_bytes(1000, 50) == 512 + tile                           # one slice, one tile pair
        assert _ffi.moments_workspace_bytes(20371, 768) == 16 * 768 * 8 + 16 * 78 * tile      # 16 slices of 1276 rows
        monkeypatch.setenv("ACX_MOMENTS_SLICE_ROWS", "16")
        refresh()
        assert _ffi.moments_workspace_bytes(257, 50) == 17 * 50 * 8 + 112 + 17 * tile          # 17 slices; 6800 -> 6912 aligned
        monkeypatch.setenv("ACX_MOMENTS_SLICE_ROWS", "7")                                     # out of range: ignored
        refresh()
        assert _ffi.moments_workspace_bytes(1000, 50) == 512 + tile
    finally:
        monkeypatch.delenv("ACX_MOMENTS_SLICE_ROWS", raising=False)
        refresh()
    assert _ffi.eigh_workspace_bytes(1) == 4 * 32 * 32 * 8 + 3 * 256
    assert _ffi.eigh_workspace_bytes(1024) == 4 * 1024 * 1024 * 8 + 3 * 256
    for args in ((0, 8), ((1 << 30) + 1, 8), (8, 0), (8, _ffi.STATS_MAX_DIM + 1)):
        with pytest.raises(_ffi.AcxError):
            _ffi.moments_workspace_bytes(*args)
    for dim in (0, _ffi.STATS_MAX_DIM + 1):
        with pytest.raises(_ffi.AcxError):
            _ffi.eigh_workspace_bytes(dim)


P = lambda v: None if v is None else ctypes.c_void_p(v)


def _moments_rc(x=64, ld=8, n=4, dim=8, ddof=1, mean=64, cov=64, ld_c=8, st_=64, ws=256, ws_bytes=1 << 30):
    return _ffi.lib().acx_moments(P(x), ld, n, dim, ddof, P(mean), P(cov), ld_c, P(st_), P(ws), ws_bytes, None)


def _gram_rc(a=64, ld_a=8, b=64, ld_b=8, rows=4, m=8, n=8, out=64, ld_o=8):
    return _ffi.lib().acx_gram_f64(P(a), ld_a, P(b), ld_b, rows, m, n, P(out), ld_o, None)


def _eigh_rc(a=64, ld_a=8, dim=8, sweeps=4, values=64, vectors=64, ld_v=8, state=64, st_=64, ws=256, ws_bytes=1 << 30):
    return _ffi.lib().acx_eigh(P(a), ld_a, dim, sweeps, P(values), P(vectors), ld_v, P(state), P(st_), P(ws), ws_bytes, None)


def _transform_rc(x=64, ld_x=8, n=4, dim=8, mean=64, w=64, ld_w=8, k=2, scale=None, out=64, ld_o=2):
    return _ffi.lib().acx_pca_transform(P(x), ld_x, n, dim, P(mean), P(w), ld_w, k, P(scale), P(out), ld_o, None)


def _inverse_rc(z=64, ld_z=2, n=4, k=2, scale=None, w=64, ld_w=8, dim=8, mean=64, out=64, ld_o=8):
    return _ffi.lib().acx_pca_inverse(P(z), ld_z, n, k, P(scale), P(w), ld_w, dim, P(mean), P(out), ld_o, None)


def test_argument_errors_return_before_any_launch():
    """Made-up (never dereferenced) pointers: every argument error of the header's list is negative without a device."""
    lib = _ffi.lib()
    for kw in (dict(x=None), dict(mean=None), dict(cov=None), dict(st_=None), dict(ws=None), dict(n=0), dict(dim=0),
               dict(dim=_ffi.STATS_MAX_DIM + 1), dict(ddof=2), dict(ddof=-1), dict(ld=7), dict(ld_c=7), dict(x=66), dict(mean=68),
               dict(cov=68)):
        assert _moments_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert _moments_rc(n=(1 << 30) + 1) == -6
    assert _moments_rc(ws_bytes=0) == -5 and _moments_rc(ws=264) == -5
    assert b"ddof = 2" in (_moments_rc(ddof=2), lib.acx_last_error())[1]
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(rows=0), dict(m=0), dict(n=0), dict(m=_ffi.STATS_MAX_DIM + 1),
               dict(n=_ffi.STATS_MAX_DIM + 1), dict(ld_a=7), dict(ld_b=7), dict(ld_o=7), dict(a=68), dict(out=68)):
        assert _gram_rc(**kw) == -1, kw
    assert _gram_rc(rows=(1 << 30) + 1) == -6
    for kw in (dict(a=None), dict(values=None), dict(vectors=None), dict(state=None), dict(st_=None), dict(ws=None), dict(dim=0),
               dict(dim=_ffi.STATS_MAX_DIM + 1), dict(sweeps=0), dict(sweeps=_ffi.EIGH_MAX_SWEEPS + 1), dict(ld_a=7), dict(ld_v=7),
               dict(a=68), dict(state=68)):
        assert _eigh_rc(**kw) == -1, kw
        assert lib.acx_last_error()
    assert _eigh_rc(ws_bytes=0) == -5 and _eigh_rc(ws=264) == -5
    assert b"max_sweeps = 0" in (_eigh_rc(sweeps=0), lib.acx_last_error())[1]
    for kw in (dict(x=None), dict(mean=None), dict(w=None), dict(out=None), dict(n=0), dict(dim=0), dict(k=0), dict(k=9), dict(ld_x=7),
               dict(ld_w=7), dict(ld_o=1), dict(x=66), dict(scale=66), dict(dim=_ffi.STATS_MAX_DIM + 1, ld_x=2000, ld_w=2000)):
        assert _transform_rc(**kw) == -1, kw
    assert _transform_rc(n=(1 << 30) + 1) == -6
    for kw in (dict(z=None), dict(w=None), dict(mean=None), dict(out=None), dict(n=0), dict(k=0), dict(k=9, ld_z=9), dict(ld_z=1),
               dict(ld_w=7), dict(ld_o=7), dict(z=66), dict(scale=66)):
        assert _inverse_rc(**kw) == -1, kw
    assert _inverse_rc(n=(1 << 30) + 1) == -6


# ---- the Python API: errors raised before any device call ----------------------------------------------------------------------
def test_python_value_errors_need_no_device():
    e = np.zeros((5, 8), np.float32)
    with pytest.raises(ValueError, match="not cpu"):
        st.moments(e, device="cpu")
    with pytest.raises(ValueError, match="ddof"):
        st.moments(e, ddof=3)
    with pytest.raises(ValueError, match="2-D"):
        st.PCA.fit(np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="components"):
        st.PCA.fit(e, 9)
    with pytest.raises(ValueError, match="max_sweeps"):
        st.eigh(np.eye(3), max_sweeps=0)
    with pytest.raises(ValueError, match="Moments or a PCA"):
        st.mahalanobis(e, None)
    assert st._count_for_share([4.0, 3.0, 2.0, 1.0], 0.7) == 2 and st._count_for_share([4.0, 3.0, 2.0, 1.0], 0.71) == 3
    assert st._count_for_share([0.0, 0.0], 0.5) == 1
