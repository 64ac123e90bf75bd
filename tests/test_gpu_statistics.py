"""GPU: embedding statistics (pytorch/statistics.py; acx_moments, acx_gram_f64, acx_eigh, acx_pca_* in include/acx.h;
csrc/moments.hip, csrc/eigh.hip) against the numpy float64 host definitions: (1) the operand and result maps of the float64
matrix instruction, (2) exact and rounded moments, (3) the eigensolver on the shared case list under the recorded bars,
(4) the PCA projections, (5) the Frechet distance under a bar derived from the eigen bar, (6) the model and index hooks.
Shapes sit at the tile and tail boundaries (16-wide instruction tiles, 64 x 64 workgroup tiles, slices of 16 rows), not at
workload size."""
import numpy as np
import pytest
import torch

import statistics_cases as sc
from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd._ffi import vp
from audioset_convnext_inf_amd.pytorch import statistics as st
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.retrieval import EmbeddingIndex

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


@pytest.fixture
def slices_of_16(monkeypatch):
    """acx_moments cut into slices of 16 rows: 257 rows make 17 slices with a short last one."""
    refresh = _ffi.lib().acx_tuning_refresh
    monkeypatch.setenv("ACX_MOMENTS_SLICE_ROWS", "16")
    refresh()
    yield
    monkeypatch.delenv("ACX_MOMENTS_SLICE_ROWS", raising=False)
    refresh()


# ---- (1) the operand maps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,m,n", [(16, 16, 16), (64, 64, 64), (70, 70, 33), (130, 130, 97), (5, 5, 3)])
def test_gram_identity_against_an_asymmetric_integer_matrix(rows, m, n):
    """A = identity rows (zero padded) against an asymmetric integer B picks out B's rows one by one, and with the roles swapped
    its transpose: any slip in the A / B operand maps or in the float64 result map (which is NOT the f32 one) moves entries."""
    rng = np.random.default_rng(rows * 131 + n)
    b = rng.integers(-9, 10, (rows, n)).astype(np.float64) + 17.0 * np.arange(rows)[:, None] + np.arange(n)[None, :] / 4.0
    eye = np.zeros((rows, m))
    eye[np.arange(min(rows, m)), np.arange(min(rows, m))] = 1.0
    np.testing.assert_array_equal(st.gram(f64(eye), f64(b)).cpu().numpy(), eye.T @ b)
    np.testing.assert_array_equal(st.gram(f64(b), f64(eye)).cpu().numpy(), b.T @ eye)
    a = rng.integers(-9, 10, (rows, m)).astype(np.float64)
    wide = f64(np.concatenate([a, a], axis=1))[:, 1:1 + m]                      # ld > m, a shifted base
    np.testing.assert_array_equal(st.gram(wide, f64(b)).cpu().numpy(), wide.cpu().numpy().T @ b)


# ---- (2) moments ---------------------------------------------------------------------------------------------------------------
EXACT_DIMS = (1, 3, 15, 16, 17, 33, 50, 768)
EXACT_ROWS = (1, 2, 3, 4, 5, 63, 64, 65, 257)


@pytest.mark.parametrize("dim", EXACT_DIMS)
def test_exact_moments_equal_the_host(dim, slices_of_16):
    """Integer rows whose column sums are multiples of n: the mean, the centred values, every product and every sum are exact,
    so mean and cov EQUAL the host definition, in slices of 16 rows, with ld_x > dim, for both ddof; cov is exactly symmetric
    and a second run gives the same bits."""
    for n in EXACT_ROWS:
        x = sc.exact_rows(n, dim, 1000 * dim + n)
        wide = f32(np.concatenate([x, x[:, :1] + 1.0, x], axis=1))[:, :dim]      # ld_x = 2 dim + 1
        for ddof in (0, 1):
            want = st.moments_host(x, ddof)
            got = st.moments(wide, ddof)
            status = int(got.status.cpu()[0])
            assert status == (_ffi.STATS_DEGENERATE if n - ddof == 0 else 0), (n, ddof, status)
            mean, cov = got.mean.cpu().numpy(), got.cov.cpu().numpy()
            np.testing.assert_array_equal(mean, want.mean, err_msg="n %d ddof %d" % (n, ddof))
            np.testing.assert_array_equal(cov, want.cov, err_msg="n %d ddof %d" % (n, ddof))
            np.testing.assert_array_equal(cov, cov.T)
        again = st.moments(wide, 1)
        assert torch.equal(again.cov, got.cov) and torch.equal(again.mean, got.mean)


@pytest.mark.parametrize("n,dim,forced", [(1000, 768, False), (257, 50, True), (257, 50, False)])
def test_rounded_moments_within_the_bound(n, dim, forced, monkeypatch):
    """Gaussian rows with mean 100 and std 1 -- the cancellation case of a one-pass formula -- within (n + 4) 2^-53 |Xc|^T |Xc| /
    (n - ddof) elementwise of the host definition; the mean within 2 n 2^-53 mean |x| (either side's sum is off by at most
    (n - 1) 2^-53 sum |x| in any order, and rounds once more in the division)."""
    refresh = _ffi.lib().acx_tuning_refresh
    if forced:
        monkeypatch.setenv("ACX_MOMENTS_SLICE_ROWS", "16")
    refresh()
    try:
        x = (np.random.default_rng(n + dim).standard_normal((n, dim)) + 100.0).astype(np.float32)
        want = st.moments_host(x, 1)
        got = st.moments(f32(x), 1).check()
        cov, mean = got.cov.cpu().numpy(), got.mean.cpu().numpy()
        excess = (np.abs(cov - want.cov) / sc.moments_bound(x, 1)).max()
        print("moments (%d, %d) forced=%s: max |cov - host| / bound = %.3f" % (n, dim, forced, excess))
        assert excess <= 1.0
        assert (np.abs(mean - want.mean) <= 2 * n * sc.U * np.abs(x.astype(np.float64)).mean(axis=0)).all()
        np.testing.assert_array_equal(cov, cov.T)
    finally:
        monkeypatch.delenv("ACX_MOMENTS_SLICE_ROWS", raising=False)
        refresh()


def test_moments_status_bits():
    x = sc.gaussian_rows(70, 33, 3)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[41, 17] = bad
        got = st.moments(f32(y))
        assert int(got.status.cpu()[0]) == _ffi.STATS_NONFINITE
        cov = got.cov.cpu().numpy()
        assert not np.isfinite(cov[17, 17]) and np.isfinite(cov[:17, :17]).all()    # written, and only column 17 is touched
        with pytest.raises(ValueError, match="NaN or infinite"):
            got.check()
    one = st.moments(f32(x[:1]), 1)
    assert int(one.status.cpu()[0]) == _ffi.STATS_DEGENERATE and not one.cov.any()
    np.testing.assert_array_equal(one.mean.cpu().numpy(), x[0].astype(np.float64))
    with pytest.raises(ValueError, match="too few rows"):
        one.check()
    assert int(st.moments(f32(x[:1]), 0).status.cpu()[0]) == 0


def test_merge_pools_two_sets():
    x = sc.gaussian_rows(300, 50, 8, offset=3.0)
    whole = st.moments_host(x, 1)
    merged = st.moments(f32(x[:113])).merge(st.moments(f32(x[113:]))).check()
    assert merged.n == 300
    assert (np.abs(merged.cov.cpu().numpy() - whole.cov) <= 4 * sc.moments_bound(x, 1)).all()
    np.testing.assert_allclose(merged.mean.cpu().numpy(), whole.mean, rtol=0, atol=304 * sc.U * np.abs(x).max())


# ---- (3) the eigensolver -------------------------------------------------------------------------------------------------------
CASES = sc.eigh_cases()


@pytest.mark.parametrize("name,a,repeated", CASES, ids=[c[0] for c in CASES])
def test_eigh_on_the_case_list(name, a, repeated):
    """Within the recorded bars against numpy.linalg.eigh, and within +-2 sweeps of the host definition: a threshold tie may move
    a rotation across a sweep boundary, another algorithm would not land there."""
    host = sc.host_solutions()[name]
    values, vectors, state = st.eigh(f64(a))
    state.check()
    w, v = values.cpu().numpy(), vectors.cpu().numpy()
    m = sc.eigh_measures(a, w, v)
    sweeps = int(state.sweeps.cpu())
    print("eigh %s: %s sweeps %d (host %d) rotations %d (host %d)" % (name, {k: round(float(x), 3) for k, x in m.items()}, sweeps,
                                                                     host.sweeps, int(state.rotations.cpu()), host.rotations))
    for k, bar in sc.EIGH_BAR.items():
        assert m[k] <= bar, (k, m[k], bar)
    assert abs(sweeps - host.sweeps) <= 2 and bool(state.converged.cpu())
    assert (np.diff(w) <= 0).all()
    top = np.argmax(np.abs(v), axis=1)
    assert (v[np.arange(len(w)), top] > 0).all()
    if repeated:
        ref = np.linalg.eigh(a)[1].T[::-1]
        for lo, hi in repeated:
            assert np.abs(sc.projector(v, lo, hi) - sc.projector(ref, lo, hi)).max() <= sc.projector_bar(len(w), 3.0, 1.0)


def test_eigh_one_sweep_does_not_converge():
    a = CASES[0][1]
    values, vectors, state = st.eigh(f64(a), max_sweeps=1)
    assert int(state.status.cpu()[0]) == _ffi.STATS_NOT_CONVERGED and int(state.sweeps.cpu()) == 1 and not bool(state.converged.cpu())
    with pytest.raises(RuntimeError, match="max_sweeps"):
        state.check()
    d = np.diag([3.0, 1.0, 2.0])
    values, vectors, state = st.eigh(f64(d), max_sweeps=1)
    assert int(state.status.cpu()[0]) == 0 and int(state.rotations.cpu()) == 0
    np.testing.assert_array_equal(values.cpu().numpy(), [3.0, 2.0, 1.0])
    np.testing.assert_array_equal(vectors.cpu().numpy(), np.eye(3)[[0, 2, 1]])


def test_eigh_nonfinite_input_is_reported():
    a = CASES[0][1].copy()
    a[2, 5] = np.nan
    _, _, state = st.eigh(f64(a))
    assert int(state.status.cpu()[0]) & _ffi.STATS_NONFINITE and int(state.rotations.cpu()) == 0


def test_eigh_reads_the_upper_triangle_and_a_wide_matrix():
    a = CASES[-1][1]
    junk = np.triu(a) + np.tril(np.full_like(a, 99.0), -1)
    wide = f64(np.concatenate([junk, junk], axis=1))[:, :17]
    got = st.eigh(wide)
    want = st.eigh(f64(a))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_eigh_replays_from_a_graph_with_the_eager_bits():
    a = f64(CASES[-1][1])                                                        # d = 17: odd, 17 rounds a sweep
    dim = a.shape[0]
    out = [torch.empty(dim, dtype=torch.float64, device=DEV), torch.empty((dim, dim), dtype=torch.float64, device=DEV),
           torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)]
    ws_bytes = _ffi.eigh_workspace_bytes(dim)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def run():
        _ffi.eigh(vp(a), a.stride(0), dim, 12, vp(out[0]), vp(out[1]), dim, vp(out[2]), vp(out[3]), (vp(ws), ws_bytes),
                  _ffi.stream_ptr(a.device))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.clone() for t in out]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for e, t in zip(eager, out):
        assert torch.equal(e, t)
    assert int(out[3].cpu()[0]) == 0 and int(out[2].cpu()[0]) >= 2


# ---- (4) the PCA projections ---------------------------------------------------------------------------------------------------
def host_transform(x, mean, w, scale):
    xc = (x.astype(np.float32) - mean.astype(np.float32)[None, :]).astype(np.float64)
    z = xc @ w.astype(np.float64).T
    mag = np.abs(xc) @ np.abs(w.astype(np.float64)).T
    if scale is not None:
        z, mag = z * scale.astype(np.float64)[None, :], mag * np.abs(scale.astype(np.float64))[None, :]
    return z, mag


def dev_transform(x, mean, w, scale):
    n, dim = x.shape
    k = w.shape[0]
    out = torch.full((n, k + 3), -77.0, dtype=torch.float32, device=DEV)
    xs, ms, wsd = f32(x), f32(mean), f32(w)
    ss = None if scale is None else f32(scale)
    _ffi.pca_transform(vp(xs), xs.stride(0), n, dim, vp(ms), vp(wsd), wsd.stride(0), k, vp(ss), vp(out), out.stride(0),
                       _ffi.stream_ptr(out.device))
    assert (out[:, k:] == -77.0).all()
    return out[:, :k].cpu().numpy()


def dev_inverse(z, scale, w, mean):
    n, k = z.shape
    dim = w.shape[1]
    out = torch.full((n, dim + 3), -77.0, dtype=torch.float32, device=DEV)
    zs, ms, wsd = f32(z), f32(mean), f32(w)
    ss = None if scale is None else f32(scale)
    _ffi.pca_inverse(vp(zs), zs.stride(0), n, k, vp(ss), vp(wsd), wsd.stride(0), dim, vp(ms), vp(out), out.stride(0),
                     _ffi.stream_ptr(out.device))
    assert (out[:, dim:] == -77.0).all()
    return out[:, :dim].cpu().numpy()


@pytest.mark.parametrize("dim,k", [(50, 1), (50, 2), (50, 50), (768, 1), (768, 2), (768, 50), (768, 128)])
def test_pca_projections(dim, k):
    rng = np.random.default_rng(dim + k)
    for n in (1, 33, 129):
        # integers: exact in fp32 in any order
        x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
        mean = rng.integers(-3, 4, dim).astype(np.float32)
        w = rng.integers(-2, 3, (k, dim)).astype(np.float32)
        scale = (2.0 ** rng.integers(-2, 3, k)).astype(np.float32)
        for s in (None, scale):
            want, _ = host_transform(x, mean, w, s)
            np.testing.assert_array_equal(dev_transform(x, mean, w, s).astype(np.float64), want)
        z = rng.integers(-4, 5, (n, k)).astype(np.float32)
        for s in (None, scale):
            zz = z.astype(np.float64) * (1.0 if s is None else s.astype(np.float64)[None, :])
            np.testing.assert_array_equal(dev_inverse(z, s, w, mean).astype(np.float64), zz @ w.astype(np.float64) + mean[None, :])
        # Gaussian rows: (dim + 2) 2^-24 sum |a||b|, one more rounding for the scale
        x = rng.standard_normal((n, dim)).astype(np.float32)
        mean = rng.standard_normal(dim).astype(np.float32)
        w = (rng.standard_normal((k, dim)) / np.sqrt(dim)).astype(np.float32)
        scale = rng.uniform(0.5, 2.0, k).astype(np.float32)
        want, mag = host_transform(x, mean, w, scale)
        got = dev_transform(x, mean, w, scale).astype(np.float64)
        assert (np.abs(got - want) <= (dim + 2) * U24 * mag + U24 * np.abs(want)).all()
        z = rng.standard_normal((n, k)).astype(np.float32)
        zz = (z * scale[None, :]).astype(np.float64)                             # the device rounds the product to fp32 as well
        want = zz @ w.astype(np.float64) + mean[None, :]
        mag = np.abs(zz) @ np.abs(w.astype(np.float64)) + np.abs(mean)[None, :]
        got = dev_inverse(z, scale, w, mean).astype(np.float64)
        assert (np.abs(got - want) <= (k + 3) * U24 * mag).all()


def test_pca_fit_whitens_and_inverts():
    """A whitened fit of all components: the output's sample covariance is the identity.  The bar has two parts.  The eigen part:
    W S W^T = diag(lambda) + E with |E| <= (residual + orthogonality bar) d 2^-53 lambda_0, divided by the smallest lambda by the
    scaling.  The fp32 part: an entry of the output is off by at most (dim + 3) 2^-24 of M = scale sum_j |x_j - mean_j| |W_cj|
    (the rounding of the centring, of W, mean and scale, and of the dim sums), so a product of two by twice that, plus the square."""
    n, dim = 600, 50
    x = sc.gaussian_rows(n, dim, 21, offset=2.0)
    pca = st.PCA.fit(f32(x), whiten=True).check()
    host = st.pca_host(x, whiten=True, solver="lapack")
    var = pca.explained_variance_.cpu().numpy()
    bar = sc.EIGH_BAR["values"] * dim * sc.U * host.explained_variance[0]
    assert (np.abs(var - host.explained_variance) <= bar).all()
    assert (np.abs(pca.explained_variance_ratio_.cpu().numpy() - host.explained_variance_ratio)
            <= 2 * bar / host.explained_variance.sum()).all()
    z = pca.transform(f32(x))
    cov = st.moments_host(z.cpu().numpy(), 1).cov
    _, mag = host_transform(x, host.mean, host.components, host.scale)
    M = mag.T @ mag / (n - 1)
    r = (dim + 3) * U24
    eigen = (sc.EIGH_BAR["residual"] + sc.EIGH_BAR["orthogonality"]) * dim * sc.U * host.explained_variance[0] / host.explained_variance.min()
    excess = (np.abs(cov - np.eye(dim)) / ((2 * r + r * r) * M + eigen)).max()
    print("whitened covariance: max |cov - I| = %.3e, / bar = %.3f" % (np.abs(cov - np.eye(dim)).max(), excess))
    assert excess <= 1.0
    back = pca.inverse_transform(z).cpu().numpy()
    # x -> z -> x: each direction within (dim + 3) 2^-24 of its magnitudes, |W| rows of unit length: sum_j |.| <= sqrt(dim) |.|_2
    assert np.abs(back - x).max() <= 2 * r * dim ** 0.5 * np.abs(x.astype(np.float64) - host.mean).sum(axis=1).max()
    d = st.mahalanobis(f32(x), pca)
    assert torch.equal(d, torch.sqrt((z * z).sum(dim=1)))
    assert torch.equal(st.mahalanobis(f32(x), st.moments(f32(x))), d)


def test_pca_components_by_count_and_share(tmp_path):
    x = sc.gaussian_rows(400, 33, 22)
    full = st.PCA.fit(f32(x))
    assert full.components_.shape == (33, 33)
    part = st.PCA.fit(f32(x), 7)
    assert torch.equal(part.components_, full.components_[:7]) and torch.equal(part.explained_variance_, full.explained_variance_[:7])
    share = st.PCA.fit(f32(x), 0.9)
    ratio = full.explained_variance_ratio_.cpu().numpy()
    k = share.n_components_
    assert ratio[:k].sum() >= 0.9 > ratio[:k - 1].sum() and k == st.pca_host(x, 0.9).components.shape[0]
    path = str(tmp_path / "pca.npz")
    st.PCA.fit(f32(x), 5, whiten=True).save(path)
    a, b = st.PCA.fit(f32(x), 5, whiten=True), st.PCA.load(path)
    assert torch.equal(a.transform(f32(x)), b.transform(f32(x)))


# ---- (5) the Frechet distance --------------------------------------------------------------------------------------------------
def frechet_bar(x, y):
    """2 sum_i (sqrt(max(l_i, 0) + e) - sqrt(max(l_i - e, 0))) with e the eigen bar of the inner matrix Sa^1/2 Sb Sa^1/2, plus the
    moments bound on the two traces and on the mean term (2 |mu_a - mu_b| times the means' own bound, and the sum's rounding)."""
    ma, mb = st.moments_host(x), st.moments_host(y)
    d = x.shape[1]
    wa, va = np.linalg.eigh(ma.cov)
    h = (va * np.sqrt(np.maximum(wa, 0))[None, :]) @ va.T
    lam = np.linalg.eigvalsh(h @ mb.cov @ h)
    e = sc.EIGH_BAR["values"] * d * sc.U * max(np.abs(lam).max(), np.finfo(float).tiny)
    eig = 2 * (np.sqrt(np.maximum(lam, 0) + e) - np.sqrt(np.maximum(lam - e, 0))).sum()
    traces = np.trace(sc.moments_bound(x, 1)) + np.trace(sc.moments_bound(y, 1))
    diff = np.abs(ma.mean - mb.mean)
    slack = 2 * sc.U * (x.shape[0] * np.abs(x).mean(axis=0) + y.shape[0] * np.abs(y).mean(axis=0))      # of mu_a - mu_b, both sides
    means = (2 * diff * slack + slack * slack).sum() + (d + 2) * sc.U * (diff @ diff)
    return eig + traces + means


FRECHET = [("d16", 64, 80, 16, 0.1), ("d64", 256, 300, 64, 0.1), ("rank_deficient", 20, 24, 64, 0.1), ("identical", 100, 100, 16, None),
           ("shifted", 100, 100, 16, "shift")]


@pytest.mark.parametrize("name,n,m,d,kind", FRECHET, ids=[c[0] for c in FRECHET])
def test_frechet_distance_against_the_host(name, n, m, d, kind):
    x = sc.gaussian_rows(n, d, 30 + d)
    if kind is None:
        y = x.copy()
    elif kind == "shift":
        x = (np.round(x * 256.0) / 256.0).astype(np.float32)                     # multiples of 2^-8: the shift below is exact in fp32
        y = x + (np.arange(d, dtype=np.float32) % 3 - 1.0) * np.float32(0.75)
    else:
        y = sc.gaussian_rows(m, d, 40 + d, offset=kind, spread=np.linspace(0.3, 1.1, d))
    want = st.frechet_distance_host(x, y)
    got = st.frechet_distance(f32(x), f32(y)).check()
    bar = frechet_bar(x, y)
    value, mean_term, trace_term = (float(t.cpu()) for t in got)
    print("frechet %s: device %.12g host %.12g |diff| %.3e bar %.3e" % (name, value, want.value, abs(value - want.value), bar))
    assert abs(value - want.value) <= bar and abs(mean_term - want.mean_term) <= bar and abs(trace_term - want.trace_term) <= bar
    assert value == mean_term + trace_term and float(got) == value
    if kind is None:
        assert mean_term == 0.0 and abs(value) <= bar
    if kind == "shift":
        t = (y.astype(np.float64) - x.astype(np.float64)).mean(axis=0)
        assert abs(mean_term - t @ t) <= bar and abs(trace_term) <= bar


def test_frechet_distance_of_diagonal_covariances():
    a, b = np.array([4.0, 1.0, 0.25, 9.0, 0.0]), np.array([1.0, 1.0, 4.0, 0.0, 2.25])
    zero = torch.zeros(5, dtype=torch.float64, device=DEV)
    ma, mb = st.Moments(zero, f64(np.diag(a)), 10), st.Moments(zero + 1.0, f64(np.diag(b)), 10)
    got = st.frechet_distance_from_moments(ma, mb).check()
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    # diagonal input: no rotation, so only roundings remain -- lambda^1/4 twice, three products and a square root per term, each
    # sqrt(a b) <= (a + b) / 2, and the sums: under 16 roundings of (a + b) in all
    assert abs(float(got.trace_term.cpu()) - want) <= 16 * sc.U * (a.sum() + b.sum()) and float(got.mean_term.cpu()) == 5.0


# ---- (6) the hooks -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(synth_sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    return m.to("cuda").eval()


def test_statistics_through_the_model(model):
    """The hooks equal the module calls on forward_scene_embeddings' rows bit for bit.  Two sweeps only: the 768-d eigenproblem is
    not what this test is about (NOT_CONVERGED is expected and nothing calls check())."""
    wa, wb = synth.synth_waveforms(6, 32000, seed=61).cuda(), synth.synth_waveforms(5, 32000, seed=62).cuda()
    ea, eb = model.forward_scene_embeddings(wa), model.forward_scene_embeddings(wb)
    want = st.frechet_distance(ea, eb, max_sweeps=2)
    got = model.frechet_distance([w for w in wa], [w for w in wb], max_sweeps=2)
    for name in ("value", "mean_term", "trace_term"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert int(got.status.cpu()[0]) == _ffi.STATS_NOT_CONVERGED
    pca = model.fit_pca([w for w in wa], 3, max_sweeps=2)
    ref = st.PCA.fit(ea, 3, max_sweeps=2)
    assert pca.components_.shape == (3, 768)
    assert torch.equal(pca.components_, ref.components_) and torch.equal(pca.explained_variance_, ref.explained_variance_)
    assert torch.equal(model.fit_pca(ea, 3, max_sweeps=2).components_, ref.components_)


def test_index_moments_and_pca():
    x = sc.gaussian_rows(200, 40, 9)
    target = (np.random.default_rng(1).random((200, 3)) > 0.5)
    idx = EmbeddingIndex(f32(x), target=torch.from_numpy(target).to(DEV))
    mo = idx.moments()
    ref = st.moments(f32(x))
    assert torch.equal(mo.cov, ref.cov) and torch.equal(mo.mean, ref.mean)
    pca, small = idx.pca(8)
    assert len(small) == 200 and small.dim == 8 and small.metric == idx.metric
    assert torch.equal(small.embeddings, pca.transform(f32(x))) and torch.equal(small.target, idx.target)
    scores, indices = small.search(small.embeddings[:5], k=1)
    assert indices.reshape(-1).tolist() == [0, 1, 2, 3, 4]
