"""Shared cases and bars of the statistics tests (test_statistics_cpu.py, test_gpu_statistics.py).

The eigensolver bars.  Three measures of a solution (values w, vectors as rows V) of a symmetric A of d rows, each in units of
u = d 2^-53 (times max |w| for the first and the third):
    residual   max |A V^T - V^T diag(w)|
    orthogon.  max |V V^T - I|
    values     max |w - w_LAPACK|
RECORDED: statistics.eigh_host on eigh_cases() below gives, at worst over the cases,
    residual 0.53 u   orthogonality 4.12 u   values 0.82 u        (7 - 24 sweeps at d >= 16; 18 and 24 on the two d = 192 cases)
(values: 0.81 u on zero_diagonal_d17, whose threshold 2^-53 max |a_ii| is 0 -- only exactly zero pivots stop a rotation there, and
they do, after 11 sweeps: once |theta| overflows, t is 0 and the pivot is stored as 0; 0.68 u at worst over the other cases)
(numpy.linalg.eigh's own residual and orthogonality on the same cases: <= 0.56 u and <= 1.34 u).  The bar for the host definition
AND for the device is 4 x the recorded worst, never under 1 u: the factor covers another rotation order among tied pivots and
the device's own sqrt / division roundings, nothing else -- a different algorithm does not fit under it.

The Frechet bar.  frechet_distance_host against the textbook route tr Sa + tr Sb - 2 tr sqrtm(Sa Sb) (scipy.linalg.sqrtm) on the
full-rank cases: RECORDED worst difference 2.6e-12 relative to tr Sa + tr Sb; the bar is 10 x that, since the BLAS behind sqrtm
differs between machines."""
import functools

import numpy as np

U = 2.0 ** -53

EIGH_RECORDED = {"residual": 0.53, "orthogonality": 4.12, "values": 0.82}
EIGH_BAR = {k: max(1.0, 4.0 * v) for k, v in EIGH_RECORDED.items()}
FRECHET_RECORDED_REL = 2.6e-12
FRECHET_BAR_REL = 10.0 * FRECHET_RECORDED_REL


def gaussian_rows(n, d, seed, offset=0.0, spread=None):
    """n rows of d correlated Gaussian columns (float32): independent columns of decaying spread mixed by a random matrix."""
    rng = np.random.default_rng(seed)
    spread = np.linspace(1.0, 0.2, d) if spread is None else spread
    mix = rng.standard_normal((d, d)) / np.sqrt(d)
    return ((rng.standard_normal((n, d)) * spread[None, :]) @ mix + offset).astype(np.float32)


def _orthogonal(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q


def _cov(n, d, seed):
    x = gaussian_rows(n, d, seed).astype(np.float64)
    xc = x - x.mean(axis=0)
    c = xc.T @ xc / (n - 1)
    return np.triu(c) + np.triu(c, 1).T


def _spectrum(values, seed):
    q = _orthogonal(len(values), seed)
    a = (q * np.asarray(values, dtype=np.float64)[None, :]) @ q.T
    return np.triu(a) + np.triu(a, 1).T


def eigh_cases():
    """[(name, symmetric float64 matrix, repeated)]: repeated = the eigenvalue groups whose vectors are compared as projectors."""
    rng = np.random.default_rng(77)
    g = rng.standard_normal((17, 17))
    return [
        ("full_n50_d16", _cov(50, 16, 1), None),
        ("full_n400_d64", _cov(400, 64, 2), None),
        ("rankdef_n40_d64", _cov(40, 64, 3), None),
        ("rankdef_n100_d192", _cov(100, 192, 4), None),
        ("geometric_d192", _spectrum(0.85 ** np.arange(192), 5), None),
        ("repeated_d6", _spectrum([3.0, 3.0, 3.0, 1.0, 1.0, 0.0], 6), [(0, 3), (3, 5), (5, 6)]),
        ("one_by_one", np.array([[2.5]]), None),
        ("two_by_two", np.array([[1.0, 2.0], [2.0, -3.0]]), None),
        ("three_by_three", np.array([[4.0, 1.0, -2.0], [1.0, 2.0, 0.5], [-2.0, 0.5, 3.0]]), None),
        ("diagonal_d5", np.diag([5.0, -1.0, 3.0, 3.5, 0.0]), None),
        ("indefinite_d17", g + g.T, None),
        # next to the solver's 32 x 32 tiles: one tile less a row, one tile, one row into the second (31 padded rows), and one
        # row into the third
        ("full_n200_d31", _cov(200, 31, 8), None),
        ("full_n200_d32", _cov(200, 32, 9), None),
        ("full_n200_d33", _cov(200, 33, 10), None),
        ("full_n300_d65", _cov(300, 65, 11), None),
        # a zero diagonal: the convergence threshold 2^-53 max |a_ii| starts at 0
        ("zero_diagonal_d17", g + g.T - np.diag(np.diag(g + g.T)), None),
    ]


@functools.lru_cache(maxsize=None)
def host_solutions():
    """{name: statistics.eigh_host(matrix)} over eigh_cases(), computed once per process (the d = 192 cases take seconds)."""
    from audioset_convnext_inf_amd.pytorch import statistics
    return {name: statistics.eigh_host(a) for name, a, _ in eigh_cases()}


def eigh_measures(a, values, vectors):
    """(residual, orthogonality, values) in the units of the header, against numpy.linalg.eigh."""
    a = np.asarray(a, dtype=np.float64)
    d = a.shape[0]
    w = np.asarray(values, dtype=np.float64)
    vt = np.asarray(vectors, dtype=np.float64).T
    ref = np.linalg.eigvalsh(a)[::-1]
    top = max(np.abs(ref).max(), np.finfo(np.float64).tiny)
    unit = d * U
    resid = np.abs(a @ vt - vt * w[None, :]).max() / (unit * top)
    orth = np.abs(vt.T @ vt - np.eye(d)).max() / unit
    vals = np.abs(w - ref).max() / (unit * top)
    return {"residual": resid, "orthogonality": orth, "values": vals}


def projector(vectors, lo, hi):
    v = np.asarray(vectors, dtype=np.float64)[lo:hi]
    return v.T @ v


def projector_bar(d, top, gap):
    """max |P - P_ref| allowed for the projector onto an eigenspace separated by `gap` from the rest, values up to `top`: a vector
    is off its space by at most residual / gap (sin theta), twice that in the projector, plus the loss of orthogonality -- for
    the solution under test and for the LAPACK reference alike, hence the leading 2."""
    return 2.0 * (2.0 * EIGH_BAR["residual"] * top / gap + EIGH_BAR["orthogonality"]) * d * U


def exact_rows(n, d, seed):
    """Integer-valued float32 rows in [-8, 8] whose column sums are multiples of n: the mean, the centred values, every product
    and every sum of the moments are exact in float64 (and the mean is an integer)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.int64)
    for j in range(d):
        r = int(x[:, j].sum()) % n                           # lower r entries by 1 (or raise n - r by 1), staying inside [-8, 8]
        i = 0
        while r:
            if x[i % n, j] > -8:
                x[i % n, j] -= 1
                r -= 1
            i += 1
    assert (x.sum(axis=0) % n == 0).all() and x.min() >= -8 and x.max() <= 8
    return x.astype(np.float32)


def moments_bound(x, ddof):
    """(n + 4) 2^-53 |Xc|^T |Xc| / (n - ddof), elementwise: the rounding of centring, products and any order of summation."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    xc = np.abs(x - x.mean(axis=0))
    return (n + 4) * U * (xc.T @ xc) / (n - ddof)
