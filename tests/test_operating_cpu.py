"""CPU: per-class operating points on the host side -- operating_points_host (pytorch/metrics.py), the numpy float64 statement of
acx_operating_points, against sklearn.metrics.precision_recall_curve; its tie rule and degenerate classes; decode_events with one
threshold / low per class; the ctypes declarations of the new symbols and their argument checks.  No device needed."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import precision_recall_curve

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch.metrics import OperatingPoints, operating_points_host

N, C = 3000, 24


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(11)
    prior = np.concatenate([[0.01, 0.9], rs.uniform(0.01, 0.9, size=C - 2)])
    t = rs.uniform(size=(N, C)) < prior
    t[0], t[1] = True, False
    s = (1.0 / (1.0 + np.exp(-(rs.standard_normal((N, C)) * 1.5 + 1.5 * t)))).astype(np.float32)
    s[:, 5] = np.round(s[:, 5] * 20) / 20                           # a class full of ties
    t.setflags(write=False)
    s.setflags(write=False)
    return t, s


def pr_curve(t, s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return precision_recall_curve(t, s)


def counts_at(t, s, thr):
    """(TP, FP, FN, TN) of s >= thr, by numpy"""
    fire = s >= thr
    return [int((fire & t).sum()), int((fire & ~t).sum()), int((~fire & t).sum()), int((~fire & ~t).sum())]


def test_max_f1_against_sklearn(data):
    t, s = data
    op = operating_points_host(t, s, "f1")
    assert op.threshold.dtype == np.float32 and op.threshold.shape == (C,)
    assert op.counts.dtype == np.int64 and op.counts.shape == (C, 4)
    f = op.f(1.0)
    for c in range(C):
        p, r, th = pr_curve(t[:, c], s[:, c])
        with np.errstate(invalid="ignore", divide="ignore"):
            fs = np.where(p + r > 0, 2 * p * r / (p + r), 0.0)[:-1]
        assert abs(f[c] - fs.max()) <= 1e-12, (c, f[c], fs.max())
        # at the returned threshold sklearn's own precision and recall are those of the counts
        i = np.nonzero(th == op.threshold[c])[0]
        assert len(i) == 1, "the threshold is one of the scores"
        tp, fp, fn, tn = op.counts[c]
        assert abs(p[i[0]] - tp / (tp + fp)) <= 1e-15 and abs(r[i[0]] - tp / (tp + fn)) <= 1e-15
        assert op.counts[c].tolist() == counts_at(t[:, c], s[:, c], op.threshold[c])
    assert op.precision.dtype == np.float64 and np.allclose(op.precision, op.counts[:, 0] / (op.counts[:, 0] + op.counts[:, 1]))
    assert abs(op.macro()["f"] - f.mean()) <= 1e-15
    tp, fp, fn, tn = op.counts.sum(axis=0)
    assert abs(op.micro()["f"] - 2 * tp / (2 * tp + fn + fp)) <= 1e-15


@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_fbeta_against_sklearn(data, beta):
    t, s = data
    op = operating_points_host(t, s, ("fbeta", beta))
    f = op.f(beta)
    b2 = beta * beta
    for c in range(C):
        p, r, th = pr_curve(t[:, c], s[:, c])
        with np.errstate(invalid="ignore", divide="ignore"):
            fs = np.where(p + r > 0, (1 + b2) * p * r / (b2 * p + r), 0.0)[:-1]
        assert abs(f[c] - fs.max()) <= 1e-12, (c, f[c], fs.max())
        assert op.counts[c].tolist() == counts_at(t[:, c], s[:, c], op.threshold[c])


@pytest.mark.parametrize("level", [0.5, 0.9, 1.0])
def test_precision_criterion(data, level):
    t, s = data
    op = operating_points_host(t, s, ("precision", level))
    reached = 0
    for c in range(C):
        cand = np.unique(s[t[:, c], c])
        prec = np.array([(lambda k: k[0] / (k[0] + k[1]))(counts_at(t[:, c], s[:, c], v)) for v in cand])
        if not (prec >= level).any():
            assert op.threshold[c] == np.inf and op.counts[c].tolist() == [0, 0, int(t[:, c].sum()), int((~t[:, c]).sum())]
            continue
        reached += 1
        i = int(np.nonzero(cand == op.threshold[c])[0][0])
        assert op.counts[c].tolist() == counts_at(t[:, c], s[:, c], op.threshold[c])
        assert op.precision[c] >= level
        assert (prec[:i] < level).all(), "every lower candidate misses the precision: this is the lowest that reaches it"
        # sklearn agrees on the precision at this threshold
        p, r, th = pr_curve(t[:, c], s[:, c])
        assert abs(p[np.nonzero(th == op.threshold[c])[0][0]] - op.precision[c]) <= 1e-15
    assert reached >= (C // 2 if level < 1.0 else 1)


@pytest.mark.parametrize("level", [0.5, 0.8, 1.0])
def test_recall_criterion(data, level):
    t, s = data
    op = operating_points_host(t, s, ("recall", level))
    for c in range(C):
        cand = np.unique(s[t[:, c], c])
        i = int(np.nonzero(cand == op.threshold[c])[0][0])
        assert op.counts[c].tolist() == counts_at(t[:, c], s[:, c], op.threshold[c])
        assert op.recall[c] >= level
        if i + 1 < len(cand):                                       # the next higher candidate loses the recall
            k = counts_at(t[:, c], s[:, c], cand[i + 1])
            assert k[0] / (k[0] + k[2]) < level
        p, r, th = pr_curve(t[:, c], s[:, c])
        assert abs(r[np.nonzero(th == op.threshold[c])[0][0]] - op.recall[c]) <= 1e-15
    if level == 1.0:
        assert np.array_equal(op.threshold, np.array([s[t[:, c], c].min() for c in range(C)]))


def test_tie_rule_equal_f_takes_the_highest_threshold():
    # t = 0.9: TP 1, FP 0, FN 2 -> F1 = 2 / 4;  t = 0.5: TP 3, FP 6, FN 0 -> F1 = 6 / 12: equal, bit for bit
    s = np.array([0.9, 0.5, 0.5] + [0.6] * 6 + [0.1], np.float32)[:, None]
    t = np.array([1, 1, 1] + [0] * 6 + [0])[:, None]
    op = operating_points_host(t, s, "f1")
    assert op.threshold[0] == np.float32(0.9) and op.counts[0].tolist() == [1, 0, 2, 7]
    # nudged: one negative fewer above 0.5 and the lower threshold wins
    s2 = s.copy()
    s2[3, 0] = 0.2
    op = operating_points_host(t, s2, "f1")
    assert op.threshold[0] == np.float32(0.5) and op.counts[0].tolist() == [3, 5, 0, 2]


def test_degenerate_inputs():
    inf = np.inf
    # signed zeros are one score, returned as +0.0
    s = np.array([[-0.0], [0.0], [-0.0], [-1.0]], np.float32)
    t = np.array([[1], [0], [1], [0]])
    for crit in ("f1", ("precision", 0.5), ("recall", 1.0)):
        op = operating_points_host(t, s, crit)
        assert op.threshold[0] == 0.0 and not np.signbit(op.threshold[0])
        assert op.counts[0].tolist() == [2, 1, 0, 1]
    # no positives; no negatives; a precision no threshold reaches
    rs = np.random.RandomState(3)
    s = rs.uniform(size=(50, 3)).astype(np.float32)
    t = rs.uniform(size=(50, 3)) < 0.4
    t[:, 0] = False
    t[:, 1] = True
    s[:, 2] = np.where(t[:, 2], s[:, 2] * 0.5, s[:, 2])
    s[np.nonzero(~t[:, 2])[0][0], 2] = 0.99                         # a negative on top: precision 1 is out of reach
    for crit in ("f1", ("precision", 1.0), ("recall", 0.5)):
        op = operating_points_host(t, s, crit)
        assert op.threshold[0] == inf and op.counts[0].tolist() == [0, 0, 0, 50]
        if crit != ("precision", 1.0):
            assert op.threshold[1] == s[:, 1].min() or crit == ("recall", 0.5)
            assert op.counts[1, 1] == 0 and op.counts[1, 3] == 0
    op = operating_points_host(t, s, ("precision", 1.0))
    P2 = int(t[:, 2].sum())
    assert op.threshold[2] == inf and op.counts[2].tolist() == [0, 0, P2, 50 - P2]
    assert op.precision[2] == 0.0 and op.recall[0] == 0.0 and op.f()[0] == 0.0           # 0 / 0 reads 0
    # N = 1
    op = operating_points_host(np.array([[1, 0]]), np.array([[0.3, 0.7]], np.float32), "f1")
    assert op.threshold.tolist() == [np.float32(0.3), inf] and op.counts.tolist() == [[1, 0, 0, 0], [0, 0, 0, 1]]


def test_argument_errors():
    t, s = np.zeros((4, 2)), np.zeros((4, 2), np.float32)
    for bad in ("f2", ("fbeta", 0.0), ("fbeta", np.inf), ("precision", 0.0), ("precision", 1.1), ("recall", -0.1), ("auc", 0.5), 3):
        with pytest.raises(ValueError):
            operating_points_host(t, s, bad)
    with pytest.raises(ValueError, match="differs"):
        operating_points_host(np.zeros((4, 3)), s)
    with pytest.raises(ValueError, match="NaN or infinite"):
        operating_points_host(t, np.full((4, 2), np.nan, np.float32))
    with pytest.raises(ValueError, match="other than 0 and 1"):
        operating_points_host(np.full((4, 2), 2), s)
    assert isinstance(operating_points_host(t, s), OperatingPoints)


# ---- decode_events with one threshold / low per class ------------------------------------------------------------------------

def probabilities(S, K, seed):
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((S + 4, K))
    z = (z[:-4] + z[1:-3] + z[2:-2] + z[3:-1] + z[4:]) / 5 ** 0.5
    return (1.0 / (1.0 + np.exp(-3.0 * (z - 0.3)))).astype(np.float32)


@pytest.mark.parametrize("args", [dict(), dict(median=3, merge_gap=0.33), dict(median=5, min_duration=0.65)])
def test_decode_events_per_class_equals_column_by_column(args):
    p = probabilities(60, 9, 1)
    rs = np.random.RandomState(2)
    thr = rs.uniform(0.3, 0.8, size=9).astype(np.float32)
    thr[4] = np.inf
    thr[6] = p[17, 6]                                               # exactly a value of the column
    low = (thr * rs.uniform(0.4, 1.0, size=9)).astype(np.float32)
    low[4] = 0.2
    got = seg.decode_events(p, threshold=thr, low=low, **args)
    want = []
    for c in range(9):
        want += [(c,) + e[1:] for e in seg.decode_events(p[:, c:c + 1], threshold=float(thr[c]), low=float(low[c]), **args)]
    want.sort(key=lambda ev: (ev[1], ev[2], str(ev[0])))
    assert got == want and len(got) >= 9
    assert not [e for e in got if e[0] == 4], "+inf: the class emits nothing"
    # low=None: every class's own threshold; tensors and lists are taken like arrays
    assert seg.decode_events(p, threshold=thr, **args) == seg.decode_events(p, threshold=torch.from_numpy(thr), low=thr.tolist(), **args)
    # a number beside per-class values
    mixed = seg.decode_events(p, threshold=thr, low=0.1, **args)
    assert mixed == seg.decode_events(p, threshold=thr, low=np.full(9, 0.1, np.float32), **args)
    mixed = seg.decode_events(p, threshold=0.9, low=np.minimum(low, 0.9), **args)
    assert mixed == seg.decode_events(p, threshold=np.full(9, 0.9), low=np.minimum(low, 0.9), **args)


def test_decode_events_constant_array_equals_scalar():
    p = probabilities(80, 7, 3)
    for args in (dict(), dict(low=0.3, median=3), dict(low=0.3, merge_gap=0.7, min_duration=0.65)):
        a = dict(args)
        if "low" in a:
            a["low"] = np.full(7, a["low"])
        assert seg.decode_events(p, threshold=np.full(7, 0.5), **a) == seg.decode_events(p, threshold=0.5, **args)
        assert seg.decode_events(p, threshold=np.full(7, 0.5, np.float32), **a) == seg.decode_events(p, **args)


def test_decode_events_per_class_argument_errors():
    p = probabilities(10, 4, 4)
    with pytest.raises(ValueError, match="3 per-class values for 4 classes"):
        seg.decode_events(p, threshold=np.full(3, 0.5))
    with pytest.raises(ValueError, match="5 per-class values for 4 classes"):
        seg.decode_events(p, low=np.full(5, 0.1))
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\] .* in class 2"):
        seg.decode_events(p, threshold=np.array([0.5, 0.5, 0.5, 0.5]), low=np.array([0.5, 0.1, 0.6, 0.0]))
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\] .* in class 1"):
        seg.decode_events(p, threshold=np.array([0.5, np.nan, 0.5, 0.5]))
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\] .* in class 3"):
        seg.decode_events(p, threshold=0.5, low=np.array([0.5, 0.1, 0.2, -0.1]))
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\] .* in class 0"):
        seg.decode_events(p, threshold=np.array([0.2, 0.9, 0.9, 0.9]), low=0.3)
    with pytest.raises(ValueError, match="one-dimensional"):
        seg.decode_events(p, threshold=np.full((4, 1), 0.5))
    with pytest.raises(ValueError, match="numbers"):
        seg.decode_events(p, threshold=np.array(["a", "b", "c", "d"]))
    # the device decoder checks host arrays the same way, before it looks for a GPU
    x = torch.from_numpy(p)
    with pytest.raises(ValueError, match=r"low must be in \[0, threshold\] .* in class 2"):
        seg.decode_events_gpu(x, threshold=np.array([0.5, 0.5, 0.5, 0.5]), low=np.array([0.5, 0.1, 0.6, 0.0]))
    with pytest.raises(ValueError, match="3 per-class values for 4 classes"):
        seg.decode_events_gpu(x, threshold=np.full(3, 0.5))
    assert seg.check_event_args(0.5, None, 1, 0.0, 0.0) == (0.5, 0.5)
    thr, low = seg.check_event_args([0.5, 0.6], None, 1, 0.0, 0.0, classes=2)
    assert thr.dtype == np.float32 and low is thr


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_ffi_declarations_and_argument_checks():
    lib = _ffi.lib()
    for name in ("acx_operating_points", "acx_threshold_counts", "acx_decode_events_classwise", "acx_decode_events_varlen_classwise"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert ctypes.sizeof(_ffi.AcxOperatingSpec) == 16 and _ffi.AcxOperatingSpec.param.offset == 8
    assert (_ffi.OP_FBETA, _ffi.OP_PRECISION, _ffi.OP_RECALL) == (0, 1, 2)
    assert _ffi.METRICS_BAD_THRESHOLD == 4 and _ffi.EVENTS_BAD_THRESHOLD == 4
    # argument errors come back before anything touches a device: the pointers below are never read
    fake = ctypes.c_void_p(4096)
    n, classes = 100, 7
    need = _ffi.metrics_workspace_bytes(n, classes)                 # the workspace of acx_tagging_metrics, reused

    def op(criterion, param, ws_bytes=need, scores=fake, n_=n):
        spec = _ffi.AcxOperatingSpec(criterion, param)
        return lib.acx_operating_points(scores, classes, fake, _ffi.TARGET_U8, classes, n_, classes, ctypes.byref(spec), fake, fake,
                                        fake, fake, ws_bytes, None)

    for criterion, param in ((3, 0.5), (-1, 0.5), (_ffi.OP_FBETA, 0.0), (_ffi.OP_FBETA, float("inf")), (_ffi.OP_FBETA, float("nan")),
                             (_ffi.OP_PRECISION, 0.0), (_ffi.OP_PRECISION, 1.5), (_ffi.OP_RECALL, float("nan"))):
        assert op(criterion, param) == -1, (criterion, param)
        assert b"acx_operating_points" in lib.acx_last_error()
    assert op(_ffi.OP_FBETA, 1.0, ws_bytes=need - 256) == -5 and b"workspace" in lib.acx_last_error()
    assert op(_ffi.OP_FBETA, 1.0, scores=None) == -1
    assert op(_ffi.OP_FBETA, 1.0, n_=0) == -1
    assert lib.acx_threshold_counts(fake, classes, fake, _ffi.TARGET_U8, classes, n, classes, None, fake, fake, None) == -1
    assert lib.acx_threshold_counts(fake, classes - 1, fake, _ffi.TARGET_U8, classes, n, classes, fake, fake, fake, None) == -1
    assert lib.acx_threshold_counts(fake, classes, fake, 5, classes, n, classes, fake, fake, fake, None) == -1
    # the classwise decoder: the scalar checks still hold where a scalar is still in use
    ws = _ffi.events_workspace_bytes(2, 70)
    params = _ffi.event_params(0.5, 0.6)                            # low > threshold

    def dec(thr, low, p=params):
        return lib.acx_decode_events_classwise(fake, 70, 2, 10, 70, ctypes.byref(p), 0.32, 0.0, fake, 16, fake, fake, fake, ws - 256,
                                               None, thr, low)

    assert dec(None, None) == -1 and b"low" in lib.acx_last_error()
    assert dec(fake, None) == -5                                    # the fields are ignored; next in line is the short workspace
    assert dec(fake, fake) == -5
    assert dec(None, fake, _ffi.event_params(-0.5, -0.5)) == -1
