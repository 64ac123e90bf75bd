"""CPU: single-label heads -- the host definitions of pytorch/classify.py (softmax_topk_host, classification_metrics_host,
cross_entropy_host) against hand-worked cases, sklearn and F.cross_entropy; fit_head's loss="ce" argument validation; the
ctypes declarations of the new symbols and their argument errors that need no launch.  No device needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import sklearn.metrics as sk
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import classify as cl
from audioset_convnext_inf_amd.pytorch.finetune import fit_head, labels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("acx_head_fit_ce_workspace_bytes", "acx_head_fit_step_ce", "acx_head_fit_grad_ce", "acx_softmax_topk",
       "acx_classification_counts")


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------
def test_topk_order_by_hand():
    z = np.array([[1.0, 3.0, 3.0, 0.5],            # a tie at the maximum: the lower index first
                  [2.0, 1.0, 1.0, 1.0],            # a tie at rank k = 2: class 1 is in, 2 and 3 are out
                  [-0.0, 0.0, -1.0, 0.0],          # -0.0 equals +0.0: index order among the three zeros
                  [5.0, 5.0, 5.0, 5.0]], dtype=np.float32)
    probs, top_prob, top_index = cl.softmax_topk_host(z, k=2)
    assert top_index.tolist() == [[1, 2], [0, 1], [0, 1], [0, 1]]
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-15)
    assert np.array_equal(top_prob, np.take_along_axis(probs, top_index, axis=1))
    assert np.allclose(probs[3], 0.25) and np.allclose(probs[0, 1], probs[0, 2])
    e = np.exp(np.array([1.0, 3.0, 3.0, 0.5]) - 3.0)
    assert np.allclose(probs[0], e / e.sum(), rtol=1e-15)
    # logits around +-80: exp overflows in float32 (and e^160 in the ratio) without the max subtraction
    big = np.array([[80.0, -80.0, 79.0]], dtype=np.float32)
    p = cl.softmax_topk_host(big, k=1)[0]
    assert np.isfinite(p).all() and abs(p[0, 0] - 1.0 / (1.0 + np.exp(-1.0) + np.exp(-160.0))) < 1e-15
    # a non-finite row
    bad = np.array([[1.0, np.nan], [np.inf, 0.0], [0.0, 1.0]], dtype=np.float32)
    p, tp, ti = cl.softmax_topk_host(bad, k=1)
    assert np.isnan(p[:2]).all() and np.isnan(tp[:2]).all() and ti[:, 0].tolist() == [-1, -1, 1]


def test_counts_by_hand():
    #            class:  0     1     2     3
    z = np.array([[1.0, 3.0, 3.0, 0.5],            # y = 2: prediction 1 (first maximum), rank of 2 is 1 -> top-2 hit
                  [2.0, 1.0, 1.0, 1.0],            # y = 2: rank 2 (0 above, 1 ties with a lower index) -> no top-2 hit
                  [2.0, 1.0, 1.0, 1.0],            # y = 1: rank 1 -> top-2 hit
                  [-0.0, 0.0, -1.0, 0.0],          # y = 0: prediction 0 (-0.0 == +0.0, first index), correct
                  [0.0, -0.0, -1.0, 0.0],          # y = 1: rank 1 (class 0 ties with a lower index)
                  [9.0, 0.0, 0.0, 0.0]], dtype=np.float32)   # y = 0: correct
    y = np.array([2, 2, 1, 0, 1, 0])
    m = cl.classification_metrics_host(y, z, k=2)
    assert m.per_class.tolist() == [[2, 5, 2], [2, 1, 0], [2, 0, 0], [0, 0, 0]]      # support, predicted, correct
    assert m.hits.tolist() == [2, 5]
    conf = np.zeros((4, 4), dtype=np.int64)
    for t, p in zip(y, [1, 0, 0, 0, 0, 0]):
        conf[t, p] += 1
    assert np.array_equal(m.confusion, conf)
    assert m.accuracy == 2 / 6 and m.topk_accuracy == 5 / 6
    assert m.recall.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert m.precision.tolist() == [2 / 5, 0.0, 0.0, 0.0]          # class 2 was never predicted: precision 0; class 3 too
    assert m.f1.tolist() == [4 / 7, 0.0, 0.0, 0.0]
    assert m.balanced_accuracy == pytest.approx(1.0 / 3.0)         # class 3 has no support: left out of both means
    assert m.macro_f1 == pytest.approx(4 / 7 / 3)
    # rows left out: a non-finite logit, labels outside [0, N)
    z2 = np.vstack([z, [[np.nan, 0, 0, 0]], [[1, 2, 3, 4]], [[1, 2, 3, 4]]]).astype(np.float32)
    m2 = cl.classification_metrics_host(np.concatenate([y, [0, -1, 4]]), z2, k=2)
    assert m2.skipped == 3 and np.array_equal(m2.per_class, m.per_class) and np.array_equal(m2.hits, m.hits)
    assert m2.counted == 6 and m2.accuracy == m.accuracy


# ---- sklearn -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,k", [(500, 7, 3), (2000, 50, 5), (300, 2, 1)])
def test_metrics_against_sklearn(n, N, k):
    rng = np.random.default_rng(n + N)
    y = rng.integers(0, N - 1 if N > 2 else N, size=n)                               # N > 2: the last class has no support
    z = rng.standard_normal((n, N)).astype(np.float32)
    z[np.arange(n), y] += 1.5
    if N > 2:
        z[:, 1] -= 50.0                                                              # class 1 is never predicted
    assert all(len(np.unique(r)) == N for r in z)                                    # no score ties
    m = cl.classification_metrics_host(y, z, k=k)
    pred = z.argmax(axis=1)
    assert m.accuracy == pytest.approx(sk.accuracy_score(y, pred), abs=1e-15)
    if N > 2:
        want_topk = sk.top_k_accuracy_score(y, z, k=k, labels=np.arange(N))
    else:
        want_topk = sk.accuracy_score(y, pred)                                       # k = 1
    assert m.topk_accuracy == pytest.approx(want_topk, abs=1e-15)
    assert np.array_equal(m.confusion, sk.confusion_matrix(y, pred, labels=np.arange(N)))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                              # "y_pred contains classes not in y_true"
        assert m.balanced_accuracy == pytest.approx(sk.balanced_accuracy_score(y, pred), abs=1e-14)
    present = np.unique(y)
    assert m.macro_f1 == pytest.approx(sk.f1_score(y, pred, labels=present, average="macro", zero_division=0), abs=1e-14)
    assert np.allclose(m.precision, sk.precision_score(y, pred, labels=np.arange(N), average=None, zero_division=0), atol=1e-15)
    assert np.allclose(m.recall, sk.recall_score(y, pred, labels=np.arange(N), average=None, zero_division=0), atol=1e-15)
    probs, top_prob, top_index = cl.softmax_topk_host(z, k=k)
    assert np.array_equal(top_index, np.argsort(-z.astype(np.float64), axis=1)[:, :k])
    assert np.allclose(probs, torch.softmax(torch.from_numpy(z).double(), dim=1).numpy(), rtol=1e-13, atol=0)


# ---- cross-entropy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("rows,N,scale", [(1, 1, 1.0), (7, 2, 1.0), (64, 50, 3.0), (5, 527, 30.0)])
def test_cross_entropy_host_against_torch(rows, N, scale, eps):
    g = torch.Generator().manual_seed(rows * 1000 + N)
    z = (torch.randn(rows, N, generator=g, dtype=torch.float64) * scale).requires_grad_()
    y = torch.randint(0, N, (rows,), generator=g)
    want = F.cross_entropy(z, y, label_smoothing=eps)
    want.backward()
    loss, per_row, grad = cl.cross_entropy_host(z.detach().numpy(), y.numpy(), eps)
    assert loss == pytest.approx(float(want.detach()), rel=1e-13, abs=1e-14)
    assert np.allclose(per_row, F.cross_entropy(z.detach(), y, label_smoothing=eps, reduction="none").numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(grad, z.grad.numpy(), rtol=1e-12, atol=1e-16)
    if N == 1:
        assert loss == 0.0 and not grad.any()


# ---- fit_head(loss="ce") argument validation: every error comes before any device call --------------------------------------
def test_fit_head_ce_validation():
    emb = torch.zeros(4, 768)
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        fit_head(emb, torch.tensor([0, 1, 2, 3]), loss="ce", classes=3)
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        fit_head(emb, torch.tensor([0, -1, 2, 1]), loss="ce", classes=3)
    with pytest.raises(ValueError, match="exactly one 1"):
        fit_head(emb, torch.tensor([[1, 0, 0], [0, 1, 1], [0, 0, 1], [1, 0, 0]]), loss="ce")
    with pytest.raises(ValueError, match="exactly one 1"):
        fit_head(emb, torch.tensor([[1, 0, 0], [0, 0, 0], [0, 0, 1], [1, 0, 0]]).float(), loss="ce")
    with pytest.raises(ValueError, match="other than 0 and 1"):
        fit_head(emb, torch.tensor([[0.5, 0.5, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]]), loss="ce")
    with pytest.raises(ValueError, match="label_smoothing"):
        fit_head(emb, torch.zeros(4, 3), label_smoothing=0.1)
    with pytest.raises(ValueError, match="label_smoothing"):
        fit_head(emb, torch.tensor([0, 1, 2, 0]), loss="ce", classes=3, label_smoothing=1.0)
    with pytest.raises(ValueError, match="classes= is required"):
        fit_head(emb, torch.tensor([0, 1, 2, 0]), loss="ce")
    with pytest.raises(ValueError, match="classes="):
        fit_head(emb, torch.zeros(4, 3), classes=3)                                # bce takes the width of the target
    with pytest.raises(ValueError, match="integer"):
        fit_head(emb, torch.tensor([0.0, 1.0, 2.0, 0.0]), loss="ce", classes=3)
    with pytest.raises(ValueError, match="loss must be"):
        fit_head(emb, torch.zeros(4, 3), loss="mse")
    with pytest.raises(ValueError, match="CUDA"):
        fit_head(emb, torch.tensor([0, 1, 2, 0]), loss="ce", classes=3)             # valid labels: the GPU-only error is next
    lab, N = labels_of(torch.tensor([[0, 0, 1], [1, 0, 0]], dtype=torch.bool), 2)
    assert lab.tolist() == [2, 0] and N == 3 and lab.dtype == torch.int64
    lab, N = labels_of(torch.tensor([3, 0], dtype=torch.int32), 2, classes=4)
    assert lab.tolist() == [3, 0] and N == 4 and lab.dtype == torch.int64


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    declared = set(re.findall(r"^ACX_API[^;(]*?\b(acx_\w+)\s*\(", hdr, flags=re.M))
    lib = _ffi.lib()
    for name in NEW:
        assert name in declared and name in _ffi.SIGNATURES and hasattr(lib, name)
    assert declared == set(_ffi.SIGNATURES)                                        # the agreement still holds
    sig = _ffi.SIGNATURES
    assert len(sig["acx_head_fit_step_ce"][1]) == 24 and len(sig["acx_head_fit_grad_ce"][1]) == 19
    assert len(sig["acx_softmax_topk"][1]) == 11 and len(sig["acx_classification_counts"][1]) == 11
    assert sig["acx_head_fit_step_ce"][1][7] is ctypes.c_double and sig["acx_head_fit_grad_ce"][1][7] is ctypes.c_double
    assert sig["acx_head_fit_step_ce"][1][6] is ctypes.c_int and sig["acx_head_fit_step_ce"][1][16] == ctypes.POINTER(_ffi.AcxAdam)
    for name, value in (("ACX_FIT_BAD_LABEL", _ffi.FIT_BAD_LABEL), ("ACX_CLASSIFY_MAX_K", _ffi.CLASSIFY_MAX_K),
                        ("ACX_CLASSIFY_NONFINITE", _ffi.CLASSIFY_NONFINITE), ("ACX_CLASSIFY_BAD_LABEL", _ffi.CLASSIFY_BAD_LABEL)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == value


def err():
    return _ffi.lib().acx_last_error().decode()


def test_workspace_size_and_depth():
    for rows, N in ((1, 1), (64, 50), (512, 527), (256, 4096), (7, 32768)):
        a = lambda v: (v + 255) & ~255
        assert _ffi.head_fit_ce_workspace_bytes(rows, N) == 2 * a(rows * N * 4) + a(rows * 4)
    assert _ffi.head_fit_ce_workspace_bytes(64, 50) <= _ffi.head_fit_ce_workspace_bytes(65, 50) <= _ffi.head_fit_ce_workspace_bytes(65, 51)
    with pytest.raises(_ffi.AcxError, match="rows"):
        _ffi.head_fit_ce_workspace_bytes(0, 10)
    with pytest.raises(_ffi.AcxError, match="classes"):
        _ffi.head_fit_ce_workspace_bytes(4, _ffi.MAX_CLASSES + 1)
    assert _ffi.lib().acx_head_fit_ce_workspace_bytes(4, 4, None) == -1 and "out_bytes" in err()
    assert [_ffi.softmax_depth(N) for N in (1, 64, 65, 527, 2048, 2049, 4096, 32768)] == [7, 7, 8, 15, 38, 18, 25, 137]


def test_argument_errors_need_no_device():
    """Every check below fails before the first device call; the pointers are never dereferenced."""
    lib = _ffi.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256)     # 256-byte aligned host memory
    hp = _ffi.adam()

    def step(**o):
        a = dict(E=p, ld_e=768, n=8, labels=p, idx=p, rows=4, N=10, eps=0.0, W=p, b=p, mW=p, vW=p, xW=p, mb=p, vb=p, xb=p,
                 hp=ctypes.byref(hp), t=1, lr=1e-3, loss=p, status=p, ws=p, wsb=1 << 20)
        a.update(o)
        return lib.acx_head_fit_step_ce(a["E"], a["ld_e"], a["n"], a["labels"], a["idx"], a["rows"], a["N"], a["eps"], a["W"], a["b"],
                                        a["mW"], a["vW"], a["xW"], a["mb"], a["vb"], a["xb"], a["hp"], a["t"], a["lr"], a["loss"],
                                        a["status"], a["ws"], a["wsb"], None)

    for over, code, word in [({"E": None}, -1, "E"), ({"labels": None}, -1, "labels"), ({"idx": None}, -1, "idx"),
                             ({"W": None}, -1, "W"), ({"b": None}, -1, "b"), ({"status": None}, -1, "status"),
                             ({"ws": None}, -1, "workspace"), ({"eps": -0.1}, -1, "label_smoothing"),
                             ({"eps": 1.0}, -1, "label_smoothing"), ({"eps": float("nan")}, -1, "label_smoothing"),
                             ({"rows": 0}, -1, "rows"), ({"N": 0}, -1, "classes"), ({"N": _ffi.MAX_CLASSES + 1}, -1, "classes"),
                             ({"rows": (1 << 22) + 1}, -6, "rows"), ({"n": 0}, -1, "n_rows_total"), ({"ld_e": 767}, -1, "ld_e"),
                             ({"ld_e": 770}, -1, "ld_e"), ({"wsb": 100}, -5, "workspace"),
                             ({"ws": ctypes.c_void_p(p.value + 64)}, -5, "aligned"), ({"mW": None}, -1, "mW"),
                             ({"loss": None}, -1, "loss_out"), ({"hp": None}, -1, "hp"), ({"t": 0}, -1, "step_t"),
                             ({"lr": -1.0}, -1, "lr"), ({"xW": None}, -1, "vmaxW")]:
        rc = step(**over)
        assert rc == code and word in err(), (over, rc, err())

    def grad(**o):
        a = dict(E=p, ld_e=768, n=8, labels=p, idx=p, rows=4, N=10, eps=0.0, W=p, b=p, z=p, G=p, dW=p, db=p, loss=p, status=p,
                 ws=p, wsb=1 << 20)
        a.update(o)
        return lib.acx_head_fit_grad_ce(a["E"], a["ld_e"], a["n"], a["labels"], a["idx"], a["rows"], a["N"], a["eps"], a["W"], a["b"],
                                        a["z"], a["G"], a["dW"], a["db"], a["loss"], a["status"], a["ws"], a["wsb"], None)

    for over, code, word in [({"z": None}, -1, "z"), ({"G": None}, -1, "G"), ({"labels": None}, -1, "labels"),
                             ({"eps": 2.0}, -1, "label_smoothing"), ({"wsb": 0}, -5, "workspace")]:
        rc = grad(**over)
        assert rc == code and word in err(), (over, rc, err())

    def topk(**o):
        a = dict(z=p, ld=16, rows=3, N=10, k=5, probs=p, ld_p=10, ti=p, tp=p, status=p)
        a.update(o)
        return lib.acx_softmax_topk(a["z"], a["ld"], a["rows"], a["N"], a["k"], a["probs"], a["ld_p"], a["ti"], a["tp"], a["status"],
                                    None)

    for over, code, word in [({"z": None}, -1, "logits"), ({"ti": None}, -1, "top_index"), ({"tp": None}, -1, "top_prob"),
                             ({"status": None}, -1, "status"), ({"rows": 0}, -1, "rows"), ({"N": 0}, -1, "classes"),
                             ({"N": _ffi.MAX_CLASSES + 1, "ld": 1 << 20}, -1, "classes"), ({"ld": 9}, -1, "ld ="),
                             ({"ld_p": 9}, -1, "ld_p"), ({"k": 0}, -1, "k ="), ({"k": 11}, -1, "k ="),
                             ({"N": 100, "ld": 100, "ld_p": 100, "k": 65}, -1, "k ="), ({"rows": (1 << 30) + 1}, -6, "rows")]:
        rc = topk(**over)
        assert rc == code and word in err(), (over, rc, err())

    def counts(**o):
        a = dict(z=p, ld=16, labels=p, n=3, N=10, k=5, pc=p, hits=p, conf=p, status=p)
        a.update(o)
        return lib.acx_classification_counts(a["z"], a["ld"], a["labels"], a["n"], a["N"], a["k"], a["pc"], a["hits"], a["conf"],
                                             a["status"], None)

    for over, code, word in [({"z": None}, -1, "logits"), ({"labels": None}, -1, "labels"), ({"pc": None}, -1, "per_class"),
                             ({"hits": None}, -1, "hits"), ({"status": None}, -1, "status"), ({"n": 0}, -1, "n ="),
                             ({"ld": 9}, -1, "ld ="), ({"k": 0}, -1, "k ="), ({"k": 11}, -1, "k ="),
                             ({"N": 4097, "ld": 4097}, -6, "confusion"), ({"n": (1 << 30) + 1}, -6, "n =")]:
        rc = counts(**over)
        assert rc == code and word in err(), (over, rc, err())
    assert buf.raw == b"\0" * 4096                                                  # nothing was written
