"""CPU: the host side of the weak-label SED fit (pytorch/finetune.py fit_sed_head / mil_grad_host / fit_sed_head_host /
sed_schedule, pytorch/segments.py pool_segments_host, acx_head_fit_step_mil / acx_head_fit_grad_mil / acx_segment_pool in
include/acx.h): the closed-form bag pass against torch's float64 autograd through sigmoid -> pooling -> F.binary_cross_entropy,
hand-worked cases, the schedule builder against a loop, argument checks that return before any device call, and the planted-event
fit on the host definition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import finetune as ft
from audioset_convnext_inf_amd.pytorch import segments as seg
from sed_fit_cases import PLANT, POOLINGS, localisation, planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED, WORKSPACE = -1, -6, -5


def q_of(z):
    return torch.sigmoid(torch.as_tensor(z, dtype=torch.float64))


# ---- 1. the closed form against autograd -------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("pooling", POOLINGS)
def test_mil_grad_host_equals_autograd(pooling, soft):
    """Ragged bags of 1, 2, 7, 0 (empty), 31 and 3 rows, 5 classes: G, P and the loss of mil_grad_host against autograd through
    mil_forward_host and F.binary_cross_entropy in float64, to 1e-12 relative."""
    g = torch.Generator().manual_seed(3)
    lens = [1, 2, 7, 0, 31, 3]
    off = np.concatenate([[0], np.cumsum(lens)])
    z = (torch.randn(sum(lens), 5, generator=g, dtype=torch.float64) * 3).requires_grad_()
    y = torch.rand(len(lens), 5, generator=g, dtype=torch.float64)
    if not soft:
        y = (y < 0.5).double()
    P, _ = ft.mil_forward_host(z, off, pooling)
    loss = F.binary_cross_entropy(P, y)
    loss.backward()
    got = ft.mil_grad_host(z.detach(), off, y, pooling)
    assert got.G.shape == z.shape and got.P.shape == (6, 5)
    assert torch.allclose(got.G, z.grad, rtol=1e-12, atol=1e-18), float((got.G - z.grad).abs().max())
    assert torch.allclose(got.P, P.detach(), rtol=0, atol=0)
    assert abs(float(got.loss) - float(loss.detach())) <= 1e-13 * abs(float(loss.detach()))
    assert bool((got.P[3] == 0).all()) and torch.allclose(got.terms[3], 100 * y[3])     # the empty bag: P = 0, its loss term, no rows


def test_max_is_the_reference_recipe():
    """pooling="max" on uniform bags is the reference's decision-level path stated in torch: segmentwise = sigmoid(z),
    clipwise = max over time (models.py:5767), clip_bce = F.binary_cross_entropy(clipwise, target) (losses.py)."""
    g = torch.Generator().manual_seed(5)
    B, S, N = 6, 31, 10
    z = torch.randn(B, S, N, generator=g, dtype=torch.float64).requires_grad_()
    y = (torch.rand(B, N, generator=g) < 0.3).double()
    clipwise = torch.sigmoid(z).max(dim=1).values
    loss = F.binary_cross_entropy(clipwise, y)
    loss.backward()
    got = ft.mil_grad_host(z.detach().reshape(B * S, N), np.arange(B + 1) * S, y, "max")
    assert torch.equal(got.P, clipwise.detach())
    assert abs(float(got.loss) - float(loss.detach())) <= 1e-14
    assert torch.allclose(got.G, z.grad.reshape(B * S, N), rtol=1e-12, atol=1e-18)
    assert torch.equal(got.tstar, z.detach().argmax(dim=1))                        # continuous inputs: no ties
    assert torch.equal(seg.pool_segments_host(z.detach(), "max"), clipwise.detach())


# ---- 2. hand-worked cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooling", POOLINGS)
def test_one_segment_bag_pools_to_its_probability(pooling):
    z = torch.tensor([[0.3, -2.0, 5.0]], dtype=torch.float64)
    y = torch.tensor([[1.0, 0.0, 0.25]], dtype=torch.float64)
    got = ft.mil_grad_host(z, [0, 1], y, pooling)
    q = q_of(z)
    assert torch.allclose(got.P, q, rtol=1e-15, atol=0)
    # dP/dq = 1, so G = (q - y) / max(q (1 - q), 1e-12) q (1 - q) / 3 = (q - y) / 3: the logit form
    assert torch.allclose(got.G, (q - y) / 3, rtol=1e-12, atol=0)


def test_two_equal_maxima_send_the_gradient_to_the_lower_row():
    z = torch.tensor([[-1.0], [2.0], [0.5], [2.0]], dtype=torch.float64)
    got = ft.mil_grad_host(z, [0, 4], torch.ones(1, 1), "max")
    assert int(got.tstar) == 1
    q = float(q_of(2.0))
    assert float(got.P) == q
    assert got.G[:, 0].tolist() == [0.0, (q - 1.0) / (q * (1 - q)) * q * (1 - q), 0.0, 0.0]
    # saturation: every row at the same large logit is a tie as well
    got = ft.mil_grad_host(torch.full((3, 1), 40.0, dtype=torch.float64), [0, 3], torch.zeros(1, 1), "max")
    assert int(got.tstar) == 0 and float(got.P) == 1.0 and bool((got.G == 0).all())
    assert float(got.loss) == 100.0                                                # log1p(-1) = -inf, held at -100


def test_no_probability_mass_pools_to_zero():
    z = torch.full((4, 2), -1000.0, dtype=torch.float64)                           # sigmoid underflows to 0 in float64 too
    y = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    for pooling in POOLINGS:
        got = ft.mil_grad_host(z, [0, 4], y, pooling)
        assert bool((got.P == 0).all()) and bool((got.G == 0).all()), pooling
        assert got.terms.tolist() == [[100.0, 0.0]], pooling


def test_linear_and_exp_by_hand():
    z = torch.tensor([[0.0], [np.log(3.0)]], dtype=torch.float64)                  # q = 1/2, 3/4
    got = ft.mil_grad_host(z, [0, 2], torch.zeros(1, 1), "linear")
    P = (0.25 + 0.5625) / 1.25
    assert abs(float(got.P) - P) < 1e-15
    dLdP = P / (P * (1 - P))
    want = [dLdP * (2 * q - P) / 1.25 * q * (1 - q) for q in (0.5, 0.75)]
    assert np.allclose(got.G[:, 0].numpy(), want, rtol=1e-13, atol=0)
    got = ft.mil_grad_host(z, [0, 2], torch.zeros(1, 1), "exp")
    e = np.exp([0.5, 0.75])
    P = float((np.array([0.5, 0.75]) * e).sum() / e.sum())
    assert abs(float(got.P) - P) < 1e-15
    want = [P / (P * (1 - P)) * e[i] * (1 + q - P) / e.sum() * q * (1 - q) for i, q in enumerate((0.5, 0.75))]
    assert np.allclose(got.G[:, 0].numpy(), want, rtol=1e-13, atol=0)
    got = ft.mil_grad_host(z, [0, 2], torch.zeros(1, 1), "mean")
    assert abs(float(got.P) - 0.625) < 1e-15


def test_pool_segments_host_forms():
    g = torch.Generator().manual_seed(8)
    z = torch.randn(3, 5, 4, generator=g)
    for pooling in POOLINGS:
        a = seg.pool_segments_host(z, pooling)
        b = seg.pool_segments_host(z.reshape(15, 4), pooling, steps=[5, 5, 5])
        assert a.shape == (3, 4) and a.dtype == torch.float64 and torch.equal(a, b)
        r = seg.pool_segments_host(z.reshape(15, 4), pooling, steps=[2, 0, 13])
        assert bool((r[1] == 0).all())
    with pytest.raises(ValueError, match="add up"):
        seg.pool_segments_host(z.reshape(15, 4), "max", steps=[5, 5])
    with pytest.raises(ValueError, match="pooling"):
        seg.pool_segments_host(z, "median")


# ---- 3. the schedule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [True, False])
def test_schedule_against_a_loop(shuffle, drop_last):
    lens = [3, 1, 70, 2, 5, 1, 1, 31, 4, 9, 6]
    first = np.concatenate([[0], np.cumsum(lens)])
    epochs, batch = 3, 4
    s = ft.sed_schedule(lens, epochs, batch, seed=7, shuffle=shuffle, drop_last=drop_last)
    order = ft.epoch_orders(len(lens), epochs, 7, shuffle)
    want_steps = epochs * (2 if drop_last else 3)
    assert len(s.steps) == want_steps
    assert s.bag_idx.dtype == np.int64 and s.seg_idx.dtype == np.int64 and s.bag_off.dtype == np.int32
    k = nb = no = ns = 0
    for e in range(epochs):
        for start in range(0, len(lens), batch):
            clips = order[e, start:start + batch].tolist()
            if len(clips) < batch and drop_last:
                continue
            seg_rows, off = [], [0]
            for c in clips:
                seg_rows += list(range(first[c], first[c + 1]))
                off.append(len(seg_rows))
            assert s.steps[k] == (nb, len(clips), no, ns, len(seg_rows))
            assert s.bag_idx[nb:nb + len(clips)].tolist() == clips
            assert s.bag_off[no:no + len(clips) + 1].tolist() == off
            assert s.seg_idx[ns:ns + len(seg_rows)].tolist() == seg_rows
            nb, no, ns, k = nb + len(clips), no + len(clips) + 1, ns + len(seg_rows), k + 1
    assert k == want_steps and (nb, no, ns) == (len(s.bag_idx), len(s.bag_off), len(s.seg_idx))
    if not drop_last:
        assert len(clips) == 3                                                     # the last batch of an epoch is short
    empty = ft.sed_schedule(lens, 0, batch)
    assert empty.steps == [] and len(empty.seg_idx) == 0


# ---- 4. arguments ----------------------------------------------------------------------------------------------------------------
def test_segment_input_forms():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 4, 768, generator=g)
    packed, lens = ft.check_segments(x, device=False)
    assert packed.shape == (12, 768) and lens == [4, 4, 4]
    p2, l2 = ft.check_segments([x[0], x[1, :2], x[2, :1]], device=False)
    assert l2 == [4, 2, 1] and torch.equal(p2[4:6], x[1, :2])
    p3, l3 = ft.check_segments((packed, [5, 7]), device=False)
    assert l3 == [5, 7] and p3.data_ptr() == packed.data_ptr()
    p4, l4 = ft.check_segments((packed, torch.tensor([11, 1])), device=False)
    assert l4 == [11, 1]
    for bad, word in ((x[:, :, :700], "768"), ((packed, [5, 5]), "sum"), ((packed, [12, 0]), "at least one segment"),
                      ([x[0], x[1].double()], "dtype"), (x.double(), "float32"), ("no", "must be"), ([], "must be")):
        with pytest.raises(ValueError, match=word):
            ft.check_segments(bad, device=False)


def test_value_errors_come_before_any_device_call():
    x = torch.randn(4, 3, 768)
    y = (torch.rand(4, 2) < 0.5).float()
    with pytest.raises(ValueError, match="pooling"):
        ft.fit_sed_head(x, y, pooling="attention")
    with pytest.raises(ValueError, match="epochs"):
        ft.fit_sed_head(x, y, epochs=-1)
    with pytest.raises(ValueError, match="batch_size"):
        ft.fit_sed_head(x, y, batch_size=0)
    with pytest.raises(ValueError, match="betas"):
        ft.fit_sed_head(x, y, betas=(1.0, 0.9))
    with pytest.raises(ValueError, match="CUDA"):
        ft.fit_sed_head(x, y)                                                      # CPU tensors: the fit runs on the GPU only
    with pytest.raises(ValueError, match="pooling"):
        ft.fit_sed_head_host(x, y, pooling="median")
    with pytest.raises(ValueError, match=r"\(4, N\)"):
        ft.fit_sed_head_host(x, y[:3])
    with pytest.raises(ValueError, match="CUDA"):
        seg.pool_segments(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="bag_off"):
        ft.mil_grad_host(torch.zeros(4, 2), [0, 3, 2, 4], torch.zeros(3, 2), "max")


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    declared = set(re.findall(r"^ACX_API[^;(]*?\b(acx_\w+)\s*\(", hdr, flags=re.M))
    names = ("acx_head_fit_mil_workspace_bytes", "acx_head_fit_step_mil", "acx_head_fit_grad_mil", "acx_segment_pool")
    lib = _ffi.lib()
    for name in names:
        assert name in declared and name in _ffi.SIGNATURES and hasattr(lib, name)
    assert [len(_ffi.SIGNATURES[k][1]) for k in names] == [4, 30, 26, 9]
    assert "models.py:5757-5771" in hdr and "losses.py" in hdr
    for name, value in (("ACX_FIT_BAD_INDEX", 1), ("ACX_FIT_BAD_LABEL", 2), ("ACX_FIT_BAD_BAG", _ffi.FIT_BAD_BAG)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr)
    assert _ffi.FIT_BAD_BAG not in (_ffi.FIT_BAD_INDEX, _ffi.FIT_BAD_LABEL)
    assert re.search(r"ACX_MIL_MAX = 0, ACX_MIL_MEAN = 1, ACX_MIL_LINEAR = 2, ACX_MIL_EXP = 3", hdr)
    assert ft.MIL_POOLS == {"max": _ffi.MIL_MAX, "mean": _ffi.MIL_MEAN, "linear": _ffi.MIL_LINEAR, "exp": _ffi.MIL_EXP}


def test_workspace_query():
    q = _ffi.head_fit_mil_workspace_bytes
    base = q(1984, 64, 527)
    assert base >= 2 * 1984 * 527 * 4 + 64 * 527 * 4 + 64 * 9 * 4 and base % 256 == 0
    assert q(1985, 64, 527) >= base and q(1984, 65, 527) >= base and q(1984, 64, 528) >= base
    assert q(1, 1, 1) > 0
    for args, code in (((0, 1, 1), ARG), ((1, 0, 1), ARG), ((1, 1, 0), ARG), ((1, 1, _ffi.MAX_CLASSES + 1), ARG),
                       (((1 << 22) + 1, 1, 1), UNSUPPORTED)):
        n = ctypes.c_size_t()
        assert _ffi.lib().acx_head_fit_mil_workspace_bytes(*args, ctypes.byref(n)) == code, args
    assert _ffi.lib().acx_head_fit_mil_workspace_bytes(1, 1, 1, None) == ARG


def _aligned(nbytes):
    raw = (ctypes.c_char * (nbytes + 256))()
    return raw, (ctypes.addressof(raw) + 255) & ~255


def _abi(grad=False, **change):
    """one acx_head_fit_step_mil / acx_head_fit_grad_mil call with dummy HOST buffers in every pointer: the checks under test
    return before anything reads them"""
    keep, p = _aligned(1 << 16)
    ws_bytes = _ffi.head_fit_mil_workspace_bytes(8, 2, 3)
    hp = _ffi.adam()
    a = dict(E=p, ld_e=768, n_total=10, Y=p, dtype=_ffi.TARGET_F32, ld_y=3, n_bags=4, seg_idx=p, seg_rows=8, bag_off=p, bag_idx=p,
             bags=2, N=3, pool=_ffi.MIL_MAX, W=p, b=p, mW=p, vW=p, xW=p, mb=p, vb=p, xb=p, hp=ctypes.byref(hp), t=1, lr=1e-3, loss=p,
             status=p, ws=p, ws_bytes=ws_bytes, z=p, P=p, G=p, dW=p, db=p)
    a.update(change)
    l = _ffi.lib()
    head = (a["E"], a["ld_e"], a["n_total"], a["Y"], a["dtype"], a["ld_y"], a["n_bags"], a["seg_idx"], a["seg_rows"], a["bag_off"],
            a["bag_idx"], a["bags"], a["N"], a["pool"], a["W"], a["b"])
    if grad:
        rc = l.acx_head_fit_grad_mil(*head, a["z"], a["P"], a["G"], a["dW"], a["db"], a["loss"], a["status"], a["ws"], a["ws_bytes"], None)
    else:
        rc = l.acx_head_fit_step_mil(*head, a["mW"], a["vW"], a["xW"], a["mb"], a["vb"], a["xb"], a["hp"], a["t"], a["lr"], a["loss"],
                                     a["status"], a["ws"], a["ws_bytes"], None)
    del keep
    return rc, l.acx_last_error().decode()


def test_abi_argument_checks_return_before_the_device():
    who = "acx_head_fit_step_mil: "
    cases = [({"E": None}, ARG, "E is null"), ({"Y": None}, ARG, "target is null"), ({"seg_idx": None}, ARG, "seg_idx is null"),
             ({"bag_off": None}, ARG, "bag_off is null"), ({"bag_idx": None}, ARG, "bag_idx is null"), ({"W": None}, ARG, "W is null"),
             ({"b": None}, ARG, "b is null"), ({"status": None}, ARG, "status is null"), ({"ws": None}, ARG, "workspace is null"),
             ({"mW": None}, ARG, "moment buffer"), ({"xb": None}, ARG, "vmaxW / vmaxb"), ({"loss": None}, ARG, "loss_out is null"),
             ({"hp": None}, ARG, "hp is null"), ({"bags": 0}, ARG, "bags = 0"), ({"seg_rows": 0}, ARG, "seg_rows = 0"),
             ({"seg_rows": (1 << 22) + 1}, UNSUPPORTED, "seg_rows"), ({"bags": (1 << 22) + 1}, UNSUPPORTED, "bags"),
             ({"pool": 4}, ARG, "pool 4"), ({"pool": -1}, ARG, "pool -1"), ({"N": 0}, ARG, "classes = 0"),
             ({"N": _ffi.MAX_CLASSES + 1}, ARG, "classes"), ({"dtype": 7}, ARG, "target_dtype 7"), ({"n_bags": 0}, ARG, "n_bags_total"),
             ({"n_total": 0}, ARG, "n_rows_total"), ({"ld_e": 767}, ARG, "ld_e"), ({"ld_e": 770}, ARG, "multiple of 4"),
             ({"ld_y": 2}, ARG, "ld_target"), ({"t": 0}, ARG, "step_t"), ({"lr": -1.0}, ARG, "lr"),
             ({"ws_bytes": 16}, WORKSPACE, "workspace of 16 bytes")]
    for change, code, word in cases:
        rc, msg = _abi(**change)
        assert rc == code and msg.startswith(who) and word in msg, (change, rc, msg)
    base = _aligned(1 << 16)
    rc, msg = _abi(E=base[1] + 4)
    assert rc == ARG and "16-byte aligned" in msg
    rc, msg = _abi(ws=base[1] + 64)
    assert rc == WORKSPACE and "256-byte aligned" in msg
    for change, word in (({"z": None}, "output"), ({"P": None}, "output"), ({"G": None}, "output"), ({"dW": None}, "output"),
                         ({"bags": 0}, "bags"), ({"pool": 9}, "pool 9")):
        rc, msg = _abi(grad=True, **change)
        assert rc == ARG and msg.startswith("acx_head_fit_grad_mil: ") and word in msg, (change, rc, msg)
    l = _ffi.lib()
    p = base[1]
    pool = lambda **c: (lambda a: (l.acx_segment_pool(a["z"], a["ld"], a["off"], a["bags"], a["N"], a["pool"], a["out"], a["status"], None),  # noqa: E731
                                   l.acx_last_error().decode()))(dict(dict(z=p, ld=3, off=p, bags=2, N=3, pool=0, out=p, status=p), **c))
    for change, code, word in (({"z": None}, ARG, "logits is null"), ({"off": None}, ARG, "bag_off is null"), ({"out": None}, ARG, "out is null"),
                               ({"status": None}, ARG, "status is null"), ({"bags": 0}, ARG, "bags = 0"), ({"N": 0}, ARG, "classes"),
                               ({"pool": 5}, ARG, "pool 5"), ({"ld": 2}, ARG, "ld = 2"), ({"bags": (1 << 22) + 1}, UNSUPPORTED, "bags")):
        rc, msg = pool(**change)
        assert rc == code and msg.startswith("acx_segment_pool: ") and word in msg, (change, rc, msg)


# ---- 5. the planted-event fit on the host definition ---------------------------------------------------------------------------
def test_planted_events_localise_on_the_host():
    """PLANT (sed_fit_cases.py): heads fitted from clip labels through "max" and "linear" pooling put their arg-max segment inside
    the planted span on held-out clips more often than the clip-level fit -- the same BCE + Adam loop on the bags' mean rows,
    i.e. bags of one row, where every pooling is the identity."""
    xtr, ytr, _, _ = planted(PLANT["train"], PLANT["train_seed"])
    xte, _, start, klass = planted(PLANT["test"], PLANT["test_seed"])
    kw = dict(epochs=PLANT["epochs"], batch_size=PLANT["batch"], lr=PLANT["lr"], seed=PLANT["fit_seed"])
    clip = ft.fit_sed_head_host(xtr.mean(dim=1, keepdim=True), ytr, "max", **kw)
    base = localisation(clip.weight, clip.bias, xte, start, klass)
    assert clip.loss.shape == (PLANT["epochs"] * PLANT["train"] // PLANT["batch"],)
    for pooling in ("max", "linear"):
        fit = ft.fit_sed_head_host(xtr, ytr, pooling, **kw)
        got = localisation(fit.weight, fit.bias, xte, start, klass)
        print("%s: arg-max inside the span %.3f, clip-level fit %.3f, chance %.3f" % (pooling, got, base, 3 / 31))
        assert float(fit.loss[-10:].mean()) < float(fit.loss[:10].mean())
        assert got > base, (pooling, got, base)
