"""GPU (`-m gpu`): sound event detection heads from clip-level labels (pytorch/finetune.py fit_sed_head, ConvNeXt.fit_sed_head,
segments.pool_segments; acx_head_fit_step_mil / acx_head_fit_grad_mil / acx_segment_pool).

The oracle is finetune.mil_grad_host, the float64 closed form that tests/test_sed_fit_cpu.py holds to torch's autograd through
sigmoid -> pooling -> F.binary_cross_entropy.  The bag pass is compared FROM THE DEVICE'S OWN z (its fp32 values, read as float64: the
arg-max decisions of "max" are then the same on both sides, ties included); z itself is compared with float64 from E and W.

Bounds (bag_bounds below), all from float64 quantities, u = 2^-24, gamma(k) = k u / (1 - k u), first order in u with every
first-order relative term required to stay below 2^-10 and the total widened by 1 + 2^-9 for the products of such terms:
  expf, logf, log1pf: 2 ulp = 4 u relative each.
  q = sigmoid(z): expf, one sum, one quotient                             -> |dq| <= 6 u q
  "max"     P = sigmoid(max z)                                            -> |dP| <= 6 u P
  "mean"    S - 1 sums of q, one quotient by S                            -> |dP| <= gamma(S + 6) P
  "linear"  s1 = sum q: gamma(S + 5); s2 = sum q^2: gamma(S + 12) (13 u per term); one quotient
                                                                          -> |dP| <= gamma(2 S + 18) P
  "exp"     e = expf(q): 6 u q + 4 u <= 10 u; s1 = sum e: gamma(S + 9); s2 = sum q e: gamma(S + 16); one quotient
                                                                          -> |dP| <= gamma(2 S + 26) P
  term      y lp + (1 - y) lq with lp = log P: dP / P + 4 u |lp|, lq = log1p(-P): dP / (1 - P) + 4 u |lq|, and 4 u for 1 - y, the
            two products and the sum
  dL/dP     (P - y) / den, den = max(P (1 - P), 1e-12): numerator dP + u |P - y|; den relative dP / P + (dP + u (1 - P)) /
            (1 - P) + u where it is not held at 1e-12 -- the 1 / (1 - P) amplification, carried explicitly; one quotient
  dP/dq     "max" 1; "mean" 1 / S: u; "linear" (2 q - P) / s1: (2 dq + dP + u |2 q - P|) / s1 + |d| gamma(S + 6);
            "exp" e (1 + q - P) / s1: e (dq + dP + u (1 + q) + u |1 + q - P|) / s1 + |d| gamma(S + 21)
  q (1 - q) relative 6 u + (dq + u (1 - q)) / (1 - q) + u
  G         three products and the rounding of 1 / (bags N): 4 u
  loss      the terms' own bounds, plus a sum of depth 6 (lanes) + ceil(items / 256) + 6 + 3 (the update kernel's loss block)
            and two roundings for the scale
  dW, db    (seg_rows + 4) u |G64|^T |E| + dG^T |E|, as tests/test_gpu_finetune.py."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import finetune as ft
from audioset_convnext_inf_amd.pytorch import segments as seg
from audioset_convnext_inf_amd.pytorch._inputs import target_code
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from fit_calls import call_update, fresh_state, last_error, vp
from sed_fit_cases import PLANT, POOLINGS, localisation, planted, random_bags

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DEV = "cuda"
SR = 32000
POOL = ft.MIL_POOLS
WORST = {}                                                                         # quantity -> worst err / bound seen (printed)


def gamma(k):
    return k * U / (1 - k * U)


def note(name, err, bound):
    r = float((err / bound).max()) if torch.is_tensor(err) else err / bound
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


# ---- raw calls -------------------------------------------------------------------------------------------------------------------
def workspace(seg_rows, bags, N):
    nbytes = _ffi.head_fit_mil_workspace_bytes(max(seg_rows, 1), max(bags, 1), N)
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def mil_args(E, Y, seg_idx, bag_off, bag_idx, W, pooling, over=None):
    a = dict(E=vp(E), ld_e=E.stride(0), n_total=E.shape[0], Y=vp(Y), dtype=target_code(Y), ld_y=Y.stride(0), n_bags=Y.shape[0],
             seg_idx=vp(seg_idx), seg_rows=seg_idx.numel(), bag_off=vp(bag_off), bag_idx=vp(bag_idx), bags=bag_idx.numel(),
             N=W.shape[0], pool=POOL[pooling])
    a.update(over or {})
    return a, (a["E"], a["ld_e"], a["n_total"], a["Y"], a["dtype"], a["ld_y"], a["n_bags"], a["seg_idx"], a["seg_rows"], a["bag_off"],
               a["bag_idx"], a["bags"], a["N"], a["pool"])


def call_grad_mil(E, Y, seg_idx, bag_off, bag_idx, W, b, pooling, ws=None, over=None):
    """acx_head_fit_grad_mil on device tensors -> (rc, dict of z P G dW db loss status)."""
    a, head = mil_args(E, Y, seg_idx, bag_off, bag_idx, W, pooling, over)
    rows, bags, N = max(a["seg_rows"], 1), max(a["bags"], 1), W.shape[0]
    nan = float("nan")
    o = dict(z=torch.full((rows, N), nan, device=DEV), P=torch.full((bags, N), nan, device=DEV), G=torch.full((rows, N), nan, device=DEV),
             dW=torch.full((N, 768), nan, device=DEV), db=torch.full((N,), nan, device=DEV), loss=torch.full((1,), nan, device=DEV),
             status=torch.zeros(1, dtype=torch.int32, device=DEV))
    wsb, nbytes = workspace(rows, bags, N) if ws is None else ws
    rc = _ffi.lib().acx_head_fit_grad_mil(*head, vp(W), vp(b), vp(o["z"]), vp(o["P"]), vp(o["G"]), vp(o["dW"]), vp(o["db"]),
                                          vp(o["loss"]), vp(o["status"]), vp(wsb), nbytes, _ffi.stream_ptr(torch.device(DEV)))
    return rc, o


def call_step_mil(E, Y, seg_idx, bag_off, bag_idx, st, pooling, hp, t, lr, loss, status, ws, over=None):
    a, head = mil_args(E, Y, seg_idx, bag_off, bag_idx, st["W"], pooling, over)
    return _ffi.lib().acx_head_fit_step_mil(*head, vp(st["W"]), vp(st["b"]), vp(st["mW"]), vp(st["vW"]), vp(st["xW"]), vp(st["mb"]),
                                            vp(st["vb"]), vp(st["xb"]), ctypes.byref(hp), t, lr, vp(loss), vp(status), vp(ws[0]), ws[1],
                                            _ffi.stream_ptr(torch.device(DEV)))


def call_pool(z, bag_off, pooling, bags=None, N=None):
    bags = bag_off.numel() - 1 if bags is None else bags
    N = z.shape[1] if N is None else N
    out = torch.full((bags, N), float("nan"), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _ffi.lib().acx_segment_pool(vp(z), z.stride(0), vp(bag_off), bags, N, POOL[pooling], vp(out), vp(status),
                                     _ffi.stream_ptr(torch.device(DEV)))
    return rc, out, status


def call_grad_ce(E, idx, W, b):
    """acx_head_fit_grad_ce's z on rows idx (labels all 0: z does not depend on them)."""
    rows, N = idx.numel(), W.shape[0]
    z, G = torch.empty(rows, N, device=DEV), torch.empty(rows, N, device=DEV)
    dW, db, loss = torch.empty(N, 768, device=DEV), torch.empty(N, device=DEV), torch.empty(1, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    labels = torch.zeros(E.shape[0], dtype=torch.int64, device=DEV)
    nbytes = _ffi.head_fit_ce_workspace_bytes(rows, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = _ffi.lib().acx_head_fit_grad_ce(vp(E), E.stride(0), E.shape[0], vp(labels), vp(idx), rows, N, 0.0, vp(W), vp(b), vp(z), vp(G),
                                         vp(dW), vp(db), vp(loss), vp(status), vp(ws), nbytes, _ffi.stream_ptr(torch.device(DEV)))
    assert rc == 0, last_error()
    return z


def on_device(case, u8=False):
    d = {k: v.to(DEV) for k, v in case.items()}
    if u8:
        d["Y"] = d["Y"].to(torch.uint8)
    return d


def run_grad(case, pooling, u8=False, **kw):
    d = on_device(case, u8)
    rc, o = call_grad_mil(d["E"], d["Y"], d["seg_idx"], d["bag_off"], d["bag_idx"], d["W"], d["b"], pooling, **kw)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return d, {k: v.cpu() for k, v in o.items()}


# ---- the bounds of the bag pass (module docstring) -------------------------------------------------------------------------------
def bag_bounds(z, bag_off, y, pooling):
    """z (rows, N) float64 (the device's fp32 logits), y (bags, N) float64 -> the float64 results and their bounds:
    dict(P, dP, G, dG, terms, dterms, tstar)."""
    ref = ft.mil_grad_host(z, bag_off, y, pooling)
    zb, mask, lens = ft._padded_bags(z, bag_off)
    m3 = mask[:, :, None]
    S = lens.clamp(min=1).double()[:, None]                                          # (bags, 1)
    q = torch.sigmoid(zb)
    dq = 6 * U * q
    P = ref.P
    cP = {"max": 6 + 0 * S, "mean": S + 6, "linear": 2 * S + 18, "exp": 2 * S + 26}[pooling]
    dP = gamma(cP) * P
    small = [float(gamma(cP).max())]
    lp, lq = torch.log(P).clamp(min=-100), torch.log1p(-P).clamp(min=-100)
    one_m = (1 - P).clamp(min=1e-300)
    dterms = y * (dP / P.clamp(min=1e-300) + 4 * U * lp.abs()) + (1 - y) * (dP / one_m + 4 * U * lq.abs()) \
        + 4 * U * ((y * lp).abs() + ((1 - y) * lq).abs())
    den = (P * (1 - P)).clamp(min=1e-12)
    held = (P * (1 - P)) < 1e-12
    rel_den = torch.where(held, torch.zeros_like(P), dP / P.clamp(min=1e-300) + (dP + U * (1 - P)) / one_m + U)
    small.append(float(rel_den.max()))
    dLdP = (P - y) / den
    d_dLdP = (dP + U * (P - y).abs()) / den + dLdP.abs() * (rel_den + U)
    dLdP3, d_dLdP3, P3, dP3 = dLdP[:, None, :], d_dLdP[:, None, :], P[:, None, :], dP[:, None, :]
    if pooling == "max":
        d = (torch.arange(zb.shape[1])[None, :, None] == ref.tstar[:, None, :]).double()
        dd = torch.zeros_like(d)
    elif pooling == "mean":
        d = (1 / S)[:, :, None].expand_as(q)
        dd = U * d
    elif pooling == "linear":
        s1 = torch.where(m3, q, torch.zeros_like(q)).sum(dim=1, keepdim=True)
        d = (2 * q - P3) / s1
        dd = (2 * dq + dP3 + U * (2 * q - P3).abs()) / s1 + d.abs() * gamma(S + 6)[:, :, None]
    else:
        e = torch.exp(q)
        s1 = torch.where(m3, e, torch.zeros_like(e)).sum(dim=1, keepdim=True)
        d = e * (1 + q - P3) / s1
        dd = e * (dq + dP3 + U * (1 + q) + U * (1 + q - P3).abs()) / s1 + d.abs() * gamma(S + 21)[:, :, None]
    qq = q * (1 - q)
    rel_qq = 6 * U + (dq + U * (1 - q)) / (1 - q) + U
    small.append(float(rel_qq[m3.expand_as(q)].max()) if bool(mask.any()) else 0.0)
    inv = 1.0 / (P.shape[0] * P.shape[1])
    G = dLdP3 * d * qq * inv
    dG = inv * qq * (d_dLdP3 * d.abs() + dLdP3.abs() * dd) + G.abs() * (rel_qq + 4 * U)
    assert max(small) < 2.0 ** -10, small                                          # first order is the whole story (docstring)
    wide = 1 + 2.0 ** -9
    assert torch.allclose(G[mask], ref.G, rtol=1e-12, atol=1e-300)
    return dict(P=P, dP=dP * wide, G=ref.G, dG=(dG * wide)[mask], terms=ref.terms, dterms=dterms * wide, tstar=ref.tstar, mask=mask)


def check_bag_pass(o, case, pooling, tag):
    """P, G, the loss, dW and db of one acx_head_fit_grad_mil call against float64 from its own z."""
    z = o["z"].double()
    off = case["bag_off"].numpy()
    y = case["Y"].double()[case["bag_idx"]]
    bags, N, rows = y.shape[0], y.shape[1], z.shape[0]
    B = bag_bounds(z, off, y, pooling)
    assert bool(torch.isfinite(o["P"]).all()) and bool(torch.isfinite(o["G"]).all())
    err = (o["P"].double() - B["P"]).abs()
    rP = note("P " + pooling, err, B["dP"].clamp(min=1e-300))
    assert bool((err <= B["dP"]).all()), (tag, "P", rP)
    err = (o["G"].double() - B["G"]).abs()
    ok = err <= B["dG"]
    rG = note("G " + pooling, err[B["dG"] > 0], B["dG"][B["dG"] > 0]) if bool((B["dG"] > 0).any()) else 0.0
    assert bool(ok.all()), (tag, "G", rG)
    items = bags * math.ceil(N / 64)
    depth = 6 + math.ceil(items / 256) + 6 + 3
    bound = float(B["dterms"].mean()) + (depth + 2) * U * float(B["terms"].abs().mean())
    err = abs(float(o["loss"]) - float(B["terms"].mean()))
    rL = note("loss " + pooling, err, bound)
    assert err <= bound, (tag, "loss", err, bound)
    e = case["E"].double()[case["seg_idx"]]
    bound = (rows + 4) * U * (B["G"].abs().T @ e.abs()) + B["dG"].T @ e.abs()
    err = (o["dW"].double() - B["G"].T @ e).abs()
    rW = note("dW " + pooling, err, bound.clamp(min=1e-300))
    assert bool((err <= bound).all()), (tag, "dW", rW)
    bound = (rows + 4) * U * B["G"].abs().sum(0) + B["dG"].sum(0)
    err = (o["db"].double() - B["G"].sum(0)).abs()
    rb = note("db " + pooling, err, bound.clamp(min=1e-300))
    assert bool((err <= bound).all()), (tag, "db", rb)
    print("%s %s: err / bound  P %.3g  G %.3g  loss %.3g  dW %.3g  db %.3g" % (tag, pooling, rP, rG, rL, rW, rb))
    return B


def device_tstar(G, mask_off, bags):
    """The row of each (bag, class) that carries the gradient of a "max" pass, from G: exactly one non-zero per column and bag."""
    out = []
    for i in range(bags):
        g = G[mask_off[i]:mask_off[i + 1]]
        assert bool(((g != 0).sum(0) == 1).all()), i
        out.append((g != 0).double().argmax(0))
    return torch.stack(out)


# ---- 1. logits, pooled probabilities, gradient and loss ------------------------------------------------------------------------
SHAPES = {  # name: (bag lengths, N, u8)
    "N1_one_bag": ([5], 1, True),
    "N50_three": ([1, 2, 31], 50, False),
    "N64_ragged_1_70": ([1, 70, 1, 1, 70, 1, 70], 64, True),
    "N65_bags67": ([2, 1, 3] * 22 + [63], 65, False),
    "N527_bags64": ([31] * 63 + [2], 527, True),
    "N527_long": ([313, 63], 527, False),
}


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradient_against_float64(shape, pooling):
    """One acx_head_fit_grad_mil call per shape and pooling: z torch.equal to acx_head_fit_grad_ce's z on idx = seg_idx and within
    768 u |E||W|^T + u |b| of float64; P torch.equal to acx_segment_pool on that z; P, G, loss, dW, db within bag_bounds from the
    device's own z; |z| <= 10; soft targets on the f32 cases."""
    lens, N, u8 = SHAPES[shape]
    case = random_bags(lens, N, seed=sum(lens) + N, soft=not u8)
    rows = sum(lens)
    assert rows % 16 != 0 and rows % 32 != 0
    d, o = run_grad(case, pooling, u8)
    assert int(o["status"]) == 0
    assert torch.equal(o["z"], call_grad_ce(d["E"], d["seg_idx"], d["W"], d["b"]).cpu())
    e = case["E"].double()[case["seg_idx"]]
    z64 = e @ case["W"].double().T + case["b"].double()
    dz = 768 * U * (e.abs() @ case["W"].double().abs().T) + U * case["b"].double().abs()
    assert float(z64.abs().max()) <= 10 and bool(((o["z"].double() - z64).abs() <= dz).all())
    rc, pooled, status = call_pool(o["z"].to(DEV), d["bag_off"], pooling)
    assert rc == 0, last_error()
    assert torch.equal(pooled.cpu(), o["P"]) and int(status) == 0
    check_bag_pass(o, case, pooling, shape)
    again = run_grad(case, pooling, u8)[1]
    for k in o:
        assert torch.equal(o[k], again[k]), k                                      # the same inputs, the same bits


def test_max_picks_the_float64_row():
    """Random inputs: wherever the float64 top-two margin of a (bag, class) exceeds twice the z bound, the row that carries the
    gradient is the float64 arg-max; at most 1 % of the pairs may be exempt.  No row repeats (a repeat is an exact tie): 3 of the
    1 150 pairs of this seed are exempt."""
    lens, N = [31] * 20 + [70, 3, 2], 50
    case = random_bags(lens, N, seed=77)
    case["seg_idx"] = torch.randperm(case["E"].shape[0], generator=torch.Generator().manual_seed(1))[:sum(lens)]
    d, o = run_grad(case, "max")
    off = case["bag_off"].tolist()
    e = case["E"].double()[case["seg_idx"]]
    z64 = e @ case["W"].double().T + case["b"].double()
    dz = 768 * U * (e.abs() @ case["W"].double().abs().T) + U * case["b"].double().abs()
    got = device_tstar(o["G"], off, len(lens))
    exempt = 0
    for i in range(len(lens)):
        zz, bb = z64[off[i]:off[i + 1]], dz[off[i]:off[i + 1]]
        top = zz.topk(2, dim=0)
        clear = (top.values[0] - top.values[1]) > 2 * bb.max(0).values
        exempt += int((~clear).sum())
        assert bool((got[i][clear] == top.indices[0][clear]).all()), i
    print("exempt %d of %d pairs" % (exempt, len(lens) * N))
    assert exempt <= 0.01 * len(lens) * N


def integer_case(seed=5):
    """E, W, b of small integers (z exact in fp32 and in float64), bags whose seg_idx repeats rows: exact ties."""
    g = torch.Generator().manual_seed(seed)
    n_total, N = 40, 65
    E = torch.zeros(n_total, 768)
    for r in range(n_total):
        E[r, torch.randperm(768, generator=g)[:6]] = torch.randint(-1, 2, (6,), generator=g).float()
    W = torch.randint(-1, 2, (N, 768), generator=g).float()
    b = torch.randint(-2, 3, (N,), generator=g).float()
    lens = [9, 1, 17, 4]
    seg_idx = torch.randint(0, n_total, (sum(lens),), generator=g)
    seg_idx[3], seg_idx[7] = seg_idx[0], seg_idx[0]                                 # bag 0 holds one row three times
    seg_idx[12:20] = seg_idx[11]                                                   # bag 2 opens with nine copies of one row
    Y = (torch.rand(6, N, generator=g) < 0.5).float()
    return dict(E=E, W=W, b=b, Y=Y, seg_idx=seg_idx, bag_idx=torch.tensor([0, 5, 2, 0]),
                bag_off=torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))), lens


def test_exact_logits_give_the_host_rows_everywhere():
    case, lens = integer_case()
    d, o = run_grad(case, "max")
    z64 = case["E"].double()[case["seg_idx"]] @ case["W"].double().T + case["b"].double()
    assert torch.equal(o["z"].double(), z64) and float(z64.abs().max()) <= 8
    ref = ft.mil_grad_host(z64, case["bag_off"].numpy(), case["Y"].double()[case["bag_idx"]], "max")
    got = device_tstar(o["G"], case["bag_off"].tolist(), len(lens))
    assert torch.equal(got, ref.tstar)
    ties = sum(int(((z64[a:b] == z64[a:b].max(0).values).sum(0) > 1).sum()) for a, b in zip(case["bag_off"][:-1], case["bag_off"][1:]))
    assert ties > 20                                                               # the case does hold ties
    for pooling in POOLINGS:
        check_bag_pass(run_grad(case, pooling)[1], case, pooling, "integers")


# ---- 2. saturation ----------------------------------------------------------------------------------------------------------------
def test_saturated_logits():
    """z = +-40 (class 0) and +-110 (class 1), exact: E[t, 0] = +-1, W[c, 0] = 40 / 110, b = 0.  Six bags of five rows -- all +,
    all -, mixed (+ - - + -) -- with targets 0 (bags 0 .. 2) and 1 (bags 3 .. 5).  In fp32 sigmoid(40) = sigmoid(110) = 1 and
    sigmoid(-110) = 0 exactly, sigmoid(-40) = e^-40.  Stated values:
      all +     P = 1 for every pooling; P (1 - P) = 0 is held at 1e-12 and q (1 - q) = 0: G = 0; term 100 at y = 0 (log1p(-1) = -inf,
                held at -100), 0 at y = 1
      all -110  every q = 0: sum q = 0, P = 0, G = 0; term 100 at y = 1 (log 0 held), 0 at y = 0
      +-110     every q is 0 or 1: G = 0 whatever the pooling
    Every output is finite, and the loss is the mean of the float64 terms of the same z: a term's relative error is at most
    (c_P + 4 * 100 + 4) u (its logarithm is at most 100 in size), the sum's depth 18."""
    S = 5
    signs = torch.tensor([1.0] * S + [-1.0] * S + [1.0, -1.0, -1.0, 1.0, -1.0]).repeat(2)
    E = torch.zeros(6 * S, 768)
    E[:, 0] = signs
    W = torch.zeros(2, 768)
    W[0, 0], W[1, 0] = 40.0, 110.0
    Y = torch.tensor([[0.0, 0.0], [1.0, 1.0]])
    case = dict(E=E, W=W, b=torch.zeros(2), Y=Y, seg_idx=torch.arange(6 * S), bag_idx=torch.tensor([0, 0, 0, 1, 1, 1]),
                bag_off=torch.arange(7, dtype=torch.int32) * S)
    for pooling in POOLINGS:
        d, o = run_grad(case, pooling)
        assert int(o["status"]) == 0
        for k in ("z", "P", "G", "dW", "db", "loss"):
            assert bool(torch.isfinite(o[k]).all()), (pooling, k)
        assert torch.equal(o["z"][:, 0], signs * 40) and torch.equal(o["z"][:, 1], signs * 110)
        P, G = o["P"], o["G"]
        assert P[0].tolist() == [1.0, 1.0] and P[3].tolist() == [1.0, 1.0]          # all +
        assert float(P[1, 1]) == 0.0 and float(P[4, 1]) == 0.0                      # all -110: sum q = 0
        assert 0.0 < float(P[1, 0]) < 1e-17 and 0.0 < float(P[4, 0]) < 1e-17        # all -40: e^-40
        assert bool((G[:S] == 0).all()) and bool((G[3 * S:4 * S] == 0).all())       # all +: q (1 - q) = 0
        assert bool((G[:, 1] == 0).all())                                           # +-110: every q is 0 or 1
        ref = ft.mil_grad_host(o["z"].double(), case["bag_off"].numpy(), Y.double()[case["bag_idx"]], pooling)
        assert ref.terms[0].tolist() == [100.0, 100.0] and ref.terms[3].tolist() == [0.0, 0.0] and float(ref.terms[4, 1]) == 100.0
        cP = {"max": 6, "mean": S + 6, "linear": 2 * S + 18, "exp": 2 * S + 26}[pooling]
        bound = (cP + 404 + 18) * U * float(ref.terms.mean())
        err = abs(float(o["loss"]) - float(ref.terms.mean()))
        print("%s: loss %.6f, err / bound %.3g" % (pooling, float(o["loss"]), err / bound))
        assert err <= bound, (pooling, float(o["loss"]), float(ref.terms.mean()))
    # bags of -40 alone: P (1 - P) = e^-40 is held at 1e-12, nothing else saturates, and the whole pass obeys bag_bounds
    low = dict(E=-E[:2 * S].abs(), W=W[:1], b=torch.zeros(1), Y=Y[:, :1], seg_idx=torch.arange(2 * S), bag_idx=torch.tensor([0, 1]),
               bag_off=torch.tensor([0, S, 2 * S], dtype=torch.int32))
    for pooling in POOLINGS:
        d, o = run_grad(low, pooling)
        assert bool((o["z"] == -40).all())
        assert bool((o["G"] != 0).all()) if pooling != "max" else (o["G"] != 0).sum() == 2     # tiny, not flushed away
        B = check_bag_pass(o, low, pooling, "z = -40")
        assert abs(float(B["terms"][1, 0]) - 40.0) < 1e-9


# ---- 3. data errors ---------------------------------------------------------------------------------------------------------------
def guarded(case):
    """E and the targets as the middle slices of larger NaN-filled buffers: an index that escaped the clamp would read NaN, not
    fault."""
    n, nb, N = case["E"].shape[0], case["Y"].shape[0], case["Y"].shape[1]
    big = torch.full((3 * n, 768), float("nan"), device=DEV)
    bigy = torch.full((3 * nb, N), float("nan"), device=DEV)
    big[n:2 * n], bigy[nb:2 * nb] = case["E"].to(DEV), case["Y"].to(DEV)
    return big[n:2 * n], bigy[nb:2 * nb]


def grad_with(case, Ed, Yd, pooling="linear", **change):
    c = {k: v.to(DEV) for k, v in dict(case, **change).items()}
    rc, o = call_grad_mil(Ed, Yd, c["seg_idx"], c["bag_off"], c["bag_idx"], c["W"], c["b"], pooling)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def test_bad_indices_and_offsets_are_clamped_and_flagged():
    lens = [4, 0, 7, 3, 5]
    case = random_bags(lens, 10, seed=9)
    Ed, Yd = guarded(case)
    n, nb, rows = case["E"].shape[0], case["Y"].shape[0], sum(lens)
    good = grad_with(case, Ed, Yd)
    assert int(good["status"]) == 0 and bool((good["P"][1] == 0).all())            # the empty bag is no error
    check_bag_pass(good, case, "linear", "empty bag")

    def same(a, b):
        return all(torch.equal(a[k], b[k]) for k in ("z", "P", "G", "dW", "db", "loss"))

    si = case["seg_idx"].clone()
    si[2], si[11] = -1, n
    sc = si.clone()
    sc[2], sc[11] = 0, n - 1
    bad, clamped = grad_with(case, Ed, Yd, seg_idx=si), grad_with(case, Ed, Yd, seg_idx=sc)
    assert int(bad["status"]) == _ffi.FIT_BAD_INDEX and int(clamped["status"]) == 0 and same(bad, clamped)
    bi = case["bag_idx"].clone()
    bi[0], bi[3] = nb + 3, -7
    bc = bi.clone()
    bc[0], bc[3] = nb - 1, 0
    bad, clamped = grad_with(case, Ed, Yd, bag_idx=bi), grad_with(case, Ed, Yd, bag_idx=bc)
    assert int(bad["status"]) == _ffi.FIT_BAD_INDEX and int(clamped["status"]) == 0 and same(bad, clamped)
    # offsets: a decreasing entry empties its bag, entries beyond seg_rows / below 0 are held inside, the ends are 0 and seg_rows
    for off, held in (([0, 4, 2, 11, 14, rows], [0, 4, 4, 11, 14, rows]), ([0, 4, 4, 11, rows + 9, rows], [0, 4, 4, 11, rows, rows]),
                      ([-3, 4, 4, 11, 14, rows], [0, 4, 4, 11, 14, rows]), ([0, 4, 4, 11, 14, rows - 2], [0, 4, 4, 11, 14, rows]),
                      ([0, 4, 4, 11, 14, rows + 100], [0, 4, 4, 11, 14, rows])):
        bad = grad_with(case, Ed, Yd, bag_off=torch.tensor(off, dtype=torch.int32))
        assert int(bad["status"]) == _ffi.FIT_BAD_BAG, off
        for k in ("z", "P", "G", "dW", "db", "loss"):
            assert bool(torch.isfinite(bad[k]).all()), (off, k)
        if off[2] >= off[1]:                                                       # (overlapping bags write rows twice: no one answer)
            clamped = grad_with(case, Ed, Yd, bag_off=torch.tensor(held, dtype=torch.int32))
            assert int(clamped["status"]) == 0 and same(bad, clamped), off
    # the fused step flags as well and stays finite
    st = fresh_state(case["W"], case["b"])
    loss, status = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = call_step_mil(Ed, Yd, si.to(DEV), torch.tensor([0, 4, 2, 11, 14, rows], dtype=torch.int32, device=DEV), bi.to(DEV), st, "max",
                       _ffi.adam(), 1, 1e-3, loss, status, workspace(rows, len(lens), 10))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert int(status) == _ffi.FIT_BAD_INDEX | _ffi.FIT_BAD_BAG
    assert bool(torch.isfinite(st["W"]).all()) and bool(torch.isfinite(loss).all())
    # acx_segment_pool: decreasing and negative entries
    z = good["z"].to(DEV)
    rc, out, status = call_pool(z, torch.tensor([0, 4, 2, 11, 14, rows], dtype=torch.int32, device=DEV), "mean")
    rc2, want, status2 = call_pool(z, torch.tensor([0, 4, 4, 11, 14, rows], dtype=torch.int32, device=DEV), "mean")
    assert rc == 0 and rc2 == 0
    assert int(status) == _ffi.FIT_BAD_BAG and int(status2) == 0 and bool(torch.isfinite(out).all())
    assert torch.equal(out[3:], want[3:]) and torch.equal(out[0], want[0]) and bool((out[1] == 0).all())    # bag 2 starts at row 2


# ---- 4. the fused step leaves the bits of its components -----------------------------------------------------------------------
@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("mode", ["adam_ams", "adam", "adamw_ams", "adamw"])
def test_step_equals_grad_then_update(mode, pooling):
    lens, N = [31, 1, 70, 2, 5, 3, 31, 7, 1], 50
    case = random_bags(lens, N, seed=21)
    d = on_device(case, u8=True)
    amsgrad, decoupled = mode.endswith("ams"), mode.startswith("adamw")
    hp = _ffi.adam(0.9, 0.999, 1e-8, 0.01, amsgrad, decoupled)
    a, b = fresh_state(case["W"], case["b"]), fresh_state(case["W"], case["b"])
    ws = workspace(sum(lens), len(lens), N)
    loss_a, status = torch.zeros(2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in (1, 2):
        st = dict(a) if amsgrad else {**a, "xW": None, "xb": None}
        rc = call_step_mil(d["E"], d["Y"], d["seg_idx"], d["bag_off"], d["bag_idx"], st, pooling, hp, t, 1e-3, loss_a[t - 1:], status, ws)
        assert rc == 0, last_error()
        rc, o = call_grad_mil(d["E"], d["Y"], d["seg_idx"], d["bag_off"], d["bag_idx"], b["W"], b["b"], pooling, ws=ws)
        assert rc == 0, last_error()
        assert call_update(b["W"], o["dW"], b["mW"], b["vW"], b["xW"] if amsgrad else None, hp, t, 1e-3) == 0, last_error()
        assert call_update(b["b"], o["db"], b["mb"], b["vb"], b["xb"] if amsgrad else None, hp, t, 1e-3) == 0, last_error()
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (mode, pooling, t, k)
        assert torch.equal(loss_a[t - 1:t], o["loss"]), (mode, pooling, t)
    assert int(status) == 0 and not torch.equal(a["W"].cpu(), case["W"])


def test_captured_step_replays_the_eager_bits():
    lens, N = [31] * 12 + [5, 70], 50
    case = random_bags(lens, N, seed=23)
    d = on_device(case)
    st, keep = fresh_state(case["W"], case["b"]), fresh_state(case["W"], case["b"])
    hp = _ffi.adam()
    ws = workspace(sum(lens), len(lens), N)
    loss, status = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    args = (d["E"], d["Y"], d["seg_idx"], d["bag_off"], d["bag_idx"], st, "linear", hp, 1, 1e-3, loss, status, ws)
    assert call_step_mil(*args) == 0, last_error()
    torch.cuda.synchronize()
    eager, eager_loss = {k: v.clone() for k, v in st.items()}, loss.clone()
    for k in st:
        st[k].copy_(keep[k])
    loss.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                   # a linear graph: three kernels in a row
        rc = call_step_mil(*args)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(st["W"], keep["W"])                                          # capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(st[k], eager[k]), k
    assert torch.equal(loss, eager_loss) and int(status) == 0


# ---- 5. fits ------------------------------------------------------------------------------------------------------------------------
def weak_data(n, N, seed=0):
    """Ragged clips of 1 .. 12 segments; a positive class adds its prototype to a run of segments."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(N, 768, generator=g)
    lens = torch.randint(1, 13, (n,), generator=g).tolist()
    y = torch.rand(n, N, generator=g) < 0.15
    clips = []
    for i, S in enumerate(lens):
        x = torch.randn(S, 768, generator=g)
        for c in torch.nonzero(y[i]).flatten().tolist():
            a = int(torch.randint(0, S, (1,), generator=g))
            x[a:a + 3] += 0.7 * proto[c]
        clips.append(F.layer_norm(x, (768,)))
    return clips, y.float()


@pytest.mark.parametrize("pooling", POOLINGS)
def test_trajectory_against_the_host_fit(pooling):
    """fit_sed_head against fit_sed_head_host in float64 over 40 steps (160 ragged clips, 10 classes, batches of 32 clips):
    max|W - W64| <= max(8 floor, steps u max|W64|) with floor = max|W32 - W64| of the host definition run in float32 -- the
    trajectory bound of tests/test_gpu_finetune.py -- and the same for b and the step losses.  The floor is taken over TWO float32
    evaluations of the host definition, autograd and the closed form (closed_form=True; in float64 the two agree to 1e-16): Adam
    divides by sqrt(v), so an element of dW whose terms nearly cancel turns u-sized errors of G into a relative error of 5e-3
    of its step, and how far a float32 run strays depends on where its roundings fall -- on the host alone the two evaluations
    stray 2.5e-8 and 2.1e-7 from float64 for "exp" (W), 2.5e-8 and 3.6e-8 for "linear".  "max" is not continuous in z: a
    run whose arg-max differs in one (bag, class) of one step follows another trajectory.  Its case is 24 steps of 4 clips and 2
    classes (192 maxima), seeded so that the float64 run's smallest top-two margin (1.5e-3) exceeds twice the largest z bound of the
    run (768 u |E||W|^T + u |b|: 9.6e-4; the drift of W the bound below allows is four orders smaller): no arg-max can differ."""
    clips, y = weak_data(160, 10) if pooling != "max" else weak_data(24, 2, seed=1)
    kw = dict(epochs=8, batch_size=32, lr=1e-3, seed=2) if pooling != "max" else dict(epochs=4, batch_size=4, lr=1e-3, seed=2)
    gaps, dzs = [], []

    def watch(t, z, off, e, W, b):
        for lo, hi in zip(off[:-1], off[1:]):
            if hi - lo > 1:
                top = z[lo:hi].topk(2, dim=0).values
                gaps.append(float((top[0] - top[1]).min()))
        dzs.append(float((768 * U * (e.abs() @ W.abs().T) + U * b.abs()).max()))
    r64 = ft.fit_sed_head_host(clips, y, pooling, on_step=watch if pooling == "max" else None, **kw)
    r32 = ft.fit_sed_head_host(clips, y, pooling, dtype=torch.float32, **kw)
    c32 = ft.fit_sed_head_host(clips, y, pooling, dtype=torch.float32, closed_form=True, **kw)
    if pooling == "max":
        print("smallest top-two margin %.3g, twice the largest z bound %.3g" % (min(gaps), 2 * max(dzs)))
        assert min(gaps) > 2 * max(dzs)
    fit = ft.fit_sed_head([c.to(DEV) for c in clips], y.to(DEV), pooling, **kw)
    torch.cuda.synchronize()
    steps = r64.loss.numel()
    assert steps == (24 if pooling == "max" else 40) and fit.loss.shape == (steps,) and len(fit.history) == kw["epochs"]
    for name, got, a, fl in (("W", fit.weight, r64.weight, (r32.weight, c32.weight)), ("b", fit.bias, r64.bias, (r32.bias, c32.bias)),
                             ("loss", fit.loss, r64.loss, (r32.loss, c32.loss))):
        floor = max(float((b.double() - a).abs().max()) for b in fl)
        bound = max(8 * floor, steps * U * float(a.abs().max()))
        err = float((got.double().cpu() - a).abs().max())
        note("fit %s %s" % (name, pooling), err, bound)
        print("%s %s: max|gpu - f64| %.3g, host f32 floor %.3g, bound %.3g" % (pooling, name, err, floor, bound))
        assert err <= bound, (pooling, name, err, bound)
    assert float(r64.loss[-5:].mean()) < float(r64.loss[:5].mean())
    again = ft.fit_sed_head((torch.cat(clips).to(DEV), [c.shape[0] for c in clips]), y.to(DEV).bool(), pooling, **kw)
    assert torch.equal(again.weight, fit.weight) and torch.equal(again.loss, fit.loss)      # the packed form, bool targets: the same fit


def test_validation_history_pools_the_clips():
    clips, y = weak_data(96, 6)
    vclips, vy = weak_data(40, 6, seed=1)
    to = lambda cs: [c.to(DEV) for c in cs]                                          # noqa: E731
    kw = dict(batch_size=32, lr=3e-3, seed=1)
    fit = ft.fit_sed_head(to(clips), y.to(DEV), "linear", epochs=2, val=(to(vclips), vy.to(DEV)), **kw)
    part = ft.fit_sed_head(to(clips), y.to(DEV), "linear", epochs=2, **kw)
    assert torch.equal(part.weight, fit.weight)
    from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics
    packed = torch.cat(vclips).to(DEV)
    probs = seg.pool_segments(torch.addmm(fit.bias, packed, fit.weight.t()), "linear", steps=[c.shape[0] for c in vclips])
    stats = tagging_metrics(vy.to(DEV), probs)
    assert np.array_equal(fit.history[1]["average_precision"], stats["average_precision"])
    assert fit.history[1]["mAP"] == float(np.mean(stats["average_precision"]))
    host = seg.pool_segments_host(torch.addmm(fit.bias, packed, fit.weight.t()).cpu(), "linear", steps=[c.shape[0] for c in vclips])
    S = max(c.shape[0] for c in vclips)
    assert bool(((probs.double().cpu() - host).abs() <= gamma(2 * S + 18) * host).all())


def test_planted_events_localise_on_the_device():
    """sed_fit_cases.PLANT, as tests/test_sed_fit_cpu.py runs it on the host definition: the heads fitted on the device through "max"
    and "linear" pooling localise held-out events more often than the clip-level fit (bags of one mean row)."""
    xtr, ytr, _, _ = planted(PLANT["train"], PLANT["train_seed"])
    xte, _, start, klass = planted(PLANT["test"], PLANT["test_seed"])
    kw = dict(epochs=PLANT["epochs"], batch_size=PLANT["batch"], lr=PLANT["lr"], seed=PLANT["fit_seed"])
    xd, yd = xtr.to(DEV), ytr.to(DEV)
    clip = ft.fit_sed_head(xd.mean(dim=1, keepdim=True), yd, "max", **kw)
    base = localisation(clip.weight, clip.bias, xte, start, klass)
    for pooling in ("max", "linear"):
        fit = ft.fit_sed_head(xd, yd, pooling, **kw)
        got = localisation(fit.weight, fit.bias, xte, start, klass)
        print("%s: arg-max inside the span %.3f, clip-level fit %.3f, chance %.3f" % (pooling, got, base, 3 / 31))
        assert got > base, (pooling, got, base)


def test_model_fit_sed_head(synth_sd):
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    model.load_state_dict(synth_sd)
    model = model.to(DEV).eval()
    N = 3
    lens = [SR, 10 * SR, SR, 10 * SR, SR + 4000, 10 * SR]
    waves = [synth.synth_waveforms(1, L, seed=30 + i)[0] for i, L in enumerate(lens)]
    target = torch.tensor([[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [0, 1, 1], [1, 0, 1]], dtype=torch.bool)
    kw = dict(epochs=3, batch_size=4, lr=1e-2, seed=4)
    with torch.no_grad():
        segs = [s.clone() for s in model.forward_varlen([w.to(DEV) for w in waves], what="segment_embeddings", pool=3)]
    assert [s.shape[0] for s in segs] == [seg.segment_count(L) for L in lens]
    want = ft.fit_sed_head(segs, target.to(DEV), "linear", **kw)
    fit = model.fit_sed_head(waves, target, pooling="linear", pool=3, **kw)
    for a, b in ((fit.weight, want.weight), (fit.bias, want.bias), (fit.loss, want.loss)):
        assert torch.equal(a, b)
    assert not model.training and model.head_audioset.out_features == N
    assert torch.equal(model.head_audioset.weight.data, fit.weight) and torch.equal(model.head_audioset.bias.data, fit.bias)
    w64, b64 = fit.weight.double().cpu(), fit.bias.double().cpu()
    for L in (SR, 10 * SR):
        x = synth.synth_waveforms(2, L, seed=50).to(DEV)
        with torch.no_grad():
            out = model.forward_segments(x, pool=3)
            emb = model.forward_segment_embeddings(x, pool=3)
        e = emb.double().cpu()
        bound = 768 * U * (e.abs() @ w64.abs().T) + U * b64.abs()
        assert out["segmentwise_logits"].shape == (2, seg.segment_count(L), N)
        assert bool(((out["segmentwise_logits"].double().cpu() - (e @ w64.T + b64)).abs() <= bound).all()), L
        # "max" pooling is forward_segments' clip output: two fp32 sigmoids of the same logit, 6 u each
        pooled = seg.pool_segments(out["segmentwise_logits"], "max")
        assert bool(((pooled - out["clipwise_output"]).abs() <= 12 * U * pooled).all())
    # a uniform batch of waveforms, and embeddings handed over directly
    xb = synth.synth_waveforms(4, SR, seed=60)
    f2 = model.fit_sed_head(xb, target[:4], pooling="max", epochs=1, batch_size=4)
    with torch.no_grad():
        e2 = model.forward_segment_embeddings(xb.to(DEV), pool=3)
    f3 = model.fit_sed_head(e2, target[:4], pooling="max", epochs=1, batch_size=4)
    assert torch.equal(f2.weight, f3.weight)
    with pytest.raises(ValueError, match="pooling"):
        model.fit_sed_head(xb, target[:4], pooling="softmax")


def test_worst_ratios_are_printed():
    """Runs last: the worst err / bound of every quantity over the cases above (the README's results row quotes them)."""
    for k in sorted(WORST):
        print("worst err / bound  %-16s %.3g" % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())
