"""GPU (`-m gpu`): fitting a classifier head on frozen scene embeddings (pytorch/finetune.py fit_head, ConvNeXt.fit_head,
acx_head_fit_step / acx_head_fit_grad / acx_adam_update).

The oracle is torch itself on the CPU: sigmoid(E W^T + b), F.binary_cross_entropy, torch.optim.Adam / AdamW, batches cut from
torch.randperm(n, generator=manual_seed(seed)) drawn once per epoch -- in float64 (the reference) and in float32 (its own
rounding floor).  Every bound below is computed from float64 quantities; u = 2^-24 is the float32 unit roundoff.

The float64 evaluation of one optimiser step (test 2) takes the scalars that depend only on the hyper-parameters and the step
number -- beta, 1 - beta, eps, lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - lr wd -- as the library defines them: evaluated in
double, rounded to float32 once (include/acx.h)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch.convnext import ConvNeXt, convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract
from audioset_convnext_inf_amd.pytorch._inputs import target_code
from audioset_convnext_inf_amd.pytorch.finetune import fit_head
from audioset_convnext_inf_amd.pytorch.metrics import tagging_metrics
from fit_calls import call_update, fresh_state, init, last_error, vp

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SR = 32000
DEV = "cuda"


def data(n, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(N, 768, generator=g)
    y = torch.rand(n, N, generator=g) < 0.06
    y[torch.arange(n), torch.randint(0, N, (n,), generator=g)] = True
    x = y.float() @ proto * 0.7 + torch.randn(n, 768, generator=g)
    return F.layer_norm(x, (768,)), y.float()


def oracle(E, Y, W0, b0, batch, epochs, lr, dtype, seed=2, adamw=False, wd=0.0, amsgrad=True):
    """The reference loop on the CPU -> (W, b, losses (steps,), max |z| seen)."""
    E, Y = E.to(dtype), Y.to(dtype)
    W, b = W0.to(dtype).clone().requires_grad_(), b0.to(dtype).clone().requires_grad_()
    lr0 = lr if isinstance(lr, float) else lr[0]
    opt = (torch.optim.AdamW if adamw else torch.optim.Adam)([W, b], lr=lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd,
                                                             amsgrad=amsgrad)
    g = torch.Generator().manual_seed(seed)
    losses, zmax, t = [], 0.0, 0
    for _ in range(epochs):
        perm = torch.randperm(E.shape[0], generator=g)
        for s in range(0, E.shape[0], batch):
            i = perm[s:s + batch]
            if not isinstance(lr, float):
                opt.param_groups[0]["lr"] = lr[t]
            z = E[i] @ W.T + b
            loss = F.binary_cross_entropy(torch.sigmoid(z), Y[i])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            zmax = max(zmax, float(z.detach().abs().max()))
            t += 1
    return W.detach(), b.detach(), torch.stack(losses), zmax


def workspace(rows, N):
    nbytes = _ffi.head_fit_workspace_bytes(rows, N)
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def call_grad(E, Y, idx, W, b, n_total=None, rows=None, N=None, ws=None, over=None):
    """acx_head_fit_grad on device tensors -> (rc, z, G, dW, db, loss, status)."""
    N = W.shape[0] if N is None else N
    rows = idx.numel() if rows is None else rows
    z = torch.full((max(rows, 1), W.shape[0]), float("nan"), device=DEV)
    G = torch.full_like(z, float("nan"))
    dW, db = torch.full((W.shape[0], 768), float("nan"), device=DEV), torch.full((W.shape[0],), float("nan"), device=DEV)
    loss, status = torch.full((1,), float("nan"), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    wsb, nbytes = workspace(max(rows, 1), W.shape[0]) if ws is None else ws
    a = dict(E=vp(E), ld_e=E.stride(0), n_total=E.shape[0] if n_total is None else n_total, Y=vp(Y),
             dtype=target_code(Y), ld_y=Y.stride(0), idx=vp(idx), rows=rows, N=N,
             W=vp(W), b=vp(b), z=vp(z), G=vp(G), dW=vp(dW), db=vp(db), loss=vp(loss), status=vp(status), ws=vp(wsb),
             ws_bytes=nbytes)
    a.update(over or {})
    rc = _ffi.lib().acx_head_fit_grad(a["E"], a["ld_e"], a["n_total"], a["Y"], a["dtype"], a["ld_y"], a["idx"], a["rows"], a["N"],
                                      a["W"], a["b"], a["z"], a["G"], a["dW"], a["db"], a["loss"], a["status"], a["ws"],
                                      a["ws_bytes"], _ffi.stream_ptr(torch.device(DEV)))
    return rc, z, G, dW, db, loss, status


def call_step(E, Y, idx, st, hp, t, lr, loss, status, ws, stream=None, over=None):
    """acx_head_fit_step; st: dict of W b mW vW xW mb vb xb device tensors."""
    a = dict(E=vp(E), ld_e=E.stride(0), n_total=E.shape[0], Y=vp(Y),
             dtype=target_code(Y), ld_y=Y.stride(0), idx=vp(idx), rows=idx.numel(),
             N=st["W"].shape[0], hp=ctypes.byref(hp) if hp is not None else None, t=t, lr=lr, loss=vp(loss), status=vp(status),
             ws=vp(ws[0]), ws_bytes=ws[1])
    a.update({k: vp(v) for k, v in st.items()})
    a.update(over or {})
    return _ffi.lib().acx_head_fit_step(a["E"], a["ld_e"], a["n_total"], a["Y"], a["dtype"], a["ld_y"], a["idx"], a["rows"], a["N"],
                                        a["W"], a["b"], a["mW"], a["vW"], a["xW"], a["mb"], a["vb"], a["xb"], a["hp"], a["t"],
                                        a["lr"], a["loss"], a["status"], a["ws"], a["ws_bytes"],
                                        stream if stream is not None else _ffi.stream_ptr(torch.device(DEV)))


# ---- 1. the gradient pass against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("N", [1, 10, 50, 527, 4096])
def test_gradient_against_float64(N, u8):
    """z, G, dW, db and the loss of acx_head_fit_grad against float64, rows in {1, 7, 64, 208, 1000}, shuffled idx with
    repeats, row strides larger than the rows.  Bounds: |z - z64| <= 768 u |E||W|^T + u |b| =: dz (test_head_independence);
    G = (sigmoid(z) - y) / (rows N) with sigmoid' <= 1/4 moves by at most dG = dz / (4 rows N), plus 4 u / (rows N) for the
    fp32 evaluation of p <= 1, the subtraction and the scaling; |dW - dW64| <= (rows + 4) u |G64|^T|E| + dG'^T |E| with dG' the
    whole G bound, the same for db; the loss moves by at most mean(dz) (|dl/dz| = |p - y| <= 1) plus (D + 8) u mean|l64| for a
    sum of depth D = 64 + tiles / 256 and the fp32 evaluation of each term."""
    n_total = 1200
    g = torch.Generator().manual_seed(40 + N)
    buf = torch.randn(n_total, 772, generator=g)
    E = F.layer_norm(buf[:, :768], (768,))
    buf[:, :768] = E
    W, b = torch.randn(N, 768, generator=g) * 0.05, torch.randn(N, generator=g) * 0.1
    ybuf = torch.zeros(n_total, N + 3, dtype=torch.uint8 if u8 else torch.float32)
    ybuf[:, :N] = (torch.rand(n_total, N, generator=g) < 0.2).to(ybuf.dtype) if u8 else torch.rand(n_total, N, generator=g)
    Ed, Yd, Wd, bd = buf.to(DEV)[:, :768], ybuf.to(DEV)[:, :N], W.to(DEV), b.to(DEV)
    assert Ed.stride(0) == 772 and Yd.stride(0) == N + 3
    E64, W64, b64, Y64 = E.double(), W.double(), b.double(), ybuf[:, :N].double()
    for rows in (1, 7, 64, 208, 1000):
        idx = torch.randint(0, n_total, (rows,), generator=g)
        rc, z, G, dW, db, loss, status = call_grad(Ed, Yd, idx.to(DEV), Wd, bd)
        assert rc == 0, last_error()
        torch.cuda.synchronize()
        assert int(status) == 0
        e, y = E64[idx], Y64[idx]
        z64 = e @ W64.T + b64
        dz = 768 * U * (e.abs() @ W64.abs().T) + U * b64.abs()
        err = (z.double().cpu() - z64).abs()
        print("N %d rows %d: z err/bound %.3g" % (N, rows, float((err / dz).max())))
        assert bool((err <= dz).all()), (N, rows, float((err - dz).max()))
        p64 = torch.sigmoid(z64)
        G64 = (p64 - y) / (rows * N)
        dG = dz / (4 * rows * N) + 4 * U / (rows * N)
        err = (G.double().cpu() - G64).abs()
        print("   G err/bound %.3g" % float((err / dG).max()))
        assert bool((err <= dG).all()), (N, rows, float((err - dG).max()))
        dW64 = G64.T @ e
        bound = (rows + 4) * U * (G64.abs().T @ e.abs()) + dG.T @ e.abs()
        err = (dW.double().cpu() - dW64).abs()
        print("   dW err/bound %.3g" % float((err / bound).max()))
        assert bool((err <= bound).all()), (N, rows, float((err - bound).max()))
        db64 = G64.sum(0)
        bound = (rows + 4) * U * G64.abs().sum(0) + dG.sum(0)
        err = (db.double().cpu() - db64).abs()
        print("   db err/bound %.3g" % float((err / bound).max()))
        assert bool((err <= bound).all()), (N, rows, float((err - bound).max()))
        l64 = -(y * torch.log(p64).clamp(min=-100) + (1 - y) * torch.log1p(-p64).clamp(min=-100))
        depth = 64 + math.ceil(rows / 16) * math.ceil(N / 16) / 256
        bound = float(dz.mean()) + (depth + 8) * U * float(l64.abs().mean())
        err = abs(float(loss) - float(l64.mean()))
        print("   loss %.6f err/bound %.3g" % (float(loss), err / bound))
        assert err <= bound, (N, rows, err, bound)
        # the scale 1 / (rows N), which no trajectory can see (Adam is invariant to it): db sums G, G sums to (p - y) / (rows N)
        assert abs(float(G.double().sum()) - float(G64.sum())) <= float(dG.sum()) + rows * N * U * float(G64.abs().max())


# ---- 2. the update against float64 -----------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def adam64(p, g, m, v, x, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, amsgrad=True, decoupled=False):
    """One step of section 1's formulas in float64 from float32 state -> (p, m, v, vmax, M, step_size / denom)."""
    p, g, m, v, x = (a.double() for a in (p, g, m, v, x))
    b1, ob1, b2, ob2, ep = f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    step, bc2 = f32(lr / (1.0 - beta1 ** t)), f32(math.sqrt(1.0 - beta2 ** t))
    if decoupled:
        p = p * f32(1.0 - lr * wd)
    else:
        g = g + f32(wd) * p
    M = b1 * m.abs() + ob1 * g.abs()
    m = b1 * m + ob1 * g
    v = b2 * v + ob2 * g * g
    if amsgrad:
        x = torch.maximum(x, v)
    denom = (x if amsgrad else v).sqrt() / bc2 + ep
    return p - step * m / denom, m, v, x, M, step / denom


@pytest.mark.parametrize("t0", [1, 1000])
@pytest.mark.parametrize("mode", ["adam", "adam_wd", "adamw", "adam_noams"])
def test_update_against_float64(mode, t0):
    """acx_adam_update on crafted vectors, three consecutive steps, each compared with the float64 evaluation from the GPU's own
    fp32 state before that step: |g| from 1e-12 to 1e+3 (below, at and above eps = 1e-8, where the place of eps decides the
    result), a large gradient followed by one a thousand times smaller (where amsgrad decides), then the first with its sign
    flipped (m and g of opposite signs).  With M = beta1 |m0| + (1 - beta1) |g|: |m - m64| <= 4 u M; v, vmax within 4 u relative;
    |p - p64| <= u |p64| + 8 u step_size M / denom64."""
    n = 8192
    gen = torch.Generator().manual_seed(7)
    mag = 10.0 ** (torch.rand(n, generator=gen) * 15 - 12)
    mag[:2048] = 10.0 ** (torch.rand(2048, generator=gen) * 3 - 10)                  # 1e-10 .. 1e-7: around eps
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g1 = mag * sign
    grads = [g1, g1 * 1e-3 * (1 + torch.rand(n, generator=gen)), -g1]
    p = torch.randn(n, generator=gen)
    if t0 == 1:
        m, v, x = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    else:
        m = mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0) * torch.rand(n, generator=gen)
        v = (mag * torch.rand(n, generator=gen)) ** 2
        x = v * (1 + torch.rand(n, generator=gen))
    kw = {"adam": {}, "adam_wd": {"wd": 0.01}, "adamw": {"wd": 0.01, "decoupled": True}, "adam_noams": {"amsgrad": False}}[mode]
    hp = _ffi.adam(0.9, 0.999, 1e-8, kw.get("wd", 0.0), kw.get("amsgrad", True), kw.get("decoupled", False))
    lr = 1e-3
    pd, md, vd, xd = (a.to(DEV) for a in (p, m, v, x))
    for k, g in enumerate(grads):
        t = t0 + k
        before = [a.cpu().clone() for a in (pd, md, vd, xd)]
        assert call_update(pd, g.to(DEV), md, vd, xd if kw.get("amsgrad", True) else None, hp, t, lr) == 0, last_error()
        torch.cuda.synchronize()
        p64, m64, v64, x64, M, ratio = adam64(before[0], g, before[1], before[2], before[3], t, lr, **kw)
        em = (md.double().cpu() - m64).abs()
        print("%s t %d: m err / (u M) %.3g" % (mode, t, float((em / (U * M)).max())))
        assert bool((em <= 4 * U * M).all())
        ev = (vd.double().cpu() - v64).abs()
        print("   v err / (u v) %.3g" % float((ev / (U * v64)).max()))
        assert bool((ev <= 4 * U * v64).all())
        if kw.get("amsgrad", True):
            ex = (xd.double().cpu() - x64).abs()
            assert bool((ex <= 4 * U * x64).all())
        else:
            assert torch.equal(xd.cpu(), before[3])                                # untouched (and never read: NULL was passed)
        ep = (pd.double().cpu() - p64).abs()
        bound = U * p64.abs() + 8 * U * ratio * M
        print("   p err / bound %.3g" % float((ep / bound).max()))
        assert bool((ep <= bound).all()), float((ep - bound).max())


# ---- 3. the fused step leaves the bits of its components --------------------------------------------------------------------
@pytest.mark.parametrize("N,rows", [(50, 64), (527, 512), (1, 37), (4096, 256), (10, 1000)])
@pytest.mark.parametrize("amsgrad", [True, False])
def test_fused_step_equals_components(N, rows, amsgrad):
    E, Y = data(1500, N, seed=3)
    W0, b0 = init(N)
    Ed, Yd = E.to(DEV), Y.to(DEV).to(torch.uint8)
    a, b = fresh_state(W0, b0), fresh_state(W0, b0)
    hp = _ffi.adam(0.9, 0.999, 1e-8, 0.01, amsgrad, False)
    ws = workspace(rows, N)
    loss_a, status = torch.zeros(2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    for t in (1, 2):
        idx = torch.randint(0, 1500, (rows,), generator=gen).to(DEV)
        st = dict(a) if amsgrad else {**a, "xW": None, "xb": None}
        assert call_step(Ed, Yd, idx, st, hp, t, 1e-3, loss_a[t - 1:], status, ws) == 0, last_error()
        rc, z, G, dW, db, loss_b, _ = call_grad(Ed, Yd, idx, b["W"], b["b"], ws=ws)
        assert rc == 0, last_error()
        assert call_update(b["W"], dW, b["mW"], b["vW"], b["xW"] if amsgrad else None, hp, t, 1e-3) == 0, last_error()
        assert call_update(b["b"], db, b["mb"], b["vb"], b["xb"] if amsgrad else None, hp, t, 1e-3) == 0, last_error()
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (N, rows, t, k)
        assert torch.equal(loss_a[t - 1:t], loss_b), (N, rows, t)
        assert not torch.equal(a["W"].cpu(), W0)
    assert int(status) == 0


# ---- 4. trajectories against the reference optimiser ------------------------------------------------------------------------
CASES = {"n2000_N50": (2000, 50, 256, 10, 80), "n3000_N527": (3000, 527, 512, 6, 36), "n300_N1": (300, 1, 64, 10, 50)}


def run_trajectory(n, N, batch, epochs, steps, lr=1e-3, **kw):
    E, Y = data(n, N)
    W0, b0 = init(N)
    W64, b64, l64, zmax = oracle(E, Y, W0, b0, batch, epochs, lr, torch.float64, **kw)
    W32, b32, l32, _ = oracle(E, Y, W0, b0, batch, epochs, lr, torch.float32, **kw)
    assert l64.numel() == steps and zmax < 12, zmax            # far from the saturation of the fp32 sigmoid: both gradient forms agree
    fit = fit_head(E.to(DEV), Y.to(DEV), epochs=epochs, batch_size=batch, lr=lr, init=(W0, b0), seed=2,
                   weight_decay=kw.get("wd", 0.0), decoupled=kw.get("adamw", False))
    torch.cuda.synchronize()
    for name, got, r64, r32 in (("W", fit.weight, W64, W32), ("b", fit.bias, b64, b32), ("loss", fit.loss, l64, l32)):
        floor = float((r32.double() - r64).abs().max())
        bound = max(8 * floor, steps * U * float(r64.abs().max()))
        err = float((got.double().cpu() - r64).abs().max())
        print("%s: max|gpu - f64| %.3g, torch f32 floor %.3g, bound %.3g" % (name, err, floor, bound))
        assert err <= bound, (name, err, bound)
    assert float(l64[-1]) < 0.5 * float(l64[0])
    return fit


@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_against_torch_adam(case):
    """fit_head with the oracle's init and permutation against torch.optim.Adam(amsgrad=True) in float64:
    max|W - W64| <= max(8 floor, steps u max|W64|), floor = max|W32 - W64| of torch's own float32 run (the GPU sums the same
    terms in tile order: another draw of the same rounding noise), the second term one rounding of the parameter per step;
    the same for b and for the step losses."""
    run_trajectory(*CASES[case])


def test_trajectory_adamw():
    run_trajectory(*CASES["n2000_N50"], adamw=True, wd=0.01)


def test_trajectory_lr_sequence():
    n, N, batch, epochs, steps = CASES["n2000_N50"]
    lrs = [1e-3 * min(1.0, (t + 1) / 20) for t in range(steps)]                    # linear warm-up over the first 20 steps
    run_trajectory(n, N, batch, epochs, steps, lr=lrs)


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------
def test_same_arguments_same_bits_other_seed_other_fit():
    E, Y = data(2000, 50)
    Ed, Yd = E.to(DEV), Y.to(DEV).bool()
    a = fit_head(Ed, Yd, epochs=3, batch_size=256, lr=1e-3)
    b = fit_head(Ed, Yd, epochs=3, batch_size=256, lr=1e-3)
    c = fit_head(Ed, Yd, epochs=3, batch_size=256, lr=1e-3, seed=1)
    for x, y in ((a.weight, b.weight), (a.bias, b.bias), (a.loss, b.loss)):
        assert torch.equal(x, y)
    assert not torch.equal(a.weight, c.weight) and not torch.equal(a.loss, c.loss)
    assert a.loss.shape == (24,) and len(a.history) == 3
    assert float(a.history[1]["loss"]) == float(a.loss[8:16].mean())


def test_fit_on_a_side_stream_beside_a_forward(synth_sd):
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    model.load_state_dict(synth_sd)
    model = model.to(DEV).eval()
    wav = synth.synth_waveforms(16, 2 * SR, seed=4).to(DEV)
    E, Y = data(3000, 527)
    Ed, Yd = E.to(DEV), Y.to(DEV)
    alone = fit_head(Ed, Yd, epochs=4, batch_size=512, lr=1e-3)
    with torch.no_grad():
        ref = model(wav)["clipwise_logits"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        beside = fit_head(Ed, Yd, epochs=4, batch_size=512, lr=1e-3)
    with torch.no_grad():
        outs = [model(wav)["clipwise_logits"] for _ in range(6)]
    torch.cuda.synchronize()
    for x, y in ((alone.weight, beside.weight), (alone.bias, beside.bias), (alone.loss, beside.loss)):
        assert torch.equal(x, y)
    assert all(torch.equal(o, ref) for o in outs)


def test_captured_step_replays_the_eager_bits():
    E, Y = data(2000, 50)
    W0, b0 = init(50)
    Ed, Yd = E.to(DEV), Y.to(DEV)
    idx = torch.randperm(2000, generator=torch.Generator().manual_seed(2))[:256].to(DEV)
    st, keep = fresh_state(W0, b0), fresh_state(W0, b0)
    hp = _ffi.adam()
    ws = workspace(256, 50)
    loss, status = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert call_step(Ed, Yd, idx, st, hp, 1, 1e-3, loss, status, ws) == 0, last_error()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in st.items()}
    eager_loss = loss.clone()
    for k in st:
        st[k].copy_(keep[k])
    loss.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                   # a linear graph: two kernels in a row
        rc = call_step(Ed, Yd, idx, st, hp, 1, 1e-3, loss, status, ws)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(st["W"], keep["W"])                                          # capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(st[k], eager[k]), k
    assert torch.equal(loss, eager_loss) and int(status) == 0


# ---- 6. a fit of no epochs ---------------------------------------------------------------------------------------------------
def test_no_epochs_returns_the_head_unchanged():
    E, Y = data(100, 527)
    g = torch.Generator().manual_seed(9)
    W, b = torch.randn(527, 768, generator=g) * 0.05, torch.randn(527, generator=g)
    fit = fit_head(E.to(DEV), Y.to(DEV), epochs=0, init=(W, b))
    assert torch.equal(fit.weight.cpu(), W) and torch.equal(fit.bias.cpu(), b)
    assert fit.loss.shape == (0,) and fit.history == []
    fit = fit_head(E.to(DEV), Y.to(DEV), epochs=0, init=(W.to(DEV), b.to(DEV)))
    assert torch.equal(fit.weight.cpu(), W) and fit.weight.data_ptr() != W.data_ptr()


# ---- 7. model level --------------------------------------------------------------------------------------------------------------
def make_model(sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def test_model_fit_head(synth_sd, tmp_path):
    model = make_model(synth_sd)
    N = 5
    lens = [SR, 20000, SR + 777, 9000, 2 * SR, SR, 12345, 30000, SR, 25000]
    waves = [synth.synth_waveforms(1, L, seed=60 + i)[0] for i, L in enumerate(lens)]
    target = torch.rand(len(lens), N, generator=torch.Generator().manual_seed(3)) < 0.4
    kw = dict(epochs=3, batch_size=4, lr=1e-2, seed=5)
    emb = torch.stack(extract(model, waves, what="scene", pack=True)).to(DEV)
    want = fit_head(emb, target.to(DEV), **kw)
    fit = model.fit_head(waves, target, **kw)
    for x, y in ((fit.weight, want.weight), (fit.bias, want.bias), (fit.loss, want.loss)):
        assert torch.equal(x, y)
    assert not model.training and not model.head_audioset.training
    assert model.head_audioset.out_features == N and model.head_audioset.weight.device.type == "cuda"
    assert torch.equal(model.head_audioset.weight.data, fit.weight) and torch.equal(model.head_audioset.bias.data, fit.bias)
    x = synth.synth_waveforms(3, SR, seed=8).to(DEV)
    with torch.no_grad():
        out = model(x)["clipwise_logits"]
        scene = model.forward_scene_embeddings(x)
    assert out.shape == (3, N)
    e, w64, b64 = scene.double().cpu(), fit.weight.double().cpu(), fit.bias.double().cpu()
    bound = 768 * U * (e.abs() @ w64.abs().T) + U * b64.abs()
    assert bool(((out.double().cpu() - (e @ w64.T + b64)).abs() <= bound).all())
    # embeddings handed over directly: the same fit
    again = make_model(synth_sd)
    f2 = again.fit_head(emb, target.to(DEV), **kw)
    assert torch.equal(f2.weight, fit.weight)
    # checkpoints of both forms load as a fine-tuned model with the same output bits
    from safetensors.torch import save_file
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.save({"model": sd}, str(tmp_path / "head.pth"))
    save_file(sd, str(tmp_path / "model.safetensors"))
    for name in ("head.pth", "model.safetensors"):
        loaded = ConvNeXt.from_pretrained(str(tmp_path / name)).to(DEV).eval()
        assert loaded.head_audioset.out_features == N
        with torch.no_grad():
            assert torch.equal(loaded(x)["clipwise_logits"], out), name
    # the other forward paths write N-wide rows
    recs = [synth.synth_waveforms(1, 3 * SR + 5, seed=70)[0].to(DEV)]
    with torch.no_grad():
        rows = model.forward_windows(recs, window=1.0, hop=0.5)
        assert rows[0]["clipwise_logits"].shape[1] == N
        st = model.stream(slots=1, window=1.0, hop=0.5, max_push=1.0)
        assert st.classes == N
        assert st.push({0: recs[0][:2 * SR]})["clipwise_logits"].shape[1] == N
        st.close_handle()
    # 44.1 kHz input
    waves44 = [synth.synth_waveforms(1, L, seed=90 + i)[0] for i, L in enumerate([44100, 30000, 50000, 44100])]
    t44 = target[:4]
    m44 = make_model(synth_sd)
    f44 = m44.fit_head(waves44, t44, sample_rate=44100, **kw)
    e44 = torch.stack(extract(make_model(synth_sd), waves44, what="scene", pack=True, sample_rate=44100)).to(DEV)
    w44 = fit_head(e44, t44.to(DEV), **kw)
    assert torch.equal(f44.weight, w44.weight) and torch.equal(f44.loss, w44.loss)


# ---- 8. validation history ---------------------------------------------------------------------------------------------------
def test_validation_history():
    E, Y = data(1000, 20)
    Ev, Yv = data(400, 20, seed=1)
    Ed, Yd, Evd, Yvd = E.to(DEV), Y.to(DEV), Ev.to(DEV), Yv.to(DEV)
    kw = dict(batch_size=128, lr=1e-3, seed=3)
    fit = fit_head(Ed, Yd, epochs=3, val=(Evd, Yvd), **kw)
    assert len(fit.history) == 3
    for e in range(3):
        part = fit_head(Ed, Yd, epochs=e + 1, **kw)
        probs = torch.sigmoid(torch.addmm(part.bias, Evd, part.weight.t()))
        stats = tagging_metrics(Yvd, probs)
        for k in ("average_precision", "auc", "d_prime"):
            assert np.array_equal(fit.history[e][k], stats[k]), (e, k)
        assert fit.history[e]["mAP"] == float(np.mean(stats["average_precision"]))
    assert torch.equal(part.weight, fit.weight)
    assert fit.history[2]["mAP"] > fit.history[0]["mAP"]


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_codes_without_a_launch():
    E, Y = data(100, 10)
    W0, b0 = init(10)
    Ed, Yd = E.to(DEV), Y.to(DEV)
    idx = torch.arange(32, device=DEV)
    ws = workspace(32, 10)
    hp = _ffi.adam()
    loss, status = torch.full((1,), 7.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    st = fresh_state(W0, b0)
    misaligned = (ctypes.c_void_p(ws[0].data_ptr() + 64), ws[1])
    cases = [({"E": None}, -1, "E"), ({"Y": None}, -1, "target"), ({"idx": None}, -1, "idx"), ({"W": None}, -1, "W"),
             ({"b": None}, -1, "b"), ({"mW": None}, -1, "mW"), ({"xW": None}, -1, "vmaxW"), ({"loss": None}, -1, "loss_out"),
             ({"status": None}, -1, "status"), ({"ws": None}, -1, "workspace"), ({"hp": None}, -1, "hp"),
             ({"rows": 0}, -1, "rows"), ({"N": 0}, -1, "classes"), ({"N": _ffi.MAX_CLASSES + 1}, -1, "classes"),
             ({"ld_e": 767}, -1, "ld_e"), ({"ld_y": 9}, -1, "ld_target"), ({"dtype": 5}, -1, "target_dtype"),
             ({"ws_bytes": ws[1] - 1}, -5, "workspace"), ({"ws": misaligned[0]}, -5, "aligned"), ({"t": 0}, -1, "step_t"),
             ({"lr": -1.0}, -1, "lr"),
             ({"hp": ctypes.byref(_ffi.adam(beta1=1.0))}, -1, "beta1"), ({"hp": ctypes.byref(_ffi.adam(beta2=-0.1))}, -1, "beta2"),
             ({"hp": ctypes.byref(_ffi.adam(eps=0.0))}, -1, "eps"), ({"hp": ctypes.byref(_ffi.adam(weight_decay=-1.0))}, -1, "weight_decay")]
    for over, code, word in cases:
        rc = call_step(Ed, Yd, idx, st, hp, 1, 1e-3, loss, status, ws, over=over)
        assert rc == code, (over, rc)
        assert word in last_error(), (over, last_error())
    for over, code, word in [({"z": None}, -1, "z"), ({"rows": 0}, -1, "rows"), ({"ld_e": 700}, -1, "ld_e"),
                             ({"ws_bytes": 0}, -5, "workspace")]:
        rc = call_grad(Ed, Yd, idx, st["W"], st["b"], ws=ws, over=over)[0]
        assert rc == code and word in last_error(), (over, rc, last_error())
    for over, code, word in [({"p": None}, -1, "param"), ({"n": 0}, -1, "n ="), ({"x": None}, -1, "vmax"), ({"t": -3}, -1, "step_t"),
                             ({"hp": None}, -1, "hp")]:
        rc = call_update(st["W"], st["mW"], st["mW"], st["vW"], st["xW"], hp, 1, 1e-3, over=over)
        assert rc == code and word in last_error(), (over, rc, last_error())
    torch.cuda.synchronize()
    assert torch.equal(st["W"].cpu(), W0) and float(loss) == 7.0 and int(status) == 0       # nothing ran
    assert float(st["mW"].abs().max()) == 0.0
    with pytest.raises(_ffi.AcxError, match="rows"):
        _ffi.head_fit_workspace_bytes(0, 10)


def test_bad_indices_are_clamped_and_flagged():
    """E and the targets are the middle slices of larger NaN-filled buffers and idx holds -1 and n_rows_total: addresses inside
    those buffers, so even a kernel without the clamp could not fault -- it would read NaN."""
    n, N = 64, 10
    E, Y = data(n, N)
    big = torch.full((3 * n, 768), float("nan"), device=DEV)
    bigy = torch.full((3 * n, N), float("nan"), device=DEV)
    big[n:2 * n], bigy[n:2 * n] = E.to(DEV), Y.to(DEV)
    Ed, Yd = big[n:2 * n], bigy[n:2 * n]
    W0, b0 = init(N)
    idx = torch.arange(16)
    idx[3], idx[9] = -1, n
    rc, z, G, dW, db, loss, status = call_grad(Ed, Yd, idx.to(DEV), W0.to(DEV), b0.to(DEV))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert int(status) & _ffi.FIT_BAD_INDEX
    for t in (z, G, dW, db, loss):
        assert bool(torch.isfinite(t).all())
    good = idx.clone()
    good[3], good[9] = 0, n - 1                                                    # what the clamp reads
    rc, z2, G2, dW2, db2, loss2, status2 = call_grad(Ed, Yd, good.to(DEV), W0.to(DEV), b0.to(DEV))
    torch.cuda.synchronize()
    assert int(status2) == 0 and torch.equal(dW, dW2) and torch.equal(z, z2) and torch.equal(loss, loss2)
    st = fresh_state(W0, b0)
    lossb, statusb = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert call_step(Ed, Yd, idx.to(DEV), st, _ffi.adam(), 1, 1e-3, lossb, statusb, workspace(16, N)) == 0
    torch.cuda.synchronize()
    assert int(statusb) & _ffi.FIT_BAD_INDEX and bool(torch.isfinite(st["W"]).all()) and bool(torch.isfinite(lossb).all())


def test_value_errors_before_any_launch():
    E, Y = data(64, 5)
    Ed, Yd = E.to(DEV), Y.to(DEV)
    with pytest.raises(ValueError, match="emb"):
        fit_head(E, Y)                                                             # CPU tensors: GPU only
    with pytest.raises(ValueError, match="target"):
        fit_head(Ed, Yd * 2)
    with pytest.raises(ValueError, match="target"):
        fit_head(Ed, (Yd * 2).to(torch.int64))
    with pytest.raises(ValueError, match="lr"):
        fit_head(Ed, Yd, epochs=2, batch_size=32, lr=[1e-3] * 3)
