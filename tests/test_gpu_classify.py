"""GPU (`-m gpu`): single-label heads -- the cross-entropy training step (acx_head_fit_step_ce / acx_head_fit_grad_ce,
fit_head(loss="ce")), softmax top-k (acx_softmax_topk) and the classification counts (acx_classification_counts), up to
ConvNeXt.fit_head(loss="ce") / ConvNeXt.classify.

The oracles are the float64 host definitions of pytorch/classify.py and torch on the CPU (F.cross_entropy, torch.optim.Adam) in
float64, with torch's own float32 run as the rounding floor of a trajectory.  u = 2^-24; every bound is computed from float64
quantities.  D = _ffi.softmax_depth(N) is the depth of the row sum that csrc/head_fit.hip's header declares."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import classify as cl
from audioset_convnext_inf_amd.pytorch.convnext import ConvNeXt, convnext_tiny
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract
from audioset_convnext_inf_amd.pytorch.finetune import fit_head
from fit_calls import call_update, fresh_state, init, last_error, vp

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SR = 32000
DEV = "cuda"


def data(n, N, seed=0):
    """proto[y] * 0.7 + randn, layer-normed; y = randint(N)."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(N, 768, generator=g)
    y = torch.randint(0, N, (n,), generator=g)
    x = proto[y] * 0.7 + torch.randn(n, 768, generator=g)
    return F.layer_norm(x, (768,)), y


def workspace(rows, N):
    nbytes = _ffi.head_fit_ce_workspace_bytes(rows, N)
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def stream():
    return _ffi.stream_ptr(torch.device(DEV))


def call_grad(E, y, idx, W, b, eps=0.0, ws=None, over=None):
    """acx_head_fit_grad_ce on device tensors -> (rc, z, G, dW, db, loss, status)."""
    rows, N = idx.numel(), W.shape[0]
    z = torch.full((rows, N), float("nan"), device=DEV)
    G = torch.full_like(z, float("nan"))
    dW, db = torch.full((N, 768), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    loss, status = torch.full((1,), float("nan"), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    wsb, nbytes = workspace(rows, N) if ws is None else ws
    a = dict(E=vp(E), ld_e=E.stride(0), n_total=E.shape[0], y=vp(y), idx=vp(idx), rows=rows, N=N, eps=eps, W=vp(W), b=vp(b),
             z=vp(z), G=vp(G), dW=vp(dW), db=vp(db), loss=vp(loss), status=vp(status), ws=vp(wsb), ws_bytes=nbytes)
    a.update(over or {})
    rc = _ffi.lib().acx_head_fit_grad_ce(a["E"], a["ld_e"], a["n_total"], a["y"], a["idx"], a["rows"], a["N"], a["eps"], a["W"],
                                         a["b"], a["z"], a["G"], a["dW"], a["db"], a["loss"], a["status"], a["ws"], a["ws_bytes"],
                                         stream())
    return rc, z, G, dW, db, loss, status


def call_step(E, y, idx, st, hp, t, lr, loss, status, ws, eps=0.0, over=None):
    a = dict(E=vp(E), ld_e=E.stride(0), n_total=E.shape[0], y=vp(y), idx=vp(idx), rows=idx.numel(), N=st["W"].shape[0], eps=eps,
             hp=ctypes.byref(hp) if hp is not None else None, t=t, lr=lr, loss=vp(loss), status=vp(status), ws=vp(ws[0]),
             ws_bytes=ws[1])
    a.update({k: vp(v) for k, v in st.items()})
    a.update(over or {})
    return _ffi.lib().acx_head_fit_step_ce(a["E"], a["ld_e"], a["n_total"], a["y"], a["idx"], a["rows"], a["N"], a["eps"], a["W"],
                                           a["b"], a["mW"], a["vW"], a["xW"], a["mb"], a["vb"], a["xb"], a["hp"], a["t"], a["lr"],
                                           a["loss"], a["status"], a["ws"], a["ws_bytes"], stream())


def p_bound(z64, delta, N):
    """|p - p64| <= p64 (e^{2 delta_r} - 1) + p64 (|z_c - m| + D + 16) u, with p64 (float64 tensors; delta (rows, 1) or 0)."""
    m = z64.max(dim=1, keepdim=True).values
    p64 = torch.softmax(z64, dim=1)
    return p64, p64 * torch.expm1(2 * delta) + p64 * ((z64 - m).abs() + _ffi.softmax_depth(N) + 16) * U


# ---- 1. the gradient pass against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N", [1, 2, 10, 50, 257, 527, 4096, 32768])
def test_gradient_against_float64(N, eps):
    """z, G, dW, db and the loss of acx_head_fit_grad_ce against float64; rows in {1, 7, 64, 208} ({1, 7} at N = 32 768),
    shuffled idx with repeats, ld_e = 772, and a second weight set scaled so that max |z| is about 80.  With dz = 768 u |E||W|^T
    + u |b| and delta_r = max_c dz[r, c]: |z - z64| <= dz; p within p_bound; G = (p - q) / rows within dG = p_bound / rows +
    4 u / rows; |dW - dW64| <= (rows + 4) u |G64|^T |E| + dG^T |E|, the same for db; the loss within mean_r 2 delta_r +
    (D + 8) u mean(|lse| + |sum q z|).  N = 1: G = 0 and loss = 0 exactly."""
    n_total = 300
    g = torch.Generator().manual_seed(140 + N)
    buf = torch.randn(n_total, 772, generator=g)
    E = F.layer_norm(buf[:, :768], (768,))
    buf[:, :768] = E
    W1, b1 = torch.randn(N, 768, generator=g) * 0.05, torch.randn(N, generator=g) * 0.1
    y = torch.randint(0, N, (n_total,), generator=g)
    Ed, yd = buf.to(DEV)[:, :768], y.to(DEV)
    assert Ed.stride(0) == 772
    E64 = E.double()
    scale80 = 80.0 / float((E64 @ W1.double().T + b1.double()).abs().max())
    D = _ffi.softmax_depth(N)
    for W, b in ((W1, b1), (W1 * scale80, b1 * scale80)):
        Wd, bd, W64, b64 = W.to(DEV), b.to(DEV), W.double(), b.double()
        for rows in ((1, 7) if N == 32768 else (1, 7, 64, 208)):
            idx = torch.randint(0, n_total, (rows,), generator=g)
            rc, z, G, dW, db, loss, status = call_grad(Ed, yd, idx.to(DEV), Wd, bd, eps)
            assert rc == 0, last_error()
            torch.cuda.synchronize()
            assert int(status) == 0
            e, yy = E64[idx], y[idx]
            z64 = e @ W64.T + b64
            dz = 768 * U * (e.abs() @ W64.abs().T) + U * b64.abs()
            err = (z.double().cpu() - z64).abs()
            print("N %d rows %d max|z| %.1f: z err/bound %.3g" % (N, rows, float(z64.abs().max()), float((err / dz).max())))
            assert bool((err <= dz).all()), (N, rows, float((err - dz).max()))
            delta = dz.max(dim=1, keepdim=True).values
            p64, dp = p_bound(z64, delta, N)
            q = torch.full((rows, N), eps / N, dtype=torch.float64)
            q[torch.arange(rows), yy] += 1.0 - eps
            G64 = (p64 - q) / rows
            dG = dp / rows + 4 * U / rows
            err = (G.double().cpu() - G64).abs()
            print("   G err/bound %.3g" % float((err / dG).max()))
            assert bool((err <= dG).all()), (N, rows, float((err - dG).max()))
            bound = (rows + 4) * U * (G64.abs().T @ e.abs()) + dG.T @ e.abs()
            err = (dW.double().cpu() - G64.T @ e).abs()
            print("   dW err/bound %.3g" % float((err / bound).max()))
            assert bool((err <= bound).all()), (N, rows, float((err - bound).max()))
            bound = (rows + 4) * U * G64.abs().sum(0) + dG.sum(0)
            err = (db.double().cpu() - G64.sum(0)).abs()
            print("   db err/bound %.3g" % float((err / bound).max()))
            assert bool((err <= bound).all()), (N, rows, float((err - bound).max()))
            lse, qz = torch.logsumexp(z64, dim=1), (q * z64).sum(dim=1)
            l64 = float((lse - qz).mean())
            want, _, g_host = cl.cross_entropy_host(z64.numpy(), yy.numpy(), eps)            # the host definition agrees
            assert abs(want - l64) <= 1e-12 * max(1.0, abs(l64)) and np.allclose(g_host, G64.numpy(), rtol=1e-10, atol=1e-16)
            bound = float((2 * delta).mean()) + (D + 8) * U * float((lse.abs() + qz.abs()).mean())
            err = abs(float(loss) - l64)
            print("   loss %.6f err/bound %.3g" % (float(loss), err / bound if bound else 0.0))
            assert err <= bound, (N, rows, err, bound)
            if N == 1:
                assert not bool(G.any()) and float(loss) == 0.0


# ---- 2. the fused step leaves the bits of its components --------------------------------------------------------------------
@pytest.mark.parametrize("N,rows", [(50, 64), (527, 512), (2, 37), (4096, 256)])
@pytest.mark.parametrize("amsgrad", [True, False])
def test_fused_step_equals_components(N, rows, amsgrad):
    E, y = data(1500, N, seed=3)
    W0, b0 = init(N)
    Ed, yd = E.to(DEV), y.to(DEV)
    a, b = fresh_state(W0, b0), fresh_state(W0, b0)
    hp = _ffi.adam(0.9, 0.999, 1e-8, 0.01, amsgrad, False)
    ws = workspace(rows, N)
    loss_a, status = torch.zeros(2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    for t in (1, 2):
        idx = torch.randint(0, 1500, (rows,), generator=gen).to(DEV)
        st = dict(a) if amsgrad else {**a, "xW": None, "xb": None}
        assert call_step(Ed, yd, idx, st, hp, t, 1e-3, loss_a[t - 1:], status, ws, eps=0.1) == 0, last_error()
        rc, z, G, dW, db, loss_b, _ = call_grad(Ed, yd, idx, b["W"], b["b"], eps=0.1, ws=ws)
        assert rc == 0, last_error()
        assert call_update(b["W"], dW, b["mW"], b["vW"], b["xW"] if amsgrad else None, hp, t, 1e-3) == 0, last_error()
        assert call_update(b["b"], db, b["mb"], b["vb"], b["xb"] if amsgrad else None, hp, t, 1e-3) == 0, last_error()
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (N, rows, t, k)
        assert torch.equal(loss_a[t - 1:t], loss_b), (N, rows, t)
        assert not torch.equal(a["W"].cpu(), W0)
    assert int(status) == 0


# ---- 3. a row's bits do not depend on its batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [50, 527, 4096])
def test_row_independence(N):
    """The same clip as a batch of one and at three positions of two different 208-row batches: equal z bits everywhere (N = 50:
    16 x 16 logit tiles and the wave shape of the row pass; 527: 32 x 32 tiles; 4096: 32 x 32 tiles and the workgroup shape --
    the logit tile shape is a function of N, so the batch of one runs the tiles the batch of 208 runs).  Equal G bits at equal
    `rows` across positions and batches; against the batch of one, G differs by the factor 1 / 208 alone: two roundings."""
    E, y = data(400, N, seed=6)
    W0, b0 = init(N)
    W0 = W0 * 20
    Ed, yd, Wd, bd = E.to(DEV), y.to(DEV), W0.to(DEV), b0.to(DEV)
    clip = 17
    g = torch.Generator().manual_seed(8)
    _, z1, G1, _, _, _, _ = call_grad(Ed, yd, torch.tensor([clip], device=DEV), Wd, bd, 0.1)
    z_seen, g_seen = [], []
    for trial in range(2):
        idx = torch.randint(0, 400, (208,), generator=g)
        pos = [0, 101, 207] if trial == 0 else [5, 64, 150]
        idx[pos] = clip
        rc, z, G, _, _, _, _ = call_grad(Ed, yd, idx.to(DEV), Wd, bd, 0.1)
        assert rc == 0, last_error()
        torch.cuda.synchronize()
        z_seen += [z[p].clone() for p in pos]
        g_seen += [G[p].clone() for p in pos]
    for zz, gg in zip(z_seen, g_seen):
        assert torch.equal(zz, z1[0]) and torch.equal(gg, g_seen[0])
    assert float(z1.abs().max()) > 1.0
    ref = G1[0].double() / 208
    assert bool(((g_seen[0].double() - ref).abs() <= (2 * U + U * U) * ref.abs() + 2.0 ** -149).all())
    # other batch sizes, the sizes at which the BCE gradient kernel changes its tile shape among them
    for rows in (7, 33, 64, 300):
        idx = torch.full((rows,), clip, dtype=torch.int64)
        idx[: rows // 2] = torch.randint(0, 400, (rows // 2,), generator=g)
        _, z, _, _, _, _, _ = call_grad(Ed, yd, idx.to(DEV), Wd, bd, 0.1)
        assert torch.equal(z[rows - 1], z1[0]), (N, rows)


# ---- 4. trajectories against the reference optimiser -------------------------------------------------------------------------
def oracle(E, y, W0, b0, batch, epochs, lr, dtype, eps, seed=2):
    E = E.to(dtype)
    W, b = W0.to(dtype).clone().requires_grad_(), b0.to(dtype).clone().requires_grad_()
    opt = torch.optim.Adam([W, b], lr=lr, betas=(0.9, 0.999), eps=1e-8, amsgrad=True)
    g = torch.Generator().manual_seed(seed)
    losses, zmax = [], 0.0
    for _ in range(epochs):
        perm = torch.randperm(E.shape[0], generator=g)
        for s in range(0, E.shape[0], batch):
            i = perm[s:s + batch]
            z = E[i] @ W.T + b
            loss = F.cross_entropy(z, y[i], label_smoothing=eps)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            zmax = max(zmax, float(z.detach().abs().max()))
    return W.detach(), b.detach(), torch.stack(losses), zmax


CASES = {"n2000_N50": (2000, 50, 256, 10, 0.0), "n2000_N50_ls": (2000, 50, 256, 10, 0.1), "n3000_N527": (3000, 527, 512, 6, 0.0),
         "n300_N2": (300, 2, 64, 10, 0.0)}


@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_against_torch_adam(case):
    """fit_head(loss="ce") with the oracle's init and permutation against torch.optim.Adam(amsgrad=True) + F.cross_entropy in
    float64: max|W - W64| <= max(8 floor, steps u max|W64|), floor = max|W32 - W64| of torch's own float32 run; the same for b
    and the step losses (the rule of test_gpu_finetune.py's test_trajectory_against_torch_adam)."""
    n, N, batch, epochs, eps = CASES[case]
    E, y = data(n, N)
    W0, b0 = init(N)
    lr = 1e-3
    W64, b64, l64, zmax = oracle(E, y, W0, b0, batch, epochs, lr, torch.float64, eps)
    W32, b32, l32, _ = oracle(E, y, W0, b0, batch, epochs, lr, torch.float32, eps)
    steps = l64.numel()
    fit = fit_head(E.to(DEV), y.to(DEV), classes=N, loss="ce", label_smoothing=eps, epochs=epochs, batch_size=batch, lr=lr,
                   init=(W0, b0), seed=2)
    torch.cuda.synchronize()
    print("%s: loss %.3f -> %.3f, max|z| %.1f" % (case, float(l64[0]), float(l64[-1]), zmax))
    for name, got, r64, r32 in (("W", fit.weight, W64, W32), ("b", fit.bias, b64, b32), ("loss", fit.loss, l64, l32)):
        floor = float((r32.double() - r64).abs().max())
        bound = max(8 * floor, steps * U * float(r64.abs().max()))
        err = float((got.double().cpu() - r64).abs().max())
        print("%s: max|gpu - f64| %.3g, torch f32 floor %.3g, bound %.3g" % (name, err, floor, bound))
        assert err <= bound, (name, err, bound)
    assert float(l64[-1]) < 0.5 * float(l64[0])


# ---- 5. determinism and scheduling -------------------------------------------------------------------------------------------
def test_same_arguments_same_bits_other_seed_other_fit():
    E, y = data(2000, 50)
    Ed, yd = E.to(DEV), y.to(DEV)
    kw = dict(classes=50, loss="ce", label_smoothing=0.1, epochs=3, batch_size=256, lr=1e-3)
    a, b, c = fit_head(Ed, yd, **kw), fit_head(Ed, yd, **kw), fit_head(Ed, yd, seed=1, **kw)
    for p, q in ((a.weight, b.weight), (a.bias, b.bias), (a.loss, b.loss)):
        assert torch.equal(p, q)
    assert not torch.equal(a.weight, c.weight) and not torch.equal(a.loss, c.loss)
    assert a.loss.shape == (24,) and len(a.history) == 3
    onehot = F.one_hot(yd, 50)
    d = fit_head(Ed, onehot, **{**kw, "classes": None})                             # one-hot rows: the same labels, the same fit
    assert torch.equal(d.weight, a.weight) and torch.equal(d.loss, a.loss)
    bce = fit_head(Ed, onehot, epochs=1, batch_size=256, lr=1e-3)
    bce2 = fit_head(Ed, onehot, epochs=1, batch_size=256, lr=1e-3, loss="bce")
    assert torch.equal(bce.weight, bce2.weight) and torch.equal(bce.loss, bce2.loss) and not torch.equal(bce.loss[:8], a.loss[:8])


def test_captured_step_replays_the_eager_bits():
    E, y = data(2000, 50)
    W0, b0 = init(50)
    Ed, yd = E.to(DEV), y.to(DEV)
    idx = torch.randperm(2000, generator=torch.Generator().manual_seed(2))[:256].to(DEV)
    st, keep = fresh_state(W0, b0), fresh_state(W0, b0)
    hp = _ffi.adam()
    ws = workspace(256, 50)
    loss, status = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert call_step(Ed, yd, idx, st, hp, 1, 1e-3, loss, status, ws, eps=0.1) == 0, last_error()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in st.items()}
    eager_loss = loss.clone()
    for k in st:
        st[k].copy_(keep[k])
    loss.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                   # a linear graph: three kernels in a row
        rc = call_step(Ed, yd, idx, st, hp, 1, 1e-3, loss, status, ws, eps=0.1)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(st["W"], keep["W"])                                          # capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(st[k], eager[k]), k
    assert torch.equal(loss, eager_loss) and int(status) == 0 and float(loss) > 0


def make_model(sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def test_fit_on_a_side_stream_beside_a_forward(synth_sd):
    model = make_model(synth_sd)
    wav = synth.synth_waveforms(16, 2 * SR, seed=4).to(DEV)
    E, y = data(3000, 527)
    Ed, yd = E.to(DEV), y.to(DEV)
    kw = dict(classes=527, loss="ce", epochs=4, batch_size=512, lr=1e-3)
    alone = fit_head(Ed, yd, **kw)
    with torch.no_grad():
        ref = model(wav)["clipwise_logits"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        beside = fit_head(Ed, yd, **kw)
    with torch.no_grad():
        outs = [model(wav)["clipwise_logits"] for _ in range(6)]
    torch.cuda.synchronize()
    for p, q in ((alone.weight, beside.weight), (alone.bias, beside.bias), (alone.loss, beside.loss)):
        assert torch.equal(p, q)
    assert all(torch.equal(o, ref) for o in outs)


# ---- 6. bad labels and argument errors ---------------------------------------------------------------------------------------
def test_bad_labels_are_clamped_and_flagged():
    """E and the labels are the middle slices of larger buffers (NaN rows; labels that are themselves out of range) and the
    labels of batch rows 2 and 8 of 16 are -1 and N: a kernel without the clamp would read z one element outside those rows,
    which is still inside the (16, N) logits -- nothing here can leave an allocation."""
    n, N = 64, 10
    E, y = data(n, N)
    big = torch.full((3 * n, 768), float("nan"), device=DEV)
    bigy = torch.full((3 * n,), 10 ** 6, dtype=torch.int64, device=DEV)
    big[n:2 * n], bigy[n:2 * n] = E.to(DEV), y.to(DEV)
    Ed, yd = big[n:2 * n], bigy[n:2 * n]
    yd[3], yd[9] = -1, N
    W0, b0 = init(N)
    idx = torch.arange(1, 17, device=DEV)
    rc, z, G, dW, db, loss, status = call_grad(Ed, yd, idx, W0.to(DEV), b0.to(DEV), 0.1)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert int(status) == _ffi.FIT_BAD_LABEL
    for t in (z, G, dW, db, loss):
        assert bool(torch.isfinite(t).all())
    good = yd.clone()
    good[3], good[9] = 0, N - 1                                                    # what the clamp reads
    rc, z2, G2, dW2, db2, loss2, status2 = call_grad(Ed, good, idx, W0.to(DEV), b0.to(DEV), 0.1)
    torch.cuda.synchronize()
    assert int(status2) == 0
    for p, q in ((z, z2), (G, G2), (dW, dW2), (db, db2), (loss, loss2)):
        assert torch.equal(p, q)
    bad_idx = idx.clone()
    bad_idx[0], bad_idx[5] = -1, n                                                 # bad row numbers too: both flags
    st = fresh_state(W0, b0)
    lossb, statusb = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert call_step(Ed, yd, bad_idx, st, _ffi.adam(), 1, 1e-3, lossb, statusb, workspace(16, N)) == 0
    torch.cuda.synchronize()
    assert int(statusb) == _ffi.FIT_BAD_LABEL | _ffi.FIT_BAD_INDEX
    assert bool(torch.isfinite(st["W"]).all()) and bool(torch.isfinite(lossb).all())


def test_argument_errors_return_codes_without_a_launch():
    E, y = data(100, 10)
    W0, b0 = init(10)
    Ed, yd = E.to(DEV), y.to(DEV)
    idx = torch.arange(32, device=DEV)
    ws = workspace(32, 10)
    hp = _ffi.adam()
    loss, status = torch.full((1,), 7.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    st = fresh_state(W0, b0)
    cases = [({"E": None}, -1, "E"), ({"y": None}, -1, "labels"), ({"idx": None}, -1, "idx"), ({"W": None}, -1, "W"),
             ({"b": None}, -1, "b"), ({"mW": None}, -1, "mW"), ({"xW": None}, -1, "vmaxW"), ({"loss": None}, -1, "loss_out"),
             ({"status": None}, -1, "status"), ({"ws": None}, -1, "workspace"), ({"hp": None}, -1, "hp"),
             ({"rows": 0}, -1, "rows"), ({"N": 0}, -1, "classes"), ({"N": _ffi.MAX_CLASSES + 1}, -1, "classes"),
             ({"ld_e": 767}, -1, "ld_e"), ({"eps": 1.0}, -1, "label_smoothing"), ({"eps": -0.5}, -1, "label_smoothing"),
             ({"ws_bytes": ws[1] - 1}, -5, "workspace"), ({"ws": ctypes.c_void_p(ws[0].data_ptr() + 64)}, -5, "aligned"),
             ({"t": 0}, -1, "step_t"), ({"lr": -1.0}, -1, "lr"), ({"hp": ctypes.byref(_ffi.adam(beta1=1.0))}, -1, "beta1")]
    for over, code, word in cases:
        rc = call_step(Ed, yd, idx, st, hp, 1, 1e-3, loss, status, ws, over=over)
        assert rc == code and word in last_error(), (over, rc, last_error())
    for over, code, word in [({"z": None}, -1, "z"), ({"rows": 0}, -1, "rows"), ({"ld_e": 700}, -1, "ld_e"),
                             ({"eps": 1.5}, -1, "label_smoothing"), ({"ws_bytes": 0}, -5, "workspace")]:
        rc = call_grad(Ed, yd, idx, st["W"], st["b"], ws=ws, over=over)[0]
        assert rc == code and word in last_error(), (over, rc, last_error())
    torch.cuda.synchronize()
    assert torch.equal(st["W"].cpu(), W0) and float(loss) == 7.0 and int(status) == 0       # nothing ran
    assert float(st["mW"].abs().max()) == 0.0
    with pytest.raises(ValueError, match="label_smoothing"):
        fit_head(Ed, F.one_hot(yd, 10), label_smoothing=0.1)
    with pytest.raises(ValueError, match="outside"):
        fit_head(Ed, yd, loss="ce", classes=5)


# ---- 7. softmax_topk against the host definition -----------------------------------------------------------------------------
def topk_logits(rows, N, seed):
    """Rows at offsets up to +-80 with a spread of 60 inside a row (the smallest probability, e^-60 / N, stays a normal float32:
    a relative bound cannot hold for a result the format flushes), plus constructed ties."""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(rows, N, generator=g) * 60.0
    top = torch.tensor([80.0, 20.0, -20.0])[torch.arange(rows) % 3]
    z = z - 60.0 + top[:, None]
    if rows >= 3:
        z[1] = 3.25                                                               # a whole row equal: index order
        z[2] = torch.randint(-2, 3, (N,), generator=g).float()                   # few distinct values: ties straddle every rank
        z[2, ::2] *= -0.0 if N > 1 else 1.0                                       # ... and -0.0 beside +0.0 (the zeros of even columns)
    if rows >= 70:
        z[5] = torch.where(torch.rand(N, generator=g) < 0.5, 0.0, -0.0)          # +-0.0 only
        z[6, : N // 2] = z[6, N // 2: 2 * (N // 2)]                               # every value twice
    return z


@pytest.mark.parametrize("rows", [1, 3, 70])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 527, 2048, 2049, 4096, 32768])
def test_softmax_topk_against_host(N, rows):
    """probs within p_bound (delta = 0), row sums within (D + 4) u of 1, top_index exactly the host's (ties included), top_prob
    the bits of the gathered probs; ld > N; k in {1, 5, min(N, 64)}.  2048 / 2049: the last wave-shaped and the first
    workgroup-shaped row."""
    z = topk_logits(rows, N, 1000 * rows + N)
    buf = torch.full((rows, N + 5), float("nan"))
    buf[:, :N] = z
    zd = buf.to(DEV)[:, :N]
    assert zd.stride(0) == N + 5 and float(z.abs().max()) <= 80.0
    z64 = z.double()
    p64, dp = p_bound(z64, torch.zeros(rows, 1, dtype=torch.float64), N)
    D = _ffi.softmax_depth(N)
    for k in sorted({1, min(5, N), min(N, 64)}):
        status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        probs, top_prob, top_index = cl.softmax_topk(zd, k=k, status=status)
        torch.cuda.synchronize()
        assert int(status) == 0
        hp, htp, hti = cl.softmax_topk_host(z.numpy(), k=k)
        assert np.array_equal(top_index.cpu().numpy(), hti), (N, rows, k)
        err = (probs.double().cpu() - p64).abs()
        print("N %d rows %d k %d: p err/bound %.3g" % (N, rows, k, float((err / dp).max())))
        assert bool((err <= dp).all()), float((err - dp).max())
        assert np.allclose(hp, p64.numpy(), rtol=1e-12, atol=0)
        assert bool(((probs.double().sum(dim=1).cpu() - 1.0).abs() <= (D + 4) * U).all())
        assert torch.equal(top_prob, torch.gather(probs, 1, top_index.long()))
        none, tp2, ti2 = cl.softmax_topk(zd, k=k, probabilities=False)
        assert none is None and torch.equal(tp2, top_prob) and torch.equal(ti2, top_index)
    # a row's outputs depend on that row alone: each row as a batch of one, from a contiguous copy
    if rows > 1:
        for r in (0, rows // 2, rows - 1):
            p1, tp1, ti1 = cl.softmax_topk(zd[r:r + 1].clone(), k=k)
            assert torch.equal(p1[0], probs[r]) and torch.equal(tp1[0], top_prob[r]) and torch.equal(ti1[0], top_index[r])


def test_softmax_topk_nonfinite_rows():
    for N in (65, 4096):
        z = topk_logits(70, N, 5)
        zd = z.to(DEV)
        clean = cl.softmax_topk(zd, k=5)
        bad = z.clone()
        bad[4, N - 1], bad[9, 0], bad[69, N // 2] = float("nan"), float("inf"), float("-inf")
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        probs, top_prob, top_index = cl.softmax_topk(bad.to(DEV), k=5, status=status)
        torch.cuda.synchronize()
        assert int(status) == _ffi.CLASSIFY_NONFINITE
        rows_bad = torch.tensor([4, 9, 69])
        keep = torch.ones(70, dtype=torch.bool)
        keep[rows_bad] = False
        assert bool(torch.isnan(probs[rows_bad]).all()) and bool(torch.isnan(top_prob[rows_bad]).all())
        assert bool((top_index[rows_bad] == -1).all())
        for got, want in zip((probs, top_prob, top_index), clean):
            assert torch.equal(got[keep], want[keep])
    with pytest.raises(ValueError, match="k must be"):
        cl.softmax_topk(zd, k=65)
    with pytest.raises(ValueError, match="k must be"):
        cl.softmax_topk(zd[:, :3], k=4)
    with pytest.raises(ValueError, match="CUDA"):
        cl.softmax_topk(z, k=1)


# ---- 8. classification counts = the host's, exactly ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, 70001])
@pytest.mark.parametrize("N", [1, 2, 50, 527, 4096])
def test_classification_counts_equal_host(N, n):
    """Small-integer logits (ties at the maximum and at every rank, -0.0 beside +0.0) with ld > N, labels that include -1 and N,
    rows with a NaN or an infinity; outputs pre-filled with garbage.  Confusion at N <= 527, and once at 4096 (n = 1000)."""
    g = torch.Generator(device=DEV).manual_seed(n * 7 + N)
    buf = torch.randint(-3, 4, (n, N + 3), generator=g, device=DEV).float()
    buf[:, ::3] *= -1.0                                                            # turns a third of the zeros into -0.0
    zd = buf[:, :N]
    yd = torch.randint(0, N, (n,), generator=g, device=DEV)
    flags = 0
    if n >= 1000:
        yd[7], yd[n - 1] = -1, N
        zd[11, N - 1], zd[500, 0] = float("nan"), float("inf")
        flags = _ffi.CLASSIFY_NONFINITE | _ffi.CLASSIFY_BAD_LABEL
    z, y = zd.cpu().numpy(), yd.cpu().numpy()
    ranks = cl.prediction_and_rank_host(y, z)
    with_conf = N <= 527 or n == 1000
    for k in (1, 5):
        host = cl.classification_metrics_host(y, z, k=k, ranks=ranks)
        kk = min(k, N)
        per_class = torch.full((N, 3), -5, dtype=torch.int64, device=DEV)
        hits = torch.full((2,), 1 << 40, dtype=torch.int64, device=DEV)
        conf = torch.full((N, N), 9, dtype=torch.int64, device=DEV) if with_conf else None
        status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        _ffi.classification_counts(vp(zd), zd.stride(0), vp(yd), n, N, kk, vp(per_class), vp(hits), vp(conf), vp(status), stream())
        torch.cuda.synchronize()
        assert int(status) == flags
        assert np.array_equal(per_class.cpu().numpy(), host.per_class), (N, n, k)
        assert np.array_equal(hits.cpu().numpy(), host.hits), (N, n, k, hits, host.hits)
        if with_conf:
            assert np.array_equal(conf.cpu().numpy(), host.confusion)
        assert host.skipped == (4 if n >= 1000 else 0)
    m = cl.classification_metrics(yd, zd, k=5, confusion=with_conf)
    for name in ("accuracy", "topk_accuracy", "macro_f1", "balanced_accuracy"):
        assert getattr(m, name) == getattr(host, name), name
    assert np.array_equal(m.precision, host.precision) and np.array_equal(m.recall, host.recall) and np.array_equal(m.f1, host.f1)
    assert m.n == n and m.counted == n - host.skipped
    if flags:
        with pytest.raises(ValueError):
            m.check()
    else:
        assert m.check() is m


def test_classification_counts_errors():
    z = torch.zeros(4, 4097, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.zeros(4097 * 3 + 2, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _ffi.lib().acx_classification_counts(vp(z), 4097, vp(y), 4, 4097, 1, vp(out), vp(out[-2:]), vp(out), vp(status), stream())
    assert rc == -6 and "confusion" in last_error()
    with pytest.raises(ValueError, match="confusion"):
        cl.classification_metrics(y, z)
    m = cl.classification_metrics(y, z, confusion=False)                           # every logit 0: class 0 everywhere, all correct
    assert m.accuracy == 1.0 and m.confusion is None
    with pytest.raises(ValueError, match="labels"):
        cl.classification_metrics(y[:3], z, confusion=False)
    with pytest.raises(ValueError, match="integer"):
        cl.classification_metrics(y.float(), z, confusion=False)


# ---- 9. model level ----------------------------------------------------------------------------------------------------------
def test_model_fit_head_ce_and_classify(synth_sd, tmp_path):
    model = make_model(synth_sd)
    N = 5
    lens = [SR, 20000, SR + 777, 9000, 2 * SR, SR, 12345, 30000, SR, 25000]
    waves = [synth.synth_waveforms(1, L, seed=60 + i)[0] for i, L in enumerate(lens)]
    labels = torch.randint(0, N, (len(lens),), generator=torch.Generator().manual_seed(3))
    kw = dict(epochs=3, batch_size=4, lr=1e-2, seed=5, loss="ce", classes=N, label_smoothing=0.1)
    emb = torch.stack(extract(model, waves, what="scene", pack=True)).to(DEV)
    want = fit_head(emb, labels.to(DEV), **kw)
    fit = model.fit_head(waves, labels, **kw)
    for p, q in ((fit.weight, want.weight), (fit.bias, want.bias), (fit.loss, want.loss)):
        assert torch.equal(p, q)
    assert not model.training and model.head_audioset.out_features == N
    assert torch.equal(model.head_audioset.weight.data, fit.weight) and torch.equal(model.head_audioset.bias.data, fit.bias)
    x = synth.synth_waveforms(3, SR, seed=8).to(DEV)
    with torch.no_grad():
        out = model(x)
        res = model.classify(x, k=3)
    logits = out["clipwise_logits"]
    probs, top_prob, top_index = cl.softmax_topk(logits, k=3)
    assert torch.equal(res["clipwise_logits"], logits) and torch.equal(res["probabilities"], probs)
    assert torch.equal(res["top_probabilities"], top_prob) and torch.equal(res["top_indices"], top_index)
    assert torch.equal(res["labels"], top_index[:, 0].long()) and res["labels"].dtype == torch.int64
    assert torch.equal(out["clipwise_output"], torch.sigmoid(logits)) or bool(
        ((out["clipwise_output"].double() - torch.sigmoid(logits.double())).abs() <= 4 * U).all())     # still the sigmoid
    assert float((res["probabilities"].sum(dim=1) - 1).abs().max()) <= (_ffi.softmax_depth(N) + 4) * U
    assert model.classify(x, k=99)["top_indices"].shape == (3, N)                   # k is cut to N
    assert len(model.state_dict()) == 190
    # a saved and reloaded checkpoint classifies identically
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.save({"model": sd}, str(tmp_path / "head.pth"))
    loaded = ConvNeXt.from_pretrained(str(tmp_path / "head.pth")).to(DEV).eval()
    with torch.no_grad():
        res2 = loaded.classify(x, k=3)
    for key in res:
        assert torch.equal(res2[key], res[key]), key
    # 44.1 kHz input
    x44 = synth.synth_waveforms(2, 44100, seed=9).to(DEV)
    with torch.no_grad():
        r44 = model.classify(x44, k=2, sample_rate=44100)
        l44 = model(x44, sample_rate=44100)["clipwise_logits"]
    assert torch.equal(r44["clipwise_logits"], l44) and torch.equal(r44["top_indices"], cl.softmax_topk(l44, k=2)[2])
    waves44 = [synth.synth_waveforms(1, L, seed=90 + i)[0] for i, L in enumerate([44100, 30000, 50000, 44100])]
    m44 = make_model(synth_sd)
    f44 = m44.fit_head(waves44, labels[:4], sample_rate=44100, **kw)
    e44 = torch.stack(extract(make_model(synth_sd), waves44, what="scene", pack=True, sample_rate=44100)).to(DEV)
    w44 = fit_head(e44, labels[:4].to(DEV), **kw)
    assert torch.equal(f44.weight, w44.weight) and torch.equal(f44.loss, w44.loss)
    # loss="bce" is the call without the argument
    target = torch.rand(len(lens), N, generator=torch.Generator().manual_seed(3)) < 0.4
    a = fit_head(emb, target.to(DEV), epochs=2, batch_size=4, lr=1e-2, seed=5)
    b = fit_head(emb, target.to(DEV), epochs=2, batch_size=4, lr=1e-2, seed=5, loss="bce")
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias) and torch.equal(a.loss, b.loss)


def test_validation_history_ce():
    E, y = data(1000, 20)
    Ev, yv = data(400, 20, seed=0)                                                  # the same prototypes
    Ev, yv = Ev[200:], yv[200:]
    Ed, yd, Evd, yvd = E.to(DEV), y.to(DEV), Ev.to(DEV), yv.to(DEV)
    kw = dict(batch_size=128, lr=1e-3, seed=3, loss="ce", classes=20)
    fit = fit_head(Ed, yd, epochs=3, val=(Evd, yvd), **kw)
    assert len(fit.history) == 3
    for e in range(3):
        part = fit_head(Ed, yd, epochs=e + 1, **kw)
        m = cl.classification_metrics(yvd, torch.addmm(part.bias, Evd, part.weight.t()), k=5, confusion=False)
        for k in ("accuracy", "topk_accuracy", "macro_f1"):
            assert fit.history[e][k] == getattr(m, k), (e, k)
    assert fit.history[2]["accuracy"] >= fit.history[0]["accuracy"] and fit.history[2]["topk_accuracy"] >= fit.history[2]["accuracy"]
