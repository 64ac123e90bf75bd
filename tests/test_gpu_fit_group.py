"""GPU (`-m gpu`): group fits (pytorch/finetune.py fit_heads / cross_validate_head, acx_head_fit_group_step in include/acx.h).
The yardstick needs no tolerance: the fit kernels are deterministic, so every head of a group must equal, bit for bit
(torch.equal on weight, bias and loss), the fit_head call it replaces -- whatever tile form the job's own single call takes,
however many steps the job sits out, whatever its neighbours do."""
import ctypes

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch import finetune as ft
from audioset_convnext_inf_amd.pytorch._inputs import target_code
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
from audioset_convnext_inf_amd.pytorch.finetune import cross_validate_head, fit_head, fit_heads, kfold_ids

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}


def data(n, N, seed=0):
    """Random fp32 embeddings with multi-label targets (bool) and single labels, on the device; made once per shape."""
    key = (n, N, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(seed)
        E = torch.randn(n, 768, generator=g)
        Y = torch.rand(n, N, generator=g) < 0.3
        lab = torch.randint(0, N, (n,), generator=g)
        _cache[key] = (E.to(DEV), Y.to(DEV), lab.to(DEV))
    return _cache[key]


def target_of(n, N, kind):
    E, Y, lab = data(n, N)
    if kind == "u8":
        return E, Y.to(torch.uint8), dict(loss="bce")
    if kind == "f32":
        return E, Y.float() * 0.9 + 0.05, dict(loss="bce")                                # soft targets
    return E, lab, dict(loss="ce", classes=N, label_smoothing=0.1 if kind == "ce_smooth" else 0.0)


def single(E, T, job, **shared):
    """The fit_head call that a job of fit_heads replaces."""
    rows = job.get("rows")
    kw = {k: v for k, v in job.items() if k not in ("rows", "val")}
    return fit_head(E if rows is None else E[rows.to(DEV)], T if rows is None else T[rows.to(DEV)], **kw, **shared)


def assert_same(got, want, what=""):
    assert got.weight.shape == want.weight.shape and got.loss.shape == want.loss.shape, what
    assert torch.equal(got.weight, want.weight), what
    assert torch.equal(got.bias, want.bias), what
    assert torch.equal(got.loss, want.loss), what


def fold_jobs(n, folds, settings):
    ids = kfold_ids(n, folds, seed=3)
    return [dict(settings[f % len(settings)], rows=torch.nonzero(ids != f).reshape(-1)) for f in range(folds)]


# ---- 1. equality with fit_head -------------------------------------------------------------------------------------------------
SETTINGS = [dict(lr=1e-3, weight_decay=0.0, seed=1), dict(lr=3e-3, weight_decay=0.1, seed=2), dict(lr=1e-2, weight_decay=0.01, seed=3),
            dict(lr=3e-4, weight_decay=0.3, seed=4, betas=(0.8, 0.99)), dict(lr=2e-3, weight_decay=0.05, seed=5, eps=1e-6)]


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("kind", ["u8", "f32", "ce", "ce_smooth"])
@pytest.mark.parametrize("N", [1, 10, 50, 527])
def test_five_folds_equal_fit_head(N, kind, amsgrad, decoupled):
    E, T, shared = target_of(161, N, kind)
    shared.update(epochs=2, batch_size=64, amsgrad=amsgrad, decoupled=decoupled)
    jobs = fold_jobs(161, 5, SETTINGS)
    sizes = sorted(int(j["rows"].numel()) for j in jobs)
    assert sizes == [128, 129, 129, 129, 129]                       # 2 and 3 steps per epoch: one job sits steps out
    fits = fit_heads(E, T, jobs, **shared)
    assert len(fits) == 5
    for j, job in enumerate(jobs):
        want = single(E, T, job, **shared)
        assert fits[j].loss.shape == (2 * (2 if job["rows"].numel() == 128 else 3),)
        assert_same(fits[j], want, j)
        assert [r["epoch"] for r in fits[j].history] == [0, 1]
        assert torch.equal(torch.stack([r["loss"] for r in fits[j].history]), torch.stack([r["loss"] for r in want.history]))


# ---- 2. both tile forms in one step --------------------------------------------------------------------------------------------
def test_both_tile_forms_in_one_step():
    """N = 527, batch 512: a full batch takes 32 x 32 tiles on a 256-CU part, the short last batch of 88 rows 16 x 16.  In the
    second step of each epoch the first job runs 512 rows and the second 88."""
    E, Y, _ = data(1100, 527)
    g = torch.Generator().manual_seed(5)
    jobs = [dict(rows=torch.randperm(1100, generator=g)[:1024], lr=1e-3, seed=1),
            dict(rows=torch.randperm(1100, generator=g)[:600], lr=2e-3, weight_decay=0.1, seed=2)]
    assert ft.group_schedule([1024, 600], 2, 512).tolist() == [[512, 512], [512, 88]] * 2
    shared = dict(epochs=2, batch_size=512)
    fits = fit_heads(E, Y, jobs, **shared)
    for j, job in enumerate(jobs):
        assert_same(fits[j], single(E, Y, job, **shared), j)


@pytest.mark.parametrize("kind", ["u8", "ce"])
def test_wide_head_two_jobs(kind):
    """N = 4 096, batch 256: BCE takes 32 x 32 tiles for 33 rows and more, 16 x 16 for the last batch of 20; the cross-entropy
    row pass runs its one-workgroup-per-row shape (N > 2 048)."""
    E, T, shared = target_of(1100, 4096, kind)
    g = torch.Generator().manual_seed(6)
    jobs = [dict(rows=torch.randperm(1100, generator=g)[:512], lr=1e-3, seed=1),
            dict(rows=torch.randperm(1100, generator=g)[:276], lr=3e-3, seed=2)]
    shared.update(epochs=1, batch_size=256)
    fits = fit_heads(E, T, jobs, **shared)
    for j, job in enumerate(jobs):
        assert_same(fits[j], single(E, T, job, **shared), j)


# ---- 3. groups -----------------------------------------------------------------------------------------------------------------
def test_one_job_and_all_rows():
    E, Y, lab = data(161, 50)
    for T, shared in ((Y, dict(loss="bce")), (lab, dict(loss="ce", classes=50))):
        shared.update(epochs=2, batch_size=64)
        job = dict(lr=1e-3, seed=4)                                  # rows=None: every row
        (fit,) = fit_heads(E, T, [job], **shared)
        assert_same(fit, fit_head(E, T, lr=1e-3, seed=4, **shared))
        init = (fit.weight.clone(), fit.bias.cpu())                  # continue from a head: init on either device
        (more,) = fit_heads(E, T, [dict(job, init=init)], **shared)
        assert_same(more, fit_head(E, T, lr=1e-3, seed=4, init=init, **shared))
    (none,) = fit_heads(E, Y, [dict(seed=4)], epochs=0)
    want = fit_head(E, Y, seed=4, epochs=0)
    assert_same(none, want)
    assert none.history == [] and none.loss.shape == (0,)


def test_neighbours_do_not_matter():
    E, Y, _ = data(161, 10)
    A, B, C = fold_jobs(161, 3, SETTINGS)
    shared = dict(epochs=2, batch_size=32, drop_last=True)
    abc = fit_heads(E, Y, [A, B, C], **shared)
    ca = fit_heads(E, Y, [C, A], **shared)
    assert_same(abc[0], ca[1], "A")
    assert_same(abc[2], ca[0], "C")
    assert_same(abc[1], single(E, Y, B, **shared), "B")
    plain = fit_heads(E, Y, [A, B], epochs=2, batch_size=32, shuffle=False)
    assert_same(plain[1], single(E, Y, B, epochs=2, batch_size=32, shuffle=False))


def test_more_jobs_than_a_group_holds():
    E, Y, _ = data(40, 1)
    g = torch.Generator().manual_seed(8)
    kinds = [dict(rows=torch.randperm(40, generator=g)[:m], lr=lr, seed=s) for m, lr, s in ((40, 1e-3, 1), (33, 1e-2, 2), (17, 3e-3, 3))]
    jobs = [kinds[j % 3] for j in range(_ffi.FIT_MAX_JOBS + 2)]
    jobs[-1] = dict(rows=torch.arange(5, 40), lr=5e-3, seed=9)        # the second group's own
    shared = dict(epochs=1, batch_size=64)
    fits = fit_heads(E, Y, jobs, **shared)
    assert len(fits) == _ffi.FIT_MAX_JOBS + 2
    want = [single(E, Y, k, **shared) for k in kinds]
    for j, fit in enumerate(fits[:-1]):
        assert_same(fit, want[j % 3], j)
    assert_same(fits[-1], single(E, Y, jobs[-1], **shared), "last")


# ---- 4. per-step learning rates ------------------------------------------------------------------------------------------------
def test_lr_sequences_per_job():
    E, _, lab = data(161, 10)
    jobs = fold_jobs(161, 5, [dict(seed=1), dict(seed=2)])
    for j, job in enumerate(jobs):
        steps = 2 * (2 if job["rows"].numel() == 128 else 3)
        job["lr"] = [1e-3 * (1 + j) * 0.9 ** t for t in range(steps)] if j != 2 else 2e-3
    assert sorted({len(j["lr"]) for j in jobs if isinstance(j["lr"], list)}) == [4, 6]
    shared = dict(epochs=2, batch_size=64, loss="ce", classes=10)
    fits = fit_heads(E, lab, jobs, **shared)
    for j, job in enumerate(jobs):
        assert_same(fits[j], single(E, lab, job, **shared), j)


# ---- the C entries, called directly ------------------------------------------------------------------------------------------------
def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Group:
    """A group of J jobs set up by hand: batches[j] is the list of the job's batches (int64 index tensors; an empty one: the job
    sits that step out)."""

    def __init__(self, E, Y, batches, N, ce=False, lr=1e-3, wd=0.0):
        self.E, self.Y, self.N, self.ce = E, Y, N, ce
        self.J, self.steps = len(batches), len(batches[0])
        self.rows = np.array([[b[s].numel() for b in batches] for s in range(self.steps)], dtype=np.int32)
        self.rows_max = int(self.rows.max())
        off = np.zeros_like(self.rows, dtype=np.int64)
        for j, b in enumerate(batches):
            off[:, j] = np.cumsum([0] + [x.numel() for x in b[:-1]])
        self.idx = [torch.cat(b).to(DEV) for b in batches]
        self.hps = [_ffi.adam(0.9, 0.999, 1e-8, wd * j, True, False) for j in range(self.J)]
        self.lr = np.array([[lr * (1 + j) for j in range(self.J)]] * self.steps)
        self.code = _ffi.FIT_LOSS_CE if ce else _ffi.FIT_LOSS_BCE
        self.plan = torch.from_numpy(_ffi.head_fit_plan(self.rows, off, self.lr, self.hps, self.rows_max, N, self.code)).to(DEV)
        g = torch.Generator().manual_seed(1)
        self.st = {"W": (torch.randn(self.J, N, 768, generator=g) * 0.02).to(DEV), "b": torch.zeros(self.J, N, device=DEV),
                   "mom": torch.zeros(self.J, 3, N, 768, device=DEV), "momb": torch.zeros(self.J, 3, N, device=DEV),
                   "loss": torch.zeros(self.J, self.steps, device=DEV)}
        self.status = torch.zeros(self.J, dtype=torch.int32, device=DEV)
        table = (_ffi.AcxFitJob * self.J)()
        for j in range(self.J):
            t, s = table[j], self.st
            t.idx, t.W, t.b, t.loss = self.idx[j].data_ptr(), s["W"][j].data_ptr(), s["b"][j].data_ptr(), s["loss"][j].data_ptr()
            t.mW, t.vW, t.vmaxW = (s["mom"][j, k].data_ptr() for k in range(3))
            t.mb, t.vb, t.vmaxb = (s["momb"][j, k].data_ptr() for k in range(3))
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
        self.ws_bytes = _ffi.head_fit_group_workspace_bytes(self.J, self.rows_max, N, self.code)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)

    def step(self, s, **over):
        a = dict(E=vp(self.E), ld_e=self.E.stride(0), n=self.E.shape[0], Y=vp(self.Y), jobs=self.J, rows_max=self.rows_max,
                 N=self.N, table=vp(self.table), plan=vp(self.plan), steps=self.steps, step=s, status=vp(self.status),
                 ws=vp(self.ws), ws_bytes=self.ws_bytes, dtype=None if self.ce else target_code(self.Y),
                 ld_y=None if self.ce else self.Y.stride(0), smooth=0.0)
        a.update(over)
        stream = _ffi.stream_ptr(torch.device(DEV))
        if self.ce:
            return _ffi.lib().acx_head_fit_group_step_ce(a["E"], a["ld_e"], a["n"], a["Y"], a["jobs"], a["rows_max"], a["N"], a["smooth"],
                                                         a["table"], a["plan"], a["steps"], a["step"], a["status"], a["ws"],
                                                         a["ws_bytes"], stream)
        return _ffi.lib().acx_head_fit_group_step(a["E"], a["ld_e"], a["n"], a["Y"], a["dtype"], a["ld_y"], a["jobs"], a["rows_max"],
                                                  a["N"], a["table"], a["plan"], a["steps"], a["step"], a["status"], a["ws"],
                                                  a["ws_bytes"], stream)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.st.items()}

    def restore(self, snap):
        for k, v in snap.items():
            self.st[k].copy_(v)
        torch.cuda.synchronize()


def last_error():
    return _ffi.lib().acx_last_error().decode()


def some_batches(n, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n, generator=g)[:m] for m in sizes]


# ---- 5. graph capture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ce", [False, True])
def test_captured_group_step_replays_the_eager_bits(ce):
    E, Y, lab = data(161, 50)
    grp = Group(E, lab if ce else Y.float(), [some_batches(161, (64, 64), 1), some_batches(161, (64, 0), 2),
                                              some_batches(161, (40, 64), 3)], 50, ce=ce)
    start = grp.snapshot()
    assert grp.step(0) == 0, last_error()
    first = grp.snapshot()
    assert grp.step(1) == 0, last_error()
    eager = grp.snapshot()
    assert not torch.equal(eager["W"][0], first["W"][0]) and torch.equal(eager["W"][1], first["W"][1])
    grp.restore(first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # captured on a side stream
        rc = grp.step(1)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert torch.equal(grp.st["W"], first["W"])                      # capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(grp.st[k], eager[k]), k
    assert grp.status.tolist() == [0, 0, 0]
    assert not torch.equal(start["W"], eager["W"])


# ---- 6. status -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ce", [False, True])
def test_a_bad_index_is_clamped_and_flagged_in_its_own_word(ce):
    E, Y, lab = data(161, 10)
    T = lab if ce else Y.float()
    clean = [some_batches(161, (33, 20), 1), some_batches(161, (33, 33), 2), some_batches(161, (17, 33), 3)]
    bad = [[b.clone() for b in job] for job in clean]
    bad[1][0][5], bad[1][1][0] = 161 + 7, -3
    clamped = [[b.clone() for b in job] for job in clean]
    clamped[1][0][5], clamped[1][1][0] = 160, 0
    out = []
    for batches in (clean, bad, clamped):
        grp = Group(E, T, batches, 10, ce=ce, wd=0.1)
        for s in range(2):
            assert grp.step(s) == 0, last_error()
        out.append((grp.snapshot(), grp.status.tolist()))
    (c, cs), (b, bs), (k, ks) = out
    assert cs == [0, 0, 0] and ks == [0, 0, 0] and bs == [0, _ffi.FIT_BAD_INDEX, 0]
    for name in c:
        assert torch.equal(b[name][0], c[name][0]) and torch.equal(b[name][2], c[name][2]), name      # the neighbours
        assert torch.equal(b[name][1], k[name][1]), name                                               # clamped, not dropped
    assert not torch.equal(b["W"][1], c["W"][1])


def test_a_bad_label_is_flagged_in_its_own_word():
    E, _, lab = data(161, 10)
    lab = lab.clone()
    batches = [[torch.arange(0, 30)], [torch.arange(30, 60)], [torch.arange(60, 90)]]
    lab[70] = 10
    grp = Group(E, lab, batches, 10, ce=True)
    assert grp.step(0) == 0, last_error()
    torch.cuda.synchronize()
    assert grp.status.tolist() == [0, 0, _ffi.FIT_BAD_LABEL]


# ---- 7. cross_validate_head ----------------------------------------------------------------------------------------------------
def separable(n, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, N, (n,), generator=g)
    means = torch.randn(N, 768, generator=g)
    return (means[lab] * 0.5 + torch.randn(n, 768, generator=g)).to(DEV), lab.to(DEV)


def test_cross_validation_single_label():
    E, lab = separable(203, 4)
    settings = dict(loss="ce", classes=4, epochs=3, batch_size=32)
    cv = cross_validate_head(E, lab, folds=5, grid={"lr": [1e-5, 1e-2], "weight_decay": [0.0, 0.1]}, seed=2, **settings)
    assert cv.metric == "accuracy" and cv.scores.shape == (4, 5) and cv.scores.dtype == np.float64
    assert [(c["lr"], c["weight_decay"]) for c in cv.configs] == [(1e-5, 0.0), (1e-5, 0.1), (1e-2, 0.0), (1e-2, 0.1)]
    assert torch.equal(cv.fold_ids, kfold_ids(203, 5, 2, lab))       # stratified by default for ce
    for c, cfg in enumerate(cv.configs):
        for f in range(5):
            tr, te = (cv.fold_ids != f).to(DEV), (cv.fold_ids == f).to(DEV)
            want = fit_head(E[tr], lab[tr], val=(E[te], lab[te]), **cfg)
            assert_same(cv.fits[c][f], want, (c, f))
            assert cv.scores[c, f] == want.history[-1]["accuracy"], (c, f)
    assert np.array_equal(cv.mean, cv.scores.mean(axis=1)) and np.array_equal(cv.std, cv.scores.std(axis=1))
    assert cv.best == ft.select_best(cv.mean) and cv.best in (2, 3)  # the useful learning rate wins
    assert cv.mean[cv.best] > 0.9 and cv.mean[cv.best] == np.nanmax(cv.mean)
    assert_same(cv.final, fit_head(E, lab, **cv.configs[cv.best]))
    other = cross_validate_head(E, lab, folds=5, grid=[{"lr": 1e-2}], seed=2, refit=False, keep_fits=False, metric="macro_f1",
                                stratify=False, **settings)
    assert other.final is None and other.fits is None and other.metric == "macro_f1" and other.best == 0
    assert torch.equal(other.fold_ids, kfold_ids(203, 5, 2))


def test_cross_validation_multi_label_and_shared_grid():
    E, lab = separable(150, 3, seed=1)
    Y = torch.nn.functional.one_hot(lab, 3).bool()
    Y[torch.arange(0, 150, 7), 0] = True
    ids = torch.arange(150) % 3
    grid = [{"lr": 1e-2, "batch_size": 32}, {"lr": 1e-2}, {"lr": 1e-3, "batch_size": 32, "seed": 4}]
    cv = cross_validate_head(E, Y, folds=3, grid=grid, fold_ids=ids, epochs=2, batch_size=64, decoupled=True, weight_decay=0.01)
    assert cv.metric == "mAP" and cv.scores.shape == (3, 3) and torch.equal(cv.fold_ids, ids)
    for c, cfg in enumerate(cv.configs):
        assert cfg["decoupled"] is True and cfg["batch_size"] == (64 if c == 1 else 32) and cfg["seed"] == (4 if c == 2 else 0)
        for f in range(3):
            tr, te = (ids != f).to(DEV), (ids == f).to(DEV)
            want = fit_head(E[tr], Y[tr], val=(E[te], Y[te]), **cfg)
            assert_same(cv.fits[c][f], want, (c, f))
            assert cv.scores[c, f] == want.history[-1]["mAP"], (c, f)
    assert cv.best == ft.select_best(cv.mean)
    assert_same(cv.final, fit_head(E, Y, **cv.configs[cv.best]))


def test_model_cross_validate_head_installs_the_final_head(synth_sd):
    model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    model.load_state_dict(synth_sd)
    model = model.to(DEV).eval()
    E, lab = separable(60, 3, seed=2)
    kw = dict(folds=3, grid={"lr": [1e-3, 1e-2]}, loss="ce", classes=3, epochs=2, batch_size=16)
    want = cross_validate_head(E, lab, **kw)
    before = model.head_audioset.weight.clone()
    kept = model.cross_validate_head(E, lab.cpu(), install=False, **kw)
    assert torch.equal(model.head_audioset.weight, before) and kept.best == want.best
    cv = model.cross_validate_head(E, lab.cpu(), **kw)
    assert cv.best == want.best and np.array_equal(cv.scores, want.scores)
    assert_same(cv.final, want.final)
    assert model.head_audioset.out_features == 3 and not model.head_audioset.training
    assert torch.equal(model.head_audioset.weight.data, cv.final.weight) and torch.equal(model.head_audioset.bias.data, cv.final.bias)
    x = synth.synth_waveforms(2, 32000, seed=8).to(DEV)
    with torch.no_grad():
        out = model(x)["clipwise_logits"]
        scene = model.forward_scene_embeddings(x)
    assert out.shape == (2, 3)
    e, w64, b64 = scene.double().cpu(), cv.final.weight.double().cpu(), cv.final.bias.double().cpu()
    bound = 768 * 2.0 ** -24 * (e.abs() @ w64.abs().T) + 2.0 ** -24 * b64.abs()
    assert bool(((out.double().cpu() - (e @ w64.T + b64)).abs() <= bound).all())


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ce", [False, True])
def test_argument_errors_return_codes_without_a_launch(ce):
    E, Y, lab = data(161, 10)
    grp = Group(E, lab if ce else Y.float(), [some_batches(161, (33, 20), 1), some_batches(161, (33, 33), 2)], 10, ce=ce)
    before = grp.snapshot()
    cases = [(dict(E=None), "E is null"), (dict(Y=None), "is null"), (dict(table=None), "jobs is null"), (dict(plan=None), "plan is null"),
             (dict(status=None), "status is null"), (dict(ws=None), "workspace is null"), (dict(jobs=0), "jobs = 0"),
             (dict(jobs=_ffi.FIT_MAX_JOBS + 1), "jobs = 257"), (dict(rows_max=0), "rows = 0"), (dict(N=0), "classes = 0"),
             (dict(N=_ffi.MAX_CLASSES + 1), "classes"), (dict(steps=0), "n_steps"), (dict(step=2), "step = 2"), (dict(step=-1), "step = -1"),
             (dict(n=0), "n_rows_total"), (dict(ld_e=767), "ld_e"), (dict(ld_e=770), "multiple of 4"),
             (dict(E=ctypes.c_void_p(E.data_ptr() + 4)), "16-byte"), (dict(ws_bytes=grp.ws_bytes - 1), "workspace"),
             (dict(ws=ctypes.c_void_p(grp.ws.data_ptr() + 16)), "aligned")]
    cases += [(dict(smooth=1.0), "label_smoothing"), (dict(smooth=-0.1), "label_smoothing")] if ce else \
             [(dict(dtype=7), "target_dtype"), (dict(ld_y=9), "ld_target")]
    for over, text in cases:
        rc = grp.step(0, **over)
        assert rc < 0 and text in last_error(), (over, rc, last_error())
    after = grp.snapshot()
    for k in before:
        assert torch.equal(after[k], before[k]), k
    assert grp.status.tolist() == [0, 0]
    assert grp.step(0) == 0, last_error()
    assert not torch.equal(grp.snapshot()["W"], before["W"])
