"""CPU: the host side of group fits (pytorch/finetune.py fit_heads / kfold_ids / cross_validate_head, acx_head_fit_plan_* and
acx_head_fit_group_* in include/acx.h) -- the fold assignment against its definition, the group schedule against per-job
epoch_batches, grid expansion and partitioning, the choice of the best config, the plan (host only: the optimiser scalars and step
counts of every (step, job)), the ValueErrors that come before the GPU-only one, and the C ABI's declarations."""
import ctypes
import os

import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import finetune as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- kfold_ids -----------------------------------------------------------------------------------------------------------------
def kfold_definition(n, folds, seed, labels=None):
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    if labels is not None:
        perm = sorted(perm, key=lambda r: int(labels[r]))             # Python's sort is stable
    ids = [None] * n
    for i, r in enumerate(perm):
        ids[r] = i % folds
    return torch.tensor(ids)


def test_kfold_hand_worked():
    # randperm(11) with seed 0 is [10, 0, 4, 3, 5, 8, 2, 1, 9, 7, 6]: row perm[i] goes to fold i % 3
    assert torch.randperm(11, generator=torch.Generator().manual_seed(0)).tolist() == [10, 0, 4, 3, 5, 8, 2, 1, 9, 7, 6]
    assert ft.kfold_ids(11, 3, seed=0).tolist() == [1, 1, 0, 0, 2, 1, 1, 0, 2, 2, 0]
    # stratified: perm sorted stably by label is 0 3 8 9 6 | 10 4 1 7 | 5 2, dealt 0 1 2 0 1 | 2 0 1 2 | 0 1
    labels = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 0, 0, 1])
    assert ft.kfold_ids(11, 3, seed=0, labels=labels).tolist() == [0, 1, 1, 1, 0, 0, 1, 2, 2, 0, 2]


@pytest.mark.parametrize("n,folds,classes", [(11, 3, 3), (161, 5, 7), (400, 10, 50), (50, 50, 2), (97, 4, 1)])
def test_kfold_balance_and_definition(n, folds, classes):
    labels = torch.randint(0, classes, (n,), generator=torch.Generator().manual_seed(n))
    for seed in (0, 7):
        plain = ft.kfold_ids(n, folds, seed)
        assert plain.dtype == torch.int64 and plain.shape == (n,) and plain.device.type == "cpu"
        assert torch.equal(plain, kfold_definition(n, folds, seed))
        sizes = torch.bincount(plain, minlength=folds)
        assert int(sizes.max() - sizes.min()) <= 1 and int(sizes.min()) >= 1
        strat = ft.kfold_ids(n, folds, seed, labels)
        assert torch.equal(strat, kfold_definition(n, folds, seed, labels))
        sizes = torch.bincount(strat, minlength=folds)
        assert int(sizes.max() - sizes.min()) <= 1
        for c in range(classes):
            per = torch.bincount(strat[labels == c], minlength=folds)
            assert int(per.max() - per.min()) <= 1, c
        assert torch.equal(strat, ft.kfold_ids(n, folds, seed, labels))                   # deterministic per seed
    assert not torch.equal(ft.kfold_ids(n, folds, 0), ft.kfold_ids(n, folds, 7)) or n == folds == 1


def test_kfold_errors():
    for n, folds in ((10, 1), (10, 11), (0, 2), (10, 2.0), (10, True)):
        with pytest.raises(ValueError):
            ft.kfold_ids(n, folds)
    with pytest.raises(ValueError, match="multi-label"):
        ft.kfold_ids(10, 2, labels=torch.zeros(10, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ft.kfold_ids(10, 2, labels=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer"):
        ft.kfold_ids(10, 2, labels=torch.zeros(10))


# ---- group_schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,epochs,batch,drop_last", [
    ([128, 129, 129, 128, 129], 2, 64, False),        # 2 and 3 steps per epoch: the short jobs sit the third step out
    ([128, 129], 3, 64, True),
    ([1024, 600], 1, 512, False),
    ([40], 4, 64, False),
    ([10, 70, 200], 2, 64, True),                      # a job with no full batch never runs
    ([5, 6], 0, 4, False),
])
def test_group_schedule_equals_per_job_batches(sizes, epochs, batch, drop_last):
    rows = ft.group_schedule(sizes, epochs, batch, drop_last)
    per = [ft.epoch_batches(m, batch, drop_last) for m in sizes]
    spe = max(len(b) for b in per)
    assert rows.dtype == np.int32 and rows.shape == (epochs * spe, len(sizes))
    for j, b in enumerate(per):
        want = ([r for _, r in b] + [0] * (spe - len(b))) * epochs
        assert rows[:, j].tolist() == want
        assert int((rows[:, j] > 0).sum()) == epochs * len(b)                             # the job's own step count


# ---- grids ---------------------------------------------------------------------------------------------------------------------
def test_grid_expansion_order():
    assert ft.expand_grid(None) == [{}]
    got = ft.expand_grid({"lr": [1e-3, 1e-2], "weight_decay": [0.0, 0.1, 0.2]})
    assert got == [{"lr": a, "weight_decay": b} for a in (1e-3, 1e-2) for b in (0.0, 0.1, 0.2)]
    got = ft.expand_grid({"weight_decay": [0.0, 0.1], "lr": [1e-3, 1e-2]})
    assert got == [{"weight_decay": b, "lr": a} for b in (0.0, 0.1) for a in (1e-3, 1e-2)]
    listed = [{"lr": 1e-3}, {"lr": 1e-2, "betas": (0.8, 0.9)}]
    assert ft.expand_grid(listed) == listed and ft.expand_grid(listed) is not listed
    for bad in ({"lr": []}, {"lr": 1e-3}, {"init": [None]}, [], [1, 2], "lr", [{"val": None}]):
        with pytest.raises(ValueError):
            ft.expand_grid(bad)


def test_grid_partition_by_shared_settings():
    configs = ft.expand_grid({"lr": [1e-3, 1e-2], "label_smoothing": [0.0, 0.1], "weight_decay": [0.0, 0.5]})
    parts = ft.partition_configs(configs)
    assert parts == [({"label_smoothing": 0.0}, [0, 1, 4, 5]), ({"label_smoothing": 0.1}, [2, 3, 6, 7])]
    assert ft.partition_configs(ft.expand_grid({"lr": [1.0, 2.0], "seed": [0, 1]})) == [({}, [0, 1, 2, 3])]
    parts = ft.partition_configs([{"batch_size": 32}, {"lr": 1.0}, {"batch_size": 32, "decoupled": True}, {"batch_size": 32}])
    assert parts == [({"batch_size": 32}, [0, 3]), ({}, [1]), ({"batch_size": 32, "decoupled": True}, [2])]
    assert set(ft.GRID_JOB_KEYS) == {"lr", "weight_decay", "betas", "eps", "seed"}


def test_select_best_ties_and_nan():
    nan = float("nan")
    assert ft.select_best([0.1, 0.5, 0.3]) == 1
    assert ft.select_best([0.5, 0.5, 0.3]) == 0
    assert ft.select_best([0.2, 0.5, 0.5]) == 1
    assert ft.select_best([nan, 0.1, nan, 0.1]) == 1
    assert ft.select_best([nan, -1.0]) == 1
    assert ft.select_best([nan, nan]) is None
    assert ft.select_best(np.array([0.25, nan, 0.75])) == 2


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def plan_fields(plan):
    """The entries of a plan as (rows, idx_off, loss_slot, inv, scalars (9 floats), amsgrad), by their 64-byte layout."""
    e = plan.reshape(-1, 64)
    i32, f32 = e.view(np.int32), e.view(np.float32)
    return i32[:, 2], e.view(np.int64)[:, 0], i32[:, 3], f32[:, 4], f32[:, 6:15], i32[:, 15]


def test_plan_counts_a_jobs_own_steps():
    rows = ft.group_schedule([128, 129], 2, 64)                       # job 0 sits steps 2 and 5 out
    off = np.arange(rows.size, dtype=np.int64).reshape(rows.shape)
    lr = np.full(rows.shape, 1e-3)
    lr[:, 1] = np.linspace(1e-3, 2e-3, rows.shape[0])
    hps = [_ffi.adam(0.9, 0.999, 1e-8, 0.0, True, True), _ffi.adam(0.8, 0.99, 1e-6, 0.1, True, True)]
    plan = _ffi.head_fit_plan(rows, off, lr, hps, 64, 10, _ffi.FIT_LOSS_CE)
    assert plan.dtype == np.uint8 and plan.size == 64 * rows.size
    r, o, slot, inv, sc, ams = plan_fields(plan)
    assert r.tolist() == rows.reshape(-1).tolist()
    t = [0, 0]
    for s in range(rows.shape[0]):
        for j in range(2):
            i = 2 * s + j
            if rows[s, j] == 0:                                       # an idle entry is all zeros and advances nothing
                assert not plan[64 * i:64 * i + 64].any()
                continue
            t[j] += 1
            assert slot[i] == t[j] - 1 and o[i] == off[s, j] and ams[i] == 1
            assert inv[i] == np.float32(1.0 / rows[s, j])
            b1, b2, wd = hps[j].beta1, hps[j].beta2, hps[j].weight_decay
            want = [b1, 1.0 - b1, b2, 1.0 - b2, hps[j].eps, 0.0, 1.0 - lr[s, j] * wd, lr[s, j] / (1.0 - b1 ** t[j]),
                    np.sqrt(1.0 - b2 ** t[j])]
            assert sc[i].tolist() == [float(np.float32(v)) for v in want], (s, j)
    assert t == [4, 6]
    bce = _ffi.head_fit_plan(rows, off, lr, [_ffi.adam(), _ffi.adam()], 64, 10, _ffi.FIT_LOSS_BCE)
    assert plan_fields(bce)[3][0] == np.float32(1.0 / (64.0 * 10.0))


def test_plan_and_workspace_argument_errors():
    rows = np.array([[4, 0], [4, 4]], dtype=np.int32)
    off, lr, hps = np.zeros((2, 2), dtype=np.int64), np.full((2, 2), 1e-3), [_ffi.adam(), _ffi.adam()]

    def refused(match, **over):
        a = dict(rows=rows, idx_offset=off, lr=lr, hps=hps, rows_max=4, classes=3, loss=_ffi.FIT_LOSS_BCE)
        a.update(over)
        with pytest.raises(_ffi.AcxError, match=match):
            _ffi.head_fit_plan(**a)

    refused("rows", rows=np.array([[5, 0], [4, 4]], dtype=np.int32))
    refused("rows", rows=np.array([[-1, 0], [4, 4]], dtype=np.int32))
    refused("idx_offset", idx_offset=np.array([[-1, 0], [0, 0]], dtype=np.int64))
    refused("lr", lr=np.array([[1e-3, 0.0], [float("nan"), 1e-3]]))
    refused("beta1", hps=[_ffi.adam(), _ffi.adam(beta1=1.0)])
    refused("amsgrad", hps=[_ffi.adam(), _ffi.adam(amsgrad=False)])
    refused("amsgrad", hps=[_ffi.adam(), _ffi.adam(decoupled=True)])
    refused("classes", classes=0)
    refused("loss", loss=2)
    _ffi.head_fit_plan(rows, off, np.array([[1e-3, float("nan")], [1e-3, 1e-3]]), hps, 4, 3, 0)   # lr of an idle entry is not read
    with pytest.raises(_ffi.AcxError, match="jobs"):
        _ffi.head_fit_group_workspace_bytes(_ffi.FIT_MAX_JOBS + 1, 64, 10, 0)
    with pytest.raises(_ffi.AcxError, match="jobs"):
        _ffi.head_fit_group_workspace_bytes(0, 64, 10, 0)
    with pytest.raises(_ffi.AcxError, match="loss"):
        _ffi.head_fit_group_workspace_bytes(1, 64, 10, 5)
    for loss, single in ((0, _ffi.head_fit_workspace_bytes), (1, _ffi.head_fit_ce_workspace_bytes)):
        assert _ffi.head_fit_group_workspace_bytes(1, 64, 50, loss) == single(64, 50)
        assert _ffi.head_fit_group_workspace_bytes(7, 64, 50, loss) == 7 * single(64, 50)


# ---- ValueErrors come before the GPU-only error ------------------------------------------------------------------------------------
def test_value_errors_before_the_gpu_only_error():
    emb, target = torch.zeros(10, 768), torch.zeros(10, 3)
    ok = torch.arange(5)
    cases = [
        ([], "non-empty"),
        ("jobs", "non-empty"),
        ([{"rows": torch.tensor([0, 10])}], "outside"),
        ([{"rows": torch.tensor([-1, 2])}], "outside"),
        ([{"rows": torch.tensor([], dtype=torch.int64)}], "no rows"),
        ([{"rows": torch.tensor([0.0, 1.0])}], "int64"),
        ([{"rows": [0, 1]}], "int64"),
        ([{"rows": ok, "val": torch.tensor([12])}], "outside"),
        ([{"rows": ok, "learning_rate": 1e-3}], "keys"),
        ([{"rows": ok, "lr": -1.0}], "lr"),
        ([{"rows": ok, "lr": [1e-3] * 3}], "lr has 3 values for 4 steps"),
        ([{"rows": ok, "betas": (0.9, 1.0)}], "betas"),
        ([{"rows": ok, "eps": 0.0}], "eps"),
        ([{"rows": ok}, {"rows": ok, "weight_decay": -1.0}], "weight_decay"),
    ]
    for jobs, match in cases:
        with pytest.raises(ValueError, match=match):
            ft.fit_heads(emb, target, jobs, epochs=2, batch_size=4)
    with pytest.raises(ValueError, match="loss"):
        ft.fit_heads(emb, target, [{}], loss="mse")
    with pytest.raises(ValueError, match="label_smoothing"):
        ft.fit_heads(emb, target, [{}], label_smoothing=0.1)
    with pytest.raises(ValueError, match="batch_size"):
        ft.fit_heads(emb, target, [{}], batch_size=0)
    with pytest.raises(ValueError, match="CUDA"):                                         # valid jobs: only the device is wrong
        ft.fit_heads(emb, target, [{"rows": ok, "val": ok + 5}], epochs=2, batch_size=4)
    # cross_validate_head: its own errors, then the jobs', then the device
    labels = torch.arange(10) % 2
    with pytest.raises(ValueError, match="folds"):
        ft.cross_validate_head(emb, target, folds=1)
    with pytest.raises(ValueError, match="grid key"):
        ft.cross_validate_head(emb, target, folds=2, grid={"init": [None]})
    with pytest.raises(ValueError, match="stratify"):
        ft.cross_validate_head(emb, target, folds=2, stratify=True)
    with pytest.raises(ValueError, match="fold_ids"):
        ft.cross_validate_head(emb, target, folds=2, fold_ids=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="empty"):
        ft.cross_validate_head(emb, target, folds=3, fold_ids=torch.arange(10) % 2)
    with pytest.raises(ValueError, match="no setting"):
        ft.cross_validate_head(emb, target, folds=2, val=None)
    with pytest.raises(ValueError, match="lr"):
        ft.cross_validate_head(emb, target, folds=2, grid={"lr": [1e-3, -1.0]})
    with pytest.raises(ValueError, match="CUDA"):
        ft.cross_validate_head(emb, labels, folds=2, loss="ce", classes=2, epochs=1)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared():
    lib = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    names = ("acx_head_fit_group_workspace_bytes", "acx_head_fit_plan_bytes", "acx_head_fit_plan_fill", "acx_head_fit_group_step",
             "acx_head_fit_group_step_ce")
    for name in names:
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert _ffi.SIGNATURES[name][0] is ctypes.c_int
        assert "ACX_API int %s(" % name in hdr
    assert [len(_ffi.SIGNATURES[k][1]) for k in names] == [5, 3, 11, 17, 16]
    assert "#define ACX_FIT_MAX_JOBS %d" % _ffi.FIT_MAX_JOBS in hdr
    assert "ACX_FIT_LOSS_BCE = %d, ACX_FIT_LOSS_CE = %d" % (_ffi.FIT_LOSS_BCE, _ffi.FIT_LOSS_CE) in hdr
    assert ctypes.sizeof(_ffi.AcxFitJob) == 80
    assert hasattr(ft, "fit_heads") and hasattr(ft, "cross_validate_head") and ft.CrossValidation._fields == (
        "configs", "fold_ids", "metric", "scores", "mean", "std", "best", "fits", "final")
