"""Host-side parts of head fitting (pytorch/finetune.py, acx_head_fit_workspace_bytes): no GPU needed."""
import ctypes
import inspect

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import finetune as ft
from audioset_convnext_inf_amd.pytorch.convnext import ConvNeXt


@pytest.mark.parametrize("n,batch", [(10, 4), (12, 4), (3, 8), (1, 1), (2000, 256), (300, 64)])
@pytest.mark.parametrize("drop_last", [False, True])
def test_batch_schedule_matches_a_brute_force_restatement(n, batch, drop_last):
    want = []
    for s in range(0, n, batch):
        rows = list(range(n))[s:s + batch]
        if len(rows) == batch or not drop_last:
            want.append((s, len(rows)))
    assert ft.epoch_batches(n, batch, drop_last) == want


def test_epoch_orders_come_from_one_generator():
    g = torch.Generator().manual_seed(11)
    want = torch.stack([torch.randperm(37, generator=g) for _ in range(4)])
    got = ft.epoch_orders(37, 4, seed=11)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(ft.epoch_orders(37, 2, seed=11), want[:2])                  # a shorter fit is a prefix of a longer one
    assert not torch.equal(ft.epoch_orders(37, 1, seed=12), want[:1])
    assert torch.equal(ft.epoch_orders(5, 3, seed=0, shuffle=False), torch.arange(5).repeat(3, 1))
    assert ft.epoch_orders(5, 0).shape == (0, 5)


def test_seeded_init_is_the_models_head_init():
    g = torch.Generator().manual_seed(4)
    want = torch.empty(50, 768)
    torch.nn.init.trunc_normal_(want, std=0.02, generator=g)
    w, b = ft.init_head(50, seed=4)
    assert torch.equal(w, want) and torch.equal(b, torch.zeros(50))
    assert float(w.abs().max()) <= 2.0 and 0.018 < float(w.std()) < 0.022
    # the order of an epoch does not depend on whether the init was drawn: two generators
    assert torch.equal(ft.epoch_orders(9, 1, seed=4), torch.randperm(9, generator=torch.Generator().manual_seed(4))[None])


def test_value_errors_name_the_argument():
    e, y = torch.zeros(8, 768), torch.zeros(8, 3)
    with pytest.raises(ValueError, match="emb must be a"):
        ft.fit_head(torch.zeros(8, 100), y)
    with pytest.raises(ValueError, match="emb must be float32"):
        ft.fit_head(e.double(), y)
    with pytest.raises(ValueError, match="emb must be a CUDA"):
        ft.fit_head(e, y)
    with pytest.raises(ValueError, match="epochs"):
        ft.fit_head(e, y, epochs=-1)
    with pytest.raises(ValueError, match="batch_size"):
        ft.fit_head(e, y, batch_size=0)
    with pytest.raises(ValueError, match="betas"):
        ft.fit_head(e, y, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="eps"):
        ft.fit_head(e, y, eps=0.0)
    with pytest.raises(ValueError, match="weight_decay"):
        ft.fit_head(e, y, weight_decay=-0.1)
    with pytest.raises(ValueError, match="lr has 3 values for 4 steps"):
        ft._lr_schedule([1e-3] * 3, 4)
    with pytest.raises(ValueError, match="lr"):
        ft._lr_schedule(-1.0, 4)
    assert ft._lr_schedule(1e-4, 3) == [1e-4] * 3 and ft._lr_schedule((1.0, 2.0), 2) == [1.0, 2.0]


def test_defaults_are_the_reference_finetune_settings():
    p = inspect.signature(ft.fit_head).parameters
    assert (p["lr"].default, p["betas"].default, p["eps"].default, p["weight_decay"].default) == (1e-4, (0.9, 0.999), 1e-8, 0.0)
    assert p["amsgrad"].default is True and p["decoupled"].default is False
    assert callable(ConvNeXt.fit_head)
    hp = _ffi.adam()
    assert (hp.beta1, hp.beta2, hp.eps, hp.weight_decay, hp.amsgrad, hp.decoupled) == (0.9, 0.999, 1e-8, 0.0, 1, 0)


def test_workspace_query():
    last_row = 0
    for rows in (1, 7, 64, 208, 1000, 4096):
        last = 0
        for classes in (1, 10, 50, 527, 4096, _ffi.MAX_CLASSES):
            b = _ffi.head_fit_workspace_bytes(rows, classes)
            assert b >= rows * classes * 4 and b % 256 == 0 and b >= last
            last = b
        assert last >= last_row
        last_row = last
    lib = _ffi.lib()
    out = ctypes.c_size_t()
    for args, word in (((0, 10), "rows"), ((-5, 10), "rows"), ((8, 0), "classes"), ((8, _ffi.MAX_CLASSES + 1), "classes")):
        assert lib.acx_head_fit_workspace_bytes(args[0], args[1], ctypes.byref(out)) == -1
        assert word in lib.acx_last_error().decode()
    assert lib.acx_head_fit_workspace_bytes(8, 8, None) == -1 and "out_bytes" in lib.acx_last_error().decode()
    assert lib.acx_head_fit_workspace_bytes(1 << 23, 8, ctypes.byref(out)) == -6
