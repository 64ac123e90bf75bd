"""CPU: classifier heads of any size -- constructor range, checkpoints with a fine-tuned head, evaluate_sharded over N columns,
and the demo's label-table fallback.  No GPU needed."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from audioset_convnext_inf_amd import _ffi, synth
from audioset_convnext_inf_amd.pytorch.convnext import ConvNeXt, check_num_classes, convnext_tiny, load_checkpoint
from audioset_convnext_inf_amd.utils.utilities import label_names_for

N = 50


def tiny():
    return convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)


def head_sd(n, seed=3):
    sd = synth.synth_state_dict(0)
    g = torch.Generator().manual_seed(seed)
    sd["head_audioset.weight"] = torch.randn(n, 768, generator=g) * 0.05
    sd["head_audioset.bias"] = torch.randn(n, generator=g) * 0.1
    return sd


@pytest.mark.parametrize("n", [1, 10, 50, 200, 527, 1000, 4096, 32768])
def test_constructor_accepts_any_class_count(n):
    m = ConvNeXt(in_chans=1, num_classes=n)
    assert m.head_audioset.out_features == n and m.num_classes == n
    assert tuple(m.head_audioset.weight.shape) == (n, 768) and tuple(m.head_audioset.bias.shape) == (n,)


def test_reference_default_of_1000_classes():
    assert ConvNeXt().num_classes == 1000


@pytest.mark.parametrize("n", [0, -1, 32769, 1 << 20, 2.0, "50", True, None])
def test_constructor_rejects_out_of_range(n):
    with pytest.raises(ValueError):
        ConvNeXt(in_chans=1, num_classes=n)
    with pytest.raises(ValueError):
        check_num_classes(n)


def test_other_restrictions_stay():
    with pytest.raises(NotImplementedError):
        ConvNeXt(depths=[2, 2, 8, 2], dims=[80, 160, 320, 640], num_classes=N)
    with pytest.raises(NotImplementedError):
        ConvNeXt(num_classes=N, use_torchaudio=True)
    assert _ffi.MAX_CLASSES == 32768 and _ffi.NUM_CLASSES == 527


def test_head_swap_state_dict_round_trip():
    m = tiny()
    m.head_audioset = nn.Linear(768, N)
    sd = head_sd(N)
    m.load_state_dict(sd, strict=True)
    assert m.num_classes == N
    assert torch.equal(m.state_dict()["head_audioset.weight"], sd["head_audioset.weight"])
    m.head_audioset = nn.Linear(768, 527)
    m.load_state_dict(synth.synth_state_dict(0), strict=True)
    assert m.num_classes == 527


def test_headless_bias_is_rejected():
    m = tiny()
    m.head_audioset = nn.Linear(768, N, bias=False)
    with pytest.raises(ValueError, match="head_audioset.bias"):
        m._check_head()
    m.head_audioset = nn.Linear(512, N)
    with pytest.raises(ValueError):
        m._check_head()


def _assert_loaded(m, sd, n):
    assert m.num_classes == n
    got = m.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())


def test_load_checkpoint_pth_sizes_the_head(tmp_path):
    sd = head_sd(N)
    p = str(tmp_path / "ft.pth")
    torch.save({"model": sd}, p)
    _assert_loaded(load_checkpoint(tiny(), p), sd, N)
    bare = str(tmp_path / "bare.pth")
    torch.save(sd, bare)
    _assert_loaded(ConvNeXt.from_pretrained(bare), sd, N)
    # a 527-row checkpoint loads exactly as before, also into a model that had another head
    sd527 = synth.synth_state_dict(0)
    p527 = str(tmp_path / "as.pth")
    torch.save({"model": sd527}, p527)
    m = tiny()
    m.head_audioset = nn.Linear(768, N)
    _assert_loaded(load_checkpoint(m, p527), sd527, 527)


def test_load_checkpoint_safetensors_sizes_the_head(tmp_path):
    pytest.importorskip("safetensors")
    from safetensors.torch import save_model
    src = ConvNeXt(in_chans=1, num_classes=N)
    sd = head_sd(N)
    src.load_state_dict(sd)
    p = str(tmp_path / "model.safetensors")
    save_model(src, p)
    _assert_loaded(ConvNeXt.from_pretrained(p), sd, N)
    _assert_loaded(load_checkpoint(tiny(), p), sd, N)


def test_converter_keeps_the_head_size(tmp_path):
    pytest.importorskip("safetensors")
    import convert_pytorch_ckpt_to_safetensors as conv
    sd = head_sd(N)
    p = str(tmp_path / "ft.pth")
    torch.save({"model": sd}, p)
    out = conv.convert(p, str(tmp_path / "model.safetensors"))
    _assert_loaded(ConvNeXt.from_pretrained(out), sd, N)


def test_checkpoint_with_out_of_range_head_is_rejected(tmp_path):
    sd = head_sd(N)
    sd["head_audioset.weight"] = torch.zeros(32769, 768)
    sd["head_audioset.bias"] = torch.zeros(32769)
    p = str(tmp_path / "big.pth")
    torch.save(sd, p)
    with pytest.raises(ValueError):
        load_checkpoint(tiny(), p)


# ---- evaluate_sharded over N columns, world size 2 over gloo (as tests/test_parallel_cpu.py) ----------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _FakeHeadModel(nn.Module):
    """Stands in for the GPU model: an N-class head on a deterministic per-clip function of the input."""

    def __init__(self, n):
        super().__init__()
        self.head_audioset = nn.Linear(768, n)
        self.training = False

    def forward(self, x):
        x = x.float()
        k = torch.arange(1, self.head_audioset.out_features + 1, dtype=torch.float32)
        logits = torch.sin(x[:, :1] * k + x[:, 1:2])
        return {"clipwise_output": torch.sigmoid(logits), "clipwise_logits": logits}


class _Shard:
    def __init__(self, wav, target):
        self.waveforms, self.targets = wav, target
        self.audio_names = np.array(["clip%d" % i for i in range(len(wav))])

    def __len__(self):
        return len(self.waveforms)


def _sharded_worker(rank, world, port, n_clips, n, batch, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from audioset_convnext_inf_amd.pytorch import evaluate as ev
    rs = np.random.RandomState(0)
    wav = rs.randint(-3000, 3000, size=(n_clips, 64)).astype(np.int16)
    target = rs.uniform(size=(n_clips, n)) < 0.3
    target[0], target[1] = True, False
    model = _FakeHeadModel(n)
    try:
        stats = ev.evaluate_sharded(model, _Shard(wav, target), batch_size=batch)
        full = ev.forward(model, ev_batches(wav, target, batch), return_target=True)
        ref = ev.calculate_statistics(full["target"], full["clipwise_output"])
        ok = all(np.allclose(stats[k], ref[k], equal_nan=True) and stats[k].shape == (n,) for k in ref)
    except Exception as e:  # noqa: BLE001
        ok = repr(e)
    ret[rank] = ok
    dist.destroy_process_group()


def ev_batches(wav, target, batch):
    from audioset_convnext_inf_amd.utils.data_generator import evaluate_batches
    return evaluate_batches(_Shard(wav, target), batch, 0, 1, device_cast=True)


def _run_sharded(n_clips, n, batch):
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, n_clips, n, batch, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    assert ret[0] is True and ret[1] is True, (ret[0], ret[1])


def test_evaluate_sharded_n_columns_world2():
    _run_sharded(24, N, 8)


def test_evaluate_sharded_rank_without_batches():
    # one batch in all: rank 1 scores nothing, and still gathers N columns
    _run_sharded(6, 10, 8)


# ---- the demo's label table -----------------------------------------------------------------------------------------------------
def test_label_table_only_when_row_count_matches(tmp_path):
    names, why = label_names_for(527)
    assert why is None and len(names) == 527
    names, why = label_names_for(N)
    assert names is None and "527" in why and str(N) in why
    csv = tmp_path / "labels.csv"
    csv.write_text("index,mid,display_name\n" + "".join('%d,/m/x%d,"class %d"\n' % (i, i, i) for i in range(N)))
    names, why = label_names_for(N, str(csv))
    assert why is None and len(names) == N and names[3] == "class 3"
    names, why = label_names_for(527, str(csv))
    assert names is None and str(csv) in why
