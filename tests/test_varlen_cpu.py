"""CPU: the host side of variable-length batches -- workspace sizing and argument checks of the C ABI (no device needed),
the frame-output layout against the oracle's geometry, the grouping of extract(pack=True) and the wrapper's validation."""
import ctypes

import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny, varlen_frame_layout
from audioset_convnext_inf_amd.pytorch.extract_embeddings import pack_groups
from oracle import ref_cpu


def ws_bytes(lengths, mode=_ffi.MODE_LOGITS):
    lens = (ctypes.c_int64 * max(1, len(lengths)))(*lengths)
    out = ctypes.c_size_t()
    rc = _ffi.lib().acx_workspace_bytes_varlen(None, lens, len(lengths), mode, ctypes.byref(out))
    return rc, out.value, _ffi.lib().acx_last_error().decode()


def test_version():
    assert _ffi.lib().acx_version() == 101


def test_workspace_bytes_and_errors():
    rc, one, _ = ws_bytes([320000])
    assert rc == _ffi.OK and one > 0
    rc, two, _ = ws_bytes([320000, 7360])
    assert rc == _ffi.OK and two > one
    # at least the uniform plan of the same clips
    uni = ctypes.c_size_t()
    assert _ffi.lib().acx_workspace_bytes(None, 1, 320000, 0, ctypes.byref(uni)) == _ffi.OK
    assert one >= uni.value
    rc, _, msg = ws_bytes([8000, 7359, 9000])
    assert rc != _ffi.OK and "clip 1" in msg and "kernel size can't be greater than actual input size" in msg
    rc, _, msg = ws_bytes([])
    assert rc != _ffi.OK
    rc, _, msg = ws_bytes([8000] * 257)
    assert rc != _ffi.OK and "257" in msg
    assert ws_bytes([8000] * 256)[0] == _ffi.OK


@pytest.mark.parametrize("lengths", [[7360], [7360, 7361, 17000, 16000, 23000, 320000, 320319, 960000, 48000, 48000]])
def test_frame_layout_matches_oracle_geometry(lengths):
    offs = varlen_frame_layout(lengths)
    assert offs[0] == 0 and len(offs) == len(lengths) + 1
    for i, L in enumerate(lengths):
        h3, w3 = ref_cpu.out_hw(L)[3]
        assert offs[i + 1] - offs[i] == 768 * h3 * w3
        assert (h3, w3) == _ffi.stage_hw(L, 3)


def test_pack_groups():
    lengths = [10, 50, 30, 20, 40, 60]
    g = pack_groups(lengths, max_batch=2, max_samples=1000)
    assert g == [[5, 1], [4, 2], [3, 0]]
    g = pack_groups(lengths, max_batch=64, max_samples=100)
    assert sorted(i for grp in g for i in grp) == list(range(6))
    assert all(sum(lengths[i] for i in grp) <= 100 or len(grp) == 1 for grp in g)
    assert pack_groups([500, 10], max_batch=8, max_samples=100) == [[0], [1]]


def test_wrapper_validation_without_a_device(synth_sd):
    m = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    m.load_state_dict(synth_sd)
    m.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        m.forward_varlen([torch.zeros(8000), torch.zeros(9000)])
    with pytest.raises(ValueError, match="lengths sum"):
        m.forward_varlen(torch.zeros(20000), [8000, 8000])
    with pytest.raises(ValueError, match="needs `lengths`"):
        m.forward_varlen(torch.zeros(20000))
    with pytest.raises(ValueError):
        m.forward_varlen([torch.zeros(8000)], what="pooled")
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_varlen([torch.zeros(8000)])
