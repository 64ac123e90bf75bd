"""CPU: the host-side input rules of the analysis calls (pytorch/_inputs.py) and the raw-pointer helper beside _ffi.ptr, on CPU
tensors: what is handed to a kernel as it lies, what is copied first, how a target travels and which device a call takes."""
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch._inputs import cuda_device, kernel_target, rows, target_code


def strided(row_stride, offset, n=3, width=768):
    """(n, width) float32 view at `offset` floats into a 16-byte aligned buffer, rows `row_stride` floats apart."""
    buf = torch.arange(float(offset + n * row_stride))
    assert buf.data_ptr() % 16 == 0
    return buf.as_strided((n, width), (row_stride, 1), offset)


def test_rows_keeps_what_a_kernel_can_read():
    x = torch.arange(24.0).reshape(4, 6)
    assert rows(x) is x
    cols = x[:, 1:5]                                       # a column slice of a wider tensor: stride 6 >= 4
    assert rows(cols) is cols
    every_other = x[::2]                                   # row stride 12
    assert rows(every_other) is every_other


@pytest.mark.parametrize("view", ["transposed", "expanded", "column_stride_2"])
def test_rows_copies_what_it_cannot(view):
    x = torch.arange(24.0).reshape(4, 6)
    v = {"transposed": x.t(), "expanded": torch.arange(5.0).expand(3, 5), "column_stride_2": x[:, ::2]}[view]
    assert v.stride(1) != 1 or v.stride(0) < v.shape[1]
    got = rows(v)
    assert got is not v and got.is_contiguous() and torch.equal(got, v)


def test_rows_align4():
    ok = strided(772, 4)                                   # base 16 bytes in, row stride a multiple of 4
    assert rows(ok, align4=True) is ok
    for bad in (strided(772, 1), strided(770, 0), strided(770, 4)):
        assert rows(bad) is bad                            # readable by the scalar loaders
        got = rows(bad, align4=True)
        assert got is not bad and got.is_contiguous() and got.data_ptr() % 16 == 0 and torch.equal(got, bad)
    short = torch.arange(5.0).expand(3, 5)
    assert rows(short, align4=True).is_contiguous()


def test_kernel_target_and_code():
    b = torch.tensor([[True, False, True], [False, False, True]])
    t, code = kernel_target(b)
    assert t.dtype == torch.uint8 and code == _ffi.TARGET_U8 and t.data_ptr() == b.data_ptr() and t.tolist() == [[1, 0, 1], [0, 0, 1]]
    u = b.to(torch.uint8)
    t, code = kernel_target(u)
    assert t is u and code == _ffi.TARGET_U8
    f = b.to(torch.float32)
    t, code = kernel_target(f)
    assert t is f and code == _ffi.TARGET_F32
    for other in (torch.float64, torch.int64):
        t, code = kernel_target(b.to(other))
        assert t.dtype == torch.float32 and code == _ffi.TARGET_F32 and torch.equal(t, f)
    bt = b.t()                                             # a bool view no kernel can read in place
    t, code = kernel_target(bt)
    assert t.dtype == torch.uint8 and code == _ffi.TARGET_U8 and t.is_contiguous() and torch.equal(t, u.t())
    wide = torch.zeros((2, 8), dtype=torch.bool)[:, 2:5]   # a column slice stays where it is
    assert kernel_target(wide)[0].data_ptr() == wide.data_ptr()
    assert target_code(u) == _ffi.TARGET_U8 and target_code(f) == _ffi.TARGET_F32
    assert (_ffi.TARGET_F32, _ffi.TARGET_U8) == (0, 1)     # enum acx_target_dtype


@pytest.mark.parametrize("what", ["tagging_metrics runs on", "the search runs on", "bootstrap weights are drawn on"])
def test_cuda_device_refuses_the_host_in_the_callers_words(what):
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(ValueError) as e:
            cuda_device(device, what)
        assert str(e.value) == what + " a CUDA (HIP) device, not cpu"


def test_vp_takes_views_where_ptr_refuses():
    assert _ffi.vp(None) is None and _ffi.ptr(None) is None
    x = torch.arange(24.0).reshape(4, 6)
    assert _ffi.vp(x).value == x.data_ptr() == _ffi.ptr(x).value
    v = x[:, 1:5]
    assert _ffi.vp(v).value == x.data_ptr() + 4
    with pytest.raises(ValueError, match="contiguous"):
        _ffi.ptr(v)
