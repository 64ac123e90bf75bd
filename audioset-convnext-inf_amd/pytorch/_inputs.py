"""The host-side input rules of the analysis calls (metrics, retrieval, finetune, classify), each written once: what a kernel
may read where it lies, how a target travels, and which device a call runs on.  Plain functions on tensors of any device."""
import torch

from .. import _ffi


def rows(t, align4=False):
    """t (2-D) if a kernel can read its rows in place -- unit column stride and a row stride no shorter than the row (a column
    slice of a wider tensor too); align4, for the 16-byte loaders: also a row stride that is a multiple of 4 elements and a
    16-byte aligned base -- otherwise t.contiguous()."""
    ok = t.stride(1) == 1 and t.stride(0) >= t.shape[1]
    if ok and align4:
        ok = t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def target_code(t):
    """ACX_TARGET_U8 or ACX_TARGET_F32 of a tensor that is already uint8 or float32."""
    return _ffi.TARGET_U8 if t.dtype == torch.uint8 else _ffi.TARGET_F32


def kernel_target(t):
    """2-D targets -> (tensor, ACX_TARGET_*): bool is viewed as uint8, uint8 and float32 are read as they are, anything else
    travels as float32; in a layout rows() accepts."""
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype not in (torch.uint8, torch.float32):
        t = t.to(torch.float32)
    t = rows(t)
    return t, target_code(t)


def cuda_device(device, what):
    """The torch.device a call runs on: None is the current CUDA device, and so is "cuda" without an index; anything that is
    not CUDA raises ValueError("<what> a CUDA (HIP) device, not <device>")."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError("%s a CUDA (HIP) device, not %s" % (what, device))
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
