"""What the GPU tests of the two head-fit losses (test_gpu_finetune.py: BCE, test_gpu_classify.py: cross-entropy) share
verbatim: the initial head, the optimiser state, and the raw acx_adam_update call.  A plain helper module, not a conftest."""
import ctypes

import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd._ffi import vp        # noqa: F401  (re-exported: the tests pass raw pointers with it)

DEV = "cuda"


def init(N):
    return torch.randn(N, 768, generator=torch.Generator().manual_seed(1)) * 0.02, torch.zeros(N)


def fresh_state(W0, b0):
    st = {"W": W0.to(DEV).clone(), "b": b0.to(DEV).clone()}
    for k, ref in (("mW", "W"), ("vW", "W"), ("xW", "W"), ("mb", "b"), ("vb", "b"), ("xb", "b")):
        st[k] = torch.zeros_like(st[ref])
    return st


def last_error():
    return _ffi.lib().acx_last_error().decode()


def call_update(p, g, m, v, x, hp, t, lr, over=None):
    a = dict(p=vp(p), g=vp(g), m=vp(m), v=vp(v), x=vp(x), n=p.numel(), hp=ctypes.byref(hp) if hp is not None else None, t=t,
             lr=lr)
    a.update(over or {})
    return _ffi.lib().acx_adam_update(a["p"], a["g"], a["m"], a["v"], a["x"], a["n"], a["hp"], a["t"], a["lr"],
                                      _ffi.stream_ptr(torch.device(DEV)))
