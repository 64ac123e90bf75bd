"""One analysis call inside guards, a plain helper imported like forward_guard.py (tests/test_analysis_guard_cpu.py,
tests/test_gpu_analysis_guard.py).

The analysis wrappers (pytorch/metrics.py ... pytorch/sed_metrics.py) take their workspaces and outputs from torch.empty: a
workspace of exactly the bytes the size call promises, an output of exactly its shape.  The caching allocator rounds every block
up and very often hands out zeros or the leftovers of an identical earlier call, so a write a little past the end, an output
element nobody wrote and a partial sum nobody cleared all go unseen.  guarded_allocations() replaces torch.empty for its duration:
every device allocation becomes a view into the payload of a layer_ref.Guarded buffer --

    [256 B canary][payload: the requested bytes, prefilled with the poison byte, padded to 256 B with canary][256 B canary]

so a write past either end meets canary words, and whatever the call reads before it writes is poison.  run_guarded() makes the
same call unpatched, under 0xFF (NaN as fp32 / fp64, -1 as an integer) and under 0x7F (3.4e38 as fp32, 1.4e306 as fp64, a huge
positive integer) and asks for the same bits three times: an unwritten output element or scratch read before it was written
differs between the two poisons, a dependence on stale zeros differs from the unpatched run.
"""
import contextlib
import struct

import numpy as np
import pytest
import torch

import layer_ref as lr
from forward_guard import POISONS


class Allocations:
    """The guards one guarded_allocations() block handed out, in the order of the requests."""

    def __init__(self, poison):
        self.poison = poison
        self.records = []                          # (Guarded, requested bytes, shape, dtype)

    def __len__(self):
        return len(self.records)

    def payloads(self):
        """The requested bytes of every allocation as uint8 views, in the order of the requests."""
        return [g.payload.view(torch.uint8)[:nbytes] for g, nbytes, _, _ in self.records]

    def untouched(self, first=0):
        """Whether every payload from allocation `first` on is still entirely poison."""
        return all(bool((p == self.poison).all()) for p in self.payloads()[first:])

    def check(self):
        for k, (g, _, shape, dtype) in enumerate(self.records):
            assert g.intact(), "canary at allocation %d overwritten: torch.empty(%s, dtype=%s), poison 0x%02X" % (
                k, tuple(shape), dtype, self.poison)


def _resolve_size(args, kwargs):
    if "size" in kwargs:
        size = kwargs.pop("size")
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        size = args[0]
    else:
        size = args
    return tuple(int(s) for s in size)


def _device_type(device):
    if device is None:
        return torch.get_default_device().type
    if isinstance(device, bool):
        raise TypeError("device given as a bool")
    if isinstance(device, int):
        return "cuda"                              # a bare index is an accelerator index
    return torch.device(device).type


@contextlib.contextmanager
def guarded_allocations(monkeypatch, poison, device_type="cuda"):
    """torch.empty hands out poisoned payloads of layer_ref.Guarded buffers for every non-empty request on a `device_type`
    device ("cuda"; the CPU tests of this helper pass "cpu") -> Allocations.  Everything else goes to the real torch.empty."""
    real = torch.empty
    allocs = Allocations(poison)

    def empty(*args, **kwargs):
        kw = dict(kwargs)
        try:
            shape = _resolve_size(args, kw)
            dtype = kw.pop("dtype", None)
            device = kw.pop("device", None)
            kind = _device_type(device)
        except (TypeError, ValueError, RuntimeError):
            return real(*args, **kwargs)
        if kw or kind != device_type or int(np.prod(shape, dtype=np.int64)) == 0:   # (out=, pin_memory=, memory_format= ...: not ours)
            return real(*args, **kwargs)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        numel = int(np.prod(shape, dtype=np.int64))
        nbytes = numel * dtype.itemsize
        if device is None:
            target = torch.get_default_device()
        else:
            target = torch.device(kind, device) if isinstance(device, int) else torch.device(device)
        g = lr.Guarded((nbytes + 3) // 4 * 4, device=target)
        raw = g.payload.view(torch.uint8)
        raw.fill_(poison)
        allocs.records.append((g, nbytes, shape, dtype))
        return raw[:nbytes].view(dtype).view(shape)

    monkeypatch.setattr(torch, "empty", empty)
    try:
        yield allocs
    finally:
        monkeypatch.setattr(torch, "empty", real)


def _bits(v):
    """A result entry as something == compares bit for bit: tensors and arrays as (shape, dtype, bytes), floats as their words."""
    if isinstance(v, torch.Tensor):
        t = v.detach().cpu().contiguous()
        return ("tensor", tuple(t.shape), str(t.dtype), t.reshape(-1).view(torch.uint8).numpy().tobytes())
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return ("array", a.shape, str(a.dtype), a.tobytes())
    if isinstance(v, (float, np.floating)):
        return ("float", struct.pack("<d", float(v)))
    if isinstance(v, (bool, int, np.integer, np.bool_, str, type(None))):
        return ("plain", v if isinstance(v, (str, type(None))) else int(v))
    raise TypeError("extract() returned a %s: it must flatten the result to tensors, arrays and numbers" % type(v).__name__)


def _snapshot(result, extract):
    flat = extract(result)
    assert isinstance(flat, tuple), "extract() must return a flat tuple"
    return [_bits(v) for v in flat]


def _describe(entry):
    return "%s %s %s" % entry[:3] if entry[0] in ("tensor", "array") else repr(entry)


def _same(a, b, what):
    assert len(a) == len(b), "%s: %d result entries against %d" % (what, len(a), len(b))
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, "result entry %d (%s) %s" % (k, _describe(x), what)


def run_guarded(call, extract, monkeypatch=None, device_type="cuda", poisons=POISONS):
    """call() makes one public wrapper call; extract(result) -> the flat tuple of tensors and numbers that are its documented
    result (the valid part only).  Runs it unpatched, then once per poison inside guarded_allocations(); after each guarded run
    every canary must be intact, and all runs must agree bit for bit (floats by their words, so NaN equals NaN).  Returns the
    unpatched result.  monkeypatch: the test's fixture; None: one of this call's own."""
    if monkeypatch is None:
        with pytest.MonkeyPatch.context() as mp:
            return run_guarded(call, extract, mp, device_type, poisons)
    sync = torch.cuda.synchronize if device_type == "cuda" else (lambda: None)
    result = call()
    sync()
    plain = _snapshot(result, extract)
    runs = []
    for poison in poisons:
        with guarded_allocations(monkeypatch, poison, device_type) as allocs:
            guarded = call()
            sync()
            runs.append(_snapshot(guarded, extract))
            assert len(allocs), "the call allocated nothing through torch.empty on a %s device: nothing was guarded" % device_type
            allocs.check()
    for poison, run in zip(poisons[1:], runs[1:]):
        _same(runs[0], run, "differs between poison 0x%02X and 0x%02X: an unwritten element, or scratch read before it was written"
              % (poisons[0], poison))
    _same(plain, runs[0], "differs between fresh memory and poison 0x%02X: something relies on memory being zero" % poisons[0])
    return result


def undersized(monkeypatch, module, name, call, error, device_type="cuda", short=256, poison=POISONS[0]):
    """module.<name> (a *_workspace_bytes function) answers `short` bytes less than the truth; call() must then raise `error`
    naming the workspace, launch nothing -- every payload allocated after the size query still poison -- and leave every canary
    intact.  Returns the error text."""
    truth = getattr(module, name)
    marks = []
    with guarded_allocations(monkeypatch, poison, device_type) as allocs:
        def less(*args, **kwargs):
            marks.append(len(allocs))
            return max(truth(*args, **kwargs) - short, 0)

        monkeypatch.setattr(module, name, less)
        try:
            try:
                call()
            except error as e:
                text = str(e)
            else:
                raise AssertionError("%s answered %d bytes too few and the call went through" % (name, short))
        finally:
            monkeypatch.setattr(module, name, truth)
            if device_type == "cuda":
                torch.cuda.synchronize()
        assert marks, "%s was never asked" % name
        assert "workspace" in text, "the error does not name the workspace: %s" % text
        assert allocs.untouched(marks[0]), "%s: a kernel ran although the workspace was refused" % name
        allocs.check()
    return text
