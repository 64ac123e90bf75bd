"""tests/analysis_guard.py on the CPU: the torch.empty interceptor takes every call form the analysis wrappers use and keeps shape,
dtype and alignment; run_guarded fails on each of four toy wrappers with one of the defects it is there to find, and passes the
clean one.  The guards are device="cpu" buffers here: the same code path, no GPU."""
import pytest
import torch

import analysis_guard as ag
import layer_ref as lr


def _guard_of(allocs, k):
    return allocs.records[k][0]


@pytest.mark.parametrize("form", ["n", "a_b", "tuple", "list", "size_kw", "torch_size"])
@pytest.mark.parametrize("device", ["cpu", torch.device("cpu")])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.float32, torch.float64, torch.int64, torch.bool, torch.float16])
def test_interceptor_forms(monkeypatch, form, device, dtype):
    with ag.guarded_allocations(monkeypatch, 0x7F, device_type="cpu") as allocs:
        t = {"n": lambda: torch.empty(15, dtype=dtype, device=device),
             "a_b": lambda: torch.empty(3, 5, dtype=dtype, device=device),
             "tuple": lambda: torch.empty((3, 5), dtype=dtype, device=device),
             "list": lambda: torch.empty([3, 5], device=device, dtype=dtype),
             "size_kw": lambda: torch.empty(size=(3, 5), dtype=dtype, device=device),
             "torch_size": lambda: torch.empty(torch.Size((3, 5)), dtype=dtype, device=device)}[form]()
        assert len(allocs) == 1
        assert t.shape == ((15,) if form == "n" else (3, 5)) and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous()
        g = _guard_of(allocs, 0)
        nbytes = 15 * dtype.itemsize
        assert t.data_ptr() == g.payload.data_ptr() and t.data_ptr() == g.buf.data_ptr() + 4 * lr.GUARD_WORDS
        assert t.data_ptr() % 64 == 0                       # the host allocator's alignment; Guarded asserts 256 B on the device
        assert g.words == (nbytes + 3) // 4 and g.buf.numel() == 2 * lr.GUARD_WORDS + (g.words + 63) // 64 * 64
        assert bool((t.contiguous().view(-1).view(torch.uint8) == 0x7F).all())
        (payload,) = allocs.payloads()
        assert payload.numel() == nbytes and allocs.untouched()
        allocs.check()
        t.view(-1).view(torch.uint8)[-1] = 0
        assert not allocs.untouched()
        allocs.check()                                      # the last requested byte is payload, not canary


def test_interceptor_passes_the_rest_on(monkeypatch):
    real = torch.empty
    with ag.guarded_allocations(monkeypatch, 0xFF, device_type="cpu") as allocs:
        assert torch.empty is not real
        assert torch.empty(0, dtype=torch.float32, device="cpu").numel() == 0
        assert torch.empty((4, 0), dtype=torch.float32, device="cpu").shape == (4, 0)
        assert torch.empty(3, dtype=torch.float32, device="meta").device.type == "meta"         # another device
        assert torch.empty(3, device="cpu", pin_memory=False).shape == (3,)                      # a keyword that is not ours
        assert len(allocs) == 0
        assert torch.empty(3).dtype == torch.get_default_dtype() and len(allocs) == 1            # no device: the default one, the CPU
    assert torch.empty is real
    with ag.guarded_allocations(monkeypatch, 0xFF) as allocs:                                    # the default: CUDA devices only
        assert torch.empty(3, device="cpu").shape == (3,) and torch.empty(3).shape == (3,) and len(allocs) == 0
    assert torch.empty is real


def test_device_forms():
    assert ag._device_type("cuda") == ag._device_type("cuda:1") == ag._device_type(torch.device("cuda", 0)) == "cuda"
    assert ag._device_type(0) == ag._device_type(1) == "cuda"
    assert ag._device_type("cpu") == ag._device_type(torch.device("cpu")) == ag._device_type(None) == "cpu"


def test_check_names_the_allocation(monkeypatch):
    with ag.guarded_allocations(monkeypatch, 0xFF, device_type="cpu") as allocs:
        torch.empty(8, dtype=torch.float64, device="cpu")
        t = torch.empty((3, 5), dtype=torch.int32, device="cpu")
        _guard_of(allocs, 1).buf[lr.GUARD_WORDS + 15] = 7          # one word past the 15 requested
        with pytest.raises(AssertionError, match=r"allocation 1 .*\(3, 5\).*torch\.int32"):
            allocs.check()
        _guard_of(allocs, 1).buf[lr.GUARD_WORDS + 15] = lr.CANARY
        allocs.check()
        _guard_of(allocs, 0).buf[lr.GUARD_WORDS - 1] = 7           # one word in front
        with pytest.raises(AssertionError, match=r"allocation 0 .*\(8,\).*torch\.float64"):
            allocs.check()
        assert t.shape == (3, 5)


# ---- toy wrappers: y[i] = 2 x[i], and the sum of x over partial sums, as the analysis wrappers do it --------------------------------

def _raw_store(t, index, value):
    """What a kernel does with a pointer: store at t's base + index elements, in bounds of t or not."""
    torch.as_strided(t, (index + 1,), (1,))[index] = value


def toy_clean(x):
    n = x.numel()
    out = torch.empty(n, dtype=torch.float64, device="cpu")
    part = torch.empty(4, dtype=torch.float64, device="cpu")
    part.zero_()
    for i in range(n):
        out[i] = 2.0 * x[i]
        part[i % 4] += x[i]
    return out, float(part.sum())


def toy_overrun(x):
    out, total = toy_clean(x)
    scratch = torch.empty(5, dtype=torch.float32, device="cpu")
    scratch.zero_()
    _raw_store(scratch, 5, 1.0)                             # one element past the end
    return out, total


def toy_unwritten(x):
    n = x.numel()
    out = torch.empty(n, dtype=torch.float64, device="cpu")
    for i in range(n - 1):                                  # the last element stays as allocated
        out[i] = 2.0 * x[i]
    return out, float(x.sum())


def toy_uncleared_sum(x):
    part = torch.empty(4, dtype=torch.float64, device="cpu")
    for i in range(x.numel()):                              # accumulates into slots nobody cleared
        part[i % 4] += x[i]
    return 2.0 * x, float(part.sum())


def toy_needs_zero(x):
    changed = torch.empty(1, dtype=torch.int32, device="cpu")      # a flag the "kernel" only ever raises
    if bool((x < 0).any()):
        changed[0] = 1
    return 2.0 * x, int(changed[0] != 0)


def _extract(result):
    return (result[0], result[1])


@pytest.fixture
def zero_fresh_memory(monkeypatch):
    """torch.empty as a fresh process very often sees it on the device: blocks rounded up to 512 bytes, holding zeros.  The
    unpatched run of run_guarded then stands for the suite as it was, in which every toy below gives the right answer."""
    real = torch.empty

    def empty(*args, dtype=torch.float32, device=None):
        shape = ag._resolve_size(args, {})
        nbytes = dtype.itemsize * int(torch.Size(shape).numel())
        block = real((nbytes + 511) // 512 * 512, dtype=torch.uint8, device=device).zero_()
        return block[:nbytes].view(dtype).view(shape)

    monkeypatch.setattr(torch, "empty", empty)


X = torch.arange(1.0, 8.0, dtype=torch.float64)


def test_toys_are_right_on_zero_memory(zero_fresh_memory):
    for toy in (toy_clean, toy_overrun, toy_unwritten, toy_uncleared_sum, toy_needs_zero):
        out, number = toy(X)
        if toy is toy_unwritten:
            assert torch.equal(out[:-1], 2.0 * X[:-1])
        else:
            assert torch.equal(out, 2.0 * X)
        assert number == (0 if toy is toy_needs_zero else 28.0)


def test_run_guarded_passes_the_clean_toy(monkeypatch, zero_fresh_memory):
    out, total = ag.run_guarded(lambda: toy_clean(X), _extract, monkeypatch, device_type="cpu")
    assert torch.equal(out, 2.0 * X) and total == 28.0
    ag.run_guarded(lambda: toy_clean(X), _extract, device_type="cpu")            # with a MonkeyPatch of its own


@pytest.mark.parametrize("toy, message", [
    (toy_overrun, r"canary at allocation 2 overwritten: torch\.empty\(\(5,\), dtype=torch\.float32\)"),
    (toy_unwritten, r"result entry 0 .*differs between poison 0xFF and 0x7F"),
    (toy_uncleared_sum, r"result entry 1 .*differs between poison 0xFF and 0x7F"),
    (toy_needs_zero, r"result entry 1 .*differs between fresh memory and poison 0xFF"),
], ids=["overrun", "unwritten", "uncleared_sum", "needs_zero"])
def test_run_guarded_fails_the_broken_toys(monkeypatch, zero_fresh_memory, toy, message):
    with pytest.raises(AssertionError, match=message):
        ag.run_guarded(lambda: toy(X), _extract, monkeypatch, device_type="cpu")


def test_nan_results_compare_equal(monkeypatch):
    def nans():
        out = torch.empty(2, dtype=torch.float32, device="cpu")
        out[0], out[1] = float("nan"), 1.0
        return out, float("nan")

    ag.run_guarded(nans, _extract, monkeypatch, device_type="cpu")
    with pytest.raises(TypeError, match="flatten"):
        ag.run_guarded(lambda: ([1.0], 0), _extract, monkeypatch, device_type="cpu")
    with pytest.raises(AssertionError, match="nothing was guarded"):
        ag.run_guarded(lambda: (torch.zeros(2), 0), _extract, monkeypatch, device_type="cpu")


class _ToyError(RuntimeError):
    pass


class _toy_sizes:                                           # stands for _ffi: the size function is looked up at call time
    @staticmethod
    def toy_workspace_bytes(n):
        return 512 * n


def _toy_sized(n, launch_anyway=False, overrun=False):
    out = torch.empty(n, dtype=torch.float32, device="cpu")
    need = 512 * n
    nbytes = _toy_sizes.toy_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cpu")
    if overrun:
        _raw_store(ws, nbytes + 2, 1)
    if nbytes < need and not launch_anyway:
        raise _ToyError("toy: workspace of %d bytes, %d needed" % (nbytes, need))
    ws.zero_()
    out.zero_()
    if nbytes < need:
        raise _ToyError("toy: workspace of %d bytes, %d needed" % (nbytes, need))
    return out


def test_undersized(monkeypatch):
    text = ag.undersized(monkeypatch, _toy_sizes, "toy_workspace_bytes", lambda: _toy_sized(3), _ToyError, device_type="cpu")
    assert "workspace of 1280 bytes" in text and _toy_sizes.toy_workspace_bytes(3) == 1536
    with pytest.raises(AssertionError, match="a kernel ran"):
        ag.undersized(monkeypatch, _toy_sizes, "toy_workspace_bytes", lambda: _toy_sized(3, launch_anyway=True), _ToyError,
                      device_type="cpu")
    with pytest.raises(AssertionError, match="canary at allocation 1"):
        ag.undersized(monkeypatch, _toy_sizes, "toy_workspace_bytes", lambda: _toy_sized(3, overrun=True), _ToyError,
                      device_type="cpu")
    with pytest.raises(AssertionError, match="went through"):
        ag.undersized(monkeypatch, _toy_sizes, "toy_workspace_bytes", lambda: _toy_sized(3), _ToyError, device_type="cpu", short=0)
    with pytest.raises(AssertionError, match="never asked"):
        ag.undersized(monkeypatch, _toy_sizes, "toy_workspace_bytes", lambda: (_ for _ in ()).throw(_ToyError("workspace")),
                      _ToyError, device_type="cpu")
    assert _toy_sizes.toy_workspace_bytes(3) == 1536
