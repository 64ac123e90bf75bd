"""CPU: the host plumbing of the evaluation sweep (pytorch/evaluate.py::forward) without a GPU -- the echo sweep against its host
fold, the stager coming back to the per-device cache however the sweep ends, ACX_FRONTEND checked at construction, and the
slot / turn table of tests/sweep_cases.py that the GPU ordering tests (tests/test_gpu_sweep_order.py) rely on."""
import numpy as np
import pytest
import torch

from audioset_convnext_inf_amd import _ffi
from audioset_convnext_inf_amd.pytorch import evaluate as ev
from audioset_convnext_inf_amd.pytorch.convnext import convnext_tiny
import sweep_cases as sc

CPU = torch.device("cpu")


@pytest.fixture
def seeded():
    """A stager seeded into the per-device cache, so that forward() checks out THIS object; the cache is emptied afterwards."""
    ev.drop_stagers()
    stage = ev._Stager(CPU)
    ev.release_stager(stage)
    yield stage
    ev.drop_stagers()


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_echo_sweep_equals_host_fold(dtype):
    """Both outputs of the echo model over the eleven batches, and the targets in order, equal the numpy fold bit for bit."""
    out = ev.forward(sc.EchoModel(), sc.batches(sc.SIZES, sc.L, 1, dtype), return_target=True)
    sc.assert_exact(out, sc.expected(sc.SIZES, sc.L, 1, dtype))
    assert sorted(out) == ["clipwise_output", "segmentwise_output", "target"]


def test_empty_sweep_returns_nothing_and_the_stager(seeded):
    assert ev.forward(sc.EchoModel(), iter(()), return_target=True) == {}
    assert ev._STAGERS[ev._stager_key(CPU)] is seeded


@pytest.mark.parametrize("how", ["model_first_batch", "model_second_batch", "reader_after_two"])
def test_stager_comes_back_after_an_exception(seeded, how):
    """whichever party raises and at whichever batch, the sweep hands its stager back (the next sweep then finds the
    pinned ring instead of pinning a new one) -- and a sweep after the failed one is exact on the same object."""
    model = sc.EchoModel(fail_at={"model_first_batch": 1, "model_second_batch": 2}.get(how))
    reader = sc.batches(sc.SIZES, sc.L, 2, np.int16, fail_after=2 if how == "reader_after_two" else None)
    with pytest.raises(RuntimeError, match="fails a"):
        ev.forward(model, reader, return_target=True)
    assert ev._STAGERS.get(ev._stager_key(CPU)) is seeded
    out = ev.forward(sc.EchoModel(), sc.batches(sc.SIZES, sc.L, 3, np.int16), return_target=True)
    sc.assert_exact(out, sc.expected(sc.SIZES, sc.L, 3, np.int16))
    assert ev._STAGERS.get(ev._stager_key(CPU)) is seeded


def test_failed_sweep_stops_its_reader():
    """The read-ahead generator is closed on the way out: when forward() has raised, its reader thread has ended (it would
    otherwise sit on the full queue, and on the stager's pinned ring, for as long as the traceback keeps the generator alive) and
    has pulled no more than the batches in flight."""
    import threading
    pulled = []                         # the thread that pulled each batch: forward()'s reader

    def reader():
        for b in sc.batches([2] * 50, sc.L, 4, np.int16):
            pulled.append(threading.current_thread())
            yield b

    with pytest.raises(RuntimeError, match="fails as asked") as e:
        ev.forward(sc.EchoModel(fail_at=2), reader())
    assert len(set(pulled)) == 1 and pulled[0] is not threading.current_thread()
    assert not pulled[0].is_alive()
    assert len(pulled) <= 2 + ev.kAheadDepth + 1, len(pulled)       # taken, queued, and the one being put
    del e


def test_bogus_frontend_in_the_environment_raises_at_construction(monkeypatch):
    """ACX_FRONTEND is validated where it is read, like ACX_PRECISION next to it, and the message names the allowed values."""
    def make():
        return convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
    monkeypatch.setenv("ACX_FRONTEND", "bogus")
    with pytest.raises(ValueError, match="ACX_FRONTEND") as e:
        make()
    assert all(name in str(e.value) for name in _ffi.FRONTENDS)
    for name in _ffi.FRONTENDS:
        monkeypatch.setenv("ACX_FRONTEND", name)
        assert make().frontend == name
    monkeypatch.delenv("ACX_FRONTEND")
    assert make().frontend == "auto"


def test_slot_and_turn_table():
    """Where each of the eleven int16 batches lands (pinned slot = batch mod 4, float32 turn = batch mod 3) and which buffers it
    finds too small: each replacement branch of the stager is reached, at three different slots and two different turns, in
    mid-sweep; the last batch is shorter than its buffers.  tests/test_gpu_sweep_order.py holds the real stager to this table."""
    assert ev._Stager.kRing == 4 and len(ev._Stager(CPU).dev32) == 3
    both = ("pinned", "dev16")
    assert sc.walk(sc.SIZES) == [
        (0, 0, ()), (1, 1, ()), (2, 2, ()), (3, 0, ()),
        (0, 1, ()), (1, 2, both + ("dev32",)), (2, 0, both + ("dev32",)), (3, 1, ()),
        (0, 2, both), (1, 0, both + ("dev32",)), (2, 1, ())]
    rows = sc.walk(sc.SIZES)
    assert len(sc.SIZES) > 2 * ev._Stager.kRing and len(sc.SIZES) > 3 * 3
    for name in ("pinned", "dev16", "dev32"):
        assert any(name in r[2] for r in rows), name
    assert len({r[0] for r in rows if "dev16" in r[2]}) == 3 and len({r[1] for r in rows if "dev32" in r[2]}) == 2
    assert sc.SIZES[-1] < min(sc.SIZES[:-1])
    assert sc.L % sc.CLASSES == 0
