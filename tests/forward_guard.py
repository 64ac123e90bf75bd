"""One forward through the raw C ABI inside guards, a plain helper imported like layer_ref.py (tests/test_gpu_forward_workspace.py,
the poison tests of test_gpu_varlen.py and test_gpu_windows.py).

  * the workspace has exactly the bytes the entry point's size call promises, as a layer_ref.Guarded payload: canaries lie directly
    in front of it and behind it, and it is prefilled with a poison;
  * every device input (waveform, feature map, augmentation plans) lives in a Guarded tensor: a read past either end of the batch
    meets canary words, and the input must come back unchanged;
  * every output is a Guarded tensor prefilled with NaN: an element nobody wrote stays NaN.

The call runs once per poison.  0xFF is a NaN as fp32, fp16 and bf16.  A NaN alone can be swallowed: fmaxf(NaN, 1e-10) is 1e-10 (the
dense frontend's log-mel clamp), and a max pool drops NaNs the same way.  0x7F is 3.4e38 as fp32 and bf16 and a NaN as fp16: it
survives every fmaxf and turns into inf or into a different number at the first multiply.  Scratch that is read before it was
written therefore changes the result between the two runs, or makes it non-finite in one of them.
"""
import torch

import layer_ref as lr
from audioset_convnext_inf_amd import _ffi

POISONS = (0xFF, 0x7F)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_guarded(need, inputs, out_shapes, call, poisons=POISONS):
    """call(ws, ins, outs) -> the entry point's return code, with ws a uint8 view of exactly `need` bytes, ins the guarded copies of
    `inputs` (device tensors) and outs fp32 tensors of `out_shapes` (None: the call has no such output).  Runs it once per poison;
    asserts after each run that every canary is intact, that every output element was written and is finite and that the inputs
    are unchanged, and afterwards that the runs agree bit for bit.  Returns the outputs of the first run."""
    runs = []
    for poison in poisons:
        gws, ws = lr.Guarded.scratch(need, fill=poison)
        assert need % 4 == 0 and ws.numel() == need and ws.data_ptr() % 256 == 0
        gin = [lr.Guarded.tensor(t) for t in inputs]
        gout = [None if s is None else lr.Guarded.filled(tuple(s)) for s in out_shapes]
        _ffi.check(call(ws, [v for _, v in gin], [None if o is None else o[1] for o in gout]))
        torch.cuda.synchronize()
        assert gws.intact(), "canary at the workspace overwritten (poison 0x%02X)" % poison
        for k, ((g, v), t) in enumerate(zip(gin, inputs)):
            assert g.intact(), "canary at input %d overwritten" % k
            assert torch.equal(v.view(torch.uint8), t.contiguous().view(torch.uint8)), "input %d changed" % k
        for k, o in enumerate(gout):
            if o is not None:
                assert o[0].intact(), "canary at output %d overwritten" % k
                assert bool(torch.isfinite(o[1]).all()), "output %d: unwritten or non-finite elements (poison 0x%02X)" % (k, poison)
        runs.append([None if o is None else o[1] for o in gout])
    for other in runs[1:]:
        for k, (a, b) in enumerate(zip(runs[0], other)):
            assert a is None or same_bits(a, b), "output %d depends on the workspace's poison" % k
    return runs[0]
