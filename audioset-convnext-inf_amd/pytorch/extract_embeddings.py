"""Variable-length extraction ("next" row 4 of SURVEY.md 8f).  The reference's `pytorch/extract_embeddings.py`
(:64-99) feeds un-padded clips of arbitrary length one at a time (bs=1).  The model is fully convolutional, so
clips of EQUAL length can share a launch: this helper buckets clips by length, runs each bucket as one batch
(chunked to `max_batch`) and returns results in the original order.  Output length follows
T' = ((L//320 + 1) + 4)//4 + 1 -> //2 -> //2 -> //2.

extract(..., sample_rate=r) takes clips at any integer rate (the reference's script loads 44.1 kHz Clotho WAVs through
librosa.load(sr=32000) on the host): they cross PCIe at their own rate and are resampled to 32 kHz on the device
(acx_resample) before the forward; bucketing and packing see the resampled lengths."""
import torch

from . import resample as _rs


def bucket_by_length(lengths):
    """-> {length: [indices]} preserving first-seen order of lengths."""
    buckets = {}
    for i, n in enumerate(lengths):
        buckets.setdefault(int(n), []).append(i)
    return buckets


def pack_groups(lengths, max_batch=64, max_samples=64 * 320000):
    """Indices grouped for packed (variable-length) forwards: sorted by length, at most `max_batch` clips and -- unless one clip
    alone is longer -- at most `max_samples` samples per group."""
    order = sorted(range(len(lengths)), key=lambda i: -int(lengths[i]))
    groups, cur, tot = [], [], 0
    for i in order:
        n = int(lengths[i])
        if cur and (len(cur) >= max_batch or tot + n > max_samples):
            groups.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n
    if cur:
        groups.append(cur)
    return groups


@torch.no_grad()
def _extract_packed(model, waveforms, what, max_batch, max_samples, rate=None):
    import numpy as np
    device = next(model.parameters()).device
    n = len(waveforms)
    out = [None] * n
    lens = [len(w) for w in waveforms]
    groups = pack_groups(lens if rate is None else [_rs.resampled_length(L, rate) for L in lens], max_batch, max_samples)
    sizes = [sum(len(waveforms[i]) for i in g) for g in groups]
    pin = torch.empty(max(sizes), dtype=torch.float32).pin_memory()
    pin_np = pin.numpy()
    staged = torch.cuda.Event()
    staged.record()
    rows = None
    for g, size in zip(groups, sizes):
        staged.synchronize()                                       # the previous group has left the pinned buffer
        lengths, off = [], 0
        for i in g:
            w = waveforms[i]
            w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
            np.copyto(pin_np[off:off + len(w)], w, casting="same_kind")
            lengths.append(len(w))
            off += len(w)
        packed = pin[:size].to(device, non_blocking=True)
        staged.record()
        res = model.forward_varlen(packed, lengths, what=what, sample_rate=rate)
        if what == "frame":                                        # one device -> host copy per output buffer, not per clip
            hosts = {}
            for j, i in enumerate(g):
                v = res[j]
                base = v._base if v._base is not None else v
                if id(base) not in hosts:
                    hosts[id(base)] = (base, base.cpu())
                o = v.storage_offset() - base.storage_offset()
                out[i] = hosts[id(base)][1].reshape(-1)[o:o + v.numel()].view(v.shape).clone()
            continue
        res = res["clipwise_logits"] if what == "logits" else res
        if rows is None:
            rows = torch.empty(n, res.shape[1], dtype=res.dtype, device=device)
        rows[torch.as_tensor(g, device=device)] = res
    if rows is not None:
        rows = rows.cpu()
        for i in range(n):
            out[i] = rows[i].clone()
    return out


@torch.no_grad()
def extract(model, waveforms, what="logits", max_batch=64, pack=False, max_samples=64 * 320000, sample_rate=None):
    """waveforms: list of 1-D float tensors/arrays of arbitrary lengths (>= 7360 samples).
    what: 'logits' -> (N,) (the head's classes, 527 for AudioSet), 'scene' -> (768,), 'frame' -> (768, T', 7) per clip.
    Returns a list (CPU tensors, input order).

    The host side is kept off the critical path (with one clip per launch a forward is ~1.5 ms; torch.stack on a many-core host,
    a pageable copy and a synchronising .cpu() per clip cost ten times that): chunks run largest first, so the model's workspace
    and the pinned staging buffer are sized once instead of growing with every longer clip; a chunk's clips are copied into the
    pinned buffer with plain memcpys and cross PCIe asynchronously; logits / scene rows collect in one device tensor that is
    fetched once at the end (frame embeddings, whose shapes differ, are fetched per chunk).

    pack=True: clips of any lengths share a launch (model.forward_varlen): sorted by length, at most `max_batch` clips and
    `max_samples` samples per call.  Same results, bit for bit.

    sample_rate: the rate of every clip (None or 32000: the model's own).  Any other integer rate is resampled to 32 kHz on the
    device after the pinned copy (acx_resample); the length limits above (7360 samples,
    `max_samples`) then count 32 kHz samples.  Results equal
    extract() of the clips resampled first with pytorch.resample.resample, bit for bit."""
    rate = _rs.check_rate(sample_rate) if sample_rate is not None else None
    if rate == _rs.MODEL_RATE:
        rate = None
    if rate is not None:
        for i, w in enumerate(waveforms):
            _rs.check_min_length(len(w), rate, index=i)
    if pack:
        if what not in ("logits", "scene", "frame"):
            raise ValueError("what must be 'logits', 'scene' or 'frame' (got %r)" % (what,))
        return _extract_packed(model, waveforms, what, max_batch, max_samples, rate) if len(waveforms) else []
    import numpy as np
    device = next(model.parameters()).device
    fn = {"logits": lambda x: model(x)["clipwise_logits"], "scene": model.forward_scene_embeddings,
          "frame": model.forward_frame_embeddings}[what]
    n = len(waveforms)
    out = [None] * n
    if n == 0:
        return out
    lens = [len(w) for w in waveforms]
    chunks = []
    for length, idx in bucket_by_length(lens if rate is None else [_rs.resampled_length(L, rate) for L in lens]).items():
        for s in range(0, len(idx), max_batch):
            chunks.append((length, idx[s:s + max_batch]))
    chunks.sort(key=lambda c: -c[0] * len(c[1]))                   # stable: equal sizes keep their first-seen order
    if rate is not None:                 # clips of one bucket may differ in input length: staged packed, resampled to (b, length)
        return _extract_resampled(model, waveforms, fn, chunks, lens, rate, what, device)
    pin = torch.empty(chunks[0][0] * len(chunks[0][1]), dtype=torch.float32).pin_memory()
    pin_np = pin.numpy()
    staged = torch.cuda.Event()
    staged.record()
    rows = None                                                    # (n, dim) device tensor of the fixed-size outputs
    for length, chunk in chunks:
        staged.synchronize()                                       # the previous chunk has left the pinned buffer
        view = pin_np[:length * len(chunk)].reshape(len(chunk), length)
        for j, i in enumerate(chunk):
            w = waveforms[i]
            np.copyto(view[j], w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w), casting="same_kind")
        batch = pin[:length * len(chunk)].view(len(chunk), length).to(device, non_blocking=True)
        staged.record()
        res = fn(batch)
        if what == "frame":
            res = res.cpu()                                        # one device -> host copy per chunk, not one per clip
            for j, i in enumerate(chunk):
                out[i] = res[j].clone()
        else:
            if rows is None:
                rows = torch.empty(n, res.shape[1], dtype=res.dtype, device=device)
            rows[torch.as_tensor(chunk, device=device)] = res
    if rows is not None:
        rows = rows.cpu()
        for i in range(n):
            out[i] = rows[i].clone()
    return out


def _extract_resampled(model, waveforms, fn, chunks, lens, rate, what, device):
    """extract()'s bucketed loop for clips at `rate`: each chunk's clips are packed at their input lengths into the pinned
    buffer, cross PCIe, and are resampled on the device into one (b, length) batch of 32 kHz clips."""
    import numpy as np
    n = len(waveforms)
    out = [None] * n
    pin = torch.empty(max(sum(lens[i] for i in chunk) for _, chunk in chunks), dtype=torch.float32).pin_memory()
    pin_np = pin.numpy()
    staged = torch.cuda.Event()
    staged.record()
    rows = None
    for length, chunk in chunks:
        staged.synchronize()                                       # the previous chunk has left the pinned buffer
        in_lengths, off = [], 0
        for i in chunk:
            w = waveforms[i]
            w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
            np.copyto(pin_np[off:off + len(w)], w, casting="same_kind")
            in_lengths.append(len(w))
            off += len(w)
        packed = pin[:off].to(device, non_blocking=True)
        staged.record()
        batch, _ = _rs.resample(packed, rate, _rs.MODEL_RATE, lengths=in_lengths, _cache=getattr(model, "_resamplers", None))
        res = fn(batch.view(len(chunk), length))
        if what == "frame":
            res = res.cpu()
            for j, i in enumerate(chunk):
                out[i] = res[j].clone()
        else:
            if rows is None:
                rows = torch.empty(n, res.shape[1], dtype=res.dtype, device=device)
            rows[torch.as_tensor(chunk, device=device)] = res
    if rows is not None:
        rows = rows.cpu()
        for i in range(n):
            out[i] = rows[i].clone()
    return out
