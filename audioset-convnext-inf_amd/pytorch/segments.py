"""Sound event detection on the host side (ConvNeXt.forward_segments / forward_segment_embeddings, include/acx.h "sound event
detection"): the geometry of segments, frames and the segment timeline -- one definition shared with the C ABI -- and the
decoding of probabilities over time into events.  Nothing here touches the GPU.

The trunk halves time four times after a stride-4 stem on hop-320 frames, so one row of the stage-3 map -- one SEGMENT -- stands
for 32 STFT frames = 10240 samples = 0.32 s at 32 kHz.  A clip of L samples has T = L // 320 + 1 frames and
S = ((T + 4) // 4 + 1) // 8 = (T + 8) // 32 segments (acx_stage_hw(L, 3)); segment t covers samples [10240 t, 10240 (t + 1)) and the
last one reaches to the clip's end.  Frame u belongs to segment min(u // 32, S - 1): the reference's interpolate(x, 32) followed
by pad_framewise_output (pytorch/pytorch_utils.py:140-176)."""
import numpy as np

from .. import _ffi
from . import windows as _win

MODEL_RATE = 32000
HOP = 320
FRAMES_PER_SEGMENT = 32
SEGMENT_SAMPLES = _ffi.SEGMENT_SAMPLES          # 10240
SEGMENT_SECONDS = SEGMENT_SAMPLES / MODEL_RATE  # 0.32


def check_pool(pool):
    """The pooling widths of the recipe: odd, 1 .. 31 (ValueError otherwise)."""
    if isinstance(pool, bool) or not isinstance(pool, int) or not 1 <= pool <= _ffi.MAX_SEGMENT_POOL or pool % 2 == 0:
        raise ValueError("pool must be an odd integer in [1, %d] (got %r)" % (_ffi.MAX_SEGMENT_POOL, pool))
    return pool


def _check_length(L):
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < _ffi.MIN_SAMPLES:
        raise ValueError("a clip needs at least %d samples at 32 kHz (got %r)" % (_ffi.MIN_SAMPLES, L))
    return int(L)


def segment_count(L):
    """S of a clip of L samples at 32 kHz: the height of the stage-3 map, (T + 8) // 32 with T = L // 320 + 1."""
    return (_check_length(L) // HOP + 1 + 8) // FRAMES_PER_SEGMENT


def segment_edges(L, duration=None):
    """The S + 1 segment boundaries of a clip of L samples at 32 kHz, in seconds (float64 numpy): 0, 0.32, 0.64, ... and the
    clip's end -- `duration` seconds when given (the length of the audio before resampling), else L / 32000."""
    S = segment_count(L)
    edges = np.arange(S + 1, dtype=np.float64) * SEGMENT_SECONDS
    edges[S] = L / MODEL_RATE if duration is None else float(duration)
    return edges


def frame_to_segment(T, S):
    """The segment of each of T frames (int64 numpy): min(u // 32, S - 1)."""
    if T < 1 or S < 1:
        raise ValueError("frame_to_segment needs T >= 1 and S >= 1 (got %r, %r)" % (T, S))
    return np.minimum(np.arange(T, dtype=np.int64) // FRAMES_PER_SEGMENT, S - 1)


def window_segments(L, window):
    """Segments of one window of a recording of L samples: the window holds min(window, L) samples."""
    return segment_count(min(L, window))


def segment_timeline_cover(lengths, window, hop):
    """The segment timeline of forward_windows(what="segment") / acx_segment_timeline, spelled out.  Recording r of L samples has
    ceil(L / 10240) rows; row k has the midpoint m = min(10240 k + 5120, L - 1) and takes, from every window j with
    s_j <= m < s_j + min(window, L), the segment i = min((m - s_j) // 10240, S_w - 1).  Returns one list per row, in row order,
    of (recording, j, i, probs_row) in ascending j; probs_row indexes the windows' (S_w, N) blocks laid back to back in window
    order."""
    _win.check_window(window, hop)
    out, base = [], 0
    for r, L in enumerate(lengths):
        L = int(L)
        if L == 0:
            continue
        Sw = window_segments(L, window)
        span = min(window, L)
        starts = _win.window_starts([L], window, hop)
        for k in range((L + SEGMENT_SAMPLES - 1) // SEGMENT_SAMPLES):
            m = min(k * SEGMENT_SAMPLES + SEGMENT_SAMPLES // 2, L - 1)
            row = []
            for j, s in enumerate(starts):
                if s <= m < s + span:
                    i = min((m - s) // SEGMENT_SAMPLES, Sw - 1)
                    row.append((r, j, i, base + j * Sw + i))
            out.append(row)
        base += len(starts) * Sw
    return out


def median_filter(p, width):
    """Odd-width running median over axis 0; the ends repeat the first / last row."""
    if width == 1:
        return p
    h = width // 2
    padded = np.concatenate([np.repeat(p[:1], h, axis=0), p, np.repeat(p[-1:], h, axis=0)])
    return np.median(np.stack([padded[i:i + p.shape[0]] for i in range(width)]), axis=0).astype(p.dtype)


def decode_events(probs, threshold=0.5, low=None, median=1, min_duration=0.0, merge_gap=0.0, step=SEGMENT_SECONDS, labels=None):
    """Probabilities over time -> events.  probs: (steps, classes), a torch tensor or array -- "segmentwise_output" /
    "framewise_output" of one clip, or a forward_windows timeline.  Per class, after an optional odd `median` filter over time:
    an event is a maximal run of steps with p >= low that holds a value >= threshold (hysteresis; low=None: low = threshold);
    events of a class closer than `merge_gap` seconds are merged, then events shorter than `min_duration` seconds are dropped.
    step: seconds per row (0.32 for segments, 0.01 for frames), or the steps + 1 boundaries in seconds ("segment_edges").
    Returns [(class, onset_s, offset_s, peak, mean), ...] sorted by onset; class is labels[c] when labels are given, else c;
    peak / mean are taken over the event's rows of the filtered probabilities."""
    if hasattr(probs, "detach"):
        probs = probs.detach().cpu().numpy()
    p = np.asarray(probs)
    if p.ndim != 2:
        raise ValueError("decode_events expects (steps, classes) probabilities, got shape %r" % (p.shape,))
    low = threshold if low is None else low
    if not 0.0 <= low <= threshold:
        raise ValueError("low must be in [0, threshold] (got low=%r, threshold=%r)" % (low, threshold))
    if isinstance(median, bool) or not isinstance(median, int) or median < 1 or median % 2 == 0:
        raise ValueError("median must be an odd positive integer (got %r)" % (median,))
    if min_duration < 0 or merge_gap < 0:
        raise ValueError("min_duration and merge_gap must not be negative")
    if labels is not None and len(labels) != p.shape[1]:
        raise ValueError("%d labels for %d classes" % (len(labels), p.shape[1]))
    n = p.shape[0]
    if np.ndim(step) == 0:
        if not step > 0:
            raise ValueError("step must be positive (got %r)" % (step,))
        edges = np.arange(n + 1, dtype=np.float64) * float(step)
    else:
        edges = np.asarray(step, dtype=np.float64)
        if edges.shape != (n + 1,):
            raise ValueError("%d boundaries for %d steps (expected steps + 1)" % (edges.size, n))
    if n == 0:
        return []
    p = median_filter(p, median)
    events = []
    for c in np.nonzero((p >= threshold).any(axis=0))[0]:
        col = p[:, c]
        on = np.concatenate([[False], col >= low, [False]])
        begins = np.nonzero(on[1:] & ~on[:-1])[0]
        ends = np.nonzero(~on[1:] & on[:-1])[0]                 # exclusive
        runs = [[b, e] for b, e in zip(begins, ends) if col[b:e].max() >= threshold]
        merged = []
        for b, e in runs:
            if merged and edges[b] - edges[merged[-1][1]] < merge_gap:
                merged[-1][1] = e
            else:
                merged.append([b, e])
        for b, e in merged:
            if edges[e] - edges[b] < min_duration:
                continue
            events.append((labels[c] if labels is not None else int(c), float(edges[b]), float(edges[e]),
                           float(col[b:e].max()), float(col[b:e].mean())))
    events.sort(key=lambda ev: (ev[1], ev[2], str(ev[0])))
    return events
