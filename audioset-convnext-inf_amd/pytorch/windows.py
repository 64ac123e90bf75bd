"""Sliding windows over long recordings (ConvNeXt.forward_windows, acx_forward_windows / acx_window_timeline in include/acx.h):
the host-side enumeration of windows and timeline steps, one definition shared with the C ABI.

All lengths are in samples at 32 kHz.  A recording of L samples, windows of W samples every H samples (1 <= H <= W):
  - n = 1 window if L <= W, else 1 + ceil((L - W) / H);
  - window j starts at s_j = min(j H, max(0, L - W)) -- the last window ends with the recording -- and holds min(W, L) samples;
  - the timeline has ceil(L / H) steps; step k has the midpoint m_k = min(k H + H // 2, L - 1) and reduces over the windows
    with s_j <= m_k < s_j + W (mean: an fp32 sum in ascending j, then one division by their count; or max).
Windows and steps are numbered recording by recording."""
from fractions import Fraction

from .. import _ffi

MODEL_RATE = 32000


def seconds_to_samples(seconds, name="window", rate=MODEL_RATE):
    """seconds -> samples at `rate`; a duration that is not a whole number of samples raises ValueError."""
    if isinstance(seconds, bool) or not isinstance(seconds, (int, float, Fraction)):
        raise ValueError("%s must be a number of seconds (got %r)" % (name, seconds))
    exact = Fraction(repr(seconds)) if isinstance(seconds, float) else Fraction(seconds)
    n = exact * rate
    if n.denominator != 1:
        raise ValueError("%s of %r s is not a whole number of samples at %d Hz" % (name, seconds, rate))
    return int(n)


def check_window(window, hop):
    """The argument checks of the C ABI (ValueError): window >= MIN_SAMPLES and 1 <= hop <= window."""
    if window < _ffi.MIN_SAMPLES:
        raise ValueError("window of %d samples is too short: kernel size can't be greater than actual input size "
                         "(minimum is %d samples)" % (window, _ffi.MIN_SAMPLES))
    if not 1 <= hop <= window:
        raise ValueError("hop of %d samples must be in [1, window = %d]: a longer hop leaves audio uncovered" % (hop, window))


def window_count(L, window, hop):
    return 1 if L <= window else 1 + (L - window + hop - 1) // hop


def window_starts(lengths, window, hop):
    """Sample starts (within each recording) of all windows, in window order."""
    check_window(window, hop)
    out = []
    for L in lengths:
        last = max(0, L - window)
        out.extend(min(j * hop, last) for j in range(window_count(L, window, hop)))
    return out


def timeline_steps(lengths, window, hop):
    """Midpoints m_k (samples within each recording) of all timeline steps, in row order: ceil(L / hop) per recording."""
    check_window(window, hop)
    out = []
    for L in lengths:
        out.extend(min(k * hop + hop // 2, L - 1) for k in range((L + hop - 1) // hop))
    return out
