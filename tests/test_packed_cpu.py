"""CPU: the packed-batch indexing of csrc/packed.h (lengths by value, prefix sums, the search for the entry that owns a flat
index, the windows that cover a midpoint), compiled for the host from the header the HIP kernels include (tests/packed_check.cpp)
and checked against brute force."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from audioset_convnext_inf_amd.pytorch import windows as win

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I64 = ctypes.c_int, ctypes.c_longlong


@pytest.fixture(scope="module")
def packed():
    so = os.path.join(ROOT, "build", "libpackedcheck.so")
    srcs = [os.path.join(ROOT, "tests", "packed_check.cpp"), os.path.join(ROOT, "audioset-convnext-inf_amd", "csrc", "packed.h")]
    if not os.path.isfile(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.acx_packed_find_all_i32.argtypes = lib.acx_packed_find_all_i64.argtypes = [ctypes.c_void_p, I32, I32, I64, ctypes.c_void_p]
    lib.acx_packed_prefix_i32.argtypes = lib.acx_packed_prefix_i64.argtypes = [ctypes.c_void_p, I32, ctypes.c_void_p]
    lib.acx_packed_prefix_i32.restype, lib.acx_packed_prefix_i64.restype = I32, I64
    lib.acx_packed_lens.argtypes = [ctypes.c_void_p, I32, ctypes.c_void_p, ctypes.c_void_p]
    lib.acx_win_mid.argtypes, lib.acx_win_mid.restype = [I64] * 3, I64
    lib.acx_win_cover_all.argtypes = [I64] * 3 + [ctypes.c_void_p] * 2
    lib.acx_win_cover.argtypes = [I64] * 4 + [ctypes.c_void_p] * 2
    return lib


def prefix(lib, counts, dtype):
    counts = np.ascontiguousarray(counts, dtype=dtype)
    off = np.full(len(counts) + 1, -1, dtype=dtype)
    fn = lib.acx_packed_prefix_i32 if dtype == np.int32 else lib.acx_packed_prefix_i64
    total = fn(counts.ctypes.data, len(counts), off.ctypes.data)
    return off, total


def count_sets(n):
    """Per-entry counts with zeros in every position: leading, trailing, runs in the middle, and none at all."""
    rs = np.random.RandomState(n)
    sets = [rs.randint(1, 6, size=n), rs.randint(0, 4, size=n), np.where(rs.rand(n) < 0.6, 0, rs.randint(1, 9, size=n))]
    lead = rs.randint(0, 5, size=n)
    lead[:max(1, n // 3)] = 0
    trail = rs.randint(0, 5, size=n)
    trail[-max(1, n // 3):] = 0
    both = rs.randint(1, 5, size=n)
    both[0] = both[-1] = 0
    return sets + [lead, trail, both]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n", [1, 2, 255, 256])
def test_prefix_and_find_against_brute_force(packed, n, dtype):
    find = packed.acx_packed_find_all_i32 if dtype == np.int32 else packed.acx_packed_find_all_i64
    for counts in count_sets(n):
        off, total = prefix(packed, counts, dtype)
        want = np.concatenate([[0], np.cumsum(counts)])
        assert np.array_equal(off, want) and total == want[-1]
        for gap in (0, 3):
            # unit v belongs to entry i when it is one of the entry's count[i] units or of the gap units after them
            owner = np.repeat(np.arange(n), np.asarray(counts) + gap)
            assert len(owner) == total + gap * n
            got = np.full(len(owner), -1, dtype=np.int32)
            find(off.ctypes.data, n, gap, len(owner), got.ctypes.data)
            assert np.array_equal(got, owner), (n, gap, counts)
            if gap == 0 and total:          # never an empty entry: the last of the entries that share an offset owns it
                assert np.all(np.asarray(counts)[got] > 0)


def test_lengths_by_value(packed):
    lengths = np.array([0, 1, 7360, 2 ** 31 - 1], dtype=np.int64)
    n, out = ctypes.c_int(-1), np.full(256, -1, dtype=np.int32)
    packed.acx_packed_lens(lengths.ctypes.data, 4, ctypes.byref(n), out.ctypes.data)
    assert n.value == 4 and np.array_equal(out[:4], lengths) and not out[4:].any()      # the unused slots are zero


def test_win_cover_is_the_definition_exhaustively(packed):
    """{j : s_j <= m < s_j + W} for W = 1..12, H = 1..W, L = 1..40 and every m: 63 960 cases, none of them empty."""
    cases = 0
    for W in range(1, 13):
        for H in range(1, W + 1):
            for L in range(1, 41):
                n = 1 if L <= W else 1 + (L - W + H - 1) // H
                starts = [min(j * H, max(0, L - W)) for j in range(n)]
                j0, j1 = np.empty(L, dtype=np.int64), np.empty(L, dtype=np.int64)
                packed.acx_win_cover_all(L, W, H, j0.ctypes.data, j1.ctypes.data)
                for m in range(L):
                    js = [j for j, s in enumerate(starts) if s <= m < s + W]
                    assert js and js == list(range(j0[m], j1[m])), (W, H, L, m)
                    cases += 1
    assert cases == 63960


# (window, hop, lengths) of tests/test_gpu_windows.py
GPU_SIZES = [(320000, 32000, [1193600, 320000, 61 * 32000]), (48000, 7000, [100001, 30000, 48000]), (16000, 16000, [64321]),
             (48000, 17000, [130001, 48000, 97777]), (64000, 9000, [200000, 64000, 151234]), (48000, 16000, [150000, 60001]),
             (7360, 3680, [1, 7359, 7360, 7361, 11040, 22097]), (7360, 7360, [1, 7359, 7360, 7361, 11040, 22097])]


@pytest.mark.parametrize("W, H, lengths", GPU_SIZES)
def test_win_mid_and_cover_match_the_python_definition(packed, W, H, lengths):
    for L in lengths:
        starts = win.window_starts([L], W, H)
        steps = win.timeline_steps([L], W, H)
        for k, m in enumerate(steps):
            assert packed.acx_win_mid(k, H, L) == m
            j0, j1 = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
            packed.acx_win_cover(m, L, W, H, ctypes.byref(j0), ctypes.byref(j1))
            assert [j for j, s in enumerate(starts) if s <= m < s + W] == list(range(j0.value, j1.value)), (W, H, L, k)
