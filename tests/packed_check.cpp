// The packed-batch indexing of csrc/packed.h on the CPU: the very functions the HIP kernels and their launchers call,
// exported for tests/test_packed_cpu.py.  Test infrastructure only.
#include "../audioset-convnext-inf_amd/csrc/packed.h"
using namespace acx;

// owner[v] = packed_find(off, n, v, gap) for every v in [0, total)
extern "C" void acx_packed_find_all_i32(const int* off, int n, int gap, long long total, int* owner) {
    for (long long v = 0; v < total; ++v) owner[v] = packed_find(off, n, v, gap);
}
extern "C" void acx_packed_find_all_i64(const long long* off, int n, int gap, long long total, int* owner) {
    for (long long v = 0; v < total; ++v) owner[v] = packed_find(off, n, v, gap);
}

// off[0 .. n] = the exclusive prefix of count[0 .. n - 1]; returns the total
extern "C" int acx_packed_prefix_i32(const int* count, int n, int* off) {
    return packed_prefix(n, off, [count](int i) { return count[i]; });
}
extern "C" long long acx_packed_prefix_i64(const long long* count, int n, long long* off) {
    return packed_prefix(n, off, [count](int i) { return count[i]; });
}

extern "C" void acx_packed_lens(const int64_t* lengths, int n, int* out_n, int* out_len) {
    const PackedLens a = packed_lens(lengths, n);
    *out_n = a.n;
    for (int i = 0; i < kVarMaxClips; ++i) out_len[i] = a.len[i];
}

extern "C" long long acx_win_mid(long long k, long long step, long long L) { return win_mid(k, step, L); }
// j0[m], j1[m] = win_cover(m, L, W, H) for every m in [0, L)
extern "C" void acx_win_cover_all(long long L, long long W, long long H, long long* j0, long long* j1) {
    for (long long m = 0; m < L; ++m) win_cover(m, L, W, H, &j0[m], &j1[m]);
}
extern "C" void acx_win_cover(long long m, long long L, long long W, long long H, long long* j0, long long* j1) {
    win_cover(m, L, W, H, j0, j1);
}
