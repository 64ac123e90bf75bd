// Geometry tables of a variable-length batch (acx_forward_varlen).  The host knows the B clip lengths; the kernels need, per
// clip, where its samples, frames and image rows start, and, per row, which clip it belongs to.  One kernel writes all of them
// into the head of the forward's workspace: the lengths travel BY VALUE as a kernel argument, so the call stays free of
// host -> device copies (a pageable copy is not capturable), allocations and synchronisation.
#include "acx_internal.h"

namespace acx {

struct VarTabOut {
    long long* soff; int* foff; int* roff[4]; int* vclip[4]; unsigned* vbits[4]; int* rclip0; int* irow[4];
    int rows[4], vrows[4], vwords[4];
};

__global__ __launch_bounds__(256) void varlen_tables_kernel(PackedLens a, VarTabOut o) {
    __shared__ long long s_soff[kVarMaxClips + 1];
    __shared__ int s_foff[kVarMaxClips + 1];
    __shared__ int s_roff[4][kVarMaxClips + 1];
    const int B = a.n, tid = threadIdx.x;
    if (tid == 0) {                                  // B <= 256: serial prefixes are a few microseconds at most
        packed_prefix(B, s_soff, [&a](int i) { return (long long)a.len[i]; });
        packed_prefix(B, s_foff, [&a](int i) { return a.len[i] / kHop + 1; });
        for (int s = 0; s < 4; ++s) packed_prefix(B, s_roff[s], [&a, s](int i) { return stage_h0(a.len[i] / kHop + 1) >> s; });
    }
    __syncthreads();
    const long long gtid = (long long)blockIdx.x * 256 + tid, gstride = (long long)gridDim.x * 256;
    if (blockIdx.x == 0) {
        for (int i = tid; i <= B; i += 256) {
            o.soff[i] = s_soff[i];
            o.foff[i] = s_foff[i];
            for (int s = 0; s < 4; ++s) o.roff[s][i] = s_roff[s][i];
        }
    }
    for (int s = 0; s < 4; ++s) {
        const int* ro = s_roff[s];
        for (long long v = gtid; v < o.vrows[s]; v += gstride) o.vclip[s][v] = packed_find(ro, B, v, 3);
        for (long long w = gtid; w < o.vwords[s]; w += gstride) {
            unsigned bits = 0;
            for (int j = 0; j < 32; ++j) {
                const long long v = 32 * w + j - 32;
                if (v < 0 || v >= o.vrows[s]) continue;
                const int c = packed_find(ro, B, v, 3);
                if (v - (ro[c] + 3 * c) < ro[c + 1] - ro[c]) bits |= 1u << j;
            }
            o.vbits[s][w] = bits;
        }
        if (s == 0) {
            for (long long r = gtid; r < o.rows[0]; r += gstride) o.rclip0[r] = packed_find(ro, B, r);
        } else {
            const int* rp = s_roff[s - 1];
            for (long long r = gtid; r < o.rows[s]; r += gstride) {
                const int c = packed_find(ro, B, r);
                o.irow[s][r] = rp[c] + 2 * ((int)r - ro[c]);
            }
        }
    }
}

int varlen_geometry(const int64_t* lengths, int B, char* ws, VarGeom* vg, size_t* bytes) {
    if (B <= 0 || B > kVarMaxClips)
        ACX_FAIL(ACX_ERR_ARG, "variable-length batch of %d clips (expected 1 .. %d)", B, kVarMaxClips);
    if (!lengths) ACX_FAIL(ACX_ERR_ARG, "variable-length batch: lengths is null");
    VarGeom g{};
    g.B = B;
    long long frames = 0, rows[4] = {0, 0, 0, 0};
    for (int i = 0; i < B; ++i) {
        const int64_t L = lengths[i];
        if (L < ACX_MIN_SAMPLES)
            ACX_FAIL(ACX_ERR_SHAPE,
                     "clip %d of %lld samples is too short: the last 2x2 downsample needs at least %d samples "
                     "(kernel size can't be greater than actual input size)", i, (long long)L, ACX_MIN_SAMPLES);
        if (L > 0x7fffffffLL) ACX_FAIL(ACX_ERR_SHAPE, "clip %d of %lld samples is longer than 2^31 - 1", i, (long long)L);
        g.samples += L;
        const int T = (int)(L / kHop + 1);
        frames += T;
        if (T > g.maxT) g.maxT = T;
        int h = stage_h0(T);
        for (int s = 0; s < 4; ++s) {
            rows[s] += h;
            if (h > g.maxH[s]) g.maxH[s] = h;
            h /= 2;
        }
    }
    if (frames >= (1LL << 31) || rows[0] * kStemW >= (1LL << 31))
        ACX_FAIL(ACX_ERR_SHAPE, "variable-length batch of %lld frames is too large for one forward", frames);
    g.frames = (int)frames;
    for (int s = 0; s < 4; ++s) {
        g.rows[s] = (int)rows[s];
        g.vrows[s] = (int)rows[s] + 3 * B;
        g.vwords[s] = (g.vrows[s] + 32) / 32 + 2;         // bits of virtual rows -32 .. vrows - 1, then zero words
    }
    size_t off = 0;
    char* base = ws;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += align_up(n); return p; };
    g.soff = reinterpret_cast<const long long*>(take((size_t)(B + 1) * 8));
    g.foff = reinterpret_cast<const int*>(take((size_t)(B + 1) * 4));
    for (int s = 0; s < 4; ++s) g.roff[s] = reinterpret_cast<const int*>(take((size_t)(B + 1) * 4));
    for (int s = 0; s < 4; ++s) g.vclip[s] = reinterpret_cast<const int*>(take((size_t)g.vrows[s] * 4));
    for (int s = 0; s < 4; ++s) g.vbits[s] = reinterpret_cast<const unsigned*>(take((size_t)g.vwords[s] * 4));
    g.rclip0 = reinterpret_cast<const int*>(take((size_t)g.rows[0] * 4));
    g.irow[0] = nullptr;
    for (int s = 1; s < 4; ++s) g.irow[s] = reinterpret_cast<const int*>(take((size_t)g.rows[s] * 4));
    *vg = g;
    *bytes = off;
    return ACX_OK;
}

int launch_varlen_tables(const int64_t* lengths, const VarGeom& g, hipStream_t s) {
    VarTabOut o{};
    o.soff = const_cast<long long*>(g.soff);
    o.foff = const_cast<int*>(g.foff);
    for (int st = 0; st < 4; ++st) {
        o.roff[st] = const_cast<int*>(g.roff[st]);
        o.vclip[st] = const_cast<int*>(g.vclip[st]);
        o.vbits[st] = const_cast<unsigned*>(g.vbits[st]);
        o.irow[st] = const_cast<int*>(g.irow[st]);
        o.rows[st] = g.rows[st]; o.vrows[st] = g.vrows[st]; o.vwords[st] = g.vwords[st];
    }
    o.rclip0 = const_cast<int*>(g.rclip0);
    long long blocks = ((long long)g.vrows[0] + 255) / 256;
    if (blocks > 256) blocks = 256;
    if (blocks < 1) blocks = 1;
    launch_kernel(&varlen_tables_kernel, dim3((unsigned)blocks), dim3(256), 0, s, packed_lens(lengths, g.B), o);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx
