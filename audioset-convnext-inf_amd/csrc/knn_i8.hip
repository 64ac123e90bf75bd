// Two-stage nearest-neighbour search (acx_knn_quantize_i8 / acx_knn_search_i8 / acx_knn_rescore, include/acx.h): a coarse
// search on per-row int8 codes on the i8 matrix cores, then the exact fp32 scores of a short candidate list.
//
//   knn_quantize_i8_kernel  one wave per row: y = x * inv_norm, amax = max |y| (order-free), g = 127 / amax,
//                           code = clamp(rint(y g), -127, 127), scale = amax / 127; pad columns up to a multiple of 32 are
//                           written as zeros.  Every product and quotient is rounded on its own (no contraction, no fast-math).
//   knn_search_i8_kernel    knn_search_kernel's grid (query tiles) x (slices), steps of 256 rows, candidate buffers, trim and
//                           slice lists (knn_common.h), with the 32 x 32 score tiles formed by v_mfma_i32_32x32x32_i8: the dot
//                           product of two code rows is exact in int32, and score = ((float)t * sq[i]) * sd[j] is one
//                           conversion and cos_scale's two products.  The query tile's codes are staged once per workgroup in
//                           LDS in fragment order (where they fit beside the candidate buffers; read from global memory
//                           otherwise), database codes stream from global memory, 64 contiguous bytes per lane and four MFMA
//                           steps, the next group in flight while the current one is multiplied.
//                           Filter: the queries' thresholds are kept as fp32 scores in registers (they change only in a trim),
//                           so a score costs a conversion, two products and one compare; only a score that reaches its
//                           query's threshold builds its key and goes through the exact key comparison, the exclusion test
//                           and the slot atomic.
//                           The workgroup is CU-EXCLUSIVE (acx_internal.h): all 160 KB of LDS requested, 256
//                           threads x 512 registers claimed (tools/check_exclusive.py).
//   knn_merge_keys_kernel   the first level of a two-level merge (many slices, room in the workspace): one wave per (query,
//                           group of slices), keys out; knn_merge_kernel (knn.hip) finishes every search.
//   knn_rescore_kernel      one wave per query: dot_tile with the query row as every A row and the candidates as B rows, so
//                           candidate r's score stands in every accumulator row of column r -- the bits acx_knn_search gives the
//                           pair -- then cos_scale, keys, knn_sort_desc in registers, the first k out.
//
// Operand map of the i8 MFMA.  Lane (r = lane % 32, h = lane / 32) passes 16 bytes of row r as A (queries) or B (database);
// the C/D map is F32Tile<32>::row (lane = database column, register i = query row(i, h)).  Which 16 of the 32 contraction
// columns of a step a lane half holds does not matter to a dot product as long as A and B agree, and both use chunk_of()
// below; tests/test_gpu_retrieval_i8.py derives the row / column map from identity queries against an asymmetric database.
#include <cmath>
#include <type_traits>

#include "acx_internal.h"
#include "device_common.h"
#include "knn_common.h"

namespace acx {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// ---- quantise ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_quantize_i8_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ inv_norm,
                                                              long long n, int dim, signed char* __restrict__ codes, long long ld_c,
                                                              float* __restrict__ scale, int* status) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + row * ld;
    const float inv = inv_norm ? inv_norm[row] : 1.f;
    float amax = 0.f;
    bool bad = false;
    for (int k = lane * 4; k < dim; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + k);
        const float y[4] = {v.x * inv, v.y * inv, v.z * inv, v.w * inv};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bad |= acx_nonfinite(y[e]);
            amax = fmaxf(amax, fabsf(y[e]));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    bad = __ballot(bad) != 0ull;
    const bool zero = bad || amax == 0.f;
    const float g = 127.0f / amax;
    const int dim_pad = (dim + ACX_KNN_I8_K - 1) & ~(ACX_KNN_I8_K - 1);
    signed char* cr = codes + row * ld_c;
    for (int k = lane * 4; k < dim_pad; k += 256) {
        unsigned packed = 0u;
        if (!zero && k < dim) {
            const float4 v = *reinterpret_cast<const float4*>(xr + k);
            const float y[4] = {v.x * inv, v.y * inv, v.z * inv, v.w * inv};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c = fminf(fmaxf(rintf(y[e] * g), -127.0f), 127.0f);
                packed |= ((unsigned)(int)c & 255u) << (8 * e);
            }
        }
        *reinterpret_cast<unsigned*>(cr + k) = packed;
    }
    if (lane == 0) {
        scale[row] = bad ? __uint_as_float(0x7fc00000u) : amax / 127.0f;
        if (bad) atomicOr(status, ACX_KNN_NONFINITE);
    }
}

// ---- coarse search ---------------------------------------------------------------------------------------------------------------
struct KnnI8P {
    const signed char* cq; long long ld_cq; const float* sq; long long nq;
    const signed char* cd; long long ld_cd; const float* sd; long long n;
    int dim, k;
    const int* exclude;
    knn_key* ws;             // [nq][slices][k]
    int* status;
    int slices; long long slice_rows;
};

// The 16-byte chunk of a code row that lane half h holds at MFMA step s (steps = dim / 32): in whole groups of four steps a
// lane owns 64 contiguous bytes; the last one to three steps take the chunks pairwise.  A bijection onto 0 .. 2 steps - 1.
__device__ __forceinline__ int chunk_of(int s, int h, int steps) {
    return s < (steps & ~3) ? 8 * (s >> 2) + 4 * h + (s & 3) : 2 * s + h;
}

// LDS of a workgroup: the candidate buffers, then per query of the tile the threshold key, the count, the excluded index, the
// scale and the threshold as an fp32 score, three flag words, then the query codes
constexpr size_t knn_i8_lds_fixed(int tq, int cap) { return (size_t)tq * cap * sizeof(knn_key) + (size_t)tq * 24 + 16; }

template <int QT, int R, bool QLDS>
__global__ __launch_bounds__(kKnnThreads) void knn_search_i8_kernel(KnnI8P p) {
    constexpr int TQ = 32 * QT, CAP = 64 * R;
    extern __shared__ __align__(16) unsigned char s_raw[];
    knn_key* s_buf = reinterpret_cast<knn_key*>(s_raw);          // [TQ][CAP]
    knn_key* s_thr = s_buf + TQ * CAP;                            // [TQ]
    int* s_cnt = reinterpret_cast<int*>(s_thr + TQ);              // [TQ]
    int* s_excl = s_cnt + TQ;                                     // [TQ]
    float* s_sq = reinterpret_cast<float*>(s_excl + TQ);          // [TQ] the queries' scales, NaN past nq: such a score passes no threshold
    float* s_thrf = s_sq + TQ;                                    // [TQ] the score of s_thr (-inf while it is 0); changes only in a trim
    int* s_over = reinterpret_cast<int*>(s_thrf + TQ);            // [3] "a lane found no slot" of round n in word n % 3
    const i32x4* s_q = reinterpret_cast<const i32x4*>(s_raw + knn_i8_lds_fixed(TQ, CAP));     // [steps][QT][64] fragments
    ACX_CLAIM_VGPR(255);          // CU-exclusive: one wave per SIMD holds the SIMD's whole register file
    ACX_CLAIM_AGPR(255);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const long long q0 = (long long)blockIdx.x * TQ;
    const long long j_lo = (long long)blockIdx.y * p.slice_rows;
    const long long j_hi = min(p.n, j_lo + p.slice_rows);
    const int steps = p.dim >> 5, groups = steps >> 2;

    bool bad = false;
    if (tid < TQ) {
        const long long qi = q0 + tid;
        s_thr[tid] = 0ull;
        s_cnt[tid] = 0;
        s_excl[tid] = (p.exclude && qi < p.nq) ? p.exclude[qi] : -1;
        const float v = p.sq[min(qi, p.nq - 1)];
        if (qi < p.nq && acx_nonfinite(v)) bad = true;
        s_sq[tid] = qi < p.nq ? v : __uint_as_float(0x7fc00000u);
        s_thrf[tid] = -INFINITY;
    }
    if (tid < 3) s_over[tid] = 0;
    // rows past nq / the slice repeat the last valid one: loads stay inside the buffers, results are dropped
    if (QLDS) {
        i32x4* dst = reinterpret_cast<i32x4*>(s_raw + knn_i8_lds_fixed(TQ, CAP));
        for (int idx = tid; idx < steps * QT * 64; idx += kKnnThreads) {
            const int l = idx & 63, t = (idx >> 6) % QT, s = idx / (64 * QT);
            const long long qi = min(q0 + 32 * t + (l & 31), p.nq - 1);
            dst[idx] = *reinterpret_cast<const i32x4*>(p.cq + qi * p.ld_cq + 16 * chunk_of(s, l >> 5, steps));
        }
    }
    const signed char* qa[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) qa[t] = p.cq + min(q0 + 32 * t + r32, p.nq - 1) * p.ld_cq;

    int round = 0;               // of the block-wide OR below
    __syncthreads();

    for (long long j0 = j_lo; j0 < j_hi; j0 += kKnnStepRows) {
        const long long jw = j0 + wave * 64;
        const bool active = jw < j_hi;               // wave-uniform
        i32x16 acc[QT][2];
        float sdv[2] = {0.f, 0.f};
        if (active) {
            const signed char* db[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long long j = jw + 32 * u + r32;
                const long long jc = min(j, j_hi - 1);
                db[u] = p.cd + jc * p.ld_cd;
                const float v = p.sd[jc];
                if (j < j_hi && acx_nonfinite(v)) bad = true;
                sdv[u] = j < j_hi ? v : __uint_as_float(0x7fc00000u);
            }
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[t][u] = i32x16(0);
            auto load_b = [&](i32x4 (&b)[2][4], int g) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int m = 0; m < 4; ++m) b[u][m] = *reinterpret_cast<const i32x4*>(db[u] + 128 * g + 64 * h + 16 * m);
            };
            auto step = [&](int s, int chunk, const i32x4 (&b)[2]) {
                i32x4 a[QT];
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    a[t] = QLDS ? s_q[(s * QT + t) * 64 + lane] : *reinterpret_cast<const i32x4*>(qa[t] + 16 * chunk);
#pragma unroll
                for (int t = 0; t < QT; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[t], b[u], acc[t][u], 0, 0, 0);
            };
            auto group = [&](const i32x4 (&b)[2][4], int g) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const i32x4 bm[2] = {b[0][m], b[1][m]};
                    step(4 * g + m, 8 * g + 4 * h + m, bm);
                }
            };
            i32x4 b0[2][4], b1[2][4];
            int g = 0;
            if (groups) load_b(b0, 0);
            for (; g + 2 <= groups; g += 2) {
                load_b(b1, g + 1);
                group(b0, g);
                if (g + 2 < groups) load_b(b0, g + 2);
                group(b1, g + 1);
            }
            if (g < groups) group(b0, g);
            for (int s = 4 * groups; s < steps; ++s) {
                const int c = 2 * s + h;
                const i32x4 bm[2] = {*reinterpret_cast<const i32x4*>(db[0] + 16 * c), *reinterpret_cast<const i32x4*>(db[1] + 16 * c)};
                step(s, c, bm);
            }
        }

        // filter the tile into the candidate buffers; lanes left without a slot try again after the trim
        unsigned long long pend = 0ull;
        auto pass = [&](auto first_tag) -> int {
            constexpr bool FIRST = decltype(first_tag)::value;
            int over = 0;
            float sqv[QT][16], thrf[QT][16];          // of this lane's 16 QT queries
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sqv[t][i] = s_sq[32 * t + F32Tile<32>::row(i, h)];
                    thrf[t][i] = s_thrf[32 * t + F32Tile<32>::row(i, h)];
                }
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int bit = (t * 2 + u) * 16 + i;
                        if (FIRST || ((pend >> bit) & 1ull)) {
                            const float s = cos_scale((float)acc[t][u][i], sqv[t][i], sdv[u]);
                            bool keep = false;
                            if (s >= thrf[t][i]) {
                                const int ql = 32 * t + F32Tile<32>::row(i, h);
                                const long long j = jw + 32 * u + r32;
                                if (j != (long long)s_excl[ql]) keep = !knn_offer<CAP>(knn_make_key(s, j), ql, s_thr, s_cnt, s_buf);
                            }
                            if (FIRST) { if (keep) pend |= 1ull << bit; }
                            else if (!keep) pend &= ~(1ull << bit);
                            over |= keep ? 1 : 0;
                        }
                    }
            return over;
        };
        bool first = true;
        for (;;) {
            int over = 0;
            if (active && first) over = pass(std::true_type());
            else if (pend) over = pass(std::false_type());
            first = false;
            // the block-wide OR of `over`: a flag word per round, cleared two rounds ahead (no static LDS: the dynamic request
            // is the whole CU's)
            if (__ballot(over) && lane == 0) s_over[round % 3] = 1;
            __syncthreads();
            const int any = s_over[round % 3];
            if (tid == 0) s_over[(round + 2) % 3] = 0;
            ++round;
            if (!any) break;
            knn_trim_full<R>(TQ, p.k, s_thr, s_cnt, s_buf, wave, lane);
            if (lane < TQ / 4) {                         // the wave's own queries: wave, wave + 4, ...
                const knn_key key = s_thr[wave + 4 * lane];
                s_thrf[wave + 4 * lane] = key ? knn_key_score(key) : -INFINITY;
            }
            __syncthreads();
        }
    }

    knn_store_slice<R>(TQ, q0, p.nq, p.k, p.slices, (int)blockIdx.y, p.ws, s_cnt, s_buf, wave, lane);
    if (__ballot(bad) && lane == 0) atomicOr(p.status, ACX_KNN_NONFINITE);
}

// ---- first level of a two-level merge -------------------------------------------------------------------------------------------
// One wave per (query, group of `per` consecutive slices): the k best keys of the group's lists, sorted, as KEYS to out
// [nq][groups][k] -- knn_merge_kernel's fold, so that knn_merge_kernel itself then folds `groups` lists instead of `slices`.
// A single query over a long database has hundreds of slices and ONE wave to merge them; the selection is on keys of one total
// order, so the result does not depend on how the lists were grouped.
template <int R>
__global__ __launch_bounds__(kKnnThreads) void knn_merge_keys_kernel(const knn_key* __restrict__ ws, long long nq, int slices, int per,
                                                                     int groups, int k, knn_key* __restrict__ out) {
    constexpr int CAP = 64 * R;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nq * groups) return;
    const long long q = w / groups;
    const int first = (int)(w % groups) * per;
    const knn_key* flat = ws + (q * slices + first) * k;
    const long long total = (long long)min(per, slices - first) * k;
    knn_key v[R];
    knn_load_sorted<R>(flat, (int)min(total, (long long)CAP), v, lane);
    for (long long pos = CAP; pos < total; pos += CAP - k) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            if (e >= k) v[r] = pos + (e - k) < total ? flat[pos + (e - k)] : 0ull;
        }
        knn_sort_desc<R>(v, lane);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        if (e < k) out[w * k + e] = v[r];
    }
}

// ---- rerank ----------------------------------------------------------------------------------------------------------------------
struct KnnRescoreP {
    const float* q; long long ld_q; const float* rq; long long nq;
    const float* d; long long ld_d; const float* rd; long long n;
    int dim;
    const int* cand; long long ld_cand; int kc, k;
    int* indices; float* scores; int* status;
};

// One wave per query.  R = 1: kc <= 64, R = 2: kc <= 128 (two passes of 64 candidates).
template <int R>
__global__ __launch_bounds__(256) void knn_rescore_kernel(KnnRescoreP p) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= p.nq) return;
    const int r32 = lane & 31, h = lane >> 5;
    const bool cosine = p.rq != nullptr;
    const float* const qa[1] = {p.q + q * p.ld_q};
    const float rqv = cosine ? p.rq[q] : 1.f;
    const int* cand = p.cand + q * p.ld_cand;
    knn_key v[R];
    bool bad = false, oob = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int idx[2];
        bool valid[2];
        const float* db[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = 64 * r + 32 * u + r32;
            idx[u] = c < p.kc ? cand[c] : -1;
            valid[u] = idx[u] >= 0 && idx[u] < p.n;
            if (idx[u] != -1 && !valid[u]) oob = true;
            db[u] = p.d + (valid[u] ? (long long)idx[u] : 0LL) * p.ld_d;      // row 0 exists: n >= 1
        }
        F32Tile<32>::acc_t acc[1][2];
        dot_tile<1>(acc, qa, db, p.dim, h, [](const float4 (&)[2], const float4 (&)[2]) {});
        // every accumulator row of column r32 holds (query, candidate 32 u + r32); lane half h keeps u = h: element lane
        float s = h ? acc[0][1][0] : acc[0][0][0];
        const int j = h ? idx[1] : idx[0];
        const bool ok = h ? valid[1] : valid[0];
        if (ok && acx_nonfinite(s)) bad = true;
        if (cosine) s = cos_scale(s, rqv, p.rd[ok ? j : 0]);
        v[r] = ok ? knn_make_key(s, j) : 0ull;
    }
    knn_sort_desc<R>(v, lane);
    const bool nonfinite = __ballot(bad) != 0ull, outside = __ballot(oob) != 0ull;
    if (lane == 0 && (nonfinite || outside))
        atomicOr(p.status, (nonfinite ? ACX_KNN_NONFINITE : 0) | (outside ? ACX_KNN_BAD_INDEX : 0));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        if (e < p.k) {
            const bool none = nonfinite || v[r] == 0ull;
            p.indices[q * p.k + e] = none ? -1 : knn_key_index(v[r]);
            p.scores[q * p.k + e] = none ? __uint_as_float(0x7fc00000u) : knn_key_score(v[r]);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static int check_i8_rows(const char* who, const char* name, const int8_t* x, int64_t ld, int dim) {
    if (!x) ACX_FAIL(ACX_ERR_ARG, "%s: %s is null", who, name);
    if (ld < dim || (ld & 15))
        ACX_FAIL(ACX_ERR_ARG, "%s: row stride of %s = %lld (expected a multiple of 16, at least %d)", who, name, (long long)ld, dim);
    if (reinterpret_cast<uintptr_t>(x) & 15) ACX_FAIL(ACX_ERR_ARG, "%s: %s is not 16-byte aligned", who, name);
    return ACX_OK;
}

static DeviceOnce g_knn_i8_lds[2][3][2];
constexpr int kKnnTwoLevelSlices = 16;       // from this many slices on, the merge runs in two levels where the workspace has room

template <int QT, int R, bool QLDS>
static int knn_i8_launch(const KnnI8P& p, long long qtiles, hipStream_t s) {
    ACX_TRY(set_max_dynamic_lds(g_knn_i8_lds[QT - 1][R == 1 ? 0 : R == 2 ? 1 : 2][QLDS], &knn_search_i8_kernel<QT, R, QLDS>, kCuLdsBytes));
    launch_kernel(&knn_search_i8_kernel<QT, R, QLDS>, dim3((unsigned)qtiles, (unsigned)p.slices), dim3(kKnnThreads),
                  kCuLdsBytes /* all of it: CU-exclusive */, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}
template <int QT, int R>
static int knn_i8_launch_q(const KnnI8P& p, long long qtiles, hipStream_t s) {
    // the query tile's codes go to LDS when they fit beside the candidate buffers
    const bool qlds = knn_i8_lds_fixed(32 * QT, 64 * R) + (size_t)32 * QT * p.dim <= kCuLdsBytes;
    return qlds ? knn_i8_launch<QT, R, true>(p, qtiles, s) : knn_i8_launch<QT, R, false>(p, qtiles, s);
}
template <int QT>
static int knn_i8_launch_r(const KnnI8P& p, int r, long long qtiles, hipStream_t s) {
    return r == 1 ? knn_i8_launch_q<QT, 1>(p, qtiles, s) : r == 2 ? knn_i8_launch_q<QT, 2>(p, qtiles, s) : knn_i8_launch_q<QT, 4>(p, qtiles, s);
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_knn_quantize_i8(const float* x, int64_t ld, const float* inv_norm, int64_t n, int dim, int8_t* codes, int64_t ld_c,
                        float* scale, int32_t* status, void* stream) {
    static const char* who = "acx_knn_quantize_i8";
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    ACX_TRY(check_f32_rows(who, "x", x, ld, dim));
    ACX_TRY(check_i8_rows(who, "codes", codes, ld_c, (dim + ACX_KNN_I8_K - 1) / ACX_KNN_I8_K * ACX_KNN_I8_K));
    if (!scale) ACX_FAIL(ACX_ERR_ARG, "%s: scale is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    launch_kernel(&knn_quantize_i8_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long long)ld, inv_norm,
                  (long long)n, dim, (signed char*)codes, (long long)ld_c, scale, (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_knn_search_i8(const int8_t* cq, int64_t ld_cq, const float* sq, int64_t nq, const int8_t* cd, int64_t ld_cd, const float* sd,
                      int64_t n, int dim, int k, const int32_t* exclude, int32_t* indices, float* scores, int32_t* status, void* ws,
                      size_t ws_bytes, void* stream) {
    static const char* who = "acx_knn_search_i8";
    ACX_TRY(knn_check_shape(who, nq, n, k));
    if (dim < ACX_KNN_I8_K || dim > ACX_KNN_MAX_DIM || dim % ACX_KNN_I8_K)
        ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected a multiple of %d in %d .. %d)", who, dim, ACX_KNN_I8_K, ACX_KNN_I8_K, ACX_KNN_MAX_DIM);
    ACX_TRY(check_i8_rows(who, "cq", cq, ld_cq, dim));
    ACX_TRY(check_i8_rows(who, "cd", cd, ld_cd, dim));
    if (!sq || !sd) ACX_FAIL(ACX_ERR_ARG, "%s: sq / sd is null", who);
    if (!indices || !scores) ACX_FAIL(ACX_ERR_ARG, "%s: indices / scores is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    if (k > n - (exclude ? 1 : 0))
        ACX_FAIL(ACX_ERR_ARG, "%s: k = %d exceeds the %lld rows a query may return%s", who, k, (long long)(n - (exclude ? 1 : 0)),
                 exclude ? " (n - 1 with exclude)" : "");
    ACX_TRY(check_workspace(ws, ws_bytes, knn_ws_bytes(nq, n, k)));
    hipStream_t s = (hipStream_t)stream;
    const KnnPlan pl = knn_plan(nq, n, k);
    KnnI8P p;
    p.cq = (const signed char*)cq; p.ld_cq = ld_cq; p.sq = sq; p.nq = nq;
    p.cd = (const signed char*)cd; p.ld_cd = ld_cd; p.sd = sd; p.n = n;
    p.dim = dim; p.k = k; p.exclude = exclude; p.ws = static_cast<knn_key*>(ws); p.status = (int*)status;
    p.slices = pl.slices; p.slice_rows = pl.slice_rows;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const long long qtiles = cdiv(nq, 32 * pl.qt);
    ACX_TRY(pl.qt == 1 ? knn_i8_launch_r<1>(p, pl.r, qtiles, s) : knn_i8_launch_r<2>(p, pl.r, qtiles, s));
    // many slices and room behind the slices' lists: merge in two levels of about sqrt(slices) lists each
    const int per = (int)std::ceil(std::sqrt((double)pl.slices)), groups = (int)cdiv(pl.slices, per);
    const size_t lists = (size_t)nq * pl.slices * k, mids = (size_t)nq * groups * k;
    if (pl.slices >= kKnnTwoLevelSlices && (lists + mids) * sizeof(knn_key) <= ws_bytes) {
        knn_key* mid = p.ws + lists;
        const dim3 grid((unsigned)cdiv(nq * groups, 4));
        if (pl.r == 1) launch_kernel(&knn_merge_keys_kernel<1>, grid, dim3(kKnnThreads), 0, s, (const knn_key*)p.ws, (long long)nq, pl.slices, per, groups, k, mid);
        else if (pl.r == 2) launch_kernel(&knn_merge_keys_kernel<2>, grid, dim3(kKnnThreads), 0, s, (const knn_key*)p.ws, (long long)nq, pl.slices, per, groups, k, mid);
        else launch_kernel(&knn_merge_keys_kernel<4>, grid, dim3(kKnnThreads), 0, s, (const knn_key*)p.ws, (long long)nq, pl.slices, per, groups, k, mid);
        ACX_HIP(hipGetLastError());
        return knn_launch_merge(mid, nq, groups, k, pl.r, (int*)indices, scores, (const int*)status, s);
    }
    return knn_launch_merge(p.ws, nq, pl.slices, k, pl.r, (int*)indices, scores, (const int*)status, s);
}

int acx_knn_rescore(const float* q, int64_t ld_q, const float* q_inv_norm, int64_t nq, const float* d, int64_t ld_d,
                    const float* d_inv_norm, int64_t n, int dim, int metric, const int32_t* cand, int64_t ld_cand, int kc, int k,
                    int32_t* indices, float* scores, int32_t* status, void* stream) {
    static const char* who = "acx_knn_rescore";
    ACX_TRY(knn_check_shape(who, nq, n, kc));
    if (k < 1 || k > kc) ACX_FAIL(ACX_ERR_ARG, "%s: k = %d (expected 1 .. kc = %d)", who, k, kc);
    if (metric != ACX_KNN_DOT && metric != ACX_KNN_COSINE)
        ACX_FAIL(ACX_ERR_ARG, "%s: metric %d (expected ACX_KNN_DOT or ACX_KNN_COSINE)", who, metric);
    ACX_TRY(check_f32_rows(who, "q", q, ld_q, dim));
    ACX_TRY(check_f32_rows(who, "d", d, ld_d, dim));
    if (metric == ACX_KNN_COSINE && (!q_inv_norm || !d_inv_norm))
        ACX_FAIL(ACX_ERR_ARG, "%s: q_inv_norm / d_inv_norm is null with ACX_KNN_COSINE", who);
    if (!cand) ACX_FAIL(ACX_ERR_ARG, "%s: cand is null", who);
    if (ld_cand < kc) ACX_FAIL(ACX_ERR_ARG, "%s: ld_cand = %lld is shorter than kc = %d", who, (long long)ld_cand, kc);
    if (!indices || !scores) ACX_FAIL(ACX_ERR_ARG, "%s: indices / scores is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    hipStream_t s = (hipStream_t)stream;
    KnnRescoreP p;
    p.q = q; p.ld_q = ld_q; p.rq = metric == ACX_KNN_COSINE ? q_inv_norm : nullptr; p.nq = nq;
    p.d = d; p.ld_d = ld_d; p.rd = metric == ACX_KNN_COSINE ? d_inv_norm : nullptr; p.n = n;
    p.dim = dim; p.cand = (const int*)cand; p.ld_cand = ld_cand; p.kc = kc; p.k = k;
    p.indices = (int*)indices; p.scores = scores; p.status = (int*)status;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const dim3 grid((unsigned)((nq + 3) / 4));
    if (kc <= 64) launch_kernel(&knn_rescore_kernel<1>, grid, dim3(256), 0, s, p);
    else launch_kernel(&knn_rescore_kernel<2>, grid, dim3(256), 0, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
