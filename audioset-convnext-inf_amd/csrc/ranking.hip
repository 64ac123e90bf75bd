// Ranking metrics per clip (acx_ranking_metrics, include/acx.h): the integer counts behind LRAP, lwlrap, coverage error,
// label-ranking loss, one-error and precision / recall at k -- the classes of ONE row ranked against each other, where
// metrics.hip ranks the rows of one class.
//
// For a positive class j of a row, with key() the float32 bits mapped to an unsigned order (-0.0 canonicalised to +0.0:
// equal scores, equal keys; denormals keep their order whatever the float mode):
//   ge  = #{c : key_c >= key_j}    pge = #{c positive : key_c >= key_j}    ord = #{c : key_c > key_j or (key_c == key_j, c < j)}
// and per row  psum = sum_j pge / ge (float64, one correctly rounded division each, added in ascending j by one owner),
// coverage = max_j ge, bad_pairs = sum_j (ge - pge), hits_k = #{j : ord_j < k}.
//
// The row pass.  A TEAM stages its row once in LDS as keys; the positives are kept as the ballot words of the staging loop
// (word i = classes 64 i .. 64 i + 63), which IS their list in ascending index -- no atomics, and 4 KiB beside the 128 KiB
// of keys of the widest head, so every supported N fits in the CU's 160 KiB.  The team then walks the set bits in ascending
// order; for each positive its lanes stride over the staged keys, count in integers (ge and pge share one register, 16 bits
// each: both are at most 32 768) and the counts are reduced by shuffles, across waves through LDS.  Nothing is a float until
// the one division.
//   N <= kRankWaveMaxN (1 024): a team is ONE WAVE, kRankWaveRows = 4 rows per workgroup of 256 threads -- the 527-class case.
//   N >  kRankWaveMaxN:         a team is a WORKGROUP of 1 024 threads, one row each, one barrier per positive.
// The cost is O(n_pos * N) per row: right for tagging data with a few positives per clip, quadratic for dense targets on very
// wide heads (32 768 positives of 32 768 classes are 2^30 key reads for one row).  There is no second algorithm for those.
//
// The per-class sums use no float atomics.  The rows run in slices of slice_rows; the row pass writes the slice's quotients
// q[row][class] (float64, 0.0 where the class is not positive -- a positive's quotient is never 0: it counts itself) to the
// workspace, 8 * classes bytes per slice row, and ranking_column_kernel adds them per class in ascending row onto the running
// class_psum / class_count: tiles of 64 rows x 16 classes go through LDS, four to a step with the next step's four loads in
// flight; wave w owns class w, lane l holds row l, and the non-zero quotients are handed to the sum in lane order (v_readlane).
// Adding a 0.0 would not change a sum, so skipping it does not either.  The slices follow each other on the stream; the same
// inputs give the same bits on every run.
//
// Registers (gfx950, this toolchain): see the README row; no scratch in any of the three kernels.
#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kRankWaveMaxN = ACX_RANK_WAVE_MAX_CLASSES;   // 1 024: up to here a wave per row, beyond a workgroup per row
constexpr int kRankWaveRows = 4;                  // rows (waves) per workgroup of the wave-per-row form
constexpr int kRankWgWaves = 16;                  // waves of the workgroup-per-row form
constexpr int kRankColClasses = 16;               // classes per workgroup of the column pass: one 128-byte line of quotients
constexpr int kRankColTiles = 4;                  // tiles of 64 rows per step of the column pass
constexpr long long kRankSliceBytes = 1LL << 26;  // default slice: 64 MiB of quotients, at least kRankMinSliceRows rows
constexpr long long kRankMinSliceRows = 256;
constexpr long long kRankMaxSlices = 1LL << 22;   // the default slicing of 2^30 rows stays under it

__device__ __forceinline__ unsigned rank_key(float v) {
    unsigned u = __float_as_uint(v);
    if (v == 0.0f) u = 0u;                                           // -0.0 == +0.0: one key
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ double rank_readlane(double v, int lane) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// what one lane's LDS stores are to the other lanes of its team
template <int WAVES>
__device__ __forceinline__ void rank_team_sync() {
    if (WAVES > 1) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// One team of WAVES waves per row.  s_key: n keys, s_mask: ceil(n / 64) ballot words of this team, s_part: [2][WAVES][2]
// partial counts (WAVES > 1).  q: the slice's quotient rows, row_counts / row_psum: the outputs at this slice's first row.
template <int WAVES>
__device__ __forceinline__ void rank_row(const float* __restrict__ srow, const void* __restrict__ trow, int u8, int n, int k,
                                         unsigned* s_key, unsigned long long* s_mask, unsigned* s_part, int tid, double* qrow,
                                         long long* counts, double* psum_out, int* status) {
    constexpr int T = WAVES * 64;
    const int lane = tid & 63, wave = tid >> 6;
    const int words = (n + 63) >> 6;
    int bad = 0;
    for (int c0 = 0; c0 < words * 64; c0 += T) {                     // whole words: every lane of a wave votes
        const int c = c0 + tid;
        bool pos = false;
        if (c < n) {
            const float v = srow[c];
            if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) bad |= ACX_METRICS_NONFINITE;
            s_key[c] = rank_key(v);
            if (u8) {
                const unsigned char t = static_cast<const unsigned char*>(trow)[c];
                if (t > 1) bad |= ACX_METRICS_BAD_TARGET;
                pos = t != 0;
            } else {
                const float t = static_cast<const float*>(trow)[c];
                if (!(t == 0.0f || t == 1.0f)) bad |= ACX_METRICS_BAD_TARGET;
                pos = t == 1.0f;
            }
            if (!pos) qrow[c] = 0.0;
        }
        const unsigned long long b = __ballot(pos);
        if (lane == 0 && (c0 >> 6) + wave < words) s_mask[(c0 >> 6) + wave] = b;
    }
    const int bits = (__ballot(bad & ACX_METRICS_NONFINITE) ? ACX_METRICS_NONFINITE : 0) |
                     (__ballot(bad & ACX_METRICS_BAD_TARGET) ? ACX_METRICS_BAD_TARGET : 0);
    if (lane == 0 && bits) atomicOr(status, bits);
    rank_team_sync<WAVES>();

    // every thread of the team walks the same words and bits: all of the control flow below is uniform over the team
    int n_pos = 0, coverage = 0, hits = 0, step = 0;
    long long badp = 0;
    double psum = 0.0;
    for (int w0 = 0; w0 < words; w0 += 64) {
        const unsigned long long mine = w0 + lane < words ? s_mask[w0 + lane] : 0ULL;
        unsigned long long live = __ballot(mine != 0ULL);            // the words of this group of 64 that hold a positive
        while (live) {
            const int wi = w0 + __builtin_ctzll(live);
            live &= live - 1;
            unsigned long long m = s_mask[wi];
            while (m) {
                const int j = (wi << 6) + __builtin_ctzll(m);
                m &= m - 1;
                const unsigned kj = s_key[j];
                unsigned gp = 0, ord = 0;                            // ge | pge << 16, and ord
                for (int c0 = 0; c0 < n; c0 += T) {
                    const int c = c0 + tid;
                    if (c < n) {
                        const unsigned kc = s_key[c];
                        const unsigned p = (unsigned)(s_mask[c >> 6] >> (c & 63)) & 1u;
                        if (kc >= kj) gp += 1u + (p << 16);
                        ord += (kc > kj || (kc == kj && c < j)) ? 1u : 0u;
                    }
                }
                gp = wave_sum(gp);
                ord = wave_sum(ord);
                if (WAVES > 1) {
                    unsigned* part = s_part + (step & 1) * (2 * WAVES);
                    if (lane == 0) { part[2 * wave] = gp; part[2 * wave + 1] = ord; }
                    __syncthreads();                                 // one barrier per positive: the two buffers alternate
                    gp = 0; ord = 0;
#pragma unroll
                    for (int i = 0; i < WAVES; ++i) { gp += part[2 * i]; ord += part[2 * i + 1]; }
                    ++step;
                }
                const int ge = (int)(gp & 0xffffu), pge = (int)(gp >> 16);
                ++n_pos;
                coverage = max(coverage, ge);
                badp += ge - pge;
                hits += (int)ord < k ? 1 : 0;
                if (wave == 0) {                                     // the owner: ascending j, one division each
                    const double qv = (double)pge / (double)ge;
                    psum += qv;
                    if (lane == 0) qrow[j] = qv;
                }
            }
        }
    }
    if (tid == 0) {
        counts[0] = n_pos; counts[1] = coverage; counts[2] = badp; counts[3] = hits;
        *psum_out = psum;
    }
}

// N <= kRankWaveMaxN: wave w of a workgroup takes row 4 blockIdx.x + w of the slice
__global__ __launch_bounds__(kRankWaveRows * 64) void ranking_wave_kernel(const float* __restrict__ scores, long long ld_s,
                                                                          const void* __restrict__ target, int u8, long long ld_t,
                                                                          int rows, int n, int k, double* __restrict__ q,
                                                                          long long* __restrict__ row_counts,
                                                                          double* __restrict__ row_psum, int* status) {
    extern __shared__ unsigned long long s_dyn[];                    // per wave: ceil(n / 64) words, then n keys
    const int wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * kRankWaveRows + wave;
    if (r >= rows) return;                                           // no workgroup barrier in this form
    const int words = (n + 63) >> 6;
    const int per_wave = words + ((n + 1) >> 1);                     // in 8-byte units
    unsigned long long* s_mask = s_dyn + (size_t)wave * per_wave;
    unsigned* s_key = reinterpret_cast<unsigned*>(s_mask + words);
    const char* trow = static_cast<const char*>(target) + (size_t)r * ld_t * (u8 ? 1 : 4);
    rank_row<1>(scores + r * ld_s, trow, u8, n, k, s_key, s_mask, nullptr, threadIdx.x & 63, q + r * n, row_counts + r * 4,
                row_psum + r, status);
}

// N > kRankWaveMaxN: one workgroup of 1 024 threads per row of the slice
__global__ __launch_bounds__(kRankWgWaves * 64) void ranking_wg_kernel(const float* __restrict__ scores, long long ld_s,
                                                                       const void* __restrict__ target, int u8, long long ld_t,
                                                                       int rows, int n, int k, double* __restrict__ q,
                                                                       long long* __restrict__ row_counts,
                                                                       double* __restrict__ row_psum, int* status) {
    extern __shared__ unsigned long long s_dyn[];                    // ceil(n / 64) words, then n keys
    __shared__ unsigned s_part[2 * 2 * kRankWgWaves];
    const long long r = blockIdx.x;
    const int words = (n + 63) >> 6;
    unsigned long long* s_mask = s_dyn;
    unsigned* s_key = reinterpret_cast<unsigned*>(s_mask + words);
    const char* trow = static_cast<const char*>(target) + (size_t)r * ld_t * (u8 ? 1 : 4);
    rank_row<kRankWgWaves>(scores + r * ld_s, trow, u8, n, k, s_key, s_mask, s_part, threadIdx.x, q + r * n, row_counts + r * 4,
                           row_psum + r, status);
}

// class_psum[c] / class_count[c] += the slice's quotients of class c in ascending row (first: the sums start at zero)
__global__ __launch_bounds__(kRankColClasses * 64) void ranking_column_kernel(const double* __restrict__ q, int rows, int n,
                                                                              int first, long long* __restrict__ class_count,
                                                                              double* __restrict__ class_psum) {
    __shared__ double s_q[kRankColTiles][kRankColClasses][65];
    const int c0 = blockIdx.x * kRankColClasses;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = threadIdx.x & (kRankColClasses - 1), lr = threadIdx.x / kRankColClasses;      // a load: 64 rows x 16 classes
    const int c = c0 + wave;
    const bool col = c0 + lc < n;
    double acc = 0.0;
    long long cnt = 0;
    if (!first && c < n) { acc = class_psum[c]; cnt = class_count[c]; }
    double nxt[kRankColTiles];
    auto fetch = [&](long long base) {                               // the step's four tiles: four loads in flight per thread
#pragma unroll
        for (int u = 0; u < kRankColTiles; ++u) {
            const long long r = base + 64 * u + lr;
            nxt[u] = (col && r < rows) ? q[r * n + c0 + lc] : 0.0;
        }
    };
    fetch(0);
    for (long long r0 = 0; r0 < rows; r0 += 64 * kRankColTiles) {
#pragma unroll
        for (int u = 0; u < kRankColTiles; ++u) s_q[u][lc][lr] = nxt[u];
        __syncthreads();
        fetch(r0 + 64 * kRankColTiles);                              // the next step flies under this one's sums
#pragma unroll
        for (int u = 0; u < kRankColTiles; ++u) {                    // ascending row: tile after tile, lane after lane
            const double v = s_q[u][wave][lane];
            unsigned long long m = __ballot(v != 0.0);
            cnt += __popcll(m);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                acc += rank_readlane(v, b);
            }
        }
        __syncthreads();
    }
    if (lane == 0 && c < n) { class_psum[c] = acc; class_count[c] = cnt; }
}

static long long rank_slice_rows(long long rows, int classes, long long slice_rows) {
    long long s = slice_rows > 0 ? slice_rows : std::max(kRankMinSliceRows, kRankSliceBytes / (8LL * classes));
    return std::min(s, rows);
}

static int rank_check_shape(const char* who, int64_t rows, int classes, int64_t slice_rows) {
    if (rows < 1) ACX_FAIL(ACX_ERR_ARG, "%s: rows = %lld (expected >= 1)", who, (long long)rows);
    if (rows > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: rows = %lld (at most 2^30 rows)", who, (long long)rows);
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "%s: %d classes (expected 1 .. %d)", who, classes, ACX_MAX_CLASSES);
    if (slice_rows < 0 || slice_rows > kF32MaxRows)
        ACX_FAIL(ACX_ERR_ARG, "%s: slice_rows = %lld (expected 0 for the default, or 1 .. 2^30)", who, (long long)slice_rows);
    const long long s = rank_slice_rows(rows, classes, slice_rows);
    if (cdiv(rows, s) > kRankMaxSlices)
        ACX_FAIL(ACX_ERR_ARG, "%s: %lld slices of %lld rows (at most %lld)", who, cdiv(rows, s), s, kRankMaxSlices);
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_ranking_workspace_bytes(int64_t rows, int classes, int64_t slice_rows, size_t* out_bytes) {
    static const char* who = "acx_ranking_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(rank_check_shape(who, rows, classes, slice_rows));
    *out_bytes = align_up((size_t)rank_slice_rows(rows, classes, slice_rows) * (size_t)classes * sizeof(double));
    return ACX_OK;
}

int acx_ranking_metrics(const float* scores, int64_t ld_s, const void* target, int target_dtype, int64_t ld_t, int64_t rows,
                        int classes, int k, int64_t slice_rows, int64_t* row_counts, double* row_psum, int64_t* class_count,
                        double* class_psum, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_ranking_metrics";
    if (!scores || !target || !row_counts || !row_psum || !class_count || !class_psum || !status || !ws)
        ACX_FAIL(ACX_ERR_ARG, "%s: null argument", who);
    if (target_dtype != ACX_TARGET_F32 && target_dtype != ACX_TARGET_U8)
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, target_dtype);
    ACX_TRY(rank_check_shape(who, rows, classes, slice_rows));
    if (k < 1 || k > classes) ACX_FAIL(ACX_ERR_ARG, "%s: k = %d (expected 1 .. classes = %d)", who, k, classes);
    if (ld_s < classes || ld_t < classes)
        ACX_FAIL(ACX_ERR_ARG, "%s: row strides %lld / %lld are shorter than %d classes", who, (long long)ld_s, (long long)ld_t,
                 classes);
    const long long srows = rank_slice_rows(rows, classes, slice_rows);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, align_up((size_t)srows * (size_t)classes * sizeof(double))));
    const hipStream_t s = (hipStream_t)stream;
    const int u8 = target_dtype == ACX_TARGET_U8 ? 1 : 0;
    const int words = (classes + 63) / 64;
    const bool wide = classes > kRankWaveMaxN;
    const size_t team_lds = ((size_t)words + (size_t)((classes + 1) / 2)) * 8;
    if (wide) {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &ranking_wg_kernel, ((size_t)ACX_MAX_CLASSES / 64 + ACX_MAX_CLASSES / 2) * 8));
    }
    double* q = static_cast<double*>(ws);
    const char* tbase = static_cast<const char*>(target);
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    for (long long r0 = 0; r0 < rows; r0 += srows) {
        const int nr = (int)std::min<long long>(srows, rows - r0);
        const float* sp = scores + r0 * ld_s;
        const void* tp = tbase + (size_t)r0 * (size_t)ld_t * (u8 ? 1 : 4);
        long long* rc = reinterpret_cast<long long*>(row_counts) + r0 * 4;
        if (wide)
            launch_kernel(&ranking_wg_kernel, dim3((unsigned)nr), dim3(kRankWgWaves * 64), team_lds, s, sp, (long long)ld_s, tp, u8,
                          (long long)ld_t, nr, classes, k, q, rc, row_psum + r0, (int*)status);
        else
            launch_kernel(&ranking_wave_kernel, dim3((unsigned)cdiv(nr, kRankWaveRows)), dim3(kRankWaveRows * 64),
                          team_lds * kRankWaveRows, s, sp, (long long)ld_s, tp, u8, (long long)ld_t, nr, classes, k, q, rc,
                          row_psum + r0, (int*)status);
        launch_kernel(&ranking_column_kernel, dim3((unsigned)cdiv(classes, kRankColClasses)), dim3(kRankColClasses * 64), 0, s,
                      (const double*)q, nr, classes, r0 == 0 ? 1 : 0, reinterpret_cast<long long*>(class_count), class_psum);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
