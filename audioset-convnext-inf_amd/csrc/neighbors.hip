// Radius search, connected components and DBSCAN (acx_radius_count / acx_radius_neighbors / acx_graph_components /
// acx_dbscan_labels in include/acx.h): which rows lie within a given distance of each other, as ordered neighbour lists, and what
// is built on such lists.
//
//   radius_rowsq_kernel      xx[i] = sum x_i^2 in fp32 (row_sumsq + wave_sum, device_common.h): the bits the silhouette forms.
//   radius_tile_kernel<EMIT> one workgroup per (query tile of 256, range of database rows).  A WAVE owns 64 queries and streams its
//                            range 64 columns per step; the four waves of a workgroup take four query tiles over the same columns, so the
//                            column loads of three of them hit the cache.  The 64 x 64 tile of dot products comes from dot_tile
//                            (a pair's dot product has the bits acx_knn_search gives it) and goes straight to a keep bit per
//                            accumulator register.  One __ballot of the keep bits of register i holds the 32 columns of tile row
//                            row(i, 0) in its low word and those of row(i, 1) in its high word: a kept pair's rank inside its row
//                            and step is a popcount below the lane's bit, and lane r carries row r's running count.  No barrier
//                            in the loop, no atomic, no LDS traffic but the queries' norms; ascending database index comes for
//                            free.  EMIT = false writes the count of each (query, range) to the workspace; EMIT = true starts
//                            from the scanned counts and stores index (and value) of every kept pair at its final position.
//                            Neither the (nq, n) values nor a mask are ever written.
//   nb_scan_*                the exclusive scan of the (query, range) counts in that order, int32 -> int64: blocks of 1024, the
//                            block sums by one workgroup, then each block again with its offset.  Also the cluster numbers of
//                            DBSCAN (a scan over the root flags, so ascending root index).
//   graph_*                  components: labels[i] = the smallest row index of i's component.  A round is hook (edge-parallel:
//                            the larger root takes the smaller by an integer atomicMin), jump (every node to its root) and decide
//                            (one thread: nothing hooked -> done).  Parents never exceed their node, so every chain ends and the
//                            fixed point is unique whatever the schedule.  The rounds are queued; after the stop each returns at
//                            its first instruction.
//   dbscan_*                 core flags from the row lengths, components over core-core edges, cluster numbers by the scan,
//                            border labels by an integer atomicMin over both directions of every edge.
//
// f32 arithmetic only: no packed FP32 (the Makefile builds this file with -fno-slp-vectorize) and -ffp-contract=off, so the one
// fused multiply-add below is the one that is spelled out.  Integer atomics only (they commute).
#include <climits>
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kRadRowsPerWave = 64;
constexpr int kRadRowsPerGroup = 256;        // four waves, four query tiles
constexpr int kRadStep = 64;                 // database rows per step
constexpr int kRadUnits = 256;               // compute units the ranges are balanced over
constexpr int kRadXcds = 8;                  // workgroups are dealt round-robin over this many L2 domains
constexpr int kScanBlock = 1024;             // elements per workgroup of the scan (256 threads x 4)
constexpr int kGraphMaxGrid = 4096;          // workgroups of the edge kernels: fixed, since the number of entries (offsets[n]) is known
                                             // on the device only; they walk the entries with a grid stride
// internal bits of the status word while a components call is queued; cleared by its last kernel
constexpr int kGraphChanged = 1 << 29, kGraphDone = 1 << 30;

// The ranges of database rows: a function of (nq, n, slices) alone (include/acx.h states it)
// slices = 0: the kernel is bound by the matrix pipe, so a call takes as long as the busiest compute unit.  With w = groups * ns
// workgroups dealt over 256 units that is ceil(w / 256) workgroups of len rows each: the ns (at most ACX_RADIUS_MAX_SLICES) with the
// smallest ceil(w / 256) * len wins, the largest such ns among equals (finer ranges even out what the model does not see).
// Measured at (20 371, 768): 7 ranges (560 workgroups, 3 per unit at worst) 9.7 ms, 16 ranges (1 280, 5 per unit) 7.0 ms.
struct RadGeom { int ns; long long len; };
static RadGeom rad_geom(long long nq, long long n, int slices) {
    const long long chunks = cdiv(n, kRadStep), groups = cdiv(nq, kRadRowsPerGroup);
    const long long most = std::min<long long>(ACX_RADIUS_MAX_SLICES, chunks);
    RadGeom g;
    if (slices > 0) {
        g.len = kRadStep * cdiv(chunks, std::min<long long>(slices, most));
    } else {
        long long best = -1;
        g.len = kRadStep * chunks;
        for (long long ns = 1; ns <= most; ++ns) {
            const long long len = kRadStep * cdiv(chunks, ns);
            const long long cost = cdiv(groups * cdiv(n, len), kRadUnits) * len;
            if (best < 0 || cost <= best) { best = cost; g.len = len; }
        }
    }
    g.ns = (int)cdiv(n, g.len);
    return g;
}

__global__ __launch_bounds__(256) void radius_rowsq_kernel(const float* __restrict__ x, long long ld, long long n, int dim,
                                                           float* __restrict__ xx) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float s = wave_sum(row_sumsq(x + row * ld, dim, lane, [](const float4&) {}));
    if (lane == 0) xx[row] = s;
}

// acx_radius_emit: the overflow bit against the new capacity; the other bits stay as the counting call left them
__global__ void radius_recheck_kernel(int* status, const long long* total, long long capacity) {
    const int st = *status & ~ACX_RADIUS_OVERFLOW;
    *status = *total > capacity ? st | ACX_RADIUS_OVERFLOW : st;
}

__global__ void nb_clear_kernel(int* status, long long* total) {
    *status = 0;
    if (total) *total = 0;
}

struct RadP {
    const float* q; long long ld_q; const float* q_aux; long long nq;
    const float* d; long long ld_d; const float* d_aux; long long n;
    int dim, metric, self_mode;
    float level;
    int ns; long long len;
    int qgroups;                  // tiles of 256 queries
    int* part;                    // [nq][ns] counts (EMIT = false)
    const long long* pos;         // [nq][ns] their exclusive scan (EMIT = true)
    int* indices; float* values; long long capacity;
    int* status;
};

template <bool EMIT>
__global__ __launch_bounds__(256, 2) void radius_tile_kernel(RadP p) {
    constexpr int QT = 2;
    __shared__ float s_c[4][kRadRowsPerWave];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    // Which (query tile, range) this workgroup takes -- a matter of speed only.  Workgroups are dealt round-robin over the 8 L2
    // domains, so id % 8 names the domain: domain k takes the query tiles k, k + 8, .. and walks all ranges of one before the next.
    // The workgroups resident in one domain then re-read the rows of a few query tiles, which fit its L2, while every range is
    // streamed once per tile.  Ids past the last tile (the grid is padded to whole rounds) have nothing to do.
    const int id = blockIdx.x, slot = id / kRadXcds;
    const int qtile = (slot / p.ns) * kRadXcds + id % kRadXcds;
    if (qtile >= p.qgroups) return;                                                  // uniform over the workgroup
    const int split = slot % p.ns;
    const long long lo = (long long)split * p.len, hi = min(p.n, lo + p.len);       // lo < hi: ns = ceil(n / len)
    const long long q0 = (long long)qtile * kRadRowsPerGroup + wave * kRadRowsPerWave;
    const bool cosine = p.metric == ACX_RADIUS_COSINE, euclid = p.metric == ACX_RADIUS_EUCLIDEAN;

    // tile rows past nq compute on the last query and are never kept
    s_c[wave][lane] = p.q_aux ? p.q_aux[min(q0 + lane, p.nq - 1)] : 0.f;
    __syncthreads();
    const float* xa[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) xa[t] = p.q + min(q0 + 32 * t + r32, p.nq - 1) * p.ld_q;

    // lane r carries tile row r: its count so far (EMIT: its next position)
    long long run = 0;
    if (EMIT && q0 + lane < p.nq) run = p.pos[(q0 + lane) * p.ns + split];
    bool bad = false;
    const unsigned below = (1u << r32) - 1u;

    for (long long j0 = lo; j0 < hi; j0 += kRadStep) {
        long long j[2];
        const float* cb[2];
        float cj[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            j[u] = j0 + 32 * u + r32;
            const long long jc = min(j[u], hi - 1);                  // past the range: its last row again, never kept
            cb[u] = p.d + jc * p.ld_d;
            cj[u] = p.d_aux ? p.d_aux[jc] : 0.f;
        }
        F32Tile<32>::acc_t acc[QT][2];
        dot_tile<QT>(acc, xa, cb, p.dim, h, [](const float4 (&)[2], const float4 (&)[2]) {});
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = 32 * t + F32Tile<32>::row(i, h);
                const long long qg = q0 + row;
                const float ci = s_c[wave][row];
                float v[2];
                bool keep[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float a = acc[t][u][i];
                    const bool valid = qg < p.nq && j[u] < hi;
                    if (valid && acx_nonfinite(a)) bad = true;
                    if (cosine) v[u] = cos_scale(a, ci, cj[u]);
                    else if (euclid) {
                        const float s = __builtin_fmaf(-2.f, a, ci + cj[u]);
                        v[u] = s < 0.f ? 0.f : s;                    // a NaN stays a NaN
                    } else v[u] = a;
                    bool k = euclid ? v[u] <= p.level : v[u] >= p.level;       // a NaN is never kept
                    if (p.self_mode && qg == j[u]) k = p.self_mode == ACX_RADIUS_SELF_INCLUDE;     // the pair (i, i), by position
                    keep[u] = k && valid;
                }
                const unsigned long long b0 = __ballot(keep[0]), b1 = __ballot(keep[1]);
                const unsigned w0 = h ? (unsigned)(b0 >> 32) : (unsigned)b0, w1 = h ? (unsigned)(b1 >> 32) : (unsigned)b1;
                if (EMIT) {
                    const long long base = __shfl(run, row);
                    if (keep[0]) {
                        const long long o = base + __popc(w0 & below);
                        if (o < p.capacity) {
                            p.indices[o] = (int)j[0];
                            if (p.values) p.values[o] = v[0];
                        }
                    }
                    if (keep[1]) {
                        const long long o = base + __popc(w0) + __popc(w1 & below);
                        if (o < p.capacity) {
                            p.indices[o] = (int)j[1];
                            if (p.values) p.values[o] = v[1];
                        }
                    }
                }
                const int row0 = 32 * t + F32Tile<32>::row(i, 0), row1 = 32 * t + F32Tile<32>::row(i, 1);
                if (lane == row0) run += __popc((unsigned)b0) + __popc((unsigned)b1);
                if (lane == row1) run += __popc((unsigned)(b0 >> 32)) + __popc((unsigned)(b1 >> 32));
            }
    }
    if (!EMIT && q0 + lane < p.nq) p.part[(q0 + lane) * p.ns + split] = (int)run;
    if (__ballot(bad) && lane == 0) atomicOr(p.status, ACX_RADIUS_NONFINITE);
}

// the padded 1-D grid of the tile kernel: whole rounds of 8 query tiles, ns ranges each
static dim3 rad_grid(long long nq, int ns) { return dim3((unsigned)(cdiv(cdiv(nq, kRadRowsPerGroup), kRadXcds) * kRadXcds * ns)); }

// counts[q] = the ranges' counts added in ascending range
__global__ __launch_bounds__(256) void radius_sum_kernel(const int* __restrict__ part, long long nq, int ns, int* __restrict__ counts) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    int c = 0;
    for (int r = 0; r < ns; ++r) c += part[q * ns + r];
    counts[q] = c;
}

// ---- the exclusive scan, int32 -> int64 ----------------------------------------------------------------------------------------
// flag != nullptr: the elements are (v[i] == i && flag[i]) -- DBSCAN's root flags -- instead of v[i]
__device__ __forceinline__ int scan_elem(const int* v, const unsigned char* flag, long long i, long long m) {
    if (i >= m) return 0;
    return flag ? (flag[i] && v[i] == (int)i ? 1 : 0) : v[i];
}

__global__ __launch_bounds__(256) void nb_scan_sums_kernel(const int* __restrict__ v, const unsigned char* __restrict__ flag, long long m,
                                                           long long* __restrict__ bsum) {
    __shared__ long long s_red[256];
    const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    long long s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += scan_elem(v, flag, base + e, m);
    s = km_block_sum<long long, 256>(s, s_red);
    if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// one workgroup: bsum -> its exclusive scan, in chunks of 256 with a carry; the grand total to *total (and to *total32)
__global__ __launch_bounds__(256) void nb_scan_top_kernel(long long* bsum, long long nb, long long* total, int* total32,
                                                          long long capacity, int* status) {
    __shared__ long long s_v[256];
    __shared__ long long s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < nb; b0 += 256) {
        const long long mine = b0 + tid < nb ? bsum[b0 + tid] : 0;
        s_v[tid] = mine;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                          // Hillis-Steele, inclusive
            const long long add = tid >= o ? s_v[tid - o] : 0;
            __syncthreads();
            s_v[tid] += add;
            __syncthreads();
        }
        const long long carry = s_carry;
        if (b0 + tid < nb) bsum[b0 + tid] = carry + s_v[tid] - mine;
        __syncthreads();
        if (tid == 255) s_carry = carry + s_v[255];
        __syncthreads();
    }
    if (tid == 0) {
        if (total) *total = s_carry;
        if (total32) *total32 = (int)s_carry;
        if (capacity >= 0 && s_carry > capacity) atomicOr(status, ACX_RADIUS_OVERFLOW);
    }
}

// out[i] = the sum of the elements before i; offsets (stride != 0): offsets[q] = out[q * stride], offsets[nq] = the total
__global__ __launch_bounds__(256) void nb_scan_apply_kernel(const int* __restrict__ v, const unsigned char* __restrict__ flag, long long m,
                                                            const long long* __restrict__ bsum, long long* __restrict__ out,
                                                            long long* __restrict__ offsets, int stride, const long long* total) {
    __shared__ long long s_v[256];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kScanBlock + tid * 4;
    int e[4];
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { e[k] = scan_elem(v, flag, base + k, m); mine += e[k]; }
    s_v[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const long long add = tid >= o ? s_v[tid - o] : 0;
        __syncthreads();
        s_v[tid] += add;
        __syncthreads();
    }
    long long at = bsum[blockIdx.x] + s_v[tid] - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = base + k;
        if (i < m) {
            out[i] = at;
            if (offsets && i % stride == 0) offsets[i / stride] = at;
        }
        at += e[k];
    }
    if (offsets && blockIdx.x == 0 && tid == 0) offsets[m / stride] = *total;
}

// v / flag (m elements) -> out (m) int64 exclusive scan; bsum: cdiv(m, kScanBlock) int64 of scratch
static void nb_launch_scan(const int* v, const unsigned char* flag, long long m, long long* bsum, long long* out, long long* offsets,
                           int stride, long long* total, int* total32, long long capacity, int* status, hipStream_t s) {
    const long long nb = cdiv(m, kScanBlock);
    launch_kernel(&nb_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, v, flag, m, bsum);
    launch_kernel(&nb_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, nb, total, total32, capacity, status);
    launch_kernel(&nb_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, v, flag, m, (const long long*)bsum, out, offsets, stride,
                  (const long long*)total);
}

// ---- components ------------------------------------------------------------------------------------------------------------------
// labels and the status word are read and written by many workgroups inside one launch: every access is an agent-scope atomic
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x: parents never exceed their node, so the chain descends and ends
__device__ __forceinline__ int g_find(const int* labels, int x) {
    for (;;) {
        const int p = g_load(labels + x);
        if (p >= x || p < 0) return x;       // p > x or p < 0: a label the caller handed in with resume (treated as a root)
        x = p;
    }
}

__global__ __launch_bounds__(256) void graph_init_kernel(int* labels, long long n, int resume, int* status, int clear_status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && clear_status) *status = 0;
    if (i < n) {
        // resume: a label outside [0, i] cannot be a parent (it would break the descent): the node starts as its own root
        if (!resume || (unsigned)labels[i] > (unsigned)i) labels[i] = (int)i;
    }
}

// the row of entry e: the last i with offsets[i] <= e
__device__ __forceinline__ long long g_row_of(const long long* __restrict__ offsets, long long n, long long e) {
    long long a = 0, b = n - 1;
    while (a < b) {
        const long long m = (a + b + 1) >> 1;
        if (offsets[m] <= e) a = m; else b = m - 1;
    }
    return a;
}

// core != nullptr: only the edges whose two ends are core rows
__global__ __launch_bounds__(256) void graph_hook_kernel(const long long* __restrict__ offsets, const int* __restrict__ indices,
                                                         long long n, const unsigned char* __restrict__ core, int* labels, int* status) {
    if (g_load(status) & kGraphDone) return;
    const long long nnz = offsets[n];
    int flags = 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
        const int j = indices[e];
        if ((unsigned)j >= (unsigned)n) { flags |= ACX_GRAPH_BAD_INDEX; continue; }
        const int i = (int)g_row_of(offsets, n, e);
        if (i == j || (core && !(core[i] && core[j]))) continue;
        const int ri = g_find(labels, i), rj = g_find(labels, j);
        if (ri != rj) {
            atomicMin(labels + max(ri, rj), min(ri, rj));
            flags |= kGraphChanged;
        }
    }
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(256) void graph_jump_kernel(int* labels, long long n, const int* status) {
    if (g_load(status) & kGraphDone) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = g_find(labels, (int)i);
    if (r != (int)i) __hip_atomic_store(labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread, after a round: nothing hooked -> done.  last: the call's final kernel -- not done: ACX_GRAPH_NOT_CONVERGED; the
// internal bits are cleared
__global__ void graph_decide_kernel(int* status, int last) {
    int st = *status;
    if (!(st & kGraphDone)) {
        if (st & kGraphChanged) st &= ~kGraphChanged;
        else st |= kGraphDone;
    }
    if (last) {
        if (!(st & kGraphDone)) st |= ACX_GRAPH_NOT_CONVERGED;
        st &= ~(kGraphDone | kGraphChanged);
    }
    *status = st;
}

// init + max_rounds rounds on `labels`; clear_status: the call owns the status word
static void graph_launch_components(const long long* offsets, const int* indices, long long n, const unsigned char* core, int* labels,
                                    int* status, int max_rounds, int resume, bool clear_status, hipStream_t s) {
    const unsigned nodes = (unsigned)cdiv(n, 256);
    launch_kernel(&graph_init_kernel, dim3(nodes), dim3(256), 0, s, labels, n, resume, status, clear_status ? 1 : 0);
    for (int r = 0; r < max_rounds; ++r) {
        launch_kernel(&graph_hook_kernel, dim3(kGraphMaxGrid), dim3(256), 0, s, offsets, indices, n, core, labels, status);
        launch_kernel(&graph_jump_kernel, dim3(nodes), dim3(256), 0, s, labels, n, (const int*)status);
        launch_kernel(&graph_decide_kernel, dim3(1), dim3(1), 0, s, status, r == max_rounds - 1 ? 1 : 0);
    }
}

// ---- DBSCAN -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dbscan_core_kernel(const long long* __restrict__ offsets, long long n, int min_samples,
                                                          unsigned char* __restrict__ core) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) core[i] = offsets[i + 1] - offsets[i] >= (long long)min_samples ? 1 : 0;
}

// a core row takes the number of its component's root; every other row starts without a cluster
__global__ __launch_bounds__(256) void dbscan_number_kernel(const int* __restrict__ comp, const unsigned char* __restrict__ core,
                                                            const long long* __restrict__ rank, long long n, int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) labels[i] = core[i] ? (int)rank[comp[i]] : INT_MAX;
}

// both directions of every edge: a row that is not core takes the smallest cluster number among its core neighbours
__global__ __launch_bounds__(256) void dbscan_border_kernel(const long long* __restrict__ offsets, const int* __restrict__ indices,
                                                            long long n, const unsigned char* __restrict__ core,
                                                            const int* __restrict__ comp, const long long* __restrict__ rank, int* labels) {
    const long long nnz = offsets[n];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
        const int j = indices[e];
        if ((unsigned)j >= (unsigned)n) continue;                    // the components kernel has set ACX_GRAPH_BAD_INDEX
        const int i = (int)g_row_of(offsets, n, e);
        if (core[j] && !core[i]) atomicMin(labels + i, (int)rank[comp[j]]);
        if (core[i] && !core[j]) atomicMin(labels + j, (int)rank[comp[i]]);
    }
}

__global__ __launch_bounds__(256) void dbscan_finish_kernel(int* labels, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && labels[i] == INT_MAX) labels[i] = -1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int rad_check_shape(const char* who, int64_t nq, int64_t n, int slices) {
    if (nq < 1 || n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: nq = %lld, n = %lld (expected >= 1)", who, (long long)nq, (long long)n);
    if (nq > kF32MaxRows || n > kF32MaxRows)
        ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: nq = %lld, n = %lld (at most 2^30 rows)", who, (long long)nq, (long long)n);
    if (slices < 0 || slices > ACX_RADIUS_MAX_SLICES)
        ACX_FAIL(ACX_ERR_ARG, "%s: slices = %d (expected 0 .. %d)", who, slices, ACX_RADIUS_MAX_SLICES);
    return ACX_OK;
}

// The workspace, carved in this order (each piece 256-byte aligned)
struct RadWs { size_t part, pos, bsum, end; };
static RadWs rad_carve(long long nq, long long n, int slices) {
    const RadGeom g = rad_geom(nq, n, slices);
    const size_t m = (size_t)nq * g.ns;
    RadWs w;
    size_t off = 0;
    w.part = off; off += align_up(m * sizeof(int));
    w.pos = off; off += align_up(m * sizeof(long long));
    w.bsum = off; off += align_up((size_t)cdiv((long long)m, kScanBlock) * sizeof(long long));
    w.end = off;
    return w;
}

struct DbWs { size_t comp, rank, bsum, end; };
static DbWs db_carve(long long n) {
    DbWs w;
    size_t off = 0;
    w.comp = off; off += align_up((size_t)n * sizeof(int));
    w.rank = off; off += align_up((size_t)n * sizeof(long long));
    w.bsum = off; off += align_up((size_t)cdiv(n, kScanBlock) * sizeof(long long));
    w.end = off;
    return w;
}

static int rad_check_args(const char* who, const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d,
                          const float* d_aux, int64_t n, int dim, int metric, float level, int self_mode, int slices,
                          const int32_t* status, const void* ws, size_t ws_bytes) {
    ACX_TRY(rad_check_shape(who, nq, n, slices));
    if (metric != ACX_RADIUS_DOT && metric != ACX_RADIUS_COSINE && metric != ACX_RADIUS_EUCLIDEAN)
        ACX_FAIL(ACX_ERR_ARG, "%s: metric %d (expected ACX_RADIUS_DOT, ACX_RADIUS_COSINE or ACX_RADIUS_EUCLIDEAN)", who, metric);
    ACX_TRY(check_f32_rows(who, "q", q, ld_q, dim));
    ACX_TRY(check_f32_rows(who, "d", d, ld_d, dim));
    if (metric != ACX_RADIUS_DOT && (!q_aux || !d_aux))
        ACX_FAIL(ACX_ERR_ARG, "%s: q_aux / d_aux is null with ACX_RADIUS_COSINE or ACX_RADIUS_EUCLIDEAN", who);
    if (level != level) ACX_FAIL(ACX_ERR_ARG, "%s: level is NaN", who);
    if (self_mode != ACX_RADIUS_SELF_NONE && self_mode != ACX_RADIUS_SELF_EXCLUDE && self_mode != ACX_RADIUS_SELF_INCLUDE)
        ACX_FAIL(ACX_ERR_ARG, "%s: self_mode %d (expected an acx_radius_self)", who, self_mode);
    if (self_mode != ACX_RADIUS_SELF_NONE && nq != n)
        ACX_FAIL(ACX_ERR_ARG, "%s: a self-join needs nq == n, got %lld and %lld", who, (long long)nq, (long long)n);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    return check_workspace_for(who, ws, ws_bytes, rad_carve(nq, n, slices).end);
}

static RadP rad_params(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d, const float* d_aux,
                       int64_t n, int dim, int metric, float level, int self_mode, const RadGeom& g, int32_t* status) {
    RadP p;
    const bool aux = metric != ACX_RADIUS_DOT;
    p.q = q; p.ld_q = ld_q; p.q_aux = aux ? q_aux : nullptr; p.nq = nq;
    p.d = d; p.ld_d = ld_d; p.d_aux = aux ? d_aux : nullptr; p.n = n;
    p.dim = dim; p.metric = metric; p.self_mode = self_mode; p.level = level;
    p.ns = g.ns; p.len = g.len; p.qgroups = (int)cdiv(nq, kRadRowsPerGroup);
    p.part = nullptr; p.pos = nullptr; p.indices = nullptr; p.values = nullptr; p.capacity = 0;
    p.status = (int*)status;
    return p;
}

static int graph_check_args(const char* who, const int64_t* offsets, const int32_t* indices, int64_t n, const int32_t* labels,
                            const int32_t* status, int max_rounds) {
    if (!offsets || !indices) ACX_FAIL(ACX_ERR_ARG, "%s: offsets / indices is null", who);
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    if (reinterpret_cast<uintptr_t>(offsets) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: offsets is not 8-byte aligned", who);
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (max_rounds < 1 || max_rounds > ACX_GRAPH_MAX_ROUNDS)
        ACX_FAIL(ACX_ERR_ARG, "%s: max_rounds = %d (expected 1 .. %d)", who, max_rounds, ACX_GRAPH_MAX_ROUNDS);
    return ACX_OK;
}

// acx_radius_neighbors (count, scan, emit) and acx_radius_emit (the emit pass alone, on the workspace such a call left)
static int rad_run_neighbors(const char* who, bool count, const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d,
                             int64_t ld_d, const float* d_aux, int64_t n, int dim, int metric, float level, int self_mode, int slices,
                             int64_t* offsets, int32_t* indices, float* values, int64_t capacity, int64_t* total, int32_t* status,
                             void* ws, size_t ws_bytes, void* stream) {
    if (!offsets || !total) ACX_FAIL(ACX_ERR_ARG, "%s: offsets / total is null", who);
    if (capacity < 0) ACX_FAIL(ACX_ERR_ARG, "%s: capacity = %lld (expected >= 0)", who, (long long)capacity);
    if (capacity > 0 && !indices) ACX_FAIL(ACX_ERR_ARG, "%s: indices is null with capacity %lld", who, (long long)capacity);
    if ((reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(total)) & 7)
        ACX_FAIL(ACX_ERR_ARG, "%s: offsets / total is not 8-byte aligned", who);
    ACX_TRY(rad_check_args(who, q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, slices, status, ws, ws_bytes));
    hipStream_t st = (hipStream_t)stream;
    const RadGeom g = rad_geom(nq, n, slices);
    const RadWs w = rad_carve(nq, n, slices);
    char* base = static_cast<char*>(ws);
    RadP p = rad_params(q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, g, status);
    p.part = reinterpret_cast<int*>(base + w.part);
    long long* pos = reinterpret_cast<long long*>(base + w.pos);
    const dim3 grid = rad_grid(nq, g.ns);
    if (count) {
        launch_kernel(&nb_clear_kernel, dim3(1), dim3(1), 0, st, (int*)status, (long long*)total);
        launch_kernel(&radius_tile_kernel<false>, grid, dim3(256), 0, st, p);
        nb_launch_scan(p.part, nullptr, (long long)nq * g.ns, reinterpret_cast<long long*>(base + w.bsum), pos, (long long*)offsets, g.ns,
                       (long long*)total, nullptr, (long long)capacity, (int*)status, st);
    } else {
        launch_kernel(&radius_recheck_kernel, dim3(1), dim3(1), 0, st, (int*)status, (const long long*)total, (long long)capacity);
    }
    if (capacity > 0) {
        p.pos = pos; p.indices = (int*)indices; p.values = values; p.capacity = capacity;
        launch_kernel(&radius_tile_kernel<true>, grid, dim3(256), 0, st, p);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_radius_workspace_bytes(int64_t nq, int64_t n, int slices, size_t* out_bytes) {
    static const char* who = "acx_radius_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(rad_check_shape(who, nq, n, slices));
    *out_bytes = rad_carve(nq, n, slices).end;
    return ACX_OK;
}

int acx_radius_slices(int64_t nq, int64_t n, int slices, int* out_slices) {
    static const char* who = "acx_radius_slices";
    if (!out_slices) ACX_FAIL(ACX_ERR_ARG, "%s: out_slices is null", who);
    ACX_TRY(rad_check_shape(who, nq, n, slices));
    *out_slices = rad_geom(nq, n, slices).ns;
    return ACX_OK;
}

int acx_radius_row_sumsq(const float* x, int64_t ld, int64_t n, int dim, float* xx, void* stream) {
    static const char* who = "acx_radius_row_sumsq";
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    ACX_TRY(check_f32_rows(who, "x", x, ld, dim));
    if (!xx) ACX_FAIL(ACX_ERR_ARG, "%s: xx is null", who);
    launch_kernel(&radius_rowsq_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, x, (long long)ld, (long long)n,
                  dim, xx);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_radius_count(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d, const float* d_aux,
                     int64_t n, int dim, int metric, float level, int self_mode, int32_t* counts, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
    static const char* who = "acx_radius_count";
    if (!counts) ACX_FAIL(ACX_ERR_ARG, "%s: counts is null", who);
    ACX_TRY(rad_check_args(who, q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, 0, status, ws, ws_bytes));
    hipStream_t st = (hipStream_t)stream;
    const RadGeom g = rad_geom(nq, n, 0);
    const RadWs w = rad_carve(nq, n, 0);
    RadP p = rad_params(q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, g, status);
    p.part = reinterpret_cast<int*>(static_cast<char*>(ws) + w.part);
    launch_kernel(&nb_clear_kernel, dim3(1), dim3(1), 0, st, (int*)status, (long long*)nullptr);
    launch_kernel(&radius_tile_kernel<false>, rad_grid(nq, g.ns), dim3(256), 0, st, p);
    launch_kernel(&radius_sum_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, st, (const int*)p.part, (long long)nq, g.ns,
                  (int*)counts);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_radius_neighbors(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d,
                         const float* d_aux, int64_t n, int dim, int metric, float level, int self_mode, int slices,
                         int64_t* offsets, int32_t* indices, float* values, int64_t capacity, int64_t* total, int32_t* status,
                         void* ws, size_t ws_bytes, void* stream) {
    return rad_run_neighbors("acx_radius_neighbors", true, q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, slices,
                             offsets, indices, values, capacity, total, status, ws, ws_bytes, stream);
}

int acx_radius_emit(const float* q, int64_t ld_q, const float* q_aux, int64_t nq, const float* d, int64_t ld_d, const float* d_aux,
                    int64_t n, int dim, int metric, float level, int self_mode, int slices, const int64_t* offsets, int32_t* indices,
                    float* values, int64_t capacity, const int64_t* total, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    return rad_run_neighbors("acx_radius_emit", false, q, ld_q, q_aux, nq, d, ld_d, d_aux, n, dim, metric, level, self_mode, slices,
                             const_cast<int64_t*>(offsets), indices, values, capacity, const_cast<int64_t*>(total), status, ws, ws_bytes,
                             stream);
}

int acx_graph_components(const int64_t* offsets, const int32_t* indices, int64_t n, int32_t* labels, int32_t* status, int max_rounds,
                         int resume, void* stream) {
    static const char* who = "acx_graph_components";
    ACX_TRY(graph_check_args(who, offsets, indices, n, labels, status, max_rounds));
    graph_launch_components((const long long*)offsets, (const int*)indices, n, nullptr, (int*)labels, (int*)status, max_rounds,
                            resume ? 1 : 0, true, (hipStream_t)stream);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_dbscan_workspace_bytes(int64_t n, size_t* out_bytes) {
    static const char* who = "acx_dbscan_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (n > kF32MaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30 rows)", who, (long long)n);
    *out_bytes = db_carve(n).end;
    return ACX_OK;
}

int acx_dbscan_labels(const int64_t* offsets, const int32_t* indices, int64_t n, int min_samples, int32_t* labels, uint8_t* core,
                      int32_t* clusters, int32_t* status, void* ws, size_t ws_bytes, int max_rounds, void* stream) {
    static const char* who = "acx_dbscan_labels";
    ACX_TRY(graph_check_args(who, offsets, indices, n, labels, status, max_rounds));
    if (min_samples < 1) ACX_FAIL(ACX_ERR_ARG, "%s: min_samples = %d (expected >= 1)", who, min_samples);
    if (!core || !clusters) ACX_FAIL(ACX_ERR_ARG, "%s: core / clusters is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const DbWs w = db_carve(n);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, w.end));
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    int* comp = reinterpret_cast<int*>(base + w.comp);
    long long* rank = reinterpret_cast<long long*>(base + w.rank);
    const unsigned nodes = (unsigned)cdiv(n, 256);
    const long long* off = (const long long*)offsets;
    launch_kernel(&dbscan_core_kernel, dim3(nodes), dim3(256), 0, st, off, (long long)n, min_samples, (unsigned char*)core);
    graph_launch_components(off, (const int*)indices, n, (const unsigned char*)core, comp, (int*)status, max_rounds, 0, true, st);
    nb_launch_scan(comp, (const unsigned char*)core, n, reinterpret_cast<long long*>(base + w.bsum), rank, nullptr, 0, nullptr,
                   (int*)clusters, -1, (int*)status, st);
    launch_kernel(&dbscan_number_kernel, dim3(nodes), dim3(256), 0, st, (const int*)comp, (const unsigned char*)core,
                  (const long long*)rank, (long long)n, (int*)labels);
    launch_kernel(&dbscan_border_kernel, dim3(kGraphMaxGrid), dim3(256), 0, st, off, (const int*)indices, (long long)n,
                  (const unsigned char*)core, (const int*)comp, (const long long*)rank, (int*)labels);
    launch_kernel(&dbscan_finish_kernel, dim3(nodes), dim3(256), 0, st, (int*)labels, (long long)n);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
