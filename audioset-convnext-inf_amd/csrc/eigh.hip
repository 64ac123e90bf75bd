// Embedding statistics, part 2: acx_eigh (include/acx.h, which states the algorithm) -- the symmetric eigenproblem in float64 by
// cyclic Jacobi with the round-robin ordering, one launch per round.
//
//   eigh_init_kernel        the upper triangle of `a`, mirrored, into copy 0 of the matrix (P x P, P = dim rounded up to the 32 x 32
//                           tile, zero padding); the identity into copy 0 of the vectors; max |a_ii| and the NaN / Inf flag.
//   eigh_thr_kernel         threshold = 2^-53 max |a_ii|; a non-finite input sets state->done, so no round runs.
//   eigh_round_kernel       one round: reads copy `src`, writes copy 1 - src.  A workgroup owns one 32 x 32 tile -- an upper
//                           triangle tile of the matrix (written with its mirror image through LDS) or a tile of the vectors --
//                           and recomputes the rotations of its 32 rows and 32 columns from the OLD diagonal and pivot elements:
//                           no workgroup waits on another, there is no grid barrier and no cooperative launch.  The workgroups of
//                           the first tile row count the applied rotations of their columns (a pair at its lower index).
//   eigh_final_kernel       reads state: which copy is current, the order of the eigenvalues, the signs; NOT_CONVERGED.
//
// The vectors are kept TRANSPOSED (row j = the j-th accumulated vector), so a round's update Vt <- J^T Vt combines rows.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kEgTile = 32;

struct EgWs { size_t a[2], v[2], count, thr, info, end; int P; };
static EgWs eg_carve(int dim) {
    EgWs w;
    w.P = (dim + kEgTile - 1) / kEgTile * kEgTile;
    const size_t mat = align_up((size_t)w.P * w.P * sizeof(double));
    size_t off = 0;
    for (int i = 0; i < 2; ++i) { w.a[i] = off; off += mat; }
    for (int i = 0; i < 2; ++i) { w.v[i] = off; off += mat; }
    w.count = off; off += align_up((size_t)ACX_EIGH_MAX_SWEEPS * sizeof(int));
    w.thr = off; off += align_up(sizeof(double));
    w.info = off; off += align_up(4 * sizeof(unsigned long long));         // [0] bits of max |a_ii|, [1] non-finite flag, [2] rounds run
    w.end = off;
    return w;
}

__device__ __forceinline__ bool eg_nonfinite(double v) { return !(fabs(v) <= 1.7976931348623157e308); }

__global__ __launch_bounds__(256) void eigh_init_kernel(const double* __restrict__ a, long long ld_a, int dim, int P,
                                                        double* __restrict__ A0, double* __restrict__ V0,
                                                        unsigned long long* info) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (e < (long long)P * P) {
        const int i = (int)(e / P), j = (int)(e % P);
        double v = 0.0;
        if (i < dim && j < dim) {
            v = i <= j ? a[i * ld_a + j] : a[j * ld_a + i];
            bad = eg_nonfinite(v);
            // bit patterns of non-negative doubles order as the doubles; a NaN diagonal is caught by `bad`
            if (i == j && !bad) atomicMax(info, (unsigned long long)__double_as_longlong(fabs(v)));
        }
        A0[e] = v;
        V0[e] = i == j ? 1.0 : 0.0;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(info + 1, 1ull);
}

__global__ void eigh_thr_kernel(const unsigned long long* info, double* thr, acx_eigh_state* st, int* status) {
    *thr = ldexp(__longlong_as_double((long long)info[0]), -53);
    if (info[1]) {
        st->done = 1;
        atomicOr(status, ACX_STATS_NONFINITE);
    }
}

// the partner of index i in round r of a sweep over m (even) indices
__device__ __forceinline__ int eg_partner(int i, int r, int m) {
    if (i == m - 1) return r;
    if (i == r) return m - 1;
    const int q = m - 1;
    return ((2 * r - i) % q + q) % q;
}

struct EgRot { double c, g, delta; int partner, on; };
// The rotation of index i's pair from the old matrix A (P x P): c, g = the partner's weight in column i of J (-s at the pair's lower
// index, +s at the upper), delta = the change of a_ii, on = rotated.  An index without a pair: the identity, partner = i.
__device__ __forceinline__ EgRot eg_rotation(const double* __restrict__ A, int P, int dim, int m, int r, int i, double thr) {
    EgRot o;
    o.c = 1.0; o.g = 0.0; o.delta = 0.0; o.partner = i; o.on = 0;
    if (i >= dim) return o;
    const int p = eg_partner(i, r, m);
    if (p >= dim) return o;
    o.partner = p;
    const int lo = min(i, p), hi = max(i, p);
    const double apq = A[(long long)lo * P + hi];
    if (!(fabs(apq) > thr)) return o;
    const double app = A[(long long)lo * P + lo], aqq = A[(long long)hi * P + hi];
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    o.c = c;
    o.g = i == lo ? -s : s;
    o.delta = i == lo ? -(t * apq) : t * apq;
    o.on = 1;
    return o;
}

__global__ __launch_bounds__(256) void eigh_round_kernel(const double* __restrict__ A, double* __restrict__ An,
                                                         const double* __restrict__ V, double* __restrict__ Vn, int P, int dim, int m,
                                                         int sweep, int r, int ntri, const double* thr_p, int* count,
                                                         acx_eigh_state* st, unsigned long long* info) {
    __shared__ double s_c[64], s_g[64], s_d[64];
    __shared__ int s_p[64], s_on[64];
    __shared__ double s_t[kEgTile][kEgTile + 1];
    if (st->done) return;
    if (r == 0 && sweep > 0 && count[sweep - 1] == 0) {              // the sweep before applied nothing: converged
        if (blockIdx.x == 0 && threadIdx.x == 0) st->done = 1;
        return;
    }
    const int tid = threadIdx.x;
    const int T = P / kEgTile;
    const bool vec = (int)blockIdx.x >= ntri;
    int ti, tj;
    if (vec) { ti = (blockIdx.x - ntri) / T; tj = (blockIdx.x - ntri) % T; }
    else {
        int a = 0, p = blockIdx.x;
        while (p >= T - a) { p -= T - a; ++a; }
        ti = a; tj = a + p;
    }
    if (blockIdx.x == 0 && tid == 0) {
        info[2] = (unsigned long long)sweep * (m - 1) + r + 1;       // rounds run so far: which copy is current
        if (r == 0) st->sweeps = sweep + 1;
    }
    const double thr = *thr_p;
    if (tid < 64) {
        const int i = (tid < 32 ? ti : tj) * kEgTile + (tid & 31);
        const EgRot o = eg_rotation(A, P, dim, m, r, i, thr);
        s_c[tid] = o.c; s_g[tid] = o.g; s_d[tid] = o.delta; s_p[tid] = o.partner; s_on[tid] = o.on;
    }
    __syncthreads();
    const int lx = tid & 31, ly0 = tid >> 5;
    if (vec) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ly = ly0 + 8 * q;
            const int j = ti * kEgTile + ly, k = tj * kEgTile + lx;
            Vn[(long long)j * P + k] = s_c[ly] * V[(long long)j * P + k] + s_g[ly] * V[(long long)s_p[ly] * P + k];
        }
        return;
    }
    if (ti == 0 && tid >= 32 && tid < 64) {                          // tiles (0, tj): their columns run over every index once
        const int j = tj * kEgTile + (tid & 31);
        const int applied = __popcll(__ballot(s_on[tid] && j < s_p[tid]));
        if (tid == 32 && applied) {
            atomicAdd(count + sweep, applied);
            atomicAdd((unsigned long long*)&st->rotations, (unsigned long long)applied);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ly = ly0 + 8 * q;
        const int i = ti * kEgTile + ly, j = tj * kEgTile + lx;
        if (ti < tj || ly <= lx) {
            const int pi = s_p[ly], pj = s_p[32 + lx];
            double v;
            if (i == j) v = A[(long long)i * P + i] + s_d[ly];
            else if (j == pi && s_on[ly]) v = 0.0;
            else {
                const double ci = s_c[ly], gi = s_g[ly], cj = s_c[32 + lx], gj = s_g[32 + lx];
                const double u0 = ci * A[(long long)i * P + j] + gi * A[(long long)pi * P + j];
                const double u1 = ci * A[(long long)i * P + pj] + gi * A[(long long)pi * P + pj];
                v = cj * u0 + gj * u1;
            }
            s_t[ly][lx] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ly = ly0 + 8 * q;
        if (ti < tj) {
            An[(long long)(ti * kEgTile + ly) * P + tj * kEgTile + lx] = s_t[ly][lx];
            An[(long long)(tj * kEgTile + ly) * P + ti * kEgTile + lx] = s_t[lx][ly];
        } else {
            An[(long long)(ti * kEgTile + ly) * P + tj * kEgTile + lx] = ly <= lx ? s_t[ly][lx] : s_t[lx][ly];
        }
    }
}

// One workgroup per original column j: its rank in (value descending, index ascending), its sign, its row of `vectors`.
__global__ __launch_bounds__(256) void eigh_final_kernel(const double* __restrict__ ws_a0, const double* __restrict__ ws_a1,
                                                         const double* __restrict__ ws_v0, const double* __restrict__ ws_v1, int P,
                                                         int dim, const int* __restrict__ count, int max_sweeps,
                                                         const unsigned long long* info, double* __restrict__ values,
                                                         double* __restrict__ vectors, long long ld_v, int* status) {
    __shared__ int s_cnt[256];
    __shared__ double s_abs[256];
    __shared__ int s_idx[256];
    const int tid = threadIdx.x, j = blockIdx.x;
    const bool odd = info[2] & 1ull;
    const double* A = odd ? ws_a1 : ws_a0;
    const double* V = odd ? ws_v1 : ws_v0;
    if (j == 0 && tid == 0 && count[max_sweeps - 1] != 0) atomicOr(status, ACX_STATS_NOT_CONVERGED);
    const double lam = A[(long long)j * P + j];
    int c = 0;
    for (int l = tid; l < dim; l += 256) {
        const double o = A[(long long)l * P + l];
        c += (o > lam || (o == lam && l < j)) ? 1 : 0;
    }
    double best = -1.0;
    int bi = 0x7fffffff;
    for (int k = tid; k < dim; k += 256) {
        const double a = fabs(V[(long long)j * P + k]);
        if (a > best) { best = a; bi = k; }                          // ascending k: the lowest index of equal magnitudes stays
    }
    s_cnt[tid] = c; s_abs[tid] = best; s_idx[tid] = bi;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) {
            s_cnt[tid] += s_cnt[tid + o];
            const double a = s_abs[tid + o];
            const int b = s_idx[tid + o];
            if (a > s_abs[tid] || (a == s_abs[tid] && b < s_idx[tid])) { s_abs[tid] = a; s_idx[tid] = b; }
        }
        __syncthreads();
    }
    const int rank = min(s_cnt[0], dim - 1);                         // (NaN values compare false everywhere: stay in bounds)
    const int top = min(s_idx[0], dim - 1);
    const bool flip = V[(long long)j * P + top] < 0.0;
    if (tid == 0) values[rank] = lam;
    for (int k = tid; k < dim; k += 256) {
        const double v = V[(long long)j * P + k];
        vectors[rank * ld_v + k] = flip ? -v : v;
    }
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_eigh_workspace_bytes(int dim, size_t* out_bytes) {
    static const char* who = "acx_eigh_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    if (dim < 1 || dim > ACX_STATS_MAX_DIM) ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected 1 .. %d)", who, dim, ACX_STATS_MAX_DIM);
    *out_bytes = eg_carve(dim).end;
    return ACX_OK;
}

int acx_eigh(const double* a, int64_t ld_a, int dim, int max_sweeps, double* values, double* vectors, int64_t ld_v,
             acx_eigh_state* state, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    static const char* who = "acx_eigh";
    if (dim < 1 || dim > ACX_STATS_MAX_DIM) ACX_FAIL(ACX_ERR_ARG, "%s: dim = %d (expected 1 .. %d)", who, dim, ACX_STATS_MAX_DIM);
    if (max_sweeps < 1 || max_sweeps > ACX_EIGH_MAX_SWEEPS)
        ACX_FAIL(ACX_ERR_ARG, "%s: max_sweeps = %d (expected 1 .. %d)", who, max_sweeps, ACX_EIGH_MAX_SWEEPS);
    if (!a || !values || !vectors) ACX_FAIL(ACX_ERR_ARG, "%s: a / values / vectors is null", who);
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(vectors)) & 7)
        ACX_FAIL(ACX_ERR_ARG, "%s: a / values / vectors is not 8-byte aligned", who);
    if (ld_a < dim || ld_v < dim) ACX_FAIL(ACX_ERR_ARG, "%s: ld_a = %lld / ld_v = %lld under dim = %d", who, (long long)ld_a, (long long)ld_v, dim);
    if (!state) ACX_FAIL(ACX_ERR_ARG, "%s: state is null", who);
    if (reinterpret_cast<uintptr_t>(state) & 7) ACX_FAIL(ACX_ERR_ARG, "%s: state is not 8-byte aligned", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ws) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    const EgWs w = eg_carve(dim);
    ACX_TRY(check_workspace_for(who, ws, ws_bytes, w.end));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    double* A[2] = {reinterpret_cast<double*>(base + w.a[0]), reinterpret_cast<double*>(base + w.a[1])};
    double* V[2] = {reinterpret_cast<double*>(base + w.v[0]), reinterpret_cast<double*>(base + w.v[1])};
    int* count = reinterpret_cast<int*>(base + w.count);
    double* thr = reinterpret_cast<double*>(base + w.thr);
    unsigned long long* info = reinterpret_cast<unsigned long long*>(base + w.info);
    const int P = w.P, T = P / kEgTile, ntri = T * (T + 1) / 2;
    const int m = (dim + 1) & ~1;
    ACX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    ACX_HIP(hipMemsetAsync(state, 0, sizeof(acx_eigh_state), s));
    ACX_HIP(hipMemsetAsync(base + w.count, 0, w.end - w.count, s));
    launch_kernel(&eigh_init_kernel, dim3((unsigned)cdiv((long long)P * P, 256)), dim3(256), 0, s, a, (long long)ld_a, dim, P, A[0], V[0], info);
    launch_kernel(&eigh_thr_kernel, dim3(1), dim3(1), 0, s, (const unsigned long long*)info, thr, state, (int*)status);
    int src = 0;
    for (int sw = 0; sw < max_sweeps; ++sw)
        for (int r = 0; r < m - 1; ++r) {
            launch_kernel(&eigh_round_kernel, dim3(ntri + T * T), dim3(256), 0, s, (const double*)A[src], A[1 - src], (const double*)V[src],
                          V[1 - src], P, dim, m, sw, r, ntri, (const double*)thr, count, state, info);
            src = 1 - src;
        }
    launch_kernel(&eigh_final_kernel, dim3(dim), dim3(256), 0, s, (const double*)A[0], (const double*)A[1], (const double*)V[0],
                  (const double*)V[1], P, dim, (const int*)count, max_sweeps, (const unsigned long long*)info, values, vectors,
                  (long long)ld_v, (int*)status);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
