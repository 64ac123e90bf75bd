// Calibration of probabilities (include/acx.h, "calibration"): reliability counts behind ECE / MCE / Brier, per-class Platt
// scaling and temperature scaling, fitted and applied on the device.  float64 wherever a sum runs over rows; every float sum has
// ONE order that depends on the shape alone, so a call repeated gives the same bits (no float atomics anywhere).
//
//   reliability_counts_kernel   one wave per class, 16 classes per workgroup.  The wave walks its column 64 rows at a time (lane l
//                               loads row r0 + l), then hands the 64 values round in ascending row order (v_readlane): lane b IS
//                               bin b and adds what falls into it.  count / positive / conf_sum of a (class, bin) are therefore
//                               plain sequential sums over ascending rows; brier_sum is the lanes' partials by the xor butterfly.
//   toplabel_row_kernel         one group per row (device_common.h, "softmax of one row").  The scaled row (float)beta * z is
//                               staged in LDS -- thread t writes and reads elements t, t + W, ... only, so no barrier is needed --
//                               and soft_row_stats / soft_prob run on it: the bits of acx_softmax_topk on the scaled logits;
//                               the row's loss log s + (m - z_y) is evaluated in float64 (its own sum of exp).  Per row a 16-byte record {confidence, bin and hit, nll} goes to the workspace.
//   toplabel_reduce_kernel      one workgroup: wave w takes the w-th run of rows and bins them as above; the 16 waves' partials
//                               are added in wave order.
//   platt_prep_kernel           logits / targets (n, C) -> columns z[c][i], y[c][i] of the workspace through a 64 x 64 LDS tile.
//   platt_fit_kernel            one workgroup of 512 per class; thread t owns rows t, t + 512, ...  n <= 32 768: the column in
//                               LDS (own elements only) and the labels as one bit mask per thread; beyond: both streamed from the
//                               workspace.  Newton with backtracking, the whole iteration in the kernel: each evaluation is six
//                               float64 sums (thread partials in ascending row order, xor butterfly, 8 waves in wave order);
//                               every thread holds the same bits and takes the same branches.
//   platt_apply_kernel          p = head_sigmoid(fmaf((float)a_c, z, (float)b_c)).
//   temperature_eval_kernel     one evaluation (F, F', F'') at the state's trial beta: a group of W threads per run of rows,
//                               float64 partials per group to the workspace; the LAST workgroup (integer ticket) adds them in
//                               index order and takes the accept / halve / stop decision in device memory.  The partials cross
//                               workgroups as agent-scope atomic stores / loads with fences on both sides of the ticket.
//   temperature_apply_kernel    out = (float)beta * z.
// Built with -ffp-contract=off (a z + b and (float)beta * z are rounded as the host definitions round them) and
// -fno-slp-vectorize.
#include <cmath>

#include "acx_internal.h"
#include "device_common.h"

namespace acx {

constexpr int kCalThreads = 1024;
constexpr int kCalWaves = kCalThreads / 64;
constexpr int kPlattThreads = 512;               // float64 exp / log1p and six sums: more than the 128 registers of a 1024-thread workgroup
constexpr int kPlattWaves = kPlattThreads / 64;
constexpr int kCalLdsRows = 32768;                // platt: columns up to this many rows live in LDS (128 KiB)
constexpr long long kCalMaxRows = 1LL << 30;
constexpr int kCalTile = 64;
constexpr int kRowThreads = 256;
constexpr size_t kTempStateBytes = 256;
// "F does not increase" is judged up to this fraction of max(1, |F|): near the minimiser a Newton step changes F by less than
// the rounding of its float64 sum, and a comparison of two roundings would halve good steps for ever
constexpr double kCalFSlack = 0x1p-40;

extern __shared__ __attribute__((aligned(16))) float cal_dyn[];

__device__ __forceinline__ bool cal_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ int cal_bin(float p, int bins) {
    const int b = (int)(p * (float)bins);
    return b < bins - 1 ? b : bins - 1;
}
__device__ __forceinline__ float lane_float(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ double lane_double(double v, int j) {
    const long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- reliability of (n, C) probabilities ------------------------------------------------------------------------------------
struct RelCountsP {
    const float* probs; long long ld; const void* target; int u8; long long ld_t; int n; int C; int bins;
    long long* count; long long* positive; double* conf_sum; double* brier_sum; int* status;
};

__global__ __launch_bounds__(kCalThreads) void reliability_counts_kernel(RelCountsP p) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * kCalWaves + (threadIdx.x >> 6);
    if (c >= p.C) return;                                          // a whole wave; the kernel has no barrier
    int cnt = 0, pos = 0, flags = 0;
    double conf = 0.0, brier = 0.0;
    for (int r0 = 0; r0 < p.n; r0 += 64) {
        const int r = r0 + lane;
        float v = 0.f;
        int y = 0, b = -1;
        if (r < p.n) {
            v = p.probs[(long long)r * p.ld + c];
            bool tbad;
            if (p.u8) {
                const unsigned char t = static_cast<const unsigned char*>(p.target)[(long long)r * p.ld_t + c];
                tbad = t > 1;
                y = t != 0;
            } else {
                const float t = static_cast<const float*>(p.target)[(long long)r * p.ld_t + c];
                tbad = !(t == 0.0f || t == 1.0f);
                y = t == 1.0f;
            }
            const bool nf = cal_nonfinite(v);
            const bool pbad = !nf && !(v >= 0.0f && v <= 1.0f);
            flags |= (nf ? ACX_CAL_NONFINITE : 0) | (pbad ? ACX_CAL_BAD_PROBABILITY : 0) | (tbad ? ACX_CAL_BAD_TARGET : 0);
            if (!nf && !pbad && !tbad) b = cal_bin(v, p.bins);
        }
        const int m = min(64, p.n - r0);
        for (int j = 0; j < m; ++j) {                              // ascending rows; j is uniform
            const int bj = __builtin_amdgcn_readlane(b, j);
            const int yj = __builtin_amdgcn_readlane(y, j);
            const double pj = (double)lane_float(v, j);
            if (lane == bj) {
                ++cnt;
                pos += yj;
                conf += pj;
                const double d = pj - (double)yj;
                brier += d * d;
            }
        }
    }
    if (lane < p.bins) {
        const long long o = (long long)c * p.bins + lane;
        p.count[o] = cnt;
        p.positive[o] = pos;
        p.conf_sum[o] = conf;
    }
    brier = wave_sum(brier);
    if (lane == 0) p.brier_sum[c] = brier;
    if (__ballot(flags != 0)) {
        const int bits = (__ballot(flags & ACX_CAL_NONFINITE) ? ACX_CAL_NONFINITE : 0) |
                         (__ballot(flags & ACX_CAL_BAD_PROBABILITY) ? ACX_CAL_BAD_PROBABILITY : 0) |
                         (__ballot(flags & ACX_CAL_BAD_TARGET) ? ACX_CAL_BAD_TARGET : 0);
        if (lane == 0) atomicOr(p.status, bits);
    }
}

// ---- top-label reliability of (n, N) logits ----------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ knn_key cal_group_max_key(knn_key v, knn_key* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const knn_key w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    if (W == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        const knn_key a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        v = a > b ? a : b;
    }
    return v;
}

// a float64 sum over a group of W threads (device_common.h, "softmax of one row"): lanes by the xor butterfly, waves in order
template <int W>
__device__ __forceinline__ double cal_group_sum(double v, double* red) {
    v = wave_sum(v);
    if (W == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = ((red[0] + red[1]) + red[2]) + red[3];
    }
    return v;
}

struct TopRec { float conf; int code; double nll; };              // code: -1 = not counted, else bin | hit << 8

struct TopRowP {
    const float* z; long long ld; const long long* labels; long long n; int N; const double* beta; int bins;
    TopRec* rec; int* status;
};

template <int W>
__global__ __launch_bounds__(kRowThreads) void toplabel_row_kernel(TopRowP p) {
    __shared__ float red[4];
    __shared__ double redd[4];
    __shared__ knn_key redk[4];
    const int t = soft_thread<W>();
    const long long row = W == 64 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
    if (row >= p.n) return;                                        // W = 64 only: a whole wave, which meets no barrier
    const float bf = p.beta ? (float)*p.beta : 1.0f;
    const float* z = p.z + row * p.ld;
    float* zs = cal_dyn + (W == 64 ? (size_t)(threadIdx.x >> 6) * p.N : 0);
    bool bad = false;
    knn_key best = 0ull;
    for (int c = t; c < p.N; c += W) {                             // thread t touches zs[t + k W] only, here and below
        const float v = bf * z[c];
        zs[c] = v;
        bad |= acx_nonfinite(v);
        const knn_key key = knn_make_key(v, c);
        best = key > best ? key : best;
    }
    bad = group_any<W>(bad);
    const long long y = p.labels[row];
    const bool ybad = y < 0 || y >= p.N;
    if (bad || ybad) {                                             // uniform over the group
        if (t == 0) {
            atomicOr(p.status, (bad ? ACX_CAL_NONFINITE : 0) | (ybad ? ACX_CAL_BAD_LABEL : 0));
            p.rec[row] = TopRec{0.f, -1, 0.0};
        }
        return;
    }
    float m, s;
    soft_row_stats<W>(zs, p.N, red, m, s);
    best = cal_group_max_key<W>(best, redk);
    // the row's loss in float64: s64 = sum_c exp(z_c - m) once more, thread partials in ascending c
    double s64 = 0.0;
    for (int c = t; c < p.N; c += W) s64 += exp((double)zs[c] - (double)m);
    s64 = cal_group_sum<W>(s64, redd);
    if (t == 0) {
        const int pred = knn_key_index(best);
        const float conf = soft_prob(bf * z[pred], m, s);
        const double nll = log(s64) + ((double)m - (double)(bf * z[y]));
        p.rec[row] = TopRec{conf, cal_bin(conf, p.bins) | (pred == (int)y ? 256 : 0), nll};
    }
}

struct TopReduceP {
    const TopRec* rec; long long n; int bins;
    long long* count; long long* correct; double* conf_sum; double* nll_sum;
};

__global__ __launch_bounds__(kCalThreads) void toplabel_reduce_kernel(TopReduceP p) {
    __shared__ int s_cnt[kCalWaves][64], s_hit[kCalWaves][64];
    __shared__ double s_conf[kCalWaves][64], s_nll[kCalWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long run = ((p.n + kCalWaves - 1) / kCalWaves + 63) / 64 * 64;      // rows per wave, a multiple of 64
    const long long lo = w * run, hi = min(p.n, lo + run);
    int cnt = 0, hit = 0;
    double conf = 0.0, nll = 0.0;
    for (long long r0 = lo; r0 < hi; r0 += 64) {
        const long long r = r0 + lane;
        TopRec x{0.f, -1, 0.0};
        if (r < hi) x = p.rec[r];
        if (x.code >= 0) nll += x.nll;                             // lane partials over ascending rows
        const int m = (int)min(64LL, hi - r0);
        for (int j = 0; j < m; ++j) {
            const int cj = __builtin_amdgcn_readlane(x.code, j);
            const double pj = (double)lane_float(x.conf, j);
            if (cj >= 0 && lane == (cj & 255)) {
                ++cnt;
                hit += cj >> 8;
                conf += pj;
            }
        }
    }
    nll = wave_sum(nll);
    s_cnt[w][lane] = cnt; s_hit[w][lane] = hit; s_conf[w][lane] = conf;
    if (lane == 0) s_nll[w] = nll;
    __syncthreads();
    if (threadIdx.x < p.bins) {
        long long c = 0, h = 0;
        double f = 0.0;
        for (int k = 0; k < kCalWaves; ++k) { c += s_cnt[k][lane]; h += s_hit[k][lane]; f += s_conf[k][lane]; }
        p.count[lane] = c; p.correct[lane] = h; p.conf_sum[lane] = f;
    }
    if (threadIdx.x == 0) {
        double f = 0.0;
        for (int k = 0; k < kCalWaves; ++k) f += s_nll[k];
        p.nll_sum[0] = f;
    }
}

// ---- Platt scaling -------------------------------------------------------------------------------------------------------------
// logits (n, C) row stride ld and targets (n, C) row stride ld_t -> zc[c][i] and yc[c][i], coalesced both ways
__global__ __launch_bounds__(256) void platt_prep_kernel(const float* __restrict__ logits, long long ld,
                                                         const void* __restrict__ target, int u8, long long ld_t, int n, int C,
                                                         float* __restrict__ zc, unsigned char* __restrict__ yc, int* status) {
    __shared__ float s_z[kCalTile][kCalTile + 1];
    __shared__ unsigned char s_y[kCalTile][kCalTile + 4];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * kCalTile;
    const int c0 = blockIdx.y * kCalTile;
    int bad = 0;
    for (int rr = ty; rr < kCalTile; rr += 4) {
        const long long r = r0 + rr;
        const int c = c0 + tx;
        if (r < n && c < C) {
            const float v = logits[r * ld + c];
            if (cal_nonfinite(v)) bad |= ACX_CAL_NONFINITE;
            s_z[rr][tx] = v;
            unsigned char l;
            if (u8) {
                const unsigned char t = static_cast<const unsigned char*>(target)[r * ld_t + c];
                if (t > 1) bad |= ACX_CAL_BAD_TARGET;
                l = t != 0;
            } else {
                const float t = static_cast<const float*>(target)[r * ld_t + c];
                if (!(t == 0.0f || t == 1.0f)) bad |= ACX_CAL_BAD_TARGET;
                l = t == 1.0f;
            }
            s_y[rr][tx] = l;
        }
    }
    __syncthreads();
    for (int cc = ty; cc < kCalTile; cc += 4) {
        const int c = c0 + cc;
        const long long r = r0 + tx;
        if (r < n && c < C) {
            zc[(long long)c * n + r] = s_z[tx][cc];
            yc[(long long)c * n + r] = s_y[tx][cc];
        }
    }
    const unsigned long long b1 = __ballot(bad & ACX_CAL_NONFINITE), b2 = __ballot(bad & ACX_CAL_BAD_TARGET);
    const int bits = (b1 ? ACX_CAL_NONFINITE : 0) | (b2 ? ACX_CAL_BAD_TARGET : 0);
    if (__lane_id() == 0 && bits) atomicOr(status, bits);
}

// v[k] summed over the workgroup: lanes by the xor butterfly, then the 8 waves in wave order; the same bits in every thread
template <int K>
__device__ __forceinline__ void cal_block_sum(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();                                               // the previous reduction's reads of red
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = red[k];
        for (int w = 1; w < kPlattWaves; ++w) s += red[w * K + k];
        v[k] = s;
    }
}

struct PlattP {
    const float* zc; const unsigned char* yc; int n; int smooth; const int* status; double* ab; int* info;
};

// F, the gradient (ga, gb) and the Hessian (haa, hab, hbb) of one class at (a, b); LDS: the column in cal_dyn, labels in `mask`
template <bool LDS>
__device__ __forceinline__ void platt_eval(const float* zc, const unsigned char* yc, unsigned long long mask, int n, double a, double b,
                                           double tp, double tn, double* red, double (&v)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0.0;
    int k = 0;
    for (int i = threadIdx.x; i < n; i += kPlattThreads, ++k) {
        const double z = (double)(LDS ? cal_dyn[i] : zc[i]);
        const bool y = LDS ? ((mask >> k) & 1ull) != 0 : yc[i] != 0;
        const double t = y ? tp : tn;
        const double u = a * z + b;
        const double e = exp(-fabs(u));
        const double l1 = log1p(e);
        const double lp = fmin(u, 0.0) - l1, lq = fmin(-u, 0.0) - l1;
        const double inv = 1.0 / (1.0 + e);
        const double pr = u >= 0.0 ? inv : e * inv;
        const double g = pr - t, h = e * inv * inv;
        v[0] -= t * lp + (1.0 - t) * lq;
        v[1] += g * z;
        v[2] += g;
        v[3] += h * z * z;
        v[4] += h * z;
        v[5] += h;
    }
    cal_block_sum<6>(v, red);
}

template <bool LDS>
__global__ __launch_bounds__(kPlattThreads) void platt_fit_kernel(PlattP p) {
    __shared__ double red[kPlattWaves * 6];
    const int c = blockIdx.x, n = p.n;
    const float* zc = p.zc + (long long)c * n;
    const unsigned char* yc = p.yc + (long long)c * n;
    double* ab = p.ab + 2 * (long long)c;
    if (*p.status) {                                               // bad data: nothing to fit (uniform over the grid)
        if (threadIdx.x == 0) { ab[0] = 1.0; ab[1] = 0.0; p.info[c] = ACX_CAL_DEGENERATE; }
        return;
    }
    unsigned long long mask = 0;
    double st[3] = {0.0, 0.0, 0.0};                                // P, and whether any value lies below / above the first
    const float z0 = zc[0];
    {
        int k = 0;
        for (int i = threadIdx.x; i < n; i += kPlattThreads, ++k) {
            const float z = zc[i];
            const bool y = yc[i] != 0;
            if (LDS) { cal_dyn[i] = z; mask |= y ? 1ull << k : 0ull; }
            st[0] += y ? 1.0 : 0.0;
            st[1] += z != z0 ? 1.0 : 0.0;
        }
    }
    cal_block_sum<3>(st, red);                                     // counts: exact in float64
    const double P = st[0], Nn = (double)n - st[0];
    if (P == 0.0 || Nn == 0.0 || st[1] == 0.0) {
        if (threadIdx.x == 0) { ab[0] = 1.0; ab[1] = 0.0; p.info[c] = ACX_CAL_DEGENERATE; }
        return;
    }
    const double tp = p.smooth ? (P + 1.0) / (P + 2.0) : 1.0, tn = p.smooth ? 1.0 / (Nn + 2.0) : 0.0;
    // ONE evaluation site: (a, b) is the accepted point, (ta, tb) the trial.  The first evaluation is accepted as it is;
    // afterwards a trial is accepted when F does not increase (kCalFSlack), else the step is halved (50 times at the most).  The iteration
    // stops at an accepted point whose full Newton step is within 1e-10 max(1, |a|, |b|): F itself cannot see steps that small.
    double a = 0.0, b = log((P + 1.0) / (Nn + 1.0));
    double ta = a, tb = b, da = 0.0, db = 0.0, step = 1.0;
    double Fa = 0.0;                                               // F at (a, b)
    int info = ACX_CAL_NOT_CONVERGED, it = 0, halvings = 0;
    bool first = true;
    for (;;) {
        double w[6];
        platt_eval<LDS>(zc, yc, mask, n, ta, tb, tp, tn, red, w);
        if (first || w[0] <= Fa + kCalFSlack * fmax(1.0, fabs(Fa))) {
            first = false;
            a = ta;
            b = tb;
            Fa = w[0];
            const double haa = w[3] + 1e-12, hbb = w[5] + 1e-12, hab = w[4];
            const double det = haa * hbb - hab * hab;
            da = -(hbb * w[1] - hab * w[2]) / det;
            db = -(haa * w[2] - hab * w[1]) / det;
            if (fmax(fabs(da), fabs(db)) <= 1e-10 * fmax(1.0, fmax(fabs(a), fabs(b)))) { info = it; break; }
            if (it == 100) break;                                  // ACX_CAL_NOT_CONVERGED
            ++it;
            step = 1.0;
            halvings = 0;
        } else {
            step *= 0.5;
            if (++halvings == 50) { info = it; break; }            // no step lowers F any more: the minimiser to rounding
        }
        ta = a + step * da;
        tb = b + step * db;
    }
    if (threadIdx.x == 0) { ab[0] = a; ab[1] = b; p.info[c] = info; }
}

__global__ __launch_bounds__(256) void platt_apply_kernel(const float* __restrict__ z, long long ld, long long rows, int C,
                                                          const double* __restrict__ ab, float* __restrict__ out, long long ld_p) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    if (c >= C) return;
    const float a = (float)ab[2 * c], b = (float)ab[2 * c + 1];
#pragma clang loop vectorize(disable) interleave(disable)       // no packed-FP32 instructions
    for (long long r = (long long)blockIdx.y * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.y * 4)
        out[r * ld_p + c] = head_sigmoid(fmaf(a, z[r * ld + c], b));
}

// ---- temperature scaling -----------------------------------------------------------------------------------------------------
struct TempState {
    double beta_try;      // where the next evaluation runs
    double base, Fb;      // the last accepted beta and F there
    double d, step;       // the Newton direction from base and the current step scale
    int evals, done, code, cut;
    unsigned ticket;
};
static_assert(sizeof(TempState) <= kTempStateBytes, "state block");

// the decision after one evaluation gave (F, g, h) at st->beta_try; nonconst: rows that are not constant
__device__ void temp_decide(TempState* st, double F, double g, double h, double nonconst, double* beta, int* info) {
    st->evals += 1;
    bool accepted = false, done = false;
    int code = 0;
    if (st->evals == 1) {
        st->base = 1.0;
        st->beta_try = 1.0;
        if (nonconst == 0.0) { done = true; code = ACX_CAL_DEGENERATE; }
        else { st->Fb = F; accepted = true; }
    } else if (F <= st->Fb + kCalFSlack * fmax(1.0, fabs(st->Fb))) {
        const double delta = st->step * st->d;
        st->base = st->beta_try;
        st->Fb = F;
        // a step the bound has cut down to nothing: the iteration stands against 1e-4 or 1e4
        if (st->cut && fabs(delta) <= 1e-10 * fmax(1.0, st->base)) { done = true; code = ACX_CAL_AT_BOUND; }
        else accepted = true;
    } else {
        st->step *= 0.5;
        if (st->step < 0x1p-60) { done = true; code = st->cut ? ACX_CAL_AT_BOUND : st->evals; }
        else st->beta_try = st->base + st->step * st->d;
    }
    if (accepted) {
        const double d = -g / fmax(h, 1e-12);
        if (!(fabs(d) <= 1.79e308)) { done = true; code = ACX_CAL_NOT_CONVERGED; }
        else if (fabs(d) <= 1e-10 * fmax(1.0, st->base)) { done = true; code = st->evals; }   // the Newton step at an accepted point
        else {
            double step = 1.0;
            int cut = 0;
            for (int k = 0; k < 1200; ++k) {
                const double bt = st->base + step * d;
                if (bt >= 1e-4 && bt <= 1e4) break;
                step *= 0.5;
                cut = 1;
            }
            st->d = d; st->step = step; st->cut = cut;
            st->beta_try = st->base + step * d;
        }
    }
    if (done) { st->done = 1; st->code = code; }
    *beta = st->base;
    *info = st->done ? st->code : ACX_CAL_NOT_CONVERGED;
}

struct TempEvalP {
    const float* z; long long ld; const long long* labels; long long n; int N; int rpg; long long groups;
    TempState* st; double* part;   // [groups][4]: F, F', F'', rows that are not constant
    double* beta; int* info; int* status;
};

__global__ __launch_bounds__(64) void temperature_clear_kernel(unsigned* state, int* status) {
    state[threadIdx.x] = 0u;                                       // kTempStateBytes = 64 words
    if (threadIdx.x == 0) *status = 0;
}
static_assert(kTempStateBytes == 64 * 4, "temperature_clear_kernel clears 64 words");

template <int W>
__global__ __launch_bounds__(kRowThreads) void temperature_eval_kernel(TempEvalP p) {
    __shared__ double red[4];
    __shared__ double s_tot[4][4];
    __shared__ unsigned s_last;
    if (p.st->done) return;                                        // written by an earlier launch: uniform over the grid
    const double beta = p.st->evals == 0 ? 1.0 : p.st->beta_try;  // a cleared state block: the first evaluation, at beta = 1
    const int t = soft_thread<W>();
    const long long g = W == 64 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
    const long long r_lo = min(p.n, g * p.rpg), r_hi = min(p.n, r_lo + p.rpg);
    double aF = 0.0, aG = 0.0, aH = 0.0, aC = 0.0;
    int flags = 0;
    for (long long row = r_lo; row < r_hi; ++row) {
        const float* z = p.z + row * p.ld;
        const long long y = p.labels[row];
        const bool ybad = y < 0 || y >= p.N;
        bool bad = false;
        float mx = -INFINITY, mn = INFINITY;
        for (int c = t; c < p.N; c += W) {
            const float v = z[c];
            bad |= acx_nonfinite(v);
            mx = fmaxf(mx, v);
            mn = fminf(mn, v);
        }
        bad = group_any<W>(bad);
        if (bad || ybad) {                                         // uniform over the group
            flags |= (bad ? ACX_CAL_NONFINITE : 0) | (ybad ? ACX_CAL_BAD_LABEL : 0);
            continue;
        }
        // max and min over the group (order-free); beta > 0, so the largest scaled logit is beta * max
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); mn = fminf(mn, __shfl_xor(mn, o)); }
        if (W == 256) {
            __shared__ float s_mx[4], s_mn[4];
            __syncthreads();
            if ((threadIdx.x & 63) == 0) { s_mx[threadIdx.x >> 6] = mx; s_mn[threadIdx.x >> 6] = mn; }
            __syncthreads();
            mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
            mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
        }
        const double zm = (double)mx;
        double s = 0.0, sz = 0.0;
        for (int c = t; c < p.N; c += W) {
            const double zc = (double)z[c];
            const double e = exp(beta * (zc - zm));
            s += e;
            sz += e * zc;
        }
        s = cal_group_sum<W>(s, red);
        sz = cal_group_sum<W>(sz, red);
        const double E = sz / s;
        double var = 0.0;
        for (int c = t; c < p.N; c += W) {
            const double zc = (double)z[c];
            const double e = exp(beta * (zc - zm));
            var += e * ((zc - E) * (zc - E));
        }
        var = cal_group_sum<W>(var, red) / s;
        const double zy = (double)z[y];
        aF += log(s) + beta * (zm - zy);
        aG += E - zy;
        aH += var;
        aC += mx != mn ? 1.0 : 0.0;
    }
    // one partial per group, through to L2 (agent scope); the fence orders it in front of the ticket
    if (t == 0 && g < p.groups) {
        double* o = p.part + 4 * g;
        __hip_atomic_store(o + 0, aF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, aG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 2, aH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 3, aC, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (flags) atomicOr(p.status, flags);
        __threadfence();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = atomicAdd(&p.st->ticket, 1u);
        s_last = prev == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last workgroup: thread t adds partials t, t + 256, ... in ascending order, lanes by the butterfly, waves in order
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < p.groups; i += kRowThreads) {
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k] += __hip_atomic_load(p.part + 4 * i + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] = wave_sum(tot[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_tot[threadIdx.x >> 6][k] = tot[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = ((s_tot[0][k] + s_tot[1][k]) + s_tot[2][k]) + s_tot[3][k];
        p.st->ticket = 0u;                                         // the next launch counts from zero again
        temp_decide(p.st, f[0], f[1], f[2], f[3], p.beta, p.info);
    }
}

__global__ __launch_bounds__(256) void temperature_apply_kernel(const float* __restrict__ z, long long ld, long long rows, int N,
                                                                const double* __restrict__ beta, float* __restrict__ out,
                                                                long long ld_o) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    if (c >= N) return;
    const float bf = (float)*beta;
#pragma clang loop vectorize(disable) interleave(disable)
    for (long long r = (long long)blockIdx.y * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.y * 4)
        out[r * ld_o + c] = bf * z[r * ld + c];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static int cal_check_shape(const char* who, int64_t n, int classes, int64_t ld, const char* ld_name) {
    if (n < 1) ACX_FAIL(ACX_ERR_ARG, "%s: n = %lld (expected >= 1)", who, (long long)n);
    if (classes < 1 || classes > ACX_MAX_CLASSES)
        ACX_FAIL(ACX_ERR_ARG, "%s: classes = %d (expected 1 .. %d)", who, classes, ACX_MAX_CLASSES);
    if (ld < classes) ACX_FAIL(ACX_ERR_ARG, "%s: %s = %lld is shorter than %d classes", who, ld_name, (long long)ld, classes);
    if (n > kCalMaxRows) ACX_FAIL(ACX_ERR_UNSUPPORTED, "%s: n = %lld (at most 2^30)", who, (long long)n);
    return ACX_OK;
}
static int cal_check_bins(const char* who, int bins) {
    if (bins < 1 || bins > ACX_CAL_MAX_BINS) ACX_FAIL(ACX_ERR_ARG, "%s: bins = %d (expected 1 .. %d)", who, bins, ACX_CAL_MAX_BINS);
    return ACX_OK;
}
static int cal_check_target(const char* who, const void* target, int target_dtype, int64_t ld_t, int classes) {
    if (!target) ACX_FAIL(ACX_ERR_ARG, "%s: target is null", who);
    if (target_dtype != ACX_TARGET_F32 && target_dtype != ACX_TARGET_U8)
        ACX_FAIL(ACX_ERR_ARG, "%s: target_dtype %d (expected ACX_TARGET_F32 or ACX_TARGET_U8)", who, target_dtype);
    if (ld_t < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld_t = %lld is shorter than %d classes", who, (long long)ld_t, classes);
    return ACX_OK;
}
static void platt_layout(long long n, long long C, size_t* y_off, size_t* total) {
    const size_t zb = align_up((size_t)n * C * 4), yb = align_up((size_t)n * C);
    *y_off = zb;
    *total = zb + yb;
}
static size_t temp_bytes(long long n) { return kTempStateBytes + align_up((size_t)n * 32); }
static dim3 cal_apply_grid(int64_t rows, int classes) {
    const long long by = (rows + 3) / 4;
    return dim3((unsigned)((classes + 63) / 64), (unsigned)(by > 4096 ? 4096 : by));
}

}  // namespace acx

using namespace acx;

extern "C" {

int acx_reliability_counts(const float* probs, int64_t ld, const void* target, int target_dtype, int64_t ld_t, int64_t n,
                           int classes, int bins, int64_t* count, int64_t* positive, double* conf_sum, double* brier_sum,
                           int32_t* status, void* stream) {
    static const char* who = "acx_reliability_counts";
    if (!probs) ACX_FAIL(ACX_ERR_ARG, "%s: probs is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!count || !positive || !conf_sum || !brier_sum) ACX_FAIL(ACX_ERR_ARG, "%s: an output is null", who);
    ACX_TRY(cal_check_bins(who, bins));
    ACX_TRY(cal_check_shape(who, n, classes, ld, "ld"));
    ACX_TRY(cal_check_target(who, target, target_dtype, ld_t, classes));
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, 4, s));
    const RelCountsP p{probs, ld, target, target_dtype == ACX_TARGET_U8 ? 1 : 0, ld_t, (int)n, classes, bins,
                       reinterpret_cast<long long*>(count), reinterpret_cast<long long*>(positive), conf_sum, brier_sum,
                       (int*)status};
    launch_kernel(&reliability_counts_kernel, dim3((unsigned)((classes + kCalWaves - 1) / kCalWaves)), dim3(kCalThreads), 0, s, p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_temperature_workspace_bytes(int64_t n, int classes, size_t* out_bytes) {
    static const char* who = "acx_temperature_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(cal_check_shape(who, n, classes, classes, "ld"));
    *out_bytes = temp_bytes(n);
    return ACX_OK;
}

int acx_reliability_toplabel(const float* logits, int64_t ld, const int64_t* labels, int64_t n, int classes, const double* beta,
                             int bins, int64_t* count, int64_t* correct, double* conf_sum, double* nll_sum, int32_t* status,
                             void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "acx_reliability_toplabel";
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!count || !correct || !conf_sum || !nll_sum) ACX_FAIL(ACX_ERR_ARG, "%s: an output is null", who);
    if (!workspace) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    ACX_TRY(cal_check_bins(who, bins));
    ACX_TRY(cal_check_shape(who, n, classes, ld, "ld"));
    ACX_TRY(check_workspace_for(who, workspace, workspace_bytes, temp_bytes(n)));
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, 4, s));
    TopRec* rec = reinterpret_cast<TopRec*>(static_cast<char*>(workspace) + kTempStateBytes);
    const TopRowP p{logits, ld, reinterpret_cast<const long long*>(labels), n, classes, beta, bins, rec, (int*)status};
    if (classes <= kSoftWaveMaxN) {
        launch_kernel(&toplabel_row_kernel<64>, dim3((unsigned)((n + 3) / 4)), dim3(kRowThreads), (size_t)classes * 16, s, p);
    } else {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &toplabel_row_kernel<256>, (size_t)ACX_MAX_CLASSES * 4));
        launch_kernel(&toplabel_row_kernel<256>, dim3((unsigned)n), dim3(kRowThreads), (size_t)classes * 4, s, p);
    }
    ACX_HIP(hipGetLastError());
    const TopReduceP q{rec, n, bins, reinterpret_cast<long long*>(count), reinterpret_cast<long long*>(correct), conf_sum, nll_sum};
    launch_kernel(&toplabel_reduce_kernel, dim3(1), dim3(kCalThreads), 0, s, q);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_platt_workspace_bytes(int64_t n, int classes, size_t* out_bytes) {
    static const char* who = "acx_platt_workspace_bytes";
    if (!out_bytes) ACX_FAIL(ACX_ERR_ARG, "%s: out_bytes is null", who);
    ACX_TRY(cal_check_shape(who, n, classes, classes, "ld"));
    size_t yo;
    platt_layout(n, classes, &yo, out_bytes);
    return ACX_OK;
}

int acx_platt_fit(const float* logits, int64_t ld, const void* target, int target_dtype, int64_t ld_t, int64_t n, int classes,
                  int smooth, double* ab, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "acx_platt_fit";
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!ab || !info) ACX_FAIL(ACX_ERR_ARG, "%s: an output is null", who);
    if (!workspace) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    ACX_TRY(cal_check_shape(who, n, classes, ld, "ld"));
    ACX_TRY(cal_check_target(who, target, target_dtype, ld_t, classes));
    size_t yo, need;
    platt_layout(n, classes, &yo, &need);
    ACX_TRY(check_workspace_for(who, workspace, workspace_bytes, need));
    hipStream_t s = (hipStream_t)stream;
    ACX_HIP(hipMemsetAsync(status, 0, 4, s));
    float* zc = static_cast<float*>(workspace);
    unsigned char* yc = reinterpret_cast<unsigned char*>(static_cast<char*>(workspace) + yo);
    const dim3 pgrid((unsigned)((n + kCalTile - 1) / kCalTile), (unsigned)((classes + kCalTile - 1) / kCalTile));
    launch_kernel(&platt_prep_kernel, pgrid, dim3(256), 0, s, logits, (long long)ld, target, target_dtype == ACX_TARGET_U8 ? 1 : 0,
                  (long long)ld_t, (int)n, classes, zc, yc, (int*)status);
    ACX_HIP(hipGetLastError());
    const PlattP p{zc, yc, (int)n, smooth ? 1 : 0, (const int*)status, ab, (int*)info};
    if (n <= kCalLdsRows) {
        static DeviceOnce once;
        ACX_TRY(set_max_dynamic_lds(once, &platt_fit_kernel<true>, (size_t)kCalLdsRows * 4));
        launch_kernel(&platt_fit_kernel<true>, dim3(classes), dim3(kPlattThreads), (size_t)n * 4, s, p);
    } else {
        launch_kernel(&platt_fit_kernel<false>, dim3(classes), dim3(kPlattThreads), 0, s, p);
    }
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_platt_apply(const float* logits, int64_t ld, int64_t rows, int classes, const double* ab, float* probs, int64_t ld_p,
                    void* stream) {
    static const char* who = "acx_platt_apply";
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!ab) ACX_FAIL(ACX_ERR_ARG, "%s: ab is null", who);
    if (!probs) ACX_FAIL(ACX_ERR_ARG, "%s: probs is null", who);
    ACX_TRY(cal_check_shape(who, rows, classes, ld, "ld"));
    if (ld_p < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld_p = %lld is shorter than %d classes", who, (long long)ld_p, classes);
    hipStream_t s = (hipStream_t)stream;
    launch_kernel(&platt_apply_kernel, cal_apply_grid(rows, classes), dim3(256), 0, s, logits, (long long)ld, (long long)rows,
                  classes, ab, probs, (long long)ld_p);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

int acx_temperature_fit(const float* logits, int64_t ld, const int64_t* labels, int64_t n, int classes, int evaluations,
                        double* beta, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "acx_temperature_fit";
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!labels) ACX_FAIL(ACX_ERR_ARG, "%s: labels is null", who);
    if (!status) ACX_FAIL(ACX_ERR_ARG, "%s: status is null", who);
    if (!beta || !info) ACX_FAIL(ACX_ERR_ARG, "%s: an output is null", who);
    if (!workspace) ACX_FAIL(ACX_ERR_ARG, "%s: workspace is null", who);
    if (evaluations < 1 || evaluations > ACX_CAL_MAX_EVALUATIONS)
        ACX_FAIL(ACX_ERR_ARG, "%s: evaluations = %d (expected 1 .. %d)", who, evaluations, ACX_CAL_MAX_EVALUATIONS);
    ACX_TRY(cal_check_shape(who, n, classes, ld, "ld"));
    ACX_TRY(check_workspace_for(who, workspace, workspace_bytes, temp_bytes(n)));
    hipStream_t s = (hipStream_t)stream;
    // the status word and the state block, cleared by a kernel of the call's own: all zero means "nothing evaluated yet"
    launch_kernel(&temperature_clear_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned*>(workspace), (int*)status);
    ACX_HIP(hipGetLastError());
    TempEvalP p{logits, ld, reinterpret_cast<const long long*>(labels), n, classes, 1, 0,
                reinterpret_cast<TempState*>(workspace),
                reinterpret_cast<double*>(static_cast<char*>(workspace) + kTempStateBytes), beta, (int*)info, (int*)status};
    const long long rpg = (n + 4095) / 4096;
    p.rpg = (int)rpg;
    p.groups = (n + rpg - 1) / rpg;
    for (int e = 0; e < evaluations; ++e) {
        if (classes <= kSoftWaveMaxN)
            launch_kernel(&temperature_eval_kernel<64>, dim3((unsigned)((p.groups + 3) / 4)), dim3(kRowThreads), 0, s, p);
        else
            launch_kernel(&temperature_eval_kernel<256>, dim3((unsigned)p.groups), dim3(kRowThreads), 0, s, p);
        ACX_HIP(hipGetLastError());
    }
    return ACX_OK;
}

int acx_temperature_apply(const float* logits, int64_t ld, int64_t rows, int classes, const double* beta, float* out, int64_t ld_o,
                          void* stream) {
    static const char* who = "acx_temperature_apply";
    if (!logits) ACX_FAIL(ACX_ERR_ARG, "%s: logits is null", who);
    if (!beta) ACX_FAIL(ACX_ERR_ARG, "%s: beta is null", who);
    if (!out) ACX_FAIL(ACX_ERR_ARG, "%s: out is null", who);
    ACX_TRY(cal_check_shape(who, rows, classes, ld, "ld"));
    if (ld_o < classes) ACX_FAIL(ACX_ERR_ARG, "%s: ld_o = %lld is shorter than %d classes", who, (long long)ld_o, classes);
    hipStream_t s = (hipStream_t)stream;
    launch_kernel(&temperature_apply_kernel, cal_apply_grid(rows, classes), dim3(256), 0, s, logits, (long long)ld, (long long)rows,
                  classes, beta, out, (long long)ld_o);
    ACX_HIP(hipGetLastError());
    return ACX_OK;
}

}  // extern "C"
