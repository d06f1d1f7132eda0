// Feasibility form: separable sums of convex vector sets projected on the device.
//   reference: src/problemforms/Feasibility/Feasibility.jl:2-6 -- Feasibility(S1, S2, n) takes ANY two ProximableFunctions.  IndAffine, IndBox and
//   ConeProduct have kernels of their own (feas.hip); this file adds the sets a user of the form reaches for next -- IndBallL2, IndBallL1, IndSimplex,
//   IndHalfspace, IndHyperslab, IndPoint, IndFree and IndBox with scalar bounds -- alone or as a SeparableSum of contiguous blocks (the shape of
//   examples/youla.jl:199-205), so that a projection onto them no longer crosses the host link (fos_feas_set_callback).
//
// One projection is a FIXED number of launches, whatever the data, with no host synchronise and no copy.  Blocks fall into three classes by length:
//   wavefront class (len <= 1024)    one wavefront per block, four blocks per workgroup: the block is read once into registers (16 per lane), norms, dots and
//                                    the whole threshold search run on chip, y is written once.  ALL blocks of this class: one launch.
//   workgroup class (len <= 16 384)  one 256-thread workgroup per block, the values in LDS (up to 128 KiB); the same traffic.  ALL blocks: one launch.
//   grid class (longer)              per block, one after another: a reduction pass by the whole grid (per-workgroup partials), a one-workgroup decision,
//                                    for the threshold sets THR_CAP x (pass + decision) launches that return at once when the device flag says the search
//                                    has ended, then the apply pass.  Loads and stores are double2.
// No floating-point atomics; every sum has a fixed order, so two runs give the same bits.
//
// The threshold search (IndSimplex on x, IndBallL1 on |x|): find tau with g(tau) = sum max(v_i - tau, 0) = a.
//   bracket [max v - a, max v - a / len] (g >= a at the left end, <= a at the right); every pass evaluates g at THR_C interior candidates in ONE sweep
//   over the data (THR_C accumulators per lane) together with count(v > lo), count(v >= hi) and sum(v : v > lo), and keeps the sub-interval where g
//   crosses a.  The search ends when count(v > lo) == count(v >= hi) (no breakpoint inside: the finish is exact) or when the width is
//   <= 2^-50 max(|max v|, a); the finish is tau = (sum(v : v > lo) - a) / count(v > lo), whose error is at most the bracket's width, ties included.
//   A pass divides the width by THR_C + 1 = 33 = 2^5.04, the first width is <= a, so after 10 narrowing passes it is <= 2^-50.4 a and the 11th pass
//   finishes: THR_CAP = ceil(52 / log2(THR_C + 1)) = 11.  thr_decide ends the search at the cap in any case (NaN data cannot spin).
// fos_host_set_project runs the same steps on the CPU (the same inline functions; lane-strided partial sums combined in the kernels' order).
//
// Proximable functions that are not indicators (FOS_FN_*, numbered from 32; the step is 1 as in prox!(y, S, x)) are further kinds of the same three classes:
//   elementwise   NormL1 (soft threshold), SqrNormL2 (x / (1 + lambda)), ElasticNet (both), Linear (x - c)
//   one reduction NormL2 and HuberLoss on |x|_2, the shape of IndBallL2
//   threshold     NormLinf: prox = x - P_{|.|_1 <= lambda}(x) = sign(x) min(|x|, tau) with IndBallL1's tau for the radius lambda
// A decision is 0 (apply the formula), 1 (y = x, the same bits) or 2 (y = 0).
//
// Dense Quadratic / LeastSquares / IndAffine blocks (kinds 48..50, fos_feas_set_blocks2) are the optional dense part of the same object: they take no part in the
// three classes above, and dense_blocks.hip adds their one or two launches behind the ones of this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dev_common.hpp"
#include "fos_internal.hpp"

namespace fos {

constexpr int SET_THREADS = 256;
constexpr int SET_WAVE_MAX = 1024;            // wavefront class: 64 lanes x 16 values
constexpr int SET_WAVE_NV = SET_WAVE_MAX / 64;
constexpr int SET_WG_MAX = 16384;             // workgroup class: 128 KiB of LDS
constexpr int SET_PARTS = 256;                // workgroups of a grid-class pass (fixed: results do not depend on the device)
constexpr int THR_C = 32;                     // candidates per pass
constexpr int THR_NACC = THR_C + 3;           // g at the candidates, count(v > lo), count(v >= hi), sum(v : v > lo)
constexpr int THR_CAP = 11;                   // ceil(52 / log2(THR_C + 1))

struct SetBlock {
    int64_t start, len;
    int32_t kind, pad;
    double s0, s1;          // r, - | a, - | lo, hi (IndHalfspace: -inf, b) | IndBox lo, hi | lambda, - | ElasticNet mu, lambda | HuberLoss rho, mu
    double aa;              // <a, a> of a halfspace / hyperslab | 1 / (1 + lambda) of SqrNormL2 and ElasticNet, 1 / (1 + mu) of HuberLoss
};

// ------------------------------------------------------------------------------------------ the formulas, shared by the kernels and the host emulation
// Kind tests are one shift of a constant bit set, not a chain of comparisons: the chain `kind == FOS_SET_BALL_L1 || kind == FOS_FN_NORM_LINF` becomes a two-case
// switch whose gfx950 code lost the fabs of set_thr_value for FOS_SET_BALL_L1 (the optimised IR is right, the emitted code is not); a shift has no control
// flow to lower.  Kinds are validated (set_block_make) to lie in 0..63.
#define SET_BIT(k) (1ull << (k))
__host__ __device__ inline bool set_kind_in(int kind, unsigned long long mask) { return (mask >> (kind & 63)) & 1ull; }
__host__ __device__ inline bool set_is_threshold(int kind) { return set_kind_in(kind, SET_BIT(FOS_SET_BALL_L1) | SET_BIT(FOS_SET_SIMPLEX) | SET_BIT(FOS_FN_NORM_LINF)); }
__host__ __device__ inline bool set_is_scalar(int kind) {
    return set_kind_in(kind, SET_BIT(FOS_SET_BALL_L2) | SET_BIT(FOS_SET_HALFSPACE) | SET_BIT(FOS_SET_HYPERSLAB) | SET_BIT(FOS_FN_NORM_L2) | SET_BIT(FOS_FN_HUBER));
}
__host__ __device__ inline bool set_thr_abs(int kind) { return set_kind_in(kind, SET_BIT(FOS_SET_BALL_L1) | SET_BIT(FOS_FN_NORM_LINF)); }      // the search runs on |x|, after a test of |x|_1
__host__ __device__ inline bool set_reads_vec(int kind) {
    return set_kind_in(kind, SET_BIT(FOS_SET_BALL_L2) | SET_BIT(FOS_SET_HALFSPACE) | SET_BIT(FOS_SET_HYPERSLAB) | SET_BIT(FOS_SET_POINT) | SET_BIT(FOS_FN_LINEAR));
}
// the summand of the one reduction a set needs: |x - c|^2, <a, x>, |x|_1, |x|^2
__host__ __device__ inline double set_term(int kind, double xi, double vi) {
    if (kind == FOS_SET_BALL_L2) { const double d = xi - vi; return d * d; }
    if (kind == FOS_SET_HALFSPACE || kind == FOS_SET_HYPERSLAB) return vi * xi;
    if (set_thr_abs(kind)) return fabs(xi);
    if (kind == FOS_FN_NORM_L2 || kind == FOS_FN_HUBER) return xi * xi;
    return 0.0;
}
__host__ __device__ inline double set_thr_value(int kind, double xi) { return set_thr_abs(kind) ? fabs(xi) : xi; }

// copy: 1: y = x, the same bits; 2: y = 0; 0: the formula with p0: the scale r / |d|, the step along the normal, the threshold, the shrink factor
struct SetDecision { int copy; double p0; };
// from the block's one sum s (set_term); a threshold kind that comes back with copy == 0 goes on to its search
__host__ __device__ inline SetDecision set_decide_scalar(const SetBlock& b, double s) {
    SetDecision d{1, 0.0};
    switch (b.kind) {
    case FOS_SET_BALL_L2: {
        const double nd = sqrt(s);
        if (!(nd <= b.s0)) { d.copy = 0; d.p0 = b.s0 / nd; }
        break;
    }
    case FOS_SET_HALFSPACE:
    case FOS_SET_HYPERSLAB:                                        // towards whichever side is violated
        if (s > b.s1) { d.copy = 0; d.p0 = (s - b.s1) / b.aa; }
        else if (s < b.s0) { d.copy = 0; d.p0 = (s - b.s0) / b.aa; }
        break;
    case FOS_SET_BALL_L1: d.copy = s <= b.s0; break;
    case FOS_FN_NORM_LINF: d.copy = b.s0 == 0.0 ? 1 : s <= b.s0 ? 2 : 0; break;       // lambda = 0: f = 0; |x|_1 <= lambda: x is its own projection onto the ball
    case FOS_FN_NORM_L2: {
        const double nd = sqrt(s);
        if (b.s0 == 0.0) break;
        if (nd <= b.s0) d.copy = 2;
        else { d.copy = 0; d.p0 = 1.0 - b.s0 / nd; }
        break;
    }
    case FOS_FN_HUBER: {
        const double nd = sqrt(s);
        d.copy = 0;
        d.p0 = nd <= b.s0 * (1.0 + b.s1) ? b.aa : 1.0 - b.s0 * b.s1 / nd;
        break;
    }
    default: d.copy = b.kind == FOS_SET_FREE; break;               // no reduction: IndSimplex goes to its search, the elementwise kinds to set_apply
    }
    return d;
}
__host__ __device__ inline double set_soft(double xi, double t) { const double m = fabs(xi) - t; return copysign(m > 0.0 ? m : 0.0, xi); }
__host__ __device__ inline double set_apply(const SetBlock& b, int copy, double p0, double xi, double vi) {
    if (copy) return copy == 1 ? xi : 0.0;
    switch (b.kind) {
    case FOS_SET_BALL_L2: return vi + (xi - vi) * p0;
    case FOS_SET_BALL_L1: { const double m = fabs(xi) - p0; return copysign(m > 0.0 ? m : 0.0, xi); }
    case FOS_SET_SIMPLEX: { const double m = xi - p0; return m > 0.0 ? m : 0.0; }
    case FOS_SET_HALFSPACE:
    case FOS_SET_HYPERSLAB: return xi - p0 * vi;
    case FOS_SET_POINT: return vi;
    case FOS_SET_BOX: return fmin(fmax(xi, b.s0), b.s1);
    case FOS_FN_NORM_L1: return set_soft(xi, b.s0);                 // (lambda = 0: copysign(|x|, x), the same bits)
    case FOS_FN_SQR_NORM_L2: return xi * b.aa;
    case FOS_FN_ELASTIC_NET: return set_soft(xi, b.s0) * b.aa;
    case FOS_FN_LINEAR: return xi - vi;
    case FOS_FN_NORM_L2:
    case FOS_FN_HUBER: return xi * p0;
    case FOS_FN_NORM_LINF: return copysign(fmin(fabs(xi), p0), xi);
    default: return xi;                                            // FOS_SET_FREE
    }
}

struct ThrState { double lo, hi, tau, scale; int done, passes; };
__host__ __device__ inline void thr_init(ThrState& s, double mx, double a, double len, bool l1) {
    s.lo = mx - a;
    if (l1 && s.lo < 0.0) s.lo = 0.0;                              // |x|_1 > r: the threshold is positive
    s.hi = mx - a / len;
    if (!(s.hi >= s.lo)) s.hi = s.lo;
    s.tau = s.lo; s.scale = fmax(fabs(mx), a); s.done = 0; s.passes = 0;
}
__host__ __device__ inline double thr_cand(double lo, double hi, int j) {          // candidate j = 1 .. THR_C (0: lo, THR_C + 1: hi)
    return fmin(fma(hi - lo, (double)j * (1.0 / (THR_C + 1)), lo), hi);
}
__host__ __device__ inline void thr_accumulate(double v, double lo, double hi, double (&acc)[THR_NACC]) {
#pragma unroll
    for (int j = 0; j < THR_C; ++j) { const double d = v - thr_cand(lo, hi, j + 1); acc[j] += d > 0.0 ? d : 0.0; }
    acc[THR_C] += v > lo ? 1.0 : 0.0;
    acc[THR_C + 1] += v >= hi ? 1.0 : 0.0;
    acc[THR_C + 2] += v > lo ? v : 0.0;
}
// one pass's totals -> the search has ended (tau) or the sub-interval where g crosses a
__host__ __device__ inline void thr_decide(ThrState& s, const double* red, double a) {
    s.passes += 1;
    const double cnt_lo = red[THR_C], cnt_hi = red[THR_C + 1], sum_lo = red[THR_C + 2];
    if (cnt_lo == cnt_hi || !((s.hi - s.lo) > 0x1p-50 * s.scale) || s.passes >= THR_CAP) {
        s.tau = cnt_lo > 0.0 ? (sum_lo - a) / cnt_lo : s.lo;
        s.done = 1;
        return;
    }
    int j = 0;                                                     // g decreases: the last candidate still at or above a
    for (int k = 1; k <= THR_C; ++k) if (red[k - 1] >= a) j = k;
    const double nlo = j == 0 ? s.lo : thr_cand(s.lo, s.hi, j), nhi = j == THR_C ? s.hi : thr_cand(s.lo, s.hi, j + 1);
    s.lo = nlo; s.hi = nhi;
}

// ------------------------------------------------------------------------------------------ on chip: wavefront and workgroup classes
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
// sums over a team of NT threads (a wavefront, or the workgroup through sm[4 K]); every thread gets the same bits
template <int NT, int K>
__device__ __forceinline__ void team_sum(double (&a)[K], double* sm) {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = wave_sum(a[k]);
    if constexpr (NT > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        __syncthreads();                                           // (what the last call left in sm has been read)
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) sm[wave * K + k] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = ((sm[k] + sm[K + k]) + sm[2 * K + k]) + sm[3 * K + k];
    }
}
template <int NT>
__device__ __forceinline__ double team_max(double v, double* sm) {
    v = wave_max(v);
    if constexpr (NT > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 0) sm[wave] = v;
        __syncthreads();
        v = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
    }
    return v;
}

// The values of one block, held by a team of NT threads; thread t owns the elements t, t + NT, ...: NV > 0 keeps them in NV registers (len <= NT NV),
// NV == 0 in LDS (xs[len]; a thread reads back only what it wrote itself, so no barrier is needed).
template <int NT, int NV>
struct TeamValues {
    double v[NV];
    __device__ __forceinline__ void load(const double* __restrict__ xb, int len, int t, double*) {
#pragma unroll
        for (int k = 0; k < NV; ++k) { const int i = t + NT * k; v[k] = i < len ? xb[i] : 0.0; }
    }
    template <typename F>
    __device__ __forceinline__ void each(int len, int t, F&& f) const {
#pragma unroll
        for (int k = 0; k < NV; ++k) { const int i = t + NT * k; if (i < len) f(i, v[k]); }
    }
};
template <int NT>
struct TeamValues<NT, 0> {
    double* xs;
    __device__ __forceinline__ void load(const double* __restrict__ xb, int len, int t, double* lds) {
        xs = lds;
        for (int i = t; i < len; i += NT) xs[i] = xb[i];
    }
    template <typename F>
    __device__ __forceinline__ void each(int len, int t, F&& f) const {
        for (int i = t; i < len; i += NT) f(i, xs[i]);
    }
};

// one block by a team of NT threads: read once, every norm, dot and the whole threshold search on chip, written once.  Every branch is uniform over the team.
template <int NT, int NV>
__device__ __forceinline__ void set_block_onchip(const SetBlock& b, const double* __restrict__ x, const double* __restrict__ vec, double* __restrict__ y,
                                                 int32_t* __restrict__ passes, int t, double* sm, double* lds) {
    const int len = (int)b.len, kind = __builtin_amdgcn_readfirstlane(b.kind);      // one block per team: the kind tests become scalar branches
    const double* vb = vec ? vec + b.start : nullptr;
    double* yb = y + b.start;
    TeamValues<NT, NV> xv;
    xv.load(x + b.start, len, t, lds);
    int npass = 0;
    double s[1] = {0.0};
    if (set_is_scalar(kind) || set_thr_abs(kind)) {
        xv.each(len, t, [&](int i, double xi) { s[0] += set_term(kind, xi, vb ? vb[i] : 0.0); });
        team_sum<NT, 1>(s, sm);
    }
    const SetDecision d = set_decide_scalar(b, s[0]);
    const int copy = d.copy;
    double p0 = d.p0;
    if (set_is_threshold(kind) && !copy) {
        double m = -INFINITY;
        xv.each(len, t, [&](int, double xi) { m = fmax(m, set_thr_value(kind, xi)); });
        m = team_max<NT>(m, sm);
        ThrState st;
        thr_init(st, m, b.s0, (double)len, set_thr_abs(kind));
        while (!st.done) {                                         // at most THR_CAP passes (thr_decide)
            double acc[THR_NACC];
#pragma unroll
            for (int a = 0; a < THR_NACC; ++a) acc[a] = 0.0;
            const double lo = st.lo, hi = st.hi;
            xv.each(len, t, [&](int, double xi) { thr_accumulate(set_thr_value(kind, xi), lo, hi, acc); });
            team_sum<NT, THR_NACC>(acc, sm);
            thr_decide(st, acc, b.s0);
        }
        p0 = st.tau; npass = st.passes;
    }
    const bool needs_vec = !copy && vb && set_reads_vec(kind);
    xv.each(len, t, [&](int i, double xi) { yb[i] = set_apply(b, copy, p0, xi, needs_vec ? vb[i] : 0.0); });
    if (t == 0) *passes = npass;
}

__global__ __launch_bounds__(SET_THREADS) void sets_wave_kernel(const SetBlock* __restrict__ blocks, const int32_t* __restrict__ ids, int count,
                                                                const double* __restrict__ x, const double* __restrict__ vec, double* __restrict__ y,
                                                                int32_t* __restrict__ passes) {
    const int w = blockIdx.x * (SET_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= count) return;                                        // (a whole wavefront; this kernel has no workgroup barrier)
    const int id = ids[w];
    const SetBlock b = blocks[id];
    set_block_onchip<64, SET_WAVE_NV>(b, x, vec, y, passes + id, threadIdx.x & 63, nullptr, nullptr);
}
// dynamic LDS: 8 bytes x the longest block of this class (at most 128 KiB of the CU's 160)
__global__ __launch_bounds__(SET_THREADS) void sets_wg_kernel(const SetBlock* __restrict__ blocks, const int32_t* __restrict__ ids,
                                                              const double* __restrict__ x, const double* __restrict__ vec, double* __restrict__ y,
                                                              int32_t* __restrict__ passes) {
    extern __shared__ __attribute__((aligned(16))) double set_xs[];
    __shared__ double sm[4 * THR_NACC];
    const int id = ids[blockIdx.x];
    const SetBlock b = blocks[id];
    set_block_onchip<SET_THREADS, 0>(b, x, vec, y, passes + id, threadIdx.x, sm, set_xs);
}

// ------------------------------------------------------------------------------------------ grid class
// state of one grid-class block, in doubles: done, copy, p0, lo, hi, passes, scale
enum { GS_DONE = 0, GS_COPY, GS_P0, GS_LO, GS_HI, GS_PASSES, GS_SCALE, GS_WORDS = 8 };

// the elements start .. start + len - 1 as aligned pairs (i even: one 16-byte access) by the whole grid, plus an odd head / tail by thread 0
template <typename F>
__device__ __forceinline__ void set_grid_for(int64_t start, int64_t len, F&& f) {
    const int64_t end = start + len, a0 = (start + 1) & ~(int64_t)1, a1 = end & ~(int64_t)1;
    const int64_t gid = blockIdx.x * (int64_t)SET_THREADS + threadIdx.x, gsz = (int64_t)gridDim.x * SET_THREADS;
    for (int64_t i = a0 + 2 * gid; i < a1; i += 2 * gsz) f(i, true);
    if (gid == 0) {
        if (start < a0) f(start, false);
        if (a1 >= a0 && a1 < end) f(a1, false);
    }
}
__device__ __forceinline__ double2 set_ld2(const double* __restrict__ p, int64_t i, bool two) {
    if (!p) return make_double2(0.0, 0.0);
    return two ? *reinterpret_cast<const double2*>(p + i) : make_double2(p[i], 0.0);
}

__global__ __launch_bounds__(SET_THREADS) void sets_grid_reduce_kernel(SetBlock b, const double* __restrict__ x, const double* __restrict__ vec,
                                                                       double* __restrict__ partials) {
    __shared__ double sm[8];
    double s = 0.0, m = -INFINITY;
    const int kind = b.kind;
    set_grid_for(b.start, b.len, [&](int64_t i, bool two) {
        const double2 xx = set_ld2(x, i, two), vv = set_ld2(vec, i, two);
        s += set_term(kind, xx.x, vv.x); m = fmax(m, set_thr_value(kind, xx.x));
        if (two) { s += set_term(kind, xx.y, vv.y); m = fmax(m, set_thr_value(kind, xx.y)); }
    });
    s = wave_sum(s); m = wave_max(m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sm[wave] = s; sm[4 + wave] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
        partials[2 * blockIdx.x + 1] = fmax(fmax(sm[4], sm[5]), fmax(sm[6], sm[7]));
    }
}
// one wavefront: the records in order, the set's decision or the start of its threshold search
__global__ __launch_bounds__(64) void sets_grid_decide_kernel(SetBlock b, const double* __restrict__ partials, int nparts, double* __restrict__ gs) {
    const int lane = threadIdx.x;
    double s = 0.0, m = -INFINITY;
    for (int r = lane; r < nparts; r += 64) { s += partials[2 * r]; m = fmax(m, partials[2 * r + 1]); }
    s = wave_sum(s); m = wave_max(m);
    if (lane != 0) return;
    const SetDecision d = set_decide_scalar(b, s);
    double done = 1.0, copy = d.copy, p0 = d.p0, lo = 0.0, hi = 0.0, scale = 0.0;
    if (set_is_threshold(b.kind) && !d.copy) {
        ThrState st;
        thr_init(st, m, b.s0, (double)b.len, set_thr_abs(b.kind));
        done = 0.0; lo = st.lo; hi = st.hi; scale = st.scale; p0 = st.tau;
    }
    gs[GS_DONE] = done; gs[GS_COPY] = copy; gs[GS_P0] = p0; gs[GS_LO] = lo; gs[GS_HI] = hi; gs[GS_PASSES] = 0.0; gs[GS_SCALE] = scale;
}
__global__ __launch_bounds__(SET_THREADS) void sets_grid_pass_kernel(SetBlock b, const double* __restrict__ x, const double* __restrict__ gs,
                                                                     double* __restrict__ partials) {
    __shared__ double sm[4 * THR_NACC];
    if (gs[GS_DONE] != 0.0) return;                                // the search has ended (every thread reads the same word)
    const double lo = gs[GS_LO], hi = gs[GS_HI];
    const int kind = b.kind;
    double acc[THR_NACC];
#pragma unroll
    for (int a = 0; a < THR_NACC; ++a) acc[a] = 0.0;
    set_grid_for(b.start, b.len, [&](int64_t i, bool two) {
        const double2 xx = set_ld2(x, i, two);
        thr_accumulate(set_thr_value(kind, xx.x), lo, hi, acc);
        if (two) thr_accumulate(set_thr_value(kind, xx.y), lo, hi, acc);
    });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < THR_NACC; ++a) {
        const double v = wave_sum(acc[a]);
        if (lane == 0) sm[wave * THR_NACC + a] = v;
    }
    __syncthreads();
    if (threadIdx.x < THR_NACC) {
        const int a = threadIdx.x;
        partials[(size_t)blockIdx.x * THR_NACC + a] = ((sm[a] + sm[THR_NACC + a]) + sm[2 * THR_NACC + a]) + sm[3 * THR_NACC + a];
    }
}
__global__ __launch_bounds__(SET_THREADS) void sets_grid_pass_decide_kernel(SetBlock b, const double* __restrict__ partials, int nparts,
                                                                            double* __restrict__ gs) {
    __shared__ double sm[4 * THR_NACC];
    if (gs[GS_DONE] != 0.0) return;
    const int a = threadIdx.x & 63, q = threadIdx.x >> 6;
    if (a < THR_NACC) {
        double s = 0.0;
        for (int r = q; r < nparts; r += 4) s += partials[(size_t)r * THR_NACC + a];
        sm[q * THR_NACC + a] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double red[THR_NACC];
    for (int k = 0; k < THR_NACC; ++k) red[k] = ((sm[k] + sm[THR_NACC + k]) + sm[2 * THR_NACC + k]) + sm[3 * THR_NACC + k];
    ThrState st;
    st.lo = gs[GS_LO]; st.hi = gs[GS_HI]; st.tau = gs[GS_P0]; st.scale = gs[GS_SCALE]; st.done = 0; st.passes = (int)gs[GS_PASSES];
    thr_decide(st, red, b.s0);
    gs[GS_LO] = st.lo; gs[GS_HI] = st.hi; gs[GS_P0] = st.tau; gs[GS_PASSES] = (double)st.passes; gs[GS_DONE] = st.done ? 1.0 : 0.0;
}
// gs == nullptr: a kind without a reduction (IndFree, IndPoint, IndBox, the elementwise functions)
__global__ __launch_bounds__(SET_THREADS) void sets_grid_apply_kernel(SetBlock b, const double* __restrict__ x, const double* __restrict__ vec,
                                                                      double* __restrict__ y, const double* __restrict__ gs) {
    const int copy = gs ? (int)gs[GS_COPY] : (b.kind == FOS_SET_FREE);
    const double p0 = gs ? gs[GS_P0] : 0.0;
    set_grid_for(b.start, b.len, [&](int64_t i, bool two) {
        const double2 xx = set_ld2(x, i, two), vv = set_ld2(vec, i, two);
        if (two) *reinterpret_cast<double2*>(y + i) = make_double2(set_apply(b, copy, p0, xx.x, vv.x), set_apply(b, copy, p0, xx.y, vv.y));
        else y[i] = set_apply(b, copy, p0, xx.x, vv.x);
    });
}

// ------------------------------------------------------------------------------------------ host side
struct SetBlocks : ProxObject, DevOwned {
    SetBlocks() : ProxObject(FEAS_BLOCKS) { what = "fos_feas_set_blocks"; }
    ~SetBlocks() override { dense_blocks_free(dense); }
    DenseBlocks* dense = nullptr;               // the dense Quadratic / LeastSquares / IndAffine blocks (dense_blocks.hip): at most two more launches
    int prox(hipStream_t stream, double* y, const double* x) override;
    int64_t n = 0;
    std::vector<SetBlock> blocks;
    std::vector<int> grid_ids;                  // grid-class blocks, in order
    int nwave = 0, nwg = 0, launches = 0;
    size_t wg_lds = 0;                          // bytes of dynamic LDS of the workgroup-class launch
    SetBlock* d_blocks = nullptr;
    int32_t *d_wave_ids = nullptr, *d_wg_ids = nullptr, *d_passes = nullptr;
    double *d_vec = nullptr, *d_partials = nullptr, *d_gstate = nullptr;
};

namespace {

bool set_kind_is_fn(int kind) { return kind >= FOS_FN_NORM_L1 && kind <= FOS_FN_NORM_LINF; }
const char* set_kind_name(int kind) {
    static const char* names[] = {"IndFree", "IndBallL2", "IndBallL1", "IndSimplex", "IndHalfspace", "IndHyperslab", "IndPoint", "IndBox"};
    static const char* fn_names[] = {"NormL1", "SqrNormL2", "ElasticNet", "Linear", "NormL2", "HuberLoss", "NormLinf"};
    if (set_kind_is_fn(kind)) return fn_names[kind - FOS_FN_NORM_L1];
    return kind >= 0 && kind <= FOS_SET_BOX ? names[kind] : "?";
}
bool is_fin(double v) { return v == v && std::fabs(v) <= 1.79e308; }
// pairwise sum of f(0 .. len - 1): <a, a> is computed once, to rounding
template <typename F>
double pairwise_sum(int64_t lo, int64_t hi, F&& f) {
    if (hi - lo <= 64) { double s = 0.0; for (int64_t i = lo; i < hi; ++i) s += f(i); return s; }
    const int64_t mid = lo + (hi - lo) / 2;
    return pairwise_sum(lo, mid, f) + pairwise_sum(mid, hi, f);
}
int set_grid_size(int64_t len) { return (int)std::min<int64_t>(SET_PARTS, (len + 2 * SET_THREADS - 1) / (2 * SET_THREADS)); }

// one block's parameters -> its descriptor; `blk` (1-based) names it in the message
int set_block_make(int64_t blk, int32_t kind, int64_t start, int64_t len, const double* scal2, const double* vec, SetBlock* out) {
    if ((kind < FOS_SET_FREE || kind > FOS_SET_BOX) && !set_kind_is_fn(kind)) { set_error("set block %lld: unknown kind %d (FOS_SET_*, FOS_FN_*)", (long long)blk, (int)kind); return FOS_EINVAL; }
    if (len < 1) { set_error("set block %lld (%s): length %lld < 1", (long long)blk, set_kind_name(kind), (long long)len); return FOS_EINVAL; }
    SetBlock b{};
    b.start = start; b.len = len; b.kind = kind; b.s0 = scal2[0]; b.s1 = scal2[1]; b.aa = 0.0;
    const bool needs_vec = set_reads_vec(kind) && kind != FOS_SET_BALL_L2;                // (a ball without a centre is around the origin)
    if (needs_vec && !vec) { set_error("set block %lld (%s): the vector argument is required", (long long)blk, set_kind_name(kind)); return FOS_EINVAL; }
    if (vec && set_reads_vec(kind)) {
        for (int64_t i = 0; i < len; ++i) if (!is_fin(vec[start + i])) { set_error("set block %lld (%s): entry %lld of its vector is not finite", (long long)blk, set_kind_name(kind), (long long)i + 1); return FOS_EINVAL; }
    }
    switch (kind) {
    case FOS_SET_BALL_L2: case FOS_SET_BALL_L1:
        if (!is_fin(b.s0) || b.s0 < 0.0) { set_error("set block %lld (%s): the radius must be finite and >= 0", (long long)blk, set_kind_name(kind)); return FOS_EINVAL; }
        b.s1 = 0.0; break;
    case FOS_SET_SIMPLEX:
        if (!is_fin(b.s0) || !(b.s0 > 0.0)) { set_error("set block %lld (IndSimplex): a must be finite and > 0", (long long)blk); return FOS_EINVAL; }
        b.s1 = 0.0; break;
    case FOS_SET_HALFSPACE:
        if (!is_fin(b.s0)) { set_error("set block %lld (IndHalfspace): b must be finite", (long long)blk); return FOS_EINVAL; }
        b.s1 = b.s0; b.s0 = -INFINITY; break;                      // the hyperslab without a lower side
    case FOS_SET_HYPERSLAB:
        if (!is_fin(b.s0) || !is_fin(b.s1) || b.s0 > b.s1) { set_error("set block %lld (IndHyperslab): finite lo <= hi are required", (long long)blk); return FOS_EINVAL; }
        break;
    case FOS_SET_BOX:
        if (!(b.s0 <= b.s1)) { set_error("set block %lld (IndBox): lo <= hi is required", (long long)blk); return FOS_EINVAL; }
        break;
    case FOS_FN_NORM_L1: case FOS_FN_SQR_NORM_L2: case FOS_FN_NORM_L2: case FOS_FN_NORM_LINF:
        if (!is_fin(b.s0) || b.s0 < 0.0) { set_error("set block %lld (%s): lambda must be finite and >= 0", (long long)blk, set_kind_name(kind)); return FOS_EINVAL; }
        b.s1 = 0.0; b.aa = 1.0 / (1.0 + b.s0); break;
    case FOS_FN_ELASTIC_NET:
        if (!is_fin(b.s0) || b.s0 < 0.0 || !is_fin(b.s1) || b.s1 < 0.0) { set_error("set block %lld (ElasticNet): mu and lambda must be finite and >= 0", (long long)blk); return FOS_EINVAL; }
        b.aa = 1.0 / (1.0 + b.s1); break;
    case FOS_FN_HUBER:
        if (!is_fin(b.s0) || !(b.s0 > 0.0) || !is_fin(b.s1) || b.s1 < 0.0) { set_error("set block %lld (HuberLoss): rho must be finite and > 0, mu finite and >= 0", (long long)blk); return FOS_EINVAL; }
        b.aa = 1.0 / (1.0 + b.s1); break;
    default: b.s0 = b.s1 = 0.0; break;
    }
    if (kind == FOS_SET_HALFSPACE || kind == FOS_SET_HYPERSLAB) {
        b.aa = pairwise_sum(0, len, [&](int64_t i) { return vec[start + i] * vec[start + i]; });
        if (!(b.aa > 0.0) || !is_fin(b.aa)) { set_error("set block %lld (%s): the normal vector is zero (or its square overflows)", (long long)blk, set_kind_name(kind)); return FOS_EINVAL; }
    }
    *out = b;
    return FOS_OK;
}

// the host emulation's sums: element i belongs to lane i mod T; a wavefront's 64 lanes are added pairwise, a workgroup's four wavefronts and then the
// workgroups in order -- the association of the kernels
double host_combine(const std::vector<double>& lane, int64_t T, int K, int k) {
    double total = 0.0;
    for (int64_t g0 = 0; g0 < T; g0 += SET_THREADS) {
        double wg = 0.0;
        for (int64_t w0 = g0; w0 < std::min<int64_t>(T, g0 + SET_THREADS); w0 += 64) {
            double v[64];
            for (int l = 0; l < 64; ++l) v[l] = lane[(size_t)(w0 + l) * K + k];
            for (int off = 1; off < 64; off <<= 1) for (int l = 0; l < 64; l += 2 * off) v[l] += v[l + off];
            wg = (w0 == g0) ? v[0] : wg + v[0];
        }
        total = (g0 == 0) ? wg : total + wg;
    }
    return total;
}

}  // namespace

int set_blocks_setup(int64_t n, int64_t nblocks, const int32_t* kind, const int64_t* len, const double* scal, const double* vec, ProxObject** out) {
    return set_blocks_setup2(n, nblocks, kind, len, scal, vec, DenseBlockArgs{}, out);
}

// dense.block_mat != nullptr: blocks of the kinds 48..50 are dense blocks (dense_blocks.hip) and take no part in the three classes below
int set_blocks_setup2(int64_t n, int64_t nblocks, const int32_t* kind, const int64_t* len, const double* scal, const double* vec, const DenseBlockArgs& dense,
                      ProxObject** out) {
    if (!out || n < 1 || nblocks < 1 || !kind || !len || !scal) { set_error("fos_feas_set_blocks: bad argument (nblocks >= 1; kind, len and scal are required)"); return FOS_EINVAL; }
    SetBlocks* p = new SetBlocks();
    p->n = n;
    auto fail = [&](int code) { delete p; return code; };
    int64_t pos = 0;
    bool any_vec = false;
    std::vector<int32_t> wave_ids, wg_ids;
    for (int64_t i = 0; i < nblocks; ++i) {
        if (len[i] < 1 || len[i] > n - pos) {
            set_error("set block %lld: length %lld does not fit the %lld entries left of n = %lld (contiguous blocks, in order, covering 1..n)", (long long)i + 1,
                      (long long)len[i], (long long)(n - pos), (long long)n);
            return fail(FOS_EINVAL);
        }
        SetBlock b;
        if (dense.block_mat && dense_block_kind(kind[i])) {        // validated, with its matrix, by dense_blocks_setup below
            b = SetBlock{};
            b.start = pos; b.len = len[i]; b.kind = kind[i];
            p->blocks.push_back(b);
            pos += len[i];
            continue;
        }
        const int rc = set_block_make(i + 1, kind[i], pos, len[i], scal + 2 * i, vec, &b);
        if (rc != FOS_OK) return fail(rc);
        any_vec = any_vec || set_reads_vec(b.kind);
        if (b.len <= SET_WAVE_MAX) wave_ids.push_back((int32_t)i);
        else if (b.len <= SET_WG_MAX) { wg_ids.push_back((int32_t)i); p->wg_lds = std::max(p->wg_lds, sizeof(double) * (size_t)b.len); }
        else {
            p->grid_ids.push_back((int)i);
            p->launches += set_is_threshold(b.kind) ? 3 + 2 * THR_CAP : set_is_scalar(b.kind) ? 3 : 1;
        }
        p->blocks.push_back(b);
        pos += len[i];
    }
    if (pos != n) { set_error("fos_feas_set_blocks: the %lld blocks cover %lld of the %lld entries", (long long)nblocks, (long long)pos, (long long)n); return fail(FOS_EINVAL); }
    p->nwave = (int)wave_ids.size(); p->nwg = (int)wg_ids.size();
    p->launches += (p->nwave > 0) + (p->nwg > 0);
    if (dense.block_mat) {
        std::vector<int64_t> start(p->blocks.size());
        for (size_t i = 0; i < p->blocks.size(); ++i) start[i] = p->blocks[i].start;
        const int rc = dense_blocks_setup(nblocks, kind, len, start.data(), scal, dense, &p->dense);
        if (rc != FOS_OK) return fail(rc);
        p->launches += dense_blocks_launches(p->dense);
    }
    const hipStream_t sync = nullptr;                        // (this set-up has no stream: blocking copies)
    int rc = p->upload(&p->d_blocks, p->blocks, sync);
    if (rc == FOS_OK && p->nwave > 0) rc = p->upload(&p->d_wave_ids, wave_ids, sync);
    if (rc == FOS_OK && p->nwg > 0) rc = p->upload(&p->d_wg_ids, wg_ids, sync);
    if (rc == FOS_OK) rc = p->zeros(&p->d_passes, p->blocks.size(), sync);
    if (rc == FOS_OK && any_vec && vec) rc = p->upload(&p->d_vec, vec, (size_t)n, sync);
    if (rc == FOS_OK && !p->grid_ids.empty()) rc = p->zeros(&p->d_partials, (size_t)SET_PARTS * THR_NACC, sync);
    if (rc == FOS_OK && !p->grid_ids.empty()) rc = p->zeros(&p->d_gstate, p->grid_ids.size() * GS_WORDS, sync);
    if (rc != FOS_OK) return fail(rc);
    if (p->wg_lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(sets_wg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SET_WG_MAX * (int)sizeof(double)) != hipSuccess) {
        set_error("fos_feas_set_blocks: %d bytes of LDS per workgroup are not available on this device", SET_WG_MAX * (int)sizeof(double));
        return fail(FOS_EUNSUPPORTED);
    }
    *out = p;
    return FOS_OK;
}

// y = the projection of x onto the product (device vectors of length n, y must not alias x): p->launches launches, nothing else
int SetBlocks::prox(hipStream_t stream, double* y, const double* x) {
    const SetBlocks* p = this;
    const double* vec = p->d_vec;
    if (p->nwave > 0)
        hipLaunchKernelGGL(sets_wave_kernel, dim3((p->nwave + 3) / 4), dim3(SET_THREADS), 0, stream, (const SetBlock*)p->d_blocks, (const int32_t*)p->d_wave_ids,
                           p->nwave, x, vec, y, p->d_passes);
    if (p->nwg > 0)
        hipLaunchKernelGGL(sets_wg_kernel, dim3(p->nwg), dim3(SET_THREADS), p->wg_lds, stream, (const SetBlock*)p->d_blocks, (const int32_t*)p->d_wg_ids, x, vec, y,
                           p->d_passes);
    for (size_t g = 0; g < p->grid_ids.size(); ++g) {
        const SetBlock& b = p->blocks[(size_t)p->grid_ids[g]];
        const int grid = set_grid_size(b.len);
        double* gs = p->d_gstate + g * GS_WORDS;
        const bool thr = set_is_threshold(b.kind);
        if (thr || set_is_scalar(b.kind)) {
            hipLaunchKernelGGL(sets_grid_reduce_kernel, dim3(grid), dim3(SET_THREADS), 0, stream, b, x, vec, p->d_partials);
            hipLaunchKernelGGL(sets_grid_decide_kernel, dim3(1), dim3(64), 0, stream, b, (const double*)p->d_partials, grid, gs);
            for (int pass = 0; thr && pass < THR_CAP; ++pass) {
                hipLaunchKernelGGL(sets_grid_pass_kernel, dim3(grid), dim3(SET_THREADS), 0, stream, b, x, (const double*)gs, p->d_partials);
                hipLaunchKernelGGL(sets_grid_pass_decide_kernel, dim3(1), dim3(SET_THREADS), 0, stream, b, (const double*)p->d_partials, grid, gs);
            }
            hipLaunchKernelGGL(sets_grid_apply_kernel, dim3(grid), dim3(SET_THREADS), 0, stream, b, x, vec, y, (const double*)gs);
        } else {
            hipLaunchKernelGGL(sets_grid_apply_kernel, dim3(grid), dim3(SET_THREADS), 0, stream, b, x, vec, y, (const double*)nullptr);
        }
    }
    if (p->dense) dense_blocks_prox(p->dense, stream, y, x);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("separable sum of sets: a kernel launch failed: %s", hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}

// out8: blocks, blocks of the wavefront / workgroup / grid class, launches of one projection, threshold passes of the last projection (max over the
// blocks), the pass cap, candidates per pass
int set_blocks_stats(const ProxObject* obj, hipStream_t stream, double* out8) {
    const SetBlocks* p = static_cast<const SetBlocks*>(obj);
    FOS_HIP(hipStreamSynchronize(stream));
    std::vector<int32_t> passes(p->blocks.size(), 0);
    FOS_HIP(hipMemcpy(passes.data(), p->d_passes, sizeof(int32_t) * passes.size(), hipMemcpyDeviceToHost));
    int mx = 0;
    for (int32_t v : passes) mx = std::max(mx, (int)v);
    if (!p->grid_ids.empty()) {
        std::vector<double> gs(p->grid_ids.size() * GS_WORDS);
        FOS_HIP(hipMemcpy(gs.data(), p->d_gstate, sizeof(double) * gs.size(), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < p->grid_ids.size(); ++g)
            if (set_is_threshold(p->blocks[(size_t)p->grid_ids[g]].kind)) mx = std::max(mx, (int)gs[g * GS_WORDS + GS_PASSES]);
    }
    out8[0] = (double)p->blocks.size(); out8[1] = p->nwave; out8[2] = p->nwg; out8[3] = (double)p->grid_ids.size();
    out8[4] = p->launches; out8[5] = mx; out8[6] = THR_CAP; out8[7] = THR_C;
    return FOS_OK;
}

const DenseBlocks* set_blocks_dense(const ProxObject* obj) { return static_cast<const SetBlocks*>(obj)->dense; }

}  // namespace fos

using namespace fos;

extern "C" {

// Test-only host emulation of one block's projection (no GPU needed): the threshold search and the formulas of the kernels above, with the sums of the
// class `len` falls in.  vec: the centre / normal / point (NULL where the kind has none; a NULL centre is the origin).  passes: threshold passes used.
int fos_host_set_project(int32_t kind, int64_t len, const double* scal2, const double* vec, const double* x, double* y, int32_t* passes) {
    if (!scal2 || !x || !y || len < 1) { set_error("fos_host_set_project: bad argument"); return FOS_EINVAL; }
    SetBlock b;
    FOS_TRY(set_block_make(1, kind, 0, len, scal2, vec, &b));
    const int64_t T = len <= SET_WAVE_MAX ? 64 : len <= SET_WG_MAX ? SET_THREADS : (int64_t)set_grid_size(len) * SET_THREADS;
    auto V = [&](int64_t i) { return vec ? vec[i] : 0.0; };
    int npass = 0;
    double s = 0.0;
    std::vector<double> lane;
    if (set_is_scalar(kind) || set_thr_abs(kind)) {
        lane.assign((size_t)T, 0.0);
        for (int64_t i = 0; i < len; ++i) lane[(size_t)(i % T)] += set_term(kind, x[i], V(i));
        s = host_combine(lane, T, 1, 0);
    }
    const SetDecision d = set_decide_scalar(b, s);
    const int copy = d.copy;
    double p0 = d.p0;
    if (set_is_threshold(kind) && !copy) {
        double mx = -INFINITY;
        for (int64_t i = 0; i < len; ++i) mx = std::fmax(mx, set_thr_value(kind, x[i]));
        ThrState st;
        thr_init(st, mx, b.s0, (double)len, set_thr_abs(kind));
        while (!st.done) {
            lane.assign((size_t)T * THR_NACC, 0.0);
            for (int64_t i = 0; i < len; ++i) thr_accumulate(set_thr_value(kind, x[i]), st.lo, st.hi, *reinterpret_cast<double(*)[THR_NACC]>(&lane[(size_t)(i % T) * THR_NACC]));
            double red[THR_NACC];
            for (int k = 0; k < THR_NACC; ++k) red[k] = host_combine(lane, T, THR_NACC, k);
            thr_decide(st, red, b.s0);
        }
        p0 = st.tau; npass = st.passes;
    }
    for (int64_t i = 0; i < len; ++i) y[i] = set_apply(b, copy, p0, x[i], V(i));
    if (passes) *passes = npass;
    return FOS_OK;
}

}  // extern "C"
