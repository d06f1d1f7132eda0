// Proximable functions whose prox is a solve in the n-space, for a SPARSE Q or A of ANY size:  y = M^-1 (x + c)  by conjugate gradients, nothing dense.
//   Quadratic(Q, q):            M = I + Q,            c = -q             (prox_f(x) = (I + Q)^-1 (x - q))
//   LeastSquares(A, b, lambda): M = I + lambda A'A,   c = lambda A'b     (prox_f(x) = (I + lambda A'A)^-1 (x + lambda A'b))
// The counterpart of ProximalOperators' iterative=true for both functions, which Feasibility.jl accepts as either set (src/problemforms/Feasibility/Feasibility.jl:2-6);
// nspace.hip keeps the same matrices as a dense inverse, up to order 46 000.
//
//   * set-up (host): validated by csc_check (sparse_rows.hpp).  Quadratic: the entries i >= j of the CSC Q are mirrored into ONE full symmetric CSR of
//     M = I + Q (the unit diagonal included: every row has an entry), so the product only gathers.  LeastSquares: A and A' as two CSR matrices by a counting pass,
//     WITHOUT a row scaling (the preconditioner below is the n-space diagonal, a row scaling of A would change M).  D = diag(M) > 0; c = lambda A'b on the device.
//   * rows (sf_plan_pass of sparse_rows.hpp): a row longer than 2 048 entries is cut into segments, one wavefront each; the others are packed 64 / g to a
//     wavefront.  A bounded grid walks the items, so a launch leaves at most NC_PARTS partial sums.  The LAST segment of a cut row to arrive (one counter per cut
//     row, no waiting) adds the row's partials in segment order and runs the row's epilogue; its share of the launch's sums goes to a slot of its own, so every sum
//     is formed in one fixed order whichever segment came last: a prox repeats bit for bit.
//   * a prox: warm start from the previous answer (reset(): from D^-1 (x + c)).  The TRUE residual r = x + c - M y and its rounding level | |M||y| + |x + c| |
//     are evaluated (nc_pass_kernel<NC_QR> / <NC_ATR> + <NC_TR>, nc_start_kernel); at |r| <= max(tol |x + c|, 16 eps level) the prox ends.  Otherwise preconditioned
//     CG runs in launches gated on a device flag, a batch per host look, then the residual is evaluated again (SparseAffine::prox of affine_sparse.hip).
//   * a CG iteration k, Quadratic, TWO launches:
//       nc_pass_kernel<NC_QW>:   [stop test on |r|^2 of k - 1; beta = rz_k / rz_k-1]   p_k = z + beta p_k-1 formed WHILE GATHERED (two operands per entry) and
//                                written row by row to the other p buffer;   w = M p_k;   sum p_k w
//       nc_update_kernel:        [alpha = rz_k / p'w; p'w <= 0: Q is not positive semidefinite]   y += alpha p;  r -= alpha w;  z = D^-1 r;   sums r z, r r
//     LeastSquares, THREE, by the single-reduction (merged) recurrence of the HSDE CG -- a second operand per gathered entry costs a pentadiagonal Q nothing (its
//     columns are its neighbours) but a third of the time on a random A, and p'M p needs no test of its own here, M being positive definite:
//       nc_pass_kernel<NC_AT>:   [stop test]   t = A z;   sum t t
//       nc_pass_kernel<NC_TG>:   w = M z = z + lambda A't;   sums r z and z z
//       nc_update_kernel:        [gamma = r'z;  delta = |z|^2 + lambda |A z|^2;  beta = gamma / gamma_k-1;  p'M p = delta - beta gamma / alpha_k-1;  alpha = gamma / p'M p]
//                                p = z + beta p;  s = w + beta s (= M p);  y += alpha p;  r -= alpha s;  z = D^-1 r;   sum r r
//     (p'M p <= 0 there is rounding: CG ends and starts again from the recomputed residual, as it does whenever that residual is above its level.)
//   Every scalar is recomputed by each workgroup from the same partial sums in the same order; workgroup 0 writes it for the launches behind.
//   * the host emulation (tests) runs the same items, lanes, trees and element formulas (shared __host__ __device__ functions, every multiply-add an explicit fma).
#include "fos_internal.hpp"
#include "dev_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

namespace fos {

namespace {

constexpr int NC_T = 256;                     // threads per workgroup: four wavefronts, an item each
constexpr int NC_W = NC_T / 64;
constexpr int NC_PARTS = 1024;                // workgroups of any launch (= length of a partial-sum region)
constexpr int NC_NSUM = 4;                    // sums of a sparse pass at the most
constexpr int NC_BATCH = 16, NC_ROUNDS_MAX = 8;
constexpr double NC_EPS = 2.220446049250313e-16;
// regions of part[] (NC_PARTS doubles each): the sums of the A pass, of the M / A' pass, of the update
enum : int { NC_R_A = 0, NC_R_M = 1, NC_R_U = NC_R_M + NC_NSUM, NC_REGIONS = NC_R_U + 2 };

struct NcState {                              // device scalars of the solve (+ a pinned host copy)
    double rz[2];                             // r'z of iteration k at rz[k & 1]
    double alpha[2];                          // LeastSquares (merged recurrence): the step of iteration k at alpha[k & 1]
    double rr, pmp;                           // |r|^2 of the last test; the p'M p that stopped the solve (flag)
    double level2, b2;                        // | |M||y| + |x + c| |^2 and |x + c|^2 of the last true residual
    double tol_abs, tol_in;                   // the prox ends at |r| <= tol_abs; CG stops at tol_in = tol_abs / 2 (the recomputed residual then passes at once)
    int32_t iter, done, flag, pad;            // flag: 1 = p'M p <= 0 (or NaN); 2 = the merged recurrence's denominator <= 0 (rounding): CG ends, the residual is recomputed
};

enum NcMode : int { NC_QW = 0, NC_QR = 1, NC_AT = 2, NC_ATR = 3, NC_TW = 4, NC_TR = 5, NC_TC = 6, NC_TG = 7 };
constexpr __host__ __device__ int nc_nsum(int mode) {
    return mode == NC_QW || mode == NC_AT || mode == NC_TW ? 1 : (mode == NC_TG ? 2 : (mode == NC_QR || mode == NC_TR ? 4 : 0));
}
constexpr __host__ __device__ bool nc_abs(int mode) { return mode == NC_QR || mode == NC_ATR || mode == NC_TR; }
constexpr __host__ __device__ bool nc_first(int mode) { return mode == NC_QW || mode == NC_AT; }       // the first launch of an iteration: the stop test
constexpr __host__ __device__ bool nc_cg(int mode) { return mode == NC_QW || mode == NC_AT || mode == NC_TW || mode == NC_TG; }
constexpr __host__ __device__ bool nc_beta(int mode) { return mode == NC_QW || mode == NC_TW; }      // the launches that form p_k = z + beta p_k-1 themselves

// one sparse matrix with its work items (device pointers; on the host emulation: host pointers)
struct NcMat {
    int nitems = 0, nfold = 0, grid = 1;
    const SfItem* items = nullptr;
    const int32_t *rp = nullptr, *ci = nullptr, *fptr = nullptr, *segk = nullptr;      // segk[slot] = the cut row (index into fptr) the slot belongs to
    const double* va = nullptr;
    int32_t* cnt = nullptr;                   // per cut row: segments arrived (0 between launches)
    double *seg = nullptr, *seg2 = nullptr;   // per slot: the segment's sum, its sum of absolute values
    double* fsum = nullptr;                   // [NC_NSUM][nfold]: the cut rows' shares of a launch's sums
};
// a launch's sums as its consumer reads them: nparts workgroup partials, then the cut rows' slots
struct NcSum { const double* part; int nparts; const double* fsum; int nfold; };
// the vectors a pass or an update touches (n- or m-vectors; which are read depends on the mode)
struct NcVec {
    const double *x, *c, *dinv;               // n
    double *y, *r, *z, *w, *pold, *pnew;      // n   (pold / pnew: the two p buffers of iteration k)
    double *t, *ta;                           // m   (t = A p or A y; ta = |A||y|;  NC_TC: t = b)
    double* cw;                               // NC_TC: c is written
    double lambda;
};

// ---- element formulas, shared by the kernels and the host emulation.  Every multiply-add is an explicit fma and nothing else may be contracted.
// p_k at an index: z + beta p_k-1 (k = 0: z)
__host__ __device__ __forceinline__ double nc_p(const NcVec& v, int64_t i, double beta, bool two) { return two ? fma(beta, v.pold[i], v.z[i]) : v.z[i]; }
// the operand of entry (row, col) and, for the residual modes, its absolute value
template <int MODE>
__host__ __device__ __forceinline__ double nc_operand(const NcVec& v, int32_t col, double beta, bool two, double& av) {
    if (MODE == NC_QW) return nc_p(v, col, beta, two);
    if (MODE == NC_AT) return v.z[col];
    if (MODE == NC_QR || MODE == NC_ATR) { const double o = v.y[col]; av = fabs(o); return o; }
    if (MODE == NC_TR) av = v.ta[col];
    return v.t[col];                                                                    // NC_TW, NC_TR, NC_TC
}
// a row's epilogue: s = the row's sum, sa = its sum of absolute values; f[] += the row's share of the launch's sums
template <int MODE>
__host__ __device__ __forceinline__ void nc_row(const NcVec& v, int64_t row, double s, double sa, double beta, bool two, double* f) {
#pragma clang fp contract(off)
    if (MODE == NC_QW) {
        const double pn = nc_p(v, row, beta, two);
        v.pnew[row] = pn; v.w[row] = s;
        f[0] = fma(pn, s, f[0]);
    } else if (MODE == NC_TW) {
        const double pn = nc_p(v, row, beta, two);
        v.pnew[row] = pn; v.w[row] = fma(v.lambda, s, pn);
        f[0] = fma(pn, pn, f[0]);
    } else if (MODE == NC_TG) {
        const double zi = v.z[row];
        v.w[row] = fma(v.lambda, s, zi);
        f[0] = fma(v.r[row], zi, f[0]); f[1] = fma(zi, zi, f[1]);
    } else if (MODE == NC_AT) {
        v.t[row] = s;
        f[0] = fma(s, s, f[0]);
    } else if (MODE == NC_ATR) {
        v.t[row] = s; v.ta[row] = sa;
    } else if (MODE == NC_TC) {
        v.cw[row] = v.lambda * s;
    } else {                                                                            // NC_QR, NC_TR: r = (x + c) - M y
        const double b = v.x[row] + v.c[row];
        double my = s, lv = sa;
        if (MODE == NC_TR) { const double yv = v.y[row]; my = fma(v.lambda, s, yv); lv = fma(v.lambda, sa, fabs(yv)); }
        const double rn = b - my, zn = v.dinv[row] * rn;
        lv += fabs(b);
        v.r[row] = rn; v.z[row] = zn;
        f[0] = fma(rn, rn, f[0]); f[1] = fma(rn, zn, f[1]); f[2] = fma(lv, lv, f[2]); f[3] = fma(b, b, f[3]);
    }
}
// the update of element i: f[0] += r z, f[1] += r r
__host__ __device__ __forceinline__ void nc_update(const NcVec& v, int64_t i, double alpha, double* f) {
#pragma clang fp contract(off)
    v.y[i] = fma(alpha, v.pnew[i], v.y[i]);
    const double rn = fma(-alpha, v.w[i], v.r[i]), zn = v.dinv[i] * rn;
    v.r[i] = rn; v.z[i] = zn;
    f[0] = fma(rn, zn, f[0]); f[1] = fma(rn, rn, f[1]);
}
// the same for the merged recurrence (LeastSquares): p (in pnew) and s = M p (in pold) are advanced here, in place
__host__ __device__ __forceinline__ void nc_update_merged(const NcVec& v, int64_t i, double alpha, double beta, bool two, double* f) {
#pragma clang fp contract(off)
    const double p = two ? fma(beta, v.pnew[i], v.z[i]) : v.z[i], s = two ? fma(beta, v.pold[i], v.w[i]) : v.w[i];
    v.pnew[i] = p; v.pold[i] = s;
    v.y[i] = fma(alpha, p, v.y[i]);
    const double rn = fma(-alpha, s, v.r[i]), zn = v.dinv[i] * rn;
    v.r[i] = rn; v.z[i] = zn;
    f[0] = fma(rn, zn, f[0]); f[1] = fma(rn, rn, f[1]);
}
// its scalars: gamma = r'z, delta = z'M z = |z|^2 + lambda |A z|^2  ->  beta, and p'M p = delta - beta gamma / alpha_k-1 (k = 0: delta)
__host__ __device__ __forceinline__ double nc_merged_pmp(const NcState* st, int k, double gamma, double delta, double* beta) {
#pragma clang fp contract(off)
    *beta = 0.0;
    if (k == 0) return delta;
    *beta = gamma / st->rz[(k - 1) & 1];
    return fma(-*beta, gamma / st->alpha[(k - 1) & 1], delta);
}
// the scalars at the head of a CG launch
__host__ __device__ __forceinline__ bool nc_stop(double rr, double tol_in, int k, int maxit) { return !(sqrt(rr) > tol_in) || k >= maxit; }
__host__ __device__ __forceinline__ void nc_start_scalars(NcState* st, double rr, double rz, double lev2, double b2, double tol) {
    const double ta = fmax(tol * sqrt(b2), 16.0 * NC_EPS * sqrt(lev2));
    st->rz[0] = rz; st->rz[1] = rz; st->rr = rr; st->pmp = 0.0; st->level2 = lev2; st->b2 = b2; st->tol_abs = ta; st->tol_in = 0.5 * ta;
    st->iter = 0; st->flag = 0; st->done = !(sqrt(rr) > ta) ? 1 : 0;                  // (a NaN ends the solve too: the host reports it)
}

// ------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ double nc_block_sum(double v, double* sh) {                 // fixed order: lanes by the wave's tree, wavefronts in index order
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < NC_W; ++i) s += sh[i];
    return s;
}
// the gate of a CG launch, read once per workgroup: its threads must not part ways on a flag that workgroup 0 of the same launch may be setting
__device__ __forceinline__ bool nc_gate(const NcState* st, int* flag) {
    if (threadIdx.x == 0) *flag = st->done;
    __syncthreads();
    return *flag != 0;
}
__device__ __forceinline__ double nc_total(const NcSum& q, int j, double* sh) {          // sum j of a launch: every workgroup adds the same numbers in the same order
    double v = 0.0;
    const double *p = q.part + (size_t)j * NC_PARTS, *f = q.fsum + (size_t)j * q.nfold;
    for (int i = threadIdx.x; i < q.nparts; i += NC_T) v += p[i];
    for (int i = threadIdx.x; i < q.nfold; i += NC_T) v += f[i];
    return nc_block_sum(v, sh);
}

// One sparse pass over the items of M (modes NC_Q*), A (NC_AT*) or A' (NC_T*).  A workgroup takes a contiguous run of items, its wavefronts one item at a time.
//   NC_QW / NC_AT / NC_TW: a CG launch of iteration k (gated; prev = the sums of the update in front: r z, r r).   NC_QR / NC_ATR / NC_TR: the true residual.
//   NC_TC (set-up): c = lambda A'b.
template <int MODE>
__global__ __launch_bounds__(NC_T) void nc_pass_kernel(NcMat M, NcVec v, double* __restrict__ part, NcSum prev, NcState* __restrict__ st, int k, int maxit) {
    __shared__ double sh[NC_W];
    __shared__ int gate;
    constexpr int NS = nc_nsum(MODE);
    constexpr bool ABS = nc_abs(MODE);
    double beta = 0.0;
    const bool two = nc_cg(MODE) && k > 0;
    if (nc_cg(MODE)) {
        if (nc_gate(st, &gate)) return;
        if (two) {
            if (nc_first(MODE)) {                                  // the stop test of iteration k - 1.  (Workgroup 0 sets `done` only where EVERY workgroup returns here
                const double rr = nc_total(prev, 1, sh);           //  by its own test, so a workgroup that reads the flag early or late does the same thing.)
                const bool stop = nc_stop(rr, st->tol_in, k, maxit);
                if (blockIdx.x == 0 && threadIdx.x == 0) { st->rr = rr; if (stop) st->done = 1; }
                if (stop) return;
            }
            if (nc_beta(MODE)) {
                const double rz = nc_total(prev, 0, sh);
                beta = rz / st->rz[(k - 1) & 1];
                if (nc_first(MODE) && blockIdx.x == 0 && threadIdx.x == 0) st->rz[k & 1] = rz;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per = (M.nitems + (int)gridDim.x - 1) / (int)gridDim.x;
    const int i0 = blockIdx.x * per, i1 = min(M.nitems, i0 + per);
    double acc[NS > 0 ? NS : 1];
#pragma unroll
    for (int j = 0; j < (NS > 0 ? NS : 1); ++j) acc[j] = 0.0;
    for (int it = i0 + wv; it < i1; it += NC_W) {                  // (wave-uniform)
        const SfItem w = M.items[it];
        const bool segment = w.c > 0;
        const int g = segment ? 64 : -w.c;
        const int sub = lane & (g - 1), kk = lane >> __builtin_ctz(g);
        const bool live = segment ? true : kk < w.b;
        const int row = segment ? w.a : w.a + kk;
        int e0 = 0, e1 = 0;
        if (segment) { e0 = w.b; e1 = w.b + w.c; }
        else if (live) { e0 = M.rp[row]; e1 = M.rp[row + 1]; }
        double s = 0.0, sa = 0.0;
        int e = e0 + sub;
        for (; e + 3 * g < e1; e += 4 * g) {                       // four loads of each stream in flight; the sum stays in entry order
            const int c0 = M.ci[e], c1 = M.ci[e + g], c2 = M.ci[e + 2 * g], c3 = M.ci[e + 3 * g];
            const double a0 = M.va[e], a1 = M.va[e + g], a2 = M.va[e + 2 * g], a3 = M.va[e + 3 * g];
            double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
            const double v0 = nc_operand<MODE>(v, c0, beta, two, b0), v1 = nc_operand<MODE>(v, c1, beta, two, b1);
            const double v2 = nc_operand<MODE>(v, c2, beta, two, b2), v3 = nc_operand<MODE>(v, c3, beta, two, b3);
            s = fma(a0, v0, s); s = fma(a1, v1, s); s = fma(a2, v2, s); s = fma(a3, v3, s);
            if (ABS) { sa = fma(fabs(a0), b0, sa); sa = fma(fabs(a1), b1, sa); sa = fma(fabs(a2), b2, sa); sa = fma(fabs(a3), b3, sa); }
        }
        for (; e < e1; e += g) {
            double b0 = 0.0;
            const double a0 = M.va[e], v0 = nc_operand<MODE>(v, M.ci[e], beta, two, b0);
            s = fma(a0, v0, s);
            if (ABS) sa = fma(fabs(a0), b0, sa);
        }
        s = group_sum(s, g);
        if (ABS) sa = group_sum(sa, g);
        if (!segment) {
            if (live && sub == 0) nc_row<MODE>(v, row, s, sa, beta, two, acc);
        } else if (lane == 0) {                                    // the last segment of the row to arrive folds it: nothing waits
            M.seg[w.d] = s;
            if (ABS) M.seg2[w.d] = sa;
            const int kf = M.segk[w.d], p0 = M.fptr[kf], p1 = M.fptr[kf + 1];
            __threadfence();
            const int arrived = atomicAdd(&M.cnt[kf], 1);
            if (arrived == p1 - p0 - 1) {
                __threadfence();
                double fs = 0.0, fa = 0.0, f[NC_NSUM] = {0.0, 0.0, 0.0, 0.0};
                for (int p = p0; p < p1; ++p) { fs += ((const volatile double*)M.seg)[p]; if (ABS) fa += ((const volatile double*)M.seg2)[p]; }
                M.cnt[kf] = 0;
                nc_row<MODE>(v, row, fs, fa, beta, two, f);
#pragma unroll
                for (int j = 0; j < NS; ++j) M.fsum[(size_t)j * M.nfold + kf] = f[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double tot = nc_block_sum(acc[j], sh);
        if (threadIdx.x == 0) part[(size_t)j * NC_PARTS + blockIdx.x] = tot;
    }
}

// measurement only (FOS_NC_UNFUSED=1): the head of the first launch and p_k = z + beta p_k-1 in a launch of their own; the passes behind it then gather ONE operand
// (they run with z = p_k and k = 0) -- the unfused iteration the two- and three-launch ones are timed against
__global__ __launch_bounds__(NC_T) void nc_pvec_kernel(int64_t n, NcVec v, NcSum prev, NcState* __restrict__ st, int k, int maxit) {
    __shared__ double sh[NC_W];
    __shared__ int gate;
    if (nc_gate(st, &gate)) return;
    double beta = 0.0;
    if (k > 0) {
        const double rr = nc_total(prev, 1, sh);
        const bool stop = nc_stop(rr, st->tol_in, k, maxit);
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->rr = rr; if (stop) st->done = 1; }
        if (stop) return;
        const double rz = nc_total(prev, 0, sh);
        beta = rz / st->rz[(k - 1) & 1];
        if (blockIdx.x == 0 && threadIdx.x == 0) st->rz[k & 1] = rz;
    }
    for (int64_t i = (int64_t)blockIdx.x * NC_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * NC_T) v.pnew[i] = nc_p(v, i, beta, k > 0);
}

// closes iteration k: alpha = rz_k / p'M p with p'M p = sum p w (Quadratic: ls == 0), |p|^2 + lambda |A p|^2 (ls == 1: the unfused LeastSquares) or the merged
// recurrence's (ls == 2: sm = r'z and |z|^2, sa = |A z|^2; p and s advanced here);  y, r, z;  the sums r z and r r
__global__ __launch_bounds__(NC_T) void nc_update_kernel(int64_t n, NcVec v, int ls, NcSum sm, NcSum sa, double* __restrict__ part, NcState* __restrict__ st, int k) {
    __shared__ double sh[NC_W];
    __shared__ int gate;
    if (nc_gate(st, &gate)) return;
    double pmp = nc_total(sm, 0, sh), beta = 0.0, rz = 0.0;
    if (ls == 1) pmp = fma(v.lambda, nc_total(sa, 0, sh), pmp);
    if (ls == 2) { rz = pmp; pmp = nc_merged_pmp(st, k, rz, fma(v.lambda, nc_total(sa, 0, sh), nc_total(sm, 1, sh)), &beta); }
    else rz = st->rz[k & 1];
    if (!(pmp > 0.0)) {                                            // (every workgroup returns: see nc_pass_kernel)
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->pmp = pmp; st->flag = ls == 2 ? 2 : 1; st->done = 1; }
        return;
    }
    const double alpha = rz / pmp;
    double f[2] = {0.0, 0.0};
    if (ls == 2) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->rz[k & 1] = rz; st->alpha[k & 1] = alpha; }
        for (int64_t i = (int64_t)blockIdx.x * NC_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * NC_T) nc_update_merged(v, i, alpha, beta, k > 0, f);
    } else
        for (int64_t i = (int64_t)blockIdx.x * NC_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * NC_T) nc_update(v, i, alpha, f);
    for (int j = 0; j < 2; ++j) {
        const double tot = nc_block_sum(f[j], sh);
        if (threadIdx.x == 0) part[(size_t)j * NC_PARTS + blockIdx.x] = tot;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->iter = k + 1;
}

// behind a true residual (one workgroup): the scalars of a (re)start
__global__ __launch_bounds__(NC_T) void nc_start_kernel(NcSum q, NcState* __restrict__ st, double tol) {
    __shared__ double sh[NC_W];
    const double rr = nc_total(q, 0, sh), rz = nc_total(q, 1, sh), lev2 = nc_total(q, 2, sh), b2 = nc_total(q, 3, sh);
    if (threadIdx.x == 0) nc_start_scalars(st, rr, rz, lev2, b2, tol);
}
// a cold start: y = D^-1 (x + c)
__global__ __launch_bounds__(NC_T) void nc_cold_kernel(int64_t n, NcVec v) {
    for (int64_t i = (int64_t)blockIdx.x * NC_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * NC_T) v.y[i] = v.dinv[i] * (v.x[i] + v.c[i]);
}

// ------------------------------------------------------------------------------------------------ host: validation, the matrices, the plans
// the plan of one matrix and what the device (or the emulation) needs beside it
struct NcPlan {
    SfPass P;
    std::vector<int32_t> segk;
    int grid = 1;
    void build(int64_t nrows, const HostCsr& A, bool lpr) {
        if (!lpr) sf_plan_pass(nrows, A.rp.data(), SF_SEG_DEFAULT, &P);
        else {                                // measurement only: lanes_per_row (sparse_rows.hpp) -- every row the same g, no row cut
            P = SfPass();
            P.fptr.assign(1, 0);
            const int g = lanes_per_row(A.rp[(size_t)nrows], nrows);
            for (int64_t r = 0; r < nrows; r += 64 / g) P.items.push_back(SfItem{(int32_t)r, (int32_t)std::min<int64_t>(64 / g, nrows - r), -g, -1});
        }
        segk.assign((size_t)P.nparts, 0);
        for (size_t kf = 0; kf + 1 < P.fptr.size(); ++kf) for (int32_t p = P.fptr[kf]; p < P.fptr[kf + 1]; ++p) segk[(size_t)p] = (int32_t)kf;
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(NC_PARTS, ((int64_t)P.items.size() + NC_W - 1) / NC_W));
    }
};
// the two measurement switches, read at every set-up (per handle), for tools/nspace_cg_bench.py: FOS_NC_ROWS=lpr plans the rows as lanes_per_row does,
// FOS_NC_UNFUSED=1 forms p in a launch of its own (three launches for a Quadratic, the same bits; four for a LeastSquares, which then runs the plain recurrence
// with p'M p = |p|^2 + lambda |A p|^2 from its own sums: the same answer at the same bar, other roundings).
bool nc_env_is(const char* name, const char* value) { const char* s = std::getenv(name); return s && std::string(s) == value; }
struct NcHost {                               // what a set-up leaves on the host
    int64_t n = 0, m = 0;                     // m = 0: Quadratic
    double lambda = 1.0;
    HostCsr M, A;                             // Quadratic: M = I + Q;  LeastSquares: M = A' (n rows), A (m rows)
    NcPlan pm, pa;
    std::vector<double> dinv, c, b;           // c: Quadratic only (LeastSquares forms it with a pass)
    int64_t stored = 0;
    int longest = 0;
    bool lpr = nc_env_is("FOS_NC_ROWS", "lpr");
};
int nc_grid_n(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(NC_PARTS, (n + NC_T - 1) / NC_T)); }
constexpr CscRules NC_RULES{false, true, CSC_BOUND_BOTH, "the matrix"};
int nc_check_tol(const char* what, double tol) {
    if (!(tol >= 0.0) || tol >= 1.0) { set_error("%s: tol must be in [0, 1)", what); return FOS_EINVAL; }
    return FOS_OK;
}

int nc_host_quadratic(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol, NcHost* H) {
    const char* what = "Quadratic (cg)";
    FOS_TRY(nc_check_tol(what, tol));
    FOS_TRY(csc_check(what, n, n, colptr, rowval, nzval, NC_RULES));
    if (!q) { set_error("%s: bad argument", what); return FOS_EINVAL; }
    for (int64_t i = 0; i < n; ++i) if (!csc_finite(q[i])) { set_error("%s: q has non-finite entries", what); return FOS_EINVAL; }
    H->n = n; H->m = 0; H->lambda = 1.0;
    // rows of M = I + Q from the entries i >= j: row i takes (i, j), j < i, in column order, its diagonal, then the mirrors of column i: columns ascending
    std::vector<int64_t> cnt((size_t)n + 1, 0);
    std::vector<double> diag((size_t)n, 1.0);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t e = colptr[j] - 1; e < colptr[j + 1] - 1; ++e) {
            const int64_t i = rowval[e] - 1;
            if (i > j) { cnt[(size_t)i + 1]++; cnt[(size_t)j + 1]++; }
            else if (i == j) diag[(size_t)j] = 1.0 + nzval[e];
        }
    for (int64_t i = 0; i < n; ++i) {
        if (!(diag[(size_t)i] > 0.0) || !csc_finite(diag[(size_t)i])) {
            set_error("%s: 1 + Q[%lld, %lld] = %g is not a positive finite number (Q is not positive semidefinite)", what, (long long)i + 1, (long long)i + 1, diag[(size_t)i]);
            return FOS_EINVAL;
        }
        cnt[(size_t)i + 1] += 1 + cnt[(size_t)i];
    }
    if (cnt[(size_t)n] > 2000000000LL) { set_error("%s: I + Q has %lld stored entries (up to 2e9 supported)", what, (long long)cnt[(size_t)n]); return FOS_EINVAL; }
    HostCsr& M = H->M;
    M.rp.resize((size_t)n + 1); M.ci.resize((size_t)cnt[(size_t)n]); M.va.resize((size_t)cnt[(size_t)n]);
    for (int64_t i = 0; i <= n; ++i) M.rp[(size_t)i] = (int32_t)cnt[(size_t)i];
    std::vector<int32_t> fill(M.rp.begin(), M.rp.end() - 1);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t e = colptr[j] - 1; e < colptr[j + 1] - 1; ++e) {
            const int64_t i = rowval[e] - 1;
            if (i > j) { const int32_t p = fill[(size_t)i]++; M.ci[(size_t)p] = (int32_t)j; M.va[(size_t)p] = nzval[e]; }
        }
    for (int64_t j = 0; j < n; ++j) {
        int32_t p = fill[(size_t)j]++;
        M.ci[(size_t)p] = (int32_t)j; M.va[(size_t)p] = diag[(size_t)j];
        for (int64_t e = colptr[j] - 1; e < colptr[j + 1] - 1; ++e) {
            const int64_t i = rowval[e] - 1;
            if (i > j) { p = fill[(size_t)j]++; M.ci[(size_t)p] = (int32_t)i; M.va[(size_t)p] = nzval[e]; }
        }
    }
    H->dinv.resize((size_t)n); H->c.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) { H->dinv[(size_t)i] = 1.0 / diag[(size_t)i]; H->c[(size_t)i] = -q[i]; }
    H->pm.build(n, M, H->lpr);
    H->stored = cnt[(size_t)n]; H->longest = M.longest();
    return FOS_OK;
}
int nc_host_ls(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, double tol, NcHost* H) {
    const char* what = "LeastSquares (cg)";
    if (!(lambda > 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    FOS_TRY(nc_check_tol(what, tol));
    FOS_TRY(csc_check(what, m, n, colptr, rowval, nzval, NC_RULES));
    if (!b) { set_error("%s: bad argument", what); return FOS_EINVAL; }
    for (int64_t i = 0; i < m; ++i) if (!csc_finite(b[i])) { set_error("%s: b has non-finite entries", what); return FOS_EINVAL; }
    H->n = n; H->m = m; H->lambda = lambda;
    HostCsr &T = H->M, &A = H->A;                                 // T = A' (n rows)
    csc_to_csr_pair(m, n, colptr, rowval, nzval, nullptr, &A, &T);
    H->dinv.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        double d = 0.0;
        for (int32_t e = T.rp[(size_t)j]; e < T.rp[(size_t)j + 1]; ++e) d += T.va[(size_t)e] * T.va[(size_t)e];
        const double dj = 1.0 + lambda * d;
        if (!csc_finite(dj)) { set_error("%s: 1 + lambda |A[:, %lld]|^2 overflows", what, (long long)j + 1); return FOS_EINVAL; }
        H->dinv[(size_t)j] = 1.0 / dj;
    }
    H->b.assign(b, b + m);
    H->pm.build(n, T, H->lpr); H->pa.build(m, A, H->lpr);
    H->stored = 2 * (int64_t)T.ci.size(); H->longest = T.longest() + A.longest();
    return FOS_OK;
}

}  // namespace

struct NSpaceCG : ProxObject, DevOwned {
    NSpaceCG() : ProxObject(FEAS_NSPACE_CG) {}
    ~NSpaceCG() override { if (st_host) (void)hipHostFree(st_host); }
    int prox(hipStream_t stream, double* y, const double* x) override;
    void reset(hipStream_t) override { cold = true; }             // a new solve: the next prox starts from D^-1 (x + c)
    int64_t n = 0, m = 0, stored = 0;                             // m = 0: Quadratic
    double tol = 0.0;
    bool cold = true, unfused = nc_env_is("FOS_NC_UNFUSED", "1");
    NcMat M, A;                                                   // M: I + Q or A';  A: LeastSquares only
    NcVec v{};                                                    // x is set per prox
    double *pb[2] = {nullptr, nullptr}, *part = nullptr;
    NcState *st = nullptr, *st_host = nullptr;
    int grid_n = 1;
    // statistics (fos_feas_nspace_cg_stats)
    int64_t calls = 0, iters_total = 0;
    int last_iters = 0, last_rounds = 0;
    double last_resid = 0.0, last_level = 0.0;
};

namespace {

int nc_upload_mat(NSpaceCG* a, hipStream_t s, const HostCsr& C, const NcPlan& pl, NcMat* D) {
    DevCsr c;
    DevPass p;                                                    // (its part[] is seg: a slot per segment)
    int32_t* segk = nullptr;
    FOS_TRY(p.upload(*a, pl.P, s)); FOS_TRY(c.upload(*a, C, s)); FOS_TRY(a->upload(&segk, pl.segk, s));
    D->nitems = p.nitems; D->nfold = p.nfold; D->grid = pl.grid;
    D->items = p.items; D->rp = c.rp; D->ci = c.ci; D->va = c.va; D->fptr = p.fptr; D->segk = segk; D->seg = p.part;
    FOS_TRY(a->zeros(&D->cnt, (size_t)D->nfold, s));
    FOS_TRY(a->zeros(&D->seg2, (size_t)pl.P.nparts, s));
    FOS_TRY(a->zeros(&D->fsum, (size_t)NC_NSUM * (size_t)D->nfold, s));
    return FOS_OK;
}
template <int MODE>
void nc_launch_pass(hipStream_t s, const NcMat& M, const NcVec& v, double* part, const NcSum& prev, NcState* st, int k, int maxit) {
    hipLaunchKernelGGL((nc_pass_kernel<MODE>), dim3(M.grid), dim3(NC_T), 0, s, M, v, part, prev, st, k, maxit);
}
int nc_fill(NSpaceCG* a, const NcHost& H, double tol, hipStream_t stream) {
    a->n = H.n; a->m = H.m; a->stored = H.stored; a->tol = tol; a->grid_n = nc_grid_n(H.n);
    const size_t n = (size_t)H.n, m = (size_t)H.m;
    FOS_TRY(nc_upload_mat(a, stream, H.M, H.pm, &a->M));
    if (H.m) FOS_TRY(nc_upload_mat(a, stream, H.A, H.pa, &a->A));
    double *dinv = nullptr, *c = nullptr;
    FOS_TRY(a->upload(&dinv, H.dinv, stream));
    if (H.m) FOS_TRY(a->zeros(&c, n, stream)); else FOS_TRY(a->upload(&c, H.c, stream));
    NcVec& v = a->v;
    v.dinv = dinv; v.c = c; v.cw = c; v.lambda = H.lambda;
    for (double** p : {&v.y, &v.r, &v.z, &v.w, &a->pb[0], &a->pb[1]}) FOS_TRY(a->zeros(p, n, stream));
    for (double** p : {&v.t, &v.ta}) FOS_TRY(a->zeros(p, m, stream));
    FOS_TRY(a->zeros(&a->part, (size_t)NC_REGIONS * NC_PARTS, stream));
    FOS_TRY(a->zeros(&a->st, 1, stream));
    if (hipHostMalloc((void**)&a->st_host, sizeof(NcState), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_error("%s: hipHostMalloc failed", a->what); return FOS_ENOMEM; }
    if (H.m) {                                                     // c = lambda A'b (t holds b for this one pass)
        FOS_TRY(a->hip("hipMemcpyAsync", hipMemcpyAsync(v.t, H.b.data(), sizeof(double) * m, hipMemcpyHostToDevice, stream)));
        nc_launch_pass<NC_TC>(stream, a->M, v, a->part, NcSum{a->part, 0, a->part, 0}, a->st, 0, 0);
    }
    FOS_TRY(a->hip("hipStreamSynchronize", hipStreamSynchronize(stream)));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s set-up: a kernel launch failed: %s", a->what, hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}
int nc_setup(const char* what, const NcHost& H, double tol, hipStream_t stream, ProxObject** out) {
    NSpaceCG* a = new NSpaceCG();
    a->what = what;
    const int rc = nc_fill(a, H, tol, stream);
    if (rc != FOS_OK) { (void)hipStreamSynchronize(stream); delete a; return rc; }
    *out = a;
    return FOS_OK;
}

}  // namespace

// Quadratic(Q, q), Q sparse n x n (CSC, 1-based; the entries i >= j are read), q[n].  Synchronises `stream`.
int nspace_cg_setup_quadratic(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol, hipStream_t stream,
                              ProxObject** out) {
    NcHost H;
    FOS_TRY(nc_host_quadratic(n, colptr, rowval, nzval, q, tol, &H));
    return nc_setup("Quadratic (cg)", H, tol, stream, out);
}
// LeastSquares(A, b, lambda), A sparse m x n (CSC, 1-based), any m, n >= 1.  Synchronises `stream`.
int nspace_cg_setup_ls(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, double tol,
                       hipStream_t stream, ProxObject** out) {
    NcHost H;
    FOS_TRY(nc_host_ls(m, n, colptr, rowval, nzval, b, lambda, tol, &H));
    return nc_setup("LeastSquares (cg)", H, tol, stream, out);
}

// y = prox_f(x) (device vectors of at least n doubles, y must not alias x), on `stream`
int NSpaceCG::prox(hipStream_t stream, double* yout, const double* x) {
    NSpaceCG* a = this;
    const bool ls = a->m > 0;
    const int maxit = (int)std::min<int64_t>(20000, 2 * a->n + 100);
    NcVec v = a->v;
    v.x = x;
    double* const part = a->part;
    const NcSum none{part, 0, part, 0};
    const NcSum sum_a{part + (size_t)NC_R_A * NC_PARTS, a->A.grid, a->A.fsum, a->A.nfold};
    const NcSum sum_m{part + (size_t)NC_R_M * NC_PARTS, a->M.grid, a->M.fsum, a->M.nfold};
    const NcSum sum_u{part + (size_t)NC_R_U * NC_PARTS, a->grid_n, part, 0};
    int total = 0, round = 0;
    a->calls++;
    if (a->cold) hipLaunchKernelGGL(nc_cold_kernel, dim3(a->grid_n), dim3(NC_T), 0, stream, a->n, v);
    a->cold = true;                                               // (until this prox has ended well: a failed one leaves nothing to start from)
    for (;; ++round) {
        // r = x + c - M y, z = D^-1 r, the rounding level; the scalars of the (re)start
        if (ls) {
            nc_launch_pass<NC_ATR>(stream, a->A, v, part + (size_t)NC_R_A * NC_PARTS, none, a->st, 0, 0);
            nc_launch_pass<NC_TR>(stream, a->M, v, part + (size_t)NC_R_M * NC_PARTS, none, a->st, 0, 0);
        } else nc_launch_pass<NC_QR>(stream, a->M, v, part + (size_t)NC_R_M * NC_PARTS, none, a->st, 0, 0);
        hipLaunchKernelGGL(nc_start_kernel, dim3(1), dim3(NC_T), 0, stream, sum_m, a->st, a->tol);
        FOS_HIP(hipMemcpyAsync(a->st_host, a->st, sizeof(NcState), hipMemcpyDeviceToHost, stream));
        FOS_HIP(hipStreamSynchronize(stream));
        const double resid = std::sqrt(a->st_host->rr), level = std::sqrt(a->st_host->level2);
        a->last_resid = resid; a->last_level = level;
        if (!(resid == resid) || !(level == level)) { set_error("%s: the residual is NaN (non-finite input?)", a->what); return FOS_EINVAL; }
        if (a->st_host->done) break;                               // the true residual is at its level: y is the answer
        if (round >= NC_ROUNDS_MAX) {
            set_error("%s: |x + c - M y| = %.3e stays above %.3e after %d restarts and %d CG iterations", a->what, resid, a->st_host->tol_abs, round, total);
            return FOS_EINVAL;
        }
        for (int k = 0;;) {
            for (int q = 0; q < NC_BATCH; ++q, ++k) {
                const int flip = (ls && !a->unfused) ? 0 : (k & 1);        // (the merged recurrence keeps p in pb[1] and s = M p in pb[0], in place)
                v.pold = a->pb[flip]; v.pnew = a->pb[flip ^ 1];
                NcVec vp = v;
                int kp = k, kind = ls ? 2 : 0;
                if (a->unfused) {
                    hipLaunchKernelGGL(nc_pvec_kernel, dim3(a->grid_n), dim3(NC_T), 0, stream, a->n, v, sum_u, a->st, k, maxit);
                    vp.z = v.pnew; kp = 0; kind = ls ? 1 : 0;
                }
                if (ls) {
                    nc_launch_pass<NC_AT>(stream, a->A, vp, part + (size_t)NC_R_A * NC_PARTS, sum_u, a->st, kp, maxit);
                    if (a->unfused) nc_launch_pass<NC_TW>(stream, a->M, vp, part + (size_t)NC_R_M * NC_PARTS, sum_u, a->st, kp, maxit);
                    else nc_launch_pass<NC_TG>(stream, a->M, vp, part + (size_t)NC_R_M * NC_PARTS, sum_u, a->st, kp, maxit);
                } else nc_launch_pass<NC_QW>(stream, a->M, vp, part + (size_t)NC_R_M * NC_PARTS, sum_u, a->st, kp, maxit);
                hipLaunchKernelGGL(nc_update_kernel, dim3(a->grid_n), dim3(NC_T), 0, stream, a->n, v, kind, sum_m, sum_a, part + (size_t)NC_R_U * NC_PARTS, a->st, k);
            }
            FOS_HIP(hipMemcpyAsync(a->st_host, a->st, sizeof(NcState), hipMemcpyDeviceToHost, stream));
            FOS_HIP(hipStreamSynchronize(stream));
            if (a->st_host->done) break;
        }
        total += a->st_host->iter;
        if (a->st_host->flag == 1) {
            if (ls) set_error("%s: p'(I + lambda A'A) p = %g in CG (non-finite input?)", a->what, a->st_host->pmp);
            else set_error("%s: p'(I + Q) p = %g <= 0 in CG: Q is not positive semidefinite", a->what, a->st_host->pmp);
            return FOS_EINVAL;
        }
    }
    FOS_HIP(hipMemcpyAsync(yout, v.y, sizeof(double) * (size_t)a->n, hipMemcpyDeviceToDevice, stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: a kernel launch failed: %s", a->what, hipGetErrorString(e)); return FOS_EHIP; }
    a->cold = false;
    a->last_iters = total; a->last_rounds = round; a->iters_total += total;
    return FOS_OK;
}

// out8 = prox calls, CG iterations so far, CG iterations / restarts of the last prox, its |x + c - M y| and rounding level, stored entries, launches per CG iteration
void nspace_cg_stats(const ProxObject* obj, double* out8) {
    const NSpaceCG* a = static_cast<const NSpaceCG*>(obj);
    out8[0] = (double)a->calls; out8[1] = (double)a->iters_total; out8[2] = (double)a->last_iters; out8[3] = (double)a->last_rounds;
    out8[4] = a->last_resid; out8[5] = a->last_level; out8[6] = (double)a->stored; out8[7] = (a->m > 0 ? 3.0 : 2.0) + (a->unfused ? 1.0 : 0.0);
}

// ---------------------------------------------------------------------------------- host emulation (tests; no GPU)
namespace {

double nc_host_tree(const double* v, int g) { return g == 1 ? v[0] : nc_host_tree(v, g / 2) + nc_host_tree(v + g / 2, g / 2); }       // wave_sum / group_sum: pairs, quads, ...
// a workgroup's threads' accumulators -> its partial (nc_block_sum)
double nc_host_block(const double* acc) {
    double s = 0.0;
    for (int w = 0; w < NC_W; ++w) s += nc_host_tree(acc + 64 * w, 64);
    return s;
}
struct NcHostSum { std::vector<double> part, fsum; int nparts = 0, nfold = 0; };          // [NC_NSUM][nparts], [NC_NSUM][nfold]
double nc_host_total(const NcHostSum& q, int j) {
    double th[NC_T];
    for (int t = 0; t < NC_T; ++t) {
        double v = 0.0;
        for (int i = t; i < q.nparts; i += NC_T) v += q.part[(size_t)j * q.nparts + i];
        for (int i = t; i < q.nfold; i += NC_T) v += q.fsum[(size_t)j * q.nfold + i];
        th[t] = v;
    }
    return nc_host_block(th);
}
template <int MODE>
void nc_host_pass(const HostCsr& C, const NcPlan& pl, const NcVec& v, double beta, bool two, NcHostSum* out) {
    constexpr int NS = nc_nsum(MODE);
    constexpr bool ABS = nc_abs(MODE);
    const int nitems = (int)pl.P.items.size(), grid = pl.grid, nfold = (int)pl.P.frow.size();
    out->nparts = grid; out->nfold = nfold;
    out->part.assign((size_t)NC_NSUM * grid, 0.0); out->fsum.assign((size_t)NC_NSUM * std::max(nfold, 1), 0.0);
    std::vector<double> seg((size_t)pl.P.nparts, 0.0), seg2((size_t)pl.P.nparts, 0.0);
    std::vector<int> cnt((size_t)nfold, 0);
    const int per = (nitems + grid - 1) / grid;
    for (int blk = 0; blk < grid; ++blk) {
        double acc[NC_NSUM][NC_T] = {};
        const int i0 = blk * per, i1 = std::min(nitems, i0 + per);
        for (int it = i0; it < i1; ++it) {
            const int wv = (it - i0) % NC_W;
            const SfItem w = pl.P.items[(size_t)it];
            const bool segment = w.c > 0;
            const int g = segment ? 64 : -w.c, rows = segment ? 1 : w.b;
            for (int kk = 0; kk < rows; ++kk) {
                const int row = w.a + kk;
                const int e0 = segment ? w.b : C.rp[(size_t)row], e1 = segment ? w.b + w.c : C.rp[(size_t)row + 1];
                double ls[64] = {}, la[64] = {};
                for (int sub = 0; sub < g; ++sub)
                    for (int e = e0 + sub; e < e1; e += g) {
                        double av = 0.0;
                        const double a0 = C.va[(size_t)e], v0 = nc_operand<MODE>(v, C.ci[(size_t)e], beta, two, av);
                        ls[sub] = std::fma(a0, v0, ls[sub]);
                        if (ABS) la[sub] = std::fma(std::fabs(a0), av, la[sub]);
                    }
                const double s = nc_host_tree(ls, g), sa = ABS ? nc_host_tree(la, g) : 0.0;
                if (!segment) {
                    double f[NC_NSUM] = {0.0, 0.0, 0.0, 0.0};
                    for (int j = 0; j < NS; ++j) f[j] = acc[j][64 * wv + kk * g];
                    nc_row<MODE>(v, row, s, sa, beta, two, f);
                    for (int j = 0; j < NS; ++j) acc[j][64 * wv + kk * g] = f[j];
                } else {
                    seg[(size_t)w.d] = s; seg2[(size_t)w.d] = sa;
                    const int kf = pl.segk[(size_t)w.d], p0 = pl.P.fptr[(size_t)kf], p1 = pl.P.fptr[(size_t)kf + 1];
                    if (++cnt[(size_t)kf] == p1 - p0) {
                        double fs = 0.0, fa = 0.0, f[NC_NSUM] = {0.0, 0.0, 0.0, 0.0};
                        for (int p = p0; p < p1; ++p) { fs += seg[(size_t)p]; if (ABS) fa += seg2[(size_t)p]; }
                        nc_row<MODE>(v, row, fs, fa, beta, two, f);
                        for (int j = 0; j < NS; ++j) out->fsum[(size_t)j * nfold + kf] = f[j];
                    }
                }
            }
        }
        for (int j = 0; j < NS; ++j) out->part[(size_t)j * grid + blk] = nc_host_block(acc[j]);
    }
}
// the prox of NSpaceCG::prox from a cold start, on the host
int nc_host_prox(const char* what, NcHost& H, double tol, const double* x, double* yout, int32_t* iters) {
    const int64_t n = H.n, m = H.m;
    const bool ls = m > 0;
    const int maxit = (int)std::min<int64_t>(20000, 2 * n + 100), grid_n = nc_grid_n(n);
    std::vector<double> y((size_t)n), r((size_t)n), z((size_t)n), w((size_t)n), p0((size_t)n, 0.0), p1((size_t)n, 0.0), t((size_t)std::max<int64_t>(m, 1)), ta((size_t)std::max<int64_t>(m, 1));
    std::vector<double> c = H.c;
    double* pb[2] = {p0.data(), p1.data()};
    NcVec v{};
    v.x = x; v.dinv = H.dinv.data(); v.lambda = H.lambda;
    v.y = y.data(); v.r = r.data(); v.z = z.data(); v.w = w.data(); v.t = t.data(); v.ta = ta.data();
    NcHostSum sa, sm, su;
    if (ls) {                                                      // c = lambda A'b
        c.assign((size_t)n, 0.0);
        v.cw = c.data();
        std::copy(H.b.begin(), H.b.end(), t.begin());
        nc_host_pass<NC_TC>(H.M, H.pm, v, 0.0, false, &sm);
    }
    v.c = c.data();
    for (int64_t i = 0; i < n; ++i) y[(size_t)i] = v.dinv[i] * (x[i] + v.c[i]);
    NcState st{};
    int total = 0;
    for (int round = 0;; ++round) {
        if (ls) { nc_host_pass<NC_ATR>(H.A, H.pa, v, 0.0, false, &sa); nc_host_pass<NC_TR>(H.M, H.pm, v, 0.0, false, &sm); }
        else nc_host_pass<NC_QR>(H.M, H.pm, v, 0.0, false, &sm);
        nc_start_scalars(&st, nc_host_total(sm, 0), nc_host_total(sm, 1), nc_host_total(sm, 2), nc_host_total(sm, 3), tol);
        if (!(st.rr == st.rr) || !(st.level2 == st.level2)) { set_error("%s: the residual is NaN (non-finite input?)", what); return FOS_EINVAL; }
        if (st.done) break;
        if (round >= NC_ROUNDS_MAX) {
            set_error("%s: |x + c - M y| = %.3e stays above %.3e after %d restarts and %d CG iterations", what, std::sqrt(st.rr), st.tol_abs, round, total);
            return FOS_EINVAL;
        }
        for (int k = 0; !st.done; ++k) {
            const bool two = k > 0;
            double beta = 0.0;
            if (two) {
                const double rr = nc_host_total(su, 1);
                st.rr = rr;
                if (nc_stop(rr, st.tol_in, k, maxit)) { st.done = 1; break; }
                if (!ls) {
                    const double rz = nc_host_total(su, 0);
                    beta = rz / st.rz[(k - 1) & 1];
                    st.rz[k & 1] = rz;
                }
            }
            const int flip = ls ? 0 : (k & 1);
            v.pold = pb[flip]; v.pnew = pb[flip ^ 1];
            double pmp, alpha;
            if (ls) {                                              // the merged recurrence
                nc_host_pass<NC_AT>(H.A, H.pa, v, 0.0, false, &sa);
                nc_host_pass<NC_TG>(H.M, H.pm, v, 0.0, false, &sm);
                const double rz = nc_host_total(sm, 0);
                pmp = nc_merged_pmp(&st, k, rz, std::fma(v.lambda, nc_host_total(sa, 0), nc_host_total(sm, 1)), &beta);
                if (!(pmp > 0.0)) { st.done = 1; break; }         // (rounding: the residual is recomputed and CG starts again)
                alpha = rz / pmp;
                st.rz[k & 1] = rz; st.alpha[k & 1] = alpha;
            } else {
                nc_host_pass<NC_QW>(H.M, H.pm, v, beta, two, &sm);
                pmp = nc_host_total(sm, 0);
                if (!(pmp > 0.0)) { set_error("%s: p'(I + Q) p = %g <= 0 in CG: Q is not positive semidefinite", what, pmp); return FOS_EINVAL; }
                alpha = st.rz[k & 1] / pmp;
            }
            su.nparts = grid_n; su.nfold = 0; su.part.assign((size_t)2 * grid_n, 0.0); su.fsum.assign(1, 0.0);
            for (int blk = 0; blk < grid_n; ++blk) {
                double acc[2][NC_T] = {};
                for (int tt = 0; tt < NC_T; ++tt) {
                    double f[2] = {0.0, 0.0};
                    for (int64_t i = (int64_t)blk * NC_T + tt; i < n; i += (int64_t)grid_n * NC_T) {
                        if (ls) nc_update_merged(v, i, alpha, beta, two, f);
                        else nc_update(v, i, alpha, f);
                    }
                    acc[0][tt] = f[0]; acc[1][tt] = f[1];
                }
                for (int j = 0; j < 2; ++j) su.part[(size_t)j * grid_n + blk] = nc_host_block(acc[j]);
            }
            st.iter = k + 1;
        }
        total += st.iter;
    }
    std::copy(y.begin(), y.end(), yout);
    if (iters) *iters = total;
    return FOS_OK;
}

}  // namespace

int host_nspace_cg_quadratic(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol, const double* x, double* y,
                             int32_t* iters) {
    NcHost H;
    FOS_TRY(nc_host_quadratic(n, colptr, rowval, nzval, q, tol, &H));
    if (!x || !y) { set_error("Quadratic (cg): bad argument"); return FOS_EINVAL; }
    return nc_host_prox("Quadratic (cg)", H, tol, x, y, iters);
}
int host_nspace_cg_ls(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, double tol,
                      const double* x, double* y, int32_t* iters) {
    NcHost H;
    FOS_TRY(nc_host_ls(m, n, colptr, rowval, nzval, b, lambda, tol, &H));
    if (!x || !y) { set_error("LeastSquares (cg): bad argument"); return FOS_EINVAL; }
    return nc_host_prox("LeastSquares (cg)", H, tol, x, y, iters);
}

}  // namespace fos
