// IndAffine(A, b) with a DENSE A on the device, factored form: the exact projection  y = x - A'(A A')^-1 (A x - b)  evaluated as written -- two passes over A
// and an inverse of order m -- instead of the n x n projector of fos_feas_set_affine.  For the wide sets users intersect (m << n) that is 16 m n + O(m^2)
// bytes per projection instead of 8 n^2, no limit on n, and a set-up that inverts A A' (order m), not an n x n matrix.
//
//   * set-up: the rows of [A | b] are scaled to unit norm (the set does not change; G = A A' gets a unit diagonal); the scaled A is kept ONCE, row-major with
//     the leading dimension ld = n rounded up to 64 doubles, zero filled (every row starts 16-byte aligned, the kernels need no tail case); G = A A' by
//     gram_rows_kernel (dense_chol.hip), X = G^-1 by dense_spd_inverse (direct.cpp: blocked Cholesky, probe, polish, or Newton-Schulz).  The inverse is
//     accepted at a probe residual of DA_BAR, not the 1e-12 of direct = true: there the matrix is I + Q Q' (lambda_min >= 1), here cond(G) = cond(A)^2 and an
//     explicit fp64 inverse cannot do better than ~cond(G) eps (6e-10 at cond 2e7, a square Gaussian A of order 500).  The projection does not need more:
//   * a projection:  r = A x - b (pass 1);  d = X r;  d += X (r - G d) -- one correction step in the m-space, its error (I - X G)^2 G^-1 r, which squares what
//     the explicit inverse left (DA_BAR^2 = 1e-14 at worst) without touching A;  y = x - A'd (pass 2);  then `refine` times  r = A y - b, d = X r, y -= A'd.
//     A fixed number of launches, no host synchronise, no copy.
//   * pass 1 (da_rows_kernel): a wavefront takes DA_RG rows x one span of columns, 16 bytes per lane per row step (non-temporal), one accumulator per row in
//     the lane, one crossing of the lanes per row at the end of the span; partial[span][row], folded in index order by da_rows_fold_kernel.
//   * pass 2 (da_cols_kernel): a lane owns two adjacent columns and walks the rows of its row block with d in LDS; with one row block it writes x - sum itself,
//     otherwise partial[rowblock][column], folded in index order by da_cols_fold_kernel.
//   A is read exactly once per pass; nothing is atomic; every sum has a fixed order: the same input gives the same bits.
//
// LeastSquares(A, b, lambda), f(x) = lambda/2 |A x - b|^2, is the same object with a shifted G: prox_f(x) = x - A'(A A' + I/lambda)^-1 (A x - b) (from
// lambda A'(A y - b) + y - x = 0 with y = x - A'u), with the rows scaled by D:  x - Ah'(Ah Ah' + D^2/lambda)^-1 (Ah x - D b).  The set-up adds scale[i]^2 / lambda
// to the diagonal of G (da_shift_diag_kernel) and everything after it is unchanged; refine is 0 (its steps assume A y = b), a zero row keeps scale 1 and a
// rank-deficient A is accepted (the shifted G is positive definite).  lambda = 0 is IndAffine, to the bit.
#include "fos_solver.hpp"
#include "dev_common.hpp"

#include <cmath>
#include <vector>

namespace fos {

namespace {

constexpr int DA_T = 256;                     // threads per workgroup
constexpr int DA_RG = 8;                      // pass 1: rows per wavefront
constexpr int DA_STEP = 128;                  // pass 1: columns per wavefront step (64 lanes x 2 doubles)
constexpr int DA_SPAN_MIN = 512;              // pass 1: shortest span (4 steps per lane-crossing)
constexpr int DA_CB = 2 * DA_T;               // pass 2: columns per workgroup
constexpr int DA_DCH = 1024;                  // pass 2: entries of d staged in LDS at a time
constexpr int DA_ROWS_MIN = 32;               // pass 2: fewest rows of a row block (a partial slice costs 16 bytes per column: <= 1/16 of the block's bytes of A)
constexpr double DA_BAR = 1e-7;               // the inverse of A A' is accepted at this residual (see above)
typedef double da_v2d __attribute__((ext_vector_type(2)));

// pass 1: part[s * Lm + row] = sum over the columns of span s of A[row, c] x[c]
__global__ __launch_bounds__(DA_T) void da_rows_kernel(int64_t m, int64_t n, int64_t ld, int64_t Lm, int64_t span, int64_t ngroups, int64_t nunits,
                                                       const double* __restrict__ A, const double* __restrict__ x, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * (DA_T / 64) + (threadIdx.x >> 6);      // the wavefronts of a workgroup: the same span, neighbouring row groups
    if (unit >= nunits) return;
    const int64_t s = unit / ngroups, row0 = (unit % ngroups) * DA_RG;
    const int64_t c0 = s * span, c1 = c0 + span < ld ? c0 + span : ld;
    const double* __restrict__ a0 = A + row0 * ld;
    double acc[DA_RG];
#pragma unroll
    for (int q = 0; q < DA_RG; ++q) acc[q] = 0.0;
    for (int64_t c = c0 + 2 * lane; c < c1; c += DA_STEP) {                          // (c is even and ld a multiple of 64: c + 1 < ld)
        da_v2d xv = {0.0, 0.0};
        if (c + 1 < n) xv = *reinterpret_cast<const da_v2d*>(x + c);
        else if (c < n) xv.x = x[c];
        da_v2d a[DA_RG];
#pragma unroll
        for (int q = 0; q < DA_RG; ++q) {
            a[q] = da_v2d{0.0, 0.0};
            if (row0 + q < m) a[q] = __builtin_nontemporal_load(reinterpret_cast<const da_v2d*>(a0 + q * ld + c));
        }
#pragma unroll
        for (int q = 0; q < DA_RG; ++q) acc[q] += a[q].x * xv.x + a[q].y * xv.y;
    }
#pragma unroll
    for (int q = 0; q < DA_RG; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0 && row0 + q < m) part[s * Lm + row0 + q] = v;
    }
}
// r = sum_s part[s] - b, the spans in index order
__global__ __launch_bounds__(DA_T) void da_rows_fold_kernel(int64_t m, int64_t Lm, int nspan, const double* __restrict__ part, const double* __restrict__ b,
                                                            double* __restrict__ r) {
    for (int64_t i = blockIdx.x * (int64_t)DA_T + threadIdx.x; i < m; i += (int64_t)gridDim.x * DA_T) {
        double s = 0.0;
        for (int k = 0; k < nspan; ++k) s += part[(int64_t)k * Lm + i];
        r[i] = s - b[i];
    }
}
// the m-space: out = add + sign M v for a symmetric column-major M of order l (add == nullptr: 0); one wavefront per column as dense_symv_kernel (vecops.hip).
// out may be add (the lane that writes out[col] is the one that read add[col]).
__global__ __launch_bounds__(DA_T) void da_symv_kernel(int64_t l, int64_t ld, const double* __restrict__ M, const double* __restrict__ v, const double* add, double sign,
                                                       double* out) {
    const int lane = threadIdx.x & 63;
    const int64_t col = blockIdx.x * (int64_t)(DA_T / 64) + (threadIdx.x >> 6);
    if (col >= l) return;
    const da_v2d* __restrict__ g2 = reinterpret_cast<const da_v2d*>(M + col * ld);
    const int64_t npair = l / 2;
    double acc = 0.0;
    for (int64_t q = lane; q < npair; q += 64) {
        const da_v2d a = __builtin_nontemporal_load(g2 + q);
        acc += a.x * v[2 * q] + a.y * v[2 * q + 1];
    }
    if (lane == 0 && 2 * npair < l) acc += M[col * ld + l - 1] * v[l - 1];
    acc = wave_sum(acc);
    if (lane == 0) out[col] = (add ? add[col] : 0.0) + sign * acc;
}
// pass 2: the columns [512 blockIdx.x, + 512) over the rows of row block blockIdx.y:  s[c] = sum_i A[i, c] d[i], rows ascending.
// direct: y[c] = x[c] - s[c] (one row block; y may be x: every entry is read and written by the same lane); otherwise part[blockIdx.y * ld + c] = s[c].
__global__ __launch_bounds__(DA_T) void da_cols_kernel(int64_t m, int64_t n, int64_t ld, int64_t rows_blk, int direct, const double* __restrict__ A,
                                                       const double* __restrict__ d, const double* x, double* y, double* __restrict__ part) {
    __shared__ double ds[DA_DCH];
    const int64_t c = ((int64_t)blockIdx.x * DA_T + threadIdx.x) * 2;
    const int64_t r0 = (int64_t)blockIdx.y * rows_blk, r1 = r0 + rows_blk < m ? r0 + rows_blk : m;
    const bool live = c < ld;                                                        // (c even, ld a multiple of 64: c + 1 < ld too)
    double s0 = 0.0, s1 = 0.0;
    for (int64_t rc = r0; rc < r1; rc += DA_DCH) {
        const int cnt = (int)(r1 - rc < DA_DCH ? r1 - rc : DA_DCH);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += DA_T) ds[k] = d[rc + k];
        __syncthreads();
        if (live) {
            const double* __restrict__ ap = A + rc * ld + c;
            int k = 0;
            for (; k + 8 <= cnt; k += 8) {
                da_v2d a[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) a[q] = __builtin_nontemporal_load(reinterpret_cast<const da_v2d*>(ap + (int64_t)(k + q) * ld));
#pragma unroll
                for (int q = 0; q < 8; ++q) { const double dv = ds[k + q]; s0 += a[q].x * dv; s1 += a[q].y * dv; }
            }
            for (; k < cnt; ++k) {
                const da_v2d a = __builtin_nontemporal_load(reinterpret_cast<const da_v2d*>(ap + (int64_t)k * ld));
                const double dv = ds[k];
                s0 += a.x * dv; s1 += a.y * dv;
            }
        }
    }
    if (!live) return;
    if (direct) {
        if (c < n) y[c] = x[c] - s0;
        if (c + 1 < n) y[c + 1] = x[c + 1] - s1;
    } else {
        *reinterpret_cast<da_v2d*>(part + (int64_t)blockIdx.y * ld + c) = da_v2d{s0, s1};
    }
}
// y = x - sum_k part[k], the row blocks in index order (y may be x)
__global__ __launch_bounds__(DA_T) void da_cols_fold_kernel(int64_t n, int64_t ld, int nrb, const double* __restrict__ part, const double* x, double* y) {
    for (int64_t c = blockIdx.x * (int64_t)DA_T + threadIdx.x; c < n; c += (int64_t)gridDim.x * DA_T) {
        double s = 0.0;
        for (int k = 0; k < nrb; ++k) s += part[(int64_t)k * ld + c];
        y[c] = x[c] - s;
    }
}
// set-up: row i of the zero-padded row-major A times scale[i]
__global__ __launch_bounds__(DA_T) void da_scale_rows_kernel(int64_t m, int64_t ld, double* __restrict__ A, const double* __restrict__ scale) {
    for (int64_t e = blockIdx.x * (int64_t)DA_T + threadIdx.x; e < m * ld; e += (int64_t)gridDim.x * DA_T) A[e] *= scale[e / ld];
}

// set-up of LeastSquares: G[i, i] += scale[i]^2 / lambda
__global__ __launch_bounds__(DA_T) void da_shift_diag_kernel(int64_t m, int64_t Lm, double* __restrict__ G, const double* __restrict__ scale, double inv_lambda) {
    for (int64_t i = blockIdx.x * (int64_t)DA_T + threadIdx.x; i < m; i += (int64_t)gridDim.x * DA_T) G[i + i * Lm] += scale[i] * scale[i] * inv_lambda;
}

// how the two passes are split, from m, n and the CU count alone
struct DaPlan {
    int64_t ld = 0, Lm = 0;
    int64_t span = 0, ngroups = 0;            // pass 1: columns per span, row groups
    int nspan = 1;
    int64_t rows_blk = 0;                     // pass 2: rows per row block
    int nrb = 1;
};
DaPlan da_plan(int64_t m, int64_t n, int cus) {
    DaPlan p;
    p.ld = (n + 63) / 64 * 64; p.Lm = (m + 63) / 64 * 64;
    p.ngroups = (m + DA_RG - 1) / DA_RG;
    const int64_t waves = 8 * (int64_t)std::max(1, cus);                               // pass 1: about eight wavefronts per CU, when the spans allow it
    const int64_t want = std::max<int64_t>(1, waves / p.ngroups);
    p.span = std::max<int64_t>(DA_SPAN_MIN, ((p.ld + want - 1) / want + DA_STEP - 1) / DA_STEP * DA_STEP);
    p.nspan = (int)((p.ld + p.span - 1) / p.span);
    const int64_t ncb = (p.ld + DA_CB - 1) / DA_CB;                                    // pass 2: the column blocks alone, or about four workgroups per CU
    const int64_t wantb = ncb >= 2 * (int64_t)cus ? 1 : (4 * (int64_t)std::max(1, cus) + ncb - 1) / ncb;
    p.rows_blk = std::max<int64_t>(DA_ROWS_MIN, ((m + wantb - 1) / wantb + 7) / 8 * 8);
    p.nrb = (int)((m + p.rows_blk - 1) / p.rows_blk);
    return p;
}

const char* da_name(double lambda) { return lambda > 0.0 ? "LeastSquares" : "IndAffine (factored)"; }
// the argument checks both objects share; lambda = 0: IndAffine
int da_check_shape(int64_t m, int64_t n, bool ptrs, double lambda) {
    if (!(lambda >= 0.0) || std::fabs(lambda) > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    if (lambda > 0.0) {
        if (m < 1 || n < 1 || m > n || !ptrs) {
            set_error("LeastSquares: bad argument (1 <= m <= n; m > n is not supported on the device: pass an object with a prox(y, x) method, evaluated on the host through fos_feas_set_callback)");
            return FOS_EINVAL;
        }
        if (m > 46000) {
            set_error("LeastSquares: the inverse of A A' + I/lambda has order m = %lld: supported up to m = 46000 (beyond that: a host prox through fos_feas_set_callback)", (long long)m);
            return FOS_EUNSUPPORTED;
        }
        return FOS_OK;
    }
    if (m < 1 || n < 1 || m > n || !ptrs) { set_error("IndAffine (factored): bad argument (1 <= m <= n)"); return FOS_EINVAL; }
    if (m > 46000) { set_error("IndAffine (factored): the inverse of A A' has order m = %lld: supported up to m = 46000", (long long)m); return FOS_EUNSUPPORTED; }
    return FOS_OK;
}

// validation and row scaling shared by the device set-up and the host emulation: scale[i] = 1 / |A[i, :]|, bs = scale .* b.  lambda > 0 (LeastSquares): a zero
// row is legal and keeps scale 1
int da_scaling(int64_t m, int64_t n, const double* A, const double* b, double lambda, std::vector<double>& scale, std::vector<double>& bs) {
    const char* what = da_name(lambda);
    scale.assign((size_t)m, 0.0); bs.assign((size_t)m, 0.0);
    for (int64_t i = 0; i < m; ++i) {
        double s2 = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            const double v = A[i * n + j];
            if (!(v == v) || std::fabs(v) > 1e300) { set_error("%s: A has non-finite entries", what); return FOS_EINVAL; }
            s2 += v * v;
        }
        if (!(s2 > 0.0) && !(lambda > 0.0)) { set_error("IndAffine (factored): row %lld of A is zero (A must have full row rank)", (long long)i + 1); return FOS_EINVAL; }
        if (!(b[i] == b[i]) || std::fabs(b[i]) > 1e300) { set_error("%s: b has non-finite entries", what); return FOS_EINVAL; }
        scale[(size_t)i] = s2 > 0.0 ? 1.0 / std::sqrt(s2) : 1.0;
        bs[(size_t)i] = b[i] * scale[(size_t)i];
    }
    return FOS_OK;
}

}  // namespace

struct DenseAffine : ProxObject, DevOwned {
    DenseAffine() : ProxObject(FEAS_AFFINE_FACTORED) {}
    int prox(hipStream_t stream, double* y, const double* x) override;
    int64_t m = 0, n = 0;
    DaPlan p;
    int refine = 0;
    double *A = nullptr, *G = nullptr, *X = nullptr, *b = nullptr;       // A: m x ld row-major (scaled); G, X: Lm x Lm column-major; b: scaled
    double *r = nullptr, *d = nullptr, *e = nullptr, *t = nullptr;       // m-space vectors (Lm)
    double *part1 = nullptr, *part2 = nullptr;                           // [nspan][Lm], [nrb][ld] (nrb > 1)
    DenseInv inv;
};

// X = G^-1 for a factored form (this file and affine_sparse_factored.hip): G of order m, L x L column-major with the identity on its padding, X: L x L, both the
// caller's.  The work-set comes from a scratch that lives to the end of the call; the inverse is accepted at `bar`; a refusal of IndAffine (lambda == 0) names
// the full row rank it needs.  Synchronises `stream`.
int factored_inverse(const DevOwned& own, double lambda, int factor, double bar, hipStream_t stream, int64_t m, int64_t L, double* G, double* Xout, DenseInv* inv) {
    const size_t L2 = (size_t)L * (size_t)L;
    DenseWork w;
    w.c.stream = stream; w.c.l = m; w.L = L; w.G = G;
    Scratch s;
    w.fill(s);
    if (s.err != hipSuccess) { (void)hipGetLastError(); set_error("%s: hipMalloc of the set-up buffers (3 x %zu bytes) failed: %s", own.what, L2 * 8, hipGetErrorString(s.err)); return FOS_ENOMEM; }
    double* X = nullptr;
    DenseOpts o{own.what, lambda > 0.0 ? "A A' + I/lambda" : "A A'", factor, false};
    o.bar = bar; o.newton_extra = 40;                      // cond(A A') up to ~1e8: ceil(log2 cond) + 7 steps at most, each of the extra ones checked
    const int rc = dense_spd_inverse(w, o, &X, inv);
    if (rc == FOS_EINVAL && !(lambda > 0.0)) {
        const std::string why = fos_last_error();
        set_error("%s: the inverse of A A' (rows scaled to unit norm) was not accepted: A needs full row rank  [%s]", own.what, why.c_str());
    }
    FOS_TRY(rc);
    FOS_TRY(own.hip("hipMemcpyAsync", hipMemcpyAsync(Xout, X, sizeof(double) * L2, hipMemcpyDeviceToDevice, stream)));
    return own.hip("hipStreamSynchronize", hipStreamSynchronize(stream));
}

// A: m x n ROW-major, b[m]; lambda: 0: IndAffine(A, b), > 0: LeastSquares(A, b, lambda) (refine is then 0); factor: FOS_DIRECT_FACTOR_*; refine: 0..2 refinement
// steps per projection.  Synchronises `stream`.
int dense_affine_setup(int64_t m, int64_t n, const double* A, const double* b, double lambda, int factor, int refine, int cus, hipStream_t stream, ProxObject** out) {
    FOS_TRY(da_check_shape(m, n, A && b, lambda));
    if (lambda > 0.0) refine = 0;
    if (refine < 0 || refine > 2) { set_error("IndAffine (factored): refine = %d (0, 1 or 2 refinement steps per projection)", refine); return FOS_EINVAL; }
    if (factor != FOS_DIRECT_FACTOR_NEWTON && factor != FOS_DIRECT_FACTOR_CHOLESKY) { set_error("%s: factor must be FOS_DIRECT_FACTOR_NEWTON or FOS_DIRECT_FACTOR_CHOLESKY", da_name(lambda)); return FOS_EINVAL; }
    std::vector<double> scale, bs;
    FOS_TRY(da_scaling(m, n, A, b, lambda, scale, bs));
    DenseAffine* a = new DenseAffine();
    a->what = da_name(lambda);
    a->m = m; a->n = n; a->refine = refine; a->p = da_plan(m, n, cus);
    const DaPlan& p = a->p;
    const size_t L2 = (size_t)p.Lm * (size_t)p.Lm;
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete a; return code; };
    int rc = FOS_OK;
    if ((rc = a->alloc(&a->A, (size_t)m * (size_t)p.ld)) != FOS_OK || (rc = a->alloc(&a->G, L2)) != FOS_OK || (rc = a->alloc(&a->X, L2)) != FOS_OK ||
        (rc = a->alloc(&a->part1, (size_t)p.nspan * (size_t)p.Lm)) != FOS_OK || (p.nrb > 1 && (rc = a->alloc(&a->part2, (size_t)p.nrb * (size_t)p.ld)) != FOS_OK))
        return fail(rc);
    for (double** v : {&a->b, &a->r, &a->d, &a->e, &a->t}) if ((rc = a->zeros(v, (size_t)p.Lm, stream)) != FOS_OK) return fail(rc);
    DEV_HIP(a, hipMemsetAsync(a->A, 0, sizeof(double) * (size_t)m * (size_t)p.ld, stream));
    DEV_HIP(a, hipMemcpy2DAsync(a->A, sizeof(double) * (size_t)p.ld, A, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)m, hipMemcpyHostToDevice, stream));
    DEV_HIP(a, hipMemcpyAsync(a->b, bs.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
    DEV_HIP(a, hipMemcpyAsync(a->t, scale.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(da_scale_rows_kernel, dim3(1024), dim3(DA_T), 0, stream, m, p.ld, a->A, (const double*)a->t);
    LaunchCtx c{};
    c.stream = stream; c.l = m;
    launch_dense_gram_rows(c, m, p.ld, a->A, p.Lm, a->G);      // G = A A' (+ identity on the padding)
    if (lambda > 0.0)                                          // (the row scales are still in a->t)
        hipLaunchKernelGGL(da_shift_diag_kernel, dim3((unsigned)std::min<int64_t>(256, (m + DA_T - 1) / DA_T)), dim3(DA_T), 0, stream, m, p.Lm, a->G, (const double*)a->t, 1.0 / lambda);
    DEV_HIP(a, hipMemsetAsync(a->t, 0, sizeof(double) * (size_t)p.Lm, stream));
    if ((rc = factored_inverse(*a, lambda, factor, DA_BAR, stream, m, p.Lm, a->G, a->X, &a->inv)) != FOS_OK) return fail(rc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("IndAffine (factored) set-up: a kernel launch failed: %s", hipGetErrorString(e)); return fail(FOS_EHIP); }
    *out = a;
    return FOS_OK;
}

// the m-space product for the factored forms (this file and affine_sparse_factored.hip)
void launch_da_symv(hipStream_t s, int64_t l, int64_t ld, const double* M, const double* v, const double* add, double sign, double* out) {
    hipLaunchKernelGGL(da_symv_kernel, dim3((unsigned)((l + DA_T / 64 - 1) / (DA_T / 64))), dim3(DA_T), 0, s, l, ld, M, v, add, sign, out);
}
void mspace_correct(hipStream_t s, int64_t m, int64_t L, const double* X, const double* G, const double* r, double* d, double* e) {
    launch_da_symv(s, m, L, X, r, nullptr, 1.0, d);                  // d = X r
    launch_da_symv(s, m, L, G, d, r, -1.0, e);                       // e = r - G d
    launch_da_symv(s, m, L, X, e, d, 1.0, d);                        // d += X e
}

namespace {
// r = A v - b
void da_residual(const DenseAffine* a, hipStream_t s, const double* v) {
    const DaPlan& p = a->p;
    const int64_t nunits = p.ngroups * p.nspan;
    hipLaunchKernelGGL(da_rows_kernel, dim3((unsigned)((nunits + DA_T / 64 - 1) / (DA_T / 64))), dim3(DA_T), 0, s, a->m, a->n, p.ld, p.Lm, p.span, p.ngroups, nunits,
                       (const double*)a->A, v, a->part1);
    hipLaunchKernelGGL(da_rows_fold_kernel, dim3((unsigned)std::min<int64_t>(256, (a->m + DA_T - 1) / DA_T)), dim3(DA_T), 0, s, a->m, p.Lm, p.nspan, (const double*)a->part1,
                       (const double*)a->b, a->r);
}
// y = x - A'd
void da_correct(const DenseAffine* a, hipStream_t s, double* y, const double* x) {
    const DaPlan& p = a->p;
    const dim3 grid((unsigned)((p.ld + DA_CB - 1) / DA_CB), (unsigned)p.nrb);
    hipLaunchKernelGGL(da_cols_kernel, grid, dim3(DA_T), 0, s, a->m, a->n, p.ld, p.rows_blk, p.nrb == 1 ? 1 : 0, (const double*)a->A, (const double*)a->d, x, y, a->part2);
    if (p.nrb > 1)
        hipLaunchKernelGGL(da_cols_fold_kernel, dim3((unsigned)std::min<int64_t>(1024, (a->n + DA_T - 1) / DA_T)), dim3(DA_T), 0, s, a->n, p.ld, p.nrb, (const double*)a->part2, x, y);
}
int da_launches(const DenseAffine* a) { return (2 + 3 + 1 + (a->p.nrb > 1 ? 1 : 0)) + a->refine * (2 + 1 + 1 + (a->p.nrb > 1 ? 1 : 0)); }
}  // namespace

// y = the projection of x onto {A x = b} (device vectors of length n, y must not alias x), on `stream`: da_launches(a) launches, nothing else
int DenseAffine::prox(hipStream_t stream, double* y, const double* x) {
    const DenseAffine* a = this;
    da_residual(a, stream, x);                                       // r = A x - b
    mspace_correct(stream, m, p.Lm, X, G, r, d, e);                  // d = X r, corrected once
    da_correct(a, stream, y, x);                                     // y = x - A'd
    for (int k = 0; k < refine; ++k) {
        da_residual(a, stream, y);                                   // r = A y - b
        launch_da_symv(stream, m, p.Lm, X, r, nullptr, 1.0, d);      // d = X r
        da_correct(a, stream, y, y);                                 // y -= A'd
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("IndAffine (factored): a kernel launch failed: %s", hipGetErrorString(err)); return FOS_EHIP; }
    return FOS_OK;
}

// out8 = m, n, refine, factor that produced the accepted inverse, fell_back, probe residual, kernel launches per projection, bytes kept
void dense_affine_stats(const ProxObject* obj, double* out8) {
    const DenseAffine* a = static_cast<const DenseAffine*>(obj);
    out8[0] = (double)a->m; out8[1] = (double)a->n; out8[2] = (double)a->refine; out8[3] = (double)a->inv.used; out8[4] = a->inv.fell_back ? 1.0 : 0.0;
    out8[5] = a->inv.probe; out8[6] = (double)da_launches(a); out8[7] = (double)a->bytes;
}
// out6 = leading dimension of A, padded order of A A', pass 1: columns per span, spans; pass 2: rows per row block, row blocks
void dense_affine_plan(const ProxObject* obj, int64_t* out6) {
    const DenseAffine* a = static_cast<const DenseAffine*>(obj);
    out6[0] = a->p.ld; out6[1] = a->p.Lm; out6[2] = a->p.span; out6[3] = a->p.nspan; out6[4] = a->p.rows_blk; out6[5] = a->p.nrb;
}

// ---------------------------------------------------------------------------------- host emulation (tests; no GPU)
namespace {
double da_host_wave(const double (&lane)[64]) {                     // wave_sum: neighbours, pairs of pairs, ... (every step commutative: a balanced tree)
    double v[64];
    for (int i = 0; i < 64; ++i) v[i] = lane[i];
    for (int w = 1; w < 64; w <<= 1)
        for (int i = 0; i < 64; i += 2 * w) v[i] = v[i] + v[i + w];
    return v[0];
}
// out = add + sign M v, M symmetric column-major of order l with leading dimension ld, in da_symv_kernel's order
void da_host_symv(int64_t l, int64_t ld, const double* M, const double* v, const double* add, double sign, double* out) {
    for (int64_t col = 0; col < l; ++col) {
        double lane[64] = {0.0};
        const double* g = M + col * ld;
        for (int64_t q = 0; q < l / 2; ++q) lane[q % 64] += g[2 * q] * v[2 * q] + g[2 * q + 1] * v[2 * q + 1];
        if (l % 2) lane[0] += g[l - 1] * v[l - 1];
        out[col] = (add ? add[col] : 0.0) + sign * da_host_wave(lane);
    }
}
}  // namespace

void host_da_symv(int64_t l, int64_t ld, const double* M, const double* v, const double* add, double sign, double* out) { da_host_symv(l, ld, M, v, add, sign, out); }
void host_mspace_correct(int64_t m, const double* X, const double* G, const double* r, double* d, double* e) {
    da_host_symv(m, m, X, r, nullptr, 1.0, d);
    da_host_symv(m, m, G, d, r, -1.0, e);
    da_host_symv(m, m, X, e, d, 1.0, d);
}
double host_da_wave(const double* lane64) {
    double lane[64];
    for (int i = 0; i < 64; ++i) lane[i] = lane64[i];
    return da_host_wave(lane);
}
// X = G^-1 by host_chol_inverse (G, X: order m, column-major), accepted by the probe of dense_spd_inverse at DA_BAR, evaluated on the host
int host_da_inverse(const char* what, int64_t m, const double* G, double* X) {
    const int64_t bad = host_chol_inverse(m, G, X);
    double probe = bad >= 0 ? INFINITY : 0.0;
    std::vector<double> v((size_t)m), w((size_t)m), u((size_t)m);
    for (int j = 0; j < 4 && bad < 0; ++j) {
        direct_test_vector(m, j, v);
        da_host_symv(m, m, X, v.data(), nullptr, 1.0, w.data());
        da_host_symv(m, m, G, w.data(), nullptr, 1.0, u.data());
        double dmax = 0.0, nv = 0.0;
        for (int64_t i = 0; i < m; ++i) { const double e = std::fabs(u[(size_t)i] - v[(size_t)i]); dmax = (e > dmax || e != e) ? e : dmax; nv = std::max(nv, std::fabs(v[(size_t)i])); }
        dmax /= nv;
        probe = (dmax > probe || dmax != dmax) ? dmax : probe;
    }
    if (!(probe <= DA_BAR)) {
        set_error("%s: the inverse of A A' (rows scaled to unit norm) was not accepted (probe residual %.3e): A needs full row rank", what, probe);
        return FOS_EINVAL;
    }
    return FOS_OK;
}

// the same scaling, host_chol_inverse for X (accepted by the probe of dense_spd_inverse at DA_BAR, evaluated on the host), and the two passes with the split and
// the summation order the kernels have for this (m, n) on a device of 256 CUs
// lambda > 0: LeastSquares(A, b, lambda) -- the diagonal of G shifted as in the set-up, refine = 0
int host_affine_factored(int64_t m, int64_t n, const double* A, const double* b, double lambda, int refine, const double* x, double* y) {
    FOS_TRY(da_check_shape(m, n, A && b && x && y, lambda));
    if (lambda > 0.0) refine = 0;
    if (refine < 0 || refine > 2) { set_error("IndAffine (factored): refine = %d (0, 1 or 2 refinement steps per projection)", refine); return FOS_EINVAL; }
    std::vector<double> scale, bs;
    FOS_TRY(da_scaling(m, n, A, b, lambda, scale, bs));
    const DaPlan p = da_plan(m, n, 256);
    std::vector<double> As((size_t)m * (size_t)p.ld, 0.0), G((size_t)m * (size_t)m), X((size_t)m * (size_t)m);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < n; ++j) As[(size_t)(i * p.ld + j)] = A[i * n + j] * scale[(size_t)i];
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int64_t k = 0; k < p.ld; ++k) s += As[(size_t)(i * p.ld + k)] * As[(size_t)(j * p.ld + k)];
            G[(size_t)(i + j * m)] = s; G[(size_t)(j + i * m)] = s;
        }
    if (lambda > 0.0)
        for (int64_t i = 0; i < m; ++i) G[(size_t)(i + i * m)] += scale[(size_t)i] * scale[(size_t)i] * (1.0 / lambda);
    FOS_TRY(host_da_inverse(da_name(lambda), m, G.data(), X.data()));
    std::vector<double> r((size_t)m), d((size_t)m), e((size_t)m), part((size_t)std::max(p.nspan, p.nrb));
    auto residual = [&](const double* vin) {                         // da_rows_kernel + da_rows_fold_kernel
        for (int64_t i = 0; i < m; ++i) {
            for (int s = 0; s < p.nspan; ++s) {
                double lane[64] = {0.0};
                const int64_t c0 = s * p.span, c1 = std::min(c0 + p.span, p.ld);
                for (int64_t c = c0; c < c1; c += 2) {
                    const double x0 = c < n ? vin[c] : 0.0, x1 = c + 1 < n ? vin[c + 1] : 0.0;
                    lane[((c - c0) / 2) % 64] += As[(size_t)(i * p.ld + c)] * x0 + As[(size_t)(i * p.ld + c + 1)] * x1;
                }
                part[(size_t)s] = da_host_wave(lane);
            }
            double s = 0.0;
            for (int k = 0; k < p.nspan; ++k) s += part[(size_t)k];
            r[(size_t)i] = s - bs[(size_t)i];
        }
    };
    auto correct = [&](double* yout, const double* xin) {            // da_cols_kernel + da_cols_fold_kernel
        for (int64_t c = 0; c < n; ++c) {
            for (int k = 0; k < p.nrb; ++k) {
                double s = 0.0;
                for (int64_t i = k * p.rows_blk; i < std::min(m, (k + 1) * p.rows_blk); ++i) s += As[(size_t)(i * p.ld + c)] * d[(size_t)i];
                part[(size_t)k] = s;
            }
            double s = part[0];
            if (p.nrb > 1) { s = 0.0; for (int k = 0; k < p.nrb; ++k) s += part[(size_t)k]; }
            yout[c] = xin[c] - s;
        }
    };
    residual(x);
    host_mspace_correct(m, X.data(), G.data(), r.data(), d.data(), e.data());
    correct(y, x);
    for (int k = 0; k < refine; ++k) {
        residual(y);
        da_host_symv(m, m, X.data(), r.data(), nullptr, 1.0, d.data());
        correct(y, y);
    }
    return FOS_OK;
}

}  // namespace fos
