// IndAffine(A, b) with a SPARSE A on the device, factored form: the exact projection  y = x - A'(A A')^-1 (A x - b)  evaluated as written, A kept sparse and
// (A A')^-1 of order m <= 46 000 kept dense -- the direct counterpart of affine_sparse.hip's conjugate gradients: a fixed number of launches whatever cond(A A'),
// no host synchronise, no copy.  (ProximalOperators.IndAffine factorises A once and applies the factor; this is the same idea with the m-space kept as an inverse.)
//
//   * set-up: sparse_affine_rows (affine_sparse.hip) validates, scales the rows of [A | b] to unit norm and leaves A and A' as two CSR matrices (fp64 values, int32
//     columns); G = A A' (order L = m rounded up to 64, identity on the padding) by sf_gram_kernel; X = G^-1 by dense_spd_inverse with the options of the dense
//     factored form (affine_dense.hip: probe bar 1e-7, which the projection's correction step squares).  G and X stay, 16 L^2 bytes.
//   * a projection:  r = A x - b (pass 1, the CSR of A);  d = X r;  d += X (r - G d) (da_symv_kernel, three launches);  y = x - A'd (pass 2, the CSR of A');
//     then `refine` times  r = A y - b, d = X r, y -= A'd.
//   * the two passes are one kernel over a table of WORK ITEMS, one wavefront each, built on the host: a row longer than SEG stored entries is cut into segments of
//     at most SEG, one item each (the 64 lanes walk the segment's (column, value) stream side by side: coalesced, one wave_sum, the sum to part[segment]); the
//     other rows are packed, neighbours together, into packets of 64 / g rows with g = 1 .. 64 lanes per row, g chosen PER PACKET so that no lane has more than
//     SF_LANE_ENTRIES entries of the packet's longest row (or, at g = 64, SEG / 64).  No wavefront's work depends on the longest row of the matrix.  A packed row
//     writes its result itself (r_j = s - b_j / y_i = x_i - s; an empty row of A': y_i = x_i); sf_fold_kernel adds a cut row's partials in segment order and
//     applies the same epilogue.
//   Nothing is atomic and every sum has a fixed order: the same input gives the same bits, from run to run and from handle to handle.
//
// LeastSquares(A, b, lambda) with a sparse wide A is the same object with a shifted G, as in affine_dense.hip: prox_f(x) = x - A'(A A' + I/lambda)^-1 (A x - b), with
// the rows scaled by D:  x - Ah'(Ah Ah' + D^2/lambda)^-1 (Ah x - D b).  The set-up adds scale[i]^2 / lambda to the diagonal of G (sf_shift_diag_kernel) and everything
// after it is unchanged; refine is 0, a zero row keeps scale 1 and dependent rows are accepted (the shifted G is positive definite).  lambda = 0 is IndAffine, to the bit.
#include "fos_solver.hpp"
#include "dev_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace fos {

namespace {

constexpr int SF_T = 256;                     // threads per workgroup: four work items
constexpr double SF_BAR = 1e-7;               // the inverse of A A' is accepted at this probe residual (as affine_dense.hip)

// PASS 1 (the CSR of A):  s = A[row, segment] in  ->  out[row] = s - aux[row]          (in = x or y, aux = b, out = r)
// PASS 2 (the CSR of A'): s = A'[row, segment] in ->  out[row] = aux[row] - s          (in = d, aux = x or y, out = y; out may be aux: same lane reads and writes)
template <int PASS>
__global__ __launch_bounds__(SF_T) void sf_pass_kernel(int nitems, const SfItem* __restrict__ items, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                       const double* __restrict__ va, const double* __restrict__ in, const double* aux, double* out,
                                                       double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int it = blockIdx.x * (SF_T / 64) + (threadIdx.x >> 6);
    if (it >= nitems) return;                                                        // (wave-uniform)
    const SfItem w = items[it];
    const bool segment = w.c > 0;
    const int g = segment ? 64 : -w.c;
    const int sub = lane & (g - 1), k = lane >> __builtin_ctz(g);
    const bool live = segment ? true : k < w.b;
    const int row = segment ? w.a : w.a + k;
    int e0 = 0, e1 = 0;
    if (segment) { e0 = w.b; e1 = w.b + w.c; }
    else if (live) { e0 = rp[row]; e1 = rp[row + 1]; }
    double s = 0.0;
    int e = e0 + sub;
    for (; e + 3 * g < e1; e += 4 * g) {                                             // four loads of each stream in flight; the sum stays in entry order
        const int c0 = ci[e], c1 = ci[e + g], c2 = ci[e + 2 * g], c3 = ci[e + 3 * g];
        const double a0 = va[e], a1 = va[e + g], a2 = va[e + 2 * g], a3 = va[e + 3 * g];
        const double v0 = in[c0], v1 = in[c1], v2 = in[c2], v3 = in[c3];
        s += a0 * v0; s += a1 * v1; s += a2 * v2; s += a3 * v3;
    }
    for (; e < e1; e += g) s += va[e] * in[ci[e]];
    s = group_sum(s, g);
    if (!live || sub != 0) return;
    if (segment) part[w.d] = s;
    else out[row] = PASS == 1 ? s - aux[row] : aux[row] - s;
}
// the rows that were cut: out[frow[k]] = epilogue(sum of part[fptr[k] .. fptr[k + 1]) in segment order)
template <int PASS>
__global__ __launch_bounds__(SF_T) void sf_fold_kernel(int nfold, const int32_t* __restrict__ frow, const int32_t* __restrict__ fptr, const double* __restrict__ part,
                                                       const double* aux, double* out) {
    for (int k = blockIdx.x * SF_T + threadIdx.x; k < nfold; k += gridDim.x * SF_T) {
        double s = 0.0;
        for (int p = fptr[k]; p < fptr[k + 1]; ++p) s += part[p];
        const int row = frow[k];
        out[row] = PASS == 1 ? s - aux[row] : aux[row] - s;
    }
}
// set-up: G = A A' + (identity on the padding), L x L column-major, zeroed by the caller.  One workgroup per column i of G: the entries (i, c) of row i one after
// the other in column order, the entries of column c (= row c of A') side by side -- they hit distinct rows of G (the set-up refuses duplicated entries), so
// nothing is atomic, every element is summed over c ascending, and G[i, j] and G[j, i] add the same products in the same order: exactly symmetric.
__global__ __launch_bounds__(SF_T) void sf_gram_kernel(int64_t m, int64_t L, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci, const double* __restrict__ va,
                                                       const int32_t* __restrict__ trp, const int32_t* __restrict__ tci, const double* __restrict__ tva, double* G) {
    for (int64_t i = blockIdx.x; i < L; i += gridDim.x) {
        double* col = G + i * L;
        if (i < m) {
            for (int e = rp[i]; e < rp[i + 1]; ++e) {
                const int c = ci[e];
                const double a = va[e];
                for (int t = trp[c] + (int)threadIdx.x; t < trp[c + 1]; t += SF_T) col[tci[t]] += a * tva[t];
                __syncthreads();
            }
        } else if (threadIdx.x == 0) col[i] = 1.0;
    }
}

// set-up of LeastSquares: G[i, i] += scale[i]^2 / lambda  (da_shift_diag_kernel of affine_dense.hip)
__global__ __launch_bounds__(SF_T) void sf_shift_diag_kernel(int64_t m, int64_t L, double* __restrict__ G, const double* __restrict__ scale, double inv_lambda) {
    for (int64_t i = blockIdx.x * (int64_t)SF_T + threadIdx.x; i < m; i += (int64_t)gridDim.x * SF_T) G[i + i * L] += scale[i] * scale[i] * inv_lambda;
}

// FOS_SF_SEG (read at every set-up: per handle): a multiple of 64 from 64 up to the default
int sf_segment_length(int* seg) {
    *seg = SF_SEG_DEFAULT;
    const char* s = std::getenv("FOS_SF_SEG");
    if (!s || !*s) return FOS_OK;
    char* end = nullptr;
    const long v = std::strtol(s, &end, 10);
    if (*end || v < 64 || v > SF_SEG_DEFAULT || v % 64) {
        set_error("IndAffine (sparse, factored): FOS_SF_SEG = \"%s\" (a multiple of 64 from 64 to %d)", s, SF_SEG_DEFAULT);
        return FOS_EINVAL;
    }
    *seg = (int)v;
    return FOS_OK;
}

// what both the device set-up and the host emulation refuse; the scaled rows and the plans of the two passes (0: the CSR of A, 1: the CSR of A')
const char* sf_name(double lambda) { return lambda > 0.0 ? "LeastSquares (sparse, factored)" : "IndAffine (sparse, factored)"; }
struct SfHost { ScaledRows R; SfPass P[2]; int seg = 0; };
int sf_rows(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int refine, SfHost* H) {
    const char* what = sf_name(lambda);
    if (!(lambda >= 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    if (m < 1 || n < 1 || m > n) { set_error("%s: bad argument (1 <= m <= n)", what); return FOS_EINVAL; }
    if (m > 46000) { set_error("%s: the inverse of A A' has order m = %lld: supported up to m = 46000", what, (long long)m); return FOS_EUNSUPPORTED; }
    if (refine < 0 || refine > 2) { set_error("%s: refine = %d (0, 1 or 2 refinement steps per projection)", what, refine); return FOS_EINVAL; }
    FOS_TRY(sparse_affine_rows(what, m, n, colptr, rowval, nzval, b, true, lambda > 0.0, &H->R));      // (ascending: sf_gram_kernel adds a column's entries side by side)
    FOS_TRY(sf_segment_length(&H->seg));
    sf_plan_pass(m, H->R.A.rp.data(), H->seg, &H->P[0]);
    sf_plan_pass(n, H->R.At.rp.data(), H->seg, &H->P[1]);
    return FOS_OK;
}

}  // namespace

struct SparseFactored : ProxObject, DevOwned {
    SparseFactored() : ProxObject(FEAS_SPARSE_FACTORED) {}
    int prox(hipStream_t stream, double* y, const double* x) override;
    int64_t m = 0, n = 0, nnz = 0, L = 0;
    int refine = 0, seg = 0;
    DevCsr A, At;
    DevPass pass[2];                                                    // 0: r = A v - b;  1: y = x - A'd
    double *G = nullptr, *X = nullptr, *b = nullptr;                    // G, X: L x L column-major; b: scaled
    double *r = nullptr, *d = nullptr, *e = nullptr;                    // m-space vectors (L)
    DenseInv inv;
};

// A: m x n CSC, 1-based; b[m]; factor: FOS_DIRECT_FACTOR_*; refine: 0..2 refinement steps per projection.  Synchronises `stream`.
int sparse_factored_setup(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int factor,
                          int refine, hipStream_t stream, ProxObject** out) {
    if (factor != FOS_DIRECT_FACTOR_NEWTON && factor != FOS_DIRECT_FACTOR_CHOLESKY) {
        set_error("%s: factor must be FOS_DIRECT_FACTOR_NEWTON or FOS_DIRECT_FACTOR_CHOLESKY", sf_name(lambda));
        return FOS_EINVAL;
    }
    if (lambda > 0.0) refine = 0;
    SfHost H;
    FOS_TRY(sf_rows(m, n, colptr, rowval, nzval, b, lambda, refine, &H));
    const ScaledRows& R = H.R;
    SparseFactored* a = new SparseFactored();
    a->what = sf_name(lambda);
    a->m = m; a->n = n; a->nnz = (int64_t)R.A.ci.size(); a->L = (m + 63) / 64 * 64; a->refine = refine; a->seg = H.seg;
    const size_t L = (size_t)a->L, L2 = L * L;
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete a; return code; };
    int rc = FOS_OK;
    if ((rc = a->A.upload(*a, R.A, stream)) != FOS_OK || (rc = a->At.upload(*a, R.At, stream)) != FOS_OK ||
        (rc = a->pass[0].upload(*a, H.P[0], stream)) != FOS_OK || (rc = a->pass[1].upload(*a, H.P[1], stream)) != FOS_OK ||
        (rc = a->zeros(&a->G, L2, stream)) != FOS_OK || (rc = a->alloc(&a->X, L2)) != FOS_OK)
        return fail(rc);
    for (double** v : {&a->b, &a->r, &a->d, &a->e}) if ((rc = a->zeros(v, L, stream)) != FOS_OK) return fail(rc);
    DEV_HIP(a, hipMemcpyAsync(a->b, R.bs.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
    launch_sf_gram(stream, m, a->L, a->A.rp, a->A.ci, a->A.va, a->At.rp, a->At.ci, a->At.va, a->G);
    if (lambda > 0.0) {                                    // (a->e holds the row scales until the first projection overwrites it)
        DEV_HIP(a, hipMemcpyAsync(a->e, R.scale.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(sf_shift_diag_kernel, dim3((unsigned)std::min<int64_t>(256, (m + SF_T - 1) / SF_T)), dim3(SF_T), 0, stream, m, a->L, a->G, (const double*)a->e, 1.0 / lambda);
    }
    if ((rc = factored_inverse(*a, lambda, factor, SF_BAR, stream, m, a->L, a->G, a->X, &a->inv)) != FOS_OK) return fail(rc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("IndAffine (sparse, factored) set-up: a kernel launch failed: %s", hipGetErrorString(e)); return fail(FOS_EHIP); }
    *out = a;
    return FOS_OK;
}

// G = B B' (+ identity on the padding m .. L-1) for a sparse B of m rows: its CSR (rp / ci / va) and the CSR of B' (trp / tci / tva), column indices strictly
// ascending in every row of B'; G: L x L column-major, zeroed by the caller (sf_gram_kernel; nspace.hip forms A'A with it)
void launch_sf_gram(hipStream_t stream, int64_t m, int64_t L, const int32_t* rp, const int32_t* ci, const double* va, const int32_t* trp, const int32_t* tci,
                    const double* tva, double* G) {
    hipLaunchKernelGGL(sf_gram_kernel, dim3((unsigned)std::min<int64_t>(L, 65536)), dim3(SF_T), 0, stream, m, L, rp, ci, va, trp, tci, tva, G);
}

namespace {
// PASS 1: out = A in - aux (r = A v - b);  PASS 2: out = aux - A'in (y = x - A'd); the fold behind it when a row was cut
template <int PASS>
void sf_launch_pass(const SparseFactored* a, hipStream_t s, const double* in, const double* aux, double* out) {
    const DevCsr& M = PASS == 1 ? a->A : a->At;
    const DevPass& P = a->pass[PASS - 1];
    hipLaunchKernelGGL(sf_pass_kernel<PASS>, dim3((unsigned)((P.nitems + SF_T / 64 - 1) / (SF_T / 64))), dim3(SF_T), 0, s, P.nitems, (const SfItem*)P.items,
                       (const int32_t*)M.rp, (const int32_t*)M.ci, (const double*)M.va, in, aux, out, P.part);
    if (P.nfold > 0)
        hipLaunchKernelGGL(sf_fold_kernel<PASS>, dim3((unsigned)std::min(1024, (P.nfold + SF_T - 1) / SF_T)), dim3(SF_T), 0, s, P.nfold, (const int32_t*)P.frow,
                           (const int32_t*)P.fptr, (const double*)P.part, aux, out);
}
int sf_launches(const SparseFactored* a) {
    const int p1 = 1 + (a->pass[0].nfold > 0 ? 1 : 0), p2 = 1 + (a->pass[1].nfold > 0 ? 1 : 0);
    return (p1 + 3 + p2) + a->refine * (p1 + 1 + p2);
}
}  // namespace

// y = the projection of x onto {A x = b} (device vectors of length n, y must not alias x), on `stream`: sf_launches(a) launches, nothing else
int SparseFactored::prox(hipStream_t stream, double* y, const double* x) {
    const SparseFactored* a = this;
    sf_launch_pass<1>(a, stream, x, b, r);                                       // r = A x - b
    mspace_correct(stream, m, L, X, G, r, d, e);                                 // d = X r, corrected once
    sf_launch_pass<2>(a, stream, d, x, y);                                       // y = x - A'd
    for (int k = 0; k < refine; ++k) {
        sf_launch_pass<1>(a, stream, y, b, r);                                   // r = A y - b
        launch_da_symv(stream, m, L, X, r, nullptr, 1.0, d);                     // d = X r
        sf_launch_pass<2>(a, stream, d, y, y);                                   // y -= A'd
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) { set_error("IndAffine (sparse, factored): a kernel launch failed: %s", hipGetErrorString(err)); return FOS_EHIP; }
    return FOS_OK;
}

// out8 = m, n, refine, factor that produced the accepted inverse, fell_back, probe residual, kernel launches per projection, bytes kept
void sparse_factored_stats(const ProxObject* obj, double* out8) {
    const SparseFactored* a = static_cast<const SparseFactored*>(obj);
    out8[0] = (double)a->m; out8[1] = (double)a->n; out8[2] = (double)a->refine; out8[3] = (double)a->inv.used; out8[4] = a->inv.fell_back ? 1.0 : 0.0;
    out8[5] = a->inv.probe; out8[6] = (double)sf_launches(a); out8[7] = (double)a->bytes;
}
// out8 = stored entries, padded order of A A', SEG in force, pass 1: work items, rows cut (folded); pass 2: work items, rows cut; segments of the cut rows of both passes
void sparse_factored_plan(const ProxObject* obj, int64_t* out8) {
    const SparseFactored* a = static_cast<const SparseFactored*>(obj);
    out8[0] = a->nnz; out8[1] = a->L; out8[2] = a->seg; out8[3] = a->pass[0].nitems; out8[4] = a->pass[0].nfold; out8[5] = a->pass[1].nitems; out8[6] = a->pass[1].nfold;
    out8[7] = a->pass[0].nparts + a->pass[1].nparts;
}

// ---------------------------------------------------------------------------------- host emulation (tests; no GPU)
namespace {
// one pass in sf_pass_kernel's and sf_fold_kernel's order: out[row] = s - aux[row] (pass 1) / aux[row] - s (pass 2)
void sf_host_pass(int pass, const SfPass& P, const HostCsr& M, const double* in, const double* aux, double* out) {
    const std::vector<int32_t>&rp = M.rp, &ci = M.ci;
    const std::vector<double>& va = M.va;
    std::vector<double> part((size_t)std::max<int64_t>(P.nparts, 1));
    auto group = [&](int e0, int e1, int g) {                         // the lanes' sums in entry order, then group_sum's tree over g lanes
        double lane[64] = {0.0};
        for (int e = e0; e < e1; ++e) lane[(e - e0) % g] += va[(size_t)e] * in[ci[(size_t)e]];
        for (int w = 1; w < g; w <<= 1)
            for (int i = 0; i < g; i += 2 * w) lane[i] = lane[i] + lane[i + w];
        return lane[0];
    };
    for (const SfItem& w : P.items) {
        if (w.c > 0) { part[(size_t)w.d] = group(w.b, w.b + w.c, 64); continue; }
        for (int k = 0; k < w.b; ++k) {
            const int row = w.a + k;
            const double s = group(rp[(size_t)row], rp[(size_t)row + 1], -w.c);
            out[row] = pass == 1 ? s - aux[row] : aux[row] - s;
        }
    }
    for (size_t k = 0; k < P.frow.size(); ++k) {
        double s = 0.0;
        for (int p = P.fptr[k]; p < P.fptr[k + 1]; ++p) s += part[(size_t)p];
        const int row = P.frow[k];
        out[row] = pass == 1 ? s - aux[row] : aux[row] - s;
    }
}
}  // namespace

// the same validation and scaling, G in sf_gram_kernel's order, host_da_inverse for X, the segment tables of this matrix (FOS_SF_SEG honoured; the tables do not depend on
// the device) and both passes, the folds and the m-space products in the kernels' summation order
int host_affine_sparse_factored(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int refine,
                                const double* x, double* y) {
    if (!x || !y) { set_error("%s: bad argument", sf_name(lambda)); return FOS_EINVAL; }
    if (lambda > 0.0) refine = 0;
    SfHost H;
    FOS_TRY(sf_rows(m, n, colptr, rowval, nzval, b, lambda, refine, &H));
    const HostCsr &A = H.R.A, &At = H.R.At;
    const std::vector<double>&bs = H.R.bs, &scale = H.R.scale;
    std::vector<double> G((size_t)m * (size_t)m, 0.0), X((size_t)m * (size_t)m);
    for (int64_t i = 0; i < m; ++i)
        for (int32_t e = A.rp[(size_t)i]; e < A.rp[(size_t)i + 1]; ++e) {
            const int32_t c = A.ci[(size_t)e];
            for (int32_t t = At.rp[(size_t)c]; t < At.rp[(size_t)c + 1]; ++t) G[(size_t)(At.ci[(size_t)t] + i * m)] += A.va[(size_t)e] * At.va[(size_t)t];
        }
    if (lambda > 0.0)
        for (int64_t i = 0; i < m; ++i) G[(size_t)(i + i * m)] += scale[(size_t)i] * scale[(size_t)i] * (1.0 / lambda);
    FOS_TRY(host_da_inverse(sf_name(lambda), m, G.data(), X.data()));
    std::vector<double> r((size_t)m), d((size_t)m), e((size_t)m);
    sf_host_pass(1, H.P[0], A, x, bs.data(), r.data());
    host_mspace_correct(m, X.data(), G.data(), r.data(), d.data(), e.data());
    sf_host_pass(2, H.P[1], At, d.data(), x, y);
    for (int k = 0; k < refine; ++k) {
        sf_host_pass(1, H.P[0], A, y, bs.data(), r.data());
        host_da_symv(m, m, X.data(), r.data(), nullptr, 1.0, d.data());
        sf_host_pass(2, H.P[1], At, d.data(), y, y);
    }
    return FOS_OK;
}

}  // namespace fos
