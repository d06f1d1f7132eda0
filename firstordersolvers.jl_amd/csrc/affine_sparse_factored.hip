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
#include <string>
#include <vector>

namespace fos {

namespace {

constexpr int SF_T = 256;                     // threads per workgroup: four work items
constexpr int SF_LANE_ENTRIES = 4;            // packed rows: entries per lane of the packet's longest row, while g < 64
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

int sf_lanes(int len) {                                  // the fewest lanes (a power of two, at most 64) that leave a lane at most SF_LANE_ENTRIES entries of a row
    int g = 1;
    while (g < 64 && g * SF_LANE_ENTRIES < len) g <<= 1;
    return g;
}

}  // namespace

// the work items of one pass, from the row pointers and SEG alone (SfItem, SfPass: fos_internal.hpp; nspace_cg.hip plans its passes with it too)
void sf_plan_pass(int64_t nrows, const int32_t* rp, int seg, SfPass* P) {
    P->items.clear(); P->frow.clear(); P->fptr.assign(1, 0); P->nparts = 0;
    auto len = [&](int64_t r) { return rp[r + 1] - rp[r]; };
    int64_t r = 0;
    while (r < nrows) {
        const int l0 = len(r);
        if (l0 > seg) {
            for (int e = rp[r]; e < rp[r + 1]; e += seg) P->items.push_back(SfItem{(int32_t)r, e, std::min(seg, rp[r + 1] - e), (int32_t)P->nparts++});
            P->frow.push_back((int32_t)r); P->fptr.push_back((int32_t)P->nparts);
            ++r;
            continue;
        }
        int g = sf_lanes(l0), cnt = 1;
        while (r + cnt < nrows && len(r + cnt) <= seg) {
            const int g2 = std::max(g, sf_lanes(len(r + cnt)));
            if ((cnt + 1) * g2 > 64) break;
            g = g2; ++cnt;
        }
        P->items.push_back(SfItem{(int32_t)r, cnt, -g, -1});
        r += cnt;
    }
}

namespace {

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

// what both the device set-up and the host emulation refuse, and the scaled rows
const char* sf_name(double lambda) { return lambda > 0.0 ? "LeastSquares (sparse, factored)" : "IndAffine (sparse, factored)"; }
int sf_rows(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int refine, SparseRows* R) {
    const char* what = sf_name(lambda);
    if (!(lambda >= 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    if (m < 1 || n < 1 || m > n) { set_error("%s: bad argument (1 <= m <= n)", what); return FOS_EINVAL; }
    if (m > 46000) { set_error("%s: the inverse of A A' has order m = %lld: supported up to m = 46000", what, (long long)m); return FOS_EUNSUPPORTED; }
    if (refine < 0 || refine > 2) { set_error("%s: refine = %d (0, 1 or 2 refinement steps per projection)", what, refine); return FOS_EINVAL; }
    FOS_TRY(sparse_affine_rows(what, m, n, colptr, rowval, nzval, b, R, lambda > 0.0));
    for (int64_t j = 0; j < n; ++j)                                                   // (sf_gram_kernel adds a column's entries side by side)
        for (int32_t e = R->trp[(size_t)j] + 1; e < R->trp[(size_t)j + 1]; ++e)
            if (R->tci[(size_t)e] <= R->tci[(size_t)e - 1]) {
                set_error("%s: the row indices of column %lld are not strictly ascending (duplicated or unsorted entries)", what, (long long)j + 1);
                return FOS_EINVAL;
            }
    return FOS_OK;
}

}  // namespace

struct SparseFactored : ProxObject, DevOwned {
    SparseFactored() : ProxObject(FEAS_SPARSE_FACTORED) {}
    int prox(hipStream_t stream, double* y, const double* x) override;
    int64_t m = 0, n = 0, nnz = 0, L = 0;
    int refine = 0, seg = 0;
    int32_t *rp = nullptr, *ci = nullptr, *trp = nullptr, *tci = nullptr;
    double *va = nullptr, *tva = nullptr;
    double *G = nullptr, *X = nullptr, *b = nullptr;                    // G, X: L x L column-major; b: scaled
    double *r = nullptr, *d = nullptr, *e = nullptr;                    // m-space vectors (L)
    SfItem *items1 = nullptr, *items2 = nullptr;
    int32_t *frow1 = nullptr, *fptr1 = nullptr, *frow2 = nullptr, *fptr2 = nullptr;
    double *part1 = nullptr, *part2 = nullptr;
    int nitems1 = 0, nitems2 = 0, nfold1 = 0, nfold2 = 0;
    int64_t nparts1 = 0, nparts2 = 0;
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
    SparseRows R;
    FOS_TRY(sf_rows(m, n, colptr, rowval, nzval, b, lambda, refine, &R));
    int seg = 0;
    FOS_TRY(sf_segment_length(&seg));
    SfPass P1, P2;
    sf_plan_pass(m, R.rp.data(), seg, &P1);
    sf_plan_pass(n, R.trp.data(), seg, &P2);
    SparseFactored* a = new SparseFactored();
    a->what = sf_name(lambda);
    a->m = m; a->n = n; a->nnz = R.nnz; a->L = (m + 63) / 64 * 64; a->refine = refine; a->seg = seg;
    a->nitems1 = (int)P1.items.size(); a->nitems2 = (int)P2.items.size(); a->nfold1 = (int)P1.frow.size(); a->nfold2 = (int)P2.frow.size();
    a->nparts1 = P1.nparts; a->nparts2 = P2.nparts;
    const size_t L = (size_t)a->L, L2 = L * L;
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete a; return code; };
    int rc = FOS_OK;
    if ((rc = a->upload(&a->rp, R.rp, stream)) != FOS_OK || (rc = a->upload(&a->ci, R.ci, stream)) != FOS_OK || (rc = a->upload(&a->va, R.va, stream)) != FOS_OK ||
        (rc = a->upload(&a->trp, R.trp, stream)) != FOS_OK || (rc = a->upload(&a->tci, R.tci, stream)) != FOS_OK || (rc = a->upload(&a->tva, R.tva, stream)) != FOS_OK ||
        (rc = a->upload(&a->items1, P1.items, stream)) != FOS_OK || (rc = a->upload(&a->items2, P2.items, stream)) != FOS_OK ||
        (rc = a->upload(&a->frow1, P1.frow, stream)) != FOS_OK || (rc = a->upload(&a->fptr1, P1.fptr, stream)) != FOS_OK ||
        (rc = a->upload(&a->frow2, P2.frow, stream)) != FOS_OK || (rc = a->upload(&a->fptr2, P2.fptr, stream)) != FOS_OK ||
        (rc = a->alloc(&a->part1, (size_t)P1.nparts)) != FOS_OK || (rc = a->alloc(&a->part2, (size_t)P2.nparts)) != FOS_OK ||
        (rc = a->zeros(&a->G, L2, stream)) != FOS_OK || (rc = a->alloc(&a->X, L2)) != FOS_OK)
        return fail(rc);
    for (double** v : {&a->b, &a->r, &a->d, &a->e}) if ((rc = a->zeros(v, L, stream)) != FOS_OK) return fail(rc);
    DEV_HIP(a, hipMemcpyAsync(a->b, R.bs.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
    launch_sf_gram(stream, m, a->L, a->rp, a->ci, a->va, a->trp, a->tci, a->tva, a->G);
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
unsigned sf_grid(int nitems) { return (unsigned)((nitems + SF_T / 64 - 1) / (SF_T / 64)); }
// r = A v - b
void sf_residual(const SparseFactored* a, hipStream_t s, const double* v) {
    hipLaunchKernelGGL(sf_pass_kernel<1>, dim3(sf_grid(a->nitems1)), dim3(SF_T), 0, s, a->nitems1, (const SfItem*)a->items1, (const int32_t*)a->rp, (const int32_t*)a->ci,
                       (const double*)a->va, v, (const double*)a->b, a->r, a->part1);
    if (a->nfold1 > 0)
        hipLaunchKernelGGL(sf_fold_kernel<1>, dim3((unsigned)std::min(1024, (a->nfold1 + SF_T - 1) / SF_T)), dim3(SF_T), 0, s, a->nfold1, (const int32_t*)a->frow1,
                           (const int32_t*)a->fptr1, (const double*)a->part1, (const double*)a->b, a->r);
}
// y = x - A'd
void sf_correct(const SparseFactored* a, hipStream_t s, double* y, const double* x) {
    hipLaunchKernelGGL(sf_pass_kernel<2>, dim3(sf_grid(a->nitems2)), dim3(SF_T), 0, s, a->nitems2, (const SfItem*)a->items2, (const int32_t*)a->trp, (const int32_t*)a->tci,
                       (const double*)a->tva, (const double*)a->d, x, y, a->part2);
    if (a->nfold2 > 0)
        hipLaunchKernelGGL(sf_fold_kernel<2>, dim3((unsigned)std::min(1024, (a->nfold2 + SF_T - 1) / SF_T)), dim3(SF_T), 0, s, a->nfold2, (const int32_t*)a->frow2,
                           (const int32_t*)a->fptr2, (const double*)a->part2, x, y);
}
int sf_launches(const SparseFactored* a) {
    const int p1 = 1 + (a->nfold1 > 0 ? 1 : 0), p2 = 1 + (a->nfold2 > 0 ? 1 : 0);
    return (p1 + 3 + p2) + a->refine * (p1 + 1 + p2);
}
}  // namespace

// y = the projection of x onto {A x = b} (device vectors of length n, y must not alias x), on `stream`: sf_launches(a) launches, nothing else
int SparseFactored::prox(hipStream_t stream, double* y, const double* x) {
    const SparseFactored* a = this;
    sf_residual(a, stream, x);                                                   // r = A x - b
    mspace_correct(stream, m, L, X, G, r, d, e);                                 // d = X r, corrected once
    sf_correct(a, stream, y, x);                                                 // y = x - A'd
    for (int k = 0; k < refine; ++k) {
        sf_residual(a, stream, y);                                               // r = A y - b
        launch_da_symv(stream, m, L, X, r, nullptr, 1.0, d);                     // d = X r
        sf_correct(a, stream, y, y);                                             // y -= A'd
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
    out8[0] = a->nnz; out8[1] = a->L; out8[2] = a->seg; out8[3] = a->nitems1; out8[4] = a->nfold1; out8[5] = a->nitems2; out8[6] = a->nfold2;
    out8[7] = a->nparts1 + a->nparts2;
}

// ---------------------------------------------------------------------------------- host emulation (tests; no GPU)
namespace {
// one pass in sf_pass_kernel's and sf_fold_kernel's order: out[row] = s - aux[row] (pass 1) / aux[row] - s (pass 2)
void sf_host_pass(int pass, const SfPass& P, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, const std::vector<double>& va, const double* in,
                  const double* aux, double* out) {
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
    SparseRows R;
    FOS_TRY(sf_rows(m, n, colptr, rowval, nzval, b, lambda, refine, &R));
    int seg = 0;
    FOS_TRY(sf_segment_length(&seg));
    SfPass P1, P2;
    sf_plan_pass(m, R.rp.data(), seg, &P1);
    sf_plan_pass(n, R.trp.data(), seg, &P2);
    std::vector<double> G((size_t)m * (size_t)m, 0.0), X((size_t)m * (size_t)m);
    for (int64_t i = 0; i < m; ++i)
        for (int32_t e = R.rp[(size_t)i]; e < R.rp[(size_t)i + 1]; ++e) {
            const int32_t c = R.ci[(size_t)e];
            for (int32_t t = R.trp[(size_t)c]; t < R.trp[(size_t)c + 1]; ++t) G[(size_t)(R.tci[(size_t)t] + i * m)] += R.va[(size_t)e] * R.tva[(size_t)t];
        }
    if (lambda > 0.0)
        for (int64_t i = 0; i < m; ++i) G[(size_t)(i + i * m)] += R.scale[(size_t)i] * R.scale[(size_t)i] * (1.0 / lambda);
    FOS_TRY(host_da_inverse(sf_name(lambda), m, G.data(), X.data()));
    std::vector<double> r((size_t)m), d((size_t)m), e((size_t)m);
    sf_host_pass(1, P1, R.rp, R.ci, R.va, x, R.bs.data(), r.data());
    host_mspace_correct(m, X.data(), G.data(), r.data(), d.data(), e.data());
    sf_host_pass(2, P2, R.trp, R.tci, R.tva, d.data(), x, y);
    for (int k = 0; k < refine; ++k) {
        sf_host_pass(1, P1, R.rp, R.ci, R.va, y, R.bs.data(), r.data());
        host_da_symv(m, m, X.data(), r.data(), nullptr, 1.0, d.data());
        sf_host_pass(2, P2, R.trp, R.tci, R.tva, d.data(), y, y);
    }
    return FOS_OK;
}

}  // namespace fos
