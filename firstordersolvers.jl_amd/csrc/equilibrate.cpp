// Opt-in equilibration of  minimize c'x  s.t.  A x + s = b, s in K1, x in K2  (fos_create3 with equil_passes > 0; fos_host_equilibrate is the same code
// without a GPU).  The reference does not scale its data (HSDE.jl:7-29 takes A, b, c as given), so this has no counterpart there: it is Ruiz scaling in the
// infinity norm with factors that are CONSTANT over every non-separable cone -- the condition under which D K1 = K1 and E K2 = K2, so that the scaled problem
// has the same cones and the same embedding -- followed by a common scale of A (mean square singular value 1) and of b, c (norm EQ_TARGET_NORM).
//   A^ = D A E,  b^ = sigma D b,  c^ = rho E c;   x = E x^ / sigma,  y = D y^ / rho,  tau = tau^,  r = r^ / (rho E),  s = s^ / (sigma D),  kappa = kappa^ / (sigma rho)
#include <cmath>

#include "fos_internal.hpp"

namespace fos {

namespace {
// SOC, SOCRotated, SDP, ExpPrimal, ExpDual: a cone that is not a product of half-lines, so its factor must be one number
bool cone_couples(int32_t type) { return type >= FOS_CONE_SOC; }

// v over every coupling cone's range <- its arithmetic mean there (summed in index order)
void cone_means(std::vector<double>& v, int64_t nK, const int32_t* type, const int64_t* start, const int64_t* len) {
    for (int64_t k = 0; k < nK; ++k) {
        if (!cone_couples(type[k])) continue;
        const int64_t i0 = start[k] - 1;
        double s = 0.0;
        for (int64_t i = 0; i < len[k]; ++i) s += v[i0 + i];
        const double mean = s / (double)len[k];
        for (int64_t i = 0; i < len[k]; ++i) v[i0 + i] = mean;
    }
}
}  // namespace

int host_equilibrate(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, const double* c,
                     int64_t nK1, const int32_t* K1type, const int64_t* K1start, const int64_t* K1len,
                     int64_t nK2, const int32_t* K2type, const int64_t* K2start, const int64_t* K2len, int passes, EqScaling* out) {
    if (m < 0 || n < 0 || !colptr || (!rowval && colptr[n] > 1) || (!nzval && colptr[n] > 1) || (!b && m) || (!c && n) || !out) {
        set_error("NULL or negative argument");
        return FOS_EINVAL;
    }
    if (passes < 1 || passes > EQ_MAX_PASSES) { set_error("equil_passes = %d: 1 .. %d (0: no equilibration)", passes, EQ_MAX_PASSES); return FOS_EINVAL; }
    FOS_TRY(cone_table_check("K1", m, nK1, K1type, K1start, K1len));
    FOS_TRY(cone_table_check("K2", n, nK2, K2type, K2start, K2len));
    if (colptr[0] != 1) { set_error("colptr[0] = %lld: the CSC arrays are 1-based", (long long)colptr[0]); return FOS_EINVAL; }
    for (int64_t j = 0; j < n; ++j)
        if (colptr[j + 1] < colptr[j]) { set_error("colptr decreases at column %lld", (long long)j + 1); return FOS_EINVAL; }
    const int64_t nnz = colptr[n] - 1;
    for (int64_t k = 0; k < nnz; ++k)
        if (rowval[k] < 1 || rowval[k] > m) { set_error("rowval[%lld] = %lld outside 1..%lld", (long long)k, (long long)rowval[k], (long long)m); return FOS_EINVAL; }

    std::vector<double> D((size_t)m, 1.0), E((size_t)n, 1.0), r((size_t)m), cn((size_t)n);
    for (int pass = 0; pass < passes; ++pass) {
        // A^ = (D A) E from the ORIGINAL values, every pass anew: the rounding of an entry does not depend on how many passes went before
        std::fill(r.begin(), r.end(), 0.0);
        std::fill(cn.begin(), cn.end(), 0.0);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t k = colptr[j] - 1; k < colptr[j + 1] - 1; ++k) {
                const int64_t i = rowval[k] - 1;
                const double a = std::fabs((D[i] * nzval[k]) * E[j]);
                r[i] = std::max(r[i], a);
                cn[j] = std::max(cn[j], a);
            }
        for (double& v : r) if (v == 0.0) v = 1.0;           // an empty row / column keeps its factor
        for (double& v : cn) if (v == 0.0) v = 1.0;
        cone_means(r, nK1, K1type, K1start, K1len);
        cone_means(cn, nK2, K2type, K2start, K2len);
        for (int64_t i = 0; i < m; ++i) D[i] /= std::sqrt(r[i]);
        for (int64_t j = 0; j < n; ++j) E[j] /= std::sqrt(cn[j]);
    }
    // gamma: |A^|_F^2 = min(m, n), the mean square singular value 1
    double fro2 = 0.0;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t k = colptr[j] - 1; k < colptr[j + 1] - 1; ++k) {
            const double a = (D[rowval[k] - 1] * nzval[k]) * E[j];
            fro2 += a * a;
        }
    const double gamma = fro2 > 0.0 ? std::sqrt((double)std::min(m, n)) / std::sqrt(fro2) : 1.0;
    for (double& v : D) v *= gamma;
    for (int64_t i = 0; i < m; ++i)
        if (!(D[i] > 0.0) || !std::isfinite(D[i])) { set_error("equilibration: row factor %lld is %g (entries of A that are not finite?)", (long long)i + 1, D[i]); return FOS_EINVAL; }
    for (int64_t j = 0; j < n; ++j)
        if (!(E[j] > 0.0) || !std::isfinite(E[j])) { set_error("equilibration: column factor %lld is %g (entries of A that are not finite?)", (long long)j + 1, E[j]); return FOS_EINVAL; }

    out->passes = passes;
    out->gamma = gamma;
    out->nz.resize((size_t)nnz);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t k = colptr[j] - 1; k < colptr[j + 1] - 1; ++k) out->nz[k] = (D[rowval[k] - 1] * nzval[k]) * E[j];
    out->b.resize((size_t)m);
    out->c.resize((size_t)n);
    double nb2 = 0.0, nc2 = 0.0;
    for (int64_t i = 0; i < m; ++i) { out->b[i] = D[i] * b[i]; nb2 += out->b[i] * out->b[i]; }
    for (int64_t j = 0; j < n; ++j) { out->c[j] = E[j] * c[j]; nc2 += out->c[j] * out->c[j]; }
    out->sigma = nb2 > 0.0 ? EQ_TARGET_NORM / std::sqrt(nb2) : 1.0;
    out->rho = nc2 > 0.0 ? EQ_TARGET_NORM / std::sqrt(nc2) : 1.0;
    if (!std::isfinite(out->sigma) || !std::isfinite(out->rho)) { set_error("equilibration: b or c has entries that are not finite"); return FOS_EINVAL; }
    for (double& v : out->b) v *= out->sigma;
    for (double& v : out->c) v *= out->rho;
    out->D.swap(D);
    out->E.swap(E);
    return FOS_OK;
}

}  // namespace fos

extern "C" int fos_host_equilibrate(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, const double* c,
                                    int64_t nK1, const int32_t* K1type, const int64_t* K1start, const int64_t* K1len,
                                    int64_t nK2, const int32_t* K2type, const int64_t* K2start, const int64_t* K2len,
                                    int32_t passes, double* D, double* E, double* scal3, double* nz_out, double* b_out, double* c_out) {
    fos::EqScaling s;
    FOS_TRY(fos::host_equilibrate(m, n, colptr, rowval, nzval, b, c, nK1, K1type, K1start, K1len, nK2, K2type, K2start, K2len, passes, &s));
    if (D) std::copy(s.D.begin(), s.D.end(), D);
    if (E) std::copy(s.E.begin(), s.E.end(), E);
    if (scal3) { scal3[0] = s.sigma; scal3[1] = s.rho; scal3[2] = s.gamma; }
    if (nz_out) std::copy(s.nz.begin(), s.nz.end(), nz_out);
    if (b_out) std::copy(s.b.begin(), s.b.end(), b_out);
    if (c_out) std::copy(s.c.begin(), s.c.end(), c_out);
    return FOS_OK;
}
