// The wrappers' host side, for both problem forms (wrappers.hpp): the set-up the fos_[feas_]set_* entries share, the LongstepWrapper's plane
// buffers, and its projection onto the saved planes -- the small dual QP in 113-bit arithmetic.  Nothing here names a handle type.
#include "wrappers.hpp"

#include <cstdlib>

namespace fos {

// ------------------------------------------------------------------------------------------------ set-up
int wrappers_check(const Wrappers& w, WrapperKind kind, int alg, bool sharded, int64_t interval, int64_t nsave) {
    if (interval == 0) return FOS_OK;                                              // switching off is always fine
    switch (kind) {
        case WRAP_LINESEARCH:
            if (alg != FOS_ALG_GAP && alg != FOS_ALG_GAPA) { set_error("this algorithm does not support line search (support_linesearch: GAP and GAPA only, solvers/defaults.jl:22)"); return FOS_EUNSUPPORTED; }
            // normres / normdiff (linesearch.jl:50,62) are GLOBAL norms; the search adds this rank's partial sums only
            if (sharded) { set_error("LineSearchWrapper is built for single-GPU handles only (its step-length scores are global norms)"); return FOS_EUNSUPPORTED; }
            // (a search iteration returns before the planes of a saving window are written: the two wrappers exclude each other, both ways)
            if (w.lp.interval > 0) { set_error("LineSearchWrapper inside a LongstepWrapper is not supported"); return FOS_EUNSUPPORTED; }
            return FOS_OK;
        case WRAP_GAPP:
            if (alg != FOS_ALG_GAP) { set_error("GAPP is GAP with a projected search: fos_set_alg(FOS_ALG_GAP, ...) first"); return FOS_EUNSUPPORTED; }
            if (sharded) { set_error("GAPP is built for single-GPU handles only (its test norms are global norms)"); return FOS_EUNSUPPORTED; }
            if (w.ls_interval > 0) { set_error("GAPP and the LineSearchWrapper exclude each other"); return FOS_EUNSUPPORTED; }
            if (w.lp.interval > 0) { set_error("GAPP inside a LongstepWrapper is not supported (fos_set_longstep(h, 0, 0) first)"); return FOS_EUNSUPPORTED; }
            return FOS_OK;
        case WRAP_LONGSTEP:
            if (alg == FOS_ALG_GAPP) { set_error("Algorithm alg does not support longstep (support_longstep(::GAPP) = false, gapproj.jl:83)"); return FOS_EUNSUPPORTED; }
            if (2 * (nsave + 1) > LONG_KMAX_ROWS) { set_error("LongstepWrapper: nsave <= %d (2 (nsave + 1) saved planes, small dual QP solved by enumeration)", LONG_KMAX_ROWS / 2 - 1); return FOS_EUNSUPPORTED; }
            if (interval < nsave + 1) { set_error("LongstepWrapper: longinterval must be at least nsave + 1 (every plane is written before it is read)"); return FOS_EINVAL; }
            if (sharded) { set_error("LongstepWrapper is built for single-GPU handles only (the planes' products are global sums)"); return FOS_EUNSUPPORTED; }
            if (w.ls_interval > 0 || w.gapp_iproj > 0) { set_error("LongstepWrapper around a LineSearchWrapper / GAPP is not supported"); return FOS_EUNSUPPORTED; }
            return FOS_OK;
    }
    return FOS_EINVAL;
}

int long_setup(LongPlanes& lp, int64_t interval, int64_t nsave, size_t l, size_t blocks, hipStream_t stream, std::vector<void*>& owned, const ZeroAlloc& zeros) {
    const size_t K = (size_t)(2 * (nsave + 1));
    if (!lp.P || lp.nsave != nsave) {
        FOS_HIP(hipStreamSynchronize(stream));
        double* P = reinterpret_cast<double*>(lp.P);
        for (double** old : {&P, &lp.bpart, &lp.dots, &lp.nu}) {                   // (a caller sweeping nsave must not pile buffers up)
            if (!*old) continue;
            auto it = std::find(owned.begin(), owned.end(), (void*)*old);
            if (it != owned.end()) owned.erase(it);
            (void)hipFree(*old);
            *old = nullptr;
        }
        lp.P = nullptr;
        // rows a saving window never wrote (the step entered in the middle of one) are zero planes, not uninitialised memory
        FOS_TRY(zeros(&P, K * 2 * l)); lp.P = reinterpret_cast<double2*>(P);
        FOS_TRY(zeros(&lp.bpart, K * blocks));
        FOS_TRY(zeros(&lp.dots, blocks * 2 * (LONG_KMAX_ROWS + 1)));
        FOS_TRY(zeros(&lp.nu, 2 * K));
    }
    lp.interval = interval; lp.nsave = nsave; lp.savepos = 0; lp.now = false;
    // budget of candidate supports: a COUNT only -- a wall-clock cut-off made the iterate sequence depend on the load of the machine (0 tries none: the failure path, tests)
    lp.max_supports = getenv("FOS_LONG_MAX_SUPPORTS") ? atoll(getenv("FOS_LONG_MAX_SUPPORTS")) : 4096;
    lp.log[7] = 0.0;
    return FOS_OK;
}

int wrappers_copy_log(const double* log, size_t count, double* out) {
    if (!log || !out) { set_error("NULL argument"); return FOS_EINVAL; }
    memcpy(out, log, sizeof(double) * count);
    return FOS_OK;
}
int norm_of_partials(const double* partials, size_t count, hipStream_t stream, double* out) {
    std::vector<double> part(count);
    FOS_HIP(hipMemcpyAsync(part.data(), partials, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
    FOS_HIP(hipStreamSynchronize(stream));
    double s = 0.0;
    for (double v : part) s += v;
    *out = std::sqrt(s);
    return FOS_OK;
}

// ------------------------------------------------------------------------------------------------ the LongstepWrapper's projection
// The projection of x onto {v : A v = b, C v >= d}, A = the first nsave + 1 saved rows, C = the others (saveplanes.jl:17-28 -- the rows are
// saved equality, inequality, equality, ... and split here into halves: the reference's behaviour, kept).  The reference hands the n-variable
// problem to QPDAS in BigFloat; the solution is v = x + P' nu with nu = (lambda, mu >= 0) the minimiser of the SMALL dual
//     1/2 nu' G nu - nu' (beta - P x),  G = P P'  (K = 2 (nsave + 1) <= 32 unknowns),
// solved on the host: the inequality multipliers by enumeration of their support (<= 2^16 candidate supports; each a K x K symmetric system
// by eigen-decomposition, singular ones -- parallel planes -- through the pseudo-inverse); a support is accepted when its multipliers are
// non-negative and the inequalities outside it hold.  Only G, P x and beta leave the device; x += P' nu runs there.
namespace {
// 113-bit arithmetic for the small dual QP of the LongstepWrapper (the reference solves it in BigFloat, saveplanes.jl:24)
typedef __float128 qreal;
inline qreal qabs(qreal x) { return x < 0 ? -x : x; }
inline qreal qsqrt(qreal x) {
    if (!(x > 0)) return 0;
    qreal y = (qreal)sqrtl((long double)x);
    y = (y + x / y) / 2; y = (y + x / y) / 2;
    return y;
}
void sym_eig_jacobi(int n, std::vector<qreal>& A, std::vector<qreal>& V) {      // A (n x n, row-major) -> eigenvalues on its diagonal, eigenvectors in the columns of V
    V.assign((size_t)n * n, (qreal)0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1;
    for (int sweep = 0; sweep < 80; ++sweep) {
        qreal off = 0, diag = 0;
        for (int i = 0; i < n; ++i) { diag += A[(size_t)i * n + i] * A[(size_t)i * n + i]; for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j]; }
        if (off <= (qreal)1e-64 * diag || off == 0) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const qreal apq = A[(size_t)p * n + q];
                if (apq == 0) continue;
                const qreal theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2 * apq);
                const qreal t = (theta >= 0 ? (qreal)1 : (qreal)-1) / (qabs(theta) + qsqrt(theta * theta + 1));
                const qreal cs = 1 / qsqrt(t * t + 1), sn = t * cs;
                for (int k = 0; k < n; ++k) {
                    const qreal akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = cs * akp - sn * akq; A[(size_t)k * n + q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const qreal apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = cs * apk - sn * aqk; A[(size_t)q * n + k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const qreal vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                    V[(size_t)k * n + p] = cs * vkp - sn * vkq; V[(size_t)k * n + q] = sn * vkp + cs * vkq;
                }
            }
    }
}
// nu_F = pinv(G_FF) c_F on the index set F, zero elsewhere.  Cholesky first (a few thousand 113-bit operations); a pivot below 1e-26 of the
// trace = dependent planes -> the pseudo-inverse through the eigendecomposition (eigenvalues below that cut dropped)
void long_solve_support(int K, const std::vector<qreal>& G, const std::vector<qreal>& cvec, const std::vector<int>& F, std::vector<qreal>& nu) {
    const int nf = (int)F.size();
    nu.assign((size_t)K, (qreal)0);
    if (nf == 0) return;
    std::vector<qreal> A((size_t)nf * nf), V;
    qreal tr = 0;
    for (int i = 0; i < nf; ++i) { for (int j = 0; j < nf; ++j) A[(size_t)i * nf + j] = G[(size_t)F[i] * K + F[j]]; tr += A[(size_t)i * nf + i]; }
    const qreal cut = (qreal)1e-26 * (tr > 0 ? tr : (qreal)1e-300);
    {
        std::vector<qreal> L(A);
        bool ok = true;
        for (int j = 0; j < nf && ok; ++j) {
            qreal dj = L[(size_t)j * nf + j];
            for (int k = 0; k < j; ++k) dj -= L[(size_t)j * nf + k] * L[(size_t)j * nf + k];
            if (!(dj > cut)) { ok = false; break; }
            const qreal ljj = qsqrt(dj);
            L[(size_t)j * nf + j] = ljj;
            for (int i = j + 1; i < nf; ++i) {
                qreal v = L[(size_t)i * nf + j];
                for (int k = 0; k < j; ++k) v -= L[(size_t)i * nf + k] * L[(size_t)j * nf + k];
                L[(size_t)i * nf + j] = v / ljj;
            }
        }
        if (ok) {
            std::vector<qreal> y((size_t)nf);
            for (int i = 0; i < nf; ++i) { qreal v = cvec[(size_t)F[i]]; for (int k = 0; k < i; ++k) v -= L[(size_t)i * nf + k] * y[(size_t)k]; y[(size_t)i] = v / L[(size_t)i * nf + i]; }
            for (int i = nf - 1; i >= 0; --i) { qreal v = y[(size_t)i]; for (int k = i + 1; k < nf; ++k) v -= L[(size_t)k * nf + i] * y[(size_t)k]; y[(size_t)i] = v / L[(size_t)i * nf + i]; }
            for (int i = 0; i < nf; ++i) nu[(size_t)F[i]] = y[(size_t)i];
            return;
        }
    }
    sym_eig_jacobi(nf, A, V);
    for (int e = 0; e < nf; ++e) {
        const qreal lam = A[(size_t)e * nf + e];
        if (!(lam > cut)) continue;
        qreal proj = 0;
        for (int i = 0; i < nf; ++i) proj += V[(size_t)i * nf + e] * cvec[(size_t)F[i]];
        proj /= lam;
        for (int i = 0; i < nf; ++i) nu[(size_t)F[i]] += V[(size_t)i * nf + e] * proj;
    }
}

// The small dual, on the host only: G = P P' (K x K, row-major) and c = beta - P x in, the multipliers out.  The first neq rows are equalities.  true: best_nu
// is the KKT point; false: none within the budget of max_supports candidate supports (best_nu is then not to be applied).  log[1..6]: active inequalities,
// KKT violation (relative to the problem's scale when it failed), |P' nu| (0 when it failed), rows, supports tried, failed; log[7] counts the failures.
bool long_dual_solve(int K, int neq, const std::vector<qreal>& G, const std::vector<qreal>& cvec, int64_t max_supports, std::vector<qreal>& best_nu, double* log) {
    const int nin = K - neq;
    qreal scale = 0;
    for (int a = 0; a < K; ++a) { const qreal v = qabs(cvec[(size_t)a]) + qsqrt(G[(size_t)a * K + a]); if (v > scale) scale = v; }
    if (!(scale > 0)) scale = (qreal)1e-300;
    std::vector<qreal> nu;
    best_nu.assign((size_t)K, (qreal)0);
    qreal best_viol = (qreal)INFINITY;
    int best_active = 0;
    int64_t tried = 0;
    std::vector<int> F;
    std::vector<qreal> gres((size_t)K);
    // one candidate support: solve, residuals g = G nu - c, KKT violation (equality residuals, negative multipliers inside the support, violated
    // inequalities outside it); true when it is the solution
    auto try_support = [&](uint32_t mask) {
        F.clear();
        for (int a = 0; a < neq; ++a) F.push_back(a);
        for (int j = 0; j < nin; ++j) if (mask & (1u << j)) F.push_back(neq + j);
        long_solve_support(K, G, cvec, F, nu);
        ++tried;
        qreal viol = 0;
        for (int a = 0; a < K; ++a) {
            qreal g = -cvec[(size_t)a];                                       // (G nu - c)_a = P_a v - beta_a
            for (int b2 = 0; b2 < K; ++b2) g += G[(size_t)a * K + b2] * nu[(size_t)b2];
            gres[(size_t)a] = g;
            qreal va;
            if (a < neq) va = qabs(g);
            else if (mask & (1u << (a - neq))) { const qreal gd = G[(size_t)a * K + a]; const qreal m2 = -nu[(size_t)a] * qsqrt(gd > 0 ? gd : (qreal)1e-300); va = qabs(g) > m2 ? qabs(g) : m2; }
            else va = -g;
            if (va > viol) viol = va;
        }
        if (viol < best_viol) { best_viol = viol; best_nu = nu; best_active = __builtin_popcount(mask); }
        return best_viol <= (qreal)1e-12 * scale;
    };
    // (i) an active-set walk from the empty support: drop the most negative multiplier, else add the most violated inequality -- a handful of
    //     solves when it ends at the solution (it is accepted by the same KKT test); (ii) otherwise the enumeration of all supports
    bool found = false;
    {
        uint32_t mask = 0;
        std::vector<uint32_t> seen;
        for (int it = 0; it < 4 * nin + 4 && !found && tried < max_supports; ++it) {
            if (std::find(seen.begin(), seen.end(), mask) != seen.end()) break;
            seen.push_back(mask);
            if (try_support(mask)) { found = true; break; }
            int drop = -1, add = -1;
            qreal worst_nu = 0, worst_g = 0;
            for (int j = 0; j < nin; ++j) {
                const int a = neq + j;
                if (mask & (1u << j)) { if (nu[(size_t)a] < worst_nu) { worst_nu = nu[(size_t)a]; drop = j; } }
                else if (gres[(size_t)a] < worst_g) { worst_g = gres[(size_t)a]; add = j; }
            }
            if (drop >= 0) mask &= ~(1u << drop);
            else if (add >= 0) mask |= 1u << add;
            else break;
        }
    }
    // (ii) bounded: inconsistent or dependent planes have NO support that passes the KKT test, and 2^nin solves in 113-bit arithmetic (each a
    // Jacobi eigen-decomposition when Cholesky rejects the block) would hold the step for minutes -- at most max_supports candidates, smallest
    // supports first in counting order (deterministic: the same problem projects, or does not, on every run)
    for (uint32_t mask = 0; !found && mask < (1u << nin) && tried < max_supports; ++mask) found = try_support(mask);
    log[1] = (double)best_active; log[4] = (double)K; log[5] = (double)tried;
    log[6] = found ? 0.0 : 1.0;
    if (!found) {
        // no KKT point of the small dual within the budget: the planes do not describe a projection -- the iterate stays as the wrapped
        // algorithm left it (the reference's QP solver throws here; a step that is not the projection must not be applied silently)
        log[7] += 1.0;                                                        // projections given up since set_longstep (the host mirrors warn when it grows)
        log[2] = (double)(best_viol / scale); log[3] = 0.0;
        return false;
    }
    qreal step2 = 0;                                                          // |P' nu|^2 = nu' G nu
    for (int a = 0; a < K; ++a) for (int b2 = 0; b2 < K; ++b2) step2 += best_nu[(size_t)a] * G[(size_t)a * K + b2] * best_nu[(size_t)b2];
    log[2] = (double)best_viol; log[3] = (double)qsqrt(step2 > 0 ? step2 : (qreal)0);
    return true;
}
}  // namespace

int long_project_planes(const LaunchCtx& c, LongPlanes& lp, double2* X, int64_t i) {
    const int K = (int)(2 * (lp.nsave + 1)), neq = (int)(lp.nsave + 1);
    const int nb = c.vec_blocks;
    const size_t W = 2 * (LONG_KMAX_ROWS + 1);                                // (hi, lo) pairs per workgroup
    std::vector<qreal> G((size_t)K * K, (qreal)0), Px((size_t)K, (qreal)0), beta((size_t)K, (qreal)0);
    std::vector<double> part((size_t)nb * W), bp((size_t)K * nb);
    for (int a = 0; a < K; ++a) {
        launch_long_dots(c, lp.P, K, a, X, lp.dots);
        FOS_HIP(hipMemcpyAsync(part.data(), lp.dots, sizeof(double) * part.size(), hipMemcpyDeviceToHost, c.stream));
        FOS_HIP(hipStreamSynchronize(c.stream));
        for (int k = 0; a + k < K; ++k) {
            qreal sacc = 0;
            for (int b = 0; b < nb; ++b) sacc += (qreal)part[(size_t)b * W + 2 * k] + (qreal)part[(size_t)b * W + 2 * k + 1];
            G[(size_t)a * K + a + k] = G[(size_t)(a + k) * K + a] = sacc;
        }
        qreal sx = 0;
        for (int b = 0; b < nb; ++b) sx += (qreal)part[(size_t)b * W + 2 * LONG_KMAX_ROWS] + (qreal)part[(size_t)b * W + 2 * LONG_KMAX_ROWS + 1];
        Px[(size_t)a] = sx;
    }
    FOS_HIP(hipMemcpyAsync(bp.data(), lp.bpart, sizeof(double) * bp.size(), hipMemcpyDeviceToHost, c.stream));
    FOS_HIP(hipStreamSynchronize(c.stream));
    // (the offsets b = (x - y).y are float64 sums in the reference too, longstep.jl:71-75: data of the QP, not part of its solution)
    for (int a = 0; a < K; ++a) { double sacc = 0.0; for (int b = 0; b < nb; ++b) sacc += bp[(size_t)a * nb + b]; beta[(size_t)a] = (qreal)sacc; }
    std::vector<qreal> cvec((size_t)K), best_nu;
    for (int a = 0; a < K; ++a) cvec[(size_t)a] = beta[(size_t)a] - Px[(size_t)a];
    lp.log[0] = (double)i;
    if (!long_dual_solve(K, neq, G, cvec, lp.max_supports, best_nu, lp.log)) return FOS_OK;
    std::vector<double> nu2((size_t)2 * K);                                   // multipliers as (hi, lo) pairs for the double-double update
    for (int a = 0; a < K; ++a) { const double hi = (double)best_nu[(size_t)a]; nu2[(size_t)2 * a] = hi; nu2[(size_t)2 * a + 1] = (double)(best_nu[(size_t)a] - (qreal)hi); }
    FOS_HIP(hipMemcpyAsync(lp.nu, nu2.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, c.stream));
    launch_long_apply(c, X, lp.P, K, lp.nu);                     // x .= longstep.tmp      longstep.jl:57
    FOS_HIP(hipStreamSynchronize(c.stream));                                 // (nu2 leaves scope)
    return FOS_OK;
}
void long_save_plane(const LaunchCtx& c, LongPlanes& lp, int which, const double2* y, const double2* x) {
    const int64_t row = 2 * (lp.savepos - 1) + which;
    launch_long_plane(c, lp.P + row * c.l, x, y, lp.bpart + row * c.vec_blocks);
}
}  // namespace fos

// test-only, host: the projection of x onto {v : P[0:neq] v = beta[0:neq], P[neq:] v >= beta[neq:]} through the same small dual as the device path, with
// G = P P' and P x formed in 113-bit arithmetic from the doubles; x_out = x + P' nu rounded once; log8 as fos_longstep_log (iteration 0, step = |P' nu|)
extern "C" int fos_host_long_project(int64_t n, int64_t neq, int64_t nin, const double* P, const double* beta, const double* x, int64_t max_supports,
                                     double* x_out, double* log8) {
    using fos::qreal;
    if (n < 1 || neq < 0 || nin < 0 || neq + nin < 1 || neq + nin > fos::LONG_KMAX_ROWS || nin > fos::LONG_KMAX_ROWS / 2 || !P || !beta || !x || !x_out || !log8) {
        fos::set_error("fos_host_long_project: n >= 1, 1 <= neq + nin <= %d, nin <= %d and non-NULL arrays are required", fos::LONG_KMAX_ROWS, fos::LONG_KMAX_ROWS / 2);
        return FOS_EINVAL;
    }
    const int K = (int)(neq + nin);
    std::vector<qreal> G((size_t)K * K), cvec((size_t)K), nu;
    for (int a = 0; a < K; ++a) {
        for (int b = a; b < K; ++b) {
            qreal s = 0;
            for (int64_t j = 0; j < n; ++j) s += (qreal)P[(size_t)a * n + j] * (qreal)P[(size_t)b * n + j];
            G[(size_t)a * K + b] = G[(size_t)b * K + a] = s;
        }
        qreal sx = 0;
        for (int64_t j = 0; j < n; ++j) sx += (qreal)P[(size_t)a * n + j] * (qreal)x[j];
        cvec[(size_t)a] = (qreal)beta[a] - sx;
    }
    for (int k = 0; k < 8; ++k) log8[k] = 0.0;
    const bool found = fos::long_dual_solve(K, (int)neq, G, cvec, max_supports, nu, log8);
    for (int64_t j = 0; j < n; ++j) {
        qreal v = (qreal)x[j];
        if (found) for (int a = 0; a < K; ++a) v += nu[(size_t)a] * (qreal)P[(size_t)a * n + j];
        x_out[j] = (double)v;
    }
    return FOS_OK;
}
