// The reference's three wrappers -- wrappers/linesearch.jl, solvers/gapproj.jl, wrappers/longstep.jl + saveplanes.jl -- for both problem forms: one state
// (Wrappers: one member of fos_solver, one of fos_feas), one set-up path and the LongstepWrapper's projection (wrappers.cpp), one search loop per wrapper
// (the two templates below, instantiated by solver.cpp and feas.hip over a form adapter).
#pragma once

#include <cmath>
#include <functional>

#include "fos_internal.hpp"

namespace fos {

struct Wrappers {
    int64_t ls_interval = 0;           // LineSearchWrapper: every ls_interval-th iteration is a 31-point step-length search (0: off)
    double ls_log[34] = {0};           // last search: ||res||, the 31 test residuals, the chosen alpha, the iteration
    int64_t gapp_iproj = 0;            // GAPP: every gapp_iproj-th iteration is a 21-point projected search (0: off)
    double gapp_log[23] = {0};         // 21 test norms, alpha_best, iteration
    LongPlanes lp;                     // LongstepWrapper: the last nsave + 1 iterations of every interval save the two half-planes of their projections
    bool ls_now = false, gapp_now = false;     // the iteration in flight is a search (HSDE: between step_once and step_finish; lp.now is the LongstepWrapper's)
    // a fresh algorithm is unwrapped (the set_linesearch / set_gapp / set_longstep of the caller follow)
    void off() { ls_interval = gapp_iproj = lp.interval = lp.savepos = 0; ls_now = gapp_now = lp.now = false; }
    bool active() const { return ls_interval > 0 || gapp_iproj > 0 || lp.interval > 0; }
};

// ---- set-up (wrappers.cpp): what the six fos_[feas_]set_* entries and the six *_log entries share
enum WrapperKind { WRAP_LINESEARCH, WRAP_GAPP, WRAP_LONGSTEP };
// may wrapper `kind` be switched on (interval > 0; nsave: the LongstepWrapper's) around algorithm `alg` next to what `w` has on?  FOS_OK, or the refusal
// with its message.  sharded: the handle's sums cross ranks (the Feasibility form has no sharding: false)
int wrappers_check(const Wrappers& w, WrapperKind kind, int alg, bool sharded, int64_t interval, int64_t nsave);
// a zero-filled device buffer of `count` doubles, entered into the owner's list
using ZeroAlloc = std::function<int(double** out, size_t count)>;
// the LongstepWrapper on (interval > 0, checked) with the four plane buffers for rows of l double2 and `blocks` partial sums per reduction: replaced when nsave
// changed (freed and taken out of `owned`: a caller sweeping nsave must not pile buffers up), all four zero-filled; the budget of supports is read here
int long_setup(LongPlanes& lp, int64_t interval, int64_t nsave, size_t l, size_t blocks, hipStream_t stream, std::vector<void*>& owned, const ZeroAlloc& zeros);
int wrappers_copy_log(const double* log, size_t count, double* out);       // log == nullptr: the handle was NULL
// *out = sqrt of the sum of `count` partial sums on the device, read back and summed on the host in index order (the searches' norms, the Feasibility status)
int norm_of_partials(const double* partials, size_t count, hipStream_t stream, double* out);

// ---- the saving window, once for both step functions
inline bool long_window(LongPlanes& lp, int64_t i) {                        // longstep.jl:44-49: does iteration i save planes?
    lp.now = false;
    if (lp.interval > 0) {
        const int64_t savepos = (i - 1) % lp.interval - lp.interval + lp.nsave + 2;
        if (savepos > 0) lp.savepos = savepos;
        lp.now = lp.savepos > 0;
    }
    return lp.now;
}
// behind the step of a saving iteration: the window's last one projects the iterate onto the saved planes (savepos = -1 says so)      longstep.jl:53-58
inline int long_window_close(const LaunchCtx& c, LongPlanes& lp, double2* X, int64_t i) {
    if (lp.now && lp.savepos == lp.nsave + 1) {
        FOS_TRY(long_project_planes(c, lp, X, i));
        lp.savepos = -1;
    }
    lp.now = false;
    return FOS_OK;
}

// ---- the searches.  A form adapter F supplies
//   the vectors   x, tmp1, tmp2, res, tmp3, tmp4 (the scratch the form's algorithms leave free) and res_from (GAPP: where prox!(res, S1, tmp2) left its result),
//   relaxed_s1(in)          S1!(tmp2, in)              tmp2 = a1 prox_S1(in) + (1 - a1) in
//   relaxed_s2(out)         S2!(out, tmp2)             out  = a2 prox_S2(tmp2) + (1 - a2) tmp2
//   prox_s2(out, in)        prox!(out, S2, in)
//   axpy(out, base, a, dir) out = base + a dir ;       sub(out, a, b)   out = a - b
//   normdiff(a, b, &v)      v = ||a - b||, read back and summed on the host
// -- each the launches that form has always used (1.0 y + a r and y + a r need not round alike).  The status check sits before the search in both
// forms but at different places of their step functions, so it stays with the callers.

// LineSearchWrapper: x = S2!(S1!(tmp1)) is in place; the search along res = x - tmp1      linesearch.jl:49-70
template <class F>
int linesearch_search(F& f, double* log, int64_t i) {
    f.sub(f.res, f.x, f.tmp1);                                                      // res .= x .- tmp1     :49
    FOS_TRY(f.normdiff(f.x, f.tmp1, &log[0]));                                      // normres = norm(res)  :50
    double best = INFINITY, abest = 1.0, a = 0.1;                                   // :53-55
    for (int k = 0; k <= 30; ++k) {                                                 // :56
        a = a * 1.8;                                                                // :57
        f.axpy(f.x, f.tmp1, a, f.res);                                              // x .= tmp1 .+ a.*res  :58
        FOS_TRY(f.relaxed_s1(f.x));                                                 // S1!(tmp2, x, nostatus) :60
        FOS_TRY(f.relaxed_s2(f.tmp3));                                              // S2!(tmp3, tmp2, nostatus) :61
        double tr = 0.0;
        FOS_TRY(f.normdiff(f.x, f.tmp3, &tr));                                      // testres = normdiff(x, tmp3) :62
        log[1 + k] = tr;
        if (tr < best) { best = tr; abest = a; }                                    // :64-67
    }
    f.axpy(f.x, f.tmp1, abest, f.res);                                              // x .= tmp1 .+ abest.*res :70
    log[32] = abest; log[33] = (double)i;
    return FOS_OK;
}

// GAPP: tmp1 = P_S1 x and res_from = P_S1 P_S2 tmp1 are in place; leaves the new tmp1 in tmp3 and its S2 projection in tmp2      gapproj.jl:41-59
template <class F>
int gapp_search(F& f, double* log, int64_t i) {
    f.sub(f.res, f.res_from, f.tmp1);                                               // res .= res - tmp1         :41
    double normbest = INFINITY, abest = -1.0;                                       // :44-45
    for (int k = 0; k <= 20; ++k) {                                                 // :46
        const double at = std::ldexp(1.0, k);                                       // 2.0^k
        f.axpy(f.tmp3, f.tmp1, at, f.res);                                          // tmp3 .= tmp1 .+ at.*res
        FOS_TRY(f.prox_s2(f.tmp4, f.tmp3));                                         // prox!(tmp4, S2, tmp3)
        double nt = 0.0;
        FOS_TRY(f.normdiff(f.tmp4, f.tmp3, &nt));                                   // norm(tmp4 - tmp3)
        log[k] = nt;
        if (nt < normbest) { abest = at; normbest = nt; }
    }
    log[21] = abest; log[22] = (double)i;
    f.axpy(f.tmp3, f.tmp1, abest, f.res);                                           // tmp1 .= tmp1 .+ abest.*res :58
    return f.prox_s2(f.tmp2, f.tmp3);                                               // prox!(tmp2, S2, tmp1)     :59
}

}  // namespace fos
