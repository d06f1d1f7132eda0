// libfoship: the outer iteration of the HSDE handle -- the affine projection (its CG solve: cg.cpp; direct = true: direct.cpp), the cone projection, the status
// check, ONE description per algorithm (GAP/GAPA, FISTA, Dykstra) with the two drivers that run it (the plain step with its gated `post`, the LongstepWrapper's
// saving iteration), the searches' adapter, and the entries of include/foship.h that are only the step.  What a handle is: solver.cpp.
#include <cmath>

#include "fos_solver.hpp"

using namespace fos;

// ---- the step's switches.  Per handle, read when the handle is created (fos_create2):
void fos::step_read_switches(StepState& s) {
    s.shift_fuse = !(getenv("FOS_SHIFT_FUSE") && atoi(getenv("FOS_SHIFT_FUSE")) == 0);
    s.psd_fuse = !(getenv("FOS_PSD_FUSE") && atoi(getenv("FOS_PSD_FUSE")) == 0);
    s.relax_ew = !(getenv("FOS_RELAX_EW") && atoi(getenv("FOS_RELAX_EW")) == 0);
}
// ... and the one that is per PROCESS, read once, by the first projection that runs a CG solve (FOS_FUSED_RHS=0: prox_affine forms its right-hand side)
static bool fused_rhs_env() {
    static const bool on = !(getenv("FOS_FUSED_RHS") && atoi(getenv("FOS_FUSED_RHS")) == 0);
    return on;
}

namespace {

// prox!(y, S1::AffinePlusLinear, x) with the result left in h->SOL       affinepluslinear.jl:83-126
int prox_affine(fos_solver* h, const d2* x, const PostFn* post = nullptr, bool* post_ran = nullptr) {
    if (h->direct_exact()) return prox_affine_direct(h, x);
    RoctxRange range("fos:prox_affine (rhs build + warm-started CG over the KKT operator)");
    LaunchCtx c = h->ctx();
    StepState& s = h->step;
    // The right-hand side [x1 - Q x2; 0] (:94-95) costs a sweep over A, and CG starts with another one for rhs - M y (:32-33).
    // Since M [0; x2] = [-Q x2; -x2], rhs = x + M [0; x2] and the start residual is  x - M (y - [0; x2]) : ONE sweep, applied
    // to the warm start shifted by the input's second part, and rhs is never formed (FOS_FUSED_RHS=0: the two sweeps).
    const bool fused_rhs = fused_rhs_env();
    if (!fused_rhs) {
        int fr = 0;
        launch_q1(c, Q_RHS, x, 1, 1.0, h->RHS);                        // :94-95
        FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
        launch_q1_finalize(c, Q_RHS, x, 1, 1.0, h->RHS, fr);
    }
    if (s.firstrun) {                                                   // :101-104
        FOS_HIP(hipMemcpyAsync(h->SOL, x, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
        s.firstrun = false;
    }
    if (fused_rhs && !(s.shift_ready && x == h->X)) {
        const int po = prof_begin_other(h, 0);
        launch_shift_part2(c, h->RHS, h->SOL, x);                       // RHS buffer := y - [0; x2]
        prof_end(h, po);
    }
    s.shift_ready = false;                                              // (SOL changes below)
    // :108-112   tol = max(0.2^sqrt(i), size(A,2)*eps())
    const double eps = 2.220446049250313e-16;
    const bool at_floor = h->direct_form == DIRECT_CG;                  // direct = true by CG: the tolerance floor from the first call on
    double tol = std::max(at_floor ? 0.0 : std::pow(0.2, std::sqrt((double)s.prox_i)), (double)h->l_global * eps);
    s.prox_i += 1;                                                      // :114
    int64_t it = 0;
    const int64_t cap = at_floor ? 10000 : 1000;                   // (:115: 1000; the exact projection is given the default cap of conjugategradients.jl:31)
    CgCall call{h->SOL, fused_rhs ? x : h->RHS, tol, (int)cap, fused_rhs ? h->RHS : nullptr, post, post_ran};
    FOS_TRY(cg_solve(h, call, &it));                                    // :115-117 ; y aliases xinit (:106,:122)
    s.cgiter = it;                                                      // :121
    return FOS_OK;                                                      // :124 y2 .*= beta with beta = 1
}

// prox!(y, S2::DualConeProduct, x)                                        cones.jl:122-142
// ew_done: the elementwise cones were projected by the kernel that wrote `in` (launch_relax_ew)
int prox_cones(fos_solver* h, d2* out, const d2* in, const int32_t* gate = nullptr, bool ew_done = false) {
    RoctxRange range("fos:prox_cones (elementwise + SOC + Exp + batched PSD)");
    LaunchCtx c = h->ctx();
    c.gate = gate;
    ConeSet* cs = h->cones;
    const int po = (!ew_done || cs->nsoc > 0 || cs->nexp > 0) ? prof_begin_other(h, gate ? 1 : 0) : -1;
    cone_set_project_vector(cs, c, out, in, ew_done);
    prof_end(h, po);
    const int pe = (cs->npsd > 0 || cs->big) ? prof_begin(h, FOS_PROF_PSD, 0, h->prof_seen[FOS_PROF_PSD]++) : -1;
    FOS_TRY(cone_set_project_psd(cs, c, out, in));
    prof_end(h, pe);
    return check_launch("cone projection");
}

// the decision of checkstatus from its values                             HSDEStatus.jl:53-63
int32_t status_decide(const fos_check_result* res, double eps) {
    const double nb = res->norm_b, nc = res->norm_c, ctx = res->ctx, bty = res->bty, tau = res->tau;
    if (res->p <= eps * (1 + nb) && res->d <= eps * (1 + nc) &&
        res->g <= eps * (1 + std::fabs(ctx / tau) + std::fabs(bty / tau)))
        return FOS_STATUS_OPTIMAL;
    if (res->norm_axs <= eps * (-ctx / nc)) return FOS_STATUS_UNBOUNDED;
    if (res->norm_aty <= eps * (-bty / nb)) return FOS_STATUS_INFEASIBLE;
    return FOS_STATUS_CONTINUE;
}

// checkstatus(status, z, override=true) values + decision               HSDEStatus.jl:27-63
// The six sums of the problem the handle holds come first (a plain handle: the status sweep and its finalize).  On an equilibrated handle z is the SCALED
// problem's iterate and the sums are taken in the CALLER's units: w = Q^ [x^; y^; 0] (rows 0 .. n+m-1; its tau row is not read, so no finalize) feeds one
// kernel that forms them on the caller's A, b, c (equilibrate.hip), tau included; sigma and rho come in here (a plain handle: 1, and dividing by 1 is exact).
// At tau = 0 the sums, hence p, d and g, are Inf / NaN as the reference's divisions leave them.
int status_check(fos_solver* h, const d2* z, double eps, fos_check_result* res) {
    const bool eq = h->equilibrated();
    RoctxRange range(eq ? "fos:checkstatus_eq" : "fos:checkstatus");
    LaunchCtx c = h->ctx();
    if (eq) {
        launch_q1(c, Q_PLAIN_NOTAU, z, 0, 1.0, h->eq_w);
        launch_eq_status(c, z, h->eq_w, h->eq_cb, h->eq_inv, h->partials);
    } else {
        int fr = 0;
        launch_q1(c, Q_STATUS, z, 0, 1.0, nullptr);
        FOS_TRY(finish_reduce(h, c, c.S.npart, 6, 0, &fr, c.S.part_off));
        launch_status_finalize(c, z, fr);
    }
    FOS_TRY(poll_state(h));
    const double* s = h->st_host->stat;
    const double sg = eq ? h->eq_sigma : 1.0, rho = eq ? h->eq_rho : 1.0;
    const double tau = s[ST_TAU], kappa = s[ST_KAPPA] / (sg * rho);
    const double nb = eq ? h->eq_nb : h->nb, nc = eq ? h->eq_nc : h->nc;
    const double ctx = s[ST_CTX] / (sg * rho), bty = s[ST_BTY] / (sg * rho);
    res->p = std::sqrt(s[ST_RP2]) / sg / std::fabs(1 + nb);                              // :34
    res->d = std::sqrt(s[ST_RD2]) / rho / std::fabs(1 + nc);                             // :35
    res->ctx = ctx;                                                                      // :36
    res->bty = bty;                                                                      // :37
    res->g = std::fabs(ctx / tau + bty / tau) / (1 + std::fabs(ctx / tau) + std::fabs(bty / tau));   // :38
    res->kappa = kappa;
    res->tau = tau;
    res->norm_axs = std::sqrt(s[ST_AXS2]) / sg;
    res->norm_aty = std::sqrt(s[ST_ATY2]) / rho;
    res->norm_b = nb;
    res->norm_c = nc;
    res->cgiter = h->step.cgiter;
    res->cg_maxiter_hit = h->cg.hit_max_accum;
    h->cg.hit_max_accum = 0;
    res->status = status_decide(res, eps);
    return FOS_OK;
}

// ---- LineSearchWrapper(GAP / GAPA)                                   wrappers/linesearch.jl:36-75
// S1!(y, x) = a1 prox_S1(x) + (1 - a1) x ,  S2!(y, x) = a2 prox_S2(x) + (1 - a2) x   (gap.jl:42-59; GAPA: a1 = a2 = alpha12, gapa.jl:61-79)
void ls_relax(fos_solver* h, const LaunchCtx& c, d2* out, const d2* y, const d2* x, int which) {
    if (h->step.alg == FOS_ALG_GAPA) { launch_relax_a12(c, out, y, x); return; }
    const double a = which == 1 ? h->step.alpha1 : h->step.alpha2;
    launch_axpby(c, out, a, y, 1 - a, x);
}
// the searches' view of the handle (wrappers.hpp).  Scratch: Y = tmp1 (the point the search starts from), XOLD = res, W = tmp3 -- unused by GAP and GAPA; the
// line search's tmp2 is T1 with prox_S2's result in T2; GAPP's tmp2 is T2, its tmp4 T1, and prox!(res, S1, .) leaves its result in SOL
struct HsdeSearch {
    fos_solver* h; LaunchCtx c;
    d2 *x, *tmp1, *tmp2, *res, *tmp3, *tmp4; const d2* res_from;
    explicit HsdeSearch(fos_solver* h_) : h(h_), c(h_->ctx()), x(h_->X), tmp1(h_->Y), tmp2(h_->T2), res(h_->XOLD), tmp3(h_->W), tmp4(h_->T1), res_from(h_->SOL) {}
    int relaxed_s1(const d2* in) { FOS_TRY(prox_affine(h, in)); ls_relax(h, c, h->T1, h->SOL, in, 1); return FOS_OK; }
    int relaxed_s2(d2* out) { FOS_TRY(prox_cones(h, h->T2, h->T1)); ls_relax(h, c, out, h->T2, h->T1, 2); return FOS_OK; }
    int prox_s2(d2* out, const d2* in) { return prox_cones(h, out, in); }
    void axpy(d2* out, const d2* base, double a, const d2* dir) { launch_axpby(c, out, 1.0, base, a, dir); }
    void sub(d2* out, const d2* a, const d2* b) { launch_axpby(c, out, 1.0, a, -1.0, b); }
    int normdiff(const d2* a, const d2* b, double* out) { launch_normdiff(c, a, b); return norm_of_partials(c.partials, (size_t)c.vec_blocks, h->stream, out); }
};
int ls_begin(fos_solver* h, const d2** check_on) {
    HsdeSearch f(h);
    FOS_HIP(hipMemcpyAsync(h->Y, h->X, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));     // tmp1 .= x            :41
    FOS_TRY(f.relaxed_s1(h->X));                                                                    // S1!(tmp2, x)         :45
    FOS_TRY(prox_cones(h, h->T2, h->T1));                                                           // S2!(x, tmp2): prox + checkstatus :46
    *check_on = h->T2;
    return FOS_OK;
}
int ls_finish(fos_solver* h, int64_t i) {
    HsdeSearch f(h);
    ls_relax(h, f.c, h->X, h->T2, h->T1, 2);                                                        //   ... and its relaxation
    return linesearch_search(f, h->wr.ls_log, i);
}

// ---- GAPP, a search iteration                                       solvers/gapproj.jl:29-62
int gapp_begin(fos_solver* h, int64_t i, const d2** check_on) {
    HsdeSearch f(h);
    FOS_TRY(prox_affine(h, h->X));                                                                  // prox!(tmp1, S1, x)        :33
    FOS_HIP(hipMemcpyAsync(h->Y, h->SOL, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
    FOS_TRY(prox_cones(h, h->T2, h->Y));                                                            // prox!(tmp2, S2, tmp1)     :39
    FOS_TRY(prox_affine(h, h->T2));                                                                 // prox!(res, S1, tmp2)      :40
    FOS_TRY(gapp_search(f, h->wr.gapp_log, i));
    *check_on = h->T2;                                                                              // checkstatus(status, tmp2) :60
    return FOS_OK;
}
int gapp_finish(fos_solver* h) {
    launch_axpby(h->ctx(), h->X, h->step.alpha2, h->T2, 1 - h->step.alpha2, h->W);                  // x .= a2 tmp2 + (1-a2) tmp1 :61-62
    return FOS_OK;
}

// ---- the algorithms: what one outer iteration runs around its two projections, stated ONCE per algorithm.  Both drivers read it: the plain step (step_once,
// which hands everything behind S1 to the CG solve as gated `post` work) and the LongstepWrapper's saving iteration (long_begin / long_finish).  The step's
// last pass, behind the status check, is step_finish_launch.
struct StepDesc {
    int (*before_s1)(fos_solver*, const LaunchCtx&, int64_t i);   // launched in front of S1 (nullptr: nothing)
    const d2* s1_in;                                              // S1: prox!(SOL, S1, s1_in) -- the pair the saving iteration takes as its equality plane
    void (*between)(fos_solver*, const LaunchCtx&);               // from SOL to S2's input, in its plain form (GAP / GAPA have fused forms of it: step_once)
    d2 *s2_in, *s2_out;                                           // S2: prox!(s2_out, S2, s2_in) -- the pair of the inequality plane; checkstatus is taken on s2_out
};
StepDesc step_desc(fos_solver* h) {
    switch (h->step.alg) {
        case FOS_ALG_GAP:                                         // gap.jl:42-80
        case FOS_ALG_GAPA:                                        // gapa.jl:61-105
            return {nullptr, h->X,
                    [](fos_solver* h, const LaunchCtx& c) { ls_relax(h, c, h->T1, h->SOL, h->X, 1); },         // y = a1 y + (1-a1) x   gap.jl:48  gapa.jl:67
                    h->T1, h->T2};
        case FOS_ALG_FISTA:                                       // fista.jl:28-48
            return {[](fos_solver* h, const LaunchCtx&, int64_t i) -> int {
                        if (i == 1) FOS_HIP(hipMemcpyAsync(h->Y, h->X, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));   // :31-33
                        return FOS_OK;
                    },
                    h->Y,
                    [](fos_solver* h, const LaunchCtx& c) {
                        launch_axpby(c, h->T1, h->step.alpha, h->SOL, 1 - h->step.alpha, h->Y);                // :37
                        launch_copy(c, h->XOLD, h->X);                                                        // :39  xold .= x
                    },
                    h->T1, h->X};
        case FOS_ALG_DYKSTRA:                                     // dykstra.jl:25-36   (p = Y, q = XOLD)
            return {[](fos_solver* h, const LaunchCtx& c, int64_t) -> int { launch_add(c, h->W, h->X, h->Y); return FOS_OK; },   // x .+ p
                    h->W,
                    [](fos_solver* h, const LaunchCtx& c) {
                        launch_dykstra_corr(c, h->Y, h->X, h->SOL);                                           // p .= x .+ p .- y      :30
                        launch_add(c, h->W, h->SOL, h->XOLD);                                                 // y .+ q
                    },
                    h->W, h->X};
    }
    return {};
}

// ---- LongstepWrapper                                                 wrappers/longstep.jl:41-101, saveplanes.jl:13-35
int step_finish_launch(fos_solver* h, const LaunchCtx& c);
// addprojeq (which = 0) / addprojineq (which = 1): row i = (savepos - 1) (neq + nineq) + eqi (+ uneqi) + 1 with neq = nineq = 1     longstep.jl:69,88
void long_save(fos_solver* h, const LaunchCtx& c, int which, const d2* y, const d2* x) { fos::long_save_plane(c, h->wr.lp, which, y, x); }
// a saving iteration: the description run ungated and unfused, with the two planes taken where the reference's step calls addprojeq / addprojineq
// (gap.jl:47,57  gapa.jl:66,76  fista.jl:36,42  dykstra.jl:30,34)
int long_begin(fos_solver* h, const LaunchCtx& c, const StepDesc& d) {
    FOS_TRY(prox_affine(h, d.s1_in));
    long_save(h, c, 0, h->SOL, d.s1_in);
    d.between(h, c);
    return prox_cones(h, d.s2_out, d.s2_in);
}
int long_finish(fos_solver* h, int64_t i) {
    LaunchCtx c = h->ctx();
    const StepDesc d = step_desc(h);
    long_save(h, c, 1, d.s2_out, d.s2_in);
    FOS_TRY(step_finish_launch(h, c));
    FOS_TRY(long_window_close(c, h->wr.lp, h->X, i));
    if (h->wr.lp.savepos == -1) h->step.shift_ready = false;                  // (projected: the iterate changed behind the step's last kernel)
    return FOS_OK;
}

// prox!(.., S1, in) followed by `post` -- everything of the step behind the CG solve (relaxation, cone projection and, when no
// status check sits in between, the step's last pass).  `post` is handed to the solve, which enqueues it behind the first CG
// batch, gated, so that the GPU does not wait for the host to learn the iteration count (cg_solve); if the batch did not
// suffice the gated launches were no-ops: the host-side state they advanced is rolled back and `post` runs again, ungated.
int affine_then(fos_solver* h, const LaunchCtx& c, const d2* in, const PostFn& post) {
    const ConeSet::Mark cones = h->cones->mark();
    const size_t prof_used = h->prof_used;
    const int64_t psd_seen = h->prof_seen[FOS_PROF_PSD];
    const double fista_t = h->step.fista_t;
    bool ran = false;
    FOS_TRY(prox_affine(h, in, &post, &ran));
    if (!ran) {
        h->cones->rewind(cones); h->prof_seen[FOS_PROF_PSD] = psd_seen; h->step.fista_t = fista_t;
        // (event pairs recorded around no-op launches: forget them; the CG records of this solve stay)
        for (size_t k = prof_used; k < h->prof_used; ++k)
            if (h->prof_recs[k].cls == FOS_PROF_PSD || (h->prof_recs[k].cls == FOS_PROF_OTHER && h->prof_recs[k].j == 1)) h->prof_recs[k].cls = -1;
        FOS_TRY(post(c));
    }
    return FOS_OK;
}
// one outer iteration up to the status check; *check_on receives the vector checkstatus is evaluated on (the cone-feasible point)
int step_once(fos_solver* h, int64_t i, const d2** check_on, bool will_check, bool* finish_done) {
    LaunchCtx c = h->ctx();
    *finish_done = false;
    Wrappers& wr = h->wr;
    wr.ls_now = wr.ls_interval > 0 && (i % wr.ls_interval) == 0;                                    // linesearch.jl:39
    if (wr.ls_now) return ls_begin(h, check_on);
    wr.gapp_now = wr.gapp_iproj > 0 && (i % wr.gapp_iproj) == 0;                                    // gapproj.jl:34
    if (wr.gapp_now) return gapp_begin(h, i, check_on);
    const StepDesc d = step_desc(h);
    if (!d.s1_in) { set_error("unknown algorithm %d", h->step.alg); return FOS_EINVAL; }
    *check_on = d.s2_out;
    if (d.before_s1) FOS_TRY(d.before_s1(h, c, i));
    if (long_window(wr.lp, i)) return long_begin(h, c, d);                                          // longstep.jl:44-49
    // everything behind the CG solve of S1 -- and, when no status check sits in between, the step's last pass too -- is handed to the solve as its `post`
    // work (cg_solve): enqueued behind the first CG batch, gated, so that the GPU does not wait for the host to learn the iteration count
    const PostFn post = [h, &d, will_check](const LaunchCtx& cg) -> int {
        const StepState& s = h->step;                                      // (its switches are per handle: read at fos_create)
        const bool gap = s.alg == FOS_ALG_GAP, gapa = s.alg == FOS_ALG_GAPA;
        // GAP / DR, no status check in this step, every non-elementwise cone a PSD(64) cone with a basis from the last projection:
        // relaxation, projection and the step's last pass are ONE launch (PsdFuse, fos_internal.hpp)
        if (s.psd_fuse && gap && !will_check && !h->wr.active() && cone_set_can_fuse(*h->cones, cg)) {
            RoctxRange range("fos:relaxation + PSD projection + final pass (one launch)");
            const bool sh = leaves_shift(h);
            PsdFuse fz{};
            fz.sol = h->SOL; fz.xv = h->X; fz.shift = sh ? h->RHS : nullptr;
            fz.a1 = s.alpha1; fz.alpha = s.alpha; fz.alpha2 = s.alpha2;
            fz.ew_op = h->cones->ew_op; fz.l = h->l;
            const int pe = prof_begin(h, FOS_PROF_PSD, 0, h->prof_seen[FOS_PROF_PSD]++);
            FOS_TRY(cone_set_project_psd(h->cones, cg, h->T2, h->T1, &fz));
            prof_end(h, pe);
            h->step.shift_ready = sh;
            return check_launch("fused relaxation + PSD projection + final pass");
        }
        const bool fuse_ew = (gap || gapa) && s.relax_ew;                  // GAP / GAPA: the relaxation and the elementwise cones of S2 in one pass
        const int pg = cg.gate ? 1 : 0;
        int po = prof_begin_other(h, pg);
        if (fuse_ew) launch_relax_ew(cg, h->T1, h->T2, h->SOL, h->X, s.alpha1, gapa, h->cones->ew_op);
        else d.between(h, cg);
        prof_end(h, po);
        FOS_TRY(prox_cones(h, d.s2_out, d.s2_in, cg.gate, fuse_ew));
        if (!will_check) { po = prof_begin_other(h, pg); FOS_TRY(step_finish_launch(h, cg)); prof_end(h, po); }
        return FOS_OK;
    };
    FOS_TRY(affine_then(h, c, d.s1_in, post));
    *finish_done = !will_check;
    return FOS_OK;
}

// the part of the step after checkstatus
int step_finish(fos_solver* h, int64_t i) {
    LaunchCtx c = h->ctx();
    if (h->wr.ls_now) { h->wr.ls_now = false; return ls_finish(h, i); }
    if (h->wr.gapp_now) { h->wr.gapp_now = false; return gapp_finish(h); }
    if (h->wr.lp.now) return long_finish(h, i);
    return step_finish_launch(h, c);
}
int step_finish_launch(fos_solver* h, const LaunchCtx& c) {
    StepState& s = h->step;
    switch (s.alg) {
        case FOS_ALG_GAP:
            // (inside fos_step, CG projection: the kernel also leaves SOL - [0; X.y] in RHS for the next iteration's CG start)
            s.shift_ready = leaves_shift(h);
            launch_gap_final(c, h->X, h->T2, h->T1, s.alpha, s.alpha2, s.shift_ready ? h->RHS : nullptr, h->SOL);      // gap.jl:58,78
            return FOS_OK;
        case FOS_ALG_GAPA: {
            s.shift_ready = leaves_shift(h);
            launch_gapa_final(c, h->X, h->T2, h->T1, s.alpha, s.shift_ready ? h->RHS : nullptr, h->SOL);               // gapa.jl:77,96,103
            int fr = 0;
            FOS_TRY(finish_reduce(h, c, c.vec_blocks, 3, 0, &fr));
            launch_gapa_finalize(c, s.beta, fr);                                   // gapa.jl:96-101
            return FOS_OK;
        }
        case FOS_ALG_FISTA: {
            const double told = s.fista_t;                                         // fista.jl:44-46
            s.fista_t = (1 + std::sqrt(1 + 4 * told * told)) / 2;
            launch_fista_extrap(c, h->Y, h->X, h->XOLD, (told - 1) / s.fista_t);
            return FOS_OK;
        }
        case FOS_ALG_DYKSTRA:
            launch_dykstra_corr(c, h->XOLD, h->SOL, h->X);                         // q .= y .+ q .- x   dykstra.jl:34
            return FOS_OK;
    }
    return FOS_EINVAL;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI: the entries that are only the step
extern "C" {

int fos_set_alg(fos_handle h, int alg, double alpha, double alpha1, double alpha2, double beta) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    if (alg < FOS_ALG_GAP || alg > FOS_ALG_DYKSTRA) { set_error("unknown algorithm %d", alg); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    StepState& s = h->step;
    s.alg = alg; s.alpha = alpha; s.alpha1 = alpha1; s.alpha2 = alpha2; s.beta = beta;
    h->wr.off();                                                        // a fresh algorithm is unwrapped (fos_set_linesearch / _gapp / _longstep follow)
    s.fista_t = 1.0;                                                    // fista.jl:24
    // fresh *Data: alpha12 = 2.0 (gapa.jl:29); y = xold = 0 (fista.jl:24); p = q = 0 (dykstra.jl:21)
    DevState z;
    FOS_HIP(hipStreamSynchronize(h->stream));
    FOS_HIP(hipMemcpy(&z, h->st, sizeof(DevState), hipMemcpyDeviceToHost));
    z.alpha12 = 2.0;
    z.gapa_scl = 0.0;
    FOS_HIP(hipMemcpy(h->st, &z, sizeof(DevState), hipMemcpyHostToDevice));
    FOS_HIP(hipMemsetAsync(h->Y, 0, sizeof(d2) * h->l, h->stream));
    FOS_HIP(hipMemsetAsync(h->XOLD, 0, sizeof(d2) * h->l, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

int fos_reset_affine(fos_handle h) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    h->step.prox_i = 1; h->step.firstrun = true; h->step.cgiter = 0; h->cg.hit_max_accum = 0; h->cg.last_cg_pred = 0;
    h->step.firstrun2 = true;
    return FOS_OK;
}

int fos_step(fos_handle h, int64_t i_first, int64_t count, int64_t checki, double eps,
             int64_t* iters_done, int32_t* checked, fos_check_result* res) {
    if (!h || checki < 1 || count < 0) { set_error("bad fos_step arguments"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (checked) *checked = 0;
    int64_t done = 0;
    h->step.shift_ready = false;
    struct InStep { fos_solver* h; ~InStep() { h->step.in_step = false; h->step.shift_ready = false; } } in_step{h};
    h->step.in_step = true;
    for (int64_t i = i_first; done < count; ++i) {
        const d2* check_on = nullptr;
        const bool do_check = (i % checki) == 0;                         // HSDEStatus.jl:28
        bool finish_done = false;
        h->prof_step_on = h->prof && (h->prof_steps++ % h->prof_period) == 0;
        if (h->prof_step_on) h->prof_steps_sampled += 1;
        FOS_TRY(step_once(h, i, &check_on, do_check, &finish_done));
        fos_check_result r;
        if (do_check) {
            FOS_TRY(status_check(h, check_on, eps, &r));
            h->step.last_checked = check_on;
        }
        if (!finish_done) { const int po = prof_begin_other(h, 0); FOS_TRY(step_finish(h, i)); prof_end(h, po); }
        h->prof_step_on = false;
        ++done;
        if (do_check) {
            if (res) *res = r;
            if (checked) *checked = 1;
            break;
        }
    }
    if (iters_done) *iters_done = done;
    FOS_TRY(check_launch("fos_step"));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

// LineSearchWrapper(alg; lsinterval) around GAP (AP, DR) or GAPA: iterations i with i % lsinterval == 0 become a 31-point search of
// the step length along S2(S1(x)) - x; 0 switches it off.  fos_linesearch_log: what the reference prints during the last search.
int fos_set_linesearch(fos_handle h, int64_t lsinterval) {
    if (!h || lsinterval < 0) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_TRY(wrappers_check(h->wr, WRAP_LINESEARCH, h->step.alg, h->sharded() || h->row_sharded, lsinterval, 0));
    h->wr.ls_interval = lsinterval;
    return FOS_OK;
}
// GAPP(alpha, alpha1, alpha2; iproj) (solvers/gapproj.jl, README solver table): fos_set_alg(FOS_ALG_GAP, alpha, alpha1, alpha2) and then
// fos_set_gapp(iproj > 0): iterations i with i % iproj == 0 search 21 step lengths 2^k along P_S1(P_S2(P_S1 x)) - P_S1 x.
int fos_set_gapp(fos_handle h, int64_t iproj) {
    if (!h || iproj < 0) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_TRY(wrappers_check(h->wr, WRAP_GAPP, h->step.alg, h->sharded() || h->row_sharded, iproj, 0));
    h->wr.gapp_iproj = iproj;
    return FOS_OK;
}
// LongstepWrapper(alg; longinterval, nsave) around the algorithm set last (wrappers/longstep.jl:22-40): 0 switches it off
int fos_set_longstep(fos_handle h, int64_t longinterval, int64_t nsave) {
    if (!h || longinterval < 0 || nsave < 0) { set_error("bad argument"); return FOS_EINVAL; }
    if (longinterval == 0) { h->wr.lp.interval = 0; h->wr.lp.savepos = 0; return FOS_OK; }
    FOS_TRY(wrappers_check(h->wr, WRAP_LONGSTEP, h->step.alg, h->sharded() || h->row_sharded, longinterval, nsave));
    FOS_HIP(hipSetDevice(h->device));
    return long_setup(h->wr.lp, longinterval, nsave, (size_t)h->l, (size_t)h->vec_blocks, h->stream, h->owned, [h](double** out, size_t count) { return dev_zeros(h, out, count); });
}
// the last search / projection: fos_linesearch_log: ||res||, 31 test residuals, alpha, iteration; fos_gapp_log: 21 test norms, alpha, iteration; fos_longstep_log:
// iteration, active inequalities, largest KKT violation of the small dual, |x_new - x|, rows, supports tried, failed, projections given up
int fos_linesearch_log(fos_handle h, double* out34) { return wrappers_copy_log(h ? h->wr.ls_log : nullptr, 34, out34); }
int fos_gapp_log(fos_handle h, double* out23) { return wrappers_copy_log(h ? h->wr.gapp_log : nullptr, 23, out23); }
int fos_longstep_log(fos_handle h, double* out8) { return wrappers_copy_log(h ? h->wr.lp.log : nullptr, 8, out8); }

int fos_getsol(fos_handle h, double* z_out, int32_t force_check, double eps, fos_check_result* res) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(prox_affine(h, h->X));                       // prox!(tmp1, S1, x)
    FOS_TRY(prox_cones(h, h->T2, h->SOL));               // prox!(tmp2, S2, tmp1)
    if (force_check && res) {                                              // solverwrapper.jl:32-34
        FOS_TRY(status_check(h, h->T2, eps, res));
        h->step.last_checked = h->T2;
    }
    if (z_out) FOS_TRY(download_caller(h, z_out, h->T2));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

int fos_get_affine_state(fos_handle h, double* xinit, int64_t* i, int32_t* firstrun) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (xinit) FOS_TRY(download_plain(h, xinit, h->SOL));
    if (i) *i = h->step.prox_i;
    if (firstrun) *firstrun = h->step.firstrun ? 1 : 0;
    return FOS_OK;
}

int fos_set_affine_state(fos_handle h, const double* xinit, int64_t i) {
    if (!h || !xinit || i < 1) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(upload_plain(h, h->SOL, xinit));
    h->step.firstrun = false;
    h->step.prox_i = i;
    return FOS_OK;
}

// FISTAData (y, xold, t), DykstraData (p, q), GAPAData.alpha12: the algorithm's own state     fista.jl:15-25, dykstra.jl:12-23, gapa.jl:29
int fos_get_alg_state(fos_handle h, double* a, double* b, double* scal2) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (a) FOS_TRY(download_plain(h, a, h->Y));
    if (b) FOS_TRY(download_plain(h, b, h->XOLD));
    if (scal2) {
        FOS_TRY(poll_state(h));
        scal2[0] = h->step.fista_t;
        scal2[1] = h->st_host->alpha12;
    }
    return FOS_OK;
}

int fos_set_alg_state(fos_handle h, const double* a, const double* b, const double* scal2) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (a) FOS_TRY(upload_plain(h, h->Y, a));
    if (b) FOS_TRY(upload_plain(h, h->XOLD, b));
    if (scal2) {
        if (!(scal2[0] >= 1.0)) { set_error("fos_set_alg_state: FISTA's t is >= 1 (fista.jl:24,45), got %g", scal2[0]); return FOS_EINVAL; }
        h->step.fista_t = scal2[0];
        FOS_HIP(hipStreamSynchronize(h->stream));
        FOS_HIP(hipMemcpy(&h->st->alpha12, &scal2[1], sizeof(double), hipMemcpyHostToDevice));
    }
    return FOS_OK;
}

int fos_get_cgiter(fos_handle h, int64_t* cgiter) {
    if (!h || !cgiter) { set_error("NULL argument"); return FOS_EINVAL; }
    *cgiter = h->step.cgiter;
    return FOS_OK;
}

int fos_get_alpha12(fos_handle h, double* a) {
    if (!h || !a) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(poll_state(h));
    *a = h->st_host->alpha12;
    return FOS_OK;
}

int fos_get_prox_count(fos_handle h, int64_t* i) {
    if (!h || !i) { set_error("NULL argument"); return FOS_EINVAL; }
    *i = h->step.prox_i;
    return FOS_OK;
}

// ---- fine-grained entries ----------------------------------------------------------------------------

int fos_prox_affine(fos_handle h, double* y, const double* x) {
    if (!h || !y || !x) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(upload_plain(h, h->W, x));
    FOS_TRY(prox_affine(h, h->W));
    return download_plain(h, y, h->SOL);
}

int fos_hsdematrix_prox(fos_handle h, double* y, const double* x) {
    if (!h || !y || !x) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    LaunchCtx c = h->ctx();
    FOS_TRY(upload_plain(h, h->RHS, x));                               // rhs = x   HSDEAffine.jl:116
    if (h->step.firstrun2) {                                           // :109-112
        FOS_HIP(hipMemcpyAsync(h->SOL2, h->RHS, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
        h->step.firstrun2 = false;
    }
    const double eps = 2.220446049250313e-16;
    const double tol = (double)(2 * h->l_global) * eps;                // :106
    int64_t it = 0;
    CgCall call{h->SOL2, h->RHS, tol, 1000};
    call.predict = false;
    FOS_TRY(cg_solve(h, call, &it));                                   // :116 ; xinit .= y :119
    h->step.cgiter = it;
    // v = Q*u                                                          :122-124
    int fr = 0;
    launch_q1(c, Q_VFROMU, h->SOL2, 0, 1.0, h->W);
    FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
    launch_q1_finalize(c, Q_VFROMU, h->SOL2, 0, 1.0, h->W, fr);
    return download_plain(h, y, h->W);
}

int fos_prox_cones(fos_handle h, double* y, const double* x) {
    if (!h || !y || !x) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(upload_plain(h, h->W, x));
    FOS_TRY(prox_cones(h, h->T2, h->W));
    return download_plain(h, y, h->T2);
}

int fos_check(fos_handle h, const double* z, double eps, fos_check_result* res) {
    if (!h || !z || !res) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(upload_caller(h, h->W, z));
    return status_check(h, h->W, eps, res);
}

}  // extern "C"
