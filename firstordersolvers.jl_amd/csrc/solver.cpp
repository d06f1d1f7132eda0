// libfoship: handle life cycle, the affine projection (its CG solve: cg.cpp), the GAP/GAPA/FISTA/Dykstra step loops, the status
// check and the C ABI of include/foship.h.  Host C++ only orchestrates launches on ONE HIP stream; all data stays
// in HBM between fos_create and fos_destroy (the only transfers are N doubles at set/get-iterate and ~100 bytes of
// scalars per CG poll / convergence check).
#include <dlfcn.h>

#include <cmath>
#include <mutex>

#include "fos_solver.hpp"

namespace fos {
const char* last_error_cstr();

// ------------------------------------------------------------------------------------------------ roctx ranges
// Named ranges around the phases of an outer iteration (affine projection / cone projection / status check) for
// `rocprofv3 --marker-trace`.  Resolved by dlopen at first use and only when FOS_ROCTX=1: no link-time dependency, no cost
// otherwise (one predictable branch per phase).
struct Roctx {
    int state = 0;                         // 0: not tried, 1: on, -1: off
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
static Roctx g_roctx;
static bool roctx_on() {
    if (g_roctx.state == 0) {
        g_roctx.state = -1;
        const char* e = getenv("FOS_ROCTX");
        if (e && atoi(e) != 0) {
            const char* names[] = {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"};
            for (const char* nm : names) {
                void* lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
                if (!lib) continue;
                g_roctx.push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
                g_roctx.pop = (int (*)())dlsym(lib, "roctxRangePop");
                if (g_roctx.push && g_roctx.pop) { g_roctx.state = 1; break; }
            }
        }
    }
    return g_roctx.state == 1;
}

RoctxRange::RoctxRange(const char* name) : on(roctx_on()) { if (on) g_roctx.push(name); }
RoctxRange::~RoctxRange() { if (on) g_roctx.pop(); }

// a kernel launch that the runtime rejected (bad configuration, missing attribute) is only reported by hipGetLastError
int check_launch(const char* where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: a kernel launch failed: %s", where, hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}

// profiling: a launch group whose ordinal (CG: the iteration's number counted over all solves since fos_create, so that every
// position inside a solve gets sampled; PSD: the call's number) is a multiple of prof_period is bracketed by an event pair
int prof_begin(fos_solver* h, int cls, int j, int64_t ordinal) {
    if (!h->prof) return -1;
    if ((ordinal % h->prof_period) != 0 || h->prof_used >= fos_solver::PROF_CAP) return -1;
    if (h->prof_recs.size() <= h->prof_used) {
        fos_solver::ProfRec r{};
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return -1;
        h->prof_recs.push_back(r);
    }
    fos_solver::ProfRec& r = h->prof_recs[h->prof_used];
    r.cls = cls; r.j = j;
    if (hipEventRecord(r.a, h->stream) != hipSuccess) return -1;
    return (int)h->prof_used++;
}
// FOS_PROF_OTHER: a launch group that is neither sweep, CG vector update nor PSD projection, in a sampled outer iteration; post = 1: the group
// belongs to the work enqueued (gated) behind a CG solve -- dropped with it when the gate stayed shut (affine_then)
int prof_begin_other(fos_solver* h, int post) {
    if (!h->prof || !h->prof_step_on) return -1;
    return prof_begin(h, FOS_PROF_OTHER, post, 0);
}
void prof_end(fos_solver* h, int idx) {
    if (idx >= 0) (void)hipEventRecord(h->prof_recs[idx].b, h->stream);
}

int poll_state(fos_solver* h) {
    FOS_TRY(check_launch("poll"));
    FOS_HIP(hipMemcpyAsync(h->st_host, h->st, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    if (h->st_host->xchg_failed) {
        set_error("rank %d: a peer-mailbox exchange timed out (a peer rank stopped or is not running the same call sequence)", h->rank);
        return FOS_ECOMM;
    }
    if (h->st_host->bar_failed) {
        set_error("a wait between the workgroups of one launch timed out (cg_update_kernel's producer flags: FOS_CG_PRE=0 switches them off; "
                  "the resident CG solve's records: FOS_CG_VARIANT=3 runs the launch-per-iteration form)");
        return FOS_EHIP;
    }
    return FOS_OK;
}

// out = [I Q'; Q -I] w, all l rows (sweep + tau-row finalize)
// deferred = false: the slot-spread rows of `out` (rows of A' under dual tiles) are not finished; tau_row = false: nor is the tau row -- for callers that
// need neither (the block-direct projection: single-GPU handles only)
int kkt_apply_full(fos_solver* h, const LaunchCtx& c, const d2* w, d2* out, bool deferred, bool tau_row) {
    launch_kkt2(c, w, out, 0, deferred || tau_row);          // (the tau-row kernel reads the records the deferred-row kernel leaves)
    if (!tau_row) return FOS_OK;
    int fr = 0;
    FOS_TRY(finish_reduce(h, c, c.S.npart, 3, 0, &fr, c.S.part_off));
    launch_kkt_finalize(c, w, out, 0, fr);
    return FOS_OK;
}

// UNCACHED device memory (the mailboxes, the relay and vector-exchange buffers, the resident solve's record arrays) is kept for the life of the
// process and handed from handle to handle, never returned to the runtime: on this image (ROCm 7.2), device memory that had been allocated
// uncached, freed, and handed out again by a later hipMalloc gave a WRONG dense IndAffine set-up several handles later (deterministic;
// DESIGN_LOG.md "the recycled uncached pages") -- so these pages are never recycled as anything else.  A block serves a later request of
// the same device for at most its own size and at least half of it.
namespace {
struct UncachedBlock { int device; void* p; size_t bytes; bool uncached; };
std::mutex g_unc_mu;
std::vector<UncachedBlock> g_unc_free, g_unc_used;
}
// falls back to fine-grained memory (what the mailboxes accept), or with `allow_plain` (the records: cache-bypassing accesses work on any
// memory) to ordinary memory
int uncached_acquire(int device, size_t bytes, bool allow_plain, void** out, const char* what) {
    UncachedBlock r{device, nullptr, 0, false};
    {
        std::lock_guard<std::mutex> lk(g_unc_mu);
        for (size_t i = 0; i < g_unc_free.size(); ++i) {
            const UncachedBlock& f = g_unc_free[i];
            if (f.device == device && f.bytes >= bytes && f.bytes / 2 <= bytes) { r = f; g_unc_free.erase(g_unc_free.begin() + (long)i); break; }
        }
    }
    if (!r.p) {
        static const bool unc = !(getenv("FOS_RES_UNCACHED") && atoi(getenv("FOS_RES_UNCACHED")) == 0);
        hipError_t e = (unc || !allow_plain) ? hipExtMallocWithFlags(&r.p, bytes, hipDeviceMallocUncached) : hipErrorUnknown;
        r.uncached = (e == hipSuccess);
        if (e != hipSuccess && !allow_plain) { (void)hipGetLastError(); e = hipExtMallocWithFlags(&r.p, bytes, hipDeviceMallocFinegrained); }
        if (e != hipSuccess && allow_plain) { (void)hipGetLastError(); e = hipMalloc(&r.p, bytes); }
        if (e != hipSuccess) { set_error("hipExtMallocWithFlags(%s, %zu bytes): %s", what, bytes, hipGetErrorString(e)); return FOS_ENOMEM; }
        r.bytes = bytes;
    }
    { std::lock_guard<std::mutex> lk(g_unc_mu); g_unc_used.push_back(r); }
    *out = r.p;
    return FOS_OK;
}
static void uncached_release(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_unc_mu);
    for (size_t i = 0; i < g_unc_used.size(); ++i)
        if (g_unc_used[i].p == p) { g_unc_free.push_back(g_unc_used[i]); g_unc_used.erase(g_unc_used.begin() + (long)i); return; }
}

// sharded set-up: global problem size and norms (tolerance floor, status normalisation) from the shards'
int global_setup(fos_solver* h) {
    // the resident CG solve runs on a sharded handle only where EVERY rank's shard qualifies (all ranks must run the same exchanges) and
    // the sums cross the ranks through mailboxes (no collective call can sit inside a kernel): a vote through the handle's transport
    FOS_TRY(resident_setup(h, (h->tr.peer_same_device && h->nranks > 1) ? std::max(1, h->cus / h->nranks) : h->cus));
    h->op.res_all = false;
    if (h->tr.peer_on) {
        LaunchCtx cv = h->ctx();
        double q = h->op.res_ok ? 1.0 : 0.0;
        FOS_HIP(hipMemcpyAsync(h->partials, &q, sizeof(q), hipMemcpyHostToDevice, h->stream));
        launch_reduce1(cv, 1, 1, 0);
        FOS_TRY(allreduce(h, 1));
        FOS_HIP(hipMemcpyAsync(&q, h->reduced, sizeof(q), hipMemcpyDeviceToHost, h->stream));
        FOS_TRY(poll_state(h));
        h->op.res_all = q == (double)h->nranks;
    }
    LaunchCtx c = h->ctx();
    const bool cnt = !h->row_sharded || h->rank == 0;     // row-sharded: the n columns and c are replicated, counted by rank 0
    double loc[3] = {(double)(h->m + (cnt ? h->n : 0)), h->nb_local * h->nb_local, cnt ? h->nc_local * h->nc_local : 0.0};
    FOS_HIP(hipMemcpyAsync(h->partials, loc, sizeof(loc), hipMemcpyHostToDevice, h->stream));
    launch_reduce1(c, 1, 3, 0);
    FOS_TRY(allreduce(h, 3));
    FOS_HIP(hipMemcpyAsync(loc, h->reduced, sizeof(loc), hipMemcpyDeviceToHost, h->stream));
    FOS_TRY(poll_state(h));
    h->l_global = (int64_t)std::llround(loc[0]) + 1;
    h->nb = std::sqrt(loc[1]);
    h->nc = std::sqrt(loc[2]);
    return FOS_OK;
}

int upload_plain(fos_solver* h, d2* dst, const double* z) {
    LaunchCtx c = h->ctx();
    FOS_HIP(hipMemcpyAsync(h->plain, z, sizeof(double) * 2 * h->l, hipMemcpyHostToDevice, h->stream));
    launch_interleave(c, dst, h->plain);
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}
int download_plain(fos_solver* h, double* z, const d2* src) {
    LaunchCtx c = h->ctx();
    launch_deinterleave(c, h->plain, src);
    FOS_HIP(hipMemcpyAsync(z, h->plain, sizeof(double) * 2 * h->l, hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

}  // namespace fos

using namespace fos;

namespace {

// prox!(y, S1::AffinePlusLinear, x) with the result left in h->SOL       affinepluslinear.jl:83-126
int prox_affine(fos_solver* h, const d2* x, const PostFn* post = nullptr, bool* post_ran = nullptr) {
    if (h->direct_exact()) return prox_affine_direct(h, x);
    RoctxRange range("fos:prox_affine (rhs build + warm-started CG over the KKT operator)");
    LaunchCtx c = h->ctx();
    // The right-hand side [x1 - Q x2; 0] (:94-95) costs a sweep over A, and CG starts with another one for rhs - M y (:32-33).
    // Since M [0; x2] = [-Q x2; -x2], rhs = x + M [0; x2] and the start residual is  x - M (y - [0; x2]) : ONE sweep, applied
    // to the warm start shifted by the input's second part, and rhs is never formed (FOS_FUSED_RHS=0: the two sweeps).
    static const bool fused_rhs = !(getenv("FOS_FUSED_RHS") && atoi(getenv("FOS_FUSED_RHS")) == 0);
    if (!fused_rhs) {
        int fr = 0;
        launch_q1(c, Q_RHS, x, 1, 1.0, h->RHS);                        // :94-95
        FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
        launch_q1_finalize(c, Q_RHS, x, 1, 1.0, h->RHS, fr);
    }
    if (h->firstrun) {                                                  // :101-104
        FOS_HIP(hipMemcpyAsync(h->SOL, x, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
        h->firstrun = false;
    }
    if (fused_rhs && !(h->shift_ready && x == h->X)) {
        const int po = prof_begin_other(h, 0);
        launch_shift_part2(c, h->RHS, h->SOL, x);                       // RHS buffer := y - [0; x2]
        prof_end(h, po);
    }
    h->shift_ready = false;                                             // (SOL changes below)
    // :108-112   tol = max(0.2^sqrt(i), size(A,2)*eps())
    const double eps = 2.220446049250313e-16;
    const bool at_floor = h->direct_form == DIRECT_CG;                  // direct = true by CG: the tolerance floor from the first call on
    double tol = std::max(at_floor ? 0.0 : std::pow(0.2, std::sqrt((double)h->prox_i)), (double)h->l_global * eps);
    h->prox_i += 1;                                                     // :114
    int64_t it = 0;
    const int64_t cap = at_floor ? 10000 : 1000;                   // (:115: 1000; the exact projection is given the default cap of conjugategradients.jl:31)
    CgCall call{h->SOL, fused_rhs ? x : h->RHS, tol, (int)cap, fused_rhs ? h->RHS : nullptr, post, post_ran};
    FOS_TRY(cg_solve(h, call, &it));                                    // :115-117 ; y aliases xinit (:106,:122)
    h->cgiter = it;                                                     // :121
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
static int32_t status_decide(const fos_check_result* res, double eps) {
    const double nb = res->norm_b, nc = res->norm_c, ctx = res->ctx, bty = res->bty, tau = res->tau;
    if (res->p <= eps * (1 + nb) && res->d <= eps * (1 + nc) &&
        res->g <= eps * (1 + std::fabs(ctx / tau) + std::fabs(bty / tau)))
        return FOS_STATUS_OPTIMAL;
    if (res->norm_axs <= eps * (-ctx / nc)) return FOS_STATUS_UNBOUNDED;
    if (res->norm_aty <= eps * (-bty / nb)) return FOS_STATUS_INFEASIBLE;
    return FOS_STATUS_CONTINUE;
}

// The same on an equilibrated handle, in the CALLER's units: z is the scaled problem's iterate; w = Q^ [x^; y^; 0] (rows 0 .. n+m-1; its tau row is not read, so
// no finalize) feeds one kernel that forms the six sums on the caller's A, b, c (equilibrate.hip), tau included; sigma and rho come in here.  At tau = 0 the
// sums, hence p, d and g, are Inf / NaN as the reference's divisions leave them.
static int eq_status_check(fos_solver* h, const d2* z, double eps, fos_check_result* res) {
    RoctxRange range("fos:checkstatus_eq");
    LaunchCtx c = h->ctx();
    launch_q1(c, Q_PLAIN_NOTAU, z, 0, 1.0, h->eq_w);
    launch_eq_status(c, z, h->eq_w, h->eq_cb, h->eq_inv, h->partials);
    FOS_TRY(poll_state(h));
    const double* s = h->st_host->stat;
    const double sg = h->eq_sigma, rho = h->eq_rho;
    const double tau = s[ST_TAU], kappa = s[ST_KAPPA] / (sg * rho);
    const double nb = h->eq_nb, nc = h->eq_nc;
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
    res->cgiter = h->cgiter;
    res->cg_maxiter_hit = h->cg.hit_max_accum;
    h->cg.hit_max_accum = 0;
    res->status = status_decide(res, eps);
    return FOS_OK;
}

// checkstatus(status, z, override=true) values + decision               HSDEStatus.jl:27-63
int status_check(fos_solver* h, const d2* z, double eps, fos_check_result* res) {
    if (h->equilibrated()) return eq_status_check(h, z, eps, res);
    RoctxRange range("fos:checkstatus");
    LaunchCtx c = h->ctx();
    int fr = 0;
    launch_q1(c, Q_STATUS, z, 0, 1.0, nullptr);
    FOS_TRY(finish_reduce(h, c, c.S.npart, 6, 0, &fr, c.S.part_off));
    launch_status_finalize(c, z, fr);
    FOS_TRY(poll_state(h));
    const double* s = h->st_host->stat;
    const double tau = s[ST_TAU], kappa = s[ST_KAPPA];
    const double nb = h->nb, nc = h->nc;
    const double ctx = s[ST_CTX], bty = s[ST_BTY];
    res->p = std::sqrt(s[ST_RP2]) / std::fabs(1 + nb);                                   // :34
    res->d = std::sqrt(s[ST_RD2]) / std::fabs(1 + nc);                                   // :35
    res->ctx = ctx;                                                                      // :36
    res->bty = bty;                                                                      // :37
    res->g = std::fabs(ctx / tau + bty / tau) / (1 + std::fabs(ctx / tau) + std::fabs(bty / tau));   // :38
    res->kappa = kappa;
    res->tau = tau;
    res->norm_axs = std::sqrt(s[ST_AXS2]);
    res->norm_aty = std::sqrt(s[ST_ATY2]);
    res->norm_b = nb;
    res->norm_c = nc;
    res->cgiter = h->cgiter;
    res->cg_maxiter_hit = h->cg.hit_max_accum;
    h->cg.hit_max_accum = 0;
    res->status = status_decide(res, eps);
    return FOS_OK;
}

// ---- LineSearchWrapper(GAP / GAPA)                                   wrappers/linesearch.jl:36-75
// S1!(y, x) = a1 prox_S1(x) + (1 - a1) x ,  S2!(y, x) = a2 prox_S2(x) + (1 - a2) x   (gap.jl:42-59; GAPA: a1 = a2 = alpha12, gapa.jl:61-79)
void ls_relax(fos_solver* h, const LaunchCtx& c, d2* out, const d2* y, const d2* x, int which) {
    if (h->alg == FOS_ALG_GAPA) { launch_relax_a12(c, out, y, x); return; }
    const double a = which == 1 ? h->alpha1 : h->alpha2;
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
    launch_axpby(h->ctx(), h->X, h->alpha2, h->T2, 1 - h->alpha2, h->W);                            // x .= a2 tmp2 + (1-a2) tmp1 :61-62
    return FOS_OK;
}

// ---- LongstepWrapper                                                 wrappers/longstep.jl:41-101, saveplanes.jl:13-35
int step_finish_launch(fos_solver* h, const LaunchCtx& c);
// addprojeq (which = 0) / addprojineq (which = 1): row i = (savepos - 1) (neq + nineq) + eqi (+ uneqi) + 1 with neq = nineq = 1     longstep.jl:69,88
void long_save(fos_solver* h, const LaunchCtx& c, int which, const d2* y, const d2* x) { fos::long_save_plane(c, h->wr.lp, which, y, x); }
// a saving iteration: the step of the wrapped algorithm, unfused, with the two planes taken where the reference's step calls addprojeq /
// addprojineq (gap.jl:47,57  gapa.jl:66,76  fista.jl:36,42  dykstra.jl:30,34)
int long_begin(fos_solver* h, int64_t i, const d2** check_on) {
    LaunchCtx c = h->ctx();
    switch (h->alg) {
        case FOS_ALG_GAP:
        case FOS_ALG_GAPA:
            FOS_TRY(prox_affine(h, h->X));                                       // prox!(y, S1, x)
            long_save(h, c, 0, h->SOL, h->X);                                    // addprojeq(longstep, y, x)
            ls_relax(h, c, h->T1, h->SOL, h->X, 1);                              // y .= a1 y + (1 - a1) x
            FOS_TRY(prox_cones(h, h->T2, h->T1));                                // prox!(y, S2, x); checkstatus(status, y)
            *check_on = h->T2;
            return FOS_OK;
        case FOS_ALG_FISTA:
            if (i == 1) FOS_HIP(hipMemcpyAsync(h->Y, h->X, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
            FOS_TRY(prox_affine(h, h->Y));                                       // prox!(tmp1, S1, y)
            long_save(h, c, 0, h->SOL, h->Y);                                    // addprojeq(longstep, tmp1, y)
            launch_axpby(c, h->T1, h->alpha, h->SOL, 1 - h->alpha, h->Y);
            launch_copy(c, h->XOLD, h->X);
            FOS_TRY(prox_cones(h, h->X, h->T1));
            *check_on = h->X;
            return FOS_OK;
        case FOS_ALG_DYKSTRA:
            launch_add(c, h->W, h->X, h->Y);                                     // x .+ p
            FOS_TRY(prox_affine(h, h->W));                                       // prox!(y, S1, x .+ p)
            long_save(h, c, 0, h->SOL, h->W);                                    // addprojeq(longstep, y, x .+ p)
            launch_dykstra_corr(c, h->Y, h->X, h->SOL);                          // p .= x .+ p .- y
            launch_add(c, h->W, h->SOL, h->XOLD);                                // y .+ q
            FOS_TRY(prox_cones(h, h->X, h->W));                                  // prox!(x, S2, y .+ q)
            *check_on = h->X;
            return FOS_OK;
    }
    return FOS_EINVAL;
}
int long_finish(fos_solver* h, int64_t i) {
    LaunchCtx c = h->ctx();
    switch (h->alg) {
        case FOS_ALG_GAP:
        case FOS_ALG_GAPA: long_save(h, c, 1, h->T2, h->T1); break;           // addprojineq(longstep, y, x)
        case FOS_ALG_FISTA: long_save(h, c, 1, h->X, h->T1); break;           // addprojineq(longstep, x, tmp1)
        case FOS_ALG_DYKSTRA: long_save(h, c, 1, h->X, h->W); break;          // addprojineq(longstep, x, y .+ q)
    }
    FOS_TRY(step_finish_launch(h, c));
    FOS_TRY(long_window_close(c, h->wr.lp, h->X, i));
    if (h->wr.lp.savepos == -1) h->shift_ready = false;                       // (projected: the iterate changed behind the step's last kernel)
    return FOS_OK;
}

// one outer iteration; *check_on receives the vector checkstatus is evaluated on (the cone-feasible point)

// prox!(.., S1, in) followed by `post` -- everything of the step behind the CG solve (relaxation, cone projection and, when no
// status check sits in between, the step's last pass).  `post` is handed to the solve, which enqueues it behind the first CG
// batch, gated, so that the GPU does not wait for the host to learn the iteration count (cg_solve); if the batch did not
// suffice the gated launches were no-ops: the host-side state they advanced is rolled back and `post` runs again, ungated.
int affine_then(fos_solver* h, const LaunchCtx& c, const d2* in, const PostFn& post) {
    const ConeSet::Mark cones = h->cones->mark();
    const size_t prof_used = h->prof_used;
    const int64_t psd_seen = h->prof_seen[FOS_PROF_PSD];
    const double fista_t = h->fista_t;
    bool ran = false;
    FOS_TRY(prox_affine(h, in, &post, &ran));
    if (!ran) {
        h->cones->rewind(cones); h->prof_seen[FOS_PROF_PSD] = psd_seen; h->fista_t = fista_t;
        // (event pairs recorded around no-op launches: forget them; the CG records of this solve stay)
        for (size_t k = prof_used; k < h->prof_used; ++k)
            if (h->prof_recs[k].cls == FOS_PROF_PSD || (h->prof_recs[k].cls == FOS_PROF_OTHER && h->prof_recs[k].j == 1)) h->prof_recs[k].cls = -1;
        FOS_TRY(post(c));
    }
    return FOS_OK;
}
int step_once(fos_solver* h, int64_t i, const d2** check_on, bool will_check, bool* finish_done) {
    LaunchCtx c = h->ctx();
    *finish_done = false;
    Wrappers& wr = h->wr;
    wr.ls_now = wr.ls_interval > 0 && (i % wr.ls_interval) == 0;                                    // linesearch.jl:39
    if (wr.ls_now) return ls_begin(h, check_on);
    wr.gapp_now = wr.gapp_iproj > 0 && (i % wr.gapp_iproj) == 0;                                    // gapproj.jl:34
    if (wr.gapp_now) return gapp_begin(h, i, check_on);
    if (long_window(wr.lp, i)) return long_begin(h, i, check_on);                                   // longstep.jl:44-49
    switch (h->alg) {
        case FOS_ALG_GAP:                                                // gap.jl:61-80
        case FOS_ALG_GAPA: {                                             // gapa.jl:80-105
            // everything behind the CG solve of S1! -- and, when no status check sits in between, the final relaxation of
            // the step too -- is handed to the solve as its `post` work (cg_solve): enqueued behind the first CG batch,
            // gated, so that the GPU does not wait for the host to learn the iteration count
            const bool gapa = h->alg == FOS_ALG_GAPA;
            const PostFn post = [h, gapa, will_check](const LaunchCtx& cg) -> int {
                const bool fuse_ew = h->relax_ew, fuse_psd = h->psd_fuse;          // (per handle: read at fos_create)
                // GAP / DR, no status check in this step, every non-elementwise cone a PSD(64) cone with a basis from the last projection:
                // relaxation, projection and the step's last pass are ONE launch (PsdFuse, fos_internal.hpp)
                if (fuse_psd && !gapa && !will_check && !h->wr.active() && cone_set_can_fuse(*h->cones, cg)) {
                    RoctxRange range("fos:relaxation + PSD projection + final pass (one launch)");
                    const bool sh = h->in_step && h->shift_fuse && !h->direct_exact();
                    PsdFuse fz{};
                    fz.sol = h->SOL; fz.xv = h->X; fz.shift = sh ? h->RHS : nullptr;
                    fz.a1 = h->alpha1; fz.alpha = h->alpha; fz.alpha2 = h->alpha2;
                    fz.ew_op = h->cones->ew_op; fz.l = h->l;
                    const int pe = prof_begin(h, FOS_PROF_PSD, 0, h->prof_seen[FOS_PROF_PSD]++);
                    FOS_TRY(cone_set_project_psd(h->cones, cg, h->T2, h->T1, &fz));
                    prof_end(h, pe);
                    h->shift_ready = sh;
                    return check_launch("fused relaxation + PSD projection + final pass");
                }
                const int pg = cg.gate ? 1 : 0;
                int po = prof_begin_other(h, pg);
                if (fuse_ew) {                       // the relaxation and the elementwise cones of S2! in one pass
                    launch_relax_ew(cg, h->T1, h->T2, h->SOL, h->X, h->alpha1, gapa, h->cones->ew_op);
                    prof_end(h, po);
                    FOS_TRY(prox_cones(h, h->T2, h->T1, cg.gate, true));
                } else {
                if (gapa) launch_relax_a12(cg, h->T1, h->SOL, h->X);                          // gapa.jl:67
                else launch_axpby(cg, h->T1, h->alpha1, h->SOL, 1 - h->alpha1, h->X);          //   y = a1 y + (1-a1) x     :48
                prof_end(h, po);
                FOS_TRY(prox_cones(h, h->T2, h->T1, cg.gate));                                // S2!: prox!(y,S2,x)  :55
                }
                if (!will_check) { po = prof_begin_other(h, pg); FOS_TRY(step_finish_launch(h, cg)); prof_end(h, po); }
                return FOS_OK;
            };
            FOS_TRY(affine_then(h, c, h->X, post));                      // S1!: prox!(y,S1,x)          :45
            *check_on = h->T2;                                           //   checkstatus(status, y)    :56
            *finish_done = !will_check;
            return FOS_OK;
        }
        case FOS_ALG_FISTA: {                                            // fista.jl:28-48
            if (i == 1) FOS_HIP(hipMemcpyAsync(h->Y, h->X, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));   // :31-33
            const PostFn post = [h, will_check](const LaunchCtx& cg) -> int {
                const int pg = cg.gate ? 1 : 0;
                int po = prof_begin_other(h, pg);
                launch_axpby(cg, h->T1, h->alpha, h->SOL, 1 - h->alpha, h->Y);                 // :37
                launch_copy(cg, h->XOLD, h->X);                                               // :39  xold .= x
                prof_end(h, po);
                FOS_TRY(prox_cones(h, h->X, h->T1, cg.gate));                                 // :40
                if (!will_check) { po = prof_begin_other(h, pg); FOS_TRY(step_finish_launch(h, cg)); prof_end(h, po); }
                return FOS_OK;
            };
            FOS_TRY(affine_then(h, c, h->Y, post));                      // :35
            *check_on = h->X;                                            // :41
            *finish_done = !will_check;
            return FOS_OK;
        }
        case FOS_ALG_DYKSTRA: {                                          // dykstra.jl:25-36   (p = Y, q = XOLD)
            launch_add(c, h->W, h->X, h->Y);                             // x .+ p
            const PostFn post = [h, will_check](const LaunchCtx& cg) -> int {
                const int pg = cg.gate ? 1 : 0;
                int po = prof_begin_other(h, pg);
                launch_dykstra_corr(cg, h->Y, h->X, h->SOL);                                  // p .= x .+ p .- y            :30
                launch_add(cg, h->W, h->SOL, h->XOLD);                                        // y .+ q
                prof_end(h, po);
                FOS_TRY(prox_cones(h, h->X, h->W, cg.gate));                                  // prox!(x, S2, y .+ q)        :31
                if (!will_check) { po = prof_begin_other(h, pg); FOS_TRY(step_finish_launch(h, cg)); prof_end(h, po); }
                return FOS_OK;
            };
            FOS_TRY(affine_then(h, c, h->W, post));                      // prox!(y, S1, x .+ p)        :28
            *check_on = h->X;                                            // :32
            *finish_done = !will_check;
            return FOS_OK;
        }
    }
    set_error("unknown algorithm %d", h->alg);
    return FOS_EINVAL;
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
    switch (h->alg) {
        case FOS_ALG_GAP: {
            // (inside fos_step, CG projection: the kernel also leaves SOL - [0; X.y] in RHS for the next iteration's CG start)
            const bool sh = h->in_step && h->shift_fuse && !h->direct_exact();
            launch_gap_final(c, h->X, h->T2, h->T1, h->alpha, h->alpha2, sh ? h->RHS : nullptr, h->SOL);          // gap.jl:58,78
            h->shift_ready = sh;
            return FOS_OK;
        }
        case FOS_ALG_GAPA: {
            const bool sh = h->in_step && h->shift_fuse && !h->direct_exact();
            launch_gapa_final(c, h->X, h->T2, h->T1, h->alpha, sh ? h->RHS : nullptr, h->SOL);                    // gapa.jl:77,96,103
            h->shift_ready = sh;
            int fr = 0;
            FOS_TRY(finish_reduce(h, c, c.vec_blocks, 3, 0, &fr));
            launch_gapa_finalize(c, h->beta, fr);                                  // gapa.jl:96-101
            return FOS_OK;
        }
        case FOS_ALG_FISTA: {
            const double told = h->fista_t;                                        // fista.jl:44-46
            h->fista_t = (1 + std::sqrt(1 + 4 * told * told)) / 2;
            launch_fista_extrap(c, h->Y, h->X, h->XOLD, (told - 1) / h->fista_t);
            return FOS_OK;
        }
        case FOS_ALG_DYKSTRA:
            launch_dykstra_corr(c, h->XOLD, h->SOL, h->X);                         // q .= y .+ q .- x   dykstra.jl:34
            return FOS_OK;
    }
    return FOS_EINVAL;
}

// the iterate's way in and out of an equilibrated handle: the same staging with the scaling kernels (plain handles: upload_plain / download_plain)
int upload_caller(fos_solver* h, d2* dst, const double* z) {
    if (!h->equilibrated()) return upload_plain(h, dst, z);
    LaunchCtx c = h->ctx();
    FOS_HIP(hipMemcpyAsync(h->plain, z, sizeof(double) * 2 * h->l, hipMemcpyHostToDevice, h->stream));
    launch_eq_interleave(c, dst, h->plain, h->eq_up);
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}
int download_caller(fos_solver* h, double* z, const d2* src) {
    if (!h->equilibrated()) return download_plain(h, z, src);
    LaunchCtx c = h->ctx();
    launch_eq_deinterleave(c, h->plain, src, h->eq_up);
    FOS_HIP(hipMemcpyAsync(z, h->plain, sizeof(double) * 2 * h->l, hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int fos_abi_version(void) { return FOS_ABI_VERSION; }
const char* fos_last_error(void) { return fos::last_error_cstr(); }

int fos_device_count(int* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        if (count) *count = 0;
        set_error("no HIP device visible (%s): libfoship has no CPU fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return FOS_ENODEVICE;
    }
    if (count) *count = n;
    return FOS_OK;
}

int fos_device_name(int device, char* buf, int buflen) {
    hipDeviceProp_t prop;
    FOS_HIP(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return FOS_OK;
}

struct HandleGuard {                     // frees everything on an early error return of a create
    fos_solver* h;
    ~HandleGuard() { if (h) fos_destroy(h); }
};

int fos_create(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
               const double* b, const double* c,
               int64_t nK1, const int32_t* K1type, const int64_t* K1start, const int64_t* K1len,
               int64_t nK2, const int32_t* K2type, const int64_t* K2start, const int64_t* K2len,
               int device, fos_handle* out) {
    return fos_create2(m, n, colptr, rowval, nzval, b, c, nK1, K1type, K1start, K1len, nK2, K2type, K2start, K2len, device, 0, out);
}

int fos_create2(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                const double* b, const double* c,
                int64_t nK1, const int32_t* K1type, const int64_t* K1start, const int64_t* K1len,
                int64_t nK2, const int32_t* K2type, const int64_t* K2start, const int64_t* K2len,
                int device, int32_t flags, fos_handle* out) {
    if (!out) { set_error("out handle is NULL"); return FOS_EINVAL; }
    *out = nullptr;
    if (m < 0 || n < 0 || !colptr || (!rowval && colptr[n] > 1) || (!b && m) || (!c && n)) { set_error("NULL or negative argument"); return FOS_EINVAL; }
    int ndev = 0;
    FOS_TRY(fos_device_count(&ndev));
    if (device < 0 || device >= ndev) { set_error("device %d out of range (0..%d)", device, ndev - 1); return FOS_EINVAL; }
    FOS_TRY(cone_table_check("K1", m, nK1, K1type, K1start, K1len));
    FOS_TRY(cone_table_check("K2", n, nK2, K2type, K2start, K2len));
    FOS_HIP(hipSetDevice(device));

    HandleGuard guard{new fos_solver()};
    fos_solver* h = guard.h;
    h->device = device;
    h->m = m; h->n = n; h->l = n + m + 1; h->l_global = h->l;
    h->nnz = colptr[n] - 1;
    FOS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->shift_fuse = !(getenv("FOS_SHIFT_FUSE") && atoi(getenv("FOS_SHIFT_FUSE")) == 0);

    hipDeviceProp_t prop;
    FOS_HIP(hipGetDeviceProperties(&prop, device));
    const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->cus = cus;
    const PsdTuning psd_tuning = PsdTuning::from_env();
    h->psd_fuse = !(getenv("FOS_PSD_FUSE") && atoi(getenv("FOS_PSD_FUSE")) == 0);
    h->relax_ew = !(getenv("FOS_RELAX_EW") && atoi(getenv("FOS_RELAX_EW")) == 0);
    if (const char* e = getenv("FOS_RS_LOWP")) h->rs_lowp = std::max(0, std::min(2, atoi(e)));
    if (const char* e = getenv("FOS_RS_LOWP_ETA")) { const double eta = atof(e); if (eta > 0.0 && eta <= 1.0) h->rs_lowp_eta = eta; }
    if (const char* e = getenv("FOS_RS_LOWP_CACHE")) h->rs_lowp_cache = atoi(e) != 0;
    if (const char* e = getenv("FOS_RS_LOWP_CACHE_MB")) h->rs_lowp_cache_budget = rs_lowp_cache_budget(std::max<long long>(0, atoll(e)));

    // ---- operator (operator.cpp)
    h->row_sharded = (flags & FOS_CREATE_ROW_SHARDED) != 0;
    FOS_TRY(operator_setup(h, colptr, rowval, nzval));

    std::vector<double> cbv((size_t)(n + m));
    for (int64_t j = 0; j < n; ++j) { cbv[j] = c[j]; }
    for (int64_t i = 0; i < m; ++i) { cbv[n + i] = b[i]; }
    h->nb = std::sqrt(sum_squares(b, m)); h->nc = std::sqrt(sum_squares(c, n));
    h->nb_local = h->nb; h->nc_local = h->nc;
    FOS_TRY(dev_upload(h, &h->cb, cbv));

    // ---- vectors
    const size_t l = (size_t)h->l;
    d2** vecs[] = {&h->X, &h->T1, &h->T2, &h->SOL, &h->RHS, &h->R, &h->PB[0], &h->PB[1], &h->AP, &h->Y, &h->XOLD, &h->W, &h->SOL2};
    for (d2** v : vecs) FOS_TRY(dev_zeros(h, v, l));
    FOS_TRY(dev_alloc(h, &h->plain, 2 * l));
    h->vec_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((h->l + 255) / 256, 1024));

    // ---- cones
    ConeTable table;
    table.ew.assign(l, 0);
    cone_table_add(table, 0, CONE_K2, nK2, K2type, K2start, K2len);
    cone_table_add(table, n, CONE_K1, nK1, K1type, K1start, K1len);
    table.ew[l - 1] = (uint8_t)(EW_MAX0 | (EW_MAX0 << 2));      // tau, kappa  cones.jl:138,141
    ConeSetOptions cone_opts;
    cone_opts.warm = !getenv("FOS_PSD_COLD");
    cone_opts.refine_records = true;
    cone_opts.debug_rec = getenv("FOS_PSD_DEBUG_REC") != nullptr;
    FOS_TRY(cone_set_build(table, (int64_t)l, cone_opts, psd_tuning, &h->cones));

    // ---- scalars
    FOS_TRY(dev_zeros(h, &h->st, 1));
    FOS_TRY(cg_setup(h));                                 // the CG solve's state, switches and grid (cg.cpp)
    FOS_HIP(hipHostMalloc((void**)&h->st_host, sizeof(DevState), hipHostMallocDefault));
    memset(h->st_host, 0, sizeof(DevState));
    FOS_TRY(dev_alloc(h, &h->partials, (size_t)6 * PART_CAP));
    FOS_TRY(dev_zeros(h, &h->reduced, 16));

    FOS_TRY(resident_setup(h, cus));                      // FOS_CG_RESIDENT: does the operator qualify, and the plan if so
    {   // where the resident solve is the handle's default, its float copy is part of the set-up (and of what a caller times as set-up)
        int32_t v = FOS_CG_REFERENCE;
        FOS_TRY(fos_get_cg_variant(h, &v));
        if (v == FOS_CG_RESIDENT) FOS_TRY(resident_lowp_ensure(h));
    }
    FOS_TRY(fos_set_alg(h, FOS_ALG_GAP, 0.8, 1.8, 1.8, 0.0));
    FOS_TRY(fos_set_iterate(h, nullptr));
    FOS_HIP(hipStreamSynchronize(h->stream));
    *out = h;
    guard.h = nullptr;
    return FOS_OK;
}

// fos_create2 with opt-in equilibration: the scaling is computed on the host from the caller's CSC arrays (equilibrate.cpp), the handle is built from
// the SCALED data by the path above, and the vectors the caller's-units kernels read (equilibrate.hip) are added to it.
int fos_create3(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                const double* b, const double* c,
                int64_t nK1, const int32_t* K1type, const int64_t* K1start, const int64_t* K1len,
                int64_t nK2, const int32_t* K2type, const int64_t* K2start, const int64_t* K2len,
                int device, int32_t flags, int32_t equil_passes, fos_handle* out) {
    if (equil_passes == 0) return fos_create2(m, n, colptr, rowval, nzval, b, c, nK1, K1type, K1start, K1len, nK2, K2type, K2start, K2len, device, flags, out);
    if (!out) { set_error("out handle is NULL"); return FOS_EINVAL; }
    *out = nullptr;
    if (equil_passes < 0 || equil_passes > EQ_MAX_PASSES) { set_error("equil_passes = %d: 0 .. %d", (int)equil_passes, EQ_MAX_PASSES); return FOS_EINVAL; }
    if (flags & FOS_CREATE_ROW_SHARDED) {
        set_error("equilibration needs the whole problem on one handle: a rank knows neither the other ranks' column norms nor the global sigma, rho");
        return FOS_EUNSUPPORTED;
    }
    EqScaling eq;
    FOS_TRY(host_equilibrate(m, n, colptr, rowval, nzval, b, c, nK1, K1type, K1start, K1len, nK2, K2type, K2start, K2len, equil_passes, &eq));
    fos_handle h = nullptr;
    FOS_TRY(fos_create2(m, n, colptr, rowval, eq.nz.data(), eq.b.data(), eq.c.data(), nK1, K1type, K1start, K1len, nK2, K2type, K2start, K2len, device, flags, &h));
    HandleGuard guard{h};
    h->eq_nb = std::sqrt(sum_squares(b, m)); h->eq_nc = std::sqrt(sum_squares(c, n));      // the caller's norms, summed as the handle's
    h->eq_sigma = eq.sigma; h->eq_rho = eq.rho; h->eq_gamma = eq.gamma;
    const size_t l = (size_t)h->l;
    std::vector<d2> up(l);
    std::vector<double> inv((size_t)(n + m)), cbv((size_t)(n + m));
    for (int64_t j = 0; j < n; ++j) {
        up[j] = make_double2(eq.sigma / eq.E[j], eq.rho * eq.E[j]);
        inv[j] = 1.0 / eq.E[j];
        cbv[j] = eq.c[j];
    }
    for (int64_t i = 0; i < m; ++i) {
        up[n + i] = make_double2(eq.rho / eq.D[i], eq.sigma * eq.D[i]);
        inv[n + i] = 1.0 / eq.D[i];
        cbv[n + i] = eq.b[i];
    }
    up[l - 1] = make_double2(1.0, eq.sigma * eq.rho);
    for (const d2& u : up)
        if (!(u.x > 0.0) || !(u.y > 0.0) || !std::isfinite(u.x) || !std::isfinite(u.y)) { set_error("equilibration: a scale factor left the range of fp64"); return FOS_EINVAL; }
    FOS_TRY(dev_upload(h, &h->eq_up, up));
    FOS_TRY(dev_upload(h, &h->eq_inv, inv));
    FOS_TRY(dev_upload(h, &h->eq_cb, cbv));
    FOS_TRY(dev_zeros(h, &h->eq_w, l));
    h->eq_D.swap(eq.D);
    h->eq_E.swap(eq.E);
    h->eq_passes = equil_passes;
    *out = h;
    guard.h = nullptr;
    return FOS_OK;
}

int fos_get_equilibration(fos_handle h, int32_t* passes, double* D, double* E, double* scal3) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    if (passes) *passes = h->eq_passes;
    if (D) { if (h->equilibrated()) std::copy(h->eq_D.begin(), h->eq_D.end(), D); else std::fill(D, D + h->m, 1.0); }
    if (E) { if (h->equilibrated()) std::copy(h->eq_E.begin(), h->eq_E.end(), E); else std::fill(E, E + h->n, 1.0); }
    if (scal3) { scal3[0] = h->eq_sigma; scal3[1] = h->eq_rho; scal3[2] = h->eq_gamma; }
    return FOS_OK;
}

int fos_destroy(fos_handle h) {
    if (!h) return FOS_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    transport_teardown(h, true);
    for (auto& r : h->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    cone_set_destroy(h->cones, h->stream);
    for (void* p : h->pooled) uncached_release(p);
    for (void* p : h->owned) (void)hipFree(p);
    if (h->st_host) (void)hipHostFree(h->st_host);
    cg_teardown(h);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return FOS_OK;
}

int fos_sizes(fos_handle h, int64_t* m, int64_t* n, int64_t* N, int64_t* nnz) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    if (m) *m = h->m;
    if (n) *n = h->n;
    if (N) *N = 2 * h->l;
    if (nnz) *nnz = h->nnz;
    return FOS_OK;
}

int fos_set_alg(fos_handle h, int alg, double alpha, double alpha1, double alpha2, double beta) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    if (alg < FOS_ALG_GAP || alg > FOS_ALG_DYKSTRA) { set_error("unknown algorithm %d", alg); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    h->alg = alg; h->alpha = alpha; h->alpha1 = alpha1; h->alpha2 = alpha2; h->beta = beta;
    h->wr.off();                                                        // a fresh algorithm is unwrapped (fos_set_linesearch / _gapp / _longstep follow)
    h->fista_t = 1.0;                                                   // fista.jl:24
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
    h->prox_i = 1; h->firstrun = true; h->cgiter = 0; h->cg.hit_max_accum = 0; h->cg.last_cg_pred = 0;
    h->firstrun2 = true;
    return FOS_OK;
}

int fos_set_iterate(fos_handle h, const double* z) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (z) return upload_caller(h, h->X, z);
    // HSDE_getinitialvalue: zeros, tau = kappa = 1     HSDE.jl:40-47
    FOS_HIP(hipMemsetAsync(h->X, 0, sizeof(d2) * h->l, h->stream));
    const d2 one = make_double2(1.0, 1.0);
    FOS_HIP(hipMemcpyAsync(h->X + (h->l - 1), &one, sizeof(d2), hipMemcpyHostToDevice, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

int fos_get_iterate(fos_handle h, double* z) {
    if (!h || !z) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    return download_caller(h, z, h->X);
}

int fos_get_checked(fos_handle h, double* z) {
    if (!h || !z) { set_error("NULL argument"); return FOS_EINVAL; }
    if (!h->last_checked) { set_error("no convergence check has run yet"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    return download_caller(h, z, h->last_checked);
}

int fos_step(fos_handle h, int64_t i_first, int64_t count, int64_t checki, double eps,
             int64_t* iters_done, int32_t* checked, fos_check_result* res) {
    if (!h || checki < 1 || count < 0) { set_error("bad fos_step arguments"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (checked) *checked = 0;
    int64_t done = 0;
    h->shift_ready = false;
    struct InStep { fos_solver* h; ~InStep() { h->in_step = false; h->shift_ready = false; } } in_step{h};
    h->in_step = true;
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
            h->last_checked = check_on;
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
    FOS_TRY(wrappers_check(h->wr, WRAP_LINESEARCH, h->alg, h->sharded() || h->row_sharded, lsinterval, 0));
    h->wr.ls_interval = lsinterval;
    return FOS_OK;
}
// GAPP(alpha, alpha1, alpha2; iproj) (solvers/gapproj.jl, README solver table): fos_set_alg(FOS_ALG_GAP, alpha, alpha1, alpha2) and then
// fos_set_gapp(iproj > 0): iterations i with i % iproj == 0 search 21 step lengths 2^k along P_S1(P_S2(P_S1 x)) - P_S1 x.
int fos_set_gapp(fos_handle h, int64_t iproj) {
    if (!h || iproj < 0) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_TRY(wrappers_check(h->wr, WRAP_GAPP, h->alg, h->sharded() || h->row_sharded, iproj, 0));
    h->wr.gapp_iproj = iproj;
    return FOS_OK;
}
// LongstepWrapper(alg; longinterval, nsave) around the algorithm set last (wrappers/longstep.jl:22-40): 0 switches it off
int fos_set_longstep(fos_handle h, int64_t longinterval, int64_t nsave) {
    if (!h || longinterval < 0 || nsave < 0) { set_error("bad argument"); return FOS_EINVAL; }
    if (longinterval == 0) { h->wr.lp.interval = 0; h->wr.lp.savepos = 0; return FOS_OK; }
    FOS_TRY(wrappers_check(h->wr, WRAP_LONGSTEP, h->alg, h->sharded() || h->row_sharded, longinterval, nsave));
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
        h->last_checked = h->T2;
    }
    if (z_out) FOS_TRY(download_caller(h, z_out, h->T2));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

int fos_get_affine_state(fos_handle h, double* xinit, int64_t* i, int32_t* firstrun) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (xinit) FOS_TRY(download_plain(h, xinit, h->SOL));
    if (i) *i = h->prox_i;
    if (firstrun) *firstrun = h->firstrun ? 1 : 0;
    return FOS_OK;
}

int fos_set_affine_state(fos_handle h, const double* xinit, int64_t i) {
    if (!h || !xinit || i < 1) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(upload_plain(h, h->SOL, xinit));
    h->firstrun = false;
    h->prox_i = i;
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
        scal2[0] = h->fista_t;
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
        h->fista_t = scal2[0];
        FOS_HIP(hipStreamSynchronize(h->stream));
        FOS_HIP(hipMemcpy(&h->st->alpha12, &scal2[1], sizeof(double), hipMemcpyHostToDevice));
    }
    return FOS_OK;
}

int fos_get_cgiter(fos_handle h, int64_t* cgiter) {
    if (!h || !cgiter) { set_error("NULL argument"); return FOS_EINVAL; }
    *cgiter = h->cgiter;
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
    *i = h->prox_i;
    return FOS_OK;
}

// ---- fine-grained entries ----------------------------------------------------------------------------

int fos_q_apply(fos_handle h, double* y, const double* x, int32_t transpose) {
    if (!h || !y || !x) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    LaunchCtx c = h->ctx();
    const size_t l = (size_t)h->l;
    FOS_HIP(hipMemcpyAsync(h->plain, x, sizeof(double) * l, hipMemcpyHostToDevice, h->stream));
    launch_set_comp(c, h->W, h->plain, 0);
    const double sign = transpose ? -1.0 : 1.0;           // HSDEAffine.jl:61-65
    int fr = 0;
    launch_q1(c, Q_PLAIN, h->W, 0, sign, h->plain + l);
    FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
    launch_q1_finalize(c, Q_PLAIN, h->W, 0, sign, h->plain + l, fr);
    FOS_HIP(hipMemcpyAsync(y, h->plain + l, sizeof(double) * l, hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

int fos_kkt_apply(fos_handle h, double* y, const double* x) {
    if (!h || !y || !x) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    LaunchCtx c = h->ctx();
    FOS_TRY(upload_plain(h, h->W, x));
    FOS_TRY(kkt_apply_full(h, c, h->W, h->AP));
    return download_plain(h, y, h->AP);
}

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
    if (h->firstrun2) {                                                // :109-112
        FOS_HIP(hipMemcpyAsync(h->SOL2, h->RHS, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
        h->firstrun2 = false;
    }
    const double eps = 2.220446049250313e-16;
    const double tol = (double)(2 * h->l_global) * eps;                // :106
    int64_t it = 0;
    CgCall call{h->SOL2, h->RHS, tol, 1000};
    call.predict = false;
    FOS_TRY(cg_solve(h, call, &it));                                   // :116 ; xinit .= y :119
    h->cgiter = it;
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

// ---- measurement -------------------------------------------------------------------------------------

int fos_profile(fos_handle h, int32_t enable) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    h->prof = enable != 0;
    h->prof_period = enable > 1 ? enable : 1;
    for (int k = 0; k < FOS_PROF_CLASSES; ++k) h->prof_seen[k] = 0;
    h->prof_steps = 0; h->prof_steps_sampled = 0; h->prof_step_on = false;
    return FOS_OK;
}

static double kkt_bytes(const fos_solver* h) {
    // B_kkt,min = 24 nnz + 4(m+n+2) + 32(m+n)
    return 24.0 * (double)h->nnz + 4.0 * (double)(h->m + h->n + 2) + 32.0 * (double)(h->m + h->n);
}

// launches / summed milliseconds per class of the bracketed launch groups since the last read; resets the records
int fos_profile_read_classes(fos_handle h, int64_t* launches3, double* total_ms3) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipStreamSynchronize(h->stream));
    int64_t n[FOS_PROF_CLASSES] = {0, 0, 0, 0, 0};
    double t[FOS_PROF_CLASSES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t i = 0; i < h->prof_used; ++i) {
        const auto& r = h->prof_recs[i];
        if (r.cls < 0 || r.cls >= FOS_PROF_CLASSES) continue;
        float ms = 0.f;
        FOS_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        n[r.cls] += 1; t[r.cls] += ms;
    }
    n[FOS_PROF_OTHER] = h->prof_steps_sampled;           // this class is normalised per sampled OUTER ITERATION (foship.h)
    h->prof_steps_sampled = 0;
    for (int k = 0; k < FOS_PROF_CLASSES; ++k) {
        if (launches3) launches3[k] = n[k];
        if (total_ms3) total_ms3[k] = t[k];
    }
    h->prof_used = 0;
    return FOS_OK;
}

int fos_profile_read(fos_handle h, int64_t* launches, double* total_ms, double* bytes_per_launch) {
    int64_t n[FOS_PROF_CLASSES];
    double t[FOS_PROF_CLASSES];
    FOS_TRY(fos_profile_read_classes(h, n, t));
    if (launches) *launches = n[FOS_PROF_KKT];
    if (total_ms) *total_ms = t[FOS_PROF_KKT];
    if (bytes_per_launch) *bytes_per_launch = kkt_bytes(h);
    return FOS_OK;
}

int fos_bench_kkt(fos_handle h, int32_t reps, double* total_ms) {
    if (!h || reps < 1) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    LaunchCtx c = h->ctx();
    hipEvent_t e0, e1;
    FOS_HIP(hipEventCreate(&e0));
    FOS_HIP(hipEventCreate(&e1));
    launch_kkt2(c, h->X, h->AP, 0);           // warm
    FOS_HIP(hipEventRecord(e0, h->stream));
    for (int i = 0; i < reps; ++i) launch_kkt2(c, h->X, h->AP, 0);
    FOS_HIP(hipEventRecord(e1, h->stream));
    FOS_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FOS_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (total_ms) *total_ms = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return FOS_OK;
}

int fos_sync(fos_handle h) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

int fos_set_tuning(fos_handle h, int32_t spmv_workgroups, int32_t cg_chunk, int32_t fuse_p) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(cg_set_tuning(h, cg_chunk, fuse_p));
    if (spmv_workgroups > 0) FOS_TRY(operator_repartition(h, spmv_workgroups));
    return FOS_OK;
}

// test hooks
int fos_debug_set(fos_handle h, int32_t what, int64_t value) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (what == FOS_DEBUG_PUPDATE_DELAY) {
        const int32_t v = (int32_t)std::max<int64_t>(0, std::min<int64_t>(value, 100000000));     // <= 1 s
        FOS_HIP(hipStreamSynchronize(h->stream));
        FOS_HIP(hipMemcpy(&h->st->dbg_delay, &v, sizeof(v), hipMemcpyHostToDevice));
        return FOS_OK;
    }
    set_error("unknown debug switch %d", (int)what);
    return FOS_EINVAL;
}

}  // extern "C"
