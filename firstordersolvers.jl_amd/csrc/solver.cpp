// libfoship: what a handle IS -- its life cycle, the iterate's way in and out, profiling records, the uncached pool, the sharded set-up -- and the entries of
// include/foship.h about those (the outer iteration: step.cpp).  Host C++ only orchestrates launches on ONE HIP stream; all data stays
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

}  // namespace fos

using namespace fos;

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

    hipDeviceProp_t prop;
    FOS_HIP(hipGetDeviceProperties(&prop, device));
    const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->cus = cus;
    const PsdTuning psd_tuning = PsdTuning::from_env();
    step_read_switches(h->step);                          // FOS_SHIFT_FUSE, FOS_PSD_FUSE, FOS_RELAX_EW (step.cpp)
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
    if (!h->step.last_checked) { set_error("no convergence check has run yet"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    return download_caller(h, z, h->step.last_checked);
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
