// struct fos_solver (the handle behind fos_handle) and the helpers that solver.cpp, step.cpp, cg.cpp, operator.cpp, cones.cpp, direct.cpp and transport.cpp share.  Private: not part of the ABI.
#pragma once

#include <rccl/rccl.h>

#include <algorithm>
#include <functional>

#include "fos_internal.hpp"
#include "wrappers.hpp"

typedef double2 d2;

// which form S1 = IndAffine([Q -I], 0) runs in: the values of fos_get_direct_mode
enum DirectForm : int32_t { DIRECT_OFF = 0, DIRECT_DENSE = 1, DIRECT_BLOCK = 2, DIRECT_CG = 3, DIRECT_REDUCED = 4 };

// how the stored inverse of the dense or the reduced form was built (dense_spd_inverse, direct.cpp)
struct DenseInv {
    int used = FOS_DIRECT_FACTOR_NEWTON;       // the factor that produced the accepted inverse (NEWTON after a fallback)
    int steps = 0;                             // Newton-Schulz steps (Newton), polish steps (Cholesky: 0..2)
    double seconds = 0.0, probe = 0.0;         // the inversion stage alone (matrix formed -> inverse accepted); last probe residual of the Cholesky path (0 on the Newton path)
    bool fell_back = false;                    // the Cholesky path gave up and Newton-Schulz ran
    int64_t bad_col = -1;                      // first column whose Cholesky pivot was not a positive finite number
};

// ------------------------------------------------------------------------------------------------ the transports' state (transport.cpp)
// which of them carries a sharded handle's sums: VIA_PEER before VIA_HOST before VIA_RCCL, whatever else is set up beside it
enum ReduceVia { VIA_NONE, VIA_RCCL, VIA_HOST, VIA_PEER };
// the POSIX shared-memory segment behind the host-pinned mailboxes
struct HostSeg {
    void* p = nullptr;                         // the mapping (nullptr: no segment)
    int fd = -1;                               // kept open: host_seg_stale asks it whether the mapped segment is still linked under its name
    size_t bytes = 0;
    std::string name;
    bool creator = false;                      // this process created the name (rank 0) and unlinks it
    // the last page: every rank's device identity, written by the rank when it opens the segment (zero: that rank has not opened it yet)
    volatile unsigned long long* ids() const { return reinterpret_cast<volatile unsigned long long*>(static_cast<char*>(p) + bytes - 4096); }
};
struct Transport {
    ncclComm_t comm = nullptr;                 // in-stream RCCL all-reduce (fos_comm_init)
    // the caller's own collective on host buffers (fos_comm_init_host: MPI.jl, gloo, ...)
    fos_allreduce_fn host_fn = nullptr; void* host_user = nullptr;
    double* host_buf = nullptr;                // pinned, max(2n, 16) doubles
    // peer mailboxes: in device memory, mapped through HIP IPC (fos_peer_open), or in one host-pinned shm segment (fos_peer_open_host)
    unsigned long long* peer_mbox = nullptr;   // own mailbox (uncached device memory, exported through HIP IPC)
    unsigned long long* peer_relay = nullptr;  // host-pinned mailboxes: the local relay
    std::vector<void*> peer_opened;            // IPC mappings of the peers' mailboxes
    fos::PeerBox peer{};                       // the installed mailboxes (box != nullptr: open)
    bool peer_on{false};                       // ... and whether the sums go through them (fos_peer_enable)
    bool peer_same_device = false;             // a peer rank's mailbox lives on THIS device (several ranks on one GPU: tests)
    HostSeg host_seg;                          // the mapped + registered shm segment
    // row-sharded + peer mailboxes: the n-vector A'y crosses the ranks through peer-mapped memory too (fos_internal.hpp, fos::VecBox)
    double* vec_buf = nullptr;                 // own exchange buffer: [2][nranks][2n] doubles, then [2][nranks] flags (uncached, IPC-exported)
    std::vector<void*> vec_opened;
    fos::VecBox vec{};
    uint32_t vec_seq = 0;                      // exchanges enqueued so far (the same on every rank: all make the same calls)
    ReduceVia via() const { return peer_on ? VIA_PEER : (host_fn ? VIA_HOST : (comm ? VIA_RCCL : VIA_NONE)); }
};

// ------------------------------------------------------------------------------------------------ the stacked operator S = [A'; A] (operator.cpp)
// Its device arrays are on the handle's `owned` and `pooled` lists like everything else.
struct Operator {
    fos::HostBlkCsr host;                      // kept only for re-partitioning (indices freed after upload)
    fos::DevBlkCsr dev{};                      // what the kernels read (LaunchCtx::S)
    int32_t* wave_blk0 = nullptr; fos::BlkDesc* wave_first = nullptr;      // dev.wave_blk0 and dev.wave_first, writable: operator_repartition
    uint32_t* def_mask = nullptr;              // bit i: row i of S is finished from partial slots (dual tiles)
    int64_t win_stats[4] = {0, 0, 0, 0};       // window panels: panels, (panel, window) segments, 64-row slices, stored entries
    int nwg_target = 2048;                     // workgroups the row blocks are partitioned for
    // row-sharded: the slots of the rows of A' summed over the ranks (what dev.slots_rd names; fos_solver::sum_slots_over_ranks fills it)
    double* slots_rd = nullptr;
    // row-sharded WITH dual tiles: the sweep fills local slot lists (dev.slots = slots_rd + 2n doubles); between sweep and consumers the
    // lists of the n rows of A' are added up (cmp_rec / cmp_idx -> cmp_local) and THAT n-vector crosses the ranks into slots_rd[0..n);
    // the consumers' records (dev.def_rec) name slot j for row j < n and the local lists, shifted by n, for the rows of A
    fos::DefRow* cmp_rec = nullptr; int32_t* cmp_idx = nullptr; double* cmp_local = nullptr; int cmp_lpr = 1;
    // FOS_CG_RESIDENT (resident.hip): the plan (which workgroup holds which tiles), its device copy and the workgroups' record arrays
    fos::ResPlan res_plan;
    fos::ResLaunch res{};
    fos::ResWG* res_wg = nullptr;              // res.wg, writable: resident_setup replaces it
    bool res_ok = false;                       // this handle's operator qualifies (under the current workgroup budget)
    bool res_all = false;                      // ... and so does every rank's (sharded: the vote of global_setup)
    int res_gmax = 0;                          // the budget the plan was made for
    // the streamed form's fp32 walk (resident_lowp_ensure; res.val32 / res.lowp_out name them): the tile values as float, the last solve's record
    float* res_val32 = nullptr;
    bool res_lowp_pending = false;             // the plan in force has not been given its float copy and delta yet (resident_lowp_ensure)
    double* res_lowp_out = nullptr;
};

// ------------------------------------------------------------------------------------------------ the CG solve behind prox_affine (cg.cpp)
struct CgState {
    bool fuse_p = false;                       // the p update of CG rides on the next sweep (2 launches per iteration)
    int cg_variant = -1;                       // FOS_CG_*: -1 = the handle's default (sharded: merged reduction, closing in the update)
    int cg_chunk = 8;                          // iterations enqueued per host poll
    int cg_blocks = 0;                         // fos::LaunchCtx::cg_blocks
    int last_cg_pred = 0;                      // the last predicted solve's iteration count: the size of the next one's first batch
    int cg_same_run = 0;                       // consecutive solves that took exactly last_cg_pred iterations
    int64_t cg_total = 0;                      // CG iterations since fos_create
    uint32_t cg_epoch = 0;                     // windows of 2048 sequence numbers used so far (cg_windows): the folded exchanges, the resident solve
    int hit_max_accum = 0;                     // a solve since the last status check ended on its cap
    // speculation past a CG solve: the kernels that follow it are enqueued (gated on fos::DevState.done) BEFORE the host learns the
    // iteration count, which it then reads from a record the CG kernels write into pinned host memory (wait_cg_mark)
    bool speculate = true;
    fos::HostMark* mark = nullptr;             // pinned + mapped; fos::DevState.hostmark points at it
    double* pre_sums = nullptr;                // fos::LaunchCtx::pre
    bool pre_on = true;
};

// ------------------------------------------------------------------------------------------------ the outer iteration (step.cpp)
struct StepState {
    // algorithm (gap.jl:6-21, gapa.jl:9-25, fista.jl:6-18, dykstra.jl:5-17)
    int alg = FOS_ALG_GAP;
    double alpha = 0.8, alpha1 = 1.8, alpha2 = 1.8, beta = 0.0;
    double fista_t = 1.0;
    // S1 = AffinePlusLinear state (affinepluslinear.jl:58-69)
    int64_t prox_i = 1;
    bool firstrun = true;
    int64_t cgiter = 0;
    bool firstrun2 = true;                     // HSDEMatrix.cgdata.firstrun
    bool shift_ready = false;                  // RHS already holds SOL - [0; X.y] (written by the step's last kernel): inside fos_step only
    bool in_step = false;                      // fos_step is running (the entries that project outside it leave no shift behind)
    // the step's switches (step_read_switches; FOS_FUSED_RHS is per process and sits beside it)
    bool shift_fuse = true;                    // FOS_SHIFT_FUSE=0: every projection runs its own shift pass
    bool psd_fuse = true;                      // FOS_PSD_FUSE=0: relaxation, projection and the step's last pass stay separate launches
    bool relax_ew = true;                      // FOS_RELAX_EW=0: the relaxation does not project the elementwise cones in the same pass
    const d2* last_checked = nullptr;          // vector the last checkstatus was evaluated on
};

// ------------------------------------------------------------------------------------------------ the handle
struct fos_solver {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t m = 0, n = 0, l = 0, nnz = 0;
    int64_t l_global = 0;                      // == l unless sharded (tolerance floor uses the global size)

    Operator op;
    std::vector<void*> owned;                  // every hipMalloc'd pointer
    std::vector<void*> pooled;                 // blocks of the process-wide pool of uncached memory (uncached_acquire): released, never freed
    double* cb = nullptr;
    double nb = 0.0, nc = 0.0;                 // ||b||, ||c|| (global)
    double nb_local = 0.0, nc_local = 0.0;     // this shard's ||b||, ||c||

    // vectors: l double2 each
    d2 *X = nullptr, *T1 = nullptr, *T2 = nullptr;          // iterate, tmp1, tmp2
    d2 *SOL = nullptr, *RHS = nullptr, *R = nullptr, *AP = nullptr;                 // CG: xinit/y, rhs, r, z
    d2 *PB[2] = {nullptr, nullptr};                         // CG direction, ping-pong: p_j lives in PB[j & 1]
    d2 *Y = nullptr, *XOLD = nullptr;                       // FISTA y / xold ; Dykstra p / q
    d2 *W = nullptr;                                        // scratch (Dykstra sums, test entries)
    d2 *SOL2 = nullptr;                                     // HSDEMatrix.cgdata.xinit
    double* plain = nullptr;                                // 2l doubles: ABI staging

    // cones: S2 = DualConeProduct, its table, workspaces and warm-start state (cones.cpp)
    fos::ConeSet* cones = nullptr;
    int cus = 256;                             // compute units of `device`
    int rs_lowp = 1;                           // FOS_RS_LOWP: 0 the streamed CG solve reads doubles only, 1 fp32 tiles by the rule (default), 2 on every sweep behind the start (tests)
    double rs_lowp_eta = 0.1;                  // FOS_RS_LOWP_ETA: the share of min(a solve's tolerance, the schedule's floor l eps) the fp32 sweeps may cost
    bool rs_lowp_cache = true;                 // FOS_RS_LOWP_CACHE=0: the float copy is read with non-temporal loads whatever its size (rs_lowp_cached, fos_internal.hpp)
    int64_t rs_lowp_cache_budget = fos::RS_LOWP_CACHE_BUDGET_BYTES;      // FOS_RS_LOWP_CACHE_MB: another budget for the rule (tests)

    // scalars
    fos::DevState* st = nullptr;
    fos::DevState* st_host = nullptr;               // pinned
    CgState cg;                                // the CG solve's state and switches (cg.cpp)
    double* partials = nullptr;
    double* reduced = nullptr;                 // 16 doubles
    int vec_blocks = 0;

    // direct = true (HSDE.jl:12-15): S1 = IndAffine([Q -I], 0), an exact projection through a one-time dense factorisation (direct.cpp).
    // direct_form says which form is ACTIVE; what is STORED (Ginv, blk_ready, red_ready) does not depend on it: a disabled handle keeps its factorisation
    DirectForm direct_form = DIRECT_OFF;
    bool direct_exact() const { return direct_form != DIRECT_OFF && direct_form != DIRECT_CG; }     // S1 runs no CG
    double* Ginv = nullptr;                    // (I + Q Q')^-1, symmetric, column-major, leading dimension Gld (l padded to 64)
    int64_t Gld = 0;
    int direct_factor_req = 0;                 // FOS_DIRECT_FACTOR_*: how the stored inverse (dense or reduced form) was asked to be built
    DenseInv direct_inv;                       // ... and how it was built
    double* dvec[2] = {nullptr, nullptr};      // two plain l-vectors
    // direct = true on a BLOCK-SEPARABLE operator: I + A'A is block diagonal with blocks of order <= BLKDIR_MAX (an SDP with few variables per
    // block: C4), so the exact projection costs three KKT sweeps -- no CG, no dense l x l inverse (prox_affine_direct_block)
    int blk_n = 0;                             // diagonal blocks of I + A'A
    int64_t* blk_goff = nullptr;               // [blk_n] start of block b's inverse (s_b x s_b, column-major) in blk_ginv
    int32_t* blk_ioff = nullptr;               // [blk_n + 1] start of block b's column list in blk_idx
    int32_t* blk_idx = nullptr;
    double* blk_ginv = nullptr;
    d2 *blk_phg = nullptr, *blk_qphg = nullptr;   // (D^-1 h, D^-1 M h) and their images under Q, per row
    double* blk_prm = nullptr;                 // the 3 x 3 inverse of the border system (9), delta = 1 + |[c; b]|^2
    double* blk_ctx = nullptr;                 // [blk_n] the blocks' shares of c'x^ (blkdir_solve_kernel)
    bool blk_skip_tail = true;                 // the third apply runs without its deferred-row and tau-row kernels (FOS_BLKDIR_FULL_APPLY=1: with them)
    bool blk_ready = false;                    // blkdir_setup ran to its end (a half-finished set-up must not pass for the block form)
    // direct = true, REDUCED form (direct_reduced.hip): K^-1, K = I + A'A (n <= m) or I + A A' (m < n), as tiles of its lower triangle stored once
    bool red_ready = false;                    // reduced_setup ran to its end
    int red_swap = 0;                          // 1: m < n, K = I + A A'
    int red_refine = 1;                        // steps of iterative refinement on the matrix-free G = I - Q Q per projection (FOS_DIRECT_REDUCED_REFINE)
    fos::RedPlan red_plan;
    fos::RedDev red{};
    d2 *red_pq = nullptr, *red_yk = nullptr;   // the two right-hand sides of the tile product and its result, interleaved (kpad pairs)
    double *red_s = nullptr, *red_d = nullptr, *red_r = nullptr, *red_z = nullptr;   // plain l-vectors: a Q sweep's result, D^-1 t1, the refinement's residual, Q w / Q Q w
    double *red_p = nullptr, *red_q = nullptr, *red_g = nullptr;                     // D^-1 h, D^-1 g, g = -Q0 h
    double* red_dots = nullptr;                // [RED_DOT_BLOCKS][2] the workgroups' shares of h'd and g'd
    double red_minv[4] = {0, 0, 0, 0};         // inverse of the 2 x 2 border system, row-major
    double direct_setup_s = 0.0;               // wall time of the last set-up (fos_get_direct_stats)

    StepState step;                            // the outer iteration's state and switches (step.cpp)
    fos::Wrappers wr;                          // LineSearchWrapper, GAPP, LongstepWrapper (wrappers.hpp)

    // sharding: how the sums cross the ranks is the transport's business (transport.cpp); what is sharded is the handle's, the solves' sequence windows are the CG state's
    Transport tr;
    int nranks = 1, rank = 0;
    bool sharded() const { return tr.via() != VIA_NONE; }
    // row sharding of a non-block-diagonal A: the first n entries (and tau, kappa) of every vector are replicated,
    // the slots of the rows of A' are summed over the ranks (RCCL all-reduce of 2n doubles) between a sweep and its slot-list sums
    bool row_sharded = false;

    // opt-in equilibration (fos_create3): the handle holds the SCALED problem; eq_passes == 0: a plain handle, nothing below is allocated
    int eq_passes = 0;
    std::vector<double> eq_D, eq_E;            // host: row factors (gamma folded in), column factors
    double eq_sigma = 1.0, eq_rho = 1.0, eq_gamma = 1.0;
    double eq_nb = 0.0, eq_nc = 0.0;           // ||b||, ||c|| of the CALLER's data (nb, nc above are the scaled problem's)
    d2* eq_up = nullptr;                       // [l] caller's (part 1, part 2) -> scaled, per element (equilibrate.hip)
    double *eq_inv = nullptr, *eq_cb = nullptr, *eq_w = nullptr;   // [1 ./ E; 1 ./ D] and [c^; b^] (n + m each), w = Q^ u^ of a status check (l)
    bool equilibrated() const { return eq_passes > 0; }

    // tuning / measurement
    bool prof = false;
    int prof_period = 1;                       // every prof_period-th launch of a class is bracketed by events (1: all)
    int64_t direct_sweeps = 0;                 // sweeps of the block-direct projection since fos_create (profiling ordinal)
    struct ProfRec { hipEvent_t a, b; int cls; int j; };
    std::vector<ProfRec> prof_recs;            // event pairs, reused
    size_t prof_used = 0;
    int64_t prof_seen[FOS_PROF_CLASSES] = {0, 0, 0, 0, 0};
    int64_t prof_steps = 0, prof_steps_sampled = 0;   // outer iterations since fos_profile / of them sampled for FOS_PROF_OTHER
    bool prof_step_on = false;                 // the outer iteration in flight brackets its FOS_PROF_OTHER groups
    static constexpr size_t PROF_CAP = 16384;

    static int sum_slots_over_ranks(void* self);      // transport.cpp

    // mailboxes = true: with the open mailboxes attached although the sums do not go through them (yet): fos_peer_selftest
    fos::LaunchCtx ctx(bool mailboxes = false) const {
        fos::LaunchCtx c;
        c.stream = stream; c.S = op.dev; c.cb = cb; c.n = n; c.m = m; c.l = l; c.st = st;
        c.partials = partials; c.reduced = reduced; c.vec_blocks = vec_blocks; c.cg_blocks = cg.cg_blocks;
        c.peer = (tr.peer_on || mailboxes) ? &tr.peer : nullptr;
        c.def_mask = op.def_mask;
        c.pre = cg.pre_on ? cg.pre_sums : nullptr;
        c.between = nullptr; c.between_arg = nullptr;
        c.cus = cus;
        c.psd_refine_max_mats = (tr.peer_same_device && nranks > 1) ? std::max(1, cus / nranks) : 0;
        c.count_repl = (!row_sharded || rank == 0) ? 1 : 0;
        c.n_repl = row_sharded ? n : 0;
        if (row_sharded) { c.between = &fos_solver::sum_slots_over_ranks; c.between_arg = const_cast<fos_solver*>(this); }
        return c;
    }
};

// does the step's last kernel also leave SOL - [0; X.y] in RHS for the next iteration's CG start?  (inside fos_step, and where S1 runs a CG solve)
inline bool leaves_shift(const fos_solver* h) { return h->step.in_step && h->step.shift_fuse && !h->direct_exact(); }

// ------------------------------------------------------------------------------------------------ shared helpers (defined in solver.cpp where no other file is named)
namespace fos {
// transport.cpp: the sums of a sharded handle (allreduce: `count` doubles in h->reduced, in place, in stream), the end of its transports, the two switches
// of the mailboxes (FOS_PEER_FOLD: read once per process; FOS_PEER_LOOPBACK: at every call)
int allreduce(fos_solver* h, int count);
int finish_reduce(fos_solver* h, const LaunchCtx& c, int count, int nacc, int gate, int* from_reduced, int off = 0);
void transport_teardown(fos_solver* h, bool destroy = false);
bool peer_fold_env(), peer_loopback_env();
// solver.cpp, for transport.cpp and operator.cpp: the sharded set-up and the process-wide pool of uncached memory
int global_setup(fos_solver* h);
int uncached_acquire(int device, size_t bytes, bool allow_plain, void** out, const char* what);
struct RoctxRange {                            // a named range for `rocprofv3 --marker-trace` (FOS_ROCTX=1)
    bool on;
    explicit RoctxRange(const char* name);
    ~RoctxRange();
};
int check_launch(const char* where);
int prof_begin(fos_solver* h, int cls, int j, int64_t ordinal);
int prof_begin_other(fos_solver* h, int post);
void prof_end(fos_solver* h, int idx);
int poll_state(fos_solver* h);
int kkt_apply_full(fos_solver* h, const LaunchCtx& c, const d2* w, d2* out, bool deferred = true, bool tau_row = true);
int upload_plain(fos_solver* h, d2* dst, const double* z);      // a caller's plain 2l-vector <-> a device vector, through h->plain; synchronise
int download_plain(fos_solver* h, double* z, const d2* src);
int upload_caller(fos_solver* h, d2* dst, const double* z);     // the same in the CALLER's units: an equilibrated handle scales on the way (plain handles: the two above)
int download_caller(fos_solver* h, double* z, const d2* src);
// step.cpp: the per-handle switches of the outer iteration, read into a new handle's state
void step_read_switches(StepState& s);
// cg.cpp: the CG state of a new handle (the operator must exist: cg_blocks reads op.dev.ndef) and its end, the solve, the CG half of fos_set_tuning
int cg_setup(fos_solver* h);
void cg_teardown(fos_solver* h);
typedef std::function<int(const LaunchCtx&)> PostFn;
// conjugategradient!(x, KKTMatrix(Q), rhs, r, p, Ap; tol, max_iters)      conjugategradients.jl:31-55
struct CgCall {
    d2* x; const d2* rhs; double tol; int maxit;
    const d2* apply_on = nullptr;              // the vector the start residual's operator product is taken of (default: x)
    const PostFn* post = nullptr;              // what follows the solve on the stream, enqueued gated behind the first batch ...
    bool* post_ran = nullptr;                  // ... and whether that batch sufficed (else the caller runs `post` itself)
    bool predict = true;                       // false: a solve outside the outer iteration -- first batch of cg_chunk, last_cg_pred left alone
};
int cg_solve(fos_solver* h, const CgCall& a, int64_t* iters);
int cg_set_tuning(fos_solver* h, int32_t cg_chunk, int32_t fuse_p);
// operator.cpp: the operator of a new handle (h->m, n, cus and row_sharded set), another grid for its sweep (fos_set_tuning), the resident solve's plan
int operator_setup(fos_solver* h, const int64_t* colptr, const int64_t* rowval, const double* nzval);
int operator_repartition(fos_solver* h, int nwg);
int resident_setup(fos_solver* h, int gmax);
int resident_lowp_ensure(fos_solver* h);    // the streamed plan's float copy and delta, once per plan: before a resident solve
// direct.cpp: prox!(y, S1::IndAffine([Q -I], 0), x) in the handle's exact form, the result left in h->SOL
int prox_affine_direct(fos_solver* h, const d2* x);

// ---- set-up scratch: device buffers that live to the end of a scope.  The first hipMalloc that fails stays in `err` (later requests give nullptr): ask for
// everything, then look at err once.
struct Scratch {
    std::vector<void*> held;
    hipError_t err = hipSuccess;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { for (void* p : held) (void)hipFree(p); }
    template <class T> T* alloc(size_t count) {
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, sizeof(T) * count);
        if (err != hipSuccess) return nullptr;
        held.push_back(p);
        return static_cast<T*>(p);
    }
};

// ---- the inverse of the dense symmetric positive definite matrix of a direct form (I + Q Q' or K) or of the factored IndAffine (A A'), direct.cpp.
// Its work-set: G (the caller's), L x L column-major (L % 64 == 0, padding = identity) of order c.l; B0, B1, B2: L x L work buffers; v0, v1: two L-vectors; partials: 256 doubles.
// The launches take the stream (and symv the order) from c.
struct DenseWork {
    LaunchCtx c{};
    int64_t L = 0;
    double *G = nullptr, *B0 = nullptr, *B1 = nullptr, *B2 = nullptr, *v0 = nullptr, *v1 = nullptr, *partials = nullptr;
    // the buffers the caller did not bring, from the set-up's scratch (a failure stays in s.err)
    void fill(Scratch& s) {
        const size_t L2 = (size_t)L * (size_t)L;
        for (double** b : {&B0, &B1, &B2}) *b = s.alloc<double>(L2);
        for (double** v : {&v0, &v1}) if (!*v) *v = s.alloc<double>((size_t)L);
        if (!partials) partials = s.alloc<double>(256);
    }
};
struct DenseOpts {
    const char *what, *gname;                  // the caller's name and the matrix's in messages
    int factor;                                // FOS_DIRECT_FACTOR_*
    bool pivot_fallback;                       // a pivot that fails on finite entries: Newton-Schulz instead of FOS_EINVAL
    double bar = 1e-12;                        // the inverse is accepted at this probe residual (Cholesky path) / max |G X - I| (Newton-Schulz)
    int newton_extra = 6;                      // Newton-Schulz steps past the planned ceil(log2 lambda_max) + 7, each followed by a look at the residual
};
int dense_spd_inverse(const DenseWork& k, const DenseOpts& o, double** Xout, DenseInv* st);
void direct_test_vector(int64_t k, int which, std::vector<double>& v);      // the four fixed vectors of the probe (which = 0: also the power iteration's start)
// affine_dense.hip: X = G^-1 for the factored forms (G of order m, L x L with the identity on its padding; X: L x L, the caller's) through dense_spd_inverse at `bar`,
// its work-set from a scratch of its own; own.what names the caller; lambda == 0 (IndAffine): a refusal names the full row rank A needs.  Synchronises `stream`.
int factored_inverse(const DevOwned& own, double lambda, int factor, double bar, hipStream_t stream, int64_t m, int64_t L, double* G, double* Xout, DenseInv* inv);

// (Owner: the handle, or a state with its own `owned` list -- ConeSet)
template <class Owner, class T>
int dev_alloc(Owner* h, T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { set_error("hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); return FOS_ENOMEM; }
    h->owned.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return FOS_OK;
}

template <class Owner, class T>
int dev_zeros(Owner* h, T** p, size_t count) {    // dev_alloc, zero-filled
    FOS_TRY(dev_alloc(h, p, count));
    FOS_HIP(hipMemset(*p, 0, sizeof(T) * count));
    return FOS_OK;
}

template <class T>
void dev_release(fos_solver* h, T** p) {          // frees a dev_alloc'd buffer before the handle's end
    if (!*p) return;
    auto it = std::find(h->owned.begin(), h->owned.end(), (void*)*p);
    if (it != h->owned.end()) h->owned.erase(it);
    (void)hipFree(*p);
    *p = nullptr;
}

template <class Owner, class T>
int dev_upload(Owner* h, T** p, const std::vector<T>& v) {
    FOS_TRY(dev_alloc(h, p, v.size()));
    if (!v.empty()) FOS_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FOS_OK;
}

// sum of squares in index order (norm(b), norm(c): values are O(1)-scaled problem data)
inline double sum_squares(const double* v, int64_t count) {
    double s = 0;
    for (int64_t i = 0; i < count; ++i) s += v[i] * v[i];
    return s;
}
}  // namespace fos
