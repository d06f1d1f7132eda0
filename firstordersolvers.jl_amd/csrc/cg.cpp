// libfoship: the conjugate-gradient solve behind prox_affine -- its state (fos_solver::cg, CgState), the two pure rules (sequence windows, which
// recurrence), the solve and the ABI entries about CG alone.  prox_affine, the step loops and fos_hsdematrix_prox (solver.cpp) call cg_solve.
#include <chrono>
#include <cmath>

#include "fos_solver.hpp"

namespace fos {

// ------------------------------------------------------------------------------------------------ the two pure rules
// A solve's sequence numbers: seq_base + 1 .. seq_base + 2 maxit + 3 (the folded exchanges: 2 j + phase; the resident solve: maxit + 2 exchange
// rounds, the streamed form's early r.r rounds on top) in windows of 2048 -- as many as `maxit` can use, so that no record of this solve carries a
// number of the next one.  Counted from maxit alone: the same on every rank (all ranks make the same calls), whatever form a shard takes.  A window
// run never wraps through epoch 0 mod 2^21 (sequence number 0 is never sent), it starts there instead (no speculation: the mark's initial value).
// cg_epoch: the last window used so far; *first: the solve's first window, *last: its last one = the new cg_epoch.
static void cg_windows(uint32_t cg_epoch, int maxit, uint32_t* first, uint32_t* last) {
    const uint32_t nwin = (uint32_t)std::min<int64_t>((2 * (int64_t)std::max(maxit, 0) + 4 + 2047) / 2048, (int64_t)1 << 20);
    uint32_t epoch = cg_epoch + 1u;                      // the solve's first window
    if (const uint32_t off = epoch & 0x1FFFFFu; off != 0u && off + (nwin - 1u) > 0x1FFFFFu) epoch += 0x200000u - off;
    *first = epoch;
    *last = epoch + (nwin - 1u);
}

// what decides the recurrence of a solve (fos_get_cg_variant fills it from the handle and the environment)
struct CgVariantIn {
    int request;                               // CgState::cg_variant: FOS_CG_*, -1 = the handle's default
    int32_t flags;                             // FOS_CGV_* (foship.h)
    int64_t l;                                 // rows of the KKT operator
    int plan_G, cus;                           // the resident plan's workgroups; the device's compute units
};
static int cg_resolve_variant(const CgVariantIn& in) {
    const auto on = [&in](int32_t f) { return (in.flags & f) != 0; };
    const bool asked = in.request >= 0, fuse_p = on(FOS_CGV_FUSE_P), sharded = on(FOS_CGV_SHARDED), row_sharded = on(FOS_CGV_ROW_SHARDED);
    const bool peer_on = on(FOS_CGV_MAILBOXES), fold_env = on(FOS_CGV_FOLD);
    // default: the reference's recurrence -- except where a CG iteration is bound by its launches, not its bytes: sharded handles (one
    // exchange per iteration instead of two) and cache-resident gather-type operators of 32 768 rows or more (C3: two launches per iteration
    // instead of three, 370 -> 385 iterations/s; the streamed operators C2 / C4 / C5 are faster on the reference recurrence; small problems
    // keep the reference's arithmetic).  Same Krylov iterates, same
    // iteration counting and stop test; FOS_CG_VARIANT=0 / fos_set_cg_variant restore the reference recurrence everywhere.
    int v = asked ? in.request
            : (fuse_p ? FOS_CG_FUSED_P : ((sharded || (on(FOS_CGV_CACHE_RESIDENT) && !row_sharded && in.l >= 32768)) ? FOS_CG_MERGED_UPDATE : FOS_CG_REFERENCE));
    // the resident solve: on request wherever the operator qualifies; by default on sharded handles whose sums travel through mailboxes and
    // whose shards ALL qualify (FOS_RESIDENT_DEFAULT=0: never by default).  Sharded without mailboxes (RCCL, the caller's collective): a
    // collective call cannot sit inside a kernel -- the launch-per-iteration form of the same recurrence runs instead.
    const bool res_usable = on(FOS_CGV_QUALIFIES) && !row_sharded && (!sharded || (peer_on && fold_env && on(FOS_CGV_ALL_QUALIFY)));
    const bool by_default = !asked && !fuse_p && res_usable && on(FOS_CGV_RESIDENT_DEFAULT);
    if (by_default && sharded) v = FOS_CG_RESIDENT;
    // one GPU: the STREAMED form where it fills at least half of the chip (C4: 66.3 us per CG iteration against 89 for three launches); operators
    // small enough for the register form keep the reference's arithmetic by default
    if (by_default && !sharded && on(FOS_CGV_PLAN_STREAMED) && 2 * in.plan_G >= in.cus) v = FOS_CG_RESIDENT;
    if (v == FOS_CG_RESIDENT && !res_usable) v = FOS_CG_MERGED_UPDATE;
    if (v == FOS_CG_FUSED_P && on(FOS_CGV_WINDOW_PANELS)) v = FOS_CG_REFERENCE;      // (FOS_CG_FUSE_P is set for the whole process: window-panel handles keep three launches)
    if (v == FOS_CG_MERGED_SWEEP && sharded) v = FOS_CG_MERGED_UPDATE;
    if (v == FOS_CG_MERGED_UPDATE && peer_on && !fold_env) v = FOS_CG_REFERENCE;
    return v;
}
// fos_bench_cg_chain's own rule (single-GPU handles): the explicit request, else fuse_p, else the reference recurrence; no default is merged or
// resident, and a resident request runs the reference chain
static int cg_chain_variant(int request, bool fuse_p, bool window_panels) {
    const int v = request >= 0 ? request : (fuse_p ? FOS_CG_FUSED_P : FOS_CG_REFERENCE);
    return (v == FOS_CG_RESIDENT || (v == FOS_CG_FUSED_P && window_panels)) ? FOS_CG_REFERENCE : v;
}

// ------------------------------------------------------------------------------------------------ set-up and end
int cg_setup(fos_solver* h) {
    CgState& cg = h->cg;
    FOS_HIP(hipHostMalloc((void**)&cg.mark, sizeof(HostMark), hipHostMallocMapped));
    memset(cg.mark, 0, sizeof(HostMark));
    {
        void* dp = nullptr;
        FOS_HIP(hipHostGetDevicePointer(&dp, cg.mark, 0));
        const unsigned long long addr = (unsigned long long)(uintptr_t)dp;
        FOS_HIP(hipMemcpy(&h->st->hostmark, &addr, sizeof(addr), hipMemcpyHostToDevice));
    }
    cg.speculate = !(getenv("FOS_SPECULATE") && atoi(getenv("FOS_SPECULATE")) == 0);
    // The p update of CG can ride on the next sweep (two launches per iteration, launch_kkt2_cg): built and measured -- on
    // MI355X it is SLOWER than the separate launch at every size tried (C4: sweep 59 -> 86 us against a 10 us p update kernel;
    // 64-block shard: 13 -> 20 us against 5 us), so it stays an option (fos_set_tuning / FOS_CG_FUSE_P)
    if (const char* e = getenv("FOS_CG_FUSE_P")) cg.fuse_p = atoi(e) != 0;
    if (const char* e = getenv("FOS_CG_VARIANT")) cg.cg_variant = std::max(-1, std::min((int)FOS_CG_RESIDENT, atoi(e)));
    if (const char* e = getenv("FOS_CG_CHUNK")) cg.cg_chunk = std::max(1, atoi(e));
    FOS_TRY(dev_zeros(h, &cg.pre_sums, 128));            // 16 producers x 3 sums x 2 self-validating words (sweep_sums3)
    cg.pre_on = !(getenv("FOS_CG_PRE") && atoi(getenv("FOS_CG_PRE")) == 0);
    cg.cg_blocks = std::min(h->vec_blocks, getenv("FOS_CG_BLOCKS") ? std::max(1, atoi(getenv("FOS_CG_BLOCKS"))) : 2 * h->cus);
    // the x,r update kernel also adds the slot lists of the rows spread over dual tiles (`def_lpr` lanes per row): its grid must
    // cover them in ONE pass even when the vectors are short (dense LP C2: 15 000 such rows x 16 lanes against l = 15 001 --
    // sized by l alone the kernel took 105 us instead of 17)
    if (h->op.dev.ndef > 0)
        cg.cg_blocks = std::max<int>(cg.cg_blocks, (int)std::min<int64_t>(1024, ((int64_t)h->op.dev.ndef * h->op.dev.def_lpr + 255) / 256));
    cg.cg_blocks = std::min(cg.cg_blocks, 1024);         // (cg_close_iteration adds at most 1024 r.r records per wavefront)
    return FOS_OK;
}
void cg_teardown(fos_solver* h) { if (h->cg.mark) (void)hipHostFree(h->cg.mark); }

// FOS_CG_FUSED_P closes the previous iteration and builds p on the fly inside kkt2_kernel; the window-panel sweeps (kkt2_win_kernel) have no such
// form -- they would apply M to the PREVIOUS p and leave the iteration unclosed -- so the variant is refused where the operator is stored that way
static int refuse_fused_p_on_window_panels(const fos_solver* h) {
    if (h->op.dev.npanel == 0) return FOS_OK;
    set_error("FOS_CG_FUSED_P: the operator is stored in window panels, whose sweeps cannot build p on the fly (row-block and tile storage only)");
    return FOS_EUNSUPPORTED;
}
int cg_set_tuning(fos_solver* h, int32_t cg_chunk, int32_t fuse_p) {
    if (fuse_p > 0) FOS_TRY(refuse_fused_p_on_window_panels(h));
    if (fuse_p >= 0) { h->cg.fuse_p = fuse_p != 0; h->cg.cg_variant = -1; }
    if (cg_chunk > 0) h->cg.cg_chunk = cg_chunk;
    return FOS_OK;
}

// ------------------------------------------------------------------------------------------------ the solve
// Has CG solve number `epoch` ended within its first batch of iterations?  No stream synchronisation and nothing in the stream:
// the kernel that ends a solve writes HostMark.seq in pinned host memory, the marked p update of a batch that runs out before
// convergence writes HostMark.batch; the host spins on the two (and looks at the stream now and then, in case neither comes).
static int wait_cg_mark(fos_solver* h, uint32_t epoch, int32_t batch_id, bool* ended) {
    FOS_TRY(check_launch("poll"));
    volatile HostMark* m = h->cg.mark;
    // a wall-clock bound (FOS_CG_WAIT_S, default 120 s): a kernel of the solve that never ends must not hang the host either
    static const double wait_s = getenv("FOS_CG_WAIT_S") ? atof(getenv("FOS_CG_WAIT_S")) : 120.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 1;; ++spin) {
        if (__atomic_load_n(&m->seq, __ATOMIC_ACQUIRE) == epoch) { *ended = true; break; }
        if (__atomic_load_n(&m->batch, __ATOMIC_ACQUIRE) == batch_id) { *ended = false; break; }
        __builtin_ia32_pause();
        if ((spin & 0xFFFFu) == 0 && hipStreamQuery(h->stream) == hipSuccess) {          // everything enqueued has run
            if (__atomic_load_n(&m->seq, __ATOMIC_ACQUIRE) == epoch) { *ended = true; break; }
            if (__atomic_load_n(&m->batch, __ATOMIC_ACQUIRE) == batch_id) { *ended = false; break; }
            // no mark: a kernel of the solve gave up (a peer exchange timed out, ...) -- the ordinary state read reports why
            FOS_TRY(poll_state(h));
            *ended = h->st_host->done != 0;
            return FOS_OK;
        }
        if ((spin & 0xFFFFFu) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > wait_s) {
            set_error("CG solve %u: neither its end mark nor its batch mark arrived within %.0f s (a kernel of the solve does not finish)", epoch, wait_s);
            return FOS_EHIP;
        }
    }
    if (*ended) { h->st_host->done = 1; h->st_host->iter = m->iter; h->st_host->hit_max = m->hit_max; h->st_host->rr = m->rr; }
    else h->st_host->done = 0;
    return FOS_OK;
}

// one solve, as its pieces below see it: built once at the top of cg_solve (fos_bench_cg_chain fills its own)
struct CgRun {
    fos_solver* h;
    LaunchCtx c;
    // which recurrence: the reference's (three launches, two reduction points per iteration), the merged-reduction form (two launches, one
    // reduction point) or the resident launch; start_fused: single GPU, reference recurrence -- the solve starts like the merged one: sweep, ONE
    // launch for r_0 = rhs - M v, p_1 = r_0, the tau row, the slot-spread rows and the r.r records (added by the sweep of iteration 1) instead of five
    bool resident, merged, close_in_update, fuse_p, start_fused;
    bool fold;                                 // the exchanges of a sharded handle happen inside the CG kernels (folded mailboxes)
    bool rccl;                                 // sums cross the ranks between the kernels (reduce kernel + all-reduce, or unfolded mailboxes)
    bool spec;                                 // `post` is enqueued behind the first batch, gated
    uint32_t seq_base;                         // + 2 j + phase
    int32_t batch_id;
    d2* x; const d2* rhs; const d2* v;         // v: the vector the start applies M to
    double tol; int maxit;
    int next_j;                                // iteration number of the next enqueued launch group (if CG still runs)
    bool mark_last;                            // the batch being enqueued ends with a marked launch
};
static CgRun cg_run(fos_solver* h, const CgCall& a, int variant, uint32_t epoch) {
    CgRun r{};
    r.h = h; r.c = h->ctx();
    r.fold = h->tr.peer_on && peer_fold_env();
    r.rccl = h->sharded() && !r.fold;
    r.resident = variant == FOS_CG_RESIDENT;
    r.merged = variant == FOS_CG_MERGED_SWEEP || variant == FOS_CG_MERGED_UPDATE;
    r.close_in_update = variant == FOS_CG_MERGED_UPDATE;
    r.fuse_p = variant == FOS_CG_FUSED_P;
    static const bool start_env = !(getenv("FOS_CG_FUSED_START") && atoi(getenv("FOS_CG_FUSED_START")) == 0);
    r.start_fused = !r.merged && !h->sharded() && !r.c.between && start_env;
    r.seq_base = (uint32_t)(epoch * 2048u);
    // (sharded: only with the exchanges folded into the CG kernels -- no collective call sits in the stream -- and only for GAP,
    //  whose post-solve kernels contain no reduction; every rank takes the same decisions, so all mispredict together.
    //  Solve number 0 mod 2^21 is the mark's initial value.)
    r.spec = a.post && h->cg.speculate && !r.c.between && !r.fuse_p && (r.seq_base >> 11) != 0u &&
             (!h->sharded() || (r.fold && h->step.alg != FOS_ALG_GAPA));
    r.batch_id = (int32_t)(((r.seq_base >> 11) & 0x7FFFFFu) << 8 | 1u);
    r.x = a.x; r.rhs = a.rhs; r.v = a.apply_on ? a.apply_on : a.x; r.tol = a.tol; r.maxit = a.maxit;
    r.next_j = 1;
    r.mark_last = r.spec;                      // the first batch ends with a marked launch
    return r;
}

// the two descriptors of iteration j
static CgIter cg_iter(const CgRun& r, int j) {
    fos_solver* h = r.h;
    CgIter it;
    it.j = j; it.r = h->R; it.p_prev = h->PB[(j - 1) & 1]; it.p_cur = h->PB[j & 1];
    it.fuse_p = r.fuse_p; it.rr_from_reduced = r.rccl ? 1 : 0; it.fold = r.fold ? &h->tr.peer : nullptr; it.seq_base = r.seq_base;
    it.start_fused = r.start_fused;
    return it;
}
static CgmIter cgm_iter(const CgRun& r, int j) {
    fos_solver* h = r.h;
    CgmIter it;
    it.j = j; it.x = r.x; it.r = h->R; it.p = h->PB[0]; it.s = h->PB[1]; it.w = h->AP;
    it.close_in_update = r.close_in_update; it.from_reduced = r.rccl ? 1 : 0; it.fold = r.fold ? &h->tr.peer : nullptr; it.seq_base = r.seq_base;
    return it;
}

// what follows the solve, gated on DevState.done, then the mark: did the solve end within what is enqueued?
static int cg_speculate(const CgRun& r, const CgCall& a, bool* ended) {
    LaunchCtx cg = r.c;
    cg.gate = &r.h->st->done;
    FOS_TRY((*a.post)(cg));
    FOS_TRY(wait_cg_mark(r.h, (uint32_t)(r.seq_base >> 11), r.batch_id, ended));
    if (a.post_ran) *a.post_ran = *ended;
    return FOS_OK;
}

// the whole solve is ONE launch (resident.hip): nothing to enqueue ahead, nothing to predict; what follows the solve is enqueued behind it
// (gated on DevState.done, which the launch sets when it ends) and the host reads the iteration count from the mark the launch leaves
static int cg_resident(const CgRun& r, const CgCall& a) {
    fos_solver* h = r.h;
    FOS_TRY(resident_lowp_ensure(h));                  // (a handle whose default is another recurrence builds its float copy here, once)
    const int pe = prof_begin(h, FOS_PROF_RESIDENT, 1, h->prof_seen[FOS_PROF_RESIDENT]++);
    const hipError_t le = launch_cg_resident(r.c, h->op.res, r.x, r.rhs, r.v, r.tol, r.maxit, r.fold ? &h->tr.peer : nullptr, r.seq_base);
    prof_end(h, pe);
    if (le != hipSuccess) { set_error("resident CG launch: %s", hipGetErrorString(le)); return FOS_EHIP; }
    if (r.spec) {
        bool ended = false;
        FOS_TRY(cg_speculate(r, a, &ended));
        if (!ended) { set_error("resident CG solve %u ended without its mark", (unsigned)(r.seq_base >> 11)); return FOS_EHIP; }
    } else {
        FOS_TRY(poll_state(h));
        if (!h->st_host->done) { set_error("resident CG solve %u did not finish", (unsigned)(r.seq_base >> 11)); return FOS_EHIP; }
    }
    return FOS_OK;
}

// The start of a launch-per-iteration solve.  Merged: sweep M v, ONE launch for r = rhs - M v (+ r.r records, tau row, slot-spread rows, the solve's
// scalars), then w_0 = M r_0, the sweep every iteration's update starts from (it also adds g_0 = r_0.r_0 unless the first update does).  Fused (the
// reference recurrence on one GPU): the same two launches, which also leave p_1 = r_0, and no sweep.  Plain: the reference's five launches.
static int cg_start(const CgRun& r) {
    fos_solver* h = r.h;
    const LaunchCtx& c = r.c;
    const int po = prof_begin_other(h, 0);
    if (r.merged || r.start_fused) {
        const CgmIter it0 = cgm_iter(r, 0);
        launch_cgm_apply(c, it0, r.v);                                     // :32  mul!(Ap, A, x)
        if (c.between) FOS_TRY(c.between(c.between_arg));                   // (neither on a handle that starts fused)
        if (r.rccl) { launch_reduce1(c, c.S.nwg, 3, 0, 0); FOS_TRY(allreduce(h, 3)); }
        launch_cgm_start(c, it0, r.rhs, r.v, r.tol, r.maxit, r.merged ? nullptr : h->PB[1]);     // :33-36   (fused: p_1 in buffer 1)
        prof_end(h, po);
        if (!r.merged) return FOS_OK;
        const int pe = prof_begin(h, FOS_PROF_KKT, 0, h->cg.cg_total);
        launch_cgm_sweep(c, it0, r.close_in_update ? -1 : 0);
        prof_end(h, pe);
        return FOS_OK;
    }
    int fr = 0;
    FOS_TRY(kkt_apply_full(h, c, r.v, h->AP));                             // :32  mul!(Ap, A, x)
    launch_cg_init(c, r.rhs, h->AP, h->R, h->PB[1]);                       // :33-34   (p_1 in buffer 1)
    FOS_TRY(finish_reduce(h, c, c.vec_blocks, 1, 0, &fr));
    launch_cg_init_finalize(c, h->R, r.tol, r.maxit, fr);                  // :35-36
    prof_end(h, po);
    return FOS_OK;
}

// the profiling ordinal of an iteration's vector update: a quarter of the sweeps' rate, other iterations
static int64_t cgvec_ordinal(const fos_solver* h, int j) {
    const int64_t k = h->cg.cg_total + j - 1;
    return k % 4 == 1 ? k / 4 : 1;
}

// merged reduction, sharded without folded mailboxes: the sweep's three sums and the update's r.r cross the ranks together,
// between the sweep of iteration j-1 and the update of iteration j -- ONE all-reduce of four doubles per iteration
static int merged_reduce(const CgRun& r, int j) {
    const LaunchCtx& c = r.c;
    if (c.between) FOS_TRY(c.between(c.between_arg));         // row-sharded: A'y partial sums over the ranks (n-vector)
    if (!r.rccl) return FOS_OK;
    launch_reduce1(c, c.S.nwg, 3, 1, 0);
    LaunchCtx c2 = c;
    c2.partials = c.partials + 3 * (size_t)PART_CAP + (size_t)((j - 1) & 1) * CGM_RR_STRIDE;
    c2.reduced = c.reduced + 3;
    launch_reduce1(c2, c.cg_blocks, 1, 1);
    return allreduce(r.h, 4);
}
// up to `count` further iterations of the merged recurrence, every launch gated on DevState.done
static int enqueue_merged(CgRun& r, int count) {
    fos_solver* h = r.h;
    const LaunchCtx& c = r.c;
    for (int q = 0; q < count && r.next_j <= r.maxit; ++q, ++r.next_j) {
        const int j = r.next_j;
        CgmIter it = cgm_iter(r, j);
        if (r.mark_last && (q == count - 1 || j == r.maxit)) it.batch_mark = r.batch_id;
        FOS_TRY(merged_reduce(r, j));
        // launch 1: scalars, p = r + beta p, s = w + beta s, x += alpha p, r -= alpha s, r.r partials             :39-41,:46-50
        int pe = prof_begin(h, FOS_PROF_CGVEC, j, cgvec_ordinal(h, j));
        launch_cgm_update(c, it, false);
        prof_end(h, pe);
        // launch 2: [close iteration j: r.r, stop test] sweep w = M r + partial sums                               :38,:42
        // (closing in the sweep: the sweep behind the LAST update returns in its prologue -- recorded as iteration j+1, which
        //  the profile drops)
        pe = prof_begin(h, FOS_PROF_KKT, j + (r.close_in_update ? 0 : 1), h->cg.cg_total + j);
        launch_cgm_sweep(c, it, r.close_in_update ? -1 : j);
        prof_end(h, pe);
    }
    if (r.close_in_update) {                   // the last enqueued iteration is closed by a one-workgroup launch of the update kernel
        CgmIter it = cgm_iter(r, r.next_j);
        if (r.mark_last) it.batch_mark = r.batch_id;
        FOS_TRY(merged_reduce(r, r.next_j));
        launch_cgm_update(c, it, true);
    }
    return FOS_OK;
}
// the same of the reference recurrence
static int enqueue_reference(CgRun& r, int count) {
    fos_solver* h = r.h;
    const LaunchCtx& c = r.c;
    for (int q = 0; q < count && r.next_j <= r.maxit; ++q, ++r.next_j) {
        const int j = r.next_j;
        CgIter it = cg_iter(r, j);
        if (r.mark_last && (q == count - 1 || j == r.maxit)) it.batch_mark = r.batch_id;
        // launch 1: [close iteration j-1: r.r, stop test, beta; p_j on the fly] KKT sweep Ap = M p_j + partial sums   :38,:42-50
        int pe = prof_begin(h, FOS_PROF_KKT, j, h->cg.cg_total + j - 1);
        launch_kkt2_cg(c, it, h->AP);
        prof_end(h, pe);
        int f1 = 0;
        if (c.between) FOS_TRY(c.between(c.between_arg));         // row-sharded: A'y partial sums over the ranks (n-vector)
        if (r.rccl) { launch_reduce1(c, c.S.nwg, 3, 1, 0); FOS_TRY(allreduce(h, 3)); f1 = 1; }
        // launch 2: alpha, tau rows, slot-spread rows, x += alpha p, r -= alpha Ap, r.r partials                       :39-41
        pe = prof_begin(h, FOS_PROF_CGVEC, j, cgvec_ordinal(h, j));
        launch_cg_update(c, it, r.x, h->R, h->AP, f1);
        if (r.rccl) {
            LaunchCtx c2 = c;
            c2.partials = c.partials + 3 * (size_t)PART_CAP;
            launch_reduce1(c2, c.cg_blocks, 1, 1);
            FOS_TRY(allreduce(h, 1));
        }
        // gather-bound operators: closing the iteration and p_{j+1} = r + beta p_j stay a launch of their own           :42-51
        if (!r.fuse_p) launch_cg_pupdate(c, it, r.x, h->PB[(j + 1) & 1]);
        prof_end(h, pe);
    }
    // the last update of the batch is closed by a one-workgroup launch (a following batch's sweep repeats it, same result)
    if (r.fuse_p) launch_cg_stop_check(c, cg_iter(r, r.next_j));
    return FOS_OK;
}
static int cg_enqueue(CgRun& r, int count) { return r.merged ? enqueue_merged(r, count) : enqueue_reference(r, count); }

// the first batch: what the last predicted solve took, or a chunk
static int cg_first_batch(const fos_solver* h, const CgCall& a) {
    static const int pred_slack = getenv("FOS_CG_SLACK") ? atoi(getenv("FOS_CG_SLACK")) : 1;   // iterations enqueued beyond the last solve's count (each costs a few gated no-op launches when not needed; too few costs a poll)
    // (the slack iteration is dropped once three solves in a row took the same number of iterations: steady state of a
    // well-conditioned problem -- C4: 17, 17, 17, ... -- where it would be three gated no-op launches per solve)
    const int slack = (pred_slack == 1 && h->cg.cg_same_run >= 3) ? 0 : pred_slack;
    const int pred = a.predict ? h->cg.last_cg_pred : 0;
    return std::max(1, std::min(pred > 0 ? pred + slack : h->cg.cg_chunk, a.maxit));
}

// the book-keeping behind a solve: the host's copy of DevState says how it ended
static void cg_close(const CgRun& r, size_t prof_start, bool predict, int64_t* iters) {
    fos_solver* h = r.h;
    CgState& cg = h->cg;
    const int it = h->st_host->iter;
    *iters = it;
    // profiling: launches enqueued past convergence were gated no-ops -- drop their event pairs (the resident launch is never one)
    for (size_t k = prof_start; !r.resident && k < h->prof_used; ++k)
        if (h->prof_recs[k].cls != FOS_PROF_OTHER && h->prof_recs[k].j > it) h->prof_recs[k].cls = -1;
    cg.cg_same_run = (it == (predict ? cg.last_cg_pred : 0)) ? cg.cg_same_run + 1 : 0;
    if (predict) cg.last_cg_pred = it;
    cg.cg_total += it;
    if (h->st_host->hit_max) cg.hit_max_accum = 1;
}

// Device resident: the host enqueues iterations AHEAD (every CG kernel is gated on DevState.done) and polls once per batch.
// a.apply_on (default: x): the vector the start residual's operator product is taken of -- prox_affine passes x - (0, in.y)
// together with rhs = in, which is rhs - M x without ever forming rhs (see there).
// a.post (optional): what follows the solve on the stream (relaxation, cone projection, ...), taking a LaunchCtx whose `gate`
// it must hand to every launch.  It is enqueued right behind the FIRST batch of iterations, gated on DevState.done, and the host
// then reads the mark the batch leaves: when the batch sufficed (the steady state) the GPU has gone straight on while the host was
// still finding that out, and *a.post_ran = true.  Otherwise the gated launches were no-ops, CG continues as usual and the caller
// runs `post` itself.
int cg_solve(fos_solver* h, const CgCall& a, int64_t* iters) {
    uint32_t epoch = 0;
    cg_windows(h->cg.cg_epoch, a.maxit, &epoch, &h->cg.cg_epoch);
    int32_t variant = FOS_CG_REFERENCE;
    FOS_TRY(fos_get_cg_variant(h, &variant));
    CgRun r = cg_run(h, a, variant, epoch);
    const size_t prof_start = h->prof_used;
    if (r.resident) {
        FOS_TRY(cg_resident(r, a));
    } else {
        FOS_TRY(cg_start(r));
        FOS_TRY(cg_enqueue(r, cg_first_batch(h, a)));
        r.mark_last = false;
        bool ended = false;
        if (r.spec) FOS_TRY(cg_speculate(r, a, &ended));
        else FOS_TRY(poll_state(h));
        while (!h->st_host->done) {
            FOS_TRY(cg_enqueue(r, h->cg.cg_chunk));
            FOS_TRY(poll_state(h));
        }
    }
    cg_close(r, prof_start, a.predict, iters);
    return FOS_OK;
}

}  // namespace fos

using namespace fos;

// ------------------------------------------------------------------------------------------------ C ABI: the entries about CG alone
extern "C" {

int fos_host_cg_windows(int64_t cg_epoch, int64_t maxit, int64_t* first_epoch, int64_t* new_cg_epoch) {
    if (!first_epoch || !new_cg_epoch || cg_epoch < 0 || cg_epoch > (int64_t)UINT32_MAX || maxit < INT32_MIN || maxit > INT32_MAX) { set_error("bad argument"); return FOS_EINVAL; }
    uint32_t first = 0, last = 0;
    cg_windows((uint32_t)cg_epoch, (int)maxit, &first, &last);
    *first_epoch = first; *new_cg_epoch = last;
    return FOS_OK;
}

int fos_host_cg_variant(int32_t request, int32_t flags, int64_t l, int32_t plan_workgroups, int32_t cus, int32_t* variant) {
    if (!variant || request < -1 || request > FOS_CG_RESIDENT) { set_error("bad argument"); return FOS_EINVAL; }
    *variant = cg_resolve_variant(CgVariantIn{request, flags, l, plan_workgroups, cus});
    return FOS_OK;
}

// which CG recurrence the affine projection runs (FOS_CG_*; -1: the handle's default)
int fos_set_cg_variant(fos_handle h, int32_t variant) {
    if (!h || variant < -1 || variant > FOS_CG_RESIDENT) { set_error("unknown CG variant %d", (int)variant); return FOS_EINVAL; }
    if (variant == FOS_CG_RESIDENT && !h->op.res_ok) {
        set_error("FOS_CG_RESIDENT: the operator does not qualify (%s)", h->op.res_plan.why.empty() ? "no plan" : h->op.res_plan.why.c_str());
        return FOS_EUNSUPPORTED;
    }
    if (variant == FOS_CG_FUSED_P) FOS_TRY(refuse_fused_p_on_window_panels(h));
    if (variant == FOS_CG_RESIDENT) { FOS_HIP(hipSetDevice(h->device)); FOS_TRY(resident_lowp_ensure(h)); }      // (asked for: its float copy is built now)
    h->cg.cg_variant = variant;
    if (variant >= 0) h->cg.fuse_p = variant == FOS_CG_FUSED_P;
    h->cg.last_cg_pred = 0; h->cg.cg_same_run = 0;
    return FOS_OK;
}

// the variant the next affine projection will run (the default resolved: sharded handles take the merged recurrence)
int fos_get_cg_variant(fos_handle h, int32_t* variant) {
    if (!h || !variant) { set_error("NULL argument"); return FOS_EINVAL; }
    const bool res_default = !(getenv("FOS_RESIDENT_DEFAULT") && atoi(getenv("FOS_RESIDENT_DEFAULT")) == 0);      // (read at every call: bench.py turns it off after a failed warm-up)
    const std::pair<bool, int32_t> flags[] = {
        {h->cg.fuse_p, FOS_CGV_FUSE_P}, {h->sharded(), FOS_CGV_SHARDED}, {h->tr.peer_on, FOS_CGV_MAILBOXES}, {peer_fold_env(), FOS_CGV_FOLD},
        {h->row_sharded, FOS_CGV_ROW_SHARDED}, {h->op.res_ok, FOS_CGV_QUALIFIES}, {h->op.res_all, FOS_CGV_ALL_QUALIFY},
        {h->op.dev.resident != 0, FOS_CGV_CACHE_RESIDENT}, {h->op.dev.npanel > 0, FOS_CGV_WINDOW_PANELS}, {h->op.res_plan.stream != 0, FOS_CGV_PLAN_STREAMED},
        {res_default, FOS_CGV_RESIDENT_DEFAULT}};
    CgVariantIn in{h->cg.cg_variant, 0, h->l, h->op.res_plan.G, h->cus};
    for (const auto& f : flags) if (f.first) in.flags |= f.second;
    *variant = cg_resolve_variant(in);
    return FOS_OK;
}

int fos_get_cg_total(fos_handle h, int64_t* total) {
    if (!h || !total) { set_error("NULL argument"); return FOS_EINVAL; }
    *total = h->cg.cg_total;
    return FOS_OK;
}

int fos_cg_kkt(fos_handle h, double* x, const double* rhs, double tol, int64_t max_iters, int64_t* iters) {
    if (!h || !x || !rhs || max_iters < 1) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(upload_plain(h, h->W, x));
    FOS_TRY(upload_plain(h, h->RHS, rhs));
    int64_t it = 0;
    CgCall call{h->W, h->RHS, tol, (int)std::min<int64_t>(max_iters, INT32_MAX)};
    call.predict = false;
    FOS_TRY(cg_solve(h, call, &it));
    if (iters) *iters = it;
    return download_plain(h, x, h->W);
}

int fos_bench_cg_chain(fos_handle h, int32_t iters, int32_t reps, int32_t use_graph, double* ms_per_iter) {
    if (!h || iters < 1 || reps < 1 || !ms_per_iter) { set_error("bad argument"); return FOS_EINVAL; }
    if (h->sharded()) { set_error("fos_bench_cg_chain: single-GPU handles only"); return FOS_EUNSUPPORTED; }
    FOS_HIP(hipSetDevice(h->device));
    // CG on M y = X from y = 0 with a tolerance that is never met: every enqueued iteration really runs.  No profiling brackets (the chain may be
    // captured), no batch marks, no closing launch behind a chain
    CgRun r{};
    r.h = h; r.c = h->ctx();
    const int variant = cg_chain_variant(h->cg.cg_variant, h->cg.fuse_p, h->op.dev.npanel > 0);
    r.merged = variant == FOS_CG_MERGED_SWEEP || variant == FOS_CG_MERGED_UPDATE;
    r.close_in_update = variant == FOS_CG_MERGED_UPDATE;
    r.fuse_p = variant == FOS_CG_FUSED_P;
    r.x = h->W; r.rhs = h->RHS; r.v = h->W; r.tol = -1.0; r.maxit = INT32_MAX;
    const LaunchCtx& c = r.c;
    FOS_HIP(hipMemcpyAsync(h->RHS, h->X, sizeof(d2) * h->l, hipMemcpyDeviceToDevice, h->stream));
    FOS_HIP(hipMemsetAsync(h->W, 0, sizeof(d2) * h->l, h->stream));
    FOS_TRY(kkt_apply_full(h, c, h->W, h->AP));
    launch_cg_init(c, h->RHS, h->AP, h->R, h->PB[1]);
    launch_cg_init_finalize(c, h->R, r.tol, r.maxit, 0);
    // (the producer flags of the update kernels carry the launch's sequence number: a replayed graph would present the SAME
    //  numbers again and the consumers would not wait -- the graph runs without the producers)
    if (use_graph) r.c.pre = nullptr;
    uint32_t chain_no = 0;
    auto chain = [&]() {
        r.seq_base = (++chain_no) * 2048u;
        if (r.merged) {
            const CgmIter it0 = cgm_iter(r, 0);
            launch_cgm_apply(c, it0, r.v);
            launch_cgm_start(c, it0, r.rhs, r.v, r.tol, r.maxit);
            launch_cgm_sweep(c, it0, r.close_in_update ? -1 : 0);
            for (int j = 1; j <= iters; ++j) {
                const CgmIter it = cgm_iter(r, j);
                launch_cgm_update(c, it, false);
                launch_cgm_sweep(c, it, r.close_in_update ? -1 : j);
            }
            return;
        }
        for (int j = 1; j <= iters; ++j) {
            const CgIter it = cg_iter(r, j);
            launch_kkt2_cg(c, it, h->AP);
            launch_cg_update(c, it, r.x, h->R, h->AP, 0);
            if (!r.fuse_p) launch_cg_pupdate(c, it, r.x, h->PB[(j + 1) & 1]);
        }
    };
    hipEvent_t e0, e1;
    FOS_HIP(hipEventCreate(&e0));
    FOS_HIP(hipEventCreate(&e1));
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (use_graph) {
        FOS_HIP(hipStreamSynchronize(h->stream));
        FOS_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        chain();
        FOS_HIP(hipStreamEndCapture(h->stream, &graph));
        FOS_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        FOS_HIP(hipGraphLaunch(exec, h->stream));          // warm
    } else {
        chain();                                           // warm
    }
    FOS_HIP(hipEventRecord(e0, h->stream));
    for (int rep = 0; rep < reps; ++rep) {
        if (use_graph) FOS_HIP(hipGraphLaunch(exec, h->stream));
        else chain();
    }
    FOS_HIP(hipEventRecord(e1, h->stream));
    FOS_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FOS_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_iter = (double)ms / ((double)reps * iters);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    // leave the handle as fos_reset_affine + a fresh iterate would: the CG state used above is scratch
    FOS_TRY(check_launch("fos_bench_cg_chain"));
    FOS_TRY(poll_state(h));
    return FOS_OK;
}

}  // extern "C"
