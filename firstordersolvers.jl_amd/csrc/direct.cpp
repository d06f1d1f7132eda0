// libfoship, direct = true (HSDE.jl:12-15): S1 = IndAffine([Q -I], 0) as an exact projection.  Its forms, their projections, their set-ups and the
// fos_*direct* entries of include/foship.h (the handle and the helpers shared with solver.cpp: fos_solver.hpp).
//
// The ACTIVE form is one field, fos_solver::direct_form (DirectForm: the values of fos_get_direct_mode).  What is STORED does not depend on it: Ginv (dense
// inverse), blk_ready (block form's data), red_ready (reduced form's data); direct_factor_req / direct_inv describe the stored dense or reduced inverse.
// The transitions (fos_enable_direct3 with the form after FOS_DIRECT_MODE=reduced and the factor after FOS_DIRECT_FACTOR; "set-up" = direct_setup_s is rewritten):
//
//   call                      condition                                        active form afterwards       stored afterwards                           set-up
//   ------------------------  -----------------------------------------------  ---------------------------  ------------------------------------------  ------
//   enable(AUTO, factor)      Ginv stored with ANOTHER factor                  (Ginv released first; then the rows below -- where one of them fails, a
//                                                                              handle that was DENSE stays DENSE with no Ginv: as before, see (**))
//                             Ginv or a ready block form stored                BLOCK if blk_ready else      unchanged; reduced data released            no
//                                                                              DENSE, at once -- whatever
//                                                                              FOS_DIRECT_MODE says
//                             mode auto|block, A'A separable (blkdir_setup)    BLOCK                        + block data; reduced data released         yes
//                             mode block, not separable                        unchanged (FOS_EUNSUPPORTED)
//                             sharded handle, no block form                    unchanged (FOS_EUNSUPPORTED)
//                             l > FOS_DIRECT_DENSE_MAX or mode cg              CG                           reduced data released                       yes (*)
//                             otherwise                                        DENSE                        + Ginv, factor; reduced data released       yes
//   enable(REDUCED, factor)   reduced data ready with the same factor          REDUCED                      Ginv released; block data stays             no
//                             otherwise (not ready, or another factor)         REDUCED                      reduced data rebuilt; Ginv released;        yes
//                                                                                                           block data stays
//                             the set-up fails before it touches the handle    unchanged                    unchanged
//                             ... or later                                     OFF if it was REDUCED (**),  reduced data released
//                                                                              else unchanged
//   disable                                                                    OFF                          unchanged (a later enable finds it)         no
//
//   (*) nothing is built for CG, but the time spent finding that out (the block form's attempt) is recorded: direct_setup_s is rewritten whenever AUTO
//       found neither Ginv nor a ready block form on entry, and whenever reduced_setup ran.
//   (**) the one transition that differs from the code this file replaces: there a REDUCED handle whose re-set-up failed reported DENSE, with neither inverse
//       stored.  The AUTO row above still ends in such a state; a later enable or disable leaves it.
//   Only one of Ginv and the reduced data exists at a time ("one form's inverse at a time"); the block form's data, once built, lives until fos_destroy.
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>

#include "fos_solver.hpp"

using namespace fos;

// ---- the environment switches of direct = true: constructing a DirectEnv reads all five (fos_enable_direct3 does, at every call; nothing is cached --
// FOS_BLKDIR_FULL_APPLY stays with blkdir_setup)
struct DirectEnv {
    const std::string mode = getenv("FOS_DIRECT_MODE") ? getenv("FOS_DIRECT_MODE") : "auto";                             // auto|block|dense|cg|reduced
    const char* const factor = getenv("FOS_DIRECT_FACTOR");                // newton|cholesky, for callers that pass NEWTON (validated by fos_enable_direct3)
    const int64_t dense_max = getenv("FOS_DIRECT_DENSE_MAX") ? atoll(getenv("FOS_DIRECT_DENSE_MAX")) : 46000;            // largest l of the dense inverse
    const int64_t reduced_max = getenv("FOS_DIRECT_REDUCED_MAX") ? atoll(getenv("FOS_DIRECT_REDUCED_MAX")) : 46000;      // largest min(m, n) of the reduced form
    const int reduced_refine = getenv("FOS_DIRECT_REDUCED_REFINE") ? std::max(0, std::min(4, atoi(getenv("FOS_DIRECT_REDUCED_REFINE")))) : 1;   // refinement steps per projection
};

// (the set-up scratch, `Scratch`, is in fos_solver.hpp: the factored IndAffine of the Feasibility form shares it with the inversion below)
// a HIP call of a set-up: its failure is reported under the set-up's name (`what`) and the call's
static int hip_ok(const char* what, const char* call, hipError_t e) {
    if (e != hipSuccess) { set_error("%s set-up: %s -> %s", what, call, hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}

// ------------------------------------------------------------------------------------------------ the projections
// prox!(y, S1::IndAffine([Q -I], 0), x) on a block-separable operator: the exact projection in THREE KKT sweeps.
//   The projection of (u, v) onto {v = Q u} is (u^, Q u^) with (I - Q^2) u^ = u - Q v =: g   (Q' = -Q).  With h = [c; b], M = [0 A'; -A 0]:
//       I - Q^2 = [ P + h h', -M h ; -(M h)', delta ],   P = blkdiag(I + A'A, I + AA'),  delta = 1 + h'h
//               = D + W C W',   D = blkdiag(P, delta),  W = [ (h; 0), (M h; 0), e_tau ],  C = [1 0 0; 0 0 -1; 0 -1 0]
//   so by Woodbury  u^ = D^-1 g - [ph, pg, e_tau / delta] kappa,  kappa = (C^-1 + W' D^-1 W)^-1 [ph.g, pg.g, g_tau / delta],  ph = D^-1 (h; 0), pg = D^-1 (M h; 0)
//   (ph, pg, Q ph, Q pg and the 3 x 3 inverse are formed once).  D^-1 g: the x part is a product with the inverted diagonal blocks of I + A'A,
//   the y part (I + AA')^-1 g2 = g2 - A q, q = (I + A'A)^-1 A' g2.  Q D^-1 g needs A'(g2 - A q) = q (no sweep) and A x^.  Sweeps, all through the
//   dual-right-hand-side KKT apply out = (w1 - Q w2, Q w1 - w2):   (1) w = (u, v) -> g;   (2) w = (0, (0, g2, 0)) -> A' g2;   (3) w = ((q,0,0), (x^,0,0)) -> A q, A x^.
//   `from_T`: h->R already holds g in its first part (set-up: ph, pg); zero_kappa: no border correction (set-up).  Scratch: the CG vectors.
static int prox_affine_direct_block(fos_solver* h, const d2* x, d2* out, bool from_T = false, bool zero_kappa = false) {
    RoctxRange range("fos:prox_affine_direct_block (3 KKT sweeps + block-diagonal solve)");
    LaunchCtx c = h->ctx();
    d2 *T = h->R, *W2 = h->PB[0], *Rr = h->AP, *W3 = h->PB[1], *V = h->RHS;
    double* p1 = h->partials + (size_t)4 * PART_CAP;
    double* p2 = h->partials + (size_t)5 * PART_CAP;
    // Cone-sharded handles: D is block diagonal, so everything above is local to a rank -- except the scalars: the tau row of the first apply (summed over
    // the ranks by kkt_apply_full), the two dots behind kappa and the tau row of the result (c'x^ + b'y^): three exchanges per projection instead of one per
    // CG iteration.  The sums go through the handle's transport (reduce kernel with the mailbox exchange inside, or reduce kernel + all-reduce).
    const bool sh = h->sharded();
    int fr = 0;
    // (profiling: the three sweeps -- each with the deferred-row kernel and the tau-row finalize of a stand-alone apply -- are the KKT class)
    int pe = -1;
    if (!from_T) { pe = prof_begin(h, FOS_PROF_KKT, 1, h->direct_sweeps++); FOS_TRY(kkt_apply_full(h, c, x, T)); prof_end(h, pe); }      // T.x = u - Q v = g
    int po = prof_begin_other(h, 0);
    launch_blkdir_prep(c, T, h->blk_phg, W2, W3, p1);
    if (sh) { LaunchCtx c2 = c; c2.partials = p1; launch_reduce1(c2, c.vec_blocks, 3, 0); FOS_TRY(allreduce(h, 3)); fr = 1; }
    prof_end(h, po);
    pe = prof_begin(h, FOS_PROF_KKT, 1, h->direct_sweeps++);
    FOS_TRY(kkt_apply_full(h, c, W2, Rr, true, false));                // Rr.x = -Q (0, g2, 0): its x part is -A' g2 (rows of A': the deferred rows; the tau row is not needed)
    prof_end(h, pe);
    po = prof_begin_other(h, 0);
    launch_blkdir_solve(c, h->blk_n, h->blk_goff, h->blk_ioff, h->blk_idx, h->blk_ginv, Rr, T, W3, h->blk_ctx);
    prof_end(h, po);
    pe = prof_begin(h, FOS_PROF_KKT, 1, h->direct_sweeps++);
    // V.y = -A q, V.x = A x^ on the rows of A -- rows the sweep finishes itself; with dual tiles neither the rows of A' nor the tau row (c'x^: the solve kernel's records) are needed.
    // The tau row of THIS apply is needed by nobody, and on a sharded handle its reduce would overwrite the prep sums in c.reduced that blkdir_combine reads
    // (from_reduced) and add an exchange that only some ranks make: never run there.  The deferred-row kernel runs where rows of A are slot-spread.
    FOS_TRY(kkt_apply_full(h, c, W3, V, !h->blk_skip_tail, !h->blk_skip_tail && !sh));
    prof_end(h, pe);
    po = prof_begin_other(h, 0);
    launch_blkdir_combine(c, T, W3, V, h->blk_phg, h->blk_qphg, h->blk_prm, zero_kappa ? 1 : 0, out, p1, p2, fr);
    if (sh && h->tr.peer_on && c.peer) {
        // mailbox transports: the tau kernel sums the rank's record, exchanges it and forms the tau row itself (one launch instead of three)
        launch_blkdir_tau(c, T, h->blk_qphg, h->blk_prm, zero_kappa ? 1 : 0, out, p1, p2, h->blk_ctx, h->blk_n, 2);
    } else {
        if (sh) {
            double* p3 = p1;                                           // (the prep records are spent)
            launch_blkdir_tausum(c, p2, h->blk_ctx, h->blk_n, p3);
            LaunchCtx c3 = c; c3.partials = p3;
            launch_reduce1(c3, 1, 1, 0);
            FOS_TRY(allreduce(h, 1));
        }
        launch_blkdir_tau(c, T, h->blk_qphg, h->blk_prm, zero_kappa ? 1 : 0, out, p1, p2, h->blk_ctx, h->blk_n, fr);
    }
    prof_end(h, po);
    h->step.cgiter = 0;
    return check_launch("block-direct affine projection");
}

// prox!(y, S1::IndAffine([Q -I], 0), x) with the result left in h->SOL        HSDE.jl:12-15 (direct = true)
// d = D^-1 t1, D = diag(I + A'A, I + A A'), through K^-1 alone: two Q sweeps (B' t_other, then B e) around ONE pass over the stored triangle with the two
// right-hand sides (t_own, B' t_other).  dots != nullptr: the workgroups' shares of h'd and g'd (returns how many).  Scratch: PB[0], red_s, red_pq, red_yk.
static int reduced_dinv(fos_solver* h, const LaunchCtx& c, const double* t, double* d, double* dots) {
    launch_red_in1(c, h->red_swap, t, h->PB[0]);
    launch_q1(c, Q_PLAIN, h->PB[0], 0, 1.0, h->red_s);                  // (the tau row is not needed: no finalize)
    launch_red_pair(c, h->red, h->red_swap, t, h->red_s, h->red_pq);
    launch_red_symm(c, h->red, h->red_pq, h->red_yk);                   // (K^-1 t_own, e = K^-1 B' t_other)
    launch_red_in2(c, h->red_swap, h->red_yk, h->PB[0]);
    launch_q1(c, Q_PLAIN, h->PB[0], 0, 1.0, h->red_s);
    return launch_red_d(c, h->red_swap, t, h->red_s, h->red_yk, h->cb, h->red_g, d, dots);
}
// w = G^-1 t (add: w += G^-1 t) by the border formula of direct_reduced.hip
static void reduced_solve(fos_solver* h, const LaunchCtx& c, const double* t, double* w, int add) {
    const int nrec = reduced_dinv(h, c, t, h->red_d, h->red_dots);
    launch_red_w(c, t, h->red_d, h->red_p, h->red_q, h->red_dots, nrec, h->red_minv, add, w);
}
// out_plain = Q v for a plain l-vector v, tau row included (scratch: AP)
static int reduced_q_plain(fos_solver* h, const LaunchCtx& c, const double* v, double* out) {
    int fr = 0;
    launch_set_comp(c, h->AP, v, 0);
    launch_q1(c, Q_PLAIN, h->AP, 0, 1.0, out);
    FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
    launch_q1_finalize(c, Q_PLAIN, h->AP, 0, 1.0, out, fr);
    return FOS_OK;
}
// the dense and the reduced form: t = Q u - v, w = (I + Q Q')^-1 t, u+ = u + Q w; the two differ in how w is found.  The second half of the result is
// Q u+ from a sweep of its own, not v + w: the two agree only as far as the stored inverse solves its system (1e-13 .. 1e-12 relative), and the result is
// to satisfy v = Q u to the rounding of one product, as the CG path's (u, Q u) and the block form's do.
int fos::prox_affine_direct(fos_solver* h, const d2* x) {
    if (h->direct_form == DIRECT_BLOCK) return prox_affine_direct_block(h, x, h->SOL);
    const bool red = h->direct_form == DIRECT_REDUCED;
    RoctxRange range(red ? "fos:prox_affine_direct_reduced (Q sweeps + one pass over the lower triangle of K^-1)" : "fos:prox_affine_direct (3 Q sweeps + dense symmetric matvec)");
    LaunchCtx c = h->ctx();
    int fr = 0;
    double *t = h->dvec[0], *w = h->dvec[1];
    // (scratch: the CG vectors R, AP -- the input may be X, Y or W)
    launch_q1(c, Q_VFROMU, x, 0, 1.0, h->R);                           // R = (u, Q u)
    FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
    launch_q1_finalize(c, Q_VFROMU, x, 0, 1.0, h->R, fr);
    launch_direct_rhs(c, h->R, x, t);                                  // t = Q u - v
    if (!red) launch_dense_symv(c, h->Gld, h->Ginv, t, w);             // w = (I + Q Q')^-1 t: the stored inverse
    else reduced_solve(h, c, t, w, 0);                                 // ... or the border formula,
    for (int it = 0; red && it < h->red_refine; ++it) {                // refined: w += G^-1 (t - G w), G w = w - Q Q w
        FOS_TRY(reduced_q_plain(h, c, w, h->red_z));
        FOS_TRY(reduced_q_plain(h, c, h->red_z, h->red_z));
        launch_red_resid(c, t, w, h->red_z, h->red_r);
        reduced_solve(h, c, h->red_r, w, 1);
    }
    launch_set_comp(c, h->AP, w, 0);                                   // (w, 0)
    launch_q1(c, Q_VFROMU, h->AP, 0, 1.0, h->R);                       // R = (w, Q w)
    FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
    launch_q1_finalize(c, Q_VFROMU, h->AP, 0, 1.0, h->R, fr);
    launch_direct_finish(c, x, h->R, h->AP);                           // AP = (u + Q w, v + w): its first half is u+
    launch_q1(c, Q_VFROMU, h->AP, 0, 1.0, h->SOL);                     // SOL = (u+, Q u+)
    FOS_TRY(finish_reduce(h, c, c.S.npart, 1, 0, &fr, c.S.part_off));
    launch_q1_finalize(c, Q_VFROMU, h->AP, 0, 1.0, h->SOL, fr);
    h->step.cgiter = 0;
    return check_launch(red ? "reduced direct affine projection" : "direct affine projection");
}

// ---- direct = true, block-separable operators: the set-up.  Columns j, j' of A belong to one block when they share a row (connected components of the
// pattern of A'A); separable = every component has at most BLKDIR_MAX columns.  Per block G_b = I + A_b' A_b is formed on the host (row-wise outer
// products), inverted through its Cholesky factor and polished by one Newton step in extended precision; ph, pg and the 3 x 3 border system follow
// from two runs of the device path itself.  *ok = false: not separable (nothing allocated).
// v[0..2] <- their sums over the ranks of a sharded handle (set-up: through the handle's transport, one host round trip); no-op on one GPU
static int global_sum3(fos_solver* h, double* v) {
    if (!h->sharded()) return FOS_OK;
    LaunchCtx c = h->ctx();
    FOS_HIP(hipMemcpyAsync(h->partials, v, sizeof(double) * 3, hipMemcpyHostToDevice, h->stream));
    launch_reduce1(c, 1, 3, 0);
    FOS_TRY(allreduce(h, 3));
    FOS_HIP(hipMemcpyAsync(v, h->reduced, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
    return poll_state(h);
}

static int blkdir_setup(fos_solver* h, const int64_t* colptr, const int64_t* rowval, const double* nzval, bool* ok) {
    *ok = false;
    const int64_t n = h->n, m = h->m, l = h->l;
    // (sharded handles: every rank takes part in the vote below, whatever its own operator looks like)
    bool local_ok = !(n < 1 || n > (int64_t)INT32_MAX);
    if (!local_ok && !h->sharded()) return FOS_OK;
    std::vector<int32_t> parent((size_t)n);
    for (int64_t j = 0; j < n; ++j) parent[(size_t)j] = (int32_t)j;
    auto find = [&](int32_t a) { while (parent[(size_t)a] != a) { parent[(size_t)a] = parent[(size_t)parent[(size_t)a]]; a = parent[(size_t)a]; } return a; };
    bool bad_index = false;
    {
        std::vector<int32_t> first((size_t)m, -1);
        for (int64_t j = 0; j < n && !bad_index; ++j)
            for (int64_t p = colptr[j] - 1; p < colptr[j + 1] - 1; ++p) {
                const int64_t r = rowval[p] - 1;
                if (r < 0 || r >= m) { bad_index = true; local_ok = false; break; }          // (reported behind the vote: the peers of a sharded handle are waiting in it)
                if (first[(size_t)r] < 0) { first[(size_t)r] = (int32_t)j; continue; }
                const int32_t a = find((int32_t)j), b = find(first[(size_t)r]);
                if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);       // the root of a component is its smallest column
            }
    }
    std::vector<int32_t> cnt((size_t)n, 0), blkid((size_t)n, -1);
    for (int64_t j = 0; j < n; ++j) cnt[(size_t)find((int32_t)j)] += 1;
    int nblk = 0;
    size_t gtotal = 0;
    for (int64_t j = 0; j < n && local_ok; ++j)
        if (cnt[(size_t)j] > 0) {
            if (cnt[(size_t)j] > BLKDIR_MAX) { local_ok = false; break; }          // a block of I + A'A too large to invert densely per wavefront
            blkid[(size_t)j] = nblk++;
            gtotal += (size_t)cnt[(size_t)j] * (size_t)cnt[(size_t)j];
        }
    if (gtotal * sizeof(double) > ((size_t)1 << 31)) local_ok = false;
    {
        // the form is taken by ALL ranks or by none (its reductions are collective)
        double vote[3] = {local_ok ? 1.0 : 0.0, 0.0, 0.0};
        FOS_TRY(global_sum3(h, vote));
        if (bad_index) { set_error("fos_enable_direct: row index out of range"); return FOS_EINVAL; }
        if (h->sharded() ? vote[0] != (double)h->nranks : !local_ok) return FOS_OK;
    }
    std::vector<int32_t> ioff((size_t)nblk + 1, 0), idx((size_t)n);
    std::vector<int64_t> goff((size_t)nblk, 0);
    for (int64_t j = 0; j < n; ++j) if (cnt[(size_t)j] > 0) ioff[(size_t)blkid[(size_t)j] + 1] = cnt[(size_t)j];
    for (int b = 0; b < nblk; ++b) { goff[(size_t)b] = b ? goff[(size_t)b - 1] + (int64_t)(ioff[(size_t)b] - ioff[(size_t)b - 1]) * (ioff[(size_t)b] - ioff[(size_t)b - 1]) : 0; ioff[(size_t)b + 1] += ioff[(size_t)b]; }
    {
        std::vector<int32_t> fill(ioff.begin(), ioff.end() - 1);
        for (int64_t j = 0; j < n; ++j) idx[(size_t)fill[(size_t)blkid[(size_t)find((int32_t)j)]]++] = (int32_t)j;      // ascending inside a block
    }
    std::vector<double> ginv(gtotal, 0.0);
    std::vector<int32_t> rowlocal((size_t)m, -1);            // (the blocks' row sets are disjoint: one shared map, no conflicts between threads)
    std::atomic<int> next{0}, bad{0};
    auto work = [&]() {
        std::vector<int32_t> rcount, rstart, ecol;
        std::vector<double> eval, G;
        std::vector<long double> Lc, X, Y;
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= nblk) break;
            const int32_t i0 = ioff[(size_t)b], sdim = ioff[(size_t)b + 1] - i0;
            // rows of the block, in order of first appearance; entries bucketed by row
            int32_t nrows = 0;
            int64_t nent = 0;
            rcount.clear();
            for (int32_t q = 0; q < sdim; ++q) {
                const int64_t j = idx[(size_t)i0 + q];
                for (int64_t p = colptr[j] - 1; p < colptr[j + 1] - 1; ++p) {
                    const int64_t r = rowval[p] - 1;
                    if (rowlocal[(size_t)r] < 0) { rowlocal[(size_t)r] = nrows++; rcount.push_back(0); }
                    rcount[(size_t)rowlocal[(size_t)r]] += 1;
                    ++nent;
                }
            }
            rstart.assign((size_t)nrows + 1, 0);
            for (int32_t r = 0; r < nrows; ++r) rstart[(size_t)r + 1] = rstart[(size_t)r] + rcount[(size_t)r];
            ecol.resize((size_t)nent); eval.resize((size_t)nent);
            std::fill(rcount.begin(), rcount.end(), 0);
            for (int32_t q = 0; q < sdim; ++q) {
                const int64_t j = idx[(size_t)i0 + q];
                for (int64_t p = colptr[j] - 1; p < colptr[j + 1] - 1; ++p) {
                    const int32_t r = rowlocal[(size_t)(rowval[p] - 1)];
                    const size_t at = (size_t)rstart[(size_t)r] + (size_t)rcount[(size_t)r]++;
                    ecol[at] = q; eval[at] = nzval[p];
                }
            }
            G.assign((size_t)sdim * sdim, 0.0);
            for (int32_t r = 0; r < nrows; ++r)
                for (int32_t a = rstart[(size_t)r]; a < rstart[(size_t)r + 1]; ++a)
                    for (int32_t c2 = a; c2 < rstart[(size_t)r + 1]; ++c2) G[(size_t)ecol[(size_t)a] * sdim + ecol[(size_t)c2]] += eval[(size_t)a] * eval[(size_t)c2];
            for (int32_t a = 0; a < sdim; ++a) {
                G[(size_t)a * sdim + a] += 1.0;
                for (int32_t c2 = a + 1; c2 < sdim; ++c2) {          // (entries of a row arrive in ascending column order: the upper triangle was filled)
                    const double v = G[(size_t)a * sdim + c2] + G[(size_t)c2 * sdim + a];
                    G[(size_t)a * sdim + c2] = G[(size_t)c2 * sdim + a] = v;
                }
            }
            // X = G^-1 through Cholesky (extended precision: the blocks are tiny), one Newton step X <- X + X (I - G X)
            Lc.assign((size_t)sdim * sdim, 0.0L);
            bool pd = true;
            for (int32_t j = 0; j < sdim && pd; ++j) {
                long double dj = G[(size_t)j * sdim + j];
                for (int32_t k = 0; k < j; ++k) dj -= Lc[(size_t)j * sdim + k] * Lc[(size_t)j * sdim + k];
                if (!(dj > 0.0L)) { pd = false; break; }
                const long double ljj = sqrtl(dj);
                Lc[(size_t)j * sdim + j] = ljj;
                for (int32_t i = j + 1; i < sdim; ++i) {
                    long double v = G[(size_t)i * sdim + j];
                    for (int32_t k = 0; k < j; ++k) v -= Lc[(size_t)i * sdim + k] * Lc[(size_t)j * sdim + k];
                    Lc[(size_t)i * sdim + j] = v / ljj;
                }
            }
            if (!pd) { bad.store(1); continue; }
            X.assign((size_t)sdim * sdim, 0.0L);
            Y.assign((size_t)sdim, 0.0L);
            for (int32_t e = 0; e < sdim; ++e) {
                for (int32_t i = 0; i < sdim; ++i) { long double v = (i == e) ? 1.0L : 0.0L; for (int32_t k = 0; k < i; ++k) v -= Lc[(size_t)i * sdim + k] * Y[(size_t)k]; Y[(size_t)i] = v / Lc[(size_t)i * sdim + i]; }
                for (int32_t i = sdim - 1; i >= 0; --i) { long double v = Y[(size_t)i]; for (int32_t k = i + 1; k < sdim; ++k) v -= Lc[(size_t)k * sdim + i] * X[(size_t)e * sdim + k]; X[(size_t)e * sdim + i] = v / Lc[(size_t)i * sdim + i]; }
            }
            double* out = ginv.data() + goff[(size_t)b];
            for (int32_t e = 0; e < sdim; ++e)
                for (int32_t i = 0; i < sdim; ++i) out[(size_t)e * sdim + i] = (double)((X[(size_t)e * sdim + i] + X[(size_t)i * sdim + e]) / 2);      // symmetric, column-major
        }
    };
    {
        const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < hw; ++t) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
    }
    {
        double vote[3] = {bad.load() ? 1.0 : 0.0, 0.0, 0.0};       // (collective again: a rank that failed here must not leave its peers in the sums below)
        FOS_TRY(global_sum3(h, vote));
        if (bad.load()) { set_error("fos_enable_direct: I + A'A has a block that is not positive definite (non-finite entries in A?)"); return FOS_EINVAL; }
        if (vote[0] != 0.0) { set_error("fos_enable_direct: I + A'A has a block that is not positive definite on another rank"); return FOS_EINVAL; }
    }
    // ---- device data
    FOS_TRY(dev_upload(h, &h->blk_goff, goff));
    FOS_TRY(dev_upload(h, &h->blk_ioff, ioff));
    FOS_TRY(dev_upload(h, &h->blk_idx, idx));
    FOS_TRY(dev_upload(h, &h->blk_ginv, ginv));
    h->blk_n = nblk;
    FOS_TRY(dev_alloc(h, &h->blk_phg, (size_t)l));
    FOS_TRY(dev_alloc(h, &h->blk_qphg, (size_t)l));
    FOS_TRY(dev_alloc(h, &h->blk_prm, 16));
    FOS_TRY(dev_alloc(h, &h->blk_ctx, (size_t)nblk));
    // (rows of A that the sweep does not finish itself -- rows wider than one tile chunk are slot-spread too -- need the deferred-row kernel behind the third apply)
    h->blk_skip_tail = !(getenv("FOS_BLKDIR_FULL_APPLY") && atoi(getenv("FOS_BLKDIR_FULL_APPLY")) != 0);
    for (int32_t r : h->op.host.def_rows) if (r >= n) { h->blk_skip_tail = false; break; }
    FOS_HIP(hipMemset(h->blk_phg, 0, sizeof(d2) * (size_t)l));
    FOS_HIP(hipMemset(h->blk_qphg, 0, sizeof(d2) * (size_t)l));
    // ---- the border: h = [c; b], M h = [A'b; -A c], ph = D^-1 (h; 0), pg = D^-1 (M h; 0) by two runs of the device path without the border terms
    std::vector<double> cbv((size_t)(n + m));
    FOS_HIP(hipMemcpy(cbv.data(), h->cb, sizeof(double) * (size_t)(n + m), hipMemcpyDeviceToHost));
    long double hh2 = 0.0L;
    for (double v : cbv) hh2 += (long double)v * v;
    {
        double g3[3] = {(double)hh2, 0.0, 0.0};                    // |[c; b]|^2 over all ranks
        FOS_TRY(global_sum3(h, g3));
        hh2 = g3[0];
    }
    const double delta = (double)(1.0L + hh2);
    std::vector<double> prm(16, 0.0);
    prm[9] = delta;
    FOS_HIP(hipMemcpy(h->blk_prm, prm.data(), sizeof(double) * 16, hipMemcpyHostToDevice));
    std::vector<double> mh((size_t)(n + m), 0.0);
    for (int64_t j = 0; j < n; ++j) {
        long double acc = 0.0L;
        for (int64_t p = colptr[j] - 1; p < colptr[j + 1] - 1; ++p) {
            const int64_t r = rowval[p] - 1;
            acc += (long double)nzval[p] * cbv[(size_t)(n + r)];
            mh[(size_t)(n + r)] -= nzval[p] * cbv[(size_t)j];
        }
        mh[(size_t)j] = (double)acc;
    }
    std::vector<d2> tv((size_t)l), res((size_t)l), phg((size_t)l), qphg((size_t)l);
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<double>& src = pass == 0 ? cbv : mh;
        for (int64_t i = 0; i < l - 1; ++i) tv[(size_t)i] = make_double2(src[(size_t)i], 0.0);
        tv[(size_t)l - 1] = make_double2(0.0, 0.0);
        FOS_HIP(hipMemcpy(h->R, tv.data(), sizeof(d2) * (size_t)l, hipMemcpyHostToDevice));
        FOS_TRY(prox_affine_direct_block(h, nullptr, h->W, true, true));
        FOS_HIP(hipStreamSynchronize(h->stream));
        FOS_HIP(hipMemcpy(res.data(), h->W, sizeof(d2) * (size_t)l, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < l; ++i) {
            if (pass == 0) { phg[(size_t)i].x = res[(size_t)i].x; qphg[(size_t)i].x = res[(size_t)i].y; }
            else { phg[(size_t)i].y = res[(size_t)i].x; qphg[(size_t)i].y = res[(size_t)i].y; }
        }
    }
    long double hph = 0, hpg = 0, gph = 0, gpg = 0;
    for (int64_t i = 0; i < l - 1; ++i) {
        hph += (long double)cbv[(size_t)i] * phg[(size_t)i].x; hpg += (long double)cbv[(size_t)i] * phg[(size_t)i].y;
        gph += (long double)mh[(size_t)i] * phg[(size_t)i].x; gpg += (long double)mh[(size_t)i] * phg[(size_t)i].y;
    }
    {
        double g3[3] = {(double)hph, (double)hpg, (double)gph}, g1[3] = {(double)gpg, 0.0, 0.0};       // the border's dots over all ranks
        FOS_TRY(global_sum3(h, g3));
        FOS_TRY(global_sum3(h, g1));
        if (h->sharded()) { hph = g3[0]; hpg = g3[1]; gph = g3[2]; gpg = g1[0]; }
    }
    // S3 = C^-1 + W' D^-1 W,  C^-1 = [1 0 0; 0 0 -1; 0 -1 0]
    long double S3[3][3] = {{1 + hph, hpg, 0}, {gph, gpg, -1}, {0, -1, 1 / (long double)delta}}, Inv[3][3];
    const long double det = S3[0][0] * (S3[1][1] * S3[2][2] - S3[1][2] * S3[2][1]) - S3[0][1] * (S3[1][0] * S3[2][2] - S3[1][2] * S3[2][0]) +
                            S3[0][2] * (S3[1][0] * S3[2][1] - S3[1][1] * S3[2][0]);
    if (!(fabsl(det) > 0.0L) || !std::isfinite((double)det)) { set_error("fos_enable_direct: the 3 x 3 border system of the block form is singular"); return FOS_EINVAL; }
    for (int a = 0; a < 3; ++a)
        for (int bq = 0; bq < 3; ++bq) {
            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (bq + 1) % 3, b2 = (bq + 2) % 3;
            Inv[bq][a] = (S3[a1][b1] * S3[a2][b2] - S3[a1][b2] * S3[a2][b1]) / det;          // adjugate, transposed
        }
    for (int a = 0; a < 3; ++a) for (int bq = 0; bq < 3; ++bq) prm[(size_t)(3 * a + bq)] = (double)Inv[a][bq];
    FOS_HIP(hipMemcpy(h->blk_prm, prm.data(), sizeof(double) * 16, hipMemcpyHostToDevice));
    FOS_HIP(hipMemcpy(h->blk_phg, phg.data(), sizeof(d2) * (size_t)l, hipMemcpyHostToDevice));
    FOS_HIP(hipMemcpy(h->blk_qphg, qphg.data(), sizeof(d2) * (size_t)l, hipMemcpyHostToDevice));
    *ok = true;
    return FOS_OK;
}

// ---- the inverse of the dense symmetric positive definite matrix of a direct form (I + Q Q' or K), shared by the dense form, the reduced form, the test entry and
// the factored IndAffine of the Feasibility form (affine_dense.hip).  Its work-set and options, DenseWork and DenseOpts, are in fos_solver.hpp.
// the start vector of the power iteration (which = 0) and three more of its kind for the probe
void fos::direct_test_vector(int64_t k, int which, std::vector<double>& v) {
    for (int64_t i = 0; i < k; ++i) v[i] = 1.0 + 0.37 * std::sin((1.7 + 0.6 * which) * (double)i + (double)which);
}
// v <- G v through the device, *nw = |G v|_2; FOS_EINVAL when that is not a finite number: the check both factors make of the operator
static int dense_symv_norm(const DenseWork& k, const DenseOpts& o, std::vector<double>& v, double* nw) {
    const int64_t l = k.c.l;
    FOS_TRY(hip_ok(o.what, "hipMemcpyAsync", hipMemcpyAsync(k.v0, v.data(), sizeof(double) * l, hipMemcpyHostToDevice, k.c.stream)));
    launch_dense_symv(k.c, k.L, k.G, k.v0, k.v1);
    FOS_TRY(hip_ok(o.what, "hipMemcpyAsync", hipMemcpyAsync(v.data(), k.v1, sizeof(double) * l, hipMemcpyDeviceToHost, k.c.stream)));
    FOS_TRY(hip_ok(o.what, "hipStreamSynchronize", hipStreamSynchronize(k.c.stream)));
    *nw = 0.0;
    for (int64_t i = 0; i < l; ++i) *nw += v[i] * v[i];
    *nw = std::sqrt(*nw);
    if (!(*nw == *nw) || *nw > 1e300) { set_error("direct=true: the operator has non-finite entries"); return FOS_EINVAL; }
    return FOS_OK;
}
// Newton-Schulz:  X_0 = I / (1.25 lambda~),  X_{k+1} = 2 X_k - X_k (G X_k),  lambda~ a power-iteration estimate of lambda_max(G); accepted when max |G X - I| <= o.bar (1e-12)
static int dense_inverse_newton(const DenseWork& k, const DenseOpts& o, double** Xout, int* steps) {
    const LaunchCtx& c = k.c;
    const int64_t l = c.l, L = k.L;
    // ---- power iteration for lambda_max(G) (Rayleigh quotients from below; host-side norms of an l-vector)
    std::vector<double> v((size_t)l);
    direct_test_vector(l, 0, v);
    double lam = 1.0;
    for (int it = 0; it < 20; ++it) {
        double nv = 0.0, nw = 0.0;
        for (int64_t i = 0; i < l; ++i) nv += v[i] * v[i];
        nv = std::sqrt(nv);
        for (int64_t i = 0; i < l; ++i) v[i] /= nv;
        FOS_TRY(dense_symv_norm(k, o, v, &nw));
        lam = std::max(lam, nw);
    }
    // ---- Newton-Schulz
    FOS_TRY(hip_ok(o.what, "hipMemsetAsync", hipMemsetAsync(k.B1, 0, sizeof(double) * (size_t)L * (size_t)L, c.stream)));
    launch_dense_scale_identity(c, L, k.B1, 1.0 / (1.25 * lam));            // X_0
    double *X = k.B1, *Xn = k.B2;
    const int planned = (int)std::ceil(std::log2(std::max(1.0, lam))) + 7;
    double resid = 1.0;
    int it = 0;
    std::vector<double> part(256);
    for (; it < planned + o.newton_extra; ++it) {
        launch_dense_gemm(c, (int)L, 1.0, k.G, X, 0.0, nullptr, k.B0);      // Y = G X
        if (it >= planned) {                                                // converged?  max |Y - I|
            launch_dense_resid(c, L, k.B0, k.partials, 256);
            FOS_TRY(hip_ok(o.what, "hipMemcpyAsync", hipMemcpyAsync(part.data(), k.partials, sizeof(double) * 256, hipMemcpyDeviceToHost, c.stream)));
            FOS_TRY(hip_ok(o.what, "hipStreamSynchronize", hipStreamSynchronize(c.stream)));
            resid = 0.0;
            for (double r : part) resid = (r > resid || r != r) ? r : resid;
            if (resid <= o.bar) break;
        }
        launch_dense_gemm(c, (int)L, -1.0, X, k.B0, 2.0, X, Xn);            // X <- 2 X - X Y
        std::swap(X, Xn);
    }
    if (!(resid <= o.bar)) { set_error("%s: the inverse of %s did not converge (max |G X - I| = %.3e after %d steps, lambda_max ~ %.3e)", o.what, o.gname, resid, it, lam); return FOS_EINVAL; }
    *Xout = X; *steps = it;
    return FOS_OK;
}
// r = max_j |G (X v_j) - v_j|_inf / |v_j|_inf over four fixed vectors: the acceptance test of the Cholesky path (two matrix-vector products each, no l^3 product)
static int dense_inverse_probe(const DenseWork& k, const DenseOpts& o, const double* X, double* r) {
    const LaunchCtx& c = k.c;
    const int64_t l = c.l;
    std::vector<double> v((size_t)l), w((size_t)l);
    double worst = 0.0;
    for (int j = 0; j < 4; ++j) {
        direct_test_vector(l, j, v);
        FOS_TRY(hip_ok(o.what, "hipMemcpyAsync", hipMemcpyAsync(k.v0, v.data(), sizeof(double) * l, hipMemcpyHostToDevice, c.stream)));
        launch_dense_symv(c, k.L, X, k.v0, k.v1);
        launch_dense_symv(c, k.L, k.G, k.v1, k.v0);
        FOS_TRY(hip_ok(o.what, "hipMemcpyAsync", hipMemcpyAsync(w.data(), k.v0, sizeof(double) * l, hipMemcpyDeviceToHost, c.stream)));
        FOS_TRY(hip_ok(o.what, "hipStreamSynchronize", hipStreamSynchronize(c.stream)));
        double d = 0.0, nv = 0.0;
        for (int64_t i = 0; i < l; ++i) { const double e = std::fabs(w[i] - v[i]); d = (e > d || e != e) ? e : d; nv = std::max(nv, std::fabs(v[i])); }
        d /= nv;
        worst = (d > worst || d != d) ? d : worst;
    }
    *r = worst;
    return FOS_OK;
}
// factor = FOS_DIRECT_FACTOR_CHOLESKY: blocked Cholesky (dense_chol.hip), probe, at most two Newton-Schulz polish steps, then -- if the probe stays above o.bar (1e-12), or
// (pivot_fallback) a pivot failed on finite entries -- the Newton-Schulz set-up as if it had been asked for.  Without pivot_fallback a bad pivot is FOS_EINVAL.
// *Xout: the buffer (B1 or B2) that holds the accepted inverse.
int fos::dense_spd_inverse(const DenseWork& k, const DenseOpts& o, double** Xout, DenseInv* st) {
    const LaunchCtx& c = k.c;
    *st = DenseInv{};
    FOS_TRY(hip_ok(o.what, "hipStreamSynchronize", hipStreamSynchronize(c.stream)));                   // G is formed: the clock of the inversion stage starts here
    const auto t0 = std::chrono::steady_clock::now();
    auto stamp = [&]() { st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    if (o.factor == FOS_DIRECT_FACTOR_CHOLESKY) {
        std::vector<double> v((size_t)c.l);                                 // the non-finite check of the power iteration: one product with its start vector
        double nw = 0.0;
        direct_test_vector(c.l, 0, v);
        FOS_TRY(dense_symv_norm(k, o, v, &nw));
        Scratch s;
        int32_t* dinfo = s.alloc<int32_t>(1);
        FOS_TRY(hip_ok(o.what, "hipMalloc", s.err));
        int32_t info = 0;
        launch_dense_spd_inverse_chol(c, k.L, k.G, k.B2, k.B0, k.B1, dinfo);   // B0: the factor, B1: its inverse, B2: G^-1
        hipError_t e = hipMemcpyAsync(&info, dinfo, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess) { set_error("%s set-up: Cholesky factorisation -> %s", o.what, hipGetErrorString(e)); return FOS_EHIP; }
        FOS_TRY(check_launch("direct=true set-up (Cholesky factorisation)"));
        if (info != 0) {
            st->bad_col = (int64_t)info - 1;
            if (!o.pivot_fallback) {
                set_error("%s: Cholesky factorisation of %s: the pivot of column %lld is not a positive finite number (the matrix is not positive definite)", o.what, o.gname, (long long)st->bad_col);
                return FOS_EINVAL;
            }
        } else {
            double *X = k.B2, *Xn = k.B1;
            FOS_TRY(dense_inverse_probe(k, o, X, &st->probe));
            while (!(st->probe <= o.bar) && st->steps < 2) {
                launch_dense_gemm(c, (int)k.L, 1.0, k.G, X, 0.0, nullptr, k.B0);    // Y = G X
                launch_dense_gemm(c, (int)k.L, -1.0, X, k.B0, 2.0, X, Xn);          // X <- 2 X - X Y
                std::swap(X, Xn);
                st->steps += 1;
                FOS_TRY(dense_inverse_probe(k, o, X, &st->probe));
            }
            if (st->probe <= o.bar) { st->used = FOS_DIRECT_FACTOR_CHOLESKY; *Xout = X; stamp(); return FOS_OK; }
        }
        st->fell_back = true;
    }
    st->used = FOS_DIRECT_FACTOR_NEWTON;
    FOS_TRY(dense_inverse_newton(k, o, Xout, &st->steps));
    stamp();
    return FOS_OK;
}

// direct = true: build (I + Q Q')^-1 once.  A is handed over again (the handle keeps only its device format).
// G = I + Q Q' = I - Q Q is symmetric positive definite with lambda_min >= 1; its inverse is formed by the Newton-Schulz iteration
//     X_0 = I / (1.25 lambda~),   X_{k+1} = 2 X_k - X_k (G X_k),        lambda~ = a power-iteration estimate of lambda_max(G),
// whose residual I - G X_k squares every step: ceil(log2 lambda~) + 7 steps reach rounding level (verified at the end: the
// entries of G X - I).  Only matrix products are needed: the hand-written fp64 MFMA GEMM of vecops.hip.
static int enable_direct_auto(fos_handle h, const int64_t* colptr, const int64_t* rowval, const double* nzval, int factor, const DirectEnv& env) {
    if (h->row_sharded) { set_error("direct=true is not available on row-sharded handles"); return FOS_EUNSUPPORTED; }
    if (h->Ginv || h->blk_ready) { h->direct_form = h->blk_ready ? DIRECT_BLOCK : DIRECT_DENSE; return FOS_OK; }
    const int64_t l = h->l, nnz = colptr[h->n] - 1;
    if (nnz != h->nnz) { set_error("fos_enable_direct: A has %lld non-zeros, the handle was created with %lld", (long long)nnz, (long long)h->nnz); return FOS_EINVAL; }
    // (1) block-separable operators: I + A'A block diagonal with small blocks -> three sweeps per projection, any size (blkdir_setup)
    if (env.mode == "auto" || env.mode == "block") {              // (FOS_DIRECT_MODE=block|dense|cg forces one form; default: the first that applies)
        FOS_HIP(hipSetDevice(h->device));
        bool ok = false;
        FOS_TRY(blkdir_setup(h, colptr, rowval, nzval, &ok));
        if (ok) { h->blk_ready = true; h->direct_form = DIRECT_BLOCK; return FOS_OK; }
        if (env.mode == "block") { set_error("FOS_DIRECT_MODE=block: A'A has a diagonal block of more than %d columns", BLKDIR_MAX); return FOS_EUNSUPPORTED; }
    }
    // cone-sharded handles: only the block form (its three scalar exchanges per projection go through the handle's transport); collective -- every rank
    // has taken part in blkdir_setup's vote above
    if (h->sharded()) { set_error("direct=true on a sharded handle needs the block form on every rank (I + A'A block diagonal with blocks of at most %d columns)", BLKDIR_MAX); return FOS_EUNSUPPORTED; }
    // beyond what a dense l x l inverse can hold, S1 = IndAffine([Q -I], 0) and S1 = AffinePlusLinear(Q, 0, 0, 1) are still the SAME set (HSDE.jl:12-15 / :22): the
    // exact projection is what the warm-started CG converges to, so "direct" becomes CG run to its tolerance floor l eps from the first call on
    // (no 0.2^sqrt(i) schedule: affinepluslinear.jl:108-112 is what direct = true switches off) -- the reference's sparse factorisation is not rebuilt.
    if (l > env.dense_max || env.mode == "cg") { h->direct_form = DIRECT_CG; return FOS_OK; }
    FOS_HIP(hipSetDevice(h->device));
    const char* what = "direct=true";
    DenseWork k;
    k.c = h->ctx();
    k.L = (l + 63) / 64 * 64;
    const size_t L2 = (size_t)k.L * (size_t)k.L;
    Scratch s;
    int64_t* dcp = s.alloc<int64_t>((size_t)h->n + 1);
    int64_t* drv = s.alloc<int64_t>((size_t)std::max<int64_t>(nnz, 1));
    double* dnz = s.alloc<double>((size_t)std::max<int64_t>(nnz, 1));
    for (double** v : {&h->dvec[0], &h->dvec[1]}) if (!*v) FOS_TRY(dev_alloc(h, v, (size_t)k.L));
    k.v0 = h->dvec[0]; k.v1 = h->dvec[1]; k.partials = h->partials;
    k.fill(s);                                                              // B0: Q, later Y = G X;  B1, B2: X ping-pong
    if (s.err != hipSuccess) { set_error("direct=true: hipMalloc of the dense set-up buffers (4 x %zu bytes) failed: %s", L2 * 8, hipGetErrorString(s.err)); return FOS_ENOMEM; }
    FOS_TRY(dev_alloc(h, &k.G, L2));                                        // the handle's (it keeps the inverse): asked for last, so that no failure above leaves it behind
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dcp, colptr, sizeof(int64_t) * (h->n + 1), hipMemcpyHostToDevice, h->stream)));
    if (nnz) FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(drv, rowval, sizeof(int64_t) * nnz, hipMemcpyHostToDevice, h->stream)));
    if (nnz) FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dnz, nzval, sizeof(double) * nnz, hipMemcpyHostToDevice, h->stream)));
    for (double* b : {k.B0, k.B1}) FOS_TRY(hip_ok(what, "hipMemsetAsync", hipMemsetAsync(b, 0, sizeof(double) * L2, h->stream)));
    launch_dense_q_fill(k.c, dcp, drv, dnz, k.B0, k.L);                     // B0 = Q (zero padded to L x L)
    launch_dense_scale_identity(k.c, k.L, k.B1, 1.0);                       // B1 = I
    launch_dense_gemm(k.c, (int)k.L, -1.0, k.B0, k.B0, 1.0, k.B1, k.G);     // G = I - Q Q  (padding rows/columns: identity)
    double* X = nullptr;
    DenseInv inv;
    FOS_TRY(dense_spd_inverse(k, {what, "I + Q Q'", factor, true}, &X, &inv));
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(k.G, X, sizeof(double) * L2, hipMemcpyDeviceToDevice, h->stream)));     // keep the inverse in the handle's buffer
    FOS_TRY(hip_ok(what, "hipStreamSynchronize", hipStreamSynchronize(h->stream)));
    FOS_TRY(check_launch("direct=true set-up"));
    h->Ginv = k.G; h->Gld = k.L;
    h->direct_factor_req = factor; h->direct_inv = inv;
    h->direct_form = DIRECT_DENSE;
    return FOS_OK;
}

// direct = true, reduced form: K = I + B'B of order k = min(m, n) (B = A, or A' when m < n) formed densely from the sparse A, inverted by the same Newton-Schulz
// iteration as the dense form, repacked as the tiles of its lower triangle; then p = D^-1 h, q = D^-1 g and the 2 x 2 border system through the projection's own path.
static void reduced_release(fos_solver* h) {
    dev_release(h, &h->red.tiles); dev_release(h, &h->red.rowslot); dev_release(h, &h->red.colslot);
    { RedUnit* u = const_cast<RedUnit*>(h->red.units); dev_release(h, &u); h->red.units = nullptr; }
    { int32_t* u = const_cast<int32_t*>(h->red.strip_u0); dev_release(h, &u); h->red.strip_u0 = nullptr; }
    dev_release(h, &h->red_pq); dev_release(h, &h->red_yk); dev_release(h, &h->red_s); dev_release(h, &h->red_d); dev_release(h, &h->red_r); dev_release(h, &h->red_z);
    dev_release(h, &h->red_p); dev_release(h, &h->red_q); dev_release(h, &h->red_g); dev_release(h, &h->red_dots);
    h->red_ready = false;
    if (h->direct_form == DIRECT_REDUCED) h->direct_form = DIRECT_OFF;     // (a set-up that fails on a handle in the reduced form: nothing is left to run it)
}
static int reduced_setup(fos_solver* h, const int64_t* colptr, const int64_t* rowval, const double* nzval, int factor, const DirectEnv& env) {
    const char* what = "direct=true, reduced form";
    const int64_t n = h->n, m = h->m, l = h->l, nnz = colptr[n] - 1;
    if (h->row_sharded || h->sharded()) { set_error("direct=true, reduced form: not available on sharded handles"); return FOS_EUNSUPPORTED; }
    if (nnz != h->nnz) { set_error("fos_enable_direct2: A has %lld non-zeros, the handle was created with %lld", (long long)nnz, (long long)h->nnz); return FOS_EINVAL; }
    const int64_t k = std::min(m, n);
    if (k < 1) { set_error("direct=true, reduced form: min(m, n) = 0, nothing to factorise"); return FOS_EUNSUPPORTED; }
    if (k > env.reduced_max) { set_error("direct=true, reduced form: min(m, n) = %lld exceeds the largest order of the stored inverse (%lld; FOS_DIRECT_REDUCED_MAX)", (long long)k, (long long)env.reduced_max); return FOS_EUNSUPPORTED; }
    if (nnz > INT32_MAX || m > INT32_MAX || n > INT32_MAX) { set_error("direct=true, reduced form: operator too large for 32-bit indices"); return FOS_EUNSUPPORTED; }
    h->red_refine = env.reduced_refine;
    // ---- A by columns and by rows, 0-based (the rows in column order: the summation order of K's entries)
    std::vector<int32_t> cp((size_t)n + 1), ci((size_t)nnz), rp((size_t)m + 1, 0), ri((size_t)nnz);
    std::vector<double> rv((size_t)nnz);
    for (int64_t j = 0; j <= n; ++j) {
        if (colptr[j] < 1 || colptr[j] > nnz + 1 || (j > 0 && colptr[j] < colptr[j - 1])) { set_error("fos_enable_direct2: malformed colptr"); return FOS_EINVAL; }
        cp[j] = (int32_t)(colptr[j] - 1);
    }
    for (int64_t e = 0; e < nnz; ++e) {
        const int64_t r = rowval[e] - 1;
        if (r < 0 || r >= m) { set_error("fos_enable_direct2: row index out of range"); return FOS_EINVAL; }
        ci[e] = (int32_t)r;
        rp[r + 1] += 1;
    }
    for (int64_t r = 0; r < m; ++r) rp[r + 1] += rp[r];
    {
        std::vector<int32_t> fill(rp.begin(), rp.end() - 1);
        for (int64_t j = 0; j < n; ++j)
            for (int32_t e = cp[j]; e < cp[j + 1]; ++e) { const int32_t q = fill[ci[e]]++; ri[q] = (int32_t)j; rv[q] = nzval[e]; }
    }
    FOS_HIP(hipSetDevice(h->device));
    LaunchCtx c = h->ctx();
    const int swap = m < n ? 1 : 0;
    const size_t lpad = (size_t)((l + 63) / 64 * 64);
    reduced_release(h);                                                    // (from here on a failure leaves a half-built form: the caller releases it)
    DenseInv inv;
    {   // ---- K and its inverse; the scratch (the square buffers among it) goes at the end of this block: the handle keeps the packed triangle
        build_reduced_plan(k, &h->red_plan);
        const RedPlan& P = h->red_plan;
        DenseWork w;                                                       // (the launches of the inversion see the order k)
        w.c = c; w.c.l = k;
        w.L = (k + 63) / 64 * 64;
        const size_t L2 = (size_t)w.L * (size_t)w.L, ne = (size_t)std::max<int64_t>(nnz, 1);
        Scratch s;
        int32_t *dcp = s.alloc<int32_t>((size_t)n + 1), *dci = s.alloc<int32_t>(ne), *drp = s.alloc<int32_t>((size_t)m + 1), *dri = s.alloc<int32_t>(ne);
        double *dcv = s.alloc<double>(ne), *drv = s.alloc<double>(ne);
        const size_t kpad = (size_t)P.nt * RED_TR;
        RedUnit* dunits = nullptr; int32_t* dstrip = nullptr;
        FOS_TRY(dev_alloc(h, &dunits, P.units.size()));
        h->red.units = dunits;
        FOS_TRY(dev_alloc(h, &dstrip, P.strip_u0.size()));
        h->red.strip_u0 = dstrip;
        FOS_TRY(dev_alloc(h, &h->red.tiles, (size_t)P.ntiles * RED_TILE));
        FOS_TRY(dev_alloc(h, &h->red.rowslot, (size_t)P.ntiles * 64));
        FOS_TRY(dev_alloc(h, &h->red.colslot, P.units.size() * 64));
        FOS_TRY(dev_alloc(h, &h->red_pq, kpad));
        FOS_TRY(dev_alloc(h, &h->red_yk, kpad));
        for (double** v : {&h->red_s, &h->red_d, &h->red_r, &h->red_z, &h->red_p, &h->red_q, &h->red_g}) FOS_TRY(dev_alloc(h, v, lpad));
        FOS_TRY(dev_alloc(h, &h->red_dots, (size_t)2 * RED_DOT_BLOCKS));
        for (double** v : {&h->dvec[0], &h->dvec[1]}) if (!*v) FOS_TRY(dev_alloc(h, v, lpad));
        w.v0 = h->dvec[0]; w.v1 = h->dvec[1]; w.partials = h->partials;
        w.G = s.alloc<double>(L2);
        w.fill(s);
        if (s.err != hipSuccess) { set_error("direct=true, reduced form: hipMalloc of the set-up buffers (4 x %zu bytes) failed: %s", L2 * 8, hipGetErrorString(s.err)); return FOS_ENOMEM; }
        h->red.k = k; h->red.kpad = (int64_t)kpad; h->red.nt = P.nt; h->red.nunits = (int)P.units.size();
        h->red_swap = swap;
        FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dunits, P.units.data(), sizeof(RedUnit) * P.units.size(), hipMemcpyHostToDevice, h->stream)));
        FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dstrip, P.strip_u0.data(), sizeof(int32_t) * P.strip_u0.size(), hipMemcpyHostToDevice, h->stream)));
        FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dcp, cp.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, h->stream)));
        FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(drp, rp.data(), sizeof(int32_t) * (m + 1), hipMemcpyHostToDevice, h->stream)));
        if (nnz) {
            FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dci, ci.data(), sizeof(int32_t) * nnz, hipMemcpyHostToDevice, h->stream)));
            FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dcv, nzval, sizeof(double) * nnz, hipMemcpyHostToDevice, h->stream)));
            FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(dri, ri.data(), sizeof(int32_t) * nnz, hipMemcpyHostToDevice, h->stream)));
            FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(drv, rv.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, h->stream)));
        }
        FOS_TRY(hip_ok(what, "hipMemsetAsync", hipMemsetAsync(w.G, 0, sizeof(double) * L2, h->stream)));
        for (double* v : {h->red_s, h->red_d, h->red_r, h->red_z, h->red_p, h->red_q, h->red_g}) FOS_TRY(hip_ok(what, "hipMemsetAsync", hipMemsetAsync(v, 0, sizeof(double) * lpad, h->stream)));
        // K = I + B'B: B = A (its columns: A's columns, its rows: A's rows), or B = A' (the two exchanged)
        if (!swap) launch_red_form_k(c, k, w.L, dcp, dci, dcv, drp, dri, drv, w.G);
        else launch_red_form_k(c, k, w.L, drp, dri, drv, dcp, dci, dcv, w.G);
        // ---- K^-1: Newton-Schulz as in the dense form, or the blocked Cholesky factorisation
        double* X = nullptr;
        FOS_TRY(dense_spd_inverse(w, {what, "K", factor, true}, &X, &inv));
        launch_red_pack_tiles(c, h->red, w.L, X);
        FOS_TRY(hip_ok(what, "hipStreamSynchronize", hipStreamSynchronize(h->stream)));
        FOS_TRY(check_launch("direct=true set-up (reduced form)"));
    }
    // ---- g = -Q0 h, p = D^-1 h, q = D^-1 g through the projection's path; the border system on the host
    const int64_t nm = n + m;
    double* hfull = h->dvec[0];
    FOS_TRY(hip_ok(what, "hipMemsetAsync", hipMemsetAsync(hfull, 0, sizeof(double) * lpad, h->stream)));
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(hfull, h->cb, sizeof(double) * nm, hipMemcpyDeviceToDevice, h->stream)));
    launch_set_comp(c, h->AP, hfull, 0);
    launch_q1(c, Q_PLAIN, h->AP, 0, -1.0, h->red_g);                        // rows 0 .. n+m-1 of -Q (h, 0) = -Q0 h (the tau entry of red_g stays 0)
    (void)reduced_dinv(h, c, hfull, h->red_p, nullptr);
    (void)reduced_dinv(h, c, h->red_g, h->red_q, nullptr);
    std::vector<double> hh((size_t)nm), gg((size_t)nm), pp((size_t)nm), qq((size_t)nm);
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(hh.data(), h->cb, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream)));
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(gg.data(), h->red_g, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream)));
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(pp.data(), h->red_p, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream)));
    FOS_TRY(hip_ok(what, "hipMemcpyAsync", hipMemcpyAsync(qq.data(), h->red_q, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream)));
    FOS_TRY(hip_ok(what, "hipStreamSynchronize", hipStreamSynchronize(h->stream)));
    FOS_TRY(check_launch("direct=true set-up (reduced form, border)"));
    long double hp = 0, hq = 0, gp = 0, gq = 0, h2 = 0;
    for (int64_t i = 0; i < nm; ++i) { hp += (long double)hh[i] * pp[i]; hq += (long double)hh[i] * qq[i]; gp += (long double)gg[i] * pp[i]; gq += (long double)gg[i] * qq[i]; h2 += (long double)hh[i] * hh[i]; }
    const long double a00 = 1.0L + hp, a01 = hq, a10 = gp, a11 = gq - (1.0L + h2);
    const long double det = a00 * a11 - a01 * a10;
    if (!(fabsl(det) > 0.0L) || !std::isfinite((double)det)) { set_error("direct=true, reduced form: the 2 x 2 border system is singular"); return FOS_EINVAL; }
    h->red_minv[0] = (double)(a11 / det); h->red_minv[1] = (double)(-a01 / det); h->red_minv[2] = (double)(-a10 / det); h->red_minv[3] = (double)(a00 / det);
    h->direct_factor_req = factor; h->direct_inv = inv;
    h->red_ready = true;
    return FOS_OK;
}

int fos_enable_direct3(fos_handle h, const int64_t* colptr, const int64_t* rowval, const double* nzval, int32_t form, int32_t factor) {
    if (!h || !colptr || (!rowval && colptr[h->n] > 1)) { set_error("NULL argument"); return FOS_EINVAL; }
    if (form != FOS_DIRECT_FORM_AUTO && form != FOS_DIRECT_FORM_REDUCED) { set_error("fos_enable_direct3: form must be FOS_DIRECT_FORM_AUTO or FOS_DIRECT_FORM_REDUCED"); return FOS_EINVAL; }
    if (factor != FOS_DIRECT_FACTOR_NEWTON && factor != FOS_DIRECT_FACTOR_CHOLESKY) { set_error("fos_enable_direct3: factor must be FOS_DIRECT_FACTOR_NEWTON or FOS_DIRECT_FACTOR_CHOLESKY"); return FOS_EINVAL; }
    // an equilibrated handle (fos_create3) holds D A E: the caller's values are scaled the way its create path scaled them (equilibrate.cpp)
    std::vector<double> scaled;
    if (h->equilibrated() && nzval) {
        scaled.resize((size_t)(colptr[h->n] - 1));
        for (int64_t j = 0; j < h->n; ++j)
            for (int64_t k = colptr[j] - 1; k < colptr[j + 1] - 1; ++k) {
                if (rowval[k] < 1 || rowval[k] > h->m) { set_error("rowval[%lld] = %lld outside 1..%lld", (long long)k, (long long)rowval[k], (long long)h->m); return FOS_EINVAL; }
                scaled[k] = (h->eq_D[rowval[k] - 1] * nzval[k]) * h->eq_E[j];
            }
        nzval = scaled.data();
    }
    const DirectEnv env;
    if (form == FOS_DIRECT_FORM_AUTO && env.mode == "reduced") form = FOS_DIRECT_FORM_REDUCED;
    if (env.factor) {                                                      // only for callers that did not choose: the old entries pass NEWTON
        const std::string f = env.factor;
        if (f != "newton" && f != "cholesky") { set_error("FOS_DIRECT_FACTOR must be newton or cholesky, not '%s'", env.factor); return FOS_EINVAL; }
        if (factor == FOS_DIRECT_FACTOR_NEWTON && f == "cholesky") factor = FOS_DIRECT_FACTOR_CHOLESKY;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (form == FOS_DIRECT_FORM_REDUCED) {
        if (!h->red_ready || h->direct_factor_req != factor) {             // another factor: the set-up runs again
            const int rc = reduced_setup(h, colptr, rowval, nzval, factor, env);
            if (rc != FOS_OK) { if (!h->red_ready) reduced_release(h); return rc; }
            h->direct_setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        if (h->Ginv) { dev_release(h, &h->Ginv); h->Gld = 0; }            // one form's inverse at a time
        h->direct_form = DIRECT_REDUCED;
        return FOS_OK;
    }
    if (h->Ginv && h->direct_factor_req != factor) { dev_release(h, &h->Ginv); h->Gld = 0; }
    const bool had = h->Ginv || h->blk_ready;
    FOS_TRY(enable_direct_auto(h, colptr, rowval, nzval, factor, env));
    if (h->red_ready) reduced_release(h);
    if (!had) h->direct_setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return FOS_OK;
}
int fos_enable_direct2(fos_handle h, const int64_t* colptr, const int64_t* rowval, const double* nzval, int32_t form) {
    return fos_enable_direct3(h, colptr, rowval, nzval, form, FOS_DIRECT_FACTOR_NEWTON);
}
int fos_enable_direct(fos_handle h, const int64_t* colptr, const int64_t* rowval, const double* nzval) {
    return fos_enable_direct3(h, colptr, rowval, nzval, FOS_DIRECT_FORM_AUTO, FOS_DIRECT_FACTOR_NEWTON);
}

int fos_disable_direct(fos_handle h) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    h->direct_form = DIRECT_OFF;
    return FOS_OK;
}

// which form S1 = IndAffine([Q -I], 0) runs in: 0 = off (AffinePlusLinear's CG schedule), 1 = dense inverse, 2 = block form, 3 = CG at its tolerance floor, 4 = reduced form
int fos_get_direct_mode(fos_handle h, int32_t* mode) {
    if (!h || !mode) { set_error("NULL argument"); return FOS_EINVAL; }
    *mode = h->direct_form;
    return FOS_OK;
}

// form (as fos_get_direct_mode), order of the stored inverse (dense: l, reduced: min(m, n), else 0), wall seconds of the last set-up, its Newton-Schulz steps
int fos_get_direct_stats(fos_handle h, double* out4) {
    if (!h || !out4) { set_error("NULL argument"); return FOS_EINVAL; }
    const DirectForm f = h->direct_form;
    out4[0] = (double)f;
    out4[1] = f == DIRECT_REDUCED ? (double)h->red.k : (f == DIRECT_DENSE ? (double)h->l : 0.0);
    out4[2] = h->direct_setup_s;
    out4[3] = (f == DIRECT_DENSE || f == DIRECT_REDUCED) ? (double)h->direct_inv.steps : 0.0;
    return FOS_OK;
}

// the four values of fos_get_direct_stats, then: the factor that built the stored inverse (FOS_DIRECT_FACTOR_*), the seconds of the inversion stage alone, the
// last probe residual of the Cholesky path, 1.0 if that path fell back to Newton-Schulz
int fos_get_direct_stats2(fos_handle h, double* out8) {
    if (!h || !out8) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_TRY(fos_get_direct_stats(h, out8));
    const bool stored = h->direct_form == DIRECT_DENSE || h->direct_form == DIRECT_REDUCED;
    out8[4] = stored ? (double)h->direct_inv.used : 0.0;
    out8[5] = stored ? h->direct_inv.seconds : 0.0;
    out8[6] = stored ? h->direct_inv.probe : 0.0;
    out8[7] = stored && h->direct_inv.fell_back ? 1.0 : 0.0;
    return FOS_OK;
}

// test-only: X = K^-1 for a symmetric positive definite k x k host matrix (column-major) through the set-up's own path (padding, factor, probe, polish, fallback
// for a probe that stays above the bar; a bad pivot is an error here).  info4: bad-pivot column or -1, Newton-Schulz / polish steps, probe residual, fallback flag
int fos_dense_spd_inverse(int32_t device, int64_t k, const double* K, double* X, int32_t factor, double* info4) {
    if (k < 1 || k > 46000 || !K || !X || !info4) { set_error("fos_dense_spd_inverse: bad argument"); return FOS_EINVAL; }
    if (factor != FOS_DIRECT_FACTOR_NEWTON && factor != FOS_DIRECT_FACTOR_CHOLESKY) { set_error("fos_dense_spd_inverse: factor must be FOS_DIRECT_FACTOR_NEWTON or FOS_DIRECT_FACTOR_CHOLESKY"); return FOS_EINVAL; }
    info4[0] = -1.0; info4[1] = info4[2] = info4[3] = 0.0;
    FOS_HIP(hipSetDevice(device));
    DenseWork w;
    w.L = (k + 63) / 64 * 64;
    w.c.l = k;
    const int64_t L = w.L;
    const size_t L2 = (size_t)L * (size_t)L;
    std::vector<double> pad(L2, 0.0);
    for (int64_t i = 0; i < L; ++i) pad[(size_t)i + (size_t)i * L] = 1.0;
    for (int64_t j = 0; j < k; ++j) std::copy(K + j * k, K + j * k + k, pad.begin() + (size_t)j * L);
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream() { if (s) (void)hipStreamDestroy(s); }
    } stream;
    Scratch s;                                                             // (declared after the stream: freed before it is destroyed)
    hipError_t e = hipStreamCreate(&stream.s);
    if (e == hipSuccess) { w.G = s.alloc<double>(L2); w.fill(s); e = s.err; }
    if (e == hipSuccess) e = hipMemcpyAsync(w.G, pad.data(), sizeof(double) * L2, hipMemcpyHostToDevice, stream.s);
    if (e != hipSuccess) { set_error("fos_dense_spd_inverse: %s", hipGetErrorString(e)); return FOS_EHIP; }
    w.c.stream = stream.s;
    double* Xd = nullptr;
    DenseInv inv;
    int rc = dense_spd_inverse(w, {"fos_dense_spd_inverse", "K", factor, false}, &Xd, &inv);
    info4[0] = (double)inv.bad_col; info4[1] = (double)inv.steps; info4[2] = inv.probe; info4[3] = inv.fell_back ? 1.0 : 0.0;
    if (rc == FOS_OK) e = hipMemcpyAsync(pad.data(), Xd, sizeof(double) * L2, hipMemcpyDeviceToHost, stream.s);
    if (e == hipSuccess) e = hipStreamSynchronize(stream.s);               // (after a failure too: the scratch goes next)
    if (rc != FOS_OK) return rc;
    if (e != hipSuccess) { set_error("fos_dense_spd_inverse: %s", hipGetErrorString(e)); return FOS_EHIP; }
    for (int64_t j = 0; j < k; ++j) std::copy(pad.begin() + (size_t)j * L, pad.begin() + (size_t)j * L + k, X + j * k);
    return FOS_OK;
}

// test-only, host: the blocked Cholesky inverse of dense_chol.hip with the same blocking and block order on the CPU; *bad_pivot: the first bad column or -1
int fos_host_chol_inverse(int64_t k, const double* K, double* X, int64_t* bad_pivot) {
    if (k < 1 || !K || !X || !bad_pivot) { set_error("bad argument"); return FOS_EINVAL; }
    *bad_pivot = host_chol_inverse(k, K, X);
    if (*bad_pivot >= 0) { set_error("fos_host_chol_inverse: the pivot of column %lld is not a positive finite number (the matrix is not positive definite)", (long long)*bad_pivot); return FOS_EINVAL; }
    return FOS_OK;
}

// test-only, host: the reduced form's tile packing and the tile product in the kernels' summation order, for a symmetric k x k matrix X (column-major) and k
// operand pairs pq; y: k pairs; count (k x k, may be NULL): in how many tile slots each entry is stored
int fos_host_reduced_symm(int64_t k, const double* X, const double* pq, double* y, int32_t* count) {
    if (k < 1 || !X || !pq || !y) { set_error("bad argument"); return FOS_EINVAL; }
    RedPlan P;
    build_reduced_plan(k, &P);
    std::vector<double> tiles;
    if (count) std::fill(count, count + k * k, 0);
    host_reduced_pack(P, X, &tiles, count);
    const size_t kpad = (size_t)P.nt * RED_TR;
    std::vector<double> pin(2 * kpad, 0.0), out(2 * kpad, 0.0);
    std::copy(pq, pq + 2 * k, pin.begin());
    host_reduced_symm(P, tiles, pin.data(), out.data());
    std::copy(out.begin(), out.begin() + 2 * k, y);
    return FOS_OK;
}
