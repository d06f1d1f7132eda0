// libfoship: the stacked operator S = [A'; A] of a handle (fos_solver::op).  How the product builds it, the sweep's grid, its upload and cache
// residency, the deferred rows' views, re-partitioning, the resident CG solve's plan -- and the ABI entries that are about the operator alone.
// Host C++ only: set-up ahead of every timed region.
#include "fos_solver.hpp"

namespace fos {

// ------------------------------------------------------------------------------------------------ the product's operator and its grid
// the workgroups the builder partitions for; wg_env: the value of FOS_SPMV_WG as the caller read it (nullptr: unset)
static int first_target(int cus, const char* wg_env) {
    return wg_env ? std::max(1, std::min(16384, atoi(wg_env))) : cus * 12;      // ~1.7x the resident workgroups (7/CU): measured best for the KKT sweep (dynamic balance)
}

// the builder with the product's parameters for `cus` compute units: what fos_create2 stores, and what the fos_host_resident_* entries plan for
static int build_product_operator(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, int cus, bool row_sharded,
                                  const char* wg_env, HostBlkCsr* out) {
    return build_stacked_csr(m, n, colptr, rowval, nzval, first_target(cus, wg_env), out, cus * 28, -1, row_sharded, cus * 16);
}

// the sweep's grid for a freshly built operator: returns the workgroup target (and re-partitions the row blocks where a rule says so)
static int choose_sweep_grid(HostBlkCsr& hs, int cus, const char* wg_env) {
    int target = first_target(cus, wg_env);
    if (!hs.wpanel.empty()) {
        // window panels: persistent workgroups, one per CU (96 KB of LDS each), walking the panels (measured on C5: 116 us per
        // sweep with 256 workgroups, 122 us with one workgroup per panel)
        int nwg = std::min<int>((int)hs.wpanel.size(), cus * hs.wgeom.wg_per_cu);
        if (wg_env) nwg = std::max(1, std::min<int>(atoi(wg_env), (int)hs.wpanel.size()));
        // (a multiple of 8 lets xcd_remap give every XCD a contiguous run of panels -- but never at the price of a workgroup walking two
        //  panels while others walk one: with fewer panels than slots every panel gets its own workgroup, remapped or not)
        if (nwg >= 8 && (int)hs.wpanel.size() > nwg) nwg -= nwg % 8;
        hs.nwg = nwg;
    } else if (!wg_env && hs.ntiles > hs.nblk / 2) {
        // tile-dominated operator: the blocks are (nearly) equal work units, so give every wavefront the SAME whole number of them
        // -- one, unless that needs more than 16384 workgroups (C4: 16896 tiles over 12288 wavefronts leaves 3/8 of them with
        // twice the work: 77 us; 4224 workgroups: 71 us; tall tiles: 8704 blocks over 4096 wavefronts 73 us, one each 64)
        const int64_t waves_target = (int64_t)target * SPMV_WAVES;
        int64_t per_wave = std::max<int64_t>(1, (hs.nblk + waves_target / 2) / waves_target);
        while ((hs.nblk + SPMV_WAVES * per_wave - 1) / (SPMV_WAVES * per_wave) > 16384) ++per_wave;
        target = (int)((hs.nblk + SPMV_WAVES * per_wave - 1) / (SPMV_WAVES * per_wave));
        partition_workgroups(&hs, target);
    } else if (!wg_env && hs.nblk / SPMV_WAVES < target) {
        // small operators: one row block per wavefront up to ONE resident round of workgroups (4 per CU); beyond that a
        // wavefront walks several blocks rather than queueing a second round behind the first (C3, 11 736 blocks: 2 934
        // workgroups 38.3 us per CG iteration, 1 024: 32.6, 1 152: 40.7)
        target = std::min(cus * 4, std::max(cus, (hs.nblk + SPMV_WAVES - 1) / SPMV_WAVES));
        partition_workgroups(&hs, target);
    }
    return target;
}

// ------------------------------------------------------------------------------------------------ deferred rows
// lanes per row from the average slot-list length: about a quarter of it, a power of two <= 64
static int lanes_per_row(double avg_list) {
    int lpr = 1;
    while (lpr < 64 && 4.0 * lpr < avg_list) lpr <<= 1;
    return lpr;
}

// Two views of the lists the builder makes for a row-sharded tile operator (Operator::cmp_rec); it lists the n rows of A' first (rows ascending).  Pure host code.
struct TwoViews {
    std::vector<DefRow> cmp_rec, rec;          // the compaction's records (rows of A'); the consumers' records (all deferred rows) ...
    std::vector<int32_t> idx;                  // ... and their index list
    double cmp_avg = 0.0, avg = 0.0;           // average list length of either view
};
static void two_views(const std::vector<DefRow>& def_rec, const std::vector<int32_t>& def_idx, const std::vector<int32_t>& def_ptr, size_t nn, TwoViews* out) {
    // (1) what slots_compact_kernel adds up: the records of rows 0..n-1 as built, over the sweep's slot array
    out->cmp_rec.assign(def_rec.begin(), def_rec.begin() + nn);
    const double lsum = (double)(def_ptr[nn] - def_ptr[0]);      // entries of the first n lists
    out->cmp_avg = lsum / (double)nn;
    // (2) what the consumers read, over slots_rd = [n summed rows | the sweep's slot array]: row j < n -> the single slot j;
    //     rows of A spread over column chunks -> their local lists, shifted by n
    out->rec = def_rec;
    out->idx.resize(def_idx.size() + nn);
    for (size_t k = 0; k < def_idx.size(); ++k) out->idx[k] = def_idx[k] + (int32_t)nn;
    for (size_t j = 0; j < nn; ++j) out->idx[def_idx.size() + j] = (int32_t)j;
    const int32_t own_stride = getenv("FOS_DEF_EXPLICIT") ? DEF_EXPLICIT : 0;
    for (size_t q = 0; q < out->rec.size(); ++q) {
        DefRow& d = out->rec[q];
        if (q < nn) { d.own = -1; d.count = 1; d.base = (int32_t)q; d.stride = own_stride; d.kidx = (int32_t)(def_idx.size() + q); }
        else { if (d.own >= 0) d.own += (int32_t)nn; d.base += (int32_t)nn; }
    }
    // consumers: one slot per row of A', the lists of the rows of A
    out->avg = ((double)nn + ((double)def_ptr.back() - lsum)) / (double)def_rec.size();
}

// the partial-sum records a sweep leaves for its consumers (DevBlkCsr::npart)
static void set_parts(DevBlkCsr& D) {
    D.npart = D.nwg_def > 0 ? D.nwg_def : D.nwg;
    D.part_off = D.nwg_def > 0 ? D.nwg : 0;
}

// a per-wavefront array, with room for re-partitioning up to 16384 workgroups
template <class T>
static int upload_waves(fos_solver* h, T** p, const std::vector<T>& v) {
    std::vector<T> w(std::max<size_t>(v.size(), (size_t)SPMV_WAVES * 16384 + 16), T{});
    std::copy(v.begin(), v.end(), w.begin());
    return dev_upload(h, p, w);
}

template <class T>
static int upload(fos_solver* h, const T** p, const std::vector<T>& v) {      // dev_upload into a pointer the kernels read
    T* q = nullptr;
    FOS_TRY(dev_upload(h, &q, v));
    *p = q;
    return FOS_OK;
}
template <class V> static void drop(V& v) { V().swap(v); }      // frees a host array

static void window_stats4(const HostBlkCsr& S, int64_t* stats4) {
    stats4[0] = (int64_t)S.wpanel.size(); stats4[1] = (int64_t)S.wdesc.size() / S.wgeom.waves; stats4[2] = S.wnslice; stats4[3] = (int64_t)S.wval.size();
}

// ------------------------------------------------------------------------------------------------ set-up (fos_create2)
int operator_setup(fos_solver* h, const int64_t* colptr, const int64_t* rowval, const double* nzval) {
    Operator& o = h->op; HostBlkCsr& hs = o.host; DevBlkCsr& D = o.dev;
    const char* wg_env = getenv("FOS_SPMV_WG");
    FOS_TRY(build_product_operator(h->m, h->n, colptr, rowval, nzval, h->cus, h->row_sharded, wg_env, &hs));
    o.nwg_target = choose_sweep_grid(hs, h->cus, wg_env);
    FOS_TRY(upload(h, &D.val, hs.val));
    FOS_TRY(upload(h, &D.col, hs.col));
    FOS_TRY(upload(h, &D.blk, hs.blk));
    FOS_TRY(upload(h, &D.row_rel, hs.row_rel));
    FOS_TRY(upload_waves(h, &o.wave_blk0, hs.wave_blk0));
    FOS_TRY(upload_waves(h, &o.wave_first, hs.wave_first));
    D.npanel = (int32_t)hs.wpanel.size(); D.win_tall = hs.wgeom.rows == WinTall::ROWS ? 1 : 0;
    if (D.npanel > 0) {                                 // (D starts all zero: no panel arrays otherwise)
        FOS_TRY(upload(h, &D.wpanel, hs.wpanel));
        FOS_TRY(upload(h, &D.wwave, hs.wwave));
        FOS_TRY(upload(h, &D.wdesc, hs.wdesc));
        FOS_TRY(upload(h, &D.wval, hs.wval));
        FOS_TRY(upload(h, &D.wcol, hs.wcol));
        FOS_TRY(upload(h, &D.wrow, hs.wrow));
        window_stats4(hs, o.win_stats);
        drop(hs.wval); drop(hs.wcol); drop(hs.wrow);
    }
    D.nrows = hs.nrows; D.nnz = hs.nnz; D.nnz_padded = hs.nnz_padded;
    D.dbg_flags = getenv("FOS_DBG_FLAGS") ? atoi(getenv("FOS_DBG_FLAGS")) : 0;
    // an operator whose stored form (with the dozen vectors of the solver beside it) fits the XCDs' L2s / the Infinity Cache is
    // read with ordinary loads: it then stays on-die from one sweep to the next (FOS_RESIDENT=0/1 forces)
    const double op_bytes = 8.0 * (double)hs.nnz_padded + 4.0 * (double)hs.ncol_stored + 48.0 * (double)hs.nblk;
    // (measured: C3, 12 MB, sweep 22.0 -> 17.1 us; the 64-block shard of C4, 34 MB = 4.3 MB per XCD against 4 MB of L2 each,
    //  24.5 -> 26.2 us per CG iteration: an operator that does not fit the L2s only evicts the vectors)
    //  (C3's stored form is 34.4 MB too -- what differs is the access: row blocks that GATHER (explicit column indices, latency
    //  bound) gain from a cache-resident matrix, a streamed dual-tile operator of that size does not)
    D.resident = (hs.wpanel.empty() && hs.ntiles == 0 && op_bytes <= 48e6) ? 1 : 0;
    if (const char* e = getenv("FOS_RESIDENT")) D.resident = atoi(e) != 0 ? 1 : 0;
    D.wave_blk0 = o.wave_blk0; D.wave_first = o.wave_first; D.nblk = hs.nblk; D.nwg = hs.nwg; D.nwaves = hs.nwaves;
    // dual tiles: partial-sum slots and the deferred rows' slot lists (none: the pointers stay null, nwg_def 0)
    D.ndef = (int32_t)hs.def_rows.size(); D.def_lpr = 1;
    if (D.ndef > 0) {
        int32_t* ddi;
        FOS_TRY(upload(h, &D.row_defer, hs.row_defer));
        FOS_TRY(upload(h, &D.def_rows, hs.def_rows));
        FOS_TRY(upload(h, &D.def_ptr, hs.def_ptr));
        FOS_TRY(dev_upload(h, &ddi, hs.def_idx));
        double avg_list = (double)hs.def_ptr.back() / (double)D.ndef;
        if (!(h->row_sharded && hs.ntiles > 0)) {
            FOS_TRY(upload(h, &D.def_rec, hs.def_rec));
            FOS_TRY(dev_zeros(h, &D.slots, (size_t)2 * hs.nslots));
            D.slots_rd = D.slots; D.def_idx = ddi;
            if (h->row_sharded) {                      // the all-reduced copy the slot-list sums read
                FOS_TRY(dev_zeros(h, &o.slots_rd, (size_t)2 * hs.nslots));
                D.slots_rd = o.slots_rd;
            }
        } else {
            // Two views of the builder's lists (Operator::cmp_rec).  The builder lists the n rows of A' first (rows ascending).
            const size_t nn = (size_t)h->n;
            if (hs.def_rows.size() < nn || hs.def_rows[nn - 1] != (int32_t)(nn - 1)) { set_error("internal: row-sharded tile operator without all rows of A' deferred"); return FOS_EINVAL; }
            TwoViews v;
            two_views(hs.def_rec, hs.def_idx, hs.def_ptr, nn, &v);
            FOS_TRY(dev_upload(h, &o.cmp_rec, v.cmp_rec));
            o.cmp_idx = ddi; o.cmp_lpr = lanes_per_row(v.cmp_avg);
            FOS_TRY(dev_zeros(h, &o.cmp_local, 2 * nn));
            FOS_TRY(upload(h, &D.def_rec, v.rec));
            FOS_TRY(upload(h, &D.def_idx, v.idx));
            FOS_TRY(dev_zeros(h, &o.slots_rd, 2 * (nn + (size_t)hs.nslots)));
            D.slots_rd = o.slots_rd; D.slots = o.slots_rd + 2 * nn;
            avg_list = v.avg;
        }
        // lanes per deferred row: about a quarter of the average slot-list length (C4: 33 slots -> 8 lanes, dense LP: 80 -> 16)
        int lpr = lanes_per_row(avg_list);
        if (getenv("FOS_DEF_LPR")) lpr = std::max(1, std::min(64, atoi(getenv("FOS_DEF_LPR"))));
        while (lpr & (lpr - 1)) lpr &= lpr - 1;
        D.def_lpr = lpr;
        D.nwg_def = (int32_t)std::min<int64_t>(DEF_MAX_WG, ((int64_t)D.ndef * lpr + DEF_THREADS - 1) / DEF_THREADS);
        // bit mask of the rows finished from partial slots (cg_update_kernel skips them in its streaming pass)
        std::vector<uint32_t> mask((size_t)(h->l + 31) / 32 + 1, 0u);
        for (int32_t r : hs.def_rows) mask[(size_t)r >> 5] |= 1u << (r & 31);
        FOS_TRY(dev_upload(h, &o.def_mask, mask));
        drop(hs.row_defer); drop(hs.def_idx);
    }
    set_parts(D);
    // free the big host arrays (keep block table for re-partitioning)
    drop(hs.val); drop(hs.col); drop(hs.row_rel);
    return FOS_OK;
}

// fos_set_tuning(spmv_workgroups = nwg > 0): another grid for the sweep over the stored operator
int operator_repartition(fos_solver* h, int nwg) {
    Operator& o = h->op;
    nwg = std::min(nwg, 16384);
    if (o.dev.npanel > 0) {
        // window panels: the grid is a number of persistent workgroups walking the panels
        o.dev.nwg = std::max(1, std::min<int32_t>(nwg, o.dev.npanel));
    } else {
        FOS_HIP(hipStreamSynchronize(h->stream));
        partition_workgroups(&o.host, nwg);
        FOS_HIP(hipMemcpy(o.wave_blk0, o.host.wave_blk0.data(), o.host.wave_blk0.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        FOS_HIP(hipMemcpy(o.wave_first, o.host.wave_first.data(), o.host.wave_first.size() * sizeof(BlkDesc), hipMemcpyHostToDevice));
        o.dev.nwg = o.host.nwg; o.dev.nwaves = o.host.nwaves; o.nwg_target = nwg;
    }
    set_parts(o.dev);
    return FOS_OK;
}

// ------------------------------------------------------------------------------------------------ the resident CG solve's plan
// `rl` with what a launch takes from its plan (ResLaunch's arrays and time limit are the handle's)
static ResLaunch plan_launch(const ResPlan& p, ResLaunch rl) {
    rl.G = p.G; rl.nw = p.nw; rl.ncomm = p.ncomm; rl.rpt = p.rpt; rl.tmax = p.tmax; rl.stream = p.stream; rl.nt = p.nt; rl.tiles_wg_max = p.tiles_wg_max;
    return rl;
}

// fos_resident_stats' record of a plan; ok: it can run, all: ... on every rank
static void plan_stats8(const ResPlan& p, bool ok, bool all, int64_t* stats8) {
    stats8[0] = ok ? 1 : 0; stats8[1] = p.G; stats8[2] = p.nw; stats8[3] = p.stream ? -p.nt : p.rpt; stats8[4] = p.units; stats8[5] = p.tiles_wg_max;
    stats8[6] = p.tmax; stats8[7] = all ? 1 : 0;
}

// The streamed form's fp32 walk (resident.hip, rs_lowp_decide), for the plan in force: val32 = the tile values rounded to float, at val's offsets and
// from the same allocator (+4 bytes per stored value), and delta >= |A - fl32(A)|_2 from the workgroups' Gram bounds (rs_lowp_delta_kernel; widened by
// 2^-20, far more than the rounding of the Gram sums themselves).  delta == 0: every value is a float already.  An operator whose values do not round to
// finite floats keeps the doubles.  Built when the resident solve is what the handle runs -- at fos_create where it is the default, else in front of the
// first resident solve (cg_solve): a handle that never runs it never pays the bytes.  A new plan (resident_setup) asks for it again.
int resident_lowp_ensure(fos_solver* h) {
    Operator& o = h->op;
    if (!o.res_lowp_pending) return FOS_OK;
    o.res_lowp_pending = false;
    if (!o.res_ok || !o.res_plan.stream || h->rs_lowp == 0 || h->sharded() || o.dev.nnz_padded <= 0) return FOS_OK;
    const int G = o.res_plan.G;
    if (!o.res_val32) {
        FOS_TRY(dev_alloc(h, &o.res_val32, (size_t)o.dev.nnz_padded));
        FOS_TRY(dev_zeros(h, &o.res_lowp_out, 4));
    }
    double* part = nullptr;
    FOS_TRY(dev_alloc(h, &part, (size_t)G));
    std::vector<double> hp((size_t)G);
    hipError_t e = launch_rs_lowp_setup(h->stream, o.dev.blk, o.dev.val, o.dev.nnz_padded, o.res_wg, G, o.res_val32, part);
    if (e == hipSuccess) e = hipMemcpyAsync(hp.data(), part, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    dev_release(h, &part);                                             // (on every path)
    FOS_HIP(e);
    double delta = 0.0;
    for (double v : hp) delta = (v > delta || v != v) ? v : delta;
    if (!(delta < std::numeric_limits<double>::infinity())) return FOS_OK;
    o.res.val32 = o.res_val32; o.res.lowp_out = o.res_lowp_out; o.res.lowp_delta = delta * (1.0 + 0x1p-20); o.res.lowp_mode = h->rs_lowp;
    o.res.lowp_cached = rs_lowp_cached(4 * o.dev.nnz_padded, h->rs_lowp_cache, h->rs_lowp_cache_budget) ? 1 : 0;
    return FOS_OK;
}

// FOS_CG_RESIDENT: (re)plan the resident solve for at most `gmax` workgroups -- every one of them must be on the device at once, so ranks that
// share ONE device (the tests' stand-in for a multi-GPU box) share its CUs
int resident_setup(fos_solver* h, int gmax) {
    Operator& o = h->op;
    if (const char* e = getenv("FOS_RESIDENT_GMAX")) gmax = std::max(1, std::min(gmax, atoi(e)));      // (tests: several tiles per workgroup on small problems)
    if (o.res_gmax == gmax) return FOS_OK;
    o.res_gmax = gmax; o.res_ok = false;
    ResPlan plan;
    bool ok = build_resident_plan(o.host, h->m, h->n, gmax, &plan);
    if (ok) {   // the kernel instance the plan launches must fit the device's LDS (the planner assumed 160 KiB and a static allowance)
        std::string why;
        ok = res_lds_fits(plan_launch(plan, ResLaunch{}), h->device, &why);
        if (!ok) { plan.why = why; plan.G = 0; plan.wg.clear(); }
    }
    if (!ok) { o.res_plan = plan; o.res_all = false; return FOS_OK; }
    FOS_HIP(hipStreamSynchronize(h->stream));
    if (!o.res.grec) {
        constexpr size_t b1 = sizeof(unsigned long long) * 2 * RES_GMAX * 8, b2 = sizeof(unsigned long long) * 2 * RES_GMAX * 64 * 4;
        void *q1 = nullptr, *q2 = nullptr;
        FOS_TRY(uncached_acquire(h->device, b1, true, &q1, "resident CG records"));
        h->pooled.push_back(q1);
        FOS_TRY(uncached_acquire(h->device, b2, true, &q2, "resident CG column records"));
        h->pooled.push_back(q2);
        FOS_HIP(hipMemset(q1, 0, b1));                           // sequence number 0 is never sent
        FOS_HIP(hipMemset(q2, 0, b2));
        o.res.grec = static_cast<unsigned long long*>(q1); o.res.crec = static_cast<unsigned long long*>(q2);
    }
    dev_release(h, &o.res_wg);
    FOS_TRY(dev_upload(h, &o.res_wg, plan.wg));
    o.res.wg = o.res_wg;
    o.res = plan_launch(plan, o.res);
    static const double res_wait_s = getenv("FOS_RESIDENT_WAIT_S") ? atof(getenv("FOS_RESIDENT_WAIT_S")) : 5.0;
    o.res.timeout_ticks = (int64_t)(res_wait_s * 1e8);
    o.res.val32 = nullptr; o.res.lowp_out = nullptr; o.res.lowp_delta = 0.0; o.res.lowp_eta = h->rs_lowp_eta; o.res.lowp_mode = 0;
    o.res.lowp_cached = 0;
    o.res_lowp_pending = true;                             // (resident_lowp_ensure, in front of the first resident solve on this plan)
    o.res_plan = plan; o.res_ok = true; o.res_all = !h->sharded();
    return FOS_OK;
}

// the twelve format statistics of fos_operator_stats, of the operator as built
static void format_stats12(const HostBlkCsr& S, int64_t* stats) {
    int64_t nell = 0, nlds = 0, nlong = 0, nrun = 0;
    for (const BlkDesc& d : S.blk) {
        if (d.kind() == BLK_ELL) ++nell; else if (d.kind() == BLK_LDS) ++nlds; else if (d.kind() == BLK_LONG) ++nlong;
        if (d.run()) ++nrun;
    }
    stats[0] = S.nblk; stats[1] = nell; stats[2] = nlds; stats[3] = nlong; stats[4] = nrun;
    stats[5] = S.nnz_padded; stats[6] = S.ncol_stored; stats[7] = S.nwaves;
    stats[8] = S.ntiles; stats[9] = S.nslots; stats[10] = (int64_t)S.def_rows.size(); stats[11] = S.tile_values;
}

}  // namespace fos

using namespace fos;

// ------------------------------------------------------------------------------------------------ C ABI: the operator's entries
extern "C" {

int fos_operator_stats(fos_handle h, int64_t* stats) {
    if (!h || !stats) { set_error("NULL argument"); return FOS_EINVAL; }
    format_stats12(h->op.host, stats);
    stats[7] = h->op.dev.nwaves; stats[10] = h->op.dev.ndef;      // (the grid in use, after any re-partitioning)
    return FOS_OK;
}

int fos_window_stats(fos_handle h, int64_t* stats4) {
    if (!h || !stats4) { set_error("NULL argument"); return FOS_EINVAL; }
    for (int k = 0; k < 4; ++k) stats4[k] = h->op.win_stats[k];
    return FOS_OK;
}

int fos_resident_stats(fos_handle h, int64_t* stats8) {
    if (!h || !stats8) { set_error("NULL argument"); return FOS_EINVAL; }
    const Operator& o = h->op;
    plan_stats8(o.res_plan, o.res_ok, h->sharded() ? o.res_all : o.res_ok, stats8);
    if (!o.res_ok) set_error("FOS_CG_RESIDENT: %s", o.res_plan.why.empty() ? "no plan" : o.res_plan.why.c_str());
    return FOS_OK;
}

int fos_resident_lowp_stats(fos_handle h, double* stats8) {
    if (!h || !stats8) { set_error("NULL argument"); return FOS_EINVAL; }
    const Operator& o = h->op;
    for (int k = 0; k < 8; ++k) stats8[k] = 0.0;
    if (!o.res_ok || !o.res.val32) return FOS_OK;
    double rec[4];
    FOS_HIP(hipStreamSynchronize(h->stream));
    FOS_HIP(hipMemcpy(rec, o.res.lowp_out, sizeof(rec), hipMemcpyDeviceToHost));
    stats8[0] = o.res.lowp_delta; stats8[1] = rec[0]; stats8[2] = rec[1]; stats8[3] = rec[2];
    stats8[4] = 4.0 * (double)o.dev.nnz_padded; stats8[5] = (double)o.res.lowp_mode; stats8[6] = o.res.lowp_eta;
    return FOS_OK;
}

int fos_resident_lowp_cache_stats(fos_handle h, int64_t* stats2) {
    if (!h || !stats2) { set_error("NULL argument"); return FOS_EINVAL; }
    const Operator& o = h->op;
    stats2[0] = o.res_ok && o.res.val32 && o.res.lowp_cached ? 1 : 0;
    stats2[1] = h->rs_lowp_cache_budget;
    return FOS_OK;
}

int fos_host_lowp_cached(int64_t val32_bytes, int32_t cache_switch, int64_t budget_mb, int32_t* cached, int64_t* budget_bytes) {
    if (!cached || !budget_bytes || val32_bytes < 0) { set_error("bad argument"); return FOS_EINVAL; }
    *budget_bytes = rs_lowp_cache_budget(budget_mb);
    *cached = rs_lowp_cached(val32_bytes, cache_switch != 0, *budget_bytes) ? 1 : 0;
    return FOS_OK;
}

// (the two fos_host_resident_* entries: the operator as fos_create builds it on a 256-CU device)
int fos_host_resident_cg(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, const double* c,
                         int32_t gmax, double* x, const double* rhs, double tol, int64_t max_iters, int64_t* iters, int64_t* stats8) {
    if (!colptr || m < 0 || n < 0 || gmax < 1 || (x && (!rhs || !b || !c || max_iters < 1))) { set_error("bad argument"); return FOS_EINVAL; }
    HostBlkCsr S;
    FOS_TRY(build_product_operator(m, n, colptr, rowval, nzval, 256, false, nullptr, &S));
    ResPlan P;
    const bool ok = build_resident_plan(S, m, n, gmax, &P);
    if (stats8) plan_stats8(P, ok, ok, stats8);
    if (!ok) { set_error("FOS_CG_RESIDENT: the operator does not qualify (%s)", P.why.c_str()); return x ? FOS_EUNSUPPORTED : FOS_OK; }
    if (!x) return FOS_OK;
    const int64_t l = n + m + 1;
    std::vector<double> cb((size_t)(n + m));
    for (int64_t j = 0; j < n; ++j) cb[j] = c[j];
    for (int64_t i = 0; i < m; ++i) cb[n + i] = b[i];
    std::vector<double2> xv((size_t)l), rv((size_t)l);
    for (int64_t i = 0; i < l; ++i) { xv[i] = double2{x[i], x[l + i]}; rv[i] = double2{rhs[i], rhs[l + i]}; }      // plain [part1; part2] -> interleaved
    std::vector<double2> v0(xv);
    int it = 0;
    FOS_TRY(host_resident_cg(S, P, m, n, cb.data(), xv.data(), rv.data(), v0.data(), tol, (int)std::min<int64_t>(max_iters, 1 << 30), &it));
    for (int64_t i = 0; i < l; ++i) { x[i] = xv[i].x; x[l + i] = xv[i].y; }
    if (iters) *iters = it;
    return FOS_OK;
}

int fos_host_resident_plan(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, int32_t gmax,
                           int64_t* info8, int32_t* wg7, int64_t wg_cap, int64_t* tile5, int64_t tile_cap) {
    if (!colptr || !info8 || m < 0 || n < 0 || gmax < 1) { set_error("bad argument"); return FOS_EINVAL; }
    HostBlkCsr S;
    FOS_TRY(build_product_operator(m, n, colptr, rowval, nzval, 256, false, nullptr, &S));
    ResPlan P;
    const bool ok = build_resident_plan(S, m, n, gmax, &P);
    int64_t ntiles = 0;
    for (const ResWG& w : P.wg) ntiles += w.nblk;
    info8[0] = ok ? (P.stream ? 2 : 1) : 0; info8[1] = P.G; info8[2] = P.nt; info8[3] = P.tmax; info8[4] = P.nw; info8[5] = P.rpt; info8[6] = P.ncomm;
    info8[7] = ntiles;
    if (!ok) { set_error("FOS_CG_RESIDENT: the operator does not qualify (%s)", P.why.c_str()); return FOS_OK; }
    if (wg7 && wg_cap >= P.G)
        for (int q = 0; q < P.G; ++q) {
            const ResWG& w = P.wg[q];
            const int32_t r[7] = {w.blk0, w.nblk, w.c0, w.tc, w.wg0, w.wpu, w.idx};
            memcpy(wg7 + 7 * (size_t)q, r, sizeof(r));
        }
    if (tile5 && tile_cap >= ntiles) {
        int64_t k = 0;
        for (const ResWG& w : P.wg)
            for (int ti = 0; ti < w.nblk; ++ti, ++k) {
                const BlkDesc& d = S.blk[w.blk0 + ti];
                int64_t* t = tile5 + 5 * k;
                t[0] = d.meta[0]; t[1] = d.meta[3]; t[2] = d.steps(); t[3] = d.nrows(); t[4] = d.row0;
            }
    }
    return FOS_OK;
}

// (not part of the ABI: the CPU test-suite's view of the streamed form's deal -- cnt8 = the tiles each of the eight wavefronts of a workgroup of `tiles`
//  tiles of at most `steps` steps walks, seven compute wavefronts and then the communication wavefront, consecutive tiles in wavefront order, as the
//  plan carries them to the kernel; lds_bytes (may be NULL) = the dynamic LDS of the launch)
int fos_debug_resident_deal(int32_t tiles, int32_t steps, int32_t* cnt8, int64_t* lds_bytes) {
    if (tiles < 0 || steps < 1 || steps > 64 || !cnt8) { set_error("bad argument"); return FOS_EINVAL; }
    const uint32_t deal = rs_deal(tiles, rs_ntc(steps));
    for (int w = 0, t0, cnt; w <= RS_NCOMP; ++w) { rs_split(deal, w, t0, cnt); cnt8[w] = cnt; }
    if (lds_bytes) *lds_bytes = (int64_t)res_stream_lds_bytes(tiles);
    return FOS_OK;
}

int fos_host_stacked_spmv(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                          const double* v, double* out, int32_t spmv_workgroups, int32_t resident_waves, int64_t* stats) {
    if (!colptr || !v || !out || m < 0 || n < 0) { set_error("bad argument"); return FOS_EINVAL; }
    HostBlkCsr S;
    FOS_TRY(build_stacked_csr(m, n, colptr, rowval, nzval, spmv_workgroups > 0 ? spmv_workgroups : 1024, &S, resident_waves));
    std::string why;
    int rc = host_stacked_spmv(S, v, out, &why);
    if (rc != FOS_OK) { set_error("operator format check failed: %s", why.c_str()); return rc; }
    if (stats) format_stats12(S, stats);
    return FOS_OK;
}

int fos_host_stacked_spmv_mode(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                               const double* v, double* out, int32_t window_mode, int64_t* stats16) {
    if (!colptr || !v || !out || m < 0 || n < 0) { set_error("bad argument"); return FOS_EINVAL; }
    HostBlkCsr S;
    const bool rs = getenv("FOS_HOST_SPMV_ROW_SHARDED") && atoi(getenv("FOS_HOST_SPMV_ROW_SHARDED")) != 0;      // (tests: the row-sharded builder)
    FOS_TRY(build_stacked_csr(m, n, colptr, rowval, nzval, 1024, &S, 0, window_mode, rs));
    std::string why;
    int rc = host_stacked_spmv(S, v, out, &why);
    if (rc != FOS_OK) { set_error("operator format check failed: %s", why.c_str()); return rc; }
    if (stats16) {
        for (int k = 0; k < 16; ++k) stats16[k] = 0;
        stats16[0] = S.nblk; stats16[5] = S.nnz_padded; stats16[6] = S.ncol_stored; stats16[8] = S.ntiles; stats16[9] = S.nslots;
        window_stats4(S, stats16 + 12);
    }
    return FOS_OK;
}

}  // extern "C"
