// A product of cones and its projection: the host table (one validator, one classifier of cone codes), the device state ConeSet and the one sequence that
// calls the cone kernels.  The HSDE handle's DualConeProduct (solver.cpp) and the Feasibility form's ConeProduct (feas.hip) are both one ConeSet.
#include <cmath>

#include "fos_solver.hpp"

namespace fos {

int psd_order(int64_t len) {
    int64_t k = (int64_t)std::llround(std::sqrt(0.25 + 2.0 * (double)len) - 0.5);
    if (k * (k + 1) / 2 != len) return -1;
    return (int)k;
}

namespace {
// the cone codes: which kernel projects a cone and, for the elementwise ones, the op of the primal and of the dual cone
enum ConeClass { CC_UNKNOWN, CC_EW, CC_SOC, CC_PSD, CC_EXP };
ConeClass cone_class(int32_t type, uint8_t* prim, uint8_t* dual) {
    switch (type) {
        case FOS_CONE_FREE: *prim = EW_COPY; *dual = EW_ZERO; return CC_EW;      // cones.jl:100
        case FOS_CONE_ZERO: *prim = EW_ZERO; *dual = EW_COPY; return CC_EW;      // cones.jl:98
        case FOS_CONE_NONNEG: *prim = *dual = EW_MAX0; return CC_EW;             // cones.jl:101
        case FOS_CONE_NONPOS: *prim = *dual = EW_MIN0; return CC_EW;             // cones.jl:102
        case FOS_CONE_SOC: case FOS_CONE_SOCROT: return CC_SOC;
        case FOS_CONE_SDP: return CC_PSD;
        case FOS_CONE_EXPPRIMAL: case FOS_CONE_EXPDUAL: return CC_EXP;
        default: return CC_UNKNOWN;
    }
}

int cone_set_fill(ConeSet* cs, const ConeTable& t, const ConeSetOptions& o) {
    std::vector<ConeDesc> psd = t.psd;
    FOS_TRY(dev_upload(cs, &cs->ew_op, t.ew));
    FOS_TRY(dev_upload(cs, &cs->soc, t.soc));
    FOS_TRY(dev_upload(cs, &cs->expc, t.expc));
    FOS_TRY(psd_sign_setup(psd, &cs->big));               // (orders > 64 leave the list: projected by matrix products)
    FOS_TRY(dev_upload(cs, &cs->psd, psd));
    cs->nsoc = (int)t.soc.size(); cs->nexp = (int)t.expc.size(); cs->npsd = (int)psd.size();
    for (const ConeDesc& cd : psd) cs->kmax = std::max(cs->kmax, cd.k);
    cs->kmin = cs->kmax;
    for (const ConeDesc& cd : psd) cs->kmin = std::min(cs->kmin, cd.k);
    const size_t sb = psd_scratch_bytes(cs->kmax, cs->npsd);
    if (sb) FOS_TRY(dev_alloc(cs, &cs->scratch, sb / sizeof(double)));
    const size_t vb = o.warm ? psd_basis_doubles(cs->kmax, cs->npsd) : 0;
    if (vb) { FOS_TRY(dev_alloc(cs, &cs->V[0], vb)); FOS_TRY(dev_alloc(cs, &cs->V[1], vb)); }
    if (vb && o.refine_records && cs->kmin == 64 && cs->kmax == 64) {
        const size_t words = (size_t)8 * cs->npsd + 16;   // code [2 npsd] + 64-bit column mask [2 npsd] + a diagnostics switch
        FOS_TRY(dev_alloc(cs, &cs->redo, words));
        FOS_HIP(hipMemset(cs->redo, 0, sizeof(int32_t) * words));
        if (o.debug_rec) { const int32_t v = 77; FOS_HIP(hipMemcpy(cs->redo + 8 * cs->npsd, &v, sizeof(v), hipMemcpyHostToDevice)); }
    }
    return FOS_OK;
}
}  // namespace

int cone_table_check(const char* which, int64_t total, int64_t nK, const int32_t* type, const int64_t* start, const int64_t* len) {
    int64_t prev_end = 0;                                   // cones.jl:66-72
    for (int64_t i = 0; i < nK; ++i) {
        if (start[i] != prev_end + 1) { set_error("%s cone %lld: range starts at %lld, expected %lld (ranges must be contiguous and ordered)", which, (long long)i + 1, (long long)start[i], (long long)prev_end + 1); return FOS_EINVAL; }
        if (len[i] < 1) { set_error("%s cone %lld: empty range", which, (long long)i + 1); return FOS_EINVAL; }
        if (len[i] > (int64_t)INT32_MAX) { set_error("%s cone %lld: %lld entries exceed the int32 cone descriptor", which, (long long)i + 1, (long long)len[i]); return FOS_EUNSUPPORTED; }
        prev_end = start[i] + len[i] - 1;
        uint8_t prim, dual;
        switch (cone_class(type[i], &prim, &dual)) {
            case CC_EW: break;
            case CC_SOC:
                if (type[i] == FOS_CONE_SOCROT && len[i] < 2) { set_error("%s cone %lld: rotated SOC needs >= 2 entries", which, (long long)i + 1); return FOS_EINVAL; }
                break;
            case CC_PSD:
                if (psd_order(len[i]) < 0) { set_error("%s cone %lld: SDP length %lld is not k(k+1)/2", which, (long long)i + 1, (long long)len[i]); return FOS_EINVAL; }
                break;
            case CC_EXP:
                if (len[i] != 3) { set_error("%s cone %lld: an exponential cone has exactly 3 entries (got %lld)", which, (long long)i + 1, (long long)len[i]); return FOS_EINVAL; }
                break;
            case CC_UNKNOWN:
                set_error("%s cone %lld: unknown cone code %d", which, (long long)i + 1, (int)type[i]);
                return FOS_EINVAL;
        }
    }
    if (prev_end != total) { set_error("%s cones cover 1..%lld, expected 1..%lld", which, (long long)prev_end, (long long)total); return FOS_EINVAL; }
    return FOS_OK;
}

void cone_table_add(ConeTable& t, int64_t offset, ConeRole role, int64_t nK, const int32_t* type, const int64_t* start, const int64_t* len) {
    // K2 cone on [x | r]: part1 primal, part2 dual.   K1 cone on [y | s]: part1 dual, part2 primal.   cones.jl:136-140
    // A ConeProduct set on [v | -]: part 1 primal (cones.jl:89-94), part 2 is not looked at
    for (int64_t i = 0; i < nK; ++i) {
        const int64_t s0 = offset + start[i] - 1;
        uint8_t prim = 0, dual = 0;
        const ConeClass cc = cone_class(type[i], &prim, &dual);
        if (cc == CC_EW) {
            const uint8_t op = role == CONE_K1 ? (uint8_t)(dual | (prim << 2)) : role == CONE_K2 ? (uint8_t)(prim | (dual << 2)) : (uint8_t)(prim | (EW_COPY << 2));
            for (int64_t k = 0; k < len[i]; ++k) t.ew[s0 + k] = op;
        } else {
            for (int64_t k = 0; k < len[i]; ++k) t.ew[s0 + k] = EW_SKIP;
            ConeDesc cd;
            cd.start = s0; cd.len = (int32_t)len[i]; cd.type = type[i];
            cd.dual_part = role == CONE_K1 ? 0 : 1;
            cd.k = cc == CC_PSD ? psd_order(len[i]) : 0;
            (cc == CC_PSD ? t.psd : cc == CC_EXP ? t.expc : t.soc).push_back(cd);
        }
    }
}

PsdTuning PsdTuning::from_env() {
    PsdTuning t;
    if (const char* e = getenv("FOS_PSD_WAVE")) t.wave = atoi(e);
    if (const char* e = getenv("FOS_PSD_REFINE")) t.refine = atoi(e);
    if (const char* e = getenv("FOS_PSD_EXTRAPOLATE")) t.extrapolate = atoi(e) != 0;
    if (const char* e = getenv("FOS_PSD_THETA")) t.theta = atof(e);
    t.narrow = getenv("FOS_PSD_NARROW") != nullptr;
    t.wide = getenv("FOS_PSD_WIDE") != nullptr;
    if (const char* e = getenv("FOS_PSD_THREADS")) t.wide_threads = atoi(e);
    return t;
}

int cone_set_build(const ConeTable& t, int64_t l, const ConeSetOptions& o, const PsdTuning& tune, ConeSet** out) {
    *out = nullptr;
    if ((int64_t)t.ew.size() != l) { set_error("cone product: the table holds %zu ops for %lld entries", t.ew.size(), (long long)l); return FOS_EINVAL; }
    ConeSet* cs = new ConeSet();
    cs->tune = tune;
    const int rc = cone_set_fill(cs, t, o);
    if (rc != FOS_OK) { cone_set_destroy(cs, nullptr); return rc; }       // (nothing of it has been launched on)
    *out = cs;
    return FOS_OK;
}

void cone_set_destroy(ConeSet* cs, hipStream_t stream) {
    if (!cs) return;
    if (stream) (void)hipStreamSynchronize(stream);
    psd_sign_destroy(cs->big);
    for (void* p : cs->owned) (void)hipFree(p);
    delete cs;
}

void cone_set_project_vector(ConeSet* cs, const LaunchCtx& c, double2* out, const double2* in, bool ew_done) {
    if (!ew_done) launch_cones_elementwise(c, out, in, cs->ew_op);
    launch_cones_soc(c, out, in, cs->soc, cs->nsoc);
    launch_cones_exp(c, out, in, cs->expc, cs->nexp);
}

int cone_set_project_psd(ConeSet* cs, const LaunchCtx& c, double2* out, const double2* in, const PsdFuse* fuse) {
    FOS_TRY(launch_cones_psd(c, *cs, out, in, fuse));
    FOS_TRY(launch_cones_psd_sign(c, cs->big, out, in));                     // cones of order > 64
    // the basis just written becomes the warm start of the next projection (a diagnostic launch truncated before the basis store leaves the previous one current)
    if (cs->npsd > 0 && cs->V[0] && (cs->phase_limit == 0 || (cs->phase_limit >= 4 && cs->phase_limit < 11))) { cs->cur = 1 - cs->cur; cs->have_prev = std::min(cs->have_prev + 1, 2); }
    if (fuse) cs->fused_steps += 1;
    return FOS_OK;
}

}  // namespace fos

using namespace fos;

extern "C" {

int fos_psd_debug(fos_handle h, int32_t collect_stats, int32_t phase_limit) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ConeSet* cs = h->cones;
    if (collect_stats && !cs->stats && cs->npsd > 0) {
        FOS_TRY(dev_alloc(cs, &cs->stats, (size_t)2 * cs->npsd));
        FOS_HIP(hipMemset(cs->stats, 0, sizeof(int) * 2 * cs->npsd));
    }
    cs->phase_limit = phase_limit;
    return FOS_OK;
}

int fos_psd_stats(fos_handle h, int32_t* sweeps, int64_t cap, int64_t* count) {
    if (!h || !count) { set_error("NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    const ConeSet* cs = h->cones;
    *count = cs->stats ? 2 * (int64_t)cs->npsd : 0;
    if (sweeps && cs->stats) {
        FOS_HIP(hipStreamSynchronize(h->stream));
        FOS_HIP(hipMemcpy(sweeps, cs->stats, sizeof(int32_t) * (size_t)std::min<int64_t>(cap, *count), hipMemcpyDeviceToHost));
    }
    return FOS_OK;
}

int fos_psd_fused_steps(fos_handle h, int64_t* count) {
    if (!h || !count) { set_error("NULL argument"); return FOS_EINVAL; }
    *count = h->cones->fused_steps;
    return FOS_OK;
}

}  // extern "C"
