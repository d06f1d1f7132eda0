// Feasibility form on the device: find a point of S1 n S2 with the solvers' own steps.
//   reference: src/problemforms/Feasibility/Feasibility.jl (model, zeros(n) start, populate_solution),
//              src/problemforms/Feasibility/FeasibilityStatus.jl:32-72 (err = norm(prev - z) every checki-th iteration),
//              src/solvers/{gap,gapa,fista,dykstra}.jl (the steps: the same files the HSDE path follows).
// The reference takes ANY two ProximalOperators objects (host callbacks); here a set is a device object behind one interface (ProxObject, fos_internal.hpp): the
// handle owns one per slot and calls its prox.  The objects live in feas_objects.hip (dense IndAffine projector, IndBox, ConeProduct, host callback) and in the
// back-ends' own files (affine_sparse.hip, affine_dense.hip, affine_sparse_factored.hip, nspace.hip, sets.hip with its dense blocks in dense_blocks.hip).  This file keeps the algorithms, the status check,
// the wrappers and the ABI.  Every fos_feas_set_* entry does three things: validate, build, feas_install -- the object is built first, so that a refused call
// leaves the set as it was, and the install frees what the slot held.  Vectors are plain n-vectors in HBM, zero padded to L.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "dev_common.hpp"
#include "fos_internal.hpp"
#include "wrappers.hpp"

namespace fos {

constexpr int FEAS_PARTS = 256;               // partial sums per reduction (fixed: results do not depend on the device)

__global__ __launch_bounds__(FEAS_THREADS) void feas_fill_kernel(int64_t n, double* __restrict__ y, double v) { FEAS_STRIDE(i, n) y[i] = v; }
__global__ __launch_bounds__(FEAS_THREADS) void feas_copy_kernel(int64_t n, double* __restrict__ y, const double* __restrict__ x) { FEAS_STRIDE(i, n) y[i] = x[i]; }
// y = a y + (1 - a) x       gap.jl:48,58 ; gapa.jl:67,77 (a = alpha12, a device scalar) ; fista.jl:37
__global__ __launch_bounds__(FEAS_THREADS) void feas_relax_kernel(int64_t n, double* __restrict__ y, const double* __restrict__ x, double a,
                                                                  const double* __restrict__ a_dev) {
    const double aa = a_dev ? *a_dev : a;
    FEAS_STRIDE(i, n) y[i] = aa * y[i] + (1.0 - aa) * x[i];
}
// out = a + b ; p = a - b
__global__ __launch_bounds__(FEAS_THREADS) void feas_add_kernel(int64_t n, double* __restrict__ out, const double* __restrict__ a, const double* __restrict__ b) {
    FEAS_STRIDE(i, n) out[i] = a[i] + b[i];
}
__global__ __launch_bounds__(FEAS_THREADS) void feas_sub_kernel(int64_t n, double* __restrict__ out, const double* __restrict__ a, const double* __restrict__ b) {
    FEAS_STRIDE(i, n) out[i] = a[i] - b[i];
}
// y = x + coef (x - xold)      fista.jl:46
__global__ __launch_bounds__(FEAS_THREADS) void feas_extrap_kernel(int64_t n, double* __restrict__ y, const double* __restrict__ x,
                                                                   const double* __restrict__ xold, double coef) {
    FEAS_STRIDE(i, n) y[i] = x[i] + coef * (x[i] - xold[i]);
}

// out = base + a dir      linesearch.jl:58,70
__global__ __launch_bounds__(FEAS_THREADS) void feas_axpy_kernel(int64_t n, double* __restrict__ out, const double* __restrict__ base, double a,
                                                                 const double* __restrict__ dir) {
    FEAS_STRIDE(i, n) out[i] = base[i] + a * dir[i];
}

template <int NACC>
__device__ __forceinline__ void feas_block_store(const double (&acc)[NACC], double* __restrict__ partials) {
    __shared__ double sm[4 * NACC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const double v = wave_sum(acc[a]);
        if (lane == 0) sm[wave * NACC + a] = v;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        double s = 0.0;
        for (int w = 0; w < FEAS_THREADS / 64; ++w) s += sm[w * NACC + threadIdx.x];
        partials[(size_t)blockIdx.x * NACC + threadIdx.x] = s;
    }
}
// partial sums of |a - b|^2      FeasibilityStatus.jl:40
__global__ __launch_bounds__(FEAS_THREADS) void feas_normdiff_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                                     double* __restrict__ partials) {
    double acc[1] = {0.0};
    FEAS_STRIDE(i, n) { const double d = a[i] - b[i]; acc[0] += d * d; }
    feas_block_store<1>(acc, partials);
}
// alpha12 = (1 - beta) 2 / (1 + sqrt(1 - scl^2)) + 2 beta,  scl = clamp(|s| / sqrt(n1 n2), 0, 1), NaN -> 0      gapa.jl:96-101
__global__ void feas_alpha12_kernel(const double* __restrict__ partials, int nparts, double beta, double* __restrict__ a12) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, n1 = 0.0, n2 = 0.0;
    for (int b = 0; b < nparts; ++b) { s += partials[3 * b]; n1 += partials[3 * b + 1]; n2 += partials[3 * b + 2]; }
    double scl = fabs(s) / sqrt(n1 * n2);
    if (scl != scl) scl = 0.0;
    scl = fmin(fmax(scl, 0.0), 1.0);
    const double aopt = 2.0 / (1.0 + sqrt(1.0 - scl * scl));
    *a12 = (1.0 - beta) * aopt + beta * 2.0;
}
// checkstatus in ONE pass (FeasibilityStatus.jl:40,61,69): partial sums of |prev - z|^2 when this iteration checks, and prev = z -- every call
__global__ __launch_bounds__(FEAS_THREADS) void feas_check_kernel(int64_t n, double* __restrict__ prev, const double* __restrict__ z, int do_norm,
                                                                  double* __restrict__ partials) {
    double acc[1] = {0.0};
    if (do_norm) {
        FEAS_STRIDE(i, n) { const double zi = z[i], d = prev[i] - zi; acc[0] += d * d; prev[i] = zi; }
        feas_block_store<1>(acc, partials);
    } else {
        FEAS_STRIDE(i, n) prev[i] = z[i];
    }
}
// the tail of a GAP / GAPA step in ONE pass: t2 = a2 t2 + (1 - a2) t1 (gap.jl:58, gapa.jl:77; a2 = alpha12 from the device for GAPA), for GAPA the
// partial sums of normedScalar(t2, t1, t1, x) on the relaxed t2 and the OLD x (gapa.jl:96), then x = alpha t2 + (1 - alpha) x (gap.jl:78, gapa.jl:103)
template <bool GAPA>
__global__ __launch_bounds__(FEAS_THREADS) void feas_gap_tail_kernel(int64_t n, double* __restrict__ x, double* __restrict__ t2, const double* __restrict__ t1,
                                                                     double a2, const double* __restrict__ a_dev, double alpha, double* __restrict__ partials) {
    const double aa = a_dev ? *a_dev : a2;
    double acc[3] = {0.0, 0.0, 0.0};
    FEAS_STRIDE(i, n) {
        const double t1i = t1[i], xi = x[i];
        const double t2i = aa * t2[i] + (1.0 - aa) * t1i;
        t2[i] = t2i;
        if constexpr (GAPA) {
            const double d1 = t2i - t1i, d2 = t1i - xi;
            acc[0] += d1 * d2; acc[1] += d1 * d1; acc[2] += d2 * d2;
        }
        x[i] = alpha * t2i + (1.0 - alpha) * xi;
    }
    if constexpr (GAPA) feas_block_store<3>(acc, partials);
}
// x = alpha t2 + (1 - alpha) x      gap.jl:78, gapa.jl:103
__global__ __launch_bounds__(FEAS_THREADS) void feas_combine_kernel(int64_t n, double* __restrict__ x, const double* __restrict__ t2, double alpha) {
    FEAS_STRIDE(i, n) x[i] = alpha * t2[i] + (1.0 - alpha) * x[i];
}
}  // namespace fos

using namespace fos;

struct fos_feas : DevOwned {                      // (owns the vectors below; the sets own theirs)
    fos_feas() { what = "feasibility form"; }
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0, L = 0;
    std::unique_ptr<ProxObject> S[2];      // the two sets: nullptr until defined
    int alg = FOS_ALG_GAP;
    double alpha = 0.8, alpha1 = 1.8, alpha2 = 1.8, beta = 0.0;
    double fista_t = 1.0;
    // vectors of length L (zero padded)
    double *x = nullptr, *t1 = nullptr, *t2 = nullptr, *y = nullptr, *xold = nullptr, *p = nullptr, *q = nullptr, *prev = nullptr, *tmp = nullptr;
    int cus = 256;
    double* partials = nullptr;     // [3 x FEAS_PARTS]
    double* a12 = nullptr;          // device scalar alpha12 (GAPA)
    int grid = 1;
    int status = FOS_STATUS_CONTINUE;
    int checked = 0;
    double err = NAN;
    Wrappers wr;                    // LineSearchWrapper, GAPP (an algorithm of its own here: FOS_ALG_GAPP), LongstepWrapper (wrappers.hpp; the planes see the vectors as L/2 double2)
};

namespace {

int feas_check_launch(const char* where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: a kernel launch failed: %s", where, hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}

#define FEAS_K(kernel, ...) hipLaunchKernelGGL(kernel, dim3(h->grid), dim3(FEAS_THREADS), 0, h->stream, __VA_ARGS__)

LaunchCtx feas_ctx(const fos_feas* h, int64_t l) {
    LaunchCtx c{};
    c.stream = h->stream;
    c.l = l;
    return c;
}

// the LongstepWrapper's kernels see the zero-padded vectors of L doubles as L / 2 double2
LaunchCtx feas_long_ctx(const fos_feas* h) {
    LaunchCtx c = feas_ctx(h, h->L / 2);
    c.vec_blocks = h->grid;
    return c;
}
inline void feas_long_save(fos_feas* h, int which, const double* y, const double* x) {
    if (h->wr.lp.now) long_save_plane(feas_long_ctx(h), h->wr.lp, which, reinterpret_cast<const double2*>(y), reinterpret_cast<const double2*>(x));
}

// prox!(y, S, x): the projection onto set `which`; y must not alias x
int feas_prox(fos_feas* h, int which, double* y, const double* x) {
    if (!h->S[which]) { set_error("feasibility form: set %d has not been defined", which + 1); return FOS_EINVAL; }
    return h->S[which]->prox(h->stream, y, x);
}

FeasEnv feas_env(const fos_feas* h) { return FeasEnv{h->stream, h->n, h->L, h->grid, h->cus, h->partials}; }

// the one way a set enters a slot (which = 1 | 2): `fresh` was built first, so a refused call never gets here and leaves the set as it was; no prox of the object
// being replaced runs any more once the stream is idle, and what it owned goes with it, whatever its kind
int feas_install(fos_feas* h, int32_t which, ProxObject* fresh) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { delete fresh; set_error("feasibility form: hipStreamSynchronize -> %s", hipGetErrorString(e)); return FOS_EHIP; }
    h->S[which - 1].reset(fresh);
    return FOS_OK;
}
// the object of slot `which` when it is of `kind`, for the accessors; otherwise FOS_EINVAL with "<fn>: set <which> <is_not>"
int feas_object(fos_feas* h, int32_t which, const void* out, int kind, const char* fn, const char* is_not, const ProxObject** obj) {
    if (!h || !out || which < 1 || which > 2 || !h->S[which - 1] || h->S[which - 1]->kind != kind) { set_error("%s: set %d %s", fn, (int)which, is_not); return FOS_EINVAL; }
    *obj = h->S[which - 1].get();
    return FOS_OK;
}

// checkstatus(stat, z) at iteration i      FeasibilityStatus.jl:32-72
int feas_check(fos_feas* h, const double* z, int64_t i, int64_t checki, double eps, bool override_) {
    if (override_ || (checki > 0 && i % checki == 0)) {
        FEAS_K(feas_check_kernel, h->n, h->prev, z, 1, h->partials);                   // |prev - z|^2 and prev = z in one pass
        FOS_TRY(norm_of_partials(h->partials, (size_t)h->grid, h->stream, &h->err));
        h->status = (h->err <= eps) ? FOS_STATUS_OPTIMAL : FOS_STATUS_CONTINUE;       // :57 (NaN <= eps is false)
        h->checked = 1;
    } else {
        h->checked = 0;
        FEAS_K(feas_check_kernel, h->n, h->prev, z, 0, h->partials);                   // :61,69: prev = z at every call
    }
    return FOS_OK;
}

// the searches' view of the handle (wrappers.hpp).  Scratch the algorithms with a search leave free: the line search's tmp1 = y, tmp2 = t1, res = xold, tmp3 = p;
// GAPP's tmp1 = t1, tmp2 = t2, res = xold (prox!(res, S1, .) writes it directly), tmp3 = p, tmp4 = q
struct FeasSearch {
    fos_feas* h;
    double *x, *tmp1, *tmp2, *res, *tmp3, *tmp4; const double *res_from, *a12;          // (a12: GAPA relaxes with the device scalar alpha12)
    explicit FeasSearch(fos_feas* h_) : h(h_), x(h_->x), tmp1(h_->alg == FOS_ALG_GAPP ? h_->t1 : h_->y), tmp2(h_->t2), res(h_->xold), tmp3(h_->p), tmp4(h_->q), res_from(h_->xold),
                                        a12(h_->alg == FOS_ALG_GAPA ? h_->a12 : nullptr) {}
    int relaxed_s1(const double* in) { FOS_TRY(feas_prox(h, 0, h->t1, in)); FEAS_K(feas_relax_kernel, h->n, h->t1, in, h->alpha1, a12); return FOS_OK; }
    int relaxed_s2(double* out) { FOS_TRY(feas_prox(h, 1, out, h->t1)); FEAS_K(feas_relax_kernel, h->n, out, (const double*)h->t1, h->alpha2, a12); return FOS_OK; }
    int prox_s2(double* out, const double* in) { return feas_prox(h, 1, out, in); }
    void axpy(double* out, const double* base, double a, const double* dir) { FEAS_K(feas_axpy_kernel, h->n, out, base, a, dir); }
    void sub(double* out, const double* a, const double* b) { FEAS_K(feas_sub_kernel, h->n, out, a, b); }
    int normdiff(const double* a, const double* b, double* out) { FEAS_K(feas_normdiff_kernel, h->n, a, b, h->partials); return norm_of_partials(h->partials, (size_t)h->grid, h->stream, out); }
};

// LineSearchWrapper(GAP / GAPA), one search iteration      wrappers/linesearch.jl:36-75
int feas_linesearch_iteration(fos_feas* h, int64_t i, int64_t checki, double eps) {
    FeasSearch f(h);
    FEAS_K(feas_copy_kernel, h->n, h->y, (const double*)h->x);                         // tmp1 .= x                 :41
    FOS_TRY(f.relaxed_s1(h->x));                                                       // S1!(tmp2, x)              :45
    FOS_TRY(feas_prox(h, 1, h->x, h->t1));                                             // S2!(x, tmp2, status)      :46
    FOS_TRY(feas_check(h, h->x, i, checki, eps, false));
    FEAS_K(feas_relax_kernel, h->n, h->x, (const double*)h->t1, h->alpha2, f.a12);
    return linesearch_search(f, h->wr.ls_log, i);
}

// GAPP, one iteration      solvers/gapproj.jl:29-72
int feas_gapp_iteration(fos_feas* h, int64_t i, int64_t checki, double eps) {
    const int64_t n = h->n;
    FOS_TRY(feas_prox(h, 0, h->t1, h->x));                                             // prox!(tmp1, S1, x)        :33
    if (i % h->wr.gapp_iproj != 0) {                                                   // the GAP step              :63-70
        FEAS_K(feas_relax_kernel, n, h->t1, (const double*)h->x, h->alpha1, (const double*)nullptr);
        FOS_TRY(feas_prox(h, 1, h->t2, h->t1));
        FOS_TRY(feas_check(h, h->t2, i, checki, eps, false));
        FEAS_K(feas_relax_kernel, n, h->t2, (const double*)h->t1, h->alpha2, (const double*)nullptr);
        FEAS_K(feas_combine_kernel, n, h->x, (const double*)h->t2, h->alpha);
        return FOS_OK;
    }
    FeasSearch f(h);
    FOS_TRY(feas_prox(h, 1, h->t2, h->t1));                                            // prox!(tmp2, S2, tmp1)     :39
    FOS_TRY(feas_prox(h, 0, h->xold, h->t2));                                          // prox!(res, S1, tmp2)      :40
    FOS_TRY(gapp_search(f, h->wr.gapp_log, i));
    FOS_TRY(feas_check(h, h->t2, i, checki, eps, false));                              // :60
    FEAS_K(feas_relax_kernel, n, h->t2, (const double*)h->p, h->alpha2, (const double*)nullptr);   // :61
    FEAS_K(feas_copy_kernel, n, h->x, (const double*)h->t2);                           // x .= tmp2                 :62
    return FOS_OK;
}

int feas_step_once(fos_feas* h, int64_t i, int64_t checki, double eps) {
    const int64_t n = h->n;
    if (h->alg == FOS_ALG_GAPP) return feas_gapp_iteration(h, i, checki, eps);
    if (h->wr.ls_interval > 0 && i % h->wr.ls_interval == 0) return feas_linesearch_iteration(h, i, checki, eps);      // linesearch.jl:39
    long_window(h->wr.lp, i);                                                          // longstep.jl:44-49
    switch (h->alg) {
    case FOS_ALG_GAP:
    case FOS_ALG_GAPA: {
        const bool ad = h->alg == FOS_ALG_GAPA;
        const double* a12 = ad ? h->a12 : nullptr;
        FOS_TRY(feas_prox(h, 0, h->t1, h->x));                                         // S1!  gap.jl:42-51, gapa.jl:61-70
        feas_long_save(h, 0, h->t1, h->x);                                             // addprojeq(longstep, y, x)
        FEAS_K(feas_relax_kernel, n, h->t1, (const double*)h->x, h->alpha1, a12);
        FOS_TRY(feas_prox(h, 1, h->t2, h->t1));                                        // S2!  gap.jl:53-59, gapa.jl:72-78
        FOS_TRY(feas_check(h, h->t2, i, checki, eps, false));
        feas_long_save(h, 1, h->t2, h->t1);                                            // addprojineq(longstep, y, x)
        if (ad) {                                                                      // relaxation, the sums of gapa.jl:96 (relaxed t1, t2 and the old x) and x's update: one pass
            FEAS_K(feas_gap_tail_kernel<true>, n, h->x, h->t2, (const double*)h->t1, h->alpha2, a12, h->alpha, h->partials);
            hipLaunchKernelGGL(feas_alpha12_kernel, dim3(1), dim3(64), 0, h->stream, (const double*)h->partials, h->grid, h->beta, h->a12);    // gapa.jl:96-101
        } else {
            FEAS_K(feas_gap_tail_kernel<false>, n, h->x, h->t2, (const double*)h->t1, h->alpha2, a12, h->alpha, h->partials);                  // gap.jl:58,78
        }
        break;
    }
    case FOS_ALG_FISTA: {                                                              // fista.jl:28-48
        if (i == 1) FEAS_K(feas_copy_kernel, n, h->y, (const double*)h->x);
        FOS_TRY(feas_prox(h, 0, h->t1, h->y));
        feas_long_save(h, 0, h->t1, h->y);                                             // addprojeq(longstep, tmp1, y)      fista.jl:36
        FEAS_K(feas_relax_kernel, n, h->t1, (const double*)h->y, h->alpha, (const double*)nullptr);
        FEAS_K(feas_copy_kernel, n, h->xold, (const double*)h->x);
        FOS_TRY(feas_prox(h, 1, h->x, h->t1));
        FOS_TRY(feas_check(h, h->x, i, checki, eps, false));
        feas_long_save(h, 1, h->x, h->t1);                                             // addprojineq(longstep, x, tmp1)    fista.jl:42
        const double told = h->fista_t;
        h->fista_t = (1.0 + std::sqrt(1.0 + 4.0 * told * told)) / 2.0;
        FEAS_K(feas_extrap_kernel, n, h->y, (const double*)h->x, (const double*)h->xold, (told - 1.0) / h->fista_t);
        break;
    }
    case FOS_ALG_DYKSTRA: {                                                            // dykstra.jl:25-36
        FEAS_K(feas_add_kernel, n, h->tmp, (const double*)h->x, (const double*)h->p);
        FOS_TRY(feas_prox(h, 0, h->y, h->tmp));
        feas_long_save(h, 0, h->y, h->tmp);                                            // addprojeq(longstep, y, x .+ p)    dykstra.jl:30
        FEAS_K(feas_sub_kernel, n, h->p, (const double*)h->tmp, (const double*)h->y);
        FEAS_K(feas_add_kernel, n, h->tmp, (const double*)h->y, (const double*)h->q);
        FOS_TRY(feas_prox(h, 1, h->x, h->tmp));
        FOS_TRY(feas_check(h, h->x, i, checki, eps, false));
        feas_long_save(h, 1, h->x, h->tmp);                                            // addprojineq(longstep, x, y .+ q)  dykstra.jl:34
        FEAS_K(feas_sub_kernel, n, h->q, (const double*)h->tmp, (const double*)h->x);
        break;
    }
    default: set_error("feasibility form: unknown algorithm %d", h->alg); return FOS_EINVAL;
    }
    return long_window_close(feas_long_ctx(h), h->wr.lp, reinterpret_cast<double2*>(h->x), i);      // longstep.jl:53-58: projectonnormals!, x .= tmp
}

}  // namespace

extern "C" {

int fos_feas_create(int64_t n, int32_t device, fos_feas_handle* out) {
    if (!out || n < 1) { set_error("fos_feas_create: n >= 1 and a handle pointer are required"); return FOS_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device is visible: the HIP path has no CPU fallback"); return FOS_ENODEVICE; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (0..%d)", device, ndev - 1); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(device));
    fos_feas* h = new fos_feas();
    h->device = device; h->n = n; h->L = (n + 63) / 64 * 64;
    h->grid = (int)std::min<int64_t>(FEAS_PARTS, (n + FEAS_THREADS - 1) / FEAS_THREADS);
    if (hipStreamCreate(&h->stream) != hipSuccess) { delete h; set_error("hipStreamCreate failed"); return FOS_EHIP; }
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->cus = prop.multiProcessorCount; }
    int rc = FOS_OK;
    double** vecs[] = {&h->x, &h->t1, &h->t2, &h->y, &h->xold, &h->p, &h->q, &h->prev, &h->tmp};
    for (double** v : vecs) { rc = h->zeros(v, (size_t)h->L, h->stream); if (rc != FOS_OK) break; }
    if (rc == FOS_OK) rc = h->zeros(&h->partials, 3 * (size_t)FEAS_PARTS, h->stream);
    if (rc == FOS_OK) rc = h->zeros(&h->a12, 8, h->stream);
    if (rc != FOS_OK) { fos_feas_destroy(h); return rc; }
    *out = h;
    return fos_feas_set_iterate(h, nullptr);
}

int fos_feas_destroy(fos_feas_handle h) {
    if (!h) return FOS_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& s : h->S) s.reset();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return FOS_OK;
}

// IndAffine(A, b) as the dense n x n projector (feas_objects.hip): A is m x n, ROW-major (C order), full row rank
int fos_feas_set_affine(fos_feas_handle h, int32_t which, int64_t m, const double* A, const double* b) {
    if (!h || !A || !b || which < 1 || which > 2 || m < 1 || m > h->n) { set_error("fos_feas_set_affine: bad argument (1 <= m <= n, which = 1 | 2)"); return FOS_EINVAL; }
    if (h->n > 46000) { set_error("IndAffine: the dense projector holds %lld x %lld doubles: supported up to n = 46000", (long long)h->n, (long long)h->n); return FOS_EUNSUPPORTED; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(dense_projector_setup(feas_env(h), m, A, b, &s));
    return feas_install(h, which, s);
}

// IndAffine(A, b), A a sparse m x n matrix (CSC, 1-based: Julia's SparseMatrixCSC{Float64,Int64}), full row rank: nothing dense is formed, any n
int fos_feas_set_affine_sparse(fos_feas_handle h, int32_t which, int64_t m, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b) {
    if (!h || which < 1 || which > 2 || m < 1 || m > h->n) { set_error("fos_feas_set_affine_sparse: bad argument (1 <= m <= n, which = 1 | 2)"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(sparse_affine_setup(m, h->n, colptr, rowval, nzval, b, h->cus, &s));
    return feas_install(h, which, s);
}

// out8: projections so far, CG iterations so far, CG iterations / restarts of the last projection, its |A y - b| and the rounding level | |A||y| + |b| |
// (rows scaled to unit norm), stored entries, lanes per row of A x 1000 + of A'
int fos_feas_affine_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_AFFINE_SPARSE, "fos_feas_affine_stats", "is not a sparse IndAffine", &s));
    sparse_affine_stats(s, out8);
    return FOS_OK;
}

// IndAffine(A, b), A dense m x n ROW-major, factored form (affine_dense.hip)
int fos_feas_set_affine_factored(fos_feas_handle h, int32_t which, int64_t m, const double* A, const double* b, int32_t factor, int32_t refine) {
    if (!h || which < 1 || which > 2 || m < 1 || m > h->n) { set_error("fos_feas_set_affine_factored: bad argument (1 <= m <= n, which = 1 | 2)"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(dense_affine_setup(m, h->n, A, b, 0.0, factor, refine, h->cus, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_affine_factored_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_AFFINE_FACTORED, "fos_feas_affine_factored_stats", "is not a factored IndAffine", &s));
    dense_affine_stats(s, out8);
    return FOS_OK;
}
int fos_feas_affine_factored_plan(fos_feas_handle h, int32_t which, int64_t* out6) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out6, FEAS_AFFINE_FACTORED, "fos_feas_affine_factored_plan", "is not a factored IndAffine", &s));
    dense_affine_plan(s, out6);
    return FOS_OK;
}
// test-only, host: the factored form's scaling, inverse and two passes in the kernels' order (affine_dense.hip)
int fos_host_affine_factored(int64_t m, int64_t n, const double* A, const double* b, int32_t refine, const double* x, double* y) {
    return host_affine_factored(m, n, A, b, 0.0, refine, x, y);
}
// LeastSquares(A, b, lambda), A dense m x n ROW-major: the factored form with the diagonal of A A' shifted by 1 / lambda (affine_dense.hip); the same object
// kind, so the stats and the plan of the factored form describe it
int fos_feas_set_least_squares(fos_feas_handle h, int32_t which, int64_t m, const double* A, const double* b, double lambda, int32_t factor) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_least_squares: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    if (!(lambda > 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(dense_affine_setup(m, h->n, A, b, lambda, factor, 0, h->cus, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_host_least_squares(int64_t m, int64_t n, const double* A, const double* b, double lambda, const double* x, double* y) {
    if (!(lambda > 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    return host_affine_factored(m, n, A, b, lambda, 0, x, y);
}

// IndAffine(A, b), A sparse m x n (CSC, 1-based), factored form (affine_sparse_factored.hip)
int fos_feas_set_affine_sparse_factored(fos_feas_handle h, int32_t which, int64_t m, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b,
                                        int32_t factor, int32_t refine) {
    if (!h || which < 1 || which > 2 || m < 1) { set_error("fos_feas_set_affine_sparse_factored: bad argument (m >= 1, which = 1 | 2)"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(sparse_factored_setup(m, h->n, colptr, rowval, nzval, b, 0.0, factor, refine, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_affine_sparse_factored_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_SPARSE_FACTORED, "fos_feas_affine_sparse_factored_stats", "is not a sparse factored IndAffine", &s));
    sparse_factored_stats(s, out8);
    return FOS_OK;
}
int fos_feas_affine_sparse_factored_plan(fos_feas_handle h, int32_t which, int64_t* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_SPARSE_FACTORED, "fos_feas_affine_sparse_factored_plan", "is not a sparse factored IndAffine", &s));
    sparse_factored_plan(s, out8);
    return FOS_OK;
}
// test-only, host: the sparse factored form's scaling, inverse, segment tables and two passes in the kernels' order (affine_sparse_factored.hip)
int fos_host_affine_sparse_factored(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, int32_t refine,
                                    const double* x, double* y) {
    return host_affine_sparse_factored(m, n, colptr, rowval, nzval, b, 0.0, refine, x, y);
}

// ---- the n-space forms (nspace.hip) and the sparse wide LeastSquares (affine_sparse_factored.hip with a shifted diagonal)
int fos_feas_set_quadratic(fos_feas_handle h, int32_t which, const double* Q, const double* q, int32_t factor) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_quadratic: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(nspace_setup_quadratic(h->n, Q, q, factor, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_set_least_squares_normal(fos_feas_handle h, int32_t which, int64_t m, const double* A, const double* b, double lambda, int32_t factor) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_least_squares_normal: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(nspace_setup_ls_dense(m, h->n, A, b, lambda, factor, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_set_least_squares_sparse(fos_feas_handle h, int32_t which, int64_t m, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b,
                                      double lambda, int32_t form, int32_t factor) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_least_squares_sparse: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    if (!(lambda > 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    if (form != FOS_LS_FORM_NORMAL && form != FOS_LS_FORM_SPARSE_FACTORED) { set_error("LeastSquares (sparse): form must be FOS_LS_FORM_SPARSE_FACTORED or FOS_LS_FORM_NORMAL"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    if (form == FOS_LS_FORM_NORMAL) FOS_TRY(nspace_setup_ls_sparse(m, h->n, colptr, rowval, nzval, b, lambda, factor, h->stream, &s));
    else FOS_TRY(sparse_factored_setup(m, h->n, colptr, rowval, nzval, b, lambda, factor, 0, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_nspace_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_NSPACE, "fos_feas_nspace_stats", "is not a Quadratic or a LeastSquares in the normal-equations form", &s));
    nspace_stats(s, out8);
    return FOS_OK;
}
// test-only, host: the n-space forms' scaling, inverse, packing and three tile products in the kernels' order (nspace.hip)
int fos_host_quadratic(int64_t n, const double* Q, const double* q, const double* x, double* y) { return host_nspace_quadratic(n, Q, q, x, y); }
int fos_host_least_squares_normal(int64_t m, int64_t n, const double* A, const double* b, double lambda, const double* x, double* y) {
    return host_nspace_ls_dense(m, n, A, b, lambda, x, y);
}
int fos_host_least_squares_sparse(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int32_t form,
                                  const double* x, double* y) {
    if (!(lambda > 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    if (form == FOS_LS_FORM_NORMAL) return host_nspace_ls_sparse(m, n, colptr, rowval, nzval, b, lambda, x, y);
    if (form != FOS_LS_FORM_SPARSE_FACTORED) { set_error("LeastSquares (sparse): form must be FOS_LS_FORM_SPARSE_FACTORED or FOS_LS_FORM_NORMAL"); return FOS_EINVAL; }
    return host_affine_sparse_factored(m, n, colptr, rowval, nzval, b, lambda, 0, x, y);
}
int fos_host_symv_packed(int64_t k, const double* X, const double* v, double* y, int32_t* count) { return host_nspace_symv_packed(k, X, v, y, count); }
// ---- the n-space forms by CG (nspace_cg.hip): a sparse Q or A of any size
int fos_feas_set_quadratic_sparse(fos_feas_handle h, int32_t which, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_quadratic_sparse: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(nspace_cg_setup_quadratic(h->n, colptr, rowval, nzval, q, tol, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_set_least_squares_cg(fos_feas_handle h, int32_t which, int64_t m, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b,
                                  double lambda, double tol) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_least_squares_cg: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(nspace_cg_setup_ls(m, h->n, colptr, rowval, nzval, b, lambda, tol, h->stream, &s));
    return feas_install(h, which, s);
}
int fos_feas_nspace_cg_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_NSPACE_CG, "fos_feas_nspace_cg_stats", "is not a Quadratic or a LeastSquares in the cg form", &s));
    nspace_cg_stats(s, out8);
    return FOS_OK;
}
// test-only, host: the cg forms' matrices, work items, recurrence and sums in the kernels' order (nspace_cg.hip)
int fos_host_quadratic_cg(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol, const double* x, double* y,
                          int32_t* iters) {
    return host_nspace_cg_quadratic(n, colptr, rowval, nzval, q, tol, x, y, iters);
}
int fos_host_least_squares_cg(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, double tol,
                              const double* x, double* y, int32_t* iters) {
    return host_nspace_cg_ls(m, n, colptr, rowval, nzval, b, lambda, tol, x, y, iters);
}
// measurement: the one-rhs tile product against red_symm_kernel on the same tiles (nspace.hip); out4 = ms per product of each, bytes of the stream, max |difference|
int fos_bench_symv_packed(int32_t device, int64_t k, int32_t reps, double* out4) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device is visible: the HIP path has no CPU fallback"); return FOS_ENODEVICE; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (0..%d)", device, ndev - 1); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(device));
    hipStream_t stream = nullptr;
    FOS_HIP(hipStreamCreate(&stream));
    const int rc = nspace_bench_symv(k, reps, stream, out4);
    (void)hipStreamDestroy(stream);
    return rc;
}

int fos_feas_set_box(fos_feas_handle h, int32_t which, double lo, double hi) {
    if (!h || which < 1 || which > 2 || !(lo <= hi)) { set_error("fos_feas_set_box: which = 1 | 2 and lo <= hi are required"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(box_setup(feas_env(h), lo, hi, nullptr, nullptr, &s));
    return feas_install(h, which, s);
}

// IndBox(lo, hi) with array bounds (n entries each; +-INFINITY allowed)
int fos_feas_set_box_arrays(fos_feas_handle h, int32_t which, const double* lo, const double* hi) {
    if (!h || which < 1 || which > 2 || !lo || !hi) { set_error("fos_feas_set_box_arrays: bad argument"); return FOS_EINVAL; }
    for (int64_t i = 0; i < h->n; ++i) if (!(lo[i] <= hi[i])) { set_error("IndBox: lo[%lld] <= hi[%lld] is required", (long long)i + 1, (long long)i + 1); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(box_setup(feas_env(h), 0.0, 0.0, lo, hi, &s));
    return feas_install(h, which, s);
}

// ConeProduct (cones.jl:31-77): ncones cones in order, contiguous from index 1, together covering all n entries
int fos_feas_set_cones(fos_feas_handle h, int32_t which, int64_t ncones, const int32_t* type, const int64_t* len) {
    if (!h || which < 1 || which > 2 || ncones < 1 || !type || !len) { set_error("fos_feas_set_cones: bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    const int64_t n = h->n;
    std::vector<int64_t> start((size_t)ncones);
    int64_t pos = 0;
    for (int64_t i = 0; i < ncones; ++i) {                 // contiguous from index 1 (cones.jl:66-72): the starts follow from the lengths
        if (len[i] < 1 || len[i] > n - pos) { set_error("ConeProduct: cone %lld (length %lld) does not fit the %lld entries (cones.jl:66-72: contiguous, gap-free ranges)", (long long)i + 1, (long long)len[i], (long long)n); return FOS_EINVAL; }
        start[(size_t)i] = pos + 1;
        pos += len[i];
    }
    FOS_TRY(cone_table_check("ConeProduct", n, ncones, type, start.data(), len));
    ConeTable table;
    table.ew.assign((size_t)n, 0);
    cone_table_add(table, 0, CONE_PRIMAL, ncones, type, start.data(), len);
    ProxObject* s = nullptr;
    FOS_TRY(cone_product_setup(feas_env(h), table, &s));
    return feas_install(h, which, s);
}

int fos_feas_set_callback(fos_feas_handle h, int32_t which, fos_prox_fn fn, void* ctx) {
    if (!h || (which != 1 && which != 2) || !fn) { set_error("fos_feas_set_callback: NULL handle / callback or which not in {1, 2}"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(callback_setup(feas_env(h), which, fn, ctx, &s));
    return feas_install(h, which, s);
}

// A separable sum of convex vector sets (sets.hip; Feasibility.jl:2-6)
int fos_feas_set_blocks(fos_feas_handle h, int32_t which, int64_t nblocks, const int32_t* kind, const int64_t* len, const double* scal, const double* vec) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_blocks: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    ProxObject* s = nullptr;
    FOS_TRY(set_blocks_setup(h->n, nblocks, kind, len, scal, vec, &s));
    return feas_install(h, which, s);
}
int fos_feas_set_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_BLOCKS, "fos_feas_set_stats", "was not defined by fos_feas_set_blocks", &s));
    FOS_HIP(hipSetDevice(h->device));
    return set_blocks_stats(s, h->stream, out8);
}

// A separable sum that may hold dense Quadratic / LeastSquares / IndAffine blocks (dense_blocks.hip); nmat == 0: fos_feas_set_blocks
int fos_feas_set_blocks2(fos_feas_handle h, int32_t which, int64_t nblocks, const int32_t* kind, const int64_t* len, const double* scal, const double* vec,
                         int64_t nmat, const int64_t* mat_rows, const int64_t* mat_cols, const double* const* mats, const int64_t* block_mat, const double* const* block_vec) {
    if (!h || which < 1 || which > 2) { set_error("fos_feas_set_blocks2: NULL handle or which not in {1, 2}"); return FOS_EINVAL; }
    if (nmat < 0) { set_error("fos_feas_set_blocks2: nmat >= 0 is required"); return FOS_EINVAL; }
    if (nmat > 0 && !block_mat) { set_error("fos_feas_set_blocks2: block_mat is required with matrices"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    DenseBlockArgs dense;
    dense.nmat = nmat; dense.mat_rows = mat_rows; dense.mat_cols = mat_cols; dense.mats = mats; dense.block_mat = block_mat; dense.block_vec = block_vec;
    ProxObject* s = nullptr;
    FOS_TRY(set_blocks_setup2(h->n, nblocks, kind, len, scal, vec, dense, &s));
    return feas_install(h, which, s);
}
int fos_feas_dense_block_stats(fos_feas_handle h, int32_t which, double* out8) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, out8, FEAS_BLOCKS, "fos_feas_dense_block_stats", "is not a separable sum with dense blocks", &s));
    if (!set_blocks_dense(s)) { set_error("fos_feas_dense_block_stats: set %d is not a separable sum with dense blocks", (int)which); return FOS_EINVAL; }
    dense_blocks_stats(set_blocks_dense(s), out8);
    return FOS_OK;
}
int fos_feas_dense_block_get(fos_feas_handle h, int32_t which, int64_t block, double* G, double* d) {
    const ProxObject* s = nullptr;
    FOS_TRY(feas_object(h, which, G, FEAS_BLOCKS, "fos_feas_dense_block_get", "is not a separable sum with dense blocks", &s));
    if (!d || !set_blocks_dense(s)) { set_error("fos_feas_dense_block_get: set %d is not a separable sum with dense blocks (or d is NULL)", (int)which); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return dense_blocks_get(set_blocks_dense(s), block, G, d);
}

int fos_feas_set_alg(fos_feas_handle h, int32_t alg, double alpha, double alpha1, double alpha2, double beta) {
    if (!h || alg < FOS_ALG_GAP || alg > FOS_ALG_DYKSTRA) { set_error("fos_feas_set_alg: unknown algorithm"); return FOS_EINVAL; }
    h->alg = alg; h->alpha = alpha; h->alpha1 = alpha1; h->alpha2 = alpha2; h->beta = beta;
    if (alg == FOS_ALG_GAPA) h->alpha1 = h->alpha2 = 2.0;              // (unused: GAPA relaxes with the device scalar alpha12)
    h->wr.off();                                                       // a fresh algorithm is unwrapped (fos_feas_set_linesearch / _longstep follow)
    return FOS_OK;
}

// GAPP(alpha, alpha1, alpha2; iproj)      solvers/gapproj.jl:5-13 (Feasibility form only)
int fos_feas_set_gapp(fos_feas_handle h, double alpha, double alpha1, double alpha2, int64_t iproj) {
    if (!h || iproj < 1) { set_error("fos_feas_set_gapp: iproj >= 1 is required"); return FOS_EINVAL; }
    h->alg = FOS_ALG_GAPP; h->alpha = alpha; h->alpha1 = alpha1; h->alpha2 = alpha2; h->beta = 0.0;
    h->wr.off();                                                       // a fresh algorithm is unwrapped (support_longstep(::GAPP) = false, gapproj.jl:83)
    h->wr.gapp_iproj = iproj;
    return FOS_OK;
}
int fos_feas_set_linesearch(fos_feas_handle h, int64_t lsinterval) {
    if (!h || lsinterval < 0) { set_error("bad argument"); return FOS_EINVAL; }
    FOS_TRY(wrappers_check(h->wr, WRAP_LINESEARCH, h->alg, false, lsinterval, 0));
    h->wr.ls_interval = lsinterval;
    return FOS_OK;
}
// LongstepWrapper on the Feasibility form (as fos_set_longstep)
int fos_feas_set_longstep(fos_feas_handle h, int64_t longinterval, int64_t nsave) {
    if (!h || longinterval < 0 || nsave < 0) { set_error("bad argument"); return FOS_EINVAL; }
    if (longinterval == 0) { h->wr.lp.interval = 0; h->wr.lp.savepos = 0; h->wr.lp.now = false; return FOS_OK; }
    FOS_TRY(wrappers_check(h->wr, WRAP_LONGSTEP, h->alg, false, longinterval, nsave));
    FOS_HIP(hipSetDevice(h->device));
    return long_setup(h->wr.lp, longinterval, nsave, (size_t)h->L / 2, (size_t)h->grid, h->stream, h->owned, [h](double** out, size_t count) { return h->zeros(out, count, h->stream); });
}
int fos_feas_linesearch_log(fos_feas_handle h, double* out34) { return wrappers_copy_log(h ? h->wr.ls_log : nullptr, 34, out34); }
int fos_feas_gapp_log(fos_feas_handle h, double* out23) { return wrappers_copy_log(h ? h->wr.gapp_log : nullptr, 23, out23); }
int fos_feas_longstep_log(fos_feas_handle h, double* out8) { return wrappers_copy_log(h ? h->wr.lp.log : nullptr, 8, out8); }

// x = x0 (NULL: zeros(n), Feasibility.jl:58) and the state of a fresh init_algorithm!: alpha12 = 2 (gapa.jl:29), t = 1, y = xold = 0
// (fista.jl:22-24), p = q = 0 (dykstra.jl:21-22), prev = NaN (Feasibility.jl:78)
int fos_feas_set_iterate(fos_feas_handle h, const double* x0) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    const size_t bytes = sizeof(double) * (size_t)h->L;
    for (double* v : {h->x, h->t1, h->t2, h->y, h->xold, h->p, h->q, h->tmp}) FOS_HIP(hipMemsetAsync(v, 0, bytes, h->stream));
    if (x0) FOS_HIP(hipMemcpyAsync(h->x, x0, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    FEAS_K(feas_fill_kernel, h->n, h->prev, (double)NAN);
    const double two = 2.0;
    FOS_HIP(hipMemcpyAsync(h->a12, &two, sizeof(double), hipMemcpyHostToDevice, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    h->fista_t = 1.0; h->status = FOS_STATUS_CONTINUE; h->checked = 0; h->err = NAN;
    for (auto& s : h->S) if (s) s->reset(h->stream);       // a new solve starts its PSD projections cold, the sparse IndAffine's multipliers at zero
    return feas_check_launch("fos_feas_set_iterate");
}

// iterations first_iter .. first_iter + niter - 1 of `iterate` (solverwrapper.jl:23-29): stops behind the iteration whose check
// found err <= eps.  done = iterations run; status / err / checked describe the LAST iteration (FeasibilityStatus fields).
int fos_feas_step(fos_feas_handle h, int64_t first_iter, int64_t niter, int64_t checki, double eps, int64_t* done, int32_t* status, double* err,
                  int32_t* checked) {
    if (!h || first_iter < 1 || niter < 0) { set_error("fos_feas_step: bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    int64_t k = 0;
    for (; k < niter; ++k) {
        FOS_TRY(feas_step_once(h, first_iter + k, checki, eps));
        if (h->status != FOS_STATUS_CONTINUE) { ++k; break; }
    }
    FOS_HIP(hipStreamSynchronize(h->stream));
    if (done) *done = k;
    if (status) *status = h->status;
    if (err) *err = h->err;
    if (checked) *checked = h->checked;
    return feas_check_launch("fos_feas_step");
}

// getsol (gap.jl:82-87, gapa.jl:107-112, fista.jl:50-56, dykstra.jl:38-44): P_S2(P_S1(x)); force_check = the `checkstatus(...,
// override = true)` of solverwrapper.jl:31-33 on that point
int fos_feas_getsol(fos_feas_handle h, double* sol, int32_t force_check, double eps, int32_t* status, double* err) {
    if (!h || !sol) { set_error("fos_feas_getsol: NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(feas_prox(h, 0, h->t1, h->x));
    FOS_TRY(feas_prox(h, 1, h->tmp, h->t1));
    if (force_check) FOS_TRY(feas_check(h, h->tmp, 0, 0, eps, true));
    FOS_HIP(hipMemcpyAsync(sol, h->tmp, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    if (status) *status = h->status;
    if (err) *err = h->err;
    return feas_check_launch("fos_feas_getsol");
}

int fos_feas_get_iterate(fos_feas_handle h, double* x) {
    if (!h || !x) { set_error("fos_feas_get_iterate: NULL argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipMemcpyAsync(x, h->x, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return FOS_OK;
}

// prox!(y, S_which, x) on host vectors (tests; the reference's prox! protocol)
int fos_feas_prox(fos_feas_handle h, int32_t which, const double* x, double* y) {
    if (!h || !x || !y || which < 1 || which > 2) { set_error("fos_feas_prox: bad argument"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipMemcpyAsync(h->tmp, x, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    FOS_TRY(feas_prox(h, which - 1, h->t2, h->tmp));
    FOS_HIP(hipMemcpyAsync(y, h->t2, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    FOS_HIP(hipStreamSynchronize(h->stream));
    return feas_check_launch("fos_feas_prox");
}

// diagnostics: alpha12 (GAPA), Newton-Schulz steps / final residual of an IndAffine set-up (0 when the set is not affine)
int fos_feas_info(fos_feas_handle h, double* alpha12, int32_t* ns_iters, double* ns_resid) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (alpha12) { FOS_HIP(hipMemcpyAsync(alpha12, h->a12, sizeof(double), hipMemcpyDeviceToHost, h->stream)); FOS_HIP(hipStreamSynchronize(h->stream)); }
    for (int k = 0; k < 2; ++k) {
        int32_t it = 0;
        double res = 0.0;
        dense_projector_stats(h->S[k].get(), &it, &res);
        if (ns_iters) ns_iters[k] = it;
        if (ns_resid) ns_resid[k] = res;
    }
    return FOS_OK;
}

}  // extern "C"
