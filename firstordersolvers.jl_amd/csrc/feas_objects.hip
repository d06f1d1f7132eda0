// The sets of the Feasibility form that need no back-end file of their own (feas.hip holds the algorithms and the ABI): each is a ProxObject that owns what its prox
// needs.
//   * IndAffine(A, b), dense projector: y = x - P x + q with P = A'(A A')^-1 A (n x n) and q = A'(A A')^-1 b from a one-time Newton-Schulz inverse of A A' on the
//     fp64 MFMA GEMM of vecops.hip (test/testfeasibility.jl:9); one dense symmetric matrix-vector product per projection (n^2 x 8 bytes: HBM bound)
//   * IndBox(lo, hi), scalar or array bounds (test/testfeasibility.jl:10)
//   * ConeProduct (cones.jl:31-94) on the batched cone kernels of the HSDE path (a ConeSet, cones.cpp) through the two-part layout those kernels read
//   * any other ProximableFunction: the caller's prox! on pinned host vectors
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "dev_common.hpp"
#include "fos_internal.hpp"

namespace fos {

namespace {

// y = x - P x + q      IndAffine: x - A'(A A')^-1 (A x - b) with P = A'(A A')^-1 A, q = A'(A A')^-1 b
__global__ __launch_bounds__(FEAS_THREADS) void feas_affine_finish_kernel(int64_t n, double* __restrict__ y, const double* __restrict__ x,
                                                                          const double* __restrict__ Px, const double* __restrict__ q) {
    FEAS_STRIDE(i, n) y[i] = (x[i] - Px[i]) + q[i];
}
// y = clamp(x, lo, hi)      IndBox
__global__ __launch_bounds__(FEAS_THREADS) void feas_box_kernel(int64_t n, double* __restrict__ y, const double* __restrict__ x, double lo, double hi) {
    FEAS_STRIDE(i, n) y[i] = fmin(fmax(x[i], lo), hi);
}
// y = clamp(x, lo[i], hi[i])      IndBox with array bounds
__global__ __launch_bounds__(FEAS_THREADS) void feas_boxv_kernel(int64_t n, double* __restrict__ y, const double* __restrict__ x,
                                                                 const double* __restrict__ lo, const double* __restrict__ hi) {
    FEAS_STRIDE(i, n) y[i] = fmin(fmax(x[i], lo[i]), hi[i]);
}
// plain vector <-> the two-part layout of the cone kernels (part 1 = the vector, part 2 = zeros: its dual projections are of zero)
__global__ __launch_bounds__(FEAS_THREADS) void feas_to_parts_kernel(int64_t n, double2* __restrict__ z, const double* __restrict__ x) {
    FEAS_STRIDE(i, n) z[i] = make_double2(x[i], 0.0);
}
__global__ __launch_bounds__(FEAS_THREADS) void feas_from_parts_kernel(int64_t n, double* __restrict__ y, const double2* __restrict__ z) {
    FEAS_STRIDE(i, n) y[i] = z[i].x;
}
// set-up: the row-major m x n matrix A as a column-major L x L array (rows 0..m-1, zero padded) and its transpose
__global__ __launch_bounds__(FEAS_THREADS) void feas_spread_kernel(int64_t m, int64_t n, int64_t L, const double* __restrict__ A,
                                                                   double* __restrict__ Ah, double* __restrict__ At) {
    FEAS_STRIDE(e, m * n) {
        const int64_t i = e / n, j = e % n;
        const double v = A[e];
        Ah[i + j * L] = v;
        At[j + i * L] = v;
    }
}
// set-up: E[i + i L] = 1 for i >= m (the padding of G = A A' + E keeps it positive definite)
__global__ __launch_bounds__(FEAS_THREADS) void feas_pad_identity_kernel(int64_t L, int64_t m, double* __restrict__ E) {
    FEAS_STRIDE(i, L) if (i >= m) E[i + i * L] = 1.0;
}

#define OBJ_K(kernel, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(FEAS_THREADS), 0, stream, __VA_ARGS__)

// what the four share: the handle's geometry and the device memory they own
struct FeasObject : ProxObject, DevOwned {
    FeasObject(int kind, const FeasEnv& env, const char* name) : ProxObject(kind), n(env.n), L(env.L), grid(env.grid), cus(env.cus) { what = name; }
    const int64_t n, L;
    const int grid, cus;
};

struct DenseProjector : FeasObject {
    explicit DenseProjector(const FeasEnv& env) : FeasObject(FEAS_AFFINE_DENSE, env, "IndAffine") {}
    double *P = nullptr, *q = nullptr, *px = nullptr;      // [L x L] A'(A A')^-1 A, column-major; [L] A'(A A')^-1 b; [L] P x
    int ns_iters = 0;                                      // Newton-Schulz steps of the set-up
    double ns_resid = 0.0;                                 // max |G X - I| it ended with
    int prox(hipStream_t stream, double* y, const double* x) override {
        LaunchCtx c{};
        c.stream = stream; c.l = n;
        launch_dense_symv(c, L, P, x, px);                 // P is symmetric: column dots = P x
        OBJ_K(feas_affine_finish_kernel, n, y, x, (const double*)px, (const double*)q);
        return FOS_OK;
    }
};

struct Box : FeasObject {
    explicit Box(const FeasEnv& env) : FeasObject(FEAS_BOX, env, "IndBox") {}
    double lo = 0.0, hi = 0.0;
    double *lov = nullptr, *hiv = nullptr;                 // [n] array bounds; nullptr: the scalars
    int prox(hipStream_t stream, double* y, const double* x) override {
        if (lov) OBJ_K(feas_boxv_kernel, n, y, x, (const double*)lov, (const double*)hiv);
        else OBJ_K(feas_box_kernel, n, y, x, lo, hi);
        return FOS_OK;
    }
};

struct ConeProduct : FeasObject {
    explicit ConeProduct(const FeasEnv& env) : FeasObject(FEAS_CONES, env, "ConeProduct") {}
    ~ConeProduct() override { cone_set_destroy(cones, nullptr); }
    ConeSet* cones = nullptr;
    double2 *zin = nullptr, *zout = nullptr;               // [n] the two-part scratch of the cone kernels
    int prox(hipStream_t stream, double* y, const double* x) override {        // prox!(y, ::ConeProduct, x)   cones.jl:89-94
        LaunchCtx c{};
        c.stream = stream; c.l = n; c.vec_blocks = grid; c.cus = cus;
        OBJ_K(feas_to_parts_kernel, n, zin, x);
        cone_set_project_vector(cones, c, zout, zin);
        FOS_TRY(cone_set_project_psd(cones, c, zout, zin));                     // (the next projection starts warm from this one's basis)
        OBJ_K(feas_from_parts_kernel, n, y, (const double2*)zout);
        return FOS_OK;
    }
    void reset(hipStream_t) override { cones->start_cold(); }                  // a new solve starts its PSD projections cold
};

struct Callback : ProxObject {
    Callback() : ProxObject(FEAS_CALLBACK) {}
    ~Callback() override { if (hx) (void)hipHostFree(hx); if (hy) (void)hipHostFree(hy); }
    fos_prox_fn fn = nullptr;
    void* ctx = nullptr;
    int64_t n = 0;
    int which = 0;
    double *hx = nullptr, *hy = nullptr;                   // pinned
    int prox(hipStream_t stream, double* y, const double* x) override {
        FOS_HIP(hipMemcpyAsync(hx, x, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
        FOS_HIP(hipStreamSynchronize(stream));
        const int32_t rc = fn(ctx, n, hx, hy);
        if (rc != 0) { set_error("feasibility form: the prox callback of set %d returned %d", which, (int)rc); return FOS_EINVAL; }
        FOS_HIP(hipMemcpyAsync(y, hy, sizeof(double) * n, hipMemcpyHostToDevice, stream));
        return FOS_OK;
    }
};

}  // namespace

// IndAffine(A, b): A is m x n, ROW-major (C order), full row rank.  One-time set-up on the device:
//   G = A A' (+ identity on the padding), X = G^-1 by Newton-Schulz  X <- 2 X - X (G X)  from X_0 = I / (1.25 |A|_F^2),
//   P = A' X A,  q = A' X b.
int dense_projector_setup(const FeasEnv& env, int64_t m, const double* A, const double* b, ProxObject** out) {
    const int64_t n = env.n, L = env.L;
    const hipStream_t stream = env.stream;
    const int grid = env.grid;
    const size_t L2 = (size_t)L * (size_t)L;
    std::vector<double> bp((size_t)L, 0.0);
    double fro2 = 0.0;
    for (int64_t e = 0; e < m * n; ++e) {
        const double v = A[e];
        if (!(v == v) || std::fabs(v) > 1e300) { set_error("IndAffine: A has non-finite entries"); return FOS_EINVAL; }
        fro2 += v * v;
    }
    for (int64_t i = 0; i < m; ++i) bp[(size_t)i] = b[i];
    if (!(fro2 > 0.0)) { set_error("IndAffine: A is zero"); return FOS_EINVAL; }
    DenseProjector* s = new DenseProjector(env);
    DevOwned work;                                                                      // the set-up's buffers: freed when this returns
    work.what = s->what;
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete s; return code; };
    double *dA = nullptr, *dAt = nullptr, *G = nullptr, *B0 = nullptr, *B1 = nullptr, *B2 = nullptr, *db = nullptr, *dt = nullptr, *draw = nullptr;
    int rc = FOS_OK;
    for (double** q : {&dA, &dAt, &G, &B0, &B1, &B2}) if (rc == FOS_OK) rc = work.alloc(q, L2);
    for (double** q : {&db, &dt}) if (rc == FOS_OK) rc = work.alloc(q, (size_t)L);
    if (rc == FOS_OK) rc = work.alloc(&draw, (size_t)(m * n));
    if (rc == FOS_OK) rc = s->zeros(&s->P, L2, stream);
    if (rc == FOS_OK) rc = s->zeros(&s->q, (size_t)L, stream);
    if (rc == FOS_OK) rc = s->zeros(&s->px, (size_t)L, stream);
    if (rc != FOS_OK) return fail(rc);
    DEV_HIP(s, hipMemcpyAsync(draw, A, sizeof(double) * (size_t)(m * n), hipMemcpyHostToDevice, stream));
    DEV_HIP(s, hipMemsetAsync(dA, 0, sizeof(double) * L2, stream));
    DEV_HIP(s, hipMemsetAsync(dAt, 0, sizeof(double) * L2, stream));
    hipLaunchKernelGGL(feas_spread_kernel, dim3(1024), dim3(FEAS_THREADS), 0, stream, m, n, L, (const double*)draw, dA, dAt);
    DEV_HIP(s, hipMemcpyAsync(db, bp.data(), sizeof(double) * (size_t)L, hipMemcpyHostToDevice, stream));
    DEV_HIP(s, hipMemsetAsync(B0, 0, sizeof(double) * L2, stream));
    DEV_HIP(s, hipMemsetAsync(B1, 0, sizeof(double) * L2, stream));
    LaunchCtx c{};
    c.stream = stream; c.l = L;
    OBJ_K(feas_pad_identity_kernel, L, m, B0);                                         // E
    launch_dense_gemm(c, (int)L, 1.0, dA, dAt, 1.0, B0, G);                            // G = A A' + E   (block diagonal, positive definite)
    launch_dense_scale_identity(c, L, B1, 1.0 / (1.25 * std::max(fro2, 1.0)));         // X_0: lambda_max(G) <= max(|A|_F^2, 1)
    double *X = B1, *Xn = B2;
    std::vector<double> part(256);
    double resid = 1.0, prev_resid = 2.0;
    int it = 0;
    for (; it < 120; ++it) {
        launch_dense_gemm(c, (int)L, 1.0, G, X, 0.0, nullptr, B0);                     // Y = G X
        launch_dense_resid(c, L, B0, env.partials, 256);
        DEV_HIP(s, hipMemcpyAsync(part.data(), env.partials, sizeof(double) * 256, hipMemcpyDeviceToHost, stream));
        DEV_HIP(s, hipStreamSynchronize(stream));
        resid = 0.0;
        for (double r : part) resid = (r > resid || r != r) ? r : resid;
        if (resid != resid) { set_error("IndAffine set-up: the inverse of A A' produced NaN"); return fail(FOS_EINVAL); }
        if (resid <= 2e-14 || (resid <= 1e-10 && resid >= 0.5 * prev_resid)) break;   // rounding level: the residual no longer squares
        prev_resid = resid;
        launch_dense_gemm(c, (int)L, -1.0, X, B0, 2.0, X, Xn);                         // X <- 2 X - X Y
        std::swap(X, Xn);
    }
    if (!(resid <= 1e-10)) {
        set_error("IndAffine set-up: the inverse of A A' did not converge (max |G X - I| = %.3e after %d Newton-Schulz steps): A needs full row rank and a moderate condition number", resid, it);
        return fail(FOS_EINVAL);
    }
    launch_dense_gemm(c, (int)L, 1.0, X, dA, 0.0, nullptr, B0);                        // B0 = X A
    launch_dense_gemm(c, (int)L, 1.0, dAt, B0, 0.0, nullptr, s->P);                    // P = A' X A
    launch_dense_symv(c, L, X, db, dt);                                                // t = X b   (X symmetric)
    launch_dense_symv(c, L, dA, dt, s->q);                                             // q[col] = A[:, col] . t = (A' t)[col]
    DEV_HIP(s, hipStreamSynchronize(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("IndAffine set-up: a kernel launch failed: %s", hipGetErrorString(e)); return fail(FOS_EHIP); }
    s->ns_iters = it; s->ns_resid = resid;
    *out = s;
    return FOS_OK;
}
void dense_projector_stats(const ProxObject* p, int32_t* ns_iters, double* ns_resid) {
    const DenseProjector* s = p && p->kind == FEAS_AFFINE_DENSE ? static_cast<const DenseProjector*>(p) : nullptr;
    *ns_iters = s ? s->ns_iters : 0;
    *ns_resid = s ? s->ns_resid : 0.0;
}

// IndBox(lo, hi); lov, hiv: array bounds on the host (n entries each; +-INFINITY allowed), or both nullptr: the scalars
int box_setup(const FeasEnv& env, double lo, double hi, const double* lov, const double* hiv, ProxObject** out) {
    Box* s = new Box(env);
    s->lo = lo; s->hi = hi;
    if (lov) {
        auto fail = [&](int code) { (void)hipStreamSynchronize(env.stream); delete s; return code; };
        int rc = s->upload(&s->lov, lov, (size_t)env.n, env.stream);
        if (rc == FOS_OK) rc = s->upload(&s->hiv, hiv, (size_t)env.n, env.stream);
        if (rc != FOS_OK) return fail(rc);
        DEV_HIP(s, hipStreamSynchronize(env.stream));
    }
    *out = s;
    return FOS_OK;
}

// ConeProduct over a validated table of n entries (feas.hip builds it)
int cone_product_setup(const FeasEnv& env, const ConeTable& table, ProxObject** out) {
    ConeProduct* s = new ConeProduct(env);
    auto fail = [&](int code) { (void)hipStreamSynchronize(env.stream); delete s; return code; };
    int rc = cone_set_build(table, env.n, ConeSetOptions{}, PsdTuning{}, &s->cones);
    if (rc == FOS_OK) rc = s->zeros(&s->zin, (size_t)env.n, env.stream);
    if (rc == FOS_OK) rc = s->zeros(&s->zout, (size_t)env.n, env.stream);
    if (rc != FOS_OK) return fail(rc);
    DEV_HIP(s, hipStreamSynchronize(env.stream));
    *out = s;
    return FOS_OK;
}

int callback_setup(const FeasEnv& env, int which, fos_prox_fn fn, void* ctx, ProxObject** out) {
    Callback* s = new Callback();
    s->fn = fn; s->ctx = ctx; s->n = env.n; s->which = which;
    const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(env.n, 1);
    if (hipHostMalloc((void**)&s->hx, bytes) != hipSuccess || hipHostMalloc((void**)&s->hy, bytes) != hipSuccess) {
        delete s;
        set_error("fos_feas_set_callback: pinned host buffers of %lld doubles could not be allocated", (long long)env.n);
        return FOS_ENOMEM;
    }
    *out = s;
    return FOS_OK;
}

}  // namespace fos
