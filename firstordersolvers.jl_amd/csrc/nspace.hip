// Proximable functions whose prox is a solve in the n-space:  y = M^-1 (x + c)  for a symmetric positive definite M of order n <= 46 000 with lambda_min(M) >= 1.
//   Quadratic(Q, q):           f(x) = 1/2 x'Qx + q'x,       prox_f(x) = (I + Q)^-1 (x - q):                  M = I + Q,           c = -q
//   LeastSquares(A, b, lambda): f(x) = lambda/2 |A x - b|^2, prox_f(x) = (I + lambda A'A)^-1 (x + lambda A'b): M = I + lambda A'A,  c = lambda A'b   (any m >= 1)
// (gamma = 1: the Feasibility form calls every prox with step 1, as Feasibility.jl does.)  ProximalOperators factors the same matrices (Quadratic; LeastSquares
// with a tall or sparse A); here the n-space is kept as an explicit inverse, as the factored IndAffine keeps its m-space (affine_dense.hip).
//
//   * set-up: M on the device -- dense A: launch_dense_gram_rows (dense_chol.hip) on A', the row-major n x m matrix transposed once; sparse A: sf_gram_kernel
//     (affine_sparse_factored.hip) on the CSR of A'; Q: its LOWER triangle (no symmetry test).  Jacobi scaling to a unit diagonal, Mt = D M D with
//     D_ii = M_ii^-1/2 (the factored forms do the same with rows); K = Mt^-1 by dense_spd_inverse (direct.cpp) at the probe bar of the factored forms; a pivot that
//     fails (Q not positive semidefinite) is FOS_EINVAL naming the column.  BOTH Mt and K are packed as the lower-triangle tile streams of direct_reduced.hip
//     (build_reduced_plan, red_pack_tiles_kernel: 4 L^2 bytes each) and the dense squares are freed.  D and ct = D c stay.
//   * a prox, with w = D x + ct:   z = K w;   z += K (w - Mt z)  (one correction step: its error is (I - K Mt)^2 Mt^-1 w, the square of what the explicit inverse
//     left);   y = D z.   Three products and their folds: six launches, whatever n.  w, the residual and the last scaling are formed in the operand loads and the
//     fold epilogues, not in launches of their own.  No host synchronise, no copy.
//   * the product (ns_symv_kernel): ONE right-hand side over the packed tiles -- RedPlan units, 64 x 32 tiles, lane = row.  T x_J stays in the lane and goes to the
//     tile's own slot; T' x_I is kept in 32 accumulators per lane over the whole unit and crosses the lanes once, at the unit's end, in a fixed order.  16
//     non-temporal 16-byte loads per lane per tile, issued half a tile ahead of their use.  With half the accumulators of red_symm_kernel (built around two
//     right-hand sides, one workgroup per CU) the kernel takes 164 registers: three workgroups per CU.  A second whole tile in flight per wavefront (256 registers,
//     one workgroup per CU) measured the same time and was not kept.  ns_fold_kernel adds the slots.
//   Nothing is atomic and every sum has a fixed order: the same input gives the same bits.
#include "fos_solver.hpp"
#include "dev_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace fos {

namespace {

constexpr int NS_T = 256;                     // threads per workgroup: four units
constexpr int NS_FOLD_WAVES = 16;             // wavefronts of a fold workgroup
constexpr int NS_LAUNCHES = 6;                // per prox: three products, three folds
constexpr int64_t NS_MAX_N = 46000;
constexpr double NS_BAR = 1e-7;               // the inverse of Mt is accepted at this probe residual (DA_BAR of affine_dense.hip: the correction step squares it)
typedef double ns_v2d __attribute__((ext_vector_type(2)));

// an operand of the product or the first term of a fold: element i is 0 beyond n, else v[i] (d == nullptr) or fma(d[i], v[i], c[i]) -- w = D x + ct, formed where it is used
struct NsVec { const double* v; const double* d; const double* c; int64_t n; };
__device__ __forceinline__ double ns_elem(const NsVec& o, int64_t i) {
    if (i >= o.n) return 0.0;
    const double v = o.v[i];
    return o.d ? fma(o.d[i], v, o.c[i]) : v;
}

// ------------------------------------------------------------------------------------------------ the tile product (hot path)
__device__ __forceinline__ void ns_load_half(ns_v2d (&a)[16], int half, const double* __restrict__ tile, int lane) {
    const ns_v2d* __restrict__ tp = reinterpret_cast<const ns_v2d*>(tile);
#pragma unroll
    for (int q = 0; q < 8; ++q) a[8 * half + q] = __builtin_nontemporal_load(tp + (8 * half + q) * 64 + lane);
}
// half a tile: the row side into ry (columns ascending), the column side into the unit's 32 accumulators
__device__ __forceinline__ void ns_mul_half(const ns_v2d (&a)[16], int half, const double* xs, double xi, double& ry, double (&ca)[32]) {
#pragma unroll
    for (int q = 8 * half; q < 8 * half + 8; ++q) {
        const ns_v2d x = *reinterpret_cast<const ns_v2d*>(xs + 2 * q);
        ry += a[q].x * x.x;
        ry += a[q].y * x.y;
        ca[2 * q] += a[q].x * xi;
        ca[2 * q + 1] += a[q].y * xi;
    }
}
// the strip's 32 operands stay in LDS: hoisted out of the tile loop they would cost 64 registers
__device__ __forceinline__ const double* ns_pin(const double* xs) {
    int xoff = 0;
    asm volatile("" : "+v"(xoff));
    return xs + xoff;
}
// One tile in registers, requested half a tile ahead: while a half is multiplied, the other half and the next tile's first half are in flight.  164 registers,
// three workgroups per CU (red_symm_kernel: one).  (I, strip j) -> rowslot[(I (I + 1) + j) * 64 + lane]: row block I has its 2 I + 2 strips side by side.
__global__ __launch_bounds__(NS_T, 3) void ns_symv_kernel(const RedUnit* __restrict__ units, int nunits, const double* __restrict__ tiles, NsVec op,
                                                          double* __restrict__ rowslot, double* __restrict__ colslot) {
    __shared__ __attribute__((aligned(16))) double xs_all[NS_T / 64 * RED_TC];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int unit = blockIdx.x * (NS_T / 64) + wv;
    if (unit >= nunits) return;                                   // (no workgroup barrier below: wavefronts are independent)
    const RedUnit u = units[unit];
    double* xs = xs_all + wv * RED_TC;
    if (lane < RED_TC) xs[lane] = ns_elem(op, (int64_t)RED_TC * u.j + lane);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);                                // the wavefront's own LDS writes have landed before its reads
    double ca[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) ca[i] = 0.0;
    const int J = u.j >> 1;
    const double* tile = tiles + (size_t)u.tile0 * RED_TILE;
    double* slot = rowslot + ((int64_t)u.i0 * (u.i0 + 1) + u.j) * 64 + lane;
    ns_v2d a[16];
    ns_load_half(a, 0, tile, lane);
    ns_load_half(a, 1, tile, lane);
    double xi = ns_elem(op, (int64_t)RED_TR * u.i0 + lane);
    int I = u.i0;
    for (; I + 1 < u.i1; ++I) {                                   // (the unit's last tile is peeled off: nothing to request behind it)
        const double* next = tile + RED_TILE;
        const double xin = ns_elem(op, (int64_t)RED_TR * (I + 1) + lane);
        const double xe = (I == J) ? 0.0 : xi;
        const double* xsv = ns_pin(xs);
        double ry = 0.0;
        ns_mul_half(a, 0, xsv, xe, ry, ca);
        ns_load_half(a, 0, next, lane);
        ns_mul_half(a, 1, xsv, xe, ry, ca);
        ns_load_half(a, 1, next, lane);
        *slot = ry;
        slot += (int64_t)(2 * I + 2) * 64;
        tile = next;
        xi = xin;
    }
    {
        const double xe = (I == J) ? 0.0 : xi;
        double ry = 0.0;
        ns_mul_half(a, 0, xs, xe, ry, ca);
        ns_mul_half(a, 1, xs, xe, ry, ca);
        *slot = ry;
    }
    // column sums: 32 values per lane over 64 lanes -> after five halving stages lane L holds column L & 31 summed over the 32 lanes of its half, then the halves
#pragma unroll
    for (int half = 16; half >= 1; half >>= 1) {
        const bool up = (lane & half) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const double send = up ? ca[i] : ca[i + half];
            const double keep = up ? ca[i + half] : ca[i];
            ca[i] = keep + __shfl_xor(send, half, 64);
        }
    }
    const double s = ca[0] + __shfl_xor(ca[0], 32, 64);
    if (lane < RED_TC) colslot[(int64_t)unit * RED_TC + lane] = s;
}
// s[64 I + r] = the row slots of (I, 0 .. 2 I + 1) + the column slots of the units of the row's strip, in a fixed order: 16 wavefronts take the row slots round
// robin, their sums are added in wavefront order, then the units in stream order.  The epilogue (i = 64 I + r):
//   mode 0: out[i] = s                       z = K w
//   mode 1: out[i] = w[i] - s                the residual w - Mt z   (w = D x + ct, formed again from the same three numbers: the same bits)
//   mode 2: out[i] = d[i] (z[i] + s), i < n  y = D (z + K r)
__global__ __launch_bounds__(64 * NS_FOLD_WAVES) void ns_fold_kernel(const double* __restrict__ rowslot, const double* __restrict__ colslot,
                                                                     const int32_t* __restrict__ strip_u0, int mode, NsVec w, const double* __restrict__ z,
                                                                     double* __restrict__ out) {
    __shared__ double part[NS_FOLD_WAVES][64];
    const int I = blockIdx.x, r = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc = 0.0;
    const double* base = rowslot + (int64_t)I * (I + 1) * 64 + r;
    for (int jj = wv; jj < 2 * I + 2; jj += NS_FOLD_WAVES) acc += base[(int64_t)jj * 64];
    part[wv][r] = acc;
    __syncthreads();
    if (wv != 0) return;
    double s = part[0][r];
    for (int q = 1; q < NS_FOLD_WAVES; ++q) s += part[q][r];
    const int j = 2 * I + (r >> 5), c = r & 31;
    for (int u = strip_u0[j]; u < strip_u0[j + 1]; ++u) s += colslot[(int64_t)u * RED_TC + c];
    const int64_t i = (int64_t)RED_TR * I + r;
    if (mode == 0) out[i] = s;
    else if (mode == 1) out[i] = ns_elem(w, i) - s;
    else if (i < w.n) out[i] = w.d[i] * (z[i] + s);
}

// ------------------------------------------------------------------------------------------------ set-up kernels
// At[j * ld + i] = A[i * n + j]: the row-major n x ld transpose (ld >= m, zeroed by the caller) of the row-major m x n matrix A
__global__ __launch_bounds__(NS_T) void ns_transpose_kernel(int64_t m, int64_t n, int64_t ld, const double* __restrict__ A, double* __restrict__ At) {
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const int64_t nbj = (n + 31) / 32, nbi = (m + 31) / 32;
    for (int64_t blk = blockIdx.x; blk < nbi * nbj; blk += gridDim.x) {
        const int64_t i0 = (blk / nbj) * 32, j0 = (blk % nbj) * 32;
        __syncthreads();
        for (int k = ty; k < 32; k += 8) { const int64_t i = i0 + k, j = j0 + tx; t[k][tx] = (i < m && j < n) ? A[i * n + j] : 0.0; }
        __syncthreads();
        for (int k = ty; k < 32; k += 8) { const int64_t j = j0 + k, i = i0 + tx; if (i < m && j < n) At[j * ld + i] = t[tx][k]; }
    }
}
// c[j] = lambda sum_i At[j, i] b[i]: one wavefront per row, the lanes stride the row, one wave_sum
__global__ __launch_bounds__(NS_T) void ns_rowdot_kernel(int64_t n, int64_t m, int64_t ld, const double* __restrict__ At, const double* __restrict__ b, double lambda,
                                                         double* __restrict__ c) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = blockIdx.x * (int64_t)(NS_T / 64) + (threadIdx.x >> 6); j < n; j += (int64_t)gridDim.x * (NS_T / 64)) {
        double acc = 0.0;
        for (int64_t i = lane; i < m; i += 64) acc += At[j * ld + i] * b[i];
        acc = wave_sum(acc);
        if (lane == 0) c[j] = lambda * acc;
    }
}
// the same over the CSR of A' (rows j of A' = columns of A): entries in order, lane-strided
__global__ __launch_bounds__(NS_T) void ns_rowdot_csr_kernel(int64_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci, const double* __restrict__ va,
                                                             const double* __restrict__ b, double lambda, double* __restrict__ c) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = blockIdx.x * (int64_t)(NS_T / 64) + (threadIdx.x >> 6); j < n; j += (int64_t)gridDim.x * (NS_T / 64)) {
        double acc = 0.0;
        for (int e = rp[j] + lane; e < rp[j + 1]; e += 64) acc += va[e] * b[ci[e]];
        acc = wave_sum(acc);
        if (lane == 0) c[j] = lambda * acc;
    }
}
// element (i, j), i >= j, of S: the lower triangle of the row-major n x n Q (quad), or of the column-major Gram matrix with leading dimension L
__device__ __forceinline__ double ns_src(int quad, int64_t n, int64_t L, const double* __restrict__ S, int64_t i, int64_t j) { return quad ? S[i * n + j] : S[i + j * L]; }
// D[i] = (1 + lambda S[i, i])^-1/2, i < n; 0 on the padding
__global__ __launch_bounds__(NS_T) void ns_diag_kernel(int64_t n, int64_t L, int quad, const double* __restrict__ S, double lambda, double* __restrict__ D) {
    for (int64_t i = blockIdx.x * (int64_t)NS_T + threadIdx.x; i < L; i += (int64_t)gridDim.x * NS_T) D[i] = i < n ? 1.0 / sqrt(fma(lambda, ns_src(quad, n, L, S, i, i), 1.0)) : 0.0;
}
// Mt = D (I + lambda S) D, L x L column-major, both triangles from the lower triangle of S (exactly symmetric); identity on the padding
__global__ __launch_bounds__(NS_T) void ns_scale_kernel(int64_t n, int64_t L, int quad, const double* __restrict__ S, double lambda, const double* __restrict__ D,
                                                        double* __restrict__ Mt) {
    for (int64_t e = blockIdx.x * (int64_t)NS_T + threadIdx.x; e < L * L; e += (int64_t)gridDim.x * NS_T) {
        const int64_t i = e % L, j = e / L;
        double v = i == j ? 1.0 : 0.0;
        if (i < n && j < n) {
            const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
            v = D[hi] * (fma(lambda, ns_src(quad, n, L, S, hi, lo), v) * D[lo]);
        }
        Mt[e] = v;
    }
}
// ct = D c
__global__ __launch_bounds__(NS_T) void ns_ct_kernel(int64_t L, const double* __restrict__ D, const double* __restrict__ c, double* __restrict__ ct) {
    for (int64_t i = blockIdx.x * (int64_t)NS_T + threadIdx.x; i < L; i += (int64_t)gridDim.x * NS_T) ct[i] = D[i] * c[i];
}

int ns_check_common(const char* what, int64_t n, int factor) {
    if (n < 1) { set_error("%s: n >= 1 is required", what); return FOS_EINVAL; }
    if (n > NS_MAX_N) { set_error("%s: the inverse of the n-space matrix has order n = %lld: supported up to n = %lld (beyond that: a host prox through fos_feas_set_callback)", what, (long long)n, (long long)NS_MAX_N); return FOS_EUNSUPPORTED; }
    if (factor != FOS_DIRECT_FACTOR_NEWTON && factor != FOS_DIRECT_FACTOR_CHOLESKY) { set_error("%s: factor must be FOS_DIRECT_FACTOR_NEWTON or FOS_DIRECT_FACTOR_CHOLESKY", what); return FOS_EINVAL; }
    return FOS_OK;
}
bool ns_finite(const double* v, int64_t count) {
    for (int64_t i = 0; i < count; ++i) if (!(v[i] == v[i]) || std::fabs(v[i]) > 1e300) return false;
    return true;
}
int ns_check_lambda(double lambda) {
    if (!(lambda > 0.0) || lambda > 1e300) { set_error("LeastSquares: lambda must be finite and > 0"); return FOS_EINVAL; }
    return FOS_OK;
}
// Quadratic: finite entries, and a diagonal of I + Q the scaling can take a root of (the first test a Q that is not positive semidefinite can fail)
int ns_check_quadratic(int64_t n, const double* Q, const double* q) {
    if (!Q || !q) { set_error("Quadratic: bad argument"); return FOS_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (!ns_finite(Q + i * n, i + 1)) { set_error("Quadratic: Q has non-finite entries"); return FOS_EINVAL; }
    if (!ns_finite(q, n)) { set_error("Quadratic: q has non-finite entries"); return FOS_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (!(1.0 + Q[i * n + i] > 0.0)) { set_error("Quadratic: the pivot of column %lld of I + Q is not a positive finite number (Q is not positive semidefinite)", (long long)i); return FOS_EINVAL; }
    return FOS_OK;
}
// a sparse A for the normal-equations form: CSC, 1-based, row indices strictly ascending in every column (sf_gram_kernel adds a row's entries side by side): validated, then A and A' in CSR
int ns_sparse_rows(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, HostCsr* A, HostCsr* At) {
    const char* what = "LeastSquares (sparse, normal)";
    if (!b) { set_error("%s: bad argument", what); return FOS_EINVAL; }
    FOS_TRY(csc_check(what, m, n, colptr, rowval, nzval, CscRules{false, true, CSC_BOUND_ROWS, "A"}));
    if (!ns_finite(b, m)) { set_error("%s: b has non-finite entries", what); return FOS_EINVAL; }
    csc_to_csr_pair(m, n, colptr, rowval, nzval, nullptr, A, At);
    return FOS_OK;
}

}  // namespace

struct NSpace : ProxObject, DevOwned {
    NSpace() : ProxObject(FEAS_NSPACE) {}
    int prox(hipStream_t stream, double* y, const double* x) override;
    int64_t n = 0, m = 0, L = 0;              // m = 0: Quadratic
    RedPlan plan;
    RedDev rM{}, rK{};                        // the two tile streams over one plan, one set of slots
    RedUnit* units = nullptr; int32_t* strip_u0 = nullptr;
    double *tilesM = nullptr, *tilesK = nullptr, *rowslot = nullptr, *colslot = nullptr;
    double *D = nullptr, *ct = nullptr, *z = nullptr, *r = nullptr;     // L-vectors, zero on the padding
    DenseInv inv;
};

namespace {
int ns_grid(int64_t count) { return (int)std::max<int64_t>(1, std::min<int64_t>((count + NS_T - 1) / NS_T, 4096)); }

// what the three set-ups share.  `form` leaves S (the lower triangle of Q, or of A'A: quad says which) readable until this returns and c (L doubles, zero on
// the padding) in a->r; B0 of the work-set may hold S.
struct NsSource { int quad; const double* S; double lambda; };
int ns_build(NSpace* a, int factor, hipStream_t stream, const char* gname, DenseWork& w, const NsSource& src) {
    const int64_t n = a->n, L = a->L;
    const size_t L2 = (size_t)L * (size_t)L;
    const char* what = a->what;
    hipLaunchKernelGGL(ns_diag_kernel, dim3(ns_grid(L)), dim3(NS_T), 0, stream, n, L, src.quad, src.S, src.lambda, a->D);
    hipLaunchKernelGGL(ns_scale_kernel, dim3(ns_grid((int64_t)L2)), dim3(NS_T), 0, stream, n, L, src.quad, src.S, src.lambda, (const double*)a->D, w.G);
    hipLaunchKernelGGL(ns_ct_kernel, dim3(ns_grid(L)), dim3(NS_T), 0, stream, L, (const double*)a->D, (const double*)a->r, a->ct);
    FOS_TRY(a->hip("hipMemcpyAsync", hipMemcpyAsync(a->units, a->plan.units.data(), sizeof(RedUnit) * a->plan.units.size(), hipMemcpyHostToDevice, stream)));
    FOS_TRY(a->hip("hipMemcpyAsync", hipMemcpyAsync(a->strip_u0, a->plan.strip_u0.data(), sizeof(int32_t) * a->plan.strip_u0.size(), hipMemcpyHostToDevice, stream)));
    double* X = nullptr;
    DenseOpts o{what, gname, factor, false};
    o.bar = NS_BAR; o.newton_extra = 40;
    FOS_TRY(dense_spd_inverse(w, o, &X, &a->inv));
    launch_red_pack_tiles(w.c, a->rM, L, w.G);
    launch_red_pack_tiles(w.c, a->rK, L, X);
    FOS_TRY(a->hip("hipMemsetAsync", hipMemsetAsync(a->r, 0, sizeof(double) * (size_t)L, stream)));
    FOS_TRY(a->hip("hipStreamSynchronize", hipStreamSynchronize(stream)));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s set-up: a kernel launch failed: %s", what, hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}
// the object's own buffers and the work-set of the inversion (w.G = Mt and B0..B2 from the scratch)
int ns_prepare(NSpace* a, int64_t n, int64_t m, const char* what, hipStream_t stream, Scratch& s, DenseWork& w) {
    a->n = n; a->m = m; a->what = what; a->L = (n + 63) / 64 * 64;
    build_reduced_plan(n, &a->plan);
    const RedPlan& P = a->plan;
    const size_t L = (size_t)a->L, L2 = L * L;
    FOS_TRY(a->alloc(&a->units, P.units.size()));
    FOS_TRY(a->alloc(&a->strip_u0, P.strip_u0.size()));
    FOS_TRY(a->alloc(&a->tilesM, (size_t)P.ntiles * RED_TILE));
    FOS_TRY(a->alloc(&a->tilesK, (size_t)P.ntiles * RED_TILE));
    FOS_TRY(a->alloc(&a->rowslot, (size_t)P.ntiles * 64));
    FOS_TRY(a->alloc(&a->colslot, P.units.size() * RED_TC));
    for (double** v : {&a->D, &a->ct, &a->z, &a->r}) {
        FOS_TRY(a->zeros(v, L, stream));
    }
    RedDev R{};
    R.k = n; R.kpad = a->L; R.nt = P.nt; R.nunits = (int)P.units.size(); R.units = a->units; R.strip_u0 = a->strip_u0;
    a->rM = R; a->rM.tiles = a->tilesM;
    a->rK = R; a->rK.tiles = a->tilesK;
    w.c.stream = stream; w.c.l = n; w.L = a->L;
    w.G = s.alloc<double>(L2);
    w.fill(s);
    if (s.err != hipSuccess) { (void)hipGetLastError(); set_error("%s: hipMalloc of the set-up buffers (4 x %zu bytes) failed: %s", what, L2 * 8, hipGetErrorString(s.err)); return FOS_ENOMEM; }
    return FOS_OK;
}
}  // namespace

// Quadratic(Q, q): Q n x n (its lower triangle is read: Q[i * n + j], i >= j), q[n].  Synchronises `stream`.
int nspace_setup_quadratic(int64_t n, const double* Q, const double* q, int factor, hipStream_t stream, ProxObject** out) {
    const char* what = "Quadratic";
    FOS_TRY(ns_check_common(what, n, factor));
    FOS_TRY(ns_check_quadratic(n, Q, q));
    NSpace* a = new NSpace();
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete a; return code; };
    int rc = FOS_OK;
    {
        Scratch s;
        DenseWork w;
        if ((rc = ns_prepare(a, n, 0, what, stream, s, w)) != FOS_OK) return fail(rc);
        double* dQ = s.alloc<double>((size_t)n * (size_t)n);
        if (s.err != hipSuccess) { (void)hipGetLastError(); set_error("Quadratic: hipMalloc of Q (%zu bytes) failed: %s", (size_t)n * (size_t)n * 8, hipGetErrorString(s.err)); return fail(FOS_ENOMEM); }
        std::vector<double> c((size_t)n);
        for (int64_t i = 0; i < n; ++i) c[(size_t)i] = -q[i];
        DEV_HIP(a, hipMemcpyAsync(dQ, Q, sizeof(double) * (size_t)n * (size_t)n, hipMemcpyHostToDevice, stream));
        DEV_HIP(a, hipMemcpyAsync(a->r, c.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream));
        if ((rc = ns_build(a, factor, stream, "I + Q", w, NsSource{1, dQ, 1.0})) != FOS_OK) return fail(rc);
    }
    *out = a;
    return FOS_OK;
}

// LeastSquares(A, b, lambda), normal-equations form, A dense m x n ROW-major, any m >= 1.  Synchronises `stream`.
int nspace_setup_ls_dense(int64_t m, int64_t n, const double* A, const double* b, double lambda, int factor, hipStream_t stream, ProxObject** out) {
    const char* what = "LeastSquares (normal)";
    FOS_TRY(ns_check_lambda(lambda));
    FOS_TRY(ns_check_common(what, n, factor));
    if (m < 1 || !A || !b) { set_error("%s: bad argument (m >= 1)", what); return FOS_EINVAL; }
    if (!ns_finite(A, m * n)) { set_error("%s: A has non-finite entries", what); return FOS_EINVAL; }
    if (!ns_finite(b, m)) { set_error("%s: b has non-finite entries", what); return FOS_EINVAL; }
    NSpace* a = new NSpace();
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete a; return code; };
    int rc = FOS_OK;
    {
        Scratch s;
        DenseWork w;
        if ((rc = ns_prepare(a, n, m, what, stream, s, w)) != FOS_OK) return fail(rc);
        const int64_t ld = (m + 63) / 64 * 64;
        double* dA = s.alloc<double>((size_t)m * (size_t)n);
        double* dAt = s.alloc<double>((size_t)n * (size_t)ld);
        double* db = s.alloc<double>((size_t)m);
        if (s.err != hipSuccess) { (void)hipGetLastError(); set_error("%s: hipMalloc of A and A' (%zu bytes) failed: %s", what, ((size_t)m * n + (size_t)n * ld) * 8, hipGetErrorString(s.err)); return fail(FOS_ENOMEM); }
        DEV_HIP(a, hipMemcpyAsync(dA, A, sizeof(double) * (size_t)m * (size_t)n, hipMemcpyHostToDevice, stream));
        DEV_HIP(a, hipMemcpyAsync(db, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
        DEV_HIP(a, hipMemsetAsync(dAt, 0, sizeof(double) * (size_t)n * (size_t)ld, stream));
        const int64_t nblk = ((m + 31) / 32) * ((n + 31) / 32);
        hipLaunchKernelGGL(ns_transpose_kernel, dim3((unsigned)std::min<int64_t>(nblk, 65536)), dim3(NS_T), 0, stream, m, n, ld, (const double*)dA, dAt);
        hipLaunchKernelGGL(ns_rowdot_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, 4096)), dim3(NS_T), 0, stream, n, m, ld, (const double*)dAt, (const double*)db, lambda, a->r);
        launch_dense_gram_rows(w.c, n, ld, dAt, a->L, w.B0);                       // A'A (+ identity on the padding) in B0: read before the inversion reuses it
        if ((rc = ns_build(a, factor, stream, "I + lambda A'A", w, NsSource{0, w.B0, lambda})) != FOS_OK) return fail(rc);
    }
    *out = a;
    return FOS_OK;
}

// the same with a sparse A (CSC, 1-based, strictly ascending row indices per column).  Synchronises `stream`.
int nspace_setup_ls_sparse(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int factor,
                           hipStream_t stream, ProxObject** out) {
    const char* what = "LeastSquares (sparse, normal)";
    FOS_TRY(ns_check_lambda(lambda));
    FOS_TRY(ns_check_common(what, n, factor));
    HostCsr A, At;
    FOS_TRY(ns_sparse_rows(m, n, colptr, rowval, nzval, b, &A, &At));
    NSpace* a = new NSpace();
    auto fail = [&](int code) { (void)hipStreamSynchronize(stream); delete a; return code; };
    int rc = FOS_OK;
    {
        Scratch s;
        DenseWork w;
        if ((rc = ns_prepare(a, n, m, what, stream, s, w)) != FOS_OK) return fail(rc);
        DevOwned tmp;                                                              // A, A' and b: needed for the set-up only
        DevCsr dA, dAt;
        double* db = nullptr;
        tmp.what = what;
        if ((rc = dAt.upload(tmp, At, stream)) != FOS_OK || (rc = dA.upload(tmp, A, stream)) != FOS_OK || (rc = tmp.upload(&db, b, (size_t)m, stream)) != FOS_OK) return fail(rc);
        DEV_HIP(a, hipMemsetAsync(w.B0, 0, sizeof(double) * (size_t)a->L * (size_t)a->L, stream));
        hipLaunchKernelGGL(ns_rowdot_csr_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, 4096)), dim3(NS_T), 0, stream, n, (const int32_t*)dAt.rp, (const int32_t*)dAt.ci,
                           (const double*)dAt.va, (const double*)db, lambda, a->r);
        launch_sf_gram(stream, n, a->L, dAt.rp, dAt.ci, dAt.va, dA.rp, dA.ci, dA.va, w.B0);       // A'A = B B', B = A': its CSR is A's CSC, the CSR of B' is A's
        if ((rc = ns_build(a, factor, stream, "I + lambda A'A", w, NsSource{0, w.B0, lambda})) != FOS_OK) return fail(rc);
    }
    *out = a;
    return FOS_OK;
}

namespace {
void ns_product(const NSpace* a, hipStream_t s, const double* tiles, const NsVec& op, int mode, const NsVec& w, double* out) {
    const int nunits = a->rK.nunits, per = NS_T / 64;
    hipLaunchKernelGGL(ns_symv_kernel, dim3((unsigned)((nunits + per - 1) / per)), dim3(NS_T), 0, s, (const RedUnit*)a->units, nunits, tiles, op, a->rowslot, a->colslot);
    hipLaunchKernelGGL(ns_fold_kernel, dim3((unsigned)a->rK.nt), dim3(64 * NS_FOLD_WAVES), 0, s, (const double*)a->rowslot, (const double*)a->colslot,
                       (const int32_t*)a->strip_u0, mode, w, (const double*)a->z, out);
}
}  // namespace

// y = prox_f(x) (device vectors of at least n doubles), on `stream`: NS_LAUNCHES launches, nothing else
int NSpace::prox(hipStream_t stream, double* y, const double* x) {
    const NSpace* a = this;
    const NsVec w{x, a->D, a->ct, a->n};
    ns_product(a, stream, a->tilesK, w, 0, w, a->z);                                       // z = K w
    ns_product(a, stream, a->tilesM, NsVec{a->z, nullptr, nullptr, a->L}, 1, w, a->r);     // r = w - Mt z
    ns_product(a, stream, a->tilesK, NsVec{a->r, nullptr, nullptr, a->L}, 2, w, y);        // y = D (z + K r)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: a kernel launch failed: %s", a->what, hipGetErrorString(e)); return FOS_EHIP; }
    return FOS_OK;
}

// out8 = n, m (0: Quadratic), factor that produced the accepted inverse, fell_back, probe residual, kernel launches per prox, bytes kept, tiles of one stream
void nspace_stats(const ProxObject* obj, double* out8) {
    const NSpace* a = static_cast<const NSpace*>(obj);
    out8[0] = (double)a->n; out8[1] = (double)a->m; out8[2] = (double)a->inv.used; out8[3] = a->inv.fell_back ? 1.0 : 0.0; out8[4] = a->inv.probe;
    out8[5] = (double)NS_LAUNCHES; out8[6] = (double)a->bytes; out8[7] = (double)a->plan.ntiles;
}

// the one-rhs product alone, for measurements: a symmetric test matrix of order k is generated and packed on the device, then y = X v is timed `reps` times through
// ns_symv_kernel + ns_fold_kernel and through red_symm_kernel + red_fold_kernel (direct_reduced.hip) on the SAME tiles with a zero second right-hand side.
// out4 = milliseconds per product (one-rhs), milliseconds per product (two-rhs kernel), bytes of the tile stream, max |difference| of the two results
namespace {
__global__ __launch_bounds__(NS_T) void ns_bench_fill_kernel(int64_t k, int64_t L, double* __restrict__ X, double* __restrict__ v, double2* __restrict__ pq) {
    for (int64_t e = blockIdx.x * (int64_t)NS_T + threadIdx.x; e < L * L; e += (int64_t)gridDim.x * NS_T) {
        const int64_t i = e % L, j = e / L, hi = i > j ? i : j, lo = i > j ? j : i;
        X[e] = (i < k && j < k) ? cos(0.37 * (double)hi + 1.3 * (double)lo) / (1.0 + (double)(hi - lo)) : 0.0;
        if (j == 0) { const double vi = i < k ? sin(0.11 * (double)i + 0.5) : 0.0; v[i] = vi; pq[i] = make_double2(vi, 0.0); }
    }
}
__global__ __launch_bounds__(NS_T) void ns_bench_diff_kernel(int64_t k, const double* __restrict__ y1, const double2* __restrict__ y2, double* __restrict__ out) {
    double d = 0.0;                                                // (one workgroup)
    for (int64_t i = threadIdx.x; i < k; i += NS_T) d = fmax(d, fabs(y1[i] - y2[i].x));
    __shared__ double sm[NS_T];
    sm[threadIdx.x] = d;
    __syncthreads();
    if (threadIdx.x == 0) { for (int t = 1; t < NS_T; ++t) d = fmax(d, sm[t]); *out = d; }
}
}  // namespace
int nspace_bench_symv(int64_t k, int reps, hipStream_t stream, double* out4) {
    if (k < 1 || k > NS_MAX_N || reps < 1 || !out4) { set_error("fos_bench_symv_packed: bad argument (1 <= k <= %lld, reps >= 1)", (long long)NS_MAX_N); return FOS_EINVAL; }
    NSpace* a = new NSpace();
    a->what = "fos_bench_symv_packed";
    a->n = k; a->L = (k + 63) / 64 * 64;
    build_reduced_plan(k, &a->plan);
    const RedPlan& P = a->plan;
    const size_t L = (size_t)a->L;
    int rc = FOS_OK;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto done = [&](int code) { (void)hipStreamSynchronize(stream); for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); delete a; return code; };
    double *X = nullptr, *v = nullptr, *col2 = nullptr, *dd = nullptr;
    double2 *pq = nullptr, *y2 = nullptr, *row2 = nullptr;
    if ((rc = a->alloc(&a->units, P.units.size())) != FOS_OK || (rc = a->alloc(&a->strip_u0, P.strip_u0.size())) != FOS_OK ||
        (rc = a->alloc(&a->tilesK, (size_t)P.ntiles * RED_TILE)) != FOS_OK || (rc = a->alloc(&a->rowslot, (size_t)P.ntiles * 64)) != FOS_OK ||
        (rc = a->alloc(&a->colslot, P.units.size() * RED_TC)) != FOS_OK || (rc = a->alloc(&a->z, L)) != FOS_OK ||
        (rc = a->alloc(&X, L * L)) != FOS_OK || (rc = a->alloc(&v, L)) != FOS_OK || (rc = a->alloc(&pq, L)) != FOS_OK || (rc = a->alloc(&y2, L)) != FOS_OK ||
        (rc = a->alloc(&row2, (size_t)P.ntiles * 64)) != FOS_OK || (rc = a->alloc(&col2, P.units.size() * 64)) != FOS_OK || (rc = a->alloc(&dd, 1)) != FOS_OK)
        return done(rc);
    RedDev R{};
    R.k = k; R.kpad = a->L; R.nt = P.nt; R.nunits = (int)P.units.size(); R.units = a->units; R.strip_u0 = a->strip_u0; R.tiles = a->tilesK;
    R.rowslot = row2; R.colslot = col2;
    a->rK = R;
    if ((rc = a->hip("hipMemcpyAsync", hipMemcpyAsync(a->units, P.units.data(), sizeof(RedUnit) * P.units.size(), hipMemcpyHostToDevice, stream))) != FOS_OK ||
        (rc = a->hip("hipMemcpyAsync", hipMemcpyAsync(a->strip_u0, P.strip_u0.data(), sizeof(int32_t) * P.strip_u0.size(), hipMemcpyHostToDevice, stream))) != FOS_OK)
        return done(rc);
    for (hipEvent_t& e : ev) if ((rc = a->hip("hipEventCreate", hipEventCreate(&e))) != FOS_OK) return done(rc);
    LaunchCtx c{};
    c.stream = stream; c.l = k;
    hipLaunchKernelGGL(ns_bench_fill_kernel, dim3(ns_grid((int64_t)(L * L))), dim3(NS_T), 0, stream, k, a->L, X, v, pq);
    launch_red_pack_tiles(c, R, a->L, X);
    const NsVec op{v, nullptr, nullptr, k};
    ns_product(a, stream, a->tilesK, op, 0, op, a->z);                                     // warm-up of both
    launch_red_symm(c, R, pq, y2);
    (void)hipEventRecord(ev[0], stream);
    for (int i = 0; i < reps; ++i) ns_product(a, stream, a->tilesK, op, 0, op, a->z);
    (void)hipEventRecord(ev[1], stream);
    for (int i = 0; i < reps; ++i) launch_red_symm(c, R, pq, y2);
    (void)hipEventRecord(ev[2], stream);
    hipLaunchKernelGGL(ns_bench_diff_kernel, dim3(1), dim3(NS_T), 0, stream, k, (const double*)a->z, (const double2*)y2, dd);
    double diff = 0.0;
    if ((rc = a->hip("hipMemcpyAsync", hipMemcpyAsync(&diff, dd, sizeof(double), hipMemcpyDeviceToHost, stream))) != FOS_OK ||
        (rc = a->hip("hipStreamSynchronize", hipStreamSynchronize(stream))) != FOS_OK)
        return done(rc);
    float ms1 = 0.f, ms2 = 0.f;
    (void)hipEventElapsedTime(&ms1, ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms2, ev[1], ev[2]);
    out4[0] = (double)ms1 / reps; out4[1] = (double)ms2 / reps; out4[2] = (double)P.ntiles * RED_TILE * 8.0; out4[3] = diff;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: a kernel launch failed: %s", a->what, hipGetErrorString(e)); return done(FOS_EHIP); }
    return done(FOS_OK);
}

// ---------------------------------------------------------------------------------- host emulation (tests; no GPU)
// y = X v over the packed tiles in ns_symv_kernel's and ns_fold_kernel's order (slots, the lanes' crossing, the fold); v, y: kpad doubles
void host_nspace_symv(const RedPlan& P, const std::vector<double>& tiles, const double* v, double* y) {
    std::vector<double> rowslot((size_t)P.ntiles * 64, 0.0), colslot(P.units.size() * RED_TC, 0.0);
    for (size_t un = 0; un < P.units.size(); ++un) {
        const RedUnit& u = P.units[un];
        std::vector<double> ca((size_t)64 * 32, 0.0);            // [lane][column]
        for (int I = u.i0; I < u.i1; ++I) {
            const double* t = tiles.data() + (size_t)(u.tile0 + (I - u.i0)) * RED_TILE;
            for (int lane = 0; lane < 64; ++lane) {
                const double xi = (I == u.j / 2) ? 0.0 : v[(int64_t)RED_TR * I + lane];
                double ry = 0.0;
                for (int c = 0; c < RED_TC; ++c) {
                    const double e = t[128 * (c >> 1) + 2 * lane + (c & 1)];
                    ry = std::fma(e, v[(int64_t)RED_TC * u.j + c], ry);        // (the device compiler fuses every multiply-add of the tile loop)
                    ca[(size_t)lane * 32 + c] = std::fma(e, xi, ca[(size_t)lane * 32 + c]);
                }
                rowslot[(size_t)(((int64_t)I * (I + 1) + u.j) * 64 + lane)] = ry;
            }
        }
        for (int half = 16; half >= 1; half >>= 1) {
            std::vector<double> nx((size_t)64 * 32, 0.0);
            for (int lane = 0; lane < 64; ++lane) {
                const bool up = (lane & half) != 0;
                const int other = lane ^ half;
                for (int i = 0; i < half; ++i) {
                    const double keep = up ? ca[(size_t)lane * 32 + i + half] : ca[(size_t)lane * 32 + i];
                    const double got = up ? ca[(size_t)other * 32 + i + half] : ca[(size_t)other * 32 + i];      // what the partner sends: the half IT does not keep
                    nx[(size_t)lane * 32 + i] = keep + got;
                }
            }
            ca.swap(nx);
        }
        for (int lane = 0; lane < RED_TC; ++lane) colslot[un * RED_TC + lane] = ca[(size_t)lane * 32] + ca[(size_t)(lane + 32) * 32];
    }
    for (int I = 0; I < P.nt; ++I)
        for (int r = 0; r < 64; ++r) {
            double part[NS_FOLD_WAVES];
            for (int w = 0; w < NS_FOLD_WAVES; ++w) {
                part[w] = 0.0;
                for (int jj = w; jj < 2 * I + 2; jj += NS_FOLD_WAVES) part[w] += rowslot[(size_t)(((int64_t)I * (I + 1) + jj) * 64 + r)];
            }
            double s = part[0];
            for (int w = 1; w < NS_FOLD_WAVES; ++w) s += part[w];
            const int j = 2 * I + (r >> 5), c = r & 31;
            for (int u = P.strip_u0[j]; u < P.strip_u0[j + 1]; ++u) s += colslot[(size_t)u * RED_TC + c];
            y[(int64_t)RED_TR * I + r] = s;
        }
}

namespace {
// Every multiply-add below rounds ONCE (std::fma), k ascending, as the device's contracted code and its fp64 matrix-core products do: on instances that amplify a
// last-bit difference of Mt or K by 1e5 (a rank-deficient A at lambda = 1e3) the emulation agrees with the device only because it is exact to the bit.
// from S = the lower triangle of Q or of A'A (column-major n x n, entries (i, j), i >= j) and c: scaling, the inverse by host_chol_inverse accepted by the probe
// of dense_spd_inverse at NS_BAR, both tile streams and the three products with their epilogues
int ns_host_prox(const char* what, const char* gname, int64_t n, const std::vector<double>& S, double lambda, const std::vector<double>& c, const double* x, double* y) {
    std::vector<double> D((size_t)n), Mt((size_t)n * (size_t)n), K((size_t)n * (size_t)n);
    for (int64_t i = 0; i < n; ++i) D[(size_t)i] = 1.0 / std::sqrt(std::fma(lambda, S[(size_t)(i + i * n)], 1.0));      // (the fused forms of ns_diag_kernel and ns_scale_kernel)
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j; i < n; ++i) {
            const double v = D[(size_t)i] * (std::fma(lambda, S[(size_t)(i + j * n)], i == j ? 1.0 : 0.0) * D[(size_t)j]);
            Mt[(size_t)(i + j * n)] = v; Mt[(size_t)(j + i * n)] = v;
        }
    const int64_t bad = host_chol_inverse(n, Mt.data(), K.data(), true);
    if (bad >= 0) {
        set_error("%s: Cholesky factorisation of %s: the pivot of column %lld is not a positive finite number (the matrix is not positive definite)", what, gname, (long long)bad);
        return FOS_EINVAL;
    }
    RedPlan P;
    build_reduced_plan(n, &P);
    std::vector<double> tM, tK;
    host_reduced_pack(P, Mt.data(), &tM, nullptr);
    host_reduced_pack(P, K.data(), &tK, nullptr);
    const size_t L = (size_t)P.nt * RED_TR;
    std::vector<double> w(L, 0.0), z(L, 0.0), r(L, 0.0), s(L, 0.0);
    {   // the probe (the product in the tiles' order instead of dense_symv_kernel's: the bar is five orders above either's rounding)
        std::vector<double> v((size_t)n);
        double probe = 0.0;
        for (int j = 0; j < 4; ++j) {
            direct_test_vector(n, j, v);
            std::fill(w.begin(), w.end(), 0.0);
            std::copy(v.begin(), v.end(), w.begin());
            host_nspace_symv(P, tK, w.data(), z.data());
            host_nspace_symv(P, tM, z.data(), s.data());
            double dmax = 0.0, nv = 0.0;
            for (int64_t i = 0; i < n; ++i) { const double e = std::fabs(s[(size_t)i] - v[(size_t)i]); dmax = (e > dmax || e != e) ? e : dmax; nv = std::max(nv, std::fabs(v[(size_t)i])); }
            dmax /= nv;
            probe = (dmax > probe || dmax != dmax) ? dmax : probe;
        }
        if (!(probe <= NS_BAR)) { set_error("%s: the inverse of %s was not accepted (probe residual %.3e)", what, gname, probe); return FOS_EINVAL; }
    }
    std::fill(w.begin(), w.end(), 0.0);
    for (int64_t i = 0; i < n; ++i) w[(size_t)i] = std::fma(D[(size_t)i], x[i], D[(size_t)i] * c[(size_t)i]);
    host_nspace_symv(P, tK, w.data(), z.data());                                  // z = K w
    host_nspace_symv(P, tM, z.data(), s.data());
    for (size_t i = 0; i < L; ++i) r[i] = w[i] - s[i];                            // r = w - Mt z
    host_nspace_symv(P, tK, r.data(), s.data());
    for (int64_t i = 0; i < n; ++i) y[i] = D[(size_t)i] * (z[(size_t)i] + s[(size_t)i]);      // y = D (z + K r)
    return FOS_OK;
}
}  // namespace

int host_nspace_quadratic(int64_t n, const double* Q, const double* q, const double* x, double* y) {
    FOS_TRY(ns_check_common("Quadratic", n, FOS_DIRECT_FACTOR_CHOLESKY));
    if (!x || !y) { set_error("Quadratic: bad argument"); return FOS_EINVAL; }
    FOS_TRY(ns_check_quadratic(n, Q, q));
    std::vector<double> S((size_t)n * (size_t)n, 0.0), c((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j <= i; ++j) S[(size_t)(i + j * n)] = Q[i * n + j];
        c[(size_t)i] = -q[i];
    }
    return ns_host_prox("Quadratic", "I + Q", n, S, 1.0, c, x, y);
}
int host_nspace_ls_dense(int64_t m, int64_t n, const double* A, const double* b, double lambda, const double* x, double* y) {
    const char* what = "LeastSquares (normal)";
    FOS_TRY(ns_check_lambda(lambda));
    FOS_TRY(ns_check_common(what, n, FOS_DIRECT_FACTOR_CHOLESKY));
    if (m < 1 || !A || !b || !x || !y) { set_error("%s: bad argument (m >= 1)", what); return FOS_EINVAL; }
    if (!ns_finite(A, m * n)) { set_error("%s: A has non-finite entries", what); return FOS_EINVAL; }
    if (!ns_finite(b, m)) { set_error("%s: b has non-finite entries", what); return FOS_EINVAL; }
    std::vector<double> At((size_t)n * (size_t)m), S((size_t)n * (size_t)n, 0.0), c((size_t)n);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < n; ++j) At[(size_t)(j * m + i)] = A[i * n + j];
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            double s = 0.0;
            const double *ri = At.data() + i * m, *rj = At.data() + j * m;
            for (int64_t k = 0; k < m; ++k) s = std::fma(ri[k], rj[k], s);          // gram_rows_kernel: k ascending, every product fused into the sum
            S[(size_t)(i + j * n)] = s;
        }
    for (int64_t j = 0; j < n; ++j) {                                             // ns_rowdot_kernel: lane-strided, then the wave's tree
        double lane[64] = {0.0};
        for (int64_t i = 0; i < m; ++i) lane[i % 64] = std::fma(At[(size_t)(j * m + i)], b[i], lane[i % 64]);      // (fused on the device)
        c[(size_t)j] = lambda * host_da_wave(lane);
    }
    return ns_host_prox(what, "I + lambda A'A", n, S, lambda, c, x, y);
}
int host_nspace_ls_sparse(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, const double* x,
                          double* y) {
    const char* what = "LeastSquares (sparse, normal)";
    FOS_TRY(ns_check_lambda(lambda));
    FOS_TRY(ns_check_common(what, n, FOS_DIRECT_FACTOR_CHOLESKY));
    if (!x || !y) { set_error("%s: bad argument", what); return FOS_EINVAL; }
    HostCsr A, At;
    FOS_TRY(ns_sparse_rows(m, n, colptr, rowval, nzval, b, &A, &At));
    std::vector<double> S((size_t)n * (size_t)n, 0.0), c((size_t)n);
    for (int64_t i = 0; i < n; ++i)                                               // sf_gram_kernel on B = A': column i of the result, the entries of row i of B in order
        for (int32_t e = At.rp[(size_t)i]; e < At.rp[(size_t)i + 1]; ++e) {
            const int32_t row = At.ci[(size_t)e];
            for (int32_t t = A.rp[(size_t)row]; t < A.rp[(size_t)row + 1]; ++t) {
                double& g = S[(size_t)(A.ci[(size_t)t] + i * n)];
                g = std::fma(At.va[(size_t)e], A.va[(size_t)t], g);                   // (fused on the device)
            }
        }
    for (int64_t j = 0; j < n; ++j) {
        double lane[64] = {0.0};
        for (int32_t e = At.rp[(size_t)j]; e < At.rp[(size_t)j + 1]; ++e) {
            double& l = lane[(e - At.rp[(size_t)j]) % 64];
            l = std::fma(At.va[(size_t)e], b[At.ci[(size_t)e]], l);                   // (fused on the device)
        }
        c[(size_t)j] = lambda * host_da_wave(lane);
    }
    return ns_host_prox(what, "I + lambda A'A", n, S, lambda, c, x, y);
}
// packs the symmetric column-major k x k matrix X as the device does and multiplies: y = X v in the kernels' order; `count` as host_reduced_pack's
int host_nspace_symv_packed(int64_t k, const double* X, const double* v, double* y, int32_t* count) {
    if (k < 1 || k > NS_MAX_N || !X || !v || !y) { set_error("fos_host_symv_packed: bad argument (1 <= k <= %lld)", (long long)NS_MAX_N); return FOS_EINVAL; }
    RedPlan P;
    build_reduced_plan(k, &P);
    std::vector<double> tiles;
    host_reduced_pack(P, X, &tiles, count);
    const size_t L = (size_t)P.nt * RED_TR;
    std::vector<double> vp(L, 0.0), yp(L, 0.0);
    std::copy(v, v + k, vp.begin());
    host_nspace_symv(P, tiles, vp.data(), yp.data());
    std::copy(yp.begin(), yp.begin() + k, y);
    return FOS_OK;
}

}  // namespace fos
