// Device side of an equilibrated handle (fos_create3, equil_passes > 0): the handle solves the scaled problem A^ = D A E, b^ = sigma D b,
// c^ = rho E c; these three kernels are where the caller's units meet it.
//   eq_status        the six sums of checkstatus (HSDEStatus.jl:34-38,59,61) ON THE CALLER'S A, b, c, formed from the scaled iterate and w = Q^ [x^; y^; 0]
//   eq_interleave    fos_set_iterate / fos_check: plain z in the caller's units -> interleaved scaled iterate
//   eq_deinterleave  fos_get_iterate / fos_get_checked / fos_getsol: the way back
// All three are streams over l = n + m + 1 elements.  The sums have a fixed order (lane -> wavefront -> workgroup -> the records in
// index order) and use no atomics: a check gives the same bits on every run.
//
// FP contraction is OFF: the residual terms are differences of nearly equal numbers at an optimal point, and the (de)interleave pair
// must round the same way in both directions.
#include "dev_common.hpp"

#pragma clang fp contract(off)

namespace fos {

constexpr int EQ_FIN_THREADS = 1024;

// w: plain l-vector, rows 0 .. n+m-1 of Q^ [x^; y^; 0] -- w_x = A^'y^, w_y = -A^ x^ (launch_q1, Q_PLAIN_NOTAU: the tau entry taken as zero, so that
// no c^ tau or b^ tau is added here only to be subtracted again: at a large tau that cost ||A x + s|| and ||A'y|| their digits); cb = [c^; b^];
// inv = [1 ./ E; 1 ./ D].  With x = E x^ / sigma, y = D y^ / rho, r = r^ / (rho E), s = s^ / (sigma D), b = D^-1 b^ / sigma, c = E^-1 c^ / rho:
//   A x + s           = D^-1 (s^ - w_y) / sigma                        A'y               = E^-1 w_x / rho
//   (A x + s)/tau - b = D^-1 ((-w_y / tau + s^ / tau) - b^) / sigma     (A'y - r)/tau + c = E^-1 ((w_x / tau + c^) - r^ / tau) / rho
// term by term the reference's A x / tau + s / tau - b and A'y / tau + c - r / tau (HSDEStatus.jl:34-35), each row times a positive factor: at tau = 0
// a row is +-Inf or NaN exactly where the reference's is, so p and d carry its Inf / NaN pattern; tau < 0 enters with its sign, as there.
// The scalars sigma and rho are applied by the host (solver.cpp eq_status_check).  Records: partials[block][6] in StatusIdx order.
__global__ __launch_bounds__(EQ_THREADS) void eq_status_kernel(int64_t n, int64_t nm, const d2* __restrict__ z, const double* __restrict__ w,
                                                               const double* __restrict__ cb, const double* __restrict__ inv,
                                                               double* __restrict__ partials) {
    __shared__ double smem[(EQ_THREADS / 64) * 6];
    const double tau = z[nm].x;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * (int64_t)EQ_THREADS + threadIdx.x; i < nm; i += (int64_t)gridDim.x * EQ_THREADS) {
        const d2 zi = z[i];
        const double wi = w[i], c = cb[i], e = inv[i];
        if (i < n) {                       // zi = (x^_i, r^_i), c = c^_i, e = 1 / E_i
            const double rd = e * ((wi / tau + c) - zi.y / tau);
            const double aty = e * wi;
            acc[ST_RD2] += rd * rd;
            acc[ST_ATY2] += aty * aty;
            acc[ST_CTX] += c * zi.x;
        } else {                           // zi = (y^_j, s^_j), c = b^_j, e = 1 / D_j
            const double rp = e * ((zi.y / tau - wi / tau) - c);
            const double axs = e * (zi.y - wi);
            acc[ST_RP2] += rp * rp;
            acc[ST_AXS2] += axs * axs;
            acc[ST_BTY] += c * zi.x;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double v = wave_sum(acc[a]);
        if (lane == 0) smem[wave * 6 + a] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double s = 0.0;
        for (int k = 0; k < EQ_THREADS / 64; ++k) s += smem[k * 6 + threadIdx.x];
        partials[6 * (int64_t)blockIdx.x + threadIdx.x] = s;
    }
}

// the records in index order -> DevState.stat, tau^ and kappa^ appended (as status_finalize_kernel does for a plain handle)
__global__ __launch_bounds__(EQ_FIN_THREADS) void eq_status_finalize_kernel(const double* __restrict__ partials, int count, const d2* __restrict__ z,
                                                                            int64_t nm, DevState* st) {
    __shared__ double sums[6];
    reduce_partials<6>(partials, count, sums);
    if (threadIdx.x < 6) st->stat[threadIdx.x] = sums[threadIdx.x];
    if (threadIdx.x == 0) { st->stat[ST_TAU] = z[nm].x; st->stat[ST_KAPPA] = z[nm].y; }
}

// up[i] = what takes element i of the caller's (part 1, part 2) to the scaled problem's:
//   i < n: (sigma / E_i, rho E_i)    n <= i < n+m: (rho / D_j, sigma D_j)    i = n+m: (1, sigma rho)
// The way back DIVIDES by the same numbers, so that a round trip costs two roundings per entry, not four.
__global__ __launch_bounds__(EQ_THREADS) void eq_interleave_kernel(int64_t l, d2* __restrict__ out, const double* __restrict__ plain,
                                                                   const d2* __restrict__ up) {
    for (int64_t i = blockIdx.x * (int64_t)EQ_THREADS + threadIdx.x; i < l; i += (int64_t)gridDim.x * EQ_THREADS) {
        const d2 u = up[i];
        out[i] = make_double2(plain[i] * u.x, plain[l + i] * u.y);
    }
}
__global__ __launch_bounds__(EQ_THREADS) void eq_deinterleave_kernel(int64_t l, double* __restrict__ plain, const d2* __restrict__ in,
                                                                     const d2* __restrict__ up) {
    for (int64_t i = blockIdx.x * (int64_t)EQ_THREADS + threadIdx.x; i < l; i += (int64_t)gridDim.x * EQ_THREADS) {
        const d2 u = up[i], v = in[i];
        plain[i] = v.x / u.x;
        plain[l + i] = v.y / u.y;
    }
}

void launch_eq_status(const LaunchCtx& c, const double2* z, const double* w, const double* cb, const double* inv, double* partials) {
    const int blocks = eq_blocks(c.n + c.m);
    hipLaunchKernelGGL(eq_status_kernel, dim3(blocks), dim3(EQ_THREADS), 0, c.stream, c.n, c.n + c.m, z, w, cb, inv, partials);
    hipLaunchKernelGGL(eq_status_finalize_kernel, dim3(1), dim3(EQ_FIN_THREADS), 0, c.stream, partials, blocks, z, c.n + c.m, c.st);
}
void launch_eq_interleave(const LaunchCtx& c, double2* out, const double* plain, const double2* up) {
    hipLaunchKernelGGL(eq_interleave_kernel, dim3(eq_blocks(c.l)), dim3(EQ_THREADS), 0, c.stream, c.l, out, plain, up);
}
void launch_eq_deinterleave(const LaunchCtx& c, double* plain, const double2* in, const double2* up) {
    hipLaunchKernelGGL(eq_deinterleave_kernel, dim3(eq_blocks(c.l)), dim3(EQ_THREADS), 0, c.stream, c.l, plain, in, up);
}

}  // namespace fos
