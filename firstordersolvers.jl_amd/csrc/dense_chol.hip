// direct = true (HSDE.jl:12-15), set-up: the inverse of a dense symmetric positive definite G (I + Q Q' of the dense form, K = I + A'A or I + A A' of the reduced
// form) through a blocked Cholesky factorisation instead of the Newton-Schulz iteration -- about k^3 flops instead of 62 k^3.
//   G = L L'          left-looking by block columns of 64: tile (i, j) = G_ij - sum_{p<j} L_ip L_jp' (written once), the diagonal block factored in LDS by one
//                     workgroup that also writes L_jj^-1, the panel L_ij = T_ij L_jj^-T as one 64 x 64 x 64 product per tile;
//   W = L^-1          by block rows: W_ii = L_ii^-1 (already there), W_ij = -L_ii^-1 sum_{j<=p<i} L_ip W_pj;
//   X = W'W           lower triangle, mirrored into the upper in the same store: X is exactly symmetric.
// All products run on v_mfma_f64_16x16x4_f64 with the register maps of dense_gemm_kernel (vecops.hip): one 64 x 64 tile per workgroup, each of the 4 wavefronts
// a 32 x 32 quadrant.  Matrices are column-major with leading dimension L (a multiple of 64; padding rows / columns of G: identity, so L and W carry it too).
// Every sum runs in a fixed order and nothing is atomic: two runs on the same G give the same bits.  Only lower tiles of Lw and Ww are ever read or written.
// A non-positive or non-finite pivot stores (column + 1) in *info (an ordinary store; the launches are serial on one stream, so it is the FIRST such column);
// every later kernel of the chain returns at once when *info != 0.
#include "fos_internal.hpp"
#include "dev_common.hpp"

#include <cfloat>
#include <cmath>
#include <vector>

namespace fos {

namespace {
constexpr int CH_T = 256;            // threads per workgroup
constexpr int CH_B = 64;             // block order
constexpr int CH_KC = 32;            // K per staged chunk
constexpr int CH_LDX = 80;           // LDS row stride of an operand staged [k][x]: 160 dwords = 32 mod 64, the two k of a 32-lane half on disjoint banks
constexpr int CH_LDK = 34;           // LDS row stride of an operand staged [x][k]: 68 dwords, 4 x + 2 k distinct over a 32-lane half
constexpr int CH_OP = CH_KC * CH_LDX;                // doubles per staged operand (>= 64 * CH_LDK)
static_assert(CH_OP >= CH_B * CH_LDK, "operand stage too small");
static_assert(2 * CH_OP >= CH_B * CH_LDX, "a whole 64 x 64 tile must fit the two stages");
typedef double ch_v4d __attribute__((ext_vector_type(4)));

// An operand is a 64 x K matrix E(x, k).  KM = false: E(x, k) = P[x + k ld] (x contiguous), staged [k][x];  KM = true: E(x, k) = P[k + x ld] (k contiguous), staged [x][k].
// GUARD (KM only): rows x >= nx of the operand are not read and count as zero.
template <bool KM, bool GUARD = false> __device__ __forceinline__ void ch_fetch(double (&r)[8], const double* __restrict__ P, size_t ld, int tid, int nx = CH_B) {
    if (!KM) {
        const int x = tid & 63, k = tid >> 6;
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = P[(size_t)x + (size_t)(k + 4 * q) * ld];
    } else {
        const int k = tid & 31, x = tid >> 5;
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = (!GUARD || x + 8 * q < nx) ? P[(size_t)k + (size_t)(x + 8 * q) * ld] : 0.0;
    }
}
template <bool KM> __device__ __forceinline__ void ch_stash(const double (&r)[8], double* __restrict__ S, int tid) {
    if (!KM) {
        const int x = tid & 63, k = tid >> 6;
#pragma unroll
        for (int q = 0; q < 8; ++q) S[(k + 4 * q) * CH_LDX + x] = r[q];
    } else {
        const int k = tid & 31, x = tid >> 5;
#pragma unroll
        for (int q = 0; q < 8; ++q) S[(x + 8 * q) * CH_LDK + k] = r[q];
    }
}
template <bool KM> __device__ __forceinline__ double ch_frag(const double* __restrict__ S, int x, int k) { return KM ? S[x * CH_LDK + k] : S[k * CH_LDX + x]; }

// acc += A B over K (a multiple of CH_KC): A(i, k) and B(j, k) given as operands above (the product is sum_k A(i, k) B(j, k)).  The next chunk's global loads are
// issued before the current chunk's MFMAs: with about one workgroup per CU in the panel chain nothing else hides their latency.  Ends behind a barrier.
template <bool KA, bool KB, bool GUARD = false>
__device__ __forceinline__ void ch_tile_mma(ch_v4d (&acc)[2][2], const double* __restrict__ A, size_t lda, const double* __restrict__ B, size_t ldb, int K, double* sh,
                                            int na = CH_B, int nb = CH_B) {
    if (K <= 0) return;
    double* As = sh;
    double* Bs = sh + CH_OP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = (wv >> 1) * 32, wc = (wv & 1) * 32, lr = lane & 15, lk = lane >> 4;
    double ra[8], rb[8];
    ch_fetch<KA, GUARD>(ra, A, lda, tid, na);
    ch_fetch<KB, GUARD>(rb, B, ldb, tid, nb);
    for (int k0 = 0; k0 < K; k0 += CH_KC) {
        ch_stash<KA>(ra, As, tid);
        ch_stash<KB>(rb, Bs, tid);
        __syncthreads();
        if (k0 + CH_KC < K) {
            A += KA ? (size_t)CH_KC : (size_t)CH_KC * lda;
            B += KB ? (size_t)CH_KC : (size_t)CH_KC * ldb;
            ch_fetch<KA, GUARD>(ra, A, lda, tid, na);
            ch_fetch<KB, GUARD>(rb, B, ldb, tid, nb);
        }
#pragma unroll
        for (int ks = 0; ks < CH_KC; ks += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = ch_frag<KA>(As, wr + 16 * a + lr, ks + lk);
#pragma unroll
            for (int b = 0; b < 2; ++b) bv[b] = ch_frag<KB>(Bs, wc + 16 * b + lr, ks + lk);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
}
__device__ __forceinline__ void ch_zero(ch_v4d (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ch_v4d{0.0, 0.0, 0.0, 0.0};
}
// result map of the f64 MFMA: column lane & 15, rows (lane >> 4) + 4 r.  f(row, col, value) for the 16 results of this thread
template <class F> __device__ __forceinline__ void ch_for_result(const ch_v4d (&acc)[2][2], F&& f) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = (wv >> 1) * 32, wc = (wv & 1) * 32, lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) f(wr + 16 * a + lk + 4 * r, wc + 16 * b + lr, acc[a][b][r]);
}

// (1) block column j, tiles i = j .. nb-1:  Lw_ij = G_ij - sum_{p<j} L_ip L_jp'
__global__ __launch_bounds__(CH_T) void chol_update_kernel(int64_t L, int j, const double* __restrict__ G, double* __restrict__ Lw, const int32_t* __restrict__ info) {
    __shared__ double sh[2 * CH_OP];
    if (*info != 0) return;
    const size_t i0 = (size_t)(j + blockIdx.x) * CH_B, j0 = (size_t)j * CH_B;
    ch_v4d acc[2][2];
    ch_zero(acc);
    ch_tile_mma<false, false>(acc, Lw + i0, (size_t)L, Lw + j0, (size_t)L, j * CH_B, sh);
    ch_for_result(acc, [&](int row, int col, double v) {
        const size_t idx = (i0 + row) + (j0 + col) * (size_t)L;
        Lw[idx] = G[idx] - v;
    });
}

// (2) the diagonal block of column j: T_jj = L_jj L_jj' in LDS (column by column, lower triangle), L_jj back to Lw (upper part zero), L_jj^-1 to the diagonal
// tile of Ww (upper part zero).  One workgroup.
__global__ __launch_bounds__(CH_T) void chol_diag_kernel(int64_t L, int j, double* __restrict__ Lw, double* __restrict__ Ww, int32_t* __restrict__ info) {
    __shared__ double Sc[CH_B * CH_B];           // Sc[c * 64 + i] = T(i, c), later L_jj(i, c)
    __shared__ double Xi[CH_B * CH_B];           // Xi[i * 64 + c] = L_jj^-1 (i, c)
    if (*info != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t j0 = (size_t)j * CH_B;
    double* __restrict__ T = Lw + j0 + j0 * (size_t)L;
    for (int q = 0; q < 16; ++q) { const int c = wv + 4 * q; Sc[c * CH_B + lane] = T[(size_t)lane + (size_t)c * L]; }
    for (int c = 0; c < CH_B; ++c) {
        __syncthreads();
        const double d = Sc[c * CH_B + c];
        if (!(d > 0.0) || !(d <= DBL_MAX)) {     // the same value in every thread: the whole workgroup leaves
            if (tid == 0) *info = (int32_t)(j0 + c + 1);
            return;
        }
        const double rt = sqrt(d);
        __syncthreads();
        if (wv == 0 && lane >= c) Sc[c * CH_B + lane] = lane == c ? rt : Sc[c * CH_B + lane] / rt;
        __syncthreads();
        for (int jj = c + 1 + wv; jj < CH_B; jj += 4)
            if (lane >= jj) Sc[jj * CH_B + lane] -= Sc[c * CH_B + lane] * Sc[c * CH_B + jj];
    }
    __syncthreads();
    if (wv == 0) {                               // column `lane` of the inverse by forward substitution
        const int c = lane;
        for (int i = 0; i < CH_B; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int p = c; p < i; ++p) s -= Sc[p * CH_B + i] * Xi[p * CH_B + c];
            Xi[i * CH_B + c] = i < c ? 0.0 : s / Sc[i * CH_B + i];
        }
    }
    __syncthreads();
    double* __restrict__ Wd = Ww + j0 + j0 * (size_t)L;
    for (int q = 0; q < 16; ++q) {
        const int c = wv + 4 * q;
        T[(size_t)lane + (size_t)c * L] = lane >= c ? Sc[c * CH_B + lane] : 0.0;
        Wd[(size_t)lane + (size_t)c * L] = Xi[lane * CH_B + c];
    }
}

// (3) the panel of column j, tiles i = j+1 .. nb-1:  L_ij = T_ij L_jj^-T  (in place: every load of the tile precedes the first store)
__global__ __launch_bounds__(CH_T) void chol_panel_kernel(int64_t L, int j, double* Lw, const double* __restrict__ Ww, const int32_t* __restrict__ info) {
    __shared__ double sh[2 * CH_OP];
    if (*info != 0) return;
    const size_t i0 = (size_t)(j + 1 + blockIdx.x) * CH_B, j0 = (size_t)j * CH_B;
    ch_v4d acc[2][2];
    ch_zero(acc);
    ch_tile_mma<false, false>(acc, Lw + i0 + j0 * (size_t)L, (size_t)L, Ww + j0 + j0 * (size_t)L, (size_t)L, CH_B, sh);
    ch_for_result(acc, [&](int row, int col, double v) { Lw[(i0 + row) + (j0 + col) * (size_t)L] = v; });
}

// (4) block row i >= 1 of W = L^-1, tiles j = 0 .. i-1:  S = sum_{j<=p<i} L_ip W_pj, then W_ij = -L_ii^-1 S (S through LDS as the second product's B operand,
// L_ii^-1 read from Ww's diagonal tile in fragment order)
__global__ __launch_bounds__(CH_T) void chol_invrow_kernel(int64_t L, int i, const double* __restrict__ Lw, double* __restrict__ Ww, const int32_t* __restrict__ info) {
    __shared__ double sh[2 * CH_OP];
    if (*info != 0) return;
    const int j = blockIdx.x;
    const size_t i0 = (size_t)i * CH_B, j0 = (size_t)j * CH_B;
    ch_v4d acc[2][2];
    ch_zero(acc);
    ch_tile_mma<false, true>(acc, Lw + i0 + j0 * (size_t)L, (size_t)L, Ww + j0 + j0 * (size_t)L, (size_t)L, (i - j) * CH_B, sh);
    ch_for_result(acc, [&](int row, int col, double v) { sh[row * CH_LDX + col] = v; });          // S(k = row, x = col), staged [k][x]
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = (wv >> 1) * 32, wc = (wv & 1) * 32, lr = lane & 15, lk = lane >> 4;
    const double* __restrict__ Di = Ww + i0 + i0 * (size_t)L;
    ch_v4d out[2][2];
    ch_zero(out);
#pragma unroll 4
    for (int ks = 0; ks < CH_B; ks += 4) {
        double av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = Di[(size_t)(wr + 16 * a + lr) + (size_t)(ks + lk) * L];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = sh[(ks + lk) * CH_LDX + wc + 16 * b + lr];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) out[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], out[a][b], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ww[(i0 + wr + 16 * a + lk + 4 * r) + (j0 + wc + 16 * b + lr) * (size_t)L] = -out[a][b][r];
}

// (5) X = W'W, tiles i >= j:  X_ij = sum_{p>=i} W_pi' W_pj, stored at (i, j) and transposed at (j, i); of a diagonal tile only the lower half is taken
__global__ __launch_bounds__(CH_T) void chol_wtw_kernel(int64_t L, const double* __restrict__ Ww, double* __restrict__ X, const int32_t* __restrict__ info) {
    __shared__ double sh[2 * CH_OP];
    const int i = blockIdx.x, j = blockIdx.y;
    if (j > i || *info != 0) return;
    const size_t i0 = (size_t)i * CH_B, j0 = (size_t)j * CH_B;
    ch_v4d acc[2][2];
    ch_zero(acc);
    ch_tile_mma<true, true>(acc, Ww + i0 + i0 * (size_t)L, (size_t)L, Ww + i0 + j0 * (size_t)L, (size_t)L, (int)(L - (int64_t)i0), sh);
    ch_for_result(acc, [&](int row, int col, double v) {
        if (i != j || row >= col) {
            X[(i0 + row) + (j0 + col) * (size_t)L] = v;
            X[(j0 + col) + (i0 + row) * (size_t)L] = v;
        }
    });
}

// G = A A' + E for a ROW-major m x ld matrix A (ld % 64 == 0), E the identity on the padding m .. L-1: tiles i >= j of the L x L result, stored at (i, j) and mirrored
// at (j, i), so G is exactly symmetric.  Both operands are contiguous along K = ld (the [x][34] staging); K is walked in order by the tile's one workgroup: no split,
// nothing atomic, the same bits from every set-up.  Rows >= m of A do not exist: they are not read.
__global__ __launch_bounds__(CH_T) void gram_rows_kernel(int64_t m, int64_t ld, const double* __restrict__ A, int64_t L, double* __restrict__ G) {
    __shared__ double sh[2 * CH_OP];
    const int i = blockIdx.x, j = blockIdx.y;
    if (j > i) return;
    const size_t i0 = (size_t)i * CH_B, j0 = (size_t)j * CH_B;
    const int na = (int)std::min<int64_t>(CH_B, std::max<int64_t>(0, m - (int64_t)i0)), nb = (int)std::min<int64_t>(CH_B, std::max<int64_t>(0, m - (int64_t)j0));
    ch_v4d acc[2][2];
    ch_zero(acc);
    ch_tile_mma<true, true, true>(acc, A + i0 * (size_t)ld, (size_t)ld, A + j0 * (size_t)ld, (size_t)ld, (int)ld, sh, na, nb);
    ch_for_result(acc, [&](int row, int col, double v) {
        if (i != j || row >= col) {
            const size_t gi = i0 + row, gj = j0 + col;
            if (gi == gj && gi >= (size_t)m) v = 1.0;
            G[gi + gj * (size_t)L] = v;
            G[gj + gi * (size_t)L] = v;
        }
    });
}
}  // namespace

void launch_dense_gram_rows(const LaunchCtx& c, int64_t m, int64_t ld, const double* A, int64_t L, double* G) {
    const int nb = (int)(L / CH_B);
    hipLaunchKernelGGL(gram_rows_kernel, dim3(nb, nb), dim3(CH_T), 0, c.stream, m, ld, A, L, G);
}

// X = G^-1 for the symmetric positive definite G (column-major, leading dimension L, L % 64 == 0, padding = identity), on c.stream.  Lw and Ww: L x L work
// buffers (the factor and its inverse; only their lower tiles are touched), X: the full symmetric inverse.  G is not modified.  *info (device): 0, or the first
// column (1-based) whose pivot was not a positive finite number -- then X is not written.
void launch_dense_spd_inverse_chol(const LaunchCtx& c, int64_t L, const double* G, double* X, double* Lw, double* Ww, int32_t* info) {
    const int nb = (int)(L / CH_B);
    (void)hipMemsetAsync(info, 0, sizeof(int32_t), c.stream);
    for (int j = 0; j < nb; ++j) {
        hipLaunchKernelGGL(chol_update_kernel, dim3(nb - j), dim3(CH_T), 0, c.stream, L, j, G, Lw, info);
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(CH_T), 0, c.stream, L, j, Lw, Ww, info);
        if (j + 1 < nb) hipLaunchKernelGGL(chol_panel_kernel, dim3(nb - j - 1), dim3(CH_T), 0, c.stream, L, j, Lw, Ww, info);
    }
    for (int i = 1; i < nb; ++i) hipLaunchKernelGGL(chol_invrow_kernel, dim3(i), dim3(CH_T), 0, c.stream, L, i, Lw, Ww, info);
    hipLaunchKernelGGL(chol_wtw_kernel, dim3(nb, nb), dim3(CH_T), 0, c.stream, L, Ww, X, info);
}

// The same blocking and block order on the host (tests): K is k x k column-major, X its inverse (full, exactly symmetric).  Returns the first bad pivot's
// column (0-based) or -1.  fused: every multiply-add is one fused operation, k ascending, as the device's matrix-core products and contracted scalar code round them
// (the n-space forms' emulation, nspace.hip); otherwise product and sum round separately, as this emulation always did.
int64_t host_chol_inverse(int64_t k, const double* K, double* X, bool fused) {
    auto mad = [fused](double a, double b, double c) { return fused ? std::fma(a, b, c) : c + a * b; };      // c + a b
    auto msub = [fused](double a, double b, double c) { return fused ? std::fma(-a, b, c) : c - a * b; };    // c - a b
    const int64_t L = (k + CH_B - 1) / CH_B * CH_B, nb = L / CH_B;
    const size_t L2 = (size_t)L * (size_t)L;
    std::vector<double> G(L2, 0.0), Lw(L2, 0.0), Ww(L2, 0.0), Xf(L2, 0.0);
    for (int64_t i = 0; i < L; ++i) G[i + i * L] = 1.0;
    for (int64_t jc = 0; jc < k; ++jc)
        for (int64_t i = 0; i < k; ++i) G[i + jc * L] = K[i + jc * k];
    auto at = [L](std::vector<double>& M, int64_t bi, int64_t bj, int r, int cc) -> double& { return M[(bi * CH_B + r) + (bj * CH_B + cc) * L]; };
    double S[CH_B][CH_B];
    for (int64_t j = 0; j < nb; ++j) {
        for (int64_t i = j; i < nb; ++i)                                    // (1)
            for (int cc = 0; cc < CH_B; ++cc)
                for (int r = 0; r < CH_B; ++r) {
                    double acc = 0.0;
                    for (int64_t kk = 0; kk < j * CH_B; ++kk) acc = mad(Lw[(i * CH_B + r) + kk * L], Lw[(j * CH_B + cc) + kk * L], acc);
                    at(Lw, i, j, r, cc) = at(G, i, j, r, cc) - acc;
                }
        for (int cc = 0; cc < CH_B; ++cc) {                                 // (2)
            const double d = at(Lw, j, j, cc, cc);
            if (!(d > 0.0) || !(d <= DBL_MAX)) return j * CH_B + cc;
            const double rt = std::sqrt(d);
            for (int r = cc; r < CH_B; ++r) at(Lw, j, j, r, cc) = r == cc ? rt : at(Lw, j, j, r, cc) / rt;
            for (int jj = cc + 1; jj < CH_B; ++jj)
                for (int r = jj; r < CH_B; ++r) at(Lw, j, j, r, jj) = msub(at(Lw, j, j, r, cc), at(Lw, j, j, jj, cc), at(Lw, j, j, r, jj));
        }
        for (int cc = 0; cc < CH_B; ++cc)
            for (int r = 0; r < CH_B; ++r) {
                if (r < cc) at(Lw, j, j, r, cc) = 0.0;
                double s = r == cc ? 1.0 : 0.0;
                for (int p = cc; p < r; ++p) s = msub(at(Lw, j, j, r, p), at(Ww, j, j, p, cc), s);
                at(Ww, j, j, r, cc) = r < cc ? 0.0 : s / at(Lw, j, j, r, r);
            }
        for (int64_t i = j + 1; i < nb; ++i) {                              // (3)
            for (int cc = 0; cc < CH_B; ++cc)
                for (int r = 0; r < CH_B; ++r) {
                    double acc = 0.0;
                    for (int kk = 0; kk < CH_B; ++kk) acc = mad(at(Lw, i, j, r, kk), at(Ww, j, j, cc, kk), acc);
                    S[r][cc] = acc;
                }
            for (int cc = 0; cc < CH_B; ++cc)
                for (int r = 0; r < CH_B; ++r) at(Lw, i, j, r, cc) = S[r][cc];
        }
    }
    for (int64_t i = 1; i < nb; ++i)                                        // (4)
        for (int64_t j = 0; j < i; ++j) {
            for (int cc = 0; cc < CH_B; ++cc)
                for (int r = 0; r < CH_B; ++r) {
                    double acc = 0.0;
                    for (int64_t kk = j * CH_B; kk < i * CH_B; ++kk) acc = mad(Lw[(i * CH_B + r) + kk * L], Ww[kk + (j * CH_B + cc) * L], acc);
                    S[r][cc] = acc;
                }
            for (int cc = 0; cc < CH_B; ++cc)
                for (int r = 0; r < CH_B; ++r) {
                    double acc = 0.0;
                    for (int kk = 0; kk < CH_B; ++kk) acc = mad(at(Ww, i, i, r, kk), S[kk][cc], acc);
                    at(Ww, i, j, r, cc) = -acc;
                }
        }
    for (int64_t i = 0; i < nb; ++i)                                        // (5)
        for (int64_t j = 0; j <= i; ++j)
            for (int cc = 0; cc < CH_B; ++cc)
                for (int r = 0; r < CH_B; ++r) {
                    if (i == j && r < cc) continue;
                    double acc = 0.0;
                    for (int64_t kk = i * CH_B; kk < L; ++kk) acc = mad(Ww[kk + (i * CH_B + r) * L], Ww[kk + (j * CH_B + cc) * L], acc);
                    at(Xf, i, j, r, cc) = acc;
                    Xf[(j * CH_B + cc) + (i * CH_B + r) * L] = acc;
                }
    for (int64_t jc = 0; jc < k; ++jc)
        for (int64_t i = 0; i < k; ++i) X[i + jc * k] = Xf[i + jc * L];
    return -1;
}

}  // namespace fos
