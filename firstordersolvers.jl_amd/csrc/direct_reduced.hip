// direct = true, REDUCED form (HSDE.jl:12-15): the exact projection onto {Q u = v} through the inverse of the SMALLER Gram matrix only.
//   Q = [Q0 h; -h' 0],  Q0 = [0 A'; -A 0],  h = [c; b]:     G = I + Q Q' = I - Q Q = [ D + h h'   g ;  g'   1 + h'h ],
//   D = diag(I + A'A, I + A A'),   g = -Q0 h = [-A'b; A c].
// With k = min(m, n) and K = I + A'A (n <= m) or I + A A' (m < n), the other block of D^-1 is I - B K^-1 B' (B = A resp. A'), so d = D^-1 t1 needs
// K^-1 applied to TWO independent vectors (the block's own part of t1 and B' times the other part): ONE pass over K^-1 with two right-hand sides.
// K^-1 is symmetric: the tiles of its lower triangle are stored once (4 k^2 bytes) and every stored tile serves both T x_J -> y_I and T' x_I -> y_J.
// With p = D^-1 h, q = D^-1 g (formed at set-up through the same path) and t = [t1; t2]:
//   [ 1 + h'p   h'q             ] [ sigma ]   [ h'd      ]
//   [ g'p       g'q - (1 + h'h) ] [ w2    ] = [ g'd - t2 ],      w = G^-1 t = [ d - sigma p - w2 q ;  w2 ].
// Everything here adds in a fixed order: no floating-point atomics, two projections of the same input are bit-identical.
#include "fos_internal.hpp"
#include "dev_common.hpp"

#include <algorithm>

namespace fos {

namespace {
constexpr int RED_THREADS = 256;
#define RED_GRID_STRIDE(i, n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)
typedef double v2d __attribute__((ext_vector_type(2)));
}  // namespace

// ------------------------------------------------------------------------------------------------ the plan (host)
// Tiles of RED_TR = 64 rows x RED_TC = 32 columns.  Row block I covers rows [64 I, 64 I + 64), strip j columns [32 j, 32 j + 32); strip j lies in
// column block J = j / 2.  Stored: every tile (I, j) with I >= J -- the two strips of a diagonal block whole.  A UNIT = one strip and a run of at
// most RED_CHUNK row blocks: the work of one wavefront, its tiles contiguous in the stream.
void build_reduced_plan(int64_t k, RedPlan* P) {
    P->k = k;
    P->nt = (int)((k + RED_TR - 1) / RED_TR);
    P->ns = 2 * P->nt;
    P->ntiles = (int64_t)P->nt * (P->nt + 1);
    P->units.clear();
    P->strip_u0.assign((size_t)P->ns + 1, 0);
    int64_t tile = 0;
    for (int j = 0; j < P->ns; ++j) {
        P->strip_u0[j] = (int32_t)P->units.size();
        for (int i0 = j / 2; i0 < P->nt; i0 += RED_CHUNK) {
            const int i1 = std::min(P->nt, i0 + RED_CHUNK);
            P->units.push_back(RedUnit{j, i0, i1, (int32_t)tile});
            tile += i1 - i0;
        }
    }
    P->strip_u0[P->ns] = (int32_t)P->units.size();
}

// ------------------------------------------------------------------------------------------------ set-up kernels
// K = I + B'B, dense column-major with leading dimension ld (zeroed by the caller; rows / columns k.. of the padding: identity), from B's columns
// (cptr / cidx / cval) and B's rows (rptr / ridx / rval).  One workgroup per column jc: the entries (r, a) of column jc one after the other, the entries of
// row r side by side (distinct rows of K) -- every entry of K is added up in the order of B's rows, the same in every run.
__global__ __launch_bounds__(RED_THREADS) void red_form_k_kernel(int64_t k, int64_t ld, const int32_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                                 const double* __restrict__ cval, const int32_t* __restrict__ rptr,
                                                                 const int32_t* __restrict__ ridx, const double* __restrict__ rval, double* K) {
    for (int64_t jc = blockIdx.x; jc < ld; jc += gridDim.x) {
        double* col = K + jc * ld;
        if (jc < k) {
            for (int e = cptr[jc]; e < cptr[jc + 1]; ++e) {
                const int r = cidx[e];
                const double a = cval[e];
                for (int t = rptr[r] + (int)threadIdx.x; t < rptr[r + 1]; t += RED_THREADS) col[ridx[t]] += a * rval[t];
                __syncthreads();
            }
        }
        if (threadIdx.x == 0) col[jc] += 1.0;
        __syncthreads();
    }
}

// the tile stream from the dense symmetric X (column-major, leading dimension ld): element (r, c) of a tile at 128 (c / 2) + 2 r + (c & 1), so that lane r
// reads columns 2 q, 2 q + 1 of its row with one 16-byte load; entries beyond order k: zero
__global__ __launch_bounds__(RED_THREADS) void red_pack_tiles_kernel(int64_t k, int64_t ld, const double* __restrict__ X, const RedUnit* __restrict__ units,
                                                                     double* __restrict__ tiles) {
    const RedUnit u = units[blockIdx.x];
    for (int I = u.i0; I < u.i1; ++I) {
        double* t = tiles + (size_t)(u.tile0 + (I - u.i0)) * RED_TILE;
        for (int e = threadIdx.x; e < RED_TILE; e += RED_THREADS) {
            const int q = e >> 7, r = (e & 127) >> 1, c = 2 * q + (e & 1);
            const int64_t row = (int64_t)RED_TR * I + r, colx = (int64_t)RED_TC * u.j + c;
            t[e] = (row < k && colx < k) ? X[colx * ld + row] : 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the tile product (hot path)
// (y_p, y_q) = K^-1 (p, q) from the packed lower triangle.  One wavefront per unit, lane = row of the tile.  Per tile: 16 non-temporal 16-byte loads per
// lane (issued half a tile ahead: the second half of this tile and the first half of the next are in flight while the first half is multiplied), the
// strip's 32 operand pairs broadcast from LDS, the row block's pair in registers.  T x_J stays in the lane and goes to the tile's own slot; T' x_I is kept in
// 64 accumulators per lane over the whole unit and crosses the lanes once, at the unit's end (a butterfly in a fixed order).  The diagonal tiles feed
// the row side only.  red_fold_kernel adds the slots.
__device__ __forceinline__ void red_load_half(v2d (&a)[16], int half, const double* __restrict__ tile, int lane) {
    const v2d* __restrict__ tp = reinterpret_cast<const v2d*>(tile);
#pragma unroll
    for (int q = 0; q < 8; ++q) a[8 * half + q] = __builtin_nontemporal_load(tp + (8 * half + q) * 64 + lane);
}
__device__ __forceinline__ void red_mul_half(const v2d (&a)[16], int half, const d2* xs, const d2& xi, d2& ry, double (&ca)[64]) {
#pragma unroll
    for (int q = 8 * half; q < 8 * half + 8; ++q) {
        const d2 x0 = xs[2 * q], x1 = xs[2 * q + 1];
        ry.x += a[q].x * x0.x; ry.y += a[q].x * x0.y;
        ry.x += a[q].y * x1.x; ry.y += a[q].y * x1.y;
        ca[4 * q + 0] += a[q].x * xi.x; ca[4 * q + 1] += a[q].x * xi.y;
        ca[4 * q + 2] += a[q].y * xi.x; ca[4 * q + 3] += a[q].y * xi.y;
    }
}
__global__ __launch_bounds__(RED_THREADS, 1) void red_symm_kernel(const RedUnit* __restrict__ units, int nunits, const double* __restrict__ tiles,
                                                                  const d2* __restrict__ pq, d2* __restrict__ rowslot, double* __restrict__ colslot) {
    __shared__ d2 xs_all[RED_THREADS / 64][RED_TC];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int unit = blockIdx.x * (RED_THREADS / 64) + wv;
    if (unit >= nunits) return;                                   // (no workgroup barrier below: wavefronts are independent)
    const RedUnit u = units[unit];
    d2* xs = xs_all[wv];
    if (lane < RED_TC) xs[lane] = pq[(int64_t)RED_TC * u.j + lane];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);                                // the wavefront's own LDS writes have landed before its reads
    double ca[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) ca[i] = 0.0;
    const int J = u.j >> 1;
    const double* tile = tiles + (size_t)u.tile0 * RED_TILE;
    v2d a[16];
    red_load_half(a, 0, tile, lane);
    red_load_half(a, 1, tile, lane);
    d2 xi = pq[(int64_t)RED_TR * u.i0 + lane];
    for (int I = u.i0; I < u.i1 - 1; ++I) {                       // (the unit's last tile is peeled off: nothing to request behind it)
        const double* next = tile + RED_TILE;
        const d2 xin = pq[(int64_t)RED_TR * (I + 1) + lane];
        const d2 xe = (I == J) ? make_double2(0.0, 0.0) : xi;     // a diagonal tile: the row side only
        int xoff = 0;
        asm volatile("" : "+v"(xoff));                            // (keeps the 32 operand pairs in LDS: hoisted out of the loop they would cost 128 registers)
        const d2* xsv = xs + xoff;
        d2 ry = make_double2(0.0, 0.0);
        red_mul_half(a, 0, xsv, xe, ry, ca);
        red_load_half(a, 0, next, lane);
        red_mul_half(a, 1, xsv, xe, ry, ca);
        red_load_half(a, 1, next, lane);
        rowslot[((int64_t)I * (I + 1) + u.j) * 64 + lane] = ry;
        tile = next;
        xi = xin;
    }
    {
        const int I = u.i1 - 1;
        const d2 xe = (I == J) ? make_double2(0.0, 0.0) : xi;
        d2 ry = make_double2(0.0, 0.0);
        red_mul_half(a, 0, xs, xe, ry, ca);
        red_mul_half(a, 1, xs, xe, ry, ca);
        rowslot[((int64_t)I * (I + 1) + u.j) * 64 + lane] = ry;
    }
    // column sums: 64 values per lane (index 2 c + rhs) over 64 lanes -> lane L ends with value L
#pragma unroll
    for (int half = 32; half >= 1; half >>= 1) {
        const bool up = (lane & half) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const double send = up ? ca[i] : ca[i + half];
            const double keep = up ? ca[i + half] : ca[i];
            ca[i] = keep + __shfl_xor(send, half, 64);
        }
    }
    colslot[(int64_t)unit * 64 + lane] = ca[0];
}

// y[64 I + r] = the row slots of (I, 0 .. 2 I + 1) + the column slots of the units of the row's strip, in a fixed order: 16 wavefronts take the row slots
// round robin, their sums are added in wavefront order, then the units in stream order
constexpr int RED_FOLD_WAVES = 16;
__global__ __launch_bounds__(64 * RED_FOLD_WAVES) void red_fold_kernel(const d2* __restrict__ rowslot, const double* __restrict__ colslot,
                                                                       const int32_t* __restrict__ strip_u0, d2* __restrict__ y) {
    __shared__ d2 part[RED_FOLD_WAVES][64];
    const int I = blockIdx.x, r = threadIdx.x & 63, w = threadIdx.x >> 6;
    d2 acc = make_double2(0.0, 0.0);
    const d2* base = rowslot + (int64_t)I * (I + 1) * 64 + r;
    for (int jj = w; jj < 2 * I + 2; jj += RED_FOLD_WAVES) { const d2 v = base[(int64_t)jj * 64]; acc.x += v.x; acc.y += v.y; }
    part[w][r] = acc;
    __syncthreads();
    if (w != 0) return;
    d2 s = part[0][r];
    for (int q = 1; q < RED_FOLD_WAVES; ++q) { s.x += part[q][r].x; s.y += part[q][r].y; }
    const int j = 2 * I + (r >> 5), c = r & 31;
    for (int u = strip_u0[j]; u < strip_u0[j + 1]; ++u) { s.x += colslot[(int64_t)u * 64 + 2 * c]; s.y += colslot[(int64_t)u * 64 + 2 * c + 1]; }
    y[(int64_t)RED_TR * I + r] = s;
}

// ------------------------------------------------------------------------------------------------ the vector work around it
// swap = 0 (n <= m): K = I + A'A, the block's own part of t is t_x, the other t_y;  swap = 1 (m < n): K = I + A A', own part t_y, other t_x.
// (1) vin = the OTHER part of t in place (component 0), zero elsewhere: Q vin carries B' t_other in the own part's rows
__global__ __launch_bounds__(RED_THREADS) void red_in1_kernel(int64_t l, int64_t n, int swap, const double* __restrict__ t, d2* __restrict__ vin) {
    RED_GRID_STRIDE(i, l) {
        const bool other = swap ? (i < n) : (i >= n && i < l - 1);
        vin[i] = make_double2(other ? t[i] : 0.0, 0.0);
    }
}
// (2) the operand pairs (own part of t, B' t_other):  n <= m: (t_x, A' t_y) = (t_i, s1_i);  m < n: (t_y, A t_x) = (t_{n+i}, -s1_{n+i});  zero beyond k
__global__ __launch_bounds__(RED_THREADS) void red_pair_kernel(int64_t kpad, int64_t k, int64_t n, int swap, const double* __restrict__ t,
                                                               const double* __restrict__ s1, d2* __restrict__ pq) {
    RED_GRID_STRIDE(i, kpad) {
        d2 v = make_double2(0.0, 0.0);
        if (i < k) v = swap ? make_double2(t[n + i], -s1[n + i]) : make_double2(t[i], s1[i]);
        pq[i] = v;
    }
}
// (3) vin = e = K^-1 B' t_other in the own part's place: Q vin carries B e in the other part's rows
__global__ __launch_bounds__(RED_THREADS) void red_in2_kernel(int64_t l, int64_t n, int swap, const d2* __restrict__ yk, d2* __restrict__ vin) {
    RED_GRID_STRIDE(i, l) {
        const bool own = swap ? (i >= n && i < l - 1) : (i < n);
        vin[i] = make_double2(own ? yk[swap ? i - n : i].y : 0.0, 0.0);
    }
}
// (4) d = D^-1 t1: own part K^-1 t_own, other part t_other - B e  (n <= m: t_y + s2_y, s2 = Q (e, 0, 0);  m < n: t_x - s2_x, s2 = Q (0, e, 0));
//     partial sums of h'd and g'd per workgroup (dots != nullptr)
__global__ __launch_bounds__(RED_THREADS) void red_d_kernel(int64_t l, int64_t n, int swap, const double* __restrict__ t, const double* __restrict__ s2,
                                                            const d2* __restrict__ yk, const double* __restrict__ hv, const double* __restrict__ gv,
                                                            double* __restrict__ d, double* __restrict__ dots) {
    double a0 = 0.0, a1 = 0.0;
    RED_GRID_STRIDE(i, l - 1) {
        double v;
        if (swap) v = (i < n) ? t[i] - s2[i] : yk[i - n].x;
        else v = (i < n) ? yk[i].x : t[i] + s2[i];
        d[i] = v;
        if (dots) { a0 += hv[i] * v; a1 += gv[i] * v; }
    }
    if (!dots) return;
    __shared__ double sm[2][RED_THREADS / 64];
    a0 = wave_sum(a0); a1 = wave_sum(a1);
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = a0; sm[1][threadIdx.x >> 6] = a1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double b0 = sm[0][0], b1 = sm[1][0];
        for (int w = 1; w < RED_THREADS / 64; ++w) { b0 += sm[0][w]; b1 += sm[1][w]; }
        dots[2 * blockIdx.x] = b0; dots[2 * blockIdx.x + 1] = b1;
    }
}
// (5) every workgroup adds the records in order, solves the 2 x 2 border system (its inverse minv, row-major) and writes its share of
//     w = [d - sigma p - w2 q; w2]   (add != 0: w += that -- the refinement step)
__global__ __launch_bounds__(RED_THREADS) void red_w_kernel(int64_t l, const double* __restrict__ t, const double* __restrict__ d, const double* __restrict__ pv,
                                                            const double* __restrict__ qv, const double* __restrict__ dots, int nrec, double m00, double m01,
                                                            double m10, double m11, int add, double* __restrict__ w) {
    __shared__ double sg[2];
    if (threadIdx.x < 128) {                                        // wavefront 0: h'd, wavefront 1: g'd -- lane by lane, then the butterfly: a fixed order
        const int which = threadIdx.x >> 6;
        double s = 0.0;
        for (int q = threadIdx.x & 63; q < nrec; q += 64) s += dots[2 * q + which];
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) sg[which] = s;
    }
    __syncthreads();
    const double r0 = sg[0], r1 = sg[1] - t[l - 1];
    const double sigma = m00 * r0 + m01 * r1, w2 = m10 * r0 + m11 * r1;
    RED_GRID_STRIDE(i, l) {
        const double v = (i < l - 1) ? d[i] - sigma * pv[i] - w2 * qv[i] : w2;
        w[i] = add ? w[i] + v : v;
    }
}
// r = t - (w - z), z = Q Q w: the residual of G w = t  (G = I - Q Q)
__global__ __launch_bounds__(RED_THREADS) void red_resid_kernel(int64_t l, const double* __restrict__ t, const double* __restrict__ w, const double* __restrict__ z,
                                                                double* __restrict__ r) {
    RED_GRID_STRIDE(i, l) r[i] = t[i] - (w[i] - z[i]);
}

// ------------------------------------------------------------------------------------------------ launchers
static int red_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + RED_THREADS - 1) / RED_THREADS, RED_DOT_BLOCKS)); }

void launch_red_form_k(const LaunchCtx& c, int64_t k, int64_t ld, const int32_t* cptr, const int32_t* cidx, const double* cval, const int32_t* rptr,
                       const int32_t* ridx, const double* rval, double* K) {
    hipLaunchKernelGGL(red_form_k_kernel, dim3((unsigned)std::min<int64_t>(ld, 65536)), dim3(RED_THREADS), 0, c.stream, k, ld, cptr, cidx, cval, rptr, ridx, rval, K);
}
void launch_red_pack_tiles(const LaunchCtx& c, const RedDev& R, int64_t ld, const double* X) {
    hipLaunchKernelGGL(red_pack_tiles_kernel, dim3((unsigned)R.nunits), dim3(RED_THREADS), 0, c.stream, R.k, ld, X, R.units, R.tiles);
}
void launch_red_symm(const LaunchCtx& c, const RedDev& R, const double2* pq, double2* y) {
    const int per = RED_THREADS / 64;
    hipLaunchKernelGGL(red_symm_kernel, dim3((unsigned)((R.nunits + per - 1) / per)), dim3(RED_THREADS), 0, c.stream, R.units, R.nunits, R.tiles, pq, R.rowslot,
                       R.colslot);
    hipLaunchKernelGGL(red_fold_kernel, dim3((unsigned)R.nt), dim3(64 * RED_FOLD_WAVES), 0, c.stream, R.rowslot, R.colslot, R.strip_u0, y);
}
void launch_red_in1(const LaunchCtx& c, int swap, const double* t, double2* vin) {
    hipLaunchKernelGGL(red_in1_kernel, dim3(red_blocks(c.l)), dim3(RED_THREADS), 0, c.stream, c.l, c.n, swap, t, vin);
}
void launch_red_pair(const LaunchCtx& c, const RedDev& R, int swap, const double* t, const double* s1, double2* pq) {
    hipLaunchKernelGGL(red_pair_kernel, dim3(red_blocks(R.kpad)), dim3(RED_THREADS), 0, c.stream, R.kpad, R.k, c.n, swap, t, s1, pq);
}
void launch_red_in2(const LaunchCtx& c, int swap, const double2* yk, double2* vin) {
    hipLaunchKernelGGL(red_in2_kernel, dim3(red_blocks(c.l)), dim3(RED_THREADS), 0, c.stream, c.l, c.n, swap, yk, vin);
}
int launch_red_d(const LaunchCtx& c, int swap, const double* t, const double* s2, const double2* yk, const double* hv, const double* gv, double* d, double* dots) {
    const int nb = red_blocks(c.l - 1);
    hipLaunchKernelGGL(red_d_kernel, dim3(nb), dim3(RED_THREADS), 0, c.stream, c.l, c.n, swap, t, s2, yk, hv, gv, d, dots);
    return nb;
}
void launch_red_w(const LaunchCtx& c, const double* t, const double* d, const double* pv, const double* qv, const double* dots, int nrec, const double* minv,
                  int add, double* w) {
    hipLaunchKernelGGL(red_w_kernel, dim3(red_blocks(c.l)), dim3(RED_THREADS), 0, c.stream, c.l, t, d, pv, qv, dots, nrec, minv[0], minv[1], minv[2], minv[3], add, w);
}
void launch_red_resid(const LaunchCtx& c, const double* t, const double* w, const double* z, double* r) {
    hipLaunchKernelGGL(red_resid_kernel, dim3(red_blocks(c.l)), dim3(RED_THREADS), 0, c.stream, c.l, t, w, z, r);
}

// ------------------------------------------------------------------------------------------------ host emulation (CPU tests of the packing and the order)
// packs the lower triangle of the symmetric k x k matrix X (column-major) as the device does; `count` (k x k, optional) receives how many tile slots hold each
// entry of the lower triangle (diagonal blocks: of the whole block)
void host_reduced_pack(const RedPlan& P, const double* X, std::vector<double>* tiles, int32_t* count) {
    tiles->assign((size_t)P.ntiles * RED_TILE, 0.0);
    const int64_t k = P.k;
    for (const RedUnit& u : P.units)
        for (int I = u.i0; I < u.i1; ++I) {
            double* t = tiles->data() + (size_t)(u.tile0 + (I - u.i0)) * RED_TILE;
            for (int e = 0; e < RED_TILE; ++e) {
                const int q = e >> 7, r = (e & 127) >> 1, c = 2 * q + (e & 1);
                const int64_t row = (int64_t)RED_TR * I + r, colx = (int64_t)RED_TC * u.j + c;
                if (row < k && colx < k) { t[e] = X[colx * k + row]; if (count) count[colx * k + row] += 1; }
            }
        }
}
// the kernels' product over the packed tiles: slots, butterfly and fold in the device's order; pq, y: kpad pairs
void host_reduced_symm(const RedPlan& P, const std::vector<double>& tiles, const double* pq, double* y) {
    const int64_t kpad = (int64_t)P.nt * RED_TR;
    std::vector<double> rowslot((size_t)P.ntiles * 64 * 2, 0.0), colslot(P.units.size() * 64, 0.0);
    for (size_t un = 0; un < P.units.size(); ++un) {
        const RedUnit& u = P.units[un];
        std::vector<double> ca((size_t)64 * 64, 0.0);            // [lane][2 c + rhs]
        for (int I = u.i0; I < u.i1; ++I) {
            const double* t = tiles.data() + (size_t)(u.tile0 + (I - u.i0)) * RED_TILE;
            for (int lane = 0; lane < 64; ++lane) {
                const double* xi = pq + 2 * ((int64_t)RED_TR * I + lane);
                const double x0 = (I == u.j / 2) ? 0.0 : xi[0], x1 = (I == u.j / 2) ? 0.0 : xi[1];
                double r0 = 0.0, r1 = 0.0;
                for (int c = 0; c < RED_TC; ++c) {
                    const double a = t[128 * (c >> 1) + 2 * lane + (c & 1)];
                    const double* xj = pq + 2 * ((int64_t)RED_TC * u.j + c);
                    r0 += a * xj[0]; r1 += a * xj[1];
                    ca[(size_t)lane * 64 + 2 * c] += a * x0; ca[(size_t)lane * 64 + 2 * c + 1] += a * x1;
                }
                double* rs = rowslot.data() + 2 * (((int64_t)I * (I + 1) + u.j) * 64 + lane);
                rs[0] = r0; rs[1] = r1;
            }
        }
        for (int half = 32; half >= 1; half >>= 1) {
            std::vector<double> nx((size_t)64 * 64, 0.0);
            for (int lane = 0; lane < 64; ++lane) {
                const bool up = (lane & half) != 0;
                const int other = lane ^ half;
                for (int i = 0; i < half; ++i) {
                    const double keep = up ? ca[(size_t)lane * 64 + i + half] : ca[(size_t)lane * 64 + i];
                    const double got = up ? ca[(size_t)other * 64 + i + half] : ca[(size_t)other * 64 + i];      // what the partner sends: the half IT does not keep
                    nx[(size_t)lane * 64 + i] = keep + got;
                }
            }
            ca.swap(nx);
        }
        for (int lane = 0; lane < 64; ++lane) colslot[un * 64 + lane] = ca[(size_t)lane * 64];
    }
    for (int I = 0; I < P.nt; ++I)
        for (int r = 0; r < 64; ++r) {
            double part[RED_FOLD_WAVES][2];
            for (int w = 0; w < RED_FOLD_WAVES; ++w) {
                part[w][0] = part[w][1] = 0.0;
                for (int jj = w; jj < 2 * I + 2; jj += RED_FOLD_WAVES) {
                    const double* rs = rowslot.data() + 2 * (((int64_t)I * (I + 1) + jj) * 64 + r);
                    part[w][0] += rs[0]; part[w][1] += rs[1];
                }
            }
            double s0 = part[0][0], s1 = part[0][1];
            for (int w = 1; w < RED_FOLD_WAVES; ++w) { s0 += part[w][0]; s1 += part[w][1]; }
            const int j = 2 * I + (r >> 5), c = r & 31;
            for (int u = P.strip_u0[j]; u < P.strip_u0[j + 1]; ++u) { s0 += colslot[(size_t)u * 64 + 2 * c]; s1 += colslot[(size_t)u * 64 + 2 * c + 1]; }
            const int64_t i = (int64_t)RED_TR * I + r;
            if (i < kpad) { y[2 * i] = s0; y[2 * i + 1] = s1; }
        }
}

}  // namespace fos
