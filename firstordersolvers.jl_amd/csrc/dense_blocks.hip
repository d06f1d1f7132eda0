// Feasibility form: dense Quadratic, LeastSquares and IndAffine blocks of a SeparableSum (the dense part of SetBlocks, sets.hip).
//   A block of p <= 1024 entries with a dense matrix of its own has the prox (step 1)
//     FOS_FN_BLK_QUADRATIC      y = (I + Q)^-1 (x - q)
//     FOS_SET_BLK_AFFINE        y = x - A^+ (A x - b)
//     FOS_FN_BLK_LEAST_SQUARES  y = (I + lambda A'A)^-1 (x + lambda A'b)
//   and all three are ONE device formula, y = G x + d, with a symmetric apply matrix G of order p and an offset d per block:
//     Quadratic G = (I + Q)^-1, d = -G q | LeastSquares G = (I + lambda A'A)^-1, d = lambda G A'b | IndAffine G = I - A^+ A, d = A^+ b.
// Set-up, on the host in long double (the precedent: the block form of direct.cpp), per DISTINCT matrix -- blocks name their matrix by index, many blocks may
// name one -- on a pool of at most 16 threads:
//     Quadratic / LeastSquares  M = L L' (Cholesky, a failed pivot is refused with its column), K = L^-1, G = K'K
//     IndAffine                 rows of A scaled to unit norm (as affine_dense.hip), A A' = L L' (a pivot <= 2^-48 is refused: A needs full row rank; a smaller
//                               pivot t puts 2^-64 / sqrt(t) > 2^-40 ~ the project's 1e-12 into the apply), W = L^-1 A (orthonormal rows), G = I - W'W, d = W' L^-1 b
//   G and d are rounded to fp64 once.  Rounding G from long double keeps the factor cond(M) eps of an fp64 inverse out of the apply: no refinement step.
// Storage, per matrix: the packed lower triangle of G, row by row (entry (i, j), i >= j, at i (i + 1) / 2 + j; 4 p (p + 1) bytes, half the traffic of the square)
//   wherever it is staged in LDS, and the full square (coalesced straight from memory) for the orders whose triangle does not fit: the faster one per case on the
//   MI355X.  FOS_DENSE_BLOCKS_SQUARE = 1 | 0 at set-up forces either everywhere (measurements: tools/dense_blocks_bench.py); the bits of y do not depend on it.
// Kernels: a prox adds at most two launches, one per class present, no synchronise and no copy.
//   wavefront class (p <= 64)         one 64-thread workgroup serves 64 / T runs, T the power of two that holds p (p <= 32: several runs per wavefront); x_b and the
//                                     triangle sit in LDS, one output row per lane
//   workgroup class (65 <= p <= 1024) one 256-thread workgroup per run; x_b in LDS, the rows dealt to the threads (row r to thread r mod 256); the triangle in LDS
//                                     while it fits the CU's 160 KiB beside x (p <= 200), else the full square, read coalesced
//   A run is up to DB_RUN blocks that name one matrix: the triangle is loaded once (coalesced) and the run's blocks are walked.
// One order of additions everywhere: row r is the chain acc = d_r; acc = fma(G(r, j), x_j, acc), j = 0 .. p - 1.  No atomics: two runs give the same bits, a
// shared matrix changes traffic and never bits, and the host emulation (fos_host_dense_block) reproduces the bits.  A thread stores y only at its own rows of its
// own block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "fos_internal.hpp"

namespace fos {

constexpr int DB_MAX = 1024;                  // the largest order
constexpr int DB_WAVE_MAX = 64;               // wavefront class
constexpr int DB_WG_THREADS = 256;
constexpr int DB_RUN = 8;                     // blocks of one matrix served by one team
constexpr int DB_WAVE_TRI = DB_WAVE_MAX * (DB_WAVE_MAX + 1) / 2;      // doubles of LDS for the triangles of a wavefront-class workgroup
constexpr size_t DB_LDS_BYTES = 160 * 1024;   // gfx950: LDS of a CU, all of which one workgroup may take
constexpr int DB_POOL = 16;                   // host threads of the set-up, at most

struct DbSlot {                               // a run: blocks run[first .. first + nblk - 1] on the matrix at goff
    int64_t goff;
    int32_t p, nblk, first, in_lds, square, pad;      // square: the matrix is kept as the full square (never staged in LDS)
};
struct DbItem { int32_t first_slot, nslots, T, maxrun; };      // a workgroup: nslots sub-teams of T threads
struct DbBlock { int64_t start, doff; };      // first entry of the block in x / y, of its offset in d

__host__ __device__ inline int64_t db_tri(int64_t i, int64_t j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// One workgroup of NT threads = NT / T sub-teams; each stages its run's matrix (in_lds) and walks the run.  Every barrier is reached by every thread: the trip
// counts (item.maxrun) are uniform over the workgroup.
template <int NT>
__device__ __forceinline__ void db_team(const DbItem item, const DbSlot* __restrict__ slots, const int32_t* __restrict__ run, const DbBlock* __restrict__ blocks,
                                        const double* __restrict__ G, const double* __restrict__ dvec, const double* __restrict__ x,
                                        double* __restrict__ y, double* lds) {
    const int t = threadIdx.x, T = item.T, sub = t / T, r0 = t - sub * T;
    const bool active = sub < item.nslots;
    DbSlot s{};
    if (active) s = slots[item.first_slot + sub];
    const int p = s.p;
    double *tri, *xs;
    if constexpr (NT == 64) { tri = lds + (size_t)sub * (T * (T + 1) / 2); xs = lds + DB_WAVE_TRI + (size_t)sub * T; }      // 64 / T triangles (32 (T + 1) doubles at most), then the x
    else { xs = lds; tri = lds + ((p + 1) & ~1); }                                                                        // x, then the triangle (16-byte aligned)
    const double* Gm = G + s.goff;
    if (active && s.in_lds) {
        const int ne = p * (p + 1) / 2;
        for (int e = r0; e < ne; e += T) tri[e] = Gm[e];
    }
    for (int k = 0; k < item.maxrun; ++k) {
        const bool has = active && k < s.nblk;
        DbBlock b{};
        if (has) {
            b = blocks[run[s.first + k]];
            for (int i = r0; i < p; i += T) xs[i] = x[b.start + i];
        }
        __syncthreads();
        if (has) {
            for (int r = r0; r < p; r += T) {
                double acc = dvec[b.doff + r];
                if (s.square) {
                    for (int j = 0; j < p; ++j) acc = fma(Gm[(size_t)j * p + r], xs[j], acc);
                } else if (s.in_lds) {
                    const double* row = tri + r * (r + 1) / 2;
                    for (int j = 0; j <= r; ++j) acc = fma(row[j], xs[j], acc);
                    int idx = (r + 1) * (r + 2) / 2 + r;
                    for (int j = r + 1; j < p; ++j) { acc = fma(tri[idx], xs[j], acc); idx += j + 1; }
                } else {
                    const double* row = Gm + (size_t)r * (r + 1) / 2;
                    for (int j = 0; j <= r; ++j) acc = fma(row[j], xs[j], acc);
                    size_t idx = (size_t)(r + 1) * (r + 2) / 2 + r;
                    for (int j = r + 1; j < p; ++j) { acc = fma(Gm[idx], xs[j], acc); idx += j + 1; }
                }
                y[b.start + r] = acc;
            }
        }
        __syncthreads();                                          // (xs is rewritten by the next block of the run)
    }
}

__global__ __launch_bounds__(64) void dense_blocks_wave_kernel(const DbItem* __restrict__ items, const DbSlot* __restrict__ slots, const int32_t* __restrict__ run,
                                                               const DbBlock* __restrict__ blocks, const double* __restrict__ G, const double* __restrict__ dvec,
                                                               const double* __restrict__ x, double* __restrict__ y) {
    __shared__ double lds[DB_WAVE_TRI + 64];
    const DbItem item = items[blockIdx.x];
    db_team<64>(item, slots, run, blocks, G, dvec, x, y, lds);
}
// dynamic LDS: 8 bytes x the largest (p + the triangle, where it is staged) of the launch's runs
__global__ __launch_bounds__(DB_WG_THREADS) void dense_blocks_wg_kernel(const DbItem* __restrict__ items, const DbSlot* __restrict__ slots,
                                                                        const int32_t* __restrict__ run, const DbBlock* __restrict__ blocks,
                                                                        const double* __restrict__ G, const double* __restrict__ dvec,
                                                                        const double* __restrict__ x, double* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) double db_lds[];
    const DbItem item = items[blockIdx.x];
    db_team<DB_WG_THREADS>(item, slots, run, blocks, G, dvec, x, y, db_lds);
}

// ------------------------------------------------------------------------------------------ host: the set-up of one distinct matrix
namespace {

typedef long double ldbl;

const char* db_kind_name(int kind) { return kind == FOS_FN_BLK_QUADRATIC ? "Quadratic" : kind == FOS_SET_BLK_AFFINE ? "IndAffine" : "LeastSquares"; }
bool db_fin(double v) { return v == v && std::fabs(v) <= 1.79e308; }

std::string db_msg(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// f(t, nt) on nt threads (t = 0 .. nt - 1; the caller is thread 0).  Every use below gives each output entry to ONE thread, which adds in the serial order:
// the bits do not depend on nt
template <typename F>
void db_par(int nt, F&& f) {
    if (nt <= 1) { f(0, 1); return; }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back([&f, t, nt]() { f(t, nt); });
    f(0, nt);
    for (auto& th : pool) th.join();
}

// M (order k, row-major, lower triangle) = L L' in place; the column (1-based) of the first pivot that is not > floor, or 0
int db_cholesky(int k, std::vector<ldbl>& M, ldbl floor) {
    for (int i = 0; i < k; ++i) {
        ldbl* ri = &M[(size_t)i * k];
        for (int j = 0; j <= i; ++j) {
            const ldbl* rj = &M[(size_t)j * k];
            ldbl v = ri[j];
            for (int c = 0; c < j; ++c) v -= ri[c] * rj[c];
            if (j < i) ri[j] = v / rj[j];
            else {
                if (!(v > floor) || !(v <= LDBL_MAX)) return i + 1;
                ri[i] = sqrtl(v);
            }
        }
    }
    return 0;
}

// What one distinct matrix leaves: G (order p, full square, symmetric bit for bit) and what d needs
struct DbFactor {
    int kind = 0, p = 0, m = 0;
    double lambda = 0.0;
    std::vector<double> G;                    // p x p
    std::vector<ldbl> Gl;                     // Quadratic, LeastSquares: G in long double (p x p)
    std::vector<ldbl> W, L, scale;            // IndAffine: W = L^-1 As (m x p), L (m x m), the row factors
    const double* M = nullptr;                // the caller's matrix (LeastSquares: A'b)
};

// blk: the 1-based block named in a message.  M: m x p row-major (Quadratic: m == p, the lower triangle is read).  nt: threads this matrix may use (orders from 128)
int db_factor(int64_t blk, int kind, int64_t m, int64_t p, const double* M, double lambda, int nt, DbFactor* F, std::string* err) {
    if (p < 128) nt = 1;
    const char* name = db_kind_name(kind);
    F->kind = kind; F->p = (int)p; F->m = (int)m; F->lambda = lambda; F->M = M;
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < (kind == FOS_FN_BLK_QUADRATIC ? i + 1 : p); ++j)
            if (!db_fin(M[i * p + j])) { *err = db_msg("set block %lld (%s): entry (%lld, %lld) of its matrix is not finite", (long long)blk, name, (long long)i + 1, (long long)j + 1); return FOS_EINVAL; }
    const int P = (int)p;
    F->G.assign((size_t)P * P, 0.0);
    if (kind == FOS_SET_BLK_AFFINE) {
        const int mm = (int)m;
        std::vector<ldbl>& W = F->W;
        W.assign((size_t)mm * P, 0.0L);
        F->scale.assign((size_t)mm, 0.0L);
        for (int i = 0; i < mm; ++i) {                             // rows to unit norm
            ldbl s2 = 0.0L;
            for (int j = 0; j < P; ++j) s2 += (ldbl)M[(size_t)i * P + j] * M[(size_t)i * P + j];
            if (!(s2 > 0.0L)) { *err = db_msg("set block %lld (IndAffine): row %d of A is zero: A needs full row rank", (long long)blk, i + 1); return FOS_EINVAL; }
            const ldbl sc = 1.0L / sqrtl(s2);
            F->scale[(size_t)i] = sc;
            for (int j = 0; j < P; ++j) W[(size_t)i * P + j] = sc * M[(size_t)i * P + j];
        }
        std::vector<ldbl>& L = F->L;
        L.assign((size_t)mm * mm, 0.0L);
        db_par(nt, [&](int t, int n) {
            for (int i = t; i < mm; i += n)
                for (int j = 0; j <= i; ++j) {
                    ldbl v = 0.0L;
                    for (int c = 0; c < P; ++c) v += W[(size_t)i * P + c] * W[(size_t)j * P + c];
                    L[(size_t)i * mm + j] = v;
                }
        });
        const int bad = db_cholesky(mm, L, 0x1p-48L);
        if (bad) { *err = db_msg("set block %lld (IndAffine): the pivot of row %d of A A' (rows scaled to unit norm) is not above 2^-48: A needs full row rank", (long long)blk, bad); return FOS_EINVAL; }
        db_par(nt, [&](int t, int n) {                             // W = L^-1 As, row by row; a thread owns the columns j0 .. j1 - 1
            const int j0 = (int)((int64_t)P * t / n), j1 = (int)((int64_t)P * (t + 1) / n);
            for (int i = 0; i < mm; ++i) {
                ldbl* wi = &W[(size_t)i * P];
                for (int c = 0; c < i; ++c) {
                    const ldbl l = L[(size_t)i * mm + c];
                    const ldbl* wc = &W[(size_t)c * P];
                    for (int j = j0; j < j1; ++j) wi[j] -= l * wc[j];
                }
                const ldbl inv = 1.0L / L[(size_t)i * mm + i];
                for (int j = j0; j < j1; ++j) wi[j] *= inv;
            }
        });
        db_par(nt, [&](int t, int n) {                             // G = I - W'W, the lower triangle mirrored; a thread owns the rows i = t, t + n, ...
            std::vector<ldbl> acc((size_t)P);
            for (int i = t; i < P; i += n) {
                std::fill(acc.begin(), acc.begin() + i + 1, 0.0L);
                for (int r = 0; r < mm; ++r) {
                    const ldbl* wr = &W[(size_t)r * P];
                    const ldbl wi = wr[i];
                    for (int j = 0; j <= i; ++j) acc[(size_t)j] += wi * wr[j];
                }
                for (int j = 0; j <= i; ++j) {
                    const double g = (double)((i == j ? 1.0L : 0.0L) - acc[(size_t)j]);
                    F->G[(size_t)i * P + j] = F->G[(size_t)j * P + i] = g;
                }
            }
        });
        return FOS_OK;
    }
    std::vector<ldbl> Mx((size_t)P * P, 0.0L);
    if (kind == FOS_FN_BLK_QUADRATIC) {
        for (int i = 0; i < P; ++i)
            for (int j = 0; j <= i; ++j) Mx[(size_t)i * P + j] = (ldbl)M[(size_t)i * P + j] + (i == j ? 1.0L : 0.0L);
    } else {                                                       // I + lambda A'A, accumulated row of A by row of A
        db_par(nt, [&](int t, int n) {
            for (int i = t; i < P; i += n) {
                ldbl* mi = &Mx[(size_t)i * P];
                for (int64_t r = 0; r < m; ++r) {
                    const double* ar = M + r * p;
                    const ldbl ai = ar[i];
                    if (ai == 0.0L) continue;
                    for (int j = 0; j <= i; ++j) mi[j] += ai * ar[j];
                }
                for (int j = 0; j <= i; ++j) mi[j] = (ldbl)lambda * mi[j] + (i == j ? 1.0L : 0.0L);
            }
        });
    }
    const int bad = db_cholesky(P, Mx, 0.0L);
    if (bad) {
        *err = db_msg("set block %lld (%s): the pivot of column %d of I + %s is not a positive finite number%s", (long long)blk, name, bad,
                      kind == FOS_FN_BLK_QUADRATIC ? "Q" : "lambda A'A", kind == FOS_FN_BLK_QUADRATIC ? " (Q must be positive semidefinite)" : "");
        return FOS_EINVAL;
    }
    // K = L^-1 (lower triangular), row by row, stored over a fresh array; G = K'K
    std::vector<ldbl> K((size_t)P * P, 0.0L);
    db_par(nt, [&](int t, int n) {                                 // a thread owns the columns j = t, t + n, ... (column j is a forward substitution of its own)
        for (int i = 0; i < P; ++i) {
            ldbl* ki = &K[(size_t)i * P];
            if (i % n == t) ki[i] = 1.0L;
            for (int c = 0; c < i; ++c) {
                const ldbl l = Mx[(size_t)i * P + c];
                const ldbl* kc = &K[(size_t)c * P];
                for (int j = t; j <= c; j += n) ki[j] -= l * kc[j];
            }
            const ldbl inv = 1.0L / Mx[(size_t)i * P + i];
            for (int j = t; j <= i; j += n) ki[j] *= inv;
        }
    });
    std::vector<ldbl>& Gl = F->Gl;
    Gl.assign((size_t)P * P, 0.0L);
    db_par(nt, [&](int t, int n) {                                 // G(i, j) = sum_r K(r, i) K(r, j), r >= i >= j; a thread owns the rows i = t, t + n, ...
        for (int i = t; i < P; i += n) {
            ldbl* gi = &Gl[(size_t)i * P];
            for (int r = i; r < P; ++r) {
                const ldbl* kr = &K[(size_t)r * P];
                const ldbl ki = kr[i];
                for (int j = 0; j <= i; ++j) gi[j] += ki * kr[j];
            }
        }
    });
    for (int i = 0; i < P; ++i)
        for (int j = 0; j <= i; ++j) {
            Gl[(size_t)j * P + i] = Gl[(size_t)i * P + j];
            F->G[(size_t)i * P + j] = F->G[(size_t)j * P + i] = (double)Gl[(size_t)i * P + j];
        }
    return FOS_OK;
}

// d of one block from its vector v (q: p entries; b: m entries; nullptr: zeros), in long double, rounded once
int db_offset(int64_t blk, const DbFactor& F, const double* v, double* d, std::string* err) {
    const int P = F.p, mm = F.m;
    const int nv = F.kind == FOS_FN_BLK_QUADRATIC ? P : mm;
    if (!v) { std::fill(d, d + P, 0.0); return FOS_OK; }
    for (int i = 0; i < nv; ++i)
        if (!db_fin(v[i])) { *err = db_msg("set block %lld (%s): entry %d of its vector is not finite", (long long)blk, db_kind_name(F.kind), i + 1); return FOS_EINVAL; }
    if (F.kind == FOS_SET_BLK_AFFINE) {                            // d = W' L^-1 bs
        std::vector<ldbl> u((size_t)mm);
        for (int i = 0; i < mm; ++i) {
            ldbl s = F.scale[(size_t)i] * v[i];
            for (int c = 0; c < i; ++c) s -= F.L[(size_t)i * mm + c] * u[(size_t)c];
            u[(size_t)i] = s / F.L[(size_t)i * mm + i];
        }
        std::vector<ldbl> acc((size_t)P, 0.0L);
        for (int r = 0; r < mm; ++r) {
            const ldbl* wr = &F.W[(size_t)r * P];
            for (int j = 0; j < P; ++j) acc[(size_t)j] += u[(size_t)r] * wr[j];
        }
        for (int j = 0; j < P; ++j) d[j] = (double)acc[(size_t)j];
        return FOS_OK;
    }
    std::vector<ldbl> rhs((size_t)P, 0.0L);
    if (F.kind == FOS_FN_BLK_QUADRATIC) {
        for (int j = 0; j < P; ++j) rhs[(size_t)j] = -(ldbl)v[j];
    } else {                                                       // lambda A'b
        for (int r = 0; r < mm; ++r) {
            const double* ar = F.M + (size_t)r * P;
            const ldbl br = (ldbl)F.lambda * v[r];
            for (int j = 0; j < P; ++j) rhs[(size_t)j] += br * ar[j];
        }
    }
    for (int i = 0; i < P; ++i) {
        const ldbl* gi = &F.Gl[(size_t)i * P];
        ldbl s = 0.0L;
        for (int j = 0; j < P; ++j) s += gi[j] * rhs[(size_t)j];
        d[i] = (double)s;
    }
    return FOS_OK;
}

// the shapes a dense block accepts: FOS_OK or the message
int db_check_shape(int64_t blk, int kind, int64_t len, int64_t m, int64_t c, double lambda, std::string* err) {
    const char* name = db_kind_name(kind);
    if (len > DB_MAX) {
        *err = db_msg("set block %lld (%s): a dense block holds at most %d entries, this one %lld: use the whole-vector form of %s for a longer one", (long long)blk, name,
                      DB_MAX, (long long)len, name);
        return FOS_EINVAL;
    }
    if (m < 1 || c < 1) { *err = db_msg("set block %lld (%s): its matrix is %lld x %lld", (long long)blk, name, (long long)m, (long long)c); return FOS_EINVAL; }
    if (kind == FOS_FN_BLK_QUADRATIC && (m != len || c != len)) {
        *err = db_msg("set block %lld (Quadratic): Q is %lld x %lld, the block has %lld entries", (long long)blk, (long long)m, (long long)c, (long long)len);
        return FOS_EINVAL;
    }
    if (kind != FOS_FN_BLK_QUADRATIC && c != len) {
        *err = db_msg("set block %lld (%s): A has %lld columns, the block has %lld entries", (long long)blk, name, (long long)c, (long long)len);
        return FOS_EINVAL;
    }
    if (kind == FOS_SET_BLK_AFFINE && m > len) {
        *err = db_msg("set block %lld (IndAffine): A is %lld x %lld: m <= p is required (A needs full row rank)", (long long)blk, (long long)m, (long long)c);
        return FOS_EINVAL;
    }
    if (kind == FOS_FN_BLK_LEAST_SQUARES && (!(lambda > 0.0) || !db_fin(lambda))) {
        *err = db_msg("set block %lld (LeastSquares): lambda must be finite and > 0", (long long)blk);
        return FOS_EINVAL;
    }
    return FOS_OK;
}

}  // namespace

bool dense_block_kind(int kind) { return kind == FOS_FN_BLK_QUADRATIC || kind == FOS_SET_BLK_AFFINE || kind == FOS_FN_BLK_LEAST_SQUARES; }

struct DenseBlocks : DevOwned {
    DenseBlocks() { what = "fos_feas_set_blocks2"; }
    struct Mat { int64_t goff; int p; bool square, in_lds; };                           // a distinct (matrix, kind, lambda)
    struct Blk { int64_t index, start, doff; int mat; };           // a dense block: its place among all blocks, in x, in d
    std::vector<Mat> mats;
    std::vector<Blk> blks;
    int nwave_blocks = 0, nwg_blocks = 0, nwave_items = 0, nwg_items = 0, lds_blocks = 0, pmax = 0;
    size_t wg_lds = 0, gbytes = 0;
    DbItem *d_wave_items = nullptr, *d_wg_items = nullptr;
    DbSlot* d_slots = nullptr;
    int32_t* d_run = nullptr;
    DbBlock* d_blocks = nullptr;
    double *d_G = nullptr, *d_d = nullptr;
};

void dense_blocks_free(DenseBlocks* p) { delete p; }
int dense_blocks_launches(const DenseBlocks* p) { return p ? (p->nwave_items > 0) + (p->nwg_items > 0) : 0; }

// kind / len / start: all nblocks blocks of the sum.  *out stays nullptr when the sum holds no dense block.
int dense_blocks_setup(int64_t nblocks, const int32_t* kind, const int64_t* len, const int64_t* start, const double* scal, const DenseBlockArgs& a, DenseBlocks** out) {
    *out = nullptr;
    if (a.nmat < 0 || (a.nmat > 0 && (!a.mat_rows || !a.mat_cols || !a.mats))) { set_error("fos_feas_set_blocks2: nmat >= 0 and, with matrices, mat_rows, mat_cols and mats are required"); return FOS_EINVAL; }
    // ---- the blocks and their distinct (matrix, kind, lambda)
    struct Key { int64_t mat; int32_t kind; double lambda; bool operator<(const Key& o) const { return mat != o.mat ? mat < o.mat : kind != o.kind ? kind < o.kind : lambda < o.lambda; } };
    std::map<Key, int> seen;
    struct Entry { Key key; int64_t first_blk; std::vector<int> blocks; };
    std::vector<Entry> entries;
    DenseBlocks* p = new DenseBlocks();
    auto fail = [&](int code) { delete p; return code; };
    int64_t doff = 0;
    for (int64_t i = 0; i < nblocks; ++i) {
        const int64_t mi = a.block_mat[i];
        if (!dense_block_kind(kind[i])) {
            if (mi != -1) { set_error("set block %lld: kind %d is a vector kind and takes no matrix (block_mat = %lld, -1 is required)", (long long)i + 1, (int)kind[i], (long long)mi); return fail(FOS_EINVAL); }
            continue;
        }
        if (mi < 0) { set_error("set block %lld (%s): a dense kind needs a matrix (block_mat = %lld)", (long long)i + 1, db_kind_name(kind[i]), (long long)mi); return fail(FOS_EINVAL); }
        if (mi >= a.nmat) { set_error("set block %lld (%s): matrix index %lld is out of range (nmat = %lld)", (long long)i + 1, db_kind_name(kind[i]), (long long)mi, (long long)a.nmat); return fail(FOS_EINVAL); }
        if (!a.mats[mi]) { set_error("set block %lld (%s): matrix %lld is NULL", (long long)i + 1, db_kind_name(kind[i]), (long long)mi); return fail(FOS_EINVAL); }
        const double lambda = kind[i] == FOS_FN_BLK_LEAST_SQUARES ? scal[2 * i] : 0.0;
        std::string err;
        if (db_check_shape(i + 1, kind[i], len[i], a.mat_rows[mi], a.mat_cols[mi], lambda, &err) != FOS_OK) { set_error("%s", err.c_str()); return fail(FOS_EINVAL); }
        const Key key{mi, kind[i], lambda};
        auto it = seen.find(key);
        if (it == seen.end()) { it = seen.emplace(key, (int)entries.size()).first; entries.push_back(Entry{key, i + 1, {}}); }
        entries[(size_t)it->second].blocks.push_back((int)p->blks.size());
        p->blks.push_back(DenseBlocks::Blk{i, start[i], doff, it->second});
        doff += len[i];
        p->pmax = std::max(p->pmax, (int)len[i]);
    }
    if (p->blks.empty()) { delete p; return FOS_OK; }
    // storage per matrix: the packed triangle where it is staged in LDS (every order up to 64; a larger one while it fits beside x), the full square above that --
    // measured on the MI355X (profiles/dense_blocks_bench.json): packed 92 against 159 us at 10^4 blocks of order 64, 433 against 146 us at 10^3 of order 256, where
    // the triangle is read through the caches.  FOS_DENSE_BLOCKS_SQUARE = 1 | 0 at set-up forces the square | the triangle everywhere (measurements)
    int force = -1;
    { const char* e = std::getenv("FOS_DENSE_BLOCKS_SQUARE"); if (e && (e[0] == '0' || e[0] == '1')) force = e[0] - '0'; }
    size_t lds_cap = DB_LDS_BYTES;
    {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0) lds_cap = std::min<size_t>(lds_cap, (size_t)v);
    }
    // ---- G of every distinct matrix and d of every block, on the pool
    int64_t goff = 0;
    for (const Entry& e : entries) {
        const int P = (int)a.mat_cols[e.key.mat];
        const bool fits = P <= DB_WAVE_MAX || sizeof(double) * ((size_t)((P + 1) & ~1) + (size_t)P * (P + 1) / 2) <= lds_cap;
        const bool square = force >= 0 ? force == 1 : !fits;
        p->mats.push_back(DenseBlocks::Mat{goff, P, square, !square && fits});
        goff += square ? (int64_t)P * P : (int64_t)P * (P + 1) / 2;
    }
    std::vector<double> hG((size_t)goff), hd((size_t)doff);
    std::vector<std::string> errs(entries.size());
    std::vector<int64_t> err_blk(entries.size(), 0);
    std::atomic<int> next{0};
    const int nthreads = (int)std::min<size_t>(DB_POOL, entries.size()), inner = DB_POOL / nthreads;      // outer x inner <= DB_POOL threads
    auto work = [&]() {
        for (;;) {
            const int e = next.fetch_add(1);
            if (e >= (int)entries.size()) break;
            const Entry& en = entries[(size_t)e];
            DbFactor F;
            if (db_factor(en.first_blk, en.key.kind, a.mat_rows[en.key.mat], a.mat_cols[en.key.mat], a.mats[en.key.mat], en.key.lambda, inner, &F, &errs[(size_t)e]) != FOS_OK) { err_blk[(size_t)e] = en.first_blk; continue; }
            const int P = F.p;
            double* g = hG.data() + p->mats[(size_t)e].goff;
            if (p->mats[(size_t)e].square) std::copy(F.G.begin(), F.G.end(), g);
            else for (int i = 0; i < P; ++i) for (int j = 0; j <= i; ++j) g[db_tri(i, j)] = F.G[(size_t)i * P + j];
            for (int bi : en.blocks) {
                const DenseBlocks::Blk& b = p->blks[(size_t)bi];
                if (db_offset(b.index + 1, F, a.block_vec ? a.block_vec[b.index] : nullptr, hd.data() + b.doff, &errs[(size_t)e]) != FOS_OK) { err_blk[(size_t)e] = b.index + 1; break; }
            }
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; ++t) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
    }
    {
        int worst = -1;                                            // the refusal of the lowest block
        for (size_t e = 0; e < entries.size(); ++e) if (err_blk[e] && (worst < 0 || err_blk[e] < err_blk[(size_t)worst])) worst = (int)e;
        if (worst >= 0) { set_error("%s", errs[(size_t)worst].c_str()); return fail(FOS_EINVAL); }
    }
    // ---- runs of up to DB_RUN blocks of one matrix; wavefront-class runs packed 64 / T to a workgroup
    std::vector<DbSlot> slots;
    std::vector<int32_t> run;
    std::vector<DbBlock> dblocks(p->blks.size());
    for (size_t b = 0; b < p->blks.size(); ++b) dblocks[b] = DbBlock{p->blks[b].start, p->blks[b].doff};
    std::vector<int> wave_slots, wg_slots;
    for (size_t e = 0; e < entries.size(); ++e) {
        const int P = p->mats[e].p;
        const int in_lds = p->mats[e].in_lds, square = p->mats[e].square;
        for (size_t k = 0; k < entries[e].blocks.size(); k += DB_RUN) {
            const int cnt = (int)std::min<size_t>(DB_RUN, entries[e].blocks.size() - k);
            (P <= DB_WAVE_MAX ? wave_slots : wg_slots).push_back((int)slots.size());
            slots.push_back(DbSlot{p->mats[e].goff, P, cnt, (int32_t)run.size(), in_lds, square, 0});
            for (int c = 0; c < cnt; ++c) run.push_back(entries[e].blocks[k + (size_t)c]);
            (P <= DB_WAVE_MAX ? p->nwave_blocks : p->nwg_blocks) += cnt;
            if (in_lds) p->lds_blocks += cnt;
        }
    }
    // the device walks slots through an order table: slot_order[item.first_slot + sub]
    std::vector<DbSlot> ordered;
    std::vector<DbItem> wave_items, wg_items;
    auto team_of = [](int P) { int T = 1; while (T < P) T <<= 1; return T; };
    std::stable_sort(wave_slots.begin(), wave_slots.end(), [&](int x, int y) { return team_of(slots[(size_t)x].p) < team_of(slots[(size_t)y].p); });
    for (size_t k = 0; k < wave_slots.size();) {
        const int T = team_of(slots[(size_t)wave_slots[k]].p), cap = 64 / T;
        DbItem it{(int32_t)ordered.size(), 0, T, 0};
        while (k < wave_slots.size() && it.nslots < cap && team_of(slots[(size_t)wave_slots[k]].p) == T) {
            const DbSlot& s = slots[(size_t)wave_slots[k]];
            ordered.push_back(s); it.nslots += 1; it.maxrun = std::max(it.maxrun, s.nblk); ++k;
        }
        wave_items.push_back(it);
    }
    for (int si : wg_slots) {
        const DbSlot& s = slots[(size_t)si];
        wg_items.push_back(DbItem{(int32_t)ordered.size(), 1, DB_WG_THREADS, s.nblk});
        ordered.push_back(s);
        p->wg_lds = std::max(p->wg_lds, sizeof(double) * ((size_t)((s.p + 1) & ~1) + (s.in_lds ? (size_t)s.p * (s.p + 1) / 2 : 0)));
    }
    p->nwave_items = (int)wave_items.size(); p->nwg_items = (int)wg_items.size();
    p->gbytes = sizeof(double) * hG.size();
    const hipStream_t sync = nullptr;
    int rc = p->upload(&p->d_G, hG, sync);
    if (rc == FOS_OK) rc = p->upload(&p->d_d, hd, sync);
    if (rc == FOS_OK) rc = p->upload(&p->d_slots, ordered, sync);
    if (rc == FOS_OK) rc = p->upload(&p->d_run, run, sync);
    if (rc == FOS_OK) rc = p->upload(&p->d_blocks, dblocks, sync);
    if (rc == FOS_OK && p->nwave_items > 0) rc = p->upload(&p->d_wave_items, wave_items, sync);
    if (rc == FOS_OK && p->nwg_items > 0) rc = p->upload(&p->d_wg_items, wg_items, sync);
    if (rc != FOS_OK) return fail(rc);
    if (p->wg_lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(dense_blocks_wg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap) != hipSuccess) {
        set_error("fos_feas_set_blocks2: %zu bytes of LDS per workgroup are not available on this device", lds_cap);
        return fail(FOS_EUNSUPPORTED);
    }
    *out = p;
    return FOS_OK;
}

// the dense blocks of y = prox(x): one launch per class present; the caller checks hipGetLastError
void dense_blocks_prox(const DenseBlocks* p, hipStream_t stream, double* y, const double* x) {
    if (p->nwave_items > 0)
        hipLaunchKernelGGL(dense_blocks_wave_kernel, dim3(p->nwave_items), dim3(64), 0, stream, (const DbItem*)p->d_wave_items, (const DbSlot*)p->d_slots,
                           (const int32_t*)p->d_run, (const DbBlock*)p->d_blocks, (const double*)p->d_G, (const double*)p->d_d, x, y);
    if (p->nwg_items > 0)
        hipLaunchKernelGGL(dense_blocks_wg_kernel, dim3(p->nwg_items), dim3(DB_WG_THREADS), p->wg_lds, stream, (const DbItem*)p->d_wg_items, (const DbSlot*)p->d_slots,
                           (const int32_t*)p->d_run, (const DbBlock*)p->d_blocks, (const double*)p->d_G, (const double*)p->d_d, x, y);
}

// out8: dense blocks, distinct matrices, wavefront-class blocks, workgroup-class blocks, launches, bytes of G kept, largest order, blocks served from a matrix in LDS
void dense_blocks_stats(const DenseBlocks* p, double* out8) {
    out8[0] = (double)p->blks.size(); out8[1] = (double)p->mats.size(); out8[2] = p->nwave_blocks; out8[3] = p->nwg_blocks;
    out8[4] = dense_blocks_launches(p); out8[5] = (double)p->gbytes; out8[6] = p->pmax; out8[7] = p->lds_blocks;
}

// block: 0-based among ALL blocks of the sum; G: p x p, the square; d: p -- read back from the device
int dense_blocks_get(const DenseBlocks* p, int64_t block, double* G, double* d) {
    for (const DenseBlocks::Blk& b : p->blks) {
        if (b.index != block) continue;
        const DenseBlocks::Mat& m = p->mats[(size_t)b.mat];
        const int P = m.p;
        std::vector<double> g(m.square ? (size_t)P * P : (size_t)P * (P + 1) / 2);
        FOS_HIP(hipMemcpy(g.data(), p->d_G + m.goff, sizeof(double) * g.size(), hipMemcpyDeviceToHost));
        FOS_HIP(hipMemcpy(d, p->d_d + b.doff, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost));
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j) G[(size_t)i * P + j] = m.square ? g[(size_t)i * P + j] : g[(size_t)db_tri(i, j)];
        return FOS_OK;
    }
    set_error("fos_feas_dense_block_get: block %lld is not a dense block of this sum", (long long)block);
    return FOS_EINVAL;
}

}  // namespace fos

using namespace fos;

extern "C" {

// Test-only host emulation of one dense block (no GPU needed): the set-up above, then y = G x + d by the kernels' chain (one order for every class)
int fos_host_dense_block(int32_t kind, int64_t m, int64_t p, const double* M, const double* v, double lambda, const double* x, double* y, double* G_out, double* d_out) {
    if (!dense_block_kind(kind)) { set_error("fos_host_dense_block: kind %d is not a dense block kind (FOS_FN_BLK_QUADRATIC, FOS_SET_BLK_AFFINE, FOS_FN_BLK_LEAST_SQUARES)", (int)kind); return FOS_EINVAL; }
    if (!M || !x || !y || p < 1) { set_error("fos_host_dense_block: M, x, y and p >= 1 are required"); return FOS_EINVAL; }
    std::string err;
    if (db_check_shape(1, kind, p, m, p, lambda, &err) != FOS_OK) { set_error("%s", err.c_str()); return FOS_EINVAL; }
    DbFactor F;
    std::vector<double> d((size_t)p);
    if (db_factor(1, kind, m, p, M, kind == FOS_FN_BLK_LEAST_SQUARES ? lambda : 0.0, DB_POOL, &F, &err) != FOS_OK || db_offset(1, F, v, d.data(), &err) != FOS_OK) { set_error("%s", err.c_str()); return FOS_EINVAL; }
    for (int64_t r = 0; r < p; ++r) {
        double acc = d[(size_t)r];
        for (int64_t j = 0; j < p; ++j) acc = std::fma(F.G[(size_t)(r * p + j)], x[j], acc);
        y[r] = acc;
    }
    if (G_out) std::copy(F.G.begin(), F.G.end(), G_out);
    if (d_out) std::copy(d.begin(), d.end(), d_out);
    return FOS_OK;
}

}  // extern "C"
