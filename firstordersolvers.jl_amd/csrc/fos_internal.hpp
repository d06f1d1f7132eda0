// Internal declarations of libfoship (not part of the ABI).
//
// Device data layout (DESIGN.md "Data layout in HBM"):
//   * every N-vector of the reference (N = 2l, l = n+m+1, layout [x;y;tau;r;s;kappa]) lives on the device
//     as l `double2` elements, INTERLEAVED:  v[i] = (part1[i], part2[i])  with part1 = [x;y;tau],
//     part2 = [r;s;kappa].  All CG / relaxation kernels are elementwise or reductions, so the layout is
//     free; interleaving makes the dual-right-hand-side KKT SpMV gather ONE 16-byte element per non-zero and
//     lets one cone workgroup project the primal and the dual copy of a cone from the same loads.
//   * the operator is stored once as the stacked matrix S = [[0, A'],[A, 0]] ((n+m) x (n+m)) in a
//     block-padded CSR (fp64 values, int32 columns into the stacked vector [x(n); y(m)]).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "foship.h"
#include "sparse_rows.hpp"

namespace fos {

// ---------------------------------------------------------------------------------- errors (set_error, FOS_TRY: sparse_rows.hpp)
#define FOS_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::fos::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return FOS_EHIP;                                                                  \
        }                                                                                     \
    } while (0)

// ---------------------------------------------------------------------------------- SpMV storage
constexpr int SPMV_THREADS = 256;   // 4 independent wavefronts per workgroup
constexpr int SPMV_WAVES = SPMV_THREADS / 64;
constexpr int WNNZ = 256;           // LDS-staged row block: max non-zeros (16 B each for 2 RHS in the wavefront's LDS slice)
constexpr int ELL_MAX = 2048;       // lane-major ("ELL") row block: max padded entries (a multiple of 64)
constexpr int WROWS = 64;           // max rows per row block (>= 1 epilogue lane per row)
constexpr int LONG_ROWS = 4;        // long run-rows over one column range handled together by a wavefront
constexpr int NNZ_ALIGN = 4;        // every row block starts at a multiple of 4 entries (16/32-byte aligned)

enum BlkKind : int32_t { BLK_LDS = 0, BLK_ELL = 1, BLK_LONG = 2, BLK_TILE = 3 };

// Dual tiles (BLK_TILE).  A dense rectangle of A -- R <= 64 consecutive rows whose non-zeros are the SAME run of
// consecutive columns -- is stored ONCE, lane-major (lane = row, step = column), and serves both products of the
// stacked operator in one pass: the row sums (A x) stay in the lanes, the column sums (A'y) are formed by an
// in-register butterfly over 8 steps at a time and written as PARTIALS to a slot array; the A' entries the tile
// covers are not stored at all.  Rows of S whose sum is spread over several tiles (columns of A covered by tiles;
// rows of A wider than TILE_TC_MAX columns) are DEFERRED: a second small kernel adds their partial slots in a fixed
// order and runs the row epilogue.  Halves the matrix bytes of dense operators (C2, C4).
constexpr int TILE_MIN_ROWS = 16;   // fewer rows: not worth a 64-lane wavefront
constexpr int TILE_MIN_COLS = 8;
constexpr int TILE_TC_MAX = 64;     // columns (steps) per tile: 32 KB of values per wavefront work unit (measured best on C2: 32..128 tried)
constexpr int TILE_GROUP = 8;       // steps per butterfly; stored steps are padded to a multiple
constexpr int TILE_TALL_MAX = 16;   // sub-tiles a tall tile may stack (5 bits in the descriptor)

// Window panels (gather-bound random-sparse operators, C5 class).  A PANEL = WIN_ROWS consecutive rows of S, the unit of
// work of ONE WORKGROUP (two of them share a CU), which walks the column WINDOWS (WIN_COLS consecutive entries of the stacked vector) its rows touch:
// the window is staged in LDS by coalesced loads, the panel's non-zeros inside it are multiplied against LDS (no 128-byte L1
// line fill per 16-byte gather: the bound of the row-block formats on such operators), and the row sums are kept in LDS across
// the windows.  Inside a (panel, window) SEGMENT the rows that have entries there are sorted by their entry count (SELL-sigma)
// and cut into SLICES of 64 rows stored lane-major (lane = row, step = entry; padded to the slice's longest row: ~10 %, not the
// 40-50 % of panel-wide ELL), with 16-bit column offsets inside the window and a 16-bit local row id per lane.
// Two geometries (round 4), chosen per operator at fos_create (csr_build.cpp, window_geometry):
//   WinStd   2016-row panels, windows of <= 3072 columns, 512 threads, TWO workgroups per CU (2 x 80 KB of LDS);
//   WinTall  4032-row panels, windows of <= 6144 columns, 1024 threads, ONE workgroup per CU (160 KB): four times the entries per
//            segment against the same fixed cost of a segment (its memory latency, two barriers) and half the window bytes per entry
//            -- C5 sweep 96.6 -> 89.2 us -- for operators with enough rows to give (nearly) every CU a panel.
struct WinStd {
    static constexpr int COLS = 3072, ROWS = 2016, THREADS = 512, WG_PER_CU = 2, WAVES = THREADS / 64;
    // steps of a wavefront's slice u (descending step counts) requested with the window, so that one memory latency covers the window
    // and the matrix; the rest -- and, here, a fourth slice -- is streamed behind the barriers
    static constexpr int PRE0 = 6, PRE1 = 6, PRE2 = 6, PRE3 = 0;
    static constexpr bool PREFETCH = false;
    static constexpr bool PIPELINE = false;
};
struct WinTall {
    static constexpr int COLS = 6144, ROWS = 4032, THREADS = 1024, WG_PER_CU = 1, WAVES = THREADS / 64;
    static constexpr int PRE0 = 8, PRE1 = 4, PRE2 = 2, PRE3 = 2;
#ifdef FOS_WIN_PREFETCH
    static constexpr bool PREFETCH = FOS_WIN_PREFETCH != 0;   // the next segment's window requested behind this segment's second barrier (one workgroup per CU: nobody else fills the bubble)
#else
    static constexpr bool PREFETCH = true;
#endif
#ifdef FOS_WIN_PIPELINE
    static constexpr bool PIPELINE = FOS_WIN_PIPELINE != 0;   // slot-level software pipeline over the segments (kernels.hip, win_walk)
#else
    static constexpr bool PIPELINE = true;
#endif
};
static_assert((WinStd::ROWS + 64 * WinStd::WAVES - 1) / (64 * WinStd::WAVES) <= 4 && (WinTall::ROWS + 64 * WinTall::WAVES - 1) / (64 * WinTall::WAVES) <= 4,
              "a WinDesc holds the step counts of four slices per wavefront");
struct WinGeomRt { int32_t rows, cols, waves, wg_per_cu; };       // the same numbers for the host-side builder / emulation
constexpr WinGeomRt WIN_GEOM_STD = {WinStd::ROWS, WinStd::COLS, WinStd::WAVES, WinStd::WG_PER_CU};
constexpr WinGeomRt WIN_GEOM_TALL = {WinTall::ROWS, WinTall::COLS, WinTall::WAVES, WinTall::WG_PER_CU};
// Storage = WAVE STREAMS (round 4).  Slice j of a segment (slices in descending step count) belongs to wavefront j % WIN_WAVES; everything
// one wavefront reads of a panel -- its slices' values / column offsets / row words, segment after segment -- is CONTIGUOUS, so the
// wavefront walks it with a running offset, and what it has to be told per segment (the window and the step counts of its <= 4
// slices) is one 16-byte record, all records of a panel loaded in ONE request at the panel's start (lane k holds segment k's record,
// read back by v_readlane): no dependent descriptor load sits in front of a segment's memory requests any more (the round-3 form paid
// two scalar round trips -- segment, then slice descriptor -- before the slice loads of EVERY segment could be issued).
struct WinPanel { int32_t row0, nrows, seg0, nseg; };      // seg0: first record of wavefront 0 in wdesc; wavefront w: seg0 + w * nseg
struct WinWave { int64_t off; int32_t slice0, pad; };       // per (panel, wavefront): first value / column offset (multiple of 64), first row-word slice
struct WinDesc { uint32_t col0, t01, t23, ncols; };         // per (panel, wavefront, segment): the window [col0, col0 + ncols) of the stacked vector; steps of the
                                                            // wavefront's slices u = 0..3 (16 bits each, 0: no such slice; descending).  Values at off + 64 t + lane,
                                                            // then the next slice.  Windows are cut PER PANEL: the span of the panel's columns in equal parts of at most
                                                            // COLS columns (C5: every panel of a block gets 21 -- tall: 11 -- equally filled segments; a global grid gave
                                                            // some panels one more, nearly empty one, and the sweep lasts as long as its slowest panel).


// One slot-spread row and its list of partial-sum slots, in summation order: [its own partial `own` (>= 0) from the sweep] followed
// by `count` tile partials, which for regular tilings form an arithmetic progression base + k * stride (dense blocks: one slot
// per tile below each other) -- then the kernels compute the slot numbers instead of loading them (one memory round trip less
// in the kernels that add the lists: they sit on the latency chain of every CG iteration); stride == DEF_EXPLICIT: the slot
// numbers are def_idx[kidx + k].
constexpr int32_t DEF_EXPLICIT = INT32_MIN;
struct DefRow { int32_t row, own, base, stride, count, kidx, pad0, pad1; };     // 32 bytes

struct BlkDesc {                    // one row block = the unit of work of ONE wavefront (48 bytes, wave-uniform: read by scalar loads)
    int64_t nnz0;                   // first value in `val` (multiple of NNZ_ALIGN)
    int64_t colpos;                 // first entry in `col`: per-entry column indices, or -- for a RUN block, whose rows
                                    // all have consecutive columns -- one first-column per row (index compression)
    int64_t cnt;                    // stored values (ELL: 64 * steps, padding included; LONG: entries per row, rows at stride align4(cnt))
    int32_t row0;                   // first row
    int32_t info;                   // nrows (bits 0..7; dual tile: rows of its LAST sub-tile) | kind << 8 | run << 10 | sub-tiles of a
                                    // tall dual tile << 11 (5 bits) | ELL steps T << 16
    int32_t meta[4];                // dual tile: first column, column-slot base, row-slot base (-1: none), real columns -- in the
                                    // descriptor so that a tile costs ONE dependent load before its values, not two (0 otherwise)
    __host__ __device__ int nrows() const { return info & 0xFF; }
    __host__ __device__ int kind() const { return (info >> 8) & 0x3; }
    __host__ __device__ int run() const { return (info >> 10) & 0x1; }
    __host__ __device__ int steps() const { return (info >> 16) & 0xFFFF; }
    __host__ __device__ int tall() const { return (info >> 11) & 0x1F; }
};

// Host-side result of building the stacked operator; uploaded verbatim.
struct HostBlkCsr {
    int64_t nrows = 0, nnz = 0, nnz_padded = 0, ncol_stored = 0;
    std::vector<double> val;
    std::vector<int32_t> col;
    std::vector<BlkDesc> blk;          // [nblk]
    std::vector<uint16_t> row_rel;     // [nrows]  row start relative to its block's nnz0 (stream blocks)
    std::vector<int32_t> wave_blk0;    // [nwaves+1]  row blocks owned by each wavefront of the grid
    std::vector<BlkDesc> wave_first;   // [nwaves]    blk[wave_blk0[w]] (zero for a wavefront without blocks)
    int32_t tile_tmax = 0;             // longest dual tile, in steps (0: no tile)
    int32_t nblk = 0, nwg = 0, nwaves = 0;
    // dual tiles / deferred rows (empty when the operator has no tile)
    int64_t nslots = 0;                // partial-sum slots (2 doubles each)
    int64_t ntiles = 0, tile_values = 0;
    std::vector<int32_t> row_defer;    // [nrows] -1: epilogue in the sweep; >= 0: the sweep stores the row's own partial in that
                                       // slot; -2: deferred, no entries outside tiles (the sweep never sees the row)
    std::vector<int32_t> def_rows;     // [ndef]   deferred rows, ascending
    std::vector<int32_t> def_ptr;      // [ndef+1] their slot lists
    std::vector<int32_t> def_idx;      // slot indices, in summation order
    std::vector<DefRow> def_rec;       // [ndef]   the same lists in the form the kernels read (progressions where they are ones)
    bool row_sharded = false;          // every row of A' is deferred: the single slot `row`, or -- with dual tiles -- its local slot list (summed over the ranks before use)
    // window panels (empty unless the operator is stored that way; then blk is empty and val/col are unused)
    std::vector<WinPanel> wpanel;
    WinGeomRt wgeom = WIN_GEOM_STD;    // geometry the panels were built for
    std::vector<WinWave> wwave;        // [npanel * waves]
    std::vector<WinDesc> wdesc;        // [sum over panels of waves * nseg]
    int64_t wnslice = 0;               // slices stored
    std::vector<double> wval;
    std::vector<uint16_t> wcol;        // column offset inside the window, per stored entry
    std::vector<uint16_t> wrow;        // [nslice * 64] local row of each lane (0xFFFF: no row)
};

struct DevBlkCsr {
    int64_t nrows, nnz, nnz_padded;
    const double* val;
    const int32_t* col;
    const BlkDesc* blk;
    const uint16_t* row_rel;
    const int32_t* wave_blk0;
    const BlkDesc* wave_first;         // [nwaves] copy of each wavefront's first descriptor (requested together with wave_blk0)
    int32_t resident;                  // 1: the whole operator stays in the caches from sweep to sweep -- ordinary loads for the matrix stream
    int32_t dbg_flags;                 // timing experiments only (FOS_DBG_FLAGS; WRONG results): 1 = dual tiles skip the column-sum butterflies;
                                       // cg_update_kernel: 4 = slot-spread rows left unfinished, 16 = scalar prologue only, 32 = no prologue
                                       // (sums taken from the first record); bits 8-10 = elements requested in front of its prologue (1..4)
    int32_t nblk, nwg, nwaves;
    // dual tiles / deferred rows (ndef == 0: none)
    double* slots;                     // [nslots][2]   written by the sweeps
    const double* slots_rd;            // what the slot-list sums read: == slots, or -- row-sharded operators -- the all-reduced copy
                                       // (with dual tiles: [n summed rows of A' | the sweep's slot array], solver.cpp cmp_rec)
    const int32_t* row_defer;          // nullptr when ndef == 0
    const int32_t* def_rows;
    const int32_t* def_ptr;
    const int32_t* def_idx;
    const DefRow* def_rec;
    int32_t ndef, nwg_def;             // deferred rows, workgroups of the deferred-row kernel
    int32_t def_lpr;                   // lanes per deferred row (power of two <= 64)
    int32_t npart, part_off;           // the partial-sum records a sweep leaves for its consumers: `npart` records starting at
                                       // record `part_off` (no tiles: the sweep's nwg; tiles: the deferred-row kernel folds the
                                       // sweep's records into its own nwg_def, stored behind them)
    // window panels (npanel == 0: row-block storage)
    int32_t npanel;
    int32_t win_tall;                  // 1: WinTall geometry (else WinStd)
    const WinPanel* wpanel;
    const WinWave* wwave;
    const WinDesc* wdesc;
    const double* wval;
    const uint16_t* wcol;
    const uint16_t* wrow;
};

// Builds S = [[0, A'],[A, 0]] from Julia CSC (1-based).  Returns FOS_EINVAL on malformed input.
int build_stacked_csr(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                      int nwg_target, HostBlkCsr* out, int resident_waves = 0, int window_mode = -1,   // -1: decide from the operator, 0: no window panels, 1 / 2: force WinStd / WinTall
                      bool row_sharded = false, int tall_target = 0);   // tall_target: tile blocks that fit one resident round (0: 4096)
void partition_workgroups(HostBlkCsr* S, int nwg_target);
int host_stacked_spmv(const HostBlkCsr& S, const double* v, double* out, std::string* why);
constexpr int DEF_THREADS = 256;    // deferred-row kernel: one thread per deferred row
constexpr int DEF_MAX_WG = 1024;    // its grid (grid-stride beyond)
constexpr int PART_CAP = 16384 + DEF_MAX_WG + 8;   // per-workgroup partial-sum records a kernel may produce (sweep + deferred rows)

// ---------------------------------------------------------------------------------- device scalar state
// One struct in device memory; kernels read/write it, the host polls a pinned copy.
struct DevState {
    // CG  (conjugategradients.jl:31-55)
    double rn, rn_old, alpha, beta, pAp, rr, tol;
    double rn2[2];         // r.r ping-pong: CG iteration j reads rn2[j&1] and writes rn2[(j+1)&1] (lets every workgroup of the
                           // fused finalize+p-update kernel derive beta itself without racing the one that stores it)
    int32_t iter, done;    // (adjacent and 8-byte aligned: cg_pupdate_kernel reads the pair with ONE load)
    int32_t maxit, hit_max;
    int32_t xchg_failed;   // a peer-mailbox exchange timed out (PeerBox below); every later exchange is skipped
    int32_t bar_failed;    // a wait between workgroups inside a kernel timed out (cg_update_kernel's producer flags)
    // algorithm scalars
    double alpha12;        // GAPAData.alpha12 (gapa.jl:29,101)
    double gapa_scl;       // last normedScalar value (diagnostic)
    // status sums, filled by status_finalize: see StatusIdx
    double stat[12];
    // host-visible (pinned, mapped) record the kernel that ends a CG solve fills: lets the host see the end of the solve
    // without a stream synchronisation (HostMark below; 0: none)
    unsigned long long hostmark;
    // merged-reduction CG (cgm_update_kernel): the step lengths ping-pong like r.r (iteration j reads alpha2[j & 1], written by
    // the launch before, and writes alpha2[(j + 1) & 1]); vtau = the tau element of the vector the last sweep applied M to
    // (stashed by the sweep: the update kernel overwrites that vector while other workgroups still need the element)
    double alpha2[2];
    double vtau[2];
    int32_t dbg_delay;     // test hook (fos_debug_set): workgroups != 0 of cg_pupdate_kernel wait this many 100 MHz ticks at entry
    int32_t pad_;
};
static_assert(offsetof(DevState, iter) % 8 == 0 && offsetof(DevState, done) == offsetof(DevState, iter) + 4, "iter/done are read as one 64-bit word");
struct HostMark { uint32_t seq; int32_t iter; int32_t hit_max; int32_t batch; double rr; };   // seq = the solve's number, written last;
                                                                                            // batch: id of a batch of iterations that ended WITHOUT convergence

enum StatusIdx { ST_RP2 = 0, ST_RD2, ST_CTX, ST_BTY, ST_AXS2, ST_ATY2, ST_TAU, ST_KAPPA, ST_COUNT };

// ---------------------------------------------------------------------------------- cone tables
// Elementwise op per (index, part):  2 bits each.
enum EwOp : uint8_t { EW_COPY = 0, EW_ZERO = 1, EW_MAX0 = 2, EW_MIN0 = 3 };
constexpr uint8_t EW_SKIP = 0xFF;   // index belongs to a SOC / PSD cone (handled by the batched kernels)

struct ConeDesc {          // a SOC / rotated SOC / PSD cone in stacked index space [0, n+m)
    int64_t start;         // first stacked index
    int32_t len;           // number of entries
    int32_t k;             // PSD order (0 for SOC)
    int32_t dual_part;     // which part (0: part1, 1: part2) takes the DUAL projection (Moreau); the other takes the primal
    int32_t type;          // FOS_CONE_*
};

// ---------------------------------------------------------------------------------- peer mailboxes (sharded scalar sums)
// All-reduce of <= PEER_MAX_VALS doubles over <= PEER_MAX_RANKS GPUs without a collective library: every rank owns a
// mailbox in UNCACHED device memory that its peers map through HIP IPC.  An exchange (inside reduce_kernel) stores the
// rank's local sums into every peer's mailbox and polls its own until all ranks' words of this exchange have arrived,
// then adds them in rank order -- bitwise the same result on every rank.  Every 64-bit word carries its own validity:
//   word = (sequence number << 32) | 32 payload bits         (two words per double; 8-byte stores are single-copy atomic)
// so no fence or separate flag is needed.  Layout: [parity 2][source rank][value][half]; the parity of the sequence
// number selects the half a given exchange uses (a rank can be at most one exchange ahead of a peer).
constexpr int PEER_MAX_RANKS = 16;
constexpr int PEER_MAX_VALS = 8;
constexpr size_t PEER_BOX_WORDS = (size_t)2 * PEER_MAX_RANKS * PEER_MAX_VALS * 2;     // region 0; region 1 (folded exchanges, four slots) is twice that
constexpr size_t PEER_BOX_TOTAL_WORDS = 3 * PEER_BOX_WORDS;
// A mailbox has TWO such regions: region 0 for the exchanges of the single-workgroup reduce kernel (sequence = a device
// counter of executed exchanges), region 1 for the two exchanges of a CG iteration that are FOLDED into the CG vector kernels
// (every workgroup reduces the local records itself, workgroup 0 also writes them to the peers, every workgroup polls; the
// sequence number is (CG solve number, iteration, phase), known at launch, its parity = the phase).
// Second transport, HOST-PINNED mailboxes (round 5; fos_peer_open_host): the same words in ONE segment of pinned host memory (POSIX shm, registered
// by every rank with hipHostRegister) -- no peer access between the devices and no IPC handle is needed, every box[r] is that one segment
// (`shared`: a rank writes its words once, not once per peer).  A read of host memory is a PCIe round trip, so of the workgroups of a folded
// exchange only workgroup 0 polls the segment; it republishes every word it has seen in `relay`, a mailbox-shaped array in local uncached
// device memory that the other workgroups poll (the words validate themselves there as well).
struct PeerBox {
    unsigned long long* const* box;   // device table [nranks]: box[r] = mailbox of rank r (own entry: the local allocation)
    uint32_t* seq;                    // device counter of EXECUTED exchanges (gated no-op launches do not count)
    int32_t nranks, rank;
    int64_t timeout_ticks;            // wall_clock64() ticks (100 MHz) an exchange may wait for its peers
    unsigned long long* relay;        // host-pinned transport: local republication of the peers' words (nullptr: device mailboxes)
    int32_t shared;                   // 1: all box[r] are one segment
    int32_t loopback;                 // measurement (FOS_PEER_LOOPBACK=1): a rank's OWN words travel through the mailbox too, so that a single
                                      // rank pays the store -> poll latency of the transport in every folded exchange
};

// Row-sharded operators without a collective library: the n-vector exchange of HSDEAffine.jl:51 (A'y = sum over the ranks of
// A_g' y_g, both right-hand sides: 2n doubles) through peer-mapped memory.  Every rank owns a buffer [2 parities][nranks][2n]
// doubles + flags [2][nranks] in UNCACHED device memory that its peers map through HIP IPC.  An exchange = two launches:
//   push   every workgroup copies a chunk of this rank's slots into every peer's buffer (slot [parity][this rank]); the LAST
//          workgroup to finish (a local counter) raises this rank's flag in every peer's flag array with the exchange's number;
//   sum    every workgroup waits for all peers' flags of this exchange, then adds the contributions in rank order (its own from
//          the local slots) into slots_rd -- the same bits on every rank.
// The parity of the exchange number selects the half: a rank can be at most one exchange ahead of a peer (its next push needs
// the peer's flag of the one in between).  Bandwidth: 16 n (g-1) bytes written over xGMI per rank and apply.
struct LaunchCtx;
struct VecBox {
    double* const* buf;        // device table [nranks]: rank r's buffer (own entry: the local allocation)
    uint32_t* const* flags;    // device table [nranks]: rank r's flag array
    uint32_t* counter;         // local: workgroups of the push kernel that have finished
    int32_t nranks, rank;
    int64_t n2;                // doubles per contribution (2 n)
    int64_t timeout_ticks;
};
void launch_vec_exchange(const LaunchCtx& c, const VecBox& vb, uint32_t seq, const double* slots, double* slots_rd);
// row-sharded + dual tiles: the local slot lists of the rows of A' -> one partial sum per row (kernels.hip)
void launch_slots_compact(const LaunchCtx& c, int nrows, const DefRow* rec, const int32_t* idx, int lpr, const double* slots, double* out);

// ---------------------------------------------------------------------------------- kernel launchers (kernels.hip / psd.hip)
struct LaunchCtx {
    hipStream_t stream;
    DevBlkCsr S;
    const double* cb;      // [n+m] = [c; b]
    int64_t n, m, l;       // l = n+m+1
    DevState* st;
    double* partials;      // scratch for per-workgroup partial sums
    double* reduced;       // small buffer of locally reduced sums (all-reduced in place when sharded)
    int32_t vec_blocks;    // grid of the vector kernels
    int32_t cg_blocks;     // grid of the two fused CG kernels (every workgroup re-reduces the partials: fewer, fatter groups)
    const PeerBox* peer;   // non-null: launch_reduce1 also exchanges the sums with the peer ranks (no RCCL call follows)
    const uint32_t* def_mask;   // bit i set: row i of S is finished from partial slots (nullptr: no dual tiles)
    // row-sharded operators (rank g owns rows of A, the column space is replicated): the slots the sweep filled are
    // summed over the ranks between the sweep and whatever adds the slot lists (`between`, called by the launchers); sums over
    // replicated entries (indices < n_repl) are counted by ONE rank only (count_repl).
    int (*between)(void*);
    void* between_arg;
    double* pre = nullptr;           // 3 x 16 doubles + 16 flags: the producer workgroups' sums of the sweep records (cg_update_kernel)
    const int32_t* gate = nullptr;   // non-null: the relaxation / cone kernels run only if *gate != 0 (DevState.done: enqueued behind a CG batch)
    // batched PSD projection: the launch environment (the cones' own state and switches: ConeSet below)
    int32_t cus = 0;                 // compute units of the handle's device
    int32_t psd_refine_max_mats = 0; // > 0: peer ranks share THIS device (tests): the refinement kernel only for batches this small (psd.hip)
    int32_t count_repl;         // 1: this rank counts the replicated entries in scalar sums (always 1 when not row-sharded)
    int64_t n_repl;             // replicated leading entries of every vector (0 when not row-sharded)
};

// KKT apply, 2 RHS interleaved:  out = [I Q'; Q -I] * w   (rows 0..n+m-1; the tau row is written by kkt_finalize).
// Stand-alone form: sweep (+ deferred-row kernel for operators with dual tiles); partial sums: c.S.npart records at c.S.part_off
void launch_kkt2(const LaunchCtx& c, const double2* w, double2* out, int gate, bool finish_deferred = true);
// finishes the tau rows of out = M w from the sweep's partial sums (CG init / test entry)
void launch_kkt_finalize(const LaunchCtx& c, const double2* w, double2* out, int gate, int from_reduced);

// One CG iteration = TWO dependent launches (conjugategradients.jl:37-51):
//   launch_kkt2_cg   iteration j >= 2 with fuse_p: closes iteration j-1 (r.r, stop test, beta), then sweeps with
//                    p_j = r + beta p_{j-1} formed on the fly and stored through the rows' owners; partial sums of Ap.p and
//                    of the tau rows, including the share of rows spread over dual-tile slots (c.S.nwg records at record 0);
//   launch_cg_update alpha, tau rows, the slot-spread rows of Ap, x += alpha p, r -= alpha Ap, r.r partials.
// Without fuse_p (gather-bound sparse operators: forming p on the fly would double the gathers) the p update stays a third
// launch (launch_cg_pupdate).  p_j lives in buffer j & 1.
struct CgIter {
    int j;                     // iteration number, from 1
    const double2* r;
    const double2* p_prev;     // p_{j-1}
    double2* p_cur;            // p_j
    bool fuse_p;
    int rr_from_reduced;       // r.r of iteration j-1 was all-reduced into c.reduced (sharded, RCCL)
    const PeerBox* fold;       // non-null: the two exchanges of the iteration happen inside the two kernels (peer mailboxes)
    uint32_t seq_base;
    int32_t batch_mark = 0;    // != 0: this is the last iteration the host enqueued; if CG goes on after it, the p update tells the host (HostMark.batch)
    bool start_fused = false;  // the solve was started by launch_cgm_apply / launch_cgm_start: the sweep of iteration 1 adds g_0 = r_0.r_0
};
void launch_kkt2_cg(const LaunchCtx& c, const CgIter& it, double2* Ap);
void launch_cg_stop_check(const LaunchCtx& c, const CgIter& it);      // closes iteration it.j - 1 when no sweep follows in this batch
void launch_cg_update(const LaunchCtx& c, const CgIter& it, double2* x, double2* r, double2* Ap, int kkt_from_reduced);
void launch_cg_pupdate(const LaunchCtx& c, const CgIter& it, double2* x, double2* p_next);   // !fuse_p: x += alpha p_j, closes iteration j, p_{j+1} = r + beta p_j

// Merged-reduction CG (Chronopoulos & Gear 1989; SURVEY 7 "hard parts"): the same Krylov iterates as conjugategradients.jl:31-55
// in exact arithmetic, rearranged so that ONE reduction point per iteration carries both inner products -- one exchange per
// iteration when sharded, and two launches instead of three:
//     w_0 = M r_0 ;  iteration j (i = j-1):   beta_i = g_i / g_{i-1} (0 for i = 0),  alpha_i = g_i / (d_i - beta_i g_i / alpha_{i-1})
//     UPDATE  p = r + beta p ; s = w + beta s (= M p) ; x += alpha p ; r -= alpha s ; partial sums of g_{i+1} = r.r
//     SWEEP   w = M r ; partial sums of d_{i+1} = w.r and of the tau row
// with g = r.r, d = w.r.  The stop test of iteration j (norm(r) <= tol || j >= max_iters, conjugategradients.jl:42) needs g_j:
//   close_in_update = false  the sweep behind the update adds the r.r records in its prologue and returns when CG has stopped
//                            (single GPU: no sweep is wasted; costs every sweep workgroup a short prologue);
//   close_in_update = true   the NEXT update adds them together with the sweep's sums -- one exchange of four doubles per iteration
//                            (sharded handles); the sweep of the last iteration has then run for nothing, and a batch of
//                            enqueued iterations ends with a one-workgroup launch of the update kernel that only closes.
// p lives in PB[0], s in PB[1], w in AP.
struct CgmIter {
    int j;                     // iteration number, from 1
    double2 *x, *r, *p, *s, *w;
    bool close_in_update;
    int from_reduced;          // the four sums were all-reduced into c.reduced (RCCL / host collective)
    const PeerBox* fold;       // non-null: the exchange happens inside the update kernel (peer mailboxes)
    uint32_t seq_base;
    int32_t batch_mark = 0;    // != 0: the launch that ends the host's batch tells the host when CG goes on after it (HostMark.batch)
};
constexpr int CGM_RR_STRIDE = 1024;   // r.r records ping-pong: the update of iteration j writes [j & 1][...]
void launch_cgm_sweep(const LaunchCtx& c, const CgmIter& it, int closes);        // w = M r (gated); closes >= 0: first closes that iteration (0: the start, g_0 only)
void launch_cgm_update(const LaunchCtx& c, const CgmIter& it, bool close_only);
// the start of a solve: the sweep it.w = M v (all rows but the tau row, slot-spread rows unfinished; launch_cgm_apply) and
// r = rhs - M v with the r.r records of "iteration 0"; its first workgroup also opens the solve in DevState (done = 0, tol, ...)
void launch_cgm_apply(const LaunchCtx& c, const CgmIter& it, const double2* v);
void launch_cgm_start(const LaunchCtx& c, const CgmIter& it, const double2* rhs, const double2* v, double tol, int maxit,
                      double2* p_out = nullptr);     // p_out: also p_1 = r_0 (the reference recurrence started this way)

// RESIDENT CG (round 6; resident.hip): the merged-reduction recurrence above as ONE launch per solve, for operators that are
// nothing but dual tiles of a block-separable A (a block-diagonal SDP: C4 and its shards) and small enough per workgroup to be
// HELD IN REGISTERS.  A UNIT = the tiles over one run of <= 64 columns of A (one diagonal block); its tiles are dealt to `wpu`
// consecutive workgroups, one tile per (wavefront, slot): lane = row keeps its row's values, its vector elements x, r, p, s, w
// and [c;b] in registers for the whole solve, the unit's <= 64 column elements are replicated in every workgroup of the unit.
// Per iteration nothing crosses workgroups but (i) the four sums {r.r, w.r, [c;b].r1, [c;b].r2} -- every workgroup publishes its
// record as self-validating words (the mailboxes' trick) and adds all G records in workgroup order: the same bits everywhere, no
// grid barrier, no L2 write-back or invalidate -- and (ii) the unit's column sums between its `wpu` workgroups, the same way.
// Across GPUs the four sums go on through the handle's mailboxes (peer_fold_sum), exactly as in cgm_update_kernel.
struct ResWG { int32_t blk0, nblk, c0, tc, T, wg0, wpu, idx; };     // 32 bytes: tiles blk0 .. blk0 + nblk - 1 of S.blk, the unit's columns [c0, c0 + tc), T steps;
                                                                    // the unit's workgroups wg0 .. wg0 + wpu - 1, this one is number idx
                                                                    // (a STREAMED workgroup: T is its tiles' deal to the wavefronts, rs_deal below)
constexpr int RES_GMAX = 512;        // workgroups of a resident solve (records every workgroup adds)
constexpr int RES_WPU_MAX = 16;      // workgroups per unit
constexpr int RES_SLOTS = 21;        // tiles per workgroup
// the STREAMED form's shape (resident.hip, cg_stream_kernel): workgroups (= records), workgroups a unit may be split over, compute wavefronts (+ 1 that
// communicates), the tiles the communication wavefront walks itself
constexpr int RS_GMAX = 256;
constexpr int RS_WPU_MAX = 4;
constexpr int RS_NCOMP = 7;
constexpr int RS_NTC = 6;
// THE DEAL of a streamed workgroup's tiles to its wavefronts: a table of eight tile counts carried in the plan (ResWG::T of a streamed workgroup:
// wavefront w's count in bits 4 w .. 4 w + 3), not a formula in the kernel.  Wavefront w walks the cnt[w] tiles behind those of the wavefronts in front
// of it -- slot order = tile order, the communication wavefront (w = RS_NCOMP) last -- so the rows' p and s sit in LDS by tile number.
// The table: the communication wavefront takes min(nblk % 7, RS_NTC_BASE) tiles, as it always did, and up to RS_NTC where that still leaves it
// RS_COMM_LEAD tiles lighter than the heaviest compute wavefront (it publishes and polls behind its sweep; 8 tiles or fewer: never); the other tiles go to
// the compute wavefronts evenly, the LATER wavefronts one tile fewer: they end their sweeps last (the stamps), and every CU's sweep ends on its last
// wavefront.  C4's 66 tiles: 9 9 9 9 8 8 8 + 6, where 9 x 7 + 3 left three of eight wavefronts streaming for the last 2 us of every sweep.
constexpr int RS_NTC_BASE = 3;
constexpr int RS_COMM_LEAD = 2;
// (tiles of more than 32 steps are walked in two passes each: their kernels keep the communication wavefront's three)
inline int rs_ntc(int tmax) { return tmax > 32 ? RS_NTC_BASE : RS_NTC; }
// which tiles of its workgroup wavefront w walks (w < RS_NCOMP: compute; w == RS_NCOMP: the communication wavefront, the LAST tiles)
__host__ __device__ inline void rs_split(uint32_t deal, int w, int& t0, int& cnt) {
    t0 = 0;
    for (int k = 0; k < w; ++k) t0 += (int)((deal >> (4 * k)) & 15u);
    cnt = (int)((deal >> (4 * w)) & 15u);
}
inline uint32_t rs_pack(const int (&cnt)[RS_NCOMP + 1]) {
    uint32_t deal = 0;
    for (int w = 0; w <= RS_NCOMP; ++w) deal |= (uint32_t)cnt[w] << (4 * w);       // (at most 10 tiles per wavefront: four bits)
    return deal;
}
inline uint32_t rs_deal(int nblk, int ntc = RS_NTC) {
    int kc = std::min(nblk % RS_NCOMP, RS_NTC_BASE);
    for (int k = std::min(ntc, RS_NTC); k > kc; --k)
        if (k <= (nblk - k + RS_NCOMP - 1) / RS_NCOMP - RS_COMM_LEAD) { kc = k; break; }
    const int per = (nblk - kc) / RS_NCOMP, rem = (nblk - kc) % RS_NCOMP;
    int cnt[RS_NCOMP + 1];
    for (int w = 0; w < RS_NCOMP; ++w) cnt[w] = per + (w < rem ? 1 : 0);
    cnt[RS_NCOMP] = kc;
    return rs_pack(cnt);
}
// what the kernels ask of ANY table for a workgroup of nblk tiles (the planner checks a forced one, FOS_RS_DEAL, against it): every tile dealt once, at
// most nt_cap per compute wavefront and ntc for the communication wavefront, and no compute wavefront with tiles behind one without (slots = tiles)
inline bool rs_deal_ok(uint32_t deal, int nblk, int nt_cap, int ntc) {
    int sum = 0;
    bool gap = false;
    for (int w = 0, t0, cnt; w <= RS_NCOMP; ++w) {
        rs_split(deal, w, t0, cnt);
        if (cnt > (w < RS_NCOMP ? nt_cap : ntc)) return false;
        if (w < RS_NCOMP && cnt > 0 && gap) return false;
        if (cnt == 0) gap = true;
        sum += cnt;
    }
    return sum == nblk;
}
// the heaviest compute wavefront of a table: what the kernel instance's NT must hold
inline int rs_deal_nt(uint32_t deal) {
    int nt = 0;
    for (int w = 0, t0, cnt; w < RS_NCOMP; ++w) { rs_split(deal, w, t0, cnt); nt = std::max(nt, cnt); }
    return nt;
}
// LDS of a launch (one function for the planner and the launch): the dynamic bytes of cg_stream_kernel for a workgroup of `tiles` tiles -- the wavefronts'
// column sums, the G records, the other workgroups' column sums, the rows' p and s -- and of cg_resident_kernel<TMAX = tmax, NSLOT = nslot>; the planner adds
// RS_STATIC_LDS_MAX for the kernel's static arrays (2176 bytes) and refuses a plan beyond the 160 KiB of a gfx950 CU, resident_setup checks the launch
// against the device's limit and the kernel's own static size
constexpr size_t RES_LDS_BUDGET = 160 * 1024;
constexpr size_t RS_STATIC_LDS_MAX = 2560;
inline size_t res_stream_lds_bytes(int tiles) {
    return (size_t)(RS_NCOMP + 1) * 64 * sizeof(double2) + (size_t)4 * RS_GMAX * sizeof(double) + (size_t)(RS_WPU_MAX - 1) * 64 * 2 * sizeof(double) +
           (size_t)tiles * 128 * sizeof(double2);
}
inline size_t res_reg_lds_bytes(int nslot, int tmax) {
    return (size_t)nslot * 64 * 4 * sizeof(double2) + (size_t)nslot * tmax * sizeof(double2) + (size_t)(RES_WPU_MAX - 1) * tmax * 2 * sizeof(double) +
           (size_t)4 * RES_GMAX * sizeof(double);
}
struct ResPlan {                     // host
    int G = 0, nw = 0, ncomm = 0, rpt = 0, tmax = 0, tiles_wg_max = 0, units = 0;      // nw compute wavefronts + ncomm communication wavefronts per workgroup
    int stream = 0, nt = 0;          // stream: the STREAMED form (tiles re-read every iteration, whole units per workgroup); nt: tiles per compute wavefront
    std::vector<ResWG> wg;
    std::string why;                 // why the operator does not qualify (G == 0)
};
// the plan for at most `gmax` workgroups; false (and why) when the operator does not qualify
bool build_resident_plan(const HostBlkCsr& S, int64_t m, int64_t n, int gmax, ResPlan* out);
// host emulation of the resident solve over the same plan (CPU tests of the plan and of the arithmetic; csr_build.cpp)
int host_resident_cg(const HostBlkCsr& S, const ResPlan& P, int64_t m, int64_t n, const double* cb, double2* x, const double2* rhs, const double2* v0,
                     double tol, int maxit, int* iters);
struct ResLaunch {
    const ResWG* wg; int G, nw, ncomm, rpt, tmax, stream, nt, tiles_wg_max;
    unsigned long long* grec;        // [2][G][4][2] words: the workgroups' records of the four sums
    unsigned long long* crec;        // [2][G][tmax][2][2] words: the workgroups' column sums (units of more than one workgroup)
    int64_t timeout_ticks;
    // the fp32 walk of the streamed form (resident.hip, rs_lowp_decide; all zero: none): the tile values as float at val's offsets, delta >= |A - fl32(A)|_2,
    // eta = the share of a solve's stop tolerance the walk may cost, mode 1: by the rule, 2: every sweep behind the start (tests), and the device
    // record of the last solve {fp32 sweeps, reverted, bound}
    const float* val32; double lowp_delta, lowp_eta; int lowp_mode; double* lowp_out;
    int lowp_cached;                 // the sweeps read val32 with default-policy loads, not non-temporal ones (rs_lowp_cached below; resident.hip, rs_request)
};
// WHERE THE FLOAT COPY IS READ FROM.  A solve's fp32 sweeps read the same val32 bytes one sweep after the other, with nothing else of size in between; read
// with loads that pass the CU's L1 by and take the default policy behind it, the sweeps are 2 us shorter.  Why is not established (the Infinity Cache serves
// non-temporal loads too: DESIGN_LOG.md), so the budget is not a cache's size but the largest copy this was MEASURED to pay for, and little more: copies of 69,
// 104 and 138.4 MB in the solve (profiles/stream_lowp_cache_sizes.txt, stream_lowp_cache_ab.json) and the bare walk at 138 MB; at 200 MB the bare walk reads no
// faster than with non-temporal loads (profiles/stream_reread_ceiling.json: the file this budget was read from) and nothing between was measured.  138 MiB
// (144.7 MB) is the largest copy a plan of 32-step tiles can have (69 tiles of 8 KB in each of 256 workgroups) and 4.5 % above the flagship's 132 MiB: that
// margin is a guess.  A larger copy (plans of 64-step tiles alone) keeps the non-temporal loads.
constexpr int64_t RS_LOWP_CACHE_BUDGET_BYTES = (int64_t)138 << 20;
// the budget in force: FOS_RS_LOWP_CACHE_MB (MiB, tests) or the constant
inline int64_t rs_lowp_cache_budget(int64_t mb_override) {
    return mb_override < 0 ? RS_LOWP_CACHE_BUDGET_BYTES : std::min<int64_t>(mb_override, (int64_t)1 << 20) << 20;
}
// the rule (pure; fos_host_lowp_cached): a plan with a float copy of val32_bytes reads it with the cached policy unless FOS_RS_LOWP_CACHE=0 says no
inline bool rs_lowp_cached(int64_t val32_bytes, bool cache_on, int64_t budget_bytes) { return cache_on && val32_bytes > 0 && val32_bytes <= budget_bytes; }
// rounds `nvals` tile values to val32 and leaves, per workgroup of the streamed plan, its bound of |A - fl32(A)|_2 in part[G] (the maximum is delta)
hipError_t launch_rs_lowp_setup(hipStream_t stream, const BlkDesc* blk, const double* val, int64_t nvals, const ResWG* wg, int G, float* val32, double* part);
// x (in: the start iterate, out: the solution), r_0 = rhs - M v; fold != nullptr: the sums cross the ranks through the mailboxes
// (hipSuccess, or the error of the LDS opt-in: a plan that does not fit is refused by resident_setup before it gets here)
hipError_t launch_cg_resident(const LaunchCtx& c, const ResLaunch& rl, double2* x, const double2* rhs, const double2* v, double tol, int maxit,
                              const PeerBox* fold, uint32_t seq_base);
// does the kernel instance `rl` launches fit the device's LDS (its dynamic bytes + its static arrays, and the opt-in)?  false: why
bool res_lds_fits(const ResLaunch& rl, int device, std::string* why);

// single right-hand side Q apply on component `comp` of an interleaved vector
//   Q_PLAIN : out_plain[i] = sign * (Q v)_i            (rows 0..n+m-1; tau row by q1_finalize)
//   Q_RHS   : out[i] = (x[i].x - (Q x.y)_i, 0)         (affinepluslinear.jl:94-95 with beta=1, q=0, b=0)
//   Q_STATUS: residual sums of checkstatus             (HSDEStatus.jl:34-38,59,61)
//   Q_PLAIN_NOTAU : Q_PLAIN with the tau entry of v taken as zero: out_plain = sign * [A'v_y; -A v_x], no c tau / b tau term (no finalize)
enum QMode { Q_PLAIN = 0, Q_RHS = 1, Q_STATUS = 2, Q_VFROMU = 3, Q_PLAIN_NOTAU = 4 };
void launch_q1(const LaunchCtx& c, QMode mode, const double2* v, int comp, double sign, void* out);
void launch_q1_finalize(const LaunchCtx& c, QMode mode, const double2* v, int comp, double sign, void* out, int from_reduced);

// CG vector kernels
void launch_cg_init(const LaunchCtx& c, const double2* rhs, const double2* Ap, double2* r, double2* p);
void launch_cg_init_finalize(const LaunchCtx& c, const double2* r, double tol, int maxit, int from_reduced);
void launch_reduce1(const LaunchCtx& c, int count, int nacc, int gate, int off = 0);
void launch_peer_chain(const LaunchCtx& c, int rounds);     // `rounds` mailbox exchanges of four doubles inside one launch (fos_exchange_bench)   // partials[off.. +count][nacc] -> reduced[nacc] (+ peer exchange)

// outer-loop vector kernels (gap.jl:48,58,78; gapa.jl:67,77,96-103; fista.jl:31-46; dykstra.jl)
constexpr int LONG_KMAX_ROWS = 32;   // saved planes of a LongstepWrapper: 2 (nsave + 1) <= 32
// LongstepWrapper state of a handle (wrappers/longstep.jl:12-22 LongstepWrapperData + saveplanes.jl:5-11 SavedPlanes), device resident
struct LongPlanes {
    int64_t interval = 0, nsave = 0;
    int64_t savepos = 0;               // LongstepWrapperData.savepos (0 at the start, -1 after a projection)
    bool now = false;                  // the iteration in flight saves planes
    double2* P = nullptr;              // [2 (nsave + 1)][l] saved rows x - y, in the reference's row order (equality, inequality, equality, ...)
    double* bpart = nullptr;           // [rows][vec_blocks] partial sums of the offsets (x - y).y
    double* dots = nullptr;            // [vec_blocks][33][hi, lo] scratch of the Gram products (double-double)
    double* nu = nullptr;              // [rows][hi, lo] multipliers, device copy
    double log[8] = {0};               // last projection: iteration, active inequalities, KKT violation, |x_new - x|, rows, supports tried, [6] given up (0 / 1),
                                       // [7] projections given up since fos_set_longstep
    int64_t max_supports = 4096;       // candidate supports a projection may try (FOS_LONG_MAX_SUPPORTS, read at long_setup)
};
struct LaunchCtx;
void long_save_plane(const LaunchCtx& c, LongPlanes& lp, int which, const double2* y, const double2* x);      // addprojeq (0) / addprojineq (1) at lp.savepos
int long_project_planes(const LaunchCtx& c, LongPlanes& lp, double2* X, int64_t i);                          // projectonnormals! + x .= tmp   (wrappers.cpp)
void launch_long_plane(const LaunchCtx& c, double2* row, const double2* x, const double2* y, double* bpart);          // row = x - y; bpart[blocks]: partial sums of (x - y).y
void launch_long_dots(const LaunchCtx& c, const double2* P, int K, int a, const double2* x, double* out);              // out[blocks][33][hi, lo]: row_a . row_{a+k}, k < 32; [32]: row_a . x (double-double)
void launch_long_apply(const LaunchCtx& c, double2* x, const double2* P, int K, const double* nu);                     // x += sum_k nu[k] row_k
void launch_normdiff(const LaunchCtx& c, const double2* x, const double2* y);   // c.partials[0 .. vec_blocks) = partial sums of |x - y|^2
void launch_shift_part2(const LaunchCtx& c, double2* out, const double2* y, const double2* x);   // out = (y.x, y.y - x.y)
void launch_axpby(const LaunchCtx& c, double2* out, double a, const double2* x, double b, const double2* y);          // out = a x + b y
void launch_relax_a12(const LaunchCtx& c, double2* out, const double2* y, const double2* x);                          // out = a12 y + (1-a12) x, a12 from state
// shift_out != nullptr: also shift_out = sol - [0; x2_new] (launch_shift_part2 for the next affine projection, saved a launch)
void launch_gap_final(const LaunchCtx& c, double2* x, const double2* t2, const double2* t1, double alpha, double alpha2,
                      double2* shift_out = nullptr, const double2* sol = nullptr);   // x = alpha(alpha2 t2+(1-alpha2)t1) + (1-alpha) x
void launch_gapa_final(const LaunchCtx& c, double2* x, const double2* t2, const double2* t1, double alpha,
                       double2* shift_out = nullptr, const double2* sol = nullptr);  // + normedScalar partials
void launch_gapa_finalize(const LaunchCtx& c, double beta, int from_reduced);
void launch_fista_extrap(const LaunchCtx& c, double2* y, const double2* x, const double2* xold, double coef);         // y = x + coef (x - xold)
void launch_add(const LaunchCtx& c, double2* out, const double2* a, const double2* b);                                // out = a + b
void launch_copy(const LaunchCtx& c, double2* out, const double2* in);                                                 // out = in (gateable)
void launch_dykstra_corr(const LaunchCtx& c, double2* p, const double2* x, const double2* y);                         // p = x + p - y

// direct = true (HSDE.jl:12-15): dense set-up helpers and the per-projection kernels
void launch_dense_q_fill(const LaunchCtx& c, const int64_t* colptr, const int64_t* rowval, const double* nzval, double* Q, int64_t ld);
void launch_dense_gemm(const LaunchCtx& c, int L, double alpha, const double* A, const double* B, double gamma, const double* D, double* Cm);
void launch_dense_resid(const LaunchCtx& c, int64_t L, const double* Y, double* partials, int nblocks);
void launch_dense_scale_identity(const LaunchCtx& c, int64_t L, double* X, double s);
void launch_dense_symv(const LaunchCtx& c, int64_t ld, const double* G, const double* t, double* w);
// the inverse of a dense symmetric positive definite matrix through a blocked Cholesky factorisation (dense_chol.hip); the same blocking on the host (tests)
void launch_dense_spd_inverse_chol(const LaunchCtx& c, int64_t L, const double* G, double* X, double* Lw, double* Ww, int32_t* info);
int64_t host_chol_inverse(int64_t k, const double* K, double* X, bool fused = false);      // fused: one rounding per multiply-add, as the device rounds
// G = A A' + (identity on the padding m .. L-1) for a ROW-major m x ld matrix A (ld % 64 == 0): L x L column-major, exactly symmetric, fixed summation order (dense_chol.hip)
void launch_dense_gram_rows(const LaunchCtx& c, int64_t m, int64_t ld, const double* A, int64_t L, double* G);
void launch_direct_rhs(const LaunchCtx& c, const double2* W, const double2* x, double* t);
void launch_direct_finish(const LaunchCtx& c, const double2* x, const double2* W, double2* out);

// direct = true, reduced form (direct_reduced.hip): K^-1, K = I + A'A or I + A A' of order k = min(m, n), as tiles of its lower triangle stored once
constexpr int RED_TR = 64, RED_TC = 32;          // rows (= lanes) and columns of a tile
constexpr int RED_TILE = RED_TR * RED_TC;        // doubles per tile
constexpr int RED_CHUNK = 16;                    // row blocks per unit (the walk of one wavefront)
constexpr int RED_DOT_BLOCKS = 1024;             // most workgroups (= records of the two border dots) of the vector kernels
struct RedUnit { int32_t j, i0, i1, tile0; };    // strip j (columns [32 j, 32 j + 32)), row blocks [i0, i1), first tile in the stream
struct RedPlan {                                 // host
    int64_t k = 0, ntiles = 0;
    int nt = 0, ns = 0;                          // row blocks, strips
    std::vector<RedUnit> units;
    std::vector<int32_t> strip_u0;               // [ns + 1] units of strip j: strip_u0[j] .. strip_u0[j + 1] - 1
};
struct RedDev {                                  // device
    int64_t k, kpad; int nt, nunits;
    const RedUnit* units; const int32_t* strip_u0;
    double* tiles;                               // [ntiles][RED_TILE]
    double2* rowslot;                            // [ntiles][64]: T x_J of every tile
    double* colslot;                             // [nunits][64]: T' x_I summed over a unit, (column, right-hand side) interleaved
};
void build_reduced_plan(int64_t k, RedPlan* P);
void host_reduced_pack(const RedPlan& P, const double* X, std::vector<double>* tiles, int32_t* count);
void host_reduced_symm(const RedPlan& P, const std::vector<double>& tiles, const double* pq, double* y);
void launch_red_form_k(const LaunchCtx& c, int64_t k, int64_t ld, const int32_t* cptr, const int32_t* cidx, const double* cval, const int32_t* rptr,
                       const int32_t* ridx, const double* rval, double* K);
void launch_red_pack_tiles(const LaunchCtx& c, const RedDev& R, int64_t ld, const double* X);
void launch_red_symm(const LaunchCtx& c, const RedDev& R, const double2* pq, double2* y);          // y = K^-1 (p, q), pairs interleaved, kpad of them
void launch_red_in1(const LaunchCtx& c, int swap, const double* t, double2* vin);
void launch_red_pair(const LaunchCtx& c, const RedDev& R, int swap, const double* t, const double* s1, double2* pq);
void launch_red_in2(const LaunchCtx& c, int swap, const double2* yk, double2* vin);
int  launch_red_d(const LaunchCtx& c, int swap, const double* t, const double* s2, const double2* yk, const double* hv, const double* gv, double* d, double* dots);
void launch_red_w(const LaunchCtx& c, const double* t, const double* d, const double* pv, const double* qv, const double* dots, int nrec, const double* minv,
                  int add, double* w);
void launch_red_resid(const LaunchCtx& c, const double* t, const double* w, const double* z, double* r);

// direct = true on a block-separable operator (I + A'A block diagonal with blocks of order <= BLKDIR_MAX): vecops.hip, direct.cpp prox_affine_direct_block
constexpr int BLKDIR_MAX = 64;
void launch_blkdir_prep(const LaunchCtx& c, const double2* T, const double2* phg, double2* W2, double2* W3, double* partials);
void launch_blkdir_solve(const LaunchCtx& c, int nblk, const int64_t* goff, const int32_t* ioff, const int32_t* idx, const double* Ginv, const double2* R,
                         const double2* T, double2* W3, double* ctx_rec);
void launch_blkdir_combine(const LaunchCtx& c, const double2* T, const double2* W3, const double2* V, const double2* phg, const double2* qphg,
                           double* prm, int zero_kappa, double2* out, const double* prep_partials, double* partials, int from_reduced);
void launch_blkdir_tausum(const LaunchCtx& c, const double* partials, const double* ctx_rec, int nblk, double* out1);
void launch_blkdir_tau(const LaunchCtx& c, const double2* T, const double2* qphg, const double* prm, int zero_kappa, double2* out, const double* prep_partials,
                       const double* partials, const double* ctx_rec, int nblk, int from_reduced);

// layout conversion at the ABI boundary
void launch_interleave(const LaunchCtx& c, double2* out, const double* plain);    // plain [part1(l); part2(l)] -> interleaved
void launch_deinterleave(const LaunchCtx& c, double* plain, const double2* in);
void launch_set_comp(const LaunchCtx& c, double2* out, const double* plain_l, int comp);   // out[i].comp = plain[i], other comp = 0
void launch_get_plain(const LaunchCtx& c, double* plain_l, const double2* in, int comp);

// opt-in equilibration (fos_create3): the scaling computed on the host (equilibrate.cpp) and the kernels of an equilibrated handle (equilibrate.hip)
constexpr double EQ_TARGET_NORM = 10.0;          // |b^| = |c^| = this (workloads.TARGET_NORM)
constexpr int EQ_MAX_PASSES = 50;
constexpr int EQ_THREADS = 256, EQ_MAX_BLOCKS = 512;     // the kernels' grid: a workgroup per 256 elements up to 512, grid-stride beyond (l > 131 072)
inline int eq_blocks(int64_t count) { return (int)std::max<int64_t>(1, std::min<int64_t>((count + EQ_THREADS - 1) / EQ_THREADS, EQ_MAX_BLOCKS)); }
struct EqScaling {                               // host
    int passes = 0;
    std::vector<double> D, E;                    // m row factors (gamma folded in), n column factors
    double sigma = 1.0, rho = 1.0, gamma = 1.0;
    std::vector<double> nz, b, c;                // A^ = D A E in the caller's CSC pattern, b^ = sigma D b, c^ = rho E c
};
// validates the problem as fos_create does (FOS_EINVAL / FOS_EUNSUPPORTED with a message) and fills `out`; passes in 1 .. EQ_MAX_PASSES
int host_equilibrate(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, const double* c,
                     int64_t nK1, const int32_t* K1type, const int64_t* K1start, const int64_t* K1len,
                     int64_t nK2, const int32_t* K2type, const int64_t* K2start, const int64_t* K2len, int passes, EqScaling* out);
void launch_eq_status(const LaunchCtx& c, const double2* z, const double* w, const double* cb, const double* inv, double* partials);
void launch_eq_interleave(const LaunchCtx& c, double2* out, const double* plain, const double2* up);
void launch_eq_deinterleave(const LaunchCtx& c, double* plain, const double2* in, const double2* up);

// cones (cones.jl:122-142)
void launch_cones_elementwise(const LaunchCtx& c, double2* out, const double2* in, const uint8_t* ew_op);
// t1 = a sol + (1 - a) x (a, or alpha12 of the device state) and t2 = P(t1) on the elementwise cones' indices, one pass (vecops.hip)
void launch_relax_ew(const LaunchCtx& c, double2* t1, double2* t2, const double2* sol, const double2* x, double a, bool use_a12, const uint8_t* ew_op);
void launch_cones_soc(const LaunchCtx& c, double2* out, const double2* in, const ConeDesc* cones, int ncones);
void launch_cones_exp(const LaunchCtx& c, double2* out, const double2* in, const ConeDesc* cones, int ncones);
// Fusion of the GAP / DR step around the batched PSD(64) projection (psd64_refine_kernel): the kernel's input is not read from a vector t1
// but FORMED, t1 = a1 sol + (1 - a1) x (the relaxation behind S1, gap.jl:48), and its output is not written to t2 but taken on to the step's
// last pass, x = alpha (alpha2 t2 + (1 - alpha2) t1) + (1 - alpha) x (gap.jl:58,78), with the vector the next CG start applies M to
// (sol - [0; x2]) -- for the entries of the PSD cones; the other entries (elementwise cones) are done by extra workgroups of the same launch.
struct PsdFuse {
    int on;
    const double2* sol; double2* xv; double2* shift;     // shift: nullptr when the next projection is not a CG solve inside fos_step
    double a1, alpha, alpha2;
    const uint8_t* ew_op; int64_t l; int nmat;           // elementwise entries: workgroups nmat.. of the grid
};
// PSD cones of order > 64: the projection by matrix products only, P = (M + M sign(M)) / 2 with sign(M) from an inverse-free polynomial iteration on the fp64
// matrix cores (psd_sign.hip).  psd_sign_setup takes those cones OUT of `psd` (what stays goes to the kernels of psd.hip) and allocates their workspace.
struct PsdSign;
int psd_sign_setup(std::vector<ConeDesc>& psd, PsdSign** out);
void psd_sign_destroy(PsdSign* p);
int psd_sign_count(const PsdSign* p);
int launch_cones_psd_sign(const LaunchCtx& c, PsdSign* p, double2* out, const double2* in);

// ---- a product of cones, projected (cones.cpp): the HSDE handle's DualConeProduct and the Feasibility form's ConeProduct are both one ConeSet.
// The host table: built once per product by the one validator and the one classifier of cone codes
struct ConeTable { std::vector<uint8_t> ew; std::vector<ConeDesc> soc, psd, expc; };      // ew: one op per stacked index (sized by the caller); the batched cones
enum ConeRole { CONE_K2, CONE_K1, CONE_PRIMAL };     // K2 on [x | r]: part 1 primal, part 2 dual; K1 on [y | s]: the other way round; a ConeProduct set: part 1 primal, part 2 copied
int psd_order(int64_t len);                          // k with k (k + 1) / 2 == len, or -1
// ranges 1-based, contiguous, ordered and covering 1..total (cones.jl:66-72); FOS_EINVAL / FOS_EUNSUPPORTED with a message naming `which`
int cone_table_check(const char* which, int64_t total, int64_t nK, const int32_t* type, const int64_t* start, const int64_t* len);
void cone_table_add(ConeTable& t, int64_t offset, ConeRole role, int64_t nK, const int32_t* type, const int64_t* start, const int64_t* len);
struct PsdTuning {                   // the FOS_PSD_* switches of a handle
    int wave = -1;                   // FOS_PSD_WAVE: -1 decide from the batch size, 0 / 1 force the workgroup / wavefront kernel at order 64
    int refine = -1;                 // FOS_PSD_REFINE: -1 by batch size, 0 / 1 never / always (order 64, warm)
    bool extrapolate = true;         // FOS_PSD_EXTRAPOLATE=0: the refinement starts from the previous basis only
    double theta = 0.0;              // FOS_PSD_THETA: rotation threshold of the refinement (0: the built-in value)
    bool narrow = false, wide = false;      // FOS_PSD_NARROW / FOS_PSD_WIDE
    int wide_threads = 512;          // FOS_PSD_THREADS
    static PsdTuning from_env();
};
struct ConeSetOptions {
    bool warm = true;                // keep the two warm-start bases (orders <= 64)
    bool refine_records = false;     // allocate the refinement kernel's records when every order is 64 (without them that kernel never runs)
    bool debug_rec = false;          // FOS_PSD_DEBUG_REC: the records' diagnostics switch
};
// The device state: the uploaded table, the PSD workspaces and warm-start bases, the switches.  It owns every buffer it names.
struct ConeSet {
    uint8_t* ew_op = nullptr;                  // [l] elementwise op per index (EW_SKIP inside SOC / Exp / PSD cones)
    ConeDesc *soc = nullptr, *expc = nullptr, *psd = nullptr;      // psd: orders <= 64 (psd.hip)
    int nsoc = 0, nexp = 0, npsd = 0, kmin = 0, kmax = 0;
    PsdSign* big = nullptr;                    // PSD cones of order > 64 (psd_sign.hip)
    double* scratch = nullptr;
    double* V[2] = {nullptr, nullptr};         // warm-start eigenvector bases (ping-pong): the last projection's is V[cur]
    int cur = 0, have_prev = 0;                // have_prev: projections behind the basis, capped at 2
    int32_t* redo = nullptr;                   // per (cone, copy): 1 = the refinement kernel left the matrix to the Jacobi kernel
    int* stats = nullptr;                      // Jacobi sweeps of the last projection, per (cone, copy)  (fos_psd_debug)
    int phase_limit = 0;                       // diagnostic: stop the PSD kernel after a phase (wrong results!)
    bool attr_set = false, attr_set_r = false; // the "LDS opt-in done" flags of psd_kernel / psd64_refine_kernel
    PsdTuning tune;
    int64_t fused_steps = 0;                   // projections taken through the fused launch (host count; fos_psd_fused_steps)
    std::vector<void*> owned;
    // the host-side state a projection advances: what a caller that enqueues projections speculatively takes back (affine_then)
    struct Mark { int cur, have_prev; int64_t fused_steps; };
    Mark mark() const { return {cur, have_prev, fused_steps}; }
    void rewind(const Mark& k) { cur = k.cur; have_prev = k.have_prev; fused_steps = k.fused_steps; }
    void start_cold() { cur = 0; have_prev = 0; }
};
int cone_set_build(const ConeTable& t, int64_t l, const ConeSetOptions& o, const PsdTuning& tune, ConeSet** out);      // on the current device
void cone_set_destroy(ConeSet* cs, hipStream_t stream);      // waits for `stream` (the projections in flight) before it frees; nullptr: nothing to do
// prox!(out, K, in) in two parts: elementwise (unless ew_done: the kernel that wrote `in` projected them), SOC and Exp cones; then the PSD cones, orders <= 64
// before orders > 64, and the warm-start advance.  fuse: the step's relaxation and last pass ride on the PSD launch (cone_set_can_fuse says when that is possible)
void cone_set_project_vector(ConeSet* cs, const LaunchCtx& c, double2* out, const double2* in, bool ew_done = false);
int cone_set_project_psd(ConeSet* cs, const LaunchCtx& c, double2* out, const double2* in, const PsdFuse* fuse = nullptr);
bool cone_set_can_fuse(const ConeSet& cs, const LaunchCtx& c);      // psd.hip: the next projection would take the refinement kernel
int launch_cones_psd(const LaunchCtx& c, ConeSet& cs, double2* out, const double2* in, const PsdFuse* fuse);
// ---- the sets of the Feasibility form (feas.hip).  A set is a device object with prox!(y, S, x); the handle owns one per slot and knows nothing else about it.
// A new kind is one file with a set-up function (build, hand back a ProxObject*) and a prox override, plus an ABI entry: validate, build, feas_install.
enum FeasKind : int {
    FEAS_AFFINE_DENSE = 1,           // IndAffine, the dense n x n projector (feas_objects.hip)
    FEAS_BOX = 2,                    // IndBox, scalar or array bounds (feas_objects.hip)
    FEAS_CONES = 3,                  // ConeProduct around a ConeSet (feas_objects.hip)
    FEAS_CALLBACK = 4,               // the caller's prox! on host vectors (feas_objects.hip)
    FEAS_AFFINE_SPARSE = 5,          // IndAffine over a sparse A, CG (affine_sparse.hip)
    FEAS_BLOCKS = 6,                 // separable sum of vector sets and functions (sets.hip)
    FEAS_AFFINE_FACTORED = 7,        // IndAffine / LeastSquares over a dense A, factored (affine_dense.hip)
    FEAS_SPARSE_FACTORED = 8,        // IndAffine / LeastSquares over a sparse A, factored (affine_sparse_factored.hip)
    FEAS_NSPACE = 9,                 // Quadratic / LeastSquares in the n-space (nspace.hip)
    FEAS_NSPACE_CG = 10,             // Quadratic / LeastSquares over a sparse Q / A of any size, CG in the n-space (nspace_cg.hip)
};
struct ProxObject {
    explicit ProxObject(int k) : kind(k) {}
    ProxObject(const ProxObject&) = delete;
    ProxObject& operator=(const ProxObject&) = delete;
    virtual ~ProxObject() = default;                                       // frees what the object owns; the caller has synchronised the stream its prox ran on
    virtual int prox(hipStream_t stream, double* y, const double* x) = 0;  // y, x: device vectors of length n (zero padded to a multiple of 64), y must not alias x
    virtual void reset(hipStream_t) {}                                     // a new solve (fos_feas_set_iterate): cold PSD bases, zero multipliers
    const int kind;                                                        // FeasKind: the ABI accessors check it before they downcast
};
// The device memory an object owns, with the three helpers every set-up needs.  `what` names the caller in the messages.
struct DevOwned {
    std::vector<void*> owned;
    size_t bytes = 0;
    const char* what = "";
    DevOwned() = default;
    DevOwned(const DevOwned&) = delete;
    DevOwned& operator=(const DevOwned&) = delete;
    ~DevOwned() { for (void* q : owned) (void)hipFree(q); }
    // FOS_OK, or FOS_ENOMEM / FOS_EHIP with "<what> set-up: <call> -> <error>"
    int hip(const char* call, hipError_t e) const {
        if (e != hipSuccess) { set_error("%s set-up: %s -> %s", what, call, hipGetErrorString(e)); return e == hipErrorOutOfMemory ? FOS_ENOMEM : FOS_EHIP; }
        return FOS_OK;
    }
    template <class T> int alloc(T** out, size_t count) {
        void* q = nullptr;
        const size_t nb = sizeof(T) * std::max<size_t>(count, 1);
        const hipError_t e = hipMalloc(&q, nb);
        if (e != hipSuccess) { (void)hipGetLastError(); set_error("%s: hipMalloc of %zu bytes failed: %s", what, nb, hipGetErrorString(e)); return FOS_ENOMEM; }
        owned.push_back(q); bytes += nb;
        *out = static_cast<T*>(q);
        return FOS_OK;
    }
    // stream == nullptr: the blocking calls (a set-up without a stream of its own)
    template <class T> int zeros(T** out, size_t count, hipStream_t s) {
        FOS_TRY(alloc(out, count));
        const size_t nb = sizeof(T) * std::max<size_t>(count, 1);
        return hip("hipMemset", s ? hipMemsetAsync(*out, 0, nb, s) : hipMemset(*out, 0, nb));
    }
    template <class T> int upload(T** out, const T* src, size_t count, hipStream_t s) {
        FOS_TRY(alloc(out, count));
        if (count == 0) return FOS_OK;
        return hip("hipMemcpy", s ? hipMemcpyAsync(*out, src, sizeof(T) * count, hipMemcpyHostToDevice, s) : hipMemcpy(*out, src, sizeof(T) * count, hipMemcpyHostToDevice));
    }
    template <class T> int upload(T** out, const std::vector<T>& v, hipStream_t s) { return upload(out, v.data(), v.size(), s); }
};
// The device twins of HostCsr and SfPass (sparse_rows.hpp): owned by `o`, uploaded on `s` (nullptr: blocking)
struct DevCsr {
    int32_t *rp = nullptr, *ci = nullptr;
    double* va = nullptr;
    int upload(DevOwned& o, const HostCsr& h, hipStream_t s) { FOS_TRY(o.upload(&rp, h.rp, s)); FOS_TRY(o.upload(&ci, h.ci, s)); return o.upload(&va, h.va, s); }
};
struct DevPass {
    SfItem* items = nullptr;
    int32_t *frow = nullptr, *fptr = nullptr;
    double* part = nullptr;                       // one slot per segment of a cut row (zeroed)
    int nitems = 0, nfold = 0;
    int64_t nparts = 0;
    int upload(DevOwned& o, const SfPass& P, hipStream_t s) {
        nitems = (int)P.items.size(); nfold = (int)P.frow.size(); nparts = P.nparts;
        FOS_TRY(o.upload(&items, P.items, s)); FOS_TRY(o.upload(&frow, P.frow, s)); FOS_TRY(o.upload(&fptr, P.fptr, s));
        return o.zeros(&part, (size_t)P.nparts, s);
    }
};
// inside a set-up that defines fail(code) (release the half-built object, hand the code back): a HIP call of owner `a`
#define DEV_HIP(a, expr) do { const int _r = (a)->hip(#expr, (expr)); if (_r != FOS_OK) return fail(_r); } while (0)

// the element-wise kernels of feas.hip and feas_objects.hip: FEAS_THREADS threads, a grid-stride loop
constexpr int FEAS_THREADS = 256;
#define FEAS_STRIDE(i, n) for (int64_t i = blockIdx.x * (int64_t)FEAS_THREADS + threadIdx.x; i < (n); i += (int64_t)gridDim.x * FEAS_THREADS)
// what a set-up in feas_objects.hip takes from the handle
struct FeasEnv { hipStream_t stream; int64_t n, L; int grid, cus; double* partials; };
// feas_objects.hip: the dense projector (A: m x n ROW-major), the box (lov == nullptr: the scalars), the ConeProduct, the host callback (which: 1 | 2, for its message)
int dense_projector_setup(const FeasEnv& env, int64_t m, const double* A, const double* b, ProxObject** out);
void dense_projector_stats(const ProxObject* p, int32_t* ns_iters, double* ns_resid);      // 0, 0 when p is no dense projector
int box_setup(const FeasEnv& env, double lo, double hi, const double* lov, const double* hiv, ProxObject** out);
int cone_product_setup(const FeasEnv& env, const ConeTable& table, ProxObject** out);
int callback_setup(const FeasEnv& env, int which, fos_prox_fn fn, void* ctx, ProxObject** out);

// The stats / plan functions below take the object the set-up of the same file built (the caller checked `kind`).
// IndAffine(A, b) with a sparse A (affine_sparse.hip): exact projection by warm-started CG on the row-scaled normal equations, the true residual re-checked
struct ScaledRows {                              // host: the rows of [A | b] scaled to unit norm -- A and A' in CSR, the scaled b, the row factors (1 for a zero row)
    HostCsr A, At;
    std::vector<double> bs, scale;
};
// both sparse IndAffine forms and the sparse factored LeastSquares.  ascending: csc_check's rule; zero_rows: a zero row is accepted, otherwise it is FOS_EINVAL
int sparse_affine_rows(const char* what, int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, bool ascending,
                       bool zero_rows, ScaledRows* out);
int sparse_affine_setup(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, int cus, ProxObject** out);
void sparse_affine_stats(const ProxObject* a, double* out8);
// IndAffine(A, b) with a dense A, factored form (affine_dense.hip): A kept once, (A A')^-1 of order m, two passes over A per projection
int dense_affine_setup(int64_t m, int64_t n, const double* A, const double* b, double lambda, int factor, int refine, int cus, hipStream_t stream, ProxObject** out);
void dense_affine_stats(const ProxObject* a, double* out8);
void dense_affine_plan(const ProxObject* a, int64_t* out6);
int host_affine_factored(int64_t m, int64_t n, const double* A, const double* b, double lambda, int refine, const double* x, double* y);
// the m-space product of the factored forms (da_symv_kernel): out = add + sign M v, M symmetric column-major of order l, leading dimension ld (add == nullptr: 0;
// out may be add); the same on the host in the kernel's order, the host's wave_sum tree, and the host's accepted inverse of G (order m, unpadded; `what` in the message)
void launch_da_symv(hipStream_t s, int64_t l, int64_t ld, const double* M, const double* v, const double* add, double sign, double* out);
void host_da_symv(int64_t l, int64_t ld, const double* M, const double* v, const double* add, double sign, double* out);
double host_da_wave(const double* lane64);
int host_da_inverse(const char* what, int64_t m, const double* G, double* X);
// the m-space step of a factored projection, d = X r corrected once: d = X r; e = r - G d; d += X e (X, G of order m, leading dimension L); its host twin (L = m)
void mspace_correct(hipStream_t s, int64_t m, int64_t L, const double* X, const double* G, const double* r, double* d, double* e);
void host_mspace_correct(int64_t m, const double* X, const double* G, const double* r, double* d, double* e);
// IndAffine(A, b) with a sparse A, factored form (affine_sparse_factored.hip): A and A' kept as CSR, (A A')^-1 of order m dense, two segmented sparse passes per projection
// lambda: 0: IndAffine(A, b), > 0: LeastSquares(A, b, lambda) (refine is then 0, zero and dependent rows are accepted)
int sparse_factored_setup(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int factor,
                          int refine, hipStream_t stream, ProxObject** out);
void launch_sf_gram(hipStream_t stream, int64_t m, int64_t L, const int32_t* rp, const int32_t* ci, const double* va, const int32_t* trp, const int32_t* tci,
                    const double* tva, double* G);
void sparse_factored_stats(const ProxObject* a, double* out8);
void sparse_factored_plan(const ProxObject* a, int64_t* out8);
int host_affine_sparse_factored(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int refine,
                                const double* x, double* y);
// Quadratic(Q, q) and LeastSquares in the normal-equations form (nspace.hip): y = M^-1 (x + c), M and its inverse kept as packed lower-triangle tile streams,
// three one-right-hand-side tile products per prox
int nspace_setup_quadratic(int64_t n, const double* Q, const double* q, int factor, hipStream_t stream, ProxObject** out);
int nspace_setup_ls_dense(int64_t m, int64_t n, const double* A, const double* b, double lambda, int factor, hipStream_t stream, ProxObject** out);
int nspace_setup_ls_sparse(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, int factor,
                           hipStream_t stream, ProxObject** out);
void nspace_stats(const ProxObject* a, double* out8);
int nspace_bench_symv(int64_t k, int reps, hipStream_t stream, double* out4);
void host_nspace_symv(const RedPlan& P, const std::vector<double>& tiles, const double* v, double* y);
int host_nspace_quadratic(int64_t n, const double* Q, const double* q, const double* x, double* y);
int host_nspace_ls_dense(int64_t m, int64_t n, const double* A, const double* b, double lambda, const double* x, double* y);
int host_nspace_ls_sparse(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, const double* x,
                          double* y);
int host_nspace_symv_packed(int64_t k, const double* X, const double* v, double* y, int32_t* count);
// Quadratic(Q, q) with a sparse Q and LeastSquares(A, b, lambda) with a sparse A of any size (nspace_cg.hip): y = M^-1 (x + c) by warm-started Jacobi-preconditioned CG,
// nothing dense.  Q, A: CSC, 1-based, row indices strictly ascending in a column; of Q only the entries i >= j are read.  tol: relative stop (0: the rounding level)
int nspace_cg_setup_quadratic(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol, hipStream_t stream,
                              ProxObject** out);
int nspace_cg_setup_ls(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, double tol,
                       hipStream_t stream, ProxObject** out);
void nspace_cg_stats(const ProxObject* a, double* out8);
int host_nspace_cg_quadratic(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* q, double tol, const double* x, double* y,
                             int32_t* iters);
int host_nspace_cg_ls(int64_t m, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double lambda, double tol,
                      const double* x, double* y, int32_t* iters);
// Separable sums of convex vector sets (sets.hip): norm balls, simplex, halfspace / hyperslab, point, free, scalar box -- contiguous blocks covering 1..n
int set_blocks_setup(int64_t n, int64_t nblocks, const int32_t* kind, const int64_t* len, const double* scal, const double* vec, ProxObject** out);
int set_blocks_stats(const ProxObject* p, hipStream_t stream, double* out8);
// Dense Quadratic / LeastSquares / IndAffine blocks of a separable sum (dense_blocks.hip): the optional dense part of SetBlocks.  The arrays are those of
// fos_feas_set_blocks2; block_mat == nullptr: the sum has no dense part (kinds 48..50 are then unknown kinds)
struct DenseBlockArgs {
    int64_t nmat = 0;
    const int64_t *mat_rows = nullptr, *mat_cols = nullptr;
    const double* const* mats = nullptr;
    const int64_t* block_mat = nullptr;
    const double* const* block_vec = nullptr;
};
struct DenseBlocks;
bool dense_block_kind(int kind);
int dense_blocks_setup(int64_t nblocks, const int32_t* kind, const int64_t* len, const int64_t* start, const double* scal, const DenseBlockArgs& a, DenseBlocks** out);
void dense_blocks_free(DenseBlocks* p);
int dense_blocks_launches(const DenseBlocks* p);
void dense_blocks_prox(const DenseBlocks* p, hipStream_t stream, double* y, const double* x);
void dense_blocks_stats(const DenseBlocks* p, double* out8);
int dense_blocks_get(const DenseBlocks* p, int64_t block, double* G, double* d);
int set_blocks_setup2(int64_t n, int64_t nblocks, const int32_t* kind, const int64_t* len, const double* scal, const double* vec, const DenseBlockArgs& dense,
                      ProxObject** out);
const DenseBlocks* set_blocks_dense(const ProxObject* p);      // nullptr: the sum holds no dense block
size_t psd_scratch_bytes(int kmax, int ncones);
size_t psd_basis_doubles(int kmax, int ncones);

void launch_status_finalize(const LaunchCtx& c, const double2* z, int from_reduced);

}  // namespace fos
