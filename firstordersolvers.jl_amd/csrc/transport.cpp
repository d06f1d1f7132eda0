// libfoship, the transports: how the sums of a sharded handle cross the ranks, and the fos_comm_* / fos_peer_* / fos_exchange_bench entries of include/foship.h.
// Their state is one member of the handle, fos_solver::tr (struct Transport, fos_solver.hpp); what is sharded (nranks, rank, row_sharded) is the handle's, the
// solves' sequence windows (cg_epoch) are the CG state's (fos_solver::cg, cg.cpp).  Nothing outside this file knows RCCL, HIP IPC or the shm segment.
//
//   transport (ReduceVia)   scalar sums (allreduce, <= 8 doubles in h->reduced)                  row-sharded n-vector (sum_slots_over_ranks, 2n doubles)
//   ----------------------  ---------------------------------------------------------------------  ---------------------------------------------------------
//   VIA_PEER   mailboxes    inside the reducing kernel (launch_reduce1) or folded into the CG      the peer-mapped exchange buffers (fos::VecBox), in stream;
//                           kernels: allreduce has nothing left to do.  Two kinds of mailboxes:    without them (never on an enabled row-sharded handle): as
//                           device memory mapped through HIP IPC, or ONE host-pinned shm segment   VIA_RCCL if there is a communicator, else the copy
//   VIA_HOST   callback     staged through the pinned host_buf and handed to the caller's          the same, 2n doubles
//                           collective (synchronises the stream: the slow, always possible path)
//   VIA_RCCL   communicator ncclAllReduce in stream                                                ncclAllReduce in stream
//   VIA_NONE   not sharded  nothing                                                                the sum is the copy
//
// Precedence (Transport::via): peer_on, then host_fn, then comm -- several may be set up on one handle, the first of them carries the sums;
// fos_peer_enable(h, 0) returns to whichever of the other two is there.
//
// Call sequences (every call collective: all ranks make it, with the same arguments but `rank`):
//   RCCL          fos_comm_get_unique_id (rank 0; the host broadcasts the id) -> fos_comm_init
//   callback      fos_comm_init_host
//   mailboxes     fos_peer_export -> (the host all-gathers the 64-byte handles) -> fos_peer_open      [device memory]
//                 or fos_peer_open_host                                                                [host-pinned segment; cone-sharded handles only]
//                 row-sharded: -> fos_peer_vec_export -> (all-gather) -> fos_peer_vec_open
//                 -> (the host's barrier) -> fos_peer_selftest -> (the host agrees on the outcome) -> fos_peer_enable(h, 1)
//   close         fos_peer_enable(h, 0) leaves the mailboxes open and unused; fos_peer_close drops them (either kind, the vector buffers with them) so that
//                 another kind can be opened on the same handle; fos_destroy ends everything.  Both end in transport_teardown.
//
// What a failed call leaves behind:
//   fos_comm_init, fos_comm_init_host   failing in their own checks: nothing.  Failing in the sharded set-up behind them (global_setup): the communicator /
//                                       the callback stays installed.
//   fos_peer_export, _vec_export        the own mailbox / buffer stays allocated (it is the pool's, handed on at fos_destroy).
//   fos_peer_open, _open_host,          nothing of its own open: no IPC mapping, no registered segment, no shm name (rank 0); the next open starts afresh.
//   fos_peer_vec_open                   (The small device tables an interrupted install allocated stay the handle's until fos_destroy.)
//   fos_peer_selftest                   *ok = 0 and FOS_OK after a mismatch, a time-out or a stale segment: the mailboxes stay open but off, the exchange's
//                                       failure mark is cleared, the handle keeps the reduction it had.
//   fos_peer_enable                     peer_on is as asked; a failure of the set-up behind it (a time-out of the first exchange: FOS_ECOMM) leaves it so --
//                                       the caller closes the mailboxes (fos_peer_close switches them off first).
//   fos_peer_close                      a failing fos_peer_enable(h, 0) inside it: everything still open.  Afterwards: closed, whatever else it reports.
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>

#include "fos_solver.hpp"

namespace fos {

// ------------------------------------------------------------------------------------------------ RCCL via dlopen
// (no link-time dependency: single-GPU users never load it; inside a torch process dlopen returns the copy torch
// already mapped, so both share one RCCL instance)
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static Rccl g_rccl;

static int rccl_load() {
    if (g_rccl.lib) return FOS_OK;
    // ONE copy of RCCL per process: a host that already carries one (PyTorch ships its own librccl.so) must be joined, not
    // doubled -- two copies interpose each other's globals and the process dies in their destructors at exit.  So: the copy that
    // is already loaded, if any; otherwise a private one (local scope, own symbols first) that a later-loaded copy cannot touch.
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* nm : names) {
        lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
        if (lib) break;
    }
    for (int k = 0; !lib && k < 3; ++k) lib = dlopen(names[k], RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
    if (!lib) { set_error("cannot dlopen librccl.so: %s", dlerror()); return FOS_ECOMM; }
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(lib, "ncclAllReduce");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) {
        set_error("librccl.so lacks a required symbol");
        return FOS_ECOMM;
    }
    g_rccl.lib = lib;
    return FOS_OK;
}

// an RCCL call: its failure is reported under the call's name
static int nccl_ok(const char* call, ncclResult_t r) {
    if (r != ncclSuccess) { set_error("%s -> %s", call, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "rccl error"); return FOS_ECOMM; }
    return FOS_OK;
}
#define FOS_NCCL(call, ...) FOS_TRY(nccl_ok(#call, g_rccl.call(__VA_ARGS__)))

// ------------------------------------------------------------------------------------------------ the sums
// the caller's collective: stage `count` doubles through the pinned host buffer (synchronises the stream; a slow path by design)
static int host_allreduce(fos_solver* h, const double* src, double* dst, size_t count) {
    const Transport& t = h->tr;
    if (hipMemcpyAsync(t.host_buf, src, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return FOS_EHIP;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return FOS_EHIP;
    if (t.host_fn(t.host_user, t.host_buf, (int64_t)count) != 0) { set_error("the caller's all-reduce callback failed"); return FOS_ECOMM; }
    if (hipMemcpyAsync(dst, t.host_buf, sizeof(double) * count, hipMemcpyHostToDevice, h->stream) != hipSuccess) return FOS_EHIP;
    return hipStreamSynchronize(h->stream) == hipSuccess ? FOS_OK : FOS_EHIP;          // the buffer is reused by the next call
}

// all-reduce of `count` doubles in h->reduced (in place, in stream) when sharded
int allreduce(fos_solver* h, int count) {
    switch (h->tr.via()) {
    case VIA_HOST: return host_allreduce(h, h->reduced, h->reduced, (size_t)count);
    case VIA_RCCL: return nccl_ok("AllReduce", g_rccl.AllReduce(h->reduced, h->reduced, (size_t)count, ncclDouble, ncclSum, h->tr.comm, h->stream));
    default: return FOS_OK;                                    // peer mailboxes: launch_reduce1 already exchanged; not sharded: nothing to do
    }
}

// partials[count][nacc] --(sharded: local reduce + all-reduce)--> returns from_reduced flag for the finalize kernel
int finish_reduce(fos_solver* h, const LaunchCtx& c, int count, int nacc, int gate, int* from_reduced, int off) {
    if (!h->sharded()) { *from_reduced = 0; return FOS_OK; }
    launch_reduce1(c, count, nacc, gate, off);
    FOS_TRY(allreduce(h, nacc));
    *from_reduced = 1;
    return FOS_OK;
}

// ------------------------------------------------------------------------------------------------ the environment's two switches
bool peer_fold_env() {          // 0: the mailbox exchange in its own kernel instead of folded into the CG kernels.  Read once per process.
    static const bool on = [] { const char* e = getenv("FOS_PEER_FOLD"); return !(e && atoi(e) == 0); }();
    return on;
}
// 1: a rank's own words travel through the mailbox too (measurement).  Read at every open.
bool peer_loopback_env() { const char* e = getenv("FOS_PEER_LOOPBACK"); return e && atoi(e) != 0; }

// ------------------------------------------------------------------------------------------------ the shm segment: POSIX only, no HIP call
// unmap, close the descriptor, unlink the name if this process created it; the segment is empty afterwards
static void host_seg_close(HostSeg& s) {
    if (s.p) (void)munmap(s.p, s.bytes);
    if (s.fd >= 0) (void)close(s.fd);
    if (s.creator) (void)shm_unlink(s.name.c_str());
    s = HostSeg{};
}

// `create` (rank 0) CREATES the segment -- exclusively, after unlinking whatever a crashed run left under the name: a fresh segment is zero filled (sequence
// number 0 is never sent), a reused one would carry sequence-tagged words that validate themselves.  The other ranks open it WITHOUT creating, waiting for it to
// appear at its full size.  A rank that was quick enough to open a stale segment before rank 0 unlinked it holds an unlinked file: host_seg_stale says so
// (fos_peer_selftest asks, behind the caller's barrier).  The last page is every rank's device identity (HostSeg::ids), zero until a rank has written its own.
// false: *why says what failed, and the failure went through host_seg_close -- no mapping, no descriptor, no name of this call's making is left.
static bool host_seg_open(HostSeg& s, const char* name, size_t bytes, bool create, double wait_s, std::string* why) {
    auto fail = [&](const char* call, const char* detail) { *why = std::string(call) + "(" + name + "): " + detail; host_seg_close(s); return false; };
    s = HostSeg{};
    s.name = name; s.bytes = bytes;
    const auto t0 = std::chrono::steady_clock::now();
    if (create) {
        (void)shm_unlink(name);
        s.fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (s.fd < 0 && errno == EEXIST) { (void)shm_unlink(name); s.fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600); }
        if (s.fd < 0) return fail("shm_open O_CREAT | O_EXCL", strerror(errno));
        s.creator = true;
        if (ftruncate(s.fd, (off_t)bytes) != 0) return fail("ftruncate", strerror(errno));
    } else for (;;) {
        struct stat sb;
        s.fd = shm_open(name, O_RDWR, 0600);
        if (s.fd >= 0 && fstat(s.fd, &sb) == 0 && (size_t)sb.st_size >= bytes) break;
        if (s.fd < 0 && errno != ENOENT) return fail("shm_open", strerror(errno));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > wait_s) return fail("shm_open", "rank 0 did not create the segment in time");
        if (s.fd >= 0) { (void)close(s.fd); s.fd = -1; }
        usleep(1000);
    }
    void* q = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, s.fd, 0);
    if (q == MAP_FAILED) return fail("mmap", strerror(errno));
    s.p = q;
    return true;
}

// the mapped file is no longer linked under its name: a segment some crashed run left behind, opened before rank 0 got to replacing it
static bool host_seg_stale(const HostSeg& s) { struct stat sb; return s.fd >= 0 && (fstat(s.fd, &sb) != 0 || sb.st_nlink == 0); }

// ------------------------------------------------------------------------------------------------ the scaffold of the opens and the close
// a block of the uncached pool, the handle's until fos_destroy: zeroed when it is taken (sequence number 0 is never sent), and again where `rezero`
template <class T> static int pool_zeroed(fos_solver* h, T** p, size_t bytes, const char* what, bool rezero = false) {
    void* q = *p;
    if (!q) {
        FOS_TRY(uncached_acquire(h->device, bytes, false, &q, what));
        h->pooled.push_back(q);
        rezero = true;
    }
    if (rezero) FOS_HIP(hipMemset(q, 0, bytes));
    *p = static_cast<T*>(q);
    return FOS_OK;
}

static void ipc_close(std::vector<void*>& opened) { for (void* q : opened) (void)hipIpcCloseMemHandle(q); opened.clear(); }

// tab[r] = rank r's block: `own` for this rank, the IPC mapping of handles[r] (64 bytes each) for the nranks - 1 others, which `opened` lists.  The first
// mapping that fails closes those before it.
static int ipc_open_peers(int nranks, int rank, const void* handles, void* own, const char* what, std::vector<void*>& opened, std::vector<void*>& tab) {
    tab.assign((size_t)nranks, own);
    for (int r = 0; r < nranks; ++r) {
        if (r == rank) continue;
        hipIpcMemHandle_t ipc;
        memcpy(&ipc, (const char*)handles + (size_t)r * sizeof(ipc), sizeof(ipc));
        const hipError_t e = hipIpcOpenMemHandle(&tab[r], ipc, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ipc_close(opened);
            set_error("hipIpcOpenMemHandle(%s of rank %d): %s", what, r, hipGetErrorString(e));
            return FOS_ECOMM;
        }
        opened.push_back(tab[r]);
    }
    return FOS_OK;
}

// The one close path -- of fos_peer_close, of fos_destroy (`destroy`: the communicator and the callback's buffer go too) and of a mailbox open that fails: whatever
// is mapped from other ranks is dropped, and the installed mailbox state with it (the small device tables stay owned by the handle until fos_destroy).
void transport_teardown(fos_solver* h, bool destroy) {
    Transport& t = h->tr;
    if (destroy && t.comm && g_rccl.CommDestroy) g_rccl.CommDestroy(t.comm);
    if (destroy && t.host_buf) (void)hipHostFree(t.host_buf);
    t.peer_on = false;
    ipc_close(t.peer_opened);
    ipc_close(t.vec_opened);
    t.vec = VecBox{};
    if (t.host_seg.p) (void)hipHostUnregister(t.host_seg.p);
    host_seg_close(t.host_seg);
    t.peer = PeerBox{};
    t.peer_same_device = false;
}

// the installed mailbox state of either kind: tab[r] = rank r's mailbox as this device addresses it; relay != nullptr: the host-pinned kind (all tab[r] one segment)
static int peer_install(fos_solver* h, int nranks, int rank, const std::vector<void*>& tab, double timeout_s, unsigned long long* relay) {
    void** dtab = nullptr;
    FOS_TRY(dev_upload(h, &dtab, tab));
    uint32_t* seq = nullptr;
    FOS_TRY(dev_alloc(h, &seq, 1));
    FOS_HIP(hipMemset(seq, 0, sizeof(uint32_t)));
    PeerBox& b = h->tr.peer = PeerBox{};
    b.box = reinterpret_cast<unsigned long long**>(dtab); b.seq = seq; b.nranks = nranks; b.rank = rank;
    b.timeout_ticks = (int64_t)((timeout_s > 0 ? timeout_s : 20.0) * 1e8);
    b.relay = relay; b.shared = relay ? 1 : 0; b.loopback = peer_loopback_env() ? 1 : 0;
    h->nranks = nranks; h->rank = rank;
    return FOS_OK;
}

// ... and of the vector exchange: tab[r] = rank r's buffer, its flags behind the [2][nranks][2n] doubles
static int vec_install(fos_solver* h, const std::vector<void*>& tab) {
    const size_t doubles = (size_t)2 * tab.size() * 2 * (size_t)h->n;
    std::vector<double*> bt;
    std::vector<uint32_t*> ft;
    for (void* q : tab) { bt.push_back(static_cast<double*>(q)); ft.push_back(reinterpret_cast<uint32_t*>(bt.back() + doubles)); }
    double** dbt = nullptr; uint32_t** dft = nullptr; uint32_t* cnt = nullptr;
    FOS_TRY(dev_upload(h, &dbt, bt));
    FOS_TRY(dev_upload(h, &dft, ft));
    FOS_TRY(dev_alloc(h, &cnt, 1));
    FOS_HIP(hipMemset(cnt, 0, sizeof(uint32_t)));
    VecBox& v = h->tr.vec;
    v.buf = dbt; v.flags = dft; v.counter = cnt; v.nranks = h->tr.peer.nranks; v.rank = h->tr.peer.rank;
    v.n2 = 2 * h->n; v.timeout_ticks = h->tr.peer.timeout_ticks;
    return FOS_OK;
}

// a failed exchange leaves its mark in the device state: clear it, the next transport starts clean
static int clear_exchange_failure(fos_solver* h) {
    DevState z;
    FOS_HIP(hipMemcpy(&z, h->st, sizeof(DevState), hipMemcpyDeviceToHost));
    z.xchg_failed = 0; z.done = 0;
    FOS_HIP(hipMemcpy(h->st, &z, sizeof(DevState), hipMemcpyHostToDevice));
    h->st_host->xchg_failed = 0;
    return FOS_OK;
}

}  // namespace fos

using namespace fos;

// row-sharded operators: slots (this rank's partial sums of A'y, 2n doubles) -> slots_rd (their sum over the ranks), in stream
int fos_solver::sum_slots_over_ranks(void* self) {
    fos_solver* h = static_cast<fos_solver*>(self);
    Transport& t = h->tr;
    const double* src = h->op.dev.slots;       // one slot per row of A' ...
    if (h->op.cmp_local) {                     // ... or, with dual tiles, the rows' local slot lists added up first
        launch_slots_compact(h->ctx(), (int)h->n, h->op.cmp_rec, h->op.cmp_idx, h->op.cmp_lpr, h->op.dev.slots, h->op.cmp_local);
        src = h->op.cmp_local;
    }
    const size_t n2 = (size_t)2 * (size_t)h->n;
    switch (t.via()) {
    case VIA_HOST: return host_allreduce(h, src, h->op.slots_rd, n2);
    case VIA_PEER:             // peer-mapped memory: push + sum, in stream, no library call
        if (t.vec.buf) { launch_vec_exchange(h->ctx(), t.vec, ++t.vec_seq, src, h->op.slots_rd); return FOS_OK; }
        [[fallthrough]];
    case VIA_RCCL:
        if (t.comm) return nccl_ok("AllReduce", g_rccl.AllReduce(src, h->op.slots_rd, n2, ncclDouble, ncclSum, t.comm, h->stream));
        [[fallthrough]];
    case VIA_NONE: break;      // no communicator yet (set-up calls before fos_comm_init, or a single process): the sum is the copy
    }
    return hipMemcpyAsync(h->op.slots_rd, src, sizeof(double) * n2, hipMemcpyDeviceToDevice, h->stream) == hipSuccess ? FOS_OK : FOS_EHIP;
}

extern "C" {

int fos_comm_get_unique_id(void* id128) {
    FOS_TRY(rccl_load());
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    FOS_NCCL(GetUniqueId, &id);
    memcpy(id128, &id, sizeof(id));
    return FOS_OK;
}

// an equilibrated handle (fos_create3) cannot be a shard: its scaling came from this handle's data alone
static int eq_refuse_sharding() {
    set_error("an equilibrated handle cannot be sharded: a rank knows neither the other ranks' column norms nor the global sigma, rho (create it with equil_passes = 0)");
    return FOS_EUNSUPPORTED;
}
// nor can a wrapped one: the searches' norms and the planes' Gram products are sums over this rank's part only (wrappers_check refuses the other order)
static int wrappers_refuse_sharding() {
    set_error("switch the LineSearchWrapper / GAPP / LongstepWrapper off before sharding the handle (fos_set_linesearch(h, 0), fos_set_gapp(h, 0), fos_set_longstep(h, 0, 0))");
    return FOS_EUNSUPPORTED;
}
int fos_comm_init(fos_handle h, int nranks, int rank, const void* id128) {
    if (!h || nranks < 1 || rank < 0 || rank >= nranks) { set_error("bad comm arguments"); return FOS_EINVAL; }
    if (h->equilibrated()) return eq_refuse_sharding();
    if (h->wr.active()) return wrappers_refuse_sharding();
    FOS_TRY(rccl_load());
    FOS_HIP(hipSetDevice(h->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    FOS_NCCL(CommInitRank, &h->tr.comm, nranks, id, rank);
    h->nranks = nranks; h->rank = rank;
    return global_setup(h);            // all-reduce [n+m, ||b||^2, ||c||^2]
}

// Sharding with the CALLER's collective (MPI.jl's Allreduce!, torch.distributed on any backend, ...): every cross-rank sum is
// staged through a pinned host buffer and handed to `fn` (in place, blocking).  Correct for both shardings, slow (one stream
// synchronisation per sum): the path for a host that owns no RCCL communicator, and the one a single-GPU box can run with two
// processes (tests/test_gpu_peer_mailbox.py::test_row_sharded_two_processes_host_exchange).
int fos_comm_init_host(fos_handle h, int nranks, int rank, fos_allreduce_fn fn, void* user) {
    if (!h || !fn || nranks < 1 || rank < 0 || rank >= nranks) { set_error("bad comm arguments"); return FOS_EINVAL; }
    if (h->equilibrated()) return eq_refuse_sharding();
    if (h->wr.active()) return wrappers_refuse_sharding();
    Transport& t = h->tr;
    if (t.comm || t.peer_on) { set_error("this handle already has a communicator"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (!t.host_buf) {
        void* q = nullptr;
        FOS_HIP(hipHostMalloc(&q, sizeof(double) * std::max<size_t>((size_t)2 * (size_t)h->n, 16), hipHostMallocDefault));
        t.host_buf = static_cast<double*>(q);
    }
    t.host_fn = fn; t.host_user = user;
    h->nranks = nranks; h->rank = rank;
    return global_setup(h);
}

// ---- peer mailboxes: the sharded scalar sums without a collective library (fos_internal.hpp, PeerBox)
int fos_peer_export(fos_handle h, void* handle64) {
    if (!h || !handle64) { set_error("NULL argument"); return FOS_EINVAL; }
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    FOS_HIP(hipSetDevice(h->device));
    FOS_TRY(pool_zeroed(h, &h->tr.peer_mbox, PEER_BOX_TOTAL_WORDS * sizeof(unsigned long long), "mailbox"));      // region 0 + region 1 (four slots)
    hipIpcMemHandle_t ipc;
    FOS_HIP(hipIpcGetMemHandle(&ipc, h->tr.peer_mbox));
    memcpy(handle64, &ipc, sizeof(ipc));
    return FOS_OK;
}

int fos_peer_open(fos_handle h, int nranks, int rank, const void* handles, double timeout_s) {
    if (!h || !handles || nranks < 1 || nranks > PEER_MAX_RANKS || rank < 0 || rank >= nranks) {
        set_error("bad peer arguments (1 <= nranks <= %d)", PEER_MAX_RANKS); return FOS_EINVAL;
    }
    if (h->equilibrated()) return eq_refuse_sharding();
    Transport& t = h->tr;
    if (!t.peer_mbox) { set_error("fos_peer_open before fos_peer_export"); return FOS_EINVAL; }
    if (!t.peer_opened.empty() || t.peer.box) { set_error("peer mailboxes are already open"); return FOS_EINVAL; }
    if (t.comm && (h->nranks != nranks || h->rank != rank)) { set_error("peer ranks differ from the RCCL communicator's"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    std::vector<void*> tab;
    FOS_TRY(ipc_open_peers(nranks, rank, handles, t.peer_mbox, "mailbox", t.peer_opened, tab));
    // first contact between DIFFERENT devices: the mapping can succeed where loads and stores over the link cannot -- ask the
    // runtime, and say which pair it is (the caller falls back to its collective: bench.py `peer_fallback_reason`)
    int rc = FOS_OK;
    for (int r = 0; r < nranks && rc == FOS_OK; ++r) {
        hipPointerAttribute_t attr;
        if (r == rank) continue;
        const bool known = hipPointerGetAttributes(&attr, tab[r]) == hipSuccess;
        if (known && attr.device == h->device) t.peer_same_device = true;
        int can = 0;
        if (!(known && attr.device >= 0 && attr.device != h->device)) (void)hipGetLastError();
        else if (hipDeviceCanAccessPeer(&can, h->device, attr.device) == hipSuccess && !can) {
            set_error("device %d cannot access the memory of device %d, rank %d's (hipDeviceCanAccessPeer = 0)", h->device, attr.device, r);
            rc = FOS_ECOMM;
        }
    }
    if (rc == FOS_OK) rc = peer_install(h, nranks, rank, tab, timeout_s, nullptr);
    if (rc != FOS_OK) transport_teardown(h);
    return rc;
}

// Host-pinned mailboxes: ONE shm segment of mailbox size that every rank maps and registers; every box[r] is that segment (PeerBox::shared),
// workgroup 0 of a folded exchange republishes the peers' words in a local relay (PeerBox::relay).
int fos_peer_open_host(fos_handle h, int nranks, int rank, const char* shm_name, double timeout_s) {
    if (!h || !shm_name || shm_name[0] != '/' || nranks < 1 || nranks > PEER_MAX_RANKS || rank < 0 || rank >= nranks) {
        set_error("bad arguments (shm_name \"/...\", 1 <= nranks <= %d)", PEER_MAX_RANKS); return FOS_EINVAL;
    }
    if (h->equilibrated()) return eq_refuse_sharding();
    Transport& t = h->tr;
    if (!t.peer_opened.empty() || t.peer.box || t.host_seg.p) { set_error("peer mailboxes are already open (fos_peer_close first)"); return FOS_EINVAL; }
    if (h->row_sharded) { set_error("host-pinned mailboxes carry the scalar sums of cone-sharded handles only"); return FOS_EUNSUPPORTED; }
    if (t.comm && (h->nranks != nranks || h->rank != rank)) { set_error("peer ranks differ from the RCCL communicator's"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    // (one more page behind the mailbox words: every rank's device identity, so that ranks which share a device can find out -- fos_peer_selftest)
    const size_t bytes = ((PEER_BOX_TOTAL_WORDS * sizeof(unsigned long long) + 4095) / 4096) * 4096 + 4096;
    FOS_TRY(pool_zeroed(h, &t.peer_relay, PEER_BOX_TOTAL_WORDS * sizeof(unsigned long long), "relay", true));
    std::string why;
    if (!host_seg_open(t.host_seg, shm_name, bytes, rank == 0, timeout_s > 0 ? std::max(timeout_s, 5.0) : 20.0, &why)) { set_error("%s", why.c_str()); return FOS_ECOMM; }
    // from here on a failure ends in transport_teardown: unregistered, unmapped, closed, the name unlinked by rank 0
    int rc = FOS_ECOMM;
    void* dptr = nullptr;
    hipError_t e = hipHostRegister(t.host_seg.p, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dptr, t.host_seg.p, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipHostRegister / hipHostGetDevicePointer(%s): %s", shm_name, hipGetErrorString(e));
    } else {
        char bus[64] = {0};
        unsigned long long id = 0x9E3779B97F4A7C15ull;
        if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), h->device) == hipSuccess) { for (const char* q = bus; *q; ++q) id = (id ^ (unsigned char)*q) * 0x100000001B3ull; }
        else { (void)hipGetLastError(); id ^= (unsigned long long)(h->device + 1); }
        t.host_seg.ids()[rank] = id | 1ull;                     // (never zero: a zero entry = that rank has not opened the segment yet)
        rc = peer_install(h, nranks, rank, std::vector<void*>((size_t)nranks, dptr), timeout_s, t.peer_relay);
    }
    if (rc != FOS_OK) { transport_teardown(h); (void)hipGetLastError(); }
    return rc;
}

// drop the open mailboxes (device or host): another transport may be opened on the handle afterwards
int fos_peer_close(fos_handle h) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipStreamSynchronize(h->stream));
    if (h->tr.peer_on) FOS_TRY(fos_peer_enable(h, 0));
    transport_teardown(h);
    if (h->tr.peer_mbox) FOS_TRY(pool_zeroed(h, &h->tr.peer_mbox, PEER_BOX_TOTAL_WORDS * sizeof(unsigned long long), "mailbox", true));   // (a re-opened mailbox starts its sequence numbers again)
    return clear_exchange_failure(h);
}

// `rounds` exchanges of known values, checked exactly; *ok = 0 on a mismatch or a time-out (the handle then keeps
// whatever reduction it had: RCCL if fos_comm_init was called).  Collective: every rank calls it with the same rounds.
int fos_peer_selftest(fos_handle h, int rounds, int32_t* ok) {
    if (!h || !ok) { set_error("NULL argument"); return FOS_EINVAL; }
    Transport& t = h->tr;
    if (!t.peer.box) { set_error("fos_peer_selftest before fos_peer_open"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    if (t.host_seg.p) {
        // (the caller's barrier stands between the opens and this call: rank 0 has unlinked and re-created the segment by now)
        if (host_seg_stale(t.host_seg)) {
            set_error("rank %d mapped a stale shared-memory segment under %s (a crashed run's): the self test fails, use another transport or name", t.peer.rank, t.host_seg.name.c_str());
            *ok = 0;
            return FOS_OK;
        }
        // host-pinned mailboxes: do ranks share THIS device (tests: several ranks on one GPU)?  Every rank left its device's identity behind the
        // mailbox words when it opened the segment, and the caller's barrier stands between the opens and this call.  A shared device keeps the
        // PSD refinement kernel to small batches (it needs whole CUs, which a peer's spinning CG kernel may hold: DESIGN 3)
        const volatile unsigned long long* ids = t.host_seg.ids();
        for (int r = 0; r < t.peer.nranks; ++r)
            if (r != t.peer.rank && ids[r] != 0ull && ids[r] == ids[t.peer.rank]) t.peer_same_device = true;
    }
    LaunchCtx c = h->ctx(true);                 // the mailboxes attached, whether or not the sums go through them yet
    *ok = 1;
    auto val = [](int r, int k, int a) { return (a == 0) ? (double)(r + 1) * (k + 1) : (a == 1 ? 0.1 * (r + 1) + 1e-3 * k : -1.0 / (r + 1 + k)); };
    for (int k = 0; k < rounds && *ok; ++k) {
        const int nacc = (k % 3 == 0) ? 3 : (k % 3 == 1 ? 1 : 6);
        double loc[6], got[6];
        for (int a = 0; a < nacc; ++a) loc[a] = val(t.peer.rank, k, a % 3) + a;
        FOS_HIP(hipMemcpyAsync(h->partials, loc, sizeof(double) * nacc, hipMemcpyHostToDevice, h->stream));
        launch_reduce1(c, 1, nacc, 0);
        FOS_HIP(hipMemcpyAsync(got, h->reduced, sizeof(double) * nacc, hipMemcpyDeviceToHost, h->stream));
        FOS_HIP(hipMemcpyAsync(h->st_host, h->st, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
        FOS_HIP(hipStreamSynchronize(h->stream));
        if (h->st_host->xchg_failed) { *ok = 0; break; }
        for (int a = 0; a < nacc; ++a) {
            double s = 0.0;
            for (int r = 0; r < t.peer.nranks; ++r) s += val(r, k, a % 3) + a;
            if (s != got[a]) *ok = 0;
        }
    }
    if (h->st_host->xchg_failed) FOS_TRY(clear_exchange_failure(h));     // leave the handle usable with its previous reduction
    return FOS_OK;
}

// What ONE exchange of four doubles costs on the transport this sharded handle uses -- `rounds` of them back to back, in stream, between two events:
// mailboxes: inside one launch (no launch or host round trip between them); RCCL: `rounds` ncclAllReduce calls.  Collective (every rank, same rounds).
int fos_exchange_bench(fos_handle h, int rounds, double* us_per_exchange) {
    if (!h || !us_per_exchange || rounds < 1) { set_error("bad argument"); return FOS_EINVAL; }
    *us_per_exchange = 0.0;
    const ReduceVia via = h->tr.via();
    if (via != VIA_PEER && via != VIA_RCCL) { set_error("fos_exchange_bench: the handle has no in-stream transport (mailboxes or RCCL)"); return FOS_EUNSUPPORTED; }
    FOS_HIP(hipSetDevice(h->device));
    LaunchCtx c = h->ctx();
    hipEvent_t e0, e1;
    FOS_HIP(hipEventCreate(&e0));
    FOS_HIP(hipEventCreate(&e1));
    auto run = [&](int n) -> int {
        switch (via) {
        case VIA_PEER: launch_peer_chain(c, n); return FOS_OK;
        default: for (int r = 0; r < n; ++r) FOS_TRY(allreduce(h, 4)); return FOS_OK;
        }
    };
    int rc = run(4);                                     // warm
    if (rc == FOS_OK) rc = hipEventRecord(e0, h->stream) == hipSuccess ? FOS_OK : FOS_EHIP;
    if (rc == FOS_OK) rc = run(rounds);
    if (rc == FOS_OK) rc = hipEventRecord(e1, h->stream) == hipSuccess ? FOS_OK : FOS_EHIP;
    if (rc == FOS_OK) rc = poll_state(h);
    float ms = 0.f;
    if (rc == FOS_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = FOS_EHIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != FOS_OK) return rc;
    *us_per_exchange = 1e3 * (double)ms / (double)rounds;
    return FOS_OK;
}

// Row-sharded handles: the exchange buffer of the n-vector A'y (fos_internal.hpp, VecBox).  Protocol as for the mailboxes, after
// fos_peer_open (which fixes nranks): fos_peer_vec_export -> the host all-gathers the 64-byte handles -> fos_peer_vec_open.
int fos_peer_vec_export(fos_handle h, void* handle64) {
    if (!h || !handle64) { set_error("NULL argument"); return FOS_EINVAL; }
    if (!h->row_sharded) { set_error("fos_peer_vec_export: not a row-sharded handle"); return FOS_EINVAL; }
    Transport& t = h->tr;
    if (!t.peer.box) { set_error("fos_peer_vec_export before fos_peer_open"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    const size_t g = (size_t)t.peer.nranks, doubles = 2 * g * 2 * (size_t)h->n;
    FOS_TRY(pool_zeroed(h, &t.vec_buf, doubles * sizeof(double) + 4 * g * sizeof(uint32_t) + 64, "vector exchange buffer"));   // flags: [stage 1 | stage 2][parity][rank]
    hipIpcMemHandle_t ipc;
    FOS_HIP(hipIpcGetMemHandle(&ipc, t.vec_buf));
    memcpy(handle64, &ipc, sizeof(ipc));
    return FOS_OK;
}
int fos_peer_vec_open(fos_handle h, const void* handles) {
    if (!h || !handles) { set_error("NULL argument"); return FOS_EINVAL; }
    Transport& t = h->tr;
    if (!t.vec_buf || !t.peer.box) { set_error("fos_peer_vec_open before fos_peer_vec_export"); return FOS_EINVAL; }
    if (!t.vec_opened.empty() || t.vec.buf) { set_error("the vector exchange buffers are already open"); return FOS_EINVAL; }
    FOS_HIP(hipSetDevice(h->device));
    std::vector<void*> tab;
    FOS_TRY(ipc_open_peers(t.peer.nranks, t.peer.rank, handles, t.vec_buf, "vector exchange buffer", t.vec_opened, tab));
    const int rc = vec_install(h, tab);
    if (rc != FOS_OK) ipc_close(t.vec_opened);
    return rc;
}

// switch the sharded sums to the peer mailboxes (collective: all ranks make the same choice after the self test)
int fos_peer_enable(fos_handle h, int32_t on) {
    if (!h) { set_error("NULL handle"); return FOS_EINVAL; }
    if (on && !h->tr.peer.box) { set_error("fos_peer_enable before fos_peer_open"); return FOS_EINVAL; }
    if (on && h->row_sharded && !h->tr.vec.buf) { set_error("row-sharded handle: fos_peer_vec_export / fos_peer_vec_open before fos_peer_enable"); return FOS_EINVAL; }
    if (on && h->wr.active()) return wrappers_refuse_sharding();
    FOS_HIP(hipSetDevice(h->device));
    FOS_HIP(hipStreamSynchronize(h->stream));
    h->tr.peer_on = on != 0;
    if (h->sharded()) return global_setup(h);
    h->l_global = h->l; h->nb = h->nb_local; h->nc = h->nc_local;
    return resident_setup(h, h->cus);          // (the whole device is this handle's again)
}

}  // extern "C"
