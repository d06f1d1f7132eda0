// What a float stream read again and again costs per round, by where it is served from: the ceiling of the streamed CG solve's fp32 sweeps.
// One persistent launch in the shape of rs_walk<float> (csrc/resident.hip): 256 workgroups of 512 threads, every wavefront walks its own contiguous
// share of a float buffer in 2 KB chunks of eight 256-byte wave loads, four chunks in flight, widens what it reads and spends four fp64 FMAs on every
// value (row sums against column elements in LDS, products into eight accumulator pairs), R rounds inside the launch, rounds following each other per
// wavefront -- or one launch per round ("meet").  Every wavefront stamps the 100 MHz clock in front of and behind each round.
//   hipcc --offload-arch=gfx950 -O3 tools/ub_stream_reread.hip -o build/ub_stream_reread && build/ub_stream_reread <MB> <policy> [rounds] [launches] [mode]
// policy: plain | nt (__builtin_nontemporal_load) | sc1 (relaxed agent-scope atomic load: bypasses the CU's L1).  One JSON line per process
// (tools/stream_reread.py runs the sizes and policies, one process each, into profiles/stream_reread_ceiling.json).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

constexpr int WG = 256, WAVES = 8, NWAVE = WG * WAVES, CHUNK = 512, RING = 4, RMAX = 16;
enum Policy { PLAIN = 0, NT = 1, SC1 = 2 };

template <int P> __device__ __forceinline__ float ld(const float* p) {
    if constexpr (P == NT) return __builtin_nontemporal_load(p);
    else if constexpr (P == SC1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// (always eight loads per request, as rs_request: the waits behind a chunk are exact counts)
template <int P> __device__ __forceinline__ void request(const float* __restrict__ base, long long chunk, int lane, float (&val)[8]) {
    const float* __restrict__ vp = base + chunk * CHUNK + lane;
#pragma unroll
    for (int t = 0; t < 8; ++t) val[t] = ld<P>(vp + 64 * t);
}

template <int P>
__global__ __launch_bounds__(64 * WAVES) void reread(const float* __restrict__ buf, long long chunks_per_wave, int rounds, double* __restrict__ out,
                                                     long long* __restrict__ stamps /* [NWAVE][RMAX][start, end] */, int r0) {
    __shared__ __attribute__((aligned(16))) double2 s_gcol[64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 64) s_gcol[threadIdx.x] = make_double2(1.0 + threadIdx.x * 1e-3, 1.0 - threadIdx.x * 1e-3);
    __syncthreads();
    const long long w = (long long)blockIdx.x * WAVES + wv;
    const float* __restrict__ mine = buf + w * chunks_per_wave * CHUNK;
    const double2 g = make_double2(1.0 + lane * 1e-6, 1.0 - lane * 1e-6);
    double2 u = make_double2(0.0, 0.0);
    double a1[8], a2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a1[k] = a2[k] = 0.0;
    for (int r = 0; r < rounds; ++r) {
        if (lane == 0) { stamps[(w * RMAX + r0 + r) * 2] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); }
        float val[RING][8];
#pragma unroll
        for (int s = 0; s < RING; ++s) request<P>(mine, s < chunks_per_wave ? s : chunks_per_wave - 1, lane, val[s]);
        for (long long c = 0; c < chunks_per_wave; c += RING) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                if (c + s < chunks_per_wave) {                       // wave-uniform
                    const double2* __restrict__ gcol = s_gcol + 8 * ((c + s) & 7);
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const double2 x0 = gcol[2 * h], x1 = gcol[2 * h + 1];
                        const double v0 = (double)val[s][2 * h], v1 = (double)val[s][2 * h + 1];
                        u.x += v0 * x0.x; u.y += v0 * x0.y; a1[2 * h] += v0 * g.x; a2[2 * h] += v0 * g.y;
                        u.x += v1 * x1.x; u.y += v1 * x1.y; a1[2 * h + 1] += v1 * g.x; a2[2 * h + 1] += v1 * g.y;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                // (the refill behind the walk's end reads the share's last chunk again: never consumed)
                const long long nxt = c + s + RING;
                request<P>(mine, nxt < chunks_per_wave ? nxt : chunks_per_wave - 1, lane, val[s]);
            }
        }
        if (lane == 0) { __builtin_amdgcn_sched_barrier(0); stamps[(w * RMAX + r0 + r) * 2 + 1] = wall_clock64(); }
    }
    double s = u.x + u.y;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += a1[k] + a2[k];
    out[w * 64 + lane] = s;
}

__global__ void fill(float* p, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = 1.0f + (float)(i & 1023) * 1e-3f;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <MB> <plain|nt|sc1> [rounds = 13] [launches = 3] [persistent|meet]\n", argv[0]); return 1; }
    const double mb = atof(argv[1]);
    const int pol = !strcmp(argv[2], "plain") ? PLAIN : !strcmp(argv[2], "nt") ? NT : !strcmp(argv[2], "sc1") ? SC1 : -1;
    const int rounds = argc > 3 ? atoi(argv[3]) : 13, launches = argc > 4 ? atoi(argv[4]) : 3;
    // persistent: the R rounds inside one launch, every wavefront on its own (they drift apart: late rounds are a few stragglers on an idle chip);
    // meet: one launch per round, back to back in one stream -- the rounds meet, as the solve's sweeps do at every exchange
    const bool meet = argc > 5 && !strcmp(argv[5], "meet");
    if (pol < 0 || mb <= 0.0 || rounds < 2 || rounds > RMAX || launches < 1) { fprintf(stderr, "bad arguments\n"); return 1; }
    const long long cpw = std::max<long long>(1, (long long)(mb * 1e6 / 4.0) / ((long long)NWAVE * CHUNK));
    const long long nflt = cpw * NWAVE * CHUNK;                  // every load of the kernel lies inside [0, nflt)
    const size_t flush_bytes = (size_t)640 << 20;                // more than the Infinity Cache: written in front of every launch, so round 1 starts cold
    float* buf; char* flush; double* out; long long* stamps;
    const size_t nst = (size_t)NWAVE * RMAX * 2;
    CK(hipMalloc(&buf, sizeof(float) * nflt)); CK(hipMalloc(&flush, flush_bytes));
    CK(hipMalloc(&out, sizeof(double) * NWAVE * 64)); CK(hipMalloc(&stamps, sizeof(long long) * nst));
    hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, buf, nflt);
    CK(hipDeviceSynchronize());
    std::vector<long long> h(nst);
    auto go = [&](int nr, int r0) {
        if (pol == PLAIN) hipLaunchKernelGGL(reread<PLAIN>, dim3(WG), dim3(64 * WAVES), 0, 0, buf, cpw, nr, out, stamps, r0);
        else if (pol == NT) hipLaunchKernelGGL(reread<NT>, dim3(WG), dim3(64 * WAVES), 0, 0, buf, cpw, nr, out, stamps, r0);
        else hipLaunchKernelGGL(reread<SC1>, dim3(WG), dim3(64 * WAVES), 0, 0, buf, cpw, nr, out, stamps, r0);
    };
    printf("{\"mb\": %.1f, \"bytes\": %lld, \"policy\": \"%s\", \"mode\": \"%s\", \"rounds\": %d, \"launches\": [", mb, nflt * 4, argv[2],
           meet ? "meet" : "persistent", rounds);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int l = 0; l < launches; ++l) {
        CK(hipMemset(flush, l, flush_bytes));
        CK(hipMemset(stamps, 0, sizeof(long long) * nst));
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        if (meet) for (int r = 0; r < rounds; ++r) go(1, r);
        else go(rounds, 0);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipMemcpy(h.data(), stamps, sizeof(long long) * nst, hipMemcpyDeviceToHost));
        // a round of the chip: from its first wavefront's start (persistent: from the end of the round before) to its last wavefront's end
        std::vector<double> chip(rounds);
        long long prev = 0;
        for (int r = 0; r < rounds; ++r) {
            long long start = h[(size_t)r * 2], end = 0;
            for (int w = 0; w < NWAVE; ++w) {
                start = std::min(start, h[((size_t)w * RMAX + r) * 2]);
                end = std::max(end, h[((size_t)w * RMAX + r) * 2 + 1]);
            }
            chip[r] = (end - (meet || r == 0 ? start : prev)) / 100.0; prev = end;
        }
        std::vector<double> rest(chip.begin() + 1, chip.end());
        std::sort(rest.begin(), rest.end());
        printf("%s{\"all_rounds_us\": %.1f, \"round1_us\": %.2f, \"rounds2_median_us\": %.2f, \"rounds2_min_us\": %.2f, \"rounds2_max_us\": %.2f, \"chip_us\": [",
               l ? ", " : "", ms * 1e3, chip[0], rest[rest.size() / 2], rest.front(), rest.back());
        for (int r = 0; r < rounds; ++r) printf("%s%.2f", r ? ", " : "", chip[r]);
        printf("]}");
    }
    printf("]}\n");
    return 0;
}
