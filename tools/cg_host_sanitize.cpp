// The two pure rules of the CG solve (csrc/cg.cpp: fos_host_cg_windows, fos_host_cg_variant) under AddressSanitizer and UBSan, on the cases of
// tests/test_cg_host.py.  A program of its own: nothing is loaded into Python, nothing runs on a GPU.  cg.cpp is compiled INTO the program with the
// sanitizers; everything else it refers to comes from the library as built:
//   cd firstordersolvers.jl_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I../../include -Xarch_host -fsanitize=address,undefined \
//       -x hip cg.cpp ../../tools/cg_host_sanitize.cpp -L. -lfoship -Wl,-rpath,$PWD -o /tmp/cg_host_sanitize && /tmp/cg_host_sanitize
#include <cstdint>
#include <cstdio>

#include "foship.h"

int main() {
    const int64_t maxits[] = {0, 1, 1021, 1022, 1023, 1000, 10000, 2147483647LL};
    const int64_t epochs[] = {0, 1, (1LL << 21) - 2, (1LL << 21) - 1, 1LL << 21, 3 * (1LL << 21) - 3, (1LL << 32) - 2049};
    long long sum = 0, calls = 0;
    for (int64_t e : epochs)
        for (int64_t k : maxits) {
            int64_t first = 0, last = 0;
            if (fos_host_cg_windows(e, k, &first, &last) != FOS_OK) { fprintf(stderr, "fos_host_cg_windows(%lld, %lld) failed\n", (long long)e, (long long)k); return 1; }
            sum += first ^ last; ++calls;
        }
    const int64_t ls[] = {32767, 32768, 100000};
    const int32_t Gs[] = {127, 128, 256};
    for (int32_t request = -1; request <= FOS_CG_RESIDENT; ++request)
        for (int32_t flags = 0; flags < 0x800; ++flags)
            for (int64_t l : ls)
                for (int32_t G : Gs) {
                    int32_t v = -1;
                    if (fos_host_cg_variant(request, flags, l, G, 256, &v) != FOS_OK || v < FOS_CG_REFERENCE || v > FOS_CG_RESIDENT) { fprintf(stderr, "fos_host_cg_variant failed\n"); return 1; }
                    sum += v; ++calls;
                }
    printf("%lld calls, checksum %lld: no report\n", calls, sum);
    return 0;
}
