// The sparse intake (csrc/sparse_rows.cpp: csc_check, csc_to_csr_pair, sf_plan_pass, lanes_per_row) under AddressSanitizer and UBSan: the fault table and the edge
// shapes of tests/test_sparse_intake_cpu.py and a few hundred random small matrices.  A program of its own: nothing is loaded into Python, nothing runs on a GPU,
// nothing comes from the library (sparse_rows.cpp includes no HIP header; set_error is defined below).  sparse_rows.cpp is compiled INTO the program:
//   cd firstordersolvers.jl_amd/csrc && clang++ -std=c++17 -O1 -g -I../../include -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       sparse_rows.cpp ../../tools/sparse_intake_sanitize.cpp -o /tmp/sparse_intake_sanitize && /tmp/sparse_intake_sanitize
// (plain C++: ROCm's clang++ or any other; on a hipcc line the flags are -Xarch_host -fsanitize=address,undefined)
// Every array handed over is exactly as long as the arguments say (a read past it is a report); every result is also compared with a dense restatement.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "sparse_rows.hpp"

namespace fos {
static std::string g_msg;
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_msg = buf;
}
}  // namespace fos

using namespace fos;

namespace {

struct Csc { int64_t m, n; std::vector<int64_t> cp, rv; std::vector<double> nz; };
unsigned long long g_sum = 0;
long long g_cases = 0;

[[noreturn]] void die(const char* what, const Csc& a) {
    fprintf(stderr, "FAILED: %s (%lld x %lld, %zu entries; last message \"%s\")\n", what, (long long)a.m, (long long)a.n, a.nz.size(), g_msg.c_str());
    exit(1);
}
void mix(long long v) { g_sum = g_sum * 1000003ULL + (unsigned long long)v; }

Csc from_dense(int64_t m, int64_t n, const std::vector<double>& d) {          // d row-major; a stored entry wherever d != 0
    Csc a{m, n, {1}, {}, {}};
    a.rv.reserve(1); a.nz.reserve(1);                                         // (nothing stored: the arrays still exist)
    for (int64_t j = 0; j < n; ++j) {
        for (int64_t i = 0; i < m; ++i) if (d[(size_t)(i * n + j)] != 0.0) { a.rv.push_back(i + 1); a.nz.push_back(d[(size_t)(i * n + j)]); }
        a.cp.push_back((int64_t)a.rv.size() + 1);
    }
    return a;
}

int check(const Csc& a, const CscRules& r) { return csc_check("intake", a.m, a.n, a.cp.data(), a.rv.data(), a.nz.data(), r); }
void expect(const Csc& a, const CscRules& r, int code, const char* text) {
    g_msg.clear();
    const int rc = check(a, r);
    if (rc != code || (code != FOS_OK && g_msg != std::string("intake: ") + text)) die(text, a);
    mix(rc); ++g_cases;
}

// a valid matrix: the pair against the dense matrix, every plan against the row lengths
void accept(const Csc& a, bool scaled) {
    static const CscRules rules[] = {{true, false, CSC_BOUND_BOTH, "A"}, {true, true, CSC_BOUND_BOTH, "A"}, {false, true, CSC_BOUND_ROWS, "A"},
                                     {false, true, CSC_BOUND_BOTH, "the matrix"}};
    const bool empty = a.nz.empty();
    for (const CscRules& r : rules) {
        g_msg.clear();
        const int rc = check(a, r);
        if (rc != (empty && r.refuse_empty ? FOS_EINVAL : FOS_OK)) die("a valid matrix was refused", a);
    }
    std::vector<double> scale((size_t)a.m);
    for (int64_t i = 0; i < a.m; ++i) scale[(size_t)i] = 0.5 + (double)(i % 3);
    HostCsr A, At;
    csc_to_csr_pair(a.m, a.n, a.cp.data(), a.rv.data(), a.nz.data(), scaled ? scale.data() : nullptr, &A, &At);
    std::vector<double> dense((size_t)(a.m * a.n), 0.0), fromA(dense), fromAt(dense);
    for (int64_t j = 0; j < a.n; ++j)
        for (int64_t e = a.cp[(size_t)j] - 1; e < a.cp[(size_t)j + 1] - 1; ++e) dense[(size_t)((a.rv[(size_t)e] - 1) * a.n + j)] = a.nz[(size_t)e] * (scaled ? scale[(size_t)(a.rv[(size_t)e] - 1)] : 1.0);
    if (A.rp.size() != (size_t)a.m + 1 || At.rp.size() != (size_t)a.n + 1) die("pair: shape", a);
    if (A.rp[0] != 0 || At.rp[0] != 0 || A.rp.back() != (int32_t)a.nz.size() || At.rp.back() != (int32_t)a.nz.size() || A.ci.size() != a.nz.size()) die("pair: pointers", a);
    for (int64_t i = 0; i < a.m; ++i)
        for (int32_t e = A.rp[(size_t)i]; e < A.rp[(size_t)i + 1]; ++e) {
            if (e > A.rp[(size_t)i] && A.ci[(size_t)e] <= A.ci[(size_t)e - 1]) die("pair: the columns of a row of A do not ascend", a);
            fromA[(size_t)(i * a.n + A.ci[(size_t)e])] = A.va[(size_t)e];
        }
    for (int64_t j = 0; j < a.n; ++j)
        for (int32_t e = At.rp[(size_t)j]; e < At.rp[(size_t)j + 1]; ++e) fromAt[(size_t)(At.ci[(size_t)e] * a.n + j)] = At.va[(size_t)e];
    if (fromA != dense || fromAt != dense) die("pair: entries", a);
    int longest = 0;
    for (int64_t i = 0; i < a.m; ++i) longest = std::max(longest, A.rp[(size_t)i + 1] - A.rp[(size_t)i]);
    if (A.longest() != longest) die("longest", a);
    for (const HostCsr* M : {&A, &At})
        for (int seg : {64, 2048}) {
            SfPass P;
            const int64_t nrows = (int64_t)M->rp.size() - 1;
            sf_plan_pass(nrows, M->rp.data(), seg, &P);
            std::vector<int> covered(M->ci.size(), 0), rows(M->rp.size() - 1, 0);
            size_t cut = 0;
            for (const SfItem& w : P.items) {
                if (w.c > 0) {                                                       // a segment of a cut row
                    if (w.c > seg || w.d < 0 || w.d >= P.nparts || w.b < M->rp[(size_t)w.a] || w.b + w.c > M->rp[(size_t)w.a + 1]) die("plan: segment", a);
                    for (int e = w.b; e < w.b + w.c; ++e) covered[(size_t)e]++;
                    rows[(size_t)w.a] = 1;
                } else {
                    const int g = -w.c;
                    if (g < 1 || g > 64 || (g & (g - 1)) || w.b < 1 || w.b * g > 64 || w.a + w.b > nrows) die("plan: packet", a);
                    for (int k = 0; k < w.b; ++k) {
                        const int row = w.a + k, len = M->rp[(size_t)row + 1] - M->rp[(size_t)row];
                        if (len > seg || (g < 64 && len > 4 * g) || rows[(size_t)row]) die("plan: packed row", a);
                        rows[(size_t)row] = 1;
                        for (int e = M->rp[(size_t)row]; e < M->rp[(size_t)row + 1]; ++e) covered[(size_t)e]++;
                    }
                }
                mix(w.a + 3 * w.b + 5 * w.c + 7 * w.d);
            }
            for (int c : covered) if (c != 1) die("plan: an entry is not covered exactly once", a);
            for (int r : rows) if (r != 1) die("plan: a row is missing", a);
            for (size_t k = 0; k < P.frow.size(); ++k) {
                if (M->rp[(size_t)P.frow[k] + 1] - M->rp[(size_t)P.frow[k]] <= seg || P.fptr[k + 1] <= P.fptr[k]) die("plan: fold table", a);
                ++cut;
            }
            if (P.fptr.size() != cut + 1 || P.fptr.back() != P.nparts) die("plan: slots", a);
        }
    const int l = lanes_per_row((int64_t)a.nz.size(), a.m);
    if (l < 1 || l > 64 || (l & (l - 1)) || (l > 1 && (double)l > (double)a.nz.size() / (double)a.m)) die("lanes_per_row", a);
    mix(l); ++g_cases;
}

}  // namespace

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const CscRules sorted{true, true, CSC_BOUND_BOTH, "A"}, unsorted{true, false, CSC_BOUND_BOTH, "A"}, cg{false, true, CSC_BOUND_BOTH, "the matrix"},
        normal{false, true, CSC_BOUND_ROWS, "A"};
    // the fault table, 3 x 5
    const Csc base = from_dense(3, 5, {2, 0, 1, 0, 3, 0, 4, 1, 0, 0, 1, 0, 0, 5, 2});
    const char* asc = "the row indices of column 1 are not strictly ascending (duplicated or unsorted entries)";
    for (const CscRules& r : {sorted, unsorted, cg, normal}) {
        expect(base, r, FOS_OK, "");
        Csc a = base; a.cp[0] = 0;                        expect(a, r, FOS_EINVAL, "colptr must be 1-based (colptr[0] = 0)");
        a = base; std::swap(a.cp[1], a.cp[2]);            expect(a, r, FOS_EINVAL, "colptr decreases at column 2");
        a = base; a.rv[1] = 0;                            expect(a, r, FOS_EINVAL, "row index 0 outside 1..3");
        a = base; a.rv[1] = 4;                            expect(a, r, FOS_EINVAL, "row index 4 outside 1..3");
        a = base; std::swap(a.rv[0], a.rv[1]);            expect(a, r, r.ascending ? FOS_EINVAL : FOS_OK, asc);
        a = base; a.rv[1] = a.rv[0];                      expect(a, r, r.ascending ? FOS_EINVAL : FOS_OK, asc);
        const std::string nonfinite = std::string(r.noun) + " has non-finite entries";
        for (double v : {nan, inf, -inf, 1e301}) { a = base; a.nz[3] = v; expect(a, r, FOS_EINVAL, nonfinite.c_str()); }
        a = base; a.cp.assign(6, 1); a.rv.clear(); a.nz.clear();
        expect(a, r, r.refuse_empty ? FOS_EINVAL : FOS_OK, "0 stored entries (1 .. 2e9 supported)");
        a = base; a.m = 0;                                expect(a, r, FOS_EINVAL, "bad argument");
        a = base; a.m = 3000000000LL;                     expect(a, r, FOS_EUNSUPPORTED, r.bound == CSC_BOUND_ROWS ? "m = 3000000000 rows (up to 2e9 supported)"
                                                                                                                     : "3000000000 x 5 (up to 2e9 rows and columns supported)");
        if (csc_check("intake", 3, 5, nullptr, base.rv.data(), base.nz.data(), r) != FOS_EINVAL) die("null colptr", base);
    }
    // the edge shapes
    accept(from_dense(4, 7, {0, 2, 0, 1, 0, 0, 0, 0, 0, 3, 0, 0, 1, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 4, 1, 0}), false);      // first and last column empty
    accept(from_dense(4, 7, {1, 2, 0, 1, 0, 0, 5, 0, 0, 3, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 4, 1, 7}), true);       // row 3 empty
    accept(from_dense(1, 6, {0, 1.5, 0, -2, 0.25, 0}), true);                                                                  // m = 1
    accept(from_dense(5, 1, {1, 0, -2, 0.5, 0}), false);                                                                       // n = 1
    accept(from_dense(1, 1, {3}), true);
    accept(from_dense(2, 3, {0, 0, 0, 0, 0, 0}), false);                                                                       // nothing stored
    {
        std::vector<double> d(6 * 8, 0.0), r(3 * 260, 0.0);
        for (int i = 0; i < 6; ++i) { d[(size_t)(i * 8)] = 1.0 + i; d[(size_t)(i * 8 + 1 + i)] = 2.0; }
        accept(from_dense(6, 8, d), true);                                                                                     // a dense column beside a diagonal
        for (int j = 0; j < 200; ++j) r[(size_t)(40 + j)] = 1.0 + j;
        for (int i = 0; i < 3; ++i) r[(size_t)(i * 260 + 1 + i)] = 2.0;
        accept(from_dense(3, 260, r), false);                                                                                  // a row of 201: cut at 64
        std::vector<double> big(2 * 2100, 1.0);
        accept(from_dense(2, 2100, big), true);                                                                                // cut at 2 048 too
    }
    // random small matrices: m, n <= 40, whole rows and columns emptied at random
    std::mt19937_64 rng(20);
    for (int t = 0; t < 400; ++t) {
        const int64_t m = 1 + (int64_t)(rng() % 40), n = 1 + (int64_t)(rng() % 40);
        const double density = (double)(rng() % 100) / 100.0;
        std::vector<double> d((size_t)(m * n), 0.0);
        std::vector<char> row_off((size_t)m), col_off((size_t)n);
        for (char& c : row_off) c = rng() % 5 == 0;
        for (char& c : col_off) c = rng() % 5 == 0;
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < n; ++j)
                if (!row_off[(size_t)i] && !col_off[(size_t)j] && (double)(rng() % 1000) / 1000.0 < density) d[(size_t)(i * n + j)] = 1.0 + (double)(rng() % 97);
        accept(from_dense(m, n, d), t % 2 == 0);
    }
    printf("%lld cases, checksum %llu: no report\n", g_cases, g_sum);
    return 0;
}
