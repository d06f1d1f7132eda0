// The sparse intake of the Feasibility sets and the plans of their row passes (sparse_rows.hpp): host code only.
#include "sparse_rows.hpp"

#include <algorithm>

namespace fos {

namespace {
constexpr int64_t CSC_MAX = 2000000000LL;     // rows, columns and stored entries: int32 indices on the device
constexpr int SF_LANE_ENTRIES = 4;            // packed rows: entries per lane of the packet's longest row, while g < 64
int sf_lanes(int len) {                       // the fewest lanes (a power of two, at most 64) that leave a lane at most SF_LANE_ENTRIES entries of a row
    int g = 1;
    while (g < 64 && g * SF_LANE_ENTRIES < len) g <<= 1;
    return g;
}
}  // namespace

int csc_check(const char* what, int64_t rows, int64_t cols, const int64_t* colptr, const int64_t* rowval, const double* nzval, const CscRules& rules) {
    if (rows < 1 || cols < 1 || !colptr || !rowval || !nzval) { set_error("%s: bad argument", what); return FOS_EINVAL; }
    if (rows > CSC_MAX || (rules.bound == CSC_BOUND_BOTH && cols > CSC_MAX)) {
        if (rules.bound == CSC_BOUND_ROWS) set_error("%s: m = %lld rows (up to 2e9 supported)", what, (long long)rows);
        else set_error("%s: %lld x %lld (up to 2e9 rows and columns supported)", what, (long long)rows, (long long)cols);
        return FOS_EUNSUPPORTED;
    }
    if (colptr[0] != 1) { set_error("%s: colptr must be 1-based (colptr[0] = %lld)", what, (long long)colptr[0]); return FOS_EINVAL; }
    for (int64_t j = 0; j < cols; ++j)
        if (colptr[j + 1] < colptr[j]) { set_error("%s: colptr decreases at column %lld", what, (long long)j + 1); return FOS_EINVAL; }
    const int64_t nnz = colptr[cols] - 1;
    if (rules.refuse_empty && (nnz < 1 || nnz > CSC_MAX)) { set_error("%s: %lld stored entries (1 .. 2e9 supported)", what, (long long)nnz); return FOS_EINVAL; }
    if (nnz > CSC_MAX) { set_error("%s: %lld stored entries (up to 2e9 supported)", what, (long long)nnz); return FOS_EINVAL; }
    for (int64_t j = 0; j < cols; ++j)
        for (int64_t e = colptr[j] - 1; e < colptr[j + 1] - 1; ++e) {
            if (rowval[e] < 1 || rowval[e] > rows) { set_error("%s: row index %lld outside 1..%lld", what, (long long)rowval[e], (long long)rows); return FOS_EINVAL; }
            if (rules.ascending && e > colptr[j] - 1 && rowval[e] <= rowval[e - 1]) {
                set_error("%s: the row indices of column %lld are not strictly ascending (duplicated or unsorted entries)", what, (long long)j + 1);
                return FOS_EINVAL;
            }
            if (!csc_finite(nzval[e])) { set_error("%s: %s has non-finite entries", what, rules.noun); return FOS_EINVAL; }
        }
    return FOS_OK;
}

void csc_to_csr_pair(int64_t rows, int64_t cols, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* row_scale, HostCsr* A, HostCsr* At) {
    const size_t nnz = (size_t)(colptr[cols] - 1);
    At->rp.resize((size_t)cols + 1); At->ci.resize(nnz); At->va.resize(nnz);
    A->rp.assign((size_t)rows + 1, 0); A->ci.resize(nnz); A->va.resize(nnz);
    for (int64_t j = 0; j <= cols; ++j) At->rp[(size_t)j] = (int32_t)(colptr[j] - 1);
    for (size_t e = 0; e < nnz; ++e) {
        const int32_t i = (int32_t)(rowval[e] - 1);
        At->ci[e] = i; At->va[e] = row_scale ? nzval[e] * row_scale[i] : nzval[e];
        A->rp[(size_t)i + 1]++;
    }
    for (int64_t i = 0; i < rows; ++i) A->rp[(size_t)i + 1] += A->rp[(size_t)i];
    std::vector<int32_t> next(A->rp.begin(), A->rp.end() - 1);
    for (int64_t j = 0; j < cols; ++j)
        for (int32_t e = At->rp[(size_t)j]; e < At->rp[(size_t)j + 1]; ++e) {
            const int32_t p = next[(size_t)At->ci[(size_t)e]]++;
            A->ci[(size_t)p] = (int32_t)j; A->va[(size_t)p] = At->va[(size_t)e];
        }
}

void sf_plan_pass(int64_t nrows, const int32_t* rp, int seg, SfPass* P) {
    P->items.clear(); P->frow.clear(); P->fptr.assign(1, 0); P->nparts = 0;
    auto len = [&](int64_t r) { return rp[r + 1] - rp[r]; };
    int64_t r = 0;
    while (r < nrows) {
        const int l0 = len(r);
        if (l0 > seg) {
            for (int e = rp[r]; e < rp[r + 1]; e += seg) P->items.push_back(SfItem{(int32_t)r, e, std::min(seg, rp[r + 1] - e), (int32_t)P->nparts++});
            P->frow.push_back((int32_t)r); P->fptr.push_back((int32_t)P->nparts);
            ++r;
            continue;
        }
        int g = sf_lanes(l0), cnt = 1;
        while (r + cnt < nrows && len(r + cnt) <= seg) {
            const int g2 = std::max(g, sf_lanes(len(r + cnt)));
            if ((cnt + 1) * g2 > 64) break;
            g = g2; ++cnt;
        }
        P->items.push_back(SfItem{(int32_t)r, cnt, -g, -1});
        r += cnt;
    }
}

int lanes_per_row(int64_t nnz, int64_t rows) {
    const double avg = rows > 0 ? (double)nnz / (double)rows : 1.0;
    int l = 1;
    while (l < 64 && 2 * l <= avg) l <<= 1;
    return l;
}

}  // namespace fos
