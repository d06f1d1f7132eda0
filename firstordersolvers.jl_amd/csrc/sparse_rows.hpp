// Host only (no HIP header): the intake of a caller's 1-based CSC matrix (Julia SparseMatrixCSC{Float64,Int64}) for the sparse sets of the Feasibility form --
// csc_check validates under the caller's rules, csc_to_csr_pair leaves A and A' as two CSR matrices -- and the plans of their row passes.
//   caller (`what` in the messages)                          empty      ascending   bound   noun
//   IndAffine (sparse)                 affine_sparse.hip     refused    no          both    "A"            CG sums a duplicated entry like any other
//   IndAffine (sparse, factored)       ..._factored.hip      refused    yes         both    "A"            sf_gram_kernel adds a column's entries side by side
//   LeastSquares (sparse, factored)    ..._factored.hip      refused    yes         both    "A"
//   LeastSquares (sparse, normal)      nspace.hip            accepted   yes         rows    "A"            sf_gram_kernel again
//   Quadratic (cg), LeastSquares (cg)  nspace_cg.hip         accepted   yes         both    "the matrix"   the mirror pass of Q needs sorted columns
// The first fault is the one reported, in this order: arguments, bound, colptr[0], colptr monotone (every column), stored entries, then entry by entry: row
// index, ascending, finite.  What a caller tests itself (its vector, zero rows, a diagonal) comes after the matrix.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "foship.h"

namespace fos {

void set_error(const char* fmt, ...);
#define FOS_TRY(expr)                    \
    do {                                 \
        int _r = (expr);                 \
        if (_r != FOS_OK) return _r;     \
    } while (0)

struct HostCsr {                                  // rp.size() - 1 rows
    std::vector<int32_t> rp, ci;
    std::vector<double> va;
    int longest() const { int l = 0; for (size_t i = 0; i + 1 < rp.size(); ++i) l = std::max(l, rp[i + 1] - rp[i]); return l; }      // entries of the longest row
};

enum CscBound : int { CSC_BOUND_ROWS = 0, CSC_BOUND_BOTH = 1 };
struct CscRules {
    bool refuse_empty;                            // nnz == 0 is FOS_EINVAL ("... stored entries (1 .. 2e9 supported)")
    bool ascending;                               // the row indices of a column must be strictly ascending (no duplicates)
    CscBound bound;                               // more than 2e9 rows (rows and columns) is FOS_EUNSUPPORTED; the message names what is bounded
    const char* noun;                             // "<noun> has non-finite entries"
};
inline bool csc_finite(double v) { return v == v && (v < 0.0 ? -v : v) <= 1e300; }
// FOS_OK, or the code of the first fault with "<what>: ..." as the message.  After FOS_OK every index is in range and colptr[cols] - 1 <= 2e9.
int csc_check(const char* what, int64_t rows, int64_t cols, const int64_t* colptr, const int64_t* rowval, const double* nzval, const CscRules& rules);
// checked CSC arrays -> At = the arrays themselves, 0-based (cols x rows), and A (rows x cols, columns ascending within a row: a counting pass).
// row_scale != nullptr: every value is multiplied by row_scale[its row].
void csc_to_csr_pair(int64_t rows, int64_t cols, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* row_scale, HostCsr* A, HostCsr* At);

// a work item of a segmented sparse pass (16 bytes, read wave-uniformly), one wavefront each:
//   segment: a = row, b = first entry, c = entries (> 0), d = slot of part[] (-1: the row's only segment, never built: such rows are packed)
//   packet:  a = first row, b = rows (<= 64 / g), c = -g (lanes per row, a power of two), d unused
struct SfItem { int32_t a, b, c, d; };
struct SfPass {
    std::vector<SfItem> items;
    std::vector<int32_t> frow, fptr;              // cut rows and their slots of part[]: fptr[k] .. fptr[k + 1] - 1, in segment order
    int64_t nparts = 0;
};
constexpr int SF_SEG_DEFAULT = 2048;              // stored entries per segment (FOS_SF_SEG: a multiple of 64 from 64 up to this)
// the work items of one pass, from the row pointers and the segment length alone (the rule: affine_sparse_factored.hip's header)
void sf_plan_pass(int64_t nrows, const int32_t* rp, int seg, SfPass* P);
// one g for every row: the largest power of two (at most 64) not above the average row length
int lanes_per_row(int64_t nnz, int64_t rows);

}  // namespace fos
