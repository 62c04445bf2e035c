// xsort.hpp -- what the three parts of the xsort SpMV (algo 5) share: the
// planner (xsort_plan.cpp: plain host code, no GPU), the layout builders
// (xsort_layout.hip) and the kernel with the plan build (xsort.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace sblas {

void set_error(const char *fmt, ...);

// LDS row accumulators per workgroup: 16384 = 128 KiB (default); an
// experiment build may raise it towards the 160 KiB of a gfx950 CU
// (SBLAS_XS_LDS_ROWS=19456: 152 KiB of rows + ~6 KiB of bookkeeping)
#ifndef SBLAS_XS_LDS_ROWS
#define SBLAS_XS_LDS_ROWS 16384
#endif
constexpr int kXsRows = SBLAS_XS_LDS_ROWS;
static_assert(kXsRows % 512 == 0, "two teams of whole 256-row blocks");
constexpr int kXsHalfRows = kXsRows / 2;
constexpr int kXsRowBits = 14;     // packed key: local row in the low 14 bits
constexpr int kXsColBits = 18;     //             group-local column above
constexpr int kXsChunk = 256;      // entries per chunk: one wave, 4 per lane
constexpr uint32_t kXsPad = ((1u << kXsColBits) - 1) << kXsRowBits;  // column all ones, row 0
static_assert(kXsRowBits + kXsColBits == 32, "packed key is 32 bits");
static_assert(kXsHalfRows <= (1 << kXsRowBits), "a team's local row must fit the key");
// a range's rows: a team's half, or (solo items) the whole workgroup's
// accumulators up to what the key's row field addresses
constexpr int kXsItemRows = kXsRows < (1 << kXsRowBits) ? kXsRows : (1 << kXsRowBits);
constexpr size_t kXsChunkBytes = (size_t)kXsChunk * (sizeof(uint32_t) + sizeof(double));
constexpr long long kXsAllWideMaxNnz = 6000000;  // all ranges wide up to this many entries (planner)

struct XsRange {
    int row0;
    int nrows;
    int wide;
    int widx;         // wide: index among the wide ranges, else -1
    long long pbase;  // wide: offset of the range's [8][nrows] partials
};

// The planner's overrides (test options "xs_cap", "xs_allwide", "xs_solo").
struct XsPlanOptions {
    bool has_cap = false;  // cap fixes the sub-item cost instead of the search
    double cap = 0.0;
    int allwide = -1;      // 0 / 1, -1 = the planner decides
    int solo = -1;
};

// What the planner decides for a matrix: a function of rowptr, n and the
// resident workgroups alone (xs_plan_host).
struct XsHostPlan {
    int q = 0, G = 0, Wg = 0;
    bool solo = false;
    int rows_cap = 0, nrows_cap = 0;  // rows of a wide / a narrow range at most
    std::vector<XsRange> ranges;      // widx / pbase filled in
    std::vector<int> wide;            // indices of the wide ranges, in order
    long long partial_len = 0;        // sum of 8 * nrows over the wide ranges
    // items (sub, sub) per XCD queue: sub = range << 8 | k, k = 0 narrow,
    // k = 1..8 the wide sub-item of XCD k - 1; -1 = none
    std::vector<std::pair<int, int>> queue[8];
    int qlen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int qstat[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // items per queue taken statically
    int qstride = 0, nitems = 0, grid = 0, dynamic = 0;
};

// m rows, n columns, nnz = rowptr[m] entries; resident = workgroups the
// device holds at once (>= 1).  SBLAS_OK or SBLAS_ERR_UNSUPPORTED (set_error).
int xs_plan_host(int m, int n, long long nnz, const int *rowptr, int resident, const XsPlanOptions &opt,
                 XsHostPlan &out);

}  // namespace sblas
