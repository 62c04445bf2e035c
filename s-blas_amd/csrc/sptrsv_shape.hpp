// sptrsv_shape.hpp -- what the triangular solve decides on the host before a
// launch (sptrsv_shape.cpp; plain host code, no GPU).
#pragma once

#include <vector>

namespace sblas {

constexpr int kLevelWG = 1024;              // threads of a level-set workgroup
constexpr int kLevelNarrow = 2 * kLevelWG;  // a level with <= this many rows is narrow
constexpr int kLevelMaxWG = 1024;           // grid-barrier workgroups (arrival words)

enum TrsvExecutor { kTrsvPush = 0, kTrsvPull = 1, kTrsvLevelSet = 2 };

// The shape of one solve.  c .. slp describe the pull executor (0 for the
// others, whose kernels have no such parameters).
struct TrsvShape {
    int executor;        // TrsvExecutor
    int level_order;     // tickets / rows in level order
    int c;               // pass width: rhs rounded up to a power of two, <= 64
    int rp, v;           // lanes per row, right-hand sides per lane (rp * v == c)
    int passes;          // ceil(rhs / c)
    int rows_per_claim;  // 64 / rp rows on one ticket claim (push: one column)
    int sys;             // x polled and published at system scope
    int threads, grid;   // threads per workgroup, workgroups (level-set: of a wide run)
    int slp;             // poll back-off (trsv_backoff)
};
constexpr int kTrsvShapeFields = 11;

// algo 0 push, 1 pull, 2 level-set, 3 pull in level order (4 is resolved by
// the caller's probe).  opt: the push lane mapping of the SpTRSM (1..3), 0 =
// the rhs = 1 push kernel.  SBLAS_OK or SBLAS_ERR_INVALID.
int trsv_shape(int algo, int opt, int rhs, bool mgpu, int blocks, int blocks_on_device, int ncu, TrsvShape *out);
void trsv_shape_info(const TrsvShape &S, long long *info);  // the 11 fields in order

// level(i) = 1 + max level of i's dependencies over a host CSC (findlevel.h:71-147)
void host_levels(int n, int substitution, const int *colptr, const int *rowidx, std::vector<int> &lev, int &nl);

// maximal runs of narrow / of wide levels, levels [l0, l1) each
struct TrsvRun {
    int l0, l1;
    bool wide;
};
std::vector<TrsvRun> level_schedule(const std::vector<int> &lptr);

}  // namespace sblas
