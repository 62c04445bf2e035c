// sptrsv_shape.cpp -- everything the triangular solve decides before a launch,
// as plain host arithmetic: the solve shape (executor, pass width, lanes per
// row, scope, threads, grid, back-off) and the level analysis with its
// narrow / wide run schedule.  No GPU, no handle, no process state, so the same
// arguments always give the same answer (sblas_trsv_shape_host and
// sblas_trsv_levels_host let CPU code call it).
#include <algorithm>

#include "../../include/sblas.h"
#include "sptrsv_shape.hpp"

namespace sblas {

// Right-hand sides per lane for pass width c.  Measured (r03_trsm_v3, ms;
// config-5 stand-in natural order / 27-point 100^3 stencil level order):
//   rhs   V=1          V=2          V=4          V=8
//    4    4.22 / 3.01  3.21 / 3.50  4.95 / 8.19  4.95 / 8.19
//    8    8.21 / 3.14  4.29 / 3.30  4.61 / 5.68  8.29 / 19.2
//   16   16.2  / 3.81  8.25 / 3.51  6.48 / 5.10  7.58 / 13.2
//   32   32.2  / 6.32  16.3 / 3.85  10.2 / 5.01  10.2 / 8.54
//   64   64.3  / 11.8  32.6 / 6.38  17.2 / 4.94  16.0 / 7.94
// Natural order is bound by the ticket counter (~85 M claims/s, one claim
// per 64 / RP rows) up to V = 4: wider lanes, fewer claims.  In level order a
// wave's rows are independent rows of one level and longer per-lane rows
// lengthen every level.
static int trsm_cols_per_lane(int c, bool level)
{
    if (level) return c <= 8 ? 1 : c <= 32 ? 2 : 4;
    return c <= 8 ? 2 : c <= 32 ? 4 : 8;
}

int trsv_shape(int algo, int opt, int rhs, bool mgpu, int blocks, int blocks_on_device, int ncu, TrsvShape *out)
{
    if (!out || algo < 0 || algo > 3 || rhs <= 0 || ncu <= 0 || blocks <= 0 || blocks_on_device <= 0 ||
        blocks_on_device > blocks)
        return SBLAS_ERR_INVALID;
    // the multi-device blocks run the natural-order pull executor only; one
    // handle is one block
    if (mgpu ? algo != 1 : blocks != 1) return SBLAS_ERR_INVALID;
    TrsvShape S{};
    if (algo == 2) {  // level-set: rows of a level side by side, no tickets
        if (rhs != 1) return SBLAS_ERR_INVALID;
        S.executor = kTrsvLevelSet;
        S.level_order = 1;
        S.threads = kLevelWG;
        // a wide run: one 1024-thread workgroup per CU, all resident (the grid
        // barrier's premise); a narrow run is one such workgroup
        S.grid = std::max(1, std::min(ncu, kLevelMaxWG));
        *out = S;
        return SBLAS_OK;
    }
    if (algo == 0) {  // push: one wave per column
        if (opt < (rhs == 1 ? 0 : 1) || opt > 3) return SBLAS_ERR_INVALID;
        S.executor = kTrsvPush;
        S.rows_per_claim = 1;
        S.threads = 256;
        S.grid = ncu;
        *out = S;
        return SBLAS_OK;
    }
    const bool level = algo == 3;
    S.executor = kTrsvPull;
    S.level_order = level;
    S.c = 1;
    while (S.c < rhs && S.c < 64) S.c *= 2;
    S.v = std::min(trsm_cols_per_lane(S.c, level), S.c);
    S.rp = S.c / S.v;
    S.passes = (rhs + S.c - 1) / S.c;
    S.rows_per_claim = 64 / S.rp;
    // Poll back-off: natural order one s_sleep(1) per poll; level order the
    // adaptive back-off up to 64 units (-6: 27-point 100^3 2.25 -> 2.03 ms,
    // 7-point 0.97 -> 0.88 ms; -8 and deeper lose; profiles/r03/sptrsv_sleep/)
    S.slp = level ? -6 : 1;
    // Grid: one workgroup per CU.  More spinning waves is slower: every
    // polling lane costs an L2 request the producers need (config 5, pull:
    // 1/CU 2.44 ms, 2/CU 2.99 ms, 4/CU 4.92 ms at 256 threads; 8/CU starves
    // the chain).
    if (mgpu) {
        // Co-resident blocks split the device's workgroup budget.  Four
        // blocks sharing one GPU ran 4.7 ms at 4 waves per CU and 6.2 at 2
        // (each block then has a quarter of the grid), and one block per GPU
        // is unmeasured, so the rhs = 1 kernel keeps 256 threads here, unlike
        // the single handle's 128 / 64.  It also polls at system scope even
        // as a single block, while the SpTRSM takes system scope only when
        // there are peers to publish to; and the SpTRSM's x 2 / x 4 grid
        // multiplier below is not applied to blocks.  Kept as measured.
        S.sys = rhs == 1 || blocks > 1;
        S.threads = 256;
        S.grid = std::max(1, ncu / blocks_on_device);
    } else if (rhs == 1) {
        // Threads per workgroup: the waves spinning on a CU.  Every pending
        // lane polls, and the polls share the memory path with the producers'
        // stores and loads, so fewer waves shorten each dependency hop -- as
        // long as enough rows are in flight to cover a level.  Config-5
        // stand-in (natural order, 985 levels): 1 / 2 / 3 / 4 waves per CU
        // 2.44 / 2.12 / 2.24 / 2.45 ms; level order (a ticket holds 64 rows
        // of one level): 27-point 100^3 1.79 / 1.92 / 1.99 / 2.03 ms, 7-point
        // 0.81 / 0.85 / 0.87 / 0.89 ms (profiles/r05/trsv_waves/).
        S.threads = level ? 64 : 128;
        S.grid = ncu;
    } else {
        // Workgroups per CU: natural order at rhs >= 16 gains from more rows
        // in flight (config 5: rhs 16 / 32 / 64 at 1 -> 2 -> 4 per CU: 6.50 /
        // 10.2 / 16.1 -> 4.63 / 8.55 / 10.4 -> 4.86 / 8.53 / 9.26 ms); level
        // order loses (27-point stencil rhs 64: 4.93 / 5.12 / 5.32 ms;
        // profiles/r03/sptrsm/trsm_grid2/).
        S.threads = 256;
        S.grid = ncu * (level || rhs < 16 ? 1 : rhs <= 32 ? 2 : 4);
    }
    *out = S;
    return SBLAS_OK;
}

void trsv_shape_info(const TrsvShape &S, long long *info)
{
    const int f[kTrsvShapeFields] = {S.executor, S.level_order, S.c,       S.rp,   S.v,  S.passes,
                                     S.rows_per_claim, S.sys,   S.threads, S.grid, S.slp};
    std::copy(f, f + kTrsvShapeFields, info);
}

void host_levels(int n, int substitution, const int *cp, const int *ri, std::vector<int> &lev, int &nl)
{
    lev.assign((size_t)n, 0);
    nl = 0;
    for (int k = 0; k < n; ++k) {
        const int i = substitution ? n - 1 - k : k;
        const int li = lev[(size_t)i];
        nl = std::max(nl, li + 1);
        for (int j = cp[i]; j < cp[i + 1]; ++j)
            if (ri[j] != i) lev[(size_t)ri[j]] = std::max(lev[(size_t)ri[j]], li + 1);
    }
}

std::vector<TrsvRun> level_schedule(const std::vector<int> &lptr)
{
    std::vector<TrsvRun> runs;
    const int nl = (int)lptr.size() - 1;
    auto wide = [&](int l) { return lptr[(size_t)l + 1] - lptr[(size_t)l] > kLevelNarrow; };
    for (int l = 0; l < nl;) {
        const bool w = wide(l);
        int e = l;
        while (e < nl && wide(e) == w) ++e;
        runs.push_back({l, e, w});
        l = e;
    }
    return runs;
}

}  // namespace sblas

extern "C" {

int sblas_trsv_shape_host(int algo, int opt, int rhs, int mgpu, int blocks, int blocks_on_device, int ncu,
                          long long *info)
{
    if (!info || (mgpu != 0 && mgpu != 1)) return SBLAS_ERR_INVALID;
    sblas::TrsvShape S;
    const int st = sblas::trsv_shape(algo, opt, rhs, mgpu != 0, blocks, blocks_on_device, ncu, &S);
    if (st == SBLAS_OK) sblas::trsv_shape_info(S, info);
    return st;
}

int sblas_trsv_levels_host(int n, const int *colptr, const int *rowidx, int substitution, long long *info)
{
    if (n < 0 || !colptr || !info || (substitution != 0 && substitution != 1) || colptr[0] != 0)
        return SBLAS_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (colptr[i + 1] < colptr[i]) return SBLAS_ERR_INVALID;
    if (colptr[n] && !rowidx) return SBLAS_ERR_INVALID;
    for (int j = 0; j < colptr[n]; ++j)
        if (rowidx[j] < 0 || rowidx[j] >= n) return SBLAS_ERR_INVALID;
    std::vector<int> lev;
    int nl = 0;
    sblas::host_levels(n, substitution, colptr, rowidx, lev, nl);
    std::vector<int> lptr((size_t)nl + 1, 0);
    for (int i = 0; i < n; ++i) lptr[(size_t)lev[(size_t)i] + 1]++;
    int widest = 0;
    for (int l = 0; l < nl; ++l) {
        widest = std::max(widest, lptr[(size_t)l + 1]);
        lptr[(size_t)l + 1] += lptr[(size_t)l];
    }
    info[0] = nl;
    info[1] = widest;
    info[2] = info[3] = 0;
    for (const auto &r : sblas::level_schedule(lptr)) info[r.wide ? 3 : 2]++;
    return SBLAS_OK;
}

}  // extern "C"
