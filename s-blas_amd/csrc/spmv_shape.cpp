// spmv_shape.cpp -- what the row-split, CSR5 and XCD-panel SpMV decide before
// a plan is built: which algorithm AUTO takes, whether a row-oriented kernel
// runs over XCD column panels and over how many, the row blocks of the row
// split, and CSR5's host-built tile descriptors.  Plain host arithmetic on the
// arguments: no GPU, no handle, no environment and no test hook (the caller
// passes those in), so the same arguments always give the same answer
// (sblas_spmv_shape_host, sblas_rowsplit_blocks_host and sblas_csr5_plan_host
// let CPU code call it).
#include <algorithm>
#include <climits>

#include "../../include/sblas.h"
#include "spmv_shape.hpp"

namespace sblas {

constexpr long long kAutoXsortMinNnz = 2000000;  // bench slices: xsort leads from ~2M nnz

// Whether a row-oriented kernel (row split, CSR5) should run over XCD column
// panels (~4 MiB of x each, P = 4 partials added after): x outgrows an XCD's
// L2, the rows' columns are scattered (the column probe: most sampled rows
// span > n/4 of the columns, spread over the eighths) and the matrix is large
// enough to amortise the partial-y pass (kPanelMinNnz).  Measured on the uniform
// config 2 and its rank slices (cold spans, profiles/r05/sweep/, c5P/; plain
// / 4 panels): CSR5 567 / 287 us at N = 1, 77 / 46 (heavy) and 80 / 60
// (light rows) on configs[2]'s N = 8 ranks (5M entries), 45 / 38 on a 2.5M
// cyclic slice, 29.6 / 30.4 on 1.2M; the row split alike (573 / 310, 76 / 47,
// 79 / 58, 42 / 32, 24 / 25).  So both take panels from 2M entries.
// (Rounds 1-4 set 8M / 4M thresholds and 2 panels on short rows on the
// correlated generator, profiles/r05/gen/, whose heavy rows shared x lines.)
// The test hooks "rs_panel" / "csr5_panel" = 1 / 0 force either form.
constexpr long long kPanelMinNnz = 2000000LL;
constexpr long long kC5WidePanelNnz = 32000000LL;  // CSR5: 2 MiB x panels from here

static bool panels_size_gate(int n, long long nnz) { return (long long)n * 8 > (8LL << 20) && nnz >= kPanelMinNnz; }

static bool xcd_panels_pay(int forced, int n, long long nnz, double share, double scattered)
{
    if (forced >= 0) return forced == 1;
    return panels_size_gate(n, nnz) && scattered >= 0.5 && share <= 0.25;
}

// ~4 MiB of x per panel (one XCD's L2), at most one panel per XCD (config 2:
// P = 4 beats 8, fewer partial-y bytes); the test hook "panels" overrides
static int default_panels(int n, int forced)
{
    int P = (int)std::min<long long>(8, std::max<long long>(1, ((long long)n * 8 + (4 << 20) - 1) >> 22));
    if (forced >= 0) P = std::max(1, std::min(64, forced));
    if (n < P) P = std::max(1, n);
    return P;
}

// AUTO: the column-sorted kernel wherever it applies at size and its column
// groups share the work: it leads on random columns (config 2: 0.51 of
// 8 TB/s vs 0.21 row split) and on banded / stencil matrices too (3-D
// 27-point stencil 0.84 vs 0.55, 7-point 0.71 vs 0.58), but
// columns crowded into one eighth (the reference generator's prefix
// columns) leave one XCD all of it: the row split there (0.68), as for
// any matrix whose rows read neighbouring x lines; the XCD-panel row
// split below 2M nonzeros.
static int pick_algo(int n, long long nnz, double adj, double share, int auto_env)
{
    if (auto_env >= SBLAS_SPMV_ROWSPLIT && auto_env <= SBLAS_SPMV_XSORT) return auto_env;
    const bool spread = share <= 0.25;  // no eighth of the columns holds > 2x its share
    if (nnz >= kAutoXsortMinNnz && (long long)n * 8 <= (120LL << 20) && spread) return SBLAS_SPMV_XSORT;
    if (adj >= 0.5 || !spread) return SBLAS_SPMV_ROWSPLIT;
    return SBLAS_SPMV_PANEL;
}

bool spmv_shape_wants_probe(int algo, int n, long long nnz, const SpmvOverrides &o)
{
    switch (algo) {
    case SBLAS_SPMV_AUTO: return true;
    case SBLAS_SPMV_ROWSPLIT: return o.rs_panel < 0 && panels_size_gate(n, nnz);
    case SBLAS_SPMV_CSR5:
    case SBLAS_SPMV_CSR5_ALT: return o.csr5_panel < 0 && panels_size_gate(n, nnz);
    default: return false;
    }
}

int spmv_shape(int algo, int m, int n, long long nnz, double adjacency, double share, double scattered,
               const SpmvOverrides &o, SpmvShape *out)
{
    if (!out || algo < SBLAS_SPMV_AUTO || algo > SBLAS_SPMV_XSORT || m < 0 || n < 0 || nnz < 0)
        return SBLAS_ERR_INVALID;
    if (algo == SBLAS_SPMV_AUTO) algo = pick_algo(n, nnz, adjacency, share, o.auto_env);
    SpmvShape S{algo, 0, 0, 0, 0};
    switch (algo) {
    case SBLAS_SPMV_ROWSPLIT:
        // the same row blocks per XCD column panel on large scattered matrices
        // (the panel plan, algo 4's layout)
        S.npanels = default_panels(n, o.panels);
        S.panels = xcd_panels_pay(o.rs_panel, n, nnz, share, scattered);
        break;
    case SBLAS_SPMV_CSR5:
    case SBLAS_SPMV_CSR5_ALT:
        // P = default_panels (4 on config 2) whatever the row length: on the
        // uniform config 2 4 panels beat 2 and 8 on short rows (N = 8 light rank
        // 60 vs 68 / 67 us) and are within 4-8% of 8 on 96-entry rows
        // (profiles/r05/c5P/).  From 32M entries the panels halve to
        // ~2 MiB of x (P = 8, one per XCD): the x re-fetch the panel's entry
        // stream forces through a 4 MiB L2 grows with the entries, the partial
        // y (16 B per row and panel) with the rows -- config 2 at N = 1 (39.75M
        // entries, 2M rows): 284.6-285.1 us at P = 4, 273.7-274.6 at P = 8
        // (profiles/r06/panels/); the N = 8 light slice keeps P = 4.
        S.npanels = default_panels(n, o.panels);
        if (nnz >= kC5WidePanelNnz && o.panels < 0) S.npanels = std::min(8, 2 * S.npanels);
        S.c5_host = o.csr5_hostplan > 0;
        S.panels = xcd_panels_pay(o.csr5_panel, n, nnz, share, scattered) && S.npanels >= 2 && !S.c5_host;
        break;
    case SBLAS_SPMV_PANEL:
        S.npanels = default_panels(n, o.panels);
        S.panels = 1;
        break;
    default: break;  // xsort: its own planner (xsort_plan.cpp)
    }
    if (S.npanels) S.W = ((long long)n + S.npanels - 1) / S.npanels;
    *out = S;
    return SBLAS_OK;
}

void make_row_blocks(const int *rp, int m, std::vector<RowBlock> &blocks, std::vector<LongRow> &longs, int &nslots)
{
    int r = 0;
    while (r < m) {
        const int len = rp[r + 1] - rp[r];
        if (len > kRsBlockNnz) {
            const int nch = (len + kRsLongChunk - 1) / kRsLongChunk;
            if (nch == 1) {
                blocks.push_back({r, -1, -1, 0});
            } else {
                longs.push_back({r, nslots, nch, 0});
                for (int k = 0; k < nch; ++k) blocks.push_back({r, -1 - k, nslots + k, 0});
                nslots += nch;
            }
            ++r;
            continue;
        }
        const int start = r;
        int nz = 0;
        while (r < m && r - start < kRsMaxRows) {
            const int l = rp[r + 1] - rp[r];
            if (l > kRsBlockNnz || nz + l > kRsBlockNnz) break;
            nz += l;
            ++r;
        }
        blocks.push_back({start, r, 0, 0});
    }
}

void count_row_blocks(const std::vector<RowBlock> &blocks, long long *c)
{
    for (const RowBlock &b : blocks) {
        ++c[0];
        if (b.a >= 0) {
            ++c[1];
            c[5] = std::max<long long>(c[5], b.a - b.row);
        } else {
            if (b.b < 0) ++c[2];
            else ++c[4];
            if (b.b >= 0 && b.a == -1) ++c[3];
            c[5] = std::max<long long>(c[5], 1);
        }
    }
}

void csr5_host_plan(const int *rp, int m, Csr5Host &H)
{
    const long long nnz = m > 0 ? rp[m] : 0;
    const long long nt = (nnz + kC5Tile - 1) / kC5Tile;
    H = Csr5Host{};
    H.ntiles = nt;
    H.flags.assign((size_t)nt * 64, 0u);
    for (int r = 0; r < m; ++r) {
        const int a = rp[r], b = rp[r + 1];
        if (a == b) {
            H.empty_rows.push_back(r);
            continue;
        }
        const long long t = a / kC5Tile;
        const int w = (int)(a - t * kC5Tile);
        H.flags[(size_t)t * 64 + w / kC5Sigma] |= 1u << (w % kC5Sigma);
    }
    // tile_row: row holding the tile's first element (last r with rp[r] <= e)
    H.tile_row.assign((size_t)nt + 1, m);
    H.seg_off.assign((size_t)nt + 1, 0);
    int r = 0;
    for (long long t = 0; t < nt; ++t) {
        const long long e = t * kC5Tile;
        while (r < m && rp[r + 1] <= e) ++r;
        const int rfirst = r;
        // last row of tile
        const long long elast = std::min(nnz, e + kC5Tile) - 1;
        int rl = r;
        while (rl < m && rp[rl + 1] <= elast) ++rl;
        int nstarts = 0;
        for (int l = 0; l < 64; ++l) nstarts += __builtin_popcount(H.flags[(size_t)t * 64 + l]);
        const bool start0 = H.flags[(size_t)t * 64] & 1u;
        const int expected = rl - rfirst + (start0 ? 1 : 0);
        H.tile_row[t] = rfirst;
        H.seg_off[t] = (int)H.seg_row.size();
        if (nstarts != expected) {
            H.tile_row[t] = rfirst | (int)0x80000000u;
            for (int q = (start0 ? rfirst : rfirst + 1); q <= rl; ++q)
                if (rp[q + 1] > rp[q] && rp[q] >= e && rp[q] <= elast) H.seg_row.push_back(q);
        }
    }
    H.seg_off[nt] = (int)H.seg_row.size();
}

// A tile's first and last rows hold entries, and every row between them
// starts in the tile: the row starts fall short of that count exactly when
// one of the rows between them is empty.
long long csr5_gap_tiles(const int *rp, int m)
{
    const long long nnz = m > 0 ? rp[m] : 0;
    const long long nt = (nnz + kC5Tile - 1) / kC5Tile;
    long long gaps = 0;
    int r = 0;
    for (long long t = 0; t < nt; ++t) {
        const long long e = t * kC5Tile;
        while (r < m && rp[r + 1] <= e) ++r;
        const long long elast = std::min(nnz, e + kC5Tile) - 1;
        bool hole = false;
        for (int rl = r; rl < m && rp[rl + 1] <= elast; ++rl) hole = hole || rp[rl + 2] == rp[rl + 1];
        gaps += hole ? 1 : 0;
    }
    return gaps;
}

void csr5_head_runs(const Csr5Host &H, std::vector<int> &head_run)
{
    const long long nt = H.ntiles;
    head_run.assign((size_t)nt, 0);
    auto has_head = [&](long long u) { return (H.flags[(size_t)u * 64] & 1u) == 0u; };
    auto row = [&](long long u) { return H.tile_row[(size_t)u] & 0x7fffffff; };
    for (long long t = 0; t < nt; ++t) {
        if (!has_head(t) || (t > 0 && row(t - 1) == row(t) && has_head(t - 1))) continue;
        int L = 0;
        for (long long u = t; u < nt && row(u) == row(t) && has_head(u); ++u) ++L;
        head_run[(size_t)t] = L;
    }
}

// rowptr of the C API (long long) as the plans' 32-bit offsets
static int host_rowptr(const char *who, int m, const long long *rowptr, std::vector<int> &rp)
{
    rp.resize((size_t)m + 1);
    for (int r = 0; r <= m; ++r) {
        if (rowptr[r] < 0 || rowptr[r] > INT_MAX || (r ? rowptr[r] < rowptr[r - 1] : rowptr[0] != 0)) {
            set_error("%s: rowptr[%d] is not an ascending 32-bit offset from 0", who, r);
            return SBLAS_ERR_INVALID;
        }
        rp[(size_t)r] = (int)rowptr[r];
    }
    return SBLAS_OK;
}

}  // namespace sblas

using namespace sblas;

extern "C" int sblas_spmv_shape_host(int algo, int m, int n, long long nnz, double adjacency, double share,
                                     double scattered, int auto_env, int rs_panel, int csr5_panel, int panels,
                                     int csr5_hostplan, long long *info)
{
    if (!info) return SBLAS_ERR_INVALID;
    SpmvOverrides o;
    o.auto_env = auto_env;
    o.rs_panel = rs_panel;
    o.csr5_panel = csr5_panel;
    o.panels = panels;
    o.csr5_hostplan = csr5_hostplan;
    SpmvShape S;
    const int st = spmv_shape(algo, m, n, nnz, adjacency, share, scattered, o, &S);
    if (st != SBLAS_OK) return st;
    const long long v[kSpmvShapeFields + 1] = {S.algo, S.panels, S.npanels, S.W, S.c5_host,
                                               spmv_shape_wants_probe(algo, n, nnz, o) ? 1 : 0};
    for (int i = 0; i <= kSpmvShapeFields; ++i) info[i] = v[i];
    return SBLAS_OK;
}

extern "C" int sblas_rowsplit_blocks_host(int m, const long long *rowptr, long long *info, int *blocks,
                                          long long blocks_cap)
{
    if (!rowptr || !info || m < 0) return SBLAS_ERR_INVALID;
    std::vector<int> rp;
    const int st = host_rowptr("sblas_rowsplit_blocks_host", m, rowptr, rp);
    if (st != SBLAS_OK) return st;
    std::vector<RowBlock> b;
    std::vector<LongRow> longs;
    int nslots = 0;
    make_row_blocks(rp.data(), m, b, longs, nslots);
    for (int i = 0; i < kRowBlockCounts; ++i) info[i] = 0;
    count_row_blocks(b, info);
    if (!blocks) return SBLAS_OK;
    if (blocks_cap < (long long)b.size()) {
        set_error("sblas_rowsplit_blocks_host: room for %lld blocks, %lld needed", blocks_cap, (long long)b.size());
        return SBLAS_ERR_INVALID;
    }
    for (const RowBlock &k : b) {
        *blocks++ = k.row;
        *blocks++ = k.a;
        *blocks++ = k.b;
    }
    return SBLAS_OK;
}

extern "C" int sblas_csr5_plan_host(int m, const long long *rowptr, long long *info, unsigned *flags, int *tile_row,
                                    int *seg_off, int *seg_row, int *empty_rows, int *head_run)
{
    if (!rowptr || !info || m < 0) return SBLAS_ERR_INVALID;
    std::vector<int> rp;
    const int st = host_rowptr("sblas_csr5_plan_host", m, rowptr, rp);
    if (st != SBLAS_OK) return st;
    Csr5Host H;
    csr5_host_plan(rp.data(), m, H);
    std::vector<int> hr;
    csr5_head_runs(H, hr);
    long long gaps = 0, runs = 0, longest = 0;
    for (long long t = 0; t < H.ntiles; ++t) {
        gaps += H.tile_row[(size_t)t] < 0 ? 1 : 0;
        runs += hr[(size_t)t] > 0 ? 1 : 0;
        longest = std::max<long long>(longest, hr[(size_t)t]);
    }
    const long long v[6] = {H.ntiles, gaps, (long long)H.seg_row.size(), (long long)H.empty_rows.size(), runs,
                            longest};
    for (int i = 0; i < 6; ++i) info[i] = v[i];
    if (flags) std::copy(H.flags.begin(), H.flags.end(), flags);
    if (tile_row) std::copy(H.tile_row.begin(), H.tile_row.end(), tile_row);
    if (seg_off) std::copy(H.seg_off.begin(), H.seg_off.end(), seg_off);
    if (seg_row) std::copy(H.seg_row.begin(), H.seg_row.end(), seg_row);
    if (empty_rows) std::copy(H.empty_rows.begin(), H.empty_rows.end(), empty_rows);
    if (head_run) std::copy(hr.begin(), hr.end(), head_run);
    return SBLAS_OK;
}
