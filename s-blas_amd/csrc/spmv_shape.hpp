// spmv_shape.hpp -- what the row-split, CSR5 and XCD-panel SpMV decide on the
// host before a plan is built (spmv_shape.cpp; plain host code, no GPU).
#pragma once

#include <cstdint>
#include <vector>

namespace sblas {

void set_error(const char *fmt, ...);

// Row-split (CSR-adaptive) tuning. One 256-thread workgroup per row block.
constexpr int kRsThreads = 256;
constexpr int kRsBlockNnz = 2048;   // LDS product stream capacity (16 KiB f64)
constexpr int kRsMaxRows = 1024;    // rows per stream block
constexpr int kRsLongChunk = 8192;  // nnz per workgroup for long rows

// Row block descriptor (16 B): stream block when a > row (a = end row);
// long-row chunk when a < 0 (chunk k = -a-1, b = partial slot or -1).
struct RowBlock {
    int row;
    int a;
    int b;
    int c;
};

// A multi-chunk long row (16 B; the device reads it as an int4).
struct LongRow {
    int row, slot, nchunks, panel;
};
static_assert(sizeof(LongRow) == 16, "the device layout of a long-row record");

// CSR5-style tiles: 64 lanes x kC5Sigma nnz per tile (one wave per tile).
constexpr int kC5Lanes = 64;
constexpr int kC5Sigma = 16;
constexpr int kC5Tile = kC5Lanes * kC5Sigma;

// What the caller read from the environment and the test hooks; -1 = unset.
struct SpmvOverrides {
    int auto_env = 0;        // SBLAS_AUTO's value (an algorithm 1..5; anything else is ignored)
    int rs_panel = -1;       // "rs_panel": 1 / 0 forces the row split onto / off XCD panels
    int csr5_panel = -1;     // "csr5_panel": the same for CSR5
    int panels = -1;         // "panels": the panel count (clamped to 1..64)
    int csr5_hostplan = -1;  // "csr5_hostplan": != 0 builds CSR5's descriptors on the host
};

struct SpmvShape {
    int algo;        // the algorithm that runs (AUTO resolved)
    int panels;      // the plan runs over XCD column panels
    int npanels;     // the panel count the column split is made with (0: xsort)
    long long W;     // columns per panel
    int c5_host;     // CSR5: the host descriptor builder
};
constexpr int kSpmvShapeFields = 5;

// Whether spmv_shape will look at the probe results for this request (AUTO
// always; the row split and CSR5 only past the panels' size gate, unless a
// hook forces the form): the plan build runs the column probe only then.
bool spmv_shape_wants_probe(int algo, int n, long long nnz, const SpmvOverrides &o);

// algo 0..5 as SBLAS_SPMV_*; adjacency, share (largest eighth) and scattered
// are the column probe's results (ignored when spmv_shape_wants_probe is
// false).  SBLAS_OK or SBLAS_ERR_INVALID.
int spmv_shape(int algo, int m, int n, long long nnz, double adjacency, double share, double scattered,
               const SpmvOverrides &o, SpmvShape *out);

// Greedy CSR-adaptive blocking of rows [0, m): whole rows up to kRsBlockNnz
// nnz / kRsMaxRows rows per block; longer rows in kRsLongChunk chunks (slot
// numbers continue from `nslots`).
void make_row_blocks(const int *rp, int m, std::vector<RowBlock> &blocks, std::vector<LongRow> &longs, int &nslots);
// adds to c: blocks, stream blocks, single-chunk long rows, multi-chunk long
// rows, partial slots; c[5] = the most rows in one block
constexpr int kRowBlockCounts = 6;
void count_row_blocks(const std::vector<RowBlock> &blocks, long long *c);

// CSR5 tile descriptors of a host rowptr (the "csr5_hostplan" builder; the
// device builder in spmv.hip fills the same arrays).
struct Csr5Host {
    long long ntiles = 0;
    std::vector<uint32_t> flags;   // [ntiles*64] per-lane row-start bits
    std::vector<int> tile_row;     // [ntiles+1] row of the tile's first element; bit31: tile has empty rows
    std::vector<int> seg_off;      // [ntiles+1] offsets into seg_row
    std::vector<int> seg_row;      // rows starting in the tiles that have empty rows
    std::vector<int> empty_rows;
};
void csr5_host_plan(const int *rp, int m, Csr5Host &out);
// the tiles of that plan with bit31 set, from rowptr alone (one walk over the rows)
long long csr5_gap_tiles(const int *rp, int m);
// head_run[t] as k_c5_headruns computes it
void csr5_head_runs(const Csr5Host &H, std::vector<int> &head_run);

}  // namespace sblas
