// spmm.hip -- fp64 CSR x dense SpMM for gfx950.
//
// Replaces cusparseDcsrmm (spmm/src/dspmm_mgpu_baseline.cu:225-240):
// C(m x n, col-major, ldc) = alpha * A(m x k, CSR) * B(k x n) + beta * C.
//
// Layout: B is consumed ROW-major (row j of B = the n values A's column j
// multiplies), so each nonzero a_ij pulls one contiguous n*8-byte row of B
// (512 B at n = 64: one wave load).  A column-major B (the reference's
// host layout) is transposed once into a row-major panel owned by the
// handle (k_transpose_B, LDS-tiled 64x64).
//
// Kernels:
//  * row-wave: one wave per (row of A, 64-column slab of C).  The wave loads
//    64 (col, val) pairs of the row with one coalesced load each, then
//    broadcasts them lane-to-lane (__shfl) while every lane FMAs its column
//    of B; eight independent B-row loads are kept in flight.  Accumulation
//    order per C entry is the row's storage order (same as the oracle).
//  * MFMA B-panel tile: for a 16-row block whose column union U
//    is dense (nnz / (16|U|) >= fill threshold), A is stored as a dense
//    16 x |U| tile and C(16 x 64) += A_tile * B[U, :] runs as
//    v_mfma_f64_16x16x4f64 over 4-column k-chunks -- each B row is read once
//    per 16 rows instead of once per nonzero.  This is a real contraction
//    only when rows share columns (banded / FEM-block matrices); a random
//    matrix like rail4284 has no dense blocks and stays on the row-wave
//    kernel.
#include <algorithm>
#include <array>
#include <climits>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "sblas_internal.hpp"

namespace sblas {

template <bool kBeta>
__global__ __launch_bounds__(256) void k_spmm_rowwave(
    const int *__restrict__ rowptr, const int *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ B, long long ldb,
    int m, int n, int nslab, double alpha, double beta, double *__restrict__ C,
    long long ldc, const int *__restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)m * nslab) return;
    const int r = rows ? rows[w / nslab] : (int)(w / nslab);
    const int c = (int)(w % nslab) * 64 + lane;
    const bool live = c < n;
    const int cc = live ? c : 0;
    const int a0 = rowptr[r], a1 = rowptr[r + 1];
    double acc = 0.0;
    for (int base = a0; base < a1; base += 64) {
        const int cnt = min(64, a1 - base);
        const int my_j = lane < cnt ? col[base + lane] : 0;
        const double my_a = lane < cnt ? val[base + lane] : 0.0;
        int q = 0;
        for (; q + 8 <= cnt; q += 8) {
            double b[8], a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = __shfl(my_j, q + u, 64);
                a[u] = __shfl(my_a, q + u, 64);
                b[u] = B[(long long)j * ldb + cc];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += a[u] * b[u];
        }
        for (; q < cnt; ++q) {
            const int j = __shfl(my_j, q, 64);
            const double a = __shfl(my_a, q, 64);
            acc += a * B[(long long)j * ldb + cc];
        }
    }
    if (live) {
        double *o = C + (long long)c * ldc + r;
        *o = kBeta ? alpha * acc + beta * *o : alpha * acc;
    }
}

// Long rows (rail4284: ~2,600 nnz per row, only m = 4,284 rows): one
// WORKGROUP per (row, 64-column slab), the row's nonzeros split over its 4
// waves, 16 B-row gathers in flight per lane, partial sums combined in LDS.
// A wave-per-row kernel leaves each wave walking ~2,600 dependent B-row
// gathers 8 at a time -- latency-bound with only m waves in the grid.
template <bool kBeta>
__global__ __launch_bounds__(256) void k_spmm_rowsplitk(
    const int *__restrict__ rbeg, const int *__restrict__ rend, const int *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ B, long long ldb,
    int m, int n, int nslab, double alpha, double beta, double *__restrict__ C,
    long long ldc, const int *__restrict__ rows)
{
    __shared__ double part[3][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long blk = blockIdx.x;
    const int r = rows ? rows[blk / nslab] : (int)(blk / nslab);
    const int c = (int)(blk % nslab) * 64 + lane;
    const bool live = c < n;
    const int cc = live ? c : 0;
    const int a0 = rbeg[r], a1 = rend[r];
    const int len = a1 - a0;
    const int q0 = a0 + (int)((long long)len * wv / 4), q1 = a0 + (int)((long long)len * (wv + 1) / 4);
    double acc = 0.0, acc2 = 0.0;
    for (int base = q0; base < q1; base += 64) {
        const int cnt = min(64, q1 - base);
        const int my_j = lane < cnt ? col[base + lane] : 0;
        const double my_a = lane < cnt ? val[base + lane] : 0.0;
        int q = 0;
        for (; q + 16 <= cnt; q += 16) {
            double b[16], a[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = __shfl(my_j, q + u, 64);
                a[u] = __shfl(my_a, q + u, 64);
                b[u] = B[(long long)j * ldb + cc];
            }
#pragma unroll
            for (int u = 0; u < 16; u += 2) {
                acc += a[u] * b[u];
                acc2 += a[u + 1] * b[u + 1];
            }
        }
        for (; q < cnt; ++q) {
            const int j = __shfl(my_j, q, 64);
            const double a = __shfl(my_a, q, 64);
            acc += a * B[(long long)j * ldb + cc];
        }
    }
    acc += acc2;
    if (wv > 0) part[wv - 1][lane] = acc;
    __syncthreads();
    if (wv == 0 && live) {
        acc += part[0][lane] + part[1][lane] + part[2][lane];
        double *o = C + (long long)c * ldc + r;
        *o = kBeta ? alpha * acc + beta * *o : alpha * acc;
    }
}

typedef double v4d __attribute__((ext_vector_type(4)));

// One wave per (MFMA block, 64-column group of C): 4 accumulators of
// 16 x 16.  f64 MFMA lane maps (cdna_hip_programming.md §3): A[i=l&15][k=l>>4],
// B[k=l>>4][j=l&15], D col = l&15, row = (l>>4) + 4*reg.
template <bool kBeta>
__global__ __launch_bounds__(256) void k_spmm_mfma(
    const int *__restrict__ mblock, const int *__restrict__ mchunk, const int *__restrict__ ucol,
    const double *__restrict__ atile, int nmfma, const double *__restrict__ B, long long ldb,
    int m, int n, int ngrp, double alpha, double beta, double *__restrict__ C, long long ldc)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)nmfma * ngrp) return;
    const int q = (int)(w / ngrp), g = (int)(w % ngrp);
    const int r0 = mblock[q] * 16;
    const int kq = lane >> 4, jq = lane & 15;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    int cj[4];
    bool live[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        cj[t] = g * 64 + t * 16 + jq;
        live[t] = cj[t] < n;
        if (!live[t]) cj[t] = 0;
    }
    // kU chunks per step, every load of the step issued before its first MFMA
    // (the union-column -> B-row loads are a dependent pair per chunk)
    constexpr int kU = 2;
    const int c0 = mchunk[q], c1 = mchunk[q + 1];
    for (int c = c0; c < c1; c += kU) {  // wave-uniform
        double a[kU], b[kU][4];
        long long brow[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int cu = min(c + u, c1 - 1);
            a[u] = c + u < c1 ? atile[(long long)cu * 64 + lane] : 0.0;
            brow[u] = (long long)ucol[cu * 4 + kq] * ldb;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t) b[u][t] = live[t] ? B[brow[u] + cj[t]] : 0.0;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (c + u >= c1) break;  // wave-uniform: no MFMA for a padding step
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][t], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!live[t]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + kq + 4 * r;
            if (row < m) {
                double *o = C + (long long)cj[t] * ldc + row;
                *o = kBeta ? alpha * acc[t][r] + beta * *o : alpha * acc[t][r];
            }
        }
    }
}

// ---- column-sorted C-tile SpMM (few rows, tall B) -------------------------
// The row forms move one B row (n*8 B) from L2 to the CU per NONZERO: 5.8 GB
// per call on rail4284, at the L2/Infinity-Cache gather rate.  Here a
// workgroup owns a tile of C -- R rows x 16 columns, accumulated in LDS --
// and walks its entries sorted by column: the nonzeros of one column inside
// the tile's rows sit next to each other, so their 128-B B segment is
// fetched once (same address in one instruction, or an L1 hit in the next)
// and applied to all of them.  A's entries are read once per 16 C columns
// instead.  Per nonzero: 12 B of A per column group + one 128-B segment per
// (column, tile) instead of n*8 B; the products land in LDS with ds_add_f64.
// XCD k owns the column slabs s % 8 == k (its B rows stay in its L2); its
// slabs are split into ns sets, and each (set, row block, column group) is
// one workgroup writing an alpha-free partial, added in slot order after.
constexpr int kCtCols = 16;      // C columns per tile (one 128-B B segment)
constexpr int kCtPad = 17;       // LDS row stride in doubles (bank spread; col 16 = pad sink)
constexpr int kCtThreads = 1024;
constexpr int kCtMaxRows = 163840 / (kCtPad * 8);  // 1204: one tile per CU

// DPP row_newbcast:s (gfx90a+): every 16-lane row reads lane s of that row
template <int kS>
__device__ __forceinline__ unsigned dpp_rowbcast(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + kS, 0xf, 0xf, false);
}

// Step T's value for this lane: lanes 0-7 of each 16-lane DPP row (banks 0-1)
// take lane T of the row, lanes 8-15 (banks 2-3) lane 8 + T -- two bank-masked
// row_newbcast moves, no select.  Must run with every lane active (a
// broadcast from an inactive lane returns `old`), so no branch encloses it.
template <int kT>
__device__ __forceinline__ unsigned ct_bcast(unsigned v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)v, 0x150 + kT, 0xf, 0x3, false);
    return (unsigned)__builtin_amdgcn_update_dpp(lo, (int)v, 0x150 + 8 + kT, 0xf, 0xc, false);
}

// Inner loop: per 64 entries ONE coalesced key load and ONE value load; lane
// L = 16g + 8h + T holds entry 8T + 2g + h of the 64 (g = DPP row, h = half
// row), so step T's 8 entries (entry 8T + 2g + h for the lanes of half-row
// (g, h)) come from row broadcasts, no memory instruction.  An entry's 16 C
// columns are 8 lanes x 2 doubles: one 16-B B load per lane and two
// ds_add_f64.  kDirect: keys hold the global column (j << rbits | row);
// otherwise the XCD-local column of the slab layout.  kFast: B rows 16-B
// aligned, n % 16 == 0 and B < 4 GiB (32-bit byte offsets); else per-column
// guards and scalar loads.  Full 64-entry iterations run without checks;
// the one partial iteration per item routes dead lanes' +0.0 into the row's
// padding column.
// kSlots: the item's units are column-run SLOTS of up to two entries of one
// column (key2 = second row or ~0, val2 its value): one B segment feeds both,
// so ~41% fewer B bytes cross L1 -> lanes on rail4284 (runs average 2.7
// entries per tile); a single-entry slot's second adds go to the padding
// column.
template <bool kDirect, bool kFast, bool kSlots>
__global__ __launch_bounds__(kCtThreads) void k_spmm_ctile(
    const unsigned *__restrict__ key, const double *__restrict__ val,
    const unsigned *__restrict__ key2, const double *__restrict__ val2,
    const long long *__restrict__ off, int ns, int nrb, int R, int rbits, int wlog, int ncg,
    const double *__restrict__ B, long long ldb, int n, int m, double *__restrict__ part)
{
    extern __shared__ double tile[];  // [R][kCtPad]
    const int x = (int)(blockIdx.x & 7);
    int rest = (int)(blockIdx.x >> 3);
    const int cg = rest % ncg;
    rest /= ncg;
    const int rb = rest % nrb, ss = rest / nrb;
    const int slot = x * ns + ss;
    const int r0 = rb * R, nr = min(R, m - r0);
    for (int i = threadIdx.x; i < nr * kCtPad; i += kCtThreads) tile[i] = 0.0;
    __syncthreads();
    const long long e0 = off[(long long)slot * nrb + rb], e1 = off[(long long)slot * nrb + rb + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, h = (lane >> 3) & 1, q = lane & 7;
    const int myoff = 8 * (lane & 7) + 2 * g + h;
    const int mypos = 2 * g + h;  // this lane's entry within a step
    const int c0 = cg * kCtCols + 2 * q;
    const bool live0 = kFast || c0 < n, live1 = kFast || c0 + 1 < n;
    const unsigned rmask = (1u << rbits) - 1;
    const unsigned wmask = (1u << wlog) - 1;
    const int cq0 = live0 ? c0 : 0, cq1 = live1 ? c0 + 1 : cq0;
    const unsigned ldb8 = (unsigned)(ldb * 8);
    const char *Bc = reinterpret_cast<const char *>(B) + (size_t)cq0 * 8;
    typedef double v2d_t __attribute__((ext_vector_type(2)));
    auto brow = [&](unsigned kt) -> long long {
        const unsigned jc = kt >> rbits;
        if constexpr (kDirect) return (long long)jc;
        return ((long long)(jc >> wlog) << (wlog + 3)) | ((long long)x << wlog) | (jc & wmask);
    };
    constexpr long long kStride = (long long)(kCtThreads / 64) * 64;
    auto body = [&](long long it, bool tail) {
        const long long e = it + myoff;
        const long long ec = e < e1 ? e : e1 - 1;
        const unsigned kk = key[ec];
        const unsigned long long vb = (unsigned long long)__double_as_longlong(val[ec]);
        const unsigned vlo = (unsigned)vb, vhi = (unsigned)(vb >> 32);
        unsigned kt[8];
        kt[0] = ct_bcast<0>(kk); kt[1] = ct_bcast<1>(kk); kt[2] = ct_bcast<2>(kk); kt[3] = ct_bcast<3>(kk);
        kt[4] = ct_bcast<4>(kk); kt[5] = ct_bcast<5>(kk); kt[6] = ct_bcast<6>(kk); kt[7] = ct_bcast<7>(kk);
        double b0[8], b1[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if constexpr (kFast) {
                const v2d_t bb = *reinterpret_cast<const v2d_t *>(Bc + (unsigned)brow(kt[t]) * ldb8);
                b0[t] = bb.x;
                b1[t] = bb.y;
            } else {
                const double *br = B + brow(kt[t]) * ldb;
                b0[t] = br[cq0];
                b1[t] = br[cq1];
            }
        }
        unsigned lo[8], hi[8];
        lo[0] = ct_bcast<0>(vlo); lo[1] = ct_bcast<1>(vlo); lo[2] = ct_bcast<2>(vlo); lo[3] = ct_bcast<3>(vlo);
        lo[4] = ct_bcast<4>(vlo); lo[5] = ct_bcast<5>(vlo); lo[6] = ct_bcast<6>(vlo); lo[7] = ct_bcast<7>(vlo);
        hi[0] = ct_bcast<0>(vhi); hi[1] = ct_bcast<1>(vhi); hi[2] = ct_bcast<2>(vhi); hi[3] = ct_bcast<3>(vhi);
        hi[4] = ct_bcast<4>(vhi); hi[5] = ct_bcast<5>(vhi); hi[6] = ct_bcast<6>(vhi); hi[7] = ct_bcast<7>(vhi);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const double vt = __longlong_as_double((long long)(((unsigned long long)hi[t] << 32) | lo[t]));
            double *row_p = &tile[(kt[t] & rmask) * kCtPad];
            if (!tail && kFast) {
                atomicAdd(row_p + 2 * q, vt * b0[t]);
                atomicAdd(row_p + 2 * q + 1, vt * b1[t]);
            } else {  // dead lanes add +0.0 into the padding column
                const bool ok = it + 8 * t + mypos < e1;
                atomicAdd(row_p + ((ok && live0) ? 2 * q : kCtCols), (ok && live0) ? vt * b0[t] : 0.0);
                atomicAdd(row_p + ((ok && live1) ? 2 * q + 1 : kCtCols), (ok && live1) ? vt * b1[t] : 0.0);
            }
        }
        if constexpr (kSlots) {  // the slots' second entries (same B segments)
            const unsigned k2 = key2[ec];
            const unsigned long long wb = (unsigned long long)__double_as_longlong(val2[ec]);
            const unsigned wlo = (unsigned)wb, whi = (unsigned)(wb >> 32);
            unsigned r2[8];
            r2[0] = ct_bcast<0>(k2); r2[1] = ct_bcast<1>(k2); r2[2] = ct_bcast<2>(k2); r2[3] = ct_bcast<3>(k2);
            r2[4] = ct_bcast<4>(k2); r2[5] = ct_bcast<5>(k2); r2[6] = ct_bcast<6>(k2); r2[7] = ct_bcast<7>(k2);
            lo[0] = ct_bcast<0>(wlo); lo[1] = ct_bcast<1>(wlo); lo[2] = ct_bcast<2>(wlo); lo[3] = ct_bcast<3>(wlo);
            lo[4] = ct_bcast<4>(wlo); lo[5] = ct_bcast<5>(wlo); lo[6] = ct_bcast<6>(wlo); lo[7] = ct_bcast<7>(wlo);
            hi[0] = ct_bcast<0>(whi); hi[1] = ct_bcast<1>(whi); hi[2] = ct_bcast<2>(whi); hi[3] = ct_bcast<3>(whi);
            hi[4] = ct_bcast<4>(whi); hi[5] = ct_bcast<5>(whi); hi[6] = ct_bcast<6>(whi); hi[7] = ct_bcast<7>(whi);
            // predicated, not routed to the padding column: the 8 lanes of a
            // single-entry slot would all hit ONE address there, and
            // same-address LDS atomics serialise (measured 4x slower).  Every
            // row broadcast above already ran with all lanes active.
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const double vt = __longlong_as_double((long long)(((unsigned long long)hi[t] << 32) | lo[t]));
                const bool has2 = r2[t] != ~0u && (!tail || it + 8 * t + mypos < e1);
                double *row_p = &tile[(r2[t] & rmask) * kCtPad];
                if (has2 && live0) atomicAdd(row_p + 2 * q, vt * b0[t]);
                if (has2 && live1) atomicAdd(row_p + 2 * q + 1, vt * b1[t]);
            }
        }
    };
    long long it = e0 + (long long)wv * 64;
    for (; it + 64 <= e1; it += kStride) body(it, false);
    if (it < e1) body(it, true);  // uniform: this wave's partial iteration
    __syncthreads();
    // partial [slot][column][row] (column-major like C): coalesced over rows
    const int ncol = min(kCtCols, n - cg * kCtCols);
    double *out = part + ((long long)slot * n + cg * kCtCols) * m + r0;
    for (int i = threadIdx.x; i < nr * ncol; i += kCtThreads) {
        const int c = i / nr, r = i - c * nr;
        out[(long long)c * m + r] = tile[r * kCtPad + c];
    }
}

// C = alpha * sum_slot part[slot] (+ beta * C).  A workgroup owns 64 C
// entries (consecutive in the column-major partials, so every load is one
// coalesced 512-B run); its 4 waves split the slots (wave w: w, w+4, ...,
// 8 loads in flight per lane) and wave 0 adds the four sums in wave order:
// a fixed order, so C is the same on every run.  (One thread per entry
// walking all slots took 18-34 us on a rank's slice at N = 8, 64-128 slots.)
constexpr int kCtRedWaves = 4;
template <bool kBeta>
__global__ __launch_bounds__(64 * kCtRedWaves) void k_spmm_ctreduce(const double *__restrict__ part, int nslot,
                                                                    int m, int n, double alpha, double beta,
                                                                    double *__restrict__ C, long long ldc)
{
    __shared__ double red[kCtRedWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + lane;
    const long long mn = (long long)m * n;
    const bool live = i < mn;
    const int c = live ? (int)(i / m) : 0, r = live ? (int)(i - (long long)c * m) : 0;
    const double *p = part + (long long)c * m + r;
    const long long qs = (long long)n * m;  // one slot
    double s = 0.0;
    if (live) {
#pragma unroll 8
        for (int q = w; q < nslot; q += kCtRedWaves) s += p[(long long)q * qs];
    }
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && live) {
        double t = red[0][lane];
#pragma unroll
        for (int k = 1; k < kCtRedWaves; ++k) t += red[k][lane];
        double *o = C + (long long)c * ldc + r;
        *o = kBeta ? alpha * t + beta * *o : alpha * t;
    }
}

// ---- the SpMM shape ---------------------------------------------------------
// Every decision of the plan build (build_spmm_plan, build_ctile) and of a
// launch (launch_spmm) is taken by the pure host functions of this section;
// sblas_spmm_shape_host reports them for a host CSR without a GPU, and
// sblas_spmm_info what a built plan and its last launch took.
#ifndef SBLAS_SPMM_CTW
#define SBLAS_SPMM_CTW 11
#endif
#ifndef SBLAS_SPMM_CTR
#define SBLAS_SPMM_CTR kCtMaxRows
#endif

// the test options a plan build reads ("spmm_mfma_fill", "spmm_ctile")
struct SpmmOptions {
    double fill = SpmmPlan{}.fill_thresh;
    bool has_ct = false, ct = false;
};

static SpmmOptions spmm_options()
{
    SpmmOptions o;
    double opt = 0.0;
    if (test_option("spmm_mfma_fill", &opt)) o.fill = opt;
    if (test_option("spmm_ctile", &opt)) {
        o.has_ct = true;
        o.ct = opt != 0.0;
    }
    return o;
}

// a 16-row block of nz entries over nU distinct columns takes the MFMA tile
static bool spmm_block_dense(long long nz, size_t nU, double fill)
{
    return fill <= 1.0 && nU > 0 && (double)nz >= fill * 16.0 * (double)nU;
}

// The 16-row blocks: which are dense, and what the row kernels keep.  Blocks
// are analysed in parallel (a sort per block); Us (optional) receives the
// sorted column union of every dense block.
struct SpmmBlocks {
    std::vector<char> dense;
    int nmfma = 0, nsparse = 0;
    long long sparse_nnz = 0;
};

template <class RP>
static SpmmBlocks spmm_blocks(int m, const RP *rp, const int *col, double fill, std::vector<std::vector<int>> *Us)
{
    SpmmBlocks S;
    const int nblk = (m + 15) / 16;
    S.dense.assign((size_t)nblk, 0);
    if (Us) Us->assign((size_t)nblk, {});
#pragma omp parallel for schedule(dynamic, 4)
    for (int b = 0; b < nblk; ++b) {
        const int r0 = b * 16, r1 = std::min(m, r0 + 16);
        std::vector<int> U(col + rp[r0], col + rp[r1]);
        std::sort(U.begin(), U.end());
        U.erase(std::unique(U.begin(), U.end()), U.end());
        S.dense[(size_t)b] = spmm_block_dense((long long)(rp[r1] - rp[r0]), U.size(), fill);
        if (Us && S.dense[(size_t)b]) (*Us)[(size_t)b] = std::move(U);
    }
    for (int b = 0; b < nblk; ++b) {
        const int r0 = b * 16, r1 = std::min(m, r0 + 16);
        if (S.dense[(size_t)b]) {
            ++S.nmfma;
        } else {
            S.nsparse += r1 - r0;
            S.sparse_nnz += (long long)(rp[r1] - rp[r0]);
        }
    }
    return S;
}

// C-tile form: few rows (m <= 16,384: a tile of <= 1,204 rows per CU covers
// them in <= 14 row blocks), B much taller than the L2s (k >= 2^17: >= 64 MiB
// at n = 64), no MFMA blocks.  The test hook "spmm_ctile" = 0/1 overrides the
// size rule (0: the row kernels).
static bool spmm_wants_ctile(const SpmmOptions &o, int nmfma, int m, int k)
{
    if (o.has_ct) return o.ct && nmfma == 0 && m > 0;
    return nmfma == 0 && m > 0 && m <= 16384 && k >= (1 << 17);
}

// The C-tile layout's sizes for an m x k matrix whose plan is built by a call
// of width ncols.  supported = false when the packed key cannot hold
// XCD-local column and row (the caller keeps the row forms).
struct CtileShape {
    bool supported = false;
    int ns = 0, nrb = 0, R = 0, rbits = 0, wlog = 0;
    bool direct = false;
};

static CtileShape spmm_ctile_shape(int m, int k, int ncols)
{
    CtileShape T;
    if (m <= 0) return T;
    // slab width 2^wlog columns (11: 2048 B rows = 1 MiB of B per slab at n =
    // 64) and tile rows: experiment builds (Makefile `alt`) set
    // -DSBLAS_SPMM_CTW / -DSBLAS_SPMM_CTR
    T.wlog = std::max(4, std::min(20, SBLAS_SPMM_CTW));
    const int rmax = std::max(16, std::min(kCtMaxRows, (int)(SBLAS_SPMM_CTR)));
    T.nrb = (m + rmax - 1) / rmax;
    T.R = (m + T.nrb - 1) / T.nrb;
    T.rbits = 1;
    while ((1 << T.rbits) < T.R) ++T.rbits;
    const long long nslab = ((long long)k + (1LL << T.wlog) - 1) >> T.wlog;
    const long long jc_max = ((nslab + 7) / 8) << T.wlog;  // XCD-local columns
    T.supported = T.rbits + 1 <= 32 && jc_max <= (1LL << (32 - T.rbits));
    // slab sets per XCD: about one workgroup per CU (8 x ns x nrb x column
    // groups) for the C width of the call that builds the plan -- a rank of
    // a column split (16 or 32 columns) otherwise filled only 1/4 or 1/2 of
    // the CUs (config 4's column split at N = 2: 332 us against 345 at N = 1)
    // (two workgroups per CU where two tiles fit the LDS measured slower on
    // rank slices: config 4's N = 8 row block 105 -> 127 us, twice the
    // partial slots for the reduce; profiles/r05/spmm_grid/)
    const int ncg = std::max(1, (ncols + kCtCols - 1) / kCtCols);
    T.ns = std::max(1, 32 / (T.nrb * ncg));
    // direct keys (global column << rbits | row) when the column fits: the
    // kernel then needs no slab arithmetic; sorting is the same order
    T.direct = (long long)k <= (1LL << (32 - T.rbits));
    return T;
}

// which row kernel serves the rows outside MFMA blocks: 0 none (the C-tile
// form, or no such row), 1 wave per row, 2 workgroup per row (long rows on
// average)
static int spmm_rowform(bool ctile, int nrows, long long nnz_rows)
{
    if (ctile || nrows <= 0) return 0;
    return nnz_rows >= 256LL * nrows ? 2 : 1;
}

// One call's choices.  A column-major B is transposed into the handle's
// row-major panel (ld = n; a device allocation, so 16-B aligned whatever
// b_addr is).  fast: the C-tile kernel's 16-B loads at 32-bit byte offsets.
struct SpmmCall {
    bool transposes_B = false, fast = false, kbeta = false;
    long long ldr = 0;
};

static SpmmCall spmm_call_shape(bool ctile, int k, int n, long long ldb, int b_layout, unsigned long long b_addr,
                                double beta)
{
    SpmmCall c;
    c.transposes_B = b_layout == 0;
    c.ldr = c.transposes_B ? (long long)n : ldb;
    const unsigned long long addr = c.transposes_B ? 0ULL : b_addr;
    c.fast = ctile && (c.ldr % 2 == 0) && (n % kCtCols == 0) && ((addr & 15) == 0) &&
             (unsigned long long)k * (unsigned long long)c.ldr * 8ULL < (1ULL << 32);
    c.kbeta = beta != 0.0;
    return c;
}

// host: the C-tile layout of a supported shape T (spmm_ctile_shape)
static int build_ctile(sblas_csr_s &A, const std::vector<int> &rp, const std::vector<int> &hcol,
                       const std::vector<double> &hval, const CtileShape &T)
{
    SpmmPlan &P = A.mm;
    const int m = A.m, k = A.n;
    const int wlog = T.wlog, nrb = T.nrb, R = T.R, rbits = T.rbits, ns = T.ns;
    const long long nslab = ((long long)k + (1LL << wlog) - 1) >> wlog;
    // per-slab entry counts -> contiguous sets of about equal entries per XCD
    std::vector<long long> scount((size_t)nslab, 0);
    for (long long e = 0; e < A.nnz; ++e) scount[(size_t)(hcol[(size_t)e] >> wlog)]++;
    std::vector<int> set_of((size_t)nslab, 0);
    for (int x = 0; x < 8; ++x) {
        long long tot = 0;
        for (long long s = x; s < nslab; s += 8) tot += scount[(size_t)s];
        long long run = 0;
        for (long long s = x; s < nslab; s += 8) {
            set_of[(size_t)s] = tot ? (int)std::min<long long>(ns - 1, run * ns / tot) : 0;
            run += scount[(size_t)s];
        }
    }
    const int nbk = 8 * ns * nrb;  // buckets (XCD, set, row block)
    auto bucket = [&](int row, int c) {
        const int s = c >> wlog;
        return ((s & 7) * ns + set_of[(size_t)s]) * nrb + row / R;
    };
    std::vector<long long> off((size_t)nbk + 1, 0);
    for (int r = 0; r < m; ++r)
        for (int e = rp[r]; e < rp[r + 1]; ++e) off[(size_t)bucket(r, hcol[e]) + 1]++;
    for (int b = 0; b < nbk; ++b) off[(size_t)b + 1] += off[(size_t)b];
    const bool direct = T.direct;
    std::vector<unsigned long long> kv((size_t)std::max<long long>(A.nnz, 1));  // key << 32 | entry index
    {
        std::vector<long long> next(off.begin(), off.end() - 1);
        for (int r = 0; r < m; ++r)
            for (int e = rp[r]; e < rp[r + 1]; ++e) {
                const int c = hcol[e];
                const unsigned jc = direct ? (unsigned)c
                                           : (unsigned)((((long long)(c >> wlog) >> 3) << wlog) | (c & ((1 << wlog) - 1)));
                const unsigned kk = (jc << rbits) | (unsigned)(r % R);
                kv[(size_t)next[(size_t)bucket(r, c)]++] = ((unsigned long long)kk << 32) | (unsigned)e;
            }
    }
    // LDS banks: the entries 2g and 2g+1 of a kernel step share one 16-lane
    // group of the ds_add_f64 (b64: 32 banks of dwords); with the 17-double
    // row stride their dwords are disjoint exactly when the two rows differ
    // in parity.  So inside each aligned 8-entry step, odd rows go to the even
    // slots and even rows to the odd slots as far as the step allows (the
    // order inside a step does not change which products are summed).
    constexpr bool pair_rows = true;
#pragma omp parallel for schedule(dynamic, 1)
    for (int b = 0; b < nbk; ++b) {
        std::sort(kv.begin() + off[(size_t)b], kv.begin() + off[(size_t)b + 1]);
        if (!pair_rows) continue;
        const unsigned rm = (1u << rbits) - 1;
        for (long long w = off[(size_t)b]; w + 8 <= off[(size_t)b + 1]; w += 8) {
            unsigned long long odd[8], even[8];
            int no = 0, ne = 0;
            for (int i = 0; i < 8; ++i) {
                const unsigned long long e = kv[(size_t)(w + i)];
                if (((unsigned)(e >> 32) & rm) & 1u) odd[no++] = e;
                else even[ne++] = e;
            }
            int io = 0, ie = 0;
            for (int i = 0; i < 8; ++i) {  // even slot: odd row first; odd slot: even row first
                const bool want_odd = (i & 1) == 0;
                if ((want_odd && io < no) || (!want_odd && ie >= ne)) kv[(size_t)(w + i)] = odd[io++];
                else kv[(size_t)(w + i)] = even[ie++];
            }
        }
    }
    // Column-run slots (experiment builds, -DSBLAS_SPMM_CTSLOT=1): consecutive entries of
    // one column are paired into slots of two so one B segment feeds both
    // (rail4284: 0.59 slots per entry).  Measured slower on config 4: 0.435
    // against 0.362 ms -- L2 misses 10.0M against 6.0M per launch and more TD
    // stall cycles (the second key/value arrays), so entries stay the unit.
    std::vector<long long> soff((size_t)nbk + 1, 0);
    for (int b = 0; b < nbk; ++b) {
        long long ns_b = 0;
        for (long long e = off[(size_t)b]; e < off[(size_t)b + 1];) {
            long long f = e;
            const unsigned col = (unsigned)(kv[(size_t)e] >> 32) >> rbits;
            while (f < off[(size_t)b + 1] && ((unsigned)(kv[(size_t)f] >> 32) >> rbits) == col) ++f;
            ns_b += (f - e + 1) / 2;
            e = f;
        }
        soff[(size_t)b + 1] = soff[(size_t)b] + ns_b;
    }
#ifndef SBLAS_SPMM_CTSLOT
#define SBLAS_SPMM_CTSLOT 0
#endif
    const bool slots = SBLAS_SPMM_CTSLOT != 0 && A.nnz > 0;
    const long long nunits = slots ? soff.back() : A.nnz;
    std::vector<unsigned> hkey((size_t)std::max<long long>(nunits, 1)), hkey2;
    std::vector<double> hv((size_t)std::max<long long>(nunits, 1)), hv2;
    if (!slots) {
#pragma omp parallel for schedule(static)
        for (long long e = 0; e < A.nnz; ++e) {
            hkey[(size_t)e] = (unsigned)(kv[(size_t)e] >> 32);
            hv[(size_t)e] = hval[(size_t)(kv[(size_t)e] & 0xffffffffu)];
        }
    } else {
        hkey2.assign(hkey.size(), ~0u);
        hv2.assign(hv.size(), 0.0);
        const unsigned rm = (1u << rbits) - 1;
#pragma omp parallel for schedule(dynamic, 1)
        for (int b = 0; b < nbk; ++b) {
            // entries were parity-shuffled inside steps above: re-sort the
            // bucket so runs are contiguous, then pair each run's rows
            std::sort(kv.begin() + off[(size_t)b], kv.begin() + off[(size_t)b + 1]);
            long long o = soff[(size_t)b];
            for (long long e = off[(size_t)b]; e < off[(size_t)b + 1];) {
                long long f = e;
                const unsigned col = (unsigned)(kv[(size_t)e] >> 32) >> rbits;
                while (f < off[(size_t)b + 1] && ((unsigned)(kv[(size_t)f] >> 32) >> rbits) == col) ++f;
                for (long long i = e; i < f; i += 2, ++o) {
                    hkey[(size_t)o] = (unsigned)(kv[(size_t)i] >> 32);
                    hv[(size_t)o] = hval[(size_t)(kv[(size_t)i] & 0xffffffffu)];
                    if (i + 1 < f) {
                        hkey2[(size_t)o] = (unsigned)(kv[(size_t)i + 1] >> 32) & rm;
                        hv2[(size_t)o] = hval[(size_t)(kv[(size_t)i + 1] & 0xffffffffu)];
                    }
                }
                e = f;
            }
            // LDS banks: opposite-parity first rows in each 16-lane pair of a step
            if (!pair_rows) continue;
            for (long long w = soff[(size_t)b]; w + 8 <= soff[(size_t)b + 1]; w += 8) {
                int odd[8], even[8], no = 0, ne = 0;
                for (int i = 0; i < 8; ++i) {
                    if ((hkey[(size_t)(w + i)] & rm) & 1u) odd[no++] = i;
                    else even[ne++] = i;
                }
                unsigned tk[8], tk2[8];
                double tv[8], tv2[8];
                int io = 0, ie = 0;
                for (int i = 0; i < 8; ++i) {
                    const bool want_odd = (i & 1) == 0;
                    const int src = ((want_odd && io < no) || (!want_odd && ie >= ne)) ? odd[io++] : even[ie++];
                    tk[i] = hkey[(size_t)(w + src)];
                    tk2[i] = hkey2[(size_t)(w + src)];
                    tv[i] = hv[(size_t)(w + src)];
                    tv2[i] = hv2[(size_t)(w + src)];
                }
                for (int i = 0; i < 8; ++i) {
                    hkey[(size_t)(w + i)] = tk[i];
                    hkey2[(size_t)(w + i)] = tk2[i];
                    hv[(size_t)(w + i)] = tv[i];
                    hv2[(size_t)(w + i)] = tv2[i];
                }
            }
        }
        off = soff;
        SBLAS_HIP(hipMalloc(&P.ct_key2, sizeof(unsigned) * hkey2.size()));
        SBLAS_HIP(hipMalloc(&P.ct_val2, sizeof(double) * hv2.size()));
        SBLAS_HIP(hipMemcpy(P.ct_key2, hkey2.data(), sizeof(unsigned) * hkey2.size(), hipMemcpyHostToDevice));
        SBLAS_HIP(hipMemcpy(P.ct_val2, hv2.data(), sizeof(double) * hv2.size(), hipMemcpyHostToDevice));
    }
    P.ct_slots = slots;
    SBLAS_HIP(hipMalloc(&P.ct_key, sizeof(unsigned) * hkey.size()));
    SBLAS_HIP(hipMalloc(&P.ct_val, sizeof(double) * hv.size()));
    SBLAS_HIP(hipMalloc(&P.ct_off, sizeof(long long) * off.size()));
    SBLAS_HIP(hipMemcpy(P.ct_key, hkey.data(), sizeof(unsigned) * hkey.size(), hipMemcpyHostToDevice));
    SBLAS_HIP(hipMemcpy(P.ct_val, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice));
    SBLAS_HIP(hipMemcpy(P.ct_off, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice));
    P.ct_ns = ns;
    P.ct_nrb = nrb;
    P.ct_R = R;
    P.ct_rbits = rbits;
    P.ct_wlog = wlog;
    P.ct_direct = direct;
    return SBLAS_OK;
}

int build_spmm_plan(sblas_csr_s &A, int ncols, hipStream_t s)
{
    if (A.mm.ready) return SBLAS_OK;
    SpmmPlan &P = A.mm;
    const SpmmOptions opts = spmm_options();  // test hooks
    P.fill_thresh = opts.fill;
    const int m = A.m;
    const std::vector<int> &rp = A.h_rowptr;
    std::vector<int> hcol((size_t)A.nnz);
    std::vector<double> hval((size_t)A.nnz);
    if (A.nnz) {
        SBLAS_HIP(hipMemcpy(hcol.data(), A.col, sizeof(int) * A.nnz, hipMemcpyDeviceToHost));
        SBLAS_HIP(hipMemcpy(hval.data(), A.val, sizeof(double) * A.nnz, hipMemcpyDeviceToHost));
    }
    std::vector<int> mblock, mchunk{0}, ucol, srows;
    std::vector<double> atile;

    // 16-row blocks: the distinct columns of each (sorted) decide whether the
    // block is dense enough for the MFMA tile; assembled in block order
    const int nblk = (m + 15) / 16;
    std::vector<std::vector<int>> Us;
    const SpmmBlocks S = spmm_blocks(m, rp.data(), hcol.data(), P.fill_thresh, &Us);
    const std::vector<char> &dense = S.dense;
    for (int b = 0; b < nblk; ++b) {
        const int r0 = b * 16, r1 = std::min(m, r0 + 16);
        if (!dense[(size_t)b]) {
            for (int r = r0; r < r1; ++r) srows.push_back(r);
            continue;
        }
        const std::vector<int> &U = Us[(size_t)b];
        const int nch = ((int)U.size() + 3) / 4;
        const size_t t0 = atile.size();
        atile.resize(t0 + (size_t)nch * 64, 0.0);
        for (int c = 0; c < nch * 4; ++c) ucol.push_back(c < (int)U.size() ? U[c] : U[0]);
        for (int r = r0; r < r1; ++r)
            for (int j = rp[r]; j < rp[r + 1]; ++j) {
                const int k = (int)(std::lower_bound(U.begin(), U.end(), hcol[j]) - U.begin());
                // lane l of chunk k/4 holds A[l & 15][4*(k/4) + (l >> 4)]
                atile[t0 + (size_t)(k / 4) * 64 + (size_t)((k % 4) * 16 + (r - r0))] += hval[j];
            }
        mblock.push_back(b);
        mchunk.push_back(mchunk.back() + nch);
    }
    P.nmfma = S.nmfma;
    P.nsparse = S.nsparse;
    P.sparse_nnz = S.sparse_nnz;
    auto up = [&](auto **dst, const auto &v) -> int {
        using T = typename std::decay_t<decltype(v)>::value_type;
        SBLAS_HIP(hipMalloc(dst, sizeof(T) * std::max<size_t>(v.size(), 1)));
        if (!v.empty()) SBLAS_HIP(hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
        return SBLAS_OK;
    };
    SBLAS_TRY(up(&P.mblock, mblock));
    SBLAS_TRY(up(&P.mchunk, mchunk));
    SBLAS_TRY(up(&P.ucol, ucol));
    SBLAS_TRY(up(&P.atile, atile));
    SBLAS_TRY(up(&P.srows, srows));
    const CtileShape T = spmm_ctile_shape(m, A.n, ncols);
    P.ct_supported = T.supported;
    if (spmm_wants_ctile(opts, P.nmfma, m, A.n) && T.supported) SBLAS_TRY(build_ctile(A, rp, hcol, hval, T));
    (void)s;
    P.ready = true;
    return SBLAS_OK;
}

void free_spmm_plan(sblas_csr_s &A)
{
    SpmmPlan &P = A.mm;
    (void)hipFree(P.mblock);
    (void)hipFree(P.mchunk);
    (void)hipFree(P.ucol);
    (void)hipFree(P.atile);
    (void)hipFree(P.srows);
    (void)hipFree(P.ct_key);
    (void)hipFree(P.ct_val);
    (void)hipFree(P.ct_off);
    (void)hipFree(P.ct_key2);
    (void)hipFree(P.ct_val2);
    A.mm = SpmmPlan{};
}

// col-major B (k x n, ld=ldb) -> row-major panel Bt (k x n, ld=n)
__global__ void k_transpose_B(const double *__restrict__ B, long long ldb, int k, int n,
                              double *__restrict__ Bt)
{
    __shared__ double tile[64][65];
    const int j0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 256 threads: 64 x 4
    for (int cc = ty; cc < 64; cc += 4) {
        const int j = j0 + tx, c = c0 + cc;
        if (j < k && c < n) tile[cc][tx] = B[(long long)c * ldb + j];
    }
    __syncthreads();
    for (int jj = ty; jj < 64; jj += 4) {
        const int j = j0 + jj, c = c0 + tx;
        if (j < k && c < n) Bt[(long long)j * n + c] = tile[tx][jj];
    }
}

// grow a handle-owned scratch buffer (sblas_csr_s::spmm_*)
static int grow_scratch(double *&buf, size_t &bytes, size_t need)
{
    if (bytes >= need) return SBLAS_OK;
    (void)hipFree(buf);
    buf = nullptr;
    bytes = 0;
    SBLAS_HIP(hipMalloc(&buf, need));
    bytes = need;
    return SBLAS_OK;
}

int launch_spmm(const sblas_csr_s &A, int n, double alpha, const double *B, int ldb,
                int b_layout, double beta, double *C, int ldc, hipStream_t s)
{
    if (A.m == 0 || n == 0) return SBLAS_OK;
    const SpmmPlan &P = A.mm;
    const bool ctile = P.ready && P.ct_nrb > 0;
    const SpmmCall call = spmm_call_shape(ctile, A.n, n, ldb, b_layout, (unsigned long long)(uintptr_t)B, beta);
    A.spmm_last[0] = call.fast;
    A.spmm_last[1] = call.transposes_B;
    A.spmm_last[2] = call.kbeta;
    const double *Brow = B;
    const long long ldr = call.ldr;
    if (call.transposes_B) {
        SBLAS_TRY(grow_scratch(A.spmm_bt, A.spmm_bt_bytes, sizeof(double) * (size_t)A.n * (size_t)n));
        if (A.n > 0) {
            dim3 grid((A.n + 63) / 64, (n + 63) / 64);
            hipLaunchKernelGGL(k_transpose_B, grid, dim3(256), 0, s, B, (long long)ldb, A.n, n, A.spmm_bt);
        }
        Brow = A.spmm_bt;
    }
    const int nslab = (n + 63) / 64;
    if (ctile) {
        const int ncg = (n + kCtCols - 1) / kCtCols;
        const int nslot = 8 * P.ct_ns;
        SBLAS_TRY(grow_scratch(A.spmm_part, A.spmm_part_bytes,
                               sizeof(double) * (size_t)nslot * (size_t)n * (size_t)A.m));
        double *const part = A.spmm_part;
        const long long nwg = 8LL * P.ct_ns * P.ct_nrb * ncg;
        const size_t lds = sizeof(double) * (size_t)P.ct_R * kCtPad;
        static thread_local bool attr_set[64] = {};
        if (!attr_set[A.device & 63]) {  // > 64 KiB of dynamic LDS
            const void *ks[8] = {
                (const void *)k_spmm_ctile<true, false, false>, (const void *)k_spmm_ctile<true, true, false>,
                (const void *)k_spmm_ctile<false, false, false>, (const void *)k_spmm_ctile<false, true, false>,
                (const void *)k_spmm_ctile<true, false, true>, (const void *)k_spmm_ctile<true, true, true>,
                (const void *)k_spmm_ctile<false, false, true>, (const void *)k_spmm_ctile<false, true, true>};
            for (const void *kf : ks)
                SBLAS_HIP(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)(sizeof(double) * kCtMaxRows * kCtPad)));
            attr_set[A.device & 63] = true;
        }
        const bool fast = call.fast;
        using K = void (*)(const unsigned *, const double *, const unsigned *, const double *, const long long *,
                           int, int, int, int, int, int, const double *, long long, int, int, double *);
        K kern;
        if (P.ct_slots)
            kern = P.ct_direct ? (fast ? k_spmm_ctile<true, true, true> : k_spmm_ctile<true, false, true>)
                               : (fast ? k_spmm_ctile<false, true, true> : k_spmm_ctile<false, false, true>);
        else
            kern = P.ct_direct ? (fast ? k_spmm_ctile<true, true, false> : k_spmm_ctile<true, false, false>)
                               : (fast ? k_spmm_ctile<false, true, false> : k_spmm_ctile<false, false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(kCtThreads), lds, s, P.ct_key, P.ct_val, P.ct_key2,
                           P.ct_val2, P.ct_off, P.ct_ns, P.ct_nrb, P.ct_R, P.ct_rbits, P.ct_wlog, ncg, Brow, ldr,
                           n, A.m, part);
        const unsigned nb = (unsigned)(((long long)A.m * n + 63) / 64);
        if (call.kbeta)
            hipLaunchKernelGGL(k_spmm_ctreduce<true>, dim3(nb), dim3(64 * kCtRedWaves), 0, s, part, nslot, A.m, n,
                               alpha, beta, C, (long long)ldc);
        else
            hipLaunchKernelGGL(k_spmm_ctreduce<false>, dim3(nb), dim3(64 * kCtRedWaves), 0, s, part, nslot, A.m, n,
                               alpha, beta, C, (long long)ldc);
        SBLAS_HIP(hipGetLastError());
        return SBLAS_OK;
    }
    // rows of sparse blocks (all rows when no plan / no dense block)
    const int nrows = P.ready ? P.nsparse : A.m;
    const int *rows = P.ready ? P.srows : nullptr;
    const int rowform = spmm_rowform(false, nrows, P.ready ? P.sparse_nnz : A.nnz);
    if (rowform == 2) {
        const unsigned nb = (unsigned)((long long)nrows * nslab);
        if (call.kbeta)
            hipLaunchKernelGGL(k_spmm_rowsplitk<true>, dim3(nb), dim3(256), 0, s, A.rowptr, A.rowptr + 1,
                               A.col, A.val, Brow, ldr, nrows, n, nslab, alpha, beta, C, (long long)ldc, rows);
        else
            hipLaunchKernelGGL(k_spmm_rowsplitk<false>, dim3(nb), dim3(256), 0, s, A.rowptr, A.rowptr + 1,
                               A.col, A.val, Brow, ldr, nrows, n, nslab, alpha, beta, C, (long long)ldc, rows);
    } else if (rowform == 1) {
        const long long waves = (long long)nrows * nslab;
        const unsigned nb = (unsigned)((waves + 3) / 4);
        if (call.kbeta)
            hipLaunchKernelGGL(k_spmm_rowwave<true>, dim3(nb), dim3(256), 0, s, A.rowptr, A.col, A.val,
                               Brow, ldr, nrows, n, nslab, alpha, beta, C, (long long)ldc, rows);
        else
            hipLaunchKernelGGL(k_spmm_rowwave<false>, dim3(nb), dim3(256), 0, s, A.rowptr, A.col, A.val,
                               Brow, ldr, nrows, n, nslab, alpha, beta, C, (long long)ldc, rows);
    }
    if (P.ready && P.nmfma > 0) {
        const long long waves = (long long)P.nmfma * nslab;
        const unsigned nb = (unsigned)((waves + 3) / 4);
        if (call.kbeta)
            hipLaunchKernelGGL(k_spmm_mfma<true>, dim3(nb), dim3(256), 0, s, P.mblock, P.mchunk, P.ucol,
                               P.atile, P.nmfma, Brow, ldr, A.m, n, nslab, alpha, beta, C,
                               (long long)ldc);
        else
            hipLaunchKernelGGL(k_spmm_mfma<false>, dim3(nb), dim3(256), 0, s, P.mblock, P.mchunk, P.ucol,
                               P.atile, P.nmfma, Brow, ldr, A.m, n, nslab, alpha, beta, C,
                               (long long)ldc);
    }
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

}  // namespace sblas

extern "C" int sblas_spmm_shape_host(int m, int k, const long long *rowptr, const int *col, int ncols_plan,
                                     int ncols, long long ldb, int b_layout, unsigned long long b_addr,
                                     double beta, long long *info)
{
    using namespace sblas;
    if (m < 0 || k < 0 || !rowptr || !info || ncols_plan < 0 || ncols < 0 || (b_layout != 0 && b_layout != 1))
        return SBLAS_ERR_INVALID;
    if (rowptr[0] != 0 || rowptr[m] > INT_MAX || (rowptr[m] > 0 && !col)) return SBLAS_ERR_INVALID;
    for (int r = 0; r < m; ++r)
        if (rowptr[r + 1] < rowptr[r]) return SBLAS_ERR_INVALID;
    const SpmmOptions opts = spmm_options();
    const SpmmBlocks S = spmm_blocks(m, rowptr, col, opts.fill, nullptr);
    const CtileShape T = spmm_ctile_shape(m, k, ncols_plan);
    const bool ctile = spmm_wants_ctile(opts, S.nmfma, m, k) && T.supported;
    const SpmmCall c = spmm_call_shape(ctile, k, ncols, ldb, b_layout, b_addr, beta);
    const long long v[15] = {S.nmfma, S.nsparse, S.sparse_nnz, spmm_rowform(ctile, S.nsparse, S.sparse_nnz),
                             ctile ? 1 : 0, T.supported ? 1 : 0, ctile ? T.ns : 0, ctile ? T.nrb : 0,
                             ctile ? T.R : 0, ctile ? T.rbits : 0, ctile ? T.wlog : 0, ctile && T.direct ? 1 : 0,
                             c.fast ? 1 : 0, c.transposes_B ? 1 : 0, c.kbeta ? 1 : 0};
    for (int i = 0; i < 15; ++i) info[i] = v[i];
    return SBLAS_OK;
}

extern "C" int sblas_spmm_info(sblas_csr A, long long *info)
{
    using namespace sblas;
    if (!A || !info || !A->mm.ready) return SBLAS_ERR_INVALID;
    const SpmmPlan &P = A->mm;
    const bool ctile = P.ct_nrb > 0;
    const long long v[15] = {P.nmfma, P.nsparse, P.sparse_nnz, spmm_rowform(ctile, P.nsparse, P.sparse_nnz),
                             ctile ? 1 : 0, P.ct_supported ? 1 : 0, P.ct_ns, P.ct_nrb, P.ct_R, P.ct_rbits, P.ct_wlog,
                             P.ct_direct ? 1 : 0, A->spmm_last[0], A->spmm_last[1], A->spmm_last[2]};
    for (int i = 0; i < 15; ++i) info[i] = v[i];
    return SBLAS_OK;
}
