// transpose.hip -- device CSR -> CSC transpose with bit-exact indices.
//
// Semantics of sptrsv/sptrsv_v1/src/tranpose.h:6-43 (matrix_transposition):
// column histogram, exclusive scan, then a STABLE scatter in row order, so
// row indices ascend inside every column and equal-(row,col) duplicates keep
// their CSR order.  GPU forms, both stable sorts of the nonzeros (in CSR
// order) by column, so rows ascend inside each column exactly as the
// reference's ordered scatter leaves them:
//  * MSD (512 < n <= 2^24) -- two stable partition passes on the high column
//    bits (pass A over fixed segments of the CSR order, deriving each entry's
//    row from rowptr; pass B inside each pass-A bucket), then one pass per
//    final bucket of 2^c columns that counts, ranks and writes its run in
//    column order with its colptr entries.  Between the passes an entry
//    travels as one packed word (the key bits still needed + the row or its
//    offset in the segment) and its value;
//  * LSD radix passes of <= 8-bit digits carrying (key, row, value), colptr
//    read off the sorted keys: where the two MSD passes do not exist (n <=
//    512) or their digits would exceed 8 bits (n > 2^24).
// Which form a matrix takes, and every launch shape, is decided by the pure
// host function transpose_shape; launch_transpose only reads it off.
// The multi-device driver is transpose_mgpu.hip, the scan scan.hip.
#include <algorithm>
#include <climits>

#include "sblas_internal.hpp"
#include "scan.hpp"

namespace sblas {

// Tiles of kRxTile consecutive nonzeros, digits of at most kRxMaxBits bits.
// No pass uses global atomics (they execute memory-side, one 64-B request
// per lane).
constexpr int kRxTile = 4096;
// a workgroup's partially written digit runs -- 2^rb per array -- must fit
// its share of the XCD's L2 until they merge; 11-bit digits measured 0.85 ms
// per pass against ~0.3 ms
constexpr int kRxMaxBits = 8;
// workgroups per CU a pass is sized for: one round of resident workgroups
constexpr int kRxWgPerCu = 2;

// row of every nonzero (the LSD passes; MSD pass A derives the rows from
// rowptr itself): a wave per 64 rows writes them one after another,
// all 64 lanes on one row's entries (consecutive stores).  (A thread per
// row left a long row's lane storing ~100 words alone -- 84 us on the
// config-2 matrix; 16-B stores per thread 157 us; a binary search per four
// entries 176 us, its 21 dependent loads per thread.)
__global__ __launch_bounds__(256) void k_expand_rows(const int *__restrict__ rowptr, int m, int *__restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const int r0 = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 64;
    if (r0 >= m) return;
    const int nrow = min(64, m - r0);
    const int b = rowptr[min(r0 + lane, m)];
    const int last = rowptr[r0 + nrow];
    for (int j = 0; j < nrow; ++j) {
        const int s = __builtin_amdgcn_readlane(b, j);
        const int e = j + 1 < nrow ? __builtin_amdgcn_readlane(b, j + 1) : last;
        for (int k = s + lane; k < e; k += 64) rows[k] = r0 + j;
    }
}

// ---- the passes.  Workgroup b sorts the contiguous tiles [b*S, (b+1)*S) in
// order, so (i) the count matrix is digits x workgroups, not digits x tiles,
// and (ii) a digit's output run of tile t+1 continues exactly where tile t's
// ended: the same CU appends to the same lines, which its XCD's L2 merges
// before write-back.  Ranking per 64-element batch: rb wave ballots give the
// in-wave rank; the first lane of each (wave, digit) group posts the group's
// size, so LDS work per element is O(waves), not O(digits).
// scatter workgroup size: 512 threads = 8 waves, 8 entries per thread of a
// 4096-entry tile (256 threads left only 8 waves per CU at 71 KiB of LDS)
constexpr int kR2Threads = 512;

// Segments.  kSegTiles: workgroup w's contiguous tiles [w*S, (w+1)*S), counts
// indexed [digit][w].  kSegBuckets (the MSD passes): workgroup w = b*J + j
// takes part j of J of bucket b, the bucket's range read off the previous
// pass's scanned counts (bucket b = entries [Jp*b, Jp*b + Jp) of prev), and
// counts are indexed [(b*D + digit)*J + j], so one inclusive scan of them,
// bucket-major, yields the stable partition of every bucket by the digit.
constexpr int kSegTiles = 0, kSegBuckets = 1;

struct SegArgs {
    int S, nwg;               // kSegTiles
    const int *prev;          // kSegBuckets: previous pass's inclusive scan
    int Jp, J;
    int nb;                   // kSegFinal: number of buckets (grid-stride)
};

__device__ __forceinline__ void seg_range(int mode, const SegArgs &g, int wg, long long nnz, long long &s0,
                                          long long &s1)
{
    if (mode == kSegTiles) {
        s0 = (long long)wg * g.S * kRxTile;
        s1 = min(nnz, s0 + (long long)g.S * kRxTile);
        if (s0 > s1) s0 = s1;
        return;
    }
    const int b = wg / g.J, j = wg % g.J;
    const long long i0 = (long long)b * g.Jp;
    const long long bs = i0 ? g.prev[i0 - 1] : 0, be = g.prev[i0 + g.Jp - 1];
    const long long len = be - bs;
    s0 = bs + len * j / g.J;
    s1 = bs + len * (j + 1) / g.J;
}

__device__ __forceinline__ size_t seg_count_idx(int mode, const SegArgs &g, int wg, int D, int d)
{
    if (mode == kSegTiles) return (size_t)d * g.nwg + wg;
    return ((size_t)(wg / g.J) * D + d) * g.J + (wg % g.J);
}

// counts of each scatter workgroup's segment: one 1024-thread workgroup per
// segment, 16 keys in flight per thread, LDS histogram, then every digit's
// count stored plainly (no zeroing, no global atomics: with eight workgroups
// per segment merging by atomics the two count passes took 75 us each on the
// config-2 matrix, memory-side atomics being one 64-B request per lane).
constexpr int kCntThreads = 1024;
// wgrow (MSD pass A): also the row holding each segment's first entry,
// the start of the scatter's row derivation.
template <int kSeg>
__global__ __launch_bounds__(kCntThreads) void k_rx2_count(const int *__restrict__ keys, long long nnz,
                                                           int shift, int rb, SegArgs g,
                                                           int *__restrict__ counts,
                                                           const int *__restrict__ rowptr = nullptr, int m = 0,
                                                           int *__restrict__ wgrow = nullptr)
{
    // digits <= 128: one private histogram per wave (waves do not contend
    // for the same LDS words), summed at the end
    constexpr int kCW = kCntThreads / 64;
    __shared__ int h[128 * kCW];  // 2,048 ints
    static_assert(128 * kCW >= (1 << kRxMaxBits), "the shared histogram of wider digits fits");
    __shared__ int s_first;
    const int D = 1 << rb;
    const bool priv = D <= 128;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int *hw = priv ? h + wv * 128 : h;
    for (int d = threadIdx.x; d < (priv ? 128 * kCW : D); d += kCntThreads) h[d] = 0;
    const int wg = (int)blockIdx.x;
    long long p0, p1;
    seg_range(kSeg, g, wg, nnz, p0, p1);
    int lo = 0;
    if (wgrow && wv < 2) {
        // wave 0: the row holding the segment's first entry (largest r with
        // rowptr[r] <= p0); wave 1: the row of its last; wgrow[nseg + wg] =
        // the rows the segment spans beyond its first (0 when empty).  A
        // 64-ary search: each round the 64 lanes probe evenly spaced rows.
        const long long p = wv == 0 ? p0 : max(p0, p1 - 1);
        int hi = m - 1;  // rowptr[lo] <= p
        while (lo < hi) {
            const int step = (hi - lo + 63) / 64;
            const long long r = (long long)lo + (long long)(lane + 1) * step;
            const bool ok = r <= hi && rowptr[r] <= p;
            const int k = __popcll(__ballot(ok));  // ok holds for a prefix of the lanes
            lo += k * step;
            hi = min(hi, lo + step - 1);
        }
        if (wv == 0 && lane == 0) {
            wgrow[wg] = lo;
            s_first = lo;
        }
    }
    __syncthreads();  // histograms zeroed, s_first set
    if (wgrow && wv == 1 && lane == 0) wgrow[(int)gridDim.x + wg] = p1 > p0 ? lo - s_first : 0;
    // 16-B loads over the aligned body (keys arrays are 16-B aligned), single
    // keys for the head and tail
    const long long q0 = min(p1, (p0 + 3) & ~3LL), q1 = max(q0, p1 & ~3LL);
    for (long long i = p0 + threadIdx.x; i < q0; i += kCntThreads) atomicAdd(&hw[(keys[i] >> shift) & (D - 1)], 1);
    for (long long i = q1 + threadIdx.x; i < p1; i += kCntThreads) atomicAdd(&hw[(keys[i] >> shift) & (D - 1)], 1);
    const int4 *k4 = reinterpret_cast<const int4 *>(keys + q0);
    const long long n4 = (q1 - q0) >> 2;
    constexpr int kU = 8;
    for (long long i0 = 0; i0 < n4; i0 += (long long)kU * kCntThreads) {
        int4 v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long i = i0 + (long long)u * kCntThreads + threadIdx.x;
            v[u] = i < n4 ? k4[i] : make_int4(-1, -1, -1, -1);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (v[u].x != -1) {
                atomicAdd(&hw[(v[u].x >> shift) & (D - 1)], 1);
                atomicAdd(&hw[(v[u].y >> shift) & (D - 1)], 1);
                atomicAdd(&hw[(v[u].z >> shift) & (D - 1)], 1);
                atomicAdd(&hw[(v[u].w >> shift) & (D - 1)], 1);
            }
    }
    __syncthreads();
    for (int dd = threadIdx.x; dd < D; dd += kCntThreads) {
        int c = h[dd];
        if (priv)
            for (int q = 1; q < kCW; ++q) c += h[q * 128 + dd];
        counts[seg_count_idx(kSeg, g, wg, D, dd)] = c;
    }
}

// Scatter: workgroup b sorts tiles [b*S, (b+1)*S) in order.  Wave w ranks
// the contiguous quarter [w*1024, (w+1)*1024) of a tile in 16 batches of 64
// with WAVE-PRIVATE digit counters (a wave's LDS operations retire in
// program order, so no barrier per batch): rank = wcnt[w][d] + in-batch rank
// from RB ballots.  Two barriers per tile then turn the per-wave counts into
// the tile's digit offsets.  The next tile's (key, row, value) are loaded
// into registers while the current one is ranked and written.
// kSegFinal (the MSD transpose's last pass): workgroup b owns bucket b of the
// previous pass whole (its entries share every column bit above `rb`), counts
// its digits itself, so its output is the contiguous run [s0, s1) in column
// order; it writes colptr for its 2^rb columns, and keys only if kout.
constexpr int kSegFinal = 2;

// kDerive (the MSD transpose's pass A): the entries' rows are not read from
// an expanded array but derived per tile from rowptr.  The workgroup walks
// its tiles in order with the row rc that contains the tile's first entry
// (the first from wgrow[], written by the count pass).  Thread t holds the
// start of row rc+1+t (a window of kR2Threads rows, loaded one tile ahead);
// each row starting inside the tile marks its position in srow with atomicMax
// (empty rows share a position, the largest wins), and a prefix max over the
// positions -- per wave over its contiguous part, then across waves -- is
// every entry's row.  Rows starting exactly at the tile's end give the next
// tile's rc.  A tile holding more than kR2Threads row starts takes more
// windows.
// kPkF (last pass, packed input): rows are unpacked from the staged keys, so
// no row array is staged (less LDS: more workgroups per CU); kWpe: waves per
// SIMD asked of the register allocator.
template <int kMaxD, int kSeg, bool kDerive = false, int kTile = kRxTile, bool kPkF = false,
          int kWpe = 1>
__global__ __launch_bounds__(kR2Threads, kWpe) void k_rx2_scatter(
    const int *__restrict__ kin, const int *__restrict__ rin, const double *__restrict__ vin, long long nnz,
    int shift, int rb, SegArgs sg, const int *__restrict__ incl, int *__restrict__ kout,
    int *__restrict__ rout, double *__restrict__ vout, int *__restrict__ colptr, int n, int pack,
    const int *__restrict__ rowptr = nullptr, int m = 0, const int *__restrict__ wgrow = nullptr,
    int packA = -1)
{
    constexpr bool kFinal = kSeg == kSegFinal;
    // packA (MSD passes A and B): pass A writes ONE word per entry, the key's
    // low packA bits (all pass B and the last pass read) with the row's offset
    // from its segment's first row above them, and no row array; pass B finds
    // each entry's segment (the segments' runs inside its bucket, in LDS) and
    // adds that segment's first row.  Taken when every segment spans fewer
    // than 2^(32 - packA) rows (wgrow[nseg + s] = segment s's span, from the
    // count pass); all workgroups read the same spans, so all agree.
    constexpr bool kPA = (kSeg == kSegTiles && kDerive) || kSeg == kSegBuckets;
    constexpr int kSegMax = 512;
    __shared__ int s_segstart[kSeg == kSegBuckets ? kSegMax + 1 : 1];
    __shared__ int s_segrow[kSeg == kSegBuckets ? kSegMax : 1];
    constexpr int kW = kR2Threads / 64;  // waves
    __shared__ int wcnt[kW][kMaxD];  // per-wave counts, then per-wave starts
    __shared__ int lstart[kMaxD], gbase[kMaxD];
    __shared__ int wtot[kW];
    __shared__ int wmaxs[kW], s_next, s_more[2];  // kDerive
    __shared__ int skey[kTile], srow[kPkF ? 1 : kTile];
    __shared__ double sval[kTile];
    constexpr int kQ = kTile / kW;  // elements per wave per tile
    constexpr int kB = kQ / 64;             // batches per wave (16)
    static_assert(kB * kR2Threads == kTile, "one register slot per batch");
    static_assert(kTile == kRxTile || kFinal, "tile segments (seg_range) assume kRxTile");
    const int D = 1 << rb, dm = D - 1;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    long long s0, s1;
    seg_range(kFinal ? kSegBuckets : kSeg, sg, (int)blockIdx.x, nnz, s0, s1);
    int bk = (int)blockIdx.x;  // the last pass: current bucket (grid-stride)
    // column written to kout by the last pass: its bucket's bits and the key's
    // low rb bits (the key above them may be a packed word)
    auto colkey = [&](int k) { return kFinal ? ((bk << rb) | (k & dm)) : k; };
    bool pA = false;  // workgroup-uniform
    const int nseg = kSeg == kSegBuckets ? sg.Jp : (int)gridDim.x;
    if constexpr (kPA) {
        if (packA >= 0 && nseg <= kSegMax) {
            int v = 0;
            for (int i = t; i < nseg; i += kR2Threads) v = max(v, wgrow[nseg + i]);
#pragma unroll
            for (int off = 32; off; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
            if (lane == 0) wmaxs[w] = v;
            __syncthreads();
            int mx = 0;
#pragma unroll
            for (int q = 0; q < kW; ++q) mx = max(mx, wmaxs[q]);
            pA = packA >= 31 || mx < (1 << (32 - packA));
            __syncthreads();
        }
    }
    const unsigned kbmask = packA >= 0 && packA < 32 ? (1u << packA) - 1u : ~0u;
    int segrow0 = 0;  // pass A: the segment's first row
    int scur = 0;     // pass B: this wave's current segment
    int kk[kB], rr[kB];
    double vv[kB];
    auto rowof = [&](int j) { return (kFinal && pack >= 0) ? (int)((unsigned)kk[j] >> pack) : rr[j]; };
    auto load_tile = [&](long long base, int valid) {
#pragma unroll
        for (int j = 0; j < kB; ++j) {
            const int li = w * kQ + j * 64 + lane;
            const bool ok = li < valid;
            const long long gi = ok ? base + li : 0;
            kk[j] = ok ? kin[gi] : -1;  // top digit, ranked after every real element
            // a packed last-pass key carries the row; it is unpacked where it is
            // used (here it would make the prefetch wait for its load)
            if (!(kFinal && pack >= 0) && !kDerive && !(kSeg == kSegBuckets && pA)) rr[j] = ok ? rin[gi] : 0;
            vv[j] = ok ? vin[gi] : 0.0;
        }
    };
    // Steps 1-5 on the tile in registers (valid entries); the tile at
    // (nbase, nvalid) is loaded into the registers between staging and
    // write-out; gbase[] then points past this tile's runs.
    int rc = 0, wv = 0;  // kDerive: row containing the tile's first entry; window
    auto derive_rows = [&](long long cbase, int valid) {
        int rw = rc, wvv = wv;
        for (int round = 0;; ++round) {
            const int r = rw + 1 + t;
            if (r < m) {
                const long long p = (long long)wvv - cbase;  // >= 1: rows after rc start past cbase
                if (p < valid) atomicMax(&srow[p], r);
                else if (p == valid) atomicMax(&s_next, r);
            }
            if (t == kR2Threads - 1) s_more[round & 1] = (r < m && (long long)wvv <= cbase + valid) ? 1 : 0;
            __syncthreads();
            if (!s_more[round & 1]) break;
            rw += kR2Threads;
            wvv = rowptr[min(rw + 1 + t, m)];
        }
        int run = -1;
#pragma unroll
        for (int j = 0; j < kB; ++j) {
            int v = srow[w * kQ + j * 64 + lane];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int u = __shfl_up(v, off, 64);
                if (lane >= off) v = max(v, u);
            }
            v = max(v, run);
            rr[j] = v;
            run = __builtin_amdgcn_readlane(v, 63);
        }
        if (lane == 0) wmaxs[w] = run;
        __syncthreads();
        int pre = -1, all = s_next;
#pragma unroll
        for (int q = 0; q < kW; ++q) {
            const int mq = wmaxs[q];
            if (q < w) pre = max(pre, mq);
            all = max(all, mq);
        }
#pragma unroll
        for (int j = 0; j < kB; ++j) rr[j] = max(rr[j], pre);
        rc = all;  // the next tile's first entry lies in row rc
        wv = rowptr[min(rc + 1 + t, m)];
    };
    // srow = -1 everywhere but srow[0] = rc (the row of the tile's first entry)
    auto derive_init = [&]() {
#pragma unroll
        for (int j = 0; j < kB; ++j) srow[w * kQ + j * 64 + lane] = -1;
        if (t == 0) {
            srow[0] = rc;
            s_next = rc;
        }
    };
    auto process_tile = [&](int valid, long long nbase, int nvalid, long long cbase) {
        if constexpr (kDerive) derive_rows(cbase, valid);
        int lp[kB];
        // 1. wave-private ranking
#pragma unroll
        for (int j = 0; j < kB; ++j) {
            const int d = (kk[j] >> shift) & dm;
            unsigned long long mm = ~0ull;
            for (int b = 0; b < rb; ++b) {
                const unsigned long long bal = __ballot((d >> b) & 1);
                mm &= ((d >> b) & 1) ? bal : ~bal;
            }
            const int rank = __popcll(mm & lt);
            lp[j] = wcnt[w][d] + rank;
            if (rank == 0) wcnt[w][d] += __popcll(mm);
        }
        // padding (top digit, after every real element) is not part of the output
        if (t == kR2Threads - 1 && valid < kTile) wcnt[kW - 1][dm] -= kTile - valid;
        __syncthreads();
        // 2. digit totals, per-wave starts inside each digit, exclusive scan
        constexpr int kPer = (kMaxD + kR2Threads - 1) / kR2Threads;
        int tot[kPer];
        int sum = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int d = t * kPer + k;
            int c = 0;
            if (d < D) {
#pragma unroll
                for (int q = 0; q < kW; ++q) {
                    const int v = wcnt[q][d];
                    wcnt[q][d] = c;  // this wave's start within digit d
                    c += v;
                }
            }
            tot[k] = c;
            sum += c;
        }
        const int inc = wave_incl_scan(sum);
        if (lane == 63) wtot[w] = inc;
        __syncthreads();
        int ex = inc - sum;
        for (int q = 0; q < w; ++q) ex += wtot[q];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int d = t * kPer + k;
            if (d < D) {
                lstart[d] = ex;
#pragma unroll
                for (int q = 0; q < kW; ++q) wcnt[q][d] += ex;  // absolute tile position
            }
            ex += tot[k];
        }
        __syncthreads();
        if constexpr (kSeg == kSegBuckets) {
            if (pA) {  // rows from the packed pass-A words: segment (cursor walk) + offset
#pragma unroll
                for (int j = 0; j < kB; ++j) {
                    const long long gi = cbase + min(w * kQ + j * 64 + lane, valid - 1);
                    int sgi = scur;
                    while (gi >= s_segstart[sgi + 1]) ++sgi;
                    rr[j] = s_segrow[sgi] + (int)((unsigned)kk[j] >> packA);
                    scur = __builtin_amdgcn_readlane(sgi, 63);
                }
            }
        }
        // 3. stage in digit order
#pragma unroll
        for (int j = 0; j < kB; ++j) {
            if (w * kQ + j * 64 + lane < valid) {
                const int pos = wcnt[w][(kk[j] >> shift) & dm] + lp[j];
                skey[pos] = kk[j];
                if constexpr (!kPkF) srow[pos] = rowof(j);
                sval[pos] = vv[j];
            }
        }
        __syncthreads();
        // 4. prefetch the next tile, write this one out as per-digit runs
        if (nvalid > 0) load_tile(nbase, nvalid);
        for (int li = t; li < valid; li += kR2Threads) {
            const int k = skey[li];
            const int d = (k >> shift) & dm;
            const long long g = (long long)gbase[d] + (li - lstart[d]);
            if (kSeg == kSegTiles && kDerive && pA) {  // pass A -> pass B: low key bits + row offset
                kout[g] = (int)(((unsigned)k & kbmask) | ((unsigned)(srow[li] - segrow0) << packA));
            } else if (!kFinal && pack >= 0) {  // pass B -> last pass: row and the low `pack` bits in one word
                kout[g] = (srow[li] << pack) | (k & ((1 << pack) - 1));
            } else {
                if (kout) kout[g] = colkey(k);
                if constexpr (kPkF) rout[g] = (int)((unsigned)k >> pack);
                else rout[g] = srow[li];
            }
            vout[g] = sval[li];
        }
        __syncthreads();
        // 5. the next tile appends after this one; counters restart
        for (int d = t; d < D; d += kR2Threads) {
            const int nxt = d < dm ? lstart[d + 1] : valid;
            gbase[d] += nxt - lstart[d];
#pragma unroll
            for (int q = 0; q < kW; ++q) wcnt[q][d] = 0;
        }
        if constexpr (kDerive) derive_init();
        __syncthreads();
    };
    long long base = s0;
    int valid = base < s1 ? (int)min((long long)kTile, s1 - base) : 0;
    if (valid > 0) load_tile(base, valid);
    if constexpr (kFinal) {
        // buckets bk = blockIdx.x, + gridDim.x, ...; each: its own digit
        // histogram -> exclusive starts -> colptr for its 2^rb columns, then
        // its tiles; the next bucket's first tile is loaded while the last
        // tile of this one is written.  A one-tile bucket counts from the
        // registers of its tile, a longer one reads its keys first.
        static_assert(kMaxD <= kR2Threads, "one digit per thread");
        if (blockIdx.x == 0 && t == 0) colptr[n] = (int)nnz;
        while (bk < sg.nb) {
            if (t < D) gbase[t] = 0;
            __syncthreads();
            if (s1 - s0 <= kTile) {
#pragma unroll
                for (int j = 0; j < kB; ++j)
                    if (w * kQ + j * 64 + lane < valid) atomicAdd(&gbase[(kk[j] >> shift) & dm], 1);
            } else {
                constexpr int kU = 8;
                for (long long i0 = s0; i0 < s1; i0 += (long long)kU * kR2Threads) {
                    int d[kU];
#pragma unroll
                    for (int u = 0; u < kU; ++u) {
                        const long long i = i0 + (long long)u * kR2Threads + t;
                        d[u] = i < s1 ? ((kin[i] >> shift) & dm) : -1;
                    }
#pragma unroll
                    for (int u = 0; u < kU; ++u)
                        if (d[u] >= 0) atomicAdd(&gbase[d[u]], 1);
                }
            }
            __syncthreads();
            {
                const int c = t < D ? gbase[t] : 0;
                const int inc = wave_incl_scan(c);
                if (lane == 63) wtot[w] = inc;
                __syncthreads();
                int ex = inc - c;
                for (int q = 0; q < w; ++q) ex += wtot[q];
                if (t < D) {
                    gbase[t] = (int)s0 + ex;
                    const long long col = ((long long)bk << rb) + t;
                    if (col < n) colptr[col] = (int)s0 + ex;
#pragma unroll
                    for (int q = 0; q < kW; ++q) wcnt[q][t] = 0;
                }
                __syncthreads();
            }
            for (;;) {  // the bucket's tiles (all values workgroup-uniform)
                long long nbase = 0, ns0 = s0, ns1 = s1;
                int nvalid = 0, nbk = bk;
                if (base + kTile < s1) {
                    nbase = base + kTile;
                    nvalid = (int)min((long long)kTile, s1 - nbase);
                } else {
                    nbk = bk + (int)gridDim.x;
                    if (nbk < sg.nb) {
                        seg_range(kSegBuckets, sg, nbk, nnz, ns0, ns1);
                        nbase = ns0;
                        nvalid = (int)min((long long)kTile, ns1 - ns0);
                    }
                }
                if (valid > 0) process_tile(valid, nbase, nvalid, base);
                else if (nvalid > 0) load_tile(nbase, nvalid);
                base = nbase;
                valid = nvalid;
                if (nbk != bk) {
                    bk = nbk;
                    s0 = ns0;
                    s1 = ns1;
                    break;
                }
            }
        }
    } else {
        for (int d = t; d < D; d += kR2Threads) {
            const size_t idx = seg_count_idx(kSeg, sg, (int)blockIdx.x, D, d);
            gbase[d] = idx ? incl[idx - 1] : 0;  // exclusive start of this workgroup's run of d
#pragma unroll
            for (int q = 0; q < kW; ++q) wcnt[q][d] = 0;
        }
        if constexpr (kDerive) {
            if (valid > 0) {
                rc = wgrow[blockIdx.x];
                segrow0 = rc;
                wv = rowptr[min(rc + 1 + t, m)];
                derive_init();
            }
        }
        if constexpr (kSeg == kSegBuckets) {
            if (pA) {  // the segments' runs inside this bucket, and their first rows
                const long long i0 = (long long)(blockIdx.x / sg.J) * nseg;
                for (int i = t; i < nseg; i += kR2Threads) {
                    s_segstart[i] = (i0 + i) ? sg.prev[i0 + i - 1] : 0;
                    s_segrow[i] = wgrow[i];
                }
                if (t == 0) s_segstart[nseg] = INT_MAX;
            }
        }
        __syncthreads();
        if constexpr (kSeg == kSegBuckets) {
            if (pA && valid > 0) {  // this wave's first entry: largest i with s_segstart[i] <= p
                const long long p = min(s0 + (long long)w * kQ, s1 - 1);
                int lo = 0, hi = nseg - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_segstart[mid] <= p) lo = mid;
                    else hi = mid - 1;
                }
                scur = lo;
            }
        }
        while (valid > 0) {  // valid: workgroup-uniform
            const long long nbase = base + kTile;
            const int nvalid = nbase < s1 ? (int)min((long long)kTile, s1 - nbase) : 0;
            process_tile(valid, nbase, nvalid, base);
            base = nbase;
            valid = nvalid;
        }
    }
}

// colptr from the sorted keys: colptr[c] = first position whose key >= c
__global__ void k_colptr_sorted(const int *__restrict__ keys, long long nnz, int n, int *__restrict__ colptr)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int k = keys[p];
    const int prev = p == 0 ? -1 : keys[p - 1];
    for (int c = prev + 1; c <= k; ++c) colptr[c] = (int)p;
    if (p == nnz - 1)
        for (int c = k + 1; c <= n; ++c) colptr[c] = (int)nnz;
}

struct TransposeScratch {
    void *buf = nullptr;
    size_t bytes = 0;
};
static thread_local TransposeScratch g_tscratch[64];

// What launch_transpose runs for an m x n matrix of nnz > 0 entries on a
// device of ncu CUs: the form and every launch shape.
// MSD: two stable partition passes on the high column bits (pass A, bA bits,
// over the whole array in fixed tile segments; pass B, bB bits, inside each
// pass-A bucket), then one pass per final bucket of 2^c columns that counts,
// ranks and writes the bucket's run in column order together with its colptr
// entries.  Every pass is a stable partition, so the composition is the
// stable sort by column (rows ascend in a column).  Writes: passes A and B
// append per-digit runs (few partially written lines per workgroup); the last
// pass writes one contiguous run per workgroup and no keys (unless colidx is
// asked for).
// LSD: `passes` passes of rb-bit digits over the same tile segments, rows
// from an expanded row array, colptr read off the sorted keys.
struct TransposeShape {
    bool msd = false;
    int c = 0, bA = 0, bB = 0;  // MSD: digit bits of the last pass, pass A, pass B
    int passes = 0, rb = 0;     // LSD: passes and their digit bits
    int ntiles = 0;             // kRxTile-entry tiles of the input
    int S = 0, nwg = 0;         // tile segments (pass A, LSD passes): tiles per workgroup, workgroups
    int JB = 0, nwgB = 0;       // MSD pass B: parts per pass-A bucket, workgroups
    // MSD: key bits of the one word pass A may hand pass B (-1: never; else
    // the device decides from the segments' row spans), and of the one word
    // pass B hands the last pass (-1: keys and rows travel apart)
    int packA = -1, pack = -1;
    int nbC = 0;                // MSD: final buckets
    int ftile = 0;              // MSD: entries of a last-pass tile, 3072 or 4096
    bool lean = false;          // MSD: last pass without row staging
    int fgrid = 0;              // MSD: workgroups of the last pass
    long long ncntA = 0, ncntB = 0, ncnt = 0;  // counts: pass A, pass B, all (LSD: one pass)
};

static TransposeShape transpose_shape(int m, int n, long long nnz, int ncu)
{
    TransposeShape T;
    int nbits = 0;
    while (nbits < 31 && (n - 1) >> nbits) ++nbits;
    // final buckets of 2^c columns: the widest whose average fits one
    // 4096-entry tile with room for the spread (<= 3072 entries), so most
    // final workgroups count from the registers of their only tile
    int c = std::min(8, nbits);
    while (c > 1 && nnz / std::max<long long>(1, ((long long)n + (1LL << c) - 1) >> c) > 3072) --c;
    const int high = nbits - c;
    const int bA = (high + 1) / 2;
    const int bB = high - bA;
    // MSD where both high passes exist (n > 2^9) with digits of at most 8
    // bits (n <= 2^24), else the LSD passes
    T.msd = bA >= 1 && bB >= 1 && bA <= kRxMaxBits && bB <= kRxMaxBits;
    // LSD: digits of at most kRxMaxBits bits, spread evenly over the passes
    const int passes = std::max(1, (nbits + kRxMaxBits - 1) / kRxMaxBits);
    const int rb = std::max(1, (nbits + passes - 1) / passes);
    T.ntiles = (int)((nnz + kRxTile - 1) / kRxTile);
    // tiles per workgroup: one round of resident workgroups
    T.S = std::max(1, (T.ntiles + ncu * kRxWgPerCu - 1) / (ncu * kRxWgPerCu));
    T.nwg = (T.ntiles + T.S - 1) / T.S;
    if (!T.msd) {
        T.passes = passes;
        T.rb = rb;
        T.ncnt = (long long)(1 << rb) * T.nwg;
        return T;
    }
    T.c = c;
    T.bA = bA;
    T.bB = bB;
    // pass B: J parts per pass-A bucket, about two workgroups per CU
    T.JB = std::max(1, (ncu * kRxWgPerCu) >> bA);
    T.ncntA = (long long)(1 << bA) * T.nwg;
    T.ncntB = (long long)(1 << (bA + bB)) * T.JB;
    T.ncnt = T.ncntA + T.ncntB;
    // pass A -> pass B in one word per key (low bB + c bits + row offset in
    // the segment) when the segments' row spans allow; decided on the
    // device from the spans the count pass wrote.
    T.packA = (T.nwg <= 512 && bB + c <= 24) ? bB + c : -1;
    // pass B's output keeps (row << c | low c column bits) in one word when
    // they fit (the last pass needs nothing else of the key): 12 B per
    // entry written and read instead of 16.
    int mbits = 0;
    while (mbits < 31 && (m - 1) >> mbits) ++mbits;
    T.pack = mbits + c <= 31 ? c : -1;
    T.nwgB = (1 << bA) * T.JB;
    // last pass: one workgroup per pass-B bucket (2^c columns)
    T.nbC = 1 << (bA + bB);
    // final tile: 3072 entries (6 per thread) when the buckets average <=
    // 2600 -- uniform columns then fit one tile (spread ~ sqrt(avg)) with
    // 83% of its lanes busy instead of 62% in a 4096 tile; fuller buckets
    // keep the 4096 tile
    const long long favg = nnz / std::max(1, T.nbC);
    T.ftile = favg <= 2600 ? 3072 : 4096;
    // lean last pass (packed input, <= 7 final bits, 3072 tile): no row
    // staging and 128-digit tables leave 42 KB of LDS, and 80 VGPRs, so
    // three workgroups share a CU (config 2: 332 -> 290 us).
    T.lean = T.pack >= 0 && c <= 7 && T.ftile == 3072;
    T.fgrid = std::min(T.nbC, ncu * (T.lean ? 3 : kRxWgPerCu));
    return T;
}

int launch_transpose(const sblas_csr_s &A, int *colptr, int *rowidx, double *cval, hipStream_t s,
                     int *colidx)
{
    const long long nnz = A.nnz;
    const int n = A.n, m = A.m;
    if (nnz == 0) {
        SBLAS_HIP(hipMemsetAsync(colptr, 0, sizeof(int) * ((size_t)n + 1), s));
        return SBLAS_OK;
    }
    int ncu = 256;
    {
        int dev = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    }
    const TransposeShape T = transpose_shape(m, n, nnz, ncu);
    const int nwg = T.nwg;
    // scratch: keysA rowsA valsA | keysB rowsB valsB | counts | scan (+ outputs when null)
    const size_t scan_ints = scan_scratch_len(T.ncnt);
    const size_t z = ((size_t)nnz + 3) & ~(size_t)3;  // array stride: every array 16-B aligned
    const size_t wg_ints = ((size_t)2 * nwg + 67) & ~(size_t)3;  // MSD: segment first rows + spans
    const size_t need = z * 32 + (size_t)T.ncnt * 4 + scan_ints * 4 + wg_ints * 4 + (rowidx ? 0 : z * 4) +
                        (cval ? 0 : z * 8) + 256;
    TransposeScratch &S = g_tscratch[A.device & 63];
    if (S.bytes < need) {
        if (S.buf) SBLAS_HIP(hipStreamSynchronize(s));  // earlier work on s may still use it
        (void)hipFree(S.buf);
        S.buf = nullptr;
        S.bytes = 0;
        SBLAS_HIP(hipMalloc(&S.buf, need));
        S.bytes = need;
    }
    char *p = (char *)S.buf;
    double *valsA = (double *)p;
    double *valsB = valsA + z;
    int *keysA = (int *)(valsB + z);
    int *rowsA = keysA + z;
    int *keysB = rowsA + z;
    int *rowsB = keysB + z;
    int *counts = rowsB + z;
    int *scan = counts + T.ncnt;
    int *wgrow = scan + scan_ints;
    int *rout_final = rowidx ? rowidx : wgrow + wg_ints;
    double *vout_final = cval ? cval : (double *)(((uintptr_t)(rout_final + (rowidx ? 0 : z)) + 7) & ~(uintptr_t)7);
    const SegArgs gt{T.S, nwg, nullptr, 1, 1};  // the tile segments of pass A and the LSD passes
    if (T.msd) {
        int *cntA = counts, *cntB = counts + T.ncntA;
        // pass A: the top bA bits, fixed tile segments, rows derived from
        // rowptr, (col, row, val) -> set A
        const int shA = T.c + T.bB;
        hipLaunchKernelGGL(k_rx2_count<kSegTiles>, dim3((unsigned)nwg), dim3(kCntThreads), 0, s,
                           A.col, nnz, shA, T.bA, gt, cntA, A.rowptr, m, wgrow);
        SBLAS_TRY(scan_inclusive(cntA, T.ncntA, scan, s));
        hipLaunchKernelGGL((k_rx2_scatter<256, kSegTiles, true>), dim3(nwg), dim3(kR2Threads), 0, s,
                           A.col, nullptr, A.val, nnz, shA, T.bA, gt, cntA, keysA, rowsA, valsA, nullptr, n, -1,
                           A.rowptr, m, wgrow, T.packA);
        // pass B: the next bB bits inside each pass-A bucket, set A -> set B
        const SegArgs gB{0, 0, cntA, nwg, T.JB};
        hipLaunchKernelGGL(k_rx2_count<kSegBuckets>, dim3((unsigned)T.nwgB), dim3(kCntThreads), 0,
                           s, keysA, nnz, T.c, T.bB, gB, cntB);
        SBLAS_TRY(scan_inclusive(cntB, T.ncntB, scan, s));
        // 128 digits: smaller count tables leave LDS for the segment tables
        auto kpb = T.bB <= 7 ? k_rx2_scatter<128, kSegBuckets> : k_rx2_scatter<256, kSegBuckets>;
        hipLaunchKernelGGL(kpb, dim3(T.nwgB), dim3(kR2Threads), 0, s, keysA, rowsA, valsA, nnz, T.c, T.bB, gB,
                           cntB, keysB, rowsB, valsB, nullptr, n, T.pack, nullptr, 0, wgrow, T.packA);
        // last pass: set B -> CSC + colptr
        const SegArgs gC{0, 0, cntB, T.JB, 1, T.nbC};
        auto kfin = T.lean           ? k_rx2_scatter<128, kSegFinal, false, 3072, true, 6>
                    : T.ftile == 3072 ? k_rx2_scatter<256, kSegFinal, false, 3072>
                                      : k_rx2_scatter<256, kSegFinal>;
        hipLaunchKernelGGL(kfin, dim3((unsigned)T.fgrid), dim3(kR2Threads), 0, s,
                           keysB, T.pack >= 0 ? nullptr : rowsB, valsB, nnz, 0, T.c, gC, nullptr, colidx, rout_final,
                           vout_final, colptr, n, T.pack, nullptr, 0, nullptr, -1);
        SBLAS_HIP(hipGetLastError());
        return SBLAS_OK;
    }
    hipLaunchKernelGGL(k_expand_rows, dim3((m + 255) / 256), dim3(256), 0, s, A.rowptr, m, rowsB);
    const int *kin = A.col, *rin = rowsB;
    const double *vin = A.val;
    for (int ps = 0; ps < T.passes; ++ps) {
        const bool last = ps == T.passes - 1;
        // pass ps reads set (ps even: input/B, odd: A) and writes the other
        int *ko = (ps & 1) ? keysB : keysA;
        int *ro = last ? rout_final : ((ps & 1) ? rowsB : rowsA);
        double *vo = last ? vout_final : ((ps & 1) ? valsB : valsA);
        const int sh = T.rb * ps;
        hipLaunchKernelGGL(k_rx2_count<kSegTiles>, dim3((unsigned)nwg), dim3(kCntThreads), 0, s,
                           kin, nnz, sh, T.rb, gt, counts);
        SBLAS_TRY(scan_inclusive(counts, T.ncnt, scan, s));
        hipLaunchKernelGGL((k_rx2_scatter<256, kSegTiles>), dim3(nwg), dim3(kR2Threads), 0, s, kin, rin, vin,
                           nnz, sh, T.rb, gt, counts, ko, ro, vo, nullptr, n, -1);
        kin = ko;
        rin = ro;
        vin = vo;
    }
    hipLaunchKernelGGL(k_colptr_sorted, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, kin, nnz, n,
                       colptr);
    if (colidx)  // column of every CSC entry (the sorted keys)
        SBLAS_HIP(hipMemcpyAsync(colidx, kin, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

}  // namespace sblas

extern "C" int sblas_transpose_shape_host(int m, int n, long long nnz, int ncu, long long *info)
{
    using namespace sblas;
    if (m < 0 || n < 0 || nnz < 0 || nnz > INT_MAX || ncu < 1 || !info) return SBLAS_ERR_INVALID;
    const TransposeShape T = transpose_shape(m, n, nnz, ncu);
    const long long v[18] = {T.msd ? 1 : 0, T.c, T.bA,    T.bB, T.passes, T.rb,    T.ntiles,        T.S,     T.nwg,
                             T.JB,          T.nwgB, T.packA, T.pack, T.nbC,  T.ftile, T.lean ? 1 : 0, T.fgrid, T.ncnt};
    for (int i = 0; i < 18; ++i) info[i] = v[i];
    return SBLAS_OK;
}
