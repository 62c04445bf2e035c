// xsort_layout.hip -- the layout (inspector) of the xsort SpMV (algo 5): the
// chunk storage of a plan, built on the device (xs_layout_device) or, as its
// byte-identical reference and fallback, on the host (xs_layout_host).  The
// storage format is described at the top of xsort.hip; the ranges come from
// the planner (xsort_plan.cpp).
#include <algorithm>
#include <memory>
#include <utility>
#include <vector>

#include "sblas_internal.hpp"
#include "scan.hpp"

namespace sblas {

// Both builders produce the same bytes: blk[] (I*G + 1 chunk offsets) and the
// chunk storage.  ranges[] come from the planner (xs_plan_host); G and Wg are
// read from the handle's plan.
static const char *const kXsBadMsg = "xsort: column index out of [0, n) or key overflow";

// Host build (the reference form; test hook "xs_hostplan", and the fallback
// when the device build's scratch does not fit): copies col / val to the
// host, buckets and stable-sorts every block under OpenMP, fills hbuf.
int xs_layout_host(sblas_csr_s &A, const std::vector<XsRange> &ranges, int rows_cap, int nrows_cap,
                   std::vector<long long> &blk, std::unique_ptr<unsigned char[]> &hbuf)
{
    XsPlan &P = A.xs;
    const int n = A.n, G = P.G, Wg = P.Wg, I = (int)ranges.size();
    const long long nnz = A.nnz;
    const long long wmax = (1LL << kXsColBits) - 1;
    const std::vector<int> &rp = A.h_rowptr;
    // host copies of the CSR entries (uninitialised: the copies fill them)
    std::unique_ptr<int[]> hcol(new int[(size_t)std::max<long long>(nnz, 1)]);
    std::unique_ptr<double[]> hval(new double[(size_t)std::max<long long>(nnz, 1)]);
    if (nnz) {
        SBLAS_HIP(hipMemcpy(hcol.get(), A.col, sizeof(int) * nnz, hipMemcpyDeviceToHost));
        SBLAS_HIP(hipMemcpy(hval.get(), A.val, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        P.d2h_bytes += (long long)(sizeof(int) + sizeof(double)) * nnz;
    }

    // pass 1: every block (range, group) bucketed and sorted by (column, row)
    // once, kept for the fill.  One range per task for the bucketing (a wide
    // range holds ~13x a narrow one's entries, and they sit together at the
    // heavy rows), then the blocks are sorted as tasks of their own.
    const size_t nblk = (size_t)I * G;
    std::vector<std::vector<std::pair<uint32_t, double>>> bk(nblk);
    bool bad = false;
#pragma omp parallel for schedule(dynamic, 1) reduction(|| : bad)
    for (int i = 0; i < I; ++i) {
        const XsRange &R = ranges[i];
        std::vector<int> cnt(G, 0);
        for (int e = rp[R.row0]; e < rp[R.row0 + R.nrows]; ++e) {
            const int c = hcol[e];
            if (c >= 0 && c < n) ++cnt[c / Wg];
        }
        for (int g = 0; g < G; ++g) bk[(size_t)i * G + g].reserve(cnt[g]);
        for (int r = R.row0; r < R.row0 + R.nrows; ++r) {
            for (int e = rp[r]; e < rp[r + 1]; ++e) {
                const int c = hcol[e];
                if (c < 0 || c >= n) {
                    bad = true;
                    continue;
                }
                const int g = c / Wg;
                const uint32_t cp = (uint32_t)(c - g * Wg), lr = (uint32_t)(r - R.row0);
                if ((long long)cp >= wmax || lr >= (uint32_t)(R.wide ? rows_cap : nrows_cap)) bad = true;
                bk[(size_t)i * G + g].push_back({(cp << kXsRowBits) | lr, hval[e]});
            }
        }
    }
#pragma omp parallel for schedule(dynamic, 4)
    for (long long k = 0; k < (long long)nblk; ++k) {
        auto &bb = bk[(size_t)k];
        std::stable_sort(bb.begin(), bb.end(),
                         [](const std::pair<uint32_t, double> &u, const std::pair<uint32_t, double> &v) {
                             return u.first < v.first;
                         });
    }
    if (bad) {
        set_error("%s", kXsBadMsg);
        return SBLAS_ERR_INVALID;
    }
    blk.assign(nblk + 1, 0);
    for (size_t k = 0; k < nblk; ++k)
        blk[k + 1] = blk[k] + ((long long)bk[k].size() + kXsChunk - 1) / kXsChunk;
    const long long nchunks = blk.back();

    // pass 2: fill every chunk (lane-transposed, header comment).  Every byte
    // of every chunk is written by the fill below: no zeroing pass.
    const size_t cbytes = kXsChunkBytes;
    const size_t hb_n = (size_t)std::max<long long>(nchunks, 1) * cbytes;
    hbuf.reset(new unsigned char[hb_n]);
    auto chunk_keys = [&](long long c) { return (uint32_t *)(hbuf.get() + (size_t)c * cbytes); };
    auto chunk_vals = [&](long long c) {
        return (double *)(hbuf.get() + (size_t)c * cbytes + kXsChunk * sizeof(uint32_t));
    };
#pragma omp parallel for schedule(dynamic, 64)
    for (long long k = 0; k < (long long)nblk; ++k) {
        const auto &bb = bk[(size_t)k];
        const long long c0 = blk[(size_t)k], c1 = blk[(size_t)k + 1];
        for (long long c = c0; c < c1; ++c) {
            uint32_t *kc = chunk_keys(c);
            double *vc = chunk_vals(c);
            for (int p = 0; p < kXsChunk; ++p) {
                const long long src = (c - c0) * kXsChunk + p;
                const bool in = src < (long long)bb.size();
                const int l = p & 63, j = p >> 6;
                kc[4 * l + j] = in ? bb[src].first : kXsPad;
                vc[(j < 2 ? 0 : 128) + 2 * l + (j & 1)] = in ? bb[src].second : 0.0;
            }
        }
    }
    return SBLAS_OK;
}

// Device build.  A range's entries are a contiguous span of the CSR arrays in
// (row, position) order, and block (i, g) is that span's entries of group g
// stably sorted by group-local column: the whole layout is ONE stable sort of
// the entries, taken in CSR order, by (block id i*G + g, local column).  It
// runs as an LSD radix sort of 64-bit sort words
//     block id << 32 | local column << 14 | local row
// (the low 32 bits ARE the entry's packed key) that carry the entry's CSR
// position, over the digits of (block id, local column) only:
//   k_xsd_keys     a wave per 64 rows: every entry's sort word and position;
//                  raises the `bad` flag (column outside [0, n), key overflow)
//                  -- such an entry is only counted (word 0), its column never
//                  becomes an address;
//   per digit      k_xsd_count (tile histograms in LDS, stored plainly
//                  [digit][tile]), scan_inclusive, k_xsd_scatter (stable
//                  in-tile ranking by wave ballots, the tile staged in LDS in
//                  digit order, written as per-digit runs).  No global atomic
//                  decides a place, so the order is the same on every run;
//   k_xsd_bounds   the blocks' entry offsets, read off the sorted words;
//   k_xsd_chunks / scan / k_xsd_blk   blk[] in chunks (+ the bad flag), the
//                  one array copied to the host -- the build's only wait;
//   k_xsd_fill     a workgroup per chunk: gathers the values by position and
//                  writes the chunk lane-transposed, padding included.
// Any block size takes the same path (a block is just a run of the sorted
// words).  Scratch: two (word, position) buffers of 12 B per entry plus the
// digit counts, freed before returning.
constexpr int kXdThreads = 256;
constexpr int kXdWaves = kXdThreads / 64;
constexpr int kXdItems = 16;
constexpr int kXdTile = kXdThreads * kXdItems;  // entries per radix tile
constexpr int kXdMaxBits = 8;                   // digit bits: one digit per thread
static_assert(kXdThreads == 1 << kXdMaxBits, "one digit per thread");
typedef unsigned long long xsw_t;

struct XsDevRange {
    int row0;
    int lim;  // rows the range's keys may address
};

// the sorted part of a word: block id above the local column's cpb bits
__device__ __forceinline__ unsigned long long xsd_sortbits(xsw_t w, int cpb)
{
    return ((w >> 32) << cpb) | ((w >> kXsRowBits) & ((1u << kXsColBits) - 1));
}

__global__ __launch_bounds__(256) void k_xsd_keys(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                  int m, int n, const XsDevRange *__restrict__ rng, int I,
                                                  int G, int Wg, xsw_t *__restrict__ words,
                                                  int *__restrict__ pos, int *__restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const int r0 = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 64;
    if (r0 >= m) return;
    const int nrow = min(64, m - r0);
    const int b = rowptr[min(r0 + lane, m)];
    const int last = rowptr[r0 + nrow];
    // this lane's row's range: the largest i with rng[i].row0 <= row
    const int myrow = min(r0 + lane, m - 1);
    int lo = 0, hi = I - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (rng[mid].row0 <= myrow) lo = mid;
        else hi = mid - 1;
    }
    const XsDevRange mine = rng[lo];
    for (int j = 0; j < nrow; ++j) {
        const int s = __builtin_amdgcn_readlane(b, j);
        const int e = j + 1 < nrow ? __builtin_amdgcn_readlane(b, j + 1) : last;
        const int i = __builtin_amdgcn_readlane(lo, j);
        const int row0 = __builtin_amdgcn_readlane(mine.row0, j);
        const int lim = __builtin_amdgcn_readlane(mine.lim, j);
        const unsigned lr = (unsigned)(r0 + j - row0);
        for (int k = s + lane; k < e; k += 64) {
            const int c = col[k];
            xsw_t w = 0;
            bool ok = c >= 0 && c < n;
            if (ok) {
                const int g = c / Wg;
                const unsigned cp = (unsigned)(c - g * Wg);
                ok = cp < (1u << kXsColBits) - 1 && lr < (unsigned)lim && g < G;
                w = ((xsw_t)((unsigned)i * (unsigned)G + (unsigned)g) << 32) | ((xsw_t)cp << kXsRowBits) | lr;
            }
            if (!ok) {
                w = 0;
                *bad = 1;
            }
            words[k] = w;
            pos[k] = k;
        }
    }
}

__global__ __launch_bounds__(kXdThreads) void k_xsd_count(const xsw_t *__restrict__ words, long long nnz,
                                                          int shift, int rb, int cpb, int ntiles,
                                                          int *__restrict__ counts)
{
    __shared__ int h[1 << kXdMaxBits];
    const int t = threadIdx.x, dm = (1 << rb) - 1;
    h[t] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kXdTile;
#pragma unroll
    for (int j = 0; j < kXdItems; ++j) {
        const long long i = base + j * kXdThreads + t;
        if (i < nnz) atomicAdd(&h[(int)(xsd_sortbits(words[i], cpb) >> shift) & dm], 1);
    }
    __syncthreads();
    if (t <= dm) counts[(size_t)t * ntiles + blockIdx.x] = h[t];
}

// One tile per workgroup.  Wave w ranks the contiguous quarter [w*1024,
// (w+1)*1024) of the tile in 16 batches of 64 with wave-private digit
// counters (a wave's LDS operations retire in program order): rank = the
// wave's count so far + the in-batch rank from rb ballots.  The per-wave
// counts then become the tile's digit offsets, the tile is staged in LDS in
// digit order (stable: wave order, then batch order, then lane order = tile
// order) and written out as per-digit runs from incl[] (the inclusive scan
// of the [digit][tile] counts).
__global__ __launch_bounds__(kXdThreads) void k_xsd_scatter(const xsw_t *__restrict__ win,
                                                            const int *__restrict__ pin, long long nnz,
                                                            int shift, int rb, int cpb, int ntiles,
                                                            const int *__restrict__ incl,
                                                            xsw_t *__restrict__ wout, int *__restrict__ pout)
{
    __shared__ int wcnt[kXdWaves][1 << kXdMaxBits];
    __shared__ int lstart[1 << kXdMaxBits], gbase[1 << kXdMaxBits], wtot[kXdWaves];
    __shared__ xsw_t sword[kXdTile];
    __shared__ int spos[kXdTile];
    constexpr int kQ = kXdTile / kXdWaves;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int D = 1 << rb, dm = D - 1;
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int q = 0; q < kXdWaves; ++q) wcnt[q][t] = 0;
    const long long base = (long long)blockIdx.x * kXdTile;
    const int valid = (int)min((long long)kXdTile, nnz - base);
    xsw_t ww[kXdItems];
    int pp[kXdItems], lp[kXdItems], dd[kXdItems];
#pragma unroll
    for (int j = 0; j < kXdItems; ++j) {
        const int li = w * kQ + j * 64 + lane;
        const bool ok = li < valid;
        ww[j] = ok ? win[base + li] : 0;
        pp[j] = ok ? pin[base + li] : 0;
        dd[j] = (int)(xsd_sortbits(ww[j], cpb) >> shift) & dm;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kXdItems; ++j) {
        const bool ok = w * kQ + j * 64 + lane < valid;
        const int d = dd[j];
        unsigned long long mm = __ballot(ok);
        for (int b = 0; b < rb; ++b) {
            const unsigned long long bal = __ballot((d >> b) & 1);
            mm &= ((d >> b) & 1) ? bal : ~bal;
        }
        const int rank = __popcll(mm & lt);
        const int sofar = wcnt[w][d];
        lp[j] = sofar + rank;
        if (ok && rank == 0) wcnt[w][d] = sofar + __popcll(mm);
    }
    __syncthreads();
    // digit t: the waves' starts inside the digit, then the tile's digit offsets
    int c = 0;
    if (t < D) {
#pragma unroll
        for (int q = 0; q < kXdWaves; ++q) {
            const int v = wcnt[q][t];
            wcnt[q][t] = c;
            c += v;
        }
    }
    const int inc = wave_incl_scan(c);
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    int ex = inc - c;
    for (int q = 0; q < w; ++q) ex += wtot[q];
    lstart[t] = ex;
    gbase[t] = t < D ? incl[(size_t)t * ntiles + blockIdx.x] - c : 0;  // inclusive scan -> this tile's start
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kXdItems; ++j) {
        if (w * kQ + j * 64 + lane < valid) {
            const int p = lstart[dd[j]] + wcnt[w][dd[j]] + lp[j];
            sword[p] = ww[j];
            spos[p] = pp[j];
        }
    }
    __syncthreads();
    for (int li = t; li < valid; li += kXdThreads) {
        const xsw_t k = sword[li];
        const int d = (int)(xsd_sortbits(k, cpb) >> shift) & dm;
        const long long g = (long long)gbase[d] + (li - lstart[d]);
        if (g >= 0 && g < nnz) {  // always: the counts are this pass's own
            wout[g] = k;
            pout[g] = spos[li];
        }
    }
}

// start[k] = first sorted entry of block k (start[nblk] = nnz): the entry that
// opens a new block id writes the starts of every block since the last one.
__global__ __launch_bounds__(256) void k_xsd_bounds(const xsw_t *__restrict__ words, long long nnz,
                                                    long long nblk, int *__restrict__ start)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const long long b = min((long long)(words[p] >> 32), nblk - 1);
    const long long pb = p ? min((long long)(words[p - 1] >> 32), nblk - 1) : -1;
    for (long long k = pb + 1; k <= b; ++k) start[k] = (int)p;
    if (p == nnz - 1)
        for (long long k = b + 1; k <= nblk; ++k) start[k] = (int)nnz;
}

__global__ __launch_bounds__(256) void k_xsd_chunks(const int *__restrict__ start, long long nblk,
                                                    int *__restrict__ cnt)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < nblk) cnt[k] = (start[k + 1] - start[k] + kXsChunk - 1) / kXsChunk;
}

// blk[0] = 0, blk[k + 1] = chunks of blocks 0..k, blk[nblk + 1] = the bad flag
__global__ __launch_bounds__(256) void k_xsd_blk(const int *__restrict__ incl, long long nblk,
                                                 const int *__restrict__ bad, long long *__restrict__ blk)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < nblk) blk[k + 1] = incl[k];
    if (k == 0) {
        blk[0] = 0;
        blk[nblk + 1] = *bad;
    }
}

// One chunk per workgroup: thread p takes the chunk's entry p (a padding
// entry past the block's end), the chunk is transposed through LDS and stored
// whole: keys at 4*l + j, values at (j < 2 ? 0 : 128) + 2*l + (j & 1) for
// l = p & 63, j = p >> 6.
__global__ __launch_bounds__(kXsChunk) void k_xsd_fill(const xsw_t *__restrict__ words,
                                                       const int *__restrict__ pos,
                                                       const double *__restrict__ val, long long nnz,
                                                       const int *__restrict__ start,
                                                       const long long *__restrict__ blk, long long nblk,
                                                       unsigned char *__restrict__ out)
{
    __shared__ uint32_t sk[kXsChunk];
    __shared__ double sv[kXsChunk];
    const long long c = blockIdx.x;
    // the chunk's block: blk[k] <= c < blk[k + 1] (blk[0] = 0, blk[nblk] > c)
    long long lo = 1, hi = nblk;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (blk[mid] > c) hi = mid;
        else lo = mid + 1;
    }
    const long long k = lo - 1;
    const int p = threadIdx.x;
    const long long src = (long long)start[k] + (c - blk[k]) * kXsChunk + p;
    const bool in = src >= 0 && src < (long long)start[k + 1] && src < nnz;
    uint32_t key = kXsPad;
    double v = 0.0;
    if (in) {
        key = (uint32_t)words[src];
        const int e = pos[src];
        v = (e >= 0 && e < nnz) ? val[e] : 0.0;  // always in range: a permutation of the positions
    }
    const int l = p & 63, j = p >> 6;
    sk[4 * l + j] = key;
    sv[(j < 2 ? 0 : 128) + 2 * l + (j & 1)] = v;
    __syncthreads();
    unsigned char *oc = out + (size_t)c * kXsChunkBytes;
    reinterpret_cast<uint32_t *>(oc)[p] = sk[p];
    reinterpret_cast<double *>(oc + kXsChunk * sizeof(uint32_t))[p] = sv[p];
}

namespace {
// the device build's temporaries: freed together, whatever way it returns
struct XsScratch {
    std::vector<void *> ptrs;
    long long bytes = 0;
    bool deny = false;  // test hook "xs_devplan_nomem": the second allocation fails
    template <class T>
    bool take(T **p, size_t count)
    {
        const size_t b = sizeof(T) * std::max<size_t>(count, 1);
        *p = nullptr;
        if ((deny && !ptrs.empty()) || hipMalloc((void **)p, b) != hipSuccess) {
            (void)hipGetLastError();  // not an error of the call: the host build takes over
            *p = nullptr;
            return false;
        }
        ptrs.push_back(*p);
        bytes += (long long)b;
        return true;
    }
    ~XsScratch()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
};

}  // namespace

// on_device = false on return: nothing was published, build on the host
int xs_layout_device(sblas_csr_s &A, const std::vector<XsRange> &ranges, int rows_cap, int nrows_cap,
                     hipStream_t s, std::vector<long long> &blk, bool &on_device)
{
    XsPlan &P = A.xs;
    const int m = A.m, I = (int)ranges.size(), G = P.G, Wg = P.Wg;
    const long long nnz = A.nnz;
    const long long nblk = (long long)I * G;
    on_device = true;
    if (nnz == 0 || nblk == 0) {  // no entries: no chunks (the storage's one spare chunk is never read)
        blk.assign((size_t)nblk + 1, 0);
        SBLAS_HIP(hipMalloc(&P.key, kXsChunkBytes));
        return SBLAS_OK;
    }
    if (nblk >= (1LL << 27)) {  // counts and offsets are scanned as 32-bit words
        on_device = false;
        return SBLAS_OK;
    }
    auto bits = [](long long v) {
        int b = 0;
        while (v > 0) {
            ++b;
            v >>= 1;
        }
        return b;
    };
    const int cpb = bits((long long)Wg - 1);  // local column < Wg
    const int tot = cpb + bits(nblk - 1);
    const int passes = (tot + kXdMaxBits - 1) / kXdMaxBits;
    const int rb = passes ? (tot + passes - 1) / passes : 1;
    const int ntiles = (int)((nnz + kXdTile - 1) / kXdTile);
    const long long ncnt = (long long)ntiles << rb;

    double opt = 0.0;
    XsScratch sc;
    sc.deny = test_option("xs_devplan_nomem", &opt) && opt != 0.0;
    xsw_t *w0 = nullptr, *w1 = nullptr;
    int *p0 = nullptr, *p1 = nullptr, *counts = nullptr, *cscr = nullptr, *start = nullptr, *cnt = nullptr,
        *bscr = nullptr, *bad = nullptr;
    long long *dblk = nullptr;
    XsDevRange *drng = nullptr;
    if (!sc.take(&w0, (size_t)nnz) || !sc.take(&p0, (size_t)nnz) || !sc.take(&w1, (size_t)nnz) ||
        !sc.take(&p1, (size_t)nnz) || !sc.take(&counts, (size_t)ncnt) ||
        !sc.take(&cscr, scan_scratch_len(ncnt)) || !sc.take(&start, (size_t)nblk + 1) ||
        !sc.take(&cnt, (size_t)nblk) || !sc.take(&bscr, scan_scratch_len(nblk)) || !sc.take(&bad, 1) ||
        !sc.take(&dblk, (size_t)nblk + 2) || !sc.take(&drng, (size_t)I)) {
        on_device = false;
        return SBLAS_OK;
    }
    std::vector<XsDevRange> hr((size_t)I);
    for (int i = 0; i < I; ++i) hr[(size_t)i] = {ranges[(size_t)i].row0, ranges[(size_t)i].wide ? rows_cap : nrows_cap};
    SBLAS_HIP(hipMemcpyAsync(drng, hr.data(), sizeof(XsDevRange) * (size_t)I, hipMemcpyHostToDevice, s));
    SBLAS_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_xsd_keys, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, A.rowptr, A.col, m, A.n,
                       drng, I, G, Wg, w0, p0, bad);
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(k_xsd_count, dim3((unsigned)ntiles), dim3(kXdThreads), 0, s, w0, nnz, p * rb, rb, cpb,
                           ntiles, counts);
        SBLAS_TRY(scan_inclusive(counts, ncnt, cscr, s));
        hipLaunchKernelGGL(k_xsd_scatter, dim3((unsigned)ntiles), dim3(kXdThreads), 0, s, w0, p0, nnz, p * rb, rb,
                           cpb, ntiles, counts, w1, p1);
        std::swap(w0, w1);
        std::swap(p0, p1);
    }
    hipLaunchKernelGGL(k_xsd_bounds, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, w0, nnz, nblk, start);
    const unsigned bgrid = (unsigned)((nblk + 255) / 256);
    hipLaunchKernelGGL(k_xsd_chunks, dim3(bgrid), dim3(256), 0, s, start, nblk, cnt);
    SBLAS_TRY(scan_inclusive(cnt, nblk, bscr, s));
    hipLaunchKernelGGL(k_xsd_blk, dim3(bgrid), dim3(256), 0, s, cnt, nblk, bad, dblk);
    SBLAS_HIP(hipGetLastError());
    // the one wait of the build: blk[] (and the bad flag behind it)
    std::vector<long long> hb((size_t)nblk + 2);
    SBLAS_HIP(hipMemcpyAsync(hb.data(), dblk, sizeof(long long) * hb.size(), hipMemcpyDeviceToHost, s));
    SBLAS_HIP(hipStreamSynchronize(s));
    P.d2h_bytes += (long long)(sizeof(long long) * hb.size());
    P.scratch_bytes = sc.bytes;
    if (hb[(size_t)nblk + 1] != 0) {
        set_error("%s", kXsBadMsg);
        return SBLAS_ERR_INVALID;
    }
    hb.pop_back();
    const long long nchunks = hb.back();
    bool sane = hb[0] == 0 && nchunks >= 0 && nchunks <= nnz / kXsChunk + nblk;
    for (size_t k = 0; sane && k < (size_t)nblk; ++k) sane = hb[k + 1] >= hb[k];
    if (!sane) {
        set_error("xsort: device layout build produced inconsistent block offsets");
        return SBLAS_ERR_HIP;
    }
    if (hipMalloc(&P.key, (size_t)std::max<long long>(nchunks, 1) * kXsChunkBytes) != hipSuccess) {
        (void)hipGetLastError();
        P.key = nullptr;
        on_device = false;  // the host build holds no scratch beside the storage
        return SBLAS_OK;
    }
    if (nchunks)
        hipLaunchKernelGGL(k_xsd_fill, dim3((unsigned)nchunks), dim3(kXsChunk), 0, s, w0, p0, A.val, nnz, start,
                           dblk, nblk, reinterpret_cast<unsigned char *>(P.key));
    SBLAS_HIP(hipGetLastError());
    // the scratch is freed on return: the fill must have read it
    SBLAS_HIP(hipStreamSynchronize(s));
    blk.swap(hb);
    return SBLAS_OK;
}

}  // namespace sblas
