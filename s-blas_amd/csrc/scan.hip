// scan.hip -- in-place inclusive scan of 32-bit counts: 2048-element tiles,
// the tile totals scanned by the same kernels one level up, then added back.
// Used by the transpose's and the xsort layout's radix passes and by the CSR5
// and panel plan builds.
#include "sblas_internal.hpp"
#include "scan.hpp"

namespace sblas {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;

// Inclusive scan of each 2048-element tile; tile totals to bsum.
__global__ __launch_bounds__(kScanThreads) void k_scan_tiles(int *__restrict__ a, long long len,
                                                             int *__restrict__ bsum)
{
    __shared__ int wtot[kScanThreads / 64];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    int v[kScanItems];
    int run = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const long long i = base + k;
        run += (i < len) ? a[i] : 0;
        v[k] = run;
    }
    const int incl = wave_incl_scan(run);
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wtot[wid] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += wtot[w];
    const int off = woff + incl - run;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const long long i = base + k;
        if (i < len) a[i] = v[k] + off;
    }
    if (threadIdx.x == kScanThreads - 1) bsum[blockIdx.x] = woff + incl;
}

__global__ void k_scan_add(int *__restrict__ a, long long len, const int *__restrict__ bsum)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long tile = i / kScanTile;
    if (i < len && tile > 0) a[i] += bsum[tile - 1];
}

// level k's tile totals lie behind level k - 1's in scratch
int scan_inclusive(int *a, long long len, int *scratch, hipStream_t s)
{
    if (len <= 0) return SBLAS_OK;
    const long long tiles = (len + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, a, len, scratch);
    if (tiles > 1) {
        SBLAS_TRY(scan_inclusive(scratch, tiles, scratch + tiles, s));
        hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, a, len,
                           scratch);
    }
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

// the same walk as scan_inclusive's recursion: `tiles` ints per level, while
// a level has more than one element
size_t scan_scratch_len(long long len)
{
    size_t tot = 0;
    for (long long t = len; t > 1;) {
        t = (t + kScanTile - 1) / kScanTile;
        tot += (size_t)t;
    }
    return tot + 2;
}

}  // namespace sblas
