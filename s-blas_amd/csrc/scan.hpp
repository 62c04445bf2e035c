// scan.hpp -- the library's device scan (scan.hip) and the wave scan its
// kernels and the radix passes share.  For .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace sblas {

// In-place inclusive scan of a[0, len) on stream s; scratch holds
// scan_scratch_len(len) ints.
int scan_inclusive(int *a, long long len, int *scratch, hipStream_t s);
// ints of scratch scan_inclusive(., len, ., .) uses: its tiles, level by level
size_t scan_scratch_len(long long len);

__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

}  // namespace sblas
