// value_ranges.cpp -- the element ranges behind sblas_ctx_matrix_set_values
// (value_ranges.hpp).
#include "value_ranges.hpp"

#include <algorithm>
#include <cstring>

namespace sblas {

void cyclic_value_ranges(int m, const long long *rowptr, int g, long long chunk_rows, int d, long long lc0,
                         long long lc1, std::vector<ValRange> &out)
{
    if (m <= 0 || !rowptr || g <= 0 || chunk_rows <= 0 || d < 0 || d >= g) return;
    const long long nchunks = ((long long)m + chunk_rows - 1) / chunk_rows;
    for (long long lc = std::max(0LL, lc0); lc < lc1; ++lc) {
        const long long j = d + lc * g;
        if (j >= nchunks) break;
        const long long a = j * chunk_rows, b = std::min<long long>(m, a + chunk_rows);
        out.push_back({rowptr[a], rowptr[b]});
    }
}

long long value_ranges_count(const std::vector<ValRange> &r)
{
    long long n = 0;
    for (const ValRange &v : r) n += std::max(0LL, v.end - v.begin);
    return n;
}

long long stage_values(const std::vector<ValRange> &r, const double *val, double *dst)
{
    long long o = 0;
    for (const ValRange &v : r) {
        const long long cnt = v.end - v.begin;
        if (cnt <= 0) continue;
        std::memcpy(dst + o, val + v.begin, sizeof(double) * (size_t)cnt);
        o += cnt;
    }
    return o;
}

}  // namespace sblas
