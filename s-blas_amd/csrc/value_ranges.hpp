// value_ranges.hpp -- which elements of the global CSR value array each handle
// of a context holds (sblas_ctx_matrix_set_values): plain host code, no GPU.
#pragma once

#include <vector>

namespace sblas {

struct ValRange {
    long long begin, end;  // elements [begin, end) of the global arrays
};

// Cyclic partition (sblas_cyclic_local_csr): device d of g holds the chunks
// d, d + g, ... of chunk_rows rows.  Appends one range per local chunk
// lc in [lc0, lc1) that exists (rows below m), in local order: O(chunks).
void cyclic_value_ranges(int m, const long long *rowptr, int g, long long chunk_rows, int d, long long lc0,
                         long long lc1, std::vector<ValRange> &out);

// elements of the ranges
long long value_ranges_count(const std::vector<ValRange> &r);

// val's elements of the ranges, in order, to dst (room for value_ranges_count); returns the count
long long stage_values(const std::vector<ValRange> &r, const double *val, double *dst);

}  // namespace sblas
