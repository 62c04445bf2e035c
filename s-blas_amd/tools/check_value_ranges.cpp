// check_value_ranges.cpp -- stand-alone check of csrc/value_ranges.cpp (the
// element ranges behind sblas_ctx_matrix_set_values), meant for a sanitizer
// build on the host; not part of the test suite:
//   c++ -std=c++17 -g -fsanitize=address,undefined -o check_value_ranges \
//       tools/check_value_ranges.cpp csrc/value_ranges.cpp && ./check_value_ranges
// For random row pointers, device counts and chunk sizes it stages every
// device's share through the ranges and compares it with the values gathered
// row by row as the cyclic local CSR is built (chunks d, d + g, ... in order),
// and the per-part counts with the rows of the parts' chunks.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../csrc/value_ranges.hpp"

using namespace sblas;

static int fails = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                \
        }                                                           \
    } while (0)

static void one_case(std::mt19937_64 &rng, int m, int g, int chunks_per_rank, int parts)
{
    std::vector<long long> rp((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + (long long)(rng() % 7 == 0 ? 0 : rng() % 9);
    const long long nnz = rp[(size_t)m];
    std::vector<double> val((size_t)nnz);
    for (long long i = 0; i < nnz; ++i) val[(size_t)i] = (double)i + 0.5;
    // sblas_cyclic_plan
    const long long R = std::max(1LL, ((long long)m + (long long)g * chunks_per_rank - 1) / ((long long)g * chunks_per_rank));
    const long long nchunks = m ? (m + R - 1) / R : 0;
    const long long stride = std::max(1LL, ((nchunks + g - 1) / g) * R);
    const long long ncmax = stride / R;
    long long total = 0;
    for (int d = 0; d < g; ++d) {
        std::vector<double> want;
        std::vector<long long> chunk_cnt;
        for (long long j = d; j < nchunks; j += g) {
            const long long a = j * R, b = std::min<long long>(m, a + R);
            for (long long r = a; r < b; ++r)
                for (long long e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) want.push_back(val[(size_t)e]);
            chunk_cnt.push_back(rp[(size_t)b] - rp[(size_t)a]);
        }
        std::vector<ValRange> vr;
        cyclic_value_ranges(m, rp.data(), g, R, d, 0, ncmax, vr);
        EXPECT(vr.size() == chunk_cnt.size());
        EXPECT(value_ranges_count(vr) == (long long)want.size());
        std::vector<double> got(want.size());  // exactly the count: an overrun is the sanitizer's to catch
        EXPECT(stage_values(vr, val.data(), got.data()) == (long long)want.size());
        EXPECT(got == want);
        total += (long long)want.size();
        // parts of consecutive local chunks: their counts follow one another
        long long off = 0;
        for (int p = 0; p < parts; ++p) {
            const long long lo = (long long)p * ncmax / parts, hi = (long long)(p + 1) * ncmax / parts;
            std::vector<ValRange> pr;
            cyclic_value_ranges(m, rp.data(), g, R, d, lo, hi, pr);
            long long w = 0;
            for (long long lc = lo; lc < hi && lc < (long long)chunk_cnt.size(); ++lc) w += chunk_cnt[(size_t)lc];
            EXPECT(value_ranges_count(pr) == w);
            std::vector<double> pg((size_t)w);
            stage_values(pr, val.data(), pg.data());
            EXPECT(std::equal(pg.begin(), pg.end(), want.begin() + off));
            off += w;
        }
        EXPECT(off == (long long)want.size());
    }
    EXPECT(total == nnz);
}

int main()
{
    std::mt19937_64 rng(12345);
    const int ms[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 1000, 4099};
    for (int m : ms)
        for (int g = 1; g <= 5; ++g)
            for (int cpr : {1, 3, 8})
                for (int parts : {1, 2, 3}) one_case(rng, m, g, cpr, parts);
    // arguments that name no chunk give no range
    std::vector<ValRange> none;
    const long long rp1[2] = {0, 3};
    cyclic_value_ranges(1, rp1, 2, 1, 1, 0, 8, none);   // device 1 of 2 holds no chunk of a 1-row matrix
    cyclic_value_ranges(1, rp1, 2, 1, 2, 0, 8, none);   // d out of range
    cyclic_value_ranges(1, nullptr, 1, 1, 0, 0, 8, none);
    cyclic_value_ranges(1, rp1, 1, 1, 0, 3, 2, none);   // empty chunk interval
    EXPECT(none.empty());
    std::printf(fails ? "%d checks failed\n" : "value ranges: all checks passed\n", fails);
    return fails ? 1 : 0;
}
