// xsort_plan.cpp -- the planner of the xsort SpMV (algo 5): column groups,
// row ranges, items and their XCD queues.  Plain host arithmetic on rowptr, n
// and the number of resident workgroups: no GPU, no handle, no process state,
// so the same arguments always give the same plan (sblas_xsort_plan_host lets
// CPU code call it).  build_xsort_plan turns the result into the device plan.
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/sblas.h"
#include "xsort.hpp"

namespace sblas {
namespace {

// Cost model (work units ~ one streamed entry): a sub-item's time is its
// entries plus lambda per distinct x line its gathers touch; with uniform
// columns a block of c entries over L lines touches L*(1 - exp(-c/L))
// lines.  A narrow sub-item spreads its entries over all of x (G*Lg
// lines), a wide one its 1/8 share over its XCD's q groups.  lambda = 1.0
// is the best of a sweep (0.3 .. 1.7) on config 2.
struct XsCost {
    int G, q;
    double Lg;  // 128-B lines of one group's x slice
    static constexpr double lam = 1.0;
    double narrow(double c) const { return c + lam * G * Lg * (1.0 - std::exp(-c / (G * Lg))); }
    double wide(double c) const
    {
        const double ci = c / 8.0;
        return ci + lam * q * Lg * (1.0 - std::exp(-ci / (q * Lg)));
    }
};

// what the range cutting reads beside the cap
struct XsCut {
    int m;
    const int *rp;
    XsCost cost;
    bool all_wide;
    int rows_cap, nrows_cap;
    double nfac;  // a narrow range's cost, in sub-item caps
};

// column groups: G = 8q groups of Wg < 2^18 columns (the all-ones column
// field is the padding key) and ~1 MiB of x (an XCD's current group plus
// the entry stream must fit its 4 MiB L2)
int plan_groups(int n, XsHostPlan &P)
{
    const long long wmax = (1LL << kXsColBits) - 1;
    const long long ng = ((long long)std::max(n, 1) + wmax - 1) / wmax;
    const long long nmib = ((long long)std::max(n, 1) * 8 + (1LL << 20) - 1) >> 20;
    P.q = (int)std::max<long long>({1LL, (ng + 7) / 8, (nmib + 7) / 8});
    P.G = 8 * P.q;
    if (P.G > 127) {
        set_error("xsort: n = %d needs %d column groups (> 127)", n, P.G);
        return SBLAS_ERR_UNSUPPORTED;
    }
    P.Wg = (int)std::max<long long>(1, ((long long)std::max(n, 1) + P.G - 1) / P.G);
    return SBLAS_OK;
}

// cut(r): the first row always, then rows while the range's cost stays
// <= cap, at most rows_cap rows.  The cost grows strictly with the
// entry count rp[e] - rp[r], so the end is a binary search over e
// (O(log m) cost evaluations per range instead of one per row: the
// cap search below cuts the ranges many times over all m rows).
int cut(const XsCut &c, double cap, int r, bool wide, long long &cnt)
{
    const int *rp = c.rp;
    const int start = r;
    const int emax = (int)std::min<long long>(c.m, (long long)start + (wide ? c.rows_cap : c.nrows_cap));
    auto fits = [&](int e) {
        const double w = (double)(rp[e] - rp[start]);
        return wide ? c.cost.wide(w) <= cap : c.cost.narrow(w) <= c.nfac * cap;
    };
    int lo = start + 1, hi = emax;  // answer in [lo, hi]; lo always taken
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (fits(mid)) lo = mid;
        else hi = mid - 1;
    }
    cnt = rp[lo] - rp[start];
    return lo;
}

// Row ranges: from row r, a wide candidate takes <= rows_cap rows while
// one of its 8 sub-items costs <= cap.  It is WIDE (8 sub-items + 8
// partials per row) when it holds more than one narrow sub-item's work and
// its rows average >= 16 entries (the partials then cost <= 8 B per
// entry); otherwise a narrow range of cost <= cap is cut afresh from r.
void ranges_for_cap(const XsCut &c, double cap, std::vector<XsRange> &ranges)
{
    ranges.clear();
    int r = 0;
    while (r < c.m) {
        long long cnt;
        int e = cut(c, cap, r, true, cnt);
        const bool wide = cnt > 0 && (c.all_wide || (c.cost.narrow((double)cnt) > c.nfac * cap &&
                                                     cnt >= 16LL * (e - r)));
        if (!wide) e = cut(c, cap, r, false, cnt);
        XsRange R{};
        R.row0 = r;
        R.nrows = e - r;
        R.wide = wide ? 1 : 0;
        ranges.push_back(R);
        r = e;
    }
}

long long count_subs(const std::vector<XsRange> &ranges, bool solo)
{
    long long c = 0;
    for (const XsRange &R : ranges) c += R.wide ? 8 : solo ? 2 : 1;
    return c;
}

// grow the sub-item cost until the sub-items fit the resident grid (a
// second round for a few items would double the kernel's tail).  The
// "xs_cap" test hook fixes the cap instead (many small items: the
// dynamic claims run on small matrices).
void search_cap(const XsCut &c, long long nnz, long long slots, bool solo, const XsPlanOptions &opt,
                std::vector<XsRange> &ranges)
{
    const bool fixed_cap = opt.has_cap;
    double cap = fixed_cap ? std::max(1.0, opt.cap) : c.cost.narrow((double)nnz) / (double)slots;
    // Ranges hold at most rows_cap rows, so once ceil(m / rows_cap) exceeds
    // the slots no cap can fit them: stop there (and after 50 growth steps
    // without fewer sub-items) instead of 400 O(m) passes.  Leftover
    // sub-items are still correct: the grid claims them in a second round.
    const long long min_ranges = ((long long)c.m + c.rows_cap - 1) / c.rows_cap;
    long long best_subs = -1;
    for (int it = 0, flat = 0; it < 400; ++it) {
        ranges_for_cap(c, cap, ranges);
        const long long subs = count_subs(ranges, solo);
        if (subs <= slots || fixed_cap || min_ranges > slots) break;
        flat = (best_subs >= 0 && subs >= best_subs) ? flat + 1 : 0;
        if (flat >= 50) break;
        if (best_subs < 0 || subs < best_subs) best_subs = subs;
        cap *= 1.02;
    }
}

typedef std::vector<std::pair<int, int>> XsQueue;

// solo narrow items (narrow, -1); wide sub-items paired within their
// XCD; each queue alternates the two kinds
void pair_solo(const std::vector<int> &nsub, const std::vector<int> *wsub, XsQueue *q)
{
    XsQueue qn[8], qw[8];
    for (size_t j = 0; j < nsub.size(); ++j) qn[j % 8].push_back({nsub[j], -1});
    for (int k = 0; k < 8; ++k)
        for (size_t j = 0; j < wsub[k].size(); j += 2)
            qw[k].push_back({wsub[k][j], j + 1 < wsub[k].size() ? wsub[k][j + 1] : -1});
    for (int k = 0; k < 8; ++k)
        for (size_t j = 0; j < std::max(qn[k].size(), qw[k].size()); ++j) {
            if (j < qn[k].size()) q[k].push_back(qn[k][j]);
            if (j < qw[k].size()) q[k].push_back(qw[k][j]);
        }
}

// a narrow (gather-bound) with a wide (stream-bound) sub-item where
// possible, the XCDs interleaved so the narrow ones spread evenly;
// leftovers pair among themselves (wide ones within their XCD)
void pair_mixed(const std::vector<int> &nsub, const std::vector<int> *wsub, int resident, XsQueue *q)
{
    size_t ni = 0;
    std::vector<int> wleft[8];
    for (size_t j = 0;; ++j) {
        bool any = false;
        for (int k = 0; k < 8; ++k) {
            if (j >= wsub[k].size()) continue;
            any = true;
            if (ni < nsub.size()) q[k].push_back({nsub[ni++], wsub[k][j]});
            else wleft[k].push_back(wsub[k][j]);
        }
        if (!any) break;
    }
    for (int k = 0; k < 8; ++k)
        for (size_t j = 0; j < wleft[k].size(); j += 2)
            q[k].push_back({wleft[k][j], j + 1 < wleft[k].size() ? wleft[k][j + 1] : -1});
    // leftover light sub-items: two to an item only as far as the grid
    // needs it; the rest run alone (both teams on one sub-item), so an
    // item never carries twice a light sub-item's work while workgroups
    // idle (power-law matrices: most rows light, few heavy sub-items)
    long long items_now = 0;
    for (int k = 0; k < 8; ++k) items_now += (long long)q[k].size();
    const long long left = (long long)(nsub.size() - ni);
    const long long free_slots = std::max<long long>(0, (long long)resident - items_now);
    long long npairs = std::max<long long>(0, left - free_slots);  // items = left - npairs <= free
    if (2 * npairs > left) npairs = left / 2;
    for (int t = 0; ni < nsub.size(); ++t) {
        const int a0 = nsub[ni++];
        const int a1 = (npairs > 0 && ni < nsub.size()) ? nsub[ni++] : -1;
        if (a1 >= 0) --npairs;
        q[t % 8].push_back({a0, a1});
    }
}

// queue lengths, the grid, and the items each queue hands out statically
// (block b takes index b / 8 of queue b % 8); anything beyond is claimed
void queue_stats(int resident, XsHostPlan &P)
{
    P.qstride = 1;
    P.nitems = 0;
    for (int k = 0; k < 8; ++k) {
        P.qlen[k] = (int)P.queue[k].size();
        P.qstride = std::max(P.qstride, P.qlen[k]);
        P.nitems += P.qlen[k];
    }
    P.grid = std::min(P.nitems, resident);
    int nstat = 0;
    for (int k = 0; k < 8; ++k) {
        const int blocks_k = P.grid > k ? (P.grid - k + 7) / 8 : 0;  // blocks b < grid with b % 8 == k
        P.qstat[k] = std::min(P.qlen[k], blocks_k);
        nstat += P.qstat[k];
    }
    P.dynamic = nstat < P.nitems ? 1 : 0;
}

}  // namespace

int xs_plan_host(int m, int n, long long nnz, const int *rp, int resident, const XsPlanOptions &opt,
                 XsHostPlan &P)
{
    P = XsHostPlan{};
    const int st = plan_groups(n, P);
    if (st != SBLAS_OK) return st;
    // Resident workgroups = item slots; a paired item holds two sub-items.
    const long long slots = (long long)resident * 2;  // sub-items
    // every range wide (8 XCD-local sub-items + partials per row) on small
    // matrices: a rank's slice of the uniform config 2 at N = 8 (5.0M
    // entries) 47.0 -> 41.8 us, N = 16 (2.5M) 33.8 -> 29.9, but N = 4 (9.9M)
    // 66.8 -> 104 (profiles/r05/sweep2/): the partials (16 B per row and XCD)
    // outweigh XCD-local gathers beyond ~6M entries.
    const bool all_wide = opt.allwide >= 0 ? opt.allwide != 0 : nnz <= kXsAllWideMaxNnz;
    P.rows_cap = kXsHalfRows;
    // Solo narrow items: a narrow range is an item of its own -- both teams'
    // waves and all 16,384 LDS rows -- so its blocks are twice as dense
    // (fewer x line requests per entry); wide ranges still pair (wide, wide)
    // at 8,192 rows a team.  Chosen when >= 40% of the rows are empty
    // (power-law graphs: an empty row spends an accumulator row, so 16,384
    // rows per light range hold what 8,192 would without them): R-MAT scale
    // 21 (50% empty) 158.8 -> 147.3 us; config 2 and the stencils have none
    // and keep pairs (solo there: 146.7 vs 131 us; profiles/r04/rmat/).
    {
        long long empty = 0;
        for (int r = 0; r < m; ++r) empty += rp[r + 1] == rp[r];
        P.solo = opt.solo >= 0 ? opt.solo != 0 : (m > 0 && 5 * empty >= 2LL * m);
    }
    P.nrows_cap = P.solo ? kXsItemRows : P.rows_cap;  // narrow ranges
    const XsCut c{m, rp, XsCost{P.G, P.q, std::max(1.0, P.Wg / 16.0)}, all_wide, P.rows_cap, P.nrows_cap,
                  P.solo ? 2.0 : 1.0};
    search_cap(c, nnz, slots, P.solo, opt, P.ranges);
    const int I = (int)P.ranges.size();
    if ((long long)I >= (1LL << 23)) {
        set_error("xsort: %d row ranges (> 2^23)", I);
        return SBLAS_ERR_UNSUPPORTED;
    }

    // sub-items, wide partial slots, then items (pairs) in XCD queues
    std::vector<int> nsub, wsub[8];
    for (int i = 0; i < I; ++i) {
        XsRange &R = P.ranges[i];
        R.widx = -1;
        if (R.wide) {
            R.pbase = P.partial_len;
            P.partial_len += 8LL * R.nrows;
            R.widx = (int)P.wide.size();
            P.wide.push_back(i);
            for (int k = 0; k < 8; ++k) wsub[k].push_back((i << 8) | (k + 1));
        } else {
            nsub.push_back(i << 8);
        }
    }
    if (P.solo) pair_solo(nsub, wsub, P.queue);
    else pair_mixed(nsub, wsub, resident, P.queue);
    queue_stats(resident, P);
    return SBLAS_OK;
}

}  // namespace sblas

using namespace sblas;

extern "C" int sblas_xsort_plan_host(int m, int n, const long long *rowptr, int resident, const double *cap,
                                     int allwide, int solo, long long *info, long long *ranges,
                                     long long ranges_cap, int *items, long long items_cap)
{
    if (!rowptr || !info || m < 0 || n < 0 || resident < 1) return SBLAS_ERR_INVALID;
    std::vector<int> rp((size_t)m + 1);
    for (int r = 0; r <= m; ++r) {
        if (rowptr[r] < 0 || rowptr[r] > INT_MAX || (r && rowptr[r] < rowptr[r - 1])) {
            set_error("sblas_xsort_plan_host: rowptr[%d] is not an ascending 32-bit offset", r);
            return SBLAS_ERR_INVALID;
        }
        rp[(size_t)r] = (int)rowptr[r];
    }
    XsPlanOptions opt;
    opt.has_cap = cap != nullptr;
    opt.cap = cap ? *cap : 0.0;
    opt.allwide = allwide < 0 ? -1 : allwide != 0;
    opt.solo = solo < 0 ? -1 : solo != 0;
    XsHostPlan P;
    const int st = xs_plan_host(m, n, rp[(size_t)m] - rp[0], rp.data(), resident, opt, P);
    if (st != SBLAS_OK) return st;
    const long long head[11] = {P.q, P.G, P.Wg, P.solo ? 1 : 0, (long long)P.ranges.size(),
                                (long long)P.wide.size(), P.nitems, P.grid, P.dynamic, P.qstride,
                                P.partial_len};
    for (int i = 0; i < 11; ++i) info[i] = head[i];
    for (int k = 0; k < 8; ++k) {
        info[11 + k] = P.qlen[k];
        info[19 + k] = P.qstat[k];
    }
    if ((ranges && ranges_cap < (long long)P.ranges.size()) || (items && items_cap < P.nitems)) {
        set_error("sblas_xsort_plan_host: room for %lld ranges and %lld items, %lld and %d needed",
                  ranges ? ranges_cap : 0, items ? items_cap : 0, (long long)P.ranges.size(), P.nitems);
        return SBLAS_ERR_INVALID;
    }
    if (ranges)
        for (size_t i = 0; i < P.ranges.size(); ++i) {
            const XsRange &R = P.ranges[i];
            const long long v[5] = {R.row0, R.nrows, R.wide, R.widx, R.pbase};
            for (int j = 0; j < 5; ++j) ranges[5 * i + j] = v[j];
        }
    if (items)
        for (int k = 0; k < 8; ++k)
            for (const auto &it : P.queue[k]) {
                *items++ = it.first;
                *items++ = it.second;
            }
    return SBLAS_OK;
}
