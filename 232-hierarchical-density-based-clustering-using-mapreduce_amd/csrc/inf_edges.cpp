// inf_edges.cpp -- the infinite-weight tail of the exact-leaf MST (K2b), on the host.
//
// K2b's kernels treat w == +inf as "no edge yet" (Best starts at (inf, inf, MAX, MAX), and only
// w < inf is published to a component), so its rounds find exactly the finite-weight edges of
// the minimum spanning tree: the minimum spanning forest of the finite edges.  When a round
// adds nothing and the forest has more than one tree, every edge between two trees weighs +inf
// (a row with an infinite coordinate, a squared distance that overflows, an infinite core) or
// NaN.  Kruskal's order puts those after every finite edge, so the rest of the tree is the MST
// of the trees under the same strict total order (w, s, lo, hi) with w = +inf throughout: ties
// go by the squared distance s, then the ids.  A pair whose weight is NaN is not an edge.
//
// Such inputs are degenerate and carry no geometry, so the tail is a plain Boruvka on the host:
// every row outside the largest tree scans all rows (the largest tree's best edge is seen from
// its other end), O((n - largest) * n * d) per round, at most log2(trees) rounds.
#include <cmath>
#include <cstdint>
#include <vector>

#include "internal.hpp"

namespace hdb {

namespace {
struct TailKey {
    double s;
    int32_t lo, hi;
};
inline bool tail_less(const TailKey &a, const TailKey &b) {
    if (a.s < b.s) return true;
    if (a.s > b.s) return false;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.hi < b.hi;
}
}  // namespace

int64_t inf_edges_host(const double *X, const double *core, int64_t n, int d, const int32_t *ea, const int32_t *eb,
                       int64_t m, int32_t *oa, int32_t *ob, double *ow, int64_t *rows_left, int32_t *first_left) {
    std::vector<int32_t> par((size_t)n);
    for (int64_t i = 0; i < n; i++) par[i] = (int32_t)i;
    auto find = [&](int32_t x) {
        while (par[x] != x) {
            par[x] = par[par[x]];
            x = par[x];
        }
        return x;
    };
    int64_t trees = n;
    for (int64_t e = 0; e < m; e++) {
        const int32_t a = find(ea[e]), b = find(eb[e]);
        if (a == b) HDB_THROW(HDB_EINVAL, "boruvka: the finite edges hold a cycle (internal error)");
        par[b] = a;
        trees--;
    }
    std::vector<int32_t> root((size_t)n), size((size_t)n);
    std::vector<TailKey> best((size_t)n);
    int64_t added = 0;
    int32_t big = 0;
    auto label = [&]() {  // roots, and the largest tree (the smallest root id among equals)
        for (int64_t i = 0; i < n; i++) size[i] = 0;
        for (int64_t i = 0; i < n; i++) size[root[i] = find((int32_t)i)]++;
        big = root[0];
        for (int64_t i = 0; i < n; i++)
            if (size[root[i]] > size[big] || (size[root[i]] == size[big] && root[i] < big)) big = root[i];
    };
    while (trees > 1) {
        label();
        for (int64_t i = 0; i < n; i++) best[i] = TailKey{INFINITY, INT32_MAX, INT32_MAX};
        for (int64_t p = 0; p < n; p++) {
            const int32_t rp = root[p];
            if (rp == big) continue;
            const double *xp = X + p * d;
            for (int64_t q = 0; q < n; q++) {
                const int32_t rq = root[q];
                if (rq == rp || (rq != big && q < p)) continue;  // a pair of two small trees: once, from its smaller id
                const double *xq = X + q * d;
                double t = xp[0] - xq[0];
                double s = t * t;  // EuclideanDistance.java:31-33 order, as the scan kernel
                for (int c = 1; c < d; c++) {
                    t = xp[c] - xq[c];
                    s = s + t * t;
                }
                double w = std::sqrt(s);  // HDBSCANStar.java:162-168 order
                if (core[p] > w) w = core[p];
                if (core[q] > w) w = core[q];
                if (w != w) continue;  // NaN: not an edge
                if (w < INFINITY) HDB_THROW(HDB_EINVAL, "boruvka stalled with a finite edge left (internal error)");
                const TailKey k{s, (int32_t)(p < q ? p : q), (int32_t)(p < q ? q : p)};
                if (tail_less(k, best[rp])) best[rp] = k;
                if (tail_less(k, best[rq])) best[rq] = k;
            }
        }
        int64_t hooked = 0;
        for (int64_t c = 0; c < n; c++) {
            if (root[c] != (int32_t)c || best[c].lo == INT32_MAX) continue;
            // minima under a strict total order close no cycle but the mutual pair, which the
            // second of its two trees finds already joined
            const int32_t a = find(best[c].lo), b = find(best[c].hi);
            if (a == b) continue;
            par[b] = a;
            oa[added] = best[c].lo;
            ob[added] = best[c].hi;
            ow[added] = INFINITY;
            added++;
            hooked++;
            trees--;
        }
        if (hooked == 0) break;  // the trees left have only NaN pairs between them
    }
    *rows_left = 0;
    *first_left = -1;
    if (trees > 1) {
        label();
        for (int64_t i = 0; i < n; i++)
            if (root[i] != big) {
                if (*first_left < 0) *first_left = (int32_t)i;
                ++*rows_left;
            }
    }
    return added;
}

}  // namespace hdb
