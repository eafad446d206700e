// ASan/UBSan driver for the host constraint-aware flat extraction (csrc/constraints.cpp,
// constrained_flat_labels_host): the hand-worked vector bit for bit, 300 seeded random trees
// (built by flat_cluster_tree_host; continuous and tie-heavy weights, every optional output on
// and off) against a linear-walk restatement -- every constraint walks its chains cluster by
// cluster, every cluster walks to the root for its selected ancestor -- and the error paths (the
// constraint limit, out-of-range trees, point ids and types).  Built and run by
// tests/test_constraints_sanitize.py (hipcc --cuda-host-only -fsanitize=address,undefined).  No
// device, no library: a host stub stands in for the error setter.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "internal.hpp"

namespace hdb {
void set_error(const std::string &) {}
}  // namespace hdb

template <class F>
static int guarded(F &&f) {
    try {
        return f();
    } catch (const hdb::Error &e) {
        return e.code;
    }
}

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    rs ^= rs << 13, rs ^= rs >> 7, rs ^= rs << 17;
    return rs;
}
static double urand() { return (double)(next() >> 11) / 9007199254740992.0; }
static int irand(int n) { return (int)(next() % (uint64_t)n); }
static bool same_bits(double x, double y) { return memcmp(&x, &y, 8) == 0; }

struct Tree {
    int64_t K = 0;
    int n = 0;
    std::vector<int32_t> parent, min_id, flat, pc;
    std::vector<double> stab;
};
struct Cons {
    std::vector<int32_t> a, b, t;
};
struct Out {  // exactly K / n entries: ASan sees any write past them
    std::vector<int32_t> num, prop, flat, labels;
    std::vector<double> pstab;
    int64_t k = -7;
    Out(int64_t K, int n) : num((size_t)K, -7), prop((size_t)K, -7), flat((size_t)K, -7), labels((size_t)n, -7), pstab((size_t)K, -7.0) {}
};

static int run(const Tree &t, const Cons &c, Out &o, int skip = -1, int64_t m = INT64_MIN) {
    const hdb::ConstrainedOut co{skip == 0 ? nullptr : o.num.data(),   skip == 1 ? nullptr : o.prop.data(),
                                 skip == 2 ? nullptr : o.pstab.data(), skip == 3 ? nullptr : o.flat.data(),
                                 skip == 4 ? nullptr : o.labels.data(), skip == 5 ? nullptr : &o.k};
    return guarded([&] {
        return hdb::constrained_flat_labels_host(t.parent.data(), t.stab.data(), t.min_id.data(), t.K, t.pc.data(), t.n,
                                                 c.a.data(), c.b.data(), c.t.data(), m == INT64_MIN ? (int64_t)c.a.size() : m, co);
    });
}

// the restatement: plain walks over 1-based labels
static void walk(const Tree &t, const Cons &c, Out &w) {
    const int64_t K = t.K;
    auto par = [&](int32_t x) { return t.parent[x - 1]; };
    std::vector<long long> num((size_t)K + 1, 0), virt((size_t)K + 1, 0);
    std::vector<char> mark((size_t)K + 1, 0);
    std::vector<std::vector<int32_t>> kids((size_t)K + 1);
    for (int32_t x = 2; x <= K; x++) kids[par(x)].push_back(x);  // ascending label
    for (size_t k = 0; k < c.a.size(); k++) {
        const int32_t la = t.pc[c.a[k]], lb = t.pc[c.b[k]];
        for (int32_t x = la; x; x = par(x)) mark[x] = 1;
        int32_t L = lb;
        while (!mark[L]) L = par(L);
        for (int32_t x = la; x; x = par(x)) mark[x] = 0;
        if (c.t[k] == HDB_CONSTRAINT_MUST_LINK) {
            for (int32_t x = L; x; x = par(x)) num[x] += 2;
        } else {
            for (int32_t x = la; x != L; x = par(x)) num[x] += 1;
            for (int32_t x = lb; x != L; x = par(x)) num[x] += 1;
            if (!kids[la].empty()) virt[la]++;
            if (!kids[lb].empty()) virt[lb]++;
        }
    }
    std::vector<long long> csat((size_t)K + 1, 0), psat((size_t)K + 1, 0);
    std::vector<double> cstab((size_t)K + 1, 0.0), pstab((size_t)K + 1, 0.0);
    std::vector<char> self((size_t)K + 1, 0);
    for (int32_t x = (int32_t)K; x >= 1; x--) {
        long long ps = virt[x];
        double pst = 0.0;
        for (int32_t ch : kids[x]) ps += csat[ch], pst = pst + cstab[ch];
        psat[x] = ps, pstab[x] = pst;
        const double st = t.stab[x - 1];
        self[x] = x != 1 && (kids[x].empty() || num[x] > ps || (num[x] == ps && st >= pst));
        csat[x] = self[x] ? num[x] : ps;
        cstab[x] = self[x] ? st : pst;
    }
    std::vector<int32_t> top((size_t)K + 1, 0), sel;
    for (int32_t x = 2; x <= K; x++) {
        for (int32_t y = x; y; y = par(y))
            if (self[y]) top[x] = y;  // the last one seen on the way up is the topmost
        if (top[x] == x) sel.push_back(x);
    }
    std::sort(sel.begin(), sel.end(), [&](int32_t p, int32_t q) {
        return t.min_id[p - 1] != t.min_id[q - 1] ? t.min_id[p - 1] < t.min_id[q - 1] : p < q;
    });
    std::vector<int32_t> flat((size_t)K + 1, 0);
    for (size_t i = 0; i < sel.size(); i++) flat[sel[i]] = (int32_t)i + 1;
    for (int64_t i = 0; i < K; i++)
        w.num[i] = (int32_t)num[i + 1], w.prop[i] = (int32_t)psat[i + 1], w.pstab[i] = pstab[i + 1], w.flat[i] = flat[i + 1];
    for (int v = 0; v < t.n; v++) w.labels[v] = flat[top[t.pc[v]]];
    w.k = (int64_t)sel.size();
}

static int differ(const Out &x, const Out &y, int skip = -1) {
    int bad = 0;
    if (skip != 0) bad += x.num != y.num;
    if (skip != 1) bad += x.prop != y.prop;
    if (skip != 3) bad += x.flat != y.flat;
    if (skip != 4) bad += x.labels != y.labels;
    if (skip != 5) bad += x.k != y.k;
    for (size_t i = 0; skip != 2 && i < x.pstab.size(); i++) bad += !same_bits(x.pstab[i], y.pstab[i]);
    return bad;
}

// the first hand-worked vector of tests/test_constraints.py (tree A, list A1)
static int known() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Tree t;
    t.K = 5, t.n = 8;
    t.parent = {0, 1, 1, 3, 3}, t.min_id = {0, 0, 3, 3, 6}, t.pc = {2, 2, 2, 4, 4, 4, 5, 5};
    t.stab = {nan, 0.3 + 1.6, 5 * (1.0 / 3 - 1.0 / 5), 2.0, 3.3333333333333335};
    const Cons c{{3, 0, 1, 6, 0}, {6, 3, 1, 6, 7}, {0, 0, 0, 1, 1}};
    Out o(5, 8), w(5, 8);
    int bad = run(t, c, o) != 0;
    const std::vector<int32_t> num{6, 3, 3, 0, 1}, prop{6, 0, 1, 0, 0}, flat{0, 1, 2, 0, 0}, labels{1, 1, 1, 2, 2, 2, 2, 2};
    const double pstab[] = {0.0 + t.stab[1] + t.stab[2], 0.0, 0.0 + t.stab[3] + t.stab[4], 0.0, 0.0};
    bad += o.num != num || o.prop != prop || o.flat != flat || o.labels != labels || o.k != 2;
    for (int i = 0; i < 5; i++) bad += !same_bits(o.pstab[i], pstab[i]);
    walk(t, c, w);
    bad += differ(o, w);
    if (bad) printf("known answer: %d mismatches\n", bad);
    return bad;
}

static int random_trees() {
    int bad = 0, changed = 0;
    for (int tr = 0; tr < 300; tr++) {
        const int n = 2 + irand(tr % 10 == 0 ? 2000 : 300), mcs = 2 + irand(4), wmax = tr % 2 ? 1 + irand(6) : 0;
        std::vector<int32_t> va, vb, perm(n);
        std::vector<double> w;
        for (int i = 0; i < n; i++) perm[i] = i;
        for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[irand(i + 1)]);
        for (int i = 1; i < n; i++) va.push_back(perm[irand(i)]), vb.push_back(perm[i]), w.push_back(wmax ? (double)irand(wmax + 1) : urand());
        Tree t;
        t.n = n;
        const int64_t cap = hdb::cluster_tree_bound(n, mcs);
        t.parent.assign((size_t)cap, 0), t.min_id.assign((size_t)cap, 0), t.flat.assign((size_t)cap, 0), t.stab.assign((size_t)cap, 0.0);
        t.pc.assign((size_t)n, 0);
        int64_t nsel = -1;
        const hdb::ClusterTreeOut to{cap, &t.K, t.parent.data(), nullptr, nullptr, t.stab.data(), nullptr, t.min_id.data(),
                                     t.flat.data(), t.pc.data(), nullptr};
        if (guarded([&] { return hdb::flat_cluster_tree_host(va.data(), vb.data(), w.data(), n - 1, n, mcs, to, nullptr, &nsel); })) {
            bad++, printf("tree %d: no tree\n", tr);
            continue;
        }
        const int64_t K = t.K;
        t.parent.resize((size_t)K), t.min_id.resize((size_t)K), t.flat.resize((size_t)K), t.stab.resize((size_t)K);
        Cons c;
        const int m = tr % 5 == 0 ? 0 : 1 + irand(tr % 3 == 0 ? 3000 : 80);
        for (int k = 0; k < m; k++) {
            const int a = irand(n);
            c.a.push_back(a), c.b.push_back(irand(20) == 0 ? a : irand(n)), c.t.push_back(irand(2));
        }
        if (m == 0) c.a.reserve(1), c.b.reserve(1), c.t.reserve(1);
        Out o(K, n), ref(K, n);
        walk(t, c, ref);
        int miss = run(t, c, o) != 0 || differ(o, ref);
        if (m == 0) miss += o.flat != t.flat || o.k != nsel;  // the unconstrained selection
        changed += o.flat != t.flat;
        for (int skip = 0; skip < 6; skip++) {  // each output NULL on its own
            Out p(K, n);
            miss += run(t, c, p, skip) != 0 || differ(p, ref, skip);
        }
        if (miss) bad++, printf("tree %d (n %d, mcs %d, K %lld, m %d): %d mismatches\n", tr, n, mcs, (long long)K, m, miss);
        // error paths: nothing is read or written out of bounds
        Out q(K, n);
        if (run(t, c, q, -1, (int64_t(1) << 30)) != HDB_EINVAL || run(t, c, q, -1, -1) != HDB_EINVAL) bad++;
        const int v = irand(n);
        const int32_t keep = t.pc[v];
        if (m > 0) c.a[0] = v;  // the bad point is one a constraint names
        for (int32_t x : {0, -1, (int32_t)K + 1, INT32_MAX}) {
            t.pc[v] = x;
            if (run(t, c, q) != HDB_EINVAL) bad++;
        }
        t.pc[v] = keep;
        const int64_t ci = irand((int)K);
        const int32_t pk = t.parent[ci];
        for (int32_t x : {(int32_t)ci + 1, -1, INT32_MAX}) {
            t.parent[ci] = x;
            if (run(t, c, q) != HDB_EINVAL) bad++;
        }
        t.parent[ci] = pk;
        if (m > 0) {
            const int k = irand(m);
            const int32_t ka = c.a[k], kt = c.t[k];
            for (int32_t x : {-1, n, INT32_MAX}) {
                c.a[k] = x;
                if (run(t, c, q) != HDB_EINVAL) bad++;
            }
            c.a[k] = ka;
            for (int32_t x : {2, -1, INT32_MIN}) {
                c.t[k] = x;
                if (run(t, c, q) != HDB_EINVAL) bad++;
            }
            c.t[k] = kt;
        }
        if (run(t, c, q) != 0) bad++;
    }
    if (changed < 100) bad++, printf("the constraints changed the selection in only %d trees\n", changed);
    return bad;
}

int main() {
    int bad = known();
    bad += random_trees();
    if (bad) {
        printf("host constraints: %d mismatches\n", bad);
        return 1;
    }
    printf("host constraints ok\n");
    return 0;
}
