// ASan/UBSan driver for the host cluster tree and level cuts (csrc/flat.cpp,
// flat_cluster_tree_host / labels_at_levels_host): the hand-checked known-answer vector bit for
// bit, a few hundred seeded random trees (continuous and tie-heavy weights, n below and above
// minClSize, every optional output on and off; the flat labels and noise levels re-derived from
// the tree against flat_labels_host / flat_outlier_scores_host, the cuts against a plain linear
// walk) and the error paths (capacity, NaN level, out-of-range trees, the input errors of
// flat_labels_host).  Built and run by tests/test_cluster_tree_sanitize.py (hipcc
// --cuda-host-only -fsanitize=address,undefined).  No device, no library: a host stub stands in
// for the error setter.
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

static uint64_t rs = 0x2545F4914F6CDD1Dull;
static uint64_t next() {
    rs ^= rs << 13, rs ^= rs >> 7, rs ^= rs << 17;
    return rs;
}
static double urand() { return (double)(next() >> 11) / 9007199254740992.0; }
static int irand(int n) { return (int)(next() % (uint64_t)n); }

static uint64_t digest = 1469598103934665603ull;
static void mix(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    digest = (digest ^ b) * 1099511628211ull;
}
static bool same_bits(double x, double y) { return memcmp(&x, &y, 8) == 0; }

struct Tree {
    int64_t K = -1, nsel = -1;
    std::vector<int32_t> parent, size, min_id, flat, pc;
    std::vector<double> birth, death, stab, pl;
};

static int build(const std::vector<int32_t> &va, const std::vector<int32_t> &vb, const std::vector<double> &w, int64_t ne,
                 int n, int mcs, Tree &t, int64_t cap = -1) {
    if (cap < 0) cap = hdb::cluster_tree_bound(n, mcs);
    const size_t c = (size_t)cap;  // exactly cap entries: ASan sees any write past them
    t.parent.assign(c, -7), t.size.assign(c, -7), t.min_id.assign(c, -7), t.flat.assign(c, -7);
    t.birth.assign(c, -7), t.death.assign(c, -7), t.stab.assign(c, -7);
    t.pc.assign((size_t)n, -7), t.pl.assign((size_t)n, -7);
    const hdb::ClusterTreeOut o{cap,           &t.K,           t.parent.data(), t.birth.data(), t.death.data(), t.stab.data(),
                                t.size.data(), t.min_id.data(), t.flat.data(),  t.pc.data(),    t.pl.data()};
    return guarded([&] { return hdb::flat_cluster_tree_host(va.data(), vb.data(), w.data(), ne, n, mcs, o, nullptr, &t.nsel); });
}

static int known() {
    const std::vector<int32_t> a{0, 1, 2, 3, 4, 5, 6}, b{1, 2, 3, 4, 5, 6, 7};
    const std::vector<double> w{1, 2, 5, 1, 1, 3, 0.5};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t parent[] = {0, 1, 1, 3, 3}, size[] = {8, 3, 5, 3, 2}, min_id[] = {0, 0, 3, 3, 6}, flat[] = {0, 1, 0, 2, 3};
    const int32_t pc[] = {2, 2, 2, 4, 4, 4, 5, 5};
    const double birth[] = {nan, 5, 5, 3, 3}, death[] = {5, 1, 3, 1, 0.5}, pl[] = {1, 1, 2, 1, 1, 1, 0.5, 0.5};
    const double stab[] = {nan, 0.3 + 1.6, 5 * (1.0 / 3 - 1.0 / 5), 2.0, 3.3333333333333335};
    Tree t;
    int bad = build(a, b, w, 7, 8, 2, t) != 0 || t.K != 5 || t.nsel != 3;
    for (int i = 0; i < 5 && !bad; i++) {
        bad += t.parent[i] != parent[i] || t.size[i] != size[i] || t.min_id[i] != min_id[i] || t.flat[i] != flat[i];
        bad += !(same_bits(t.death[i], death[i]) && same_bits(t.stab[i], stab[i]));
        bad += i ? !same_bits(t.birth[i], birth[i]) : !std::isnan(t.birth[0]);
    }
    for (int i = 0; i < 8 && !bad; i++) bad += t.pc[i] != pc[i] || !same_bits(t.pl[i], pl[i]);
    const double lv[] = {7, 5, 4, 2, 1.5, 0.75, 0.25};
    const int32_t want[7][8] = {{1, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}, {2, 2, 2, 3, 3, 3, 3, 3}, {2, 2, 2, 4, 4, 4, 5, 5},
                                {2, 2, 0, 4, 4, 4, 5, 5}, {0, 0, 0, 0, 0, 0, 5, 5}, {0, 0, 0, 0, 0, 0, 0, 0}};
    std::vector<int32_t> rows(7 * 8, -1);
    if (!bad)
        bad += guarded([&] {
            return hdb::labels_at_levels_host(t.parent.data(), t.birth.data(), 5, t.pc.data(), t.pl.data(), 8, lv, 7, rows.data());
        }) != 0;
    bad += memcmp(rows.data(), want, sizeof(want)) != 0;
    if (bad) printf("known answer: %d mismatches\n", bad);
    return bad;
}

static void random_tree(int n, int wmax, std::vector<int32_t> &va, std::vector<int32_t> &vb, std::vector<double> &w) {
    std::vector<int32_t> perm(n);
    for (int i = 0; i < n; i++) perm[i] = i;
    for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[irand(i + 1)]);
    va.clear(), vb.clear(), w.clear();
    for (int i = 1; i < n; i++) {
        va.push_back(perm[irand(i)]);
        vb.push_back(perm[i]);
        w.push_back(wmax ? (double)irand(wmax + 1) : urand());
    }
}

static int random_trees() {
    int bad = 0;
    for (int tr = 0; tr < 300; tr++) {
        const int n = 1 + irand(tr % 10 == 0 ? 2000 : 300), mcs = 2 + irand(7);
        std::vector<int32_t> va, vb;
        std::vector<double> w;
        random_tree(n, tr % 2 ? 1 + irand(6) : 0, va, vb, w);
        if (tr % 7 == 0)  // self edges are ignored
            for (int i = 0; i < n; i += 3) va.push_back(i), vb.push_back(i), w.push_back(urand());
        const int64_t ne = (int64_t)w.size();
        Tree t;
        int rc = build(va, vb, w, ne, n, mcs, t);
        const int64_t K = t.K;
        if (rc != 0 || K < 1 || K > hdb::cluster_tree_bound(n, mcs)) {
            bad++, printf("tree %d (n %d, mcs %d): status %d, K %lld\n", tr, n, mcs, rc, (long long)K);
            continue;
        }
        // optional outputs off: the same count; a capacity of exactly K suffices, K - 1 does not
        int64_t K2 = -1;
        const hdb::ClusterTreeOut none{K, &K2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        rc = guarded([&] { return hdb::flat_cluster_tree_host(va.data(), vb.data(), w.data(), ne, n, mcs, none, nullptr, nullptr); });
        Tree t3;
        const int rc3 = build(va, vb, w, ne, n, mcs, t3, K - 1);
        if (rc != 0 || K2 != K || rc3 != HDB_EINVAL || t3.K != K) bad++, printf("tree %d: capacity handling\n", tr);
        for (int64_t i = 0; i < K - 1; i++)
            if (t3.parent[i] != -7) bad++;
        // flat labels and noise levels of the existing entry points, re-derived from the tree
        std::vector<int32_t> lab(n), near(K);
        std::vector<double> s(n), e(n);
        int64_t k = -1;
        rc = guarded([&] { return hdb::flat_outlier_scores_host(va.data(), vb.data(), w.data(), ne, n, mcs, s.data(), e.data(), lab.data(), &k); });
        for (int64_t i = 0; i < K; i++) {
            if (i && (t.parent[i] < 1 || t.parent[i] > i)) bad++;
            near[i] = t.flat[i] ? t.flat[i] : (i ? near[t.parent[i] - 1] : 0);
        }
        std::vector<double> emax(t.death.begin(), t.death.begin() + K);
        emax[0] = std::numeric_limits<double>::max();
        for (int64_t i = K - 1; i >= 1; i--) emax[t.parent[i] - 1] = std::min(emax[t.parent[i] - 1], emax[i]);
        int miss = rc != 0 || k != t.nsel;
        for (int v = 0; v < n; v++) {
            miss += near[t.pc[v] - 1] != lab[v] || !same_bits(t.pl[v], e[v]);
            miss += !same_bits(t.pl[v] == 0.0 ? 0.0 : 1.0 - emax[t.pc[v] - 1] / t.pl[v], s[v]);
            mix(t.pl[v]);
        }
        for (int64_t i = 0; i < K; i++) mix(t.death[i]), mix(t.stab[i]);
        // cuts: levels of the tree, between, above, below, +-inf, duplicates -- against a linear walk
        std::vector<double> lv{std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), urand() * 3};
        for (int q = 0; q < 6; q++) lv.push_back(t.pl[irand(n)]), lv.push_back(t.pl[irand(n)] + 0.5);
        for (int q = 0; q < 4 && K > 1; q++) lv.push_back(t.birth[1 + irand((int)K - 1)]);
        lv.push_back(lv[3]);
        const int L = (int)lv.size();
        std::vector<int32_t> rows((size_t)L * n, -1);
        rc = guarded([&] {
            return hdb::labels_at_levels_host(t.parent.data(), t.birth.data(), K, t.pc.data(), t.pl.data(), n, lv.data(), L, rows.data());
        });
        miss += rc != 0;
        for (int l = 0; l < L && rc == 0; l++)
            for (int v = 0; v < n; v++) {
                int32_t c = 0;
                if (!(lv[l] < t.pl[v]))
                    for (c = t.pc[v]; c && t.birth[c - 1] <= lv[l];) c = t.parent[c - 1];
                miss += rows[(size_t)l * n + v] != c;
            }
        if (miss) bad++, printf("tree %d (n %d, mcs %d, K %lld): %d mismatches\n", tr, n, mcs, (long long)K, miss);
        // error paths of the cuts: NaN level, out-of-range tree (nothing is read out of bounds)
        auto cut_rc = [&] {
            return guarded([&] {
                return hdb::labels_at_levels_host(t.parent.data(), t.birth.data(), K, t.pc.data(), t.pl.data(), n, lv.data(), L, rows.data());
            });
        };
        lv[1] = std::nan("");
        if (cut_rc() != HDB_EINVAL) bad++;
        lv[1] = 0.5;
        const int v = irand(n);
        const int32_t keep = t.pc[v];
        for (int32_t x : {0, -1, (int32_t)K + 1, INT32_MAX}) {
            t.pc[v] = x;
            if (cut_rc() != HDB_EINVAL) bad++;
        }
        t.pc[v] = keep;
        const int64_t ci = irand((int)K);
        const int32_t pk = t.parent[ci];
        for (int32_t x : {(int32_t)ci + 1, -1, INT32_MAX}) {
            t.parent[ci] = x;
            if (cut_rc() != HDB_EINVAL) bad++;
        }
        t.parent[ci] = pk;
        if (cut_rc() != 0) bad++;
        if (n > 3) {  // not spanning / minClSize < 2 / cycle / bad id: the statuses of flat_labels_host
            auto both = [&](int64_t m, int c) {
                const int r1b = guarded([&] {
                    return hdb::flat_cluster_tree_host(va.data(), vb.data(), w.data(), m, n, c, none, nullptr, nullptr);
                });
                const int r2 = guarded([&] { return hdb::flat_labels_host(va.data(), vb.data(), w.data(), m, n, c, lab.data(), &k); });
                if (r1b != r2 || r2 == 0) bad++, printf("tree %d: error statuses %d / %d\n", tr, r1b, r2);
            };
            both(n - 2, mcs);
            both(n - 1, 1);
            const int32_t k0 = va[0];
            va[0] = va[1], vb[0] = vb[1];  // a doubled edge: cycle
            both(n - 1, mcs);
            va[0] = n + 5;
            both(n - 1, mcs);
            va[0] = k0;
        }
    }
    return bad;
}

int main() {
    int bad = known();
    bad += random_trees();
    printf("host cluster tree digest %016llx\n", (unsigned long long)digest);
    if (bad) {
        printf("host cluster tree: %d mismatches\n", bad);
        return 1;
    }
    printf("host cluster tree ok\n");
    return 0;
}
