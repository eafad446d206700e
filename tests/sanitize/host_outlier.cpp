// ASan/UBSan driver for the host GLOSH outlier scores (csrc/flat.cpp,
// flat_outlier_scores_host): the four hand-checked known-answer cases, bit for bit, then a few
// hundred seeded random trees (continuous and tie-heavy weights, n below and above minClSize,
// every optional output on and off) and the error paths.  Built and run by
// tests/test_outlier_sanitize.py (hipcc --cuda-host-only -fsanitize=address,undefined); prints
// a digest of every score.  No device, no library: a host stub stands in for the error setter.
#include <cfloat>
#include <cstdio>
#include <cstring>
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

static uint64_t digest = 1469598103934665603ull;
static void mix(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    digest = (digest ^ b) * 1099511628211ull;
}

struct Known {
    std::vector<int32_t> a, b;
    std::vector<double> w;
    int n, mcs;
    std::vector<double> eps, score;
};

static bool same_bits(double x, double y) { return memcmp(&x, &y, 8) == 0; }

static int known() {
    const double M = DBL_MAX;
    const Known cases[] = {
        {{0, 1, 3, 2, 4}, {1, 2, 4, 3, 5}, {1, 2, 1.5, 5, 4}, 6, 2, {1, 1, 2, 1.5, 1.5, 4}, {0, 0, 0.5, 0, 0, 0.625}},
        {{0, 1, 2, 3, 4, 5}, {1, 2, 3, 4, 5, 6}, {1, 1, 6, 2, 2, 9}, 7, 2, {1, 1, 1, 2, 2, 2, 9},
         {0, 0, 0, 0, 0, 0, 1.0 - 1.0 / 9.0}},
        {{0, 1, 2}, {1, 2, 3}, {0.5, 2, 3}, 4, 3, {2, 2, 2, 3}, {1.0 - M / 2.0, 1.0 - M / 2.0, 1.0 - M / 2.0, 1.0 - M / 3.0}},
        {{0, 1, 2, 3}, {1, 2, 3, 4}, {0, 0, 3, 0}, 5, 2, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}},
    };
    int bad = 0, id = 0;
    for (const Known &c : cases) {
        id++;
        std::vector<double> s(c.n), e(c.n);
        std::vector<int32_t> lab(c.n);
        int64_t k = -1;
        const int rc = guarded([&] {
            return hdb::flat_outlier_scores_host(c.a.data(), c.b.data(), c.w.data(), (int64_t)c.w.size(), c.n, c.mcs,
                                                 s.data(), e.data(), lab.data(), &k);
        });
        if (rc != 0) bad++, printf("case %d: status %d\n", id, rc);
        for (int i = 0; i < c.n; i++) {
            if (!same_bits(s[i], c.score[i]) || !same_bits(e[i], c.eps[i])) {
                bad++;
                printf("case %d point %d: eps %.17g (want %.17g) score %.17g (want %.17g)\n", id, i, e[i], c.eps[i], s[i],
                       c.score[i]);
            }
            mix(s[i]);
        }
    }
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
    for (int t = 0; t < 300; t++) {
        const int n = 1 + irand(t % 10 == 0 ? 2000 : 300), mcs = 2 + irand(7);
        std::vector<int32_t> va, vb;
        std::vector<double> w;
        random_tree(n, t % 2 ? 1 + irand(6) : 0, va, vb, w);
        if (t % 7 == 0)  // self edges are ignored
            for (int i = 0; i < n; i += 3) va.push_back(i), vb.push_back(i), w.push_back(urand());
        const int64_t ne = (int64_t)w.size();
        std::vector<double> s(n), e(n), s2(n);
        std::vector<int32_t> lab(n), lab2(n);
        int64_t k = -1, k2 = -2;
        int rc = guarded([&] {
            return hdb::flat_outlier_scores_host(va.data(), vb.data(), w.data(), ne, n, mcs, s.data(), e.data(), lab.data(), &k);
        });
        rc |= guarded([&] {  // optional outputs off: the same scores
            return hdb::flat_outlier_scores_host(va.data(), vb.data(), w.data(), ne, n, mcs, s2.data(), nullptr, nullptr, nullptr);
        });
        rc |= guarded([&] { return hdb::flat_labels_host(va.data(), vb.data(), w.data(), ne, n, mcs, lab2.data(), &k2); });
        if (rc != 0 || k != k2 || lab != lab2 || memcmp(s.data(), s2.data(), sizeof(double) * n) != 0) {
            bad++;
            printf("tree %d (n %d, mcs %d): status %d, K %lld / %lld\n", t, n, mcs, rc, (long long)k, (long long)k2);
        }
        for (int i = 0; i < n; i++) mix(s[i]), mix(e[i]);
        if (n > 3) {  // not spanning / cycle / bad id / minClSize < 2: the error paths, as flat_labels_host
            auto both = [&](int64_t m, int c) {
                const int r1 = guarded([&] {
                    return hdb::flat_outlier_scores_host(va.data(), vb.data(), w.data(), m, n, c, s.data(), e.data(), lab.data(), &k);
                });
                const int r2 = guarded([&] { return hdb::flat_labels_host(va.data(), vb.data(), w.data(), m, n, c, lab2.data(), &k2); });
                if (r1 != r2 || r1 == 0) bad++, printf("tree %d: error statuses %d / %d\n", t, r1, r2);
            };
            both(n - 2, mcs);
            both(n - 1, 1);
            const int32_t keep = va[0];
            va[0] = va[1], vb[0] = vb[1];  // a doubled edge: cycle
            both(n - 1, mcs);
            va[0] = n + 5;
            both(n - 1, mcs);
            va[0] = keep;
        }
    }
    return bad;
}

int main() {
    int bad = known();
    bad += random_trees();
    printf("host outlier digest %016llx\n", (unsigned long long)digest);
    if (bad) {
        printf("host outlier: %d mismatches\n", bad);
        return 1;
    }
    printf("host outlier ok\n");
    return 0;
}
