// ASan/UBSan driver for the product's host C++: csrc/flat.cpp (global flat
// labels), csrc/formats.cpp (record formats), csrc/local_model.cpp (bubble core epilogue,
// UndirectedGraph quicksort, cluster tree, FOSC + noise reassignment), csrc/inf_edges.cpp (the
// exact leaf's infinite-weight tail, against an all-pairs Kruskal), and common.hpp's Carver (the
// bump allocator every device scratch layout goes through); with --options, csrc/options.cpp (the
// option table and the HDB_OPTS parser).  Built by
// tests/sanitize/Makefile (hipcc --cuda-host-only -fsanitize=address,undefined) and run by
// tests/test_sanitizers.py on tie-heavy seeded inputs and malformed records.  The library's
// error message lives in context.cpp (HIP runtime); a host stub stands in for it here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "internal.hpp"

namespace hdb {
static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
const char *last_error() { return g_error.c_str(); }
}  // namespace hdb

// the library's C-ABI wrapper (guarded) turns hdb::Error into a status code; do the same
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

static void flat() {
    for (int t = 0; t < 40; t++) {
        int n = 1 + irand(2000);
        std::vector<int32_t> va, vb;
        std::vector<double> w;
        random_tree(n, t % 4 == 0 ? 0 : 3 * (t % 5), va, vb, w);
        std::vector<int32_t> lab(n);
        int64_t k = 0;
        for (int mcs = 2; mcs <= 30; mcs += 7)
            guarded([&] { return hdb::flat_labels_host(va.data(), vb.data(), w.data(), n - 1, n, mcs, lab.data(), &k); });
        if (n > 2) {  // not spanning / cycle / bad ids: error paths
            auto fl = [&](int64_t ne) {
                return guarded([&] { return hdb::flat_labels_host(va.data(), vb.data(), w.data(), ne, n, 4, lab.data(), &k); });
            };
            fl(n - 2);
            va[0] = vb[0];
            fl(n - 1);
            va[1] = n + 5;
            fl(n - 1);
        }
    }
}

static void formats() {
    char buf[64];
    for (int i = 0; i < 20000; i++) {
        uint64_t bits = next();
        double v;
        memcpy(&v, &bits, 8);
        hdb_format_double(v, buf, sizeof buf);
        hdb_format_double(std::ldexp(1.0, irand(2098) - 1074), buf, sizeof buf);
    }
    hdb_format_double(1.0, buf, 2);  // too small
    const char *texts[] = {"1 2 3\n4 5 6\n", "1 2 3", "1  2\n", "\n\n", "", "0x1.8p1 2F 1e+2D\n", "1 2\n3\n",
                           "74\t85\t123\t1\n74\t85\t124\t1", "a b c", "1e 2", "+ -", "1 2 3   \r\n4 5 6 \n"};
    for (const char *t : texts)
        for (int strict = 0; strict < 2; strict++)
            for (int d = 0; d < 4; d++) {
                int64_t n = 0;
                int32_t dd = 0;
                hdb_parse_points(t, (int64_t)strlen(t), d, strict, nullptr, 0, &n, &dd);
                std::vector<double> X((size_t)std::max<int64_t>(n * std::max(dd, 1), 1));
                hdb_parse_points(t, (int64_t)strlen(t), d, strict, X.data(), n, &n, &dd);
                hdb_parse_points(t, (int64_t)strlen(t), d, strict, X.data(), 0, &n, &dd);  // capacity error
            }
    std::vector<int32_t> va, vb;
    std::vector<double> w;
    random_tree(500, 0, va, vb, w);
    std::vector<int32_t> f((size_t)va.size(), -7);
    int64_t len = 0;
    hdb_format_mst_records(va.data(), vb.data(), w.data(), f.data(), nullptr, f.data(), (int64_t)va.size(), nullptr, 0, &len);
    std::string s((size_t)len + 1, '\0');
    hdb_format_mst_records(va.data(), vb.data(), w.data(), f.data(), nullptr, f.data(), (int64_t)va.size(), &s[0], len + 1, &len);
    hdb_format_mst_records(va.data(), vb.data(), w.data(), nullptr, nullptr, nullptr, (int64_t)va.size(), &s[0], len / 2, &len);
    s.resize((size_t)len);
    std::vector<int32_t> a(va.size()), b(va.size()), c(va.size());
    std::vector<double> ww(va.size());
    int64_t ne = 0;
    hdb_parse_mst_records(s.data(), (int64_t)s.size(), a.data(), b.data(), ww.data(), c.data(), c.data(), c.data(),
                          (int64_t)a.size(), &ne);
    hdb_parse_mst_records(s.data(), (int64_t)s.size(), a.data(), b.data(), ww.data(), nullptr, nullptr, nullptr, 3, &ne);
    const char *bad[] = {"", "1 2 x", "1 2 0.5", "1 2 0.5 0 0 2147483648", "1 2 1.0E-5 0 0 0\n3 4 5.0 0 0 1\n\n", "\n",
                         " 1 2 3 4 5 6", "1 2 3 4 5 6 7 8"};
    for (const char *t : bad) hdb_parse_mst_records(t, (int64_t)strlen(t), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &ne);
}

static void local_model() {
    for (int t = 0; t < 60; t++) {
        const int b = 2 + irand(400), d = 1 + irand(4), min_pts = 2 + irand(6), K = min_pts - 1;
        std::vector<double> rep((size_t)b * d), eB(b), nnB(b), knn((size_t)b * K), core(b);
        std::vector<int32_t> nB(b), log((size_t)b * K);
        for (auto &x : rep) x = std::round(urand() * 20.0);
        for (int i = 0; i < b; i++) {
            nB[i] = irand(6);  // zeros included: the reference's divide-by-zero path
            eB[i] = irand(3) * 0.5;
            nnB[i] = eB[i];
            double acc = 0;
            for (int k = 0; k < K; k++) {
                acc += irand(3);
                knn[(size_t)i * K + k] = acc;
                log[(size_t)i * K + k] = irand(3) == 0 ? -1 : irand(b);
            }
        }
        guarded([&] { return hdb::bubble_core_epilogue(rep.data(), nB.data(), eB.data(), nnB.data(), b, d, min_pts, 0, knn.data(), log.data(),
                                  core.data()); });
        // MST over the bubbles (random tree) + self edges, as constructMSTBubbles emits them
        std::vector<int32_t> va, vb;
        std::vector<double> w;
        random_tree(b, t % 3 == 0 ? 0 : 4, va, vb, w);
        for (int i = 0; i < b; i++) {
            va.push_back(i), vb.push_back(i), w.push_back(core[i]);
            if (nB[i] == 0) nB[i] = 1;
        }
        std::vector<int32_t> labels(b), iva(2 * b), ivb(2 * b);
        std::vector<double> iw(2 * b);
        int64_t nic = 0;
        for (int mcs = 2; mcs <= 8; mcs += 3) {
            std::vector<int32_t> a = va, bb = vb;
            std::vector<double> ww = w;
            guarded([&] { return hdb::local_model_host(rep.data(), eB.data(), nnB.data(), nB.data(), b, d, mcs, t % 5, a.data(), bb.data(),
                                  ww.data(), labels.data(), iva.data(), ivb.data(), iw.data(), &nic); });
        }
        std::vector<int32_t> a = va, bb = vb;
        std::vector<double> ww = w;
        guarded([&] { return hdb::quicksort_edges(a.data(), bb.data(), ww.data(), (int64_t)ww.size()); });
    }
}

// csrc/inf_edges.cpp against Kruskal over all pairs under (w, s, lo, hi): small inputs with
// overflowing, infinite and NaN rows; the finite edges of Kruskal's tree go in (what K2b's
// device rounds find), its +inf edges must come out, and rows that only NaN pairs reach are counted
static bool inf_tail() {
    struct E {
        double w, s;
        int32_t lo, hi;
    };
    for (int t = 0; t < 60; t++) {
        const int n = 2 + irand(150), d = 1 + irand(4);
        std::vector<double> X((size_t)n * d), core(n);
        for (auto &x : X) x = std::round(urand() * 8.0);
        for (int i = 0; i < n; i++) core[i] = irand(4) == 0 ? -0.0 : irand(3) * 0.5;
        const int bad = t % 6 == 0 ? 0 : 1 + irand(1 + n / 4);
        for (int k = 0; k < bad; k++) {
            const int r = irand(n), c = irand(d);
            switch (t % 5) {
            case 0: X[(size_t)r * d + c] = INFINITY; break;
            case 1: X[(size_t)r * d + c] = (irand(2) ? 1e200 : -1.7e308) * (1 + irand(3)); break;
            case 2: core[r] = INFINITY; break;
            case 3: X[(size_t)r * d + c] = irand(2) ? NAN : -INFINITY; break;
            default: for (int cc = 0; cc < d; cc++) X[(size_t)r * d + cc] = 1e160 * (irand(5) - 2); break;
            }
        }
        std::vector<E> es;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                double u = X[(size_t)p * d] - X[(size_t)q * d], s = u * u;
                for (int c = 1; c < d; c++) {
                    u = X[(size_t)p * d + c] - X[(size_t)q * d + c];
                    s = s + u * u;
                }
                double w = std::sqrt(s);
                if (core[p] > w) w = core[p];
                if (core[q] > w) w = core[q];
                if (w == w) es.push_back(E{w, s, p, q});
            }
        std::sort(es.begin(), es.end(), [](const E &a, const E &b) {
            if (a.w != b.w) return a.w < b.w;
            if (a.s != b.s) return a.s < b.s;
            return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
        });
        std::vector<int32_t> par(n), ea, eb, xa, xb, cnt(n, 0);
        for (int i = 0; i < n; i++) par[i] = i;
        auto find = [&](int32_t x) {
            while (par[x] != x) x = par[x] = par[par[x]];
            return x;
        };
        for (const E &e : es) {
            const int32_t a = find(e.lo), b = find(e.hi);
            if (a == b) continue;
            par[b] = a;
            (e.w < INFINITY ? ea : xa).push_back(e.lo);
            (e.w < INFINITY ? eb : xb).push_back(e.hi);
        }
        int32_t biggest = 0;
        for (int i = 0; i < n; i++) biggest = std::max(biggest, ++cnt[find(i)]);
        std::vector<int32_t> oa(n), ob(n);
        std::vector<double> ow(n);
        int64_t left = -1;
        int32_t first = -2;
        const int64_t added = hdb::inf_edges_host(X.data(), core.data(), n, d, ea.data(), eb.data(), (int64_t)ea.size(),
                                                  oa.data(), ob.data(), ow.data(), &left, &first);
        std::vector<std::pair<int32_t, int32_t>> got, want;
        for (int64_t i = 0; i < added; i++) got.emplace_back(oa[i], ob[i]);
        for (size_t i = 0; i < xa.size(); i++) want.emplace_back(xa[i], xb[i]);
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        bool ok = got == want && left == n - biggest && (left == 0) == (first == -1);
        for (int64_t i = 0; i < added; i++) ok = ok && ow[i] == INFINITY;
        if (!ok) {
            printf("inf_edges_host differs from Kruskal: trial %d n %d d %d added %lld want %zu left %lld\n", t, n, d,
                   (long long)added, want.size(), (long long)left);
            return false;
        }
    }
    return true;
}

// common.hpp's Carver: a layout of mixed types and counts (0 and 1 among them) run once on a null
// base and once on a malloc(off) buffer gives the same offsets, 256-byte aligned, pairwise disjoint
// ranges, the last one ending at off; every element of every range is then written (ASan: in bounds)
static bool carver() {
    struct Range {
        size_t begin, bytes;
    };
    auto layout = [](hdb::Carver &cv, std::vector<Range> &r) {
        auto note = [&](size_t before, size_t elem, int64_t count) {
            r.push_back(Range{before, elem * (size_t)std::max<int64_t>(count, 1)});
        };
        const int64_t counts[] = {0, 1, 3, 64, 65, 257, 1000, 4097};
        for (int64_t c : counts) {
            size_t o = cv.off;
            uint8_t *a = cv.take<uint8_t>(c);
            note(o, 1, c);
            o = cv.off;
            int32_t *b = cv.take<int32_t>(c);
            note(o, 4, c);
            o = cv.off;
            double *d = cv.take<double>(c);
            note(o, 8, c);
            struct Rec24 {
                double x[3];
            };
            o = cv.off;
            Rec24 *e = cv.take<Rec24>(c);
            note(o, sizeof(Rec24), c);
            if (cv.base) {  // write every element; the pointers are where the offsets say
                const int64_t k = std::max<int64_t>(c, 1);
                if ((char *)a != cv.base + r[r.size() - 4].begin || (char *)b != cv.base + r[r.size() - 3].begin ||
                    (char *)d != cv.base + r[r.size() - 2].begin || (char *)e != cv.base + r[r.size() - 1].begin)
                    return false;
                for (int64_t i = 0; i < k; i++) a[i] = 1, b[i] = 2, d[i] = 3.0, e[i].x[2] = 4.0;
            } else if (a || b || d || e) {
                return false;  // a probing carver hands out no pointers
            }
        }
        return true;
    };
    hdb::Carver probe;
    std::vector<Range> pr, ar;
    if (!layout(probe, pr)) return false;
    hdb::Carver cv{(char *)malloc(probe.off)};
    bool ok = layout(cv, ar) && cv.off == probe.off && pr.size() == ar.size();
    for (size_t i = 0; ok && i < ar.size(); i++) {
        ok = pr[i].begin == ar[i].begin && pr[i].bytes == ar[i].bytes && ar[i].begin % 256 == 0;
        // bump order: a range ends at or before the next begins (so all are pairwise disjoint), the last at off
        const size_t next = i + 1 < ar.size() ? ar[i + 1].begin : cv.off;
        ok = ok && ar[i].begin + ar[i].bytes <= next && next - ar[i].begin == ((ar[i].bytes + 255) & ~size_t(255));
    }
    free(cv.base);
    if (!ok) printf("Carver: probing and assigning passes disagree, or a range is misplaced\n");
    return ok;
}

// --options NAME...: the accept matrix of hdb_ctx_set_option (csrc/options.cpp) on a default-constructed
// context.  One line per (name, probe): the status, the message if any and, when a field of the
// context changed, its position in the declaration order of the option fields and its new value.
// Then HDB_OPTS strings through apply_opts: status and message.  tests/golden/option_accept.txt
// holds the output of the if-chain this table replaced.
static int options_matrix(int argc, char **argv) {
    auto fields = [](const hdb_ctx &c) {
        return std::vector<int64_t>{
            c.force_fp64, c.knn_tree, c.knn_tree_min_n, c.knn_mfma, c.knn_mfma_min_n, c.knn_mfma_single,
            c.knn_mfma_prune, c.nearest_grouped, c.boruvka_seed, c.leaf_seed_k, c.leaf_list_rounds,
            c.boruvka_knn_seed, c.boruvka_wave_pts, c.boruvka_early_pts, c.boruvka_early_rounds,
            c.boruvka_adj_seed, c.bor_xcd_chunks, c.k1t_xcd_chunks, c.trav_pop_test, c.prim_coop,
            c.prim_coop_plain, c.bubble_fold_dim, c.bubble_knn_split, c.prim_coop_xcd, c.prim_coop_bs,
            c.prim_coop_plain_spin_log2, c.prim_coop_slots, c.flat_link_variant, c.flat_root_variant,
            c.flat_relabel, c.flat_block_log, c.flat_mid_log, c.flat_deep_depth, c.flat_deep_root,
            c.flat_deep_link, c.ssort, c.ssort_cap, c.count_evals};
    };
    const int64_t two31 = int64_t(1) << 31;
    const int64_t probes[] = {-two31 - 1, -two31, -2,  -1,  0,   1,   2,   3,    4,    5,    6,    7,     8,         9,
                              10,         11,     12,  16,  24,  25,  31,  32,   63,   64,   65,   127,   128,       129,
                              256,        512,    1023, 1024, 1025, 4096, 4097, two31 - 1, two31, int64_t(1) << 40};
    for (int i = 0; i < argc; i++)
        for (int64_t v : probes) {
            hdb_ctx c;
            const std::vector<int64_t> before = fields(c);
            hdb::set_error("");
            const int rc = hdb_ctx_set_option(&c, argv[i], v);
            printf("%s %lld -> %d '%s'", argv[i], (long long)v, rc, hdb::last_error());
            const std::vector<int64_t> after = fields(c);
            for (size_t f = 0; f < after.size(); f++)
                if (after[f] != before[f]) printf(" field %zu = %lld", f, (long long)after[f]);
            printf("\n");
        }
    hdb_ctx c;
    printf("null ctx %d, null name %d\n", hdb_ctx_set_option(nullptr, "ssort", 1), hdb_ctx_set_option(&c, nullptr, 1));
    const char *opts[] = {"flat_block_log=7", "no_such=1", "flat_block_log", "knn_tree_min_n=99999999999999999999",
                          "", ",,", "flat_block_log=9,", "=1", "ssort=0,flat_mid_log=3,,ssort_cap=4097,ssort=1",
                          "ssort= 1", "ssort=1x", "ssort=", "flat_deep_depth=-1"};
    for (const char *o : opts) {
        hdb_ctx k;
        hdb::set_error("");
        const int rc = hdb::apply_opts(&k, o);
        printf("opts '%s' -> %d '%s' ssort %d block_log %d mid_log %d\n", o, rc, hdb::last_error(), (int)k.ssort,
               k.flat_block_log, k.flat_mid_log);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--options")) return options_matrix(argc - 2, argv + 2);
    if (!carver()) return 1;
    // K6 relabel limit (flat.hip): contracted labels nv + rank < 3m must fit int32
    if (!hdb::flat_relabel_fits(715827882) || hdb::flat_relabel_fits(715827883) || !hdb::flat_relabel_fits(0)) {
        printf("flat_relabel_fits limit wrong\n");
        return 1;
    }
    flat();
    formats();
    local_model();
    if (!inf_tail()) return 1;
    printf("host asan ok\n");
    return 0;
}
