// soft.cpp -- the host side of soft clustering (include/hdbmi.h "soft clustering"): the exemplar
// selection of hdb_exemplars and the host path of hdb_membership_vectors.  Plain loops over the
// arrays of the cluster tree, in the operation order the contract fixes (FP64, no contraction,
// sums over clusters in ascending flat label); soft.hip computes the same bits on the device.
#include <cmath>
#include <limits>

#include "internal.hpp"

namespace hdb {

namespace {

// the tree checks of hdb_labels_at_levels plus the selection's range
void soft_check_tree(const int32_t *parent, const int32_t *flat_label, int64_t K, int64_t C, const char *what) {
    const std::string w(what);
    if (K >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, w + ": too many clusters");
    if (C >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, w + ": too many selected clusters");
    if (K > 0 && parent[0] != 0) HDB_THROW(HDB_EINVAL, w + ": the root (label 1) must have parent 0");
    for (int64_t i = 1; i < K; i++)
        if (parent[i] < 0 || parent[i] > i) HDB_THROW(HDB_EINVAL, w + ": parent label out of range");
    for (int64_t i = 0; i < K; i++)
        if (flat_label[i] < 0 || flat_label[i] > C) HDB_THROW(HDB_EINVAL, w + ": flat_label out of range");
}

}  // namespace

// hdb_exemplars on host arrays.  ids has room for n entries, offsets for C + 1; returns the count.
int64_t exemplars_host(const int32_t *parent, const int32_t *flat_label, int64_t K, int64_t C,
                       const int32_t *point_cluster, const double *point_level, int64_t n, int32_t *ids,
                       int64_t *offsets) {
    if (K < 0 || C < 0 || n < 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    if (n > (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "exemplars: n must be below 2^31 (int32 ids)");
    soft_check_tree(parent, flat_label, K, C, "exemplars");
    for (int64_t v = 0; v < n; v++)
        if (point_cluster[v] < 1 || point_cluster[v] > K) HDB_THROW(HDB_EINVAL, "exemplars: point_cluster out of range");
    // by tree label (index 0: none): leaf flag, the smallest point level under '<' (a NaN level is
    // never the smallest and never equal to it), the flat label of the nearest selected cluster
    std::vector<char> leaf((size_t)K + 1, 1);
    std::vector<double> low((size_t)K + 1, std::numeric_limits<double>::infinity());
    std::vector<int32_t> near((size_t)K + 1, 0);
    for (int64_t c = 1; c <= K; c++) leaf[parent[c - 1]] = 0;
    for (int64_t c = 1; c <= K; c++) near[c] = flat_label[c - 1] != 0 ? flat_label[c - 1] : near[parent[c - 1]];
    for (int64_t v = 0; v < n; v++)
        if (point_level[v] < low[point_cluster[v]]) low[point_cluster[v]] = point_level[v];
    const auto flat_of = [&](int64_t v) -> int32_t {
        const int32_t c = point_cluster[v];
        return leaf[c] && point_level[v] == low[c] ? near[c] : 0;
    };
    for (int64_t f = 0; f <= C; f++) offsets[f] = 0;
    for (int64_t v = 0; v < n; v++) {
        const int32_t f = flat_of(v);
        if (f > 0) offsets[f]++;  // the count of f, one slot up: the prefix sum below turns it into f's end
    }
    for (int64_t f = 1; f <= C; f++) offsets[f] += offsets[f - 1];
    const int64_t E = offsets[C];
    // ascending id inside each segment: fill from the starts, which are the previous segment's ends
    std::vector<int64_t> at((size_t)C + 1, 0);
    for (int64_t f = 1; f <= C; f++) at[f] = offsets[f - 1];
    for (int64_t v = 0; v < n; v++) {
        const int32_t f = flat_of(v);
        if (f > 0) ids[at[f]++] = (int32_t)v;
    }
    return E;
}

// hdb_membership_vectors on host arrays: the plain walk.  For the pair (query anchored at a,
// selected cluster c) the climb from c stops at the first cluster that is a or one of a's
// ancestors; the step before it is the child whose birth is the merge level.
int membership_vectors_host(const int32_t *parent, const double *birth, const double *death,
                            const int32_t *flat_label, int64_t K, int64_t C, const int32_t *anchor,
                            const double *level, const double *dmin, int64_t m, double *vectors, double *prob,
                            int32_t *labels) {
    if (K < 0 || C < 0 || m < 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    if (m == 0) return HDB_OK;
    soft_check_tree(parent, flat_label, K, C, "membership vectors");
    for (int64_t i = 0; i < m; i++)
        if (anchor[i] < 0 || anchor[i] > K) HDB_THROW(HDB_EINVAL, "membership vectors: anchor out of range");
    auto key = [](double x) {
        uint64_t u;
        std::memcpy(&u, &x, 8);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    };
    // eps_max by tree label as hdb_predict_labels has it; sel[f]: the lowest tree label that carries f
    std::vector<double> eps_max((size_t)K + 1, std::numeric_limits<double>::max());
    for (int64_t c = 2; c <= K; c++) eps_max[c] = death[c - 1];
    for (int64_t c = K; c >= 2; c--) {
        const int32_t p = parent[c - 1];
        if (p > 0 && key(eps_max[c]) < key(eps_max[p])) eps_max[p] = eps_max[c];
    }
    std::vector<int32_t> sel((size_t)C + 1, 0);
    for (int64_t c = K; c >= 1; c--)
        if (flat_label[c - 1] > 0) sel[flat_label[c - 1]] = (int32_t)c;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<char> mark((size_t)K + 1, 0);
    std::vector<double> t((size_t)C), p((size_t)C);
    for (int64_t i = 0; i < m; i++) {
        const int32_t a = anchor[i];
        const double l = level[i];
        const double *dm = dmin + i * C;
        double *row = vectors + i * C;
        if (a == 0) {
            for (int64_t f = 0; f < C; f++) row[f] = 0.0;
            if (prob) prob[i] = 0.0;
            if (labels) labels[i] = 0;
            continue;
        }
        for (int32_t x = a; x > 0; x = parent[x - 1]) mark[x] = 1;
        double mx = 0.0, S = 0.0;
        int64_t nz = 0;
        for (int64_t f = 0; f < C; f++) {
            const int32_t c = sel[f + 1];
            double tf = 0.0;
            if (c > 0) {
                int32_t prev = 0, cur = c;
                while (cur > 0 && !mark[cur]) {
                    prev = cur;
                    cur = parent[cur - 1];
                }
                const double B = prev == 0 ? -inf : birth[prev - 1];
                const double M = B > l ? B : l;
                tf = M == 0.0 ? 1.0 : eps_max[c] / M;
            }
            t[f] = tf;
            if (tf > mx) mx = tf;
            if (dm[f] <= 0.0)
                nz++;
            else
                S = S + (dm[f] == inf ? 0.0 : 1.0 / dm[f]);
        }
        for (int32_t x = a; x > 0; x = parent[x - 1]) mark[x] = 0;
        const double pr = 1.0 < mx ? 1.0 : mx;
        double P = 0.0;
        for (int64_t f = 0; f < C; f++) {
            double dv;
            if (nz > 0)
                dv = dm[f] <= 0.0 ? 1.0 / (double)nz : 0.0;
            else
                dv = S == 0.0 ? 0.0 : (dm[f] == inf ? 0.0 : 1.0 / dm[f]) / S;
            p[f] = dv * t[f];
            P = P + p[f];
        }
        int32_t lab = 0;
        double best = 0.0;
        for (int64_t f = 0; f < C; f++) {
            const double v = P == 0.0 ? 0.0 : pr * (p[f] / P);
            row[f] = v;
            if (v > best) {
                best = v;
                lab = (int32_t)(f + 1);
            }
        }
        if (prob) prob[i] = pr;
        if (labels) labels[i] = lab;
    }
    return HDB_OK;
}

}  // namespace hdb
