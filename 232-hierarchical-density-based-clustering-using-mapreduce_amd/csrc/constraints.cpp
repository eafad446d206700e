// constraints.cpp -- host path of hdb_constrained_flat_labels: the semi-supervised flat
// extraction (HDBSCANStar.calculateNumConstraintsSatisfied :738-789, Cluster.propagate :98-142,
// findProminentClusters) restated over the arrays of hdb_flat_cluster_tree.  DESIGN.md
// "Constrained flat labels" has the rule; csrc/constraints.hip must equal this bit for bit.
//
// With last(x) = point_cluster[x] and L = LCA(last(a), last(b)):
//   must-link   adds 2 to every cluster of anc(L), the root included;
//   cannot-link adds 1 to every cluster from last(a) up to but excluding L, the same for b, and
//               1 per endpoint to the virtual child of last(x) (read only where that cluster splits).
// Both are subtree sums of a difference array: ML diff[L] += 2; CL diff[last(a)] += 1,
// diff[last(b)] += 1, diff[L] -= 2.  A parent's tree label is below its children's, so one
// descending-label loop has every child final before its parent, and the LCA steps the larger
// label up (the larger label is never an ancestor of the smaller).
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "internal.hpp"

namespace hdb {

int constrained_flat_labels_host(const int32_t *parent, const double *stability, const int32_t *min_id, int64_t K,
                                 const int32_t *point_cluster, int64_t n, const int32_t *ca, const int32_t *cb,
                                 const int32_t *ctype, int64_t m, const ConstrainedOut &o) {
    if (m > HDB_MAX_CONSTRAINTS) HDB_THROW(HDB_EINVAL, "constrained flat labels: m exceeds 2^30 - 1 constraints");
    if (K < 0 || n < 0 || m < 0 || (K > 0 && (!parent || !stability || !min_id)) || (n > 0 && !point_cluster) ||
        (m > 0 && (!ca || !cb || !ctype)))
        HDB_THROW(HDB_EINVAL, "bad arguments");
    if (K >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, "constrained flat labels: too many clusters");
    if (n > INT32_MAX) HDB_THROW(HDB_EINVAL, "constrained flat labels: too many points");
    if (o.n_clusters) *o.n_clusters = 0;
    if (K == 0) {  // no tree (n == 0): nothing to select, every point is noise
        if (o.labels) std::fill(o.labels, o.labels + n, 0);
        return HDB_OK;
    }
    // the input is validated, never trusted: every index below is bounded by these checks
    if (parent[0] != 0) HDB_THROW(HDB_EINVAL, "constrained flat labels: parent: the root (label 1) must have parent 0");
    for (int64_t i = 1; i < K; i++)
        if (parent[i] < 0 || parent[i] > i) HDB_THROW(HDB_EINVAL, "constrained flat labels: parent label out of range");
    for (int64_t v = 0; v < n; v++)
        if (point_cluster[v] < 1 || point_cluster[v] > K)
            HDB_THROW(HDB_EINVAL, "constrained flat labels: point_cluster out of range");
    for (int64_t k = 0; k < m; k++)
        if (ca[k] < 0 || ca[k] >= n || cb[k] < 0 || cb[k] >= n)
            HDB_THROW(HDB_EINVAL, "constrained flat labels: constraint point id out of range (ca / cb)");
    for (int64_t k = 0; k < m; k++)
        if (ctype[k] != HDB_CONSTRAINT_MUST_LINK && ctype[k] != HDB_CONSTRAINT_CANNOT_LINK)
            HDB_THROW(HDB_EINVAL, "constrained flat labels: ctype is neither must-link (0) nor cannot-link (1)");

    // indices below are tree labels 1..K (0 = none)
    const size_t S = (size_t)K + 1;
    std::vector<int32_t> par(S, 0), off(S + 1, 0), kids((size_t)K > 0 ? (size_t)K - 1 : 0);
    for (int64_t i = 1; i < K; i++) par[i + 1] = parent[i], off[(size_t)parent[i] + 1]++;
    for (size_t c = 0; c < S; c++) off[c + 1] += off[c];  // children of c: kids[off[c] .. off[c + 1])
    {
        std::vector<int32_t> fill(off.begin(), off.end() - 1);
        for (int64_t c = 2; c <= K; c++) kids[(size_t)fill[par[c]]++] = (int32_t)c;  // ascending label
    }
    // unsigned: the partial sums of a difference array stay within +-2m, and wrap harmlessly
    std::vector<uint32_t> sub(S, 0), virt(S, 0);
    for (int64_t k = 0; k < m; k++) {
        const int32_t la = point_cluster[ca[k]], lb = point_cluster[cb[k]];
        int32_t x = la, y = lb;
        while (x != y) {
            if (x > y) x = par[x];
            else y = par[y];
        }
        if (ctype[k] == HDB_CONSTRAINT_MUST_LINK) {
            sub[x] += 2u;
        } else {
            sub[la] += 1u, sub[lb] += 1u, sub[x] -= 2u;
            virt[la] += 1u, virt[lb] += 1u;
        }
    }
    std::vector<int32_t> csat(S, 0), psat(S, 0);
    std::vector<double> cstab(S, 0.0), pstab(S, 0.0);
    std::vector<char> self(S, 0);
    for (int64_t c = K; c >= 1; c--) {
        const bool leaf = off[c] == off[c + 1];
        uint32_t ps = leaf ? 0u : virt[c];  // the virtual child counts only where the cluster splits
        double pst = 0.0;
        for (int32_t q = off[c]; q < off[c + 1]; q++) {
            const int32_t ch = kids[q];
            sub[c] += sub[ch];
            ps += (uint32_t)csat[ch];
            pst = pst + cstab[ch];  // one addition per child, ascending label
        }
        const int32_t num = (int32_t)sub[c];
        psat[c] = (int32_t)ps, pstab[c] = pst;
        const double st = stability[c - 1];
        self[c] = par[c] != 0 && (leaf || num > psat[c] || (num == psat[c] && st >= pst));
        csat[c] = self[c] ? num : psat[c];
        cstab[c] = self[c] ? st : pst;
        if (o.num_sat) o.num_sat[c - 1] = num;
        if (o.prop_sat) o.prop_sat[c - 1] = psat[c];
        if (o.prop_stability) o.prop_stability[c - 1] = pst;
    }
    // top[c]: the topmost self-chosen cluster on the chain from below the root to c (0: none)
    std::vector<int32_t> top(S, 0), sel, flat(S, 0);
    for (int64_t c = 2; c <= K; c++) {  // a cluster without a parent is a root: never chosen (self is 0)
        top[c] = top[par[c]] ? top[par[c]] : (self[c] ? (int32_t)c : 0);
        if (top[c] == c) sel.push_back((int32_t)c);
    }
    std::sort(sel.begin(), sel.end(), [&](int32_t a, int32_t b) {
        return min_id[a - 1] < min_id[b - 1] || (min_id[a - 1] == min_id[b - 1] && a < b);
    });
    for (size_t i = 0; i < sel.size(); i++) flat[sel[i]] = (int32_t)(i + 1);
    if (o.flat_label)
        for (int64_t c = 1; c <= K; c++) o.flat_label[c - 1] = flat[c];
    if (o.labels)
        for (int64_t v = 0; v < n; v++) o.labels[v] = flat[top[point_cluster[v]]];  // flat[0] = 0
    if (o.n_clusters) *o.n_clusters = (int64_t)sel.size();
    return HDB_OK;
}

}  // namespace hdb
