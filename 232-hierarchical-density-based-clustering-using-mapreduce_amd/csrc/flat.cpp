// flat.cpp -- global HDBSCAN* hierarchy and flat (FOSC / excess-of-mass) labels over the
// merged MST: SURVEY.md §8(f) #1, the step the reference never completes (Main.java:351-408
// exits inside its first level).  Semantics: the canonical top-down procedure of
// HDBSCANStar.computeHierarchyAndClusterTree / propagateTree / findProminentClusters
// (HDBSCANStar.java:208-625, commented out in the reference) with the canonical choices
// listed in oracle/flat_labels.py (tie groups removed together, one stability term per
// (cluster, level), children summed in ascending smallest point id, labels 1..K by smallest
// point id, 0 = noise).
//
// Implementation: bottom-up instead of the Java's repeated BFS (O(levels * n)):
//   1. sort the tree edges by weight; union-find over tie groups builds a multi-way
//      dendrogram (a node = the merge of the components a tie group joins);
//   2. one top-down pass over the dendrogram condenses it (valid child = >= minClSize points)
//      and accumulates each cluster's stability in descending level order, exactly the
//      order the top-down Java visits them;
//   3. FOSC propagation children-before-parents, then one pass labels the points;
//   4. on request, the GLOSH outlier scores (HDBSCANStar.java:505-540, 653-686): step 2 records
//      where each point leaves and each cluster's lowest level, one pass children-before-parents
//      propagates the levels, one pass scores the points;
//   5. on request, the condensed cluster tree itself (hdb_flat_cluster_tree): the clusters of
//      step 2 under canonical tree labels, root first, then (birth descending, smallest member
//      ascending), with where and when each point leaves.
// O(E log E + n) host work; the inputs may live in HBM (staged once).
#include <algorithm>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "internal.hpp"

namespace hdb {

namespace {

struct UF {
    std::vector<int32_t> p;
    explicit UF(int64_t n) : p((size_t)n) { std::iota(p.begin(), p.end(), 0); }
    int32_t find(int32_t x) {
        while (p[x] != x) {
            p[x] = p[p[x]];
            x = p[x];
        }
        return x;
    }
};

struct Node {  // dendrogram node; ids 0..n-1 are the points
    double level;
    int64_t size;
    int32_t minid;
    int32_t first_child, n_children;  // into child_pool
};

struct Clu {
    double birth;
    int32_t parent;
    int32_t node;   // dendrogram node at birth
    int32_t minid;
    double stab = 0.0;
    std::vector<int32_t> kids;  // ascending minid
};

// labels / n_clusters: the flat partition (labels nullable).  scores / noise (nullable): GLOSH
// outlier scores and eps(x) from the same hierarchy (see flat_outlier_scores_host below).
// tree (nullable): the cluster tree's arrays (flat_cluster_tree_host).
int flat_host_impl(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n, int32_t mcs,
                   int32_t *labels, int64_t *n_clusters, double *scores, double *noise,
                   const ClusterTreeOut *tree = nullptr) {
    if (n <= 0) {
        if (n_clusters) *n_clusters = 0;
        if (tree) *tree->n_tree = 0;
        return HDB_OK;
    }
    if (mcs < 2) HDB_THROW(HDB_EINVAL, "flat labels: minClSize must be >= 2");
    std::vector<int64_t> e;
    e.reserve((size_t)std::max<int64_t>(ne, 0));
    for (int64_t i = 0; i < ne; i++) {
        if (va[i] == vb[i]) continue;  // self edges (core distances) carry no split for minClSize >= 2
        if (va[i] < 0 || vb[i] < 0 || va[i] >= n || vb[i] >= n) HDB_THROW(HDB_EINVAL, "flat labels: vertex id out of range");
        if (w[i] != w[i]) HDB_THROW(HDB_EINVAL, "flat labels: NaN edge weight");
        e.push_back(i);
    }
    if ((int64_t)e.size() != n - 1) HDB_THROW(HDB_EINVAL, "flat labels: the edges are not a spanning tree");
    std::sort(e.begin(), e.end(), [&](int64_t a, int64_t b) { return w[a] < w[b] || (w[a] == w[b] && a < b); });

    // ---- 1. multi-way dendrogram over tie groups
    std::vector<Node> nodes((size_t)n);
    for (int64_t i = 0; i < n; i++) nodes[i] = Node{0.0, 1, (int32_t)i, -1, 0};
    std::vector<int32_t> pool;
    pool.reserve((size_t)(2 * n));
    UF uf(n);
    std::vector<int32_t> comp_node((size_t)n);  // UF root -> current dendrogram node
    std::iota(comp_node.begin(), comp_node.end(), 0);
    std::vector<int32_t> pre_a, pre_b, stamp((size_t)(2 * n), -1), root_slot((size_t)n, -1);  // stamp: node ids < 2n
    std::vector<std::vector<int32_t>> groups;
    for (size_t g0 = 0; g0 < e.size();) {
        size_t g1 = g0;
        // -0.0 and 0.0 are one level, +0.0 whichever edge leads the group: 1 / level (the
        // stability terms here and at the children born at it) and the GLOSH level read this value
        const double lev = w[e[g0]] == 0.0 ? 0.0 : w[e[g0]];
        while (g1 < e.size() && w[e[g1]] == lev) g1++;
        const size_t m = g1 - g0;
        pre_a.resize(m);
        pre_b.resize(m);
        for (size_t k = 0; k < m; k++) {  // components before the group
            pre_a[k] = comp_node[uf.find(va[e[g0 + k]])];
            pre_b[k] = comp_node[uf.find(vb[e[g0 + k]])];
        }
        for (size_t k = 0; k < m; k++) {
            int32_t ra = uf.find(va[e[g0 + k]]), rb = uf.find(vb[e[g0 + k]]);
            if (ra == rb) HDB_THROW(HDB_EINVAL, "flat labels: the edges contain a cycle");
            uf.p[rb] = ra;
        }
        // one new node per resulting component, children = distinct pre-group nodes
        groups.clear();
        std::vector<int32_t> roots;
        for (size_t k = 0; k < m; k++) {
            const int32_t r = uf.find(va[e[g0 + k]]);
            if (root_slot[r] < 0) {
                root_slot[r] = (int32_t)groups.size();
                groups.emplace_back();
                roots.push_back(r);
            }
            auto &kids = groups[(size_t)root_slot[r]];
            for (int32_t c : {pre_a[k], pre_b[k]}) {
                if (stamp[c] != (int32_t)g0) {
                    stamp[c] = (int32_t)g0;
                    kids.push_back(c);
                }
            }
        }
        for (size_t gi = 0; gi < roots.size(); gi++) {
            auto &kids = groups[gi];
            Node nd{lev, 0, INT32_MAX, (int32_t)pool.size(), (int32_t)kids.size()};
            for (int32_t c : kids) {
                nd.size += nodes[c].size;
                nd.minid = std::min(nd.minid, nodes[c].minid);
                pool.push_back(c);
            }
            comp_node[roots[gi]] = (int32_t)nodes.size();
            nodes.push_back(nd);
            root_slot[roots[gi]] = -1;
        }
        g0 = g1;
    }
    const int32_t root = n == 1 ? 0 : (int32_t)nodes.size() - 1;

    // ---- 2. condense top-down; stability terms in descending level per cluster
    std::vector<Clu> cl;
    cl.push_back(Clu{NAN, -1, root, nodes[root].minid});
    std::vector<std::pair<int32_t, int32_t>> stack;  // (node, cluster)
    if (n > 1) stack.push_back({root, 0});
    std::vector<int32_t> valid;
    // outlier scores: a point leaves (becomes noise) at the reached node whose invalid child
    // holds it -- eps(x) = that node's level, last(x) = that node's cluster; a cluster's own
    // lowest level is the level of the last node on its chain (levels fall along it)
    const bool want_scores = scores != nullptr || tree != nullptr;
    std::vector<double> eps_pt, death;
    std::vector<int32_t> last_pt, sub;
    if (want_scores) {
        eps_pt.assign((size_t)n, 0.0);
        last_pt.assign((size_t)n, 0);
        death.assign(1, 0.0);
    }
    while (!stack.empty()) {
        auto [x, L] = stack.back();
        stack.pop_back();
        const Node &X = nodes[x];
        const double eps = X.level;
        valid.clear();
        int64_t invalid_pts = 0;
        for (int32_t k = 0; k < X.n_children; k++) {
            int32_t c = pool[X.first_child + k];
            if (nodes[c].size >= mcs) {
                valid.push_back(c);
                continue;
            }
            invalid_pts += nodes[c].size;
            if (!want_scores) continue;
            sub.assign(1, c);  // every point below an invalid child leaves here
            while (!sub.empty()) {
                const int32_t y = sub.back();
                sub.pop_back();
                if (y < n) {
                    eps_pt[y] = eps;
                    last_pt[y] = L;
                    continue;
                }
                for (int32_t q = 0; q < nodes[y].n_children; q++) sub.push_back(pool[nodes[y].first_child + q]);
            }
        }
        if (want_scores) {
            death.resize(cl.size() + (valid.size() >= 2 ? valid.size() : 0), 0.0);
            death[L] = eps;  // descending along the chain: the last write is the lowest
        }
        const double inv_birth = 1.0 / cl[L].birth;
        if (valid.size() >= 2) {
            cl[L].stab += (double)X.size * (1.0 / eps - inv_birth);  // Cluster.detachPoints
            std::sort(valid.begin(), valid.end(), [&](int32_t a, int32_t b) { return nodes[a].minid < nodes[b].minid; });
            for (int32_t c : valid) {
                cl[L].kids.push_back((int32_t)cl.size());
                cl.push_back(Clu{eps, L, c, nodes[c].minid});
            }
            // push in reverse so the smallest-minid child is condensed first (order-free)
            for (size_t k = valid.size(); k-- > 0;) stack.push_back({valid[k], cl[L].kids[cl[L].kids.size() - valid.size() + k]});
        } else if (valid.size() == 1) {
            if (invalid_pts > 0) cl[L].stab += (double)invalid_pts * (1.0 / eps - inv_birth);
            stack.push_back({valid[0], L});
        } else {
            cl[L].stab += (double)X.size * (1.0 / eps - inv_birth);
        }
    }

    // ---- 3. FOSC propagation (children were created after their parent)
    const int64_t nc = (int64_t)cl.size();
    std::vector<double> contrib((size_t)nc, 0.0);
    std::vector<char> self_sel((size_t)nc, 0);
    for (int64_t c = nc - 1; c >= 1; c--) {
        double prop = 0.0;
        for (int32_t k : cl[c].kids) prop = prop + contrib[k];
        if (cl[c].kids.empty() || cl[c].stab >= prop) {  // Cluster.propagate: ties keep the parent
            contrib[c] = cl[c].stab;
            self_sel[c] = 1;
        } else {
            contrib[c] = prop;
        }
    }
    std::vector<int32_t> sel, todo(cl[0].kids.begin(), cl[0].kids.end());
    while (!todo.empty()) {
        int32_t c = todo.back();
        todo.pop_back();
        if (self_sel[c]) sel.push_back(c);
        else todo.insert(todo.end(), cl[c].kids.begin(), cl[c].kids.end());
    }
    std::sort(sel.begin(), sel.end(), [&](int32_t a, int32_t b) { return cl[a].minid < cl[b].minid; });
    if (labels) std::fill(labels, labels + n, 0);
    std::vector<int32_t> dfs;
    for (size_t i = 0; labels && i < sel.size(); i++) {
        dfs.assign(1, cl[sel[i]].node);
        while (!dfs.empty()) {
            int32_t x = dfs.back();
            dfs.pop_back();
            if (x < n) {
                labels[x] = (int32_t)(i + 1);
                continue;
            }
            for (int32_t k = 0; k < nodes[x].n_children; k++) dfs.push_back(pool[nodes[x].first_child + k]);
        }
    }
    if (n_clusters) *n_clusters = (int64_t)sel.size();

    // ---- 5. the cluster tree under canonical labels: 1 = the root, 2.. by (birth level
    // descending, smallest member ascending) -- total, since clusters born at one level are
    // disjoint; a parent is born above its children, so its label is the smaller one
    if (tree) {
        *tree->n_tree = nc;
        if (tree->cap < nc)
            HDB_THROW(HDB_EINVAL, "cluster tree: capacity " + std::to_string(tree->cap) + " is below the " +
                                      std::to_string(nc) + " clusters of the tree");
        std::vector<int32_t> order((size_t)nc), newlab((size_t)nc), flat_of((size_t)nc, 0);
        std::iota(order.begin(), order.end(), 0);
        std::sort(order.begin() + 1, order.end(), [&](int32_t a, int32_t b) {
            return cl[a].birth > cl[b].birth || (cl[a].birth == cl[b].birth && cl[a].minid < cl[b].minid);
        });
        for (int64_t i = 0; i < nc; i++) newlab[order[i]] = (int32_t)(i + 1);
        for (size_t i = 0; i < sel.size(); i++) flat_of[sel[i]] = (int32_t)(i + 1);
        auto level = [](double x) { return x == 0.0 ? 0.0 : x; };  // -0.0 and 0.0 are one level
        for (int64_t i = 0; i < nc; i++) {
            const int32_t c = order[i];
            if (tree->parent) tree->parent[i] = c ? newlab[cl[c].parent] : 0;
            if (tree->birth) tree->birth[i] = level(cl[c].birth);
            if (tree->death) tree->death[i] = level(death[c]);
            if (tree->stability) tree->stability[i] = cl[c].stab;
            if (tree->size) tree->size[i] = (int32_t)nodes[cl[c].node].size;
            if (tree->min_id) tree->min_id[i] = cl[c].minid;
            if (tree->flat_label) tree->flat_label[i] = flat_of[c];
        }
        for (int64_t v = 0; v < n; v++) {
            if (tree->point_cluster) tree->point_cluster[v] = newlab[last_pt[v]];
            if (tree->point_level) tree->point_level[v] = level(eps_pt[v]);
        }
    }

    // ---- 4. GLOSH: eps_max(C) = the lowest level among C and its descendants
    // (Cluster.propagate's propagatedLowestChildDeathLevel, Cluster.java:99-105); the root
    // takes its descendants only and keeps Double.MAX_VALUE when it never splits
    if (scores) {
        std::vector<double> eps_max(death);
        eps_max[0] = std::numeric_limits<double>::max();
        for (int64_t c = nc - 1; c >= 1; c--) eps_max[cl[c].parent] = std::min(eps_max[cl[c].parent], eps_max[c]);
        for (int64_t v = 0; v < n; v++) {  // n == 1: no level at all, eps = 0
            const double e = eps_pt[v];
            scores[v] = e == 0.0 ? 0.0 : 1.0 - eps_max[last_pt[v]] / e;  // calculateOutlierScores :662-667
            if (noise) noise[v] = e == 0.0 ? 0.0 : e;  // a -0.0 level is reported as 0.0, as the device does
        }
    }
    return HDB_OK;
}

}  // namespace

int flat_labels_host(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n, int32_t mcs,
                     int32_t *labels, int64_t *n_clusters) {
    return flat_host_impl(va, vb, w, ne, n, mcs, labels, n_clusters, nullptr, nullptr);
}

// GLOSH outlier scores (HDBSCANStar.propagateTree :505-540 + calculateOutlierScores :653-686)
// over the hierarchy above: score(x) = eps(x) == 0 ? 0 : 1 - eps_max(last(x)) / eps(x).
// labels, n_clusters and noise (eps per point) are optional outputs of the same pass.
int flat_outlier_scores_host(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                             int32_t mcs, double *scores, double *noise, int32_t *labels, int64_t *n_clusters) {
    return flat_host_impl(va, vb, w, ne, n, mcs, labels, n_clusters, scores, noise);
}

// The condensed cluster tree of the hierarchy above (HDBSCANStar.computeHierarchyAndClusterTree
// :208-474), canonical tree labels; labels and n_clusters as flat_labels_host (nullable).
int flat_cluster_tree_host(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                           int32_t mcs, const ClusterTreeOut &tree, int32_t *labels, int64_t *n_clusters) {
    return flat_host_impl(va, vb, w, ne, n, mcs, labels, n_clusters, nullptr, nullptr, &tree);
}

// hierarchy rows at arbitrary levels: label(x, eps) = 0 below eps(x), else the first cluster on
// the chain from last(x) to the root that is not born at or below eps (the root's NaN birth
// stops the climb).  One top-down pass over the clusters per level (a parent's label is below
// its children's), then one lookup per point.
int labels_at_levels_host(const int32_t *parent, const double *birth, int64_t K, const int32_t *point_cluster,
                          const double *point_level, int64_t n, const double *levels, int32_t L,
                          int32_t *labels_out) {
    if (K < 0 || n < 0 || L < 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    for (int32_t l = 0; l < L; l++)
        if (levels[l] != levels[l]) HDB_THROW(HDB_EINVAL, "labels at levels: NaN level");
    if (L == 0 || n == 0) return HDB_OK;
    if (K >= INT32_MAX) HDB_THROW(HDB_EINVAL, "labels at levels: too many clusters");
    if (K > 0 && parent[0] != 0) HDB_THROW(HDB_EINVAL, "labels at levels: the root (label 1) must have parent 0");
    for (int64_t i = 1; i < K; i++)
        if (parent[i] < 0 || parent[i] > i) HDB_THROW(HDB_EINVAL, "labels at levels: parent label out of range");
    for (int64_t v = 0; v < n; v++)
        if (point_cluster[v] < 1 || point_cluster[v] > K)
            HDB_THROW(HDB_EINVAL, "labels at levels: point cluster out of range");
    std::vector<int32_t> res((size_t)K + 1);
    for (int32_t l = 0; l < L; l++) {
        const double eps = levels[l];
        res[0] = 0;
        for (int64_t i = 0; i < K; i++) res[i + 1] = birth[i] <= eps ? res[parent[i]] : (int32_t)(i + 1);
        int32_t *row = labels_out + (int64_t)l * n;
        for (int64_t v = 0; v < n; v++) row[v] = eps < point_level[v] ? 0 : res[point_cluster[v]];
    }
    return HDB_OK;
}

// hdb_predict_labels on host arrays: the plain walk.  Query i attached at (y, e) = (nearest[i],
// level[i]) starts at point_cluster[y] and climbs while birth <= e (the root's NaN birth stops it);
// its flat label is that of the nearest selected cluster from there to the root; its score is GLOSH
// at eps = max(e, point_level[y]) with the eps_max of hdb_flat_outlier_scores (the subtree minimum
// of death; the root takes its descendants only, from Double.MAX_VALUE).  Minima are taken under
// the order of the device's integer keys (-0.0 below +0.0), so both paths give the same bits.
int predict_labels_host(const int32_t *parent, const double *birth, const double *death, const int32_t *flat_label,
                        int64_t K, const int32_t *point_cluster, const double *point_level, int64_t n,
                        const int32_t *nearest, const double *level, int64_t m, int32_t *tree_label, int32_t *labels,
                        double *scores) {
    if (K < 0 || n < 0 || m < 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    if (m == 0) return HDB_OK;
    if (K >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, "predict labels: too many clusters");
    if (K > 0 && parent[0] != 0) HDB_THROW(HDB_EINVAL, "predict labels: the root (label 1) must have parent 0");
    for (int64_t i = 1; i < K; i++)
        if (parent[i] < 0 || parent[i] > i) HDB_THROW(HDB_EINVAL, "predict labels: parent label out of range");
    for (int64_t v = 0; v < n; v++)
        if (point_cluster[v] < 1 || point_cluster[v] > K)
            HDB_THROW(HDB_EINVAL, "predict labels: point_cluster out of range");
    for (int64_t i = 0; i < m; i++)
        if (nearest[i] < -1 || nearest[i] >= n) HDB_THROW(HDB_EINVAL, "predict labels: nearest out of range");
    for (int64_t i = 0; i < m; i++)
        if (nearest[i] >= 0 && level[i] != level[i]) HDB_THROW(HDB_EINVAL, "predict labels: NaN level");
    auto key = [](double x) {
        uint64_t u;
        std::memcpy(&u, &x, 8);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    };
    // by tree label (index 0: none): eps_max and the flat label of the nearest selected cluster
    // on the way up; a parent's label is below its children's
    std::vector<double> eps_max((size_t)K + 1, std::numeric_limits<double>::max());
    std::vector<int32_t> near((size_t)K + 1, 0);
    for (int64_t c = 2; c <= K; c++) eps_max[c] = death[c - 1];
    for (int64_t c = K; c >= 2; c--) {
        const int32_t p = parent[c - 1];
        if (p > 0 && key(eps_max[c]) < key(eps_max[p])) eps_max[p] = eps_max[c];
    }
    for (int64_t c = 1; c <= K; c++) near[c] = flat_label[c - 1] != 0 ? flat_label[c - 1] : near[parent[c - 1]];
    for (int64_t i = 0; i < m; i++) {
        const int32_t y = nearest[i];
        int32_t C = 0;
        double sc = 1.0;
        if (y >= 0) {
            const double e = level[i];
            C = point_cluster[y];
            while (C > 0 && birth[C - 1] <= e) C = parent[C - 1];
            const double pl = point_level[y], eps = pl > e ? pl : e;
            sc = eps == 0.0 ? 0.0 : 1.0 - eps_max[C] / eps;  // C == 0 (a malformed tree's walk): MAX_VALUE
        }
        if (tree_label) tree_label[i] = C;
        if (labels) labels[i] = near[C];
        if (scores) scores[i] = sc;
    }
    return HDB_OK;
}

}  // namespace hdb
