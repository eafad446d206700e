// internal.hpp -- device-side building blocks shared by the C-ABI layer.
#pragma once
#include <algorithm>
#include <new>
#include <type_traits>

#include "common.hpp"

namespace hdb {

// The guard of the C ABI: every extern "C" function that can throw runs its body through entry()
// or guarded(), so no exception leaves the library.  f returns a status, or nothing for HDB_OK.
template <class F>
int entry(F &&f) {
    try {
        if constexpr (std::is_void_v<decltype(f())>) {
            f();
            return HDB_OK;
        } else {
            return f();
        }
    } catch (const Error &e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return HDB_ENOMEM;
    }
}
// entry() for a call that runs on ctx's device
template <class F>
int guarded(hdb_ctx *ctx, F &&f) {
    return entry([&] {
        if (!ctx) HDB_THROW(HDB_EINVAL, "ctx is NULL");
        HIP_CHECK(hipSetDevice(ctx->device));
        return f();
    });
}

struct PrimIn {
    const double *X;
    const double *core;
    const int32_t *ids;
    const double *eB;
    const double *nnB;
    int d;
    int metric;
};

void pack_rows(hdb_ctx *ctx, const double *X, int64_t n, int d, int dp, double *Xp);
void knn_lists_device(hdb_ctx *ctx, const double *X_dev, int64_t n, int d, int k, int metric, bool excl,
                      double *lists_v, int32_t *lists_i, int *KC_out);
void core_epilogue_device(hdb_ctx *ctx, const double *lists, int64_t n, int KC, int K, int semantics, double *core);
// list bucket for k neighbours (K1/K1t keep KC >= k values per row)
inline int pick_kc(int k) {
    if (k <= 1) return 1;
    if (k <= 3) return 3;
    if (k <= 7) return 7;
    if (k <= 15) return 15;
    if (k <= 31) return 31;
    return -1;
}
void core_distances_device(hdb_ctx *ctx, const double *X_dev, int64_t n, int d, int min_pts, int metric,
                           int semantics, double *core);
void prim_batched_device(hdb_ctx *ctx, const PrimIn &in, const int64_t *h_offs, int P, int self_edges, int32_t *va,
                         int32_t *vb, double *w);
void leaf_cores_device(hdb_ctx *ctx, const double *X, int d, int metric, int P, const int64_t *d_off,
                       const int32_t *d_parts, int np, int64_t total_rows, int K, double *core);
void nearest_sample_device(hdb_ctx *ctx, const double *X, int64_t n, const double *S, int64_t m, int d, int metric,
                           const int32_t *xkey, const int32_t *skey, int32_t *out_i, double *out_d);
void bubble_stats_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const int32_t *bo, int64_t nb, int variant,
                         double *ls, double *ss, double *rep, double *info);
void bubble_partials_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const int32_t *bo, int64_t nb,
                            const int64_t *h_cuts, int S, double *pls, double *pss, double *pn);
void bubble_combine_device(hdb_ctx *ctx, const double *pls, const double *pss, const double *pn, int S, int64_t nb,
                           int d, double *ls, double *ss, double *rep, double *info);
void bubble_knn_device(hdb_ctx *ctx, const double *rep, const double *eB, const double *nnB, int64_t b, int d,
                       int metric, int K, double *knn_out, int32_t *log_out);
void sort_edges_desc_device(hdb_ctx *ctx, int32_t *va, int32_t *vb, double *w, int64_t ne);
// stable merge of two descending runs held in separate arrays (A first on equal weights)
void merge_two_runs_device(hdb_ctx *ctx, const int32_t *aA, const int32_t *bA, const double *wA, int64_t na,
                           const int32_t *aB, const int32_t *bB, const double *wB, int64_t nb, int32_t *oa,
                           int32_t *ob, double *ow);
// CreateLocalMST record fields: local indices of each edge's vertices in `ids` (synchronises)
void merge_sorted_runs_device(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w,
                              const std::vector<int64_t> &off, int32_t *oa, int32_t *ob, double *ow);
void local_mst_ids_device(hdb_ctx *ctx, const int32_t *ids, int64_t n, const int32_t *va, const int32_t *vb,
                          const double *w, int64_t ne,
                          int32_t node, int32_t *fake1, int32_t *fake2, int32_t *node_out);
void distance_rows_device(hdb_ctx *ctx, const double *a, const double *b, int64_t n, int d, int metric, double *out);
bool knn_tree_device(hdb_ctx *ctx, const double *X, int64_t n, int d, int KC, bool excl, double *lists);
// K1m: MFMA-screened exact lists for 16 < d <= 256 (false: not applicable, use the FP64 scan)
bool knn_mfma_device(hdb_ctx *ctx, const double *X, int64_t n, int d, int KC, bool excl, double *lists);
// self edges (v, v, core[v]) as FirstStep emits them after the tree edges (HDBSCANStar.java:190-203)
void self_edges_device(hdb_ctx *ctx, const double *core, int64_t n, int32_t *va, int32_t *vb, double *w);
void exact_leaf_device(hdb_ctx *ctx, const double *X, int64_t n, int d, int min_pts, int metric, int semantics,
                       double *core, int self_edges, int32_t *va, int32_t *vb, double *w);
void boruvka_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const double *core, int metric, int32_t *va,
                    int32_t *vb, double *w);
// K2g (boruvka_generic.hip): the same contract for every metric and d by a tiled all-pairs FP64
// scan; boruvka_device routes to it whatever K2b's index does not cover
void boruvka_generic_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const double *core, int metric,
                            int32_t *va, int32_t *vb, double *w);
// its tile constants and round count as stats (boruvka_gen_qt / _ct / _dc / _rounds)
void boruvka_generic_stats_init(hdb_ctx *ctx);
// the attach scan of out-of-sample prediction (attach.hip): per query row its core distance
// against the training rows (core_q, nullable) and its cheapest mutual-reachability edge into them
// (nearest, level); splits: candidate columns over grid.y (0: chosen from m and n); all arrays on
// the device, stream-ordered
void attach_points_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const double *core, const double *Q,
                          int64_t m, int min_pts, int metric, int splits, double *core_q, int32_t *nearest,
                          double *level);
void attach_stats_init(hdb_ctx *ctx);  // stat attach_last_splits
// hdb_validity_index (validity.hip): the K-length results and the index are host values, entry c - 1
// for label c
struct ValidityResult {
    double index = 0.0;
    std::vector<double> validity, sparseness, separation;
    std::vector<int32_t> nearest, size;
};
constexpr int32_t VALIDITY_SMALL_LIMIT = 2048;  // members the small-cluster Prim holds in LDS, at most
// the DBCV index of a labelling; X, labels and the nullable n-length outputs on the device; splits:
// candidate columns of both scans over grid.y (0: chosen); small_max: clusters up to this size share the
// one Prim launch, larger ones go through boruvka_device (0: all of them); synchronises
void validity_index_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const int32_t *labels, int32_t K,
                           int metric, int splits, int32_t small_max, ValidityResult &res, double *core_out,
                           int32_t *internal_out);
void validity_stats_init(hdb_ctx *ctx);  // stats validity_last_splits, validity_last_core_splits
// its host epilogue (validity.cpp)
void validity_cores_host(const double *totals, const int64_t *off, int32_t K, int d, double *cores);
void validity_finish_host(ValidityResult &r, int64_t n);
// soft clustering (soft.hip, soft.cpp; include/hdbmi.h "soft clustering")
// the exemplar-distance scan: dmin (m x C) = per query row and segment of ids the smallest
// dist(Q[i], X[ids[e]]); every array on the device; ids and offsets are validated on the device
// (one word read back) before anything is written; splits: candidate columns over grid.y (0: chosen)
void exemplar_distances_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const int32_t *ids, int64_t E,
                               const int64_t *offsets, int64_t C, const double *Q, int64_t m, int metric, int splits,
                               double *dmin);
void soft_stats_init(hdb_ctx *ctx);  // stat soft_last_splits
// hdb_membership_vectors with every array on the device (prob, labels nullable); synchronises
void membership_vectors_device(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                               const int32_t *flat_label, int64_t K, int64_t C, const int32_t *anchor,
                               const double *level, const double *dmin, int64_t m, double *vectors, double *prob,
                               int32_t *labels);
// the same on host arrays, and the exemplar selection (host only): returns the exemplar count
int membership_vectors_host(const int32_t *parent, const double *birth, const double *death,
                            const int32_t *flat_label, int64_t K, int64_t C, const int32_t *anchor,
                            const double *level, const double *dmin, int64_t m, double *vectors, double *prob,
                            int32_t *labels);
int64_t exemplars_host(const int32_t *parent, const int32_t *flat_label, int64_t K, int64_t C,
                       const int32_t *point_cluster, const double *point_level, int64_t n, int32_t *ids,
                       int64_t *offsets);
// the ancestor, birth, eps_max and nearest-selected tables of the level cut and the out-of-sample
// labels (flat.hip sections 8 and 9) in the caller's scratch; returns the final nearest-selected buffer
constexpr int TREE_TABLES_BAD_PARENT = 1;
const int32_t *tree_tables_device(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                                  const int32_t *flat_label, int32_t K, int J, int32_t *anc, double *bt,
                                  unsigned long long *em, int32_t *near_a, int32_t *near_b, int *err);
// K2b's infinite-weight tail on host arrays (inf_edges.cpp): X, core in id order; (ea, eb)[m] the
// finite edges K2b found.  Writes the +inf edges that join their trees under (w, s, lo, hi) and
// returns their count; rows_left / first_left: rows outside the largest tree that only NaN
// pairs reach (0 / -1 when the tree spans).
int64_t inf_edges_host(const double *X, const double *core, int64_t n, int d, const int32_t *ea, const int32_t *eb,
                       int64_t m, int32_t *oa, int32_t *ob, double *ow, int64_t *rows_left, int32_t *first_left);

// K6 rank-order vertex labels: contracted labels reach nv + rank < 3m, stored as int32
inline bool flat_relabel_fits(int64_t m) { return m >= 0 && 3 * m < (int64_t)INT32_MAX; }
// K6: global hierarchy + flat labels over a merged MST (flat.hip); synchronises
void flat_labels_device(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                        int32_t mcs, int32_t *labels, int64_t *n_clusters);
// K6 + GLOSH outlier scores from the same hierarchy: scores (n, required), noise (n, eps per
// point) and labels nullable; synchronises
void flat_outlier_scores_device(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne,
                                int64_t n, int32_t mcs, double *scores, double *noise, int32_t *labels,
                                int64_t *n_clusters);

// outputs of hdb_flat_cluster_tree: cap entries per cluster array, n per point array, each
// nullable but n_tree (a host scalar); entry i describes tree label i + 1
struct ClusterTreeOut {
    int64_t cap;
    int64_t *n_tree;
    int32_t *parent;
    double *birth, *death, *stability;
    int32_t *size, *min_id, *flat_label;
    int32_t *point_cluster;
    double *point_level;
};
// K6 + the condensed cluster tree it builds, under canonical tree labels; synchronises
void flat_cluster_tree_device(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne,
                              int64_t n, int32_t mcs, const ClusterTreeOut &tree, int64_t *n_clusters);
// hierarchy rows (L x n) at arbitrary levels from a cluster tree, all arrays on the device; synchronises
void labels_at_levels_device(hdb_ctx *ctx, const int32_t *parent, const double *birth, int64_t K,
                             const int32_t *point_cluster, const double *point_level, int64_t n,
                             const double *levels, int32_t L, int32_t *labels_out);
// hdb_predict_labels: queries attached at (nearest, level) read their tree label, flat label and
// GLOSH score out of a cluster tree; every output nullable; all arrays on the device; synchronises
void predict_labels_device(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                           const int32_t *flat_label, int64_t K, const int32_t *point_cluster,
                           const double *point_level, int64_t n, const int32_t *nearest, const double *level,
                           int64_t m, int32_t *tree_label, int32_t *labels, double *scores);
// outputs of hdb_constrained_flat_labels: K entries per cluster array (entry i = tree label
// i + 1), n labels, each nullable; n_clusters is a host scalar
struct ConstrainedOut {
    int32_t *num_sat, *prop_sat;
    double *prop_stability;
    int32_t *flat_label;
    int32_t *labels;
    int64_t *n_clusters;
};
constexpr int64_t HDB_MAX_CONSTRAINTS = (int64_t(1) << 30) - 1;  // counts reach 2m and are Java ints
// constraint-aware flat extraction over a cluster tree, all arrays on the device (constraints.hip);
// synchronises
void constrained_flat_labels_device(hdb_ctx *ctx, const int32_t *parent, const double *stability,
                                    const int32_t *min_id, int64_t K, const int32_t *point_cluster, int64_t n,
                                    const int32_t *ca, const int32_t *cb, const int32_t *ctype, int64_t m,
                                    const ConstrainedOut &o);
// the same on host arrays (constraints.cpp)
int constrained_flat_labels_host(const int32_t *parent, const double *stability, const int32_t *min_id, int64_t K,
                                 const int32_t *point_cluster, int64_t n, const int32_t *ca, const int32_t *cb,
                                 const int32_t *ctype, int64_t m, const ConstrainedOut &o);
// K <= max(1, 2 floor(n / mcs) - 1): disjoint leaves of >= mcs points, every split >= 2 ways
inline int64_t cluster_tree_bound(int64_t n, int32_t mcs) {
    if (n <= 0) return 0;
    return std::max<int64_t>(1, 2 * (n / std::max<int32_t>(mcs, 1)) - 1);
}

// host logic (local_model.cpp)
int bubble_core_epilogue(const double *rep, const int32_t *nB, const double *eB, const double *nnB, int64_t b, int d,
                         int min_pts, int metric, const double *knn, const int32_t *log, double *core);
int flat_labels_host(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n, int32_t mcs,
                     int32_t *labels, int64_t *n_clusters);
int flat_outlier_scores_host(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                             int32_t mcs, double *scores, double *noise, int32_t *labels, int64_t *n_clusters);
int flat_cluster_tree_host(const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                           int32_t mcs, const ClusterTreeOut &tree, int32_t *labels, int64_t *n_clusters);
int labels_at_levels_host(const int32_t *parent, const double *birth, int64_t K, const int32_t *point_cluster,
                          const double *point_level, int64_t n, const double *levels, int32_t L,
                          int32_t *labels_out);
int predict_labels_host(const int32_t *parent, const double *birth, const double *death, const int32_t *flat_label,
                        int64_t K, const int32_t *point_cluster, const double *point_level, int64_t n,
                        const int32_t *nearest, const double *level, int64_t m, int32_t *tree_label, int32_t *labels,
                        double *scores);
int quicksort_edges(int32_t *va, int32_t *vb, double *w, int64_t ne);
// message of the last HDB_EREF_NEGATIVE_CLUSTER on this thread (cluster label, level, numPoints)
const char *local_model_error_detail();
// host phase times of local_model_host (us): quicksort, cluster tree, FOSC + noise
extern thread_local int64_t g_lm_us[6];  // + FOSC parts: selection walk, labelling, noise
int local_model_host(const double *rep, const double *eB, const double *nnB, const int32_t *nB, int64_t b, int d,
                     int32_t min_cl_size, int metric, int32_t *mva, int32_t *mvb, double *mw, int32_t *labels,
                     int32_t *ic_va, int32_t *ic_vb, double *ic_w, int64_t *n_ic);

}  // namespace hdb
