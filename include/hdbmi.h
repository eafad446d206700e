/*
 * hdbmi.h -- C-ABI of the MI355X-native MR-HDBSCAN* hot path.
 *
 * The reference (SZU-AdvTech-2022/232, Java 8 + Spark 2.x) keeps its driver and operator
 * surface; each entry point below is the body a JNI shim substitutes for the Java method
 * cited next to it (see INTEGRATION.md for the binding).  Plain C types only.
 *
 * Memory: every array argument may be HOST memory or DEVICE memory of the context's
 * device (detected per pointer).  Host inputs are staged to HBM on the context stream and
 * host outputs copied back before the call returns (PCIe-inclusive).  When every pointer
 * is device memory the call is stream-ordered on the context stream and returns without
 * synchronising (except where noted).  The caller allocates every output; the library
 * never retains a caller pointer after return.
 *
 * Errors: int status, 0 = OK, < 0 = error; hdb_last_error() returns a thread-local message.
 * The HDB_EREF_* codes reproduce the reference's own exceptions (a JNI shim maps them to
 * the corresponding Java RuntimeException).
 *
 * Threading: re-entrant; use one hdb_ctx per calling thread.
 */
#ifndef HDBMI_H
#define HDBMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDB_OK 0
#define HDB_EINVAL (-1)
#define HDB_EDEVICE (-2)
#define HDB_ENOMEM (-3)
#define HDB_EREF_NPE (-10)              /* java.lang.NullPointerException                    */
#define HDB_EREF_OOB (-11)              /* java.lang.ArrayIndexOutOfBoundsException          */
#define HDB_EREF_NEGATIVE_CLUSTER (-12) /* Clusters.java:45-46 "Cluster cannot have less than 0 points." */
#define HDB_EREF_DIVZERO (-13)          /* java.lang.ArithmeticException: / by zero          */
#define HDB_EREF_NUMBER_FORMAT (-14)    /* java.lang.NumberFormatException                   */
#define HDB_EUNSUPPORTED (-20)          /* a reference behaviour not emulated: a treeified
                                           java.util.HashMap bin (iteration order) or a loop the
                                           reference never leaves (NaN edge weight)            */

/* DistanceCalculator.getName() (distance/DistanceCalculator.java:20) */
#define HDB_METRIC_EUCLIDEAN 0 /* EuclideanDistance.java:28-36  */
#define HDB_METRIC_COSINE 1    /* CosineSimilarity.java:28-40   */
#define HDB_METRIC_PEARSON 2   /* PearsonCorrelation.java:28-51 */
#define HDB_METRIC_MANHATTAN 3 /* ManhattanDistance.java:28-36  */
#define HDB_METRIC_SUPREMUM 4  /* SupremumDistance.java:28-38   */

/* Core-distance semantics present in the reference */
#define HDB_CORE_INCL_SELF_CUMULATIVE 0 /* HDBSCANStar.java:71-106 (live; buffer never reset) */
#define HDB_CORE_INCL_SELF 1            /* CoreDistanceMapper.java:71-109                      */
#define HDB_CORE_EXCL_SELF 2            /* CreateLocalMST.java:138-185 (standard HDBSCAN*)     */

/* Bubble-statistics variants */
#define HDB_BUBBLE_COMBINESTEP 0 /* mappers/CombineStep.java:18-64 (live)            */
#define HDB_BUBBLE_CF 1          /* datastructure/ClusterFeatureDataBubbles.java:192-215 */
#define HDB_MAX_BUBBLE_SLICES 64 /* hdb_bubble_partials: slices per call                  */

typedef struct hdb_ctx hdb_ctx;

/* ------------------------------------------------------------------ context */
/* Environment read here: HDB_KERNEL_TIMING=1 (hdb_ctx_set_timing from birth) and
 * HDB_OPTS="name=value,name=value", every pair applied with hdb_ctx_set_option; a malformed pair
 * or one that call rejects fails the creation with its status (no context is returned). */
int hdb_ctx_create(int device, hdb_ctx **out);
void hdb_ctx_destroy(hdb_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL = the device's default
 * (null) stream.  A fresh context owns a private non-blocking stream until this is called. */
int hdb_ctx_set_stream(hdb_ctx *ctx, void *hip_stream);
/* Per-kernel HIP-event timing (off by default). */
int hdb_ctx_set_timing(hdb_ctx *ctx, int enable);
/* Synchronises, returns the summed device time (ms) and launch count of kernel `name`
 * since the last reset, then resets that accumulator when reset != 0. */
int hdb_ctx_kernel_time(hdb_ctx *ctx, const char *name, double *ms_total, int64_t *launches, int reset);
int hdb_ctx_synchronize(hdb_ctx *ctx);
/* Tuning/diagnostic switches (results are identical under every setting):
 *   "knn_fp32_screen" (default 1): K1 screens pairs in FP32 with a rigorous bound before the
 *                                  exact FP64 test;
 *   "knn_tree"        (default 1): euclidean k-NN lists of partitions with n >= "knn_tree_min_n"
 *                                  (default 8192) and d in {1,2,3,4,8,16} use K1t, the
 *                                  box-pruned traversal of the Morton/BVH index, instead of
 *                                  the all-pairs K1;
 *   "knn_mfma"        (default 1): euclidean lists with 16 < d <= 256 and n >= "knn_mfma_min_n"
 *                                  (default 2048) use K1m (bf16-split MFMA screen, FP64 re-check);
 *                                  "knn_mfma_single" (1: one screen pass + candidate log; 0: the
 *                                  two-pass kernel, which is also what a call falls back to when a
 *                                  query's candidate log overflows: stat "knn_mfma_log_overflow"),
 *                                  "knn_mfma_prune" (1: k-means order + FP64-ball superblock pruning);
 *   "nearest_grouped" (default 1): K3g (median-split sample groups, box pruning) for large
 *                                  euclidean nearest-sample scans;
 *   "prim_coop"       (default 1): single-launch cooperative Prim for 4096 < n <= 65536;
 *                                  "prim_coop_plain" (1: launched as a plain kernel first --
 *                                  cooperative launches serialise device-wide -- with a timed-out
 *                                  co-residency wait falling back to the cooperative launch;
 *                                  stat "prim_coop_plain_retries" counts those fallbacks),
 *                                  "prim_coop_plain_spin_log2" (default 20: polls per exchange
 *                                  before the plain attempt reports non-co-residency),
 *                                  "prim_coop_xcd" (default 1: the plain attempt's working
 *                                  workgroups, when the run-time XCC_ID check finds them on one
 *                                  XCD, exchange through that XCD's L2 -- placement changes only
 *                                  speed), "prim_coop_slots" (default 4: rows of d <= 16 in registers,
 *                                  tagged-granule exchange; 0: the counter-barrier kernel for every
 *                                  d, which 4 also falls back to; any other value is HDB_EINVAL);
 *   "bubble_knn_split"(default 1): bubble core distances scan their candidates in chunks and
 *                                  replay the sequential insertion log exactly;
 *   "boruvka_seed"    (default 1): a Boruvka round starts from the previous round's still
 *                                  valid per-point edges;
 *   "boruvka_knn_seed"(default 1): hdb_exact_mst keeps the k-NN lists for its Boruvka rounds:
 *                                  as seeds (lanes whose seed is provably exact skip the scan)
 *                                  and, in every round, as lower bounds (a lane whose list
 *                                  proves every outgoing edge heavier than its component's
 *                                  bound skips the scan); 0: no lists, neither;
 *                                  "leaf_seed_k" (list length, -1: by dimension),
 *                                  "leaf_list_rounds" (default 2: rounds whose list members are
 *                                  candidate edges; the lower bound runs in every round);
 *   "boruvka_wave_pts" (default 64; 16/32/64): points per scan wave; "boruvka_early_pts" /
 *                                  "boruvka_early_rounds": another size for the first rounds;
 *   "boruvka_adj_seed"(default 1): Morton-adjacent pairs across components bound every
 *                                  component before a Boruvka scan (valid edges only);
 *   "k1t_xcd_chunks" / "bor_xcd_chunks" (default 8): K1t and the Boruvka scan deal their
 *                                  Morton-ordered workgroups to the 8 XCDs as 8 interleaved chunks
 *                                  per XCD (L2 reuse of neighbour tiles; 0: dispatch order) --
 *                                  placement only, results unchanged;
 *   "trav_pop_test"   (default 0): bit 0 Boruvka, bit 1 K1t re-test a popped node;
 *   "ssort"           (default 1): the Morton order, the MST edge orders, K6's term order and
 *                                  hdb_sort_edges_desc use the sample sort (unique 128-bit keys:
 *                                  the same orders as the rocPRIM radix path, 0); "ssort_cap"
 *                                  (default 0 = 4096: keys per bucket sorted in LDS; larger
 *                                  buckets are merged in global memory);
 *   "flat_relabel"    (default 1): hdb_flat_labels renumbers vertex labels in rank order first
 *                                  (locality of the label records; the labels are unchanged);
 *   "flat_mid_log"    (default 12): hdb_flat_labels runs the divide-and-conquer depths below
 *                                  2^flat_mid_log ranks per workgroup (<= 10: all global);
 *                                  "flat_block_log" (default 10; 8..10: the 2^x-rank blocks the
 *                                  deepest depths run in LDS, 0: the sequential 256-rank kernel),
 *                                  "flat_root_variant" (0..5, default 3) / "flat_link_variant"
 *                                  (0..1, default 1): the kernels of the global depths (A/B);
 *                                  "flat_deep_depth" (default 64): global depths >= it use
 *                                  "flat_deep_root" / "flat_deep_link" instead; stats
 *                                  "flat_global_depths" / "flat_mid_depths" of the last call
 *                                  (of its contracted tree when "flat_contract" is 1: trees of
 *                                  2^18 edges or more, "flat_alpha_edges" edges of which branch);
 *   "prim_coop_bs"    (default 1024; 0, 128..1024): cooperative Prim workgroup size, 0 = the
 *                                  smallest that keeps the Prim within 32 workgroups; stats
 *                                  "prim_coop_last_bs" / "prim_coop_last_spread" of the last one;
 *   "count_evals"     (default 0): K1t/K2b count the pairs they evaluate (read "last_evals"). */
int hdb_ctx_set_option(hdb_ctx *ctx, const char *name, int64_t value);
/* Diagnostic counters: "last_evals" = pair evaluations of the last K1t call (count_evals on). */
int hdb_ctx_get_stat(hdb_ctx *ctx, const char *name, int64_t *value);
const char *hdb_last_error(void);
int hdb_version(void);

/* ------------------------------------------------------- distance (a1, a2) */
/* Pairwise distance of rows a[i] and b[i], i < n -- DistanceCalculator.computeDistance. */
int hdb_distance_rows(hdb_ctx *ctx, const double *a, const double *b, int64_t n, int32_t d, int32_t metric,
                      double *out);

/* ------------------------------------------------------ core distances (a3, a4)
 * Replaces HDBSCANStar.calculateCoreDistances(double[][] dataSet, int k, DistanceCalculator)
 * (HDBSCANStar.java:71) and its variants CreateLocalMST.java:138 / CoreDistanceMapper.java:71.
 * X: n x d row-major doubles.  core_out: n doubles. */
int hdb_core_distances(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t min_pts, int32_t metric,
                       int32_t semantics, double *core_out);

/* Per-row k smallest distances, ascending (Double.MAX_VALUE padded), optional neighbour
 * indices.  The value lists are the kernel output every core semantics derives from.
 * idx_out exists only for the euclidean metric with d in {1..6, 8, 16}: any other metric or
 * dimension with a non-null idx_out is HDB_EINVAL.
 *
 * Degenerate and non-finite input at d > 16 (hdb_core_distances and hdb_knn; every path gives the
 * reference's result, bit for bit: the strict '<' insertion into a Double.MAX_VALUE buffer,
 * HDBSCANStar.java:79-97, over distances summed in dimension order):
 *  - A pair whose distance is NaN (a NaN coordinate; inf - inf in one coordinate) or not below
 *    Double.MAX_VALUE (an infinite coordinate, a squared distance that overflows) never enters
 *    a list.  A row all of whose pairs are such keeps Double.MAX_VALUE in every entry, and so
 *    does every entry past the number of candidates when fewer than k rows qualify (n - 1 < k
 *    with excl_self, n < k without): the reference's padding, also as a core distance.
 *  - With a NaN or infinite coordinate anywhere in X, or column sums that overflow, the matrix-
 *    core path (euclidean, 16 < d <= 256, n >= "knn_mfma_min_n") declines before it runs a
 *    kernel and the FP64 scan answers, as it does for d > 256 and for "knn_mfma" = 0.
 *  - Squared distances that underflow are the reference's: +0.0 or the subnormal the sequential
 *    sum rounds to, ties included.  Finite input whose column sums are finite stays on the
 *    matrix-core path at any magnitude: its power-of-two scale is clamped where the ideal one
 *    would leave the double range (max |x - mean| below 2^-456), the square of the scale is
 *    never formed (it would round to 0 from max |x - mean| >= 2^537 on, where rows closer than
 *    2^512 still have finite distances; csrc/knn_mfma.hip "Range"), and input it cannot
 *    separate (identical rows, rows far below the largest) is re-computed pair by pair in
 *    FP64. */
int hdb_knn(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t k, int32_t metric, int32_t excl_self,
            double *dist_out /* n*k */, int32_t *idx_out /* n*k, nullable */);

/* ----------------------------------------------------------------- MST (a5, a6)
 * Replaces HDBSCANStar.constructMST(double[][] dataSet, double[] coreDistances, boolean
 * selfEdges, DistanceCalculator, int[] indices, int totalLength) (HDBSCANStar.java:124-125).
 * Exact reference Prim: start vertex n-1, strict '<' update, '<=' select, Double.MAX_VALUE
 * init.  Edge i < n-1 = (va=parent of i, vb=ids[i], w); then n self edges if self_edges.
 * ids nullable (identity). */
int hdb_prim_mst(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core, const int32_t *ids,
                 int32_t metric, int32_t self_edges, int32_t *va, int32_t *vb, double *w);

/* The same Prim for P independent partitions stored back to back: partition p = rows
 * offsets[p] .. offsets[p+1]-1 of X/core/ids.  Edges of partition p start at
 * edge_offsets[p] = sum_{q<p} (n_q - 1 + (self_edges ? n_q : 0)). */
int hdb_prim_mst_batched(hdb_ctx *ctx, const double *X, const int64_t *offsets, int32_t P, int32_t d,
                         const double *core, const int32_t *ids, int32_t metric, int32_t self_edges, int32_t *va,
                         int32_t *vb, double *w);

/* FirstStep.call leaf branch (mappers/FirstStep.java:104-120) for P partitions at once:
 * live cumulative core distances (HDBSCANStar.java:71-106) + Prim with self edges, vertex
 * ids = global point ids.  core_out nullable. */
int hdb_leaf_msts(hdb_ctx *ctx, const double *X, const int64_t *offsets, int32_t P, int32_t d, const int32_t *ids,
                  int32_t min_pts, int32_t metric, double *core_out, int32_t *va, int32_t *vb, double *w);

/* Exact minimum spanning tree of the mutual-reachability graph for large n (Boruvka), for
 * every HDB_METRIC_* and every d >= 1 that hdb_core_distances accepts; n < 2^31 (int32 ids).
 * Any MST: the sorted weight sequence equals the reference Prim's exactly; the
 * topology can differ only among equal-weight edges (ties broken by (w, min id, max id)).
 * Outputs n-1 edges (va < vb, by the library's order), then n self edges if self_edges.
 *
 * Exactly: the unique MST under the strict total edge order (w, s, min id, max id).
 *   w  the reference's weight (HDBSCANStar.java:162-168): the pair's distance, replaced by
 *      core_p, then by core_q, on a strict '>' only.
 *   s  the tie key below w.  Euclidean: the squared distance summed in dimension order (w
 *      starts from sqrt(s)).  Every other metric: the pair's distance itself, in the
 *      reference's operation order (no contraction).
 * Two paths, one contract.  Euclidean with d in {1,2,3,4,8,16} runs K2b (Morton/BVH index).
 * Everything else runs K2g, a tiled all-pairs FP64 scan (kernel timers "boruvka_gen_scan" and
 * "boruvka_gen_total", stats "boruvka_gen_rounds" = rounds of the last call and
 * "boruvka_gen_qt" / "_ct" / "_dc" = its query tile, candidate tile and dimension chunk).
 * For a Euclidean input both keys are the same, so the two paths agree edge for edge.
 * Weights and tie keys can be negative on K2g: cosine and Pearson distances are 1 - x with x
 * rounded, and x can exceed 1 by a few ulps (rows that are positive multiples of one another).
 * Every non-NaN double is ordered numerically; a tree edge may then weigh less than zero and
 * comes back as computed, and the edge list ascends numerically.  (The hierarchy calls'
 * contracts on weights are unchanged.)
 * Non-finite and signed-zero input (the same for hdb_exact_mst):
 *  - A pair whose mutual-reachability distance is NaN (a NaN coordinate; inf - inf in one
 *    coordinate) is not an edge.
 *  - A row with an infinite coordinate, a squared distance that overflows or an infinite core
 *    gives edges of weight +inf.  They are edges like any other and fall under the same tie
 *    rule: among +inf weights the smaller s wins, then the smaller ids.  (K2b's device rounds
 *    find the finite edges; the +inf edges that join what is left are chosen on the host, stat
 *    "boruvka_inf_edges".  K2g keeps "no edge yet" apart from the weight and finds +inf edges
 *    on the device like any other; it does not count them in that stat.)
 *  - Input whose non-NaN pairs do not connect all rows (e.g. any row with a NaN coordinate) is
 *    HDB_EINVAL with a message that names "non-finite input", the number of unreachable rows
 *    and the first of them.  No output is defined then; the context stays usable.
 *  - A NaN core never raises a weight (the reference's '>' comparisons), and neither does a
 *    -0.0 core: weights compare as numbers, so -0.0 acts as +0.0.  A tree edge's weight is
 *    never -0.0 (it starts from a distance that is not -0.0 -- sqrt(s) >= +0.0, a sum of
 *    absolute values, 1 - x -- and only a strictly larger core replaces it);
 *    a self edge's weight is the core as passed, so a -0.0 core comes back as -0.0 there. */
int hdb_mst_boruvka(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core, int32_t metric,
                    int32_t self_edges, int32_t *va, int32_t *vb, double *w);

/* FirstStep's leaf branch for one large partition in one call (FirstStep.java:104-108:
 * HDBSCANStar.calculateCoreDistances then constructMST): core distances (semantics as
 * hdb_core_distances, bit-identical) and the exact mutual-reachability MST of
 * hdb_mst_boruvka (same weights and edge order), for every metric and d it accepts.  K2b's
 * shapes share one spatial index and the k-NN lists seed every Boruvka round; every other
 * shape is hdb_core_distances (so Euclidean 16 < d <= 256 with n >= 2048 takes its MFMA path)
 * followed by K2g.  core_out nullable.  Local vertex ids 0..n-1.
 * NaN pairs, +inf weights and rows that no non-NaN pair reaches (HDB_EINVAL, "non-finite
 * input") are handled exactly as documented at hdb_mst_boruvka; core_out is then undefined. */
#define HDB_EDGES_SELF 1   /* append the n self edges (HDBSCANStar.java:196-203)                  */
#define HDB_EDGES_MERGED 2 /* return the edges in the reducers' merge order instead: exactly what
                              hdb_sort_edges_desc returns for the plain list (UnionFindReducer.java:
                              19-69 + SortMST.java:9-17, stable descending), without the re-sort */
int hdb_exact_mst(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t min_pts, int32_t metric,
                  int32_t semantics, int32_t self_edges /* HDB_EDGES_* flags; 0/1 as before */, double *core_out,
                  int32_t *va, int32_t *vb, double *w);

/* ---------------------------------------------------------- nearest sample (a8, a9)
 * FirstStep.call non-leaf branch (FirstStep.java:74-85): the FIRST minimum over the sample
 * list (strict '<').  With x_key/s_key non-NULL only samples of the point's key are scanned
 * (D3; ClusterFeaturesByNodesMapper.java:53-61).  nearest_out = list position (0 if no
 * candidate, as the Java init), dist_out nullable (Double.MAX_VALUE if none).
 *
 * Degenerate and non-finite input (every path gives the reference's result, bit for bit):
 *  - A (point, sample) pair whose distance is NaN (a NaN coordinate, inf - inf, a cosine or Pearson
 *    of rows whose norm or variance is 0, underflows or overflows) or is not below Double.MAX_VALUE
 *    (an infinite coordinate, a squared distance that overflows) is no candidate: the reference's
 *    'distance < minDistance' from Double.MAX_VALUE never holds for it.
 *  - A point without any candidate -- a NaN row, every sample out of range, a key without samples
 *    -- gets list position 0 and Double.MAX_VALUE.  Position 0 is also a legitimate winner: only
 *    dist_out tells the two apart.
 *  - Distances compare as sqrt values; among equal sqrt values (also from different squares, and
 *    when every squared distance underflows to 0) the smaller list position wins.
 *  - The grouped scan (K3g; option nearest_grouped) runs for Euclidean distance, d in {2, 3, 4, 8,
 *    16}, n >= 8192 points and m >= 1024 samples, and only when every sample coordinate is finite.
 *    Any NaN or infinite SAMPLE, like any other shape, metric or nearest_grouped = 0, takes the
 *    plain scan.  Non-finite POINTS go through either path. */
int hdb_nearest_sample(hdb_ctx *ctx, const double *X, int64_t n, const double *S, int64_t m, int32_t d,
                       int32_t metric, const int32_t *x_key, const int32_t *s_key, int32_t *nearest_out,
                       double *dist_out);

/* --------------------------------------------------------- out-of-sample prediction: the attach scan
 * Attaches m query rows Q (m x d) to a fitted set: X (n x d) training rows and core (n), their
 * core distances as passed -- whatever semantics the fit used.  Everything is exact, in the
 * reference's operation order (no contraction); all five metrics, every d >= 1.
 *   dist(i, j)  DistanceCalculator.computeDistance(Q[i], X[j]), the query row first: the bits of
 *               hdb_distance_rows.
 *   core_q[i]   (m, nullable) entry K - 1 of the ascending list of the K = min_pts - 1 smallest
 *               dist(i, j) over all n training rows, filled by the reference's strict '<' insertion
 *               into a Double.MAX_VALUE buffer (HDBSCANStar.java:79-97): a NaN distance, or one not
 *               below Double.MAX_VALUE, never enters, and fewer than K candidates leave
 *               Double.MAX_VALUE -- the core distance HDB_CORE_EXCL_SELF gives the query as the last
 *               row of [X; Q[i]].  min_pts == 1: 0.  min_pts outside 1..32: HDB_EINVAL, as
 *               hdb_core_distances.
 *   w(i, j)     dist(i, j), replaced by core_q[i], then by core[j], on a strict '>' only
 *               (HDBSCANStar.java:162-168): a NaN core never raises a weight, a -0.0 core acts as
 *               +0.0.  A pair whose w is NaN is no candidate; +inf is a candidate like any other.
 *   nearest[i]  (m) the j that minimises the strict total order (w, s, j), s as in hdb_mst_boruvka:
 *               Euclidean: the squared distance summed in dimension order; every other metric: the
 *               distance itself.  Negative cosine and Pearson values are ordered numerically.
 *   level[i]    (m) that w.
 * A query without a candidate (a NaN query row, only NaN weights, n == 0): nearest = -1, level =
 * Double.MAX_VALUE.  m == 0: HDB_OK.  n >= 2^31: HDB_EINVAL.  Pointer rules as hdb_knn: host or
 * device per pointer, stream-ordered when all pointers are device memory.
 * Two passes of one tiled all-pairs FP64 scan (kernel timers "attach_knn": the lists, "attach_min":
 * the arg-min), the training rows split over workgroup columns whose partial lists and partial
 * (w, s, j) minima a second kernel merges; the column count changes no bit of the output.
 * hdb_attach_points_splits is the same call with that count as an argument: attach_splits = 0
 * chooses it from m and n (what hdb_attach_points does), 1..65535 forces it (columns past the last
 * tile are empty), anything else is HDB_EINVAL; stat "attach_last_splits" = the count of the last
 * call.  The count is an argument of the call, not a context option: nothing is left set. */
int hdb_attach_points(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core, const double *Q,
                      int64_t m, int32_t min_pts, int32_t metric, double *core_q, int32_t *nearest, double *level);
int hdb_attach_points_splits(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core,
                             const double *Q, int64_t m, int32_t min_pts, int32_t metric, int32_t attach_splits,
                             double *core_q, int32_t *nearest, double *level);

/* --------------------------------------------------------- validity of a labelling: the DBCV index
 * Density-Based Clustering Validation (Moulavi, Jaskowiak, Campello, Zimek, Sander, SDM 2014) of a
 * labelling of X, for all five metrics and every d >= 1.  The reference has no such routine: the
 * contract is this library's own, one fixed operation order, bit-exact against a plain restatement
 * (tests/validity_reference.py).
 * Input: X (n x d), labels (n; 0 is noise, 1..K are clusters), K >= 0, metric.  A label outside
 * 0..K is HDB_EINVAL and the message names the first offending row.  Rows labelled 0 are never read
 * as coordinates (a NaN there is accepted).  A non-finite coordinate in a labelled row is HDB_EINVAL
 * with "non-finite input" and the first such row.  The context stays usable after either.
 *   dist(i, j)   DistanceCalculator.computeDistance(X[i], X[j]), i < j: the bits of
 *                hdb_distance_rows.  No contraction.
 *   members      of cluster c: its rows in ascending id; n_c their count.
 *   1. all-points core distance of a member x of c: over the other members y of c with
 *      dist(x, y) > 0 (self -- also skipped by index --, duplicates, slightly negative cosine and
 *      Pearson values and NaN contribute nothing), t = 1.0 / dist and p = t^d by right-to-left binary
 *      exponentiation (r = 1; b = t; e = d; while e: if e & 1: r = r * b; e >>= 1; if e: b = b * b).
 *      Summation shape: the members are cut into blocks of HDB_VALIDITY_SUM_BLOCK consecutive
 *      members by position in the member order; a block's partial starts at 0.0 and adds its
 *      contributing p in member order; the total starts at 0.0 and adds the block partials in block
 *      order.  apts_core[x] = total == 0 ? 0.0 : pow(total / (double)(n_c - 1), -1.0 / d), the host
 *      libm's pow, applied on the host to the n totals for device and host pointers alike (the call
 *      synchronises).  n_c == 1 and noise rows: 0.0.  An overflow of p or of the total to +inf gives
 *      the core 0.0, as computed: at large d (or tiny distances) the index inherits DBCV's known
 *      range problem.
 *   2. MST of c: the tree hdb_mst_boruvka returns for the members' rows, in member order, with these
 *      cores -- the unique MST under the strict order (w, s, lo, hi).  A status it returns
 *      propagates, with the cluster label added to the message (cosine with an all-zero member row:
 *      only NaN pairs reach it, "non-finite input").
 *   3. deg = the degree in that tree; internal members have deg >= 2, internal edges are the tree
 *      edges with both ends internal.  If c has no internal edge (n_c <= 3, stars), every member is
 *      internal and every tree edge is internal.  sparseness[c] = the largest internal edge weight;
 *      0.0 for n_c <= 1.
 *   4. for internal x in c and internal y in c' != c: w(x, y) = dist, replaced by apts_core[x], then
 *      by apts_core[y], on a strict '>' only; a pair whose w is NaN is no candidate.  separation[c] =
 *      the minimum of w over all such pairs, nearest_cluster[c] = the smallest label c' that attains
 *      it; with no such pair (c empty, no other non-empty cluster): +inf and 0.
 *   5. validity[c] = (separation - sparseness) / max(separation, sparseness); 0.0 when that max is
 *      0, when c is empty, or when separation is +inf.
 *   6. index = the sum, in ascending label order from 0.0, of ((double)n_c / (double)n) *
 *      validity[c]; n includes noise; computed on the host.  n == 0 or K == 0: HDB_OK, index 0.0.
 * Outputs: index (a host double, required); each of the others may be NULL on its own: validity,
 * sparseness, separation (K doubles each), nearest_cluster, size (K int32 each; entry c - 1 is
 * label c), apts_core (n doubles), internal (n int32: 0 or 1, 0 for noise).  Pointer rules as
 * hdb_knn: host or device per pointer; ctx is required.  n >= 2^31: HDB_EINVAL.
 * Two tiled all-pairs FP64 scans in the style of the attach scan (kernel timers "validity_core",
 * "validity_sep"); clusters of up to small_max members get their trees from one launch of a dense
 * Prim, one workgroup per cluster ("validity_mst_small"), larger ones go one by one through
 * hdb_mst_boruvka's device path under its own timers.
 * hdb_validity_index_splits is the same call with the candidate-column count of both scans as an
 * argument: splits = 0 chooses it, 1..65535 forces it, anything else is HDB_EINVAL; it changes no
 * bit of any output.  In the core scan the columns fall on sum-block boundaries and every block's
 * partial is stored (sum over c of n_c * ceil(n_c / HDB_VALIDITY_SUM_BLOCK) doubles); a chosen
 * count drops to 1 when that store would exceed 2^22 doubles, a forced one is honoured.  Stats
 * "validity_last_splits" (the separation scan) and "validity_last_core_splits" of the last call.
 * hdb_validity_index_route adds small_max (0..2048; 0 sends every cluster through the Boruvka
 * path), HDB_VALIDITY_SMALL_MAX in the other two; it changes no bit either.  Both are arguments of
 * the call, not context options: nothing is left set. */
#define HDB_VALIDITY_SUM_BLOCK 512
#define HDB_VALIDITY_SMALL_MAX 1024
int hdb_validity_index(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *labels, int32_t K,
                       int32_t metric, double *index, double *validity, double *sparseness, double *separation,
                       int32_t *nearest_cluster, int32_t *size, double *apts_core, int32_t *internal);
int hdb_validity_index_splits(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *labels, int32_t K,
                              int32_t metric, int32_t splits, double *index, double *validity, double *sparseness,
                              double *separation, int32_t *nearest_cluster, int32_t *size, double *apts_core,
                              int32_t *internal);
int hdb_validity_index_route(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *labels, int32_t K,
                             int32_t metric, int32_t splits, int32_t small_max, double *index, double *validity,
                             double *sparseness, double *separation, int32_t *nearest_cluster, int32_t *size,
                             double *apts_core, int32_t *internal);

/* --------------------------------------------------------- bubble statistics (a11, a12)
 * Bulk CombineStep (CombineStep.java:18-64) over a partition: member order = ascending
 * point index (D5).  Outputs per bubble: ls, ss, rep (nb*d), info (nb*3: extent, nnDist, n).
 * Empty bubbles: all zero.  A one-member bubble: rep = the row, extent = nnDist = 0.
 *
 * Degenerate and non-finite input (the same for hdb_bubble_partials + hdb_bubble_combine; both
 * fold kernels, option bubble_fold_dim, give the same bits):
 *  - ls and ss are the sequential sums in member order; ss may overflow to +inf, ls may become
 *    NaN (+inf and -inf members) and both carry a member's NaN.  rep = ls / n as it comes out.
 *  - HDB_BUBBLE_COMBINESTEP: a dimension adds sqrt(v / (n (n - 1))) to the extent only when
 *    v = 2 n SS - 2 LS^2 satisfies v >= 0 (CombineStep.java:46-56).  A negative v (rounding noise of
 *    members that agree to a few ulps) and a NaN v (inf - inf after an overflow, a non-finite
 *    member) add nothing, so the extent is never NaN; it is 0 when no dimension qualifies and
 *    +inf when a v is +inf.  v is computed without contraction: a fused multiply-add changes its
 *    sign on such members.
 *  - HDB_BUBBLE_CF sums v / (n (n - 1)) over the dimensions without the test and takes one sqrt
 *    (ClusterFeatureDataBubbles.java:192-215): a negative or NaN sum gives a NaN extent and nnDist.
 *    n (n - 1) is a Java int and wraps: exact up to n = 46,341, negative from 46,342 on (NaN
 *    extent), 0 at n = 65,536 (division by zero: NaN or inf), as the reference computes it. */
int hdb_bubble_stats(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *bubble_of, int64_t nb,
                     int32_t variant, double *ls, double *ss, double *rep, double *info);

/* CombineStep as Spark runs it: reduceByKey(new CombineStep()) (Main.java:236-237) folds each
 * partition map-side, then merges the partials (CombineStep.java:18-40 on two partials).  With
 * the partitions fixed (D11) the statistics shard: a rank folds the rows of its slices
 * (cuts[0..S]: S + 1 non-decreasing row offsets, cuts[0] = 0, cuts[S] = n; S <= 64) into
 * per-(slice, bubble) partials -- part_ls / part_ss: S x nb x d, part_n: S x nb member counts --
 * and hdb_bubble_combine merges the gathered partials of all slices in slice order (empty
 * partials skipped) and computes rep / extent / nnDist from the merged (LS, SS, n) with
 * CombineStep.java:42-64's formulas.  One slice is hdb_bubble_stats(HDB_BUBBLE_COMBINESTEP)
 * bit for bit.  Degenerate and non-finite members: as documented at hdb_bubble_stats (the sign test
 * on v runs once, on the merged sums; an empty slice between two others changes nothing). */
int hdb_bubble_partials(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *bubble_of, int64_t nb,
                        const int64_t *cuts, int32_t S, double *part_ls, double *part_ss, double *part_n);
int hdb_bubble_combine(hdb_ctx *ctx, const double *part_ls, const double *part_ss, const double *part_n, int32_t S,
                       int64_t nb, int32_t d, double *ls, double *ss, double *rep, double *info);

/* ------------------------------------------------------------- bubble model (a13-a15)
 * HdbscanDataBubbles.calculateCoreDistancesBubbles(double[][] repB, int[] nB, double[] eB,
 * double[] nnDistB, int k, DistanceCalculator) (HdbscanDataBubbles.java:75-76).
 *
 * Degenerate statistics: the k-NN buffer starts at Double.MAX_VALUE and a neighbour enters on a
 * strict '<', so a bubble pair whose transformed distance is NaN (a NaN rep, a NaN nnDist) or is
 * not below Double.MAX_VALUE (an infinite rep or extent) is no candidate, and a bubble with fewer
 * than minPts - 1 candidates keeps Double.MAX_VALUE entries that the core formula then reads.
 * Extent 0 and nnDist 0 (one-member bubbles, identical members) are ordinary values: equal
 * distances keep the first neighbour in index order.  The chunked scan (option bubble_knn_split)
 * and the plain scan give the same bits. */
int hdb_bubble_core_distances(hdb_ctx *ctx, const double *rep, const int32_t *nB, const double *eB,
                              const double *nnB, int64_t b, int32_t d, int32_t min_pts, int32_t metric,
                              double *core_out);

/* HdbscanDataBubbles.constructMSTBubbles(...) (HdbscanDataBubbles.java:165-167).
 * Degenerate statistics: the reference's Prim, edge for edge in its order.  A candidate weight
 * that is NaN or not below Double.MAX_VALUE never relaxes a vertex; a vertex that no comparison
 * relaxed is attached with weight Double.MAX_VALUE, in the reference's order, by every kernel
 * here (block, cooperative register, cooperative counter-barrier). */
int hdb_bubble_prim_mst(hdb_ctx *ctx, const double *rep, const double *eB, const double *nnB,
                        const int32_t *id_bubbles, const double *core, int64_t b, int32_t d, int32_t metric,
                        int32_t self_edges, int32_t *va, int32_t *vb, double *w);

/* LocalModelReduceByKey.call body (LocalModelReduceByKey.java:88-104) with D4 vertex ids
 * 0..b-1: bubble cores, bubble Prim, UndirectedGraph.quicksortByEdgeWeight, cluster tree,
 * FOSC + noise reassignment, inter-cluster edges.  info = b*3 (extent, nnDist, n).
 * Outputs: labels[b]; mst_* (2b-1, quicksorted ascending, nullable); ic_* (capacity 2b-1),
 * *n_ic = number of inter-cluster edges.  rep and info may be host or device memory; the
 * outputs (labels, mst_*, ic_*, n_ic) are host memory only: HDB_EINVAL for a device pointer. */
int hdb_local_model(hdb_ctx *ctx, const double *rep, const double *info, int64_t b, int32_t d, int32_t min_pts,
                    int32_t min_cl_size, int32_t metric, int32_t *labels, int32_t *mst_va, int32_t *mst_vb,
                    double *mst_w, int32_t *ic_va, int32_t *ic_vb, double *ic_w, int64_t *n_ic);

/* hdb_local_model from precomputed bubble core distances (host or device, b values: hdb_bubble_core_distances
 * of the same rep / nB = (int) info[:, 2] / eB = info[:, 0] / nnB = info[:, 1], min_pts, metric) --
 * the same outputs; lets a caller compute every model's cores of a level before any model's Prim
 * (round 6: a Prim holds its CUs for its whole run and slows concurrent work). */
int hdb_local_model_cores(hdb_ctx *ctx, const double *rep, const double *info, int64_t b, int32_t d, int32_t min_pts,
                          int32_t min_cl_size, int32_t metric, const double *core, int32_t *labels, int32_t *mst_va,
                          int32_t *mst_vb, double *mst_w, int32_t *ic_va, int32_t *ic_vb, double *ic_w,
                          int64_t *n_ic);

/* UndirectedGraph.quicksortByEdgeWeight (UndirectedGraph.java:93-124), in place, host. */
int hdb_quicksort_edges(int32_t *va, int32_t *vb, double *w, int64_t ne);

/* ------------------------------------------------------------------- merge (a20)
 * UnionFindReducer.call + SortMST (UnionFindReducer.java:19-69, SortMST.java:9-17): stable
 * sort by DESCENDING weight of the concatenated local edge lists, in place (device radix
 * sort).  The cross-GPU all-gather feeding it runs over RCCL in the host layer. */
int hdb_sort_edges_desc(hdb_ctx *ctx, int32_t *va, int32_t *vb, double *w, int64_t ne);

/* The same result when the concatenation is made of runs that are each already sorted
 * descending (as hdb_sort_edges_desc returns them): runs r = [run_off[r], run_off[r+1]) of
 * (va, vb, w), nruns of them; output (oa, ob, ow) = the stable descending sort of their
 * concatenation -- equal weights keep run order, then their order inside the run.  The
 * stable sort of a rank-major concatenation of raw lists equals this merge of the ranks'
 * individually sorted lists, so a reducer merges instead of re-sorting (pairwise merge-path
 * tiles, O(E log nruns)).  Outputs must not alias inputs.  HDB_EINVAL on a NaN weight or a
 * run that is not descending.  run_off (nruns + 1 values) may be host or device memory like
 * the other arrays.  Synchronises. */
int hdb_merge_sorted_runs(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, const int64_t *run_off,
                          int32_t nruns, int32_t *oa, int32_t *ob, double *ow);

/* ---------------------------------------------- cross-GPU merge over RCCL (§8(b), §8(e))
 * One communicator per rank (one process per GPU).  The caller moves the unique id from the
 * rank that made it to the others (Spark broadcast, torch.distributed, MPI ...). */
typedef struct hdb_comm hdb_comm;
/* Writes an RCCL unique id (128 bytes) into id_out; returns its size or an error. */
int hdb_comm_unique_id(void *id_out, int32_t cap);
/* Collective over the nranks ranks; the context fixes the device and stream. */
int hdb_comm_init(hdb_ctx *ctx, int32_t nranks, int32_t rank, const void *id, hdb_comm **out);
void hdb_comm_destroy(hdb_comm *comm);
/* Frees a buffer the library allocated (hdb_merge_edges outputs). */
int hdb_free(void *p);
/* Copies bytes between any two host/device buffers on the context stream; synchronises. */
int hdb_copy(hdb_ctx *ctx, void *dst, const void *src, int64_t bytes);
/* Main.java:302-347 + UnionFindReducer.call + SortMST (UnionFindReducer.java:19-69,
 * SortMST.java:9-17): every rank passes its local edge list; all ranks receive the merged
 * list of all E edges (device memory allocated by the library, freed with hdb_free), stably
 * sorted by DESCENDING weight.  seq (nullable; on every rank that has local edges or on
 * none -- a rank with e_local == 0 is consistent with either): the canonical
 * position of each local edge in the global concatenation (a permutation of [0, E) over all
 * ranks) -- the sort then sees that concatenation, independent of which rank computed which
 * partition; NULL = rank-major concatenation.  Collective; synchronises. */
int hdb_merge_edges(hdb_comm *comm, const int32_t *va, const int32_t *vb, const double *w, const int64_t *seq,
                    int64_t e_local, int32_t **va_all, int32_t **vb_all, double **w_all, int64_t *e_all);

/* CreateLocalMST's record fields (partition/mappers/CreateLocalMST.java:242,266,276-285):
 * for a partition's edge list with global vertex ids (e.g. hdb_prim_mst / hdb_leaf_msts /
 * hdb_exact_mst output), fake1[e] / fake2[e] = the local index of va[e] / vb[e] in the
 * partition's `indices` (ids, n; NULL = identity), node_out[e] = node (nullable).  On
 * hdb_prim_mst's output this is exactly nearestneighborsID / otherVertexIndicesID, so
 * hdb_format_mst_records reproduces the reference's local-MST text.  w (nullable) = the
 * edge weights of hdb_prim_mst's layout (n - 1 tree edges first): a tree edge whose weight is
 * still Double.MAX_VALUE was never relaxed (every MRD NaN or >= MAX_VALUE), and the
 * reference keeps its Java default nearestneighborsID = 0 (CreateLocalMST.java:203,242) --
 * fake1 = 0 there, whatever va holds.  Errors: HDB_EINVAL on duplicate ids or an edge vertex
 * outside the partition.  Synchronises. */
int hdb_local_mst_ids(hdb_ctx *ctx, const int32_t *ids, int64_t n, const int32_t *va, const int32_t *vb,
                      const double *w, int64_t ne, int32_t node, int32_t *fake1, int32_t *fake2, int32_t *node_out);

/* ------------------------------------------------ global flat labels (§8(f) #1)
 * The step the reference never completes (Main.java:351-408): HDBSCAN* hierarchy over the
 * merged MST and its flat FOSC / excess-of-mass partition -- HDBSCANStar.java:208-625
 * (computeHierarchyAndClusterTree, propagateTree, findProminentClusters; commented out in the
 * reference) without constraints, canonical tie rules (DESIGN.md "flat labels").
 * va/vb/w: the merged edge list (self edges ignored; the rest must form a spanning tree of
 * the n points).  labels: n ints, 1..K by ascending smallest member id, 0 = noise.
 * min_cl_size >= 2.  ctx may be NULL when every pointer is host memory (pure host algorithm). */
int hdb_flat_labels(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                    int32_t min_cl_size, int32_t *labels, int64_t *n_clusters);

/* GLOSH outlier scores over the same hierarchy (HDBSCANStar.propagateTree :505-540,
 * calculateOutlierScores :653-686, Cluster.propagate :99-105), optionally with the flat labels
 * of hdb_flat_labels from the one hierarchy the call builds.  Inputs, tie rules, pointer rules
 * (device, host or mixed; ctx may be NULL when every pointer is host memory) and status codes
 * are exactly those of hdb_flat_labels.
 *   eps(x) (noise_level, pointNoiseLevels): the weight of the tie group whose removal leaves x
 *     in a component of fewer than min_cl_size points; with n < min_cl_size every point leaves at
 *     the heaviest edge's weight.  last(x) (pointLastClusters): the cluster x leaves from.
 *   eps_max(C) (propagatedLowestChildDeathLevel): the lowest level at which C or any of its
 *     descendant clusters loses its last points.  For the ROOT cluster only the descendants
 *     count, and a root that never splits into two valid children keeps Java's initial
 *     Double.MAX_VALUE: the points that leave such a root score 1 - DBL_MAX / eps(x), a huge
 *     negative number or -inf, as the reference's arithmetic gives.
 *   scores[x] = eps(x) == 0 ? 0.0 : 1.0 - eps_max(last(x)) / eps(x): one IEEE double division
 *     and one subtraction, bit-identical on host and device.
 * scores: n doubles, required.  noise_level (n doubles), labels (n ints, as hdb_flat_labels)
 * and n_clusters may be NULL.  n == 0 is HDB_OK; n == 1 gives score 0 and noise level 0.
 * Non-finite weights are out of scope.  Ranking and the output file are host formatting
 * (ascending (score, core distance, id); "score,id" lines). */
int hdb_flat_outlier_scores(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne,
                            int64_t n, int32_t min_cl_size, double *scores, double *noise_level, int32_t *labels,
                            int64_t *n_clusters);

/* The condensed cluster tree of the same hierarchy (HDBSCANStar.computeHierarchyAndClusterTree
 * :208-474): what hdb_flat_labels builds and discards.  Inputs, tie rules, pointer rules (device,
 * host or mixed; ctx may be NULL when every pointer is host memory) and status codes are exactly
 * those of hdb_flat_labels; non-finite weights are out of scope, as for the scores.
 *   K >= 1 clusters (0 only for n == 0) with 1-based TREE LABELS; 0 = noise / no parent.  Label 1
 *   is the root (all points); labels 2..K order the other clusters by (birth level descending,
 *   smallest member id ascending), so a parent's label is below its children's.  Entry i of a
 *   per-cluster array describes tree label i + 1:
 *     parent      tree label of the parent, 0 for the root
 *     birth       the level at which the cluster appears (its parent's split); NaN for the root
 *     death       the level at which its last points leave: its children's birth level when it
 *                 splits, else the level of the last node on its chain
 *     stability   the value FOSC compares: sum over its levels, descending, of
 *                 count * (1/eps - 1/birth); NaN for the root (n >= 2), 0 for n == 1
 *     size        points at birth;  min_id  smallest member id at birth
 *     flat_label  1..n_clusters (the numbering of hdb_flat_labels) when FOSC selected the
 *                 cluster, else 0 -- also 0 for a cluster below a selected one, and for the root
 *   per point x:
 *     point_cluster  tree label of last(x), the cluster x leaves as noise from
 *     point_level    eps(x), bit-identical to hdb_flat_outlier_scores' noise_level; 0 for n == 1
 *   The flat label of x is flat_label of the nearest selected cluster on the path from last(x)
 *   to the root; the GLOSH eps_max is the subtree minimum of death.
 * cap: entries available in each per-cluster array; hdb_cluster_tree_bound gives a value that
 * always suffices.  *n_tree (required, host) receives K.  cap < K: HDB_EINVAL, *n_tree is still
 * set to K, the message names both numbers and no array has been written.  Every per-cluster and
 * per-point output, and n_clusters (host), may be NULL on its own.  n == 1: K = 1,
 * point_cluster 1, point_level 0, death 0.  n < min_cl_size: K = 1 and every point leaves the
 * root at the heaviest weight.  Synchronises (K returns to the host). */
int hdb_flat_cluster_tree(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne,
                          int64_t n, int32_t min_cl_size, int64_t cap, int64_t *n_tree, int32_t *parent,
                          double *birth, double *death, double *stability, int32_t *size, int32_t *min_id,
                          int32_t *flat_label, int32_t *point_cluster, double *point_level, int64_t *n_clusters);

/* Upper bound of K for n points: max(1, 2 * floor(n / min_cl_size) - 1) (leaf clusters are
 * disjoint with >= min_cl_size points each, every split has >= 2 children); 0 for n <= 0.
 * Host only, no context. */
int64_t hdb_cluster_tree_bound(int64_t n, int32_t min_cl_size);

/* Hierarchy rows at arbitrary levels (the DBSCAN*-style partitions; HDBSCANStar.java:393-414)
 * from the arrays of hdb_flat_cluster_tree.  labels_out is L x n, row-major: row l holds the tree
 * labels while every edge of weight <= levels[l] is still present:
 *   0 when levels[l] < point_level[x]; otherwise start at C = point_cluster[x] and move to
 *   parent[C] while birth[C] <= levels[l] (the root's NaN birth stops the walk).
 * So a cluster's points carry the parent's label AT its birth level, a point is still in its
 * cluster AT its own level, any level >= the heaviest weight (+inf too) gives all 1 and any level
 * below every point level gives all 0.  Levels may come in any order, repeat, and be +-inf; a
 * NaN level is HDB_EINVAL.  L == 0 or n == 0 is HDB_OK.  Pointer rules as hdb_flat_labels.  The
 * tree is validated, never trusted: point_cluster outside 1..K, parent[i] outside 0..i, or
 * parent[0] != 0 give HDB_EINVAL (no out-of-bounds read on host or device).  The device kernel
 * climbs by binary lifting, O(log K) per (point, level).  Synchronises. */
int hdb_labels_at_levels(hdb_ctx *ctx, const int32_t *parent, const double *birth, int64_t K,
                         const int32_t *point_cluster, const double *point_level, int64_t n,
                         const double *levels, int32_t L, int32_t *labels_out);

/* Out-of-sample labels from the arrays of hdb_flat_cluster_tree (flat_label may equally be the one
 * hdb_constrained_flat_labels returns) and the (nearest, level) pairs of hdb_attach_points.  For
 * query i, y = nearest[i] and e = level[i]:
 *   tree_label[i]  start at C = point_cluster[y] and move to parent[C] while birth[C] <= e (the
 *                  root's NaN birth stops the walk).  No noise rule: a query that reaches y below
 *                  y's own level shares y's last cluster, as y's own flat label does.
 *   labels[i]      the flat_label of the nearest selected cluster on the path from C to the root,
 *                  C included; 0 if there is none.
 *   scores[i]      eps = max(e, point_level[y]); eps == 0 ? 0.0 : 1.0 - eps_max(C) / eps, eps_max as
 *                  in hdb_flat_outlier_scores: the subtree minimum of death, for the root its
 *                  descendants only (Double.MAX_VALUE for a root that never splits).
 * nearest[i] == -1: tree label 0, label 0, score 1.0.  Every output is nullable.  m == 0: HDB_OK.
 * The input is validated, never trusted (no out-of-bounds access on host or device): nearest
 * outside -1..n-1, a NaN level where nearest >= 0, and the tree checks of hdb_labels_at_levels
 * give HDB_EINVAL with a message naming the field.  Pointer rules as hdb_labels_at_levels: host,
 * device or mixed, ctx may be NULL when every pointer is host memory; both paths give the same
 * bits.  The device climbs by the level cut's binary lifting (kernel timer "predict_labels").
 * Synchronises. */
int hdb_predict_labels(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                       const int32_t *flat_label, int64_t K, const int32_t *point_cluster,
                       const double *point_level, int64_t n, const int32_t *nearest, const double *level,
                       int64_t m, int32_t *tree_label, int32_t *labels, double *scores);

/* ---------------------------------------------------------------- soft clustering
 * Exemplars, exemplar distances and membership vectors: how strongly a point -- a training point or
 * a new row -- belongs to each selected cluster.  The reference has no such routine: the contract is
 * this library's own, restated in plain numpy over oracle distances (tests/soft_reference.py), and
 * every comparison is bit-exact.
 * Levels are distances: smaller means denser.  The arithmetic is FP64 with no contraction (no FMA).
 * Every sum over clusters runs in ascending flat label.  Where a host and a device path exist they
 * give the same bits.  Results that are NaN (they need negative, NaN or non-finite levels, or NaN
 * entries in dmin) are out of scope: the value is whatever the arithmetic gives.
 * Inputs are the arrays of hdb_flat_cluster_tree (K clusters; entry i describes tree label i + 1)
 * plus a selection flat_label (K) with values 0..C: the tree's own, or the one
 * hdb_constrained_flat_labels returns; C is the caller's count of selected clusters.  The selected
 * cluster c_f of flat label f is the lowest tree label that carries f; an f that no cluster carries
 * is an empty cluster (no exemplar, tree part 0).  The tree is validated with the rules of
 * hdb_labels_at_levels and never trusted: parent[0] != 0, parent[i] outside 0..i, point_cluster
 * outside 1..K, and a flat_label outside 0..C, give HDB_EINVAL and nothing has been written; there
 * is no out-of-bounds read on host or device.
 *
 * 1. Exemplars: hdb_exemplars.
 *   A tree cluster is a leaf when no cluster names it as parent.  Point x is an exemplar when
 *   point_cluster[x] is a leaf and point_level[x] equals (== on doubles, -0.0 == 0.0) the smallest
 *   point_level, under '<' from +inf, among the points with that point_cluster; a NaN level is
 *   neither.  Its cluster is f(x), the flat_label of the nearest selected cluster on the path from
 *   point_cluster[x] to the root, the leaf included; exemplars with f(x) = 0 are dropped.
 *   ids (int32, room for n entries; the first offsets[C] are written) lists the exemplars ordered by
 *   (f, id); offsets (int64, C + 1) has the segment of flat label f at offsets[f - 1] ..
 *   offsets[f].  *n_exemplars (host, nullable) receives offsets[C].  A selected cluster without an
 *   exemplar cannot arise from a real tree, but the format allows an empty segment.  The selection
 *   itself is host work, O(n + K): device arrays are copied down and the result up; ctx may be NULL
 *   when every pointer is host memory.  Synchronises.
 *
 * 2. Exemplar distances: hdb_exemplar_distances (device only, like hdb_attach_points).
 *   dist(i, e) = DistanceCalculator.computeDistance(Q[i], X[ids[e]]), the query row first, in the
 *   operation order of hdb_attach_points: the bits of hdb_distance_rows.  All five metrics, every
 *   d >= 1.  dmin (m x C, row-major, 64-bit indexing): dmin[i][f - 1] = the minimum over the
 *   exemplars e of segment f under numeric '<'; a NaN distance is never a candidate; a -0.0 result is
 *   stored as +0.0; +inf when the segment is empty or every distance is NaN.
 *   ids (n_ids) and offsets (C + 1) are arbitrary caller arrays: an id outside 0..n-1, offsets[0]
 *   != 0, a descending pair, or offsets[C] != n_ids give HDB_EINVAL and dmin has not been written.
 *   m == 0 or C == 0: HDB_OK.  Pointer rules as hdb_knn.  Kernel timers "soft_scan", "soft_merge".
 *   The candidate tiles are split over workgroup columns when m alone gives too few workgroups, and a
 *   second kernel merges the columns' minima; the minimum is exact and commutative, so the count
 *   changes no bit.  hdb_exemplar_distances_splits is the same call with that count as an
 *   argument: 0 chooses it (what hdb_exemplar_distances does), 1..65535 forces it, anything else is
 *   HDB_EINVAL; stat "soft_last_splits" = the count of the last call.
 *   Memory: the output is m * C doubles.  Scratch beyond it is the gathered exemplar rows
 *   (n_ids * d doubles), their packed copy and the packed queries (rows padded to a multiple of 8
 *   columns) and, with more than one column, splits * m * C doubles of partial minima (a chosen
 *   count keeps these within 2^25 doubles).  The caller chunks Q when that is too much.
 *
 * 3. Membership vectors: hdb_membership_vectors.
 *   Query i is described by an anchor cluster a = anchor[i] (a tree label 1..K, or 0 for "no
 *   anchor"; anything else is HDB_EINVAL), a level l = level[i] and its row of dmin (m x C).
 *   A training point uses (point_cluster, point_level); a new row uses the tree_label of
 *   hdb_predict_labels and max(level, point_level[nearest]) of hdb_attach_points, anchor 0 when
 *   nearest is -1.
 *   Merge level: with A = LCA(a, c) in the tree, B(c) = birth of A's child on the path to c when A
 *     is a proper ancestor of c (c's own root when a forest leaves them without a common
 *     ancestor), B(c) = -inf when a == c or a lies in c's subtree; M = B(c) > l ? B(c) : l.
 *     A root's birth is NaN (hdb_flat_cluster_tree), the further roots of a forest included: as
 *     B(c) it fails the comparison, so M = l, as for -inf.
 *   Tree part: t[f] = M == 0 ? 1.0 : eps_max(c_f) / M with M taken for c = c_f; eps_max as in
 *     hdb_predict_labels (the subtree minimum of death; the root: its descendants only).  For
 *     finite non-negative levels t lies in [0, 1].
 *   Probability: prob = min(1.0, max over f of t[f]), the maximum taken from 0.0 under '>'.
 *   Distance part: Z = { f : dmin[f] <= 0 }.  Z non-empty: dv[f] = 1.0 / |Z| on Z, 0 elsewhere.
 *     Else r[f] = 1.0 / dmin[f] (0 for +inf), S = the sum of r in ascending f, dv[f] = r[f] / S,
 *     all 0 when S == 0.
 *   Result: p[f] = dv[f] * t[f], P = the sum of p in ascending f,
 *     vectors[i][f - 1] = P == 0 ? 0.0 : prob * (p[f] / P).  a == 0: a row of zeros and prob 0.
 *   labels[i] = the first f whose entry exceeds ('>') every entry before it and 0.0, i.e. 1 + the
 *     index of the row's first maximum, or 0 when the whole row is zero.
 *   vectors (m x C) is required when m * C > 0; prob (m) and labels (m) are nullable.  m == 0:
 *   HDB_OK.  Pointer rules as hdb_labels_at_levels: host, device or mixed, ctx may be NULL when
 *   every pointer is host memory.  The device finds every LCA by binary lifting over the level
 *   cut's ancestor tables, O(log K) per (query, cluster); kernel timer "soft_membership".
 *   Synchronises. */
int hdb_exemplars(hdb_ctx *ctx, const int32_t *parent, const int32_t *flat_label, int64_t K, int64_t C,
                  const int32_t *point_cluster, const double *point_level, int64_t n, int32_t *ids,
                  int64_t *offsets, int64_t *n_exemplars);
int hdb_exemplar_distances(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *ids, int64_t n_ids,
                           const int64_t *offsets, int64_t C, const double *Q, int64_t m, int32_t metric,
                           double *dmin);
int hdb_exemplar_distances_splits(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *ids,
                                  int64_t n_ids, const int64_t *offsets, int64_t C, const double *Q, int64_t m,
                                  int32_t metric, int32_t splits, double *dmin);
int hdb_membership_vectors(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                           const int32_t *flat_label, int64_t K, int64_t C, const int32_t *anchor,
                           const double *level, const double *dmin, int64_t m, double *vectors, double *prob,
                           int32_t *labels);

/* Semi-supervised flat extraction (Main.java:49,434-436 "constraints=<file>"; Constraint.java,
 * HDBSCANStar.calculateNumConstraintsSatisfied :738-789, the constraint branches of
 * Cluster.propagate :98-142, findProminentClusters) from the arrays of hdb_flat_cluster_tree:
 * parent / stability / min_id (K each) and point_cluster (n), in tree labels.  m constraints:
 * ca[k], cb[k] are point ids, ctype[k] one of the two values below.
 *   last(x) = point_cluster[x]; anc(C) = C and its ancestors; L = LCA(last(a), last(b)).
 *   num_sat[C]  (numConstraintsSatisfied): a must-link pair adds 2 to every C in anc(L), the root
 *     included, a == b too; a cannot-link pair adds 1 to every C from last(a) up to but excluding
 *     L, and the same for b (nothing when last(a) == last(b); never to the root).
 *   virt[C]: for a cluster with children, the cannot-link endpoints x with last(x) == C (both
 *     endpoints, a == b too); 0 for a leaf.
 *   Children before parents, a node's children in ASCENDING TREE LABEL:
 *     prop_sat[C] = virt[C] + sum of chosen_sat(child); prop_stability[C] = 0.0 + the children's
 *     chosen_stab, one IEEE addition per child in that order; both 0 for a leaf.
 *     A non-root C is chosen as itself when it is a leaf, or num_sat > prop_sat, or
 *     num_sat == prop_sat && stability >= prop_stability (a NaN stability loses); then
 *     chosen = (num_sat, stability), else chosen = (prop_sat, prop_stability).  The root is never
 *     chosen; 0.5 * prop_sat[root] / m is the satisfied fraction the reference prints.
 *   The selected clusters are the topmost self-chosen ones below the root on each chain;
 *   flat_label numbers them 1..n_clusters by ascending (min_id, tree label), 0 for every other
 *   cluster; labels[x] = flat_label of the nearest selected cluster in anc(last(x)), else 0.
 *   With m == 0 flat_label and labels are exactly those of hdb_flat_cluster_tree / hdb_flat_labels.
 * Outputs: num_sat, prop_sat, prop_stability, flat_label (K each), labels (n), n_clusters (host);
 * each may be NULL on its own.  Counts are int32 (Java int): m > 2^30 - 1 is HDB_EINVAL, checked
 * before any array is read.  The input is validated, never trusted: parent[0] != 0, parent[i]
 * outside 0..i (a further cluster with parent 0 is a root of its own: never chosen), point_cluster outside 1..K, a point id outside 0..n-1 or a type other than 0 / 1
 * give HDB_EINVAL with a message naming the field (no out-of-bounds access on host or device; the
 * outputs are then undefined).  K == 1: n_clusters 0, every label 0, num_sat[0] = 2 * the
 * must-link count.  K == 0 (the tree of n == 0): HDB_OK.  Pointer rules as hdb_labels_at_levels
 * (host, device or mixed; ctx may be NULL when every pointer is host memory).  Synchronises. */
#define HDB_CONSTRAINT_MUST_LINK 0
#define HDB_CONSTRAINT_CANNOT_LINK 1
int hdb_constrained_flat_labels(hdb_ctx *ctx, const int32_t *parent, const double *stability, const int32_t *min_id,
                                int64_t K, const int32_t *point_cluster, int64_t n, const int32_t *ca,
                                const int32_t *cb, const int32_t *ctype, int64_t m, int32_t *num_sat,
                                int32_t *prop_sat, double *prop_stability, int32_t *flat_label, int32_t *labels,
                                int64_t *n_clusters);

/* -------------------------------------------------- record formats (§8(f) #3)
 * Host-only (no context, no device); see csrc/formats.cpp. */

/* Double.toString(v) (Java layout, shortest round-trip digits) into buf (cap bytes, NUL
 * terminated).  Returns the length (>= 0) or HDB_EINVAL when cap is too small (32 always
 * suffices).  Used by the record writer below. */
int hdb_format_double(double v, char *buf, int32_t cap);

/* MapperDataset_github.call over a text file's bytes (MapperDataset_github.java:12-20):
 * one point per line, fields Double.parseDouble'd, points numbered in file order.
 * strict = 1: s.split(" ") exactly (a doubled space or an empty line -> NumberFormatException);
 * strict = 0: deviation D1 (fields separated by runs of ' '/'\t', blank lines skipped, the
 * first d fields kept).  d = 0 takes the first line's field count.  X = NULL: count only
 * (*n_out points, *d_out columns); else X holds cap points of *d_out doubles.
 * Errors: HDB_EREF_NUMBER_FORMAT (bad field), HDB_EREF_OOB (short line). */
int hdb_parse_points(const char *text, int64_t len, int32_t d, int32_t strict, double *X, int64_t cap,
                     int64_t *n_out, int32_t *d_out);

/* CreateLocalMST's local-MST text (CreateLocalMST.java:110-123): "v1 v2 w f1 f2 node" per
 * edge, '\n'-joined, no trailing newline, w via Double.toString; fake1/fake2/node nullable
 * (written as 0).  out = NULL: *len_out = the byte length; else out (cap bytes) receives
 * the text plus a NUL. */
int hdb_format_mst_records(const int32_t *va, const int32_t *vb, const double *w, const int32_t *fake1,
                           const int32_t *fake2, const int32_t *node, int64_t ne, char *out, int64_t cap,
                           int64_t *len_out);

/* UnionFindReducer.call's record parse (UnionFindReducer.java:22-45): split("\n"),
 * split(" "), Integer.parseInt / Double.parseDouble of fields 0-5.  va = NULL: count only.
 * Errors: HDB_EREF_OOB (fewer than 6 fields), HDB_EREF_NUMBER_FORMAT. */
int hdb_parse_mst_records(const char *text, int64_t len, int32_t *va, int32_t *vb, double *w, int32_t *fake1,
                          int32_t *fake2, int32_t *node, int64_t cap, int64_t *ne_out);

#ifdef __cplusplus
}
#endif
#endif /* HDBMI_H */
