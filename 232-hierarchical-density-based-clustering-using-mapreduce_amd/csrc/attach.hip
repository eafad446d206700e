// attach.hip -- the attach scan of out-of-sample prediction (hdb_attach_points): for every query
// row, its core distance against the training rows and the training row it reaches through its
// cheapest mutual-reachability edge.  A tiled all-pairs FP64 scan of one set of rows against
// another, in the style of K1 (knn_impl.hpp) and K2g (boruvka_generic.hip): a lane owns one
// query, candidate rows arrive wave-uniformly in tiles, no FMA.
//
// Contract (include/hdbmi.h): dist(i, j) = computeDistance(Q[i], X[j]), the query row first.
//   core_q[i]  entry K - 1 of the ascending list of the K = minPts - 1 smallest dist(i, j), built
//              by the strict '<' insertion into a Double.MAX_VALUE buffer (HDBSCANStar.java:79-97):
//              a NaN distance, or one not below Double.MAX_VALUE, never enters.
//   w(i, j)    dist(i, j), replaced by core_q[i], then core[j], on a strict '>' only
//              (HDBSCANStar.java:162-168); a NaN core never raises a weight, a -0.0 core acts as
//              +0.0, a pair whose w is NaN is no candidate, +inf is a candidate like any other.
//   nearest[i] the j that minimises the strict total order (w, s, j); s = K2g's tie key: the
//              squared distance summed in dimension order for Euclidean, else the distance.
//   level[i]   that w.  No candidate: nearest = -1, level = Double.MAX_VALUE.
//
// Bit parity with metric_distance, exactly as K2g has it: each pair's sum runs over the
// dimensions in order, in chunks of ATT_DC with the running sum carried across chunks; rows are
// packed to a multiple of ATT_DC with zeros, which change no sum; cosine's m1 / m2 and Pearson's
// mean, centred coordinates and s1 / s2 depend on one row alone and are hoisted into the packing
// pass by the same operations (cosine and Pearson then share OP_DOT).
//
// Two passes over one tile loader, because the weight needs core_q: pass 1 (timer attach_knn)
// builds the lists in registers, pass 2 (timer attach_min) finds the arg-min.  m is often small
// against n, so the candidate tiles are split over grid.y (hdb_attach_points_splits forces the count, stat
// attach_last_splits); each split writes a partial list / a partial (w, s, j) minimum per query
// and a second kernel merges them: the K smallest of the union of the splits' lists are the K
// smallest of all rows, and the minimum of the splits' minima under the same total order is the
// minimum over all rows -- the split count cannot change a bit of the output.
//
// Launch rules: plain launches only, no workgroup waits on another, every loop is bounded by the
// tile count, scratch comes from the context's arenas (one packed copy of X and Q, the partials),
// indices are 64-bit.  Stream-ordered: nothing here reads a result on the host.
#include <algorithm>

#include "attach_scan.hpp"

namespace hdb {

namespace {

// The tile constants (ATT_QT, ATT_CT, ATT_DC, ATT_CB), the packing pass and the fold / batch /
// finish functors are in attach_scan.hpp, shared with the exemplar-distance scan (soft.hip).

// Pass 1.  grid: (ceil(m / ATT_QT), splits); split y scans tiles [y * tps, (y + 1) * tps).  Every
// lane keeps the KC >= K smallest distances of its query in registers and stores them to
// plist[(y * KC + k) * m + q].
template <int OP, int KC>
__global__ __launch_bounds__(ATT_QT) void att_knn_kernel(const double *__restrict__ Xp, const double *__restrict__ xnrm,
                                                         int64_t n, int64_t ntiles, int64_t tps,
                                                         const double *__restrict__ Qp, const double *__restrict__ qnrm,
                                                         int64_t m, int dp, double *__restrict__ plist) {
    const int64_t q = (int64_t)blockIdx.x * ATT_QT + threadIdx.x;
    if (q - (threadIdx.x & 63) >= m) return;  // a wave without a query
    const bool inr = q < m;
    const int64_t r = inr ? q : m - 1;
    const double *qrow = Qp + r * dp;
    const double qn = qnrm[r];
    const int nch = dp / ATT_DC;
    double xq[ATT_DC];
#pragma unroll
    for (int i = 0; i < ATT_DC; i++) xq[i] = qrow[i];
    double buf[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) buf[k] = JMAX;
    const int64_t t0 = (int64_t)blockIdx.y * tps, t1 = min(t0 + tps, ntiles);
#pragma unroll 1
    for (int64_t t = t0; t < t1; t++) {
        const int64_t j0 = t * ATT_CT;
        const int rows = (int)min((int64_t)ATT_CT, n - j0);
#pragma unroll 1
        for (int jb = 0; jb < rows; jb += ATT_CB) {
            double acc[ATT_CB];
            att_batch<OP>(acc, xq, qrow, Xp + (j0 + jb) * dp, dp, nch);
#pragma unroll
            for (int u = 0; u < ATT_CB; u++) {
                const int64_t j = j0 + jb + u;
                if (j >= n) break;
                double dist, s;
                att_finish<OP>(acc[u], qn, OP == OP_DOT ? xnrm[j] : 0.0, dist, s);
                topk_insert<KC>(buf, dist);  // strict '<': NaN and values not below MAX_VALUE stay out
            }
        }
    }
    if (inr) {
#pragma unroll
        for (int k = 0; k < KC; k++) plist[((int64_t)blockIdx.y * KC + k) * m + q] = buf[k];
    }
}

// merge of the splits' lists: one thread per query, the same strict insertion; core_q = entry K - 1
template <int KC>
__global__ void att_knn_merge_kernel(const double *__restrict__ plist, int64_t m, int splits, int K,
                                     double *__restrict__ core_q) {
    HDB_GRID_STRIDE(q, m) {
        double buf[KC];
#pragma unroll
        for (int k = 0; k < KC; k++) buf[k] = JMAX;
        for (int sp = 0; sp < splits; sp++) {
#pragma unroll
            for (int k = 0; k < KC; k++) topk_insert<KC>(buf, plist[((int64_t)sp * KC + k) * m + q]);
        }
        double v = buf[0];
#pragma unroll
        for (int k = 1; k < KC; k++) v = k == K - 1 ? buf[k] : v;
        core_q[q] = v;
    }
}

__device__ __forceinline__ bool att_key_less(double w, double s, int32_t j, double bw, double bs, int32_t bj) {
    if (bj < 0) return true;
    if (w < bw) return true;
    if (w > bw) return false;
    if (s < bs) return true;
    if (s > bs) return false;
    return j < bj;
}

// Pass 2.  The same grid and tile ranges; every lane keeps the smallest (w, s, j) of its query and
// stores it to slot y * m + q of pw / ps / pj (pj < 0: no candidate in this split).
template <int OP>
__global__ __launch_bounds__(ATT_QT) void att_min_kernel(const double *__restrict__ Xp, const double *__restrict__ xnrm,
                                                         const double *__restrict__ xcore, int64_t n, int64_t ntiles,
                                                         int64_t tps, const double *__restrict__ Qp,
                                                         const double *__restrict__ qnrm,
                                                         const double *__restrict__ core_q, int64_t m, int dp,
                                                         double *__restrict__ pw, double *__restrict__ ps,
                                                         int32_t *__restrict__ pj) {
    const int64_t q = (int64_t)blockIdx.x * ATT_QT + threadIdx.x;
    if (q - (threadIdx.x & 63) >= m) return;
    const bool inr = q < m;
    const int64_t r = inr ? q : m - 1;
    const double *qrow = Qp + r * dp;
    const double qn = qnrm[r], cq = core_q[r];
    const int nch = dp / ATT_DC;
    double xq[ATT_DC];
#pragma unroll
    for (int i = 0; i < ATT_DC; i++) xq[i] = qrow[i];
    double bw = 0.0, bs = 0.0;
    int32_t bj = -1;
    const int64_t t0 = (int64_t)blockIdx.y * tps, t1 = min(t0 + tps, ntiles);
#pragma unroll 1
    for (int64_t t = t0; t < t1; t++) {
        const int64_t j0 = t * ATT_CT;
        const int rows = (int)min((int64_t)ATT_CT, n - j0);
#pragma unroll 1
        for (int jb = 0; jb < rows; jb += ATT_CB) {
            double acc[ATT_CB];
            att_batch<OP>(acc, xq, qrow, Xp + (j0 + jb) * dp, dp, nch);
#pragma unroll
            for (int u = 0; u < ATT_CB; u++) {
                const int64_t j = j0 + jb + u;
                if (j >= n) break;
                double dist, s;
                att_finish<OP>(acc[u], qn, OP == OP_DOT ? xnrm[j] : 0.0, dist, s);
                double w = dist;
                const double cx = xcore[j];
                if (cq > w) w = cq;
                if (cx > w) w = cx;
                if (w != w) continue;  // NaN: no candidate
                if (att_key_less(w, s, (int32_t)j, bw, bs, bj)) {
                    bw = w;
                    bs = s;
                    bj = (int32_t)j;
                }
            }
        }
    }
    if (inr) {
        const int64_t o = (int64_t)blockIdx.y * m + q;
        pw[o] = bw;
        ps[o] = bs;
        pj[o] = bj;
    }
}

// merge of the splits' minima under the same order
__global__ void att_min_merge_kernel(const double *__restrict__ pw, const double *__restrict__ ps,
                                     const int32_t *__restrict__ pj, int64_t m, int splits,
                                     int32_t *__restrict__ nearest, double *__restrict__ level) {
    HDB_GRID_STRIDE(q, m) {
        double bw = 0.0, bs = 0.0;
        int32_t bj = -1;
        for (int sp = 0; sp < splits; sp++) {
            const int64_t o = (int64_t)sp * m + q;
            const int32_t j = pj[o];
            if (j < 0) continue;
            const double w = pw[o], s = ps[o];
            if (att_key_less(w, s, j, bw, bs, bj)) {
                bw = w;
                bs = s;
                bj = j;
            }
        }
        nearest[q] = bj;
        level[q] = bj < 0 ? JMAX : bw;
    }
}

__global__ void att_fill_kernel(double *__restrict__ core_q, double cv, int32_t *__restrict__ nearest,
                                double *__restrict__ level, int64_t m) {
    HDB_GRID_STRIDE(q, m) {
        if (core_q) core_q[q] = cv;
        if (nearest) nearest[q] = -1;
        if (level) level[q] = JMAX;
    }
}

struct AttState {
    double *Xp, *xnrm, *xcore, *Qp, *qnrm, *cq, *plist, *pw, *ps;
    int32_t *pj;
};
AttState att_carve(Carver &cv, int64_t n, int64_t npad, int64_t m, int dp, int splits, int KC, bool own_cq) {
    AttState s;
    s.Xp = cv.take<double>((size_t)npad * dp);
    s.xnrm = cv.take<double>((size_t)n);
    s.xcore = cv.take<double>((size_t)n);
    s.Qp = cv.take<double>((size_t)m * dp);
    s.qnrm = cv.take<double>((size_t)m);
    s.cq = own_cq ? cv.take<double>((size_t)m) : nullptr;
    s.plist = cv.take<double>((size_t)splits * KC * m);
    s.pw = cv.take<double>((size_t)splits * m);
    s.ps = cv.take<double>((size_t)splits * m);
    s.pj = cv.take<int32_t>((size_t)splits * m);
    return s;
}

template <int OP>
void att_knn_launch(int KC, dim3 grid, hipStream_t st, const AttState &s, int64_t n, int64_t ntiles, int64_t tps,
                    int64_t m, int dp) {
#define HDB_ATT_KNN(KCV)                                                                                             \
    hipLaunchKernelGGL((att_knn_kernel<OP, KCV>), grid, dim3(ATT_QT), 0, st, s.Xp, s.xnrm, n, ntiles, tps, s.Qp, s.qnrm, \
                       m, dp, s.plist)
    switch (KC) {
    case 1: HDB_ATT_KNN(1); break;
    case 3: HDB_ATT_KNN(3); break;
    case 7: HDB_ATT_KNN(7); break;
    case 15: HDB_ATT_KNN(15); break;
    default: HDB_ATT_KNN(31); break;
    }
#undef HDB_ATT_KNN
}

}  // namespace

void attach_stats_init(hdb_ctx *ctx) { ctx->stats["attach_last_splits"] = 0; }

void attach_points_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const double *core, const double *Q,
                          int64_t m, int min_pts, int metric, int forced_splits, double *core_q, int32_t *nearest,
                          double *level) {
    if (min_pts < 1) HDB_THROW(HDB_EINVAL, "minPts must be >= 1");
    const int K = min_pts - 1;
    const int KC = K == 0 ? 1 : pick_kc(K);
    if (KC < 0) HDB_THROW(HDB_EINVAL, "minPts too large (max 32)");
    if (n > (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "attach: n must be below 2^31 (int32 ids)");
    if (m == 0) return;
    hipStream_t st = ctx->stream;
    const int gm = (int)std::min<int64_t>(ceil_div(m, 256), 4096);
    const int64_t ntiles = ceil_div(n, (int64_t)ATT_CT), npad = ntiles * ATT_CT;
    const int64_t qblocks = ceil_div(m, (int64_t)ATT_QT);
    // enough workgroups to fill the device twice over when m alone does not give them
    int64_t splits = forced_splits;
    if (splits <= 0) splits = std::max<int64_t>(1, std::min<int64_t>(ceil_div(2 * (int64_t)ctx->num_cus, qblocks), ntiles));
    splits = std::min<int64_t>(splits, 65535);
    ctx->stats["attach_last_splits"] = splits;
    if (n == 0) {  // no candidate at all
        hipLaunchKernelGGL(att_fill_kernel, dim3(gm), dim3(256), 0, st, core_q, K == 0 ? 0.0 : JMAX, nearest, level, m);
        HIP_CHECK(hipGetLastError());
        return;
    }
    const int dp = (int)(ceil_div(d, ATT_DC) * ATT_DC);
    const int64_t tps = ceil_div(ntiles, splits);  // tiles per split; the last splits may be empty
    const AttState s =
        carve(ctx, A_WORK0, [&](Carver &cv) { return att_carve(cv, n, npad, m, dp, (int)splits, KC, core_q == nullptr); });
    double *cq = core_q ? core_q : s.cq;
    const int gn = (int)std::min<int64_t>(ceil_div(n, 256), 4096);
    if (npad > n) HIP_CHECK(hipMemsetAsync(s.Xp + (size_t)n * dp, 0, sizeof(double) * (size_t)(npad - n) * dp, st));
    hipLaunchKernelGGL(att_pack_kernel, dim3(gn), dim3(256), 0, st, X, n, d, dp, metric, core, s.Xp, s.xnrm, s.xcore);
    hipLaunchKernelGGL(att_pack_kernel, dim3(gm), dim3(256), 0, st, Q, m, d, dp, metric, (const double *)nullptr, s.Qp,
                       s.qnrm, (double *)nullptr);
    const dim3 grid((unsigned)qblocks, (unsigned)splits);
    if (K == 0) {  // HDBSCANStar.java:75-77: minPts 1 has no neighbour list, the core distance is 0
        hipLaunchKernelGGL(att_fill_kernel, dim3(gm), dim3(256), 0, st, cq, 0.0, (int32_t *)nullptr, (double *)nullptr, m);
    } else {
        KernelTimer t1(ctx, "attach_knn");
        switch (metric) {
        case HDB_METRIC_EUCLIDEAN: att_knn_launch<OP_SQ>(KC, grid, st, s, n, ntiles, tps, m, dp); break;
        case HDB_METRIC_MANHATTAN: att_knn_launch<OP_ABS>(KC, grid, st, s, n, ntiles, tps, m, dp); break;
        case HDB_METRIC_SUPREMUM: att_knn_launch<OP_MAX>(KC, grid, st, s, n, ntiles, tps, m, dp); break;
        default: att_knn_launch<OP_DOT>(KC, grid, st, s, n, ntiles, tps, m, dp); break;
        }
        switch (KC) {
        case 1: hipLaunchKernelGGL(att_knn_merge_kernel<1>, dim3(gm), dim3(256), 0, st, s.plist, m, (int)splits, K, cq); break;
        case 3: hipLaunchKernelGGL(att_knn_merge_kernel<3>, dim3(gm), dim3(256), 0, st, s.plist, m, (int)splits, K, cq); break;
        case 7: hipLaunchKernelGGL(att_knn_merge_kernel<7>, dim3(gm), dim3(256), 0, st, s.plist, m, (int)splits, K, cq); break;
        case 15: hipLaunchKernelGGL(att_knn_merge_kernel<15>, dim3(gm), dim3(256), 0, st, s.plist, m, (int)splits, K, cq); break;
        default: hipLaunchKernelGGL(att_knn_merge_kernel<31>, dim3(gm), dim3(256), 0, st, s.plist, m, (int)splits, K, cq); break;
        }
    }
    {
        KernelTimer t2(ctx, "attach_min");
        switch (metric) {
        case HDB_METRIC_EUCLIDEAN:
            hipLaunchKernelGGL(att_min_kernel<OP_SQ>, grid, dim3(ATT_QT), 0, st, s.Xp, s.xnrm, s.xcore, n, ntiles, tps, s.Qp,
                               s.qnrm, cq, m, dp, s.pw, s.ps, s.pj);
            break;
        case HDB_METRIC_MANHATTAN:
            hipLaunchKernelGGL(att_min_kernel<OP_ABS>, grid, dim3(ATT_QT), 0, st, s.Xp, s.xnrm, s.xcore, n, ntiles, tps, s.Qp,
                               s.qnrm, cq, m, dp, s.pw, s.ps, s.pj);
            break;
        case HDB_METRIC_SUPREMUM:
            hipLaunchKernelGGL(att_min_kernel<OP_MAX>, grid, dim3(ATT_QT), 0, st, s.Xp, s.xnrm, s.xcore, n, ntiles, tps, s.Qp,
                               s.qnrm, cq, m, dp, s.pw, s.ps, s.pj);
            break;
        default:
            hipLaunchKernelGGL(att_min_kernel<OP_DOT>, grid, dim3(ATT_QT), 0, st, s.Xp, s.xnrm, s.xcore, n, ntiles, tps, s.Qp,
                               s.qnrm, cq, m, dp, s.pw, s.ps, s.pj);
            break;
        }
        hipLaunchKernelGGL(att_min_merge_kernel, dim3(gm), dim3(256), 0, st, s.pw, s.ps, s.pj, m, (int)splits, nearest,
                           level);
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace hdb
