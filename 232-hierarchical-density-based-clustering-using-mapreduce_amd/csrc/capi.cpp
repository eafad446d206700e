// capi.cpp -- extern "C" entry points of libhdbmi (declared in include/hdbmi.h).
// Each entry: validate, select the device, stage host arrays (Stager), run the device
// building blocks on the context stream, copy host outputs back.
#include <algorithm>
#include <vector>

#include <chrono>

#include "internal.hpp"

using namespace hdb;

namespace {

template <class T>
std::vector<T> to_host(hdb_ctx *ctx, const T *p, size_t count) {
    std::vector<T> v(count);
    if (!count) return v;
    if (is_device_ptr(p)) {
        HIP_CHECK(hipMemcpyAsync(v.data(), p, sizeof(T) * count, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
        std::copy(p, p + count, v.begin());
    }
    return v;
}

void check_metric(int metric) {
    if (metric < HDB_METRIC_EUCLIDEAN || metric > HDB_METRIC_SUPREMUM) HDB_THROW(HDB_EINVAL, "unknown metric");
}

// The hierarchy entries also run on the host, without a context (all pointers in host memory, no
// device needed): one argument check, then the part the context selects.
template <class D, class H>
int host_or_device(hdb_ctx *ctx, bool bad, D &&device_part, H &&host_part) {
    const auto check = [&] {
        if (bad) HDB_THROW(HDB_EINVAL, "bad arguments");
    };
    if (!ctx)
        return entry([&] {
            check();
            return host_part();
        });
    return guarded(ctx, [&] {
        check();
        return device_part();
    });
}

// CSR offsets of P partitions (host copy, P + 1 values): they start at 0 and never decrease, and
// with int32_parts no partition has more than INT32_MAX rows.  Returns the edge count: rows - 1
// tree edges per non-empty partition, plus its rows with self_edges.
int64_t check_offsets(const std::vector<int64_t> &offs, int P, bool self_edges, bool int32_parts) {
    if (offs[0] != 0) HDB_THROW(HDB_EINVAL, "offsets[0] must be 0");
    int64_t ne = 0;
    for (int p = 0; p < P; p++) {
        const int64_t np_ = offs[p + 1] - offs[p];
        if (np_ < 0) HDB_THROW(HDB_EINVAL, "offsets must be non-decreasing");
        if (int32_parts && np_ > INT32_MAX) HDB_THROW(HDB_EINVAL, "partition too large");
        if (np_ > 0) ne += (np_ - 1) + (self_edges ? np_ : 0);
    }
    return ne;
}

}  // namespace

extern "C" {

int hdb_distance_rows(hdb_ctx *ctx, const double *a, const double *b, int64_t n, int32_t d, int32_t metric,
                      double *out) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (n < 0 || d <= 0 || !a || !b || !out) HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager s(ctx);
        const double *da = s.in(a, n * d), *db = s.in(b, n * d);
        double *dout = s.out(out, n);
        distance_rows_device(ctx, da, db, n, d, metric, dout);
        s.finish();
    });
}

int hdb_core_distances(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t min_pts, int32_t metric,
                       int32_t semantics, double *core_out) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (n < 0 || d <= 0 || !X || !core_out || min_pts < 1) HDB_THROW(HDB_EINVAL, "bad arguments");
        if (semantics < 0 || semantics > 2) HDB_THROW(HDB_EINVAL, "unknown core semantics");
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        double *dc = s.out(core_out, n);
        core_distances_device(ctx, dX, n, d, min_pts, metric, semantics, dc);
        s.finish();
    });
}

int hdb_knn(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t k, int32_t metric, int32_t excl_self,
            double *dist_out, int32_t *idx_out) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (n < 0 || d <= 0 || k < 1 || !X || !dist_out) HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        double *dv = s.out(dist_out, n * k);
        int32_t *di = s.out(idx_out, n * k);
        int KC = 0;
        // lists with the bucket width, then compact to k columns
        int kc_guess = k <= 1 ? 1 : (k <= 3 ? 3 : (k <= 7 ? 7 : (k <= 15 ? 15 : 31)));
        double *lv = (double *)arena(ctx, A_WORK0, sizeof(double) * std::max<int64_t>(n * kc_guess, 1));
        int32_t *li = di ? (int32_t *)arena(ctx, A_WORK1, sizeof(int32_t) * std::max<int64_t>(n * kc_guess, 1)) : nullptr;
        knn_lists_device(ctx, dX, n, d, k, metric, excl_self != 0, lv, li, &KC);
        if (n > 0) {
            HIP_CHECK(hipMemcpy2DAsync(dv, sizeof(double) * k, lv, sizeof(double) * KC, sizeof(double) * k, n,
                                       hipMemcpyDeviceToDevice, ctx->stream));
            if (di)
                HIP_CHECK(hipMemcpy2DAsync(di, sizeof(int32_t) * k, li, sizeof(int32_t) * KC, sizeof(int32_t) * k, n,
                                           hipMemcpyDeviceToDevice, ctx->stream));
        }
        s.finish();
    });
}

static void prim_common(hdb_ctx *ctx, const double *X, const int64_t *offsets, int32_t P, int32_t d,
                        const double *core, const int32_t *ids, const double *eB, const double *nnB, int32_t metric,
                        int32_t self_edges, int32_t *va, int32_t *vb, double *w) {
    check_metric(metric);
    if (P < 0 || d <= 0 || !X || !core || !va || !vb || !w) HDB_THROW(HDB_EINVAL, "bad arguments");
    std::vector<int64_t> offs = to_host(ctx, offsets, (size_t)P + 1);
    const int64_t ne = check_offsets(offs, P, self_edges != 0, true);
    const int64_t n = offs[P];
    Stager s(ctx);
    PrimIn in;
    in.X = s.in(X, n * d);
    in.core = s.in(core, n);
    in.ids = ids ? s.in(ids, n) : nullptr;
    in.eB = eB ? s.in(eB, n) : nullptr;
    in.nnB = nnB ? s.in(nnB, n) : nullptr;
    in.d = d;
    in.metric = metric;
    int32_t *dva = s.out(va, ne), *dvb = s.out(vb, ne);
    double *dw = s.out(w, ne);
    if (!in.ids) {
        // identity per partition: local index within each partition
        std::vector<int32_t> h(n);
        for (int p = 0; p < P; p++)
            for (int64_t i = offs[p]; i < offs[p + 1]; i++) h[i] = (int32_t)(i - offs[p]);
        int32_t *dids = (int32_t *)arena(ctx, A_STAGE_OUT, sizeof(int32_t) * std::max<int64_t>(n, 1));
        HIP_CHECK(hipMemcpyAsync(dids, h.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        in.ids = dids;
    }
    prim_batched_device(ctx, in, offs.data(), P, self_edges, dva, dvb, dw);
    s.finish();
}

int hdb_prim_mst(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core, const int32_t *ids,
                 int32_t metric, int32_t self_edges, int32_t *va, int32_t *vb, double *w) {
    return guarded(ctx, [&] {
        if (n < 1) HDB_THROW(HDB_EINVAL, "n must be >= 1 (new int[n-1])");
        int64_t offs[2] = {0, n};
        prim_common(ctx, X, offs, 1, d, core, ids, nullptr, nullptr, metric, self_edges, va, vb, w);
    });
}

int hdb_prim_mst_batched(hdb_ctx *ctx, const double *X, const int64_t *offsets, int32_t P, int32_t d,
                         const double *core, const int32_t *ids, int32_t metric, int32_t self_edges, int32_t *va,
                         int32_t *vb, double *w) {
    return guarded(ctx, [&] {
        if (!offsets) HDB_THROW(HDB_EINVAL, "offsets is NULL");
        prim_common(ctx, X, offsets, P, d, core, ids, nullptr, nullptr, metric, self_edges, va, vb, w);
    });
}

int hdb_leaf_msts(hdb_ctx *ctx, const double *X, const int64_t *offsets, int32_t P, int32_t d, const int32_t *ids,
                  int32_t min_pts, int32_t metric, double *core_out, int32_t *va, int32_t *vb, double *w) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (!X || !offsets || !ids || !va || !vb || !w || P < 0 || d <= 0 || min_pts < 1)
            HDB_THROW(HDB_EINVAL, "bad arguments");
        std::vector<int64_t> offs = to_host(ctx, offsets, (size_t)P + 1);
        const int64_t ne = check_offsets(offs, P, true, false);
        const int64_t n = offs[P];
        std::vector<int32_t> small;
        std::vector<int32_t> large;
        for (int p = 0; p < P; p++) {
            const int64_t np_ = offs[p + 1] - offs[p];
            if (np_ > 0 && np_ <= 4096) small.push_back(p);
            else if (np_ > 4096) large.push_back(p);
        }
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        const int32_t *dids = s.in(ids, n);
        int32_t *dva = s.out(va, ne), *dvb = s.out(vb, ne);
        double *dw = s.out(w, ne);
        double *dcore = core_out ? s.out(core_out, n)
                                 : (double *)arena(ctx, A_STAGE_OUT, sizeof(double) * std::max<int64_t>(n, 1));
        if (min_pts == 1) {
            HIP_CHECK(hipMemsetAsync(dcore, 0, sizeof(double) * std::max<int64_t>(n, 0), ctx->stream));
        } else {
            // offsets + small list on device
            int64_t *d_off;
            int32_t *d_parts;
            carve(ctx, A_STAGE_IN, [&](Carver &cv) {
                d_off = cv.take<int64_t>(P + 1);
                d_parts = cv.take<int32_t>(P + 1);
            });
            HIP_CHECK(hipMemcpyAsync(d_off, offs.data(), sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice, ctx->stream));
            if (!small.empty())
                HIP_CHECK(hipMemcpyAsync(d_parts, small.data(), sizeof(int32_t) * small.size(), hipMemcpyHostToDevice,
                                         ctx->stream));
            leaf_cores_device(ctx, dX, d, metric, P, d_off, d_parts, (int)small.size(), n, min_pts - 1, dcore);
            HIP_CHECK(hipStreamSynchronize(ctx->stream));  // d_off/d_parts live in a reused arena
            for (int32_t p : large)
                core_distances_device(ctx, dX + offs[p] * d, offs[p + 1] - offs[p], d, min_pts, metric,
                                      HDB_CORE_INCL_SELF_CUMULATIVE, dcore + offs[p]);
        }
        PrimIn in;
        in.X = dX;
        in.core = dcore;
        in.ids = dids;
        in.eB = in.nnB = nullptr;
        in.d = d;
        in.metric = metric;
        prim_batched_device(ctx, in, offs.data(), P, 1, dva, dvb, dw);
        s.finish();
    });
}

int hdb_mst_boruvka(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core, int32_t metric,
                    int32_t self_edges, int32_t *va, int32_t *vb, double *w) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (n < 1 || d <= 0 || !X || !core || !va || !vb || !w) HDB_THROW(HDB_EINVAL, "bad arguments");
        int64_t ne = (n - 1) + (self_edges ? n : 0);
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        const double *dc = s.in(core, n);
        int32_t *dva = s.out(va, ne), *dvb = s.out(vb, ne);
        double *dw = s.out(w, ne);
        boruvka_device(ctx, dX, n, d, dc, metric, dva, dvb, dw);
        if (self_edges) self_edges_device(ctx, dc, n, dva + (n - 1), dvb + (n - 1), dw + (n - 1));
        s.finish();
    });
}

int hdb_exact_mst(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t min_pts, int32_t metric,
                  int32_t semantics, int32_t self_edges, double *core_out, int32_t *va, int32_t *vb, double *w) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (n < 1 || d <= 0 || !X || !va || !vb || !w) HDB_THROW(HDB_EINVAL, "bad arguments");
        if (semantics < 0 || semantics > 2) HDB_THROW(HDB_EINVAL, "unknown core semantics");
        if (self_edges & ~(HDB_EDGES_SELF | HDB_EDGES_MERGED)) HDB_THROW(HDB_EINVAL, "unknown edge flags");
        const int64_t ne = (n - 1) + ((self_edges & HDB_EDGES_SELF) ? n : 0);
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        double *dc = core_out ? s.out(core_out, n) : (double *)arena(ctx, A_STAGE_OUT, sizeof(double) * (size_t)n);
        int32_t *dva = s.out(va, ne), *dvb = s.out(vb, ne);
        double *dw = s.out(w, ne);
        exact_leaf_device(ctx, dX, n, d, min_pts, metric, semantics, dc, self_edges, dva, dvb, dw);
        s.finish();
    });
}

int hdb_nearest_sample(hdb_ctx *ctx, const double *X, int64_t n, const double *S, int64_t m, int32_t d,
                       int32_t metric, const int32_t *x_key, const int32_t *s_key, int32_t *nearest_out,
                       double *dist_out) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (n < 0 || m < 0 || d <= 0 || !X || (!S && m > 0) || !nearest_out) HDB_THROW(HDB_EINVAL, "bad arguments");
        if ((x_key == nullptr) != (s_key == nullptr)) HDB_THROW(HDB_EINVAL, "x_key and s_key go together");
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        const double *dS = m ? s.in(S, m * d) : nullptr;
        const int32_t *dxk = s.in(x_key, n), *dsk = s.in(s_key, m);
        int32_t *dn = s.out(nearest_out, n);
        double *dd = s.out(dist_out, n);
        nearest_sample_device(ctx, dX, n, dS, m, d, metric, dxk, dsk, dn, dd);
        s.finish();
    });
}

int hdb_attach_points(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core, const double *Q,
                      int64_t m, int32_t min_pts, int32_t metric, double *core_q, int32_t *nearest, double *level) {
    return hdb_attach_points_splits(ctx, X, n, d, core, Q, m, min_pts, metric, 0, core_q, nearest, level);
}

int hdb_attach_points_splits(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const double *core,
                             const double *Q, int64_t m, int32_t min_pts, int32_t metric, int32_t attach_splits,
                             double *core_q, int32_t *nearest, double *level) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (attach_splits < 0 || attach_splits > 65535) HDB_THROW(HDB_EINVAL, "attach_splits must be in 0..65535");
        if (n < 0 || m < 0 || d <= 0 || min_pts < 1 || (n > 0 && (!X || !core)) || (m > 0 && (!Q || !nearest || !level)))
            HDB_THROW(HDB_EINVAL, "bad arguments");
        if (n > (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "attach: n must be below 2^31 (int32 ids)");
        Stager s(ctx);
        const double *dX = s.in(X, (size_t)n * d), *dc = s.in(core, (size_t)n);
        const double *dQ = s.in(Q, (size_t)m * d);
        double *dcq = s.out(core_q, (size_t)m), *dl = s.out(level, (size_t)m);
        int32_t *dn = s.out(nearest, (size_t)m);
        attach_points_device(ctx, dX, n, d, dc, dQ, m, min_pts, metric, attach_splits, dcq, dn, dl);
        s.finish();
    });
}

int hdb_validity_index(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *labels, int32_t K,
                       int32_t metric, double *index, double *validity, double *sparseness, double *separation,
                       int32_t *nearest_cluster, int32_t *size, double *apts_core, int32_t *internal) {
    return hdb_validity_index_route(ctx, X, n, d, labels, K, metric, 0, HDB_VALIDITY_SMALL_MAX, index, validity,
                                    sparseness, separation, nearest_cluster, size, apts_core, internal);
}

int hdb_validity_index_splits(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *labels, int32_t K,
                              int32_t metric, int32_t splits, double *index, double *validity, double *sparseness,
                              double *separation, int32_t *nearest_cluster, int32_t *size, double *apts_core,
                              int32_t *internal) {
    return hdb_validity_index_route(ctx, X, n, d, labels, K, metric, splits, HDB_VALIDITY_SMALL_MAX, index, validity,
                                    sparseness, separation, nearest_cluster, size, apts_core, internal);
}

int hdb_validity_index_route(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *labels, int32_t K,
                             int32_t metric, int32_t splits, int32_t small_max, double *index, double *validity,
                             double *sparseness, double *separation, int32_t *nearest_cluster, int32_t *size,
                             double *apts_core, int32_t *internal) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (splits < 0 || splits > 65535) HDB_THROW(HDB_EINVAL, "validity: splits must be in 0..65535");
        if (n < 0 || d <= 0 || K < 0 || !index || (n > 0 && (!X || !labels))) HDB_THROW(HDB_EINVAL, "bad arguments");
        if (n >= (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "validity: n must be below 2^31 (int32 ids)");
        ValidityResult r;
        {
            Stager s(ctx);
            const double *dX = s.in(X, (size_t)n * d);
            const int32_t *dl = s.in(labels, (size_t)n);
            double *dc = s.out(apts_core, (size_t)n);
            int32_t *di = s.out(internal, (size_t)n);
            validity_index_device(ctx, dX, n, d, dl, K, metric, splits, small_max, r, dc, di);
            s.finish();
        }
        // the K-length results are host values: to the caller's memory, wherever it is
        const auto put = [&](void *dst, const void *src, size_t bytes) {
            if (!dst || !bytes) return;
            if (is_device_ptr(dst))
                HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
            else
                std::memcpy(dst, src, bytes);
        };
        const size_t nk = (size_t)K;
        put(validity, r.validity.data(), 8 * nk);
        put(sparseness, r.sparseness.data(), 8 * nk);
        put(separation, r.separation.data(), 8 * nk);
        put(nearest_cluster, r.nearest.data(), 4 * nk);
        put(size, r.size.data(), 4 * nk);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));  // r dies with this call
        *index = r.index;
    });
}

int hdb_bubble_stats(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *bubble_of, int64_t nb,
                     int32_t variant, double *ls, double *ss, double *rep, double *info) {
    return guarded(ctx, [&] {
        if (n < 0 || nb < 0 || d <= 0 || (!X && n) || (!bubble_of && n) || !ls || !ss || !rep || !info)
            HDB_THROW(HDB_EINVAL, "bad arguments");
        if (variant != HDB_BUBBLE_COMBINESTEP && variant != HDB_BUBBLE_CF) HDB_THROW(HDB_EINVAL, "unknown variant");
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        const int32_t *dbo = s.in(bubble_of, n);
        double *dls = s.out(ls, nb * d), *dss = s.out(ss, nb * d), *drep = s.out(rep, nb * d), *dinfo = s.out(info, nb * 3);
        bubble_stats_device(ctx, dX, n, d, dbo, nb, variant, dls, dss, drep, dinfo);
        s.finish();
    });
}

int hdb_bubble_partials(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *bubble_of, int64_t nb,
                        const int64_t *cuts, int32_t S, double *part_ls, double *part_ss, double *part_n) {
    return guarded(ctx, [&] {
        if (n < 0 || nb < 0 || d <= 0 || (!X && n) || (!bubble_of && n) || !cuts || !part_ls || !part_ss || !part_n)
            HDB_THROW(HDB_EINVAL, "bad arguments");
        if (S < 1 || S > HDB_MAX_BUBBLE_SLICES) HDB_THROW(HDB_EINVAL, "bubble slices: 1..HDB_MAX_BUBBLE_SLICES");
        std::vector<int64_t> h_cuts = to_host(ctx, cuts, (size_t)S + 1);
        Stager s(ctx);
        const double *dX = s.in(X, n * d);
        const int32_t *dbo = s.in(bubble_of, n);
        double *pl = s.out(part_ls, (int64_t)S * nb * d), *pq = s.out(part_ss, (int64_t)S * nb * d),
               *pn = s.out(part_n, (int64_t)S * nb);
        bubble_partials_device(ctx, dX, n, d, dbo, nb, h_cuts.data(), S, pl, pq, pn);
        s.finish();
    });
}

int hdb_bubble_combine(hdb_ctx *ctx, const double *part_ls, const double *part_ss, const double *part_n, int32_t S,
                       int64_t nb, int32_t d, double *ls, double *ss, double *rep, double *info) {
    return guarded(ctx, [&] {
        if (nb < 0 || d <= 0 || S < 1 || !part_ls || !part_ss || !part_n || !ls || !ss || !rep || !info)
            HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager s(ctx);
        const double *pl = s.in(part_ls, (int64_t)S * nb * d), *pq = s.in(part_ss, (int64_t)S * nb * d),
                     *pn = s.in(part_n, (int64_t)S * nb);
        double *dls = s.out(ls, nb * d), *dss = s.out(ss, nb * d), *drep = s.out(rep, nb * d), *dinfo = s.out(info, nb * 3);
        bubble_combine_device(ctx, pl, pq, pn, S, nb, d, dls, dss, drep, dinfo);
        s.finish();
    });
}

static void bubble_core_impl(hdb_ctx *ctx, const double *rep, const int32_t *nB, const double *eB, const double *nnB,
                             int64_t b, int32_t d, int32_t min_pts, int32_t metric, std::vector<double> &core_h) {
    const int K = min_pts - 1;
    core_h.assign(b, 0.0);
    if (min_pts == 1 || b == 0) return;
    Stager s(ctx);
    const double *drep = s.in(rep, b * d), *deB = s.in(eB, b), *dnnB = s.in(nnB, b);
    double *knn = (double *)arena(ctx, A_WORK0, sizeof(double) * b * K);
    int32_t *lg = (int32_t *)arena(ctx, A_WORK1, sizeof(int32_t) * b * K);
    bubble_knn_device(ctx, drep, deB, dnnB, b, d, metric, K, knn, lg);
    std::vector<double> knn_h = to_host(ctx, (const double *)knn, (size_t)(b * K));
    std::vector<int32_t> lg_h = to_host(ctx, (const int32_t *)lg, (size_t)(b * K));
    std::vector<double> rep_h = to_host(ctx, rep, (size_t)(b * d)), eB_h = to_host(ctx, eB, (size_t)b),
                        nnB_h = to_host(ctx, nnB, (size_t)b);
    std::vector<int32_t> nB_h = to_host(ctx, nB, (size_t)b);
    int rc = bubble_core_epilogue(rep_h.data(), nB_h.data(), eB_h.data(), nnB_h.data(), b, d, min_pts, metric,
                                  knn_h.data(), lg_h.data(), core_h.data());
    if (rc) HDB_THROW(rc, "calculateCoreDistancesBubbles raised a reference exception");
    s.finish();
}

int hdb_bubble_core_distances(hdb_ctx *ctx, const double *rep, const int32_t *nB, const double *eB,
                              const double *nnB, int64_t b, int32_t d, int32_t min_pts, int32_t metric,
                              double *core_out) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (b < 0 || d <= 0 || min_pts < 1 || !rep || !nB || !eB || !nnB || !core_out)
            HDB_THROW(HDB_EINVAL, "bad arguments");
        if (min_pts > 32) HDB_THROW(HDB_EINVAL, "minPts too large (max 32)");
        std::vector<double> core_h;
        bubble_core_impl(ctx, rep, nB, eB, nnB, b, d, min_pts, metric, core_h);
        if (is_device_ptr(core_out)) {
            HIP_CHECK(hipMemcpyAsync(core_out, core_h.data(), sizeof(double) * b, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
        } else {
            std::copy(core_h.begin(), core_h.end(), core_out);
        }
    });
}

int hdb_bubble_prim_mst(hdb_ctx *ctx, const double *rep, const double *eB, const double *nnB,
                        const int32_t *id_bubbles, const double *core, int64_t b, int32_t d, int32_t metric,
                        int32_t self_edges, int32_t *va, int32_t *vb, double *w) {
    return guarded(ctx, [&] {
        if (b < 1) HDB_THROW(HDB_EINVAL, "b must be >= 1");
        if (!eB || !nnB) HDB_THROW(HDB_EINVAL, "eB/nnB required");
        int64_t offs[2] = {0, b};
        prim_common(ctx, rep, offs, 1, d, core, id_bubbles, eB, nnB, metric, self_edges, va, vb, w);
    });
}

int hdb_quicksort_edges(int32_t *va, int32_t *vb, double *w, int64_t ne) {
    if (!va || !vb || !w || ne < 0) return HDB_EINVAL;
    return entry([&] {  // the sort allocates ne-sized host arrays
        const int rc = quicksort_edges(va, vb, w, ne);
        if (rc) set_error("quicksortByEdgeWeight: stack overflow (ArrayIndexOutOfBoundsException)");
        return rc;
    });
}

// core_in (nullable, host or device, b values): the bubble core distances already computed by
// hdb_bubble_core_distances on the same (rep, nB, eB, nnB) -- the model then starts at the Prim.
// The outputs are written by the host algorithm: host memory only (a device pointer is EINVAL)
static int local_model_impl(hdb_ctx *ctx, const double *rep, const double *info, int64_t b, int32_t d,
                            int32_t min_pts, int32_t min_cl_size, int32_t metric, const double *core_in,
                            int32_t *labels, int32_t *mst_va, int32_t *mst_vb, double *mst_w, int32_t *ic_va,
                            int32_t *ic_vb, double *ic_w, int64_t *n_ic) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (b < 1 || d <= 0 || !rep || !info || !labels || min_pts < 1) HDB_THROW(HDB_EINVAL, "bad arguments");
        if (min_pts > 32) HDB_THROW(HDB_EINVAL, "minPts too large (max 32)");
        for (const void *o : {(const void *)labels, (const void *)mst_va, (const void *)mst_vb, (const void *)mst_w,
                              (const void *)ic_va, (const void *)ic_vb, (const void *)ic_w, (const void *)n_ic})
            if (is_device_ptr(o)) HDB_THROW(HDB_EINVAL, "local model: outputs must be host memory (device pointer given)");
        std::vector<double> rep_h = to_host(ctx, rep, (size_t)(b * d));
        std::vector<double> info_h = to_host(ctx, info, (size_t)(b * 3));
        std::vector<double> eB(b), nnB(b);
        std::vector<int32_t> nB(b), ids(b);
        for (int64_t i = 0; i < b; i++) {  // LocalModelReduceByKey.java:80-84
            eB[i] = info_h[i * 3 + 0];
            nnB[i] = info_h[i * 3 + 1];
            nB[i] = (int32_t)info_h[i * 3 + 2];
            ids[i] = (int32_t)i;  // D4: vertex id == position
        }
        using clk = std::chrono::steady_clock;
        auto us = [](clk::time_point a, clk::time_point b) {
            return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
        };
        auto t0 = clk::now();
        std::vector<double> core;
        if (core_in)
            core = to_host(ctx, core_in, (size_t)b);
        else
            bubble_core_impl(ctx, rep_h.data(), nB.data(), eB.data(), nnB.data(), b, d, min_pts, metric, core);
        auto t1 = clk::now();
        const int64_t ne = 2 * b - 1;
        std::vector<int32_t> mva(ne), mvb(ne);
        std::vector<double> mw(ne);
        {
            int64_t offs[2] = {0, b};
            prim_common(ctx, rep_h.data(), offs, 1, d, core.data(), ids.data(), eB.data(), nnB.data(), metric, 1,
                        mva.data(), mvb.data(), mw.data());
        }
        auto t2 = clk::now();
        for (auto &v : g_lm_us) v = 0;
        std::vector<int32_t> lab(b);
        std::vector<int32_t> iva(ne), ivb(ne);
        std::vector<double> iw(ne);
        int64_t nic = 0;
        int rc = local_model_host(rep_h.data(), eB.data(), nnB.data(), nB.data(), b, d, min_cl_size, metric, mva.data(),
                                  mvb.data(), mw.data(), lab.data(), iva.data(), ivb.data(), iw.data(), &nic);
        ctx->stats["lm_core_us"] += us(t0, t1);
        ctx->stats["lm_prim_us"] += us(t1, t2);
        ctx->stats["lm_quicksort_us"] += g_lm_us[0];
        ctx->stats["lm_tree_us"] += g_lm_us[1];
        ctx->stats["lm_fosc_us"] += g_lm_us[2];
        ctx->stats["lm_fosc_select_us"] += g_lm_us[3];
        ctx->stats["lm_fosc_label_us"] += g_lm_us[4];
        ctx->stats["lm_fosc_noise_us"] += g_lm_us[5];
        ctx->stats["lm_calls"] += 1;
        if (rc == HDB_EREF_NEGATIVE_CLUSTER) HDB_THROW(rc, local_model_error_detail());
        if (rc) HDB_THROW(rc, "local model raised a reference exception");
        std::copy(lab.begin(), lab.end(), labels);
        if (mst_va) std::copy(mva.begin(), mva.end(), mst_va);
        if (mst_vb) std::copy(mvb.begin(), mvb.end(), mst_vb);
        if (mst_w) std::copy(mw.begin(), mw.end(), mst_w);
        if (ic_va) std::copy(iva.begin(), iva.begin() + nic, ic_va);
        if (ic_vb) std::copy(ivb.begin(), ivb.begin() + nic, ic_vb);
        if (ic_w) std::copy(iw.begin(), iw.begin() + nic, ic_w);
        if (n_ic) *n_ic = nic;
    });
}

int hdb_local_model(hdb_ctx *ctx, const double *rep, const double *info, int64_t b, int32_t d, int32_t min_pts,
                    int32_t min_cl_size, int32_t metric, int32_t *labels, int32_t *mst_va, int32_t *mst_vb,
                    double *mst_w, int32_t *ic_va, int32_t *ic_vb, double *ic_w, int64_t *n_ic) {
    return local_model_impl(ctx, rep, info, b, d, min_pts, min_cl_size, metric, nullptr, labels, mst_va, mst_vb,
                            mst_w, ic_va, ic_vb, ic_w, n_ic);
}

int hdb_local_model_cores(hdb_ctx *ctx, const double *rep, const double *info, int64_t b, int32_t d,
                          int32_t min_pts, int32_t min_cl_size, int32_t metric, const double *core, int32_t *labels,
                          int32_t *mst_va, int32_t *mst_vb, double *mst_w, int32_t *ic_va, int32_t *ic_vb,
                          double *ic_w, int64_t *n_ic) {
    if (!core) return entry([] { HDB_THROW(HDB_EINVAL, "hdb_local_model_cores: core is required"); });
    return local_model_impl(ctx, rep, info, b, d, min_pts, min_cl_size, metric, core, labels, mst_va, mst_vb, mst_w,
                            ic_va, ic_vb, ic_w, n_ic);
}

int hdb_sort_edges_desc(hdb_ctx *ctx, int32_t *va, int32_t *vb, double *w, int64_t ne) {
    return guarded(ctx, [&] {
        if (ne < 0 || (ne > 0 && (!va || !vb || !w))) HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager s(ctx);
        int32_t *dva = s.inout(va, ne), *dvb = s.inout(vb, ne);
        double *dw = s.inout(w, ne);
        sort_edges_desc_device(ctx, dva, dvb, dw, ne);
        s.finish();
    });
}

int hdb_merge_sorted_runs(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, const int64_t *run_off,
                          int32_t nruns, int32_t *oa, int32_t *ob, double *ow) {
    return guarded(ctx, [&] {
        if (nruns < 0 || (nruns > 0 && !run_off)) HDB_THROW(HDB_EINVAL, "bad arguments");
        std::vector<int64_t> off = nruns ? to_host(ctx, run_off, (size_t)nruns + 1) : std::vector<int64_t>(1, 0);
        for (int r = 0; r < nruns; r++)
            if (off[r + 1] < off[r] || off[0] != 0) HDB_THROW(HDB_EINVAL, "merge_sorted_runs: bad run offsets");
        const int64_t ne = off.back();
        if (ne > INT32_MAX) HDB_THROW(HDB_EINVAL, "too many edges");
        if (ne > 0 && (!va || !vb || !w || !oa || !ob || !ow)) HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager s(ctx);
        const int32_t *da = s.in(va, ne), *db = s.in(vb, ne);
        const double *dw = s.in(w, ne);
        int32_t *xa = s.out(oa, ne), *xb = s.out(ob, ne);
        double *xw = s.out(ow, ne);
        merge_sorted_runs_device(ctx, da, db, dw, off, xa, xb, xw);
        s.finish();
    });
}

int hdb_local_mst_ids(hdb_ctx *ctx, const int32_t *ids, int64_t n, const int32_t *va, const int32_t *vb,
                      const double *w, int64_t ne, int32_t node, int32_t *fake1, int32_t *fake2, int32_t *node_out) {
    return guarded(ctx, [&] {
        if (n < 0 || ne < 0 || (ne > 0 && (!va || !vb || !fake1 || !fake2))) HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager sg(ctx);
        const int32_t *di = sg.in(ids, (size_t)n);
        const int32_t *da = sg.in(va, (size_t)ne), *db = sg.in(vb, (size_t)ne);
        const double *dw = sg.in(w, (size_t)ne);
        int32_t *f1 = sg.out(fake1, (size_t)ne), *f2 = sg.out(fake2, (size_t)ne), *nd = sg.out(node_out, (size_t)ne);
        local_mst_ids_device(ctx, di, n, da, db, dw, ne, node, f1, f2, nd);
        sg.finish();
    });
}

int hdb_flat_labels(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                    int32_t min_cl_size, int32_t *labels, int64_t *n_clusters) {
    const bool bad = ne < 0 || n < 0 || (ne > 0 && (!va || !vb || !w)) || (n > 0 && !labels);
    return host_or_device(
        ctx, bad,
        [&] {
            // device algorithm (K6, flat.hip); host arrays are staged
            Stager sg(ctx);
            const int32_t *da = sg.in(va, (size_t)ne), *db = sg.in(vb, (size_t)ne);
            const double *dw = sg.in(w, (size_t)ne);
            int32_t *dl = sg.out(labels, (size_t)std::max<int64_t>(n, 0));
            flat_labels_device(ctx, da, db, dw, ne, n, min_cl_size, dl, n_clusters);
            sg.finish();
        },
        [&] { return flat_labels_host(va, vb, w, ne, n, min_cl_size, labels, n_clusters); });
}

int hdb_flat_outlier_scores(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne, int64_t n,
                            int32_t min_cl_size, double *scores, double *noise_level, int32_t *labels,
                            int64_t *n_clusters) {
    const bool bad = ne < 0 || n < 0 || (ne > 0 && (!va || !vb || !w)) || (n > 0 && !scores);
    return host_or_device(
        ctx, bad,
        [&] {
            Stager sg(ctx);
            const int32_t *da = sg.in(va, (size_t)ne), *db = sg.in(vb, (size_t)ne);
            const double *dw = sg.in(w, (size_t)ne);
            const size_t np = (size_t)std::max<int64_t>(n, 0);
            double *ds = sg.out(scores, np), *dn = sg.out(noise_level, np);
            int32_t *dl = sg.out(labels, np);
            flat_outlier_scores_device(ctx, da, db, dw, ne, n, min_cl_size, ds, dn, dl, n_clusters);
            sg.finish();
        },
        [&] { return flat_outlier_scores_host(va, vb, w, ne, n, min_cl_size, scores, noise_level, labels, n_clusters); });
}

int64_t hdb_cluster_tree_bound(int64_t n, int32_t min_cl_size) { return cluster_tree_bound(n, min_cl_size); }

int hdb_flat_cluster_tree(hdb_ctx *ctx, const int32_t *va, const int32_t *vb, const double *w, int64_t ne,
                          int64_t n, int32_t min_cl_size, int64_t cap, int64_t *n_tree, int32_t *parent,
                          double *birth, double *death, double *stability, int32_t *size, int32_t *min_id,
                          int32_t *flat_label, int32_t *point_cluster, double *point_level, int64_t *n_clusters) {
    const bool bad = ne < 0 || n < 0 || cap < 0 || !n_tree || (ne > 0 && (!va || !vb || !w));
    return host_or_device(
        ctx, bad,
        [&] {
            Stager sg(ctx);
            const int32_t *da = sg.in(va, (size_t)ne), *db = sg.in(vb, (size_t)ne);
            const double *dw = sg.in(w, (size_t)ne);
            // staged per-cluster outputs are sized by what the tree can hold, not by a generous cap
            const size_t nk = (size_t)std::min<int64_t>(cap, cluster_tree_bound(n, std::max<int32_t>(min_cl_size, 2)));
            const size_t np = (size_t)n;
            ClusterTreeOut t{(int64_t)nk, n_tree, sg.out(parent, nk), sg.out(birth, nk), sg.out(death, nk),
                             sg.out(stability, nk), sg.out(size, nk), sg.out(min_id, nk), sg.out(flat_label, nk),
                             sg.out(point_cluster, np), sg.out(point_level, np)};
            flat_cluster_tree_device(ctx, da, db, dw, ne, n, min_cl_size, t, n_clusters);
            sg.finish();
        },
        [&] {
            const ClusterTreeOut t{cap, n_tree, parent, birth, death, stability, size, min_id, flat_label,
                                   point_cluster, point_level};
            return flat_cluster_tree_host(va, vb, w, ne, n, min_cl_size, t, nullptr, n_clusters);
        });
}

int hdb_labels_at_levels(hdb_ctx *ctx, const int32_t *parent, const double *birth, int64_t K,
                         const int32_t *point_cluster, const double *point_level, int64_t n,
                         const double *levels, int32_t L, int32_t *labels_out) {
    const bool bad = K < 0 || n < 0 || L < 0 || (L > 0 && !levels) || (K > 0 && (!parent || !birth)) ||
                     (n > 0 && (!point_cluster || !point_level)) || (n > 0 && L > 0 && !labels_out);
    return host_or_device(
        ctx, bad,
        [&] {
            Stager sg(ctx);
            const int32_t *dp = sg.in(parent, (size_t)K), *dpc = sg.in(point_cluster, (size_t)n);
            const double *db = sg.in(birth, (size_t)K), *dpl = sg.in(point_level, (size_t)n);
            const double *dlv = sg.in(levels, (size_t)L);
            int32_t *dout = sg.out(labels_out, (size_t)L * (size_t)n);
            labels_at_levels_device(ctx, dp, db, K, dpc, dpl, n, dlv, L, dout);
            sg.finish();
        },
        [&] { return labels_at_levels_host(parent, birth, K, point_cluster, point_level, n, levels, L, labels_out); });
}

int hdb_predict_labels(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                       const int32_t *flat_label, int64_t K, const int32_t *point_cluster,
                       const double *point_level, int64_t n, const int32_t *nearest, const double *level,
                       int64_t m, int32_t *tree_label, int32_t *labels, double *scores) {
    const bool bad = K < 0 || n < 0 || m < 0 || (K > 0 && (!parent || !birth || !death || !flat_label)) ||
                     (n > 0 && (!point_cluster || !point_level)) || (m > 0 && (!nearest || !level));
    return host_or_device(
        ctx, bad,
        [&] {
            if (m == 0) return;
            Stager sg(ctx);
            const size_t nk = (size_t)K, np = (size_t)n, nm = (size_t)m;
            const int32_t *dp = sg.in(parent, nk), *dfl = sg.in(flat_label, nk), *dpc = sg.in(point_cluster, np);
            const double *db = sg.in(birth, nk), *dd = sg.in(death, nk), *dpl = sg.in(point_level, np);
            const int32_t *dnr = sg.in(nearest, nm);
            const double *dlv = sg.in(level, nm);
            int32_t *dtl = sg.out(tree_label, nm), *dlab = sg.out(labels, nm);
            double *dsc = sg.out(scores, nm);
            predict_labels_device(ctx, dp, db, dd, dfl, K, dpc, dpl, n, dnr, dlv, m, dtl, dlab, dsc);
            sg.finish();
        },
        [&] {
            return predict_labels_host(parent, birth, death, flat_label, K, point_cluster, point_level, n, nearest,
                                       level, m, tree_label, labels, scores);
        });
}

int hdb_exemplars(hdb_ctx *ctx, const int32_t *parent, const int32_t *flat_label, int64_t K, int64_t C,
                  const int32_t *point_cluster, const double *point_level, int64_t n, int32_t *ids,
                  int64_t *offsets, int64_t *n_exemplars) {
    const bool bad = K < 0 || C < 0 || n < 0 || !offsets || (K > 0 && (!parent || !flat_label)) ||
                     (n > 0 && (!point_cluster || !point_level || !ids));
    return host_or_device(
        ctx, bad,
        [&] {  // the selection is host work: device arrays come down, the results go back up
            const auto hp = to_host(ctx, parent, (size_t)K), hf = to_host(ctx, flat_label, (size_t)K);
            const auto hc = to_host(ctx, point_cluster, (size_t)n);
            const auto hl = to_host(ctx, point_level, (size_t)n);
            std::vector<int32_t> hi((size_t)n);
            std::vector<int64_t> ho((size_t)C + 1);
            const int64_t E = exemplars_host(hp.data(), hf.data(), K, C, hc.data(), hl.data(), n, hi.data(), ho.data());
            const auto put = [&](void *dst, const void *src, size_t bytes) {
                if (!bytes) return;
                if (is_device_ptr(dst))
                    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
                else
                    std::memcpy(dst, src, bytes);
            };
            put(ids, hi.data(), sizeof(int32_t) * (size_t)E);
            put(offsets, ho.data(), sizeof(int64_t) * ((size_t)C + 1));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host copies die with this call
            if (n_exemplars) *n_exemplars = E;
        },
        [&] {
            std::vector<int64_t> ho((size_t)C + 1);  // nothing is written when the input is refused
            std::vector<int32_t> hi((size_t)n);
            const int64_t E = exemplars_host(parent, flat_label, K, C, point_cluster, point_level, n, hi.data(), ho.data());
            std::copy(hi.begin(), hi.begin() + E, ids);
            std::copy(ho.begin(), ho.end(), offsets);
            if (n_exemplars) *n_exemplars = E;
            return HDB_OK;
        });
}

int hdb_exemplar_distances(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *ids, int64_t n_ids,
                           const int64_t *offsets, int64_t C, const double *Q, int64_t m, int32_t metric,
                           double *dmin) {
    return hdb_exemplar_distances_splits(ctx, X, n, d, ids, n_ids, offsets, C, Q, m, metric, 0, dmin);
}

int hdb_exemplar_distances_splits(hdb_ctx *ctx, const double *X, int64_t n, int32_t d, const int32_t *ids,
                                  int64_t n_ids, const int64_t *offsets, int64_t C, const double *Q, int64_t m,
                                  int32_t metric, int32_t splits, double *dmin) {
    return guarded(ctx, [&] {
        check_metric(metric);
        if (splits < 0 || splits > 65535) HDB_THROW(HDB_EINVAL, "exemplar distances: splits must be in 0..65535");
        if (n < 0 || m < 0 || d <= 0 || n_ids < 0 || C < 0 || !offsets || (n > 0 && !X) || (n_ids > 0 && !ids) ||
            (m > 0 && !Q) || (m > 0 && C > 0 && !dmin))
            HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager s(ctx);
        const double *dX = s.in(X, (size_t)n * d), *dQ = s.in(Q, (size_t)m * d);
        const int32_t *di = s.in(ids, (size_t)n_ids);
        const int64_t *dof = s.in(offsets, (size_t)C + 1);
        double *dd = s.out(dmin, (size_t)m * (size_t)C);
        exemplar_distances_device(ctx, dX, n, d, di, n_ids, dof, C, dQ, m, metric, splits, dd);
        s.finish();
    });
}

int hdb_membership_vectors(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                           const int32_t *flat_label, int64_t K, int64_t C, const int32_t *anchor,
                           const double *level, const double *dmin, int64_t m, double *vectors, double *prob,
                           int32_t *labels) {
    const bool bad = K < 0 || C < 0 || m < 0 || (K > 0 && (!parent || !birth || !death || !flat_label)) ||
                     (m > 0 && (!anchor || !level)) || (m > 0 && C > 0 && (!dmin || !vectors));
    return host_or_device(
        ctx, bad,
        [&] {
            if (m == 0) return;
            Stager sg(ctx);
            const size_t nk = (size_t)K, nm = (size_t)m, nmc = (size_t)m * (size_t)C;
            const int32_t *dp = sg.in(parent, nk), *dfl = sg.in(flat_label, nk), *da = sg.in(anchor, nm);
            const double *db = sg.in(birth, nk), *dd = sg.in(death, nk), *dlv = sg.in(level, nm);
            const double *ddm = sg.in(dmin, nmc);
            double *dv = sg.out(vectors, nmc), *dpr = sg.out(prob, nm);
            int32_t *dlab = sg.out(labels, nm);
            membership_vectors_device(ctx, dp, db, dd, dfl, K, C, da, dlv, ddm, m, dv, dpr, dlab);
            sg.finish();
        },
        [&] {
            return membership_vectors_host(parent, birth, death, flat_label, K, C, anchor, level, dmin, m, vectors, prob,
                                           labels);
        });
}

int hdb_constrained_flat_labels(hdb_ctx *ctx, const int32_t *parent, const double *stability, const int32_t *min_id,
                                int64_t K, const int32_t *point_cluster, int64_t n, const int32_t *ca,
                                const int32_t *cb, const int32_t *ctype, int64_t m, int32_t *num_sat,
                                int32_t *prop_sat, double *prop_stability, int32_t *flat_label, int32_t *labels,
                                int64_t *n_clusters) {
    if (!ctx)  // the host path makes its own checks
        return entry([&] {
            const ConstrainedOut o{num_sat, prop_sat, prop_stability, flat_label, labels, n_clusters};
            return constrained_flat_labels_host(parent, stability, min_id, K, point_cluster, n, ca, cb, ctype, m, o);
        });
    return guarded(ctx, [&] {
        // the same checks, here before any array is staged
        if (m > HDB_MAX_CONSTRAINTS) HDB_THROW(HDB_EINVAL, "constrained flat labels: m exceeds 2^30 - 1 constraints");
        if (K < 0 || n < 0 || m < 0 || (K > 0 && (!parent || !stability || !min_id)) || (n > 0 && !point_cluster) ||
            (m > 0 && (!ca || !cb || !ctype)))
            HDB_THROW(HDB_EINVAL, "bad arguments");
        Stager sg(ctx);
        const size_t nk = (size_t)K, np = (size_t)n, nm = (size_t)m;
        const int32_t *dp = sg.in(parent, nk), *dmin = sg.in(min_id, nk), *dpc = sg.in(point_cluster, np);
        const double *dst = sg.in(stability, nk);
        const int32_t *da = sg.in(ca, nm), *db = sg.in(cb, nm), *dt = sg.in(ctype, nm);
        const ConstrainedOut o{sg.out(num_sat, nk),    sg.out(prop_sat, nk), sg.out(prop_stability, nk),
                               sg.out(flat_label, nk), sg.out(labels, np),   n_clusters};
        constrained_flat_labels_device(ctx, dp, dst, dmin, K, dpc, n, da, db, dt, m, o);
        sg.finish();
    });
}

}  // extern "C"
