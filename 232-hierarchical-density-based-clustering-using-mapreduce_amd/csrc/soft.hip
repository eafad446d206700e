// soft.hip -- the device side of soft clustering (include/hdbmi.h "soft clustering"): the
// exemplar-distance scan of hdb_exemplar_distances and the membership kernel of
// hdb_membership_vectors.
//
// The scan.  dmin[i][f] = the smallest dist(Q[i], X[ids[e]]) over the exemplars e of segment f
// (offsets[f] <= e < offsets[f + 1]) under numeric '<': a NaN distance is no candidate, -0.0 is
// stored as +0.0, an empty or all-NaN segment gives +inf.  It is the attach scan (attach.hip) with
// another epilogue: a lane owns one query, the candidate rows -- here the exemplar rows, gathered
// into one packed copy in segment order -- arrive wave-uniformly in tiles of ATT_CT rows, ATT_CB at a
// time, through the same packing pass and fold / batch / finish functors (attach_scan.hpp), so
// every distance has the bits of metric_distance.  The row index and the current segment's end are
// wave-uniform: at a segment end every lane stores its running minimum and starts again from +inf,
// with no divergence.  Candidate tiles are split over grid.y when m alone gives too few workgroups
// (hdb_exemplar_distances_splits forces the count, stat soft_last_splits): a split stores the minima
// of the segments its rows belong to into its own m x C slice, and a merge kernel takes, for every
// (query, segment), the minimum over exactly the splits whose rows meet the segment.  The minimum
// of doubles without NaN and with one zero is exact, commutative and associative: the split count
// cannot change a bit.  One split writes the output directly, empty segments included.
//
// Launch rules (as attach.hip): plain launches only, no workgroup waits on another, every loop is
// bounded by the tile count or the segment count, scratch comes from the context's Carver (the
// gathered rows, their packed copy, the packed queries, the partial slices), indices are 64-bit.
// ids and offsets are caller arrays and never trusted: the gather clamps what it reads, a check
// kernel flags what is wrong, and that one word is read on the host before any result is written
// (HDB_EINVAL leaves dmin untouched).  Nothing else is read back.
//
// The membership kernel: one thread per query, three passes over its row of C clusters with the
// sums in ascending flat label (the order is the contract); the merge level of (anchor, cluster)
// comes from an LCA by binary lifting over the ancestor tables of the level cut (flat.hip sections
// 8 and 9, tree_tables_device) and a depth table built from them, O(log K) per pair.
#include <algorithm>

#include "attach_scan.hpp"

namespace hdb {

namespace {

enum : int { SE_IDS = 32, SE_OFFSETS = 64, SE_FLAT = 128, SE_ANCHOR = 256 };

__device__ __forceinline__ void soft_flag(int *err, int e) {
    if (e) atomicOr(err, e);
}

// ------------------------------------------------------------------ the scan
// one thread per exemplar: its row of X, unpacked, in segment order; an id outside 0..n-1 is
// flagged and reads row 0 (n >= 1 here)
__global__ void sf_gather_kernel(const double *__restrict__ X, int64_t n, int d, const int32_t *__restrict__ ids,
                                 int64_t E, double *__restrict__ G, int *__restrict__ err) {
    int e = 0;
    HDB_GRID_STRIDE(pos, E) {
        int64_t id = ids[pos];
        if (id < 0 || id >= n) {
            e = SE_IDS;
            id = 0;
        }
        const double *a = X + id * d;
        double *o = G + pos * d;
        for (int i = 0; i < d; i++) o[i] = a[i];
    }
    soft_flag(err, e);
}

// offsets[0] == 0, offsets[C] == E, ascending
__global__ void sf_check_offsets_kernel(const int64_t *__restrict__ off, int64_t C, int64_t E, int *__restrict__ err) {
    int e = 0;
    HDB_GRID_STRIDE(f, C + 1) {
        const int64_t o = off[f];
        if (f == 0 && o != 0) e = SE_OFFSETS;
        if (f == C && o != E) e = SE_OFFSETS;
        if (f < C && off[f + 1] < o) e = SE_OFFSETS;
    }
    soft_flag(err, e);
}

__global__ void sf_fill_kernel(double *__restrict__ out, int64_t count, double v) {
    HDB_GRID_STRIDE(i, count) out[i] = v;
}

// grid: (ceil(m / ATT_QT), splits); split y scans tiles [y * tps, (y + 1) * tps) and stores into
// out + y * m * C (splits == 1: the output itself).  off is valid here: off[0] = 0 <= ... <=
// off[C] = E, so the segment walk below ends before C.
template <int OP>
__global__ __launch_bounds__(ATT_QT) void sf_scan_kernel(const double *__restrict__ Ep, const double *__restrict__ enrm,
                                                         int64_t E, int64_t ntiles, int64_t tps,
                                                         const int64_t *__restrict__ off, int64_t C,
                                                         const double *__restrict__ Qp, const double *__restrict__ qnrm,
                                                         int64_t m, int dp, double *__restrict__ out, int direct) {
    const int64_t q = (int64_t)blockIdx.x * ATT_QT + threadIdx.x;
    if (q - (threadIdx.x & 63) >= m) return;  // a wave without a query
    const int64_t t0 = (int64_t)blockIdx.y * tps, t1 = min(t0 + tps, ntiles);
    const int64_t r0 = t0 * ATT_CT, r1 = min(t1 * ATT_CT, E);
    if (r0 >= r1) return;  // a split past the last tile
    const bool inr = q < m;
    const int64_t r = inr ? q : m - 1;
    const double *qrow = Qp + r * dp;
    const double qn = qnrm[r];
    const int nch = dp / ATT_DC;
    double xq[ATT_DC];
#pragma unroll
    for (int i = 0; i < ATT_DC; i++) xq[i] = qrow[i];
    double *orow = out + ((int64_t)blockIdx.y * m + r) * C;
    // the segment the walk starts in: the first one when this split writes the output itself (it
    // then stores +inf for the empty segments it passes), else the one that holds row r0
    int64_t f = 0;
    if (!direct) {
        int64_t lo = 0, hi = C - 1;  // the smallest f with off[f + 1] > r0; off[C] = E > r0
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (off[mid + 1] > r0)
                hi = mid;
            else
                lo = mid + 1;
        }
        f = lo;
    }
    int64_t fend = off[f + 1];
    double cur = INFINITY;
#pragma unroll 1
    for (int64_t t = t0; t < t1; t++) {
        const int64_t j0 = t * ATT_CT;
        const int rows = (int)min((int64_t)ATT_CT, r1 - j0);
#pragma unroll 1
        for (int jb = 0; jb < rows; jb += ATT_CB) {
            double acc[ATT_CB];
            att_batch<OP>(acc, xq, qrow, Ep + (j0 + jb) * dp, dp, nch);
#pragma unroll
            for (int u = 0; u < ATT_CB; u++) {
                const int64_t j = j0 + jb + u;
                if (j >= r1) break;
                while (j >= fend) {  // wave-uniform: a segment ends; j < E = off[C] keeps f below C
                    if (inr) orow[f] = cur == 0.0 ? 0.0 : cur;
                    cur = INFINITY;
                    f++;
                    fend = off[f + 1];
                }
                double dist, s;
                att_finish<OP>(acc[u], qn, OP == OP_DOT ? enrm[j] : 0.0, dist, s);
                if (dist < cur) cur = dist;  // false for NaN
            }
        }
    }
    if (inr) {
        orow[f] = cur == 0.0 ? 0.0 : cur;
        if (direct)
            for (f++; f < C; f++) orow[f] = INFINITY;  // empty segments after the last row
    }
}

// one thread per (query, segment): the minimum over the splits whose rows meet the segment
__global__ void sf_merge_kernel(const double *__restrict__ part, const int64_t *__restrict__ off, int64_t C, int64_t m,
                                int64_t rows_per_split, double *__restrict__ out) {
    HDB_GRID_STRIDE(idx, m * C) {
        const int64_t f = idx % C;
        const int64_t a = off[f], b = off[f + 1];
        double best = INFINITY;
        if (a < b) {
            const int64_t y1 = (b - 1) / rows_per_split;
            for (int64_t y = a / rows_per_split; y <= y1; y++) {
                const double v = part[y * m * C + idx];
                if (v < best) best = v;
            }
        }
        out[idx] = best;
    }
}

struct SoftScan {
    int *err;
    double *G, *Ep, *enrm, *Qp, *qnrm, *part;
};

// ------------------------------------------------------------------ membership
__device__ __forceinline__ double soft_key_dec(unsigned long long k) {  // flat.hip's ord_dec
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}

// depth by tree label (the root: 1; index 0: 0) from the ancestor rows
__global__ void sm_depth_kernel(const int32_t *__restrict__ anc, int32_t K, int J, int32_t *__restrict__ depth) {
    const int64_t stride = (int64_t)K + 1;
    HDB_GRID_STRIDE(i, stride) {
        int32_t cur = (int32_t)i, dep = 0;
        for (int j = J - 1; j >= 0; j--) {
            const int32_t a = anc[j * stride + cur];
            if (a != 0) {
                cur = a;
                dep += 1 << j;
            }
        }
        depth[i] = i == 0 ? 0 : dep + 1;
    }
}

// sel[f] = the lowest tree label whose flat_label is f (INT32_MAX: none); a value outside 0..C is flagged
__global__ void sm_select_kernel(const int32_t *__restrict__ flat_label, int32_t K, int64_t C, int32_t *__restrict__ sel,
                                 int *__restrict__ err) {
    int e = 0;
    HDB_GRID_STRIDE(i, K) {
        const int32_t f = flat_label[i];
        if (f < 0 || f > C)
            e = SE_FLAT;
        else if (f > 0)
            atomicMin(sel + f, (int32_t)(i + 1));
    }
    soft_flag(err, e);
}
__global__ void sm_fill_kernel(int32_t *__restrict__ sel, int64_t count, int32_t v) {
    HDB_GRID_STRIDE(i, count) sel[i] = v;
}

__device__ __forceinline__ int32_t sm_lift(const int32_t *__restrict__ anc, int64_t stride, int32_t x, int32_t k) {
    for (int j = 0; k != 0; j++, k >>= 1)
        if (k & 1) x = anc[j * stride + x];
    return x;
}

// B(c) for anchor a >= 1 and cluster c >= 1: -inf when a is c or lies below it, else the birth of
// the child of LCA(a, c) on the way to c (in a forest: of c's own root)
__device__ __forceinline__ double sm_merge_birth(const int32_t *__restrict__ anc, const double *__restrict__ bt,
                                                 const int32_t *__restrict__ depth, int64_t stride, int J, int32_t a,
                                                 int32_t c) {
    const int32_t da = depth[a], dc = depth[c];
    int32_t x = a, y = c;
    if (da >= dc) {
        x = sm_lift(anc, stride, a, da - dc);
        if (x == c) return -INFINITY;
    } else {
        y = sm_lift(anc, stride, c, dc - da - 1);
        if (anc[y] == a) return bt[y];
        y = anc[y];
    }
    // x != y at one depth: climb while the ancestors differ
    for (int j = J - 1; j >= 0; j--) {
        const int32_t ax = anc[j * stride + x], ay = anc[j * stride + y];
        if (ax != ay) {
            x = ax;
            y = ay;
        }
    }
    return bt[y];
}

__device__ __forceinline__ double sm_recip(double dm) { return dm == INFINITY ? 0.0 : 1.0 / dm; }

// one thread per query; the row of vectors holds t, then p, then the result
__global__ __launch_bounds__(256) void sm_member_kernel(const int32_t *__restrict__ anc, const double *__restrict__ bt,
                                                         const int32_t *__restrict__ depth,
                                                         const unsigned long long *__restrict__ em,
                                                         const int32_t *__restrict__ sel, int32_t K, int J, int64_t C,
                                                         const int32_t *__restrict__ anchor,
                                                         const double *__restrict__ level,
                                                         const double *__restrict__ dmin, int64_t m,
                                                         double *__restrict__ vectors, double *__restrict__ prob,
                                                         int32_t *__restrict__ labels, int *__restrict__ err) {
    const int64_t stride = (int64_t)K + 1;
    int e = 0;
    HDB_GRID_STRIDE(i, m) {
        int32_t a = anchor[i];
        if (a < 0 || a > K) {
            e = SE_ANCHOR;
            a = 0;
        }
        const double l = level[i];
        const double *dm = dmin + i * C;
        double *row = vectors + i * C;
        if (a == 0) {
            for (int64_t f = 0; f < C; f++) row[f] = 0.0;
            if (prob) prob[i] = 0.0;
            if (labels) labels[i] = 0;
            continue;
        }
        double mx = 0.0, S = 0.0;
        int64_t nz = 0;
        for (int64_t f = 0; f < C; f++) {
            const int32_t c = sel[f + 1];
            double tf = 0.0;
            if (c != INT32_MAX) {
                const double B = sm_merge_birth(anc, bt, depth, stride, J, a, c);
                const double M = B > l ? B : l;
                tf = M == 0.0 ? 1.0 : soft_key_dec(em[c]) / M;
            }
            row[f] = tf;
            if (tf > mx) mx = tf;
            const double v = dm[f];
            if (v <= 0.0)
                nz++;
            else
                S = S + sm_recip(v);
        }
        const double pr = 1.0 < mx ? 1.0 : mx;
        double P = 0.0;
        for (int64_t f = 0; f < C; f++) {
            const double v = dm[f];
            double dv;
            if (nz > 0)
                dv = v <= 0.0 ? 1.0 / (double)nz : 0.0;
            else
                dv = S == 0.0 ? 0.0 : sm_recip(v) / S;
            const double p = dv * row[f];
            row[f] = p;
            P = P + p;
        }
        int32_t lab = 0;
        double best = 0.0;
        for (int64_t f = 0; f < C; f++) {
            const double v = P == 0.0 ? 0.0 : pr * (row[f] / P);
            row[f] = v;
            if (v > best) {
                best = v;
                lab = (int32_t)(f + 1);
            }
        }
        if (prob) prob[i] = pr;
        if (labels) labels[i] = lab;
    }
    soft_flag(err, e);
}

}  // namespace

void soft_stats_init(hdb_ctx *ctx) { ctx->stats["soft_last_splits"] = 0; }

void exemplar_distances_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const int32_t *ids, int64_t E,
                               const int64_t *offsets, int64_t C, const double *Q, int64_t m, int metric,
                               int forced_splits, double *dmin) {
    if (n < 0 || E < 0 || C < 0 || m < 0 || d <= 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    if (n > (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "exemplar distances: n must be below 2^31 (int32 ids)");
    if (E > 0 && C == 0) HDB_THROW(HDB_EINVAL, "exemplar distances: offsets[C] must equal the id count");
    if (m == 0 || C == 0) return;
    if (E > 0 && n == 0) HDB_THROW(HDB_EINVAL, "exemplar distances: id out of range");
    hipStream_t st = ctx->stream;
    const int64_t ntiles = ceil_div(E, (int64_t)ATT_CT), epad = ntiles * ATT_CT;
    const int64_t qblocks = ceil_div(m, (int64_t)ATT_QT);
    // eight workgroups per CU when m alone does not give them (the attach scan's measured optimum
    // for these tiles), while the partial slices stay within 2^25 doubles
    int64_t splits = forced_splits;
    if (splits <= 0) {
        splits = std::max<int64_t>(1, std::min<int64_t>(ceil_div(8 * (int64_t)ctx->num_cus, qblocks), ntiles));
        splits = std::min<int64_t>(splits, std::max<int64_t>(1, (int64_t(1) << 25) / (m * C)));
    }
    splits = std::min<int64_t>(splits, 65535);
    ctx->stats["soft_last_splits"] = splits;
    const int dp = (int)(ceil_div(d, ATT_DC) * ATT_DC);
    const bool direct = splits == 1;
    const SoftScan s = carve(ctx, A_WORK0, [&](Carver &cv) {
        SoftScan s;
        s.err = (int *)cv.take<int64_t>(1);
        s.G = cv.take<double>(E * d);
        s.Ep = cv.take<double>(epad * dp);
        s.enrm = cv.take<double>(E);
        s.Qp = cv.take<double>(m * dp);
        s.qnrm = cv.take<double>(m);
        s.part = cv.take<double>(direct ? 0 : splits * m * C);
        return s;
    });
    HIP_CHECK(hipMemsetAsync(s.err, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(sf_check_offsets_kernel, dim3(grid_for(C + 1)), dim3(256), 0, st, offsets, C, E, s.err);
    if (E > 0) hipLaunchKernelGGL(sf_gather_kernel, dim3(grid_for(E)), dim3(256), 0, st, X, n, d, ids, E, s.G, s.err);
    HIP_CHECK(hipGetLastError());
    int64_t *pin = pinned_words(ctx) + PINNED_WORDS - 8;
    HIP_CHECK(hipMemcpyAsync(pin, s.err, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int e = (int)pin[0];
    if (e & SE_OFFSETS)
        HDB_THROW(HDB_EINVAL, "exemplar distances: offsets must ascend from 0 to the id count");
    if (e & SE_IDS) HDB_THROW(HDB_EINVAL, "exemplar distances: id out of range");
    if (E == 0) {  // every segment is empty
        hipLaunchKernelGGL(sf_fill_kernel, dim3(grid_for(m * C)), dim3(256), 0, st, dmin, m * C, (double)INFINITY);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (epad > E) HIP_CHECK(hipMemsetAsync(s.Ep + (size_t)E * dp, 0, sizeof(double) * (size_t)(epad - E) * dp, st));
    hipLaunchKernelGGL(att_pack_kernel, dim3(grid_for(E)), dim3(256), 0, st, (const double *)s.G, E, d, dp, metric,
                       (const double *)nullptr, s.Ep, s.enrm, (double *)nullptr);
    hipLaunchKernelGGL(att_pack_kernel, dim3(grid_for(m)), dim3(256), 0, st, Q, m, d, dp, metric,
                       (const double *)nullptr, s.Qp, s.qnrm, (double *)nullptr);
    const int64_t tps = ceil_div(ntiles, splits);  // tiles per split; the last splits may be empty
    const dim3 grid((unsigned)qblocks, (unsigned)splits);
    double *out = direct ? dmin : s.part;
    {
        KernelTimer t1(ctx, "soft_scan");
#define HDB_SOFT_SCAN(OP)                                                                                          \
    hipLaunchKernelGGL(sf_scan_kernel<OP>, grid, dim3(ATT_QT), 0, st, s.Ep, s.enrm, E, ntiles, tps, offsets, C, s.Qp, \
                       s.qnrm, m, dp, out, direct ? 1 : 0)
        switch (metric) {
        case HDB_METRIC_EUCLIDEAN: HDB_SOFT_SCAN(OP_SQ); break;
        case HDB_METRIC_MANHATTAN: HDB_SOFT_SCAN(OP_ABS); break;
        case HDB_METRIC_SUPREMUM: HDB_SOFT_SCAN(OP_MAX); break;
        default: HDB_SOFT_SCAN(OP_DOT); break;
        }
#undef HDB_SOFT_SCAN
    }
    if (!direct) {
        KernelTimer t2(ctx, "soft_merge");
        hipLaunchKernelGGL(sf_merge_kernel, dim3(grid_for(m * C)), dim3(256), 0, st, s.part, offsets, C, m,
                           tps * ATT_CT, dmin);
    }
    HIP_CHECK(hipGetLastError());
}

void membership_vectors_device(hdb_ctx *ctx, const int32_t *parent, const double *birth, const double *death,
                               const int32_t *flat_label, int64_t K, int64_t C, const int32_t *anchor,
                               const double *level, const double *dmin, int64_t m, double *vectors, double *prob,
                               int32_t *labels) {
    if (K < 0 || C < 0 || m < 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    if (m == 0) return;
    if (K >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, "membership vectors: too many clusters");
    if (C >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, "membership vectors: too many selected clusters");
    hipStream_t st = ctx->stream;
    KernelTimer tt(ctx, "soft_membership");
    int J = 1;
    while ((int64_t(1) << J) < K) J++;  // 2^J >= K > the deepest chain
    const int64_t stride = K + 1;
    int *err;
    double *bt;
    int32_t *anc, *near_a, *near_b, *depth, *sel;
    unsigned long long *em;
    carve(ctx, A_FLAT1, [&](Carver &cv) {
        err = (int *)cv.take<int64_t>(1);
        bt = cv.take<double>(stride);
        anc = cv.take<int32_t>(stride * J);
        em = cv.take<unsigned long long>(stride);
        near_a = cv.take<int32_t>(stride), near_b = cv.take<int32_t>(stride);
        depth = cv.take<int32_t>(stride);
        sel = cv.take<int32_t>(C + 1);
    });
    HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int64_t), st));
    tree_tables_device(ctx, parent, birth, death, flat_label, (int32_t)K, J, anc, bt, em, near_a, near_b, err);
    hipLaunchKernelGGL(sm_depth_kernel, dim3(grid_for(stride)), dim3(256), 0, st, anc, (int32_t)K, J, depth);
    hipLaunchKernelGGL(sm_fill_kernel, dim3(grid_for(C + 1)), dim3(256), 0, st, sel, C + 1, INT32_MAX);
    if (K > 0)
        hipLaunchKernelGGL(sm_select_kernel, dim3(grid_for(K)), dim3(256), 0, st, flat_label, (int32_t)K, C, sel, err);
    HIP_CHECK(hipGetLastError());
    // the tree and the selection are checked before the kernel that writes the results runs
    int64_t *pin = pinned_words(ctx) + PINNED_WORDS - 8;
    HIP_CHECK(hipMemcpyAsync(pin, err, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    int e = (int)pin[0];
    if (e & TREE_TABLES_BAD_PARENT) HDB_THROW(HDB_EINVAL, "membership vectors: parent label out of range");
    if (e & SE_FLAT) HDB_THROW(HDB_EINVAL, "membership vectors: flat_label out of range");
    hipLaunchKernelGGL(sm_member_kernel, dim3(grid_for(m)), dim3(256), 0, st, anc, bt, depth, em, sel, (int32_t)K, J, C,
                       anchor, level, dmin, m, vectors, prob, labels, err);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(pin, err, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    e = (int)pin[0];
    if (e & SE_ANCHOR) HDB_THROW(HDB_EINVAL, "membership vectors: anchor out of range");
}

}  // namespace hdb
