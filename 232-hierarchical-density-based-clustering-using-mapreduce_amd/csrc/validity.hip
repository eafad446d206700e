// validity.hip -- the DBCV validity index of a labelling (hdb_validity_index): per cluster the
// all-points core distances, the exact mutual-reachability MST over them, its internal nodes and
// sparseness, the separation to the nearest other cluster, and the weighted index.  The contract
// is in include/hdbmi.h; every floating-point operation has one fixed order, so the result is
// bit-exact against a plain restatement (tests/validity_reference.py).
//
// The scans are the tiled all-pairs FP64 scan of attach.hip and K2g (boruvka_generic.hip): a
// lane owns one query, candidate rows arrive wave-uniformly in tiles of VAL_CT rows, VAL_CB
// candidates share one query chunk of VAL_DC dimensions, no FMA.  Bit parity with
// metric_distance as there: sums run over the dimensions in order with the running sum carried
// across chunks, rows are packed to a multiple of VAL_DC with zeros, cosine's and Pearson's
// per-row terms are hoisted into the packing pass by the same operations (both then share OP_DOT).
//
// Steps (validity_index_device):
//  1. group   labels validated and counted, the labelled rows stably sorted by label (member
//             order = ascending id inside a cluster), one packed copy in that order;
//  2. core    val_core_kernel: every wave's 64 queries share a cluster (a host-built tile table)
//             and scan that cluster's members only.  The sum of t^d has the two-level shape of
//             the contract: blocks of HDB_VALIDITY_SUM_BLOCK members, block partials in block
//             order.  With the candidate range split over grid.y the splits fall on block
//             boundaries, every block's partial is stored, and val_core_merge_kernel folds them
//             in block order -- the same additions, so the split count changes no bit.  The
//             partial store is sum_c n_c * blocks_c doubles; a chosen split count is dropped to 1
//             when that exceeds VAL_PARTIAL_MAX doubles (large clusters fill the device with
//             query tiles alone); a forced count is honoured as given.
//             The totals go to the host for std::pow (validity.cpp) and the cores come back.
//  3. MSTs    clusters above small_max members (an argument of the call, default
//             HDB_VALIDITY_SMALL_MAX): boruvka_device on their slice, one by one; the others: val_prim_small_kernel, one workgroup per cluster, a dense Prim
//             whose per-vertex key is the full (w, s, lo, hi) order, keys in LDS.  Under a strict
//             total order the MST is unique, so Prim and Boruvka return the same edges.
//  4. degrees, internal flags (all members when a cluster has no internal edge), sparseness;
//  5. sep     val_sep_kernel over the compacted internal rows, still grouped by cluster: a wave
//             skips candidate tiles wholly inside its own cluster; the per-lane best is
//             (w, label); candidate columns over grid.y, merged per query, then per cluster
//             through atomicMin on the order-preserving image of a double;
//  6. the K-length arrays and the index on the host.
//
// Launch rules: plain launches only, no workgroup waits on another, every loop is bounded by a
// tile, block or member count, scratch comes from the context's carver, indices are 64-bit.
#include <algorithm>
#include <string>
#include <vector>

#include "internal.hpp"
#include "sort.hpp"

namespace hdb {

namespace {

constexpr int VAL_QT = 256;  // queries per workgroup: one per lane, four waves, one tile-table entry per wave
constexpr int VAL_CT = 64;   // rows per candidate tile
constexpr int VAL_DC = 8;    // dimension chunk held in registers
constexpr int VAL_CB = 4;    // candidates evaluated together
constexpr int VAL_SB = HDB_VALIDITY_SUM_BLOCK;
constexpr int64_t VAL_PARTIAL_MAX = int64_t(1) << 22;  // doubles (32 MiB) a chosen split may store
static_assert(VAL_SB % VAL_CB == 0 && VAL_CT % VAL_CB == 0, "blocks and tiles are whole batches");

enum { OP_SQ = 0, OP_ABS = 1, OP_MAX = 2, OP_DOT = 3 };

// order-preserving image of a non-NaN double (-0.0 as +0.0), as K2g's; 0 is below and ~0 above every image
__device__ __forceinline__ unsigned long long ukey(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x == 0.0 ? 0.0 : x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double unukey(unsigned long long u) {
    const unsigned long long b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    double x;
    std::memcpy(&x, &b, 8);
    return x;
}

__global__ void val_count_kernel(const int32_t *__restrict__ labels, int64_t n, int32_t K, int32_t *__restrict__ cnt,
                                 unsigned long long *__restrict__ bad, uint32_t *__restrict__ keys,
                                 int32_t *__restrict__ iota) {
    HDB_GRID_STRIDE(i, n) {
        const int32_t l = labels[i];
        if (l < 0 || l > K)
            atomicMin(bad, (unsigned long long)i);
        else
            atomicAdd(&cnt[l], 1);
        keys[i] = (uint32_t)l;
        iota[i] = (int32_t)i;
    }
}

// One thread per member position: the row of id members[pos] transformed for the metric and packed
// to dp columns (att_pack_kernel's operations), its per-row term, label and id, and the plain row
// for boruvka_device.  A non-finite coordinate reports its row.
__global__ void val_pack_kernel(const double *__restrict__ X, int d, int dp, int metric,
                                const int32_t *__restrict__ members, int64_t M, const int32_t *__restrict__ labels,
                                double *__restrict__ Xp, double *__restrict__ Xc, double *__restrict__ nrm_out,
                                int32_t *__restrict__ glabel, int32_t *__restrict__ gid,
                                unsigned long long *__restrict__ bad) {
    HDB_GRID_STRIDE(pos, M) {
        const int32_t id = members[pos];
        const double *a = X + (int64_t)id * d;
        double *o = Xp + pos * dp, *c = Xc + pos * d;
        double nrm = 0;
        bool finite = true;
        if (metric == HDB_METRIC_PEARSON) {
            double mean = 0;
            for (int i = 0; i < d; i++) mean = mean + a[i];
            mean = mean / d;
            for (int i = 0; i < d; i++) {
                const double t = a[i] - mean;
                o[i] = t;
                nrm = nrm + t * t;
            }
        } else {
            for (int i = 0; i < d; i++) {
                const double t = a[i];
                o[i] = t;
                if (metric == HDB_METRIC_COSINE) nrm = nrm + t * t;
            }
        }
        for (int i = 0; i < d; i++) {
            const double t = a[i];
            c[i] = t;
            finite = finite && fabs(t) <= JMAX;
        }
        for (int i = d; i < dp; i++) o[i] = 0.0;
        nrm_out[pos] = nrm;
        glabel[pos] = labels[id];
        gid[pos] = id;
        if (!finite) atomicMin(bad, (unsigned long long)id);
    }
}

template <int OP>
__device__ __forceinline__ double val_fold(double acc, double a, double b) {
    if (OP == OP_SQ) {
        const double t = a - b;
        return acc + t * t;
    } else if (OP == OP_ABS) {
        return acc + fabs(a - b);
    } else if (OP == OP_MAX) {
        const double t = fabs(a - b);
        return t > acc ? t : acc;
    } else {
        return acc + a * b;
    }
}

// the sums of one batch of VAL_CB candidate rows against the lane's query; xq holds the query's
// first chunk (the whole row when nch == 1)
template <int OP>
__device__ __forceinline__ void val_batch(double (&acc)[VAL_CB], double (&xq)[VAL_DC], const double *__restrict__ qrow,
                                          const double *__restrict__ cbase, int dp, int nch) {
#pragma unroll
    for (int u = 0; u < VAL_CB; u++) acc[u] = 0.0;
#pragma unroll 1
    for (int ch = 0; ch < nch; ch++) {
        if (nch > 1) {
#pragma unroll
            for (int i = 0; i < VAL_DC; i++) xq[i] = qrow[ch * VAL_DC + i];
        }
#pragma unroll
        for (int u = 0; u < VAL_CB; u++) {
            const double *cr = cbase + (int64_t)u * dp + ch * VAL_DC;
#pragma unroll
            for (int i = 0; i < VAL_DC; i++) acc[u] = val_fold<OP>(acc[u], xq[i], cr[i]);
        }
    }
}

// the distance and K2g's tie key of a finished sum
template <int OP>
__device__ __forceinline__ void val_finish(double acc, double qn, double xn, double &dist, double &s) {
    if (OP == OP_SQ) {
        s = acc;
        dist = sqrt(acc);
    } else if (OP == OP_DOT) {
        dist = 1 - (acc / sqrt(qn * xn));
        s = dist;
    } else {
        dist = acc;
        s = dist;
    }
}

// t^d by right-to-left binary exponentiation (the contract's operation order)
__device__ __forceinline__ double val_powi(double t, int d) {
    double r = 1.0, b = t;
    int e = d;
    while (e) {
        if (e & 1) r = r * b;
        e >>= 1;
        if (e) b = b * b;
    }
    return r;
}

// Step 2.  grid: (ceil(ntq / 4), splits); wave = one tile-table entry: up to 64 consecutive
// members of one cluster.  Split y folds sum blocks [y * bps, (y + 1) * bps) of that cluster,
// bps = ceil(blocks / splits).  splits == 1: the total goes to totals[q]; else every block's
// partial goes to pp[pbase[c] + b * n_c + (q - c0)].
template <int OP>
__global__ __launch_bounds__(VAL_QT) void val_core_kernel(const double *__restrict__ Xp, const double *__restrict__ nrm,
                                                          int dp, int d, int64_t ntq,
                                                          const int32_t *__restrict__ qt_start,
                                                          const int32_t *__restrict__ qt_cl,
                                                          const int64_t *__restrict__ coff,
                                                          const int64_t *__restrict__ pbase, int splits,
                                                          double *__restrict__ totals, double *__restrict__ pp) {
    const int64_t tile = (int64_t)blockIdx.x * (VAL_QT / 64) + (threadIdx.x >> 6);
    if (tile >= ntq) return;  // a wave without a tile
    const int32_t c = qt_cl[tile];
    const int64_t c0 = coff[c], c1 = coff[c + 1], nc = c1 - c0;
    const int64_t q = (int64_t)qt_start[tile] + (threadIdx.x & 63);
    const bool inr = q < c1;
    const int64_t r = inr ? q : c1 - 1;
    const double *qrow = Xp + r * dp;
    const double qn = nrm[r];
    const int nch = dp / VAL_DC;
    double xq[VAL_DC];
#pragma unroll
    for (int i = 0; i < VAL_DC; i++) xq[i] = qrow[i];
    const int64_t nb = ceil_div(nc, (int64_t)VAL_SB), bps = ceil_div(nb, (int64_t)splits);
    const int64_t b0 = (int64_t)blockIdx.y * bps, b1 = min(b0 + bps, nb);
    double total = 0.0;
#pragma unroll 1
    for (int64_t b = b0; b < b1; b++) {
        double partial = 0.0;
        const int64_t j0 = c0 + b * VAL_SB, j1 = min(j0 + (int64_t)VAL_SB, c1);
#pragma unroll 1
        for (int64_t jb = j0; jb < j1; jb += VAL_CB) {
            double acc[VAL_CB];
            // rows past j1 inside the last batch are the next cluster's rows or the zero rows of the padding
            val_batch<OP>(acc, xq, qrow, Xp + jb * dp, dp, nch);
#pragma unroll
            for (int u = 0; u < VAL_CB; u++) {
                const int64_t j = jb + u;
                if (j >= j1) break;
                double dist, s;
                val_finish<OP>(acc[u], qn, OP == OP_DOT ? nrm[j] : 0.0, dist, s);
                if (j != r && dist > 0) {  // self, duplicates, negative and NaN values contribute nothing
                    const double t = 1.0 / dist;
                    partial = partial + val_powi(t, d);
                }
            }
        }
        if (splits == 1)
            total = total + partial;
        else if (inr)
            pp[pbase[c] + b * nc + (q - c0)] = partial;
    }
    if (splits == 1 && inr) totals[q] = total;
}

// the block partials of every member folded in block order
__global__ void val_core_merge_kernel(const double *__restrict__ pp, const int32_t *__restrict__ glabel,
                                      const int64_t *__restrict__ coff, const int64_t *__restrict__ pbase, int64_t M,
                                      double *__restrict__ totals) {
    HDB_GRID_STRIDE(q, M) {
        const int32_t c = glabel[q];
        const int64_t c0 = coff[c], nc = coff[c + 1] - c0;
        double total = 0.0;
        if (nc >= 2) {
            const int64_t nb = ceil_div(nc, (int64_t)VAL_SB);
            for (int64_t b = 0; b < nb; b++) total = total + pp[pbase[c] + b * nc + (q - c0)];
        }
        totals[q] = total;
    }
}

// strict total order (w, s, lo, hi) of two edges
__device__ __forceinline__ bool val_key_less(double w, double s, int32_t lo, int32_t hi, double bw, double bs,
                                             int32_t blo, int32_t bhi) {
    if (w < bw) return true;
    if (w > bw) return false;
    if (s < bs) return true;
    if (s > bs) return false;
    if (lo != blo) return lo < blo;
    return hi < bhi;
}

// Step 3, small clusters.  One workgroup per cluster of list[]; vertices are member positions
// 0 .. n_c - 1.  Keys in LDS: kw / ks the cheapest edge of vertex v into the tree, kf its tree end
// (-1: none yet, -2: v is in the tree).  n_c - 1 steps: relax against the vertex added last, select
// the smallest key.  A pair whose w is NaN is no edge; a cluster the tree cannot span reports its
// label (what hdb_mst_boruvka calls non-finite input).  Dynamic LDS: 20 bytes per vertex of maxn.
template <int OP>
__global__ __launch_bounds__(256) void val_prim_small_kernel(const double *__restrict__ Xp,
                                                             const double *__restrict__ nrm,
                                                             const double *__restrict__ gcore, int dp, int maxn,
                                                             const int32_t *__restrict__ list,
                                                             const int64_t *__restrict__ coff,
                                                             int32_t *__restrict__ ea, int32_t *__restrict__ eb,
                                                             double *__restrict__ ew,
                                                             unsigned long long *__restrict__ fail) {
    extern __shared__ double val_lds[];
    double *kw = val_lds, *ks = val_lds + maxn;
    int32_t *kf = (int32_t *)(val_lds + 2 * (size_t)maxn);
    __shared__ double rw[4], rs[4];
    __shared__ int32_t rlo[4], rhi[4], rv[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t c = list[blockIdx.x];
    const int64_t c0 = coff[c];
    const int nc = (int)(coff[c + 1] - c0);
    for (int v = tid; v < nc; v += 256) kf[v] = v == 0 ? -2 : -1;
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int step = 0; step < nc - 1; step++) {
        const double *crow = Xp + (c0 + cur) * dp;
        const double ccore = gcore[c0 + cur], cn = nrm[c0 + cur];
        double bw = 0.0, bs = 0.0;
        int32_t blo = 0, bhi = 0, bv = -1;
#pragma unroll 1
        for (int v = tid; v < nc; v += 256) {
            int32_t f = kf[v];
            if (f == -2) continue;
            const double *row = Xp + (c0 + v) * dp;
            double acc = 0.0;
            for (int i = 0; i < dp; i++) acc = val_fold<OP>(acc, crow[i], row[i]);
            double dist, s;
            val_finish<OP>(acc, cn, OP == OP_DOT ? nrm[c0 + v] : 0.0, dist, s);
            double w = dist;
            const double vc = gcore[c0 + v];
            if (ccore > w) w = ccore;
            if (vc > w) w = vc;
            if (w == w) {
                const int32_t lo = cur < v ? cur : v, hi = cur < v ? v : cur;
                if (f == -1 || val_key_less(w, s, lo, hi, kw[v], ks[v], f < v ? f : v, f < v ? v : f)) {
                    kw[v] = w;
                    ks[v] = s;
                    kf[v] = cur;
                    f = cur;
                }
            }
            if (f >= 0) {
                const int32_t lo = f < v ? f : v, hi = f < v ? v : f;
                if (bv < 0 || val_key_less(kw[v], ks[v], lo, hi, bw, bs, blo, bhi)) {
                    bw = kw[v];
                    bs = ks[v];
                    blo = lo;
                    bhi = hi;
                    bv = v;
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ow = __shfl_xor(bw, o), os = __shfl_xor(bs, o);
            const int32_t olo = __shfl_xor(blo, o), ohi = __shfl_xor(bhi, o), ov = __shfl_xor(bv, o);
            if (ov >= 0 && (bv < 0 || val_key_less(ow, os, olo, ohi, bw, bs, blo, bhi))) {
                bw = ow;
                bs = os;
                blo = olo;
                bhi = ohi;
                bv = ov;
            }
        }
        if (lane == 0) {
            rw[wave] = bw;
            rs[wave] = bs;
            rlo[wave] = blo;
            rhi[wave] = bhi;
            rv[wave] = bv;
        }
        __syncthreads();
        bv = -1;
#pragma unroll
        for (int k = 0; k < 4; k++) {  // every thread folds the four wave winners alike
            if (rv[k] >= 0 && (bv < 0 || val_key_less(rw[k], rs[k], rlo[k], rhi[k], bw, bs, blo, bhi))) {
                bw = rw[k];
                bs = rs[k];
                blo = rlo[k];
                bhi = rhi[k];
                bv = rv[k];
            }
        }
        if (bv < 0) {  // only NaN pairs leave the tree: uniform over the workgroup
            if (tid == 0) atomicMin(fail, (unsigned long long)c);
            return;
        }
        if (tid == 0) {
            ea[c0 + step] = blo;
            eb[c0 + step] = bhi;
            ew[c0 + step] = bw;
            kf[bv] = -2;
        }
        cur = bv;
        __syncthreads();
    }
}

// Step 4.  Edge slot e of cluster c (member positions c0 .. c0 + n_c - 2) holds a tree edge in
// local vertex numbers.
__global__ void val_deg_kernel(const int32_t *__restrict__ ea, const int32_t *__restrict__ eb,
                               const int32_t *__restrict__ glabel, const int64_t *__restrict__ coff, int64_t M,
                               int32_t *__restrict__ deg) {
    HDB_GRID_STRIDE(e, M) {
        const int32_t c = glabel[e];
        const int64_t c0 = coff[c], nc = coff[c + 1] - c0;
        if (e - c0 >= nc - 1) continue;
        atomicAdd(&deg[c0 + ea[e]], 1);  // both ends are in 0 .. n_c - 1: a tree of the cluster's own rows
        atomicAdd(&deg[c0 + eb[e]], 1);
    }
}
// per cluster: the count and the largest weight of the internal edges, the largest weight of all edges
__global__ void val_edge_kernel(const int32_t *__restrict__ ea, const int32_t *__restrict__ eb,
                                const double *__restrict__ ew, const int32_t *__restrict__ glabel,
                                const int64_t *__restrict__ coff, int64_t M, const int32_t *__restrict__ deg,
                                int32_t *__restrict__ nint, unsigned long long *__restrict__ int_u,
                                unsigned long long *__restrict__ all_u) {
    HDB_GRID_STRIDE(e, M) {
        const int32_t c = glabel[e];
        const int64_t c0 = coff[c], nc = coff[c + 1] - c0;
        if (e - c0 >= nc - 1) continue;
        const unsigned long long u = ukey(ew[e]);
        atomicMax(&all_u[c], u);
        if (deg[c0 + ea[e]] >= 2 && deg[c0 + eb[e]] >= 2) {
            atomicAdd(&nint[c], 1);
            atomicMax(&int_u[c], u);
        }
    }
}
// internal flags (every member of a cluster without an internal edge), the outputs in id order
__global__ void val_flag_kernel(const int32_t *__restrict__ glabel, const int32_t *__restrict__ gid,
                                const int32_t *__restrict__ deg, const int32_t *__restrict__ nint,
                                const double *__restrict__ gcore, int64_t M, int32_t *__restrict__ flag,
                                int32_t *__restrict__ internal_out, double *__restrict__ core_out) {
    HDB_GRID_STRIDE(q, M + 1) {
        if (q == M) {
            flag[q] = 0;  // the scan's total lands here
            continue;
        }
        const int32_t f = (nint[glabel[q]] == 0 || deg[q] >= 2) ? 1 : 0;
        flag[q] = f;
        if (internal_out) internal_out[gid[q]] = f;
        if (core_out) core_out[gid[q]] = gcore[q];
    }
}
// first internal position of every cluster: ioff[c], c = 1 .. K + 1 (the last one: the count)
__global__ void val_ioff_kernel(const int32_t *__restrict__ scan, const int64_t *__restrict__ coff, int32_t K,
                                int32_t *__restrict__ ioff) {
    HDB_GRID_STRIDE(i, (int64_t)K + 1) ioff[i + 1] = scan[coff[i + 1]];
}
__global__ void val_compact_kernel(const double *__restrict__ Xp, const double *__restrict__ nrm,
                                   const double *__restrict__ gcore, const int32_t *__restrict__ glabel,
                                   const int32_t *__restrict__ flag, const int32_t *__restrict__ scan, int64_t M, int dp,
                                   double *__restrict__ Xi, double *__restrict__ inrm, double *__restrict__ icore,
                                   int32_t *__restrict__ ilab) {
    HDB_GRID_STRIDE(q, M) {
        if (!flag[q]) continue;
        const int64_t ip = scan[q];
        const double *a = Xp + q * dp;
        double *o = Xi + ip * dp;
        for (int i = 0; i < dp; i++) o[i] = a[i];
        inrm[ip] = nrm[q];
        icore[ip] = gcore[q];
        ilab[ip] = glabel[q];
    }
}

// Step 5.  grid: (ceil(ntq / 4), splits); wave = up to 64 consecutive internal rows of one cluster;
// split y scans candidate tiles [y * tps, (y + 1) * tps) of all Mi internal rows and stores the
// lane's smallest (w, label) to slot y * Mi + q (label 0: no candidate in this split).
template <int OP>
__global__ __launch_bounds__(VAL_QT) void val_sep_kernel(const double *__restrict__ Xi, const double *__restrict__ inrm,
                                                         const double *__restrict__ icore,
                                                         const int32_t *__restrict__ ilab, int64_t Mi, int64_t nct,
                                                         int64_t tps, int dp, int64_t ntq,
                                                         const int32_t *__restrict__ qt_start,
                                                         const int32_t *__restrict__ qt_cl,
                                                         const int32_t *__restrict__ ioff, double *__restrict__ pw,
                                                         int32_t *__restrict__ pl) {
    const int64_t tile = (int64_t)blockIdx.x * (VAL_QT / 64) + (threadIdx.x >> 6);
    if (tile >= ntq) return;
    const int32_t c = qt_cl[tile];
    const int64_t i0 = ioff[c], i1 = ioff[c + 1];
    const int64_t q = (int64_t)qt_start[tile] + (threadIdx.x & 63);
    const bool inr = q < i1;
    const int64_t r = inr ? q : i1 - 1;
    const double *qrow = Xi + r * dp;
    const double qn = inrm[r], cq = icore[r];
    const int nch = dp / VAL_DC;
    double xq[VAL_DC];
#pragma unroll
    for (int i = 0; i < VAL_DC; i++) xq[i] = qrow[i];
    double bw = 0.0;
    int32_t bl = 0;
    const int64_t t0 = (int64_t)blockIdx.y * tps, t1 = min(t0 + tps, nct);
#pragma unroll 1
    for (int64_t t = t0; t < t1; t++) {
        const int64_t j0 = t * VAL_CT;
        const int rows = (int)min((int64_t)VAL_CT, Mi - j0);
        if (j0 >= i0 && j0 + rows <= i1) continue;  // wholly inside the wave's own cluster
#pragma unroll 1
        for (int jb = 0; jb < rows; jb += VAL_CB) {
            double acc[VAL_CB];
            val_batch<OP>(acc, xq, qrow, Xi + (j0 + jb) * dp, dp, nch);
#pragma unroll
            for (int u = 0; u < VAL_CB; u++) {
                const int64_t j = j0 + jb + u;
                if (j >= Mi) break;
                const int32_t l = ilab[j];
                if (l == c) continue;
                double dist, s;
                val_finish<OP>(acc[u], qn, OP == OP_DOT ? inrm[j] : 0.0, dist, s);
                double w = dist;
                const double cx = icore[j];
                if (cq > w) w = cq;
                if (cx > w) w = cx;
                if (w != w) continue;  // NaN: no candidate
                if (bl == 0 || w < bw || (w == bw && l < bl)) {
                    bw = w;
                    bl = l;
                }
            }
        }
    }
    if (inr) {
        const int64_t o = (int64_t)blockIdx.y * Mi + q;
        pw[o] = bw;
        pl[o] = bl;
    }
}
// merge of the splits' minima per query, and the cluster's smallest w
__global__ void val_sep_merge_kernel(const double *__restrict__ pw, const int32_t *__restrict__ pl, int64_t Mi,
                                     int splits, const int32_t *__restrict__ ilab, double *__restrict__ qw,
                                     int32_t *__restrict__ ql, unsigned long long *__restrict__ sep_u) {
    HDB_GRID_STRIDE(q, Mi) {
        double bw = 0.0;
        int32_t bl = 0;
        for (int sp = 0; sp < splits; sp++) {
            const int64_t o = (int64_t)sp * Mi + q;
            const int32_t l = pl[o];
            if (l == 0) continue;
            const double w = pw[o];
            if (bl == 0 || w < bw || (w == bw && l < bl)) {
                bw = w;
                bl = l;
            }
        }
        qw[q] = bw;
        ql[q] = bl;
        if (bl) atomicMin(&sep_u[ilab[q]], ukey(bw));
    }
}
// the smallest label among the queries that attain it
__global__ void val_sep_label_kernel(const double *__restrict__ qw, const int32_t *__restrict__ ql, int64_t Mi,
                                     const int32_t *__restrict__ ilab, const unsigned long long *__restrict__ sep_u,
                                     uint32_t *__restrict__ near) {
    HDB_GRID_STRIDE(q, Mi) {
        const int32_t l = ql[q], c = ilab[q];
        if (l && ukey(qw[q]) == sep_u[c]) atomicMin(&near[c], (uint32_t)l);
    }
}

struct ValGroup {  // stage 1: sized by n and K
    int32_t *cnt, *iota, *perm;
    unsigned long long *bad;
    uint32_t *keys, *keys2;
};
struct ValState {  // stage 2: sized by the member count M
    double *Xp, *Xc, *nrm, *gcore, *totals, *pp, *ew, *Xi, *inrm, *icore;
    int32_t *glabel, *gid, *qt_start, *qt_cl, *list, *ea, *eb, *deg, *flag, *scan, *nint, *ioff, *ilab, *qt2_start,
        *qt2_cl;
    int64_t *coff, *pbase;
    unsigned long long *int_u, *all_u, *fail;
};
struct ValSep {  // stage 3: sized by the internal count Mi and the split count
    double *pw, *qw;
    int32_t *pl, *ql;
    unsigned long long *sep_u;
    uint32_t *near;
};

template <class T>
void val_upload(hipStream_t st, T *dst, const std::vector<T> &src) {
    if (!src.empty()) HIP_CHECK(hipMemcpyAsync(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, st));
}
template <class T>
std::vector<T> val_download(hipStream_t st, const T *src, size_t count) {
    std::vector<T> v(count);
    if (count) HIP_CHECK(hipMemcpyAsync(v.data(), src, sizeof(T) * count, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return v;
}

// the wave tile table of clusters laid out at off[1 .. K + 1]: up to 64 consecutive rows of one
// cluster per entry; clusters below min_rows rows get none
void val_tiles(const std::vector<int64_t> &off, int32_t K, int64_t min_rows, std::vector<int32_t> &start,
               std::vector<int32_t> &cl) {
    start.clear();
    cl.clear();
    for (int32_t c = 1; c <= K; c++) {
        if (off[c + 1] - off[c] < min_rows) continue;
        for (int64_t q = off[c]; q < off[c + 1]; q += 64) {
            start.push_back((int32_t)q);
            cl.push_back(c);
        }
    }
}

#define HDB_VAL_BY_METRIC(CALL)                              \
    switch (metric) {                                        \
    case HDB_METRIC_EUCLIDEAN: CALL(OP_SQ); break;           \
    case HDB_METRIC_MANHATTAN: CALL(OP_ABS); break;          \
    case HDB_METRIC_SUPREMUM: CALL(OP_MAX); break;           \
    default: CALL(OP_DOT); break;                            \
    }

}  // namespace

void validity_stats_init(hdb_ctx *ctx) {
    ctx->stats["validity_last_splits"] = 0;
    ctx->stats["validity_last_core_splits"] = 0;
}

void validity_index_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const int32_t *labels, int32_t K,
                           int metric, int forced_splits, int32_t small_max, ValidityResult &res, double *core_out,
                           int32_t *internal_out) {
    if (small_max < 0 || small_max > VALIDITY_SMALL_LIMIT)
        HDB_THROW(HDB_EINVAL, "validity: small_max must be in 0.." + std::to_string(VALIDITY_SMALL_LIMIT));
    if (n >= (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "validity: n must be below 2^31 (int32 ids)");
    hipStream_t st = ctx->stream;
    const size_t nk = (size_t)K;
    res.index = 0.0;
    res.validity.assign(nk, 0.0);
    res.sparseness.assign(nk, 0.0);
    res.separation.assign(nk, INFINITY);
    res.nearest.assign(nk, 0);
    res.size.assign(nk, 0);
    ctx->stats["validity_last_splits"] = 0;
    ctx->stats["validity_last_core_splits"] = 0;
    if (n == 0) return;
    if (core_out) HIP_CHECK(hipMemsetAsync(core_out, 0, sizeof(double) * (size_t)n, st));
    if (internal_out) HIP_CHECK(hipMemsetAsync(internal_out, 0, sizeof(int32_t) * (size_t)n, st));

    // ---- 1. group
    const ValGroup g = carve(ctx, A_FLAT0, [&](Carver &cv) {
        ValGroup s;
        s.cnt = cv.take<int32_t>((int64_t)K + 1);
        s.bad = cv.take<unsigned long long>(2);
        s.keys = cv.take<uint32_t>(n);
        s.keys2 = cv.take<uint32_t>(n);
        s.iota = cv.take<int32_t>(n);
        s.perm = cv.take<int32_t>(n);
        return s;
    });
    HIP_CHECK(hipMemsetAsync(g.cnt, 0, sizeof(int32_t) * (nk + 1), st));
    HIP_CHECK(hipMemsetAsync(g.bad, 0xff, 16, st));
    hipLaunchKernelGGL(val_count_kernel, dim3(grid_for(n)), dim3(256), 0, st, labels, n, K, g.cnt, g.bad, g.keys, g.iota);
    HIP_CHECK(hipGetLastError());
    {
        const std::vector<unsigned long long> hb = val_download(st, (const unsigned long long *)g.bad, 1);
        if (hb[0] != ~0ull)
            HDB_THROW(HDB_EINVAL, "validity: label outside 0.." + std::to_string(K) + " (first: row " +
                                      std::to_string(hb[0]) + ")");
    }
    const std::vector<int32_t> cnt = val_download(st, (const int32_t *)g.cnt, nk + 1);
    std::vector<int64_t> off(nk + 2, 0);  // off[c]: first member position of cluster c; off[K + 1] = M
    for (int32_t c = 1; c <= K; c++) {
        res.size[c - 1] = cnt[c];
        off[c + 1] = off[c] + cnt[c];
    }
    const int64_t n0 = cnt[0], M = n - n0;
    if (M == 0 || K == 0) return;
    int B = 1;
    while (B < 31 && ((int64_t)1 << B) <= (int64_t)K) B++;
    sort_pairs(ctx, A_FLAT_TMP, g.keys, g.keys2, g.iota, g.perm, n, 0, B);  // stable: ascending id inside a label
    const int32_t *members = g.perm + n0;

    // ---- the plan of the core scan and of the trees, from the cluster sizes alone
    const int dp = (int)(ceil_div(d, VAL_DC) * VAL_DC);
    std::vector<int32_t> qt_start, qt_cl;
    val_tiles(off, K, 2, qt_start, qt_cl);
    const int64_t ntq = (int64_t)qt_start.size(), qblocks = ceil_div(ntq, (int64_t)(VAL_QT / 64));
    std::vector<int64_t> pbase(nk + 2, 0);
    int64_t pstore = 0, max_blocks = 1;
    for (int32_t c = 1; c <= K; c++) {
        const int64_t nc = off[c + 1] - off[c], nb = ceil_div(nc, (int64_t)VAL_SB);
        pbase[c] = pstore;
        if (nc >= 2) pstore += nc * nb;
        max_blocks = std::max(max_blocks, nb);
    }
    int64_t csplits = forced_splits;
    if (csplits <= 0) {  // enough workgroups to fill the device twice over, if the partial store stays small
        csplits = std::max<int64_t>(1, std::min<int64_t>(ceil_div(2 * (int64_t)ctx->num_cus, std::max<int64_t>(qblocks, 1)),
                                                         max_blocks));
        if (pstore > VAL_PARTIAL_MAX) csplits = 1;
    }
    csplits = std::min<int64_t>(csplits, 65535);
    std::vector<int32_t> small, large;
    int maxn = 2;
    for (int32_t c = 1; c <= K; c++) {
        const int64_t nc = off[c + 1] - off[c];
        if (nc < 2) continue;
        if (nc <= small_max) {
            small.push_back(c);
            maxn = std::max<int>(maxn, (int)nc);
        } else {
            large.push_back(c);
        }
    }

    const int64_t tq2_cap = M / 64 + (int64_t)K + 1;  // entries of the separation scan's tile table, at most
    const ValState s = carve(ctx, A_FLAT1, [&](Carver &cv) {
        ValState v;
        v.Xp = cv.take<double>((M + VAL_CT) * dp);
        v.Xc = cv.take<double>(M * d);
        v.nrm = cv.take<double>(M);
        v.gcore = cv.take<double>(M);
        v.totals = cv.take<double>(M);
        v.pp = cv.take<double>(csplits > 1 ? pstore : 1);
        v.ew = cv.take<double>(M);
        v.Xi = cv.take<double>((M + VAL_CT) * dp);
        v.inrm = cv.take<double>(M);
        v.icore = cv.take<double>(M);
        v.glabel = cv.take<int32_t>(M);
        v.gid = cv.take<int32_t>(M);
        v.qt_start = cv.take<int32_t>(ntq);
        v.qt_cl = cv.take<int32_t>(ntq);
        v.list = cv.take<int32_t>((int64_t)small.size());
        v.ea = cv.take<int32_t>(M);
        v.eb = cv.take<int32_t>(M);
        v.deg = cv.take<int32_t>(M);
        v.flag = cv.take<int32_t>(M + 1);
        v.scan = cv.take<int32_t>(M + 1);
        v.nint = cv.take<int32_t>((int64_t)K + 1);
        v.ioff = cv.take<int32_t>((int64_t)K + 2);
        v.ilab = cv.take<int32_t>(M);
        v.qt2_start = cv.take<int32_t>(tq2_cap);
        v.qt2_cl = cv.take<int32_t>(tq2_cap);
        v.coff = cv.take<int64_t>((int64_t)K + 2);
        v.pbase = cv.take<int64_t>((int64_t)K + 2);
        v.int_u = cv.take<unsigned long long>((int64_t)K + 1);
        v.all_u = cv.take<unsigned long long>((int64_t)K + 1);
        v.fail = cv.take<unsigned long long>(2);
        return v;
    });
    const int gM = grid_for(M);
    HIP_CHECK(hipMemsetAsync(s.Xp + (size_t)M * dp, 0, sizeof(double) * (size_t)VAL_CT * dp, st));
    HIP_CHECK(hipMemsetAsync(s.totals, 0, sizeof(double) * (size_t)M, st));
    HIP_CHECK(hipMemsetAsync(s.deg, 0, sizeof(int32_t) * (size_t)M, st));
    HIP_CHECK(hipMemsetAsync(s.ea, 0, sizeof(int32_t) * (size_t)M, st));  // an edge slot never holds a stale index
    HIP_CHECK(hipMemsetAsync(s.eb, 0, sizeof(int32_t) * (size_t)M, st));
    HIP_CHECK(hipMemsetAsync(s.nint, 0, sizeof(int32_t) * (nk + 1), st));
    HIP_CHECK(hipMemsetAsync(s.int_u, 0, 8 * (nk + 1), st));
    HIP_CHECK(hipMemsetAsync(s.all_u, 0, 8 * (nk + 1), st));
    HIP_CHECK(hipMemsetAsync(s.fail, 0xff, 16, st));
    val_upload(st, s.coff, off);
    val_upload(st, s.pbase, pbase);
    val_upload(st, s.qt_start, qt_start);
    val_upload(st, s.qt_cl, qt_cl);
    val_upload(st, s.list, small);
    hipLaunchKernelGGL(val_pack_kernel, dim3(gM), dim3(256), 0, st, X, d, dp, metric, members, M, labels, s.Xp, s.Xc, s.nrm,
                       s.glabel, s.gid, s.fail + 1);
    HIP_CHECK(hipGetLastError());

    // ---- 2. all-points core distances
    ctx->stats["validity_last_core_splits"] = csplits;
    if (ntq > 0) {
        KernelTimer t(ctx, "validity_core");
        const dim3 grid((unsigned)qblocks, (unsigned)csplits);
#define HDB_VAL_CORE(OP)                                                                                              \
    hipLaunchKernelGGL(val_core_kernel<OP>, grid, dim3(VAL_QT), 0, st, s.Xp, s.nrm, dp, d, ntq, s.qt_start, s.qt_cl, s.coff, \
                       s.pbase, (int)csplits, s.totals, s.pp)
        HDB_VAL_BY_METRIC(HDB_VAL_CORE)
#undef HDB_VAL_CORE
        if (csplits > 1)
            hipLaunchKernelGGL(val_core_merge_kernel, dim3(gM), dim3(256), 0, st, s.pp, s.glabel, s.coff, s.pbase, M,
                               s.totals);
        HIP_CHECK(hipGetLastError());
    }
    {
        std::vector<double> tot = val_download(st, (const double *)s.totals, (size_t)M);  // synchronises
        const std::vector<unsigned long long> hb = val_download(st, (const unsigned long long *)s.fail + 1, 1);
        if (hb[0] != ~0ull)
            HDB_THROW(HDB_EINVAL, "validity: non-finite input (first: row " + std::to_string(hb[0]) + ")");
        validity_cores_host(tot.data(), off.data(), K, d, tot.data());
        HIP_CHECK(hipMemcpyAsync(s.gcore, tot.data(), sizeof(double) * (size_t)M, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));  // tot dies with this block
    }

    // ---- 3. one tree per cluster, edges in local vertex numbers at the cluster's member positions
    if (!small.empty()) {
        KernelTimer t(ctx, "validity_mst_small");
        const size_t lds = (size_t)maxn * 20 + 16;
#define HDB_VAL_PRIM(OP)                                                                                           \
    hipLaunchKernelGGL(val_prim_small_kernel<OP>, dim3((unsigned)small.size()), dim3(256), lds, st, s.Xp, s.nrm, s.gcore, \
                       dp, maxn, s.list, s.coff, s.ea, s.eb, s.ew, s.fail)
        HDB_VAL_BY_METRIC(HDB_VAL_PRIM)
#undef HDB_VAL_PRIM
        HIP_CHECK(hipGetLastError());
        // a cluster it could not span has no edges to read: stop here
        const std::vector<unsigned long long> hf = val_download(st, (const unsigned long long *)s.fail, 1);
        if (hf[0] != ~0ull)
            HDB_THROW(HDB_EINVAL, "validity: cluster " + std::to_string(hf[0]) +
                                      ": non-finite input: only NaN distances join some of its rows");
    }
    for (int32_t c : large) {
        const int64_t c0 = off[c], nc = off[c + 1] - c0;
        try {
            boruvka_device(ctx, s.Xc + c0 * d, nc, d, s.gcore + c0, metric, s.ea + c0, s.eb + c0, s.ew + c0);
        } catch (const Error &e) {
            HDB_THROW(e.code, "validity: cluster " + std::to_string(c) + ": " + e.msg);
        }
    }

    // ---- 4. degrees, internal flags, sparseness
    hipLaunchKernelGGL(val_deg_kernel, dim3(gM), dim3(256), 0, st, s.ea, s.eb, s.glabel, s.coff, M, s.deg);
    hipLaunchKernelGGL(val_edge_kernel, dim3(gM), dim3(256), 0, st, s.ea, s.eb, s.ew, s.glabel, s.coff, M, s.deg, s.nint,
                       s.int_u, s.all_u);
    hipLaunchKernelGGL(val_flag_kernel, dim3(grid_for(M + 1)), dim3(256), 0, st, s.glabel, s.gid, s.deg, s.nint, s.gcore, M,
                       s.flag, internal_out, core_out);
    HIP_CHECK(hipGetLastError());
    exclusive_sum(ctx, A_FLAT_TMP, s.flag, s.scan, M + 1);
    hipLaunchKernelGGL(val_ioff_kernel, dim3(grid_for((int64_t)K + 1)), dim3(256), 0, st, s.scan, s.coff, K, s.ioff);
    HIP_CHECK(hipGetLastError());
    const std::vector<int32_t> hio = val_download(st, (const int32_t *)s.ioff, nk + 2);
    const std::vector<int32_t> hnint = val_download(st, (const int32_t *)s.nint, nk + 1);
    const std::vector<unsigned long long> hint = val_download(st, (const unsigned long long *)s.int_u, nk + 1);
    const std::vector<unsigned long long> hall = val_download(st, (const unsigned long long *)s.all_u, nk + 1);
    for (int32_t c = 1; c <= K; c++) {
        if (cnt[c] <= 1) continue;
        res.sparseness[c - 1] = unukey(hnint[c] == 0 ? hall[c] : hint[c]);
    }

    // ---- 5. separation over the internal rows
    std::vector<int64_t> ioff(nk + 2, 0);
    for (int32_t c = 1; c <= K + 1; c++) ioff[c] = hio[c];
    const int64_t Mi = ioff[K + 1];
    std::vector<int32_t> q2_start, q2_cl;
    val_tiles(ioff, K, 1, q2_start, q2_cl);
    const int64_t ntq2 = (int64_t)q2_start.size(), qblocks2 = ceil_div(ntq2, (int64_t)(VAL_QT / 64));
    const int64_t nct = ceil_div(Mi, (int64_t)VAL_CT);
    int64_t splits = forced_splits;
    if (splits <= 0)
        splits = std::max<int64_t>(1, std::min<int64_t>(ceil_div(2 * (int64_t)ctx->num_cus, std::max<int64_t>(qblocks2, 1)), nct));
    splits = std::min<int64_t>(splits, 65535);
    ctx->stats["validity_last_splits"] = splits;
    const ValSep p = carve(ctx, A_LOG, [&](Carver &cv) {
        ValSep v;
        v.pw = cv.take<double>(splits * Mi);
        v.qw = cv.take<double>(Mi);
        v.pl = cv.take<int32_t>(splits * Mi);
        v.ql = cv.take<int32_t>(Mi);
        v.sep_u = cv.take<unsigned long long>((int64_t)K + 1);
        v.near = cv.take<uint32_t>((int64_t)K + 1);
        return v;
    });
    HIP_CHECK(hipMemsetAsync(p.sep_u, 0xff, 8 * (nk + 1), st));
    HIP_CHECK(hipMemsetAsync(p.near, 0xff, 4 * (nk + 1), st));
    HIP_CHECK(hipMemsetAsync(s.Xi + (size_t)Mi * dp, 0, sizeof(double) * (size_t)VAL_CT * dp, st));
    val_upload(st, s.qt2_start, q2_start);
    val_upload(st, s.qt2_cl, q2_cl);
    hipLaunchKernelGGL(val_compact_kernel, dim3(gM), dim3(256), 0, st, s.Xp, s.nrm, s.gcore, s.glabel, s.flag, s.scan, M, dp,
                       s.Xi, s.inrm, s.icore, s.ilab);
    HIP_CHECK(hipGetLastError());
    if (ntq2 > 0) {
        KernelTimer t(ctx, "validity_sep");
        const dim3 grid((unsigned)qblocks2, (unsigned)splits);
        const int64_t tps = ceil_div(nct, splits);
        const int gi = grid_for(Mi);
#define HDB_VAL_SEP(OP)                                                                                               \
    hipLaunchKernelGGL(val_sep_kernel<OP>, grid, dim3(VAL_QT), 0, st, s.Xi, s.inrm, s.icore, s.ilab, Mi, nct, tps, dp, ntq2, \
                       s.qt2_start, s.qt2_cl, s.ioff, p.pw, p.pl)
        HDB_VAL_BY_METRIC(HDB_VAL_SEP)
#undef HDB_VAL_SEP
        hipLaunchKernelGGL(val_sep_merge_kernel, dim3(gi), dim3(256), 0, st, p.pw, p.pl, Mi, (int)splits, s.ilab, p.qw, p.ql,
                           p.sep_u);
        hipLaunchKernelGGL(val_sep_label_kernel, dim3(gi), dim3(256), 0, st, p.qw, p.ql, Mi, s.ilab, p.sep_u, p.near);
        HIP_CHECK(hipGetLastError());
    }

    // ---- 6. the per-cluster results and the index (validity.cpp)
    const std::vector<unsigned long long> hsep = val_download(st, (const unsigned long long *)p.sep_u, nk + 1);
    const std::vector<uint32_t> hnear = val_download(st, (const uint32_t *)p.near, nk + 1);  // the host vectors above are done
    for (int32_t c = 1; c <= K; c++) {
        if (hsep[c] == ~0ull) continue;
        res.separation[c - 1] = unukey(hsep[c]);
        res.nearest[c - 1] = (int32_t)hnear[c];
    }
    validity_finish_host(res, n);
}

}  // namespace hdb
