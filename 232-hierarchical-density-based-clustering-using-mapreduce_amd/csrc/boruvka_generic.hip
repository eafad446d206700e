// boruvka_generic.hip -- K2g: the exact mutual-reachability MST for any metric and any d.
//
// K2b (spatial.hip) walks a Morton/BVH index and exists for the Euclidean metric at
// d in {1, 2, 3, 4, 8, 16}.  K2g is the path for everything else: a Boruvka whose rounds find
// every point's nearest foreign neighbour with a tiled all-pairs FP64 scan, in the style of K1
// (knn_impl.hpp): a lane owns one query, candidate rows arrive wave-uniformly, no FMA.
//
// Edge order: the strict total order (w, s, lo, hi).
//   w   HDBSCANStar.java:162-168: the pair's distance, replaced by core_p, then core_q, on a
//       strict '>' only (a NaN core never raises a weight; a NaN distance stays NaN).
//   s   Euclidean: the squared distance summed in dimension order (K2b's key, so both paths
//       pick the same tree); every other metric: the distance as metric_distance computes it.
//   A pair whose w is NaN is no edge.  +inf weights are edges like any other: "no edge yet"
//   is a flag of its own (lo < 0), not a weight.
// Weights and tie keys may be negative (cosine and Pearson are 1 - x with x rounded): lanes
// compare doubles as numbers (key_less), and the per-component atomicMin runs on the
// order-preserving u64 image of a double (ukey: sign-flip map, -0.0 read as +0.0).
//
// Bit parity with metric_distance: each pair's sum runs over the dimensions in order, in
// chunks of GEN_DC with the running sum carried across chunks -- the same additions.  Rows are
// packed to a multiple of GEN_DC with zeros, which change no sum: t*t, |t| and a*b of a padded
// column are +0, and a sum that starts at +0 is never -0.  What depends on one row alone is
// hoisted into the per-round gather by the same operations: cosine's m1 / m2, Pearson's mean
// (divided by the true d), its centred coordinates a_i - mean and its s1 / s2.  Pearson's
// covariance is then the dot product of two centred rows, so cosine and Pearson share OP_DOT.
//
// Pruning, all exact:
//  (a) component skip: rows are kept grouped by component (stable radix sort by component of
//      the core-ascending order, then one O(n d) gather per round); a candidate tile of one
//      component is skipped by a wave whose 64 queries are all of that component.  Inside a
//      component the rows that must scan come first, the seeded rows of (c) after them.
//  (b) core bound: w(p, q) >= core_q for every edge (NaN cores count as -inf), so a tile whose
//      smallest core exceeds the best w of every live lane of the wave cannot hold a smaller
//      key.  Strict: a tile whose bound EQUALS a best w is evaluated, because ties go by s.
//  (c) seeding: a lane's best edge of the previous round, if its partner is still foreign, is
//      this round's best too (the minimum over a set that still contains it), so the lane
//      does not scan at all; a wave without a scanning lane skips every tile.
//
// Launch rules: plain launches only, no workgroup waits on another, every loop is bounded by n
// or the tile count, rounds are capped (GEN_MAX_ROUNDS), scratch comes from the context's
// arenas (O(n) words and one packed copy of X), indices are 64-bit.  Stream-ordered; the host
// reads the edge count one round behind, as K2b does, and synchronises for the non-finite error.
#include <algorithm>
#include <string>
#include <vector>

#include "internal.hpp"
#include "sort.hpp"

namespace hdb {

namespace {

constexpr int GEN_QT = 256;  // queries per workgroup: one per lane, four waves
constexpr int GEN_CT = 64;   // rows per candidate tile (and per wave of queries)
constexpr int GEN_DC = 8;    // dimension chunk held in registers
constexpr int GEN_CB = 4;    // candidates evaluated together (one query chunk load serves all)
constexpr int GEN_MAX_ROUNDS = 64;
constexpr int GEN_NSTAT = 5;  // per round: tiles evaluated, skipped by (a), (b), (c), pair evaluations
static_assert(GEN_QT % GEN_CT == 0 && GEN_CT == 64 && GEN_CT % GEN_CB == 0, "a wave of queries is one tile");

enum { OP_SQ = 0, OP_ABS = 1, OP_MAX = 2, OP_DOT = 3 };

struct GBest {
    double w, s;
    int32_t lo, hi;  // original ids; lo < 0: no edge yet
};
__device__ __forceinline__ bool gen_key_less(double w, double s, int32_t lo, int32_t hi, const GBest &b) {
    if (w < b.w) return true;
    if (w > b.w) return false;
    if (s < b.s) return true;
    if (s > b.s) return false;
    if (lo != b.lo) return lo < b.lo;
    return hi < b.hi;
}
// order-preserving image of a non-NaN double (-0.0 as +0.0); ~0 is above every image
__device__ __forceinline__ unsigned long long ukey(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x == 0.0 ? 0.0 : x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void gen_iota_kernel(int32_t *__restrict__ a, int32_t *__restrict__ b, int64_t n) {
    HDB_GRID_STRIDE(i, n) {
        a[i] = (int32_t)i;
        if (b) b[i] = (int32_t)i;
    }
}
__global__ void gen_corekey_kernel(const double *__restrict__ core, int64_t n, uint64_t *__restrict__ k) {
    HDB_GRID_STRIDE(i, n) k[i] = ukey(core[i]);  // NaN cores land at either end: any order is valid
}
// the round's row order: by component, and inside a component the rows that must scan before
// the rows whose previous best edge still stands (rule (c), the scan kernel's own test), so
// that the seeded rows fill whole waves and those waves skip the scan
__global__ void gen_compkey_kernel(const int32_t *__restrict__ comp, const int32_t *__restrict__ base, int64_t n,
                                   const int32_t *__restrict__ best_lo, const int32_t *__restrict__ best_hi,
                                   uint32_t *__restrict__ k) {
    HDB_GRID_STRIDE(i, n) {
        const int32_t id = base[i], c = comp[id], lo = best_lo[id];
        bool seeded = false;
        if (lo >= 0) {
            const int32_t partner = lo == id ? best_hi[id] : lo;
            seeded = comp[partner] != c;
        }
        k[i] = ((uint32_t)c << 1) | (seeded ? 1u : 0u);  // c < n < 2^31
    }
}

// One thread per position: the row of id order[pos], transformed for the metric and packed to
// dp columns; its core, component, id and per-row term.  Positions n .. npad-1 are zero rows
// that no lane reads as a candidate (every candidate index is checked against n).
__global__ void gen_gather_kernel(const double *__restrict__ X, int64_t n, int d, int dp, int metric,
                                  const int32_t *__restrict__ order, const double *__restrict__ core,
                                  const int32_t *__restrict__ comp, double *__restrict__ Xg,
                                  double *__restrict__ gcore, int32_t *__restrict__ gcomp, int32_t *__restrict__ gid,
                                  double *__restrict__ gnrm) {
    HDB_GRID_STRIDE(pos, n) {
        const int32_t id = order[pos];
        const double *a = X + (int64_t)id * d;
        double *o = Xg + pos * dp;
        double nrm = 0;
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
        for (int i = d; i < dp; i++) o[i] = 0.0;
        gcore[pos] = core[id];
        gcomp[pos] = comp[id];
        gid[pos] = id;
        gnrm[pos] = nrm;
    }
}

// per candidate tile: its component if all rows share one (else -1), and the lower bound of
// every weight into it: the smallest core, a NaN core counting as -inf
__global__ void gen_tile_kernel(const double *__restrict__ gcore, const int32_t *__restrict__ gcomp, int64_t n,
                                int64_t ntiles, int32_t *__restrict__ ttag, double *__restrict__ tmin) {
    HDB_GRID_STRIDE(t, ntiles) {
        const int64_t j0 = t * GEN_CT, j1 = min(j0 + (int64_t)GEN_CT, n);
        int32_t tag = gcomp[j0];
        double m = INFINITY;
        for (int64_t j = j0; j < j1; j++) {
            if (gcomp[j] != tag) tag = -1;
            const double c = gcore[j];
            const double lb = c == c ? c : -INFINITY;
            m = lb < m ? lb : m;
        }
        ttag[t] = tag;
        tmin[t] = m;
    }
}

template <int OP>
__device__ __forceinline__ double gen_fold(double acc, double a, double b) {
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

// K2g.  grid: ceil(n / GEN_QT) workgroups of 256; lane = one query position.  ONE: the packed
// row is a single chunk and stays in registers for the whole scan.
template <int OP, bool ONE>
__global__ __launch_bounds__(256) void gen_scan_kernel(
    const double *__restrict__ Xg, int dp, int64_t n, int64_t ntiles, const double *__restrict__ gcore,
    const int32_t *__restrict__ gcomp, const int32_t *__restrict__ gid, const double *__restrict__ gnrm,
    const int32_t *__restrict__ ttag, const double *__restrict__ tmin, const int32_t *__restrict__ comp, int seeded,
    double *__restrict__ best_w, double *__restrict__ best_s, int32_t *__restrict__ best_lo,
    int32_t *__restrict__ best_hi, unsigned long long *__restrict__ comp_w, unsigned long long *__restrict__ stats) {
    const int64_t pos = (int64_t)blockIdx.x * GEN_QT + threadIdx.x;
    const bool inr = pos < n;
    const int64_t r = inr ? pos : n - 1;
    const int32_t myid = gid[r], myc = gcomp[r];
    const double mycore = gcore[r], mynrm = gnrm[r];
    const double *qrow = Xg + r * dp;
    GBest b{0.0, 0.0, -1, -1};
    bool live = inr;
    if (inr && seeded) {
        b.lo = best_lo[myid];
        if (b.lo >= 0) {
            b.hi = best_hi[myid];
            const int32_t partner = b.lo == myid ? b.hi : b.lo;
            if (comp[partner] != myc) {  // (c): still the minimum over the foreign rows
                b.w = best_w[myid];
                b.s = best_s[myid];
                live = false;
            } else {
                b.lo = -1;
            }
        }
    }
    const int nch = dp / GEN_DC;
    const int64_t qtile = (int64_t)blockIdx.x * (GEN_QT / GEN_CT) + (threadIdx.x >> 6);  // wave-uniform
    const int32_t qtag = qtile < ntiles ? ttag[qtile] : -1;
    unsigned long long n_eval = 0, n_a = 0, n_b = 0, n_c = 0, n_pairs = 0;
    double xq[GEN_DC];
    if (ONE) {
#pragma unroll
        for (int i = 0; i < GEN_DC; i++) xq[i] = qrow[i];
    }
    if (!__any(live)) {
        n_c = (unsigned long long)ntiles;
    } else {
#pragma unroll 1
        for (int64_t t = 0; t < ntiles; t++) {
            const int32_t tag = ttag[t];
            if (tag >= 0 && tag == qtag) {  // (a)
                n_a++;
                continue;
            }
            const double tm = tmin[t];
            if (__all(!live || (b.lo >= 0 && b.w < tm))) {  // (b)
                n_b++;
                continue;
            }
            n_eval++;
            const int64_t j0 = t * GEN_CT;
            const int rows = (int)min((int64_t)GEN_CT, n - j0);
            n_pairs += (unsigned long long)rows * 64;
#pragma unroll 1
            for (int jb = 0; jb < rows; jb += GEN_CB) {
                double acc[GEN_CB];
#pragma unroll
                for (int u = 0; u < GEN_CB; u++) acc[u] = 0.0;
                // rows past n inside the last batch are the zero rows of the padded copy
                const double *cbase = Xg + (j0 + jb) * dp;
#pragma unroll 1
                for (int ch = 0; ch < nch; ch++) {
                    if (!ONE) {
#pragma unroll
                        for (int i = 0; i < GEN_DC; i++) xq[i] = qrow[ch * GEN_DC + i];
                    }
#pragma unroll
                    for (int u = 0; u < GEN_CB; u++) {
                        const double *cr = cbase + (int64_t)u * dp + ch * GEN_DC;
#pragma unroll
                        for (int i = 0; i < GEN_DC; i++) acc[u] = gen_fold<OP>(acc[u], xq[i], cr[i]);
                    }
                }
#pragma unroll
                for (int u = 0; u < GEN_CB; u++) {
                    const int64_t j = j0 + jb + u;
                    if (j >= n) break;
                    if (!live || gcomp[j] == myc) continue;
                    double dist, s;
                    if (OP == OP_SQ) {
                        s = acc[u];
                        dist = sqrt(s);
                    } else if (OP == OP_DOT) {
                        dist = 1 - (acc[u] / sqrt(mynrm * gnrm[j]));
                        s = dist;
                    } else {
                        dist = acc[u];
                        s = dist;
                    }
                    double w = dist;
                    const double cq = gcore[j];
                    if (mycore > w) w = mycore;
                    if (cq > w) w = cq;
                    if (w != w) continue;  // NaN: not an edge
                    const int32_t qid = gid[j];
                    const int32_t lo = myid < qid ? myid : qid, hi = myid < qid ? qid : myid;
                    if (b.lo < 0 || gen_key_less(w, s, lo, hi, b)) b = GBest{w, s, lo, hi};
                }
            }
        }
    }
    if (inr) {
        best_lo[myid] = b.lo;
        if (b.lo >= 0) {
            best_hi[myid] = b.hi;
            best_w[myid] = b.w;
            best_s[myid] = b.s;
            atomicMin(&comp_w[myc], ukey(b.w));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_eval) atomicAdd(&stats[0], n_eval);
        if (n_a) atomicAdd(&stats[1], n_a);
        if (n_b) atomicAdd(&stats[2], n_b);
        if (n_c) atomicAdd(&stats[3], n_c);
        if (n_pairs) atomicAdd(&stats[4], n_pairs);
    }
}

// component minimum in three steps: comp_w = min w (the scan), min s among the points at that
// w, min (lo, hi) among the points at (w, s); all through ukey, so negative values order
__global__ void gen_comp_s_kernel(const int32_t *__restrict__ comp, int64_t n,
                                  const unsigned long long *__restrict__ comp_w, const double *__restrict__ best_w,
                                  const double *__restrict__ best_s, const int32_t *__restrict__ best_lo,
                                  unsigned long long *__restrict__ comp_s) {
    HDB_GRID_STRIDE(i, n) {
        if (best_lo[i] < 0) continue;
        const int32_t c = comp[i];
        if (ukey(best_w[i]) == comp_w[c]) atomicMin(&comp_s[c], ukey(best_s[i]));
    }
}
__global__ void gen_comp_key_kernel(const int32_t *__restrict__ comp, int64_t n,
                                    const unsigned long long *__restrict__ comp_w,
                                    const unsigned long long *__restrict__ comp_s, const double *__restrict__ best_w,
                                    const double *__restrict__ best_s, const int32_t *__restrict__ best_lo,
                                    const int32_t *__restrict__ best_hi, unsigned long long *__restrict__ comp_key) {
    HDB_GRID_STRIDE(i, n) {
        if (best_lo[i] < 0) continue;
        const int32_t c = comp[i];
        if (ukey(best_w[i]) == comp_w[c] && ukey(best_s[i]) == comp_s[c])
            atomicMin(&comp_key[c], ((unsigned long long)(uint32_t)best_lo[i] << 32) | (uint32_t)best_hi[i]);
    }
}
// the point that holds its component's chosen edge records the weight as computed; the root
// hooks onto the component at the edge's other end
__global__ void gen_hook_kernel(const int32_t *__restrict__ comp, int64_t n,
                                const unsigned long long *__restrict__ comp_w,
                                const unsigned long long *__restrict__ comp_s,
                                const unsigned long long *__restrict__ comp_key, const double *__restrict__ best_w,
                                const double *__restrict__ best_s, const int32_t *__restrict__ best_lo,
                                const int32_t *__restrict__ best_hi, int32_t *__restrict__ parent,
                                double *__restrict__ win_w) {
    HDB_GRID_STRIDE(i, n) {
        const int32_t c = comp[i];
        const unsigned long long k = comp_key[c];
        if (best_lo[i] >= 0 && ukey(best_w[i]) == comp_w[c] && ukey(best_s[i]) == comp_s[c] &&
            (((unsigned long long)(uint32_t)best_lo[i] << 32) | (uint32_t)best_hi[i]) == k)
            win_w[c] = best_w[i];
        if (c != (int32_t)i) continue;  // not a root
        if (k == ~0ull) {
            parent[i] = (int32_t)i;
            continue;
        }
        const int32_t lo = (int32_t)(k >> 32), hi = (int32_t)(k & 0xffffffffu);
        const int32_t cl = comp[lo], chh = comp[hi];
        parent[i] = cl == c ? chh : cl;
    }
}
// Mutual pairs (two components that chose the same edge: under a strict total order the only
// cycle) keep the smaller id as root and emit the edge once.  One atomic per wave reserves
// the edge slots.
__global__ __launch_bounds__(256) void gen_hook_fix_kernel(const int32_t *__restrict__ comp, int64_t n,
                                                           const unsigned long long *__restrict__ comp_key,
                                                           const double *__restrict__ win_w,
                                                           const int32_t *__restrict__ parent,
                                                           int32_t *__restrict__ parent2, int32_t *__restrict__ out_a,
                                                           int32_t *__restrict__ out_b, double *__restrict__ out_w,
                                                           unsigned long long *__restrict__ n_edges) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool emit = false;
    if (c < n) {
        if (comp[c] != (int32_t)c) {
            parent2[c] = -1;  // not a root: resolve skips it
        } else {
            const int32_t p = parent[c];
            if (p == (int32_t)c) {
                parent2[c] = p;
            } else {
                const bool mutual = parent[p] == (int32_t)c;
                parent2[c] = (mutual && (int32_t)c < p) ? (int32_t)c : p;
                emit = !(mutual && (int32_t)c > p);
            }
        }
    }
    const unsigned long long m = __ballot(emit);
    if (m == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(n_edges, (unsigned long long)__popcll(m));
    base = ((unsigned long long)(unsigned)__shfl((int)(base >> 32), 0) << 32) | (unsigned)__shfl((int)base, 0);
    if (emit) {
        const unsigned long long sl = base + __popcll(m & ((1ull << lane) - 1));
        if (sl < (unsigned long long)(n - 1)) {  // a forest has at most n - 1 edges
            const unsigned long long k = comp_key[c];
            out_a[sl] = (int32_t)(k >> 32);
            out_b[sl] = (int32_t)(k & 0xffffffffu);
            out_w[sl] = win_w[c];
        }
    }
}
// hook trees -> roots (chains only shorten while other lanes write; at most n steps)
__global__ void gen_resolve_kernel(int32_t *__restrict__ parent, int64_t n) {
    HDB_GRID_STRIDE(c, n) {
        int32_t p = parent[c];
        if (p < 0) continue;
        for (int64_t step = 0; step < n; step++) {
            const int32_t pp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (pp == p) break;
            p = pp;
        }
        parent[c] = p;
    }
}
__global__ void gen_relabel_kernel(int32_t *__restrict__ comp, const int32_t *__restrict__ root, int64_t n) {
    HDB_GRID_STRIDE(i, n) comp[i] = root[comp[i]];
}

// the output order (w, lo, hi): a stable sort by (lo, hi), then a stable sort by ukey(w)
__global__ void gen_idkey_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ b, int64_t m,
                                 uint64_t *__restrict__ k, int32_t *__restrict__ io) {
    HDB_GRID_STRIDE(i, m) {
        k[i] = ((uint64_t)(uint32_t)a[i] << 32) | (uint32_t)b[i];
        io[i] = (int32_t)i;
    }
}
__global__ void gen_wkey_kernel(const int32_t *__restrict__ perm, const double *__restrict__ w, int64_t m,
                                uint64_t *__restrict__ k) {
    HDB_GRID_STRIDE(i, m) k[i] = ukey(w[perm[i]]);
}
__global__ void gen_out_kernel(const int32_t *__restrict__ perm, const int32_t *__restrict__ a,
                               const int32_t *__restrict__ b, const double *__restrict__ w, int64_t m,
                               int32_t *__restrict__ oa, int32_t *__restrict__ ob, double *__restrict__ ow) {
    HDB_GRID_STRIDE(i, m) {
        const int32_t p = perm[i];
        oa[i] = a[p];
        ob[i] = b[p];
        ow[i] = w[p];
    }
}

struct GenState {
    double *Xg, *gcore, *gnrm, *tmin, *best_w, *best_s, *win_w, *ew;
    int32_t *gcomp, *gid, *ttag, *comp, *base_order, *order, *best_lo, *best_hi, *parent, *parent2, *ea, *eb, *p1, *p2;
    unsigned long long *comp3, *n_edges, *stats;
    uint64_t *k1, *k2;
    uint32_t *ck1, *ck2;
};
GenState gen_carve(Carver &cv, int64_t n, int64_t npad, int dp, int64_t ntiles) {
    const size_t per = (size_t)n;
    GenState s;
    s.Xg = cv.take<double>((size_t)npad * dp);
    s.gcore = cv.take<double>(per);
    s.gnrm = cv.take<double>(per);
    s.tmin = cv.take<double>((size_t)ntiles);
    s.best_w = cv.take<double>(per);
    s.best_s = cv.take<double>(per);
    s.win_w = cv.take<double>(per);
    s.ew = cv.take<double>(per);
    s.gcomp = cv.take<int32_t>(per);
    s.gid = cv.take<int32_t>(per);
    s.ttag = cv.take<int32_t>((size_t)ntiles);
    s.comp = cv.take<int32_t>(per);
    s.base_order = cv.take<int32_t>(per);
    s.order = cv.take<int32_t>(per);
    s.best_lo = cv.take<int32_t>(per);
    s.best_hi = cv.take<int32_t>(per);
    s.parent = cv.take<int32_t>(per);
    s.parent2 = cv.take<int32_t>(per);
    s.ea = cv.take<int32_t>(per);
    s.eb = cv.take<int32_t>(per);
    s.p1 = cv.take<int32_t>(per);
    s.p2 = cv.take<int32_t>(per);
    s.comp3 = cv.take<unsigned long long>(3 * per);
    s.n_edges = cv.take<unsigned long long>(1);
    s.stats = cv.take<unsigned long long>((size_t)GEN_NSTAT * GEN_MAX_ROUNDS);
    s.k1 = cv.take<uint64_t>(per);
    s.k2 = cv.take<uint64_t>(per);
    s.ck1 = cv.take<uint32_t>(per);
    s.ck2 = cv.take<uint32_t>(per);
    return s;
}

template <int OP>
void gen_scan_launch(bool one, unsigned grid, hipStream_t st, const GenState &s, int dp, int64_t n, int64_t ntiles,
                     int seeded, unsigned long long *comp_w, unsigned long long *stats) {
    if (one)
        hipLaunchKernelGGL((gen_scan_kernel<OP, true>), dim3(grid), dim3(GEN_QT), 0, st, s.Xg, dp, n, ntiles, s.gcore,
                           s.gcomp, s.gid, s.gnrm, s.ttag, s.tmin, s.comp, seeded, s.best_w, s.best_s, s.best_lo,
                           s.best_hi, comp_w, stats);
    else
        hipLaunchKernelGGL((gen_scan_kernel<OP, false>), dim3(grid), dim3(GEN_QT), 0, st, s.Xg, dp, n, ntiles, s.gcore,
                           s.gcomp, s.gid, s.gnrm, s.ttag, s.tmin, s.comp, seeded, s.best_w, s.best_s, s.best_lo,
                           s.best_hi, comp_w, stats);
}

}  // namespace

void boruvka_generic_stats_init(hdb_ctx *ctx) {
    ctx->stats["boruvka_gen_qt"] = GEN_QT;
    ctx->stats["boruvka_gen_ct"] = GEN_CT;
    ctx->stats["boruvka_gen_dc"] = GEN_DC;
    ctx->stats["boruvka_gen_rounds"] = 0;
}

void boruvka_generic_device(hdb_ctx *ctx, const double *X, int64_t n, int d, const double *core, int metric,
                            int32_t *va, int32_t *vb, double *w) {
    if (n <= 1) return;
    if (n >= (int64_t)INT32_MAX) HDB_THROW(HDB_EINVAL, "boruvka: n must be below 2^31 (int32 ids)");
    KernelTimer tt(ctx, "boruvka_gen_total");
    hipStream_t st = ctx->stream;
    const int dp = (int)(ceil_div(d, GEN_DC) * GEN_DC);
    const int64_t ntiles = ceil_div(n, (int64_t)GEN_CT), npad = ntiles * GEN_CT;
    const GenState s = carve(ctx, A_WORK0, [&](Carver &cv) { return gen_carve(cv, n, npad, dp, ntiles); });
    const size_t per = (size_t)n;
    unsigned long long *comp_w = s.comp3, *comp_s = s.comp3 + per, *comp_key = s.comp3 + 2 * per;
    int B = 1;  // bits of a component id (the sort key carries one more: the seeded flag)
    while (B < 31 && ((int64_t)1 << B) < n) B++;
    // one radix scratch sized for the three sorts up front: the arena synchronises the stream when it
    // grows, which the round loop (one round in flight) must not do
    arena(ctx, A_SORT, std::max({sort_pairs_bytes<uint64_t, int32_t>(n, 0, 64), sort_pairs_bytes<uint32_t, int32_t>(n, 0, B + 1),
                                 sort_pairs_bytes<uint64_t, int32_t>(n - 1, 0, 64)}));

    const int g = (int)std::min<int64_t>(ceil_div(n, 256), 4096);
    const int gt = (int)std::min<int64_t>(ceil_div(ntiles, 256), 4096);
    HIP_CHECK(hipMemsetAsync(s.n_edges, 0, 8, st));
    HIP_CHECK(hipMemsetAsync(s.stats, 0, 8 * (size_t)GEN_NSTAT * GEN_MAX_ROUNDS, st));
    if (npad > n) HIP_CHECK(hipMemsetAsync(s.Xg + (size_t)n * dp, 0, sizeof(double) * (size_t)(npad - n) * dp, st));
    // every point its own component; the base order: ids by ascending core distance
    hipLaunchKernelGGL(gen_iota_kernel, dim3(g), dim3(256), 0, st, s.comp, s.p1, n);
    hipLaunchKernelGGL(gen_corekey_kernel, dim3(g), dim3(256), 0, st, core, n, s.k1);
    sort_pairs(ctx, A_SORT, s.k1, s.k2, s.p1, s.base_order, n, 0, 64);
    HIP_CHECK(hipGetLastError());

    int64_t *hcnt = pinned_words(ctx);
    std::vector<hipEvent_t> round_ev;
    auto release_events = [&]() {
        for (auto e : round_ev) (void)hipEventDestroy(e);
        round_ev.clear();
    };
    const bool one = dp == GEN_DC;
    const unsigned scan_grid = (unsigned)ceil_div(n, (int64_t)GEN_QT);
    int stalled_round = -1, rounds = 0;
    for (int round = 0;; round++) {
        if (round >= GEN_MAX_ROUNDS || round >= PINNED_WORDS) {
            release_events();
            HDB_THROW(HDB_EINVAL, "boruvka did not converge (internal error)");
        }
        rounds = round + 1;
        // rows grouped by component, ascending core inside a component (round 0: every point
        // is a component, the core order itself)
        const int32_t *order = s.base_order;
        if (round > 0) {
            hipLaunchKernelGGL(gen_compkey_kernel, dim3(g), dim3(256), 0, st, s.comp, s.base_order, n, s.best_lo,
                               s.best_hi, s.ck1);
            sort_pairs(ctx, A_SORT, s.ck1, s.ck2, s.base_order, s.order, n, 0, B + 1);
            order = s.order;
        }
        hipLaunchKernelGGL(gen_gather_kernel, dim3(g), dim3(256), 0, st, X, n, d, dp, metric, order, core, s.comp, s.Xg,
                           s.gcore, s.gcomp, s.gid, s.gnrm);
        hipLaunchKernelGGL(gen_tile_kernel, dim3(gt), dim3(256), 0, st, s.gcore, s.gcomp, n, ntiles, s.ttag, s.tmin);
        HIP_CHECK(hipMemsetAsync(s.comp3, 0xff, 8 * 3 * per, st));
        {
            KernelTimer ts(ctx, "boruvka_gen_scan");
            unsigned long long *rs = s.stats + (size_t)GEN_NSTAT * round;
            switch (metric) {
            case HDB_METRIC_EUCLIDEAN: gen_scan_launch<OP_SQ>(one, scan_grid, st, s, dp, n, ntiles, round > 0, comp_w, rs); break;
            case HDB_METRIC_MANHATTAN: gen_scan_launch<OP_ABS>(one, scan_grid, st, s, dp, n, ntiles, round > 0, comp_w, rs); break;
            case HDB_METRIC_SUPREMUM: gen_scan_launch<OP_MAX>(one, scan_grid, st, s, dp, n, ntiles, round > 0, comp_w, rs); break;
            default: gen_scan_launch<OP_DOT>(one, scan_grid, st, s, dp, n, ntiles, round > 0, comp_w, rs); break;
            }
        }
        hipLaunchKernelGGL(gen_comp_s_kernel, dim3(g), dim3(256), 0, st, s.comp, n, comp_w, s.best_w, s.best_s, s.best_lo,
                           comp_s);
        hipLaunchKernelGGL(gen_comp_key_kernel, dim3(g), dim3(256), 0, st, s.comp, n, comp_w, comp_s, s.best_w, s.best_s,
                           s.best_lo, s.best_hi, comp_key);
        hipLaunchKernelGGL(gen_hook_kernel, dim3(g), dim3(256), 0, st, s.comp, n, comp_w, comp_s, comp_key, s.best_w,
                           s.best_s, s.best_lo, s.best_hi, s.parent, s.win_w);
        hipLaunchKernelGGL(gen_hook_fix_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, s.comp, n, comp_key,
                           s.win_w, s.parent, s.parent2, s.ea, s.eb, s.ew, s.n_edges);
        hipLaunchKernelGGL(gen_resolve_kernel, dim3(g), dim3(256), 0, st, s.parent2, n);
        hipLaunchKernelGGL(gen_relabel_kernel, dim3(g), dim3(256), 0, st, s.comp, s.parent2, n);
        HIP_CHECK(hipMemcpyAsync(hcnt + round, s.n_edges, 8, hipMemcpyDeviceToHost, st));
        hipEvent_t ev;
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        round_ev.push_back(ev);
        HIP_CHECK(hipEventRecord(ev, st));
        HIP_CHECK(hipGetLastError());
        if (round == 0) continue;  // keep one round in flight
        HIP_CHECK(hipEventSynchronize(round_ev[round - 1]));
        const int64_t c = hcnt[round - 1];
        if (c >= n - 1) break;  // the tree was complete: round `round` was a no-op
        if (round >= 2 && c == hcnt[round - 2]) {  // only NaN pairs are left between two trees
            stalled_round = round;
            break;
        }
    }
    release_events();
    ctx->stats["boruvka_gen_rounds"] = rounds;
    if (ctx->count_evals) {  // diagnostic: what each pruning rule skipped, per round (one sync)
        std::vector<unsigned long long> h((size_t)GEN_NSTAT * rounds);
        HIP_CHECK(hipMemcpyAsync(h.data(), s.stats, 8 * h.size(), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        static const char *names[GEN_NSTAT] = {"tiles_eval", "tiles_skip_comp", "tiles_skip_core", "tiles_skip_seed",
                                               "pair_evals"};
        int64_t pairs = 0;
        for (int r = 0; r < rounds; r++)
            for (int k = 0; k < GEN_NSTAT; k++) {
                ctx->stats["boruvka_gen_r" + std::to_string(r) + "_" + names[k]] = (int64_t)h[(size_t)r * GEN_NSTAT + k];
                if (k == 4) pairs += (int64_t)h[(size_t)r * GEN_NSTAT + k];
            }
        ctx->stats["boruvka_gen_pair_evals"] = pairs;
    }
    if (stalled_round >= 0) {
        // what is left are trees that only NaN pairs join: the rows outside the largest tree
        // (the smallest root id among equals) are the error's rows
        std::vector<int32_t> hc(per);
        HIP_CHECK(hipMemcpyAsync(hc.data(), s.comp, 4 * per, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<int32_t> size(per, 0);
        for (int64_t i = 0; i < n; i++) size[hc[i]]++;
        int32_t big = hc[0];
        for (int64_t i = 0; i < n; i++)
            if (size[hc[i]] > size[big] || (size[hc[i]] == size[big] && hc[i] < big)) big = hc[i];
        int64_t left = 0;
        int32_t first = -1;
        for (int64_t i = 0; i < n; i++)
            if (hc[i] != big) {
                if (first < 0) first = (int32_t)i;
                left++;
            }
        HDB_THROW(HDB_EINVAL, "boruvka: non-finite input: " + std::to_string(left) +
                                  " row(s) have only NaN distances to the other rows (first: row " +
                                  std::to_string(first) + ")");
    }
    const int64_t ne = n - 1;
    hipLaunchKernelGGL(gen_idkey_kernel, dim3(g), dim3(256), 0, st, s.ea, s.eb, ne, s.k1, s.p1);
    sort_pairs(ctx, A_SORT, s.k1, s.k2, s.p1, s.p2, ne, 0, 64);
    hipLaunchKernelGGL(gen_wkey_kernel, dim3(g), dim3(256), 0, st, s.p2, s.ew, ne, s.k1);
    sort_pairs(ctx, A_SORT, s.k1, s.k2, s.p2, s.p1, ne, 0, 64);
    hipLaunchKernelGGL(gen_out_kernel, dim3(g), dim3(256), 0, st, s.p1, s.ea, s.eb, s.ew, ne, va, vb, w);
    HIP_CHECK(hipGetLastError());
}

}  // namespace hdb
