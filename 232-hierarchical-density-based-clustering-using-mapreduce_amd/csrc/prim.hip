// prim.hip -- K2: dense Prim on the mutual-reachability graph with the reference's exact
// tie rules (HDBSCANStar.constructMST, HDBSCANStar.java:124-205; the bubble variant
// HdbscanDataBubbles.constructMSTBubbles, HdbscanDataBubbles.java:165-254):
//   * start at vertex n-1, best[] = Double.MAX_VALUE, parent[] = 0 (Java default);
//   * update iff mrd < best[nb] (strict), parent = ids[cur];
//   * select the unattached vertex with the smallest best, ties -> LARGEST index ('<=').
// mrd = max(dist, core[cur], core[nb]) evaluated with Java's two '>' tests.
//
// Three launch shapes:
//   prim_block_kernel   one workgroup per partition (n <= BS*PPT), whole Prim in-kernel,
//                       per-step argmin = DPP/shuffle wave reduce + one LDS exchange;
//   leaf_core_kernel    FirstStep leaf branch: cumulative core distances per partition;
//   prim_step_kernel    large graphs: one launch per Prim step over many workgroups; each
//                       workgroup re-reduces the previous step's per-workgroup partials
//                       (visible across the kernel boundary), so no inter-workgroup
//                       hand-off is needed inside a launch.  Launches are replayed from a
//                       captured hipGraph chunk.
// Euclidean pairs use a squared filter: s > fl(b*b)*(1+2^-50) proves sqrt(s) >= b, so
// the exact sqrt + mrd path runs only for pairs that can improve best[nb].
#include <atomic>

#include "internal.hpp"

// Between the block kernel and the stepwise one, a partition of 4096 < n <= 65536 vertices runs
// as one launch over co-resident workgroups: prim_coop4_kernel (rows of d <= 16 in registers,
// tagged-granule exchange; prim_coop_slots 4, the default) and prim_coop_kernel (any d, counter
// barrier), which is also what prim_coop4 falls back to when it declines.

namespace hdb {

// exact mrd for (cur, nb); returns true if it improves best
__device__ __forceinline__ bool mrd_improves(const PrimIn &in, int64_t cur, int64_t nb, double best, double &mrd_out) {
    const double *a = in.X + cur * in.d;
    const double *b = in.X + nb * in.d;
    double dist;
    if (in.metric == HDB_METRIC_EUCLIDEAN && !in.eB) {
        double s = sq_diff(a[0], b[0]);
        for (int c = 1; c < in.d; c++) s = s + sq_diff(a[c], b[c]);
        double thr = (best * best) * 1.0000000000000009;  // >= best^2 exactly
        if (s > thr) return false;
        dist = sqrt(s);
    } else {
        dist = metric_distance(a, b, in.d, in.metric);
        if (in.eB) dist = distance_bubbles(dist, in.eB[cur], in.eB[nb], in.nnB[cur], in.nnB[nb]);
    }
    double mrd = dist;
    double cc = in.core[cur], cn = in.core[nb];
    if (cc > mrd) mrd = cc;
    if (cn > mrd) mrd = cn;
    mrd_out = mrd;
    return mrd < best;
}

__device__ __forceinline__ void wave_argmin_last(double &v, int &i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        double v2 = __shfl_xor(v, off);
        int i2 = __shfl_xor(i, off);
        argmin_last(v, i, v2, i2);
    }
}


// Order-preserving u64 key of any non-NaN MRD value: the sign bit set for v >= 0, every bit
// complemented for v < 0 (cosine and Pearson weights can lie a few ulps below zero), +-0 one key.
// min over keys = min value.  best starts at Double.MAX_VALUE and a NaN never replaces it, so no
// NaN is keyed.
// Integer form (every wave keys its lanes on the step's critical path): v + 0.0 turns -0.0 into
// +0.0 and changes no other value, then the bits are flipped by the sign spread over the word,
// with the sign bit always in it.
constexpr unsigned long long MRD_KEY_SIGN = 0x8000000000000000ull;
__device__ __forceinline__ unsigned long long mrd_key(double v) {
    const long long b = __double_as_longlong(v + 0.0);
    return (unsigned long long)b ^ ((unsigned long long)(b >> 63) | MRD_KEY_SIGN);
}

// highest lane whose predicate holds (-1: none)
__device__ __forceinline__ int last_lane(bool p) {
    const unsigned long long m = __ballot(p);
    return m ? 63 - __clzll(m) : -1;
}

// ---------------------------------------------------------- block kernel
// parts: partition list for this launch (indices into offsets); vertex rows of partition
// p are [offsets[p], offsets[p+1]).  Edges at eoff[p].
template <int BS, int PPT>
__global__ __launch_bounds__(BS) void prim_block_kernel(PrimIn in, const int64_t *__restrict__ offsets,
                                                        const int64_t *__restrict__ eoff,
                                                        const int32_t *__restrict__ parts, int self_edges,
                                                        int32_t *__restrict__ va, int32_t *__restrict__ vb,
                                                        double *__restrict__ w) {
    constexpr int NW = BS / 64;
    __shared__ double s_v[2][NW];
    __shared__ int s_i[2][NW];
    const int p = parts[blockIdx.x];
    const int64_t o = offsets[p];
    const int n = (int)(offsets[p + 1] - o);
    if (n <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    PrimIn L = in;
    L.X = in.X + o * in.d;
    L.core = in.core + o;
    L.ids = in.ids + o;
    if (in.eB) {
        L.eB = in.eB + o;
        L.nnB = in.nnB + o;
    }
    double best[PPT];
    int par[PPT];
    unsigned att = 0;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        best[k] = JMAX;
        par[k] = 0;
        int i = tid + k * BS;
        if (i == n - 1 || i >= n) att |= 1u << k;
    }
    int cur = n - 1;
    for (int step = 1; step < n; step++) {
        double lv = INFINITY;
        int li = -1;
        const int cid = L.ids[cur];
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            if (att & (1u << k)) continue;
            int i = tid + k * BS;
            double mrd;
            if (mrd_improves(L, cur, i, best[k], mrd)) {
                best[k] = mrd;
                par[k] = cid;
            }
            argmin_last(lv, li, best[k], i);
        }
        wave_argmin_last(lv, li);
        if (NW > 1) {
            const int buf = step & 1;
            if (lane == 0) {
                s_v[buf][wid] = lv;
                s_i[buf][wid] = li;
            }
            __syncthreads();
            lv = s_v[buf][0];
            li = s_i[buf][0];
#pragma unroll
            for (int q = 1; q < NW; q++) argmin_last(lv, li, s_v[buf][q], s_i[buf][q]);
        }
        cur = li;  // uniform
        if (cur < 0) break;  // unreachable: an unattached vertex always exists
        if ((cur % BS) == tid) att |= 1u << (cur / BS);
    }
    const int64_t eo = eoff[p];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        int i = tid + k * BS;
        if (i < n - 1) {
            va[eo + i] = par[k];
            vb[eo + i] = L.ids[i];
            w[eo + i] = best[k];
        }
        if (self_edges && i < n) {
            va[eo + n - 1 + i] = L.ids[i];
            vb[eo + n - 1 + i] = L.ids[i];
            w[eo + n - 1 + i] = L.core[i];
        }
    }
}

// ------------------------------------------------- leaf cumulative cores
// HDBSCANStar.calculateCoreDistances inside a leaf partition (HDBSCANStar.java:79-103):
// per-row top-KC lists (self included, values as Java computes them), then the
// never-reset buffer = prefix merge over rows in row order (one lane).  KC >= K; the
// K-th smallest of a union is element K-1 of its top-KC.
template <int KC>
__device__ __forceinline__ void ins_kc(double (&buf)[KC], double x) {
    if (!(x < buf[KC - 1])) return;
#pragma unroll
    for (int i = 0; i < KC; i++) {
        double b = buf[i];
        bool lt = x < b;
        buf[i] = lt ? x : b;
        x = lt ? b : x;
    }
}

template <int BS, int KC>
__global__ __launch_bounds__(BS) void leaf_core_kernel(const double *__restrict__ X, int d, int metric,
                                                       const int64_t *__restrict__ offsets,
                                                       const int32_t *__restrict__ parts, int K,
                                                       double *__restrict__ lists /* rows*KC */,
                                                       double *__restrict__ core) {
    const int p = parts[blockIdx.x];
    const int64_t o = offsets[p];
    const int n = (int)(offsets[p + 1] - o);
    for (int i = threadIdx.x; i < n; i += BS) {
        double buf[KC];
#pragma unroll
        for (int k = 0; k < KC; k++) buf[k] = JMAX;
        const double *xi = X + (o + i) * d;
        for (int j = 0; j < n; j++) ins_kc<KC>(buf, metric_distance(xi, X + (o + j) * d, d, metric));
#pragma unroll
        for (int k = 0; k < KC; k++) lists[(o + i) * KC + k] = buf[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double buf[KC];
#pragma unroll
        for (int k = 0; k < KC; k++) buf[k] = JMAX;
        for (int i = 0; i < n; i++) {
#pragma unroll
            for (int k = 0; k < KC; k++) ins_kc<KC>(buf, lists[(o + i) * KC + k]);
            double c = buf[0];
#pragma unroll
            for (int k = 1; k < KC; k++)
                if (k == K - 1) c = buf[k];
            core[o + i] = c;
        }
    }
}

void leaf_cores_device(hdb_ctx *ctx, const double *X, int d, int metric, int P, const int64_t *d_off,
                       const int32_t *d_parts, int np, int64_t total_rows, int K, double *core) {
    if (np == 0) return;
    int KC = K <= 3 ? 3 : (K <= 7 ? 7 : (K <= 15 ? 15 : 31));
    if (K > 31) HDB_THROW(HDB_EINVAL, "minPts too large (max 32)");
    double *lists = (double *)arena(ctx, A_WORK2, sizeof(double) * (size_t)std::max<int64_t>(total_rows, 1) * KC);
    KernelTimer t(ctx, "leaf_core");
    switch (KC) {
    case 3: hipLaunchKernelGGL((leaf_core_kernel<256, 3>), dim3(np), dim3(256), 0, ctx->stream, X, d, metric, d_off, d_parts, K, lists, core); break;
    case 7: hipLaunchKernelGGL((leaf_core_kernel<256, 7>), dim3(np), dim3(256), 0, ctx->stream, X, d, metric, d_off, d_parts, K, lists, core); break;
    case 15: hipLaunchKernelGGL((leaf_core_kernel<256, 15>), dim3(np), dim3(256), 0, ctx->stream, X, d, metric, d_off, d_parts, K, lists, core); break;
    default: hipLaunchKernelGGL((leaf_core_kernel<256, 31>), dim3(np), dim3(256), 0, ctx->stream, X, d, metric, d_off, d_parts, K, lists, core); break;
    }
    HIP_CHECK(hipGetLastError());
    (void)P;
}

// ------------------------------------------------------ stepwise kernel
// State per partition (global): best[], par[], att[] over its vertices; partials
// [2][nwg_p] (value, index) double-buffered by step parity; step counter ctr[2].
struct StepState {
    double *best;
    int32_t *par;
    uint8_t *att;
    double *pv;     // [2][total_wg]
    int32_t *pidx;  // [2][total_wg]
    int32_t *cur0;  // start vertex per partition (n-1)
};

// Block b belongs to partition wg_part[b]; its local index within the partition's
// workgroups is b - wg_first[p]; partition p has wg_count[p] workgroups.
template <int BS, int PPT>
__global__ __launch_bounds__(BS) void prim_step_kernel(PrimIn in, const int64_t *__restrict__ offsets,
                                                       const int32_t *__restrict__ wg_part,
                                                       const int32_t *__restrict__ wg_first,
                                                       const int32_t *__restrict__ wg_count, StepState st,
                                                       int step, int parity) {
    constexpr int NW = BS / 64;
    __shared__ double s_v[NW];
    __shared__ int s_i[NW];
    __shared__ int s_cur;
    const int b = blockIdx.x;
    const int p = wg_part[b];
    const int64_t o = offsets[p];
    const int n = (int)(offsets[p + 1] - o);
    if (step >= n) return;  // this partition is done
    const int first = wg_first[p], cnt = wg_count[p];
    const int lb = b - first;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    // current vertex: reduce the previous step's partials (or the start vertex)
    int cur;
    if (step == 1) {
        cur = n - 1;
    } else {
        if (tid < 64) {
            double v = INFINITY;
            int i = -1;
            for (int q = lane; q < cnt; q += 64)
                argmin_last(v, i, st.pv[(parity ^ 1) * gridDim.x + first + q], st.pidx[(parity ^ 1) * gridDim.x + first + q]);
            wave_argmin_last(v, i);
            if (lane == 0) s_cur = i;
        }
        __syncthreads();
        cur = s_cur;
        if (cur < 0) return;
    }
    PrimIn L = in;
    L.X = in.X + o * in.d;
    L.core = in.core + o;
    L.ids = in.ids + o;
    if (in.eB) {
        L.eB = in.eB + o;
        L.nnB = in.nnB + o;
    }
    // mark cur attached (owner workgroup), skip it below
    const int per_wg = BS * PPT;
    const int base = lb * per_wg;
    double lv = INFINITY;
    int li = -1;
    const int cid = L.ids[cur];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        int i = base + tid + k * BS;
        if (i >= n) continue;
        const int64_t gi = o + i;
        if (i == cur) {
            st.att[gi] = 1;
            continue;
        }
        if (st.att[gi]) continue;
        double bst = st.best[gi];
        double mrd;
        if (mrd_improves(L, cur, i, bst, mrd)) {
            bst = mrd;
            st.best[gi] = mrd;
            st.par[gi] = cid;
        }
        argmin_last(lv, li, bst, i);
    }
    wave_argmin_last(lv, li);
    if (lane == 0) {
        s_v[wid] = lv;
        s_i[wid] = li;
    }
    __syncthreads();
    if (tid == 0) {
        double v = s_v[0];
        int i = s_i[0];
        for (int q = 1; q < NW; q++) argmin_last(v, i, s_v[q], s_i[q]);
        st.pv[parity * gridDim.x + b] = v;
        st.pidx[parity * gridDim.x + b] = i;
    }
}

__global__ void prim_step_init_kernel(const int64_t *__restrict__ offsets, int P, double *best, int32_t *par,
                                      uint8_t *att, int64_t total) {
    HDB_GRID_STRIDE(g, total) {
        best[g] = JMAX;
        par[g] = 0;
        att[g] = 0;
    }
}

__global__ void prim_step_final_kernel(PrimIn in, const int64_t *__restrict__ offsets,
                                       const int64_t *__restrict__ eoff, int P, StepState st, int self_edges,
                                       int32_t *__restrict__ va, int32_t *__restrict__ vb, double *__restrict__ w) {
    // one block per partition
    const int p = blockIdx.x;
    const int64_t o = offsets[p];
    const int n = (int)(offsets[p + 1] - o);
    const int64_t eo = eoff[p];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (i < n - 1) {
            va[eo + i] = st.par[o + i];
            vb[eo + i] = in.ids[o + i];
            w[eo + i] = st.best[o + i];
        }
        if (self_edges) {
            va[eo + n - 1 + i] = in.ids[o + i];
            vb[eo + n - 1 + i] = in.ids[o + i];
            w[eo + n - 1 + i] = in.core[o + i];
        }
    }
}

// ------------------------------------------------------------------ host

// --------------------------------------------------- cooperative kernel
// One partition of 4096 < n <= 65536 vertices (bubble models of the C3/C5 configs): one
// lane per vertex over ceil(n / BS) co-resident workgroups (cooperative launch), the whole
// Prim in one launch.  Each step: update + workgroup argmin, publish the partial, one
// grid barrier (monotone counter), every workgroup folds the nwg partials (argmin_last is
// associative and commutative, so all agree on the next vertex).  Partials are double
// buffered by step parity: a workgroup can be at most one step ahead of any other.
// Partial reads use agent-scope atomic loads (bypass the non-coherent L1).
template <int BS>
__global__ __launch_bounds__(BS) void prim_coop_kernel(PrimIn in, int n, int self_edges, int32_t *__restrict__ va,
                                                       int32_t *__restrict__ vb, double *__restrict__ w,
                                                       unsigned long long *__restrict__ part, unsigned *counter,
                                                       int *err) {
    constexpr int NW = BS / 64;
    __shared__ double s_v[NW];
    __shared__ int s_i[NW];
    __shared__ int s_cur;
    const int nwg = (int)gridDim.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i = (int)blockIdx.x * BS + tid;
    double best = JMAX;
    int par = -1;  // partition-local; ids[] applied once at the end (HDBSCANStar.java:137,172: 0 if never set)
    bool att = (i >= n) || (i == n - 1);
    int cur = n - 1;
    for (int step = 1; step < n; step++) {
        double lv = INFINITY;
        int li = -1;
        if (!att) {
            double mrd;
            if (mrd_improves(in, cur, i, best, mrd)) {
                best = mrd;
                par = cur;
            }
            argmin_last(lv, li, best, i);
        }
        wave_argmin_last(lv, li);
        if (lane == 0) {
            s_v[wid] = lv;
            s_i[wid] = li;
        }
        __syncthreads();
        const int buf = step & 1;
        if (tid == 0) {
            double v = s_v[0];
            int ii = s_i[0];
#pragma unroll
            for (int q = 1; q < NW; q++) argmin_last(v, ii, s_v[q], s_i[q]);
            __hip_atomic_store(&part[2 * (buf * nwg + blockIdx.x)], (unsigned long long)__double_as_longlong(v),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&part[2 * (buf * nwg + blockIdx.x) + 1], (unsigned long long)(unsigned)ii,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned target = (unsigned)step * (unsigned)nwg;
            unsigned spins = 0;
            while (__hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
                if (++spins > (1u << 26)) {  // a co-residency failure must not hang the device
                    atomicExch(err, 1);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __syncthreads();
        if (wid == 0) {
            double v = INFINITY;
            int ii = -1;
            for (int k = lane; k < nwg; k += 64) {
                const unsigned long long bv =
                    __hip_atomic_load(&part[2 * (buf * nwg + k)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long bi =
                    __hip_atomic_load(&part[2 * (buf * nwg + k) + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                argmin_last(v, ii, __longlong_as_double((long long)bv), (int)(unsigned)bi);
            }
            wave_argmin_last(v, ii);
            if (lane == 0) s_cur = ii;
        }
        __syncthreads();
        cur = s_cur;
        if (cur < 0) break;  // unreachable (an unattached vertex always exists) -- uniform exit
        if (i == cur) att = true;
        if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
    if (i < n - 1) {
        va[i] = par >= 0 ? in.ids[par] : 0;
        vb[i] = in.ids[i];
        w[i] = best;
    }
    if (self_edges && i < n) {
        va[n - 1 + i] = in.ids[i];
        vb[n - 1 + i] = in.ids[i];
        w[n - 1 + i] = in.core[i];
    }
}

// ------------------------------------------ cooperative kernel, rows in registers
// Same Prim (HDBSCANStar.java:124-205, select '<=' = last index, update '<'), restructured
// around the step's critical path: each lane keeps its own row (d <= DM), core and bubble
// terms in registers, and a workgroup publishes its candidate TOGETHER with that candidate's
// row, so there is no barrier counter and no dependent load of X[cur].  The exchange is double
// buffered by step parity (a workgroup is at most one step ahead).  prim_coop4_kernel below
// runs 3.0 us/step at 16 workgroups, 3.3 at 4, 3.9 at 64; the counter barrier 7.0 at 16, 17.8
// at 4.
// What was tried and removed ("Round 5" item 3 and "Round 6" item 5): step-tagged
// slots with a release/acquire tag, 6.3 us/step at 16 workgroups and 7.2 at 4 (s_memtime phases
// showed the __shfl_xor argmin folds, the dependent ids[cur] load and the single-lane slot
// stores, not the fences, held it there; tools/coop_prof.py); the same slots with a drained
// write-through payload and a relaxed poll; whole slots as tagged granules swept flat; every
// candidate row inside prim_coop4's key sweep; and a speculative kernel committing several
// steps per exchange (1.91 vs 2.07 us/step alone at 16,384 x 8, but 16.3 vs 10.8 s in the C5
// job, where several Prims share the device).
#ifdef HDB_COOP_PROF  // phase timestamps of steps [1024, 1088) of workgroup 0 (tools/coop_prof.py)
__device__ unsigned long long g_coop_prof[64 * 8];
#define COOP_T(k)                                                                                              \
    if (blockIdx.x == 0 && tid == 0 && step >= 1024 && step < 1088) g_coop_prof[(step - 1024) * 8 + (k)] =  \
        __builtin_amdgcn_s_memtime()
extern "C" int hdb_debug_coop_prof(unsigned long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_coop_prof), sizeof(g_coop_prof));
}
#else
#define COOP_T(k)
#endif

template <int DM>
__device__ __forceinline__ double coop_mrd(const PrimIn &in, const double (&xc)[DM], double cc, double ebc, double nnc,
                                           const double (&xi)[DM], double ci, double ebi, double nni, double best,
                                           bool &improves) {
    double dist;
    if (in.metric == HDB_METRIC_EUCLIDEAN) {  // the rows stay in registers (predicated, same order)
        double s = sq_diff(xc[0], xi[0]);
#pragma unroll
        for (int c = 1; c < DM; c++)
            if (c < in.d) s = s + sq_diff(xc[c], xi[c]);
        if (!in.eB) {
            const double thr = (best * best) * 1.0000000000000009;  // >= best^2 exactly
            if (s > thr) {
                improves = false;
                return best;
            }
        } else {
            // bubbles: with E = eB_c + eB_i >= 0 and nnB_c + nnB_i >= 0, distanceBubbles(d) >=
            // fl(d - E) > best once d > (best + E)(1 + 1e-12) (the margin covers every rounding
            // of sqrt, the subtraction and the square): no improvement, skip the sqrt
            const double E = ebc + ebi, T = (best + E) * (1.0 + 1e-12);
            if (s > T * T && E >= 0.0 && nnc + nni >= 0.0) {
                improves = false;
                return best;
            }
        }
        dist = sqrt(s);
    } else {
        dist = metric_distance(xc, xi, in.d, in.metric);
    }
    if (in.eB) dist = distance_bubbles(dist, ebc, ebi, nnc, nni);
    double mrd = dist;
    if (cc > mrd) mrd = cc;
    if (ci > mrd) mrd = ci;
    improves = mrd < best;
    return mrd;
}

typedef __attribute__((address_space(1))) unsigned long long gu64;

// prim_coop_slots = 4: one step = DPP wave minimum of order-preserving keys (the
// highest lane among equal keys is the argmin_last winner: indices grow with the lane), the
// wave's winner lane parks its row in LDS, ONE barrier, wave 0 folds the 16 waves the same way
// and publishes the workgroup's candidate as data-tagged 8-byte granules (Guideline 16 R2: 3
// key granules {value lo, value hi, index} + 2 (DM + 3) row granules, one sc1 store per lane),
// sweeps the nwg x 3 key granules flat until every tag is this step, picks the winner workgroup
// and reads its row granules straight into the LDS row; ONE barrier.  No fences, no counters.
// Same-XCD exchange (spread = 8): the grid is 8x the workgroups and only blocks b % 8 == res
// work -- blocks b and b + 8 are dealt to one XCD (res rotates per launch, so concurrent Prims
// of the model pool tend to land on different XCDs).  They check that at run time (XCC_ID): when
// every working block reports the same XCC, the granules are published with plain stores (the
// line stays in that XCD's L2, which every CU's sc1 poll reads) instead of sc1 stores (which
// drop the line from L2, so every poll crossed the fabric).  Any other placement keeps the sc1
// protocol: placement changes only speed.
template <int BS, int DM>
__global__ __launch_bounds__(BS) void prim_coop4_kernel(PrimIn in, int n, int self_edges, int32_t *__restrict__ va,
                                                        int32_t *__restrict__ vb, double *__restrict__ w,
                                                        gu64 *__restrict__ gkey, gu64 *__restrict__ grow, int *err,
                                                        unsigned spin_limit, int spread, int *__restrict__ xcc,
                                                        int res) {
    if ((int)(blockIdx.x % spread) != res) return;  // an idle block of a spread grid
    constexpr int NW = BS / 64;
    constexpr int ND = DM + 3;  // x, core, eB, nnB
    __shared__ double s_cand[NW][ND + 1];
    __shared__ int s_ci[NW];
    __shared__ unsigned s_key[3 * 64];
    __shared__ double s_row[ND];
    __shared__ int s_cur, s_local;
    const int nwg = (int)gridDim.x / spread;
    const int bid = (int)blockIdx.x / spread;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i = bid * BS + tid;
    if (tid == 0) s_local = 0;
    if (spread > 1 && wid == 0) {  // every working block on one XCC?
        if (lane == 0) {
            unsigned x;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
            __hip_atomic_store(xcc + bid, (int)(x & 15u) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        bool same = true;
        int first = 0;
        for (unsigned spins = 0;;) {
            bool ok = true;
            int mn = 1 << 30, mx = -1;
            for (int j = lane; j < nwg; j += 64) {
                const int v = __hip_atomic_load(xcc + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok &= v != 0;
                mn = min(mn, v);
                mx = max(mx, v);
            }
            if (__all(ok)) {
                for (int o = 32; o >= 1; o >>= 1) {
                    mn = min(mn, __shfl_xor(mn, o));
                    mx = max(mx, __shfl_xor(mx, o));
                }
                same = mn == mx;
                first = mn;
                break;
            }
            if (++spins > spin_limit) {  // not co-resident: the retry takes over
                if (lane == 0) atomicExch(err, 1);
                first = -1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (lane == 0) s_local = first < 0 ? -1 : (same && first > 0);
    }
    __syncthreads();
    if (s_local < 0) return;
    const bool local = s_local != 0;
    double xi[DM], ci = 0, ebi = 0, nni = 0;
#pragma unroll
    for (int c = 0; c < DM; c++) xi[c] = (i < n && c < in.d) ? in.X[(int64_t)i * in.d + c] : 0.0;
    if (i < n) {
        ci = in.core[i];
        if (in.eB) {
            ebi = in.eB[i];
            nni = in.nnB[i];
        }
    }
    double best = JMAX;
    int par = -1;
    bool att = (i >= n) || (i == n - 1);
    double xc[DM], cc, ebc = 0, nnc = 0;
#pragma unroll
    for (int c = 0; c < DM; c++) xc[c] = c < in.d ? in.X[(int64_t)(n - 1) * in.d + c] : 0.0;
    cc = in.core[n - 1];
    if (in.eB) {
        ebc = in.eB[n - 1];
        nnc = in.nnB[n - 1];
    }
    int cur = n - 1;
    constexpr unsigned long long KINF = 0x7ff0000000000000ull | MRD_KEY_SIGN;  // mrd_key(+inf): nothing to offer
    // Candidate caching: a wave's candidate changes only when one of its lanes
    // improved or its parked winner was attached in the last step, and a workgroup's only when
    // one of its waves' did -- most steps relax nothing near most waves (the sqrt-free rejection
    // in coop_mrd), so the wave minimum, the parking and the workgroup fold are skipped and the
    // workgroup republishes its cached granule values under the new step's tag.
    __shared__ int s_dirty;
    if (tid == 0) s_dirty = 0;
    bool just = false;    // this lane was attached at the end of the last step
    unsigned val_c = 0u;  // wave 0: the workgroup's cached granule value (this lane's)
    for (int step = 1; step < n; step++) {
        COOP_T(0);
        bool imp = false;
        double mrd = 0.0;
        if (!att) mrd = coop_mrd<DM>(in, xc, cc, ebc, nnc, xi, ci, ebi, nni, best, imp);
        if (imp) {
            best = mrd;
            par = cur;
        }
        COOP_T(6);
        const bool dirty = step == 1 || __any(imp || just);
        just = false;
        if (dirty) {
            const unsigned long long key = att ? KINF : mrd_key(best);
            const unsigned long long wmin = wave_min_u64(key);
            const int wl = last_lane(key == wmin);
            if (lane == wl) {  // the wave's candidate parks its row
#pragma unroll
                for (int c = 0; c < DM; c++) s_cand[wid][c] = xi[c];
                s_cand[wid][DM] = ci;
                s_cand[wid][DM + 1] = ebi;
                s_cand[wid][DM + 2] = nni;
                s_cand[wid][ND] = best;
                s_ci[wid] = wmin < KINF ? i : -1;
                s_dirty = 1;
            }
        }
        COOP_T(7);
        __syncthreads();
        COOP_T(1);
        if (wid == 0) {
            const int buf = step & 1;
            const unsigned tag = (unsigned)step;
            unsigned val;
            if (s_dirty) {
                // fold the waves: lane q holds wave q's candidate
                const int qi = lane < NW ? s_ci[lane] : -1;
                const unsigned long long qk = qi >= 0 ? mrd_key(s_cand[lane < NW ? lane : 0][ND]) : KINF;
                const unsigned long long gmin = wave_min_u64(qk);
                const int q = min(last_lane(qk == gmin), NW - 1);  // all waves empty: any wave (index -1)
                const unsigned *cw = (const unsigned *)s_cand[q];
                const int gidx = __builtin_amdgcn_readlane(qi, q);  // q is wave-uniform
                // publish: lanes 0-2 the key granules, lanes 3 .. 3 + 2 ND the row granules
                if (lane < 2) val = cw[2 * ND + lane];
                else if (lane == 2) val = (unsigned)gidx;
                else val = lane < 3 + 2 * ND ? cw[lane - 3] : 0u;
                val_c = val;
            } else
                val = val_c;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) s_dirty = 0;  // every lane of wave 0 has read it; set again only after the next barrier
            const unsigned long long gv = ((unsigned long long)tag << 32) | val;
            gu64 *dst = nullptr;
            if (lane < 3)
                dst = gkey + ((size_t)buf * nwg + bid) * 3 + lane;
            else if (lane < 3 + 2 * ND)
                dst = grow + ((size_t)buf * nwg + bid) * (2 * ND) + (lane - 3);
            if (dst) {
                // local: a plain (workgroup-scope) store -- the line stays in the XCD's L2, which
                // every CU of that XCD polls with agent-scope loads.  This relies on gfx950
                // details the HIP memory model does not promise (a write-through L1 and one L2
                // per XCD; every working block checked to be on one XCC above).  Correctness never
                // depends on it: each granule carries its step tag, and if the values were not
                // seen the plain attempt times out and the cooperative launch (agent-scope
                // stores) runs instead -- visible as prim_coop_plain_retries in the C3/C5 lines
                if (local)
                    __hip_atomic_store(dst, gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    __hip_atomic_store(dst, gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            COOP_T(2);
            // sweep every workgroup's key granules
            const gu64 *kb = gkey + (size_t)buf * nwg * 3;
            const int T = 3 * nwg;
            bool tmo = false;
            for (unsigned spins = 0;;) {
                bool ok = true;
                for (int j = lane; j < T; j += 64) {
                    const unsigned long long x = __hip_atomic_load(kb + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok &= (unsigned)(x >> 32) == tag;
                    s_key[j] = (unsigned)x;
                }
                if (__all(ok)) break;
                if (++spins > spin_limit) {  // a co-residency failure must not hang the device
                    if (lane == 0) atomicExch(err, 1);
                    tmo = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            COOP_T(3);
            __builtin_amdgcn_wave_barrier();
            int kidx = -1;
            unsigned long long kk = KINF;
            if (lane < nwg) {
                kidx = (int)s_key[3 * lane + 2];
                const double kv = __longlong_as_double(
                    (long long)(((unsigned long long)s_key[3 * lane + 1] << 32) | s_key[3 * lane]));
                if (kidx >= 0) kk = mrd_key(kv);
            }
            const unsigned long long amin = wave_min_u64(kk);
            const int k = last_lane(kk == amin);
            const int win = __builtin_amdgcn_readlane(kidx, k);  // k is wave-uniform
            if (tmo || amin == KINF) {
                if (lane == 0) s_cur = -1;
            } else {
                bool row_tmo = false;
                if (lane < 2 * ND) {  // the winner's row granules, straight into the LDS row
                    const gu64 *rb = grow + ((size_t)buf * nwg + k) * (2 * ND) + lane;
                    unsigned long long x;
                    for (unsigned spins = 0;;) {
                        x = __hip_atomic_load(rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((unsigned)(x >> 32) == tag) break;
                        if (++spins > spin_limit) {  // a stale row must not be used: report, exit
                            row_tmo = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    ((unsigned *)s_row)[lane] = (unsigned)x;
                }
                if (__any(row_tmo)) {
                    if (lane == 0) {
                        atomicExch(err, 1);
                        s_cur = -1;
                    }
                } else if (lane == 0)
                    s_cur = win;
            }
            COOP_T(4);
        }
        __syncthreads();
        COOP_T(5);
        cur = s_cur;
        if (cur < 0) break;
#pragma unroll
        for (int c = 0; c < DM; c++) xc[c] = s_row[c];
        cc = s_row[DM];
        ebc = s_row[DM + 1];
        nnc = s_row[DM + 2];
        if (i == cur) {
            att = true;
            just = true;
        }
    }
    if (i < n - 1) {
        va[i] = par >= 0 ? in.ids[par] : 0;
        vb[i] = in.ids[i];
        w[i] = best;
    }
    if (self_edges && i < n) {
        va[n - 1 + i] = in.ids[i];
        vb[n - 1 + i] = in.ids[i];
        w[n - 1 + i] = in.core[i];
    }
}

// the plain attempt's same-XCD exchange (prim_coop_xcd) is for Prims of at most this many
// workgroups (one XCD: 32 CUs)
constexpr int PRIM_XCD_MAX_WG = 32;

// the inputs as one partition sees them: its rows start at o
static PrimIn partition_slice(const PrimIn &in, int64_t o) {
    PrimIn L = in;
    L.X = in.X + o * in.d;
    L.core = in.core + o;
    L.ids = in.ids + o;
    if (in.eB) {
        L.eB = in.eB + o;
        L.nnB = in.nnB + o;
    }
    return L;
}

// workgroups of `kernel` (bs threads, no dynamic LDS) one CU holds, or 0 when the device cannot
// keep nwg of them co-resident under a cooperative launch
static int coop_per_cu(hdb_ctx *ctx, const void *kernel, int bs, int nwg) {
    int coop = 0, ncu = 0, per_cu = 0;
    HIP_CHECK(hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, ctx->device));
    HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, bs, 0));
    return coop && (int64_t)per_cu * ncu >= nwg ? per_cu : 0;
}

template <int DM, int BS>
static bool launch_coop4_bs(hdb_ctx *ctx, const PrimIn &in, int64_t o, int64_t n, int64_t eo, int self_edges,
                            int32_t *va, int32_t *vb, double *w) {
    const int nwg = (int)ceil_div(n, BS);
    if (nwg > 64) return false;
    const int per_cu = coop_per_cu(ctx, (const void *)prim_coop4_kernel<BS, DM>, BS, nwg);
    if (!per_cu) return false;
    constexpr int ND = DM + 3;
    char *state;
    gu64 *gkey, *grow;
    int *err;
    const size_t state_bytes = carve(ctx, A_WORK3, [&](Carver &cv) {
        state = cv.base;
        gkey = (gu64 *)cv.take<unsigned long long>(3 * 2 * nwg);
        grow = (gu64 *)cv.take<unsigned long long>(2 * ND * 2 * nwg);
        err = cv.take<int>(128);
        return cv.off;
    });
    int *xcc = err + 64;  // the working blocks' XCC ids (spread launch)
    HIP_CHECK(hipMemsetAsync(state, 0, state_bytes, ctx->stream));  // tags 0: no step yet
    PrimIn L = partition_slice(in, o);
    int nn = (int)n;
    int32_t *pva = va + eo, *pvb = vb + eo;
    double *pw = w + eo;
    unsigned spin = 1u << 24;
    int spread1 = 1, res0 = 0;
    void *args[] = {&L, &nn, &self_edges, &pva, &pvb, &pw, &gkey, &grow, &err, &spin, &spread1, &xcc, &res0};
    // same-XCD exchange for the plain attempt when its blocks fit one XCD (32 CUs)
    const int spread = (ctx->prim_coop_xcd && nwg <= PRIM_XCD_MAX_WG && nwg <= 32 * per_cu) ? 8 : 1;
    static std::atomic<int> launches{0};
    const int res = spread > 1 ? (launches.fetch_add(1) & 7) : 0;
    // A plain launch first: ROCm serialises cooperative launches device-wide, so the concurrent
    // local models of one level (driver model pool) would queue behind each other.  The grid
    // (<= 64 workgroups) is far below the device's capacity, and every inter-workgroup wait has
    // a timeout: if the workgroups were not co-resident the kernel reports it and exits, the
    // state is reset and the cooperative launch (guaranteed co-residency) runs instead.  The
    // plain attempt waits at most 2^prim_coop_plain_spin_log2 polls per exchange (a step takes
    // microseconds once every workgroup runs; the default 2^20 polls is ~1 s), the cooperative
    // one 2^24.
    const unsigned plain_spin = 1u << ctx->prim_coop_plain_spin_log2;
    int h_err = 0;
    for (int attempt = ctx->prim_coop_plain ? 0 : 1; attempt < 2; attempt++) {
        if (attempt == 1 && h_err) HIP_CHECK(hipMemsetAsync(state, 0, state_bytes, ctx->stream));
        {
            KernelTimer t(ctx, "prim_coop");
            if (attempt == 0)
                hipLaunchKernelGGL((prim_coop4_kernel<BS, DM>), dim3(nwg * spread), dim3(BS), 0, ctx->stream, L, nn,
                                   self_edges, pva, pvb, pw, gkey, grow, err, plain_spin, spread, xcc, res);
            else
                HIP_CHECK(hipLaunchCooperativeKernel((const void *)prim_coop4_kernel<BS, DM>, dim3(nwg), dim3(BS), args,
                                                     0, ctx->stream));
            HIP_CHECK(hipGetLastError());
        }
        h_err = 0;
        HIP_CHECK(hipMemcpyAsync(&h_err, err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (!h_err) {
            ctx->stats["prim_coop_steps"] += n - 1;  // sequential Prim steps (roofline: bench.py)
            ctx->stats["prim_coop_launches"] += 1;
            ctx->stats["prim_coop_last_bs"] = BS;  // what the last cooperative Prim ran with (tests)
            ctx->stats["prim_coop_last_spread"] = attempt == 0 ? spread : 1;
            return true;
        }
        if (attempt == 0) ctx->stats["prim_coop_plain_retries"] += 1;
    }
    HDB_THROW(HDB_EDEVICE, "prim_coop: key sweep timed out (workgroups not co-resident)");
    return true;
}

// workgroup size: 1024 by default; prim_coop_bs = 0 takes the smallest of 128..1024 that keeps
// the Prim within PRIM_XCD_MAX_WG workgroups (one XCD), so more CUs -- and fewer waves per
// SIMD -- share each step's relaxation
template <int DM>
static bool launch_coop4(hdb_ctx *ctx, const PrimIn &in, int64_t o, int64_t n, int64_t eo, int self_edges,
                         int32_t *va, int32_t *vb, double *w) {
    int bs = ctx->prim_coop_bs;
    if (bs == 0) {
        bs = 1024;
        for (int b = 128; b < 1024; b *= 2)
            if (ceil_div(n, (int64_t)b) <= PRIM_XCD_MAX_WG) {
                bs = b;
                break;
            }
    }
    switch (bs) {
    case 128: return launch_coop4_bs<DM, 128>(ctx, in, o, n, eo, self_edges, va, vb, w);
    case 256: return launch_coop4_bs<DM, 256>(ctx, in, o, n, eo, self_edges, va, vb, w);
    case 512: return launch_coop4_bs<DM, 512>(ctx, in, o, n, eo, self_edges, va, vb, w);
    default: return launch_coop4_bs<DM, 1024>(ctx, in, o, n, eo, self_edges, va, vb, w);
    }
}

static bool launch_coop(hdb_ctx *ctx, const PrimIn &in, int64_t o, int64_t n, int64_t eo, int self_edges,
                        int32_t *va, int32_t *vb, double *w) {
    constexpr int BS = 1024;
    const int nwg = (int)ceil_div(n, BS);
    if (n > 65536 || nwg < 1) return false;
    if (!coop_per_cu(ctx, (const void *)prim_coop_kernel<BS>, BS, nwg)) return false;
    // scratch: partials [2][nwg] x (value, index), barrier counter, error flag
    char *base = (char *)arena(ctx, A_WORK3, 16 * 2 * (size_t)nwg + 512);
    unsigned long long *part = (unsigned long long *)base;
    unsigned *counter = (unsigned *)(base + 16 * 2 * (size_t)nwg + 256);
    int *err = (int *)(counter + 16);
    HIP_CHECK(hipMemsetAsync(counter, 0, 256, ctx->stream));
    PrimIn L = partition_slice(in, o);
    int nn = (int)n;
    int32_t *pva = va + eo, *pvb = vb + eo;
    double *pw = w + eo;
    void *args[] = {&L, &nn, &self_edges, &pva, &pvb, &pw, &part, &counter, &err};
    {
        KernelTimer t(ctx, "prim_coop");
        HIP_CHECK(hipLaunchCooperativeKernel((const void *)prim_coop_kernel<BS>, dim3(nwg), dim3(BS), args, 0,
                                             ctx->stream));
    }
    int h_err = 0;
    HIP_CHECK(hipMemcpyAsync(&h_err, err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h_err) HDB_THROW(HDB_EDEVICE, "prim_coop: grid barrier timed out (workgroups not co-resident)");
    return true;
}

template <int BS, int PPT>
static void launch_block(hdb_ctx *ctx, const PrimIn &in, const int64_t *offs, const int64_t *eoff,
                         const int32_t *parts, int np, int self_edges, int32_t *va, int32_t *vb, double *w) {
    if (np == 0) return;
    KernelTimer t(ctx, "prim_block");
    hipLaunchKernelGGL((prim_block_kernel<BS, PPT>), dim3(np), dim3(BS), 0, ctx->stream, in, offs, eoff, parts,
                       self_edges, va, vb, w);
    HIP_CHECK(hipGetLastError());
}

// size classes for the block kernel
static int block_class(int64_t n) {
    if (n <= 64) return 0;        // 64 x 1
    if (n <= 256) return 1;       // 64 x 4
    if (n <= 1024) return 2;      // 256 x 4
    if (n <= 4096) return 3;      // 1024 x 4
    return 4;                     // stepwise
}

// Batched Prim. Device pointers: X (rows), offsets (P+1, host copy h_offs), core, ids.
void prim_batched_device(hdb_ctx *ctx, const PrimIn &in, const int64_t *h_offs, int P, int self_edges,
                         int32_t *va, int32_t *vb, double *w) {
    // edge offsets + per-class partition lists (host side), then upload
    std::vector<int64_t> eoff(P + 1, 0);
    std::vector<int32_t> cls[5];
    int64_t total_v = h_offs[P] - h_offs[0];
    for (int p = 0; p < P; p++) {
        int64_t n = h_offs[p + 1] - h_offs[p];
        if (n < 0) HDB_THROW(HDB_EINVAL, "offsets must be non-decreasing");
        eoff[p + 1] = eoff[p] + (n > 0 ? (n - 1) + (self_edges ? n : 0) : 0);
        // wide rows (d >= 8): one workgroup re-reads n x d doubles per step through one CU; the
        // cooperative kernel keeps one row per lane in registers across ceil(n / 1024) CUs
        // (C3's 4,096-bubble models: 19.6 -> 7.4 us/step)
        int c = block_class(n);
        if (c == 3 && in.d >= 8 && in.d <= 16 && ctx->prim_coop && ctx->prim_coop_slots == 4) c = 4;
        if (n > 0) cls[c].push_back(p);
    }
    // cooperative single-launch Prim for 4096 < n <= 65536 when the device allows it
    if (ctx->prim_coop) {
        std::vector<int32_t> rest;
        for (int32_t p : cls[4]) {
            int64_t n = h_offs[p + 1] - h_offs[p];
            const int64_t o = h_offs[p] - h_offs[0];
            bool ok = false;
            if (n <= 65536 && ctx->prim_coop_slots == 4) {  // rows in registers: d <= 16 only
                if (in.d <= 4) ok = launch_coop4<4>(ctx, in, o, n, eoff[p], self_edges, va, vb, w);
                else if (in.d <= 8) ok = launch_coop4<8>(ctx, in, o, n, eoff[p], self_edges, va, vb, w);
                else if (in.d <= 16) ok = launch_coop4<16>(ctx, in, o, n, eoff[p], self_edges, va, vb, w);
            }
            if (!ok) ok = launch_coop(ctx, in, o, n, eoff[p], self_edges, va, vb, w);  // any d; declines n > 65536
            if (!ok) rest.push_back(p);
        }
        cls[4].swap(rest);
    }
    // stepwise state
    std::vector<int32_t> wg_part, wg_first(P, 0), wg_count(P, 0);
    constexpr int SBS = 256, SPPT = 4;
    for (int32_t p : cls[4]) {
        int64_t n = h_offs[p + 1] - h_offs[p];
        int c = (int)ceil_div(n, SBS * SPPT);
        wg_first[p] = (int)wg_part.size();
        wg_count[p] = c;
        for (int q = 0; q < c; q++) wg_part.push_back(p);
    }
    int nwg = (int)wg_part.size();
    int64_t *d_off, *d_eoff;
    int32_t *d_parts, *d_wgp, *d_wgf, *d_wgc;
    StepState st{};
    carve(ctx, A_WORK1, [&](Carver &cv) {
        d_off = cv.take<int64_t>(P + 1), d_eoff = cv.take<int64_t>(P + 1);
        d_parts = cv.take<int32_t>(P + 1);
        d_wgp = cv.take<int32_t>(nwg + 1), d_wgf = cv.take<int32_t>(P + 1), d_wgc = cv.take<int32_t>(P + 1);
        if (nwg) {
            st.best = cv.take<double>(total_v);
            st.par = cv.take<int32_t>(total_v);
            st.att = cv.take<uint8_t>(total_v);
            st.pv = cv.take<double>(2 * nwg);
            st.pidx = cv.take<int32_t>(2 * nwg);
        }
    });
    std::vector<int64_t> rel(P + 1);
    for (int p = 0; p <= P; p++) rel[p] = h_offs[p] - h_offs[0];
    HIP_CHECK(hipMemcpyAsync(d_off, rel.data(), sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(d_eoff, eoff.data(), sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> plist;
    int cstart[5];
    for (int c = 0; c < 5; c++) {
        cstart[c] = (int)plist.size();
        plist.insert(plist.end(), cls[c].begin(), cls[c].end());
    }
    if (!plist.empty())
        HIP_CHECK(hipMemcpyAsync(d_parts, plist.data(), sizeof(int32_t) * plist.size(), hipMemcpyHostToDevice,
                                 ctx->stream));
    launch_block<64, 1>(ctx, in, d_off, d_eoff, d_parts + cstart[0], (int)cls[0].size(), self_edges, va, vb, w);
    launch_block<64, 4>(ctx, in, d_off, d_eoff, d_parts + cstart[1], (int)cls[1].size(), self_edges, va, vb, w);
    launch_block<256, 4>(ctx, in, d_off, d_eoff, d_parts + cstart[2], (int)cls[2].size(), self_edges, va, vb, w);
    launch_block<1024, 4>(ctx, in, d_off, d_eoff, d_parts + cstart[3], (int)cls[3].size(), self_edges, va, vb, w);
    if (nwg) {
        HIP_CHECK(hipMemcpyAsync(d_wgp, wg_part.data(), sizeof(int32_t) * nwg, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(d_wgf, wg_first.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(d_wgc, wg_count.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(prim_step_init_kernel, dim3(1024), dim3(256), 0, ctx->stream, d_off, P, st.best, st.par,
                           st.att, total_v);
        int64_t maxn = 0;
        for (int32_t p : cls[4]) maxn = std::max(maxn, h_offs[p + 1] - h_offs[p]);
        // steps 1..maxn-1 run on the context's side stream (capturable) in chunks captured
        // into a hipGraph and replayed; fenced to/from the caller's stream by events.
        const int CH = 256;
        hipStream_t ss = ctx->side;
        stream_fence(ctx, ctx->stream, ss);
        hipGraphExec_t exec = nullptr;
        KernelTimer t(ctx, "prim_step_total");
        int step = 1;
        auto launch_one = [&](int s) {
            hipLaunchKernelGGL((prim_step_kernel<SBS, SPPT>), dim3(nwg), dim3(SBS), 0, ss, in, d_off, d_wgp, d_wgf,
                               d_wgc, st, s, s & 1);
        };
        try {
            while (step < maxn) {
                int remain = (int)(maxn - step);
                if (remain < CH) {
                    for (int s = 0; s < remain; s++) launch_one(step + s);
                    HIP_CHECK(hipGetLastError());
                    step += remain;
                    continue;
                }
                hipGraph_t graph;
                HIP_CHECK(hipStreamBeginCapture(ss, hipStreamCaptureModeThreadLocal));
                for (int s = 0; s < CH; s++) launch_one(step + s);
                hipError_t ce = hipStreamEndCapture(ss, &graph);
                HIP_CHECK(ce);
                if (!exec) {
                    HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
                } else {
                    hipGraphExecUpdateResult res;
                    hipGraphNode_t errn;
                    if (hipGraphExecUpdate(exec, graph, &errn, &res) != hipSuccess) {
                        (void)hipGetLastError();
                        HIP_CHECK(hipGraphExecDestroy(exec));
                        HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
                    }
                }
                HIP_CHECK(hipGraphLaunch(exec, ss));
                HIP_CHECK(hipGraphDestroy(graph));
                step += CH;
            }
        } catch (...) {
            hipGraph_t g = nullptr;
            hipStreamCaptureStatus cs;
            if (hipStreamIsCapturing(ss, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) {
                (void)hipStreamEndCapture(ss, &g);
                if (g) (void)hipGraphDestroy(g);
            }
            if (exec) (void)hipGraphExecDestroy(exec);
            throw;
        }
        stream_fence(ctx, ss, ctx->stream);
        if (exec) {
            HIP_CHECK(hipStreamSynchronize(ss));
            HIP_CHECK(hipGraphExecDestroy(exec));
        }
        // edges for stepwise partitions
        std::vector<int32_t> big(cls[4].begin(), cls[4].end());
        for (int32_t p : big) {
            // one block per partition via a shifted offsets view
            hipLaunchKernelGGL(prim_step_final_kernel, dim3(1), dim3(256), 0, ctx->stream, in, d_off + p, d_eoff + p, 1,
                               st, self_edges, va, vb, w);
        }
        HIP_CHECK(hipGetLastError());
    }
}

}  // namespace hdb
