// constraints.hip -- hdb_constrained_flat_labels on the device: the semi-supervised flat
// extraction over the arrays of hdb_flat_cluster_tree (DESIGN.md "Constrained flat labels";
// csrc/constraints.cpp is the host algorithm this must equal bit for bit).
//
// All arrays below are indexed by TREE LABEL 0..K (0 = none), stride K + 1.
//  1. cs_init / cs_double: validated parents (a bad one becomes 0, so every later index is
//     bounded), child counts, the binary-lifting table anc[j][c] = the 2^j-th ancestor and the
//     depth of every cluster, both by pointer doubling (J = ceil(log2 K) rounds).
//  2. cs_constraints: one thread per constraint.  The deeper endpoint cluster is lifted to the
//     other's depth, then both descend the table to the LCA: O(log K) reads of a table that
//     stays in the L2.  Integer atomics into a difference array (must-link diff[L] += 2;
//     cannot-link diff[last(a)] += 1, diff[last(b)] += 1, diff[L] -= 2) and into virt: adds are
//     order-free, so the counts are exact.  num_sat is the subtree sum of diff.  The diff[L]
//     updates of a wave are combined first, one add per distinct target: random pairs meet in
//     the few clusters under the root.
//  3. children lists: a stable radix sort of (parent, label) and an exclusive scan of the child
//     counts: the children of a cluster in ascending label.  cs_meta packs what the climb reads
//     per cluster into one 16-byte record; a cluster's slot in the lists is where its hand-off
//     record goes, so a parent reads its children's records contiguously.
//  4. cs_climb: ONE launch for the whole bottom-up pass, whatever the depth of the tree (a
//     condensed tree is chain-like, thousands of levels deep: one launch per level is out).
//     A lane starts at each leaf, evaluates it, stores its record, and adds 1 to its parent's
//     arrival counter; only the lane whose add returns nch - 1 -- the last child to arrive --
//     goes on to evaluate the parent, reading the children's records in list order.  No lane
//     ever waits for another, so nothing can hang.  The hand-off between the lanes is the form
//     measured on gfx950: records stored with agent-scope atomic stores, the storing wave's
//     s_waitcnt vmcnt(0), a returning agent-scope atomic add, and agent-scope atomic loads of the
//     records only after that add has returned.  At most one workgroup per CU.
//  5. selection: pointer jumping for the topmost self-chosen cluster of every chain, numbering
//     by a radix sort of (min_id, label) over the selected clusters, one gather per point.
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <optional>

#include "common.hpp"
#include "internal.hpp"
#include "sort.hpp"

namespace hdb {

namespace {

enum : int { CE_ROOT = 1, CE_PARENT = 2, CE_POINT = 4, CE_ID = 8, CE_TYPE = 16 };
constexpr int CS_TB = 256;

__device__ __forceinline__ void cs_flag(int *flag, int bits) {  // every thread of the workgroup calls it
    __shared__ int sbits;
    if (threadIdx.x == 0) sbits = 0;
    __syncthreads();
    if (bits) atomicOr(&sbits, bits);
    __syncthreads();
    if (threadIdx.x == 0 && sbits) atomicOr(flag, sbits);
}

// relaxed agent-scope accesses (global_load / global_store sc1: served by the L2, never by a
// CU's L1) for the records one lane hands to another inside cs_climb
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// row 0 of the table, depths of one step, child counts, the sort input of the children lists
__global__ void cs_init(const int32_t *__restrict__ parent, int32_t K, int32_t *__restrict__ anc0,
                        int32_t *__restrict__ dep0, int32_t *__restrict__ nch, uint32_t *__restrict__ skey,
                        int32_t *__restrict__ sval, int *__restrict__ err) {
    int e = 0;
    HDB_GRID_STRIDE(i, (int64_t)K + 1) {
        int32_t p = 0;
        if (i > 0) {
            p = parent[i - 1];
            if (i == 1 && p != 0) e |= CE_ROOT, p = 0;
            if (p < 0 || p >= i) e |= CE_PARENT, p = 0;  // parent label in 0..label - 1
            atomicAdd(&nch[p], 1);                       // nch[0] counts the roots
            skey[i - 1] = (uint32_t)p;
            sval[i - 1] = (int32_t)i;
        }
        anc0[i] = p;
        dep0[i] = i > 0;
    }
    cs_flag(err, e);
}

__global__ void cs_double(const int32_t *__restrict__ prev, int32_t *__restrict__ next,
                          const int32_t *__restrict__ dprev, int32_t *__restrict__ dnext, int32_t K) {
    HDB_GRID_STRIDE(i, (int64_t)K + 1) {
        const int32_t a = prev[i];  // values are in 0..K by construction
        next[i] = prev[a];
        dnext[i] = dprev[i] + dprev[a];
    }
}

__global__ void cs_constraints(const int32_t *__restrict__ anc, const int32_t *__restrict__ depth, int32_t K, int J,
                               const int32_t *__restrict__ point_cluster, int64_t n, const int32_t *__restrict__ ca,
                               const int32_t *__restrict__ cb, const int32_t *__restrict__ ctype, int64_t m,
                               uint32_t *__restrict__ diff, uint32_t *__restrict__ virt, int *__restrict__ err) {
    const int64_t stride = (int64_t)K + 1;
    const int lane = threadIdx.x & 63;
    int e = 0;
    // the trip count is uniform per workgroup: the wave votes below need every lane
    for (int64_t base = (int64_t)blockIdx.x * CS_TB; base < m; base += (int64_t)gridDim.x * CS_TB) {
        const int64_t k = base + threadIdx.x;
        int32_t x = 0, t = HDB_CONSTRAINT_MUST_LINK;
        bool pending = false;  // an update of diff[x] is due: +2 (must-link) or -2 (cannot-link)
        if (k < m) {
            const int32_t a = ca[k], b = cb[k];
            t = ctype[k];
            if (a < 0 || a >= n || b < 0 || b >= n) {
                e |= CE_ID;
            } else if (t != HDB_CONSTRAINT_MUST_LINK && t != HDB_CONSTRAINT_CANNOT_LINK) {
                e |= CE_TYPE;
            } else {
                const int32_t la = point_cluster[a], lb = point_cluster[b];
                if (la < 1 || la > K || lb < 1 || lb > K) {
                    e |= CE_POINT;
                } else {
                    x = la;
                    int32_t y = lb, dx = depth[x], dy = depth[y];
                    if (dx < dy) {
                        int32_t s = x;
                        x = y, y = s;
                        s = dx, dx = dy, dy = s;
                    }
                    int32_t up = dx - dy;  // < 2^J: a chain has at most K clusters
                    for (int j = 0; up != 0 && j < J; j++, up >>= 1)
                        if (up & 1) x = anc[j * stride + x];
                    if (x != y) {
                        for (int j = J - 1; j >= 0; j--) {
                            const int32_t ax = anc[j * stride + x], ay = anc[j * stride + y];
                            if (ax != ay) x = ax, y = ay;
                        }
                        x = anc[x];  // 0 when the two clusters hang under different roots (an invalid tree)
                    }
                    if (t == HDB_CONSTRAINT_MUST_LINK) {
                        pending = true;
                    } else if (la != lb) {  // equal: +1 +1 -2 on one word
                        atomicAdd(&diff[la], 1u);
                        atomicAdd(&diff[lb], 1u);
                        atomicAdd(&virt[la], 1u);
                        atomicAdd(&virt[lb], 1u);
                        pending = true;
                    } else {
                        atomicAdd(&virt[la], 2u);
                    }
                }
            }
        }
        // The LCA of two random points is mostly one of the few clusters under the root, so a
        // wave's updates land on a handful of words (1M uniform pairs: 4.0 ms of this kernel were
        // atomics on one cache line: the top clusters have adjacent labels).  Per round the lanes
        // that share the first pending lane's target send one add between them; at most 64 rounds
        // of a few wave instructions each, one atomic per distinct target of the wave.
        while (true) {
            const unsigned long long act = __ballot(pending);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const int32_t tx = __shfl(x, leader);
            const bool mine = pending && x == tx;
            const unsigned long long mm = __ballot(mine && t == HDB_CONSTRAINT_MUST_LINK), mall = __ballot(mine);
            if (lane == leader) atomicAdd(&diff[tx], 2u * (uint32_t)__popcll(mm) - 2u * (uint32_t)__popcll(mall & ~mm));
            if (mine) pending = false;
        }
    }
    cs_flag(err, e);
}

// the record a cluster hands to its parent: {subtree sum of diff | chosen_sat << 32, chosen_stab}
struct __align__(16) CRec {
    unsigned long long cnt, stab;
};

// per cluster, for the climb: one 16-byte load instead of a chain of dependent ones.  slot = the
// cluster's position in the children lists (records are kept in list order, so a parent reads
// its children's records at off .. off + nch without going through the list)
struct __align__(16) CMeta {
    int32_t parent, nch, off, slot;
};

__global__ void cs_meta(const int32_t *__restrict__ anc0, const int32_t *__restrict__ nch,
                        const int32_t *__restrict__ off, const int32_t *__restrict__ kids, int32_t K,
                        CMeta *__restrict__ meta, int32_t *__restrict__ pnch) {
    HDB_GRID_STRIDE(r, K) {
        const int32_t c = kids[r], p = anc0[c];  // kids: a permutation of 1..K, grouped by parent
        meta[c] = CMeta{p, nch[c], off[c], (int32_t)r};
        pnch[c] = nch[p];
    }
}

__global__ __launch_bounds__(CS_TB) void cs_climb(const CMeta *__restrict__ meta, const int32_t *__restrict__ pnch,
                                                 const uint32_t *__restrict__ diff, const uint32_t *__restrict__ virt,
                                                 const double *__restrict__ stability, int32_t K, CRec *rec,
                                                 int32_t *arrive, int32_t *__restrict__ self,
                                                 int32_t *__restrict__ num_sat, int32_t *__restrict__ prop_sat,
                                                 double *__restrict__ prop_stab) {
    HDB_GRID_STRIDE(i, K) {
        int32_t c = (int32_t)i + 1;
        if (meta[c].nch != 0) continue;  // lanes start at the leaves
        while (true) {
            const CMeta mc = meta[c];
            const int32_t kc = mc.nch, p = mc.parent, pn = pnch[c];
            uint32_t sub = diff[c], ps = kc ? virt[c] : 0u;
            const double st = stability[c - 1];
            double pst = 0.0;
            for (int32_t q = 0; q < kc; q++) {  // list order = ascending label: the order of the stability sum
                const unsigned long long w = ld_agent(&rec[mc.off + q].cnt);
                const double s = __longlong_as_double((long long)ld_agent(&rec[mc.off + q].stab));
                sub += (uint32_t)w;
                ps += (uint32_t)(w >> 32);
                pst = pst + s;
            }
            const int32_t num = (int32_t)sub, psi = (int32_t)ps;
            const bool me = p != 0 && (kc == 0 || num > psi || (num == psi && st >= pst));
            self[c] = me;
            if (num_sat) num_sat[c - 1] = num;
            if (prop_sat) prop_sat[c - 1] = psi;
            if (prop_stab) prop_stab[c - 1] = pst;
            if (p == 0) break;  // a root hands nothing on
            st_agent(&rec[mc.slot].cnt, (unsigned long long)sub | ((unsigned long long)(me ? sub : ps) << 32));
            st_agent(&rec[mc.slot].stab, (unsigned long long)__double_as_longlong(me ? st : pst));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the record has left before the counter moves
            const int32_t before = __hip_atomic_fetch_add(&arrive[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the add has returned before any record is loaded
            if (before != pn - 1) break;                      // a sibling arrives later and goes on
            c = p;
        }
    }
}

// pointer jumping: {up, best} per cluster, best = the topmost self-chosen cluster among the
// 2^r clusters from c upwards that the pair covers (0: none), up = the first cluster above them
__global__ void cs_jump_init(const int32_t *__restrict__ anc0, const int32_t *__restrict__ self, int32_t K,
                             unsigned long long *__restrict__ jp) {
    HDB_GRID_STRIDE(i, (int64_t)K + 1) {
        const uint32_t up = (uint32_t)anc0[i], best = i > 0 && self[i] ? (uint32_t)i : 0u;
        jp[i] = (unsigned long long)up << 32 | best;
    }
}

__global__ void cs_jump(const unsigned long long *__restrict__ prev, unsigned long long *__restrict__ next, int32_t K) {
    HDB_GRID_STRIDE(i, (int64_t)K + 1) {
        const unsigned long long a = prev[i];
        const uint32_t up = (uint32_t)(a >> 32);
        const unsigned long long b = prev[up];  // entry 0 is {0, 0}
        const uint32_t best = (uint32_t)b ? (uint32_t)b : (uint32_t)a;
        next[i] = (b >> 32) << 32 | best;
    }
}

// sort keys of the selected clusters (top == the cluster itself): (min_id, label) ascending
__global__ __launch_bounds__(CS_TB) void cs_sel_keys(const unsigned long long *__restrict__ jp,
                                                    const int32_t *__restrict__ min_id, int32_t K,
                                                    unsigned long long *__restrict__ key, int32_t *__restrict__ val,
                                                    int32_t *__restrict__ top, int32_t *__restrict__ count) {
    const int64_t per = (int64_t)gridDim.x * CS_TB;
    for (int64_t base = (int64_t)blockIdx.x * CS_TB; base < K; base += per) {  // uniform per workgroup
        const int64_t i = base + threadIdx.x;
        int sel = 0;
        if (i < K) {
            const int32_t c = (int32_t)i + 1, t = (int32_t)(uint32_t)jp[c];
            top[c] = t;
            sel = t == c;
            key[i] = sel ? (unsigned long long)((uint32_t)min_id[i] ^ 0x80000000u) << 32 | (uint32_t)c : ~0ull;
            val[i] = c;
        }
        const int cnt = __syncthreads_count(sel);
        if (threadIdx.x == 0 && cnt) atomicAdd(count, cnt);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) top[0] = 0;
}

__global__ void cs_number(const unsigned long long *__restrict__ skey, const int32_t *__restrict__ sval, int32_t K,
                          int32_t *__restrict__ flab, int32_t *__restrict__ flat_label) {
    HDB_GRID_STRIDE(r, K) {
        const int32_t c = sval[r];  // a permutation of 1..K
        const int32_t f = skey[r] != ~0ull ? (int32_t)r + 1 : 0;
        flab[c] = f;
        if (flat_label) flat_label[c - 1] = f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) flab[0] = 0;
}

__global__ void cs_labels(const int32_t *__restrict__ point_cluster, int64_t n, int32_t K,
                          const int32_t *__restrict__ top, const int32_t *__restrict__ flab,
                          int32_t *__restrict__ labels, int *__restrict__ err) {
    int e = 0;
    HDB_GRID_STRIDE(x, n) {
        int32_t c = point_cluster[x];
        if (c < 1 || c > K) e = CE_POINT, c = 0;
        if (labels) labels[x] = flab[top[c]];  // top[0] = flab[0] = 0
    }
    cs_flag(err, e);
}

}  // namespace

void constrained_flat_labels_device(hdb_ctx *ctx, const int32_t *parent, const double *stability,
                                    const int32_t *min_id, int64_t K, const int32_t *point_cluster, int64_t n,
                                    const int32_t *ca, const int32_t *cb, const int32_t *ctype, int64_t m,
                                    const ConstrainedOut &o) {
    if (m > HDB_MAX_CONSTRAINTS) HDB_THROW(HDB_EINVAL, "constrained flat labels: m exceeds 2^30 - 1 constraints");
    if (K < 0 || n < 0 || m < 0) HDB_THROW(HDB_EINVAL, "bad arguments");
    if (K >= (int64_t(1) << 30)) HDB_THROW(HDB_EINVAL, "constrained flat labels: too many clusters");
    if (n > INT32_MAX) HDB_THROW(HDB_EINVAL, "constrained flat labels: too many points");
    hipStream_t st = ctx->stream;
    if (o.n_clusters) *o.n_clusters = 0;
    if (K == 0) {  // no tree (n == 0): nothing to select, every point is noise
        if (o.labels && n > 0) HIP_CHECK(hipMemsetAsync(o.labels, 0, sizeof(int32_t) * (size_t)n, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    KernelTimer tt(ctx, "constrained_flat_labels");
    int J = 1;
    while ((int64_t(1) << J) < K) J++;  // 2^J >= K > the deepest chain
    const int64_t stride = K + 1;
    // temporary memory, sized once from K (n and m are only read): one zero-filled block first
    int32_t *zero = nullptr, *nch = nullptr, *arrive = nullptr, *anc = nullptr, *dep[2] = {}, *off = nullptr,
            *kids = nullptr, *sval = nullptr, *self = nullptr, *top = nullptr, *flab = nullptr, *val1 = nullptr,
            *val2 = nullptr;
    uint32_t *diff = nullptr, *virt = nullptr, *skey1 = nullptr, *skey2 = nullptr;
    unsigned long long *jp[2] = {}, *key1 = nullptr, *key2 = nullptr;
    CRec *rec = nullptr;
    CMeta *meta = nullptr;
    int32_t *pnch = nullptr;
    size_t zero_bytes = 0;
    carve(ctx, A_FLAT1, [&](Carver &cv) {
        zero = cv.take<int32_t>(64);  // [0] error bits, [1] selected clusters
        nch = cv.take<int32_t>(stride);
        arrive = cv.take<int32_t>(stride);
        diff = cv.take<uint32_t>(stride);
        virt = cv.take<uint32_t>(stride);
        zero_bytes = cv.off;
        anc = cv.take<int32_t>(stride * J);
        dep[0] = cv.take<int32_t>(stride), dep[1] = cv.take<int32_t>(stride);
        off = cv.take<int32_t>(stride);
        skey1 = cv.take<uint32_t>(K), skey2 = cv.take<uint32_t>(K);
        sval = cv.take<int32_t>(K), kids = cv.take<int32_t>(K);
        rec = cv.take<CRec>(stride);
        meta = cv.take<CMeta>(stride);
        pnch = cv.take<int32_t>(stride);
        self = cv.take<int32_t>(stride), top = cv.take<int32_t>(stride), flab = cv.take<int32_t>(stride);
        jp[0] = cv.take<unsigned long long>(stride), jp[1] = cv.take<unsigned long long>(stride);
        key1 = cv.take<unsigned long long>(K), key2 = cv.take<unsigned long long>(K);
        val1 = cv.take<int32_t>(K), val2 = cv.take<int32_t>(K);
    });
    int *err = zero;
    int32_t *count = zero + 1;
    HIP_CHECK(hipMemsetAsync(zero, 0, zero_bytes, st));
    const int32_t K32 = (int32_t)K;
    const int gk = grid_for(stride);
    // 1. validated parents, child counts, ancestor table and depths (the parts are timed under
    // names of their own, inside the call's span "constrained_flat_labels")
    std::optional<KernelTimer> part;
    auto next_part = [&](const char *name) {
        part.reset();
        if (name) part.emplace(ctx, name);
    };
    next_part("cfl_tables");
    hipLaunchKernelGGL(cs_init, dim3(gk), dim3(CS_TB), 0, st, parent, K32, anc, dep[0], nch, skey1, sval, err);
    for (int j = 1; j <= J; j++)  // the table needs J rows; the depths one more doubling (2^J steps)
        hipLaunchKernelGGL(cs_double, dim3(gk), dim3(CS_TB), 0, st, anc + (j - 1) * stride,
                           j < J ? anc + j * stride : (int32_t *)jp[0], dep[(j - 1) & 1], dep[j & 1], K32);
    const int32_t *depth = dep[J & 1];
    // 2. the constraints
    next_part("cfl_constraints");
    if (m > 0)
        hipLaunchKernelGGL(cs_constraints, dim3(grid_for(m)), dim3(CS_TB), 0, st, anc, depth, K32, J, point_cluster,
                           n, ca, cb, ctype, m, diff, virt, err);
    // 3. children lists in ascending label: stable sort by parent, offsets by an exclusive scan
    next_part("cfl_children");
    {
        int kb = 1;
        while ((int64_t(1) << kb) <= K) kb++;
        // (both take A_FLAT_TMP in turn; the arena only grows, so from the second call on neither request moves it)
        sort_pairs(ctx, A_FLAT_TMP, skey1, skey2, sval, kids, K, 0, kb);
        exclusive_sum(ctx, A_FLAT_TMP, nch, off, stride);
        hipLaunchKernelGGL(cs_meta, dim3(grid_for(K)), dim3(CS_TB), 0, st, anc, nch, off, kids, K32, meta, pnch);
    }
    // 4. the bottom-up pass, one launch: at most one workgroup per CU
    next_part("cfl_climb");
    const int gc = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(K, CS_TB), ctx->num_cus));
    hipLaunchKernelGGL(cs_climb, dim3(gc), dim3(CS_TB), 0, st, meta, pnch, diff, virt, stability, K32, rec,
                       arrive, self, o.num_sat, o.prop_sat, o.prop_stability);
    // 5. topmost self-chosen cluster per chain, numbering, labels
    next_part("cfl_select");
    hipLaunchKernelGGL(cs_jump_init, dim3(gk), dim3(CS_TB), 0, st, anc, self, K32, jp[0]);
    for (int j = 0; j < J; j++)
        hipLaunchKernelGGL(cs_jump, dim3(gk), dim3(CS_TB), 0, st, jp[j & 1], jp[(j + 1) & 1], K32);
    hipLaunchKernelGGL(cs_sel_keys, dim3(grid_for(K)), dim3(CS_TB), 0, st, jp[J & 1], min_id, K32, key1, val1, top,
                       count);
    sort_pairs(ctx, A_FLAT_TMP, key1, key2, val1, val2, K, 0, 64);
    hipLaunchKernelGGL(cs_number, dim3(grid_for(K)), dim3(CS_TB), 0, st, key2, val2, K32, flab, o.flat_label);
    next_part("cfl_labels");
    if (n > 0)
        hipLaunchKernelGGL(cs_labels, dim3(grid_for(n)), dim3(CS_TB), 0, st, point_cluster, n, K32, top, flab, o.labels,
                           err);
    next_part(nullptr);
    HIP_CHECK(hipGetLastError());
    int64_t *pin = pinned_words(ctx) + PINNED_WORDS - 8;
    HIP_CHECK(hipMemcpyAsync(pin, zero, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int e = (int)(pin[0] & 0xffffffff);
    if (e & CE_ROOT) HDB_THROW(HDB_EINVAL, "constrained flat labels: parent: the root (label 1) must have parent 0");
    if (e & CE_PARENT) HDB_THROW(HDB_EINVAL, "constrained flat labels: parent label out of range");
    if (e & CE_POINT) HDB_THROW(HDB_EINVAL, "constrained flat labels: point_cluster out of range");
    if (e & CE_ID) HDB_THROW(HDB_EINVAL, "constrained flat labels: constraint point id out of range (ca / cb)");
    if (e & CE_TYPE) HDB_THROW(HDB_EINVAL, "constrained flat labels: ctype is neither must-link (0) nor cannot-link (1)");
    if (o.n_clusters) *o.n_clusters = (int64_t)(pin[0] >> 32);
}

}  // namespace hdb
