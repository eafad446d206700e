// attach_scan.hpp -- the pieces the tiled FP64 row-against-row scans share: the attach scan
// (attach.hip) and the exemplar-distance scan (soft.hip).  The tile constants, the packing pass and
// the fold / batch / finish functors, moved here from attach.hip as they were: a lane owns one query,
// candidate rows arrive wave-uniformly in tiles of ATT_CT rows, ATT_CB rows at a time, each pair's sum
// runs over the dimensions in order in chunks of ATT_DC with the running sum carried across chunks
// (bit parity with metric_distance; the header of attach.hip has the argument).  Everything sits in
// an unnamed namespace: each translation unit that includes this compiles its own copy.
#pragma once

#include "internal.hpp"

namespace hdb {

namespace {

constexpr int ATT_QT = 256;  // queries per workgroup: one per lane, four waves
constexpr int ATT_CT = 64;   // rows per candidate tile
constexpr int ATT_DC = 8;    // dimension chunk held in registers
constexpr int ATT_CB = 4;    // candidates evaluated together (one query chunk load serves all)
static_assert(ATT_CT % ATT_CB == 0, "a tile is whole batches");

enum { OP_SQ = 0, OP_ABS = 1, OP_MAX = 2, OP_DOT = 3 };

// One thread per row: the row transformed for the metric and packed to dp columns, its per-row
// term (cosine: the squared norm; Pearson: the centred squared norm), and for the training rows
// the core distance with -0.0 read as +0.0.
__global__ void att_pack_kernel(const double *__restrict__ X, int64_t n, int d, int dp, int metric,
                                const double *__restrict__ core, double *__restrict__ Xp, double *__restrict__ nrm_out,
                                double *__restrict__ core_out) {
    HDB_GRID_STRIDE(pos, n) {
        const double *a = X + pos * d;
        double *o = Xp + pos * dp;
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
        nrm_out[pos] = nrm;
        if (core_out) {
            const double c = core[pos];
            core_out[pos] = c == 0.0 ? 0.0 : c;
        }
    }
}

template <int OP>
__device__ __forceinline__ double att_fold(double acc, double a, double b) {
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

// the sums of one batch of ATT_CB candidate rows against the lane's query.  xq holds the query's
// first chunk (the whole row when nch == 1); rows past n inside the last batch are the zero rows
// of the padded copy.
template <int OP>
__device__ __forceinline__ void att_batch(double (&acc)[ATT_CB], double (&xq)[ATT_DC], const double *__restrict__ qrow,
                                          const double *__restrict__ cbase, int dp, int nch) {
#pragma unroll
    for (int u = 0; u < ATT_CB; u++) acc[u] = 0.0;
#pragma unroll 1
    for (int ch = 0; ch < nch; ch++) {
        if (nch > 1) {
#pragma unroll
            for (int i = 0; i < ATT_DC; i++) xq[i] = qrow[ch * ATT_DC + i];
        }
#pragma unroll
        for (int u = 0; u < ATT_CB; u++) {
            const double *cr = cbase + (int64_t)u * dp + ch * ATT_DC;
#pragma unroll
            for (int i = 0; i < ATT_DC; i++) acc[u] = att_fold<OP>(acc[u], xq[i], cr[i]);
        }
    }
}

// the distance and the tie key of a finished sum
template <int OP>
__device__ __forceinline__ void att_finish(double acc, double qn, double xn, double &dist, double &s) {
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

}  // namespace

}  // namespace hdb
