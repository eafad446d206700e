// sort.hpp -- stable LSD radix sorts of (key, value) pairs that always take rocprim's
// onesweep path.  rocprim's default config switches to block-sort + merge-path below 2^20
// items; for the ~1M-item sorts on the hot path (Morton order, Boruvka edge order) that
// took ~200 us per sort vs ~90-140 us for onesweep (profiles/r01).  Both are stable, so
// the results are identical.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"

namespace hdb {

using OnesweepOnly = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                rocprim::default_config, 0>;

template <class K, class V>
inline hipError_t sort_pairs(void *tmp, size_t &bytes, const K *kin, K *kout, const V *vin, V *vout, int64_t n,
                             int begin_bit, int end_bit, hipStream_t st) {
    return rocprim::radix_sort_pairs<OnesweepOnly>(tmp, bytes, kin, kout, vin, vout, (size_t)n, (unsigned)begin_bit,
                                                   (unsigned)end_bit, st);
}

template <class K, class V>
inline hipError_t sort_pairs_desc(void *tmp, size_t &bytes, const K *kin, K *kout, const V *vin, V *vout, int64_t n,
                                  int begin_bit, int end_bit, hipStream_t st) {
    return rocprim::radix_sort_pairs_desc<OnesweepOnly>(tmp, bytes, kin, kout, vin, vout, (size_t)n,
                                                        (unsigned)begin_bit, (unsigned)end_bit, st);
}

// The two-call protocol of the rocPRIM / hipCUB device primitives, written once: f(nullptr, bytes)
// reports the temp size, the arena slot supplies it, f(tmp, bytes) runs.
template <class F>
inline void with_tmp(hdb_ctx *ctx, int slot, F &&f) {
    size_t bytes = 0;
    HIP_CHECK(f((void *)nullptr, bytes));
    void *tmp = arena(ctx, slot, bytes);
    HIP_CHECK(f(tmp, bytes));
}

template <class T>
inline void exclusive_sum(hdb_ctx *ctx, int slot, const T *in, T *out, int64_t n) {
    with_tmp(ctx, slot, [&](void *tmp, size_t &b) {
        return rocprim::exclusive_scan(tmp, b, in, out, T(0), (size_t)n, rocprim::plus<T>(), ctx->stream);
    });
}

template <class K, class V>
inline void sort_pairs(hdb_ctx *ctx, int slot, const K *kin, K *kout, const V *vin, V *vout, int64_t n, int begin_bit,
                       int end_bit) {
    with_tmp(ctx, slot, [&](void *tmp, size_t &b) {
        return sort_pairs(tmp, b, kin, kout, vin, vout, n, begin_bit, end_bit, ctx->stream);
    });
}

template <class K, class V>
inline void sort_pairs_desc(hdb_ctx *ctx, int slot, const K *kin, K *kout, const V *vin, V *vout, int64_t n,
                            int begin_bit, int end_bit) {
    with_tmp(ctx, slot, [&](void *tmp, size_t &b) {
        return sort_pairs_desc(tmp, b, kin, kout, vin, vout, n, begin_bit, end_bit, ctx->stream);
    });
}

// temp bytes of sort_pairs<K, V>, for a caller that folds them into a layout of its own or sizes one
// arena for several sorts before a loop that must not grow it
template <class K, class V>
inline size_t sort_pairs_bytes(int64_t n, int begin_bit, int end_bit) {
    size_t bytes = 0;
    HIP_CHECK(sort_pairs(nullptr, bytes, (const K *)nullptr, (K *)nullptr, (const V *)nullptr, (V *)nullptr, n, begin_bit,
                         end_bit, (hipStream_t) nullptr));
    return bytes;
}

}  // namespace hdb
