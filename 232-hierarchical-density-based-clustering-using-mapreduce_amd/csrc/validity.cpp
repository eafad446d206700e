// validity.cpp -- the host epilogue of hdb_validity_index (validity.hip): the real-exponent
// power of the all-points core distance, which the contract pins to the host libm, and the
// per-cluster validity and the index, which it pins to one summation order.
#include <cmath>

#include "internal.hpp"

namespace hdb {

// cores[pos] = total == 0 ? 0 : pow(total / (n_c - 1), -1 / d) for the members of clusters
// 1 .. K laid out at off[c] .. off[c + 1]; may run in place.  A total of +inf gives 0.0 as computed.
void validity_cores_host(const double *totals, const int64_t *off, int32_t K, int d, double *cores) {
    const double ex = -1.0 / d;
    for (int32_t c = 1; c <= K; c++) {
        const int64_t nc = off[c + 1] - off[c];
        const double m = (double)(nc - 1);
        for (int64_t q = off[c]; q < off[c + 1]; q++) {
            const double total = totals[q];
            cores[q] = (nc <= 1 || total == 0.0) ? 0.0 : std::pow(total / m, ex);
        }
    }
}

// validity[c] = (separation - sparseness) / max(separation, sparseness), 0 for an empty cluster,
// an infinite separation or a zero maximum; index = the sum in ascending label order of
// (n_c / n) * validity[c]
void validity_finish_host(ValidityResult &r, int64_t n) {
    double index = 0.0;
    for (size_t c = 0; c < r.validity.size(); c++) {
        const double sep = r.separation[c], sp = r.sparseness[c];
        const double mx = sep > sp ? sep : sp;
        double v = 0.0;
        if (r.size[c] > 0 && sep != INFINITY && mx != 0.0) v = (sep - sp) / mx;
        r.validity[c] = v;
        index = index + ((double)r.size[c] / (double)n) * v;
    }
    r.index = index;
}

}  // namespace hdb
