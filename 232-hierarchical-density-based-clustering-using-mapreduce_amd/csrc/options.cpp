// options.cpp -- runtime options of a context: the option table, hdb_ctx_set_option and the
// HDB_OPTS parser.  No HIP runtime call: host programs link this file without a device.
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "internal.hpp"

using namespace hdb;

namespace {

// One row per option: the field it sets (defaults: hdb_ctx, common.hpp) and the values it accepts,
// lo <= v <= hi and, where the set has holes, ok(v).  A value goes to the field's type by
// static_cast, so any non-zero value switches a bool on.  Options without a range here are checked
// where they are used (boruvka_wave_pts, boruvka_early_pts: boruvka_carve).
struct Option {
    const char *name;
    void (*set)(hdb_ctx &, int64_t);
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    bool (*ok)(int64_t) = nullptr;
};

template <auto Field>
void set(hdb_ctx &c, int64_t v) {
    c.*Field = static_cast<std::remove_reference_t<decltype(c.*Field)>>(v);
}
// the one option stored negated
void set_fp32_screen(hdb_ctx &c, int64_t v) { c.force_fp64 = v == 0; }

const Option OPTIONS[] = {
    {"knn_fp32_screen", set_fp32_screen},
    {"knn_tree", set<&hdb_ctx::knn_tree>},
    {"knn_mfma", set<&hdb_ctx::knn_mfma>},
    {"nearest_grouped", set<&hdb_ctx::nearest_grouped>},
    {"knn_mfma_prune", set<&hdb_ctx::knn_mfma_prune>},
    {"knn_mfma_single", set<&hdb_ctx::knn_mfma_single>},
    {"knn_mfma_min_n", set<&hdb_ctx::knn_mfma_min_n>},
    {"knn_tree_min_n", set<&hdb_ctx::knn_tree_min_n>},
    {"prim_coop_plain", set<&hdb_ctx::prim_coop_plain>},
    {"bubble_fold_dim", set<&hdb_ctx::bubble_fold_dim>},
    {"bubble_knn_split", set<&hdb_ctx::bubble_knn_split>},
    {"prim_coop_xcd", set<&hdb_ctx::prim_coop_xcd>},
    {"prim_coop_plain_spin_log2", set<&hdb_ctx::prim_coop_plain_spin_log2>, 0, 24},
    {"prim_coop", set<&hdb_ctx::prim_coop>},
    {"prim_coop_bs", set<&hdb_ctx::prim_coop_bs>, 0, 1024,
     [](int64_t v) { return v == 0 || (v >= 128 && (v & (v - 1)) == 0); }},  // 0, 128, 256, 512, 1024
    {"prim_coop_slots", set<&hdb_ctx::prim_coop_slots>, 0, 4, [](int64_t v) { return v == 0 || v == 4; }},
    {"leaf_seed_k", set<&hdb_ctx::leaf_seed_k>, -1, 31},
    {"leaf_list_rounds", set<&hdb_ctx::leaf_list_rounds>, 0, INT64_MAX},
    {"boruvka_seed", set<&hdb_ctx::boruvka_seed>},
    {"trav_pop_test", set<&hdb_ctx::trav_pop_test>},
    {"bor_xcd_chunks", set<&hdb_ctx::bor_xcd_chunks>, 0, 4096},
    {"k1t_xcd_chunks", set<&hdb_ctx::k1t_xcd_chunks>, 0, 4096},
    {"boruvka_adj_seed", set<&hdb_ctx::boruvka_adj_seed>},
    {"boruvka_wave_pts", set<&hdb_ctx::boruvka_wave_pts>},
    {"boruvka_early_pts", set<&hdb_ctx::boruvka_early_pts>},
    {"boruvka_early_rounds", set<&hdb_ctx::boruvka_early_rounds>},
    {"boruvka_knn_seed", set<&hdb_ctx::boruvka_knn_seed>},
    {"flat_mid_log", set<&hdb_ctx::flat_mid_log>, 0, 24},
    {"flat_block_log", set<&hdb_ctx::flat_block_log>, 0, 10, [](int64_t v) { return v == 0 || v >= 8; }},
    {"flat_root_variant", set<&hdb_ctx::flat_root_variant>, 0, 5},
    {"flat_deep_root", set<&hdb_ctx::flat_deep_root>, 0, 5},
    {"flat_link_variant", set<&hdb_ctx::flat_link_variant>, 0, 1},
    {"flat_deep_link", set<&hdb_ctx::flat_deep_link>, 0, 1},
    {"flat_deep_depth", set<&hdb_ctx::flat_deep_depth>, 0, 64},
    {"flat_relabel", set<&hdb_ctx::flat_relabel>},
    {"ssort", set<&hdb_ctx::ssort>},
    {"ssort_cap", set<&hdb_ctx::ssort_cap>, 0, 4096},
    {"count_evals", set<&hdb_ctx::count_evals>},
};

}  // namespace

namespace hdb {

// "name=value,name=value" through hdb_ctx_set_option; the first pair that is malformed or
// rejected ends it with that status and names the pair in last_error()
int apply_opts(hdb_ctx *c, const char *opts) {
    const std::string s(opts);
    for (size_t a = 0; a < s.size();) {
        const size_t b = std::min(s.find(',', a), s.size());
        const std::string pair = s.substr(a, b - a);
        a = b + 1;
        if (pair.empty()) continue;
        const size_t eq = pair.find('=');
        char *end = nullptr;
        errno = 0;
        const long long v = eq == std::string::npos ? 0 : strtoll(pair.c_str() + eq + 1, &end, 10);
        if (eq == std::string::npos || eq == 0 || end == pair.c_str() + eq + 1 || *end != '\0' || errno == ERANGE) {
            set_error("malformed pair '" + pair + "' (name=integer)");
            return HDB_EINVAL;
        }
        set_error("");
        const int rc = hdb_ctx_set_option(c, pair.substr(0, eq).c_str(), (int64_t)v);
        if (rc != HDB_OK) {
            const std::string why = last_error();
            set_error("'" + pair + "' rejected" + (why.empty() ? std::string(" (value out of range)") : ": " + why));
            return rc;
        }
    }
    return HDB_OK;
}

}  // namespace hdb

// an out-of-range value sets no message: apply_opts tells it from an unknown name by that
extern "C" int hdb_ctx_set_option(hdb_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return HDB_EINVAL;
    return entry([&]() -> int {
        for (const Option &o : OPTIONS) {
            if (std::strcmp(o.name, name) != 0) continue;
            if (value < o.lo || value > o.hi || (o.ok && !o.ok(value))) return HDB_EINVAL;
            o.set(*ctx, value);
            return HDB_OK;
        }
        HDB_THROW(HDB_EINVAL, std::string("unknown option ") + name);
    });
}
