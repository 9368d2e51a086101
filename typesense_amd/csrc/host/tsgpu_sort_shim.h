// tsgpu_sort_shim.h — maps one of the reference's sort_by objects onto a tsgpu_sort_by, creating the device key an `_eval` slot needs, and drops that key
// again when the request is done (RAII). Header-only, written against the reference's types through a template parameter, like the other shims:
//     SortBy: members  name (std::string), order (std::string, "ASC"/"DESC" in any case), missing_values (an enum whose values are named
//             first / last / normal: sort_by::missing_values_t, include/field.h), and eval with eval_ids_vec (std::vector<uint32_t*>),
//             eval_ids_count_vec (std::vector<uint32_t>), scores (std::vector<int64_t>)                      (sort_by::eval_t)
// The call site classifies the slot the way Index::compute_sort_scores does through its sentinels (src/index.cpp:5722-5761) and passes that class in:
//     SortSlotClass::text_match / seq_id / int64_column / string_column / eval / vector_query; anything else (geo, decay, random, reference sorts,
//     _group_found) is not mapped: map_sort_slot returns TSGPU_ERR_UNSUPPORTED and the caller keeps its CPU body.
// vector_query (sort_by::vector_query.query.values is set, src/index.cpp:5837; sort_vector_query_t, include/field.h:544): SortBy additionally has
//     vector_query.query with values (std::vector<float>) and distance_threshold (float)                        (vector_query_t, include/vector_query_ops.h)
//     and `column` carries the tsgpu vector field the call site mirrors vector_query.vector_index into. The key is created with
//     tsgpu_sort_key_create_vector_query (which normalises the values for a cosine field) and dropped by the guard like an `_eval` key.
//     A SortBy type without that member (older call sites) maps the class to TSGPU_ERR_UNSUPPORTED.
// Kinds (include/tsgpu.h): int64 column + missing_values first -> TSGPU_SORT_INT64_COLUMN_MISSING_FIRST, last / normal -> TSGPU_SORT_INT64_COLUMN;
// string column -> TSGPU_SORT_STRING_RANK_FLIP exactly when (asc and first) or (desc and last) (:5750-5760), else TSGPU_SORT_STRING_RANK.
#pragma once
#include <cctype>
#include <cstdint>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../../include/tsgpu.h"

namespace tsgpu {

enum class SortSlotClass { text_match, seq_id, int64_column, string_column, eval, vector_query };

// owns the sort keys created for ONE request: destroyed with it (after the last search_across_fields pass that names them has returned)
class SortKeyGuard {
public:
    explicit SortKeyGuard(tsgpu_ctx* ctx) : ctx_(ctx) {}
    SortKeyGuard(const SortKeyGuard&) = delete;
    SortKeyGuard& operator=(const SortKeyGuard&) = delete;
    ~SortKeyGuard() { release(); }
    void adopt(uint16_t handle) { handles_.push_back(handle); }
    void release() {
        for (uint16_t h : handles_) (void)tsgpu_sort_key_destroy(ctx_, h);
        handles_.clear();
    }
    size_t size() const { return handles_.size(); }
    tsgpu_ctx* ctx() const { return ctx_; }
private:
    tsgpu_ctx* ctx_;
    std::vector<uint16_t> handles_;
};

inline bool sort_order_is_asc(const std::string& order) {
    return order.size() == 3 && std::toupper((unsigned char)order[0]) == 'A' && std::toupper((unsigned char)order[1]) == 'S' && std::toupper((unsigned char)order[2]) == 'C';
}

// `_vector_query(...)`: sf.vector_query.query -> a device key on vector field vec_field_id + TSGPU_SORT_VECTOR_QUERY
template <class SortBy>
auto map_vector_query_slot(const SortBy& sf, uint32_t vec_field_id, SortKeyGuard& guard, tsgpu_sort_by* out, int) -> decltype(sf.vector_query.query.values.data(), int()) {
    const auto& vq = sf.vector_query.query;
    if (vq.values.empty()) return TSGPU_ERR_INVALID;       // (the slot is a vector-query slot only when the values are set)
    uint16_t handle = 0;
    const int rc = tsgpu_sort_key_create_vector_query(guard.ctx(), vec_field_id, vq.values.data(), vq.distance_threshold, &handle);
    if (rc != TSGPU_OK) return rc;                          // (404: the field is not mirrored; 507: every handle is live — the caller keeps its CPU body)
    guard.adopt(handle);
    out->kind = TSGPU_SORT_VECTOR_QUERY;
    out->column = handle;
    return TSGPU_OK;
}
template <class SortBy>
int map_vector_query_slot(const SortBy&, uint32_t, SortKeyGuard&, tsgpu_sort_by*, long) { return TSGPU_ERR_UNSUPPORTED; }      // SortBy has no vector_query member

// column: the tsgpu column the call site mirrors this field into (sort_index[name] as int64 values, or str_sort_index[name]->rank() values with
// INT64_MAX for a document without a value); ignored for the other classes. Returns a tsgpu_status.
template <class SortBy>
int map_sort_slot(const SortBy& sf, SortSlotClass cls, uint16_t column, SortKeyGuard& guard, tsgpu_sort_by* out) {
    using MV = decltype(sf.missing_values);
    const bool asc = sort_order_is_asc(sf.order);
    out->order = asc ? -1 : 1;
    out->column = 0;
    switch (cls) {
        case SortSlotClass::text_match: out->kind = TSGPU_SORT_TEXT_MATCH; return TSGPU_OK;
        case SortSlotClass::seq_id: out->kind = TSGPU_SORT_SEQ_ID; return TSGPU_OK;
        case SortSlotClass::int64_column:
            out->kind = sf.missing_values == MV::first ? TSGPU_SORT_INT64_COLUMN_MISSING_FIRST : TSGPU_SORT_INT64_COLUMN;
            out->column = column;
            return TSGPU_OK;
        case SortSlotClass::string_column: {
            const bool flip = (asc && sf.missing_values == MV::first) || (!asc && sf.missing_values == MV::last);
            out->kind = flip ? TSGPU_SORT_STRING_RANK_FLIP : TSGPU_SORT_STRING_RANK;
            out->column = column;
            return TSGPU_OK;
        }
        case SortSlotClass::eval: {
            const size_t n = sf.eval.eval_ids_vec.size();
            if (sf.eval.eval_ids_count_vec.size() != n || sf.eval.scores.size() != n) return TSGPU_ERR_INVALID;      // (:5766-5768)
            if (n < 1 || n > 255) return TSGPU_ERR_UNSUPPORTED;
            std::vector<const uint32_t*> ids(sf.eval.eval_ids_vec.begin(), sf.eval.eval_ids_vec.end());
            uint16_t handle = 0;
            const int rc = tsgpu_sort_key_create_eval(guard.ctx(), ids.data(), sf.eval.eval_ids_count_vec.data(), sf.eval.scores.data(), (uint32_t)n, &handle);
            if (rc != TSGPU_OK) return rc;          // (507: every handle is live — the caller keeps its CPU body)
            guard.adopt(handle);
            out->kind = TSGPU_SORT_EVAL;
            out->column = handle;
            return TSGPU_OK;
        }
        case SortSlotClass::vector_query: return map_vector_query_slot(sf, (uint32_t)column, guard, out, 0);
    }
    return TSGPU_ERR_UNSUPPORTED;
}

}  // namespace tsgpu
