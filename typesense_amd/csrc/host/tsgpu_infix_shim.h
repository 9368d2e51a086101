// tsgpu_infix_shim.h — the patch body for the field loop of the reference's Index::do_infix_search (src/index.cpp:6144-6272, reached from Index::search at
// :4019) when the index and the infix fields' vocabularies are mirrored in a tsgpu context.
//
// Written against the reference's own types through template parameters, like tsgpu_keyword_shim.h:
//     KV              : KV(uint16_t query_index, uint64_t key, uint64_t distinct_key, int8_t match_score_index, const int64_t* scores)
//                       + members scores[3], text_match_score, vector_distance           (include/topster.h:20-47)
//     TopsterT        : int add(KV*) — keeps the greater of two KVs with one key        (include/topster.h:321)
//     SearchedQueries : push_back({})                                                   (std::vector<std::vector<art_leaf*>>)
// Contract kept from the reference, per field IN FIELD ORDER: a field runs when its setting is `always`, or `fallback` while all_result_ids_len == 0 AT THAT
// MOMENT (:6174) — an earlier field's infix ids switch a later fallback field off; its KVs carry query_index = searched_queries.size() (:6243); the ids that
// survived exclusion and filter are or_scalar-ed into all_result_ids (:6256-6260: a new array, the old one delete[]d); searched_queries grows by one iff the
// union of the matching tokens' lists was not empty (:6183, :6266). A field that is not an infix field answers 400 (:3270-3273). group_limit != 0 is not
// covered: 501, nothing touched, the server keeps its own loop. A query that is already late (408) sets search_cutoff and the loop goes on to the next
// field. Any other status of a field's query (501: a sort slot the device does not serve) is
// returned at once; fields before it have been applied, as in the reference, whose loop returns from the middle too.
#pragma once
#include <cstdint>
#include <vector>
#include "../../../include/tsgpu.h"

namespace tsgpu {

enum class InfixMode : uint8_t { off = 0, always = 1, fallback = 2 };          // enable_t of the field's infix setting in this search (include/field.h)

struct InfixShimField { uint32_t field_id; InfixMode mode; };

struct InfixShimArgs {
    tsgpu_ctx* ctx = nullptr;
    std::vector<InfixShimField> fields;          // the_fields with infixes[field_id], in order
    const uint8_t* pattern = nullptr;            // query_tokens[0].value
    uint32_t pattern_len = 0;
    uint32_t max_extra_prefix = 32767, max_extra_suffix = 32767;
    uint32_t n_sort = 0;
    tsgpu_sort_by sort[TSGPU_MAX_SORT_KEYS]{};
    uint32_t topster_size = 0;
    const uint32_t* excluded_ids = nullptr; uint32_t n_excluded = 0;     // curated_ids_sorted
    const uint32_t* filter_ids = nullptr; uint32_t n_filter = 0;         // NULL: no filter
    uint64_t deadline_us = 0;
    size_t group_limit = 0;
};

template <class KV, class TopsterT, class SearchedQueries>
int do_infix_search_gpu(const InfixShimArgs& a, TopsterT* topster, uint32_t*& all_result_ids, size_t& all_result_ids_len, SearchedQueries& searched_queries,
                        bool& search_cutoff) {
    if (a.group_limit != 0) return TSGPU_ERR_UNSUPPORTED;
    const uint32_t K = a.topster_size ? a.topster_size : TSGPU_DEFAULT_TOPSTER_SIZE;
    std::vector<uint64_t> keys(K);
    std::vector<int64_t> scores((size_t)K * 3), text_match(K);
    std::vector<float> vdist(K);
    std::vector<int8_t> msi(K);
    for (const InfixShimField& f : a.fields) {
        if (!(f.mode == InfixMode::always || (f.mode == InfixMode::fallback && all_result_ids_len == 0))) continue;
        tsgpu_infix_query q{};
        q.field_id = f.field_id;
        q.pattern = a.pattern; q.pattern_len = a.pattern_len;
        q.max_extra_prefix = a.max_extra_prefix; q.max_extra_suffix = a.max_extra_suffix;
        q.n_sort = a.n_sort;
        for (uint32_t s = 0; s < a.n_sort && s < TSGPU_MAX_SORT_KEYS; s++) q.sort[s] = a.sort[s];
        q.topster_size = K;
        q.excluded_ids = a.excluded_ids; q.n_excluded = a.n_excluded;
        q.filter_ids = a.filter_ids; q.n_filter = a.n_filter;
        q.deadline_us = a.deadline_us;
        uint32_t n_hits = 0;
        uint64_t num_matched = 0, n_infix_ids = 0;
        int32_t status = 0, cutoff = 0;
        tsgpu_hits h;
        h.mem = TSGPU_MEM_HOST; h.k_stride = K;
        h.keys = keys.data(); h.scores = scores.data(); h.text_match = text_match.data(); h.vector_distance = vdist.data(); h.match_score_index = msi.data();
        h.n_hits = &n_hits; h.num_matched = &num_matched; h.status = &status; h.search_cutoff = &cutoff;
        tsgpu_id_lists* ids = nullptr;
        const int rc = tsgpu_infix_search_batch(a.ctx, &q, 1, &h, nullptr, &n_infix_ids, &ids);
        if (rc != TSGPU_OK) return rc;
        search_cutoff = search_cutoff || cutoff != 0;
        if (status == TSGPU_ERR_DEADLINE) { tsgpu_id_lists_free(ids); search_cutoff = true; continue; }      // out of time: search_cutoff is set and the loop carries on, like the reference
        if (status != TSGPU_OK) { tsgpu_id_lists_free(ids); return status; }
        if (n_infix_ids == 0) { tsgpu_id_lists_free(ids); continue; }                  // :6183: nothing else happens
        const uint16_t query_index = (uint16_t)searched_queries.size();
        for (uint32_t i = 0; i < n_hits && topster != nullptr; i++) {
            KV kv(query_index, keys[i], keys[i], msi[i], &scores[(size_t)i * 3]);
            kv.text_match_score = text_match[i];
            kv.vector_distance = vdist[i];
            topster->add(&kv);
        }
        const uint64_t n = tsgpu_id_lists_count(ids, 0);
        if (n) {                                                                       // ArrayUtils::or_scalar: both ascending, the result a new array
            const uint32_t* p = tsgpu_id_lists_ids(ids, 0);
            uint32_t* merged = new uint32_t[all_result_ids_len + n];
            size_t i = 0, j = 0, o = 0;
            while (i < all_result_ids_len && j < n) {
                if (all_result_ids[i] < p[j]) merged[o++] = all_result_ids[i++];
                else if (p[j] < all_result_ids[i]) merged[o++] = p[j++];
                else { merged[o++] = p[j++]; i++; }
            }
            while (i < all_result_ids_len) merged[o++] = all_result_ids[i++];
            while (j < n) merged[o++] = p[j++];
            delete[] all_result_ids;
            all_result_ids = merged;
            all_result_ids_len = o;
        }
        tsgpu_id_lists_free(ids);
        searched_queries.push_back({});
    }
    return TSGPU_OK;
}

}  // namespace tsgpu
