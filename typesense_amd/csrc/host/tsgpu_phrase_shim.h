// tsgpu_phrase_shim.h — the patch bodies for the reference's Index::do_phrase_search (src/index.cpp:5909-6086) and Index::handle_exclusion (:6274-6324) when
// the index is mirrored in a tsgpu context. Both field loops travel in ONE tsgpu_phrase_search_batch call each (the batch call carries the fields, their
// phrases and their weights); what stays here is what the reference does around them.
//
// Written against the reference's own types through template parameters, like tsgpu_infix_shim.h:
//     KV              : KV(uint16_t query_index, uint64_t key, uint64_t distinct_key, int8_t match_score_index, const int64_t* scores)
//                       + members scores[3], text_match_score, vector_distance           (include/topster.h:20-47)
//     TopsterT        : int add(KV*)                                                    (include/topster.h:321)
//     SearchedQueries : push_back({})                                                   (std::vector<std::vector<art_leaf*>>)
// Contract kept from the reference:
//   do_phrase_search_gpu   is_wildcard_query (the query holds phrases only): every surviving id is ranked, the KVs carry query_index = searched_queries.size()
//                          (:6070), all_result_ids BECOMES the surviving ids (to_filter_id_array, :6035: a new array, the old one delete[]d) and searched_queries
//                          grows by one, hits or not (:6084). Otherwise (:6028-6032) nothing of that happens: phrase_filter_ids receives the ids, the filter of the
//                          keyword search that follows (an EMPTY vector is a filter that matches nothing, never "no filter"). filter_ids == NULL: no filter_by.
//   handle_exclusion_gpu   the ids of every excluded phrase whose tokens all exist are or_scalar-ed into exclude_token_ids (:6300-6320: a new array).
// group_limit != 0 is not covered: 501, nothing touched, the server keeps its own loop. A query that is already late (408) sets search_cutoff and leaves
// everything else alone. Any other status is returned.
#pragma once
#include <cstdint>
#include <vector>
#include "../../../include/tsgpu.h"

namespace tsgpu {

struct PhraseShimField {
    uint32_t field_id; int32_t weight;
    std::vector<std::vector<uint32_t>> phrases;          // q_phrases (do_phrase_search) or q_exclude_tokens (handle_exclusion) as term ids; an unknown token: any id without a list
};

struct PhraseShimArgs {
    tsgpu_ctx* ctx = nullptr;
    std::vector<PhraseShimField> fields;         // search_fields, in order
    uint32_t n_sort = 0;
    tsgpu_sort_by sort[TSGPU_MAX_SORT_KEYS]{};
    uint32_t topster_size = 0;
    const uint32_t* excluded_ids = nullptr; uint32_t n_excluded = 0;     // excluded_result_ids
    const uint32_t* filter_ids = nullptr; uint32_t n_filter = 0;         // NULL: no filter
    uint64_t deadline_us = 0;
    size_t group_limit = 0;
    bool is_wildcard_query = true;
};

inline int phrase_shim_fill(const PhraseShimArgs& a, uint32_t mode, tsgpu_phrase_query& q) {
    q = tsgpu_phrase_query{};
    q.mode = mode;
    if (a.fields.size() > TSGPU_MAX_PHRASE_FIELDS) return TSGPU_ERR_UNSUPPORTED;
    q.n_fields = (uint32_t)a.fields.size();
    for (size_t f = 0; f < a.fields.size(); f++) {
        q.field_ids[f] = a.fields[f].field_id; q.field_weights[f] = a.fields[f].weight;
        if (a.fields[f].phrases.size() > TSGPU_MAX_PHRASES) return TSGPU_ERR_UNSUPPORTED;
        q.n_phrases[f] = (uint32_t)a.fields[f].phrases.size();
        for (size_t p = 0; p < a.fields[f].phrases.size(); p++) {
            const std::vector<uint32_t>& ph = a.fields[f].phrases[p];
            if (ph.size() > TSGPU_MAX_QUERY_TOKENS) return TSGPU_ERR_UNSUPPORTED;
            q.phrases[f][p].n_tokens = (uint32_t)ph.size();
            for (size_t t = 0; t < ph.size(); t++) q.phrases[f][p].term_ids[t] = ph[t];
        }
    }
    q.n_sort = a.n_sort;
    for (uint32_t s = 0; s < a.n_sort && s < TSGPU_MAX_SORT_KEYS; s++) q.sort[s] = a.sort[s];
    q.excluded_ids = a.excluded_ids; q.n_excluded = a.n_excluded;
    q.filter_ids = a.filter_ids; q.n_filter = a.n_filter;
    q.deadline_us = a.deadline_us;
    return TSGPU_OK;
}

template <class KV, class TopsterT, class SearchedQueries>
int do_phrase_search_gpu(const PhraseShimArgs& a, TopsterT* topster, uint32_t*& all_result_ids, size_t& all_result_ids_len, SearchedQueries& searched_queries,
                         bool& search_cutoff, std::vector<uint32_t>& phrase_filter_ids) {
    if (a.group_limit != 0) return TSGPU_ERR_UNSUPPORTED;
    const uint32_t K = a.topster_size ? a.topster_size : TSGPU_DEFAULT_TOPSTER_SIZE;
    tsgpu_phrase_query q;
    int rc = phrase_shim_fill(a, a.is_wildcard_query ? TSGPU_PHRASE_RANK : TSGPU_PHRASE_IDS, q);
    if (rc != TSGPU_OK) return rc;
    q.topster_size = K;
    std::vector<uint64_t> keys(K);
    std::vector<int64_t> scores((size_t)K * 3), text_match(K);
    std::vector<float> vdist(K);
    std::vector<int8_t> msi(K);
    uint32_t n_hits = 0;
    uint64_t num_matched = 0;
    int32_t status = 0, cutoff = 0;
    tsgpu_hits h;
    h.mem = TSGPU_MEM_HOST; h.k_stride = K;
    h.keys = keys.data(); h.scores = scores.data(); h.text_match = text_match.data(); h.vector_distance = vdist.data(); h.match_score_index = msi.data();
    h.n_hits = &n_hits; h.num_matched = &num_matched; h.status = &status; h.search_cutoff = &cutoff;
    tsgpu_id_lists* ids = nullptr;
    rc = tsgpu_phrase_search_batch(a.ctx, &q, 1, &h, nullptr, &ids);
    if (rc != TSGPU_OK) return rc;
    search_cutoff = search_cutoff || cutoff != 0;
    if (status == TSGPU_ERR_DEADLINE) { tsgpu_id_lists_free(ids); search_cutoff = true; return TSGPU_OK; }
    if (status != TSGPU_OK) { tsgpu_id_lists_free(ids); return status; }
    const uint64_t n = tsgpu_id_lists_count(ids, 0);
    const uint32_t* p = n ? tsgpu_id_lists_ids(ids, 0) : nullptr;
    if (!a.is_wildcard_query) {                                        // :6028-6032
        phrase_filter_ids.assign(p, p + n);
        tsgpu_id_lists_free(ids);
        return TSGPU_OK;
    }
    const uint16_t query_index = (uint16_t)searched_queries.size();
    for (uint32_t i = 0; i < n_hits && topster != nullptr; i++) {
        KV kv(query_index, keys[i], keys[i], msi[i], &scores[(size_t)i * 3]);
        kv.text_match_score = text_match[i];
        kv.vector_distance = vdist[i];
        topster->add(&kv);
    }
    uint32_t* fresh = new uint32_t[n ? n : 1];                          // to_filter_id_array(all_result_ids), :6035
    for (uint64_t i = 0; i < n; i++) fresh[i] = p[i];
    delete[] all_result_ids;
    all_result_ids = fresh;
    all_result_ids_len = (size_t)n;
    tsgpu_id_lists_free(ids);
    searched_queries.push_back({});                                    // :6084
    return TSGPU_OK;
}

inline int handle_exclusion_gpu(const PhraseShimArgs& a, uint32_t*& exclude_token_ids, size_t& exclude_token_ids_size) {
    tsgpu_phrase_query q;
    int rc = phrase_shim_fill(a, TSGPU_PHRASE_EXCLUDE, q);
    if (rc != TSGPU_OK) return rc;
    q.deadline_us = 0;                                                 // (handle_exclusion has no circuit breaker)
    tsgpu_id_lists* ids = nullptr;
    rc = tsgpu_phrase_search_batch(a.ctx, &q, 1, nullptr, nullptr, &ids);
    if (rc != TSGPU_OK) return rc;
    const uint64_t n = tsgpu_id_lists_count(ids, 0);
    if (n) {                                                           // ArrayUtils::or_scalar: both ascending, the result a new array
        const uint32_t* p = tsgpu_id_lists_ids(ids, 0);
        uint32_t* merged = new uint32_t[exclude_token_ids_size + n];
        size_t i = 0, j = 0, o = 0;
        while (i < exclude_token_ids_size && j < n) {
            if (exclude_token_ids[i] < p[j]) merged[o++] = exclude_token_ids[i++];
            else if (p[j] < exclude_token_ids[i]) merged[o++] = p[j++];
            else { merged[o++] = p[j++]; i++; }
        }
        while (i < exclude_token_ids_size) merged[o++] = exclude_token_ids[i++];
        while (j < n) merged[o++] = p[j++];
        delete[] exclude_token_ids;
        exclude_token_ids = merged;
        exclude_token_ids_size = o;
    }
    tsgpu_id_lists_free(ids);
    return TSGPU_OK;
}

}  // namespace tsgpu
