// kw_translate.h — tsgpu_kw_query -> KwQueryDev / KwQueryMF, once (host; included by tsgpu.hip after kw_kernels.hip.h, used by tsgpu_groupby.inc.h too).
// The entry points (keyword / wildcard batches, group_by, aux scores, the shards' token masks) differ in WHICH checks they make and in their order —
// the first failing check decides a query's status — so the predicates and the fills live here and every caller keeps its own sequence.
#pragma once

namespace tsgpu {

inline bool kw_token_count_ok(const tsgpu_kw_query& in) { return in.n_tokens != 0 && in.n_tokens <= TSGPU_MAX_QUERY_TOKENS; }
inline bool kw_field_count_ok(const tsgpu_kw_query& in) { return in.n_fields != 0 && in.n_fields <= (uint32_t)KW_MAX_FIELDS; }
inline bool kw_dropped_count_ok(const tsgpu_kw_query& in) { return in.n_dropped <= TSGPU_MAX_DROPPED_TOKENS && in.n_tokens + in.n_dropped <= TSGPU_MAX_QUERY_TOKENS; }

// the sort slots (the caller has checked n_sort and the slots: check_sort_slots); all a wildcard query has
inline void kw_fill_sort_slots(const tsgpu_kw_query& in, KwQueryDev& q) {
    q.n_sort = (uint8_t)in.n_sort;
    for (uint32_t s = 0; s < in.n_sort; s++) { q.sort_kind[s] = in.sort[s].kind; q.sort_order[s] = in.sort[s].order; q.sort_col[s] = in.sort[s].column; }
}

// what the scoring functions read of the query itself (the kernels test the flags for non-zero only)
inline void kw_fill_scoring(const tsgpu_kw_query& in, KwQueryDev& q) {
    q.n_query_tokens = in.n_tokens;
    q.match_type = in.match_type;
    q.prio_exact = in.prioritize_exact_match ? 1 : 0; q.prio_pos = in.prioritize_token_position ? 1 : 0; q.prio_nfields = in.prioritize_num_matching_fields ? 1 : 0;
    q.total_cost = in.total_cost;
    q.weight = in.field_weights[0];
    q.syn_orig_num_tokens = (int8_t)((int)in.syn_orig_num_tokens_p1 - 1);
    q.orig_num_tokens = in.orig_num_tokens; q.is_synonym = in.is_synonym_query ? 1 : 0; q.demote_synonym = in.demote_synonym_match ? 1 : 0;
}

// the query_by fields of the multi-field form: n_fields, is_array and weight per field (0 behind the last); TSGPU_ERR_NOT_FOUND for a field the
// snapshot does not hold. any_array (nullable) is raised by a string[] field.
inline int kw_fill_fields(const Snapshot& snap, const tsgpu_kw_query& in, KwQueryMF& m, bool* any_array = nullptr) {
    m.n_fields = in.n_fields;
    for (uint32_t f = 0; f < (uint32_t)KW_MAX_FIELDS; f++) {
        m.is_array[f] = 0; m.weight[f] = 0;
        if (f >= in.n_fields) continue;
        const auto fa = snap.field_is_array.find(in.field_ids[f]);
        if (fa == snap.field_is_array.end()) return TSGPU_ERR_NOT_FOUND;
        m.is_array[f] = fa->second ? 1 : 0; m.weight[f] = in.field_weights[f];
        if (fa->second && any_array) *any_array = true;
    }
    return TSGPU_OK;
}

// One query token over the query_by fields = one or_iterator, the union of its lists (get_field_token_its, src/index.cpp:5598-5660); a token that no
// field holds gets none (:5651-5655).
struct KwTokenLists {
    uint32_t handle[KW_MAX_FIELDS];      // per field, KW_NONE = the field does not hold the token
    uint32_t first = KW_NONE;            // the first field's list that holds it (all there is with one query_by field)
    uint64_t ids = 0; uint32_t blocks = 0;      // summed over the fields
    bool found = false;
};
inline KwTokenLists kw_resolve_token(const Snapshot& snap, const tsgpu_kw_query& in, uint32_t term) {
    KwTokenLists r;
    for (uint32_t f = 0; f < (uint32_t)KW_MAX_FIELDS; f++) r.handle[f] = KW_NONE;
    for (uint32_t f = 0; f < in.n_fields && f < (uint32_t)KW_MAX_FIELDS; f++) {
        const uint32_t h = snap.find_handle(in.field_ids[f], term);
        if (h == 0xFFFFFFFFu) continue;
        if (!r.found) r.first = h;
        r.found = true; r.handle[f] = h;
        r.ids += snap.h_lists[h].n_ids; r.blocks += snap.h_lists[h].n_blocks;
    }
    return r;
}

// the multi-field form's lists of a query: its own tokens that exist, in query order, then the dropped tokens that exist (scored when the document holds
// them, never required: src/index.cpp:5271-5290) -> q.n_required / q.n_lists, m.list. The scoring-only callers (group_by, aux scores) need no more.
inline void kw_fill_token_lists(const Snapshot& snap, const tsgpu_kw_query& in, bool with_dropped, KwQueryDev& q, KwQueryMF& m) {
    uint32_t nl = 0;
    auto add_token = [&](uint32_t term) {
        const KwTokenLists tl = kw_resolve_token(snap, in, term);
        if (!tl.found) return;
        for (uint32_t f = 0; f < in.n_fields; f++) if (tl.handle[f] != KW_NONE) m.list[nl][f] = tl.handle[f];
        nl++;
    };
    for (uint32_t t = 0; t < in.n_tokens; t++) add_token(in.term_ids[t]);
    q.n_required = nl;
    for (uint32_t t = 0; with_dropped && t < in.n_dropped; t++) add_token(in.dropped_term_ids[t]);
    q.n_lists = nl;
}

}  // namespace tsgpu
