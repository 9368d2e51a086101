// kw_plan_digest.h — TESTS ONLY (option "kw_plan_digest"): two 64-bit FNV-1a digests of a keyword batch's plan.
//
// Any valid plan gives the same hits, so the results cannot tell whether a change of the planner moved the chunking, the launch
// order or the merge grouping; these digests can. They are taken over FIELDS in a fixed order (every value fed as eight little-endian bytes), never
// over struct bytes, and over no pointer: a layout change of KwQueryDev does not move them. A query that was refused contributes its status and its
// count of work items (zero) only — its record is whatever the planner had filled in when it gave up —, and an offset enters only where the kernels
// read it (ids_out_off with work items, fbits_off of a filtered multi-field query): the parallel planner shifts the unused ones by its slices' bases.
//   cut    : per query, in query order — status, k, n_lists, n_required, the wildcard range, its list handles (per field for a multi-field query),
//            the probe order / driver and second token, its work items (field, blk_begin, blk_end, ids_out_off), m_n
//   layout : per query first_work, m_first, ids_out_off, aux_off, fbits_off, mf_index; the five table sizes, the merge groups, every table's hoff
#pragma once

namespace tsgpu {

struct KwPlanTables {                // a host-readable view of one batch's plan (the device planner's tables: read back)
    const KwQueryDev* q; const int32_t* status; uint32_t n_queries;
    const KwQueryMF* mf; const KwWorkItem* work;
    const KwMergeGroup* groups; size_t n_groups;
    size_t n_tab[5];                 // work items per table (<= 3 tokens, up to 10, multi-field <= 3, multi-field up to 10, wildcard)
    const uint64_t* hoff[4]; size_t n_hoff[4];
};

struct Fnv64 {
    uint64_t h = 0xCBF29CE484222325ull;
    void add(uint64_t v) { for (int b = 0; b < 8; b++) { h ^= (v >> (8 * b)) & 0xFFu; h *= 0x100000001B3ull; } }
};

inline void kw_plan_digests(const KwPlanTables& t, uint64_t& cut_out, uint64_t& layout_out) {
    Fnv64 cut, lay;
    for (uint32_t i = 0; i < t.n_queries; i++) {
        const KwQueryDev& q = t.q[i];
        cut.add((uint64_t)(int64_t)t.status[i]);
        if (t.status[i] != 0) { cut.add(q.n_work); continue; }
        const bool mf = q.mf_index != KW_NONE && !q.wild_n_ids;
        cut.add(q.k); cut.add(q.n_lists); cut.add(q.n_required);
        cut.add(q.wild_n_ids); cut.add(q.wild_base); cut.add(q.n_filt);
        if (mf) {
            const KwQueryMF& m = t.mf[q.mf_index];
            cut.add(m.n_fields);
            for (uint32_t l = 0; l < q.n_lists; l++) for (uint32_t f = 0; f < (uint32_t)KW_MAX_FIELDS; f++) cut.add(m.list[l][f]);
            cut.add(m.driver_token); cut.add(m.second_token);
        } else {
            for (uint32_t l = 0; l < q.n_required; l++) cut.add(q.list[l]);
            for (uint32_t l = 0; l < q.n_required; l++) cut.add(q.probe_order[l]);
        }
        cut.add(q.n_work);
        for (uint32_t c = 0; c < q.n_work; c++) {
            const KwWorkItem& w = t.work[q.first_work + c];
            cut.add(w.query >> 28); cut.add(w.blk_begin); cut.add(w.blk_end); cut.add(w.ids_out_off);
        }
        cut.add(q.m_n);
        lay.add(q.first_work); lay.add(q.m_first); lay.add(q.n_work ? q.ids_out_off : 0); lay.add(q.aux_off);
        lay.add(mf && q.n_filt ? q.fbits_off : 0); lay.add(q.mf_index);
    }
    for (int tb = 0; tb < 5; tb++) lay.add(t.n_tab[tb]);
    lay.add(t.n_groups);
    for (size_t g = 0; g < t.n_groups; g++) { lay.add(t.groups[g].query); lay.add(t.groups[g].first); lay.add(t.groups[g].n); lay.add(t.groups[g].dst); }
    for (int tb = 0; tb < 4; tb++) { lay.add(t.n_hoff[tb]); for (size_t w = 0; w < t.n_hoff[tb]; w++) lay.add(t.hoff[tb][w]); }
    cut_out = cut.h; layout_out = lay.h;
}

}  // namespace tsgpu
