// Compiles typesense_amd/csrc/host/tsgpu_phrase_shim.h against small mocks of the reference's KV / Topster / searched_queries and runs do_phrase_search and
// handle_exclusion on the library given on the link line. Five documents over two plain fields (the titles of PhraseSearch, test/collection_specific_test.cpp:2515-2519,
// and a second field). Prints "ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "../../typesense_amd/csrc/host/tsgpu_phrase_shim.h"

struct MockKV {
    uint16_t query_index; uint64_t key, distinct_key; int8_t match_score_index; int64_t scores[3]; int64_t text_match_score = 0; float vector_distance = -1.0f;
    MockKV(uint16_t qi, uint64_t k, uint64_t dk, int8_t msi, const int64_t* s) : query_index(qi), key(k), distinct_key(dk), match_score_index(msi) { memcpy(scores, s, sizeof scores); }
};
struct MockTopster {
    std::map<uint64_t, MockKV> kvs;
    int add(MockKV* kv) { kvs.erase(kv->key); kvs.emplace(kv->key, *kv); return 1; }
};
typedef std::vector<std::vector<void*>> MockSearchedQueries;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, tsgpu_last_error()); return 1; } } while (0)

// tokens: then 1, and 2, there 3, by 4, the 5, down 6, train 7, state 8, trooper 9; 50: no list
enum { THEN = 1, AND, THERE, BY, THE, DOWN, TRAIN, STATE, TROOPER, NONE = 50 };

// what Index::tokenize_string + posting_t::upsert leave per (field, token): positions + 1, a trailing 0 for the field's last token (src/index.cpp:1323-1348)
static int load_field(tsgpu_ctx* ctx, uint32_t field, const std::vector<std::vector<uint32_t>>& docs) {
    std::map<uint32_t, std::map<uint32_t, std::vector<uint32_t>>> lists;       // term -> doc -> offsets
    for (uint32_t d = 0; d < docs.size(); d++)
        for (uint32_t p = 0; p < docs[d].size(); p++) lists[docs[d][p]][d].push_back(p + 1);
    for (uint32_t d = 0; d < docs.size(); d++) if (!docs[d].empty()) lists[docs[d].back()][d].push_back(0);
    for (auto& tl : lists) {
        std::vector<uint32_t> ids, oi, off;
        for (auto& dl : tl.second) { ids.push_back(dl.first); oi.push_back((uint32_t)off.size()); off.insert(off.end(), dl.second.begin(), dl.second.end()); }
        if (int rc = tsgpu_term_upsert(ctx, field, tl.first, ids.data(), oi.data(), off.data(), (uint32_t)ids.size(), (uint32_t)off.size())) return rc;
    }
    return TSGPU_OK;
}

struct Run { MockTopster top; uint32_t* all = nullptr; size_t len = 0; MockSearchedQueries sq; bool cutoff = false; std::vector<uint32_t> filter; ~Run() { delete[] all; } };

static tsgpu::PhraseShimArgs args(tsgpu_ctx* ctx, std::vector<tsgpu::PhraseShimField> fields) {
    tsgpu::PhraseShimArgs a;
    a.ctx = ctx; a.fields = fields;
    a.n_sort = 2; a.sort[0] = {TSGPU_SORT_TEXT_MATCH, 1, 0}; a.sort[1] = {TSGPU_SORT_SEQ_ID, 1, 0};
    return a;
}
static int search(Run& r, const tsgpu::PhraseShimArgs& a) { return tsgpu::do_phrase_search_gpu<MockKV>(a, &r.top, r.all, r.len, r.sq, r.cutoff, r.filter); }

int main() {
    tsgpu_ctx* ctx = nullptr;
    CHECK(tsgpu_create(0, &ctx) == TSGPU_OK);
    for (uint32_t f = 0; f < 2; f++) CHECK(tsgpu_field_create(ctx, f, 0) == TSGPU_OK);
    CHECK(load_field(ctx, 0, {{THEN, AND, THERE, BY, THE, DOWN}, {DOWN, THERE, BY, THE, TRAIN}, {THE, STATE, TROOPER}, {BY, STATE, THE}, {}}) == TSGPU_OK);
    CHECK(load_field(ctx, 1, {{}, {}, {BY, THE}, {}, {THERE, BY, THE}}) == TSGPU_OK);
    int64_t points[5] = {0, 10, 20, 30, 40};
    CHECK(tsgpu_column_set(ctx, 0, points, nullptr, 5, TSGPU_MEM_HOST) == TSGPU_OK && tsgpu_set_num_docs(ctx, 5) == TSGPU_OK);
    CHECK(tsgpu_commit(ctx) == TSGPU_OK);

    {   // a query of phrases only over two fields: ranked, the greater field weight wins, all_result_ids replaced, searched_queries grows by one
        Run r;
        r.all = new uint32_t[2]{1, 3}; r.len = 2; r.sq.push_back({});
        CHECK(search(r, args(ctx, {{0, 3, {{BY, THE}}}, {1, 9, {{BY, THE}}}})) == TSGPU_OK);
        CHECK(r.sq.size() == 2 && r.len == 4 && r.all[0] == 0 && r.all[1] == 1 && r.all[2] == 2 && r.all[3] == 4);
        CHECK(r.top.kvs.size() == 4 && r.top.kvs.at(0).scores[0] == 100003 && r.top.kvs.at(2).scores[0] == 100009 && r.top.kvs.at(4).text_match_score == 100009);
        CHECK(r.top.kvs.at(1).query_index == 1 && r.top.kvs.at(1).match_score_index == 0 && r.top.kvs.at(1).vector_distance == -1.0f && r.top.kvs.at(1).scores[1] == 1);
    }
    {   // two phrases of a field are ANDed; a phrase with an unknown token is skipped; nothing found: searched_queries still grows, all_result_ids is emptied
        Run r;
        CHECK(search(r, args(ctx, {{0, 1, {{BY, THE}, {BY, NONE}, {THEN, AND}}}})) == TSGPU_OK);
        CHECK(r.len == 1 && r.all[0] == 0 && r.sq.size() == 1);
        Run e;
        e.all = new uint32_t[1]{2}; e.len = 1;
        CHECK(search(e, args(ctx, {{0, 1, {{TRAIN, BY, THE}}}})) == TSGPU_OK);
        CHECK(e.len == 0 && e.sq.size() == 1 && e.top.kvs.empty());
    }
    {   // excluded ids and a filter
        Run r;
        tsgpu::PhraseShimArgs a = args(ctx, {{0, 1, {{BY, THE}}}});
        const uint32_t ex[1] = {0}, fl[3] = {0, 1, 2};
        a.excluded_ids = ex; a.n_excluded = 1; a.filter_ids = fl; a.n_filter = 3;
        CHECK(search(r, a) == TSGPU_OK && r.len == 1 && r.all[0] == 1 && r.top.kvs.size() == 1);
    }
    {   // phrases + ordinary tokens: no ranking, the ids are the keyword search's filter; an empty result is an empty filter
        Run r;
        r.all = new uint32_t[1]{3}; r.len = 1;
        tsgpu::PhraseShimArgs a = args(ctx, {{0, 1, {{BY, THE}}}});
        a.is_wildcard_query = false;
        CHECK(search(r, a) == TSGPU_OK && r.filter.size() == 2 && r.filter[0] == 0 && r.filter[1] == 1 && r.len == 1 && r.sq.empty() && r.top.kvs.empty());
        a.fields[0].phrases = {{THE, BY}};
        CHECK(search(r, a) == TSGPU_OK && r.filter.empty());
    }
    {   // handle_exclusion: a phrase, a single token and a phrase with an unknown token over two fields, merged into the ids that were there
        uint32_t* ex = new uint32_t[1]{3};
        size_t n = 1;
        CHECK(tsgpu::handle_exclusion_gpu(args(ctx, {{0, 0, {{BY, THE, DOWN}, {TROOPER}, {BY, NONE}}}, {1, 0, {{THERE, BY}}}}), ex, n) == TSGPU_OK);
        CHECK(n == 4 && ex[0] == 0 && ex[1] == 2 && ex[2] == 3 && ex[3] == 4);
        delete[] ex;
    }
    {   // group_limit != 0: 501 and nothing touched; an unknown field: 400; a deadline in the past: search_cutoff, nothing else
        Run r;
        tsgpu::PhraseShimArgs a = args(ctx, {{0, 1, {{BY, THE}}}});
        a.group_limit = 3;
        CHECK(search(r, a) == TSGPU_ERR_UNSUPPORTED && r.sq.empty() && r.len == 0 && r.top.kvs.empty());
        CHECK(search(r, args(ctx, {{7, 1, {{BY, THE}}}})) == TSGPU_ERR_INVALID && r.sq.empty());
        a.group_limit = 0; a.deadline_us = 1;
        CHECK(search(r, a) == TSGPU_OK && r.cutoff && r.sq.empty() && r.len == 0 && r.top.kvs.empty());
        std::vector<std::vector<uint32_t>> nine(TSGPU_MAX_PHRASES + 1, std::vector<uint32_t>{BY, THE});
        CHECK(search(r, args(ctx, {{0, 1, nine}})) == TSGPU_ERR_UNSUPPORTED);
    }
    tsgpu_destroy(ctx);
    std::puts("ok");
    return 0;
}
