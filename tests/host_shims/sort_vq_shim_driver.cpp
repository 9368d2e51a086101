// Compiles typesense_amd/csrc/host/tsgpu_sort_shim.h against a mock of the reference's sort_by WITH its vector_query member (same member names) and runs
// the `_vector_query(...)` slot class on the library given on the link line: the key is created on the mirrored vector field, a wildcard search sorted
// by it returns float_to_int64_t(dist_func(q, row)) per document (threshold and missing row included), and the guard drops the key. Prints "ok", exits 0.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../typesense_amd/csrc/host/tsgpu_sort_shim.h"

struct mock_vector_query_t { std::string field_name; float distance_threshold = FLT_MAX; std::vector<float> values; };
struct mock_sort_vector_query_t { mock_vector_query_t query; void* vector_index = nullptr; };
struct mock_sort_by {
    enum missing_values_t { first, last, normal };
    struct eval_t { std::vector<uint32_t*> eval_ids_vec; std::vector<uint32_t> eval_ids_count_vec; std::vector<int64_t> scores; };
    std::string name, order;
    missing_values_t missing_values = normal;
    eval_t eval;
    mock_sort_vector_query_t vector_query;
};
struct old_sort_by {                    // a call site compiled against a sort_by without the member
    enum missing_values_t { first, last, normal };
    struct eval_t { std::vector<uint32_t*> eval_ids_vec; std::vector<uint32_t> eval_ids_count_vec; std::vector<int64_t> scores; };
    std::string name, order;
    missing_values_t missing_values = normal;
    eval_t eval;
};

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, tsgpu_last_error()); return 1; } } while (0)

static uint64_t live(tsgpu_ctx* ctx) { uint64_t v = ~0ull; tsgpu_get_counter(ctx, "sort_keys_live", &v); return v; }
static int64_t float_to_int64(float f) {          // Index::float_to_int64_t, src/index.cpp:266-274
    int32_t i; std::memcpy(&i, &f, 4);
    if (i < 0) i ^= INT32_MAX;
    return (int64_t)i;
}

int main() {
    tsgpu_ctx* ctx = nullptr;
    CHECK(tsgpu_create(0, &ctx) == TSGPU_OK);
    const uint32_t n_docs = 5, dim = 4, FIELD = 3;
    CHECK(tsgpu_set_num_docs(ctx, n_docs) == TSGPU_OK);
    CHECK(tsgpu_commit(ctx) == TSGPU_OK);
    // documents 0..3 have a row, document 4 has none
    const float rows[4][4] = {{1, 0, 0, 0}, {0.5f, 0.5f, 0, 0}, {-1, 2, 0.25f, 0}, {0, 0, 0, 3}};
    const uint64_t labels[4] = {0, 1, 2, 3};
    CHECK(tsgpu_vec_create(ctx, FIELD, dim, TSGPU_METRIC_IP, 0) == TSGPU_OK);
    CHECK(tsgpu_vec_upsert(ctx, FIELD, labels, &rows[0][0], 4, TSGPU_MEM_HOST) == TSGPU_OK);
    using tsgpu::SortSlotClass;
    {
        tsgpu::SortKeyGuard guard(ctx);
        tsgpu_sort_by s{};
        mock_sort_by vq; vq.order = "ASC";
        vq.vector_query.query.values = {0.75f, 0.25f, 2.0f, -0.5f};
        vq.vector_query.query.distance_threshold = 1.0f;
        CHECK(tsgpu::map_sort_slot(vq, SortSlotClass::vector_query, (uint16_t)FIELD, guard, &s) == TSGPU_OK && s.kind == TSGPU_SORT_VECTOR_QUERY && s.order == -1);
        CHECK(guard.size() == 1 && live(ctx) == 1);
        // expected: ASC -> -float_to_int64_t(d), d > 1 -> FLT_MAX, no row -> 2.0f
        int64_t want[5];
        for (uint32_t d = 0; d < n_docs; d++) {
            float dist = 2.0f;
            if (d < 4) { dist = tsgpu_ip_distance(vq.vector_query.query.values.data(), rows[d], dim, 4); if (dist > 1.0f) dist = FLT_MAX; }
            want[d] = -float_to_int64(dist);
        }
        tsgpu_kw_query q;
        std::memset(&q, 0, sizeof q);
        q.n_sort = 2; q.sort[0] = s; q.sort[1].kind = TSGPU_SORT_SEQ_ID; q.sort[1].order = 1;
        uint64_t keys[8]; int64_t scores[24]; uint32_t n_hits = 0; int32_t status = -1;
        tsgpu_hits h;
        std::memset(&h, 0, sizeof h);
        h.mem = TSGPU_MEM_HOST; h.k_stride = 8; h.keys = keys; h.scores = scores; h.n_hits = &n_hits; h.status = &status;
        CHECK(tsgpu_wildcard_search_batch(ctx, &q, 1, &h) == TSGPU_OK && status == TSGPU_OK && n_hits == n_docs);
        bool seen[5] = {false, false, false, false, false};
        for (uint32_t i = 0; i < n_hits; i++) {
            CHECK(keys[i] < n_docs && !seen[keys[i]]);
            seen[keys[i]] = true;
            CHECK(scores[3 * i] == want[keys[i]] && scores[3 * i + 1] == (int64_t)keys[i]);
            CHECK(i == 0 || scores[3 * i] < scores[3 * (i - 1)] || (scores[3 * i] == scores[3 * (i - 1)] && keys[i] < keys[i - 1]));
        }
        // a second slot of the request gets a key of its own; errors create nothing
        tsgpu_sort_by s2{};
        vq.order = "desc";
        CHECK(tsgpu::map_sort_slot(vq, SortSlotClass::vector_query, (uint16_t)FIELD, guard, &s2) == TSGPU_OK && s2.column != s.column && s2.order == 1 && live(ctx) == 2);
        CHECK(tsgpu::map_sort_slot(vq, SortSlotClass::vector_query, (uint16_t)77, guard, &s2) == TSGPU_ERR_NOT_FOUND && live(ctx) == 2);      // the field is not mirrored
        vq.vector_query.query.values.clear();
        CHECK(tsgpu::map_sort_slot(vq, SortSlotClass::vector_query, (uint16_t)FIELD, guard, &s2) == TSGPU_ERR_INVALID && live(ctx) == 2);
        old_sort_by old; old.order = "ASC";
        CHECK(tsgpu::map_sort_slot(old, SortSlotClass::vector_query, (uint16_t)FIELD, guard, &s2) == TSGPU_ERR_UNSUPPORTED && live(ctx) == 2);
        CHECK(tsgpu::map_sort_slot(old, SortSlotClass::seq_id, 0, guard, &s2) == TSGPU_OK && s2.kind == TSGPU_SORT_SEQ_ID);
    }
    CHECK(live(ctx) == 0);                      // the guard dropped its keys
    tsgpu_destroy(ctx);
    std::puts("ok");
    return 0;
}
