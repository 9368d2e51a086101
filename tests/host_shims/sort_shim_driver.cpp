// Compiles typesense_amd/csrc/host/tsgpu_sort_shim.h against a mock of the reference's sort_by (same member names) and runs it on the library
// given on the link line: kinds, orders and the key guard's lifetime. Prints "ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../typesense_amd/csrc/host/tsgpu_sort_shim.h"

struct mock_sort_by {
    enum missing_values_t { first, last, normal };
    struct eval_t { std::vector<uint32_t*> eval_ids_vec; std::vector<uint32_t> eval_ids_count_vec; std::vector<int64_t> scores; };
    std::string name, order;
    missing_values_t missing_values = normal;
    eval_t eval;
};

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, tsgpu_last_error()); return 1; } } while (0)

static uint64_t live(tsgpu_ctx* ctx) { uint64_t v = ~0ull; tsgpu_get_counter(ctx, "sort_keys_live", &v); return v; }

int main() {
    tsgpu_ctx* ctx = nullptr;
    CHECK(tsgpu_create(0, &ctx) == TSGPU_OK);
    CHECK(tsgpu_set_num_docs(ctx, 100) == TSGPU_OK);
    using tsgpu::SortSlotClass;
    {
        tsgpu::SortKeyGuard guard(ctx);
        tsgpu_sort_by s{};
        mock_sort_by tm; tm.order = "DESC";
        CHECK(tsgpu::map_sort_slot(tm, SortSlotClass::text_match, 0, guard, &s) == TSGPU_OK && s.kind == TSGPU_SORT_TEXT_MATCH && s.order == 1);
        mock_sort_by num; num.order = "asc"; num.missing_values = mock_sort_by::first;
        CHECK(tsgpu::map_sort_slot(num, SortSlotClass::int64_column, 3, guard, &s) == TSGPU_OK && s.kind == TSGPU_SORT_INT64_COLUMN_MISSING_FIRST && s.order == -1 && s.column == 3);
        num.missing_values = mock_sort_by::last;
        CHECK(tsgpu::map_sort_slot(num, SortSlotClass::int64_column, 3, guard, &s) == TSGPU_OK && s.kind == TSGPU_SORT_INT64_COLUMN);
        num.missing_values = mock_sort_by::normal;
        CHECK(tsgpu::map_sort_slot(num, SortSlotClass::int64_column, 3, guard, &s) == TSGPU_OK && s.kind == TSGPU_SORT_INT64_COLUMN);
        const struct { const char* order; mock_sort_by::missing_values_t mv; int kind; } str_cases[] = {
            {"ASC", mock_sort_by::first, TSGPU_SORT_STRING_RANK_FLIP}, {"ASC", mock_sort_by::last, TSGPU_SORT_STRING_RANK}, {"ASC", mock_sort_by::normal, TSGPU_SORT_STRING_RANK},
            {"DESC", mock_sort_by::first, TSGPU_SORT_STRING_RANK}, {"DESC", mock_sort_by::last, TSGPU_SORT_STRING_RANK_FLIP}, {"DESC", mock_sort_by::normal, TSGPU_SORT_STRING_RANK}};
        for (const auto& c : str_cases) {
            mock_sort_by st; st.order = c.order; st.missing_values = c.mv;
            CHECK(tsgpu::map_sort_slot(st, SortSlotClass::string_column, 7, guard, &s) == TSGPU_OK && s.kind == c.kind && s.column == 7);
        }
        CHECK(guard.size() == 0 && live(ctx) == 0);
        uint32_t a[] = {1, 5, 9}, b[] = {2, 5};
        mock_sort_by ev; ev.order = "DESC";
        ev.eval.eval_ids_vec = {a, b, nullptr}; ev.eval.eval_ids_count_vec = {3, 2, 0}; ev.eval.scores = {10, -4, 7};
        CHECK(tsgpu::map_sort_slot(ev, SortSlotClass::eval, 0, guard, &s) == TSGPU_OK && s.kind == TSGPU_SORT_EVAL && s.order == 1);
        CHECK(guard.size() == 1 && live(ctx) == 1);
        tsgpu_sort_by s2{};
        CHECK(tsgpu::map_sort_slot(ev, SortSlotClass::eval, 0, guard, &s2) == TSGPU_OK && s2.column != s.column && live(ctx) == 2);
        ev.eval.scores.pop_back();
        CHECK(tsgpu::map_sort_slot(ev, SortSlotClass::eval, 0, guard, &s2) == TSGPU_ERR_INVALID && live(ctx) == 2);       // counts do not match (:5766-5768)
    }
    CHECK(live(ctx) == 0);                      // the guard dropped its keys
    tsgpu_destroy(ctx);
    std::puts("ok");
    return 0;
}
