// kw_plan_policy.h — the keyword planner's POLICY, once: how a batch's driver lists are cut into work items, in which order the items are
// launched and when a query's partial lists are merged in two levels. plan_batch() (tsgpu.hip, host) and the kernels of kw_plan.hip.h (device)
// both call these functions; included after kw_kernels.hip.h (KW_SEL_PMAX). Every constant below was measured on the 10M-document collection;
// the numbers stay with the rule they justify.
//
// The rules for SMALL batches take the batch's size as an argument. The device planner is built for the large batches of the server and has
// never applied them: it passes KW_POLICY_LARGE_BATCH, the host planner passes n_queries.
#pragma once

namespace tsgpu {

static const uint32_t KW_POLICY_LARGE_BATCH = 0xFFFFFFFFu;
static const uint32_t KW_POLICY_WILDCARD_CHUNK = 64;   // blocks of ids per work item of a wildcard scan (16K ids)
static const uint32_t KW_MERGE_GROUP = 8;            // partial lists folded by one workgroup of kw_merge_groups_kernel

// Driver blocks per work item of the whole batch, from the sum of the queries' driver blocks (a multi-field driver block counts a quarter, see
// plan_batch): a few thousand work items (>= 3 per resident workgroup slot) without fragmenting the queries into more partial top-K lists than needed.
// A small batch is as slow as its longest work item, and with the selecting merge (kw_select_partials) the merge no longer grows with the number of
// partial lists: cut finer (16 queries 0.256 -> 0.223 ms, 64 queries 0.330 -> 0.305 ms; from 256 queries on the chip is full and coarser items win again).
__host__ __device__ inline uint32_t kw_policy_batch_chunk(unsigned long long total_driver_blocks, uint32_t max_chunk, uint32_t n_queries, uint32_t merge_select_min) {
    if (merge_select_min && n_queries <= 128) return 8;
    const unsigned long long c = total_driver_blocks / 3000;
    uint32_t chunk = 16;
    while (chunk < max_chunk && (unsigned long long)chunk * 2 <= c) chunk *= 2;
    return chunk;
}

// Partial top-K lists a query may have: kw_merge_kernel folds them one after the other, and a small batch (batch chunk 16) would otherwise cut a
// long driver list into hundreds of work items (a few thousand work items fill the chip, more only lengthen the per-query merge chain: 100 queries
// 1.47 -> 1.15 ms, while a cap of 8 at 1 000+ queries unbalances the search kernel).
// Below 512 queries the batch is as slow as its heaviest query: its longest work item (~3 us per driver block when the chip is not full) plus the chain
// of partial folds (~4.5 us each); with the two-level merge a chain of P folds costs G + P / G, G = 8: the two balance at ~sqrt(2.7 x blocks) items.
// Up to 128 queries the selecting merge takes whatever it can hold (see the batch chunk).
__host__ __device__ inline uint32_t kw_policy_max_partials(uint32_t max_partials_opt, uint32_t driver_blocks, uint32_t n_queries, uint32_t merge_select_min) {
    uint32_t mp = max_partials_opt;
    if (n_queries < 512) {
        const uint32_t bal = (uint32_t)sqrt((double)driver_blocks * 2.7);
        const uint32_t capped = bal < 384u ? bal : 384u;
        mp = mp > capped ? mp : capped;
    }
    if (merge_select_min && n_queries <= 128) mp = (uint32_t)KW_SEL_PMAX;
    return mp;
}

// Driver blocks per work item of ONE query: the batch chunk, or longer so that the query stays within max_partials items — but never longer than 256
// blocks (only the batch chunk of a very large batch goes beyond, up to KW_MAX_CHUNK): the batch is as slow as its longest work item (a 16K-block
// driver list cut in 16 would run 1 000 blocks in sequence), and folding 64 sorted partials costs kw_merge_kernel ~0.3 ms. A chunk fixed by option
// kw_chunk_blocks (auto_chunk false) is taken as it is.
__host__ __device__ inline uint32_t kw_policy_query_chunk(uint32_t batch_chunk, bool auto_chunk, uint32_t driver_blocks, uint32_t max_partials) {
    if (!auto_chunk) return batch_chunk;
    const uint32_t per = (driver_blocks + max_partials - 1) / max_partials;
    const uint32_t capped = per < 256u ? per : 256u;
    return batch_chunk > capped ? batch_chunk : capped;
}

__host__ __device__ inline uint32_t kw_policy_item_count(uint32_t driver_blocks, uint32_t chunk) { return driver_blocks ? (driver_blocks + chunk - 1) / chunk : 0; }

// Merge sources of a query: its work items' lists, or — more than 2 x 8 of them — group lists of 8 folded in parallel first. With the selecting merge
// (kw_select_partials: cost independent of their number) no groups up to its capacity; beyond it the lists are folded in two levels as before.
__host__ __device__ inline bool kw_policy_needs_merge_groups(uint32_t n_items, uint32_t merge_select_min) {
    if (n_items <= 2 * KW_MERGE_GROUP) return false;
    return !(merge_select_min && n_items >= merge_select_min && n_items <= (uint32_t)KW_SEL_PMAX);
}

// Launch-order key: estimated cost of the query's LARGEST work item = driver blocks x (fixed cost + second-list ids per driver id, at most 64 + third-list
// probes: every stage-1 survivor, 256 |B| / N per driver block, costs a two-level global binary search). The tables are laid out heaviest first, so that
// the long items do not start last (tail of the launch). F: double on the host, float on the device, as each planner has always computed it.
template <class F>
__host__ __device__ inline F kw_policy_item_cost(uint32_t chunk, uint32_t driver_blocks, uint32_t n_lists, uint32_t len_driver, uint32_t len_second, uint32_t num_docs,
                                                 F cost_fixed, F cost_r, F cost_probe) {
    F r = n_lists >= 2 ? (F)len_second / (F)(len_driver ? len_driver : 1u) : (F)0;
    r = r < (F)64 ? r : (F)64;
    const F surv = n_lists >= 3 ? (F)256 * (F)len_second / (F)(num_docs ? num_docs : 1u) : (F)0;
    return (F)(chunk < driver_blocks ? chunk : driver_blocks) * (cost_fixed + cost_r * r + cost_probe * surv);
}

}  // namespace tsgpu
