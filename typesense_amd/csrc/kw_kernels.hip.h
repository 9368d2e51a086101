// kw_kernels.hip.h — gfx950 kernels of the keyword hot path (seam B1, include/tsgpu.h).
//
// One launch of kw_search_kernel does, for a whole batch of queries, what the reference does per query on
// one CPU thread in or_iterator_t::intersect (include/or_iterator.h:61-182) and its scoring lambda
// (src/index.cpp:5479-5551): conjunctive doc-id intersection, per-hit Match window scoring
// (include/match_score.h:129-275), score_results2 / compute_aggregated_score packing
// (src/index.cpp:6966-7098, 5227-5383), compute_sort_scores (src/index.cpp:5662-5907) and the bounded
// top-K of Topster (include/topster.h:321-473).
//
// Mapping to the machine (64-wide wavefronts, 256-thread workgroups, LDS queues):
//   * a work item = (query, range of <=CHUNK 256-id blocks of the query's SHORTEST list, the "driver");
//     one workgroup per work item, grid = all work items of the batch (>> 256 CUs);
//   * stage 0: thread t extracts id t of the driver block straight from the bit-packed payload
//     (coalesced dword loads, funnel shift) — no decode buffer, no allocation;
//   * stage 1: the 256 ascending candidates of a driver block meet the next-shortest list B as a block-level
//     MERGE, not 256 independent probes: the run of B blocks that overlaps the driver block's id range is
//     found with one coalesced 64-entry window load of blk_last[] + a wave ballot (the cursor only moves
//     forward), those B blocks are decoded cooperatively (coalesced dword loads) into an LDS id tile, and each
//     candidate finishes with two LDS binary searches (block, then slot). A window wider than 64 B blocks
//     falls back to the per-candidate probe (binary search of blk_last[], then of the packed block);
//     survivors are compacted IN ORDER with wave ballot + popcount prefix sums into an LDS queue;
//   * stage 2 (>=3 tokens): runs only when >=256 survivors are queued, so the remaining probes execute
//     with full wavefronts; survivors -> final queue;
//   * score stage: dense again (>=256 queued hits or flush): per hit, token positions are read on demand
//     from the packed offsets, the Match window runs in registers, the 64-bit text score and the
//     (<=3) sort keys are assembled and the hit is offered to an LDS top-K buffer guarded by the
//     current K-th-best threshold; the buffer is bitonic-sorted + truncated when it fills;
//   * each work item writes its sorted partial top-K; kw_merge_kernel folds the partials of a query
//     (usually 1-4) into the final Topster::sort() order.
// Text scores depend only on the document, so chunking / sharding never changes a score.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tsgpu_format.h"
#include "vec_ip_order.hip.h"      // the `_vector_query` sort slot (kw_vq_sort.hip.h) takes its distances in the k-NN paths' summation orders

#include <type_traits>

namespace tsgpu {

// TSGPU_PROF builds only (tools/): per-phase cycle accounting of kw_search_kernel (wave 0 lane 0 of every workgroup)
#ifdef TSGPU_PROF
#define KW_PROF_DECL unsigned long long prof_t[12] = {0,0,0,0,0,0,0,0,0,0,0,0}; unsigned long long prof_last = __builtin_readcyclecounter();
#define KW_PROF(i) { const unsigned long long _n = __builtin_readcyclecounter(); prof_t[i] += _n - prof_last; prof_last = _n; }
#define KW_PROF_FLUSH(ptr) if (threadIdx.x == 0 && (ptr)) { for (int _i = 0; _i < 12; _i++) atomicAdd((ptr) + _i, prof_t[_i]); atomicAdd((ptr) + 12, 1ull); }
#else
#define KW_PROF_DECL
#define KW_PROF(i)
#define KW_PROF_FLUSH(ptr)
#endif

// 4 workgroups (16 waves) per CU need <= 128 VGPRs: tell the register allocator (it lands 3 over without the hint)
#ifndef TSGPU_SCORE_WAVES
#define TSGPU_SCORE_WAVES 6      // kw_score_kernel: <= 80 VGPRs = 6 waves per SIMD (round 1: 4 -> 5 waves 2.01 -> 1.73 ms; round 4, after the PLAIN instantiation: 5 -> 6 waves 1.45 -> 1.38 ms, 7: 1.42, 8: 1.70)
#endif
#ifndef TSGPU_SCORE_MF_WAVES
#define TSGPU_SCORE_MF_WAVES 4   // kw_score_kernel<.., MF = true>: its 31.6 KB of LDS allow four workgroups per CU = four waves per SIMD whatever the registers: <= 128 VGPRs,
#endif                           // room for the six staged runs of a two-field hit (round 6; as MF ? .. : .. in the attribute: the template argument decides)
#ifdef TSGPU_HIP_EMU
#define KW_FOUR_WAVES_PER_SIMD
#define KW_SCORE_WAVES
#else
#define KW_SCORE_WAVES __attribute__((amdgpu_waves_per_eu(MF ? TSGPU_SCORE_MF_WAVES : TSGPU_SCORE_WAVES)))
#define KW_FOUR_WAVES_PER_SIMD __attribute__((amdgpu_waves_per_eu(4)))
#endif

#ifndef TSGPU_MF_STAGED
#define TSGPU_MF_STAGED 1        // multi-field score kernel (<= 3 tokens): a hit's runs loaded level by level for all tokens of a field (load_runs_staged_slots); 0 = one load_run per (token, field)
#endif
static const bool KW_MF_STAGED = TSGPU_MF_STAGED != 0;
// A UNIFORM integer the compiler may not reason about across this point ("+s": it stays in an SGPR). Loop-invariant uniform PREDICATES (T >= 3, a list's
// flag bit, ...) are hoisted out of a loop as i1 values, and a uniform i1 lives in an SGPR PAIR as a lane mask for the whole loop — in the find kernels that
// is what pushes the allocator past 102 SGPRs, and every reload of a spilled SGPR is a v_readlane on the vector ALU, the kernels' busiest port. Laundering the
// integer inside the loop makes the test a fresh s_cmp where it is used.
#ifdef TSGPU_HIP_EMU
#define KW_UNIFORM_OPAQUE(x) ((void)0)
#else
#define KW_UNIFORM_OPAQUE(x) asm volatile("" : "+s"(x))
#endif
static const int KW_THREADS = 256;
static const int KW_QCAP = 512;            // LDS queue capacity (>= 255 leftover + 256 new)
static const int KW_MAX_TOKENS = 10;       // TSGPU_MAX_QUERY_TOKENS
static const int KW_MAX_FIELDS = 4;        // query_by fields per query (tsgpu_kw_query::field_ids)
static const int KW_MAX_CANDIDATE_PASSES = 16;   // candidate-token combinations folded per user query (reference: max(10, max_candidates), src/index.cpp:1841-1842)
static const uint32_t KW_NONE = 0xFFFFFFFFu;
static const uint32_t KW_WINDOW_SIZE = 10; // WINDOW_SIZE, include/match_score.h:11
#ifndef TSGPU_KW_TILE_WORDS
#define TSGPU_KW_TILE_WORDS 2048
#endif
#ifndef TSGPU_KW_MAX_CHUNK
#define TSGPU_KW_MAX_CHUNK 512
#endif
static const int KW_MAX_CHUNK = TSGPU_KW_MAX_CHUNK;        // driver blocks per work item (host clamps kw_chunk_blocks to this)
static const int KW_PIPE_WORDS = 4;         // dwords per thread of the register-pipelined tile copy (4 x 256 words = 2048 16-bit ids)
// the find kernels (two-kernel form): two tile buffers of 7 slabs (256 words each) — with 8, the pair kernel's LDS (tile + 6 KB survivor queue +
// 2 KB window copies) is 24.4 KB = six workgroups per CU; 7 slabs = 22.4 KB = SEVEN (and <= 72 VGPRs since the multi-round path left the loop):
// find 5.04 -> 4.80 ms. Runs beyond a buffer are probed per candidate (one load where the list has an id directory).
#ifndef TSGPU_KW_FIND_PIPE_WORDS
#define TSGPU_KW_FIND_PIPE_WORDS 7
#endif
#ifndef TSGPU_KW_FIND_TILE_WORDS
#define TSGPU_KW_FIND_TILE_WORDS 3584
#endif
#ifndef TSGPU_KW_MF_TILE_WORDS
#define TSGPU_KW_MF_TILE_WORDS 2048
#endif
static const int KW_MF_TILE_WORDS = TSGPU_KW_MF_TILE_WORDS;   // the multi-field find kernel's tile: 2048 (default: 23 KB of LDS = 7 workgroups per CU, 17.5 -> 16.2 ms on the two-field bench leg; wider runs are probed), 3072 or 4096
static const int KW_FIND_PIPE_WORDS = TSGPU_KW_FIND_PIPE_WORDS;
static const int KW_FIND_TILE_WORDS = TSGPU_KW_FIND_TILE_WORDS;
static const int KW_TILE_WORDS = TSGPU_KW_TILE_WORDS;   // LDS tile of PACKED second-list ids per round (8 KB ~ 20 blocks of 12-bit ids); multiple of 256

// One `_eval(...)` sort key (tsgpu_sort_key_create_eval; compute_sort_scores, src/index.cpp:5761-5834): the id lists of its expressions in one of two forms.
// DENSE: dense[seq_id] = first matching expression + 1, 0 = none (one byte load per candidate). SPARSE (dense == nullptr): the sorted lists back to back in
// ids[], expression e = ids[expr_off[e] .. expr_off[e + 1]), probed by binary search, expression by expression. scores[e] either way.
// The same table holds the `_vector_query(...)` keys (tsgpu_sort_key_create_vector_query, form = SORT_KEY_FORM_VECTOR_QUERY; :5837-5851, kw_vq_sort.hip.h):
// the stored query and the key's vector field AS IT IS WHEN THE BATCH RUNS — a batch that names such a key rewrites the vq_ fields behind `vq_q` under
// ctx->mu before its kernels start (the row matrix may have moved, the row map been rebuilt) and holds the mutex until they have finished.
static const uint32_t SORT_KEY_FORM_EVAL = 0, SORT_KEY_FORM_VECTOR_QUERY = 1;
struct SortKeyDesc {
    const uint8_t* dense;
    const uint32_t* ids;
    const uint32_t* expr_off;        // [n_expr + 1]
    const int64_t* scores;           // [n_expr]
    uint32_t dense_len;              // bytes of dense[] (seq_ids beyond it match nothing)
    uint32_t n_expr;
    uint32_t form;                   // SORT_KEY_FORM_*; the fields above belong to the _eval form, the fields below to the vector-query form
    uint32_t vq_dim;
    const float* vq_q;               // [vq_dim] the query, normalised at creation for a cosine field (16-byte aligned)
    const float* vq_X;               // the field's rows [vq_n_rows][vq_dim]
    const uint32_t* vq_row_of_seq;   // [vq_map_len] seq_id -> row, 0xFFFFFFFF = none; nullptr: identity numbering (row = seq_id)
    const uint8_t* vq_row_ok;        // [vq_n_rows] 0 = deleted
    uint32_t vq_n_rows;
    uint32_t vq_map_len;
    float vq_threshold;              // distance_threshold (FLT_MAX = none)
    uint32_t vq_ip_lanes;            // option vec_ip_lanes when the batch started
};
static const uint32_t KW_SORT_KEY_SLOTS = 4096;     // handles of the context's key table (IndexView::sort_keys)

struct IndexView {
    const ListDesc* lists;
    const uint32_t* blk_last;
    const BlockIds* blk_ids;
    const BlockMeta* blk_meta;
    const uint32_t* ids_payload;
    const uint32_t* payload;
    const int64_t* const* columns;   // columns[c][seq_id], INT64_MIN = no value (default_score, index.cpp:5696)
    const uint32_t* column_len;
    uint32_t n_columns;
    uint32_t num_docs;
    const uint2* iddir;              // id directories of the long lists (tsgpu_format.h): slot s at iddir + s * iddir_slot_entries
    uint32_t iddir_slot_entries;     // entries per slot (= ceil(iddir_cap_ids / 32))
    uint32_t iddir_cap_ids;          // doc ids the directories cover: [0, cap)
    unsigned long long* prof;        // TSGPU_PROF builds: 13 counters; else null
    unsigned long long* touched;     // option kw_count_touched: 12 counters the COUNT instantiation of the find kernel adds its requested bytes to; else null
    const struct KwQueryMF* mf;      // multi-field queries of the batch (KwQueryDev::mf_index)
    uint32_t* fbits;                 // filtered multi-field queries: one bit per filter rank (KwQueryDev::fbits_off), zeroed per batch
    // in-flight deadline (search_cutoff, include/or_iterator.h:148-153): t0 = device wall clock when the batch started (stamped by
    // kw_stamp_kernel), ticks_per_us its rate; cutoff[query] is raised by the first work item that runs out of time
    const long long* t0;
    uint32_t ticks_per_us;
    uint32_t find_dir_span;          // kw_find2_kernel, directory-tile stage 1: the widest mean pair span (doc ids) of a work item that takes it; 0 = never (option kw_find_dir_tile)
    uint32_t* cutoff;
    const SortKeyDesc* sort_keys;    // the context's key table, KW_SORT_KEY_SLOTS entries (KwQueryDev::sort_col of a TSGPU_SORT_EVAL slot indexes it; the planner checked the handle)
};

// The kernel's IndexView argument RE-READ from the kernarg segment (s_load where it is used) instead of kept live: the find kernels use most of its
// fields only in their occasional paths (third-list probes of a drained batch, probes of wide runs, the deadline check), but hipcc loads every kernel
// argument once at entry and keeps it in SGPRs for the whole pair loop — with the loop's own state that is ~150 uniform values for 102 registers, and
// every reload of a spilled one is a v_readlane on the vector ALU. Valid only inside a __global__ function whose FIRST parameter is the IndexView.
#if defined(TSGPU_HIP_EMU) || defined(TSGPU_NO_KERNARG_RELOAD)
#define KW_RELOAD_VIEW(ix) (ix)
#else
__device__ __forceinline__ IndexView kw_reload_view_from_kernarg(const IndexView& ix) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t* KernargWords;
    KernargWords p = (KernargWords)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    union { IndexView v; uint32_t w[sizeof(IndexView) / 4]; } u;
    static_assert(sizeof(IndexView) % 4 == 0, "copied as dwords");
#pragma unroll
    for (int i = 0; i < (int)(sizeof(IndexView) / 4); i++) u.w[i] = p[i];      // (scalar loads; only the fields the caller uses survive)
    return u.v;
#else
    return ix;
#endif
}
#define KW_RELOAD_VIEW(ix) kw_reload_view_from_kernarg(ix)
#endif

struct KwQueryDev {                  // one search_across_fields call
    uint32_t n_lists;                // tokens that exist in the index (token_its.size())
    uint32_t n_query_tokens;         // query_tokens.size()
    uint32_t list[KW_MAX_TOKENS];    // list handle per found token, QUERY order (Match depends on it)
    uint8_t probe_order[KW_MAX_TOKENS + 2];  // indices into list[], ascending n_ids; [0] = driver
    uint8_t match_type, prio_exact, prio_pos, prio_nfields;
    uint32_t total_cost;
    int32_t weight;
    uint8_t n_sort;
    uint8_t sort_kind[3];
    int8_t sort_order[3];
    uint8_t pad0;
    uint16_t sort_col[3];
    uint16_t pad1;
    uint32_t k;                      // Topster capacity
    uint32_t first_work, n_work;     // this query's work items (contiguous)
    uint32_t aux_off, n_excl, n_filt;  // excluded ids then filter ids in the aux id arena
    uint64_t ids_out_off;            // where this query's matched ids go (if kept)
    uint32_t mf_index;               // KW_NONE = one query_by field; else index into IndexView::mf
    uint32_t wild_n_ids;             // wildcard query (q = "*"): ids to scan = filter ids, or every seq_id < num_docs; 0 = keyword query
    uint64_t fbits_off;              // filtered multi-field query: word offset of its rank bitmap in IndexView::fbits
    uint32_t deadline_rem_us;        // microseconds this query may still run, counted from the batch's start stamp (0 = no deadline)
    uint32_t n_required;             // lists [0, n_required) form the AND; lists [n_required, n_lists) are dropped tokens: scored when the document
                                     // holds them, never required (compute_aggregated_score, src/index.cpp:5271-5290); multi-field form only
    int8_t syn_orig_num_tokens;      // synonym passes (src/index.cpp:5292-5294, 6989-6994, 7024-7060): -1 = not one
    uint8_t orig_num_tokens, is_synonym, demote_synonym;
    uint32_t m_first, m_n;           // the sorted partial lists kw_merge_kernel folds: the work items themselves, or (many work items) the
                                     // group lists kw_merge_groups_kernel left behind them (counters always come from the work items)
    uint64_t vdist;                  // wildcard form used by the FLAT branch of the vector search (process_results_bruteforce, src/index.cpp:3345-3374,
                                     // :3675-3723): device address of float dist[wild_n_ids], entry i = exact distance of filter id i (NaN: the label has
                                     // no vector / is the query document -> skipped); 0 = a plain wildcard query
    float vdist_thr;                 // vector_query.distance_threshold (:3702)
    uint8_t vdist_abs;               // cosine field: std::abs(dist) (:3699)
    uint8_t pad2[3];
    uint32_t wild_base;              // wildcard query without filter ids on a doc-range shard (context options doc_range_lo / _hi): the ids scanned are wild_base + [0, wild_n_ids)
    uint32_t pad3;
    uint64_t wild_ids;               // wildcard query whose n_filt filter ids are ALREADY on the device (the id list the infix front expanded, kw_infix.hip.h): their
                                     // address; 0 = the filter ids follow the excluded ids in the aux arena
    uint64_t wild_tm;                // with wild_ids, the phrase front (kw_phrase.hip.h): device address of int64 tm[n_filt], the text-match value of filter id i
                                     // (do_phrase_search's phrase_match_id_scores, src/index.cpp:6050); 0 = the constant of the wildcard / flat vector forms
};

// query_by over several fields (get_field_token_its, src/index.cpp:5598-5660): token t is the UNION over the fields of its
// posting lists (or_iterator_t, src/or_iterator.cpp:95-171), the query the AND over tokens of those unions
struct KwQueryMF {
    uint32_t list[KW_MAX_TOKENS][KW_MAX_FIELDS];   // list handle of (found token t, field f) or KW_NONE
    int32_t weight[KW_MAX_FIELDS];                 // the_fields[f].weight
    uint8_t is_array[KW_MAX_FIELDS];               // field f is a string[] field
    uint32_t n_fields;
    uint32_t driver_token;                         // the token whose lists (one work item group per field) drive the scan
    uint32_t second_token;                         // the required token with the next fewest postings (KW_NONE: the query has one required token): checked
                                                   // first, for every candidate of a driver block, as a block-level MERGE through the LDS tile (kw_mf_merge_field)
};

struct KwWorkItem {
    uint32_t query;                  // multi-field work items: | driver field << 28
    uint32_t blk_begin, blk_end;     // driver-list block range
    uint32_t ids_out_off;            // offset (relative to the query's ids_out_off) of this chunk's id segment
};

struct KwPartials {                  // per work item, stride = k_stride
    int64_t* s0; int64_t* s1; int64_t* s2; int64_t* key;
    uint32_t* cnt;                   // entries written (<= k)
    uint32_t* n_match;               // num_keyword_matches contribution
    uint32_t* n_emit;                // ids emitted (after exclusion / filter)
    uint64_t* off_words;             // sum over hits of (offsets read + 1 offset_index entry) per token: algorithmic bytes / 4
    // filtered queries only (num_keyword_matches under filter-driven skipping, see kw_filter_count): matches counted if the
    // chunk's first hit is NOT counted (n_match) / IS counted (n_match1), filter rank of the first / last hit, and
    // flags = nonempty | carry_out(first not counted) << 1 | carry_out(first counted) << 2
    uint32_t* n_match1; uint32_t* first_rank; uint32_t* last_rank; uint32_t* fflags;
    uint32_t k_stride;
};

struct KwOut {                       // final, per query, stride = k_stride (tsgpu_hits layout)
    uint64_t* keys; int64_t* scores; int64_t* text_match; float* vector_distance; int8_t* match_score_index;
    uint32_t* n_hits; uint64_t* num_matched; uint64_t* off_words;
    uint32_t k_stride;
};

// The reference checks its deadline every 65 536 loop iterations and breaks out with whatever the Topster holds
// (include/or_iterator.h:148-153, RETURN_CIRCUIT_BREAKER). Here every work item looks at the device wall clock every 16 driver blocks
// (wave-uniform: one s_memrealtime + a scalar load): past the query's budget it raises the query's cutoff flag and stops scanning;
// what it found so far is scored and merged as usual, the caller gets partial hits with search_cutoff = 1.
// Workgroup-uniform: every thread of the workgroup must call it at the same point. (Each wavefront reading the clock for itself is a
// race — one wave leaves the loop, its siblings wait for it at the next barrier; the decision is taken by thread 0 and shared.)
// KNOWN = the caller has already established (outside its loop) that the query has a deadline: the per-call test of the LDS copy of the query — a
// dependent LDS round trip the compiler hoists to the top of EVERY iteration of the caller's loop — is left out
template <bool KNOWN = false>
__device__ inline bool kw_out_of_time(const IndexView& ix, const KwQueryDev& q, uint32_t query, uint32_t* s_flag) {
#ifdef TSGPU_NO_DEADLINE
    return false;
#endif
    if constexpr (!KNOWN) { if (q.deadline_rem_us == 0) return false; }      // (uniform: the query record is shared by the workgroup)
    __syncthreads();                                                // the previous decision has been read by everyone
    if (threadIdx.x == 0) {
#ifdef TSGPU_HIP_EMU
        const long long now = hipemu_wall_clock64();
#else
        const long long now = wall_clock64();
#endif
        const bool late = (unsigned long long)(now - *ix.t0) > (unsigned long long)q.deadline_rem_us * ix.ticks_per_us;
        if (late) atomicOr(&ix.cutoff[query], 1u);
        *s_flag = late ? 1u : 0u;
    }
    __syncthreads();
    return *s_flag != 0;
}
__global__ void kw_stamp_kernel(long long* t0) {
#ifdef TSGPU_HIP_EMU
    *t0 = hipemu_wall_clock64();
#else
    *t0 = wall_clock64();
#endif
}

// ------------------------------------------------------------------------------------------------
// ordered compaction: exclusive prefix of `pred` over the workgroup (wave ballot + popcount, then the
// 4 wave totals through LDS). Every thread must call it (uniform control flow).
__device__ inline uint32_t block_compact(bool pred, uint32_t* s_wave_cnt /*[4]*/, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(pred ? 1 : 0);
    const uint32_t lane_off = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();                       // protect s_wave_cnt reuse from a previous call
    if (lane == 0) s_wave_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < KW_THREADS / 64; w++) {
        const uint32_t c = s_wave_cnt[w];
        if ((uint32_t)w < wave) base += c;
        tot += c;
    }
    total = tot;
    return base + lane_off;
}

// single-barrier variant for the main loop: the caller alternates between two count arrays, so the barrier of
// call i+1 orders every read of call i before the writes of call i+2
__device__ inline uint32_t block_compact1(bool pred, uint32_t* s_wave_cnt /*[4], alternate per call*/, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(pred ? 1 : 0);
    const uint32_t lane_off = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < KW_THREADS / 64; w++) {
        const uint32_t c = s_wave_cnt[w];
        if ((uint32_t)w < wave) base += c;
        tot += c;
    }
    total = tot;
    return base + lane_off;
}

// (Also measured and rejected — profiles/r01/sweep_kw_s4_bitmap_stage1.txt: a BITMAP stage 1 for 16-bit blocks (driver block -> 64 Kbit
// LDS bitmap, the second list's prefetched ids tested against it: independent LDS reads instead of dependent search steps, the
// same number of LDS operations) ran 26.7 ms vs 19.0 ms: one more barrier per block, 151 VGPRs = 3 waves per SIMD. The loop is
// bound by LDS operation COUNT and occupancy, not by the dependency chain of the searches.)
// (Again after the two-kernel split, with registers to spare in the find kernel: a 4-ary slot search — three independent probes per
// level, four levels — ran the find kernel at 10.35 ms vs 8.92 ms for the binary search: 12 LDS reads instead of 8.)
// (16-ary versions of these searches — 16 independent probes per round instead of 4 dependent binary steps — were measured
// 1.5x SLOWER end to end: 3.5x the LDS reads and +14..16 VGPRs, i.e. 3 waves per SIMD instead of 4, cost more than the
// dependent-read latency they save; profiles/r01/prof_kw_s4_kary.txt)
// is id x in the list? -> posting position (block*256 + slot). Two binary searches, all loads are
// broadcast / same-line for neighbouring lanes because candidates ascend with the lane id.
// Lower bound of x in an ascending u32 / u16 array a[0 .. n) whose answer exists (a[n - 1] >= x), started from an INTERPOLATED guess:
// doc ids are spread roughly evenly over a list, so the answer usually lies inside a 16-entry window around
// (x - first) / (last - first) * n — one cache line. Two independent loads test the window; inside it four short steps finish the search
// (the window's cache line is hot), otherwise the half that must hold the answer is searched by plain bisection. A dependent chain of
// log2(n) long-latency loads becomes ~2 long + 4 short ones; the result is the same index whatever the data looks like.
template <class LoadFn>
__device__ inline uint32_t guided_lower_bound(uint32_t n, uint32_t x, uint32_t first, uint32_t last, LoadFn at) {
    uint32_t lo = 0, hi = n - 1;                                  // the answer is in [lo, hi]
    if (n > 16) {
        const float frac = (float)(x - first) / ((float)(last - first) + 1.0f);
        uint32_t g = (uint32_t)(frac * (float)n);
        g = g < n ? g : n - 1;
        const uint32_t wlo = g > 8 ? g - 8 : 0;
        const uint32_t whi = wlo + 15 < n - 1 ? wlo + 15 : n - 1;
        const uint32_t below = wlo ? at(wlo - 1) : 0u, top = at(whi);          // independent loads
        const bool low_ok = wlo == 0 || below < x;
        if (low_ok && top >= x) { lo = wlo; hi = whi; }
        else if (!low_ok) hi = wlo - 1;                           // a[wlo - 1] >= x: the answer is at or before it
        else lo = whi + 1;                                        // a[whi] < x
    }
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (at(mid) >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// is id x in the list? -> posting position (block*256 + slot). Two guided searches (block among the list's last ids, slot among the
// block's ids); neighbouring lanes probe ascending candidates, so their loads share cache lines.
// (COUNT: *cnt += the bytes of every load this probe issues — the counting instantiation of the find kernel, kw_find2.hip.h)
template <bool COUNT = false>
__device__ inline bool probe_list(const IndexView& ix, const ListDesc& d, uint32_t x, uint32_t& pos, uint32_t* cnt = nullptr) {
    if (x < d.first_id || x > d.last_id) return false;
    if (d.dir_slot && x < ix.iddir_cap_ids) {                  // a long list: one load answers most probes (tsgpu_format.h, ID DIRECTORY)
        if constexpr (COUNT) *cnt += 8;
        const uint2 e = ix.iddir[(size_t)(d.dir_slot - 1) * ix.iddir_slot_entries + (x >> 5)];
        const uint32_t b = x & 31u;
        if (!((e.y >> b) & 1u)) return false;
        if (!(e.x & IDDIR_SPLIT)) { pos = e.x + (uint32_t)__popc(e.y & ((1u << b) - 1u)); return true; }
    }
#ifdef TSGPU_EXP_FAKEBM                                       // tools/ experiment only (results are WRONG): what a one-load bitmap probe of dense lists would cost
    if (d.n_ids >= (1u << 18)) {
        const uint2 wv = ((const uint2*)(ix.ids_payload + d.ids_base))[(x >> 5) % (d.n_ids >> 2)];
        pos = (wv.x % (d.n_blocks - 1)) * BLOCK_IDS + ((wv.x >> 20) & 255u);
        return ((wv.y >> (x & 31)) & 1u) && ((wv.y >> ((x + 7) & 31)) & 1u);
    }
#endif
    const uint32_t* __restrict__ bl = ix.blk_last + d.blk_base;
    const uint32_t lo = guided_lower_bound(d.n_blocks, x, d.first_id, d.last_id, [&](uint32_t i) { if constexpr (COUNT) *cnt += 4; return bl[i]; });
    const BlockIds m = ix.blk_ids[d.blk_base + lo];
    if constexpr (COUNT) *cnt += 16;
    if (x < m.first_id) return false;
    const uint32_t* __restrict__ w = ix.ids_payload + d.ids_base + m.ids_woff;
    const uint32_t target = x - m.first_id;
    const bool w16 = (m.n_ids_bits >> 16) == 16;
    const uint32_t n = m.n_ids_bits & 0xFFFF;                 // ids[n - 1] = block last >= target
    const uint32_t l = guided_lower_bound(n, target, 0u, m.last_id - m.first_id, [&](uint32_t i) { if constexpr (COUNT) *cnt += w16 ? 2 : 4; return w16 ? (uint32_t)((const uint16_t*)w)[i] : w[i]; });
    if constexpr (COUNT) *cnt += w16 ? 2 : 4;
    if ((w16 ? (uint32_t)((const uint16_t*)w)[l] : w[l]) != target) return false;
    pos = lo * BLOCK_IDS + l;
    return true;
}

// probe_list in two halves, so that SEVERAL probes of one candidate (the lists of a token in every query_by field) have their first — usually
// only — load in flight together: probe_issue() requests the directory entry, probe_finish() evaluates it (and falls back to the two-level search
// for lists without a directory, split entries and ids beyond the directories' range). Same answers as probe_list.
struct ProbeReq { uint2 e; uint32_t state; };                 // state: 0 = x outside the list's id range, 1 = directory entry requested, 2 = no directory: search
__device__ inline void probe_issue(const IndexView& ix, const ListDesc& d, uint32_t x, ProbeReq& r) {
    r.e = make_uint2(0u, 0u); r.state = 0;
    if (x < d.first_id || x > d.last_id) return;
    if (d.dir_slot && x < ix.iddir_cap_ids) { r.e = ix.iddir[(size_t)(d.dir_slot - 1) * ix.iddir_slot_entries + (x >> 5)]; r.state = 1; }
    else r.state = 2;
}
// (COUNT: *cnt += the bytes of every load of the search, as probe_list counts them)
template <bool COUNT = false>
__device__ inline bool probe_search(const IndexView& ix, const ListDesc& d, uint32_t x, uint32_t& pos, uint32_t* cnt = nullptr) {     // (the two-level search of probe_list)
    const uint32_t* __restrict__ bl = ix.blk_last + d.blk_base;
    const uint32_t lo = guided_lower_bound(d.n_blocks, x, d.first_id, d.last_id, [&](uint32_t i) { if constexpr (COUNT) *cnt += 4; return bl[i]; });
    const BlockIds m = ix.blk_ids[d.blk_base + lo];
    if constexpr (COUNT) *cnt += 16;
    if (x < m.first_id) return false;
    const uint32_t* __restrict__ w = ix.ids_payload + d.ids_base + m.ids_woff;
    const uint32_t target = x - m.first_id;
    const bool w16 = (m.n_ids_bits >> 16) == 16;
    const uint32_t n = m.n_ids_bits & 0xFFFF;
    const uint32_t l = guided_lower_bound(n, target, 0u, m.last_id - m.first_id, [&](uint32_t i) { if constexpr (COUNT) *cnt += w16 ? 2 : 4; return w16 ? (uint32_t)((const uint16_t*)w)[i] : w[i]; });
    if constexpr (COUNT) *cnt += w16 ? 2 : 4;
    if ((w16 ? (uint32_t)((const uint16_t*)w)[l] : w[l]) != target) return false;
    pos = lo * BLOCK_IDS + l;
    return true;
}
// guided_lower_bound with the whole 16-entry window around the interpolated guess requested AT ONCE (17 independent loads, counted in registers)
// instead of two window tests followed by four dependent steps inside the window: one memory round trip per search level where the guided form
// takes 2 long + 4 short ones. TSGPU_PROF, kw_find_mf2_kernel on the two-field bench leg: a 256-survivor stage-2 batch took ~25 000 cycles, almost
// all of it the dependent chain of the ONE probe per survivor that has no directory behind it (the driver token's list in the other field: a short
// list) — two search levels x (2 + 4) loads + the block record + the final compare. Same index on any data (the fallback bisection is the guided form's).
template <class LoadFn>
__device__ inline uint32_t wide_lower_bound(uint32_t n, uint32_t x, uint32_t first, uint32_t last, LoadFn at) {
    uint32_t lo = 0, hi = n - 1;                                  // the answer is in [lo, hi] (a[n - 1] >= x)
    const float frac = (float)(x - first) / ((float)(last - first) + 1.0f);
    uint32_t g = (uint32_t)(frac * (float)n);
    g = g < n ? g : n - 1;
    const uint32_t w0 = g > 8 ? g - 8 : 0;
    const uint32_t whi = w0 + 15 < n - 1 ? w0 + 15 : n - 1;
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = at(w0 + (uint32_t)i < n - 1 ? w0 + (uint32_t)i : n - 1);
    const uint32_t below = w0 ? at(w0 - 1) : 0u;
    const bool low_ok = w0 == 0 || below < x;
    if (low_ok && v[15] >= x) {                                   // (v[15] = a[whi]; slots past the array's end repeat a[n - 1] >= x: they count 0)
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) c += v[i] < x ? 1u : 0u;
        return w0 + c;
    }
    if (!low_ok) hi = w0 - 1; else lo = whi + 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (at(mid) >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ inline bool probe_search_wide(const IndexView& ix, const ListDesc& d, uint32_t x, uint32_t& pos) {
    const uint32_t* __restrict__ bl = ix.blk_last + d.blk_base;
    const uint32_t lo = wide_lower_bound(d.n_blocks, x, d.first_id, d.last_id, [&](uint32_t i) { return bl[i]; });
    const BlockIds m = ix.blk_ids[d.blk_base + lo];
    if (x < m.first_id) return false;
    const uint32_t* __restrict__ w = ix.ids_payload + d.ids_base + m.ids_woff;
    const uint32_t target = x - m.first_id;
    const bool w16 = (m.n_ids_bits >> 16) == 16;
    const uint32_t n = m.n_ids_bits & 0xFFFF;
    const uint32_t l = wide_lower_bound(n, target, 0u, m.last_id - m.first_id, [&](uint32_t i) { return w16 ? (uint32_t)((const uint16_t*)w)[i] : w[i]; });
    if ((w16 ? (uint32_t)((const uint16_t*)w)[l] : w[l]) != target) return false;
    pos = lo * BLOCK_IDS + l;
    return true;
}
template <bool WIDE = false>
__device__ inline bool probe_finish(const IndexView& ix, const ListDesc& d, uint32_t x, const ProbeReq& r, uint32_t& pos) {
    if (r.state == 0) return false;
    if (r.state == 1) {
        const uint32_t b = x & 31u;
        if (!((r.e.y >> b) & 1u)) return false;
        if (!(r.e.x & IDDIR_SPLIT)) { pos = r.e.x + (uint32_t)__popc(r.e.y & ((1u << b) - 1u)); return true; }
    }
    if constexpr (WIDE) return probe_search_wide(ix, d, x, pos);
    else return probe_search(ix, d, x, pos);
}

// LIST TABLE (kw_find2_kernel, kw_score_kernel): what a work item needs of its query's ListDesc records, one compact row per token in LDS, filled
// once per work item next to the copy of the query (before the kernel's first barrier). A probe / a run load through ix.lists[q.list[tok]] re-reads
// per-query constants from global memory every time — the handle comes out of LDS, so the compiler keeps it per lane: vector loads of one address by
// 64 lanes, each a dependent round trip in front of the load that matters (profiles/r12/exp_list_table.txt). TSGPU_LIST_TABLE=0 restores the
// descriptor loads (tools/ A/B builds only; same results).
#ifndef TSGPU_LIST_TABLE
#define TSGPU_LIST_TABLE 1
#endif
static const bool KW_LIST_TABLE = TSGPU_LIST_TABLE != 0;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(TSGPU_HIP_EMU)
#define KW_GLOBAL_AS __attribute__((address_space(1)))       // a pointer into global memory: global_load (vmcnt only), not flat_load (vmcnt AND lgkmcnt)
#define KW_UNIFORM32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))      // a value every lane holds alike: into an SGPR
#else
#define KW_GLOBAL_AS
#define KW_UNIFORM32(x) ((uint32_t)(x))
#endif
// find kernel: the range test and the directory probe of one list. dir = index of the list's first directory entry in IndexView::iddir, KW_NO_DIR = none
struct alignas(16) KwProbeRow { uint32_t first_id, last_id, dir_lo, dir_hi; };
static const unsigned long long KW_NO_DIR = ~0ull;
__device__ inline KwProbeRow kw_probe_row(const IndexView& ix, const ListDesc& d) {
    const unsigned long long dir = d.dir_slot ? (unsigned long long)(d.dir_slot - 1) * ix.iddir_slot_entries : KW_NO_DIR;
    KwProbeRow r; r.first_id = d.first_id; r.last_id = d.last_id; r.dir_lo = (uint32_t)dir; r.dir_hi = (uint32_t)(dir >> 32);
    return r;
}
__device__ inline KwProbeRow kw_probe_row_none() { KwProbeRow r; r.first_id = 0xFFFFFFFFu; r.last_id = 0u; r.dir_lo = r.dir_hi = 0xFFFFFFFFu; return r; }      // (matches no id)
__device__ inline KwProbeRow kw_probe_row_uniform(const KwProbeRow* row) {          // the row of a token every lane asks about alike
    KwProbeRow r; r.first_id = KW_UNIFORM32(row->first_id); r.last_id = KW_UNIFORM32(row->last_id); r.dir_lo = KW_UNIFORM32(row->dir_lo); r.dir_hi = KW_UNIFORM32(row->dir_hi);
    return r;
}
// one directory entry: ONE 8-byte global load, requested before either word is looked at
__device__ __forceinline__ uint2 kw_dir_entry(const uint2* iddir, unsigned long long idx) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(TSGPU_HIP_EMU)
    const unsigned long long v = ((const KW_GLOBAL_AS unsigned long long*)iddir)[idx];
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
#else
    return iddir[idx];
#endif
}
// probe_issue / probe_finish / probe_list on a table row. handle = the list's handle: only the two-level search (no directory, a marked entry, an id
// beyond the directories' range) reads the descriptor itself. Same answers as probe_list.
__device__ inline void probe_row_issue(const IndexView& ix, const KwProbeRow& r, uint32_t x, ProbeReq& q) {
    q.e = make_uint2(0u, 0u); q.state = 0;
    if (x < r.first_id || x > r.last_id) return;
    const unsigned long long dir = (unsigned long long)r.dir_lo | ((unsigned long long)r.dir_hi << 32);
    if (dir != KW_NO_DIR && x < ix.iddir_cap_ids) { q.e = kw_dir_entry(ix.iddir, dir + (x >> 5)); q.state = 1; }
    else q.state = 2;
}
template <bool COUNT = false>
__device__ inline bool probe_row_finish(const IndexView& ix, uint32_t handle, uint32_t x, const ProbeReq& q, uint32_t& pos, uint32_t* cnt = nullptr) {
    if (q.state == 0) return false;
    if (q.state == 1) {
        if constexpr (COUNT) *cnt += 8;
        const uint32_t b = x & 31u;
        if (!((q.e.y >> b) & 1u)) return false;
        if (!(q.e.x & IDDIR_SPLIT)) { pos = q.e.x + (uint32_t)__popc(q.e.y & ((1u << b) - 1u)); return true; }
    }
    const ListDesc d = ix.lists[handle];
    if constexpr (COUNT) *cnt += (uint32_t)sizeof(ListDesc);
    return probe_search<COUNT>(ix, d, x, pos, cnt);
}
template <bool COUNT = false>
__device__ inline bool probe_row(const IndexView& ix, const KwProbeRow& r, uint32_t handle, uint32_t x, uint32_t& pos, uint32_t* cnt = nullptr) {
    ProbeReq q;
    probe_row_issue(ix, r, x, q);
    return probe_row_finish<COUNT>(ix, handle, x, q, pos, cnt);
}

// one token's occurrences inside one document (plain string field, src/index.cpp:1323-1348 encoding)
struct TokRun {
    const uint32_t* w;   // packed offsets of the block
    uint32_t start;      // first element of the run
    uint32_t n;          // number of POSITIONS (the trailing 0 flag excluded)
    uint32_t base;
    uint32_t raw_len;    // elements in the run (for the algorithmic byte count)
    uint32_t meta;       // bits 0..5 element width | bit 8: run ends with 0 (token is the last token of the field) | bits 16..17: nc
    // the run's first two elements, 16 bits each, fetched together with the run header: a token rarely occurs more than once or
    // twice in a document, so the Match window loop runs out of registers instead of issuing one dependent global load per step
    // (nc = elements served from c01; 0 when one of them needs more than 16 bits)
    uint32_t c01;
};
__device__ inline uint32_t run_bits(const TokRun& r) { return r.meta & 63u; }
__device__ inline uint32_t run_last_flag(const TokRun& r) { return (r.meta >> 8) & 1u; }
__device__ inline uint32_t run_raw_len(const TokRun& r) { return r.raw_len; }

__device__ inline uint32_t run_raw(const TokRun& r, uint32_t j) {
    if (j < (r.meta >> 16)) return (r.c01 >> (j * 16)) & 0xFFFFu;
    return r.base + unpack_at(r.w, r.start + j, run_bits(r));
}
// positions.push_back((uint16_t)pos - 1), src/posting_list.cpp:906
__device__ inline uint32_t run_pos(const TokRun& r, uint32_t j) { return (uint32_t)(uint16_t)((uint16_t)run_raw(r, j) - 1); }

// score kernel's row of the list table: what a run load needs of a ListDesc (the payload arena's word index, the list's first block)
struct alignas(16) KwRunRow { uint32_t payload_lo, payload_hi, blk_base, pad; };
__device__ inline KwRunRow kw_run_row(const ListDesc& d) {
    KwRunRow r; r.payload_lo = (uint32_t)d.payload_base; r.payload_hi = (uint32_t)(d.payload_base >> 32); r.blk_base = d.blk_base; r.pad = 0;
    return r;
}
struct KwRunSrc { const uint32_t* base; uint32_t blk_base; };          // the same, resolved: the list's payload words, its first block
__device__ inline KwRunSrc kw_run_src(const IndexView& ix, const ListDesc& d) { KwRunSrc s; s.base = ix.payload + d.payload_base; s.blk_base = d.blk_base; return s; }
__device__ inline KwRunSrc kw_run_src(const IndexView& ix, const KwRunRow* row) {          // (a row every lane reads alike: scalar registers)
    KwRunSrc s;
    s.base = ix.payload + ((unsigned long long)KW_UNIFORM32(row->payload_lo) | ((unsigned long long)KW_UNIFORM32(row->payload_hi) << 32));
    s.blk_base = KW_UNIFORM32(row->blk_base);
    return s;
}
// a block's 32-byte BlockMeta record as TWO 16-byte loads (the array is 32-byte aligned: tsgpu_index.hip). Field by field the compiler fetched it as a
// dwordx2 or dwordx4, two ushort and a dword — per token and scored hit.
__device__ __forceinline__ BlockMeta kw_load_block_meta(const BlockMeta* __restrict__ p) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(TSGPU_HIP_EMU)
    if constexpr (KW_LIST_TABLE) {
        // (whole vectors, taken apart in registers: through a union in memory the optimiser turns the copy back into field loads)
        static_assert(sizeof(BlockMeta) == 32 && offsetof(BlockMeta, n_off) == 16 && offsetof(BlockMeta, n_ids) == 24 && offsetof(BlockMeta, off_bits) == 28, "two 16-byte halves");
        typedef uint32_t KwU32x4 __attribute__((ext_vector_type(4)));
        const KwU32x4* __restrict__ h = (const KwU32x4*)p;
        const KwU32x4 a = h[0], b = h[1];
        BlockMeta m;
        m.first_id = a.x; m.ids_woff = a.y; m.oi_woff = a.z; m.off_woff = a.w;
        m.n_off = b.x; m.off_base = b.y;
        m.n_ids = (uint16_t)(b.z & 0xFFFFu); m.ids_bits = (uint8_t)((b.z >> 16) & 0xFFu); m.oi_bits = (uint8_t)(b.z >> 24);
        m.off_bits = (uint8_t)(b.w & 0xFFu); m.pad[0] = m.pad[1] = m.pad[2] = 0;
        return m;
    }
#endif
    return *p;
}
// elements i and i_next (= i + 1, or i in a block's last slot, where the caller takes n_off instead) of a packed offset_index. Up to 16 bits wide both
// lie inside the 8-byte window at element i's word (shift <= 31, 2 x bits <= 32): ONE load; wider: two windows. The guard word behind every packed
// array (tsgpu_format.h) covers the window's second word.
__device__ __forceinline__ unsigned long long kw_window_at(const uint32_t* __restrict__ w, uint32_t idx, uint32_t bits, uint32_t& shift) {
    const uint64_t bitpos = (uint64_t)idx * bits;
    const uint32_t* __restrict__ p = w + (bitpos >> 5);
    shift = (uint32_t)(bitpos & 31);
    return (uint64_t)p[0] | ((uint64_t)p[1] << 32);
}

__device__ inline uint32_t unpack_at_nb(const uint32_t* __restrict__ w, uint32_t idx, uint32_t bits) {      // (branch-free; guard word behind every packed array: tsgpu_format.h)
    uint32_t sh;
    const uint64_t two = kw_window_at(w, idx, bits, sh);
    const uint64_t mask = bits >= 32 ? 0xFFFFFFFFull : ((1ull << bits) - 1ull);
    return (uint32_t)((two >> sh) & mask);
}
__device__ inline TokRun load_run(const IndexView& ix, const KwRunSrc& src, uint32_t pos) {
    const uint32_t b = pos >> 8, i = pos & 255;
    const BlockMeta m = kw_load_block_meta(ix.blk_meta + src.blk_base + b);
    const uint32_t* __restrict__ base = src.base;
    uint32_t s, e;
    if constexpr (KW_LIST_TABLE) {
        const uint32_t* __restrict__ oi = base + m.oi_woff;
        const bool last = i == (uint32_t)m.n_ids - 1;
        uint32_t sh;
        const unsigned long long two = kw_window_at(oi, i, m.oi_bits, sh);
        const uint64_t mask = m.oi_bits >= 32 ? 0xFFFFFFFFull : ((1ull << m.oi_bits) - 1ull);
        s = (uint32_t)((two >> sh) & mask);
        uint32_t nx = (uint32_t)((two >> ((sh + m.oi_bits) & 63u)) & mask);
        if (m.oi_bits > 16) nx = unpack_at_nb(oi, last ? i : i + 1, m.oi_bits);
        e = last ? m.n_off : nx;
    } else {
        s = unpack_at(base + m.oi_woff, i, m.oi_bits);
        e = (i == (uint32_t)m.n_ids - 1) ? m.n_off : unpack_at(base + m.oi_woff, i + 1, m.oi_bits);
    }
    TokRun r;
    r.w = base + m.off_woff;
    r.start = s;
    r.base = m.off_base;
    r.raw_len = e - s;
    r.meta = m.off_bits;
    r.c01 = 0;
    if (m.off_bits <= 16) {
        const uint64_t bitpos = (uint64_t)s * m.off_bits;
        const uint32_t* __restrict__ cw = r.w + (bitpos >> 5);
        const uint32_t sh = (uint32_t)(bitpos & 31);
        const uint64_t x = ((uint64_t)cw[0] | ((uint64_t)cw[1] << 32)) >> sh;          // 2 x <=16 bits from bit sh <= 31: inside two words
        const uint32_t mask = (1u << m.off_bits) - 1u;
        const uint32_t v0 = m.off_base + ((uint32_t)x & mask), v1 = m.off_base + ((uint32_t)(x >> m.off_bits) & mask);
        const uint32_t have = (e - s) < 2 ? (e - s) : 2;
        if (((v0 | (have > 1 ? v1 : 0)) >> 16) == 0) { r.c01 = v0 | (v1 << 16); r.meta |= have << 16; }
    }
    if (e > s && run_raw(r, e - s - 1) == 0) r.meta |= 1u << 8;
    r.n = (e - s) - run_last_flag(r);
    return r;
}
__device__ inline TokRun load_run(const IndexView& ix, const ListDesc& d, uint32_t pos) { return load_run(ix, kw_run_src(ix, d), pos); }

// load_run for ALL of a hit's tokens, level by level: descriptors, block metadata, the offset_index pair, the first offsets, the last-element
// flag — each level's loads for every token are issued before any of them is waited for. Called token by token, hipcc emitted the chains one
// after the other (`s_waitcnt vmcnt(0)` at each of a chain's five levels before the next token's first load): fifteen dependent memory round
// trips per scored hit where five do; the score kernel spent 0.81 of its 1.38 ms there. Same values as load_run (the branch-free element fetch
// reads the same two words; a width of 0 masks to 0).
// src(k) = the KwRunSrc of the query's token k: from the descriptors (one more level of loads in front of the chain) or from the work item's list table
// (kw_score_kernel: no load at all). Per token and hit: two 16-byte BlockMeta loads, one offset_index window, one offsets window, and the run's last
// element where the offsets window does not hold it.
template <int TMAX, class SrcFn>
__device__ inline void load_runs_staged_from(const IndexView& ix, SrcFn src, const uint32_t (&pos)[TMAX], uint32_t T, TokRun (&runs)[TMAX], uint32_t& off_words) {
    const uint32_t* base[TMAX];
    uint32_t blk[TMAX];
    bool on[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        on[t] = (uint32_t)t < T && (t == 0 || T > 1);
        const KwRunSrc d = src(on[t] ? (uint32_t)t : 0u);
        base[t] = d.base;
        blk[t] = d.blk_base + (pos[on[t] ? t : 0] >> 8);
    }
    BlockMeta m[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) m[t] = kw_load_block_meta(ix.blk_meta + blk[t]);
    uint32_t s[TMAX], e[TMAX];
    if constexpr (KW_LIST_TABLE) {
        unsigned long long two[TMAX];
        uint32_t sh[TMAX], nxw[TMAX];
        bool wide = false;
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            two[t] = kw_window_at(base[t] + m[t].oi_woff, pos[on[t] ? t : 0] & 255, m[t].oi_bits, sh[t]);
            wide = wide || m[t].oi_bits > 16;
            nxw[t] = 0;
        }
        if (wide) {                                       // (a block of more than 65 535 offsets: elements i and i + 1 may not share a window)
#pragma unroll
            for (int t = 0; t < TMAX; t++) {
                const uint32_t i = pos[on[t] ? t : 0] & 255;
                nxw[t] = unpack_at_nb(base[t] + m[t].oi_woff, i + 1 < (uint32_t)m[t].n_ids ? i + 1 : i, m[t].oi_bits);
            }
        }
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            const uint32_t i = pos[on[t] ? t : 0] & 255;
            const uint64_t mask = m[t].oi_bits >= 32 ? 0xFFFFFFFFull : ((1ull << m[t].oi_bits) - 1ull);
            s[t] = (uint32_t)((two[t] >> sh[t]) & mask);
            const uint32_t nx = m[t].oi_bits > 16 ? nxw[t] : (uint32_t)((two[t] >> ((sh[t] + m[t].oi_bits) & 63u)) & mask);
            e[t] = (i == (uint32_t)m[t].n_ids - 1) ? m[t].n_off : nx;
        }
    } else {
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            const uint32_t i = pos[on[t] ? t : 0] & 255;
            const uint32_t* __restrict__ oi = base[t] + m[t].oi_woff;
            s[t] = unpack_at_nb(oi, i, m[t].oi_bits);
            const uint32_t nx = unpack_at_nb(oi, i + 1 < (uint32_t)m[t].n_ids ? i + 1 : i, m[t].oi_bits);
            e[t] = (i == (uint32_t)m[t].n_ids - 1) ? m[t].n_off : nx;
        }
    }
    uint64_t x[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        const uint32_t ob = m[t].off_bits <= 16 ? m[t].off_bits : 0;
        const uint64_t bitpos = (uint64_t)s[t] * ob;
        const uint32_t* __restrict__ cw = base[t] + m[t].off_woff + (bitpos >> 5);
        x[t] = ((uint64_t)cw[0] | ((uint64_t)cw[1] << 32)) >> (uint32_t)(bitpos & 31);
    }
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        TokRun r;
        r.w = base[t] + m[t].off_woff;
        r.start = s[t];
        r.base = m[t].off_base;
        r.raw_len = e[t] - s[t];
        r.meta = m[t].off_bits;
        r.c01 = 0;
        if (m[t].off_bits <= 16) {
            const uint32_t mask = (1u << m[t].off_bits) - 1u;
            const uint32_t v0 = m[t].off_base + ((uint32_t)x[t] & mask), v1 = m[t].off_base + ((uint32_t)(x[t] >> m[t].off_bits) & mask);
            const uint32_t have = (e[t] - s[t]) < 2 ? (e[t] - s[t]) : 2;
            if (((v0 | (have > 1 ? v1 : 0)) >> 16) == 0) { r.c01 = v0 | (v1 << 16); r.meta |= have << 16; }
        }
        runs[t] = r;
    }
    uint32_t lastv[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) {                      // the run's last element (0 = the token ends the field): from c01 when it is there, else one more fetch
        const uint32_t n = runs[t].raw_len, j = n ? n - 1 : 0;
        lastv[t] = j < (runs[t].meta >> 16) ? ((runs[t].c01 >> (j * 16)) & 0xFFFFu) : runs[t].base + unpack_at_nb(runs[t].w, runs[t].start + j, run_bits(runs[t]));
    }
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        if (on[t]) {
            if (runs[t].raw_len > 0 && lastv[t] == 0) runs[t].meta |= 1u << 8;
            runs[t].n = runs[t].raw_len - run_last_flag(runs[t]);
            off_words += run_raw_len(runs[t]) + 1;
        } else { TokRun r; r.w = nullptr; r.start = 0; r.n = 0; r.base = 0; r.raw_len = 0; r.meta = 0; r.c01 = 0; runs[t] = r; }      // (= empty_run())
    }
}
template <int TMAX>
__device__ inline void load_runs_staged(const IndexView& ix, const KwQueryDev& q, const uint32_t (&pos)[TMAX], uint32_t T, TokRun (&runs)[TMAX], uint32_t& off_words) {
    load_runs_staged_from<TMAX>(ix, [&](uint32_t k) { return kw_run_src(ix, ix.lists[q.list[k]]); }, pos, T, runs, off_words);
}

// The same for N (list, posting position) SLOTS of one hit — the multi-field score kernel's form (round 6): a hit of a query over two query_by fields holds up
// to T x 2 runs, and agg_score_mf fetched them ONE load_run AFTER THE OTHER — up to six dependent chains of five round trips per scored hit. Here every
// level's loads of all slots (the tokens of one field) are issued before any is waited for. A slot that is off (token absent from that field) reads
// the addresses of the caller's fallback slot (always a present one: the driver token's own field) — loads a neighbour issues anyway — and yields empty_run().
// Same values as load_run (the arithmetic is load_runs_staged's, which is checked against the oracle on every single-field hit).
template <int N>
__device__ inline void load_runs_staged_slots(const IndexView& ix, const uint32_t (&lst)[N], const uint32_t (&pos)[N], const bool (&on)[N], TokRun (&runs)[N], uint32_t& off_words) {
    const uint32_t* base[N];
    uint32_t blk[N];
#pragma unroll
    for (int t = 0; t < N; t++) {
        const ListDesc& d = ix.lists[lst[t]];
        base[t] = ix.payload + d.payload_base;
        blk[t] = d.blk_base + (pos[t] >> 8);
    }
    BlockMeta m[N];
#pragma unroll
    for (int t = 0; t < N; t++) m[t] = ix.blk_meta[blk[t]];
    uint32_t s[N], e[N];
#pragma unroll
    for (int t = 0; t < N; t++) {
        const uint32_t i = pos[t] & 255;
        const uint32_t* __restrict__ oi = base[t] + m[t].oi_woff;
        s[t] = unpack_at_nb(oi, i, m[t].oi_bits);
        const uint32_t nx = unpack_at_nb(oi, i + 1 < (uint32_t)m[t].n_ids ? i + 1 : i, m[t].oi_bits);
        e[t] = (i == (uint32_t)m[t].n_ids - 1) ? m[t].n_off : nx;
    }
    uint64_t x[N];
#pragma unroll
    for (int t = 0; t < N; t++) {
        const uint32_t ob = m[t].off_bits <= 16 ? m[t].off_bits : 0;
        const uint64_t bitpos = (uint64_t)s[t] * ob;
        const uint32_t* __restrict__ cw = base[t] + m[t].off_woff + (bitpos >> 5);
        x[t] = ((uint64_t)cw[0] | ((uint64_t)cw[1] << 32)) >> (uint32_t)(bitpos & 31);
    }
#pragma unroll
    for (int t = 0; t < N; t++) {
        TokRun r;
        r.w = base[t] + m[t].off_woff;
        r.start = s[t];
        r.base = m[t].off_base;
        r.raw_len = e[t] - s[t];
        r.meta = m[t].off_bits;
        r.c01 = 0;
        if (m[t].off_bits <= 16) {
            const uint32_t mask = (1u << m[t].off_bits) - 1u;
            const uint32_t v0 = m[t].off_base + ((uint32_t)x[t] & mask), v1 = m[t].off_base + ((uint32_t)(x[t] >> m[t].off_bits) & mask);
            const uint32_t have = (e[t] - s[t]) < 2 ? (e[t] - s[t]) : 2;
            if (((v0 | (have > 1 ? v1 : 0)) >> 16) == 0) { r.c01 = v0 | (v1 << 16); r.meta |= have << 16; }
        }
        runs[t] = r;
    }
    uint32_t lastv[N];
#pragma unroll
    for (int t = 0; t < N; t++) {                         // the run's last element (0 = the token ends the field): from c01 when it is there, else one more fetch
        const uint32_t n = runs[t].raw_len, j = n ? n - 1 : 0;
        lastv[t] = j < (runs[t].meta >> 16) ? ((runs[t].c01 >> (j * 16)) & 0xFFFFu) : runs[t].base + unpack_at_nb(runs[t].w, runs[t].start + j, run_bits(runs[t]));
    }
#pragma unroll
    for (int t = 0; t < N; t++) {
        if (on[t]) {
            if (runs[t].raw_len > 0 && lastv[t] == 0) runs[t].meta |= 1u << 8;
            runs[t].n = runs[t].raw_len - run_last_flag(runs[t]);
            off_words += run_raw_len(runs[t]) + 1;
        } else { TokRun r; r.w = nullptr; r.start = 0; r.n = 0; r.base = 0; r.raw_len = 0; r.meta = 0; r.c01 = 0; runs[t] = r; }      // (= empty_run())
    }
}

// Match::Match(doc, token_positions, populate_window=false, check_exact_match) — include/match_score.h:129-275.
// Window state lives in registers: every array index below is a compile-time constant after unrolling
// (dynamic token ids are resolved with unrolled selects), so nothing spills to scratch.
struct MatchOut { uint32_t words_present, distance, max_offset, exact_match; };

template <int TMAX>
__device__ inline MatchOut match_window(const TokRun (&runs)[TMAX], const uint32_t T, const bool check_exact) {
    const uint32_t tokens_size = T < KW_WINDOW_SIZE ? T : KW_WINDOW_SIZE;
    uint32_t wo[TMAX];   // offset (uint16 value)
    uint32_t wt[TMAX];   // token id
    uint32_t wi[TMAX];   // offset_index (cursor into the token's positions)
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        wo[t] = ((uint32_t)t < tokens_size) ? run_pos(runs[t], 0) : 0;
        wt[t] = (uint32_t)t;
        wi[t] = 0;
    }
    uint32_t wsize = tokens_size;
    uint32_t best_num_match = 1, best_displacement = 0xFFFFu /*MAX_DISPLACEMENT*/, max_offset = 0;
    int prev_min_offset = -1;

    while (wsize > 1) {
        // ---- sort descending with the reference's exact tie behaviour ----
        if (wsize == 2) {                                   // sort2, :79-84
            if (wo[0] < wo[1]) { uint32_t a = wo[0], b = wt[0], c = wi[0]; wo[0] = wo[1]; wt[0] = wt[1]; wi[0] = wi[1]; wo[1] = a; wt[1] = b; wi[1] = c; }
        } else if (TMAX >= 3 && wsize == 3) {               // sort3, :86-111 (NOT a stable sort: keep it literal)
            const int i1 = TMAX >= 3 ? 1 : 0, i2 = TMAX >= 3 ? 2 : 0;
#define TSGPU_SWAP(i, j) { uint32_t a = wo[i], b = wt[i], c = wi[i]; wo[i] = wo[j]; wt[i] = wt[j]; wi[i] = wi[j]; wo[j] = a; wt[j] = b; wi[j] = c; }
#define TSGPU_ROT(i0, j0, k0) { /* tmp=a[i0]; a[i0]=a[j0]; a[j0]=a[k0]; a[k0]=tmp */ \
            uint32_t a = wo[i0], b = wt[i0], c = wi[i0]; wo[i0] = wo[j0]; wt[i0] = wt[j0]; wi[i0] = wi[j0]; \
            wo[j0] = wo[k0]; wt[j0] = wt[k0]; wi[j0] = wi[k0]; wo[k0] = a; wt[k0] = b; wi[k0] = c; }
            if (wo[0] > wo[i1]) {
                if (wo[i1] > wo[i2]) { /* sorted */ }
                else if (wo[0] > wo[i2]) TSGPU_SWAP(i1, i2)
                else TSGPU_ROT(0, i2, i1)           // tmp=a0; a0=a2; a2=a1; a1=tmp
            } else {
                if (wo[0] > wo[i2]) TSGPU_SWAP(0, i1)
                else if (wo[i2] > wo[i1]) TSGPU_SWAP(0, i2)
                else TSGPU_ROT(0, i1, i2)           // tmp=a0; a0=a1; a1=a2; a2=tmp
            }
        } else {
            // std::sort(greater) on <=10 elements = libstdc++ insertion sort = a stable descending sort
#pragma unroll
            for (int i = 1; i < TMAX; i++) {
#pragma unroll
                for (int j = i; j >= 1; j--) {
                    if ((uint32_t)i < wsize && wo[j - 1] < wo[j]) TSGPU_SWAP(j - 1, j)
                }
            }
        }
        // ---- smallest offset = window.back() ----
        uint32_t min_offset = 0, back_t = 0, back_i = 0, front = wo[0];
#pragma unroll
        for (int i = 0; i < TMAX; i++) if ((uint32_t)i == wsize - 1) { min_offset = wo[i]; back_t = wt[i]; back_i = wi[i]; }
        if ((int)min_offset < prev_min_offset) break;       // uint16 wrap-around, :164-167
        prev_min_offset = (int)min_offset;

        uint32_t this_displacement = 0, this_num_match = 0;
#pragma unroll
        for (int i = 0; i < TMAX; i++) {
            if ((uint32_t)i < wsize && (wo[i] - min_offset) <= KW_WINDOW_SIZE) {
                uint32_t next_offset = wo[i];
                if (i + 1 < TMAX) { if ((uint32_t)(i + 1) < wsize) next_offset = wo[i + 1 < TMAX ? i + 1 : i]; }
                this_displacement += wo[i] - next_offset;
                this_num_match++;
            }
        }
        if (this_num_match > best_num_match || (this_num_match == best_num_match && this_displacement < best_displacement)) {
            best_displacement = this_displacement;
            best_num_match = this_num_match;
            max_offset = front < 255u ? front : 255u;
        }
        if (best_num_match == tokens_size && best_displacement == (wsize - 1)) break;

        // ---- pop the smallest, push the same token's next position ----
        wsize--;
        uint32_t tok_n = 0, tok_last = 0, tok_next = 0;
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            if ((uint32_t)t == back_t) {
                tok_n = runs[t].n;
                tok_last = run_pos(runs[t], runs[t].n - 1);
                tok_next = (back_i + 1 < runs[t].n) ? run_pos(runs[t], back_i + 1) : 0;
            }
        }
        (void)tok_n;
        if (min_offset == tok_last) continue;               // "no more offsets for this token" (value compare, :212-215)
#pragma unroll
        for (int i = 0; i < TMAX; i++) if ((uint32_t)i == wsize) { wo[i] = tok_next; wt[i] = back_t; wi[i] = back_i + 1; }
        wsize++;
    }
#undef TSGPU_SWAP
#undef TSGPU_ROT
    if (best_displacement == 0xFFFFu) best_displacement = 0;
    MatchOut out;
    out.words_present = best_num_match & 0xFF;
    out.distance = best_displacement & 0xFF;
    out.max_offset = max_offset;
    out.exact_match = 0;
    if (check_exact) {
        const uint32_t distance = out.distance;
        if (!(distance > T - 1)) {
            int last_token_index = -1;
            uint32_t total_offsets = 0;
            bool bail = false;
#pragma unroll
            for (int t = 0; t < TMAX; t++) {
                if ((uint32_t)t < T && !bail) {
                    if (run_last_flag(runs[t]) && runs[t].n != 0) last_token_index = (int)run_pos(runs[t], runs[t].n - 1);
                    total_offsets += runs[t].n;
                    if (total_offsets > T && distance == T - 1) bail = true;
                }
            }
            if (!bail && last_token_index == (int)T - 1) {
                if (total_offsets == T && distance == T - 1) out.exact_match = 1;
                else if (distance < T - 1) out.exact_match = 1;
            }
        }
    }
    return out;
}

// Match::get_match_score, include/match_score.h:56-68 (int64 shifts restated on uint64: identical bits)
__device__ inline uint64_t pack_match_score(uint32_t words_present, uint32_t unique_words, uint32_t total_cost,
                                            uint32_t distance, uint32_t exact, uint32_t max_offset, uint32_t synonym) {
    return ((uint64_t)(int64_t)(int32_t)words_present << 40) | ((uint64_t)(int64_t)(int32_t)unique_words << 32) |
           ((uint64_t)((int64_t)(255 - (int64_t)total_cost)) << 24) | ((uint64_t)((int64_t)(100 - (int64_t)distance)) << 16) |
           ((uint64_t)exact << 12) | ((uint64_t)((int64_t)(255 - (int64_t)max_offset)) << 4) | (uint64_t)synonym;
}

struct ScoredHit { int64_t s0, s1, s2; int64_t text_match; uint32_t off_words; };

// the unpack / synonym adjustment / re-pack of score_results2's window loop (src/index.cpp:7031-7072); s = get_match_score of the window
__device__ inline uint64_t repack_match_score(const KwQueryDev& q, uint64_t s, bool field_is_array, uint32_t n_posting_lists) {
    uint64_t this_words_present = (s >> 40) & 0xFF;
    uint64_t unique_words = field_is_array ? this_words_present : ((s >> 32) & 0xFF);
    uint64_t typo_score = (s >> 24) & 0xFF, proximity = (s >> 16) & 0xFF;
    const uint64_t verbatim = (s >> 12) & 0xF, synonym_score = s & 0xF;
    uint64_t offset_score = q.prio_pos ? ((s >> 4) & 0xFF) : 0;
    if (q.is_synonym) {
        if (q.n_query_tokens == n_posting_lists) { unique_words = (uint64_t)(int64_t)q.syn_orig_num_tokens; this_words_present = unique_words; }
        if (q.syn_orig_num_tokens > 0 && q.orig_num_tokens > 0) {
            const double rel_factor = (double)q.orig_num_tokens / (double)q.syn_orig_num_tokens;
            auto scale = [&](uint64_t v) -> uint64_t { double sc = (double)v * rel_factor; if (sc > 255.0) sc = 255.0; return (uint64_t)sc; };
            this_words_present = scale(this_words_present);
            unique_words = scale(unique_words);
            typo_score = 255 - scale(255 - typo_score);
            proximity = 100 - scale(100 - proximity);
            offset_score = q.prio_pos ? 255 - scale(255 - offset_score) : 0;
        }
    }
    return ((uint64_t)(int64_t)this_words_present << 40) | ((uint64_t)(int64_t)unique_words << 32) | ((uint64_t)(int64_t)typo_score << 24) |
           ((uint64_t)(int64_t)proximity << 16) | (verbatim << 12) | ((uint64_t)(int64_t)offset_score << 4) | synonym_score;
}
// the single-token fast path's packing (:6985-6996)
__device__ inline uint64_t single_token_match_score(const KwQueryDev& q, uint32_t verbatim, uint32_t max_offset) {
    const bool syn1 = q.n_query_tokens == 1 && q.is_synonym;
    const uint32_t words_present = syn1 ? (uint32_t)(uint8_t)q.syn_orig_num_tokens : 1u;                  // Match(uint8_t words_present, ...)
    const uint32_t distance = syn1 ? (uint32_t)(uint8_t)(q.syn_orig_num_tokens - 1) : 0u;
    const uint32_t synonym_score = (q.is_synonym && q.demote_synonym) ? 0u : 1u;
    return pack_match_score(words_present, words_present, q.total_cost, distance, verbatim, max_offset, synonym_score);
}

// score_results2 (src/index.cpp:6966-7098) for ONE plain-string field: `runs[0..n_present)` = the occurrences of the query tokens
// that this field holds for the document, in query-token order (field_to_tokens[fi], src/index.cpp:5250-5265)
template <int TMAX>
__device__ inline uint64_t field_match_score(const KwQueryDev& q, const TokRun (&runs)[TMAX], uint32_t n_present) {
    if (n_present <= 1) {   // single-token fast path, src/index.cpp:6985-6996
        const TokRun& r = runs[0];
        const bool single_exact_query_token = (q.total_cost == 0 && q.n_query_tokens == 1);
        uint32_t verbatim = 0;
        if (q.prio_exact && single_exact_query_token) {
            // is_single_token_verbatim_match, src/posting_list.cpp:918-959 (plain field)
            verbatim = (run_raw(r, 0) == 1 && run_raw_len(r) == 2 && run_raw(r, 1) == 0) ? 1u : 0u;
        }
        uint32_t max_offset = 255;
        if (q.prio_pos) {   // get_last_offset, src/posting_list.cpp:1899-1951 (plain field); narrowed to uint8 by Match()
            const uint32_t lastv = run_raw(r, run_raw_len(r) - 1);
            max_offset = (lastv == 0 ? run_raw(r, run_raw_len(r) - 2) : lastv) & 0xFF;
        }
        return single_token_match_score(q, verbatim, max_offset);
    }
    const MatchOut m = match_window<TMAX>(runs, n_present, q.prio_exact != 0);
    const uint64_t s = pack_match_score(m.words_present, n_present, q.total_cost, m.distance, m.exact_match, m.max_offset, (q.is_synonym && q.demote_synonym) ? 0u : 1u);
    return repack_match_score(q, s, false, n_present);
}

__device__ inline TokRun empty_run() { TokRun r; r.w = nullptr; r.start = 0; r.n = 0; r.base = 0; r.raw_len = 0; r.meta = 0; r.c01 = 0; return r; }

// ---- string[] fields: one token's run holds one group per array element it occurs in —
//      p1 .. pn, pn (last position repeated), array_index [, 0 if the token is that element's last token]
// (src/index.cpp:1351-1395). The three readers below restate posting_list_t::get_offsets (src/posting_list.cpp:832-916),
// is_single_token_verbatim_match (:918-959) and get_last_offset (:1899-1951) literally, quirks included.
struct ArrCursor { uint32_t i; uint32_t is_last; };
struct ArrElem { uint32_t start, n, aidx, last; bool valid; };

// next (array_index, positions) group of the run, get_offsets' while-loop resumed at c.i
__device__ inline ArrElem arr_next_elem(const TokRun& r, ArrCursor& c) {
    ArrElem e; e.start = 0; e.n = 0; e.aidx = 0; e.last = 0; e.valid = false;
    int prev_pos = -1;
    const uint32_t len = run_raw_len(r);
    while (c.i < len) {
        const int pos = (int)run_raw(r, c.i);
        c.i++;
        if (pos == 0) { c.is_last = 1; c.i++; continue; }
        if (pos == prev_pos) {                         // end of an array element
            if (e.n != 0) {
                e.aidx = c.i < len ? run_raw(r, c.i) : 0;
                c.is_last = 0;
                if (c.i + 1 < len && run_raw(r, c.i + 1) == 0) { c.is_last = 1; c.i++; }
                c.i++;
                e.last = c.is_last; e.valid = true;
                return e;
            }
            c.i++;
            prev_pos = -1;
            continue;
        }
        prev_pos = pos;
        if (e.n == 0) e.start = r.start + c.i - 1;
        e.n++;
    }
    if (e.n != 0) { e.aidx = 0; e.last = c.is_last; e.valid = true; }     // unterminated tail: treated as a plain string run
    return e;
}

__device__ inline uint32_t arr_single_verbatim(const TokRun& r) {
    int prev_pos = -1;
    uint32_t i = 0;
    const uint32_t len = run_raw_len(r);
    while (i < len) {
        const int pos = (int)run_raw(r, i);
        i++;
        if (pos == prev_pos && pos == 1 && i + 1 < len && run_raw(r, i + 1) == 0) return 1;
        prev_pos = pos;
    }
    return 0;
}

__device__ inline uint32_t arr_last_offset(const TokRun& r) {
    int prev_pos = -1;
    uint32_t i = 0, max_offset = 0;
    const uint32_t len = run_raw_len(r);
    while (i < len) {
        const int pos = (int)run_raw(r, i);
        i++;
        if ((uint32_t)pos > max_offset) max_offset = (uint32_t)pos;
        if (pos == prev_pos) {
            if (i + 1 < len && run_raw(r, i + 1) == 0) i++;
            i++;
            prev_pos = -1;
            continue;
        }
        prev_pos = pos;
    }
    return max_offset;
}

// score_results2 for a string[] field: Match per array element over the tokens that occur in it, best element wins
template <int TMAX>
__device__ inline uint64_t field_match_score_array(const KwQueryDev& q, const TokRun (&runs)[TMAX], uint32_t n_present) {
    if (n_present <= 1) {
        const TokRun& r = runs[0];
        const bool single_exact_query_token = (q.total_cost == 0 && q.n_query_tokens == 1);
        const uint32_t verbatim = (q.prio_exact && single_exact_query_token) ? arr_single_verbatim(r) : 0u;
        const uint32_t max_offset = q.prio_pos ? (arr_last_offset(r) & 0xFF) : 255u;
        return single_token_match_score(q, verbatim, max_offset);
    }
    ArrCursor cur[TMAX];
    ArrElem el[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        cur[t].i = 0; cur[t].is_last = 0;
        if ((uint32_t)t < n_present) el[t] = arr_next_elem(runs[t], cur[t]);
        else { el[t].valid = false; el[t].aidx = 0; el[t].start = 0; el[t].n = 0; el[t].last = 0; }
    }
    uint64_t best = 0;
    for (;;) {
        uint32_t a = 0xFFFFFFFFu;
        bool any = false;
#pragma unroll
        for (int t = 0; t < TMAX; t++) if (el[t].valid && el[t].aidx <= a) { if (!any || el[t].aidx < a) a = el[t].aidx; any = true; }
        if (!any) break;
        TokRun sub[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; t++) sub[t] = empty_run();
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            if (el[t].valid && el[t].aidx == a) {
                TokRun r = runs[t];
                r.start = el[t].start; r.n = el[t].n; r.raw_len = el[t].n; r.meta = run_bits(r) | (el[t].last << 8);      // (nc = 0: the register cache belongs to the run's own start)
#pragma unroll
                for (int j = 0; j < TMAX; j++) if ((uint32_t)j == m) sub[j] = r;
                m++;
                el[t] = arr_next_elem(runs[t], cur[t]);       // a token may occur in the same element index only once per group
            }
        }
        const MatchOut mo = match_window<TMAX>(sub, m, q.prio_exact != 0);
        const uint64_t s = pack_match_score(mo.words_present, n_present, q.total_cost, mo.distance, mo.exact_match, mo.max_offset, (q.is_synonym && q.demote_synonym) ? 0u : 1u);
        const uint64_t mod = repack_match_score(q, s, true /* array field: unique_words = this_words_present, :7041 */, n_present);
        if (mod > best) best = mod;
    }
    return best;
}

// the per-field fold of compute_aggregated_score (src/index.cpp:5296-5330) and its packing (:5332-5382)
struct AggState { int64_t best_fms = 0, best_w = 0, sum = 0; uint32_t n_fields = 0; };
__device__ inline void agg_add(AggState& st, uint32_t match_type, uint64_t field_score, int64_t field_weight) {
    const int64_t fms = (int64_t)field_score;
    if (match_type == 0 && fms > st.best_fms) { st.best_fms = fms; st.best_w = field_weight; }
    if (match_type == 1 && field_weight > st.best_w) { st.best_w = field_weight; st.best_fms = fms; }
    if (match_type == 2) st.sum += field_weight * fms;
    st.n_fields++;
}
__device__ inline uint64_t agg_finish(const AggState& st, const KwQueryDev& q, uint32_t tokens_found) {
    if (q.syn_orig_num_tokens != -1) tokens_found = (uint32_t)(int32_t)q.syn_orig_num_tokens;       // :5292-5294 (size_t query_len = int)
    const uint64_t query_len = (st.best_fms == 0) ? 0 : (tokens_found < 15 ? tokens_found : 15);
    const uint64_t max_field_weight = (uint64_t)st.best_w < 15 ? (uint64_t)st.best_w : 15;   // std::min<size_t>(15, w)
    const uint64_t num_matching_fields = q.prio_nfields ? (st.n_fields < 7 ? st.n_fields : 7) : 0;
    if (q.match_type == 0) return (query_len << 59) | ((uint64_t)st.best_fms << 11) | (max_field_weight << 3) | num_matching_fields;
    if (q.match_type == 1) return (query_len << 59) | (max_field_weight << 51) | ((uint64_t)st.best_fms << 3) | num_matching_fields;
    return (query_len << 59) | ((uint64_t)st.sum << 3) | num_matching_fields;
}

// compute_sort_scores, src/index.cpp:5662-5907 (text_match / seq_id / int64 column) + :5541-5544 override
__device__ inline int64_t float_to_int64_dev(float f) {       // Index::float_to_int64_t, src/index.cpp:266-274
    int32_t i = (int32_t)__float_as_uint(f);
    if (i < 0) i ^= INT32_MAX;
    return (int64_t)i;
}
// The `_eval` branch (:5761-5834) for a document taken on its own: the score of the FIRST expression whose id list holds it, else 0. (The reference keeps one
// forward-only cursor per expression; over ascending seq_ids — every caller of the keyword paths — that is plain membership.)
__device__ inline int64_t sort_key_eval(const SortKeyDesc& d, uint32_t seq_id) {
    if (d.dense) {
        const uint32_t e = seq_id < d.dense_len ? d.dense[seq_id] : 0u;
        return e ? d.scores[e - 1] : 0;
    }
    for (uint32_t e = 0; e < d.n_expr; e++) {
        uint32_t lo = d.expr_off[e];
        const uint32_t end = d.expr_off[e + 1];
        uint32_t hi = end;
        while (lo < hi) {                                   // std::lower_bound (:5823)
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (d.ids[mid] < seq_id) lo = mid + 1; else hi = mid;
        }
        if (lo < end && d.ids[lo] == seq_id) return d.scores[e];
    }
    return 0;
}
// Builds the DENSE form of a key: dense[id] = tag (= expression + 1) for the ids of ONE expression. The host launches it once per expression, LAST to FIRST on one
// stream, so where lists overlap the first expression's byte is the one that stays; ids are unique within a launch: plain byte stores, no atomics.
__global__ __launch_bounds__(256) void sort_key_scatter_kernel(const uint32_t* __restrict__ ids, uint32_t n, uint8_t* __restrict__ dense, uint32_t dense_len, uint32_t tag) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t id = ids[i];
        if (id < dense_len) dense[id] = (uint8_t)tag;
    }
}
// the sort kinds beyond the four of the headline path (include/tsgpu.h): _eval, missing_values: first on a numeric column, string ranks
__device__ inline int64_t sort_key_value(const IndexView& ix, uint32_t kind, uint32_t col, int order, uint32_t seq_id) {
    if (kind == 4) return sort_key_eval(ix.sort_keys[col < KW_SORT_KEY_SLOTS ? col : 0], seq_id);
    if (kind == 9) return 0;                   // TSGPU_SORT_VECTOR_QUERY: the wave fills the slot in afterwards (wave_vq_sort_patch, kw_vq_sort.hip.h)
    int64_t v = (col < ix.n_columns && seq_id < ix.column_len[col]) ? ix.columns[col][seq_id] : (kind == 5 ? INT64_MIN : INT64_MAX);
    if (kind == 5) { if (v == INT64_MIN) v = order == -1 ? INT64_MIN + 1 : INT64_MAX; }                 // (:5892-5898)
    else if (kind == 7 && v == INT64_MAX) v = (int64_t)(0ull - (uint64_t)v);                            // adi_tree_t::NOT_FOUND, flipped (:5750-5760)
    return v;
}
// KEYS = false: no query of the launch has a slot of kind >= TSGPU_SORT_EVAL (the planner knows) — the score kernel's PLAIN instantiations, i.e. the headline
// path, are compiled without those branches (profiles/r07/sortkeys_resource_usage.txt: with them the <3, 512, false, false, true> score kernel spilled 7 more VGPRs).
template <bool KEYS = true>
__device__ inline ScoredHit sort_scores(const IndexView& ix, const KwQueryDev& q, uint32_t seq_id, uint64_t agg, uint32_t off_words,
                                        bool override_text_match = true, float vector_distance = 0.0f) {
    int64_t sc[3] = {0, 0, 0};
    int msi = -1;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (i < q.n_sort) {
            int64_t v;
            if (q.sort_kind[i] == 0) { v = (int64_t)agg; msi = i; }
            else if (q.sort_kind[i] == 1) v = (int64_t)seq_id;
            else if (q.sort_kind[i] == 2) {
                const uint32_t c = q.sort_col[i];
                v = (c < ix.n_columns && seq_id < ix.column_len[c]) ? ix.columns[c][seq_id] : INT64_MIN;
            } else if (q.sort_kind[i] == 3) v = float_to_int64_dev(vector_distance);   // (:5835-5836; keyword passes hand 0: float_to_int64_t(0) == 0)
            else if constexpr (KEYS) v = sort_key_value(ix, q.sort_kind[i], q.sort_col[i], q.sort_order[i], seq_id);
            else v = 0;
            if (q.sort_order[i] == -1) v = (int64_t)(0ull - (uint64_t)v);
            sc[i] = v;
        }
    }
    int64_t tm = (int64_t)agg;
#pragma unroll
    for (int i = 0; i < 3; i++) if (i == msi) { if (override_text_match) sc[i] = (int64_t)agg; else tm = sc[i]; }
    if (!override_text_match && msi < 0) tm = 0;
    ScoredHit h;
    h.s0 = sc[0]; h.s1 = sc[1]; h.s2 = sc[2];
    h.text_match = tm;
    h.off_words = off_words;
    return h;
}

#include "kw_vq_sort.hip.h"


// score_results2 + compute_aggregated_score + compute_sort_scores for ONE query_by field (plain string); pos[t] = posting
// position of found token t
// TAB: tab = the work item's list table (kw_score_kernel): one KwRunRow per token of the query instead of a descriptor load per token and hit
template <int TMAX, bool KEYS = true, bool TAB = false>
__device__ inline ScoredHit score_hit(const IndexView& ix, const KwQueryDev& q, uint32_t seq_id, const uint32_t (&pos)[TMAX], const KwRunRow* tab = nullptr) {
    const uint32_t T = q.n_lists;
    uint32_t off_words = 0;
    TokRun runs[TMAX];
    if constexpr (TMAX <= 3 && TAB) load_runs_staged_from<TMAX>(ix, [&](uint32_t k) { return kw_run_src(ix, tab + k); }, pos, T, runs, off_words);
    else if constexpr (TMAX <= 3) load_runs_staged<TMAX>(ix, q, pos, T, runs, off_words);
    else {
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            if constexpr (TAB) { if ((uint32_t)t < T && (t == 0 || T > 1)) { runs[t] = load_run(ix, kw_run_src(ix, tab + t), pos[t]); off_words += run_raw_len(runs[t]) + 1; } else runs[t] = empty_run(); }
            else if ((uint32_t)t < T && (t == 0 || T > 1)) { runs[t] = load_run(ix, ix.lists[q.list[t]], pos[t]); off_words += run_raw_len(runs[t]) + 1; }
            else runs[t] = empty_run();
        }
    }
    AggState st;
    agg_add(st, q.match_type, field_match_score<TMAX>(q, runs, T), q.weight);      // (string[] fields take the multi-field kernel: the planner routes them)
    return sort_scores<KEYS>(ix, q, seq_id, agg_finish(st, q, T), off_words);
}

// the same for several query_by fields: pos[t * KW_MAX_FIELDS + f] = position of found token t in field f's list, or KW_NONE.
// Per field, the tokens it holds for this document (query order) are scored together; the fields are folded by match_type.
// compute_aggregated_score for several query_by fields: pos[t * KW_MAX_FIELDS + f] = position of found token t in field f's list, or
// KW_NONE. Per field, the tokens it holds for this document (query order) are scored together; the fields are folded by match_type.
// tokens_found = tokens present in at least one field (query_len of src/index.cpp:5265-5268).
// ARR = false: no query of the launch has a string[] field (the host knows) — the instantiation without the per-element scorer.
template <int TMAX, bool ARR = true>
__device__ inline uint64_t agg_score_mf(const IndexView& ix, const KwQueryDev& q, const KwQueryMF& mf, const uint32_t (&pos)[TMAX * KW_MAX_FIELDS],
                                        uint32_t tokens_found, uint32_t& off_words) {
    const uint32_t T = q.n_lists;
    AggState st;
    if constexpr (TMAX <= 3 && KW_MF_STAGED) {
        // (round 6) the runs of ONE field's tokens level by level (load_runs_staged_slots): five dependent round trips per field instead of five per (token, field).
        // (Two fields at a time — six staged runs — needs more than the 128 registers the kernel's occupancy allows: 108 B of scratch, 3.41 -> 3.76 ms.)
        uint32_t fb_list = 0, fb_pos = 0;
        bool have_fb = false;
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
#pragma unroll
            for (int ff = 0; ff < KW_MAX_FIELDS; ff++) {
                const uint32_t p = pos[t * KW_MAX_FIELDS + ff];
                if (!have_fb && (uint32_t)t < T && (uint32_t)ff < mf.n_fields && p != KW_NONE) { have_fb = true; fb_list = mf.list[t][ff]; fb_pos = p; }
            }
        }
        if (!have_fb) return agg_finish(st, q, tokens_found);      // (cannot happen: a hit holds the driver token in the item's own field)
        for (uint32_t f = 0; f < mf.n_fields; f++) {
            uint32_t lst[TMAX], ps[TMAX];
            bool on[TMAX];
            uint32_t n_on = 0;
#pragma unroll
            for (int t = 0; t < TMAX; t++) {
                uint32_t p = KW_NONE;
#pragma unroll
                for (int g = 0; g < KW_MAX_FIELDS; g++) if ((uint32_t)g == f) p = pos[t * KW_MAX_FIELDS + g];
                const bool o = (uint32_t)t < T && p != KW_NONE;
                on[t] = o;
                lst[t] = o ? mf.list[t][f] : fb_list;
                ps[t] = o ? p : fb_pos;
                n_on += o ? 1u : 0u;
            }
            if (n_on == 0) continue;                          // field holds none of the tokens for this document (:5298-5300)
            TokRun all[TMAX];
            load_runs_staged_slots<TMAX>(ix, lst, ps, on, all, off_words);
            TokRun runs[TMAX];
#pragma unroll
            for (int t = 0; t < TMAX; t++) runs[t] = empty_run();
            uint32_t n_present = 0;
#pragma unroll
            for (int t = 0; t < TMAX; t++) {
                if (on[t]) {
#pragma unroll
                    for (int j = 0; j < TMAX; j++) if ((uint32_t)j == n_present) runs[j] = all[t];      // append without dynamic register indexing
                    n_present++;
                }
            }
            agg_add(st, q.match_type, (ARR && mf.is_array[f]) ? field_match_score_array<TMAX>(q, runs, n_present) : field_match_score<TMAX>(q, runs, n_present), mf.weight[f]);
        }
        return agg_finish(st, q, tokens_found);
    }
    for (uint32_t f = 0; f < mf.n_fields; f++) {
        TokRun runs[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; t++) runs[t] = empty_run();
        uint32_t n_present = 0;
#pragma unroll
        for (int t = 0; t < TMAX; t++) {
            uint32_t p = KW_NONE;
#pragma unroll
            for (int ff = 0; ff < KW_MAX_FIELDS; ff++) if ((uint32_t)ff == f) p = pos[t * KW_MAX_FIELDS + ff];
            if ((uint32_t)t < T && p != KW_NONE) {
                const TokRun r = load_run(ix, ix.lists[mf.list[t][f]], p);
                off_words += run_raw_len(r) + 1;
#pragma unroll
                for (int j = 0; j < TMAX; j++) if ((uint32_t)j == n_present) runs[j] = r;      // append without dynamic register indexing
                n_present++;
            }
        }
        if (n_present == 0) continue;                     // field holds none of the tokens for this document (:5298-5300)
        agg_add(st, q.match_type, (ARR && mf.is_array[f]) ? field_match_score_array<TMAX>(q, runs, n_present) : field_match_score<TMAX>(q, runs, n_present), mf.weight[f]);
    }
    return agg_finish(st, q, tokens_found);
}
template <int TMAX, bool ARR = true, bool KEYS = true>
__device__ inline ScoredHit score_hit_mf(const IndexView& ix, const KwQueryDev& q, const KwQueryMF& mf, uint32_t seq_id,
                                         const uint32_t (&pos)[TMAX * KW_MAX_FIELDS]) {
    uint32_t off_words = 0;
    // query_len = tokens found in some field: every required token (the AND) + the dropped tokens this document holds (:5265-5290)
    uint32_t tokens_found = q.n_required;
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        bool any = false;
#pragma unroll
        for (int f = 0; f < KW_MAX_FIELDS; f++) any = any || pos[t * KW_MAX_FIELDS + f] != KW_NONE;
        if ((uint32_t)t >= q.n_required && (uint32_t)t < q.n_lists && any) tokens_found++;
    }
    const uint64_t agg = agg_score_mf<TMAX, ARR>(ix, q, mf, pos, tokens_found, off_words);
    return sort_scores<KEYS>(ix, q, seq_id, agg, off_words);
}

// ------------------------------------------------------------------------------------------------
// LDS top-K buffer. Entry = (s0, s1, s2, key) with key < 0 marking padding; order = KV::is_greater
// (include/topster.h:146-149). CAP is a power of two >= k + 256.
__device__ inline bool ent_greater(int64_t a0, int64_t a1, int64_t a2, int64_t ak, int64_t b0, int64_t b1, int64_t b2, int64_t bk) {
    if (ak < 0 || bk < 0) return bk < 0 && ak >= 0;       // padding sorts last
    if (a0 != b0) return a0 > b0;
    if (a1 != b1) return a1 > b1;
    if (a2 != b2) return a2 > b2;
    return ak > bk;
}

// S2 = false: no query of the launch has a third sort key, scores[2] is 0 everywhere and its column shrinks to one slot
// (4 KB of LDS at CAP = 512 -> one more resident workgroup per CU)
template <int CAP, bool S2 = true>
struct TopkLds {
    int64_t s0[CAP], s1[CAP], s2[S2 ? CAP : 1], key[CAP];
    __device__ static inline int i2(int i) { return S2 ? i : 0; }
};

// bitonic sort, descending, of the first n entries (n a power of two <= CAP, uniform; entries >= cnt must be padding): a work item
// with a dozen hits sorts 16 slots (10 stages), not the whole buffer (45 stages at CAP = 512)
template <int CAP, bool S2>
__device__ inline void topk_sort(TopkLds<CAP, S2>& tk, int n = CAP) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int p = threadIdx.x; p < n / 2; p += KW_THREADS) {
                const int i = 2 * p - (p & (stride - 1));     // lower index of the pair
                const int j = i + stride;
                const bool desc = ((i & size) == 0);
                const int64_t a0 = tk.s0[i], a1 = tk.s1[i], a2 = tk.s2[tk.i2(i)], ak = tk.key[i];
                const int64_t b0 = tk.s0[j], b1 = tk.s1[j], b2 = tk.s2[tk.i2(j)], bk = tk.key[j];
                const bool b_gt_a = ent_greater(b0, b1, b2, bk, a0, a1, a2, ak);
                const bool a_gt_b = ent_greater(a0, a1, a2, ak, b0, b1, b2, bk);
                if (desc ? b_gt_a : a_gt_b) {
                    tk.s0[i] = b0; tk.s1[i] = b1; tk.key[i] = bk;
                    tk.s0[j] = a0; tk.s1[j] = a1; tk.key[j] = ak;
                    if (S2) { tk.s2[tk.i2(i)] = b2; tk.s2[tk.i2(j)] = a2; }
                }
            }
        }
    }
    __syncthreads();
}

// sort + keep the best k; returns new count; thr* = k-th best when the buffer holds >= k entries
template <int CAP, bool S2>
__device__ inline void topk_compact(TopkLds<CAP, S2>& tk, uint32_t* s_cnt, uint32_t k, int64_t* s_thr /*[4]*/, uint32_t* s_have_thr) {
    __syncthreads();
    const uint32_t cnt = *s_cnt;
    int n = 2;
    while ((uint32_t)n < cnt) n <<= 1;                      // cnt <= CAP (a power of two)
    for (int i = threadIdx.x; i < n; i += KW_THREADS) if ((uint32_t)i >= cnt) tk.key[i] = -1;
    topk_sort<CAP, S2>(tk, n);
    if (threadIdx.x == 0) {
        const uint32_t n = cnt < k ? cnt : k;
        *s_cnt = n;
        if (n >= k) { s_thr[0] = tk.s0[k - 1]; s_thr[1] = tk.s1[k - 1]; s_thr[2] = tk.s2[tk.i2(k - 1)]; s_thr[3] = tk.key[k - 1]; *s_have_thr = 1; }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
struct KwNoTopk {};
// DEFER = the "find" half of the two-kernel form (kw_search_kernel<.., DEFER = true> writes complete hits to memory, kw_score_kernel
// scores them): no final queue, no top-K buffer, no filter bookkeeping -> 18 KB instead of 38 KB of LDS
// SCORE = the other half (kw_score_kernel): no stage-1 queue, tile or window
template <int TMAX, int CAP, bool MF, bool S2 = true, bool DEFER = false, bool SCORE = false>
struct KwSmem {
    static const int Q1 = SCORE ? 1 : KW_QCAP;
    static const int NP = MF ? TMAX * KW_MAX_FIELDS : TMAX;    // posting positions carried per complete hit
    static const bool HAS_S2 = S2;
    static const int QF = DEFER ? 1 : (SCORE ? KW_THREADS : KW_QCAP);     // (the score kernel stages 256 records per round: half the queue — 13 KB less LDS in the
                                                                         //  multi-field instantiation, whose records carry TMAX x 4 positions: 3 -> 4 workgroups per CU)
    // stage-1 survivors: id, driver position, first-probe position
    uint32_t q1_id[Q1], q1_p0[Q1], q1_p1[Q1];
    // several query_by fields: the queued survivor's positions in the SECOND token's lists of fields 1.. (field 0: q1_p1)
    uint32_t q1_px[(MF && !SCORE) ? KW_MAX_FIELDS - 1 : 1][(MF && !SCORE) ? Q1 : 1];
    // complete hits: id + posting position per token (query order; multi-field: per token and field, KW_NONE = absent)
    uint32_t qf_id[QF];
    uint32_t qf_pos[NP][QF];
    typename std::conditional<DEFER, KwNoTopk, TopkLds<CAP, S2>>::type tk;
    int64_t thr[4];
    static const int TILE_WORDS = SCORE ? 2 : (DEFER ? (MF ? KW_MF_TILE_WORDS : KW_FIND_TILE_WORDS) : KW_TILE_WORDS);
    uint32_t btile[TILE_WORDS + 2];          // packed ids of the second list's blocks under the current driver block
    static const int BW = SCORE ? 1 : 64;
    uint32_t bw_last[2][BW], bw_first[2][BW], bw_woff[2][BW], bw_nb[2][BW];   // the second list's BlockIds window, SoA, two versions
    uint32_t wave_cnt[KW_THREADS / 64];
    uint32_t wave_cnt2[2][KW_THREADS / 64];  // block_compact1 ping-pong
    uint32_t stop;                           // kw_out_of_time's shared decision
    uint32_t q1_cnt, qf_cnt, tk_cnt, have_thr;
    uint32_t n_match, n_emit;
    unsigned long long off_words;
    // filter-id bookkeeping (take_id with filter ids, src/or_iterator.cpp:218-272)
    uint32_t f_rank[DEFER ? 1 : KW_THREADS]; // filter rank (# filter ids <= hit) of the hits of the current score batch
    uint8_t f_ex[DEFER ? 4 : KW_THREADS];    // hit is an excluded id
    uint32_t f_first, f_frank, f_rp, f_ep, f_c0, f_c1, f_cnt0, f_cnt1;
};

// PLAIN (score kernel only): no query of the launch has filter ids, excluded ids or a sort slot of kind >= TSGPU_SORT_EVAL and no caller keeps the matched ids — the host knows, and the
// instantiation without those paths is a smaller kernel (registers, not LDS, set the score kernel's occupancy).
// VQ: some query of the launch has a TSGPU_SORT_VECTOR_QUERY slot (the host knows): only those launches carry the wave-cooperative distance code (kw_vq_sort.hip.h).
template <int TMAX, int CAP, bool MF, bool S2, bool SCORE, bool PLAIN = false, bool VQ = false>
__device__ inline void kw_score_stage(KwSmem<TMAX, CAP, MF, S2, false, SCORE>& sm, const IndexView& ix, const KwQueryDev& q, uint32_t n_take,
                                      const uint32_t* __restrict__ aux_ids, uint32_t* __restrict__ ids_out, uint32_t ids_out_base, const KwRunRow* tab = nullptr) {
    // make room: at most n_take (<=256) new entries. (The score kernel decides AFTER scoring, from the number of hits that beat the
    // current k-th best — see below; in the fused kernel that would keep the scores live across the sort and cost it a workgroup per CU.)
    if constexpr (!SCORE) { if (sm.tk_cnt + KW_THREADS > (uint32_t)CAP) topk_compact<CAP, S2>(sm.tk, &sm.tk_cnt, q.k, sm.thr, &sm.have_thr); }
    const uint32_t t = threadIdx.x;
    const bool active = t < n_take;
    bool emit = false, excl = false;
    uint32_t seq_id = 0, rank = 0;
    ScoredHit h;
    h.s0 = h.s1 = h.s2 = h.text_match = 0; h.off_words = 0;
    if (active) {
        seq_id = sm.qf_id[t];
        emit = true;
        // take_id(): excluded ids first (src/or_iterator.cpp:222-229) ...
        if (!PLAIN && q.n_excl) {
            const uint32_t* ex = aux_ids + q.aux_off;
            uint32_t lo = 0, hi = q.n_excl;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ex[mid] < seq_id) lo = mid + 1; else hi = mid; }
            if (lo < q.n_excl && ex[lo] == seq_id) { emit = false; excl = true; }
        }
        // ... then the filter ids (:232-253): the hit is taken iff it is a filter id. rank = # filter ids <= hit (upper bound)
        if (!PLAIN && q.n_filt) {
            const uint32_t* fl = aux_ids + q.aux_off + q.n_excl;
            uint32_t lo = 0, hi = q.n_filt;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (fl[mid] <= seq_id) lo = mid + 1; else hi = mid; }
            rank = lo;
            if (!(rank > 0 && fl[rank - 1] == seq_id)) emit = false;
        }
        if (emit) {
            constexpr int NP = KwSmem<TMAX, CAP, MF, S2, false, SCORE>::NP;
            uint32_t pos[NP];
#pragma unroll
            for (int k = 0; k < NP; k++) pos[k] = sm.qf_pos[k][t];
            if constexpr (MF) h = score_hit_mf<TMAX, !PLAIN, !PLAIN>(ix, q, ix.mf[q.mf_index], seq_id, pos);     // (PLAIN multi-field launches: no string[] field and no sort-key slot either)
            else {
#if defined(TSGPU_EXP) && TSGPU_EXP == 6
                h.s0 = (int64_t)(seq_id * 2654435761u); h.s1 = (int64_t)pos[0] + pos[TMAX - 1]; h.s2 = 0; h.text_match = h.s0; h.off_words = 1;
#else
                h = score_hit<TMAX, !PLAIN, SCORE && KW_LIST_TABLE>(ix, q, seq_id, pos, tab);      // (the score kernel hands its list table; the fused kernel has none)
#endif
            }
        }
    }
    if constexpr (VQ) wave_vq_sort_patch(ix, q, seq_id, emit, h);          // (every lane of the wave is here; hits that are not emitted cost no distance)
    // num_keyword_matches under a filter (kw_filter_count below): which intersection ids does the reference's loop VISIT?
    if constexpr (PLAIN) {
    } else if (MF && q.n_filt) {
        // Several driver lists (query_by over several fields): the work items' hit streams interleave in id order, so the slices cannot
        // be chained. Without exclusions the count has an order-free form: filter ranks never decrease along the intersection, so the
        // ids the reference's loop lands on — rank exceeds the predecessor's — number exactly the DISTINCT POSITIVE ranks of the
        // intersection. Every hit's rank is recorded in the query's bitmap (equal ranks of one work item are adjacent: only the first
        // of a run touches memory); a work item counts the bits it set first. (Filter + exclusions + several fields: kw_mf_ordered_count_kernel.)
        if (active) sm.f_rank[t] = rank;
        __syncthreads();
        bool fresh = false;
        if (active && rank > 0 && (t == 0 || sm.f_rank[t - 1] != rank)) {
            const uint32_t bit = 1u << ((rank - 1) & 31);
            fresh = (atomicOr(&ix.fbits[q.fbits_off + ((rank - 1) >> 5)], bit) & bit) == 0;
        }
        const unsigned long long m = __ballot(fresh ? 1 : 0);
        if ((t & 63) == 0 && m) atomicAdd(&sm.f_cnt0, (uint32_t)__popcll(m));
        __syncthreads();
    } else if (q.n_filt) {
        if (active) { sm.f_rank[t] = rank; sm.f_ex[t] = excl ? 1 : 0; }
        __syncthreads();
        if (q.n_excl == 0) {
            // a visited id = the first intersection id at or after some filter id = a hit whose filter rank exceeds its predecessor's.
            // The chunk's very first hit depends on the previous chunk (resolved by kw_merge_kernel): it is left out of f_cnt0.
            bool a = false;
            if (active) {
                if (t == 0) a = sm.f_first ? false : rank > sm.f_rp;
                else a = rank > sm.f_rank[t - 1];
            }
            const unsigned long long m = __ballot(a ? 1 : 0);
            if ((t & 63) == 0 && m) atomicAdd(&sm.f_cnt0, (uint32_t)__popcll(m));
            __syncthreads();
            if (t == 0) {
                if (sm.f_first) { sm.f_frank = sm.f_rank[0]; sm.f_first = 0; }
                sm.f_rp = sm.f_rank[n_take - 1];
            }
        } else if (t == 0) {
            // exclusions AND a filter (curated hits + filter_by; rare): after an excluded id the reference advances to the very next
            // intersection id instead of skipping to the filter (include/or_iterator.h:161-176), so "visited" becomes a first-order
            // recurrence c_j = (rank_j > rank_{j-1}) | (c_{j-1} & excluded_{j-1}); evaluated in order by one thread, for both
            // possible values of the chunk's first c (f_c0 / f_c1).
            uint32_t c0 = sm.f_c0, c1 = sm.f_c1, ep = sm.f_ep, rp = sm.f_rp, first = sm.f_first, n0 = sm.f_cnt0, n1 = sm.f_cnt1;
            for (uint32_t j = 0; j < n_take; j++) {
                const uint32_t r = sm.f_rank[j], e = sm.f_ex[j];
                if (first) { sm.f_frank = r; c0 = 0; c1 = 1; first = 0; }
                else { const uint32_t a = r > rp ? 1u : 0u; c0 = a | (c0 & ep); c1 = a | (c1 & ep); }
                n0 += c0; n1 += c1; ep = e; rp = r;
            }
            sm.f_c0 = c0; sm.f_c1 = c1; sm.f_ep = ep; sm.f_rp = rp; sm.f_first = first; sm.f_cnt0 = n0; sm.f_cnt1 = n1;
        }
    }
    // ordered emission of matched ids (id_buff, src/index.cpp:5549)
    uint32_t total;
    const uint32_t my = block_compact(emit, sm.wave_cnt, total);
    if (!PLAIN && emit && ids_out) ids_out[ids_out_base + sm.n_emit + my] = seq_id;
    if constexpr (SCORE) {
        // only hits that beat the current k-th best are appended, and the buffer is re-sorted only when THEY do not fit: once the
        // threshold is up, a batch of 256 hits adds a handful of entries
        bool pass = emit && (!sm.have_thr || ent_greater(h.s0, h.s1, h.s2, (int64_t)seq_id, sm.thr[0], sm.thr[1], sm.thr[2], sm.thr[3]));
        const uint32_t held = sm.tk_cnt;                             // stable: the last appends were followed by a barrier; read BEFORE anyone appends again
        const uint32_t n_pass = (uint32_t)__syncthreads_count(pass ? 1 : 0);
        if (held + n_pass > (uint32_t)CAP) {
            topk_compact<CAP, S2>(sm.tk, &sm.tk_cnt, q.k, sm.thr, &sm.have_thr);   // -> <= k entries, CAP >= k + 256
            pass = pass && (!sm.have_thr || ent_greater(h.s0, h.s1, h.s2, (int64_t)seq_id, sm.thr[0], sm.thr[1], sm.thr[2], sm.thr[3]));
        }
        if (pass) {
            const uint32_t slot = atomicAdd(&sm.tk_cnt, 1u);
            sm.tk.s0[slot] = h.s0; sm.tk.s1[slot] = h.s1; sm.tk.key[slot] = (int64_t)seq_id;
            if (S2) sm.tk.s2[sm.tk.i2(slot)] = h.s2;
        }
        uint32_t ow = emit ? h.off_words : 0u;                       // offsets read (algorithmic byte count): one LDS atomic per wave
        for (int d = 32; d > 0; d >>= 1) ow += __shfl_down(ow, d, 64);
        if ((t & 63) == 0 && ow) atomicAdd(&sm.off_words, (unsigned long long)ow);
    } else if (emit) {
#if defined(TSGPU_EXP) && TSGPU_EXP == 5
        const bool pass = seq_id == 0xFFFFFFFEu;
#else
        const bool pass = !sm.have_thr || ent_greater(h.s0, h.s1, h.s2, (int64_t)seq_id, sm.thr[0], sm.thr[1], sm.thr[2], sm.thr[3]);
#endif
        if (pass) {
            const uint32_t slot = atomicAdd(&sm.tk_cnt, 1u);
            sm.tk.s0[slot] = h.s0; sm.tk.s1[slot] = h.s1; sm.tk.key[slot] = (int64_t)seq_id;
            if (S2) sm.tk.s2[sm.tk.i2(slot)] = h.s2;
        }
        atomicAdd(&sm.off_words, (unsigned long long)h.off_words);
    }
    __syncthreads();
    if (t == 0) { sm.n_match += n_take; sm.n_emit += total; }
    if constexpr (SCORE) return;                  // (the score kernel refills the whole queue itself)
    // drop the processed head of the final queue
    constexpr int NPQ = KwSmem<TMAX, CAP, MF, S2, false, SCORE>::NP;
    const uint32_t rest = sm.qf_cnt - n_take;
    uint32_t mv_id = 0, mv_pos[NPQ];
    if (t < rest) {
        mv_id = sm.qf_id[n_take + t];
#pragma unroll
        for (int k = 0; k < NPQ; k++) mv_pos[k] = sm.qf_pos[k][n_take + t];
    }
    __syncthreads();
    if (t < rest) {
        sm.qf_id[t] = mv_id;
#pragma unroll
        for (int k = 0; k < NPQ; k++) sm.qf_pos[k][t] = mv_pos[k];
    }
    if (t == 0) sm.qf_cnt = rest;
    __syncthreads();
}

// one complete hit of a query of <= 3 tokens as the find kernel hands it to kw_score_kernel: seq_id + posting position per token
struct KwHitRec { uint32_t id, p0, p1, p2; };              // TMAX = 3: one 16-byte store / load
// generic record: 1 + TMAX words {seq_id, pos[0 .. TMAX)}; the buffer is addressed in words, hit_off[] counts records
template <int TMAX>
__device__ inline void kw_hit_store(uint32_t* __restrict__ hits, uint32_t slot, uint32_t id, const uint32_t (&pos)[TMAX]) {
    if constexpr (TMAX == 3) {
        KwHitRec r; r.id = id; r.p0 = pos[0]; r.p1 = pos[1]; r.p2 = pos[2];
        ((KwHitRec*)hits)[slot] = r;
    } else {
        uint32_t* __restrict__ d = hits + (size_t)slot * (TMAX + 1);
        d[0] = id;
#pragma unroll
        for (int k = 0; k < TMAX; k++) d[1 + k] = pos[k];
    }
}

// probes lists probe_order[2..] for the first n_take entries of queue 1 and moves survivors to the final queue
// (DEFER: to the work item's hit segment in memory; sm.qf_cnt counts them)
template <int TMAX, int CAP, bool S2, bool DEFER>
__device__ inline void kw_probe_rest_stage(KwSmem<TMAX, CAP, false, S2, DEFER>& sm, const IndexView& ix, const KwQueryDev& q, uint32_t n_take,
                                           uint32_t* __restrict__ hits) {
    const uint32_t t = threadIdx.x;
    bool ok = t < n_take;
    uint32_t id = 0;
    uint32_t pos[TMAX];
#pragma unroll
    for (int k = 0; k < TMAX; k++) pos[k] = 0;
    if (ok) {
        id = sm.q1_id[t];
        const uint32_t p0 = sm.q1_p0[t], p1 = sm.q1_p1[t];
#pragma unroll
        for (int k = 0; k < TMAX; k++) { if (k == q.probe_order[0]) pos[k] = p0; if (k == q.probe_order[1]) pos[k] = p1; }
        for (uint32_t s = 2; s < q.n_lists && ok; s++) {
            const uint32_t tok = q.probe_order[s];
            uint32_t p;
            ok = probe_list(ix, ix.lists[q.list[tok]], id, p);
#pragma unroll
            for (int k = 0; k < TMAX; k++) if ((uint32_t)k == tok) pos[k] = p;
        }
    }
#if defined(TSGPU_EXP) && TSGPU_EXP == 4
    ok = ok && (id == 0xFFFFFFFEu);
#endif
    uint32_t total;
    const uint32_t my = block_compact(ok, sm.wave_cnt, total);
    if (ok) {
        const uint32_t slot = sm.qf_cnt + my;
        if constexpr (DEFER) {
            kw_hit_store<TMAX>(hits, slot, id, pos);
        } else {
            sm.qf_id[slot] = id;
#pragma unroll
            for (int k = 0; k < TMAX; k++) sm.qf_pos[k][slot] = pos[k];
        }
    }
    // drop processed head of queue 1
    const uint32_t rest = sm.q1_cnt - n_take;
    uint32_t a = 0, b = 0, c = 0;
    if (t < rest) { a = sm.q1_id[n_take + t]; b = sm.q1_p0[n_take + t]; c = sm.q1_p1[n_take + t]; }
    __syncthreads();
    if (t < rest) { sm.q1_id[t] = a; sm.q1_p0[t] = b; sm.q1_p1[t] = c; }
    if (t == 0) { sm.q1_cnt = rest; sm.qf_cnt += total; }
    __syncthreads();
}

// the work item's partial result: its top-K in sort() order + the counters kw_merge_kernel folds
template <int TMAX, int CAP, bool MF, bool S2, bool SCORE>
__device__ inline void kw_write_partial(KwSmem<TMAX, CAP, MF, S2, false, SCORE>& sm, const KwQueryDev& q, const KwPartials& part, const uint32_t bid) {
    const uint32_t t = threadIdx.x;
    topk_compact<CAP, S2>(sm.tk, &sm.tk_cnt, q.k, sm.thr, &sm.have_thr);
    const uint32_t n = sm.tk_cnt;
    const size_t base = (size_t)bid * part.k_stride;
    for (uint32_t i = t; i < n; i += KW_THREADS) {
        part.s0[base + i] = sm.tk.s0[i]; part.s1[base + i] = sm.tk.s1[i]; part.s2[base + i] = sm.tk.s2[sm.tk.i2(i)]; part.key[base + i] = sm.tk.key[i];
    }
    if (t == 0) {
        part.cnt[bid] = n;
        part.n_emit[bid] = sm.n_emit;
        part.off_words[bid] = sm.off_words;
        if (q.n_filt == 0) part.n_match[bid] = sm.n_match;
        else if (MF) part.n_match[bid] = sm.f_cnt0;            // rank bits this work item set first (summed by kw_merge_kernel)
        else {
            const uint32_t nonempty = sm.f_first ? 0u : 1u;
            const bool seq = q.n_excl != 0;                       // sequential mode tracked both variants itself
            part.n_match[bid] = sm.f_cnt0;
            part.n_match1[bid] = seq ? sm.f_cnt1 : sm.f_cnt0 + nonempty;
            part.first_rank[bid] = sm.f_frank;
            part.last_rank[bid] = sm.f_rp;
            part.fflags[bid] = nonempty | (seq ? ((sm.f_c0 & sm.f_ep) << 1) | ((sm.f_c1 & sm.f_ep) << 2) : 0u);
        }
    }
}

// grid = work items; block = 256 threads
// DEFER = false: intersect + score + select in one kernel. DEFER = true (queries of <= 3 tokens): the "find" half — complete hits go
// to hits[hit_off[work item] ..] as KwHitRec, part.cnt[work item] = how many; kw_score_kernel scores them with full wavefronts.
// Splitting takes the scoring code's registers and the top-K buffer's LDS out of the merge loop (more resident waves there) and
// lets the score stage run on dense batches instead of on whatever a work item's queue holds when it flushes.
template <int TMAX, int CAP, bool S2, bool DEFER = false, bool VQ = false>
__global__ __launch_bounds__(KW_THREADS) KW_FOUR_WAVES_PER_SIMD void kw_search_kernel(IndexView ix, const KwQueryDev* __restrict__ queries,
                                                                const KwWorkItem* __restrict__ work, KwPartials part,
                                                                const uint32_t* __restrict__ aux_ids, uint32_t* __restrict__ ids_out,
                                                                uint32_t* __restrict__ hits_all, const uint64_t* __restrict__ hit_off) {
    __shared__ KwSmem<TMAX, CAP, false, S2, DEFER> sm;
    uint32_t* __restrict__ hits = DEFER ? hits_all + hit_off[blockIdx.x] * (uint64_t)(TMAX + 1) : nullptr;
    __shared__ KwQueryDev sq;
    const uint32_t t = threadIdx.x;
    const KwWorkItem wi = work[blockIdx.x];
    // stage the query descriptor in LDS (uniform data)
    {
        const uint32_t* src = (const uint32_t*)(queries + wi.query);
        uint32_t* dst = (uint32_t*)&sq;
        for (uint32_t i = t; i < sizeof(KwQueryDev) / 4; i += KW_THREADS) dst[i] = src[i];
    }
    if (t == 0) {
        sm.q1_cnt = 0; sm.qf_cnt = 0; sm.tk_cnt = 0; sm.have_thr = 0; sm.n_match = 0; sm.n_emit = 0; sm.off_words = 0;
        sm.f_first = 1; sm.f_frank = 0; sm.f_rp = 0; sm.f_ep = 0; sm.f_c0 = 0; sm.f_c1 = 0; sm.f_cnt0 = 0; sm.f_cnt1 = 0;
        if constexpr (!DEFER) { if (!S2) sm.tk.s2[0] = 0; }     // the one shared scores[2] slot of the two-key build
    }
    __syncthreads();
    const KwQueryDev& q = sq;
    const uint32_t T = q.n_lists;
    const ListDesc dA = ix.lists[q.list[q.probe_order[0]]];
    const uint32_t ids_out_base = (uint32_t)0;
    uint32_t* my_ids_out = ids_out ? ids_out + q.ids_out_off + wi.ids_out_off : nullptr;

    const ListDesc dB = ix.lists[q.list[q.probe_order[T >= 2 ? 1 : 0]]];
    const uint32_t* __restrict__ blB = ix.blk_last + dB.blk_base;
    const BlockIds* __restrict__ biA = ix.blk_ids + dA.blk_base;
    const BlockIds* __restrict__ biB = ix.blk_ids + dB.blk_base;
    const uint32_t* __restrict__ idwA = ix.ids_payload + dA.ids_base;
    const uint32_t* __restrict__ idwB = ix.ids_payload + dB.ids_base;
    const uint32_t lane = t & 63;
    const BlockIds PAD = {0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};

    // Doc ids of a block are stored as fixed-width deltas from the block's first id: 16 bits when the block's id
    // range fits (the common case), else 32 (tsgpu_pack.h) — one aligned load per id, no bit arithmetic.
    auto load_id_raw = [&](const uint32_t* __restrict__ base, const BlockIds& m, uint32_t slot) -> uint32_t {
        const uint32_t n = m.n_ids_bits & 0xFFFF;
        const uint32_t s2 = slot < n ? slot : 0;
        const uint32_t* __restrict__ w = base + m.ids_woff;
        return (m.n_ids_bits >> 16) == 16 ? (uint32_t)((const uint16_t*)w)[s2] : w[s2];
    };
    auto load_window = [&](uint32_t base) -> BlockIds { return (T >= 2 && base + lane < dB.n_blocks) ? biB[base + lane] : PAD; };

    // driver-side BlockIds: read from memory (uniform 16-byte loads), kept TWO blocks ahead in registers — block b+1's record
    // is needed by make_plan while block b is searched. (Measured and rejected: a lane-resident 64-block window of the driver list +
    // four v_readlane per block instead of the scalar load: 9.45 -> 10.27 ms per 10 000-query batch.)
    auto a_meta_of = [&](uint32_t bb) -> BlockIds { return biA[bb < wi.blk_end ? bb : wi.blk_end - 1]; };

    KW_PROF_DECL
    // Software pipeline over the driver blocks (global round trips cost 1-2K cycles under load): block b+1's ids and
    // block b+1's tile of second-list ids are requested while block b is being searched; the second list's BlockIds
    // window lives in registers (lane <-> block; win = [wbase, wbase+64), nxt = [wbase+32, wbase+96) already in
    // flight) and only slides forward.
    uint32_t wbase = 0, wver = 0;
    BlockIds win = load_window(0), nxt = load_window(32);
    bool win_dirty = true;                    // LDS copy of the window (sm.bw[wver]) is stale
    struct Plan { uint32_t mode, rlo, rhi, w_begin, W, ver, base; };   // mode: 0 tile, 1 tile in several rounds, 2 wide run (probe), 3 exhausted, 4 no second list
    constexpr int PIPE_WORDS = DEFER ? KW_FIND_PIPE_WORDS : KW_PIPE_WORDS;
    constexpr int TILE_WORDS = decltype(sm)::TILE_WORDS;
    uint32_t cw[PIPE_WORDS] = {};                 // block b's tile of second-list ids, in flight from the previous iteration
    // decide how driver block `bb` meets the second list and (mode 0) request its tile
    auto make_plan = [&](const BlockIds& m) -> Plan {
        Plan P; P.mode = 4; P.rlo = P.rhi = P.w_begin = P.W = 0; P.ver = wver; P.base = wbase;
        if (T < 2) return P;
        const uint32_t lo_id = m.first_id, hi_id = m.last_id;
        unsigned long long mk = __ballot(win.last_id >= lo_id ? 1 : 0);
        if (mk != 0 && (uint32_t)__builtin_ctzll(mk) >= 32) {          // cursor entered the upper half: slide by 32 blocks
            wbase += 32; win = nxt; nxt = load_window(wbase + 32); win_dirty = true;
            mk = __ballot(win.last_id >= lo_id ? 1 : 0);
        }
        if (mk == 0) {                                                   // all 64 blocks end before lo_id: uniform search, re-centre
            uint32_t lo = wbase + 64, hi = dB.n_blocks;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (blB[mid] >= lo_id) hi = mid; else lo = mid + 1; }
            wbase = lo; win = load_window(wbase); nxt = load_window(wbase + 32); win_dirty = true;
            mk = __ballot(win.last_id >= lo_id ? 1 : 0);               // lane 0 votes yes (real block or padding)
        }
        P.rlo = (uint32_t)__builtin_ctzll(mk);
        P.base = wbase;
        if (wbase + P.rlo >= dB.n_blocks) { P.mode = 3; return P; }     // every remaining driver id is beyond B's last id
        const unsigned long long mh = __ballot(win.last_id >= hi_id ? 1 : 0);
        if (mh == 0) { P.mode = 2; return P; }                           // run of B blocks wider than the window
        P.rhi = (uint32_t)__builtin_ctzll(mh);
        if (wbase + P.rhi >= dB.n_blocks) P.rhi = dB.n_blocks - 1 - wbase;   // hi_id beyond B's last id
        if (win_dirty) {                                                 // publish the window for the block search
            wver ^= 1;
            if (t < 64) { sm.bw_last[wver][t] = win.last_id; sm.bw_first[wver][t] = win.first_id; sm.bw_woff[wver][t] = win.ids_woff; sm.bw_nb[wver][t] = win.n_ids_bits; }
            win_dirty = false;
        }
        P.ver = wver;
        const uint32_t w_endw = win.ids_woff + packed_words(win.n_ids_bits & 0xFFFF, win.n_ids_bits >> 16);
        if (dB.flags & LIST_HAS_BREAKS) {                                // (uniform, rare: blocks re-written by an incremental commit)
            // the tile copy below takes the run's ids as ONE range of the arena: a run with a relocated block inside is probed per candidate
            const uint32_t nxt_woff = (uint32_t)__shfl(win.ids_woff, (int)((lane + 1) & 63));
            const bool brk = lane >= P.rlo && lane < P.rhi && w_endw != nxt_woff;
            if (__ballot(brk ? 1 : 0) != 0) { P.mode = 2; return P; }
        }
        P.w_begin = (uint32_t)__shfl(win.ids_woff, (int)P.rlo);
        P.W = (uint32_t)__shfl(w_endw, (int)P.rhi) - P.w_begin;
        if (P.W <= (uint32_t)(PIPE_WORDS * KW_THREADS)) {
            P.mode = 0;
            const uint32_t* __restrict__ src = idwB + P.w_begin;
            // (a short run — the common case — does not issue the loads it has no words for: two tiers instead of a guard per load)
            if (DEFER && P.W <= 2u * KW_THREADS) {            // (find kernel only: the fused kernel has no register to spare for a second code path)
#pragma unroll
                for (int k = 0; k < 2 && k < PIPE_WORDS; k++) { const uint32_t i = t + k * KW_THREADS; cw[k] = src[i < P.W ? i : 0]; }
            } else {
#pragma unroll
                for (int k = 0; k < PIPE_WORDS; k++) { const uint32_t i = t + k * KW_THREADS; cw[k] = src[i < P.W ? i : 0]; }
            }
        } else P.mode = 1;
        return P;
    };

    BlockIds mA = a_meta_of(wi.blk_begin), mA1 = a_meta_of(wi.blk_begin + 1);
    uint32_t araw = load_id_raw(idwA, mA, t);
    Plan P = make_plan(mA);
    uint32_t q1n = 0, qfn = 0, par = 0;       // queue fill levels mirrored in registers (identical in every thread)

    for (uint32_t b = wi.blk_begin; b < wi.blk_end; b++) {
        if (P.mode == 3) break;
        if (((b - wi.blk_begin) & 15) == 0 && kw_out_of_time(ix, q, wi.query, &sm.stop)) break;
        // ---- stage 0: thread t = slot t of driver block b ----
        const uint32_t m_n = mA.n_ids_bits & 0xFFFF;
        bool ok = t < m_n;
        const uint32_t id = ok ? mA.first_id + araw : 0xFFFFFFFFu;
        uint32_t p1 = 0;
        // (filter ids are applied to complete hits in kw_score_stage: the reference's num_keyword_matches needs the whole intersection)
        KW_PROF(0)
        const Plan C = P;                      // this block's plan; P becomes the next block's below
        // ---- stage 1: merge with the second-shortest list B ----
        uint32_t kb = 0, b_first = 0, b_nb = 0, b_rel = 0;
        bool done = !ok || C.mode >= 2, found = false;
        if (C.mode == 0) {
            // (words beyond the run are never read by the searches below: when the tile can hold a whole pipeline the stores carry no
            //  guard — a guarded store is an exec-mask branch per word)
            constexpr bool GUARD = PIPE_WORDS * KW_THREADS > TILE_WORDS;
            if (DEFER && C.W <= 2u * KW_THREADS) {
#pragma unroll
                for (int k = 0; k < 2 && k < PIPE_WORDS; k++) { const uint32_t i = t + k * KW_THREADS; if (!GUARD || i < C.W) sm.btile[i] = cw[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < PIPE_WORDS; k++) { const uint32_t i = t + k * KW_THREADS; if (!GUARD || i < C.W) sm.btile[i] = cw[k]; }
            }
        }
        KW_PROF(1)
        __syncthreads();
        KW_PROF(2)
        // (a) which block: lower bound of id among the window's last ids (bw_last[rhi] >= hi_id >= id unless B ended).
        // The common short run: the block = rlo + #{run blocks that END before the id}. The run's last ids are wave-uniform values sitting
        // in the window registers (this plan's window: the next plan has not moved it yet) — one v_readlane and one compare per block
        // instead of dependent LDS reads. (Every lane runs it: wave-uniform control flow.)
        const uint32_t span = C.rhi - C.rlo;
        uint32_t pos_short = C.rlo;
#ifndef TSGPU_KW_SHORT_SPAN
#define TSGPU_KW_SHORT_SPAN 8
#endif
        if (C.mode <= 1 && span <= TSGPU_KW_SHORT_SPAN) {
            for (uint32_t j = C.rlo; j < C.rhi; j++) {
                const uint32_t last_j = (uint32_t)__builtin_amdgcn_readlane((int)win.last_id, (int)j);
                pos_short += last_j < id ? 1u : 0u;
            }
        }
        if (C.mode <= 1 && !done) {
            const uint32_t* __restrict__ bl = sm.bw_last[C.ver];
            uint32_t pos = pos_short;
            if (span > TSGPU_KW_SHORT_SPAN) {
                // (uniform trip count: a run of s+1 blocks needs the steps from the largest power of two <= s down)
                for (uint32_t step = 1u << (31 - __builtin_clz(span)); step > 0; step >>= 1) {
                    const uint32_t j = pos + step;                       // (clamped load + select: no branch per step)
                    const uint32_t v = bl[(j <= C.rhi ? j : C.rhi) - 1];
                    pos = (j <= C.rhi && v < id) ? j : pos;
                }
            }
            kb = pos;
            b_first = sm.bw_first[C.ver][pos];
            if (bl[pos] < id || id < b_first) done = true;             // beyond B's end / in the gap between two blocks
            b_nb = sm.bw_nb[C.ver][pos];
            b_rel = sm.bw_woff[C.ver][pos] - C.w_begin;
        }
#if defined(TSGPU_EXP) && TSGPU_EXP >= 2 && TSGPU_EXP < 4
        done = true;
#endif
        KW_PROF(3)
        // ---- request the next driver block's ids and its tile (in flight during the slot search below) ----
        const BlockIds mA2 = a_meta_of(b + 2);              // in flight during this block's search
        uint32_t araw1 = 0;
        if (b + 1 < wi.blk_end) {
            araw1 = load_id_raw(idwA, mA1, t);
            KW_PROF(10)
            P = make_plan(mA1);
        }
        KW_PROF(4)
        // (b) which slot: branch-free lower bound over the block's ids in the LDS tile
        auto slot_search = [&](uint32_t tile_rel) {
            const uint32_t n = b_nb & 0xFFFF, target = id - b_first;
            uint32_t pos = 0, hit;
            if ((b_nb >> 16) == 16) {
                const uint16_t* __restrict__ a16 = (const uint16_t*)(sm.btile + tile_rel);
                if (n == (uint32_t)BLOCK_IDS) {
                    // every block but a list's last is full: no bound checks, and without them the steps compile to straight-line
                    // code (load, compare, select) instead of eight exec-mask branches
#pragma unroll
                    for (uint32_t step = 128; step > 0; step >>= 1) { const uint32_t v = a16[pos + step - 1]; pos = v < target ? pos + step : pos; }
                } else {
#pragma unroll
                    for (uint32_t step = 128; step > 0; step >>= 1) {
                        const uint32_t j = pos + step;
                        const uint32_t v = a16[(j <= n ? j : n) - 1];
                        pos = (j <= n && v < target) ? j : pos;
                    }
                }
                hit = a16[pos];
            } else {
                const uint32_t* __restrict__ a32 = sm.btile + tile_rel;
#pragma unroll
                for (uint32_t step = 128; step > 0; step >>= 1) {
                    const uint32_t j = pos + step;
                    const uint32_t v = a32[(j <= n ? j : n) - 1];
                    pos = (j <= n && v < target) ? j : pos;
                }
                hit = a32[pos];
            }
            done = true;
            if (hit == target) { found = true; p1 = (C.base + kb) * BLOCK_IDS + pos; }
        };
        if (C.mode == 0) {
            if (!done) slot_search(b_rel);
        } else if (C.mode == 1) {
            // the run does not fit the pipelined tile: several rounds over [rlo, rhi], each a coalesced copy of as many
            // whole blocks as fit the LDS tile (at least one: a block is <= 257 words)
            const uint32_t* __restrict__ woff = sm.bw_woff[C.ver];
            const uint32_t* __restrict__ wnb = sm.bw_nb[C.ver];
            for (uint32_t r_lo = C.rlo; r_lo <= C.rhi;) {
                const uint32_t w_begin = woff[r_lo];
                uint32_t r_hi = r_lo;
                while (r_hi < C.rhi && woff[r_hi + 1] + packed_words(wnb[r_hi + 1] & 0xFFFF, wnb[r_hi + 1] >> 16) - w_begin <= (uint32_t)TILE_WORDS) r_hi++;
                const uint32_t W = woff[r_hi] + packed_words(wnb[r_hi] & 0xFFFF, wnb[r_hi] >> 16) - w_begin;
                const uint32_t* __restrict__ src = idwB + w_begin;
                __syncthreads();                                        // previous round's searches are done with the tile
                for (uint32_t i0 = t; i0 < W + t; i0 += 2 * KW_THREADS) {   // uniform trip count; 2 loads in flight per trip
                    const uint32_t i1 = i0 + KW_THREADS;
                    const uint32_t c0 = src[i0 < W ? i0 : 0], c1 = src[i1 < W ? i1 : 0];
                    if (i0 < W) sm.btile[i0] = c0;
                    if (i1 < W) sm.btile[i1] = c1;
                }
                __syncthreads();
                if (!done && kb >= r_lo && kb <= r_hi) slot_search(woff[kb] - w_begin);
                r_lo = r_hi + 1;
            }
        } else if (C.mode == 2) {
            // the run of B blocks under this driver block is wider than the window: per-candidate probe; the cursor
            // moved with the next plan (its window search re-centres)
            if (ok) found = probe_list(ix, dB, id, p1);
        }
        if (T >= 2) ok = ok && found;
#if defined(TSGPU_EXP) && TSGPU_EXP >= 1 && TSGPU_EXP < 4
        ok = ok && (id == 0xFFFFFFFEu);   // ablation: drop survivors without letting the compiler drop stage 1
#endif
        KW_PROF(5)
        uint32_t total;
        const uint32_t my = block_compact1(ok, sm.wave_cnt2[par], total);
        par ^= 1;
        KW_PROF(6)
        const uint32_t p0 = b * BLOCK_IDS + t;
        if (T >= 3) {
            if (ok) { const uint32_t slot = q1n + my; sm.q1_id[slot] = id; sm.q1_p0[slot] = p0; sm.q1_p1[slot] = p1; }
            q1n += total;
            KW_PROF(11)
            if (q1n >= KW_THREADS) {
                __syncthreads();
                if (t == 0) sm.q1_cnt = q1n;
                __syncthreads();
                while (sm.q1_cnt >= KW_THREADS) {
                    kw_probe_rest_stage<TMAX, CAP, S2, DEFER>(sm, ix, q, KW_THREADS, hits);
                    if constexpr (!DEFER)
                        while (sm.qf_cnt >= KW_THREADS) kw_score_stage<TMAX, CAP, false, S2, false, false, VQ>(sm, ix, q, KW_THREADS, aux_ids, my_ids_out, ids_out_base);
                }
                q1n = sm.q1_cnt;
            }
        } else if constexpr (DEFER) {
            if (ok) {                                   // one or two lists: the stage-1 survivors ARE the complete hits
                uint32_t v[TMAX];
#pragma unroll
                for (int k = 0; k < TMAX; k++) { v[k] = 0; if (k == q.probe_order[0]) v[k] = p0; if (T >= 2 && k == q.probe_order[1]) v[k] = p1; }
                kw_hit_store<TMAX>(hits, qfn + my, id, v);
            }
            qfn += total;
        } else {
            if (ok) {
                const uint32_t slot = qfn + my;
                sm.qf_id[slot] = id;
#pragma unroll
                for (int k = 0; k < TMAX; k++) {
                    uint32_t v = 0;
                    if (k == q.probe_order[0]) v = p0;
                    if (T >= 2 && k == q.probe_order[1]) v = p1;
                    sm.qf_pos[k][slot] = v;
                }
            }
            qfn += total;
            if (qfn >= KW_THREADS) {
                __syncthreads();
                if (t == 0) sm.qf_cnt = qfn;
                __syncthreads();
                while (sm.qf_cnt >= KW_THREADS) kw_score_stage<TMAX, CAP, false, S2, false, false, VQ>(sm, ix, q, KW_THREADS, aux_ids, my_ids_out, ids_out_base);
                qfn = sm.qf_cnt;
            }
        }
        KW_PROF(7)
        mA = mA1; mA1 = mA2; araw = araw1;
    }
    __syncthreads();
    if (t == 0) { if (T >= 3) sm.q1_cnt = q1n; else sm.qf_cnt = qfn; }
    __syncthreads();
    // ---- flush ----
    if (T >= 3) {
        while (sm.q1_cnt > 0) {
            kw_probe_rest_stage<TMAX, CAP, S2, DEFER>(sm, ix, q, sm.q1_cnt < KW_THREADS ? sm.q1_cnt : KW_THREADS, hits);
            if constexpr (!DEFER)
                while (sm.qf_cnt >= KW_THREADS) kw_score_stage<TMAX, CAP, false, S2, false, false, VQ>(sm, ix, q, KW_THREADS, aux_ids, my_ids_out, ids_out_base);
        }
    }
    if constexpr (DEFER) {
        if (t == 0) part.cnt[blockIdx.x] = sm.qf_cnt;              // hits handed to kw_score_kernel
    } else {
        while (sm.qf_cnt > 0) kw_score_stage<TMAX, CAP, false, S2, false, false, VQ>(sm, ix, q, sm.qf_cnt < KW_THREADS ? sm.qf_cnt : KW_THREADS, aux_ids, my_ids_out, ids_out_base);
        KW_PROF(8)
        // ---- partial result of this work item: sorted, <= k entries ----
        kw_write_partial(sm, q, part, blockIdx.x);
    }
    KW_PROF(9)
    KW_PROF_FLUSH(ix.prof)
}

// The "score" half of the two-kernel form: one workgroup per work item of the find kernel; its hits (seq_id + posting positions,
// ascending seq_id) are scored 256 at a time — every wavefront full except the segment's last — through the same score stage,
// top-K buffer and filter bookkeeping as the fused kernel, and leave the same partial result for kw_merge_kernel.
// (body = a device function with the work item's index as a parameter; round 5's one-launch round kernel, measured slower and removed in round 6 —
//  profiles/r05/exp_one_launch_rounds.txt — ran it behind the find body)
template <int TMAX, int CAP, bool S2, bool MF = false, bool PLAIN = false, bool VQ = false>
__device__ __forceinline__ void kw_score_body(const IndexView& ix, const KwQueryDev* __restrict__ queries, const KwWorkItem* __restrict__ work,
                                              const KwPartials& part, const uint32_t* __restrict__ aux_ids, uint32_t* __restrict__ ids_out,
                                              const uint32_t* __restrict__ hits_all, const uint64_t* __restrict__ hit_off, const uint32_t bid) {
    __shared__ KwSmem<TMAX, CAP, MF, S2, false, true> sm;
    __shared__ KwQueryDev sq;
    __shared__ KwRunRow tab[(KW_LIST_TABLE && !MF) ? TMAX : 1];          // the list table (single-field launches): a row per token of the query
    constexpr int NP = decltype(sm)::NP;          // posting positions per record: TMAX, or TMAX x KW_MAX_FIELDS for several query_by fields
    const uint32_t t = threadIdx.x;
    const KwWorkItem wi = work[bid];
    {
        const uint32_t* src = (const uint32_t*)(queries + (wi.query & 0x0FFFFFFFu));      // (multi-field items carry the driver field in the top bits)
        uint32_t* dst = (uint32_t*)&sq;
        for (uint32_t i = t; i < sizeof(KwQueryDev) / 4; i += KW_THREADS) dst[i] = src[i];
    }
    if constexpr (KW_LIST_TABLE && !MF) {
        // lane k of the second wave fills token k's row from the query in global memory (the copy above is not visible before the barrier); rows behind
        // the query's last token repeat token 0's, which is what the staged loader reads for an absent token
        if (t >= 64 && t < 64 + (uint32_t)TMAX) {
            const KwQueryDev* __restrict__ gq = queries + (wi.query & 0x0FFFFFFFu);
            const uint32_t k = t - 64;
            const uint32_t n = gq->n_lists;
            KwRunRow r; r.payload_lo = r.payload_hi = r.blk_base = r.pad = 0;                  // (a query without a token has no hit to score)
            if (n) r = kw_run_row(ix.lists[gq->list[k < n ? k : 0u]]);
            tab[k] = r;
        }
    }
    if (t == 0) {
        sm.q1_cnt = 0; sm.qf_cnt = 0; sm.tk_cnt = 0; sm.have_thr = 0; sm.n_match = 0; sm.n_emit = 0; sm.off_words = 0;
        sm.f_first = 1; sm.f_frank = 0; sm.f_rp = 0; sm.f_ep = 0; sm.f_c0 = 0; sm.f_c1 = 0; sm.f_cnt0 = 0; sm.f_cnt1 = 0;
        if (!S2) sm.tk.s2[0] = 0;
    }
    __syncthreads();
    const KwQueryDev& q = sq;
    uint32_t* my_ids_out = ids_out ? ids_out + q.ids_out_off + wi.ids_out_off : nullptr;
    const uint32_t count = part.cnt[bid];
    const uint32_t* __restrict__ mine = hits_all + hit_off[bid] * (uint64_t)(NP + 1);
    for (uint32_t i0 = 0; i0 < count; i0 += KW_THREADS) {
        const uint32_t n = count - i0 < (uint32_t)KW_THREADS ? count - i0 : (uint32_t)KW_THREADS;
        if (t < n) {
            if constexpr (TMAX == 3 && !MF) {
                const KwHitRec r = ((const KwHitRec*)mine)[i0 + t];
                sm.qf_id[t] = r.id; sm.qf_pos[0][t] = r.p0; sm.qf_pos[1][t] = r.p1; sm.qf_pos[2][t] = r.p2;
            } else {
                const uint32_t* __restrict__ r = mine + (size_t)(i0 + t) * (NP + 1);
                sm.qf_id[t] = r[0];
#pragma unroll
                for (int k = 0; k < NP; k++) sm.qf_pos[k][t] = r[1 + k];
            }
        }
        if (t == 0) sm.qf_cnt = n;
        __syncthreads();
        kw_score_stage<TMAX, CAP, MF, S2, true, PLAIN, VQ>(sm, ix, q, n, aux_ids, my_ids_out, 0u, tab);
    }
    kw_write_partial(sm, q, part, bid);
}
template <int TMAX, int CAP, bool S2, bool MF = false, bool PLAIN = false, bool VQ = false>
__global__ __launch_bounds__(KW_THREADS) KW_SCORE_WAVES void kw_score_kernel(IndexView ix, const KwQueryDev* __restrict__ queries, const KwWorkItem* __restrict__ work,
                                                              KwPartials part, const uint32_t* __restrict__ aux_ids, uint32_t* __restrict__ ids_out,
                                                              const uint32_t* __restrict__ hits_all, const uint64_t* __restrict__ hit_off) {
    kw_score_body<TMAX, CAP, S2, MF, PLAIN, VQ>(ix, queries, work, part, aux_ids, ids_out, hits_all, hit_off, blockIdx.x);
}

// LDS-DMA tile fill: N slabs of 256 words, lane t of the workgroup copies word (slab * 256 + t) of the run straight from global memory
// into the LDS tile (global_load_lds_dword: destination = M0 base + lane * 4 + instruction offset, the same offset advances the source) —
// no staging registers, no ds_write. Words past the run's end are read, too: the ids arena ends with KW_TILE_OVERREAD_WORDS of padding
// (tsgpu_index.hip) and nothing searches them. Issued through inline asm: the one wait the pipeline needs is kw_glds_wait() before the
// barrier at the top of the next iteration (cf. vec_glds16 in vec_kernels.hip.h).
template <int N>
__device__ inline void kw_glds_slabs(const uint32_t* lane_src, uint32_t* lds_wave_base) {
    static_assert(N == 2 || N == 4 || N == 6 || N == 7 || N == 8, "slabs of 256 words, four per M0 setting");
#ifdef TSGPU_HIP_EMU
    for (int k = 0; k < N; k++) hipemu_global_load_lds4(lane_src + k * 256, lds_wave_base + k * 256);
#else
    const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds_wave_base);
    uint32_t keep;
    if constexpr (N == 2) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\tglobal_load_lds_dword %1, off offset:1024\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane_src), "s"(dst) : "memory");
    } else if constexpr (N == 4) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                     "global_load_lds_dword %1, off\n\tglobal_load_lds_dword %1, off offset:1024\n\t"
                     "global_load_lds_dword %1, off offset:2048\n\tglobal_load_lds_dword %1, off offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane_src), "s"(dst) : "memory");
    } else if constexpr (N == 7) {
        const uint32_t* lane_src2 = lane_src + 1024;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dword %1, off\n\tglobal_load_lds_dword %1, off offset:1024\n\t"
                     "global_load_lds_dword %1, off offset:2048\n\tglobal_load_lds_dword %1, off offset:3072\n\t"
                     "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
                     "global_load_lds_dword %2, off\n\tglobal_load_lds_dword %2, off offset:1024\n\tglobal_load_lds_dword %2, off offset:2048\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane_src), "v"(lane_src2), "s"(dst) : "memory", "scc");
    } else if constexpr (N == 6) {
        const uint32_t* lane_src2 = lane_src + 1024;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dword %1, off\n\tglobal_load_lds_dword %1, off offset:1024\n\t"
                     "global_load_lds_dword %1, off offset:2048\n\tglobal_load_lds_dword %1, off offset:3072\n\t"
                     "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
                     "global_load_lds_dword %2, off\n\tglobal_load_lds_dword %2, off offset:1024\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane_src), "v"(lane_src2), "s"(dst) : "memory", "scc");
    } else {
        const uint32_t* lane_src2 = lane_src + 1024;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dword %1, off\n\tglobal_load_lds_dword %1, off offset:1024\n\t"
                     "global_load_lds_dword %1, off offset:2048\n\tglobal_load_lds_dword %1, off offset:3072\n\t"
                     "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\t"
                     "global_load_lds_dword %2, off\n\tglobal_load_lds_dword %2, off offset:1024\n\t"
                     "global_load_lds_dword %2, off offset:2048\n\tglobal_load_lds_dword %2, off offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane_src), "v"(lane_src2), "s"(dst) : "memory", "scc");
    }
#endif
}
__device__ inline void kw_glds_wait() {
#ifndef TSGPU_HIP_EMU
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}

// The multi-field find kernel's form of stage 1 (kw_find2.hip.h has the pipelined single-field one): the ids of ONE driver block against ONE
// other list L as a block-level merge. The run of L's blocks under the driver block's id range [lo_id, hi_id] is found with a 64-block register
// window behind a cursor that only moves forward (one coalesced load of BlockIds + two ballots; every wave computes the same), the ids of that
// run — ONE contiguous range of the ids arena — are copied coalesced into the LDS tile, and each candidate does two LDS lower bounds (block among
// the run's last ids, slot among the block's ids). Before, every candidate probed L in global memory (probe_list: ~6 dependent loads per probe,
// 64-byte lines per lane — the kernel moved 5.7 TB/s out of L2 for 2 000 two-field queries on 10M documents). Runs wider than the window or the
// tile and lists with relocated blocks keep the per-candidate probe. Must be called by every thread of the workgroup; uniform arguments except
// want / id / found / p.
template <class SM>
__device__ inline void kw_mf_merge_field(SM& sm, const IndexView& ix, const ListDesc& d, uint32_t& wbase, uint32_t lo_id, uint32_t hi_id, bool want, uint32_t id,
                                         bool& found, uint32_t& p) {
    constexpr uint32_t TILE = (uint32_t)SM::TILE_WORDS;
    const uint32_t t = threadIdx.x, lane = t & 63;
    found = false;
    if (wbase >= d.n_blocks || lo_id > d.last_id) { wbase = d.n_blocks; return; }             // the list ends before this driver block: nothing more to find (uniform)
    if (hi_id < d.first_id) return;
    const BlockIds* __restrict__ bi = ix.blk_ids + d.blk_base;
    const BlockIds PAD = {0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
    BlockIds win = wbase + lane < d.n_blocks ? bi[wbase + lane] : PAD;
    unsigned long long mk = __ballot(win.last_id >= lo_id ? 1 : 0);
    if (mk == 0) {                                                                           // all 64 blocks end before lo_id: uniform search, re-centre
        const uint32_t* __restrict__ bl = ix.blk_last + d.blk_base;                           // (lo_id <= d.last_id: some block ends at or behind it)
        wbase = guided_lower_bound(d.n_blocks, lo_id, d.first_id, d.last_id, [&](uint32_t i) { return bl[i]; });      // interpolation-guided: ~2 long + 4 short loads
        if (wbase >= d.n_blocks) return;
        win = wbase + lane < d.n_blocks ? bi[wbase + lane] : PAD;
        mk = __ballot(win.last_id >= lo_id ? 1 : 0);
    }
    const uint32_t rlo = (uint32_t)__builtin_ctzll(mk);
    const uint32_t base = wbase;                                                             // the window's first block (positions below are relative to it)
    wbase += rlo;                                                                            // the cursor: blocks before rlo end before every later driver block, too
    if (base + rlo >= d.n_blocks) return;
    if (__shfl(win.first_id, (int)rlo) > hi_id) return;                                     // the run's first block starts behind the driver block: no candidate can be in L
    const unsigned long long mh = __ballot(win.last_id >= hi_id ? 1 : 0);
    bool probe = mh == 0;                                                                    // the run leaves the window
    uint32_t rhi = probe ? 63u : (uint32_t)__builtin_ctzll(mh);
    if (base + rhi >= d.n_blocks) rhi = d.n_blocks - 1 - base;
    const uint32_t w_endw = win.ids_woff + packed_words(win.n_ids_bits & 0xFFFF, win.n_ids_bits >> 16);
    if (!probe && (d.flags & LIST_HAS_BREAKS)) {
        const uint32_t nxt_woff = (uint32_t)__shfl(win.ids_woff, (int)((lane + 1) & 63));
        if (__ballot((lane >= rlo && lane < rhi && w_endw != nxt_woff) ? 1 : 0) != 0) probe = true;
    }
    const uint32_t w_begin = (uint32_t)__shfl(win.ids_woff, (int)rlo);
    const uint32_t W = (uint32_t)__shfl(w_endw, (int)rhi) - w_begin;
    if (!probe && W > TILE) probe = true;
    if (probe) { if (want) found = probe_list(ix, d, id, p); return; }                       // (uniform decision; no barrier taken)
    // the run's ids -> LDS (one coalesced range), its block table -> LDS
    const uint32_t* __restrict__ src = ix.ids_payload + d.ids_base + w_begin;
    __syncthreads();                                                                         // (the previous field's searches have left the tile)
    // LDS-DMA, every slab of the run in flight at once (a load -> ds_write loop keeps ONE load per thread in flight: 16 round trips for a 16 KB
    // run); slabs past the run's end read the arena's padding (KW_TILE_OVERREAD_WORDS) and are never searched
    {
        const uint32_t* lane_src = src + t;
        uint32_t* lds_wave_base = sm.btile + (t >> 6) * 64;
        if (W <= 2u * KW_THREADS) kw_glds_slabs<2>(lane_src, lds_wave_base);
        else {
            kw_glds_slabs<8>(lane_src, lds_wave_base);
            if constexpr (TILE > 8u * KW_THREADS) { if (W > 8u * KW_THREADS) kw_glds_slabs<(int)(TILE / KW_THREADS) - 8>(lane_src + 8 * KW_THREADS, lds_wave_base + 8 * KW_THREADS); }
        }
    }
    if (t < 64) { sm.bw_last[0][t] = win.last_id; sm.bw_first[0][t] = win.first_id; sm.bw_woff[0][t] = win.ids_woff - w_begin; sm.bw_nb[0][t] = win.n_ids_bits; }
    kw_glds_wait();
    __syncthreads();
    if (!want) return;
    // (a) which block of the run: branch-free lower bound over the run's last ids
    uint32_t pos = rlo;
    const uint32_t span = rhi - rlo;
    if (span) {
        for (uint32_t step = 1u << (31 - __builtin_clz(span)); step > 0; step >>= 1) {
            const uint32_t j = pos + step;
            const uint32_t v = sm.bw_last[0][(j <= rhi ? j : rhi) - 1];
            pos = (j <= rhi && v < id) ? j : pos;
        }
    }
    const uint32_t b_first = sm.bw_first[0][pos], b_last = sm.bw_last[0][pos];
    if (id < b_first || id > b_last) return;
    // (b) which slot of the block
    const uint32_t nb = sm.bw_nb[0][pos], n = nb & 0xFFFF, target = id - b_first;
    const uint32_t* __restrict__ tw = sm.btile + sm.bw_woff[0][pos];
    uint32_t sl = 0, hit;
    if ((nb >> 16) == 16) {
        const uint16_t* __restrict__ a16 = (const uint16_t*)tw;
#pragma unroll
        for (uint32_t step = 128; step > 0; step >>= 1) { const uint32_t j = sl + step; const uint32_t v = a16[(j <= n ? j : n) - 1]; sl = (j <= n && v < target) ? j : sl; }
        hit = a16[sl < n ? sl : n - 1];
    } else {
#pragma unroll
        for (uint32_t step = 128; step > 0; step >>= 1) { const uint32_t j = sl + step; const uint32_t v = tw[(j <= n ? j : n) - 1]; sl = (j <= n && v < target) ? j : sl; }
        hit = tw[sl < n ? sl : n - 1];
    }
    if (sl < n && hit == target) { found = true; p = (base + pos) * BLOCK_IDS + sl; }
}

// ------------------------------------------------------------------------------------------------
// Multi-field queries (query_by = f0,f1,..): work item = (query, one field's list of the DRIVER token, block range). Thread t
// takes id t of the driver block; an id also present in an EARLIER field's list of the driver token is left to that field's
// work items (every document of the union is produced exactly once); the other tokens are probed in every field (a token is
// satisfied by any field, include/or_iterator.h + src/or_iterator.cpp:95-171); complete hits carry their position in every
// (token, field) list into the shared score stage. Per-candidate probes, no block merge: the slow, general path.
// DEFER = true: the find half of the two-kernel form (records of 1 + TMAX x KW_MAX_FIELDS words -> kw_score_kernel<.., MF = true>)
template <int TMAX, int CAP, bool DEFER = false, bool VQ = false>
__global__ __launch_bounds__(KW_THREADS) void kw_search_mf_kernel(IndexView ix, const KwQueryDev* __restrict__ queries,
                                                                   const KwWorkItem* __restrict__ work, KwPartials part,
                                                                   const uint32_t* __restrict__ aux_ids, uint32_t* __restrict__ ids_out,
                                                                   uint32_t* __restrict__ hits_all, const uint64_t* __restrict__ hit_off) {
    __shared__ KwSmem<TMAX, CAP, true, true, DEFER> sm;
    __shared__ KwQueryDev sq;
    __shared__ KwQueryMF smf;
    const uint32_t t = threadIdx.x;
    const KwWorkItem wi = work[blockIdx.x];
    const uint32_t qi = wi.query & 0x0FFFFFFFu, fdrv = wi.query >> 28;
    {
        const uint32_t* src = (const uint32_t*)(queries + qi);
        uint32_t* dst = (uint32_t*)&sq;
        for (uint32_t i = t; i < sizeof(KwQueryDev) / 4; i += KW_THREADS) dst[i] = src[i];
    }
    if (t == 0) {
        sm.q1_cnt = 0; sm.qf_cnt = 0; sm.tk_cnt = 0; sm.have_thr = 0; sm.n_match = 0; sm.n_emit = 0; sm.off_words = 0;
        sm.f_first = 1; sm.f_frank = 0; sm.f_rp = 0; sm.f_ep = 0; sm.f_c0 = 0; sm.f_c1 = 0; sm.f_cnt0 = 0; sm.f_cnt1 = 0;
    }
    __syncthreads();
    {
        const uint32_t* src = (const uint32_t*)(ix.mf + sq.mf_index);
        uint32_t* dst = (uint32_t*)&smf;
        for (uint32_t i = t; i < sizeof(KwQueryMF) / 4; i += KW_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const KwQueryDev& q = sq;
    const KwQueryMF& mf = smf;
    const uint32_t T = q.n_lists, F = mf.n_fields, td = mf.driver_token;
    const ListDesc dA = ix.lists[mf.list[td][fdrv]];
    const BlockIds* __restrict__ biA = ix.blk_ids + dA.blk_base;
    const uint32_t* __restrict__ idwA = ix.ids_payload + dA.ids_base;
    uint32_t* my_ids_out = ids_out ? ids_out + q.ids_out_off + wi.ids_out_off : nullptr;
    constexpr int NP = TMAX * KW_MAX_FIELDS;
    uint32_t* __restrict__ hits = DEFER ? hits_all + hit_off[blockIdx.x] * (uint64_t)(NP + 1) : nullptr;
    uint32_t qfn = 0, par = 0, q1n = 0;
    uint32_t cur[KW_MAX_FIELDS];                               // the second token's lists: first block that can still hold an id >= the driver block's first
#pragma unroll
    for (int f = 0; f < KW_MAX_FIELDS; f++) cur[f] = 0;
    const uint32_t ts = mf.second_token;

    // Stage 2 on the first n_take queued stage-1 survivors, with FULL wavefronts (per driver block only a handful of the 256 candidates survive:
    // probing the remaining lists right there left ~10 lanes waiting on six dependent global loads per probe): the other tokens in every field,
    // then the driver token's other fields (an id an EARLIER field's list of the driver token holds is left to that field's work items: every
    // document of the union is produced once). Complete hits leave in queue order (= ascending id).
    auto stage2 = [&](uint32_t n_take) {
        bool ok = t < n_take;
        uint32_t id = 0xFFFFFFFFu;
        uint32_t pos[NP];
#pragma unroll
        for (int k = 0; k < NP; k++) pos[k] = KW_NONE;
        auto set_pos = [&](uint32_t idx, uint32_t v) {             // (unrolled selects: a dynamically indexed register array would live in scratch)
#pragma unroll
            for (int k = 0; k < NP; k++) if ((uint32_t)k == idx) pos[k] = v;
        };
        if (ok) {
            id = sm.q1_id[t];
            set_pos(td * KW_MAX_FIELDS + fdrv, sm.q1_p0[t]);
            if (ts != KW_NONE) {
                set_pos(ts * KW_MAX_FIELDS + 0, sm.q1_p1[t]);
#pragma unroll
                for (int f = 1; f < KW_MAX_FIELDS; f++) if ((uint32_t)f < F) set_pos(ts * KW_MAX_FIELDS + f, sm.q1_px[f - 1][t]);
            }
#pragma unroll
            for (int tt = 0; tt < TMAX; tt++) {
                if ((uint32_t)tt < T && (uint32_t)tt != td && (uint32_t)tt != ts && ok) {
                    bool any = false;
#pragma unroll
                    for (int f = 0; f < KW_MAX_FIELDS; f++) {
                        if ((uint32_t)f < F) {
                            const uint32_t h = mf.list[tt][f];
                            uint32_t pp;
                            if (h != KW_NONE && probe_list(ix, ix.lists[h], id, pp)) { any = true; pos[tt * KW_MAX_FIELDS + f] = pp; }
                        }
                    }
                    ok = ok && (any || (uint32_t)tt >= q.n_required);      // (a dropped token is probed, not required)
                }
            }
#pragma unroll
            for (int f = 0; f < KW_MAX_FIELDS; f++) {
                if ((uint32_t)f < F && (uint32_t)f != fdrv && ok) {
                    const uint32_t h = mf.list[td][f];
                    uint32_t pp;
                    if (h != KW_NONE && probe_list(ix, ix.lists[h], id, pp)) {
                        if ((uint32_t)f < fdrv) ok = false;
                        else set_pos(td * KW_MAX_FIELDS + f, pp);
                    }
                }
            }
        }
        uint32_t total;
        const uint32_t my = block_compact1(ok, sm.wave_cnt2[par], total);
        par ^= 1;
        if constexpr (DEFER) {
            if (ok) {
                uint32_t* __restrict__ d = hits + (size_t)(qfn + my) * (NP + 1);
                d[0] = id;
#pragma unroll
                for (int k = 0; k < NP; k++) d[1 + k] = pos[k];
            }
            qfn += total;
        } else {
            if (ok) {
                const uint32_t slot = qfn + my;
                sm.qf_id[slot] = id;
#pragma unroll
                for (int k = 0; k < NP; k++) sm.qf_pos[k][slot] = pos[k];
            }
            qfn += total;
            if (qfn >= KW_THREADS) {
                __syncthreads();
                if (t == 0) sm.qf_cnt = qfn;
                __syncthreads();
                while (sm.qf_cnt >= KW_THREADS) kw_score_stage<TMAX, CAP, true, true, false, false, VQ>(sm, ix, q, KW_THREADS, aux_ids, my_ids_out, 0u);
                qfn = sm.qf_cnt;
            }
        }
        // drop the processed head of the queue
        const uint32_t rest = q1n - n_take;
        uint32_t a = 0, b2 = 0, c[KW_MAX_FIELDS];
#pragma unroll
        for (int f = 0; f < KW_MAX_FIELDS; f++) c[f] = 0;
        __syncthreads();                                           // (every thread has read its entry)
        if (t < rest) {
            a = sm.q1_id[n_take + t]; b2 = sm.q1_p0[n_take + t]; c[0] = sm.q1_p1[n_take + t];
#pragma unroll
            for (int f = 1; f < KW_MAX_FIELDS; f++) c[f] = sm.q1_px[f - 1][n_take + t];
        }
        __syncthreads();
        if (t < rest) {
            sm.q1_id[t] = a; sm.q1_p0[t] = b2; sm.q1_p1[t] = c[0];
#pragma unroll
            for (int f = 1; f < KW_MAX_FIELDS; f++) sm.q1_px[f - 1][t] = c[f];
        }
        q1n = rest;
        __syncthreads();
    };

    // driver-list metadata in a lane-resident window (as kw_find2_kernel: a per-block uniform load is a memory round trip exposed per block), and the
    // NEXT block's ids requested at the top of this block's stage 1 (their latency runs beside the tile DMA's instead of in front of it)
    const uint32_t lane_a = t & 63;
    uint32_t abase = wi.blk_begin;
    auto load_awin = [&](uint32_t base) -> BlockIds { const uint32_t bb = base + lane_a; return biA[bb < wi.blk_end ? bb : wi.blk_end - 1]; };
    BlockIds awin = load_awin(abase);
    auto meta_a = [&](uint32_t bb) -> BlockIds {        // bb uniform; abase <= min(bb, blk_end - 1) < abase + 64
        const int j = (int)((bb < wi.blk_end ? bb : wi.blk_end - 1) - abase);
        BlockIds m;
        m.first_id = (uint32_t)__builtin_amdgcn_readlane((int)awin.first_id, j); m.last_id = (uint32_t)__builtin_amdgcn_readlane((int)awin.last_id, j);
        m.ids_woff = (uint32_t)__builtin_amdgcn_readlane((int)awin.ids_woff, j); m.n_ids_bits = (uint32_t)__builtin_amdgcn_readlane((int)awin.n_ids_bits, j);
        return m;
    };
    auto load_raw = [&](const BlockIds& m) -> uint32_t {
        const uint32_t n = m.n_ids_bits & 0xFFFF, s2 = t < n ? t : 0;
        const uint32_t* __restrict__ w = idwA + m.ids_woff;
        return (m.n_ids_bits >> 16) == 16 ? (uint32_t)((const uint16_t*)w)[s2] : w[s2];
    };
    const bool has_deadline = q.deadline_rem_us != 0;
    BlockIds mA = meta_a(wi.blk_begin), mN = meta_a(wi.blk_begin + 1);
    uint32_t araw = load_raw(mA);
    for (uint32_t b = wi.blk_begin; b < wi.blk_end; b++) {
        if (has_deadline && ((b - wi.blk_begin) & 15) == 0 && kw_out_of_time(ix, q, qi, &sm.stop)) break;
        const uint32_t m_n = mA.n_ids_bits & 0xFFFF;
        bool ok = t < m_n;
        const uint32_t id = ok ? mA.first_id + araw : 0xFFFFFFFFu;
        const uint32_t araw_n = b + 1 < wi.blk_end ? load_raw(mN) : 0u;
        // stage 1 — the SECOND token (fewest postings after the driver's), every field, every candidate of the block: block-level merge through the LDS tile
        uint32_t ps[KW_MAX_FIELDS];
#pragma unroll
        for (int f = 0; f < KW_MAX_FIELDS; f++) ps[f] = KW_NONE;
        if (ts != KW_NONE) {
            bool any = false;
#pragma unroll
            for (int f = 0; f < KW_MAX_FIELDS; f++) {
                if ((uint32_t)f < F) {
                    const uint32_t h = mf.list[ts][f];
                    if (h != KW_NONE) {                                                  // (uniform)
                        bool fnd; uint32_t pp = KW_NONE;
                        kw_mf_merge_field(sm, ix, ix.lists[h], cur[f], mA.first_id, mA.last_id, ok, id, fnd, pp);
                        if (ok && fnd) { any = true; ps[f] = pp; }
                    }
                }
            }
            ok = ok && any;
        }
        // survivors -> the queue (block order = ascending id)
        uint32_t total;
        const uint32_t my = block_compact1(ok, sm.wave_cnt2[par], total);
        par ^= 1;
        if (ok) {
            const uint32_t slot = q1n + my;
            sm.q1_id[slot] = id; sm.q1_p0[slot] = b * BLOCK_IDS + t; sm.q1_p1[slot] = ps[0];
#pragma unroll
            for (int f = 1; f < KW_MAX_FIELDS; f++) sm.q1_px[f - 1][slot] = ps[f];
        }
        q1n += total;
        if (q1n >= (uint32_t)KW_THREADS) { __syncthreads(); stage2(KW_THREADS); }      // (the queue holds 512: < 256 left over + one block's survivors)
        if (b + 3 >= abase + 64 && b + 2 < wi.blk_end) { abase = b + 2; awin = load_awin(abase); }
        mA = mN; mN = meta_a(b + 2); araw = araw_n;
    }
    __syncthreads();
    while (q1n > 0) stage2(q1n < (uint32_t)KW_THREADS ? q1n : (uint32_t)KW_THREADS);
    if constexpr (DEFER) {
        if (t == 0) part.cnt[blockIdx.x] = qfn;                     // hits handed to kw_score_kernel
        return;
    } else {
    __syncthreads();
    if (t == 0) sm.qf_cnt = qfn;
    __syncthreads();
    while (sm.qf_cnt > 0) kw_score_stage<TMAX, CAP, true, true, false, false, VQ>(sm, ix, q, sm.qf_cnt < KW_THREADS ? sm.qf_cnt : KW_THREADS, aux_ids, my_ids_out, 0u);
    topk_compact<CAP, decltype(sm)::HAS_S2>(sm.tk, &sm.tk_cnt, q.k, sm.thr, &sm.have_thr);
    const uint32_t n = sm.tk_cnt;
    const size_t base = (size_t)blockIdx.x * part.k_stride;
    for (uint32_t i = t; i < n; i += KW_THREADS) {
        part.s0[base + i] = sm.tk.s0[i]; part.s1[base + i] = sm.tk.s1[i]; part.s2[base + i] = sm.tk.s2[sm.tk.i2(i)]; part.key[base + i] = sm.tk.key[i];
    }
    if (t == 0) {
        part.cnt[blockIdx.x] = n;
        part.n_emit[blockIdx.x] = sm.n_emit;
        part.off_words[blockIdx.x] = sm.off_words;
        part.n_match[blockIdx.x] = q.n_filt ? sm.f_cnt0 : sm.n_match;
    }
    }
}

// ------------------------------------------------------------------------------------------------
// Wildcard search (q = "*", Index::search_wildcard, src/index.cpp:6616-6818): every filter id (every seq_id
// without a filter) minus the excluded ids is ranked by its sort keys alone — the text-match slot is the constant 100
// (compute_sort_scores(..., 100, ...), :6728-6730, sign-flipped for ASC, no :5541 override) — into a Topster. The reference
// splits the id array over threads and merges per-thread Topsters; here a work item = 256-id blocks [blk_begin, blk_end) of the
// id array, partial top-K per work item, kw_merge_kernel folds them. A pure column gather: one 8-byte load per id and key.
template <int CAP, bool VQ = false>            // VQ: some query of the launch has a TSGPU_SORT_VECTOR_QUERY slot (kw_vq_sort.hip.h)
__global__ __launch_bounds__(KW_THREADS) void kw_wildcard_kernel(IndexView ix, const KwQueryDev* __restrict__ queries,
                                                                  const KwWorkItem* __restrict__ work, KwPartials part,
                                                                  const uint32_t* __restrict__ aux_ids, uint32_t* __restrict__ ids_out) {
    __shared__ TopkLds<CAP> tk;
    __shared__ int64_t thr[4];
    __shared__ uint32_t s_cnt, s_have, s_emit, s_stop, wave_cnt[KW_THREADS / 64];
    __shared__ KwQueryDev sq;
    const uint32_t t = threadIdx.x;
    const KwWorkItem wi = work[blockIdx.x];
    {
        const uint32_t* src = (const uint32_t*)(queries + wi.query);
        uint32_t* dst = (uint32_t*)&sq;
        for (uint32_t i = t; i < sizeof(KwQueryDev) / 4; i += KW_THREADS) dst[i] = src[i];
    }
    if (t == 0) { s_cnt = 0; s_have = 0; s_emit = 0; }
    __syncthreads();
    const KwQueryDev& q = sq;
    const uint32_t* ex = aux_ids + q.aux_off;
    const uint32_t* fl = q.wild_ids ? (const uint32_t*)q.wild_ids : ex + q.n_excl;
    uint32_t* my_ids_out = ids_out ? ids_out + q.ids_out_off + wi.ids_out_off : nullptr;
    for (uint32_t b = wi.blk_begin; b < wi.blk_end; b++) {
        if (((b - wi.blk_begin) & 15) == 0 && kw_out_of_time(ix, q, wi.query, &s_stop)) break;
        if (s_cnt + KW_THREADS > (uint32_t)CAP) topk_compact<CAP, true>(tk, &s_cnt, q.k, thr, &s_have);
        const uint32_t idx = b * BLOCK_IDS + t;
        bool emit = idx < q.wild_n_ids;
        uint32_t seq_id = 0;
        ScoredHit h;
        h.s0 = h.s1 = h.s2 = h.text_match = 0; h.off_words = 0;
        if (emit) {
            seq_id = q.n_filt ? fl[idx] : idx + q.wild_base;
            if (q.n_excl) {      // get_n_ids skips exclude_token_ids (:6674-6676)
                uint32_t lo = 0, hi = q.n_excl;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ex[mid] < seq_id) lo = mid + 1; else hi = mid; }
                if (lo < q.n_excl && ex[lo] == seq_id) emit = false;
            }
            float vd = 0.0f;
            if (emit && q.vdist) {           // flat vector branch: the id's exact distance, abs() for cosine, the threshold (:3699-3704)
                vd = ((const float*)q.vdist)[idx];
                if (q.vdist_abs) vd = fabsf(vd);
                if (vd != vd || vd > q.vdist_thr) emit = false;
            }
            if (emit) h = sort_scores(ix, q, seq_id, q.wild_tm ? (uint64_t)((const int64_t*)q.wild_tm)[idx] : (q.vdist ? 0 : 100), 0, false, vd);      // (text-match slot: 100 for q=*, 0 in the vector branch :3711, the id's phrase score :6050)
        }
        if constexpr (VQ) wave_vq_sort_patch(ix, q, seq_id, emit, h);
        uint32_t total;
        const uint32_t my = block_compact(emit, wave_cnt, total);
        if (emit && my_ids_out) my_ids_out[s_emit + my] = seq_id;
        if (emit) {
            const bool pass = !s_have || ent_greater(h.s0, h.s1, h.s2, (int64_t)seq_id, thr[0], thr[1], thr[2], thr[3]);
            if (pass) {
                const uint32_t slot = atomicAdd(&s_cnt, 1u);
                tk.s0[slot] = h.s0; tk.s1[slot] = h.s1; tk.s2[slot] = h.s2; tk.key[slot] = (int64_t)seq_id;
            }
        }
        __syncthreads();
        if (t == 0) s_emit += total;
        __syncthreads();
    }
    topk_compact<CAP, true>(tk, &s_cnt, q.k, thr, &s_have);
    const uint32_t n = s_cnt;
    const size_t base = (size_t)blockIdx.x * part.k_stride;
    for (uint32_t i = t; i < n; i += KW_THREADS) {
        part.s0[base + i] = tk.s0[i]; part.s1[base + i] = tk.s1[i]; part.s2[base + i] = tk.s2[i]; part.key[base + i] = tk.key[i];
    }
    if (t == 0) { part.cnt[blockIdx.x] = n; part.n_match[blockIdx.x] = s_emit; part.n_emit[blockIdx.x] = s_emit; part.off_words[blockIdx.x] = 0; }
}

// flat vector branch: KV::vector_distance of the merged hits (kv.vector_distance = vec_dist_score, src/index.cpp:3717) — the hit's seq_id is
// looked up in the query's filter ids, whose index addresses the distance array. grid = queries.
__global__ __launch_bounds__(KW_THREADS) void kw_vflat_distance_kernel(const KwQueryDev* __restrict__ queries, const uint32_t* __restrict__ aux_ids, KwOut out) {
    const KwQueryDev& q = queries[blockIdx.x];
    if (!q.vdist || !out.vector_distance) return;
    const uint32_t* fl = aux_ids + q.aux_off + q.n_excl;
    const uint32_t nh = out.n_hits[blockIdx.x], n = nh < out.k_stride ? nh : out.k_stride;
    const size_t ob = (size_t)blockIdx.x * out.k_stride;
    for (uint32_t i = threadIdx.x; i < n; i += KW_THREADS) {
        const uint32_t key = (uint32_t)out.keys[ob + i];
        uint32_t lo = 0, hi = q.n_filt;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (fl[mid] < key) lo = mid + 1; else hi = mid; }
        float d = lo < q.n_filt ? ((const float*)q.vdist)[lo] : -1.0f;
        if (q.vdist_abs) d = fabsf(d);
        out.vector_distance[ob + i] = d;
    }
}

// num_keyword_matches of a FILTERED query (include/or_iterator.h:61-182 with istate.filter_ids): the reference counts the
// intersection ids its loop lands on, and after every non-excluded one it skips all lists to the next filter id. So an
// intersection id x_j is counted iff a filter id lies in (x_{j-1}, x_j] — its filter rank exceeds its predecessor's — or the
// previous visited id was excluded (then the loop just advances to the next intersection id). Every work item (a contiguous
// slice of the intersection) reports its count for both possible states of its first hit; this chains the slices in order.
__device__ inline unsigned long long kw_filter_count(const KwPartials& part, uint32_t first_work, uint32_t n_work) {
    unsigned long long total = 0;
    uint32_t r_prev = 0, carry = 0;
    for (uint32_t w = first_work; w < first_work + n_work; w++) {
        const uint32_t fl = part.fflags[w];
        if (!(fl & 1u)) continue;                                  // no hit in this slice: the state carries over
        const uint32_t u = (part.first_rank[w] > r_prev ? 1u : 0u) | carry;
        total += u ? part.n_match1[w] : part.n_match[w];
        carry = u ? (fl >> 2) & 1u : (fl >> 1) & 1u;
        r_prev = part.last_rank[w];
    }
    return total;
}

// Every partial list is SORTED (KV::is_greater order) and keys are unique, so folding one into the running top-k is a merge
// by rank, not a sort: an entry's place = its index in its own list + the number of entries of the other list that are
// greater (one binary search). A = tk[0, na) sorted; the partial comes in pieces of <= 256 entries parked in tk[CAP-256, CAP)
// (k <= CAP - 256): ~10 dependent LDS steps per piece instead of a 45-stage bitonic sort. A partial whose best remaining entry
// cannot beat the current k-th is skipped. Folds partial lists [first, first + n) into tk; returns the number of entries held.
template <int CAP>
__device__ inline uint32_t kw_fold_partials(TopkLds<CAP>& tk, const KwPartials& part, uint32_t first, uint32_t n_lists, uint32_t k) {
    constexpr int PER = CAP / KW_THREADS - 1;                    // A entries per thread (na <= k <= CAP - 256)
    constexpr int PB = CAP - KW_THREADS;                         // where the piece is parked
    const uint32_t t = threadIdx.x;
    uint32_t na = 0;
    // Two-stage software pipeline over the lists: a list's first 256 entries (all of it up to k = 256) and the count of the list after
    // it are requested one list ahead — a fold is a chain of short LDS phases behind a global-memory round trip per list otherwise.
    uint32_t nw = n_lists ? part.cnt[first] : 0, nw_next = n_lists > 1 ? part.cnt[first + 1] : 0;
    int64_t c0 = 0, c1 = 0, c2 = 0, ck = -1;
    if (t < nw) { const size_t e = (size_t)first * part.k_stride + t; c0 = part.s0[e]; c1 = part.s1[e]; c2 = part.s2[e]; ck = part.key[e]; }
    for (uint32_t li = 0; li < n_lists; li++) {
        const uint32_t w = first + li;
        const size_t base = (size_t)w * part.k_stride;
        int64_t n0 = 0, n1 = 0, n2 = 0, nk = -1;
        if (li + 1 < n_lists && t < nw_next) { const size_t e = (size_t)(w + 1) * part.k_stride + t; n0 = part.s0[e]; n1 = part.s1[e]; n2 = part.s2[e]; nk = part.key[e]; }
        const uint32_t nw_after = li + 2 < n_lists ? part.cnt[w + 2] : 0;
        for (uint32_t p0 = 0; p0 < nw; p0 += KW_THREADS) {
            const uint32_t nb = nw - p0 < (uint32_t)KW_THREADS ? nw - p0 : (uint32_t)KW_THREADS;
            int64_t b0 = c0, b1 = c1, b2 = c2, bk = ck;
            if (p0 > 0) {                                        // (k > 256 only: later pieces of a list are fetched on demand)
                b0 = 0; b1 = 0; b2 = 0; bk = -1;
                if (t < nb) { b0 = part.s0[base + p0 + t]; b1 = part.s1[base + p0 + t]; b2 = part.s2[base + p0 + t]; bk = part.key[base + p0 + t]; }
            }
            if (t < nb) { tk.s0[PB + t] = b0; tk.s1[PB + t] = b1; tk.s2[PB + t] = b2; tk.key[PB + t] = bk; }
            __syncthreads();
            if (na == k && !ent_greater(tk.s0[PB], tk.s1[PB], tk.s2[PB], tk.key[PB], tk.s0[na - 1], tk.s1[na - 1], tk.s2[na - 1], tk.key[na - 1])) {
                __syncthreads();                                 // (uniform) the piece's best entry cannot enter: neither can the rest of the list
                break;
            }
            // piece entry t: place = t + #{A entries greater than it}
            uint32_t rank_b = 0xFFFFFFFFu;
            if (t < nb) {
                uint32_t lo = 0, hi = na;                        // first A index that is NOT greater than b
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (ent_greater(tk.s0[mid], tk.s1[mid], tk.s2[mid], tk.key[mid], b0, b1, b2, bk)) lo = mid + 1; else hi = mid;
                }
                rank_b = t + lo;
            }
            // A entry i: place = i + #{piece entries greater than it}
            int64_t a0[PER], a1[PER], a2[PER], ak[PER];
            uint32_t rank_a[PER];
#pragma unroll
            for (int r = 0; r < PER; r++) {
                const uint32_t i = r * KW_THREADS + t;
                rank_a[r] = 0xFFFFFFFFu;
                if (i < na) {
                    a0[r] = tk.s0[i]; a1[r] = tk.s1[i]; a2[r] = tk.s2[i]; ak[r] = tk.key[i];
                    uint32_t lo = 0, hi = nb;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (ent_greater(tk.s0[PB + mid], tk.s1[PB + mid], tk.s2[PB + mid], tk.key[PB + mid], a0[r], a1[r], a2[r], ak[r])) lo = mid + 1; else hi = mid;
                    }
                    rank_a[r] = i + lo;
                }
            }
            __syncthreads();                                     // every read of the old layout is done
            if (rank_b < k) { tk.s0[rank_b] = b0; tk.s1[rank_b] = b1; tk.s2[rank_b] = b2; tk.key[rank_b] = bk; }
#pragma unroll
            for (int r = 0; r < PER; r++)
                if (rank_a[r] < k) { tk.s0[rank_a[r]] = a0[r]; tk.s1[rank_a[r]] = a1[r]; tk.s2[rank_a[r]] = a2[r]; tk.key[rank_a[r]] = ak[r]; }
            na = na + nb < k ? na + nb : k;
            __syncthreads();
        }
        c0 = n0; c1 = n1; c2 = n2; ck = nk;
        nw = nw_next; nw_next = nw_after;
    }
    return na;
}

// First level of a TWO-LEVEL merge (queries cut into many work items — small batches are cut fine so that no work item runs long):
// group g folds the partial lists [first, first + n) of one query into the sorted list `dst`, all groups in parallel; kw_merge_kernel
// then folds a query's group lists. A chain of P sequential folds becomes G + P / G.
struct KwMergeGroup { uint32_t query, first, n, dst; };
template <int CAP>
__global__ __launch_bounds__(KW_THREADS) void kw_merge_groups_kernel(const KwQueryDev* __restrict__ queries, KwPartials part, const KwMergeGroup* __restrict__ groups) {
    __shared__ TopkLds<CAP> tk;
    const KwMergeGroup g = groups[blockIdx.x];
    const uint32_t k = queries[g.query].k;
    const uint32_t n = kw_fold_partials<CAP>(tk, part, g.first, g.n, k);
    const size_t base = (size_t)g.dst * part.k_stride;
    for (uint32_t i = threadIdx.x; i < n; i += KW_THREADS) {
        part.s0[base + i] = tk.s0[i]; part.s1[base + i] = tk.s1[i]; part.s2[base + i] = tk.s2[i]; part.key[base + i] = tk.key[i];
    }
    if (threadIdx.x == 0) part.cnt[g.dst] = n;
}

// SELECT instead of fold, for a query cut into many work items (small batches are cut fine so that no work item runs long): the top k
// of P sorted lists without touching most of their entries, at a cost that does not grow with P (a fold per list does).
//   1. every list offers a PREFIX of ~2k / P entries; the union of the prefixes (<= 1 024 entries) is sorted in LDS: its k-th largest
//      entry tau is a lower bound of the k-th best overall (k real entries are >= tau);
//   2. per list a binary search counts its entries >= tau (one thread per list) — the prefixes' share of them is exactly k, the rest
//      comes from lists whose whole prefix beat tau; these candidates (typically k .. 1.5 k) are gathered and sorted: the first k are
//      the result (keys are unique: no ties).
// Returns false (nothing written) when prefixes or candidates do not fit the LDS buffer: the caller folds the lists instead.
// exclusive prefix sums of in[0 .. n) (n <= 2 * KW_THREADS, LDS) into out[0 .. n], out[n] = total; wsum: [KW_THREADS / 64] scratch.
// Every thread of the block calls it. (A single thread walking 384 LDS words costs ~11 us at one wave per SIMD; this is ~1 us.)
__device__ inline void block_excl_scan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* wsum) {
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t a = 2 * t < n ? in[2 * t] : 0u, b = 2 * t + 1 < n ? in[2 * t + 1] : 0u;
    uint32_t incl = a + b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < KW_THREADS / 64; w++) { const uint32_t c = wsum[w]; if ((uint32_t)w < wave) base += c; tot += c; }
    const uint32_t ex = base + incl - (a + b);
    if (2 * t < n) out[2 * t] = ex;
    if (2 * t + 1 < n) out[2 * t + 1] = ex + a;
    if (t == 0) out[n] = tot;
    __syncthreads();
}
static const int KW_SEL_PMAX = 384;                      // lists per query (planner: max_partials <= 384)
static const int KW_SEL_CCAP = 1024;                     // entries the LDS buffer holds
struct KwSelectLds {
    TopkLds<KW_SEL_CCAP, true> cb;
    uint32_t cnt[KW_SEL_PMAX], take[KW_SEL_PMAX], off[KW_SEL_PMAX + 1], wsum[KW_THREADS / 64];
    uint32_t total, n_nonempty, ok;
    int64_t tau[4];
};
__device__ inline bool kw_select_partials(KwSelectLds& sl, const KwPartials& part, uint32_t first, uint32_t P, uint32_t k, const KwOut& out, size_t ob, int msi,
                                          uint32_t& n_out) {
    const uint32_t t = threadIdx.x;
    if (t == 0) sl.ok = 1;
    uint32_t my_nne = 0;
    for (uint32_t w = t; w < P; w += KW_THREADS) {
        const uint32_t c = part.cnt[first + w];
        sl.cnt[w] = c;
        sl.take[w] = c ? 1u : 0u;
        my_nne += c ? 1u : 0u;
    }
    __syncthreads();
    block_excl_scan(sl.cnt, sl.off, P, sl.wsum);
    if (t == 0) sl.total = sl.off[P];
    block_excl_scan(sl.take, sl.off, P, sl.wsum);
    if (t == 0) sl.n_nonempty = sl.off[P];
    __syncthreads();
    (void)my_nne;
    const uint32_t total = sl.total, nne = sl.n_nonempty;
    if (total == 0) { n_out = 0; return true; }
    auto emit = [&](uint32_t i, int64_t a0, int64_t a1, int64_t a2, int64_t ak) {
        out.keys[ob + i] = (uint64_t)ak;
        out.scores[(ob + i) * 3 + 0] = a0; out.scores[(ob + i) * 3 + 1] = a1; out.scores[(ob + i) * 3 + 2] = a2;
        out.text_match[ob + i] = msi == 0 ? a0 : (msi == 1 ? a1 : (msi == 2 ? a2 : 0));
        out.vector_distance[ob + i] = -1.0f;
        out.match_score_index[ob + i] = (int8_t)msi;
    };
    // gathers take[w] leading entries of every list and calls fn(rank, entry) for each with its place in the descending order of the
    // gathered set; returns the count (0 and !ok: more than the buffer holds).
    //   * up to HALF entries: a TREE of pairwise merges by rank. The lists are sorted and keys are unique, so merging two neighbouring
    //     segments moves an entry to (index in its own segment) + (entries of the partner segment that are greater): one LDS binary
    //     search per entry and level, log2(P) levels, one barrier each, ping-pong between the two halves of the buffer; an entry stays
    //     in its thread's registers from the gather to its final rank. (36 lists: 6 levels ~ 1 us each — the bitonic sort of 512 slots
    //     is 45 barrier stages, ~30 us for the ONE workgroup a small round's query has: profiles/r03/exp_concurrency_analysis.txt)
    //   * more: padded to a power of two and sorted (bitonic), as before.
    constexpr uint32_t HALF = KW_SEL_CCAP / 2;
    constexpr int RPT = (int)(HALF / KW_THREADS);
    auto gather_ordered = [&](auto&& fn) -> uint32_t {
        block_excl_scan(sl.take, sl.off, P, sl.wsum);
        if (t == 0 && sl.off[P] > (uint32_t)KW_SEL_CCAP) sl.ok = 0;
        __syncthreads();
        if (!sl.ok) return 0;
        const uint32_t C = sl.off[P];
        if (C <= HALF) {
            int64_t e0[RPT], e1[RPT], e2[RPT], ek[RPT];
            uint32_t ew[RPT], pos[RPT];
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                const uint32_t i = r * KW_THREADS + t;
                pos[r] = i;
                if (i < C) {                             // entry i belongs to the list w with off[w] <= i < off[w + 1]
                    uint32_t lo = 0, hi = P;
                    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sl.off[mid] <= i) lo = mid; else hi = mid; }
                    const size_t e = (size_t)(first + lo) * part.k_stride + (i - sl.off[lo]);
                    ew[r] = lo;
                    e0[r] = part.s0[e]; e1[r] = part.s1[e]; e2[r] = part.s2[e]; ek[r] = part.key[e];
                    sl.cb.s0[i] = e0[r]; sl.cb.s1[i] = e1[r]; sl.cb.s2[i] = e2[r]; sl.cb.key[i] = ek[r];
                }
            }
            __syncthreads();
            uint32_t cur = 0;                            // the half that holds the current level's segments
            for (uint32_t span = 1; span < P; span <<= 1) {          // segments of `span` lists merge pairwise (uniform loop)
#pragma unroll
                for (int r = 0; r < RPT; r++) {
                    if (r * KW_THREADS + t < C) {
                        const uint32_t seg = ew[r] / span, own_list = seg * span, pair_list = (seg & ~1u) * span, other_list = (seg ^ 1u) * span;
                        uint32_t lo = sl.off[other_list < P ? other_list : P], hi = sl.off[other_list + span < P ? other_list + span : P];
                        const uint32_t a = lo;
                        while (lo < hi) {                // first entry of the partner segment that is NOT greater than this one
                            const uint32_t mid = (lo + hi) >> 1;
                            const int64_t m0 = sl.cb.s0[cur + mid];
                            bool gt;
                            if (m0 != e0[r]) gt = m0 > e0[r];
                            else {
                                const int64_t m1 = sl.cb.s1[cur + mid], m2 = sl.cb.s2[cur + mid];
                                gt = m1 != e1[r] ? m1 > e1[r] : (m2 != e2[r] ? m2 > e2[r] : sl.cb.key[cur + mid] > ek[r]);
                            }
                            if (gt) lo = mid + 1; else hi = mid;
                        }
                        pos[r] = sl.off[pair_list] + (pos[r] - sl.off[own_list]) + (lo - a);
                        const uint32_t d = (cur ^ HALF) + pos[r];
                        sl.cb.s0[d] = e0[r]; sl.cb.s1[d] = e1[r]; sl.cb.s2[d] = e2[r]; sl.cb.key[d] = ek[r];
                    }
                }
                __syncthreads();
                cur ^= HALF;
            }
#pragma unroll
            for (int r = 0; r < RPT; r++) if (r * KW_THREADS + t < C) fn(pos[r], e0[r], e1[r], e2[r], ek[r]);
            __syncthreads();                             // (the buffer may be gathered into again)
            return C;
        }
        uint32_t n2 = 2;
        while (n2 < C) n2 <<= 1;
        for (uint32_t i = t; i < n2; i += KW_THREADS) {
            if (i < C) {
                uint32_t lo = 0, hi = P;
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (sl.off[mid] <= i) lo = mid; else hi = mid; }
                const size_t e = (size_t)(first + lo) * part.k_stride + (i - sl.off[lo]);
                sl.cb.s0[i] = part.s0[e]; sl.cb.s1[i] = part.s1[e]; sl.cb.s2[i] = part.s2[e]; sl.cb.key[i] = part.key[e];
            } else sl.cb.key[i] = -1;                    // padding sorts last
        }
        topk_sort<KW_SEL_CCAP, true>(sl.cb, (int)n2);   // (starts and ends with a barrier)
        for (uint32_t i = t; i < C; i += KW_THREADS) fn(i, sl.cb.s0[i], sl.cb.s1[i], sl.cb.s2[i], sl.cb.key[i]);
        __syncthreads();
        return C;
    };
    auto emit_top = [&](uint32_t rank, int64_t a0, int64_t a1, int64_t a2, int64_t ak) { if (rank < k) emit(rank, a0, a1, a2, ak); };
    uint32_t C;
    if (total <= HALF || total <= k) {
        for (uint32_t w = t; w < P; w += KW_THREADS) sl.take[w] = sl.cnt[w];          // few entries altogether: all of them (one tree merge)
        __syncthreads();
        C = gather_ordered(emit_top);
    } else {
        uint32_t m = (2 * k + nne - 1) / nne;            // prefixes: ~2k entries offered in total (total > k)
        // (any prefix length whose union holds k entries gives a valid bound; one that keeps the union within HALF takes the tree path)
        if (m * nne > HALF && (HALF / nne) * nne >= k + k / 4) m = HALF / nne;
        for (uint32_t w = t; w < P; w += KW_THREADS) { const uint32_t c = sl.cnt[w]; sl.take[w] = c < m ? c : m; }
        __syncthreads();
        const uint32_t S = gather_ordered([&](uint32_t rank, int64_t a0, int64_t a1, int64_t a2, int64_t ak) {
            if (rank == k - 1) { sl.tau[0] = a0; sl.tau[1] = a1; sl.tau[2] = a2; sl.tau[3] = ak; } });
        if (!sl.ok) return false;
        const bool bound = S >= k;                       // (S < k: many short lists next to a few long ones — the bound needs k prefix entries)
        if (!bound && total > (uint32_t)KW_SEL_CCAP) return false;
        const int64_t u0 = sl.tau[0], u1 = sl.tau[1], u2 = sl.tau[2], uk = sl.tau[3];         // tau
        for (uint32_t w = t; w < P; w += KW_THREADS) {
            if (!bound) { sl.take[w] = sl.cnt[w]; continue; }       // no bound, but everything fits the buffer: all entries, sorted
            const uint32_t c = sl.cnt[w], mw = c < m ? c : m;
            const size_t base = (size_t)(first + w) * part.k_stride;
            uint32_t lo = 0, hi = c;                     // first index whose entry is LESS than tau (tau itself counts)
            if (mw) {                                    // one probe at the prefix's end: most lists end inside their (short) prefix
                const size_t e = base + mw - 1;
                if (ent_greater(u0, u1, u2, uk, part.s0[e], part.s1[e], part.s2[e], part.key[e])) hi = mw - 1; else lo = mw;
            }
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ent_greater(u0, u1, u2, uk, part.s0[base + mid], part.s1[base + mid], part.s2[base + mid], part.key[base + mid])) hi = mid; else lo = mid + 1;
            }
            sl.take[w] = lo;
        }
        __syncthreads();
        C = gather_ordered(emit_top);
    }
    if (!sl.ok) return false;
    n_out = C < k ? C : k;
    return true;
}

// grid = queries; folds a query's partials into the final order and writes the tsgpu_hits slots
template <int CAP>
__device__ __forceinline__ void kw_merge_body(const KwQueryDev* __restrict__ queries, const KwPartials& part, const KwOut& out, uint32_t select_min, const uint32_t qid) {
    __shared__ TopkLds<CAP> tk;
    __shared__ KwSelectLds sl;
    __shared__ unsigned long long s_nm, s_ow;
    const uint32_t t = threadIdx.x;
    const KwQueryDev q = queries[qid];
    if (t == 0) { s_nm = 0; s_ow = 0; }
    __syncthreads();
    const size_t ob = (size_t)qid * out.k_stride;
    int msi = -1;
    for (int i = 0; i < 3; i++) if (i < q.n_sort && q.sort_kind[i] == 0) msi = i;
    uint32_t n = 0;
    bool selected = false;
    if (select_min && q.m_n >= select_min && q.m_n <= (uint32_t)KW_SEL_PMAX) selected = kw_select_partials(sl, part, q.m_first, q.m_n, q.k, out, ob, msi, n);   // (uniform)
    if (selected) {
    } else if (q.m_n == 1) {
        // a single list already holds the query's final order: copy it through
        const uint32_t w = q.m_first;
        n = part.cnt[w];
        const size_t base = (size_t)w * part.k_stride;
        for (uint32_t i = t; i < n; i += KW_THREADS) {
            const int64_t a0 = part.s0[base + i], a1 = part.s1[base + i], a2 = part.s2[base + i];
            out.keys[ob + i] = (uint64_t)part.key[base + i];
            out.scores[(ob + i) * 3 + 0] = a0; out.scores[(ob + i) * 3 + 1] = a1; out.scores[(ob + i) * 3 + 2] = a2;
            out.text_match[ob + i] = msi == 0 ? a0 : (msi == 1 ? a1 : (msi == 2 ? a2 : 0));
            out.vector_distance[ob + i] = -1.0f;
            out.match_score_index[ob + i] = (int8_t)msi;
        }
    } else {
        n = kw_fold_partials<CAP>(tk, part, q.m_first, q.m_n, q.k);
        for (uint32_t i = t; i < n; i += KW_THREADS) {
            const int64_t a0 = tk.s0[i], a1 = tk.s1[i], a2 = tk.s2[i];
            out.keys[ob + i] = (uint64_t)tk.key[i];
            out.scores[(ob + i) * 3 + 0] = a0; out.scores[(ob + i) * 3 + 1] = a1; out.scores[(ob + i) * 3 + 2] = a2;
            out.text_match[ob + i] = msi == 0 ? a0 : (msi == 1 ? a1 : (msi == 2 ? a2 : 0));
            out.vector_distance[ob + i] = -1.0f;
            out.match_score_index[ob + i] = (int8_t)msi;
        }
    }
    // counters: always from the work items themselves (num_keyword_matches, offsets read); a filtered query chains its slices in id order
    {
        unsigned long long nm = 0, ow = 0;
        const bool chain = q.n_filt && !q.wild_n_ids && q.mf_index == KW_NONE;      // (several fields: order-free count, summed)
        const bool ordered_mf = q.n_filt && q.n_excl && !q.wild_n_ids && q.mf_index != KW_NONE;    // ... with exclusions: kw_mf_ordered_count_kernel's walk
        for (uint32_t w = q.first_work + t; w < q.first_work + q.n_work; w += KW_THREADS) { if (!chain && !ordered_mf) nm += part.n_match[w]; ow += part.off_words[w]; }
        for (int d = 32; d > 0; d >>= 1) { nm += __shfl_down(nm, d, 64); ow += __shfl_down(ow, d, 64); }
        if ((t & 63) == 0) { if (nm) atomicAdd(&s_nm, nm); if (ow) atomicAdd(&s_ow, ow); }
        __syncthreads();
        if (t == 0 && chain) s_nm = kw_filter_count(part, q.first_work, q.n_work);
        if (t == 0 && ordered_mf && q.n_work) s_nm = part.n_match1[q.first_work];
    }
    __syncthreads();
    if (t == 0) { out.n_hits[qid] = n; out.num_matched[qid] = s_nm; out.off_words[qid] = s_ow; }
}
template <int CAP>
__global__ __launch_bounds__(KW_THREADS) void kw_merge_kernel(const KwQueryDev* __restrict__ queries, KwPartials part, KwOut out,
                                                               uint32_t* __restrict__ ids_out, const KwWorkItem* __restrict__ work, uint32_t select_min) {
    kw_merge_body<CAP>(queries, part, out, select_min, blockIdx.x);
    (void)ids_out; (void)work;
}

// ------------------------------------------------------------------------------------------------
// Doc-range shards: exact merge of G gathered per-shard Topster lists into the global order, one workgroup per
// query. Inputs are what an all-gather of tsgpu_hits delivers: arrays laid out [shard][query][k_in]. Keys are unique across
// shards, so sorting by (s0, s1, s2, key) = KV::is_greater reproduces Topster::sort() of the unsharded collection; the origin
// slot rides in the low 16 bits of the packed key so the per-hit payload (text_match, distance, index) follows its hit.
struct KwShardIn {
    const uint64_t* keys; const int64_t* scores; const int64_t* text_match; const float* vector_distance; const int8_t* match_score_index;
    const uint32_t* n_hits; const uint64_t* num_matched;
    uint32_t n_shards, n_queries, k_in;
    // PACKED form (tsgpu_group's exchange buffer): shard g's block = per query k_in x words u64 {key, s0, s1, s2(, text_match)} followed by
    // 3 u64 {n_hits, num_matched, status} — a query's record is contiguous (k_in * words + 3 words), so a RANGE of queries is one
    // contiguous slice (the all-to-all form sends every rank only the queries it merges); blocks are shard_stride words apart; workgroup
    // b reads record b of every block and writes query b + q_out_offset. packed == nullptr: the arrays above.
    const uint64_t* packed; uint64_t shard_stride; uint32_t words; uint32_t q_out_offset;
    // BOUND-PRUNED packed form (pruned_per > 0; kw_group_pack_pruned_kernel): shard g's slice = pruned_per header pairs
    // {n | status << 16 | first entry << 32, num_matched} — one per query of the slice — followed by the slice's entries, `words` u64 each,
    // compact: query b's are entries [first, first + n). Slices are shard_stride words apart.
    uint32_t pruned_per;
    int32_t* status_out;           // (packed form) merged per-query status: the first non-zero status among the shards
    const uint32_t* cap_per_query; // nullable: the merged list of query q holds min(k, cap_per_query[q]) hits (its own Topster's capacity)
};
// this member's top-k of a device-resident result (tsgpu_hits layout, stride k_stride) -> its exchange block (see KwShardIn::packed)
__global__ void kw_group_pack_kernel(KwOut loc, const int32_t* status, uint32_t n_queries, uint32_t k, uint32_t words, uint64_t* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = i / k, j = i - q * k;
    if (q >= n_queries) return;
    const bool failed = status && status[q] != 0;              // a query that was not run may expose stale slots in device outputs
    const uint32_t n = failed ? 0u : (loc.n_hits[q] < k ? loc.n_hits[q] : k);
    const size_t qw = (size_t)k * words + 3;
    uint64_t* d = dst + (size_t)q * qw + (size_t)j * words;
    const size_t src = (size_t)q * loc.k_stride + j;
    const bool live = j < n;
    d[0] = live ? loc.keys[src] : 0;
    d[1] = live ? (uint64_t)loc.scores[src * 3 + 0] : 0; d[2] = live ? (uint64_t)loc.scores[src * 3 + 1] : 0; d[3] = live ? (uint64_t)loc.scores[src * 3 + 2] : 0;
    if (words > 4) d[4] = live && loc.text_match ? (uint64_t)loc.text_match[src] : 0;
    if (j == 0) {
        uint64_t* c = dst + (size_t)q * qw + (size_t)k * words;
        c[0] = n; c[1] = (loc.num_matched && !failed) ? loc.num_matched[q] : 0; c[2] = status ? (uint64_t)(uint32_t)status[q] : 0;
    }
}
// ---- bound-pruned exchange (round 5) ----------------------------------------------------------------------------------------
// A merged list holds kq = min(k, the query's Topster capacity) hits, ordered by KV::is_greater (/root/reference/include/topster.h:146-154; keys
// are unique: a strict total order). Any entry e such that at least kq entries >= e exist in the whole collection is a LOWER BOUND of the global
// kq-th best entry, and nothing below a lower bound can be in the merged list. Every shard reports two of its own entries per query —
//   e_k = its kq-th best (it alone owns kq entries >= e_k), and
//   e_r = its r-th best, r = ceil(1.5 kq / G)   (when the winners are spread over the G shards the global kq-th sits near every shard's (kq / G)-th)
// — and with m = ceil(kq / r):   B[q] = the greater of  max over shards of e_k  and  the m-th largest of the shards' e_r
// (the m shards behind the m largest e_r own at least m x r >= kq entries >= the m-th largest). A shard with too few hits reports "none" (key < 0:
// sorts below everything); when neither bound exists nothing is pruned. Every shard then sends only its entries >= B[q]: about kq .. 1.6 kq per query
// over ALL shards when the winners are spread evenly (instead of G x k), and only the winning shard's when one shard owns them all.
__device__ inline uint32_t kw_group_bound_rank(uint32_t kq, uint32_t n_shards) {           // r: 1 <= r <= kq
    const uint32_t r = (3u * kq + 2u * n_shards - 1u) / (2u * n_shards);
    return r < 1u ? 1u : (r > kq ? kq : r);
}
// (1) this shard's two reported entries per query: kth[q][0] = e_r, kth[q][1] = e_k, each {s0, s1, s2, key} (key = -1: none)
__global__ void kw_group_kth_kernel(KwOut loc, const int32_t* status, const uint32_t* cap_per_query, uint32_t n_queries, uint32_t k, uint32_t n_shards, int64_t* kth) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    const bool failed = status && status[q] != 0;
    const uint32_t n = failed ? 0u : (loc.n_hits[q] < k ? loc.n_hits[q] : k);
    const uint32_t kq = cap_per_query && cap_per_query[q] < k ? cap_per_query[q] : k;
    int64_t* d = kth + (size_t)q * 8;
    const uint32_t want[2] = {kq ? kw_group_bound_rank(kq, n_shards) : 0u, kq};
#pragma unroll
    for (int w = 0; w < 2; w++) {
        if (want[w] == 0 || n < want[w]) { d[4 * w] = 0; d[4 * w + 1] = 0; d[4 * w + 2] = 0; d[4 * w + 3] = -1; continue; }
        const size_t src = (size_t)q * loc.k_stride + (want[w] - 1);
        d[4 * w] = loc.scores[src * 3 + 0]; d[4 * w + 1] = loc.scores[src * 3 + 1]; d[4 * w + 2] = loc.scores[src * 3 + 2]; d[4 * w + 3] = (int64_t)loc.keys[src];
    }
}
// (2) + (3) ONE WAVEFRONT PER QUERY: B[q] from the gathered reports ([shard][query][2][4]); this shard's entries >= B[q] are a PREFIX of its sorted
// list (every lane tests its own entries, one ballot counts them); lane 0 takes their place in the destination slice with one atomicAdd on the slice's
// cursor (queries land in the slice's entry area in arrival order — the header pair says where), the lanes copy them, lane 0 writes the header pair.
// cursor[slice] ends as the slice's entry total (what the exact-size exchange sends). Queries >= n_queries (padding of the last slice): empty headers.
// Slice layout: [per header pairs][entries], slices slice_words apart (capacity: per * k entries).
__global__ __launch_bounds__(256) void kw_group_prune_pack_kernel(KwOut loc, const int32_t* status, const uint32_t* cap_per_query, uint32_t n_queries, uint32_t n_pad, uint32_t k,
                                                                  uint32_t words, const int64_t* kth_all, uint32_t n_shards, uint32_t per, uint64_t slice_words, uint64_t* dst,
                                                                  uint32_t* cursor) {
    const uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (q >= n_pad) return;
    const uint32_t j = q / per, i = q - j * per;
    uint64_t* slice = dst + (size_t)j * slice_words;
    if (q >= n_queries) { if (lane == 0) { slice[(size_t)i * 2] = 0; slice[(size_t)i * 2 + 1] = 0; } return; }
    const bool failed = status && status[q] != 0;
    const uint32_t n = failed ? 0u : (loc.n_hits[q] < k ? loc.n_hits[q] : k);
    const uint32_t kq = cap_per_query && cap_per_query[q] < k ? cap_per_query[q] : k;
    int64_t b0 = 0, b1 = 0, b2 = 0, bk = -1;
    auto rec = [&](uint32_t g, int w) { return kth_all + (((size_t)g * n_queries + q) * 2 + (size_t)w) * 4; };
    for (uint32_t g = 0; g < n_shards; g++) {                  // the single-shard bound: the greatest e_k (uniform loads)
        const int64_t* e = rec(g, 1);
        if (ent_greater(e[0], e[1], e[2], e[3], b0, b1, b2, bk)) { b0 = e[0]; b1 = e[1]; b2 = e[2]; bk = e[3]; }
    }
    if (kq) {                                                  // the spread bound: the m-th largest e_r — lane g ranks shard g's report among the others
        const uint32_t r = kw_group_bound_rank(kq, n_shards), m = (kq + r - 1) / r;
        if (m <= n_shards) {
            for (uint32_t g0 = 0; g0 < n_shards; g0 += 64) {
                const uint32_t g = g0 + lane;
                bool mine = false;
                int64_t e0 = 0, e1 = 0, e2 = 0, e3 = -1;
                if (g < n_shards) {
                    const int64_t* e = rec(g, 0);
                    e0 = e[0]; e1 = e[1]; e2 = e[2]; e3 = e[3];
                    if (e3 >= 0) {
                        uint32_t above = 0;
                        for (uint32_t h = 0; h < n_shards; h++) { const int64_t* f = rec(h, 0); if (h != g && ent_greater(f[0], f[1], f[2], f[3], e0, e1, e2, e3)) above++; }
                        mine = above == m - 1;
                    }
                }
                const unsigned long long who = __ballot(mine ? 1 : 0);
                if (who) {                                     // (keys are unique: at most one report has exactly m - 1 above it)
                    const int src = (int)__builtin_ctzll(who);
                    e0 = __shfl(e0, src); e1 = __shfl(e1, src); e2 = __shfl(e2, src); e3 = __shfl(e3, src);
                    if (ent_greater(e0, e1, e2, e3, b0, b1, b2, bk)) { b0 = e0; b1 = e1; b2 = e2; bk = e3; }
                    break;
                }
            }
        }
    }
    // entries at or above the bound: a prefix of the sorted list
    uint32_t c = 0;
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
        const uint32_t e = e0 + lane;
        bool keep = false;
        if (e < n) {
            const size_t src = (size_t)q * loc.k_stride + e;
            keep = bk < 0 || !ent_greater(b0, b1, b2, bk, loc.scores[src * 3 + 0], loc.scores[src * 3 + 1], loc.scores[src * 3 + 2], (int64_t)loc.keys[src]);
        }
        c += (uint32_t)__popcll(__ballot(keep ? 1 : 0));
    }
    uint32_t first = 0;
    if (lane == 0 && c) first = atomicAdd(cursor + j, c);
    first = __shfl(first, 0);
    uint64_t* ent = slice + (size_t)per * 2 + (size_t)first * words;
    for (uint32_t e = lane; e < c; e += 64) {
        const size_t src = (size_t)q * loc.k_stride + e;
        uint64_t* d = ent + (size_t)e * words;
        d[0] = loc.keys[src];
        d[1] = (uint64_t)loc.scores[src * 3 + 0]; d[2] = (uint64_t)loc.scores[src * 3 + 1]; d[3] = (uint64_t)loc.scores[src * 3 + 2];
        if (words > 4) d[4] = loc.text_match ? (uint64_t)loc.text_match[src] : 0;
    }
    if (lane == 0) {
        slice[(size_t)i * 2] = (uint64_t)c | ((uint64_t)(status ? (uint32_t)status[q] & 0xFFFFu : 0u) << 16) | ((uint64_t)first << 32);
        slice[(size_t)i * 2 + 1] = (loc.num_matched && !failed) ? loc.num_matched[q] : 0;
    }
}
// replicas form of a group (every member mirrors the whole collection, the batch is cut into query slices): the member's own result for
// its slice (stride loc.k_stride) -> rows [q_out_offset, ..) of the staged full-batch arrays (stride out.k_stride), truncated to k
// shard form of the candidate fold: (a) before the exchange every hit's key carries its pass in the low 4 bits (key' = key << 4 | pass: seq_ids are below 2^32 and a
// document lives in ONE shard, so the merge's last tie-break — the key — orders the tagged keys exactly as it orders the keys) and the shard's (pass mask, union
// count) pair is laid out for the all-gather; (b) after the merge the tags come off: key = key' >> 4, query_index = the passes before the hit's that matched on
// ANY shard (searched_queries.size() at the time of the pass, src/index.cpp:5511, 5580-5585), found = the shards' union counts added up (disjoint documents).
__global__ void kw_group_cand_tag_kernel(uint64_t* keys, const uint32_t* pass_of_hit, const uint32_t* n_hits, const int32_t* status, uint32_t k_stride, uint32_t n_groups,
                                         const uint32_t* pass_mask, const unsigned long long* found, unsigned long long* meta /*[n_groups][2]*/) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = (uint32_t)(i / k_stride), j = (uint32_t)(i % k_stride);
    if (g >= n_groups) return;
    const bool ok = status[g] == 0;
    if (ok && j < n_hits[g]) keys[i] = (keys[i] << 4) | (uint64_t)(pass_of_hit[i] & 15u);
    if (j == 0) { meta[2 * (size_t)g] = ok ? pass_mask[g] : 0u; meta[2 * (size_t)g + 1] = (ok && found) ? found[g] : 0ull; }
}
__global__ void kw_group_cand_fix_kernel(uint64_t* keys, uint32_t* query_index, const uint32_t* n_hits, uint32_t k_stride, uint32_t q0, uint32_t q1,
                                         const unsigned long long* meta_all /*[n_shards][n_groups][2]*/, uint32_t n_shards, uint32_t n_groups, unsigned long long* found) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = q0 + (uint32_t)(i / k_stride), j = (uint32_t)(i % k_stride);
    if (g >= q1) return;
    uint32_t mask = 0;
    unsigned long long f = 0;
    for (uint32_t s = 0; s < n_shards; s++) { mask |= (uint32_t)meta_all[((size_t)s * n_groups + g) * 2]; f += meta_all[((size_t)s * n_groups + g) * 2 + 1]; }
    if (j == 0 && found) found[g] = f;
    if (j >= n_hits[g]) return;
    const size_t at = (size_t)g * k_stride + j;
    const uint64_t kt = keys[at];
    const uint32_t pass = (uint32_t)(kt & 15u);
    keys[at] = kt >> 4;
    if (query_index) query_index[at] = (uint32_t)__popc(mask & ((1u << pass) - 1u));
}
__global__ void kw_group_store_slice_kernel(KwOut loc, const int32_t* status, uint32_t n_queries, uint32_t q_out_offset, uint32_t k, KwOut out, int32_t* status_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = i / k, j = i - q * k;
    if (q >= n_queries) return;
    const bool failed = status && status[q] != 0;
    const uint32_t n = failed ? 0u : (loc.n_hits[q] < k ? loc.n_hits[q] : k);
    const size_t src = (size_t)q * loc.k_stride + j, dst = (size_t)(q + q_out_offset) * out.k_stride + j;
    if (j < n) {
        out.keys[dst] = loc.keys[src];
        out.scores[dst * 3 + 0] = loc.scores[src * 3 + 0]; out.scores[dst * 3 + 1] = loc.scores[src * 3 + 1]; out.scores[dst * 3 + 2] = loc.scores[src * 3 + 2];
        if (out.text_match) out.text_match[dst] = loc.text_match ? loc.text_match[src] : 0;
    }
    if (j == 0) {
        out.n_hits[q + q_out_offset] = n;
        if (out.num_matched) out.num_matched[q + q_out_offset] = (loc.num_matched && !failed) ? loc.num_matched[q] : 0;
        if (status_out) status_out[q + q_out_offset] = status ? status[q] : 0;
    }
}
template <int CAP>
__global__ __launch_bounds__(KW_THREADS) void kw_shard_merge_kernel(KwShardIn in, KwOut out, uint32_t k) {
    __shared__ TopkLds<CAP> tk;
    __shared__ uint32_t s_total;
    const uint32_t t = threadIdx.x, qi = blockIdx.x, q = in.packed ? blockIdx.x + in.q_out_offset : blockIdx.x;
    const size_t qw = (size_t)in.k_in * in.words + 3;
    if (t == 0) s_total = 0;
    for (int i = t; i < CAP; i += KW_THREADS) tk.key[i] = -1;
    __syncthreads();
    // the entries of shard g for this query, and their number (packed forms)
    auto shard_entries = [&](uint32_t g, uint32_t& n) -> const uint64_t* {
        const uint64_t* blk = in.packed + g * in.shard_stride;
        if (in.pruned_per) {
            const uint64_t h = blk[(size_t)qi * 2];
            n = (uint32_t)(h & 0xFFFFu);
            return blk + (size_t)in.pruned_per * 2 + (size_t)(h >> 32) * in.words;
        }
        n = (uint32_t)blk[(size_t)qi * qw + (size_t)in.k_in * in.words];
        return blk + (size_t)qi * qw;
    };
    for (uint32_t g = 0; g < in.n_shards; g++) {
        uint32_t n = 0;
        const uint64_t* pk = in.packed ? shard_entries(g, n) : nullptr;
        if (!pk) n = in.n_hits[(size_t)g * in.n_queries + q];
        const size_t base = ((size_t)g * in.n_queries + q) * in.k_in;
        const uint32_t at = s_total;
        for (uint32_t i = t; i < n; i += KW_THREADS) {
            const uint32_t slot = at + i;
            if (slot < (uint32_t)CAP) {
                if (pk) {
                    const uint64_t* e = pk + (size_t)i * in.words;
                    tk.s0[slot] = (int64_t)e[1]; tk.s1[slot] = (int64_t)e[2]; tk.s2[slot] = (int64_t)e[3];
                    tk.key[slot] = (int64_t)((e[0] << 16) | (uint64_t)(g * in.k_in + i));
                } else {
                    tk.s0[slot] = in.scores[(base + i) * 3 + 0]; tk.s1[slot] = in.scores[(base + i) * 3 + 1]; tk.s2[slot] = in.scores[(base + i) * 3 + 2];
                    tk.key[slot] = (int64_t)((in.keys[base + i] << 16) | (uint64_t)(g * in.k_in + i));
                }
            }
        }
        __syncthreads();
        if (t == 0) s_total = at + n;
        __syncthreads();
    }
    const uint32_t total = s_total < (uint32_t)CAP ? s_total : (uint32_t)CAP;
    {   // sort only as many slots as hold entries (the rest is padding, key < 0): a bound-pruned query brings ~1.5 k entries, not G x k
        int n_sort = 64;
        while (n_sort < (int)total) n_sort <<= 1;
        topk_sort<CAP, true>(tk, n_sort < CAP ? n_sort : CAP);
    }
    const uint32_t kq = in.cap_per_query && in.cap_per_query[q] < k ? in.cap_per_query[q] : k;
    const uint32_t n_out = total < kq ? total : kq;
    const size_t ob = (size_t)q * out.k_stride;
    for (uint32_t i = t; i < n_out; i += KW_THREADS) {
        const uint64_t packed = (uint64_t)tk.key[i];
        const uint32_t origin = (uint32_t)(packed & 0xFFFFu);
        const size_t src = ((size_t)(origin / in.k_in) * in.n_queries + q) * in.k_in + origin % in.k_in;
        out.keys[ob + i] = packed >> 16;
        out.scores[(ob + i) * 3 + 0] = tk.s0[i]; out.scores[(ob + i) * 3 + 1] = tk.s1[i]; out.scores[(ob + i) * 3 + 2] = tk.s2[i];
        if (in.packed) {
            if (out.text_match) { uint32_t n_g; out.text_match[ob + i] = in.words > 4 ? (int64_t)shard_entries(origin / in.k_in, n_g)[(size_t)(origin % in.k_in) * in.words + 4] : 0; }
            if (out.vector_distance) out.vector_distance[ob + i] = -1.0f;
            continue;
        }
        if (out.text_match) out.text_match[ob + i] = in.text_match ? in.text_match[src] : 0;
        if (out.vector_distance) out.vector_distance[ob + i] = in.vector_distance ? in.vector_distance[src] : -1.0f;
        if (out.match_score_index) out.match_score_index[ob + i] = in.match_score_index ? in.match_score_index[src] : (int8_t)0;
    }
    if (t == 0) {
        out.n_hits[q] = n_out;
        if (in.packed) {
            unsigned long long nm = 0;
            int32_t st = 0;
            for (uint32_t g = 0; g < in.n_shards; g++) {
                if (in.pruned_per) {
                    const uint64_t* h = in.packed + g * in.shard_stride + (size_t)qi * 2;
                    nm += h[1];
                    if (st == 0) st = (int32_t)(uint32_t)((h[0] >> 16) & 0xFFFFu);
                    continue;
                }
                const uint64_t* c = in.packed + g * in.shard_stride + (size_t)qi * qw + (size_t)in.k_in * in.words;
                nm += c[1];
                if (st == 0) st = (int32_t)(uint32_t)c[2];
            }
            if (out.num_matched) out.num_matched[q] = st == 0 ? nm : 0;
            if (in.status_out) in.status_out[q] = st;
            if (st != 0) out.n_hits[q] = 0;
        } else if (out.num_matched) {
            unsigned long long nm = 0;
            if (in.num_matched) for (uint32_t g = 0; g < in.n_shards; g++) nm += in.num_matched[(size_t)g * in.n_queries + q];
            out.num_matched[q] = nm;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Candidate-token combinations (Index::search_all_candidates, src/index.cpp:1794-1894): the combinations of one
// user query ran as consecutive entries [group_begin[g], group_begin[g+1]) of one keyword batch. The reference feeds them, in
// order, to ONE Topster: a key met again replaces its KV unless the new KV is_smaller (include/topster.h:392-406), and the heap
// threshold only rises, so the final content is: per key the greatest (s0,s1,s2) — the LATEST pass among equals — then the top k
// of those in KV::is_greater order. One workgroup per group:
//   sort A: (key << 16 | pass * k_in + slot) descending with the score columns zeroed -> equal keys adjacent, later pass first;
//           the head of each run reads the run's scores from the batch output and elects the winner;
//   sort B: the winners by (s0, s1, s2, key) = the Topster's sort() order.
// query_index[hit] = number of earlier passes of the group that matched anything (searched_queries.size() at the pass, :5511,
// :5580-5585); num_matched = the last pass's (num_keyword_matches is assigned, not accumulated, :5553).
struct KwCandIn {
    const uint64_t* keys; const int64_t* scores; const int64_t* text_match; const float* vector_distance; const int8_t* match_score_index;
    const uint32_t* n_hits; const uint64_t* num_matched;
    const uint32_t* group_range;        // [n_groups][3] = first entry, one past the last entry (empty range: the group did not run), Topster capacity
    uint32_t k_in;
    // the shard form (tsgpu_group_keyword_search_candidates_batch): query_index[hit] = the PASS that produced the hit instead of the number of earlier passes that
    // matched — "matched anything" is a property of the whole collection, so the shards exchange pass_mask (bit p = pass p matched on THIS shard) and the count is
    // taken from the OR of the masks after the merge
    uint32_t raw_pass;
    uint32_t* pass_mask;                // nullable: [n_groups]
};
template <int CAP>
__global__ __launch_bounds__(KW_THREADS) void kw_candidates_merge_kernel(KwCandIn in, KwOut out, uint32_t* query_index) {
    __shared__ TopkLds<CAP> tk;
    __shared__ uint32_t s_total, s_win;
    __shared__ uint32_t s_qidx[KW_MAX_CANDIDATE_PASSES];
    constexpr int PER = CAP / KW_THREADS;
    const uint32_t t = threadIdx.x, g = blockIdx.x;
    const uint32_t e0 = in.group_range[3 * g], e1 = in.group_range[3 * g + 1], k = in.group_range[3 * g + 2];
    if (t == 0) {
        s_total = 0; s_win = 0;
        uint32_t searched = 0, mask = 0;
        for (uint32_t e = e0; e < e1; e++) { s_qidx[e - e0] = in.raw_pass ? e - e0 : searched; if (in.n_hits[e] > 0) { searched++; mask |= 1u << (e - e0); } }
        if (in.pass_mask) in.pass_mask[g] = mask;
    }
    for (int i = t; i < CAP; i += KW_THREADS) { tk.key[i] = -1; tk.s0[i] = 0; tk.s1[i] = 0; tk.s2[i] = 0; }
    __syncthreads();
    for (uint32_t e = e0; e < e1; e++) {
        const uint32_t n = in.n_hits[e];
        const uint32_t at = s_total;
        for (uint32_t i = t; i < n; i += KW_THREADS) {
            const uint32_t slot = at + i;
            if (slot < (uint32_t)CAP) tk.key[slot] = (int64_t)((in.keys[(size_t)e * in.k_in + i] << 16) | (uint64_t)((e - e0) * in.k_in + i));
        }
        __syncthreads();
        if (t == 0) s_total = at + n;
        __syncthreads();
    }
    topk_sort<CAP, true>(tk);                                   // sort A
    const uint32_t total = s_total < (uint32_t)CAP ? s_total : (uint32_t)CAP;
    int64_t win[PER];
    #pragma unroll
    for (int r = 0; r < PER; r++) {
        const uint32_t i = r * KW_THREADS + t;
        win[r] = -1;
        if (i >= total) continue;
        const uint64_t mine = (uint64_t)tk.key[i];
        if (i > 0 && ((uint64_t)tk.key[i - 1] >> 16) == (mine >> 16)) continue;          // not the head of its run
        uint64_t best = mine;
        uint32_t o = (uint32_t)(mine & 0xFFFFu);
        size_t src = (size_t)(e0 + o / in.k_in) * in.k_in + o % in.k_in;
        int64_t b0 = in.scores[src * 3], b1 = in.scores[src * 3 + 1], b2 = in.scores[src * 3 + 2];
        for (uint32_t j = i + 1; j < total; j++) {             // earlier passes of the same key: win only when strictly greater
            const uint64_t other = (uint64_t)tk.key[j];
            if ((other >> 16) != (mine >> 16)) break;
            o = (uint32_t)(other & 0xFFFFu);
            src = (size_t)(e0 + o / in.k_in) * in.k_in + o % in.k_in;
            const int64_t c0 = in.scores[src * 3], c1 = in.scores[src * 3 + 1], c2 = in.scores[src * 3 + 2];
            if (c0 > b0 || (c0 == b0 && (c1 > b1 || (c1 == b1 && c2 > b2)))) { best = other; b0 = c0; b1 = c1; b2 = c2; }
        }
        win[r] = (int64_t)best;
    }
    __syncthreads();
    for (int i = t; i < CAP; i += KW_THREADS) tk.key[i] = -1;
    __syncthreads();
    #pragma unroll
    for (int r = 0; r < PER; r++) {
        if (win[r] < 0) continue;
        const uint32_t o = (uint32_t)((uint64_t)win[r] & 0xFFFFu);
        const size_t src = (size_t)(e0 + o / in.k_in) * in.k_in + o % in.k_in;
        const uint32_t slot = atomicAdd(&s_win, 1u);
        tk.s0[slot] = in.scores[src * 3]; tk.s1[slot] = in.scores[src * 3 + 1]; tk.s2[slot] = in.scores[src * 3 + 2];
        tk.key[slot] = win[r];
    }
    __syncthreads();
    topk_sort<CAP, true>(tk);                                   // sort B
    const uint32_t n_out = s_win < k ? s_win : k;
    const size_t ob = (size_t)g * out.k_stride;
    for (uint32_t i = t; i < n_out; i += KW_THREADS) {
        const uint64_t packed = (uint64_t)tk.key[i];
        const uint32_t o = (uint32_t)(packed & 0xFFFFu);
        const size_t src = (size_t)(e0 + o / in.k_in) * in.k_in + o % in.k_in;
        out.keys[ob + i] = packed >> 16;
        out.scores[(ob + i) * 3 + 0] = tk.s0[i]; out.scores[(ob + i) * 3 + 1] = tk.s1[i]; out.scores[(ob + i) * 3 + 2] = tk.s2[i];
        if (out.text_match) out.text_match[ob + i] = in.text_match ? in.text_match[src] : 0;
        if (out.vector_distance) out.vector_distance[ob + i] = in.vector_distance ? in.vector_distance[src] : -1.0f;
        if (out.match_score_index) out.match_score_index[ob + i] = in.match_score_index ? in.match_score_index[src] : (int8_t)0;
        if (query_index) query_index[ob + i] = s_qidx[o / in.k_in];
    }
    if (t == 0) {
        out.n_hits[g] = n_out;
        if (out.num_matched) out.num_matched[g] = (in.num_matched && e1 > e0) ? in.num_matched[e1 - 1] : 0ull;
    }
}

// The same fold WITHOUT sorting (round 5; VERDICT r4 #7: the two bitonic sorts of 4 096 slots above cost 1.74 ms per 1 000 user queries x 10
// passes at one workgroup per CU). Every pass's list arrives SORTED in KV::is_greater order, so a hit's place among any set of the passes' hits
// is a sum of binary searches, and only the duplicate keys need a table:
//   1. the passes' hits side by side in LDS (pass after pass: a hit's index also orders equal scores by pass);
//   2. per key the winner — greatest (s0, s1, s2), the LATEST pass among equals (include/topster.h:392-406) — through an LDS hash table of hit
//      indices (one CAS loop per hit: the incumbent is replaced only by a better hit of the same key);
//   3. an exclusive prefix sum of the winner flags over the concatenated lists;
//   4. a winner's rank in the shared Topster's sort() order = over the passes, the winners among the hits of that pass that are greater than it
//      (one binary search per pass + two prefix reads); rank < capacity -> it is output slot `rank`.
// ~100 LDS reads per hit instead of ~15 000 per thread. Same output as kw_candidates_merge_kernel (tests run both: option kw_candidates_rank_fold).
template <int CAP, bool S2>
__global__ __launch_bounds__(KW_THREADS) void kw_candidates_rank_kernel(KwCandIn in, KwOut out, uint32_t* query_index) {
    __shared__ TopkLds<CAP, S2> tk;
    __shared__ uint32_t hs[2 * CAP];                     // hit index + 1 of the key's current winner; 0 = empty
    __shared__ uint16_t wpre[CAP + 2];                   // winner flags, then their exclusive prefix sums (wpre[N] = winners)
    __shared__ uint32_t s_base[KW_MAX_CANDIDATE_PASSES + 1], s_qidx[KW_MAX_CANDIDATE_PASSES], s_wave[KW_THREADS / 64];
    constexpr int PER = CAP / KW_THREADS;
    constexpr uint32_t HMASK = 2u * CAP - 1u;
    const uint32_t t = threadIdx.x, g = blockIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t e0 = in.group_range[3 * g], e1 = in.group_range[3 * g + 1], k = in.group_range[3 * g + 2];
    const uint32_t P = e1 - e0;
    if (t == 0) {
        uint32_t searched = 0, at = 0, mask = 0;
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t n = in.n_hits[e0 + p] < in.k_in ? in.n_hits[e0 + p] : in.k_in;
            s_base[p] = at; at += n; if (at > (uint32_t)CAP) at = CAP;           // (the host sizes CAP >= passes x k_stride)
            s_qidx[p] = in.raw_pass ? p : searched; if (n > 0) { searched++; mask |= 1u << p; }
        }
        s_base[P] = at;
        if (in.pass_mask) in.pass_mask[g] = mask;
    }
    for (int i = t; i < 2 * CAP; i += KW_THREADS) hs[i] = 0;
    __syncthreads();
    const uint32_t N = s_base[P];
    auto pass_of = [&](uint32_t gi) { uint32_t p = 0; while (p + 1 < P && s_base[p + 1] <= gi) p++; return p; };
    for (uint32_t gi = t; gi < N; gi += KW_THREADS) {
        const uint32_t p = pass_of(gi);
        const size_t src = (size_t)(e0 + p) * in.k_in + (gi - s_base[p]);
        tk.s0[gi] = in.scores[src * 3]; tk.s1[gi] = in.scores[src * 3 + 1];
        if (S2) tk.s2[tk.i2(gi)] = in.scores[src * 3 + 2];
        tk.key[gi] = (int64_t)in.keys[src];
    }
    if (!S2 && t == 0) tk.s2[0] = 0;
    __syncthreads();
    auto better = [&](uint32_t a, uint32_t b) {          // hit a beats hit b OF THE SAME KEY: greater scores, or equal scores from a later pass
        const int64_t a0 = tk.s0[a], b0 = tk.s0[b], a1 = tk.s1[a], b1 = tk.s1[b], a2 = tk.s2[tk.i2(a)], b2 = tk.s2[tk.i2(b)];
        if (a0 != b0) return a0 > b0;
        if (a1 != b1) return a1 > b1;
        if (a2 != b2) return a2 > b2;
        return a > b;
    };
    auto slot0 = [&](uint64_t key) { return (uint32_t)(((uint32_t)key ^ (uint32_t)(key >> 32)) * 2654435761u) & HMASK; };
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const uint32_t gi = r * KW_THREADS + t;
        if (gi >= N) continue;
        const int64_t key = tk.key[gi];
        uint32_t h = slot0((uint64_t)key);
        for (;;) {
            uint32_t sl = atomicCAS(&hs[h], 0u, gi + 1);
            if (sl == 0) break;                           // the first hit of this key
            const uint32_t o = sl - 1;
            if (tk.key[o] == key) {
                if (!better(gi, o)) break;                // the incumbent stays
                if (atomicCAS(&hs[h], sl, gi + 1) == sl) break;
                continue;                                 // somebody replaced it meanwhile: look at the same slot again
            }
            h = (h + 1) & HMASK;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const uint32_t gi = r * KW_THREADS + t;
        if (gi >= N) continue;
        const int64_t key = tk.key[gi];
        uint32_t h = slot0((uint64_t)key);
        uint32_t win = 0;
        for (;;) {
            const uint32_t sl = hs[h];
            if (sl == gi + 1) { win = 1; break; }
            if (tk.key[sl - 1] == key) break;             // (the key was inserted: an empty slot cannot come first)
            h = (h + 1) & HMASK;
        }
        wpre[gi] = (uint16_t)win;
    }
    __syncthreads();
    {   // exclusive prefix sums of the flags: thread t owns the PER consecutive hits [t * PER, (t + 1) * PER)
        uint32_t f[PER], sum = 0;
#pragma unroll
        for (int r = 0; r < PER; r++) { const uint32_t gi = t * PER + r; f[r] = gi < N ? wpre[gi] : 0u; sum += f[r]; }
        uint32_t incl = sum;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, (unsigned)d); if (lane >= (uint32_t)d) incl += v; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = incl - sum;
        for (uint32_t w = 0; w < wave; w++) before += s_wave[w];
#pragma unroll
        for (int r = 0; r < PER; r++) { const uint32_t gi = t * PER + r; if (gi <= N) wpre[gi] = (uint16_t)before; before += f[r]; }
        if ((t + 1) * (uint32_t)PER == N) wpre[N] = (uint16_t)before;       // (wpre[N] = the total; N == CAP lies beyond the last thread's range)
    }
    __syncthreads();
    const uint32_t U = wpre[N];
    const uint32_t n_out = U < k ? U : k;
    const size_t ob = (size_t)g * out.k_stride;
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const uint32_t gi = r * KW_THREADS + t;
        if (gi >= N || wpre[gi + 1] == wpre[gi]) continue;             // not a winner
        const uint32_t p_own = pass_of(gi);
        const int64_t w0 = tk.s0[gi], w1 = tk.s1[gi], w2 = tk.s2[tk.i2(gi)], wk = tk.key[gi];
        uint32_t rank = 0;
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t b = s_base[p], e = s_base[p + 1];
            uint32_t lo = b, hi = e;                                        // first hit of pass p that is NOT greater than this one
            if (p == p_own) lo = gi;
            else while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ent_greater(tk.s0[mid], tk.s1[mid], tk.s2[tk.i2(mid)], tk.key[mid], w0, w1, w2, wk)) lo = mid + 1; else hi = mid;
            }
            rank += (uint32_t)wpre[lo] - (uint32_t)wpre[b];
        }
        if (rank >= n_out) continue;
        const size_t src = (size_t)(e0 + p_own) * in.k_in + (gi - s_base[p_own]);
        out.keys[ob + rank] = (uint64_t)wk;
        out.scores[(ob + rank) * 3 + 0] = w0; out.scores[(ob + rank) * 3 + 1] = w1; out.scores[(ob + rank) * 3 + 2] = w2;
        if (out.text_match) out.text_match[ob + rank] = in.text_match ? in.text_match[src] : 0;
        if (out.vector_distance) out.vector_distance[ob + rank] = in.vector_distance ? in.vector_distance[src] : -1.0f;
        if (out.match_score_index) out.match_score_index[ob + rank] = in.match_score_index ? in.match_score_index[src] : (int8_t)0;
        if (query_index) query_index[ob + rank] = s_qidx[p_own];
    }
    if (t == 0) {
        out.n_hits[g] = n_out;
        if (out.num_matched) out.num_matched[g] = (in.num_matched && e1 > e0) ? in.num_matched[e1 - 1] : 0ull;
    }
}

// all_result_ids of a group = sorted-unique union of the passes' emitted ids (id_buff -> timsort + unique + or_scalar,
// src/index.cpp:5565-5578, 5081-5090): one bit per seq_id, set from the passes' id segments, then counted / expanded in order.
// Marked from the batch's own tables: one workgroup row per WORK ITEM — its segment of the id arena is queries[item.query].ids_out_off +
// item.ids_out_off, n_emit[item] ids long —, the group of the item's pass from group_of[] (KW_NONE: the group reports a failing pass -> no
// ids). A bit that this thread's atomicOr turned on is a NEW member of the union, so the marks count the union themselves (found[group]):
// no pass over the bitmaps (round 4: 0.39 ms per 1 000 groups at 10M documents), no host-built segment list, no n_emit read-back.
__global__ __launch_bounds__(KW_THREADS) void kw_idset_mark_items_kernel(const uint32_t* __restrict__ ids, const KwQueryDev* __restrict__ queries,
                                                                        const KwWorkItem* __restrict__ work, const uint32_t* __restrict__ n_emit,
                                                                        const uint32_t* __restrict__ group_of, uint32_t* __restrict__ bits,
                                                                        uint64_t words_per_group, unsigned long long* __restrict__ found) {
    const uint32_t cnt = n_emit[blockIdx.x];
    if (blockIdx.y * KW_THREADS >= cnt) return;                       // (uniform)
    const KwWorkItem wi = work[blockIdx.x];
    const uint32_t qi = wi.query & 0x0FFFFFFFu, g = group_of[qi];
    if (g == KW_NONE) return;
    const uint32_t* src = ids + queries[qi].ids_out_off + wi.ids_out_off;
    uint32_t* mine = bits + (uint64_t)g * words_per_group;
    uint32_t c = 0;
    for (uint32_t i = blockIdx.y * KW_THREADS + threadIdx.x; i < cnt; i += gridDim.y * KW_THREADS) {
        const uint32_t id = src[i], bit = 1u << (id & 31);
        c += (atomicOr(&mine[id >> 5], bit) & bit) ? 0u : 1u;
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&found[g], (unsigned long long)c);
}
// per-call id lists (tsgpu_keyword_search_batch_ids): the work items' id segments, scattered over the lane's id arena, copied into
// one dense array (query after query, segment after segment) so that ONE download hands every caller its ids
struct KwIdCopy { uint64_t src, dst; uint32_t cnt, pad; };
__global__ __launch_bounds__(KW_THREADS) void kw_ids_gather_kernel(const uint32_t* __restrict__ ids, const KwIdCopy* __restrict__ segs, uint32_t* __restrict__ out) {
    const KwIdCopy sg = segs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < sg.cnt; i += KW_THREADS) out[sg.dst + i] = ids[sg.src + i];
}
// ascending ids of one group's bitmap -> out[0 .. found) (one workgroup walks the words, 256 at a time, with a running base)
// (the walk itself: words [w_begin, w_end) of the bitmap, the first id written to out[start]; every thread of a KW_THREADS workgroup calls it. The infix
// front expands one bitmap with many workgroups, each on its own range behind the counts of the earlier ones: kw_infix.hip.h)
__device__ inline void idset_expand_range(const uint32_t* __restrict__ bits, uint64_t w_begin, uint64_t w_end, uint32_t* __restrict__ out, uint64_t start, uint64_t cap) {
    __shared__ uint32_t s_wave[KW_THREADS / 64];
    __shared__ uint64_t s_base;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n_words = w_end;
    if (t == 0) s_base = start;
    __syncthreads();
    for (uint64_t w0 = w_begin; w0 < n_words; w0 += KW_THREADS) {
        const uint64_t w = w0 + t;
        uint32_t word = w < n_words ? bits[w] : 0u;
        const uint32_t c = (uint32_t)__popc(word);
        uint32_t incl = c;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += up; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t x = 0; x < KW_THREADS / 64; x++) { if (x < wave) before += s_wave[x]; all += s_wave[x]; }
        uint64_t at = s_base + before + (incl - c);
        while (word) {
            const int b = __ffs((int)word) - 1;
            word &= word - 1;
            if (at < cap) out[at] = (uint32_t)(w * 32 + b);
            at++;
        }
        __syncthreads();
        if (t == 0) s_base += all;
        __syncthreads();
    }
}
__global__ __launch_bounds__(KW_THREADS) void kw_idset_expand_kernel(const uint32_t* __restrict__ bits, uint64_t n_words, uint32_t* __restrict__ out, uint64_t cap) {
    idset_expand_range(bits, 0, n_words, out, 0, cap);
}

// num_keyword_matches of a query with filter ids AND excluded ids AND several query_by fields: the first-order recurrence of
// kw_score_stage (c_j = rank_j > rank_{j-1} | c_{j-1} & excluded_{j-1}) needs the intersection in ascending id order, but the work
// items of a multi-field query are one ascending stream PER FIELD of the driver token. One thread per such query (rare: curated hits
// + filter_by + several fields) merges the <= 4 streams of hit records the find kernel left (every intersection id, before filter and
// exclusion) and walks the filter / excluded arrays with cursors: O(ids + filter + excluded). Runs between the find and the score
// kernel (the score kernel overwrites part.cnt); the result waits in part.n_match1[first work item] for kw_merge_kernel.
template <int TMAX>
__global__ __launch_bounds__(64) void kw_mf_ordered_count_kernel(const KwQueryDev* __restrict__ queries, const KwWorkItem* __restrict__ work, KwPartials part,
                                                                 const uint32_t* __restrict__ hits_all, const uint64_t* __restrict__ hit_off, uint32_t table_first,
                                                                 const uint32_t* __restrict__ aux_ids, const uint32_t* __restrict__ jobs) {
    if (threadIdx.x != 0) return;
    constexpr uint32_t NP1 = TMAX * KW_MAX_FIELDS + 1;
    const KwQueryDev q = queries[jobs[blockIdx.x]];
    const uint32_t* __restrict__ excl = aux_ids + q.aux_off;
    const uint32_t* __restrict__ filt = excl + q.n_excl;
    struct Stream { uint32_t item, item_end, rec, n_rec; const uint32_t* base; uint32_t id; bool valid; };
    Stream st[KW_MAX_FIELDS];
    int ns = 0;
    for (uint32_t w = q.first_work, end = q.first_work + q.n_work; w < end;) {
        const uint32_t f = work[w].query >> 28, beg = w;
        while (w < end && (work[w].query >> 28) == f) w++;
        if (ns < KW_MAX_FIELDS) { st[ns].item = beg; st[ns].item_end = w; st[ns].rec = 0; st[ns].n_rec = 0; st[ns].base = nullptr; st[ns].id = 0; st[ns].valid = false; ns++; }
    }
    auto position = [&](Stream& s) {               // on the next record of the stream, skipping work items without hits
        s.valid = false;
        while (s.item < s.item_end) {
            if (s.base == nullptr) { s.n_rec = part.cnt[s.item]; s.base = hits_all + hit_off[s.item - table_first] * (uint64_t)NP1; s.rec = 0; }
            if (s.rec < s.n_rec) { s.id = s.base[(size_t)s.rec * NP1]; s.valid = true; return; }
            s.item++; s.base = nullptr;
        }
    };
    for (int i = 0; i < ns; i++) position(st[i]);
    uint32_t fc = 0, ec = 0, rp = 0, c = 0, ep = 0;
    unsigned long long total = 0;
    for (;;) {
        int best = -1;
        for (int i = 0; i < ns; i++) if (st[i].valid && (best < 0 || st[i].id < st[best].id)) best = i;
        if (best < 0) break;
        const uint32_t x = st[best].id;
        st[best].rec++;
        position(st[best]);
        while (fc < q.n_filt && filt[fc] <= x) fc++;                  // rank = # filter ids <= x
        while (ec < q.n_excl && excl[ec] < x) ec++;
        const uint32_t e = (ec < q.n_excl && excl[ec] == x) ? 1u : 0u;
        c = (fc > rp ? 1u : 0u) | (c & ep);
        total += c;
        rp = fc; ep = e;
    }
    part.n_match1[q.first_work] = (uint32_t)total;
}

// Index::compute_aux_scores' text half (src/index.cpp:8800-8846, rerank_hybrid_matches): the aggregated text-match score of GIVEN
// documents — hybrid hits that only the vector search found — for a query's tokens: every token's lists are positioned on the document
// (skip_to), the tokens it holds are scored per field, query_len = tokens found anywhere; a document with none of them scores 0.
// One thread per (query, document); queries are described like multi-field queries (KwQueryDev with total_cost 0 + KwQueryMF).
struct KwAuxItem { uint32_t query, seq_id; };
__global__ __launch_bounds__(64) void kw_aux_score_kernel(IndexView ix, const KwQueryDev* __restrict__ queries, const KwQueryMF* __restrict__ mfs,
                                                          const KwAuxItem* __restrict__ items, uint32_t n_items, int64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const KwAuxItem it = items[i];
    const KwQueryDev& q = queries[it.query];
    const KwQueryMF& mf = mfs[q.mf_index];
    uint32_t pos[KW_MAX_TOKENS * KW_MAX_FIELDS];
    uint32_t tokens_found = 0;
    for (int t = 0; t < KW_MAX_TOKENS; t++) {
        bool any = false;
        for (int f = 0; f < KW_MAX_FIELDS; f++) {
            uint32_t p = KW_NONE;
            if ((uint32_t)t < q.n_lists && (uint32_t)f < mf.n_fields && mf.list[t][f] != KW_NONE) {
                uint32_t pp;
                if (probe_list(ix, ix.lists[mf.list[t][f]], it.seq_id, pp)) { p = pp; any = true; }
            }
            pos[t * KW_MAX_FIELDS + f] = p;               // (runtime index: the array lives in scratch — a rare, short kernel)
        }
        tokens_found += any ? 1u : 0u;
    }
    uint32_t off_words = 0;
    out[i] = (int64_t)agg_score_mf<KW_MAX_TOKENS>(ix, q, mf, pos, tokens_found, off_words);
}

#include "kw_find2.hip.h"
#include "kw_find_mf2.hip.h"

#include "kw_groupby.hip.h"

}  // namespace tsgpu
