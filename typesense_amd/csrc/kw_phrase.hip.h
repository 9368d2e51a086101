// kw_phrase.hip.h — the front of phrase search (Index::do_phrase_search, src/index.cpp:5909-6086; handle_exclusion, :6274-6324;
// posting_list_t::get_phrase_matches, src/posting_list.cpp:1791-1825) for gfx950. Included by tsgpu.hip behind kw_infix.hip.h (it uses TokRun / load_run /
// load_runs_staged / arr_next_elem / run_pos of kw_kernels.hip.h and the bitmap kernels of kw_infix.hip.h).
//
// The reference intersects a phrase's posting lists and walks every intersected id through get_offsets (a std::map of vectors per document) and
// has_phrase_match / found_token_sequence (linear rescans). Here:
//   the intersection         is the keyword path's: every multi-token (query, field, phrase) is planned as an AND item and runs through the find kernels
//                            (kw_find2_kernel / kw_search_kernel<DEFER> / the multi-field find kernels for a string[] field), which leave {seq_id, pos[T]} records
//   kw_phrase_mark_kernel    one thread per hit record: the T runs, the elements (arr_next_elem = get_offsets), the non-descending prefixes, the adjacency test;
//                            a match sets the id's bit in the bitmap of its (query, field, phrase)
//   infix_union_mark_kernel  a one-token phrase marks its list directly (get_phrase_matches passes every id, :1796-1800)
//   phrase_fold_kernel       the fold of a field's phrases (:5963-5981, the restart after an empty intersection included), decided on the device from the counts
//   phrase_or_fields_kernel  the OR of the fields' bitmaps (:5997-6009); then the infix front's clear / AND / count / expand kernels (:6012-6026)
//   phrase_tm_kernel         the per-id text score of the surviving list: max over the fields whose first `cut` folded ids hold it of 100000 + weight (:5988-5995)
// The list is ranked by kw_wildcard_kernel (KwQueryDev::wild_ids / wild_tm).
#pragma once

namespace tsgpu {

static const uint32_t PHRASE_THREADS = 256;
static const uint32_t PHRASE_MODE_RANK = 0, PHRASE_MODE_IDS = 1, PHRASE_MODE_EXCLUDE = 2;       // (= TSGPU_PHRASE_RANK / _IDS / _EXCLUDE)
static const uint32_t PHRASE_WEIGHT_BASE = 100000;          // weight_score_base, :5990
static_assert(PHRASE_THREADS == KW_THREADS && PHRASE_THREADS == INFIX_THREADS, "the mark kernel runs on the find kernels' work items, the fold beside the infix kernels");

// what the mark kernel needs beside the find kernels' tables. unit = one (query, field, phrase) of the round: its bitmap is bits + unit * words.
struct PhraseMarkArgs {
    const uint32_t* unit_of_item;        // [AND items of the keyword batch] -> unit
    uint32_t* bits;
    uint64_t words;
    unsigned long long* found;           // [units] bits turned on
    unsigned long long* stats;           // [0] records checked, [1] records matched
};

// has_phrase_match(token_positions) (src/posting_list.cpp:1771-1789) over one array element: sub[t] = token t's positions in the element (a TokRun cut to
// the element, as field_match_score_array cuts it). P_t = the longest non-descending prefix of sub[t] (a step down ends found_token_sequence's walk, :1732-1736,
// and has_phrase_match's own, :1776-1779). The element matches iff some p in P_0 has uint16(p + t) in P_t for every t >= 1 (the target is a uint16_t
// parameter, :1720: 65535 + 1 = 0). The prefixes are sorted, so a binary search stands for the reference's rescan; same answer.
template <int TMAX>
__device__ inline bool phrase_elem_match(const TokRun (&sub)[TMAX], uint32_t T) {
    uint32_t len[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        len[t] = 0;
        if ((uint32_t)t < T) {
            uint32_t prev = 0, j = 0;
            for (; j < sub[t].n; j++) {
                const uint32_t p = run_pos(sub[t], j);
                if (j != 0 && p < prev) break;
                prev = p;
            }
            len[t] = j;
        }
    }
    for (uint32_t i = 0; i < len[0]; i++) {
        const uint32_t p = run_pos(sub[0], i);
        bool ok = true;
#pragma unroll
        for (int t = 1; t < TMAX; t++) {
            if ((uint32_t)t < T && ok) {
                const uint32_t target = (p + (uint32_t)t) & 0xFFFFu;
                uint32_t lo = 0, hi = len[t];
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (run_pos(sub[t], mid) < target) lo = mid + 1; else hi = mid; }
                ok = lo < len[t] && run_pos(sub[t], lo) == target;
            }
        }
        if (ok) return true;
    }
    return false;
}

// has_phrase_match(its) for one document (:1810-1820): get_offsets groups every token's positions by array element (arr_next_elem restates its loop; a plain
// field's run is one element, 0); an element counts when it holds ALL T tokens (token_positions.size() == its.size()). The elements of a run ascend by array
// index (the indexer writes them in element order, src/index.cpp:1351-1395; field_match_score_array relies on the same), so the T cursors merge.
template <int TMAX>
__device__ inline bool phrase_doc_match(const TokRun (&runs)[TMAX], uint32_t T) {
    ArrCursor cur[TMAX];
    ArrElem el[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; t++) {
        cur[t].i = 0; cur[t].is_last = 0;
        if ((uint32_t)t < T) el[t] = arr_next_elem(runs[t], cur[t]);
        else { el[t].valid = false; el[t].aidx = 0; el[t].start = 0; el[t].n = 0; el[t].last = 0; }
    }
    while (el[0].valid) {
        const uint32_t a = el[0].aidx;
        bool all = true;
#pragma unroll
        for (int t = 1; t < TMAX; t++) {
            if ((uint32_t)t < T) {
                while (el[t].valid && el[t].aidx < a) el[t] = arr_next_elem(runs[t], cur[t]);
                all = all && el[t].valid && el[t].aidx == a;
            }
        }
        if (all) {
            TokRun sub[TMAX];
#pragma unroll
            for (int t = 0; t < TMAX; t++) {
                sub[t] = runs[t];
                sub[t].start = el[t].start; sub[t].n = el[t].n; sub[t].raw_len = el[t].n; sub[t].meta = run_bits(runs[t]);      // (nc = 0: the register cache belongs to the run's own start)
            }
            if (phrase_elem_match<TMAX>(sub, T)) return true;
        }
        el[0] = arr_next_elem(runs[0], cur[0]);
    }
    return false;
}

// grid = the work items of one find launch (the tables the find kernel ran on: same queries / work / part.cnt / hit_off); one thread per hit record, 256 at a
// time. MF: the records of the multi-field find kernels (a string[] field runs there): pos[t * KW_MAX_FIELDS + f], f = the item's driver field — an AND item
// has one field. A match turns the id's bit on; a bit THIS atomicOr turned on counts (found[unit]), as in infix_union_mark_kernel.
template <int TMAX, bool MF>
__global__ __launch_bounds__(PHRASE_THREADS) void kw_phrase_mark_kernel(IndexView ix, const KwQueryDev* __restrict__ queries, const KwWorkItem* __restrict__ work, KwPartials part,
                                                                        const uint32_t* __restrict__ hits_all, const uint64_t* __restrict__ hit_off, PhraseMarkArgs a) {
    constexpr int NP = MF ? TMAX * KW_MAX_FIELDS : TMAX;
    __shared__ KwQueryDev sq;
    __shared__ uint32_t s_list[TMAX];
    const uint32_t t = threadIdx.x;
    const KwWorkItem wi = work[blockIdx.x];
    const uint32_t qi = wi.query & 0x0FFFFFFFu, fld = wi.query >> 28;
    {
        const uint32_t* src = (const uint32_t*)(queries + qi);
        uint32_t* dst = (uint32_t*)&sq;
        for (uint32_t i = t; i < sizeof(KwQueryDev) / 4; i += PHRASE_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const KwQueryDev& q = sq;
    const uint32_t T = q.n_lists < (uint32_t)TMAX ? q.n_lists : (uint32_t)TMAX;
    if (t < (uint32_t)TMAX) s_list[t] = t < T ? (MF ? ix.mf[q.mf_index].list[t][fld] : q.list[t]) : 0u;
    __syncthreads();
    const uint32_t unit = a.unit_of_item[qi];
    uint32_t* mine_bits = a.bits + (uint64_t)unit * a.words;
    const uint32_t count = part.cnt[blockIdx.x];
    const uint32_t* __restrict__ mine = hits_all + hit_off[blockIdx.x] * (uint64_t)(NP + 1);
    uint32_t n_new = 0, n_match = 0;
    for (uint32_t i0 = 0; i0 < count; i0 += PHRASE_THREADS) {
        if (i0 + t >= count) continue;
        uint32_t id;
        uint32_t pos[TMAX];
        if constexpr (TMAX == 3 && !MF) {
            const KwHitRec r = ((const KwHitRec*)mine)[i0 + t];
            id = r.id; pos[0] = r.p0; pos[1] = r.p1; pos[2] = r.p2;
        } else {
            const uint32_t* __restrict__ r = mine + (size_t)(i0 + t) * (NP + 1);
            id = r[0];
#pragma unroll
            for (int k = 0; k < TMAX; k++) pos[k] = (uint32_t)k < T ? r[1 + (MF ? k * KW_MAX_FIELDS + fld : k)] : 0u;
        }
        TokRun runs[TMAX];
        if constexpr (TMAX <= 3 && !MF) {
            uint32_t off_words = 0;
            load_runs_staged<TMAX>(ix, q, pos, T, runs, off_words);          // the T runs level by level, as the score kernel loads them
        } else {
#pragma unroll
            for (int k = 0; k < TMAX; k++) runs[k] = (uint32_t)k < T ? load_run(ix, ix.lists[s_list[k]], pos[k]) : empty_run();
        }
        if (phrase_doc_match<TMAX>(runs, T)) {
            n_match++;
            if ((uint64_t)(id >> 5) < a.words) {
                const uint32_t bit = 1u << (id & 31u);
                n_new += (atomicOr(&mine_bits[id >> 5], bit) & bit) ? 0u : 1u;
            }
        }
    }
    uint32_t n_chk = count > t ? (count - t + PHRASE_THREADS - 1) / PHRASE_THREADS : 0u;
    for (int s = 32; s > 0; s >>= 1) { n_new += __shfl_down(n_new, s, 64); n_match += __shfl_down(n_match, s, 64); n_chk += __shfl_down(n_chk, s, 64); }
    if ((t & 63u) == 0) {
        if (n_new) atomicAdd(&a.found[unit], (unsigned long long)n_new);
        if (n_chk) atomicAdd(&a.stats[0], (unsigned long long)n_chk);
        if (n_match) atomicAdd(&a.stats[1], (unsigned long long)n_match);
    }
}

// one (query, field) of the round — or, mode EXCLUDE, one query with every phrase of every field (handle_exclusion ORs them all, :6300-6318)
struct PhraseFieldDev {
    uint32_t unit_first, n_units;        // its phrases' units, in phrase order; a phrase with an unknown token has none (:5950-5953)
    uint32_t mode;
    int32_t weight;
};

// grid = (query, field) pairs. The fold of :5963-5981 over the field's phrases, word by word with the whole workgroup: a phrase without matches is skipped;
// the first one (and the first one after an intersection that came out EMPTY: field_phrase_match_ids_size == 0 again) is taken as it is, every other one is
// ANDed in and the survivors are counted. acc = the field's bitmap of the round (zeroed), n_acc[pair] its count. EXCLUDE: a plain OR, no count.
__global__ __launch_bounds__(PHRASE_THREADS) void phrase_fold_kernel(const PhraseFieldDev* __restrict__ fields, const uint32_t* __restrict__ ubits,
                                                                    const unsigned long long* __restrict__ found, uint32_t* __restrict__ fbits, uint64_t words,
                                                                    uint32_t* __restrict__ n_acc) {
    __shared__ uint32_t s_sum;
    const PhraseFieldDev f = fields[blockIdx.x];
    uint32_t* acc = fbits + (uint64_t)blockIdx.x * words;
    uint32_t have = 0;                                       // (uniform) field_phrase_match_ids_size
    for (uint32_t p = 0; p < f.n_units; p++) {
        const uint32_t u = f.unit_first + p;
        const uint32_t c = (uint32_t)found[u];
        if (c == 0) continue;                                // (uniform) this_phrase_ids_size == 0, :5963-5967
        const uint32_t* src = ubits + (uint64_t)u * words;
        if (f.mode == PHRASE_MODE_EXCLUDE) {
            for (uint64_t w = threadIdx.x; w < words; w += PHRASE_THREADS) acc[w] |= src[w];
            have = 1;
        } else if (have == 0) {
            for (uint64_t w = threadIdx.x; w < words; w += PHRASE_THREADS) acc[w] = src[w];
            have = c;
        } else {
            if (threadIdx.x == 0) s_sum = 0;
            __syncthreads();
            uint32_t n = 0;
            for (uint64_t w = threadIdx.x; w < words; w += PHRASE_THREADS) { const uint32_t v = acc[w] & src[w]; acc[w] = v; n += (uint32_t)__popc(v); }
            for (int s = 32; s > 0; s >>= 1) n += __shfl_down(n, s, 64);
            if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&s_sum, n);
            __syncthreads();
            have = s_sum;
            __syncthreads();                                 // s_sum is read before the next phrase resets it
        }
    }
    if (threadIdx.x == 0) n_acc[blockIdx.x] = have;
}

// grid = (word chunks, queries): the query's bitmap = the OR of its fields' folded bitmaps (pairs [pair_first[q], pair_first[q + 1])), :5997-6009
__global__ __launch_bounds__(PHRASE_THREADS) void phrase_or_fields_kernel(const uint32_t* __restrict__ fbits, const uint32_t* __restrict__ pair_first, uint32_t* __restrict__ qbits,
                                                                         uint64_t words) {
    const uint64_t w = (uint64_t)blockIdx.x * PHRASE_THREADS + threadIdx.x;
    if (w >= words) return;
    uint32_t v = 0;
    for (uint32_t p = pair_first[blockIdx.y]; p < pair_first[blockIdx.y + 1]; p++) v |= fbits[(uint64_t)p * words + w];
    qbits[(uint64_t)blockIdx.y * words + w] = v;
}

// grid = (x, queries): tm[i] of the query's surviving id list = max over its fields whose capped list — the first min(cut, n_acc) ids of the folded field,
// ascending, expanded to clist + pair * cut — holds ids[i] of 100000 + weight, else 0 (std::map's default, :5993 / :6050). ids / tm: at off[query], cap[query] slots; n: n_ids[query].
__global__ __launch_bounds__(PHRASE_THREADS) void phrase_tm_kernel(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ off, const uint64_t* __restrict__ cap,
                                                                  const uint32_t* __restrict__ n_ids, const uint32_t* __restrict__ pair_first, const PhraseFieldDev* __restrict__ fields,
                                                                  const uint32_t* __restrict__ n_acc, const uint32_t* __restrict__ clist, uint32_t cut, int64_t* __restrict__ tm) {
    const uint32_t q = blockIdx.y;
    const uint32_t n = (uint64_t)n_ids[q] < cap[q] ? n_ids[q] : (uint32_t)cap[q];
    const uint32_t p0 = pair_first[q], p1 = pair_first[q + 1];
    for (uint32_t i = blockIdx.x * PHRASE_THREADS + threadIdx.x; i < n; i += gridDim.x * PHRASE_THREADS) {
        const uint32_t id = ids[off[q] + i];
        int64_t best = 0;
        for (uint32_t p = p0; p < p1; p++) {
            const uint32_t* lst = clist + (uint64_t)p * cut;
            const uint32_t m = n_acc[p] < cut ? n_acc[p] : cut;
            uint32_t lo = 0, hi = m;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (lst[mid] < id) lo = mid + 1; else hi = mid; }
            if (lo < m && lst[lo] == id) { const int64_t s = (int64_t)PHRASE_WEIGHT_BASE + (int64_t)fields[p].weight; if (s > best) best = s; }
        }
        tm[off[q] + i] = best;
    }
}

}  // namespace tsgpu
