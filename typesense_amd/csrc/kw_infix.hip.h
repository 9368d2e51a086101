// kw_infix.hip.h — the front of infix search (Index::search_infix, src/index.cpp:3265-3343; Index::do_infix_search, :6144-6272) for gfx950. Included by
// tsgpu.hip behind kw_kernels.hip.h (it uses BlockIds / ListDesc, unpack_at_nb and idset_expand_range).
//
// The reference walks every token of a field's vocabulary with std::string::find on four pool threads (:3295-3336), merges the posting lists of the
// matching tokens, sorts and uniques the ids (:3338-3340, :6184-6185) and ranks them one by one with the constant text score 100 (:6219-6229). Here:
//   infix_scan_kernel        one pass over the vocabulary mirror (tsgpu_host.h: InfixVocabDev) for ALL queries of the batch that name the field: a workgroup
//                            stages a tile of consecutive tokens into LDS and tests it against every pattern; matches go to per-query lists of term ids
//   infix_union_mark_kernel  the union of the matched tokens' posting lists: one bit per seq_id, set straight from the packed ids arena
//   infix_idlist_set_kernel / infix_idlist_clear_kernel / infix_bits_and_kernel     the filter's bitmap built and ANDed, the excluded ids cleared
//   infix_count_kernel / infix_expand_kernel             bitmap -> ascending device id list (idset_expand_range, shared with kw_idset_expand_kernel)
// The id list is then ranked by the wildcard machinery (kw_wildcard_kernel reads it through KwQueryDev::wild_ids): no second ranking kernel.
#pragma once

namespace tsgpu {

static const uint32_t INFIX_THREADS = 256;
static const uint32_t INFIX_TILE_TOKENS = 256;        // vocabulary slots per workgroup (one per thread)
static const uint32_t INFIX_TILE_BYTES = 8192;      // token bytes staged at a time; a token longer than this takes the slow path
static const uint32_t INFIX_PAT_STRIDE = 256;         // LDS bytes per pattern (TSGPU_MAX_INFIX_PATTERN + 1)
static const uint32_t INFIX_PAT_CHUNK = 32;           // patterns in LDS at a time
static const uint32_t INFIX_EXPAND_WORDS = 2048;      // bitmap words per workgroup of the count / expand kernels
static const uint32_t INFIX_NO_POS = 0xFFFFFFFFu;
static_assert(INFIX_TILE_BYTES % 16 == 0 && INFIX_TILE_BYTES >= 16, "the tile is filled with 16-byte loads");

// The vocabulary mirror of one field as a snapshot sees it. Slot i holds bytes [byte_ptr[i], byte_ptr[i + 1]) and is LIVE for the snapshot of epoch e iff
// born[i] <= e < died[i]: a commit appends slots and writes `died` of the slots it retires, so the arrays are shared by consecutive snapshots and a search
// on an older snapshot still sees exactly its own vocabulary (it never looks beyond its n_slots, and a `died` written later is greater than its epoch).
struct InfixVocabView {
    const uint8_t* bytes;            // arena, 16-byte aligned and allocated 16 bytes beyond its last byte
    const uint32_t* byte_ptr;        // [n_slots + 1]
    const uint32_t* term_id;         // [n_slots]
    const uint32_t* born;            // [n_slots]
    const uint32_t* died;            // [n_slots]
    uint32_t n_slots;
    uint32_t epoch;
};

struct InfixQueryDev {               // one pattern of the batch
    uint32_t pat_off, pat_len;       // its bytes in the batch's pattern arena
    uint32_t max_prefix, max_suffix; // max_extra_prefix / max_extra_suffix (:3305-3307)
    uint32_t list_off;               // where its match list starts in the match arena (capacity: the vocabulary's slots)
    uint32_t pad;
};

struct InfixMarkItem { uint32_t slot, list, blk_begin, blk_end; };      // slot: the query's bitmap of the round
struct InfixIdSeg { uint64_t off; uint32_t cnt, slot; };                // an id list of the upload arena and the bitmap it goes to

// first occurrence of pat[0, m) in tok[0, L) at a position <= last (std::string::find stops at the FIRST occurrence; one beyond max_extra_prefix
// rejects the token whatever follows, so the search ends there); INFIX_NO_POS = none
__device__ inline uint32_t infix_find_first(const uint8_t* tok, uint32_t L, const uint8_t* pat, uint32_t m, uint32_t last) {
    if (m > L) return INFIX_NO_POS;
    const uint32_t end = L - m < last ? L - m : last;
    for (uint32_t p = 0; p <= end; p++) {
        uint32_t i = 0;
        while (i < m && tok[p + i] == pat[i]) i++;
        if (i == m) return p;
    }
    return INFIX_NO_POS;
}

// grid = ceil(n_slots / 256). Every workgroup owns 256 consecutive slots and walks them in sub-tiles of at most INFIX_TILE_BYTES token bytes (cut at token
// boundaries, found by a search over the LDS copy of the byte_ptr slice); the bytes come in with 16-byte loads from the 16-byte-aligned address in front
// of the sub-tile. Thread t tests token t of the sub-tile against every pattern (INFIX_PAT_CHUNK at a time in LDS) inside ITS OWN byte range, so a match
// never spans two tokens. A token longer than the tile is tested from global memory by the whole workgroup: every thread tries positions t, t + 256, ...
// and the smallest wins. Matches are counted with a ballot per wave: one atomicAdd per wave and query, the lanes write behind the base it returned.
__global__ __launch_bounds__(INFIX_THREADS) void infix_scan_kernel(InfixVocabView v, const InfixQueryDev* __restrict__ queries, uint32_t n_queries,
                                                                  const uint8_t* __restrict__ patterns, uint32_t* __restrict__ match_cnt,
                                                                  uint32_t* __restrict__ match_terms) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[INFIX_TILE_BYTES + 32];
    __shared__ __attribute__((aligned(16))) uint8_t s_pat[INFIX_PAT_CHUNK * INFIX_PAT_STRIDE];
    __shared__ InfixQueryDev s_q[INFIX_PAT_CHUNK];
    __shared__ uint32_t s_ptr[INFIX_TILE_TOKENS + 1];
    __shared__ uint32_t s_min;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t s0 = blockIdx.x * INFIX_TILE_TOKENS;
    const uint32_t nt = v.n_slots - s0 < INFIX_TILE_TOKENS ? v.n_slots - s0 : INFIX_TILE_TOKENS;
    for (uint32_t i = t; i <= nt; i += INFIX_THREADS) s_ptr[i] = v.byte_ptr[s0 + i];
    bool live = false;
    uint32_t term = 0;
    if (t < nt) { live = v.born[s0 + t] <= v.epoch && v.epoch < v.died[s0 + t]; term = v.term_id[s0 + t]; }
    uint32_t staged_chunk = INFIX_NO_POS;
    __syncthreads();
    uint32_t cur = 0;
    while (cur < nt) {                                              // (uniform)
        // the sub-tile [cur, e): the most tokens whose bytes fit
        const uint32_t b0 = s_ptr[cur];
        uint32_t lo = cur, hi = nt;
        while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (s_ptr[mid] - b0 <= INFIX_TILE_BYTES) lo = mid; else hi = mid - 1; }
        const bool big = lo == cur;                                 // token `cur` alone is longer than the tile
        const uint32_t e = big ? cur + 1 : lo;
        const uint32_t a0 = b0 & ~15u;
        if (!big) {
            const uint32_t n16 = (s_ptr[e] - a0 + 15u) >> 4;
            for (uint32_t i = t; i < n16; i += INFIX_THREADS) ((uint4*)s_tile)[i] = ((const uint4*)(v.bytes + a0))[i];
        }
        const bool big_live = big && v.born[s0 + cur] <= v.epoch && v.epoch < v.died[s0 + cur];      // (uniform)
        const bool mine = live && t >= cur && t < e;
        const uint32_t my_off = mine ? s_ptr[t] - a0 : 0, my_len = mine ? s_ptr[t + 1] - s_ptr[t] : 0;
        for (uint32_t c0 = 0; c0 < n_queries; c0 += INFIX_PAT_CHUNK) {
            const uint32_t nc = n_queries - c0 < INFIX_PAT_CHUNK ? n_queries - c0 : INFIX_PAT_CHUNK;
            __syncthreads();                                        // the tile is filled / the previous chunk's patterns have been read
            if (staged_chunk != c0) {
                for (uint32_t i = t; i < nc * (uint32_t)(sizeof(InfixQueryDev) / 4); i += INFIX_THREADS) ((uint32_t*)s_q)[i] = ((const uint32_t*)(queries + c0))[i];
                __syncthreads();
                for (uint32_t j = 0; j < nc; j++)
                    for (uint32_t i = t; i < s_q[j].pat_len; i += INFIX_THREADS) s_pat[j * INFIX_PAT_STRIDE + i] = patterns[s_q[j].pat_off + i];
                staged_chunk = c0;
                __syncthreads();
            }
            for (uint32_t j = 0; j < nc; j++) {
                const InfixQueryDev q = s_q[j];
                const uint8_t* pat = s_pat + j * INFIX_PAT_STRIDE;
                bool match = false;
                if (!big) {
                    if (mine) {
                        const uint32_t p = infix_find_first(s_tile + my_off, my_len, pat, q.pat_len, q.max_prefix);
                        match = p != INFIX_NO_POS && my_len - (p + q.pat_len) <= q.max_suffix;
                    }
                } else if (big_live) {                              // (uniform branch: barriers inside)
                    const uint32_t L = s_ptr[cur + 1] - b0;
                    if (t == 0) s_min = INFIX_NO_POS;
                    __syncthreads();
                    if (q.pat_len <= L) {
                        const uint8_t* tok = v.bytes + b0;
                        const uint32_t end = L - q.pat_len < q.max_prefix ? L - q.pat_len : q.max_prefix;
                        for (uint32_t p = t; p <= end; p += INFIX_THREADS) {
                            uint32_t i = 0;
                            while (i < q.pat_len && tok[p + i] == pat[i]) i++;
                            if (i == q.pat_len) { atomicMin(&s_min, p); break; }      // (this thread's later positions are greater)
                        }
                    }
                    __syncthreads();
                    const uint32_t p = s_min;
                    match = t == cur && p != INFIX_NO_POS && L - (p + q.pat_len) <= q.max_suffix;
                    __syncthreads();                                // s_min is read before the next pattern resets it
                }
                const unsigned long long bal = __ballot(match);
                if (bal) {                                          // (wave-uniform)
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&match_cnt[c0 + j], (uint32_t)__popcll(bal));
                    base = __shfl(base, 0, 64);
                    if (match) match_terms[(uint64_t)q.list_off + base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = term;
                }
            }
        }
        __syncthreads();                                            // everyone is done with the tile before the next one overwrites it
        cur = e;
    }
}

// grid = work items (query bitmap, list, block range). Thread t decodes slot t of every block of the range from the packed ids arena and sets the id's bit
// in the query's bitmap; a bit that THIS atomicOr turned on is a new member of the union, so the marks count it (found[slot]), as in
// kw_idset_mark_items_kernel. Part-filled blocks (incremental commits) decode their n_ids slots; ids beyond the bitmap are left out.
__global__ __launch_bounds__(INFIX_THREADS) void infix_union_mark_kernel(const InfixMarkItem* __restrict__ items, const ListDesc* __restrict__ lists,
                                                                        const BlockIds* __restrict__ blk_ids, const uint32_t* __restrict__ ids_payload,
                                                                        uint32_t* __restrict__ bits, uint64_t words_per_query, unsigned long long* __restrict__ found) {
    const InfixMarkItem it = items[blockIdx.x];
    const ListDesc d = lists[it.list];
    uint32_t* mine = bits + (uint64_t)it.slot * words_per_query;
    uint32_t c = 0;
    for (uint32_t b = it.blk_begin; b < it.blk_end; b++) {
        const BlockIds m = blk_ids[d.blk_base + b];
        const uint32_t n = m.n_ids_bits & 0xFFFFu;
        if (threadIdx.x < n) {
            const uint32_t id = m.first_id + unpack_at_nb(ids_payload + d.ids_base + m.ids_woff, threadIdx.x, m.n_ids_bits >> 16);
            if ((uint64_t)(id >> 5) < words_per_query) {
                const uint32_t bit = 1u << (id & 31u);
                c += (atomicOr(&mine[id >> 5], bit) & bit) ? 0u : 1u;
            }
        }
    }
    for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&found[it.slot], (unsigned long long)c);
}

// grid = (id lists, y): sets the bit of every id of a list in bitmap `slot` (a filter's bitmap: the sibling of vec_qmask_build_kernel for plain seq_id
// bitmaps). Ids beyond the bitmap are left out.
__global__ __launch_bounds__(INFIX_THREADS) void infix_idlist_set_kernel(const uint32_t* __restrict__ ids, const InfixIdSeg* __restrict__ segs, uint32_t* __restrict__ bits,
                                                                        uint64_t words_per_query) {
    const InfixIdSeg sg = segs[blockIdx.x];
    uint32_t* mine = bits + (uint64_t)sg.slot * words_per_query;
    for (uint32_t i = blockIdx.y * INFIX_THREADS + threadIdx.x; i < sg.cnt; i += gridDim.y * INFIX_THREADS) {
        const uint32_t id = ids[sg.off + i];
        if ((uint64_t)(id >> 5) < words_per_query) atomicOr(&mine[id >> 5], 1u << (id & 31u));
    }
}

// grid = (id lists, y): clears the bits of a list of ASCENDING ids (curated_ids_sorted, :6190-6197). The thread that holds the first id of a bitmap word
// gathers the word's ids (they are neighbours in the list) and clears them with one plain store: one writer per word, no atomics.
__global__ __launch_bounds__(INFIX_THREADS) void infix_idlist_clear_kernel(const uint32_t* __restrict__ ids, const InfixIdSeg* __restrict__ segs, uint32_t* __restrict__ bits,
                                                                          uint64_t words_per_query) {
    const InfixIdSeg sg = segs[blockIdx.x];
    const uint32_t* src = ids + sg.off;
    uint32_t* mine = bits + (uint64_t)sg.slot * words_per_query;
    for (uint32_t i = blockIdx.y * INFIX_THREADS + threadIdx.x; i < sg.cnt; i += gridDim.y * INFIX_THREADS) {
        const uint32_t w = src[i] >> 5;
        if ((i > 0 && (src[i - 1] >> 5) == w) || (uint64_t)w >= words_per_query) continue;
        uint32_t mask = 0;
        for (uint32_t j = i; j < sg.cnt && (src[j] >> 5) == w; j++) mask |= 1u << (src[j] & 31u);
        mine[w] &= ~mask;
    }
}

// bits[slot] &= fbits[fslot[slot]] for the slots that carry a filter (fslot[slot] != INFIX_NO_POS: its bitmap among the filters'). grid = (word chunks, slots)
__global__ __launch_bounds__(INFIX_THREADS) void infix_bits_and_kernel(uint32_t* __restrict__ bits, const uint32_t* __restrict__ fbits, const uint32_t* __restrict__ fslot,
                                                                      uint64_t words_per_query) {
    const uint32_t fs = fslot[blockIdx.y];
    if (fs == INFIX_NO_POS) return;
    const uint64_t w = (uint64_t)blockIdx.x * INFIX_THREADS + threadIdx.x;
    if (w < words_per_query) bits[(uint64_t)blockIdx.y * words_per_query + w] &= fbits[(uint64_t)fs * words_per_query + w];
}

// grid = (chunks of INFIX_EXPAND_WORDS words, slots): the set bits of each chunk
__global__ __launch_bounds__(INFIX_THREADS) void infix_count_kernel(const uint32_t* __restrict__ bits, uint64_t words_per_query, uint32_t* __restrict__ chunk_cnt) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint64_t w0 = (uint64_t)blockIdx.x * INFIX_EXPAND_WORDS;
    const uint64_t w1 = w0 + INFIX_EXPAND_WORDS < words_per_query ? w0 + INFIX_EXPAND_WORDS : words_per_query;
    uint32_t c = 0;
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += INFIX_THREADS) c += (uint32_t)__popc(bits[(uint64_t)blockIdx.y * words_per_query + w]);
    for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = s_sum;
}

// grid = (chunks, slots): the ascending ids of a chunk go behind those of the slot's earlier chunks (their counts summed here); the last chunk leaves the
// slot's total in n_ids[slot]. out_off[slot] / out_cap[slot]: the slot's segment of the id arena.
__global__ __launch_bounds__(INFIX_THREADS) void infix_expand_kernel(const uint32_t* __restrict__ bits, uint64_t words_per_query, const uint32_t* __restrict__ chunk_cnt,
                                                                    uint32_t* __restrict__ out, const uint64_t* __restrict__ out_off, const uint64_t* __restrict__ out_cap,
                                                                    uint32_t* __restrict__ n_ids) {
    __shared__ uint32_t s_before;
    if (threadIdx.x == 0) s_before = 0;
    __syncthreads();
    const uint32_t* cc = chunk_cnt + (uint64_t)blockIdx.y * gridDim.x;
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += INFIX_THREADS) c += cc[i];
    for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_before, c);
    __syncthreads();
    const uint32_t before = s_before;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) n_ids[blockIdx.y] = before + cc[blockIdx.x];
    if (cc[blockIdx.x] == 0) return;                                 // (uniform)
    const uint64_t w0 = (uint64_t)blockIdx.x * INFIX_EXPAND_WORDS;
    const uint64_t w1 = w0 + INFIX_EXPAND_WORDS < words_per_query ? w0 + INFIX_EXPAND_WORDS : words_per_query;
    idset_expand_range(bits + (uint64_t)blockIdx.y * words_per_query, w0, w1, out + out_off[blockIdx.y], before, out_cap[blockIdx.y]);
}

}  // namespace tsgpu
