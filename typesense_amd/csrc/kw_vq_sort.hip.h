// kw_vq_sort.hip.h — the `_vector_query(field:([...]))` sort slot (TSGPU_SORT_VECTOR_QUERY) of the keyword kernels. Included by kw_kernels.hip.h, inside
// namespace tsgpu, behind sort_scores (it patches what sort_scores left in the slot).
//
// Index::compute_sort_scores, src/index.cpp:5837-5851: per matched document, getDataByLabel(seq_id) and ONE dist_func(query, row) — 4 x dim bytes of row
// per match; a document without a live row scores float_to_int64_t(2.0f). The score stage of the keyword kernels holds one hit per LANE: a per-lane walk
// over a row would touch 64 cache lines per load. So the slot is evaluated COOPERATIVELY by the wavefront, after the per-lane sort_scores call, at a point
// every lane reaches: the wave's emitting hits are taken 16 at a time (four lanes per hit, 16-byte loads: ip_dot16_quad, dim % 16 == 0) or four at a time
// (16 lanes per hit: ip_distance_group16, any dim) — the functions of vec_ip_order.hip.h, hence the bits of tsgpu_vec_distances and the k-NN paths —
// and each distance is shuffled back to the lane that owns the hit. Hits that are not emitted (excluded ids, ids outside the filter) cost nothing.
// The query vector is read from global memory (every quad reads the same addresses: L1/L2 hits); the score kernels have no LDS to spare.
#pragma once

static const uint32_t KW_SORT_VECTOR_QUERY = 9;            // TSGPU_SORT_VECTOR_QUERY
static const uint32_t KW_VQ_NO_ROW = 0xFFFFFFFFu;

// the row the key's field holds for a document, KW_VQ_NO_ROW = none (unknown label, deleted row: getDataByLabel throws, :5843-5847)
__device__ inline uint32_t vq_row_of(const SortKeyDesc& d, uint32_t seq_id) {
    uint32_t row = seq_id;                                  // identity numbering: label == row
    if (d.vq_row_of_seq) row = seq_id < d.vq_map_len ? d.vq_row_of_seq[seq_id] : KW_VQ_NO_ROW;
    if (row >= d.vq_n_rows || !d.vq_row_ok[row]) row = KW_VQ_NO_ROW;
    return row;
}

// Distances of the wave's lanes with row != KW_VQ_NO_ROW to the key's query; EVERY lane of the wave calls it, d is wave-uniform. Returns the distance of
// the calling lane's own row (unspecified for a lane without one).
// The row walk keeps 8 x 16 bytes of a row in flight per lane: registers that are the kernel's whether or not a query of the launch names the slot. So the
// kernels carry this code behind a template flag of its own (VQ), and only a launch that has such a query takes those instantiations: the filtered, excluded
// and `_eval` launches keep the kernels they had (profiles/r07/vq_sort_resource_usage.txt).
__device__ inline float wave_vq_distances(const SortKeyDesc& d, uint32_t row) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long have = __ballot(row != KW_VQ_NO_ROW ? 1 : 0);
    float dist = 0.0f;
    if (!have) return dist;                                 // (wave-uniform)
    const uint32_t spare = __shfl(row, __ffsll((long long)have) - 1);      // idle quads / groups recompute a row that exists (keeps the shuffles uniform)
    const uint32_t dim = d.vq_dim, L = d.vq_ip_lanes;
    const float* __restrict__ X = d.vq_X;
    if (dim % 16 == 0) {
        for (uint32_t trip = 0; trip < 4; trip++) {         // quad g takes the hit of lane 16 * trip + g
            if (((have >> (16 * trip)) & 0xFFFFull) == 0) continue;
            uint32_t r = __shfl(row, (int)(16 * trip + (lane >> 2)));
            if (r == KW_VQ_NO_ROW) r = spare;
            const float dd = ip_add(1.0f, -ip_dot16_quad<8>(d.vq_q, X + (size_t)r * dim, dim, lane & 3u, L));
            const float back = __shfl(dd, (int)((lane & 15u) << 2));
            if ((lane >> 4) == trip) dist = back;
        }
    } else {
        for (uint32_t trip = 0; trip < 16; trip++) {        // 16-lane group g takes the hit of lane 4 * trip + g
            if (((have >> (4 * trip)) & 0xFull) == 0) continue;
            uint32_t r = __shfl(row, (int)(4 * trip + (lane >> 4)));
            if (r == KW_VQ_NO_ROW) r = spare;
            const float dd = ip_distance_group16(d.vq_q, X + (size_t)r * dim, dim, lane & 15u, L);
            const float back = __shfl(dd, (int)((lane & 3u) << 4));
            if ((lane >> 2) == trip) dist = back;
        }
    }
    return dist;
}

// Overwrites the TSGPU_SORT_VECTOR_QUERY slots of h for the wave's emitting lanes. EVERY lane of the wave calls it (emit = false: the lane has no hit, q is
// not read). q is the lane's query: one per workgroup in the keyword kernels, one per candidate combination in group_by — lanes are served key by key.
__device__ inline void wave_vq_sort_patch(const IndexView& ix, const KwQueryDev& q, uint32_t seq_id, bool emit, ScoredHit& h) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const bool want = emit && i < (int)q.n_sort && q.sort_kind[i] == KW_SORT_VECTOR_QUERY;
        unsigned long long pending = __ballot(want ? 1 : 0);
        if (!pending) continue;                             // (wave-uniform: no lane of the wave has the slot)
        const uint32_t my_key = want ? (uint32_t)q.sort_col[i] : 0xFFFFFFFFu;
        int64_t v = 0;
        while (pending) {
            const uint32_t key = __shfl(my_key, __ffsll((long long)pending) - 1);
            const bool mine = want && my_key == key;
            pending &= ~__ballot(mine ? 1 : 0);
            const SortKeyDesc& d = ix.sort_keys[key < KW_SORT_KEY_SLOTS ? key : 0];
            const bool vq = d.form == SORT_KEY_FORM_VECTOR_QUERY;          // (the planner checked the handle's form; a key of the other form has no rows)
            const uint32_t row = mine && vq ? vq_row_of(d, seq_id) : KW_VQ_NO_ROW;
            float dist = wave_vq_distances(d, row);
            if (mine) {
                if (row == KW_VQ_NO_ROW) dist = 2.0f;                      // :5846
                else if (dist > d.vq_threshold) dist = __uint_as_float(0x7F7FFFFFu);   // std::numeric_limits<float>::max() (:5848-5850); equal stays
                v = float_to_int64_dev(dist);
            }
        }
        if (want) {
            if (q.sort_order[i] == -1) v = (int64_t)(0ull - (uint64_t)v);
            if (i == 0) h.s0 = v; else if (i == 1) h.s1 = v; else h.s2 = v;
        }
    }
}
