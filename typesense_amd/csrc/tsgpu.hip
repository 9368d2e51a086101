// tsgpu.hip — implementation of the C-ABI of include/tsgpu.h: context, index mirror upload, and the batched
// keyword search (seam B1). Host code here only plans the launches (resolve terms, order lists, cut work
// items); all scoring happens in kw_kernels.hip.h on the GPU. There is no CPU fallback: a query this
// library does not accelerate is reported per query as TSGPU_ERR_UNSUPPORTED and left to the caller.
#include "tsgpu_host.h"
#if defined(__linux__)
#include <sys/prctl.h>
#include <time.h>
#endif
#include <cmath>
#include "kw_kernels.hip.h"
#include "kw_infix.hip.h"
#include "kw_phrase.hip.h"
#include "kw_plan.hip.h"
#include "kw_plan_digest.h"
#include "kw_translate.h"

using namespace tsgpu;

namespace {


uint64_t now_us() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
               std::chrono::system_clock::now().time_since_epoch()).count();
}

int upload(DevBuf& dst, const void* src, size_t bytes, hipStream_t s) {
    int rc = dst.reserve(bytes ? bytes : 16);
    if (rc) return rc;
    if (bytes) TSGPU_HIP_TRY(hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, s));
    return TSGPU_OK;
}

int refresh_column_table(tsgpu_ctx* ctx) {
    std::vector<const int64_t*> ptrs(ctx->columns.size());
    std::vector<uint32_t> lens(ctx->columns.size());
    for (size_t i = 0; i < ctx->columns.size(); i++) { ptrs[i] = ctx->columns[i].data.as<int64_t>(); lens[i] = ctx->columns[i].n; }
    int rc = upload(ctx->d_col_ptrs, ptrs.data(), ptrs.size() * sizeof(void*), ctx->stream);
    if (rc) return rc;
    rc = upload(ctx->d_col_len, lens.data(), lens.size() * sizeof(uint32_t), ctx->stream);
    if (rc) return rc;
    TSGPU_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TSGPU_OK;
}

// lays 64-byte-aligned pieces one behind the other (the plan image, the device planner's buffers): place(bytes) -> offset
struct Placer { size_t bytes = 0; size_t operator()(size_t b) { const size_t at = (bytes + 63) & ~(size_t)63; bytes = at + b; return at; } };
// the hit buffer's budget in records of rec_bytes (options kw_hit_buffer_records / kw_hit_buffer_mb)
uint64_t hit_budget_records(const tsgpu_ctx* ctx, size_t rec_bytes) { return ctx->kw_hit_buffer_records ? ctx->kw_hit_buffer_records : ((uint64_t)ctx->kw_hit_buffer_mb << 20) / rec_bytes; }
// the Topster capacity ladder of the kernels that exist at 512, 1024 AND 2048: f(std::integral_constant<int, CAP>)
template <class F>
void with_cap(int cap, F&& f) {
    if (cap == 512) f(std::integral_constant<int, 512>());
    else if (cap == 1024) f(std::integral_constant<int, 1024>());
    else f(std::integral_constant<int, 2048>());
}

IndexView make_view(tsgpu_ctx* ctx, const Snapshot& sn) {
    IndexView v;
    v.lists = sn.lists.as<ListDesc>();
    v.blk_last = sn.ar ? sn.ar->blk_last.as<uint32_t>() : nullptr;
    v.blk_ids = sn.ar ? sn.ar->blk_ids.as<BlockIds>() : nullptr;
    v.blk_meta = sn.ar ? sn.ar->blk_meta.as<BlockMeta>() : nullptr;
    v.ids_payload = sn.ar ? sn.ar->ids_payload.as<uint32_t>() : nullptr;
    v.payload = sn.ar ? sn.ar->payload.as<uint32_t>() : nullptr;
    v.columns = ctx->d_col_ptrs.as<const int64_t*>();
    v.column_len = ctx->d_col_len.as<uint32_t>();
    v.n_columns = (uint32_t)ctx->columns.size();
    v.num_docs = ctx->num_docs;
    v.iddir = sn.dir_pool ? sn.dir_pool->buf.as<uint2>() : nullptr;
    v.iddir_slot_entries = sn.dir_pool ? sn.dir_pool->slot_entries : 0u;
    v.iddir_cap_ids = sn.dir_pool ? sn.dir_pool->cap_ids : 0u;
    v.prof = ctx->d_prof.as<unsigned long long>();
    v.touched = nullptr;                              // per batch, option kw_count_touched
    v.mf = nullptr;                                   // per lane: set by the batch
    v.fbits = nullptr;
    v.t0 = nullptr; v.ticks_per_us = 100; v.cutoff = nullptr;
    v.find_dir_span = ctx->kw_find_dir_tile ? (uint32_t)(ctx->kw_find_dir_span_pct * (long long)(KW_FIND_PIPE_WORDS * KW_THREADS * 16) / 100) : 0u;      // (one tile buffer: 2 words per 32 doc ids)
    v.sort_keys = ctx->d_sort_keys.as<SortKeyDesc>();
    return v;
}

template <int TMAX, int CAP>
void launch_search(hipStream_t s, uint32_t n_work, const IndexView& v, const KwQueryDev* q, const KwWorkItem* w,
                   const KwPartials& part, const uint32_t* aux, uint32_t* ids_out, bool s2, bool vq = false) {
    // s2 = some query of the launch sorts by three keys; the two-key build (CAP 512 only) has a smaller LDS footprint
    // vq = some query of the launch has a TSGPU_SORT_VECTOR_QUERY slot: the instantiations with the wave-cooperative distance code (three-key build only)
    if (vq) hipLaunchKernelGGL((kw_search_kernel<TMAX, CAP, true, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
    else if (CAP == 512 && !s2) hipLaunchKernelGGL((kw_search_kernel<TMAX, CAP, CAP != 512>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
    else hipLaunchKernelGGL((kw_search_kernel<TMAX, CAP, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
}

// two-kernel form: find (intersection -> hit records) then score (hit records -> partial top-K)
template <int TMAX>
void launch_find_score(int cap, hipStream_t s, uint32_t n_work, const IndexView& v, const KwQueryDev* q, const KwWorkItem* w, const KwPartials& part,
                       const uint32_t* aux, uint32_t* ids_out, bool s2, uint32_t* hits, const uint64_t* hit_off, hipEvent_t mid_ev = nullptr, bool pair = false, bool plain = false, bool vq = false,
                       const PhraseMarkArgs* phrase = nullptr) {
    if (pair && v.touched) hipLaunchKernelGGL((kw_find2_kernel<TMAX, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, hits, hit_off);   // the byte-counting instantiation (measurement option)
    else if (pair) hipLaunchKernelGGL((kw_find2_kernel<TMAX>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, hits, hit_off);
    else hipLaunchKernelGGL((kw_search_kernel<TMAX, 512, true, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    if (mid_ev) (void)hipEventRecord(mid_ev, s);           // find | score boundary of the batch's first group (tsgpu_timings::kw_find_ms)
    if (phrase) {                                          // the phrase front (kw_phrase.hip.h): the adjacency check reads the hit records; nothing is scored
        hipLaunchKernelGGL((kw_phrase_mark_kernel<TMAX, false>), dim3(n_work), dim3(PHRASE_THREADS), 0, s, v, q, w, part, hits, hit_off, *phrase);
        return;
    }
    if (vq) with_cap(cap, [&](auto c) { hipLaunchKernelGGL((kw_score_kernel<TMAX, decltype(c)::value, true, false, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off); });
    else if (cap == 512 && !s2 && plain && !ids_out) hipLaunchKernelGGL((kw_score_kernel<TMAX, 512, false, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else if (cap == 512 && !s2) hipLaunchKernelGGL((kw_score_kernel<TMAX, 512, false>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else if (cap == 512) hipLaunchKernelGGL((kw_score_kernel<TMAX, 512, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else if (cap == 1024) hipLaunchKernelGGL((kw_score_kernel<TMAX, 1024, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else hipLaunchKernelGGL((kw_score_kernel<TMAX, 2048, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
}

template <int TMAX>
void launch_search_mf_cap(int cap, hipStream_t s, uint32_t n_work, const IndexView& v, const KwQueryDev* q, const KwWorkItem* w,
                          const KwPartials& part, const uint32_t* aux, uint32_t* ids_out, bool vq = false) {
    if (vq && cap == 512) hipLaunchKernelGGL((kw_search_mf_kernel<TMAX, 512, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
    else if (vq) hipLaunchKernelGGL((kw_search_mf_kernel<TMAX, 1024, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
    else if (cap == 512) hipLaunchKernelGGL((kw_search_mf_kernel<TMAX, 512>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
    else hipLaunchKernelGGL((kw_search_mf_kernel<TMAX, 1024>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, (uint32_t*)nullptr, (const uint64_t*)nullptr);
}
// two-kernel form of the multi-field search (k + 256 <= 1024 there); oc: queries with filter + excluded ids, counted in id order between the two
struct MfOrderedCount { const uint32_t* jobs = nullptr; uint32_t n_jobs = 0, table_first = 0; const KwWorkItem* work_all = nullptr; KwPartials part_all{}; };
template <int TMAX>
void launch_find_score_mf(int cap, hipStream_t s, uint32_t n_work, const IndexView& v, const KwQueryDev* q, const KwWorkItem* w, const KwPartials& part,
                          const uint32_t* aux, uint32_t* ids_out, uint32_t* hits, const uint64_t* hit_off, const MfOrderedCount& oc, bool plain = false, int pipelined_lists = 0, bool vq = false,
                          const PhraseMarkArgs* phrase = nullptr) {
    // pipelined_lists: 2 / 4 = the pipelined find kernel's instantiation that covers every multi-field query of the launch (kw_find_mf2.hip.h); 0 = kw_search_mf_kernel.
    // Same hit records either way.
    if (pipelined_lists == 2) hipLaunchKernelGGL((kw_find_mf2_kernel<TMAX, 2>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, hits, hit_off);
    else if (pipelined_lists == 4) hipLaunchKernelGGL((kw_find_mf2_kernel<TMAX, 4>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, hits, hit_off);
    else hipLaunchKernelGGL((kw_search_mf_kernel<TMAX, 512, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    if (phrase) {                                          // (as in launch_find_score)
        hipLaunchKernelGGL((kw_phrase_mark_kernel<TMAX, true>), dim3(n_work), dim3(PHRASE_THREADS), 0, s, v, q, w, part, hits, hit_off, *phrase);
        return;
    }
    if (oc.n_jobs) hipLaunchKernelGGL((kw_mf_ordered_count_kernel<TMAX>), dim3(oc.n_jobs), dim3(64), 0, s, q, oc.work_all, oc.part_all, hits, hit_off, oc.table_first, aux, oc.jobs);
    if (vq && cap == 512) hipLaunchKernelGGL((kw_score_kernel<TMAX, 512, true, true, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else if (vq) hipLaunchKernelGGL((kw_score_kernel<TMAX, 1024, true, true, false, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else if (cap == 512 && plain && !ids_out && !oc.n_jobs) hipLaunchKernelGGL((kw_score_kernel<TMAX, 512, true, true, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else if (cap == 512) hipLaunchKernelGGL((kw_score_kernel<TMAX, 512, true, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
    else hipLaunchKernelGGL((kw_score_kernel<TMAX, 1024, true, true>), dim3(n_work), dim3(KW_THREADS), 0, s, v, q, w, part, aux, ids_out, hits, hit_off);
}

}  // namespace

extern "C" {

int tsgpu_abi_version(void) { return TSGPU_ABI_VERSION; }
const char* tsgpu_last_error(void) { return tls_error().c_str(); }

int tsgpu_create(int device_ordinal, tsgpu_ctx** out) {
    if (!out) return fail(TSGPU_ERR_INVALID, "tsgpu_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(TSGPU_ERR_DEVICE, "tsgpu_create: no HIP device visible (this library has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(TSGPU_ERR_INVALID, "tsgpu_create: bad device ordinal");
    TSGPU_HIP_TRY(hipSetDevice(device_ordinal));
    tsgpu_ctx* ctx = new (std::nothrow) tsgpu_ctx;
    if (!ctx) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_create: host allocation failed");
    ctx->device = device_ordinal;
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_ordinal) == hipSuccess && khz >= 1000) ctx->ticks_per_us = (uint32_t)(khz / 1000);
    }
    std::atomic_store(&ctx->snap, std::shared_ptr<const Snapshot>(std::make_shared<Snapshot>()));
    bool good = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    for (auto& ev : ctx->ev) good = good && hipEventCreate(&ev) == hipSuccess;
    for (int l = 0; l < tsgpu_ctx::N_LANES && good; l++) {
        KwLane& L = ctx->lanes[l];
        if (l == 0) { L.stream = ctx->stream; L.own_stream = false; }          // lane 0 shares the vector path's stream
        else good = good && hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) == hipSuccess;
        for (auto& ev : L.ev) good = good && hipEventCreate(&ev) == hipSuccess;
        good = good && hipEventCreateWithFlags(&L.ev_block, hipEventBlockingSync | hipEventDisableTiming) == hipSuccess;
        good = good && hipEventCreateWithFlags(&L.ev_chain, hipEventDisableTiming) == hipSuccess;
    }
    // the sort-key table (tsgpu_sort_key_create_eval): every slot exists from the start, so the pointer the kernels hold never moves
    static_assert(TSGPU_SORT_KEY_SLOTS == KW_SORT_KEY_SLOTS && TSGPU_SORT_KEY_SLOTS <= 65536, "a handle is the uint16_t a sort slot carries");
    good = good && hipStreamCreateWithFlags(&ctx->sk_stream, hipStreamNonBlocking) == hipSuccess;
    good = good && ctx->d_sort_keys.reserve((size_t)TSGPU_SORT_KEY_SLOTS * sizeof(SortKeyDesc)) == TSGPU_OK;
    good = good && hipMemset(ctx->d_sort_keys.p, 0, (size_t)TSGPU_SORT_KEY_SLOTS * sizeof(SortKeyDesc)) == hipSuccess;
    ctx->sort_keys.resize(TSGPU_SORT_KEY_SLOTS);
    for (uint32_t h = TSGPU_SORT_KEY_SLOTS; h-- > 0;) ctx->sk_free.push_back((uint16_t)h);      // (handed out from 0 upwards)
    if (!good) { tsgpu_destroy(ctx); return fail(TSGPU_ERR_DEVICE, "tsgpu_create: stream / event creation failed"); }
    *out = ctx;
    return ok();
}

void tsgpu_vec_destroy_all(tsgpu_ctx* ctx);   // tsgpu_vec.hip
void tsgpu_facet_destroy_all(tsgpu_ctx* ctx); // tsgpu_facet.hip
void tsgpu_groupby_destroy(tsgpu_ctx* ctx);   // tsgpu_groupby.inc.h

void tsgpu_destroy(tsgpu_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    tsgpu_vec_destroy_all(ctx);
    tsgpu_facet_destroy_all(ctx);
    tsgpu_groupby_destroy(ctx);
    for (auto& L : ctx->lanes) L.release();
    for (auto& b : ctx->infix_buf) b.release();
    for (auto& b : ctx->phrase_buf) b.release();
    std::atomic_store(&ctx->infix_test_snap, std::shared_ptr<const Snapshot>());
    if (ctx->infix_stream) (void)hipStreamDestroy(ctx->infix_stream);
    ctx->infix.clear();                              // (the staged vocabularies' device arrays go to the retire bin, drained below)
    std::atomic_store(&ctx->snap, std::shared_ptr<const Snapshot>());
    ctx->retire_bin->drain();
    deferred_frees().drain();
    ctx->d_col_ptrs.release(); ctx->d_col_len.release(); ctx->d_prof.release();
    for (auto& c : ctx->columns) c.data.release();
    for (auto& k : ctx->sort_keys) k.buf.release();
    ctx->d_sort_keys.release();
    if (ctx->sk_stream) (void)hipStreamDestroy(ctx->sk_stream);
    for (auto& ev : ctx->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->aux_ev) if (ev) (void)hipEventDestroy(ev);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int tsgpu_set_stream(tsgpu_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(TSGPU_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::lock_guard<std::mutex> lk0(ctx->lanes[0].mu);
    if (ctx->own_stream && ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    if (hip_stream) { ctx->stream = (hipStream_t)hip_stream; ctx->own_stream = false; }
    else {
        TSGPU_HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    ctx->lanes[0].stream = ctx->stream;
    return ok();
}

uint64_t tsgpu_vec_device_bytes(tsgpu_ctx* ctx);   // tsgpu_vec.hip

uint64_t tsgpu_device_bytes(tsgpu_ctx* ctx) {
    if (!ctx) return 0;
    uint64_t b = ctx->snapshot()->bytes;
    for (auto& c : ctx->columns) b += c.data.cap;
    return b + tsgpu_vec_device_bytes(ctx);
}

// ---------------------------------------------------------------- keyword index mirror: tsgpu_index.hip (posting lists), columns here
int tsgpu_column_set(tsgpu_ctx* ctx, uint32_t column_id, const int64_t* values, const uint8_t* present, uint32_t n, int mem) {
    if (!ctx) return fail(TSGPU_ERR_INVALID, "ctx is NULL");
    if (column_id >= 4096) return fail(TSGPU_ERR_INVALID, "tsgpu_column_set: column_id too large");
    if (n && !values) return fail(TSGPU_ERR_INVALID, "tsgpu_column_set: values is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (ctx->columns.size() <= column_id) ctx->columns.resize(column_id + 1);
    ColumnDev& c = ctx->columns[column_id];
    int rc = c.data.reserve((size_t)std::max<uint32_t>(n, 1) * sizeof(int64_t));
    if (rc) return rc;
    if (mem == TSGPU_MEM_DEVICE) {
        if (present) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_column_set: presence mask with device values is not supported");
        TSGPU_HIP_TRY(hipMemcpyAsync(c.data.p, values, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
        TSGPU_HIP_TRY(hipStreamSynchronize(ctx->stream));
        c.host.resize(n);
        if (n) TSGPU_HIP_TRY(hipMemcpy(c.host.data(), c.data.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    } else {
        c.host.assign(values, values + n);
        if (present) for (uint32_t i = 0; i < n; i++) if (!present[i]) c.host[i] = INT64_MIN;   // default_score, src/index.cpp:5696
        if (n) TSGPU_HIP_TRY(hipMemcpy(c.data.p, c.host.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    c.n = n;
    return refresh_column_table(ctx);
}

int tsgpu_set_num_docs(tsgpu_ctx* ctx, uint32_t num_docs) {
    if (!ctx) return fail(TSGPU_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->num_docs = num_docs;
    ctx->num_docs_set = true;
    return ok();
}

// ---------------------------------------------------------------- `_eval` sort keys (TSGPU_SORT_EVAL)
int tsgpu_sort_key_create_eval(tsgpu_ctx* ctx, const uint32_t* const* ids, const uint32_t* n_ids, const int64_t* scores, uint32_t n_expr, uint16_t* handle_out) {
    if (!ctx || !handle_out || !scores || !n_ids || !ids) return fail(TSGPU_ERR_INVALID, "tsgpu_sort_key_create_eval: NULL argument");
    if (n_expr < 1 || n_expr > 255) return fail(TSGPU_ERR_INVALID, "tsgpu_sort_key_create_eval: n_expr must be 1..255 (the dense form keeps expression + 1 in a byte)");
    uint64_t total = 0;
    uint32_t max_id_p1 = 0;
    for (uint32_t e = 0; e < n_expr; e++) {
        if (n_ids[e] && !ids[e]) return fail(TSGPU_ERR_INVALID, "tsgpu_sort_key_create_eval: an id list is NULL");
        total += n_ids[e];
        if (n_ids[e]) {
            if (ids[e][n_ids[e] - 1] == 0xFFFFFFFFu) return fail(TSGPU_ERR_INVALID, "tsgpu_sort_key_create_eval: id out of range");
            max_id_p1 = std::max(max_id_p1, ids[e][n_ids[e] - 1] + 1);          // (ascending: the last id is the largest)
        }
    }
    if (total > 0xFFFFFFFFull) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_sort_key_create_eval: more than 2^32 - 1 ids");
    uint16_t handle;
    long long div;
    uint32_t num_docs;
    {
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        if (ctx->sk_free.empty()) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_sort_key_create_eval: every sort-key handle is live (TSGPU_SORT_KEY_SLOTS)");
        handle = ctx->sk_free.back(); ctx->sk_free.pop_back();                    // (reserved: not live until the upload is done)
        div = ctx->sortkey_dense_div;
        num_docs = ctx->num_docs;
    }
    (void)hipSetDevice(ctx->device);
    const uint32_t dense_len = std::max(num_docs, max_id_p1);
    const bool dense = dense_len != 0 && (div == 1 || (div > 1 && total * (uint64_t)div >= (uint64_t)num_docs));
    // one allocation: [scores: 8 x n_expr | expr_off: 4 x (n_expr + 1) | ids: 4 x total | dense: dense_len bytes]
    const size_t at_off = (size_t)8 * n_expr, at_ids = (at_off + (size_t)4 * (n_expr + 1) + 15) & ~(size_t)15, at_dense = (at_ids + (size_t)4 * total + 15) & ~(size_t)15;
    const size_t bytes = at_dense + (dense ? dense_len : 0) + 16;
    DevBuf buf;
    auto give_back = [&](int rc) {
        if (buf.p) ctx->retire_bin->put(buf);
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        ctx->sk_free.push_back(handle);
        return rc;
    };
    if (hipMalloc(&buf.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        buf.p = nullptr;
        return give_back(fail(TSGPU_ERR_NO_MEMORY, "tsgpu_sort_key_create_eval: device allocation failed"));
    }
    buf.cap = bytes;
    uint8_t* const base = (uint8_t*)buf.p;
    std::vector<uint32_t> expr_off(n_expr + 1, 0u);
    for (uint32_t e = 0; e < n_expr; e++) expr_off[e + 1] = expr_off[e] + n_ids[e];
    hipStream_t s = ctx->sk_stream;
    bool good = hipMemcpyAsync(base, scores, (size_t)8 * n_expr, hipMemcpyHostToDevice, s) == hipSuccess;
    good = good && hipMemcpyAsync(base + at_off, expr_off.data(), (size_t)4 * (n_expr + 1), hipMemcpyHostToDevice, s) == hipSuccess;
    for (uint32_t e = 0; e < n_expr && good; e++)
        if (n_ids[e]) good = hipMemcpyAsync(base + at_ids + (size_t)4 * expr_off[e], ids[e], (size_t)4 * n_ids[e], hipMemcpyHostToDevice, s) == hipSuccess;
    if (dense && good) {
        good = hipMemsetAsync(base + at_dense, 0, dense_len, s) == hipSuccess;
        // LAST expression first, on one stream: where lists overlap the FIRST expression's byte is the one written last (ids are unique within a launch)
        for (uint32_t e = n_expr; e-- > 0 && good;) {
            if (!n_ids[e]) continue;
            const uint32_t blocks = std::min<uint32_t>((n_ids[e] + 255) / 256, 4096u);
            hipLaunchKernelGGL(sort_key_scatter_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t*)(base + at_ids) + expr_off[e], n_ids[e], base + at_dense, dense_len, (uint32_t)(e + 1));
        }
        good = good && hipGetLastError() == hipSuccess;
    }
    SortKeyDesc d;
    memset(&d, 0, sizeof d);                   // (form = SORT_KEY_FORM_EVAL: the slot may have held a vector-query key)
    d.dense = dense ? base + at_dense : nullptr;
    d.ids = (const uint32_t*)(base + at_ids);
    d.expr_off = (const uint32_t*)(base + at_off);
    d.scores = (const int64_t*)base;
    d.dense_len = dense ? dense_len : 0u;
    d.n_expr = n_expr;
    good = good && hipMemcpyAsync(ctx->d_sort_keys.as<SortKeyDesc>() + handle, &d, sizeof d, hipMemcpyHostToDevice, s) == hipSuccess;
    good = good && hipStreamSynchronize(s) == hipSuccess;             // (this stream only: the key is complete before any query can name its handle)
    if (!good) { (void)hipGetLastError(); return give_back(fail(TSGPU_ERR_DEVICE, "tsgpu_sort_key_create_eval: upload failed")); }
    {
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        SortKeyHost& k = ctx->sort_keys[handle];
        k.live = true; k.dense = dense; k.buf = buf; k.n_ids = total; k.n_expr = n_expr;
    }
    ctx->sort_keys_live.fetch_add(1);
    *handle_out = handle;
    return ok();
}

// ---------------------------------------------------------------- `_vector_query` sort keys (TSGPU_SORT_VECTOR_QUERY)
int tsgpu_sort_key_create_vector_query(tsgpu_ctx* ctx, uint32_t vec_field_id, const float* q, float distance_threshold, uint16_t* handle_out) {
    if (!ctx || !q || !handle_out) return fail(TSGPU_ERR_INVALID, "tsgpu_sort_key_create_vector_query: NULL argument");
    (void)hipSetDevice(ctx->device);
    std::lock_guard<std::mutex> mu_lk(ctx->mu);            // the field table and the vector path's stream (the query is staged and normalised there)
    VecSortView fv;
    if (const int rc = vec_sort_view(ctx, vec_field_id, &fv, false)) return rc;
    uint16_t handle;
    {
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        if (ctx->sk_free.empty()) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_sort_key_create_vector_query: every sort-key handle is live (TSGPU_SORT_KEY_SLOTS)");
        handle = ctx->sk_free.back(); ctx->sk_free.pop_back();                    // (reserved: not live until the upload is done)
    }
    DevBuf buf;
    auto give_back = [&](int rc) {
        if (buf.p) ctx->retire_bin->put(buf);
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        ctx->sk_free.push_back(handle);
        return rc;
    };
    const size_t bytes = (size_t)fv.dim * 4 + 16;
    if (hipMalloc(&buf.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        buf.p = nullptr;
        return give_back(fail(TSGPU_ERR_NO_MEMORY, "tsgpu_sort_key_create_vector_query: device allocation failed"));
    }
    buf.cap = bytes;
    hipStream_t s = ctx->sk_stream;
    bool good = vec_sort_stage_query(ctx, vec_field_id, q, (float*)buf.p) == TSGPU_OK;      // (cosine: normalised like the k-NN paths' queries; complete on return)
    // the descriptor names no rows yet (vq_n_rows = 0: every document scores "no row"): the first batch that uses the key fills in the field's state
    SortKeyDesc d;
    memset(&d, 0, sizeof d);
    d.form = SORT_KEY_FORM_VECTOR_QUERY; d.vq_dim = fv.dim; d.vq_q = (const float*)buf.p; d.vq_threshold = distance_threshold; d.vq_ip_lanes = 4;
    good = good && hipMemcpyAsync(ctx->d_sort_keys.as<SortKeyDesc>() + handle, &d, sizeof d, hipMemcpyHostToDevice, s) == hipSuccess;
    good = good && hipStreamSynchronize(s) == hipSuccess;
    if (!good) { (void)hipGetLastError(); return give_back(fail(TSGPU_ERR_DEVICE, "tsgpu_sort_key_create_vector_query: upload failed")); }
    {
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        SortKeyHost& k = ctx->sort_keys[handle];
        k = SortKeyHost();
        k.live = true; k.buf = buf; k.vq = true; k.vq_field = vec_field_id; k.vq_dim = fv.dim; k.vq_threshold = distance_threshold;
    }
    ctx->sort_keys_live.fetch_add(1);
    *handle_out = handle;
    return ok();
}

int tsgpu_sort_key_destroy(tsgpu_ctx* ctx, uint16_t handle) {
    if (!ctx) return fail(TSGPU_ERR_INVALID, "ctx is NULL");
    DevBuf buf;
    {
        std::lock_guard<std::mutex> lk(ctx->sk_mu);
        if (handle >= ctx->sort_keys.size() || !ctx->sort_keys[handle].live) return fail(TSGPU_ERR_NOT_FOUND, "tsgpu_sort_key_destroy: no such sort key");
        SortKeyHost& k = ctx->sort_keys[handle];
        buf = k.buf;
        k = SortKeyHost();
        ctx->sk_free.push_back(handle);
    }
    ctx->sort_keys_live.fetch_sub(1);
    ctx->retire_bin->put(buf);            // no hipFree here: a batch planned before this call may still read the key (freed by tsgpu_commit / tsgpu_destroy)
    return ok();
}

int tsgpu_set_option(tsgpu_ctx* ctx, const char* name, int64_t value) {
    if (!ctx || !name) return fail(TSGPU_ERR_INVALID, "tsgpu_set_option: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!strcmp(name, "kw_max_partials")) {
        if (value < 1 || value > 4096) return fail(TSGPU_ERR_INVALID, "kw_max_partials out of range (1..4096)");
        ctx->kw_max_partials = (uint32_t)value; return ok();
    }
    if (!strcmp(name, "kw_cost_r_x10")) { ctx->kw_cost_r_x10 = (uint32_t)std::max<int64_t>(value, 0); return ok(); }
    if (!strcmp(name, "kw_cost_probe_x100")) { ctx->kw_cost_probe_x100 = (uint32_t)std::max<int64_t>(value, 0); return ok(); }
    if (!strcmp(name, "kw_cost_fixed")) { ctx->kw_cost_fixed = (uint32_t)std::max<int64_t>(value, 0); return ok(); }
    if (!strcmp(name, "kw_sort_work")) { ctx->kw_sort_work = value != 0; return ok(); }
    if (!strcmp(name, "kw_two_kernels")) { ctx->kw_two_kernels = value != 0; return ok(); }
    if (!strcmp(name, "sortkey_dense_div")) {
        if (value < 0 || value > (1ll << 31)) return fail(TSGPU_ERR_INVALID, "sortkey_dense_div out of range (0..2^31)");
        std::lock_guard<std::mutex> sk(ctx->sk_mu);
        ctx->sortkey_dense_div = value; return ok();
    }
    if (!strcmp(name, "kw_device_plan_min_queries")) { ctx->kw_device_plan_min_queries = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 1 << 30); return ok(); }
    if (!strcmp(name, "kw_pair_blocks")) { ctx->kw_pair_blocks = value != 0; return ok(); }
    if (!strcmp(name, "doc_range_lo")) { ctx->doc_range_set = true; ctx->doc_range_lo = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 0xFFFFFFFFll); return ok(); }
    if (!strcmp(name, "doc_range_hi")) { ctx->doc_range_set = true; ctx->doc_range_hi = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 0xFFFFFFFFll); return ok(); }
    if (!strcmp(name, "kw_candidates_rank_fold")) { ctx->kw_candidates_rank_fold = value != 0; return ok(); }
    if (!strcmp(name, "infix_compact_min_slots")) { ctx->infix_compact_min_slots = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 1ll << 31); return ok(); }
    if (!strcmp(name, "infix_timing")) { ctx->infix_timing = value != 0; return ok(); }
    if (!strcmp(name, "infix_test_hold_snapshot")) {      // TESTS ONLY: 1 = infix batches run on the snapshot published NOW until 0 lets it go
        std::atomic_store(&ctx->infix_test_snap, value != 0 ? ctx->snapshot() : std::shared_ptr<const Snapshot>());
        return ok();
    }
    if (!strcmp(name, "phrase_round_max_bytes")) { ctx->phrase_round_max_bytes = (uint64_t)std::min<int64_t>(std::max<int64_t>(value, 1), 1ll << 36); return ok(); }
    if (!strcmp(name, "phrase_weight_cut")) { ctx->phrase_weight_cut = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 1ll << 24); return ok(); }      // TESTS ONLY
    if (!strcmp(name, "phrase_timing")) { ctx->phrase_timing = value != 0; return ok(); }
    if (!strcmp(name, "infix_round_max_bytes")) { ctx->infix_round_max_bytes = (uint64_t)std::min<int64_t>(std::max<int64_t>(value, 1), 1ll << 36); return ok(); }
    if (!strcmp(name, "kw_mf_pipelined")) { ctx->kw_mf_pipelined = value != 0; return ok(); }
    if (!strcmp(name, "kw_count_touched")) { ctx->kw_count_touched = value != 0; return ok(); }
    if (!strcmp(name, "kw_plan_digest")) { ctx->kw_plan_digest = value != 0; return ok(); }
    if (!strcmp(name, "kw_find_dir_tile")) { ctx->kw_find_dir_tile = value != 0; return ok(); }
    if (!strcmp(name, "kw_find_dir_span_pct")) { ctx->kw_find_dir_span_pct = std::min<int64_t>(std::max<int64_t>(value, 1), 1 << 20); return ok(); }
    if (!strcmp(name, "kw_iddir_min_ids")) { ctx->kw_iddir_min_ids = value < 0 ? 0 : value; ctx->commit_force_full = true; return ok(); }
    if (!strcmp(name, "kw_iddir_density_div")) { ctx->kw_iddir_density_div = value < 1 ? 1 : value; ctx->commit_force_full = true; return ok(); }
    if (!strcmp(name, "kw_iddir_budget_mb")) { ctx->kw_iddir_budget_mb = value < 0 ? 0 : value; ctx->commit_force_full = true; return ok(); }
    if (!strcmp(name, "kw_host_split_tail_slices")) { ctx->kw_host_split_tail_slices = value >= 2 ? 2 : 1; return ok(); }
    if (!strcmp(name, "kw_host_split_device_plan")) { ctx->kw_host_split_device_plan = value != 0; return ok(); }
    if (!strcmp(name, "kw_host_split_first_pct")) { ctx->kw_host_split_first_pct = (uint32_t)std::min<int64_t>(95, std::max<int64_t>(5, value)); return ok(); }
    if (!strcmp(name, "kw_host_split_queries")) { ctx->kw_host_split_queries = (uint32_t)std::max<int64_t>(0, value); return ok(); }
    if (!strcmp(name, "kw_zero_copy_max_queries")) { ctx->kw_zero_copy_max_queries = (uint32_t)std::max<int64_t>(0, value); return ok(); }
    if (!strcmp(name, "kw_timing_min_queries")) { ctx->kw_timing_min_queries = (uint32_t)std::max<int64_t>(0, value); return ok(); }
    if (!strcmp(name, "kw_merge_select_min")) { ctx->kw_merge_select_min = (uint32_t)std::max<int64_t>(0, value); return ok(); }
    if (!strcmp(name, "hnsw_visited_hash")) { ctx->hnsw_visited_hash = value != 0; return ok(); }
    if (!strcmp(name, "hnsw_test_tiny_cand")) { ctx->hnsw_test_tiny_cand = value != 0; return ok(); }
    if (!strcmp(name, "hnsw_test_slots")) { ctx->hnsw_test_slots = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 4096); return ok(); }
    if (!strcmp(name, "hnsw_test_max_maps")) { ctx->hnsw_test_max_maps = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 1 << 20); return ok(); }
    if (!strcmp(name, "hnsw_test_epoch")) { ctx->hnsw_test_epoch = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 0xFFFF); return ok(); }
    if (!strcmp(name, "hnsw_visited_max_gib")) { ctx->hnsw_visited_max_gib = (int)std::min<int64_t>(std::max<int64_t>(1, value), 128); return ok(); }
    if (!strcmp(name, "blocking_sync_min_callers")) { ctx->blocking_sync_min_callers = (int)std::max<int64_t>(0, value); return ok(); }
    if (!strcmp(name, "plan_threads")) { if (value < 1 || value > 64) return fail(TSGPU_ERR_INVALID, "plan_threads: 1..64"); ctx->plan_threads = (int)value; return ok(); }
    if (!strcmp(name, "plan_parallel_min_queries")) { if (value < 0) return fail(TSGPU_ERR_INVALID, "plan_parallel_min_queries >= 0"); ctx->plan_parallel_min_queries = (uint32_t)value; return ok(); }
    if (!strcmp(name, "fuse_threads")) { if (value < 1 || value > 256) return fail(TSGPU_ERR_INVALID, "fuse_threads: 1..256"); ctx->fuse_threads = (int)value; return ok(); }
    if (!strcmp(name, "kw_hit_buffer_records")) {       // exact budget in hit records (tests); 0 = use kw_hit_buffer_mb
        if (value < 0) return fail(TSGPU_ERR_INVALID, "kw_hit_buffer_records must be >= 0");
        ctx->kw_hit_buffer_records = (uint64_t)value; return ok();
    }
    if (!strcmp(name, "kw_hit_buffer_mb")) {
        if (value < 1) return fail(TSGPU_ERR_INVALID, "kw_hit_buffer_mb must be >= 1");
        ctx->kw_hit_buffer_mb = (uint32_t)value; return ok();
    }
    if (!strcmp(name, "kw_chunk_blocks")) {
        if (value < 0 || value > KW_MAX_CHUNK) return fail(TSGPU_ERR_INVALID, "kw_chunk_blocks out of range (0 = auto, 1..KW_MAX_CHUNK)");
        ctx->kw_chunk_blocks = (uint32_t)value;
        return ok();
    }
    if (!strcmp(name, "vec_rows_per_slab")) {
        if (value != 0 && (value < 128 || value > (1 << 24))) return fail(TSGPU_ERR_INVALID, "vec_rows_per_slab out of range");
        ctx->vec_rows_per_slab = (uint32_t)value;
        return ok();
    }
    if (!strcmp(name, "vec_sample_tiles")) {
        if (value < 0 || value > (1 << 20)) return fail(TSGPU_ERR_INVALID, "vec_sample_tiles out of range");
        ctx->vec_sample_tiles = (uint32_t)value;
        return ok();
    }
    if (!strcmp(name, "vec_cand_cap")) {
        if (value < 0 || value > (1 << 24)) return fail(TSGPU_ERR_INVALID, "vec_cand_cap out of range");
        ctx->vec_cand_cap = (uint32_t)value;
        return ok();
    }
    if (!strcmp(name, "vec_count_rescored")) { ctx->vec_count_rescored = value != 0; return ok(); }
    if (!strcmp(name, "vec_filter_direct_max")) {
        if (value < 0 || value > 65536) return fail(TSGPU_ERR_INVALID, "vec_filter_direct_max out of range (0..65536)");
        ctx->vec_filter_direct_max = (uint32_t)value;
        return ok();
    }
    if (!strcmp(name, "vec_flat_group_max_bytes")) {    // cap of the ragged distance array one launch fills (tsgpu_vector_search_batch_per_query); only lowered (tests: the split at a small shape)
        if (value < 4 || value > (1ll << 30)) return fail(TSGPU_ERR_INVALID, "vec_flat_group_max_bytes out of range (4 .. 1 GiB)");
        ctx->vec_flat_group_max_bytes = (uint64_t)value;
        return ok();
    }
    // micro-batcher (tsgpu_batcher.h): concurrent small calls are coalesced into one launch
    if (!strcmp(name, "index_min_slack_words")) { ctx->index_min_slack_words = (uint64_t)std::max<int64_t>(value, 0); return ok(); }   // (tests: small arenas)
    if (!strcmp(name, "index_compact_min_words")) { ctx->index_compact_min_words = (uint64_t)std::max<int64_t>(value, 0); return ok(); }   // (tests: small arenas)
    if (!strcmp(name, "commit_full")) { ctx->commit_force_full = value != 0; return ok(); }      // the NEXT commit re-packs every list (compaction)
    if (!strcmp(name, "kw_lanes")) {                   // execution lanes (stream + scratch each) that concurrent keyword batches spread over
        if (value < 1 || value > tsgpu_ctx::N_LANES) return fail(TSGPU_ERR_INVALID, "kw_lanes out of range (1..8)");
        ctx->n_lanes = (int)value; return ok();
    }
    if (!strcmp(name, "facet_ids_per_block")) {        // result ids per workgroup of the facet counting launch; 0 = chosen per batch (tests: the multi-round walk on small inputs)
        if (value < 0 || value > 4096 || (value % 256) != 0) return fail(TSGPU_ERR_INVALID, "facet_ids_per_block must be 0 or a multiple of 256 up to 4096");
        ctx->facet_ids_per_block = (uint32_t)value; return ok();
    }
    if (!strcmp(name, "hybrid_overlap")) { ctx->hybrid_overlap = value != 0; return ok(); }
    if (!strcmp(name, "vec_batch_post_window_us")) { ctx->vec_batch_post_window_us = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 100000); return ok(); }
    if (!strcmp(name, "batch_window_us")) { ctx->batch_window_us = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 100000); return ok(); }
    if (!strcmp(name, "batch_max_queries")) { ctx->batch_max_queries = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 1 << 20); return ok(); }   // 0 = never coalesce
    if (!strcmp(name, "batch_round_queries")) { ctx->batch_round_queries = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 1 << 20); return ok(); }
    if (!strcmp(name, "vec_ip_lanes")) {               // summation order of every exact distance = the SIMD level hnswlib is compiled for in the server
        if (value != 4 && value != 8 && value != 16) return fail(TSGPU_ERR_INVALID, "vec_ip_lanes must be 4 (SSE, stock build), 8 (AVX) or 16 (AVX-512)");
        ctx->vec_ip_lanes = (uint32_t)value;
        return ok();
    }
    if (!strcmp(name, "vec_prefilter")) {
        if (value < 0 || value > 1) return fail(TSGPU_ERR_INVALID, "vec_prefilter must be 0 (fp32 MFMA scan) or 1 (bf16 bracket scan)");
        ctx->vec_prefilter = (uint32_t)value;
        return ok();
    }
    return fail(TSGPU_ERR_NOT_FOUND, std::string("tsgpu_set_option: unknown option ") + name);
}

int tsgpu_get_counter(tsgpu_ctx* ctx, const char* name, uint64_t* out) {
    if (!ctx || !name || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_get_counter: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->tm_mu);
    if (!strcmp(name, "kw_last_hit_groups")) { *out = ctx->kw_last_hit_groups; return ok(); }      // last keyword batch: find+score groups (0 = fused kernel)
    if (!strcmp(name, "kw_candidates_rank_launches")) { *out = ctx->kw_candidates_rank_launches; return ok(); }
    // infix search (tsgpu_infix_search_batch, cumulative): vocabulary passes, live tokens they tested, tokens that matched (summed over the queries), posting lists united, rounds
    if (!strcmp(name, "infix_scan_launches")) { *out = ctx->infix_scan_launches.load(); return ok(); }
    if (!strcmp(name, "infix_tokens_scanned")) { *out = ctx->infix_tokens_scanned.load(); return ok(); }
    if (!strcmp(name, "infix_tokens_matched")) { *out = ctx->infix_tokens_matched.load(); return ok(); }
    if (!strcmp(name, "infix_lists_marked")) { *out = ctx->infix_lists_marked.load(); return ok(); }
    if (!strcmp(name, "infix_rounds")) { *out = ctx->infix_rounds.load(); return ok(); }
    if (!strcmp(name, "infix_tile_tokens")) { *out = INFIX_TILE_TOKENS; return ok(); }            // the scan kernel's tile: vocabulary slots per workgroup ...
    if (!strcmp(name, "infix_tile_bytes")) { *out = INFIX_TILE_BYTES; return ok(); }              // ... and token bytes staged in LDS at a time
    if (!strcmp(name, "infix_compactions")) { *out = ctx->infix_compactions.load(); return ok(); }       // (written by tsgpu_commit)
    if (!strcmp(name, "infix_commit_uploaded_bytes")) { *out = ctx->infix_commit_uploaded_bytes.load(); return ok(); }
    // under option "infix_timing" (cumulative, us of host wall clock with a stream sync behind each phase): vocabulary scans incl. the match lists' way back; union marks; exclusion, filter, count and expansion; ranking
    if (!strcmp(name, "infix_scan_us")) { *out = ctx->infix_scan_us.load(); return ok(); }
    if (!strcmp(name, "infix_mark_us")) { *out = ctx->infix_mark_us.load(); return ok(); }
    if (!strcmp(name, "infix_expand_us")) { *out = ctx->infix_expand_us.load(); return ok(); }
    if (!strcmp(name, "infix_rank_us")) { *out = ctx->infix_rank_us.load(); return ok(); }
    // phrase search (tsgpu_phrase_search_batch, cumulative): (query, field, phrase) items planned, hit records the adjacency kernel checked / matched, rounds, stream syncs of the front
    if (!strcmp(name, "phrase_items")) { *out = ctx->phrase_items.load(); return ok(); }
    if (!strcmp(name, "phrase_records_checked")) { *out = ctx->phrase_records_checked.load(); return ok(); }
    if (!strcmp(name, "phrase_records_matched")) { *out = ctx->phrase_records_matched.load(); return ok(); }
    if (!strcmp(name, "phrase_rounds")) { *out = ctx->phrase_rounds.load(); return ok(); }
    if (!strcmp(name, "phrase_syncs")) { *out = ctx->phrase_syncs.load(); return ok(); }
    // under option "phrase_timing" (cumulative, us of host wall clock with a stream sync behind each phase): intersections + adjacency marks; fold, field OR, exclusion, filter, expansion, scores; ranking
    if (!strcmp(name, "phrase_mark_us")) { *out = ctx->phrase_mark_us.load(); return ok(); }
    if (!strcmp(name, "phrase_fold_us")) { *out = ctx->phrase_fold_us.load(); return ok(); }
    if (!strcmp(name, "phrase_rank_us")) { *out = ctx->phrase_rank_us.load(); return ok(); }
    if (!strcmp(name, "kw_mf_pipelined_launches")) { *out = ctx->kw_mf_pipelined_launches; return ok(); }     // find launches served by kw_find_mf2_kernel
    if (!strcmp(name, "kw_last_hit_records")) { *out = ctx->kw_last_hit_records; return ok(); }    // hit-record capacity the last batch asked for
    if (!strcmp(name, "vec_overflow_rounds")) { *out = ctx->vec_overflow_rounds; return ok(); }
    if (!strcmp(name, "vec_prefilter_fallbacks")) { *out = ctx->vec_prefilter_fallbacks; return ok(); }
    if (!strcmp(name, "vec_prefilter_groups")) { *out = ctx->vec_prefilter_groups; return ok(); }
    if (!strcmp(name, "vec_filter_direct_queries")) { *out = ctx->vec_filter_direct_queries; return ok(); }
    if (!strcmp(name, "vec_filter_scan_queries")) { *out = ctx->vec_filter_scan_queries; return ok(); }
    if (!strcmp(name, "vec_search_pq_flat_queries")) { *out = ctx->vec_search_pq_flat_queries.load(); return ok(); }     // tsgpu_vector_search_batch_per_query, cumulative
    if (!strcmp(name, "vec_search_pq_kcut_queries")) { *out = ctx->vec_search_pq_kcut_queries.load(); return ok(); }
    if (!strcmp(name, "vec_search_pq_flat_lists")) { *out = ctx->vec_search_pq_flat_lists.load(); return ok(); }         // distinct flat lists uploaded
    if (!strcmp(name, "vec_grouped_flat_queries")) { *out = ctx->vec_grouped_flat_queries.load(); return ok(); }       // tsgpu_vector_search_grouped_batch
    if (!strcmp(name, "vec_grouped_kcut_queries")) { *out = ctx->vec_grouped_kcut_queries.load(); return ok(); }
    if (!strcmp(name, "vec_grouped_items")) { *out = ctx->vec_grouped_items.load(); return ok(); }
    if (!strcmp(name, "vec_grouped_syncs")) { *out = ctx->vec_grouped_syncs.load(); return ok(); }
    if (!strcmp(name, "vec_grouped_sync_us")) { *out = ctx->vec_grouped_sync_us.load(); return ok(); }
    if (!strcmp(name, "vec_search_pq_flat_launches")) { *out = ctx->vec_search_pq_flat_launches.load(); return ok(); }   // launches of vec_flat_ragged_distances_kernel
    if (!strcmp(name, "vec_filter_h2d_bytes")) { *out = ctx->vec_filter_h2d_bytes; return ok(); }
    if (!strcmp(name, "vec_filter_stage_us")) { *out = ctx->vec_filter_stage_us; return ok(); }
    if (!strcmp(name, "vec_filter_build_us")) { *out = ctx->vec_filter_build_us; return ok(); }
    if (!strcmp(name, "vec_rescored_rows")) { *out = ctx->vec_rescored_rows; return ok(); }
    if (!strcmp(name, "vec_candidate_rows")) { *out = ctx->vec_candidate_rows; return ok(); }
    if (!strcmp(name, "hnsw_last_expansions")) { *out = ctx->hnsw_last_expansions; return ok(); }
    if (!strcmp(name, "hnsw_tier_reruns")) { *out = ctx->hnsw_tier_reruns; return ok(); }
    if (!strcmp(name, "hnsw_launches")) { *out = ctx->hnsw_launches; return ok(); }
    if (!strcmp(name, "hnsw_filter_maps")) { *out = ctx->hnsw_filter_maps; return ok(); }
    if (!strcmp(name, "hnsw_batch_rounds")) { *out = ctx->hnsw_comb.rounds; return ok(); }                       // coalesced HNSW rounds (not part of batch_rounds)
    if (!strcmp(name, "hnsw_batch_coalesced_calls")) { *out = ctx->hnsw_comb.coalesced_calls; return ok(); }     // calls served by those rounds
    if (!strcmp(name, "hnsw_last_distances")) { *out = ctx->hnsw_last_distances; return ok(); }
    if (!strcmp(name, "commit_last_us")) { *out = ctx->commit_last_us; return ok(); }                        // the last tsgpu_commit: wall time, bytes uploaded
    if (!strcmp(name, "commit_last_uploaded_bytes")) { *out = ctx->commit_last_uploaded_bytes; return ok(); }
    if (!strcmp(name, "commit_failed_count")) { *out = ctx->commit_failed_count; return ok(); }
    if (!strcmp(name, "commit_compactions")) { *out = ctx->commit_compactions; return ok(); }             // full commits taken because garbage outweighed the live words
    if (!strcmp(name, "index_live_words")) { const auto sn = ctx->snapshot(); *out = sn && sn->ar ? sn->ar->live_idw + sn->ar->live_pw : 0; return ok(); }
    if (!strcmp(name, "index_used_words")) { const auto sn = ctx->snapshot(); *out = sn && sn->ar ? sn->ar->used_idw + sn->ar->used_pw : 0; return ok(); }
    if (!strcmp(name, "commit_full_count")) { *out = ctx->commit_full_count; return ok(); }                  // commits that re-packed everything / appended at the tails
    if (!strcmp(name, "commit_incremental_count")) { *out = ctx->commit_incremental_count; return ok(); }
    if (!strcmp(name, "kw_batches")) { *out = ctx->kw_batches.load(); return ok(); }                 // host-side phase totals (us) over all keyword batches
    if (!strcmp(name, "kw_plan_us")) { *out = ctx->kw_plan_us.load(); return ok(); }
    if (!strcmp(name, "kw_max_plan_us")) { *out = ctx->kw_max_plan_us.exchange(0); return ok(); }       // (reading resets the maxima)
    if (!strcmp(name, "kw_max_upload_us")) { *out = ctx->kw_max_upload_us.exchange(0); return ok(); }
    if (!strcmp(name, "kw_max_launch_us")) { *out = ctx->kw_max_launch_us.exchange(0); return ok(); }
    if (!strcmp(name, "kw_max_wait_us")) { *out = ctx->kw_max_wait_us.exchange(0); return ok(); }
    if (!strcmp(name, "kw_queue_us")) { *out = ctx->kw_queue_us.load(); return ok(); }
    if (!strcmp(name, "kw_wake_us")) { *out = ctx->kw_wake_us.load(); return ok(); }
    if (!strcmp(name, "kw_max_queue_us")) { *out = ctx->kw_max_queue_us.exchange(0); return ok(); }     // parked -> its round starts executing
    if (!strcmp(name, "kw_max_wake_us")) { *out = ctx->kw_max_wake_us.exchange(0); return ok(); }       // results ready -> the caller runs again
    if (!strcmp(name, "kw_upload_us")) { *out = ctx->kw_upload_us.load(); return ok(); }
    if (!strcmp(name, "kw_launch_us")) { *out = ctx->kw_launch_us.load(); return ok(); }
    if (!strcmp(name, "kw_wait_us")) { *out = ctx->kw_wait_us.load(); return ok(); }
    if (!strcmp(name, "kw_book_us")) { *out = ctx->kw_book_us.load(); return ok(); }
    if (!strcmp(name, "kw_device_plans")) { *out = ctx->kw_device_plans.load(); return ok(); }                     // batches planned on the device / sent back to the host planner
    if (!strcmp(name, "kw_device_plan_fallbacks")) { *out = ctx->kw_device_plan_fallbacks.load(); return ok(); }
    if (!strcmp(name, "kw_last_plan_cut_digest")) { *out = ctx->kw_last_plan_cut_digest; return ok(); }                 // the last keyword batch run under option kw_plan_digest (kw_plan_digest.h)
    if (!strcmp(name, "kw_last_plan_layout_digest")) { *out = ctx->kw_last_plan_layout_digest; return ok(); }
    if (!strcmp(name, "sort_keys_live")) { *out = ctx->sort_keys_live.load(); return ok(); }                         // tsgpu_sort_key_create_eval minus _destroy
    // the last keyword batch run under option kw_count_touched: work items that took the find kernel's directory mode, pairs of driver blocks searched,
    // of them through a directory tile, and pairs of directory-mode items too wide for the tile (probed per candidate)
    if (!strcmp(name, "kw_find_dir_items")) { *out = ctx->kw_find_dir_items; return ok(); }
    if (!strcmp(name, "kw_find_pairs")) { *out = ctx->kw_find_pairs; return ok(); }
    if (!strcmp(name, "kw_find_dir_pairs")) { *out = ctx->kw_find_dir_pairs; return ok(); }
    if (!strcmp(name, "kw_find_dir_wide_pairs")) { *out = ctx->kw_find_dir_wide_pairs; return ok(); }
    if (!strcmp(name, "kw_iddir_split_entries")) { *out = ctx->kw_iddir_split_entries; return ok(); }               // IDDIR_SPLIT entries those builds wrote
    if (!strcmp(name, "kw_iddir_built")) { *out = ctx->kw_iddir_built; return ok(); }                               // id directories (re)built by commits so far
    if (!strcmp(name, "kw_iddir_lists")) { const auto sn = ctx->snapshot(); uint64_t n = 0; if (sn) for (const auto& r : sn->dir_of) n += r ? 1 : 0; *out = n; return ok(); }   // lists of the current snapshot that carry one
    if (!strcmp(name, "batch_exec_us")) { *out = ctx->batch_exec_us.load(); return ok(); }           // coalesced rounds: batch execution / hand-out to the callers
    if (!strcmp(name, "batch_scatter_us")) { *out = ctx->batch_scatter_us.load(); return ok(); }
    if (!strcmp(name, "batch_rounds")) { *out = ctx->kw_comb.rounds + ctx->vec_comb.rounds; return ok(); }               // coalesced rounds executed so far
    if (!strcmp(name, "gb_batch_rounds")) { *out = ctx->gb_comb.rounds; return ok(); }                                          // ... of grouped keyword calls
    if (!strcmp(name, "gb_batch_coalesced_calls")) { *out = ctx->gb_comb.coalesced_calls; return ok(); }
    if (!strcmp(name, "batch_coalesced_calls")) { *out = ctx->kw_comb.coalesced_calls + ctx->vec_comb.coalesced_calls; return ok(); }   // calls served by those rounds
    return fail(TSGPU_ERR_NOT_FOUND, std::string("tsgpu_get_counter: unknown counter ") + name);
}

int tsgpu_keep_result_ids(tsgpu_ctx* ctx, int keep) {
    if (!ctx) return fail(TSGPU_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->keep_ids = keep != 0;
    return ok();
}

// ---------------------------------------------------------------- keyword search (seam B1)
namespace {
struct Plan {
    std::vector<KwQueryDev> q;
    std::vector<KwWorkItem> work;                         // ONE work table, five kernel tables back to back: single-field TMAX 3 / TMAX 10, multi-field TMAX 3 / TMAX 10, wildcard scans
    size_t n_tab[5] = {0, 0, 0, 0, 0};                    // ... and their sizes
    std::vector<KwQueryMF> mf;
    std::vector<KwMergeGroup> groups;                     // first level of the two-level merge (queries with many work items)
    std::vector<uint32_t> ordered_count_q;                // multi-field queries with filter AND excluded ids (kw_mf_ordered_count_kernel)
    uint64_t fbits_words = 0;                             // rank bitmaps of the filtered multi-field queries
    bool any_deadline = false;                            // some query carries a deadline: stamp the batch start, collect cutoff flags
    bool any_s2 = false;              // some query has a third sort key
    bool any_vq = false;              // some query has a TSGPU_SORT_VECTOR_QUERY slot: the launches take the kernels' VQ instantiations (kw_vq_sort.hip.h)
    bool any_aux = false;             // some query has filter ids, excluded ids or a sort slot of kind >= TSGPU_SORT_EVAL (else the score kernel's PLAIN instantiation serves the batch)
    bool any_array = false;           // some multi-field query has a string[] field
    uint32_t mf_max_fields = 0;       // most query_by fields of any multi-field query (<= 2: the pipelined find kernel, kw_find_mf2.hip.h)
    std::vector<uint32_t> aux;
    std::vector<int32_t> status, cutoff;
    uint32_t max_k = 1;
    uint64_t ids_total = 0;
    uint64_t list_bytes = 0;       // 4 * sum |L_t| over the batch
};
}

static uint32_t resolve_topster_size(const tsgpu_ctx* ctx, const tsgpu_kw_query& in) {
    uint32_t k = in.topster_size;
    if (k == 0) {                                                      // src/index.cpp:3506-3512
        k = TSGPU_DEFAULT_TOPSTER_SIZE;
        k = in.n_filter ? std::min<uint32_t>(k, in.n_filter) : std::min<uint32_t>(k, std::max<uint32_t>(ctx->num_docs, 1));
    } else k = std::min<uint32_t>(k, std::max<uint32_t>(ctx->num_docs, 1));
    return std::max<uint32_t>(k, 1);
}

// ---- the host planner: plan_batch() below runs these phases in order ----
namespace {
// cuts a list of n_blocks driver blocks into work items of `chunk` blocks and registers them as the next items of one query (query_word: its index, with
// the driver field of a multi-field query in the top bits); ids_base: where the list's id segment starts inside the query's
void emit_items(std::vector<KwWorkItem>& work, uint32_t& q_begin, uint32_t& q_cnt, uint32_t query_word, uint32_t n_blocks, uint32_t chunk, uint32_t ids_base) {
    for (uint32_t b = 0; b < n_blocks; b += chunk) {
        if (q_cnt++ == 0) q_begin = (uint32_t)work.size();
        work.push_back({query_word, b, std::min(n_blocks, b + chunk), ids_base + b * BLOCK_IDS});
    }
}

// The slices [bound(k), bound(k + 1)) a batch's queries are planned in, on n_thr threads: this one and the context's parked host threads. for_query_slices
// hands them out dynamically (four per thread is the callers' choice: a parked thread that wakes late still finds work, the caller never idles).
struct QuerySlices {
    uint32_t n_queries, n_thr, n_parts;
    uint32_t bound(uint32_t k) const { return (uint32_t)((uint64_t)n_queries * k / n_parts); }
};
void for_query_slices(tsgpu_ctx* ctx, const QuerySlices& sl, const std::function<void(uint32_t, uint32_t, uint32_t)>& fn) {
    if (sl.n_thr <= 1) { for (uint32_t k = 0; k < sl.n_parts; k++) fn(k, sl.bound(k), sl.bound(k + 1)); return; }
    std::atomic<uint32_t> next{0};
    std::atomic<int> oom{0};
    const std::function<void()> job = [&]() {
        try { for (;;) { const uint32_t k = next.fetch_add(1); if (k >= sl.n_parts) break; fn(k, sl.bound(k), sl.bound(k + 1)); } } catch (const std::bad_alloc&) { oom = 1; }
    };
    ctx->host_pool.run(job, (int)sl.n_thr - 1);
    if (oom) throw std::bad_alloc();
}

// The per-query part of the plan (handles, work items, id arenas) is independent per query: big batches are planned in slices, every slice into its own
// accumulator; the slices are then concatenated in query order and the offsets a query holds into the shared arenas shifted by its slice's base
// (0.5 ms -> 0.1 ms of a 9 ms step at 10 000 queries).
struct PlanAcc {
    std::vector<uint32_t> aux, ordered_count_q; std::vector<KwQueryMF> mf; std::vector<KwWorkItem> flat_work;
    uint64_t fbits_words = 0, ids_total = 0, list_bytes = 0;
    uint32_t max_k = 0;
    bool any_deadline = false, any_s2 = false, any_aux = false, any_array = false, any_vq = false;
    uint32_t mf_max_fields = 0;
};
// what the cut needs of a translated query: every token is resolved ONCE, by translate(); the batch chunk is known only after all of them
struct QueryCut {
    enum Shape : uint8_t { NONE, WILDCARD, MULTI_FIELD, SINGLE_FIELD } shape = NONE;
    uint32_t driver_blocks = 0;                   // wildcard: blocks of ids to scan; single field: the driver list's
    uint32_t n_lists = 0, len_driver = 0, len_second = 0;      // single field: what the launch-order cost reads
    uint32_t chunk_blocks = 0;                    // what the query adds to the batch chunk's input (kw_policy_batch_chunk)
};
struct QueryTokens { uint32_t nl = 0; uint32_t len_of[KW_MAX_TOKENS]; KwQueryMF mfq; };

struct BatchPlanner {
    tsgpu_ctx* ctx; const Snapshot& snap; const tsgpu_kw_query* queries; uint32_t n_queries; Plan& P; bool keep_ids, wildcard; const KwVFlat* vflat; const uint16_t* present_elsewhere;
    uint64_t now;
    std::vector<QueryCut> cut; std::vector<uint32_t> q_begin, q_cnt; std::vector<double> item_cost;
    std::vector<KwWorkItem> flat_work;                       // every query's items, contiguous, in query order
    const uint64_t* wild_ids_dev = nullptr;                  // wildcard batch of the infix front: per query the DEVICE address of its n_filter filter ids (0: host ids as usual)
    const uint64_t* wild_tm_dev = nullptr;                   // ... of the phrase front: beside it, the DEVICE address of the ids' text-match values (KwQueryDev::wild_tm)

    // one or_iterator per token that exists in some field (kw_translate.h), in query order; returns the bytes of its lists
    uint64_t add_token(uint32_t i, QueryTokens& T, const KwTokenLists& tl, uint32_t len) {
        P.q[i].list[T.nl] = tl.first;
        for (uint32_t f = 0; f < (uint32_t)KW_MAX_FIELDS; f++) if (tl.handle[f] != KW_NONE) T.mfq.list[T.nl][f] = tl.handle[f];
        T.len_of[T.nl++] = len;
        return 4ull * tl.ids;
    }

    // Index::search_wildcard (src/index.cpp:6616-6818): rank every filter id (every seq_id without a filter) by its sort keys
    void wildcard_query(uint32_t i, uint32_t lo, uint32_t k, uint64_t sort_bytes_per_id, PlanAcc& A) {
        const tsgpu_kw_query& in = queries[i];
        KwQueryDev& q = P.q[i];
        q.mf_index = KW_NONE;
        kw_fill_sort_slots(in, q);
        q.k = k;
        A.max_k = std::max(A.max_k, k);
        q.n_excl = in.n_excluded;
        q.n_filt = in.n_filter;
        if (vflat) {
            // flat vector branch: query i ranks ITS row of the distance matrix (aligned with the filter ids) — or its segment of a ragged array, with its
            // own threshold; neighbouring queries that pass the same host array share one upload of it per planning slice (the per-query entry point
            // orders its flat queries by list)
            if (in.n_excluded || !in.n_filter) { P.status[i] = TSGPU_ERR_INVALID; return; }
            q.vdist = (uint64_t)(uintptr_t)(vflat->dist_dev + (vflat->off ? (size_t)vflat->off[i] : (size_t)i * vflat->stride));
            q.vdist_thr = vflat->thr ? vflat->thr[i] : vflat->threshold; q.vdist_abs = vflat->abs ? 1 : 0;
        }
        if (vflat && i > lo && P.status[i - 1] == TSGPU_OK && queries[i - 1].filter_ids == in.filter_ids && queries[i - 1].n_filter == in.n_filter) q.aux_off = P.q[i - 1].aux_off;
        else {
            q.aux_off = (uint32_t)A.aux.size();
            if (in.n_excluded) {
                if (!in.excluded_ids) { P.status[i] = TSGPU_ERR_INVALID; return; }
                A.aux.insert(A.aux.end(), in.excluded_ids, in.excluded_ids + in.n_excluded);
            }
            if (wild_ids_dev && wild_ids_dev[i]) { q.wild_ids = wild_ids_dev[i]; if (wild_tm_dev) q.wild_tm = wild_tm_dev[i]; }      // (in.filter_ids is not a host address then)
            else if (in.n_filter) A.aux.insert(A.aux.end(), in.filter_ids, in.filter_ids + in.n_filter);
        }
        uint32_t n_ids = in.n_filter ? in.n_filter : ctx->num_docs;
        if (!vflat && ctx->doc_range_set) {
            // a doc-range shard ranks the ids it OWNS: the filter ids inside [lo, hi) (a sub-array: they ascend), or lo .. hi - 1
            const uint32_t lo_id = ctx->doc_range_lo, hi_id = std::min(ctx->doc_range_hi, ctx->num_docs);
            if (in.n_filter) {
                const uint32_t* fb = in.filter_ids;
                const uint32_t a = (uint32_t)(std::lower_bound(fb, fb + in.n_filter, lo_id) - fb), b = (uint32_t)(std::lower_bound(fb, fb + in.n_filter, hi_id) - fb);
                A.aux.resize(A.aux.size() - in.n_filter);                       // (the filter ids were appended last: keep the sub-array)
                A.aux.insert(A.aux.end(), fb + a, fb + b);
                q.n_filt = b - a;
                n_ids = b - a;
            } else { n_ids = hi_id > lo_id ? hi_id - lo_id : 0; q.wild_base = lo_id; }
        }
        q.wild_n_ids = n_ids;
        if (n_ids == 0) return;                                                 // (nothing of this query on this shard: zero hits, status 0)
        A.list_bytes += 4ull * in.n_filter + sort_bytes_per_id * n_ids;      // the id array + one column value (a key byte, the key's lists) per id and key slot
        q.ids_out_off = A.ids_total;
        cut[i].shape = QueryCut::WILDCARD;
        cut[i].driver_blocks = (n_ids + BLOCK_IDS - 1) / BLOCK_IDS;
        if (keep_ids) A.ids_total += (uint64_t)cut[i].driver_blocks * BLOCK_IDS;
    }

    // several query_by fields, a string[] field or dropped tokens: driver = the token with the fewest postings over all fields, one group of work items
    // per field list of it
    void multi_field_query(uint32_t i, uint32_t k, bool ordered_count, QueryTokens& T, PlanAcc& A) {
        const tsgpu_kw_query& in = queries[i];
        KwQueryDev& q = P.q[i];
        KwQueryMF& mfq = T.mfq;
        uint32_t td = 0;
        for (uint32_t t = 1; t < q.n_required; t++) if (T.len_of[t] < T.len_of[td]) td = t;
        A.mf_max_fields = std::max(A.mf_max_fields, (uint32_t)in.n_fields);
        mfq.driver_token = td;
        mfq.second_token = KW_NONE;             // the required token with the next fewest postings: merged block-wise by the find kernel
        for (uint32_t t = 0; t < q.n_required; t++) if (t != td && (mfq.second_token == KW_NONE || T.len_of[t] < T.len_of[mfq.second_token])) mfq.second_token = t;
        (void)kw_fill_fields(snap, in, mfq, &A.any_array);      // (the fields exist: translate() checked)
        if (k + KW_THREADS > 1024) { P.status[i] = TSGPU_ERR_UNSUPPORTED; return; }      // topster_size with several query_by fields
        q.mf_index = (uint32_t)A.mf.size();
        A.mf.push_back(mfq);
        if (ordered_count) A.ordered_count_q.push_back(i);
        if (in.n_filter) { q.fbits_off = A.fbits_words; A.fbits_words += ((uint64_t)in.n_filter + 31) / 32; }
        q.ids_out_off = A.ids_total;
        cut[i].shape = QueryCut::MULTI_FIELD;
        for (uint32_t f = 0; f < in.n_fields && keep_ids; f++)      // the fields' id segments, one behind the other
            if (mfq.list[td][f] != KW_NONE) A.ids_total += (uint64_t)snap.h_lists[mfq.list[td][f]].n_blocks * BLOCK_IDS;
    }

    // one plain string field: the block-merge kernels; probe order = ascending list length, stable
    void single_field_query(uint32_t i, const QueryTokens& T, PlanAcc& A) {
        KwQueryDev& q = P.q[i];
        uint8_t ord[KW_MAX_TOKENS];
        for (uint32_t t = 0; t < T.nl; t++) ord[t] = (uint8_t)t;
        std::stable_sort(ord, ord + T.nl, [&](uint8_t a, uint8_t b) { return T.len_of[a] < T.len_of[b]; });
        for (uint32_t t = 0; t < T.nl; t++) q.probe_order[t] = ord[t];
        QueryCut& c = cut[i];
        c.shape = QueryCut::SINGLE_FIELD;
        c.driver_blocks = snap.h_lists[q.list[ord[0]]].n_blocks;
        c.n_lists = T.nl; c.len_driver = T.len_of[ord[0]]; c.len_second = T.nl >= 2 ? T.len_of[ord[1]] : 0;
        q.ids_out_off = A.ids_total;
        if (keep_ids) A.ids_total += (uint64_t)c.driver_blocks * BLOCK_IDS;
    }

    // query i -> its KwQueryDev, its share of the slice's arenas and its QueryCut: the checks (the first that fails is the query's status), the token
    // lists, what every keyword query carries, then its shape
    void translate(uint32_t i, uint32_t lo, PlanAcc& A) {
        const tsgpu_kw_query& in = queries[i];
        KwQueryDev& q = P.q[i];
        memset(&q, 0, sizeof q);
        q.k = 1;
        auto refuse = [&](int status) { P.status[i] = status; };
        if (!wildcard && !kw_token_count_ok(in)) return refuse(TSGPU_ERR_UNSUPPORTED);
        if (!wildcard && !kw_field_count_ok(in)) return refuse(TSGPU_ERR_UNSUPPORTED);
        QueryTokens T;
        uint64_t token_bytes = 0;
        bool empty_here = false;
        if (!wildcard) {
            // the required tokens, resolved here because EVERY query with a legal token and field count enters the batch chunk, whatever it is refused for below:
            // one query_by field: its shortest list's blocks; several: the blocks of the token with the fewest postings over all fields, a quarter of them
            // (a multi-field driver block costs ~4x a single-field one — two tile merges, wider records — so these batches are cut finer; measured, 2 000
            //  two-field queries on 10M documents: 64-block items 20.4 ms, 16 -> 23.2, 256 -> 24.4; cut with the minimum chunk they were 101 000 work items)
            memset(&T.mfq, 0xFF, sizeof T.mfq);
            uint64_t best_ids = ~0ull; uint32_t best_blocks = 0xFFFFFFFFu;
            for (uint32_t t = 0; t < in.n_tokens; t++) {
                const KwTokenLists tl = kw_resolve_token(snap, in, in.term_ids[t]);
                if (!tl.found) { if (present_elsewhere && ((present_elsewhere[i] >> t) & 1u)) empty_here = true; continue; }      // (exists on another shard: an EMPTY list here)
                token_bytes += add_token(i, T, tl, (uint32_t)std::min<uint64_t>(tl.ids, 0xFFFFFFFFull));
                if (in.n_fields == 1) best_blocks = std::min(best_blocks, tl.blocks);
                else if (tl.ids < best_ids) { best_ids = tl.ids; best_blocks = tl.blocks; }
            }
            if (best_blocks == 0xFFFFFFFFu) best_blocks = 0;
            cut[i].chunk_blocks = in.n_fields == 1 ? best_blocks : best_blocks / 4;
            for (uint32_t f = 0; f < in.n_fields; f++) if (snap.field_is_array.find(in.field_ids[f]) == snap.field_is_array.end()) return refuse(TSGPU_ERR_NOT_FOUND);
        }
        // several fields, or a string[] field: the general kernel (per-candidate probes, per-field scoring incl. the array readers);
        // the block-merge kernel stays free of the array code (it costs 2x the registers)
        bool multi = !wildcard && in.n_fields > 1;
        if (!wildcard && !multi && snap.field_is_array.at(in.field_ids[0])) multi = true;
        // dropped tokens (drop_tokens passes): probed and scored per candidate, never required -> the general kernel
        if (!wildcard && in.n_dropped != 0) {
            if (!kw_dropped_count_ok(in)) return refuse(TSGPU_ERR_UNSUPPORTED);
            multi = true;
        }
        // filter ids with several query_by fields: num_keyword_matches has an order-free form only without exclusions (kw_score_stage)
        // filter ids AND excluded ids with several query_by fields: num_keyword_matches needs the intersection in id order — counted by
        // kw_mf_ordered_count_kernel from the find kernel's hit records, i.e. in the two-kernel form only (checked after the tables are laid out)
        const bool ordered_count = multi && in.n_filter != 0 && in.n_excluded != 0;
        if (ordered_count && !ctx->kw_two_kernels) return refuse(TSGPU_ERR_UNSUPPORTED);
        if (in.n_sort > TSGPU_MAX_SORT_KEYS) return refuse(TSGPU_ERR_INVALID);
        if (in.n_filter != 0 && !in.filter_ids) return refuse(TSGPU_ERR_INVALID);
        if (in.match_type > TSGPU_SUM_SCORE) return refuse(TSGPU_ERR_INVALID);
        uint64_t sort_bytes_per_id = 0;                             // what the sort slots read per ranked document (list_bytes)
        if (const int sort_rc = check_sort_slots(ctx, in.sort, in.n_sort, vflat != nullptr, vflat != nullptr, &sort_bytes_per_id)) return refuse(sort_rc);   // vector_distance belongs to the vector/hybrid entry points
        for (uint32_t s = 0; s < in.n_sort; s++) if (in.sort[s].kind == TSGPU_SORT_VECTOR_QUERY) A.any_vq = true;      // (keyword and wildcard launches: the kernels' VQ instantiations)
        const uint32_t k = vflat ? std::max<uint32_t>(in.topster_size, 1) : resolve_topster_size(ctx, in);     // (the vector branch resolved it against ITS filter / row count)
        if (k > TSGPU_MAX_TOPK) return refuse(TSGPU_ERR_UNSUPPORTED);
        if (in.deadline_us != 0 && now > in.deadline_us) { P.cutoff[i] = 1; return refuse(TSGPU_ERR_DEADLINE); }
        if (in.deadline_us != 0) { q.deadline_rem_us = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(in.deadline_us - now, 1), 0xFFFFFFFFull); A.any_deadline = true; }
        if (wildcard) return wildcard_query(i, lo, k, sort_bytes_per_id, A);

        q.mf_index = KW_NONE;
        if (empty_here) T.nl = 0;             // a required token without postings on this shard: the AND finds nothing here (zero hits below), whatever the others hold
        q.n_required = T.nl;
        for (uint32_t t = 0; t < in.n_dropped && multi; t++) {        // after the query's own tokens, in their order (:5271-5290)
            const KwTokenLists tl = kw_resolve_token(snap, in, in.dropped_term_ids[t]);
            if (tl.found) token_bytes += add_token(i, T, tl, 0xFFFFFFFFu);      // (an or_iterator without lists is left out: skip_to() is false for every document)
        }
        A.list_bytes += token_bytes;
        q.n_lists = T.nl;
        kw_fill_scoring(in, q);
        kw_fill_sort_slots(in, q);
        if (in.n_sort > 2) A.any_s2 = true;
        q.k = k;
        A.max_k = std::max(A.max_k, k);
        q.aux_off = (uint32_t)A.aux.size();
        q.n_excl = in.n_excluded;
        q.n_filt = in.n_filter;
        if (in.n_excluded || in.n_filter) A.any_aux = true;
        for (uint32_t s = 0; s < in.n_sort; s++) if (in.sort[s].kind >= TSGPU_SORT_EVAL) A.any_aux = true;      // (the PLAIN score kernels carry no sort-key code)
        if (in.n_excluded) {
            if (!in.excluded_ids) return refuse(TSGPU_ERR_INVALID);
            A.aux.insert(A.aux.end(), in.excluded_ids, in.excluded_ids + in.n_excluded);
        }
        if (in.n_filter) A.aux.insert(A.aux.end(), in.filter_ids, in.filter_ids + in.n_filter);   // sorted ascending, unique (filter_result_t::docs)
        if (q.n_required == 0) return;     // no token in the index: zero hits (intersect case 0, or_iterator.h:67-68)
        if (multi) multi_field_query(i, k, ordered_count, T, A);
        else single_field_query(i, T, A);
    }

    // the cut of query i's driver list(s) into work items (kw_plan_policy.h) and, for the block-merge kernels, its launch-order cost
    void cut_items(uint32_t i, uint32_t batch_chunk, PlanAcc& A) {
        const QueryCut& c = cut[i];
        if (P.status[i] != TSGPU_OK || c.shape == QueryCut::NONE) return;
        if (c.shape == QueryCut::WILDCARD) return emit_items(A.flat_work, q_begin[i], q_cnt[i], i, c.driver_blocks, KW_POLICY_WILDCARD_CHUNK, 0);
        if (c.shape == QueryCut::MULTI_FIELD) {
            const KwQueryMF& mfq = A.mf[P.q[i].mf_index];
            uint64_t seg = 0;
            for (uint32_t f = 0; f < mfq.n_fields; f++) {
                if (mfq.list[mfq.driver_token][f] == KW_NONE) continue;
                const uint32_t n_blocks = snap.h_lists[mfq.list[mfq.driver_token][f]].n_blocks;
                emit_items(A.flat_work, q_begin[i], q_cnt[i], i | (f << 28), n_blocks, batch_chunk, (uint32_t)seg);
                seg += (uint64_t)n_blocks * BLOCK_IDS;
            }
            return;
        }
        const uint32_t chunk_q = kw_policy_query_chunk(batch_chunk, ctx->kw_chunk_blocks == 0, c.driver_blocks,
                                                       kw_policy_max_partials(ctx->kw_max_partials, c.driver_blocks, n_queries, ctx->kw_merge_select_min));
        item_cost[i] = kw_policy_item_cost<double>(chunk_q, c.driver_blocks, c.n_lists, c.len_driver, c.len_second, ctx->num_docs, (double)ctx->kw_cost_fixed,
                                                   0.1 * ctx->kw_cost_r_x10, 0.01 * ctx->kw_cost_probe_x100);
        emit_items(A.flat_work, q_begin[i], q_cnt[i], i, c.driver_blocks, chunk_q, 0);
    }

    // the slices' arenas one behind the other, every query's offsets shifted by its slice's bases
    void concatenate(std::vector<PlanAcc>& parts, const QuerySlices& sl) {
        for (uint32_t k = 0; k < sl.n_parts; k++) {
            PlanAcc& A = parts[k];
            const uint32_t aux_base = (uint32_t)P.aux.size(), mf_base = (uint32_t)P.mf.size(), work_base = (uint32_t)flat_work.size();
            const uint64_t ids_base = P.ids_total, fbits_base = P.fbits_words;
            for (uint32_t i = sl.bound(k); k && i < sl.bound(k + 1); i++) {
                KwQueryDev& q = P.q[i];
                q.aux_off += aux_base; q.ids_out_off += ids_base; q.fbits_off += fbits_base;
                if (q.mf_index != KW_NONE && P.status[i] == TSGPU_OK && !q.wild_n_ids) q.mf_index += mf_base;
                q_begin[i] += work_base;
            }
            if (k == 0) { P.aux.swap(A.aux); P.mf.swap(A.mf); flat_work.swap(A.flat_work); }
            else {
                P.aux.insert(P.aux.end(), A.aux.begin(), A.aux.end());
                P.mf.insert(P.mf.end(), A.mf.begin(), A.mf.end());
                flat_work.insert(flat_work.end(), A.flat_work.begin(), A.flat_work.end());
            }
            P.ordered_count_q.insert(P.ordered_count_q.end(), A.ordered_count_q.begin(), A.ordered_count_q.end());
            P.ids_total += A.ids_total; P.fbits_words += A.fbits_words; P.list_bytes += A.list_bytes;
            P.max_k = std::max(P.max_k, A.max_k);
            P.any_deadline = P.any_deadline || A.any_deadline; P.any_s2 = P.any_s2 || A.any_s2; P.any_aux = P.any_aux || A.any_aux; P.any_vq = P.any_vq || A.any_vq; P.any_array = P.any_array || A.any_array; P.mf_max_fields = std::max(P.mf_max_fields, A.mf_max_fields);
        }
    }

    // the queries by descending cost, ties in query order (option kw_sort_work; else query order)
    std::vector<uint32_t> cost_order() const {
        std::vector<uint32_t> by_cost(n_queries);
        for (uint32_t i = 0; i < n_queries; i++) by_cost[i] = i;
        if (!ctx->kw_sort_work) return by_cost;
        // LSD radix sort of the float bits (costs are non-negative, so the bits order like the values), two stable counting passes of 16 bits (std::sort of
        // 10 000 keys was 0.33 ms of a 0.95 ms plan; a coarser one-pass bucket order measurably lengthened the find kernel's tail)
        // (the two 65 536-entry histograms are a FIXED ~30 us: a small round — the 1-query calling convention — sorts by comparison)
        std::vector<uint32_t> key(n_queries);
        for (uint32_t i = 0; i < n_queries; i++) { const float c = (float)item_cost[i]; uint32_t bits; memcpy(&bits, &c, 4); key[i] = 0xFFFFFFFFu - bits; }
        if (n_queries < 2048) { std::stable_sort(by_cost.begin(), by_cost.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; }); return by_cost; }
        std::vector<uint32_t> tmp(n_queries), hist(65537);
        for (int pass = 0; pass < 2; pass++) {
            const int sh = pass * 16;
            std::fill(hist.begin(), hist.end(), 0u);
            for (uint32_t i = 0; i < n_queries; i++) hist[((key[by_cost[i]] >> sh) & 0xFFFFu) + 1]++;
            for (uint32_t k = 0; k < 65536; k++) hist[k + 1] += hist[k];
            for (uint32_t i = 0; i < n_queries; i++) { const uint32_t q = by_cost[i]; tmp[hist[(key[q] >> sh) & 0xFFFFu]++] = q; }
            by_cost.swap(tmp);
        }
        return by_cost;
    }

    // work tables: one launch per kernel flavour (single-field T<=3, single-field generic, multi-field T<=3, multi-field generic, wildcard); a query's
    // items stay contiguous and first_work indexes the one table that holds the five back to back, heaviest query first inside each
    void layout_tables(const std::vector<uint32_t>& by_cost) {
        auto flavour_of = [&](uint32_t i) { return P.q[i].wild_n_ids ? 4 : (P.q[i].mf_index != KW_NONE ? 2 : 0) + (P.q[i].n_lists <= 3 ? 0 : 1); };
        size_t at[5], acc = 0;
        for (uint32_t i = 0; i < n_queries; i++) if (q_cnt[i]) P.n_tab[flavour_of(i)] += q_cnt[i];
        for (int k = 0; k < 5; k++) { at[k] = acc; acc += P.n_tab[k]; }
        P.work.resize(acc);
        for (uint32_t i : by_cost) {
            if (q_cnt[i] == 0) continue;
            size_t& dst = at[flavour_of(i)];
            P.q[i].first_work = (uint32_t)dst;
            P.q[i].n_work = q_cnt[i];
            std::copy(flat_work.begin() + q_begin[i], flat_work.begin() + q_begin[i] + q_cnt[i], P.work.begin() + dst);
            dst += q_cnt[i];
        }
    }

    // merge sources: the work items' lists, or group lists of 8 folded in parallel first (slots behind the work items' own; kw_plan_policy.h)
    void merge_sources() {
        uint32_t slot = (uint32_t)P.work.size();
        for (uint32_t i = 0; i < n_queries; i++) {
            KwQueryDev& q = P.q[i];
            q.m_first = q.first_work; q.m_n = q.n_work;
            if (!kw_policy_needs_merge_groups(q.n_work, ctx->kw_merge_select_min)) continue;
            q.m_first = slot;
            q.m_n = (q.n_work + KW_MERGE_GROUP - 1) / KW_MERGE_GROUP;
            for (uint32_t a = 0; a < q.n_work; a += KW_MERGE_GROUP) P.groups.push_back({i, q.first_work + a, std::min(KW_MERGE_GROUP, q.n_work - a), slot++});
        }
    }
};
}  // namespace

static int plan_batch(tsgpu_ctx* ctx, const Snapshot& snap, const tsgpu_kw_query* queries, uint32_t n_queries, Plan& P, bool keep_ids, bool wildcard, const KwVFlat* vflat = nullptr,
                      const uint16_t* present_elsewhere = nullptr, const uint64_t* wild_ids_dev = nullptr, const uint64_t* wild_tm_dev = nullptr) {
    static const bool plan_timing = getenv("TSGPU_HOST_TIMING") != nullptr;
    const uint64_t tp0 = now_us();
    P.q.resize(n_queries);
    P.status.assign(n_queries, TSGPU_OK);
    P.cutoff.assign(n_queries, 0);
    BatchPlanner B{ctx, snap, queries, n_queries, P, keep_ids, wildcard, vflat, present_elsewhere, tp0,
                   std::vector<QueryCut>(n_queries), std::vector<uint32_t>(n_queries, 0), std::vector<uint32_t>(n_queries, 0), std::vector<double>(n_queries, 0.0), {}};
    B.wild_ids_dev = wild_ids_dev; B.wild_tm_dev = wild_tm_dev;
    const uint32_t min_par = ctx->plan_parallel_min_queries;
    const uint32_t min_slice = std::max<uint32_t>(8, min_par / 8);                      // (256 queries per slice at the default threshold)
    QuerySlices sl{n_queries, 1, 1};
    if (min_par && n_queries >= min_par) sl.n_thr = std::min<uint32_t>((uint32_t)std::max(1, ctx->plan_threads), std::max<uint32_t>(1, n_queries / min_slice));
    if (sl.n_thr > 1) sl.n_parts = std::min<uint32_t>(4 * sl.n_thr, std::max<uint32_t>(1, n_queries / std::max<uint32_t>(8, min_slice / 4)));
    std::vector<PlanAcc> parts(sl.n_parts);
    // per-query planning
    for_query_slices(ctx, sl, [&](uint32_t k, uint32_t lo, uint32_t hi) { for (uint32_t i = lo; i < hi; i++) B.translate(i, lo, parts[k]); });
    // driver blocks per work item: fixed by the option, or sized from the batch's driver blocks
    uint32_t chunk = ctx->kw_chunk_blocks;
    if (chunk == 0) {
        uint64_t total_blocks = 0;
        for (uint32_t i = 0; i < n_queries; i++) total_blocks += B.cut[i].chunk_blocks;
        chunk = kw_policy_batch_chunk(total_blocks, (uint32_t)KW_MAX_CHUNK, n_queries, ctx->kw_merge_select_min);
    }
    for_query_slices(ctx, sl, [&](uint32_t k, uint32_t lo, uint32_t hi) { parts[k].flat_work.reserve((size_t)(hi - lo) * 4); for (uint32_t i = lo; i < hi; i++) B.cut_items(i, chunk, parts[k]); });
    B.concatenate(parts, sl);
    const uint64_t tp1 = now_us();
    const std::vector<uint32_t> by_cost = B.cost_order();
    const uint64_t tp2 = now_us();
    B.layout_tables(by_cost);
    B.merge_sources();
    if (plan_timing) fprintf(stderr, "[tsgpu] plan: per-query loop %llu us, cost sort %llu us, table layout %llu us\n", (unsigned long long)(tp1 - tp0),
                             (unsigned long long)(tp2 - tp1), (unsigned long long)(now_us() - tp2));
    return TSGPU_OK;
}

// ---- the same plan made ON THE DEVICE (kw_plan.hip.h) for batches of plain single-field queries ----
namespace {
struct DevPlan {
    bool on = false;
    const KwQueryDev* dq = nullptr; const KwWorkItem* dw = nullptr; const uint32_t* daux = nullptr; const uint64_t* hoff = nullptr;
    uint32_t n_work[2] = {0, 0};
    uint64_t hit_blocks[2] = {0, 0};
};
}
// returns TSGPU_OK (DP.on tells whether the device made the plan; false = this batch needs the host planner) or an error
static int plan_batch_device(tsgpu_ctx* ctx, KwLane& L, const Snapshot& snap, const tsgpu_kw_query* queries, uint32_t n_queries, Plan& P, DevPlan& DP, hipStream_t s) {
    DP.on = false;
    if (!snap.maps || !snap.maps->d_dense.p || !snap.lists.p) return TSGPU_OK;
    // host pre-scan: eligibility + the 76-byte record per query, straight into the pinned staging buffer
    int rc;
    if ((rc = L.h_plan.reserve((size_t)n_queries * sizeof(KwPlanIn) + 64))) return rc;
    KwPlanIn* hin = (KwPlanIn*)L.h_plan.p;
    const uint32_t n_columns = (uint32_t)ctx->columns.size();
    std::atomic<int> bad{0}, any_keys{0}, any_vq{0};
    auto scan = [&](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; i++) {
            const tsgpu_kw_query& in = queries[i];
            bool ok = in.n_fields == 1 && kw_token_count_ok(in) && in.n_dropped == 0 && in.n_filter == 0 && in.n_excluded == 0 &&
                      in.deadline_us == 0 && in.n_sort <= TSGPU_MAX_SORT_KEYS && in.match_type <= TSGPU_SUM_SCORE && in.field_ids[0] < 64;
            if (ok) { auto it = snap.field_is_array.find(in.field_ids[0]); ok = it != snap.field_is_array.end() && !it->second; }
            for (uint32_t k = 0; ok && k < in.n_sort; k++)
                ok = in.sort[k].kind != TSGPU_SORT_VECTOR_DISTANCE && (!sort_kind_reads_column(in.sort[k].kind) || in.sort[k].column < n_columns);
            for (uint32_t k = 0; ok && k < in.n_sort; k++) if (in.sort[k].kind >= TSGPU_SORT_EVAL) { any_keys.store(1, std::memory_order_relaxed); if (in.sort[k].kind == TSGPU_SORT_VECTOR_QUERY) any_vq.store(1, std::memory_order_relaxed); }
            ok = ok && check_sort_slots(ctx, in.sort, in.n_sort, false, false, nullptr) == TSGPU_OK;      // (a bad handle, two _eval slots, ...: the host planner reports them per query)
            const uint32_t k = ok ? resolve_topster_size(ctx, in) : 0;
            if (!ok || k > TSGPU_MAX_TOPK) { bad.store(1); return; }
            KwPlanIn& r = hin[i];
            for (uint32_t t = 0; t < (uint32_t)TSGPU_MAX_QUERY_TOKENS; t++) r.term_ids[t] = t < in.n_tokens ? in.term_ids[t] : 0;
            r.field = in.field_ids[0]; r.weight = in.field_weights[0]; r.k = k; r.total_cost = in.total_cost;
            r.n_tokens = (uint8_t)in.n_tokens; r.match_type = in.match_type;
            r.prio_bits = (uint8_t)((in.prioritize_exact_match ? 1 : 0) | (in.prioritize_token_position ? 2 : 0) | (in.prioritize_num_matching_fields ? 4 : 0));
            r.n_sort = (uint8_t)in.n_sort;
            for (uint32_t k2 = 0; k2 < 3; k2++) { r.sort_kind[k2] = k2 < in.n_sort ? in.sort[k2].kind : 0; r.sort_order[k2] = k2 < in.n_sort ? in.sort[k2].order : 0; r.sort_col[k2] = k2 < in.n_sort ? in.sort[k2].column : 0; }
            r.syn_orig_num_tokens = (int8_t)((int)in.syn_orig_num_tokens_p1 - 1); r.orig_num_tokens = in.orig_num_tokens;
            r.is_synonym = in.is_synonym_query ? 1 : 0; r.demote_synonym = in.demote_synonym_match ? 1 : 0;
        }
    };
    {
        const uint32_t min_par = ctx->plan_parallel_min_queries;
        const uint32_t n_thr = (min_par && n_queries >= min_par) ? std::min<uint32_t>((uint32_t)std::max(1, ctx->plan_threads), std::max<uint32_t>(1, n_queries / 512)) : 1;
        for_query_slices(ctx, QuerySlices{n_queries, n_thr, n_thr <= 1 ? 1 : 4 * n_thr}, [&](uint32_t, uint32_t lo, uint32_t hi) { if (!bad.load()) scan(lo, hi); });
    }
    if (bad.load()) return TSGPU_OK;
    // device buffers: [KwQueryDev x n | one aux word | totals | six scratch arrays] in d_plan, the input records in d_plan_in
    Placer place;
    const size_t at_q = place((size_t)n_queries * sizeof(KwQueryDev)), at_aux = place(64), at_tot = place(sizeof(KwPlanTotals)), at_nb = place((size_t)n_queries * 4),
                 at_la = place((size_t)n_queries * 4), at_lb = place((size_t)n_queries * 4), at_cnt = place((size_t)n_queries * 4), at_ch = place((size_t)n_queries * 4),
                 at_key = place((size_t)n_queries * 8), at_fw = place((size_t)n_queries * 4), at_hb = place((size_t)n_queries * 8);
    if ((rc = L.d_plan.reserve(place.bytes + 64)) || (rc = L.d_plan_in.reserve((size_t)n_queries * sizeof(KwPlanIn))) || (rc = L.h_plan_tot.reserve(2 * sizeof(KwPlanTotals)))) return rc;
    uint8_t* const dp = (uint8_t*)L.d_plan.p;
    KwPlanTotals* const d_tot = (KwPlanTotals*)(dp + at_tot);
    KwPlanTotals* const h_tot = (KwPlanTotals*)L.h_plan_tot.p;
    TSGPU_HIP_TRY(hipMemcpyAsync(L.d_plan_in.p, hin, (size_t)n_queries * sizeof(KwPlanIn), hipMemcpyHostToDevice, s));
    TSGPU_HIP_TRY(hipMemsetAsync(dp + at_aux, 0, 64 + sizeof(KwPlanTotals) + 64, s));
    KwPlanParams pp;
    pp.n_queries = n_queries; pp.num_docs = ctx->num_docs; pp.n_columns = n_columns;
    pp.chunk_blocks_opt = ctx->kw_chunk_blocks; pp.max_partials = std::max<uint32_t>(ctx->kw_max_partials, 1); pp.merge_select_min = ctx->kw_merge_select_min; pp.max_chunk = (uint32_t)KW_MAX_CHUNK;
    pp.cost_fixed = (float)ctx->kw_cost_fixed; pp.cost_r = 0.1f * ctx->kw_cost_r_x10; pp.cost_probe = 0.01f * ctx->kw_cost_probe_x100;
    pp.dense = snap.maps->d_dense.as<uint32_t>(); pp.lists = snap.lists.as<ListDesc>();
    KwPlanScratch sc;
    sc.n_blocks = (uint32_t*)(dp + at_nb); sc.len_a = (uint32_t*)(dp + at_la); sc.len_b = (uint32_t*)(dp + at_lb); sc.cnt = (uint32_t*)(dp + at_cnt); sc.chunk = (uint32_t*)(dp + at_ch);
    sc.key = (unsigned long long*)(dp + at_key);
    KwQueryDev* const dq = (KwQueryDev*)(dp + at_q);
    const dim3 grid((n_queries + 255) / 256), block(256);
    hipLaunchKernelGGL(kw_plan_resolve_kernel, grid, block, 0, s, pp, (const KwPlanIn*)L.d_plan_in.p, dq, sc, d_tot);
    hipLaunchKernelGGL(kw_plan_chunk_kernel, grid, block, 0, s, pp, (const KwQueryDev*)dq, sc, d_tot);
    TSGPU_HIP_TRY(hipGetLastError());
    TSGPU_HIP_TRY(hipMemcpyAsync(h_tot, d_tot, sizeof(KwPlanTotals), hipMemcpyDeviceToHost, s));
    TSGPU_HIP_TRY(hipStreamSynchronize(s));
    const KwPlanTotals t1 = *h_tot;
    if (t1.fallback) return TSGPU_OK;
    // the hit buffer must take each table in ONE group (else the host planner's grouping / the fused kernel decide)
    for (int tb = 0; tb < 2; tb++) {
        const size_t rec_bytes = (size_t)((tb == 0 ? 3 : KW_MAX_TOKENS) + 1) * 4;
        if (t1.hit_blocks[tb] * (uint64_t)BLOCK_IDS > hit_budget_records(ctx, rec_bytes)) return TSGPU_OK;
    }
    const size_t n_work = (size_t)t1.n_work[0] + t1.n_work[1];
    if ((rc = L.d_plan_work.reserve(std::max<size_t>(n_work, 1) * (sizeof(KwWorkItem) + 8) + 64))) return rc;
    KwWorkItem* const dw = (KwWorkItem*)L.d_plan_work.p;
    unsigned long long* const hoff = (unsigned long long*)((uint8_t*)L.d_plan_work.p + ((std::max<size_t>(n_work, 1) * sizeof(KwWorkItem) + 63) & ~(size_t)63));
    TSGPU_HIP_TRY(hipMemsetAsync(dp + at_fw, 0, (at_hb - at_fw) + (size_t)n_queries * 8, s));
    hipLaunchKernelGGL(kw_plan_rank_kernel, dim3(grid.x, KW_PLAN_JPARTS), block, 0, s, pp, sc, (uint32_t*)(dp + at_fw), (unsigned long long*)(dp + at_hb));
    hipLaunchKernelGGL(kw_plan_emit_kernel, grid, block, 0, s, pp, dq, sc, (const uint32_t*)(dp + at_fw), (const unsigned long long*)(dp + at_hb), dw, hoff, (const KwPlanTotals*)d_tot);
    TSGPU_HIP_TRY(hipGetLastError());
    P.status.assign(n_queries, TSGPU_OK);
    P.cutoff.assign(n_queries, 0);
    P.max_k = std::max<uint32_t>(t1.max_k, 1); P.any_s2 = t1.any_s2 != 0; P.list_bytes = t1.list_bytes;
    P.any_aux = any_keys.load() != 0;                  // (a sort-key slot in the batch: the score kernels with the sort-key code)
    P.any_vq = any_vq.load() != 0;
    DP.on = true;
    DP.dq = dq; DP.dw = dw; DP.daux = (const uint32_t*)(dp + at_aux); DP.hoff = (const uint64_t*)hoff;
    DP.n_work[0] = t1.n_work[0]; DP.n_work[1] = t1.n_work[1]; DP.hit_blocks[0] = t1.hit_blocks[0]; DP.hit_blocks[1] = t1.hit_blocks[1];
    return TSGPU_OK;
}

// ---- lanes ----
namespace {
struct LaneLock {                                     // holds one execution lane for the duration of a batch (FIFO: LaneDispenser)
    tsgpu_ctx* ctx; KwLane* L; int index;
    explicit LaneLock(tsgpu_ctx* c, int want = -1) : ctx(c), L(nullptr), index(-1) {
        index = c->lane_dispenser.acquire(want, c->n_lanes);
        L = &c->lanes[index];
        L->mu.lock();                                 // (uncontended among LaneLock holders; tsgpu_set_stream takes it, too)
        c->last_lane.store(index);
    }
    ~LaneLock() { L->mu.unlock(); ctx->lane_dispenser.release(index, ctx->n_lanes); }
};
// Slices of a sliced host-output batch: they are ENQUEUED in slice order (turn), whichever host thread finishes planning first — the large first
// slice has to run first, so that its device-to-host copy runs under the small ones' kernels (left to the planning race, the small second slice was
// usually enqueued ahead of it: kernel timeline in profiles/r04) — and a slice's kernels start when the previous slice's have finished (last).
struct SliceChain {
    std::mutex m; std::condition_variable cv; uint32_t turn = 0; hipEvent_t last = nullptr;
    // RAII for one slice: wait_turn() before enqueueing; the destructor passes the turn on (also on every error path, after waiting for it)
    struct Turn {
        SliceChain* c; uint32_t idx; bool waited = false; std::unique_lock<std::mutex> lk;
        Turn(SliceChain* c_, uint32_t i) : c(c_), idx(i) {}
        void wait_turn() { if (!c) return; lk = std::unique_lock<std::mutex>(c->m); c->cv.wait(lk, [&] { return c->turn == idx; }); waited = true; }
        void pass() { if (!c) return; if (!waited) wait_turn(); c->turn = idx + 1; c = nullptr; lk.unlock(); }
        ~Turn() { if (c) { SliceChain* cc = c; pass(); cc->cv.notify_all(); } }
    };
};
struct BatchOpts {
    bool wildcard = false;
    bool keep_ids = false;                            // emit matched ids into the lane's id arena
    std::vector<int32_t>* status_host = nullptr;      // receives the per-query status codes
    std::vector<int32_t>* cutoff_host = nullptr;      // ... and the per-query search_cutoff flags
    tsgpu_id_lists* id_lists = nullptr;               // when set: the matched ids of every query, gathered + downloaded (implies keep_ids)
    bool record_last = true;                          // remember the id segments for the legacy tsgpu_result_ids API
    uint32_t chain_index = 0;                         // ... this slice's position in it
    SliceChain* chain = nullptr;                      // sliced host-output batch: this slice's kernels start when the previous slice's have finished (a
                                                      // device-side wait; the previous slice's device-to-host copies run meanwhile: two slices never compute at once)
    bool alias_out = false;                           // host output through the lane's pinned image: point `out`'s arrays INTO the image instead of copying
                                                      // them out (the coalesced round hands every caller its slice straight from there)
    bool timing = true;                               // record the phase events (tsgpu_timings); a coalesced round has no single caller to report to
    const KwVFlat* vflat = nullptr;                   // wildcard form ranking a distance matrix: the flat branch of the vector search (tsgpu_vector_search_batch)
    DevBuf* ids_dev = nullptr;                        // with id_lists: gather the matched ids into THIS device buffer (the caller's) and leave id_lists->ids empty — for a
    bool* ids_dev_done = nullptr;                     // consumer on the device (group_by, tsgpu_groupby.inc.h); not done (false) when a query's ids need the host's sort
    const uint16_t* present_elsewhere = nullptr;      // doc-range shard of a group whose members' dictionaries differ: per query, the tokens that exist on ANOTHER shard
                                                      // (missing here they are empty lists, not dropped tokens: kw_search_batch_masked, tsgpu_host.h); host planner
    const uint64_t* wild_ids_dev = nullptr;           // wildcard batch of the infix front (tsgpu_infix_search_batch): the queries' filter ids are device arrays (KwQueryDev::wild_ids)
    const uint64_t* wild_tm_dev = nullptr;            // ... of the phrase front (tsgpu_phrase_search_batch): their text-match values, device arrays too (KwQueryDev::wild_tm)
};
}
static int kw_batch_on_lane(tsgpu_ctx* ctx, KwLane& L, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, const BatchOpts& bo);
static int kw_dispatch(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, bool wildcard, tsgpu_id_lists** ids_out, DevBuf* ids_dev = nullptr, bool* ids_dev_done = nullptr,
                       const uint16_t* present_elsewhere = nullptr);
static int kw_split_host(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out);

int tsgpu_keyword_search_batch(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out) {
    return kw_dispatch(ctx, queries, n_queries, out, false, nullptr);
}

int tsgpu_wildcard_search_batch(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out) {
    return kw_dispatch(ctx, queries, n_queries, out, true, nullptr);
}

int tsgpu_keyword_search_batch_ids(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, tsgpu_id_lists** ids_out) {
    if (!ids_out) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_batch_ids: ids_out is NULL");
    *ids_out = nullptr;
    return kw_dispatch(ctx, queries, n_queries, out, false, ids_out);
}

uint64_t tsgpu_id_lists_count(const tsgpu_id_lists* l, uint32_t q) { return (l && (size_t)q + 1 < l->begin.size()) ? l->begin[q + 1] - l->begin[q] : 0; }
const uint32_t* tsgpu_id_lists_ids(const tsgpu_id_lists* l, uint32_t q) { return (l && (size_t)q + 1 < l->begin.size()) ? l->ids.data() + l->begin[q] : nullptr; }
void tsgpu_id_lists_free(tsgpu_id_lists* l) { delete l; }

}  // extern "C"

namespace tsgpu {
// TSGPU_SORT_VECTOR_QUERY: the descriptor of every live vector-query key the queries name is rewritten from its field as it is NOW (tsgpu_host.h). The caller
// holds ctx->mu, so no vector mutation and no other batch that reads such a descriptor runs meanwhile; the copies are complete on return, before the batch's
// kernels are enqueued. Handles that are not live or of the other form are the planner's to refuse (check_sort_slots).
int refresh_vector_query_keys(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries) {
    std::vector<uint16_t> done;
    for (uint32_t i = 0; i < n_queries; i++) {
        for (uint32_t s = 0; s < queries[i].n_sort && s < TSGPU_MAX_SORT_KEYS; s++) {
            if (queries[i].sort[s].kind != TSGPU_SORT_VECTOR_QUERY) continue;
            const uint16_t handle = queries[i].sort[s].column;
            if (std::find(done.begin(), done.end(), handle) != done.end()) continue;
            done.push_back(handle);
            SortKeyDesc d;
            memset(&d, 0, sizeof d);
            uint32_t field;
            {
                std::lock_guard<std::mutex> lk(ctx->sk_mu);
                if (handle >= ctx->sort_keys.size() || !ctx->sort_keys[handle].live || !ctx->sort_keys[handle].vq) continue;
                const SortKeyHost& k = ctx->sort_keys[handle];
                field = k.vq_field;
                d.form = SORT_KEY_FORM_VECTOR_QUERY; d.vq_dim = k.vq_dim; d.vq_q = (const float*)k.buf.p; d.vq_threshold = k.vq_threshold;
            }
            VecSortView fv;
            if (const int rc = vec_sort_view(ctx, field, &fv, true)) return rc;
            d.vq_X = fv.X; d.vq_row_of_seq = fv.row_of_seq; d.vq_row_ok = fv.row_ok; d.vq_n_rows = fv.n_rows; d.vq_map_len = fv.map_len;
            d.vq_ip_lanes = ctx->vec_ip_lanes;
            TSGPU_HIP_TRY(hipMemcpyAsync(ctx->d_sort_keys.as<SortKeyDesc>() + handle, &d, sizeof d, hipMemcpyHostToDevice, ctx->sk_stream));
            TSGPU_HIP_TRY(hipStreamSynchronize(ctx->sk_stream));
        }
    }
    return TSGPU_OK;
}

struct KwRequest : ParkedRequest {
    const tsgpu_kw_query* q = nullptr;
    tsgpu_hits* out = nullptr;
    tsgpu_id_lists* ids = nullptr;                   // non-null: the caller wants its matched ids
    uint64_t t_arrive = 0, t_done = 0;               // diagnostics: when it parked / when its round's results were ready
};
}

// A small keyword call from one of several concurrent request threads: parked in the combiner, executed as part of one round.
static int kw_coalesced(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, tsgpu_id_lists** ids_out) {
    std::unique_ptr<tsgpu_id_lists> lists;
    if (ids_out) { lists.reset(new (std::nothrow) tsgpu_id_lists); if (!lists) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_keyword_search_batch_ids: host allocation failed"); }
    KwRequest me;
    me.units = n_queries; me.q = queries; me.out = out; me.ids = lists.get();
    me.t_arrive = now_us();
    auto amax = [](std::atomic<uint64_t>& a, uint64_t v) { uint64_t c = a.load(); while (v > c && !a.compare_exchange_weak(c, v)) {} };
    auto acquire = [&]() { return std::unique_ptr<LaneLock>(new LaneLock(ctx)); };
    const uint32_t round_cap = std::max<uint32_t>(ctx->batch_round_queries, n_queries);
    auto pick = [&](std::vector<KwRequest*>& pending, std::vector<KwRequest*>& round) {
        uint32_t units = 0;
        size_t take = 0;
        while (take < pending.size() && (take == 0 || units + pending[take]->units <= round_cap)) units += pending[take++]->units;
        round.assign(pending.begin(), pending.begin() + take);
        pending.erase(pending.begin(), pending.begin() + take);
    };
    auto exec = [&](std::vector<KwRequest*>& round, std::unique_ptr<LaneLock>& guard) {
        // a round with a vector-query sort key runs under ctx->mu (tsgpu_host.h), taken BEFORE the lane like everywhere else: the leader's lane goes back first
        CtxMuForVectorKeys vq_hold;
        if (ctx->sort_keys_live.load(std::memory_order_relaxed)) {
            bool vq = false;
            for (KwRequest* r : round) vq = vq || names_vector_query_key(r->q, r->units);
            if (vq) { guard.reset(); vq_hold.take(ctx); guard.reset(new LaneLock(ctx)); vq_hold.stream = guard->L->stream; }
        }
        KwLane& L = *guard->L;
        int rc = TSGPU_OK;
        std::string err;
        try {
            uint32_t total = 0, KS = 1;
            bool want_ids = false;
            // staging stride = the widest Topster of the round (not only the widest caller buffer): a caller whose own k_stride is too
            // small for its topster_size must fail ALONE (the per-caller `n > ks` check below), not take the round's other callers with it
            for (KwRequest* r : round) {
                total += r->units; KS = std::max(KS, r->out->k_stride); want_ids = want_ids || r->ids != nullptr;
                for (uint32_t i = 0; i < r->units; i++) KS = std::max(KS, std::min<uint32_t>(resolve_topster_size(ctx, r->q[i]), TSGPU_MAX_TOPK));
            }
            L.c_q.resize(total);
            uint32_t at = 0;
            for (KwRequest* r : round) { memcpy(L.c_q.data() + at, r->q, (size_t)r->units * sizeof(tsgpu_kw_query)); at += r->units; }
            const size_t slots = (size_t)total * KS;
            auto grow = [](auto& v, size_t n) { if (v.size() < n) v.resize(n); };     // (grow-only: a shrink + regrow zero-fills the difference every round)
            grow(L.c_keys, slots); grow(L.c_scores, slots * 3); grow(L.c_tm, slots); grow(L.c_vd, slots); grow(L.c_msi, slots);
            grow(L.c_nh, total); grow(L.c_nm, total); grow(L.c_st, total); grow(L.c_co, total);
            tsgpu_hits h;
            h.mem = TSGPU_MEM_HOST; h.k_stride = KS;
            h.keys = L.c_keys.data(); h.scores = L.c_scores.data(); h.text_match = L.c_tm.data(); h.vector_distance = L.c_vd.data();
            h.match_score_index = L.c_msi.data(); h.n_hits = L.c_nh.data(); h.num_matched = L.c_nm.data(); h.status = L.c_st.data(); h.search_cutoff = L.c_co.data();
            tsgpu_id_lists all_ids;
            BatchOpts bo;
            bo.keep_ids = want_ids;
            bo.id_lists = want_ids ? &all_ids : nullptr;
            bo.record_last = false;
            bo.timing = false;
            bo.alias_out = true;                     // h's arrays may come back pointing into the lane's pinned result image
            const uint64_t te0 = now_us();
            uint64_t qsum = 0;
            for (KwRequest* r : round) { amax(ctx->kw_max_queue_us, te0 - r->t_arrive); qsum += te0 - r->t_arrive; }
            ctx->kw_queue_us.fetch_add(qsum);
            rc = kw_batch_on_lane(ctx, L, L.c_q.data(), total, &h, bo);
            const uint64_t te1 = now_us();
            ctx->batch_exec_us.fetch_add(te1 - te0);
            if (rc != TSGPU_OK) err = tls_error();
            else {
                at = 0;
                for (KwRequest* r : round) {
                    tsgpu_hits& o = *r->out;
                    const uint32_t ks = o.k_stride;
                    for (uint32_t i = 0; i < r->units; i++) {
                        const uint32_t g = at + i;
                        int32_t st = h.status[g];
                        uint32_t n = h.n_hits[g];
                        if (st == TSGPU_OK && n > ks) { st = TSGPU_ERR_INVALID; n = 0; }       // (this caller's k_stride is smaller than its topster_size)
                        o.status[i] = st;
                        o.n_hits[i] = n;
                        if (o.num_matched) o.num_matched[i] = st == TSGPU_OK ? h.num_matched[g] : 0;
                        if (o.search_cutoff) o.search_cutoff[i] = h.search_cutoff[g];
                        const size_t src = (size_t)g * KS, dst = (size_t)i * ks;
                        memcpy(o.keys + dst, h.keys + src, (size_t)n * 8);
                        memcpy(o.scores + dst * 3, h.scores + src * 3, (size_t)n * 24);
                        if (o.text_match) memcpy(o.text_match + dst, h.text_match + src, (size_t)n * 8);
                        if (o.vector_distance) memcpy(o.vector_distance + dst, h.vector_distance + src, (size_t)n * 4);
                        if (o.match_score_index) memcpy(o.match_score_index + dst, h.match_score_index + src, (size_t)n);
                    }
                    if (r->ids) {
                        r->ids->begin.resize((size_t)r->units + 1);
                        const uint64_t b0 = all_ids.begin[at];
                        for (uint32_t i = 0; i <= r->units; i++) r->ids->begin[i] = all_ids.begin[at + i] - b0;
                        r->ids->ids.assign(all_ids.ids.begin() + b0, all_ids.ids.begin() + all_ids.begin[at + r->units]);
                    }
                    at += r->units;
                }
                ctx->batch_scatter_us.fetch_add(now_us() - te1);
            }
        } catch (const std::bad_alloc&) { rc = TSGPU_ERR_NO_MEMORY; err = "tsgpu_keyword_search_batch: host allocation failed"; }
        const uint64_t td = now_us();
        for (KwRequest* r : round) { r->rc = rc; r->err = err; r->t_done = td; }
    };
    ctx->kw_comb.run(me, ctx->kw_callers, ctx->batch_window_us, acquire, pick, exec);
    if (me.t_done) { const uint64_t w = now_us() - me.t_done; amax(ctx->kw_max_wake_us, w); ctx->kw_wake_us.fetch_add(w); }
    if (me.rc != TSGPU_OK) return fail(me.rc, me.err);
    if (ids_out) *ids_out = lists.release();
    return ok();
}

extern "C" {

// Entry of every keyword / wildcard search call. Small host-output calls from concurrent request threads (the reference calls
// the seam once per query from its thread pool, src/index.cpp:3488, src/http_server.cpp:827-832) are coalesced by the
// micro-batcher into one launch; everything else takes a lane directly.
// A LARGE batch whose results go to host memory: 82-112 MB of hit arrays per 10 000 queries cross PCIe, 1.5-2 ms behind a 6.3 ms step when
// the copies start after the last kernel. Served in slices instead, each on a lane and host thread of its own: a slice computes while the
// previous one's copies run (the slices are ENQUEUED in slice order and their kernels chained by events: sharing the chip, each would take
// twice as long and they would reach their copies together). Results are those of separate calls per slice = those of one call (a query
// never influences another).
static int kw_split_host(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out) {
    // slice sizes: the LAST slice's copies are the part nothing overlaps, and every slice costs launch tails + copy calls: a large
    // first slice (kw_host_split_first_pct of the batch), the rest in one slice (two with kw_host_split_tail_slices = 2)
    std::vector<uint32_t> start(1, 0);
    {
        uint32_t first = (uint32_t)((uint64_t)n_queries * ctx->kw_host_split_first_pct / 100);
        first = std::min(std::max(first, ctx->kw_host_split_queries), n_queries - ctx->kw_host_split_queries);
        start.push_back(first);
        // ONE tail slice (round 4, kernel timeline in profiles/r04/exp_host_delivery_r04.txt): every extra launch has its own tail of long work items —
        // three slices kept the GPU busy for 8.4 ms against 6.3 ms for one launch — and with the slices enqueued in order the large one's copy
        // hides under ONE small slice's kernels: 85 % + 15 % = 7.5 ms per 10 000 queries (70 / 15 / 15: 8.0 ms; unsliced: 8.1 ms)
        const uint32_t rest = n_queries - first, parts = ctx->kw_host_split_tail_slices >= 2 && rest >= 2 * ctx->kw_host_split_queries ? 2 : 1;
        for (uint32_t i = 1; i <= parts; i++) start.push_back(first + (uint32_t)((uint64_t)rest * i / parts));
    }
    const uint32_t n_slices = (uint32_t)start.size() - 1;
    SliceChain chain;
    std::mutex err_mu;
    std::atomic<uint32_t> next{0};
    int first_rc = TSGPU_OK;
    std::string first_err;
    const std::function<void()> job = [&]() {
        for (;;) {
            const uint32_t si = next.fetch_add(1);
            if (si >= n_slices) break;
            const uint32_t a = start[si], n = start[si + 1] - a;
            const size_t at = (size_t)a * out->k_stride;
            tsgpu_hits h = *out;
            h.keys = out->keys + at; h.scores = out->scores + at * 3; h.n_hits = out->n_hits + a; h.status = out->status + a;
            if (out->text_match) h.text_match = out->text_match + at;
            if (out->vector_distance) h.vector_distance = out->vector_distance + at;
            if (out->match_score_index) h.match_score_index = out->match_score_index + at;
            if (out->num_matched) h.num_matched = out->num_matched + a;
            if (out->search_cutoff) h.search_cutoff = out->search_cutoff + a;
            BatchOpts bo;
            bo.record_last = false;
            bo.chain = &chain;
            bo.chain_index = si;
            int rc;
            { LaneLock ll(ctx); rc = kw_batch_on_lane(ctx, *ll.L, queries + a, n, &h, bo); }
            if (rc != TSGPU_OK) { std::lock_guard<std::mutex> lk(err_mu); if (first_rc == TSGPU_OK) { first_rc = rc; first_err = tls_error(); } }
        }
    };
    // one host thread (and lane) per slice: every slice is planned at once, enqueued in order, and waits for / copies out its own results
    try { ctx->split_pool.run(job, std::min<uint32_t>(n_slices, (uint32_t)ctx->n_lanes) - 1); } catch (const std::bad_alloc&) { return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_keyword_search_batch: host allocation failed"); }
    if (first_rc != TSGPU_OK) return fail(first_rc, first_err);
    return ok();
}

static int kw_dispatch(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, bool wildcard, tsgpu_id_lists** ids_out, DevBuf* ids_dev, bool* ids_dev_done,
                       const uint16_t* present_elsewhere) {
    if (ids_dev_done) *ids_dev_done = false;
    if (!ctx || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_batch: NULL argument");
    if (n_queries == 0) { if (ids_out) { *ids_out = new (std::nothrow) tsgpu_id_lists; if (*ids_out) (*ids_out)->begin.assign(1, 0); } return ok(); }
    if (!queries) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_batch: queries is NULL");
    if (!out->keys || !out->scores || !out->n_hits || !out->status) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_batch: missing output arrays");
    struct CallerCount { std::atomic<int>& c; explicit CallerCount(std::atomic<int>& x) : c(x) { c.fetch_add(1); } ~CallerCount() { c.fetch_sub(1); } } cc(ctx->kw_callers);
    const bool legacy_keep = ctx->keep_ids;
    if (!wildcard && !legacy_keep && !ids_dev && !present_elsewhere && !tsgpu::tls_no_coalesce() && out->mem == TSGPU_MEM_HOST && n_queries <= ctx->batch_max_queries && ctx->kw_callers.load() > 1)
        return kw_coalesced(ctx, queries, n_queries, out, ids_out);
    // a batch with a vector-query sort key runs under ctx->mu (tsgpu_host.h), taken before its lane; it is served as ONE batch (the slices of a split batch run on
    // threads of their own)
    CtxMuForVectorKeys vq_hold;
    const bool vq = ctx->sort_keys_live.load(std::memory_order_relaxed) != 0 && names_vector_query_key(queries, n_queries);
    if (vq) vq_hold.take(ctx);
    if (!vq && !wildcard && !legacy_keep && !ids_out && !present_elsewhere && out->mem == TSGPU_MEM_HOST && ctx->kw_host_split_queries && ctx->n_lanes >= 2 &&
        (uint64_t)n_queries >= 4ull * ctx->kw_host_split_queries)
        return kw_split_host(ctx, queries, n_queries, out);
    std::unique_ptr<tsgpu_id_lists> lists;
    if (ids_out) { lists.reset(new (std::nothrow) tsgpu_id_lists); if (!lists) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_keyword_search_batch_ids: host allocation failed"); }
    BatchOpts bo;
    bo.wildcard = wildcard;
    bo.keep_ids = legacy_keep || ids_out != nullptr;
    bo.id_lists = lists.get();
    bo.ids_dev = lists ? ids_dev : nullptr; bo.ids_dev_done = ids_dev_done;
    bo.record_last = legacy_keep;
    bo.present_elsewhere = present_elsewhere;
    LaneLock ll(ctx, legacy_keep ? 0 : (tsgpu::tls_avoid_lane0() ? -2 : -1));          // the legacy "last batch" id API is single-caller: always lane 0
    vq_hold.stream = ll.L->stream;
    const int rc = kw_batch_on_lane(ctx, *ll.L, queries, n_queries, out, bo);
    if (rc == TSGPU_OK && ids_out) *ids_out = lists.release();
    return rc;
}

// Waits for everything enqueued on the lane's stream WITHOUT burning a CPU: hipEventSynchronize on a hipEventBlockingSync event still
// spins inside the HSA runtime for most of a small round (19 % of the process's CPU time under 256 callers, profiles/r03/
// sigprof_256threads_before.txt), and with many request threads on a CPU quota that time is the throughput. Sleep for most of the
// lane's usual wait, then poll the event between short sleeps (timer slack lowered for the sleeps: the default 50 us would triple them).
static hipError_t sleeping_wait(KwLane& L, hipStream_t s) {
    hipError_t e = hipEventRecord(L.ev_block, s);
    if (e != hipSuccess) return e;
    const uint64_t t0 = now_us();
#if defined(__linux__)
    const int slack = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    auto nap = [](uint64_t us) { timespec ts; ts.tv_sec = 0; ts.tv_nsec = (long)(us * 1000); (void)nanosleep(&ts, nullptr); };
    if (L.wait_ema_us > 40) nap(std::min<uint64_t>(L.wait_ema_us * 6 / 10, 2000));
    while ((e = hipEventQuery(L.ev_block)) == hipErrorNotReady) nap(15);
    if (slack > 0) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)slack, 0, 0, 0);
#else
    e = hipEventSynchronize(L.ev_block);
#endif
    const uint64_t w = now_us() - t0;
    L.wait_ema_us = (L.wait_ema_us * 7 + w) / 8;
    return e;
}

}  // extern "C"

// ---- the keyword batch executor: kw_batch_on_lane() below runs these phases in order ----
namespace {
// big batches of plain single-field queries: the plan is made on the device (three small kernels, one read-back) instead of ~0.5 ms of
// host threads; any other shape — and anything the device planner hands back — goes through plan_batch()
bool device_plan_applies(const tsgpu_ctx* ctx, const BatchOpts& bo, bool keep_ids, uint32_t n_queries) {
    if (bo.wildcard || bo.present_elsewhere || bo.vflat) return false;
    // (batches that keep the matched ids: only when nobody reads the segments back per query — the candidate call marks its id sets from the device tables)
    if (keep_ids && (bo.record_last || bo.id_lists)) return false;
    // (not for the chained slices of a sliced host delivery: there the host plans slice i + 1 WHILE slice i runs, and a planning kernel on the
    //  second lane would wait behind the running find kernel for a place on the chip — measured: 10.05 -> 10.18 ms per 10 000 queries)
    if (bo.chain && !(bo.chain_index == 0 && ctx->kw_host_split_device_plan)) return false;
    return ctx->kw_two_kernels && ctx->kw_device_plan_min_queries && n_queries >= ctx->kw_device_plan_min_queries;
}

// single-field tables (<= 3 tokens / up to 10 tokens) and multi-field tables: find + score kernels when the hit buffer fits, else the
// fused kernel. A work item can yield at most one hit per driver id, so its segment of the hit buffer holds (blk_end - blk_begin) * 256
// records of 1 + TMAX words; the items run in groups whose segments fit the budget.
struct TablePlan { bool two = false; std::vector<uint64_t> hoff; std::vector<size_t> group_start{0}; uint64_t need = 0, records = 0; size_t rec_bytes = 0; };
TablePlan group_hit_segments(const KwWorkItem* tab, size_t nws, size_t rec_bytes, uint64_t budget) {
    TablePlan tp;
    tp.rec_bytes = rec_bytes;
    auto records_of = [&](size_t i) { return (uint64_t)(tab[i].blk_end - tab[i].blk_begin) * BLOCK_IDS; };
    for (size_t i = 0; i < nws; i++) { budget = std::max(budget, records_of(i)); tp.records += records_of(i); }
    tp.hoff.resize(nws);
    uint64_t used = 0;
    for (size_t i = 0; i < nws; i++) {
        const uint64_t c = records_of(i);
        if (used + c > budget) { tp.group_start.push_back(i); used = 0; }
        tp.hoff[i] = used; used += c; tp.need = std::max(tp.need, used);
    }
    tp.group_start.push_back(nws);
    tp.two = tp.group_start.size() <= 3;          // each group drains the chip between its two kernels: beyond two groups the fused kernel wins
    return tp;
}
// the four kernel tables + the wildcard table of a batch: items per table, hit-buffer groups, hit records of the batch
struct HitTables {
    TablePlan tp[4]; size_t n[5], first[6] = {0}; uint64_t records = 0;      // (first: a table's place in the concatenation; first[5] = all work items)
    std::vector<uint32_t> oc_jobs[2];                                        // queries of the two multi-field tables that kw_mf_ordered_count_kernel counts
};
// force_two (the phrase front: its mark kernel needs the records): the two-kernel form whatever the number of hit-buffer groups
int plan_hit_tables(const tsgpu_ctx* ctx, KwLane& L, Plan& P, const DevPlan& DP, HitTables& H, bool force_two = false) {
    for (int tb = 0; tb < 5; tb++) { H.n[tb] = DP.on && tb < 2 ? DP.n_work[tb] : P.n_tab[tb]; H.first[tb + 1] = H.first[tb] + H.n[tb]; }
    for (int tb = 0; tb < 4; tb++) {
        if (!H.n[tb] || !ctx->kw_two_kernels) continue;
        TablePlan& tp = H.tp[tb];
        const size_t rec_bytes = (size_t)((tb & 1 ? KW_MAX_TOKENS : 3) * (tb >= 2 ? KW_MAX_FIELDS : 1) + 1) * 4;
        if (DP.on) {                                    // the device planner's two tables: one group each (it checked the budget), offsets already on the device
            tp.two = true; tp.rec_bytes = rec_bytes; tp.group_start = {0, H.n[tb]};
            tp.need = tp.records = DP.hit_blocks[tb] * (uint64_t)BLOCK_IDS;
            if (int rc = L.d_hits.reserve(std::max<uint64_t>(tp.need, 1) * rec_bytes)) return rc;
        } else {
            tp = group_hit_segments(P.work.data() + H.first[tb], H.n[tb], rec_bytes, hit_budget_records(ctx, rec_bytes));
            if (force_two) { tp.two = true; if (int rc = L.d_hits.reserve(std::max<uint64_t>(tp.need, 1) * rec_bytes)) return rc; }
            else if (tp.two && L.d_hits.reserve(std::max<uint64_t>(tp.need, 1) * rec_bytes)) { (void)hipGetLastError(); tp.two = false; }      // no room for the hit buffer: the fused kernel needs none
            if (!tp.two) tp.hoff.clear();
        }
        H.records += tp.records;
    }
    // multi-field queries with filter + excluded ids: counted from the hit records of ONE find launch of their table; a table that was
    // cut into groups or runs fused cannot serve them -> 501 for those queries (their hits are not reported)
    for (uint32_t qi : P.ordered_count_q) {
        const int tb = P.q[qi].n_lists <= 3 ? 0 : 1;
        const TablePlan& tp = H.tp[2 + tb];
        if (tp.two && tp.group_start.size() == 2) H.oc_jobs[tb].push_back(qi);
        else if (P.status[qi] == TSGPU_OK) P.status[qi] = TSGPU_ERR_UNSUPPORTED;
    }
    return TSGPU_OK;
}

// TESTS ONLY, option kw_plan_digest: the digests of this batch's plan (kw_plan_digest.h); the device planner's tables are read back for it
int record_plan_digest(tsgpu_ctx* ctx, hipStream_t s, const Plan& P, const DevPlan& DP, const std::vector<KwWorkItem>& work, const HitTables& H, uint32_t n_queries) {
    KwPlanTables t;
    std::vector<KwQueryDev> q_dev; std::vector<KwWorkItem> w_dev; std::vector<uint64_t> hoff_dev;
    if (DP.on) {
        q_dev.resize(n_queries); w_dev.resize(H.first[5]); hoff_dev.resize(H.first[5]);
        TSGPU_HIP_TRY(hipStreamSynchronize(s));
        TSGPU_HIP_TRY(hipMemcpy(q_dev.data(), DP.dq, (size_t)n_queries * sizeof(KwQueryDev), hipMemcpyDeviceToHost));
        if (H.first[5]) TSGPU_HIP_TRY(hipMemcpy(w_dev.data(), DP.dw, H.first[5] * sizeof(KwWorkItem), hipMemcpyDeviceToHost));
        if (H.first[5]) TSGPU_HIP_TRY(hipMemcpy(hoff_dev.data(), DP.hoff, H.first[5] * 8, hipMemcpyDeviceToHost));
    }
    t.q = DP.on ? q_dev.data() : P.q.data(); t.status = P.status.data(); t.n_queries = n_queries;
    t.mf = P.mf.data(); t.work = DP.on ? w_dev.data() : work.data();
    t.groups = P.groups.data(); t.n_groups = P.groups.size();
    for (int tb = 0; tb < 5; tb++) t.n_tab[tb] = H.n[tb];
    for (int tb = 0; tb < 4; tb++) {
        t.hoff[tb] = DP.on ? hoff_dev.data() + H.first[tb] : H.tp[tb].hoff.data();
        t.n_hoff[tb] = DP.on ? (H.tp[tb].two ? H.n[tb] : 0) : H.tp[tb].hoff.size();
    }
    uint64_t cut, layout;
    kw_plan_digests(t, cut, layout);
    std::lock_guard<std::mutex> tl(ctx->tm_mu);
    ctx->kw_last_plan_cut_digest = cut; ctx->kw_last_plan_layout_digest = layout;
    return TSGPU_OK;
}

// the device-side tables of one batch: staging produces them, the launch, delivery and id-list phases consume them
struct KwStaged {
    const KwQueryDev* dq = nullptr; const KwWorkItem* dw = nullptr; const uint32_t* daux = nullptr; const KwQueryMF* mf = nullptr;
    const uint64_t* hoff[4] = {nullptr, nullptr, nullptr, nullptr};         // per kernel table: its work items' offsets into the hit buffer
    const KwMergeGroup* groups = nullptr; const uint32_t* oc_jobs[2] = {nullptr, nullptr};
    KwPartials part; KwOut o; uint32_t* ids_out = nullptr;
};

// ---- the plan travels in ONE pinned staging buffer and ONE host-to-device copy (queries, work items, aux ids, multi-field
//      descriptors, hit-record offsets): a pageable source costs a staged synchronous copy per call, five calls per batch ----
int upload_plan_image(KwLane& L, hipStream_t s, const Plan& P, const DevPlan& DP, const HitTables& H, KwStaged& T) {
    const std::vector<KwWorkItem>& work = P.work;
    Placer place;
    const size_t at_q = place(P.q.size() * sizeof(KwQueryDev)), at_w = place(work.size() * sizeof(KwWorkItem)), at_aux = place(P.aux.size() * 4),
                 at_mf = place(P.mf.size() * sizeof(KwQueryMF));
    size_t at_hoff[4];
    for (int tb = 0; tb < 4; tb++) at_hoff[tb] = place(H.tp[tb].hoff.size() * 8);
    const size_t at_grp = place(P.groups.size() * sizeof(KwMergeGroup));
    const size_t at_oc[2] = {place(H.oc_jobs[0].size() * 4), place(H.oc_jobs[1].size() * 4)};
    if (!DP.on) {
        int rc;
        if ((rc = L.h_plan.reserve(place.bytes + 64)) || (rc = L.d_plan.reserve(place.bytes + 64))) return rc;
        uint8_t* hp = (uint8_t*)L.h_plan.p;
        auto put = [&](size_t at, const void* src, size_t bytes) { if (bytes) memcpy(hp + at, src, bytes); };
        put(at_q, P.q.data(), P.q.size() * sizeof(KwQueryDev)); put(at_w, work.data(), work.size() * sizeof(KwWorkItem));
        put(at_aux, P.aux.data(), P.aux.size() * 4); put(at_mf, P.mf.data(), P.mf.size() * sizeof(KwQueryMF));
        for (int tb = 0; tb < 4; tb++) put(at_hoff[tb], H.tp[tb].hoff.data(), H.tp[tb].hoff.size() * 8);
        put(at_grp, P.groups.data(), P.groups.size() * sizeof(KwMergeGroup));
        for (int tb = 0; tb < 2; tb++) put(at_oc[tb], H.oc_jobs[tb].data(), H.oc_jobs[tb].size() * 4);
        TSGPU_HIP_TRY(hipMemcpyAsync(L.d_plan.p, hp, place.bytes, hipMemcpyHostToDevice, s));
    }
    const uint8_t* const dplan = (const uint8_t*)L.d_plan.p;
    T.dq = DP.on ? DP.dq : (const KwQueryDev*)(dplan + at_q); T.dw = DP.on ? DP.dw : (const KwWorkItem*)(dplan + at_w);
    T.daux = DP.on ? DP.daux : (const uint32_t*)(dplan + at_aux); T.mf = (const KwQueryMF*)(dplan + at_mf);
    for (int tb = 0; tb < 4; tb++) T.hoff[tb] = DP.on ? DP.hoff + H.first[tb] : (const uint64_t*)(dplan + at_hoff[tb]);
    T.groups = (const KwMergeGroup*)(dplan + at_grp);
    for (int tb = 0; tb < 2; tb++) T.oc_jobs[tb] = (const uint32_t*)(dplan + at_oc[tb]);
    return TSGPU_OK;
}

// ---- scratch: pw partial lists of k_stride slots (one per work item + one per merge group) ----
int reserve_partials(KwLane& L, size_t pw, uint32_t KS, KwPartials& part) {
    int rc;
    const size_t slots = pw * KS * 8;
    if ((rc = L.d_part_s0.reserve(slots)) || (rc = L.d_part_s1.reserve(slots)) || (rc = L.d_part_s2.reserve(slots)) || (rc = L.d_part_key.reserve(slots))) return rc;
    if ((rc = L.d_part_cnt.reserve(pw * 4)) || (rc = L.d_part_nm.reserve(pw * 4)) || (rc = L.d_part_ne.reserve(pw * 4)) || (rc = L.d_part_ow.reserve(pw * 8)) || (rc = L.d_part_f.reserve(pw * 16))) return rc;
    part.s0 = L.d_part_s0.as<int64_t>(); part.s1 = L.d_part_s1.as<int64_t>(); part.s2 = L.d_part_s2.as<int64_t>();
    part.key = L.d_part_key.as<int64_t>(); part.cnt = L.d_part_cnt.as<uint32_t>(); part.n_match = L.d_part_nm.as<uint32_t>();
    part.n_emit = L.d_part_ne.as<uint32_t>(); part.off_words = L.d_part_ow.as<uint64_t>(); part.k_stride = KS;
    part.n_match1 = L.d_part_f.as<uint32_t>(); part.first_rank = part.n_match1 + pw; part.last_rank = part.first_rank + pw; part.fflags = part.last_rank + pw;
    return TSGPU_OK;
}
KwPartials shifted(KwPartials pb, size_t sh) {             // every kernel indexes the partials by its own blockIdx: shift the bases
    const size_t KS = pb.k_stride;
    pb.s0 += sh * KS; pb.s1 += sh * KS; pb.s2 += sh * KS; pb.key += sh * KS;
    pb.cnt += sh; pb.n_match += sh; pb.n_emit += sh; pb.off_words += sh;
    pb.n_match1 += sh; pb.first_rank += sh; pb.last_rank += sh; pb.fflags += sh;
    return pb;
}

// host outputs: ONE device image [n_hits | num_matched | off_words | keys | scores | text_match | vector_distance | msi]
// -> one device-to-host copy per batch (seven separate copies cost a small batch ~60 us of launch overhead)
struct KwResultImage {
    size_t n_queries, k_stride, n_hits = 0, num_matched, off_words, keys, scores, text_match, vector_distance, msi, bytes;
    KwResultImage(size_t n, size_t ks) : n_queries(n), k_stride(ks) {
        const size_t slots = n * ks;
        num_matched = (n * 4 + 7) & ~(size_t)7; off_words = num_matched + n * 8; keys = off_words + n * 8;
        scores = keys + slots * 8; text_match = scores + slots * 24; vector_distance = text_match + slots * 8; msi = vector_distance + ((slots * 4 + 7) & ~(size_t)7);
        bytes = msi + ((slots + 7) & ~(size_t)7);
    }
    template <class Arrays>
    void alias(uint8_t* b, Arrays& h) const {               // h's arrays point INTO the image at b (a tsgpu_hits: alias_out of the coalesced round)
        h.n_hits = (uint32_t*)(b + n_hits); h.num_matched = (uint64_t*)(b + num_matched);
        h.keys = (uint64_t*)(b + keys); h.scores = (int64_t*)(b + scores); h.text_match = (int64_t*)(b + text_match);
        h.vector_distance = (float*)(b + vector_distance); h.match_score_index = (int8_t*)(b + msi);
    }
    void bind(uint8_t* b, KwOut& o) const { alias(b, o); o.off_words = (uint64_t*)(b + off_words); }      // the kernels write the image at b
    void copy_live_rows(const uint8_t* b, const tsgpu_hits& h) const {      // the host image at b into h's arrays (the optional ones may be NULL)
        const uint32_t* nh = (const uint32_t*)(b + n_hits);
        memcpy(h.n_hits, nh, n_queries * 4);
        if (h.num_matched) memcpy(h.num_matched, b + num_matched, n_queries * 8);
        for (size_t i = 0; i < n_queries; i++) {           // only the hits: slots behind n_hits[i] are undefined in the image too
            const size_t at = i * k_stride, n = std::min<size_t>(nh[i], k_stride);
            memcpy(h.keys + at, b + keys + at * 8, n * 8);
            memcpy(h.scores + at * 3, b + scores + at * 24, n * 24);
            if (h.text_match) memcpy(h.text_match + at, b + text_match + at * 8, n * 8);
            if (h.vector_distance) memcpy(h.vector_distance + at, b + vector_distance + at * 4, n * 4);
            if (h.match_score_index) memcpy(h.match_score_index + at, b + msi + at, n);
        }
    }
};

// ---- launch: the index view of the batch, then find / score (or fused) kernels per table, wildcard scans, merge groups, merge ----
struct LaunchStats { uint32_t hit_groups = 0; bool find_marked = false; };
int launch_batch(tsgpu_ctx* ctx, KwLane& L, hipStream_t s, const Snapshot& snap, const Plan& P, const HitTables& H, const KwStaged& T, int cap, uint32_t n_queries,
                 bool timing, bool count_touched, bool vflat, LaunchStats& st, const PhraseMarkArgs* phrase = nullptr) {
    int rc;
    IndexView v = make_view(ctx, snap);
    v.mf = T.mf;
    if (P.fbits_words) {
        if ((rc = L.d_fbits.reserve(P.fbits_words * 4))) return rc;
        TSGPU_HIP_TRY(hipMemsetAsync(L.d_fbits.p, 0, P.fbits_words * 4, s));
    }
    v.fbits = L.d_fbits.as<uint32_t>();
    if ((rc = L.d_t0.reserve(64))) return rc;
    v.t0 = L.d_t0.as<long long>(); v.ticks_per_us = ctx->ticks_per_us;
    if (P.any_deadline) {
        if ((rc = L.d_cut.reserve((size_t)n_queries * 4))) return rc;
        TSGPU_HIP_TRY(hipMemsetAsync(L.d_cut.p, 0, (size_t)n_queries * 4, s));
        hipLaunchKernelGGL(kw_stamp_kernel, dim3(1), dim3(1), 0, s, L.d_t0.as<long long>());       // the queries' budgets count from here
    }
    v.cutoff = L.d_cut.as<uint32_t>();
    if (count_touched) {                         // measurement option: the find kernel's COUNT instantiation adds the bytes it requests here
        if ((rc = L.d_touched.reserve(12 * 8))) return rc;
        TSGPU_HIP_TRY(hipMemsetAsync(L.d_touched.p, 0, 12 * 8, s));
        v.touched = L.d_touched.as<unsigned long long>();
    }
    const KwQueryDev* dq = T.dq; const KwWorkItem* dw = T.dw; const uint32_t* daux = T.daux; uint32_t* ids_out = T.ids_out;
    if (timing) TSGPU_HIP_TRY(hipEventRecord(L.ev[0], s));
    bool phrase_fused = false;
    auto run_table = [&](int tb, auto tmax_tag, auto mf_tag) {
        constexpr int TM = decltype(tmax_tag)::value;
        constexpr bool MFT = decltype(mf_tag)::value;
        const size_t nws = H.n[tb], first = H.first[tb];
        const TablePlan& tp = H.tp[tb];
        if (nws == 0) return;
        if (tp.two) {
            st.hit_groups += (uint32_t)tp.group_start.size() - 1;
            for (size_t gi = 0; gi + 1 < tp.group_start.size(); gi++) {
                const size_t a = tp.group_start[gi], b = tp.group_start[gi + 1];
                if (b <= a) continue;
                if constexpr (MFT) {
                    MfOrderedCount oc;
                    if (!H.oc_jobs[tb - 2].empty() && tp.group_start.size() == 2) {
                        oc.jobs = T.oc_jobs[tb - 2]; oc.n_jobs = (uint32_t)H.oc_jobs[tb - 2].size(); oc.table_first = (uint32_t)first;
                        oc.work_all = dw; oc.part_all = T.part;
                    }
                    const int mf_pipe = !ctx->kw_mf_pipelined ? 0 : (P.mf_max_fields <= 2 ? 2 : (P.mf_max_fields <= 4 ? 4 : 0));
                    if (mf_pipe) ctx->kw_mf_pipelined_launches++;
                    launch_find_score_mf<TM>(cap, s, (uint32_t)(b - a), v, dq, dw + first + a, shifted(T.part, first + a), daux, ids_out, L.d_hits.as<uint32_t>(), T.hoff[tb] + a, oc, !P.any_aux && !P.any_array, mf_pipe, P.any_vq, phrase);
                }
                else {
                    const bool mark = !st.find_marked;
                    st.find_marked = true;
                    launch_find_score<TM>(cap, s, (uint32_t)(b - a), v, dq, dw + first + a, shifted(T.part, first + a), daux, ids_out, P.any_s2, L.d_hits.as<uint32_t>(), T.hoff[tb] + a, mark && timing ? L.ev[3] : nullptr, ctx->kw_pair_blocks, !P.any_aux, P.any_vq, phrase);
                }
            }
        } else if (phrase) phrase_fused = true;             // (cannot happen: plan_hit_tables(force_two))
        else if constexpr (MFT) launch_search_mf_cap<TM>(cap, s, (uint32_t)nws, v, dq, dw + first, shifted(T.part, first), daux, ids_out, P.any_vq);
        else with_cap(cap, [&](auto c) { launch_search<TM, decltype(c)::value>(s, (uint32_t)nws, v, dq, dw + first, shifted(T.part, first), daux, ids_out, P.any_s2, P.any_vq); });
    };
    run_table(0, std::integral_constant<int, 3>(), std::false_type());
    run_table(1, std::integral_constant<int, KW_MAX_TOKENS>(), std::false_type());
    run_table(2, std::integral_constant<int, 3>(), std::true_type());
    run_table(3, std::integral_constant<int, KW_MAX_TOKENS>(), std::true_type());
    if (phrase) {                                // the phrase front's find + mark launches: no partial lists, nothing to merge
        TSGPU_HIP_TRY(hipGetLastError());
        return phrase_fused ? fail(TSGPU_ERR_DEVICE, "tsgpu_phrase_search_batch: a table of AND items without hit records") : TSGPU_OK;
    }
    const size_t sh = H.first[4];
    if (H.n[4] && P.any_vq) with_cap(cap, [&](auto c) { hipLaunchKernelGGL((kw_wildcard_kernel<decltype(c)::value, true>), dim3((uint32_t)H.n[4]), dim3(KW_THREADS), 0, s, v, dq, dw + sh, shifted(T.part, sh), daux, ids_out); });
    else if (H.n[4]) with_cap(cap, [&](auto c) { hipLaunchKernelGGL((kw_wildcard_kernel<decltype(c)::value>), dim3((uint32_t)H.n[4]), dim3(KW_THREADS), 0, s, v, dq, dw + sh, shifted(T.part, sh), daux, ids_out); });
    if (timing) TSGPU_HIP_TRY(hipEventRecord(L.ev[1], s));
    if (!P.groups.empty()) with_cap(cap, [&](auto c) { hipLaunchKernelGGL((kw_merge_groups_kernel<decltype(c)::value>), dim3((uint32_t)P.groups.size()), dim3(KW_THREADS), 0, s, dq, T.part, T.groups); });
    with_cap(cap, [&](auto c) { hipLaunchKernelGGL((kw_merge_kernel<decltype(c)::value>), dim3(n_queries), dim3(KW_THREADS), 0, s, dq, T.part, T.o, ids_out, dw, ctx->kw_merge_select_min); });
    if (vflat) hipLaunchKernelGGL(kw_vflat_distance_kernel, dim3(n_queries), dim3(KW_THREADS), 0, s, dq, daux, T.o);     // KV::vector_distance of the hits
    if (timing) TSGPU_HIP_TRY(hipEventRecord(L.ev[2], s));
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}

// ---- results: device output (img == nullptr: the kernels wrote the caller's arrays), or the host image (zero-copy / staged through the lane's
//      pinned buffer) or direct copies; then status and cut-off flags, with the deadlines the kernels raised ----
int deliver(tsgpu_ctx* ctx, KwLane& L, hipStream_t s, Plan& P, const KwOut& o, const KwResultImage* img, bool zero_copy, bool alias_out, uint32_t n_queries,
            tsgpu_hits* out, std::vector<uint64_t>& off_words) {
    if (img) {
        // small results: the whole image through the pinned staging buffer (a pageable destination costs ~150 us per copy call);
        // large ones: straight to the caller's arrays (the runtime pipelines them)
        if (img->bytes <= (8u << 20)) {
            if (!zero_copy) {
                if (int rc = L.h_out.reserve(img->bytes + 64)) return rc;
                TSGPU_HIP_TRY(hipMemcpyAsync(L.h_out.p, L.d_out_keys.p, img->bytes, hipMemcpyDeviceToHost, s));
            }
            // (a spinning wait costs one CPU per lane for the whole round: with many request threads — and a CPU quota — the waiting
            //  thread sleeps on a blocking event instead: +20-40 us of latency, four CPUs back)
            if (ctx->kw_callers.load() >= ctx->blocking_sync_min_callers) TSGPU_HIP_TRY(sleeping_wait(L, s));
            else TSGPU_HIP_TRY(hipStreamSynchronize(s));
            uint8_t* hb = (uint8_t*)L.h_out.p;
            memcpy(off_words.data(), hb + img->off_words, (size_t)n_queries * 8);
            if (alias_out) img->alias(hb, *out); else img->copy_live_rows(hb, *out);
        } else {
            const size_t slots = (size_t)n_queries * o.k_stride;
            TSGPU_HIP_TRY(hipMemcpyAsync(out->n_hits, o.n_hits, (size_t)n_queries * 4, hipMemcpyDeviceToHost, s));
            if (out->num_matched) TSGPU_HIP_TRY(hipMemcpyAsync(out->num_matched, o.num_matched, (size_t)n_queries * 8, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(out->keys, o.keys, slots * 8, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(out->scores, o.scores, slots * 24, hipMemcpyDeviceToHost, s));
            if (out->text_match) TSGPU_HIP_TRY(hipMemcpyAsync(out->text_match, o.text_match, slots * 8, hipMemcpyDeviceToHost, s));
            if (out->vector_distance) TSGPU_HIP_TRY(hipMemcpyAsync(out->vector_distance, o.vector_distance, slots * 4, hipMemcpyDeviceToHost, s));
            if (out->match_score_index) TSGPU_HIP_TRY(hipMemcpyAsync(out->match_score_index, o.match_score_index, slots, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(off_words.data(), o.off_words, (size_t)n_queries * 8, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipStreamSynchronize(s));
        }
        for (uint32_t i = 0; i < n_queries; i++) out->status[i] = P.status[i];
        if (out->search_cutoff) for (uint32_t i = 0; i < n_queries; i++) out->search_cutoff[i] = P.cutoff[i];
    } else {
        TSGPU_HIP_TRY(hipMemcpyAsync(out->status, P.status.data(), (size_t)n_queries * 4, hipMemcpyHostToDevice, s));
        if (out->search_cutoff) TSGPU_HIP_TRY(hipMemcpyAsync(out->search_cutoff, P.cutoff.data(), (size_t)n_queries * 4, hipMemcpyHostToDevice, s));
        TSGPU_HIP_TRY(hipMemcpyAsync(off_words.data(), o.off_words, (size_t)n_queries * 8, hipMemcpyDeviceToHost, s));
        TSGPU_HIP_TRY(hipStreamSynchronize(s));
    }
    if (P.any_deadline) {                        // work items that ran out of time raised their query's flag: partial hits + search_cutoff
        std::vector<uint32_t> cut(n_queries);
        TSGPU_HIP_TRY(hipMemcpy(cut.data(), L.d_cut.p, (size_t)n_queries * 4, hipMemcpyDeviceToHost));
        bool any = false;
        for (uint32_t i = 0; i < n_queries; i++) if (cut[i]) { P.cutoff[i] = 1; any = true; }
        if (any && out->search_cutoff) {
            if (!img) TSGPU_HIP_TRY(hipMemcpy(out->search_cutoff, P.cutoff.data(), (size_t)n_queries * 4, hipMemcpyHostToDevice));
            else for (uint32_t i = 0; i < n_queries; i++) out->search_cutoff[i] = P.cutoff[i];
        }
    }
    return TSGPU_OK;
}

// sort keys of query i that read a column value per match (the device planner leaves P.q on the device: the caller's query tells)
uint32_t n_column_sort_keys(const Plan& P, bool dev_plan, const tsgpu_kw_query* queries, uint32_t i) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < (dev_plan ? queries[i].n_sort : P.q[i].n_sort); k++) n += sort_kind_reads_key(dev_plan ? queries[i].sort[k].kind : P.q[i].sort_kind[k]) ? 1 : 0;
    return n;
}

// ---- bookkeeping: timings + algorithmic bytes; num_matched = the host's counts (nullptr: device output, or not asked for) ----
void record_timings(tsgpu_ctx* ctx, KwLane& L, bool timing, const LaunchStats& st, uint64_t hit_records, const Plan& P, bool dev_plan, const tsgpu_kw_query* queries,
                    const std::vector<uint64_t>& off_words, const uint64_t* num_matched) {
    float ms_a = 0, ms_b = 0, ms_find = 0;
    if (timing) { (void)hipEventElapsedTime(&ms_a, L.ev[0], L.ev[1]); (void)hipEventElapsedTime(&ms_b, L.ev[1], L.ev[2]); }
    if (timing && st.find_marked && st.hit_groups == 1) (void)hipEventElapsedTime(&ms_find, L.ev[0], L.ev[3]);       // one find launch, then one score launch
    uint64_t bytes = P.list_bytes;
    for (uint32_t i = 0; i < off_words.size(); i++) bytes += 4ull * off_words[i] + (num_matched ? 8ull * num_matched[i] * n_column_sort_keys(P, dev_plan, queries, i) : 0);
    std::lock_guard<std::mutex> tl(ctx->tm_mu);
    ctx->timings.kw_search_ms = ms_a; ctx->timings.kw_merge_ms = ms_b; ctx->timings.kw_find_ms = ms_find; ctx->timings.total_ms = ms_a + ms_b;
    ctx->timings.kw_algorithmic_bytes = bytes;
    ctx->kw_last_hit_groups = st.hit_groups; ctx->kw_last_hit_records = hit_records;
}

// measurement option kw_count_touched: the bytes the find kernel counted + the score kernel's, computed from the counts of matches
int record_touched(tsgpu_ctx* ctx, KwLane& L, const Plan& P, bool dev_plan, const tsgpu_kw_query* queries, uint32_t n_queries, const uint64_t* nm, const uint64_t* nm_dev) {
    uint64_t c[12];
    TSGPU_HIP_TRY(hipMemcpy(c, L.d_touched.p, sizeof(c), hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> tl(ctx->tm_mu);
    ctx->kw_find_dir_items = c[7]; ctx->kw_find_pairs = c[8]; ctx->kw_find_dir_pairs = c[9]; ctx->kw_find_dir_wide_pairs = c[10];
    tsgpu_kw_touched& tt = ctx->kw_touched;
    tt.find_driver_ids = c[0]; tt.find_metadata = c[1]; tt.find_tile_dma = c[2]; tt.find_probes = c[3]; tt.find_records = c[4];
    tt.find_work_items = c[5]; tt.find_hit_records = c[6];
    tt.find_requested_bytes = c[0] + c[1] + c[2] + c[3] + c[4];
    // the score kernel's requests per hit record are fixed sizes (kw_score_kernel / load_runs_staged): the record itself, per token one
    // BlockMeta (32 B), the offset_index pair (one 8-byte window; TSGPU_LIST_TABLE=0: two) and the first offsets (8 B); per numeric sort key one column
    // value; the rare third.. occurrence of a token in a document and the second window of an offset_index wider than 16 bits (one more 8-byte fetch
    // each) are not counted
    uint64_t sb = 0;
    std::vector<uint64_t> nm_host;
    if (nm_dev) {                                            // (measurement only: one small read-back)
        nm_host.resize(n_queries);
        if (hipMemcpy(nm_host.data(), nm_dev, (size_t)n_queries * 8, hipMemcpyDeviceToHost) == hipSuccess) nm = nm_host.data();
    }
    for (uint32_t i = 0; nm && !dev_plan && i < n_queries; i++)
        sb += nm[i] * (4ull * ((P.q[i].n_lists <= 3 ? 3 : KW_MAX_TOKENS) + 1) + (KW_LIST_TABLE ? 48ull : 56ull) * P.q[i].n_lists +8ull * n_column_sort_keys(P, dev_plan, queries, i));
    tt.score_requested_bytes = sb;
    return TSGPU_OK;
}

// ---- matched ids (id_buff / all_result_ids, src/index.cpp:5549, 5565): every work item left an ascending segment ----
// legacy single-caller API (tsgpu_result_ids): remember where the segments live (ne: the work items' emitted counts; empty = no ids kept)
void record_last_ids(KwLane& L, const Plan& P, const std::vector<KwWorkItem>& work, const std::vector<uint32_t>& ne, uint32_t n_queries) {
    L.last_ids_off.assign(n_queries, 0); L.last_ids_unsorted.assign(n_queries, 0);
    L.last_chunk_emit.assign(n_queries, {}); L.last_chunk_off.assign(n_queries, {});
    for (uint32_t i = 0; !ne.empty() && i < n_queries; i++) {
        if (P.status[i] != TSGPU_OK || P.q[i].n_work == 0) continue;
        L.last_ids_off[i] = P.q[i].ids_out_off;
        L.last_chunk_emit[i].assign(ne.begin() + P.q[i].first_work, ne.begin() + P.q[i].first_work + P.q[i].n_work);
        L.last_chunk_off[i].resize(P.q[i].n_work);
        for (uint32_t c = 0; c < P.q[i].n_work; c++) L.last_chunk_off[i][c] = work[P.q[i].first_work + c].ids_out_off;
        L.last_ids_unsorted[i] = P.q[i].mf_index != KW_NONE;      // several driver lists: segments are sorted, their union is not
    }
}
// per-call id lists: the segments are gathered into one dense array on the device (one launch, one download) and belong
// to THIS call — concurrent callers never see each other's ids
int build_id_lists(KwLane& L, hipStream_t s, const Plan& P, const std::vector<KwWorkItem>& work, const std::vector<uint32_t>& ne, const uint32_t* ids_out, uint32_t n_queries,
                   tsgpu_id_lists& il, DevBuf* ids_dev, bool* ids_dev_done) {
    il.begin.assign((size_t)n_queries + 1, 0);
    std::vector<KwIdCopy> segs;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_queries; i++) {
        il.begin[i] = at;
        if (P.status[i] != TSGPU_OK || P.q[i].n_work == 0) continue;
        for (uint32_t c = 0; c < P.q[i].n_work; c++) {
            const uint32_t cnt = ne[P.q[i].first_work + c];
            if (!cnt) continue;
            segs.push_back({P.q[i].ids_out_off + work[P.q[i].first_work + c].ids_out_off, at, cnt, 0u});
            at += cnt;
        }
    }
    il.begin[n_queries] = at;
    bool to_dev = ids_dev != nullptr;                 // the ids stay on the device, in the caller's buffer (several driver lists: the union is sorted on the host below)
    for (uint32_t i = 0; to_dev && i < n_queries; i++) if (P.status[i] == TSGPU_OK && P.q[i].mf_index != KW_NONE) to_dev = false;
    if (ids_dev_done) *ids_dev_done = to_dev;
    il.ids.resize(to_dev ? 0 : at);                   // (on the device: nothing to download)
    if (!at) return TSGPU_OK;
    DevBuf& dst = to_dev ? *ids_dev : L.d_idflat;
    int rc;
    if ((rc = dst.reserve(at * 4)) || (rc = upload(L.d_idseg, segs.data(), segs.size() * sizeof(KwIdCopy), s))) return rc;
    hipLaunchKernelGGL(kw_ids_gather_kernel, dim3((uint32_t)segs.size()), dim3(KW_THREADS), 0, s, ids_out, L.d_idseg.as<KwIdCopy>(), dst.as<uint32_t>());
    TSGPU_HIP_TRY(hipGetLastError());
    if (!to_dev) TSGPU_HIP_TRY(hipMemcpyAsync(il.ids.data(), dst.p, at * 4, hipMemcpyDeviceToHost, s));
    TSGPU_HIP_TRY(hipStreamSynchronize(s));           // (on the device: the consumer runs on another stream)
    for (uint32_t i = 0; !to_dev && i < n_queries; i++)                      // several driver lists (query_by over several fields): ascending union
        if (P.q[i].mf_index != KW_NONE && P.status[i] == TSGPU_OK) std::sort(il.ids.begin() + il.begin[i], il.ids.begin() + il.begin[i + 1]);
    return TSGPU_OK;
}
}  // namespace

extern "C" {
// the lane's mutex is held by the caller
static int kw_batch_on_lane(tsgpu_ctx* ctx, KwLane& L, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, const BatchOpts& bo) {
    (void)hipSetDevice(ctx->device);
    const std::shared_ptr<const Snapshot> snap_ref = ctx->snapshot();     // this batch runs on this snapshot, whatever is committed meanwhile
    const Snapshot& snap = *snap_ref;
    const bool keep_ids = bo.keep_ids || bo.id_lists != nullptr;
    hipStream_t s = L.stream;
    SliceChain::Turn chain_turn(bo.chain, bo.chain_index);     // (passes the turn on when this slice leaves, whatever happens to it)
    if (ctx->sort_keys_live.load(std::memory_order_relaxed) && names_vector_query_key(queries, n_queries)) {
        // vector-query sort keys read their field as it is now; whoever sent the batch here took ctx->mu for it (kw_dispatch, kw_coalesced, the candidates and grouped calls)
        if (!tls_holds_ctx_mu()) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_keyword_search_batch: a vector-query sort key on a path that does not hold the index lock");
        if (const int rc = refresh_vector_query_keys(ctx, queries, n_queries)) return rc;
    }
    try {
        static const bool host_timing = getenv("TSGPU_HOST_TIMING") != nullptr;      // diagnostics: host phases of the call on stderr
        const uint64_t t_enter = now_us();
        Plan P; DevPlan DP;
        int rc;
        if (device_plan_applies(ctx, bo, keep_ids, n_queries)) {
            if ((rc = plan_batch_device(ctx, L, snap, queries, n_queries, P, DP, s))) return rc;
            if (DP.on) ctx->kw_device_plans.fetch_add(1); else ctx->kw_device_plan_fallbacks.fetch_add(1);
            if (DP.on && keep_ids) P.ids_total = (DP.hit_blocks[0] + DP.hit_blocks[1]) * (uint64_t)BLOCK_IDS;
        }
        if (!DP.on && (rc = plan_batch(ctx, snap, queries, n_queries, P, keep_ids, bo.wildcard, bo.vflat, bo.present_elsewhere, bo.wild_ids_dev, bo.wild_tm_dev))) return rc;
        const uint64_t t_planned = now_us();
        if (out->k_stride < P.max_k) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_batch: k_stride smaller than the largest topster_size");
        const uint32_t KS = out->k_stride;
        const int cap = P.max_k + KW_THREADS <= 512 ? 512 : (P.max_k + KW_THREADS <= 1024 ? 1024 : 2048);

        // ---- staging: hit-buffer groups, the plan image, scratch, the outputs ----
        P.aux.push_back(0);
        HitTables H;
        if ((rc = plan_hit_tables(ctx, L, P, DP, H))) return rc;
        if (ctx->kw_plan_digest && (rc = record_plan_digest(ctx, s, P, DP, P.work, H, n_queries))) return rc;
        const uint32_t n_work = (uint32_t)H.first[5];
        KwStaged T;
        if ((rc = upload_plan_image(L, s, P, DP, H, T))) return rc;
        L.last_tab_q = T.dq; L.last_tab_w = T.dw; L.last_tab_n_work = n_work;
        if ((rc = reserve_partials(L, (size_t)std::max<uint32_t>(n_work, 1) + P.groups.size(), KS, T.part))) return rc;
        if (keep_ids) {
            if ((rc = L.d_ids_out.reserve(std::max<uint64_t>(P.ids_total, 1) * 4))) return rc;
            T.ids_out = L.d_ids_out.as<uint32_t>();
        }
        T.o.k_stride = KS;
        const KwResultImage img(n_queries, KS);
        const bool dev_out = out->mem == TSGPU_MEM_DEVICE;
        // a SMALL round's merge kernel writes the image straight into the lane's pinned host buffer (device-visible, coherent): no
        // device-to-host copy kernel (4-25 us) and no launch gap (~6 us) behind the merge; only the hits themselves cross the link
        const bool zero_copy = !dev_out && img.bytes <= (8u << 20) && n_queries <= ctx->kw_zero_copy_max_queries;
        if (dev_out) {
            if (!out->text_match || !out->vector_distance || !out->match_score_index || !out->num_matched)
                return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_batch: device output needs every tsgpu_hits array");
            if ((rc = L.d_out_ow.reserve((size_t)n_queries * 8))) return rc;
            T.o.keys = out->keys; T.o.scores = out->scores; T.o.text_match = out->text_match; T.o.vector_distance = out->vector_distance;
            T.o.match_score_index = out->match_score_index; T.o.n_hits = out->n_hits; T.o.num_matched = out->num_matched; T.o.off_words = L.d_out_ow.as<uint64_t>();
        } else {
            if (zero_copy) { if ((rc = L.h_out.reserve(img.bytes + 64))) return rc; }
            else if ((rc = L.d_out_keys.reserve(img.bytes))) return rc;
            img.bind(zero_copy ? (uint8_t*)L.h_out.p : (uint8_t*)L.d_out_keys.p, T.o);
        }

        // ---- launch ----
        if (bo.chain) {
            chain_turn.wait_turn();
            if (bo.chain->last) TSGPU_HIP_TRY(hipStreamWaitEvent(s, bo.chain->last, 0));
        }
        const uint64_t t_uploaded = now_us();
        const bool timing = bo.timing && n_queries >= ctx->kw_timing_min_queries;      // (each record is a marker packet in the stream: ~2 us of a small round)
        const bool count_touched = ctx->kw_count_touched;
        LaunchStats st;
        if ((rc = launch_batch(ctx, L, s, snap, P, H, T, cap, n_queries, timing, count_touched, bo.vflat != nullptr, st))) return rc;
        if (bo.chain) { TSGPU_HIP_TRY(hipEventRecord(L.ev_chain, s)); bo.chain->last = L.ev_chain; SliceChain* cc = bo.chain; chain_turn.pass(); cc->cv.notify_all(); }
        const uint64_t t_launched = now_us();

        // ---- results ----
        std::vector<uint64_t> off_words(n_queries);
        if ((rc = deliver(ctx, L, s, P, T.o, dev_out ? nullptr : &img, zero_copy, bo.alias_out, n_queries, out, off_words))) return rc;
        if (bo.status_host) bo.status_host->assign(P.status.begin(), P.status.end());
        if (bo.cutoff_host) bo.cutoff_host->assign(P.cutoff.begin(), P.cutoff.end());
        const uint64_t t_synced = now_us();

        // ---- bookkeeping, the measurement read-back, the matched ids ----
        const uint64_t* nm_host = dev_out ? nullptr : out->num_matched;
        if (timing || bo.timing) record_timings(ctx, L, timing, st, H.records, P, DP.on, queries, off_words, nm_host);
        if (count_touched && (rc = record_touched(ctx, L, P, DP.on, queries, n_queries, nm_host, dev_out ? T.o.num_matched : nullptr))) return rc;
        std::vector<uint32_t> ne;
        if (keep_ids && n_work && (bo.record_last || bo.id_lists)) {
            ne.resize(n_work);
            TSGPU_HIP_TRY(hipMemcpy(ne.data(), T.part.n_emit, (size_t)n_work * 4, hipMemcpyDeviceToHost));
        }
        if (bo.record_last) record_last_ids(L, P, P.work, ne, n_queries);
        if (bo.id_lists && (rc = build_id_lists(L, s, P, P.work, ne, T.ids_out, n_queries, *bo.id_lists, bo.ids_dev, bo.ids_dev_done))) return rc;
        {
            const uint64_t t_end = now_us();
            ctx->kw_batches.fetch_add(1); ctx->kw_plan_us.fetch_add(t_planned - t_enter); ctx->kw_upload_us.fetch_add(t_uploaded - t_planned);
            ctx->kw_launch_us.fetch_add(t_launched - t_uploaded); ctx->kw_wait_us.fetch_add(t_synced - t_launched); ctx->kw_book_us.fetch_add(t_end - t_synced);
            auto amax = [](std::atomic<uint64_t>& a, uint64_t v) { uint64_t c = a.load(); while (v > c && !a.compare_exchange_weak(c, v)) {} };
            amax(ctx->kw_max_plan_us, t_planned - t_enter); amax(ctx->kw_max_upload_us, t_uploaded - t_planned);
            amax(ctx->kw_max_launch_us, t_launched - t_uploaded); amax(ctx->kw_max_wait_us, t_synced - t_launched);
        }
        if (host_timing)
            fprintf(stderr, "[tsgpu] kw batch %u queries: plan %llu us, upload+reserve %llu us, launch %llu us, wait+copy %llu us, bookkeeping %llu us\n", n_queries,
                    (unsigned long long)(t_planned - t_enter), (unsigned long long)(t_uploaded - t_planned), (unsigned long long)(t_launched - t_uploaded),
                    (unsigned long long)(t_synced - t_launched), (unsigned long long)(now_us() - t_synced));
        // queries that were not run must not expose stale slots
        if (!dev_out) for (uint32_t i = 0; i < n_queries; i++) if (P.status[i] != TSGPU_OK) { out->n_hits[i] = 0; if (out->num_matched) out->num_matched[i] = 0; }
    } catch (const std::bad_alloc&) { return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_keyword_search_batch: host allocation failed"); }
    return ok();
}

// device-side shard merge (the host version, tsgpu_merge_shard_hits, lives in tsgpu_vec.hip)
// Index::compute_aux_scores' text half (src/index.cpp:8800-8846): text_match score of given documents for given queries' tokens
int tsgpu_keyword_aux_scores(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, const uint32_t* item_query, const uint32_t* item_seq_id,
                             uint32_t n_items, int64_t* scores_out) {
    if (!ctx || !queries || (n_items && (!item_query || !item_seq_id || !scores_out))) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_aux_scores: NULL argument");
    if (n_items == 0) return ok();
    (void)hipSetDevice(ctx->device);
    const std::shared_ptr<const Snapshot> snap_ref = ctx->snapshot();
    const Snapshot& snap = *snap_ref;
    try {
        std::vector<KwQueryDev> qd(n_queries);
        std::vector<KwQueryMF> mf(n_queries);
        for (uint32_t i = 0; i < n_queries; i++) {
            const tsgpu_kw_query& in = queries[i];
            KwQueryDev& q = qd[i];
            KwQueryMF& m = mf[i];
            memset(&q, 0, sizeof q);
            memset(&m, 0xFF, sizeof m);
            if (!kw_token_count_ok(in) || !kw_field_count_ok(in) || in.match_type > TSGPU_SUM_SCORE)
                return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_keyword_aux_scores: 1..10 tokens, 1..4 query_by fields");
            m.driver_token = 0;
            if (kw_fill_fields(snap, in, m)) return fail(TSGPU_ERR_NOT_FOUND, "tsgpu_keyword_aux_scores: unknown field");
            kw_fill_token_lists(snap, in, false, q, m);
            kw_fill_scoring(in, q);
            q.total_cost = 0;                                    // compute_aux_scores passes total_cost = 0, syn_orig_num_tokens = -1, no synonym flags (src/index.cpp:8826-8835)
            q.syn_orig_num_tokens = -1; q.orig_num_tokens = 0; q.is_synonym = 0; q.demote_synonym = 0;
            q.mf_index = i;
        }
        for (uint32_t i = 0; i < n_items; i++) if (item_query[i] >= n_queries) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_aux_scores: item_query out of range");
        LaneLock lane(ctx);
        KwLane& L = *lane.L;
        hipStream_t s = L.stream;
        const size_t o_q = 0, o_m = (sizeof(KwQueryDev) * n_queries + 15) & ~(size_t)15, o_i = (o_m + sizeof(KwQueryMF) * n_queries + 15) & ~(size_t)15;
        const size_t o_out = (o_i + sizeof(KwAuxItem) * n_items + 15) & ~(size_t)15, total = o_out + 8 * (size_t)n_items;
        std::vector<unsigned char> h(total);
        memcpy(h.data() + o_q, qd.data(), sizeof(KwQueryDev) * n_queries);
        memcpy(h.data() + o_m, mf.data(), sizeof(KwQueryMF) * n_queries);
        KwAuxItem* items = (KwAuxItem*)(h.data() + o_i);
        for (uint32_t i = 0; i < n_items; i++) { items[i].query = item_query[i]; items[i].seq_id = item_seq_id[i]; }
        int rc;
        if ((rc = L.d_plan.reserve(total))) return rc;
        TSGPU_HIP_TRY(hipMemcpyAsync(L.d_plan.p, h.data(), o_out, hipMemcpyHostToDevice, s));
        IndexView v = make_view(ctx, snap);
        char* base = (char*)L.d_plan.p;
        hipLaunchKernelGGL(kw_aux_score_kernel, dim3((n_items + 63) / 64), dim3(64), 0, s, v, (const KwQueryDev*)(base + o_q), (const KwQueryMF*)(base + o_m),
                           (const KwAuxItem*)(base + o_i), n_items, (int64_t*)(base + o_out));
        TSGPU_HIP_TRY(hipGetLastError());
        TSGPU_HIP_TRY(hipMemcpyAsync(scores_out, base + o_out, 8 * (size_t)n_items, hipMemcpyDeviceToHost, s));
        TSGPU_HIP_TRY(hipStreamSynchronize(s));
        return ok();
    } catch (const std::bad_alloc&) { return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_keyword_aux_scores: host allocation failed"); }
}

int tsgpu_merge_shard_hits_device(tsgpu_ctx* ctx, const tsgpu_hits* gathered, uint32_t n_shards, uint32_t n_queries, uint32_t k, tsgpu_hits* out) {
    if (!ctx || !gathered || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_merge_shard_hits_device: NULL argument");
    if (gathered->mem != TSGPU_MEM_DEVICE || out->mem != TSGPU_MEM_DEVICE) return fail(TSGPU_ERR_INVALID, "tsgpu_merge_shard_hits_device: device arrays only");
    if (!gathered->keys || !gathered->scores || !gathered->n_hits || !out->keys || !out->scores || !out->n_hits)
        return fail(TSGPU_ERR_INVALID, "tsgpu_merge_shard_hits_device: missing arrays");
    if (n_queries == 0) return ok();
    if (n_shards == 0 || k == 0 || out->k_stride < k) return fail(TSGPU_ERR_INVALID, "tsgpu_merge_shard_hits_device: bad sizes");
    const uint64_t cap_need = (uint64_t)n_shards * gathered->k_stride;
    if (cap_need > 4096 || cap_need > 65535) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_merge_shard_hits_device: n_shards * k_stride > 4096");
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    KwShardIn in;
    in.keys = gathered->keys; in.scores = gathered->scores; in.text_match = gathered->text_match; in.vector_distance = gathered->vector_distance;
    in.match_score_index = gathered->match_score_index; in.n_hits = gathered->n_hits; in.num_matched = gathered->num_matched;
    in.n_shards = n_shards; in.n_queries = n_queries; in.k_in = gathered->k_stride;
    in.packed = nullptr; in.shard_stride = 0; in.words = 0; in.q_out_offset = 0; in.status_out = nullptr; in.cap_per_query = nullptr;
    KwOut o;
    o.keys = out->keys; o.scores = out->scores; o.text_match = out->text_match; o.vector_distance = out->vector_distance;
    o.match_score_index = out->match_score_index; o.n_hits = out->n_hits; o.num_matched = out->num_matched; o.off_words = nullptr; o.k_stride = out->k_stride;
    hipStream_t s = ctx->stream;
    if (cap_need <= 512) hipLaunchKernelGGL((kw_shard_merge_kernel<512>), dim3(n_queries), dim3(KW_THREADS), 0, s, in, o, k);
    else if (cap_need <= 1024) hipLaunchKernelGGL((kw_shard_merge_kernel<1024>), dim3(n_queries), dim3(KW_THREADS), 0, s, in, o, k);
    else if (cap_need <= 2048) hipLaunchKernelGGL((kw_shard_merge_kernel<2048>), dim3(n_queries), dim3(KW_THREADS), 0, s, in, o, k);
    else hipLaunchKernelGGL((kw_shard_merge_kernel<4096>), dim3(n_queries), dim3(KW_THREADS), 0, s, in, o, k);
    TSGPU_HIP_TRY(hipGetLastError());
    TSGPU_HIP_TRY(hipStreamSynchronize(s));
    return ok();
}

// SURVEY §8f rank 2 — Index::search_all_candidates (src/index.cpp:1794-1894) for a batch of user queries: the candidate-token
// combinations of group g are combos[group_begin[g] .. group_begin[g+1]) in the reference's pass order; all of them run as ONE
// keyword batch, kw_candidates_merge_kernel folds each group like the shared Topster, the id-set kernels like id_buff.
int tsgpu_keyword_search_candidates_batch(tsgpu_ctx* ctx, const tsgpu_kw_query* combos, const uint32_t* group_begin, uint32_t n_groups,
                                          tsgpu_hits* out, uint32_t* query_index, uint64_t* found) {
    return kw_candidates_batch_ex(ctx, combos, group_begin, n_groups, out, query_index, found, false, nullptr, nullptr);
}

}  // extern "C"

namespace tsgpu {
int kw_candidates_batch_ex(tsgpu_ctx* ctx, const tsgpu_kw_query* combos, const uint32_t* group_begin, uint32_t n_groups,
                           tsgpu_hits* out, uint32_t* query_index, uint64_t* found, bool raw_pass, uint32_t* pass_mask_dev, const uint16_t* present_elsewhere) {
    if (!ctx || !out || !group_begin) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_candidates_batch: NULL argument");
    if (n_groups == 0) return ok();
    if (!out->keys || !out->scores || !out->n_hits || !out->status) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_candidates_batch: missing output arrays");
    const uint32_t n_combos = group_begin[n_groups];
    if (n_combos && !combos) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_candidates_batch: combos is NULL");
    const uint32_t KS = out->k_stride;
    uint32_t max_passes = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        if (group_begin[g + 1] < group_begin[g]) return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_candidates_batch: group_begin must be non-decreasing");
        max_passes = std::max(max_passes, group_begin[g + 1] - group_begin[g]);
    }
    if (max_passes > (uint32_t)KW_MAX_CANDIDATE_PASSES || (uint64_t)max_passes * KS > 4096)
        return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_keyword_search_candidates_batch: more than 16 combinations per query, or combinations * k_stride > 4096");
    const bool dev_out = out->mem == TSGPU_MEM_DEVICE;
    if (dev_out && (!out->text_match || !out->vector_distance || !out->match_score_index || !out->num_matched))
        return fail(TSGPU_ERR_INVALID, "tsgpu_keyword_search_candidates_batch: device output needs every tsgpu_hits array");
    CtxMuForVectorKeys vq_hold;                       // combinations with a vector-query sort key: ctx->mu before the lane, until the kernels have finished (tsgpu_host.h)
    if (ctx->sort_keys_live.load(std::memory_order_relaxed) && names_vector_query_key(combos, n_combos)) vq_hold.take(ctx);
    LaneLock ll(ctx, 0);                              // (tsgpu_candidates_result_ids reads this lane's bitmaps afterwards)
    KwLane& L = *ll.L;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = L.stream;
    vq_hold.stream = s;
    try {
        int rc;
        const size_t pslots = (size_t)std::max<uint32_t>(n_combos, 1) * KS, pn = std::max<uint32_t>(n_combos, 1);
        if ((rc = L.d_cand_keys.reserve(pslots * 8)) || (rc = L.d_cand_scores.reserve(pslots * 24)) || (rc = L.d_cand_tm.reserve(pslots * 8)) ||
            (rc = L.d_cand_vd.reserve(pslots * 4)) || (rc = L.d_cand_msi.reserve(pslots)) || (rc = L.d_cand_nh.reserve(pn * 4)) ||
            (rc = L.d_cand_nm.reserve(pn * 8)) || (rc = L.d_cand_st.reserve(pn * 4)))
            return rc;
        tsgpu_hits pass;
        memset(&pass, 0, sizeof(pass));
        pass.mem = TSGPU_MEM_DEVICE; pass.k_stride = KS;
        pass.keys = L.d_cand_keys.as<uint64_t>(); pass.scores = L.d_cand_scores.as<int64_t>(); pass.text_match = L.d_cand_tm.as<int64_t>();
        pass.vector_distance = L.d_cand_vd.as<float>(); pass.match_score_index = L.d_cand_msi.as<int8_t>();
        pass.n_hits = L.d_cand_nh.as<uint32_t>(); pass.num_matched = L.d_cand_nm.as<uint64_t>(); pass.status = L.d_cand_st.as<int32_t>();
        std::vector<int32_t> st, co;
        // all_result_ids: one bitmap per group (below). They are cleared on a second stream while the passes run — 1.25 MB per group at 10M documents is
        // HBM-rate work the scalar-bound find kernel does not notice (as a memset in front of the marks it was 0.18 ms of the 7.3 ms step of 1 000 groups)
        const uint64_t id_words = std::max<uint64_t>(((uint64_t)ctx->num_docs + 31) / 32, 1);
        L.last_cand_groups = 0;
        if (found) {
            if ((uint64_t)n_groups * id_words * 4 > (8ull << 30))
                return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_keyword_search_candidates_batch: id-set bitmaps (n_groups * num_docs / 8 bytes) exceed 8 GiB; split the batch");
            if ((rc = L.d_cand_bits.reserve((size_t)n_groups * id_words * 4)) || (rc = L.d_cand_found.reserve((size_t)n_groups * 8))) return rc;
            if (!L.aux_stream) TSGPU_HIP_TRY(hipStreamCreateWithFlags(&L.aux_stream, hipStreamNonBlocking));
            if (!L.ev_aux) TSGPU_HIP_TRY(hipEventCreateWithFlags(&L.ev_aux, hipEventDisableTiming));
            TSGPU_HIP_TRY(hipEventRecord(L.ev_aux, s));                       // (whatever the caller's stream still does with the last call's bitmaps comes first)
            TSGPU_HIP_TRY(hipStreamWaitEvent(L.aux_stream, L.ev_aux, 0));
            TSGPU_HIP_TRY(hipMemsetAsync(L.d_cand_bits.p, 0, (size_t)n_groups * id_words * 4, L.aux_stream));
            TSGPU_HIP_TRY(hipMemsetAsync(L.d_cand_found.p, 0, (size_t)n_groups * 8, L.aux_stream));
            TSGPU_HIP_TRY(hipEventRecord(L.ev_aux, L.aux_stream));
        }
        L.last_tab_n_work = 0;
        if (n_combos) {
            BatchOpts bo;
            bo.keep_ids = found != nullptr;                    // the union needs every pass's emitted ids
            bo.status_host = &st;
            bo.cutoff_host = &co;
            bo.record_last = false;                            // (the marks below read the batch's tables on the device; tsgpu_candidates_result_ids reads the bitmaps)
            bo.present_elsewhere = present_elsewhere;
            rc = kw_batch_on_lane(ctx, L, combos, n_combos, &pass, bo);
            if (rc) { if (found) (void)hipStreamSynchronize(L.aux_stream); return rc; }
        }
        // a group runs only if every combination of it ran; otherwise it reports the first failing status and no hits
        std::vector<uint32_t> range((size_t)n_groups * 3 + 3, 0);        // per group: first entry, one past the last, Topster capacity
        std::vector<int32_t> gstatus(n_groups, TSGPU_OK), gcut(n_groups, 0);       // a group is cut off when any of its passes was
        for (uint32_t g = 0; g < n_groups; g++) {
            for (uint32_t e = group_begin[g]; e < group_begin[g + 1]; e++) if (e < co.size() && co[e]) gcut[g] = 1;
            for (uint32_t e = group_begin[g]; e < group_begin[g + 1]; e++) if (st[e] != TSGPU_OK) { gstatus[g] = st[e]; break; }
            if (gstatus[g] == TSGPU_OK && group_begin[g + 1] > group_begin[g]) {
                range[3 * g] = group_begin[g]; range[3 * g + 1] = group_begin[g + 1];
                range[3 * g + 2] = std::min(resolve_topster_size(ctx, combos[group_begin[g]]), KS);      // the shared Topster is sized once, by the first pass
            }
        }
        if ((rc = upload(L.d_cand_gb, range.data(), range.size() * 4, s))) return rc;

        const size_t slots = (size_t)n_groups * KS;
        KwOut o;
        o.k_stride = KS; o.off_words = nullptr;
        uint32_t* qi_dev = nullptr;
        if (dev_out) {
            o.keys = out->keys; o.scores = out->scores; o.text_match = out->text_match; o.vector_distance = out->vector_distance;
            o.match_score_index = out->match_score_index; o.n_hits = out->n_hits; o.num_matched = out->num_matched;
            qi_dev = query_index;
        } else {
            if ((rc = L.d_out_keys.reserve(slots * 8)) || (rc = L.d_out_scores.reserve(slots * 24)) || (rc = L.d_out_tm.reserve(slots * 8)) ||
                (rc = L.d_out_vd.reserve(slots * 4)) || (rc = L.d_out_msi.reserve(slots)) || (rc = L.d_out_nh.reserve((size_t)n_groups * 4)) ||
                (rc = L.d_out_nm.reserve((size_t)n_groups * 8)) || (rc = L.d_cand_qi.reserve(slots * 4)))
                return rc;
            o.keys = L.d_out_keys.as<uint64_t>(); o.scores = L.d_out_scores.as<int64_t>(); o.text_match = L.d_out_tm.as<int64_t>();
            o.vector_distance = L.d_out_vd.as<float>(); o.match_score_index = L.d_out_msi.as<int8_t>();
            o.n_hits = L.d_out_nh.as<uint32_t>(); o.num_matched = L.d_out_nm.as<uint64_t>();
            qi_dev = query_index ? L.d_cand_qi.as<uint32_t>() : nullptr;
        }
        KwCandIn in;
        in.keys = pass.keys; in.scores = pass.scores; in.text_match = pass.text_match; in.vector_distance = pass.vector_distance;
        in.match_score_index = pass.match_score_index; in.n_hits = pass.n_hits; in.num_matched = pass.num_matched;
        in.group_range = L.d_cand_gb.as<uint32_t>(); in.k_in = KS;
        in.raw_pass = raw_pass ? 1u : 0u; in.pass_mask = pass_mask_dev;
        const uint64_t cap_need = (uint64_t)std::max<uint32_t>(max_passes, 1) * KS;
        bool any_s2 = false;
        for (uint32_t e = 0; e < n_combos; e++) any_s2 = any_s2 || combos[e].n_sort > 2;
        // the sort-free fold (kw_candidates_rank_kernel); three sort keys AND more than 2 048 slots do not fit its LDS next to the hash table: the sorting kernel
        if (ctx->kw_candidates_rank_fold && !(cap_need > 2048 && any_s2)) {
            ctx->kw_candidates_rank_launches++;
#define TSGPU_CAND_RANK(C) do { if (any_s2) hipLaunchKernelGGL((kw_candidates_rank_kernel<C, true>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev); \
                                else hipLaunchKernelGGL((kw_candidates_rank_kernel<C, false>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev); } while (0)
            if (cap_need <= 512) TSGPU_CAND_RANK(512);
            else if (cap_need <= 1024) TSGPU_CAND_RANK(1024);
            else if (cap_need <= 2048) TSGPU_CAND_RANK(2048);
            else hipLaunchKernelGGL((kw_candidates_rank_kernel<4096, false>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev);
#undef TSGPU_CAND_RANK
        } else
        if (cap_need <= 512) hipLaunchKernelGGL((kw_candidates_merge_kernel<512>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev);
        else if (cap_need <= 1024) hipLaunchKernelGGL((kw_candidates_merge_kernel<1024>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev);
        else if (cap_need <= 2048) hipLaunchKernelGGL((kw_candidates_merge_kernel<2048>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev);
        else hipLaunchKernelGGL((kw_candidates_merge_kernel<4096>), dim3(n_groups), dim3(KW_THREADS), 0, s, in, o, qi_dev);
        TSGPU_HIP_TRY(hipGetLastError());

        // ---- all_result_ids: one bitmap per group, marked from the passes' id segments; the marks count the union (kw_idset_mark_items_kernel) ----
        L.last_cand_found.assign(n_groups, 0);
        if (found) {
            TSGPU_HIP_TRY(hipStreamWaitEvent(s, L.ev_aux, 0));               // the cleared bitmaps
            if (n_combos && L.last_tab_n_work) {
                std::vector<uint32_t> group_of(n_combos, KW_NONE);
                for (uint32_t g = 0; g < n_groups; g++)
                    if (gstatus[g] == TSGPU_OK) for (uint32_t e = group_begin[g]; e < group_begin[g + 1]; e++) group_of[e] = g;
                if ((rc = upload(L.d_cand_segs, group_of.data(), group_of.size() * 4, s))) return rc;
                hipLaunchKernelGGL(kw_idset_mark_items_kernel, dim3(L.last_tab_n_work, 8), dim3(KW_THREADS), 0, s, L.d_ids_out.as<uint32_t>(),
                                   (const KwQueryDev*)L.last_tab_q, (const KwWorkItem*)L.last_tab_w, L.d_part_ne.as<uint32_t>(), L.d_cand_segs.as<uint32_t>(),
                                   L.d_cand_bits.as<uint32_t>(), id_words, L.d_cand_found.as<unsigned long long>());
                TSGPU_HIP_TRY(hipGetLastError());
            }
            TSGPU_HIP_TRY(hipMemcpyAsync(L.last_cand_found.data(), L.d_cand_found.p, (size_t)n_groups * 8, hipMemcpyDeviceToHost, s));
            if (dev_out) TSGPU_HIP_TRY(hipMemcpyAsync(found, L.d_cand_found.p, (size_t)n_groups * 8, hipMemcpyDeviceToDevice, s));
            L.last_cand_groups = n_groups;
            L.last_cand_words = id_words;
        }

        // ---- results ----
        if (!dev_out) {
            TSGPU_HIP_TRY(hipMemcpyAsync(out->n_hits, o.n_hits, (size_t)n_groups * 4, hipMemcpyDeviceToHost, s));
            if (out->num_matched) TSGPU_HIP_TRY(hipMemcpyAsync(out->num_matched, o.num_matched, (size_t)n_groups * 8, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(out->keys, o.keys, slots * 8, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(out->scores, o.scores, slots * 24, hipMemcpyDeviceToHost, s));
            if (out->text_match) TSGPU_HIP_TRY(hipMemcpyAsync(out->text_match, o.text_match, slots * 8, hipMemcpyDeviceToHost, s));
            if (out->vector_distance) TSGPU_HIP_TRY(hipMemcpyAsync(out->vector_distance, o.vector_distance, slots * 4, hipMemcpyDeviceToHost, s));
            if (out->match_score_index) TSGPU_HIP_TRY(hipMemcpyAsync(out->match_score_index, o.match_score_index, slots, hipMemcpyDeviceToHost, s));
            if (query_index) TSGPU_HIP_TRY(hipMemcpyAsync(query_index, qi_dev, slots * 4, hipMemcpyDeviceToHost, s));
            for (uint32_t g = 0; g < n_groups; g++) out->status[g] = gstatus[g];
            if (out->search_cutoff) for (uint32_t g = 0; g < n_groups; g++) out->search_cutoff[g] = gcut[g];
        } else {
            TSGPU_HIP_TRY(hipMemcpyAsync(out->status, gstatus.data(), (size_t)n_groups * 4, hipMemcpyHostToDevice, s));
            if (out->search_cutoff) TSGPU_HIP_TRY(hipMemcpyAsync(out->search_cutoff, gcut.data(), (size_t)n_groups * 4, hipMemcpyHostToDevice, s));
        }
        TSGPU_HIP_TRY(hipStreamSynchronize(s));
        if (found && !dev_out) for (uint32_t g = 0; g < n_groups; g++) found[g] = L.last_cand_found[g];
    } catch (const std::bad_alloc&) { return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_keyword_search_candidates_batch: host allocation failed"); }
    return ok();
}

uint64_t kw_dictionary_fingerprint(tsgpu_ctx* ctx) {
    const std::shared_ptr<const Snapshot> sn = ctx->snapshot();
    return (sn && sn->maps) ? sn->maps->dict_fp : 0ull;
}
int kw_terms_present(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, uint16_t* masks) {
    const std::shared_ptr<const Snapshot> sn = ctx->snapshot();
    for (uint32_t i = 0; i < n_queries; i++) {
        const tsgpu_kw_query& in = queries[i];
        uint16_t m = 0;
        for (uint32_t t = 0; sn && t < in.n_tokens && t < TSGPU_MAX_QUERY_TOKENS; t++)
            if (kw_resolve_token(*sn, in, in.term_ids[t]).found) m |= (uint16_t)(1u << t);
        masks[i] = m;
    }
    return TSGPU_OK;
}
int kw_search_batch_masked(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, const uint16_t* present_elsewhere) {
    return kw_dispatch(ctx, queries, n_queries, out, false, nullptr, nullptr, nullptr, present_elsewhere);
}
int group_cand_tag(tsgpu_ctx* ctx, const tsgpu_hits* loc, const uint32_t* pass_of_hit, uint32_t n_groups, const uint32_t* pass_mask, const uint64_t* found, uint64_t* meta, hipStream_t s) {
    if (n_groups == 0) return TSGPU_OK;
    (void)hipSetDevice(ctx->device);
    const uint64_t n = (uint64_t)n_groups * loc->k_stride;
    hipLaunchKernelGGL(kw_group_cand_tag_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, loc->keys, pass_of_hit, (const uint32_t*)loc->n_hits, (const int32_t*)loc->status, loc->k_stride, n_groups,
                       pass_mask, (const unsigned long long*)found, (unsigned long long*)meta);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
int group_cand_fix(tsgpu_ctx* ctx, uint64_t* keys, uint32_t* query_index, const uint32_t* n_hits, uint32_t k_stride, uint32_t q0, uint32_t q1, const uint64_t* meta_all, uint32_t n_shards,
                   uint32_t n_groups, uint64_t* found, hipStream_t s) {
    if (q1 <= q0) return TSGPU_OK;
    (void)hipSetDevice(ctx->device);
    const uint64_t n = (uint64_t)(q1 - q0) * k_stride;
    hipLaunchKernelGGL(kw_group_cand_fix_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, keys, query_index, n_hits, k_stride, q0, q1, (const unsigned long long*)meta_all, n_shards, n_groups,
                       (unsigned long long*)found);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
}  // namespace tsgpu

extern "C" {

uint64_t tsgpu_candidates_result_ids(tsgpu_ctx* ctx, uint32_t group, uint32_t* out_host, uint64_t cap) {
    if (!ctx) return 0;
    LaneLock ll(ctx, 0);
    KwLane& L = *ll.L;
    (void)hipSetDevice(ctx->device);
    if (group >= L.last_cand_groups) return 0;
    const uint64_t total = L.last_cand_found[group];
    if (!out_host || cap == 0 || total == 0) return total;
    const uint64_t m = std::min(total, cap);
    if (L.d_cand_ids.reserve(m * 4)) return 0;
    hipLaunchKernelGGL(kw_idset_expand_kernel, dim3(1), dim3(KW_THREADS), 0, L.stream, L.d_cand_bits.as<uint32_t>() + (uint64_t)group * L.last_cand_words,
                       L.last_cand_words, L.d_cand_ids.as<uint32_t>(), m);
    if (hipMemcpyAsync(out_host, L.d_cand_ids.p, m * 4, hipMemcpyDeviceToHost, L.stream) != hipSuccess) return 0;
    if (hipStreamSynchronize(L.stream) != hipSuccess) return 0;
    return total;
}

// legacy single-caller form (the ids of the LAST batch run with tsgpu_keep_result_ids(ctx, 1)); concurrent callers use
// tsgpu_keyword_search_batch_ids, whose id lists belong to the call
uint64_t tsgpu_result_ids(tsgpu_ctx* ctx, uint32_t q, uint32_t* out_host, uint64_t cap) {
    if (!ctx) return 0;
    LaneLock ll(ctx, 0);
    KwLane& L = *ll.L;
    (void)hipSetDevice(ctx->device);
    if (q >= L.last_chunk_emit.size()) return 0;
    uint64_t total = 0;
    const auto& ce = L.last_chunk_emit[q];
    for (size_t c = 0; c < ce.size(); c++) total += ce[c];
    if (!out_host || cap == 0) return total;
    if (L.last_ids_unsorted[q]) {
        // multi-field query: one ascending segment per (driver field, chunk); id_buff is ascending in the reference -> merge on the host
        std::vector<uint32_t> all(total);
        uint64_t at = 0;
        for (size_t c = 0; c < ce.size(); c++) {
            if (!ce[c]) continue;
            if (hipMemcpy(all.data() + at, L.d_ids_out.as<uint32_t>() + L.last_ids_off[q] + L.last_chunk_off[q][c], (size_t)ce[c] * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
            at += ce[c];
        }
        std::sort(all.begin(), all.end());
        memcpy(out_host, all.data(), (size_t)std::min<uint64_t>(total, cap) * 4);
        return total;
    }
    uint64_t done = 0;
    for (size_t c = 0; c < ce.size() && done < cap; c++) {
        const uint64_t seg = L.last_ids_off[q] + L.last_chunk_off[q][c];
        const uint64_t m = std::min<uint64_t>(ce[c], cap - done);
        if (m && hipMemcpy(out_host + done, L.d_ids_out.as<uint32_t>() + seg, m * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
        done += m;
    }
    return total;
}

// TSGPU_PROF builds (tools/ only; not declared in include/tsgpu.h): per-phase cycle counters of kw_search_kernel
int tsgpu_debug_prof(tsgpu_ctx* ctx, int reset, uint64_t* out16) {
    if (!ctx) return TSGPU_ERR_INVALID;
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (ctx->d_prof.reserve(16 * 8)) return TSGPU_ERR_NO_MEMORY;
    if (out16) TSGPU_HIP_TRY(hipMemcpy(out16, ctx->d_prof.p, 16 * 8, hipMemcpyDeviceToHost));
    if (reset) TSGPU_HIP_TRY(hipMemset(ctx->d_prof.p, 0, 16 * 8));
    return TSGPU_OK;
}

int tsgpu_kw_last_touched(tsgpu_ctx* ctx, tsgpu_kw_touched* out) {
    if (!ctx || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_kw_last_touched: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->tm_mu);
    *out = ctx->kw_touched;
    return ok();
}

// measurement hook: what the DISTINCT posting lists of a set of (field, term) pairs occupy in the mirror — the working set a batch's requested
// bytes are compared with (bench.py `roofline.l2_refetch`). Exact: the lists' block records are read back from the device.
int tsgpu_kw_lists_footprint(tsgpu_ctx* ctx, const uint32_t* field_ids, const uint32_t* term_ids, uint32_t n, tsgpu_kw_footprint* out) {
    if (!ctx || !out || (n && (!field_ids || !term_ids))) return fail(TSGPU_ERR_INVALID, "tsgpu_kw_lists_footprint: NULL argument");
    (void)hipSetDevice(ctx->device);
    std::shared_ptr<const Snapshot> snap = std::atomic_load(&ctx->snap);
    memset(out, 0, sizeof(*out));
    if (!snap || !snap->ar) return ok();
    std::vector<uint32_t> handles;
    for (uint32_t i = 0; i < n; i++) { const uint32_t h = snap->find_handle(field_ids[i], term_ids[i]); if (h != 0xFFFFFFFFu) handles.push_back(h); }
    std::sort(handles.begin(), handles.end());
    handles.erase(std::unique(handles.begin(), handles.end()), handles.end());
    std::vector<BlockMeta> bm;
    for (uint32_t h : handles) {
        const ListDesc& d = snap->h_lists[h];
        bm.resize(d.n_blocks);
        if (d.n_blocks) TSGPU_HIP_TRY(hipMemcpy(bm.data(), snap->ar->blk_meta.as<BlockMeta>() + d.blk_base, (size_t)d.n_blocks * sizeof(BlockMeta), hipMemcpyDeviceToHost));
        for (const BlockMeta& m : bm) {
            out->ids_bytes += 4ull * packed_words(m.n_ids, m.ids_bits);
            out->payload_bytes += 4ull * (packed_words(m.n_ids, m.oi_bits) + packed_words(m.n_off, m.off_bits));
        }
        out->block_metadata_bytes += (uint64_t)d.n_blocks * (sizeof(BlockIds) + 4 + sizeof(BlockMeta));
        if (d.dir_slot && snap->dir_pool) out->directory_bytes += 8ull * snap->dir_pool->slot_entries;
        out->n_ids += d.n_ids;
    }
    out->n_lists = handles.size();
    return ok();
}

int tsgpu_last_aux_timings(tsgpu_ctx* ctx, tsgpu_aux_timings* out) {
    if (!ctx || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_last_aux_timings: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->tm_mu);
    *out = ctx->aux_timings;
    return ok();
}

int tsgpu_last_timings(tsgpu_ctx* ctx, tsgpu_timings* out) {
    if (!ctx || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_last_timings: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->tm_mu);
    *out = ctx->timings;
    return ok();
}

}  // extern "C"

// ---- tsgpu_group (tsgpu_group.hip): the device-side halves of the keyword exchange ----
namespace tsgpu {
// The flat branch of the vector search (tsgpu_vec.hip computes the distance matrix): every query ranks its filter ids by its sort keys with
// the id's distance as KV::vector_distance / the vector_distance sort key — the wildcard machinery (work items of 256-id blocks, LDS
// Topster, kw_merge_kernel) with one more column. num_matched = the ids the threshold kept = `found`; ids_out (optional) = those ids.
int kw_vector_flat_search(tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_queries, tsgpu_hits* out, const KwVFlat* vf, tsgpu_id_lists** ids_out) {
    if (!ctx || !out || !queries || !vf || n_queries == 0) return fail(TSGPU_ERR_INVALID, "tsgpu_vector_search_batch: bad arguments");
    struct CallerCount { std::atomic<int>& c; explicit CallerCount(std::atomic<int>& x) : c(x) { c.fetch_add(1); } ~CallerCount() { c.fetch_sub(1); } } cc(ctx->kw_callers);
    std::unique_ptr<tsgpu_id_lists> lists;
    if (ids_out) { *ids_out = nullptr; lists.reset(new (std::nothrow) tsgpu_id_lists); if (!lists) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_vector_search_batch: host allocation failed"); }
    BatchOpts bo;
    bo.wildcard = true;
    bo.vflat = vf;
    bo.keep_ids = ids_out != nullptr;
    bo.id_lists = lists.get();
    bo.record_last = false;
    LaneLock ll(ctx, tsgpu::tls_avoid_lane0() ? -2 : -1);
    const int rc = kw_batch_on_lane(ctx, *ll.L, queries, n_queries, out, bo);
    if (rc == TSGPU_OK && ids_out) *ids_out = lists.release();
    return rc;
}

int group_pack_keyword(tsgpu_ctx* ctx, const tsgpu_hits* loc, uint32_t n_q, uint32_t k, uint32_t words, uint64_t* block, hipStream_t s) {
    if (!loc || loc->mem != TSGPU_MEM_DEVICE || !loc->keys || !loc->scores || !loc->n_hits || k == 0 || k > loc->k_stride || (words != 4 && words != 5))
        return fail(TSGPU_ERR_INVALID, "tsgpu_group: bad local result");
    (void)hipSetDevice(ctx->device);
    KwOut o;
    o.keys = loc->keys; o.scores = loc->scores; o.text_match = loc->text_match; o.vector_distance = nullptr; o.match_score_index = nullptr;
    o.n_hits = loc->n_hits; o.num_matched = loc->num_matched; o.off_words = nullptr; o.k_stride = loc->k_stride;
    const uint64_t n = (uint64_t)n_q * k;
    hipLaunchKernelGGL(kw_group_pack_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, o, (const int32_t*)loc->status, n_q, k, words, block);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
// bound-pruned exchange (kw_kernels.hip.h, "bound-pruned exchange"): this shard's kq-th best entry per query -> kth[n_q][4]
static KwOut kw_out_of(const tsgpu_hits* loc) {
    KwOut o;
    o.keys = loc->keys; o.scores = loc->scores; o.text_match = loc->text_match; o.vector_distance = nullptr; o.match_score_index = nullptr;
    o.n_hits = loc->n_hits; o.num_matched = loc->num_matched; o.off_words = nullptr; o.k_stride = loc->k_stride;
    return o;
}
int group_kw_kth(tsgpu_ctx* ctx, const tsgpu_hits* loc, uint32_t n_q, uint32_t k, uint32_t n_shards, const uint32_t* caps_dev, int64_t* kth, hipStream_t s) {
    (void)hipSetDevice(ctx->device);
    hipLaunchKernelGGL(kw_group_kth_kernel, dim3((n_q + 255) / 256), dim3(256), 0, s, kw_out_of(loc), (const int32_t*)loc->status, caps_dev, n_q, k, n_shards, kth);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
// ... the bounds from the gathered reports, this shard's entries at or above them packed into n_dst slices of slice_words u64 (per header pairs + room for
// per * k entries); cursor[n_dst] (zeroed here) ends as the slices' entry totals
int group_kw_prune_pack(tsgpu_ctx* ctx, const tsgpu_hits* loc, uint32_t n_q, uint32_t n_pad, uint32_t k, uint32_t words, const uint32_t* caps_dev, const int64_t* kth_all,
                        uint32_t n_shards, uint32_t per, uint32_t n_dst, uint64_t slice_words, uint64_t* block, uint32_t* cursor, hipStream_t s) {
    (void)hipSetDevice(ctx->device);
    TSGPU_HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)n_dst * 4, s));
    hipLaunchKernelGGL(kw_group_prune_pack_kernel, dim3((n_pad + 3) / 4), dim3(256), 0, s, kw_out_of(loc), (const int32_t*)loc->status, caps_dev, n_q, n_pad, k, words, kth_all, n_shards,
                       per, slice_words, block, cursor);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
int group_store_keyword_slice(tsgpu_ctx* ctx, const tsgpu_hits* loc, uint32_t n_q, uint32_t q_out_offset, uint32_t k, const tsgpu_hits* out, hipStream_t s) {
    if (n_q == 0) return TSGPU_OK;
    (void)hipSetDevice(ctx->device);
    KwOut l, o;
    l.keys = loc->keys; l.scores = loc->scores; l.text_match = loc->text_match; l.vector_distance = nullptr; l.match_score_index = nullptr;
    l.n_hits = loc->n_hits; l.num_matched = loc->num_matched; l.off_words = nullptr; l.k_stride = loc->k_stride;
    o.keys = out->keys; o.scores = out->scores; o.text_match = out->text_match; o.vector_distance = nullptr; o.match_score_index = nullptr;
    o.n_hits = out->n_hits; o.num_matched = out->num_matched; o.off_words = nullptr; o.k_stride = out->k_stride;
    const uint64_t n = (uint64_t)n_q * k;
    hipLaunchKernelGGL(kw_group_store_slice_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, l, (const int32_t*)loc->status, n_q, q_out_offset, k, o, out->status);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
void group_resolve_topster_sizes(const tsgpu_ctx* ctx, const tsgpu_kw_query* queries, uint32_t n_q, uint32_t* caps) {
    for (uint32_t i = 0; i < n_q; i++) caps[i] = resolve_topster_size(ctx, queries[i]);
}
int group_merge_keyword(tsgpu_ctx* ctx, const uint64_t* gathered, uint64_t shard_stride_words, uint32_t n_shards, uint32_t n_q, uint32_t q_out_offset, uint32_t k, uint32_t words,
                        const uint32_t* caps_dev, const tsgpu_hits* out, hipStream_t s, uint32_t pruned_per) {
    if (n_q == 0) return TSGPU_OK;
    if (!out || out->mem != TSGPU_MEM_DEVICE || !out->keys || !out->scores || !out->n_hits || out->k_stride < k) return fail(TSGPU_ERR_INVALID, "tsgpu_group: bad output arrays");
    const uint64_t cap_need = (uint64_t)n_shards * k;
    if (cap_need > 4096) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_group: members * k > 4096");
    (void)hipSetDevice(ctx->device);
    KwShardIn in;
    memset(&in, 0, sizeof in);
    in.n_shards = n_shards; in.n_queries = n_q; in.k_in = k;
    in.packed = gathered; in.shard_stride = shard_stride_words; in.words = words; in.q_out_offset = q_out_offset; in.status_out = out->status; in.cap_per_query = caps_dev;
    in.pruned_per = pruned_per;
    KwOut o;
    o.keys = out->keys; o.scores = out->scores; o.text_match = out->text_match; o.vector_distance = out->vector_distance;
    o.match_score_index = nullptr; o.n_hits = out->n_hits; o.num_matched = out->num_matched; o.off_words = nullptr; o.k_stride = out->k_stride;
    if (cap_need <= 512) hipLaunchKernelGGL((kw_shard_merge_kernel<512>), dim3(n_q), dim3(KW_THREADS), 0, s, in, o, k);
    else if (cap_need <= 1024) hipLaunchKernelGGL((kw_shard_merge_kernel<1024>), dim3(n_q), dim3(KW_THREADS), 0, s, in, o, k);
    else if (cap_need <= 2048) hipLaunchKernelGGL((kw_shard_merge_kernel<2048>), dim3(n_q), dim3(KW_THREADS), 0, s, in, o, k);
    else hipLaunchKernelGGL((kw_shard_merge_kernel<4096>), dim3(n_q), dim3(KW_THREADS), 0, s, in, o, k);
    TSGPU_HIP_TRY(hipGetLastError());
    return TSGPU_OK;
}
}  // namespace tsgpu

// ---------------------------------------------------------------- infix search (kw_infix.hip.h)
namespace {
enum InfixBuf { IB_Q, IB_PAT, IB_MCNT, IB_MTERMS, IB_ITEMS, IB_BITS, IB_FBITS, IB_FOUND, IB_AUX, IB_SEGS, IB_FSLOT, IB_CHUNK, IB_IDS, IB_OFF, IB_NIDS };
const uint64_t INFIX_MATCH_MAX_BYTES = 1ull << 30;         // match lists of one scan launch (capacity: vocabulary slots x 4 bytes per query); more queries -> more launches
const uint32_t INFIX_MARK_BLOCKS = 64;                     // posting blocks per work item of the union
const uint32_t INFIX_ROUND_MAX_QUERIES = 32768;            // (grid.y of the bitmap kernels)
struct IndexViewLists { const ListDesc* lists; const BlockIds* blk_ids; const uint32_t* ids_payload; };     // what the union reads of a snapshot

// the wildcard machinery over id lists that are on the device already: query j ranks the n_filter ids at wild[j]
// (tm: the phrase front's text-match arrays beside them, KwQueryDev::wild_tm; nullptr = the constant 100)
int infix_rank(tsgpu_ctx* ctx, const tsgpu_kw_query* q, uint32_t m, tsgpu_hits* out, const uint64_t* wild, const uint64_t* tm = nullptr) {
    struct CallerCount { std::atomic<int>& c; explicit CallerCount(std::atomic<int>& x) : c(x) { c.fetch_add(1); } ~CallerCount() { c.fetch_sub(1); } } cc(ctx->kw_callers);
    CtxMuForVectorKeys vq_hold;
    if (ctx->sort_keys_live.load(std::memory_order_relaxed) != 0 && names_vector_query_key(q, m)) vq_hold.take(ctx);
    BatchOpts bo;
    bo.wildcard = true;
    bo.record_last = false;
    bo.wild_ids_dev = wild; bo.wild_tm_dev = tm;
    LaneLock ll(ctx, tsgpu::tls_avoid_lane0() ? -2 : -1);
    vq_hold.stream = ll.L->stream;
    return kw_batch_on_lane(ctx, *ll.L, q, m, out, bo);
}

int infix_batch(tsgpu_ctx* ctx, const tsgpu_infix_query* queries, uint32_t n_queries, tsgpu_hits* out, uint32_t* n_tokens_matched, uint64_t* n_infix_ids, tsgpu_id_lists* lists) {
    for (uint32_t i = 0; i < n_queries; i++) {
        out->n_hits[i] = 0; out->status[i] = TSGPU_OK;
        if (out->num_matched) out->num_matched[i] = 0;
        if (out->search_cutoff) out->search_cutoff[i] = 0;
        if (n_tokens_matched) n_tokens_matched[i] = 0;
        if (n_infix_ids) n_infix_ids[i] = 0;
    }
    std::lock_guard<std::mutex> lk(ctx->infix_mu);             // one front at a time: it owns the stream and the scratch below
    (void)hipSetDevice(ctx->device);
    if (!ctx->infix_stream) TSGPU_HIP_TRY(hipStreamCreateWithFlags(&ctx->infix_stream, hipStreamNonBlocking));
    hipStream_t s = ctx->infix_stream;
    DevBuf* B = ctx->infix_buf;
    const std::shared_ptr<const Snapshot> held = std::atomic_load(&ctx->infix_test_snap);
    const std::shared_ptr<const Snapshot> sn = held ? held : ctx->snapshot();
    const uint64_t now = now_us();
    const bool timing = ctx->infix_timing;
    int rc;

    // ---- the queries' own checks; the ones that pass, by field
    std::vector<std::pair<uint32_t, uint32_t>> by_field;       // (field, query)
    for (uint32_t i = 0; i < n_queries; i++) {
        const tsgpu_infix_query& q = queries[i];
        int st = TSGPU_OK;
        if ((q.pattern_len && !q.pattern) || q.n_sort > TSGPU_MAX_SORT_KEYS || (q.n_filter && !q.filter_ids) || (q.n_excluded && !q.excluded_ids) ||
            sn->infix.find(q.field_id) == sn->infix.end()) st = TSGPU_ERR_INVALID;
        else if (q.pattern_len > TSGPU_MAX_INFIX_PATTERN) st = TSGPU_ERR_UNSUPPORTED;
        else if ((st = check_sort_slots(ctx, q.sort, q.n_sort, false, false, nullptr)) != TSGPU_OK) {}
        else if (q.deadline_us != 0 && now > q.deadline_us) { st = TSGPU_ERR_DEADLINE; if (out->search_cutoff) out->search_cutoff[i] = 1; }
        out->status[i] = st;
        if (st == TSGPU_OK) by_field.emplace_back(q.field_id, i);
    }
    std::stable_sort(by_field.begin(), by_field.end(), [](const auto& a, const auto& b) { return a.first < b.first; });

    // ---- scan: one pass over a field's vocabulary for all of its queries -> per query the matching tokens' term ids -> the posting lists they have
    std::vector<std::vector<uint32_t>> lists_of(n_queries);
    for (size_t f0 = 0; f0 < by_field.size();) {
        size_t f1 = f0;
        while (f1 < by_field.size() && by_field[f1].first == by_field[f0].first) f1++;
        const uint32_t field = by_field[f0].first;
        const InfixVocabSnap& V = sn->infix.at(field);
        const uint64_t t_scan = timing ? now_us() : 0;
        if (V.n_slots != 0 && V.dev) {
            const InfixVocabView view{V.dev->bytes.as<uint8_t>(), V.dev->byte_ptr.as<uint32_t>(), V.dev->term_id.as<uint32_t>(), V.dev->born.as<uint32_t>(), V.dev->died.as<uint32_t>(),
                                      V.n_slots, V.epoch};
            const uint64_t per_q = (uint64_t)V.n_slots * 4;
            const size_t max_q = (size_t)std::max<uint64_t>(1, INFIX_MATCH_MAX_BYTES / per_q);
            for (size_t g0 = f0; g0 < f1; g0 += max_q) {
                const uint32_t ng = (uint32_t)std::min(max_q, f1 - g0);
                std::vector<InfixQueryDev> dq(ng);
                std::vector<uint8_t> pat;
                for (uint32_t j = 0; j < ng; j++) {
                    const tsgpu_infix_query& q = queries[by_field[g0 + j].second];
                    dq[j] = InfixQueryDev{(uint32_t)pat.size(), q.pattern_len, q.max_extra_prefix, q.max_extra_suffix, j * V.n_slots, 0};
                    pat.insert(pat.end(), q.pattern, q.pattern + q.pattern_len);
                }
                if ((rc = upload(B[IB_Q], dq.data(), dq.size() * sizeof(InfixQueryDev), s)) || (rc = upload(B[IB_PAT], pat.data(), pat.size(), s)) ||
                    (rc = B[IB_MCNT].reserve((size_t)ng * 4)) || (rc = B[IB_MTERMS].reserve((size_t)ng * per_q))) return rc;
                TSGPU_HIP_TRY(hipMemsetAsync(B[IB_MCNT].p, 0, (size_t)ng * 4, s));
                hipLaunchKernelGGL(infix_scan_kernel, dim3((V.n_slots + INFIX_TILE_TOKENS - 1) / INFIX_TILE_TOKENS), dim3(INFIX_THREADS), 0, s, view, B[IB_Q].as<InfixQueryDev>(), ng,
                                   B[IB_PAT].as<uint8_t>(), B[IB_MCNT].as<uint32_t>(), B[IB_MTERMS].as<uint32_t>());
                TSGPU_HIP_TRY(hipGetLastError());
                std::vector<uint32_t> cnt(ng);
                TSGPU_HIP_TRY(hipMemcpyAsync(cnt.data(), B[IB_MCNT].p, (size_t)ng * 4, hipMemcpyDeviceToHost, s));
                TSGPU_HIP_TRY(hipStreamSynchronize(s));
                std::vector<std::vector<uint32_t>> terms(ng);
                uint64_t matched = 0;
                for (uint32_t j = 0; j < ng; j++) {
                    if (cnt[j] > V.n_slots) return fail(TSGPU_ERR_DEVICE, "tsgpu_infix_search_batch: a match list beyond the vocabulary");
                    matched += cnt[j];
                    terms[j].resize(cnt[j]);
                    if (cnt[j]) TSGPU_HIP_TRY(hipMemcpyAsync(terms[j].data(), B[IB_MTERMS].as<uint32_t>() + (size_t)j * V.n_slots, (size_t)cnt[j] * 4, hipMemcpyDeviceToHost, s));
                }
                TSGPU_HIP_TRY(hipStreamSynchronize(s));
                ctx->infix_scan_launches.fetch_add(1); ctx->infix_tokens_scanned.fetch_add(V.n_live); ctx->infix_tokens_matched.fetch_add(matched);
                for (uint32_t j = 0; j < ng; j++) {
                    const uint32_t i = by_field[g0 + j].second;
                    if (n_tokens_matched) n_tokens_matched[i] = cnt[j];
                    for (uint32_t term : terms[j]) {                     // a matching token without a posting list contributes nothing (:3308-3313)
                        const uint32_t h = sn->find_handle(field, term);
                        if (h != 0xFFFFFFFFu && sn->h_lists[h].n_blocks != 0) lists_of[i].push_back(h);
                    }
                }
            }
        }
        if (timing) ctx->infix_scan_us.fetch_add(now_us() - t_scan);
        f0 = f1;
    }

    // ---- union, exclusion, filter, expansion and ranking, in rounds whose scratch fits
    const uint32_t num_docs = sn->num_docs;
    const uint64_t words = ((uint64_t)num_docs + 31) / 32;
    std::vector<uint32_t> active;
    for (uint32_t i = 0; i < n_queries; i++) if (!lists_of[i].empty() && words) active.push_back(i);
    std::vector<std::vector<uint32_t>> ids_host(lists ? n_queries : 0);
    const IndexViewLists ivl{sn->lists.as<ListDesc>(), sn->ar ? sn->ar->blk_ids.as<BlockIds>() : nullptr, sn->ar ? sn->ar->ids_payload.as<uint32_t>() : nullptr};
    for (size_t a0 = 0; a0 < active.size();) {
        size_t a1 = a0;
        uint64_t bytes = 0, ids_total = 0;
        std::vector<uint64_t> off_cap;                         // [nr] offsets, then [nr] capacities
        std::vector<uint64_t> caps;
        while (a1 < active.size() && a1 - a0 < INFIX_ROUND_MAX_QUERIES) {
            const tsgpu_infix_query& q = queries[active[a1]];
            uint64_t sum = 0;
            for (uint32_t h : lists_of[active[a1]]) sum += sn->h_lists[h].n_ids;
            const uint64_t cap = std::min<uint64_t>(sum, words * 32);          // (the bitmap's bits: an id in [num_docs, words * 32) is marked and expanded like any other)
            const uint64_t need = words * 4 * (q.filter_ids ? 2 : 1) + cap * 4;
            if (a1 > a0 && bytes + need > ctx->infix_round_max_bytes) break;
            bytes += need; caps.push_back(cap); a1++;
        }
        const uint32_t nr = (uint32_t)(a1 - a0);
        ctx->infix_rounds.fetch_add(1);
        std::vector<InfixMarkItem> items;
        std::vector<uint32_t> aux, fslot(nr, INFIX_NO_POS);
        std::vector<InfixIdSeg> segs_f, segs_x;
        uint32_t nf = 0;
        uint64_t n_lists = 0;
        for (uint32_t slot = 0; slot < nr; slot++) {
            const uint32_t i = active[a0 + slot];
            const tsgpu_infix_query& q = queries[i];
            for (uint32_t h : lists_of[i]) {
                const uint32_t nb = sn->h_lists[h].n_blocks;
                for (uint32_t b = 0; b < nb; b += INFIX_MARK_BLOCKS) items.push_back(InfixMarkItem{slot, h, b, std::min(nb, b + INFIX_MARK_BLOCKS)});
            }
            n_lists += lists_of[i].size();
            if (q.filter_ids) {
                fslot[slot] = nf;
                if (q.n_filter) { segs_f.push_back(InfixIdSeg{aux.size(), q.n_filter, nf}); aux.insert(aux.end(), q.filter_ids, q.filter_ids + q.n_filter); }
                nf++;
            }
            if (q.n_excluded) { segs_x.push_back(InfixIdSeg{aux.size(), q.n_excluded, slot}); aux.insert(aux.end(), q.excluded_ids, q.excluded_ids + q.n_excluded); }
            off_cap.push_back(ids_total);
            ids_total += caps[slot];
        }
        off_cap.insert(off_cap.end(), caps.begin(), caps.end());
        std::vector<InfixIdSeg> segs(segs_f);
        segs.insert(segs.end(), segs_x.begin(), segs_x.end());
        const uint32_t n_chunks = (uint32_t)((words + INFIX_EXPAND_WORDS - 1) / INFIX_EXPAND_WORDS);
        if ((rc = B[IB_BITS].reserve((size_t)nr * words * 4)) || (rc = B[IB_FBITS].reserve((size_t)std::max<uint32_t>(nf, 1) * words * 4)) || (rc = B[IB_FOUND].reserve((size_t)nr * 8)) ||
            (rc = upload(B[IB_ITEMS], items.data(), items.size() * sizeof(InfixMarkItem), s)) || (rc = upload(B[IB_AUX], aux.data(), aux.size() * 4, s)) ||
            (rc = upload(B[IB_SEGS], segs.data(), segs.size() * sizeof(InfixIdSeg), s)) || (rc = upload(B[IB_FSLOT], fslot.data(), fslot.size() * 4, s)) ||
            (rc = upload(B[IB_OFF], off_cap.data(), off_cap.size() * 8, s)) || (rc = B[IB_CHUNK].reserve((size_t)nr * n_chunks * 4)) ||
            (rc = B[IB_IDS].reserve((size_t)std::max<uint64_t>(ids_total, 1) * 4)) || (rc = B[IB_NIDS].reserve((size_t)nr * 4))) return rc;
        TSGPU_HIP_TRY(hipMemsetAsync(B[IB_BITS].p, 0, (size_t)nr * words * 4, s));
        TSGPU_HIP_TRY(hipMemsetAsync(B[IB_FOUND].p, 0, (size_t)nr * 8, s));
        if (nf) TSGPU_HIP_TRY(hipMemsetAsync(B[IB_FBITS].p, 0, (size_t)nf * words * 4, s));
        uint32_t* bits = B[IB_BITS].as<uint32_t>();
        uint64_t t_ph = 0;
        if (timing) { TSGPU_HIP_TRY(hipStreamSynchronize(s)); t_ph = now_us(); }
        if (!items.empty())
            hipLaunchKernelGGL(infix_union_mark_kernel, dim3((uint32_t)items.size()), dim3(INFIX_THREADS), 0, s, B[IB_ITEMS].as<InfixMarkItem>(), ivl.lists, ivl.blk_ids, ivl.ids_payload, bits,
                               words, B[IB_FOUND].as<unsigned long long>());
        if (timing) { TSGPU_HIP_TRY(hipStreamSynchronize(s)); const uint64_t t = now_us(); ctx->infix_mark_us.fetch_add(t - t_ph); t_ph = t; }
        if (!segs_f.empty())
            hipLaunchKernelGGL(infix_idlist_set_kernel, dim3((uint32_t)segs_f.size(), 8), dim3(INFIX_THREADS), 0, s, B[IB_AUX].as<uint32_t>(), B[IB_SEGS].as<InfixIdSeg>(), B[IB_FBITS].as<uint32_t>(), words);
        if (nf)
            hipLaunchKernelGGL(infix_bits_and_kernel, dim3((uint32_t)((words + INFIX_THREADS - 1) / INFIX_THREADS), nr), dim3(INFIX_THREADS), 0, s, bits, B[IB_FBITS].as<uint32_t>(),
                               B[IB_FSLOT].as<uint32_t>(), words);
        if (!segs_x.empty())
            hipLaunchKernelGGL(infix_idlist_clear_kernel, dim3((uint32_t)segs_x.size(), 8), dim3(INFIX_THREADS), 0, s, B[IB_AUX].as<uint32_t>(), B[IB_SEGS].as<InfixIdSeg>() + segs_f.size(), bits, words);
        hipLaunchKernelGGL(infix_count_kernel, dim3(n_chunks, nr), dim3(INFIX_THREADS), 0, s, bits, words, B[IB_CHUNK].as<uint32_t>());
        hipLaunchKernelGGL(infix_expand_kernel, dim3(n_chunks, nr), dim3(INFIX_THREADS), 0, s, bits, words, B[IB_CHUNK].as<uint32_t>(), B[IB_IDS].as<uint32_t>(), B[IB_OFF].as<uint64_t>(),
                           B[IB_OFF].as<uint64_t>() + nr, B[IB_NIDS].as<uint32_t>());
        TSGPU_HIP_TRY(hipGetLastError());
        std::vector<uint64_t> found(nr);
        std::vector<uint32_t> nids(nr);
        TSGPU_HIP_TRY(hipMemcpyAsync(found.data(), B[IB_FOUND].p, (size_t)nr * 8, hipMemcpyDeviceToHost, s));
        TSGPU_HIP_TRY(hipMemcpyAsync(nids.data(), B[IB_NIDS].p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
        TSGPU_HIP_TRY(hipStreamSynchronize(s));
        if (timing) ctx->infix_expand_us.fetch_add(now_us() - t_ph);
        ctx->infix_lists_marked.fetch_add(n_lists);

        // the surviving ids: to the caller's list object, and — still on the device — to the wildcard ranking
        std::vector<tsgpu_kw_query> kq;
        std::vector<uint64_t> wild;
        std::vector<uint32_t> q_of;
        for (uint32_t slot = 0; slot < nr; slot++) {
            const uint32_t i = active[a0 + slot];
            const tsgpu_infix_query& q = queries[i];
            if (nids[slot] > caps[slot]) return fail(TSGPU_ERR_DEVICE, "tsgpu_infix_search_batch: an id list beyond its bound");
            if (n_infix_ids) n_infix_ids[i] = found[slot];
            if (nids[slot] == 0) continue;
            const uint32_t* d_ids = B[IB_IDS].as<uint32_t>() + off_cap[slot];
            if (lists) { ids_host[i].resize(nids[slot]); TSGPU_HIP_TRY(hipMemcpyAsync(ids_host[i].data(), d_ids, (size_t)nids[slot] * 4, hipMemcpyDeviceToHost, s)); }
            tsgpu_kw_query k;
            memset(&k, 0, sizeof k);
            k.n_sort = q.n_sort;
            for (uint32_t x = 0; x < q.n_sort; x++) k.sort[x] = q.sort[x];
            k.topster_size = q.topster_size;
            k.filter_ids = d_ids;                                  // (a device address: read through KwQueryDev::wild_ids only)
            k.n_filter = nids[slot];
            k.deadline_us = q.deadline_us;
            kq.push_back(k); wild.push_back((uint64_t)(uintptr_t)d_ids); q_of.push_back(i);
        }
        if (lists) TSGPU_HIP_TRY(hipStreamSynchronize(s));
        const uint32_t m = (uint32_t)kq.size();
        const uint64_t t_rank = timing ? now_us() : 0;
        if (m == n_queries) { if ((rc = infix_rank(ctx, kq.data(), m, out, wild.data()))) return rc; }       // every query of the call, in order: straight into the caller's arrays
        else if (m) {
            const size_t ks = out->k_stride;
            std::vector<uint64_t> keys(m * ks), nm(m);
            std::vector<int64_t> scores(m * ks * 3), tm(m * ks);
            std::vector<float> vd(m * ks);
            std::vector<int8_t> msi(m * ks);
            std::vector<uint32_t> nh(m);
            std::vector<int32_t> st(m), co(m);
            tsgpu_hits tmp{TSGPU_MEM_HOST, out->k_stride, keys.data(), scores.data(), tm.data(), vd.data(), msi.data(), nh.data(), nm.data(), st.data(), co.data()};
            if ((rc = infix_rank(ctx, kq.data(), m, &tmp, wild.data()))) return rc;
            for (uint32_t j = 0; j < m; j++) {
                const uint32_t i = q_of[j];
                const size_t n = std::min<size_t>(nh[j], ks);
                std::copy(keys.begin() + j * ks, keys.begin() + j * ks + n, out->keys + i * ks);
                std::copy(scores.begin() + j * ks * 3, scores.begin() + (j * ks + n) * 3, out->scores + i * ks * 3);
                if (out->text_match) std::copy(tm.begin() + j * ks, tm.begin() + j * ks + n, out->text_match + i * ks);
                if (out->vector_distance) std::copy(vd.begin() + j * ks, vd.begin() + j * ks + n, out->vector_distance + i * ks);
                if (out->match_score_index) std::copy(msi.begin() + j * ks, msi.begin() + j * ks + n, out->match_score_index + i * ks);
                out->n_hits[i] = nh[j]; out->status[i] = st[j];
                if (out->num_matched) out->num_matched[i] = nm[j];
                if (out->search_cutoff) out->search_cutoff[i] = co[j];
            }
        }
        if (timing) ctx->infix_rank_us.fetch_add(now_us() - t_rank);
        a0 = a1;
    }
    if (lists) {
        lists->begin.assign((size_t)n_queries + 1, 0);
        for (uint32_t i = 0; i < n_queries; i++) { lists->ids.insert(lists->ids.end(), ids_host[i].begin(), ids_host[i].end()); lists->begin[i + 1] = lists->ids.size(); }
    }
    return TSGPU_OK;
}
}  // namespace

extern "C" int tsgpu_infix_search_batch(tsgpu_ctx* ctx, const tsgpu_infix_query* queries, uint32_t n_queries, tsgpu_hits* out, uint32_t* n_tokens_matched, uint64_t* n_infix_ids,
                                        tsgpu_id_lists** ids_out) {
    if (ids_out) *ids_out = nullptr;
    if (!ctx || !out) return fail(TSGPU_ERR_INVALID, "tsgpu_infix_search_batch: NULL argument");
    if (out->mem != TSGPU_MEM_HOST) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_infix_search_batch: host outputs only");
    if (ctx->doc_range_set) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_infix_search_batch: not served on a doc-range shard");
    std::unique_ptr<tsgpu_id_lists> lists;
    if (ids_out) { lists.reset(new (std::nothrow) tsgpu_id_lists); if (!lists) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_infix_search_batch: host allocation failed"); }
    try {
        if (lists) lists->begin.assign((size_t)n_queries + 1, 0);
        if (n_queries) {
            if (!queries) return fail(TSGPU_ERR_INVALID, "tsgpu_infix_search_batch: queries is NULL");
            if (!out->keys || !out->scores || !out->n_hits || !out->status) return fail(TSGPU_ERR_INVALID, "tsgpu_infix_search_batch: missing output arrays");
            if (const int rc = infix_batch(ctx, queries, n_queries, out, n_tokens_matched, n_infix_ids, lists.get())) return rc;
        }
    } catch (const std::bad_alloc&) { return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_infix_search_batch: host allocation failed"); }
    if (ids_out) *ids_out = lists.release();
    return ok();
}

// ---------------------------------------------------------------- phrase search (kw_phrase.hip.h)
namespace {
enum PhraseBuf { PB_UBITS, PB_FBITS, PB_QBITS, PB_XBITS, PB_FOUND, PB_FIELDS, PB_PAIR_FIRST, PB_NACC, PB_CLIST, PB_PAIR_OFF, PB_PAIR_NIDS, PB_CHUNK_P, PB_CHUNK_A, PB_CHUNK_B,
                 PB_ITEMS, PB_UNIT_OF, PB_AUX, PB_SEGS, PB_FSLOT, PB_IDS, PB_TM, PB_OFF, PB_NIDS };
const uint32_t PHRASE_ROUND_MAX_QUERIES = 8192;            // (pairs = queries x fields are grid.y of the bitmap kernels)

// the intersections of the round's multi-token phrases: the AND items through the keyword planner (plan_batch: probe order, the cut into work items, the
// hit-buffer groups) and its find kernels, kw_phrase_mark_kernel behind each find launch instead of the score kernel. Runs on the held lane's stream.
int phrase_find_mark(tsgpu_ctx* ctx, KwLane& L, hipStream_t s, const Snapshot& snap, const tsgpu_kw_query* kq, uint32_t m, const PhraseMarkArgs& pa) {
    Plan P; DevPlan DP;
    int rc;
    if ((rc = plan_batch(ctx, snap, kq, m, P, false, false))) return rc;
    for (uint32_t i = 0; i < m; i++) if (P.status[i] != TSGPU_OK) return fail(P.status[i], "tsgpu_phrase_search_batch: the planner refused an AND item");
    P.aux.push_back(0);
    HitTables H;
    if ((rc = plan_hit_tables(ctx, L, P, DP, H, true))) return rc;
    KwStaged T;
    if ((rc = upload_plan_image(L, s, P, DP, H, T))) return rc;
    if ((rc = reserve_partials(L, (size_t)std::max<size_t>(H.first[5], 1) + P.groups.size(), 1, T.part))) return rc;
    LaunchStats st;
    return launch_batch(ctx, L, s, snap, P, H, T, 512, m, false, false, false, st, &pa);
}

// the hits of ranked queries kq[j] (query q_of[j] of the call) into the caller's arrays
int phrase_rank(tsgpu_ctx* ctx, std::vector<tsgpu_kw_query>& kq, const std::vector<uint64_t>& wild, const std::vector<uint64_t>& tmv, const std::vector<uint32_t>& q_of,
                uint32_t n_queries, tsgpu_hits* out) {
    const uint32_t m = (uint32_t)kq.size();
    int rc;
    if (m == 0) return TSGPU_OK;
    if (m == n_queries) return infix_rank(ctx, kq.data(), m, out, wild.data(), tmv.data());       // every query of the call, in order: straight into the caller's arrays
    const size_t ks = out->k_stride;
    std::vector<uint64_t> keys(m * ks), nm(m);
    std::vector<int64_t> scores(m * ks * 3), tm(m * ks);
    std::vector<float> vd(m * ks);
    std::vector<int8_t> msi(m * ks);
    std::vector<uint32_t> nh(m);
    std::vector<int32_t> st(m), co(m);
    tsgpu_hits tmp{TSGPU_MEM_HOST, out->k_stride, keys.data(), scores.data(), tm.data(), vd.data(), msi.data(), nh.data(), nm.data(), st.data(), co.data()};
    if ((rc = infix_rank(ctx, kq.data(), m, &tmp, wild.data(), tmv.data()))) return rc;
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = q_of[j];
        const size_t n = std::min<size_t>(nh[j], ks);
        std::copy(keys.begin() + j * ks, keys.begin() + j * ks + n, out->keys + i * ks);
        std::copy(scores.begin() + j * ks * 3, scores.begin() + (j * ks + n) * 3, out->scores + i * ks * 3);
        if (out->text_match) std::copy(tm.begin() + j * ks, tm.begin() + j * ks + n, out->text_match + i * ks);
        if (out->vector_distance) std::copy(vd.begin() + j * ks, vd.begin() + j * ks + n, out->vector_distance + i * ks);
        if (out->match_score_index) std::copy(msi.begin() + j * ks, msi.begin() + j * ks + n, out->match_score_index + i * ks);
        out->n_hits[i] = nh[j]; out->status[i] = st[j];
        if (out->num_matched) out->num_matched[i] = nm[j];
        if (out->search_cutoff) out->search_cutoff[i] = co[j];
    }
    return TSGPU_OK;
}

int phrase_batch(tsgpu_ctx* ctx, const tsgpu_phrase_query* queries, uint32_t n_queries, tsgpu_hits* out, std::vector<int32_t>& status, uint64_t* n_phrase_ids, tsgpu_id_lists* lists) {
    for (uint32_t i = 0; i < n_queries; i++) {
        status[i] = TSGPU_OK;
        if (out) {
            out->n_hits[i] = 0;
            if (out->num_matched) out->num_matched[i] = 0;
            if (out->search_cutoff) out->search_cutoff[i] = 0;
        }
        if (n_phrase_ids) n_phrase_ids[i] = 0;
    }
    std::lock_guard<std::mutex> lk(ctx->phrase_mu);            // one front at a time: it owns the scratch below
    (void)hipSetDevice(ctx->device);
    DevBuf* B = ctx->phrase_buf;
    const std::shared_ptr<const Snapshot> sn = ctx->snapshot();
    const uint64_t now = now_us();
    const bool timing = ctx->phrase_timing;
    const uint32_t cut = ctx->phrase_weight_cut;
    int rc;

    // ---- the queries' own checks
    std::vector<uint32_t> active;
    for (uint32_t i = 0; i < n_queries; i++) {
        const tsgpu_phrase_query& q = queries[i];
        int st = TSGPU_OK;
        if (q.mode > TSGPU_PHRASE_EXCLUDE || q.n_fields == 0 || q.n_fields > TSGPU_MAX_PHRASE_FIELDS || q.n_sort > TSGPU_MAX_SORT_KEYS) st = TSGPU_ERR_INVALID;
        else if (q.mode != TSGPU_PHRASE_EXCLUDE && ((q.n_filter && !q.filter_ids) || (q.n_excluded && !q.excluded_ids))) st = TSGPU_ERR_INVALID;
        for (uint32_t f = 0; st == TSGPU_OK && f < q.n_fields; f++) if (sn->field_is_array.find(q.field_ids[f]) == sn->field_is_array.end()) st = TSGPU_ERR_INVALID;
        for (uint32_t f = 0; st == TSGPU_OK && f < q.n_fields; f++) {
            if (q.n_phrases[f] > TSGPU_MAX_PHRASES) { st = TSGPU_ERR_UNSUPPORTED; break; }
            for (uint32_t p = 0; p < q.n_phrases[f]; p++) {
                if (q.phrases[f][p].n_tokens == 0) { st = TSGPU_ERR_INVALID; break; }
                if (q.phrases[f][p].n_tokens > TSGPU_MAX_QUERY_TOKENS) st = TSGPU_ERR_UNSUPPORTED;
            }
        }
        if (st == TSGPU_OK && q.mode == TSGPU_PHRASE_RANK) st = check_sort_slots(ctx, q.sort, q.n_sort, false, false, nullptr);
        if (st == TSGPU_OK && q.deadline_us != 0 && now > q.deadline_us) { st = TSGPU_ERR_DEADLINE; if (out && out->search_cutoff) out->search_cutoff[i] = 1; }
        status[i] = st;
        if (st == TSGPU_OK) active.push_back(i);
    }

    // ---- per query: its (field, phrase) units — a phrase with a token that has no posting list has none (:5950-5953) — and an upper bound of its id list
    struct Unit { uint32_t T; uint32_t field; uint32_t h[TSGPU_MAX_QUERY_TOKENS]; const tsgpu_phrase* ph; };
    const uint32_t num_docs = sn->num_docs;
    const uint64_t words = ((uint64_t)num_docs + 31) / 32;
    std::vector<std::vector<Unit>> units_of(n_queries);
    std::vector<std::vector<uint32_t>> units_per_field(n_queries);        // [field] -> units of that field (in phrase order, contiguous in units_of)
    std::vector<uint64_t> cap_of(n_queries, 0);
    for (uint32_t i : active) {
        const tsgpu_phrase_query& q = queries[i];
        units_per_field[i].assign(q.n_fields, 0);
        uint64_t sum = 0;
        for (uint32_t f = 0; f < q.n_fields; f++)
            for (uint32_t p = 0; p < q.n_phrases[f]; p++) {
                const tsgpu_phrase& ph = q.phrases[f][p];
                Unit u; u.T = ph.n_tokens; u.field = q.field_ids[f]; u.ph = &ph;
                bool all = true;
                uint64_t shortest = ~0ull;
                for (uint32_t t = 0; t < ph.n_tokens && all; t++) {
                    u.h[t] = sn->find_handle(q.field_ids[f], ph.term_ids[t]);
                    all = u.h[t] != 0xFFFFFFFFu && sn->h_lists[u.h[t]].n_blocks != 0;
                    if (all) shortest = std::min<uint64_t>(shortest, sn->h_lists[u.h[t]].n_ids);
                }
                if (!all) continue;
                units_of[i].push_back(u); units_per_field[i][f]++;
                sum += shortest;
            }
        cap_of[i] = std::min<uint64_t>(sum, words * 32);
    }
    if (words == 0) active.clear();                          // (no documents: nothing matches, status 0)

    std::vector<std::vector<uint32_t>> ids_host(lists ? n_queries : 0);
    const IndexViewLists ivl{sn->lists.as<ListDesc>(), sn->ar ? sn->ar->blk_ids.as<BlockIds>() : nullptr, sn->ar ? sn->ar->ids_payload.as<uint32_t>() : nullptr};
    const uint32_t n_chunks = (uint32_t)((words + INFIX_EXPAND_WORDS - 1) / INFIX_EXPAND_WORDS);
    for (size_t a0 = 0; a0 < active.size();) {
        // ---- the round: the queries whose scratch fits
        size_t a1 = a0;
        uint64_t bytes = 0;
        while (a1 < active.size() && a1 - a0 < PHRASE_ROUND_MAX_QUERIES) {
            const uint32_t i = active[a1];
            const tsgpu_phrase_query& q = queries[i];
            const uint64_t n_pairs_q = q.mode == TSGPU_PHRASE_EXCLUDE ? 1 : q.n_fields;
            const uint64_t need = words * 4 * (units_of[i].size() + n_pairs_q + 1 + (q.mode != TSGPU_PHRASE_EXCLUDE && q.filter_ids ? 1 : 0)) + n_pairs_q * cut * 4ull + cap_of[i] * 12;
            if (a1 > a0 && bytes + need > ctx->phrase_round_max_bytes) break;
            bytes += need; a1++;
        }
        const uint32_t nr = (uint32_t)(a1 - a0);
        ctx->phrase_rounds.fetch_add(1);
        std::vector<PhraseFieldDev> pairs;
        std::vector<uint32_t> pair_first(nr + 1, 0), unit_of_item, aux, fslot(nr, INFIX_NO_POS);
        std::vector<tsgpu_kw_query> and_items;
        std::vector<InfixMarkItem> mark_items;
        std::vector<InfixIdSeg> segs_f, segs_x;
        std::vector<uint64_t> off_cap, caps;
        uint32_t n_units = 0, nf = 0;
        uint64_t ids_total = 0;
        bool any_rank = false;
        for (uint32_t slot = 0; slot < nr; slot++) {
            const uint32_t i = active[a0 + slot];
            const tsgpu_phrase_query& q = queries[i];
            const bool excl = q.mode == TSGPU_PHRASE_EXCLUDE;
            any_rank = any_rank || q.mode == TSGPU_PHRASE_RANK;
            pair_first[slot] = (uint32_t)pairs.size();
            if (excl) pairs.push_back(PhraseFieldDev{n_units, (uint32_t)units_of[i].size(), q.mode, 0});
            else {
                uint32_t first = n_units;
                for (uint32_t f = 0; f < q.n_fields; f++) { pairs.push_back(PhraseFieldDev{first, units_per_field[i][f], q.mode, q.field_weights[f]}); first += units_per_field[i][f]; }
            }
            for (const Unit& u : units_of[i]) {
                const uint32_t unit = n_units++;
                if (u.T == 1) {                                // get_phrase_matches passes every id of the list (:1796-1800)
                    const uint32_t nb = sn->h_lists[u.h[0]].n_blocks;
                    for (uint32_t b = 0; b < nb; b += INFIX_MARK_BLOCKS) mark_items.push_back(InfixMarkItem{unit, u.h[0], b, std::min(nb, b + INFIX_MARK_BLOCKS)});
                } else {
                    tsgpu_kw_query k;
                    memset(&k, 0, sizeof k);
                    k.n_tokens = u.T;
                    for (uint32_t t = 0; t < u.T; t++) k.term_ids[t] = u.ph->term_ids[t];
                    k.n_fields = 1; k.field_ids[0] = u.field;
                    k.topster_size = 1;
                    and_items.push_back(k); unit_of_item.push_back(unit);
                }
            }
            if (!excl && q.filter_ids) {
                fslot[slot] = nf;
                if (q.n_filter) { segs_f.push_back(InfixIdSeg{aux.size(), q.n_filter, nf}); aux.insert(aux.end(), q.filter_ids, q.filter_ids + q.n_filter); }
                nf++;
            }
            if (!excl && q.n_excluded) { segs_x.push_back(InfixIdSeg{aux.size(), q.n_excluded, slot}); aux.insert(aux.end(), q.excluded_ids, q.excluded_ids + q.n_excluded); }
            off_cap.push_back(ids_total); caps.push_back(cap_of[i]);
            ids_total += cap_of[i];
        }
        const uint32_t n_pairs = (uint32_t)pairs.size();
        pair_first[nr] = n_pairs;
        off_cap.insert(off_cap.end(), caps.begin(), caps.end());
        std::vector<uint64_t> pair_off_cap(2 * (size_t)n_pairs);
        for (uint32_t p = 0; p < n_pairs; p++) { pair_off_cap[p] = (uint64_t)p * cut; pair_off_cap[n_pairs + p] = cut; }
        std::vector<InfixIdSeg> segs(segs_f);
        segs.insert(segs.end(), segs_x.begin(), segs_x.end());
        ctx->phrase_items.fetch_add(n_units);
        if (!and_items.empty() && !ctx->kw_two_kernels) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_phrase_search_batch: needs the two-kernel keyword form (option kw_two_kernels)");

        // ---- the device side of the round, on the stream of one lane held until the front's sync (the find kernels use the lane's tables and hit buffer)
        std::vector<uint32_t> nids(nr), chunk_a((size_t)nr * n_chunks);
        unsigned long long stats[2] = {0, 0};
        {
            LaneLock ll(ctx, tsgpu::tls_avoid_lane0() ? -2 : -1);
            KwLane& L = *ll.L;
            hipStream_t s = L.stream;
            const size_t nu = std::max<uint32_t>(n_units, 1);
            if ((rc = B[PB_UBITS].reserve(nu * words * 4)) || (rc = B[PB_FBITS].reserve((size_t)n_pairs * words * 4)) || (rc = B[PB_QBITS].reserve((size_t)nr * words * 4)) ||
                (rc = B[PB_XBITS].reserve((size_t)std::max<uint32_t>(nf, 1) * words * 4)) || (rc = B[PB_FOUND].reserve((nu + 2) * 8)) ||
                (rc = upload(B[PB_FIELDS], pairs.data(), pairs.size() * sizeof(PhraseFieldDev), s)) || (rc = upload(B[PB_PAIR_FIRST], pair_first.data(), pair_first.size() * 4, s)) ||
                (rc = B[PB_NACC].reserve((size_t)n_pairs * 4)) || (rc = B[PB_CLIST].reserve((size_t)n_pairs * cut * 4)) ||
                (rc = upload(B[PB_PAIR_OFF], pair_off_cap.data(), pair_off_cap.size() * 8, s)) || (rc = B[PB_PAIR_NIDS].reserve((size_t)n_pairs * 4)) ||
                (rc = B[PB_CHUNK_P].reserve((size_t)n_pairs * n_chunks * 4)) || (rc = B[PB_CHUNK_A].reserve((size_t)nr * n_chunks * 4)) || (rc = B[PB_CHUNK_B].reserve((size_t)nr * n_chunks * 4)) ||
                (rc = upload(B[PB_ITEMS], mark_items.data(), mark_items.size() * sizeof(InfixMarkItem), s)) || (rc = upload(B[PB_UNIT_OF], unit_of_item.data(), unit_of_item.size() * 4, s)) ||
                (rc = upload(B[PB_AUX], aux.data(), aux.size() * 4, s)) || (rc = upload(B[PB_SEGS], segs.data(), segs.size() * sizeof(InfixIdSeg), s)) ||
                (rc = upload(B[PB_FSLOT], fslot.data(), fslot.size() * 4, s)) || (rc = upload(B[PB_OFF], off_cap.data(), off_cap.size() * 8, s)) ||
                (rc = B[PB_IDS].reserve((size_t)std::max<uint64_t>(ids_total, 1) * 4)) || (rc = B[PB_TM].reserve((size_t)std::max<uint64_t>(ids_total, 1) * 8)) ||
                (rc = B[PB_NIDS].reserve((size_t)nr * 4))) return rc;
            TSGPU_HIP_TRY(hipMemsetAsync(B[PB_UBITS].p, 0, nu * words * 4, s));
            TSGPU_HIP_TRY(hipMemsetAsync(B[PB_FBITS].p, 0, (size_t)n_pairs * words * 4, s));
            TSGPU_HIP_TRY(hipMemsetAsync(B[PB_FOUND].p, 0, (nu + 2) * 8, s));
            if (nf) TSGPU_HIP_TRY(hipMemsetAsync(B[PB_XBITS].p, 0, (size_t)nf * words * 4, s));
            uint32_t* ubits = B[PB_UBITS].as<uint32_t>();
            uint32_t* fbits = B[PB_FBITS].as<uint32_t>();
            uint32_t* qbits = B[PB_QBITS].as<uint32_t>();
            unsigned long long* found = B[PB_FOUND].as<unsigned long long>();
            uint64_t t_ph = 0;
            if (timing) { TSGPU_HIP_TRY(hipStreamSynchronize(s)); t_ph = now_us(); }
            if (!and_items.empty()) {
                const PhraseMarkArgs pa{B[PB_UNIT_OF].as<uint32_t>(), ubits, words, found, found + nu};
                if ((rc = phrase_find_mark(ctx, L, s, *sn, and_items.data(), (uint32_t)and_items.size(), pa))) { (void)hipStreamSynchronize(s); return rc; }
            }
            if (!mark_items.empty())
                hipLaunchKernelGGL(infix_union_mark_kernel, dim3((uint32_t)mark_items.size()), dim3(INFIX_THREADS), 0, s, B[PB_ITEMS].as<InfixMarkItem>(), ivl.lists, ivl.blk_ids, ivl.ids_payload,
                                   ubits, words, found);
            if (timing) { TSGPU_HIP_TRY(hipStreamSynchronize(s)); const uint64_t t = now_us(); ctx->phrase_mark_us.fetch_add(t - t_ph); t_ph = t; }
            hipLaunchKernelGGL(phrase_fold_kernel, dim3(n_pairs), dim3(PHRASE_THREADS), 0, s, B[PB_FIELDS].as<PhraseFieldDev>(), ubits, found, fbits, words, B[PB_NACC].as<uint32_t>());
            if (any_rank) {                                    // the first `cut` ids of every folded field: the ids that get the field's weight score
                hipLaunchKernelGGL(infix_count_kernel, dim3(n_chunks, n_pairs), dim3(INFIX_THREADS), 0, s, fbits, words, B[PB_CHUNK_P].as<uint32_t>());
                hipLaunchKernelGGL(infix_expand_kernel, dim3(n_chunks, n_pairs), dim3(INFIX_THREADS), 0, s, fbits, words, B[PB_CHUNK_P].as<uint32_t>(), B[PB_CLIST].as<uint32_t>(),
                                   B[PB_PAIR_OFF].as<uint64_t>(), B[PB_PAIR_OFF].as<uint64_t>() + n_pairs, B[PB_PAIR_NIDS].as<uint32_t>());
            }
            hipLaunchKernelGGL(phrase_or_fields_kernel, dim3((uint32_t)((words + PHRASE_THREADS - 1) / PHRASE_THREADS), nr), dim3(PHRASE_THREADS), 0, s, fbits, B[PB_PAIR_FIRST].as<uint32_t>(), qbits, words);
            if (!segs_x.empty())
                hipLaunchKernelGGL(infix_idlist_clear_kernel, dim3((uint32_t)segs_x.size(), 8), dim3(INFIX_THREADS), 0, s, B[PB_AUX].as<uint32_t>(), B[PB_SEGS].as<InfixIdSeg>() + segs_f.size(), qbits, words);
            hipLaunchKernelGGL(infix_count_kernel, dim3(n_chunks, nr), dim3(INFIX_THREADS), 0, s, qbits, words, B[PB_CHUNK_A].as<uint32_t>());      // after exclusion, before the filter: n_phrase_ids
            uint32_t* chunk_final = B[PB_CHUNK_A].as<uint32_t>();
            if (nf) {
                if (!segs_f.empty())
                    hipLaunchKernelGGL(infix_idlist_set_kernel, dim3((uint32_t)segs_f.size(), 8), dim3(INFIX_THREADS), 0, s, B[PB_AUX].as<uint32_t>(), B[PB_SEGS].as<InfixIdSeg>(), B[PB_XBITS].as<uint32_t>(), words);
                hipLaunchKernelGGL(infix_bits_and_kernel, dim3((uint32_t)((words + INFIX_THREADS - 1) / INFIX_THREADS), nr), dim3(INFIX_THREADS), 0, s, qbits, B[PB_XBITS].as<uint32_t>(),
                                   B[PB_FSLOT].as<uint32_t>(), words);
                chunk_final = B[PB_CHUNK_B].as<uint32_t>();
                hipLaunchKernelGGL(infix_count_kernel, dim3(n_chunks, nr), dim3(INFIX_THREADS), 0, s, qbits, words, chunk_final);
            }
            hipLaunchKernelGGL(infix_expand_kernel, dim3(n_chunks, nr), dim3(INFIX_THREADS), 0, s, qbits, words, chunk_final, B[PB_IDS].as<uint32_t>(), B[PB_OFF].as<uint64_t>(),
                               B[PB_OFF].as<uint64_t>() + nr, B[PB_NIDS].as<uint32_t>());
            if (any_rank)
                hipLaunchKernelGGL(phrase_tm_kernel, dim3(32, nr), dim3(PHRASE_THREADS), 0, s, B[PB_IDS].as<uint32_t>(), B[PB_OFF].as<uint64_t>(), B[PB_OFF].as<uint64_t>() + nr,
                                   B[PB_NIDS].as<uint32_t>(), B[PB_PAIR_FIRST].as<uint32_t>(), B[PB_FIELDS].as<PhraseFieldDev>(), B[PB_NACC].as<uint32_t>(), B[PB_CLIST].as<uint32_t>(), cut,
                                   B[PB_TM].as<int64_t>());
            TSGPU_HIP_TRY(hipGetLastError());
            TSGPU_HIP_TRY(hipMemcpyAsync(nids.data(), B[PB_NIDS].p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(chunk_a.data(), B[PB_CHUNK_A].p, (size_t)nr * n_chunks * 4, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipMemcpyAsync(stats, found + nu, 16, hipMemcpyDeviceToHost, s));
            TSGPU_HIP_TRY(hipStreamSynchronize(s));
            ctx->phrase_syncs.fetch_add(1);
            if (timing) ctx->phrase_fold_us.fetch_add(now_us() - t_ph);
            ctx->phrase_records_checked.fetch_add(stats[0]); ctx->phrase_records_matched.fetch_add(stats[1]);

            // the surviving ids: to the caller's list object here; the ranked queries' stay on the device for the wildcard ranking below
            bool copied = false;
            for (uint32_t slot = 0; slot < nr; slot++) {
                const uint32_t i = active[a0 + slot];
                if (nids[slot] > caps[slot]) return fail(TSGPU_ERR_DEVICE, "tsgpu_phrase_search_batch: an id list beyond its bound");
                uint64_t before_filter = 0;
                for (uint32_t c = 0; c < n_chunks; c++) before_filter += chunk_a[(size_t)slot * n_chunks + c];
                if (n_phrase_ids) n_phrase_ids[i] = before_filter;
                if (lists && nids[slot]) {
                    ids_host[i].resize(nids[slot]);
                    TSGPU_HIP_TRY(hipMemcpyAsync(ids_host[i].data(), B[PB_IDS].as<uint32_t>() + off_cap[slot], (size_t)nids[slot] * 4, hipMemcpyDeviceToHost, s));
                    copied = true;
                }
            }
            if (lists) { if (copied) TSGPU_HIP_TRY(hipStreamSynchronize(s)); ctx->phrase_syncs.fetch_add(1); }
        }

        // ---- ranking (mode RANK): the id list and its text scores, both still on the device, through the wildcard machinery
        std::vector<tsgpu_kw_query> kq;
        std::vector<uint64_t> wild, tmv;
        std::vector<uint32_t> q_of;
        for (uint32_t slot = 0; slot < nr; slot++) {
            const uint32_t i = active[a0 + slot];
            const tsgpu_phrase_query& q = queries[i];
            if (q.mode != TSGPU_PHRASE_RANK || nids[slot] == 0) continue;
            const uint32_t* d_ids = B[PB_IDS].as<uint32_t>() + off_cap[slot];
            tsgpu_kw_query k;
            memset(&k, 0, sizeof k);
            k.n_sort = q.n_sort;
            for (uint32_t x = 0; x < q.n_sort; x++) k.sort[x] = q.sort[x];
            k.topster_size = q.topster_size;
            k.filter_ids = d_ids;                                  // (a device address: read through KwQueryDev::wild_ids only)
            k.n_filter = nids[slot];
            k.deadline_us = q.deadline_us;
            kq.push_back(k); wild.push_back((uint64_t)(uintptr_t)d_ids); tmv.push_back((uint64_t)(uintptr_t)(B[PB_TM].as<int64_t>() + off_cap[slot])); q_of.push_back(i);
        }
        const uint64_t t_rank = timing ? now_us() : 0;
        if (!kq.empty()) {
            if (!out) return fail(TSGPU_ERR_INVALID, "tsgpu_phrase_search_batch: a RANK query needs out");
            // (phrase_rank writes out->status of the ranked queries; the others keep theirs, copied to out by the caller)
            if ((rc = phrase_rank(ctx, kq, wild, tmv, q_of, n_queries, out))) return rc;
            for (uint32_t j = 0; j < (uint32_t)q_of.size(); j++) status[q_of[j]] = out->status[q_of[j]];
        }
        if (timing) ctx->phrase_rank_us.fetch_add(now_us() - t_rank);
        a0 = a1;
    }
    if (lists) {
        lists->begin.assign((size_t)n_queries + 1, 0);
        for (uint32_t i = 0; i < n_queries; i++) { lists->ids.insert(lists->ids.end(), ids_host[i].begin(), ids_host[i].end()); lists->begin[i + 1] = lists->ids.size(); }
    }
    return TSGPU_OK;
}
}  // namespace

extern "C" int tsgpu_phrase_search_batch(tsgpu_ctx* ctx, const tsgpu_phrase_query* queries, uint32_t n_queries, tsgpu_hits* out, uint64_t* n_phrase_ids, tsgpu_id_lists** ids_out) {
    if (ids_out) *ids_out = nullptr;
    if (!ctx) return fail(TSGPU_ERR_INVALID, "tsgpu_phrase_search_batch: NULL argument");
    if (out && out->mem != TSGPU_MEM_HOST) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_phrase_search_batch: host outputs only");
    if (ctx->doc_range_set) return fail(TSGPU_ERR_UNSUPPORTED, "tsgpu_phrase_search_batch: not served on a doc-range shard");
    std::unique_ptr<tsgpu_id_lists> lists;
    if (ids_out) { lists.reset(new (std::nothrow) tsgpu_id_lists); if (!lists) return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_phrase_search_batch: host allocation failed"); }
    try {
        if (lists) lists->begin.assign((size_t)n_queries + 1, 0);
        if (n_queries) {
            if (!queries) return fail(TSGPU_ERR_INVALID, "tsgpu_phrase_search_batch: queries is NULL");
            if (out && (!out->n_hits || !out->status)) return fail(TSGPU_ERR_INVALID, "tsgpu_phrase_search_batch: missing output arrays");
            bool any_rank = false;
            for (uint32_t i = 0; i < n_queries; i++) any_rank = any_rank || queries[i].mode == TSGPU_PHRASE_RANK;
            if (any_rank && (!out || !out->keys || !out->scores)) return fail(TSGPU_ERR_INVALID, "tsgpu_phrase_search_batch: a RANK query needs the output arrays");
            std::vector<int32_t> status(n_queries, TSGPU_OK);
            if (const int rc = phrase_batch(ctx, queries, n_queries, out, status, n_phrase_ids, lists.get())) return rc;
            if (out) for (uint32_t i = 0; i < n_queries; i++) out->status[i] = status[i];
            else for (uint32_t i = 0; i < n_queries; i++) if (status[i] != TSGPU_OK) return fail(status[i], "tsgpu_phrase_search_batch: a query was refused (no out to report it in)");
        }
    } catch (const std::bad_alloc&) { return fail(TSGPU_ERR_NO_MEMORY, "tsgpu_phrase_search_batch: host allocation failed"); }
    if (ids_out) *ids_out = lists.release();
    return ok();
}

#include "tsgpu_groupby.inc.h"
