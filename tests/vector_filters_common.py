"""Per-query filters in ONE exact k-NN batch (tsgpu_vec_knn_batch_filtered; vec_qmask_build_kernel, vec_direct_fill_kernel and the per-query-mask
instantiations of vec_hscan_kernel / vec_scan_kernel in vec_kernels.hip.h), the hybrid entry point that now runs one such batch, and the coalescer
that now takes filtered calls. Shared by tests/test_emu_vector_filters.py (SIMT emulator) and tests/test_gpu_vector_filters.py (MI355X).

What is compared, per query of a batch:
  * the oracle's flat scan restricted to `allow - excluded - deleted` (or `all live - excluded`), computed here in numpy: n_out, labels IN ORDER
    and distance BITS, no tolerance — on the bf16 bracket path (vec_prefilter = 1), whose survivors are re-scored in hnswlib's summation order. The
    fp32 MFMA scan (vec_prefilter = 0) sums in its own order (tests/test_emu_vector.py, module docstring): there the oracle comparison is the one
    that file uses for that scan — n_out, label SETS, distances within 1e-5 relative — because the parent's single-filter call does not give the
    oracle's bits on that scan either;
  * the library's own single-filter tsgpu_vec_knn_batch on that query alone: n_out, labels in order and distance bits, no tolerance, on BOTH scans
    (a score depends on one row and one query only).
Shapes: 1000 rows = 8 tiles of 128, the last with 104 rows (its last bitmap word holds 8 rows); 129 rows = a tile with one row; dims 48 (16-byte
aligned rows) and 70 (unaligned loads); 3 / 70 / 130 queries = vec_hscan_kernel<1> / <2> / <4> and both vec_scan_kernel widths."""
import threading

import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O
from tests import helpers as H

RTOL = 1e-5
DIRECT_DEFAULT = 65536


def build(lib, n, dim, metric, seed, labels=None, deleted=()):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    labels = np.arange(n, dtype=np.uint64) if labels is None else np.asarray(labels, np.uint64)
    g = T.GpuIndex(0, lib)
    g.vec_create(1, dim, metric)
    g.vec_upsert(1, labels, X)
    orc = O.OracleIndex(1, 1)
    orc.vec_init(dim, metric)
    orc.vec_add(labels.astype(np.uint32), X)
    for d in deleted:
        g.vec_delete(1, int(d))
    live = np.setdiff1d(labels.astype(np.uint32), np.asarray(deleted, np.uint32))
    return g, orc, rng, labels.astype(np.uint32), live


def mixed_filters(rng, labels, deleted, n_q, k, short):
    """one filter per query, every one different; the eight kinds of the issue in rotation. `short` = length of the allow list shorter than k"""
    n = labels.size
    unknown = np.array([int(labels.max()) + 5, int(labels.max()) + 1000, 0xFFFFFFF0], np.uint32)
    out = []
    for i in range(n_q):
        kind = i % 8
        pick = lambda m: np.sort(rng.choice(labels, size=max(1, min(n, m)), replace=False)).astype(np.uint32)
        if kind == 0:
            f = None                                                        # no filter
        elif kind == 1:
            f = (pick(n // 3 + i), None)                                    # allow only
        elif kind == 2:
            f = (None, pick(n // 4 + i))                                    # excluded only
        elif kind == 3:
            a = pick(n // 2 + i)
            f = (a, np.sort(np.concatenate([a[::3], pick(n // 10)[:20]])).astype(np.uint32))       # both, overlapping
            f = (f[0], np.unique(f[1]))
        elif kind == 4:
            f = (np.zeros(0, np.uint32), None)                              # filtered, nothing allowed: zero hits
        elif kind == 5:
            f = (pick(short - (i // 8) % 5), None)                          # fewer allowed rows than k: n_out < k
        elif kind == 6:
            f = (np.sort(labels), None)                                     # every row
        else:
            a = np.unique(np.concatenate([pick(n // 5 + i), np.asarray(deleted, np.uint32), unknown]))
            e = np.unique(np.concatenate([pick(n // 20 + 1), unknown[:1], np.asarray(deleted, np.uint32)[:1]]))
            f = (a.astype(np.uint32), e.astype(np.uint32))                  # deleted and unknown labels in both lists
        out.append(f)
    return out


def effective_allow(f, live, any_deleted):
    """the oracle takes allow lists only: allow - excluded (or all live - excluded), deleted / unknown labels dropped; None = no restriction"""
    if f is None:
        return live if any_deleted else None
    allow, excl = f
    eff = live if allow is None else np.intersect1d(allow, live)
    if excl is not None:
        eff = np.setdiff1d(eff, excl)
    return eff.astype(np.uint32)


def check_against_oracle(orc, Q, k, filters, live, any_deleted, res, bits, what=""):
    dist, lab, cnt = res
    for i in range(Q.shape[0]):
        eff = effective_allow(filters[i], live, any_deleted)
        if eff is not None and eff.size == 0:
            assert cnt[i] == 0, (what, i, cnt[i])
            continue
        d, l = orc.flat_knn(Q[i], k, allow_ids=eff)
        assert cnt[i] == d.size, (what, i, cnt[i], d.size)
        if bits:
            assert np.array_equal(lab[i, :d.size].astype(np.uint32), l), (what, i, lab[i, :8], l[:8])
            assert np.array_equal(dist[i, :d.size].view(np.uint32), d.view(np.uint32)), (what, i)
        else:
            assert set(lab[i, :d.size].astype(np.int64).tolist()) == set(l.astype(np.int64).tolist()), (what, i)
            assert np.allclose(dist[i, :d.size], d, rtol=RTOL, atol=RTOL), (what, i)
            assert (np.diff(dist[i, :d.size]) >= 0).all(), (what, i)


def _single_call(g, q, k, allow, excl):
    """tsgpu_vec_knn_batch on one query; an EMPTY allow list goes down as a non-NULL pointer with n_allow = 0 (GpuIndex.vec_knn_batch would pass NULL = no filter)"""
    if allow is None or allow.size:
        return g.vec_knn_batch(1, q, k, allow_ids=allow, excluded_ids=excl)
    import ctypes as C
    q = np.ascontiguousarray(q, np.float32)
    dist = np.zeros((1, k), np.float32); lab = np.zeros((1, k), np.uint64); cnt = np.zeros(1, np.uint32)
    dummy = np.zeros(1, np.uint32)
    e = None if excl is None else np.ascontiguousarray(excl, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    B.check(g.L, g.L.tsgpu_vec_knn_batch(g.h, 1, vp(q), B.MEM_HOST, 1, k, vp(dummy), 0, vp(e) if e is not None else None, e.size if e is not None else 0,
                                        vp(dist), vp(lab), vp(cnt), B.MEM_HOST))
    return dist, lab, cnt


def check_against_single_calls(g, Q, k, filters, res, what="", which=None):
    """every query (or the queries `which`) alone through the single-filter tsgpu_vec_knn_batch: same n_out, labels in order, distance bits"""
    dist, lab, cnt = res
    for i in (range(Q.shape[0]) if which is None else which):
        f = filters[i] or (None, None)
        d1, l1, c1 = _single_call(g, Q[i:i + 1], k, f[0], f[1])
        n = int(c1[0])
        assert cnt[i] == n, (what, i, cnt[i], n)
        assert np.array_equal(lab[i, :n], l1[0, :n]), (what, i)
        assert np.array_equal(dist[i, :n].view(np.uint32), d1[0, :n].view(np.uint32)), (what, i)


def same_results(a, b):
    (d0, l0, c0), (d1, l1, c1) = a, b
    if not np.array_equal(c0, c1):
        return False
    return all(np.array_equal(l0[i, :c0[i]], l1[i, :c0[i]]) and np.array_equal(d0[i, :c0[i]].view(np.uint32), d1[i, :c0[i]].view(np.uint32)) for i in range(c0.size))


def case_mixed_batch(lib, n, dim, metric, n_q, prefilter, sample_tiles, k, short, seed=1, single_calls=None):
    """the whole filter mix in one batch, on the three route settings: vec_filter_direct_max = 65 536 (every allow list goes the direct route),
    0 (every filtered query through the masked scan), 64 (both routes in one group: the permutation back to caller order).
    single_calls: how many queries are also run alone through the single-filter call (None = all of them; the emulator tier, where one call takes
    seconds, takes the first 16 = every filter kind twice, plus the last query = the one that shares its Q row)"""
    deleted = (3, 64, n - 1)
    g, orc, rng, labels, live = build(lib, n, dim, metric, seed + n + dim, deleted=deleted)
    g.set_option("vec_prefilter", prefilter)
    g.set_option("vec_sample_tiles", sample_tiles)
    Q = (rng.standard_normal((n_q, dim)) * 2).astype(np.float32)
    Q[n_q - 1] = Q[1]                                   # two queries share a Q row under different filters (3 / 70 queries: another kind of filter; 130: both allow-only, different lists)
    filters = mixed_filters(rng, labels, deleted, n_q, k, short)
    results = {}
    for dm in (DIRECT_DEFAULT, 0, 64):
        g.set_option("vec_filter_direct_max", dm)
        results[dm] = g.vec_knn_batch_filtered(1, Q, k, filters)
    assert same_results(results[DIRECT_DEFAULT], results[0]), "direct route and masked scan disagree"
    assert same_results(results[64], results[0]), "mixed-route group and masked scan disagree"
    check_against_oracle(orc, Q, k, filters, live, True, results[0], bits=bool(prefilter), what=(n, dim, n_q, prefilter))
    which = None if single_calls is None or single_calls >= n_q else list(range(single_calls)) + [n_q - 1]
    check_against_single_calls(g, Q, k, filters, results[DIRECT_DEFAULT], what=(n, dim, n_q, prefilter), which=which)
    if prefilter:
        assert g.counter("vec_prefilter_fallbacks") == 0
    # filters == NULL and a batch whose filters are all "none" are the unfiltered call
    plain = g.vec_knn_batch(1, Q[:3], k)
    assert same_results(g.vec_knn_batch_filtered(1, Q[:3], k, None), plain) and same_results(g.vec_knn_batch_filtered(1, Q[:3], k, [None] * 3), plain)
    orc.close()
    g.close()


def case_non_identity_labels(lib):
    """labels 3 i + 7 inserted in shuffled order: the lists are translated to rows on the host (find_row) and sorted. A group made only of direct
    queries launches no scan: neither bracket-path counter moves"""
    n, dim, k = 600, 48, 40
    rng0 = np.random.default_rng(5)
    labels = (3 * rng0.permutation(n) + 7).astype(np.uint64)
    deleted = (int(labels[10]), int(labels[300]))
    g, orc, rng, lab32, live = build(lib, n, dim, B.METRIC_IP, 77, labels=labels, deleted=deleted)
    Q = rng.standard_normal((9, dim)).astype(np.float32)
    filters = mixed_filters(rng, lab32, deleted, 9, k, 25)
    for dm in (DIRECT_DEFAULT, 0, 64):
        g.set_option("vec_filter_direct_max", dm)
        res = g.vec_knn_batch_filtered(1, Q, k, filters)
        check_against_oracle(orc, Q, k, filters, live, True, res, bits=True, what=("non-identity", dm))
        check_against_single_calls(g, Q, k, filters, res, what=("non-identity", dm))
    g.set_option("vec_filter_direct_max", DIRECT_DEFAULT)
    direct_only = [f for f in filters if f is not None and f[0] is not None]
    Qd = Q[:len(direct_only)]
    g0, f0 = g.counter("vec_prefilter_groups"), g.counter("vec_prefilter_fallbacks")
    res = g.vec_knn_batch_filtered(1, Qd, k, direct_only)
    assert (g.counter("vec_prefilter_groups"), g.counter("vec_prefilter_fallbacks")) == (g0, f0), "an all-direct group launched a scan"
    check_against_oracle(orc, Qd, k, direct_only, live, True, res, bits=True, what="all-direct")
    orc.close()
    g.close()


def _text_and_vectors(lib, n_docs=400, dim=24, seed=3):
    """the text + vector corpus of tests/test_emu_vector.py::_text_and_vectors"""
    docs = H.zipf_docs(n_docs, 60, 8, seed=seed)
    orc, g = H.build_pair(docs, lib)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_docs, dim)).astype(np.float32)
    g.vec_create(1, dim, B.METRIC_IP)
    g.vec_upsert(1, np.arange(n_docs, dtype=np.uint64), X)
    orc.vec_init(dim, O.METRIC_IP)
    orc.vec_add(np.arange(n_docs, dtype=np.uint32), X)
    return orc, g, rng


def case_hybrid_one_pass(lib):
    """40 hybrid queries with 40 different filter_ids at vec_filter_direct_max = 0: the fused Topsters equal the oracle's bit for bit, and the vector
    half ran as ONE filtered batch — at most 2 scan groups (bracket groups + fallbacks) instead of one per filtered query"""
    orc, g, rng = _text_and_vectors(lib)
    n_docs, nq = 400, 40
    Q = rng.standard_normal((nq, 24)).astype(np.float32)
    sort = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
    toks = [[1, 2], [3], [2, 5], [1, 2, 3], [59, 1], [7, 7], [4], [2, 9]]
    cases = []
    for i in range(nq):
        c = dict(filter_ids=np.sort(rng.choice(n_docs, size=60 + 5 * i, replace=False)).astype(np.uint32))
        if i % 5 == 0:
            c["excluded_ids"] = np.arange(i % 4, n_docs, 4, dtype=np.uint32)
        cases.append(c)
    qs = [T.KwQuery(toks[i % len(toks)], sort=sort, topster_size=0, **c) for i, c in enumerate(cases)]
    g.set_option("vec_filter_direct_max", 0)
    before = g.counter("vec_prefilter_groups") + g.counter("vec_prefilter_fallbacks")
    hits = g.hybrid_search_batch(qs, 1, Q, k=0, fetch_size=10, alpha=0.3, k_stride=250)
    passes = g.counter("vec_prefilter_groups") + g.counter("vec_prefilter_fallbacks") - before
    assert (hits.status == 0).all()
    for i, (q, c) in enumerate(zip(qs, cases)):
        oq = orc.make_query(q.tokens, sort=((O.SORT_TEXT_MATCH, 0, 1), (O.SORT_INT64_COLUMN, 0, 1)), fetch_size=10, **c)
        ref = orc.search_hybrid(oq, Q[i], k=0, alpha=0.3)
        n = int(hits.n_hits[i])
        assert n == ref.keys.size, (i, n, ref.keys.size)
        assert np.array_equal(hits.keys[i, :n], ref.keys), (i, hits.keys[i, :10], ref.keys[:10])
        assert np.array_equal(hits.scores[i, :n], ref.scores)
        assert np.array_equal(hits.text_match[i, :n], ref.text_match)
        assert np.allclose(hits.vector_distance[i, :n], ref.vector_distance, rtol=RTOL, atol=RTOL)
        assert np.isin(hits.keys[i, :n], c["filter_ids"]).all()
        if "excluded_ids" in c:
            assert not np.isin(hits.keys[i, :n], c["excluded_ids"]).any()
    assert passes <= 2, "the vector half of the hybrid batch ran %d scan passes" % passes
    g.close()


def case_filtered_calls_coalesce(lib):
    """8 host threads, each issuing 1-query calls with its own allow list: every answer equals the same call made alone, and the calls shared rounds"""
    n, dim, k, n_threads = 700, 48, 10, 8
    g, orc, rng, labels, live = build(lib, n, dim, B.METRIC_IP, 9)
    Q = rng.standard_normal((2 * n_threads, dim)).astype(np.float32)
    allow = [np.sort(rng.choice(n, size=40 + 17 * j, replace=False)).astype(np.uint32) for j in range(2 * n_threads)]
    want = [g.vec_knn_batch(1, Q[j:j + 1], k, allow_ids=allow[j]) for j in range(2 * n_threads)]
    g.set_option("batch_window_us", 20000)
    r0, c0 = g.counter("batch_rounds"), g.counter("batch_coalesced_calls")

    def worker(i):
        for j in (i, i + n_threads):
            got = g.vec_knn_batch(1, Q[j:j + 1], k, allow_ids=allow[j])
            assert same_results(got, want[j]), j
    _run_threads(n_threads, worker)
    rounds, calls = g.counter("batch_rounds") - r0, g.counter("batch_coalesced_calls") - c0
    assert calls > 0, "filtered calls bypassed the coalescer"
    assert rounds < calls, "no two filtered calls shared a round (%d rounds for %d calls)" % (rounds, calls)
    orc.close()
    g.close()


def _run_threads(n_threads, worker):
    """worker(i) on n_threads threads released together; an exception in any of them fails the test"""
    start = threading.Barrier(n_threads)
    errors = []

    def body(i):
        try:
            start.wait()
            worker(i)
        except BaseException as e:                       # noqa: BLE001 (reported by the main thread)
            errors.append(repr(e))
    th = [threading.Thread(target=body, args=(i,)) for i in range(n_threads)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def case_hybrid_calls_coalesce(lib):
    """8 host threads, each issuing 1-query hybrid calls (the server's calling convention), every second query with its own filter_ids, at
    vec_filter_direct_max = 0 so that every call needs a scan: each answer equals the same call made alone, and the vector passes of concurrent calls
    share rounds — fewer scan passes than calls (alone, every call runs one; the keyword halves coalesce too and feed the same batch_* counters, so the
    scan count is what pins the vector side)"""
    orc, g, rng = _text_and_vectors(lib)
    n_docs, n_threads = 400, 8
    n_calls = 2 * n_threads
    Q = rng.standard_normal((n_calls, 24)).astype(np.float32)
    sort = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
    toks = [[1, 2], [3], [2, 5], [1, 2, 3], [59, 1], [7, 7], [4], [2, 9]]
    qs = [T.KwQuery(toks[j % len(toks)], sort=sort, topster_size=0,
                    **({"filter_ids": np.sort(rng.choice(n_docs, size=80 + 9 * j, replace=False)).astype(np.uint32)} if j % 2 else {})) for j in range(n_calls)]
    g.set_option("vec_filter_direct_max", 0)
    call = lambda j: g.hybrid_search_batch([qs[j]], 1, Q[j:j + 1], k=0, fetch_size=10, alpha=0.3, k_stride=250)
    want = [call(j) for j in range(n_calls)]
    g.set_option("batch_window_us", 20000)
    scans = lambda: g.counter("vec_prefilter_groups") + g.counter("vec_prefilter_fallbacks")
    s0, c0 = scans(), g.counter("batch_coalesced_calls")

    def worker(i):
        for j in (i, i + n_threads):
            got, ref = call(j), want[j]
            n = int(ref.n_hits[0])
            assert int(got.n_hits[0]) == n and np.array_equal(got.keys[0, :n], ref.keys[0, :n]) and np.array_equal(got.scores[0, :n], ref.scores[0, :n]), j
            assert np.array_equal(got.vector_distance[0, :n].view(np.uint32), ref.vector_distance[0, :n].view(np.uint32)), j
    _run_threads(n_threads, worker)
    passes = scans() - s0
    assert g.counter("batch_coalesced_calls") - c0 > 0
    assert 0 < passes < n_calls, "concurrent 1-query hybrid calls did not share a vector pass (%d scan passes for %d calls)" % (passes, n_calls)
    g.close()
