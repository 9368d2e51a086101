"""Per-query filters in ONE HNSW search batch (tsgpu_vec_hnsw_search_batch_filtered; the PQ instantiations of vec_hnsw_search_kernel in
csrc/vec_kernels.hip.h, hnsw_device_filtered / hnsw_search_launch in csrc/tsgpu_vec.hip) and the coalescer of small HNSW calls. Shared by
tests/test_emu_hnsw_filters.py (SIMT emulator) and tests/test_gpu_hnsw_filters.py (MI355X).

Inputs follow tests/hnsw_traversal_common.py: rows and queries are small integers cast to fp32 (tie_rows), so every distance is exact and ties are
everywhere; graphs come from the oracle's builder (hnsw_build -> hnsw_export -> vec_hnsw_load) or are the hand-made ring lattice of that file, loaded
into both sides. The comparison is that file's: n_out, labels in order, distance BITS, no tolerance. Per query of a batch, against
  * the oracle's traversal of the same graph. The oracle takes allow lists only: a filter is reduced to its effective allow set
    (vector_filters_common.effective_allow: allow - excluded - deleted, or all live - excluded); an empty set answers nothing;
  * the library's own single-filter tsgpu_vec_hnsw_search_batch on that query alone.
Every body runs with option hnsw_visited_hash 0 (16-bit tags) and 1 (hash sets)."""
import atexit
import ctypes as C

import numpy as np
import pytest

from typesense_amd import _lib as B
from tests import hnsw_traversal_common as V
from tests import vector_filters_common as F

OVERFLOWED = V.OVERFLOWED
MODES = (0, 1)
DELETED = (3, 64, V.N_TIE - 1)
MIXED_K_EF = ((10, 64), (100, 128))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class LPair(V.Pair):
    """V.Pair with labels of the caller's choice (label != row: the field leaves identity mode, the lists go through find_row)"""

    def __init__(self, lib, X, labels, metric=B.METRIC_IP):
        import typesense_amd as T
        from oracle import oracle_py as O
        self.n = X.shape[0]
        self.g = T.GpuIndex(0, lib)
        self.g.vec_create(1, X.shape[1], metric)
        self.g.vec_upsert(1, np.asarray(labels, np.uint64), X)
        self.orc = O.OracleIndex(1, 1)
        self.orc.vec_init(X.shape[1], metric)
        self.orc.vec_add(np.asarray(labels, np.uint32), X)
        self._ref = {}


def search_filtered(p, mode, Q, k, ef, filters, functor=True):
    """mode None: the visited mode stays as it is set (concurrent callers do not touch the option)"""
    if mode is None:
        return p.g.vec_hnsw_search_batch_filtered(1, Q, k, ef, filters, functor_present=functor)
    p.g.set_option("hnsw_visited_hash", mode)
    try:
        return p.g.vec_hnsw_search_batch_filtered(1, Q, k, ef, filters, functor_present=functor)
    finally:
        p.g.set_option("hnsw_visited_hash", 1)


def single_call(p, mode, q, k, ef, f, functor=True):
    """tsgpu_vec_hnsw_search_batch on ONE query with the one filter f; an EMPTY allow list goes down as a non-NULL pointer with n_allow = 0
    (GpuIndex.vec_hnsw_search_batch would pass NULL = no filter)"""
    allow, excl = f or (None, None)
    q = np.ascontiguousarray(q, np.float32).reshape(1, -1)
    dist = np.zeros((1, k), np.float32); lab = np.zeros((1, k), np.uint64); cnt = np.zeros(1, np.uint32)
    dummy = np.zeros(1, np.uint32)
    a = None if allow is None else np.ascontiguousarray(allow, np.uint32)
    e = None if excl is None or not len(excl) else np.ascontiguousarray(excl, np.uint32)
    if mode is not None:
        p.g.set_option("hnsw_visited_hash", mode)
    try:
        B.check(p.g.L, p.g.L.tsgpu_vec_hnsw_search_batch(p.g.h, 1, _vp(q), B.MEM_HOST, 1, k, ef, int(functor),
                                                         None if a is None else _vp(a if a.size else dummy), 0 if a is None else a.size,
                                                         None if e is None else _vp(e), 0 if e is None else e.size, _vp(dist), _vp(lab), _vp(cnt), B.MEM_HOST))
    finally:
        if mode is not None:
            p.g.set_option("hnsw_visited_hash", 1)
    return dist, lab, cnt


class Singles:
    """every query of a batch alone through the single-filter call, once per (case, visited mode): the results stacked like a batch's, and what
    the counters said: layer-0 expansions / distances summed over the calls, queries re-run"""

    def __init__(self, p, mode, Q, k, ef, filters, functor=True):
        n = Q.shape[0]
        self.dist = np.zeros((n, k), np.float32); self.lab = np.zeros((n, k), np.uint64); self.cnt = np.zeros(n, np.uint32)
        self.expansions = self.distances = 0
        r0 = p.reruns()
        for i in range(n):
            d, l, c = single_call(p, mode, Q[i], k, ef, filters[i], functor)
            self.dist[i], self.lab[i], self.cnt[i] = d[0], l[0], c[0]
            self.expansions += p.g.counter("hnsw_last_expansions")
            self.distances += p.g.counter("hnsw_last_distances")
        self.reruns = p.reruns() - r0

    @property
    def res(self):
        return self.dist, self.lab, self.cnt


def equal_to_oracle(p, res, Q, k, ef, filters, live, any_deleted, functor=True, what=""):
    dist, lab, cnt = res
    for i in range(Q.shape[0]):
        eff = F.effective_allow(filters[i], live, any_deleted)
        if eff is not None and eff.size == 0:
            assert cnt[i] == 0, (what, i, int(cnt[i]))
            continue
        d, l = p.ref(Q, i, k, ef, eff, functor)
        assert cnt[i] == d.size, (what, i, int(cnt[i]), d.size)
        assert np.array_equal(lab[i, :d.size], l), (what, i, lab[i, :d.size][:12], l[:12])
        assert np.array_equal(dist[i, :d.size].view(np.uint32), d.view(np.uint32)), (what, i)


def n_restricting(filters):
    return sum(f is not None for f in filters)


# ---------------------------------------------------------------------------------------------------------------- 1 / 2 / 6. the mixed batch
class Mixed:
    """1 500 rows x 16 (the last bitmap word holds 28 rows, the last tile 92), M 8, three rows deleted on both sides; n_q queries in rounds of the
    eight filter kinds of vector_filters_common.mixed_filters. The single-filter calls of a (k, ef, mode) are made once and shared."""

    def __init__(self, lib, metric, n_q):
        X, Q = V.tie_rows("tri", n_q=n_q)
        self.p = V.Pair(lib, X, metric).build(8)
        for d in DELETED:
            self.p.delete(d)
        self.Q = Q
        self.labels = np.arange(V.N_TIE, dtype=np.uint32)
        self.live = np.setdiff1d(self.labels, np.asarray(DELETED, np.uint32))
        self._filters, self._singles = {}, {}

    def filters(self, k):
        if k not in self._filters:
            self._filters[k] = F.mixed_filters(np.random.default_rng(40 + k), self.labels, DELETED, self.Q.shape[0], k, short=max(5, (7 * k) // 10))
        return self._filters[k]

    def singles(self, mode, k, ef):
        if (mode, k, ef) not in self._singles:
            self._singles[(mode, k, ef)] = Singles(self.p, mode, self.Q, k, ef, self.filters(k))
        return self._singles[(mode, k, ef)]


_MIXED = {}


@atexit.register
def _close_mixed():
    """the shared pairs live as long as the session (read-only after their deletions); their contexts and oracles are released with it"""
    while _MIXED:
        _MIXED.popitem()[1].p.close()


def mixed(lib, metric, n_q):
    key = (lib, metric, n_q)
    if key not in _MIXED:
        _MIXED[key] = Mixed(lib, metric, n_q)
    return _MIXED[key]


def body_mixed_batch(lib, metric, k, ef, n_q=24):
    m = mixed(lib, metric, n_q)
    p, Q, filters = m.p, m.Q, m.filters(k)
    for mode in MODES:
        s = m.singles(mode, k, ef)
        # the premise, on the single-filter side first: no query of this case outgrows the largest tier
        assert not (s.cnt == OVERFLOWED).any(), ("premise: a single-filter call overflowed", mode, np.nonzero(s.cnt == OVERFLOWED)[0])
        equal_to_oracle(p, s.res, Q, k, ef, filters, m.live, True, what=("single-filter calls", mode, k, ef))
        res = search_filtered(p, mode, Q, k, ef, filters)
        assert not (res[2] == OVERFLOWED).any(), (mode, res[2])
        equal_to_oracle(p, res, Q, k, ef, filters, m.live, True, what=("one filtered batch", mode, k, ef))
        assert V.same_results(res, s.res), ("the batch and the single-filter calls disagree", mode, k, ef)
        short = [i for i, f in enumerate(filters) if i % 8 == 5]
        assert short and all(0 < res[2][i] < k for i in short) and all(res[2][i] == 0 for i in range(4, Q.shape[0], 8)), res[2]


def body_one_launch_same_traversal(lib, metric, k, ef, n_q=24):
    """the whole batch is ONE traversal launch that does, query for query, the work of the single-filter calls"""
    m = mixed(lib, metric, n_q)
    p, Q, filters = m.p, m.Q, m.filters(k)
    for mode in MODES:
        s = m.singles(mode, k, ef)
        assert s.reruns == 0, ("premise: a single-filter call left its tier", mode, s.reruns)
        l0, r0, m0 = p.g.counter("hnsw_launches"), p.reruns(), p.g.counter("hnsw_filter_maps")
        search_filtered(p, mode, Q, k, ef, filters)
        assert p.g.counter("hnsw_launches") - l0 == 1, (mode, p.g.counter("hnsw_launches") - l0)
        assert p.reruns() - r0 == 0
        assert p.g.counter("hnsw_filter_maps") - m0 == n_restricting(filters)
        assert p.g.counter("hnsw_last_expansions") == s.expansions, (mode, p.g.counter("hnsw_last_expansions"), s.expansions)
        assert p.g.counter("hnsw_last_distances") == s.distances, (mode, p.g.counter("hnsw_last_distances"), s.distances)


def body_group_split(lib, metric, k, ef, n_q=24, max_maps=5):
    """TESTS ONLY option hnsw_test_max_maps caps the bitmaps of one launch (the 4 GiB arena bound needs sizes no test should run): consecutive
    groups of queries with at most 5 maps each, one launch per group, Q / outputs / off[] offset by the group's start"""
    m = mixed(lib, metric, n_q)
    p, Q, filters = m.p, m.Q, m.filters(k)
    groups = -(-n_restricting(filters) // max_maps)         # greedy consecutive groups: every group but the last is full
    assert groups >= 2
    for mode in MODES:
        s = m.singles(mode, k, ef)                           # (first: every single-filter call overwrites the hnsw_last_* counters)
        whole = search_filtered(p, mode, Q, k, ef, filters)
        p.g.set_option("hnsw_test_max_maps", max_maps)
        try:
            l0, r0, m0 = p.g.counter("hnsw_launches"), p.reruns(), p.g.counter("hnsw_filter_maps")
            split = search_filtered(p, mode, Q, k, ef, filters)
            last = p.g.counter("hnsw_last_expansions"), p.g.counter("hnsw_last_distances")
            assert p.reruns() - r0 == 0
            assert p.g.counter("hnsw_launches") - l0 == groups, (mode, p.g.counter("hnsw_launches") - l0, groups)
            assert p.g.counter("hnsw_filter_maps") - m0 == n_restricting(filters)
        finally:
            p.g.set_option("hnsw_test_max_maps", 0)
        assert V.same_results(split, whole), ("split batch differs", mode)
        equal_to_oracle(p, split, Q, k, ef, filters, m.live, True, what=("split batch", mode))
        assert last == (s.expansions, s.distances), (mode, last, s.expansions, s.distances)     # (the counters describe the batch, not its last group)


# ---------------------------------------------------------------------------------------------------------------- 3. small and ragged shapes
def body_small_shape(lib, n, label_base=0, k=5, ef=16, n_q=10):
    """129 rows = one tile plus one row; 33 rows = one bitmap word plus one row; labels = row + 1000 = not identity mode. Among the filters: one
    whose only allowed row is the LAST row, one that excludes the entry point."""
    X, Q = V.tie_rows("tri", n=n, n_q=n_q)
    labels = np.arange(n, dtype=np.uint32) + label_base
    p = LPair(lib, X, labels).build(4)
    try:
        deleted = (int(labels[1]),)
        p.delete(deleted[0])
        live = np.setdiff1d(labels, np.asarray(deleted, np.uint32))
        entry = int(labels[p.orc.hnsw_export()["enterpoint"]])
        filters = F.mixed_filters(np.random.default_rng(50 + n), labels, deleted, n_q, k, short=4)
        filters[1] = (labels[-1:].copy(), None)                          # only the last row
        filters[2] = (None, np.array([entry], np.uint32))                # the entry point excluded
        filters[3] = (labels[-1:].copy(), np.array([entry], np.uint32))
        for mode in MODES:
            res = search_filtered(p, mode, Q, k, ef, filters)
            assert not (res[2] == OVERFLOWED).any()
            equal_to_oracle(p, res, Q, k, ef, filters, live, True, what=("small shape", n, label_base, mode))
            s = Singles(p, mode, Q, k, ef, filters)
            assert V.same_results(res, s.res), ("batch vs single-filter calls", n, label_base, mode)
            assert res[2][1] == 1 and res[1][1, 0] == labels[-1] and not (res[1][2, :res[2][2]] == entry).any()
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 4. masks through the re-run ladder
def body_masks_through_the_rerun_ladder(lib, n=5000):
    """The 5 000-node ring lattice of hnsw_traversal_common.body_visited_set_past_half_full. Query 1 is filtered down to 3 rows on the far side: its
    result heap never fills, the strict stop rule walks the ring, its visited set passes half of the smallest tier's 8 192 words and it runs again on
    the largest tier THROUGH q_sel — as query 0 of that launch, with the map of query 1 of the batch. It sits between an unfiltered query and one
    with another filter. The number of re-runs expected is what the single-filter calls needed."""
    p, Q, graph = V.lattice_pair(lib, n, 16, 2, 2, 25, 3)
    try:
        far = V._far_side(graph, n, 3)
        other = np.sort(np.random.default_rng(61).choice(n, size=n // 3, replace=False)).astype(np.uint32)
        filters = [None, (far, None), (other, np.arange(0, n, 7, dtype=np.uint32))]
        live = np.arange(n, dtype=np.uint32)
        for mode in MODES:
            s = Singles(p, mode, Q, 10, 10, filters)
            if mode == 1:
                assert s.reruns >= 1, "premise: the filtered query's single-filter call never left its tier"
            r0, l0 = p.reruns(), p.g.counter("hnsw_launches")
            res = search_filtered(p, mode, Q, 10, 10, filters)
            assert p.reruns() - r0 == s.reruns, (mode, p.reruns() - r0, s.reruns)
            assert p.g.counter("hnsw_launches") - l0 == (2 if s.reruns else 1)
            equal_to_oracle(p, res, Q, 10, 10, filters, live, False, what=("re-run ladder", mode))
            assert V.same_results(res, s.res), mode
            assert res[2][1] == 3 and np.array_equal(np.sort(res[1][1, :3]), far)
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 5. several queries per block
def body_several_queries_per_block(lib, k=5, ef=12, n_q=20):
    """hnsw_test_slots = 3: every block serves 6 or 7 queries with different maps one after the other"""
    p, Q = V.slots_pair(lib)
    try:
        Q = Q[:n_q]
        labels = np.arange(p.n, dtype=np.uint32)
        filters = F.mixed_filters(np.random.default_rng(71), labels, (), n_q, k, short=4)
        singles = {mode: Singles(p, mode, Q, k, ef, filters) for mode in MODES}
        p.g.set_option("hnsw_test_slots", 3)
        for mode in MODES:
            res = search_filtered(p, mode, Q, k, ef, filters)
            equal_to_oracle(p, res, Q, k, ef, filters, labels, False, what=("3 slots", mode))
            assert V.same_results(res, singles[mode].res), mode
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the coalescer
def body_calls_coalesce(lib, n_threads=8, k=5, ef=16):
    """8 threads released together, each with ONE 1-query call and its own filter, half through tsgpu_vec_hnsw_search_batch (its one filter), half
    through the filtered entry point: every answer equals the same call made alone; the calls shared rounds of the HNSW combiner, whose counters
    are its own (batch_rounds / batch_coalesced_calls do not move); a lone caller never parks."""
    X, Q = V.tie_rows("tri", n=300, n_q=n_threads)
    p = V.Pair(lib, X).build(4)
    try:
        labels = np.arange(p.n, dtype=np.uint32)
        filters = F.mixed_filters(np.random.default_rng(81), labels, (), n_threads + 1, k, short=4)[1:]       # eight different, restricting filters
        counters = lambda: tuple(p.g.counter(c) for c in ("hnsw_batch_rounds", "hnsw_batch_coalesced_calls", "batch_rounds", "batch_coalesced_calls"))

        def call(j):
            if j % 2:
                return search_filtered(p, None, Q[j:j + 1], k, ef, [filters[j]])
            return single_call(p, None, Q[j], k, ef, filters[j])
        for mode in MODES:
            p.g.set_option("hnsw_visited_hash", mode)
            p.g.set_option("batch_window_us", 10)
            c0 = counters()
            want = [call(j) for j in range(n_threads)]
            assert counters() == c0, "a lone caller went through the coalescer"
            equal_to_oracle(p, tuple(np.concatenate([w[i] for w in want]) for i in range(3)), Q, k, ef, filters, labels, False, what=("calls made alone", mode))
            p.g.set_option("batch_window_us", 20000)
            got = [None] * n_threads

            def worker(j):
                got[j] = call(j)
            F._run_threads(n_threads, worker)
            for j in range(n_threads):
                assert V.same_results(got[j], want[j]), (mode, j)
            c1 = counters()
            calls, rounds = c1[1] - c0[1], c1[0] - c0[0]
            assert calls >= 2, "the concurrent 1-query calls bypassed the coalescer (%d coalesced calls)" % calls
            assert rounds < calls, "no two calls shared a round (%d rounds for %d calls)" % (rounds, calls)
            assert c1[2:] == c0[2:], "HNSW rounds leaked into the k-NN / keyword counters"
            call(0), call(1)
            assert counters()[:2] == c1[:2], "a lone caller went through the coalescer"
        p.g.set_option("hnsw_visited_hash", 1)
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 8. arguments
def body_arguments(lib):
    p, Q = V.tie_pair(lib, "tri", 8)
    g, L = p.g, p.g.L
    k, ef, n = 10, 64, 3
    q = np.ascontiguousarray(Q[:n])
    dist = np.zeros((n, k), np.float32); lab = np.zeros((n, k), np.uint64); cnt = np.zeros(n, np.uint32)
    raw = lambda n_q, kk, ee, arr: L.tsgpu_vec_hnsw_search_batch_filtered(g.h, 1, _vp(q), B.MEM_HOST, n_q, kk, ee, 1, arr, _vp(dist), _vp(lab), _vp(cnt), B.MEM_HOST)
    ids = np.arange(5, dtype=np.uint32)
    for bad in ((1, 3, None, 0, None), (0, 0, None, 2, None), (1, 5, ids.ctypes.data, 2, None)):       # a filter that counts ids with a NULL list
        arr = (B.VecFilterC * n)()
        arr[1].filtered, arr[1].n_allow, arr[1].allow_ids, arr[1].n_excluded, arr[1].excluded_ids = bad
        assert raw(n, k, ef, arr) == B.ERR_INVALID, bad
    for kk, ee in ((10, 1025), (1025, 10)):
        assert raw(n, kk, ee, None) == B.ERR_UNSUPPORTED, (kk, ee)
    assert raw(0, k, ef, None) == B.TSGPU_OK
    for mode in MODES:
        plain = p.search(mode, Q[:n], k, ef)
        assert V.same_results(search_filtered(p, mode, Q[:n], k, ef, None), plain), mode
        assert V.same_results(search_filtered(p, mode, Q[:n], k, ef, [None] * n), plain), mode
