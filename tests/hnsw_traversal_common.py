"""Shared bodies of tests/test_emu_hnsw_traversal.py (CPU tier, SIMT emulator) and tests/test_gpu_hnsw_traversal.py (-m gpu, libtsgpu.so): the HNSW
traversal (vec_hnsw_search_kernel in csrc/vec_kernels.hip.h, its launcher hnsw_search_launch in csrc/tsgpu_vec.hip) held to its claim -- the labels, the
order and the distance bits of searchKnnCloserFirst as oracle/hnsw_graph.h restates it (a real std::priority_queue, a plain visited array) -- on inputs
the Gaussian rows of the other HNSW tests never produce.

The comparison is always theirs: cnt[i] == d.size, labels equal in order, dist.view(uint32) equal; no tolerance. Unless a case says otherwise every
body runs with option hnsw_visited_hash 0 (16-bit tags) and 1 (hash sets), the two modes against each other and each against the oracle.

Inputs. Rows and queries are small integers cast to fp32: every inner product is exact whatever the summation order, and equal distances are
everywhere. A tie body asserts its premise from the oracle alone: the top k of EVERY query holds a repeated distance. Graphs come from the oracle's
builder (hnsw_build -> hnsw_export -> vec_hnsw_load) or are made by hand in numpy (ring_lattice) and loaded into both sides (vec_hnsw_load,
hnsw_import): the traversal must replay any valid mirror.

  1  ties in both heaps (HnswHeap::push / pop restate libstdc++'s push_heap / pop_heap "so that ties fall the same way"): rows in {-1,0,1}, and rows
     in {-2..2} whose second half duplicates the first; M 8 and 4; inner product and cosine; the non-strict stop rule; an allow list.
  2  every LDS tier on its edges: max(ef, k) = 128, 129, 256, 257, 512, 513, 1024, reached through ef and through k; TOPCAP = need + 1 is exactly the
     slack the `top.n > ef` pop needs. hnsw_tier_reruns must not move (each tier's own instantiation served the batch); 1025 is unsupported (501).
  3  hand-made graphs: full-width lists (2M = 62 ids, dim 20: the 16-lane-group distance path), a query too long for LDS (dim 1040), zero-count
     lists and an unreachable component (cnt < k), a rejected entry point, a visited set past half full (re-run on the largest tier), boosted sets
     (8x), a candidate heap beyond the largest tier (n_out = 0xFFFFFFFF, the documented status).
  4  more queries than query slots (option hnsw_test_slots: a block serves several queries; the hash set is cleared, the tag epoch advances) and the
     clear of the tags at epoch 0xFFF0 (option hnsw_test_epoch)."""
import numpy as np
import pytest

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O

N_TIE, DIM_TIE = 1500, 16
OVERFLOWED = 0xFFFFFFFF


def tie_rows(family, n=N_TIE, dim=DIM_TIE, n_q=8):
    """-> (X, Q): 'tri' = entries in {-1,0,1}; 'dup' = entries in {-2..2}, rows n/2.. repeat rows 0..n/2 (every distance occurs at least twice)"""
    rng = np.random.default_rng({"tri": 11, "dup": 12}[family])
    if family == "tri":
        X = rng.integers(-1, 2, size=(n, dim))
        Q = rng.integers(-1, 2, size=(n_q, dim))
    else:
        half = rng.integers(-2, 3, size=(n // 2, dim))
        X = np.concatenate([half, half])
        Q = rng.integers(-2, 3, size=(n_q, dim))
    assert (X != 0).any(axis=1).all() and (Q != 0).any(axis=1).all()       # (cosine: no zero vector to normalise)
    return X.astype(np.float32), Q.astype(np.float32)


def same_results(a, b):
    """two (dist, labels, counts) results of one batch agree: the counts, and the labels and distance bits of the entries a count covers (the
    library leaves the rest of a row as it finds it)"""
    (da, la, ca), (db, lb, cb) = a, b
    live = np.arange(la.shape[1])[None, :] < np.where(ca == OVERFLOWED, 0, ca)[:, None]
    return bool(np.array_equal(ca, cb) and ((la == lb) | ~live).all() and ((da.view(np.uint32) == db.view(np.uint32)) | ~live).all())


class Pair:
    """the same rows (label = row) and the same graph in a GpuIndex vector field and in the oracle; the oracle's answers are computed once per case"""

    def __init__(self, lib, X, metric=B.METRIC_IP):
        self.n = X.shape[0]
        self.g = T.GpuIndex(0, lib)
        self.g.vec_create(1, X.shape[1], metric)
        self.g.vec_upsert(1, np.arange(self.n, dtype=np.uint64), X)
        self.orc = O.OracleIndex(1, 1)
        self.orc.vec_init(X.shape[1], metric)
        self.orc.vec_add(np.arange(self.n, dtype=np.uint32), X)
        self._ref = {}

    def build(self, M, ef_construction=40):
        self.orc.hnsw_build(M=M, ef_construction=ef_construction, seed=100)
        self.g.vec_hnsw_load(1, self.orc.hnsw_export())
        return self

    def load(self, graph):
        self.g.vec_hnsw_load(1, graph)
        self.orc.hnsw_import(graph)
        return self

    def delete(self, label):
        self.g.vec_delete(1, label)
        assert self.orc.hnsw_mark_deleted(label) == 0
        self._ref = {}

    def ref(self, Q, i, k, ef, allow, functor):
        key = (Q[i].tobytes(), k, ef, None if allow is None else allow.tobytes(), functor)
        if key not in self._ref:
            d, l, _ = self.orc.hnsw_search(Q[i], k, ef, allow_ids=allow, functor_present=functor)
            self._ref[key] = (d, l)
        return self._ref[key]

    def reruns(self):
        return self.g.counter("hnsw_tier_reruns")

    def search(self, mode, Q, k, ef, allow=None, functor=True):
        self.g.set_option("hnsw_visited_hash", mode)
        try:
            return self.g.vec_hnsw_search_batch(1, Q, k, ef, allow_ids=allow, functor_present=functor)
        finally:
            self.g.set_option("hnsw_visited_hash", 1)

    def equal_to_oracle(self, res, Q, k, ef, allow=None, functor=True, what="", only=None):
        dist, lab, cnt = res
        for i in (range(Q.shape[0]) if only is None else only):
            d, l = self.ref(Q, i, k, ef, allow, functor)
            assert cnt[i] == d.size, (what, i, int(cnt[i]), d.size)
            assert np.array_equal(lab[i, :d.size], l), (what, i, lab[i, :d.size][:12], l[:12])
            assert np.array_equal(dist[i, :d.size].view(np.uint32), d.view(np.uint32)), (what, i)

    def check(self, Q, k, ef, allow=None, functor=True, modes=(0, 1), ties=False, what=""):
        """one batch per visited mode: the modes equal each other, each equals the oracle query by query; -> the last mode's result"""
        what = (what, k, ef)
        res = [self.search(m, Q, k, ef, allow, functor) for m in modes]
        for r in res[1:]:
            assert same_results(res[0], r), ("tags vs hash sets", what)
        for m, r in zip(modes, res):
            self.equal_to_oracle(r, Q, k, ef, allow, functor, what + ("hash" if m else "tags",))
        if ties:
            for i in range(Q.shape[0]):
                d, _ = self.ref(Q, i, k, ef, allow, functor)
                assert d.size - np.unique(d).size > 0, ("premise: no repeated distance in the oracle's top k", what, i)
        return res[-1]

    def close(self):
        self.g.close()
        self.orc.close()


_TIE_PAIRS = {}


def tie_pair(lib, family, M, metric=B.METRIC_IP):
    """the tie rows on the oracle-built graph, shared by the read-only bodies (never mutated: no deletions, options restored)"""
    key = (lib, family, M, metric)
    if key not in _TIE_PAIRS:
        X, Q = tie_rows(family)
        _TIE_PAIRS[key] = (Pair(lib, X, metric).build(M), Q)
    return _TIE_PAIRS[key]


# ---------------------------------------------------------------------------------------------------------------- 1. ties in both heaps
TIE_K_EF = ((10, 10), (10, 64), (100, 128), (129, 129), (100, 300))


def body_ties(lib, family, M, k, ef):
    p, Q = tie_pair(lib, family, M)
    p.check(Q, k, ef, ties=True, what="ties %s M %d" % (family, M))


def body_ties_cosine(lib, k, ef):
    """normalised integer rows are no longer exact, but a duplicated row has its twin's bits: the ties are the duplicates'"""
    p, Q = tie_pair(lib, "dup", 8, B.METRIC_COSINE)
    p.check(Q, k, ef, ties=True, what="ties cosine")


def body_ties_non_strict_stop(lib, k, ef):
    """functor_present = False on an index without deletions: hnswlib's non-strict stop rule (`top.size() == ef ||` dropped)"""
    p, Q = tie_pair(lib, "tri", 8)
    p.check(Q, k, ef, functor=False, ties=True, what="ties non-strict")


def body_ties_allow_list(lib, k, ef):
    p, Q = tie_pair(lib, "tri", 8)
    allow = np.sort(np.random.default_rng(13).choice(p.n, size=p.n // 3, replace=False)).astype(np.uint32)
    p.check(Q, k, ef, allow=allow, ties=True, what="ties allow list")


# ---------------------------------------------------------------------------------------------------------------- 2. every tier, on its edges
TIER_EDGES = (128, 129, 256, 257, 512, 513, 1024)


def body_tier_edge(lib, need, n_q=8, both_at_need=False):
    """max(ef, k) = need through ef (k = 10) and through k (ef = 10), or k = ef = need: served by that tier's own instantiation (no re-run)"""
    p, Q = tie_pair(lib, "tri", 8)
    r0 = p.reruns()
    for k, ef in (((need, need),) if both_at_need else ((10, need), (need, 10))):
        p.check(Q[:n_q], k, ef, ties=True, what="tier edge")
    assert p.reruns() == r0, "a query left its tier: hnsw_tier_reruns moved by %d" % (p.reruns() - r0)


def body_beyond_the_largest_tier_is_unsupported(lib):
    p, Q = tie_pair(lib, "tri", 8)
    for k, ef in ((10, 1025), (1025, 10)):
        with pytest.raises(B.TsgpuError) as e:
            p.g.vec_hnsw_search_batch(1, Q[:2], k, ef)
        assert e.value.code == B.ERR_UNSUPPORTED, (k, ef, e.value)


# ---------------------------------------------------------------------------------------------------------------- 3. hand-made graphs
N_HUBS = 16


def ring_lattice(n, M, reach, seed, n_main=None, dead=()):
    """A valid mirror nobody built: nodes 0 .. n_main form a ring, node i links to i +- 1..reach (mod n_main) at level 0, shuffled within the list;
    the nodes n_main .. n form a second ring of the same kind that nothing links into; the nodes in `dead` keep their in-links but have count 0.
    Sixteen evenly spaced nodes of the first ring carry level 1 and are chained as a ring; one of them is the entry point, at level 2, with an
    empty top list. -> dict in vec_hnsw_load's / hnsw_import's form, + hubs"""
    n_main = n if n_main is None else n_main
    assert 2 * reach <= 2 * M and 2 <= M <= 31 and n_main >= N_HUBS and 2 * reach < n_main and (n == n_main or 2 * reach < n - n_main)
    rng = np.random.default_rng(seed)
    step = np.concatenate([np.arange(1, reach + 1), -np.arange(1, reach + 1)])
    ids = np.arange(n)[:, None]
    nb = np.where(ids < n_main, (ids + step) % n_main, n_main + (ids - n_main + step) % max(n - n_main, 1))
    nb = rng.permuted(nb, axis=1)
    link0 = np.zeros((n, 1 + 2 * M), np.uint32)
    link0[:, 0] = 2 * reach
    link0[:, 1:1 + 2 * reach] = nb
    for i in dead:
        link0[i] = 0
    hubs = (np.arange(N_HUBS) * n_main) // N_HUBS
    entry = int(hubs[3])
    levels = np.zeros(n, np.uint64)
    levels[hubs] = 1
    levels[entry] = 2
    upper_ptr = np.zeros(n + 1, np.uint64)
    upper_ptr[1:] = np.cumsum(levels)
    upper = np.zeros((int(upper_ptr[n]), 1 + M), np.uint32)
    for j, h in enumerate(hubs):
        upper[int(upper_ptr[h])] = [2, hubs[j - 1], hubs[(j + 1) % N_HUBS]] + [0] * (M - 2)      # level 1; the entry point's level-2 list stays empty
    return dict(M=M, maxlevel=2, enterpoint=entry, link0=link0, upper_ptr=upper_ptr, upper_links=upper, hubs=hubs)


def lattice_pair(lib, n, dim, M, reach, seed, n_q, **kw):
    rng = np.random.default_rng(seed)
    X = rng.integers(-1, 2, size=(n, dim)).astype(np.float32)
    Q = rng.integers(-1, 2, size=(n_q, dim)).astype(np.float32)
    graph = ring_lattice(n, M, reach, seed + 1, **kw)
    return Pair(lib, X).load(graph), Q, graph


def body_full_width_lists(lib):
    """M 31, reach 31: 62 ids per list, the most one wavefront fetches; dim 20 is no multiple of 16 (ip_distance_group16, four rows per round)"""
    p, Q, _ = lattice_pair(lib, 700, 20, 31, 31, 21, 4)
    try:
        p.check(Q, 10, 50, what="full-width lists")
    finally:
        p.close()


def body_query_not_staged_in_lds(lib):
    """dim 1040 > VEC_HNSW_QDIM: the query is read from global memory by every distance"""
    p, Q, _ = lattice_pair(lib, 300, 1040, 4, 3, 22, 2)
    try:
        p.check(Q, 10, 40, what="dim 1040")
    finally:
        p.close()


def body_dead_ends_and_an_unreachable_component(lib):
    """80 reachable nodes, three of them with empty lists, and a ring of 40 that nothing links into: k = 100 returns fewer than k, exactly the oracle's"""
    p, Q, _ = lattice_pair(lib, 120, 20, 4, 3, 23, 4, n_main=80, dead=(7, 8, 41))
    try:
        for functor in (True, False):
            dist, lab, cnt = p.check(Q, 100, 100, functor=functor, what="unreachable component")
            assert (cnt == 80).all() and (lab[:, :80] < 80).all(), cnt
        p.check(Q, 10, 20, what="dead ends")
    finally:
        p.close()


def body_entry_point_rejected(lib):
    """the entry point fails the filter (strict stop rule), then is deleted (functor_present = False: the deletion alone selects the strict rule):
    it seeds the candidates with the largest bound and never reaches the results"""
    p, Q, graph = lattice_pair(lib, 300, 20, 4, 3, 24, 4)
    try:
        entry = graph["enterpoint"]
        allow = np.delete(np.arange(p.n, dtype=np.uint32), entry)
        dist, lab, cnt = p.check(Q, 10, 50, allow=allow, what="entry point filtered out")
        assert (cnt == 10).all() and not (lab == entry).any()
        p.delete(entry)
        dist, lab, cnt = p.check(Q, 10, 50, functor=False, what="entry point deleted")
        assert (cnt == 10).all() and not (lab == entry).any()
    finally:
        p.close()


def _far_side(graph, n, count):
    far = (graph["enterpoint"] + n // 2 + 7 * np.arange(1, count + 1)) % n
    assert not np.isin(far, graph["hubs"]).any()
    return np.sort(far).astype(np.uint32)


def body_visited_set_past_half_full(lib, n=5000, n_q=2, reruns_per_query=1):
    """three allowed ids on a ring of n: the result heap never fills, so the strict rule walks the whole ring. n = 5 000 visits pass half of the
    smallest tier's 8 192-word set but not of the largest tier's 65 536: one re-run, there, no boost. n = 40 000 pass 32 768 as well: a second
    re-run with sets 8x as large. Tags need neither."""
    p, Q, graph = lattice_pair(lib, n, 16, 2, 2, 25, n_q)
    try:
        allow = _far_side(graph, n, 3)
        r0 = p.reruns()
        res = p.search(1, Q, 10, 10, allow)
        assert p.reruns() - r0 == reruns_per_query * n_q, "hash sets: %d re-runs for %d queries" % (p.reruns() - r0, n_q)
        p.equal_to_oracle(res, Q, 10, 10, allow, what="visited set past half full, hash sets")
        assert (res[2] == 3).all() and np.array_equal(np.sort(res[1][:, :3], axis=1), np.tile(allow, (n_q, 1)))
        r0 = p.reruns()
        tags = p.search(0, Q, 10, 10, allow)
        assert p.reruns() == r0, "tags: nothing to outgrow"
        assert same_results(tags, res)
    finally:
        p.close()


def body_candidate_heap_beyond_the_largest_tier(lib):
    """n 6 000, M 31, reach 31, ONE allowed id, so the result heap never fills and every query walks the whole ring. Coordinate 0 of row i is
    half its offset from the entry point going up the ring (-2 on the last 400 nodes, which lie just below the entry point; -3 on the other level-1
    nodes, so that the descent of queries 0 and 1 stays put); the other coordinates are in {-1,0,1} and meet zeros in the queries.
    Queries 0 and 1 = (c, 0, ..), c > 0: the further up the ring the closer, so every expansion is the frontier's and adds ~31 candidates for the one
    it pops: the candidate heap passes 1 024 entries after ~1 060 nodes and 4 096 after ~4 230 (it would peak at 5 475). The documented status:
    n_out = 0xFFFFFFFF, and vec_knn_batch with the same allow list answers. One re-run each (the largest tier); larger visited sets could not
    help them and are not tried.
    Query 2 = (-1, 0, ..): the lower the closer, every expansion is an inner node's, the heap stays below 100 entries; it equals the oracle. (Its
    6 000 visits pass half of the smallest tier's visited set, so in hash mode it runs again once, too: 3 re-runs there, 2 with tags.)"""
    n, dim = 6000, 20
    graph = ring_lattice(n, 31, 31, 27)
    entry, hubs = graph["enterpoint"], graph["hubs"]
    X = np.random.default_rng(26).integers(-1, 2, size=(n, dim)).astype(np.float32)
    off = (np.arange(n) - entry) % n
    X[:, 0] = off // 2
    X[off > n - 400, 0] = -2
    X[hubs[hubs != entry], 0] = -3
    Q = np.zeros((3, dim), np.float32)
    Q[0, 0], Q[1, 0], Q[2, 0] = 1, 2, -1
    allow = _far_side(graph, n, 1)
    p = Pair(lib, X).load(graph)
    try:
        for mode, expect in ((1, 3), (0, 2)):
            r0 = p.reruns()
            dist, lab, cnt = p.search(mode, Q, 10, 10, allow)
            assert cnt[0] == OVERFLOWED and cnt[1] == OVERFLOWED, (mode, cnt)
            p.equal_to_oracle((dist, lab, cnt), Q, 10, 10, allow, what="the ordinary query of the batch", only=(2,))
            assert cnt[2] == 1 and lab[2, 0] == allow[0]
            assert p.reruns() - r0 == expect, "visited mode %d: %d re-runs, expected %d" % (mode, p.reruns() - r0, expect)
        for i in (0, 1):        # the oracle has no heap to outgrow: the answer exists, and the exact scan the header points to returns it
            d, l = p.ref(Q, i, 10, 10, allow, True)
            assert l.tolist() == [int(allow[0])]
        dist, lab, cnt = p.g.vec_knn_batch(1, Q[:2], 10, allow_ids=allow)
        assert (cnt == 1).all() and (lab[:, 0] == allow[0]).all()
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 4. query slots and the tag epoch
def slots_pair(lib):
    X, _ = tie_rows("tri", n=300)
    rng = np.random.default_rng(31)
    Q = rng.integers(-1, 2, size=(3 * 4096, DIM_TIE)).astype(np.float32)
    Q[~(Q != 0).any(axis=1)] = 1
    return Pair(lib, X).build(4), Q


def body_more_queries_than_slots(lib):
    """hnsw_test_slots = 3, 20 queries: every block serves 6 or 7 queries one after the other (hash set cleared and fenced / tag epoch + 1 between
    them). Then with hnsw_test_tiny_cand: the overflowed queries run again through q_sel, several per block."""
    p, Q = slots_pair(lib)
    try:
        p.g.set_option("hnsw_test_slots", 3)
        p.check(Q[:20], 3, 6, what="3 slots")
        p.g.set_option("hnsw_test_tiny_cand", 1)
        res = []
        for mode in (0, 1):
            r0 = p.reruns()
            res.append(p.search(mode, Q[20:40], 10, 60))
            assert p.reruns() - r0 > 3, "premise: no more overflowed queries than slots (%d re-runs)" % (p.reruns() - r0)
            p.equal_to_oracle(res[-1], Q[20:40], 10, 60, what="3 slots, 24-entry candidate heap, visited mode %d" % mode)
        assert same_results(*res)
    finally:
        p.close()


def body_tag_epoch_wrap(lib):
    """tag mode, 3 slots. A first batch leaves tags of epochs 1..7 behind. Then, as if 0xFFEC queries per slot had run (hnsw_test_epoch): the next
    batch's 7 epochs would reach 0xFFF0, so the tags are cleared and the epochs restart at 1 -- a missing or short clear shows as nodes of the
    first batch taken for visited."""
    p, Q = slots_pair(lib)
    try:
        p.g.set_option("hnsw_test_slots", 3)
        p.check(Q[:20], 3, 6, modes=(0,), what="epochs 1..7")
        p.g.set_option("hnsw_test_epoch", 0xFFEC)
        p.check(Q[20:40], 3, 6, modes=(0,), what="across the clear at 0xFFF0")
        p.check(Q[40:60], 3, 6, modes=(0,), what="after the clear")
    finally:
        p.close()


def body_more_queries_than_the_natural_slots(lib, n_q=2 * 4096 + 37):
    """4 096 slots, 8 229 queries: two or three queries per block at the library's own grid, against the oracle's batch API"""
    p, Q = slots_pair(lib)
    try:
        ref = p.orc.hnsw_search_batch(Q[:n_q], 3, 6, threads=16)
        for mode in (0, 1):
            res = p.search(mode, Q[:n_q], 3, 6)
            live = np.arange(3)[None, :] < ref[2][:, None]
            same = (res[2] == ref[2]) & ((res[1] == ref[1]) | ~live).all(axis=1) & ((res[0].view(np.uint32) == ref[0].view(np.uint32)) | ~live).all(axis=1)
            bad = np.nonzero(~same)[0].tolist()
            assert not bad, "visited mode %d: %d / %d queries differ from the oracle, first %s" % (mode, len(bad), n_q, bad[:8])
    finally:
        p.close()
