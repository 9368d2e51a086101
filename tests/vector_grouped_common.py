"""group_by for the pure vector search (tsgpu_vector_search_grouped_batch: the per-query vector front, gb_vec_items_kernel and the vector form of the
grouped core in kw_groupby.hip.h / tsgpu_groupby.inc.h). Shared by tests/test_emu_vector_grouped.py (SIMT emulator) and
tests/test_gpu_vector_grouped.py (MI355X).

Expected values, no tolerance anywhere (distance bits included): the ITEMS of a query and their KVs are what the oracle's search_vector returns for the
same k, threshold, filter ids, excluded ids, flat_search_cutoff and query document with a fetch_size so large that its Topster holds every KV; the
distinct keys are read from the column the product reads; both go through the oracle's restated distinct Topster (group_topster_run; one case also through
the reference's own Topster<KV> where oracle/_ref was built) at the product's capacity rule. Compared: groups in order, per group its keys in order, the
three scores, match_score_index, vector_distance bits, group_size, group_found, n_groups, groups_total, groups_count, num_matched and the id list."""
import numpy as np

from typesense_amd import _lib as B
from oracle import oracle_py as O
import typesense_amd as T
from tests import helpers as H
from tests import vector_search_pq_common as V
from tests.test_emu_groupby import check_query, group_column

POINTS_COL, GROUP_COL, SHORT_COL, ONE_COL = 0, 1, 2, 3
SHORT_LEN = 150
DEFAULT_SORT = V.DEFAULT_SORT
ASC_SORT = ((B.SORT_VECTOR_DISTANCE, 1, 0), (B.SORT_SEQ_ID, 1, 0))
COL_THEN_VD = ((B.SORT_INT64_COLUMN, 1, POINTS_COL), (B.SORT_VECTOR_DISTANCE, -1, 0), (B.SORT_SEQ_ID, -1, 0))
COUNTERS = ("vec_grouped_flat_queries", "vec_grouped_kcut_queries", "vec_grouped_items", "vec_grouped_syncs", "vec_search_pq_flat_launches", "vec_search_pq_flat_lists")


class World(V.Corpus):
    """V.Corpus (ties, documents without a vector, deleted rows, an int64 column) + the distinct-key columns"""
    def __init__(self, lib, dim, metric, n_docs=400, seed=5, n_values=37, deleted=(7, 100, 222)):
        super().__init__(lib, dim, metric, n_docs=n_docs, seed=seed, deleted=deleted)
        distinct, _ = group_column(n_docs, seed=seed + 1, n_values=n_values)
        self.columns = {GROUP_COL: distinct, SHORT_COL: distinct[:SHORT_LEN].copy(), ONE_COL: np.full(n_docs, 77, np.uint64)}
        for col, v in self.columns.items():
            self.g.column_set(col, v.view(np.int64))

    def counters(self):
        return {n: self.g.counter(n) for n in COUNTERS}


def run(c, Q, P, G, k_stride=750, g_stride=250, want_registers=False):
    return c.g.vector_search_grouped_batch(1, Q, P, G, k_stride=k_stride, g_stride=g_stride, want_ids=True, want_registers=want_registers)


def capacity_of(c, p):
    f = p.get("filter_ids")
    bound = f.size if f is not None and f.size else c.n_docs
    return p.get("topster_size", 0) or max(1, min(max(p.get("fetch_size", 10), 250), bound))


def expected(c, q, p, grp, through_reference=False):
    """the oracle's answer for ONE query: a GroupedHits with .vd_bits / .msi per key and .ids"""
    gl, col, first, gmv = grp[:4]
    p = dict(p)
    cap = capacity_of(c, p)
    flat = V.is_flat(p)
    sort = p.pop("sort", DEFAULT_SORT)
    k = p.pop("k", 0) or p.get("fetch_size", 10)
    p.pop("fetch_size", None)
    p.pop("topster_size", None)
    room = max(4096, c.n_docs)                                                  # a Topster (and result arrays) that hold every candidate
    ref = c.orc.search_vector(q, k=k, fetch_size=room, sort=tuple((s[0], s[2], s[1]) for s in sort), cap=room, ids_cap=c.n_docs, **p)
    # the reference's order: list order for a flat query, nearest first for a k-cut query
    order = np.argsort(ref.keys, kind="stable") if flat else np.lexsort((ref.keys, ref.vector_distance))
    keys, scores = ref.keys[order], ref.scores[order]
    colv = c.columns[col]
    dk = np.array([int(colv[i]) if i < colv.size else (1 if gmv else int(i)) for i in keys], np.uint64)
    ret, g = O.group_topster_run(cap, gl, first, keys, dk, scores)
    if through_reference:
        R = O.ref_topster_lib()
        if R is not None:
            rret, gsize, rdk, rkeys, rsc, rcount = O.ref_group_topster_run(R, cap, gl, first, keys, dk, scores)
            assert np.array_equal(ret, rret) and np.array_equal(g.group_size, gsize) and np.array_equal(g.distinct_key, rdk)
            assert np.array_equal(g.keys, rkeys) and np.array_equal(g.scores, rsc) and (not first or g.groups_count == rcount)
    g.num_keyword_matches = int(keys.size)
    g.vd_bits = dict(zip(ref.keys.tolist(), ref.vector_distance.view(np.uint32).tolist()))
    g.msi = dict(zip(ref.keys.tolist(), ref.match_score_index.tolist()))
    g.ids = np.sort(ref.keys).astype(np.uint32)
    assert int(ref.n_result_ids) == keys.size
    return g


def check(c, Q, P, G, res, which=None, what="", through_reference=()):
    h, gh, ids = res
    for i in (range(len(P)) if which is None else which):
        gl, col, first, gmv = G[i][:4]
        ref = expected(c, Q[i], P[i], G[i], through_reference=i in through_reference)
        w = (what, i, "flat" if V.is_flat(P[i]) else "k-cut", "first" if first else "second")
        check_query(h, gh, i, ref, bool(first), gl, what=str(w))
        ng = int(gh.n_groups[i])
        slots = list(range(ng)) if first else [r * gl + j for r in range(ng) for j in range(int(gh.group_size[i, r]))]
        for s in slots:
            key = int(h.keys[i, s])
            assert int(h.vector_distance[i, s:s + 1].view(np.uint32)[0]) == ref.vd_bits[key], (w, "vector_distance of", key)
            assert int(h.match_score_index[i, s]) == ref.msi[key], (w, "match_score_index of", key)
        assert np.array_equal(ids[i], ref.ids), (w, ids[i][:8], ref.ids[:8])
    return res


def assert_same(a, i, b, j, G, what=""):
    """query i of result a == query j of result b, every array the call returns"""
    (ha, ga, ia), (hb, gb, ib) = a, b
    gl, first = G[0], G[2]
    assert int(ha.status[i]) == int(hb.status[j]), (what, i, ha.status[i], hb.status[j])
    ng = int(gb.n_groups[j])
    assert int(ga.n_groups[i]) == ng and int(ha.n_hits[i]) == int(hb.n_hits[j]) and int(ha.num_matched[i]) == int(hb.num_matched[j]), (what, i)
    for name in ("distinct_key", "group_size", "group_found"):
        assert np.array_equal(getattr(ga, name)[i, :ng], getattr(gb, name)[j, :ng]), (what, i, name)
    assert int(ga.groups_total[i]) == int(gb.groups_total[j]) and int(ga.groups_count[i]) == int(gb.groups_count[j]), (what, i)
    slots = list(range(ng)) if first else [r * gl + k for r in range(ng) for k in range(int(gb.group_size[j, r]))]
    for name in ("keys", "scores", "match_score_index", "text_match"):
        assert np.array_equal(getattr(ha, name)[i][slots], getattr(hb, name)[j][slots]), (what, i, name)
    assert np.array_equal(ha.vector_distance[i][slots].view(np.uint32), hb.vector_distance[j][slots].view(np.uint32)), (what, i)
    assert np.array_equal(ia[i], ib[j]), (what, i)


def mixed_batch(c):
    """flat and k-cut queries interleaved, each with its own list, k, threshold, group_limit (1 and 3), column and pass"""
    thr = 1.02 if c.metric == B.METRIC_COSINE else 0.5
    P, G = [], []

    def add(grp, **kw):
        P.append(kw)
        G.append(grp)
    m = c.pick(90, among=c.live)
    add((3, GROUP_COL, 1, 0), fetch_size=10, filter_ids=c.pick(120), flat_search_cutoff=1000)
    add((1, GROUP_COL, 0, 0), fetch_size=40)
    add((3, GROUP_COL, 0, 0), fetch_size=10, filter_ids=c.pick(257), flat_search_cutoff=1000, distance_threshold=thr + 0.3)
    add((3, SHORT_COL, 1, 1), k=60, fetch_size=10, filter_ids=c.pick(200), excluded_ids=c.pick(25))
    add((1, SHORT_COL, 0, 0), fetch_size=30, filter_ids=c.pick(150), flat_search_cutoff=1000, distance_threshold=thr)
    add((3, GROUP_COL, 0, 0), fetch_size=30, distance_threshold=thr, filter_ids=c.pick(150))
    add((1, GROUP_COL, 1, 0), fetch_size=10, filter_ids=m, flat_search_cutoff=1000, query_doc=int(m[40]))
    add((3, GROUP_COL, 1, 0), fetch_size=10, filter_ids=m.copy(), query_doc=int(m[41]))
    add((3, GROUP_COL, 0, 0), fetch_size=25, sort=V.THREE_KEYS, filter_ids=c.pick(200), flat_search_cutoff=1000)
    add((3, SHORT_COL, 0, 1), fetch_size=25, sort=V.THREE_KEYS, filter_ids=c.pick(200), excluded_ids=c.pick(30))
    add((3, GROUP_COL, 1, 0), fetch_size=10, filter_ids=np.arange(c.n_vec + 3, c.n_vec + 30, dtype=np.uint32), flat_search_cutoff=1000)      # only ids without a vector
    add((1, ONE_COL, 0, 0), k=100, fetch_size=10, query_doc=int(c.ties[3]))
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    Q[1] = c.X[5]
    for i, p in enumerate(P):
        if "query_doc" in p:
            Q[i] = c.X[p["query_doc"]]
    return P, G, Q


def case_mixed_batch(lib, dim, metric):
    """case 1"""
    c = World(lib, dim, metric)
    P, G, Q = mixed_batch(c)
    before = c.counters()
    res = run(c, Q, P, G)
    after = c.counters()
    n_flat = sum(V.is_flat(p) for p in P)
    assert (res[0].status == 0).all(), res[0].status
    assert after["vec_grouped_flat_queries"] - before["vec_grouped_flat_queries"] == n_flat
    assert after["vec_grouped_kcut_queries"] - before["vec_grouped_kcut_queries"] == len(P) - n_flat
    assert after["vec_grouped_items"] - before["vec_grouped_items"] == int(res[0].num_matched.sum())
    assert after["vec_grouped_syncs"] - before["vec_grouped_syncs"] == 1 and after["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == 1
    assert int(res[1].n_groups[10]) == 0 and int(res[0].num_matched[10]) == 0 and res[2][10].size == 0
    check(c, Q, P, G, res, what=("mixed", dim, metric), through_reference=(0, 3, 4, 5))
    for i in range(len(P)):                                         # every query equals the same call issued for it alone
        one = run(c, Q[i:i + 1], [P[i]], [G[i]])
        assert_same(res, i, one, 0, G[i], what="alone")
    c.close()


def case_compaction_edges(lib):
    """case 2: the flat compaction at the tile boundaries (GB_THREADS = 256 ids per tile), by every cause of dropping"""
    deleted = (7, 300, 600)                                                     # deleted rows: ids without a vector in the middle of a list
    c = World(lib, 24, B.METRIC_COSINE, n_docs=700, deleted=deleted)
    novec = np.arange(c.n_vec, c.n_docs, dtype=np.uint32)                       # 40 ids without a vector
    live = c.live

    def listing(n):
        return np.sort(c.rng.choice(live, size=n, replace=False)).astype(np.uint32)
    P, G, what = [], [], []

    def add(grp, note, **kw):
        P.append(dict(fetch_size=10, flat_search_cutoff=5000, **kw))
        G.append(grp)
        what.append(note)
    for n in (1, 255, 256, 257, 513):
        add((3, GROUP_COL, n % 2, 0), ("length", n), filter_ids=listing(n))
    # ids without a vector: first of a tile (position 0 and 256), last of a tile (255), the list's tail
    base = live                                                                 # (the deleted rows are not among them)
    first_of_tile0 = np.concatenate([[7], base[base > 7][:299]]).astype(np.uint32)                       # position 0 has no vector
    add((3, GROUP_COL, 0, 0), "no vector at 0", filter_ids=first_of_tile0)
    l255 = np.concatenate([base[base < 300][-255:], [300], base[base > 300][:40]]).astype(np.uint32)    # position 255: the last id of tile 0
    assert l255[255] == 300 and first_of_tile0[0] == 7
    add((3, GROUP_COL, 1, 0), "no vector at 255", filter_ids=l255)
    l256 = np.concatenate([base[:256], novec[:1]]).astype(np.uint32)                                    # position 256: the first id of tile 1 (and the last of the list)
    add((1, GROUP_COL, 0, 0), "no vector at 256", filter_ids=l256)
    whole_tile = np.concatenate([base[-256:], novec]).astype(np.uint32)                                 # (tile 0 live, the tail of 40 dropped)
    add((3, GROUP_COL, 0, 0), "tail dropped", filter_ids=whole_tile)
    add((3, GROUP_COL, 1, 0), "whole list dropped: no vector", filter_ids=novec.copy())
    # the threshold: drops by value — a whole tile (every id beyond it), a whole list
    far = listing(300)
    add((3, GROUP_COL, 0, 0), "threshold cuts", filter_ids=far, distance_threshold=0.9)
    add((3, GROUP_COL, 1, 0), "threshold drops the whole list", filter_ids=listing(300), distance_threshold=-1.0)
    # a tile dropped whole: the first 256 ids are the tie rows' complement under a threshold only the ties meet
    ties = c.ties[np.isin(c.ties, live)]
    others = np.setdiff1d(live, ties)
    t_low = others[others < ties[-20]][:256]
    tile_gone = np.sort(np.concatenate([t_low, ties[ties > t_low[-1]][:30]])).astype(np.uint32)
    add((3, GROUP_COL, 0, 0), "first tile dropped by the threshold", filter_ids=tile_gone, distance_threshold=1e-3)
    # the query document at list positions 0, 255, 256 and last; one that is not in the list; two queries sharing one list with different documents
    A = listing(400)
    absent = int(np.setdiff1d(live, A)[9])
    for pos in (0, 255, 256, 399):
        add((3, GROUP_COL, pos % 2, 0), ("query_doc at", pos), filter_ids=A, query_doc=int(A[pos]))
    add((3, GROUP_COL, 0, 0), "query_doc absent", filter_ids=A, query_doc=absent)
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    for i, p in enumerate(P):
        if "query_doc" in p:
            Q[i] = c.X[p["query_doc"]]
    Q[len(P) - 6] = c.X[5]                                                       # "first tile dropped": the query IS the shared embedding, cosine distance ~0 to the ties only
    before = c.counters()
    res = run(c, Q, P, G, k_stride=3 * 250)
    after = c.counters()
    assert (res[0].status == 0).all(), res[0].status
    assert after["vec_search_pq_flat_lists"] - before["vec_search_pq_flat_lists"] == len(P) - 4, "A was not recognised as one list"
    for i, note in enumerate(what):
        if isinstance(note, str) and "whole list" in note:
            assert int(res[1].n_groups[i]) == 0 and int(res[0].num_matched[i]) == 0 and res[2][i].size == 0 and int(res[0].n_hits[i]) == 0, note
        if note == "first tile dropped by the threshold":
            assert 0 < int(res[0].num_matched[i]) <= 30 and int(res[2][i][0]) > int(t_low[-1]), (note, res[0].num_matched[i])
        if isinstance(note, tuple) and note[0] == "query_doc at":
            assert P[i]["query_doc"] not in res[2][i].tolist()
    check(c, Q, P, G, res, what="compaction")
    c.close()


def case_group_edges(lib):
    """case 3"""
    c = World(lib, 48, B.METRIC_IP)
    P, G = [], []

    def add(grp, **kw):
        P.append(kw)
        G.append(grp)
    big = np.arange(SHORT_LEN, c.n_docs, dtype=np.uint32)                       # every id beyond the short column
    for flat in (True, False):
        br = dict(flat_search_cutoff=5000) if flat else dict(k=120)
        add((3, SHORT_COL, 0, 0), fetch_size=10, filter_ids=big, **br)          # every item its own group (seq_id)
        add((3, SHORT_COL, 0, 1), fetch_size=10, filter_ids=big.copy(), **br)   # ... all missing ids in group 1
        add((3, SHORT_COL, 1, 1), fetch_size=10, filter_ids=big.copy(), **br)
        add((2, ONE_COL, 0, 0), fetch_size=10, filter_ids=c.pick(180), **br)    # one group for everything, group_limit below its size
        add((3, GROUP_COL, 0, 0), fetch_size=10, filter_ids=c.pick(30), **br)   # fewer groups than the capacity
        add((3, GROUP_COL, 0, 0), fetch_size=10, topster_size=5, filter_ids=c.pick(200), **br)      # more groups than the capacity
        add((3, GROUP_COL, 1, 0), fetch_size=10, topster_size=5, filter_ids=c.pick(200), **br)
        add((3, GROUP_COL, 0, 0), fetch_size=10, filter_ids=np.union1d(c.ties, c.pick(60)).astype(np.uint32), **br)     # duplicate vectors: equal distances inside and across groups
        add((1, GROUP_COL, 1, 0), fetch_size=10, filter_ids=np.union1d(c.ties, c.pick(60)).astype(np.uint32), **br)
        add((3, GROUP_COL, 0, 0), fetch_size=10, sort=COL_THEN_VD, filter_ids=c.pick(220), **br)    # _vector_distance in second place, behind an int64 column
        add((3, GROUP_COL, 0, 0), fetch_size=10, sort=ASC_SORT, filter_ids=c.pick(220), **br)       # ascending _vector_distance
        add((3, GROUP_COL, 1, 0), fetch_size=10, sort=ASC_SORT, filter_ids=c.pick(220), **br)
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    Q[7] = Q[8] = Q[19] = Q[20] = c.X[5]                                        # the ties are the nearest
    res = run(c, Q, P, G, k_stride=750)
    assert (res[0].status == 0).all(), res[0].status
    assert int(res[1].n_groups[0]) == int(res[0].num_matched[0]) > 100 and int(res[1].n_groups[1]) == 1
    assert int(res[1].n_groups[3]) == 1 and int(res[1].group_size[3, 0]) == 2 and int(res[1].group_found[3, 0]) > 2
    assert int(res[1].n_groups[5]) == 5 and int(res[1].groups_total[5]) > 5
    check(c, Q, P, G, res, what="group edges", through_reference=(5, 6))
    c.close()


def case_kcut(lib):
    """case 4: different k in one batch (prefixes of the largest), a filter list and excluded ids, query_doc passing the functor or not, a threshold that cuts"""
    c = World(lib, 24, B.METRIC_COSINE)
    allow = np.union1d(c.ties[::2], c.pick(150)).astype(np.uint32)
    P, G = [], []
    for j, k in enumerate((1, 2, 7, 31, 64, 100, 199, 200)):
        P.append(dict(k=k, fetch_size=10)); G.append((3, GROUP_COL, j % 2, 0))
        P.append(dict(k=k, fetch_size=10, query_doc=int(c.ties[4 + j]))); G.append((1, GROUP_COL, (j + 1) % 2, 0))
        P.append(dict(k=k, fetch_size=10, filter_ids=allow, excluded_ids=allow[::9].copy(), query_doc=int(allow[5 * j + 2]))); G.append((3, SHORT_COL, j % 2, 1))
        P.append(dict(k=k, fetch_size=10, filter_ids=allow, excluded_ids=allow[5 * j + 3:5 * j + 4].copy(), query_doc=int(allow[5 * j + 3]))); G.append((3, GROUP_COL, 0, 0))   # excluded: k stays
        P.append(dict(k=k, fetch_size=10, filter_ids=allow, distance_threshold=0.6)); G.append((3, GROUP_COL, 0, 0))
    Q = np.repeat(c.X[5][None, :], len(P), axis=0).copy()
    Q[4::5] = c.rng.standard_normal((len(Q[4::5]), c.dim)).astype(np.float32)   # the threshold queries: random directions, cosine distances around 1
    before = c.counters()
    res = run(c, Q, P, G, k_stride=750)
    after = c.counters()
    assert (res[0].status == 0).all(), res[0].status
    assert after["vec_grouped_kcut_queries"] - before["vec_grouped_kcut_queries"] == len(P) and after["vec_grouped_syncs"] == before["vec_grouped_syncs"]
    assert len(set(int(n) for n in res[0].num_matched)) > 5
    cut = [i for i in range(4, len(P), 5) if int(res[0].num_matched[i]) < P[i]["k"]]
    assert cut, "the threshold cut nothing"
    check(c, Q, P, G, res, what="k-cut")
    c.close()


def case_delivery(lib, big=False):
    """case 5: vector_distance at every delivery site — a first pass (gb_select_kernel), a second pass with small groups (gb_members_kernel), the same with output
    arrays beyond the packed delivery's 4 MiB (the direct copies) and, on the GPU, one group of 9 000 members (gb_chunk_kernel)"""
    c = World(lib, 48, B.METRIC_IP)
    P = [dict(fetch_size=10, filter_ids=c.pick(300), flat_search_cutoff=5000), dict(k=150, fetch_size=10, filter_ids=c.pick(300))]
    Q = c.rng.standard_normal((2, c.dim)).astype(np.float32)
    for first in (1, 0):
        G = [(3, GROUP_COL, first, 0)] * 2
        check(c, Q, P, G, run(c, Q, P, G, k_stride=750), what=("delivery", first))
    G = [(3, GROUP_COL, 0, 0)] * 2
    small = run(c, Q, P, G, k_stride=750)
    direct = check(c, Q, P, G, run(c, Q, P, G, k_stride=60000), what="direct delivery")      # 2 x 60 000 slots x 37 bytes > 4 MiB
    for i in range(2):
        assert_same(direct, i, small, i, G[i], what="direct vs packed")
    c.close()
    if big:
        n = 9200
        rng = np.random.default_rng(8)
        w = World.__new__(World)
        w.orc, w.g = H.build_pair(H.zipf_docs(n, 30, 4, seed=9), lib)
        w.rng, w.n_docs, w.dim, w.metric, w.n_vec = rng, n, 8, B.METRIC_IP, n
        X = rng.standard_normal((n, 8)).astype(np.float32)
        w.g.vec_create(1, 8, B.METRIC_IP)
        w.g.vec_upsert(1, np.arange(n, dtype=np.uint64), X)
        w.orc.vec_init(8, B.METRIC_IP)
        w.orc.vec_add(np.arange(n, dtype=np.uint32), X)
        w.columns = {ONE_COL: np.full(n, 77, np.uint64)}
        w.g.column_set(ONE_COL, w.columns[ONE_COL].view(np.int64))
        ids = np.sort(rng.choice(n, size=9000, replace=False)).astype(np.uint32)
        P = [dict(fetch_size=10, filter_ids=ids, flat_search_cutoff=100000)]
        G = [(3, ONE_COL, 0, 0)]
        Qb = rng.standard_normal((1, 8)).astype(np.float32)
        res = run(w, Qb, P, G, k_stride=750)
        assert int(res[1].n_groups[0]) == 1 and int(res[1].group_found[0, 0]) == 9000 and int(res[1].group_size[0, 0]) == 3
        check(w, Qb, P, G, res, what="one group of 9 000")
        w.close()


def case_refusals(lib):
    """case 6: refusals are per query; the neighbours' answers do not change"""
    c = World(lib, 24, B.METRIC_IP)
    good_flat = lambda: dict(fetch_size=10, filter_ids=c.pick(70), flat_search_cutoff=1000)
    good_kcut = lambda: dict(fetch_size=10, filter_ids=c.pick(110), excluded_ids=c.pick(9))
    ok = (3, GROUP_COL, 0, 0)
    bad = {1: (good_flat(), (0, GROUP_COL, 0, 0), B.ERR_INVALID),                                   # group_limit 0
           2: (good_kcut(), (257, GROUP_COL, 1, 0), B.ERR_INVALID),                                 # group_limit beyond TSGPU_MAX_GROUP_LIMIT
           4: (dict(fetch_size=10, sort=((B.SORT_EVAL, 1, 0), (B.SORT_SEQ_ID, 1, 0))), ok, B.ERR_UNSUPPORTED),
           5: (dict(k=1025, fetch_size=10), ok, B.ERR_UNSUPPORTED),
           7: (dict(fetch_size=10, topster_size=2000, filter_ids=c.pick(300), flat_search_cutoff=1000), ok, B.ERR_UNSUPPORTED),     # capacity beyond TSGPU_MAX_TOPK
           8: (dict(k=0, fetch_size=0), ok, B.ERR_INVALID)}
    P = [bad[i][0] if i in bad else (good_flat() if i % 2 == 0 else good_kcut()) for i in range(10)]
    G = [bad[i][1] if i in bad else ok for i in range(10)]
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    res = run(c, Q, P, G, k_stride=750)
    h, gh, ids = res
    good = [i for i in range(len(P)) if i not in bad]
    assert h.status.tolist() == [bad[i][2] if i in bad else 0 for i in range(len(P))], h.status
    for i in bad:
        assert int(h.n_hits[i]) == 0 and int(gh.n_groups[i]) == 0 and int(h.num_matched[i]) == 0 and ids[i].size == 0, i
    check(c, Q, P, G, res, which=good, what="refusals")
    alone = run(c, Q[good], [P[i] for i in good], [G[i] for i in good], k_stride=750)
    for j, i in enumerate(good):
        assert_same(res, i, alone, j, G[i], what="neighbours")
    # strides: B = min(capacity, item bound); g_stride must hold B groups, k_stride B hits (first pass) or B * group_limit (second pass)
    P2 = [dict(fetch_size=10, filter_ids=c.pick(70), flat_search_cutoff=1000), dict(k=40, fetch_size=10), dict(fetch_size=10, filter_ids=c.pick(300), flat_search_cutoff=1000),
          dict(k=40, fetch_size=10), dict(k=81, fetch_size=10)]
    G2 = [(3, GROUP_COL, 0, 0), (3, GROUP_COL, 1, 0), (1, GROUP_COL, 1, 0), (3, GROUP_COL, 0, 0), (1, GROUP_COL, 1, 0)]
    # B = 70, 40, 250, 40, 81 — k_stride 210 holds 70 x 3 and 40 (first pass), not 250 and not 40 x 3 ... g_stride 80 holds all but 250 and 81
    r2 = run(c, Q[:5], P2, G2, k_stride=119, g_stride=80)
    assert r2[0].status.tolist() == [B.ERR_INVALID, 0, B.ERR_INVALID, B.ERR_INVALID, B.ERR_INVALID], r2[0].status
    r3 = run(c, Q[:5], P2, G2, k_stride=250, g_stride=80)
    assert r3[0].status.tolist() == [0, 0, B.ERR_INVALID, 0, B.ERR_INVALID], r3[0].status
    check(c, Q[:5], P2, G2, r3, which=(0, 1, 3), what="strides")
    # failures of the call
    import ctypes as C
    hits, grouped = T.Hits(1, 250), T.GroupedHits(1, 250)
    hs, gs = hits.c_struct(), grouped.c_struct()
    hs.mem = B.MEM_DEVICE
    arr = (B.VecQueryC * 1)()
    keep = c.g._fill_vec_query(arr[0], fetch_size=10)
    ga = (B.GroupByC * 1)()
    ga[0].group_limit, ga[0].column = 3, GROUP_COL
    q0 = np.ascontiguousarray(Q[:1])
    assert c.g.L.tsgpu_vector_search_grouped_batch(c.g.h, 1, arr, ga, q0.ctypes.data, B.MEM_HOST, 1, C.byref(hs), C.byref(gs), None) == B.ERR_UNSUPPORTED
    hs.mem = B.MEM_HOST
    assert c.g.L.tsgpu_vector_search_grouped_batch(c.g.h, 9, arr, ga, q0.ctypes.data, B.MEM_HOST, 1, C.byref(hs), C.byref(gs), None) == B.ERR_NOT_FOUND
    assert c.g.L.tsgpu_vector_search_grouped_batch(c.g.h, 1, None, ga, q0.ctypes.data, B.MEM_HOST, 1, C.byref(hs), C.byref(gs), None) == B.ERR_INVALID
    assert c.g.L.tsgpu_vector_search_grouped_batch(c.g.h, 1, arr, ga, q0.ctypes.data, B.MEM_HOST, 1, C.byref(hs), C.byref(gs), None) == 0 and int(hits.status[0]) == 0
    del keep
    c.close()


def case_cost(lib):
    """case 7: ten flat and ten k-cut queries cost one ragged launch, one filtered k-NN batch and one count sync; lists shared by pointer are uploaded once"""
    c = World(lib, 48, B.METRIC_IP)
    g = c.g
    g.set_option("vec_filter_direct_max", 0)                                    # every filtered k-NN query needs a scan: alone, one pass each
    shared = c.pick(130)
    P, G = [], []
    for i in range(10):
        P.append(dict(fetch_size=10, filter_ids=shared if i < 3 else c.pick(60 + 11 * i), flat_search_cutoff=1000)); G.append((3, GROUP_COL, i % 2, 0))
        P.append(dict(fetch_size=10, filter_ids=c.pick(90 + 13 * i), excluded_ids=c.pick(10 + i))); G.append((3, GROUP_COL, i % 2, 0))
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    kc = [i for i, p in enumerate(P) if not V.is_flat(p)]
    passes = lambda: g.counter("vec_prefilter_groups") + g.counter("vec_prefilter_fallbacks")
    s0, q0 = passes(), g.counter("vec_filter_scan_queries")
    g.vec_knn_batch_filtered(1, Q[kc], 10, [(P[i]["filter_ids"], P[i]["excluded_ids"]) for i in kc])
    one_batch, one_batch_q = passes() - s0, g.counter("vec_filter_scan_queries") - q0
    assert 1 <= one_batch < 10 and one_batch_q == 10
    before = c.counters()
    s0, q0 = passes(), g.counter("vec_filter_scan_queries")
    res = run(c, Q, P, G, k_stride=750)
    after = c.counters()
    assert after["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == 1
    assert passes() - s0 == one_batch and g.counter("vec_filter_scan_queries") - q0 == one_batch_q
    assert after["vec_grouped_syncs"] - before["vec_grouped_syncs"] == 1
    assert after["vec_search_pq_flat_lists"] - before["vec_search_pq_flat_lists"] == 8, "the shared list was uploaded more than once"
    assert after["vec_grouped_flat_queries"] - before["vec_grouped_flat_queries"] == 10 and after["vec_grouped_kcut_queries"] - before["vec_grouped_kcut_queries"] == 10
    check(c, Q, P, G, res, what="cost")
    c.close()


def case_concurrency(lib):
    """case 8: eight threads issue the mixed batch at once; each gets the serial answer"""
    c = World(lib, 48, B.METRIC_IP)
    P, G, Q = mixed_batch(c)
    P, G, Q = P[:8], G[:8], Q[:8]                                               # (flat and k-cut queries, both passes; the whole mix is case 1's)
    want = check(c, Q, P, G, run(c, Q, P, G), what="serial")

    def worker(t):
        got = run(c, Q, P, G)
        for i in range(len(P)):
            assert_same(got, i, want, i, G[i], what=("thread", t))
    V.run_threads(8, worker)
    c.close()


def case_ungrouped_unchanged(lib):
    """case 9: a mixed ungrouped per-query batch answers identically before and after grouped calls on the same context, and as the oracle says"""
    c = World(lib, 70, B.METRIC_COSINE)
    P, Q = V.mixed_params(c)
    before = V.run_pq(c, Q, P)
    V.check_oracle(c, Q, P, before, what="before")
    Pg, G, Qg = mixed_batch(c)
    for _ in range(2):
        run(c, Qg, Pg, G)
    after = V.run_pq(c, Q, P)
    for i in range(len(P)):
        V.assert_same(after, i, before, i, what="ungrouped after grouped")
    c.g.set_option("vec_flat_group_max_bytes", 1200)                           # the forced split of the shared distance stage, on both callers
    split = V.run_pq(c, Q, P)
    for i in range(len(P)):
        V.assert_same(split, i, before, i, what="ungrouped, forced split")
    check(c, Qg, Pg, G, run(c, Qg, Pg, G), what="grouped, forced split")
    c.close()
