"""One parameter block per query in a pure vector search batch (tsgpu_vector_search_batch_per_query; vec_flat_ragged_distances_kernel in
vec_kernels.hip.h, the ragged form of KwVFlat in the wildcard planner). Shared by tests/test_emu_vector_search_pq.py (SIMT emulator) and
tests/test_gpu_vector_search_pq.py (MI355X).

Two yardsticks, per query of a batch, no tolerance anywhere:
  (a) the library's own single-block call (tsgpu_vector_search_batch_ids) on that query alone with its block: keys in order, scores,
      vector_distance viewed as uint32, match_score_index, n_hits, num_matched, status, the id list;
  (b) the oracle's search_vector, compared exactly as tests/test_emu_vector.py::_flat_case compares.
The corpus is _flat_case's: a few hundred documents, a third of the rows share one embedding (masses of exact ties), the last 40 documents have no
vector, a few rows are deleted (the oracle has no delete: it is given the live rows only, which is what "not found" means on both branches), an int64
column. The ragged kernel's tile holds 256 items: the flat list lengths 255 / 256 / 257 are its T - 1 / T / T + 1."""
import threading

import numpy as np

from typesense_amd import _lib as B
from tests import helpers as H

K_STRIDE = 320
DEFAULT_SORT = ((B.SORT_VECTOR_DISTANCE, -1, 0), (B.SORT_SEQ_ID, 1, 0))
THREE_KEYS = ((B.SORT_INT64_COLUMN, 1, 0), (B.SORT_VECTOR_DISTANCE, -1, 0), (B.SORT_SEQ_ID, -1, 0))
COUNTERS = ("vec_search_pq_flat_queries", "vec_search_pq_kcut_queries", "vec_search_pq_flat_lists", "vec_search_pq_flat_launches")


class Corpus:
    def __init__(self, lib, dim, metric, n_docs=400, seed=5, deleted=(7, 100, 222)):
        docs = H.zipf_docs(n_docs, 30, 4, seed=seed)
        self.orc, self.g = H.build_pair(docs, lib)
        self.rng = rng = np.random.default_rng(seed)
        self.n_docs, self.dim, self.metric = n_docs, dim, metric
        self.n_vec = n_vec = n_docs - 40                                 # the last 40 documents have no vector
        X = rng.standard_normal((n_vec, dim)).astype(np.float32)
        X[rng.integers(0, n_vec, size=n_vec // 3)] = X[5]                # a third of the rows share one embedding
        X[11] = X[5]
        self.X = X
        self.g.vec_create(1, dim, metric)
        self.g.vec_upsert(1, np.arange(n_vec, dtype=np.uint64), X)
        for d in deleted:
            self.g.vec_delete(1, int(d))
        self.live = np.setdiff1d(np.arange(n_vec, dtype=np.uint32), np.asarray(deleted, np.uint32))
        self.orc.vec_init(dim, metric)
        self.orc.vec_add(self.live, X[self.live])
        self.ties = np.nonzero((X == X[5]).all(axis=1))[0].astype(np.uint32)

    def pick(self, m, among=None):
        among = np.arange(self.n_docs, dtype=np.uint32) if among is None else among
        return np.sort(self.rng.choice(among, size=m, replace=False)).astype(np.uint32)

    def counters(self):
        return {c: self.g.counter(c) for c in COUNTERS}

    def close(self):
        self.orc.close()
        self.g.close()


def mixed_params(c):
    """about 30 blocks, every kind of the issue; returns (params, Q)"""
    thr = 1.02 if c.metric == B.METRIC_COSINE else 0.5
    P = []
    add = lambda **kw: P.append(kw)
    a80, a120 = c.pick(80), c.pick(120)
    add(fetch_size=10)                                                                              # no filter
    add(fetch_size=10, filter_ids=a120, excluded_ids=a120[::7].copy())                              # k-cut with allow and excluded ids
    add(fetch_size=10, filter_ids=np.zeros(0, np.uint32))                                           # filter_by_provided with an empty list
    add(fetch_size=10, filter_ids=a80, flat_search_cutoff=80)                                       # n_filter == flat_search_cutoff: k-cut
    add(fetch_size=10, filter_ids=a80.copy(), flat_search_cutoff=81)                                # n_filter == flat_search_cutoff - 1: flat
    add(fetch_size=10, filter_ids=np.arange(c.n_vec + 3, c.n_vec + 30, dtype=np.uint32), flat_search_cutoff=1000)   # flat, only ids without a vector
    add(fetch_size=30, distance_threshold=thr, filter_ids=c.pick(150), flat_search_cutoff=1000)     # a threshold, flat
    add(fetch_size=30, distance_threshold=thr, filter_ids=c.pick(150))                              # ... k-cut
    add(fetch_size=300, k=7, filter_ids=c.pick(300), flat_search_cutoff=1000)                       # k = 7 with fetch_size = 300, flat (Topster of 300)
    add(fetch_size=300, k=7, filter_ids=c.pick(300), excluded_ids=c.pick(20))                       # ... k-cut
    add(fetch_size=25, k=0)                                                                         # k = 0
    m = c.pick(90, among=c.live)
    add(fetch_size=10, filter_ids=m, flat_search_cutoff=1000, query_doc=int(m[40]))                 # query_doc, flat, a member
    add(fetch_size=10, filter_ids=m.copy(), query_doc=int(m[41]))                                   # query_doc, k-cut, passes the functor: k + 1
    add(fetch_size=10, filter_ids=m.copy(), excluded_ids=m[41:42].copy(), query_doc=int(m[41]))     # query_doc, k-cut, excluded: k stays
    add(fetch_size=10, query_doc=int(c.ties[3]))                                                    # query_doc, k-cut, no filter, in the ties
    add(fetch_size=25, sort=THREE_KEYS, filter_ids=c.pick(200), flat_search_cutoff=1000)            # the three-key sort with the int64 column, flat
    add(fetch_size=25, sort=THREE_KEYS, filter_ids=c.pick(200), excluded_ids=c.pick(30))            # ... k-cut
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):                                            # flat lists around the 16-row trip, the 64-row trip and the 256-item tile
        add(fetch_size=10 + n % 7, filter_ids=c.pick(n), flat_search_cutoff=n + 1, **({"distance_threshold": thr + 0.3} if n % 2 else {}))
    P[-3]["query_doc"] = int(P[-3]["filter_ids"][254])                                              # the last item of a 255-item tile
    P[-1]["query_doc"] = int(P[-1]["filter_ids"][256])                                              # the one item of a second tile
    Q = (c.rng.standard_normal((len(P), c.dim))).astype(np.float32)
    Q[0] = c.X[5]
    Q[3] = c.X[5]
    for i, p in enumerate(P):
        if "query_doc" in p and p["query_doc"] < c.n_vec:
            Q[i] = c.X[p["query_doc"]]                                                              # `vec:([], id: X)`: the caller passes X's stored vector
    return P, Q


def run_pq(c, Q, params, k_stride=K_STRIDE):
    return c.g.vector_search_batch_per_query(1, Q, params, k_stride=k_stride, want_ids=True)


def assert_same(a, i, b, j, what=""):
    """query i of result a == query j of result b, a result = (hits, ids): yardstick (a)'s comparison"""
    (ha, ia), (hb, ib) = a, b
    assert int(ha.status[i]) == int(hb.status[j]), (what, i, ha.status[i], hb.status[j])
    n = int(hb.n_hits[j])
    assert int(ha.n_hits[i]) == n, (what, i, ha.n_hits[i], n)
    assert np.array_equal(ha.keys[i, :n], hb.keys[j, :n]), (what, i, ha.keys[i, :12], hb.keys[j, :12])
    assert np.array_equal(ha.scores[i, :n], hb.scores[j, :n]), (what, i)
    assert np.array_equal(ha.vector_distance[i, :n].view(np.uint32), hb.vector_distance[j, :n].view(np.uint32)), (what, i)
    assert np.array_equal(ha.match_score_index[i, :n], hb.match_score_index[j, :n]), (what, i)
    assert int(ha.num_matched[i]) == int(hb.num_matched[j]), (what, i, ha.num_matched[i], hb.num_matched[j])
    assert int(ha.search_cutoff[i]) == int(hb.search_cutoff[j]), (what, i)
    assert np.array_equal(ia[i], ib[j]), (what, i)


def check_single_calls(c, Q, params, res, which=None, what="", k_stride=K_STRIDE):
    """yardstick (a)"""
    for i in (range(len(params)) if which is None else which):
        one = c.g.vector_search_batch(1, Q[i:i + 1], k_stride=k_stride, want_ids=True, **params[i])
        assert_same(res, i, one, 0, what=(what, "single call", params[i].get("flat_search_cutoff", 0)))


def check_oracle(c, Q, params, res, which=None, what=""):
    """yardstick (b), as tests/test_emu_vector.py::_flat_case"""
    hits, ids = res
    for i in (range(len(params)) if which is None else which):
        p = dict(params[i])
        sort = p.pop("sort", DEFAULT_SORT)
        osort = tuple((s[0], s[2], s[1]) for s in sort)
        ref = c.orc.search_vector(Q[i], sort=osort, cap=2048, ids_cap=c.n_docs, **p)
        n = int(hits.n_hits[i])
        w = (what, "oracle", i, {k: v for k, v in p.items() if not isinstance(v, np.ndarray)})
        assert int(hits.status[i]) == 0, w
        assert n == ref.keys.size, (w, n, ref.keys.size)
        assert np.array_equal(hits.keys[i, :n], ref.keys), (w, hits.keys[i, :12], ref.keys[:12])
        assert np.array_equal(hits.scores[i, :n], ref.scores), w
        assert np.array_equal(hits.vector_distance[i, :n].view(np.uint32), ref.vector_distance.view(np.uint32)), w
        assert np.array_equal(hits.match_score_index[i, :n], ref.match_score_index), w
        assert int(hits.num_matched[i]) == int(ref.n_result_ids), (w, hits.num_matched[i], ref.n_result_ids)
        assert np.array_equal(ids[i], ref.result_ids), w


def is_flat(p):
    f = p.get("filter_ids")
    return f is not None and f.size != 0 and f.size < p.get("flat_search_cutoff", 0)


def case_mixed_batch(lib, dim, metric):
    """case 1: every kind of block in one call"""
    c = Corpus(lib, dim, metric)
    P, Q = mixed_params(c)
    before = c.counters()
    res = run_pq(c, Q, P)
    after = c.counters()
    n_flat = sum(is_flat(p) for p in P)
    assert n_flat >= 14 and len(P) - n_flat >= 10
    assert after["vec_search_pq_flat_queries"] - before["vec_search_pq_flat_queries"] == n_flat
    assert after["vec_search_pq_kcut_queries"] - before["vec_search_pq_kcut_queries"] == len(P) - n_flat
    assert after["vec_search_pq_flat_lists"] - before["vec_search_pq_flat_lists"] == n_flat        # (every list is an array of its own)
    assert after["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == 1
    assert (res[0].status == 0).all()
    assert int(res[0].n_hits[5]) == 0 and res[1][5].size == 0                                      # the flat list made only of ids without a vector
    check_single_calls(c, Q, P, res, what=(dim, metric))
    check_oracle(c, Q, P, res, what=(dim, metric))
    c.close()


def case_shared_lists(lib):
    """case 2: three non-adjacent queries pass the same array with different query documents (two members, one absent) and thresholds"""
    c = Corpus(lib, 48, B.METRIC_IP)
    A = c.pick(130, among=c.live)
    absent = int(np.setdiff1d(c.live, A)[9])
    other, kc = c.pick(70), c.pick(60)
    P = [dict(fetch_size=10, filter_ids=A, flat_search_cutoff=500, query_doc=int(A[17]), distance_threshold=0.9),
         dict(fetch_size=10, filter_ids=other, flat_search_cutoff=500),
         dict(fetch_size=20, filter_ids=A, flat_search_cutoff=131, query_doc=int(A[129]), distance_threshold=1.4),
         dict(fetch_size=10, filter_ids=kc),
         dict(fetch_size=10, filter_ids=A, flat_search_cutoff=500, query_doc=absent)]
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    for i in (0, 2, 4):
        Q[i] = c.X[P[i]["query_doc"]]
    before = c.counters()
    res = run_pq(c, Q, P)
    after = c.counters()
    assert after["vec_search_pq_flat_lists"] - before["vec_search_pq_flat_lists"] == 2, "A was not recognised as one list"
    assert after["vec_search_pq_flat_queries"] - before["vec_search_pq_flat_queries"] == 4
    assert after["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == 1
    for i, qd in ((0, int(A[17])), (2, int(A[129]))):
        assert qd not in res[0].keys[i, :int(res[0].n_hits[i])].tolist() and qd not in res[1][i].tolist()
    check_single_calls(c, Q, P, res, what="shared")
    check_oracle(c, Q, P, res, what="shared")
    c.close()


def case_different_k(lib):
    """case 3: k from 1 to 200 in ONE k-cut group over the tie-heavy rows, with and without query_doc: every query keeps a prefix of the K = 201 nearest"""
    c = Corpus(lib, 24, B.METRIC_COSINE)
    allow = np.union1d(c.ties[::2], c.pick(150)).astype(np.uint32)
    P = []
    for j, k in enumerate((1, 2, 3, 7, 31, 64, 100, 150, 199, 200)):
        P.append(dict(k=k, fetch_size=10))
        P.append(dict(k=k, fetch_size=10, query_doc=int(c.ties[4 + j])))
        if j % 3 == 0:
            P.append(dict(k=k, fetch_size=10, filter_ids=allow, excluded_ids=allow[::9].copy(), query_doc=int(allow[5 * j + 2])))
    Q = np.repeat(c.X[5][None, :], len(P), axis=0).copy()                        # every query IS the shared embedding: the ties are its nearest
    Q[1::5] += (c.rng.standard_normal((len(Q[1::5]), c.dim)) * 0.01).astype(np.float32)
    before = c.counters()
    res = run_pq(c, Q, P)
    assert c.counters()["vec_search_pq_kcut_queries"] - before["vec_search_pq_kcut_queries"] == len(P)
    assert len(set(int(n) for n in res[0].n_hits)) > 5                           # (the prefixes differ in length)
    check_single_calls(c, Q, P, res, what="different k")
    check_oracle(c, Q, P, res, what="different k")
    c.close()


def _scan_passes(g):
    return g.counter("vec_prefilter_groups") + g.counter("vec_prefilter_fallbacks")


def case_one_pass(lib):
    """case 4: 10 flat and 10 filtered k-cut queries: one ragged launch, and the k-NN pass counters move by what ONE filtered batch of the 10 costs"""
    c = Corpus(lib, 48, B.METRIC_IP)
    g = c.g
    g.set_option("vec_filter_direct_max", 0)                                     # every filtered k-NN query needs a scan: alone, one pass each
    P = []
    for i in range(10):
        P.append(dict(fetch_size=10, filter_ids=c.pick(60 + 11 * i), flat_search_cutoff=1000))
        P.append(dict(fetch_size=10, filter_ids=c.pick(90 + 13 * i), excluded_ids=c.pick(10 + i)))
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    kc = [i for i, p in enumerate(P) if not is_flat(p)]
    s0, q0 = _scan_passes(g), g.counter("vec_filter_scan_queries")
    g.vec_knn_batch_filtered(1, Q[kc], 10, [(P[i]["filter_ids"], P[i]["excluded_ids"]) for i in kc])
    one_batch, one_batch_q = _scan_passes(g) - s0, g.counter("vec_filter_scan_queries") - q0
    assert 1 <= one_batch < 10 and one_batch_q == 10
    before = c.counters()
    s0, q0 = _scan_passes(g), g.counter("vec_filter_scan_queries")
    res = run_pq(c, Q, P)
    after = c.counters()
    assert after["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == 1
    assert _scan_passes(g) - s0 == one_batch, "the k-cut queries cost %d scan passes, one filtered batch of them costs %d" % (_scan_passes(g) - s0, one_batch)
    assert g.counter("vec_filter_scan_queries") - q0 == one_batch_q
    check_single_calls(c, Q, P, res, which=range(0, len(P), 3), what="one pass")
    check_oracle(c, Q, P, res, what="one pass")
    c.close()


def case_forced_split(lib):
    """case 5: "vec_flat_group_max_bytes" small enough for at least 3 groups: the same results, one launch per group"""
    c = Corpus(lib, 70, B.METRIC_COSINE)
    sizes = (100, 40, 257, 60, 90, 30, 120, 10, 256, 80)
    P = [dict(fetch_size=10, filter_ids=c.pick(n), flat_search_cutoff=1000) for n in sizes]
    P.insert(4, dict(fetch_size=10, filter_ids=c.pick(50)))                     # a k-cut query in between
    P[1]["query_doc"] = int(P[1]["filter_ids"][7])
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    whole = run_pq(c, Q, P)
    cap = 1200                                                                  # bytes: 300 distances
    groups, acc = 1, 0
    for n in sizes:                                                             # consecutive flat queries while their segments fit; a larger one alone
        if acc and acc + 4 * n > cap:
            groups, acc = groups + 1, 0
        acc += 4 * n
    assert groups >= 3
    c.g.set_option("vec_flat_group_max_bytes", cap)
    before = c.counters()
    split = run_pq(c, Q, P)
    assert c.counters()["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == groups
    for i in range(len(P)):
        assert_same(split, i, whole, i, what="forced split")
    check_single_calls(c, Q, P, split, which=(0, 2, 4, 9), what="forced split")
    check_oracle(c, Q, P, split, what="forced split")
    c.close()


def case_refusals(lib):
    """case 6: what the single call refuses as a call for reasons in the block is the query's status; its neighbours are answered"""
    c = Corpus(lib, 24, B.METRIC_IP)
    good_flat = lambda: dict(fetch_size=10, filter_ids=c.pick(70), flat_search_cutoff=1000)
    good_kcut = lambda: dict(fetch_size=10, filter_ids=c.pick(110), excluded_ids=c.pick(9))
    bad = {1: (dict(fetch_size=10, sort=((B.SORT_EVAL, 1, 0), (B.SORT_SEQ_ID, 1, 0))), B.ERR_UNSUPPORTED),
           3: (dict(fetch_size=10, n_sort=4, sort=THREE_KEYS, filter_ids=c.pick(50), flat_search_cutoff=1000), B.ERR_INVALID),
           4: (dict(k=1025, fetch_size=10), B.ERR_UNSUPPORTED),
           6: (dict(k=0, fetch_size=0, filter_ids=c.pick(40)), B.ERR_INVALID)}
    P = [bad[i][0] if i in bad else (good_flat() if i % 2 == 0 else good_kcut()) for i in range(9)]
    Q = c.rng.standard_normal((len(P), c.dim)).astype(np.float32)
    hits, ids = res = run_pq(c, Q, P)
    good = [i for i in range(len(P)) if i not in bad]
    assert hits.status.tolist() == [bad[i][1] if i in bad else 0 for i in range(len(P))]
    for i in bad:
        assert int(hits.n_hits[i]) == 0 and int(hits.num_matched[i]) == 0 and ids[i].size == 0, i
        if "n_sort" in P[i]:
            continue                                                            # (vector_search_batch takes the count from the tuple)
        try:                                                                    # the single call refuses the same block, with the same code
            code = int(c.g.vector_search_batch(1, Q[i:i + 1], k_stride=K_STRIDE, **P[i]).status[0])    # (the _eval refusal: the call is OK, every query carries 501)
        except B.TsgpuError as e:
            code = e.code
        assert code == bad[i][1], (i, code)
    check_single_calls(c, Q, P, res, which=good, what="refusals")
    check_oracle(c, Q, P, res, which=good, what="refusals")
    # k_stride too small for ONE query: its Topster of 300 does not fit 250 slots, the others do
    P2 = [good_flat(), dict(fetch_size=300, filter_ids=c.pick(300), flat_search_cutoff=1000), good_kcut(), dict(fetch_size=300, k=300, filter_ids=c.pick(300))]
    r2 = run_pq(c, Q[:4], P2, k_stride=250)
    assert r2[0].status.tolist() == [0, B.ERR_INVALID, 0, B.ERR_INVALID] and int(r2[0].n_hits[1]) == 0 and int(r2[0].n_hits[3]) == 0
    check_single_calls(c, Q[:4], P2, r2, which=(0, 2), what="k_stride", k_stride=250)
    # n_q == 0: OK, an empty list object
    h0, i0 = run_pq(c, np.zeros((0, c.dim), np.float32), [])
    assert h0.n_hits.size == 0 and i0 == []
    # failures of the call
    for field, code in ((9, B.ERR_NOT_FOUND),):
        try:
            c.g.vec_dim[field] = c.dim
            c.g.vector_search_batch_per_query(field, Q[:1], [good_kcut()])
            raise AssertionError("an unknown field was served")
        except B.TsgpuError as e:
            assert e.code == code
        finally:
            del c.g.vec_dim[field]
    c.close()


def run_threads(n_threads, worker):
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


def case_concurrency(lib):
    """case 7: 8 threads issue the mixed batch at once; every result equals the serial one"""
    c = Corpus(lib, 48, B.METRIC_IP)
    P, Q = mixed_params(c)
    want = run_pq(c, Q, P)
    check_oracle(c, Q, P, want, what="serial")

    def worker(t):
        got = run_pq(c, Q, P)
        for i in range(len(P)):
            assert_same(got, i, want, i, what=("thread", t))
    run_threads(8, worker)
    c.close()


def case_medium(lib, n=20000, dim=96, n_q=300):
    """case 8 (GPU): every query its own list, from 50 ids to 60 % of the rows, about half on each branch; the oracle for every query, the single call
    for every tenth"""
    docs = H.zipf_docs(n, 30, 4, seed=9)
    c = Corpus.__new__(Corpus)
    c.orc, c.g = H.build_pair(docs, lib)
    c.rng = rng = np.random.default_rng(41)
    c.n_docs, c.dim, c.metric, c.n_vec = n, dim, B.METRIC_IP, n
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[rng.integers(0, n, size=n // 50)] = X[5]
    c.g.vec_create(1, dim, B.METRIC_IP)
    c.g.vec_upsert(1, np.arange(n, dtype=np.uint64), X)
    deleted = (7, 12345)
    for d in deleted:
        c.g.vec_delete(1, d)
    c.live = np.setdiff1d(np.arange(n, dtype=np.uint32), np.asarray(deleted, np.uint32))
    c.orc.vec_init(dim, B.METRIC_IP)
    c.orc.vec_add(c.live, X[c.live])
    Q = rng.standard_normal((n_q, dim)).astype(np.float32)
    sizes = np.linspace(50, 0.6 * n, n_q).astype(np.int64)
    P = []
    for i in range(n_q):
        a = np.sort(rng.choice(n, size=int(sizes[i]), replace=False)).astype(np.uint32)
        p = dict(fetch_size=10, k=100, filter_ids=a)
        if i % 2 == 0:
            p["flat_search_cutoff"] = int(sizes[i]) + 1                          # flat: every id through a Topster of 250
        elif i % 4 == 1:
            p["excluded_ids"] = a[::5].copy()
        if i % 7 == 0:
            p["query_doc"] = int(a[a.size // 3])
        if i % 5 == 0:
            p["distance_threshold"] = 1.5
        P.append(p)
    before = c.counters()
    res = c.g.vector_search_batch_per_query(1, Q, P, k_stride=250, want_ids=True)
    after = c.counters()
    assert after["vec_search_pq_flat_queries"] - before["vec_search_pq_flat_queries"] == n_q // 2
    assert after["vec_search_pq_kcut_queries"] - before["vec_search_pq_kcut_queries"] == n_q - n_q // 2
    assert after["vec_search_pq_flat_launches"] - before["vec_search_pq_flat_launches"] == 1
    check_oracle(c, Q, P, res, what="medium")
    check_single_calls(c, Q, P, res, which=range(0, n_q, 10), what="medium", k_stride=250)
    check_single_calls(c, Q, P, res, which=range(5, n_q, 30), what="medium", k_stride=250)     # (every tenth is even = flat: some k-cut queries too)
    c.close()
