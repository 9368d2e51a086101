"""Shared bodies of tests/test_emu_vq_sort.py (CPU tier, SIMT emulator) and tests/test_gpu_vq_sort.py (-m gpu, libtsgpu.so): the sort kind
TSGPU_SORT_VECTOR_QUERY — `sort_by=_vector_query(field:([...]))`, Index::compute_sort_scores, reference src/index.cpp:5837-5851 — against the oracle.

Expected values are never made by the code under test. Per document, restated here:
    v[d] = float_to_int64_t(2.0f)                                  no live row of the key's field for seq_id d (getDataByLabel throws, :5851)
    v[d] = float_to_int64_t(dist > threshold ? FLT_MAX : dist)     dist = dist_func(q, row) (:5842-5850)
with dist from the HOST function tsgpu_ip_distance(q, row, dim, lanes) (held to the oracle's orc_ip_distance for lanes = 4), rows and cosine queries
normalised in numpy with hnsw_index_t::normalize_vector's arithmetic (include/index.h:379-388). v is loaded into a stand-in int64 column of the oracle and
every hit compared with the oracle's result for the twin query, exactly as sortkeys_common.World.twin does for `_eval`: keys in order, all three scores,
text_match, num_matched; no tolerance."""
import threading

import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O
from tests import helpers as H
from tests import sortkeys_common as S
from tests.test_vector_pins import f2i, i2f, bits, pins, QIP, F32_MAX

VQ = B.SORT_VECTOR_QUERY
TM = (B.SORT_TEXT_MATCH, 1, 0)
NO_ROW = int(f2i(np.float32(2.0)))
RUNS = (1, 15, 16, 17, 63, 64, 65)          # emitting hits of one work item: a lone hit, around a quad trip (16), around a wavefront (64)
RUN_TOKEN = 1000                             # token RUN_TOKEN + n is in exactly n documents of field 0


def normalize_rows(X):
    """hnsw_index_t::normalize_vector per row: sequential fp32 sum of squares (multiply and add rounded separately), x * 1 / (sqrt(sum) + 1e-30)"""
    X = np.array(X, np.float32, ndmin=2)
    norm = np.zeros(X.shape[0], np.float32)
    for i in range(X.shape[1]):
        norm = norm + X[:, i] * X[:, i]
    inv = np.float32(1.0) / (np.sqrt(norm) + np.float32(1e-30))
    return (X * inv[:, None]).astype(np.float32)


def mixed_rows(n, dim, seed):
    """Gaussian rows at the even positions; small-integer rows (every product and sum exact, ties everywhere) at the odd ones"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[1::2] = rng.integers(-2, 3, size=X[1::2].shape).astype(np.float32)
    return X


class Field:
    """host mirror of one vector field: the rows AS STORED (cosine: normalised), label -> row, live flags"""

    def __init__(self, dim, metric):
        self.dim, self.metric = dim, metric
        self.X = np.zeros((0, dim), np.float32)
        self.row_of, self.live = {}, {}
        self.version = 0

    def upsert(self, labels, X):
        X = np.array(X, np.float32, ndmin=2)
        X = normalize_rows(X) if self.metric == B.METRIC_COSINE else X
        new = [i for i, l in enumerate(labels) if int(l) not in self.row_of]
        for i, l in enumerate(labels):
            if int(l) in self.row_of:
                self.X[self.row_of[int(l)]] = X[i]
            self.live[int(l)] = True
        base = self.X.shape[0]
        self.X = np.ascontiguousarray(np.concatenate([self.X, X[new]]))
        for j, i in enumerate(new):
            self.row_of[int(labels[i])] = base + j
        self.version += 1

    def delete(self, label):
        self.live[int(label)] = False
        self.version += 1


class VqWorld(S.World):
    """sortkeys_common.World's collection (same fields, columns and oracle), with RUN tokens in field 0, plus vector fields mirrored on the host"""

    def __init__(self, n_docs, lib_path):
        self.n_docs = n_docs
        rng = np.random.default_rng(5)
        f0 = H.zipf_docs(n_docs, 300, 12, seed=1)
        f1 = H.zipf_docs(n_docs, 300, 6, seed=2)
        picked = np.sort(rng.choice(n_docs, size=sum(RUNS), replace=False))
        self.run_docs, at = {}, 0
        for n in RUNS:
            self.run_docs[n] = picked[at:at + n]
            f0[picked[at:at + n], 11] = RUN_TOKEN + n
            at += n
        self.orc = orc = O.OracleIndex(3, S.SCRATCH + 3)
        for d in range(n_docs):
            orc.index_plain(d, 0, f0[d])
            orc.index_plain(d, 1, f1[d])
            if d % 3 != 0:
                orc.index_array(d, 2, [list(f1[d][:2]), list(f0[d][:3]), [int(f0[d][5])]])
        orc.set_num_docs(n_docs)
        self.pts = H.points_of(n_docs)
        from tests.test_emu_groupby import group_column
        self.distinct, self.has_value = group_column(n_docs, seed=3)
        orc.set_sort_dense(S.PTS, self.pts)
        self.g = g = T.GpuIndex(0, lib_path)
        for f in (0, 1, 2):
            g.field_create(f, f == 2)
            for term in orc.terms(f):
                ids, oi, off = orc.dump_posting(f, int(term))
                g.term_upsert(f, int(term), ids, oi, off)
        g.column_set(S.PTS, self.pts)
        g.column_set(S.GROUP, self.distinct.view(np.int64))
        g.set_num_docs(n_docs)
        g.commit()
        self.keys = {}                      # _eval keys (S.World.key / drop)
        self.vkeys = {}                     # handle -> (field id, query, threshold or None)
        self.fields = {}
        self.lanes = 4
        self.seen = set()                   # coverage: what the checked hits have exercised
        self._cache = {}

    # ---- vector fields and keys ----
    def add_field(self, fid, dim, metric, labels, X):
        self.g.vec_create(fid, dim, metric)
        self.fields[fid] = Field(dim, metric)
        self.upsert(fid, labels, X)

    def upsert(self, fid, labels, X):
        labels = np.asarray(labels, np.uint64)
        self.g.vec_upsert(fid, labels, np.ascontiguousarray(X, np.float32))
        self.fields[fid].upsert(labels.tolist(), X)

    def delete(self, fid, label):
        self.g.vec_delete(fid, int(label))
        self.fields[fid].delete(label)

    def set_lanes(self, lanes):
        self.g.set_option("vec_ip_lanes", lanes)
        self.lanes = lanes

    def vkey(self, fid, q, thr=None):
        q = np.ascontiguousarray(q, np.float32)
        h = self.g.sort_key_create_vector_query(fid, q, thr)
        self.vkeys[h] = (fid, q, thr)
        return h

    def drop(self, h):
        if h in self.vkeys:
            self.g.sort_key_destroy(h)
            del self.vkeys[h]
        else:
            S.World.drop(self, h)

    def distances(self, fid, q):
        """raw distance per seq_id (NaN: no live row) by the host function, in the summation order in force"""
        f = self.fields[fid]
        qs = normalize_rows(q)[0] if f.metric == B.METRIC_COSINE else np.ascontiguousarray(q, np.float32)
        qs = np.ascontiguousarray(qs)
        d = np.full(self.n_docs, np.nan, np.float32)
        L, base, stride = self.g.L, f.X.ctypes.data, f.dim * 4
        olib = O.lib()
        for label, row in f.row_of.items():
            if label < self.n_docs and f.live[label]:
                d[label] = L.tsgpu_ip_distance(qs.ctypes.data, base + row * stride, f.dim, self.lanes)
                if self.lanes == 4 and row % 16 == 0:
                    assert bits(d[label]) == bits(np.float32(olib.orc_ip_distance(qs.ctypes.data, base + row * stride, f.dim))), (fid, label)
        return d

    def key_values(self, h):
        fid, q, thr = self.vkeys[h]
        ck = (h, fid, self.lanes, self.fields[fid].version, q.tobytes(), thr)
        if ck not in self._cache:
            d = self.distances(fid, q)
            has = ~np.isnan(d)
            t = np.where(has & (d > np.float32(B.FLT_MAX if thr is None else thr)), F32_MAX, d).astype(np.float32)
            v = np.where(has, f2i(np.where(has, t, np.float32(0))), NO_ROW).astype(np.int64)
            self._cache = {k: x for k, x in self._cache.items() if k[0] != h}
            self._cache[ck] = (v, d)
        return self._cache[ck]

    def twin(self, q):
        sort = []
        for i, (kind, order, col) in enumerate(q.sort):
            if kind < B.SORT_EVAL:
                sort.append((kind, order, col))
                continue
            assert kind in (VQ, B.SORT_EVAL)
            v = self.key_values(col)[0] if kind == VQ else S.eval_key(self.n_docs, *self.keys[col])
            self.orc.set_sort_dense(S.SCRATCH + i, v)
            sort.append((B.SORT_INT64_COLUMN, order, S.SCRATCH + i))
        return T.KwQuery(q.tokens, sort=tuple(sort), topster_size=q.topster_size, fields=q.fields, match_type=q.match_type, excluded_ids=q.excluded_ids,
                         filter_ids=q.filter_ids, dropped_tokens=q.dropped_tokens, total_cost=q.total_cost)

    # ---- coverage: which cases of the slot's definition did the hits just checked exercise? ----
    def note(self, q, keys, num_matched):
        keys = np.asarray(keys).astype(np.int64)
        if q.topster_size and num_matched > q.topster_size:
            self.seen.add("topster smaller than the match count")
        if q.excluded_ids is not None:
            self.seen.add("excluded ids")
        if q.filter_ids is not None:
            self.seen.add("filter ids")
        slots = [s for s in q.sort if s[0] == VQ]
        if len({self.vkeys[s[2]][0] for s in slots}) >= 2:
            self.seen.add("two vector slots on different fields")
        if slots and any(s[0] == B.SORT_EVAL for s in q.sort):
            self.seen.add("a vector slot with an _eval slot")
        for kind, order, h in slots:
            fid, _, thr = self.vkeys[h]
            f = self.fields[fid]
            d = self.key_values(h)[1][keys]
            if order == 1:
                self.seen.add("DESC")
            if (np.isnan(d) & np.array([int(k) not in f.row_of for k in keys], bool)).any():
                self.seen.add("no row")
            if any(int(k) in f.row_of and not f.live[int(k)] for k in keys):
                self.seen.add("deleted row")
            if (d < 0).any():
                self.seen.add("negative distance")
            if thr is not None:
                for name, m in (("above", d > np.float32(thr)), ("equal", d == np.float32(thr)), ("below", d < np.float32(thr))):
                    if m.any():
                        self.seen.add(name + " the threshold")

    def check_keyword(self, qs, what, k_stride=250):
        hits = S.World.check_keyword(self, qs, what, k_stride)
        for i, q in enumerate(qs):
            self.note(q, hits.keys[i, :int(hits.n_hits[i])], int(hits.num_matched[i]))
        return hits

    def check_wildcard(self, qs, what, k_stride=250):
        hits = S.World.check_wildcard(self, qs, what, k_stride)
        for i, q in enumerate(qs):
            self.note(q, hits.keys[i, :int(hits.n_hits[i])], int(hits.num_matched[i]))
        return hits


# ------------------------------------------------------------------------------------------------ 1. the reference's own expectations
def run_reference_pin(lib_path):
    """TestDistanceThresholdWithIP (reference test/collection_vector_search_test.cpp:5093-5196): the five seed-47 documents, sort_by
    _vector_query(vec:([...], distance_threshold: 1)):asc, rank_score:desc. The printed key is -int64_t_to_float(-float_to_int64_t(d)) (src/collection.cpp:3181-3183):
    FLT_MAX comes back as 3.4028232635611926e+38 (the pin of tests/test_vector_pins.py)."""
    P = pins()
    docs = np.array(P["seed47_ip_docs"], np.float32)
    rank = np.array(P["seed47_ip_rank_scores"], np.int64)
    g = T.GpuIndex(0, lib_path)
    try:
        g.field_create(0, False)
        g.term_upsert(0, 1, np.arange(5, dtype=np.uint32), np.arange(5, dtype=np.uint32), np.ones(5, np.uint32))
        g.column_set(0, rank)
        g.set_num_docs(5)
        g.commit()
        g.vec_create(3, 5, B.METRIC_IP)
        g.vec_upsert(3, np.arange(5, dtype=np.uint64), docs)
        h = g.sort_key_create_vector_query(3, QIP, 1.0)
        sort = ((VQ, -1, h), (B.SORT_INT64_COLUMN, 1, 0))
        want = np.array([0.2189185470342636, 0.7371898889541626] + [3.4028232635611926e+38] * 3, np.float32)
        for hits in (g.wildcard_search_batch([T.KwQuery([], sort=sort)], k_stride=10), g.keyword_search_batch([T.KwQuery([1], sort=sort)], k_stride=10)):
            assert hits.status[0] == 0 and int(hits.n_hits[0]) == 5
            assert [int(rank[int(k)]) for k in hits.keys[0, :5]] == [93, 51, 94, 80, 18]
            got = -i2f(hits.scores[0, :5, 0])
            assert np.array_equal(bits(got), bits(want)), (got, want)
            assert np.array_equal(hits.scores[0, :5, 1], rank[hits.keys[0, :5].astype(np.int64)])
        g.sort_key_destroy(h)
        h = g.sort_key_create_vector_query(3, np.full(5, -100.0, np.float32))
        want = np.array([-45.23314666748047, -38.66290283203125, -36.0988655090332, 9.637892723083496, 288.0364685058594], np.float32)
        for hits in (g.wildcard_search_batch([T.KwQuery([], sort=((VQ, -1, h),))], k_stride=10), g.keyword_search_batch([T.KwQuery([1], sort=((VQ, -1, h),))], k_stride=10)):
            assert hits.status[0] == 0 and hits.keys[0, :5].tolist() == [1, 2, 4, 3, 0]
            got = -i2f(hits.scores[0, :5, 0])
            assert np.array_equal(bits(got), bits(want)), (got, want)
        g.sort_key_destroy(h)
        assert g.counter("sort_keys_live") == 0
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 2. distance bits
def run_distance_bits(w, fid, dim, metric):
    """one field of `dim` dimensions: every summation order, Gaussian and integer queries, runs of 1 .. 65 emitting hits (a 65-hit work item: one wave full, one
    with a single hit, two that emit nothing), a filtered run, and a common token whose hits fill whole workgroups; second slot seq_id"""
    n = w.n_docs
    w.add_field(fid, dim, metric, np.arange(n - 50, dtype=np.uint64), mixed_rows(n - 50, dim, seed=100 + dim))
    rng = np.random.default_rng(dim)
    queries = [rng.standard_normal(dim).astype(np.float32) * np.float32(1.5), rng.integers(-2, 3, dim).astype(np.float32)]
    try:
        for lanes in (4, 8, 16):
            w.set_lanes(lanes)
            hs = [w.vkey(fid, q) for q in queries]
            try:
                qs = []
                for h in hs:
                    for order in (-1, 1):
                        sort = ((VQ, order, h), (B.SORT_SEQ_ID, 1, 0))
                        qs += [T.KwQuery([RUN_TOKEN + r], sort=sort, topster_size=250) for r in RUNS]
                        qs.append(T.KwQuery([RUN_TOKEN + 65], sort=sort, topster_size=250, filter_ids=w.run_docs[65][::3]))
                    qs.append(T.KwQuery([1], sort=((VQ, -1, h), (B.SORT_SEQ_ID, 1, 0)), topster_size=40))
                hits = w.check_keyword(qs, "bits dim=%d metric=%d lanes=%d" % (dim, metric, lanes))
                assert [int(x) for x in hits.num_matched[:len(RUNS)]] == list(RUNS)
                if lanes == 4:      # integer query over integer rows: exact distances, and they tie
                    d = w.key_values(hs[1])[1][1::2]
                    d = d[~np.isnan(d)]
                    assert metric != B.METRIC_IP or (np.array_equal(d, np.round(d)) and np.unique(d).size < d.size // 4)
            finally:
                for h in hs:
                    w.drop(h)
    finally:
        w.set_lanes(4)
    assert w.g.counter("sort_keys_live") == 0


# ------------------------------------------------------------------------------------------------ 3. + 4. semantics, every entry point
F_ID, F_OFF, F_SHUF = 20, 21, 22


def add_semantics_fields(w, d_id, d_off, d_shuf):
    """F_ID: identity labels, the last 100 documents have no row, deleted rows; F_OFF: cosine, labels = row + 1000 (the first 1000 documents have no row);
    F_SHUF: a shuffled label map with gaps, deleted rows"""
    n = w.n_docs
    rng = np.random.default_rng(77)
    w.add_field(F_ID, d_id, B.METRIC_IP, np.arange(n - 100, dtype=np.uint64), mixed_rows(n - 100, d_id, seed=1))
    w.add_field(F_OFF, d_off, B.METRIC_COSINE, np.arange(n - 1000, dtype=np.uint64) + 1000, mixed_rows(n - 1000, d_off, seed=2))
    labels = rng.permutation(n)[: n - n // 5].astype(np.uint64)
    w.add_field(F_SHUF, d_shuf, B.METRIC_IP, labels, mixed_rows(labels.size, d_shuf, seed=3))
    for label in np.arange(3, n - 100, 7):
        w.delete(F_ID, label)
    for label in labels[::9]:
        w.delete(F_SHUF, label)


def semantic_keys(w):
    rng = np.random.default_rng(9)
    q_id = rng.standard_normal(w.fields[F_ID].dim).astype(np.float32) * np.float32(2)
    q_int = rng.integers(-2, 3, w.fields[F_ID].dim).astype(np.float32)
    d_int = w.distances(F_ID, q_int)
    thr_equal = float(np.nanmin(d_int[1::2]))             # the smallest distance of an integer row: exact; the rows that share it stay, and lead an ASC order
    q_off = rng.standard_normal(w.fields[F_OFF].dim).astype(np.float32)
    q_shuf = rng.standard_normal(w.fields[F_SHUF].dim).astype(np.float32) * np.float32(2)
    return {"id": w.vkey(F_ID, q_id), "id_thr": w.vkey(F_ID, q_int, thr_equal), "off": w.vkey(F_OFF, q_off, 1.0), "shuf": w.vkey(F_SHUF, q_shuf),
            "shuf_thr": w.vkey(F_SHUF, q_shuf, 0.5)}


def vq_sorts(k):
    PT = (B.SORT_INT64_COLUMN, 1, S.PTS)
    return [((VQ, -1, k["id"]), TM, PT), ((VQ, -1, k["id_thr"]), (B.SORT_SEQ_ID, -1, 0)), (TM, (VQ, -1, k["off"]), PT), (TM, PT, (VQ, 1, k["shuf"])),
            ((VQ, -1, k["shuf_thr"]), (VQ, -1, k["id_thr"]), TM), ((VQ, -1, k["off"]), (VQ, 1, k["id"]), (VQ, -1, k["shuf"]))]


def run_semantics_and_entry_points(w):
    """every ranking path x the slot in every position, ASC and DESC, with and without thresholds, alone, doubled, tripled and next to an `_eval` slot"""
    from tests.test_emu_groupby import check_query, oracle_grouped
    g, n = w.g, w.n_docs
    k = semantic_keys(w)
    ev = w.key([np.arange(0, n, 3), np.arange(0, n, 2)], [50, -7])
    try:
        sorts = vq_sorts(k) + [((B.SORT_EVAL, 1, ev), (VQ, -1, k["id"]), TM), ((VQ, -1, k["shuf"]), (B.SORT_EVAL, -1, ev))]
        filt, excl, f2 = np.arange(0, n, 2), np.arange(0, n, 7), ((0, 15), (1, 7))
        plain = ((TM, (B.SORT_INT64_COLUMN, 1, S.PTS)), ((B.SORT_SEQ_ID, -1, 0),))
        for ts in (5, 250):
            ks = max(ts, 8)
            # 1-, 2-, 3-token single field (find + score kernels); the batch mixes keyed, differently keyed and plain queries
            qs = [T.KwQuery(t, sort=s, topster_size=ts) for s in sorts + list(plain) for t in ([1], [2, 1], [3, 1, 2])]
            w.check_keyword(qs, "single field ts=%d" % ts, k_stride=ks)
            sel = sorts[::2] if ts == 5 else sorts
            qs = [T.KwQuery([1, 2, 3, 4], sort=s, topster_size=ts) for s in sel]                           # more than 3 tokens
            qs += [T.KwQuery([1, 2], fields=f2, sort=s, topster_size=ts) for s in sel]                     # two query_by fields
            qs += [T.KwQuery([2, 1], fields=((2, 15),), sort=s, topster_size=ts) for s in sel]            # a string[] field
            qs += [T.KwQuery([1, 2], sort=s, topster_size=ts, filter_ids=filt) for s in sel]
            qs += [T.KwQuery([1], sort=s, topster_size=ts, excluded_ids=excl) for s in sel]
            qs += [T.KwQuery([2, 1], fields=f2, sort=s, topster_size=ts, filter_ids=filt, excluded_ids=excl) for s in sel[:3]]
            w.check_keyword(qs, "general paths ts=%d" % ts, k_stride=ks)
            g.set_option("kw_two_kernels", 0)                                                              # the fused kernel
            try:
                w.check_keyword([T.KwQuery(t, sort=s, topster_size=ts) for s in sel for t in ([1], [3, 1, 2])], "fused ts=%d" % ts, k_stride=ks)
            finally:
                g.set_option("kw_two_kernels", 1)
            g.set_option("kw_device_plan_min_queries", 1)                                                  # the device-side planner carries the slot
            try:
                n0 = g.counter("kw_device_plans")
                w.check_keyword([T.KwQuery([2, 1], sort=s, topster_size=ts) for s in sel], "device plan ts=%d" % ts, k_stride=ks)
                assert g.counter("kw_device_plans") == n0 + 1
            finally:
                g.set_option("kw_device_plan_min_queries", 512)
            qs = [T.KwQuery([], sort=s, topster_size=ts) for s in sel] + [T.KwQuery([], sort=s, topster_size=ts, filter_ids=filt, excluded_ids=excl) for s in sel]
            w.check_wildcard(qs, "wildcard ts=%d" % ts, k_stride=ks)
        # candidate folding
        groups = [[T.KwQuery(t, sort=s, topster_size=250) for t in ([1, 2], [1, 3], [2, 3], [1])] for s in sorts[::2]]
        hits, qidx, found = g.keyword_search_candidates_batch(groups, k_stride=250)
        assert (hits.status == 0).all()
        for gi, combos in enumerate(groups):
            ref, ref_qi = H.oracle_candidates(w.orc, [w.twin(c) for c in combos])
            H.assert_hits_equal(hits, gi, ref, "candidates g%d" % gi)
            assert np.array_equal(qidx[gi, :int(hits.n_hits[gi])], ref_qi)
        # both group_by passes, and the grouped candidate combinations
        for first_pass in (True, False):
            qs = [T.KwQuery(t, sort=s, topster_size=ts) for s in sorts[1::2] for t, ts in (([1], 250), ([2, 1], 5))]
            h, gh = g.keyword_search_grouped_batch(qs, [(3, S.GROUP, int(first_pass), 0, 0)] * len(qs), k_stride=750, g_stride=250)
            for i, q in enumerate(qs):
                check_query(h, gh, i, oracle_grouped(w.orc, w.twin(q), w.distinct, w.has_value, 3, first_pass), first_pass, 3, "grouped")
            users = [[T.KwQuery(t, sort=s, topster_size=40, total_cost=int(j > 0)) for j, t in enumerate(([1, 2], [1, 3], [2, 3]))] for s in sorts[:2]]
            h, gh, qx = g.keyword_search_grouped_candidates_batch(users, [(3, S.GROUP, int(first_pass), 0, 0)] * len(users), k_stride=750, g_stride=250)[:3]
            assert (h.status == 0).all()
            for u, cs in enumerate(users):
                ref, _ = w.orc.search_candidates_grouped([H.oracle_query(w.orc, w.twin(q)) for q in cs], w.distinct, 3, first_pass, has_value=w.has_value, ids_cap=1 << 20)
                check_query(h, gh, u, ref, first_pass, 3, "grouped candidates u%d" % u)
        want = {"no row", "deleted row", "above the threshold", "equal the threshold", "below the threshold", "negative distance", "DESC",
                "topster smaller than the match count", "excluded ids", "filter ids", "two vector slots on different fields", "a vector slot with an _eval slot"}
        assert want <= w.seen, want - w.seen
    finally:
        for h in list(k.values()):
            w.drop(h)
        w.drop(ev)
    assert g.counter("sort_keys_live") == 0


# ------------------------------------------------------------------------------------------------ 5. refusals and lifetime
def run_refusals(w):
    g, n = w.g, w.n_docs
    rng = np.random.default_rng(4)
    dim = w.fields[F_ID].dim
    vk = w.vkey(F_ID, rng.standard_normal(dim).astype(np.float32))
    ek = w.key([np.arange(0, n, 3)], [5])
    try:
        assert g.counter("sort_keys_live") == 2
        qs = [T.KwQuery([1], sort=((VQ, 1, 4000), TM)),            # a handle that is not live -> 400
              T.KwQuery([1], sort=((VQ, 1, ek), TM)),              # kind 9 naming an _eval key -> 400
              T.KwQuery([1], sort=((B.SORT_EVAL, 1, vk), TM)),     # kind 4 naming a vector key -> 400
              T.KwQuery([1], sort=((VQ, 1, vk), TM)),
              T.KwQuery([1], sort=((8, 1, 0), TM)),                # 8 is no kind -> 501
              T.KwQuery([1], sort=((10, 1, 0), TM)),               # nor is anything beyond 9
              T.KwQuery([1], sort=((VQ, 1, vk), (VQ, -1, vk), (VQ, 1, vk)))]
        want = [B.ERR_INVALID, B.ERR_INVALID, B.ERR_INVALID, 0, B.ERR_UNSUPPORTED, B.ERR_UNSUPPORTED, 0]
        for hits in (g.keyword_search_batch(qs, k_stride=250), g.wildcard_search_batch([T.KwQuery([], sort=q.sort) for q in qs], k_stride=250)):
            assert list(hits.status) == want
            assert [int(x) > 0 for x in hits.n_hits] == [s == 0 for s in want]
        h, gh = g.keyword_search_grouped_batch(qs, [(2, S.GROUP, 1, 0, 0)] * len(qs), k_stride=500, g_stride=250)
        assert list(h.status) == want
        # creation errors
        for args, code in (((999, np.zeros(dim, np.float32)), B.ERR_NOT_FOUND),):
            try:
                g.sort_key_create_vector_query(*args)
                raise AssertionError("created a key on an unknown field")
            except B.TsgpuError as e:
                assert e.code == code
        import ctypes as C
        out = C.c_uint16(0)
        assert g.L.tsgpu_sort_key_create_vector_query(g.h, F_ID, None, C.c_float(1.0), C.byref(out)) == B.ERR_INVALID
        assert g.L.tsgpu_sort_key_create_vector_query(g.h, F_ID, np.zeros(dim, np.float32).ctypes.data, C.c_float(1.0), None) == B.ERR_INVALID
        # the vector, hybrid and group-member entry points refuse the kind
        X = rng.standard_normal((8, dim)).astype(np.float32)
        for call in (lambda: g.vector_search_batch(F_ID, X[:2], k=5, sort=((VQ, -1, vk), (B.SORT_VECTOR_DISTANCE, -1, 0))),
                     lambda: g.vector_search_batch(F_ID, X[:2], k=5, sort=((VQ, -1, vk),), filter_ids=np.arange(10), flat_search_cutoff=100)):
            hv = call()
            hv = hv[0] if isinstance(hv, tuple) else hv
            assert list(hv.status) == [B.ERR_UNSUPPORTED] * 2 and (hv.n_hits == 0).all()
        hh = g.hybrid_search_batch([T.KwQuery([1], sort=((VQ, -1, vk), TM)), T.KwQuery([1], sort=(TM, (B.SORT_SEQ_ID, 1, 0)))], F_ID, X[:2], k=5)
        hh = hh[0] if isinstance(hh, tuple) else hh
        assert hh.status[0] == B.ERR_UNSUPPORTED and hh.n_hits[0] == 0 and hh.status[1] == 0 and hh.n_hits[1] > 0
        grp = T.GpuGroup([w.g], transport=B.XCHG_COPY)
        try:
            hits = grp.keyword_search_batch([qs[3], T.KwQuery([1], sort=(TM,))], 10)
            hits = hits[0] if isinstance(hits, tuple) else hits
            assert list(hits.status) == [B.ERR_UNSUPPORTED, 0]
        finally:
            grp.close()
        # destroy, then 400; the freed slot serves a key of the OTHER form, and the other way round
        w.drop(vk)
        assert g.keyword_search_batch(qs[3:4], k_stride=250).status[0] == B.ERR_INVALID
        e2 = w.key([np.arange(2, n, 5), np.arange(0, n, 2)], [-4, 12])
        assert e2 == vk
        w.check_keyword([T.KwQuery([1, 2], sort=((B.SORT_EVAL, 1, e2), TM), topster_size=250)], "slot reused by an _eval key")
        assert g.keyword_search_batch([T.KwQuery([1], sort=((VQ, 1, e2), TM))], k_stride=250).status[0] == B.ERR_INVALID
        w.drop(e2)
        v2 = w.vkey(F_SHUF, rng.standard_normal(w.fields[F_SHUF].dim).astype(np.float32), 0.25)
        assert v2 == vk
        w.check_keyword([T.KwQuery([1, 2], sort=((VQ, -1, v2), TM), topster_size=250)], "slot reused by a vector key")
        w.drop(v2)
    finally:
        for h in list(w.vkeys) + list(w.keys):
            w.drop(h)
    assert g.counter("sort_keys_live") == 0


def run_field_mutations_under_a_live_key(w, fid=30, dim=20):
    """a key names its field: an upsert that grows the field past its capacity (the row matrix moves), an update of a live row and a delete are each followed
    by a search whose expected values are recomputed from the field's new content"""
    n = w.n_docs
    rng = np.random.default_rng(12)
    w.add_field(fid, dim, B.METRIC_IP, np.arange(0, 600, dtype=np.uint64) * 2, mixed_rows(600, dim, seed=5))      # even seq_ids below 1200: a label map from the start
    h = w.vkey(fid, rng.standard_normal(dim).astype(np.float32) * np.float32(2), 0.0)
    try:
        q = [T.KwQuery([1], sort=((VQ, -1, h), TM), topster_size=250), T.KwQuery([2, 1], sort=(TM, (VQ, 1, h), (B.SORT_SEQ_ID, 1, 0)), topster_size=40)]
        top = w.check_keyword(q, "before the mutations").keys[0, :3].astype(np.int64)
        more = np.setdiff1d(np.arange(n), np.arange(0, 1200, 2))
        w.upsert(fid, more[: n // 2], mixed_rows(n // 2, dim, seed=6))                           # far past the capacity the field was created with
        w.check_keyword(q, "after the field grew")
        target = int(w.check_keyword(q, "again").keys[0, 0])
        w.upsert(fid, [target], -w.fields[fid].X[w.fields[fid].row_of[target]][None, :] * np.float32(3))   # the best hit's row flips: it must sink
        after = w.check_keyword(q, "after the update of a live row")
        assert int(after.keys[0, 0]) != target
        target = int(after.keys[0, 0])
        w.delete(fid, target)
        w.seen.clear()
        rowless = [int(d) for d in w.orc.dump_posting(0, 1)[0] if int(d) not in w.fields[fid].row_of][-1]       # a match of token 1 the field never held
        after = w.check_keyword(q + [T.KwQuery([1], sort=((VQ, -1, h), TM), topster_size=250, filter_ids=np.sort(np.array([target, rowless])))], "after the delete")
        assert int(after.keys[0, 0]) != target and top.size == 3 and int(after.n_hits[2]) == 2
        assert {"deleted row", "no row"} <= w.seen, w.seen
    finally:
        w.drop(h)
    assert w.g.counter("sort_keys_live") == 0


def run_threads_with_keys_of_their_own(w, n_threads=8, per=6):
    """1-query calls from several threads coalesce into rounds that mix keys; each result equals the same call made alone"""
    g = w.g
    rng = np.random.default_rng(8)
    fids = (F_ID, F_OFF, F_SHUF)
    hs = [w.vkey(fids[t % 3], rng.standard_normal(w.fields[fids[t % 3]].dim).astype(np.float32), None if t % 2 else 1.0) for t in range(n_threads)]
    try:
        plans = [T.KwQuery([[1], [2, 1], [3, 1, 2], [4]][t % 4], sort=((VQ, -1 if t % 2 else 1, hs[t]), TM) if t % 4 != 3 else (TM, (B.SORT_INT64_COLUMN, 1, S.PTS)),
                           topster_size=250) for t in range(n_threads)]
        alone = [w.check_keyword([q], "alone") for q in plans]
        rounds0 = g.counter("batch_rounds")
        errors, start = [], threading.Barrier(n_threads)

        def run(t):
            try:
                start.wait()
                for _ in range(per):
                    hits = g.keyword_search_batch([plans[t]], k_stride=250)
                    a = alone[t]
                    nh = int(a.n_hits[0])
                    assert hits.status[0] == 0 and int(hits.n_hits[0]) == nh and int(hits.num_matched[0]) == int(a.num_matched[0])
                    assert np.array_equal(hits.keys[0, :nh], a.keys[0, :nh]) and np.array_equal(hits.scores[0, :nh], a.scores[0, :nh])
                    assert np.array_equal(hits.text_match[0, :nh], a.text_match[0, :nh])
            except BaseException as e:      # noqa: BLE001 (reported by the asserting thread)
                errors.append((t, e))
        ths = [threading.Thread(target=run, args=(t,)) for t in range(n_threads)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors[:3]
        assert g.counter("batch_rounds") > rounds0
    finally:
        for h in hs:
            w.drop(h)
    assert g.counter("sort_keys_live") == 0
