"""Shared bodies of tests/test_emu_sortkeys.py (CPU tier, SIMT emulator) and tests/test_gpu_sortkeys.py (-m gpu, libtsgpu.so): the sort kinds
TSGPU_SORT_EVAL / _INT64_COLUMN_MISSING_FIRST / _STRING_RANK / _STRING_RANK_FLIP against the oracle.

The oracle knows text_match / seq_id / int64 column. The expected result of a new slot is therefore the oracle's result for an ORDINARY int64 column
slot over a per-document key restated here in numpy — what Index::compute_sort_scores (reference src/index.cpp:5703-5904) leaves in scores[i] BEFORE the
ASC negation of :5901-5903:
  _eval           :5813-5834  the score of the first expression whose id list holds the document, else 0
  missing first   :5892-5898  INT64_MIN -> INT64_MIN + 1 (asc) / INT64_MAX (desc)
  string rank     :5735       adi_tree_t::rank(seq_id), NOT_FOUND = INT64_MAX; :5750-5760 negated when (asc, first) or (desc, last)
tests/golden/sort_eval_cases.json pins these restatements to the reference's own expectations (test/collection_sorting_test.cpp)."""
import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O
from tests import helpers as H

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
PTS, MISS, RANK, GROUP, SCRATCH = 0, 1, 2, 3, 4          # columns; SCRATCH .. SCRATCH + 2: the oracle's stand-in columns (one per sort slot)


def eval_key(n_docs, id_lists, scores):
    """:5813-5834 per document"""
    v = np.zeros(n_docs, np.int64)
    for ids, s in reversed(list(zip(id_lists, scores))):          # the FIRST matching expression wins
        ids = np.asarray(ids, np.int64)
        v[ids[ids < n_docs]] = s
    return v


def missing_first_key(col, order):
    """:5892-5898"""
    v = np.array(col, np.int64)
    v[v == I64_MIN] = I64_MIN + 1 if order == -1 else I64_MAX
    return v


def rank_key(col, flip):
    """:5735 + :5750-5760"""
    v = np.array(col, np.int64)
    if flip:
        v[v == I64_MAX] = -I64_MAX
    return v


class World:
    """n_docs documents: field 0 and field 1 plain strings, field 2 a string[]; columns PTS (points), MISS (missing rows + a real INT64_MIN), RANK (string
    ranks with NOT_FOUND rows), GROUP (distinct keys). The same content in the oracle and in a GpuIndex on `lib_path`."""

    def __init__(self, n_docs, lib_path, arrays=True):
        self.n_docs = n_docs
        rng = np.random.default_rng(5)
        f0 = H.zipf_docs(n_docs, 300, 12, seed=1)
        f1 = H.zipf_docs(n_docs, 300, 6, seed=2)
        self.orc = orc = O.OracleIndex(3, SCRATCH + 3)
        for d in range(n_docs):
            orc.index_plain(d, 0, f0[d])
            orc.index_plain(d, 1, f1[d])
            if arrays and d % 3 != 0:
                orc.index_array(d, 2, [list(f1[d][:2]), list(f0[d][:3]), [int(f0[d][5])]])
        orc.set_num_docs(n_docs)
        self.pts = H.points_of(n_docs)
        miss = rng.integers(-50, 50, n_docs).astype(np.int64)
        self.present = rng.random(n_docs) > 0.2
        miss[~self.present] = I64_MIN                              # no value (default_score, :5700)
        miss[rng.choice(n_docs, 7, replace=False)] = I64_MIN       # ... and documents that really hold INT64_MIN
        self.miss = miss
        rank = rng.permutation(n_docs).astype(np.int64) // 4       # ranks tie now and then
        rank[rng.random(n_docs) < 0.25] = I64_MAX                  # adi_tree_t::NOT_FOUND
        self.rank = rank
        from tests.test_emu_groupby import group_column
        self.distinct, self.has_value = group_column(n_docs, seed=3)
        orc.set_sort_dense(PTS, self.pts)
        self.g = g = T.GpuIndex(0, lib_path)
        for f in (0, 1, 2):
            g.field_create(f, f == 2)
            for term in orc.terms(f):
                ids, oi, off = orc.dump_posting(f, int(term))
                g.term_upsert(f, int(term), ids, oi, off)
        g.column_set(PTS, self.pts)
        g.column_set(MISS, np.where(miss == I64_MIN, 0, miss), present=(miss != I64_MIN))      # (a real INT64_MIN and a missing row are the same thing to the reference)
        g.column_set(RANK, rank)
        g.column_set(GROUP, self.distinct.view(np.int64))
        g.set_num_docs(n_docs)
        g.commit()
        self.keys = {}                                             # handle -> (id_lists, scores)

    def close(self):
        self.g.close()
        self.orc.close()

    def key(self, id_lists, scores):
        h = self.g.sort_key_create_eval(id_lists, scores)
        self.keys[h] = ([np.asarray(a, np.uint32) for a in id_lists], list(scores))
        return h

    def drop(self, h):
        self.g.sort_key_destroy(h)
        del self.keys[h]

    def twin(self, q):
        """the same query with every new-kind slot replaced by an int64-column slot over its restated key, loaded into the oracle's stand-in column"""
        sort = []
        for i, (kind, order, col) in enumerate(q.sort):
            if kind < B.SORT_EVAL:
                sort.append((kind, order, col))
                continue
            if kind == B.SORT_EVAL:
                v = eval_key(self.n_docs, *self.keys[col])
            elif kind == B.SORT_INT64_COLUMN_MISSING_FIRST:
                v = missing_first_key({MISS: self.miss, PTS: self.pts}[col], order)
            else:
                v = rank_key(self.rank, kind == B.SORT_STRING_RANK_FLIP)
            self.orc.set_sort_dense(SCRATCH + i, v)
            sort.append((B.SORT_INT64_COLUMN, order, SCRATCH + i))
        t = T.KwQuery(q.tokens, sort=tuple(sort), topster_size=q.topster_size, fields=q.fields, match_type=q.match_type, excluded_ids=q.excluded_ids,
                      filter_ids=q.filter_ids, dropped_tokens=q.dropped_tokens, total_cost=q.total_cost)
        return t

    def check_keyword(self, qs, what, k_stride=250):
        hits = self.g.keyword_search_batch(qs, k_stride=k_stride)
        assert (hits.status == 0).all(), (what, hits.status)
        for i, q in enumerate(qs):
            H.assert_hits_equal(hits, i, H.oracle_keyword(self.orc, self.twin(q)), what)
        return hits

    def check_wildcard(self, qs, what, k_stride=250):
        hits = self.g.wildcard_search_batch(qs, k_stride=k_stride)
        assert (hits.status == 0).all(), (what, hits.status)
        for i, q in enumerate(qs):
            H.assert_hits_equal(hits, i, H.oracle_wildcard(self.orc, self.twin(q)), what)
        return hits


def standard_keys(w):
    """1, 3 and 8 expressions; overlapping lists; an empty list; a list covering every document; negative scores"""
    n = w.n_docs
    rng = np.random.default_rng(11)
    pick = lambda m: np.sort(rng.choice(n, size=m, replace=False))
    every = np.arange(n)
    return {
        "one": w.key([pick(n // 3)], [7]),
        "three_overlap": w.key([pick(n // 5), pick(n // 2), pick(n // 2)], [10000, -9999, 9998]),
        "eight": w.key([pick(max(1, n // (10 + e))) for e in range(8)], [5, -3, 11, 2, -8, 1, 9, 4]),
        "empty_first": w.key([np.zeros(0, np.uint32), pick(n // 4)], [99, -5]),
        "only_empty": w.key([np.zeros(0, np.uint32)], [42]),
        "every_doc": w.key([pick(n // 7), every, pick(n // 2)], [-2, 3, 8]),
        "tiny": w.key([np.array([0, 3, n - 1])], [1]),
    }


def eval_sorts(h):
    """the slot in position 0, 1 and 2; ASC and DESC"""
    E = B.SORT_EVAL
    return [((E, 1, h), (B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, PTS)),
            ((E, -1, h), (B.SORT_TEXT_MATCH, 1, 0)),
            ((B.SORT_TEXT_MATCH, 1, 0), (E, 1, h), (B.SORT_SEQ_ID, -1, 0)),
            ((B.SORT_INT64_COLUMN, -1, PTS), (B.SORT_TEXT_MATCH, 1, 0), (E, -1, h)),
            ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, PTS), (E, 1, h))]


def column_sorts():
    """kind 5 on the column with missing rows and a real INT64_MIN; kinds 6 / 7 in the four (order, missing_values) combinations:
    (asc, first) and (desc, last) flip, (asc, last) and (desc, first) do not (:5750-5760)"""
    TM = (B.SORT_TEXT_MATCH, 1, 0)
    return [((B.SORT_INT64_COLUMN_MISSING_FIRST, 1, MISS), TM), ((B.SORT_INT64_COLUMN_MISSING_FIRST, -1, MISS), TM),
            (TM, (B.SORT_INT64_COLUMN_MISSING_FIRST, -1, MISS), (B.SORT_SEQ_ID, 1, 0)),
            ((B.SORT_STRING_RANK_FLIP, -1, RANK), TM), ((B.SORT_STRING_RANK, -1, RANK), TM),
            ((B.SORT_STRING_RANK, 1, RANK), TM), ((B.SORT_STRING_RANK_FLIP, 1, RANK), TM),
            (TM, (B.SORT_STRING_RANK_FLIP, 1, RANK), (B.SORT_INT64_COLUMN_MISSING_FIRST, 1, MISS))]


def run_matrix(w, dense_div, topster_sizes=(5, 250)):
    """every ranking path x the new kinds, with the keys built in the form `dense_div` forces (0 = sparse, 1 = dense)"""
    g = w.g
    g.set_option("sortkey_dense_div", dense_div)
    keys = standard_keys(w)
    try:
        n = w.n_docs
        filt = np.arange(0, n, 2)
        excl = np.arange(0, n, 7)
        f2 = ((0, 15), (1, 7))
        all_sorts = [s for h in keys.values() for s in eval_sorts(h)]
        col_sorts = column_sorts()
        for ts in topster_sizes:
            ks = max(ts, 8)
            # 1-, 2-, 3-token single field (find + score kernels), every key and slot position
            qs = [T.KwQuery(toks, sort=s, topster_size=ts) for s in all_sorts + col_sorts for toks in ([1], [2, 1], [3, 1, 2])][:: (1 if ts == 250 else 3)]
            w.check_keyword(qs, "single field ts=%d div=%d" % (ts, dense_div), k_stride=ks)
            sel = all_sorts[::4] + col_sorts[::2]
            # more than 3 tokens, two query_by fields, a string[] field, dropped tokens, filter_ids and excluded_ids
            qs = [T.KwQuery([1, 2, 3, 4], sort=s, topster_size=ts) for s in sel]
            qs += [T.KwQuery([1, 2], fields=f2, sort=s, topster_size=ts) for s in sel]
            qs += [T.KwQuery([2, 1], fields=((2, 15),), sort=s, topster_size=ts) for s in sel]
            qs += [T.KwQuery([1], fields=((2, 3), (0, 15)), sort=s, topster_size=ts) for s in sel[:3]]
            qs += [T.KwQuery([1, 2], sort=s, topster_size=ts, dropped_tokens=[3]) for s in sel]
            qs += [T.KwQuery([1, 2], sort=s, topster_size=ts, filter_ids=filt) for s in sel]
            qs += [T.KwQuery([1], sort=s, topster_size=ts, excluded_ids=excl) for s in sel]
            qs += [T.KwQuery([2, 1], fields=f2, sort=s, topster_size=ts, filter_ids=filt, excluded_ids=excl) for s in sel[:3]]
            w.check_keyword(qs, "general paths ts=%d div=%d" % (ts, dense_div), k_stride=ks)
            # the fused kernel
            g.set_option("kw_two_kernels", 0)
            try:
                w.check_keyword([T.KwQuery(toks, sort=s, topster_size=ts) for s in sel for toks in ([1], [3, 1, 2])], "fused ts=%d div=%d" % (ts, dense_div), k_stride=ks)
            finally:
                g.set_option("kw_two_kernels", 1)
            # the device-side planner (kw_plan.hip.h) carries the slots, too
            g.set_option("kw_device_plan_min_queries", 1)
            try:
                n0 = g.counter("kw_device_plans")
                w.check_keyword([T.KwQuery([2, 1], sort=s, topster_size=ts) for s in sel], "device plan ts=%d div=%d" % (ts, dense_div), k_stride=ks)
                assert g.counter("kw_device_plans") == n0 + 1
            finally:
                g.set_option("kw_device_plan_min_queries", 512)
            # wildcard
            qs = [T.KwQuery([], sort=s, topster_size=ts) for s in sel] + [T.KwQuery([], sort=s, topster_size=ts, filter_ids=filt, excluded_ids=excl) for s in sel]
            w.check_wildcard(qs, "wildcard ts=%d div=%d" % (ts, dense_div), k_stride=ks)
        # candidate folding
        groups = [[T.KwQuery(t, sort=s, topster_size=250) for t in ([1, 2], [1, 3], [2, 3], [1])] for s in all_sorts[::5] + col_sorts[::3]]
        hits, qidx, found = g.keyword_search_candidates_batch(groups, k_stride=250)
        assert (hits.status == 0).all()
        for gi, combos in enumerate(groups):
            ref, ref_qi = H.oracle_candidates(w.orc, [w.twin(c) for c in combos])
            H.assert_hits_equal(hits, gi, ref, "candidates g%d div=%d" % (gi, dense_div))
            assert np.array_equal(qidx[gi, :int(hits.n_hits[gi])], ref_qi)
        # both group_by passes
        from tests.test_emu_groupby import check_query, oracle_grouped
        for first_pass in (True, False):
            qs = [T.KwQuery(t, sort=s, topster_size=ts) for s in all_sorts[1::6] + col_sorts[1::3] for t, ts in (([1], 250), ([2, 1], 5))]
            grp = [(3, GROUP, int(first_pass), 0, 0)] * len(qs)
            h, gh = g.keyword_search_grouped_batch(qs, grp, k_stride=250 * 3, g_stride=250)
            for i, q in enumerate(qs):
                check_query(h, gh, i, oracle_grouped(w.orc, w.twin(q), w.distinct, w.has_value, 3, first_pass), first_pass, 3, "grouped div=%d" % dense_div)
    finally:
        for h in list(keys.values()):
            w.drop(h)
        g.set_option("sortkey_dense_div", 64)
    assert g.counter("sort_keys_live") == 0


def run_refusals_and_lifetime(w, with_vectors=True):
    g = w.g
    a = w.key([np.arange(0, w.n_docs, 3)], [5])
    b = w.key([np.arange(1, w.n_docs, 3)], [6])
    try:
        assert g.counter("sort_keys_live") == 2
        TM = (B.SORT_TEXT_MATCH, 1, 0)
        qs = [T.KwQuery([1], sort=((B.SORT_EVAL, 1, a), (B.SORT_EVAL, 1, b), TM)),          # two _eval slots: the reference's shared cursors (:5809-5811)
              T.KwQuery([1], sort=((B.SORT_EVAL, 1, 4000), TM)),                            # a handle that is not live
              T.KwQuery([1], sort=((B.SORT_EVAL, 1, a), TM)),
              T.KwQuery([1], sort=((8, 1, 0), TM)),                                         # no such kind
              T.KwQuery([1], sort=((B.SORT_STRING_RANK, 1, 900), TM))]                      # no such column
        for hits in (g.keyword_search_batch(qs, k_stride=250), g.wildcard_search_batch([T.KwQuery([], sort=q.sort) for q in qs], k_stride=250)):
            assert list(hits.status) == [B.ERR_UNSUPPORTED, B.ERR_INVALID, 0, B.ERR_UNSUPPORTED, B.ERR_UNSUPPORTED]
            assert hits.n_hits[0] == 0 and hits.n_hits[1] == 0 and hits.n_hits[2] > 0
        h, gh = g.keyword_search_grouped_batch(qs, [(2, GROUP, 1, 0, 0)] * len(qs), k_stride=500, g_stride=250)
        assert list(h.status) == [B.ERR_UNSUPPORTED, B.ERR_INVALID, 0, B.ERR_UNSUPPORTED, B.ERR_UNSUPPORTED]
        # destroy, then the handle is bad; create again: the slot is reused and serves the NEW lists
        w.drop(a)
        assert g.keyword_search_batch(qs[2:3], k_stride=250).status[0] == B.ERR_INVALID
        with_err = None
        try:
            g.sort_key_destroy(a)
        except B.TsgpuError as e:
            with_err = e.code
        assert with_err == B.ERR_NOT_FOUND
        a2 = w.key([np.arange(2, w.n_docs, 5), np.arange(0, w.n_docs, 2)], [-4, 12])
        assert a2 == a
        w.check_keyword([T.KwQuery([1, 2], sort=((B.SORT_EVAL, 1, a2), TM), topster_size=250)], "reused handle")
        if with_vectors:
            # the vector and hybrid entry points do not serve the new kinds (forward-only cursor over hits in distance order, :3675 / :4115)
            rng = np.random.default_rng(1)
            X = rng.standard_normal((64, 8)).astype(np.float32)
            g.vec_create(9, 8, B.METRIC_IP)
            g.vec_upsert(9, np.arange(64, dtype=np.uint64), X)
            for sort in (((B.SORT_EVAL, 1, a2), (B.SORT_VECTOR_DISTANCE, -1, 0)), ((B.SORT_VECTOR_DISTANCE, -1, 0), (B.SORT_STRING_RANK_FLIP, 1, RANK)),
                         ((B.SORT_INT64_COLUMN_MISSING_FIRST, 1, MISS),)):
                hv = g.vector_search_batch(9, X[:2], k=5, sort=sort)
                hv = hv[0] if isinstance(hv, tuple) else hv
                assert list(hv.status) == [B.ERR_UNSUPPORTED] * 2 and (hv.n_hits == 0).all()
                hv = g.vector_search_batch(9, X[:2], k=5, sort=sort, filter_ids=np.arange(10), flat_search_cutoff=100)      # the flat branch
                hv = hv[0] if isinstance(hv, tuple) else hv
                assert list(hv.status) == [B.ERR_UNSUPPORTED] * 2 and (hv.n_hits == 0).all()
                hh = g.hybrid_search_batch([T.KwQuery([1], sort=sort), T.KwQuery([1], sort=(TM, (B.SORT_SEQ_ID, 1, 0)))], 9, X[:2], k=5)
                hh = hh[0] if isinstance(hh, tuple) else hh
                assert hh.status[0] == B.ERR_UNSUPPORTED and hh.n_hits[0] == 0 and hh.status[1] == 0 and hh.n_hits[1] > 0
        w.drop(a2)
    finally:
        for h in list(w.keys):
            w.drop(h)
    assert g.counter("sort_keys_live") == 0


def run_group_members_refuse(w, lib_path):
    """the tsgpu_group_* shard forms refuse the new kinds: a context that serves a group answers 501 for them (a key is one context's)"""
    TM = (B.SORT_TEXT_MATCH, 1, 0)
    h = w.key([np.arange(0, w.n_docs, 2)], [3])
    grp = T.GpuGroup([w.g], transport=B.XCHG_COPY)
    try:
        qs = [T.KwQuery([1], sort=((B.SORT_EVAL, 1, h), TM)), T.KwQuery([1], sort=((B.SORT_STRING_RANK, 1, RANK), TM)), T.KwQuery([1], sort=(TM, (B.SORT_INT64_COLUMN, 1, PTS)))]
        hits = grp.keyword_search_batch(qs, 10)
        hits = hits[0] if isinstance(hits, tuple) else hits
        assert list(hits.status) == [B.ERR_UNSUPPORTED, B.ERR_UNSUPPORTED, 0] and hits.n_hits[0] == 0 and hits.n_hits[1] == 0 and hits.n_hits[2] > 0
        hg = grp.keyword_search_grouped_batch(qs, [(2, GROUP, 1, 0, 0)] * 3, k_stride=500, g_stride=250)
        assert list(hg[0].status) == [B.ERR_UNSUPPORTED, B.ERR_UNSUPPORTED, 0]
    finally:
        grp.close()
        w.drop(h)
    # out of the group again, the context serves them
    h = w.key([np.arange(0, w.n_docs, 2)], [3])
    try:
        w.check_keyword([T.KwQuery([1], sort=((B.SORT_EVAL, 1, h), TM), topster_size=250)], "after the group")
    finally:
        w.drop(h)


def run_exhaustion(w):
    g = w.g
    g.set_option("sortkey_dense_div", 0)
    made = []
    try:
        one = [np.array([1, 2, 3], np.uint32)]
        for _ in range(B.SORT_KEY_SLOTS):
            made.append(g.sort_key_create_eval(one, [1]))
        assert len(set(made)) == B.SORT_KEY_SLOTS and g.counter("sort_keys_live") == B.SORT_KEY_SLOTS
        code = None
        try:
            g.sort_key_create_eval(one, [1])
        except B.TsgpuError as e:
            code = e.code
        assert code == B.ERR_NO_MEMORY
        g.sort_key_destroy(made.pop())
        made.append(g.sort_key_create_eval(one, [1]))
    finally:
        for h in made:
            g.sort_key_destroy(h)
        g.set_option("sortkey_dense_div", 64)
    assert g.counter("sort_keys_live") == 0


def run_churn_while_searching(w, rounds=30):
    """one thread creates and destroys unrelated keys (both forms) while this one searches with its own key"""
    import threading
    g = w.g
    TM = (B.SORT_TEXT_MATCH, 1, 0)
    mine = w.key([np.arange(0, w.n_docs, 3), np.arange(0, w.n_docs, 2)], [9, -9])
    stop, errors = threading.Event(), []

    def churn():
        rng = np.random.default_rng(3)
        try:
            while not stop.is_set():
                ids = np.sort(rng.choice(w.n_docs, size=int(rng.integers(1, w.n_docs // 2)), replace=False))
                hs = [g.sort_key_create_eval([ids], [1]), g.sort_key_create_eval([ids[:5], ids], [2, 3])]
                for h in hs:
                    g.sort_key_destroy(h)
        except Exception as e:      # noqa: BLE001 (reported by the asserting thread)
            errors.append(e)
    t = threading.Thread(target=churn)
    t.start()
    try:
        q = T.KwQuery([1, 2], sort=((B.SORT_EVAL, 1, mine), TM), topster_size=250)
        ref = H.oracle_keyword(w.orc, w.twin(q))
        for _ in range(rounds):
            hits = g.keyword_search_batch([q], k_stride=250)
            assert hits.status[0] == 0
            H.assert_hits_equal(hits, 0, ref, "search under key churn")
    finally:
        stop.set()
        t.join()
        w.drop(mine)
    assert not errors, errors
    assert g.counter("sort_keys_live") == 0


def run_golden(lib_path, cases):
    """tests/golden/sort_eval_cases.json: the reference's own expected orders, through the HIP path AND through the column trick"""
    for case in cases:
        n = case["n_docs"]
        docs = np.full((n, 1), 1, np.uint32)                      # every document matches the token / q = *
        orc = O.OracleIndex(1, SCRATCH + 3)
        for d in range(n):
            orc.index_plain(d, 0, docs[d])
        orc.set_num_docs(n)
        g = T.GpuIndex(0, lib_path)
        try:
            g.field_create(0, False)
            ids, oi, off = orc.dump_posting(0, 1)
            g.term_upsert(0, 1, ids, oi, off)
            cols = {}
            for name, c in case.get("columns", {}).items():
                v = np.array([I64_MIN if x is None else x for x in c["values"]], np.int64)
                if c.get("string_ranks"):
                    v = np.array([I64_MAX if x is None else x for x in c["values"]], np.int64)
                cols[name] = (len(cols), v)
                g.column_set(cols[name][0], v)
                orc.set_sort_dense(cols[name][0], v)
            g.set_num_docs(n)
            g.commit()
            for div in (0, 1):
                g.set_option("sortkey_dense_div", div)
                for rq in case["requests"]:
                    sort, tsort, handles = [], [], []
                    for i, s in enumerate(rq["sort"]):
                        order = 1 if s["order"] == "desc" else -1
                        if s["type"] == "eval":
                            h = g.sort_key_create_eval([np.array(x, np.uint32) for x in s["ids"]], s["scores"])
                            handles.append(h)
                            sort.append((B.SORT_EVAL, order, h))
                            v = eval_key(n, s["ids"], s["scores"])
                        elif s["type"] == "text_match":
                            sort.append((B.SORT_TEXT_MATCH, order, 0)); tsort.append(sort[-1])
                            continue
                        else:
                            col, base = cols[s["column"]]
                            first = s.get("missing_values") == "first"
                            if s["type"] == "int64":
                                kind = B.SORT_INT64_COLUMN_MISSING_FIRST if first else B.SORT_INT64_COLUMN
                                v = missing_first_key(base, order) if first else base
                            else:
                                flip = (order == -1 and first) or (order == 1 and s.get("missing_values") == "last")
                                kind = B.SORT_STRING_RANK_FLIP if flip else B.SORT_STRING_RANK
                                v = rank_key(base, flip)
                            sort.append((kind, order, col))
                        orc.set_sort_dense(SCRATCH + i, v)
                        tsort.append((B.SORT_INT64_COLUMN, order, SCRATCH + i))
                    try:
                        for wildcard in (rq.get("wildcard", False),) if "wildcard" in rq else (False, True):
                            q = T.KwQuery([] if wildcard else [1], sort=tuple(sort), topster_size=250)
                            tq = T.KwQuery([] if wildcard else [1], sort=tuple(tsort), topster_size=250)
                            hits = (g.wildcard_search_batch if wildcard else g.keyword_search_batch)([q], k_stride=250)
                            ref = (H.oracle_wildcard if wildcard else H.oracle_keyword)(orc, tq)
                            assert hits.status[0] == 0
                            what = "%s: %s div=%d wildcard=%d" % (case["name"], rq["name"], div, wildcard)
                            assert [int(x) for x in ref.keys] == rq["expected_ids"], what + " (column trick vs the reference's order)"
                            assert [int(x) for x in hits.keys[0, :int(hits.n_hits[0])]] == rq["expected_ids"], what + " (HIP path vs the reference's order)"
                            H.assert_hits_equal(hits, 0, ref, what)
                    finally:
                        for h in handles:
                            g.sort_key_destroy(h)
            assert g.counter("sort_keys_live") == 0
        finally:
            g.close()
            orc.close()
