"""`-m gpu` twin of tests/test_emu_sortkeys.py: `_eval`, missing_values: first and string-rank sort keys through libtsgpu.so on a real MI355X, bit-exact
against the oracle (bodies: tests/sortkeys_common.py), plus a 2M-document case with a dense and a sparse key and 256 threads of 1-query calls whose
coalesced rounds mix queries with different keys and without one."""
import json
import os
import threading

import numpy as np
import pytest

import typesense_amd as T
from typesense_amd import _lib as B
from tests import helpers as H
from tests import sortkeys_common as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = S.World(30_000, H.gpu_lib_path())
    yield w
    w.close()


@pytest.mark.parametrize("dense_div", [0, 1, 64])
def test_every_path_both_forms(world, dense_div):
    S.run_matrix(world, dense_div)


def test_refusals_and_lifetime(world):
    S.run_refusals_and_lifetime(world)


def test_group_members_refuse_the_new_kinds(world):
    S.run_group_members_refuse(world, H.gpu_lib_path())


def test_handle_exhaustion(world):
    S.run_exhaustion(world)


def test_key_churn_on_another_thread_while_searching(world):
    S.run_churn_while_searching(world, rounds=200)


def test_reference_expectations():
    with open(os.path.join(H.ROOT, "tests", "golden", "sort_eval_cases.json")) as f:
        S.run_golden(H.gpu_lib_path(), json.load(f)["cases"])


def test_two_million_documents_dense_and_sparse_key():
    from tests.test_gpu_keyword import Corpus
    c = Corpus(2_000_000, 50_000, 24, seed=7)
    try:
        n = c.n_docs
        rng = np.random.default_rng(21)
        big = np.flatnonzero(rng.random(n) < 0.5).astype(np.uint32)                   # about half the documents: dense under the default threshold
        small = np.sort(rng.choice(n, size=1000, replace=False)).astype(np.uint32)    # 1 000 ids: sparse
        keys = {"dense": ([big, small], [7, -3]), "sparse": ([small], [11])}
        TM = (B.SORT_TEXT_MATCH, 1, 0)
        orc = c.orc
        for name, (lists, scores) in keys.items():
            h = c.g.sort_key_create_eval(lists, scores)
            try:
                v = S.eval_key(n, lists, scores)
                for sort in (((B.SORT_EVAL, 1, h), TM, (B.SORT_INT64_COLUMN, 1, 0)), ((TM, (B.SORT_EVAL, -1, h), (B.SORT_SEQ_ID, 1, 0)))):
                    qs = [T.KwQuery(t, sort=sort, topster_size=250) for t in ([3], [2, 9], [5, 1, 14], [40, 7], [1, 2, 3, 4])]
                    hits = c.g.keyword_search_batch(qs, k_stride=250)
                    assert (hits.status == 0).all()
                    # the oracle of this corpus has one column: the stand-in key takes its place, the points slot (if any) is re-read from a second oracle query
                    for i, q in enumerate(qs):
                        c.need(q.tokens)
                        orc2 = _oracle_with_key(c, v)
                        tsort = tuple((B.SORT_INT64_COLUMN, s[1], 1) if s[0] == B.SORT_EVAL else s for s in sort)
                        ref = H.oracle_keyword(orc2, T.KwQuery(q.tokens, sort=tsort, topster_size=250))
                        H.assert_hits_equal(hits, i, ref, "2M %s" % name)
            finally:
                c.g.sort_key_destroy(h)
        assert c.g.counter("sort_keys_live") == 0
    finally:
        c.g.close()
        if _ORC2.get("o") is not None:
            _ORC2["o"].close()
        _ORC2.clear()


_ORC2 = {}


def _oracle_with_key(c, v):
    """a two-column oracle over the same postings (loaded on demand): column 0 = points, column 1 = the restated key"""
    from oracle import oracle_py as O
    from typesense_amd import synth
    o = _ORC2.get("o")
    if o is None:
        o = _ORC2["o"] = O.OracleIndex(1, 2)
        o.set_num_docs(c.n_docs)
        o.set_sort_dense(0, c.pts)
        _ORC2["loaded"] = set()
    for t in sorted(c.loaded - _ORC2["loaded"]):
        ids, oi, off = synth.csr_term(c.csr, t)
        if ids.size:
            o.load_posting(0, t, ids, oi, off)
        _ORC2["loaded"].add(t)
    if _ORC2.get("key_id") != id(v):
        o.set_sort_dense(1, v)
        _ORC2["key_id"] = id(v)
    return o


def test_256_threads_of_one_query_calls_each_get_their_own_result(world):
    """coalesced rounds mix queries with different keys and without a key: every caller must get exactly its own result"""
    w, g = world, world.g
    rng = np.random.default_rng(8)
    n = w.n_docs
    TM = (B.SORT_TEXT_MATCH, 1, 0)
    handles = [w.key([np.sort(rng.choice(n, size=int(m), replace=False))], [int(s)]) for m, s in ((n // 2, 5), (n // 3, -7), (40, 9), (n // 50, 3))]
    try:
        n_threads, per = 256, 6
        plans = []
        for t in range(n_threads):
            h = handles[t % 5] if t % 5 < 4 else None
            sort = ((B.SORT_EVAL, 1 if t % 2 else -1, h), TM) if h is not None else (TM, (B.SORT_INT64_COLUMN, 1, S.PTS))
            toks = [[1], [2, 1], [3, 1, 2], [4]][t % 4]
            plans.append(T.KwQuery(toks, sort=sort, topster_size=250))
        refs = [H.oracle_keyword(w.orc, w.twin(q)) for q in plans]
        rounds0 = g.counter("batch_rounds")
        errors, start = [], threading.Barrier(n_threads)

        def run(t):
            try:
                start.wait()
                for _ in range(per):
                    hits = g.keyword_search_batch([plans[t]], k_stride=250)
                    assert hits.status[0] == 0
                    H.assert_hits_equal(hits, 0, refs[t], "thread %d" % t)
            except BaseException as e:      # noqa: BLE001
                errors.append((t, e))
        ths = [threading.Thread(target=run, args=(t,)) for t in range(n_threads)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors[:3]
        assert g.counter("batch_rounds") > rounds0          # (the calls really went through the micro-batcher)
    finally:
        for h in handles:
            w.drop(h)
    assert g.counter("sort_keys_live") == 0
