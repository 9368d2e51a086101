"""The keyword planner's PLAN, pinned (shared body of tests/test_emu_kw_plan_digest.py and tests/test_gpu_kw_plan_digest.py).

Any valid plan gives the same hits, so the result tests cannot see a change of the chunking, the launch order or the merge grouping. Under the
tests-only option kw_plan_digest a keyword batch leaves two digests of its plan (typesense_amd/csrc/kw_plan_digest.h: the CUT — handles, probe order,
work items, merge sources per query — and the LAYOUT — offsets, table sizes, merge groups, hit offsets), and tests/golden/kw_plan_digests.json holds
what the planner gave BEFORE it was restructured (tests/golden/make_kw_plan_digests.py). Every case also compares its hits with the oracle's.

One world: 20 000 documents, three plain string fields; field 0's longest lists reach 68 / 49 blocks, so that a query cut into 1-block items has more
than 16 of them (merge groups). Single-field queries read field 0. The 256-block cap of a work item needs a longer list: body_block_cap builds its own."""
import json
import os

import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from tests import helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kw_plan_digests.json")
N_DOCS = 20000
SORT = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
F3 = [(0, 15), (1, 7), (2, 3)]
BATCH_SIZES = (1, 100, 129, 511, 600, 2100)          # around the planner's rules for <= 128 and < 512 queries and the radix / comparison sort switch at 2 048
OPTION_DEFAULTS = (("kw_chunk_blocks", 0), ("kw_merge_select_min", 2), ("kw_sort_work", 1), ("plan_threads", 8), ("plan_parallel_min_queries", 2048),
                   ("kw_device_plan_min_queries", 512), ("kw_host_split_queries", 1000), ("kw_plan_digest", 0))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


class World:
    def __init__(self, lib_path):
        rng = np.random.default_rng(41)
        body = H.zipf_docs(N_DOCS, 300, 12, seed=21)
        title = H.zipf_docs(N_DOCS, 300, 4, seed=22)
        tags = H.zipf_docs(N_DOCS, 300, 3, seed=23)
        title[rng.random(title.shape) < 0.3] = 0
        tags[rng.random(tags.shape) < 0.6] = 0
        self.orc, self.g = H.build_pair_fields([body, title, tags], lib_path)
        self.g.set_option("kw_host_split_queries", 0)          # one batch = one plan
        # a second context that owns the seq_ids [6 000, 15 500) only: q = * plans over its range
        self.lo, self.hi = 6000, 15500
        self.g_range = T.GpuIndex(0, lib_path)
        self.g_range.column_set(0, H.points_of(N_DOCS))
        self.g_range.set_num_docs(N_DOCS)
        self.g_range.commit()
        self.g_range.set_option("doc_range_lo", self.lo)
        self.g_range.set_option("doc_range_hi", self.hi)
        self._ref = {}
        self.seen = {}               # case name -> digests (the fixture maker writes these out)

    def close(self):
        self.g.close()
        self.g_range.close()

    def oracle(self, q):
        """the oracle's answer, computed once per distinct query"""
        key = (tuple(q.tokens), tuple(q.fields), q.sort, q.topster_size, q.match_type, q.prioritize_token_position, q.total_cost, tuple(q.dropped_tokens),
               None if q.filter_ids is None else q.filter_ids.tobytes(), None if q.excluded_ids is None else q.excluded_ids.tobytes())
        if key not in self._ref:
            self._ref[key] = H.oracle_keyword(self.orc, q)
        return self._ref[key]

    def reset(self):
        for name, v in OPTION_DEFAULTS:
            self.g.set_option(name, v)
        self.g.set_option("kw_host_split_queries", 0)

    def run(self, qs, name, check=None, wildcard=False, g=None):
        """one batch under option kw_plan_digest -> (cut, layout) digests as hex strings; hits = the oracle's"""
        g = g or self.g
        g.set_option("kw_plan_digest", 1)
        try:
            hits = (g.wildcard_search_batch if wildcard else g.keyword_search_batch)(qs, k_stride=250)
            d = {"cut": "%016x" % g.counter("kw_last_plan_cut_digest"), "layout": "%016x" % g.counter("kw_last_plan_layout_digest")}
        finally:
            g.set_option("kw_plan_digest", 0)
        if check is not None:
            check(hits)
        elif not wildcard:
            for i, q in enumerate(qs):
                if hits.status[i] == 0:
                    H.assert_hits_equal(hits, i, self.oracle(q), name)
        self.seen[name] = d
        return d, hits


# ---------------------------------------------------------------- the batches
def mixed_batch():
    """the mixed batch of test_parallel_planning_of_a_batch_gives_the_serial_plan (tests/test_emu_keyword.py) on this world: plain, filter, excluded,
    dropped tokens, an invalid 12-token query, seq-id sort — and the three-field queries, every third one with filter ids"""
    rng = np.random.default_rng(321)
    qs = []
    for rep in range(40):
        toks = rng.choice(np.arange(1, 30), size=int(rng.integers(1, 5)), replace=False)
        kind = rep % 5
        if kind == 0: qs.append(T.KwQuery(toks, sort=SORT, topster_size=250))
        elif kind == 1: qs.append(T.KwQuery(toks, sort=SORT, topster_size=40, filter_ids=np.sort(rng.choice(N_DOCS, size=4000, replace=False))))
        elif kind == 2: qs.append(T.KwQuery(toks, sort=SORT, topster_size=250, excluded_ids=np.arange(int(rng.integers(0, 5)), N_DOCS, 5)))
        elif kind == 3: qs.append(T.KwQuery(toks[:2], sort=SORT, topster_size=250, dropped_tokens=[int(rng.integers(30, 60))]))
        else: qs.append(T.KwQuery(list(range(1, 13)), sort=SORT) if rep == 4 else T.KwQuery(toks, sort=((B.SORT_SEQ_ID, 1, 0),), topster_size=17))
    for rep in range(24):
        toks = rng.choice(np.arange(1, 20), size=int(rng.integers(1, 4)), replace=False)
        qs.append(T.KwQuery(toks, fields=F3, sort=SORT, topster_size=250, filter_ids=np.sort(rng.choice(N_DOCS, size=5000, replace=False)) if rep % 3 == 0 else None))
    return qs


def small_queries():
    """100 plain single-field queries of 1..5 tokens; the first ones drive the longest lists (68, 49 and 36 blocks), a few three-field ones among them"""
    rng = np.random.default_rng(55)
    qs = [T.KwQuery([1], sort=SORT, topster_size=250), T.KwQuery([2, 1], sort=SORT, topster_size=250), T.KwQuery([1, 3, 2], sort=SORT, topster_size=40),
          T.KwQuery([2], sort=SORT, topster_size=7), T.KwQuery([3, 1], fields=F3, sort=SORT, topster_size=250), T.KwQuery([1, 2, 3, 4], sort=SORT, topster_size=250)]
    while len(qs) < 100:
        n_tok = int(rng.choice([1, 2, 2, 3, 3, 3, 4, 5]))
        toks = rng.choice(np.arange(1, 120), size=n_tok, replace=False)
        if len(qs) % 16 == 7: qs.append(T.KwQuery(toks[:3], fields=F3, sort=SORT, topster_size=40))
        else: qs.append(T.KwQuery(toks, sort=SORT, topster_size=[250, 40, 7][len(qs) % 3]))
    return qs


def batch_of(n):
    """the first n of: the first 40 small queries (the six long ones among them), then queries of one token that the index does not hold. Those get no
    work item but count in every rule that looks at the batch's size, and the emulator spends 4 ms on one (25 ms on the shortest real query, half a
    second on a long one): the whole grid stays affordable in the tier that runs without hardware"""
    base = small_queries()[:40]
    return [base[i] if i < len(base) else T.KwQuery([200000 + i], sort=SORT, topster_size=[250, 40, 7][i % 3]) for i in range(n)]


def plain_batch(n):
    """the batch of test_device_side_planner_equals_the_host_planner_and_the_oracle on this world (plain single-field queries: both planners take it),
    repeated up to n queries"""
    rng = np.random.default_rng(77)
    sorts = [SORT, ((B.SORT_INT64_COLUMN, -1, 0), (B.SORT_TEXT_MATCH, 1, 0), (B.SORT_SEQ_ID, -1, 0)), ((B.SORT_SEQ_ID, 1, 0),)]
    qs = []
    for rep in range(90):
        n_tok = int(rng.choice([1, 2, 3, 3, 3, 4, 5, 7]))
        toks = list(rng.choice(np.arange(1, 60), size=n_tok, replace=False))
        if rep % 11 == 0: toks[0] = 100000 + rep            # a token the index does not hold
        if rep % 13 == 0 and n_tok >= 2: toks[1] = toks[0]  # a duplicated token
        if rep % 17 == 0: toks = [3000000 + rep]            # no token of the query exists
        qs.append(T.KwQuery(toks, sort=sorts[rep % 3], topster_size=[250, 40, 7][rep % 3], match_type=rep % 3, prioritize_token_position=bool(rep & 1), total_cost=rep % 4))
    return [qs[i % 90] for i in range(n)]


def option_grid(n):
    """(kw_chunk_blocks, kw_merge_select_min, kw_sort_work) per batch size, the same in both tiers: the automatic chunk (the only one the batch-size rules
    act on) with both merges and both orders at every size; up to 129 queries every fixed chunk 1 / 2 / 64 with either merge, beyond that chunk 1 and 64.
    Measured on the emulator: 3 to 5 s per run up to 129 queries, 6 to 14 s beyond (the 2 100-query batch: 80 s for its six runs)"""
    grid = [(0, m, s) for m in (2, 0) for s in (1, 0)]
    if n <= 129:
        grid += [(c, m, s) for c in (1, 2, 64) for m, s in ((2, 1), (0, 0))]
    else:
        grid += [(1, 0, 1), (64, 2, 0)]
    return grid


def case_name(kind, *parts):
    return kind + "".join("/%s" % p for p in parts)


# ---------------------------------------------------------------- the test bodies
def body_mixed_batch(w):
    """serial and on five parked threads: the same plan, and the plan the golden holds"""
    gold = golden()
    qs = mixed_batch()
    w.reset()
    try:
        serial, hs = w.run(qs, case_name("mixed", "serial"))
        assert (hs.status == 0).sum() == len(qs) - 1 and hs.status[4] == B.ERR_UNSUPPORTED
        w.g.set_option("plan_parallel_min_queries", 1)
        w.g.set_option("plan_threads", 5)
        par, hp = w.run(qs, case_name("mixed", "parallel"))
        assert np.array_equal(hp.status, hs.status)
        assert par == serial, "the sliced plan differs from the serial one"
        assert serial == gold[case_name("mixed", "serial")] and par == gold[case_name("mixed", "parallel")]
    finally:
        w.reset()


def body_option_grid(w, n):
    gold = golden()
    qs = batch_of(n)
    w.reset()
    w.g.set_option("kw_device_plan_min_queries", 0)         # the host planner (three-field queries send the batch there anyway)
    try:
        for chunk, msel, sort_work in option_grid(n):
            w.g.set_option("kw_chunk_blocks", chunk)
            w.g.set_option("kw_merge_select_min", msel)
            w.g.set_option("kw_sort_work", sort_work)
            name = case_name("grid", n, "chunk%d" % chunk, "msel%d" % msel, "sort%d" % sort_work)
            d, hits = w.run(qs, name)
            assert (hits.status == 0).all()
            assert d == gold[name], name
    finally:
        w.reset()


def body_wildcard(w):
    """q = * with and without filter ids, on the whole collection and on the context that owns [lo, hi)"""
    gold = golden()
    rng = np.random.default_rng(9)
    filt = np.sort(rng.choice(N_DOCS, size=7000, replace=False)).astype(np.uint32)
    excl = np.sort(rng.choice(N_DOCS, size=300, replace=False)).astype(np.uint32)
    sort = ((B.SORT_INT64_COLUMN, 1, 0), (B.SORT_SEQ_ID, -1, 0))
    qs = [T.KwQuery([], sort=sort, topster_size=250), T.KwQuery([], sort=sort, topster_size=30, filter_ids=filt, excluded_ids=excl),
          T.KwQuery([], sort=((B.SORT_SEQ_ID, 1, 0),), topster_size=2), T.KwQuery([], sort=sort, topster_size=40, filter_ids=filt[:100])]
    w.reset()

    def check_with(own):
        def check(hits):
            assert (hits.status == 0).all()
            for i, q in enumerate(qs):
                base = np.arange(N_DOCS, dtype=np.uint32) if q.filter_ids is None else q.filter_ids
                if own:
                    base = base[(base >= w.lo) & (base < w.hi)]
                if base.size == 0:                         # nothing of this query on this shard (to the oracle an empty filter is no filter)
                    assert hits.n_hits[i] == 0
                    continue
                ref = H.oracle_wildcard(w.orc, T.KwQuery([], sort=q.sort, topster_size=q.topster_size, filter_ids=base, excluded_ids=q.excluded_ids))
                n = int(hits.n_hits[i])
                assert n == ref.keys.size and np.array_equal(hits.keys[i, :n], ref.keys) and np.array_equal(hits.scores[i, :n], ref.scores), i
        return check

    d, _ = w.run(qs, case_name("wildcard", "whole"), check=check_with(False), wildcard=True)
    assert d == gold[case_name("wildcard", "whole")]
    d, _ = w.run(qs, case_name("wildcard", "range"), check=check_with(True), wildcard=True, g=w.g_range)
    assert d == gold[case_name("wildcard", "range")]


def body_both_planners(w, layout_of_device_plan):
    """the 90-query batch through the host planner and the device planner, the 600-query batch through the device planner: the host plan and the device
    planner's cut (integer arithmetic) are the golden's in both tiers; the device planner's layout follows a float cost, which the GPU may contract
    into FMAs where the emulator build does not: compared in the emulator tier only (layout_of_device_plan)"""
    gold = golden()
    w.reset()
    try:
        qs = plain_batch(90)
        w.g.set_option("kw_device_plan_min_queries", 0)
        host, hh = w.run(qs, case_name("planners", 90, "host"))
        assert host == gold[case_name("planners", 90, "host")]
        for n in (90, 600):
            qs = plain_batch(n)
            w.g.set_option("kw_device_plan_min_queries", 8)
            n0, f0 = w.g.counter("kw_device_plans"), w.g.counter("kw_device_plan_fallbacks")
            name = case_name("planners", n, "device")
            dev, hd = w.run(qs, name)
            assert w.g.counter("kw_device_plans") == n0 + 1 and w.g.counter("kw_device_plan_fallbacks") == f0, "the batch was not planned on the device"
            assert (hd.status == 0).all()
            assert dev["cut"] == gold[name]["cut"], name
            if layout_of_device_plan:
                assert dev["layout"] == gold[name]["layout"], name
            if n == 90:
                assert np.array_equal(hd.n_hits, hh.n_hits) and np.array_equal(hd.num_matched, hh.num_matched)
                for i in range(n):
                    k = int(hh.n_hits[i])
                    assert np.array_equal(hd.keys[i, :k], hh.keys[i, :k]) and np.array_equal(hd.scores[i, :k], hh.scores[i, :k]), i
    finally:
        w.reset()


def body_block_cap(lib_path):
    """the 256-block cap of a work item: a list of more than 65 280 ids (one token in nearly every one of 72 000 documents) driven by one query of a batch
    of 512, with kw_max_partials = 1 (one item per query, unless the cap cuts it): 256 + 20 blocks. The other queries name tokens the index does not hold"""
    from typesense_amd import synth
    from oracle import oracle_py as O
    n_docs = 72000
    csr = synth.zipf_corpus_csr(n_docs, 50, 16, seed=5, device="cpu")
    pts = synth.points_column(n_docs)
    g = T.GpuIndex(0, lib_path)
    try:
        g.field_create(0, False)
        g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
        g.column_set(0, pts)
        g.set_num_docs(n_docs)
        g.commit()
        lens = np.diff(np.asarray(csr["ids_ptr"]).astype(np.int64))
        top = int(np.asarray(csr["term_ids"])[int(np.argmax(lens))])
        assert lens.max() > 255 * 256 + 255, "the driver list must be longer than 255 full blocks and a bit"
        qs = [T.KwQuery([top], sort=SORT, topster_size=40)] + [T.KwQuery([300000 + i], sort=SORT, topster_size=7) for i in range(511)]
        for name, v in (("kw_host_split_queries", 0), ("kw_device_plan_min_queries", 0), ("kw_max_partials", 1), ("kw_plan_digest", 1)):
            g.set_option(name, v)
        hits = g.keyword_search_batch(qs, k_stride=250)
        d = {"cut": "%016x" % g.counter("kw_last_plan_cut_digest"), "layout": "%016x" % g.counter("kw_last_plan_layout_digest")}
        orc = O.OracleIndex(1, 1)
        orc.set_num_docs(n_docs)
        orc.set_sort_dense(0, pts)
        orc.load_posting(0, top, *synth.csr_term(csr, top))
        assert (hits.status == 0).all() and hits.n_hits[1:].sum() == 0
        H.assert_hits_equal(hits, 0, H.oracle_keyword(orc, qs[0]), "block cap")
        assert d == golden()[case_name("cap", 512)]
        return {case_name("cap", 512): d}
    finally:
        g.close()
