"""Shared bodies of tests/test_emu_find_dir_tile.py (CPU tier, SIMT emulator) and tests/test_gpu_find_dir_tile.py (-m gpu, libtsgpu.so): the id
directory (typesense_amd/csrc/tsgpu_format.h) as the pair-find kernel reads it.

  split-free entries   index_iddir_build_kernel marks a directory entry IDDIR_SPLIT only where a block boundary falls inside its 32 ids AND the block in
                       front of the boundary is part-filled: behind a full block pos + popcount is exact across the boundary. A freshly packed index
                       has no marked entry (counter kw_iddir_split_entries); an incremental commit that leaves a part-filled block in mid-list has.
  directory tile       stage 1 of kw_find2_kernel in DIRECTORY MODE (option kw_find_dir_tile, default 1): a pair's tile holds the slice of the second
                       list's directory under the pair; a candidate is one LDS read. Same results as the window path (kw_find_dir_tile = 0), in the
                       byte-counting instantiation, from either planner, on freshly packed and on incrementally mutated lists.
  wide pairs           a pair of driver blocks that spans more doc ids than a tile buffer's entries cover (28 672) inside a directory-mode item is
                       probed per candidate; a driver of more than 64 blocks reloads its metadata window inside such an item; an item whose ids
                       reach beyond the directories' range keeps the window path.

Compared bit for bit: status, n_hits, num_matched, and of the rows in front of n_hits keys, all three score words and text_match (rows behind n_hits are
undefined, include/tsgpu.h); the matched ids through keyword_search_batch_ids. Every layout condition a test relies on is computed from
GpuIndex.term_blocks, and that the kernel took the path in question is read from the counting instantiation's counters (kw_find_dir_items, kw_find_pairs,
kw_find_dir_pairs, kw_find_dir_wide_pairs), so a test cannot pass on a layout or a plan that never exercises its case."""
import numpy as np

import typesense_amd as T
from oracle import oracle_py as O
from tests import helpers as H
from tests import mutated_index_common as M

SORT = M.SORT
K = 250
TILE_IDS = 28672                           # doc ids whose directory entries fill one tile buffer of kw_find2_kernel (896 entries of 32 ids)
SPAN_PCT = 80                              # default of option kw_find_dir_span_pct
EVERY_ITEM = 1 << 20                       # kw_find_dir_span_pct so large that every item over a second list with a directory takes directory mode


# ---------------------------------------------------------------- plumbing
def load(lib_path, n_docs, lists, num_docs=None, slack=False):
    """lists: {term: sorted ids}, one position per document -> (oracle, GpuIndex)"""
    pts = H.points_of(n_docs)
    g = T.GpuIndex(0, lib_path)
    if slack:                                                        # room at the arena tails: the commits after the first stay incremental
        g.set_option("index_min_slack_words", 1 << 20)
        g.set_option("index_compact_min_words", 1 << 26)
    g.field_create(0, False)
    for t, ids in lists.items():
        ids = np.asarray(ids, np.uint32)
        g.term_upsert(0, t, ids, np.arange(ids.size, dtype=np.uint32), M.pos_of(ids))
    g.column_set(0, pts)
    g.set_num_docs(num_docs or n_docs)
    g.commit()
    return oracle_of(n_docs, lists, num_docs), g


def oracle_of(n_docs, lists, num_docs=None):
    orc = O.OracleIndex(1, 1)
    for t, ids in lists.items():
        ids = np.asarray(ids, np.uint32)
        orc.load_posting(0, t, ids, np.arange(ids.size, dtype=np.uint32), M.pos_of(ids))
    orc.set_num_docs(num_docs or n_docs)
    orc.set_sort_dense(0, H.points_of(n_docs))
    return orc


def kwq(tokens, **kw):
    kw.setdefault("topster_size", K)
    return T.KwQuery(tokens, sort=SORT, **kw)


def search(g, qs, ids=True):
    if ids:
        return g.keyword_search_batch_ids(qs, k_stride=K)
    return g.keyword_search_batch(qs, k_stride=K), None


def assert_same(a, b, what):
    (ha, ia), (hb, ib) = a, b
    for name in ("status", "n_hits", "num_matched"):
        assert np.array_equal(getattr(ha, name), getattr(hb, name)), "%s: %s differs" % (what, name)
    for i in range(ha.n_hits.size):
        n = int(ha.n_hits[i])
        for name in ("keys", "scores", "text_match"):
            assert getattr(ha, name)[i, :n].tobytes() == getattr(hb, name)[i, :n].tobytes(), "%s q%d: %s differs" % (what, i, name)
        if ia is not None and ib is not None:
            assert np.array_equal(ia[i], ib[i]), "%s q%d: matched ids differ" % (what, i)


def assert_oracle(orc, qs, res, what, ids_cap, refs=None):
    hits, ids = res
    assert (hits.status == 0).all(), (what, hits.status)
    total = 0
    for i, q in enumerate(qs):
        ref = refs[i] if refs is not None else H.oracle_keyword(orc, q, cap=2048, ids_cap=ids_cap)
        H.assert_hits_equal(hits, i, ref, what)
        if ids is not None:
            assert ref.n_result_ids <= ids_cap and np.array_equal(ids[i], ref.result_ids), "%s q%d: matched ids" % (what, i)
        total += int(ref.num_keyword_matches)
    return total


def counted(g, qs):
    """the batch under the byte-counting instantiation -> (result, {counter: value})"""
    g.set_option("kw_count_touched", 1)
    try:
        res = search(g, qs)
    finally:
        g.set_option("kw_count_touched", 0)
    return res, {n: g.counter("kw_find_" + n) for n in ("dir_items", "pairs", "dir_pairs", "dir_wide_pairs")}


def straddles(L):
    """block boundaries of a layout whose two ids share a directory entry -> (behind a full block, behind a part-filled block)"""
    same = (L["last_id"][:-1] >> 5) == (L["first_id"][1:] >> 5)
    full = L["n_ids"][:-1] == 256
    return int((same & full).sum()), int((same & ~full).sum())


# ---------------------------------------------------------------- 1. split-free entries
N1 = 4000
LONG, MID, SHORT = 3, 2, 1


def split_lists():
    long_ids = 3 * np.arange(3 * 256 + 10) + 5                        # stride 3: ids 770 | 773, 1538 | 1541, 2306 | 2309 around the block boundaries
    windows = sorted({int(long_ids[256 * b - 1]) >> 5 for b in (1, 2, 3)})
    win_ids = np.concatenate([np.arange(32 * w, 32 * w + 32) for w in windows])
    rng = np.random.default_rng(5)
    return {SHORT: np.union1d(win_ids, rng.choice(N1, size=120, replace=False)), MID: np.union1d(win_ids, rng.choice(N1, size=500, replace=False)), LONG: long_ids}, win_ids


def split_queries():
    return [kwq([SHORT, MID, LONG]), kwq([LONG, SHORT, MID]), kwq([SHORT, LONG]), kwq([MID, LONG]), kwq([LONG]), kwq([MID, SHORT])]


def body_split_free_entries(lib_path):
    lists, win_ids = split_lists()
    assert lists[SHORT].size < lists[MID].size < lists[LONG].size and lists[SHORT].size < 256 <= lists[MID].size      # the long list is the third token
    orc, g = load(lib_path, N1, lists, slack=True)
    try:
        qs = split_queries()
        L = g.term_blocks(0, LONG)
        assert L["n_ids"].tolist() == [256, 256, 256, 10] and (L["ids_bits"] == 16).all() and L["has_dir"] and g.term_blocks(0, MID)["has_dir"]
        assert straddles(L) == (3, 0), "no block boundary of the long list falls inside a directory entry"
        for b in (1, 2, 3):                                              # ... and the queries ask for every id of those entries
            w = int(L["first_id"][b]) >> 5
            assert np.isin(np.arange(32 * w, 32 * w + 32), lists[SHORT]).all() and np.isin(np.arange(32 * w, 32 * w + 32), lists[MID]).all()
        assert g.counter("kw_iddir_built") >= 2 and g.counter("kw_iddir_split_entries") == 0
        packed = search(g, qs)
        n = assert_oracle(orc, qs, packed, "packed index", N1)
        assert n >= 6 * 20
        _, c = counted(g, qs)
        assert c["dir_pairs"] > 0
        g.set_option("kw_find_dir_tile", 0)
        assert_same(packed, search(g, qs), "packed index, window path")
        g.set_option("kw_find_dir_tile", 1)
        # directories off (the option asks for a full commit), and on again
        g.set_option("kw_iddir_min_ids", 0)
        g.commit()
        assert g.counter("kw_iddir_lists") == 0
        assert_same(packed, search(g, qs), "directories off")
        g.set_option("kw_iddir_min_ids", 256)
        g.commit()
        assert g.counter("kw_iddir_lists") >= 2 and g.counter("kw_iddir_split_entries") == 0
        assert_same(packed, search(g, qs), "directories on again")
        # an id into the middle of a full block (as tests/mutated_index_common.py splits its blocks): two halves, the second one part-filled IN FRONT of
        # a boundary that falls inside a directory entry
        ids = lists[LONG][256:512]
        new = int(ids[128]) - 1
        assert new not in lists[LONG]
        inc = g.counter("commit_incremental_count")
        for t in (LONG, MID, SHORT):
            g.posting_upsert(0, t, new, M.pos_of([new]))
            lists[t] = np.union1d(lists[t], [new])
        g.commit()
        assert g.counter("commit_incremental_count") == inc + 1 and g.counter("commit_compactions") == 0
        L = g.term_blocks(0, LONG)
        assert int(L["n_ids"].sum()) == lists[LONG].size and (L["n_ids"][1:-1] < 256).any()
        in_full, in_part = straddles(L)
        assert in_part >= 1 and in_full >= 1, (in_full, in_part, L["n_ids"])
        assert g.counter("kw_iddir_split_entries") >= in_part >= 1
        orc.close()
        orc = oracle_of(N1, lists)
        mutated = search(g, qs)
        assert_oracle(orc, qs, mutated, "after the incremental upsert", N1)
        assert any(new in x for x in mutated[1])
        g.set_option("kw_find_dir_tile", 0)
        assert_same(mutated, search(g, qs), "after the incremental upsert, window path")
    finally:
        g.close()
        orc.close()


# ---------------------------------------------------------------- 2. directory tile against window path
class ZipfWorld:
    def __init__(self, lib_path):
        self.docs = H.zipf_docs(3000, 300, 12, seed=1)
        self.orc, self.g = H.build_pair(self.docs, lib_path)
        self.refs = {}

    def close(self):
        self.g.close()
        self.orc.close()

    def oracle(self, tag, qs):
        if tag not in self.refs:
            self.refs[tag] = [H.oracle_keyword(self.orc, q, cap=2048, ids_cap=4000) for q in qs]
        return self.refs[tag]


def zipf_queries(plain_only=False):
    """frequent terms (every list of at least 256 ids carries a directory): 1, 2, 3 and 4-6 tokens; filters and exclusions"""
    rng = np.random.default_rng(321)
    qs = []
    for n_tok in (1, 2, 3, 4, 5, 6):
        toks = [rng.choice(np.arange(1, 25), size=n_tok, replace=False) for _ in range(7)]
        filt = np.sort(rng.choice(3000, size=900, replace=False)).astype(np.uint32)
        qs += [kwq(t) for t in toks[:4]]
        if not plain_only:
            qs += [kwq(toks[4], topster_size=40, filter_ids=filt), kwq(toks[5], topster_size=9, excluded_ids=np.arange(0, 3000, 4, dtype=np.uint32)),
                   kwq(toks[6], filter_ids=filt, excluded_ids=np.arange(1, 3000, 5, dtype=np.uint32))]
    return qs


def body_dir_tile_equals_window_path(w):
    g = w.g
    qs = zipf_queries()
    refs = w.oracle("all", qs)
    try:
        for chunk in (0, 1, 3):                                       # (1 and 3 blocks per item: items start mid-list, single-block and odd items)
            g.set_option("kw_chunk_blocks", chunk)
            on = search(g, qs)
            n = assert_oracle(w.orc, qs, on, "directory tile, chunk %d" % chunk, 4000, refs)
            assert n >= 1000, n
            g.set_option("kw_find_dir_tile", 0)
            assert_same(on, search(g, qs), "window path, chunk %d" % chunk)
            g.set_option("kw_find_dir_tile", 1)
            # the byte-counting instantiation: same results, and the counters say which path ran
            res, c = counted(g, qs)
            assert_same(on, res, "counting instantiation, chunk %d" % chunk)
            assert c["dir_items"] > 0 and c["pairs"] >= c["dir_pairs"] > 0 and c["dir_wide_pairs"] == 0, c
            g.set_option("kw_find_dir_tile", 0)
            res, c0 = counted(g, qs)
            assert_same(on, res, "counting instantiation, window path, chunk %d" % chunk)
            assert c0["dir_items"] == c0["dir_pairs"] == 0 and c0["pairs"] == c["pairs"], (c0, c)
            g.set_option("kw_find_dir_tile", 1)
    finally:
        g.set_option("kw_chunk_blocks", 0)
        g.set_option("kw_find_dir_tile", 1)


def body_device_planner_equals_host_planner(w):
    """the device-side planner takes batches of plain queries (no filter / excluded ids, no ids read back)"""
    g = w.g
    qs = zipf_queries(plain_only=True)
    refs = w.oracle("plain", qs)
    try:
        for chunk in (0, 3):
            g.set_option("kw_chunk_blocks", chunk)
            host = search(g, qs, ids=False)
            assert_oracle(w.orc, qs, host, "host planner, chunk %d" % chunk, 4000, refs)
            plans = g.counter("kw_device_plans")
            g.set_option("kw_device_plan_min_queries", 1)
            assert_same(host, search(g, qs, ids=False), "device planner, chunk %d" % chunk)
            g.set_option("kw_find_dir_tile", 0)
            assert_same(host, search(g, qs, ids=False), "device planner, window path, chunk %d" % chunk)
            assert g.counter("kw_device_plans") == plans + 2, "the batches were not planned on the device"
            g.set_option("kw_find_dir_tile", 1)
            g.set_option("kw_device_plan_min_queries", 512)
    finally:
        g.set_option("kw_chunk_blocks", 0)
        g.set_option("kw_find_dir_tile", 1)
        g.set_option("kw_device_plan_min_queries", 512)


def body_mutated_lists(w, token_sets=None):
    """the mutated world of tests/mutated_index_common.py: D, B and A carry directories — part-filled, one-id, widened and relocated blocks as the second
    list of a directory-mode item. Its drivers are sparse (the ids spread over 300 000 documents): at the default span only B over D qualifies, so the
    comparison also runs with a span that admits every item, where the pairs of the short drivers overflow the tile and are probed per candidate."""
    g = w.g
    sets = [ts for ts in (token_sets or M.TOKEN_SETS) if len(ts) >= 2]
    assert all(g.term_blocks(0, t)["has_dir"] and g.term_blocks(0, t)["has_breaks"] for t in (M.D, M.B, M.A))
    qs = [q for q, _ in M.single_field_queries(0, sets)]
    _, c = counted(g, qs)
    assert c["dir_items"] > 0 and c["dir_pairs"] > 0, c
    with M.options(w, {"kw_find_dir_span_pct": (EVERY_ITEM, SPAN_PCT)}):
        _, c2 = counted(g, qs)
    assert c2["dir_items"] > c["dir_items"] and c2["dir_pairs"] > c["dir_pairs"] and c2["dir_wide_pairs"] > 0, (c, c2)
    for name, opts in (("default span", {}), ("every item", {"kw_find_dir_span_pct": (EVERY_ITEM, SPAN_PCT)}), ("window path", {"kw_find_dir_tile": (0, 1)}),
                       ("every item, chunk 3", {"kw_find_dir_span_pct": (EVERY_ITEM, SPAN_PCT), "kw_chunk_blocks": (3, 0)}),
                       ("window path, chunk 3", {"kw_find_dir_tile": (0, 1), "kw_chunk_blocks": (3, 0)})):
        with M.options(w, opts):                                      # (against the oracle, and against what the body returned under the other options)
            n = M.check_queries(w, M.single_field_queries(0, sets), "mutated lists, " + name, remember=("dir tile", token_sets is None))
        assert n >= 1000, (name, n)


# ---------------------------------------------------------------- 3. a pair wider than the tile inside a directory-mode item
N3 = 200_000
DRIVER, SECOND, THIRD = 1, 2, 3


def wide_lists():
    rng = np.random.default_rng(11)
    low = np.sort(rng.choice(10_000, size=400, replace=False))
    high = 100_000 + np.sort(rng.choice(90_000, size=70 * 256 - 400, replace=False))       # 70 blocks in all: the metadata window (64) is reloaded
    second = np.nonzero(rng.random(N3) < 0.5)[0]
    third = np.nonzero(rng.random(N3) < 0.6)[0]
    return {DRIVER: np.concatenate([low, high]), SECOND: second, THIRD: third}


def body_pair_wider_than_the_tile(lib_path):
    lists = wide_lists()
    assert lists[DRIVER].size < lists[SECOND].size < lists[THIRD].size
    orc, g = load(lib_path, N3, lists)
    try:
        g.set_option("kw_chunk_blocks", 256)                           # the driver is ONE work item
        L = g.term_blocks(0, DRIVER)
        nb = L["n_ids"].size
        assert nb == 70 > 64 and g.term_blocks(0, SECOND)["has_dir"] and g.term_blocks(0, THIRD)["has_dir"]
        pairs = (nb + 1) // 2
        lo, hi = L["first_id"][0::2].astype(np.int64), L["last_id"][1::2].astype(np.int64)
        entries = (hi >> 5) - (lo >> 5) + 1
        assert (entries > TILE_IDS // 32).sum() == 1 and entries[0] > TILE_IDS // 32, "no pair of driver blocks is wider than the tile"
        assert int(L["last_id"][-1]) - int(L["first_id"][0]) <= SPAN_PCT * TILE_IDS // 100 * pairs, "the item does not qualify for directory mode"
        qs = [kwq([DRIVER, SECOND]), kwq([THIRD, DRIVER, SECOND]), kwq([DRIVER, THIRD]), kwq([DRIVER, SECOND], topster_size=40, filter_ids=np.arange(0, N3, 3, dtype=np.uint32))]
        on = search(g, qs)
        n = assert_oracle(orc, qs, on, "wide pair", N3)
        assert n > 10_000, n
        res, c = counted(g, qs)
        assert_same(on, res, "wide pair, counting instantiation")
        assert c["dir_items"] == len(qs) and c["pairs"] == len(qs) * pairs and c["dir_wide_pairs"] == len(qs) and c["dir_pairs"] == len(qs) * (pairs - 1), c
        g.set_option("kw_find_dir_tile", 0)
        assert_same(on, search(g, qs), "wide pair, window path")
    finally:
        g.close()
        orc.close()


def body_item_beyond_the_directories_range(lib_path):
    """The directories cover the doc ids [0, num_docs + num_docs / 8 + 1024 rounded up to 2048); the C-ABI takes lists with ids beyond num_docs (a doc-range
    shard keeps global seq_ids), so an index declared at 4 000 documents whose lists reach 10 000 has work items on either side of the range: those
    whose last id lies beyond it keep the window path."""
    n_ids, declared = 10_000, 4000
    cap = (declared + declared // 8 + 1024 + 2047) // 2048 * 2048
    rng = np.random.default_rng(13)
    lists = {DRIVER: np.nonzero(rng.random(n_ids) < 0.3)[0], SECOND: np.nonzero(rng.random(n_ids) < 0.5)[0], THIRD: np.nonzero(rng.random(n_ids) < 0.6)[0]}
    orc, g = load(lib_path, n_ids, lists, num_docs=declared)
    try:
        g.set_option("kw_chunk_blocks", 2)
        L = g.term_blocks(0, DRIVER)
        assert g.term_blocks(0, SECOND)["has_dir"]
        item_last = L["last_id"][1::2] if L["n_ids"].size % 2 == 0 else np.append(L["last_id"][1::2], L["last_id"][-1])
        inside = int((item_last < cap).sum())
        assert 0 < inside < item_last.size, (cap, item_last)
        qs = [kwq([DRIVER, SECOND]), kwq([DRIVER, SECOND, THIRD])]
        on = search(g, qs)
        n = assert_oracle(orc, qs, on, "beyond the range", n_ids)
        assert n > 1000, n
        res, c = counted(g, qs)
        assert_same(on, res, "beyond the range, counting instantiation")
        assert c["dir_items"] == len(qs) * inside and c["pairs"] == len(qs) * item_last.size, (c, inside)
        g.set_option("kw_find_dir_tile", 0)
        assert_same(on, search(g, qs), "beyond the range, window path")
    finally:
        g.close()
        orc.close()
