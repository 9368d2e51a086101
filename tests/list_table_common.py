"""Shared bodies of tests/test_emu_list_table.py (CPU tier, SIMT emulator) and tests/test_gpu_list_table.py (-m gpu, libtsgpu.so): the per-work-item LIST
TABLE of kw_find2_kernel and kw_score_kernel (typesense_amd/csrc/kw_kernels.hip.h).

  probes   the find kernel's third.. lists (and the second list of a pair wider than the tile) are probed through a table row {first id, last id,
           directory base}: the range test reads the row, the directory entry is one 8-byte load, and only the two-level search (no directory, a marked
           entry, an id beyond the directories' range) reads the list's descriptor.
  runs     the score kernel takes a list's payload base and first block from its table row, a block's BlockMeta as two 16-byte loads, and elements i and
           i + 1 of a packed offset_index out of ONE 8-byte window where they are at most 16 bits wide.

Compared bit for bit against the oracle: status, n_hits, num_matched, and of the rows in front of n_hits keys, all three score words and text_match; the
matched ids through keyword_search_batch_ids. Every layout condition a case relies on is asserted BEFORE the search: block sizes and has_dir from
GpuIndex.term_blocks, packed widths computed from the postings the test built (the packer's rule: required_bits of the largest value, offsets relative to
the block's smallest), the path from the counting instantiation's counters."""
import numpy as np

import typesense_amd as T
from oracle import oracle_py as O
from tests import helpers as H
from tests import mutated_index_common as M
from tests import find_dir_tile_common as F

SORT = M.SORT
K = 250
DIR_MIN = 313                              # 20 000 documents: a list of at least num_docs / 64 ids carries a directory


def kwq(tokens, **kw):
    kw.setdefault("topster_size", K)
    return T.KwQuery(tokens, sort=SORT, **kw)


def bits_of(v):
    return int(v).bit_length()


# ---------------------------------------------------------------- plumbing: lists with explicit runs
class Lists:
    """{term: (ids, [offsets of document i])} -> library + oracle"""

    def __init__(self, n_docs, num_docs=None):
        self.n_docs, self.num_docs, self.p = n_docs, num_docs or n_docs, {}

    def add(self, term, ids, runs=None):
        ids = np.asarray(ids, np.int64)
        assert ids.size and (np.diff(ids) > 0).all() and ids[-1] < self.n_docs
        if runs is None:
            runs = [(int(p),) for p in M.pos_of(ids)]
        assert len(runs) == ids.size
        self.p[term] = (ids, [tuple(int(x) for x in r) for r in runs])

    def ids(self, term):
        return self.p[term][0]

    def arrays(self, term):
        ids, runs = self.p[term]
        oi = np.zeros(ids.size, np.uint32)
        oi[1:] = np.cumsum([len(r) for r in runs])[:-1]
        return ids.astype(np.uint32), oi, np.array([x for r in runs for x in r], np.uint32)

    def widths(self, term, block):
        """(offset_index bits, offsets bits) of block `block` of a freshly packed list (blocks of 256 ids)"""
        ids, runs = self.p[term]
        r = runs[256 * block:256 * block + 256]
        starts = np.concatenate([[0], np.cumsum([len(x) for x in r])[:-1]])
        flat = [x for y in r for x in y]
        return bits_of(starts.max()), bits_of(max(flat) - min(flat))

    def load(self, lib_path):
        g = T.GpuIndex(0, lib_path)
        orc = O.OracleIndex(1, 1)
        g.field_create(0, False)
        for t in self.p:
            a = self.arrays(t)
            g.term_upsert(0, t, *a)
            orc.load_posting(0, t, *a)
        pts = H.points_of(self.n_docs)
        g.column_set(0, pts)
        g.set_num_docs(self.num_docs)
        g.commit()
        orc.set_num_docs(self.num_docs)
        orc.set_sort_dense(0, pts)
        return orc, g


def three_ways(orc, g, qs, what, ids_cap, min_matches=1):
    """the batch through the host planner (with the matched ids), the device planner and the counting instantiation -> the counters"""
    host = F.search(g, qs)
    n = F.assert_oracle(orc, qs, host, what + ", host planner", ids_cap)
    assert n >= min_matches, (what, n)
    plans = g.counter("kw_device_plans")
    g.set_option("kw_device_plan_min_queries", 1)
    try:
        dev = F.search(g, qs, ids=False)
    finally:
        g.set_option("kw_device_plan_min_queries", 512)
    assert g.counter("kw_device_plans") == plans + 1, what + ": the batch was not planned on the device"
    F.assert_same((host[0], None), dev, what + ", device planner")
    res, c = F.counted(g, qs)
    F.assert_same(host, res, what + ", counting instantiation")
    return c, host


# ---------------------------------------------------------------- 1. probes of a third list
N = 20_000
DRV, SEC, THIRD = 1, 2, 3                  # a third list WITH a directory
DRV2, SEC2, THIRD2 = 4, 5, 6               # ... without
DRV3, SEC3, THIRD3 = 7, 8, 9               # batch fill: 612 stage-1 survivors in one work item
MANY = list(range(20, 30))                 # ten lists that share a core: 4- and 10-token queries
T_FIRST, T_STRIDE, T_COUNT = 1000, 3, 3 * 256 + 10


def probe_lists():
    rng = np.random.default_rng(7)
    L = Lists(N)
    third = T_FIRST + T_STRIDE * np.arange(T_COUNT)
    last = int(third[-1])
    cases = dict(below=T_FIRST - 7, first=T_FIRST, last=last, above=last + 9, clear=T_FIRST + 1, bit0=1024, bit31=1087,
                 straddle_lo=int(third[255]), straddle_hi=int(third[256]))
    members = rng.choice(third, size=30, replace=False)
    others = rng.choice(np.setdiff1d(np.arange(T_FIRST, last), third), size=30, replace=False)
    drv = np.unique(np.concatenate([list(cases.values()), members, others]))
    sec = np.union1d(drv, rng.choice(N, size=330, replace=False))
    L.add(DRV, drv); L.add(SEC, sec); L.add(THIRD, third)
    drv2 = np.sort(rng.choice(np.arange(100, 900), size=50, replace=False))
    third2 = np.union1d(drv2[::2], rng.choice(np.arange(50, 950), size=260, replace=False))[:300]
    L.add(DRV2, drv2); L.add(SEC2, np.union1d(drv2, rng.choice(1000, size=70, replace=False))); L.add(THIRD2, third2)
    drv3 = 4000 + 7 * np.arange(612)
    L.add(DRV3, drv3); L.add(SEC3, np.union1d(drv3, rng.choice(np.arange(3500, 9000), size=150, replace=False)))
    L.add(THIRD3, np.array([x for x in range(3500, 9000) if x % 5]))
    core = np.sort(rng.choice(np.arange(10_000, 19_000), size=40, replace=False))
    for i, t in enumerate(MANY):
        L.add(t, np.union1d(core, rng.choice(np.arange(9_500, 19_500), size=60 + 150 * i, replace=False)))
    return L, cases


class ProbeWorld:
    def __init__(self, lib_path):
        self.L, self.cases = probe_lists()
        self.orc, self.g = self.L.load(lib_path)

    def close(self):
        self.g.close()
        self.orc.close()


def body_third_list_with_directory(w):
    L, g, c = w.L, w.g, w.cases
    third, drv = L.ids(THIRD), L.ids(DRV)
    assert L.ids(DRV).size < L.ids(SEC).size < third.size and np.isin(drv, L.ids(SEC)).all()      # THIRD is the third list, every case survives stage 1
    B3 = g.term_blocks(0, THIRD)
    assert B3["has_dir"] and B3["n_ids"].tolist() == [256, 256, 256, 10] and third.size >= DIR_MIN
    assert int(B3["first_id"][0]) == c["first"] and int(B3["last_id"][-1]) == c["last"] and c["below"] < c["first"] and c["above"] > c["last"]
    assert c["clear"] not in third and c["first"] < c["clear"] < c["last"] and np.isin(np.arange(c["clear"] & ~31, (c["clear"] & ~31) + 32), third).any()
    assert c["bit0"] % 32 == 0 and c["bit31"] % 32 == 31 and c["bit0"] in third and c["bit31"] in third
    assert int(B3["last_id"][0]) == c["straddle_lo"] and int(B3["first_id"][1]) == c["straddle_hi"] and c["straddle_lo"] >> 5 == c["straddle_hi"] >> 5
    assert F.straddles(B3)[1] == 0 and g.counter("kw_iddir_split_entries") == 0
    assert all(v in drv for v in c.values())
    qs = [kwq([DRV, SEC, THIRD])]
    cnt, host = three_ways(w.orc, g, qs, "third list with a directory", N, min_matches=30)
    want = np.intersect1d(drv, third)
    assert np.array_equal(host[1][0], want) and all(c[k] in want for k in ("first", "last", "bit0", "bit31", "straddle_lo", "straddle_hi"))
    assert cnt["pairs"] >= 1


def body_third_list_without_directory(w):
    L, g = w.L, w.g
    assert L.ids(DRV2).size < L.ids(SEC2).size < L.ids(THIRD2).size < DIR_MIN and not g.term_blocks(0, THIRD2)["has_dir"]
    assert g.term_blocks(0, THIRD2)["n_ids"].tolist() == [256, L.ids(THIRD2).size - 256]
    _, host = three_ways(w.orc, g, [kwq([DRV2, SEC2, THIRD2])], "third list without a directory", N, min_matches=20)
    assert np.array_equal(host[1][0], np.intersect1d(L.ids(DRV2), L.ids(THIRD2)))


def body_batch_fill(w):
    L, g = w.L, w.g
    assert np.isin(L.ids(DRV3), L.ids(SEC3)).all() and L.ids(DRV3).size == 612 < L.ids(SEC3).size < L.ids(THIRD3).size
    assert g.term_blocks(0, DRV3)["n_ids"].tolist() == [256, 256, 100] and g.term_blocks(0, THIRD3)["has_dir"]
    g.set_option("kw_chunk_blocks", 4)                                 # the driver is ONE work item: two full batches out of the first pair, a tail of 100
    try:
        cnt, host = three_ways(w.orc, g, [kwq([DRV3, SEC3, THIRD3])], "batch fill", N, min_matches=400)
    finally:
        g.set_option("kw_chunk_blocks", 0)
    assert cnt["pairs"] == 2, cnt
    assert np.array_equal(host[1][0], np.intersect1d(L.ids(DRV3), L.ids(THIRD3)))


def body_query_shapes(w):
    L, g = w.L, w.g
    sizes = [L.ids(t).size for t in MANY]
    assert sizes == sorted(sizes) and len(set(sizes)) == 10 and sum(g.term_blocks(0, t)["has_dir"] for t in MANY) >= 6
    qs = [kwq([THIRD]), kwq([DRV, THIRD]), kwq([DRV, SEC, THIRD]),
          kwq(MANY[:4]), kwq(MANY), kwq(MANY[::-1]),                   # the TMAX = 10 kernels: four and ten rows
          kwq([THIRD, SEC, THIRD]),                                    # one term twice
          kwq([THIRD, DRV, SEC]), kwq([MANY[9], MANY[3], MANY[0], MANY[5]])]      # the driver is not the first token
    assert L.ids(DRV).size < min(L.ids(SEC).size, L.ids(THIRD).size)
    three_ways(w.orc, g, qs, "query shapes", N, min_matches=len(qs) * 30)


def body_three_queries_over_disjoint_lists(w):
    g = w.g
    assert g.term_blocks(0, DRV3)["n_ids"].size == 3
    g.set_option("kw_chunk_blocks", 1)                                 # three work items for the first query
    try:
        cnt, _ = three_ways(w.orc, g, [kwq([DRV3, SEC3, THIRD3]), kwq([DRV, SEC, THIRD]), kwq([DRV2, SEC2, THIRD2])], "three queries", N, min_matches=450)
    finally:
        g.set_option("kw_chunk_blocks", 0)
    assert cnt["pairs"] == 3 + 1 + 1, cnt


def body_wide_run(lib_path):
    """a pair of driver blocks wider than the tile over a second list with a directory: both candidates' entries through the second list's row"""
    lists = F.wide_lists()
    orc, g = F.load(lib_path, F.N3, lists)
    try:
        g.set_option("kw_chunk_blocks", 256)
        assert g.term_blocks(0, F.SECOND)["has_dir"] and g.term_blocks(0, F.THIRD)["has_dir"]
        qs = [kwq([F.DRIVER, F.SECOND]), kwq([F.THIRD, F.DRIVER, F.SECOND])]
        cnt, _ = three_ways(orc, g, qs, "wide run", F.N3, min_matches=5000)
        assert cnt["dir_wide_pairs"] == len(qs) and cnt["dir_items"] == len(qs), cnt
    finally:
        g.close()
        orc.close()


def body_beyond_the_directories_range(lib_path):
    """set_num_docs below the lists' last ids: candidates at or beyond the directories' range take the two-level search although the list has a directory"""
    n_ids, declared = 10_000, 4000
    cap = (declared + declared // 8 + 1024 + 2047) // 2048 * 2048
    rng = np.random.default_rng(13)
    L = Lists(n_ids, num_docs=declared)
    drv = np.nonzero(rng.random(n_ids) < 0.05)[0]
    L.add(1, drv); L.add(2, np.union1d(drv, np.nonzero(rng.random(n_ids) < 0.1)[0])); L.add(3, np.nonzero(rng.random(n_ids) < 0.6)[0])
    orc, g = L.load(lib_path)
    try:
        assert L.ids(1).size < L.ids(2).size < L.ids(3).size and g.term_blocks(0, 3)["has_dir"] and int(L.ids(3)[-1]) >= cap
        want = np.intersect1d(L.ids(1), L.ids(3))
        assert (want >= cap).sum() >= 50 and (want < cap).sum() >= 50 and cap in range(declared, n_ids)
        _, host = three_ways(orc, g, [kwq([1, 2, 3])], "beyond the directories' range", n_ids, min_matches=100)
        assert np.array_equal(host[1][0], want)
    finally:
        g.close()
        orc.close()


def body_split_entry(w):
    """w: a mutated_index_common.World. A directory entry of D that straddles a block boundary behind a part-filled block carries IDDIR_SPLIT; D's ids in
    such entries go into R and S, so that [R, S, D] probes D — its third list — at them and takes the marked-entry fallback."""
    g = w.g
    LD = g.term_blocks(0, M.D)
    assert LD["has_dir"] and g.counter("kw_iddir_split_entries") >= 1
    part = np.nonzero((LD["n_ids"][:-1] < 256) & ((LD["last_id"][:-1] >> 5) == (LD["first_id"][1:] >> 5)))[0]
    assert part.size >= 1, "no entry of D straddles a boundary behind a part-filled block"
    d_ids = w.ids(0, M.D)
    asked = []
    for b in part[:4]:
        e = int(LD["last_id"][b]) >> 5
        asked += [int(x) for x in d_ids[(d_ids >> 5) == e]]
    assert len(asked) >= 2
    for x in asked:
        for t in (M.R, M.S):
            w.upsert(0, t, x)
    w.commit("split-entry candidates")
    w.fresh_oracle()
    assert len(w.model[0][M.R]) < len(w.model[0][M.S]) < len(w.model[0][M.D])
    LD2 = g.term_blocks(0, M.D)
    assert np.array_equal(LD2["first_id"], LD["first_id"]) and np.array_equal(LD2["n_ids"], LD["n_ids"])      # D itself was not touched
    qs = [M.kwq([M.R, M.S, M.D])]
    n = M.check_queries(w, qs, "split entry, host planner")
    assert n >= len(asked)
    ids = g.keyword_search_batch_ids([q for q in qs], k_stride=K)[1][0]
    assert np.isin(asked, ids).all()
    with M.options(w, {"kw_device_plan_min_queries": (1, 512)}):
        plans = g.counter("kw_device_plans")
        M.check_queries(w, qs, "split entry, device planner", keep_ids=False)
        assert g.counter("kw_device_plans") > plans
    with M.options(w, {"kw_count_touched": (1, 0)}):
        M.check_queries(w, qs, "split entry, counting instantiation")


# ---------------------------------------------------------------- 2. runs of the score kernel
W8, W15, W16, W17, ONE, TWO, ZERO, BIG = 40, 41, 42, 43, 44, 45, 46, 47      # subject lists
COMP = 60                                  # a dense companion (directory): the third token
PIN0 = 100                                 # PIN0 + case: a one-id list at the case's document (the driver: exactly one hit)
SCORE_N = 20_000


def run_of(doc, n, last_flag, far=False):
    """n ascending positions from a hash of the document (+ 1: 0 is the last-token flag), + the flag"""
    start = 1 + (doc * 2654435761 >> 7) % 5 + (40_000 if far else 0)
    step = 1 + (doc * 40503 >> 3) % 3
    r = [start + step * i for i in range(n)]
    return tuple(r + [0]) if last_flag else tuple(r)


def score_lists(thin):
    """thin (emulator tier): the 15 / 16 / 17-bit blocks keep their widths (one block each), the companions are shorter"""
    rng = np.random.default_rng(17)
    L = Lists(SCORE_N)
    per_doc = {W8: 1, W15: 100, W16: 200, W17: 258}
    cases = []                                                          # (subject, document, what)
    for t in (W8, W15, W16, W17):
        n_ids = 256 + 256 + 77 if t == W8 else 256 + 44                 # full blocks, then a part-filled final block
        ids = np.sort(rng.choice(np.arange(500, SCORE_N - 500), size=n_ids, replace=False))
        runs = []
        for j, d in enumerate(ids):
            n = per_doc[t] if j < 256 or t == W8 else 1 + j % 3         # (run lengths 1, 2, 3 behind the wide block)
            runs.append(run_of(int(d), n, last_flag=bool(j % 2)))
        if t == W8:                                                     # runs of 1, 2 and 3+ positions in the second block; first block: one position each
            runs[0:256] = [run_of(int(d), 1, last_flag=False) for d in ids[0:256]]
            runs[256:512] = [run_of(int(d), 1 + j % 4, last_flag=bool(j % 3 == 0)) for j, d in enumerate(ids[256:512])]
        L.add(t, ids, runs)
        slots = [0, 1, 2, 17, 127, 128, 254, 255] if t != W8 else [0, 5, 6, 255, 256, 256 + 9, 256 + 10, 511, 512, n_ids - 1]
        if t != W8:
            slots += [256, n_ids - 1]
        cases += [(t, int(ids[s]), "slot %d" % s) for s in slots]
    d1 = 7777
    L.add(ONE, [d1], [run_of(d1, 2, True)])
    L.add(TWO, [300, 9000], [run_of(300, 1, False), run_of(9000, 3, True)])
    zero_ids = np.arange(12_000, 12_000 + 256 + 3)
    L.add(ZERO, zero_ids, [(5,)] * zero_ids.size)                       # every offset alike: offsets width 0
    big_ids = np.arange(14_000, 14_300, 1)
    L.add(BIG, big_ids, [run_of(int(d), 1 + j % 3, bool(j % 2), far=(j % 50 == 7)) + ((70_000 + j,) if j % 64 == 9 else ()) for j, d in enumerate(big_ids)])
    cases += [(ONE, d1, "one-id block"), (TWO, 300, "slot 0 of two"), (TWO, 9000, "final slot of two"),
              (ZERO, 12_000, "width 0 slot 0"), (ZERO, 12_255, "width 0 slot 255"), (ZERO, int(zero_ids[-1]), "width 0 final slot"),
              (BIG, 14_009, "wide offsets, long run"), (BIG, 14_007, "far offsets"), (BIG, 14_299, "wide offsets final slot")]
    docs = np.unique([d for _, d, _ in cases])
    comp = np.union1d(docs, rng.choice(SCORE_N, size=1500 if thin else 6000, replace=False))
    L.add(COMP, comp, [run_of(int(d), 1 + int(d) % 2, bool(d % 5 == 0)) for d in comp])
    for i, (_, d, _) in enumerate(cases):
        L.add(PIN0 + i, [d], [run_of(d, 1, False)])
    return L, cases


class ScoreWorld:
    def __init__(self, lib_path, thin=False):
        self.L, self.cases = score_lists(thin)
        self.orc, self.g = self.L.load(lib_path)

    def close(self):
        self.g.close()
        self.orc.close()


def body_score_layout(w):
    """the widths and slots the score cases rely on, from the postings and the committed layout"""
    L, g = w.L, w.g
    assert L.widths(W8, 0)[0] == 8 and L.widths(W15, 0)[0] == 15 and L.widths(W16, 0)[0] == 16 and L.widths(W17, 0)[0] == 17
    assert L.widths(TWO, 0)[0] == 1 and L.widths(ONE, 0)[0] == 0
    assert L.widths(ZERO, 0)[1] == 0 and 0 < L.widths(W8, 1)[1] <= 16 and L.widths(BIG, 0)[1] > 16 and L.widths(BIG, 1)[1] > 16
    for t, nb in ((W8, [256, 256, 77]), (W15, [256, 44]), (W16, [256, 44]), (W17, [256, 44]), (ONE, [1]), (TWO, [2]), (ZERO, [256, 3]), (BIG, [256, 44])):
        assert g.term_blocks(0, t)["n_ids"].tolist() == nb, (t, g.term_blocks(0, t)["n_ids"])
    # an odd and an even slot whose offset_index entry crosses a 32-bit word: width 15: slot 2 = bits 30..44, slot 17 = bits 255..269; width 17: slots 1, 254
    for t, width, slots in ((W15, 15, (2, 17)), (W17, 17, (1, 254))):
        for s in slots:
            assert (s * width) // 32 != (s * width + width - 1) // 32, (t, s)
            assert any(ct == t and d == int(L.ids(t)[s]) for ct, d, _ in w.cases), (t, s)         # ... and a case asks for it
        assert {s % 2 for s in slots} == {0, 1}
    lens = {len(r) for _, runs in [L.p[W8]] for r in runs[256:512]}
    assert {1, 2, 3, 4, 5} <= lens                                      # runs of 1, 2 and 3+ elements, with and without the flag
    assert g.term_blocks(0, COMP)["has_dir"]


def body_score_cases(w, token_counts=(1, 2, 3)):
    """one hit each: the pin list (one id) drives, the subject list is found at the case's slot, the companion is the third token"""
    L, g, orc = w.L, w.g, w.orc
    qs = []
    for i, (t, d, what) in enumerate(w.cases):
        assert d in L.ids(t) and d in L.ids(COMP) and L.ids(PIN0 + i).tolist() == [d]
        if 2 in token_counts:
            qs += [kwq([t, PIN0 + i]), kwq([PIN0 + i, t])]
        if 3 in token_counts:
            qs += [kwq([t, PIN0 + i, COMP]), kwq([COMP, t, PIN0 + i])]
    if 1 in token_counts:
        qs += [kwq([t]) for t in (W8, W15, W16, W17, ONE, TWO, ZERO, BIG)]
    for lo in range(0, len(qs), 64):
        part = qs[lo:lo + 64]
        host = F.search(g, part)
        F.assert_oracle(orc, part, host, "score cases %d.." % lo, SCORE_N)
        for j, q in enumerate(part):
            if len(q.tokens) > 1:
                assert int(host[0].n_hits[j]) == 1, (lo + j, q.tokens)     # ONE hit: the case's document
        plans = g.counter("kw_device_plans")
        g.set_option("kw_device_plan_min_queries", 1)
        try:
            dev = F.search(g, part, ids=False)
        finally:
            g.set_option("kw_device_plan_min_queries", 512)
        assert g.counter("kw_device_plans") == plans + 1
        F.assert_same((host[0], None), dev, "score cases %d.., device planner" % lo)
