"""Shared bodies of tests/test_emu_mutated_index.py (CPU tier, SIMT emulator) and tests/test_gpu_mutated_index.py (-m gpu, libtsgpu.so): every search path
over posting lists that INCREMENTAL commits (tsgpu_index.hip) have left in shapes a from-scratch build never produces — part-filled blocks in mid-list,
one-id blocks, blocks relocated to the arena tails (LIST_HAS_BREAKS, the list's first block among them), blocks whose ids form changed between 16 and
32 bits, id-directory entries that straddle blocks which are no longer neighbours.

World: N0 = 300 000 doc ids (+ room for appended documents), two plain fields (field 1 = the lists of field 0 moved by an affine permutation of the ids),
one dense int64 sort column, one group column. Lists per field, one position per document from a hash of the id:

  D  ~150 000 ids   id directory, almost every block boundary inside a directory entry        B  ~40 000 ids, two holes of 71 000 ids: > 64 blocks, 16-bit
                                                                                                 (drawn per field: a block ends at either hole's start)
  A  ~6 400 ids     a driver of > 20 blocks (carries a directory too: >= num_docs / 64 ids)    S  ~1 100 ids over the whole range: 32-bit blocks
  R  ~450 ids       a short driver                                                            T, U  ~270 / ~210 ids: helper lists SHORTER than R, so that
                                                                                                     R and S can be a second and a third list as well

A Python model {field: {term: {doc: offsets}}} receives every operation; the expectation after a commit is a FRESH OracleIndex loaded from the model
(load_posting) — the reference never reads the library. The write rounds (World.__init__; the library's committed layout is read through
GpuIndex.term_blocks to AIM the operations, never to predict a result):

  round 1   splits of full blocks of D, B, A (an id in the middle; the ids left between the halves go into every OTHER list: their driver ids fall into
            the gap), seven NEIGHBOURING full blocks of B split in one commit (14 part-filled blocks, contiguous at the arena tail: an unbroken run of
            > KW_F2_SPAN blocks under one driver block of S / R), an id at the start of either hole of B (the block behind the hole: 16 -> 32 bits),
            first and last block of every list re-written, a run replaced by one of another length, erases of absent ids
  14 x      one appended document per commit in A and B: a run of 14 one-id blocks, each at another arena position
  round 2   erases that leave blocks of 1, 2 and 127 ids and that empty a block (D; 127 in A and B too), the erase that narrows a widened block of B back
            to 16 bits, appends behind the one-id blocks (the run is now mid-list), the tail ids into S in one block (16-bit, in a 32-bit list), R removed
  round 3   R re-created (posting_upsert, other ids), more appends, a one-id block of A erased
  round 4   a few ids into the re-created R and into S

No commit compacts (index_min_slack_words / index_compact_min_words), every one is incremental (asserted). coverage() then computes from the downloaded
layout that every state is there; the tests fail when the world stops reaching them."""
import itertools

import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B_
from oracle import oracle_py as O
from tests import helpers as H

N0 = 300_000
TAIL = 64                                  # appended documents: ids N0 .. N0 + TAIL - 1
N_DOCS = N0 + TAIL
D, B, A, S, R, TT, U = 1, 2, 3, 4, 5, 6, 7
NAMES = {D: "D", B: "B", A: "A", S: "S", R: "R", TT: "T", U: "U"}
MAIN = (D, B, A, S, R)
FIELDS = (0, 1)
GROUP_COL = 1
K = 250                                    # topster_size = k_stride
HOLES = ((60_000, 131_000), (200_000, 271_000))      # B holds no id in these ranges (71 000 > 65 535 ids wide)
ZC = 150_000                               # the splits are aimed here
SORT = ((B_.SORT_TEXT_MATCH, 1, 0), (B_.SORT_INT64_COLUMN, 1, 0))
IDS_CAP = 1 << 18
F2_SPAN = 12                               # KW_F2_SPAN of kw_find2.hip.h: runs of more second-list blocks take the binary block search
N_TINY = 14                                # one-id blocks in a row: rhi - rlo = 13 > KW_F2_SPAN


def pos_of(ids):
    """one position per document (+ 1: 0 is the last-token flag)"""
    return ((np.asarray(ids, np.uint32) * np.uint32(2654435761) >> np.uint32(27)) % np.uint32(7) + np.uint32(1)).astype(np.uint32)


def perm(ids):
    """field 1: an affine permutation of [0, N0) (7919 is coprime to 300 000); appended documents keep their ids"""
    ids = np.asarray(ids, np.int64)
    return np.where(ids < N0, (ids * 7919 + 12345) % N0, ids)


def in_holes(ids):
    ids = np.asarray(ids)
    m = np.zeros(ids.shape, bool)
    for lo, hi in HOLES:
        m |= (ids >= lo) & (ids < hi)
    return m


B_SEGMENTS = ((0, HOLES[0][0], 40), (HOLES[0][1], HOLES[1][0], 70), (HOLES[1][1], N0, 45))      # (from, to, blocks of 256 ids)


def b_list(rng, core):
    """B: the ids in front of either hole fill whole blocks, so a block ENDS at the hole's start and the next one begins behind the hole: every block of
    the initial list is 16-bit, and an id put at the hole's start widens the block behind it"""
    parts = []
    for k, (lo, hi, blocks) in enumerate(B_SEGMENTS):
        mine = core[(core >= lo) & (core < hi)]
        rest = np.setdiff1d(np.arange(lo, hi), mine)
        n = blocks * 256 - mine.size + (77 if k == 2 else 0)                  # (the list's last block is part-filled)
        parts.append(np.union1d(rng.choice(rest, size=n, replace=False), mine))
    return np.concatenate(parts)


def initial_lists():
    rng = np.random.default_rng(41)
    allowed = np.nonzero(~in_holes(np.arange(N0)) & ~in_holes(perm(np.arange(N0))))[0]
    core = rng.choice(allowed, size=150, replace=False)            # in every list of either field: the many-token queries find something
    sizes = {D: 150_000, A: 6_250, S: 950, R: 300, TT: 120, U: 60}
    f0, f1 = {B: b_list(rng, core)}, {B: b_list(rng, np.sort(perm(core)))}
    for t, n in sizes.items():
        f0[t] = np.union1d(rng.choice(N0, size=n, replace=False), core)
        f1[t] = np.sort(perm(f0[t]))
    return [f0, f1]


class World:
    def __init__(self, lib_path):
        self.model = [{}, {}]
        self._sorted = {}
        self.hot = [[], []]                 # ids around which the write rounds worked (the aux-score slice)
        self.facts = {}                     # coverage facts that only show WHILE the rounds run (a block's width before / after), read from the layout
        self._ref, self.seen = {}, {}
        self.pts = H.points_of(N_DOCS)
        from tests.test_emu_groupby import group_column
        self.distinct, self.has_value = group_column(N_DOCS, seed=3)
        self.g = g = T.GpuIndex(0, lib_path)
        g.set_option("index_min_slack_words", 1 << 22)            # tails large enough for every round, and
        g.set_option("index_compact_min_words", 1 << 26)          # garbage never outweighs this: no commit compacts
        lists = initial_lists()
        for f in FIELDS:
            g.field_create(f, False)
            terms = sorted(lists[f])
            ids = np.concatenate([lists[f][t] for t in terms]).astype(np.uint32)
            ptr = np.zeros(len(terms) + 1, np.uint64)
            ptr[1:] = np.cumsum([lists[f][t].size for t in terms])
            g.terms_load_csr(f, np.array(terms, np.uint32), ptr, ids, np.arange(ids.size, dtype=np.uint64), ptr, pos_of(ids))
            for t in terms:
                self.model[f][t] = {int(d): (int(p),) for d, p in zip(lists[f][t], pos_of(lists[f][t]))}
        g.column_set(0, self.pts)
        g.column_set(GROUP_COL, self.distinct.view(np.int64))
        g.set_num_docs(N_DOCS)
        g.commit()
        assert g.counter("commit_full_count") == 1 and g.counter("commit_incremental_count") == 0
        self.orc = None
        self._round1()
        self.commit("round 1")
        self.check_round("round 1")
        for k in range(N_TINY):
            for f in FIELDS:
                for t in (A, B):
                    self.upsert(f, t, N0 + k)
            self.commit("append %d" % k, verify=(A, B))
        self._round2()
        self.commit("round 2")
        self.check_round("round 2")
        self._round3()
        self.commit("round 3")
        self.check_round("round 3")
        self._round4()
        self.commit("round 4")
        self.fresh_oracle()

    def close(self):
        self.g.close()
        if self.orc is not None:
            self.orc.close()

    # ---------------------------------------------------------------- model + library, one operation at a time
    def ids(self, f, t):
        if (f, t) not in self._sorted:
            self._sorted[(f, t)] = np.array(sorted(self.model[f].get(t, ())), np.int64)
        return self._sorted[(f, t)]

    def upsert(self, f, t, doc, offs=None):
        offs = tuple(int(x) for x in (offs if offs is not None else pos_of([doc])))
        self.g.posting_upsert(f, t, int(doc), np.array(offs, np.uint32))
        self.model[f].setdefault(t, {})[int(doc)] = offs
        self._sorted.pop((f, t), None)

    def erase(self, f, t, doc):
        self.g.posting_erase(f, t, int(doc))
        lst = self.model[f].get(t)
        if lst is not None and int(doc) in lst:
            del lst[int(doc)]
            if not lst:
                del self.model[f][t]
            self._sorted.pop((f, t), None)

    def arrays(self, f, t, only=None):
        ids = self.ids(f, t)
        if only is not None:
            ids = ids[np.isin(ids, only)]
        lst = self.model[f][t]
        runs = [lst[d] for d in ids.tolist()]
        oi = np.zeros(ids.size, np.uint32)
        if ids.size:
            oi[1:] = np.cumsum([len(r) for r in runs])[:-1]
        return ids.astype(np.uint32), oi, np.fromiter(itertools.chain.from_iterable(runs), np.uint32)

    def commit(self, what, verify=None):
        g = self.g
        inc, full = g.counter("commit_incremental_count"), g.counter("commit_full_count")
        g.commit()
        assert g.counter("commit_incremental_count") == inc + 1, "%s: the commit was not incremental" % what
        assert g.counter("commit_full_count") == full == 1 and g.counter("commit_compactions") == 0, what
        self.verify_lists(what, verify)

    def verify_lists(self, what, terms=None):
        """every list round-trips through term_download equal to the model"""
        for f in FIELDS:
            for t in (terms or NAMES):
                if t not in self.model[f]:
                    assert self.g.term_num_ids(f, t) == 0, (what, f, NAMES[t])
                    continue
                ids, oi, off = self.arrays(f, t)
                gi, go, gf = self.g.term_download(f, t)
                assert np.array_equal(ids, gi) and np.array_equal(oi, go) and np.array_equal(off, gf), "%s: field %d list %s differs from the model" % (what, f, NAMES[t])

    def fresh_oracle(self):
        if self.orc is not None:
            self.orc.close()
        self.orc = orc = O.OracleIndex(2, 1)
        for f in FIELDS:
            for t in self.model[f]:
                orc.load_posting(f, t, *self.arrays(f, t))
        orc.set_num_docs(N_DOCS)
        orc.set_sort_dense(0, self.pts)
        self._ref = {}
        return orc

    def check_round(self, what):
        """a handful of queries against a fresh oracle after every round (the bodies run after the last one)"""
        self.fresh_oracle()
        qs = [kwq(t) for t in ([R, D], [S, B], [A, B], [S, A, D], [A, B, D], [R, S, A, B], [B])] + [kwq([A, D], fields=[(1, 15)]), kwq([S, B, D], fields=[(0, 15), (1, 10)])]
        check_queries(self, qs, what)

    def layout(self, f, t):
        L = self.g.term_blocks(f, t)
        L["start"] = np.concatenate([[0], np.cumsum(L["n_ids"])]).astype(np.int64)
        L["ids"] = self.ids(f, t)                                       # (as committed: later operations replace the model's array, not this one)
        assert int(L["start"][-1]) == L["ids"].size and np.array_equal(L["ids"][L["start"][:-1]], L["first_id"])      # no operation of this round touched the list yet
        return L

    def block(self, f, t, L, b):
        return L["ids"][int(L["start"][b]):int(L["start"][b + 1])]

    def free_id(self, f, t, lo, hi):
        """an id in (lo, hi) the list does not hold"""
        have = self.model[f][t]
        for x in range(int(lo) + 1, int(hi)):
            if x not in have:
                return x
        raise AssertionError("no free id in (%d, %d) of %s" % (lo, hi, NAMES[t]))

    # ---------------------------------------------------------------- the write rounds
    def _round1(self):
        for f in FIELDS:
            lay = {t: self.layout(f, t) for t in NAMES}
            gaps = {}
            for t in (D, B, A):
                L = lay[t]
                nb = L["n_ids"].size
                full = [b for b in range(2, nb - 2) if L["n_ids"][b] == 256]
                mids = {b: self.block(f, t, L, b)[127:129] for b in full}
                wide = sorted([b for b in full if mids[b][1] - mids[b][0] >= 4], key=lambda b: abs(int(mids[b][0]) - ZC))
                b = wide[0]
                new = int(mids[b][1]) - 1                               # the right half's first id; (left half's last id, new) stays empty
                gaps[t] = list(range(int(mids[b][0]) + 1, new))
                self.upsert(f, t, new)
                self.hot[f] += [int(mids[b][0]), new]
                used = {b}
                if t == D:                                             # three more halves of 128 for round 2 to erase from
                    for b2 in sorted(full, key=lambda b: abs(int(mids[b][0]) - ZC)):
                        if all(abs(b2 - u) >= 2 for u in used) and len(used) < 4:
                            ids = self.block(f, t, L, b2)
                            self.upsert(f, t, self.free_id(f, t, ids[0], ids[255]))
                            used.add(b2)
                    assert len(used) == 4
                if t == B:                                             # seven neighbours split in one commit: 14 part-filled blocks, contiguous at the tail
                    b0 = next(b for b in range(nb * 3 // 5, nb - 9) if all(L["n_ids"][b + i] == 256 and abs(b + i - u) >= 2 for i in range(7) for u in used))
                    for i in range(7):
                        ids = self.block(f, t, L, b0 + i)
                        self.upsert(f, t, self.free_id(f, t, ids[100], ids[255]))
                    self.facts[(f, "b_run_first")] = int(self.block(f, t, L, b0)[0])
            for t, gap in gaps.items():                                # the other lists' ids inside the gap between the two halves
                for o in NAMES:
                    if o != t:
                        for x in gap[:2]:
                            self.upsert(f, o, x)
            # the block behind either hole of B gets an id at the hole's start: its ids need 32 bits
            for k, (lo, hi) in enumerate(HOLES):
                first_behind = int(self.ids(f, B)[np.searchsorted(self.ids(f, B), hi)])
                self.facts[(f, "wide", k)] = (lo + 1, first_behind)
                self.upsert(f, B, lo + 1)
                self.hot[f].append(lo + 1)
            # first and last block of every list
            for t in NAMES:
                ids = self.ids(f, t)
                if t in (D, B, A):
                    self.erase(f, t, ids[0])
                else:
                    self.upsert(f, t, self.free_id(f, t, -1, ids[0]) if ids[0] > 0 else self.free_id(f, t, ids[0], ids[1]))
                L = lay[t]
                last = self.block(f, t, L, L["n_ids"].size - 1)
                self.upsert(f, t, self.free_id(f, t, last[0], last[-1]))
            # a run replaced in place by one of another length; erases of ids that are absent (inside a block, between two blocks, beyond the list, a term that is not there)
            doc = int(self.ids(f, A)[3000])
            self.upsert(f, A, doc, (2, 5, 9))
            self.hot[f].append(doc)
            self.erase(f, B, self.free_id(f, B, self.ids(f, B)[5000], self.ids(f, B)[5300]))
            self.erase(f, B, HOLES[0][0] + 500)
            self.erase(f, S, N_DOCS - 1)
            self.erase(f, 99, 17)

    def _round2(self):
        for f in FIELDS:
            # widths read from the layout: both blocks behind a hole are 32-bit now; the erase below narrows the second one back
            one_of_128 = {}                                            # (every layout is read before the round's first operation)
            for t in (A, B):
                L = self.layout(f, t)
                b = next(b for b in range(2, L["n_ids"].size - N_TINY - 2) if 128 <= L["n_ids"][b] <= 136)      # a half round 1 left
                one_of_128[t] = self.block(f, t, L, b)[5:5 + int(L["n_ids"][b]) - 127]
            L = self.layout(f, B)
            for k in (0, 1):
                new, _ = self.facts[(f, "wide", k)]
                b = int(np.nonzero(L["first_id"] == new)[0][0])
                self.facts[(f, "widened", k)] = int(L["ids_bits"][b]) == 32 and int(L["last_id"][b]) - new > 65535
            self.erase(f, B, self.facts[(f, "wide", 1)][0])
            # erases that leave 1, 2 and 127 ids in a block and that empty one: the halves round 1 left (read from the layout; not the list's ends)
            L = self.layout(f, D)
            halves = [b for b in range(2, L["n_ids"].size - 2) if 120 <= L["n_ids"][b] <= 136]
            assert len(halves) >= 6, halves
            picked = []
            for b in halves:                                           # no two neighbours: a block that disappears must not make two one-id blocks adjacent by accident
                if all(abs(b - p) >= 2 for p in picked) and len(picked) < 4:
                    picked.append(b)
            for b, keep in zip(picked, (1, 2, 127, 0)):
                ids = self.block(f, D, L, b)
                for x in ids[keep:] if keep != 1 else np.concatenate([ids[:60], ids[61:]]):     # (the one id left is from the block's middle)
                    self.erase(f, D, x)
                self.hot[f].append(int(ids[60]))
            for t, xs in one_of_128.items():
                for x in xs:
                    self.erase(f, t, x)
            # appends behind the one-id blocks; the tail ids into S in ONE block; R leaves the index
            for d in range(N0 + N_TINY, N0 + N_TINY + 7):
                self.upsert(f, A, d)
                self.upsert(f, B, d)
            for d in range(N0, N0 + N_TINY + 8):
                self.upsert(f, S, d)
            for x in self.ids(f, R):
                self.erase(f, R, x)
            assert R not in self.model[f]
            self.hot[f] += [N0, N0 + N_TINY]

    def _round3(self):
        rng = np.random.default_rng(43)
        for f in FIELDS:
            old = initial_lists()[f][R]
            new = np.union1d(np.union1d(old[::2], rng.choice(N0, size=200, replace=False)), np.arange(N0, N0 + N_TINY + 12))
            new = np.union1d(new, self.ids(f, S)[::9])                 # (shares ids with S beyond the core)
            for x in new:
                self.upsert(f, R, x)
            for t in (A, B):
                for d in range(N0 + N_TINY + 7, N0 + N_TINY + 16):
                    self.upsert(f, t, d)
            self.erase(f, A, N0 + 5)                                   # a one-id block disappears
            self.upsert(f, D, N0 + 2)

    def _round4(self):
        for f in FIELDS:
            ids = self.ids(f, R)
            for i in (40, 200, 300):
                self.upsert(f, R, self.free_id(f, R, ids[i], ids[i + 1] + 3))
            s = self.ids(f, S)
            self.upsert(f, S, self.free_id(f, S, s[10], s[11] + 3))
            self.upsert(f, TT, N0 + 3)
            self.upsert(f, U, N0 + 3)

    # ---------------------------------------------------------------- references
    def oracle(self, q, tag=None):
        key = (tuple(q.tokens), tuple(q.fields), tag)
        if key not in self._ref:
            self._ref[key] = H.oracle_keyword(self.orc, q, cap=2048, ids_cap=IDS_CAP)
        return self._ref[key]


def kwq(tokens, fields=((0, 15),), **kw):
    return T.KwQuery(tokens, sort=SORT, topster_size=K, fields=fields, **kw)


# ---------------------------------------------------------------- coverage conditions: computed from the downloaded layout, never assumed
def coverage(w):
    g = w.g
    assert g.counter("index_used_words") > g.counter("index_live_words")
    assert g.counter("commit_full_count") == 1 and g.counter("commit_incremental_count") >= 3 + N_TINY
    w.verify_lists("coverage")
    out = {}
    for f in FIELDS:
        lay = {t: g.term_blocks(f, t) for t in MAIN}
        fills, mixed, tiny_run, part_run = set(), [], {}, 0
        for t in (A, B, D, S):
            L = lay[t]
            n, nb = L["n_ids"], L["n_ids"].size
            assert L["has_breaks"], "field %d list %s has no break" % (f, NAMES[t])
            assert np.array_equal(L["last_id"], w.ids(f, t)[np.cumsum(n) - 1]) and (L["first_id"][1:] > L["last_id"][:-1]).all()
            fills.update(int(x) for x in n[1:-1])
            assert (np.where(L["last_id"] - L["first_id"] > 65535, 32, 16) == L["ids_bits"]).all()
            if {16, 32} <= set(L["ids_bits"].tolist()):
                mixed.append(NAMES[t])
            # the list's first block was re-written: it lives behind blocks that were never moved
            assert L["arena_pos"][0] > L["arena_pos"][1:].min(), "field %d list %s: first block not relocated" % (f, NAMES[t])
            words = np.where(L["ids_bits"] == 16, (n + 1) // 2, n) + 1          # packed_words(n, bits)
            contiguous = L["arena_pos"][1:] == L["arena_pos"][:-1] + words[:-1]
            # longest run of consecutive blocks inside ONE block's id range of another (shorter: a driver) list, (a) of blocks of <= 2 ids, (b) of part-filled
            # blocks with no break between them
            for o in (R, S, A):
                if o == t or len(w.model[f][o]) >= len(w.model[f][t]):
                    continue
                for lo, hi in zip(lay[o]["first_id"], lay[o]["last_id"]):
                    inside = (L["first_id"] >= lo) & (L["last_id"] <= hi)
                    run_a = run_b = 0
                    for b in range(1, nb - 1):
                        run_a = run_a + 1 if inside[b] and n[b] <= 2 else 0
                        run_b = run_b + 1 if inside[b] and 2 < n[b] < 256 and (run_b == 0 or contiguous[b - 1]) else 0
                        tiny_run[t] = max(tiny_run.get(t, 0), run_a)
                        part_run = max(part_run, run_b)
        assert {1, 2, 127, 128, 256} <= fills, (f, sorted(fills))
        assert "B" in mixed and "S" in mixed, (f, mixed)                   # 16- and 32-bit blocks inside one list with breaks
        assert tiny_run[A] >= N_TINY - 1 and tiny_run[B] >= N_TINY, (f, tiny_run)     # (A lost one of its 14 in round 3: a block that disappeared)
        assert tiny_run[B] - 1 > F2_SPAN and part_run - 1 > F2_SPAN, (f, tiny_run, part_run)
        assert w.facts[(f, "widened", 0)] and w.facts[(f, "widened", 1)], "the blocks behind B's holes never became 32-bit"
        LB = lay[B]
        new0, _ = w.facts[(f, "wide", 0)]
        _, behind1 = w.facts[(f, "wide", 1)]
        assert int(LB["ids_bits"][int(np.nonzero(LB["first_id"] == new0)[0][0])]) == 32            # still wide ...
        assert int(LB["ids_bits"][int(np.nonzero(LB["first_id"] == behind1)[0][0])]) == 16         # ... and narrowed back
        assert all(g.term_blocks(f, t)["has_dir"] for t in (D, B, A)) and not lay[S]["has_dir"]
        assert g.term_blocks(f, R)["has_breaks"]
        out[f] = dict(fills=sorted(fills), tiny_run=tiny_run, part_run=part_run, blocks={NAMES[t]: int(lay[t]["n_ids"].size) for t in MAIN})
    return out


# ---------------------------------------------------------------- query sets
TOKEN_SETS = [[D], [B], [A], [S], [R],
              [R, D], [D, S], [A, B], [B, D], [S, R], [R, A], [S, A], [S, B], [R, B], [A, D], [TT, R], [U, S],
              [R, S, D], [A, B, D], [R, A, B], [S, R, A], [D, B, S], [TT, R, S], [U, TT, R], [S, A, B],
              [R, S, A, B], [S, A, B, D], [TT, R, S, A], [U, TT, R, D],
              [R, S, A, B, D, TT], [U, TT, R, S, A, B], [D, B, A, S, R, U]]


# the emulator tier's thinner grid: every option still meets a driver against broken / part-filled / one-id / 32-bit second lists, third lists, 4 and 6 tokens
THIN_SETS = [[B], [R, D], [D, S], [A, B], [B, D], [S, A], [S, B], [R, B], [TT, R], [R, S, D], [A, B, D], [R, A, B], [TT, R, S], [S, A, B, D], [R, S, A, B, D, TT]]


def roles(w, f=0):
    """{list: set of positions it takes in the planner's order (by length, from the MODEL's lengths)}"""
    lens = {t: len(w.model[f][t]) for t in NAMES}
    assert len(set(lens.values())) == len(lens)
    assert lens[U] < lens[TT] < lens[R] < lens[S] < lens[A] < lens[B] < lens[D], lens
    seen = {t: set() for t in NAMES}
    for ts in TOKEN_SETS:
        assert len(ts) in (1, 2, 3, 4, 6)
        for i, t in enumerate(sorted(ts, key=lambda t: lens[t])):
            seen[t].add(min(i, 2))
    return seen


def filter_sets():
    filt = np.union1d(np.arange(0, N0, 3), np.arange(N0, N0 + 40)).astype(np.uint32)
    excl = np.union1d(np.arange(1, N0, 4), np.arange(N0 + 1, N0 + 30, 2)).astype(np.uint32)
    return filt, excl


def single_field_queries(f=0, token_sets=None):
    filt, excl = filter_sets()
    ts = token_sets or TOKEN_SETS
    qs = [(kwq(t, [(f, 15)]), None) for t in ts]
    qs += [(kwq(t, [(f, 15)], filter_ids=filt), "filter") for t in ts[5::2]]
    qs += [(kwq(t, [(f, 15)], excluded_ids=excl), "excluded") for t in ts[6::2]]
    return qs


def check_queries(w, qs, what, batch=64, remember=None, keep_ids=True):
    """every hit of every query, num_matched and the result ids against the oracle; remember: also against / into what this body returned before"""
    qs = [q if isinstance(q, tuple) else (q, None) for q in qs]
    w.g.keep_result_ids(keep_ids)
    try:
        n_hits = 0
        for lo in range(0, len(qs), batch):
            part = qs[lo:lo + batch]
            hits = w.g.keyword_search_batch([q for q, _ in part], k_stride=K)
            assert (hits.status == 0).all(), (what, hits.status)
            for i, (q, tag) in enumerate(part):
                ref = w.oracle(q, tag)
                label = "%s %s fields %s %s" % (what, [NAMES.get(t, t) for t in q.tokens], q.fields, tag or "")
                H.assert_hits_equal(hits, i, ref, label)
                assert ref.n_result_ids <= IDS_CAP and (not keep_ids or np.array_equal(w.g.result_ids(i), ref.result_ids)), label + ": result ids"
                n_hits += ref.keys.size
            if remember is not None:
                got = [(hits.keys[i, :int(hits.n_hits[i])].copy(), hits.scores[i, :int(hits.n_hits[i])].copy(), int(hits.num_matched[i])) for i in range(len(part))]
                before = w.seen.setdefault((remember, lo), got)
                for a, b in zip(before, got):
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], what + ": results changed"
        return n_hits
    finally:
        w.g.keep_result_ids(False)


class options:
    """set for the body, put back afterwards: {name: (value, default)}"""

    def __init__(self, w, opts):
        self.w, self.opts = w, opts

    def __enter__(self):
        for name, (v, _) in self.opts.items():
            self.w.g.set_option(name, v)

    def __exit__(self, *a):
        for name, (_, back) in self.opts.items():
            self.w.g.set_option(name, back)


OPTION_SETS = {
    "default": {},
    "chunk1": {"kw_chunk_blocks": (1, 0)},
    "chunk3": {"kw_chunk_blocks": (3, 0)},
    "fused": {"kw_two_kernels": (0, 1)},
    "fused_chunk1": {"kw_two_kernels": (0, 1), "kw_chunk_blocks": (1, 0)},
    "fused_chunk3": {"kw_two_kernels": (0, 1), "kw_chunk_blocks": (3, 0)},
    "one_block_find": {"kw_pair_blocks": (0, 1)},
    "one_block_find_chunk1": {"kw_pair_blocks": (0, 1), "kw_chunk_blocks": (1, 0)},
    "one_block_find_chunk3": {"kw_pair_blocks": (0, 1), "kw_chunk_blocks": (3, 0)},
    "device_plan": {"kw_device_plan_min_queries": (1, 512)},
    "device_plan_chunk3": {"kw_device_plan_min_queries": (1, 512), "kw_chunk_blocks": (3, 0)},
}


# ---------------------------------------------------------------- bodies
def body_coverage(w):
    c = coverage(w)
    seen = roles(w)
    for t in MAIN:
        assert seen[t] == {0, 1, 2}, (NAMES[t], seen[t])       # driver, second list, third-or-later list
    return c


def body_single_field(w, name, f=0, token_sets=None):
    opts = OPTION_SETS[name]
    plans = w.g.counter("kw_device_plans")
    with options(w, opts):
        if "kw_device_plan_min_queries" in opts:               # the device-side planner takes batches of plain queries only
            qs = [q for q in single_field_queries(f, token_sets) if q[1] is None]
            n = check_queries(w, qs, name, remember=("plain", f, token_sets is None), keep_ids=False)      # (... and none whose ids are read back per query)
            assert w.g.counter("kw_device_plans") > plans, "the batch was not planned on the device"
        else:
            n = check_queries(w, single_field_queries(f, token_sets), name, remember=("single", f, token_sets is None))
    assert n >= 1000, (name, n)


def body_two_fields(w, pipelined, chunk=0, token_sets=None):
    ts = token_sets or [t for t in TOKEN_SETS if len(t) <= 4]
    filt, excl = filter_sets()
    qs = [kwq(t, [(0, 15), (1, 10)]) for t in ts] + [kwq(t, [(1, 15), (0, 3)]) for t in ts]
    qs += [(kwq(t, [(0, 15), (1, 10)], filter_ids=filt), "filter") for t in ts[5::4]] + [(kwq(t, [(1, 15), (0, 3)], excluded_ids=excl), "excluded") for t in ts[6::4]]
    launches = w.g.counter("kw_mf_pipelined_launches")
    with options(w, {"kw_mf_pipelined": (pipelined, 1), "kw_chunk_blocks": (chunk, 0)}):
        n = check_queries(w, qs, "two fields pipelined=%d chunk=%d" % (pipelined, chunk), remember=("two fields", token_sets is None))
    assert (w.g.counter("kw_mf_pipelined_launches") > launches) == bool(pipelined)
    assert n >= 1000, n


def body_grouped(w, first_pass, token_sets=None):
    from tests.test_emu_groupby import check_query, oracle_grouped
    ts = token_sets or [[A], [R, D], [A, B], [S, A], [B, D], [A, B, D], [S, R, A], [R, S, A, B], [U, TT, R, S, A, B]]
    qs = [kwq(t) for t in ts] + [kwq(t, [(1, 15)]) for t in ts[1::2]]
    limit = 3
    h, gh = w.g.keyword_search_grouped_batch(qs, [(limit, GROUP_COL, int(first_pass), 0, 0)] * len(qs), k_stride=K * limit, g_stride=K)
    groups = 0
    for i, q in enumerate(qs):
        ref = oracle_grouped(w.orc, q, w.distinct, w.has_value, limit, bool(first_pass))
        check_query(h, gh, i, ref, bool(first_pass), limit, "grouped %s fields %s" % (q.tokens, q.fields))
        groups += ref.n_groups
    assert groups >= 100, groups
    got = (h.keys.copy(), gh.distinct_key.copy(), gh.n_groups.copy())
    before = w.seen.setdefault(("grouped", first_pass, token_sets is None), got)
    assert all(np.array_equal(a, b) for a, b in zip(before, got)), "grouped results changed"


def body_candidates(w):
    """candidate combinations: the combinations of a user query share mutated lists (one id pass per distinct list)"""
    filt, _ = filter_sets()
    groups = [[kwq([A, B]), kwq([A, D]), kwq([S, B])],
              [kwq([R, D]), kwq([R, B]), kwq([S, D]), kwq([S, R])],
              [kwq([S, A, B]), kwq([S, A, D]), kwq([R, A, B]), kwq([A, B, D])],
              [kwq([B, D]), kwq([A]), kwq([S])],
              [kwq([R, S, A, B]), kwq([S, A, B, D]), kwq([A, B], fields=[(0, 15)])],
              [kwq([A, B], [(1, 15)]), kwq([S, B], [(1, 15)]), kwq([S, A, B], [(1, 15)])],
              [kwq([A, B], filter_ids=filt), kwq([S, B], filter_ids=filt), kwq([S, D], filter_ids=filt)]]
    hits, qidx, found = w.g.keyword_search_candidates_batch(groups, k_stride=K)
    assert (hits.status == 0).all()
    multi = 0
    for gi, combos in enumerate(groups):
        ref, ref_qi = H.oracle_candidates(w.orc, combos, cap=2048, ids_cap=IDS_CAP)
        H.assert_hits_equal(hits, gi, ref, "candidates g%d" % gi)
        n = int(hits.n_hits[gi])
        assert np.array_equal(qidx[gi, :n], ref_qi), "g%d query_index" % gi
        assert int(found[gi]) == int(ref.n_result_ids) <= IDS_CAP and np.array_equal(w.g.candidates_result_ids(gi), ref.result_ids), gi
        multi += int(len(set(ref_qi.tolist())) > 1)
    assert multi >= 3
    got = (hits.keys.copy(), hits.scores.copy(), qidx.copy(), found.copy())
    before = w.seen.setdefault("candidates", got)
    assert all(np.array_equal(a, b) for a, b in zip(before, got)), "candidates results changed"


def aux_slice(w):
    """2 000 ids: windows around the ids the write rounds worked at (split points, the gaps between the halves, the holes' ends, erased blocks, the tail)"""
    hot = sorted(set(w.hot[0] + w.hot[1]))
    tail = np.arange(N0, N0 + 40)
    windows = lambda width: np.setdiff1d(np.unique(np.concatenate([np.arange(max(h - width, 0), min(h + width, N0)) for h in hot])), tail)
    width = 1
    while windows(width + 1).size <= 1960:                            # the widest windows that fit; the rest is filled up with ids next to the first one
        width += 1
    ids = np.union1d(windows(width), tail)
    fill = np.setdiff1d(np.arange(hot[0] + width, hot[0] + width + 4000), ids)[:2000 - ids.size]
    return np.union1d(ids, fill).astype(np.uint32)


def body_aux_scores(w):
    """tsgpu_keyword_aux_scores (probe_list on broken lists, with and without directory) over EVERY (query, document) pair of the slice vs
    Index::compute_aux_scores: an oracle that holds the model's postings of the slice's documents and one vector per document — the vector half of a
    hybrid search returns every document, so each one the keyword half did not find gets compute_text_match_aux_score's value"""
    ids = aux_slice(w)
    n = ids.size
    assert n == 2000
    orc = O.OracleIndex(2, 1)
    for f in FIELDS:
        for t in w.model[f]:
            a = w.arrays(f, t, only=ids)
            if a[0].size:
                orc.load_posting(f, t, *a)
    orc.set_num_docs(N_DOCS)
    orc.set_sort_dense(0, w.pts)
    X = np.random.default_rng(5).standard_normal((n, 4)).astype(np.float32)
    orc.vec_init(4, O.METRIC_IP)
    orc.vec_add(ids, X)
    sets = [[R, D], [A, B], [S, A, D], [A, B, D], [R, S, A, B], [D, B, A, S, R, U], [B, D], [S, R, A]]
    partial = 0
    for fields in ([(0, 15)], [(1, 15)], [(0, 15), (1, 10)]):
        qs = [kwq(t, fields, prioritize_token_position=bool(i % 2)) for i, t in enumerate(sets)]
        got = w.g.keyword_aux_scores(qs, np.repeat(np.arange(len(qs), dtype=np.uint32), n), np.tile(ids, len(qs))).reshape(len(qs), n)
        for i, q in enumerate(qs):
            big = T.KwQuery(q.tokens, sort=SORT, topster_size=2048, fields=q.fields, prioritize_token_position=q.prioritize_token_position)     # (the oracle's collector holds every document)
            ref = orc.search_hybrid(H.oracle_query(orc, big), X[0], k=n, alpha=0.3, rerank=True, cap=2048)
            assert ref.keys.size == n
            want = np.zeros(n, np.int64)
            want[np.searchsorted(ids, ref.keys.astype(np.int64))] = ref.text_match
            bad = np.nonzero(got[i] != want)[0]
            assert bad.size == 0, "aux %s fields %s: %d documents differ, first %d: %x vs oracle %x" % (q.tokens, fields, bad.size, ids[bad[0]], got[i][bad[0]], want[bad[0]])
            partial += int((want != 0).sum())
        before = w.seen.setdefault(("aux", tuple(fields)), got.copy())
        assert np.array_equal(before, got), "aux scores changed"
    orc.close()
    assert partial >= 2000, partial


def body_directories_off(w, token_sets=None):
    """kw_iddir_min_ids = 0 asks for a full commit (the option re-decides every list); withdrawn (commit_full = 0) the commit stays incremental and only
    drops the directories: the broken lists are probed by the two-level search alone. Put back the same way."""
    g = w.g
    assert g.counter("kw_iddir_lists") >= 6
    try:
        g.set_option("kw_iddir_min_ids", 0)
        g.set_option("commit_full", 0)
        w.commit("directories off")                                  # (nothing to write: the snapshot's lists stay where they are)
        assert g.counter("kw_iddir_lists") == 0 and not g.term_blocks(0, D)["has_dir"] and g.term_blocks(0, D)["has_breaks"]
        n = check_queries(w, single_field_queries(0, token_sets), "directories off", remember=("single", 0, token_sets is None))
        n += check_queries(w, [kwq(t, [(0, 15), (1, 10)]) for t in (token_sets or TOKEN_SETS)[5:29:2]], "directories off, two fields")
        assert n >= 1000
    finally:
        g.set_option("kw_iddir_min_ids", 256)
        g.set_option("commit_full", 0)
        w.commit("directories on")
    assert g.counter("kw_iddir_lists") >= 6 and g.term_blocks(0, D)["has_dir"]


def compact(w):
    g = w.g
    g.set_option("commit_full", 1)
    g.commit()
    assert g.counter("commit_full_count") == 2
    assert g.counter("index_used_words") == g.counter("index_live_words")
    for f in FIELDS:
        for t in w.model[f]:
            L = g.term_blocks(f, t)
            assert not L["has_breaks"] and (L["n_ids"][:-1] <= 256).all(), (f, NAMES[t])
    w.verify_lists("after the compaction")
