"""Shared bodies of tests/test_emu_scoring_shapes.py (CPU tier, SIMT emulator) and tests/test_gpu_scoring_shapes.py (-m gpu, libtsgpu.so): the
code that turns packed offsets into a text_match score (load_run / load_runs_staged / load_runs_staged_slots, run_raw / run_pos, match_window<TMAX>,
field_match_score, field_match_score_array and the three string[] readers of typesense_amd/csrc/kw_kernels.hip.h) on document shapes the Zipf corpora
of the other tiers never produce. One crafted corpus of N_DOCS documents, the same content in the oracle and in a GpuIndex:

  field 0  plain string, the documents below                          field 1  plain string, the same documents permuted over the seq_ids
  field 2  string[] (a subset of the documents holds an array)

  A  long documents (~70 000 tokens, one filler token nearly everywhere: runs of tens of thousands of elements, offsets that need 17 bits, query tokens
     around positions 65533..65537, tokens on one side of 65536 only, positions that collide after the uint16 narrowing of posting_list.cpp:906)
  B  a query token 3 / 17 / 64 / 300 times in a document, the other tokens next to its LAST occurrence or to a middle one
  C  256 consecutive ids of one list with the token once, at the same position, never last (offsets of the block all equal); a list of exactly 257 ids
  D  the exact-match rule of Match (match_score.h:245-273): document = query, + trailing token, one token doubled, reversed, single token, single token twice
  E  the first and only window at positions 254 / 255 / 256 / 300; a single token whose last position is 255 / 256 / 511 / 512
  F  two and three tokens at gaps of exactly 9 / 10 / 11; documents where a token occurs 1 / 2 / 5 times for the queries that repeat a token
  G  arrays with elements up to index 300, a token twice in one element, a token ending three elements, a token in 50 elements, single-token elements,
     a one-element array, elements whose tokens sit past position 255 (the clamps through field_match_score_array)
  H  short random documents over the query tokens (the bulk of the multi-token hits, many proximity values)

Query tokens are the ids 1..10 and 11 (found beyond position 65535 only); fillers are ids >= 100. The long documents' filler (id 100) is queried too: only
then does a kernel walk a run of tens of thousands of elements. Every hit of every query is compared (topster_size = k_stride = K >= the number of documents).

The coverage conditions (coverage_of_lists / coverage_of_scores) are computed from the downloaded posting lists and from the ORACLE's text_match values,
never from the code under test: the tests fail when the corpus stops reaching the paths it was built for."""
import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O
from tests import helpers as H

F_PLAIN, F_PERM, F_ARR = 0, 1, 2
GROUP_COL = 1
FILL = 100                  # the long documents' filler (queried)
K = 1000                    # topster_size = k_stride >= N_DOCS: no hit is left out
SORT = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_SEQ_ID, 1, 0))
LONG_LEN = 70000
BEYOND = 11                 # a token that occurs beyond position 65535 only (long documents): a block of few bits per offset whose values all exceed 16 bits


def _fillers(n, salt):
    """n filler tokens 101.. (never the queried filler)"""
    return [101 + (salt * 7 + i * 3) % 37 for i in range(n)]


def _placed(length, places, filler=None, salt=0):
    """a document of `length` tokens: places = {position: token}, fillers elsewhere"""
    d = np.full(length, filler, np.uint32) if filler is not None else np.array(_fillers(length, salt), np.uint32)
    for p, t in places.items():
        d[p] = t
    return d


def family_a():
    docs = []
    # query tokens 1..5 on positions 65533..65537 (stored 65534..65538: the 16-bit cache guard, run_pos at raw 65535 / 65536 / 65537), 1 also early
    docs.append(_placed(LONG_LEN, {10: 1, 65533: 1, 65534: 2, 65535: 3, 65536: 4, 65537: 5, 69999: 6, 65540: BEYOND, 65543: BEYOND, 65544: 1}, FILL))
    # 1 only before 65536, 2 only after; 3 at 65534 and 65536 (first stored element < 65536, second >= 65536); 5 straddles (65530 -> 65540 narrows DOWN: the
    # wrap-around exit of match_score.h:164-167 against 1 or 4); 7 at 5 and 65541 (the later position EQUALS the earlier one after narrowing)
    docs.append(_placed(LONG_LEN, {50: 1, 40000: 1, 65600: 2, 69990: 2, 65534: 3, 65536: 3, 65530: 5, 65540: 5, 65532: 4, 5: 7, 65541: 7, 7: 8, 20: 8, 65543: 8, 65550: BEYOND, 65553: BEYOND, 65556: BEYOND, 65557: 2}, FILL))
    # 2 at 300 and 66000, 1 between 5's straddling pair, the document ends on a query token beyond 65536
    docs.append(_placed(LONG_LEN, {300: 2, 66000: 2, 65531: 1, 65529: 5, 65539: 5, 65535: 6, 65536: 7, 65537: 8, 65538: 4, 65540: 10, LONG_LEN - 1: 3, 66001: BEYOND}, FILL))
    # just over 65536 tokens: 1 at position 0 and 3 at 65536 (both 0 after narrowing), 2 on 65535, last token = 4
    docs.append(_placed(65540, {0: 1, 65535: 2, 65536: 3, 1: 5, 65537: 5, 65539: 4}, FILL))
    return docs


def family_b():
    docs = []
    for salt, n in enumerate((3, 17, 64, 300)):
        for where in ("last", "middle"):
            length = 12 * n + 8
            places = {12 * i: 1 for i in range(n)}
            at = 12 * ((n - 1) if where == "last" else n // 2)
            places[at + 1], places[at + 2] = 2, 3
            if n == 17:
                places[at + 4] = 4
            docs.append(_placed(length, places, salt=salt))
    return docs


def family_c():
    """the FIRST 256 documents = the first block of list 9: token 9 once, at position 5, never the last token"""
    docs = []
    for i in range(256):
        places = {5: 9, 6 + i % 29: 1, 8 + (i * 7) % 31: 2}
        if i % 2:
            places[40 + i % 5] = 3
        if i % 5 == 0:
            places[46] = 4
        docs.append(_placed(48, places, salt=i))
    return docs


def family_d():
    docs = []
    for q in ([1, 2], [1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4, 5], list(range(1, 11))):
        docs += [q, q + [FILL + 1], [q[0]] + q, q[:-1] + [q[-1], q[-1]], q[::-1], q[:1] + [q[1], q[1]] + q[2:]]
    docs += [[9, 1, 110, 2, 9], [4], [4, 4], [6], [6, 6], [1], [1, 1], [FILL], [2, 2, 2], [2, 2], [1, 2, 1]]
    return [np.array(d, np.uint32) for d in docs]


def family_e():
    docs = []
    for p in (254, 255, 256, 300):
        docs.append(_placed(p + 6, {p: 1, p + 1: 2, p + 2: 3}, salt=p))
        docs.append(_placed(p + 6, {p: 4, p + 2: 5}, salt=p + 1))
    for p in (255, 256, 511, 512):
        docs.append(_placed(p + 3, {p: 6}, salt=p))
        docs.append(_placed(p + 1, {3: 6, p: 6}, salt=p + 1))         # ... as the field's last token
        docs.append(_placed(p + 2, {p: 7, 0: 1}, salt=p + 2))
    return docs


def family_f():
    docs = []
    for g in (9, 10, 11):
        docs.append(_placed(g + 3, {0: 1, g: 2}, salt=g))
        docs.append(_placed(g + 3, {0: 2, g: 1}, salt=g + 1))
        docs.append(_placed(g + 5, {1: 1, 5: 2, 1 + g: 3}, salt=g + 2))
        docs.append(_placed(2 * g + 3, {0: 1, g: 2, 2 * g: 3}, salt=g + 3))
        docs.append(_placed(g + 3, {0: 3, 4: 1, g: 2}, salt=g + 4))
    for t in (1, 2):
        o = 3 - t
        docs.append(_placed(4, {1: t}))
        docs.append(_placed(4, {0: t, 2: o}))
        docs.append(_placed(6, {0: t, 1: t}))
        docs.append(_placed(16, {2: t, 14: t, 3: o}))
        docs.append(_placed(30, {0: t, 1: t, 5: t, 17: t, 29: t, 6: o}))
        docs.append(_placed(12, {0: t, 1: t, 2: t, 3: t, 4: t}))
        docs.append(_placed(40, {0: t, 11: t, 22: t, 33: t, 39: t, 23: o, 24: o}))
    return docs


def family_h(n, seed=21):
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        length = int(rng.integers(3, 41))
        d = np.array(_fillers(length, i), np.uint32)
        hot = rng.random(length) < (0.25 + 0.5 * (i % 3) / 2)
        d[hot] = rng.integers(1, 9 if i % 4 else 11, size=int(hot.sum()))
        if i % 6 == 0:
            d[rng.integers(0, length)] = FILL
        docs.append(d)
    return docs


def family_g(n_docs, seed=22):
    """{seq_id: [elements]} of the string[] field"""
    f = lambda i: 101 + i % 37
    arr = {}
    big = [[f(i)] for i in range(301)]                       # element indexes up to 300
    big[0], big[255], big[256], big[299], big[300] = [1, f(1), 2], [3, 1], [2, 1], [1, f(2), f(3), 2, 3], [1, 2, 3]
    arr[0] = big
    arr[1] = [[1, f(4), 1, 2], [f(5), f(6)], [2, 2, 1, 1]]                                   # a token twice inside one element
    arr[2] = [[f(7), 1], [2, 1], [f(8), f(9), 1], [1, f(10)], [3, 2]]                        # 1 ends three elements
    arr[3] = [([f(i), 1] if i % 3 else [1, f(i), 2]) if i % 10 else [2, f(i), f(i + 1), 1, 3] for i in range(50)]      # 1 in 50 elements
    arr[4] = [[4], [f(11)], [4]]                                                             # single-token elements equal to the query
    arr[5] = [[4]]
    arr[6] = [[1, 2, 3]]                                                                     # a one-element array
    arr[7] = [[f(12), 4], [4, 4]]
    arr[8] = [[3, 2, 1], [1, 2, 3, f(13)], [1, 2]]
    arr[9] = [[f(i)] * (i % 3) + [6] for i in range(300)]                                    # 6 in 300 elements, as each one's last token
    arr[10] = [list(range(1, 11)), list(range(10, 0, -1)), [1, 2, 3, 4, 5]]
    # positions past 255 INSIDE an element: the window's 255 clamp and the & 0xFF of the single-token path through field_match_score_array
    arr[12] = [[f(i) for i in range(260)] + [1, 2, 3], [f(i) for i in range(300)] + [4, f(1), 5]]
    arr[13] = [[f(i) for i in range(255)] + [6], [f(i) for i in range(256)] + [6, f(2)]]
    arr[14] = [[f(3)], [f(i) for i in range(511)] + [6]]
    arr[16] = [[f(i) for i in range(512)] + [6, 7]]
    rng = np.random.default_rng(seed)
    for d in range(11, n_docs, 4):
        elems = []
        for _ in range(int(rng.integers(1, 7))):
            length = int(rng.integers(1, 9))
            e = [int(t) for t in np.where(rng.random(length) < 0.6, rng.integers(1, 11, length), rng.integers(101, 110, length))]
            elems.append(e)
        arr[d] = elems
    return arr


class World:
    """the crafted corpus in the oracle and in a GpuIndex on `lib_path`"""

    def __init__(self, lib_path):
        docs = family_c() + family_a() + family_b() + family_e() + family_d() + family_f()
        docs += family_h(699 - len(docs))
        # the LAST document that holds token 10 = the one id of its list's last block: 10 at positions 65534 and 65535 (stored 65535 and 65536: one bit per
        # offset, the first element fits 16 bits, the second does not, and its low 16 bits read as the last-token flag)
        docs.append(_placed(65545, {3: 1, 65530: 2, 65534: 10, 65535: 10, 65541: BEYOND, 65542: BEYOND}, FILL))
        with_10 = sum(1 for d in docs if (d == 10).any())
        assert 0 < 257 - with_10 <= 256
        for i in range(257 - with_10):                         # list 10 holds exactly 257 ids: its last block is a block of ONE id (oi_bits == 0)
            assert docs[i].size == 48 and 10 not in docs[i] and docs[i][47] >= 100, i      # a family C document, a filler in its last position
            docs[i][47] = 10
        self.docs = docs
        self.n_docs = n = len(docs)
        self.perm = np.random.default_rng(7).permutation(n)
        self.arrays = family_g(n)
        self.orc = orc = O.OracleIndex(3, 2)
        for d in range(n):
            orc.index_plain(d, F_PLAIN, docs[d])
            orc.index_plain(d, F_PERM, docs[self.perm[d]])
        for d, elems in self.arrays.items():
            orc.index_array(d, F_ARR, elems)
        orc.set_num_docs(n)
        self.pts = H.points_of(n)
        orc.set_sort_dense(0, self.pts)
        self._ref = {}
        self.vectors = None
        from tests.test_emu_groupby import group_column
        self.distinct, self.has_value = group_column(n, seed=3)
        self.g = None
        if lib_path is None:                                   # the oracle's half alone (the coverage conditions hold without the library)
            return
        self.g = g = T.GpuIndex(0, lib_path)
        for f in (F_PLAIN, F_PERM, F_ARR):
            g.field_create(f, f == F_ARR)
            for term in orc.terms(f):
                ids, oi, off = orc.dump_posting(f, int(term))
                g.term_upsert(f, int(term), ids, oi, off)
        g.column_set(0, self.pts)
        g.column_set(GROUP_COL, self.distinct.view(np.int64))
        g.set_num_docs(n)
        g.commit()

    def close(self):
        if self.g is not None:
            self.g.close()
        self.orc.close()

    def oracle_vectors(self):
        """one 4-dimensional vector per document in the oracle, added once (keyword searches never read them)"""
        if self.vectors is None:
            self.vectors = np.random.default_rng(5).standard_normal((self.n_docs, 4)).astype(np.float32)
            self.orc.vec_init(4, O.METRIC_IP)
            self.orc.vec_add(np.arange(self.n_docs, dtype=np.uint32), self.vectors)
        return self.vectors

    def oracle(self, q):
        key = (tuple(q.tokens), tuple(q.fields), q.match_type, q.prioritize_exact_match, q.prioritize_token_position, q.total_cost)
        if key not in self._ref:
            self._ref[key] = H.oracle_keyword(self.orc, q, cap=2048)
        return self._ref[key]


TOKEN_SETS = [[1], [4], [6], [9], [10], [BEYOND], [FILL],
              [1, 2], [2, 1], [1, 1], [3, 4], [5, 1], [9, 1], [7, 1], [FILL, 1], [4, 5], [8, 8], [BEYOND, 1], [2, BEYOND], [10, 2],
              [1, 2, 3], [3, 2, 1], [1, 2, 1], [2, 2, 2], [3, 5, 1], [1, FILL, 2], [9, 2, 1], [6, 7, 8], [1, BEYOND, 2],
              [1, 2, 3, 4], [1, 2, 1, 3], [5, 7, 8, 1], [1, 2, 3, 4, 5], [5, 4, 3, 2, 1], [2, 1, FILL, 3, 5], list(range(1, 11)), [10, 8, 7, 6, 5, 4, 3, 2, 1, 1]]
# (prioritize_exact_match, prioritize_token_position, total_cost, match_type): every flag combination, both costs, both match types
FLAG_SETS = [(True, False, 0, B.MAX_SCORE), (True, True, 0, B.MAX_SCORE), (False, True, 0, B.MAX_SCORE), (False, False, 0, B.MAX_SCORE),
             (True, True, 3, B.MAX_SCORE), (True, False, 0, B.MAX_WEIGHT), (False, True, 3, B.MAX_WEIGHT)]


def queries(fields, token_sets=TOKEN_SETS, flag_sets=FLAG_SETS):
    return [T.KwQuery(t, sort=SORT, topster_size=K, fields=fields, prioritize_exact_match=pe, prioritize_token_position=pp, total_cost=cost, match_type=mt)
            for t in token_sets for pe, pp, cost, mt in flag_sets]


def check_queries(w, qs, what, batch=64):
    """every hit of every query against the oracle -> [(query, oracle hits)]"""
    out = []
    for lo in range(0, len(qs), batch):
        part = qs[lo:lo + batch]
        hits = w.g.keyword_search_batch(part, k_stride=K)
        assert (hits.status == 0).all(), (what, hits.status)
        for i, q in enumerate(part):
            ref = w.oracle(q)
            assert ref.keys.size < K
            H.assert_hits_equal(hits, i, ref, "%s %s pe=%d pp=%d cost=%d mt=%d" % (what, q.tokens, q.prioritize_exact_match, q.prioritize_token_position,
                                                                                 q.total_cost, q.match_type))
            out.append((q, ref))
    return out


# ---------------------------------------------------------------- coverage conditions
def required_bits(x):
    return int(x).bit_length()


def coverage_of_lists(w, field=F_PLAIN, terms=tuple(range(1, 11)) + (BEYOND, FILL)):
    """per 256-id block of the downloaded lists the width its offsets need, the sizes of the blocks and the runs"""
    widths, block_ids, run_lens, straddle, straddle16, high16 = set(), set(), set(), False, False, False
    for t in terms:
        ids, oi, off = w.g.term_download(field, t)
        ref_ids, ref_oi, ref_off = w.orc.dump_posting(field, t)
        assert np.array_equal(ids, ref_ids) and np.array_equal(oi, ref_oi) and np.array_equal(off, ref_off), "term %d round trip" % t
        ends = np.append(oi[1:], off.size).astype(np.int64)
        lens = ends - oi
        run_lens.update(int(x) for x in lens)
        two = np.nonzero(lens >= 2)[0]
        straddle = straddle or bool(((off[oi[two]] < 65536) & (off[oi[two] + 1] >= 65536)).any())
        for b in range(0, ids.size, 256):
            e = min(b + 256, ids.size)
            blk = off[int(oi[b]):int(ends[e - 1])]
            width = required_bits(int(blk.max()) - int(blk.min()))
            widths.add(width)
            block_ids.add(e - b)
            if width <= 16:                                    # the blocks whose runs the 16-bit register cache is tried on
                for i in np.nonzero(lens[b:e] >= 2)[0] + b:
                    first, second = int(off[oi[i]]), int(off[oi[i] + 1])
                    straddle16 = straddle16 or (first < 65536 <= second)
                    high16 = high16 or first >= 65536
    return dict(widths=widths, block_ids=block_ids, run_lens=run_lens, straddle=straddle, straddle16=straddle16, high16=high16)


def assert_list_coverage(c):
    assert 0 in c["widths"], c["widths"]                                   # off_bits == 0
    assert any(1 <= x <= 8 for x in c["widths"]), c["widths"]
    assert any(9 <= x <= 16 for x in c["widths"]), c["widths"]
    assert any(x >= 17 for x in c["widths"]), c["widths"]                  # the 16-bit register cache is bypassed
    assert 1 in c["block_ids"] and 256 in c["block_ids"], c["block_ids"]   # a block of ONE id (oi_bits == 0) and full blocks
    for n in (1, 2, 3):
        assert n in c["run_lens"], (n, sorted(c["run_lens"])[:10])
    assert any(x >= 64 for x in c["run_lens"]) and any(x >= 10000 for x in c["run_lens"]), sorted(c["run_lens"])[-5:]
    assert c["straddle"]                                                    # first element fits 16 bits, the second does not
    assert c["straddle16"] and c["high16"]                                  # ... the same, and a first element beyond 16 bits, in blocks of <= 16 bits per offset


def field_score(q, text_match):
    """the best field's Match::get_match_score out of compute_aggregated_score's packing (src/index.cpp:5332-5382)"""
    return (int(text_match) >> (11 if q.match_type == B.MAX_SCORE else 3)) & ((1 << 48) - 1)


def coverage_of_scores(pairs):
    """pairs: [(query, oracle hits)] -> what the ORACLE's text_match values show (field layout of pack_match_score / Match::get_match_score)"""
    exact, offset_pp, proximity, fewer_words, n_hits = set(), set(), set(), False, 0
    for q, ref in pairs:
        n_hits += ref.keys.size
        for tm in ref.text_match.tolist():
            s = field_score(q, tm)
            exact.add((s >> 12) & 0xF)
            proximity.add((s >> 16) & 0xFF)
            if q.prioritize_token_position:
                offset_pp.add((s >> 4) & 0xFF)
            if len(q.tokens) >= 3 and ((s >> 40) & 0xFF) < len(q.tokens):
                fewer_words = True
    return dict(exact=exact, offset_pp=offset_pp, proximity=proximity, fewer_words=fewer_words, n_hits=n_hits)


def assert_score_coverage(c, what):
    assert c["n_hits"] >= 300, (what, c["n_hits"])
    assert {0, 1} <= c["exact"], (what, c["exact"])
    assert 0 in c["offset_pp"] and any(x != 0 for x in c["offset_pp"]), (what, sorted(c["offset_pp"])[:5])      # 255 - max_offset: 0 = clamped at 255
    assert len(c["proximity"]) >= 8, (what, c["proximity"])
    assert c["fewer_words"], what


# ---------------------------------------------------------------- bodies
def body_lists_reach_every_decoder_path(w):
    assert_list_coverage(coverage_of_lists(w))
    assert w.g.term_num_ids(F_PLAIN, 10) == 257                            # the list whose last block holds one id


def body_plain_field(w, options, what):
    """options: {name: value} set for the run and put back afterwards (value 0 or 1 knobs: (set, restore))"""
    for name, (v, _) in options.items():
        w.g.set_option(name, v)
    try:
        pairs = check_queries(w, queries([(F_PLAIN, 15)]), what)
    finally:
        for name, (_, back) in options.items():
            w.g.set_option(name, back)
    assert_score_coverage(coverage_of_scores(pairs), what)


def body_two_plain_fields(w):
    """load_runs_staged_slots / kw_score_kernel<.., MF>: the plain field and its permuted twin, both weight orders"""
    qs = queries([(F_PLAIN, 15), (F_PERM, 10)], flag_sets=FLAG_SETS[:2] + FLAG_SETS[4:]) + queries([(F_PERM, 15), (F_PLAIN, 3)], token_sets=TOKEN_SETS[::3], flag_sets=FLAG_SETS[1:3])
    pairs = check_queries(w, qs, "two fields")
    assert_score_coverage(coverage_of_scores(pairs), "two fields")


def body_array_field(w):
    alone = check_queries(w, queries([(F_ARR, 15)]), "array")
    assert_score_coverage(coverage_of_scores(alone), "array")
    mixed = check_queries(w, queries([(F_PLAIN, 15), (F_ARR, 10)], flag_sets=FLAG_SETS[:2] + FLAG_SETS[4:]) + queries([(F_ARR, 15), (F_PLAIN, 2)], token_sets=TOKEN_SETS[::3], flag_sets=FLAG_SETS[1:3]),
                          "plain + array")
    assert_score_coverage(coverage_of_scores(mixed), "plain + array")
    # the lists of the array field: element indexes >= 256 are stored, a run of hundreds of elements
    ids, oi, off = w.g.term_download(F_ARR, 1)
    ref = w.orc.dump_posting(F_ARR, 1)
    assert np.array_equal(ids, ref[0]) and np.array_equal(oi, ref[1]) and np.array_equal(off, ref[2])
    assert int(oi[1]) - int(oi[0]) > 15 and 300 in off[int(oi[0]):int(oi[1])].tolist()


def body_aux_scores(w):
    """tsgpu_keyword_aux_scores over EVERY (query, document) pair of a handful of queries vs Index::compute_aux_scores in the oracle: a hybrid search whose
    vector half returns every document, so each document the keyword half did not find gets compute_text_match_aux_score's value"""
    n = w.n_docs
    X = w.oracle_vectors()
    token_sets = [[1, 2, 3], [1, 2], [5, 1], [3, 5, 1], [1, 2, 3, 4, 5], list(range(1, 11)), [FILL, 1], [6], [2, 2, 2], [7, 8]]
    checked = partial = 0
    for fields in ([(F_PLAIN, 15)], [(F_PLAIN, 15), (F_ARR, 10)]):
        qs = [T.KwQuery(t, sort=SORT, topster_size=K, fields=fields, prioritize_token_position=bool(i % 2)) for i, t in enumerate(token_sets)]
        item_q = np.repeat(np.arange(len(qs), dtype=np.uint32), n)
        item_d = np.tile(np.arange(n, dtype=np.uint32), len(qs))
        got = w.g.keyword_aux_scores(qs, item_q, item_d).reshape(len(qs), n)
        for i, q in enumerate(qs):
            ref = w.orc.search_hybrid(H.oracle_query(w.orc, q), X[0], k=n, alpha=0.3, rerank=True, cap=2048)
            assert ref.keys.size == n                                         # every document, found by either half
            want = np.zeros(n, np.int64)
            want[ref.keys.astype(np.int64)] = ref.text_match
            full = set(w.oracle(q).keys.tolist())
            bad = np.nonzero(got[i] != want)[0]
            assert bad.size == 0, "aux %s fields %s: %d documents differ, first %d: %x vs oracle %x" % (q.tokens, fields, bad.size, bad[0], got[i][bad[0]], want[bad[0]])
            checked += n
            partial += int(sum(1 for d in range(n) if want[d] != 0 and d not in full))
    assert checked >= 300 and partial >= 300                                   # documents holding only SOME of the tokens are the bulk


def body_grouped_first_pass(w):
    """kw_groupby.hip.h instantiates match_window on its own: one grouped first pass over the plain field"""
    from tests.test_emu_groupby import check_query, oracle_grouped
    qs = queries([(F_PLAIN, 15)], flag_sets=FLAG_SETS[1:2] + FLAG_SETS[4:5])
    limit = 2
    pairs = []
    for lo in range(0, len(qs), 16):
        part = qs[lo:lo + 16]
        h, gh = w.g.keyword_search_grouped_batch(part, [(limit, GROUP_COL, 1, 0, 0)] * len(part), k_stride=K * limit, g_stride=K)
        for i, q in enumerate(part):
            ref = oracle_grouped(w.orc, q, w.distinct, w.has_value, limit, True)
            assert ref.n_groups < K
            check_query(h, gh, i, ref, True, limit, "grouped %s" % q.tokens)
            ref.text_match = ref.scores[:ref.n_groups, 0]          # (first pass: one KV per group; sort slot 0 = _text_match desc)
            pairs.append((q, ref))
    assert sum(ref.n_groups for _, ref in pairs) >= 300            # group KVs compared, all batches
    assert_score_coverage(coverage_of_scores(pairs), "grouped")
