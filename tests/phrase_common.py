"""Bodies of the phrase search tests (tests/test_emu_phrase.py under the SIMT emulator, tests/test_gpu_phrase.py on the GPU): tsgpu_phrase_search_batch against a
Python restatement of the reference that follows ITS control flow, not the device's — posting_list_t::get_offsets (src/posting_list.cpp:832-916: the map of
array index -> per-token position vectors), found_token_sequence / has_phrase_match (:1719-1789: linear rescans that stop at a step down, the uint16_t target),
get_phrase_matches (:1791-1825), Index::do_phrase_search (src/index.cpp:5909-6086: the literal fold, the 10 000-id weight cut, OR of the fields, exclusion,
filter, the ranking by compute_sort_scores in Topster::sort() order) and Index::handle_exclusion (:6274-6324). It works from OracleIndex.dump_posting (ids, offset
index, raw offsets). Where _text_match is no sort key the hit rows must ALSO equal the oracle's wildcard search over the expected id list. No tolerance anywhere.

The crafted corpus (fields 0 and 1 plain, field 2 string[]) holds the shapes at which the kernel can go wrong; every shape is asserted on the RESTATEMENT
(assert_shapes), so the corpus cannot silently lose it."""
import json
import os

import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O
from tests import helpers as H

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "phrase_cases.json")
RANK, IDS, EXCLUDE = B.PHRASE_RANK, B.PHRASE_IDS, B.PHRASE_EXCLUDE
A, Bt, Ct, D, E, X, L, M, K9, Z = 1, 2, 3, 4, 5, 6, 7, 8, 9, 30          # phrase tokens (Bt / Ct: B and C are taken)
TEN = list(range(11, 21))                                                   # the T = 10 phrase
W1, W2, W3, W4, G, Hh = 21, 22, 23, 26, 24, 25
F = 50                                                                      # the long documents' filler
U = 99                                                                      # a token without a posting list anywhere
LONG_LEN = 70000
TM_DESC = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_SEQ_ID, 1, 0))
TM_ASC = ((B.SORT_TEXT_MATCH, -1, 0), (B.SORT_INT64_COLUMN, 1, 0), (B.SORT_SEQ_ID, -1, 0))
COL_ONLY = ((B.SORT_INT64_COLUMN, -1, 0), (B.SORT_SEQ_ID, 1, 0))


# ---------------------------------------------------------------- the reference, restated
def ref_get_offsets(raws):
    """get_offsets (src/posting_list.cpp:832-916): raws[j] = token j's raw offsets for the document -> {array index: [positions of token j, ...] in token order}"""
    m = {}
    for raw in raws:
        start, end = 0, len(raw)
        positions, prev_pos = [], -1
        while start < end:
            pos = int(raw[start])
            start += 1
            if pos == 0:                                  # :875-880
                start += 1
                continue
            if pos == prev_pos:                           # :882-903 end of an array element
                if positions:
                    m.setdefault(int(raw[start]), []).append(positions)
                    positions = []
                    if start + 1 < end and int(raw[start + 1]) == 0:
                        start += 1
                start += 1
                prev_pos = -1
                continue
            prev_pos = pos
            positions.append(((pos & 0xFFFF) - 1) & 0xFFFF)      # positions.push_back((uint16_t)pos - 1) into a vector<uint16_t>, :906
        if positions:
            m.setdefault(0, []).append(positions)         # :909-912
    return m


def ref_found_token_sequence(token_positions, token_index, target_pos):
    """:1719-1751; target_pos is a uint16_t parameter"""
    if token_index == len(token_positions):
        return True
    found_pos, prev_pos = False, -1
    for tok_pos in token_positions[token_index]:
        if tok_pos < prev_pos:
            found_pos = False
            break
        if tok_pos == target_pos:
            found_pos = True
            break
        prev_pos = tok_pos
    if not found_pos:
        return False
    return ref_found_token_sequence(token_positions, token_index + 1, (target_pos + 1) & 0xFFFF)


def ref_has_phrase_match(token_positions):
    """:1771-1789"""
    prev_pos = -1
    for pos in token_positions[0]:
        if pos < prev_pos:
            return False
        if ref_found_token_sequence(token_positions, 1, (pos + 1) & 0xFFFF):
            return True
        prev_pos = pos
    return False


class Restatement:
    """do_phrase_search / handle_exclusion over an OracleIndex's posting lists"""

    def __init__(self, orc, n_fields, cut, points):
        self.orc, self.cut, self.points = orc, cut, points
        self.have = {f: set(int(t) for t in orc.terms(f)) for f in range(n_fields)}
        self._post = {}

    def posting(self, f, t):
        if (f, t) not in self._post:
            ids, oi, off = self.orc.dump_posting(f, t)
            self._post[(f, t)] = (ids, np.append(oi, off.size).astype(np.int64), off)
        return self._post[(f, t)]

    def raw_of(self, f, t, doc):
        ids, oi, off = self.posting(f, t)
        j = int(np.searchsorted(ids, doc))
        assert ids[j] == doc
        return off[oi[j]:oi[j + 1]]

    def contains_ids(self, f, phrase):
        """the leaves' lists (:5941-5953; None: a token without one) and posting_t::intersect"""
        if any(t not in self.have[f] or self.posting(f, t)[0].size == 0 for t in phrase):
            return None
        ids = self.posting(f, phrase[0])[0]
        for t in phrase[1:]:
            ids = np.intersect1d(ids, self.posting(f, t)[0])
        return ids.astype(np.uint32)

    def phrase_matches(self, f, phrase, ids):
        """get_phrase_matches (:1791-1825)"""
        if len(phrase) == 1:
            return ids
        out = []
        for doc in ids:
            m = ref_get_offsets([self.raw_of(f, t, int(doc)) for t in phrase])
            for k in sorted(m):                            # std::map order
                if len(m[k]) == len(phrase) and ref_has_phrase_match(m[k]):
                    out.append(int(doc))
                    break
        return np.array(out, np.uint32)

    def phrase_ids(self, f, phrase):
        ids = self.contains_ids(f, phrase)
        return None if ids is None else self.phrase_matches(f, phrase, ids)

    def do_phrase_search(self, q):
        """-> (ids after exclusion, ids after the filter, {id: match score})"""
        scores, result = {}, np.zeros(0, np.uint32)
        for field, weight, phrases in q.fields:
            acc = np.zeros(0, np.uint32)
            for phrase in phrases:
                this = self.phrase_ids(field, phrase)
                if this is None or this.size == 0:         # :5950-5953, :5963-5967
                    continue
                acc = this if acc.size == 0 else np.intersect1d(this, acc).astype(np.uint32)       # :5971-5981
            if acc.size == 0:
                continue
            for pi in range(min(self.cut, acc.size)):      # :5991-5995
                scores[int(acc[pi])] = max(100000 + weight, scores.get(int(acc[pi]), 0))
            result = acc if result.size == 0 else np.union1d(result, acc).astype(np.uint32)
        if q.excluded_ids is not None and q.excluded_ids.size:
            result = np.setdiff1d(result, q.excluded_ids).astype(np.uint32)
        after_exclusion = result
        if q.filter_ids is not None:
            result = np.intersect1d(result, q.filter_ids).astype(np.uint32)
        return after_exclusion, result, scores

    def handle_exclusion(self, q):
        out = np.zeros(0, np.uint32)
        for field, _, phrases in q.fields:
            for phrase in phrases:
                ids = self.contains_ids(field, phrase)
                if ids is None:
                    continue
                out = np.union1d(out, ids if len(phrase) == 1 else self.phrase_matches(field, phrase, ids)).astype(np.uint32)
        return out

    def rank(self, q, ids, scores, k):
        """the Topster of :6045-6080: (keys, scores [n, 3], text_match, match_score_index) in sort() order (descending (s0, s1, s2, key))"""
        rows = []
        for doc in ids:
            s, msi = [0, 0, 0], -1
            for i, (kind, order, col) in enumerate(q.sort):
                if kind == B.SORT_TEXT_MATCH:
                    v, msi = scores.get(int(doc), 0), i
                elif kind == B.SORT_SEQ_ID:
                    v = int(doc)
                else:
                    assert kind == B.SORT_INT64_COLUMN and col == 0
                    v = int(self.points[int(doc)])
                s[i] = -v if order == -1 else v
            rows.append((s[0], s[1], s[2], int(doc), msi))
        rows.sort(reverse=True)
        rows = rows[:k]
        keys = np.array([r[3] for r in rows], np.uint64)
        sc = np.array([r[:3] for r in rows], np.int64).reshape(-1, 3)
        msi = np.array([r[4] for r in rows], np.int8)
        tm = np.array([r[r[4]] if r[4] >= 0 else 0 for r in rows], np.int64)
        return keys, sc, tm, msi


# ---------------------------------------------------------------- the corpus
def _long(places):
    d = np.full(LONG_LEN, F, np.uint32)
    for p, t in places.items():
        d[p] = t
    return d


def build_model(n_docs):
    """{field: {doc: tokens}} for the plain fields 0 and 1, {doc: [elements]} for field 2"""
    f = lambda i: 51 + i % 17
    f0 = {0: [A, Bt, Ct], 1: [A, f(1), Bt], 2: [Bt, A], 3: [A, Bt, A], 4: [A, Bt, f(2), A],
          5: [t for i in range(300) for t in (X, f(i))][:-1] + [D],                    # X 300 times, "X D" at the LAST occurrence
          6: [t for i in range(40) for t in (X, f(i))] + [D],                          # X and D, never adjacent
          7: _long({65535: W1, 65536: W2, 60000: W3, 66000: W3, 100: W4, 66001: W4}),  # W1 W2 straddles 65535 -> 0; W3 W4 adjacent only AFTER the wrap
          8: _long({60000: W3, 60001: W4, 66000: W3, 65535: W2, 65536: W1}),           # W3 W4 before the wrap; W2 W1: the wrong order on the straddle
          9: [E], 10: [Z, A],
          11: [A, Bt, Ct, D], 12: [A, Bt, D, Ct], 13: TEN, 14: TEN[:4] + [TEN[5], TEN[4]] + TEN[6:], 15: [f(3), E, f(4)],
          16: [Ct, D, f(5)], 17: [Bt, Ct, f(6)], 18: [A, Bt], 19: [G, Hh, A, Bt]}
    for d in range(20, n_docs):
        toks = [M, f(d)]
        if d < 277:                                                                    # list L: exactly 257 ids; "L K9" in the even documents
            toks += [L, K9] if d % 2 == 0 else [L, f(d + 1), K9]
        if d == 300:
            toks = [M, E, f(d)]                                                        # "M E" adjacent only here, in the second block of M's list
        if d % 8:
            toks += [G, Hh]                                                            # the long field list of the weight cut
        else:
            toks += [Hh, G]
        f0[d] = toks
    f1 = {0: [f(0), A, Bt], 1: [A, Bt, f(1)], 2: [Ct, D], 19: [A, Bt], 25: [G, Hh], 9: [E, E]}
    for d in range(40, n_docs, 7):
        f1[d] = [f(d), G, Hh] if d % 2 else [A, f(d), Bt]
    f2 = {16: [[A, f(1)], [f(2), Bt]],                                                 # adjacent positions, but across two elements
          17: [[f(1), f(2)], [A, Bt], [f(3)]],                                         # in the second of three elements
          18: [[A, Bt, A]], 21: [[Bt, A], [A, f(1), Bt]], 22: [[E]], 23: [[f(1)], [Ct, A, Bt, D]], 24: [[A, Bt], [A, Bt]]}
    return {0: f0, 1: f1, 2: f2}


class PhraseWorld:
    def __init__(self, lib, n_docs, cut):
        assert n_docs % 32 != 0 and n_docs > 310                # the last bitmap word is part-filled
        self.lib, self.n_docs, self.cut = lib, n_docs, cut
        self.model = build_model(n_docs)
        self.pts = H.points_of(n_docs)
        self.g = T.GpuIndex(0, lib)
        self.g.set_option("phrase_weight_cut", cut)
        for fld in (0, 1, 2):
            self.g.field_create(fld, fld == 2)
        self.orc = None
        self.fresh_oracle(load=True)

    def fresh_oracle(self, load=False):
        """a FRESH OracleIndex from the model (as tests/mutated_index_common.py builds its expectation); load: its lists into the GpuIndex, too"""
        if self.orc is not None:
            self.orc.close()
        self.orc = orc = O.OracleIndex(3, 1)
        for fld in (0, 1):
            for d, toks in self.model[fld].items():
                orc.index_plain(d, fld, np.asarray(toks, np.uint32))
        for d, elems in self.model[2].items():
            orc.index_array(d, 2, elems)
        orc.set_num_docs(self.n_docs)
        orc.set_sort_dense(0, self.pts)
        if load:
            for fld in (0, 1, 2):
                for term in orc.terms(fld):
                    ids, oi, off = orc.dump_posting(fld, int(term))
                    self.g.term_upsert(fld, int(term), ids, oi, off)
            self.g.column_set(0, self.pts)
            self.g.set_num_docs(self.n_docs)
            self.g.commit()
        self.ref = Restatement(orc, 3, self.cut, self.pts)

    def close(self):
        self.g.close()
        self.orc.close()

    def check(self, queries, k_stride=400, what="", got=None):
        hits, n_ids, ids = got if got is not None else self.g.phrase_search_batch(queries, k_stride)
        for i, q in enumerate(queries):
            w = "%s q%d %r mode %d" % (what, i, q.fields, q.mode)
            assert hits.status[i] == 0, "%s: status %d" % (w, hits.status[i])
            if q.mode == EXCLUDE:
                e_ids = self.ref.handle_exclusion(q)
                assert np.array_equal(ids[i], e_ids), "%s: ids %s, expected %s" % (w, ids[i][:20], e_ids[:20])
                assert int(n_ids[i]) == e_ids.size and hits.n_hits[i] == 0, w
                continue
            before, e_ids, scores = self.ref.do_phrase_search(q)
            assert int(n_ids[i]) == before.size, "%s: n_phrase_ids %d, expected %d" % (w, n_ids[i], before.size)
            assert np.array_equal(ids[i], e_ids), "%s: ids %s (%d), expected %s (%d)" % (w, ids[i][:20], ids[i].size, e_ids[:20], e_ids.size)
            if q.mode == IDS or e_ids.size == 0:
                assert hits.n_hits[i] == 0 and hits.num_matched[i] == 0, w
                continue
            k = q.topster_size
            assert 0 < k <= k_stride
            keys, sc, tm, msi = self.ref.rank(q, e_ids, scores, k)
            n = int(hits.n_hits[i])
            assert n == keys.size, "%s: n_hits %d, expected %d" % (w, n, keys.size)
            assert np.array_equal(hits.keys[i, :n], keys), "%s: keys %s, expected %s" % (w, hits.keys[i, :n][:12], keys[:12])
            assert np.array_equal(hits.scores[i, :n], sc), "%s: scores differ" % w
            assert np.array_equal(hits.text_match[i, :n], tm), "%s: text_match differ" % w
            assert np.array_equal(hits.match_score_index[i, :n], msi), "%s: match_score_index differ" % w
            assert int(hits.num_matched[i]) == e_ids.size, "%s: num_matched %d, expected %d" % (w, hits.num_matched[i], e_ids.size)
            assert (hits.vector_distance[i, :n] == -1.0).all(), w
            if all(s[0] != B.SORT_TEXT_MATCH for s in q.sort):             # ... and the oracle's wildcard search over the expected ids
                ref = H.oracle_wildcard(self.orc, T.KwQuery([], sort=q.sort, topster_size=k, filter_ids=e_ids))
                H.assert_hits_equal(hits, i, ref, w)
                assert np.array_equal(hits.match_score_index[i, :n], ref.match_score_index), w
        return hits, n_ids, ids


def PQ(fields, mode=RANK, sort=TM_DESC, topster_size=400, **kw):
    """fields: [(field, weight, [phrases])] or, shorthand for one field, (field, [phrases])"""
    if isinstance(fields, tuple):
        fields = [(fields[0], 5, fields[1])]
    return T.PhraseQuery(fields, mode=mode, sort=sort, topster_size=topster_size, **kw)


def make_world(lib, n_docs=331, cut=50):
    return PhraseWorld(lib, n_docs, cut)


# ---------------------------------------------------------------- the shapes, asserted on the restatement
def assert_shapes(w):
    r = w.ref
    has = lambda f, ph, d: d in set(r.contains_ids(f, ph).tolist())
    hit = lambda f, ph, d: d in set(r.phrase_ids(f, ph).tolist())
    # near misses: all tokens present, not adjacent / reversed / adjacent only across two elements; a match in the second of three elements
    assert has(0, [A, Bt], 1) and not hit(0, [A, Bt], 1) and has(0, [A, Bt], 2) and not hit(0, [A, Bt], 2) and hit(0, [A, Bt], 0)
    assert has(2, [A, Bt], 16) and not hit(2, [A, Bt], 16) and hit(2, [A, Bt], 17) and hit(2, [A, Bt], 24)
    m16 = ref_get_offsets([r.raw_of(2, A, 16), r.raw_of(2, Bt, 16)])
    assert sorted(m16) == [0, 1] and m16[0] == [[0]] and m16[1] == [[1]]                 # numerically adjacent, different elements
    assert sorted(ref_get_offsets([r.raw_of(2, A, 17), r.raw_of(2, Bt, 17)])) == [1]
    # repeated tokens
    assert hit(0, [A, Bt, A], 3) and has(0, [A, Bt, A], 4) and not hit(0, [A, Bt, A], 4) and hit(2, [A, Bt, A], 18) and not hit(2, [A, Bt, A], 21)
    px = ref_get_offsets([r.raw_of(0, X, 5)])[0][0]
    assert len(px) == 300 and hit(0, [X, D], 5) and px[-1] + 1 == ref_get_offsets([r.raw_of(0, D, 5)])[0][0][0] and has(0, [X, D], 6) and not hit(0, [X, D], 6)
    # narrowing and wrap
    p1, p2 = ref_get_offsets([r.raw_of(0, W1, 7), r.raw_of(0, W2, 7)])[0]
    assert p1 == [65535] and p2 == [0] and hit(0, [W1, W2], 7)                           # the target wraps 65535 + 1 -> 0
    p3, p4 = ref_get_offsets([r.raw_of(0, W3, 7), r.raw_of(0, W4, 7)])[0]
    assert p3 == [60000, 66000 - 65536] and p4 == [100, 66001 - 65536] and not hit(0, [W3, W4], 7)      # adjacent only behind the step down: rejected
    assert hit(0, [W3, W4], 8) and has(0, [W1, W2], 8) and not hit(0, [W1, W2], 8)
    pf = ref_get_offsets([r.raw_of(0, F, 7)])[0][0]
    assert len(pf) > 65536 and hit(0, [F, W1], 7)                                          # a run of ~70 000 positions
    # list lengths
    assert r.posting(0, L)[0].size == 257 and 100 < r.phrase_ids(0, [L, K9]).size < 257
    m_ids = r.posting(0, M)[0]
    assert m_ids.size > 256 and r.phrase_ids(0, [M, E]).tolist() == [300] and int(np.searchsorted(m_ids, 300)) >= 256     # in the second block of M's list
    assert hit(0, [A, Bt, Ct], 0) and hit(0, [A, Bt, Ct, D], 11) and has(0, [A, Bt, Ct, D], 12) and not hit(0, [A, Bt, Ct, D], 12)
    assert hit(0, TEN, 13) and has(0, TEN, 14) and not hit(0, TEN, 14)
    # fold quirks
    ab, bc, ba, cd = (set(r.phrase_ids(0, p).tolist()) for p in ([A, Bt], [Bt, Ct], [Bt, A], [Ct, D]))
    assert ab & bc and ba and cd and not (ba & cd)
    restart = r.do_phrase_search(PQ((0, [[Bt, A], [Ct, D], [A, Bt]])))[1]
    assert set(restart.tolist()) == ab                                                   # the third phrase starts the field over
    assert r.contains_ids(0, [A, U]) is None and r.phrase_ids(0, [A, Z]).size == 0 and r.contains_ids(0, [A, Z]).size > 0
    # fields and the cut
    gh = r.phrase_ids(0, [G, Hh])
    assert gh.size > w.cut and 19 in set(gh.tolist()) and hit(1, [A, Bt], 19)
    assert hit(0, [A, Bt], 0) and hit(1, [A, Bt], 0) and hit(1, [A, Bt], 1) and not hit(0, [A, Bt], 1)
    assert w.n_docs % 32 != 0


# ---------------------------------------------------------------- test bodies
def run_adjacency(w):
    assert_shapes(w)
    phrases0 = [[A, Bt], [Bt, A], [A, Bt, A], [X, D], [W1, W2], [W3, W4], [W2, W1], [F, W1], [L, K9], [M, E], [A, Bt, Ct], [A, Bt, Ct, D], TEN, [E], [A, Z], [A, U], [U],
                [G, Hh], [Hh, G], [M, G], [K9, G, Hh]]
    qs = [PQ((0, [p])) for p in phrases0]
    qs += [PQ((2, [p])) for p in ([A, Bt], [A, Bt, A], [Bt, A], [E], [Ct, A, Bt, D], [A, Bt, D])]
    qs += [PQ((1, [p])) for p in ([A, Bt], [G, Hh], [E, E], [E])]
    w.check(qs, what="adjacency")
    c0, m0 = w.g.counter("phrase_records_checked"), w.g.counter("phrase_records_matched")
    w.check([PQ((0, [[A, Bt]]))], what="counters")
    n_and = w.ref.contains_ids(0, [A, Bt]).size
    assert w.g.counter("phrase_records_checked") - c0 == n_and and w.g.counter("phrase_records_matched") - m0 == w.ref.phrase_ids(0, [A, Bt]).size


def run_fold(w):
    qs = [PQ((0, [[A, Bt], [Bt, Ct]])),                                  # two phrases whose lists intersect
          PQ((0, [[Bt, A], [Ct, D], [A, Bt]])),                          # an empty intersection, then a third phrase: the restart
          PQ((0, [[Bt, A], [Ct, D]])),                                   # ... and without one: nothing
          PQ((0, [[A, Bt], [A, U], [Bt, Ct]])),                          # an unknown token between two phrases that match
          PQ((0, [[A, Z], [A, Bt]])), PQ((0, [[A, Bt], [A, Z]])), PQ((0, [[A, Z]])),
          PQ((0, [[E], [M, E]])), PQ((0, [[G, Hh], [L, K9], [M]])),
          PQ((0, [[A, Bt], [Bt, Ct], [Ct, D], [A, Bt, Ct, D], [E], [A], [Bt], [D]])),        # TSGPU_MAX_PHRASES phrases
          PQ((2, [[A, Bt], [Bt, A]])), PQ((2, [[A, Bt], [E]])), PQ((0, []))]
    hits, n_ids, ids = w.check(qs, what="fold")
    assert n_ids[2] == 0 and n_ids[6] == 0 and n_ids[12] == 0 and n_ids[1] > 0


def run_fields_and_cut(w):
    both = lambda w0, w1, **kw: PQ([(0, w0, [[A, Bt]]), (1, w1, [[A, Bt]])], **kw)
    qs = [both(3, 7), both(7, 3), both(3, 7, sort=TM_ASC), both(0, 15, sort=COL_ONLY),
          PQ([(0, 2, [[G, Hh]]), (1, 9, [[A, Bt]])]), PQ([(0, 2, [[G, Hh]]), (1, 9, [[A, Bt]])], sort=TM_ASC), PQ([(1, 9, [[A, Bt]]), (0, 2, [[G, Hh]])], sort=TM_ASC),
          PQ([(0, 4, [[G, Hh]]), (1, 6, [[G, Hh]]), (2, 1, [[A, Bt]])], sort=TM_DESC, topster_size=37),
          PQ((0, [[G, Hh]]), sort=TM_ASC, topster_size=400), PQ((0, [[G, Hh]]), sort=COL_ONLY), PQ([(0, 1, [[A, Bt]]), (1, 2, [[U]]), (2, 3, [[A, Bt]]), (1, 4, [[E]])])]
    hits, n_ids, ids = w.check(qs, k_stride=400, what="fields")
    s37 = w.ref.do_phrase_search(qs[0])[2]
    s73 = w.ref.do_phrase_search(qs[1])[2]
    assert s37[0] == 100007 and s73[0] == 100007 and s37[1] == 100007 and s73[1] == 100003          # the max over the fields wins, either order
    _, gh_ids, gh_scores = w.ref.do_phrase_search(qs[8])
    inside = [d for d in gh_ids.tolist() if gh_scores.get(d, 0)]
    assert len(inside) == w.cut and len(gh_ids) > w.cut and max(inside) < min(d for d in gh_ids.tolist() if d not in gh_scores)     # hits on both sides of the cut


def run_exclusion_and_filter(w):
    gh = w.ref.phrase_ids(0, [G, Hh])
    ab = w.ref.phrase_ids(0, [A, Bt])
    nd = w.n_docs
    qs = [PQ((0, [[G, Hh]]), excluded_ids=gh[3:9], sort=TM_ASC),                     # excluded ids INSIDE the cut: the cut is taken before exclusion
          PQ((0, [[G, Hh]]), excluded_ids=gh), PQ((0, [[G, Hh]]), excluded_ids=np.array([31, 32, 33, 63, 64, nd - 1], np.uint32)),
          PQ((0, [[A, Bt]]), filter_ids=np.zeros(0, np.uint32)),                     # a filter that matches nothing (non-NULL, n = 0)
          PQ((0, [[A, Bt]]), filter_ids=ab[::2]), PQ((0, [[G, Hh]]), filter_ids=np.arange(0, nd, 3), excluded_ids=gh[1::3], sort=COL_ONLY),
          PQ((0, [[A, Z]])),                                                         # no filter, an empty phrase result: no hits
          PQ((0, [[A, Bt]]), mode=IDS), PQ((0, [[G, Hh]]), mode=IDS, filter_ids=np.arange(0, nd, 2), excluded_ids=gh[:5]),
          PQ([(0, 1, [[A, Bt], [Bt, Ct]]), (2, 1, [[A, Bt]])], mode=IDS),
          PQ([(0, 0, [[A, Bt], [Ct, D]]), (1, 0, [[G, Hh]]), (2, 0, [[A, Bt, A]])], mode=EXCLUDE),
          PQ((0, [[E]]), mode=EXCLUDE), PQ((0, [[A, U], [Bt, A]]), mode=EXCLUDE), PQ((0, [[A, U]]), mode=EXCLUDE), PQ((0, [[U]]), mode=EXCLUDE)]
    hits, n_ids, ids = w.check(qs, what="excl/filter")
    s = w.ref.do_phrase_search(qs[0])[2]
    assert sum(1 for d in ids[0].tolist() if d in s) == w.cut - 6
    assert n_ids[3] == ab.size and ids[3].size == 0 and hits.n_hits[3] == 0 and n_ids[6] == 0 and hits.n_hits[6] == 0 and n_ids[1] == 0
    assert w.g.wildcard_search_batch([T.KwQuery([], sort=COL_ONLY)]).n_hits[0] > 0
    assert ids[11].size > 0 and ids[12].tolist() == w.ref.phrase_ids(0, [Bt, A]).tolist() and ids[13].size == 0 and ids[14].size == 0
    # IDS / EXCLUDE without an output object
    _, n2, ids2 = w.g.phrase_search_batch(qs[7:], with_hits=False)
    for a, b in zip(ids2, ids[7:]):
        assert np.array_equal(a, b)


def mixed_40(w):
    gh = w.ref.phrase_ids(0, [G, Hh])
    base = [PQ((0, [[A, Bt]])), PQ((0, [[A, Bt, Ct, D]]), sort=COL_ONLY), PQ((2, [[A, Bt]])), PQ((0, [[E]])), PQ((0, [[A, U]])), PQ((0, [[G, Hh]]), sort=TM_ASC, topster_size=60),
            PQ([(0, 3, [[A, Bt]]), (1, 7, [[A, Bt]])]), PQ((0, [[Bt, A], [Ct, D], [A, Bt]])), PQ((0, [TEN])), PQ((0, [[G, Hh]]), mode=IDS, excluded_ids=gh[:4]),
            PQ((0, [[E], [Bt, A]]), mode=EXCLUDE), PQ((0, [[L, K9]]), filter_ids=np.arange(0, w.n_docs, 2)), PQ((0, [[X, D]])), PQ((1, [[G, Hh]]), sort=COL_ONLY)]
    return [base[i % len(base)] for i in range(40)]


def run_batching(w):
    qs = mixed_40(w)
    s0 = w.g.counter("phrase_syncs")
    got = w.check(qs, what="batch40")
    per_batch = w.g.counter("phrase_syncs") - s0
    hits, n_ids, ids = got
    for i, q in enumerate(qs):                                            # every query equals its own 1-query call, which synchronises as often as the batch
        s1 = w.g.counter("phrase_syncs")
        h1, u1, i1 = w.g.phrase_search_batch([q], 400)
        assert w.g.counter("phrase_syncs") - s1 == per_batch, (i, per_batch)
        n = int(hits.n_hits[i])
        assert h1.status[0] == 0 and h1.n_hits[0] == n and h1.num_matched[0] == hits.num_matched[i], i
        assert np.array_equal(h1.keys[0, :n], hits.keys[i, :n]) and np.array_equal(h1.scores[0, :n], hits.scores[i, :n]), i
        assert np.array_equal(h1.text_match[0, :n], hits.text_match[i, :n]) and np.array_equal(h1.match_score_index[0, :n], hits.match_score_index[i, :n]), i
        assert u1[0] == n_ids[i] and np.array_equal(i1[0], ids[i]), i
    w.g.set_option("phrase_round_max_bytes", 1)                           # rounds: a scratch bound that holds one query at a time gives the same answers
    r0 = w.g.counter("phrase_rounds")
    try:
        got2 = w.check(qs, what="rounds")
    finally:
        w.g.set_option("phrase_round_max_bytes", 2 << 30)
    assert w.g.counter("phrase_rounds") - r0 == 40 > 1
    assert np.array_equal(got2[0].keys, hits.keys) and np.array_equal(got2[0].n_hits, hits.n_hits)
    i0 = w.g.counter("phrase_items")
    w.g.phrase_search_batch([PQ([(0, 1, [[A, Bt], [A, U], [E]]), (1, 1, [[A, Bt]])])], 400)
    assert w.g.counter("phrase_items") - i0 == 3                          # the phrase with the unknown token is no item


def run_statuses(w):
    too_many = PQ((0, [[A, Bt]] * (B.MAX_PHRASES + 1)))
    too_long = PQ((0, [[A] * (B.MAX_QUERY_TOKENS + 1)]))
    qs = [PQ((0, [[A, Bt]])), PQ((7, [[A, Bt]])), too_many, too_long, PQ((0, [[]])), PQ((0, [[A, Bt]]), mode=3), PQ((0, [[A, Bt]]), sort=((B.SORT_VECTOR_DISTANCE, 1, 0),)),
          PQ((0, [[A, Bt]]), sort=((8, 1, 0),)), PQ((0, [[A, Bt]]), deadline_us=1), PQ([]), PQ([(0, 1, [[A]])] * 5), PQ((0, [[A, Bt]]), mode=IDS, deadline_us=1), PQ((2, [[A, Bt]]))]
    hits, n_ids, ids = w.g.phrase_search_batch(qs, 400)
    I, UN, DL = B.ERR_INVALID, B.ERR_UNSUPPORTED, B.ERR_DEADLINE
    assert hits.status.tolist() == [0, I, UN, UN, I, I, UN, UN, DL, I, I, DL, 0]
    for i in range(1, 12):
        assert hits.n_hits[i] == 0 and n_ids[i] == 0 and ids[i].size == 0, i
    assert hits.search_cutoff[8] == 1 and hits.search_cutoff[11] == 1
    w.check([qs[0], qs[12]], what="status neighbours")
    try:                                                                  # no output object: the refused query's status is the call's
        w.g.phrase_search_batch([PQ((7, [[A, Bt]]), mode=IDS)], with_hits=False)
        raise AssertionError("a refused query without an output object must fail the call")
    except B.TsgpuError as e:
        assert e.code == I
    try:
        w.g.phrase_search_batch([PQ((0, [[A, Bt]]))], with_hits=False)    # a RANK query needs its output arrays
        raise AssertionError("RANK without an output object")
    except B.TsgpuError as e:
        assert e.code == I


def run_mutated(lib):
    """upserts and erases that touch the phrases' lists, committed: the front answers for the new lists (expectation: a fresh oracle from the model)"""
    w = make_world(lib, n_docs=331, cut=50)
    try:
        qs = [PQ((0, [[A, Bt]])), PQ((0, [[A, Bt, Ct]])), PQ((0, [[L, K9]])), PQ((0, [[M, E]])), PQ((0, [[G, Hh]]), sort=TM_ASC), PQ((0, [[Bt, A], [Ct, D], [A, Bt]])), PQ((0, [[E]]), mode=EXCLUDE)]
        before = w.check(qs, what="before")

        def replace(d, toks):
            for t in set(w.model[0].get(d, [])):
                w.g.posting_erase(0, int(t), d)
            w.model[0][d] = toks
            w.g.index_plain_doc(d, 0, toks)

        replace(0, [A, f_(0), Bt, Ct])                # A B no longer adjacent in document 0
        replace(1, [A, Bt, Ct])                       # ... and now adjacent in document 1
        replace(22, [M, L, f_(1), K9, G, Hh])         # L K9 taken apart in an even document
        replace(300, [M, f_(2), E])                   # M E no longer anywhere
        replace(310, [M, E, Hh, G])                   # ... but here
        replace(9, [f_(3)])                           # E's list loses an id
        for t in set(w.model[0][2]):                  # document 2 erased altogether ("B A")
            w.g.posting_erase(0, int(t), 2)
        del w.model[0][2]
        staged = w.g.phrase_search_batch(qs, 400)
        assert np.array_equal(staged[2][0], before[2][0])                  # nothing is visible before the commit
        w.g.commit()
        w.fresh_oracle()
        assert w.ref.phrase_ids(0, [M, E]).tolist() == [310] and 0 not in w.ref.phrase_ids(0, [A, Bt]).tolist() and 1 in w.ref.phrase_ids(0, [A, Bt]).tolist()
        after = w.check(qs, what="after commit")
        assert not np.array_equal(after[2][0], before[2][0])
    finally:
        w.close()


def f_(i):
    return 51 + i % 17


def run_golden(lib):
    """the reference's own phrase tests (tests/golden/phrase_cases.json: documents, hand-tokenised queries, expected ids in order) through the real call; a mixed
    query hands the IDS result to a keyword call as its filter"""
    cases = json.load(open(GOLDEN))
    for case in cases["cases"]:
        vocab = {}
        tid = lambda tok: vocab.setdefault(tok, len(vocab) + 1)
        fields = case["fields"]                                            # [{"name", "array"}]
        docs = [case["docs"][0]] * (case.get("repeat_first_doc", 1) - 1) + case["docs"]
        n_docs = len(docs)
        orc = O.OracleIndex(len(fields), 1)
        for d, doc in enumerate(docs):
            for fi, fd in enumerate(fields):
                v = doc.get(fd["name"])
                if v is None:
                    continue
                if fd["array"]:
                    orc.index_array(d, fi, [[tid(t) for t in e] for e in v])
                elif v:
                    orc.index_plain(d, fi, np.array([tid(t) for t in v], np.uint32))
        pts = np.array([doc.get("points", 0) for doc in docs], np.int64)
        orc.set_num_docs(n_docs)
        orc.set_sort_dense(0, pts)
        g = T.GpuIndex(0, lib)
        try:
            for fi, fd in enumerate(fields):
                g.field_create(fi, bool(fd["array"]))
                for term in orc.terms(fi):
                    ids, oi, off = orc.dump_posting(fi, int(term))
                    g.term_upsert(fi, int(term), ids, oi, off)
            g.column_set(0, pts)
            g.set_num_docs(n_docs)
            g.commit()
            for s in case["searches"]:
                fl = [(fi, w, [[vocab.get(t, 9999) for t in p] for p in s["phrases"]]) for fi, w in s["query_by"]]
                excluded = None
                if s.get("exclude_phrases"):
                    _, _, ex = g.phrase_search_batch([T.PhraseQuery([(fi, w, [[vocab.get(t, 9999) for t in p] for p in s["exclude_phrases"]]) for fi, w in s["query_by"]], mode=EXCLUDE)], with_hits=False)
                    excluded = ex[0]
                sort = TM_DESC
                flt = np.array(s["filter_ids"], np.uint32) if "filter_ids" in s else None
                if not s.get("tokens"):
                    if s["phrases"]:
                        hits, _, ids = g.phrase_search_batch([T.PhraseQuery(fl, sort=sort, topster_size=250, excluded_ids=excluded, filter_ids=flt)], 250)
                    else:                                                   # only -"...": a wildcard search without the excluded ids
                        hits = g.wildcard_search_batch([T.KwQuery([], sort=sort, excluded_ids=excluded)], 250)
                    got = hits.keys[0, :int(hits.n_hits[0])].tolist()
                else:                                                       # phrases + ordinary tokens: the phrase ids are the keyword search's filter (:6028-6032)
                    _, n_ids, ids = g.phrase_search_batch([T.PhraseQuery(fl, mode=IDS, excluded_ids=excluded, filter_ids=flt)], with_hits=False)
                    got = []
                    if ids[0].size:
                        kq = T.KwQuery([vocab.get(t, 9999) for t in s["tokens"]], fields=[(fi, w) for fi, w in s["query_by"]], sort=sort, filter_ids=ids[0], excluded_ids=excluded)
                        h = g.keyword_search_batch([kq], 250)
                        assert h.status[0] == 0
                        got = h.keys[0, :int(h.n_hits[0])].tolist()
                if s.get("unordered"):
                    got = sorted(got)
                assert got == s["expected_doc_ids"], (case["name"], s, got)
        finally:
            g.close()
            orc.close()
