"""Shared bodies of tests/test_emu_vector_values.py (CPU tier, SIMT emulator) and tests/test_gpu_vector_values.py (-m gpu, libtsgpu.so): the bf16
bracket k-NN (vec_kernels.hip.h, "bf16 PREFILTER path": vec_to_bf16_kernel, vec_tile_nmax_kernel, vec_hscan_kernel<1|2|4>, vec_thresh_kernel,
vec_refine_kernel, vec_rescore_kernel, vec_select_kernel) on VALUE distributions the standard-normal rows of the other vector tests never produce.

Every case builds the same rows in the library and in the oracle and compares vec_knn_batch with OracleIndex.flat_knn (exact fp32 scan in hnswlib's
summation order, ties -> smaller label) for EVERY query: count, labels in order, distance bits. No tolerance. vec_count_rescored = 1;
vec_prefilter_groups must rise and vec_prefilter_fallbacks must not (a fallback would mean the fp32 scan answered, not the bracket), unless the
case says otherwise.

Base shape: N = 2 000 rows (15 full 128-row tiles + 80 rows), dims 64 (one bf16 k chunk, hnswlib's SIMD16 order) and 70 (zero-padded second chunk,
SIMD16 + scalar residual order), k = 50, inner product. Routes: vec_sample_tiles = 2 (a strided sample of 2 of the 16 tiles -> L1 -> scan of all 16) and 512 (the
small-index route: the sample IS the whole index). At k = 50 the 2-tile sample holds 8 groups of 32 rows, fewer than k, so vec_thresh_kernel returns
L1 = -inf there: that route tests the "no threshold" scan, where every row is a candidate and vec_refine_kernel's L2 does all the pruning; a finite
T(L1) and the scan's `sc < T(L1) - e` test run on route 512 -- and, from a PARTIAL sample, in body_partial_sample (k = 8 <= 8 groups).
n_q = 4 / 70 / 130 instantiate vec_hscan_kernel<1> / <2> / <4>.

Families (row scale x query scale on N(0,1) entries unless stated; seeds fixed):
  a  tiny products: sum x^2 underflows in fp32 (|x| <~ 3e-23: every square is 0; 1e-22: subnormal squares), so a norm computed from it is 0 or too small
     and an error radius c * |q| * |x| built from it collapses. 1e-25 x 1e18, 1e-25 x 1, 1e18 x 1e-25, 1e-22 x 1e15, and rows alternating 1e-25 / 1
     inside every tile (the tile maximum is ordinary, single rows underflow).
  b  distance ties the score does not see: the reference ranks on fl(1 - s) and breaks ties by label; rows whose score is provably below the k-th
     best can still TIE it in distance once |s| is far below ulp(1). 1e-20 x 1 and 1e-21 x 1e10 (every distance 1.0f), 1e-4 x 1e-4 and 3e-4 x 3e-4.
     Coverage (from the oracle): some query has a row OUTSIDE the top k whose distance bits equal the k-th.
  c  non-centred data, 0.05 N(0,1) + 5 on both sides: every score ~1 600, the bracket holds everyone: vec_rescored_rows == N * n_q.
  d  one row per tile x 1e6: the tile bound keeps the whole tile (vec_candidate_rows ~ N * n_q), the per-row norms of vec_refine_kernel prune.
  e  heavy-tailed norms, x exp(N(0, 6^2)) per row and per query; one coordinate holding 1 - 1e-6 of a row's energy.
  f  signed zeros, zero rows, a zero and a negative-zero query (every distance 1.0f -> labels 0..k-1; the mass-tie exit to the fp32 scan is allowed).
  g  rows with an inf / NaN coordinate: the ranks of all other rows are the oracle's.
  h  families a and b under METRIC_COSINE (the reference's 1 / (sqrt(ss) + 1e-30) with an underflowed ss).
  i  family b at 1e-4 x 1e-4 through vector_search_batch with a filter (the entry point a server calls)."""
import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from oracle import oracle_py as O
from tests import helpers as H

N, K = 2000, 50
DIMS = (64, 70)
ROUTES = (2, 512)
N_QS = (4, 70, 130)
MAX_Q = 130
RTOL = 1e-5                 # the fp32 MFMA scan's band (tests/test_emu_vector.py: _check_knn)


def _gauss(seed, n, dim):
    return np.random.default_rng(seed).standard_normal((n, dim))


def _scaled(rs, qs):
    def make(dim):
        return (_gauss(1000 + dim, N, dim) * rs).astype(np.float32), (_gauss(2000 + dim, MAX_Q, dim) * qs).astype(np.float32)
    return make


def _mixed(dim):
    X = _gauss(1000 + dim, N, dim)
    X[0::2] *= 1e-25                                                      # even rows tiny, odd rows ordinary: interleaved inside every tile
    return X.astype(np.float32), _gauss(2000 + dim, MAX_Q, dim).astype(np.float32)


def _offset(dim):
    return (0.05 * _gauss(1000 + dim, N, dim) + 5).astype(np.float32), (0.05 * _gauss(2000 + dim, MAX_Q, dim) + 5).astype(np.float32)


GIANT_AT = 5                                                              # row % 128 of the giant row of every tile
N_GIANT = len(range(GIANT_AT, N, 128))


def _giant(dim):
    X, Q = _scaled(1, 1)(dim)
    X[GIANT_AT::128] *= np.float32(1e6)
    return X, Q


def _heavy(dim):
    rng = np.random.default_rng(3000 + dim)
    X = _gauss(1000 + dim, N, dim) * np.exp(rng.normal(0, 6, size=(N, 1)))
    Q = _gauss(2000 + dim, MAX_Q, dim) * np.exp(rng.normal(0, 6, size=(MAX_Q, 1)))
    return X.astype(np.float32), Q.astype(np.float32)


def _spike(dim):
    rng = np.random.default_rng(4000 + dim)
    X, Q = _gauss(1000 + dim, N, dim), _gauss(2000 + dim, MAX_Q, dim)
    at = rng.integers(0, dim, size=N)
    X[np.arange(N), at] = 0
    rest = (X * X).sum(axis=1)
    X[np.arange(N), at] = np.sqrt(rest * (1 - 1e-6) / 1e-6) * rng.choice([-1.0, 1.0], size=N)      # 1 - 1e-6 of the energy in one coordinate
    return X.astype(np.float32), Q.astype(np.float32)


def _zeros(dim):
    rng = np.random.default_rng(5000 + dim)
    X, Q = _scaled(1, 1)(dim)
    X[rng.random(X.shape) < 0.3] = 0.0
    X[rng.random(X.shape) < 0.1] = -0.0
    X[7] = 0.0; X[128] = -0.0; X[1999] = 0.0; X[300:310] = 0.0           # zero rows (first row of a tile, last row of the index, a run)
    Q[rng.random(Q.shape) < 0.2] = -0.0
    Q[0] = 0.0; Q[3] = -0.0                                               # a zero and a negative-zero query
    return X, Q


FAMILY_A = {"a-1e-25x1e18": _scaled(1e-25, 1e18), "a-1e-25x1": _scaled(1e-25, 1), "a-1e18x1e-25": _scaled(1e18, 1e-25), "a-1e-22x1e15": _scaled(1e-22, 1e15),
            "a-mixed": _mixed}
FAMILY_B = {"b-1e-20x1": _scaled(1e-20, 1), "b-1e-21x1e10": _scaled(1e-21, 1e10), "b-1e-4x1e-4": _scaled(1e-4, 1e-4), "b-3e-4x3e-4": _scaled(3e-4, 3e-4)}
ALL_TIE = ("b-1e-20x1", "b-1e-21x1e10")                                   # every distance is exactly 1.0f
OTHERS = {"c-offset": _offset, "d-giant": _giant, "e-heavy": _heavy, "e-spike": _spike, "f-zeros": _zeros}
CASES = dict(FAMILY_A, **FAMILY_B, **OTHERS)
FALLBACK_ALLOWED = ("f-zeros",)


class Pair:
    """the same rows (label = row) in a GpuIndex vector field and in the oracle, + the oracle's answers per query (computed once)"""

    def __init__(self, lib, X, Q, metric=B.METRIC_IP, k=K):
        self.X, self.Q, self.k, self.n = X, Q, k, X.shape[0]
        self.g = T.GpuIndex(0, lib)
        self.g.set_option("vec_count_rescored", 1)
        self.g.vec_create(1, X.shape[1], metric)
        self.orc = O.OracleIndex(1, 1)
        self.orc.vec_init(X.shape[1], metric)
        self.upsert(np.arange(self.n), X)

    def upsert(self, labels, rows):
        self.g.vec_upsert(1, np.asarray(labels, np.uint64), rows)
        self.orc.vec_add(np.asarray(labels, np.uint32), rows)
        self._ref = {}

    def ref(self, i, k=None):
        k = k or self.k
        if (i, k) not in self._ref:
            self._ref[(i, k)] = self.orc.flat_knn(self.Q[i], k)
        return self._ref[(i, k)]

    def wrong_queries(self, n_q):
        """vec_knn_batch vs flat_knn for every query: the queries whose count, label order or distance bits differ"""
        dist, lab, cnt = self.g.vec_knn_batch(1, self.Q[:n_q], self.k)
        bad = []
        for i in range(n_q):
            d, l = self.ref(i)
            if not (cnt[i] == d.size and np.array_equal(lab[i, :d.size].astype(np.uint32), l) and np.array_equal(dist[i, :d.size].view(np.uint32), d.view(np.uint32))):
                bad.append(i)
        return bad

    def close(self):
        self.g.close()
        self.orc.close()


def all_inside_band(p, i):
    """from the oracle alone: every row's distance lies within the fp32 scan's 1e-5 band of query i's k-th distance, so neither the band nor a
    label SET pins anything and the order has to"""
    d, _ = p.ref(i, p.n)
    return bool(np.all(np.abs(d - d[p.k - 1]) <= RTOL * max(1.0, abs(float(d[p.k - 1])))))


def fp32_scan_equal(p, i, dist, lab, cnt, what, ulp_swaps=False):
    """the fp32 MFMA scan's comparison (its summation order is its own, so no distance bits): test_emu_vector._check_knn's assertions -- distances
    within 1e-5, the same label set, ascending order. Where all_inside_band() holds, the labels must also come in the oracle's ORDER.
    ulp_swaps (family c ONLY): scores near 1 750 have an ulp of 1.2e-4 and the k-th distance has neighbours ONE ulp away, which the scan's own
    summation order swaps across the cut: c-offset at dim 70, query 2, on the emulator returns label 1371 (oracle distance -1752.78198, exact
    -1752.781888) for label 387 (the oracle's k-th, -1752.78210, exact -1752.782166), 7e-8 relative. There the sets may differ by rows whose
    ORACLE distance is within the 1e-5 band (1.75e-2 here, ~1 % of the rows) of the k-th; every other case compares the sets strictly."""
    d, l = p.ref(i)
    assert cnt[i] == d.size, (what, i)
    assert np.allclose(dist[i, :d.size], d, rtol=RTOL, atol=RTOL), (what, i, np.abs(dist[i, :d.size] - d).max())
    a, b = set(lab[i, :d.size].astype(np.int64).tolist()), set(l.astype(np.int64).tolist())
    if ulp_swaps and a != b:
        dall, lall = p.ref(i, p.n)
        of = dict(zip(lall.tolist(), dall.tolist()))
        band = RTOL * max(1.0, abs(float(d[-1])))
        print("%s query %d: sets differ by %s" % (what, i, sorted(a ^ b)))
        assert len(a ^ b) <= 4 and all(abs(of[x] - float(d[-1])) <= band for x in a ^ b), (what, i, sorted(a ^ b))
    else:
        assert a == b, (what, i, sorted(a ^ b))
    assert (np.diff(dist[i, :d.size]) >= 0).all(), (what, i)
    if all_inside_band(p, i):
        assert np.array_equal(lab[i, :d.size].astype(np.uint32), l), (what, i)


def bracket_run(p, n_q, sample_tiles, what, allow_fallback=False):
    """one batch through the bracket path, bit-exact against the oracle; -> dict of the counters of that batch"""
    g = p.g
    g.set_option("vec_prefilter", 1)
    g.set_option("vec_sample_tiles", sample_tiles)
    before = {c: g.counter(c) for c in ("vec_prefilter_groups", "vec_prefilter_fallbacks", "vec_overflow_rounds")}
    bad = p.wrong_queries(n_q)
    assert not bad, "%s n_q=%d sample_tiles=%d: %d / %d queries differ from the oracle (first: %s); %d rows re-scored" % (
        what, n_q, sample_tiles, len(bad), n_q, bad[:8], g.counter("vec_rescored_rows"))
    fell = g.counter("vec_prefilter_fallbacks") - before["vec_prefilter_fallbacks"]
    if allow_fallback:
        assert g.counter("vec_prefilter_groups") + g.counter("vec_prefilter_fallbacks") > before["vec_prefilter_groups"] + before["vec_prefilter_fallbacks"], what
    else:
        assert fell == 0, "%s n_q=%d sample_tiles=%d: the bracket path handed the batch to the fp32 scan" % (what, n_q, sample_tiles)
        assert g.counter("vec_prefilter_groups") > before["vec_prefilter_groups"], what
    return dict(rescored=g.counter("vec_rescored_rows"), fell=fell, overflow_rounds=g.counter("vec_overflow_rounds") - before["vec_overflow_rounds"])


def has_tie_beyond_k(p, n_q):
    """family b's coverage condition, from the oracle alone: some query has a row outside its top k with the k-th distance's bits"""
    for i in range(n_q):
        d, _ = p.ref(i, p.k + 1)
        if d.size == p.k + 1 and d[p.k - 1:p.k].view(np.uint32)[0] == d[p.k:].view(np.uint32)[0]:
            return True
    return False


def body_partial_sample(lib, name, dim, n_q=4, k=8):
    """vec_sample_tiles = 2 with k = 8: the 8 groups of the 2 sampled tiles yield a FINITE L1 from a partial sample, so T(L1) and the scan's
    tile- and row-level tests really filter the other 14 tiles (coverage: fewer candidates than rows). Not for a-mixed: its unbounded rows make
    every tile maximum +inf, so every row is a candidate by design."""
    X, Q = CASES[name](dim)
    p = Pair(lib, X, Q, k=k)
    try:
        if name in FAMILY_B:
            assert has_tie_beyond_k(p, n_q), "%s: no query ties at the k-th distance beyond k = %d" % (name, k)
        bracket_run(p, n_q, 2, "%s dim %d k %d" % (name, dim, k))
        assert p.g.counter("vec_candidate_rows") < N * n_q, "L1 filtered nothing: the sample gave no finite threshold"
    finally:
        p.close()


def body_case(lib, name, dim, routes=ROUTES, n_qs=N_QS, metric=B.METRIC_IP):
    X, Q = CASES[name](dim)
    p = Pair(lib, X, Q, metric)
    try:
        if metric == B.METRIC_COSINE:
            for lab in (0, 777, N - 1):
                assert np.array_equal(p.g.vec_get(1, lab).view(np.uint32), p.orc.vec_get(lab).view(np.uint32)), (name, lab)       # hnsw_index_t::normalize_vector
        if name in FAMILY_B and metric == B.METRIC_IP:
            assert has_tie_beyond_k(p, min(n_qs)), "%s: no query ties at the k-th distance beyond k; the case tests nothing" % name
        for st in routes:
            for n_q in n_qs:
                r = bracket_run(p, n_q, st, "%s dim %d" % (name, dim), allow_fallback=name in FALLBACK_ALLOWED)
                if name == "c-offset":
                    assert r["rescored"] == N * n_q, "the bracket should hold every row (%d of %d re-scored)" % (r["rescored"], N * n_q)
                if name == "d-giant":       # (a giant row whose own score is hugely negative may fall below even that bound)
                    assert p.g.counter("vec_candidate_rows") >= (N - N_GIANT) * n_q, "a giant row should keep every ordinary row of its tile past the tile bound"
                    assert r["rescored"] < N * n_q // 2, "the per-row norms should prune what the tile bound kept (%d re-scored)" % r["rescored"]
                if name == "f-zeros":
                    assert np.array_equal(p.ref(0)[1], np.arange(K)) and np.array_equal(p.ref(3)[1], np.arange(K))       # zero query: labels 0..k-1
    finally:
        p.close()


def body_offset_with_tiny_segments(lib, dim, n_q=4):
    """family c with vec_cand_cap = 64: every (slab, query) segment overflows -> raise L1 -> scan again; the bound may stop moving (fallback allowed)"""
    X, Q = CASES["c-offset"](dim)
    p = Pair(lib, X, Q)
    try:
        p.g.set_option("vec_cand_cap", 64)
        p.g.set_option("vec_sample_tiles", 2)
        f0, o0 = p.g.counter("vec_prefilter_fallbacks"), p.g.counter("vec_overflow_rounds")
        dist, lab, cnt = p.g.vec_knn_batch(1, Q[:n_q], K)
        fell, rounds = p.g.counter("vec_prefilter_fallbacks") - f0, p.g.counter("vec_overflow_rounds") - o0
        print("c-offset dim %d, vec_cand_cap 64: vec_overflow_rounds %d, fallbacks %d" % (dim, rounds, fell))
        assert rounds >= 1, "256 candidates per slab in segments of 64: the overflow rounds did not run"
        for i in range(n_q):
            d, l = p.ref(i)
            assert cnt[i] == d.size
            if fell:        # the fp32 MFMA scan answered
                fp32_scan_equal(p, i, dist, lab, cnt, "c-offset dim %d tiny segments" % dim, ulp_swaps=True)
            else:
                assert np.array_equal(lab[i, :d.size].astype(np.uint32), l) and np.array_equal(dist[i, :d.size].view(np.uint32), d.view(np.uint32)), i
    finally:
        p.close()


def body_giant_rows_come_and_go(lib, dim, n_q=4, sample_tiles=512):
    """family d through vec_upsert over existing labels: ordinary -> one giant row per tile -> ordinary again. The tile maxima must follow both ways:
    vec_candidate_rows (rows past the tile-level bound) rises to every ordinary row and comes back, vec_rescored_rows ends within 2x of the never-giant
    value. (sample_tiles = 512: a sample of 2 tiles holds 8 groups < k, L1 is -inf there and every row is a candidate whatever the maxima are)"""
    X0, Q = _scaled(1, 1)(dim)
    Xg, _ = _giant(dim)
    p = Pair(lib, X0, Q)
    try:
        what = "d-upsert dim %d" % dim
        r0 = bracket_run(p, n_q, sample_tiles, what + " never giant")
        c0 = p.g.counter("vec_candidate_rows")
        giants = np.arange(GIANT_AT, N, 128)
        p.upsert(giants, Xg[giants])
        bracket_run(p, n_q, sample_tiles, what + " giants upserted")
        c1 = p.g.counter("vec_candidate_rows")
        assert c1 >= (N - N_GIANT) * n_q and c1 > 2 * c0, "the tile maxima did not rise with the upserted giant rows (%d -> %d candidates)" % (c0, c1)
        p.upsert(giants, X0[giants])
        r2 = bracket_run(p, n_q, sample_tiles, what + " ordinary again")
        c2 = p.g.counter("vec_candidate_rows")
        assert c2 <= 2 * c0 and r2["rescored"] <= 2 * r0["rescored"], "stale tile maxima: candidates %d -> %d -> %d, re-scored %d -> %d" % (c0, c1, c2, r0["rescored"], r2["rescored"])
    finally:
        p.close()


NAN_ROWS, INF_ROWS = (1300, 1999), (3, 130, 700)


def finite_ranks_equal(g, orc_without_nan, Q, k, nan_labels, what=""):
    """flat_knn's comparator is not an order on NaN distances, so the oracle's place for a NaN row is unspecified: orc_without_nan holds every row
    except those (rows with an inf coordinate have a distance of +-inf and an ordinary rank). The library's top k + len(nan_labels) with the NaN
    rows dropped must be a prefix of at least k entries of the oracle's ranking: labels in order and distance bits."""
    kk = k + len(nan_labels)
    dist, lab, cnt = g.vec_knn_batch(1, Q, kk)
    for i in range(Q.shape[0]):
        assert cnt[i] == kk, (what, i, cnt[i])
        keep = ~np.isin(lab[i], np.asarray(nan_labels, np.uint64))
        d, l = orc_without_nan.flat_knn(Q[i], kk)
        m = int(keep.sum())
        assert m >= k
        assert np.array_equal(lab[i][keep].astype(np.uint32), l[:m]), (what, i)
        assert np.array_equal(dist[i][keep].view(np.uint32), d[:m].view(np.uint32)), (what, i)


def body_nonfinite(lib, dim, routes=ROUTES, n_qs=N_QS):
    """family g. ASSERTED ON THE FINITE PART (and the inf rows) ONLY: where a NaN-distance row appears is unspecified in the oracle (see finite_ranks_equal)"""
    X, Q = _scaled(1, 1)(dim)
    X[INF_ROWS[0], 3] = np.inf; X[INF_ROWS[1], dim - 1] = -np.inf; X[INF_ROWS[2], 17] = np.inf
    X[NAN_ROWS[0], 0] = np.nan; X[NAN_ROWS[1], dim - 2] = np.nan
    g = T.GpuIndex(0, lib)
    orc = O.OracleIndex(1, 1)
    try:
        g.set_option("vec_count_rescored", 1)
        g.vec_create(1, dim, B.METRIC_IP)
        g.vec_upsert(1, np.arange(N, dtype=np.uint64), X)
        orc.vec_init(dim, O.METRIC_IP)
        keep = ~np.isin(np.arange(N), NAN_ROWS)
        orc.vec_add(np.arange(N, dtype=np.uint32)[keep], X[keep])
        for st in routes:
            for n_q in n_qs:
                g.set_option("vec_sample_tiles", st)
                g0, f0 = g.counter("vec_prefilter_groups"), g.counter("vec_prefilter_fallbacks")
                finite_ranks_equal(g, orc, Q[:n_q], K, NAN_ROWS, "g dim %d n_q %d sample_tiles %d" % (dim, n_q, st))
                assert g.counter("vec_prefilter_groups") > g0 and g.counter("vec_prefilter_fallbacks") == f0
    finally:
        g.close()
        orc.close()


def body_fp32_scan(lib, name, dim, n_q=4):
    """vec_prefilter = 0 (fp32 MFMA scan of every row; not bit-exact): families a-e once, with fp32_scan_equal (_check_knn's assertions, + the
    oracle's label order where every row lies inside the band: asserted below for the eight scaled a / b cases). Where every distance is exactly
    1.0f the distance bits must match as well."""
    X, Q = CASES[name](dim)
    p = Pair(lib, X, Q)
    try:
        p.g.set_option("vec_prefilter", 0)
        p.g.set_option("vec_sample_tiles", 2)
        g0 = p.g.counter("vec_prefilter_groups")
        if name in FAMILY_A or name in FAMILY_B:
            assert (name == "a-mixed") != all(all_inside_band(p, i) for i in range(n_q)), name        # coverage: which cases get the order check
        if name in ALL_TIE:
            bad = p.wrong_queries(n_q)
            assert not bad, "%s dim %d fp32 scan: %d / %d queries differ from the oracle" % (name, dim, len(bad), n_q)
        else:
            dist, lab, cnt = p.g.vec_knn_batch(1, Q[:n_q], K)
            for i in range(n_q):
                fp32_scan_equal(p, i, dist, lab, cnt, "%s dim %d fp32 scan" % (name, dim), ulp_swaps=name == "c-offset")
        assert p.g.counter("vec_prefilter_groups") == g0
    finally:
        p.close()


def body_vector_search_with_filter(lib, dim=64, n_docs=700, n_q=3):
    """family i: rows and queries at 1e-4 through vector_search_batch with a filter, k-cut branch (the k-NN with an allow list = the bracket path with a
    row mask) and flat branch; keys, sort scores, distance bits, found and all_result_ids = the oracle's vector branch of Index::search"""
    docs = H.zipf_docs(n_docs, 30, 4, seed=6)
    orc, g = H.build_pair(docs, lib)
    try:
        n_vec = n_docs - 40
        X = (_gauss(6000 + dim, n_vec, dim) * 1e-4).astype(np.float32)
        Q = (_gauss(7000 + dim, n_q, dim) * 1e-4).astype(np.float32)
        g.vec_create(1, dim, B.METRIC_IP)
        g.vec_upsert(1, np.arange(n_vec, dtype=np.uint64), X)
        orc.vec_init(dim, O.METRIC_IP)
        orc.vec_add(np.arange(n_vec, dtype=np.uint32), X)
        filt = np.sort(np.random.default_rng(8).choice(n_docs, size=400, replace=False)).astype(np.uint32)
        allowed = filt[filt < n_vec]
        tied = 0
        for i in range(n_q):      # coverage, from the oracle: the k-cut of some query falls inside a run of equal distances
            d, _ = orc.flat_knn(Q[i], 31, allow_ids=allowed)
            tied += int(d[29:30].view(np.uint32)[0] == d[30:31].view(np.uint32)[0])
        assert tied, "no query ties at the k-th distance beyond k"
        osort = ((O.SORT_VECTOR_DISTANCE, 0, -1), (O.SORT_SEQ_ID, 0, 1))
        g0 = g.counter("vec_prefilter_groups")
        for cutoff, kw in ((0, dict(fetch_size=30)), (0, dict(fetch_size=300, k=7)), (len(filt) + 1, dict(fetch_size=30))):
            hits, ids = g.vector_search_batch(1, Q, k_stride=320, filter_ids=filt, flat_search_cutoff=cutoff, want_ids=True, **kw)
            assert (hits.status == 0).all()
            for i in range(n_q):
                ref = orc.search_vector(Q[i], sort=osort, filter_ids=filt, flat_search_cutoff=cutoff, cap=2048, ids_cap=n_docs, **kw)
                n = int(hits.n_hits[i])
                what = (cutoff, kw, i)
                assert n == ref.keys.size, what
                assert np.array_equal(hits.keys[i, :n], ref.keys), (what, hits.keys[i, :12], ref.keys[:12])
                assert np.array_equal(hits.scores[i, :n], ref.scores), what
                assert np.array_equal(hits.vector_distance[i, :n].view(np.uint32), ref.vector_distance.view(np.uint32)), what
                assert int(hits.num_matched[i]) == int(ref.n_result_ids), what
                assert np.array_equal(ids[i], ref.result_ids), what
        assert g.counter("vec_prefilter_groups") > g0 and g.counter("vec_prefilter_fallbacks") == 0
    finally:
        g.close()
        orc.close()
