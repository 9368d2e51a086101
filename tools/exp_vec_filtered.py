"""GPU experiment (not part of the product): per-query filters in one exact k-NN batch (tsgpu_vec_knn_batch_filtered) and in the hybrid batch that runs
on it — 256 queries, k = 100, 768 dims: (a) 256 distinct allow lists of 5 000 ids (direct route), (b) 256 distinct lists of 10 % of the rows (masked
scan), (c) n_q = 1 with each size, and the unfiltered 256-query scan. Warm-up + timing as tools/exp_vec.py.
Usage: python tools/exp_vec_filtered.py [n_rows] [--pkg DIR] [--no-hybrid]
  --pkg DIR  import typesense_amd from DIR (a checkout of another commit with its own libtsgpu.so). A package without vec_knn_batch_filtered is measured
             the way its callers had to work: one single-filter tsgpu_vec_knn_batch per query. Inputs are drawn from fixed seeds: identical in both runs;
             the label checksums printed per case must agree between the two."""
import os
import sys
import time

import numpy as np
import torch

args = sys.argv[1:]
pkg = None
if "--pkg" in args:
    i = args.index("--pkg")
    pkg = os.path.abspath(args[i + 1])
    del args[i:i + 2]
hybrid = "--no-hybrid" not in args
args = [a for a in args if a != "--no-hybrid"]
sys.path.insert(0, pkg or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import typesense_amd as T  # noqa: E402
from typesense_amd import _lib as B, synth  # noqa: E402

n = int(args[0]) if args else 4_000_000
dim, k, NQ = 768, 100, 256
K_TOPSTER = 250
g = T.GpuIndex(0)
batched = hasattr(g, "vec_knn_batch_filtered")
print("package: %s | rows %d x %d | k %d | %s" % ("the other checkout (--pkg)" if pkg else "this checkout", n, dim, k,
                                              "one filtered batch" if batched else "no batched filters: one single-filter call per query"), flush=True)
g.vec_create(1, dim, B.METRIC_IP, n)
S = 1 << 20
for a in range(0, n, S):
    b = min(n, a + S)
    x = synth.random_vectors(b - a, dim, seed=3 + a, device="cuda")
    lab = torch.arange(a, b, dtype=torch.int64, device="cuda")
    g.vec_upsert_device(1, lab.data_ptr(), x.data_ptr(), b - a)
    del x
torch.cuda.synchronize()
Q = synth.random_vectors(1024, dim, seed=4, device="cuda")
Qh = Q[:NQ].cpu().numpy()


def allow_lists(count, size, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return [torch.randperm(n, generator=gen, device="cuda")[:size].sort().values.to(torch.int32).cpu().numpy().view(np.uint32) for _ in range(count)]


def checksum(lab, cnt):
    return int(sum(int(lab[i, :cnt[i]].sum()) for i in range(cnt.size)) % (1 << 61)), int(cnt.sum())


def knn_filtered(Qn, lists):
    if batched:
        return g.vec_knn_batch_filtered(1, Qn, k, [(a, None) for a in lists])
    dist = np.zeros((len(lists), k), np.float32); lab = np.zeros((len(lists), k), np.uint64); cnt = np.zeros(len(lists), np.uint32)
    for i, a in enumerate(lists):
        d, l, c = g.vec_knn_batch(1, Qn[i:i + 1], k, allow_ids=a)
        dist[i], lab[i], cnt[i] = d[0], l[0], c[0]
    return dist, lab, cnt


def timed(fn, steps):
    fn()                                                  # warm-up (allocations)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def fmt(ts):
    return "%.2f ms (min %.2f max %.2f, %d steps)" % (float(np.mean(ts)), min(ts), max(ts), len(ts))


def counters():
    return {c: g.counter(c) for c in ("vec_filter_h2d_bytes", "vec_filter_build_us", "vec_filter_direct_queries", "vec_filter_scan_queries",
                                      "vec_prefilter_groups", "vec_prefilter_fallbacks", "vec_overflow_rounds")} if batched else \
           {c: g.counter(c) for c in ("vec_prefilter_groups", "vec_prefilter_fallbacks", "vec_overflow_rounds")}


# ---- the unfiltered 256-query exact k-NN (device in, device out): must not move
d = torch.zeros((NQ, k), dtype=torch.float32, device="cuda"); l = torch.zeros((NQ, k), dtype=torch.int64, device="cuda"); c = torch.zeros(NQ, dtype=torch.int32, device="cuda")
scan, step = [], []
for it in range(9):
    t0 = time.perf_counter()
    g.vec_knn_batch_raw(1, Q.data_ptr(), B.MEM_DEVICE, NQ, k, d.data_ptr(), l.data_ptr(), c.data_ptr(), B.MEM_DEVICE)
    if it:
        step.append((time.perf_counter() - t0) * 1e3); scan.append(g.timings().vec_scan_ms)
print("unfiltered B=256: scan %.3f ms (min %.3f max %.3f, 8 steps) | step %s" % (float(np.mean(scan)), min(scan), max(scan), fmt(step)), flush=True)

# ---- plain filtered k-NN, host lists, host results
small, big = allow_lists(NQ, 5000, 11), allow_lists(NQ, n // 10, 12)
for name, lists, steps in (("(a) 256 x 5000 ids", small, 3), ("(b) 256 x 10%% of the rows (%d ids)" % (n // 10), big, 2)):
    c0 = counters()
    (dist, lab, cnt), ts = timed(lambda: knn_filtered(Qh, lists), steps)
    c1 = counters()
    line = "knn %s: %s = %.0f q/s | checksum %s" % (name, fmt(ts), NQ / (np.mean(ts) * 1e-3), checksum(lab, cnt))
    if batched:
        calls = len(ts) + 1
        line += " | id lists uploaded %.1f MB per batch" % ((c1["vec_filter_h2d_bytes"] - c0["vec_filter_h2d_bytes"]) / calls / 1e6)
        g.set_option("vec_count_rescored", 1)             # (the build timer costs a sync per group: measured in a run of its own)
        s0, b0 = g.counter("vec_filter_stage_us"), g.counter("vec_filter_build_us")
        knn_filtered(Qh, lists)
        line += ", staging + upload %.2f ms, bitmap / survivor build kernels %.2f ms" % ((g.counter("vec_filter_stage_us") - s0) / 1e3, (g.counter("vec_filter_build_us") - b0) / 1e3)
        g.set_option("vec_count_rescored", 0)
    print(line + " | " + " ".join("%s +%d" % (kk, c1[kk] - c0[kk]) for kk in c1 if not kk.startswith("vec_filter_h2d") and not kk.startswith("vec_filter_build")), flush=True)
for name, lists in (("(c) n_q = 1, 5000 ids", small[:1]), ("(c) n_q = 1, 10% of the rows", big[:1])):
    (dist, lab, cnt), ts = timed(lambda: knn_filtered(Qh[:1], lists), 5)
    print("knn %s: %s | checksum %s" % (name, fmt(ts), checksum(lab, cnt)), flush=True)

# ---- hybrid: the same filters as filter_ids of the keyword queries (bench.py's corpus recipe and query stream)
if hybrid:
    vocab, tpd = (100_000, 32) if n >= 1_000_000 else (20_000, 16)
    csr = synth.zipf_corpus_csr(n, vocab, tpd, seed=2)
    g.field_create(0, False)
    g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
    g.column_set(0, synth.points_column(n))
    g.set_num_docs(n)
    g.commit()
    del csr
    sort = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
    qtok = synth.keyword_queries(NQ, 3, 8, 2000, seed=5)

    def hyb(lists, nq):
        qs = [T.KwQuery(qtok[i], sort=sort, topster_size=K_TOPSTER, **({} if lists is None else {"filter_ids": lists[i]})) for i in range(nq)]
        return g.hybrid_search_batch(qs, 1, Qh[:nq], k=k, fetch_size=100, alpha=0.3, k_stride=K_TOPSTER)
    for name, lists, nq, steps in (("unfiltered B=256", None, NQ, 3), ("(a) 256 x 5000 ids", small, NQ, 3), ("(b) 256 x 10% of the rows", big, NQ, 2),
                                   ("(c) n_q = 1, 5000 ids", small, 1, 5), ("(c) n_q = 1, 10% of the rows", big, 1, 5)):
        hits, ts = timed(lambda: hyb(lists, nq), steps)
        cs = int(sum(int(hits.keys[i, :int(hits.n_hits[i])].sum()) for i in range(nq))), int(hits.n_hits[:nq].sum())
        print("hybrid %s: %s = %.0f q/s | checksum %s" % (name, fmt(ts), nq / (np.mean(ts) * 1e-3), cs), flush=True)
g.close()
