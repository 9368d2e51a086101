"""GPU experiment (not part of the product): per-query filters in one HNSW search batch (tsgpu_vec_hnsw_search_batch_filtered) on the bench's HNSW shape
— latent rows x 768, M 16, the graph built on the device (tsgpu_vec_hnsw_build), k = 100 — with 256 queries at ef 400 and 256 DISTINCT allow lists of
(a) 10 % and (b) 50 % of the rows, and (c) every row allowed. Per case, on the same build and the same inputs:
  batch   one filtered batch (host lists in, host results out);
  loop    what a caller had to do before: 256 single-filter tsgpu_vec_hnsw_search_batch calls, one query each;
and the unfiltered 256-query batch (host in, host out) as the ceiling. The label checksums of `batch` and `loop` must agree.
Writes its report to profiles/r07/exp_hnsw_filtered.txt (or the path given with --out) and to stdout.
Usage: python tools/exp_hnsw_filtered.py [n_rows] [--out FILE]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import typesense_amd as T  # noqa: E402
from typesense_amd import _lib as B, synth  # noqa: E402

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r07", "exp_hnsw_filtered.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = os.path.abspath(args[i + 1])
    del args[i:i + 2]
n = int(args[0]) if args else 2_000_000
dim, k, ef, M, NQ = 768, 100, 400, 16, 256
os.makedirs(os.path.dirname(out_path), exist_ok=True)
report = open(out_path, "w")


def say(line):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


g = T.GpuIndex(0)
X = synth.latent_vectors(n, dim, seed=3, device="cuda")
g.vec_create(1, dim, B.METRIC_IP, n)
lab = torch.arange(n, dtype=torch.int64, device="cuda")
g.vec_upsert_device(1, lab.data_ptr(), X.data_ptr(), n)
torch.cuda.synchronize()
t0 = time.perf_counter()
info = g.vec_hnsw_build(1, M=M, ef_construction=200, seed=100, threads=16)
del X, lab
say("rows %d x %d | M %d, ef_construction 200, built on the device in %.1f s (%d seed rows) | %d queries, k %d, ef %d | host lists in, host results out"
    % (n, dim, M, time.perf_counter() - t0, info["n_seed"], NQ, k, ef))
Qh = synth.latent_vectors(NQ, dim, seed=4, device="cuda").cpu().numpy()


def allow_lists(count, size, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return [torch.randperm(n, generator=gen, device="cuda")[:size].sort().values.to(torch.int32).cpu().numpy().view(np.uint32) for _ in range(count)]


def checksum(lab, cnt):
    ok = cnt != 0xFFFFFFFF
    return int(sum(int(lab[i, :cnt[i]].sum()) for i in np.nonzero(ok)[0]) % (1 << 61)), int(cnt[ok].sum()), int((~ok).sum())


def batch(lists):
    return g.vec_hnsw_search_batch_filtered(1, Qh, k, ef, None if lists is None else [(a, None) for a in lists])


def loop(lists):
    dist = np.zeros((NQ, k), np.float32); lab = np.zeros((NQ, k), np.uint64); cnt = np.zeros(NQ, np.uint32)
    for i, a in enumerate(lists):
        d, l, c = g.vec_hnsw_search_batch(1, Qh[i:i + 1], k, ef, allow_ids=a)
        dist[i], lab[i], cnt[i] = d[0], l[0], c[0]
    return dist, lab, cnt


def timed(fn, steps):
    fn()                                                  # warm-up (allocations, code objects)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()                                        # (every entry point ends in a stream synchronise: the results are on the host)
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def fmt(ts):
    return "%.2f ms (min %.2f max %.2f, %d steps) = %.0f q/s" % (float(np.mean(ts)), min(ts), max(ts), len(ts), NQ / (np.mean(ts) * 1e-3))


COUNTERS = ("hnsw_launches", "hnsw_tier_reruns", "hnsw_filter_maps", "vec_filter_h2d_bytes")
(dist, labs, cnt), ts = timed(lambda: batch(None), 5)
say("unfiltered batch (the ceiling): %s | expansions / query %.0f, distances / query %.0f | checksum %s"
    % (fmt(ts), g.counter("hnsw_last_expansions") / NQ, g.counter("hnsw_last_distances") / NQ, checksum(labs, cnt)))
every = np.arange(n, dtype=np.uint32)
for name, make, steps in (("(a) 256 distinct lists of 10 %% of the rows (%d ids)" % (n // 10), lambda: allow_lists(NQ, n // 10, 12), 3),
                          ("(b) 256 distinct lists of 50 %% of the rows (%d ids)" % (n // 2), lambda: allow_lists(NQ, n // 2, 13), 3),
                          ("(c) every row allowed, 256 lists of %d ids" % n, lambda: [every] * NQ, 3)):
    lists = make()
    c0 = {c: g.counter(c) for c in COUNTERS}
    (dist, labs, cnt), ts = timed(lambda: batch(lists), steps)
    c1 = {c: g.counter(c) for c in COUNTERS}
    calls = steps + 1
    say("%s" % name)
    say("  batch: %s | per batch: launches %.1f, queries re-run %.1f, maps %d, id lists uploaded %.1f MB | expansions / query %.0f, distances / query %.0f | checksum %s"
        % (fmt(ts), (c1["hnsw_launches"] - c0["hnsw_launches"]) / calls, (c1["hnsw_tier_reruns"] - c0["hnsw_tier_reruns"]) / calls,
           (c1["hnsw_filter_maps"] - c0["hnsw_filter_maps"]) // calls, (c1["vec_filter_h2d_bytes"] - c0["vec_filter_h2d_bytes"]) / calls / 1e6,
           g.counter("hnsw_last_expansions") / NQ, g.counter("hnsw_last_distances") / NQ, checksum(labs, cnt)))
    g.set_option("vec_count_rescored", 1)                 # (the stage / build timers cost a sync per group: measured in a run of their own)
    s0, b0 = g.counter("vec_filter_stage_us"), g.counter("vec_filter_build_us")
    t0 = time.perf_counter()
    batch(lists)
    total = (time.perf_counter() - t0) * 1e3
    stage, build = (g.counter("vec_filter_stage_us") - s0) / 1e3, (g.counter("vec_filter_build_us") - b0) / 1e3
    g.set_option("vec_count_rescored", 0)
    say("  batch, where the time goes (one more run): list staging + upload %.2f ms, bitmap build kernel %.2f ms, the rest (traversal, results to the host, "
        "binding) %.2f ms of %.2f ms" % (stage, build, total - stage - build, total))
    (dist, labs, cnt), ts = timed(lambda: loop(lists), 1)
    say("  loop of 256 single-filter calls: %s | checksum %s" % (fmt(ts), checksum(labs, cnt)))
    del lists
g.close()
report.close()
