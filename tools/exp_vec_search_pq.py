"""GPU experiment (not part of the product): one parameter block per query in a pure vector search batch (tsgpu_vector_search_batch_per_query) on
latent rows x 768 (inner product), 256 requests, EVERY request with its own filter list, fetch_size 10, k 100. Per case, in the same run and on the same
inputs:
  batch   one per-query call (host lists in, host results out);
  loop    what a caller had to do before: 256 tsgpu_vector_search_batch calls, one query and one parameter block each.
Cases: (a) flat lists of 5 000 ids, (b) k-cut lists of 5 000 ids, (c) k-cut lists of 10 % of the rows, (d) half (a) and half (b), interleaved.
The key checksums of `batch` and `loop` must agree. Writes its report to profiles/r07/exp_vec_search_pq.txt (or the path given with --out) and to stdout.
Usage: python tools/exp_vec_search_pq.py [n_rows] [--out FILE]"""
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
out_path = os.path.join(ROOT, "profiles", "r07", "exp_vec_search_pq.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = os.path.abspath(args[i + 1])
    del args[i:i + 2]
n = int(args[0]) if args else 2_000_000
dim, k, NQ, SMALL = 768, 100, 256, 5000
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
del X, lab
g.set_num_docs(n)
g.commit()
say("rows %d x %d, inner product | %d requests, each with its own filter list, fetch_size 10, k %d | host lists in, host results out" % (n, dim, NQ, k))
Qh = synth.latent_vectors(NQ, dim, seed=4, device="cuda").cpu().numpy()


def lists_of(count, size, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return [torch.randperm(n, generator=gen, device="cuda")[:size].sort().values.to(torch.int32).cpu().numpy().view(np.uint32) for _ in range(count)]


def checksum(hits):
    return int(sum(int(hits.keys[i, :hits.n_hits[i]].sum()) for i in range(hits.n_hits.size)) % (1 << 61)), int(hits.n_hits.sum()), int((hits.status != 0).sum())


def batch(params):
    return g.vector_search_batch_per_query(1, Qh, params, k_stride=250)


def loop(params):
    out = T.Hits(NQ, 250)
    for i, p in enumerate(params):
        h = g.vector_search_batch(1, Qh[i:i + 1], k_stride=250, **p)
        nh = int(h.n_hits[0])
        out.keys[i, :nh], out.n_hits[i], out.status[i] = h.keys[0, :nh], nh, h.status[0]
    return out


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


COUNTERS = ("vec_search_pq_flat_queries", "vec_search_pq_kcut_queries", "vec_search_pq_flat_lists", "vec_search_pq_flat_launches", "vec_prefilter_groups",
            "vec_prefilter_fallbacks", "vec_filter_direct_queries", "vec_filter_scan_queries")
flat = lambda a: dict(fetch_size=10, k=k, filter_ids=a, flat_search_cutoff=a.size + 1)
kcut = lambda a: dict(fetch_size=10, k=k, filter_ids=a)
small, tenth = lists_of(NQ, SMALL, 12), lists_of(NQ, n // 10, 13)
for name, params, steps in (("(a) 256 flat lists of %d ids" % SMALL, [flat(a) for a in small], 5),
                            ("(b) 256 k-cut lists of %d ids" % SMALL, [kcut(a) for a in small], 5),
                            ("(c) 256 k-cut lists of 10 %% of the rows (%d ids)" % (n // 10), [kcut(a) for a in tenth], 3),
                            ("(d) half and half: 128 flat and 128 k-cut lists of %d ids, interleaved" % SMALL, [(flat if i % 2 else kcut)(a) for i, a in enumerate(small)], 5)):
    c0 = {c: g.counter(c) for c in COUNTERS}
    hb, tb = timed(lambda: batch(params), steps)
    c1 = {c: g.counter(c) for c in COUNTERS}
    calls = steps + 1
    hl, tl = timed(lambda: loop(params), 1)
    say(name)
    say("  batch: %s | per call: %s | checksum %s" % (fmt(tb), ", ".join("%s %.1f" % (c[4:] if c.startswith("vec_") else c, (c1[c] - c0[c]) / calls) for c in COUNTERS), checksum(hb)))
    say("  loop of 256 single-block calls: %s | checksum %s" % (fmt(tl), checksum(hl)))
    say("  batch / loop: %.2fx the loop's throughput%s" % (np.mean(tl) / np.mean(tb), "" if checksum(hb) == checksum(hl) else " | CHECKSUMS DIFFER"))
g.close()
report.close()
