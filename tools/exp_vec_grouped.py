"""GPU experiment (not part of the product): group_by for the pure vector search (tsgpu_vector_search_grouped_batch) on latent rows x 768 (inner
product), 256 requests, EVERY request with its own filter list of 5 000 ids, fetch_size 10, k 100, group_limit 3, a distinct-key column of 1 000 values.
Per batch — (a) flat lists, (b) k-cut lists, (c) half of each, interleaved — in the same run and on the same inputs:
  ungrouped     tsgpu_vector_search_batch_per_query (the entry point this work leaves unchanged);
  first pass    the grouped call with first_pass = 1;
  second pass   the grouped call with first_pass = 0.
Median of 10 repetitions after 3 warm-ups, host lists in, host results out (every call ends in a stream synchronise). The difference grouped - ungrouped is
what grouping adds; "count sync" is the host time of the grouped call's one extra stream synchronise (counter vec_grouped_sync_us), a wait that also covers
the distance launches and the compaction queued before it — an upper bound of what the download and the sync themselves cost.
Writes its report to profiles/r07/exp_vec_grouped.txt (or the path given with --out) and to stdout.
Usage: python tools/exp_vec_grouped.py [n_rows] [--out FILE]"""
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
out_path = os.path.join(ROOT, "profiles", "r07", "exp_vec_grouped.txt")
if "--out" in args:
    i = args.index("--out")
    out_path = os.path.abspath(args[i + 1])
    del args[i:i + 2]
n = int(args[0]) if args else 2_000_000
dim, k, NQ, SMALL, GROUP_LIMIT, N_VALUES, WARM, REPS = 768, 100, 256, 5000, 3, 1000, 3, 10
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
g.column_set(1, ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(N_VALUES) + np.uint64(1)).view(np.int64))
g.commit()
say("rows %d x %d, inner product | %d requests, each with its own list of %d ids, fetch_size 10, k %d, group_limit %d, %d distinct keys | median of %d after %d warm-ups"
    % (n, dim, NQ, SMALL, k, GROUP_LIMIT, N_VALUES, REPS, WARM))
Qh = synth.latent_vectors(NQ, dim, seed=4, device="cuda").cpu().numpy()
gen = torch.Generator(device="cuda")
gen.manual_seed(12)
lists = [torch.randperm(n, generator=gen, device="cuda")[:SMALL].sort().values.to(torch.int32).cpu().numpy().view(np.uint32) for _ in range(NQ)]


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts)), min(ts), max(ts)


flat = lambda a: dict(fetch_size=10, k=k, filter_ids=a, flat_search_cutoff=a.size + 1)
kcut = lambda a: dict(fetch_size=10, k=k, filter_ids=a)
for name, params in (("(a) 256 flat lists", [flat(a) for a in lists]), ("(b) 256 k-cut lists", [kcut(a) for a in lists]),
                     ("(c) 128 flat and 128 k-cut lists, interleaved", [(flat if i % 2 else kcut)(a) for i, a in enumerate(lists)])):
    say(name)
    hu, mu, lo, hi = timed(lambda: g.vector_search_batch_per_query(1, Qh, params, k_stride=250))
    say("  ungrouped:   %.2f ms (min %.2f max %.2f) | %d hits, %d refused" % (mu, lo, hi, int(hu.n_hits.sum()), int((hu.status != 0).sum())))
    for first_pass in (1, 0):
        groups = [(GROUP_LIMIT, 1, first_pass, 0)] * NQ
        s0, u0, i0 = g.counter("vec_grouped_syncs"), g.counter("vec_grouped_sync_us"), g.counter("vec_grouped_items")
        (h, gh), m, lo, hi = timed(lambda: g.vector_search_grouped_batch(1, Qh, params, groups, k_stride=250 * GROUP_LIMIT, g_stride=250))
        calls = WARM + REPS
        syncs, sync_ms, items = (g.counter("vec_grouped_syncs") - s0) / calls, (g.counter("vec_grouped_sync_us") - u0) / calls * 1e-3, (g.counter("vec_grouped_items") - i0) / calls
        a = g.aux_timings()
        share = "%.0f %% of the difference" % (100.0 * sync_ms / (m - mu)) if m > mu else "the grouped call is not the slower one: no difference to take a share of"
        say("  %s pass: %.2f ms (min %.2f max %.2f) = %.2fx ungrouped, %+.2f ms | %d groups, %d hits, %d items, %d refused | per call: %.1f count syncs, %.3f ms waiting in them"
            " (%s) | last call: group kernels %.2f ms" % ("first " if first_pass else "second", m, lo, hi, m / mu, m - mu, int(gh.n_groups.sum()), int(h.n_hits.sum()),
                                                          items, int((h.status != 0).sum()), syncs, sync_ms, share, a.gb_kernels_ms))
g.close()
report.close()
