"""Measures the `_vector_query(...)` sort slot (TSGPU_SORT_VECTOR_QUERY, kw_vq_sort.hip.h): the synth.py corpus at 1M documents with a 768-d `ip` vector field, a
256-query batch of two-token AND queries, top-100, sorted once by (_text_match, int64 column) and once by (_text_match, _vector_query). Reports the added
milliseconds, distances per second (one per emitted hit = sum of num_matched), bytes of rows read per second against the HBM figure, and what ONE host thread
needs for tsgpu_ip_distance over the same matched ids — what the reference pays in Index::compute_sort_scores. Prints one JSON document.

    python tools/exp_vq_sort.py [--docs 1000000] [--dim 768] [--queries 256] [--steps 20] [--warmup 3] [--host-sample 100000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import typesense_amd as T                                   # noqa: E402
from typesense_amd import _lib as B, synth                  # noqa: E402
from typesense_amd import build as BUILD                    # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X: 8.0 TB/s spec (the figure bench.py's rooflines use)


def timed(g, arr, n, hs, steps, warmup):
    for _ in range(warmup):
        g.keyword_search_batch_raw(arr, n, hs)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        g.keyword_search_batch_raw(arr, n, hs)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "p90_ms": float(np.percentile(ts, 90)), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=100_000)
    a = ap.parse_args()
    import torch
    BUILD.build()
    n, dim = a.docs, a.dim
    csr = synth.zipf_corpus_csr(n, 20000, 16, seed=1)
    g = T.GpuIndex(0)
    g.field_create(0, False)
    g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
    g.column_set(0, synth.points_column(n))
    g.set_num_docs(n)
    g.commit()
    X = synth.random_vectors(n, dim, seed=3, device="cuda").contiguous()
    labels = torch.arange(0, n, dtype=torch.int64, device="cuda")
    g.vec_create(1, dim, B.METRIC_IP, n)
    g.vec_upsert_device(1, labels.data_ptr(), X.data_ptr(), n)
    torch.cuda.synchronize()
    q = np.random.default_rng(7).standard_normal(dim).astype(np.float32)
    key = g.sort_key_create_vector_query(1, q)
    qtok = synth.keyword_queries(a.queries, 2, 2, 60, seed=9)
    TM = (B.SORT_TEXT_MATCH, 1, 0)
    hits = T.Hits(a.queries, 100)
    hs = hits.c_struct()
    res = {"docs": n, "dim": dim, "queries": a.queries, "legs": {}}
    for name, sort in (("text_match_column", (TM, (B.SORT_INT64_COLUMN, 1, 0))), ("text_match_vector_query", (TM, (B.SORT_VECTOR_QUERY, -1, key)))):
        arr = T.index.make_query_array([T.KwQuery(t, sort=sort, topster_size=100) for t in qtok])
        res["legs"][name] = timed(g, arr, a.queries, hs, a.steps, a.warmup)
        assert (hits.status == 0).all(), name
        print(name, res["legs"][name], flush=True)
    matched = int(hits.num_matched.sum())
    added_ms = res["legs"]["text_match_vector_query"]["median_ms"] - res["legs"]["text_match_column"]["median_ms"]
    res["distances_per_batch"] = matched
    res["added_ms"] = added_ms
    if added_ms > 0:
        res["distances_per_s"] = matched / (added_ms * 1e-3)
        res["row_bytes_per_s"] = res["distances_per_s"] * dim * 4
        res["fraction_of_hbm_peak"] = res["row_bytes_per_s"] / (HBM_PEAK_GBS * 1e9)
    # the reference's cost: one thread, one dist_func per matched document (rows already in host memory)
    ids = np.unique(np.concatenate([synth.csr_term(csr, int(t))[0] for t in np.unique(qtok)]))[: a.host_sample]
    rows = X[torch.from_numpy(ids.astype(np.int64)).cuda()].cpu().numpy()
    fn, qp, base, stride = g.L.tsgpu_ip_distance, q.ctypes.data, rows.ctypes.data, dim * 4
    t0 = time.perf_counter()
    for i in range(ids.size):
        fn(qp, base + i * stride, dim, 4)
    t_full = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(ids.size):
        fn(qp, base + i * stride, 0, 4)
    t_call = time.perf_counter() - t0                        # the ctypes call itself (dim = 0): not the reference's cost
    per = max(t_full - t_call, 0.0) / max(ids.size, 1)
    res["host_one_thread"] = {"sample": int(ids.size), "us_per_distance": per * 1e6, "ms_for_the_batch": per * matched * 1e3}
    g.sort_key_destroy(key)
    g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
