"""Measures the sort-key slots (TSGPU_SORT_EVAL, _INT64_COLUMN_MISSING_FIRST, _STRING_RANK_FLIP) on the 10M-document synthetic collection with the headline's
10 000-query 3-token batch, against the (_text_match, points) sort of the headline on the same tree. Run it on the parent commit with --baseline-only (twice:
the run-to-run spread) and on this tree; the no-regression pair is `text_match_points`. Writes one JSON document (default profiles/r07/sort_keys.json).

    python tools/exp_sort_keys.py [--docs 10000000] [--queries 10000] [--steps 25] [--warmup 5] [--baseline-only] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import typesense_amd as T                                   # noqa: E402
from typesense_amd import _lib as B, synth                  # noqa: E402
from typesense_amd import build as BUILD                    # noqa: E402


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
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r07", "sort_keys.json"))
    a = ap.parse_args()
    BUILD.build()
    n = a.docs
    csr = synth.zipf_corpus_csr(n, 20000, 16, seed=1)
    pts = synth.points_column(n)
    g = T.GpuIndex(0)
    g.field_create(0, False)
    g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
    g.column_set(0, pts)
    g.set_num_docs(n)
    g.commit()
    qtok = synth.keyword_queries(a.queries, 3, 2, 60, seed=9)
    TM = (B.SORT_TEXT_MATCH, 1, 0)
    hits = T.Hits(a.queries, 250)
    hs = hits.c_struct()
    res = {"docs": n, "queries": a.queries, "legs": {}, "key_latency_ms": {}}

    def leg(name, sort):
        arr = T.index.make_query_array([T.KwQuery(q, sort=sort, topster_size=250) for q in qtok])
        res["legs"][name] = timed(g, arr, a.queries, hs, a.steps, a.warmup)
        assert (hits.status == 0).all(), name
        print(name, res["legs"][name], flush=True)

    leg("text_match_points", (TM, (B.SORT_INT64_COLUMN, 1, 0)))
    if not a.baseline_only:
        rng = np.random.default_rng(4)
        half = np.flatnonzero(rng.random(n) < 0.5).astype(np.uint32)
        two = np.flatnonzero(rng.random(n) < 0.02).astype(np.uint32)
        small = np.sort(rng.choice(n, size=1000, replace=False)).astype(np.uint32)
        keys = {"eval_dense_50pct": ([half], [5]), "eval_dense_2pct": ([two], [5]), "eval_sparse_1000": ([small], [5]),
                "eval_8_expressions": ([np.flatnonzero(rng.random(n) < 0.05).astype(np.uint32) for _ in range(8)], list(range(8, 0, -1)))}
        for name, (lists, scores) in keys.items():
            h = g.sort_key_create_eval(lists, scores)
            leg(name, ((B.SORT_EVAL, 1, h), TM))
            g.sort_key_destroy(h)
        leg("points_missing_first", ((B.SORT_INT64_COLUMN_MISSING_FIRST, 1, 0), TM))
        leg("points_as_rank_flip", ((B.SORT_STRING_RANK_FLIP, -1, 0), TM))
        base = res["legs"]["text_match_points"]["median_ms"]
        res["ratio_to_column_sort"] = {k: v["median_ms"] / base for k, v in res["legs"].items()}
        five_m = half[:5_000_000]
        for name, ids in (("1000_ids", small), ("5M_ids", five_m)):
            c, d = [], []
            for _ in range(10):
                t0 = time.perf_counter()
                h = g.sort_key_create_eval([ids], [1])
                t1 = time.perf_counter()
                g.sort_key_destroy(h)
                c.append((t1 - t0) * 1e3)
                d.append((time.perf_counter() - t1) * 1e3)
            res["key_latency_ms"][name] = {"create_median": float(np.median(c)), "destroy_median": float(np.median(d))}
    g.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
