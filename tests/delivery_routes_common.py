"""Shared body of tests/test_emu_delivery_routes.py (CPU tier, SIMT emulator) and tests/test_gpu_delivery_routes.py (-m gpu, libtsgpu.so): a keyword
batch's results reach the caller by one of several routes chosen in the host code of kw_batch_on_lane (typesense_amd/csrc/tsgpu.hip), and every route
must hand over the same bits.

  device output    mem = MEM_DEVICE, every tsgpu_hits array present: the merge kernel writes the caller's arrays (the reference run)
  zero-copy image  host output, n <= kw_zero_copy_max_queries and an image of <= 8 MiB: the merge kernel writes ONE result image into the lane's
                   pinned host buffer, the live rows are copied out of it
  staged image     host output with kw_zero_copy_max_queries = 0: the image is built in device memory, one copy into the pinned buffer, live rows copied out
  sliced           host output with kw_host_split_queries = 7: kw_split_host serves the batch as two batches on two lanes (kw_batches + 2)
  direct copies    an image of more than 8 MiB (190 queries x k_stride 1000 x 45 B = 8 550 000 B > 8 388 608 B): seven copies to the caller's arrays

The corpus is the 3000-document Zipf collection of tests/test_emu_keyword.py (the routes are host code: the smallest corpus whose queries are still cut
into several work items). Rows behind n_hits are undefined (include/tsgpu.h) and are not compared."""
import ctypes as C

import numpy as np

import typesense_amd as T
from typesense_amd import _lib as B
from tests import helpers as H

SORT = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
ARRAYS = ("keys", "scores", "text_match", "vector_distance", "match_score_index", "n_hits", "num_matched", "status", "search_cutoff")
ROW_ARRAYS = ("keys", "scores", "text_match", "vector_distance", "match_score_index")
N_A, KS_A = 53, 250
N_B, KS_B = 190, 1000
IMAGE_LIMIT = 8 << 20                       # both image routes end here (kw_batch_on_lane)
ROW_BYTES = 8 + 24 + 8 + 4 + 1              # keys, scores x 3, text_match, vector_distance, match_score_index


class World:
    def __init__(self, lib_path):
        self.docs = H.zipf_docs(3000, 300, 12, seed=1)
        self.orc, self.g = H.build_pair(self.docs, lib_path)
        self.on_gpu = "emu" not in self.g.lib_path

    def close(self):
        self.g.close()
        self.orc.close()


def make_queries(n, seed):
    """the batch of test_host_output_batch_served_in_slices_equals_the_single_batch: 1-3 tokens, every fourth query with 500 filter ids and a Topster of 40,
    Topsters of 17 and 250, one 12-token query (fails alone), queries whose tokens match nothing"""
    rng = np.random.default_rng(seed)
    qs = []
    for rep in range(n):
        toks = rng.choice(np.arange(1, 30), size=int(rng.integers(1, 4)), replace=False)
        if rep % 4 == 1: qs.append(T.KwQuery(toks, sort=SORT, topster_size=40, filter_ids=np.sort(rng.choice(3000, size=500, replace=False))))
        elif rep == 30: qs.append(T.KwQuery(list(range(1, 13)), sort=SORT))            # too many tokens: fails alone
        elif rep % 19 == 7: qs.append(T.KwQuery([100000 + rep, 200000 + rep][:1 + rep % 2], sort=SORT, topster_size=250))     # tokens the index does not hold
        else: qs.append(T.KwQuery(toks, sort=SORT, topster_size=250 if rep % 3 else 17))
    return qs


def search_device_output(w, qs, k_stride):
    """the batch with mem = MEM_DEVICE and every array present -> a host copy (T.Hits). The emulator's "device" memory is numpy memory; on the GPU the
    arrays are torch device tensors (as test_device_shard_merge_* does on each tier)."""
    n = len(qs)
    hits = T.Hits(n, k_stride)
    hs = hits.c_struct()
    hs.mem = B.MEM_DEVICE
    dev = {}
    if w.on_gpu:
        import torch
        for name in ARRAYS:
            a = getattr(hits, name)
            dev[name] = torch.zeros(a.shape, dtype=getattr(torch, str(a.dtype).replace("uint64", "int64").replace("uint32", "int32")), device="cuda")
            setattr(hs, name, dev[name].data_ptr())
        torch.cuda.synchronize()
    arr = T.index.make_query_array(qs)
    w.g.keyword_search_batch_raw(arr, n, hs)
    for name, t in dev.items():
        getattr(hits, name)[...] = t.cpu().numpy().view(getattr(hits, name).dtype)
    return hits


def assert_same_bits(ref, got, what):
    for name in ("status", "n_hits", "num_matched", "search_cutoff"):
        assert np.array_equal(getattr(ref, name), getattr(got, name)), "%s: %s differs" % (what, name)
    for i in range(ref.n_queries):
        n = int(ref.n_hits[i])
        for name in ROW_ARRAYS:
            a, b = getattr(ref, name)[i, :n], getattr(got, name)[i, :n]
            assert a.tobytes() == b.tobytes(), "%s q%d: %s differs" % (what, i, name)


def assert_reference_equals_oracle(w, qs, ref, what):
    checked = 0
    for i, q in enumerate(qs):
        if ref.status[i] == 0:
            H.assert_hits_equal(ref, i, H.oracle_keyword(w.orc, q), what)
            checked += int(ref.n_hits[i])
    assert checked > 1000, (what, checked)


def body_small_batch_every_route(w):
    """query set A (53 queries, k_stride 250): device output, zero-copy image, staged image, sliced"""
    g = w.g
    qs = make_queries(N_A, seed=99)
    assert N_A <= 256 and N_A * KS_A * ROW_BYTES <= IMAGE_LIMIT
    try:
        r0 = g.counter("kw_batches")
        ref = search_device_output(w, qs, KS_A)
        assert g.counter("kw_batches") - r0 == 1
        zero_copy = g.keyword_search_batch(qs, k_stride=KS_A)                          # defaults: n <= kw_zero_copy_max_queries = 256
        g.set_option("kw_zero_copy_max_queries", 0)
        staged = g.keyword_search_batch(qs, k_stride=KS_A)
        assert g.counter("kw_batches") - r0 == 3
        g.set_option("kw_zero_copy_max_queries", 256)
        g.set_option("kw_host_split_first_pct", 50)
        g.set_option("kw_host_split_queries", 7)                                       # 26 queries + the other 27
        r0 = g.counter("kw_batches")
        sliced = g.keyword_search_batch(qs, k_stride=KS_A)
        assert g.counter("kw_batches") - r0 == 2
    finally:
        g.set_option("kw_zero_copy_max_queries", 256)
        g.set_option("kw_host_split_queries", 1000)
        g.set_option("kw_host_split_first_pct", 85)
    failed = np.nonzero(ref.status != 0)[0]
    assert failed.size == 1 and failed[0] == 30
    assert any(ref.status[i] == 0 and ref.n_hits[i] == 0 and ref.num_matched[i] == 0 for i in range(N_A))      # a query whose tokens match nothing
    for what, got in (("zero-copy image", zero_copy), ("staged image", staged), ("sliced", sliced)):
        assert_same_bits(ref, got, what)
    for what, got in (("device output", ref), ("zero-copy image", zero_copy), ("staged image", staged), ("sliced", sliced)):
        assert got.n_hits[30] == 0 and got.num_matched[30] == 0, what
    assert_reference_equals_oracle(w, qs, ref, "device output, set A")


def body_large_image_direct_copies(w):
    """query set B (190 queries, k_stride 1000): the host image would exceed 8 MiB, so neither image route applies and the seven direct copies run"""
    g = w.g
    qs = make_queries(N_B, seed=98)
    assert N_B * KS_B * ROW_BYTES > IMAGE_LIMIT
    r0 = g.counter("kw_batches")
    ref = search_device_output(w, qs, KS_B)
    host = g.keyword_search_batch(qs, k_stride=KS_B)
    assert g.counter("kw_batches") - r0 == 2                                           # (one batch each: not sliced, not coalesced)
    assert (ref.status != 0).sum() == 1
    assert_same_bits(ref, host, "direct copies")
    assert_reference_equals_oracle(w, qs, ref, "device output, set B")
