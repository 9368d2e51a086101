#!/usr/bin/env python
"""bench.py — throughput of the query-time scoring hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run, one rank per GPU)

A "step" = one pass of the hot path over one batch of synthetic queries. The headline (`metric`/`value`) is BASELINE
config 2 — 10M-doc Zipf collection (V=100K, 32 tokens/doc, seed 2), a batch of 10 000 3-term conjunctive queries (ranks
log-uniform [8,2000]), Topster 250 (per_page 100), sort [_text_match desc, points desc]. A plain run times only that; with
`--full` (and the default `--workload all`) the same JSON line also carries `vector` (config 3: 10M x 768 fp32, batched exact inner-product
top-100) and `hybrid` (config 4: keyword + vector + reciprocal-rank fusion) sub-objects, each timed the same way, each with
its own parity object checked at FULL size against the oracle.

N>1 (BASELINE config 5), default `--dist-mode shards`: the SAME 10M-doc collection cut into N contiguous seq_id ranges, every
GPU scores the whole query batch on its shard, then the exchange behind the C-ABI (tsgpu_group, rank form, RCCL: the shards' bounds,
the bound-pruned query slices, an exact slice merge on the device); total work is fixed -> "scaling": "strong". Rank 0
also holds an unsharded twin of the collection and checks a sample of the merged results against it inside the bench.
`--dist-mode replicas`: every GPU holds the collection and answers its own batch — N independent replicas, no collective.

`roofline` = the dominant kernel: algorithmic bytes (or flops) per launch / its HIP-event time measured inside the
library on its launch stream. `cpu_baseline` (rank 0, N=1) = the oracle — a port of the reference's CPU path — timed on
this box's host cores on a bounded sample of the same queries. `concurrency` = the reference's calling convention: 256 host
threads issuing blocking ONE-query calls on one context (micro-batcher inside the library). The oracle is never the thing
measured as `value`; there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_F32_PEAK_TF = 157.3     # fp32-input MFMA dense peak
MFMA_BF16_PEAK_TF = 2500.0   # bf16 MFMA dense peak (no sparsity)
MFMA_BF16_ISSUE_CEILING_TF = 1580.0   # measured: vec_hscan_kernel<4> with only its MFMAs left in (profiles/r02/exp_vec_abl_mfma.txt: 3.93e12 flop in 2.49 ms)
FETCH_SIZE = 100
K_TOPSTER = 250
PROFILE_ROUND = "r06"
DUMP_QUERIES = 1024          # --dump-outputs: queries of the batch whose hit lists are written (seeded sample, the same every run)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="all", choices=["all", "keyword", "vector", "hybrid", "kwgeneral", "hnsw"],
                    help="kwgeneral = only the two general-kernel keyword legs (two query_by fields; 10 candidate combinations per query) at the keyword config's size")
    ap.add_argument("--n-docs", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=0, help="keyword queries per step (default 10000)")
    ap.add_argument("--vec-batch", type=int, default=256, help="vector / hybrid queries per step")
    ap.add_argument("--cpu-sample", type=int, default=0, help="queries of the CPU-baseline sample (0 = auto)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the oracle legs (cpu_baseline + the parity checks that need it)")
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary legs (concurrency, uncached-term batch, vector batch sweep / cosine / clustered)")
    ap.add_argument("--threads", type=int, default=256, help="host threads of the concurrency leg")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--hnsw-rows", type=int, default=2_000_000, help="rows of the HNSW leg's collection (0 = skip the leg); the bulk build on the device runs at ~170 K rows/s "
                                                                    "(10M x 768: 58 s, profiles/r06/bench_hnsw_10m.json), the insertion-order build (--hnsw-graph inserted) at ~8 K rows/s on 16 host threads")
    ap.add_argument("--hnsw-graph", default="bulk", choices=["bulk", "inserted", "knn"],
                    help="bulk (default) = tsgpu_vec_hnsw_build: the graph built in batches on the device (hnswlib's level draw, beam, neighbour heuristic and reverse-link "
                         "rule per batch; csrc/vec_hnsw_build.hip.h); inserted = hnswlib's incremental addPoint inside the library (tsgpu_vec_hnsw_enable, label order, one host thread per CPU of the quota); "
                         "knn = the round-2 stand-in derived on the GPU from exact k-NN lists (typesense_amd/hnsw_synth.py)")
    ap.add_argument("--hnsw-batch", type=int, default=4096, help="queries per step of the HNSW leg")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--dry", default=None, metavar="FULL_LINE.json",
                    help="no GPU work: read a FULL bench record (e.g. profiles/r04/bench_default_final.json) and print what the driver would get "
                         "for it — the compact last line (CPU-tier test of the output contract)")
    ap.add_argument("--detail-out", default=None, help="where the full record goes (default: gpurun_out/bench_detail.json under the repo root)")
    ap.add_argument("--opt", action="append", default=[], help="tsgpu_set_option name=value (repeatable), e.g. vec_prefilter=0")
    ap.add_argument("--dist-mode", default="shards", choices=["shards", "replicas"],
                    help="N>1: shards (default, BASELINE config 5) = the collection cut into N doc ranges, every GPU scores the whole batch on its "
                         "shard, all-gather of the per-GPU top-K + exact device merge (strong scaling); replicas = every GPU holds the collection, "
                         "the global batch (N x per-GPU batch) is sharded across the GPUs (weak scaling)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: with --workload all also the vector and hybrid configs; the CPU baselines and the parity checks "
                         "against the oracle; the secondary legs (concurrency, uncached terms, vector sweeps and variants, HNSW, general kernels); the "
                         "headline's other forms (all arrays, pinned host arrays, two callers, device-only) and the keyword roofline they feed; N>1: the "
                         "unsharded twin, its in-run equality checks and the replicas forms. Without it a run sets up, warms up, times the headline's "
                         "steps and prints its line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the headline's timed path delivered in its last step as DIR/<name>.npy (float64, or "
                         "float32 for fp32 outputs); per-hit arrays of a fixed sample of %d queries" % DUMP_QUERIES)
    a = ap.parse_args()
    if a.dump_outputs and a.workload in ("kwgeneral", "hnsw"):
        ap.error("--dump-outputs writes the outputs of the headline configs (--workload all, keyword, vector or hybrid)")
    if not a.full:
        a.no_cpu_baseline = a.no_extras = True
    return a


def dist_setup(n_gpus):
    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # TSGPU_DIST_BACKEND=gloo: rehearsal of the N>1 code path on a box with fewer GPUs than ranks (all ranks share device 0,
    # collectives through gloo); the measured configuration is always nccl (= RCCL over xGMI), one GPU per rank
    backend = os.environ.get("TSGPU_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    assert world == n_gpus, "launch with torch.distributed.run --nproc-per-node %d" % n_gpus
    return rank, world, local, backend


def barrier(world):
    import torch
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()


def max_over_ranks(x, world):
    import torch
    if world == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def timed(step, steps, warmup, world, after=None):
    """W untimed warmups, then exactly K steps bracketed by barrier + synchronize; returns (max-over-ranks seconds,
    per-step latencies, last result). `after(result)` runs inside the timed loop after each step's synchronize."""
    import torch
    out = None
    for _ in range(warmup):
        out = step()
    barrier(world)
    lat = []
    t0 = time.perf_counter()
    for _ in range(steps):
        s0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - s0)
        if after:
            after(out)
    barrier(world)
    return max_over_ranks(time.perf_counter() - t0, world), lat, out


def _profile(fname):
    for rnd in (PROFILE_ROUND, "r05", "r04", "r03", "r02", "r01"):
        p = os.path.join(ROOT, "profiles", rnd, fname)
        if os.path.exists(p):
            return p
    return None


def pmc_traffic(kernel_rx, fnames, field="avg", scale=1.0):
    """HBM bytes per launch of the dominant kernel(s) from the committed rocprofv3 --pmc FETCH_SIZE pass (KB, own pass);
    None when the profile is absent. `kernel_rx`: one regex, or a list whose kernels run back to back as one step of the path
    (their bytes add up). `field`: avg over the kernel's dispatches, or max (the full-index dispatch when the same
    kernel also runs a short sample pass). `scale` = 2 for kernels whose reads are all 16 B/lane: on gfx950 FETCH_SIZE reports
    half the bytes of wide coalesced reads (MI355X_MICROARCH.md, HBM section)."""
    p = None
    for f in ([fnames] if isinstance(fnames, str) else fnames):
        p = p or _profile(f)
    if not p:
        return None
    total, seen = 0.0, 0
    for rx in ([kernel_rx] if isinstance(kernel_rx, str) else kernel_rx):
        for line in open(p):
            if re.search(rx, line) and "FETCH_SIZE" in line:
                m = re.search(field + r"=([0-9.e+]+)", line)
                if m:
                    total += float(m.group(1)) * 1024.0 * scale
                    seen += 1
                    break
    return total if seen else None


def kernel_src_sha16():
    """hash of the sources that define the keyword find / score kernels: stamped into profiles/rNN/pmc_meta.json by tools/gpu_profile.sh when a --pmc pass is
    taken and compared here, so that a counter from a pass of OTHER kernel sources is flagged instead of silently divided by a live time"""
    import hashlib
    h = hashlib.sha256()
    for f in ("kw_kernels.hip.h", "kw_find2.hip.h", "tsgpu_format.h"):
        with open(os.path.join(ROOT, "typesense_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _pmc_meta(fname):
    p = _profile(fname)
    if not p:
        return None
    m = os.path.join(os.path.dirname(p), "pmc_meta.json")
    try:
        with open(m) as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return None


def pmc_counter(kernel_rx, fnames, counter, field="avg"):
    p = None
    for f in ([fnames] if isinstance(fnames, str) else fnames):
        p = p or _profile(f)
    if not p:
        return None
    for line in open(p):
        if re.search(kernel_rx, line) and re.search(r"\b" + counter + r"\b", line):
            m = re.search(field + r"=([0-9.e+]+)", line)
            if m:
                return float(m.group(1))
    return None


def device_hits(torch, n_q, ks):
    from typesense_amd import _lib as B
    d = dict(keys=torch.zeros((n_q, ks), dtype=torch.int64, device="cuda"),
             scores=torch.zeros((n_q, ks, 3), dtype=torch.int64, device="cuda"),
             text_match=torch.zeros((n_q, ks), dtype=torch.int64, device="cuda"),
             vector_distance=torch.zeros((n_q, ks), dtype=torch.float32, device="cuda"),
             match_score_index=torch.zeros((n_q, ks), dtype=torch.int8, device="cuda"),
             n_hits=torch.zeros(n_q, dtype=torch.int32, device="cuda"),
             num_matched=torch.zeros(n_q, dtype=torch.int64, device="cuda"),
             status=torch.zeros(n_q, dtype=torch.int32, device="cuda"),
             search_cutoff=torch.zeros(n_q, dtype=torch.int32, device="cuda"))
    h = B.HitsC()
    h.mem = B.MEM_DEVICE
    h.k_stride = ks
    for k, v in d.items():
        setattr(h, k, v.data_ptr())
    return d, h


# ---------------------------------------------------------------- --dump-outputs
def dump_rows(n_q):
    """the queries whose hit lists are written: a seeded sample of the batch, ascending"""
    return np.sort(np.random.default_rng(20).choice(n_q, size=min(n_q, DUMP_QUERIES), replace=False))


def hit_rows(n_hits, rows, **per_hit):
    """per-hit arrays [n_q, k, ...] -> their `rows`; the slots past a query's n_hits are not part of its result and are written as 0 (keys: -1)"""
    nh = np.asarray(n_hits).astype(np.int64)[rows]
    out = {}
    for name, a in per_hit.items():
        a = np.asarray(a)[rows]
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        live = (np.arange(a.shape[1])[None, :] < nh[:, None]).reshape(a.shape[:2] + (1,) * (a.ndim - 2))
        out[name] = np.where(live, a, -1 if name == "keys" else 0)
    return out


def split64(a):
    """int64 words (packed scores exceed the 2^53 that float64 holds exactly) -> (signed high 32 bits, low 32 bits)"""
    a = np.asarray(a).astype(np.int64)
    return a >> 32, a & 0xFFFFFFFF


def write_outputs(dirname, arrays):
    """DIR/<name>.npy per array: float32 stays float32, every other array becomes float64, which must hold it exactly"""
    os.makedirs(dirname, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.asarray(a)
        f = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
        assert a.dtype.kind == "f" or np.array_equal(f.astype(a.dtype), a), "%s does not fit float64 exactly" % name
        np.save(os.path.join(dirname, name + ".npy"), f)
        total += f.nbytes
    assert total <= 64 << 20, "--dump-outputs wrote %d bytes (limit 64 MB)" % total
    return total


def cpu_quota_cpus():
    """CPUs the container may use (cgroup v2 cpu.max), None = unlimited: the cpu_baseline legs start one thread per visible core, the quota decides how many run"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else float(q) / float(per)
    except Exception:
        return None


def loadgen_lib():
    from typesense_amd import build as Bd
    L = C.CDLL(Bd.build_loadgen())
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.tsgpu_loadgen_hits_checksum.restype = u64
    L.tsgpu_loadgen_hits_checksum.argtypes = [vp, vp, u32, u64, u32]
    L.tsgpu_loadgen_keyword.restype = C.c_double
    L.tsgpu_loadgen_keyword.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, u32, vp, vp, C.POINTER(u64)]
    L.tsgpu_loadgen_grouped_checksum.restype = u64
    L.tsgpu_loadgen_grouped_checksum.argtypes = [u32, u64, u32, vp, vp, vp, vp, vp, u32]
    L.tsgpu_loadgen_grouped.restype = C.c_double
    L.tsgpu_loadgen_grouped.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, u32, vp, vp, C.POINTER(u64)]
    L.tsgpu_loadgen_knn.restype = C.c_double
    L.tsgpu_loadgen_knn.argtypes = [vp, vp, u32, vp, u32, u32, u32, u32, u32, vp, vp, vp, C.POINTER(u64)]
    return L


class Bench:
    def __init__(self, args, rank, world):
        import torch
        import typesense_amd as T
        self.torch, self.T, self.args, self.rank, self.world = torch, T, args, rank, world
        self.g = T.GpuIndex(torch.cuda.current_device())
        self.opts = {}
        for o in args.opt:
            name, val = o.split("=")
            self.g.set_option(name, int(val))
            self.opts[name] = int(val)
        if world > 1 and "plan_threads" not in self.opts:
            # N ranks share this node's host cores: a rank plans its batch on its share of them, not on the single-process default of 8 threads
            self.g.set_option("plan_threads", max(1, min(8, int(cpu_quota_cpus() or os.cpu_count() or 8) // world)))
        self.n_docs = args.n_docs
        from typesense_amd import hostcoll as D           # doc-range arithmetic + the torch.distributed callbacks of the group's HOST transport (plumbing only)
        self.D = D
        self.sharded = world > 1 and args.dist_mode == "shards"
        self.lo, self.hi = D.shard_range(self.n_docs, rank, world) if self.sharded else (0, self.n_docs)
        self.qseed = 1000 * rank if (world > 1 and not self.sharded) else 0      # replicas: every rank draws its own batch
        self.twin = None            # shards mode, rank 0: the unsharded collection (in-bench equality check of the merged results)
        self.sort = None
        self.csr = None
        self.exact = None           # exact k-NN of the first queries by the oracle's chunked flat scan (vector + hybrid parity)
        self.extras = not args.no_extras and world == 1
        self.head = "keyword" if args.workload == "all" else args.workload      # the leg whose figure heads the line (and whose outputs --dump-outputs writes)
        self.dump = None
        # N > 1, shards: the exchange runs behind the C-ABI (tsgpu_group, rank form): RCCL collectives on the context's stream + the library's
        # merge kernels (rank 0's ncclUniqueId travels through torch.distributed). Under TSGPU_DIST_BACKEND=gloo (rehearsal: the ranks share
        # one GPU) the same group runs over its HOST transport (the callbacks = torch.distributed on host memory). If the group cannot be
        # brought up, or its probe call fails on any rank, the bench FAILS on every rank: it never measures a path the product does not ship.
        self.group, self.exchange = None, "none (1 GPU)" if world == 1 else "none (independent replicas)"
        if self.sharded:
            self.group = self.join_group(self.g)
            if self.group_transport == "rccl":
                self.exchange = ("tsgpu_group (C-ABI, rank form, RCCL): ncclAllGather of the shards' bounds, bound-pruned query slices by ncclSend/ncclRecv, slice merge "
                                 "(kw_shard_merge_kernel), on the library's stream; k-NN: one ncclAllGather + vec_group_merge_kernel")
            else:
                self.exchange = ("tsgpu_group (C-ABI, rank form, HOST transport over torch.distributed/%s callbacks): all-gather of the shards' bounds, all-to-all of the bound-pruned "
                                 "query slices + slice merge, staged through pinned host memory; k-NN: one all-gather + vec_group_merge_kernel" % os.environ.get("TSGPU_DIST_BACKEND", "nccl"))

    def set_dump(self, n_hits, per_query, per_hit):
        """--dump-outputs of the head leg: its per-query arrays for the whole batch, its per-hit arrays for the dump_rows() sample; the
        64-bit score words go out as two exact halves (<name>_hi, <name>_lo)"""
        rows = dump_rows(len(n_hits))
        d = {"sample_rows": rows, "n_hits": np.array(n_hits)}
        d.update((k, np.array(v)) for k, v in per_query.items())
        for name, a in hit_rows(n_hits, rows, **per_hit).items():
            if name in ("scores", "text_match"):
                d[name + "_hi"], d[name + "_lo"] = split64(a)
            else:
                d[name] = a
        self.dump = d

    def all_ranks_or_die(self, ok, what, err):
        """every rank learns whether `what` succeeded everywhere; if not, every rank raises (no rank is left inside a collective, and no
        fallback path is measured in the product's name)"""
        import torch.distributed as dist
        flag = self.torch.tensor([1 if ok else 0], dtype=self.torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) != 1:
            raise RuntimeError("[bench] rank %d: tsgpu_group %s failed on at least one rank (%s here): the multi-GPU line is NOT measured on another path." % (self.rank, what, err or "ok"))

    def join_group(self, index):
        """tsgpu_group over this rank's context `index` (rank form). nccl backend: RCCL inside the library; any other backend: the group's
        HOST transport over torch.distributed callbacks. Fails on every rank if any rank fails."""
        torch, T = self.torch, self.T
        import torch.distributed as dist
        grp, err = None, None
        rccl = os.environ.get("TSGPU_DIST_BACKEND", "nccl") == "nccl" and os.environ.get("TSGPU_BENCH_TRANSPORT", "rccl") == "rccl"
        try:
            if rccl:
                uid = torch.zeros(128, dtype=torch.uint8, device="cuda")
                if self.rank == 0:
                    uid.copy_(torch.frombuffer(bytearray(T.GpuGroup.unique_id(index.L)), dtype=torch.uint8))
                dist.broadcast(uid, 0)
                grp = T.GpuGroup.join(index, bytes(uid.cpu().numpy().tobytes()), self.rank, self.world)
            else:
                if not hasattr(self, "host_pg"):
                    # host collectives need a CPU-capable process group: the default one under gloo, a gloo side group under nccl
                    self.host_pg = None if dist.get_backend() != "nccl" else dist.new_group(backend="gloo")
                ag, a2a = self.D.torch_collectives(self.host_pg)
                grp = T.GpuGroup.join_host(index, self.rank, self.world, ag, a2a)
        except Exception as e:      # noqa: BLE001 — reported on every rank, then fatal
            err = repr(e)
            sys.stderr.write("[bench] rank %d: tsgpu_group could not be created: %s\n" % (self.rank, err))
        self.group_transport = "rccl" if rccl else "host"
        self.all_ranks_or_die(err is None, "creation (%s transport)" % self.group_transport, err)
        return grp

    def group_works(self, what, fn):
        """one UNTIMED call of a tsgpu_group exchange on every rank before the timed loop: a failure anywhere is fatal everywhere"""
        if self.group is None:
            return False
        err = None
        try:
            fn()
        except Exception as e:      # noqa: BLE001 — reported on every rank, then fatal
            err = repr(e)
            sys.stderr.write("[bench] rank %d: tsgpu_group %s probe failed: %s\n" % (self.rank, what, err))
        self.all_ranks_or_die(err is None, "%s exchange" % what, err)
        return True

    # ---------------------------------------------------------------- index builds (untimed)
    def build_keyword(self):
        from typesense_amd import _lib as B, synth
        n_docs = self.n_docs
        self.vocab, self.tpd = (100_000, 32) if n_docs >= 1_000_000 else (20_000, 16)
        t0 = time.time()
        # ONE collection (seed 2) whatever N is: a shard holds the postings of documents [lo, hi) of exactly the corpus the N=1 run
        # indexes (the whole collection is drawn with the same random stream, then cut)
        self.pts = synth.points_column(n_docs)

        def load(g, doc_range):
            csr = synth.zipf_corpus_csr(n_docs, self.vocab, self.tpd, seed=2, doc_range=doc_range)
            g.field_create(0, False)
            g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
            g.column_set(0, self.pts)
            g.set_num_docs(n_docs)
            g.commit()
            return csr
        self.csr = load(self.g, (self.lo, self.hi) if self.sharded else None)
        if self.sharded:
            self.g.set_option("doc_range_lo", int(self.lo)); self.g.set_option("doc_range_hi", int(self.hi))      # the seq_ids this shard owns (q = * ranks only those)
        if self.sharded and self.args.full:
            # every rank also holds the WHOLE collection (6 GB): rank 0 checks the merged shard results against it, and all ranks run the
            # second multi-GPU form (replicas) on it
            self.twin = self.T.GpuIndex(self.torch.cuda.current_device())
            load(self.twin, None)
        self.sort = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
        return time.time() - t0

    def base_slab(self, a, b, normalize=False, clustered=False):
        """base vectors of global rows [a, b): the collection is defined on a fixed grid of 2^20-row slabs (seed 3 + slab start), so
        every shard / chunk regenerates exactly the rows of the unsharded collection"""
        from typesense_amd import synth
        torch = self.torch
        S = 1 << 20
        parts = []
        for s0 in range(a // S * S, b, S):
            n = min(S, self.n_docs - s0)
            x = synth.random_vectors(n, self.args.dim, seed=3 + s0, device="cuda")
            if clustered:
                # 1024 tight clusters: centre + 0.15 x noise, unit length — many near-ties around every query's k-th neighbour
                gcen = torch.Generator(device="cuda")
                gcen.manual_seed(77)
                cen = torch.randn((1024, self.args.dim), generator=gcen, device="cuda", dtype=torch.float32)
                gi = torch.Generator(device="cuda")
                gi.manual_seed(78 + s0)
                idx = torch.randint(0, 1024, (n,), generator=gi, device="cuda")
                x = cen[idx] + 0.15 * x
            if normalize or clustered:
                x /= (x.norm(dim=1, keepdim=True) + 1e-30)
            parts.append(x[max(a, s0) - s0:min(b, s0 + n) - s0])
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def load_vectors(self, g, field, metric, lo, hi, **kw):
        torch = self.torch
        g.vec_create(field, self.args.dim, metric, hi - lo)
        S = 1 << 20
        for a in range(lo, hi, S):
            b = min(hi, a + S)
            x = self.base_slab(a, b, **kw).contiguous()
            labels = torch.arange(a, b, dtype=torch.int64, device="cuda")
            g.vec_upsert_device(field, labels.data_ptr(), x.data_ptr(), b - a)
            del x
        torch.cuda.synchronize()

    def build_vectors(self):
        from typesense_amd import _lib as B
        t0 = time.time()
        self.load_vectors(self.g, 1, B.METRIC_IP, self.lo, self.hi)
        if self.twin is not None and self.rank == 0:          # the unsharded matrix, for the in-bench equality check
            self.load_vectors(self.twin, 1, B.METRIC_IP, 0, self.n_docs)
        return time.time() - t0

    def kw_query_array(self, qtok):
        from typesense_amd import _lib as B
        arr = (B.KwQueryC * len(qtok))()
        for i in range(len(qtok)):
            self.T.KwQuery(qtok[i], sort=self.sort, topster_size=K_TOPSTER).fill(arr[i])
        return arr

    # ---------------------------------------------------------------- keyword (config 2 / 5)
    def run_keyword(self):
        from typesense_amd import synth, _lib as B
        torch, g, args, world = self.torch, self.g, self.args, self.world
        n_q = args.batch or 10_000
        qtok = synth.keyword_queries(n_q, 3, 8, 2000, seed=4 + self.qseed)
        arr = self.kw_query_array(qtok)
        dev, hs = device_hits(torch, n_q, K_TOPSTER)
        kern_ms, merge_ms, find_ms, alg_bytes = [], [], [], []

        if self.group is not None:
            gdev, ghs = device_hits(torch, n_q, FETCH_SIZE)
            self.group_works("keyword", lambda: self.group.keyword_search_batch_raw(arr, n_q, FETCH_SIZE, ghs))

        def step():
            if self.group is not None:
                # the whole shard step behind the C-ABI: every rank's top-250 Topster, the shards' bounds (32-byte entries), the bound-pruned
                # slices of its top-100 to the ranks that merge them, exact slice merge (kw_shard_merge_kernel), device-resident result
                self.group.keyword_search_batch_raw(arr, n_q, FETCH_SIZE, ghs)
                return gdev["keys"], gdev["scores"], gdev["n_hits"], gdev["num_matched"]
            g.keyword_search_batch_raw(arr, n_q, hs)           # synchronises its stream before returning (1 GPU, or one of N independent replicas)
            return dev["keys"], dev["scores"], dev["n_hits"], dev["num_matched"]

        def after(_):
            tm = g.timings()
            kern_ms.append(tm.kw_search_ms)
            merge_ms.append(tm.kw_merge_ms)
            find_ms.append(tm.kw_find_ms)
            alg_bytes.append(tm.kw_algorithmic_bytes)

        # HEADLINE = what the B1 seam returns: the hit arrays delivered to HOST memory inside the timed steps (1 GPU: tsgpu_hits mem=HOST,
        # pageable arrays, the library's two chained slices; N GPUs: every rank copies the 1/N query slice it merged over its own PCIe
        # link, as the local form of tsgpu_group does). The device-resident step is timed as well (`value_device_only`): it is the
        # single-launch form the roofline / rocprof durations refer to.
        if self.group is None:
            # the arrays the seam's shim requests for a query that sorts on _text_match (csrc/host/tsgpu_keyword_shim.h): keys, scores[3],
            # match_score_index + the per-query counts; text_match (= scores[match_score_index]) and vector_distance (a keyword KV's default)
            # are not requested. The same step with EVERY tsgpu_hits array delivered is timed as `value_host_all_arrays`.
            hh = self.T.Hits(n_q, K_TOPSTER)
            hhs = hh.c_struct(seam_arrays_only=True)
            hhs_all = hh.c_struct()

            def step_host():
                g.keyword_search_batch_raw(arr, n_q, hhs)
                return hh

            def step_host_all():
                g.keyword_search_batch_raw(arr, n_q, hhs_all)
                return hh
            if args.full:
                el_all, _lat_all, _ = timed(step_host_all, max(args.steps // 2, 3), min(args.warmup, 2), world)
                self.host_all_arrays_ms = 1e3 * el_all / max(args.steps // 2, 3)
            el_host, lat_host, _ = timed(step_host, args.steps, args.warmup, world)
            if self.head == "keyword" and args.dump_outputs:        # (before the legs below write into the same arrays)
                self.set_dump(hh.n_hits, dict(num_matched=hh.num_matched, status=hh.status, search_cutoff=hh.search_cutoff),
                              dict(keys=hh.keys, scores=hh.scores, match_score_index=hh.match_score_index))
            if not args.full:
                return dict(elapsed=el_host, lat=lat_host, n_q=n_q, n_postings=int(self.csr["n_postings"]), nonempty=int((hh.n_hits > 0).sum()))
            # the headline's batch delivered to PINNED host arrays (hipHostMalloc'ed once by the caller, e.g. the shim's reusable result arrays): the copy-out is a
            # plain DMA instead of the runtime's staged copy to pageable memory — reported next to the headline (`value_host_pinned`)
            try:
                ph = dict(keys=torch.zeros((n_q, K_TOPSTER), dtype=torch.int64).pin_memory(), scores=torch.zeros((n_q, K_TOPSTER, 3), dtype=torch.int64).pin_memory(),
                          msi=torch.zeros((n_q, K_TOPSTER), dtype=torch.int8).pin_memory(), n_hits=torch.zeros(n_q, dtype=torch.int32).pin_memory(),
                          num_matched=torch.zeros(n_q, dtype=torch.int64).pin_memory(), status=torch.zeros(n_q, dtype=torch.int32).pin_memory())
                phs = B.HitsC()
                phs.mem, phs.k_stride = B.MEM_HOST, K_TOPSTER
                phs.keys, phs.scores, phs.match_score_index, phs.n_hits, phs.num_matched, phs.status = (ph[k].data_ptr() for k in ("keys", "scores", "msi", "n_hits", "num_matched", "status"))
                el_pin, _lp, _ = timed(lambda: g.keyword_search_batch_raw(arr, n_q, phs), args.steps, min(args.warmup, 2), world)
                nh = ph["n_hits"].numpy()
                self.host_pinned = {"ms_per_step": 1e3 * el_pin / args.steps,
                                    "same_as_pageable": bool(np.array_equal(nh, hh.n_hits.view(np.int32)) and all(
                                        np.array_equal(ph["keys"][i, :nh[i]].numpy().view(np.uint64), hh.keys[i, :nh[i]]) and np.array_equal(ph["scores"][i, :nh[i]].numpy(), hh.scores[i, :nh[i]])
                                        for i in range(0, n_q, 7)))}
                del ph
            except Exception as e:      # noqa: BLE001
                self.host_pinned = {"error": repr(e)}
            # the same host-delivered batches from TWO request threads (two lanes: one caller's copy-out runs under the other's kernels) — what a server
            # with concurrent requests sees; reported NEXT TO the headline (`value_two_callers`), which stays the single blocking caller
            try:
                import threading
                hh2 = self.T.Hits(n_q, K_TOPSTER)
                hhs2 = hh2.c_struct(seam_arrays_only=True)
                go = threading.Barrier(3)
                def caller(h):
                    go.wait()
                    for _ in range(args.steps):
                        g.keyword_search_batch_raw(arr, n_q, h)
                th = [threading.Thread(target=caller, args=(h,)) for h in (hhs, hhs2)]
                for x in th:
                    x.start()
                torch.cuda.synchronize()
                go.wait()
                t0 = time.perf_counter()
                for x in th:
                    x.join()
                torch.cuda.synchronize()
                self.two_callers = {"elapsed": time.perf_counter() - t0, "batches": 2 * args.steps,
                                    "same_as_one_caller": bool(np.array_equal(hh.n_hits, hh2.n_hits) and all(
                                        np.array_equal(hh.keys[i, :hh.n_hits[i]], hh2.keys[i, :hh.n_hits[i]]) and np.array_equal(hh.scores[i, :hh.n_hits[i]], hh2.scores[i, :hh.n_hits[i]])
                                        for i in range(0, n_q, 7)))}
            except Exception as e:      # noqa: BLE001
                self.two_callers = {"error": repr(e)}
            elapsed_dev, lat_dev, out = timed(step, args.steps, min(args.warmup, 2), world, after)
            elapsed, lat = el_host, lat_host
        else:
            per = (n_q + world - 1) // world
            q0, q1 = min(self.rank * per, n_q), min((self.rank + 1) * per, n_q)
            if True:
                # the delivery INSIDE the library (group option kw_own_slice_only): after the slice exchange and the slice merge a rank copies the
                # slice it merged straight to its host arrays — no all-gather of the merged lists, no second pass over the result in python.
                # (The full, replicated result is produced once more after the timed loop for the in-run checks below.)
                ph = dict(keys=torch.zeros((n_q, FETCH_SIZE), dtype=torch.int64).pin_memory(), scores=torch.zeros((n_q, FETCH_SIZE, 3), dtype=torch.int64).pin_memory(),
                          n_hits=torch.zeros(n_q, dtype=torch.int32).pin_memory(), num_matched=torch.zeros(n_q, dtype=torch.int64).pin_memory(),
                          status=torch.zeros(n_q, dtype=torch.int32).pin_memory())
                phs = B.HitsC()
                phs.mem, phs.k_stride = B.MEM_HOST, FETCH_SIZE
                phs.keys, phs.scores, phs.n_hits, phs.num_matched, phs.status = (ph[k].data_ptr() for k in ("keys", "scores", "n_hits", "num_matched", "status"))
                self.group.set_option("kw_own_slice_only", 1)
                try:
                    def step_own_slice():
                        self.group.keyword_search_batch_raw(arr, n_q, FETCH_SIZE, phs)
                        return None
                    elapsed, lat, _ = timed(step_own_slice, args.steps, args.warmup, world, after)
                finally:
                    self.group.set_option("kw_own_slice_only", 0)
                if not args.full and not (self.head == "keyword" and args.dump_outputs):
                    return dict(elapsed=elapsed, lat=lat, n_q=n_q, n_postings=int(self.csr["n_postings"]), nonempty=None)
                out = step()
                mine = slice(q0, q1)
                self.own_slice_ok = bool(q1 <= q0 or (torch.equal(ph["n_hits"][mine].to(torch.int64), out[2][mine].to(torch.int64).cpu()) and
                                                    torch.equal(ph["num_matched"][mine], out[3][mine].to(torch.int64).cpu()) and
                                                    torch.equal(ph["keys"][mine][torch.arange(FETCH_SIZE)[None, :] < ph["n_hits"][mine][:, None]],
                                                                out[0][mine, :FETCH_SIZE].cpu()[torch.arange(FETCH_SIZE)[None, :] < ph["n_hits"][mine][:, None]])))
            elapsed_dev, lat_dev = None, None
        touched = None
        if world == 1:
            # ONE more step, untimed, with the find kernel's byte-counting instantiation (tsgpu option kw_count_touched; host-planned, device
            # outputs = the single-launch form kernel_ms refers to): the bytes the kernels REQUEST, next to the distinct lists' footprint
            try:
                g.set_option("kw_count_touched", 1)
                g.set_option("kw_device_plan_min_queries", 1 << 30)
                g.keyword_search_batch_raw(arr, n_q, hs)
                touched = g.kw_touched()
                terms = np.unique(qtok).astype(np.uint32)
                touched["footprint"] = g.kw_lists_footprint(np.zeros(terms.size, np.uint32), terms)
            finally:
                g.set_option("kw_count_touched", 0)
                g.set_option("kw_device_plan_min_queries", 512)      # (the default, csrc/tsgpu_host.h)
        res = dict(elapsed=elapsed, lat=lat, touched=touched, kern_ms=float(np.mean(kern_ms)), merge_ms=float(np.mean(merge_ms)), find_ms=float(np.mean(find_ms)),
                   alg_bytes=float(np.mean(alg_bytes)), n_q=n_q, n_postings=int(self.csr["n_postings"]), elapsed_dev=elapsed_dev, lat_dev=lat_dev,
                   host_all_arrays_ms=getattr(self, "host_all_arrays_ms", None), two_callers=getattr(self, "two_callers", None), host_pinned=getattr(self, "host_pinned", None))
        if self.group is not None and args.full:
            # the bound-pruned exchange against the full top-k exchange (untimed): same merged result, fewer bytes
            gt = self.group.timings()
            self.group.set_option("kw_exchange_pruned", 0)
            try:
                ref = tuple(x.clone() for x in step())
                gu = self.group.timings()
            finally:
                self.group.set_option("kw_exchange_pruned", 1)
            nh_a, nh_b = out[2].to(torch.int64), ref[2].to(torch.int64)
            live = torch.arange(FETCH_SIZE, device="cuda")[None, :] < nh_a[:, None]
            same = bool(torch.equal(nh_a, nh_b)) and bool(torch.equal(out[3].to(torch.int64), ref[3].to(torch.int64))) \
                and bool(torch.equal(out[0][:, :FETCH_SIZE][live], ref[0][:, :FETCH_SIZE][live])) and bool(torch.equal(out[1][:, :FETCH_SIZE][live], ref[1][:, :FETCH_SIZE][live]))
            res["exchange_check"] = {"pruned_equals_full_exchange": bool(same), "local_ms": gt.local_ms, "exchange_merge_ms": gt.exchange_merge_ms,
                                     "exchange_bytes_per_gpu": int(gt.exchange_bytes_per_member), "hit_exchange_bytes_per_gpu": int(gt.hit_exchange_bytes_per_member),
                                     "full_topk_hit_exchange_bytes_per_gpu": int(gu.hit_exchange_bytes_per_member),
                                     "timed_form": "kw_own_slice_only: bounds all-gather + bound-pruned slice exchange + slice merge, every rank delivers the slice it merged to its own host",
                                     "own_slice_delivery_equals_full_result": getattr(self, "own_slice_ok", None)}
        keys = out[0].cpu().numpy().astype(np.uint64)
        scores = out[1].cpu().numpy()
        n_hits = out[2].cpu().numpy()
        num_matched = out[3].cpu().numpy()
        res["nonempty"] = int((n_hits > 0).sum())
        if self.group is not None and self.head == "keyword" and args.dump_outputs:
            # N>1: the merged result of the whole batch (every rank holds it; the timed steps delivered it to the ranks' hosts slice by slice)
            self.set_dump(n_hits, dict(num_matched=num_matched), dict(keys=keys[:, :FETCH_SIZE], scores=scores[:, :FETCH_SIZE]))
        if not args.full:
            return res

        if self.sharded and self.rank == 0:
            # in-bench equality: the merged result of the sharded collection == the unsharded twin's result (same corpus, same queries)
            m = min(n_q, 512)
            th = self.twin.keyword_search_batch(list(self.T.KwQuery(qtok[i], sort=self.sort, topster_size=K_TOPSTER) for i in range(m)), k_stride=K_TOPSTER)
            bad = 0
            for i in range(m):
                n = min(int(th.n_hits[i]), FETCH_SIZE)
                if int(n_hits[i]) != n or not np.array_equal(keys[i, :n], th.keys[i, :n]) or not np.array_equal(scores[i, :n], th.scores[i, :n]) \
                        or int(num_matched[i]) != int(th.num_matched[i]):
                    bad += 1
            res["shard_parity"] = {"checked": m, "mismatches": bad, "against": "the unsharded collection on rank 0 (top-100 keys, 3 scores, num_matched)"}

        if self.sharded and self.group is not None:
            try:
                # candidate combinations over the shards (tsgpu_group_keyword_search_candidates_batch; Index::search_all_candidates, src/index.cpp:1794-1894): 10 combinations per
                # user query, per-shard fold + exchange + global query_index; rank 0 checks the merged result against the unsharded twin's own fold
                n_u = max(8, min(n_q // 10, 200))
                base_c = synth.keyword_queries(n_u, 3, 8, 2000, seed=41)
                rng_c = np.random.default_rng(43)
                users = []
                for i in range(n_u):
                    combos = [base_c[i].copy()]
                    while len(combos) < 10:
                        c = combos[int(rng_c.integers(0, len(combos)))].copy()
                        c[int(rng_c.integers(0, 3))] = max(8, min(2000, int(c[int(rng_c.integers(0, 3))]) + int(rng_c.integers(1, 40))))
                        if len(set(c.tolist())) == 3 and not any(np.array_equal(c, x) for x in combos):
                            combos.append(c)
                    users.append([self.T.KwQuery(c, sort=self.sort, topster_size=K_TOPSTER, total_cost=(j > 0)) for j, c in enumerate(combos)])
                self.group.keyword_search_candidates_batch(users, k=FETCH_SIZE, k_stride=FETCH_SIZE)          # warm-up
                barrier(world)
                t0 = time.perf_counter()
                ch, cqi, cfound = self.group.keyword_search_candidates_batch(users, k=FETCH_SIZE, k_stride=FETCH_SIZE)
                el_c = max_over_ranks(time.perf_counter() - t0, world)
                res["candidate_combinations_sharded"] = {"value": n_u / el_c, "unit": "user queries/s (10 combinations each)", "ms_per_call": 1e3 * el_c, "user_queries": n_u}
                if self.rank == 0:
                    th, tqi, tfound = self.twin.keyword_search_candidates_batch(users, k_stride=K_TOPSTER)
                    bad = 0
                    for u in range(n_u):
                        n = min(int(th.n_hits[u]), FETCH_SIZE)
                        if int(ch.n_hits[u]) != n or not np.array_equal(ch.keys[u, :n], th.keys[u, :n]) or not np.array_equal(ch.scores[u, :n], th.scores[u, :n]) \
                                or not np.array_equal(cqi[u, :n], tqi[u, :n]) or int(ch.num_matched[u]) != int(th.num_matched[u]) or int(cfound[u]) != int(tfound[u]):
                            bad += 1
                    res["candidate_combinations_sharded"]["shard_parity"] = {"checked": n_u, "mismatches": bad,
                                                                             "against": "the unsharded collection's own fold on rank 0 (keys, scores, query_index, num_matched, found)"}
            except Exception as e:      # noqa: BLE001 (a secondary leg must not take the headline line with it)
                res["candidate_combinations_sharded"] = {"error": repr(e)}

        if self.sharded and self.group is not None:
            try:
                # q = * over the shards (tsgpu_group_wildcard_search_batch; Index::search_wildcard, src/index.cpp:6616-6818): every rank ranks the ids of its doc range by the
                # sort keys, the per-shard Topsters take the keyword exchange; rank 0 checks the merged result against the unsharded twin
                fl_w = np.arange(1, self.n_docs, 3, dtype=np.uint32)
                wqs = [self.T.KwQuery([], sort=((B.SORT_INT64_COLUMN, 1, 0), (B.SORT_SEQ_ID, 1, 0)), topster_size=K_TOPSTER),
                       self.T.KwQuery([], sort=((B.SORT_INT64_COLUMN, -1, 0), (B.SORT_SEQ_ID, -1, 0)), topster_size=K_TOPSTER, filter_ids=fl_w),
                       self.T.KwQuery([], sort=((B.SORT_INT64_COLUMN, 1, 0), (B.SORT_SEQ_ID, -1, 0)), topster_size=K_TOPSTER, excluded_ids=fl_w[::1000]),
                       self.T.KwQuery([], sort=((B.SORT_SEQ_ID, 1, 0),), topster_size=K_TOPSTER, filter_ids=fl_w[:5])]
                self.group.wildcard_search_batch(wqs, k=FETCH_SIZE, k_stride=FETCH_SIZE)          # warm-up
                barrier(world)
                t0 = time.perf_counter()
                wh = self.group.wildcard_search_batch(wqs, k=FETCH_SIZE, k_stride=FETCH_SIZE)
                el_w = max_over_ranks(time.perf_counter() - t0, world)
                res["wildcard_sharded"] = {"ms_per_call": 1e3 * el_w, "queries": len(wqs), "docs_ranked_per_s": (2 * self.n_docs + 2 * fl_w.size) / el_w,
                                           "workload": "q = * over %d documents cut into %d doc ranges: all ids / every third id (filter) / excluded ids / a 5-id filter" % (self.n_docs, world)}
                if self.rank == 0:
                    th = self.twin.wildcard_search_batch(wqs, k_stride=K_TOPSTER)
                    bad = 0
                    for i in range(len(wqs)):
                        n = min(int(th.n_hits[i]), FETCH_SIZE)
                        if int(wh.n_hits[i]) != n or not np.array_equal(wh.keys[i, :n], th.keys[i, :n]) or not np.array_equal(wh.scores[i, :n], th.scores[i, :n]) \
                                or int(wh.num_matched[i]) != int(th.num_matched[i]):
                            bad += 1
                    res["wildcard_sharded"]["shard_parity"] = {"checked": len(wqs), "mismatches": bad, "against": "the unsharded collection on rank 0 (keys, scores, num_matched)"}
            except Exception as e:      # noqa: BLE001 (a secondary leg must not take the headline line with it)
                res["wildcard_sharded"] = {"error": repr(e)}

        if self.sharded and self.group is not None:
            try:
                # group_by over the shards (tsgpu_group_keyword_search_grouped_batch): a group's documents live on several shards -> keyed exchange in two rounds (the shards'
                # best groups and heads; the selected groups' counts and KVs); rank 0 checks both passes against the unsharded twin's own grouped call
                n_g = max(8, min(n_q // 50, 100))
                gtok = synth.keyword_queries(n_g, 3, 8, 2000, seed=61)
                ids64 = np.arange(self.n_docs, dtype=np.uint64)
                n_grp = max(16, self.n_docs // 200)
                distinct = (((ids64 * np.uint64(2654435761)) % np.uint64(n_grp)) * np.uint64(0x100000001B3) + np.uint64(0x517cc1b727220a95)).astype(np.uint64)
                self.g.column_set(7, distinct.view(np.int64))
                gqs = [self.T.KwQuery(gtok[i], sort=self.sort, topster_size=FETCH_SIZE) for i in range(n_g)]
                gl = 3
                el_g, got = {}, {}
                for fp in (1, 0):
                    grs = [(gl, 7, fp, 0, 0)] * n_g
                    self.group.keyword_search_grouped_batch(gqs, grs, k_stride=FETCH_SIZE * gl, g_stride=FETCH_SIZE)          # warm-up
                    barrier(world)
                    t0 = time.perf_counter()
                    got[fp] = self.group.keyword_search_grouped_batch(gqs, grs, k_stride=FETCH_SIZE * gl, g_stride=FETCH_SIZE)
                    el_g[fp] = max_over_ranks(time.perf_counter() - t0, world)
                res["group_by_sharded"] = {"value": n_g / (el_g[1] + el_g[0]), "unit": "grouped user queries/s (first + second pass each)", "ms_first_pass": 1e3 * el_g[1], "ms_second_pass": 1e3 * el_g[0],
                                           "queries": n_g, "workload": "3-term queries, group_limit 3, %d groups over %d documents in %d doc ranges, Topster %d" % (n_grp, self.n_docs, world, FETCH_SIZE)}
                if self.rank == 0:
                    self.twin.column_set(7, distinct.view(np.int64))
                    bad = 0
                    for fp in (1, 0):
                        th, tg = self.twin.keyword_search_grouped_batch(gqs, [(gl, 7, fp, 0, 0)] * n_g, k_stride=FETCH_SIZE * gl, g_stride=FETCH_SIZE)
                        sh, sg = got[fp]
                        L = 1 if fp else gl
                        for i in range(n_g):
                            ng = int(tg.n_groups[i])
                            same = int(sg.n_groups[i]) == ng and int(sh.n_hits[i]) == int(th.n_hits[i]) and int(sh.num_matched[i]) == int(th.num_matched[i]) and int(sg.groups_count[i]) == int(tg.groups_count[i]) \
                                and np.array_equal(sg.distinct_key[i, :ng], tg.distinct_key[i, :ng]) and np.array_equal(sg.group_found[i, :ng], tg.group_found[i, :ng]) and np.array_equal(sg.group_size[i, :ng], tg.group_size[i, :ng])
                            for r in range(ng if same else 0):
                                n = int(tg.group_size[i, r])
                                same = same and np.array_equal(sh.keys[i, r * L:r * L + n], th.keys[i, r * L:r * L + n]) and np.array_equal(sh.scores[i, r * L:r * L + n], th.scores[i, r * L:r * L + n])
                            bad += 0 if same else 1
                    res["group_by_sharded"]["shard_parity"] = {"checked": 2 * n_g, "mismatches": bad,
                                                               "against": "the unsharded collection's grouped call on rank 0, both passes (groups, group_found, group_size, KVs, groups_count, num_matched)"}
            except Exception as e:      # noqa: BLE001 (a secondary leg must not take the headline line with it)
                res["group_by_sharded"] = {"error": repr(e)}

        if self.sharded:
            # second multi-GPU form, reported as a sub-object: replicas — every GPU holds the collection, the global batch of N x 10 000 queries
            # is sharded across the GPUs, one all-gather of the per-GPU top-100 (weak scaling)
            qt_r = synth.keyword_queries(n_q, 3, 8, 2000, seed=4 + 1000 * self.rank)
            arr_r = self.kw_query_array(qt_r)

            hh_r = self.T.Hits(n_q, K_TOPSTER)
            hhs_r = hh_r.c_struct(seam_arrays_only=True)

            def step_r():      # N independent replicas: every rank answers ITS batch on its full mirror and delivers it to its own host; no collective
                self.twin.keyword_search_batch_raw(arr_r, n_q, hhs_r)
                return hh_r
            el_r, lat_r, _ = timed(step_r, args.steps, min(args.warmup, 2), world)
            res["replicas"] = {"value": world * n_q * args.steps / el_r, "unit": "queries/s", "ms_per_step": 1e3 * el_r / args.steps, "scaling": "weak",
                               "global_batch": world * n_q, "parallelism": "%d independent replicas of the collection, every rank its own %d-query batch delivered to its own host "
                                                                           "(no collective: replicas do not exchange anything)" % (world, n_q)}
            if self.group is not None:
                # third form, through the C-ABI: REPLICAS with the SAME 10 000-query batch cut into N query slices (strong scaling): rank r answers
                # slice r on its full mirror (the twin), in-place ncclAllGathers of the slices' top-100; no merge, fixed costs shrink with the slice
                grp_r = self.join_group(self.twin)
                if grp_r is not None:
                    grp_r.set_option("replicas", 1)
                    rdev, rhs = device_hits(torch, n_q, FETCH_SIZE)

                    def step_rs():
                        grp_r.keyword_search_batch_raw(arr, n_q, FETCH_SIZE, rhs)
                        return rdev
                    el_s, _, o_s = timed(step_rs, args.steps, min(args.warmup, 2), world)
                    nh = o_s["n_hits"].to(torch.int64)
                    live = torch.arange(FETCH_SIZE, device="cuda")[None, :] < nh[:, None]
                    same = bool(torch.equal(nh, out[2].to(torch.int64))) and bool(torch.equal(o_s["keys"][live], out[0][:, :FETCH_SIZE][live])) \
                        and bool(torch.equal(o_s["scores"][live], out[1][:, :FETCH_SIZE][live])) and bool(torch.equal(o_s["num_matched"].to(torch.int64), out[3].to(torch.int64)))
                    res["replicas_strong"] = {"value": n_q * args.steps / el_s, "unit": "queries/s", "ms_per_step": 1e3 * el_s / args.steps, "scaling": "strong",
                                              "equals_the_shard_result": same,
                                              "parallelism": "%d full mirrors of the collection, the SAME %d-query batch cut into %d query slices (tsgpu_group option replicas), "
                                                             "in-place ncclAllGather of the slices' top-100" % (world, n_q, world)}
                    grp_r.close()


        if self.extras:
            res["concurrency"] = self.concurrency_keyword(arr, n_q, keys, scores, n_hits, num_matched)
            # a batch whose terms do NOT fit the Infinity Cache: ranks log-uniform over the whole vocabulary (most lists short, read once)
            qt2 = synth.keyword_queries(n_q, 3, 8, self.vocab, seed=14)
            arr2 = self.kw_query_array(qt2)
            g.keyword_search_batch_raw(arr2, n_q, hs)
            t0 = time.perf_counter()
            ks, ab = [], []
            for _ in range(3):
                g.keyword_search_batch_raw(arr2, n_q, hs)
                tm = g.timings()
                ks.append(tm.kw_search_ms)
                ab.append(tm.kw_algorithmic_bytes)
            dt = (time.perf_counter() - t0) / 3
            res["uncached"] = {"workload": "10 000 queries, 3 distinct terms, ranks log-uniform over the WHOLE vocabulary [8,%d] (2 000 hot terms no longer "
                                           "serve the batch from L2 / Infinity Cache)" % self.vocab,
                               "value": n_q / dt, "unit": "queries/s", "ms_per_step": 1e3 * dt, "kernel_ms": float(np.mean(ks)),
                               "algorithmic_bytes_per_launch": float(np.mean(ab)),
                               "achieved_GBs": float(np.mean(ab)) / (float(np.mean(ks)) * 1e-3) / 1e9 if np.mean(ks) > 0 else None,
                               "queries_with_hits": int((dev["n_hits"] > 0).sum().item())}

        if self.rank == 0 and world == 1 and not args.no_cpu_baseline:
            from oracle import oracle_py as O
            ncpu = os.cpu_count() or 1
            sample = min(args.cpu_sample or max(2 * ncpu, 32), n_q)
            orc = O.OracleIndex(1, 1)
            orc.set_num_docs(self.n_docs)
            orc.set_sort_dense(0, self.pts)
            for t in np.unique(qtok[:sample]):
                ids, oi, off = synth.csr_term(self.csr, t)
                if ids.size:
                    orc.load_posting(0, int(t), ids, oi, off)
            osort = ((O.SORT_TEXT_MATCH, 0, 1), (O.SORT_INT64_COLUMN, 0, 1))
            base = orc.make_query(qtok[0], sort=osort, fetch_size=100)
            orc.bench_keyword(base, qtok[:min(sample, ncpu)], ncpu)               # warm the page cache / allocator
            wall, per = orc.bench_keyword(base, qtok[:sample], ncpu)
            res["cpu"] = dict(value=sample / wall, unit="queries/s", cores=ncpu, cgroup_cpu_quota_cpus=cpu_quota_cpus(), kind="port",
                              sample="%d of the %d queries of the step, one query per thread on %d host threads (oracle = port of "
                                     "or_iterator_t::intersect + Match + Topster); p50 %.1f ms/query" % (sample, n_q, ncpu, float(np.median(per)) / 1e3))
            quota = cpu_quota_cpus()
            if quota and int(quota) < ncpu:
                # the same sample with as many threads as the container may actually run (the all-cores leg above is time-sliced): the
                # per-query latency of THIS leg is a latency, the other leg's is mostly waiting for a core
                nt = max(1, int(quota))
                wall_q, per_q = orc.bench_keyword(base, qtok[:sample], nt)
                res["cpu"]["at_quota_threads"] = {"threads": nt, "value": sample / wall_q, "unit": "queries/s", "p50_ms_per_query": float(np.median(per_q)) / 1e3}
                if sample / wall_q > res["cpu"]["value"]:
                    # the baseline quoted is the FASTER configuration (oversubscribing a CPU quota costs the reference's path throughput): both are stated
                    res["cpu"]["all_visible_cores"] = {"threads": ncpu, "value": res["cpu"]["value"], "unit": "queries/s"}
                    res["cpu"]["value"], res["cpu"]["cores"] = sample / wall_q, nt
                    res["cpu"]["sample"] = ("%d of the %d queries of the step, one query per thread on %d host threads = the container's CPU quota (faster than %d threads on the "
                                            "%d visible cores: that leg is time-sliced); oracle = port of or_iterator_t::intersect + Match + Topster; p50 %.1f ms/query"
                                            % (sample, n_q, nt, ncpu, ncpu, float(np.median(per_q)) / 1e3))
            bad = 0
            for i in range(min(sample, 64)):       # parity at full size: identical top-K (keys + all 3 scores) and match counts
                ref = orc.search_keyword(orc.make_query(qtok[i], sort=osort, fetch_size=100))
                n = int(n_hits[i])
                if n != ref.keys.size or not np.array_equal(keys[i, :n], ref.keys) or not np.array_equal(scores[i, :n], ref.scores) \
                        or int(num_matched[i]) != int(ref.num_keyword_matches):
                    bad += 1
            res["parity"] = {"checked": min(sample, 64), "mismatches": bad, "what": "Topster content (keys, 3 scores, order) + num_keyword_matches vs the oracle at 10M docs"}
        return res

    def run_keyword_general(self):
        """The reference's DEFAULT query shapes at the keyword config's size (10M docs), which take the general kernels instead of the
        single-field pair kernel: (i) two `query_by` fields (or_iterator_t per token = union over the fields, compute_aggregated_score fold;
        kw_search_mf_kernel + kw_score_kernel<MF>), (ii) Index::search_all_candidates (src/index.cpp:1845-1891): 10 candidate-token
        combinations per user query folded into ONE shared Topster (tsgpu_keyword_search_candidates_batch, kw_candidates_merge_kernel).
        Device time by HIP events (tsgpu_timings), parity against the oracle at full size."""
        from typesense_amd import synth, _lib as B
        from oracle import oracle_py as O
        torch, g, args = self.torch, self.g, self.args
        res = {}
        osort = ((O.SORT_TEXT_MATCH, 0, 1), (O.SORT_INT64_COLUMN, 0, 1))
        steps = max(3, min(args.steps, 10))
        # ---- (i) two query_by fields: a second string field (seed 22) over the same documents ----
        t0 = time.time()
        csr1 = synth.zipf_corpus_csr(self.n_docs, self.vocab, self.tpd, seed=22)
        g.field_create(1, False)
        g.terms_load_csr(1, csr1["term_ids"], csr1["ids_ptr"], csr1["ids"], csr1["offset_index"], csr1["off_ptr"], csr1["offsets"])
        g.commit()
        build_s = time.time() - t0
        n_q = max(16, (args.batch or 10_000) // 5)
        qtok = synth.keyword_queries(n_q, 3, 8, 2000, seed=31)
        fields = ((0, 15), (1, 14))
        qs = [self.T.KwQuery(qtok[i], sort=self.sort, topster_size=K_TOPSTER, fields=fields) for i in range(n_q)]
        arr = self.T.index.make_query_array(qs)
        dev, hs = device_hits(torch, n_q, K_TOPSTER)
        kern, merge, algb = [], [], []

        def step():
            g.keyword_search_batch_raw(arr, n_q, hs)
            return dev

        def after(_):
            tm = g.timings()
            kern.append(tm.kw_search_ms); merge.append(tm.kw_merge_ms); algb.append(tm.kw_algorithmic_bytes)
        prof = None
        if os.environ.get("KW_PROF") and hasattr(g.L, "tsgpu_debug_prof"):       # tools/ only: a TSGPU_PROF build's per-phase cycle counters of the find kernel
            step()
            prof = (C.c_uint64 * 16)()
            g.L.tsgpu_debug_prof(g.h, 1, None)
        el, lat, out = timed(step, steps, 2, 1, after)
        if prof is not None:
            g.L.tsgpu_debug_prof(g.h, 1, prof)
            v = list(prof)
            tot = sum(v[:12]) or 1
            sys.stderr.write("PROF mf find kernel: wg=%d %s cycles/wg=%.0f\n" % (v[12], " ".join("p%d=%.1f%%" % (i, 100.0 * v[i] / tot) for i in range(12)), tot / max(v[12], 1)))
        keys, scores = out["keys"].cpu().numpy().astype(np.uint64), out["scores"].cpu().numpy()
        n_hits, nm, st = out["n_hits"].cpu().numpy(), out["num_matched"].cpu().numpy(), out["status"].cpu().numpy()
        mf = {"workload": "%d queries/step, 3 distinct terms (ranks log-uniform [8,2000]), query_by = two string fields (weights 15, 14) over the same %d documents, "
                          "Topster 250, sort [_text_match desc, points desc]" % (n_q, self.n_docs),
              "value": n_q * steps / el, "unit": "queries/s", "ms_per_step": 1e3 * el / steps, "kernel_ms (kw_search_mf_kernel + kw_score_kernel<MF>)": float(np.mean(kern)),
              "merge_ms": float(np.mean(merge)), "algorithmic_bytes_per_launch": float(np.mean(algb)),
              "achieved_GBs_on_algorithmic_bytes": float(np.mean(algb)) / (float(np.mean(kern)) * 1e-3) / 1e9 if np.mean(kern) > 0 else None,
              "queries_with_hits": int((n_hits > 0).sum()), "status_nonzero": int((st != 0).sum()), "second_field_build_s": build_s}
        mf["kernel_ms"] = float(np.mean(kern))
        if np.mean(kern) > 0:
            ach = float(np.mean(algb)) / (float(np.mean(kern)) * 1e-3) / 1e9
            mf["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                              "traffic": pmc_traffic([r"kw_find_mf2_kernel<3, 2>", r"kw_score_kernel<3, 512, true, true, true>"], ["pmc_kwg_fetch.txt"], field="max"),
                              "kernel": "kw_find_mf2_kernel<3, 2> + kw_score_kernel<3, 512, MF> (back to back; kernel_ms spans both)", "kernel_ms": float(np.mean(kern)),
                              "algorithmic_bytes_per_launch": float(np.mean(algb)),
                              "note": "SURVEY 8(d) bytes over BOTH fields' lists / the two kernels' live time / 8 TB/s; like the single-field pair (frac 1.4) the kernels skip, but a two-field "
                                      "driver block costs two tile merges + the other field's probes: 0.33 of peak on the same yardstick"}
        if not args.no_cpu_baseline:
            npar = min(n_q, 32)
            orc = O.OracleIndex(2, 1)
            orc.set_num_docs(self.n_docs)
            orc.set_sort_dense(0, self.pts)
            for t in np.unique(qtok[:npar]):
                for f, c in ((0, self.csr), (1, csr1)):
                    ids, oi, off = synth.csr_term(c, t)
                    if ids.size:
                        orc.load_posting(f, int(t), ids, oi, off)
            bad = 0
            for i in range(npar):
                ref = orc.search_keyword(orc.make_query(qtok[i], fields=fields, sort=osort, fetch_size=100))
                n = int(n_hits[i])
                if n != ref.keys.size or not np.array_equal(keys[i, :n], ref.keys) or not np.array_equal(scores[i, :n], ref.scores) or int(nm[i]) != int(ref.num_keyword_matches):
                    bad += 1
            mf["parity"] = {"checked": npar, "mismatches": bad, "what": "Topster content (keys, 3 scores, order) + num_keyword_matches vs the oracle's or_iterator_t union over both fields at %d docs" % self.n_docs}
            orc.close()
        res["two_query_by_fields"] = mf
        del csr1

        # ---- (ii) search_all_candidates: 10 combinations per user query (prefix / typo candidates of each position), one shared Topster ----
        n_g = max(8, (args.batch or 10_000) // 10)
        base = synth.keyword_queries(n_g, 3, 8, 2000, seed=41)
        rng = np.random.default_rng(43)
        groups, gtoks = [], []
        for i in range(n_g):
            combos = [base[i].copy()]
            while len(combos) < 10:                       # a candidate of one position = a neighbouring term rank (what the ART walk returns: tokens near the typed one)
                c = combos[int(rng.integers(0, len(combos)))].copy()
                pos = int(rng.integers(0, 3))
                c[pos] = max(8, min(2000, int(c[pos]) + int(rng.integers(1, 40))))
                if len(set(c.tolist())) == 3 and not any(np.array_equal(c, x) for x in combos):
                    combos.append(c)
            gtoks.append(combos)
            groups.append([self.T.KwQuery(c, sort=self.sort, topster_size=K_TOPSTER, total_cost=(j > 0)) for j, c in enumerate(combos)])
        kern, merge = [], []
        flat = [q for grp in groups for q in grp]
        carr = self.T.index.make_query_array(flat)
        begin = np.arange(0, 10 * n_g + 1, 10, dtype=np.uint32)
        hits = self.T.Hits(n_g, K_TOPSTER)
        chs = hits.c_struct(seam_arrays_only=True)         # what the B1 shim requests (as in the headline): keys, scores[3], match_score_index, counts (+ query_index)
        qi = np.zeros((n_g, K_TOPSTER), np.uint32)
        found = np.zeros(n_g, np.uint64)

        def step_c():
            g.keyword_search_candidates_batch_raw(carr, begin, n_g, chs, qi, found)
            return hits, qi, found

        def after_c(_):
            tm = g.timings()
            kern.append(tm.kw_search_ms); merge.append(tm.kw_merge_ms)
        el, lat, (hits, qi, found) = timed(step_c, steps, 2, 1, after_c)
        cand = {"workload": "%d user queries/step x 10 candidate-token combinations each (= %d search_across_fields passes per step), 3 positions, shared Topster 250, "
                            "found = |union of the passes' result ids|; host outputs: the arrays the seam's shim requests (keys, scores[3], match_score_index, query_index, counts)" % (n_g, 10 * n_g),
                "value": n_g * steps / el, "unit": "user queries/s", "passes_per_s": 10 * n_g * steps / el, "ms_per_step": 1e3 * el / steps,
                "kernel_ms (find + score of all passes)": float(np.mean(kern)), "merge_ms (per-pass merge; the candidate fold runs after it)": float(np.mean(merge)),
                "queries_with_hits": int((hits.n_hits > 0).sum())}
        if not args.no_cpu_baseline:
            npar = min(n_g, 16)
            orc = O.OracleIndex(1, 1)
            orc.set_num_docs(self.n_docs)
            orc.set_sort_dense(0, self.pts)
            for t in np.unique(np.concatenate([np.concatenate(gtoks[i]) for i in range(npar)])):
                ids, oi, off = synth.csr_term(self.csr, t)
                if ids.size:
                    orc.load_posting(0, int(t), ids, oi, off)
            bad = 0
            for i in range(npar):
                combos = [orc.make_query(c, sort=osort, fetch_size=100, total_cost=int(j > 0)) for j, c in enumerate(gtoks[i])]
                ref, rqi = orc.search_candidates(combos, cap=2048, ids_cap=0)
                n = int(hits.n_hits[i])
                if n != ref.keys.size or not np.array_equal(hits.keys[i, :n], ref.keys) or not np.array_equal(hits.scores[i, :n], ref.scores) \
                        or not np.array_equal(qi[i, :n].astype(np.int64), rqi.astype(np.int64)) or int(found[i]) != int(ref.n_result_ids):
                    bad += 1
            cand["parity"] = {"checked": npar, "mismatches": bad, "what": "shared Topster (keys, 3 scores, order), query_index of every hit and found vs the oracle's search_all_candidates at %d docs" % self.n_docs}
            orc.close()
        res["candidate_combinations"] = cand

        # ---- (iii) group_by: the distinct Topster (tsgpu_keyword_search_grouped_batch) — both passes of Index::run_search's two-pass protocol ----
        n_u = max(8, (args.batch or 10_000) // 10)
        gtok = synth.keyword_queries(n_u, 3, 8, 2000, seed=51)
        ids64 = np.arange(self.n_docs, dtype=np.uint64)
        n_grp = max(16, self.n_docs // 200)
        distinct = (((ids64 * np.uint64(2654435761)) % np.uint64(n_grp)) * np.uint64(0x100000001B3) + np.uint64(0x517cc1b727220a95)).astype(np.uint64)   # ~n_docs/200 groups
        g.column_set(7, distinct.view(np.int64))
        gqs = [self.T.KwQuery(gtok[i], sort=self.sort, topster_size=K_TOPSTER) for i in range(n_u)]
        garr = self.T.index.make_query_array(gqs)
        gl = 3                                                        # group_limit default of the reference
        first = (B.GroupByC * n_u)()
        second = (B.GroupByC * n_u)()
        for i in range(n_u):
            first[i].group_limit = second[i].group_limit = gl
            first[i].column = second[i].column = 7
            first[i].first_pass = 1
        h1, g1 = self.T.Hits(n_u, K_TOPSTER), self.T.GroupedHits(n_u, K_TOPSTER)
        h2, g2 = self.T.Hits(n_u, K_TOPSTER * gl), self.T.GroupedHits(n_u, K_TOPSTER)
        c1, cg1, c2, cg2 = h1.c_struct(), g1.c_struct(), h2.c_struct(), g2.c_struct()

        def step_g():
            g._ck(g.L.tsgpu_keyword_search_grouped_batch(g.h, garr, first, n_u, C.byref(c1), C.byref(cg1), None))
            g._ck(g.L.tsgpu_keyword_search_grouped_batch(g.h, garr, second, n_u, C.byref(c2), C.byref(cg2), None))
            return None
        gb_rec = {"kern": [], "fold": [], "sel": [], "idp": [], "bytes": [], "ids": [], "slots": []}

        def after_g(_):
            t = g.aux_timings()          # (the SECOND pass of the step: the last grouped batch)
            gb_rec["kern"].append(t.gb_kernels_ms); gb_rec["fold"].append(t.gb_fold_ms); gb_rec["sel"].append(t.gb_select_ms); gb_rec["idp"].append(t.gb_id_pass_ms)
            gb_rec["bytes"].append(t.gb_algorithmic_bytes); gb_rec["ids"].append(t.gb_matched_ids); gb_rec["slots"].append(t.gb_table_slots)
        el, lat, _ = timed(step_g, steps, 2, 1, after_g)
        grp = {"workload": "%d user queries/step, each as the reference runs a group_by request: a FIRST pass (distinct Topster keyed by group, LogLogBeta group count) and a SECOND "
                           "pass (group_limit %d KVs per group, populate_result_kvs order); 3 distinct terms (ranks log-uniform [8,2000]), %d groups over %d documents, Topster 250; host "
                           "outputs" % (n_u, gl, n_grp, self.n_docs),
               "value": n_u * steps / el, "unit": "grouped user queries/s (two passes each)", "ms_per_step": 1e3 * el / steps, "matched_ids_per_step": int(h2.num_matched.sum()),
               "groups_returned_per_query": float(g2.n_groups.mean()), "queries_with_hits": int((h2.n_hits > 0).sum()), "status_nonzero": int((h2.status != 0).sum() + (h1.status != 0).sum())}
        if gb_rec["kern"] and np.mean(gb_rec["kern"]) > 0:
            km, by = float(np.mean(gb_rec["kern"])), float(np.mean(gb_rec["bytes"]))
            ach = by / (km * 1e-3) / 1e9
            grp["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": pmc_traffic([r"gb_score_kernel", r"gb_insert_kernel", r"gb_select_kernel"], ["pmc_kwg_fetch.txt"], field="max"),
                               "kernel": "the gb_* kernels of ONE pass (second pass of the step): gb_score + gb_insert (one thread per matched id) | gb_select (one workgroup per query) | gb_scatter + gb_members",
                               "kernel_ms": km, "fold_ms (score + insert)": float(np.mean(gb_rec["fold"])), "select_ms": float(np.mean(gb_rec["sel"])), "id_pass_ms (host clock: the keyword kernels that produce the matched ids)": float(np.mean(gb_rec["idp"])),
                               "algorithmic_bytes_per_launch": by, "matched_ids": float(np.mean(gb_rec["ids"])), "table_slots": float(np.mean(gb_rec["slots"])),
                               "note": "algorithmic bytes = 36 per matched id (id + its 32-byte record) + 20 per table slot (key, best, rank, count: what the select kernel walks); the kernels are bound by "
                                       "the LATENCY of random table atomics and by one workgroup per query in gb_select, not by bytes: the fraction of HBM peak is small by construction (kw_groupby.hip.h header)"}
        if not args.no_cpu_baseline:
            npar = min(n_u, 8)
            orc = O.OracleIndex(1, 1)
            orc.set_num_docs(self.n_docs)
            orc.set_sort_dense(0, self.pts)
            for t in np.unique(gtok[:npar]):
                ids, oi, off = synth.csr_term(self.csr, t)
                if ids.size:
                    orc.load_posting(0, int(t), ids, oi, off)
            bad = 0
            t_cpu = 0.0
            for i in range(npar):
                oq = orc.make_query(gtok[i], sort=osort, fetch_size=100)
                tc = time.time()
                r1 = orc.search_keyword_grouped(oq, distinct, gl, True)
                r2 = orc.search_keyword_grouped(oq, distinct, gl, False)
                t_cpu += time.time() - tc
                n1, n2 = int(g1.n_groups[i]), int(g2.n_groups[i])
                want1 = sorted(zip(r1.scores[:, 0].tolist(), r1.scores[:, 1].tolist(), r1.scores[:, 2].tolist(), r1.keys.tolist(), r1.distinct_key.tolist(), r1.group_found.tolist()), reverse=True)
                got1 = list(zip(h1.scores[i, :n1, 0].tolist(), h1.scores[i, :n1, 1].tolist(), h1.scores[i, :n1, 2].tolist(), h1.keys[i, :n1].tolist(), g1.distinct_key[i, :n1].tolist(),
                                g1.group_found[i, :n1].tolist()))
                ok = n1 == r1.n_groups and got1 == want1 and int(g1.groups_count[i]) == r1.groups_count and int(g1.groups_total[i]) == r1.groups_exact
                ok = ok and n2 == r2.n_groups and np.array_equal(g2.distinct_key[i, :n2], r2.distinct_key) and np.array_equal(g2.group_found[i, :n2], r2.group_found) \
                    and np.array_equal(g2.group_size[i, :n2], r2.group_size) and int(h2.num_matched[i]) == r2.num_keyword_matches
                for r in range(n2 if ok else 0):
                    a, b = int(r2.begin[r]), int(r2.begin[r + 1])
                    ok = ok and np.array_equal(h2.keys[i, r * gl:r * gl + b - a], r2.keys[a:b]) and np.array_equal(h2.scores[i, r * gl:r * gl + b - a], r2.scores[a:b])
                bad += 0 if ok else 1
            grp["parity"] = {"checked": npar, "mismatches": bad, "what": "first pass: the groups' greatest KVs (as a set), groups_processed, getGroupsCount (LogLogBeta), distinct-key count; second pass: "
                                                                        "group order, every KV of every group, group sizes, groups_processed vs the oracle's distinct Topster at %d docs" % self.n_docs}
            grp["cpu_baseline"] = {"value": npar / t_cpu if t_cpu > 0 else None, "unit": "grouped user queries/s (two passes each)", "cores": 1, "kind": "port",
                                   "sample": "%d of the step's queries, both passes, oracle/oracle_index.h search_keyword_grouped on one core" % npar}
            orc.close()
        # the reference's calling convention for a grouped request: T request threads, each user query = a first-pass call + a second-pass call of ONE query;
        # concurrent calls are coalesced inside the library (the grouped combiner); every call's results against the batch path's (checksums)
        try:
            LG = loadgen_lib()
            want = np.zeros(n_u, np.uint64)
            for i in range(n_u):
                n2 = int(g2.n_groups[i])
                want[i] = LG.tsgpu_loadgen_grouped_checksum(int(g1.n_groups[i]), int(g1.groups_count[i]), n2, g2.distinct_key[i].ctypes.data, g2.group_found[i].ctypes.data,
                                                            g2.group_size[i].ctypes.data, h2.keys[i].ctypes.data, h2.scores[i].ctypes.data, gl)
            fn = C.cast(g.L.tsgpu_keyword_search_grouped_batch, C.c_void_p)
            conc = {}
            for threads in (1, 64, 256):
                calls = max(2, (2000 if threads > 1 else 300) // threads)
                lat = np.zeros(threads * calls, np.float64)
                got = np.zeros(n_u, np.uint64)
                fails = C.c_uint64(0)
                LG.tsgpu_loadgen_grouped(fn, g.h, C.cast(garr, C.c_void_p), n_u, K_TOPSTER, gl, 7, threads, max(1, calls // 4), lat.ctypes.data, got.ctypes.data, C.byref(fails))   # warm-up
                r0, c0 = g.counter("gb_batch_rounds"), g.counter("gb_batch_coalesced_calls")
                wall = LG.tsgpu_loadgen_grouped(fn, g.h, C.cast(garr, C.c_void_p), n_u, K_TOPSTER, gl, 7, threads, calls, lat.ctypes.data, got.ctypes.data, C.byref(fails))
                r1, c1 = g.counter("gb_batch_rounds"), g.counter("gb_batch_coalesced_calls")
                seen = got != 0
                conc[str(threads)] = {"value": threads * calls / wall, "unit": "grouped user queries/s (two 1-query calls each)", "p50_us": float(np.percentile(lat, 50)),
                                      "p99_us": float(np.percentile(lat, 99)), "failures": int(fails.value), "calls_per_round": (c1 - c0) / max(1, r1 - r0),
                                      "checksum_mismatches_vs_batch_path": int((got[seen] != want[seen]).sum()), "queries_checked": int(seen.sum())}
            grp["concurrency"] = conc
        except Exception as e:      # noqa: BLE001  (measurement tooling must not take the leg down)
            grp["concurrency"] = {"error": repr(e)}
        # search_all_candidates with group_by: 10 candidate combinations per user query folded into ONE distinct Topster (tsgpu_keyword_search_grouped_candidates_batch)
        try:
            n_cu = max(4, n_g // 5)
            ccombos = [[self.T.KwQuery(c, sort=self.sort, topster_size=K_TOPSTER, total_cost=(j > 0)) for j, c in enumerate(gtoks[u])] for u in range(n_cu)]
            cres = {}
            for fp in (1, 0):
                tbest = None
                for _ in range(3):
                    t0 = time.time()
                    ch, cg, cq = g.keyword_search_grouped_candidates_batch(ccombos, [(gl, 7, fp, 0, 0)] * n_cu, k_stride=K_TOPSTER * gl, g_stride=K_TOPSTER)
                    dt = time.time() - t0
                    tbest = dt if tbest is None else min(tbest, dt)
                cres[fp] = (ch, cg, cq, tbest)
            cand_g = {"workload": "%d user queries x 10 candidate-token combinations each, group_by (%d groups), both passes; one distinct Topster and one groups_processed per user query" % (n_cu, n_grp),
                      "first_pass_ms": 1e3 * cres[1][3], "second_pass_ms": 1e3 * cres[0][3], "value": n_cu / (cres[1][3] + cres[0][3]), "unit": "grouped user queries/s (10 combinations, two passes each)",
                      "status_nonzero": int((cres[0][0].status != 0).sum() + (cres[1][0].status != 0).sum())}
            if not args.no_cpu_baseline:
                npar = min(n_cu, 2)                      # (20 oracle passes at full size: the leg's share of the default run stays under half a minute)
                orc = O.OracleIndex(1, 1)
                orc.set_num_docs(self.n_docs)
                orc.set_sort_dense(0, self.pts)
                for t in np.unique(np.concatenate([np.concatenate(gtoks[u]) for u in range(npar)])):
                    ids, oi, off = synth.csr_term(self.csr, t)
                    if ids.size:
                        orc.load_posting(0, int(t), ids, oi, off)
                bad = 0
                for u in range(npar):
                    oqs = [orc.make_query(c, sort=osort, fetch_size=100, total_cost=int(j > 0)) for j, c in enumerate(gtoks[u])]
                    for fp in (1, 0):
                        ref, rqi = orc.search_candidates_grouped(oqs, distinct, gl, bool(fp))
                        ch, cg, cq, _ = cres[fp]
                        n = int(cg.n_groups[u])
                        ok = n == ref.n_groups and int(ch.num_matched[u]) == ref.num_keyword_matches and int(cg.groups_total[u]) == ref.groups_exact
                        if ok and fp:
                            want = sorted(zip(ref.scores[:, 0].tolist(), ref.scores[:, 1].tolist(), ref.keys.tolist(), ref.distinct_key.tolist(), ref.group_found.tolist(), rqi.tolist()), reverse=True)
                            got = list(zip(ch.scores[u, :n, 0].tolist(), ch.scores[u, :n, 1].tolist(), ch.keys[u, :n].tolist(), cg.distinct_key[u, :n].tolist(), cg.group_found[u, :n].tolist(), cq[u, :n].tolist()))
                            ok = got == want and int(cg.groups_count[u]) == ref.groups_count
                        elif ok:
                            ok = np.array_equal(cg.distinct_key[u, :n], ref.distinct_key) and np.array_equal(cg.group_found[u, :n], ref.group_found)
                            for r in range(n if ok else 0):
                                a, b = int(ref.begin[r]), int(ref.begin[r + 1])
                                ok = ok and np.array_equal(ch.keys[u, r * gl:r * gl + b - a], ref.keys[a:b]) and np.array_equal(ch.scores[u, r * gl:r * gl + b - a], ref.scores[a:b]) \
                                    and np.array_equal(cq[u, r * gl:r * gl + b - a], rqi[a:b].astype(np.uint32))
                        bad += 0 if ok else 1
                cand_g["parity"] = {"checked": 2 * npar, "mismatches": bad, "what": "both passes of %d user queries vs the oracle's search_all_candidates over one distinct Topster at %d docs "
                                                                                    "(groups, KVs, query_index, groups_processed, group count)" % (npar, self.n_docs)}
                orc.close()
            grp["candidate_combinations"] = cand_g
        except Exception as e:      # noqa: BLE001
            grp["candidate_combinations"] = {"error": repr(e)}
        # q = * with group_by over the whole collection (every document is a matched id: the tables hold 2 x n_docs slots)
        try:
            wq = self.T.KwQuery([], sort=((B.SORT_INT64_COLUMN, 1, 0), (B.SORT_SEQ_ID, 1, 0)), topster_size=K_TOPSTER)
            wres = {}
            for fp in (1, 0):
                best = None
                for _ in range(3):
                    t0 = time.time()
                    wh, wg = g.keyword_search_grouped_batch([wq], [(gl, 7, fp, 0, 1)], k_stride=K_TOPSTER * gl, g_stride=K_TOPSTER)
                    dt = time.time() - t0
                    best = dt if best is None else min(best, dt)
                wres[fp] = (wh, wg, best)
            wild = {"workload": "q = *, group_by over all %d documents (%d groups), sort [points desc, seq_id desc], Topster 250, group_limit %d" % (self.n_docs, n_grp, gl),
                    "first_pass_ms": 1e3 * wres[1][2], "second_pass_ms": 1e3 * wres[0][2], "groups_count": int(wres[1][1].groups_count[0]), "groups_total": int(wres[1][1].groups_total[0])}
            if not args.no_cpu_baseline:
                sc = np.zeros((self.n_docs, 3), np.int64)
                sc[:, 0] = self.pts
                sc[:, 1] = ids64.astype(np.int64)
                bad = 0
                for fp in (1, 0):
                    _, ref = O.group_topster_run(K_TOPSTER, gl, bool(fp), ids64, distinct, sc)
                    wh, wg, _ = wres[fp]
                    n = int(wg.n_groups[0])
                    if fp:
                        want = sorted(zip(ref.scores[:, 0].tolist(), ref.scores[:, 1].tolist(), ref.keys.tolist(), ref.distinct_key.tolist(), ref.group_found.tolist()), reverse=True)
                        got = list(zip(wh.scores[0, :n, 0].tolist(), wh.scores[0, :n, 1].tolist(), wh.keys[0, :n].tolist(), wg.distinct_key[0, :n].tolist(), wg.group_found[0, :n].tolist()))
                        ok = n == ref.n_groups and got == want and int(wg.groups_count[0]) == ref.groups_count
                    else:
                        ok = n == ref.n_groups and np.array_equal(wg.distinct_key[0, :n], ref.distinct_key) and np.array_equal(wg.group_found[0, :n], ref.group_found)
                        for r in range(n if ok else 0):
                            a, b = int(ref.begin[r]), int(ref.begin[r + 1])
                            ok = ok and np.array_equal(wh.keys[0, r * gl:r * gl + b - a], ref.keys[a:b]) and np.array_equal(wh.scores[0, r * gl:r * gl + b - a], ref.scores[a:b])
                    bad += 0 if ok else 1
                wild["parity"] = {"checked": 2, "mismatches": bad, "what": "both passes vs the oracle's distinct Topster fed all %d documents" % self.n_docs}
            grp["wildcard"] = wild
        except Exception as e:      # noqa: BLE001
            grp["wildcard"] = {"error": repr(e)}
        res["group_by"] = grp
        # ---- (iv) facets (do_facets, hash-index branch) over the matched ids of a keyword batch and over q = * ----
        try:
            res["facets"] = self.run_facets(gtok)
        except Exception as e:      # noqa: BLE001
            res["facets"] = {"error": repr(e)}
        return res

    def run_facets(self, gtok):
        """tsgpu_facet_count_batch / _grouped_batch / tsgpu_facet_range_count_batch at the keyword config's size: an ARRAY facet field (1-3 of 2 000 values per
        document, repeats inside a document happen), counted (a) over the per-query id lists of a keyword batch, (b) over all documents (q = *) — plain,
        as the facets of a grouped search (50 000 groups) and as 10 ranges of the points column. Parity: the oracle on the batch's queries; q = * against
        a numpy recount (the oracle's std::map index over 10M documents is not built here)."""
        from oracle import oracle_py as O
        from typesense_amd import _lib as B
        g, args, n = self.g, self.args, self.n_docs
        steps = max(3, min(args.steps, 10))
        ids64 = np.arange(n, dtype=np.uint64)
        per = (1 + (ids64 * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(61)) % np.uint64(3)).astype(np.uint64)
        ptr = np.zeros(n + 1, np.uint64)
        ptr[1:] = np.cumsum(per)
        owner = np.repeat(ids64, per.astype(np.int64))
        pos = np.arange(int(ptr[-1]), dtype=np.uint64) - ptr[owner.astype(np.int64)]
        n_val = 2000
        hashes = ((((owner * np.uint64(2654435761) + pos * np.uint64(40503)) >> np.uint64(7)) % np.uint64(n_val)).astype(np.uint32) * np.uint32(2654435761)).astype(np.uint32)
        g.facet_set(5, ptr, hashes)
        n_f = min(len(gtok), 1000)
        qs = [self.T.KwQuery(gtok[i], sort=self.sort, topster_size=K_TOPSTER) for i in range(n_f)]
        _, lists = g.keyword_search_batch_ids(qs, k_stride=K_TOPSTER)
        cap = 2048
        # the C entry with caller-owned outputs, like the other legs (the numpy wrapper's per-query slicing is not the product)
        ptrs = (C.c_void_p * n_f)(*[x.ctypes.data if x.size else None for x in lists])
        cnts = np.array([x.size for x in lists], np.uint64)
        fo = B.FacetCountsC()
        oh, oc, od, op_ = (np.empty((n_f, cap), np.uint32) for _ in range(4))
        onv = np.zeros(n_f, np.uint32)
        fo.cap, fo.hash, fo.count, fo.doc_id, fo.array_pos, fo.n_values = cap, oh.ctypes.data, oc.ctypes.data, od.ctypes.data, op_.ctypes.data, onv.ctypes.data

        def step_f():
            g._ck(g.L.tsgpu_facet_count_batch(g.h, 5, C.cast(ptrs, C.c_void_p), cnts.ctypes.data_as(C.c_void_p), n_f, 1, None, 0, C.byref(fo)))
            return None
        f_rec = {"kern": [], "cnt": [], "bytes": []}

        def after_f(_):
            t = g.aux_timings()
            f_rec["kern"].append(t.facet_kernels_ms); f_rec["cnt"].append(t.facet_count_ms); f_rec["bytes"].append(t.facet_algorithmic_bytes)
        el, lat, _ = timed(step_f, steps, 1, 1, after_f)
        got = [(oh[q, :min(onv[q], cap)], oc[q, :min(onv[q], cap)], od[q, :min(onv[q], cap)], op_[q, :min(onv[q], cap)], int(onv[q])) for q in range(n_f)]
        out = {"workload": "array facet field (1-3 of %d values per document) over %d documents; (a) the id lists of %d keyword queries (3-term AND) per step, (b) q = *: all "
                           "documents, plain / grouped (the group_by leg's %d groups) / 10 ranges of the points column; host inputs and outputs" % (n_val, n, n_f, max(16, n // 200)),
               "value": n_f * steps / el, "unit": "facet-counted queries/s", "ms_per_step": 1e3 * el / steps, "ids_per_step": int(sum(x.size for x in lists)),
               "values_per_query": float(np.mean([r[4] for r in got]))}
        if f_rec["kern"] and np.mean(f_rec["kern"]) > 0:
            km, by = float(np.mean(f_rec["kern"])), float(np.mean(f_rec["bytes"]))
            ach = by / (km * 1e-3) / 1e9
            out["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": pmc_traffic([r"facet_count_kernel", r"facet_compact_kernel", r"facet_sort_kernel"], ["pmc_kwg_fetch.txt"], field="max"),
                               "kernel": "facet_count_kernel (+ facet_compact + facet_sort)", "kernel_ms": km, "count_kernel_ms": float(np.mean(f_rec["cnt"])), "algorithmic_bytes_per_launch": by,
                               "host_share_of_step": 1.0 - km / (1e3 * el / steps),
                               "note": "algorithmic bytes = 20 per id (id + doc_ptr pair) + 4 per value it holds + 20 per table slot; the step is mostly HOST work — %d pageable id arrays gathered into the "
                                       "pinned staging block, one upload, five downloads, per-query slicing of the outputs — which is why its rate moves with the box's host (580 K - 713 K q/s "
                                       "between two boxes in round 5) while the kernels do not" % n_f}
        everything = [np.arange(n, dtype=np.uint32)]
        pts = np.ascontiguousarray(self.pts, dtype=np.int64)                          # (column 0 of the collection)
        lo_v, hi_v = int(pts.min()), int(pts.max()) + 1
        edges = np.linspace(lo_v, hi_v, 11).astype(np.int64)
        ranges = [(int(edges[r + 1]), int(edges[r])) for r in range(10) if edges[r + 1] > edges[r]]
        wild = {}
        for name, fn in (("plain", lambda: g.facet_count_batch(5, everything, cap=cap)),
                         ("grouped", lambda: g.facet_count_batch(5, everything, cap=cap, group_column=7)),
                         ("ranges", lambda: g.facet_range_count_batch(5, 0, ranges, everything)),
                         ("ranges_grouped", lambda: g.facet_range_count_batch(5, 0, ranges, everything, group_column=7))):
            e2, _, r2 = timed(fn, steps, 1, 1)
            wild[name] = {"ms_per_call": 1e3 * e2 / steps}
            wild["_" + name] = r2
        # q = * recount: every (document, distinct hash) once
        pair = np.unique(owner.astype(np.uint64) << np.uint64(32) | hashes.astype(np.uint64))
        uh, uc = np.unique((pair & np.uint64(0xFFFFFFFF)).astype(np.uint32), return_counts=True)
        h0, c0, d0, p0, n0 = wild.pop("_plain")[0]
        bad = 0 if (n0 == uh.size and np.array_equal(h0, uh[:cap]) and np.array_equal(c0, uc[:cap].astype(np.uint32))) else 1
        rc = wild.pop("_ranges")[0]
        per_doc = np.diff(np.unique(pair >> np.uint64(32), return_index=True)[1], append=pair.size)          # distinct hashes per document
        which = np.searchsorted(np.array([u for u, _ in ranges], np.int64), pts, side="right")
        okr = which < len(ranges)
        okr[okr] &= pts[okr] >= np.array([l for _, l in ranges], np.int64)[which[okr]]
        want_r = np.bincount(which[okr], weights=per_doc[okr], minlength=len(ranges)).astype(np.uint32)
        bad += 0 if np.array_equal(rc, want_r) else 1
        wild.pop("_grouped"); wild.pop("_ranges_grouped")
        wild["parity"] = {"checked": 2, "mismatches": bad, "what": "q = *: plain counts (the first %d values in hash order) and the range counts vs a numpy recount of every (document, distinct hash)" % cap}
        out["wildcard"] = wild
        if not args.no_cpu_baseline:
            npar = min(n_f, 8)
            need = np.unique(np.concatenate([lists[i] for i in range(npar)] + [np.zeros(0, np.uint32)]))
            keep = np.zeros(n, bool)
            keep[need] = True
            sp = np.zeros(n + 1, np.uint64)
            sp[1:] = np.cumsum(np.where(keep, per, 0))
            orc = O.OracleIndex(1, 1)
            orc.facet_set(0, sp, hashes[keep[owner.astype(np.int64)]])               # (only the documents these queries matched: the walk meets no other)
            bad, t0 = 0, time.perf_counter()
            for i in range(npar):
                h, c, d, p, nn = orc.facet_count(0, lists[i])
                gh, gc, gd, gp, gn = got[i]
                bad += 0 if (gn == nn and np.array_equal(gh, h[:cap]) and np.array_equal(gc, c[:cap]) and np.array_equal(gd, d[:cap]) and np.array_equal(gp, p[:cap])) else 1
            cpu_s = time.perf_counter() - t0
            out["parity"] = {"checked": npar, "mismatches": bad, "what": "value hashes, counts, last document and array position of every value vs oracle/facet_count.h on the queries' own id lists"}
            out["cpu_baseline"] = {"value": npar / cpu_s, "unit": "facet-counted queries/s", "cores": 1, "kind": "port", "sample": "%d of the step's queries, oracle/facet_count.h on one core" % npar}
        return out

    def concurrency_keyword(self, arr, n_q, keys, scores, n_hits, num_matched):
        """the reference's calling convention (src/index.cpp:3488, src/http_server.cpp:827-832): T host threads, blocking 1-query calls on one
        context, results to host memory; the library coalesces them (tsgpu_batcher.h). Parity: every call's result == the batch path's."""
        g, args = self.g, self.args
        LG = loadgen_lib()
        T_ = max(1, args.threads)
        calls = max(8, min(400, (4 * n_q) // T_))
        top = FETCH_SIZE
        want = np.zeros(n_q, np.uint64)
        kc, sc = np.ascontiguousarray(keys), np.ascontiguousarray(scores)
        for i in range(n_q):
            want[i] = LG.tsgpu_loadgen_hits_checksum(kc[i].ctypes.data, sc[i].ctypes.data, int(n_hits[i]), int(num_matched[i]), top)
        fn = C.cast(g.L.tsgpu_keyword_search_batch, C.c_void_p)
        out = {}
        def cgroup_cpu():
            # the host side of this leg is CPU work of the request threads: a container CPU quota (cgroup v2 cpu.max) bounds it, and a
            # throttled period stalls every thread for tens of milliseconds -> reported next to the numbers
            try:
                st = dict(l.split() for l in open("/sys/fs/cgroup/cpu.stat"))
                q, per = open("/sys/fs/cgroup/cpu.max").read().split()
                return int(st["usage_usec"]), int(st.get("nr_throttled", 0)), int(st.get("throttled_usec", 0)), (None if q == "max" else float(q) / float(per))
            except Exception:
                return 0, 0, 0, None
        for threads in sorted({1, 16, 128, T_}):
            lat = np.zeros(threads * calls, np.float64)
            got = np.zeros(n_q, np.uint64)
            fails = C.c_uint64(0)
            LG.tsgpu_loadgen_keyword(fn, g.h, C.cast(arr, C.c_void_p), n_q, K_TOPSTER, top, threads, max(2, calls // 8), 1, lat.ctypes.data, got.ctypes.data, C.byref(fails))   # warm-up
            r0, c0 = g.counter("batch_rounds"), g.counter("batch_coalesced_calls")
            PH = ("kw_batches", "kw_plan_us", "kw_upload_us", "kw_launch_us", "kw_wait_us", "kw_book_us", "batch_exec_us", "batch_scatter_us", "kw_queue_us", "kw_wake_us")
            ph0 = [g.counter(n) for n in PH]
            cg0 = cgroup_cpu()
            wall = LG.tsgpu_loadgen_keyword(fn, g.h, C.cast(arr, C.c_void_p), n_q, K_TOPSTER, top, threads, calls, 1, lat.ctypes.data, got.ctypes.data, C.byref(fails))
            cg1 = cgroup_cpu()
            rounds, ccalls = g.counter("batch_rounds") - r0, g.counter("batch_coalesced_calls") - c0
            ph = dict(zip(PH, (g.counter(n) - a for n, a in zip(PH, ph0))))
            nb = max(1, ph.pop("kw_batches"))
            per_call = {"parked_to_round_start": ph.pop("kw_queue_us") / max(1, ccalls), "results_ready_to_caller_resumes": ph.pop("kw_wake_us") / max(1, ccalls)}
            touched = got != 0
            out[str(threads)] = {"threads": threads, "calls": threads * calls, "queries_per_call": 1, "value": threads * calls / wall, "unit": "queries/s",
                                 "p50_us": float(np.percentile(lat, 50)), "p99_us": float(np.percentile(lat, 99)), "failures": int(fails.value),
                                 "queries_per_round": (ccalls / rounds) if rounds else 1.0, "mean_us": float(lat.mean()), "max_us": float(lat.max()),
                                 "batches_per_s": nb / wall, "us_per_batch": {k_[:-3]: v_ / nb for k_, v_ in ph.items()}, "us_per_coalesced_call": per_call,
                                 "host_cpu": {"cpu_us_per_call": (cg1[0] - cg0[0]) / (threads * calls), "cpus_busy": (cg1[0] - cg0[0]) / (wall * 1e6),
                                              "cgroup_cpu_quota_cpus": cg1[3], "throttled_periods": cg1[1] - cg0[1], "throttled_thread_ms": (cg1[2] - cg0[2]) / 1e3},
                                 "parity": {"checked": int(touched.sum()), "mismatches": int((got[touched] != want[touched]).sum()),
                                            "what": "checksum of (n_hits, num_matched, top-100 keys + 3 scores) of every 1-query call vs the 10 000-query batch"}}
        return out

    # ---------------------------------------------------------------- exact k-NN by the oracle, streamed in chunks (parity at 10M)
    def exact_knn_chunked(self, Qh, k, want_rows=True, metric=None, slab_kw=None):
        """oracle flat_knn semantics (exact fp32, hnswlib summation order, ties -> smaller label) over ALL base rows, streamed slab by slab:
        tests/helpers.py::exact_knn_chunked — the same checker the `-m gpu` at-size tests use (tests/test_gpu_at_size.py). Parity legs only."""
        from oracle import oracle_py as O
        tdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests")
        if tdir not in sys.path:
            sys.path.insert(0, tdir)
        import helpers as H
        m = O.METRIC_IP if metric is None else metric
        return H.exact_knn_chunked(self.n_docs, self.args.dim, {m: np.ascontiguousarray(Qh)}, k, want_rows=want_rows, slab_kw=slab_kw)[m]

    # ---------------------------------------------------------------- vector (config 3)
    def knn_run(self, g, field, Q, n_q, k, steps, warmup):
        from typesense_amd import _lib as B
        torch, world = self.torch, self.world
        dist_o = torch.zeros((n_q, k), dtype=torch.float32, device="cuda")
        lab_o = torch.zeros((n_q, k), dtype=torch.int64, device="cuda")
        cnt_o = torch.zeros(n_q, dtype=torch.int32, device="cuda")
        rec = dict(kern_ms=[], flops=[], scan_ms=[], scan_bytes=[], post_ms=[])

        if self.sharded and self.group is not None and g is self.g:
            self.group_works("k-NN", lambda: self.group.vec_knn_batch_raw(field, Q.data_ptr(), B.MEM_DEVICE, n_q, k, dist_o.data_ptr(), lab_o.data_ptr(), cnt_o.data_ptr(), B.MEM_DEVICE))

        def step():
            if self.sharded and self.group is not None and g is self.g:
                # the exchange behind the C-ABI: per-GPU k nearest as one u64 {ord(dist), label} per hit, ONE ncclAllGather, vec_group_merge_kernel
                self.group.vec_knn_batch_raw(field, Q.data_ptr(), B.MEM_DEVICE, n_q, k, dist_o.data_ptr(), lab_o.data_ptr(), cnt_o.data_ptr(), B.MEM_DEVICE)
                return dist_o, lab_o, cnt_o
            g.vec_knn_batch_raw(field, Q.data_ptr(), B.MEM_DEVICE, n_q, k, dist_o.data_ptr(), lab_o.data_ptr(), cnt_o.data_ptr(), B.MEM_DEVICE)
            return dist_o, lab_o, cnt_o                   # (1 GPU, the unsharded twin, or one of N independent replicas)

        def after(_):
            tm = g.timings()
            rec["kern_ms"].append(tm.vec_knn_ms)
            rec["flops"].append(tm.vec_flops)
            rec["scan_ms"].append(tm.vec_scan_ms)
            rec["scan_bytes"].append(tm.vec_scan_bytes)
            rec["post_ms"].append(tm.vec_merge_ms)
        elapsed, lat, out = timed(step, steps, warmup, world, after)
        r = {k2: float(np.mean(v)) for k2, v in rec.items()}
        r.update(elapsed=elapsed, steps=steps, lat=lat, n_q=n_q)
        return r, out

    def run_vector(self):
        from typesense_amd import _lib as B, synth
        torch, g, args, world = self.torch, self.g, self.args, self.world
        n, dim, k, n_q = self.n_docs, args.dim, args.k, args.vec_batch
        self.Q = synth.random_vectors(max(n_q, 1024) if self.extras else n_q, dim, seed=4 + self.qseed, device="cuda")
        Q = self.Q
        f0, o0 = g.counter("vec_prefilter_fallbacks"), g.counter("vec_overflow_rounds")
        res, out = self.knn_run(g, 1, Q, n_q, k, args.steps, args.warmup)
        res.update(prefilter=int(self.opts.get("vec_prefilter", 1)), fallbacks=g.counter("vec_prefilter_fallbacks") - f0,
                   overflow_rounds=g.counter("vec_overflow_rounds") - o0)
        d_gpu, l_gpu, c_gpu = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()
        if self.head == "vector" and args.dump_outputs:
            self.set_dump(c_gpu, {}, dict(distances=d_gpu, labels=l_gpu))

        if self.twin is not None and self.rank == 0:
            m = min(n_q, 16)
            td, tl, tc = self.twin.vec_knn_batch(1, Q[:m].cpu().numpy(), k)
            bad = sum(1 for i in range(m) if not (np.array_equal(l_gpu[i], tl[i].astype(np.int64)) and np.array_equal(d_gpu[i].view(np.uint32), td[i].view(np.uint32))))
            res["shard_parity"] = {"checked": m, "mismatches": bad, "against": "the unsharded 10M x %d matrix on rank 0 (labels + distance bits)" % dim}

        if world == 1 and res["prefilter"] and args.full:
            # parity leg 1 (GPU vs GPU): the bf16 bracket path must return exactly what the fp32 scan of EVERY row returns
            m = min(n_q, 16)
            g.set_option("vec_prefilter", 0)
            fd, fl, fc = g.vec_knn_batch(1, Q[:m].cpu().numpy(), k)
            g.set_option("vec_prefilter", 1)
            same_sets = sum(1 for i in range(m) if set(fl[i].tolist()) == set(l_gpu[i].tolist()))
            same_order = sum(1 for i in range(m) if np.array_equal(fl[i].astype(np.int64), l_gpu[i]))
            rel = float(np.max(np.abs(fd - d_gpu[:m]) / np.maximum(1.0, np.abs(fd))))
            res["parity_fp32_scan"] = {"queries": m, "identical_top%d_sets" % k: same_sets, "identical_order": same_order, "max_rel_distance_diff": rel,
                                       "what": "bf16-bracket path vs vec_prefilter=0 (fp32 MFMA scan of every row, no pruning) at %d rows" % n}

        if self.extras:
            # config 3's other batch sizes (B = 256 is the timed headline above)
            sweep = {}
            for bq in (1, 16, 64, 1024):
                r, _ = self.knn_run(g, 1, Q, bq, k, 3, 1)
                sweep[str(bq)] = {"value": bq * r["steps"] / r["elapsed"], "unit": "queries/s", "ms_per_step": 1e3 * r["elapsed"] / r["steps"], "scan_ms": r["scan_ms"],
                                  "hbm_frac": r["scan_bytes"] / (r["scan_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS if r["scan_ms"] > 0 else None,
                                  "bf16_mfma_frac": r["flops"] / (r["scan_ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF if r["scan_ms"] > 0 else None}
            res["batch_sweep"] = sweep
            res["concurrency"] = self.concurrency_knn(Q, d_gpu, l_gpu, k)

        if self.rank == 0 and world == 1 and not args.no_cpu_baseline:
            from oracle import oracle_py as O
            ncpu = os.cpu_count() or 1
            # parity leg 2 (GPU vs the oracle at FULL size): exact flat scan of all rows, streamed in chunks
            npar = min(n_q, 64)
            t0 = time.time()
            Qh = Q[:npar].cpu().numpy()
            ed, el, rows = self.exact_knn_chunked(Qh, k)
            t_exact = time.time() - t0
            self.exact = (Qh, ed, el, rows)
            sets_ok = sum(1 for i in range(npar) if set(el[i].tolist()) == set(l_gpu[i].tolist()))
            order_ok = sum(1 for i in range(npar) if np.array_equal(el[i].astype(np.int64), l_gpu[i]))
            bits_ok = sum(1 for i in range(npar) if np.array_equal(ed[i].view(np.uint32), d_gpu[i].view(np.uint32)))
            rel = float(np.max(np.abs(ed - d_gpu[:npar]) / np.maximum(1.0, np.abs(ed))))
            res["parity"] = {"sets_checked": npar, "identical_top%d_sets" % k: sets_ok, "identical_order (ties -> smaller label)": order_ok,
                             "distance_bits_identical": bits_ok, "max_rel_distance_diff": rel, "tolerance": "1e-5 relative (north star); measured: bit-identical to the oracle (hnswlib SSE-build summation order, vec_ip_lanes=4; the oracle reproduces the reference's pinned distances, tests/test_vector_pins.py)",
                             "mismatches": npar - min(sets_ok, order_ok) + (1 if rel > 1e-5 else 0),
                             "what": "top-%d of %d queries vs the oracle's exact flat scan (hnswlib summation order) of ALL %d rows, streamed in 2^20-row chunks" % (k, npar, n)}
            # CPU baseline: the same chunked scan IS the reference's flat path on this box's cores (one query per thread)
            qps_cpu = npar / t_exact
            xs = self.base_slab(0, min(1 << 20, n))[:400_000].cpu().numpy()
            orc = O.OracleIndex(1, 1)
            orc.vec_init(dim, O.METRIC_IP)
            orc.vec_add(np.arange(xs.shape[0], dtype=np.uint32), xs)
            qs = Q[:max(ncpu, 8)].cpu().numpy()
            orc.bench_vector(qs[:ncpu], k, ncpu)
            wall, per = orc.bench_vector(qs, k, ncpu)
            qps_sample = qs.shape[0] / wall
            res["cpu"] = dict(value=qps_sample * xs.shape[0] / n, unit="queries/s", cores=ncpu, cgroup_cpu_quota_cpus=cpu_quota_cpus(), kind="port",
                              sample="exact flat scan (1 - q.x, hnswlib SSE-build 4-lane order: what the reference compiles to with its stock flags) of %d queries over the first %d of %d base vectors on %d "
                                     "host threads, %.1f q/s on the sample, scaled by %d/%d (cost is linear in N); the full-size parity scan above ran "
                                     "%d queries over all %d rows in %.1f s incl. regenerating + copying the rows (%.2f q/s)"
                                     % (qs.shape[0], xs.shape[0], n, ncpu, qps_sample, xs.shape[0], n, npar, n, t_exact, qps_cpu))
            quota = cpu_quota_cpus()
            if quota and int(quota) < ncpu:
                nt = max(1, int(quota))
                qs_q = qs[:max(nt, 8)]
                wall_q, _ = orc.bench_vector(qs_q, k, nt)
                v_q = qs_q.shape[0] / wall_q * xs.shape[0] / n
                res["cpu"]["at_quota_threads"] = {"threads": nt, "value": v_q, "unit": "queries/s"}
                if v_q > res["cpu"]["value"]:      # the faster configuration is the baseline that is quoted; both are stated
                    res["cpu"]["all_visible_cores"] = {"threads": ncpu, "value": res["cpu"]["value"], "unit": "queries/s"}
                    res["cpu"]["value"], res["cpu"]["cores"] = v_q, nt
            orc.close()
        return res

    def concurrency_knn(self, Q, d_gpu, l_gpu, k):
        g, args = self.g, self.args
        LG = loadgen_lib()
        T_ = max(1, args.threads)
        n_q = d_gpu.shape[0]
        Qh = np.ascontiguousarray(Q[:n_q].cpu().numpy())
        fn = C.cast(g.L.tsgpu_vec_knn_batch, C.c_void_p)
        calls = 6
        lat = np.zeros(T_ * calls, np.float64)
        lab = np.zeros((n_q, k), np.uint64)
        dist = np.zeros((n_q, k), np.float32)
        fails = C.c_uint64(0)
        r0, c0 = g.counter("batch_rounds"), g.counter("batch_coalesced_calls")
        LG.tsgpu_loadgen_knn(fn, g.h, 1, Qh.ctypes.data, n_q, Qh.shape[1], k, T_, 2, lat.ctypes.data, lab.ctypes.data, dist.ctypes.data, C.byref(fails))
        wall = LG.tsgpu_loadgen_knn(fn, g.h, 1, Qh.ctypes.data, n_q, Qh.shape[1], k, T_, calls, lat.ctypes.data, lab.ctypes.data, dist.ctypes.data, C.byref(fails))
        rounds, ccalls = g.counter("batch_rounds") - r0, g.counter("batch_coalesced_calls") - c0
        touched = min(n_q, T_ * calls)
        bad = sum(1 for i in range(touched) if not (np.array_equal(lab[i].astype(np.int64), l_gpu[i]) and np.array_equal(dist[i].view(np.uint32), d_gpu[i].view(np.uint32))))
        return {"threads": T_, "calls": T_ * calls, "queries_per_call": 1, "value": T_ * calls / wall, "unit": "queries/s", "p50_us": float(np.percentile(lat, 50)),
                "p99_us": float(np.percentile(lat, 99)), "failures": int(fails.value), "queries_per_round": (ccalls / rounds) if rounds else 1.0,
                "parity": {"checked": touched, "mismatches": bad, "what": "labels + distance bits of every 1-query call vs the %d-query batch" % n_q}}

    def run_vector_variants(self):
        """config 3's cosine variant and a clustered, L2-normalised collection (the hard case for the bf16 bracket: many near-ties):
        throughput, survivors that reach the exact re-score, fallbacks to the fp32 scan, and parity of a few queries vs the fp32 scan"""
        from typesense_amd import _lib as B, synth
        g, args, k, n_q = self.g, self.args, self.args.k, self.args.vec_batch
        out = {}
        for name, field, metric, kw, qkw in (("cosine", 2, B.METRIC_COSINE, {}, {}),
                                             ("clustered_unit_ip", 3, B.METRIC_IP, {"clustered": True}, {"clustered": True})):
            self.load_vectors(g, field, metric, 0, self.n_docs, **kw)
            Q = self.base_slab(12345, 12345 + n_q, **qkw).contiguous() if qkw else synth.random_vectors(n_q, args.dim, seed=4, device="cuda")
            if qkw:
                Q = Q + 0.05 * synth.random_vectors(n_q, args.dim, seed=99, device="cuda")      # near (not at) base points of some clusters
            f0, o0, g0 = g.counter("vec_prefilter_fallbacks"), g.counter("vec_overflow_rounds"), g.counter("vec_prefilter_groups")
            g.set_option("vec_count_rescored", 1)
            r, o = self.knn_run(g, field, Q, n_q, k, 3, 1)
            surv = g.counter("vec_rescored_rows") / n_q
            g.set_option("vec_count_rescored", 0)
            m = 8
            pd, pl, _ = g.vec_knn_batch(field, Q[:m].cpu().numpy(), k)
            g.set_option("vec_prefilter", 0)
            fd, fl, _ = g.vec_knn_batch(field, Q[:m].cpu().numpy(), k)
            g.set_option("vec_prefilter", 1)
            par_oracle = None
            if name == "cosine" and self.rank == 0 and not args.no_cpu_baseline:
                # cosine at FULL size vs the ORACLE (normalize_vector on insert and on the query, include/index.h:379-388; exact flat scan of all rows)
                from oracle import oracle_py as O
                mo = 4
                Qh = Q[:mo].cpu().numpy()
                ed, el, _ = self.exact_knn_chunked(Qh, k, want_rows=False, metric=O.METRIC_COSINE)
                par_oracle = {"queries": mo, "identical_order": sum(1 for i in range(mo) if np.array_equal(el[i].astype(np.int64), pl[i].astype(np.int64))),
                              "distance_bits_identical": sum(1 for i in range(mo) if np.array_equal(ed[i].view(np.uint32), pd[i].view(np.uint32))),
                              "max_rel_distance_diff": float(np.max(np.abs(ed - pd[:mo]) / np.maximum(1e-30, np.abs(ed)))),
                              "what": "top-%d of %d cosine queries vs the oracle's exact flat scan of all %d normalised rows" % (k, mo, self.n_docs)}
                par_oracle["mismatches"] = mo - min(par_oracle["identical_order"], par_oracle["distance_bits_identical"])
            out[name] = {"value": n_q * r["steps"] / r["elapsed"], "unit": "queries/s", "ms_per_step": 1e3 * r["elapsed"] / r["steps"], "scan_ms": r["scan_ms"],
                         "post_ms": r["post_ms"], "rows_rescored_per_query": surv, "prefilter_fallbacks": g.counter("vec_prefilter_fallbacks") - f0,
                         "prefilter_groups": g.counter("vec_prefilter_groups") - g0, "overflow_rounds": g.counter("vec_overflow_rounds") - o0,
                         "parity_fp32_scan": {"queries": m, "identical_sets": sum(1 for i in range(m) if set(pl[i].tolist()) == set(fl[i].tolist())),
                                              "max_rel_distance_diff": float(np.max(np.abs(pd - fd) / np.maximum(1.0, np.abs(fd))))}}
            if par_oracle is not None:
                out[name]["parity"] = par_oracle
            # (the field's 45 GB stay allocated until the context closes: 288 GB of HBM)
        return out

    # ---------------------------------------------------------------- HNSW (parity UNPINNED: hnswlib is not under /root/reference)
    def run_hnsw(self):
        """searchKnnCloserFirst on a resident graph: q/s by batch and ef, recall@k against the exact scan, the traversal checked bit for bit
        against the oracle's restatement walking the SAME graph, and that restatement timed on the host cores as cpu_baseline (port).
        The graph is built in batches on the device (tsgpu_vec_hnsw_build; --hnsw-graph inserted: hnswlib's row-by-row insertion inside the
        library, knn: the round-2 stand-in); the collection has a 32-dimensional latent structure (i.i.d. N(0,1) rows are equidistant in 768
        dimensions: no graph index has recall there, measured 0.007)."""
        from typesense_amd import _lib as B, synth, hnsw_synth
        torch, args = self.torch, self.args
        # a context of its own, closed when the leg ends: its rows, bf16 mirror, graph and visited sets go back to the device (the three 10M x 768 fields of
        # the vector legs stay resident in self.g; with a 2M-row HNSW collection next to them the general-kernel leg ran out of HBM)
        g = self.T.GpuIndex(torch.cuda.current_device())
        for name, val in self.opts.items():
            g.set_option(name, val)
        try:
            return self._run_hnsw(g)
        finally:
            g.close()
            torch.cuda.empty_cache()

    def _run_hnsw(self, g):
        from typesense_amd import _lib as B, synth, hnsw_synth
        torch, args = self.torch, self.args
        n, dim, k, M, field = args.hnsw_rows, args.dim, args.k, 16, 7
        t0 = time.time()
        X = synth.latent_vectors(n, dim, seed=3, device="cuda")
        g.vec_create(field, dim, B.METRIC_IP, n)
        lab = torch.arange(n, dtype=torch.int64, device="cuda")
        inserted = args.hnsw_graph == "inserted"
        bulk = args.hnsw_graph == "bulk"
        build_threads = max(1, int(cpu_quota_cpus() or os.cpu_count() or 1))
        build_info = None
        if bulk:
            # the graph of a LOADED collection: built in batches on the device over the rows the field holds (tsgpu_vec_hnsw_build; M 16, ef_construction 200,
            # seed 100: include/index.h:365-367's defaults). Levels as hnswlib draws them; the rows with level >= 2 and the first 1 024 inserted on the host.
            g.vec_upsert_device(field, lab.data_ptr(), X.data_ptr(), n)
            torch.cuda.synchronize()
            t1 = time.time()
            build_info = g.vec_hnsw_build(field, M=M, ef_construction=200, seed=100, threads=build_threads)
            torch.cuda.synchronize()
            t_build = time.time() - t1
            graph = g.vec_hnsw_export(field)
        elif inserted:
            # the graph the reference would have: hnswlib's addPoint in label order (M 16, ef_construction 200, seed 100: include/index.h:365-367),
            # built INSIDE the library while the rows are upserted (tsgpu_hnsw_build.h), concurrently like the reference's indexing threads
            g.vec_hnsw_enable(field, M=M, ef_construction=200, seed=100, threads=build_threads)
            t1 = time.time()
            step_rows = 1 << 16
            for a in range(0, n, step_rows):
                b = min(n, a + step_rows)
                g.vec_upsert_device(field, lab[a:b].data_ptr(), X[a:b].data_ptr(), b - a)
            torch.cuda.synchronize()
            t_build = time.time() - t1
            graph = g.vec_hnsw_export(field)
        else:
            g.vec_upsert_device(field, lab.data_ptr(), X.data_ptr(), n)
            torch.cuda.synchronize()
            t1 = time.time()
            graph = hnsw_synth.build_graph(torch, g, field, X, M=M, K0=64, seed=100, batch=1024)
            torch.cuda.synchronize()
            t_build = time.time() - t1
            g.vec_hnsw_load(field, graph)
        nq_max = max(args.hnsw_batch, 256)
        Q = synth.latent_vectors(nq_max, dim, seed=4, device="cuda")
        res = {"metric": "HNSW k-NN queries/s (searchKnnCloserFirst, k=%d), PARITY UNPINNED: hnswlib is absent from the reference tree; the traversal is "
                         "checked against the oracle's restatement of the published algorithm on the same graph" % k,
               "unit": "queries/s", "dtype": "f32",
               "config": {"workload": ("%d x %d unit rows with a 32-dim latent structure + 0.3 noise (synth.latent_vectors), M=%d, ef_construction 200, seed 100: the graph built in "
                                       "batches ON THE DEVICE (tsgpu_vec_hnsw_build: hnswlib's level draw, ef_construction beam, neighbour heuristic and reverse-link rule applied per "
                                       "batch; %d seed rows inserted by %d host threads)" % (n, dim, M, build_info["n_seed"], build_threads)) if bulk else
                                      ("%d x %d unit rows with a 32-dim latent structure + 0.3 noise (synth.latent_vectors), M=%d, ef_construction 200, seed 100: hnswlib's incremental "
                                       "addPoint in label order INSIDE the library (tsgpu_vec_hnsw_enable), %d host threads per 65 536-row upsert" % (n, dim, M, build_threads)) if inserted else
                                      ("%d x %d unit rows with a 32-dim latent structure + 0.3 noise (synth.latent_vectors), M=%d, graph = exact %d-NN lists + "
                                       "getNeighborsByHeuristic2 + reverse links, built on the GPU (graph: knn-heuristic, NOT hnswlib's insertion-order graph)" % (n, dim, M, 64)),
                          "rows": n, "graph": args.hnsw_graph, "graph_build": build_info, "graph_build_s": t_build, "graph_build_rows_per_s": n / t_build if t_build > 0 else None, "collection_s": t1 - t0, "maxlevel": int(graph["maxlevel"]), "mean_level0_degree": float(graph["link0"][:, 0].mean())},
               "runs": []}
        de = torch.zeros((256, k), dtype=torch.float32, device="cuda"); le = torch.zeros((256, k), dtype=torch.int64, device="cuda"); ce = torch.zeros(256, dtype=torch.int32, device="cuda")
        g.vec_knn_batch_raw(field, Q.data_ptr(), B.MEM_DEVICE, 256, k, de.data_ptr(), le.data_ptr(), ce.data_ptr(), B.MEM_DEVICE)
        torch.cuda.synchronize()
        le_h = le.cpu().numpy()
        keep = {}
        for ef in (100, 200, 400) + ((800,) if n > 3_000_000 else ()):      # (a 10M-row graph needs a wider beam for recall 0.9 on this data)
            for nq in sorted({256, args.hnsw_batch}):
                d = torch.zeros((nq, k), dtype=torch.float32, device="cuda"); l = torch.zeros((nq, k), dtype=torch.int64, device="cuda"); c = torch.zeros(nq, dtype=torch.int32, device="cuda")
                def step():
                    g.vec_hnsw_search_batch_raw(field, Q.data_ptr(), B.MEM_DEVICE, nq, k, ef, d.data_ptr(), l.data_ptr(), c.data_ptr(), B.MEM_DEVICE)
                el, _, _ = timed(step, 5, 2, 1)
                lh = l[:256].cpu().numpy()
                rec = float(np.mean([len(set(lh[i].tolist()) & set(le_h[i].tolist())) / k for i in range(256)]))
                dist_q = g.counter("hnsw_last_distances") / nq
                run = {"ef": ef, "batch": nq, "value": nq * 5 / el, "unit": "queries/s", "ms_per_batch": 1e3 * el / 5, "recall_at_%d" % k: rec,
                       "expansions_per_query": g.counter("hnsw_last_expansions") / nq, "distances_per_query": dist_q,
                       "row_bytes_GBs": dist_q * dim * 4 * nq * 5 / el / 1e9}
                res["runs"].append(run)
                keep[(ef, nq)] = (d[:256].cpu().numpy(), lh, c[:256].cpu().numpy())
        # the same headline batch with 16-bit visited TAGS (2 B x rows x concurrent queries of HBM) instead of the per-query hash sets
        # (the default since round 3: 32-256 KB per query whatever the row count): what the memory saving costs
        if int(self.opts.get("hnsw_visited_hash", 1)) != 0:
            nq = args.hnsw_batch
            d = torch.zeros((nq, k), dtype=torch.float32, device="cuda"); l = torch.zeros((nq, k), dtype=torch.int64, device="cuda"); c = torch.zeros(nq, dtype=torch.int32, device="cuda")
            g.set_option("hnsw_visited_hash", 0)
            try:
                el, _, _ = timed(lambda: g.vec_hnsw_search_batch_raw(field, Q.data_ptr(), B.MEM_DEVICE, nq, k, 100, d.data_ptr(), l.data_ptr(), c.data_ptr(), B.MEM_DEVICE), 5, 2, 1)
                same = bool(np.array_equal(l[:256].cpu().numpy(), keep[(100, nq)][1]))
                res["visited_tags_variant"] = {"ef": 100, "batch": nq, "value": nq * 5 / el, "unit": "queries/s", "identical_to_hash_visited": same,
                                               "visited_bytes": 2 * n * min(nq, 4096)}
            except Exception as e:      # noqa: BLE001 (the tags may not fit: reported, the headline stands)
                res["visited_tags_variant"] = {"error": repr(e)}
            finally:
                g.set_option("hnsw_visited_hash", 1)
        # the quoted run: the smallest ef whose recall@k reaches 0.9 (the reference's default ef = 10 means max(ef, k) = k = 100 candidates)
        cands = [x for x in res["runs"] if x["batch"] == args.hnsw_batch]
        good = [x for x in cands if x["recall_at_%d" % k] >= 0.9]
        head = good[0] if good else cands[-1]
        res["value"] = head["value"]
        res["ef"] = head["ef"]
        res["recall_at_%d" % k] = head["recall_at_%d" % k]
        res["roofline"] = {"bound": "hbm", "achieved": head["row_bytes_GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": head["row_bytes_GBs"] / HBM_PEAK_GBS, "traffic": None,
                           "note": "algorithmic bytes = distances computed x dim x 4 B (fp32 rows fetched at random, 3 KB each; link lists and visited tags not "
                                   "counted) over the kernel time of the QUOTED run (ef = %d, batch %d: the smallest ef with recall@%d >= 0.9; "
                                   "at the reference's effective ef = max(ef, k) = %d recall@%d is %.2f on this data: runs[])" % (
                                       head["ef"], head["batch"], k, k, k, next((x["recall_at_%d" % k] for x in cands if x["ef"] == k), float("nan")))}
        if not args.no_cpu_baseline and n > 3_000_000:
            res["parity"] = {"queries_checked": 0, "pinned": False, "what": "skipped: the oracle's copy of %d x %d rows (+ the graph) is not held on the host beyond 3M rows" % (n, dim)}
        elif not args.no_cpu_baseline:
            from oracle import oracle_py as O
            t2 = time.time()
            orc = O.OracleIndex(1, 1)
            orc.vec_init(dim, O.METRIC_IP)
            S = 1 << 18
            for a in range(0, n, S):
                b = min(n, a + S)
                orc.vec_add(np.arange(a, b, dtype=np.uint32), X[a:b].cpu().numpy())
            orc.hnsw_import(graph)
            ncpu = os.cpu_count() or 1
            Qh = synth.latent_vectors(max(64 * ncpu, 4096), dim, seed=4, device="cuda").cpu().numpy()      # (same stream as Q: its first rows are the GPU's queries)
            npar = 64
            bad = 0
            for ef in (100, 400):
                od, ol, oc = orc.hnsw_search_batch(Qh[:npar], k, ef, threads=ncpu)
                gd, gl, gc = keep[(ef, 256)]
                for i in range(npar):
                    m = int(oc[i])
                    if not (gc[i] == m and np.array_equal(gl[i, :m].astype(np.uint64), ol[i, :m]) and np.array_equal(gd[i, :m].view(np.uint32), od[i, :m].view(np.uint32))):
                        bad += 1
            res["parity"] = {"queries_checked": 2 * npar, "mismatches": bad, "pinned": False,
                             "what": "labels, order and distance bits of %d queries at ef=100 and ef=400 vs the oracle's restatement of searchKnnCloserFirst walking the "
                                     "same %d-node graph (hnsw_import); hnswlib itself is absent: parity unpinned" % (npar, n)}
            orc.hnsw_search_batch(Qh[:ncpu], k, res["ef"], threads=ncpu)
            t3 = time.time()
            orc.hnsw_search_batch(Qh, k, res["ef"], threads=ncpu)
            wall = time.time() - t3
            res["cpu_baseline"] = {"value": Qh.shape[0] / wall, "unit": "queries/s", "cores": ncpu, "cgroup_cpu_quota_cpus": cpu_quota_cpus(), "kind": "port",
                                   "sample": "%d queries at ef=%d (the quoted run's) through the oracle's HNSW restatement (scalar distances in the SSE-build order, pooled visited tags) on %d host threads, "
                                             "same graph, same rows; oracle load + import took %.0f s" % (Qh.shape[0], res["ef"], ncpu, t3 - t2)}
            res["speedup_vs_cpu_baseline"] = res["value"] / res["cpu_baseline"]["value"]
            orc.close()
        del X
        return res

    # ---------------------------------------------------------------- hybrid (config 4)
    def run_hybrid(self):
        from typesense_amd import _lib as B, synth
        torch, g, args, world = self.torch, self.g, self.args, self.world
        n_q, k = args.vec_batch, args.k
        qtok = synth.keyword_queries(n_q, 3, 8, 2000, seed=5 + self.qseed)
        qs = [self.T.KwQuery(qtok[i], sort=self.sort, topster_size=K_TOPSTER) for i in range(n_q)]
        arr = self.kw_query_array(qtok)
        if not hasattr(self, "Q"):      # (the vector leg did not run: --workload hybrid without --full)
            self.Q = synth.random_vectors(n_q, args.dim, seed=4 + self.qseed, device="cuda")
        Qh = self.Q[:n_q].cpu().numpy()
        if not self.sharded:                      # 1 GPU, or replicas: every rank fuses its own slice of the global batch
            def step():
                return g.hybrid_search_batch(qs, 1, Qh, k=k, fetch_size=100, alpha=0.3, k_stride=K_TOPSTER)
        else:
            dev, hs = device_hits(torch, n_q, K_TOPSTER)
            dist_o = torch.zeros((n_q, k), dtype=torch.float32, device="cuda")
            lab_o = torch.zeros((n_q, k), dtype=torch.int64, device="cuda")
            cnt_o = torch.zeros(n_q, dtype=torch.int32, device="cuda")

            self.group_works("hybrid", lambda: self.group.hybrid_search_batch(qs, 1, B.METRIC_IP, None, k=k, fetch_size=100, alpha=0.3, k_stride=K_TOPSTER,
                                                                               mem_q=B.MEM_DEVICE, q_ptr=self.Q.data_ptr(), dim=args.dim))

            def step():      # fuse AFTER the shard merge: reciprocal ranks are global ranks
                # tsgpu_group_hybrid_search_batch: merged Topsters (250, with text_match) + merged k nearest, then the reference's fusion
                return self.group.hybrid_search_batch(qs, 1, B.METRIC_IP, None, k=k, fetch_size=100, alpha=0.3, k_stride=K_TOPSTER,
                                                      mem_q=B.MEM_DEVICE, q_ptr=self.Q.data_ptr(), dim=args.dim)
        steps = args.steps
        elapsed, lat, out = timed(step, steps, min(args.warmup, 2), world)
        res = dict(elapsed=elapsed, steps=steps, lat=lat, n_q=n_q)
        if out is not None:
            res["fused_hits"] = int(out.n_hits.sum())
            if self.head == "hybrid" and args.dump_outputs:
                self.set_dump(out.n_hits, dict(num_matched=out.num_matched, status=out.status),
                              dict(keys=out.keys, scores=out.scores, text_match=out.text_match, vector_distance=out.vector_distance))
        if self.twin is not None and self.rank == 0:
            m = min(n_q, 16)
            th = self.twin.hybrid_search_batch(qs[:m], 1, Qh[:m], k=k, fetch_size=100, alpha=0.3, k_stride=K_TOPSTER)
            bad = 0
            for i in range(m):
                nn = int(th.n_hits[i])
                if int(out.n_hits[i]) != nn or not np.array_equal(out.keys[i, :nn], th.keys[i, :nn]) or not np.array_equal(out.scores[i, :nn], th.scores[i, :nn]):
                    bad += 1
            res["shard_parity"] = {"checked": m, "mismatches": bad, "against": "the unsharded collection on rank 0 (fused keys + score bits)"}
        if self.rank == 0 and world == 1 and not args.no_cpu_baseline and self.exact is not None:
            # parity at full size: fused Topster (key, score bits) of the first queries vs oracle.search_hybrid. The oracle's keyword half
            # runs on the loaded terms of these queries; its vector store holds the rows of the oracle's OWN exact top-100 over all 10M rows
            # (exact_knn_chunked): flat_knn over a superset of the true top-100 returns exactly the true top-100.
            from oracle import oracle_py as O
            Qe, ed, el, rows = self.exact
            m = min(n_q, Qe.shape[0], 32)
            orc = O.OracleIndex(1, 1)
            orc.set_num_docs(self.n_docs)
            orc.set_sort_dense(0, self.pts)
            for t in np.unique(qtok[:m]):
                ids, oi, off = synth.csr_term(self.csr, t)
                if ids.size:
                    orc.load_posting(0, int(t), ids, oi, off)
            orc.vec_init(args.dim, O.METRIC_IP)
            labs = np.array(sorted(rows.keys()), np.uint32)
            orc.vec_add(labs, np.stack([rows[int(x)] for x in labs]))
            osort = ((O.SORT_TEXT_MATCH, 0, 1), (O.SORT_INT64_COLUMN, 0, 1))
            bad = chk = 0
            t0 = time.time()
            for i in range(m):
                ref = orc.search_hybrid(orc.make_query(qtok[i], sort=osort, fetch_size=100, topster_size=K_TOPSTER), Qe[i], k=k, alpha=0.3, cap=1024)
                nn = int(out.n_hits[i])
                chk += 1
                if nn != ref.keys.size or not np.array_equal(out.keys[i, :nn], ref.keys) or not np.array_equal(out.scores[i, :nn], ref.scores) \
                        or not np.array_equal(out.vector_distance[i, :nn].view(np.uint32), ref.vector_distance.view(np.uint32)):
                    bad += 1
            res["parity"] = {"checked": chk, "mismatches": bad,
                             "what": "fused Topster after rank fusion: keys, all 3 score words (fused score bits), vector_distance bits vs oracle.search_hybrid at 10M docs"}
            if self.extras:
                # rerank_hybrid_matches (Index::compute_aux_scores): the same batch with the re-ranking pass, and its parity — the oracle also needs
                # the rows of the keyword-only hits (their distance is computed by label)
                def step_r():
                    return g.hybrid_search_batch(qs, 1, Qh, k=k, fetch_size=100, alpha=0.3, k_stride=K_TOPSTER, rerank=True)
                el_r, _, out_r = timed(step_r, 3, 1, 1)
                need = np.unique(np.concatenate([out_r.keys[i, :int(out_r.n_hits[i])] for i in range(m)])).astype(np.int64)
                need = need[~np.isin(need, labs.astype(np.int64))]
                S = 1 << 20
                for s0 in range(0, self.n_docs, S):
                    sel = need[(need >= s0) & (need < s0 + S)]
                    if sel.size:
                        x = self.base_slab(s0, min(self.n_docs, s0 + S))[torch.from_numpy(sel - s0).cuda()].cpu().numpy()
                        orc.vec_add(sel.astype(np.uint32), x)
                bad_r = 0
                for i in range(m):
                    ref = orc.search_hybrid(orc.make_query(qtok[i], sort=osort, fetch_size=100, topster_size=K_TOPSTER), Qe[i], k=k, alpha=0.3, cap=1024, rerank=True)
                    nn = int(out_r.n_hits[i])
                    if nn != ref.keys.size or not np.array_equal(out_r.keys[i, :nn], ref.keys) or not np.array_equal(out_r.scores[i, :nn], ref.scores) \
                            or not np.array_equal(out_r.text_match[i, :nn], ref.text_match) \
                            or not np.array_equal(out_r.vector_distance[i, :nn].view(np.uint32), ref.vector_distance.view(np.uint32)):
                        bad_r += 1
                res["rerank_hybrid_matches"] = {"value": n_q * 3 / el_r, "unit": "queries/s", "ms_per_step": 1e3 * el_r / 3,
                                                "parity": {"checked": m, "mismatches": bad_r,
                                                           "what": "Index::compute_aux_scores (src/index.cpp:8793-8923) after the fusion: keys, re-fused score bits, the filled-in "
                                                                   "text_match scores and vector_distance bits vs the oracle's restatement at 10M docs"}}
            orc.close()
        return res

    def close(self):
        if self.group is not None:
            self.group.close()
            self.group = None
        self.g.close()
        if self.twin is not None:
            self.twin.close()


def line_common(args, world, value, elapsed, steps, lat):
    return {"value": value, "unit": "queries/s", "n_gpus": world, "steps": steps, "ms_per_step": 1e3 * elapsed / steps,
            "p50_ms_per_batch": 1e3 * float(np.median(lat))}


COMPACT_LIMIT = 6144            # bytes: the driver parsed 17 KB lines and lost a 20 KB one (round 4); the last stdout line stays far below either


def _r(x, nd=4):
    """floats to `nd` significant digits (the full-precision values are in the detail record)."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return float("%.*g" % (nd + 2, x))
    return x


def _pick(d, keys):
    return {k: _r(d[k]) for k in keys if isinstance(d, dict) and k in d and not isinstance(d[k], (dict, list))}


def _short(s, n):
    s = str(s)
    return s if len(s) <= n else s[:n - 3] + "..."


def _parity_small(p):
    """{checked, mismatches} of a parity object whatever its leg calls the counters."""
    if not isinstance(p, dict):
        return None
    checked = next((p[k] for k in ("checked", "sets_checked", "queries_checked", "n_checked", "queries", "user_queries_checked") if k in p), None)
    mism = next((p[k] for k in ("mismatches", "mismatched", "n_mismatch", "mismatched_queries") if k in p), None)
    out = {"checked": checked, "mismatches": mism}
    if "vs" in p:
        out["vs"] = _short(p["vs"], 60)
    return out


def _roof_small(rf):
    if not isinstance(rf, dict):
        return None
    out = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "algorithmic_bytes_per_launch", "flops_per_launch",
                     "algorithmic_frac", "touched_bytes_per_launch", "touched_frac", "traffic_frac", "unique_list_bytes", "l2_refetch", "find_kernel_ms", "hbm_frac", "mfma_frac"))
    if "counter" in rf:
        out["counter"] = _short(rf["counter"], 90)
    if "kernel" in rf:
        out["kernel"] = _short(rf["kernel"], 72)
    return out


def _cpu_small(c):
    if not isinstance(c, dict):
        return None
    out = _pick(c, ("value", "unit", "cores", "kind"))
    if "sample" in c:
        out["sample"] = _short(c["sample"], 110)
    return out


def _sub_small(o):
    """a secondary config (vector / hybrid) reduced to what the contract asks of it."""
    out = _pick(o, ("value", "unit", "ms_per_step", "p50_ms_per_batch", "steps"))
    rf = o.get("roofline") or {}
    out["roofline"] = _pick(rf, ("bound", "frac", "kernel_ms", "achieved", "peak", "unit"))
    if rf.get("kernel") or rf.get("dominant_kernel"):
        out["roofline"]["kernel"] = _short(rf.get("kernel") or rf.get("dominant_kernel"), 40)
    if isinstance(o.get("cpu_baseline"), dict):
        out["cpu_baseline"] = _pick(o["cpu_baseline"], ("value", "unit", "cores", "kind"))
    if "parity" in o:
        out["parity"] = _parity_small(o["parity"])
    if isinstance(o.get("shard_parity"), dict):
        out["shard_parity"] = _parity_small(o["shard_parity"])
    return out


def compact_line(full, detail_path=None):
    """The LAST stdout line: the contract's keys + `roofline` + `cpu_baseline` + `parity`, `vector` / `hybrid` reduced to
    {value, ms_per_step, roofline.frac, cpu_baseline.value, parity.mismatches}; everything else lives in the detail record."""
    line = {k: _r(full.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                          "vs_baseline", "dtype", "data")}
    cfg = full.get("config") or {}
    line["config"] = {"workload": _short(cfg.get("workload", ""), 260), "parallelism": _short(cfg.get("parallelism", ""), 200),
                      "results_to": _short(cfg.get("results_to", ""), 120)}
    for k in ("p50_ms_per_batch", "queries_with_hits", "value_device_only", "ms_per_step_device_only", "value_two_callers", "value_host_pinned", "speedup_vs_cpu_baseline"):
        if k in full:
            line[k] = _r(full[k])
    line["roofline"] = _roof_small(full.get("roofline"))
    iu = (full.get("roofline") or {}).get("issue_util")
    if isinstance(iu, dict) and line["roofline"] is not None:
        line["roofline"]["issue_util"] = _pick(iu, ("valu", "salu", "pmc_of_these_sources"))
    line["cpu_baseline"] = _cpu_small(full.get("cpu_baseline"))
    line["parity"] = _parity_small(full.get("parity"))
    if isinstance(full.get("shard_parity"), dict):
        line["shard_parity"] = _parity_small(full["shard_parity"])
    if isinstance(full.get("exchange_check"), dict):
        line["exchange_check"] = _pick(full["exchange_check"], ("pruned_equals_full_exchange", "local_ms", "exchange_merge_ms", "exchange_bytes_per_gpu", "hit_exchange_bytes_per_gpu",
                                                                "full_topk_hit_exchange_bytes_per_gpu", "own_slice_delivery_equals_full_result"))
    for k in ("replicas", "replicas_strong"):
        if isinstance(full.get(k), dict):
            line[k] = _pick(full[k], ("value", "unit", "ms_per_step", "global_batch", "scaling"))
    if isinstance(full.get("wildcard_sharded"), dict):
        line["wildcard_sharded"] = _pick(full["wildcard_sharded"], ("ms_per_call", "docs_ranked_per_s"))
        if "shard_parity" in full["wildcard_sharded"]:
            line["wildcard_sharded"]["shard_parity"] = _parity_small(full["wildcard_sharded"]["shard_parity"])
    if isinstance(full.get("group_by_sharded"), dict):
        gs_ = full["group_by_sharded"]
        line["group_by_sharded"] = _pick(gs_, ("value", "unit", "ms_first_pass", "ms_second_pass", "error"))
        if "shard_parity" in gs_:
            line["group_by_sharded"]["shard_parity"] = _parity_small(gs_["shard_parity"])
    if isinstance(full.get("candidate_combinations_sharded"), dict):
        cs = full["candidate_combinations_sharded"]
        line["candidate_combinations_sharded"] = _pick(cs, ("value", "unit", "ms_per_call"))
        if isinstance(cs.get("shard_parity"), dict):
            line["candidate_combinations_sharded"]["shard_parity"] = _parity_small(cs["shard_parity"])
    conc = full.get("concurrency")
    if isinstance(conc, dict):
        line["concurrency"] = {t: _pick(c, ("value", "p50_us", "p99_us")) for t, c in conc.items() if isinstance(c, dict)}
    gk = full.get("general_kernels")
    if isinstance(gk, dict):
        line["general_kernels"] = {}
        for name, o in gk.items():
            if isinstance(o, dict):
                e = _pick(o, ("value", "unit", "ms_per_step", "kernel_ms", "find_ms", "score_ms"))
                if isinstance(o.get("roofline"), dict):
                    e["roofline"] = _pick(o["roofline"], ("bound", "frac", "kernel_ms", "achieved", "peak", "unit"))
                if "parity" in o:
                    e["parity"] = _parity_small(o["parity"])
                line["general_kernels"][name] = e
    for name in ("vector", "hybrid", "keyword"):
        if isinstance(full.get(name), dict):
            line[name] = _sub_small(full[name])
    hn = (full.get("vector") or {}).get("hnsw") if isinstance(full.get("vector"), dict) else full.get("hnsw")
    if isinstance(hn, dict):
        line["hnsw"] = _pick(hn, ("value", "unit", "rows", "ef", "batch", "recall_at_100"))
        cfg = hn.get("config") or {}
        line["hnsw"]["rows"] = cfg.get("rows")
        line["hnsw"]["graph"] = cfg.get("graph")
        line["hnsw"]["graph_build_s"] = cfg.get("graph_build_s")
        line["hnsw"]["parity"] = "UNPINNED (hnswlib is not under /root/reference); traversal = the oracle's restatement"
    if isinstance(full.get("distributed"), dict):
        line["distributed"] = _pick(full["distributed"], ("backend", "world_size", "rccl", "mode", "group_transport"))
    line["detail"] = detail_path
    # the contract is a byte budget, not a hope: shed the optional objects, last added first, until the line fits
    for k in ("hnsw", "general_kernels", "concurrency", "replicas", "replicas_strong", "exchange_check", "keyword", "hybrid", "vector"):
        if len(json.dumps(line)) <= COMPACT_LIMIT:
            break
        line.pop(k, None)
    return line


def emit(full, detail_out=None):
    """Full record -> the detail file (+ one stderr line); compact record -> the last (and only) stdout line."""
    path = detail_out or os.path.join(ROOT, "gpurun_out", "bench_detail.json")
    shown = None
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f)
        shown = os.path.relpath(path, ROOT)
    except OSError as e:
        sys.stderr.write("bench.py: could not write the detail record to %s: %s\n" % (path, e))
    sys.stderr.write("BENCH_DETAIL " + json.dumps(full) + "\n")
    sys.stderr.flush()
    sys.stdout.flush()
    print(json.dumps(compact_line(full, shown)), flush=True)


def main():
    args = parse()
    if args.dry:
        with open(args.dry) as f:
            emit(json.load(f), args.detail_out or os.path.join("/tmp", "bench_detail_dry.json"))
        return
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU visible: bench.py measures the HIP path only (there is no CPU fallback)"}))
        sys.exit(2)
    rank, world, _, backend = dist_setup(args.gpus)
    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    barrier(world)

    wl = args.workload
    if wl == "all" and not args.full:
        wl = "keyword"          # a plain run times the headline's leg only
    bn = Bench(args, rank, world)
    out = {}
    build_s = {}
    if wl in ("all", "keyword", "hybrid", "kwgeneral"):
        build_s["keyword_index"] = bn.build_keyword()
    if wl in ("all", "vector", "hybrid"):
        build_s["vector_index"] = bn.build_vectors()
    if wl in ("all", "keyword"):
        out["keyword"] = bn.run_keyword()
    if wl in ("all", "vector") or (wl == "hybrid" and args.full):
        out["vector"] = bn.run_vector()
    if wl in ("all", "hybrid"):
        out["hybrid"] = bn.run_hybrid()
    if wl in ("all", "vector") and bn.extras:
        t0 = time.time()
        out["vector"]["variants"] = bn.run_vector_variants()
        build_s["vector_variants (build + run)"] = time.time() - t0
        if args.hnsw_rows > 0:
            t0 = time.time()
            out["vector"]["hnsw"] = bn.run_hnsw()
            build_s["hnsw leg (collection + graph + runs + oracle)"] = time.time() - t0
    if world == 1 and (wl == "kwgeneral" or (wl in ("all", "keyword") and bn.extras)):
        t0 = time.time()
        out["keyword_general"] = bn.run_keyword_general()       # (last: it adds a second string field to the keyword index)
        build_s["general-kernel keyword legs (second field + runs + oracle)"] = time.time() - t0
    if wl == "hnsw":                                # only the HNSW leg (tools/gpu_profile.sh runs it at BASELINE config 3's 10M rows)
        t0 = time.time()
        hn = bn.run_hnsw()
        bn.close()
        print(json.dumps({"metric": "HNSW leg at %d x %d rows" % (args.hnsw_rows, args.dim), "n_gpus": world, "data": "synthetic", "hnsw": hn, "leg_s": time.time() - t0}))
        return
    bn.close()
    if wl == "kwgeneral":
        print(json.dumps({"metric": "queries/sec, general keyword kernels at %d docs" % args.n_docs, "n_gpus": world, "data": "synthetic", "general_kernels": out.get("keyword_general"),
                          "index_build_s": build_s}))
        return
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, bn.dump)

    sharded = world > 1 and args.dist_mode == "shards"
    mult = world if (world > 1 and not sharded) else 1            # replicas: the global batch is world x the per-GPU batch
    dist_info = None
    if world > 1:
        import torch.distributed as dist
        dist_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "rccl": backend == "nccl", "mode": args.dist_mode,
                     "group_transport": getattr(bn, "group_transport", None) if sharded else None,
                     "measured": "this line is what ran; no scaling curve is claimed here — the driver computes efficiency from the per-N values"}
    if world == 1:
        par = "1 GPU"
    elif sharded:
        par = "doc-range shards x%d of the SAME 10M-doc collection, bound-pruned exchange of the per-GPU top-100 + counts, exact device merge; exchange = %s" % (world, bn.exchange)
    else:
        par = "%d independent replicas of the collection, every rank answers its own batch (global batch = %d x the per-GPU batch), no collective" % (world, world)
    vocab, tpd = (100_000, 32) if args.n_docs >= 1_000_000 else (20_000, 16)
    sub = {}
    if "keyword" in out:
        r = out["keyword"]
        qps = mult * r["n_q"] * args.steps / r["elapsed"]
        kw = line_common(args, world, qps, r["elapsed"], args.steps, r["lat"])
        kw["config"] = {"workload": "BASELINE config 2: %d-doc Zipf(1.0) text, V=%d, %d tokens/doc, %d postings/shard; %d queries/step, 3 distinct "
                                    "terms ranks log-uniform [8,2000], Topster 250, sort [_text_match desc, points desc], num_typos=0, prefix=false"
                                    % (args.n_docs, vocab, tpd, r["n_postings"], r["n_q"] * mult),
                        "parallelism": par,
                        "results_to": ("HOST memory inside the timed steps (tsgpu_hits mem=HOST, pageable arrays: what the B1 seam hands to the server's Topster — the arrays "
                                       "its shim requests for a query that sorts on _text_match: keys, scores[3], match_score_index, n_hits, num_matched, status; "
                                       "value_host_all_arrays = text_match and vector_distance delivered as well); "
                                       "value_device_only = the same batch with device-resident outputs") if world == 1 else
                                      "device (every rank holds the merged result), then every rank copies the 1/N query slice it merged to pinned host memory over its own PCIe link, inside the timed steps"}
        kw["queries_with_hits"] = r.get("nonempty")
        if r.get("host_all_arrays_ms"):
            kw["value_host_all_arrays"] = r["n_q"] / (r["host_all_arrays_ms"] * 1e-3)
            kw["ms_per_step_host_all_arrays"] = r["host_all_arrays_ms"]
        hp = r.get("host_pinned")
        if hp and hp.get("ms_per_step"):
            kw["value_host_pinned"] = r["n_q"] / (hp["ms_per_step"] * 1e-3)
            kw["host_pinned"] = dict(hp, what="the headline's batch with the caller's result arrays in pinned host memory (allocated once, reused): the copy-out is one DMA per array")
        elif hp:
            kw["host_pinned"] = hp
        tc = r.get("two_callers")
        if tc and tc.get("elapsed"):
            kw["value_two_callers"] = r["n_q"] * tc["batches"] / tc["elapsed"]
            kw["two_callers"] = {"batches": tc["batches"], "ms_per_batch": 1e3 * tc["elapsed"] / tc["batches"], "same_as_one_caller": tc["same_as_one_caller"],
                                 "what": "two request threads, each issuing the headline's blocking host-delivered batch call (both calls are cut into chained slices over the lanes): no gain over one caller, whose own slices already hide most of the copy-out"}
        elif tc:
            kw["two_callers"] = tc
        if r.get("elapsed_dev"):
            kw["value_device_only"] = mult * r["n_q"] * args.steps / r["elapsed_dev"]       # outputs left in HBM: the single-launch form the roofline / rocprof durations refer to
            kw["ms_per_step_device_only"] = 1e3 * r["elapsed_dev"] / args.steps
        if args.full:      # (the keyword roofline is computed from the device-only and byte-counting legs)
            achieved = r["alg_bytes"] / (r["kern_ms"] * 1e-3) / 1e9 if r["kern_ms"] > 0 else 0.0
            find_rx, score_rx = r"kw_find2_kernel<3(, false)?>|kw_search_kernel<3, 512, true, true>", r"kw_score_kernel<3, 512, false, false, true>"      # (not the COUNT instantiation's one launch)
            # (max over the dispatches = the full 10 000-query launch: the profiled command also runs the host-delivery leg, whose slices
            #  are smaller launches of the same kernels and would dilute an average)
            traffic = pmc_traffic([find_rx, score_rx], ["pmc_kw_fetch.txt", "pmc_kw_s5_fetch.txt"], field="max")
            # What bounds the kernel. SURVEY 8(d)'s figure — algorithmic bytes / kernel time / 8 TB/s — is 1.3-1.4: above 1, because the
            # find kernel SKIPS (only the shortest list is scanned; the others are met per overlapping run or per candidate) — it is kept as
            # `algorithmic_frac`, it bounds nothing. The line's `frac` is the utilisation of the find kernel's busiest issue port, the CU's one scalar
            # unit (SQ_INSTS_SALU of the round's committed --pmc pass / (live kernel cycles x 256 CUs)); `touched_*` = the bytes the kernels REQUEST, counted
            # by the find kernel itself (kw_count_touched instantiation, one extra untimed step of the same batch); `traffic` = what left L2 (FETCH_SIZE);
            # `l2_refetch` = traffic / the bytes the batch's DISTINCT lists occupy (ids + block records + directories + offsets).
            roof = {"algorithmic_achieved_GBs": achieved, "algorithmic_frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                    "kernel": "kw_find2_kernel<3> (two driver blocks per iteration) + kw_score_kernel<512> (the two halves of the intersect+score+select step, "
                              "launched back to back; kernel_ms spans both)", "kernel_ms": r["kern_ms"], "merge_kernel_ms": r["merge_ms"],
                    "algorithmic_bytes_per_launch": r["alg_bytes"],
                    "note": "bound = the find kernel's busiest issue port (scalar unit: loop control, exec-mask bookkeeping, v_readlane window reads, spilled SGPRs) with "
                            "dependent LDS / L2 latency behind it; algorithmic_frac (SURVEY 8(d): 4*sum|L_t| + offsets + sort keys over kernel time over 8 TB/s) exceeds 1 "
                            "because the kernel skips — it is not a distance to any limit; touched_frac / traffic_frac are the byte rates that do exist."}
            if r["find_ms"] > 0:
                fa = r["alg_bytes"] / (r["find_ms"] * 1e-3) / 1e9
                roof["find_kernel_ms"] = r["find_ms"]
                roof["find_kernel_alone_algorithmic_frac"] = fa / HBM_PEAK_GBS
            tch = r.get("touched")
            if tch and r["kern_ms"] > 0:
                tb = tch["find_requested_bytes"] + tch["score_requested_bytes"]
                fp = tch["footprint"]
                uniq = fp["ids_bytes"] + fp["block_metadata_bytes"] + fp["directory_bytes"] + fp["payload_bytes"]
                roof["touched_bytes_per_launch"] = tb
                roof["touched_frac"] = tb / (r["kern_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                roof["touched"] = {k: tch[k] for k in ("find_requested_bytes", "find_driver_ids", "find_metadata", "find_tile_dma", "find_probes", "find_records",
                                                      "find_work_items", "find_hit_records", "score_requested_bytes")}
                roof["touched"]["note"] = ("counted by kw_find2_kernel<3, COUNT=true> itself (every lane adds the width of its own loads / LDS-DMA words / stores; one untimed step "
                                           "of the same batch); score_requested_bytes = hit records x the score kernel's fixed request sizes")
                roof["unique_list_bytes"] = uniq
                roof["unique_lists"] = fp
                roof["requested_over_unique"] = tb / uniq if uniq else None
                if traffic:
                    roof["l2_refetch"] = traffic / uniq if uniq else None
                    roof["l2_refetch_x2"] = 2.0 * traffic / uniq if uniq else None
                    roof["l2_hit_rate_of_requests"] = max(0.0, 1.0 - traffic / tb) if tb else None
            if traffic and r["kern_ms"] > 0:
                roof["traffic_frac"] = traffic / (r["kern_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                roof["traffic_frac_x2"] = 2.0 * roof["traffic_frac"]      # upper bound if every read were a wide one (FETCH_SIZE halves those on gfx950)
                roof["algorithmic_over_fetched"] = r["alg_bytes"] / traffic
            sq1 = ["pmc_kw_sq1.txt", "pmc_kw_s5_sq1.txt"]
            valu = pmc_counter(find_rx, sq1, "SQ_INSTS_VALU", field="max")
            salu = pmc_counter(find_rx, sq1, "SQ_INSTS_SALU", field="max")
            lds = pmc_counter(find_rx, sq1, "SQ_INSTS_LDS", field="max")
            cyc = (r["find_ms"] or r["kern_ms"]) * 1e-3 * 2.4e9
            # THE ROOFLINE (HBM-bound integer path): achieved = the algorithmic bytes of the launch / the live duration of the two kernels, peak = 8 TB/s.
            # The fraction exceeds 1 because the find kernel SKIPS (leap-frog: only the shortest list is scanned, the others are met per overlapping run or per
            # candidate) — SURVEY 8(d) says so in advance; `traffic` (FETCH_SIZE) and `touched_*` (counted by the kernel itself) are the byte rates that exist.
            roof.update({"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "note": "frac > 1 = leap-frog skipping (algorithmic bytes 4*sum|L_t| + offsets + sort keys are not all fetched), not a distance to a limit. What the "
                                 "find kernel waits for is the NUMBER of dependent steps per candidate (block search, four LDS metadata reads, nine dependent LDS reads, "
                                 "compaction barrier, one directory load per survivor): round 6 halved its scalar instructions (slower), cut its vector instructions 5 % (-1 %), "
                                 "made the probed directories L2-resident (< 1 %), round 5 cut its tile bytes 30 % (0) — profiles/r06/exp_find2_valu.txt; issue_util gives the ports."})
            if valu and salu and cyc > 0:
                # issue capacity per CU and cycle: a wave64 VALU instruction holds one of the CU's four 16-lane SIMDs for 4 cycles -> 1 VALU wave-instruction per CU
                # and cycle; ONE scalar unit -> 1 SALU instruction. Kernel cycles = its live HIP-event duration at the 2.4 GHz peak clock. The counters come from
                # the committed --pmc pass; `pmc_of_these_sources` says whether that pass profiled the kernel sources this run was built from.
                meta = _pmc_meta(sq1[0])
                cur = kernel_src_sha16()
                roof["issue_util"] = {"valu": valu / (cyc * 256), "salu": salu / (cyc * 256), "insts_valu": valu, "insts_salu": salu, "insts_lds": lds,
                                      "pmc_file": os.path.relpath(_profile(sq1[0]) or "profiles/", ROOT), "pmc_kernel_src_sha16": (meta or {}).get("kernel_src_sha16"),
                                      "kernel_src_sha16": cur, "pmc_of_these_sources": bool(meta) and meta.get("kernel_src_sha16") == cur,
                                      "note": "wave-instructions of the find kernel (rocprofv3 --pmc, own pass) / (live kernel cycles x 256 CUs x 1 per cycle); no port is saturated"}
            kw["roofline"] = roof
        for key in ("concurrency", "uncached", "shard_parity", "replicas", "replicas_strong", "exchange_check", "candidate_combinations_sharded", "wildcard_sharded", "group_by_sharded"):
            if key in r:
                kw[key] = r[key]
        if "cpu" in r:
            kw["cpu_baseline"] = r["cpu"]
            kw["speedup_vs_cpu_baseline"] = qps / r["cpu"]["value"] if r["cpu"]["value"] else None
        if "parity" in r:
            kw["parity"] = r["parity"]
        if "keyword_general" in out:
            kw["general_kernels"] = out["keyword_general"]
        sub["keyword"] = kw
    if "vector" in out:
        r = out["vector"]
        qps = mult * r["n_q"] * r["steps"] / r["elapsed"]
        tf = r["flops"] / (r["kern_ms"] * 1e-3) / 1e12 if r["kern_ms"] > 0 else 0.0
        v = line_common(args, world, qps, r["elapsed"], r["steps"], r["lat"])
        v["metric"] = "queries/sec, 10M x 768 fp32 exact inner-product top-100"
        v["dtype"] = "f32"
        v["config"] = {"workload": "BASELINE config 3: %d x %d fp32 N(0,1) base, %d queries/step, k=%d, dist = 1 - q.x" % (args.n_docs, args.dim, r["n_q"], args.k),
                       "parallelism": par}
        if r["prefilter"] and r["scan_ms"] > 0:
            # dominant kernel = vec_hscan_kernel (bf16 bracket scan of every row). Two floors: the bf16 mirror streamed once
            # (HBM) and 2*N*D*B flops on the bf16 MFMA; the larger one is the bound for this batch size.
            gbs = r["scan_bytes"] / (r["scan_ms"] * 1e-3) / 1e9
            tfh = r["flops"] / (r["scan_ms"] * 1e-3) / 1e12
            t_hbm, t_mfma = r["scan_bytes"] / (HBM_PEAK_GBS * 1e9), r["flops"] / (MFMA_BF16_PEAK_TF * 1e12)
            hbm_bound = t_hbm >= t_mfma
            v["roofline"] = {"bound": "hbm" if hbm_bound else "mfma", "achieved": gbs if hbm_bound else tfh,
                             "peak": HBM_PEAK_GBS if hbm_bound else MFMA_BF16_PEAK_TF, "unit": "GB/s" if hbm_bound else "TFLOP/s",
                             "frac": (gbs / HBM_PEAK_GBS) if hbm_bound else (tfh / MFMA_BF16_PEAK_TF),
                             "traffic": pmc_traffic(r"vec_hscan_kernel", ["pmc_vec_fetch.txt", "pmc_vec_s4_fetch.txt"], field="max", scale=2.0),
                             "kernel": "vec_hscan_kernel<%d> (bf16 bracket scan; survivors re-scored exactly in fp32)" % (4 if r["n_q"] > 128 else (2 if r["n_q"] > 64 else 1)),
                             "kernel_ms": r["scan_ms"], "algorithmic_bytes_per_launch": r["scan_bytes"], "flops_per_launch": r["flops"],
                             "hbm_GBs": gbs, "bf16_mfma_TFs": tfh, "pre_ms (query cast + sample pass + threshold)": r["kern_ms"] - r["scan_ms"],
                             "post_ms (refine + fp32 re-score + select)": r["post_ms"],
                             "prefilter_fallbacks": r["fallbacks"], "overflow_rounds": r["overflow_rounds"],
                             # measured, not nominal: the same kernel with everything but its MFMAs compiled out (no DMA, no operand fetches, no
                             # epilogue; profiles/r02/exp_vec_abl_mfma.txt) runs the 256-query scan of 10M x 768 in 2.49 ms
                             "mfma_issue_ceiling_TFs": MFMA_BF16_ISSUE_CEILING_TF, "frac_of_mfma_issue_ceiling": tfh / MFMA_BF16_ISSUE_CEILING_TF,
                             "note": "bound chosen from the nominal peaks (HBM 8 TB/s vs dense bf16 MFMA 2.5 PFLOP/s); back-to-back v_mfma_f32_32x32x16_bf16 "
                                     "from this kernel's two waves per SIMD deliver %.0f TFLOP/s (MFMA-only ablation), which at 256 queries per row makes MFMA "
                                     "issue (2.5 ms), not HBM (1.9 ms), the floor of the scan" % MFMA_BF16_ISSUE_CEILING_TF}
        else:
            traffic = pmc_traffic(r"vec_scan_kernel", "pmc_vec_final_fetch.txt")
            v["roofline"] = {"bound": "mfma", "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF,
                             "traffic": traffic, "kernel": "vec_scan_kernel<2,true> (+ sample pass and selects inside the timed events)",
                             "kernel_ms": r["kern_ms"], "flops_per_launch": r["flops"]}
        for key in ("parity", "parity_fp32_scan", "batch_sweep", "concurrency", "variants", "hnsw", "shard_parity"):
            if key in r:
                v[key] = r[key]
        if "cpu" in r:
            v["cpu_baseline"] = r["cpu"]
            v["speedup_vs_cpu_baseline"] = qps / r["cpu"]["value"] if r["cpu"]["value"] else None
        sub["vector"] = v
    if "hybrid" in out:
        r = out["hybrid"]
        qps = mult * r["n_q"] * r["steps"] / r["elapsed"]
        h = line_common(args, world, qps, r["elapsed"], r["steps"], r["lat"])
        h["metric"] = "queries/sec, 10M-doc hybrid (keyword + 768-d vector, reciprocal rank fusion alpha=0.3), Topster 250"
        h["config"] = {"workload": "BASELINE config 4: configs 2+3 on the same 10M ids, %d queries/step, k_vec=%d; keyword pass + exact k-NN on the GPU, "
                                   "fusion (src/index.cpp:4094-4211) on the host, results delivered to host memory" % (r["n_q"], args.k),
                       "parallelism": par + (" (fusion after the merge)" if sharded else "")}
        h["fused_hits_per_batch"] = r.get("fused_hits")
        for key in ("parity", "shard_parity", "rerank_hybrid_matches"):
            if key in r:
                h[key] = r[key]
        if "vector" in sub and "roofline" in sub["vector"]:
            h["roofline"] = {"note": "a hybrid step = the keyword pass (its roofline: `roofline` of the keyword object) + one k-NN batch (dominant: "
                                     "vec_hscan_kernel, `vector.roofline`) + host rank fusion; the dominant kernel of the step is the k-NN scan",
                             "dominant_kernel": sub["vector"]["roofline"].get("kernel"), "bound": sub["vector"]["roofline"].get("bound"),
                             "frac": sub["vector"]["roofline"].get("frac")}
        kc = sub.get("keyword", {}).get("cpu_baseline")
        vc = sub.get("vector", {}).get("cpu_baseline")
        if kc and vc and kc["value"] and vc["value"]:
            h["cpu_baseline"] = {"value": 1.0 / (1.0 / kc["value"] + 1.0 / vc["value"]), "unit": "queries/s", "cores": kc["cores"], "kind": "port",
                                 "sample": "composed from the two measured legs (a hybrid query on the CPU = one keyword query + one exact flat scan, "
                                           "src/index.cpp:4036-4221): 1 / (1/keyword_cpu + 1/vector_cpu); fusion itself is microseconds"}
        sub["hybrid"] = h

    head = "keyword" if "keyword" in sub else ("vector" if wl == "vector" else "hybrid")
    hd = sub[head]
    line = {"metric": "queries/sec, 10M-doc keyword 3-term AND top-100 (Topster 250)" if head == "keyword" else hd.get("metric"),
            "value": hd["value"], "unit": "queries/s", "n_gpus": world, "steps": hd["steps"], "warmup": args.warmup, "ms_per_step": hd["ms_per_step"],
            "higher_is_better": True, "scaling": "strong" if sharded else "weak", "vs_baseline": None, "dtype": "u32/i64" if head == "keyword" else "f32",
            "data": "synthetic", "config": hd["config"], "p50_ms_per_batch": hd["p50_ms_per_batch"]}
    for k in ("queries_with_hits", "value_device_only", "ms_per_step_device_only", "value_two_callers", "two_callers", "value_host_pinned", "host_pinned", "value_host_all_arrays", "ms_per_step_host_all_arrays", "roofline", "cpu_baseline", "speedup_vs_cpu_baseline", "parity", "shard_parity", "exchange_check", "replicas", "replicas_strong", "candidate_combinations_sharded", "wildcard_sharded", "group_by_sharded", "concurrency",
              "uncached", "general_kernels", "fused_hits_per_batch", "parity_fp32_scan", "batch_sweep", "variants", "hnsw", "rerank_hybrid_matches"):
        if k in hd:
            line[k] = hd[k]
    if dist_info:
        line["distributed"] = dist_info
    line["index_build_s"] = build_s
    for k, v in sub.items():
        if k != head:
            line[k] = v
    if rank == 0:
        emit(line, args.detail_out)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
