"""Infix search (tsgpu_infix_search_batch) measured step by step, next to a host restatement of the reference's loop on the same machine.

Corpus: the bench's keyword collection (BASELINE config 2: Zipf(1.0) text, 32 tokens per document, V = 100 000 terms; --vocab-scale 10 for the second run) with a
synthetic vocabulary: every term id gets a word of 5-12 lower-case letters derived from a hash of the id. Patterns: substrings of real tokens, lengths 2-6, drawn
with a fixed seed; batches of 1, 16 and 256.

Device: per batch size, `--warmup` calls, then `--reps` timed calls with option "infix_timing" off (the call as a server pays for it) and `--reps` with it on (a stream
sync behind every phase; the phase counters infix_scan_us / infix_mark_us / infix_expand_us / infix_rank_us). Median and min-max over the repetitions.

Host: Index::search_infix + the head of do_infix_search (src/index.cpp:3295-3340, 6184-6185) restated in C++ inside this tool and compiled with g++ -O2: per
pattern, FOUR threads walk a quarter of the vocabulary each with std::string::find (first occurrence, the two limits), the posting ids of the matching tokens are
appended to one array (posting_t::merge), then std::sort + std::unique. Ranking is not part of the host figure (it is the wildcard ranking on both sides).
--host-only runs that part alone (no GPU needed; the corpus is then built on the CPU, which is slow at 10M documents)."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_SRC = r"""
#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
extern "C" uint64_t host_infix(const uint8_t* bytes, const uint64_t* ptr, uint32_t n_tokens, const uint64_t* ids_ptr, const uint32_t* ids,
                               const uint8_t* pat_bytes, const uint64_t* pat_ptr, uint32_t n_patterns, uint32_t max_prefix, uint32_t max_suffix, uint32_t n_threads,
                               uint64_t* n_ids_out) {
    static std::vector<std::string> tokens;                 // the infix set of the field: built once per vocabulary, like the server's
    static const uint8_t* built_for = nullptr;
    if (built_for != bytes || tokens.size() != n_tokens) {
        tokens.clear();
        for (uint32_t t = 0; t < n_tokens; t++) tokens.emplace_back((const char*)bytes + ptr[t], (size_t)(ptr[t + 1] - ptr[t]));
        built_for = bytes;
    }
    uint64_t total = 0;
    for (uint32_t p = 0; p < n_patterns; p++) {
        const std::string pattern((const char*)pat_bytes + pat_ptr[p], (size_t)(pat_ptr[p + 1] - pat_ptr[p]));
        std::vector<std::vector<uint32_t>> matched(n_threads);
        std::vector<std::thread> th;
        for (uint32_t k = 0; k < n_threads; k++)
            th.emplace_back([&, k] {
                const uint32_t a = (uint32_t)((uint64_t)n_tokens * k / n_threads), b = (uint32_t)((uint64_t)n_tokens * (k + 1) / n_threads);
                for (uint32_t t = a; t < b; t++) {
                    const size_t pos = tokens[t].find(pattern);
                    if (pos != std::string::npos && pos <= max_prefix && tokens[t].size() - (pos + pattern.size()) <= max_suffix) matched[k].push_back(t);
                }
            });
        for (auto& x : th) x.join();
        std::vector<uint32_t> out;
        for (auto& m : matched) for (uint32_t t : m) out.insert(out.end(), ids + ids_ptr[t], ids + ids_ptr[t + 1]);
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
        if (n_ids_out) n_ids_out[p] = out.size();
        total += out.size();
    }
    return total;
}
"""


def synth_vocabulary(vocab, seed=41):
    """term id t (1-based) -> a word of 5-12 letters; unique (the id's base-26 digits are its tail)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 8, size=vocab)          # 0-7 random letters, then five base-26 digits of the id
    toks = []
    for t in range(vocab):
        head = bytes((rng.integers(0, 26, size=int(lens[t])) + 97).astype(np.uint8).tolist())
        x, tail = t, b""
        for _ in range(5):
            tail += bytes([97 + x % 26])
            x //= 26
        toks.append(head + tail)
    return toks


def draw_patterns(toks, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        t = toks[int(rng.integers(0, len(toks)))]
        ln = int(min(len(t), rng.integers(2, 7)))
        a = int(rng.integers(0, len(t) - ln + 1))
        out.append(t[a:a + ln])
    return out


def spread(xs):
    return "median %.3f ms (min %.3f, max %.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--vocab-scale", type=int, default=1)
    ap.add_argument("--tokens-per-doc", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--host-threads", type=int, default=4)
    ap.add_argument("--host-warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=3)     # (a batch of 256 patterns takes the host minutes at 10M documents)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from typesense_amd import synth
    vocab = a.vocab * a.vocab_scale
    t0 = time.time()
    csr = synth.zipf_corpus_csr(a.docs, vocab, a.tokens_per_doc, seed=1, device="cpu" if a.host_only else None)
    toks = synth_vocabulary(vocab)
    say("corpus: %d documents, V = %d terms, %d tokens/doc, %d postings; vocabulary %d bytes; built in %.1f s" %
        (a.docs, vocab, a.tokens_per_doc, csr["n_postings"], sum(len(t) for t in toks), time.time() - t0))
    say("machine: %d CPUs visible (os.cpu_count), host restatement on %d threads" % (os.cpu_count(), a.host_threads))
    arena = np.frombuffer(b"".join(toks), np.uint8)
    ptr = np.zeros(vocab + 1, np.uint64)
    ptr[1:] = np.cumsum([len(t) for t in toks])
    batches = [int(x) for x in a.batches.split(",")]
    pats = {b: draw_patterns(toks, b, 100 + b) for b in batches}

    # ---- host restatement
    tmp = tempfile.mkdtemp(prefix="exp_infix_")
    src, so = os.path.join(tmp, "host_infix.cpp"), os.path.join(tmp, "libhost_infix.so")
    open(src, "w").write(HOST_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src, "-lpthread"])
    HL = C.CDLL(so)
    HL.host_infix.restype = C.c_uint64
    HL.host_infix.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    host_ids, host_ms = {}, {}
    for b in batches:
        pb = np.frombuffer(b"".join(pats[b]), np.uint8)
        pp = np.zeros(b + 1, np.uint64)
        pp[1:] = np.cumsum([len(p) for p in pats[b]])
        n_ids = np.zeros(b, np.uint64)
        ts = []
        for r in range(a.host_warmup + a.host_reps):
            t1 = time.perf_counter()
            HL.host_infix(arena.ctypes.data, ptr.ctypes.data, vocab, csr["ids_ptr"].ctypes.data, csr["ids"].ctypes.data, pb.ctypes.data, pp.ctypes.data, b, 32767, 32767,
                          a.host_threads, n_ids.ctypes.data)
            if r >= a.host_warmup:
                ts.append((time.perf_counter() - t1) * 1e3)
        host_ids[b] = n_ids.copy()
        say("host  batch %4d: find + merge + sort + unique  %s; %.3f ms per pattern; union ids per pattern: median %d, max %d" %
            (b, spread(ts), statistics.median(ts) / b, int(np.median(n_ids)), int(n_ids.max())))
        host_ms[b] = statistics.median(ts)
    if a.host_only:
        say("device: NOT RUN (--host-only)")
    else:
        import typesense_amd as T
        from typesense_amd import _lib as B
        g = T.GpuIndex(0, a.lib)
        g.field_create(0, False)
        g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
        g.column_set(0, synth.points_column(a.docs))
        g.set_num_docs(a.docs)
        g.infix_enable(0)
        g.infix_tokens_load(0, csr["term_ids"], toks)
        g.commit()
        sort = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
        names = ("infix_scan_us", "infix_mark_us", "infix_expand_us", "infix_rank_us")
        for b in batches:
            qs = [T.InfixQuery(0, p, sort=sort, topster_size=250) for p in pats[b]]
            res = {}
            for timing in (0, 1):
                g.set_option("infix_timing", timing)
                ts, ph = [], {n: [] for n in names}
                for r in range(a.warmup + a.reps):
                    c0 = [g.counter(n) for n in names]
                    t1 = time.perf_counter()
                    hits, n_tok, n_ids, _ = g.infix_search_batch(qs, 250, want_ids=False)
                    dt = (time.perf_counter() - t1) * 1e3
                    if r >= a.warmup:
                        ts.append(dt)
                        for n, c in zip(names, c0):
                            ph[n].append((g.counter(n) - c) / 1e3)
                assert (hits.status == 0).all() and np.array_equal(n_ids, host_ids[b]), "device union sizes differ from the host restatement"
                res[timing] = (ts, ph)
            say("device batch %4d: whole call (ids ranked, top 250 to the host)  %s; %.3f ms per pattern; host restatement / device = %.1fx (the host figure has no ranking)" %
                (b, spread(res[0][0]), statistics.median(res[0][0]) / b, host_ms[b] / statistics.median(res[0][0])))
            say("device batch %4d: with a sync behind every phase           %s" % (b, spread(res[1][0])))
            for n, label in zip(names, ("scan (kernel + match lists to the host + handle lookup)", "union mark", "exclusion / filter / count / expand", "ranking (wildcard kernels + delivery)")):
                say("        %-58s %s" % (label, spread(res[1][1][n])))
            n_slots = vocab
            scan_ms = statistics.median(res[1][1]["infix_scan_us"])
            say("        scan reads %.2f MB of arena + slot arrays once per batch: %.1f GB/s over the scan step as timed (kernel, two syncs, D2H of the match lists, host lookup)" %
                ((arena.size + 16.0 * n_slots) / 1e6, (arena.size + 16.0 * n_slots) / 1e6 / max(scan_ms, 1e-6)))
        g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
