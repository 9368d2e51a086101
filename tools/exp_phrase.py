"""Phrase search (tsgpu_phrase_search_batch) measured next to a host restatement of the reference's loop on the same machine.

Corpus: the bench's keyword collection (BASELINE config 2: Zipf(1.0) text, 32 tokens per document, V = 100 000 terms). Phrases: 2 and 3 consecutive tokens of real
documents (the corpus generator's first slab is drawn again with the same seed to read them), alternating, one phrase = one query of mode RANK over the one field;
batches of 1, 16 and 256.

Device: per batch size, `--warmup` calls, then `--reps` timed calls with option "phrase_timing" off (the whole call: intersection, adjacency, fold, expansion,
ranking, the top 250 to host memory) and `--reps` with it on (a stream sync behind every phase; counters phrase_mark_us / phrase_fold_us / phrase_rank_us).

Host: Index::do_phrase_search's per-phrase work (src/index.cpp:5955-5961) restated in C++ inside this tool and compiled with g++ -O2, on ONE thread (do_phrase_search
is not fanned out): the lists are intersected, then every intersected id is walked as posting_list_t::get_phrase_matches walks it — get_offsets into a
std::map<size_t, std::vector<std::vector<uint16_t>>> per document (src/posting_list.cpp:832-916), has_phrase_match / found_token_sequence (:1719-1789). No ranking
on the host side. The counts of matching documents must equal the device's."""
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
#include <map>
#include <vector>
typedef std::vector<std::vector<uint16_t>> TokenPositions;
static bool found_token_sequence(const TokenPositions& tp, size_t token_index, uint16_t target_pos) {
    if (token_index == tp.size()) return true;
    bool found = false;
    int prev = -1;
    for (uint16_t p : tp[token_index]) {
        if ((int)p < prev) { found = false; break; }
        if (p == target_pos) { found = true; break; }
        prev = p;
    }
    if (!found) return false;
    return found_token_sequence(tp, token_index + 1, (uint16_t)(target_pos + 1));
}
static bool has_phrase_match(const TokenPositions& tp) {
    int prev = -1;
    for (uint16_t pos : tp[0]) {
        if ((int)pos < prev) return false;
        if (found_token_sequence(tp, 1, (uint16_t)(pos + 1))) return true;
        prev = pos;
    }
    return false;
}
// terms: 0-based term indexes, phrase p = terms[ph_ptr[p] .. ph_ptr[p + 1]); the CSR of typesense_amd.synth.zipf_corpus_csr
extern "C" uint64_t host_phrases(const uint64_t* ids_ptr, const uint32_t* ids, const uint64_t* offset_index, const uint64_t* off_ptr, const uint32_t* offsets,
                                 const uint32_t* terms, const uint32_t* ph_ptr, uint32_t n_phrases, uint64_t* n_match_out, uint64_t* n_intersect_out) {
    uint64_t total = 0;
    for (uint32_t p = 0; p < n_phrases; p++) {
        const uint32_t T = ph_ptr[p + 1] - ph_ptr[p];
        const uint32_t* tm = terms + ph_ptr[p];
        std::vector<uint32_t> acc(ids + ids_ptr[tm[0]], ids + ids_ptr[tm[0] + 1]), nxt;
        for (uint32_t t = 1; t < T; t++) {                        // posting_t::intersect
            nxt.clear();
            std::set_intersection(acc.begin(), acc.end(), ids + ids_ptr[tm[t]], ids + ids_ptr[tm[t] + 1], std::back_inserter(nxt));
            acc.swap(nxt);
        }
        uint64_t n_match = 0;
        std::vector<uint64_t> cursor(T);
        for (uint32_t t = 0; t < T; t++) cursor[t] = ids_ptr[tm[t]];
        for (uint32_t id : acc) {
            std::map<size_t, TokenPositions> array_token_positions;
            for (uint32_t t = 0; t < T; t++) {                    // skip_to(id), then get_offsets
                const uint32_t* lo = std::lower_bound(ids + cursor[t], ids + ids_ptr[tm[t] + 1], id);
                cursor[t] = (uint64_t)(lo - ids);
                uint64_t start = offset_index[cursor[t]];
                const uint64_t end = cursor[t] + 1 < ids_ptr[tm[t] + 1] ? offset_index[cursor[t] + 1] : off_ptr[tm[t] + 1];
                std::vector<uint16_t> positions;
                int prev_pos = -1;
                while (start < end) {
                    const int pos = (int)offsets[start++];
                    if (pos == 0) { start++; continue; }
                    if (pos == prev_pos) {
                        if (!positions.empty()) { array_token_positions[(size_t)offsets[start]].push_back(positions); positions.clear(); }
                        start++; prev_pos = -1; continue;
                    }
                    prev_pos = pos;
                    positions.push_back((uint16_t)pos - 1);
                }
                if (!positions.empty()) array_token_positions[0].push_back(positions);
            }
            for (auto& kv : array_token_positions)
                if (kv.second.size() == T && has_phrase_match(kv.second)) { n_match++; break; }
        }
        n_match_out[p] = n_match; n_intersect_out[p] = acc.size();
        total += n_match;
    }
    return total;
}
"""


def draw_phrases(n, n_docs, vocab, tokens_per_doc, seed, dev):
    """n phrases of 2 and 3 consecutive tokens of real documents: the corpus's first slab of draws, repeated (typesense_amd/synth.py: same generator, same order)"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    ranks = torch.arange(1, vocab + 1, dtype=torch.float64, device=dev)
    w = ranks.pow(-1.0)
    cdf = torch.cumsum(w / w.sum(), 0)
    slab = min(n_docs * tokens_per_doc, 1 << 26)
    u = torch.rand(slab, generator=g, device=dev, dtype=torch.float64)
    term = torch.searchsorted(cdf, u).clamp_(max=vocab - 1).cpu().numpy()          # 0-based term index of (doc, pos) = flat index
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T = 2 + i % 2
        d = int(rng.integers(0, slab // tokens_per_doc))
        p = int(rng.integers(0, tokens_per_doc - T + 1))
        out.append([int(x) for x in term[d * tokens_per_doc + p:d * tokens_per_doc + p + T]])
    return out


def spread(xs):
    return "median %.3f ms (min %.3f, max %.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--tokens-per-doc", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--host-warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    from typesense_amd import synth
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    t0 = time.time()
    csr = synth.zipf_corpus_csr(a.docs, a.vocab, a.tokens_per_doc, seed=1, device=dev)
    say("corpus: %d documents, V = %d terms, %d tokens/doc, %d postings; built in %.1f s" % (a.docs, a.vocab, a.tokens_per_doc, csr["n_postings"], time.time() - t0))
    batches = [int(x) for x in a.batches.split(",")]
    phrases = {b: draw_phrases(b, a.docs, a.vocab, a.tokens_per_doc, 200 + b, dev) for b in batches}

    # ---- host restatement, one thread
    tmp = tempfile.mkdtemp(prefix="exp_phrase_")
    src, so = os.path.join(tmp, "host_phrase.cpp"), os.path.join(tmp, "libhost_phrase.so")
    open(src, "w").write(HOST_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    HL = C.CDLL(so)
    HL.host_phrases.restype = C.c_uint64
    HL.host_phrases.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_void_p]
    host_match, host_isect, host_ms = {}, {}, {}
    for b in batches:
        flat = np.array([t for ph in phrases[b] for t in ph], np.uint32)
        pp = np.zeros(b + 1, np.uint32)
        pp[1:] = np.cumsum([len(ph) for ph in phrases[b]])
        n_match, n_isect = np.zeros(b, np.uint64), np.zeros(b, np.uint64)
        ts = []
        for r in range(a.host_warmup + a.host_reps):
            t1 = time.perf_counter()
            HL.host_phrases(csr["ids_ptr"].ctypes.data, csr["ids"].ctypes.data, csr["offset_index"].ctypes.data, csr["off_ptr"].ctypes.data, csr["offsets"].ctypes.data,
                            flat.ctypes.data, pp.ctypes.data, b, n_match.ctypes.data, n_isect.ctypes.data)
            if r >= a.host_warmup:
                ts.append((time.perf_counter() - t1) * 1e3)
        host_match[b], host_isect[b], host_ms[b] = n_match.copy(), n_isect.copy(), statistics.median(ts)
        say("host  batch %4d: intersect + get_phrase_matches, 1 thread  %s; %.3f ms per phrase; intersected ids per phrase: median %d, max %d; matching: median %d, max %d" %
            (b, spread(ts), statistics.median(ts) / b, int(np.median(n_isect)), int(n_isect.max()), int(np.median(n_match)), int(n_match.max())))

    # ---- device
    import typesense_amd as T
    from typesense_amd import _lib as B
    g = T.GpuIndex(0, a.lib)
    g.field_create(0, False)
    g.terms_load_csr(0, csr["term_ids"], csr["ids_ptr"], csr["ids"], csr["offset_index"], csr["off_ptr"], csr["offsets"])
    g.column_set(0, synth.points_column(a.docs))
    g.set_num_docs(a.docs)
    g.commit()
    sort = ((B.SORT_TEXT_MATCH, 1, 0), (B.SORT_INT64_COLUMN, 1, 0))
    names = ("phrase_mark_us", "phrase_fold_us", "phrase_rank_us")
    for b in batches:
        qs = [T.PhraseQuery([(0, 15, [[t + 1 for t in ph]])], sort=sort, topster_size=250) for ph in phrases[b]]          # (term id = index + 1)
        res = {}
        for timing in (0, 1):
            g.set_option("phrase_timing", timing)
            ts, ph_t = [], {n: [] for n in names}
            for r in range(a.warmup + a.reps):
                c0 = [g.counter(n) for n in names]
                k0 = g.counter("phrase_records_checked")
                t1 = time.perf_counter()
                hits, n_ids, _ = g.phrase_search_batch(qs, 250, want_ids=False)
                dt = (time.perf_counter() - t1) * 1e3
                checked = g.counter("phrase_records_checked") - k0
                if r >= a.warmup:
                    ts.append(dt)
                    for n, c in zip(names, c0):
                        ph_t[n].append((g.counter(n) - c) / 1e3)
            assert (hits.status == 0).all() and np.array_equal(n_ids, host_match[b]), "device phrase counts differ from the host restatement"
            assert checked == int(host_isect[b].sum()), "hit records checked differ from the host's intersections"
            res[timing] = (ts, ph_t)
        say("device batch %4d: whole call (ids ranked, top 250 to the host)  %s; %.3f ms per phrase; host restatement / device = %.1fx (the host figure has no ranking)" %
            (b, spread(res[0][0]), statistics.median(res[0][0]) / b, host_ms[b] / statistics.median(res[0][0])))
        say("device batch %4d: with a sync behind every phase           %s" % (b, spread(res[1][0])))
        for n, label in zip(names, ("plan + find kernels + adjacency kernel", "fold / OR / exclusion / filter / expand / scores", "ranking (wildcard kernels + delivery)")):
            say("        %-58s %s" % (label, spread(res[1][1][n])))
        # what the adjacency kernel requests per record: the record itself (16 B up to 3 tokens) and per token one BlockMeta (32 B), the offset_index pair (2 x 8 B)
        # and the first offsets (8 B): the fixed sizes of load_runs_staged; a third.. occurrence of a token costs one more 8-byte fetch each (not counted)
        total_bytes = sum((16 + 56 * len(ph)) * int(n) for ph, n in zip(phrases[b], host_isect[b]))
        rec_bytes = total_bytes / max(int(host_isect[b].sum()), 1)
        mark_ms = statistics.median(res[1][1]["phrase_mark_us"])
        say("        adjacency kernel: %d records, %.0f B requested per record (mean), %.2f MB in all; over the WHOLE first phase (planning and the find kernels included) that is %.2f GB/s = %.4f of 8 TB/s" %
            (int(host_isect[b].sum()), rec_bytes, total_bytes / 1e6, total_bytes / 1e6 / max(mark_ms, 1e-6), total_bytes / 1e6 / max(mark_ms, 1e-6) / 8000.0))
    g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
