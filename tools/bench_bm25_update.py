#!/usr/bin/env python3
"""
tools/bench_bm25_update.py -- updatable BM25 postings (hipbm25_append / _remove_ranges / _reweigh) on one synthetic
collection of 1M documents, one GPU process.  One 1 000-chunk document is appended at the end and one is removed from the
middle; timed, wall ms of the synchronous calls, median over --steps:
    append_ms + reweigh_ms        the batch CSR of the 1 000 chunks is built on the host outside the timer (it is the
                                  ingest's tokenisation of the new document, paid either way); numpy's idf inside it
    remove_ms + reweigh_ms
    rebuild_ms                    what the same change cost before: HipBM25(build_postings(...)) over the token stream of the
                                  WHOLE collection (sort of every (term, doc) pair on the host, impacts, upload); the
                                  tokenisation of every chunk table, which the overlay's rebuild also pays, is NOT in it
The reweigh kernel's algorithmic bytes = postings x 12 (doc id and tf read, impact written) + 4 per document length read
once; its GB/s from a HIP-event timing of hipbm25_reweigh alone stands beside hiprag_probe_read_gbps.

    python tools/bench_bm25_update.py [--docs 1000000] [--terms 262144] [--steps 5] [--out profiles/bm25_update_1m.json]

The collection comes from hiprag and numpy alone (Zipf(1) over --terms, 64..319 tokens per document).  One JSON line on
stdout and in --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "intool-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DOC_CHUNKS = 1000


def token_stream(n_docs, n_terms, seed):
    i = np.arange(n_docs, dtype=np.uint64)
    doc_len = (64 + (i * np.uint64(2654435761)) % np.uint64(256)).astype(np.int64)
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(1.0 / np.arange(1, n_terms + 1, dtype=np.float64))
    cdf /= cdf[-1]
    term = np.minimum(np.searchsorted(cdf, rng.random(int(doc_len.sum())), side="left"), n_terms - 1)
    return np.repeat(np.arange(n_docs, dtype=np.int64), doc_len), term, doc_len


def median_ms(f, steps):
    out = []
    for _ in range(steps):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from hiprag import HipBM25, HipBM25Updatable, _native as nat, batch_csr, build_postings
    n, V = args.docs, args.terms
    doc, term, doc_len = token_stream(n, V, 777)
    bdoc, bterm, bdl = token_stream(DOC_CHUNKS, V, 778)
    batch = batch_csr(bdoc, bterm, DOC_CHUNKS, V, bdl)

    t = time.perf_counter()
    upd = HipBM25Updatable.from_tokens(doc, term, n, V, doc_len)
    create_ms = (time.perf_counter() - t) * 1e3
    postings = upd.sizes()["postings"]
    res = {"docs": n, "terms": V, "postings": postings, "doc_chunks": DOC_CHUNKS, "steps": args.steps, "create_tf_ms": round(create_ms, 3)}

    # append one document at the end, remove it again: the handle is the same collection before every step
    times = {"append_ms": [], "append_reweigh_ms": [], "remove_ms": [], "remove_reweigh_ms": [], "remove_middle_ms": []}
    for _ in range(args.steps):
        t0 = time.perf_counter()
        upd.append_postings(DOC_CHUNKS, V, *batch)
        t1 = time.perf_counter()
        upd.commit()
        t2 = time.perf_counter()
        upd.remove_ranges([(n, n + DOC_CHUNKS)])
        t3 = time.perf_counter()
        upd.commit()
        t4 = time.perf_counter()
        times["append_ms"].append((t1 - t0) * 1e3)
        times["append_reweigh_ms"].append((t2 - t1) * 1e3)
        times["remove_ms"].append((t3 - t2) * 1e3)
        times["remove_reweigh_ms"].append((t4 - t3) * 1e3)
    res["append_info"] = None
    upd.append_postings(DOC_CHUNKS, V, *batch)
    res["append_info"] = upd.update_info()
    # a document out of the middle: every list is compacted behind its first removed posting
    t0 = time.perf_counter()
    upd.remove_ranges([(n // 2, n // 2 + DOC_CHUNKS)])
    times["remove_middle_ms"].append((time.perf_counter() - t0) * 1e3)
    res["remove_middle_info"] = upd.update_info()
    upd.commit()
    for key, v in times.items():
        res[key] = round(float(np.median(v)), 3)
    res["append_plus_reweigh_ms"] = round(res["append_ms"] + res["append_reweigh_ms"], 3)
    res["remove_plus_reweigh_ms"] = round(res["remove_ms"] + res["remove_reweigh_ms"], 3)

    # the reweigh kernel alone, HIP events around hipbm25_reweigh with the idf already on the host
    idf = np.ascontiguousarray(upd.idf())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(args.steps + 1):
        ev[0].record()
        nat.call("hipbm25_reweigh", upd._h, idf.ctypes.data)
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    sz = upd.sizes()
    rw_ms = float(np.median(ms[1:]))
    rw_bytes = sz["postings"] * 12 + sz["n_docs"] * 4
    res["reweigh_call_ms"] = round(rw_ms, 3)
    res["reweigh_bytes"] = rw_bytes
    res["reweigh_gbps"] = round(rw_bytes / (rw_ms * 1e-3) / 1e9, 1)      # includes the skip tables and the idf upload
    probe = ctypes.c_double()
    nat.call("hiprag_probe_read_gbps", 0, 1 << 30, 5, ctypes.byref(probe))
    res["probe_read_gbps"] = round(probe.value, 1)
    upd.close()

    # the way there was before: the whole collection again
    def rebuild():
        HipBM25(build_postings(doc, term, n, V, doc_len)).close()
    res["rebuild_ms"] = round(median_ms(rebuild, max(1, min(args.steps, 3))), 3)
    res["rebuild_over_append"] = round(res["rebuild_ms"] / res["append_plus_reweigh_ms"], 1)
    res["rebuild_over_remove"] = round(res["rebuild_ms"] / res["remove_plus_reweigh_ms"], 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
