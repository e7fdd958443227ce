#!/usr/bin/env python3
"""Updatable lexical postings (hipbm25_append_rows_dev / _append_impacts / _remove_ranges on an impact handle) on one
synthetic collection; writes profiles/lexical_update_1m.json.

The collection has the row statistics of tools/bench_lexical.py's: --docs documents of 64 + (i * 2654435761) % 256 tokens
drawn Zipf over --terms ids; a document's lexical row is its distinct ids, ascending, each with a weight in [0.05, 2).  The
rows are made on the GPU and the base handle is built through the device path itself, a --build-batch rows at a time.

Measured, medians of --iters with HIP events around the call (the update entries are synchronous, so this is their wall time,
host planning included); between two timed appends the appended rows are removed again, untimed:
  append of 256 and 8192 rows   device path (hipbm25_append_rows_dev over CUDA rows);
                                host path (transpose_doc_weights of the batch + hipbm25_append_impacts);
                                the parent's only way: transpose_doc_weights of EVERY row + hipbm25_create (--rebuild-runs,
                                default 1 per batch size: it is minutes of host lexsort)
  removal of 1 % at the front   hipbm25_remove_ranges; every timed run removes the next 1 % (the collection shrinks by 1 % a run)
  weighted search               256 six-term queries, k = 50, on the updated handle and on a fresh hipbm25_create over its
                                export (the same structure by the defining property: recorded, not asserted)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "intool-rag_amd"))


def make_rows(N, V, seed=777):
    """(terms int32 [N, L], weights float32 [N, L], counts int32 [N]) CUDA tensors"""
    import torch
    dev = torch.device("cuda", 0)
    i = torch.arange(N, dtype=torch.int64, device=dev)
    doc_len = 64 + (i * 2654435761) % 256
    cdf = torch.cumsum(1.0 / torch.arange(1, V + 1, dtype=torch.float64, device=dev), 0)
    cdf /= cdf[-1].clone()
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    total = int(doc_len.sum().item())
    term = torch.clamp(torch.searchsorted(cdf, torch.rand(total, generator=g, device=dev, dtype=torch.float64)), max=V - 1)
    key = torch.unique(torch.repeat_interleave(i, doc_len) * V + term)          # sorted: document-major, ids ascending, distinct
    del term
    doc, term = key // V, (key % V).to(torch.int32)
    del key
    counts = torch.bincount(doc, minlength=N)
    start = torch.cumsum(counts, 0) - counts
    pos = torch.arange(doc.numel(), device=dev) - start[doc]
    L = int(counts.max().item())
    terms = torch.full((N, L), -1, dtype=torch.int32, device=dev)
    weights = torch.zeros((N, L), dtype=torch.float32, device=dev)
    terms[doc, pos] = term
    weights[doc, pos] = 0.05 + 1.95 * torch.rand(doc.numel(), generator=g, device=dev, dtype=torch.float32)
    return terms, weights, counts.to(torch.int32)


def timed(fn, iters, restore=None):
    """median and all timings (ms) of fn() between two HIP events; restore() runs untimed behind every call"""
    import torch
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
        if restore is not None:
            restore()
    return round(statistics.median(out), 3), [round(x, 3) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=262144)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--build-batch", type=int, default=65536)
    ap.add_argument("--rebuild-runs", type=int, default=1, help="runs of the parent's way per batch size (0: not measured)")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lexical_update_1m.json"))
    args = ap.parse_args()

    import torch
    from hiprag import HipBM25, LexicalIndexUpdatable, PostingsCSR, transpose_doc_weights
    from oracle import hybrid_oracle as ho
    N, V = args.docs, args.terms
    t0 = time.perf_counter()
    terms, weights, counts = make_rows(N, V)
    torch.cuda.synchronize()
    print(json.dumps({"rows_made_s": round(time.perf_counter() - t0, 1), "row_stride": int(terms.shape[1])}), flush=True)
    lex = LexicalIndexUpdatable(n_terms=V)
    t0 = time.perf_counter()
    for lo in range(0, N, args.build_batch):
        lex.append_rows(terms[lo:lo + args.build_batch], weights[lo:lo + args.build_batch], counts[lo:lo + args.build_batch])
    build_s = time.perf_counter() - t0
    sz = lex.sizes()
    result = {"device": torch.cuda.get_device_name(0), "docs": N, "terms": V, "postings": sz["postings"], "row_stride": int(terms.shape[1]),
              "mean_terms_per_row": round(sz["postings"] / N, 1), "timing": "HIP events around the synchronous call, median of --iters",
              "iters": args.iters, "base_build": {"what": f"device appends of {args.build_batch} rows onto an empty handle", "seconds": round(build_s, 2)},
              "not_measured": []}
    print(json.dumps({"base_build_s": round(build_s, 2), "postings": sz["postings"]}), flush=True)

    host_rows = None
    result["append"] = {}
    for n in (256, 8192):
        b = (terms[:n].contiguous(), weights[:n].contiguous(), counts[:n].contiguous())
        hb = tuple(t.cpu().numpy() for t in b)
        restore = lambda: lex.remove_ranges([(N, N + n)])   # noqa: E731
        dev_ms, dev_all = timed(lambda: lex.append_rows(*b), args.iters, restore)
        lex.append_rows(*b)
        info = lex.update_info()
        restore()

        def host_path():
            p = transpose_doc_weights(*hb, V)
            lex.append_postings(n, V, p.offsets, p.doc_ids, p.impacts)
        host_ms, host_all = timed(host_path, args.iters, restore)
        entry = {"device_ms": dev_ms, "device_ms_runs": dev_all, "host_ms": host_ms, "host_ms_runs": host_all,
                 "device_update_info": {k: info[k] for k in ("postings_before", "postings_after", "postings_moved", "extra_bytes", "grew")}}
        if args.rebuild_runs > 0:
            if host_rows is None:
                host_rows = tuple(t.cpu().numpy() for t in (terms, weights, counts))
            runs = []
            for _ in range(args.rebuild_runs):
                t0 = time.perf_counter()
                p = transpose_doc_weights(*(np.concatenate([a, x]) for a, x in zip(host_rows, hb)), V)
                t1 = time.perf_counter()
                fresh = HipBM25(p)
                torch.cuda.synchronize()
                runs.append({"transpose_s": round(t1 - t0, 2), "create_s": round(time.perf_counter() - t1, 2)})
                fresh.close()
                del p, fresh
            entry["rebuild_runs"] = runs
            entry["rebuild_ms"] = round(1e3 * statistics.median(r["transpose_s"] + r["create_s"] for r in runs), 1)
            entry["rebuild_timing"] = "host wall clock: it is host work"
        else:
            result["not_measured"].append(f"the parent's way (transpose every row + hipbm25_create) for a batch of {n}")
        result["append"][str(n)] = entry
        print(json.dumps({f"append_{n}": entry}), flush=True)
    del host_rows

    # weighted search on the updated handle beside a fresh handle over the same postings
    lex.append_rows(terms[:8192].contiguous(), weights[:8192].contiguous(), counts[:8192].contiguous())
    ex = lex.export()
    fresh = HipBM25(PostingsCSR(ex["n_docs"], ex["n_terms"], ex["offsets"], ex["doc_ids"], ex["impacts"]))
    qs = ho.synthetic_sparse_queries(args.nq, n_terms=V, terms_per_query=6, seed=888, min_rank=16)
    rng = np.random.default_rng(5)
    ws = [rng.uniform(0.1, 2.0, size=len(q)).astype(np.float32) for q in qs]
    for h in (lex.bm, fresh):
        h.search_weighted_device(qs, ws, args.k)
    up_ms, up_all = timed(lambda: lex.bm.search_weighted_device(qs, ws, args.k), args.iters)
    fr_ms, fr_all = timed(lambda: fresh.search_weighted_device(qs, ws, args.k), args.iters)
    same = all(torch.equal(a, b) for a, b in zip(lex.bm.search_weighted_device(qs, ws, args.k), fresh.search_weighted_device(qs, ws, args.k)))
    result["weighted_search"] = {"nq": args.nq, "k": args.k, "terms_per_query": 6, "updated_ms": up_ms, "fresh_ms": fr_ms,
                                 "updated_qps": round(args.nq / up_ms * 1e3, 1), "fresh_qps": round(args.nq / fr_ms * 1e3, 1),
                                 "updated_ms_runs": up_all, "fresh_ms_runs": fr_all, "same_bits": bool(same)}
    print(json.dumps({"weighted_search": result["weighted_search"]}), flush=True)
    fresh.close()
    del ex

    # removal of 1 % of the documents at the front
    infos = []
    one = N // 100

    def remove():
        lex.remove_ranges([(0, one)])
        infos.append(lex.update_info())
    rm_ms, rm_all = timed(remove, args.iters)
    result["remove_front_1pct"] = {"documents": one, "ms": rm_ms, "ms_runs": rm_all, "postings_moved_first_run": infos[0]["postings_moved"],
                                   "note": "every run removes the next 1 %: the collection shrinks by 1 % a run"}
    print(json.dumps({"remove_front_1pct": result["remove_front_1pct"]}), flush=True)
    lex.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
