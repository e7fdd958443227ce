#!/usr/bin/env python3
"""
tools/bench_colbert_mxfp4.py -- the MXFP4 format of the multi-vector store beside the bf16 and the fp8 one, on
bench_colbert_fp8.py's set: --passages passages of 60-180 stored vectors at --dim (100 k x 1024-d), unit vectors, 50
candidates per query, 1 / 64 / 1024 queries of 8-24 vectors.  One MI355X, ONE process; the three stores hold the same vectors
(the quantised ones made from them on the device as they are appended), and every time alternates between the three formats,
step by step and in rotating order, between HIP events around the call (medians of --steps after a warm-up of all three).

    store_bytes      device bytes of the vectors of the three stores (2 x dim; dim + 4; dim / 2 + dim / 32 per stored vector)
    cells            hipmaxsim_dev per query count: maxsim_ms of every format, the bytes of document reads per second
                     (hipmaxsim_info's vectors x the bytes of a stored vector), the time ratios as measured; quality of mxfp4
                     against the bf16 and the fp8 store on this SYNTHETIC set: the mean top-10 overlap and the largest |score
                     difference| over all pairs
    search           hipmaxsim_search_scoped_dev, 64 queries that share one scope of 1000 documents, and 8 queries over the
                     whole store: search_ms per format, document bytes per second (hipmaxsim_search_info's vectors), the
                     top-10 overlap of mxfp4 with bf16 and fp8
    to_mxfp4         hipmv_to_mxfp4 of the whole bf16 store, and that its bytes are the appended MXFP4 store's

No speed is promised: the byte ratios are arithmetic, the times are what the run gives.  Retrieval quality on real BGE-M3
vectors CANNOT be measured here: there are no weights.  The quality figures are those of random unit vectors, which have no
structure a model's vectors have; they bound nothing but this set.

    python tools/bench_colbert_mxfp4.py [--passages 100000] [--dim 1024] [--steps 5] [--out profiles/colbert_mxfp4_100k.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "intool-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEPTH, LD_MIN, LD_MAX, LQ_MIN, LQ_MAX, BLOCK, TOP = 50, 60, 180, 8, 24, 2048, 10
FMTS = ("bf16", "fp8", "mxfp4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_colbert_mxfp4.py measures on the GPU: none is visible")
    from hiprag import MultiVectorStore, maxsim_device, maxsim_search_device
    dev = torch.device("cuda", 0)
    n, dim = args.passages, args.dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev).manual_seed(5)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    vec_bytes = {"bf16": 2 * dim, "fp8": dim + 4, "mxfp4": dim // 2 + dim // 32}

    def med(v):
        return round(float(np.median(v)), 4)

    def once(fn):
        ev[0].record()
        r = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), r

    def order(step):
        return FMTS[step % 3:] + FMTS[:step % 3]

    def overlap(a, b):
        return round(float(np.mean([len(set(x[x >= 0]) & set(y[y >= 0])) / TOP for x, y in zip(a, b)])), 4)

    # ---- the three stores from the same blocks, in rotating order ---------------------------------------------------------
    doc_len = rng.integers(LD_MIN, LD_MAX + 1, size=n).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(doc_len)
    stores = {f: MultiVectorStore(dim, max_doc_vectors=511, format=f) for f in FMTS}
    append_s = {f: 0.0 for f in FMTS}
    for b, lo in enumerate(range(0, n, BLOCK)):
        hi = min(n, lo + BLOCK)
        block = torch.randn((hi - lo, LD_MAX, dim), generator=g, device=dev)
        block = (block / block.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        torch.cuda.synchronize()
        for f in order(b):
            t0 = time.perf_counter()
            stores[f].append_device(block, doc_len[lo:hi].astype(np.int32))      # synchronous
            append_s[f] += time.perf_counter() - t0
        del block
    total = int(off[-1])
    for f in FMTS:
        assert stores[f].sizes()[:2] == (n, total) and stores[f].format_info()[:2] == (f, vec_bytes[f])
    assert stores["fp8"].format_info()[2] == 0 and stores["mxfp4"].format_info()[2] == 0      # unit vectors: the guard is no path
    res = {"passages": n, "dim": dim, "stored_vectors": total, "depth": DEPTH, "steps": args.steps,
           "store_bytes": {f: {"vectors": total * vec_bytes[f], "offsets": 8 * (n + 1), "gb": round(total * vec_bytes[f] / 1e9, 2)} for f in FMTS},
           "append": {f: {"seconds": round(append_s[f], 3), "vectors_per_s": round(total / append_s[f], 1)} for f in FMTS},
           "cells": [], "search": [],
           "note": "synthetic unit vectors; retrieval quality on real BGE-M3 vectors cannot be measured here: there are no weights"}
    res["store_bytes"]["mxfp4_over_bf16"] = round(vec_bytes["mxfp4"] / vec_bytes["bf16"], 4)
    res["store_bytes"]["mxfp4_over_fp8"] = round(vec_bytes["mxfp4"] / vec_bytes["fp8"], 4)

    def queries(nq):
        q_len = rng.integers(LQ_MIN, LQ_MAX + 1, size=nq).astype(np.int32)
        q = torch.randn((nq, LQ_MAX, dim), generator=g, device=dev)
        q = (q / q.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        return q, torch.from_numpy(q_len).to(dev)

    # ---- hipmaxsim_dev: the formats alternate step by step --------------------------------------------------------------------
    for nq in args.queries:
        q, qc = queries(nq)
        cand = rng.integers(0, n, size=(nq, DEPTH)).astype(np.int64)
        cand_dev = torch.from_numpy(cand).to(dev)
        reads = int(doc_len[cand].sum())                                       # every query has at most 32 vectors: one tile
        times, outs = {f: [] for f in FMTS}, {}
        for step in range(3 + args.steps):
            for f in order(step):
                ms, outs[f] = once(lambda: maxsim_device(stores[f], q, qc, cand_dev, TOP))
                if step >= 3:
                    times[f].append(ms)
        for f in FMTS:
            assert stores[f].maxsim_info() == (nq * DEPTH, 0, reads, 0)
        ids = {f: outs[f][1].cpu().numpy() for f in FMTS}
        cell = {"queries": nq, "pairs": nq * DEPTH, "vectors_read": reads,
                "top10_overlap": {"mxfp4_bf16": overlap(ids["mxfp4"], ids["bf16"]), "mxfp4_fp8": overlap(ids["mxfp4"], ids["fp8"]),
                                  "fp8_bf16": overlap(ids["fp8"], ids["bf16"])},
                "max_abs_score_deviation": {"mxfp4_bf16": float((outs["mxfp4"][3] - outs["bf16"][3]).abs().max()),
                                            "mxfp4_fp8": float((outs["mxfp4"][3] - outs["fp8"][3]).abs().max()),
                                            "fp8_bf16": float((outs["fp8"][3] - outs["bf16"][3]).abs().max())},
                "series_ms": {f: [round(v, 4) for v in times[f]] for f in FMTS}}
        for f in FMTS:
            ms = med(times[f])
            cell[f] = {"maxsim_ms": ms, "bytes_read": reads * vec_bytes[f],
                       "read_tbps": round(reads * vec_bytes[f] / (ms * 1e-3) / 1e12, 3), "queries_per_s": round(nq / (ms * 1e-3), 1)}
        cell["mxfp4_over_bf16"] = round(cell["mxfp4"]["maxsim_ms"] / cell["bf16"]["maxsim_ms"], 3)
        cell["mxfp4_over_fp8"] = round(cell["mxfp4"]["maxsim_ms"] / cell["fp8"]["maxsim_ms"], 3)
        res["cells"].append(cell)

    # ---- hipmaxsim_search_scoped_dev: a scope of 1000 documents shared by 64 queries, and the whole store -----------------------
    lo = n // 3
    for case, nq, scope in (("scope_1000", 64, [(lo, min(n, lo + 1000))]), ("whole_store", 8, [(0, n)])):
        q, qc = queries(nq)
        times, outs, info = {f: [] for f in FMTS}, {}, {}
        for step in range(3 + args.steps):
            for f in order(step):
                ms, outs[f] = once(lambda: maxsim_search_device(stores[f], q, qc, [scope], None, TOP))
                if step >= 3:
                    times[f].append(ms)
        for f in FMTS:
            info[f] = stores[f].search_info()
        assert info["bf16"]["doc_vectors_read"] == info["fp8"]["doc_vectors_read"] == info["mxfp4"]["doc_vectors_read"]
        ids = {f: outs[f][1].cpu().numpy() for f in FMTS}
        sc = {f: outs[f][0] for f in FMTS}
        cell = {"case": case, "queries": nq, "scope_documents": scope[0][1] - scope[0][0], "doc_vectors_read": info["bf16"]["doc_vectors_read"],
                "work_items": info["bf16"]["work_items"],
                "top10_overlap": {"mxfp4_bf16": overlap(ids["mxfp4"], ids["bf16"]), "mxfp4_fp8": overlap(ids["mxfp4"], ids["fp8"])},
                "max_abs_top_score_deviation": {"mxfp4_bf16": float((sc["mxfp4"] - sc["bf16"]).abs().max()),
                                                "mxfp4_fp8": float((sc["mxfp4"] - sc["fp8"]).abs().max())},
                "series_ms": {f: [round(v, 4) for v in times[f]] for f in FMTS}}
        for f in FMTS:
            ms = med(times[f])
            cell[f] = {"search_ms": ms, "doc_tbps": round(info[f]["doc_vectors_read"] * vec_bytes[f] / (ms * 1e-3) / 1e12, 3)}
        cell["mxfp4_over_bf16"] = round(cell["mxfp4"]["search_ms"] / cell["bf16"]["search_ms"], 3)
        cell["mxfp4_over_fp8"] = round(cell["mxfp4"]["search_ms"] / cell["fp8"]["search_ms"], 3)
        res["search"].append(cell)

    # ---- conversion of the whole bf16 store ----------------------------------------------------------------------------------
    q, qc = queries(8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    conv = stores["bf16"].to_mxfp4()
    t = time.perf_counter() - t0
    probe = torch.from_numpy(rng.integers(0, n, size=(8, DEPTH)).astype(np.int64)).to(dev)      # the same bytes, seen through MaxSim
    a, b = (maxsim_device(s, q, qc, probe, TOP) for s in (conv, stores["mxfp4"]))
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    if total * vec_bytes["mxfp4"] <= 1 << 30:                                 # small runs: the bytes themselves
        same = same and all(x.tobytes() == y.tobytes() for x, y in zip(conv.export_mxfp4(), stores["mxfp4"].export_mxfp4()))
    res["to_mxfp4"] = {"ms": round(t * 1e3, 2), "vectors_per_s": round(total / t, 1), "read_gb_per_s": round(total * dim * 2 / 1e9 / t, 2),
                       "equals_the_appended_mxfp4_store": bool(same)}
    conv.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
