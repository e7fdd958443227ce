#!/usr/bin/env python3
"""
tools/bench_colbert_fp8.py -- the fp8 format of the multi-vector store beside the bf16 one, on bench_colbert.py's set:
--passages passages of 60-180 stored vectors at --dim (100 k x 1024-d), unit vectors, 50 candidates per query, 1 / 64 / 1024
queries of 8-24 vectors.  One MI355X, ONE process; both stores hold the same vectors (the fp8 one quantised from them on the
device as they are appended), and every MaxSim time alternates between the two formats, step by step, between HIP events
around the call (medians of --steps after a warm-up of both).

    store_bytes      device bytes of the vectors of both stores (2 x dim, and dim + 4, per stored vector) and the offsets
    cells            per query count: maxsim_ms of both formats, the bytes of document reads per second (hipmaxsim_info's
                     vectors x the bytes of a stored vector), fp8_over_bf16 = the time ratio as measured;
                     quality against the bf16 store on this SYNTHETIC set: the mean top-10 overlap and the largest
                     |score difference| over all pairs
    append           documents and vectors per second through hipmv_append_dev, both formats (the same blocks, alternating)
    to_fp8           hipmv_to_fp8 of the whole bf16 store, and that its bytes are the appended fp8 store's
    remove           a removal at the front (every vector behind it moves), both formats

Retrieval quality on real BGE-M3 vectors CANNOT be measured here: there are no weights.  The quality figures are those of
random unit vectors, which have no structure a model's vectors have; they bound nothing but this set.

    python tools/bench_colbert_fp8.py [--passages 100000] [--dim 1024] [--steps 5] [--out profiles/colbert_fp8_100k.json]
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
        raise SystemExit("bench_colbert_fp8.py measures on the GPU: none is visible")
    from hiprag import MultiVectorStore, maxsim_device
    dev = torch.device("cuda", 0)
    n, dim = args.passages, args.dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev).manual_seed(5)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fmts = ("bf16", "fp8")
    vec_bytes = {"bf16": 2 * dim, "fp8": dim + 4}

    def med(v):
        return round(float(np.median(v)), 4)

    def once(fn):
        ev[0].record()
        r = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), r

    # ---- both stores from the same blocks, alternating --------------------------------------------------------------------
    doc_len = rng.integers(LD_MIN, LD_MAX + 1, size=n).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(doc_len)
    stores = {f: MultiVectorStore(dim, max_doc_vectors=511, format=f) for f in fmts}
    append_s = {f: 0.0 for f in fmts}
    for b, lo in enumerate(range(0, n, BLOCK)):
        hi = min(n, lo + BLOCK)
        block = torch.randn((hi - lo, LD_MAX, dim), generator=g, device=dev)
        block = (block / block.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        torch.cuda.synchronize()
        for f in (fmts if b % 2 == 0 else fmts[::-1]):
            t0 = time.perf_counter()
            stores[f].append_device(block, doc_len[lo:hi].astype(np.int32))      # synchronous
            append_s[f] += time.perf_counter() - t0
        del block
    total = int(off[-1])
    for f in fmts:
        assert stores[f].sizes()[:2] == (n, total) and stores[f].format_info()[:2] == (f, vec_bytes[f])
    assert stores["fp8"].format_info()[2] == 0                                # unit vectors: the domain guard is no path
    res = {"passages": n, "dim": dim, "stored_vectors": total, "depth": DEPTH, "steps": args.steps,
           "store_bytes": {f: {"vectors": total * vec_bytes[f], "offsets": 8 * (n + 1), "gb": round(total * vec_bytes[f] / 1e9, 2)} for f in fmts},
           "append": {f: {"seconds": round(append_s[f], 3), "docs_per_s": round(n / append_s[f], 1),
                          "vectors_per_s": round(total / append_s[f], 1)} for f in fmts},
           "cells": [],
           "note": "synthetic unit vectors; retrieval quality on real BGE-M3 vectors cannot be measured here: there are no weights"}
    res["store_bytes"]["fp8_over_bf16"] = round(vec_bytes["fp8"] / vec_bytes["bf16"], 4)

    # ---- MaxSim: the two formats alternate step by step ---------------------------------------------------------------------
    for nq in args.queries:
        q_len = rng.integers(LQ_MIN, LQ_MAX + 1, size=nq).astype(np.int32)
        q = torch.randn((nq, LQ_MAX, dim), generator=g, device=dev)
        q = (q / q.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        qc = torch.from_numpy(q_len).to(dev)
        cand = rng.integers(0, n, size=(nq, DEPTH)).astype(np.int64)
        cand_dev = torch.from_numpy(cand).to(dev)
        reads = int(doc_len[cand].sum())                                       # every query has at most 32 vectors: one tile
        times, outs = {f: [] for f in fmts}, {}
        for step in range(2 + args.steps):
            for f in (fmts if step % 2 == 0 else fmts[::-1]):
                ms, outs[f] = once(lambda: maxsim_device(stores[f], q, qc, cand_dev, TOP))
                if step >= 2:
                    times[f].append(ms)
        for f in fmts:
            assert stores[f].maxsim_info() == (nq * DEPTH, 0, reads, 0)
        ids = {f: outs[f][1].cpu().numpy() for f in fmts}
        overlap = float(np.mean([len(set(ids["bf16"][i]) & set(ids["fp8"][i])) / TOP for i in range(nq)]))
        dev_max = float((outs["fp8"][3] - outs["bf16"][3]).abs().max())
        cell = {"queries": nq, "pairs": nq * DEPTH, "vectors_read": reads, "top10_overlap": round(overlap, 4),
                "max_abs_score_deviation": dev_max, "series_ms": {f: [round(v, 4) for v in times[f]] for f in fmts}}
        for f in fmts:
            ms = med(times[f])
            cell[f] = {"maxsim_ms": ms, "bytes_read": reads * vec_bytes[f],
                       "read_tbps": round(reads * vec_bytes[f] / (ms * 1e-3) / 1e12, 3), "queries_per_s": round(nq / (ms * 1e-3), 1)}
        cell["fp8_over_bf16"] = round(cell["fp8"]["maxsim_ms"] / cell["bf16"]["maxsim_ms"], 3)
        res["cells"].append(cell)

    # ---- conversion of the whole bf16 store ----------------------------------------------------------------------------------
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    conv = stores["bf16"].to_fp8()
    t = time.perf_counter() - t0
    probe = torch.from_numpy(rng.integers(0, n, size=(8, DEPTH)).astype(np.int64)).to(dev)      # the same bytes, seen through MaxSim
    a, b = (maxsim_device(s, q[:8], qc[:8], probe, TOP) for s in (conv, stores["fp8"]))
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    if total * (dim + 4) <= 1 << 30:                                          # small runs: the bytes themselves
        same = same and all(x.tobytes() == y.tobytes() for x, y in zip(conv.export_fp8(), stores["fp8"].export_fp8()))
    res["to_fp8"] = {"ms": round(t * 1e3, 2), "vectors_per_s": round(total / t, 1), "read_gb_per_s": round(total * dim * 2 / 1e9 / t, 2),
                     "equals_the_appended_fp8_store": bool(same)}
    conv.close()

    # ---- a removal at the front: every vector behind it moves -----------------------------------------------------------------
    gone = min(1000, n // 2)
    moved = int(off[-1] - off[gone])
    res["remove"] = {"removed_docs": gone, "moved_vectors": moved}
    for f in fmts:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stores[f].remove_ranges([(0, gone)])
        rm = time.perf_counter() - t0
        assert stores[f].sizes()[:2] == (n - gone, moved)
        res["remove"][f] = {"ms": round(rm * 1e3, 2), "moved_gb_per_s": round(moved * vec_bytes[f] / 1e9 / rm, 2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
