#!/usr/bin/env python3
"""
tools/bench_colbert_search.py -- late-interaction SEARCH (hipmaxsim_search_scoped_dev: the exact MaxSim top k over every
document of a scope) beside the only route there was before it: hipmaxsim_dev over the scope's ids in candidate chunks of 256
with a torch merge of the chunks' lists.  One MI355X; every time is taken between HIP events around the whole route (medians
of --steps after a warm-up), the two routes alternating in one process.

Workload: tools/bench_colbert.py's set -- --passages passages of 60-180 stored vectors at --dim (100 k x 1024-d: about 25 GB
in bf16), unit vectors, as a bf16 and as an fp8 store.  Scopes of 0.1 %, 1 %, 10 % and 100 % of the documents (one range, off
the slice boundaries); 1 / 8 / 64 queries of 8-32 vectors sharing the scope, and 64 queries over 64 different 0.1 % scopes.
Per cell:
    search_ms        hipmaxsim_search_scoped_dev, merge included
    chunked_ms       hipmaxsim_dev per chunk of 256 ids (k = min(top k, ids)), torch.cat + torch.topk
    doc_vectors_read the search's counter (hipmaxsim_search_info): passes x stored vectors of the in-scope documents, summed
                     over work items; doc_tbps = their bytes per second of search_ms
The top-k SCORES of the two routes must be equal bit for bit (the ids too wherever the scores are distinct).

    python tools/bench_colbert_search.py [--passages 100000] [--dim 1024] [--steps 5] [--out profiles/colbert_search_100k.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "intool-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LD_MIN, LD_MAX, LQ_MIN, LQ_MAX, BLOCK, TOP_K = 60, 180, 8, 32, 2048, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--formats", nargs="+", default=["bf16", "fp8"])
    ap.add_argument("--scopes", type=float, nargs="+", default=[0.001, 0.01, 0.1, 1.0])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_colbert_search.py measures on the GPU: none is visible")
    from hiprag import MultiVectorStore, maxsim_device, maxsim_search_device
    dev = torch.device("cuda", 0)
    n, dim = args.passages, args.dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev).manual_seed(5)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, steps=args.steps, warm=1):
        out = []
        for i in range(warm + steps):
            ev[0].record()
            r = fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warm:
                out.append(ev[0].elapsed_time(ev[1]))
        return round(float(np.median(out)), 4), r

    doc_len = rng.integers(LD_MIN, LD_MAX + 1, size=n).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(doc_len)
    stores = {f: MultiVectorStore(dim, max_doc_vectors=511, format=f) for f in args.formats}
    for lo in range(0, n, BLOCK):
        hi = min(n, lo + BLOCK)
        block = torch.randn((hi - lo, LD_MAX, dim), generator=g, device=dev)
        block = (block / block.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        for s in stores.values():
            s.append_device(block, doc_len[lo:hi].astype(np.int32))
        del block
    info0 = next(iter(stores.values())).search_info()
    res = {"passages": n, "dim": dim, "stored_vectors": int(off[-1]), "top_k": TOP_K, "steps": args.steps,
           "pass_rows": info0["pass_rows"], "group_queries": info0["group_queries"], "slice_docs": info0["slice_docs"], "cells": []}

    nq_max = max(max(args.queries), 64)
    q_len = rng.integers(LQ_MIN, LQ_MAX + 1, size=nq_max).astype(np.int32)
    q = torch.randn((nq_max, LQ_MAX, dim), generator=g, device=dev)
    q = (q / q.norm(dim=2, keepdim=True)).to(torch.bfloat16)
    qc = torch.from_numpy(q_len).to(dev)

    def scope_at(frac, which=0):
        m = max(1, int(round(n * frac)))
        lo = min(n - m, 3 + which * (m + 5)) if m < n else 0               # off the slice boundaries, disjoint for different `which`
        return [(int(lo), int(lo + m))]

    def chunked(store, qv, qcv, scopes, soq):
        """the parent's route: every query's scope ids in chunks of 256 through hipmaxsim_dev, the lists merged with torch"""
        nq = qv.shape[0]
        ids_of = [np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in scopes[s]]) for s in soq]
        width = max(len(v) for v in ids_of)
        cand = np.full((nq, (width + 255) // 256 * 256), -1, dtype=np.int64)
        for i, v in enumerate(ids_of):
            cand[i, :len(v)] = v
        cand = torch.from_numpy(cand).to(dev)

        def run():
            ss, ii = [], []
            for c in range(0, cand.shape[1], 256):
                s_, i_, _p, _ = maxsim_device(store, qv, qcv, cand[:, c:c + 256].contiguous(), min(TOP_K, 256), want_pairs=False)
                ss.append(s_)
                ii.append(i_)
            ss, ii = torch.cat(ss, dim=1), torch.cat(ii, dim=1)
            top, pos = torch.topk(ss, TOP_K, dim=1)
            return top, torch.gather(ii, 1, pos)
        return run

    def cell(fmt, store, name, frac, nq, scopes, soq):
        qv, qcv = q[:nq].contiguous(), qc[:nq].contiguous()
        route = chunked(store, qv, qcv, scopes, soq)
        s_ms, (s_scores, s_ids) = timed(lambda: maxsim_search_device(store, qv, qcv, scopes, soq, TOP_K))
        info = store.search_info()
        c_ms, (c_scores, c_ids) = timed(route)
        s_ms2, _ = timed(lambda: maxsim_search_device(store, qv, qcv, scopes, soq, TOP_K))        # alternating: once more after the other route
        assert torch.equal(s_scores.view(torch.int32), c_scores.view(torch.int32)), "the two routes give different top-k scores"
        distinct = (s_scores[:, 1:] != s_scores[:, :-1]).all()
        assert not bool(distinct) or torch.equal(s_ids, c_ids)
        in_scope = int(sum(hi - lo for s in set(soq) for lo, hi in scopes[s]))
        ms = min(s_ms, s_ms2)
        res["cells"].append({"format": fmt, "case": name, "scope_fraction": frac, "scope_documents": in_scope, "queries": nq,
                             "search_ms": s_ms, "search_ms_again": s_ms2, "chunked_ms": c_ms, "chunked_over_search": round(c_ms / ms, 2),
                             "doc_vectors_read": info["doc_vectors_read"], "work_items": info["work_items"],
                             "doc_tbps": round(info["doc_vectors_read"] * (dim * 2 if fmt == "bf16" else dim + 4) / (ms * 1e-3) / 1e12, 3)})
        print(json.dumps(res["cells"][-1]), flush=True)

    for fmt, store in stores.items():
        for frac in args.scopes:
            for nq in args.queries:
                cell(fmt, store, "shared_scope", frac, nq, [scope_at(frac)], [0] * nq)
        cell(fmt, store, "64_scopes", 0.001, 64, [scope_at(0.001, w) for w in range(64)], list(range(64)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
