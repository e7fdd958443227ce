#!/usr/bin/env python3
"""
tools/bench_colbert_pruned.py -- the PRUNED late-interaction search (hipmaxsim_search_pruned_dev: centroid codes, candidate
generation, exact MaxSim of the candidates) beside the exact brute-force search (hipmaxsim_search_scoped_dev), the two
alternating in one process.  One MI355X; every time is taken between HIP events around the whole call (medians of --steps after
a warm-up).  The library has no per-stage entry points, so the three stages of a pruned call (table, interaction, exact) are
timed together; the cost of the exact stage alone is hipmaxsim_dev over the call's own candidates, recorded beside it.

Workload: tools/bench_colbert_search.py's set -- --passages passages of 60-180 stored vectors at --dim -- but with the token
vectors drawn from a TOPIC MIXTURE so that recall means something: --topics random unit topic vectors, a passage draws 4 of
them, each token is unit(topic + 0.5 unit noise).  A query is 8-32 token vectors of a passage of its scope plus 0.3 unit noise.
Per (ncent, scope, queries, ncand):
    pruned_ms, exact_search_ms   the two entries; exact_stage_ms: hipmaxsim_dev over the pruned call's candidates
    recall_at_10                 |pruned top 10 & exact top 10| / 10, averaged over the queries
and per ncent: train_ms (train_token_centroids), attach_ms (hipmv_attach_centroids: every stored vector coded), code bytes.

    python tools/bench_colbert_pruned.py [--passages 100000] [--dim 1024] [--steps 5] [--out profiles/colbert_pruned_100k.json]
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

LD_MIN, LD_MAX, LQ_MIN, LQ_MAX, BLOCK, TOP_K, TOPICS_PER_DOC = 60, 180, 8, 32, 2048, 10, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--topics", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--format", default="bf16")
    ap.add_argument("--ncent", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--ncand", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--scopes", type=int, nargs="+", default=[1000, 100_000])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_colbert_pruned.py measures on the GPU: none is visible")
    from hiprag import MultiVectorStore, maxsim_device, maxsim_search_device, maxsim_search_pruned_device, train_token_centroids
    dev = torch.device("cuda", 0)
    n, dim = args.passages, args.dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev).manual_seed(5)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def unit(x):
        return x / x.norm(dim=-1, keepdim=True)

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

    topics = unit(torch.randn((args.topics, dim), generator=g, device=dev))
    doc_len = rng.integers(LD_MIN, LD_MAX + 1, size=n).astype(np.int64)
    store = MultiVectorStore(dim, max_doc_vectors=511, format=args.format)
    for lo in range(0, n, BLOCK):
        hi = min(n, lo + BLOCK)
        of_doc = torch.randint(0, args.topics, (hi - lo, TOPICS_PER_DOC), generator=g, device=dev)
        pick = torch.randint(0, TOPICS_PER_DOC, (hi - lo, LD_MAX), generator=g, device=dev)
        base = topics[torch.gather(of_doc, 1, pick)]
        block = unit(base + 0.5 * unit(torch.randn(base.shape, generator=g, device=dev))).to(torch.bfloat16)
        store.append_device(block, doc_len[lo:hi].astype(np.int32))
        del block, base
    stored = store.sizes()[1]
    res = {"passages": n, "dim": dim, "format": args.format, "topics": args.topics, "stored_vectors": stored, "top_k": TOP_K,
           "steps": args.steps, "attach": [], "cells": []}

    nq_max = max(args.queries)
    q_len = rng.integers(LQ_MIN, LQ_MAX + 1, size=nq_max).astype(np.int32)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(doc_len)

    def queries_for(scope):
        """query i: the first q_len[i] vectors of a passage of the scope, plus 0.3 unit noise"""
        lo, hi = scope
        src = rng.integers(lo, hi, size=nq_max)
        idx = np.concatenate([off[d] + np.arange(LQ_MAX) % doc_len[d] for d in src])
        v = store.gather_f32(idx).reshape(nq_max, LQ_MAX, dim)
        return unit(v + 0.3 * unit(torch.randn(v.shape, generator=g, device=dev))).to(torch.bfloat16)

    qc = torch.from_numpy(q_len).to(dev)
    for ncent in args.ncent:
        t0 = time.perf_counter()
        table = train_token_centroids(store, ncent)
        train_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        store.attach_centroids(table)                           # synchronous: returns with every stored vector coded
        attach_ms = (time.perf_counter() - t0) * 1e3
        res["attach"].append({"ncent": ncent, "train_ms": round(train_ms, 1), "attach_ms": round(attach_ms, 1),
                              "code_bytes": store.centroid_info()[2]})
        print(json.dumps(res["attach"][-1]), flush=True)
        for m in args.scopes:
            m = min(m, n)
            scope = (3, 3 + m) if m < n else (0, n)
            q = queries_for(scope)
            for nq in args.queries:
                qv, qcv, soq = q[:nq].contiguous(), qc[:nq].contiguous(), [0] * nq
                e_ms, (e_scores, e_ids) = timed(lambda: maxsim_search_device(store, qv, qcv, [[scope]], soq, TOP_K))
                for ncand in args.ncand:
                    run = lambda: maxsim_search_pruned_device(store, qv, qcv, [[scope]], soq, TOP_K, ncand, want_candidates=True)  # noqa: E731
                    p_ms, (p_scores, p_ids, c_ids, _cs) = timed(run)
                    info = store.pruned_info()
                    x_ms, _ = timed(lambda: maxsim_device(store, qv, qcv, c_ids, TOP_K, want_pairs=False))
                    e_ms2, _ = timed(lambda: maxsim_search_device(store, qv, qcv, [[scope]], soq, TOP_K))     # alternating
                    hit = [(len(set(a.tolist()) & set(b.tolist()) - {-1})) / TOP_K for a, b in zip(p_ids.cpu(), e_ids.cpu())]
                    res["cells"].append({"ncent": ncent, "scope_documents": m, "queries": nq, "ncand": ncand, "pruned_ms": p_ms,
                                         "exact_stage_ms": x_ms, "exact_search_ms": min(e_ms, e_ms2), "exact_search_ms_runs": [e_ms, e_ms2],
                                         "exact_over_pruned": round(min(e_ms, e_ms2) / p_ms, 2), "recall_at_10": round(float(np.mean(hit)), 4),
                                         "codes_read": info["codes_read"], "table_bytes": info["table_bytes"], "chunks": info["chunks"],
                                         "work_items": info["work_items"]})
                    print(json.dumps(res["cells"][-1]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
