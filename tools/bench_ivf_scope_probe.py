#!/usr/bin/env python3
"""
tools/bench_ivf_scope_probe.py -- scope-aware probing (hipivf_search_scoped_probe_dev, HIPIVF_PROBE_SCOPE) on a clustered
collection of 1M x 1024 rows with DOCUMENT-COHERENT ids (consecutive blocks of 256 ids are drawn around one centre, as the
chunks of a document are), 1024 lists, nprobe 8, k = 10, inner product, one GPU process.  A cell = (share of the rows in the
scope: 0.1 % / 1 % / 10 % / 100 %, one contiguous id range = a project of consecutive documents) x (batch: 1 / 64 / 16 384
queries near rows of the scope).  In every cell, in the same process and on the same queries:

  probe_scope   hipivf_search_scoped_probe_dev, HIPIVF_PROBE_SCOPE;
  probe_any     hipivf_search_scoped_dev (the entry as it was before the mode existed), same nprobe;
  flat_scoped   hipidx_search_scoped_dev on a flat index of the same rows: exact, the reference of both recalls.

recall_at_10 = the mean share of the flat scoped search's ids a mode returns (over at most 256 queries of the batch);
`any_nprobe_for_scope_recall` = the smallest nprobe in 8, 16, 32, ... nlist at which probe_any reaches probe_scope's recall,
with its queries/s.  ms per call = HIP events around the whole call, median.  `info` = hipivf_scope_probe_info of the
probe_scope call.  No threshold: the file reports, it does not judge.

    python tools/bench_ivf_scope_probe.py [--rows 1000000] [--dim 1024] [--nlist 1024] [--nprobe 8] [--warmup 2] [--steps 7]
                                          [--out profiles/ivf_scope_probe_1m.json]

torch generates the data and holds the buffers; every search and the build run in libhiprag.  One JSON line on stdout and
in --out.
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

K = 10
SHARES = (0.001, 0.01, 0.1, 1.0)
BATCHES = (1, 64, 16384)
BLOCK = 256            # ids per document
RECALL_QUERIES = 256


def unit(torch, x):
    return x / x.norm(dim=1, keepdim=True)


def coherent(torch, n, d, n_centres, sigma, seed, dev):
    """block b of BLOCK consecutive ids = centre c(b) + sigma * g / sqrt(d), renormalised; centres uniform on the sphere"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = unit(torch, torch.randn((n_centres, d), generator=g, device=dev))
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    step = BLOCK * 512
    for o in range(0, n, step):
        m = min(step, n - o)
        c = torch.randint(0, n_centres, ((m + BLOCK - 1) // BLOCK,), generator=g, device=dev).repeat_interleave(BLOCK)[:m]
        x[o:o + m] = unit(torch, centres[c] + sigma * torch.randn((m, d), generator=g, device=dev) / d ** 0.5)
    return x


def near_rows(torch, x, lo, hi, nq, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    d = x.shape[1]
    rows = lo + torch.randint(0, hi - lo, (nq,), generator=g, device=dev)
    return unit(torch, x[rows] + 0.1 * torch.randn((nq, d), generator=g, device=dev) / d ** 0.5).contiguous()


def event_ms(torch, fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def cell(t, nq):
    return {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4), "queries_per_s": round(nq / t[0] * 1e3)}


def recall(torch, got, want):
    """mean over the queries of |got ids in want ids| / |want ids| (padding excluded; a query without a wanted id counts 1)"""
    m = min(RECALL_QUERIES, got.shape[0])
    g, w = got[:m], want[:m]
    hit = ((g.unsqueeze(2) == w.unsqueeze(1)) & (w.unsqueeze(1) >= 0)).any(dim=1).sum(dim=1).double()
    cnt = (w >= 0).sum(dim=1).double()
    return float(torch.where(cnt > 0, hit / cnt.clamp(min=1), torch.ones_like(cnt)).mean().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivf_scope_probe_1m.json"))
    args = ap.parse_args()

    import torch
    from hiprag import HipFlatIndex, HipIVFIndex
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_scope_probe needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    n, d, nprobe, nlist = args.rows, args.dim, args.nprobe, args.nlist
    x = coherent(torch, n, d, 2048, 0.5, 1, dev)
    flat = HipFlatIndex(d, "ip", device=0)
    flat.add_device(x)
    ivf = HipIVFIndex(d, nlist, "ip", device=0)
    ivf.build(x, iters=args.iters, seed=0)
    out = {"tool": "tools/bench_ivf_scope_probe.py", "device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "nlist": nlist,
           "nprobe": nprobe, "k": K, "metric": "ip", "iters": args.iters, "longest_list": int(ivf.list_lengths.max()),
           "coherent_set": f"2048 centres uniform on the sphere; every block of {BLOCK} consecutive ids = one centre + 0.5 * g / "
                           "sqrt(d), renormalised; queries: rows of the scope + 0.1 * g / sqrt(d), renormalised",
           "timing": f"HIP events around one call, median of {args.steps} after {args.warmup} warm-up calls (2 after 1 where a "
                     f"call takes > 0.5 s)",
           "probe_any_is": "hipivf_search_scoped_dev, the entry of the parent commit, on the same inputs", "cells": []}
    lo0 = (12345 % max(1, n // 2)) // BLOCK * BLOCK
    for share in SHARES:
        rows = max(1, int(round(n * share)))
        scope = [(lo0, lo0 + rows)] if lo0 + rows <= n and share < 1.0 else [(0, n)]
        lo, hi = scope[0]
        q_all = near_rows(torch, x, lo, hi, max(BATCHES), 2, dev)
        for nq in BATCHES:
            q = q_all[:nq].contiguous()
            bufs = [tuple(torch.empty((nq, K), dtype=t, device=dev) for t in (torch.float64, torch.float32, torch.int64)) for _ in range(3)]

            def timed(fn):
                first = event_ms(torch, fn, 1, 1)
                if first[0] > 500.0:
                    return event_ms(torch, fn, 0, 2)
                return event_ms(torch, fn, max(0, args.warmup - 1), args.steps)

            t_scope = timed(lambda: ivf.search_scoped_device(q, K, [scope], nprobe=nprobe, out=bufs[0], probe="scope"))
            info = ivf.scope_probe_info()
            t_any = timed(lambda: ivf.search_scoped_device(q, K, [scope], nprobe=nprobe, out=bufs[1]))
            t_flat = timed(lambda: flat.search_scoped_device(q, K, [scope], out=bufs[2]))
            torch.cuda.synchronize()
            r_scope, r_any = recall(torch, bufs[0][2], bufs[2][2]), recall(torch, bufs[1][2], bufs[2][2])
            reach, p = None, nprobe
            while p <= nlist:
                t_p = timed(lambda: ivf.search_scoped_device(q, K, [scope], nprobe=p, out=bufs[1]))
                torch.cuda.synchronize()
                r_p = recall(torch, bufs[1][2], bufs[2][2])
                if r_p >= r_scope:
                    reach = dict(nprobe=p, recall_at_10=round(r_p, 4), **cell(t_p, nq))
                    break
                p = p * 2 if p * 2 <= nlist or p == nlist else nlist
            c = {"queries": nq, "share": share, "scope_rows": hi - lo, "probe_scope": dict(recall_at_10=round(r_scope, 4), **cell(t_scope, nq)),
                 "probe_any": dict(recall_at_10=round(r_any, 4), **cell(t_any, nq)), "flat_scoped": cell(t_flat, nq),
                 "any_nprobe_for_scope_recall": reach, "info": info}
            out["cells"].append(c)
            print(json.dumps(c), file=sys.stderr, flush=True)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
