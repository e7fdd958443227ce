#!/usr/bin/env python3
"""
tools/bench_ivf_scoped.py -- the scoped IVF search (hipivf_search_scoped_dev) on a clustered collection of 1M x 1024 rows,
1024 lists, nprobe 8, k = 10, inner product, one GPU process.  A cell = (share of the rows in the scope: 0.1 % / 1 % / 10 % /
100 %, one contiguous id range) x (batch: 1 / 64 / 16 384 queries that share the scope).  In every cell, in the same process
and on the same queries, beside it the two things a caller can do without it:

  flat_scoped       hipidx_search_scoped_dev on a flat index of the same rows (exact: it reads every row of the scope);
  batch_postfilter  hipivf_search_batch_dev at a deeper k = min(256, ceil(k / share)), the caller keeping the first k hits
                    inside the scope.  `same_ids_share` is the share of the queries for which that gives the scoped IVF's
                    ids: below 1.0 the deeper list ran out of in-scope hits (k is capped at 256), i.e. it is not a substitute.

ms per call = HIP events around the whole call, median; rows_read = the library's own count (hipivf_scoped_info: 4 x the quads
loaded; hipidx_scoped_info for the flat one).  `fastest` names the quickest of the three per cell, `ivf_scoped_stops_winning_at`
per batch size the smallest measured share at which the scoped IVF is not it (null: it is at every share).  No threshold:
the file reports, it does not judge.

    python tools/bench_ivf_scoped.py [--rows 1000000] [--dim 1024] [--nlist 1024] [--nprobe 8] [--warmup 2] [--steps 7]
                                     [--out profiles/ivf_scoped_1m.json]

torch generates the data and holds the buffers; every search and the build run in libhiprag.  One JSON line on stdout and
in --out.
"""
import argparse
import json
import math
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


def unit(torch, x):
    return x / x.norm(dim=1, keepdim=True)


def clustered(torch, n, d, n_centres, sigma, seed, dev, chunk=1 << 17):
    """tools/bench_ivf.py's clustered set: centres uniform on the sphere, row = centre + sigma * g / sqrt(d), renormalised"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = unit(torch, torch.randn((n_centres, d), generator=g, device=dev))
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        c = torch.randint(0, n_centres, (m,), generator=g, device=dev)
        x[o:o + m] = unit(torch, centres[c] + sigma * torch.randn((m, d), generator=g, device=dev) / d ** 0.5)
    return x


def near_rows(torch, x, nq, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n, d = x.shape
    rows = torch.randint(0, n, (nq,), generator=g, device=dev)
    return unit(torch, x[rows] + 0.1 * torch.randn((nq, d), generator=g, device=dev) / d ** 0.5).contiguous()


def event_ms(torch, fn, warmup, steps):
    """median milliseconds of fn() between two HIP events on the current stream"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivf_scoped_1m.json"))
    args = ap.parse_args()

    import torch
    from hiprag import HipFlatIndex, HipIVFIndex
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf_scoped needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    n, d, nprobe = args.rows, args.dim, args.nprobe
    x = clustered(torch, n, d, 2048, 0.5, 1, dev)
    q_all = near_rows(torch, x, max(BATCHES), 2, dev)
    flat = HipFlatIndex(d, "ip", device=0)
    flat.add_device(x)
    ivf = HipIVFIndex(d, args.nlist, "ip", device=0)
    ivf.build(x, iters=args.iters, seed=0)
    del x
    out = {"tool": "tools/bench_ivf_scoped.py", "device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "nlist": args.nlist,
           "nprobe": nprobe, "k": K, "metric": "ip", "iters": args.iters, "longest_list": int(ivf.list_lengths.max()),
           "clustered_set": "2048 centres uniform on the sphere, row = centre + 0.5 * g / sqrt(d), renormalised; queries: rows + "
                            "0.1 * g / sqrt(d), renormalised",
           "timing": f"HIP events around one call, median of {args.steps} after {args.warmup} warm-up calls (2 after 1 where a "
                     f"call takes > 0.5 s)", "cells": []}
    lo0 = 12345 % max(1, n // 2)
    for nq in BATCHES:
        q = q_all[:nq].contiguous()
        for share in SHARES:
            rows = max(1, int(round(n * share)))
            scope = [(lo0, lo0 + rows)] if lo0 + rows <= n and share < 1.0 else [(0, n)]
            lo, hi = scope[0]
            deep = min(256, max(K, math.ceil(K / share)))
            bufs = tuple(torch.empty((nq, K), dtype=t, device=dev) for t in (torch.float64, torch.float32, torch.int64))
            deep_bufs = tuple(torch.empty((nq, deep), dtype=t, device=dev) for t in (torch.float64, torch.float32, torch.int64))

            def timed(fn):
                first = event_ms(torch, fn, 1, 1)
                if first[0] > 500.0:
                    return event_ms(torch, fn, 0, 2)
                return event_ms(torch, fn, max(0, args.warmup - 1), args.steps)

            t_ivf = timed(lambda: ivf.search_scoped_device(q, K, [scope], nprobe=nprobe, out=bufs))
            info = ivf.scoped_info()
            got = bufs[2].clone()
            t_post = timed(lambda: ivf.search_batch_device(q, deep, nprobe, out=deep_bufs))
            ids = deep_bufs[2]
            inside = (ids >= lo) & (ids < hi)
            rank = torch.cumsum(inside.to(torch.int64), dim=1)
            filtered = torch.full((nq, K), -1, dtype=torch.int64, device=dev)
            for r in range(K):                   # the r-th in-scope hit of the deeper list
                hit = inside & (rank == r + 1)
                has = hit.any(dim=1)
                filtered[has, r] = ids[has][hit[has]]
            same = float((filtered == got).all(dim=1).float().mean().item())
            t_flat = timed(lambda: flat.search_scoped_device(q, K, [scope], out=bufs))
            finfo = flat.scoped_info()
            c = {"queries": nq, "share": share, "scope_rows": hi - lo,
                 "ivf_scoped": dict(cell(t_ivf, nq), rows_read=info["rows_read"], chunks=info["chunks"]),
                 "flat_scoped": dict(cell(t_flat, nq), rows_read=finfo["rows_read"], chunks=finfo["chunks"]),
                 "batch_postfilter": dict(cell(t_post, nq), k=deep, rows_read=ivf.batch_info()["rows_read"], same_ids_share=round(same, 4))}
            c["fastest"] = min(("ivf_scoped", "flat_scoped", "batch_postfilter"), key=lambda name: c[name]["ms"])
            out["cells"].append(c)
            print(json.dumps(c), file=sys.stderr, flush=True)
    out["ivf_scoped_stops_winning_at"] = {
        str(nq): next((c["share"] for c in out["cells"] if c["queries"] == nq and c["fastest"] != "ivf_scoped"), None) for nq in BATCHES}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
