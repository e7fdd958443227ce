#!/usr/bin/env python3
"""
tools/bench_ivf_update.py -- hipivf_add_dev and hipivf_remove_ranges on one IVF-Flat index of 1M x 1024 rows in 1024 lists,
inner product, one GPU process.  Five cases: an add of 1 000 rows; a 1 000-row id range removed at the front, in the middle
and at the back; 1 % of the rows removed as 100 scattered ranges.  Per case: wall ms of the (synchronous) library call,
median over --steps fresh indexes (centroids trained once, every fresh index = hipivf_from_centroids + one hipivf_add_dev of
all rows, also timed), and hipivf_update_info of the call (rows added, removed, stored rows moved, staging chunks, extra
device bytes).  Next to each, in the same process, the only route there was before: hipivf_build_dev of the resulting row
set with the same --iters.  Nothing is gated on these numbers.

    python tools/bench_ivf_update.py [--rows 1000000] [--dim 1024] [--nlist 1024] [--iters 6] [--steps 3] [--out profiles/ivf_update_1m.json]

torch generates the data and holds the buffers; everything timed runs in libhiprag.  One JSON line on stdout and in --out.
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

DOC_ROWS = 1000


def clustered_rows(torch, n, d, n_centres, seed, dev, chunk=1 << 17):
    """rows = a centre on the sphere + 0.5 g / sqrt(d), normalised (the generator of tools/bench_ivf.py, restated)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    c = torch.randn((n_centres, d), generator=g, device=dev)
    c = c / c.norm(dim=1, keepdim=True)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        r = c[torch.randint(0, n_centres, (m,), generator=g, device=dev)] + 0.5 / d ** 0.5 * torch.randn((m, d), generator=g, device=dev)
        x[o:o + m] = r / r.norm(dim=1, keepdim=True)
    return x


def cases(n):
    docs = n // DOC_ROWS
    out = {"add_1000": None, "remove_front": [(0, DOC_ROWS)], "remove_middle": [(n // 2, n // 2 + DOC_ROWS)],
           "remove_back": [(n - DOC_ROWS, n)]}
    if docs >= 100:
        step = docs // 100 * DOC_ROWS
        out["remove_scattered_100_ranges"] = [(i * step, i * step + n // 10000) for i in range(100)] if n >= 10000 else []
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from hiprag import HipIVFIndex
    dev = torch.device("cuda", 0)
    n, d = args.rows, args.dim
    x = clustered_rows(torch, n + DOC_ROWS, d, 2 * args.nlist, 1234, dev)       # the last 1 000 rows are the add's batch
    base, extra = x[:n], x[n:]
    trained = HipIVFIndex(d, args.nlist, "ip")
    trained.build(base, iters=args.iters)
    cents = trained.centroids()
    trained.close()
    result = {"rows": n, "dim": d, "nlist": args.nlist, "metric": "ip", "iters": args.iters, "steps": args.steps, "cases": {}}
    for name, ranges in cases(n).items():
        if ranges is None:
            after = x
        else:
            keep = torch.ones(n, dtype=torch.bool, device=dev)
            for lo, hi in ranges:
                keep[lo:hi] = False
            after = base[keep].contiguous()
        up_ms, fill_ms, build_ms, info = [], [], [], None
        for _ in range(args.steps):
            ix = HipIVFIndex.from_centroids(cents, "ip")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.add(base)                                           # synchronous
            fill_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            if ranges is None:
                ix.add(extra)
            else:
                ix.remove_ranges(ranges)
            up_ms.append((time.perf_counter() - t0) * 1e3)         # includes the wrapper's re-read of the lists
            info = ix.update_info()
            assert ix.ntotal == after.shape[0]
            ix.close()
            t0 = time.perf_counter()
            fresh = HipIVFIndex(d, args.nlist, "ip")
            fresh.build(after, iters=args.iters)                   # synchronises the stream
            build_ms.append((time.perf_counter() - t0) * 1e3)
            fresh.close()
        result["cases"][name] = {
            "ranges": 0 if ranges is None else len(ranges), "update_info": info,
            "update_ms": round(float(np.median(up_ms)), 3), "update_ms_all": [round(v, 3) for v in up_ms],
            "fill_from_centroids_ms": round(float(np.median(fill_ms)), 3),
            "rebuild_ms": round(float(np.median(build_ms)), 3), "rebuild_ms_all": [round(v, 3) for v in build_ms],
        }
        if ranges is not None:
            del after, keep
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
