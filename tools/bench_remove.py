#!/usr/bin/env python3
"""
tools/bench_remove.py -- hipidx_remove_ranges on one flat index of 1M x 1024 rows, inner product, one GPU process.  Four cases:
one 1 000-row document removed at the front, in the middle and at the back, and 1 % of the rows removed as 100 scattered
documents.  Per case: wall ms of the (synchronous) call, median over --steps fresh indexes; rows_moved as the library counts
them (hipidx_remove_info); the algorithmic bytes = rows_moved x d_pad x 6 x 2 (fp32 rows and bf16 filter copy, read and
written once; the staging round trip of the in-place move is NOT counted) + the statistics pass's read of the surviving fp32
rows; GB/s = those bytes / time.  Next to each, in the same process, the only way there was before: a fresh index and
hipidx_add_dev of the surviving rows from a device tensor (the gather of the survivors is not timed).

    python tools/bench_remove.py [--rows 1000000] [--dim 1024] [--steps 3] [--out profiles/remove_1m.json]

torch generates the data and holds the buffers; the removal and the adds run in libhiprag.  One JSON line on stdout and in --out.
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


def unit_rows(torch, n, d, seed, dev, chunk=1 << 17):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        r = torch.randn((m, d), generator=g, device=dev)
        x[o:o + m] = r / r.norm(dim=1, keepdim=True)
    return x


def cases(n):
    docs = n // DOC_ROWS
    scattered = [(i * (docs // 100) * DOC_ROWS, i * (docs // 100) * DOC_ROWS + DOC_ROWS) for i in range(100)] if docs >= 100 else []
    out = {"front": [(0, DOC_ROWS)], "middle": [(n // 2, n // 2 + DOC_ROWS)], "back": [(n - DOC_ROWS, n)]}
    if scattered and sum(hi - lo for lo, hi in scattered) * 100 == n:
        out["scattered_1pct"] = scattered
    elif scattered:
        out["scattered_100_docs"] = scattered
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from hiprag import HipFlatIndex
    dev = torch.device("cuda", 0)
    n, d = args.rows, args.dim
    d_pad = (d + 127) // 128 * 128
    x = unit_rows(torch, n, d, 1234, dev)
    result = {"rows": n, "dim": d, "metric": "ip", "steps": args.steps, "cases": {}}
    for name, ranges in cases(n).items():
        keep = torch.ones(n, dtype=torch.bool, device=dev)
        for lo, hi in ranges:
            keep[lo:hi] = False
        survivors = x[keep].contiguous()
        rm_ms, add_ms, info = [], [], None
        for _ in range(args.steps):
            ix = HipFlatIndex(d, "ip")
            ix.add_device(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.remove_ranges(ranges)                       # synchronous
            rm_ms.append((time.perf_counter() - t0) * 1e3)
            info = ix.remove_info()
            assert ix.ntotal == survivors.shape[0]
            ix.close()
            t0 = time.perf_counter()
            fresh = HipFlatIndex(d, "ip")
            fresh.add_device(survivors)                    # synchronises the stream
            torch.cuda.synchronize()
            add_ms.append((time.perf_counter() - t0) * 1e3)
            fresh.close()
        ms = float(np.median(rm_ms))
        moved_bytes = info["rows_moved"] * d_pad * 6 * 2
        stats_bytes = int(survivors.shape[0]) * d_pad * 4
        result["cases"][name] = {
            "ranges": len(ranges), "rows_removed": info["rows_removed"], "rows_moved": info["rows_moved"], "chunks": info["chunks"],
            "staging_bytes": info["staging_bytes"], "remove_ms": round(ms, 3), "remove_ms_all": [round(v, 3) for v in rm_ms],
            "moved_bytes": moved_bytes, "stats_read_bytes": stats_bytes,
            "gb_per_s": round((moved_bytes + stats_bytes) / (ms * 1e-3) / 1e9, 1),
            "fresh_add_dev_ms": round(float(np.median(add_ms)), 3), "fresh_add_dev_ms_all": [round(v, 3) for v in add_ms],
        }
        del survivors, keep
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
