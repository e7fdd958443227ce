#!/usr/bin/env python3
"""
tools/bench_score_ids.py -- scoring rows by id (hipidx_score_ids_dev) on one index of 1M x 1024 rows, inner product, one GPU
process: 50 candidate ids per query (uniformly random rows, all valid), 1 / 64 / 16 384 queries per call.

  score_ids     ms per call (HIP events around the call, median) and bytes per second, counting what the kernel reads of
                the rows: 128 bytes (one quad line) per piece and valid pair = d_pad x 16 bytes per pair.  `valid`,
                `workgroups` are the library's own counts (hipidx_score_info).
  replaces      the only route to the same numbers without this call: hipidx_search_scoped_dev with k = 1 and ONE ONE-ROW
                SCOPE PER CANDIDATE, i.e. nq x 50 queries (each query repeated 50 times) over nq x 50 scopes.  At 1 and 64
                queries per call, with the repetition of the queries and the packing of the scope tables outside the timed
                region (only the library call is timed), and `same_bits` = the two calls' fp64 scores compared bit for bit.

    python tools/bench_score_ids.py [--rows 1000000] [--dim 1024] [--depth 50] [--warmup 2] [--steps 7]
                                    [--out profiles/score_ids_1m.json]

torch generates the data and holds the buffers; every score comes from libhiprag.  One JSON line on stdout and in --out.
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


def unit_rows(torch, n, d, seed, dev, chunk=1 << 17):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    for o in range(0, n, chunk):
        r = torch.randn((min(chunk, n - o), d), generator=g, device=dev)
        yield r / r.norm(dim=1, keepdim=True)


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


def cell(t):
    return {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_ids_1m.json"))
    args = ap.parse_args()

    import torch
    from hiprag import HipFlatIndex
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr, pack_scopes
    dev = torch.device("cuda", 0)
    n, d, depth = args.rows, args.dim, args.depth
    pair_bytes = (d + 7) // 8 * 128                      # one 128-byte line of each of the row's pieces
    ix = HipFlatIndex(d, "ip", device=0)
    ix.reserve_rows(n)
    for part in unit_rows(torch, n, d, 1, dev):
        ix.add_device(part)
    batches = (1, 64, 16384)
    q = torch.cat(list(unit_rows(torch, max(batches), d, 2, dev)))
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    ids = torch.randint(0, n, (max(batches), depth), generator=g, device=dev, dtype=torch.int64)
    out = {"tool": "bench_score_ids", "rows": n, "dim": d, "depth": depth, "metric": "ip", "warmup": args.warmup, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "bytes_per_pair": pair_bytes}

    cells = {}
    for nq in batches:
        qn, idn = q[:nq].contiguous(), ids[:nq].contiguous()
        bufs = (torch.empty((nq, depth), dtype=torch.float64, device=dev), torch.empty((nq, depth), dtype=torch.float32, device=dev))
        t = event_ms(torch, lambda: ix.score_ids_device(qn, idn, out=bufs), args.warmup, args.steps)
        info = ix.score_info()
        c = {"score_ids": dict(cell(t), valid=info["valid"], workgroups=info["workgroups"],
                               gbps=round(info["valid"] * pair_bytes / t[0] / 1e6, 1), pairs_per_s=round(nq * depth / t[0] * 1e3))}
        if nq <= 64:
            # one one-row scope per candidate, k = 1: query i repeated `depth` times, pair (i, j) searches scope i x depth + j
            rows = idn.cpu().numpy().reshape(-1)
            ranges, offsets, soq = pack_scopes([[(int(r), int(r) + 1)] for r in rows], None, nq * depth)
            qrep = qn.repeat_interleave(depth, dim=0).contiguous()
            sb = (torch.empty((nq * depth, 1), dtype=torch.float64, device=dev), torch.empty((nq * depth, 1), dtype=torch.float32, device=dev),
                  torch.empty((nq * depth, 1), dtype=torch.int64, device=dev))
            ts = event_ms(torch, lambda: nat.call("hipidx_search_scoped_dev", ix._h, qrep.data_ptr(), nq * depth, 1, ranges.ctypes.data,
                                                  offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, sb[0].data_ptr(), sb[1].data_ptr(),
                                                  sb[2].data_ptr(), _stream_ptr()), args.warmup, args.steps)
            torch.cuda.synchronize()
            c["one_row_scopes"] = dict(cell(ts), scopes=nq * depth,
                                       same_bits=bool(torch.equal(sb[0].view(torch.int64).view(nq, depth), bufs[0].view(torch.int64))))
            c["speedup"] = round(ts[0] / t[0], 2)
        cells[f"{nq}_queries"] = c
    out["cells"] = cells

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
