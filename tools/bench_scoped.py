#!/usr/bin/env python3
"""
tools/bench_scoped.py -- the scoped search (hipidx_search_scoped_dev) on one collection index of 1M x 1024 rows, k = 10, inner
product, one GPU process.  Three groups of cells, each next to what it is measured against in the same process:

  kernel_rate   ONE query over a contiguous scope of 1 k / 10 k / 100 k rows (unaligned ends) and over a scope of 100 ranges of
                1 000 unaligned rows, against hipivf_search_dev on an IVF index whose lists hold 1 024 stored rows each, probing
                as many lists as cover the same number of rows (the probe kernel is the project's measured rate for this
                arithmetic).  ms per call (HIP events around the whole call, median) and GB/s = rows read x d_pad x 4 / time;
                rows_read is the library's own count (hipidx_scoped_info).
  replaces      100 documents of rows/100 rows each, one query: the per-document path (one `search` per document index and a
                host merge -- what search_all_documents does) over 1 / 10 / 100 documents against ONE search_scoped call over
                the same documents' row ranges in the collection, and the unscoped `search` of the collection.  Host entries,
                wall clock (the replaced path is a host loop), median.
  break_even    1 024 queries that share one scope of 0.5 % .. 100 % of the rows against hipidx_search_dev over the whole index
                for the same queries (HIP events, median); `break_even_share` is where the two meet, linearly interpolated
                between the measured shares.

    python tools/bench_scoped.py [--rows 1000000] [--dim 1024] [--warmup 2] [--steps 7] [--out profiles/scoped_1m.json]

torch generates the data and holds the buffers; every search runs in libhiprag.  One JSON line on stdout and in --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "intool-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

K = 10
LIST_ROWS = 1024     # stored rows per list of the comparison IVF index


def unit_rows(torch, n, d, seed, dev, chunk=1 << 17):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        r = torch.randn((m, d), generator=g, device=dev)
        x[o:o + m] = r / r.norm(dim=1, keepdim=True)
    return x


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


def wall_ms(torch, fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def cell(t):
    return {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}


def make_probe_index(torch, nat, x, n_lists, dev):
    """an IVF index over the first n_lists x LIST_ROWS rows of x, list l = stored rows [l x 1024, (l + 1) x 1024), random
    centroids: whatever lists a query probes, nprobe lists are nprobe x 1024 stored rows"""
    from hiprag import HipFlatIndex
    d = x.shape[1]
    rows = HipFlatIndex(d, "ip", device=dev.index)
    rows.add_device(x[:n_lists * LIST_ROWS])
    cents = HipFlatIndex(d, "ip", device=dev.index)
    cents.add_device(unit_rows(torch, n_lists, d, 99, dev))
    offs = (np.arange(n_lists + 1, dtype=np.int64) * LIST_ROWS)
    orig = np.arange(n_lists * LIST_ROWS, dtype=np.int64)
    h = ctypes.c_uint64()
    nat.call("hipivf_create", rows._h, cents._h, offs.ctypes.data, orig.ctypes.data, n_lists, ctypes.byref(h))
    return h.value, rows, cents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--docs", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scoped_1m.json"))
    args = ap.parse_args()

    import torch
    from hiprag import HipFlatIndex
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    dev = torch.device("cuda", 0)
    n, d = args.rows, args.dim
    d_pad = (d + 127) // 128 * 128
    x = unit_rows(torch, n, d, 1, dev)
    q = unit_rows(torch, args.batch, d, 2, dev)
    q1 = q[:1].contiguous()
    ix = HipFlatIndex(d, "ip", device=0)
    ix.add_device(x)
    out = {"tool": "bench_scoped", "rows": n, "dim": d, "k": K, "metric": "ip", "warmup": args.warmup, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "group_queries": None}
    bufs1 = (torch.empty((1, K), dtype=torch.float64, device=dev), torch.empty((1, K), dtype=torch.float32, device=dev),
             torch.empty((1, K), dtype=torch.int64, device=dev))

    # ---- 1. kernel rate: one query, against the IVF probe kernel over as many stored rows -----------------------------
    n_lists = min(128, n // LIST_ROWS)
    ivf_h, ivf_rows, ivf_cents = make_probe_index(torch, nat, x, n_lists, dev)
    lo0 = 12345 % max(1, n // 2)
    scopes = {"contiguous_1k": [(lo0, lo0 + 1000)], "contiguous_10k": [(lo0, lo0 + 10000)],
              "contiguous_100k": [(lo0, min(n, lo0 + 100000))],
              "100_ranges_of_1000": [(lo0 + j * (n - lo0) // 100, lo0 + j * (n - lo0) // 100 + 1000) for j in range(100)
                                     if lo0 + j * (n - lo0) // 100 + 1000 <= n]}
    rate = {}
    for name, scope in scopes.items():
        t = event_ms(torch, lambda: ix.search_scoped_device(q1, K, [scope], out=bufs1), args.warmup, args.steps)
        info = ix.scoped_info()
        out["group_queries"] = info["group_queries"]
        rows_read = info["rows_read"]
        nprobe = max(1, min(n_lists, round(rows_read / LIST_ROWS)))
        tp = event_ms(torch, lambda: nat.call("hipivf_search_dev", ivf_h, q1.data_ptr(), 1, K, nprobe, bufs1[0].data_ptr(),
                                              bufs1[1].data_ptr(), bufs1[2].data_ptr(), _stream_ptr()), args.warmup, args.steps)
        c = {"scoped": dict(cell(t), rows_read=rows_read, ranges=len(scope), gbps=round(rows_read * d_pad * 4 / t[0] / 1e6, 1)),
             "ivf_probe": dict(cell(tp), stored_rows=nprobe * LIST_ROWS, nprobe=nprobe,
                               gbps=round(nprobe * LIST_ROWS * d_pad * 4 / tp[0] / 1e6, 1))}
        c["scoped_rate_over_probe_rate"] = round(c["scoped"]["gbps"] / c["ivf_probe"]["gbps"], 3)
        rate[name] = c
    out["kernel_rate"] = rate
    out["kernel_rate_within_20pct_of_probe_at_100k"] = bool(rate["contiguous_100k"]["scoped_rate_over_probe_rate"] >= 0.8)
    nat.call("hipivf_destroy", ivf_h)
    ivf_rows.close()
    ivf_cents.close()

    # ---- 2. what the feature replaces: one search per document and a host merge ----------------------------------------
    per_doc = n // args.docs
    docs = []
    for i in range(args.docs):
        di = HipFlatIndex(d, "ip", device=0)
        di.add_device(x[i * per_doc:(i + 1) * per_doc])
        docs.append(di)
    q1h = q1.cpu().numpy()

    def per_document(m):
        merged = []
        for i in range(m):
            s, ids = docs[i].search(q1h, K)
            merged += [(-float(sv), i, r, int(iv)) for r, (sv, iv) in enumerate(zip(s[0], ids[0])) if iv >= 0]
        merged.sort()
        return merged[:K]

    rep = {"documents": args.docs, "rows_per_document": per_doc}
    for m in (1, 10, args.docs):
        scope = [(0, m * per_doc)]
        a = wall_ms(torch, lambda: per_document(m), args.warmup, args.steps)
        b = wall_ms(torch, lambda: ix.search_scoped(q1h, K, [scope]), args.warmup, args.steps)
        want = [(i * per_doc + r) for _s, i, _r, r in per_document(m)]
        got = ix.search_scoped(q1h, K, [scope])[1][0].tolist()
        rep[f"{m}_documents"] = {"per_document_searches": cell(a), "one_scoped_call": cell(b), "same_ids": want == got,
                                 "speedup": round(a[0] / b[0], 2)}
    rep["unscoped_search_of_the_collection"] = cell(wall_ms(torch, lambda: ix.search(q1h, K), args.warmup, args.steps))
    rep["one_scoped_call_over_10_documents_faster_than_10_searches"] = bool(rep["10_documents"]["speedup"] > 1.0)
    out["replaces"] = rep
    for di in docs:
        di.close()

    # ---- 3. where it stops paying: a batch that shares one scope against the flat search -------------------------------
    nq = args.batch
    bufs = (torch.empty((nq, K), dtype=torch.float64, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev),
            torch.empty((nq, K), dtype=torch.int64, device=dev))
    tf = event_ms(torch, lambda: ix.search_device(q, K, out=bufs), args.warmup, args.steps)
    be = {"queries": nq, "flat_search_whole_index": dict(cell(tf), queries_per_s=round(nq / tf[0] * 1e3))}
    shares, times = [0.005, 0.01, 0.02, 0.05, 0.1, 1.0], []
    for share in shares:
        rows = max(1, int(n * share))
        scope = [(7, 7 + rows)] if 7 + rows <= n else [(0, n)]
        steps = args.steps if share < 1.0 else max(2, args.steps // 3)
        t = event_ms(torch, lambda: ix.search_scoped_device(q, K, [scope], out=bufs), min(args.warmup, 1), steps)
        info = ix.scoped_info()
        times.append(t[0])
        be[f"scope_{share * 100:g}pct"] = dict(cell(t), rows=rows, rows_read=info["rows_read"], chunks=info["chunks"],
                                                queries_per_s=round(nq / t[0] * 1e3), over_flat=round(t[0] / tf[0], 3))
    share_star = None
    pts = [(0.0, 0.0)] + list(zip(shares, times))
    for (s0, t0), (s1, t1) in zip(pts, pts[1:]):
        if t0 <= tf[0] <= t1 and t1 > t0:
            share_star = s0 + (s1 - s0) * (tf[0] - t0) / (t1 - t0)
            break
    be["break_even_share"] = None if share_star is None else round(share_star, 4)
    out["break_even"] = be

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
