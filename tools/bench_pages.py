#!/usr/bin/env python3
"""
tools/bench_pages.py -- the device page-ranking call (hippage_rank_dev over a page table) against the host path it
replaces, in ONE process, in alternation.  Table: 1M rows, documents of 200 rows, four rows to a page.  Per query 50
candidates drawn from three documents (so pages have several members) with float32 L2 scores; max_pages 5; 1, 64 and
16 384 queries.

Per cell, medians over --steps (step 0 warms both sides):
    device   gpu_ms       HIP events around the call on its stream
             enqueue_ms   host wall clock until the call has returned, nothing waited for
             wall_ms      until all eight outputs are on the host (two copies)
    host     wall_ms      what the retriever does today from device-resident search results: copy ids and scores back
                          (synchronises), collection._transform per query, RetrievedChunk objects keyed by the row's page,
                          group_chunks_by_page and rank_pages per query, then a synchronise.  Enriching the rows against
                          their chunk tables (collection._enrich, one lookup per row) is NOT included: the host side is a
                          lower bound.
The table's append rate (100 000-row batches) and removal rate (ten ranges of 1 000 rows spread over the table; rows moved
per second) are recorded too.

    python tools/bench_pages.py [--rows 1000000] [--steps 5] [--out profiles/pages_1m.json]
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

DEPTH, MAX_PAGES, DOC_ROWS = 50, 5, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 16384])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from hiprag import METRIC_L2, PageTable, rank_pages_device
    from hiprag.pages import doc_offsets
    from rag.query.retriever import RetrievedChunk, group_chunks_by_page, rank_pages
    from rag.storage.hip_index.collection import _transform

    n = args.rows // DOC_ROWS * DOC_ROWS
    pages = (np.arange(n, dtype=np.int64) % DOC_ROWS // 4 + 1).astype(np.int32)
    table = PageTable()
    t0 = time.perf_counter()
    for lo in range(0, n, 100_000):
        hi = min(n, lo + 100_000)
        table.append(pages[lo:hi], doc_offsets([DOC_ROWS] * ((hi - lo) // DOC_ROWS)))
    append_s = time.perf_counter() - t0
    res = {"rows": n, "documents": n // DOC_ROWS, "depth": DEPTH, "max_pages": MAX_PAGES, "steps": args.steps,
           "append_rows_per_s": round(n / append_s), "cells": []}

    class _Coll:                                   # what _transform reads of a collection
        class index:
            metric = METRIC_L2

    def med(v):
        return round(float(np.median(v)), 4)

    rng = np.random.default_rng(9)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for nq in args.queries:
        docs = rng.integers(0, n // DOC_ROWS, size=(nq, 3))
        cand = (docs[np.arange(nq)[:, None], rng.integers(0, 3, size=(nq, DEPTH))] * DOC_ROWS
                + rng.integers(0, DOC_ROWS, size=(nq, DEPTH))).astype(np.int64)
        vals = rng.uniform(0.0, 2.0, size=(nq, DEPTH)).astype(np.float32)
        ids_dev, vals_dev = torch.from_numpy(cand).cuda(), torch.from_numpy(vals).cuda()
        t = {k: [] for k in ("gpu", "enqueue", "dev_wall", "host_wall")}
        for step in range(args.steps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            out = rank_pages_device(table, ids_dev, ids_dev, vals_dev.double(), MAX_PAGES, metric=METRIC_L2)
            ev[1].record()
            t1 = time.perf_counter()
            got = out.host()
            t2 = time.perf_counter()
            # the host path from the same device-resident lists
            t3 = time.perf_counter()
            ids_h, vals_h = ids_dev.cpu().numpy(), vals_dev.cpu().numpy()
            host = []
            for q in range(nq):
                chunks = [RetrievedChunk(str(row), "", score, int(pages[row]), {}) for row, score in _transform(_Coll, vals_h[q], ids_h[q])]
                host.append(rank_pages(group_chunks_by_page(chunks))[:MAX_PAGES])
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            if step:
                t["gpu"].append(ev[0].elapsed_time(ev[1]))
                t["enqueue"].append((t1 - t0) * 1e3)
                t["dev_wall"].append((t2 - t0) * 1e3)
                t["host_wall"].append((t4 - t3) * 1e3)
        cell = {"queries": nq, "device": {"gpu_ms": med(t["gpu"]), "enqueue_ms": med(t["enqueue"]), "wall_ms": med(t["dev_wall"])},
                "host": {"wall_ms": med(t["host_wall"])}}
        cell["ms_per_query"] = {"device_wall": round(cell["device"]["wall_ms"] / nq, 5), "host_wall": round(cell["host"]["wall_ms"] / nq, 5)}
        cell["wall_host_over_device"] = round(cell["host"]["wall_ms"] / cell["device"]["wall_ms"], 2)
        del got
        res["cells"].append(cell)
    # removal: ten ranges of 1 000 rows spread over the table
    ranges = [(lo, lo + 1000) for lo in np.linspace(0, n - 1000, 10).astype(np.int64).tolist()]
    moved = n - ranges[0][0] - 10 * 1000
    t0 = time.perf_counter()
    table.remove_ranges(ranges)
    remove_s = time.perf_counter() - t0
    assert len(table) == n - 10 * 1000
    res["remove"] = {"ranges": 10, "rows_removed": 10 * 1000, "rows_moved": int(moved), "ms": round(remove_s * 1e3, 2),
                     "rows_moved_per_s": round(moved / remove_s)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
