#!/usr/bin/env python3
"""
tools/bench_ivf.py -- IVF-Flat on a CLUSTERED collection (one GPU process): build time split into assignment / update / layout,
save and load time, and recall@10 against the exact flat top-10 with the single-query p50 at nprobe 1 / 8 / 32 / 128; the same
on isotropic Gaussian rows (bench.py's legs.ivf data, where recall is nprobe / nlist by construction) for comparison.

Clustered set (seeded): C centres uniform on the sphere; row = centre + sigma * g / sqrt(d), g standard normal, renormalised.
Queries: half are rows + 0.1 * g / sqrt(d) (renormalised), half are held-out points drawn like the rows.

    python tools/bench_ivf.py [--rows 1000000] [--dim 1024] [--nlist 1024] [--iters 6] [--out profiles/ivf_clustered.json]

    python tools/bench_ivf.py --batch [--out profiles/ivf_batch_1m.json]

--batch: on the clustered set only, k = 10, inner product, queries/s of a batch of nq queries at nprobe 1 / 8 / 32 / 128 through
(a) hipivf_search_dev (query-major), (b) hipivf_search_batch_dev (list-major) and (c) the flat hipidx_search_dev over the same
rows, in one process: HIP events around each of 5 calls after 2 warm-up calls (1 where a call takes seconds), median;
`identical` compares the complete outputs of (a) and (b) on the device; `rows_read` is the batch entry's own count of the
stored rows it read.  --batch-nq / --batch-nprobe / --batch-only-new cut the grid down (for a run under rocprofv3
--kernel-trace --stats, which is a run of its own).

torch generates the data and holds the buffers; every search and the build run in libhiprag.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "intool-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def unit(torch, x):
    return x / x.norm(dim=1, keepdim=True)


def clustered(torch, n, d, n_centres, sigma, seed, dev, chunk=1 << 17):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = unit(torch, torch.randn((n_centres, d), generator=g, device=dev))
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        c = torch.randint(0, n_centres, (m,), generator=g, device=dev)
        x[o:o + m] = unit(torch, centres[c] + sigma * torch.randn((m, d), generator=g, device=dev) / d ** 0.5)
    return x, centres


def isotropic(torch, n, d, seed, dev, chunk=1 << 17):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        x[o:o + m] = unit(torch, torch.randn((m, d), generator=g, device=dev))
    return x


def queries(torch, x, centres, nq, sigma, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n, d = x.shape
    half = nq // 2
    rows = torch.randint(0, n, (half,), generator=g, device=dev)
    near_rows = unit(torch, x[rows] + 0.1 * torch.randn((half, d), generator=g, device=dev) / d ** 0.5)
    if centres is None:
        held = unit(torch, torch.randn((nq - half, d), generator=g, device=dev))
    else:
        c = torch.randint(0, centres.shape[0], (nq - half,), generator=g, device=dev)
        held = unit(torch, centres[c] + sigma * torch.randn((nq - half, d), generator=g, device=dev) / d ** 0.5)
    return torch.cat([near_rows, held]).contiguous()


def p50_single(torch, fn, q, reps=120, skip=20):
    lat = []
    for i in range(reps):
        qi = q[i % q.shape[0]:i % q.shape[0] + 1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(qi)
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(lat[skip:])), 4)


def measure(torch, name, x, q, args, dev, save_dir=None):
    from hiprag import HipFlatIndex, HipIVFIndex
    k = 10
    flat = HipFlatIndex(args.dim, "ip", device=dev.index)
    flat.add_device(x)
    truth = flat.search_device(q, k)[2].cpu().numpy()
    flat_p50 = p50_single(torch, lambda qi: flat.search_device(qi, k), q)
    flat.close()
    iv = HipIVFIndex(args.dim, args.nlist, "ip", device=dev.index)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iv.build(x, iters=args.iters, seed=0)
    build_s = time.perf_counter() - t0
    out = {"rows": int(x.shape[0]), "dim": args.dim, "nlist": args.nlist, "iters": args.iters, "queries": int(q.shape[0]),
           "build_s": round(build_s, 3), "build_split_ms": {k_: round(v, 1) for k_, v in iv.build_times().items()},
           "longest_list": int(iv.list_lengths.max()), "shortest_list": int(iv.list_lengths.min()),
           "empty_lists": int((iv.list_lengths == 0).sum()), "flat_p50_ms_single_query": flat_p50}
    if save_dir is not None:
        path = os.path.join(save_dir, f"{name}_hip.index")
        t0 = time.perf_counter()
        iv.save(path)
        out["save_s"] = round(time.perf_counter() - t0, 2)
        out["file_bytes"] = os.path.getsize(path)
        t0 = time.perf_counter()
        jv = HipIVFIndex.load(path, device=dev.index)
        out["load_s"] = round(time.perf_counter() - t0, 2)
        os.remove(path)
        same = all(np.array_equal(a, b) for a, b in zip(iv.lists(), jv.lists())) and np.array_equal(iv.centroids(), jv.centroids())
        out["load_identical"] = bool(same and np.array_equal(iv.search_device(q, k, 8)[2].cpu().numpy(),
                                                             jv.search_device(q, k, 8)[2].cpu().numpy()))
        jv.close()
    half = q.shape[0] // 2
    for nprobe in (1, 8, 32, 128):
        got = iv.search_device(q, k, nprobe)[2].cpu().numpy()
        rec = [len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(got, truth)]
        out[f"nprobe_{nprobe}"] = {"recall_at_10": round(float(np.mean(rec)), 4),
                                   "recall_at_10_row_queries": round(float(np.mean(rec[:half])), 4),
                                   "recall_at_10_held_out_queries": round(float(np.mean(rec[half:])), 4),
                                   "p50_ms_single_query": p50_single(torch, lambda qi: iv.search_device(qi, k, nprobe), q)}
    iv.close()
    return out


def event_ms(torch, fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def measure_batch(torch, x, centres, args, dev):
    from hiprag import HipFlatIndex, HipIVFIndex
    k = 10
    nqs = [int(v) for v in args.batch_nq.split(",")]
    nprobes = [int(v) for v in args.batch_nprobe.split(",")]
    q_all = queries(torch, x, centres, max(nqs), args.sigma, 2025, dev)
    iv = HipIVFIndex(args.dim, args.nlist, "ip", device=dev.index)
    iv.build(x, iters=args.iters, seed=0)
    flat = None
    if not args.batch_only_new:
        flat = HipFlatIndex(args.dim, "ip", device=dev.index)
        flat.add_device(x)
    out = {"rows": int(x.shape[0]), "dim": args.dim, "nlist": args.nlist, "k": k, "metric": "ip",
           "stored_rows": int(iv.lists()[0][-1]), "longest_list": int(iv.list_lengths.max()),
           "timing": "HIP events around one call, median of 5 after 2 warm-up calls (1 warm-up where a call takes > 0.5 s)", "cells": []}

    def triple(nq):
        return (torch.empty((nq, k), dtype=torch.float64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                torch.empty((nq, k), dtype=torch.int64, device=dev))

    for nq in nqs:
        q = q_all[:nq].contiguous()
        o_one, o_bat, o_flat = triple(nq), triple(nq), triple(nq)
        flat_ms = None
        if flat is not None:
            flat_ms, flat_all = event_ms(torch, lambda: flat.search_device(q, k, out=o_flat), 2, 5)
        for nprobe in nprobes:
            cell = {"nq": nq, "nprobe": nprobe}
            bat_ms, bat_all = event_ms(torch, lambda: iv.search_batch_device(q, k, nprobe, out=o_bat), 2, 5)
            info = iv.batch_info()
            cell.update({"batch_ms": round(bat_ms, 3), "batch_ms_all": bat_all, "batch_qps": round(nq / bat_ms * 1e3, 1),
                         "rows_read": info["rows_read"], "rows_read_over_stored": round(info["rows_read"] / out["stored_rows"], 4),
                         "chunks": info["chunks"]})
            if flat is not None:
                iv.search_device(q, k, nprobe, out=o_one)          # the first call also says how long one takes
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                iv.search_device(q, k, nprobe, out=o_one)
                torch.cuda.synchronize()
                slow = time.perf_counter() - t0 > 0.5
                one_ms, one_all = event_ms(torch, lambda: iv.search_device(q, k, nprobe, out=o_one), 0 if slow else 1, 5)
                same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32) if a.dtype == torch.float32 else a,
                                       b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32) if b.dtype == torch.float32 else b)
                           for a, b in zip(o_one, o_bat))
                best_old = max(nq / one_ms * 1e3, nq / flat_ms * 1e3)
                cell.update({"one_query_path_ms": round(one_ms, 3), "one_query_path_ms_all": one_all,
                             "one_query_path_qps": round(nq / one_ms * 1e3, 1), "flat_ms": round(flat_ms, 3), "flat_ms_all": flat_all,
                             "flat_qps": round(nq / flat_ms * 1e3, 1), "identical": bool(same),
                             "batch_over_faster_of_one_query_and_flat": round(nq / bat_ms * 1e3 / best_old, 2)})
            out["cells"].append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    iv.close()
    if flat is not None:
        flat.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--centres", type=int, default=2048)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", action="store_true", help="only the batch-search section (see the header)")
    ap.add_argument("--batch-nq", default="64,1024,16384")
    ap.add_argument("--batch-nprobe", default="1,8,32,128")
    ap.add_argument("--batch-only-new", action="store_true", help="--batch without the two older paths (for a kernel trace)")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/bench_ivf.py", "device": torch.cuda.get_device_name(0),
           "clustered_set": f"{args.centres} centres uniform on the sphere, row = centre + {args.sigma} * g / sqrt(d), renormalised; "
                            f"queries: half rows + 0.1 * g / sqrt(d), half held-out points drawn like the rows"}
    x, centres = clustered(torch, args.rows, args.dim, args.centres, args.sigma, 2024, dev)
    if args.batch:
        res["batch"] = measure_batch(torch, x, centres, args, dev)
        print(json.dumps(res))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    q = queries(torch, x, centres, args.queries, args.sigma, 2025, dev)
    save_dir = tempfile.mkdtemp(prefix="bench_ivf_")
    try:
        res["clustered"] = measure(torch, "clustered", x, q, args, dev, save_dir)
    finally:
        shutil.rmtree(save_dir, ignore_errors=True)
    del x, centres, q
    torch.cuda.empty_cache()
    x = isotropic(torch, args.rows, args.dim, 2026, dev)
    q = queries(torch, x, None, args.queries, args.sigma, 2027, dev)
    res["isotropic"] = measure(torch, "isotropic", x, q, args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
