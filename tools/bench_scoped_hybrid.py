#!/usr/bin/env python3
"""
tools/bench_scoped_hybrid.py -- scoped BM25 (hipbm25_search_scoped_dev) and scoped hybrid search (hiphybrid_search_scoped*)
on one collection of 1M documents: the synthetic postings of bench.py's hybrid leg (BASELINE configs[2]: Zipf over 262 144
terms, 64..319 tokens per document) and 1M x 1024 unit rows, 256 queries per call, depth 50, k 10, one GPU process.  Every
cell sits next to the UNSCOPED entry for the same queries in the same process:

  bm25      one shared contiguous, unaligned scope of 0.5 / 1 / 5 / 25 / 100 % of the documents, and a scope of 100 scattered
            ranges of 1 000 documents: bm25_scoped_ms next to bm25_unscoped_ms (hipbm25_search_dev), work_items from
            hipbm25_scoped_info, and break_even_share -- where the two meet, linearly interpolated between the measured shares.
  hybrid    the same scopes, hybrid_scoped_ms next to hybrid_unscoped_ms (hiphybrid_search_dev), break_even_share; and 256
            queries over 16 distinct scopes of 1 %.
  one_query nq = 1 over a 1 % scope through hiphybrid_search_scoped (host entry, wall clock) next to the per-document path it
            replaces over the documents of that scope: reader search + bm25.search + host rrf_fuse per document.

HIP events around the whole call, median of --steps after --warmup.

    python tools/bench_scoped_hybrid.py [--docs 1000000] [--dim 1024] [--warmup 2] [--steps 7] [--out profiles/scoped_hybrid_1m.json]

torch generates the data and holds the buffers; every search runs in libhiprag.  One JSON line on stdout and in --out.
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

DEPTH, K, V = 50, 10, 262144


def unit_rows(torch, n, d, seed, dev, chunk=1 << 17):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        r = torch.randn((m, d), generator=g, device=dev)
        x[o:o + m] = r / r.norm(dim=1, keepdim=True)
    return x


def synthetic_postings(torch, n, dev):
    """the postings of bench.py's hybrid leg: L_i = 64 + (i * 2654435761 mod 256), terms ~ Zipf(1) over V, seed 777"""
    from hiprag import build_postings
    i = torch.arange(n, dtype=torch.int64, device=dev)
    doc_len = 64 + (i * 2654435761) % 256
    cdf = torch.cumsum(1.0 / torch.arange(1, V + 1, dtype=torch.float64, device=dev), 0)
    cdf /= cdf[-1].clone()
    gt = torch.Generator(device=dev)
    gt.manual_seed(777)
    u = torch.rand(int(doc_len.sum().item()), generator=gt, device=dev, dtype=torch.float64)
    term = torch.clamp(torch.searchsorted(cdf, u), max=V - 1)
    doc = torch.repeat_interleave(i, doc_len)
    return build_postings(doc.cpu().numpy(), term.cpu().numpy(), n, V, doc_len.cpu().numpy())


def sparse_queries(nq, seed=888):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(17, V + 1, dtype=np.float64)           # 6 distinct terms per query, Zipf restricted to ranks >= 16
    cdfq = np.cumsum(w) / w.sum()
    out = []
    for _ in range(nq):
        t = []
        while len(t) < 6:
            c = int(min(np.searchsorted(cdfq, rng.random()), len(cdfq) - 1)) + 16
            if c not in t:
                t.append(c)
        out.append(np.asarray(t, dtype=np.uint32))
    return out


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


def break_even(shares, times, flat):
    pts = [(0.0, 0.0)] + list(zip(shares, times))
    for (s0, t0), (s1, t1) in zip(pts, pts[1:]):
        if t0 <= flat <= t1 and t1 > t0:
            return round(s0 + (s1 - s0) * (flat - t0) / (t1 - t0), 4)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scoped_hybrid_1m.json"))
    args = ap.parse_args()

    import torch
    from hiprag import HipBM25, HipFlatIndex, hybrid_search, hybrid_search_device, hybrid_search_scoped, hybrid_search_scoped_device, rrf_fuse
    dev = torch.device("cuda", 0)
    n, d, nq = args.docs, args.dim, args.batch
    t0 = time.time()
    postings = synthetic_postings(torch, n, dev)
    build_s = time.time() - t0
    bm = HipBM25(postings, device=0)
    x = unit_rows(torch, n, d, 1, dev)
    ix = HipFlatIndex(d, "ip", device=0)
    ix.add_device(x)
    q = unit_rows(torch, nq, d, 2, dev)
    sq = sparse_queries(nq)
    out = {"tool": "bench_scoped_hybrid", "docs": n, "dim": d, "queries": nq, "depth": DEPTH, "k": K, "warmup": args.warmup,
           "steps": args.steps, "device": torch.cuda.get_device_name(0), "postings": int(postings.offsets[-1]),
           "postings_build_s": round(build_s, 1), "tile_docs": bm.scoped_info()["tile_docs"]}
    bufs = (torch.empty((nq, DEPTH), dtype=torch.float64, device=dev), torch.empty((nq, DEPTH), dtype=torch.float32, device=dev),
            torch.empty((nq, DEPTH), dtype=torch.int64, device=dev))

    lo0 = 12345 % max(1, n // 2)
    shares = [0.005, 0.01, 0.05, 0.25, 1.0]
    scopes = {}
    for share in shares:
        rows = max(1, int(n * share))
        scopes[f"scope_{share * 100:g}pct"] = [(lo0, lo0 + rows)] if lo0 + rows <= n and share < 1.0 else [(0, n)]
    scattered = [(lo0 + j * (n - lo0) // 100, lo0 + j * (n - lo0) // 100 + 1000) for j in range(100)
                 if lo0 + j * (n - lo0) // 100 + 1000 <= n]
    scopes["100_ranges_of_1000"] = scattered

    # ---- 1. the BM25 leg ---------------------------------------------------------------------------------------------
    tu = event_ms(torch, lambda: bm.search_device(sq, DEPTH, out=bufs), args.warmup, args.steps)
    leg = {"bm25_unscoped_ms": cell(tu)}
    times = []
    for name, scope in scopes.items():
        t = event_ms(torch, lambda: bm.search_scoped_device(sq, DEPTH, [scope], out=bufs), args.warmup, args.steps)
        info = bm.scoped_info()
        tu_now = event_ms(torch, lambda: bm.search_device(sq, DEPTH, out=bufs), 1, args.steps)    # the unscoped entry again, beside this cell
        leg[name] = {"bm25_scoped_ms": cell(t), "bm25_unscoped_ms": cell(tu_now), "work_items": info["work_items"],
                     "max_scope_tiles": info["max_scope_tiles"], "chunks": info["chunks"], "ranges": len(scope),
                     "documents": int(sum(hi - lo for lo, hi in scope)), "over_unscoped": round(t[0] / tu_now[0], 3)}
        if name.startswith("scope_"):
            times.append(t[0])
    leg["break_even_share"] = break_even(shares, times, tu[0])
    leg["scoped_faster_at_1pct"] = bool(leg["scope_1pct"]["bm25_scoped_ms"]["ms"] < leg["scope_1pct"]["bm25_unscoped_ms"]["ms"])
    leg["ratio_at_100pct"] = leg["scope_100pct"]["over_unscoped"]
    out["bm25"] = leg

    # ---- 2. the hybrid call ----------------------------------------------------------------------------------------------
    th = event_ms(torch, lambda: hybrid_search_device(ix, bm, q, sq, depth=DEPTH, k=K), args.warmup, args.steps)
    hyb = {"hybrid_unscoped_ms": cell(th)}
    times = []
    for name, scope in scopes.items():
        steps = args.steps if name not in ("scope_100pct", "scope_25pct") else max(2, args.steps // 3)
        t = event_ms(torch, lambda: hybrid_search_scoped_device(ix, bm, q, sq, [scope], depth=DEPTH, k=K), min(args.warmup, 1), steps)
        th_now = event_ms(torch, lambda: hybrid_search_device(ix, bm, q, sq, depth=DEPTH, k=K), 1, args.steps)
        hyb[name] = {"hybrid_scoped_ms": cell(t), "hybrid_unscoped_ms": cell(th_now), "over_unscoped": round(t[0] / th_now[0], 3),
                     "dense_chunks": ix.scoped_info()["chunks"]}
        if name.startswith("scope_"):
            times.append(t[0])
    hyb["break_even_share"] = break_even(shares, times, th[0])
    hyb["scoped_faster_at_1pct"] = bool(hyb["scope_1pct"]["hybrid_scoped_ms"]["ms"] < hyb["scope_1pct"]["hybrid_unscoped_ms"]["ms"])
    rows1 = max(1, n // 100)
    sixteen = [[(j * (n // 16) + 77, j * (n // 16) + 77 + rows1)] for j in range(16)]
    soq = (np.arange(nq) % 16).astype(np.int32)
    t = event_ms(torch, lambda: hybrid_search_scoped_device(ix, bm, q, sq, sixteen, soq, depth=DEPTH, k=K), args.warmup, args.steps)
    tb = event_ms(torch, lambda: bm.search_scoped_device(sq, DEPTH, sixteen, soq, out=bufs), args.warmup, args.steps)
    hyb["16_scopes_of_1pct"] = {"hybrid_scoped_ms": cell(t), "bm25_scoped_ms": cell(tb), "work_items": bm.scoped_info()["work_items"],
                                "over_unscoped": round(t[0] / th[0], 3)}
    out["hybrid"] = hyb

    # ---- 3. one query over a 1 % scope, next to the per-document path it replaces ------------------------------------------
    n_docs_scope, per_doc = 10, max(1, rows1 // 10)
    base = lo0
    doc_ranges = [(base + i * per_doc, base + (i + 1) * per_doc) for i in range(n_docs_scope)]
    doc_ix, doc_bm = [], []
    for lo, hi in doc_ranges:
        di = HipFlatIndex(d, "ip", device=0)
        di.add_device(x[lo:hi])
        doc_ix.append(di)
        doc_bm.append(HipBM25(postings.shard(lo, hi), device=0))     # the collection's impacts: same scores as the scoped call
    q1 = q[:1].cpu().numpy()
    sq1 = sq[:1]

    def per_document():
        fused = []
        for i, (lo, _hi) in enumerate(doc_ranges):
            s, ids = doc_ix[i].search(q1, DEPTH)
            bs, bi = doc_bm[i].search(sq1, DEPTH)
            fs, fi = rrf_fuse(ids, bi, K)
            fused += [(-float(v), int(r) + lo) for v, r in zip(fs[0], fi[0]) if r >= 0]
        fused.sort()
        return fused[:K]

    scope1 = [(doc_ranges[0][0], doc_ranges[-1][1])]
    a = wall_ms(torch, per_document, args.warmup, args.steps)
    b = wall_ms(torch, lambda: hybrid_search_scoped(ix, bm, q1, sq1, [scope1], depth=DEPTH, k=K), args.warmup, args.steps)
    c = wall_ms(torch, lambda: hybrid_search(ix, bm, q1, sq1, depth=DEPTH, k=K), args.warmup, args.steps)
    out["one_query"] = {"documents": n_docs_scope, "rows_per_document": per_doc, "per_document_path": cell(a),
                        "hiphybrid_search_scoped": cell(b), "hiphybrid_search_whole_collection": cell(c), "speedup": round(a[0] / b[0], 2),
                        "note": "the per-document path fuses inside each document and merges the fused lists on the host: a different "
                                "ranking than one fusion over the scope, timed for its cost only"}

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
