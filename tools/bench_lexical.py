#!/usr/bin/env python3
"""Measurements of the lexical leg; writes profiles/lexical_1m.json.

(a) cost of the lexical head: hipenc_forward_lexical against hipenc_forward on XLM-R large (random weights), at 256 x 512
    tokens and at one 32-token query; HIP events around each call, median of --iters.
(b) weighted against unweighted sparse search: the collection of tools/bench_hybrid.py (1M documents, Zipf terms), its
    256 six-term queries, k = 50; median of --iters.
(c) with --parent-lib PATH (a libhiprag.so built from the parent commit): tools/bench_hybrid.py's BM25-alone figure -- the
    same postings, queries, depth and timing loop -- measured in fresh child processes that load the parent's library and
    this tree's in turn, --ab-runs each.  The unweighted kernels share a template with the weighted ones; this is the check
    that they do not pay for it: the median here must not fall below the parent's lowest run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "intool-rag_amd"))


def event_ms(fn, iters):
    """median and all timings (ms) of fn() between two HIP events on the current stream, after one warm-up call"""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), [round(x, 4) for x in out]


def bench_head(layers, iters):
    import torch
    from hiprag import EncoderConfig, HipEncoder, _native as nat, random_state
    from hiprag.index import _stream_ptr
    import torch
    cfg = EncoderConfig(layers=layers)
    sd = random_state(cfg, seed=0, with_lexical=True)
    # random deep weights give the tokens of a batch similar hidden rows, hence mostly one sign of the lexical dot -- with the
    # seeded bias no token of this batch has a positive weight; a bias of 1 keeps most of them, so the head writes full rows
    sd["sparse_linear.bias"] = torch.ones(1)
    enc = HipEncoder(cfg, sd)
    rng = np.random.default_rng(0)
    res = {}
    for name, bs, seq in (("batch_256x512", 256, 512), ("query_1x32", 1, 32)):
        toks = [[0] + rng.integers(4, cfg.vocab, size=seq - 2).tolist() + [2] for _ in range(bs)]
        ids, lens, max_len = enc._pad(toks)
        dense = torch.empty((bs, cfg.hidden), dtype=torch.float32, device="cuda")
        terms = torch.empty((bs, max_len), dtype=torch.int32, device="cuda")
        weights = torch.empty((bs, max_len), dtype=torch.float32, device="cuda")
        counts = torch.empty((bs,), dtype=torch.int32, device="cuda")

        def plain():
            nat.call("hipenc_forward", enc._h, ids.ctypes.data, lens.ctypes.data, bs, max_len, dense.data_ptr(), _stream_ptr())

        def lexical():
            nat.call("hipenc_forward_lexical", enc._h, ids.ctypes.data, lens.ctypes.data, bs, max_len, dense.data_ptr(), terms.data_ptr(),
                     weights.data_ptr(), counts.data_ptr(), _stream_ptr())

        p_ms, p_all = event_ms(plain, iters)
        l_ms, l_all = event_ms(lexical, iters)
        res[name] = {"forward_ms": round(p_ms, 4), "forward_lexical_ms": round(l_ms, 4), "head_ms": round(l_ms - p_ms, 4),
                     "head_share": round((l_ms - p_ms) / p_ms, 5), "forward_ms_runs": p_all, "forward_lexical_ms_runs": l_all,
                     "mean_terms_per_sequence": round(float(counts.float().mean().item()), 1)}
    enc.close()
    return {"model": f"XLM-R large shape, {layers} layers, random weights", "timing": "HIP events, median", **res}


def hybrid_postings(N, V):
    """the collection of tools/bench_hybrid.py, statement for statement"""
    import torch
    from hiprag import build_postings
    dev = torch.device("cuda", 0)
    i = torch.arange(N, dtype=torch.int64, device=dev)
    doc_len = 64 + (i * 2654435761) % 256
    cdf = torch.cumsum(1.0 / torch.arange(1, V + 1, dtype=torch.float64, device=dev), 0)
    cdf /= cdf[-1].clone()
    gt = torch.Generator(device=dev)
    gt.manual_seed(777)
    total = int(doc_len.sum().item())
    u = torch.rand(total, generator=gt, device=dev, dtype=torch.float64)
    term = torch.clamp(torch.searchsorted(cdf, u), max=V - 1)
    doc = torch.repeat_interleave(i, doc_len)
    return build_postings(doc.cpu().numpy(), term.cpu().numpy(), N, V, doc_len.cpu().numpy())


def wall_qps(fn, nq, reps=5):
    """tools/bench_hybrid.py's timeit: one warm-up, then `reps` calls between two synchronisations"""
    import torch
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return nq / ((time.perf_counter() - t) / reps)


def child_bm25(npz, nq, depth):
    """one fresh process, whatever library HIPRAG_LIB names: the BM25-alone figure"""
    import ctypes
    import torch
    torch.cuda.init()      # torch's HIP runtime first, as in every other tool here: the library then binds to the one already loaded
    from hiprag import HipBM25, PostingsCSR, _native
    from oracle import hybrid_oracle as ho
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in [n for n in _native.SIGNATURES if not hasattr(lib, n)]:
        del _native.SIGNATURES[name]          # the parent's library lacks the entries this change adds; none is called here
    with np.load(npz) as z:
        p = PostingsCSR(int(z["n_docs"]), int(z["offsets"].shape[0] - 1), z["offsets"], z["doc_ids"], z["impacts"])
    bm = HipBM25(p)
    sparse_q = ho.synthetic_sparse_queries(nq, n_terms=p.n_terms, terms_per_query=6, seed=888, min_rank=16)
    print(json.dumps({"lib": _native.LIB_PATH, "bm25_qps": round(wall_qps(lambda: bm.search_device(sparse_q, depth), nq), 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=262144)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libhiprag.so of the parent commit: adds the alternating BM25-alone runs")
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-head", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lexical_1m.json"))
    ap.add_argument("--child-bm25", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_bm25:
        return child_bm25(args.child_bm25, args.nq, args.depth)

    import torch
    from hiprag import HipBM25, _native
    from oracle import hybrid_oracle as ho
    result = {"device": torch.cuda.get_device_name(0), "docs": args.docs, "terms": args.terms, "nq": args.nq, "k": args.depth}
    if not args.skip_head:
        result["head_cost"] = bench_head(args.layers, args.iters)
        print(json.dumps({"head_cost": result["head_cost"]}), flush=True)
        torch.cuda.empty_cache()

    p = hybrid_postings(args.docs, args.terms)
    bm = HipBM25(p)
    sparse_q = ho.synthetic_sparse_queries(args.nq, n_terms=args.terms, terms_per_query=6, seed=888, min_rank=16)
    rng = np.random.default_rng(5)
    sparse_w = [rng.uniform(0.1, 2.0, size=len(q)).astype(np.float32) for q in sparse_q]
    # the C entries alone: queries flattened once, outputs allocated once (the Python wrappers' flattening is host time of its own)
    from hiprag.index import _stream_ptr
    terms, wts, qoff = bm._flatten_weighted(sparse_q, sparse_w)
    out = bm.search_device(sparse_q, args.depth)
    tail = (qoff.ctypes.data, args.nq, args.depth, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream_ptr())
    un_ms, un_all = event_ms(lambda: _native.call("hipbm25_search_dev", bm._h, terms.ctypes.data, *tail), args.iters)
    we_ms, we_all = event_ms(lambda: _native.call("hipbm25_search_weighted_dev", bm._h, terms.ctypes.data, wts.ctypes.data, *tail), args.iters)
    wrap_un_ms, _ = event_ms(lambda: bm.search_device(sparse_q, args.depth), args.iters)
    wrap_we_ms, _ = event_ms(lambda: bm.search_weighted_device(sparse_q, sparse_w, args.depth), args.iters)
    ones = [np.ones(len(q), np.float32) for q in sparse_q]
    same = all(torch.equal(a, b) for a, b in zip(bm.search_device(sparse_q, args.depth), bm.search_weighted_device(sparse_q, ones, args.depth)))
    result["weighted_vs_unweighted"] = {
        "postings": int(p.offsets[-1]), "terms_per_query": 6, "timing": "HIP events around the C entry (its host planning included), median",
        "unweighted_ms": round(un_ms, 4), "weighted_ms": round(we_ms, 4), "unweighted_qps": round(args.nq / un_ms * 1e3, 1),
        "weighted_qps": round(args.nq / we_ms * 1e3, 1), "weighted_over_unweighted": round(we_ms / un_ms, 4),
        "unweighted_ms_runs": un_all, "weighted_ms_runs": we_all,
        "python_wrapper_ms": {"search_device": round(wrap_un_ms, 4), "search_weighted_device": round(wrap_we_ms, 4)}, "unit_weights_equal_unweighted_bits": bool(same)}
    print(json.dumps({"weighted_vs_unweighted": result["weighted_vs_unweighted"]}), flush=True)
    bm.close()

    if args.parent_lib:
        with tempfile.TemporaryDirectory() as tmp:
            npz = os.path.join(tmp, "postings.npz")
            with open(npz, "wb") as f:
                np.savez(f, offsets=p.offsets, doc_ids=p.doc_ids, impacts=p.impacts, n_docs=np.int64(p.n_docs))
            del p
            runs = {"parent": [], "this": []}
            for _ in range(args.ab_runs):
                for who, lib in (("parent", os.path.abspath(args.parent_lib)), ("this", _native.LIB_PATH)):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-bm25", npz, "--nq", str(args.nq), "--depth",
                                          str(args.depth)], env=dict(os.environ, HIPRAG_LIB=lib), capture_output=True, text=True, timeout=600)
                    if out.returncode != 0:
                        raise SystemExit(f"the {who} child failed ({out.returncode}):\n{out.stderr[-2000:]}")
                    runs[who].append(json.loads(out.stdout.strip().splitlines()[-1])["bm25_qps"])
            result["unweighted_bm25_alone"] = {
                "what": "tools/bench_hybrid.py's bm25_qps (same postings, queries, depth 50, 5 calls between two synchronisations), fresh "
                        "processes alternating between the parent's library and this tree's",
                "parent_qps": runs["parent"], "this_qps": runs["this"], "parent_lowest": min(runs["parent"]),
                "this_median": statistics.median(runs["this"]),
                "not_below_the_parents_lowest_run": bool(statistics.median(runs["this"]) >= min(runs["parent"]))}
            print(json.dumps({"unweighted_bm25_alone": result["unweighted_bm25_alone"]}), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
