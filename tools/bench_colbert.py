#!/usr/bin/env python3
"""
tools/bench_colbert.py -- late interaction (hipmaxsim_dev over a multi-vector store) beside the two second stages it stands
next to, the time the ColBERT head adds to a forward, and the store's append and removal rates.  One MI355X; every time is
taken between HIP events around the call (medians of --steps after a warm-up of every shape).

Workload: --passages passages of 60-180 stored vectors at --dim (100 k x 1024-d: about 25 GB), unit vectors; 50 candidates per
query; 1 / 64 / 1024 queries of 8-24 vectors.  Per cell:
    maxsim_ms        hipmaxsim_dev, selection included
    vectors_read     document vectors read (hipmaxsim_info), their bytes per second beside the 5.5-5.8 TB/s that gathers of
                     rows of this size reach on this GPU
    einsum_ms        the obvious form without a kernel: the candidates' vectors gathered into a padded [pairs, 180, dim]
                     block, torch.einsum + amax + masked mean, 64 queries at a time; the bits differ, the values are compared
    rerank_ms        hiprerank_dev on the same candidate ids over a token store of the same lengths (--layers layers; cells
                     of at most --rerank-max queries; csrc/rerank.hip is the parent's code, so this is the parent's second stage)
and once: forward_ms / forward_colbert_ms for 256 x 512 tokens and for one 32-token query (same encoder, same library),
store_append (documents and vectors per second through hipmv_append_dev), store_remove_ms for a range at the front (every
vector behind it moves).

    python tools/bench_colbert.py [--passages 100000] [--dim 1024] [--layers 24] [--steps 5] [--out profiles/colbert_100k.json]
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

DEPTH, LD_MIN, LD_MAX, LQ_MIN, LQ_MAX, BLOCK = 50, 60, 180, 8, 24, 2048
GATHER_TBPS = (5.5, 5.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--rerank-max", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_colbert.py measures on the GPU: none is visible")
    from hiprag import (EncoderConfig, HipEncoder, MultiVectorStore, TokenStore, maxsim_device, random_state, rerank_device)
    from hiprag.index import _stream_ptr
    from hiprag import _native as nat
    dev = torch.device("cuda", 0)
    n, dim = args.passages, args.dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev).manual_seed(5)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def med(v):
        return round(float(np.median(v)), 4)

    def timed(fn, steps=args.steps, warm=2):
        out = []
        for i in range(warm + steps):
            ev[0].record()
            r = fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warm:
                out.append(ev[0].elapsed_time(ev[1]))
        return med(out), r

    # ---- the store, and a packed copy of its vectors for the einsum form ---------------------------------------------------
    doc_len = rng.integers(LD_MIN, LD_MAX + 1, size=n).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(doc_len)
    store = MultiVectorStore(dim, max_doc_vectors=511)
    packed = torch.empty((int(off[-1]), dim), dtype=torch.bfloat16, device=dev)
    append_s = 0.0
    for lo in range(0, n, BLOCK):
        hi = min(n, lo + BLOCK)
        block = torch.randn((hi - lo, LD_MAX, dim), generator=g, device=dev)
        block = (block / block.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        lens = torch.from_numpy(doc_len[lo:hi]).to(dev)
        packed[int(off[lo]):int(off[hi])] = block[torch.arange(LD_MAX, device=dev)[None, :] < lens[:, None]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.append_device(block, doc_len[lo:hi].astype(np.int32))      # synchronous
        append_s += time.perf_counter() - t0
        del block
    sizes = store.sizes()
    assert sizes[:2] == (n, int(off[-1]))
    off_dev = torch.from_numpy(off).to(dev)
    res = {"passages": n, "dim": dim, "stored_vectors": sizes[1], "store_gb": round(sizes[1] * dim * 2 / 1e9, 2), "depth": DEPTH,
           "steps": args.steps, "guide_gather_tbps": list(GATHER_TBPS),
           "store_append": {"seconds": round(append_s, 3), "docs_per_s": round(n / append_s, 1),
                            "vectors_per_s": round(sizes[1] / append_s, 1), "gb_per_s": round(sizes[1] * dim * 2 / 1e9 / append_s, 2)},
           "cells": []}

    # ---- the encoder: what the head adds, and the rerank side ----------------------------------------------------------------
    cfg = EncoderConfig(layers=args.layers, hidden=dim, heads=dim // 64, ffn=4 * dim)
    sd = random_state(cfg, seed=1, with_head=True)
    enc = HipEncoder(cfg, sd, with_head=True)
    gh = torch.Generator().manual_seed(2)
    enc.set_colbert_head(torch.randn(dim, dim, generator=gh) * 0.02, torch.randn(dim, generator=gh) * 0.02)
    head = {}
    for name, nseq, L in (("batch_256x512", 256, 512), ("one_query_32", 1, 32)):
        ids = rng.integers(3, cfg.vocab, size=(nseq, L)).astype(np.int32)
        ids[:, 0], ids[:, -1] = cfg.bos_id, cfg.eos_id
        lens = np.full(nseq, L, dtype=np.int32)
        dense = torch.empty((nseq, dim), dtype=torch.float32, device=dev)
        vecs = torch.empty((nseq, L - 1, dim), dtype=torch.bfloat16, device=dev)
        cnt = torch.empty((nseq,), dtype=torch.int32, device=dev)
        plain, _ = timed(lambda: nat.call("hipenc_forward", enc._h, ids.ctypes.data, lens.ctypes.data, nseq, L, dense.data_ptr(), _stream_ptr()))
        keep = dense.clone()
        withh, _ = timed(lambda: nat.call("hipenc_forward_colbert", enc._h, ids.ctypes.data, lens.ctypes.data, nseq, L, dense.data_ptr(),
                                          vecs.data_ptr(), cnt.data_ptr(), _stream_ptr()))
        assert torch.equal(keep, dense) and int(cnt.min()) == L - 1
        head[name] = {"forward_ms": plain, "forward_colbert_ms": withh, "added_ms": round(withh - plain, 4),
                      "added_share": round((withh - plain) / plain, 4)}
        del vecs
    res["head"] = head

    tstore = TokenStore(cfg.vocab, bos=cfg.bos_id, eos=cfg.eos_id, pad=cfg.pad_id, max_doc_tokens=508)
    for lo in range(0, n, 100_000):
        hi = min(n, lo + 100_000)
        tstore.append(rng.integers(3, cfg.vocab, size=int(off[hi] - off[lo])).astype(np.int32), off[lo:hi + 1] - off[lo])

    # ---- the cells ------------------------------------------------------------------------------------------------------------
    for nq in args.queries:
        q_len = rng.integers(LQ_MIN, LQ_MAX + 1, size=nq).astype(np.int32)
        q = torch.randn((nq, LQ_MAX, dim), generator=g, device=dev)
        q = (q / q.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        qc = torch.from_numpy(q_len).to(dev)
        cand = rng.integers(0, n, size=(nq, DEPTH)).astype(np.int64)
        cand_dev = torch.from_numpy(cand).to(dev)
        ms, out = timed(lambda: maxsim_device(store, q, qc, cand_dev, 10))
        info = store.maxsim_info()
        reads = int(doc_len[cand].sum())                                   # every query has at most 32 vectors: one tile
        assert info == (nq * DEPTH, 0, reads, 0), (info, reads)
        pair_scores = out[3]

        def einsum_form():
            parts = []
            for a in range(0, nq, 64):
                c = cand_dev[a:a + 64]
                rows = off_dev[c][:, :, None] + torch.arange(LD_MAX, device=dev)[None, None, :]
                live = torch.arange(LD_MAX, device=dev)[None, None, :] < (off_dev[c + 1] - off_dev[c])[:, :, None]
                d = packed[torch.where(live, rows, off_dev[c][:, :, None])]          # [b, depth, LD_MAX, dim]; dead rows repeat a live one
                s = torch.einsum("bid,bcjd->bcij", q[a:a + 64].float(), d.float()).amax(dim=3)     # [b, depth, LQ_MAX]
                qm = torch.arange(LQ_MAX, device=dev)[None, None, :] < qc[a:a + 64, None, None]
                parts.append((s * qm).sum(dim=2) / qc[a:a + 64, None])
            return torch.cat(parts)
        e_ms, e_scores = timed(einsum_form, warm=1)
        delta = float((e_scores - pair_scores).abs().max())
        assert delta < 1e-4, delta
        cell = {"queries": nq, "pairs": nq * DEPTH, "maxsim_ms": ms, "einsum_ms": e_ms, "einsum_over_maxsim": round(e_ms / ms, 2),
                "max_abs_score_delta": delta, "vectors_read": reads, "bytes_read": reads * dim * 2,
                "read_tbps": round(reads * dim * 2 / (ms * 1e-3) / 1e12, 3), "queries_per_s": round(nq / (ms * 1e-3), 1)}
        if nq <= args.rerank_max:
            queries = [rng.integers(3, cfg.vocab, size=int(v)).tolist() for v in q_len]
            r_ms, _ = timed(lambda: rerank_device(enc, tstore, queries, cand_dev, 10, max_len=512), warm=1)
            cell["rerank_ms"] = r_ms
            cell["rerank_over_maxsim"] = round(r_ms / ms, 1)
        res["cells"].append(cell)

    # ---- a removal at the front: every vector behind it moves -----------------------------------------------------------------
    gone = min(1000, n // 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store.remove_ranges([(0, gone)])
    rm = time.perf_counter() - t0
    moved = int(off[-1] - off[gone])
    assert store.sizes()[:2] == (n - gone, moved)
    res["store_remove"] = {"removed_docs": gone, "moved_vectors": moved, "ms": round(rm * 1e3, 2),
                           "moved_gb_per_s": round(moved * dim * 2 / 1e9 / rm, 2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
