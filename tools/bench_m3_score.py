#!/usr/bin/env python3
"""
tools/bench_m3_score.py -- BGE-M3's combined score and its two new parts, each beside the route the parent commit has.  One
MI355X, one process; every time is taken between HIP events around the call, and the two routes of a comparison ALTERNATE
step by step (medians of --steps after a warm-up of both).

Workload: --passages passages at --dim (100 k x 1024-d): a flat inner-product index of unit rows, a multi-vector store of
60-180 unit vectors per passage (about 25 GB) and lexical postings of the same passages (as many distinct term ids per
passage as it has vectors, drawn with a square-law skew from a 250 002-term vocabulary, so lists run from a handful of
postings to tens of thousands); 50 candidates per query; 1 / 64 / 1024 queries of 8-24 terms and vectors.  Per cell:
    score_ids_ms       hipbm25_score_ids_dev, with the library's counts (hipbm25_score_info)
    one_doc_scopes_ms  the only route the parent has to the same numbers: hipbm25_search_scoped_weighted_dev with k = 1 and ONE
                       ONE-DOCUMENT SCOPE PER CANDIDATE (nq x 50 queries over nq x 50 scopes, tables packed outside the timed
                       region; cells of at most --scoped-max queries); same_bits compares the scores of the documents it finds
    m3_ms              hipm3_score_dev
    parts_ms           the same result from the three component calls plus a torch combine and sort
and once: forward_m3_ms beside forward_lexical_ms + forward_colbert_ms (the two forwards a collection that wants both heads
pays without the combined entry) and forward_ms, for 256 x 512 tokens and for one 32-token query.

    python tools/bench_m3_score.py [--passages 100000] [--dim 1024] [--layers 24] [--steps 5] [--out profiles/m3_score_100k.json]
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

DEPTH, LD_MIN, LD_MAX, LQ_MIN, LQ_MAX, BLOCK, VOCAB = 50, 60, 180, 8, 24, 2048, 250002
MIX = (0.4, 0.2, 0.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--scoped-max", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "m3_score_100k.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_m3_score.py measures on the GPU: none is visible")
    from hiprag import (EncoderConfig, HipEncoder, HipFlatIndex, LexicalIndexUpdatable, MultiVectorStore, m3_score_device, maxsim_device,
                        random_state)
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr, pack_scopes
    dev = torch.device("cuda", 0)
    n, dim = args.passages, args.dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev).manual_seed(5)

    def med(v):
        return round(float(np.median(v)), 4)

    def alternate(routes, steps=args.steps, warm=2):
        """{name: fn} -> ({name: median ms}, {name: last result}); the routes take turns inside every step"""
        ms, last = {k: [] for k in routes}, {}
        for i in range(warm + steps):
            for name, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                last[name] = fn()
                b.record()
                b.synchronize()
                if i >= warm:
                    ms[name].append(a.elapsed_time(b))
        return {k: med(v) for k, v in ms.items()}, last

    def skewed_terms(rows, width):
        """[rows, width] strictly ascending term ids, square-law skew towards the low ids"""
        u = torch.rand((rows, width), generator=g, device=dev).sort(dim=1).values
        return ((u * u * (VOCAB - width)).long() + torch.arange(width, device=dev)[None, :]).to(torch.int32)

    # ---- the three structures over the same passages --------------------------------------------------------------------------
    doc_len = rng.integers(LD_MIN, LD_MAX + 1, size=n).astype(np.int32)
    index = HipFlatIndex(dim, "ip", device=0)
    index.reserve_rows(n)
    store = MultiVectorStore(dim, max_doc_vectors=511)
    lex = LexicalIndexUpdatable(n_terms=VOCAB)
    for lo in range(0, n, BLOCK):
        hi = min(n, lo + BLOCK)
        rows = torch.randn((hi - lo, dim), generator=g, device=dev)
        index.add_device(rows / rows.norm(dim=1, keepdim=True))
        block = torch.randn((hi - lo, LD_MAX, dim), generator=g, device=dev)
        store.append_device((block / block.norm(dim=2, keepdim=True)).to(torch.bfloat16), doc_len[lo:hi])
        lens = torch.from_numpy(doc_len[lo:hi]).to(dev)
        terms = skewed_terms(hi - lo, LD_MAX)
        live = torch.arange(LD_MAX, device=dev)[None, :] < lens[:, None]
        weights = torch.rand((hi - lo, LD_MAX), generator=g, device=dev) * 0.3 + 0.01
        lex.append_rows(terms.masked_fill(~live, -1).contiguous(), (weights * live).contiguous(), lens, VOCAB)
        del block
    sizes, lsz = store.sizes(), lex.sizes()
    assert sizes[0] == lsz["n_docs"] == index.ntotal == n
    df = np.diff(lex.export()["offsets"].astype(np.int64))
    res = {"tool": "bench_m3_score", "device": torch.cuda.get_device_name(0), "passages": n, "dim": dim, "depth": DEPTH, "steps": args.steps,
           "stored_vectors": sizes[1], "postings": lsz["postings"], "longest_list": int(df.max()), "lists_ge_2048": int((df >= 2048).sum()),
           "weights": list(MIX), "cells": []}

    # ---- the cells --------------------------------------------------------------------------------------------------------------
    bm = lex.bm
    for nq in args.queries:
        q_len = rng.integers(LQ_MIN, LQ_MAX + 1, size=nq).astype(np.int32)
        q = torch.randn((nq, dim), generator=g, device=dev)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
        qv = torch.randn((nq, LQ_MAX, dim), generator=g, device=dev)
        qv = (qv / qv.norm(dim=2, keepdim=True)).to(torch.bfloat16)
        qc = torch.from_numpy(q_len).to(dev)
        t_all = skewed_terms(nq, LQ_MAX).cpu().numpy()
        terms = [t_all[i, :q_len[i]].tolist() for i in range(nq)]
        tw = [rng.uniform(0.05, 0.4, size=int(v)).astype(np.float32) for v in q_len]
        cand = torch.from_numpy(rng.integers(0, n, size=(nq, DEPTH)).astype(np.int64)).to(dev)
        sbuf = torch.empty((nq, DEPTH), dtype=torch.float32, device=dev)
        routes = {"score_ids": lambda: bm.score_ids_device(terms, cand, tw, out=sbuf)}
        if nq <= args.scoped_max:
            flat = cand.cpu().numpy().reshape(-1)
            scopes = [[(int(d), int(d) + 1)] for d in flat]
            rep_t = [terms[i] for i in range(nq) for _ in range(DEPTH)]
            rep_w = [tw[i] for i in range(nq) for _ in range(DEPTH)]
            ft, fw, fo = bm._flatten_weighted(rep_t, rep_w)
            ranges, offsets, soq = pack_scopes(scopes, None, nq * DEPTH)
            so = (torch.empty((nq * DEPTH, 1), dtype=torch.float32, device=dev), torch.empty((nq * DEPTH, 1), dtype=torch.int64, device=dev))
            routes["one_doc_scopes"] = lambda: nat.call("hipbm25_search_scoped_weighted_dev", bm._h, ft.ctypes.data, fw.ctypes.data,
                                                        fo.ctypes.data, nq * DEPTH, 1, ranges.ctypes.data, offsets.ctypes.data,
                                                        len(offsets) - 1, soq.ctypes.data, None, so[0].data_ptr(), so[1].data_ptr(),
                                                        _stream_ptr())
        ms, _ = alternate(routes)
        info = bm.score_info()
        cell = {"queries": nq, "pairs": nq * DEPTH, "score_ids_ms": ms["score_ids"], "score_ids_info": info,
                "probes_per_s": round(info["probes"] / (ms["score_ids"] * 1e-3))}
        if "one_doc_scopes" in ms:
            torch.cuda.synchronize()
            found = so[1].view(nq, DEPTH) >= 0
            cell.update(one_doc_scopes_ms=ms["one_doc_scopes"], speedup=round(ms["one_doc_scopes"] / ms["score_ids"], 1),
                        found=int(found.sum()),
                        same_bits=bool(torch.equal(so[0].view(nq, DEPTH)[found].view(torch.int32), sbuf[found].view(torch.int32))))

        def parts_route():
            d64, _ = index.score_ids_device(q, cand)
            sp = bm.score_ids_device(terms, cand, tw)
            pair = maxsim_device(store, qv, qc, cand, 1)[3]
            comb = ((MIX[0] * d64 + MIX[1] * sp.double()) + MIX[2] * torch.where(pair == torch.finfo(torch.float32).min, 0.0, pair.double())) / sum(MIX)
            order = torch.sort(comb, dim=1, descending=True, stable=True)
            return order.values[:, :10], order.indices[:, :10]
        ms3, last = alternate({"m3": lambda: m3_score_device(index, bm, store, q, terms, tw, qv, qc, cand, 10, weights=MIX, want_parts=False),
                               "parts": parts_route})
        torch.cuda.synchronize()
        cell.update(m3_ms=ms3["m3"], parts_ms=ms3["parts"], parts_over_m3=round(ms3["parts"] / ms3["m3"], 2),
                    same_order=bool(torch.equal(last["m3"]["pos"].long(), last["parts"][1])))
        res["cells"].append(cell)

    # ---- one forward for three outputs beside two forwards for two ------------------------------------------------------------------
    cfg = EncoderConfig(layers=args.layers, hidden=dim, heads=dim // 64, ffn=4 * dim)
    enc = HipEncoder(cfg, random_state(cfg, seed=1))
    gh = torch.Generator().manual_seed(2)
    enc.set_colbert_head(torch.randn(dim, dim, generator=gh) * 0.02, torch.randn(dim, generator=gh) * 0.02)
    enc.set_lexical_head(torch.randn(dim, generator=gh) * 0.02, torch.randn(1, generator=gh) * 0.02, (cfg.bos_id, cfg.pad_id, cfg.eos_id, 3))
    res["forward"] = {}
    for name, nseq, L in (("batch_256x512", 256, 512), ("one_query_32", 1, 32)):
        ids = rng.integers(4, cfg.vocab, size=(nseq, L)).astype(np.int32)
        ids[:, 0], ids[:, -1] = cfg.bos_id, cfg.eos_id
        lens = np.full(nseq, L, dtype=np.int32)
        dense = torch.empty((nseq, dim), dtype=torch.float32, device=dev)
        vecs = torch.empty((2, nseq, L - 1, dim), dtype=torch.bfloat16, device=dev)
        cnt = torch.empty((2, nseq), dtype=torch.int32, device=dev)
        lt = torch.empty((2, nseq, L), dtype=torch.int32, device=dev)
        lw = torch.empty((2, nseq, L), dtype=torch.float32, device=dev)
        lc = torch.empty((2, nseq), dtype=torch.int32, device=dev)
        a = (enc._h, ids.ctypes.data, lens.ctypes.data, nseq, L, dense.data_ptr())
        st = _stream_ptr()
        ms, _ = alternate({
            "forward": lambda: nat.call("hipenc_forward", *a, st),
            "lexical": lambda: nat.call("hipenc_forward_lexical", *a, lt[0].data_ptr(), lw[0].data_ptr(), lc[0].data_ptr(), st),
            "colbert": lambda: nat.call("hipenc_forward_colbert", *a, vecs[0].data_ptr(), cnt[0].data_ptr(), st),
            "m3": lambda: nat.call("hipenc_forward_m3", *a, lt[1].data_ptr(), lw[1].data_ptr(), lc[1].data_ptr(), vecs[1].data_ptr(),
                                   cnt[1].data_ptr(), st)})
        torch.cuda.synchronize()
        assert torch.equal(lt[0], lt[1]) and torch.equal(lw[0], lw[1]) and torch.equal(vecs[0].view(torch.int16), vecs[1].view(torch.int16))
        two = ms["lexical"] + ms["colbert"]
        res["forward"][name] = {"forward_ms": ms["forward"], "forward_lexical_ms": ms["lexical"], "forward_colbert_ms": ms["colbert"],
                                "forward_m3_ms": ms["m3"], "two_forwards_ms": round(two, 4), "two_over_m3": round(two / ms["m3"], 3),
                                "m3_over_forward": round(ms["m3"] / ms["forward"], 4)}
        del vecs
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
