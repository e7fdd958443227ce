#!/usr/bin/env python3
"""
tools/bench_rerank.py -- the device rerank call (hiprerank_dev over a passage token store) against today's host path
(CrossEncoderReranker.score: tokenise every candidate text, pad, score_tokens) in ONE process, in alternation, on the
24-layer encoder with seeded weights.  Shapes: 1 and 64 queries x 50 candidates over a store of 1M passages of 60-180
tokens; queries of 8-24 tokens.

Per shape and side, medians over --steps:
    device   enqueue_ms   host wall clock until hiprerank_dev has returned: query tokenisation included, everything enqueued,
                          nothing waited for -- the host's whole share of the call
             gpu_ms       HIP events around the call on its stream (assembly, every sub-batch's forward, selection)
             wall_ms      until the results are on the host
    host     tokenise_ms  encode_pair over the candidate texts: host time before anything can be staged
             score_ms     score_tokens behind it: pad + stage + forward + copy back, synchronous (the GPU idles while the
                          host pads the next sub-batch; that is part of today's path)
             wall_ms      CrossEncoderReranker.score per query, summed over the queries of the shape
Both sides score the same pairs: the bench tokenizer maps the word "t<id>" to <id>, the candidate texts are printed from the
stored ids, and the two sides' logits are compared (max |delta| is reported; it must stay within 1.5e-2).  A dictionary
lookup per word is a LOWER bound on a real tokenizer's cost, so the host side is not handicapped.
padded_share = sum of pair lengths / (pairs x S): under the store-wide bound S of hiprerank_dev and under the tight bound of
the host entry (the longest candidate of the call).

    python tools/bench_rerank.py [--docs 1000000] [--layers 24] [--steps 5] [--out profiles/rerank_1m.json]
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

DEPTH, MAX_LEN = 50, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("HIP_ALLOW_SYNTHETIC", "1")
    import torch
    from hiprag import EncoderConfig, HipEncoder, TokenStore, random_state, rerank, rerank_device
    from hiprag.rerank import seq_len_bound
    from rag.providers.hip.tokenizer import HashTokenizer
    from rag.query.reranker import CrossEncoderReranker

    class IdTokenizer(HashTokenizer):
        """the word "t<id>" is token <id>: both sides of the bench then score the same pairs"""

        def _id(self, tok):
            hit = self._memo.get(tok)
            if hit is None:
                hit = self._memo[tok] = int(tok[1:])
            return hit

    cfg = EncoderConfig(layers=args.layers)
    enc = HipEncoder(cfg, random_state(cfg, seed=1, with_head=True), with_head=True)
    tok = IdTokenizer(cfg.vocab)
    rr = CrossEncoderReranker(encoder=enc, tokenizer=tok)

    n = args.docs
    rng = np.random.default_rng(5)
    doc_len = rng.integers(60, 181, size=n).astype(np.int64)
    store = TokenStore(cfg.vocab, bos=cfg.bos_id, eos=cfg.eos_id, pad=cfg.pad_id, max_doc_tokens=MAX_LEN - 4)
    t0 = time.perf_counter()
    off_all = np.zeros(n + 1, dtype=np.int64)
    off_all[1:] = np.cumsum(doc_len)
    starts = {}
    for lo in range(0, n, 100_000):
        hi = min(n, lo + 100_000)
        tokens = rng.integers(3, cfg.vocab, size=int(off_all[hi] - off_all[lo])).astype(np.int32)
        starts[lo] = tokens
        store.append(tokens, off_all[lo:hi + 1] - off_all[lo])
    build_ms = (time.perf_counter() - t0) * 1e3
    sizes = store.sizes()
    res = {"docs": n, "stored_tokens": sizes[1], "longest_doc": sizes[3], "depth": DEPTH, "max_len": MAX_LEN, "layers": args.layers,
           "steps": args.steps, "store_append_ms": round(build_ms, 1), "shapes": []}

    def body(row):
        lo = row // 100_000 * 100_000
        a = off_all[row] - off_all[lo]
        return starts[lo][a:a + doc_len[row]]

    def med(v):
        return round(float(np.median(v)), 3)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for nq in args.queries:
        q_words = [" ".join(f"t{v}" for v in rng.integers(3, cfg.vocab, size=int(rng.integers(8, 25)))) for _ in range(nq)]
        cand = rng.integers(0, n, size=(nq, DEPTH)).astype(np.int64)
        texts = [[" ".join(f"t{v}" for v in body(int(r))) for r in cand[q]] for q in range(nq)]
        cand_dev = torch.from_numpy(cand).cuda()
        t = {k: [] for k in ("dev_enqueue", "dev_gpu", "dev_wall", "host_tokenise", "host_score", "host_wall")}
        dev_logits = host_logits = None
        for step in range(args.steps + 1):                 # step 0 warms both sides (workspaces, staging, the tokenizer's memo)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            queries = [tok.encode(q.replace("\n", " "), MAX_LEN + 2)[1:-1] for q in q_words]
            ev[0].record()
            out = rerank_device(enc, store, queries, cand_dev, 10, max_len=MAX_LEN)
            ev[1].record()
            t1 = time.perf_counter()
            ids = out[1].cpu()
            dev_logits = out[3].cpu().numpy()
            t2 = time.perf_counter()
            # today's path, query by query; then its two parts apart
            t3 = time.perf_counter()
            host_logits = np.asarray([rr.score(q_words[q], texts[q]) for q in range(nq)], dtype=np.float32)
            t4 = time.perf_counter()
            pairs = [[tok.encode_pair(q_words[q].replace("\n", " "), p.replace("\n", " "), MAX_LEN) for p in texts[q]] for q in range(nq)]
            t5 = time.perf_counter()
            for q in range(nq):
                enc.score_tokens(pairs[q], batch_size=4096, max_tokens=256 * 512).cpu()
            t6 = time.perf_counter()
            if step:
                t["dev_enqueue"].append((t1 - t0) * 1e3)
                t["dev_gpu"].append(ev[0].elapsed_time(ev[1]))
                t["dev_wall"].append((t2 - t0) * 1e3)
                t["host_wall"].append((t4 - t3) * 1e3)
                t["host_tokenise"].append((t5 - t4) * 1e3)
                t["host_score"].append((t6 - t5) * 1e3)
            del ids
        info = store.rerank_info()
        lq = np.asarray([len(q.split()) for q in q_words])
        lens = np.minimum(4 + lq[:, None] + doc_len[cand], MAX_LEN)
        S_store = seq_len_bound(MAX_LEN, lq.max(), sizes[3])
        S_tight = seq_len_bound(MAX_LEN, lq.max(), doc_len[cand].max())
        assert info[2] == S_store, (info, S_store)
        rerank(enc, store, [tok.encode(q, MAX_LEN + 2)[1:-1] for q in q_words], cand, 10, max_len=MAX_LEN)
        assert store.rerank_info()[2] == S_tight
        delta = float(np.abs(dev_logits - host_logits).max())
        assert delta <= 1.5e-2, delta
        shape = {"queries": nq, "pairs": nq * DEPTH, "S_store_wide": S_store, "S_tight": S_tight, "sub_batches": info[3],
                 "padded_share_store_wide": round(float(lens.sum()) / (lens.size * S_store), 4),
                 "padded_share_tight": round(float(lens.sum()) / (lens.size * S_tight), 4),
                 "max_abs_logit_delta_between_sides": delta,
                 "device": {"enqueue_ms": med(t["dev_enqueue"]), "gpu_ms": med(t["dev_gpu"]), "wall_ms": med(t["dev_wall"])},
                 "host": {"tokenise_ms": med(t["host_tokenise"]), "score_ms": med(t["host_score"]), "wall_ms": med(t["host_wall"])}}
        shape["host_ms_per_query"] = {"device": round(shape["device"]["enqueue_ms"] / nq, 4), "host": round(shape["host"]["tokenise_ms"] / nq, 4)}
        shape["wall_host_over_device"] = round(shape["host"]["wall_ms"] / shape["device"]["wall_ms"], 3)
        res["shapes"].append(shape)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
