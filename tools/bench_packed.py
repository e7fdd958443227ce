#!/usr/bin/env python3
"""
tools/bench_packed.py -- the encoder's PACKED entries against the padded ones, in ONE process, in alternation, seeded inputs,
every shape warmed up first, times between HIP events around whole calls, at least five repeats each: the median and beside it
the spread (min, max).  Every cell carries the rows the padded and the packed entry run their GEMMs over; those two are
arithmetic and are written even on a machine without a GPU (the times are then "not measured").

Cells:
  rerank_1m        hiprerank_dev against hiprerank_packed_dev over a store of --docs passages of 60-180 tokens, queries of 8-24
                   tokens, 50 candidates, for 1 and 64 queries (the shapes of profiles/rerank_1m.json).  enqueue_ms is the host
                   wall clock until the call has returned: for the packed entry it contains the call's one synchronise.
  rerank_1m_long   the same store plus ten 500-token passages that no candidate names: the store-wide bound at its worst.
  ingest_10k       10 000 chunks of 60-180 tokens: length-sorted padded batches against packed input-order batches.
  full_256x512     256 x 512 tokens, all full length: nothing to save.
  padded_unchanged (--encoder-runs FILE ...) lines of tools/bench_encoder.py from the parent's library and this one, run in
                   fresh processes by the caller, are copied in and compared: "unchanged" if the difference of the medians is
                   inside the parent's own spread.

    python tools/bench_packed.py [--docs 1000000] [--layers 24] [--repeats 5] [--out profiles/packed_forward.json]
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

DEPTH, MAX_LEN, BATCH_TOKENS = 50, 512, 131072
NOT_MEASURED = "not measured"


def r64(v):
    return -(-np.asarray(v, dtype=np.int64) // 64) * 64


def stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3),
            "repeats": len(v)}


def sorted_padded_rows(lens, max_tokens, batch_size=4096):
    """rows of HipEncoder._run's length-sorted batches"""
    order = sorted(lens, reverse=True)
    rows, o = 0, 0
    while o < len(order):
        s = max(64, int(r64(order[o])))
        take = max(1, min(batch_size, max_tokens // s))
        rows += s * len(order[o:o + take])
        o += take
    return rows


def alternate(run_a, run_b, repeats):
    """(times of a, times of b): one warm-up of each, then a, b, a, b, ... between HIP events"""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = ([], [])
    for step in range(repeats + 1):
        for side, run in enumerate((run_a, run_b)):
            torch.cuda.synchronize()
            ev[0].record()
            run()
            ev[1].record()
            torch.cuda.synchronize()
            if step:
                out[side].append(ev[0].elapsed_time(ev[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--chunks", type=int, default=10_000)
    ap.add_argument("--encoder-runs", nargs="*", default=[], help="files of tools/bench_encoder.py lines, named parent*.json / this*.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    res = {"layers": args.layers, "depth": DEPTH, "max_len": MAX_LEN, "docs": args.docs, "repeats": args.repeats, "gpu": gpu, "cells": []}
    rng = np.random.default_rng(5)
    n = args.docs
    doc_len = rng.integers(60, 181, size=n).astype(np.int64)

    enc = store = None
    if gpu:
        from hiprag import EncoderConfig, HipEncoder, TokenStore, random_state, rerank_device
        cfg = EncoderConfig(layers=args.layers)
        enc = HipEncoder(cfg, random_state(cfg, seed=1, with_head=True), with_head=True)
        store = TokenStore(cfg.vocab, bos=cfg.bos_id, eos=cfg.eos_id, pad=cfg.pad_id, max_doc_tokens=MAX_LEN - 4)
        off_all = np.zeros(n + 1, dtype=np.int64)
        off_all[1:] = np.cumsum(doc_len)
        gen = np.random.default_rng(6)
        for lo in range(0, n, 100_000):
            hi = min(n, lo + 100_000)
            store.append(gen.integers(3, cfg.vocab, size=int(off_all[hi] - off_all[lo])).astype(np.int32), off_all[lo:hi + 1] - off_all[lo])
    vocab = 250002

    # ---- cells 1 and 2: the device rerank ------------------------------------------------------------------------------
    shapes = []
    for nq in args.queries:
        q_len = rng.integers(8, 25, size=nq)
        shapes.append((nq, q_len, [rng.integers(3, vocab, size=int(m)).tolist() for m in q_len], rng.integers(0, n, size=(nq, DEPTH)).astype(np.int64)))
    for name, longest in (("rerank_1m", int(doc_len.max())), ("rerank_1m_long", 500)):
        if name == "rerank_1m_long" and gpu:
            store.append([gen.integers(3, vocab, size=500).tolist() for _ in range(10)])      # ids n .. n + 9: no candidate names them
        for nq, q_len, queries, cand in shapes:
            lens = np.minimum(4 + q_len[:, None] + doc_len[cand], MAX_LEN)
            if gpu:
                longest = store.sizes()[3]
            S = int(r64(min(MAX_LEN, 4 + int(q_len.max()) + longest)))
            cell = {"cell": name, "queries": nq, "pairs": nq * DEPTH, "S_store_wide": S, "padded_rows": nq * DEPTH * S,
                    "packed_rows": int(r64(lens).sum()), "real_tokens": int(lens.sum())}
            cell["rows_packed_over_padded"] = round(cell["packed_rows"] / cell["padded_rows"], 4)
            if gpu:
                cand_dev = torch.from_numpy(cand).cuda()
                keep = {}

                def run(packed):
                    t0 = time.perf_counter()
                    keep[packed] = rerank_device(enc, store, queries, cand_dev, 10, max_len=MAX_LEN, packed=packed)
                    keep[packed, "enqueue"] = (time.perf_counter() - t0) * 1e3
                enq = {False: [], True: []}

                def timed(packed):
                    run(packed)
                    enq[packed].append(keep[packed, "enqueue"])
                t_pad, t_pack = alternate(lambda: timed(False), lambda: timed(True), args.repeats)
                assert store.rerank_info()[2] == S and store.rerank_packed_info()[2] == cell["packed_rows"]
                cell["sub_batches"] = {"padded": store.rerank_info()[3], "packed": store.rerank_packed_info()[3]}
                cell["padded"], cell["packed"] = stats(t_pad), stats(t_pack)
                cell["padded"]["enqueue_ms"] = round(float(np.median(enq[False][1:])), 3)
                cell["packed"]["enqueue_ms"] = round(float(np.median(enq[True][1:])), 3)      # holds the one synchronise
                cell["time_packed_over_padded"] = round(cell["packed"]["median_ms"] / cell["padded"]["median_ms"], 4)
                cell["max_abs_logit_delta"] = float((keep[False][3] - keep[True][3]).abs().max())
            else:
                cell["padded"] = cell["packed"] = NOT_MEASURED
            res["cells"].append(cell)

    # ---- cell 3: the ingest shape -------------------------------------------------------------------------------------------
    c_len = rng.integers(60, 181, size=args.chunks)
    cell = {"cell": "ingest_10k", "chunks": args.chunks, "real_tokens": int(c_len.sum()),
            "padded_rows": sorted_padded_rows(c_len.tolist(), BATCH_TOKENS), "packed_rows": int(r64(c_len).sum())}
    cell["rows_packed_over_padded"] = round(cell["packed_rows"] / cell["padded_rows"], 4)
    if gpu:
        toks = [[0] + rng.integers(3, vocab, size=int(m) - 2).tolist() + [2] for m in c_len]
        t_pad, t_pack = alternate(lambda: enc.encode_tokens(toks, batch_size=4096, max_tokens=BATCH_TOKENS),
                                  lambda: enc.encode_tokens(toks, max_tokens=BATCH_TOKENS, packed=True), args.repeats)
        cell["padded"], cell["packed"] = stats(t_pad), stats(t_pack)
        cell["time_packed_over_padded"] = round(cell["packed"]["median_ms"] / cell["padded"]["median_ms"], 4)
    else:
        cell["padded"] = cell["packed"] = NOT_MEASURED
    res["cells"].append(cell)

    # ---- cell 4: the headline shape: nothing to save ---------------------------------------------------------------------------
    cell = {"cell": "full_256x512", "padded_rows": 256 * 512, "packed_rows": 256 * 512, "real_tokens": 256 * 512, "rows_packed_over_padded": 1.0}
    if gpu:
        toks = [[0] + rng.integers(3, vocab, size=510).tolist() + [2] for _ in range(256)]
        t_pad, t_pack = alternate(lambda: enc.encode_tokens(toks, batch_size=256), lambda: enc.encode_tokens(toks, max_tokens=256 * 512, packed=True),
                                  args.repeats)
        t_pad2, _ = alternate(lambda: enc.encode_tokens(toks, batch_size=256), lambda: None, args.repeats)      # padded against itself
        cell["padded"], cell["packed"], cell["padded_again"] = stats(t_pad), stats(t_pack), stats(t_pad2)
        cell["time_packed_over_padded"] = round(cell["packed"]["median_ms"] / cell["padded"]["median_ms"], 4)
        spread = max(cell["padded"]["max_ms"], cell["padded_again"]["max_ms"]) - min(cell["padded"]["min_ms"], cell["padded_again"]["min_ms"])
        cell["packed_minus_padded_ms"] = round(cell["packed"]["median_ms"] - cell["padded"]["median_ms"], 3)
        cell["padded_spread_ms"] = round(spread, 3)
    else:
        cell["padded"] = cell["packed"] = NOT_MEASURED
    res["cells"].append(cell)

    # ---- the padded path against the parent's library -----------------------------------------------------------------------
    runs = {"parent": [], "this": []}
    for path in args.encoder_runs:
        side = "parent" if os.path.basename(path).startswith("parent") else "this"
        with open(path) as f:
            runs[side] += [json.loads(line) for line in f if line.strip().startswith("{")]
    cell = {"cell": "padded_unchanged", "tool": "tools/bench_encoder.py, fresh processes, alternating"}
    if runs["parent"] and runs["this"]:
        ms = {k: [r["ms_per_batch"] for r in v] for k, v in runs.items()}
        cell["parent_ms_per_batch"], cell["this_ms_per_batch"] = ms["parent"], ms["this"]
        diff = float(np.median(ms["this"]) - np.median(ms["parent"]))
        spread = float(max(ms["parent"]) - min(ms["parent"]))
        cell["median_difference_ms"], cell["parent_spread_ms"] = round(diff, 3), round(spread, 3)
        cell["verdict"] = "unchanged" if abs(diff) <= spread else "CHANGED"
    else:
        cell["verdict"] = NOT_MEASURED
    res["cells"].append(cell)

    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
