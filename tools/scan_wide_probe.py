#!/usr/bin/env python3
"""
Where the wide scan kernel starts to pay: one launch at a time (hipidx_search_dev, scan + finish, no pipelining) on a
synthetic 1M x 1024 index, for nq in NQS, through two indexes over the same rows -- one created under HIPRAG_SCAN_WIDE=0
(scan_bf16_kernel for every launch) and one under HIPRAG_SCAN_WIDE=1 (scan_wide_kernel for every launch of more than 64
queries).  One JSON line per nq: ms per launch of either kernel, candidate-list entries per query, and whether the ids
agree.  The threshold DenseIndex::kWideMinQ comes from this table.  ROWS / NQS / SPARE from the environment.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "intool-rag_amd"))


def main():
    import torch
    from hiprag import HipFlatIndex
    dev = torch.device("cuda", 0)
    rows, d, k = int(os.environ.get("ROWS", 1_000_000)), 1024, 10
    nqs = [int(v) for v in os.environ.get("NQS", "128,192,256,384,512").split(",")]
    os.environ["HIPRAG_LAUNCH_QUERIES"] = "1024"     # every nq of the table is one launch
    idx = {}
    for wide in ("0", "1"):
        os.environ["HIPRAG_SCAN_WIDE"] = wide
        ix = HipFlatIndex(d, "ip")
        ix.reserve_rows(rows)
        for c in range(0, rows, 125000):
            g = torch.Generator(device=dev)
            g.manual_seed(1234 + c // 125000)
            x = torch.randn((min(125000, rows - c), d), generator=g, device=dev)
            x /= x.norm(dim=1, keepdim=True)
            ix.add_device(x)
        del x
        ix.set_spare_cus(int(os.environ.get("SPARE", 0)))
        idx[wide] = ix
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    queries = torch.randn((max(nqs), d), generator=g, device=dev)
    queries /= queries.norm(dim=1, keepdim=True)
    for nq in nqs:
        q = queries[:nq]
        line = {"rows": rows, "nq": nq}
        ids = {}
        for wide, ix in idx.items():
            out = None
            for _ in range(3):
                out = ix.search_device(q, k, out)
            torch.cuda.synchronize()
            s0 = ix.stats()
            t0 = time.perf_counter()
            n = 20
            for _ in range(n):
                ix.search_device(q, k, out)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            s1 = ix.stats()
            tag = "wide" if wide == "1" else "narrow"
            line[tag + "_ms_per_launch"] = round(el / n * 1e3, 4)
            line[tag + "_list_entries_per_query"] = round((s1["list_entries"] - s0["list_entries"]) / (n * nq), 1)
            line[tag + "_wide_launches"] = s1["wide_launches"] - s0["wide_launches"]
            line[tag + "_fallback_queries"] = s1["fallback_queries"] - s0["fallback_queries"]
            ids[wide] = out[2].clone()
        line["ids_equal"] = bool(torch.equal(ids["0"], ids["1"]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
