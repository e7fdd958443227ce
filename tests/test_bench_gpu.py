"""GPU: bench.py's plain run (headline only), its --dump-outputs files and the figures that --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROWS, STEPS, WARMUP = 128000, 3, 2


def _bench_line(args, timeout=600, cwd=REPO):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_times_steps_and_dumps_the_last_one(gpu, tmp_path):
    """A plain run prints the headline only; --steps sets the timed launches; the dump is the last timed step's exact top-10."""
    import torch
    import bench
    out = tmp_path / "out"
    d = _bench_line(["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--rows", str(ROWS),
                     "--dump-outputs", str(out)])
    assert d["steps"] == STEPS and d["roofline"]["launches_timed"] == STEPS and d["ms_per_step"] > 0
    assert d["fallback_queries"] == 0
    for key in ("legs", "cpu_baseline", "p50_ms_single_query", "one_hipidx_search_dev_call_per_4096_queries_qps"):
        assert key not in d
    assert "read_probe_GBs" not in d["roofline"]
    s64, s32, ids = (np.load(out / f"{n}.npy") for n in ("scores64", "scores32", "ids"))
    batch = d["config"]["queries_per_step"]
    assert s64.dtype == np.float64 and s32.dtype == np.float32 and ids.dtype == np.float64
    assert s64.shape == s32.shape == ids.shape == (batch, bench.TOPK)
    assert sorted(os.listdir(out)) == ["ids.npy", "scores32.npy", "scores64.npy"]
    # the same seeded rows and queries, the last step's batch, exact fp64 top-10 on the GPU
    dev = torch.device("cuda", 0)
    chunk = ROWS // 32
    x = torch.cat([bench.gen_chunk(torch, c, min(chunk, ROWS - c * chunk), dev) for c in range((ROWS + chunk - 1) // chunk)])
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    q = torch.randn((bench.N_QUERIES, bench.DIM), generator=g, device=dev, dtype=torch.float32)
    q /= q.norm(dim=1, keepdim=True)
    b = (WARMUP + STEPS - 1) % (bench.N_QUERIES // batch)
    sc = q[b * batch:(b + 1) * batch].double() @ x.double().T
    ts, ti = torch.topk(sc, bench.TOPK, dim=1)
    assert np.array_equal(ids, ti.cpu().numpy().astype(np.float64))
    assert np.allclose(s64, ts.cpu().numpy(), rtol=0, atol=1e-12)
    assert np.array_equal(s32, s64.astype(np.float32))


def test_full_run_keeps_the_extra_figures(gpu):
    """--full still measures what moved out of the plain run: latencies, the one-call rate, the read probe, the CPU
    baseline and the legs."""
    d = _bench_line(["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--rows", str(ROWS), "--full",
                     "--legs", "fp32"])
    assert d["steps"] == STEPS and d["p50_ms_single_query"] > 0 and d["one_hipidx_search_dev_call_per_4096_queries_qps"] > 0
    assert d["roofline"]["read_probe_GBs"] > 0
    assert d["cpu_baseline"]["ids_equal_gpu"] is True
    assert d["legs"]["fp32_stream"]["ids_equal_default_mode"] is True


def test_config3_two_rank_rehearsal_dumps_into_the_callers_directory(gpu, tmp_path):
    """A relative --dump-outputs DIR is the caller's even though bench.py starts its ranks in the repository; rank 0 writes
    the fused top-10 of config3's last timed step."""
    d = _bench_line(["--gpus", "2", "--workload", "config3", "--rows", "64000", "--steps", "3", "--warmup", "1",
                     "--backend", "gloo", "--share-gpu", "--dump-outputs", "out"], cwd=tmp_path)
    assert d["steps"] == 3 and d["ranks_seen"] == 2 and d["fused_lists_equal_on_all_ranks"]
    assert sorted(os.listdir(tmp_path / "out")) == ["ids.npy", "scores.npy"]
    scores, ids = np.load(tmp_path / "out" / "scores.npy"), np.load(tmp_path / "out" / "ids.npy")
    assert scores.dtype == np.float32 and ids.dtype == np.float64
    assert scores.shape == ids.shape == (d["config"]["queries_per_step"], 10)
    assert np.all((ids >= 0) & (ids < 64000)) and np.all(np.diff(scores, axis=1) <= 0)
