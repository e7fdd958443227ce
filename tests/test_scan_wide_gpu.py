"""
The wide scan kernel (scan_wide_kernel, csrc/scan_wide.h: 256 queries per read of the bf16 filter copy) against the CPU
oracle -- ids bit-exact, scores within 1e-4, as in test_dense_gpu.py -- at the smallest shapes at which it can go wrong:
the smallest eligible index, more tiles than workgroups with ragged rows / queries / grids, the workload's K, every wave
position as the home of a best row, the narrow kernel's answers bit for bit, list lengths, the dispatch and a pipeline.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu
TOL = 1e-4


@functools.lru_cache(maxsize=None)
def _data(n, d, nq, seed):
    x = ho.synthetic_vectors(n, d, seed=seed)
    q = ho.synthetic_queries(nq, d, seed=seed + 1)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


@functools.lru_cache(maxsize=None)
def _truth(n, d, nq, seed, k, metric):
    x, q = _data(n, d, nq, seed)
    return ho.flat_search(x, q, k, metric)


def _index(monkeypatch, x, metric, wide="1"):
    from hiprag import HipFlatIndex
    if wide is None:
        monkeypatch.delenv("HIPRAG_SCAN_WIDE", raising=False)
    else:
        monkeypatch.setenv("HIPRAG_SCAN_WIDE", wide)
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def _check(ix, q, es, ei):
    s, i = ix.search(q, es.shape[1])
    assert np.array_equal(i, ei), f"ids differ: first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
    assert np.allclose(s, es, rtol=0, atol=TOL)


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_smallest_eligible_index(gpu, monkeypatch, metric):
    """16,385 rows = 513 blocks: the filter is just on; 65 row tiles (fewer than workgroups), the last with one block of one
    live row; d = 100 -> two k-steps and the scalar query path; 257 queries: the second column has one live query."""
    n, d, nq, k = 16385, 100, 257, 10
    x, q = _data(n, d, nq, 301)
    ix = _index(monkeypatch, x, metric)
    assert ix.launch_queries == 1024
    _check(ix, q, *_truth(n, d, nq, 301, k, metric))
    st = ix.stats()
    assert st["wide_launches"] == 1 and st["launches"] == 1 and st["passes"] == 5


@pytest.mark.parametrize("spare", [0, 48, 200])
@pytest.mark.parametrize("nq", [129, 256, 300, 1024, 1100])
def test_more_tiles_than_workgroups_ragged_everything(gpu, monkeypatch, nq, spare):
    """70,001 rows (274 row tiles, the last partial), d = 200; one to four columns in a launch, 1100 = two launches; with
    200 spare CUs every workgroup walks five or more tiles and the staging stream crosses tile boundaries."""
    n, d, k = 70001, 200, 10
    x, qall = _data(n, d, 1100, 311)
    es, ei = _truth(n, d, 1100, 311, k, ho.METRIC_IP)
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    ix.set_spare_cus(spare)
    _check(ix, qall[:nq], es[:nq], ei[:nq])
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == (2 if nq > 1024 else 1)
    assert st["fallback_queries"] == 0


@pytest.mark.parametrize("k", [10, 50])
def test_the_workloads_k_dimension(gpu, monkeypatch, k):
    n, d, nq = 20011, 1024, 512
    x, q = _data(n, d, nq, 321)
    ix = _index(monkeypatch, x, ho.METRIC_L2)
    _check(ix, q, *_truth(n, d, nq, 321, k, ho.METRIC_L2))
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] and st["fallback_queries"] == 0


def test_every_wave_position_is_home_of_a_best_row(gpu, monkeypatch):
    """Query j is row r_j plus 5 % noise: r_j = 32 (8 t_j + j mod 8) + (7 j mod 32), t_j cycling over the first row tile, a
    tile of the second round and the last full tile -- every (block in tile, query tile in column) pair finds some
    query's best row, in all four columns of the launch."""
    n, d, nq, k = 70001, 256, 1024, 10
    x, _ = _data(n, d, 1, 331)
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    ix.set_spare_cus(48)
    full_tiles = (n // 32) // 8                       # 273 full row tiles: 0 .. 272
    tiles = [0, full_tiles - 10, full_tiles - 1]      # 263 is in the second round of any grid of <= 256 workgroups
    j = np.arange(nq)
    t = np.array(tiles)[(j // 8) % 3]
    r = 32 * (8 * t + j % 8) + (7 * j) % 32
    rng = np.random.default_rng(332)
    noise = rng.standard_normal((nq, d))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = x[r].astype(np.float64) + 0.05 * noise
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    es, ei = ho.flat_search(x, q, k, ho.METRIC_IP)
    s, i = ix.search(q, k)
    assert np.array_equal(i[:, 0], r)
    assert np.array_equal(i, ei)
    assert np.allclose(s, es, rtol=0, atol=TOL)
    assert ix.stats()["wide_launches"] == 1


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_both_kernels_give_the_same_answers(gpu, monkeypatch, metric):
    """40 duplicates of a row, a query equal to that row and a zero query: the results of search_device are the same bits
    whichever scan kernel nominated the candidates; the zero query takes the exhaustive path in both."""
    import torch
    n, d, nq, k = 20011, 128, 200, 10
    x, q = _data(n, d, nq, 341)
    x, q = x.copy(), q.copy()
    x[1000:1040] = x[5]
    q[3] = x[5]
    q[4] = 0
    qd = torch.from_numpy(q).cuda()
    outs = []
    for wide in ("0", "1"):
        ix = _index(monkeypatch, x, metric, wide)
        s64, s32, ids = ix.search_device(qd, k)
        torch.cuda.synchronize()
        st = ix.stats()
        assert st["fallback_queries"] >= 1
        assert st["wide_launches"] == (1 if wide == "1" else 0)
        outs.append((s64.clone(), ids.clone()))
        ix.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    es, ei = ho.flat_search(x, q, k, metric)
    assert np.array_equal(outs[1][1].cpu().numpy(), ei)


@pytest.mark.parametrize("wide", ["1", "0"])
def test_the_filter_filters(gpu, monkeypatch, wide):
    """A condition on the list lengths, so that lists overflowing into the exhaustive path cannot hide behind exact results:
    at most 2048 entries per query (half of the list capacity), nobody on the exhaustive path.  The narrow kernel
    (wide = 0) meets the same condition."""
    n, d, nq, k = 70001, 256, 512, 10
    x, q = _data(n, d, 1024, 351)                       # shared with test_pipeline_and_gate
    es, ei = _truth(n, d, 1024, 351, k, ho.METRIC_IP)
    ix = _index(monkeypatch, x, ho.METRIC_IP, wide)
    _check(ix, q[:nq], es[:nq], ei[:nq])
    st = ix.stats()
    print(f"wide={wide}: list entries per query {st['list_entries'] / st['queries']:.1f}, ranked {st['ranked_entries'] / st['queries']:.1f}")
    assert st["wide_launches"] == (1 if wide == "1" else 0)
    assert st["fallback_queries"] == 0
    assert st["list_entries"] / st["queries"] <= 2048


def test_which_kernel_ran(gpu, monkeypatch):
    from hiprag import HipFlatIndex, HipRagError
    n, d, k = 16385, 64, 10
    x, q = _data(n, d, 640, 361)
    ix = _index(monkeypatch, x, ho.METRIC_IP)            # forced: every launch of more than 64 queries
    for nq, wide in ((64, 0), (65, 1), (640, 1)):
        before = ix.stats()
        ix.search(q[:nq], k)
        st = ix.stats()
        assert st["wide_launches"] - before["wide_launches"] == wide, nq
        assert st["launches"] - before["launches"] == 1
    ix.close()
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ix = _index(monkeypatch, x, ho.METRIC_IP)            # forced, but fewer than 32 scan workgroups: row tiles 0..31, the
    for spare, wide in ((n_cu - 31, 0), (n_cu - 32, 1)):  # publishers of the 64 classes, would not share the first round
        ix.set_spare_cus(spare)
        before = ix.stats()["wide_launches"]
        ix.search(q[:640], k)
        assert ix.stats()["wide_launches"] - before == wide, spare
    ix.close()
    ix = _index(monkeypatch, x, ho.METRIC_IP, None)      # unset: from 256 queries, and only where every workgroup owns a row tile
    tiles = (n + 255) // 256                             # 65
    for spare, nq, wide in ((n_cu - tiles, 64, 0), (n_cu - tiles, 255, 0), (n_cu - tiles, 256, 1), (n_cu - tiles, 640, 1),
                            (n_cu - tiles - 1, 640, 0), (0, 640, 0)):
        ix.set_spare_cus(spare)
        before = ix.stats()["wide_launches"]
        ix.search(q[:nq], k)
        assert ix.stats()["wide_launches"] - before == wide, (spare, nq)
    ix.close()
    ix = _index(monkeypatch, x, ho.METRIC_IP, "0")
    ix.search(q[:640], k)
    assert ix.stats()["wide_launches"] == 0
    ix.close()
    ix = _index(monkeypatch, x[:5000], ho.METRIC_IP)     # 157 blocks: the filter is off
    ix.search(q[:640], k)
    assert ix.stats()["wide_launches"] == 0
    ix.close()
    monkeypatch.setenv("HIPRAG_SCAN_MODE", "q64")
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    ix.search(q[:640], k)
    assert ix.stats()["wide_launches"] == 0
    ix.close()
    monkeypatch.delenv("HIPRAG_SCAN_MODE")
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", "yes")
    with pytest.raises(HipRagError):
        HipFlatIndex(d, ho.METRIC_IP)


def test_pipeline_and_gate(gpu, monkeypatch):
    """ShardedFlatIndex with the tails aside (the finish of step i runs beside the wide scan of step i + 1, behind the
    start gate): six steps of 512 queries, four in flight, then 70 queries and a step of k = 50."""
    import torch
    from collections import deque
    from hiprag.sharded import ShardedFlatIndex
    n, d = 70001, 256
    x, q = _data(n, d, 1024, 351)
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    sh = ShardedFlatIndex(ix, 0, tails_aside=True)
    qd = torch.from_numpy(q.copy()).cuda()
    # neighbouring steps take different halves of the queries: a result that landed in the wrong step's buffers shows
    plan = [(512 * (s % 2), 512 * (s % 2) + 512, 10) for s in range(6)] + [(100, 170, 10), (300, 428, 50)]
    pending, got = deque(), []
    for lo, hi, k in plan:
        pending.append((lo, hi, k, sh.search_begin(qd[lo:hi], k)))
        if len(pending) >= 4:
            a, b, kk, t = pending.popleft()
            got.append((a, b, kk, tuple(v.clone() for v in sh.search_end(t))))
    while pending:
        a, b, kk, t = pending.popleft()
        got.append((a, b, kk, tuple(v.clone() for v in sh.search_end(t))))
    torch.cuda.synchronize()
    es10, ei10 = _truth(n, d, 1024, 351, 10, ho.METRIC_IP)
    es50, ei50 = ho.flat_search(x, q[300:428], 50, ho.METRIC_IP)
    for lo, hi, k, (s64, s32, ids) in got:
        es, ei = (es10[lo:hi], ei10[lo:hi]) if k == 10 else (es50, ei50)
        assert np.array_equal(ids.cpu().numpy(), ei), (lo, hi, k)
        assert np.allclose(s32.cpu().numpy(), es, rtol=0, atol=TOL)
    st = ix.stats()
    assert st["wide_launches"] == 8 and st["fallback_queries"] == 0
