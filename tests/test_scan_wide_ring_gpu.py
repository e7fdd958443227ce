"""
The staging ring of the wide scan kernel (csrc/scan_wide.h: row pieces in a ring of five 16 KiB slots, four k-steps ahead;
query pieces in a ring of three, two ahead; counted waits) against the CPU oracle -- ids bit-exact, scores within 1e-4, as in
test_scan_wide_gpu.py -- where the ring can go wrong: every residue of the steps per tile against both ring lengths, a
sequence shorter than the ring, workgroups without a tile, clamped query pieces, the narrow kernel's answers bit for bit,
and launches in flight.
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
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", wide)
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def _check(ix, q, es, ei):
    s, i = ix.search(q, es.shape[1])
    assert np.array_equal(i, ei), f"ids differ: first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
    assert np.allclose(s, es, rtol=0, atol=TOL)


@pytest.mark.parametrize("nq", [129, 257, 512])
@pytest.mark.parametrize("d", [100, 200, 320, 600, 1024])
def test_ring_against_tile_boundaries(gpu, monkeypatch, d, nq):
    """k-steps per tile 4, 8, 12, 20, 32: mod 5 (the row ring) 4, 3, 2, 0, 2, mod 3 (the query ring) 1, 2, 0, 2, 2, so both
    rings wrap at every phase against the tile boundaries.  200 spare CUs: every workgroup walks four or five row tiles
    of 70,001 rows (one or two of 20,011 at d = 1024), times one or two columns; 129 and 257 queries end in a unit with one
    live query, 257 in a column whose other units are clamped."""
    n, k, seed = (20011 if d == 1024 else 70001), 10, 400 + d
    x, qall = _data(n, d, 512, seed)
    es, ei = _truth(n, d, 512, seed, k, ho.METRIC_IP)
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    ix.set_spare_cus(200)
    _check(ix, qall[:nq], es[:nq], ei[:nq])
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == 1
    assert st["fallback_queries"] == 0


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
@pytest.mark.parametrize("nq", [129, 256])
def test_sequence_shorter_than_the_ring(gpu, monkeypatch, nq, metric):
    """16,385 rows, d = 100, one column: a workgroup's whole sequence is the four k-steps the prologue issues, every load of
    the loop goes past its end, and 65 row tiles on a larger grid leave workgroups without a tile."""
    n, d, k = 16385, 100, 10
    x, qall = _data(n, d, 256, 451)
    es, ei = _truth(n, d, 256, 451, k, metric)
    ix = _index(monkeypatch, x, metric)
    _check(ix, qall[:nq], es[:nq], ei[:nq])
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == 1


@pytest.mark.parametrize("nq", [257, 300, 330])
def test_clamped_query_pieces(gpu, monkeypatch, nq):
    """The last column has one live unit (257: one query of it, 300: 44) or two (330); the query pieces of its other units
    are loaded from the last image there is.  Every query of the last live unit is a row plus 5 % noise, the rows spread
    over the row tiles, and finds it; the query before the last is zero and takes the exhaustive path."""
    n, d, k = 20011, 200, 10
    x, q0 = _data(n, d, 330, 461)
    q = q0[:nq].copy()
    first = 64 * ((nq - 1) // 64)                       # the last live unit
    j = np.arange(first, nq)
    r = (977 * (j - first) + 31 * j) % n
    rng = np.random.default_rng(462)
    noise = rng.standard_normal((len(j), d))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    p = x[r].astype(np.float64) + 0.05 * noise
    q[first:] = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    zero = nq - 2
    q[zero] = 0
    es, ei = ho.flat_search(x, q, k, ho.METRIC_IP)
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    s, i = ix.search(q, k)
    planted = j != zero
    assert np.array_equal(ei[first:, 0][planted], r[planted])   # the data: a planted row is its query's best
    assert np.array_equal(i, ei)
    assert np.allclose(s, es, rtol=0, atol=TOL)
    st = ix.stats()
    assert st["wide_launches"] == 1 and st["fallback_queries"] >= 1


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_same_bits_from_both_kernels(gpu, monkeypatch, metric):
    """20,011 x 320 (12 k-steps per tile), 300 queries: search_device returns the same bits whichever kernel nominated."""
    import torch
    n, d, nq, k = 20011, 320, 300, 10
    x, q = _data(n, d, nq, 471)
    qd = torch.from_numpy(q.copy()).cuda()
    outs = []
    for wide in ("0", "1"):
        ix = _index(monkeypatch, x, metric, wide)
        s64, s32, ids = ix.search_device(qd, k)
        torch.cuda.synchronize()
        assert ix.stats()["wide_launches"] == (1 if wide == "1" else 0)
        outs.append((s64.clone(), ids.clone()))
        ix.close()
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[1][1].cpu().numpy(), _truth(n, d, nq, 471, k, metric)[1])


def test_launches_in_flight_equal_launches_in_turn(gpu, monkeypatch):
    """Four launches in flight through ShardedFlatIndex.search_begin / search_end at 70,001 x 200 (the finish of one beside
    the scan of the next) return what the same launches return one at a time."""
    import torch
    from collections import deque
    from hiprag.sharded import ShardedFlatIndex
    n, d, k = 70001, 200, 10
    x, q = _data(n, d, 512, 600)                          # the data of test_ring_against_tile_boundaries at d = 200
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    sh = ShardedFlatIndex(ix, 0, tails_aside=True)
    qd = torch.from_numpy(q.copy()).cuda()
    plan = [(0, 512), (100, 400), (256, 512), (0, 257), (3, 303), (0, 512)]
    alone = []
    for lo, hi in plan:
        alone.append(tuple(v.clone() for v in sh.search_end(sh.search_begin(qd[lo:hi], k))))
    pending, flown = deque(), []
    for lo, hi in plan:
        pending.append(sh.search_begin(qd[lo:hi], k))
        if len(pending) >= 4:
            flown.append(tuple(v.clone() for v in sh.search_end(pending.popleft())))
    while pending:
        flown.append(tuple(v.clone() for v in sh.search_end(pending.popleft())))
    torch.cuda.synchronize()
    es, ei = _truth(n, d, 512, 600, k, ho.METRIC_IP)
    for (lo, hi), one, many in zip(plan, alone, flown):
        for u, v in zip(one, many):
            assert torch.equal(u, v), (lo, hi)
        assert np.array_equal(many[2].cpu().numpy(), ei[lo:hi]), (lo, hi)
    st = ix.stats()
    assert st["wide_launches"] == 2 * len(plan) and st["fallback_queries"] == 0
