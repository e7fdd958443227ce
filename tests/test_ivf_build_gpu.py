"""
GPU k-means build, layout and files of the IVF-Flat index (libhiprag hipivf_build*, hipivf_save / hipivf_load) against a
numpy fp64 restatement of the algorithm include/hiprag.h specifies.  Distances and top-k come from the CPU oracle
(oracle.hybrid_oracle.flat_search).  The reference builds faiss.IndexFlatL2 only (rag/storage/faiss_index.py:123); these
are the semantics of faiss.IndexIVFFlat.train / add / write_index / read_index restated for this library.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1


def splitmix64(seed):
    s = (seed + 1) & MASK
    while True:
        s = (s + 0x9E3779B97F4A7C15) & MASK
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        yield z ^ (z >> 31)


def train_rows(n, max_train_rows):
    m = n if max_train_rows <= 0 or max_train_rows >= n else max_train_rows
    return (np.arange(m, dtype=np.int64) * n) // m


def init_rows(m, nlist, seed):
    """positions (in the training set) of the initial centroids: partial Fisher-Yates driven by splitmix64 from seed + 1"""
    perm = list(range(m))
    g = splitmix64(seed)
    for i in range(nlist):
        j = i + next(g) % (m - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm[:nlist], dtype=np.int64)


def oracle_assign(cents, x, metric):
    return ho.flat_search(cents, x, 1, metric)[1][:, 0]


def oracle_update(xt, assign, prev, metric):
    out = prev.copy()
    for l in range(prev.shape[0]):
        members = xt[assign == l].astype(np.float64)
        if len(members) == 0:
            continue
        mean = members.sum(axis=0) / len(members)
        if metric == ho.METRIC_IP:
            nrm = np.sqrt(np.sum(mean * mean))
            if nrm > 0:
                mean = mean / nrm
        out[l] = mean.astype(np.float32)
    return out


def list_of_rows(offs, orig, n):
    """list id of every original row, from the stored layout"""
    lst = np.full(n, -1, dtype=np.int64)
    for l in range(len(offs) - 1):
        ids = orig[offs[l]:offs[l + 1]]
        lst[ids[ids >= 0]] = l
    return lst


def clustered(n, d, n_centres, sigma, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, n_centres, size=n)] + sigma * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), c


def build(x, nlist, metric, iters, seed=0, max_train_rows=0):
    from hiprag import HipIVFIndex
    ix = HipIVFIndex(x.shape[1], nlist, metric)
    ix.build(x, iters=iters, seed=seed, max_train_rows=max_train_rows)
    return ix


def read_ivf_file(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"HIPIVF01"
    version, d, metric, nlist = np.frombuffer(raw, np.int32, 4, 8)
    n, stored = np.frombuffer(raw, np.int64, 2, 24)
    o = 40
    cents = np.frombuffer(raw, np.float32, nlist * d, o).reshape(nlist, d)
    o += cents.nbytes
    offs = np.frombuffer(raw, np.int64, nlist + 1, o)
    o += offs.nbytes
    orig = np.frombuffer(raw, np.int64, stored, o)
    o += orig.nbytes
    rows = np.frombuffer(raw, np.float32, stored * d, o).reshape(stored, d)
    assert o + rows.nbytes == len(raw)
    return dict(version=version, d=d, metric=metric, nlist=nlist, n=n, stored=stored, cents=cents, offs=offs, orig=orig,
                rows=rows)


# ---- 1. init and determinism -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_init_is_the_documented_rows_and_builds_are_deterministic(gpu, metric):
    import torch
    n, d, nlist = 6000, 256, 16
    x = ho.synthetic_vectors(n, d, seed=71)
    for seed in (0, 12345, 2**63 + 7):
        c0 = build(x, nlist, metric, 0, seed).centroids()
        assert np.array_equal(c0, x[init_rows(n, nlist, seed)])
    a, b = build(x, nlist, metric, 3, seed=5), build(x, nlist, metric, 3, seed=5)
    assert np.array_equal(a.centroids(), b.centroids())
    for u, v in zip(a.lists(), b.lists()):
        assert np.array_equal(u, v)
    c = build(torch.from_numpy(x).cuda(), nlist, metric, 3, seed=5)           # the device entry point: the same build
    assert np.array_equal(a.centroids(), c.centroids())
    assert not np.array_equal(a.centroids(), build(x, nlist, metric, 3, seed=6).centroids())


# ---- 2. one round = one oracle round ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
@pytest.mark.parametrize("n,d,nlist", [(6000, 256, 16), (20011, 128, 64)])
def test_every_round_is_one_oracle_round(gpu, metric, n, d, nlist):
    x = ho.synthetic_vectors(n, d, seed=81)
    x[40:60] = x[3]                                           # exact duplicate rows
    init = init_rows(n, nlist, 0)
    x[init[1]] = x[init[0]]                                   # two equal initial centroids: list 1 starts empty
    prev = None
    for t in range(4):
        ix = build(x, nlist, metric, t)
        c = ix.centroids()
        if t == 0:
            assert np.array_equal(c, x[init])
        else:
            assert np.allclose(c, prev, rtol=0, atol=1e-6), f"round {t}: centroids differ from the oracle's update"
        offs, orig = ix.lists()
        assign = oracle_assign(c, x, metric)
        assert np.array_equal(list_of_rows(offs, orig, n), assign), f"round {t}: lists differ from the exact assignment"
        if t == 0:
            assert np.sum(assign == 1) == 0                   # ties go to the lower list
        prev = oracle_update(x, assign, c, metric)
        if t == 0:
            assert np.array_equal(prev[1], c[1])              # ... and the empty list keeps its centroid
        assert ix.ntotal == n and int(ix.list_lengths.sum()) == n
    assert np.array_equal(build(x, nlist, metric, 1).centroids()[1], x[init[1]])


# ---- 3. layout -------------------------------------------------------------------------------------------------------
def test_layout_and_file_contents(gpu, tmp_path):
    n, d, nlist = 5003, 96, 24
    x = ho.synthetic_vectors(n, d, seed=91)
    ix = build(x, nlist, ho.METRIC_L2, 4)
    offs, orig = ix.lists()
    assert offs[0] == 0 and np.all(offs % 32 == 0) and np.all(np.diff(offs) >= 0) and offs[-1] == len(orig)
    for l in range(nlist):
        ids = orig[offs[l]:offs[l + 1]]
        real = ids[ids >= 0]
        assert np.all(np.diff(real) > 0)                      # ascending original id
        assert np.all(ids[len(real):] == -1)                  # padding at the tail only
        assert offs[l + 1] - offs[l] == (len(real) + 31) // 32 * 32
        assert ix.list_lengths[l] == len(real)
    assert np.array_equal(np.sort(orig[orig >= 0]), np.arange(n))
    ix.save(str(tmp_path / "a.ivf"))
    f = read_ivf_file(tmp_path / "a.ivf")
    assert (f["version"], f["d"], f["metric"], f["nlist"], f["n"], f["stored"]) == (1, d, ho.METRIC_L2, nlist, n, len(orig))
    assert np.array_equal(f["cents"], ix.centroids()) and np.array_equal(f["offs"], offs) and np.array_equal(f["orig"], orig)
    assert np.array_equal(f["rows"][orig >= 0], x[orig[orig >= 0]])
    assert not np.any(f["rows"][orig < 0])                    # padding rows are zero


# ---- 4. training sample ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_training_sample(gpu, metric):
    n, d, nlist, m = 7001, 128, 16, 1000
    x = ho.synthetic_vectors(n, d, seed=101)
    tr = train_rows(n, m)
    xt = x[tr]
    c0 = build(x, nlist, metric, 0, seed=3, max_train_rows=m).centroids()
    assert np.array_equal(c0, xt[init_rows(m, nlist, 3)])
    ix = build(x, nlist, metric, 1, seed=3, max_train_rows=m)
    assert np.allclose(ix.centroids(), oracle_update(xt, oracle_assign(c0, xt, metric), c0, metric), rtol=0, atol=1e-6)
    offs, orig = ix.lists()
    assert np.array_equal(np.sort(orig[orig >= 0]), np.arange(n))   # every row stored
    q = ho.synthetic_queries(9, d, seed=102)
    s, i = ix.search(q, 10, nprobe=nlist)
    es, ei = ho.flat_search(x, q, 10, metric)
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=1e-4)


# ---- 5. search -------------------------------------------------------------------------------------------------------
def cpu_ivf_search(x, cents, offs, orig, q, k, nprobe, metric):
    """top-nprobe lists by exact score (ties to the lower list), then the exact top-k of their rows"""
    probe = ho.flat_search(cents, q, nprobe, metric)[1]
    ids = np.full((len(q), k), -1, dtype=np.int64)
    for j in range(len(q)):
        rows = np.sort(np.concatenate([orig[offs[l]:offs[l + 1]] for l in probe[j]]))
        rows = rows[rows >= 0]
        local = ho.flat_search(x[rows], q[j:j + 1], k, metric)[1][0]
        ids[j] = np.where(local >= 0, rows[np.maximum(local, 0)], -1)
    return ids


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_search_against_the_cpu_ivf_oracle(gpu, metric):
    n, d, nlist, k = 30000, 128, 64, 10
    x, centres = clustered(n, d, 48, 0.35, seed=111)
    rng = np.random.default_rng(112)
    q_rows = x[rng.integers(0, n, size=40)] + 0.05 * rng.standard_normal((40, d))
    q_held = centres[rng.integers(0, len(centres), size=24)] + 0.35 * rng.standard_normal((24, d))
    q = np.concatenate([q_rows, q_held]).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ix = build(x, nlist, metric, 8)
    cents = ix.centroids()
    offs, orig = ix.lists()
    es, ei = ho.flat_search(x, q, k, metric)
    s, i = ix.search(q, k, nprobe=nlist)
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=1e-4)
    last = 0.0
    for nprobe in (1, 2, 4, 8, 16, 64):
        _, i = ix.search(q, k, nprobe=nprobe)
        assert np.array_equal(i, cpu_ivf_search(x, cents, offs, orig, q, k, nprobe, metric)), f"nprobe {nprobe}"
        recall = np.mean([len(set(a) & set(b)) / k for a, b in zip(i, ei)])
        assert recall >= last - 1e-12
        last = recall
    assert last == 1.0


def test_default_nprobe(gpu):
    from hiprag import HipIVFIndex
    x = ho.synthetic_vectors(3000, 64, seed=121)
    q = ho.synthetic_queries(5, 64, seed=122)
    ix = HipIVFIndex(64, 12, "ip", nprobe=3)
    ix.build(x, iters=2)
    assert all(np.array_equal(a, b) for a, b in zip(ix.search(q, 7), ix.search(q, 7, 3)))
    with pytest.raises(ValueError):
        HipIVFIndex(64, 12, "ip").train_add(x[:5])


# ---- 6. save / load --------------------------------------------------------------------------------------------------
def test_save_load_round_trip_and_corrupt_files(gpu, tmp_path):
    from hiprag import HipFlatIndex, HipIVFIndex, HipRagError
    n, d, nlist = 8000, 160, 20
    x = ho.synthetic_vectors(n, d, seed=131)
    q = ho.synthetic_queries(17, d, seed=132)
    ix = build(x, nlist, ho.METRIC_IP, 5, seed=9)
    p = str(tmp_path / "doc_hip.index")
    ix.save(p)
    jx = HipIVFIndex.load(p, device=0)
    assert (jx.d, jx.nlist, jx.metric, jx.ntotal) == (d, nlist, ho.METRIC_IP, n)
    assert np.array_equal(jx.centroids(), ix.centroids())
    assert all(np.array_equal(a, b) for a, b in zip(jx.lists(), ix.lists()))
    assert np.array_equal(jx.list_lengths, ix.list_lengths)
    for nprobe in (1, 5, nlist):
        sa, ia = ix.search(q, 12, nprobe)
        sb, ib = jx.search(q, 12, nprobe)
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb)
    raw = open(p, "rb").read()
    f = read_ivf_file(p)
    off_offs = 40 + f["cents"].nbytes
    off_orig = off_offs + f["offs"].nbytes

    def bad(name, data):
        path = str(tmp_path / name)
        with open(path, "wb") as fh:
            fh.write(data)
        with pytest.raises(HipRagError):
            HipIVFIndex.load(path)

    for cut in (0, 5, 8, 30, 40, off_offs - 3, off_orig + 8, len(raw) - 1):
        bad(f"cut{cut}", raw[:cut])
    bad("longer", raw + b"\0" * 4)
    offs = f["offs"].copy()
    offs[1] += 1                                              # not on a 32-row block
    bad("unaligned", raw[:off_offs] + offs.tobytes() + raw[off_offs + offs.nbytes:])
    offs = f["offs"].copy()
    j = int(np.nonzero(offs[1:-1] != offs[2:])[0][0]) + 1
    offs[j], offs[j + 1] = offs[j + 1], offs[j]               # two offsets swapped: not monotone
    bad("swapped", raw[:off_offs] + offs.tobytes() + raw[off_offs + offs.nbytes:])
    orig = f["orig"].copy()
    real = np.nonzero(orig >= 0)[0]
    orig[real[1]] = orig[real[0]]                             # one id twice, another missing
    bad("dup", raw[:off_orig] + orig.tobytes() + raw[off_orig + orig.nbytes:])
    orig = f["orig"].copy()
    orig[real[0]] = n                                         # out of range
    bad("range", raw[:off_orig] + orig.tobytes() + raw[off_orig + orig.nbytes:])
    flat = HipFlatIndex(d, "ip")
    flat.add(x[:100])
    fp = str(tmp_path / "flat_hip.index")
    flat.save(fp)
    with pytest.raises(HipRagError, match="hipidx_load"):
        HipIVFIndex.load(fp)
    with pytest.raises(HipRagError):
        HipFlatIndex.load(p)


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------
def test_bad_build_arguments_raise(gpu):
    import torch
    from hiprag import HipIVFIndex, HipRagError
    x = ho.synthetic_vectors(500, 32, seed=141)
    with pytest.raises(HipRagError):
        HipIVFIndex(32, 0, "l2").build(x)                                    # nlist = 0
    with pytest.raises(HipRagError):
        HipIVFIndex(32, 8, "l2").build(x, max_train_rows=5)                  # nlist > training rows
    with pytest.raises(HipRagError):
        HipIVFIndex(32, 8, "l2").build(x, iters=-1)
    with pytest.raises(HipRagError):
        HipIVFIndex(0, 4, "l2").build(np.zeros((100, 0), np.float32))        # d = 0
    with pytest.raises(HipRagError):
        HipIVFIndex(1100, 4, "l2").build(np.ones((100, 1100), np.float32))   # d > 1024
    with pytest.raises(HipRagError):
        HipIVFIndex(1100, 4, "ip").build(torch.ones((100, 1100), device="cuda"))
    ix = HipIVFIndex(32, 8, "l2")
    ix.build(x)
    with pytest.raises(HipRagError):
        ix.search(x[:2], 257, 2)                                             # k <= 256
    with pytest.raises(HipRagError):
        ix.search(x[:2], 5, 1001)                                            # nprobe <= 1000
