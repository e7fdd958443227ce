"""
Updatable IVF-Flat (libhiprag hipivf_from_centroids, hipivf_add(_dev), hipivf_remove_ranges, hipivf_update_info) against the
numpy model of tests/test_ivf_update_cpu.py: after every update the handle must be indistinguishable from the layout step of
hipivf_build over the current rows -- lists, counts, the bytes of the HIPIVF01 file, and both searches at any nprobe (at
nprobe = nlist the flat index over the current rows, bit for bit; below it an IVF view over flat indexes built from the
model's layout).  Rows are one of five orthonormal centroids plus noise of 1 %: their lists are known by construction and
the CPU oracle agrees with a wide margin (checked in the CPU file).
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from test_ivf_update_cpu import IvfModel, clustered_rows, ranges_of, separated_centroids

pytestmark = pytest.mark.gpu

NLIST = 5
E_INVALID, E_UNSUPPORTED = -1, -6
STAGING_LIMIT = 256 << 20            # DenseIndex::kRemoveBudget: staging + run table of a move
CASES = [(ho.METRIC_IP, 64), (ho.METRIC_L2, 64), (ho.METRIC_IP, 36), (ho.METRIC_L2, 36)]


def bits_equal(a, b):
    """two (scores64, scores32, ids) triples: equal ids, equal score BIT PATTERNS"""
    import torch
    return (torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
            and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def file_of(ix, path):
    ix.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def flat_of(x, metric):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def queries(m, rng):
    """rows of the index (the planted duplicates among them: their hits tie and are ordered by id), the zero vector every
    padding row equals, and noisy centroids"""
    q = [np.zeros((1, m.d), np.float32), clustered_rows(m.cents, np.arange(m.nlist), rng, sigma=0.05)]
    if m.n:
        picks = [ids[min(3, len(ids) - 1)] for ids in m.lists if len(ids)] + [m.n - 1]
        q.append(m.x[np.asarray(picks)])
    return np.concatenate(q).astype(np.float32)


def check_searches(ix, m, rng, tag):
    import torch
    from hiprag import HipIVFIndex
    qd = torch.from_numpy(queries(m, rng)).cuda()
    if m.n == 0:                                                     # empty lists: padding only, from every entry
        for fn in (ix.search_device, ix.search_batch_device):
            for nprobe in (1, NLIST):
                out = fn(qd, 10, nprobe)
                torch.cuda.synchronize()
                assert bool((out[2] == -1).all()), f"{tag}: an empty index returned an id"
        return
    flat = flat_of(m.x, m.metric)
    for k in (10, 256):
        want = flat.search_device(qd, k)
        one, bat = ix.search_device(qd, k, NLIST), ix.search_batch_device(qd, k, NLIST)
        torch.cuda.synchronize()
        assert bits_equal(one, want), f"{tag}: search_device differs from the flat index at nprobe = nlist, k = {k}"
        assert bits_equal(bat, want), f"{tag}: search_batch_device differs from the flat index at nprobe = nlist, k = {k}"
    offs, orig = m.layout()
    rows, cents = flat_of(m.stored_rows(), m.metric), flat_of(m.cents, m.metric)
    view = HipIVFIndex.from_parts(rows, cents, offs, orig)
    for nprobe in (1, 2):
        want = view.search_device(qd, 10, nprobe)
        one, bat = ix.search_device(qd, 10, nprobe), ix.search_batch_device(qd, 10, nprobe)
        torch.cuda.synchronize()
        assert bits_equal(one, want), f"{tag}: search_device differs from the model's layout at nprobe {nprobe}"
        assert bits_equal(bat, want), f"{tag}: search_batch_device differs from the model's layout at nprobe {nprobe}"
    view.close()


def check_state(ix, m, path, tag, info=None, batch_bytes=0):
    offs, orig = ix.lists()
    eoffs, eorig = m.layout()
    assert np.array_equal(offs, eoffs), f"{tag}: list offsets"
    assert np.array_equal(orig, eorig), f"{tag}: original ids"
    assert ix.ntotal == m.n and np.array_equal(ix.list_lengths, m.lengths()), f"{tag}: counts"
    raw = file_of(ix, path)
    assert raw == m.file_bytes(), f"{tag}: HIPIVF01 file bytes"
    if info is not None:
        got = ix.update_info()
        assert {key: got[key] for key in info} == info, f"{tag}: update_info {got}, expected {info}"
        if info["added"] or info["removed"]:      # tables at least, staging where rows are written
            assert 0 < got["extra_bytes"] <= STAGING_LIMIT + 4 * batch_bytes + (1 << 20), f"{tag}: extra bytes {got['extra_bytes']}"
        else:
            assert got["extra_bytes"] == 0
    return raw


def edge_script(cents, seed):
    """(name, step): step(ix, m) applies one update to the index and the model and returns (expected update_info, bytes of
    the batch).  Lengths of the five lists are in the comments."""
    import torch
    rng = np.random.default_rng(seed)
    state = {"dev": False}

    def add_rows(ix, m, x, labels):
        state["dev"] = not state["dev"]                              # the two entry points take turns
        ix.add(torch.from_numpy(x).cuda() if state["dev"] else x)
        return m.add(x, labels), x.nbytes

    def add(labels, shuffle=False):
        def step(ix, m):
            lab = rng.permutation(labels) if shuffle else np.asarray(labels, dtype=np.int64)
            return add_rows(ix, m, clustered_rows(cents, lab, rng), lab)
        return step

    def duplicates(ix, m):                                           # exact copies of a row of list 1 and of a row of list 3
        return add_rows(ix, m, m.x[[m.lists[1][3], m.lists[3][0], m.lists[1][3]]].copy(), [1, 3, 1])

    def remove(pick):
        def step(ix, m):
            r = pick(m)
            ix.remove_ranges(r)
            return m.remove(r), 0
        return step

    return [
        ("add to an empty index", add(np.repeat(np.arange(NLIST), [31, 32, 255, 0, 40]), shuffle=True)),      # 31 32 255 0 40
        ("31 rows gain 1: fills padding", add([0])),                                                          # 32 32 255 0 40
        ("32 rows gain 1: a new block", add([1])),                                                            # 32 33 255 0 40
        ("255 to 257 across a 256-row slice", add([2, 2])),                                                   # 32 33 257 0 40
        ("a list gets nothing, an empty list gets rows", add([3, 3, 3, 0, 1, 2])),                            # 33 34 258 3 40
        ("all to the last list", add([4] * 5)),                                                               # 33 34 258 3 45
        ("all to list 0", add([0] * 40)),                                                                     # 73 34 258 3 45
        ("n_add = 0", add([])),
        ("duplicates in two lists", duplicates),                                                              # 73 36 258 4 45
        ("a removal empties a list", remove(lambda m: ranges_of(m.lists[3]))),                                # 73 36 258 0 45
        ("a list shrinks across a block boundary", remove(lambda m: ranges_of(m.lists[2][[0, 100, 257]]))),   # 73 36 255 0 45
        ("a range spanning several lists", remove(lambda m: np.asarray([[10, 60]]))),
        ("two ranges and an empty one", remove(lambda m: np.asarray([[0, 2], [5, 5], [200, 203]]))),
        ("tail ids", remove(lambda m: np.asarray([[m.n - 7, m.n]]))),
        ("an empty table", remove(lambda m: np.zeros((0, 2), np.int64))),
        ("an add after a removal", add([0, 1, 2, 3, 4, 4, 2], shuffle=True)),
        ("all rows", remove(lambda m: np.asarray([[0, m.n]]))),
        ("an add after all rows went", add(np.repeat(np.arange(NLIST), [3, 0, 33, 1, 64]), shuffle=True)),
    ]


def fresh(cents, metric):
    from hiprag import HipIVFIndex
    return HipIVFIndex.from_centroids(cents, metric), IvfModel(cents, metric)


# ---- 1. anchor: build(x) == from_centroids(build's centroids) + add(x), in one batch or many --------------------------
@pytest.mark.parametrize("metric,d", CASES)
def test_adds_under_a_builds_centroids_give_the_builds_file(gpu, tmp_path, metric, d):
    import torch
    from hiprag import HipIVFIndex
    rng = np.random.default_rng(21)
    cents = separated_centroids(NLIST, d, seed=5)
    x = clustered_rows(cents, rng.integers(0, NLIST, size=3001), rng, sigma=0.05)
    built = HipIVFIndex(d, NLIST, metric)
    built.build(x, iters=2)
    want = file_of(built, tmp_path / "built.ivf")
    assert built.update_info() == {"added": 0, "removed": 0, "moved": 0, "chunks": 0, "extra_bytes": 0}
    one = HipIVFIndex.from_centroids(built.centroids(), metric)
    one.add(x)
    assert file_of(one, tmp_path / "one.ivf") == want
    many = HipIVFIndex.from_centroids(built.centroids(), metric)
    o = 0
    for step in (1, 31, 32, 193, len(x)):
        part = x[o:o + step]
        many.add(torch.from_numpy(part).cuda() if step == 32 else part)
        o += len(part)
    assert o == len(x) and many.ntotal == len(x)
    assert file_of(many, tmp_path / "many.ivf") == want
    # ... and the built index itself takes updates: remove a range, add it back at the end == a build of the rotated rows
    built.remove_ranges([[100, 400]])
    built.add(x[100:400])
    rot = IvfModel.from_lists(built.centroids(), metric, np.concatenate([x[:100], x[400:], x[100:400]]), *built.lists())
    assert file_of(built, tmp_path / "rot.ivf") == rot.file_bytes()
    lab = ho.flat_search(built.centroids(), rot.x, 1, metric)[1][:, 0]
    assert all(np.array_equal(rot.lists[l], np.nonzero(lab == l)[0]) for l in range(NLIST))


# ---- 2. + 3. the edge script: state and searches after every step -------------------------------------------------------
@pytest.mark.parametrize("metric,d", CASES)
def test_edge_script_matches_the_model_after_every_step(gpu, tmp_path, metric, d):
    cents = separated_centroids(NLIST, d, seed=9)
    ix, m = fresh(cents, metric)
    rng = np.random.default_rng(31)
    check_state(ix, m, tmp_path / "s.ivf", "empty", {"added": 0, "removed": 0, "moved": 0, "chunks": 0})
    check_searches(ix, m, rng, "empty")
    for name, step in edge_script(cents, seed=41):
        info, batch_bytes = step(ix, m)
        m.check()
        check_state(ix, m, tmp_path / "s.ivf", name, info, batch_bytes)
        check_searches(ix, m, rng, name)            # the batch search ran before this update too: a stale list table shows
    assert m.n == 101 and np.array_equal(m.lengths(), [3, 0, 33, 1, 64])


def test_edge_script_moves_what_the_layout_rule_says(gpu):
    """the model's `moved` in words, for the steps the move is about"""
    cents = separated_centroids(NLIST, 64, seed=9)
    ix, m = fresh(cents, ho.METRIC_L2)
    moved = {}
    for name, step in edge_script(cents, seed=41)[:7]:
        step(ix, m)
        moved[name] = ix.update_info()["moved"]
    assert moved["add to an empty index"] == 0
    assert moved["31 rows gain 1: fills padding"] == 0
    assert moved["32 rows gain 1: a new block"] == 255 + 40          # everything behind list 1
    assert moved["255 to 257 across a 256-row slice"] == 40
    assert moved["all to the last list"] == 0
    assert moved["all to list 0"] == 34 + 258 + 3 + 45               # 33 -> 73 rows: two more blocks


# ---- 4. files ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [(ho.METRIC_IP, 36), (ho.METRIC_L2, 64)])
def test_saved_and_loaded_index_takes_updates(gpu, tmp_path, metric, d):
    from hiprag import HipIVFIndex
    cents = separated_centroids(NLIST, d, seed=9)
    rng = np.random.default_rng(51)
    script = edge_script(cents, seed=41)
    empty, m0 = fresh(cents, metric)
    empty.save(str(tmp_path / "empty.ivf"))
    ix = HipIVFIndex.load(str(tmp_path / "empty.ivf"))               # an empty index saves and loads
    check_state(ix, m0, tmp_path / "l.ivf", "loaded empty")
    m = m0
    for name, step in script[:11]:
        step(ix, m)
    raw = check_state(ix, m, tmp_path / "a.ivf", "before save")
    jx = HipIVFIndex.load(str(tmp_path / "a.ivf"))
    assert check_state(jx, m, tmp_path / "b.ivf", "loaded") == raw
    check_searches(jx, m, rng, "loaded")
    for name, step in script[11:16]:
        info, batch_bytes = step(jx, m)
        check_state(jx, m, tmp_path / "b.ivf", "loaded, " + name, info, batch_bytes)
        check_searches(jx, m, rng, "loaded, " + name)


# ---- 5. moves larger than the staging budget -----------------------------------------------------------------------------
def test_large_index_moves_in_several_chunks(gpu, tmp_path):
    """70 000 x 1024 (the size tests/test_remove_gpu.py uses for the same budget): an add into list 0 moves every stored row
    up, a removal from list 0 moves every one down, both through more than one staging chunk"""
    import torch
    n, d, nlist, metric = 70000, 1024, 8, ho.METRIC_L2
    rng = np.random.default_rng(61)
    cents = separated_centroids(nlist, d, seed=13)
    labels = rng.integers(0, nlist, size=n)
    labels[:40] = 0
    x = cents[labels] + np.float32(0.01) * rng.standard_normal((n, d), dtype=np.float32)
    ix, m = fresh(cents, metric)
    n0 = n - 64
    ix.add(x[:n0])
    m.add(x[:n0], labels[:n0])
    assert np.array_equal(ix.list_lengths, m.lengths())
    late = np.zeros(64, dtype=np.int64)                              # 64 more rows of list 0: at least one more block
    x[n0:] = clustered_rows(cents, late, rng)
    ix.add(torch.from_numpy(x[n0:]).cuda())
    info = m.add(x[n0:], late)
    got = ix.update_info()
    assert info["moved"] == n0 - len(m.lists[0]) + 64 and got["moved"] == info["moved"] and got["added"] == 64
    assert got["chunks"] >= 2 and got["extra_bytes"] <= STAGING_LIMIT + 4 * x[n0:].nbytes + (1 << 20)
    for u, v in zip(ix.lists(), m.layout()):
        assert np.array_equal(u, v)
    flat = flat_of(x, metric)
    qd = torch.from_numpy(np.concatenate([x[[0, n0 - 1, n0, n - 1]], np.zeros((1, d), np.float32)])).cuda()

    def same_as_flat(flat):
        want = flat.search_device(qd, 10)
        one, bat = ix.search_device(qd, 10, nlist), ix.search_batch_device(qd, 10, nlist)
        torch.cuda.synchronize()
        assert bits_equal(one, want) and bits_equal(bat, want)

    same_as_flat(flat)
    r = ranges_of(m.lists[0][[0, 1, 2, 5, 17, 33, 34, 35]].tolist() + m.lists[0][100:130].tolist())
    ix.remove_ranges(r)
    flat.remove_ranges(r)
    info = m.remove(r)
    got = ix.update_info()
    assert info["removed"] == 38 and got["removed"] == 38 and got["moved"] == info["moved"] and info["moved"] > n // 2
    assert got["chunks"] >= 2 and got["extra_bytes"] <= STAGING_LIMIT + (1 << 20)
    for u, v in zip(ix.lists(), m.layout()):
        assert np.array_equal(u, v)
    same_as_flat(flat)
    ix.save(str(tmp_path / "big.ivf"))                               # every stored row, not only the best ten
    offs, orig = m.layout()
    rows = np.fromfile(str(tmp_path / "big.ivf"), dtype=np.float32, offset=40 + cents.nbytes + offs.nbytes + orig.nbytes)
    assert np.array_equal(rows.reshape(len(orig), d), m.stored_rows())


# ---- 6. refused calls leave the handle as it was -------------------------------------------------------------------------
def test_refused_updates_leave_the_index_unchanged(gpu, tmp_path):
    import torch
    from hiprag import HipIVFIndex, HipRagError
    from hiprag import _native as nat
    d, metric = 36, ho.METRIC_IP
    cents = separated_centroids(NLIST, d, seed=9)
    ix, m = fresh(cents, metric)
    for name, step in edge_script(cents, seed=41)[:5]:
        step(ix, m)
    before, info = file_of(ix, tmp_path / "a.ivf"), ix.update_info()
    n = ix.ntotal
    xd = torch.zeros((4, d), device="cuda")

    def refused(code, fn, *args):
        with pytest.raises(HipRagError) as e:
            fn(*args)
        assert e.value.code == code, str(e.value)
        assert file_of(ix, tmp_path / "b.ivf") == before and ix.update_info() == info and ix.ntotal == n
        return str(e.value)

    for bad in ([[10, 20], [5, 8]], [[5, 10], [8, 12]], [[0, n + 1]], [[7, 3]], [[-1, 2]], [[n, n + 1]]):
        refused(E_INVALID, ix.remove_ranges, bad)
    refused(E_INVALID, nat.call, "hipivf_remove_ranges", ix._h, None, 1)
    refused(E_INVALID, nat.call, "hipivf_remove_ranges", ix._h, None, -1)
    refused(E_INVALID, nat.call, "hipivf_add", ix._h, None, 3)
    refused(E_INVALID, nat.call, "hipivf_add_dev", ix._h, None, 3, None)
    refused(E_INVALID, nat.call, "hipivf_add_dev", ix._h, xd.data_ptr(), -1, None)
    refused(E_INVALID, nat.call, "hipivf_add_dev", ix._h, xd.data_ptr(), (1 << 31) - n, None)      # n + n_add = 2^31
    refused(E_INVALID, nat.call, "hipivf_add", ix._h, xd.cpu().numpy().ctypes.data, (1 << 31) - n)
    refused(E_INVALID, nat.call, "hipivf_update_info", ix._h, None)
    for call in (lambda: ix.add(np.zeros((3, d + 1), np.float32)), lambda: ix.add(torch.zeros((3, d - 1), device="cuda")),
                 lambda: ix.add(torch.zeros((3, d), device="cuda", dtype=torch.float64)), lambda: ix.remove_ranges(np.zeros((2, 3), np.int64))):
        with pytest.raises(ValueError):
            call()
        assert file_of(ix, tmp_path / "b.ivf") == before
    # a view over the caller's own flat indexes: the caller owns those rows
    offs, orig = m.layout()
    rows, cflat = flat_of(m.stored_rows(), metric), flat_of(cents, metric)
    view = HipIVFIndex.from_parts(rows, cflat, offs, orig)
    q = m.x[:3]
    want = rows.search(q, 5), cflat.search(q, 2), view.search(q, 5, 2)
    for fn, args in ((view.add, (m.x[:2],)), (view.add, (torch.from_numpy(m.x[:2]).cuda(),)), (view.remove_ranges, ([[0, 1]],))):
        with pytest.raises(HipRagError) as e:
            fn(*args)
        assert e.value.code == E_UNSUPPORTED and "hipivf_create" in str(e.value) and "owns" in str(e.value)
    got = rows.search(q, 5), cflat.search(q, 2), view.search(q, 5, 2)
    assert all(np.array_equal(a, b) for u, v in zip(want, got) for a, b in zip(u, v))
    assert rows.ntotal == len(orig) and view.ntotal == m.n
    # the index still takes a good update
    ix.remove_ranges([[0, 1]])
    m.remove([[0, 1]])
    check_state(ix, m, tmp_path / "c.ivf", "after the refusals")


# ---- 7. determinism ------------------------------------------------------------------------------------------------------
def test_the_edge_script_gives_the_same_files_twice(gpu, tmp_path):
    cents = separated_centroids(NLIST, 36, seed=9)
    runs = []
    for run in range(2):
        ix, m = fresh(cents, ho.METRIC_IP)
        files = []
        for name, step in edge_script(cents, seed=41):
            step(ix, m)
            files.append(file_of(ix, tmp_path / f"r{run}.ivf"))
        runs.append(files)
    assert runs[0] == runs[1]
