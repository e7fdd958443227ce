"""
Centroid codes on the multi-vector store (hipmv_attach_centroids and its neighbours, csrc/maxsim_codes.hip).  The data are
vectors bf16(unit(centroid + 0.25 unit noise)): test_maxsim_pruned_cpu.py shows their best and second-best float64 dots lie
>= 0.36 apart at 64-d and 128-d with 256 centroids; every case here measures that gap on the values the store returns
(gather_f32: dequantised on an fp8 or MXFP4 store), requires it to be above 100 times the fp32 accumulation error of a
product, and then requires the codes to EQUAL the float64 argmax.
"""
import ctypes
import functools

import numpy as np
import pytest

import pruned_cases as pc
from oracle.linear_cases import bf16_values

pytestmark = pytest.mark.gpu

CAP = 40
LENGTHS = (0, 1, 31, 32, 33, CAP + 5, 7, 40, 0, 19, 32, 5)      # CAP + 5 is cut to the cap; 207 stored vectors: two blocks of 128
CASES = [(dim, fmt, ncent) for dim, fmts in ((64, ("bf16",)), (128, ("bf16", "fp8", "mxfp4")), (1024, ("bf16", "fp8", "mxfp4")))
         for fmt in fmts for ncent in (32, 96, 1024)]


@functools.lru_cache(maxsize=None)
def _data(dim, ncent, seed=11):
    cent = pc.random_centroids(ncent, dim, seed)
    docs, drawn = pc.clustered_docs(cent, LENGTHS, seed + 1)
    return cent, docs, np.concatenate([d[:CAP] for d in drawn])      # the centroid every STORED vector was drawn around


def _store(dim, fmt, docs=None):
    from hiprag import MultiVectorStore
    s = MultiVectorStore(dim, max_doc_vectors=CAP, format=fmt)
    if docs is not None:
        s.append(docs)
    return s


def _stored_values(store):
    nv = store.sizes()[1]
    return store.gather_f32(np.arange(nv, dtype=np.int64)).cpu().numpy()


def _assert_codes_are_the_argmax(store, cent, dim):
    from hiprag.colbert import centroid_codes_reference
    vals, c = _stored_values(store), bf16_values(cent)
    gap = pc.top2_margin(vals, c)
    print(f"top-2 gap of the stored values: {gap:.4f}; accumulation bound {pc.product_tolerance(dim):.2e}")
    assert gap > 100 * pc.product_tolerance(dim)
    codes = store.codes()
    assert codes.dtype == np.int32 and len(codes) == len(vals)
    assert np.array_equal(codes, centroid_codes_reference(vals, c))


@pytest.mark.parametrize("dim,fmt,ncent", CASES)
def test_codes_equal_the_float64_argmax_of_the_stored_values(gpu, dim, fmt, ncent):
    cent, docs, _ = _data(dim, ncent)
    store = _store(dim, fmt, docs)
    assert store.centroid_info() == (0, 0, 0)
    store.attach_centroids(cent)
    nv = store.sizes()[1]
    assert nv == sum(min(n, CAP) for n in LENGTHS) and store.centroid_info() == (ncent, nv, 4 * nv)
    assert np.array_equal(store.centroids(), cent)
    _assert_codes_are_the_argmax(store, cent, dim)


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
def test_equal_centroids_give_the_lower_index_and_a_zero_vector_code_zero(gpu, fmt):
    dim, ncent = 128, 96
    cent, docs, drawn = _data(dim, ncent)
    cent = cent.copy()
    cent[40], cent[77] = cent[5], cent[5]                          # three centroids with identical bits, in different tiles
    store = _store(dim, fmt, list(docs) + [np.zeros((3, dim), np.uint16)])
    store.attach_centroids(cent)
    codes = store.codes()
    assert 40 not in codes.tolist() and 77 not in codes.tolist()
    assert codes[-3:].tolist() == [0, 0, 0]                         # every product is 0: the lowest centroid
    kept = ~np.isin(drawn, (40, 77))                                # the vectors that still have their centroid
    assert np.array_equal(codes[:-3][kept], drawn[kept])


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
def test_attaching_before_or_after_appending_gives_the_same_codes(gpu, fmt):
    import torch
    dim, ncent = 128, 96
    cent, docs, _ = _data(dim, ncent)
    after = _store(dim, fmt, docs)
    after.attach_centroids(cent)
    before = _store(dim, fmt)
    before.attach_centroids(cent)                                   # an empty store
    assert before.codes().shape == (0,)
    before.append(docs[:4])
    before.append(docs[4:])                                         # grows the arrays: the codes of the first batch stay
    assert np.array_equal(before.codes(), after.codes())
    # the device append codes its vectors too
    dev = _store(dim, fmt)
    dev.attach_centroids(cent)
    rows = np.zeros((len(docs), CAP + 5, dim), np.uint16)
    for i, d in enumerate(docs):
        rows[i, :len(d)] = d
    dev.append_device(torch.from_numpy(rows.view(np.int16)).cuda().view(torch.bfloat16), np.asarray([len(d) for d in docs], np.int32))
    assert np.array_equal(dev.codes(), after.codes()) and dev.sizes() == after.sizes()


def test_an_append_that_grows_the_arrays_keeps_the_earlier_codes(gpu):
    dim, ncent = 128, 96
    cent, docs, _ = _data(dim, ncent)
    store = _store(dim, "bf16", docs[:3])
    store.attach_centroids(cent)
    first = store.codes().copy()
    for _ in range(4):                                              # 4 x 207 vectors behind 32: several regrowths
        store.append(docs)
    codes = store.codes()
    assert np.array_equal(codes[:len(first)], first)
    _assert_codes_are_the_argmax(store, cent, dim)


def _search_rows(store, qv, qc, n_docs):
    """every search entry over the whole store: exact pairs, the scoped search, the pruned search and its candidates"""
    from hiprag import maxsim, maxsim_search, maxsim_search_pruned
    if n_docs == 0:
        return []
    scopes, soq = [[(0, n_docs)]], np.zeros(len(qc), np.int32)
    cand = np.tile(np.arange(min(n_docs, 256), dtype=np.int64), (len(qc), 1))
    out = list(maxsim(store, qv, qc, cand, k=min(5, cand.shape[1])))
    out += list(maxsim_search(store, qv, qc, scopes, soq, 5))
    out += list(maxsim_search_pruned(store, qv, qc, scopes, soq, 5, 8, want_candidates=True))
    return [np.asarray(a).tobytes() for a in out]


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
@pytest.mark.parametrize("ranges", [[(0, 3)], [(4, 7)], [(9, 12)], [(0, 2), (5, 6), (10, 12)], [(0, 12)]])
def test_after_a_removal_the_store_is_a_fresh_store_of_the_survivors(gpu, fmt, ranges):
    dim, ncent = 128, 96
    cent, docs, _ = _data(dim, ncent)
    store = _store(dim, fmt, docs)
    store.attach_centroids(cent)
    store.remove_ranges(ranges)
    gone = {d for lo, hi in ranges for d in range(lo, hi)}
    left = [d for i, d in enumerate(docs) if i not in gone]
    fresh = _store(dim, fmt, left) if left else _store(dim, fmt)
    fresh.attach_centroids(cent)
    assert store.sizes() == fresh.sizes() and store.centroid_info() == fresh.centroid_info()
    assert np.array_equal(store.codes(), fresh.codes())
    assert all(np.array_equal(a, b) for a, b in zip(store.export(), fresh.export()))
    rng = np.random.default_rng(5)
    qv = pc.vectors_around(cent, rng.integers(0, ncent, size=2 * 9), rng).reshape(2, 9, dim)
    qc = np.asarray([9, 4], np.int32)
    assert _search_rows(store, qv, qc, len(left)) == _search_rows(fresh, qv, qc, len(left))
    store.append(docs[:2])                                          # and it goes on as one
    fresh.append(docs[:2])
    assert np.array_equal(store.codes(), fresh.codes())


def test_a_second_attach_replaces_the_table_and_detach_makes_the_pruned_entry_refuse(gpu):
    from hiprag import HipRagError, maxsim_search_pruned
    dim = 128
    cent_a, docs, _ = _data(dim, 96)
    cent_b = pc.random_centroids(32, dim, 99)
    store = _store(dim, "bf16", docs)
    store.attach_centroids(cent_a)
    codes_a = store.codes().copy()
    store.attach_centroids(cent_b)
    assert store.centroid_info()[0] == 32 and np.array_equal(store.centroids(), cent_b)
    only_b = _store(dim, "bf16", docs)
    only_b.attach_centroids(cent_b)
    assert np.array_equal(store.codes(), only_b.codes()) and store.codes().max() < 32 and not np.array_equal(store.codes(), codes_a)
    qv, qc = docs[3][None, :8].copy(), np.asarray([8], np.int32)
    assert maxsim_search_pruned(store, qv, qc, [[(0, len(docs))]], [0], 2, 4)[1][0, 0] >= 0
    store.detach_centroids()
    assert store.centroid_info() == (0, 0, 0)
    for call in (lambda: maxsim_search_pruned(store, qv, qc, [[(0, len(docs))]], [0], 2, 4), store.codes, store.centroids):
        with pytest.raises(HipRagError) as e:
            call()
        assert e.value.code == -6 and "centroids" in str(e.value)
    store.detach_centroids()                                        # again: no error
    store.append(docs[:2])                                          # an unattached store appends as before
    # what comes out of a file or a conversion is unattached
    only_b_q = only_b.to_fp8()
    assert only_b_q.centroid_info() == (0, 0, 0) and only_b.to_mxfp4().centroid_info() == (0, 0, 0)


def test_a_loaded_store_is_unattached_and_reattaching_restores_the_codes(gpu, tmp_path):
    from hiprag import MultiVectorStore
    dim, ncent = 128, 96
    cent, docs, _ = _data(dim, ncent)
    store = _store(dim, "fp8", docs)
    plain = _store(dim, "fp8", docs)
    store.attach_centroids(cent)
    store.save(str(tmp_path / "a.mv"))
    plain.save(str(tmp_path / "b.mv"))
    assert (tmp_path / "a.mv").read_bytes() == (tmp_path / "b.mv").read_bytes()      # the file does not know of centroids
    back = MultiVectorStore.load(str(tmp_path / "a.mv"))
    assert back.centroid_info() == (0, 0, 0)
    back.attach_centroids(cent)
    assert np.array_equal(back.codes(), store.codes())


@pytest.mark.parametrize("fmt,dim", [("bf16", 64), ("bf16", 1024), ("fp8", 128), ("mxfp4", 128), ("mxfp4", 1024)])
def test_gather_returns_the_stored_values(gpu, fmt, dim):
    _, docs, _ = _data(dim, 32)
    store = _store(dim, fmt, docs)
    stored = bf16_values(store.export()[1])
    idx = np.asarray([206, 0, 5, 5, 128, 127, 33], np.int64)
    assert np.array_equal(store.gather_f32(idx).cpu().numpy(), stored[idx])
    assert np.array_equal(_stored_values(store), stored)
    assert store.gather_f32([]).shape == (0, dim)


def test_every_check_refuses_with_nothing_written(gpu):
    import torch
    from hiprag import HipRagError
    from hiprag import _native as nat
    dim = 128
    cent, docs, _ = _data(dim, 96)
    store = _store(dim, "bf16", docs)
    store.attach_centroids(cent)
    codes = store.codes().copy()
    for bad in (np.zeros((0, dim), np.uint16), cent[:31], cent[:48], np.zeros((65536 + 32, dim), np.uint16)):
        with pytest.raises(HipRagError) as e:
            store.attach_centroids(bad)
        assert e.value.code == -1 and "ncent" in str(e.value)
    with pytest.raises(ValueError):
        store.attach_centroids(cent[:, :64])
    with pytest.raises(HipRagError):
        nat.call("hipmv_attach_centroids", store._h, None, 96)
    assert store.centroid_info()[0] == 96 and np.array_equal(store.codes(), codes) and np.array_equal(store.centroids(), cent)
    nv = store.sizes()[1]
    out = torch.full((3, dim), 7.0, dtype=torch.float32, device="cuda")
    for bad in ([0, nv, 1], [0, -1, 1]):
        ix = np.asarray(bad, np.int64)
        with pytest.raises(HipRagError) as e:
            nat.call("hipmv_gather_f32_dev", store._h, ix.ctypes.data, 3, out.data_ptr())
        assert "no stored vector" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(HipRagError):
        nat.call("hipmv_centroid_info", ctypes.c_uint64(12345), np.zeros(4, np.int64).ctypes.data)
