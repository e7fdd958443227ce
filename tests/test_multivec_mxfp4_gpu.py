"""
The MXFP4 format of the multi-vector store (hipmv_create_ex format 4, hipmv_export_mxfp4, hipmv_to_mxfp4, hipmv_format_info,
HIPMVQ41): after any sequence of appends (from the device layout and from the host) and removals, export_mxfp4 equals the
reference quantisation (hiprag.mxfp4_quantize_reference) of the surviving vectors, byte for byte, and export its
dequantisation; every position of every block decides its scale; the cap; conversion of a bf16 store; the file and its
validation; refused calls change nothing.  Cases: tests/mxfp4_cases.py.
"""
import ctypes
import os

import numpy as np
import pytest

import mxfp4_cases as mc
from colbert_cases import csr_of, drop_ranges

pytestmark = pytest.mark.gpu

DIM = 128
CAP = 40
LENS = [0, 1, 5, 33, CAP - 1, CAP, CAP + 1, 0, 3, 17, 64, 7, 0, 12, 31, 32]     # 16 documents
POISON = 0x7FC5


def _new(dim=DIM, cap=CAP):
    from hiprag import MultiVectorStore
    return MultiVectorStore(dim, max_doc_vectors=cap, format="mxfp4")


def _fresh(docs, cap=CAP, dim=DIM):
    st = _new(dim, cap)
    st.append(docs)
    return st


def _same(store, docs, cap=CAP, dim=DIM):
    """export_mxfp4 = the reference of the surviving vectors, export = its dequantisation, sizes as the bf16 store's."""
    from hiprag import mxfp4_dequantize
    off, codes, scales = store.export_mxfp4()
    eoff, ecodes, escales = mc.mxfp4_csr_of(docs, dim, cap)
    assert off.dtype == np.int64 and codes.dtype == np.uint8 and scales.dtype == np.uint8
    assert codes.shape == ecodes.shape and scales.shape == escales.shape
    assert np.array_equal(off, eoff) and scales.tobytes() == escales.tobytes() and codes.tobytes() == ecodes.tobytes()
    off2, vecs = store.export()
    assert np.array_equal(off2, eoff) and vecs.dtype == np.uint16 and vecs.tobytes() == mxfp4_dequantize(ecodes, escales).tobytes()
    n, nv, d, longest = store.sizes()
    assert (n, nv, d) == (len(docs), int(eoff[-1]), dim)
    assert longest == max([min(len(v), cap) for v in docs], default=0)
    assert store.format == "mxfp4" and store.format_info()[:2] == ("mxfp4", dim // 2 + dim // 32)


def _device_block(docs, stride, dim=DIM):
    """The layout hipenc_forward_colbert writes: [n, stride, dim] with poison behind every count."""
    import torch
    block = np.full((len(docs), stride, dim), POISON, dtype=np.uint16)
    for i, v in enumerate(docs):
        block[i, :len(v)] = v
    t = torch.from_numpy(block.view(np.int16)).cuda().view(torch.bfloat16)
    return t, np.asarray([len(v) for v in docs], dtype=np.int32)


def _split(vecs, per):
    return [vecs[i:i + per] for i in range(0, len(vecs), per)]


@pytest.mark.parametrize("dim", (128, 384, 640, 1024))
def test_both_append_forms_give_the_reference_bytes(gpu, dim):
    """Unit vectors, small integers, the special vectors, vectors at many magnitudes, and documents of 0, 1, 5, 33 vectors."""
    special = mc.special_vectors(dim)
    vecs = np.concatenate([mc.unit_vectors(31 - len(special), dim, 1), mc.integer_vectors(8, dim, 2), special])
    docs = [vecs[:0], vecs[:1], vecs[1:6], vecs[6:39]] + mc.mixed_docs([0, 1, 5, 33], dim, dim)
    assert len(vecs) == 39 and [len(d) for d in docs] == [0, 1, 5, 33] * 2
    host = _fresh(docs, dim=dim)
    _same(host, docs, dim=dim)
    dev = _new(dim)
    dev.append_device(*_device_block(docs, 33, dim))
    _same(dev, docs, dim=dim)
    for a, b in zip(host.export_mxfp4(), dev.export_mxfp4()):
        assert a.tobytes() == b.tobytes()
    guarded = sum(mc.guarded_count(d) for d in docs if len(d))
    assert guarded >= mc.N_GUARDED_SPECIAL and host.format_info()[2] == dev.format_info()[2] == guarded
    _, codes, scales = dev.export_mxfp4()
    assert not np.any(mc.nibbles(codes) == 8) and scales.min() >= 27 and scales.max() <= 185
    again = _new(dim)                                    # the same bytes on every run
    again.append_device(*_device_block(docs, 40, dim))
    for a, b in zip(again.export_mxfp4(), dev.export_mxfp4()):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dim", (128, 1024))
def test_every_position_of_every_block_decides_its_scale(gpu, dim):
    vecs = mc.position_vectors(dim)
    docs = _split(vecs, 37)
    want = np.full((dim, dim // 32), 119, np.uint8)      # 2^-6 everywhere: E = -8
    want[np.arange(dim), np.arange(dim) // 32] = 125     # 1.0 at component p: E = -2 in its block, and only there
    for st in (_fresh(docs, dim=dim), _new(dim)):
        if st.sizes()[0] == 0:
            st.append_device(*_device_block(docs, 37, dim))
        _, codes, scales = st.export_mxfp4()
        assert np.array_equal(scales, want)
        assert np.all(mc.nibbles(codes)[np.arange(dim), np.arange(dim)] == 6)
        _same(st, docs, dim=dim)


def test_append_remove_append_equals_the_reference_and_a_fresh_store(gpu):
    docs = mc.mixed_docs(LENS * 2, DIM, 11)
    st = _new()
    _same(st, [])
    st.append(docs[:9])
    _same(st, docs[:9])
    st.append_device(*_device_block(docs[9:21], 70))    # from the device layout, poison behind the counts; grows
    _same(st, docs[:21])
    front = [a[:1].copy() for a in st.export_mxfp4()[1:]]
    ranges = [(0, 0), (2, 5), (5, 6), (9, 9), (12, 17), (20, 21)]      # empty, touching, a middle one, the last document
    st.remove_ranges(ranges)
    live = drop_ranges(docs[:21], ranges)
    _same(st, live)
    for a, b in zip(front, st.export_mxfp4()[1:]):
        assert a.tobytes() == b[:1].tobytes()           # in front of the first removed document nothing changed
    for a, b in zip(st.export_mxfp4(), _fresh(live).export_mxfp4()):
        assert a.tobytes() == b.tobytes()
    st.append_device(*_device_block(docs[21:], 65))
    live += docs[21:]
    _same(st, live)
    for a, b in zip(st.export_mxfp4(), _fresh(live).export_mxfp4()):
        assert a.tobytes() == b.tobytes()
    st.remove_ranges([])
    st.remove_ranges([(3, 3), (len(live), len(live))])
    st.append([])
    extra = [np.zeros((0, DIM), np.uint16), np.zeros((0, DIM), np.uint16), docs[2][:1]]
    st.append(extra[:2])
    st.append_device(*_device_block(extra[2:] + extra[:1], 1))
    live += extra[:2] + extra[2:] + extra[:1]
    _same(st, live)
    st.remove_ranges([(0, len(live))])
    _same(st, [])
    st.append(docs[3:9])                                # and it is usable again
    _same(st, docs[3:9])
    given = docs[:21] + docs[21:] + extra[2:] + docs[3:9]       # the guard counts since creation, removed vectors included
    assert st.format_info()[2] == sum(mc.guarded_count(d[:CAP]) for d in given if len(d))


def test_the_cap_is_applied_in_both_forms(gpu):
    docs = mc.mixed_docs(LENS, DIM, 5)
    for cap in (1, 32, CAP):
        _same(_fresh(docs, cap), docs, cap)
        st = _new(cap=cap)
        st.append_device(*_device_block(docs, max(LENS)))
        _same(st, docs, cap)


@pytest.mark.parametrize("dim", (384, 1024))
def test_wide_vectors_and_many_small_appends_across_reallocations(gpu, dim):
    lens = (5, 0, 33, 2, 64, 1, 9, 40)
    docs = mc.mixed_docs(lens, dim, 3)
    st = _new(dim, 48)
    for i, v in enumerate(docs):
        if i % 2:
            st.append([v])
        else:
            st.append_device(*_device_block([v], 64, dim))
        _same(st, docs[:i + 1], 48, dim)
    st.remove_ranges([(1, 3), (6, 7)])
    live = drop_ranges(docs, [(1, 3), (6, 7)])
    _same(st, live, 48, dim)
    for a, b in zip(st.export_mxfp4(), _fresh(live, 48, dim).export_mxfp4()):
        assert a.tobytes() == b.tobytes()


def test_to_mxfp4_equals_a_fresh_store_and_leaves_the_source(gpu):
    from hiprag import HipRagError, MultiVectorStore
    docs = mc.mixed_docs(LENS, DIM, 13)
    src = MultiVectorStore(DIM, max_doc_vectors=CAP)
    src.append(docs)
    before = [a.tobytes() for a in src.export()]
    conv = src.to_mxfp4()
    _same(conv, docs)
    for a, b in zip(conv.export_mxfp4(), _fresh(docs).export_mxfp4()):
        assert a.tobytes() == b.tobytes()
    assert conv.max_doc_vectors == CAP and conv.format_info()[2] == mc.guarded_count(csr_of(docs, DIM, CAP)[1])
    assert [a.tobytes() for a in src.export()] == before and src.format == "bf16" and src.format_info() == ("bf16", 2 * DIM, 0)
    conv.append(docs[:2])                               # the converted store is an ordinary store
    _same(conv, docs + docs[:2])
    _same(MultiVectorStore(DIM, max_doc_vectors=CAP).to_mxfp4(), [])
    wide = MultiVectorStore(640, max_doc_vectors=CAP)
    wdocs = mc.mixed_docs([3, 0, 33], 640, 14)
    wide.append(wdocs)
    _same(wide.to_mxfp4(), wdocs, dim=640)
    for refused in (conv.to_mxfp4, conv.to_fp8, src.to_fp8().to_mxfp4,                   # no second quantisation
                    MultiVectorStore(64, max_doc_vectors=CAP).to_mxfp4, MultiVectorStore(192, max_doc_vectors=CAP).to_mxfp4):
        with pytest.raises(HipRagError) as e:
            refused()
        assert e.value.code == -1
    _same(conv, docs + docs[:2])


def test_save_load_round_trip_and_bad_files(gpu, tmp_path):
    from hiprag import HipRagError, MultiVectorStore
    docs = mc.mixed_docs(LENS, DIM, 9)
    st = _fresh(docs)
    path = str(tmp_path / "store.mv")
    st.save(path)
    eoff, ecodes, escales = mc.mxfp4_csr_of(docs, DIM, CAP)
    nv = int(eoff[-1])
    assert os.path.getsize(path) == 40 + 8 * (len(docs) + 1) + nv * (DIM // 32) + nv * (DIM // 2)
    raw = open(path, "rb").read()
    assert raw[:8] == b"HIPMVQ41" and np.frombuffer(raw[8:24], np.int32).tolist() == [1, DIM, CAP, 4]
    assert np.frombuffer(raw[24:40], np.int64).tolist() == [len(docs), nv]
    o0, s0 = 40, 40 + 8 * len(eoff)
    c0 = s0 + nv * (DIM // 32)
    assert raw[o0:s0] == eoff.tobytes() and raw[s0:c0] == escales.tobytes() and raw[c0:] == ecodes.tobytes()
    back = MultiVectorStore.load(path)
    assert back.max_doc_vectors == CAP and back.format == "mxfp4"
    for a, b in zip(st.export_mxfp4(), back.export_mxfp4()):
        assert a.tobytes() == b.tobytes()
    _same(back, docs)
    back.append(docs[:3])                               # a loaded store is an ordinary store
    _same(back, docs + docs[:3])
    back.remove_ranges([(1, 4)])
    _same(back, drop_ranges(docs + docs[:3], [(1, 4)]))
    empty = str(tmp_path / "empty.mv")
    _new().save(empty)
    _same(MultiVectorStore.load(empty), [])
    wide = _fresh(mc.mixed_docs([3, 0, 33], 1024, 10), dim=1024)
    wide.save(str(tmp_path / "wide.mv"))
    for a, b in zip(wide.export_mxfp4(), MultiVectorStore.load(str(tmp_path / "wide.mv")).export_mxfp4()):
        assert a.tobytes() == b.tobytes()
    # the other two kinds still load as what they are
    b16 = MultiVectorStore(DIM, max_doc_vectors=CAP)
    b16.append(docs[:4])
    b16.save(str(tmp_path / "b16.mv"))
    again = MultiVectorStore.load(str(tmp_path / "b16.mv"))
    assert again.format == "bf16" and [a.tobytes() for a in again.export()] == [a.tobytes() for a in b16.export()]
    q8 = b16.to_fp8()
    q8.save(str(tmp_path / "q8.mv"))
    again = MultiVectorStore.load(str(tmp_path / "q8.mv"))
    assert again.format == "fp8" and [a.tobytes() for a in again.export_fp8()] == [a.tobytes() for a in q8.export_fp8()]

    def refused(data, name):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(HipRagError) as e:
            MultiVectorStore.load(p)
        assert e.value.code == -4, name                 # no handle comes back: the store is registered last

    refused(raw[:-2], "truncated.mv")
    refused(raw[:38], "short_header.mv")
    refused(raw + b"\0\0", "too_long.mv")
    for fmt in (0, 1, 2):
        refused(raw[:20] + np.asarray([fmt], np.int32).tobytes() + raw[24:], f"format{fmt}.mv")
    first = int(np.flatnonzero(escales.reshape(-1) != 127)[0])
    for bad in (26, 186, 0, 255):                                         # outside [27, 185]
        sc = escales.reshape(-1).copy()
        sc[first] = bad
        refused(raw[:s0] + sc.tobytes() + raw[c0:], f"scale_{bad}.mv")
    for ok in (27, 185):                                                  # the edges are inside
        sc = escales.reshape(-1).copy()
        sc[first] = ok
        p = str(tmp_path / f"scale_{ok}.mv")
        open(p, "wb").write(raw[:s0] + sc.tobytes() + raw[c0:])
        assert MultiVectorStore.load(p).export_mxfp4()[2].reshape(-1)[first] == ok
    last = raw[-1]
    refused(raw[:-1] + bytes([(last & 0x0F) | 0x80]), "neg_zero_high_nibble_last.mv")
    refused(raw[:-1] + bytes([(last & 0xF0) | 0x08]), "neg_zero_low_nibble_last.mv")
    refused(raw[:c0] + bytes([0x08]) + raw[c0 + 1:], "neg_zero_first.mv")
    off = eoff.copy()
    off[3], off[4] = off[4], off[3]                     # descending offsets (documents 2..4 differ in length)
    assert off[3] > off[4]
    refused(raw[:o0] + off.tobytes() + raw[s0:], "descending.mv")
    refused(raw[:12] + np.asarray([DIM + 64], np.int32).tobytes() + raw[16:], "dim.mv")
    refused(b"HIPMVQ81" + raw[8:], "magic_of_fp8.mv")
    refused(b"HIPMV001" + raw[8:], "magic_of_bf16.mv")


def test_refused_calls_leave_the_store_as_it_was(gpu):
    import torch
    from hiprag import HipRagError, MultiVectorStore
    from hiprag import _native as nat
    docs = mc.mixed_docs(LENS, DIM, 7)[:12]
    st = _fresh(docs)
    before = [a.tobytes() for a in st.export_mxfp4()]
    ok = np.zeros((4, DIM), np.uint16)
    for offsets in (np.asarray([1, 2, 4], np.int64), np.asarray([0, 3, 2, 4], np.int64)):       # start, descent
        with pytest.raises(HipRagError) as e:
            st.append(ok, offsets)
        assert e.value.code == -1
    block = torch.zeros((2, 8, DIM), dtype=torch.bfloat16, device="cuda")
    for counts in ([3, 9], [-1, 2]):                                                             # count outside [0, row_stride]
        with pytest.raises(HipRagError) as e:
            st.append_device(block, counts)
        assert e.value.code == -1
    for ranges in ([(3, 2)], [(-1, 2)], [(0, 13)], [(4, 6), (5, 7)]):                            # the range table rules
        with pytest.raises(HipRagError) as e:
            st.remove_ranges(ranges)
        assert e.value.code == -1
    for refused in (st.export_fp8, st.to_fp8, st.to_mxfp4):
        with pytest.raises(HipRagError) as e:
            refused()
        assert e.value.code == -1
    assert [a.tobytes() for a in st.export_mxfp4()] == before
    _same(st, docs)
    for dim in (64, 192, 1152):                                                                  # whole 32-bit words of scales
        with pytest.raises(HipRagError) as e:
            MultiVectorStore(dim, max_doc_vectors=8, format="mxfp4")
        assert e.value.code == -1
    h = ctypes.c_uint64()
    for fmt in (2, 3, 5, -1):
        with pytest.raises(HipRagError) as e:
            nat.call("hipmv_create_ex", DIM, 8, 0, fmt, ctypes.byref(h))
        assert e.value.code == -1
    with pytest.raises(ValueError):
        MultiVectorStore(DIM, max_doc_vectors=8, format="fp4")
    b16 = MultiVectorStore(DIM, max_doc_vectors=CAP)
    b16.append(docs[:3])
    q8 = b16.to_fp8()
    was = [a.tobytes() for a in b16.export()], [a.tobytes() for a in q8.export_fp8()]
    for refused in (b16.export_mxfp4, q8.export_mxfp4, q8.to_mxfp4):                             # no e2m1 codes in these
        with pytest.raises(HipRagError) as e:
            refused()
        assert e.value.code == -1
    assert ([a.tobytes() for a in b16.export()], [a.tobytes() for a in q8.export_fp8()]) == was
    # any pointer of the export may be NULL
    n, nv, _, _ = st.sizes()
    codes = np.zeros((nv, DIM // 2), np.uint8)
    nat.call("hipmv_export_mxfp4", st._h, None, codes.ctypes.data, None)
    assert codes.tobytes() == before[1]
    nat.call("hipmv_export_mxfp4", st._h, None, None, None)


def test_format_info_counts_guarded_vectors(gpu):
    st = _new()
    assert st.format_info() == ("mxfp4", DIM // 2 + DIM // 32, 0)
    special = mc.special_vectors(DIM)
    st.append([special])
    assert st.format_info() == ("mxfp4", 68, mc.N_GUARDED_SPECIAL)
    st.append_device(*_device_block([special], CAP))
    assert st.format_info()[2] == 2 * mc.N_GUARDED_SPECIAL
    st.remove_ranges([(0, 2)])
    assert st.format_info()[2] == 2 * mc.N_GUARDED_SPECIAL          # since creation: a removal takes nothing back
    wide = _new(1024)
    assert wide.format_info() == ("mxfp4", 544, 0)
