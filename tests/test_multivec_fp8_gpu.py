"""
The fp8 format of the multi-vector store (hipmv_create_ex, hipmv_export_fp8, hipmv_to_fp8, hipmv_format_info, HIPMVQ81): after
any sequence of appends (from the device layout and from the host) and removals, export_fp8 equals the reference quantisation
(hiprag.fp8_quantize_reference) of the surviving vectors, byte for byte, and export its dequantisation; an exhaustive sweep of
bf16 patterns; the cap; conversion of a bf16 store; the file and its validation; refused calls change nothing.  The shapes are
test_multivec_gpu.py's.  Cases: tests/fp8_cases.py.
"""
import os

import numpy as np
import pytest

import fp8_cases as fc
from colbert_cases import csr_of, drop_ranges

pytestmark = pytest.mark.gpu

DIM = 128
CAP = 40
LENS = [0, 1, 31, 32, 33, CAP - 1, CAP, CAP + 1, CAP + 25, 0, 3, 17, 64, 7, 0, 12] * 2     # 32 documents
POISON = 0x7FC5


def _new(dim=DIM, cap=CAP):
    from hiprag import MultiVectorStore
    return MultiVectorStore(dim, max_doc_vectors=cap, format="fp8")


def _fresh(docs, cap=CAP, dim=DIM):
    st = _new(dim, cap)
    st.append(docs)
    return st


def _same(store, docs, cap=CAP, dim=DIM):
    """export_fp8 = the reference of the surviving vectors, export = its dequantisation, sizes as the bf16 store's."""
    from hiprag import fp8_dequantize
    off, codes, scales = store.export_fp8()
    eoff, ecodes, escales = fc.fp8_csr_of(docs, dim, cap)
    assert off.dtype == np.int64 and codes.dtype == np.uint8 and scales.dtype == np.float32
    assert np.array_equal(off, eoff) and codes.tobytes() == ecodes.tobytes() and scales.tobytes() == escales.tobytes()
    off2, vecs = store.export()
    assert np.array_equal(off2, eoff) and vecs.dtype == np.uint16 and vecs.tobytes() == fp8_dequantize(ecodes, escales).tobytes()
    n, nv, d, longest = store.sizes()
    assert (n, nv, d) == (len(docs), int(eoff[-1]), dim)
    assert longest == max([min(len(v), cap) for v in docs], default=0)
    assert store.format == "fp8" and store.format_info()[:2] == ("fp8", dim + 4)


def _device_block(docs, stride, dim=DIM):
    """The layout hipenc_forward_colbert writes: [n, stride, dim] with poison behind every count."""
    import torch
    block = np.full((len(docs), stride, dim), POISON, dtype=np.uint16)
    for i, v in enumerate(docs):
        block[i, :len(v)] = v
    t = torch.from_numpy(block.view(np.int16)).cuda().view(torch.bfloat16)
    return t, np.asarray([len(v) for v in docs], dtype=np.int32)


def test_append_remove_append_equals_the_reference_and_a_fresh_store(gpu):
    docs = fc.mixed_docs(LENS, DIM, 11)
    st = _new()
    _same(st, [])
    st.append(docs[:9])
    _same(st, docs[:9])
    st.append_device(*_device_block(docs[9:21], 70))    # from the device layout, poison behind the counts; grows
    _same(st, docs[:21])
    front = [a[:1].copy() for a in st.export_fp8()[1:]]
    ranges = [(0, 0), (2, 5), (5, 6), (9, 9), (12, 17), (20, 21)]      # empty, touching, a middle one, the last document
    st.remove_ranges(ranges)
    live = drop_ranges(docs[:21], ranges)
    _same(st, live)
    for a, b in zip(front, st.export_fp8()[1:]):
        assert a.tobytes() == b[:1].tobytes()           # in front of the first removed document nothing changed
    for a, b in zip(st.export_fp8(), _fresh(live).export_fp8()):
        assert a.tobytes() == b.tobytes()
    st.append_device(*_device_block(docs[21:], 65))
    live += docs[21:]
    _same(st, live)
    for a, b in zip(st.export_fp8(), _fresh(live).export_fp8()):
        assert a.tobytes() == b.tobytes()
    # nothing to remove: a no-op; an empty batch and empty documents: valid in both forms
    st.remove_ranges([])
    st.remove_ranges([(3, 3), (len(live), len(live))])
    st.append([])
    extra = [np.zeros((0, DIM), np.uint16), np.zeros((0, DIM), np.uint16), docs[2][:1]]
    st.append(extra[:2])
    st.append_device(*_device_block(extra[2:] + extra[:1], 1))
    live += extra[:2] + extra[2:] + extra[:1]
    _same(st, live)
    st.remove_ranges([(0, 1)])
    live = live[1:]
    _same(st, live)
    st.remove_ranges([(0, len(live))])
    _same(st, [])
    st.append(docs[3:9])                                # and it is usable again
    _same(st, docs[3:9])
    # the guard counts since creation, removed vectors included: every vector this store was ever given
    given = docs[:21] + docs[21:] + extra[2:] + docs[3:9]
    assert st.format_info()[2] == sum(fc.guarded_count(d[:CAP]) for d in given if len(d))


def test_both_append_forms_give_the_same_bytes_on_every_bf16_pattern(gpu):
    """The exhaustive case: first components fix e, the others sweep every bf16 bit pattern of magnitude <= amax."""
    vecs = np.concatenate([fc.exhaustive_vectors(DIM), fc.special_vectors(DIM)])
    lens = [37] * (len(vecs) // 37) + [len(vecs) % 37]
    docs, at = [], 0
    for n in lens:
        docs.append(vecs[at:at + n])
        at += n
    host = _fresh(docs)
    _same(host, docs)
    dev = _new()
    dev.append_device(*_device_block(docs, 37))
    _same(dev, docs)
    assert host.format_info()[2] == dev.format_info()[2] == fc.N_GUARDED_SPECIAL
    _, codes, _ = dev.export_fp8()
    assert not np.any((codes & 0x7F) == 0x7F) and not np.any(codes == 0x80)


def test_the_cap_is_applied_in_both_forms(gpu):
    docs = fc.mixed_docs(LENS, DIM, 5)
    for cap in (1, 32, CAP):
        _same(_fresh(docs, cap), docs, cap)
        st = _new(cap=cap)
        st.append_device(*_device_block(docs, max(LENS)))
        _same(st, docs, cap)


def test_wide_vectors_and_many_small_appends_across_reallocations(gpu):
    lens = (5, 0, 33, 2, 64, 1, 9, 40)
    docs = fc.mixed_docs(lens, 1024, 3)
    st = _new(1024, 48)
    for i, v in enumerate(docs):
        if i % 2:
            st.append([v])
        else:
            st.append_device(*_device_block([v], 64, 1024))
        _same(st, docs[:i + 1], 48, 1024)
    st.remove_ranges([(1, 3), (6, 7)])
    _same(st, drop_ranges(docs, [(1, 3), (6, 7)]), 48, 1024)


def test_to_fp8_equals_a_fresh_fp8_store_and_leaves_the_source(gpu):
    from hiprag import HipRagError, MultiVectorStore
    docs = fc.mixed_docs(LENS, DIM, 13)
    src = MultiVectorStore(DIM, max_doc_vectors=CAP)
    src.append(docs)
    before = [a.tobytes() for a in src.export()]
    conv = src.to_fp8()
    _same(conv, docs)
    for a, b in zip(conv.export_fp8(), _fresh(docs).export_fp8()):
        assert a.tobytes() == b.tobytes()
    assert conv.max_doc_vectors == CAP and conv.format_info()[2] == fc.guarded_count(csr_of(docs, DIM, CAP)[1])
    assert [a.tobytes() for a in src.export()] == before and src.format == "bf16" and src.format_info() == ("bf16", 2 * DIM, 0)
    conv.append(docs[:2])                               # the converted store is an ordinary store
    _same(conv, docs + docs[:2])
    empty = MultiVectorStore(DIM, max_doc_vectors=CAP).to_fp8()
    _same(empty, [])
    with pytest.raises(HipRagError) as e:
        conv.to_fp8()                                   # an fp8 store already
    assert e.value.code == -1
    with pytest.raises(HipRagError) as e:
        MultiVectorStore(64, max_doc_vectors=CAP).to_fp8()      # a dim fp8 does not take
    assert e.value.code == -1


def test_save_load_round_trip_and_bad_files(gpu, tmp_path):
    from hiprag import HipRagError, MultiVectorStore
    docs = fc.mixed_docs(LENS, DIM, 9)
    st = _fresh(docs)
    path = str(tmp_path / "store.mv")
    st.save(path)
    eoff, ecodes, escales = fc.fp8_csr_of(docs, DIM, CAP)
    nv = int(eoff[-1])
    assert os.path.getsize(path) == 40 + 8 * (len(docs) + 1) + 4 * nv + nv * DIM
    raw = open(path, "rb").read()
    assert raw[:8] == b"HIPMVQ81" and np.frombuffer(raw[8:24], np.int32).tolist() == [1, DIM, CAP, 1]
    assert np.frombuffer(raw[24:40], np.int64).tolist() == [len(docs), nv]
    o0, s0 = 40, 40 + 8 * len(eoff)
    c0 = s0 + 4 * nv
    assert raw[o0:s0] == eoff.tobytes() and raw[s0:c0] == escales.tobytes() and raw[c0:] == ecodes.tobytes()
    xoff, xcodes, xscales = st.export_fp8()             # the whole file, as the comment above hipmv_save lays it out
    assert raw == (b"HIPMVQ81" + np.asarray([1, DIM, CAP, 1], np.int32).tobytes() + np.asarray([len(docs), len(xscales)], np.int64).tobytes()
                   + xoff.tobytes() + xscales.tobytes() + xcodes.tobytes())
    back = MultiVectorStore.load(path)
    assert back.max_doc_vectors == CAP and back.format == "fp8"
    for a, b in zip(st.export_fp8(), back.export_fp8()):
        assert a.tobytes() == b.tobytes()
    _same(back, docs)
    back.append(docs[:3])                               # a loaded store is an ordinary store
    _same(back, docs + docs[:3])
    back.remove_ranges([(1, 4)])
    _same(back, drop_ranges(docs + docs[:3], [(1, 4)]))
    empty = str(tmp_path / "empty.mv")
    _new().save(empty)
    _same(MultiVectorStore.load(empty), [])
    # a bf16 file still loads as a bf16 store
    b16 = MultiVectorStore(DIM, max_doc_vectors=CAP)
    b16.append(docs[:4])
    b16.save(str(tmp_path / "b16.mv"))
    again = MultiVectorStore.load(str(tmp_path / "b16.mv"))
    assert again.format == "bf16" and [a.tobytes() for a in again.export()] == [a.tobytes() for a in b16.export()]

    def refused(data, name):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(HipRagError) as e:
            MultiVectorStore.load(p)
        assert e.value.code == -4, name

    refused(raw[:-2], "truncated.mv")
    refused(raw[:38], "short_header.mv")
    refused(raw + b"\0\0", "too_long.mv")
    first = int(np.flatnonzero(escales != 1.0)[0])
    for bad in (3.0, 0.0, -0.5, float("nan"), 2.0 ** -68, 2.0 ** 54):    # not a power of two, not positive, outside the domain
        sc = escales.copy()
        sc[first] = bad
        refused(raw[:s0] + sc.tobytes() + raw[c0:], f"scale_{bad}.mv")
    for pattern in (0x7F, 0xFF):                                         # a NaN code, either sign, in the last vector's last byte
        refused(raw[:-1] + bytes([pattern]), f"nan_{pattern}.mv")
    refused(raw[:c0] + bytes([0x7F]) + raw[c0 + 1:], "nan_first.mv")
    off = eoff.copy()
    off[3], off[4] = off[4], off[3]                     # descending offsets (documents 2..4 differ in length)
    assert off[3] > off[4]
    refused(raw[:o0] + off.tobytes() + raw[s0:], "descending.mv")
    refused(raw[:20] + np.asarray([0], np.int32).tobytes() + raw[24:], "format0.mv")
    refused(raw[:20] + np.asarray([2], np.int32).tobytes() + raw[24:], "format2.mv")
    refused(raw[:12] + np.asarray([DIM + 64], np.int32).tobytes() + raw[16:], "dim.mv")
    refused(b"HIPMV001" + raw[8:], "magic_of_the_other_kind.mv")


def test_refused_calls_leave_the_store_as_it_was(gpu):
    import torch
    from hiprag import HipRagError, MultiVectorStore
    from hiprag import _native as nat
    docs = fc.mixed_docs(LENS, DIM, 7)[:12]
    st = _fresh(docs)
    before = [a.tobytes() for a in st.export_fp8()]
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
    for ranges in ([(3, 2)], [(-1, 2)], [(0, 13)], [(4, 6), (5, 7)], [(6, 8), (1, 2)]):          # the range table rules
        with pytest.raises(HipRagError) as e:
            st.remove_ranges(ranges)
        assert e.value.code == -1
    with pytest.raises(HipRagError) as e:
        st.to_fp8()
    assert e.value.code == -1
    assert [a.tobytes() for a in st.export_fp8()] == before
    _same(st, docs)
    for dim in (64, 192, 96, 1152):                                                              # fp8 takes whole 128-byte lines
        with pytest.raises(HipRagError) as e:
            MultiVectorStore(dim, max_doc_vectors=8, format="fp8")
        assert e.value.code == -1
    import ctypes
    h = ctypes.c_uint64()
    for fmt in (2, -1):
        with pytest.raises(HipRagError) as e:
            nat.call("hipmv_create_ex", DIM, 8, 0, fmt, ctypes.byref(h))
        assert e.value.code == -1
    with pytest.raises(ValueError):
        MultiVectorStore(DIM, max_doc_vectors=8, format="fp4")
    b16 = MultiVectorStore(DIM, max_doc_vectors=CAP)
    b16.append(docs[:3])
    was = [a.tobytes() for a in b16.export()]
    with pytest.raises(HipRagError) as e:
        b16.export_fp8()                                                                         # no codes in a bf16 store
    assert e.value.code == -1
    assert [a.tobytes() for a in b16.export()] == was
    with pytest.raises(HipRagError) as e:
        nat.call("hipmv_format_info", 123456789, np.zeros(4, np.int64).ctypes.data)
    assert e.value.code == -3


def test_format_info_counts_guarded_vectors(gpu):
    st = _new()
    assert st.format_info() == ("fp8", DIM + 4, 0)
    special = fc.special_vectors(DIM)
    st.append([special])
    assert st.format_info() == ("fp8", DIM + 4, fc.N_GUARDED_SPECIAL)
    st.append_device(*_device_block([special[:CAP]], CAP))
    assert st.format_info()[2] == 2 * fc.N_GUARDED_SPECIAL
    st.remove_ranges([(0, 2)])
    assert st.format_info()[2] == 2 * fc.N_GUARDED_SPECIAL          # since creation: a removal takes nothing back
