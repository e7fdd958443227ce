"""
The multi-vector store (hipmv_*) at every width of tests/maxsim_width_cases.py, plus the 1024-d bf16 store and a 128-d fp8
store for contrast: append from padded rows (the device layout) and from packed rows (the host form), export and export_fp8,
to_fp8, remove_ranges followed by append, save and load with the whole file image.  For fp8 the codes and scales must be, byte
for byte, those of fp8_cases.quantize (the integer restatement of the format) on unit vectors, integer vectors,
special_vectors(dim) and the lane sweep, in which the largest magnitude sits alone in value 16 l for every lane l < dim / 16
of the quantiser in turn: a reduction of amax that loses any lane stores another scale.  At 128-d only lanes 0 .. 7 live.
"""
import numpy as np
import pytest

import fp8_cases as fc
import maxsim_width_cases as wc
from colbert_cases import csr_of, drop_ranges
from oracle.linear_cases import bf16_bits, bf16_values

pytestmark = pytest.mark.gpu

CAP = 40
POISON = 0x7FC5
STORE_SETS = [(d, "bf16") for d in wc.BF16_WIDTHS + (1024,)] + [(d, "fp8") for d in (128,) + wc.FP8_WIDTHS]


def _documents(dim):
    """The store vectors cut into documents of 1, 0, 17, 18 and 17 vectors (the last: the special vectors), one of 48 unit
    vectors that the cap cuts to 40, and the lane sweep in documents of its own (two from 656-d on)."""
    vecs = wc.store_vectors(dim)
    sweep = dim // 16
    head, lanes = vecs[:len(vecs) - sweep], vecs[len(vecs) - sweep:]
    assert len(head) == 53
    cuts = [0, 1, 1, 18, 36, 53]
    docs = [head[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    docs.append(np.concatenate([head[:24], head[23::-1]]))
    docs += [lanes[i:i + CAP] for i in range(0, sweep, CAP)]
    return docs


def _gone(n):
    return [(0, 0), (1, 3), (3, 4), (n - 1, n)]                 # empty, touching, the last document (lanes of the sweep)


def _device_block(docs, stride, dim):
    import torch
    block = np.full((len(docs), stride, dim), POISON, dtype=np.uint16)
    for i, v in enumerate(docs):
        block[i, :len(v)] = v[:stride]
    t = torch.from_numpy(block.view(np.int16)).cuda().view(torch.bfloat16)
    return t, np.asarray([min(len(v), stride) for v in docs], dtype=np.int32)


def _same(store, docs, dim, fmt):
    """The store holds `docs` under the cap: bf16 the vectors themselves; fp8 the codes and scales of fp8_cases.quantize, and
    export() their dequantisation, byte for byte."""
    eoff, evecs = csr_of(docs, dim, CAP)
    off, vecs = store.export()
    assert off.dtype == np.int64 and vecs.dtype == np.uint16 and np.array_equal(off, eoff)
    n, nv, d, longest = store.sizes()
    assert (n, nv, d) == (len(docs), int(eoff[-1]), dim) and longest == max([min(len(v), CAP) for v in docs], default=0)
    if fmt == "bf16":
        assert vecs.tobytes() == evecs.tobytes()
        assert store.format_info()[:2] == ("bf16", 2 * dim)
        return
    ecodes, escales = fc.quantize(evecs)
    off2, codes, scales = store.export_fp8()
    assert np.array_equal(off2, eoff) and codes.dtype == np.uint8 and scales.dtype == np.float32
    assert scales.tobytes() == escales.tobytes(), np.flatnonzero(scales != escales)[:8]
    assert codes.tobytes() == ecodes.tobytes(), np.flatnonzero((codes != ecodes).any(axis=1))[:8]
    deq = fc.dequantized(ecodes, escales)
    assert np.array_equal(bf16_values(vecs).astype(np.float64), deq)               # the values ...
    assert vecs.tobytes() == bf16_bits(deq.astype(np.float32)).tobytes()           # ... and the bits (no -0: the codes hold none)
    assert store.format_info()[:2] == ("fp8", dim + 4)


def _image(store, docs, dim, fmt):
    """The whole file as the comment above hipmv_save lays it out, from the expected arrays."""
    eoff, evecs = csr_of(docs, dim, CAP)
    counts = np.asarray([len(docs), int(eoff[-1])], np.int64).tobytes()
    if fmt == "bf16":
        return b"HIPMV001" + np.asarray([1, dim, CAP], np.int32).tobytes() + counts + eoff.tobytes() + evecs.tobytes()
    ecodes, escales = fc.quantize(evecs)
    return b"HIPMVQ81" + np.asarray([1, dim, CAP, 1], np.int32).tobytes() + counts + eoff.tobytes() + escales.tobytes() + ecodes.tobytes()


@pytest.mark.parametrize("dim,fmt", STORE_SETS)
def test_append_export_remove_save_and_load_at_every_width(gpu, dim, fmt, tmp_path):
    from hiprag import MultiVectorStore
    docs = _documents(dim)
    assert max(len(v) for v in docs) > CAP and any(len(v) == 0 for v in docs)
    guarded = lambda ds: sum(fc.guarded_count(v[:CAP]) for v in ds if len(v))
    assert guarded(docs) == fc.N_GUARDED_SPECIAL
    packed = MultiVectorStore(dim, max_doc_vectors=CAP, format=fmt)
    packed.append(docs)                                                              # packed rows, one call
    _same(packed, docs, dim, fmt)
    padded = MultiVectorStore(dim, max_doc_vectors=CAP, format=fmt)
    padded.append_device(*_device_block(docs[:4], 33, dim))                          # padded rows, poison behind the counts
    padded.append_device(*_device_block(docs[4:], 70, dim))
    _same(padded, docs, dim, fmt)
    if fmt == "fp8":
        assert packed.format_info()[2] == padded.format_info()[2] == guarded(docs)
    # removal, then an append of both forms
    gone = _gone(len(docs))
    live = drop_ranges(docs, gone)
    extra = [docs[5][7:30], docs[-1][::-1].copy()]
    for st in (packed, padded):
        st.remove_ranges(gone)
        _same(st, live, dim, fmt)
    packed.append(extra)
    padded.append_device(*_device_block(extra, 64, dim))
    now = live + extra
    for st in (packed, padded):
        _same(st, now, dim, fmt)
    if fmt == "fp8":                                                                 # since creation, removed vectors included
        assert packed.format_info()[2] == padded.format_info()[2] == guarded(docs) + guarded(extra)
    # the file
    path = str(tmp_path / "store.mv")
    packed.save(path)
    raw = open(path, "rb").read()
    assert raw == _image(packed, now, dim, fmt)
    back = MultiVectorStore.load(path)
    assert back.format == fmt and back.max_doc_vectors == CAP and back.dim == dim
    _same(back, now, dim, fmt)
    back.remove_ranges([(0, 2)])
    back.append(docs[:2])                                                            # a loaded store is an ordinary store
    _same(back, now[2:] + docs[:2], dim, fmt)
    other = str(tmp_path / "other.mv")
    padded.save(other)
    assert open(other, "rb").read() == raw


@pytest.mark.parametrize("dim", (128,) + wc.FP8_WIDTHS)
def test_to_fp8_at_every_width(gpu, dim):
    from hiprag import MultiVectorStore
    docs = _documents(dim)
    src = MultiVectorStore(dim, max_doc_vectors=CAP)
    src.append(docs)
    before = [a.tobytes() for a in src.export()]
    conv = src.to_fp8()
    _same(conv, docs, dim, "fp8")
    assert conv.format_info()[2] == fc.guarded_count(csr_of(docs, dim, CAP)[1]) and conv.max_doc_vectors == CAP
    assert [a.tobytes() for a in src.export()] == before and src.format_info() == ("bf16", 2 * dim, 0)
    conv.remove_ranges([(2, 4)])
    conv.append(docs[2:4])
    _same(conv, docs[:2] + docs[4:] + docs[2:4], dim, "fp8")


@pytest.mark.parametrize("dim", (128,) + wc.FP8_WIDTHS)
def test_every_lane_of_the_quantiser_decides_the_scale(gpu, dim):
    """The lane sweep alone, through all three ways into an fp8 store, against the scale written out by hand: vector l's
    largest value stands in lane l, so its scale is 2^(floor(log2 |that value|) - 7), whatever the other lanes hold."""
    from hiprag import MultiVectorStore
    bits = wc.lane_sweep_vectors(dim)
    n = dim // 16
    peak = bf16_values(bits[np.arange(n), 16 * np.arange(n)]).astype(np.float64)
    want = np.ldexp(1.0, np.floor(np.log2(np.abs(peak))).astype(np.int64) - 7).astype(np.float32)
    ecodes, escales = fc.quantize(bits)
    assert escales.tobytes() == want.tobytes()
    host = MultiVectorStore(dim, max_doc_vectors=n, format="fp8")
    host.append([bits])
    dev = MultiVectorStore(dim, max_doc_vectors=n, format="fp8")
    dev.append_device(*_device_block([bits], n + 3, dim))
    src = MultiVectorStore(dim, max_doc_vectors=n)
    src.append([bits])
    for name, st in (("host", host), ("device", dev), ("to_fp8", src.to_fp8())):
        _, codes, scales = st.export_fp8()
        wrong = np.flatnonzero(scales != want)
        assert not len(wrong), (name, dim, "lanes", wrong.tolist())
        assert codes.tobytes() == ecodes.tobytes(), (name, dim)
        assert st.format_info()[2] == 0
