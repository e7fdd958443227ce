"""
The MXFP4 multi-vector store inside the drop-in (HIP_COLBERT_FORMAT=mxfp4 with HIP_LATE_INTERACTION=true and
HIP_COLLECTION=true): the collection's store is created as MXFP4 and follows index_chunks, delete_document and
replace_document -- always equal to the reference quantisation (hiprag.mxfp4_quantize_reference) of the head outputs of the
surviving rows, which a bf16 collection of the same documents holds bit for bit; the manifest names the format and the file
is a HIPMVQ41, a mismatch raises; the retriever orders by the MXFP4 MaxSim; convert_multivectors("mxfp4") gives the bytes and
files of an MXFP4 ingest, a cold cache loads them, and an fp8 collection refuses the conversion.  The tiny synthetic model of
test_colbert_overlay_gpu.py.
"""
import asyncio
import json

import numpy as np
import pytest

from colbert_cases import maxsim_expected
from oracle.linear_cases import bf16_values

pytestmark = pytest.mark.gpu

DEPTH, TOP_K, MAX_PAGES, L = 12, 5, 3, 128
DOCS = [("docA", "red", 11), ("docB", "blue", 9), ("docC", "red", 10)]
WORDS = [f"w{j}" for j in range(40)]
QUERY = "w3 w17\nw5 w8 w21"


def _texts(n, seed):
    rng = np.random.default_rng(seed)
    out = [f"c{i} " + " ".join(rng.choice(WORDS, size=1 + (i * 7) % 37)) for i in range(n)]
    out[1] = ""                                          # a blank chunk is encoded as "": bos + eos, one vector
    return out


def _index_doc(storage, provider, doc, texts, project, replace=False):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=storage, provider=provider, with_sparse=False, project=project,
                                    replace=replace))


@pytest.fixture()
def world(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from hiprag import EncoderConfig, HipEncoder, random_state
    from rag.providers.hip.embeddings import HipEmbeddingProvider
    from rag.providers.hip.tokenizer import HashTokenizer
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setattr(hi.config, "RERANKER_TOP_K", TOP_K)
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    for name in ("HIP_RERANK", "HIP_PAGES", "HIP_LATE_INTERACTION", "HIP_SPARSE_MODE", "HIP_COLBERT_LINEAR", "HIP_COLBERT_FORMAT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    cfg = EncoderConfig(vocab=2000, hidden=128, layers=2, heads=2, ffn=256, max_pos=200, max_seq_len=L)
    provider = HipEmbeddingProvider(encoder=HipEncoder(cfg, random_state(cfg, seed=9)), tokenizer=HashTokenizer(cfg.vocab))
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: provider)
    texts = {doc: _texts(n, 800 + j) for j, (doc, _p, n) in enumerate(DOCS)}

    def use(name, fmt):
        """the storage directory `name`, late interaction on, HIP_COLBERT_FORMAT = fmt (None: unset), every cache cleared"""
        storage = tmp_path / name
        storage.mkdir(exist_ok=True)
        monkeypatch.setenv("STORAGE_DIR", str(storage))
        monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
        if fmt is None:
            monkeypatch.delenv("HIP_COLBERT_FORMAT", raising=False)
        else:
            monkeypatch.setenv("HIP_COLBERT_FORMAT", fmt)
        hi.clear_caches()
        return storage

    return dict(rt=rt, hi=hi, provider=provider, texts=texts, use=use, monkeypatch=monkeypatch)


def _ingest_all(w, storage):
    for doc, project, _n in DOCS:
        _index_doc(storage, w["provider"], doc, w["texts"][doc], project)


def _is_reference_of(q4_store, bf16_store):
    """the MXFP4 store holds the reference quantisation of the bf16 store's vectors (the head outputs), byte for byte"""
    from hiprag import mxfp4_dequantize, mxfp4_quantize_reference
    off, codes, scales = q4_store.export_mxfp4()
    boff, vecs = bf16_store.export()
    ecodes, escales = mxfp4_quantize_reference(vecs)
    assert np.array_equal(off, boff) and codes.tobytes() == ecodes.tobytes() and scales.tobytes() == escales.tobytes()
    assert q4_store.export()[1].tobytes() == mxfp4_dequantize(ecodes, escales).tobytes()
    assert np.abs(bf16_values(vecs)).max() > 0.05 and codes.any()             # unit vectors, not an empty comparison


def _kind(path):
    return open(path, "rb").read(8)


def test_ingest_delete_and_replace_keep_the_reference_quantisation(world):
    w = world
    from hiprag import MultiVectorStore
    from rag.storage.hip_index import collection as col
    new_a = _texts(7, 999)
    history = (("q", "mxfp4"), ("b", None))                                   # the same history under both formats
    dirs = {}
    for name, fmt in history:
        dirs[name] = w["use"](name, fmt)
        _ingest_all(w, dirs[name])
    manifest = json.load(open(dirs["q"] / col.COLLECTION_MANIFEST))
    assert manifest["mv"] == {"dim": 128, "format": "mxfp4"} and _kind(dirs["q"] / col.COLLECTION_MV) == b"HIPMVQ41"
    assert json.load(open(dirs["b"] / col.COLLECTION_MANIFEST))["mv"] == {"dim": 128}
    full = col.open_collection(dirs["q"]).mv
    assert full.format == "mxfp4" and full.format_info()[:2] == ("mxfp4", 68) and len(full) == sum(n for _d, _p, n in DOCS)
    _is_reference_of(full, col.open_collection(dirs["b"]).mv)                 # after the ingest
    stores = {}
    for name, fmt in history:
        storage = w["use"](name, fmt)
        col.delete_document("docB", storage_dir=storage)
        _index_doc(storage, w["provider"], "docA", new_a, "red", replace=True)
        stores[name] = col.open_collection(storage)
    live, twin = stores["q"], stores["b"]
    assert [d["doc_id"] for d in live.manifest.documents] == ["docC", "docA"] and len(live.mv) == live.manifest.rows == 17
    assert live.mv.format == "mxfp4" and twin.mv.format == "bf16"
    _is_reference_of(live.mv, twin.mv)                                        # after delete and replace
    assert live.mv.format_info()[2] == 0                                      # the head writes unit vectors: the guard is no path
    # a cold cache LOADS the file as an MXFP4 store, and the manifest still names it
    before = [a.tobytes() for a in live.mv.export_mxfp4()]
    late = w["use"]("q", "mxfp4")
    cold = col.open_collection(late)
    assert cold is not live and cold.mv.format == "mxfp4" and [a.tobytes() for a in cold.mv.export_mxfp4()] == before
    assert json.load(open(late / col.COLLECTION_MANIFEST))["mv"] == {"dim": 128, "format": "mxfp4"}
    assert _kind(late / col.COLLECTION_MV) == b"HIPMVQ41"
    # a file of another kind under an mxfp4 manifest raises, and so does the mxfp4 file under a bf16 or an fp8 manifest
    keep = (late / col.COLLECTION_MV).read_bytes()
    other = MultiVectorStore(128, max_doc_vectors=col.MV_MAX_DOC_VECTORS)
    other.append(list(np.split(twin.mv.export()[1], twin.mv.export()[0][1:-1])))
    for wrong, kind in ((other, "bf16"), (other.to_fp8(), "fp8")):
        wrong.save(str(late / col.COLLECTION_MV))
        w["hi"].clear_caches()
        with pytest.raises(RuntimeError, match=f"a {kind} multi-vector store, the collection manifest names a mxfp4"):
            col.open_collection(late)
    (late / col.COLLECTION_MV).write_bytes(keep)
    mpath = late / col.COLLECTION_MANIFEST
    good = mpath.read_text()
    data = json.loads(good)
    for entry, kind in (({"dim": 128}, "bf16"), ({"dim": 128, "format": "fp8"}, "fp8")):
        data["mv"] = entry
        mpath.write_text(json.dumps(data))
        w["hi"].clear_caches()
        with pytest.raises(RuntimeError, match=f"a mxfp4 multi-vector store, the collection manifest names a {kind}"):
            col.open_collection(late)
    data["mv"] = {"dim": 128, "format": "fp4"}
    mpath.write_text(json.dumps(data))
    w["hi"].clear_caches()
    with pytest.raises(ValueError, match="fp4"):
        col.open_collection(late)
    mpath.write_text(good)
    w["hi"].clear_caches()
    assert [a.tobytes() for a in col.open_collection(late).mv.export_mxfp4()] == before


def test_the_retriever_orders_by_the_mxfp4_maxsim(world):
    w = world
    rt = w["rt"]
    import torch
    from rag.storage.hip_index import collection as col
    from rag.storage.hip_index.passages import rows_of_chunks
    late = w["use"]("q", "mxfp4")
    _ingest_all(w, late)
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    w["monkeypatch"].setenv("HIP_LATE_INTERACTION", "false")                # the candidates: the dense stage alone
    cand_chunks = {p: asyncio.run(retriever.retrieve_chunks(QUERY, p)) for p in (None, "red")}
    assert all(len(v) == DEPTH for v in cand_chunks.values())
    w["monkeypatch"].setenv("HIP_LATE_INTERACTION", "true")
    coll = col.open_collection(late)
    assert coll.mv.format == "mxfp4"
    off, deq = coll.mv.export()                                               # the dequantised vectors: what the kernel multiplies
    _vec, q_vecs, q_counts = asyncio.run(w["provider"].embed_single_colbert(QUERY))
    q = bf16_values(q_vecs[0, :int(q_counts[0])].cpu().view(torch.int16).numpy().view(np.uint16)).astype(np.float64)
    for p in (None, "red"):
        got = asyncio.run(retriever.retrieve_chunks(QUERY, p))
        assert len(got) == TOP_K and all(c.metadata["rerank_mode"] == "colbert" for c in got)
        cands = cand_chunks[p]
        rows = rows_of_chunks(coll, cands)
        ref = [maxsim_expected(q, bf16_values(deq[off[r]:off[r + 1]]).astype(np.float64), "random") for r in rows]
        by_id = {c.chunk_id: j for j, c in enumerate(cands)}
        worst = 0.0
        for c in got:
            want, bound = ref[by_id[c.chunk_id]]
            worst = max(worst, abs(c.metadata["colbert_score"] - want) / bound)
            assert c.score == cands[by_id[c.chunk_id]].score                 # the dense similarity stays the chunk's score
        print(f"mxfp4 overlay maxsim project {p}: worst |got - ref of the dequantised vectors| / bound = {worst:.3g}")
        assert worst <= 1.0
        order = sorted(range(len(cands)), key=lambda j: (-ref[j][0], j))
        got_pos = [by_id[c.chunk_id] for c in got]
        assert [c.metadata["colbert_score"] for c in got] == sorted((c.metadata["colbert_score"] for c in got), reverse=True)
        for a, b in zip(order[:TOP_K], got_pos):
            assert a == b or abs(ref[a][0] - ref[b][0]) <= ref[a][1] + ref[b][1], (p, order[:TOP_K], got_pos)
    for p in (None, "red"):
        pages = asyncio.run(retriever.retrieve_and_rank_pages(QUERY, p))
        assert pages and all(c.metadata["rerank_mode"] == "colbert" for pg in pages for c in pg.chunks)


def test_convert_multivectors_gives_the_bytes_and_files_of_an_mxfp4_ingest(world):
    w = world
    from rag.storage.hip_index import collection as col
    q = w["use"]("q", "mxfp4")
    _ingest_all(w, q)
    want = [a.tobytes() for a in col.open_collection(q).mv.export_mxfp4()]
    b = w["use"]("b", None)                                                   # the first document unset, the rest under mxfp4:
    _index_doc(b, w["provider"], *DOCS[0][:1], w["texts"]["docA"], "red")
    w["use"]("b", "mxfp4")                                                    # an existing collection keeps its format
    for doc, project, _n in DOCS[1:]:
        _index_doc(b, w["provider"], doc, w["texts"][doc], project)
    coll = col.open_collection(b)
    assert coll.mv.format == "bf16" and json.load(open(b / col.COLLECTION_MANIFEST))["mv"] == {"dim": 128}
    with pytest.raises(ValueError):
        coll.convert_multivectors("fp4")
    coll.convert_multivectors("mxfp4")
    assert coll.mv.format == "mxfp4" and [a.tobytes() for a in coll.mv.export_mxfp4()] == want
    assert (b / col.COLLECTION_MV).read_bytes() == (q / col.COLLECTION_MV).read_bytes()          # the file, then the manifest
    assert json.load(open(b / col.COLLECTION_MANIFEST))["mv"] == {"dim": 128, "format": "mxfp4"}
    coll.convert_multivectors("mxfp4")                                        # already mxfp4: nothing to do
    for fmt in ("bf16", "fp8"):
        with pytest.raises(RuntimeError, match="cannot be converted"):
            coll.convert_multivectors(fmt)
    assert [a.tobytes() for a in coll.mv.export_mxfp4()] == want
    w["hi"].clear_caches()                                                    # a cold cache loads the converted collection
    cold = col.open_collection(b)
    assert cold is not coll and cold.mv.format == "mxfp4" and [a.tobytes() for a in cold.mv.export_mxfp4()] == want
    _index_doc(b, w["provider"], "docD", _texts(5, 77), "blue")               # and it goes on as an MXFP4 collection
    assert col.open_collection(b).mv.format == "mxfp4" and len(col.open_collection(b).mv) == col.open_collection(b).manifest.rows
    # an fp8 collection refuses the conversion: no second quantisation
    f8 = w["use"]("f8", "fp8")
    _ingest_all(w, f8)
    coll8 = col.open_collection(f8)
    was = [a.tobytes() for a in coll8.mv.export_fp8()]
    with pytest.raises(RuntimeError, match="cannot be converted"):
        coll8.convert_multivectors("mxfp4")
    assert coll8.mv.format == "fp8" and [a.tobytes() for a in coll8.mv.export_fp8()] == was
    assert json.load(open(f8 / col.COLLECTION_MANIFEST))["mv"] == {"dim": 128, "format": "fp8"}
