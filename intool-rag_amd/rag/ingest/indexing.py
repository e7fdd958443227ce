"""
rag/ingest/indexing.py -- phase 4 of IngestionPipeline.ingest_pdf (rag/ingest/ingestion_pipeline.py:80-94) on the GPU.

Reference:   texts = [c.text for c in chunks]
             embeddings = await embedding_provider.embed_batch(texts)          # list of lists of Python floats
             index = create_faiss_index(embeddings)                            # np.array(..., float32) -> IndexFlatL2.add
             save_faiss_index(index, STORAGE_DIR / f"{doc_id}_faiss.index")
Here the vectors never leave HBM: the provider's encoder output (a CUDA tensor) is re-tiled straight into the index
(hipidx_add_dev), the index file is written once, and -- when hybrid search is on -- the BM25 postings of the same
chunk texts are built and uploaded in the same call, so the first query does not pay for them.
Any EmbeddingProvider works; providers without a device path go through the reference's list-of-lists interface.
Row id == position in `chunks`, the convention the reader relies on (rag/storage/faiss_index.py:175-181).
HIP_SPARSE_MODE=lexical: the sparse side is the chunks' lexical weights instead (BGE-M3's, from the very forward that makes
the embeddings: provider.embed_batch_lexical_device), transposed into a hiprag.LexicalIndex, cached for the readers and
written to `{doc_id}_hip.lexical.npz`.
HIP_COLLECTION_SPARSE=lexical (with HIP_COLLECTION=true): the same forward's lexical rows are passed on to the collection, whose
lexical postings take them on the device (hipbm25_append_rows_dev); the per-document sparse files are written as ever.
HIP_LATE_INTERACTION=true (with HIP_COLLECTION=true): the chunks' per-token (ColBERT) vectors come from that same forward
(provider.embed_batch_colbert_device) and go into the collection's multi-vector store beside the rows.
HIP_M3_SCORE=true (with both of the above): ONE forward per batch (provider.embed_batch_m3_device) feeds the flat index, the
lexical postings and the multi-vector store.
"""
from __future__ import annotations

import time
from pathlib import Path
from typing import Any, Dict, Optional, Sequence

from rag.config import config
from rag.llm.embeddings.factory import get_embedding_provider
from rag.logging import logger
from rag.storage.hip_index import INDEX_SUFFIX, create_hip_index, save_hip_index


def _text_of(chunk: Any) -> str:
    return chunk["text"] if isinstance(chunk, dict) else chunk.text


async def index_chunks(doc_id: str, chunks: Sequence[Any], storage_dir: Optional[Path] = None, provider=None,
                       with_sparse: Optional[bool] = None, project: Optional[str] = None, replace: bool = False) -> Dict[str, Any]:
    """Embed `chunks` (objects with .text, or dicts with "text"), build and save `{doc_id}_hip.index`.
    Returns the same summary keys the reference's ingest returns for this phase.
    HIP_COLLECTION=true: the same vectors are also appended to the storage's collection index under `project` (the argument
    the reference's ingest_pdf takes and drops, rag/ingest/ingestion_pipeline.py:35); the summary gains "collection_rows".
    A doc_id the collection already holds raises ValueError unless `replace=True`: then its old rows leave the collection
    and the new ones are appended at the end (replace_document) -- the reference's second ingest of a document, which
    overwrites {doc_id}_faiss.index (:80-94).  Without HIP_COLLECTION `replace` changes nothing: the per-document files are
    overwritten either way."""
    start = time.time()
    storage = Path(storage_dir) if storage_dir is not None else config.STORAGE_DIR
    provider = provider or get_embedding_provider()
    texts = [_text_of(c) for c in chunks]
    sparse = config.HYBRID_SEARCH_ENABLED if with_sparse is None else with_sparse
    lexical = sparse and config.HIP_SPARSE_MODE == "lexical"      # raises on an unknown mode or with HIP_COLLECTION
    coll_lexical = config.HIP_COLLECTION_SPARSE == "lexical"      # raises on an unknown value, without HIP_COLLECTION, with late interaction
    logger.info(f"Generating embeddings for {len(texts)} chunks...")
    lex_rows = None
    colbert = None
    late = config.HIP_LATE_INTERACTION                              # raises without HIP_COLLECTION or with HIP_RERANK
    if late and not hasattr(provider, "embed_batch_colbert_device"):
        raise RuntimeError("HIP_LATE_INTERACTION=true needs an embedding provider with a ColBERT head (EMBEDDING_PROVIDER=hip)")
    m3 = config.HIP_M3_SCORE                                        # raises without the three settings it needs
    if m3 and not hasattr(provider, "embed_batch_m3_device"):
        raise RuntimeError("HIP_M3_SCORE=true needs an embedding provider with both heads (EMBEDDING_PROVIDER=hip)")
    if m3 and len(texts):
        # one forward: vectors, lexical weights and token vectors (hipenc_forward_m3)
        embeddings, lex_terms, lex_weights, lex_counts, tok_vecs, tok_counts = await provider.embed_batch_m3_device(texts)
        lex_rows, colbert = [lex_terms, lex_weights, lex_counts], [tok_vecs, tok_counts]
    elif late and len(texts):
        embeddings, *colbert = await provider.embed_batch_colbert_device(texts)    # one forward: vectors and token vectors
    elif lexical or coll_lexical:
        if not hasattr(provider, "embed_batch_lexical_device"):
            raise RuntimeError(("HIP_COLLECTION_SPARSE" if coll_lexical else "HIP_SPARSE_MODE") +
                               "=lexical needs an embedding provider with a lexical head (EMBEDDING_PROVIDER=hip)")
        embeddings, *lex_rows = await provider.embed_batch_lexical_device(texts)   # one forward: vectors and lexical weights
    elif hasattr(provider, "embed_batch_device"):
        embeddings = await provider.embed_batch_device(texts)        # CUDA tensor [n, d]
    else:
        embeddings = await provider.embed_batch(texts)
    if len(texts) == 0:
        raise ValueError("index_chunks needs at least one chunk")
    if len(texts) == 0:
        raise ValueError("index_chunks needs at least one chunk")
    index = create_hip_index(embeddings)
    index_path = storage / f"{doc_id}{INDEX_SUFFIX}"
    save_hip_index(index, str(index_path))
    postings = 0
    if lexical:
        from hiprag.lexical import LexicalIndex
        from rag.storage.hip_index.sparse import put_lexical_index
        lex = LexicalIndex.from_doc_weights(*lex_rows, n_terms=provider.encoder.cfg.vocab, device=config.HIP_DEVICE)
        postings = put_lexical_index(storage, doc_id, texts, lex)
    elif sparse:
        from rag.storage.hip_index.sparse import put_sparse_index
        postings = put_sparse_index(storage, doc_id, texts)
    collection_rows = None
    if config.HIP_COLLECTION:
        from rag.storage.hip_index.collection import append_document, replace_document
        put = replace_document if replace else append_document
        extra = {"colbert": tuple(colbert)} if colbert is not None else {}
        if coll_lexical:
            extra["lexical"] = tuple(lex_rows) + (provider.encoder.cfg.vocab,)    # the rows of the forward that made the embeddings
        collection_rows = put(doc_id, project, embeddings, storage_dir=storage, texts=texts, **extra)[1]   # live collection postings take the texts
    total = time.time() - start
    logger.info(f"Indexing complete in {total:.2f}s")
    summary = {"success": True, "doc_id": doc_id, "chunk_count": len(texts), "vectors_indexed": int(index.ntotal),
               "postings_indexed": postings, "index_path": str(index_path), "processing_time": total}
    if collection_rows is not None:
        summary["collection_rows"] = int(collection_rows)
    return summary
