"""
BM25 side index over the same chunk table the dense index uses (row id == position in `{doc_id}_chunks.json`,
rag/storage/faiss_index.py:175-181), built once per chunk-file version and kept in HBM (hiprag.HipBM25).
The reference names this leg (README.md:54-58, rag/config.py:43-45) without implementing it; spec in DESIGN.md.
With HIP_COLLECTION there is a second kind: ONE index over the chunk texts of the whole collection, document id ==
collection row (get_collection_sparse), searched through per-query scopes (hipbm25_search_scoped).  An append, a removal
or a replacement changes N, df and avgdl, hence every impact: the index is a hiprag.HipBM25Updatable, which keeps term
frequencies and document lengths on the device, so while it is live in this cache the collection's own entry points
(append_document / delete_document / replace_document) update it in place (follow_collection: the new document's chunk
texts appended, the old row range removed, one reweigh pass before the next query) and re-key it to the new manifest
version.  A cold cache (a new process) builds it from the chunk tables; any failure of an incremental update drops the
entry, so the next query rebuilds.  Out of scope: a postings file or persisted vocabulary, sharded collections,
scope-local idf, asynchronous updates.
"""
from __future__ import annotations

import hashlib
import threading
from pathlib import Path
from typing import Any, Dict, List, Tuple

from rag.config import config

_SPARSE_CACHE: Dict[str, Tuple[tuple, Any]] = {}
_LOCK = threading.Lock()


def _table_version(storage_path: Path, doc_id: str, n_rows: int) -> tuple:
    """Version key of a document's chunk table: the one `_load_chunk_list` caches by -- (path, mtime) -- plus the row
    count.  (An object identity such as id(chunks_list) is NOT a version: once a reloaded table frees the old list,
    CPython may hand its id to the new one and the old postings would be searched against the new rows.)"""
    path = Path(storage_path) / f"{doc_id}_chunks.json"
    try:
        return ("file", str(path), path.stat().st_mtime, n_rows)
    except OSError:
        return ("file", str(path), None, n_rows)


def _digest(texts: List[str]) -> bytes:
    h = hashlib.blake2b(digest_size=16)
    for t in texts:
        h.update(t.encode("utf-8", "surrogatepass"))
        h.update(b"\x00")
    return h.digest()


def get_sparse_index(storage_path: Path, doc_id: str, chunks_list: List[Dict[str, Any]]):
    from hiprag import HipBM25, build_postings_from_texts
    key = str(Path(storage_path) / doc_id)
    version = _table_version(storage_path, doc_id, len(chunks_list))
    with _LOCK:
        hit = _SPARSE_CACHE.get(key)
        if hit is not None and hit[0] == version:
            return hit[1]
    texts = [c.get("text", "") for c in chunks_list]
    if hit is not None and hit[0][0] == "ingest" and hit[0][1:] == (len(texts), _digest(texts)):
        with _LOCK:                                         # built at ingest time from these very texts: adopt it
            _SPARSE_CACHE[key] = (version, hit[1])
        return hit[1]
    index = HipBM25(build_postings_from_texts(texts), device=config.HIP_DEVICE)
    with _LOCK:
        _SPARSE_CACHE[key] = (version, index)
    return index


def put_sparse_index(storage_path: Path, doc_id: str, texts: List[str]) -> int:
    """Ingest side: build the postings of `texts` (row id == position) and keep the index for the readers of this
    document; get_sparse_index adopts it for the chunk-file version whose texts have the same digest and rebuilds
    for any other.  Returns the postings count."""
    from hiprag import HipBM25, build_postings_from_texts
    postings = build_postings_from_texts(texts)
    index = HipBM25(postings, device=config.HIP_DEVICE)
    with _LOCK:
        _SPARSE_CACHE[str(Path(storage_path) / doc_id)] = (("ingest", len(texts), _digest(list(texts))), index)
    return int(postings.offsets[-1])


# ---- HIP_SPARSE_MODE=lexical: the chunks' lexical weights (hiprag.LexicalIndex) instead of BM25 postings ------------------------
LEXICAL_SUFFIX = "_hip.lexical.npz"


def _lexical_key(storage_path: Path, doc_id: str) -> str:
    return "lexical:" + str(Path(storage_path) / doc_id)


def put_lexical_index(storage_path: Path, doc_id: str, texts: List[str], index) -> int:
    """Ingest side: keep the LexicalIndex built from the ingest's own forward for the readers of this document (adopted like
    put_sparse_index's) and write it to {doc_id}_hip.lexical.npz.  Returns the postings count."""
    index.save(str(Path(storage_path) / f"{doc_id}{LEXICAL_SUFFIX}"))
    with _LOCK:
        _SPARSE_CACHE[_lexical_key(storage_path, doc_id)] = (("ingest", len(texts), _digest(list(texts))), index)
    return int(index.p.offsets[-1])


def get_lexical_index(storage_path: Path, doc_id: str, chunks_list: List[Dict[str, Any]]):
    """The document's LexicalIndex: the cached one for this version of the chunk table, the ingest's for the same texts, else
    LOADED from {doc_id}_hip.lexical.npz -- never re-encoded.  A missing file, or one whose document count is not the chunk
    table's, raises: the document was not ingested under HIP_SPARSE_MODE=lexical (or its chunk table has changed since)."""
    from hiprag.lexical import LexicalIndex
    key = _lexical_key(storage_path, doc_id)
    version = _table_version(storage_path, doc_id, len(chunks_list))
    with _LOCK:
        hit = _SPARSE_CACHE.get(key)
        if hit is not None and hit[0] == version:
            return hit[1]
    if hit is not None and hit[0][0] == "ingest":
        texts = [c.get("text", "") for c in chunks_list]
        if hit[0][1:] == (len(texts), _digest(texts)):
            with _LOCK:
                _SPARSE_CACHE[key] = (version, hit[1])
            return hit[1]
    path = Path(storage_path) / f"{doc_id}{LEXICAL_SUFFIX}"
    if not path.exists():
        raise RuntimeError(f"{path} does not exist: ingest {doc_id} under HIP_SPARSE_MODE=lexical first")
    index = LexicalIndex.load(str(path), device=config.HIP_DEVICE)
    if index.n_docs != len(chunks_list):
        raise RuntimeError(f"{path} holds {index.n_docs} chunks, the chunk table {len(chunks_list)}: ingest {doc_id} again")
    with _LOCK:
        _SPARSE_CACHE[key] = (version, index)
    return index


def _collection_key(coll) -> str:
    return "collection:" + str(coll.manifest_path)


def _collection_version(coll) -> tuple:
    try:
        mtime = coll.manifest_path.stat().st_mtime
    except OSError:
        mtime = None
    return ("collection", mtime, len(coll.manifest.documents), coll.manifest.rows, coll.manifest.generation)


def get_collection_sparse(coll):
    """The HipBM25Updatable over `coll`'s documents in row order, kept per version of the manifest -- its file's mtime, its
    documents, its rows and its generation (a document replaced by one of the same row count within one mtime tick changes
    only that).  follow_collection keeps a live entry current; for any other version it is built from the chunk tables
    (collection_postings, which raises on a chunk table whose length disagrees with the manifest)."""
    from hiprag import HipBM25Updatable
    from rag.storage.hip_index.collection import collection_postings
    key = _collection_key(coll)
    version = _collection_version(coll)
    with _LOCK:
        hit = _SPARSE_CACHE.get(key)
        if hit is not None and hit[0] == version:
            return hit[1]
    index = HipBM25Updatable(collection_postings(coll.manifest, coll.storage_dir), device=config.HIP_DEVICE)
    with _LOCK:
        _SPARSE_CACHE[key] = (version, index)
    return index


def live_collection_sparse(coll):
    """The cached collection index if it is that of `coll`'s manifest AS IT STANDS (asked before a change), else None; an
    entry of any other version is dropped."""
    key = _collection_key(coll)
    with _LOCK:
        hit = _SPARSE_CACHE.get(key)
        if hit is None:
            return None
        if hit[0] == _collection_version(coll) and hasattr(hit[1], "append_texts"):
            return hit[1]
        del _SPARSE_CACHE[key]
    return None


def follow_collection(coll, live, removed: List[Tuple[int, int]], texts) -> bool:
    """Behind a saved change of `coll`: the live index (live_collection_sparse before the change) drops the row ranges
    `removed` (numbering before the change), takes `texts` (the chunk texts of the appended document, in row order; None: no
    append) at the end, and is re-keyed to the new manifest version -- the next hybrid query reweighs once and does not
    rebuild.  Any failure, or a document count that disagrees with the manifest, drops the entry instead: the next query
    rebuilds from the chunk tables.  Returns whether the index followed."""
    if live is None:
        return False
    key = _collection_key(coll)
    try:
        if removed:
            live.remove_ranges(removed)
        if texts is not None:
            live.append_texts(list(texts))
        if live.sizes()["n_docs"] != coll.manifest.rows:
            raise RuntimeError(f"the collection postings hold {live.sizes()['n_docs']} documents, the manifest names {coll.manifest.rows} rows")
    except Exception as e:            # noqa: BLE001 -- whatever went wrong, a rebuild is always right
        from rag.logging import logger
        logger.warning(f"Incremental update of the collection postings failed ({e}); they will be rebuilt")
        with _LOCK:
            _SPARSE_CACHE.pop(key, None)
        return False
    with _LOCK:
        _SPARSE_CACHE[key] = (_collection_version(coll), live)
    return True


def clear_sparse_cache() -> None:
    with _LOCK:
        _SPARSE_CACHE.clear()
