"""
Passage token store of the collection: the token ids of every chunk text in row order (document id == collection row), on
the device (hiprag.TokenStore), for the device rerank call -- the cross-encoder the reference only configures
(rag/config.py:25-27).  A candidate of a query is then a ROW: nothing is tokenised again per query but the query itself.

Each text is tokenised as the tokenizer's `encode` does, minus bos / eos, with newlines replaced as
CrossEncoderReranker.score replaces them, and cut to MAX_DOC_TOKENS (a 512-token pair never reads more).

The store is cached per manifest version exactly as the collection postings are (sparse.get_collection_sparse), and while
it is live the collection's own entry points (append_document / delete_document / replace_document) update it on the
device (follow_collection_tokens: the old row range removed, the new document's texts appended).  A cold cache builds it
from the chunk tables; any failure of an incremental update, or a document count that disagrees with the manifest, drops
the entry, so the next query rebuilds.  There is no file format: like the postings, it is rebuilt by a new process.
"""
from __future__ import annotations

import threading
from typing import Any, Dict, List, Optional, Sequence, Tuple

from rag.config import config
from rag.storage.hip_index.sparse import _collection_key, _collection_version

MAX_DOC_TOKENS = 508           # 512 - 4: what a pair of at most 512 tokens can hold of a passage
PAD_ID = 1                     # XLM-R's <pad>, hiprag.EncoderConfig.pad_id

_TOKEN_CACHE: Dict[str, Tuple[tuple, Any, Any]] = {}      # collection key -> (manifest version, TokenStore, tokenizer)
_LOCK = threading.Lock()


def passage_tokens(tokenizer, text: str, cap: int = MAX_DOC_TOKENS) -> List[int]:
    """The stored body of one chunk text: `encode` minus bos / eos, newlines as CrossEncoderReranker.score has them."""
    return tokenizer.encode(text.replace("\n", " "), cap + 2)[1:-1]


def query_tokens(tokenizer, query: str, max_len: int) -> List[int]:
    """The body of a query; the pair rule cuts it to max_len - 4."""
    return tokenizer.encode(query.replace("\n", " "), max_len + 2)[1:-1]


def _vocab_of(tokenizer) -> int:
    vocab = getattr(tokenizer, "vocab", None)
    return int(vocab) if vocab is not None else int(tokenizer.tk.get_vocab_size())


def get_collection_tokens(coll, tokenizer):
    """The TokenStore over `coll`'s chunk texts in row order, kept per version of the manifest (and per tokenizer);
    follow_collection_tokens keeps a live entry current, for any other version it is built from the chunk tables."""
    from hiprag import TokenStore
    from rag.storage.hip_index.collection import collection_texts
    key = _collection_key(coll)
    version = _collection_version(coll)
    with _LOCK:
        hit = _TOKEN_CACHE.get(key)
        if hit is not None and hit[0] == version and hit[2] is tokenizer:
            return hit[1]
    store = TokenStore(_vocab_of(tokenizer), bos=tokenizer.bos, eos=tokenizer.eos, pad=PAD_ID, max_doc_tokens=MAX_DOC_TOKENS,
                       device=config.HIP_DEVICE)
    store.append([passage_tokens(tokenizer, t) for t in collection_texts(coll.manifest, coll.storage_dir)])
    with _LOCK:
        _TOKEN_CACHE[key] = (version, store, tokenizer)
    return store


def live_collection_tokens(coll):
    """The cached (store, tokenizer) if it is that of `coll`'s manifest AS IT STANDS (asked before a change), else None; an
    entry of any other version is dropped."""
    key = _collection_key(coll)
    with _LOCK:
        hit = _TOKEN_CACHE.get(key)
        if hit is None:
            return None
        if hit[0] == _collection_version(coll):
            return hit[1], hit[2]
        del _TOKEN_CACHE[key]
    return None


def follow_collection_tokens(coll, live, removed: Sequence[Tuple[int, int]], texts: Optional[Sequence[str]]) -> bool:
    """Behind a saved change of `coll`: the live store (live_collection_tokens before the change) drops the row ranges
    `removed` (numbering before the change), takes the tokens of `texts` (the appended document's chunk texts in row
    order; None: no append) at the end and is re-keyed to the new manifest version.  Any failure, or a document count that
    disagrees with the manifest, drops the entry instead.  Returns whether the store followed."""
    if live is None:
        return False
    store, tokenizer = live
    key = _collection_key(coll)
    try:
        if removed:
            store.remove_ranges(list(removed))
        if texts is not None:
            store.append([passage_tokens(tokenizer, t) for t in texts])
        if len(store) != coll.manifest.rows:
            raise RuntimeError(f"the passage token store holds {len(store)} documents, the manifest names {coll.manifest.rows} rows")
    except Exception as e:            # noqa: BLE001 -- whatever went wrong, a rebuild is always right
        from rag.logging import logger
        logger.warning(f"Incremental update of the passage token store failed ({e}); it will be rebuilt")
        with _LOCK:
            _TOKEN_CACHE.pop(key, None)
        return False
    with _LOCK:
        _TOKEN_CACHE[key] = (_collection_version(coll), store, tokenizer)
    return True


def rows_of_chunks(coll, chunks) -> List[int]:
    """The collection row of every RetrievedChunk (metadata["doc_id"] + its place in that document's chunk table); a chunk
    the collection does not hold raises KeyError."""
    import rag.storage.hip_index as hi
    place: Dict[str, Dict[str, int]] = {}
    row0 = {doc["doc_id"]: doc["row0"] for doc in coll.manifest.documents}
    rows = []
    for c in chunks:
        doc_id = c.metadata.get("doc_id")
        if doc_id not in row0:
            raise KeyError(f"chunk {c.chunk_id!r}: document {doc_id!r} is not in the collection")
        if doc_id not in place:
            place[doc_id] = {ch.get("chunk_id"): i for i, ch in enumerate(hi._load_chunk_list(coll.storage_dir, doc_id))}
        rows.append(row0[doc_id] + place[doc_id][c.chunk_id])
    return rows


def clear_token_cache() -> None:
    with _LOCK:
        _TOKEN_CACHE.clear()
