"""
Page table of the collection: for every row the page its chunk lies on (`chunk.get("page", 0)`) and a tag of its document,
on the device (hiprag.PageTable), for the device page-ranking call -- the last step of the reference's retriever
(rag/query/page_retriever.py:145-236) over candidate rows that never leave the GPU.  One document of the table per manifest
entry, so two rows lie on the same page only inside one document.

The table is cached per manifest version exactly as the passage token store is (passages.get_collection_tokens), and while
it is live the collection's own entry points (append_document / delete_document / replace_document) update it on the device
(follow_collection_pages: the old row range removed, the new document's pages appended).  A cold cache builds it from the
chunk tables; any failure of an incremental update, a row count that disagrees with the manifest, or a page that is not an
integer that fits int32 drops the entry, so the next query rebuilds.  A cold build that meets such a page raises
PageValueError: the retriever then ranks on the host, where a page may be any key.  There is no file format: like the
postings and the token store, the table is rebuilt by a new process.
"""
from __future__ import annotations

import threading
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from rag.config import config
from rag.storage.hip_index.sparse import _collection_key, _collection_version

_PAGE_CACHE: Dict[str, Tuple[tuple, Any]] = {}      # collection key -> (manifest version, PageTable)
_LOCK = threading.Lock()


class PageValueError(ValueError):
    """A chunk's page is not an integer that fits int32: the device table cannot hold it."""


def page_values(pages: Sequence[Any]) -> np.ndarray:
    """chunk pages -> int32; anything that is not an integer in [-2^31, 2^31) raises PageValueError"""
    for p in pages:
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not -(1 << 31) <= int(p) < (1 << 31):
            raise PageValueError(f"page {p!r} is not an integer that fits int32")
    return np.asarray([int(p) for p in pages], dtype=np.int32)


def chunk_pages(storage_dir, doc_id: str) -> List[Any]:
    """`chunk.get("page", 0)` of every chunk of a document's chunk table, in row order"""
    import rag.storage.hip_index as hi
    return [c.get("page", 0) for c in hi._load_chunk_list(storage_dir, doc_id)]


def collection_pages(manifest, storage_dir) -> Tuple[np.ndarray, np.ndarray]:
    """(pages int32 [rows], doc_offsets int64 [documents + 1]) of `manifest` in row order.  A chunk table whose length
    differs from the rows its manifest entry names raises ValueError, as collection_texts does."""
    pages: List[Any] = []
    offsets = [0]
    for doc in manifest.documents:
        of_doc = chunk_pages(storage_dir, doc["doc_id"])
        if len(of_doc) != doc["rows"]:
            raise ValueError(f"document {doc['doc_id']!r}: its chunk table has {len(of_doc)} rows, the collection manifest names "
                             f"{doc['rows']} (rows {doc['row0']}..{doc['row0'] + doc['rows'] - 1})")
        pages.extend(of_doc)
        offsets.append(len(pages))
    return page_values(pages), np.asarray(offsets, dtype=np.int64)


def get_collection_pages(coll):
    """The PageTable over `coll`'s chunk tables in row order, kept per version of the manifest; follow_collection_pages
    keeps a live entry current, for any other version it is built from the chunk tables."""
    from hiprag import PageTable
    key = _collection_key(coll)
    version = _collection_version(coll)
    with _LOCK:
        hit = _PAGE_CACHE.get(key)
        if hit is not None and hit[0] == version:
            return hit[1]
    pages, offsets = collection_pages(coll.manifest, coll.storage_dir)
    table = PageTable(device=config.HIP_DEVICE)
    table.append(pages, offsets)
    with _LOCK:
        _PAGE_CACHE[key] = (version, table)
    return table


def live_collection_pages(coll):
    """The cached table if it is that of `coll`'s manifest AS IT STANDS (asked before a change), else None; an entry of any
    other version is dropped."""
    key = _collection_key(coll)
    with _LOCK:
        hit = _PAGE_CACHE.get(key)
        if hit is None:
            return None
        if hit[0] == _collection_version(coll):
            return hit[1]
        del _PAGE_CACHE[key]
    return None


def follow_collection_pages(coll, live, removed: Sequence[Tuple[int, int]], pages: Optional[Sequence[Any]]) -> bool:
    """Behind a saved change of `coll`: the live table (live_collection_pages before the change) drops the row ranges
    `removed` (numbering before the change), takes `pages` (the appended document's chunk pages in row order; None: no
    append) at the end as ONE document and is re-keyed to the new manifest version.  Any failure, a page that does not fit,
    or a row count that disagrees with the manifest, drops the entry instead.  Returns whether the table followed."""
    if live is None:
        return False
    key = _collection_key(coll)
    try:
        new_pages = page_values(pages) if pages is not None else None      # before anything is touched
        if removed:
            live.remove_ranges(list(removed))
        if new_pages is not None:
            live.append(new_pages)
        if len(live) != coll.manifest.rows:
            raise RuntimeError(f"the page table holds {len(live)} rows, the manifest names {coll.manifest.rows}")
    except Exception as e:            # noqa: BLE001 -- whatever went wrong, a rebuild is always right
        from rag.logging import logger
        logger.warning(f"Incremental update of the page table failed ({e}); it will be rebuilt")
        with _LOCK:
            _PAGE_CACHE.pop(key, None)
        return False
    with _LOCK:
        _PAGE_CACHE[key] = (_collection_version(coll), live)
    return True


def clear_page_cache() -> None:
    with _LOCK:
        _PAGE_CACHE.clear()
