"""
rag/storage/hip_index/collection.py -- ONE flat index for the whole store, and a `project` argument that works.

The reference carries `project` from its router through ingest (rag/ingest/ingestion_pipeline.py:35) and through every
query (rag/storage/faiss_index.py:140) and drops it at both ends ("for future filtering", :150); it searches the first
index file it finds (:162-167).  With HIP_COLLECTION=true the ingest appends every document to a collection index as
well, whole, so a document is a contiguous ROW RANGE of it, a project a handful of ranges, and "only these documents" is
one scoped search (hipidx_search_scoped, include/hiprag.h) that reads only those rows.

Hybrid search (HybridRetriever(hybrid=True) under HIP_COLLECTION) is scoped the same way: the BM25 postings of the WHOLE
collection, document id == collection row (collection_postings), and ONE library call per query, hiphybrid_search_scoped_dev
(search_collection_hybrid): both legs over the rows of scope_for(project), RRF behind them.  idf, N and avgdl are those of
the collection, whatever the scope.  An append, a removal or a replacement changes N, df and avgdl, hence every impact: the
postings are a hiprag.HipBM25Updatable, and while they are live in the process (rag/storage/hip_index/sparse.py) append_document,
delete_document and replace_document update them ON THE DEVICE -- the new document's chunk texts appended, the old row
range removed, every impact recomputed by one kernel pass before the next query -- instead of rebuilding them from every chunk
table.  A cold cache (a new process) still builds them from the chunk tables; there is no postings file.
The passage token store of the device reranker (rag/storage/hip_index/passages.py) and the page table of the device page
ranking (rag/storage/hip_index/pages.py) follow the same three entry points in the same way while they are live.
search_collection_device is search_collection / search_collection_hybrid with the results left on the device, for the
retriever under HIP_PAGES.

Files in STORAGE_DIR:
    hip_collection.index   plain HIPIDX01 (hipidx_save).  The name does not end in `_hip.index`, so the per-document
                           readers (open_first_index / open_all_indices) never see it.
    hip_collection.json    {"version": 1, "d", "metric", "documents": [{"doc_id", "project", "row0", "rows"}, ...]} in row
                           order, plus "generation" once a document has been removed or replaced; written atomically
                           (temp file + rename) AFTER the index file (itself a temp file + rename), so a manifest never
                           names rows the index file lacks.  Once an IVF companion exists: "ivf": {"nlist": N}.
    hip_collection.ivf     HIPIVF01 (hipivf_save), only after train_collection_ivf: the IVF COMPANION, see below.
    hip_collection.mv      HIPMV001 (hipmv_save), only for a collection ingested under HIP_LATE_INTERACTION=true: the per-token
                           (ColBERT) vectors of every row, document i of the store = row i (hiprag.MultiVectorStore).  Written
                           between the index file and the manifest, which then carries "mv": {"dim": d}.  A collection whose
                           store was created under HIP_COLBERT_FORMAT=fp8 (or converted, Collection.convert_multivectors)
                           keeps e4m3fn codes and a scale per vector, dim + 4 bytes a token instead of 2 x dim: the file is
                           then a HIPMVQ81 under the same name, the manifest entry {"dim": d, "format": "fp8"} (no "format"
                           means bf16), and a file whose kind is not the manifest's raises.  Under
                           HIP_COLBERT_FORMAT=mxfp4 (or convert_multivectors("mxfp4")) it keeps e2m1 codes and an e8m0 scale
                           per 32 components, dim / 2 + dim / 32 bytes a token: a HIPMVQ41 under the same name, the manifest
                           entry {"dim": d, "format": "mxfp4"}.  Unlike postings,
                           passage tokens and pages it cannot be rebuilt from the chunk tables without encoding every chunk
                           again, so a new process LOADS it; a file whose document count is not the manifest's row count
                           raises, it is never re-encoded silently.  append / remove keep it in step on the device.
    hip_collection.mvc     only after train_collection_centroids: the token centroids of the multi-vector store, bf16 bits as a
                           uint16 .npy [ncent, dim]; the manifest then carries "mvc": {"ncent": C}.  The codes are not stored:
                           open_collection attaches the table and the store computes them again.  HIP_LATE_CANDIDATES uses them.
    hip_collection.lexical.npz  only for a collection ingested under HIP_COLLECTION_SPARSE=lexical: the lexical weights of every
                           row as term-major impact postings, document i = row i (hiprag.LexicalIndexUpdatable.save, the .npz
                           layout of hiprag.LexicalIndex).  Written like the multi-vector store, and the manifest then carries
                           "lexical": {"n_terms": V}.  Like those vectors the weights cannot be rebuilt from the chunk tables
                           without encoding again: a new process LOADS the file, and a missing one, or one whose document count
                           is not the manifest's row count, raises.  append / remove keep the postings in step ON THE DEVICE
                           (hipbm25_append_rows_dev with the rows of the forward that made the embeddings,
                           hipbm25_remove_ranges); they need no reweigh and are searchable at once.

The IVF companion (HIP_INDEX_TYPE=ivf): the flat collection index stays -- it is the exact path and the dense leg of the
scoped hybrid call -- and train_collection_ivf builds an IVF-Flat index over the same rows beside it.  IVF ids are dense and
in insertion order, so they ARE collection rows: append calls ivf.add, remove calls ivf.remove_ranges with the range table
the flat index gets (both renumber densely in order), save writes the companion between the index file and the manifest.
With HIP_INDEX_TYPE=ivf and a companion present, search_collection / search_collection_batch search the companion at
nprobe = max(1, min(HIP_IVF_NPROBE, nlist)): `project=None` -> ivf.search / search_batch, a project -> ONE
hipivf_search_scoped call over scope_for(project).  With HIP_IVF_PROBE=any (default) the probed lists do not depend on the
scope (faiss's IDSelector behaviour); with HIP_IVF_PROBE=scope they are the nprobe best lists among those that hold a row
of the project (hipivf_search_scoped_probe), so a small project is not lost among lists that hold none of it.  At nprobe =
nlist (scope: at nprobe >= the lists the project touches) the result is the flat scoped search's bit for bit.  Without a
companion, or with HIP_INDEX_TYPE=flat, everything behaves as if there were none.  search_collection_hybrid uses the flat
index unless HIP_IVF_HYBRID=true as well: then its dense leg is the companion's scoped search at the same nprobe and probe
mode (hiphybrid_search_ivf_scoped_dev), the sparse leg and RRF unchanged.

Removing and replacing documents: delete_document / replace_document / index_chunks(..., replace=True).  The rows of the
document leave the index on the device (hipidx_remove_ranges: faiss.IndexFlat.remove_ids as stable compaction, in place),
the documents behind it keep their order and move down, a replacement is appended at the END (so a replaced document
changes its place in row order, as it would in a collection built from the final documents in that order).  Every removal
or replacement bumps the manifest's `generation`, which versions the collection postings beside mtime, documents and rows:
a document replaced by one of the same row count within one mtime tick must not be served stale postings.  append_document
and add_document still raise on a doc_id they already hold.

Out of scope here, deliberately: a postings file or persisted vocabulary (a new process rebuilds the postings from the chunk
tables), scope-local idf, sharded collections, asynchronous postings updates, dropping the flat index once a companion exists.
"""
from __future__ import annotations

import bisect
import json
import os
import struct
import threading
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from rag.config import config, ivf_auto_nlist
from rag.logging import logger
from rag.storage.hip_index import IVF_MAX_POINTS_PER_CENTROID, IVF_TRAIN_ITERS   # the package imports this module lazily

COLLECTION_INDEX = "hip_collection.index"
COLLECTION_MANIFEST = "hip_collection.json"
COLLECTION_IVF = "hip_collection.ivf"        # the IVF companion (HIPIVF01); like the index file, not a `*_hip.index`
COLLECTION_MV = "hip_collection.mv"          # the multi-vector store (HIPMV001; HIPMVQ81 for an fp8 store, HIPMVQ41 for an mxfp4 one)
COLLECTION_MVC = "hip_collection.mvc"        # its centroid table, bf16 bits as a uint16 .npy [ncent, dim] (train_collection_centroids)
MV_FORMATS = ("bf16", "fp8", "mxfp4")
COLLECTION_LEXICAL = "hip_collection.lexical.npz"   # the lexical postings (hiprag.LexicalIndexUpdatable.save)
MV_MAX_DOC_VECTORS = 511                     # a chunk of at most 512 tokens has at most 511 vectors (CLS carries none)
MANIFEST_VERSION = 1
SCOPED_MAX_TOP_K = 256             # hipidx_search_scoped's k limit
SCOPED_HYBRID_MAX_TOP_K = 64       # hiphybrid_search_scoped's depth limit (the scoped BM25 leg's k)
FLAT_MAGIC = b"HIPIDX01"
_METRIC_NAMES = {0: "ip", 1: "l2", "ip": "ip", "l2": "l2"}

_COLLECTION_CACHE: Dict[str, Tuple[float, "Collection"]] = {}     # manifest path -> (manifest mtime, loaded collection)
_LOCK = threading.Lock()


def _mv_format(mv) -> str:
    """a store's format; an object that names none holds bf16 vectors"""
    return getattr(mv, "format", "bf16")


def _mv_ncent(mv) -> int:
    """the centroids attached to a store; 0 for none, for no store, and for an object that knows of none"""
    info = getattr(mv, "centroid_info", None)
    return int(info()[0]) if info is not None else 0


def mv_entry(dim, fmt: str) -> Dict[str, Any]:
    """The manifest's "mv" entry: exactly {"dim": d} for a bf16 store (as before there was a second format), and
    {"dim": d, "format": "fp8"} or {"dim": d, "format": "mxfp4"} for a quantised one."""
    if fmt not in MV_FORMATS:
        raise ValueError(f"collection manifest: multi-vector format {fmt!r}, expected 'bf16', 'fp8' or 'mxfp4'")
    return {"dim": int(dim)} if fmt == "bf16" else {"dim": int(dim), "format": fmt}


class CollectionManifest:
    """The documents of a collection in row order.  Pure bookkeeping: no GPU, no files but its own."""

    def __init__(self, d: int, metric: str, documents: Optional[Iterable[Dict[str, Any]]] = None, generation: int = 0,
                 ivf: Optional[Dict[str, Any]] = None, mv: Optional[Dict[str, Any]] = None, lexical: Optional[Dict[str, Any]] = None,
                 mvc: Optional[Dict[str, Any]] = None):
        self.d = int(d)
        self.mvc = None if mvc is None else {"ncent": int(mvc["ncent"])}   # the multi-vector store's centroids; in the JSON only when there are any
        self.lexical = None if lexical is None else {"n_terms": int(lexical["n_terms"])}   # the lexical postings; in the JSON only when there are any
        self.mv = None if mv is None else mv_entry(mv["dim"], mv.get("format", "bf16"))   # the multi-vector store; in the JSON only when there is one
        self.ivf = None if ivf is None else {"nlist": int(ivf["nlist"])}     # the IVF companion; in the JSON only when there is one
        self.metric = _METRIC_NAMES[metric]
        self.documents: List[Dict[str, Any]] = []
        self._row0: List[int] = []
        self._by_id: Dict[str, int] = {}
        self.generation = int(generation)      # removals and replacements so far; in the JSON only when > 0
        for doc in documents or []:
            if int(doc["row0"]) != self.rows:
                raise ValueError(f"collection manifest: document {doc['doc_id']!r} starts at row {doc['row0']}, expected {self.rows}")
            self.add_document(doc["doc_id"], doc.get("project"), int(doc["rows"]))

    @property
    def rows(self) -> int:
        return self._row0[-1] + self.documents[-1]["rows"] if self.documents else 0

    def check_new(self, doc_id: str) -> None:
        if doc_id in self._by_id:
            raise ValueError(f"document {doc_id!r} is already in the collection (replace_document / index_chunks(replace=True) "
                             f"replaces it)")

    def add_document(self, doc_id: str, project: Optional[str], rows: int) -> Tuple[int, int]:
        """Append a document of `rows` rows; returns its row range [lo, hi).  A doc_id already present raises ValueError
        (remove_documents takes it out first)."""
        self.check_new(doc_id)
        if rows < 0:
            raise ValueError(f"document {doc_id!r}: rows = {rows}")
        lo = self.rows
        self._by_id[doc_id] = len(self.documents)
        self._row0.append(lo)
        self.documents.append({"doc_id": doc_id, "project": project, "row0": lo, "rows": int(rows)})
        return lo, lo + int(rows)

    def remove_documents(self, doc_ids: Iterable[str]) -> List[Tuple[int, int]]:
        """Drop the entries of `doc_ids`; returns their row ranges [(lo, hi)] in the numbering BEFORE the removal, ascending,
        adjacent ranges coalesced, empty documents left out -- the table hipidx_remove_ranges takes.  Everything behind a
        removed document is re-based (row0 falls by the rows removed before it) and `generation` is bumped.  An unknown
        doc_id raises KeyError and changes nothing."""
        gone = set(doc_ids)
        for doc_id in gone:
            if doc_id not in self._by_id:
                raise KeyError(f"document {doc_id!r} is not in the collection")
        if not gone:
            return []
        ranges: List[Tuple[int, int]] = []
        kept: List[Dict[str, Any]] = []
        cut = 0
        for doc in self.documents:
            lo, hi = doc["row0"], doc["row0"] + doc["rows"]
            if doc["doc_id"] in gone:
                cut += hi - lo
                if hi > lo:
                    if ranges and ranges[-1][1] == lo:
                        ranges[-1] = (ranges[-1][0], hi)
                    else:
                        ranges.append((lo, hi))
            else:
                kept.append({"doc_id": doc["doc_id"], "project": doc["project"], "row0": lo - cut, "rows": doc["rows"]})
        self.documents = kept
        self._row0 = [doc["row0"] for doc in kept]
        self._by_id = {doc["doc_id"]: i for i, doc in enumerate(kept)}
        self.generation += 1
        return ranges

    def __contains__(self, doc_id) -> bool:
        return doc_id in self._by_id

    def scope_for(self, project: Optional[str] = None, doc_ids: Optional[Sequence[str]] = None) -> List[Tuple[int, int]]:
        """Row ranges [(lo, hi)] of the documents selected -- those of `project` (if given) and among `doc_ids` (if given) --
        ascending, ADJACENT RANGES COALESCED, empty documents left out.  Neither given: the whole collection.  An unknown
        project or doc_id selects nothing: []."""
        wanted = None if doc_ids is None else set(doc_ids)
        scope: List[Tuple[int, int]] = []
        for doc in self.documents:
            if project is not None and doc["project"] != project:
                continue
            if wanted is not None and doc["doc_id"] not in wanted:
                continue
            lo, hi = doc["row0"], doc["row0"] + doc["rows"]
            if hi == lo:
                continue
            if scope and scope[-1][1] == lo:
                scope[-1] = (scope[-1][0], hi)
            else:
                scope.append((lo, hi))
        return scope

    def locate(self, row: int) -> Tuple[str, int]:
        """(doc_id, row inside the document) of a collection row, by bisection."""
        if row < 0 or row >= self.rows:
            raise IndexError(f"row {row} is outside the collection's {self.rows} rows")
        i = bisect.bisect_right(self._row0, row) - 1      # the LAST document that starts at or before row: never an empty one
        return self.documents[i]["doc_id"], row - self._row0[i]

    def projects(self) -> List[Optional[str]]:
        seen: List[Optional[str]] = []
        for doc in self.documents:
            if doc["project"] not in seen:
                seen.append(doc["project"])
        return seen

    def to_json(self) -> Dict[str, Any]:
        out = {"version": MANIFEST_VERSION, "d": self.d, "metric": self.metric, "documents": self.documents}
        if self.generation > 0:        # a manifest that never saw a removal stays byte for byte what it was
            out["generation"] = self.generation
        if self.ivf is not None:       # and one without a companion
            out["ivf"] = self.ivf
        if self.mv is not None:        # and one without per-token vectors
            out["mv"] = self.mv
        if self.lexical is not None:   # and one without lexical postings
            out["lexical"] = self.lexical
        if self.mvc is not None:       # and one without token centroids
            out["mvc"] = self.mvc
        return out

    def save(self, path) -> None:
        """Atomic: a temp file beside the target, flushed to disk, then renamed over it."""
        path = Path(path)
        tmp = path.with_name(path.name + f".tmp{os.getpid()}")
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(self.to_json(), f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)

    @classmethod
    def load(cls, path) -> "CollectionManifest":
        with open(path, "r", encoding="utf-8") as f:
            data = json.load(f)
        if data.get("version") != MANIFEST_VERSION:
            raise ValueError(f"{path}: collection manifest version {data.get('version')!r}, expected {MANIFEST_VERSION}")
        return cls(data["d"], data["metric"], data["documents"], generation=int(data.get("generation", 0)), ivf=data.get("ivf"),
                   mv=data.get("mv"), lexical=data.get("lexical"), mvc=data.get("mvc"))


class Collection:
    """A manifest, the flat index that holds its rows and, once trained, the IVF companion over the same rows."""

    def __init__(self, storage_dir, manifest: CollectionManifest, index, ivf=None, mv=None, lex=None):
        self.storage_dir = Path(storage_dir)
        self.manifest = manifest
        self.index = index
        self.ivf = ivf                 # HipIVFIndex whose ids are this collection's rows, or None
        self.mv = mv                   # hiprag.MultiVectorStore whose documents are this collection's rows, or None
        if ivf is not None:
            manifest.ivf = {"nlist": int(ivf.nlist)}
        manifest.mv = None if mv is None else mv_entry(mv.dim, _mv_format(mv))
        manifest.mvc = {"ncent": _mv_ncent(mv)} if _mv_ncent(mv) else None
        self._mvc_dirty = False        # the attached table is not the one in the centroid file
        self._mv_format_logged = False
        self.lex = lex                 # hiprag.LexicalIndexUpdatable whose documents are this collection's rows, or None
        manifest.lexical = None if lex is None else {"n_terms": int(lex.n_terms)}

    @property
    def index_path(self) -> Path:
        return self.storage_dir / COLLECTION_INDEX

    @property
    def manifest_path(self) -> Path:
        return self.storage_dir / COLLECTION_MANIFEST

    @property
    def ivf_path(self) -> Path:
        return self.storage_dir / COLLECTION_IVF

    @property
    def mv_path(self) -> Path:
        return self.storage_dir / COLLECTION_MV

    @property
    def mvc_path(self) -> Path:
        return self.storage_dir / COLLECTION_MVC

    @property
    def lexical_path(self) -> Path:
        return self.storage_dir / COLLECTION_LEXICAL

    def _check_lexical(self, lexical) -> None:
        """Before an append, as _check_colbert: a collection with lexical postings takes the rows of every document, one
        without takes none unless it is still empty.  Nothing is encoded again behind the caller's back."""
        if self.lex is not None:
            if lexical is None:
                raise RuntimeError("this collection keeps lexical postings (hip_collection.lexical.npz): ingest with "
                                   "HIP_COLLECTION_SPARSE=lexical")
            if self.lex.n_docs != self.manifest.rows:
                raise RuntimeError(f"the collection's lexical postings hold {self.lex.n_docs} documents, its manifest "
                                   f"{self.manifest.rows} rows")
        elif lexical is not None and self.manifest.rows > 0:
            raise RuntimeError("this collection was ingested without lexical weights: HIP_COLLECTION_SPARSE=lexical needs a "
                               "collection built under it from its first document")

    def _check_colbert(self, colbert) -> None:
        """Before an append: a collection with per-token vectors takes them for every document, one without takes none
        unless it is still empty (the store then starts with it).  Nothing is encoded again behind the caller's back."""
        if self.mv is not None:
            if colbert is None:
                raise RuntimeError("this collection keeps per-token vectors (hip_collection.mv): ingest with HIP_LATE_INTERACTION=true")
            if len(self.mv) != self.manifest.rows:
                raise RuntimeError(f"the collection's multi-vector store holds {len(self.mv)} documents, its manifest "
                                   f"{self.manifest.rows} rows")
        elif colbert is not None and self.manifest.rows > 0:
            raise RuntimeError("this collection was ingested without per-token vectors: HIP_LATE_INTERACTION=true needs a "
                               "collection built under it from its first document")
        if colbert is not None:
            fmt = config.HIP_COLBERT_FORMAT         # a value that is none of the three names raises here, before any row is added
            dim = int(colbert[0].shape[2])
            if self.mv is None and fmt != "bf16" and (dim % 128 or not 128 <= dim <= 1024):
                raise ValueError(f"HIP_COLBERT_FORMAT={fmt} needs per-token vectors of a dimension that is a multiple of 128 in 128..1024 (got {dim})")

    def append(self, doc_id: str, project: Optional[str], embeddings, colbert=None, lexical=None) -> Tuple[int, int]:
        """Add a document's vectors (CUDA tensor -> add_device, anything else -> add); row range = [ntotal before, after).
        `colbert`: (token vectors bfloat16 CUDA [rows, stride, dim], counts int32 [rows]) of the same chunks, what
        embed_batch_colbert_device returns behind the embeddings; they go to the multi-vector store.
        `lexical`: (terms int32 [rows, L], weights float32 [rows, L], counts int32 [rows]) of the same chunks, the CUDA tensors
        embed_batch_lexical_device returns behind the embeddings, optionally followed by the vocabulary size; they go to the
        lexical postings on the device."""
        self.manifest.check_new(doc_id)                     # before any row is added
        self._check_colbert(colbert)
        self._check_lexical(lexical)
        if lexical is not None and int(lexical[2].shape[0]) != int(embeddings.shape[0]):
            raise ValueError(f"document {doc_id!r}: {int(lexical[2].shape[0])} lexical rows for {int(embeddings.shape[0])} rows")
        if colbert is not None and int(colbert[0].shape[0]) != int(embeddings.shape[0]):
            raise ValueError(f"document {doc_id!r}: {int(colbert[0].shape[0])} token-vector blocks for {int(embeddings.shape[0])} rows")
        before = self.index.ntotal
        if before != self.manifest.rows:
            raise RuntimeError(f"collection index holds {before} rows, its manifest {self.manifest.rows}")
        self._check_ivf()
        if hasattr(embeddings, "is_cuda") and embeddings.is_cuda:
            self.index.add_device(embeddings)
        else:
            embeddings = np.asarray(embeddings, dtype=np.float32)
            self.index.add(embeddings)
        if self.ivf is not None:
            self.ivf.add(embeddings)                        # ids ntotal .. : the rows the flat index has just given them
        if colbert is not None:
            if self.mv is None:
                from hiprag import MultiVectorStore
                self.mv = MultiVectorStore(int(colbert[0].shape[2]), max_doc_vectors=MV_MAX_DOC_VECTORS, device=config.HIP_DEVICE,
                                           format=config.HIP_COLBERT_FORMAT)      # the setting applies HERE, when the store is created
                self.manifest.mv = mv_entry(self.mv.dim, _mv_format(self.mv))
            elif config.HIP_COLBERT_FORMAT != _mv_format(self.mv) and not self._mv_format_logged:
                self._mv_format_logged = True
                logger.info(f"The collection's multi-vector store is {_mv_format(self.mv)}: it keeps its format, HIP_COLBERT_FORMAT="
                            f"{config.HIP_COLBERT_FORMAT} applies to new collections (Collection.convert_multivectors converts one)")
            counts = colbert[1].cpu().numpy() if hasattr(colbert[1], "cpu") else colbert[1]
            self.mv.append_device(colbert[0], counts)       # documents n .. : the same rows
        if lexical is not None:
            terms, weights, counts = lexical[:3]
            if self.lex is None:
                from hiprag import LexicalIndexUpdatable
                self.lex = LexicalIndexUpdatable(device=config.HIP_DEVICE)
            # the vocabulary only grows.  A fourth member names its size (the ingest passes the encoder's); without one it
            # reaches as far as the largest term id seen (a query term beyond it scores nothing)
            if len(lexical) > 3:
                top = int(lexical[3])
            else:
                used = terms.masked_fill(_beyond_counts(terms, counts), -1)
                top = int(used.max()) + 1 if used.numel() else 0
            self.lex.append_rows(terms, weights, counts, n_terms_after=max(self.lex.n_terms, top))     # documents n .. : the same rows
            self.manifest.lexical = {"n_terms": int(self.lex.n_terms)}
        return self.manifest.add_document(doc_id, project, self.index.ntotal - before)

    def remove(self, doc_ids: Iterable[str]) -> int:
        """Take documents out: their entries leave the manifest, their rows the index (hipidx_remove_ranges -- on the device,
        in place, the rows behind them move down in order).  Returns the rows removed.  Unknown doc_id: KeyError, nothing
        changed."""
        if self.index.ntotal != self.manifest.rows:
            raise RuntimeError(f"collection index holds {self.index.ntotal} rows, its manifest {self.manifest.rows}")
        self._check_ivf()
        ranges = self.manifest.remove_documents(doc_ids)
        if ranges and self.ivf is not None:
            self.ivf.remove_ranges(ranges)                  # the same table: both renumber the survivors densely, in order
        if ranges and self.mv is not None:
            self.mv.remove_ranges(ranges)                   # and so does the multi-vector store
        if ranges and self.lex is not None:
            self.lex.remove_ranges(ranges)                  # and the lexical postings (hipbm25_remove_ranges on the impact handle)
        return self.index.remove_ranges(ranges) if ranges else 0

    def _check_ivf(self) -> None:
        if self.ivf is not None and self.ivf.ntotal != self.manifest.rows:
            raise RuntimeError(f"the collection's IVF companion holds {self.ivf.ntotal} rows, its manifest {self.manifest.rows} "
                               f"(train_collection_ivf rebuilds it)")

    def convert_multivectors(self, fmt: str = "fp8") -> None:
        """Convert the collection's bf16 multi-vector store to fp8 or mxfp4 on the device (hipmv_to_fp8 / hipmv_to_mxfp4: byte
        for byte the store an ingest under that HIP_COLBERT_FORMAT would have built) and save: the file, then the manifest, in
        save's order.  A store that has the format already is left alone; a quantised store is not converted again, neither
        back to bf16 (the codes have lost the bits) nor to the other quantised format (no second quantisation)."""
        if fmt not in MV_FORMATS:
            raise ValueError(f"convert_multivectors({fmt!r}): expected 'bf16', 'fp8' or 'mxfp4'")
        if self.mv is None:
            raise RuntimeError("this collection keeps no per-token vectors: there is nothing to convert")
        if self.mv.format == fmt:
            return
        if self.mv.format != "bf16":
            raise RuntimeError(f"{'an' if self.mv.format == 'fp8' else 'a'} {self.mv.format} multi-vector store cannot be converted to {fmt}: ingest the collection again")
        if len(self.mv) != self.manifest.rows:
            raise RuntimeError(f"the collection's multi-vector store holds {len(self.mv)} documents, its manifest {self.manifest.rows} rows")
        cent = self.mv.centroids() if _mv_ncent(self.mv) else None
        old, self.mv = self.mv, (self.mv.to_fp8() if fmt == "fp8" else self.mv.to_mxfp4())
        old.close()
        if cent is not None:           # the converted store comes unattached: the same table, codes of the quantised vectors
            self.mv.attach_centroids(cent)
        self.save()

    def save(self) -> None:
        """Index file first (a temp file, renamed over the target), then the IVF companion when there is one (the same way),
        then the manifest: a crash in between leaves files whose row counts disagree with the manifest's, which
        open_collection detects and names rebuild_collection (index) or train_collection_ivf (companion) for."""
        files = [(self.index, self.index_path)]
        if self.ivf is not None:
            files.append((self.ivf, self.ivf_path))
            self.manifest.ivf = {"nlist": int(self.ivf.nlist)}
        else:
            self.manifest.ivf = None
        if self.mv is not None:
            files.append((self.mv, self.mv_path))
            self.manifest.mv = mv_entry(self.mv.dim, _mv_format(self.mv))
        else:
            self.manifest.mv = None
        ncent = _mv_ncent(self.mv)
        self.manifest.mvc = {"ncent": ncent} if ncent else None
        if ncent and (self._mvc_dirty or not self.mvc_path.exists()):
            files.append((_CentroidFile(self.mv.centroids()), self.mvc_path))
            self._mvc_dirty = False
        if self.lex is not None:
            files.append((self.lex, self.lexical_path))
            self.manifest.lexical = {"n_terms": int(self.lex.n_terms)}
        else:
            self.manifest.lexical = None
        for index, path in files:
            tmp = path.with_name(path.name + f".tmp{os.getpid()}")
            try:
                index.save(str(tmp))
                os.replace(tmp, path)
            finally:
                if tmp.exists():
                    tmp.unlink()
        self.manifest.save(self.manifest_path)
        with _LOCK:
            _COLLECTION_CACHE[str(self.manifest_path)] = (self.manifest_path.stat().st_mtime, self)


class _CentroidFile:
    """the centroid table as save() writes its files: an object with save(path)"""

    def __init__(self, table):
        self.table = np.ascontiguousarray(table, dtype=np.uint16)

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            np.save(f, self.table)


def _hip():
    import rag.storage.hip_index as hi
    hi._require_hip()
    return hi


def _storage(storage_dir) -> Path:
    return Path(storage_dir) if storage_dir is not None else Path(config.STORAGE_DIR)


def open_collection(storage_dir=None) -> Optional[Collection]:
    """The collection of `storage_dir` (default STORAGE_DIR), loaded once per version of its manifest; None if there is none."""
    storage = _storage(storage_dir)
    mpath = storage / COLLECTION_MANIFEST
    if not mpath.exists():
        return None
    hi = _hip()
    mtime = mpath.stat().st_mtime
    key = str(mpath)
    with _LOCK:
        hit = _COLLECTION_CACHE.get(key)
        if hit is not None and hit[0] == mtime:
            return hit[1]
    manifest = CollectionManifest.load(mpath)
    try:
        index = hi.HipFlatIndex.load(str(storage / COLLECTION_INDEX), device=config.HIP_DEVICE)
    except Exception as e:
        raise RuntimeError(f"Failed to load the HIP collection index: {e}")
    if index.ntotal != manifest.rows or index.d != manifest.d:
        raise RuntimeError(f"{storage / COLLECTION_INDEX}: {index.ntotal} rows of dimension {index.d}, the manifest names "
                           f"{manifest.rows} of dimension {manifest.d} (rebuild_collection restores the pair)")
    coll = Collection(storage, manifest, index, _load_companion(hi, storage, manifest), _load_multivec(storage, manifest),
                      _load_lexical(storage, manifest))
    with _LOCK:
        _COLLECTION_CACHE[key] = (mtime, coll)
    logger.info(f"Loaded HIP collection: {manifest.rows} vectors of {len(manifest.documents)} documents"
                + (f", IVF companion of {coll.ivf.nlist} lists" if coll.ivf is not None else ""))
    return coll


def _load_companion(hi, storage: Path, manifest: CollectionManifest):
    """the IVF companion the manifest names (None: it names none); a missing or stale file raises"""
    if manifest.ivf is None:
        return None
    path = storage / COLLECTION_IVF
    if not path.exists():
        raise RuntimeError(f"{path}: the collection manifest names an IVF companion of {manifest.ivf['nlist']} lists, the file is "
                           f"missing (train_collection_ivf builds it again)")
    try:
        ivf = hi.HipIVFIndex.load(str(path), device=config.HIP_DEVICE)
    except Exception as e:
        raise RuntimeError(f"Failed to load the collection's IVF companion: {e} (train_collection_ivf builds it again)")
    if ivf.ntotal != manifest.rows or ivf.d != manifest.d:
        raise RuntimeError(f"{path}: {ivf.ntotal} rows of dimension {ivf.d}, the manifest names {manifest.rows} of dimension "
                           f"{manifest.d} (train_collection_ivf builds it again)")
    return ivf


def _load_multivec(storage: Path, manifest: CollectionManifest):
    """the multi-vector store the manifest names (None: it names none), LOADED from its file; a missing file, or one whose
    document count or dimension is not the manifest's, raises: these vectors are never encoded again silently"""
    if manifest.mv is None:
        return None
    from hiprag import MultiVectorStore
    path = storage / COLLECTION_MV
    if not path.exists():
        raise RuntimeError(f"{path}: the collection manifest names a multi-vector store, the file is missing (ingest the "
                           f"collection again under HIP_LATE_INTERACTION=true)")
    try:
        mv = MultiVectorStore.load(str(path), device=config.HIP_DEVICE)
    except Exception as e:
        raise RuntimeError(f"Failed to load the collection's multi-vector store: {e}")
    want = manifest.mv.get("format", "bf16")
    if mv.format != want:
        raise RuntimeError(f"{path}: the file is a {mv.format} multi-vector store, the collection manifest names a {want} one")
    if len(mv) != manifest.rows or mv.dim != manifest.mv["dim"]:
        raise RuntimeError(f"{path}: the multi-vector store holds {len(mv)} documents of dimension {mv.dim}, the manifest names {manifest.rows} rows of "
                           f"dimension {manifest.mv['dim']} (ingest the collection again under HIP_LATE_INTERACTION=true)")
    if manifest.mvc is not None:       # codes are not stored: the table is, and attaching computes them again
        cpath = storage / COLLECTION_MVC
        if not cpath.exists():
            raise RuntimeError(f"{cpath}: the collection manifest names {manifest.mvc['ncent']} token centroids, the file is missing "
                               f"(train_collection_centroids trains them again)")
        try:
            table = np.load(cpath, allow_pickle=False)
        except Exception as e:
            raise RuntimeError(f"Failed to load the collection's token centroids: {e} (train_collection_centroids trains them again)")
        if table.dtype != np.uint16 or table.shape != (manifest.mvc["ncent"], mv.dim):
            raise RuntimeError(f"{cpath}: {table.dtype} {table.shape}, the manifest names uint16 ({manifest.mvc['ncent']}, {mv.dim}) "
                               f"(train_collection_centroids trains them again)")
        mv.attach_centroids(table)
    return mv


def _load_lexical(storage: Path, manifest: CollectionManifest):
    """the lexical postings the manifest names (None: it names none), LOADED from their file; a missing file, or one whose
    document count is not the manifest's rows, raises: these weights are never encoded again silently"""
    if manifest.lexical is None:
        return None
    from hiprag import LexicalIndexUpdatable
    path = storage / COLLECTION_LEXICAL
    if not path.exists():
        raise RuntimeError(f"{path}: the collection manifest names lexical postings, the file is missing (ingest the collection "
                           f"again under HIP_COLLECTION_SPARSE=lexical)")
    try:
        lex = LexicalIndexUpdatable.load(str(path), device=config.HIP_DEVICE)
    except Exception as e:
        raise RuntimeError(f"Failed to load the collection's lexical postings: {e}")
    if lex.n_docs != manifest.rows:
        lex.close()
        raise RuntimeError(f"{path}: the lexical postings hold {lex.n_docs} documents, the manifest names {manifest.rows} rows "
                           f"(ingest the collection again under HIP_COLLECTION_SPARSE=lexical)")
    return lex


def _beyond_counts(terms, counts):
    """mask [rows, L] of the entries of lexical rows that lie behind their row's count (CUDA tensors)"""
    import torch
    return torch.arange(terms.shape[1], device=terms.device)[None, :] >= counts[:, None]


def train_collection_ivf(storage_dir=None, nlist: int = 0, iters: int = IVF_TRAIN_ITERS) -> Collection:
    """Build the IVF companion of the collection of `storage_dir` over its current rows (HipIVFIndex.build: k-means on the
    GPU, `iters` rounds, trained on at most 256 rows per list as _create_ivf_index trains) and write it: the IVF file, then
    the manifest with "ivf": {"nlist": N}.  nlist = 0: ivf_auto_nlist(rows).  Replaces a companion that exists, stale or
    not.  From then on append / remove / save keep it in step, and HIP_INDEX_TYPE=ivf searches it."""
    hi = _hip()
    storage = _storage(storage_dir)
    mpath = storage / COLLECTION_MANIFEST
    if not mpath.exists():
        raise RuntimeError(f"{storage} holds no collection to train an IVF companion for")
    with _LOCK:
        _COLLECTION_CACHE.pop(str(mpath), None)
    manifest = CollectionManifest.load(mpath)
    manifest.ivf = None                                     # whatever it named: open the pair without it
    rows, _ = read_flat_rows(storage / COLLECTION_INDEX)
    if rows.shape[0] != manifest.rows or rows.shape[0] == 0:
        raise RuntimeError(f"{storage / COLLECTION_INDEX}: {rows.shape[0]} rows, the manifest names {manifest.rows}: an IVF companion "
                           f"needs a collection with rows whose files agree (rebuild_collection restores the pair)")
    index = hi.HipFlatIndex.load(str(storage / COLLECTION_INDEX), device=config.HIP_DEVICE)
    n = rows.shape[0]
    nlist = min(int(nlist) or ivf_auto_nlist(n), n)
    ivf = hi.HipIVFIndex(manifest.d, nlist, manifest.metric, device=config.HIP_DEVICE)
    ivf.build(rows, iters=int(iters), seed=0, max_train_rows=IVF_MAX_POINTS_PER_CENTROID * nlist)
    coll = Collection(storage, manifest, index, ivf, _load_multivec(storage, manifest), _load_lexical(storage, manifest))
    coll.save()
    logger.info(f"Trained the HIP collection's IVF companion: {n} vectors, nlist={nlist}")
    return coll


def train_collection_centroids(storage_dir=None, ncent: int = 0) -> Collection:
    """Train token centroids on the multi-vector store of the collection of `storage_dir` (hiprag.train_token_centroids: a
    strided sample of its stored vectors, spherical k-means on the GPU; ncent = 0: the power of two nearest 16 sqrt(stored
    vectors)), attach them, and write: hip_collection.mvc (the bf16 table as a uint16 .npy), then the manifest with
    "mvc": {"ncent": C}.  Replaces centroids that exist.  From then on append / remove keep the codes in step,
    open_collection attaches the table again, and HIP_LATE_CANDIDATES prunes the late-interaction search with it."""
    from hiprag import train_token_centroids
    storage = _storage(storage_dir)
    mpath = storage / COLLECTION_MANIFEST
    if not mpath.exists():
        raise RuntimeError(f"{storage} holds no collection to train token centroids for")
    with _LOCK:
        _COLLECTION_CACHE.pop(str(mpath), None)
    manifest = CollectionManifest.load(mpath)
    if manifest.mvc is not None:                            # whatever it named: open the collection without it
        manifest.mvc = None
        manifest.save(mpath)
    coll = open_collection(storage)
    if coll.mv is None:
        raise RuntimeError("the collection holds no per-token vectors to train centroids on: ingest it under HIP_LATE_INTERACTION=true")
    table = train_token_centroids(coll.mv, int(ncent))
    coll.mv.attach_centroids(table)
    coll._mvc_dirty = True
    coll.save()
    logger.info(f"Trained the HIP collection's token centroids: {coll.mv.sizes()[1]} vectors, ncent={len(table)}")
    return coll


def open_or_create_collection(d: int, storage_dir=None) -> Collection:
    """The collection of `storage_dir`, or a new empty one (dimension d, metric HIP_INDEX_METRIC; no file until save())."""
    hi = _hip()
    storage = _storage(storage_dir)
    coll = open_collection(storage)
    if coll is None:
        index = hi.HipFlatIndex(int(d), config.HIP_INDEX_METRIC, device=config.HIP_DEVICE)
        coll = Collection(storage, CollectionManifest(d, _METRIC_NAMES[index.metric]), index)
    return coll


def append_document(doc_id: str, project: Optional[str], embeddings, storage_dir=None, texts: Optional[Sequence[str]] = None,
                    colbert=None, lexical=None) -> Tuple[int, int]:
    """Append a document to the collection of `storage_dir` (created on the first call) and write both files; returns its
    row range.  Every call rewrites the index file: a bulk ingest appends to one Collection and saves once, or runs
    rebuild_collection afterwards.  A doc_id already present raises ValueError (replace_document replaces it).
    `texts`: the document's chunk texts in row order (index_chunks passes them; None: its chunk table is read) -- live
    collection postings take them on the device (sparse.follow_collection).
    `colbert` / `lexical`: the per-token vectors / the lexical rows of the same chunks (Collection.append)."""
    from rag.storage.hip_index import pages, passages, sparse
    coll = open_or_create_collection(_dim_of(embeddings), storage_dir)
    live = sparse.live_collection_sparse(coll)
    live_tok = passages.live_collection_tokens(coll)       # the passage token store follows beside the postings
    live_pg = pages.live_collection_pages(coll)            # and so does the page table
    rng = coll.append(doc_id, project, embeddings, colbert=colbert, lexical=lexical)
    coll.save()
    if live_pg is not None:
        pages.follow_collection_pages(coll, live_pg, [], _chunk_pages(coll, doc_id))
    if live is not None or live_tok is not None:
        new_texts = _chunk_texts(coll, doc_id, rng, texts)
        if live is not None:
            sparse.follow_collection(coll, live, [], new_texts)
        passages.follow_collection_tokens(coll, live_tok, [], new_texts)
    return rng


def _chunk_texts(coll: "Collection", doc_id: str, rng: Tuple[int, int], texts: Optional[Sequence[str]]) -> List[str]:
    """the chunk texts the live postings take for rows `rng`: those given, else the document's chunk table; a count that is
    not the row count comes back as it is and makes follow_collection drop the postings (the rebuild then raises as ever)"""
    if texts is not None:
        return list(texts)
    try:
        return [c.get("text", "") for c in _hip()._load_chunk_list(coll.storage_dir, doc_id)]
    except Exception:                 # noqa: BLE001 -- no table: nothing to append, the count check drops the postings
        return []


def _chunk_pages(coll: "Collection", doc_id: str) -> list:
    """the chunk pages the live page table takes for a document's rows, from its chunk table; no table: nothing, and the
    row count check drops the page table"""
    from rag.storage.hip_index import pages
    try:
        return pages.chunk_pages(coll.storage_dir, doc_id)
    except Exception:                 # noqa: BLE001
        return []


def _dim_of(embeddings) -> int:
    return int(embeddings.shape[1]) if hasattr(embeddings, "shape") else len(embeddings[0])


def _forget_document(storage: Path, doc_id: str, sparse_too: bool) -> None:
    """the cached chunk table of a document whose rows have left or changed (the table is cached by mtime, and a re-ingest
    may rewrite it within one tick) and, for a deleted one, its sparse index"""
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import sparse
    with hi._LOCK:
        hi._CHUNK_CACHE.pop(str(storage / f"{doc_id}_chunks.json"), None)
    if sparse_too:
        with sparse._LOCK:
            sparse._SPARSE_CACHE.pop(str(storage / doc_id), None)


def delete_document(doc_id: str, storage_dir=None) -> int:
    """Take `doc_id` out of the collection of `storage_dir` and write both files; returns the rows removed.  Its
    `{doc_id}_hip.index` is unlinked too, so that rebuild_collection does not resurrect it; its cached chunk table and
    sparse index are dropped.  The chunk-table FILE belongs to the ingest pipeline and stays.  No collection, or a doc_id
    it does not hold: KeyError."""
    hi = _hip()
    storage = _storage(storage_dir)
    coll = open_collection(storage)
    if coll is None:
        raise KeyError(f"document {doc_id!r}: {storage} holds no collection")
    from rag.storage.hip_index import pages, passages, sparse
    live = sparse.live_collection_sparse(coll)
    live_tok = passages.live_collection_tokens(coll)
    live_pg = pages.live_collection_pages(coll)
    ranges = coll.manifest.scope_for(doc_ids=[doc_id]) if doc_id in coll.manifest else []
    removed = coll.remove([doc_id])
    coll.save()
    sparse.follow_collection(coll, live, ranges, None)
    passages.follow_collection_tokens(coll, live_tok, ranges, None)
    pages.follow_collection_pages(coll, live_pg, ranges, None)
    per_doc = storage / f"{doc_id}{hi.INDEX_SUFFIX}"
    if per_doc.exists():
        per_doc.unlink()
    with hi._LOCK:
        hi._INDEX_CACHE.pop(str(per_doc), None)
    _forget_document(storage, doc_id, sparse_too=True)
    logger.info(f"Deleted {doc_id} from the HIP collection: {removed} vectors")
    return removed


def replace_document(doc_id: str, project: Optional[str], embeddings, storage_dir=None, texts: Optional[Sequence[str]] = None,
                     colbert=None, lexical=None) -> Tuple[int, int]:
    """The overwrite-on-re-ingest of the reference (rag/ingest/ingestion_pipeline.py:80-94 writes {doc_id}_faiss.index again)
    for the collection: the document's old rows are removed if it is present, the new ones appended at the END, one save.
    Returns the new row range.  Live collection postings follow on the device: the old row range removed, `texts` (as in
    append_document) appended."""
    from rag.storage.hip_index import pages, passages, sparse
    storage = _storage(storage_dir)
    coll = open_or_create_collection(_dim_of(embeddings), storage)
    live = sparse.live_collection_sparse(coll)
    live_tok = passages.live_collection_tokens(coll)
    live_pg = pages.live_collection_pages(coll)
    ranges: List[Tuple[int, int]] = []
    coll._check_colbert(colbert)            # before the old rows leave
    coll._check_lexical(lexical)
    if doc_id in coll.manifest:
        ranges = coll.manifest.scope_for(doc_ids=[doc_id])
        coll.remove([doc_id])
    else:
        coll.manifest.generation += 1      # a replacement, whatever it found
    rng = coll.append(doc_id, project, embeddings, colbert=colbert, lexical=lexical)
    coll.save()
    if live is not None or live_tok is not None:
        if texts is None:
            _forget_document(storage, doc_id, sparse_too=False)     # the chunk table read below is the re-ingested one
        new_texts = _chunk_texts(coll, doc_id, rng, texts)
        if live is not None:
            sparse.follow_collection(coll, live, ranges, new_texts)
        passages.follow_collection_tokens(coll, live_tok, ranges, new_texts)
    if live_pg is not None:
        _forget_document(storage, doc_id, sparse_too=False)         # the pages come from the re-ingested chunk table
        pages.follow_collection_pages(coll, live_pg, ranges, _chunk_pages(coll, doc_id))
    _forget_document(storage, doc_id, sparse_too=False)   # the ingest has just put this document's postings
    return rng


def read_flat_rows(path) -> Tuple[np.ndarray, int]:
    """(rows float32 [n, d], metric) of a HIPIDX01 file: magic[8], int32 d, int32 metric, int64 ntotal, row-major fp32."""
    with open(path, "rb") as f:
        head = f.read(24)
        if head[:8] != FLAT_MAGIC:
            raise ValueError(f"{path} is not a HIPIDX01 file")
        d, metric, n = struct.unpack("<iiq", head[8:])
        rows = np.fromfile(f, dtype=np.float32, count=n * d)
    if rows.size != n * d:
        raise ValueError(f"{path} is truncated: {rows.size} of {n * d} values")
    return rows.reshape(n, d), metric


def rebuild_collection(storage_dir=None, projects: Optional[Dict[str, Optional[str]]] = None) -> Optional[Collection]:
    """Build hip_collection.index / .json from the per-document flat `*_hip.index` files of `storage_dir`, in sorted doc_id
    order; `projects` maps doc_id -> project (missing: None).  IVF files are skipped with a warning (their rows are stored
    permuted).  Replaces an existing collection; returns None when there is no flat file."""
    hi = _hip()
    storage = _storage(storage_dir)
    projects = projects or {}
    files = {f.name[:-len(hi.INDEX_SUFFIX)]: f for f in storage.glob(f"*{hi.INDEX_SUFFIX}")}
    coll: Optional[Collection] = None
    for doc_id in sorted(files):
        if hi._is_ivf_file(str(files[doc_id])):
            logger.warning(f"Skipping {doc_id}: {files[doc_id].name} is an IVF index, the collection takes flat files")
            continue
        rows, metric = read_flat_rows(files[doc_id])
        if coll is None:
            index = hi.HipFlatIndex(rows.shape[1], _METRIC_NAMES[metric], device=config.HIP_DEVICE)
            coll = Collection(storage, CollectionManifest(rows.shape[1], _METRIC_NAMES[metric]), index)
        elif rows.shape[1] != coll.manifest.d or _METRIC_NAMES[metric] != coll.manifest.metric:
            raise ValueError(f"{files[doc_id].name}: dimension {rows.shape[1]} / metric {_METRIC_NAMES[metric]} differ from the "
                             f"collection's {coll.manifest.d} / {coll.manifest.metric}")
        coll.append(doc_id, projects.get(doc_id), rows)
    if coll is None:
        return None
    coll.save()                                   # no companion: the manifest has no "ivf" key
    stale = storage / COLLECTION_IVF              # one trained over the rows this replaces
    if stale.exists():
        stale.unlink()
        logger.info(f"Dropped the stale IVF companion {stale.name} (train_collection_ivf builds one over the new rows)")
    stale = storage / COLLECTION_MV               # per-token vectors of the rows this replaces: the per-document files hold none
    if stale.exists():
        stale.unlink()
        logger.info(f"Dropped the stale multi-vector store {stale.name} (an ingest under HIP_LATE_INTERACTION builds it again)")
    stale = storage / COLLECTION_MVC              # and the centroids trained on them
    if stale.exists():
        stale.unlink()
        logger.info(f"Dropped the stale token centroids {stale.name} (train_collection_centroids trains them again)")
    stale = storage / COLLECTION_LEXICAL          # lexical weights of the rows this replaces: the per-document files are not theirs
    if stale.exists():
        stale.unlink()
        logger.info(f"Dropped the stale lexical postings {stale.name} (an ingest under HIP_COLLECTION_SPARSE=lexical builds them again)")
    logger.info(f"Rebuilt HIP collection: {coll.manifest.rows} vectors of {len(coll.manifest.documents)} documents")
    return coll


def _transform(coll: Collection, values, ids) -> List[Tuple[int, float]]:
    """HipIndexReader.search's score transform; padding rows (id -1) dropped"""
    l2 = coll.index.metric == 1
    out = []
    for idx, val in zip(ids, values):
        if idx < 0:
            continue
        val = float(val)
        score = 1.0 - (val / 2.0) if l2 else val
        out.append((int(idx), float(max(0.0, min(1.0, score)))))
    return out


def _enrich(coll: Collection, results: List[Tuple[int, float]]) -> List[dict]:
    """every row against ITS document's chunk table, plus "doc_id" (as search_all_documents)"""
    hi = _hip()
    rows = []
    for row, score in results:
        doc_id, local = coll.manifest.locate(row)
        for r in hi.enrich([(local, score)], hi._load_chunk_list(coll.storage_dir, doc_id), compat_minus_one=False):
            r["doc_id"] = doc_id
            rows.append(r)
    return rows


def _check_limit(limit: int) -> None:
    if limit > SCOPED_MAX_TOP_K:
        raise RuntimeError(f"limit={limit} is beyond what a scoped search returns ({SCOPED_MAX_TOP_K}): a `project` was "
                           f"given and HIP_COLLECTION is on")


def _ivf_nprobe(coll: Collection) -> Optional[int]:
    """the lists a search of the IVF companion probes, or None when the flat index answers: HIP_INDEX_TYPE is not "ivf", or
    there is no companion"""
    if coll.ivf is None or config.HIP_INDEX_TYPE != "ivf":
        return None
    return max(1, min(config.HIP_IVF_NPROBE, coll.ivf.nlist))


def _ivf_probe() -> Dict[str, str]:
    """the probe argument of a scoped search of the companion: none at HIP_IVF_PROBE=any (the default call, unchanged)"""
    mode = config.HIP_IVF_PROBE
    return {} if mode == "any" else {"probe": mode}


def search_collection(query_vector: List[float], limit: int = 50, project: Optional[str] = None, storage_dir=None) -> List[dict]:
    """search_hip_by_vector under HIP_COLLECTION: `project=None` -> the ordinary search over the whole collection; a project
    -> ONE scoped search over scope_for(project).  Enriched rows in score order; an unknown project or no collection -> []."""
    coll = open_collection(storage_dir)
    if coll is None or coll.manifest.rows == 0:
        logger.warning("No HIP indices found")
        return []
    q = np.array([query_vector], dtype=np.float32)
    nprobe = _ivf_nprobe(coll)                  # None: the flat index answers
    if project is None:
        values, ids = coll.index.search(q, limit) if nprobe is None else coll.ivf.search(q, limit, nprobe)
    else:
        _check_limit(limit)
        scope = coll.manifest.scope_for(project)
        if not scope:
            logger.warning(f"No HIP indices found for project {project!r}")
            return []
        if nprobe is None:
            values, ids = coll.index.search_scoped(q, limit, [scope])
        else:
            values, ids = coll.ivf.search_scoped(q, limit, [scope], nprobe=nprobe, **_ivf_probe())
    return _enrich(coll, _transform(coll, values[0], ids[0]))


def search_collection_batch(vectors, limit: int, projects: Sequence[Optional[str]], storage_dir=None) -> List[List[dict]]:
    """Many queries in ONE scoped search: query i searches the documents of projects[i] (None = the whole collection), one
    scope per distinct project, so queries of one project share the reads of its rows."""
    vectors = np.asarray(vectors, dtype=np.float32)
    if vectors.ndim != 2 or len(projects) != vectors.shape[0]:
        raise ValueError(f"search_collection_batch: {vectors.shape} vectors, {len(projects)} projects")
    _check_limit(limit)
    coll = open_collection(storage_dir)
    if coll is None or coll.manifest.rows == 0 or vectors.shape[0] == 0:
        if vectors.shape[0]:
            logger.warning("No HIP indices found")
        return [[] for _ in projects]
    distinct: List[Optional[str]] = []
    for p in projects:
        if p not in distinct:
            distinct.append(p)
    scopes = [coll.manifest.scope_for(p) for p in distinct]
    for p, s in zip(distinct, scopes):
        if not s:
            logger.warning(f"No HIP indices found for project {p!r}")
    soq = np.array([distinct.index(p) for p in projects], dtype=np.int32)
    nprobe = _ivf_nprobe(coll)
    if nprobe is None:
        values, ids = coll.index.search_scoped(vectors, limit, scopes, soq)
    elif distinct == [None]:
        values, ids = coll.ivf.search_batch(vectors, limit, nprobe)
    else:
        values, ids = coll.ivf.search_scoped(vectors, limit, scopes, soq, nprobe=nprobe, **_ivf_probe())
    return [_enrich(coll, _transform(coll, values[i], ids[i])) for i in range(vectors.shape[0])]


def search_collection_maxsim_device(q_vecs, q_counts, limit: int = 50, project: Optional[str] = None,
                                    storage_dir=None) -> Optional[Dict[str, Any]]:
    """Late interaction as the FIRST stage (HIP_LATE_SEARCH): the exact MaxSim top-`limit` over every chunk of
    scope_for(project) (`project=None`: the whole collection) in ONE library call, hipmaxsim_search_scoped_dev, on torch's
    current stream.  q_vecs bfloat16 [1, q_stride, dim] and q_counts int32 [1]: the CUDA tensors of embed_single_colbert.
    -> {"coll", "cand_ids" int64 [1, limit] (collection rows in MaxSim order, -1 past the chunks that hold a vector),
    "colbert_scores" float32 [1, limit]}, CUDA tensors, nothing synchronised; None where the host forms return [] (no
    collection, no rows, unknown project).  A collection without per-token vectors raises."""
    from hiprag import maxsim_search_device
    _check_limit(limit)
    coll = open_collection(storage_dir)
    if coll is None or coll.manifest.rows == 0:
        logger.warning("No HIP indices found")
        return None
    if coll.mv is None:
        raise RuntimeError("HIP_LATE_SEARCH=true, but the collection holds no per-token vectors: ingest it under "
                           "HIP_LATE_INTERACTION=true")
    scope = coll.manifest.scope_for(project)
    if not scope:
        logger.warning(f"No HIP indices found for project {project!r}")
        return None
    ncand = config.HIP_LATE_CANDIDATES           # raises without HIP_LATE_SEARCH=true
    if ncand:
        from hiprag import maxsim_search_pruned_device
        if not _mv_ncent(coll.mv):
            raise RuntimeError("HIP_LATE_CANDIDATES is set, but the collection's multi-vector store has no centroids: "
                               "train_collection_centroids trains and attaches them")
        scores, ids = maxsim_search_pruned_device(coll.mv, q_vecs, q_counts, [scope], None, int(limit), max(int(limit), ncand))
    else:
        scores, ids = maxsim_search_device(coll.mv, q_vecs, q_counts, [scope], None, int(limit))
    return {"coll": coll, "cand_ids": ids, "colbert_scores": scores}


def search_collection_maxsim(q_vecs, q_counts, limit: int = 50, project: Optional[str] = None, storage_dir=None,
                             query_vector: Optional[List[float]] = None) -> List[dict]:
    """search_collection_maxsim_device read back: the project's chunks in MaxSim order, enriched like search_collection's
    rows, each with "colbert_score".  "score" is the chunk's exact dense similarity to `query_vector` (ONE score_ids call on
    the flat index, the reader's transform) when one is given, else 0.0.  Unknown project / no collection -> []."""
    found = search_collection_maxsim_device(q_vecs, q_counts, limit, project, storage_dir)
    if found is None:
        return []
    coll = found["coll"]
    ids, colbert = found["cand_ids"][0].tolist(), found["colbert_scores"][0].tolist()
    rows = [(int(r), float(s)) for r, s in zip(ids, colbert) if r >= 0]
    dense: Dict[int, float] = {}
    if query_vector is not None and rows:
        values = coll.index.score_ids(np.array([query_vector], dtype=np.float32), np.array([[r for r, _ in rows]], dtype=np.int64),
                                      return64=True)
        dense = dict(_transform(coll, values[0].tolist(), [r for r, _ in rows]))
    out = []
    for row, cs in rows:
        for item in _enrich(coll, [(row, dense.get(row, 0.0))]):
            item["colbert_score"] = cs
            out.append(item)
    return out


def collection_texts(manifest: CollectionManifest, storage_dir=None) -> List[str]:
    """The chunk texts of every document of `manifest` IN ROW ORDER: entry i is collection row i.  A chunk table whose
    length differs from the rows its manifest entry names raises: a posting (or a stored passage) would otherwise point at
    another document's row."""
    import rag.storage.hip_index as hi
    storage = _storage(storage_dir)
    texts: List[str] = []
    for doc in manifest.documents:
        chunks = hi._load_chunk_list(storage, doc["doc_id"])
        if len(chunks) != doc["rows"]:
            raise ValueError(f"document {doc['doc_id']!r}: its chunk table has {len(chunks)} rows, the collection manifest names "
                             f"{doc['rows']} (rows {doc['row0']}..{doc['row0'] + doc['rows'] - 1})")
        texts.extend(c.get("text", "") for c in chunks)
    return texts


def collection_postings(manifest: CollectionManifest, storage_dir=None):
    """BM25 postings (hiprag.PostingsCSR with its vocabulary) over collection_texts: document id == collection row.  Pure
    host code."""
    from hiprag.sparse import build_postings_from_texts
    return build_postings_from_texts(collection_texts(manifest, storage_dir))


def search_collection_hybrid(query_text: str, query_vector: List[float], limit: int = 50, project: Optional[str] = None,
                             c: float = 60.0, w_dense: float = 1.0, w_sparse: float = 1.0, storage_dir=None,
                             lexical_query=None) -> List[dict]:
    """HybridRetriever._hybrid_search under HIP_COLLECTION: dense top-`limit` and BM25 top-`limit` over the rows of
    scope_for(project) (`project=None`: the whole collection) and their RRF in ONE library call,
    hiphybrid_search_scoped_dev.  Rows in fusion order, each enriched from its own document's chunk table with "doc_id",
    "rrf_score", "bm25_score" (if the sparse leg found it) and "sparse_only" (if only the sparse leg did); "score" is the
    dense similarity after the reader's transform, 0.0 for sparse-only rows (HIP_HYBRID_SCORE_ALL=true: their exact score and
    "dense_scored", _fused_rows).  Unknown project / no collection -> [].
    HIP_COLLECTION_SPARSE=lexical: the sparse leg is the collection's lexical postings searched with `lexical_query` = the
    query's (token ids, weights) inside the same scope -- the composition hybrid_search_scoped_lexical_device on one stream
    in place of the one call -- and every row carries sparse_mode = "lexical" with the lexical score under "bm25_score"."""
    if limit > SCOPED_HYBRID_MAX_TOP_K:
        raise RuntimeError(f"limit={limit} is beyond what a scoped hybrid search returns ({SCOPED_HYBRID_MAX_TOP_K}): "
                           f"hybrid search is on and HIP_COLLECTION is on")
    coll = open_collection(storage_dir)
    if coll is None or coll.manifest.rows == 0:
        logger.warning("No HIP indices found")
        return []
    scope = coll.manifest.scope_for(project)
    if not scope:
        logger.warning(f"No HIP indices found for project {project!r}")
        return []
    import torch
    from hiprag import hybrid_search_ivf_scoped_device, hybrid_search_scoped_device
    from rag.storage.hip_index.sparse import get_collection_sparse
    q = torch.tensor([query_vector], dtype=torch.float32, device=torch.device("cuda", coll.index.device))
    lexical = config.HIP_COLLECTION_SPARSE == "lexical"                # raises on an unknown value or a combination it refuses
    if lexical:
        f_scores, f_ids, ((d_scores, d_ids), (s_scores, s_ids)) = _lexical_hybrid(coll, q, lexical_query, scope, limit, c, w_dense, w_sparse)
        return _fused_rows(coll, query_vector, f_scores[0].tolist(), f_ids[0].tolist(), (d_scores[0].tolist(), d_ids[0].tolist()),
                           (s_scores[0].tolist(), s_ids[0].tolist()), sparse_mode="lexical")
    bm25 = get_collection_sparse(coll)
    nprobe = _ivf_nprobe(coll) if config.HIP_IVF_HYBRID else None       # None: the flat index is the dense leg
    if nprobe is None:
        f_scores, f_ids, ((d_scores, d_ids), (s_scores, s_ids)) = hybrid_search_scoped_device(
            coll.index, bm25, q, [bm25.terms_of(query_text)], [scope], depth=limit, k=limit, c=c, w_dense=w_dense, w_sparse=w_sparse,
            return_lists=True)
    else:
        f_scores, f_ids, ((d_scores, d_ids), (s_scores, s_ids)) = hybrid_search_ivf_scoped_device(
            coll.ivf, bm25, q, [bm25.terms_of(query_text)], [scope], depth=limit, k=limit, c=c, w_dense=w_dense, w_sparse=w_sparse,
            nprobe=nprobe, return_lists=True, **_ivf_probe())
    return _fused_rows(coll, query_vector, f_scores[0].tolist(), f_ids[0].tolist(),          # the copies synchronise
                       (d_scores[0].tolist(), d_ids[0].tolist()), (s_scores[0].tolist(), s_ids[0].tolist()))


def _lexical_hybrid(coll: Collection, q, lexical_query, scope, limit: int, c: float, w_dense: float, w_sparse: float):
    """the scoped lexical composition over the collection's postings: what hybrid_search_scoped_device returns with lists"""
    from hiprag import hybrid_search_scoped_lexical_device
    if coll.lex is None:
        raise RuntimeError("HIP_COLLECTION_SPARSE=lexical, but the collection holds no lexical postings: ingest it under "
                           "HIP_COLLECTION_SPARSE=lexical")
    if lexical_query is None:
        raise RuntimeError("HIP_COLLECTION_SPARSE=lexical needs the query's lexical weights (embed_single_lexical)")
    if coll.lex.n_docs != coll.manifest.rows:
        raise RuntimeError(f"the collection's lexical postings hold {coll.lex.n_docs} documents, its manifest {coll.manifest.rows} rows")
    return hybrid_search_scoped_lexical_device(coll.index, coll.lex, q, [list(lexical_query[0])], [lexical_query[1]], [scope], depth=limit,
                                               k=limit, c=c, w_dense=w_dense, w_sparse=w_sparse, return_lists=True)


def _fused_rows(coll: Collection, query_vector: List[float], f_scores, f_ids, dense, sparse, sparse_mode: Optional[str] = None) -> List[dict]:
    """The enriched rows of one query's fused list (host lists; dense / sparse = that leg's (scores, ids)), in fusion order.
    HIP_HYBRID_SCORE_ALL=true: ONE coll.index.score_ids call gives the rows the dense list lacks their exact fp64 score --
    from the flat index also when the IVF companion was the dense leg, which is why the collection keeps the flat index --
    and they carry the reader's transform of it as "score" and "dense_scored" where they would carry 0.0 and "sparse_only"."""
    dense_score = dict(_transform(coll, *dense))
    bm25_of = {int(i): float(s) for i, s in zip(sparse[1], sparse[0]) if i >= 0}
    rescored: Dict[int, float] = {}
    if config.HIP_HYBRID_SCORE_ALL:
        missing = [int(row) for row in f_ids if row >= 0 and row not in dense_score]
        if missing:
            values = coll.index.score_ids(np.array([query_vector], dtype=np.float32), np.array([missing], dtype=np.int64),
                                          return64=True)
            rescored = dict(_transform(coll, values[0].tolist(), missing))
    fused = []
    for row, fs in zip(f_ids, f_scores):
        if row < 0:
            continue
        for item in _enrich(coll, [(row, dense_score.get(row, rescored.get(row, 0.0)))]):
            item["rrf_score"] = float(fs)
            if sparse_mode is not None:
                item["sparse_mode"] = sparse_mode    # which sparse leg bm25_score comes from
            if row in bm25_of:
                item["bm25_score"] = bm25_of[row]
            if row in rescored:
                item["dense_scored"] = True      # scored by id, not found by the dense leg
            elif row not in dense_score:
                item["sparse_only"] = True       # no dense similarity: rank_pages keeps it out of the page mean
            fused.append(item)
    return fused


def search_collection_device(query_vector: List[float], limit: int = 50, project: Optional[str] = None,
                             query_text: Optional[str] = None, c: float = 60.0, w_dense: float = 1.0, w_sparse: float = 1.0,
                             storage_dir=None, lexical_query=None) -> Optional[Dict[str, Any]]:
    """search_collection (`query_text=None`) or search_collection_hybrid (a query text) with the results LEFT ON THE DEVICE,
    for the page-ranking call: the same library calls with the same arguments, so the lists hold what the host forms read
    back; nothing is copied or synchronised.  -> {"coll", "cand_ids" int64 [1, limit] (the result list: dense order, or
    fusion order), "dense_ids" int64 / "dense_scores" [1, limit] (the dense list: the same list with its float32 scores, or
    the dense leg with its float64 ones -- what the host form of each transforms),
    and for the hybrid form "fused_scores", "sparse_ids", "sparse_scores" and "query" (the float32 [1, d] query tensor)}, CUDA tensors; None where the host forms return
    [] (no collection, no rows, unknown project)."""
    import torch
    hybrid = query_text is not None
    if hybrid and limit > SCOPED_HYBRID_MAX_TOP_K:
        raise RuntimeError(f"limit={limit} is beyond what a scoped hybrid search returns ({SCOPED_HYBRID_MAX_TOP_K}): "
                           f"hybrid search is on and HIP_COLLECTION is on")
    coll = open_collection(storage_dir)
    if coll is None or coll.manifest.rows == 0:
        logger.warning("No HIP indices found")
        return None
    q = torch.tensor([query_vector], dtype=torch.float32, device=torch.device("cuda", coll.index.device))
    if hybrid:
        scope = coll.manifest.scope_for(project)
        if not scope:
            logger.warning(f"No HIP indices found for project {project!r}")
            return None
        from hiprag import hybrid_search_ivf_scoped_device, hybrid_search_scoped_device
        from rag.storage.hip_index.sparse import get_collection_sparse
        if config.HIP_COLLECTION_SPARSE == "lexical":                       # the lexical composition, as search_collection_hybrid
            f_scores, f_ids, ((d_scores, d_ids), (s_scores, s_ids)) = _lexical_hybrid(coll, q, lexical_query, scope, limit, c, w_dense, w_sparse)
            return {"coll": coll, "cand_ids": f_ids, "dense_ids": d_ids, "dense_scores": d_scores, "fused_scores": f_scores,
                    "sparse_ids": s_ids, "sparse_scores": s_scores, "query": q, "sparse_mode": "lexical"}
        bm25 = get_collection_sparse(coll)
        nprobe = _ivf_nprobe(coll) if config.HIP_IVF_HYBRID else None       # None: the flat index is the dense leg
        if nprobe is None:
            f_scores, f_ids, ((d_scores, d_ids), (s_scores, s_ids)) = hybrid_search_scoped_device(
                coll.index, bm25, q, [bm25.terms_of(query_text)], [scope], depth=limit, k=limit, c=c, w_dense=w_dense, w_sparse=w_sparse,
                return_lists=True)
        else:
            f_scores, f_ids, ((d_scores, d_ids), (s_scores, s_ids)) = hybrid_search_ivf_scoped_device(
                coll.ivf, bm25, q, [bm25.terms_of(query_text)], [scope], depth=limit, k=limit, c=c, w_dense=w_dense, w_sparse=w_sparse,
                nprobe=nprobe, return_lists=True, **_ivf_probe())
        return {"coll": coll, "cand_ids": f_ids, "dense_ids": d_ids, "dense_scores": d_scores, "fused_scores": f_scores,
                "sparse_ids": s_ids, "sparse_scores": s_scores, "query": q}
    nprobe = _ivf_nprobe(coll)                  # None: the flat index answers
    if project is None:
        _, values, ids = coll.index.search_device(q, limit) if nprobe is None else coll.ivf.search_device(q, limit, nprobe)
    else:
        _check_limit(limit)
        scope = coll.manifest.scope_for(project)
        if not scope:
            logger.warning(f"No HIP indices found for project {project!r}")
            return None
        if nprobe is None:
            _, values, ids = coll.index.search_scoped_device(q, limit, [scope])
        else:
            _, values, ids = coll.ivf.search_scoped_device(q, limit, [scope], nprobe=nprobe, **_ivf_probe())
    return {"coll": coll, "cand_ids": ids, "dense_ids": ids, "dense_scores": values}


def clear_collection_cache() -> None:
    with _LOCK:
        _COLLECTION_CACHE.clear()


__all__ = ["Collection", "CollectionManifest", "COLLECTION_INDEX", "COLLECTION_MANIFEST", "append_document", "delete_document",
           "replace_document", "open_collection", "open_or_create_collection",
           "rebuild_collection", "search_collection", "search_collection_batch", "search_collection_hybrid", "search_collection_device", "collection_postings", "collection_texts",
           "clear_collection_cache", "read_flat_rows", "train_collection_ivf", "train_collection_centroids", "COLLECTION_MVC", "COLLECTION_IVF", "COLLECTION_MV",
           "COLLECTION_LEXICAL"]
