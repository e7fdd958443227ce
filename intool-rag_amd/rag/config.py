"""
The handful of settings the hot path reads, under the SAME environment names as the reference's rag/config.py
(:9-11, :25-30, :41-45, :53-62) so an existing deployment's .env keeps working.  Unlike the reference this module
has no import-time side effects (the reference mkdirs at import, config.py:50,63,66).
"""
import math
import os
from pathlib import Path


class Config:
    EMBEDDING_MODEL = os.getenv("EMBEDDING_MODEL", "BAAI/bge-m3")
    EMBEDDING_BATCH_SIZE = int(os.getenv("EMBEDDING_BATCH_SIZE", "8"))
    VECTOR_DIMENSION = int(os.getenv("VECTOR_DIMENSION", "1024"))
    RERANKER_MODEL = os.getenv("RERANKER_MODEL", "BAAI/bge-reranker-v2-m3")
    RERANKER_ENABLED = os.getenv("RERANKER_ENABLED", "true").lower() == "true"
    RERANKER_TOP_K = int(os.getenv("RERANKER_TOP_K", "10"))
    RETRIEVAL_TOP_K = int(os.getenv("RETRIEVAL_TOP_K", "10"))
    RETRIEVAL_MIN_SCORE = float(os.getenv("RETRIEVAL_MIN_SCORE", "0.3"))
    HYBRID_SEARCH_ENABLED = os.getenv("HYBRID_SEARCH_ENABLED", "true").lower() == "true"
    BM25_WEIGHT = float(os.getenv("BM25_WEIGHT", "0.3"))
    VECTOR_WEIGHT = float(os.getenv("VECTOR_WEIGHT", "0.7"))
    EMBEDDING_QUERY_INSTRUCTION = os.getenv("EMBEDDING_QUERY_INSTRUCTION",
                                            "Represent this sentence for searching relevant passages: ")
    # additions of this build
    HIP_INDEX_METRIC = os.getenv("HIP_INDEX_METRIC", "l2")       # the reference builds IndexFlatL2 (faiss_index.py:123)
    HIP_DEVICE = int(os.getenv("HIP_DEVICE", "0"))
    HIP_COMPAT_MINUS_ONE = os.getenv("HIP_COMPAT_MINUS_ONE", "true").lower() == "true"
    # false (default): `instruction` arguments are accepted and ignored, exactly like the reference's HF provider
    # (hf/embeddings.py:45,64-65); true: a given instruction is prepended to each text before tokenisation (BGE recipe)
    HIP_APPLY_INSTRUCTION = os.getenv("HIP_APPLY_INSTRUCTION", "false").lower() == "true"
    EMBEDDING_PASSAGE_INSTRUCTION = os.getenv("EMBEDDING_PASSAGE_INSTRUCTION", "")
    # false (default): search the FIRST index file only, like the reference (faiss_index.py:162-167); true: every document
    HIP_SEARCH_ALL_DOCUMENTS = os.getenv("HIP_SEARCH_ALL_DOCUMENTS", "false").lower() == "true"

    @property
    def STORAGE_DIR(self) -> Path:
        return Path(os.getenv("STORAGE_DIR", "./storages"))

    # Index kind the ingest writes (read when an index is built, like STORAGE_DIR): "flat" (default; exact, HIPIDX01 files) or
    # "ivf" (IVF-Flat, HIPIVF01 files; approximate unless HIP_IVF_NPROBE >= nlist).  Readers tell the two apart by the file,
    # so a storage directory may hold both.
    @property
    def HIP_INDEX_TYPE(self) -> str:
        t = os.getenv("HIP_INDEX_TYPE", "flat").strip().lower()
        if t not in ("flat", "ivf"):
            raise ValueError(f"HIP_INDEX_TYPE={t!r}: expected 'flat' or 'ivf'")
        return t

    @property
    def HIP_IVF_NLIST(self) -> int:
        """lists of an IVF index; 0 (default) = ivf_auto_nlist(n)"""
        return int(os.getenv("HIP_IVF_NLIST", "0"))

    @property
    def HIP_IVF_NPROBE(self) -> int:
        """lists an IVF search probes (clamped to the index's nlist)"""
        return int(os.getenv("HIP_IVF_NPROBE", "16"))

    # Which lists a PROJECT-scoped search of the collection's IVF companion probes (HIP_COLLECTION=true HIP_INDEX_TYPE=ivf):
    # "any" (default) = the HIP_IVF_NPROBE best lists whatever the project (faiss's IDSelector behaviour); "scope" = the
    # HIP_IVF_NPROBE best lists among those that hold a row of the project (hipivf_search_scoped_probe).  Read at use.
    @property
    def HIP_IVF_PROBE(self) -> str:
        t = os.getenv("HIP_IVF_PROBE", "any").strip().lower()
        if t not in ("any", "scope"):
            raise ValueError(f"HIP_IVF_PROBE={t!r}: expected 'any' or 'scope'")
        return t

    # false (default): the collection's hybrid search runs its dense leg on the flat index (exact).  true: with
    # HIP_INDEX_TYPE=ivf and an IVF companion, the dense leg is the companion's scoped search (hiphybrid_search_ivf_scoped).
    @property
    def HIP_IVF_HYBRID(self) -> bool:
        return os.getenv("HIP_IVF_HYBRID", "false").strip().lower() == "true"

    # false (default): a fused chunk that only the BM25 leg found (or, under HIP_IVF_HYBRID, one outside the probed lists) has
    # score 0.0 and metadata["sparse_only"], and stays out of its page's mean.  true: the hybrid paths score such chunks
    # exactly with hipidx_score_ids (HipFlatIndex.score_ids, always on the flat index), so every chunk carries a similarity as
    # in the reference (page_retriever.py:191); those chunks carry metadata["dense_scored"] instead.  Read at use.
    @property
    def HIP_HYBRID_SCORE_ALL(self) -> bool:
        return os.getenv("HIP_HYBRID_SCORE_ALL", "false").strip().lower() == "true"

    # false (default): per-document index files only and `project` ignored, like the reference.  true: the ingest also appends
    # every document to ONE collection index (hip_collection.index / .json) and search_hip_by_vector searches that, scoped to
    # the documents of `project` when one is given (rag/storage/hip_index/collection.py).  Read at use.
    @property
    def HIP_COLLECTION(self) -> bool:
        return os.getenv("HIP_COLLECTION", "false").strip().lower() == "true"

    # Sparse leg of the per-document hybrid search: "bm25" (default; whitespace-token BM25 over the chunk texts, as ever) or
    # "lexical" (BGE-M3's lexical weights: the ingest keeps each chunk's token weights from the forward that made its embedding
    # in {doc_id}_hip.lexical.npz, and a query is scored with its own token weights, hiprag.lexical).  The provider then needs
    # HIP_SPARSE_LINEAR = the model's sparse_linear.pt (or a safetensors file with `weight` / `bias`).  This setting governs the
    # per-document path only: with HIP_COLLECTION=true the combination raises, and the collection's sparse leg is chosen by
    # HIP_COLLECTION_SPARSE below.  Read at use.
    @property
    def HIP_SPARSE_MODE(self) -> str:
        t = os.getenv("HIP_SPARSE_MODE", "bm25").strip().lower()
        if t not in ("bm25", "lexical"):
            raise ValueError(f"HIP_SPARSE_MODE={t!r}: expected 'bm25' or 'lexical'")
        if t == "lexical" and self.HIP_COLLECTION:
            raise ValueError("HIP_SPARSE_MODE=lexical with HIP_COLLECTION=true is not supported yet: HIP_SPARSE_MODE governs the "
                             "per-document path; set HIP_COLLECTION_SPARSE=lexical for the collection's sparse leg")
        return t

    # Sparse leg of the COLLECTION's hybrid search (HIP_COLLECTION=true): "bm25" (default; nothing changes) or "lexical": the
    # ingest passes each chunk's lexical weights, from the forward that makes its embedding, to the collection, which keeps
    # them as updatable impact postings on the device (hipbm25_append_rows_dev / hipbm25_remove_ranges, saved as
    # hip_collection.lexical.npz), and a query is scored with its own token weights inside its project's row ranges.  Needs
    # the hip embedding provider with HIP_SPARSE_LINEAR (or HIP_ALLOW_SYNTHETIC).  Without HIP_M3_SCORE=true one forward gives
    # one extra output, so it raises together with HIP_LATE_INTERACTION=true (HIP_M3_SCORE below lifts that: its ingest runs the
    # combined forward); the IVF hybrid has no weighted form, so it raises with HIP_IVF_HYBRID=true; and without HIP_COLLECTION
    # there is no collection to keep the postings.  Read at use.
    @property
    def HIP_COLLECTION_SPARSE(self) -> str:
        t = os.getenv("HIP_COLLECTION_SPARSE", "bm25").strip().lower()
        if t not in ("bm25", "lexical"):
            raise ValueError(f"HIP_COLLECTION_SPARSE={t!r}: expected 'bm25' or 'lexical'")
        if t == "lexical":
            if not self.HIP_COLLECTION:
                raise ValueError("HIP_COLLECTION_SPARSE=lexical needs HIP_COLLECTION=true: the lexical postings follow the collection's rows")
            if os.getenv("HIP_LATE_INTERACTION", "false").strip().lower() == "true" and not _env_true("HIP_M3_SCORE"):
                raise ValueError("HIP_COLLECTION_SPARSE=lexical with HIP_LATE_INTERACTION=true is not supported: one forward gives one "
                                 "extra output today (a combined lexical + ColBERT forward is a follow-up)")
            if self.HIP_IVF_HYBRID:
                raise ValueError("HIP_COLLECTION_SPARSE=lexical with HIP_IVF_HYBRID=true is not supported: the IVF hybrid has no "
                                 "weighted sparse leg")
        return t

    # false (default): the retriever never reranks, whatever RERANKER_ENABLED says (the reference sets it and reads it
    # nowhere).  true: HybridRetriever(rerank=None) reranks its top_chunks with the cross-encoder when RERANKER_ENABLED is
    # true as well and passes the first RERANKER_TOP_K on.  Off by default on purpose: a deployment without reranker
    # weights would raise RerankerError on every query.  Read at use.
    @property
    def HIP_RERANK(self) -> bool:
        return os.getenv("HIP_RERANK", "false").strip().lower() == "true"

    # false (default): the encoder runs padded batches (length-sorted where the host can sort).  true: the hip embedding
    # provider's embed_batch / embed_single, CrossEncoderReranker.score and the collection's device rerank (HIP_RERANK=true)
    # use the encoder's PACKED entries (hipenc_forward_packed, hipenc_score_pairs_packed, hiprerank_packed_dev): every sequence
    # costs its own length rounded up to 64 rows, not its batch's -- or, in the device rerank, the store's -- longest.  The
    # packed device rerank synchronises its stream once per call.  The lexical and ColBERT paths stay padded.  Read at use.
    @property
    def HIP_ENCODER_PACKED(self) -> bool:
        return os.getenv("HIP_ENCODER_PACKED", "false").strip().lower() == "true"

    # false (default): pages are grouped and ranked on the host from the enriched chunk list, as the reference does
    # (page_retriever.py:145-236).  true, with HIP_COLLECTION=true: HybridRetriever.retrieve_and_rank_pages keeps the
    # search results on the device, ranks the pages there (hippage_rank_dev over the collection's page table,
    # rag/storage/hip_index/pages.py) and enriches only the chunks of the selected pages; pages are keyed by (document,
    # page).  Read at use.
    @property
    def HIP_PAGES(self) -> bool:
        return os.getenv("HIP_PAGES", "false").strip().lower() == "true"

    # false (default): nothing changes.  true, with HIP_COLLECTION=true and the hip embedding provider: the ingest keeps every
    # chunk's per-token (ColBERT) vectors, BGE-M3's third output, from the forward that makes its embedding, in the
    # collection's multi-vector store (hip_collection.mv, rag/storage/hip_index/collection.py), and the retriever reorders its
    # top chunks by late interaction (MaxSim, hipmaxsim_dev) and keeps RERANKER_TOP_K of them.  The provider then needs
    # HIP_COLBERT_LINEAR = the model's colbert_linear.pt (or a safetensors file with `weight` [H, H] / `bias` [H]).  It is a
    # second stage like the cross-encoder: with HIP_RERANK=true as well the combination raises -- it asks for two.  Without
    # HIP_COLLECTION it raises too: the vectors live beside the collection's rows.  Read at use.
    @property
    def HIP_LATE_INTERACTION(self) -> bool:
        on = os.getenv("HIP_LATE_INTERACTION", "false").strip().lower() == "true"
        if on and not self.HIP_COLLECTION:
            raise ValueError("HIP_LATE_INTERACTION=true needs HIP_COLLECTION=true: the per-token vectors are kept beside the "
                             "collection's rows")
        if on and self.HIP_RERANK:
            raise ValueError("HIP_LATE_INTERACTION=true with HIP_RERANK=true asks for two second stages: choose the cross-encoder "
                             "or late interaction")
        return on

    # false (default): nothing changes.  true, with HIP_LATE_INTERACTION=true: late interaction is the FIRST stage -- the
    # retriever ranks every chunk of the project by MaxSim over the collection's multi-vector store (hipmaxsim_search_scoped_dev,
    # the `project` of rag/storage/faiss_index.py:140 honoured for the sixth structure) instead of re-ordering what the dense
    # search found; a chunk's `score` is still its exact dense similarity (score_ids).  Without HIP_LATE_INTERACTION=true it
    # raises (which in turn needs HIP_COLLECTION=true and refuses HIP_RERANK); a retriever with hybrid=True raises too: fusing
    # MaxSim with RRF is out of scope.  Read at use.
    @property
    def HIP_LATE_SEARCH(self) -> bool:
        on = os.getenv("HIP_LATE_SEARCH", "false").strip().lower() == "true"
        if on and os.getenv("HIP_LATE_INTERACTION", "false").strip().lower() != "true":
            raise ValueError("HIP_LATE_SEARCH=true needs HIP_LATE_INTERACTION=true: it searches the per-token vectors that setting keeps")
        if on:
            self.HIP_LATE_INTERACTION        # raises without HIP_COLLECTION=true or with HIP_RERANK=true
        return on

    # 0 (default): nothing changes.  1..256, with HIP_LATE_SEARCH=true: the late-interaction search generates candidates first
    # -- every chunk of the project is scored from the centroid codes of its token vectors, and only the best
    # max(limit, HIP_LATE_CANDIDATES) chunks reach the exact MaxSim (hipmaxsim_search_pruned_dev).  The collection needs
    # centroids (train_collection_centroids).  Without HIP_LATE_SEARCH=true it raises; so does a value outside 0..256.  Read
    # at use.
    @property
    def HIP_LATE_CANDIDATES(self) -> int:
        raw = os.getenv("HIP_LATE_CANDIDATES", "0").strip()
        try:
            n = int(raw)
        except ValueError:
            raise ValueError(f"HIP_LATE_CANDIDATES={raw!r}: expected an integer in 0..256")
        if not 0 <= n <= 256:
            raise ValueError(f"HIP_LATE_CANDIDATES={n}: expected 0 (off) or 1..256")
        if n and not _env_true("HIP_LATE_SEARCH"):
            raise ValueError("HIP_LATE_CANDIDATES needs HIP_LATE_SEARCH=true: it prunes the late-interaction search")
        if n:
            self.HIP_LATE_SEARCH             # raises without HIP_LATE_INTERACTION=true and what that needs
        return n

    # The storage format of the collection's multi-vector store (HIP_LATE_INTERACTION=true): "bf16" (default; nothing changes,
    # 2 x dim bytes per stored token) or "fp8": OCP e4m3fn codes with one power-of-two scale per vector, dim + 4 bytes per
    # token -- 1 M passages of 120 tokens at 1024-d take 123 GB instead of 245 GB -- quantised on the device as the vectors are
    # appended; or "mxfp4": OCP microscaling FP4, e2m1 codes with one e8m0 scale per 32 components, dim / 2 + dim / 32 bytes
    # per token (544 at 1024-d: 65 GB for the same collection).  MaxSim over either is, bit for bit, MaxSim over the
    # dequantised vectors.  It applies when a collection's store is CREATED; an existing collection keeps its format whatever
    # this says (Collection.convert_multivectors("fp8") or ("mxfp4") converts a bf16 one).  Any other value raises.  Read at use.
    @property
    def HIP_COLBERT_FORMAT(self) -> str:
        t = os.getenv("HIP_COLBERT_FORMAT", "bf16").strip().lower()
        if t not in ("bf16", "fp8", "mxfp4"):
            raise ValueError(f"HIP_COLBERT_FORMAT={t!r}: expected 'bf16', 'fp8' or 'mxfp4'")
        return t

    # false (default): nothing changes.  true: BGE-M3's own ranking -- the weighted sum of the dense, lexical and ColBERT scores
    # (FlagEmbedding's compute_score "dense + sparse + colbert").  It needs HIP_COLLECTION=true, HIP_COLLECTION_SPARSE=lexical
    # and HIP_LATE_INTERACTION=true, and with it set (and only then) those two stop refusing each other: the ingest runs ONE
    # forward per batch for all three outputs (hipenc_forward_m3), the retriever embeds the query once the same way, runs the
    # first stage it would run anyway and reorders its top chunks by hipm3_score, keeping RERANKER_TOP_K.  It is a second stage:
    # it raises with HIP_RERANK=true and HIP_LATE_SEARCH=true, and with HIP_PAGES=true (the device page path is out of scope
    # for the combined score).  Read at use.
    @property
    def HIP_M3_SCORE(self) -> bool:
        on = _env_true("HIP_M3_SCORE")
        if not on:
            return False
        if not self.HIP_COLLECTION:
            raise ValueError("HIP_M3_SCORE=true needs HIP_COLLECTION=true: the three structures it scores follow the collection's rows")
        if os.getenv("HIP_COLLECTION_SPARSE", "bm25").strip().lower() != "lexical":
            raise ValueError("HIP_M3_SCORE=true needs HIP_COLLECTION_SPARSE=lexical: its sparse term is BGE-M3's lexical score")
        if not _env_true("HIP_LATE_INTERACTION"):
            raise ValueError("HIP_M3_SCORE=true needs HIP_LATE_INTERACTION=true: its ColBERT term reads the collection's multi-vector store")
        if self.HIP_RERANK:
            raise ValueError("HIP_M3_SCORE=true with HIP_RERANK=true asks for two second stages: choose the cross-encoder or the "
                             "combined score")
        if _env_true("HIP_LATE_SEARCH"):
            raise ValueError("HIP_M3_SCORE=true with HIP_LATE_SEARCH=true is not supported: the combined score reorders the "
                             "candidates of a dense or hybrid first stage")
        if self.HIP_PAGES:
            raise ValueError("HIP_M3_SCORE=true with HIP_PAGES=true is not supported: the device page path is out of scope for the "
                             "combined score")
        self.HIP_COLLECTION_SPARSE       # its other refusals (HIP_IVF_HYBRID)
        self.HIP_M3_WEIGHTS              # a malformed mix fails here, not at the first query
        return True

    # The mix of HIP_M3_SCORE: "dense,sparse,colbert" weights, default BGE-M3's published 0.4,0.2,0.4.  Three finite numbers
    # >= 0, at least one > 0; a weight of 0 drops its leg from the score (it is not run).  Anything else raises.  Read at use.
    @property
    def HIP_M3_WEIGHTS(self):
        return parse_m3_weights(os.getenv("HIP_M3_WEIGHTS", "0.4,0.2,0.4"))


def _env_true(name: str) -> bool:
    return os.getenv(name, "false").strip().lower() == "true"


def parse_m3_weights(text: str):
    """"d,s,c" -> (dense, sparse, colbert) floats: exactly three, finite, >= 0, at least one > 0."""
    parts = [p.strip() for p in str(text).split(",")]
    try:
        w = tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError(f"HIP_M3_WEIGHTS={text!r}: expected three numbers 'dense,sparse,colbert'") from None
    if len(w) != 3:
        raise ValueError(f"HIP_M3_WEIGHTS={text!r}: expected three numbers 'dense,sparse,colbert' (got {len(w)})")
    if not all(math.isfinite(x) and x >= 0 for x in w):
        raise ValueError(f"HIP_M3_WEIGHTS={text!r}: every weight must be finite and >= 0")
    if not any(x > 0 for x in w):
        raise ValueError(f"HIP_M3_WEIGHTS={text!r}: at least one weight must be > 0")
    return w


def ivf_auto_nlist(n: int) -> int:
    """max(1, min(n // 39, 4 * ceil(sqrt(n)))): at least 39 rows per centroid (FAISS's min_points_per_centroid, below which
    k-means warns) and at most 4 sqrt(n) lists (FAISS's guidance for IVF sizes)."""
    n = int(n)
    root = math.isqrt(n)
    if root * root < n:
        root += 1
    return max(1, min(n // 39, 4 * root))


config = Config()
