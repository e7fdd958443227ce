"""hiprag -- Python host side of libhiprag.so (MI355X hybrid-retrieval hot path).  No CPU fallbacks."""
from . import _native
from ._native import METRIC_IP, METRIC_L2, HipRagError, LIB_PATH  # noqa: F401
from .index import HipFlatIndex, merge_topk_device, pack_scopes, score_ids_reference  # noqa: F401
from .ivf import HipIVFIndex  # noqa: F401
from .sparse import (HipBM25, HipBM25Updatable, PostingsCSR, batch_csr, build_postings, build_postings_from_texts,  # noqa: F401
                     bm25_score_ids_reference, tokenize, weighted_search_reference)
from .fusion import (hybrid_search, hybrid_search_device, hybrid_search_scoped, hybrid_search_scoped_device,  # noqa: F401
                     hybrid_search_ivf_scoped, hybrid_search_ivf_scoped_device, rrf_fuse, rrf_fuse_device, RRF_C)
from .encoder import EncoderConfig, HipEncoder, random_state  # noqa: F401
from .rerank import TokenStore, pair_tokens, rerank, rerank_device  # noqa: F401
from .lexical import (LexicalIndex, LexicalIndexUpdatable, hybrid_search_lexical_device,  # noqa: F401
                      hybrid_search_scoped_lexical_device, lexical_reference, lexical_token_weights, transpose_doc_weights)
from .pages import PageTable, rank_pages_device, rank_pages_reference  # noqa: F401
from .colbert import (MultiVectorStore, colbert_reference, fp8_dequantize, fp8_quantize_reference, maxsim, maxsim_device,  # noqa: F401
                      maxsim_reference, maxsim_search, maxsim_search_device, maxsim_search_reference,
                      mxfp4_dequantize, mxfp4_quantize_reference, centroid_codes_reference, centroid_interaction_reference,
                      maxsim_search_pruned, maxsim_search_pruned_device, train_token_centroids)
from .m3 import M3_WEIGHTS, m3_score, m3_score_device, m3_score_reference  # noqa: F401


def init(n_devices: int = 0) -> None:
    """hiprag_init: check that `n_devices` GPUs are visible (0 = at least one) and create their contexts now."""
    _native.call("hiprag_init", int(n_devices))


def shutdown() -> None:
    """hiprag_shutdown: synchronise every device and drop every library handle still alive.  Python objects that wrap a
    handle must not be used afterwards (their close() then reports an unknown handle)."""
    _native.call("hiprag_shutdown")
    from . import sharded
    sharded._SCAN_STREAMS.clear()      # wrappers of the library's scan and tail streams, destroyed with it
    sharded._TAIL_STREAMS.clear()
