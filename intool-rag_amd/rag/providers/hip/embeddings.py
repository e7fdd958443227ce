"""
rag/providers/hip/embeddings.py -- MI355X embedding provider behind the reference's EmbeddingProvider ABC
(rag/llm/embeddings/base.py:5-17), selected with EMBEDDING_PROVIDER=hip.

Behaviour mirrors HuggingFaceEmbeddingProvider (rag/providers/hf/embeddings.py:13-91) call for call:
  * embed_single: strip; empty / blank -> [0.0] * dim (:47-48); else encode in a worker thread (asyncio.to_thread, :53)
  * embed_batch : [] -> []; per-text strip, None / blank -> "" which IS encoded (:70-73); one batched encode (:76);
                  `instruction` and `batch_size` accepted and ignored exactly like the reference (:45, :64-65);
                  HIP_APPLY_INSTRUCTION=true prepends a given instruction instead (rag/config.py:53-60 defines them)
  * LangChain's HuggingFaceEmbeddings replaces "\\n" by " " before encoding and asks sentence-transformers for
    normalize_embeddings=True (:34): CLS pooling + L2 normalisation happen on the GPU (csrc/encoder.hip pool_kernel)
  * dimension(): the model width (the reference probes it with a dummy encode, :37-38)

Weights: HIP_ENCODER_WEIGHTS = path to a local safetensors file with XLM-R parameter names (BAAI/bge-m3 layout) and
HIP_TOKENIZER_FILE = the model's tokenizer.json.  Without them the constructor RAISES, like the reference does when its
model cannot be loaded (:26-29, :39-40).  HIP_ALLOW_SYNTHETIC=1 opts in to SEEDED RANDOM weights of the configured
architecture and the hashing tokenizer (tests and benches: there is no checkpoint in an offline image; the GPU code
path, shapes and cost are identical, the vectors are meaningless).

HIP_SPARSE_MODE=lexical or HIP_COLLECTION_SPARSE=lexical: the encoder also carries BGE-M3's lexical head.
HIP_SPARSE_LINEAR = the model's sparse_linear.pt
(a torch-saved dict) or a safetensors file, either with `weight` [1, H] and `bias` [1]; without it HIP_ALLOW_SYNTHETIC gives a
seeded head, otherwise the constructor raises.  embed_batch_lexical_device / embed_single_lexical then give the vectors AND
the per-text lexical weights from ONE forward (hipenc_forward_lexical); sequences are capped at the encoder's max_seq_len
(512), far inside the head's 2048 positions.

HIP_LATE_INTERACTION=true: the encoder carries BGE-M3's ColBERT head as well, set at the first use.  HIP_COLBERT_LINEAR = the
model's colbert_linear.pt or a safetensors file, either with `weight` [H, H] and `bias` [H]; without it HIP_ALLOW_SYNTHETIC gives
a seeded head, otherwise that first call raises.  embed_batch_colbert_device / embed_single_colbert give the vectors AND the
per-token unit vectors from ONE forward (hipenc_forward_colbert).
"""
from __future__ import annotations

import asyncio
import json
import os
import threading
from typing import List, Optional

from rag.config import config
from rag.llm.embeddings.base import EmbeddingProvider
from rag.logging import logger
from rag.providers.hip.tokenizer import allow_synthetic, load_tokenizer

try:
    from hiprag import EncoderConfig, HipEncoder
    HAS_HIP = True
    _ERR: Optional[Exception] = None
except Exception as _e:
    HAS_HIP = False
    _ERR = _e


# One forward takes up to this many padded tokens (the BASELINE config-5 batch, 256 x 512): batches are cut by token count,
# not by sequence count, so that short chunks fill the GPU as well as long ones (sentence-transformers' 32 sequences of
# ~128 tokens are a twentieth of it).  EMBEDDING_BATCH_SIZE is accepted and ignored like in the reference (:64-65).
_MAX_BATCH_TOKENS = int(os.getenv("HIP_ENCODER_BATCH_TOKENS", str(256 * 512)))
_MAX_BATCH_SEQS = 4096


UNK_ID = 3       # <unk> of the XLM-R vocabulary; with bos, pad and eos the ids BGE-M3 gives no lexical weight


def _load_sparse_linear(path: str):
    """(weight, bias) tensors from BGE-M3's sparse_linear.pt or a safetensors file with the same two names."""
    if not os.path.exists(path):
        raise RuntimeError(f"HIP_SPARSE_LINEAR={path!r} does not exist")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        state = load_file(path)
    else:
        import torch
        state = torch.load(path, map_location="cpu", weights_only=True)
    if "weight" not in state or "bias" not in state:
        raise RuntimeError(f"HIP_SPARSE_LINEAR={path!r} holds no `weight` / `bias`")
    return state["weight"], state["bias"]


def _encoder_config() -> "EncoderConfig":
    cfg = EncoderConfig()                                  # XLM-R large = BAAI/bge-m3 (config.EMBEDDING_MODEL)
    override = os.getenv("HIP_ENCODER_CONFIG")             # JSON, e.g. {"layers": 2, "hidden": 256, ...} for tests
    if override:
        for k, v in json.loads(override).items():
            setattr(cfg, k, v)
    return cfg


class HipEmbeddingProvider(EmbeddingProvider):
    def __init__(self, model_name: Optional[str] = None, encoder: Optional["HipEncoder"] = None, tokenizer=None):
        if not HAS_HIP:
            raise RuntimeError(f"libhiprag not available: {_ERR}")
        self.model_name = model_name or config.EMBEDDING_MODEL
        if encoder is None:
            cfg = _encoder_config()
            weights = os.getenv("HIP_ENCODER_WEIGHTS")
            state = None
            if weights:
                from safetensors.torch import load_file
                state = load_file(weights)
            elif not allow_synthetic():
                raise RuntimeError("HIP_ENCODER_WEIGHTS is not set: the hip embedding provider needs a local safetensors "
                                   f"file of {self.model_name} (set HIP_ALLOW_SYNTHETIC=1 to run on seeded random weights)")
            else:
                logger.warning("[EMBED] HIP_ALLOW_SYNTHETIC: seeded RANDOM weights of the "
                               f"{self.model_name} architecture -- embeddings carry no meaning")
            if tokenizer is None:
                tokenizer = load_tokenizer(cfg.vocab)      # raises before any GPU memory is taken
            encoder = HipEncoder(cfg, state, device=config.HIP_DEVICE, seed=0)
        self.encoder = encoder
        self.tokenizer = tokenizer or load_tokenizer(encoder.cfg.vocab)
        self._dimension = encoder.dimension
        self._lock = threading.Lock()      # to_thread workers share one encoder workspace
        # the per-document sparse leg (HIP_SPARSE_MODE) or the collection's (HIP_COLLECTION_SPARSE) is lexical
        if (config.HIP_SPARSE_MODE == "lexical" or config.HIP_COLLECTION_SPARSE == "lexical") and not encoder.has_lexical:
            self._set_lexical_head()
        logger.info(f"[EMBED] ✓ HIP ready (model={self.model_name}, dim={self._dimension})")

    def _set_lexical_head(self) -> None:
        cfg = self.encoder.cfg
        path = os.getenv("HIP_SPARSE_LINEAR")
        if path:
            weight, bias = _load_sparse_linear(path)
        elif allow_synthetic():
            import torch
            logger.warning("[EMBED] HIP_ALLOW_SYNTHETIC: a seeded RANDOM lexical head -- lexical weights carry no meaning")
            g = torch.Generator().manual_seed(1)
            weight, bias = torch.randn(cfg.hidden, generator=g) * 0.02, torch.randn(1, generator=g) * 0.02
        else:
            raise RuntimeError("HIP_SPARSE_MODE=lexical but HIP_SPARSE_LINEAR is not set: the lexical head needs the model's "
                               "sparse_linear.pt (set HIP_ALLOW_SYNTHETIC=1 to run on a seeded random head)")
        self.encoder.set_lexical_head(weight, bias, (cfg.bos_id, cfg.pad_id, cfg.eos_id, UNK_ID))

    def _encode_lexical(self, clean_texts: List[str]):
        if not self.encoder.has_lexical:
            raise RuntimeError("this provider was made without a lexical head (HIP_SPARSE_MODE=lexical or HIP_COLLECTION_SPARSE=lexical "
                               "at construction)")
        toks = [self.tokenizer.encode(t.replace("\n", " "), self.encoder.cfg.max_seq_len) for t in clean_texts]
        with self._lock:
            return self.encoder.encode_lexical(toks, batch_size=_MAX_BATCH_SEQS, max_tokens=_MAX_BATCH_TOKENS)

    async def embed_batch_lexical_device(self, texts: List[str]):
        """embed_batch_device plus the lexical weights of every text, from ONE forward: (vectors float32 [n, dim],
        terms int32 [n, L], weights float32 [n, L], counts int32 [n]) as CUDA tensors; row i holds counts[i] (token id,
        weight) pairs, ids ascending.  Same text cleaning as embed_batch."""
        if not texts:
            raise ValueError("embed_batch_lexical_device needs at least one text")
        clean_texts = [t.strip() if t and t.strip() else "" for t in texts]
        return await asyncio.to_thread(self._encode_lexical, clean_texts)

    async def embed_single_lexical(self, text: str, instruction: Optional[str] = None):
        """embed_single plus the query's lexical weights from the same forward: (vector as a list of floats, token ids as a
        list, weights as a float32 numpy array).  A blank text gives the zero vector and no terms, like embed_single."""
        import numpy as np
        if not text or not text.strip():
            return [0.0] * self._dimension, [], np.zeros(0, np.float32)
        clean_text = text.strip()
        if instruction and config.HIP_APPLY_INSTRUCTION:
            clean_text = instruction + clean_text
        dense, terms, weights, counts = await asyncio.to_thread(self._encode_lexical, [clean_text])
        n = int(counts[0])
        return dense[0].cpu().tolist(), terms[0, :n].cpu().tolist(), weights[0, :n].cpu().numpy()

    def _ensure_colbert_head(self) -> None:
        """BGE-M3's colbert_linear on the encoder, set at the first use: HIP_COLBERT_LINEAR (the model's colbert_linear.pt, or a
        safetensors file with `weight` [H, H] and `bias` [H]); without it HIP_ALLOW_SYNTHETIC gives a seeded head."""
        if self.encoder.has_colbert:
            return
        cfg = self.encoder.cfg
        path = os.getenv("HIP_COLBERT_LINEAR")
        if path:
            weight, bias = _load_sparse_linear(path)      # the same two names in the same two file kinds
        elif allow_synthetic():
            import torch
            logger.warning("[EMBED] HIP_ALLOW_SYNTHETIC: a seeded RANDOM ColBERT head -- late-interaction scores carry no meaning")
            g = torch.Generator().manual_seed(2)
            weight, bias = torch.randn(cfg.hidden, cfg.hidden, generator=g) * 0.02, torch.randn(cfg.hidden, generator=g) * 0.02
        else:
            raise RuntimeError("HIP_LATE_INTERACTION=true but HIP_COLBERT_LINEAR is not set: the ColBERT head needs the model's "
                               "colbert_linear.pt (set HIP_ALLOW_SYNTHETIC=1 to run on a seeded random head)")
        self.encoder.set_colbert_head(weight, bias)

    def _encode_colbert(self, clean_texts: List[str]):
        toks = [self.tokenizer.encode(t.replace("\n", " "), self.encoder.cfg.max_seq_len) for t in clean_texts]
        with self._lock:
            self._ensure_colbert_head()
            return self.encoder.encode_colbert(toks, batch_size=_MAX_BATCH_SEQS, max_tokens=_MAX_BATCH_TOKENS)

    async def embed_batch_colbert_device(self, texts: List[str]):
        """embed_batch_device plus the per-token vectors of every text, from ONE forward (hipenc_forward_colbert): (vectors
        float32 [n, dim], token vectors bfloat16 [n, L - 1, dim], counts int32 [n]) as CUDA tensors in input order; row
        p < counts[i] of text i is the unit vector of its token p + 1 (CLS skipped).  Same text cleaning as embed_batch."""
        if not texts:
            raise ValueError("embed_batch_colbert_device needs at least one text")
        clean_texts = [t.strip() if t and t.strip() else "" for t in texts]
        return await asyncio.to_thread(self._encode_colbert, clean_texts)

    async def embed_single_colbert(self, text: str, instruction: Optional[str] = None):
        """embed_single plus the query's token vectors from the same forward: (vector as a list of floats, token vectors
        bfloat16 [1, L - 1, dim], counts int32 [1]; the last two CUDA tensors, what hipmaxsim_dev takes).  A blank text gives
        the zero vector and no token vector, like embed_single: every candidate of such a query is padding."""
        import torch
        if not text or not text.strip():
            dev = torch.device("cuda", self.encoder.device)
            return ([0.0] * self._dimension, torch.zeros((1, 1, self._dimension), dtype=torch.bfloat16, device=dev),
                    torch.zeros((1,), dtype=torch.int32, device=dev))
        clean_text = text.strip()
        if instruction and config.HIP_APPLY_INSTRUCTION:
            clean_text = instruction + clean_text
        dense, vecs, counts = await asyncio.to_thread(self._encode_colbert, [clean_text])
        return dense[0].cpu().tolist(), vecs, counts

    def _encode_m3(self, clean_texts: List[str]):
        if not self.encoder.has_lexical:
            raise RuntimeError("this provider was made without a lexical head (HIP_COLLECTION_SPARSE=lexical at construction)")
        toks = [self.tokenizer.encode(t.replace("\n", " "), self.encoder.cfg.max_seq_len) for t in clean_texts]
        with self._lock:
            self._ensure_colbert_head()
            return self.encoder.encode_m3(toks, batch_size=_MAX_BATCH_SEQS, max_tokens=_MAX_BATCH_TOKENS)

    async def embed_batch_m3_device(self, texts: List[str]):
        """All three BGE-M3 outputs of every text from ONE forward (hipenc_forward_m3): what embed_batch_lexical_device and
        embed_batch_colbert_device return together -- (vectors float32 [n, dim], terms int32 [n, L], weights float32 [n, L],
        lexical counts int32 [n], token vectors bfloat16 [n, max(L, 2) - 1, dim], vector counts int32 [n]) as CUDA tensors in
        input order.  Same text cleaning as embed_batch."""
        if not texts:
            raise ValueError("embed_batch_m3_device needs at least one text")
        clean_texts = [t.strip() if t and t.strip() else "" for t in texts]
        return await asyncio.to_thread(self._encode_m3, clean_texts)

    async def embed_single_m3(self, text: str, instruction: Optional[str] = None):
        """embed_single plus the query's lexical weights and token vectors from the same forward: (vector as a list of floats,
        token ids as a list, weights as a float32 numpy array, token vectors bfloat16 [1, L - 1, dim], counts int32 [1]; the
        last two CUDA tensors).  A blank text gives the zero vector, no terms and no token vector."""
        import numpy as np
        import torch
        if not text or not text.strip():
            dev = torch.device("cuda", self.encoder.device)
            return ([0.0] * self._dimension, [], np.zeros(0, np.float32),
                    torch.zeros((1, 1, self._dimension), dtype=torch.bfloat16, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev))
        clean_text = text.strip()
        if instruction and config.HIP_APPLY_INSTRUCTION:
            clean_text = instruction + clean_text
        dense, terms, weights, counts, vecs, vcounts = await asyncio.to_thread(self._encode_m3, [clean_text])
        n = int(counts[0])
        return dense[0].cpu().tolist(), terms[0, :n].cpu().tolist(), weights[0, :n].cpu().numpy(), vecs, vcounts

    def _encode(self, texts: List[str]) -> List[List[float]]:
        toks = [self.tokenizer.encode(t.replace("\n", " "), self.encoder.cfg.max_seq_len) for t in texts]
        with self._lock:
            out = self.encoder.encode_tokens(toks, batch_size=_MAX_BATCH_SEQS, max_tokens=_MAX_BATCH_TOKENS,
                                             packed=config.HIP_ENCODER_PACKED)
            return out.cpu().tolist()

    async def embed_single(self, text: str, instruction: Optional[str] = None) -> List[float]:
        if not text or not text.strip():
            return [0.0] * self._dimension
        clean_text = text.strip()
        if instruction and config.HIP_APPLY_INSTRUCTION:
            clean_text = instruction + clean_text
        try:
            vectors = await asyncio.to_thread(self._encode, [clean_text])
            return vectors[0]
        except Exception as e:
            logger.error(f"[EMBED] HIP embed_single failed: {e}")
            raise

    async def embed_batch(self, texts: List[str], instruction: Optional[str] = None, batch_size: int = 32) -> List[List[float]]:
        if not texts:
            return []
        clean_texts = [t.strip() if t and t.strip() else "" for t in texts]
        if instruction and config.HIP_APPLY_INSTRUCTION:
            clean_texts = [instruction + t if t else t for t in clean_texts]
        try:
            vectors = await asyncio.to_thread(self._encode, clean_texts)
            return [v if v else [0.0] * self._dimension for v in vectors]
        except Exception as e:
            logger.error(f"[EMBED] HIP embed_batch failed: {e}")
            raise

    async def embed_batch_device(self, texts: List[str]):
        """embed_batch without the list-of-lists round trip: a float32 CUDA tensor [n, dim] (the ingest side feeds it
        straight into the index, rag/ingest/indexing.py).  Same text cleaning as embed_batch."""
        import torch
        if not texts:
            return torch.empty((0, self._dimension), dtype=torch.float32, device=f"cuda:{self.encoder.device}")
        clean_texts = [t.strip() if t and t.strip() else "" for t in texts]

        def run():
            toks = [self.tokenizer.encode(t.replace("\n", " "), self.encoder.cfg.max_seq_len) for t in clean_texts]
            with self._lock:
                return self.encoder.encode_tokens(toks, batch_size=_MAX_BATCH_SEQS, max_tokens=_MAX_BATCH_TOKENS,
                                                  packed=config.HIP_ENCODER_PACKED)
        return await asyncio.to_thread(run)

    def dimension(self) -> int:
        return self._dimension
