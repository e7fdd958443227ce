// multivec.h -- struct MultiVecStore, shared by multivec.hip (the hipmv_* entries) and maxsim.hip (which reads the CSR and
// keeps the workspace of its calls here, because hipmaxsim_info is asked of the store).
//
// SIZE: a stored token costs 2 x dim bytes in the bf16 format (0): 100 k passages of 120 tokens at 1024-d take 24.6 GB, 1 M
// passages 245 GB, which do not fit beside the index.  The fp8 format (1) stores OCP e4m3fn codes with one power-of-two
// fp32 scale per vector, dim + 4 bytes per token: 12.3 GB and 123 GB for the same two collections.
//
// THE FP8 FORMAT, per stored vector v[dim] of bf16 values (hiprag.colbert.fp8_quantize_reference restates it in numpy):
//   amax = max_k |v_k|.  amax == 0: codes 0x00, scale 1.0f.  A non-finite component, or amax outside [2^-60, 2^60]: stored
//   as the zero vector with scale 1.0f, and counted (hipmv_format_info).  Otherwise e = 7 - floor(log2 amax), read off amax's
//   exponent bits; code_k = e4m3fn(v_k * 2^e), round to nearest even (the product is exact in fp32 and at most 256 < 448: no
//   saturation), a -0 code stored as 0x00; scale = 2^-e.  code * scale is exact in bf16.
#pragma once
#include "doc_store.h"

namespace hiprag {

constexpr int32_t kMvBf16 = 0, kMvFp8 = 1;

struct MaxsimSearchWs;

struct MultiVecStore {
    std::mutex mu;
    int device = 0;
    int32_t dim = 0;
    DocCsr csr{"multi-vector store"};         // items = vectors, doc_cap = max_doc_vectors
    int32_t format = 0;                       // kMvBf16 or kMvFp8, fixed at creation
    DevBuf vecs;                              // format 0: bf16 [csr.cap_items][dim]
    DevBuf codes, scales;                     // format 1: uint8 [csr.cap_items][dim] | float [csr.cap_items]
    DevBuf guarded;                           // format 1: uint64 {vectors stored as zero by the domain guard since creation}

    // The per-vector arrays of this store's format, in the order of its file: all that capacity, removal, save and load know
    // of a format.  The last part is the large one.
    StoreParts parts()
    {
        if (format == kMvFp8) return StoreParts{2, {{&scales, sizeof(float)}, {&codes, (size_t)dim}}};
        return StoreParts{1, {{&vecs, (size_t)dim * 2}, {nullptr, 0}}};
    }

    // ---- workspace of the MaxSim calls on this store (maxsim.hip) ------------------------------------------------------
    DevBuf pair_scores;                       // float [pairs] when the caller wants none
    DevBuf counters;                          // uint64 {valid pairs, padding candidates, document vectors read}
    bool lds_opted_in = false;                // the kernel's dynamic LDS bound was raised on this device
    // workspace and counters of hipmaxsim_search_scoped* (maxsim_search.hip, which defines and makes it on first use)
    std::shared_ptr<MaxsimSearchWs> search_ws;
};

Registry<MultiVecStore>& mv_reg();   // multivec.hip

#define GET_MV(var, h) HR_GET_HANDLE(var, mv_reg(), h, "unknown multi-vector store handle %llu", (unsigned long long)(h))

}  // namespace hiprag
