// multivec.h -- struct MultiVecStore, shared by multivec.hip (the hipmv_* entries) and maxsim.hip (which reads the CSR and
// keeps the workspace of its calls here, because hipmaxsim_info is asked of the store).
//
// SIZE: a stored token costs 2 x dim bytes.  100 k passages of 120 tokens at 1024-d take 24.6 GB; 1 M passages take 245 GB
// and do not fit beside the index.  Narrower stored vectors (a projection, fp8) are the follow-up, not part of this store.
#pragma once
#include <vector>

#include "common.h"

namespace hiprag {

struct MultiVecStore {
    std::mutex mu;
    int device = 0;
    int32_t dim = 0, max_doc_vectors = 0;
    int64_t n_docs = 0, n_vecs = 0;
    int64_t cap_docs = 0, cap_vecs = 0;       // in entries; they grow by half again and are never given back
    std::vector<int32_t> len_host;            // stored vectors of every document: a removal plans its runs without a device read
    int32_t longest = 0;                      // max of len_host
    DevBuf offsets, vecs;                     // int64 [cap_docs + 1] | bf16 [cap_vecs][dim]

    // ---- workspace of the MaxSim calls on this store (maxsim.hip) ------------------------------------------------------
    DevBuf pair_scores;                       // float [pairs] when the caller wants none
    DevBuf counters;                          // uint64 {valid pairs, padding candidates, document vectors read}
    bool lds_opted_in = false;                // the kernel's dynamic LDS bound was raised on this device
};

Registry<MultiVecStore>& mv_reg();   // multivec.hip

#define GET_MV(var, h)                                                                                        \
    std::shared_ptr<MultiVecStore> var = mv_reg().get(h);                                                     \
    if (!var) { set_error("unknown multi-vector store handle %llu", (unsigned long long)(h)); return HIPRAG_E_HANDLE; }

}  // namespace hiprag
