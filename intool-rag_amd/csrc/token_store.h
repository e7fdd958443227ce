// token_store.h -- struct TokenStore, shared by token_store.hip (the hiptok_* entries) and rerank.hip (which reads the CSR and
// keeps the workspace of its calls here, because hiprerank_info is asked of the store).
#pragma once
#include "doc_store.h"

namespace hiprag {

struct TokenStore {
    std::mutex mu;
    int device = 0;
    int32_t vocab = 0, bos = 0, eos = 0, pad = 0;
    DocCsr csr{"token store"};                // items = tokens, doc_cap = max_doc_tokens; len_host gives a rerank call its S bound
    DevBuf tokens;                            // int32 [csr.cap_items]: bodies only, no special tokens
    StoreParts parts() { return StoreParts{1, {{&tokens, sizeof(int32_t)}, {nullptr, 0}}}; }

    // ---- workspace of the rerank calls on this store (rerank.hip) ------------------------------------------------------
    // Query arrays go through a ring of pinned buffers, each with the event of its last copy (Bm25Index::stages): a call
    // waits for nothing but the copy out of ITS buffer, kStages calls ago.
    static constexpr int kStages = 4;
    struct Stage {
        PinBuf pin;
        hipEvent_t ev = nullptr;
        bool used = false;
    };
    Stage stages[kStages];
    unsigned stage_next = 0;
    DevBuf q_dev;                             // int32: nq + 1 offsets, then the query tokens
    DevBuf logits, counters;                  // float [pairs] when the caller wants none | int32 {valid pairs, padding slots}
    int64_t last_S = 0, last_batches = 0;     // hiprerank_info
    // the packed calls (hiprerank_packed_*): counters holds their {valid pairs, padding slots} at [2], [3]
    DevBuf pk_lens;                           // int32 [pairs]: the length of every pair, from the device
    PinBuf pk_pin_lens, pk_pin_tab;           // those lengths on the host | the layout tables on their way up
    hipEvent_t pk_ev = nullptr;               // the last copy out of pk_pin_tab
    bool pk_used = false;
    int64_t pk_rows = 0, pk_batches = 0;      // hiprerank_packed_info

    ~TokenStore()
    {
        for (Stage& s : stages)
            if (s.ev) (void)hipEventDestroy(s.ev);
        if (pk_ev) (void)hipEventDestroy(pk_ev);
    }
};

Registry<TokenStore>& tok_reg();   // token_store.hip

#define GET_TOK(var, h) HR_GET_HANDLE(var, tok_reg(), h, "unknown token store handle %llu", (unsigned long long)(h))

}  // namespace hiprag
