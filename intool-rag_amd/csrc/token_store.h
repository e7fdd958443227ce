// token_store.h -- struct TokenStore, shared by token_store.hip (the hiptok_* entries) and rerank.hip (which reads the CSR and
// keeps the workspace of its calls here, because hiprerank_info is asked of the store).
#pragma once
#include <vector>

#include "common.h"

namespace hiprag {

struct TokenStore {
    std::mutex mu;
    int device = 0;
    int32_t vocab = 0, bos = 0, eos = 0, pad = 0, max_doc_tokens = 0;
    int64_t n_docs = 0, n_tokens = 0;
    int64_t cap_docs = 0, cap_tokens = 0;     // in entries; they grow by half again and are never given back
    std::vector<int32_t> len_host;            // stored length of every document: the S bound of a rerank call needs no device read
    int32_t longest = 0;                      // max of len_host
    DevBuf offsets, tokens;                   // int64 [cap_docs + 1] | int32 [cap_tokens]: bodies only, no special tokens

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

// One surviving run of a removal: `len` int32 elements at src move down to dst (dst <= src).
struct MoveRun {
    int64_t src, dst, len;
};

// The mover of a stable compaction over an int32 device array, shared by the token store and the page table
// (page_table.hip): `moves` ascend and their destinations tile [d_begin, d_end); the elements move on the device through a
// staging buffer of at most 128 MiB, on the null stream, and the call synchronises it.  Nothing in front of d_begin is
// read or written.
int32_t move_runs_down_i32(int32_t* data, const std::vector<MoveRun>& moves, int64_t d_begin, int64_t d_end);

#define GET_TOK(var, h)                                                                                      \
    std::shared_ptr<TokenStore> var = tok_reg().get(h);                                                      \
    if (!var) { set_error("unknown token store handle %llu", (unsigned long long)(h)); return HIPRAG_E_HANDLE; }

}  // namespace hiprag
