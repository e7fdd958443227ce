// doc_store.h -- what the stores that follow a collection's appends and removals share (doc_store.hip): the description of
// a store's arrays as parts, growth by half again, the mover of a stable compaction, and DocCsr, the document CSR under the
// passage token store (token_store.h) and the multi-vector store (multivec.h).  The page table (page_table.h) has no
// per-document offsets and uses the parts, the growth and the mover alone.  A further structure that follows the collection
// is a struct and a list of parts on top of this.
#pragma once
#include <vector>

#include "common.h"
#include "compaction_plan.h"

namespace hiprag {

// One of the device arrays of a store that hold one entry per stored item, and the bytes of an entry (a multiple of 4).
struct StorePart {
    DevBuf* buf;
    size_t bytes;
};
// A store's arrays, in the order of its file where it has one.  The last part is the large one.  Three at most: the two of a
// quantised multi-vector store and its centroid codes (multivec.h).
struct StoreParts {
    int n;
    StorePart p[3];
    const StorePart* begin() const { return p; }
    const StorePart* end() const { return p + n; }
};

// capacities grow by half again and are never given back
int64_t grown(int64_t need, int64_t cap);

// A larger buffer with the first `keep` bytes of the old one.  Out of device memory is HIPRAG_E_NOMEM with a message that
// names `store`, and leaves the old buffer in place.
int32_t regrow(DevBuf& buf, size_t bytes, size_t keep, const char* store);

// Every part to `cap` entries with the first `keep` of them, the large part first: it is the one that can fail.
int32_t regrow_parts(const StoreParts& parts, int64_t cap, int64_t keep, const char* store);

// The mover of a stable compaction over an int32 device array: `moves` ascend and their destinations tile [d_begin, d_end);
// the elements move on the device through a staging buffer of at most 128 MiB, on the null stream, and the call
// synchronises it.  Nothing in front of d_begin is read or written.
int32_t move_runs_down_i32(int32_t* data, const std::vector<MoveRun>& moves, int64_t d_begin, int64_t d_end);

// The same for every part of a store, the large part first (its staging buffer is the one that can fail): `runs`, `begin`
// and `end` count entries, and each part moves them as its int32 words.
int32_t move_parts_down(const StoreParts& parts, const std::vector<MoveRun>& runs, int64_t begin, int64_t end);

// The document CSR of a store: document i = collection row i holds len_host[i] items (tokens, vectors) at offsets[i] of every
// part.  Appends go at the end, each document cut to doc_cap items; a removal is a stable compaction.
struct DocCsr {
    const char* name;                         // of the store, for messages
    int32_t doc_cap = 0;                      // items a document keeps at most
    int64_t n_docs = 0, n_items = 0;
    int64_t cap_docs = 0, cap_items = 0;      // in entries
    std::vector<int32_t> len_host;            // stored length of every document: plans and bounds need no device read
    int32_t longest = 0;                      // max of len_host
    DevBuf offsets;                           // int64 [cap_docs + 1]

    explicit DocCsr(const char* store_name) : name(store_name) {}

    int32_t init(int32_t cap_per_doc);        // offsets[0] = 0 exists from the start

    // The plan of an append of n_new documents, document i bringing len_of(i) items: `lens` are the stored lengths (capped),
    // `off` the store's offsets from the first new document on.
    template <class LenOf>
    void plan_append(int64_t n_new, LenOf len_of, std::vector<int64_t>& off, std::vector<int32_t>& lens) const
    {
        off.resize((size_t)n_new + 1);
        lens.resize((size_t)n_new);
        off[0] = n_items;
        for (int64_t i = 0; i < n_new; ++i) {
            lens[(size_t)i] = (int32_t)std::min<int64_t>(len_of(i), doc_cap);
            off[(size_t)i + 1] = off[(size_t)i] + lens[(size_t)i];
        }
    }
    // room for docs_after documents and items_after items; the contents stay
    int32_t ensure_capacity(const StoreParts& parts, int64_t docs_after, int64_t items_after);
    // `off` of plan_append to the device, behind the stored offsets
    int32_t write_offsets(const std::vector<int64_t>& off);
    // The bookkeeping of an append whose items and offsets are already in place behind the stored ones.
    void commit_append(const std::vector<int64_t>& off, const std::vector<int32_t>& lens);

    // The removal of a joined, non-empty table (range_table.h): plan_compaction over len_host, then apply_removal.
    int32_t remove(const StoreParts& parts, const RangeTable& tab);
    // every part moves, the large part first; then the offsets behind the first removed document; then the host state
    int32_t apply_removal(const StoreParts& parts, CompactionPlan& plan);
};

}  // namespace hiprag
