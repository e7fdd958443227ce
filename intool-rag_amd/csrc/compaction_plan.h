// compaction_plan.h -- what the removal of a range table does to a document CSR, worked out on the host from the stored
// lengths alone: the plan DocCsr::remove (doc_store.h) carries out and hiprag_compaction_plan (include/hiprag.h) reports.
// Host-only, like range_table.h.
#pragma once
#include <algorithm>

#include "range_table.h"

namespace hiprag {

// One surviving run of a removal: `len` entries at src move down to dst (dst <= src).
struct MoveRun {
    int64_t src, dst, len;
};

struct CompactionPlan {
    int64_t first = 0;                 // the first removed document
    int64_t item_first = 0;            // its offset: nothing in front of it is read or written
    std::vector<MoveRun> runs;         // in items, ascending; their destinations tile [item_first, items_after)
    std::vector<int64_t> off;          // the new offsets of the documents first .. docs after
    std::vector<int32_t> lens_after;   // the stored length of every surviving document
    int64_t items_after = 0;
    int32_t longest = 0;               // max of lens_after
};

// `tab` is a joined table of range_table over n_docs documents.  The host knows every length, so it knows where every
// surviving run of items lies and where it goes.  A run is emitted when it holds an item, also when nothing in front of it
// was removed but empty documents (src == dst then).  An empty table gives first = n_docs and no run.
inline CompactionPlan plan_compaction(const int32_t* lens, int64_t n_docs, const RangeTable& tab)
{
    CompactionPlan p;
    p.first = tab.empty() ? n_docs : tab[0].first;
    for (int64_t i = 0; i < p.first; ++i) p.item_first += lens[i];
    p.lens_after.assign(lens, lens + p.first);
    p.off.push_back(p.item_first);
    int64_t src = p.item_first, dst = p.item_first;
    for (size_t j = 0; j < tab.size(); ++j) {
        for (int64_t i = tab[j].first; i < tab[j].second; ++i) src += lens[i];   // removed: skipped
        const int64_t keep_hi = j + 1 < tab.size() ? tab[j + 1].first : n_docs;
        int64_t run = 0;
        for (int64_t i = tab[j].second; i < keep_hi; ++i) {
            run += lens[i];
            p.lens_after.push_back(lens[i]);
            p.off.push_back(dst + run);
        }
        if (run > 0) p.runs.push_back(MoveRun{src, dst, run});
        src += run;
        dst += run;
    }
    for (int32_t len : p.lens_after) p.longest = std::max(p.longest, len);
    p.items_after = dst;
    return p;
}

}  // namespace hiprag
