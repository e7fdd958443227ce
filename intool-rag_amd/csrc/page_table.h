// page_table.h -- struct PageTable and the dispatch constants of the ranking kernel (page_table.hip).
#pragma once
#include "doc_store.h"

namespace hiprag {

// The ranking call has two forms of one kernel, both with workgroups of kRankThreads threads and one thread per candidate:
//   depth <= kRankWaveDepth   one wave per query, kRankWaveQueries queries per workgroup
//   deeper                    one workgroup per query
// hiprag/pages.py repeats the three numbers under the same names for the tests.
constexpr int kRankMaxDepth = 256;       // of the candidate list and of the dense list
constexpr int kRankThreads = 256;
constexpr int kRankWaveDepth = 64;
constexpr int kRankWaveQueries = kRankThreads / kRankWaveDepth;   // 4

struct PageTable {
    std::mutex mu;
    int device = 0;
    int64_t n_rows = 0, cap_rows = 0;      // capacity in rows; it grows by half again and is never given back
    int64_t tags_issued = 0;               // the next document tag; a value is never reused
    DevBuf page, tag;                      // int32 [cap_rows] each
    // The large part first means the last part first (doc_store.h): the page column grows and moves before the tag column.
    StoreParts parts() { return StoreParts{2, {{&tag, sizeof(int32_t)}, {&page, sizeof(int32_t)}}}; }
};

}  // namespace hiprag
