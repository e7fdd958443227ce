// range_table.h -- the table rules of hipidx_remove_ranges (include/hiprag.h), stated once for every *_remove_ranges entry
// and for hiprag_compaction_plan.  Host-only: no HIP, no device, so it compiles into a plain C++ program as well.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/hiprag.h"

namespace hiprag {

void set_error(const char* fmt, ...);   // lib.cpp

using RangeTable = std::vector<std::pair<int64_t, int64_t>>;   // [lo, hi) each, ascending

// The two rules that need no count: n_ranges >= 0, and ranges non-null unless n_ranges == 0.  range_table begins with them;
// the dense index calls them on their own because its refusal of an index with live IVF handles stands between these two
// rules and the per-range ones.
inline int32_t check_range_args(const int64_t* ranges, int32_t n_ranges)
{
    if (n_ranges < 0) { set_error("n_ranges must not be negative (got %d)", n_ranges); return HIPRAG_E_INVALID; }
    if (!ranges && n_ranges != 0) { set_error("ranges is null"); return HIPRAG_E_INVALID; }
    return HIPRAG_OK;
}

// The rules over n_ranges pairs [lo, hi) of a structure of n entries, in order: the two above; then per range, in order,
// 0 <= lo <= hi <= n, and after that lo >= the end of the range before it (an empty one included).  `name_of_n` is the word
// the structure prints for its count.  out = the non-empty ranges, touching ones joined into one when `join` is set.
// Nothing else is touched, so a caller that runs it before its first write refuses a bad table with its state as it was.
inline int32_t range_table(const int64_t* ranges, int32_t n_ranges, int64_t n, const char* name_of_n, bool join, RangeTable& out)
{
    out.clear();
    const int32_t rc = check_range_args(ranges, n_ranges);
    if (rc) return rc;
    for (int j = 0; j < n_ranges; ++j) {
        const int64_t lo = ranges[2 * j], hi = ranges[2 * j + 1];
        if (!(0 <= lo && lo <= hi && hi <= n)) {
            set_error("ranges[%d] = [%lld, %lld) is not within 0 <= lo <= hi <= %s = %lld", j, (long long)lo, (long long)hi, name_of_n,
                      (long long)n);
            return HIPRAG_E_INVALID;
        }
        if (j > 0 && lo < ranges[2 * j - 1]) {
            set_error("ranges[%d] = [%lld, %lld) starts before the end %lld of the range before it: "
                      "the ranges ascend and do not overlap", j, (long long)lo, (long long)hi, (long long)ranges[2 * j - 1]);
            return HIPRAG_E_INVALID;
        }
        if (hi == lo) continue;
        if (join && !out.empty() && out.back().second == lo) out.back().second = hi;
        else out.emplace_back(lo, hi);
    }
    return HIPRAG_OK;
}

}  // namespace hiprag
