// scope_plan.h -- the scope tables of hipidx_search_scoped_dev (include/hiprag.h), stated once for every scoped search and
// for hiprag_scope_plan: their rules, and the int64 image of them a search copies to the device.  Host-only: no HIP, no
// device, so it compiles into a plain C++ program as well.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/hiprag.h"

namespace hiprag {

void set_error(const char* fmt, ...);   // lib.cpp

// The rules over the tables of a structure of n entries, in order: scope_offsets non-null; scope_of_query non-null; the
// offsets start at 0 and do not descend; ranges non-null unless there are none; then per range, scope by scope,
// 0 <= lo <= hi <= n, and after that lo >= the end of the range before it in the scope (an empty one included); then every
// scope_of_query[i] is a scope.  n_scopes >= 1 and nq >= 1 are the caller's to check first.  `name_of_n` is the word the
// structure prints for its count.  Nothing is touched, so a caller that runs it before its first write refuses a bad table
// with its state as it was.
inline int32_t check_scope_tables(const int64_t* ranges, const int32_t* scope_offsets, int32_t n_scopes, const int32_t* scope_of_query,
                                  int32_t nq, int64_t n, const char* name_of_n)
{
    if (!scope_offsets) { set_error("scope_offsets is null"); return HIPRAG_E_INVALID; }
    if (!scope_of_query) { set_error("scope_of_query is null"); return HIPRAG_E_INVALID; }
    if (scope_offsets[0] != 0) { set_error("scope_offsets must start at 0 (got %d)", scope_offsets[0]); return HIPRAG_E_INVALID; }
    for (int s = 0; s < n_scopes; ++s)
        if (scope_offsets[s + 1] < scope_offsets[s]) {
            set_error("scope_offsets descends at scope %d (%d after %d)", s, scope_offsets[s + 1], scope_offsets[s]);
            return HIPRAG_E_INVALID;
        }
    if (!ranges && scope_offsets[n_scopes] != 0) { set_error("ranges is null"); return HIPRAG_E_INVALID; }
    for (int s = 0; s < n_scopes; ++s)
        for (int64_t j = scope_offsets[s]; j < scope_offsets[s + 1]; ++j) {
            const int64_t lo = ranges[2 * j], hi = ranges[2 * j + 1];
            if (!(0 <= lo && lo <= hi && hi <= n)) {
                set_error("ranges[%lld] = [%lld, %lld) of scope %d is not within 0 <= lo <= hi <= %s = %lld", (long long)j, (long long)lo,
                          (long long)hi, s, name_of_n, (long long)n);
                return HIPRAG_E_INVALID;
            }
            if (j != scope_offsets[s] && lo < ranges[2 * j - 1]) {
                set_error("ranges[%lld] = [%lld, %lld) of scope %d starts before the end %lld of the range "
                          "before it: the ranges of a scope ascend and do not overlap", (long long)j, (long long)lo, (long long)hi, s,
                          (long long)ranges[2 * j - 1]);
                return HIPRAG_E_INVALID;
            }
        }
    for (int i = 0; i < nq; ++i)
        if (scope_of_query[i] < 0 || scope_of_query[i] >= n_scopes) {
            set_error("scope_of_query[%d] = %d is not a scope in 0..%d", i, scope_of_query[i], n_scopes - 1);
            return HIPRAG_E_INVALID;
        }
    return HIPRAG_OK;
}

// The staging image of checked tables, all int64, and where its sections begin:
//   ranges | slice_start | scope_off | scope_rows | scope_slices | scope of every query
//   0        o_slice       o_off       o_rows       o_sl           o_soq                  .. words
// A range is cut on ABSOLUTE multiples of slice_rows: slice_start[j] = slices of the ranges before j, scope_rows and
// scope_slices are per scope.  smax = slices of the largest scope (0 when no scope has a row); bound = the work items of the
// call when `group` queries that name a scope share an item = sum over the scopes of ceil(queries naming it / group) x its
// slices.  slice_rows == 0 gives the lean image of a search that does not cut ranges: ranges | scope_off | scope of every
// query -- the three other sections are empty (o_slice == o_off, o_rows == o_sl == o_soq), smax and bound are 0.
struct ScopeImage {
    std::vector<int64_t> img;
    size_t o_slice = 0, o_off = 0, o_rows = 0, o_sl = 0, o_soq = 0, words = 0;
    int64_t smax = 0, bound = 0;
};

inline void build_scope_image(const int64_t* ranges, const int32_t* scope_offsets, int32_t n_scopes, const int32_t* scope_of_query,
                              int32_t nq, int32_t slice_rows, int32_t group, ScopeImage& out)
{
    const bool cut = slice_rows > 0;
    const int64_t n_ranges = scope_offsets[n_scopes];
    out.o_slice = (size_t)2 * n_ranges;
    out.o_off = out.o_slice + (cut ? n_ranges + 1 : 0);
    out.o_rows = out.o_off + n_scopes + 1;
    out.o_sl = out.o_rows + (cut ? n_scopes : 0);
    out.o_soq = out.o_sl + (cut ? n_scopes : 0);
    out.words = out.o_soq + nq;
    out.img.assign(out.words, 0);
    out.smax = out.bound = 0;
    int64_t* img = out.img.data();
    for (int64_t j = 0; j < 2 * n_ranges; ++j) img[j] = ranges[j];
    for (int s = 0; s <= n_scopes; ++s) img[out.o_off + s] = scope_offsets[s];
    for (int i = 0; i < nq; ++i) img[out.o_soq + i] = scope_of_query[i];
    if (!cut) return;
    int64_t* slice_start = img + out.o_slice;
    for (int64_t j = 0; j < n_ranges; ++j) {
        const int64_t lo = ranges[2 * j], hi = ranges[2 * j + 1];
        slice_start[j + 1] = slice_start[j] + (hi > lo ? (hi - 1) / slice_rows - lo / slice_rows + 1 : 0);
    }
    for (int s = 0; s < n_scopes; ++s) {
        int64_t rows = 0;
        for (int64_t j = scope_offsets[s]; j < scope_offsets[s + 1]; ++j) rows += ranges[2 * j + 1] - ranges[2 * j];
        img[out.o_rows + s] = rows;
        img[out.o_sl + s] = slice_start[scope_offsets[s + 1]] - slice_start[scope_offsets[s]];
        if (img[out.o_sl + s] > out.smax) out.smax = img[out.o_sl + s];
    }
    std::vector<int64_t> named((size_t)n_scopes, 0);
    for (int i = 0; i < nq; ++i) ++named[(size_t)scope_of_query[i]];
    for (int s = 0; s < n_scopes; ++s) out.bound += (named[(size_t)s] + group - 1) / group * img[out.o_sl + s];
}

}  // namespace hiprag
