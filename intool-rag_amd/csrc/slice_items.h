// slice_items.h -- the work items of the sliced scoped searches, stated once: the flat scoped search (dense_scoped.hip, 256 rows
// per slice, 16 queries per item), the exact late-interaction search (maxsim_search.hip, 16 documents, 8 queries) and the
// pruned one (maxsim_codes.hip, 256 documents, 8 queries).  An ITEM = (scope, slice of S entries cut on ABSOLUTE multiples
// of S, group of up to G of the queries that name the scope); items come in (scope, slice, group) order, so the workgroups
// that run side by side share a slice in L2 / MALL.  slice_item finds an item's scope, slice, group and entry window from
// the six device tables: every entry of a scope is seen exactly once per query group (tests/test_slice_items_cpu.py asks
// it through hiprag_slice_items without a device).  Host and device, no HIP runtime call, like scope_plan.h.
#pragma once

#if defined(__HIPCC__)
#define HIPRAG_SLICE_HD __attribute__((host)) __attribute__((device)) __attribute__((always_inline)) inline
#else
#define HIPRAG_SLICE_HD inline
#endif

namespace hiprag {

typedef long long i64;   // as topk_device.h has it

// The tables a sliced kernel reads: three sections of the scope image (scope_plan.h), then what the counting sort and
// group_item_scan (group_partials.hip) make of a chunk's queries.
struct SliceTables {
    const i64* ranges;       // [n_ranges][2]
    const i64* slice_start;  // [n_ranges + 1] slices of the ranges before j
    const i64* scope_off;    // [n_scopes + 1]
    const i64* pair_offs;    // [n_scopes + 1] first entry of every scope in `order`
    const i64* order;        // the chunk's queries sorted by scope (stable)
    const i64* item_start;   // [n_scopes + 1]; [n_scopes] = the item count
    int n_scopes;
};

struct SliceItem {
    int scope;
    i64 slice;           // slice of the scope = part of the partial lists
    int group, members;  // group of the scope's queries; its 1..G members are order[first .. first + members)
    i64 first, base;     // base: the slice's absolute boundary, a multiple of S
    int p_lo, p_hi;      // entries of the range in the slice: positions [p_lo, p_hi) behind base
};

// Every value is workgroup-uniform: on the device the decode runs in scalar registers.
template <int G, int S>
HIPRAG_SLICE_HD SliceItem slice_item(const SliceTables& a, i64 item)
{
    int s = 0, sh = a.n_scopes;              // item_start[s] <= item < item_start[sh]
    while (sh - s > 1) {
        const int mid = (s + sh) >> 1;
        if (a.item_start[mid] <= item) s = mid; else sh = mid;
    }
    const i64 p0 = a.pair_offs[s], cnt = a.pair_offs[s + 1] - p0;
    const int ngroups = (int)((cnt + G - 1) / G);
    const i64 within = item - a.item_start[s];
    const i64 sl = within / ngroups;                              // slice of the scope = part of the partial lists
    const int grp = (int)(within - sl * ngroups);
    const int gn = (int)(cnt - (i64)grp * G < G ? cnt - (i64)grp * G : (i64)G);   // 1..G members
    i64 j = a.scope_off[s], jh = a.scope_off[s + 1];
    const i64 s0 = a.slice_start[j] + sl;    // slice_start[j] <= s0 < slice_start[jh]: the last such j is a range with entries
    while (jh - j > 1) {
        const i64 mid = (j + jh) >> 1;
        if (a.slice_start[mid] <= s0) j = mid; else jh = mid;
    }
    const i64 lo = a.ranges[2 * j], hi = a.ranges[2 * j + 1];
    const i64 base = (lo / S + (s0 - a.slice_start[j])) * S;     // absolute slice boundary: in the flat index quad- and block-aligned
    const int p_lo = (int)((lo > base ? lo : base) - base), p_hi = (int)((hi < base + S ? hi : base + S) - base);   // entries of the range: positions [p_lo, p_hi)
    return SliceItem{s, sl, grp, gn, p0 + (i64)grp * G, base, p_lo, p_hi};
}

}  // namespace hiprag
