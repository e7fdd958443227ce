// ivf_internal.h -- struct IvfIndex and its registry, as far as ivf_search.hip (search, accessors), ivf_scoped.hip (scoped
// search), ivf_build.hip (k-means build, save / load) and ivf_update.hip (add, removal) share them.
#pragma once
#include "dense_internal.h"

namespace hiprag {

struct IvfIndex {
    std::mutex mu;
    std::shared_ptr<DenseIndex> rows, cents;
    // hipivf_create: rows and centroids are the caller's flat handles, and the list offsets name rows of `rows` (lists of
    // `cents`): while this handle lives, hipidx_remove_ranges refuses both.  (A built or loaded IVF owns private indexes no
    // handle reaches.)
    bool attached = false;
    void attach(std::shared_ptr<DenseIndex> r, std::shared_ptr<DenseIndex> c)
    {
        rows = std::move(r); cents = std::move(c);
        ++rows->ivf_refs; ++cents->ivf_refs;
        attached = true;
    }
    ~IvfIndex()
    {
        if (attached) { --rows->ivf_refs; --cents->ivf_refs; }
    }
    DevBuf offs, orig, probe64, probe_ids;
    GroupWorkspace gw;     // the partial lists of both searches; the batch search's inversion of the probe table
    DevBuf list_tab;       // batch and scoped search: [nlist] slices | [nlist] stored rows of every list (ensure_list_tab)
    // scoped search (ivf_scoped.hip): the pinned staging ring and device image of the call's scope tables, as the flat
    // index keeps them; sc.gw holds only the chunking of the last scoped call and its rows-read counter (the partial lists
    // and the inversion are gw's).  hq .. hoid: device copies of the host entry's query and outputs.
    ScopeUpload sc;
    DevBuf hq, ho64, ho32, hoid;
    int nlist = 0;
    i64 maxlen = 0;       // longest list, in stored rows
    i64 probed_rows = 0, searches = 0;   // stats: stored rows of the probed lists, queries
    std::vector<i64> offs_host;
    i64 n_rows = 0;        // original rows (ids 0..n_rows-1)
    float build_ms[3] = {0.f, 0.f, 0.f};   // hipivf_build*: assignment, update, layout (host wall clock)
    // updates (ivf_update.hip)
    std::vector<i64> lens_host;            // members of every list, once an update has read them off `orig`
    bool lens_known = false;
    i64 up_info[5] = {0, 0, 0, 0, 0};      // hipivf_update_info: rows added, removed, stored rows moved, chunks, extra device bytes
    // scope-aware probing (ivf_scoped.hip, HIPIVF_PROBE_SCOPE)
    DevBuf lens_dev;       // device copy of lens_host: valid while lens_known (ensure_lens makes it, refresh() follows the updates)
    DevBuf member;         // [n_scopes][nlist rounded up to 4] bytes: list l holds a row of scope s
    DevBuf cand_s, cand_i; // [queries of a chunk][nlist rounded up to 4] coarse candidates: fp64 score, list (-1: not a member)
    DevBuf sp_stat;        // u64 [3]: member pairs, probed slots, centroid rows read of the last PROBE_SCOPE call
    i64 sp_chunks = 0;     // its chunks
};

Registry<IvfIndex>& ivf_reg();   // ivf_search.hip
int32_t ensure_list_tab(IvfIndex& iv);   // ivf_search.hip: iv.list_tab from offs_host, unless it is there
// ivf_build.hip: out[r] = src[idx[r]] for r in [0, m), a zero row where idx[r] < 0 (ivf_gather_kernel)
int32_t ivf_gather_rows(const float* src, i64 n_src, int d, const i64* idx, i64 m, float* out, hipStream_t st);

// ivf_update.hip: the members of every list (lens_host, lens_dev), on first use read off `orig`; HIPRAG_E_UNSUPPORTED, with
// `cannot` naming what the caller may not do, unless every list is in the build's layout.  Synchronises once per handle.
int32_t ensure_lens(IvfIndex& iv, const char* cannot);

#define GET_IVF(h) HR_GET_HANDLE(iv, ivf_reg(), h, "unknown IVF handle")

}  // namespace hiprag
