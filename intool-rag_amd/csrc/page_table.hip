// page_table.hip -- the page table (hippage_*, include/hiprag.h): for every collection row the page it lies on and a tag
// of the document it belongs to, on the device, and the call that groups a query's candidates by (tag, page), scores every
// page and orders the pages (the last step of the reference's retriever, rag/query/page_retriever.py:145-236).  The table
// follows the collection as rows, IVF lists, postings and passage tokens do: append at the end, stable compaction on removal.
#include <algorithm>
#include <cfloat>
#include <vector>

#include "page_table.h"

namespace hiprag {

static Registry<PageTable>& page_reg()
{
    static Registry<PageTable> r;
    return r;
}
size_t clear_page_registry() { return page_reg().clear(); }

#define GET_PAGE(var, h) HR_GET_HANDLE(var, page_reg(), h, "unknown page table handle %llu", (unsigned long long)(h))

namespace {

// ---- ranking -------------------------------------------------------------------------------------------------------------
struct RankArgs {
    const int32_t* page;
    const int32_t* tag;
    int64_t rows;
    const int64_t* cand;
    const int64_t* dense_ids;
    const double* dense_scores;
    int depth, dense_depth, nq, metric, max_pages;
    int64_t id_base;
    int32_t* n_pages;
    double* page_scores;
    int32_t* page_first;
    int32_t* page_members;
    int32_t* page_no;
    int32_t* cand_rank;
    int32_t* cand_dpos;
    double* cand_scores;
};

// T threads per query, one per candidate (depth <= T), kRankThreads / T queries per workgroup.  Every step is a loop of at
// most 256 LDS reads per thread; the sum of a page is added by ONE thread in list order, so the bits do not depend on the
// form or on the run.  Every barrier is reached by every thread: a query past nq does the same steps with nothing valid.
template <int T>
__global__ __launch_bounds__(kRankThreads) void page_rank_kernel(RankArgs a)
{
#pragma clang fp contract(off)
    constexpr int Q = kRankThreads / T;
    __shared__ int64_t s_dense[Q][kRankMaxDepth];
    __shared__ int64_t s_key[Q][T];        // (tag << 32) | page of the candidate's row
    __shared__ double s_score[Q][T];       // the candidate's score
    __shared__ double s_pscore[Q][T];      // the score of the page this candidate leads
    __shared__ int s_first[Q][T];          // position of the first member of the candidate's page; -1: padding
    __shared__ int s_dpos[Q][T];
    __shared__ int s_members[Q][T];
    __shared__ int s_pageno[Q][T];
    __shared__ int s_rank[Q][T];           // step 2: validity; from step 4: rank of the page this candidate leads

    const int sub = threadIdx.x / T, lane = threadIdx.x % T;
    const int64_t q = (int64_t)blockIdx.x * Q + sub;
    const bool live = q < a.nq, mine = live && lane < a.depth;

    // 1. the dense list into LDS; the candidate, its row's key
    if (live)
        for (int p = lane; p < a.dense_depth; p += T) s_dense[sub][p] = a.dense_ids[q * a.dense_depth + p];
    int64_t c = -1, key = 0;
    bool valid = false;
    int page_no = 0;
    if (mine) {
        c = a.cand[q * a.depth + lane];
        if (c >= 0 && c >= a.id_base && c - a.id_base < a.rows) {
            const int64_t row = c - a.id_base;
            valid = true;
            page_no = a.page[row];
            key = (int64_t)(((uint64_t)(uint32_t)a.tag[row] << 32) | (uint32_t)page_no);
        }
    }
    s_key[sub][lane] = key;
    s_rank[sub][lane] = valid ? 1 : 0;
    s_pageno[sub][lane] = page_no;
    __syncthreads();

    // 2. dense position and score; the first member of the candidate's page
    int dpos = -1, first = -1;
    double s = 0.0;
    if (valid) {
        for (int p = 0; p < a.dense_depth; ++p)
            if (s_dense[sub][p] == c) { dpos = p; break; }     // c >= 0: a hole (id < 0) never matches
        if (dpos >= 0) {
            const double v = a.dense_scores[q * a.dense_depth + dpos];
            s = a.metric == HIPRAG_METRIC_L2 ? 1.0 - v / 2.0 : v;
            s = s < 1.0 ? s : 1.0;        // min(1.0, s) and max(0.0, s) as Python evaluates them
            s = s > 0.0 ? s : 0.0;
        }
        for (int i = 0; i <= lane; ++i)
            if (s_rank[sub][i] && s_key[sub][i] == key) { first = i; break; }
    }
    s_dpos[sub][lane] = dpos;
    s_score[sub][lane] = s;
    s_first[sub][lane] = first;
    __syncthreads();

    // 3. the leader of a page adds its members up in list order
    const bool leader = valid && first == lane;
    double ps = 0.0;
    int members = 0;
    if (leader) {
        double acc = 0.0;
        int m = 0;
        for (int i = lane; i < a.depth; ++i) {
            if (s_first[sub][i] != lane) continue;
            ++members;
            if (s_dpos[sub][i] >= 0) { acc += s_score[sub][i]; ++m; }
        }
        const double boost = (double)members * 0.05;
        ps = (m ? acc / (double)m : 0.0) + (0.15 < boost ? 0.15 : boost);
    }
    s_pscore[sub][lane] = ps;
    s_members[sub][lane] = members;
    __syncthreads();

    // 4. pages of the query; rank of a led page: score descending, ties to the page seen first
    int n_pages = 0, rank = 0;
    for (int i = 0; i < a.depth; ++i) {
        if (s_first[sub][i] != i) continue;
        ++n_pages;
        const double o = s_pscore[sub][i];
        if (o > ps || (o == ps && i < lane)) ++rank;
    }
    s_rank[sub][lane] = leader ? rank : -1;
    __syncthreads();

    // 5. outputs: thread r looks for the page ranked r, thread j reports candidate j
    if (!live) return;
    if (lane == 0) a.n_pages[q] = n_pages;
    if (lane < a.max_pages) {
        int at = -1;
        for (int i = 0; i < a.depth; ++i)
            if (s_rank[sub][i] == lane) { at = i; break; }
        const int64_t o = q * a.max_pages + lane;
        a.page_scores[o] = at >= 0 ? s_pscore[sub][at] : -DBL_MAX;
        a.page_first[o] = at;
        a.page_members[o] = at >= 0 ? s_members[sub][at] : 0;
        a.page_no[o] = at >= 0 ? s_pageno[sub][at] : 0;
    }
    if (lane < a.depth) {
        const int64_t o = q * a.depth + lane;
        a.cand_rank[o] = valid ? s_rank[sub][first] : -1;
        a.cand_dpos[o] = dpos;
        a.cand_scores[o] = s;
    }
}

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hippage_create(int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "null out");
    HR_CHECK_HIP(hipSetDevice(device));
    auto t = std::make_shared<PageTable>();
    t->device = device;
    *out_handle = page_reg().put(t);
    return HIPRAG_OK;
}

int32_t hippage_destroy(uint64_t h)
{
    GET_PAGE(t, h);
    {
        std::lock_guard<std::mutex> guard(t->mu);
        (void)hipSetDevice(t->device);
        (void)hipDeviceSynchronize();
    }
    page_reg().erase(h);
    return HIPRAG_OK;
}

int32_t hippage_append(uint64_t h, const int32_t* pages_host, const int64_t* doc_offsets_host, int64_t n_docs)
{
    GET_PAGE(t, h);
    std::lock_guard<std::mutex> guard(t->mu);
    HR_CHECK_HIP(hipSetDevice(t->device));
    // every check before anything is touched
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(doc_offsets_host, "doc_offsets is null");
    HR_REQUIRE(pages_host, "pages is null");
    HR_REQUIRE(doc_offsets_host[0] == 0, "doc_offsets must start at 0 (got %lld)", (long long)doc_offsets_host[0]);
    for (int64_t j = 0; j < n_docs; ++j)
        HR_REQUIRE(doc_offsets_host[j] <= doc_offsets_host[j + 1], "doc_offsets descend at document %lld", (long long)j);
    const int64_t n_new = doc_offsets_host[n_docs];
    HR_REQUIRE(n_new < (1ll << 31) && t->n_rows + n_new < (1ll << 31), "the table would hold %lld rows: the limit is 2^31 - 1",
               (long long)(t->n_rows + n_new));
    HR_REQUIRE(t->tags_issued + n_docs < (1ll << 31), "the table would have issued %lld document tags: the limit is 2^31 - 1",
               (long long)(t->tags_issued + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    const int64_t rows_after = t->n_rows + n_new;
    if (n_new > 0) {
        std::vector<int32_t> tags((size_t)n_new);
        for (int64_t j = 0; j < n_docs; ++j)
            std::fill(tags.begin() + doc_offsets_host[j], tags.begin() + doc_offsets_host[j + 1], (int32_t)(t->tags_issued + j));
        if (rows_after > t->cap_rows) {
            const int64_t cap = grown(rows_after, t->cap_rows);
            int32_t rc;
            if ((rc = regrow_parts(t->parts(), cap, t->n_rows, "page table"))) return rc;
            t->cap_rows = cap;
        }
        HR_CHECK_HIP(hipMemcpy(t->page.as<int32_t>() + t->n_rows, pages_host, (size_t)n_new * sizeof(int32_t), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(t->tag.as<int32_t>() + t->n_rows, tags.data(), (size_t)n_new * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    t->n_rows = rows_after;
    t->tags_issued += n_docs;      // an empty document takes a tag too
    return HIPRAG_OK;
}

int32_t hippage_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_PAGE(t, h);
    std::lock_guard<std::mutex> guard(t->mu);
    HR_CHECK_HIP(hipSetDevice(t->device));
    RangeTable tab;
    int32_t rc;
    if ((rc = range_table(ranges_host, n_ranges, t->n_rows, "rows", true, tab))) return rc;
    if (tab.empty()) return HIPRAG_OK;
    // the surviving runs of rows behind the first removed one; rows in front of it are neither read nor written
    std::vector<MoveRun> moves;
    int64_t dst = tab[0].first;
    for (size_t j = 0; j < tab.size(); ++j) {
        const int64_t keep_hi = j + 1 < tab.size() ? tab[j + 1].first : t->n_rows;
        const int64_t run = keep_hi - tab[j].second;
        if (run > 0) moves.push_back(MoveRun{tab[j].second, dst, run});
        dst += run;
    }
    if ((rc = move_parts_down(t->parts(), moves, tab[0].first, dst))) return rc;
    t->n_rows = dst;
    return HIPRAG_OK;
}

int32_t hippage_export(uint64_t h, int32_t* pages, int32_t* tags)
{
    GET_PAGE(t, h);
    std::lock_guard<std::mutex> guard(t->mu);
    HR_CHECK_HIP(hipSetDevice(t->device));
    if (pages && t->n_rows) HR_CHECK_HIP(hipMemcpy(pages, t->page.p, (size_t)t->n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tags && t->n_rows) HR_CHECK_HIP(hipMemcpy(tags, t->tag.p, (size_t)t->n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hippage_sizes(uint64_t h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_PAGE(t, h);
    std::lock_guard<std::mutex> guard(t->mu);
    out4[0] = t->n_rows;
    out4[1] = t->tags_issued;
    out4[2] = t->cap_rows;
    out4[3] = 0;
    return HIPRAG_OK;
}

int32_t hippage_rank_dev(uint64_t h, const int64_t* cand_ids_dev, int32_t depth, const int64_t* dense_ids_dev,
                         const double* dense_scores64_dev, int32_t dense_depth, int32_t nq, int64_t id_base, int32_t metric,
                         int32_t max_pages, int32_t* out_n_pages_dev, double* out_page_scores_dev, int32_t* out_page_first_dev,
                         int32_t* out_page_members_dev, int32_t* out_page_no_dev, int32_t* out_cand_rank_dev,
                         int32_t* out_cand_dense_pos_dev, double* out_cand_scores_dev, void* stream)
{
    GET_PAGE(t, h);
    std::lock_guard<std::mutex> guard(t->mu);
    HR_REQUIRE(cand_ids_dev && dense_ids_dev && dense_scores64_dev, "null input");
    HR_REQUIRE(out_n_pages_dev && out_page_scores_dev && out_page_first_dev && out_page_members_dev && out_page_no_dev &&
               out_cand_rank_dev && out_cand_dense_pos_dev && out_cand_scores_dev, "null output");
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(depth >= 1 && depth <= kRankMaxDepth, "depth must lie in 1..%d (got %d)", kRankMaxDepth, depth);
    HR_REQUIRE(dense_depth >= 1 && dense_depth <= kRankMaxDepth, "dense_depth must lie in 1..%d (got %d)", kRankMaxDepth, dense_depth);
    HR_REQUIRE(max_pages >= 1 && max_pages <= depth, "max_pages must lie in 1..depth = %d (got %d)", depth, max_pages);
    HR_REQUIRE(id_base >= 0, "id_base must not be negative (got %lld)", (long long)id_base);
    HR_REQUIRE(metric == HIPRAG_METRIC_IP || metric == HIPRAG_METRIC_L2, "unknown metric %d", metric);
    HR_CHECK_HIP(hipSetDevice(t->device));
    RankArgs a;
    a.page = t->page.as<int32_t>();
    a.tag = t->tag.as<int32_t>();
    a.rows = t->n_rows;
    a.cand = cand_ids_dev;
    a.dense_ids = dense_ids_dev;
    a.dense_scores = dense_scores64_dev;
    a.depth = depth; a.dense_depth = dense_depth; a.nq = nq; a.metric = metric; a.max_pages = max_pages;
    a.id_base = id_base;
    a.n_pages = out_n_pages_dev;
    a.page_scores = out_page_scores_dev;
    a.page_first = out_page_first_dev;
    a.page_members = out_page_members_dev;
    a.page_no = out_page_no_dev;
    a.cand_rank = out_cand_rank_dev;
    a.cand_dpos = out_cand_dense_pos_dev;
    a.cand_scores = out_cand_scores_dev;
    hipStream_t st = (hipStream_t)stream;
    if (depth <= kRankWaveDepth)
        hipLaunchKernelGGL(page_rank_kernel<kRankWaveDepth>, dim3((unsigned)((nq + kRankWaveQueries - 1) / kRankWaveQueries)),
                           dim3(kRankThreads), 0, st, a);
    else
        hipLaunchKernelGGL(page_rank_kernel<kRankThreads>, dim3((unsigned)nq), dim3(kRankThreads), 0, st, a);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

}  // extern "C"
