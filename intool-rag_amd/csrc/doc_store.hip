// doc_store.hip -- growth, the mover and the document CSR of the stores that follow a collection (doc_store.h), and
// hiprag_compaction_plan (include/hiprag.h), which answers with the plan DocCsr::remove carries out.
#include "doc_store.h"

namespace hiprag {

namespace {

constexpr int kMoveThreads = 256;
constexpr int64_t kMoveChunk = 32ll << 20;   // elements per pass of a removal: 128 MiB of staging whatever the store holds

// stage[i - d0] = data[source of destination element i], d0 <= i < d1.  One thread per element; the run is found by bisection.
__global__ __launch_bounds__(kMoveThreads) void gather_runs_kernel(const int32_t* __restrict__ tokens, const MoveRun* __restrict__ moves,
                                                                   int n_moves, int64_t d0, int64_t d1, int32_t* __restrict__ stage)
{
    const int64_t i = d0 + (int64_t)blockIdx.x * kMoveThreads + threadIdx.x;
    if (i >= d1) return;
    int lo = 0, hi = n_moves - 1;   // the last run with dst <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (moves[mid].dst <= i) lo = mid; else hi = mid - 1;
    }
    const MoveRun m = moves[lo];
    stage[i - d0] = tokens[m.src + (i - m.dst)];
}

}  // namespace

int64_t grown(int64_t need, int64_t cap) { return std::max(need, cap + cap / 2); }

int32_t regrow(DevBuf& buf, size_t bytes, size_t keep, const char* store)
{
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        set_error("out of device memory growing the %s to %zu bytes", store, bytes);
        return HIPRAG_E_NOMEM;
    }
    HR_CHECK_HIP(e);
    if (keep) {
        const hipError_t c = hipMemcpy(p, buf.p, keep, hipMemcpyDeviceToDevice);
        if (c != hipSuccess) { (void)hipFree(p); HR_CHECK_HIP(c); }
    }
    if (buf.p) (void)hipFree(buf.p);
    buf.p = p;
    buf.bytes = bytes;
    return HIPRAG_OK;
}

int32_t regrow_parts(const StoreParts& parts, int64_t cap, int64_t keep, const char* store)
{
    int32_t rc;
    for (int p = parts.n - 1; p >= 0; --p)
        if ((rc = regrow(*parts.p[p].buf, (size_t)cap * parts.p[p].bytes, (size_t)keep * parts.p[p].bytes, store))) return rc;
    return HIPRAG_OK;
}

int32_t move_runs_down_i32(int32_t* data, const std::vector<MoveRun>& moves, int64_t d_begin, int64_t d_end)
{
    if (moves.empty() || d_end <= d_begin) return HIPRAG_OK;
    int32_t rc;
    DevBuf moves_dev, stage;       // freed behind the synchronisation below
    if ((rc = moves_dev.reserve(moves.size() * sizeof(MoveRun)))) return rc;
    if ((rc = stage.reserve((size_t)std::min(kMoveChunk, d_end - d_begin) * sizeof(int32_t)))) return rc;
    HR_CHECK_HIP(hipMemcpy(moves_dev.p, moves.data(), moves.size() * sizeof(MoveRun), hipMemcpyHostToDevice));
    // Every element moves DOWN (dst <= src), so the sources of the destinations behind a chunk lie behind that chunk too:
    // chunks in ascending order, each gathered into the staging buffer and copied into place, never overwrite a source.
    for (int64_t d0 = d_begin; d0 < d_end; d0 += kMoveChunk) {
        const int64_t d1 = std::min(d_end, d0 + kMoveChunk);
        hipLaunchKernelGGL(gather_runs_kernel, dim3((unsigned)((d1 - d0 + kMoveThreads - 1) / kMoveThreads)), dim3(kMoveThreads), 0,
                           nullptr, (const int32_t*)data, (const MoveRun*)moves_dev.as<MoveRun>(), (int)moves.size(), d0, d1,
                           stage.as<int32_t>());
        HR_CHECK_HIP(hipGetLastError());
        HR_CHECK_HIP(hipMemcpyAsync(data + d0, stage.p, (size_t)(d1 - d0) * sizeof(int32_t), hipMemcpyDeviceToDevice, nullptr));
    }
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return HIPRAG_OK;
}

int32_t move_parts_down(const StoreParts& parts, const std::vector<MoveRun>& runs, int64_t begin, int64_t end)
{
    int32_t rc;
    std::vector<MoveRun> in_words(runs.size());
    for (int p = parts.n - 1; p >= 0; --p) {
        const int64_t w = (int64_t)parts.p[p].bytes / 4;   // the mover's int32 words per entry
        for (size_t j = 0; j < runs.size(); ++j) in_words[j] = MoveRun{runs[j].src * w, runs[j].dst * w, runs[j].len * w};
        if ((rc = move_runs_down_i32(parts.p[p].buf->as<int32_t>(), in_words, begin * w, end * w))) return rc;
    }
    return HIPRAG_OK;
}

int32_t DocCsr::init(int32_t cap_per_doc)
{
    doc_cap = cap_per_doc;
    int32_t rc;
    if ((rc = offsets.reserve(sizeof(int64_t)))) return rc;
    HR_CHECK_HIP(hipMemset(offsets.p, 0, sizeof(int64_t)));
    return HIPRAG_OK;
}

int32_t DocCsr::ensure_capacity(const StoreParts& parts, int64_t docs_after, int64_t items_after)
{
    int32_t rc;
    if (docs_after > cap_docs) {
        const int64_t cap = grown(docs_after, cap_docs);
        if ((rc = regrow(offsets, (size_t)(cap + 1) * sizeof(int64_t), (size_t)(n_docs + 1) * sizeof(int64_t), name))) return rc;
        cap_docs = cap;
    }
    if (items_after > cap_items) {
        const int64_t cap = grown(items_after, cap_items);
        if ((rc = regrow_parts(parts, cap, n_items, name))) return rc;
        cap_items = cap;
    }
    return HIPRAG_OK;
}

int32_t DocCsr::write_offsets(const std::vector<int64_t>& off)
{
    HR_CHECK_HIP(hipMemcpy(offsets.as<int64_t>() + n_docs, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return HIPRAG_OK;
}

void DocCsr::commit_append(const std::vector<int64_t>& off, const std::vector<int32_t>& lens)
{
    len_host.insert(len_host.end(), lens.begin(), lens.end());
    for (int32_t l : lens) longest = std::max(longest, l);
    n_docs += (int64_t)lens.size();
    n_items = off.back();
}

int32_t DocCsr::remove(const StoreParts& parts, const RangeTable& tab)
{
    CompactionPlan plan = plan_compaction(len_host.data(), n_docs, tab);
    return apply_removal(parts, plan);
}

int32_t DocCsr::apply_removal(const StoreParts& parts, CompactionPlan& plan)
{
    int32_t rc;
    if ((rc = move_parts_down(parts, plan.runs, plan.item_first, plan.items_after))) return rc;
    HR_CHECK_HIP(hipMemcpy(offsets.as<int64_t>() + plan.first, plan.off.data(), plan.off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    n_docs = (int64_t)plan.lens_after.size();
    len_host.swap(plan.lens_after);
    n_items = plan.items_after;
    longest = plan.longest;
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hiprag_compaction_plan(const int32_t* lens, int64_t n_docs, const int64_t* ranges, int32_t n_ranges, int64_t* out6,
                               int64_t* out_runs)
{
    HR_REQUIRE(out6, "null out");
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(lens || n_docs == 0, "lens is null");
    for (int64_t i = 0; i < n_docs; ++i) HR_REQUIRE(lens[i] >= 0, "lens[%lld] = %d is negative", (long long)i, lens[i]);
    RangeTable tab;
    int32_t rc;
    if ((rc = range_table(ranges, n_ranges, n_docs, "n_docs", true, tab))) return rc;
    HR_REQUIRE(out_runs || n_ranges == 0, "runs is null");
    const CompactionPlan p = plan_compaction(lens, n_docs, tab);
    const int64_t out[6] = {p.first, p.item_first, (int64_t)p.lens_after.size(), p.items_after, p.longest, (int64_t)p.runs.size()};
    std::copy(out, out + 6, out6);
    for (size_t j = 0; j < p.runs.size(); ++j) {
        out_runs[3 * j] = p.runs[j].src;
        out_runs[3 * j + 1] = p.runs[j].dst;
        out_runs[3 * j + 2] = p.runs[j].len;
    }
    return HIPRAG_OK;
}

}  // extern "C"
