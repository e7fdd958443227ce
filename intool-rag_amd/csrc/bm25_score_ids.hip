// bm25_score_ids.hip -- the sparse score of GIVEN documents (hipbm25_score_ids*): what hipidx_score_ids is to the flat index.
// A search scores a document as a by-product of finding it; a candidate the dense leg found has no lexical score unless the
// top-k list happened to hold it.  This call scores ANY (query, document id) pairs, in the bits the searches give them.
#include <cfloat>
#include <cmath>

#include "bm25_internal.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// ids int64 [nq][depth].  Entry (i, j) = c names local document c - id_base; valid iff c >= 0 and 0 <= c - id_base < n_docs.
// A valid entry gets the fp32 sum, IN QUERY-TERM ORDER, of fl32(w_t * impact[t, d]) over the query's slots whose list holds d
// (product rounded, then the add rounded: weighted_add of bm25.hip, spelled again here under contract(off)); 0.0f when no
// slot matches.  A slot that does not hold d adds nothing in the searches either (they only ever touch the documents of a
// list), so the sum over the hits in slot order IS the searches' sum.  An invalid entry is padding: nothing is read for it
// and it gets -FLT_MAX.  Duplicates are separate entries, no order is assumed.
//
// A workgroup (256 threads = 4 waves) takes one query and `chunk` consecutive entries of its list (dense_score_ids.hip's
// rule: the smallest of 4, 8, .. 64 at which the grid is at most kSidGridTarget workgroups, else 64).  The query's slot table
// -- list start, list length, weight per slot, concatenated over the queries with an offset per query -- goes to LDS in
// PASSES of 64 slots.  Within a pass wave w takes entries w, w + 4, .. one at a time: lane l owns slot l of the pass and
// bisects its list's ascending doc_ids for d (plain 4-byte loads, at most 32 steps), loads the impact on a hit and forms the
// rounded product; the wave then folds the products of the lanes that hit in ASCENDING lane order = slot order into the
// entry's running sum, which lives in LDS (one writer: the entry's wave) and is carried into the next pass.
// No float atomics, one writer per output: the same bits from run to run.  Two 64-bit integer atomics per workgroup feed
// hipbm25_score_info: (valid entries << 32) + 1, and the bisections it ran (valid entry x slot with a non-empty list).
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): 26 VGPRs, no scratch, LDS 1824 bytes, 8 waves / SIMD.
// Bound: the latency of the dependent loads of a bisection (log2 of the list length round trips per slot pass).
// ------------------------------------------------------------------------------------------------------
constexpr int kSidThreads = 256;
constexpr int kSidMaxChunk = 64;            // entries per workgroup, at most: one wave reads the chunk's ids
constexpr int kSidMinChunk = 4;             // one entry per wave
constexpr int kSidPass = 64;                // slots per pass: one per lane
constexpr i64 kSidGridTarget = 4096;        // workgroups beyond which the chunk grows

struct SidSlot {      // one query-term slot: its posting list and its weight (16 bytes)
    unsigned long long lo;
    u32 len;
    float w;
};

struct SidArgs {
    const u32* doc_ids;
    const float* impacts;
    const SidSlot* slots;   // every slot of the call, query after query
    const int* qoff;        // [nq + 1]: query i owns slots qoff[i] .. qoff[i + 1] - 1
    const i64* ids;         // [nq, depth]
    float* out;             // [nq, depth]
    u64* counter;           // [0] (valid entries << 32) + workgroups, [1] bisections
    i64 n_docs, id_base;
    int depth, chunk, groups;   // groups = ceil(depth / chunk) workgroups per query
};

__global__ __launch_bounds__(kSidThreads) void bm25_score_ids_kernel(SidArgs a)
{
#pragma clang fp contract(off)
    constexpr int NW = kSidThreads / 64;
    __shared__ unsigned long long s_lo[kSidPass];
    __shared__ u32 s_len[kSidPass];
    __shared__ float s_w[kSidPass];
    __shared__ i64 rows[kSidMaxChunk];
    __shared__ float run[kSidMaxChunk];
    __shared__ u64 wprobes[NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = blockIdx.x / a.groups;
    const int j0 = (blockIdx.x - qi * a.groups) * a.chunk;
    const int cn = min(a.chunk, a.depth - j0);            // 1..chunk entries
    const int s_begin = a.qoff[qi], ns_all = a.qoff[qi + 1] - s_begin;
    int n_valid = 0;
    if (tid < 64) {
        i64 row = -1;
        if (tid < cn) {
            const i64 c = a.ids[(i64)qi * a.depth + j0 + tid];
            // c >= id_base makes the difference exact in unsigned arithmetic whatever the sign of id_base
            if (c >= 0 && c >= a.id_base && (u64)c - (u64)a.id_base < (u64)a.n_docs) row = (i64)((u64)c - (u64)a.id_base);
        }
        rows[tid] = row;
        run[tid] = 0.f;
        n_valid = __popcll(__ballot(row >= 0));
    }
    u64 probes = 0;                                       // this wave's bisections (wave-uniform)
    for (int s0 = 0; s0 < ns_all; s0 += kSidPass) {
        const int ns = min(ns_all - s0, kSidPass);
        __syncthreads();                                  // the pass before is read through (and rows / run are written)
        if (tid < ns) {
            const SidSlot sl = a.slots[s_begin + s0 + tid];
            s_lo[tid] = sl.lo;
            s_len[tid] = sl.len;
            s_w[tid] = sl.w;
        }
        __syncthreads();
        const u64 lo = lane < ns ? s_lo[lane] : 0ull;
        const u32 len = lane < ns ? s_len[lane] : 0u;     // an unknown term and a lane past the pass: an empty list
        const float w = lane < ns ? s_w[lane] : 0.f;
        const int n_lists = __popcll(__ballot(len != 0u));
        for (int j = wave; j < cn; j += NW) {
            const i64 row = rows[j];
            if (row < 0) continue;                        // padding (wave-uniform: every lane read the same word)
            const u32 d = (u32)row;                       // n_docs < 2^32
            // lower bound of d in doc_ids[lo, lo + len): the list is strictly ascending
            u32 x = 0, y = len;
            while (x < y) {
                const u32 m = x + ((y - x) >> 1);
                if (a.doc_ids[lo + m] < d) x = m + 1;
                else y = m;
            }
            bool hit = false;
            float prod = 0.f;
            if (x < len && a.doc_ids[lo + x] == d) {
                hit = true;
                prod = w * a.impacts[lo + x];             // rounded to fp32 here; the add below is a second rounding
            }
            unsigned long long mask = __ballot(hit);
            float acc = run[j];
            while (mask) {                                // ascending lanes = the query's slot order
                const int l = __builtin_ctzll(mask);
                acc = acc + __shfl(prod, l);
                mask &= mask - 1;
            }
            if (lane == 0) run[j] = acc;                  // the same wave reads it back in the next pass
            probes += (u64)n_lists;
        }
    }
    __syncthreads();                                      // a query without slots has passed no barrier yet
    for (int j = tid; j < cn; j += kSidThreads) a.out[(i64)qi * a.depth + j0 + j] = rows[j] >= 0 ? run[j] : -FLT_MAX;
    if (lane == 0) wprobes[wave] = probes;
    __syncthreads();
    if (tid == 0) {
        u64 p = 0;
        for (int w = 0; w < NW; ++w) p += wprobes[w];
        atomicAdd(a.counter, ((u64)n_valid << 32) | 1ull);
        atomicAdd(a.counter + 1, p);
    }
}

}  // namespace

// hipbm25_score_ids_dev under the handle's mutex (include/hiprag.h); the entry has run every check.  The slot table and the
// query offsets travel through the next stage of the pinned ring (Stage::slots / Stage::nslots), as a search's tables do.
int32_t Bm25Index::score_ids(const uint32_t* terms, const float* wts, const int32_t* qoff, int nq, const int64_t* ids_dev, int depth,
                             float* out_dev, hipStream_t st)
{
    int32_t rc;
    const size_t n_slots = (size_t)(qoff[nq] - qoff[0]);
    if ((rc = score_stat.reserve(16))) return rc;         // made once per handle
    if ((rc = sid_slots_dev.reserve(std::max<size_t>(1, n_slots) * sizeof(SidSlot)))) return rc;
    if ((rc = sid_qoff_dev.reserve((size_t)(nq + 1) * sizeof(int)))) return rc;
    if (prev_ev_set && prev_stream != st) HR_CHECK_HIP(hipStreamWaitEvent(st, prev_ev, 0));
    Stage& sg = stages[stage_next++ % kStages];
    if (sg.used) HR_CHECK_HIP(hipEventSynchronize(sg.ev));   // this buffer's previous copy (kStages calls ago) has left it
    if ((rc = sg.slots.reserve(std::max<size_t>(1, n_slots) * sizeof(SidSlot))) || (rc = sg.nslots.reserve((size_t)(nq + 1) * sizeof(int))))
        return rc;
    SidSlot* ps = sg.slots.as<SidSlot>();
    int* pq = sg.nslots.as<int>();
    for (int b = 0; b <= nq; ++b) pq[b] = qoff[b] - qoff[0];
    for (size_t i = 0; i < n_slots; ++i) {
        const uint32_t t = terms[(size_t)qoff[0] + i];
        SidSlot sl{0, 0, wts ? wts[(size_t)qoff[0] + i] : 1.0f};
        if ((i64)t < n_terms) { sl.lo = offsets[t]; sl.len = (u32)(offsets[t + 1] - offsets[t]); }   // unknown terms match nothing
        ps[i] = sl;
    }
    if (n_slots) HR_CHECK_HIP(hipMemcpyAsync(sid_slots_dev.p, ps, n_slots * sizeof(SidSlot), hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipMemcpyAsync(sid_qoff_dev.p, pq, (size_t)(nq + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (!sg.ev) HR_CHECK_HIP(hipEventCreateWithFlags(&sg.ev, hipEventDisableTiming));
    HR_CHECK_HIP(hipEventRecord(sg.ev, st));
    sg.used = true;
    HR_CHECK_HIP(hipMemsetAsync(score_stat.p, 0, 16, st));
    int chunk = kSidMinChunk;
    while (chunk < kSidMaxChunk && (i64)nq * ((depth + chunk - 1) / chunk) > kSidGridTarget) chunk *= 2;
    SidArgs a;
    a.doc_ids = doc_ids.as<u32>(); a.impacts = impacts.as<float>();
    a.slots = sid_slots_dev.as<SidSlot>(); a.qoff = sid_qoff_dev.as<int>();
    a.ids = reinterpret_cast<const i64*>(ids_dev); a.out = out_dev; a.counter = score_stat.as<u64>();
    a.n_docs = n_docs; a.id_base = id_base;
    a.depth = depth; a.chunk = chunk; a.groups = (depth + chunk - 1) / chunk;
    const i64 grid = (i64)nq * a.groups;                  // <= nq x depth < 2^31
    hipLaunchKernelGGL(bm25_score_ids_kernel, dim3((unsigned)grid), dim3(kSidThreads), 0, st, a);
    HR_CHECK_HIP(hipGetLastError());
    score_pairs = (i64)nq * depth;
    if (!prev_ev) HR_CHECK_HIP(hipEventCreateWithFlags(&prev_ev, hipEventDisableTiming));
    HR_CHECK_HIP(hipEventRecord(prev_ev, st));
    prev_ev_set = true;
    prev_stream = st;
    return HIPRAG_OK;
}

// every check of hipbm25_score_ids* but the handle's own, before anything is enqueued
static int32_t bm25_score_ids_check(const uint32_t* terms, const float* wts, const int32_t* qoff, int nq, const void* ids, int depth, const void* out)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(depth >= 1, "depth must be at least 1 (got %d)", depth);
    HR_REQUIRE((i64)nq * depth < (1ll << 31), "nq x depth = %lld pairs is beyond one call (2^31)", (long long)nq * depth);
    HR_REQUIRE(qoff, "q_offsets is null");
    HR_REQUIRE(ids, "ids is null");
    HR_REQUIRE(out, "out_scores is null");
    HR_REQUIRE(qoff[0] >= 0, "q_offsets must start >= 0");
    for (int b = 0; b < nq; ++b) HR_REQUIRE(qoff[b] <= qoff[b + 1], "q_offsets must be non-decreasing");
    HR_REQUIRE(terms || qoff[nq] == qoff[0], "term_ids is null");
    if (wts)
        for (int32_t i = qoff[0]; i < qoff[nq]; ++i)
            HR_REQUIRE(std::isfinite(wts[i]) && wts[i] > 0.f, "term_weights[%d] = %g: every weight must be finite and > 0 (drop terms of weight zero)",
                       i, (double)wts[i]);
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

// The sparse scores of the documents `ids_dev` names, for every query (include/hiprag.h).
int32_t hipbm25_score_ids_dev(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host, const int32_t* q_offsets_host,
                              int32_t nq, const int64_t* ids_dev, int32_t depth, float* out_scores_dev, void* stream)
{
    GET_BM25(h);
    BM25_REQUIRE_CLEAN(ix);
    const int32_t rc = bm25_score_ids_check(term_ids_host, term_weights_host, q_offsets_host, nq, ids_dev, depth, out_scores_dev);
    if (rc) return rc;
    return ix->score_ids(term_ids_host, term_weights_host, q_offsets_host, nq, ids_dev, depth, out_scores_dev, (hipStream_t)stream);
}

int32_t hipbm25_score_ids(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host, const int32_t* q_offsets_host,
                          int32_t nq, const int64_t* ids_host, int32_t depth, float* out_scores)
{
    GET_BM25(h);
    BM25_REQUIRE_CLEAN(ix);
    int32_t rc;
    if ((rc = bm25_score_ids_check(term_ids_host, term_weights_host, q_offsets_host, nq, ids_host, depth, out_scores))) return rc;
    const size_t n = (size_t)nq * depth;
    if ((rc = ix->oid.reserve(n * sizeof(i64))) || (rc = ix->o32.reserve(n * sizeof(float)))) return rc;
    HR_CHECK_HIP(hipMemcpy(ix->oid.p, ids_host, n * sizeof(i64), hipMemcpyHostToDevice));
    if ((rc = ix->score_ids(term_ids_host, term_weights_host, q_offsets_host, nq, ix->oid.as<int64_t>(), depth, ix->o32.as<float>(), nullptr)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(out_scores, ix->o32.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// { valid entries, padding entries, workgroups launched, bisections } of the last hipbm25_score_ids* call; synchronises
int32_t hipbm25_score_info(uint64_t h, int64_t* out4)
{
    GET_BM25(h);
    HR_REQUIRE(out4, "out4 is null");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (ix->score_stat.p) {
        unsigned long long word[2] = {0, 0};
        HR_CHECK_HIP(hipDeviceSynchronize());
        HR_CHECK_HIP(hipMemcpy(word, ix->score_stat.p, 16, hipMemcpyDeviceToHost));
        out4[0] = (int64_t)(word[0] >> 32);
        out4[1] = ix->score_pairs - out4[0];
        out4[2] = (int64_t)(word[0] & 0xFFFFFFFFull);
        out4[3] = (int64_t)word[1];
    }
    return HIPRAG_OK;
}

}  // extern "C"
