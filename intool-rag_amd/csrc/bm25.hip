// bm25.hip -- BM25 term-at-a-time (TAAT) sparse scoring on MI355X.
//
// The reference names hybrid BM25 search (README.md:54-58; rag/config.py:43-45 HYBRID_SEARCH_ENABLED / BM25_WEIGHT)
// but contains no implementation; the specification is restated in oracle/hybrid_oracle.py (bm25_impacts,
// bm25_scores_taat) and DESIGN.md.  Determinism rule: the host precomputes one fp32 IMPACT per posting
// (idf * tf-normalisation, fp64 -> fp32 once); the GPU only performs acc[doc] += impact, one query-term slot per
// kernel launch, in query order.  A document occurs at most once in a posting list, so a slot needs no atomics and
// the fp32 sum of every document is formed in exactly the oracle's order.
//
// Layout: CSR postings in HBM as two SoA streams (doc_ids u32, impacts f32) -- 8 B per posting, read once per use,
// coalesced 16 B per lane; accumulators acc[query][doc] fp32 stay L2 / Infinity-Cache resident (4 MB per query per
// 1M docs).  Bound: HBM (posting streams) + the accumulator zero/select passes; bytes reported by hipbm25_get_stats.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bm25_internal.h"
#include "scope_plan.h"

namespace hiprag {
namespace {

constexpr int kBatch = kBm25Batch;  // queries scored concurrently
constexpr int kTaatThreads = 256;
constexpr int kTaatPerThread = 8;     // postings per thread
constexpr int kTaatChunk = kTaatThreads * kTaatPerThread;
constexpr int kMaxK = 1000;

struct SlotRange {  // posting range of one (query, term slot)
    unsigned long long lo, hi;
};

// One weighted step of a document's sum (hipbm25_search_weighted): the product is rounded to fp32, then added -- two
// roundings, never a fused multiply-add, so that numpy's `acc + w * impact` in fp32 gives the same bits.  Spelled with the
// operators under contract(off): __fmul_rn / __fadd_rn are plain inline `x * y` / `x + y` here, carry their own header's
// contraction default into the caller and came out as one v_fma_f32.
__device__ __forceinline__ float weighted_add(float acc, float w, float impact)
{
#pragma clang fp contract(off)
    const float p = w * impact;
    return acc + p;
}

// grid (chunks, nq): chunk c of query b's posting list for this slot.  WEIGHTED: wts[b] is the slot's query weight, which
// travels beside ranges[b] (the unweighted instantiation never looks at the pointer).
template <bool WEIGHTED>
__global__ __launch_bounds__(kTaatThreads) void taat_kernel(const u32* __restrict__ doc_ids, const float* __restrict__ impacts,
                                                           const SlotRange* __restrict__ ranges, float* __restrict__ acc,
                                                           i64 n_docs, const float* __restrict__ wts)
{
    const int b = blockIdx.y;
    const SlotRange r = ranges[b];
    const u64 start = r.lo + (u64)blockIdx.x * kTaatChunk;
    if (start >= r.hi) return;
    float* accb = acc + (i64)b * n_docs;  // n_docs here is the padded row stride
    // strided by thread so that each load instruction is a contiguous 1 KiB (u32/f32 x 256 threads).  A document
    // occurs at most once in a posting list, so the eight read-modify-writes of a thread never alias: all eight
    // accumulator loads go out together (written as three separate loops -- left as acc[d] += x the compiler must assume
    // aliasing and serialises eight L2 round trips per thread, which made the kernel latency-bound at ~1 TB/s).
    u32 d[kTaatPerThread];
    float im[kTaatPerThread], a[kTaatPerThread];
#pragma unroll
    for (int j = 0; j < kTaatPerThread; ++j) {
        const u64 i = start + (u64)j * kTaatThreads + threadIdx.x;
        const bool ok = i < r.hi;
        d[j] = ok ? doc_ids[i] : 0xFFFFFFFFu;
        im[j] = ok ? impacts[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kTaatPerThread; ++j) a[j] = d[j] != 0xFFFFFFFFu ? accb[d[j]] : 0.f;
#pragma unroll
    for (int j = 0; j < kTaatPerThread; ++j)
        if (d[j] != 0xFFFFFFFFu) {
            if constexpr (WEIGHTED) accb[d[j]] = weighted_add(a[j], wts[b], im[j]);
            else accb[d[j]] = a[j] + im[j];
        }
}

// ---------------------------------------------------------------------------------------------------------
// Tiled TAAT (the default path, k <= 64): one workgroup per (document tile, query) keeps the tile's fp32 accumulators in
// LDS (9216 documents = 36 KiB: FOUR workgroups per CU.  A workgroup spends its ~17 us mostly waiting -- six term slots x
// (barrier + LDS read-modify-write round trip), then the pass over the accumulators -- so workgroups per CU are the lever:
// 16384-document tiles (two per CU) 370 k queries/s at 1M documents, 12288 (three) 400-418 k, 9216 (four) 411-417 k, 8192
// (four, more tiles) 398 k; 13312 fit three on paper only), walks the query's term slots IN ORDER -- for each slot it streams only the postings
// whose document falls into the tile -- and then selects the tile's top-k straight out of LDS.  HBM traffic is the posting
// streams alone: no accumulator array to zero, scatter into and scan again (the global-accumulator form below moves
// 8 B per posting plus up to two 128-B lines per touched accumulator through L2, and ran at ~1.2 TB/s).
// Where a list's tile range starts comes from a SKIP TABLE built at create time for every list with >= kSkipMinDf
// postings (the posting offset at each tile boundary, u32 relative to the list start, (ntiles + 1) entries); shorter
// lists are read whole by every tile and filtered -- 109 tiles x < 2048 postings costs less than a table lookup chain.
// Determinism: a document occurs at most once per list, so within a slot no two threads touch the same accumulator and
// the barrier between slots keeps every document's fp32 sum in query-term order, exactly the oracle's.
// Selection: grid (nq, ntiles), queries fastest.  Two bounds per query, zeroed per launch: hist[q] (score histogram of the
// documents emitted so far, see the kernel) and theta[q], which carries the best K-th score any finished
// wave of query q has published, as order-preserving u32 bits; a wave whose own maximum is below it emits nothing, one
// with few survivors above it skips the threshold bisection.  A bound is only ever a score K documents already reached,
// so dropping what lies strictly below it cannot change the merged top-k (ties at the bound are kept).
// ---------------------------------------------------------------------------------------------------------
constexpr int kTileThreads = 256;   // workgroup of the tiled kernel
constexpr int kTileWaves = kTileThreads / 64;
constexpr int kHistBuckets = 2048;  // score buckets of the per-query bound histogram (+ 1 word: highest bucket used)
constexpr int kMaxSlots = 64;      // query terms the tiled kernel takes (longer queries use the global-accumulator form)

struct TileSlot {   // posting range of one (query, term slot); skip = first entry of the list's skip table or -1
    unsigned long long lo, hi;
    long long skip;
};

// SCOPED form (hipbm25_search_scoped_dev): the launch is a LIST OF WORK ITEMS, one per (query, tile that holds at least one
// document of the query's scope), so a query costs as many workgroups as its scope touches tiles.  An item names the
// ranges of the scope that meet its tile; the accumulators of the documents BETWEEN them (and before the first, after the
// last) are cleared in LDS once the stream is through and before anything is selected, so a document outside the scope is
// never emitted, never counted in theta / hist and never holds a slot of a wave's list -- the per-document fp32 sums of
// the others are untouched.  The streaming loop is the unscoped one, instruction for instruction (it is issue-bound: no
// per-posting look at the range table); the tile's running maximum stays a bound over ALL its documents, which only makes
// the "whole tile below the bound" shortcut fire less often.  Items are ordered position-in-scope major, queries fastest,
// which keeps the bound sharing of the (nq, ntiles) grid; the candidate lists are [query][position j of the tile in the
// query's scope][wave][K1], positions past a query's last tile prefilled as padding by scoped_pad_kernel.  Queries of any
// length: the slots are walked in batches of kMaxSlots with the accumulators staying in LDS, a barrier between batches.
struct ScopedItem {   // one workgroup of the scoped launch
    int q, tile, j;   // query (within the chunk), document tile, position of the tile among the tiles of the query's scope
    int r0, r1;       // ranges [r0, r1) of the range table: those of the scope that meet the tile (empty ones between them too)
};
struct ScopeArgs {
    const ScopedItem* items;
    const uint2* ranges;   // every range of the call as (lo, hi), local document ids
    int max_tiles;         // tiles of the largest scope of the chunk = list positions per query
};

// IDX32: fewer than 2^30 postings in all, so posting indices and their byte offsets fit 32 bits -- the stream's index
// arithmetic (a third of its instructions as 64-bit adds, compares and selects) becomes single 32-bit operations.
// WEIGHTED (hipbm25_search_weighted*): slot_w[q][slot] is the query's weight of the slot, laid out like `slots`; a batch's
// weights sit in LDS beside ra / rb and the accumulate step multiplies the impact by its slot's weight first.  Weights are
// positive (checked by the entry), so every contribution still is, and wmax / theta / hist bound what they bounded.
template <bool IDX32, bool SCOPED, bool WEIGHTED>
__global__ __launch_bounds__(kTileThreads) void taat_tile_kernel(const u32* __restrict__ doc_ids, const float* __restrict__ impacts,
                                                        const TileSlot* __restrict__ slots, const int* __restrict__ nslots,
                                                        const u32* __restrict__ skip, int max_slots, i64 n_docs, int K1,
                                                        u64* __restrict__ ck, i64* __restrict__ ci, u32* __restrict__ theta,
                                                        u32* __restrict__ hist, ScopeArgs sc, const float* __restrict__ slot_w)
{
    extern __shared__ float tacc[];  // kTileDocs accumulators
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // queries fastest: the tiles of one query are spread over the whole launch, so the bound its early tiles publish
    // (theta, below) is there when the later ones select; neighbours in time share a tile's postings of common terms
    int q = blockIdx.x, tile = blockIdx.y;
    i64 list0;               // this workgroup's place among the candidate lists: (list0 * kTileWaves + wave) * K1
    ScopedItem item{};
    if constexpr (SCOPED) {
        item = sc.items[blockIdx.x];
        q = item.q;
        tile = item.tile;
        list0 = (i64)q * sc.max_tiles + item.j;
    } else {
        list0 = (i64)q * gridDim.y + tile;
    }
    const u32 tlo = (u32)tile * kTileDocs;
    const u32 tlen = (u32)min((i64)kTileDocs, n_docs - (i64)tlo);
    // posting ranges of this tile for every slot, resolved up front (slot descriptor -> skip table is a chain of two
    // dependent global loads; done per slot inside the loop it cost ~4 us of latency six times per workgroup)
    __shared__ unsigned long long ra[kMaxSlots], rb[kMaxSlots];
    __shared__ float rw[WEIGHTED ? kMaxSlots : 1];
    const int ns_all = SCOPED ? nslots[q] : min(nslots[q], kMaxSlots);
    for (int i = tid; i < kTileDocs / 4; i += kTileThreads) reinterpret_cast<float4*>(tacc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    float wmax = 0.f;
    const int nbatches = SCOPED ? (ns_all + kMaxSlots - 1) / kMaxSlots : 1;   // unscoped: one batch, longer queries go elsewhere
    for (int bt = 0; bt < nbatches; ++bt) {
    const int s0 = bt * kMaxSlots;
    const int ns = min(ns_all - s0, kMaxSlots);
    if (SCOPED && bt) __syncthreads();   // every thread is through with the previous batch's ra / rb
    if (tid < ns) {
        const TileSlot sl = slots[(i64)q * max_slots + s0 + tid];
        u64 a = sl.lo, b = sl.hi;
        if (sl.skip >= 0) {
            a = sl.lo + skip[sl.skip + tile];
            b = sl.lo + skip[sl.skip + tile + 1];
        }
        ra[tid] = a;
        rb[tid] = b;
        if constexpr (WEIGHTED) rw[tid] = slot_w[(i64)q * max_slots + s0 + tid];
    }
    __syncthreads();
    // The slots form ONE stream of 2048-posting chunks: the loads of the next chunks -- of the same slot or of the next
    // ones -- are in flight while this chunk's accumulator updates run; a workgroup barrier separates slots only.
    constexpr int U = 2048 / kTileThreads;
    constexpr u64 CH = (u64)U * kTileThreads;
    // Loads are UNCONDITIONAL (lanes past the end of a range read posting 0, the buffers never have fewer than four
    // entries) and nothing touches the loaded values before the accumulate step: a load behind a lane mask or a
    // branch is compiled into branch + load + wait, i.e. one memory round trip per posting (this loop used to spend
    // 16 us per workgroup that way), and it makes the number of loads in flight unknown where the paths join.
    auto fetch = [&](u64 i0, u64 b, u32 (&d)[U], float (&im)[U]) {
#pragma unroll
        for (int j = 0; j < U; ++j) {   // eight independent 1 KiB-per-instruction loads of each stream
            if (IDX32) {
                const u32 i = (u32)i0 + (u32)j * (u32)kTileThreads + (u32)tid;
                const u32 ic = i < (u32)b ? i : 0u;
                d[j] = doc_ids[ic];
                im[j] = impacts[ic];
            } else {
                const u64 i = i0 + (u64)j * kTileThreads + tid;
                const u64 ic = i < b ? i : 0;
                d[j] = doc_ids[ic];
                im[j] = impacts[ic];
            }
        }
    };
    int cs = 0;              // cursor: next chunk to fetch = [cpos, ..) of slot cs
    u64 cpos = ns > 0 ? ra[0] : 0;
    auto next_chunk = [&](int& slot, u64& pos, u64& bound) -> bool {
        while (cs < ns && cpos >= rb[cs]) { ++cs; if (cs < ns) cpos = ra[cs]; }
        if (cs >= ns) { pos = 0; bound = 0; return false; }
        slot = cs; pos = cpos; bound = rb[cs];
        cpos += CH;
        return true;
    };
    // D chunks in flight (a tile's share of a list is usually one or two chunks, so this is "the next slots are already
    // on their way")
    constexpr int D = 4;
    u32 dR[D][U];
    float mR[D][U];
    int sR[D];
    bool hR[D];
    u64 pR[D], bR[D];
#pragma unroll
    for (int r = 0; r < D; ++r) {
        sR[r] = 0;
        hR[r] = next_chunk(sR[r], pR[r], bR[r]);
        fetch(pR[r], bR[r], dR[r], mR[r]);
    }
    while (hR[0]) {
#pragma unroll
        for (int r = 0; r < D; ++r) {
            if (!hR[r]) break;   // chunks are handed out in order: the first empty ring entry ends the stream
            // a chunk lies inside one list, so its documents are distinct: read all eight accumulators, then write
            // them (as `+=` the compiler must assume aliasing and runs eight dependent LDS round trips)
            u32 dd[U];
            float cur[U];
            float sw = 1.f;
            if constexpr (WEIGHTED) sw = rw[sR[r]];   // a chunk lies inside one slot
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const u32 x = dR[r][j] - tlo;
                const bool inr = IDX32 ? ((u32)pR[r] + (u32)j * (u32)kTileThreads + (u32)tid < (u32)bR[r])
                                       : (pR[r] + (u64)j * kTileThreads + tid < bR[r]);
                dd[j] = (inr && x < tlen) ? x : 0xFFFFFFFFu;
                cur[j] = tacc[dd[j] != 0xFFFFFFFFu ? dd[j] : 0u];
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                if (dd[j] != 0xFFFFFFFFu) {
                    float nv;
                    if constexpr (WEIGHTED) nv = weighted_add(cur[j], sw, mR[r][j]);
                    else nv = cur[j] + mR[r][j];
                    tacc[dd[j]] = nv;
                    wmax = fmaxf(wmax, nv);   // impacts are positive: the largest value ever written is the tile's best final score
                }
            }
            const int nr = (r + 1) % D;              // the chunk that follows in stream order (static after unrolling)
            const bool boundary = !hR[nr] || sR[nr] != sR[r];
            hR[r] = next_chunk(sR[r], pR[r], bR[r]); // re-arm this entry before the barrier: its loads fly through it
            fetch(pR[r], bR[r], dR[r], mR[r]);
            if (boundary) __syncthreads();           // slot boundary: later slots add to the same documents
        }
    }
    }   // slot batches
    if constexpr (SCOPED) {
        // the mask: wave w clears gaps w, w + 4, .. -- gap g lies between range r0 + g - 1 and range r0 + g of the item, the
        // first starts at the tile's first document, the last ends at its last.  Bounds are clamped to the tile, so whatever
        // the table holds nothing outside the tile's accumulators is written.
        __syncthreads();   // a query without slots has passed no barrier since the accumulators were zeroed
        const u32 tend = tlo + tlen;
        const int nr = item.r1 - item.r0;
        for (int g = wv; g <= nr; g += kTileWaves) {
            u32 a = g == 0 ? tlo : sc.ranges[item.r0 + g - 1].y;
            u32 b = g == nr ? tend : sc.ranges[item.r0 + g].x;
            a = min(max(a, tlo), tend) - tlo;
            b = min(max(b, tlo), tend) - tlo;
            for (u32 i = a + (u32)lane; i < b; i += 64u) tacc[i] = 0.f;
        }
    }
    __shared__ float smax[kTileWaves];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, off));
    if (lane == 0) smax[wv] = wmax;
    __syncthreads();
    float tile_top = 0.f;
#pragma unroll
    for (int w = 0; w < kTileWaves; ++w) tile_top = fmaxf(tile_top, smax[w]);
    // ---- tile top-K1 out of LDS: wave w filters accumulators [4096 w, 4096 (w + 1)) like select_wave_kernel<true> ----
    // theta[q] = the best K1-th score any finished wave of this query has published (ordered-integer form, grows
    // monotonically): a lower bound of the query's final K1-th score, so nothing below it can reach the result.  The
    // first tiles of a query pay the full selection; later ones start from a threshold that is already almost final
    // and keep only a handful of documents.  Which tiles profit depends on timing, the merged top-k does not.
    u32 th = __hip_atomic_load(theta + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // A second, much tighter bound: hist[q] counts the documents every finished wave of this query has emitted, by score
    // bucket (sign-free float bits >> 20: exponent and three mantissa bits, 12.5 % wide); hist[q][kHistBuckets] is the
    // highest bucket used.  If the buckets from b upwards hold K1 documents, K1 documents score at least b's lower edge.
    // theta alone is the best K1-th score of ONE wave's 2304 documents -- about the 10,000th best of 1M -- and left every
    // wave ~50 survivors to compact and rank (and often a bisection first); this bound follows the query's true K1-th
    // score to within a bucket after the first few tiles and leaves most waves none.
    if (hist) {
        const u32* hq = hist + (size_t)q * (kHistBuckets + 1);
        const u32 hm = __hip_atomic_load(hq + kHistBuckets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hm != 0) {
            const int b = (int)hm - 63 + lane;   // lanes cover the 64 buckets up to the highest one: a factor 256 in score
            u32 suffix = b > 0 ? __hip_atomic_load(hq + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u32 up = (u32)__shfl_down((int)suffix, off);
                if (lane + off < 64) suffix += up;
            }
            const unsigned long long okm = __ballot(suffix >= (u32)K1);
            if (okm) {
                const int l = 63 - __builtin_clzll(okm);
                const u32 hb = 0x80000000u | ((u32)((int)hm - 63 + l) << 20);   // ord32 image of the bucket's lower edge
                th = hb > th ? hb : th;
            }
        }
    }
    // the whole tile is below the bound: no pass over the accumulators at all (about 40 % of the tiles once the bound has
    // converged -- a query's best ~100 documents leave that share of its 109 tiles without any of them)
    if (th != 0 && (!(tile_top > 0.f) || th > ord32(tile_top))) {
        const i64 o0 = (list0 * kTileWaves + wv) * K1;
        if (lane < K1) { ck[o0 + lane] = 0; ci[o0 + lane] = -1; }
        return;
    }
    constexpr int NV = kTileDocs / (kTileWaves * 256);   // float4 per lane: a wave filters its share of the tile
    float v[NV * 4];
#pragma unroll
    for (int it = 0; it < NV; ++it) {
        const float4 x = reinterpret_cast<const float4*>(tacc)[wv * (kTileDocs / kTileWaves / 4) + it * 64 + lane];
        v[it * 4 + 0] = x.x; v[it * 4 + 1] = x.y; v[it * 4 + 2] = x.z; v[it * 4 + 3] = x.w;
    }
    float m = -INFINITY;
#pragma unroll
    for (int n = 0; n < NV * 4; ++n) m = fmaxf(m, v[n] > 0.f ? v[n] : -INFINITY);
    const u32 mo = m == -INFINITY ? 0u : ord32(m);
    u32 best = 0;
    u32 top = mo;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) top = max(top, (u32)__shfl_xor((int)top, off));
#pragma unroll
    for (int n = 0; n < NV * 4; ++n) v[n] = v[n] > 0.f ? v[n] : -INFINITY;
    if (th != 0 && th > top) {
        best = th;                       // nothing in this wave's range can reach the result
    } else if (th != 0) {
        const float tf = unord32(th);
        int c = 0;
#pragma unroll
        for (int n = 0; n < NV * 4; ++n) c += __popcll(__ballot(v[n] >= tf));
        best = c > K1 + (K1 >> 1) ? wave_bisect_threshold(v, th, top + 1, K1, 10) : th;
    } else {
        for (int j = 0; j < 64; ++j) {
            const u32 mj = (u32)__builtin_amdgcn_readlane((int)mo, j);
            const int cnt = __popcll(__ballot(mo >= mj));
            if (mj != 0 && cnt >= K1 && mj > best) best = mj;
        }
        if (best) best = wave_bisect_threshold(v, best, top + 1, K1, 10);
    }
    // Survivors: positive accumulators at or above the threshold.  When there are at most 128 of them (the bisection
    // aims at K1 .. 1.5 K1, a bound inherited from other tiles leaves fewer) they are COMPACTED into this wave's own
    // quarter of the tile (its accumulators are in registers by now; no other wave reads that quarter) and RANKED --
    // every lane counts the keys above its own one or two, keys are unique (score bits | document), so rank = final
    // position: ~64 ballots + ~m broadcast reads instead of 64 conditional serial inserts into a sorted wave list.
    const float thrf = best ? unord32(best) : 0.f;
    const i64 o = (list0 * kTileWaves + wv) * K1;
    if (tlen < (u32)kTileDocs) {   // last, partial tile only: accumulators past the end of the collection never count
#pragma unroll
        for (int n = 0; n < NV * 4; ++n) {
            const u32 local = (u32)wv * (u32)(kTileDocs / kTileWaves) + (u32)(n >> 2) * 256u + (u32)lane * 4u + (u32)(n & 3);
            if (local >= tlen) v[n] = -INFINITY;
        }
    }
    // one pass: a survivor (v >= threshold; non-positive accumulators are -inf by now) is rare -- ~75 of a wave's 4096 --
    // so most of the 64 steps are one compare and one scalar branch
    u64* comp = reinterpret_cast<u64*>(tacc + wv * (kTileDocs / kTileWaves));
    int ms = 0;
#pragma unroll
    for (int n = 0; n < NV * 4; ++n) {
        const bool keep = v[n] >= thrf;
        const unsigned long long mask = __ballot(keep);
        if (mask) {
            if (keep) {
                const int pos = ms + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                const u32 local = (u32)wv * (u32)(kTileDocs / kTileWaves) + (u32)(n >> 2) * 256u + (u32)lane * 4u + (u32)(n & 3);
                if (pos < 128) comp[pos] = pack_key(v[n], tlo + local);
            }
            ms += __popcll(mask);
        }
    }
    if (ms <= 128) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's LDS writes are done before it reads them back
        const u64 k0 = lane < ms ? comp[lane] : 0ull, k1 = 64 + lane < ms ? comp[64 + lane] : 0ull;
        int r0 = 0, r1 = 0;
#pragma unroll 4
        for (int j = 0; j < ms; ++j) {
            const u64 kj = comp[j];   // same address in every lane: an LDS broadcast
            r0 += kj > k0;
            r1 += kj > k1;
        }
        if (lane < K1 && lane >= ms) { ck[o + lane] = 0; ci[o + lane] = -1; }
        if (k0 != 0 && r0 < K1) { ck[o + r0] = k0 & 0xFFFFFFFF00000000ull; ci[o + r0] = (i64)packed_index(k0); }
        if (k1 != 0 && r1 < K1) { ck[o + r1] = k1 & 0xFFFFFFFF00000000ull; ci[o + r1] = (i64)packed_index(k1); }
        if (hist) {
            u32* hq = hist + (size_t)q * (kHistBuckets + 1);
            u32 bmax = 0;
            if (k0 != 0 && r0 < K1) { const u32 b = ((u32)(k0 >> 32) >> 20) & (kHistBuckets - 1); atomicAdd(hq + b, 1u); bmax = b; }
            if (k1 != 0 && r1 < K1) { const u32 b = ((u32)(k1 >> 32) >> 20) & (kHistBuckets - 1); atomicAdd(hq + b, 1u); bmax = max(bmax, b); }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) bmax = max(bmax, (u32)__shfl_xor((int)bmax, off));
            if (lane == 0 && bmax != 0) atomicMax(hq + kHistBuckets, bmax);
        }
        // this wave holds K1 documents at or above the key of rank K1 - 1: publish the bound
        if (k0 != 0 && r0 == K1 - 1) atomicMax(theta + q, (u32)(k0 >> 32));
        if (k1 != 0 && r1 == K1 - 1) atomicMax(theta + q, (u32)(k1 >> 32));
    } else {
        WaveListPacked L;
        L.init();
        u64 tau = best ? ((u64)best << 32) - 1 : 0;
#pragma unroll
        for (int n = 0; n < NV * 4; ++n) {
            const u32 local = (u32)wv * (u32)(kTileDocs / kTileWaves) + (u32)(n >> 2) * 256u + (u32)lane * 4u + (u32)(n & 3);
            u64 c = 0;
            if (v[n] > 0.f && local < tlen) c = pack_key(v[n], tlo + local);
            tau = L.offer(c, K1, tau);
        }
        if (lane < K1) {
            ck[o + lane] = L.e & 0xFFFFFFFF00000000ull;
            ci[o + lane] = L.e ? (i64)packed_index(L.e) : -1;
        }
        if (hist) {
            u32* hq = hist + (size_t)q * (kHistBuckets + 1);
            u32 bmax = 0;
            if (lane < K1 && L.e != 0) { const u32 b = ((u32)(L.e >> 32) >> 20) & (kHistBuckets - 1); atomicAdd(hq + b, 1u); bmax = b; }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) bmax = max(bmax, (u32)__shfl_xor((int)bmax, off));
            if (lane == 0 && bmax != 0) atomicMax(hq + kHistBuckets, bmax);
        }
        const u64 kth = L.kth(K1);   // this wave holds K1 documents at or above it: publish the bound
        if (lane == 0 && kth != 0) atomicMax(theta + q, (u32)(kth >> 32));
    }
}

// scoped launch: the list positions a query does not use (its scope has fewer tiles than the chunk's largest) are padding
__global__ __launch_bounds__(256) void scoped_pad_kernel(const int* __restrict__ qtiles, int max_tiles, int K1, u64* __restrict__ ck,
                                                         i64* __restrict__ ci)
{
    const int q = blockIdx.x;
    const i64 per_q = (i64)max_tiles * kTileWaves * K1;
    for (i64 i = (i64)qtiles[q] * kTileWaves * K1 + threadIdx.x; i < per_q; i += 256) {
        ck[(i64)q * per_q + i] = 0;
        ci[(i64)q * per_q + i] = -1;
    }
}

struct FinishArgs {
    const u64* ck;
    const i64* ci;
    double* out64;
    float* out32;
    i64* out_ids;
    i64 ncand, id_base;
    int k;
};

__global__ __launch_bounds__(256) void bm25_finish_kernel(FinishArgs a)
{
    extern __shared__ unsigned char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    i64* ids = reinterpret_cast<i64*>(keys + kTile);
    u64* selk = reinterpret_cast<u64*>(ids + kTile);
    i64* seli = reinterpret_cast<i64*>(selk + a.k);
    KeyId* red = reinterpret_cast<KeyId*>(seli + a.k);
    const int q = blockIdx.x;
    const u64* sk = a.ck + (i64)q * a.ncand;
    const i64* si = a.ci + (i64)q * a.ncand;
    wg_stream_topk<256>([&](i64 i, u64& k, i64& id) { k = sk[i]; id = si[i]; }, a.ncand, a.k, keys, ids, red, selk, seli);
    for (int r = threadIdx.x; r < a.k; r += 256) {
        const i64 o = (i64)q * a.k + r;
        const u64 k = selk[r];
        const float s = k ? unord32((u32)(k >> 32)) : -FLT_MAX;
        if (a.out64) a.out64[o] = k ? (double)s : -DBL_MAX;
        if (a.out32) a.out32[o] = s;
        a.out_ids[o] = k ? seli[r] + a.id_base : -1;
    }
}

// the one place that names the eight instantiations of the tiled kernel: the launch sites and set_tile_lds() select here
using TileKernel = decltype(&taat_tile_kernel<true, false, false>);
TileKernel tile_kernel(bool idx32, bool scoped, bool weighted)
{
    static const TileKernel ks[2][2][2] = {
        {{taat_tile_kernel<false, false, false>, taat_tile_kernel<false, false, true>},
         {taat_tile_kernel<false, true, false>, taat_tile_kernel<false, true, true>}},
        {{taat_tile_kernel<true, false, false>, taat_tile_kernel<true, false, true>},
         {taat_tile_kernel<true, true, false>, taat_tile_kernel<true, true, true>}}};
    return ks[idx32][scoped][weighted];
}

}  // namespace

struct Bm25Index::TileLaunch {
    int max_slots;        // slots per query of the slot table = the longest query of the launch
    TileKernel kernel;
};

int32_t Bm25Index::reserve(int k)
{
    int32_t rc;
    if ((rc = acc.reserve((size_t)kBatch * stride() * sizeof(float)))) return rc;
    if (k > ws_k) {
        const i64 per_q = std::max(nchunks(), nlists());
        if ((rc = ck.reserve((size_t)kBatch * per_q * k * sizeof(u64)))) return rc;
        if ((rc = ci.reserve((size_t)kBatch * per_q * k * sizeof(i64)))) return rc;
        ws_k = k;
    }
    return HIPRAG_OK;
}

// the merge behind a tiled launch: wave_cand candidates per query in ck / ci -> the query's top k
void Bm25Index::launch_merge(i64 wave_cand, int nq, int k, double* o64p, float* o32p, i64* oidp, hipStream_t st)
{
    const i64 per_lane = (wave_cand + 1023) / 1024;
    auto mk = merge_packed_loop_kernel<8>;   // any size
    if (per_lane <= 16) mk = merge_packed_kernel<16>;
    if (per_lane <= 1) mk = merge_packed_kernel<1>;
    else if (per_lane <= 2) mk = merge_packed_kernel<2>;
    else if (per_lane <= 4) mk = merge_packed_kernel<4>;
    else if (per_lane <= 8) mk = merge_packed_kernel<8>;
    hipLaunchKernelGGL(mk, dim3(nq), dim3(1024), 0, st, (const u64*)ck.as<u64>(), (const i64*)ci.as<i64>(), wave_cand, k, id_base,
                       o64p, o32p, oidp);
}

int32_t Bm25Index::set_tile_lds()
{
    static bool lds_ok = false;
    if (lds_ok) return HIPRAG_OK;
    for (int i = 0; i < 8; ++i)   // all eight instantiations
        HR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tile_kernel(i & 4, i & 2, i & 1)),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, kTileDocs * (int)sizeof(float)));
    lds_ok = true;
    return HIPRAG_OK;
}

// The front half of a tiled launch over queries [q0, q0 + m) of a call, the same for both forms: takes the next stage of
// the pinned ring, reserves every buffer of the launch (`lists` candidate lists per query), fills the slot table, the slot
// counts and the slot weights, enqueues their copies, records the stage's event and zeroes theta / hist.  A scoped launch
// has image_words > 0: fill_image(words) writes that many 4-byte words into the stage's `scoped` buffer, and they are copied
// to scoped_dev AHEAD of the event, which guards every pinned buffer of the stage.  On the stream: the copies (weights,
// slots, counts, image), the event, the two memsets; the caller's kernels follow.
// Statistics: both forms count postings_touched, the unscoped form alone counts 8 bytes per posting in bytes_alg (and
// nq * n_docs * 8 in search_tiled), the scoped form adds nothing to bytes_alg.  That is how the two grew, and
// hipbm25_get_stats keeps reporting it so.
template <class FillImage>
int32_t Bm25Index::plan_tiles(const Bm25Call& c, int q0, int m, i64 lists, size_t image_words, FillImage fill_image, TileLaunch& tl)
{
    int32_t rc;
    const int32_t* qoff = c.qoff + q0;
    const bool scoped = image_words != 0;
    int max_slots = 1;
    for (int b = 0; b < m; ++b) max_slots = std::max(max_slots, qoff[b + 1] - qoff[b]);
    Stage& sg = stages[stage_next++ % kStages];
    if (sg.used) HR_CHECK_HIP(hipEventSynchronize(sg.ev));   // this buffer's previous copy (kStages calls ago) has left it
    const size_t n_slots = (size_t)m * max_slots, hbytes = (size_t)m * (kHistBuckets + 1) * sizeof(u32);
    if ((rc = sg.slots.reserve(n_slots * sizeof(TileSlot))) || (rc = slots_dev.reserve(n_slots * sizeof(TileSlot)))) return rc;
    if ((rc = sg.nslots.reserve((size_t)m * sizeof(int))) || (rc = nslots_dev.reserve((size_t)m * sizeof(int)))) return rc;
    if (c.wts && ((rc = sg.wts.reserve(n_slots * sizeof(float))) || (rc = wts_dev.reserve(n_slots * sizeof(float))))) return rc;
    if (scoped && ((rc = sg.scoped.reserve(image_words * 4)) || (rc = scoped_dev.reserve(image_words * 4)))) return rc;
    if ((rc = ck.reserve((size_t)m * lists * c.k * sizeof(u64))) || (rc = ci.reserve((size_t)m * lists * c.k * sizeof(i64)))) return rc;
    if ((rc = theta_dev.reserve((size_t)m * sizeof(u32))) || (rc = hist_dev.reserve(hbytes)) || (rc = set_tile_lds())) return rc;
    if (c.wts) {   // the slot weights in the layout of the slot table, [m][max_slots]
        float* pw = sg.wts.as<float>();
        for (int b = 0; b < m; ++b) {
            const int nt = qoff[b + 1] - qoff[b];
            for (int s = 0; s < max_slots; ++s) pw[(size_t)b * max_slots + s] = s < nt ? c.wts[qoff[b] + s] : 0.f;
        }
        HR_CHECK_HIP(hipMemcpyAsync(wts_dev.p, pw, n_slots * sizeof(float), hipMemcpyHostToDevice, c.st));
    }
    TileSlot* plan_slots = sg.slots.as<TileSlot>();
    int* plan_nslots = sg.nslots.as<int>();
    for (size_t i = 0; i < n_slots; ++i) plan_slots[i] = TileSlot{0, 0, -1};
    for (int b = 0; b < m; ++b) {
        const int nt = qoff[b + 1] - qoff[b];
        plan_nslots[b] = nt;
        for (int s = 0; s < nt; ++s) {
            const uint32_t t = c.terms[qoff[b] + s];
            TileSlot& sl = plan_slots[(size_t)b * max_slots + s];
            if ((i64)t < n_terms) { sl.lo = offsets[t]; sl.hi = offsets[t + 1]; sl.skip = skip_index[t]; }  // unknown terms score nothing
            postings_touched += (i64)(sl.hi - sl.lo);
            if (!scoped) bytes_alg += (i64)(sl.hi - sl.lo) * 8;
        }
    }
    if (scoped) fill_image(sg.scoped.as<uint32_t>());
    HR_CHECK_HIP(hipMemcpyAsync(slots_dev.p, plan_slots, n_slots * sizeof(TileSlot), hipMemcpyHostToDevice, c.st));
    HR_CHECK_HIP(hipMemcpyAsync(nslots_dev.p, plan_nslots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c.st));
    if (scoped) HR_CHECK_HIP(hipMemcpyAsync(scoped_dev.p, sg.scoped.p, image_words * 4, hipMemcpyHostToDevice, c.st));
    if (!sg.ev) HR_CHECK_HIP(hipEventCreateWithFlags(&sg.ev, hipEventDisableTiming));
    HR_CHECK_HIP(hipEventRecord(sg.ev, c.st));
    sg.used = true;
    HR_CHECK_HIP(hipMemsetAsync(theta_dev.p, 0, (size_t)m * sizeof(u32), c.st));
    HR_CHECK_HIP(hipMemsetAsync(hist_dev.p, 0, hbytes, c.st));
    tl = TileLaunch{max_slots, tile_kernel(n_postings < ((i64)1 << 30), scoped, c.wts != nullptr)};
    return HIPRAG_OK;
}

// tiled path: the whole query batch in one TAAT launch + one merge launch
int32_t Bm25Index::search_tiled(const Bm25Call& c)
{
    const i64 lists = ntiles() * kTileWaves;
    TileLaunch tl;
    const int32_t rc = plan_tiles(c, 0, c.nq, lists, 0, [](uint32_t*) {}, tl);
    if (rc) return rc;
    hipLaunchKernelGGL(tl.kernel, dim3(c.nq, (unsigned)ntiles()), dim3(kTileThreads), kTileDocs * sizeof(float), c.st,
                       doc_ids.as<u32>(), impacts.as<float>(), slots_dev.as<TileSlot>(), nslots_dev.as<int>(), skip_dev.as<u32>(),
                       tl.max_slots, n_docs, c.k, ck.as<u64>(), ci.as<i64>(), theta_dev.as<u32>(), hist_dev.as<u32>(),
                       ScopeArgs{nullptr, nullptr, 0}, c.wts ? (const float*)wts_dev.as<float>() : nullptr);
    launch_merge(lists * c.k, c.nq, c.k, c.o64, c.o32, c.oid, c.st);
    HR_CHECK_HIP(hipGetLastError());
    queries += c.nq;
    bytes_alg += (i64)c.nq * n_docs * 8;   // SURVEY 8d counts the accumulator zero + scan passes; this path keeps them in LDS
    return HIPRAG_OK;
}

// One workspace serves every call on the handle (bm25_internal.h), so a call on another stream than the previous one is
// ordered behind it on the device; a call that fails records nothing.
int32_t Bm25Index::search(const Bm25Call& c, const ScopePlan& P)
{
    if (prev_ev_set && prev_stream != c.st) HR_CHECK_HIP(hipStreamWaitEvent(c.st, prev_ev, 0));
    const int32_t rc = c.scoped ? search_scoped(c, P) : search_unscoped(c);
    if (rc) return rc;
    if (!prev_ev) HR_CHECK_HIP(hipEventCreateWithFlags(&prev_ev, hipEventDisableTiming));
    HR_CHECK_HIP(hipEventRecord(prev_ev, c.st));
    prev_ev_set = true;
    prev_stream = c.st;
    return HIPRAG_OK;
}

// ---- scoped search (hipbm25_search_scoped_dev, include/hiprag.h) -------------------------------------------------

// every check of a scoped call (the table rules are scope_plan.h's, n_docs for n); then fills the tile plan
int32_t Bm25Index::plan_scopes(int nq, int k, const int64_t* ranges, const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query,
                    ScopePlan& P) const
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(k >= 1 && k <= 64, "k must be in 1..%d for a scoped BM25 search (got %d)", 64, k);
    HR_REQUIRE(n_scopes >= 1, "n_scopes must be at least 1 (got %d)", n_scopes);
    const int32_t rc = check_scope_tables(ranges, scope_offsets, n_scopes, scope_of_query, nq, n_docs, "n_docs");
    if (rc) return rc;
    const i64 n_ranges = scope_offsets[n_scopes];
    P.rng.resize((size_t)2 * n_ranges);
    P.toff.assign(1, 0);
    for (int s = 0; s < n_scopes; ++s) {
        for (i64 j = scope_offsets[s]; j < scope_offsets[s + 1]; ++j) {
            const i64 lo = ranges[2 * j], hi = ranges[2 * j + 1];
            P.rng[(size_t)2 * j] = (uint32_t)lo;
            P.rng[(size_t)2 * j + 1] = (uint32_t)hi;
            if (hi == lo) continue;
            const size_t first = (size_t)P.toff.back();
            for (i64 t = lo / kTileDocs; t <= (hi - 1) / kTileDocs; ++t) {
                if (P.tile.size() > first && P.tile.back() == (int)t) { P.r1.back() = (int)j + 1; continue; }   // shares the tile of the range before
                P.tile.push_back((int)t);
                P.r0.push_back((int)j);
                P.r1.push_back((int)j + 1);
            }
        }
        P.toff.push_back((i64)P.tile.size());
    }
    return HIPRAG_OK;
}

// queries [q0, q0 + m) of a scoped call: one TAAT launch over their n_items work items + pad + merge
int32_t Bm25Index::scoped_chunk(const Bm25Call& c, const ScopePlan& P, int q0, int m, int max_tiles, i64 n_items)
{
    const int32_t* soq = c.scope_of_query + q0;
    const int k = c.k;
    // scoped image, 4-byte words: range table (8-byte entries first) | work items | tiles per query
    const size_t w_items = P.rng.size(), w_qt = w_items + (size_t)n_items * (sizeof(ScopedItem) / 4), words = w_qt + (size_t)m;
    const i64 lists = (i64)max_tiles * kTileWaves;
    TileLaunch tl;
    const int32_t rc = plan_tiles(c, q0, m, lists, words, [&](uint32_t* img) {
        if (!P.rng.empty()) memcpy(img, P.rng.data(), P.rng.size() * 4);
        ScopedItem* items = reinterpret_cast<ScopedItem*>(img + w_items);
        int* qtiles = reinterpret_cast<int*>(img + w_qt);
        for (int b = 0; b < m; ++b) qtiles[b] = (int)P.tiles_of(soq[b]);
        // position-in-scope major, queries fastest: the items of one query are spread over the launch (its early tiles'
        // bounds serve its later ones), neighbours in time are different queries
        i64 n = 0;
        for (int j = 0; j < max_tiles && n < n_items; ++j)
            for (int b = 0; b < m; ++b) {
                if (qtiles[b] <= j) continue;
                const size_t e = (size_t)P.toff[(size_t)soq[b]] + j;
                items[n++] = ScopedItem{b, P.tile[e], j, P.r0[e], P.r1[e]};
            }
    }, tl);
    if (rc) return rc;
    const uint32_t* dimg = scoped_dev.as<uint32_t>();
    hipLaunchKernelGGL(scoped_pad_kernel, dim3(m), dim3(256), 0, c.st, reinterpret_cast<const int*>(dimg + w_qt), max_tiles, k, ck.as<u64>(),
                       ci.as<i64>());
    if (n_items > 0) {
        const ScopeArgs sa{reinterpret_cast<const ScopedItem*>(dimg + w_items), reinterpret_cast<const uint2*>(dimg), max_tiles};
        hipLaunchKernelGGL(tl.kernel, dim3((unsigned)n_items), dim3(kTileThreads), kTileDocs * sizeof(float), c.st, doc_ids.as<u32>(),
                           impacts.as<float>(), slots_dev.as<TileSlot>(), nslots_dev.as<int>(), skip_dev.as<u32>(), tl.max_slots, n_docs, k,
                           ck.as<u64>(), ci.as<i64>(), theta_dev.as<u32>(), hist_dev.as<u32>(), sa,
                           c.wts ? (const float*)wts_dev.as<float>() : nullptr);
    }
    launch_merge(lists * k, m, k, c.o64 ? c.o64 + (i64)q0 * k : nullptr, c.o32 ? c.o32 + (i64)q0 * k : nullptr, c.oid + (i64)q0 * k, c.st);
    HR_CHECK_HIP(hipGetLastError());
    queries += m;
    return HIPRAG_OK;
}

// Chunks of queries: the candidate lists of a chunk, (its queries) x (tiles of its largest scope) x 4 waves x k x 16 bytes,
// stay within scoped_budget; a query whose own lists pass the tiled form's 2^20 entries runs alone (the loop merge takes
// any length).  A chunk is one query at least.  Returns the queries of the chunk that starts at q0.
int Bm25Index::chunk_queries(const ScopePlan& P, const int32_t* soq, int q0, int nq, int k, i64* max_tiles, i64* n_items) const
{
    int m = 0;
    i64 mt = 1, n = 0;
    bool alone = false;
    while (q0 + m < nq && !alone) {
        const i64 t = P.tiles_of(soq[q0 + m]);
        const i64 nmt = std::max(mt, t);
        const bool big = nmt * kTileWaves * k > ((i64)1 << 20);
        if (m > 0 && (big || (i64)(m + 1) * nmt * kTileWaves * k * 16 > scoped_budget)) break;
        mt = nmt;
        n += t;
        ++m;
        alone = big;
    }
    *max_tiles = mt;
    *n_items = n;
    return m;
}

int32_t Bm25Index::search_scoped(const Bm25Call& c, const ScopePlan& P)
{
    sc_items = sc_max_tiles = sc_chunks = 0;
    for (int q0 = 0, m; q0 < c.nq; q0 += m) {
        i64 mt, n_items;
        m = chunk_queries(P, c.scope_of_query, q0, c.nq, c.k, &mt, &n_items);
        const int32_t rc = scoped_chunk(c, P, q0, m, (int)mt, n_items);
        if (rc) return rc;
        sc_items += n_items;
        sc_max_tiles = std::max(sc_max_tiles, mt);
        ++sc_chunks;
    }
    return HIPRAG_OK;
}

Bm25Index::~Bm25Index()
{
    if (prev_ev) (void)hipEventDestroy(prev_ev);
    for (Stage& sg : stages)
        if (sg.ev) (void)hipEventDestroy(sg.ev);
}

int32_t Bm25Index::search_unscoped(const Bm25Call& c)
{
    const uint32_t* terms = c.terms;
    const int32_t* qoff = c.qoff;
    const float* wts = c.wts;
    const int nq = c.nq, k = c.k;
    hipStream_t st = c.st;
    int32_t rc;
    int longest = 0;
    for (int b = 0; b < nq; ++b) longest = std::max(longest, qoff[b + 1] - qoff[b]);
    // the tiled form for any collection whose per-query candidate lists (4 per tile x k) stay below a million entries --
    // 20 M documents at k = 50; the merge walks lists of any length (merge_packed_loop_kernel).  (Until late round 3 the
    // limit was 65536 entries = 3 M documents at k = 50: a 10M-document shard on one GPU fell back to the
    // global-accumulator form, 200 ms per 256 queries.)
    if (!force_global && k <= 64 && longest <= kMaxSlots && ntiles() * kTileWaves * k <= (i64)1 << 20) return search_tiled(c);
    if ((rc = reserve(k))) return rc;
    for (int q0 = 0; q0 < nq; q0 += kBatch) {
        const int m = std::min(kBatch, nq - q0);
        int max_terms = 0;
        for (int b = 0; b < m; ++b) max_terms = std::max(max_terms, qoff[q0 + b + 1] - qoff[q0 + b]);
        // slot-major plan: ranges[slot][b]
        std::vector<SlotRange> plan((size_t)std::max(max_terms, 1) * m);
        std::vector<u64> slot_max(std::max(max_terms, 1), 0);
        std::vector<float> plan_w(wts ? plan.size() : 0, 0.f);   // weighted: the slot's weight, slot-major like the plan
        for (int s = 0; s < max_terms; ++s)
            for (int b = 0; b < m; ++b) {
                SlotRange r{0, 0};
                const int nt = qoff[q0 + b + 1] - qoff[q0 + b];
                if (s < nt) {
                    const uint32_t t = terms[qoff[q0 + b] + s];
                    if ((i64)t < n_terms) { r.lo = offsets[t]; r.hi = offsets[t + 1]; }  // unknown terms score nothing
                    if (wts) plan_w[(size_t)s * m + b] = wts[qoff[q0 + b] + s];
                }
                plan[(size_t)s * m + b] = r;
                slot_max[s] = std::max<u64>(slot_max[s], r.hi - r.lo);
                postings_touched += (i64)(r.hi - r.lo);
                bytes_alg += (i64)(r.hi - r.lo) * 8;
            }
        if ((rc = ranges.reserve(plan.size() * sizeof(SlotRange)))) return rc;
        HR_CHECK_HIP(hipMemcpyAsync(ranges.p, plan.data(), plan.size() * sizeof(SlotRange), hipMemcpyHostToDevice, st));
        if (wts) {
            if ((rc = wts_dev.reserve(plan_w.size() * sizeof(float)))) return rc;
            HR_CHECK_HIP(hipMemcpyAsync(wts_dev.p, plan_w.data(), plan_w.size() * sizeof(float), hipMemcpyHostToDevice, st));
        }
        HR_CHECK_HIP(hipStreamSynchronize(st));  // plan is a stack-local vector; tiny copy
        HR_CHECK_HIP(hipMemsetAsync(acc.p, 0, (size_t)m * stride() * sizeof(float), st));
        for (int s = 0; s < max_terms; ++s) {
            if (slot_max[s] == 0) continue;
            const unsigned gx = (unsigned)((slot_max[s] + kTaatChunk - 1) / kTaatChunk);
            hipLaunchKernelGGL(wts ? taat_kernel<true> : taat_kernel<false>, dim3(gx, m), dim3(kTaatThreads), 0, st, doc_ids.as<u32>(),
                               impacts.as<float>(), ranges.as<SlotRange>() + (size_t)s * m, acc.as<float>(), stride(),
                               wts ? (const float*)wts_dev.as<float>() + (size_t)s * m : nullptr);
        }
        double* o64q = c.o64 ? c.o64 + (i64)q0 * k : nullptr;
        float* o32q = c.o32 ? c.o32 + (i64)q0 * k : nullptr;
        i64* oidq = c.oid + (i64)q0 * k;
        const i64 wave_cand = nlists() * k;
        if (k <= 64 && wave_cand <= 16 * 64 * 16) {
            // fast selectors (topk_device.h): one wave filters 4096 accumulators, then a 16-wave merge per query.  At most
            // 16 * 64 * 16 = 16384 candidates are (16384 + 1023) / 1024 <= 16 per lane of the merge, so launch_merge picks
            // merge_packed_kernel<1 | 2 | 4 | 8 | 16> by the very thresholds this branch used to spell out, <16> being the
            // default of both; its loop kernel (more than 16 per lane) cannot be reached from here.
            hipLaunchKernelGGL(select_wave_kernel<true>, dim3((unsigned)(nlists() / 4), m), dim3(256), 0, st,
                               (const float*)acc.as<float>(), (i64)stride(), (i64)n_docs, k, ck.as<u64>(), ci.as<i64>());
            launch_merge(wave_cand, m, k, o64q, o32q, oidq, st);
        } else {
            hipLaunchKernelGGL(select_f32_kernel<true>, dim3((unsigned)nchunks(), m), dim3(256), 0, st,
                               (const float*)acc.as<float>(), (i64)stride(), (i64)n_docs, k, ck.as<u64>(), ci.as<i64>());
            FinishArgs fa;
            fa.ck = ck.as<u64>(); fa.ci = ci.as<i64>();
            fa.out64 = o64q; fa.out32 = o32q; fa.out_ids = oidq;
            fa.ncand = nchunks() * k; fa.id_base = id_base; fa.k = k;
            const size_t lds = (size_t)kTile * 16 + (size_t)k * 16 + 2 * 4 * sizeof(KeyId);
            HR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bm25_finish_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(bm25_finish_kernel, dim3(m), dim3(256), lds, st, fa);
        }
        HR_CHECK_HIP(hipGetLastError());
        queries += m;
        bytes_alg += (i64)m * n_docs * 8;
    }
    return HIPRAG_OK;
}

void Bm25Index::read_env()
{
    const char* fg = getenv("HIPBM25_GLOBAL_ACC");
    force_global = fg && fg[0] == '1';
    const char* sb = getenv("HIPBM25_SCOPED_BUDGET_MIB");   // tests: small budgets make small batches run in several chunks
    if (sb && atoll(sb) > 0) scoped_budget = atoll(sb) << 20;
}

Registry<Bm25Index>& bm25_reg()
{
    static Registry<Bm25Index> r;
    return r;
}

size_t clear_bm25_registry() { return bm25_reg().clear(); }

int32_t bm25_n_docs(uint64_t h, int64_t* out_n)
{
    std::shared_ptr<Bm25Index> ix = bm25_reg().get(h);
    if (!ix) { set_error("unknown bm25 handle %llu", (unsigned long long)h); return HIPRAG_E_HANDLE; }
    *out_n = ix->n_docs;
    return HIPRAG_OK;
}

int32_t bm25_id_base(uint64_t h, int64_t* out_base)
{
    std::shared_ptr<Bm25Index> ix = bm25_reg().get(h);
    if (!ix) { set_error("unknown bm25 handle %llu", (unsigned long long)h); return HIPRAG_E_HANDLE; }
    *out_base = ix->id_base;
    return HIPRAG_OK;
}
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipbm25_create(int64_t n_docs, int64_t n_terms, const uint64_t* offsets_host, const uint32_t* doc_ids_host,
                       const float* impacts_host, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle && offsets_host, "null argument");
    HR_REQUIRE(n_docs >= 0 && n_terms >= 0, "negative sizes");
    HR_REQUIRE(n_docs < (1ll << 32), "doc ids are u32: n_docs must be < 2^32 per shard");
    const uint64_t P = offsets_host[n_terms];
    HR_REQUIRE(offsets_host[0] == 0, "offsets[0] must be 0");
    for (int64_t t = 0; t < n_terms; ++t)
        HR_REQUIRE(offsets_host[t] <= offsets_host[t + 1], "offsets must be non-decreasing (term %lld)", (long long)t);
    HR_REQUIRE(P == 0 || (doc_ids_host && impacts_host), "null postings");
    for (uint64_t i = 0; i < P; ++i)
        HR_REQUIRE((int64_t)doc_ids_host[i] < n_docs, "posting %llu has doc id %u >= n_docs", (unsigned long long)i, doc_ids_host[i]);
    // every list strictly ascending by document: one posting per (term, document) is what makes the atomics-free
    // accumulation deterministic, and the skip tables are built by binary search
    for (int64_t t = 0; t < n_terms; ++t)
        for (uint64_t i = offsets_host[t] + 1; i < offsets_host[t + 1]; ++i)
            HR_REQUIRE(doc_ids_host[i - 1] < doc_ids_host[i], "posting list of term %lld is not strictly ascending by doc id", (long long)t);
    auto ix = std::make_shared<Bm25Index>();
    ix->device = device;
    ix->n_docs = n_docs;
    ix->n_terms = n_terms;
    ix->n_postings = (i64)P;
    ix->offsets.assign(offsets_host, offsets_host + n_terms + 1);
    HR_CHECK_HIP(hipSetDevice(device));
    int32_t rc;
    if ((rc = ix->doc_ids.reserve(std::max<size_t>(16, P * sizeof(u32))))) return rc;
    if ((rc = ix->impacts.reserve(std::max<size_t>(16, P * sizeof(float))))) return rc;
    if (P) {
        HR_CHECK_HIP(hipMemcpy(ix->doc_ids.p, doc_ids_host, P * sizeof(u32), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(ix->impacts.p, impacts_host, P * sizeof(float), hipMemcpyHostToDevice));
    }
    // skip tables of the long lists (taat_tile_kernel): posting offset at every tile boundary, relative to the list start
    {
        const i64 nt = ix->ntiles();
        ix->skip_index.assign((size_t)n_terms, -1);
        std::vector<u32> skip;
        for (int64_t t = 0; t < n_terms; ++t) {
            const uint64_t lo = offsets_host[t], hi = offsets_host[t + 1];
            if (hi - lo < kSkipMinDf) continue;
            HR_REQUIRE(hi - lo < (1ull << 32), "posting list of term %lld is too long for u32 skip offsets", (long long)t);
            ix->skip_index[(size_t)t] = (i64)skip.size();
            const uint32_t* b = doc_ids_host + lo;
            const uint32_t* e = doc_ids_host + hi;
            for (i64 tile = 0; tile <= nt; ++tile) {
                const uint64_t bound = (uint64_t)tile * kTileDocs;
                skip.push_back((u32)(std::lower_bound(b, e, bound, [](uint32_t d, uint64_t v) { return (uint64_t)d < v; }) - b));
            }
        }
        if ((rc = ix->skip_dev.reserve(std::max<size_t>(16, skip.size() * sizeof(u32))))) return rc;
        if (!skip.empty()) HR_CHECK_HIP(hipMemcpy(ix->skip_dev.p, skip.data(), skip.size() * sizeof(u32), hipMemcpyHostToDevice));
        ix->read_env();
    }
    *out_handle = bm25_reg().put(ix);
    return HIPRAG_OK;
}

int32_t hipbm25_destroy(uint64_t h)
{
    std::shared_ptr<Bm25Index> ix = bm25_reg().get(h);
    if (!ix) { set_error("unknown bm25 handle"); return HIPRAG_E_HANDLE; }
    {
        std::lock_guard<std::mutex> guard(ix->mu);
        (void)hipSetDevice(ix->device);
        (void)hipDeviceSynchronize();
    }
    bm25_reg().erase(h);
    return HIPRAG_OK;
}

int32_t hipbm25_set_id_base(uint64_t h, int64_t id_base)
{
    GET_BM25(h);
    ix->id_base = id_base;
    return HIPRAG_OK;
}

static int32_t validate_queries(const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k)
{
    HR_REQUIRE(nq >= 0 && k > 0 && k <= kMaxK, "bad nq/k (k must be in 1..%d)", kMaxK);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_offsets_host, "null q_offsets");
    HR_REQUIRE(q_offsets_host[0] >= 0, "q_offsets must start >= 0");
    for (int b = 0; b < nq; ++b) HR_REQUIRE(q_offsets_host[b] <= q_offsets_host[b + 1], "q_offsets must be non-decreasing");
    HR_REQUIRE(term_ids_host || q_offsets_host[nq] == q_offsets_host[0], "null term ids");
    return HIPRAG_OK;
}

// hipbm25_search_weighted*: one finite weight > 0 per query-term slot (the kernels' bounds rest on positive contributions)
static int32_t validate_weights(const float* term_weights_host, const int32_t* q_offsets_host, int32_t nq)
{
    HR_REQUIRE(term_weights_host, "term_weights is null");
    for (int32_t i = q_offsets_host[0]; i < q_offsets_host[nq]; ++i)
        HR_REQUIRE(std::isfinite(term_weights_host[i]) && term_weights_host[i] > 0.f,
                   "term_weights[%d] = %g: every weight must be finite and > 0 (drop terms of weight zero)", i, (double)term_weights_host[i]);
    return HIPRAG_OK;
}

// The one body of the eight search entries.  What an entry checks, in which order, and in which words it refuses is the
// entry's own and is kept as it grew:
//   unscoped: handle, dirty, queries, nq == 0 returns OK (before weights and outputs are looked at), weights, "null output";
//   scoped:   handle, dirty, scope tables (plan_scopes: nq >= 1, k <= 64), queries, weights, "out_scores / out_ids is null".
// Nothing is enqueued before the last check has passed.  A host entry runs on the null stream into the handle's o32 / oid
// and copies them back.
static int32_t run_search(uint64_t h, Bm25Call c)
{
    GET_BM25(h);
    BM25_REQUIRE_CLEAN(ix);
    Bm25Index::ScopePlan P;
    int32_t rc;
    if (c.scoped && (rc = ix->plan_scopes(c.nq, c.k, c.ranges, c.scope_offsets, c.n_scopes, c.scope_of_query, P))) return rc;
    if ((rc = validate_queries(c.terms, c.qoff, c.nq, c.k)) || c.nq == 0) return rc;
    if (c.weighted && (rc = validate_weights(c.wts, c.qoff, c.nq))) return rc;
    if (c.scoped) {
        HR_REQUIRE(!c.host || c.o32, "out_scores is null");
        HR_REQUIRE(c.oid, "out_ids is null");
    } else {
        HR_REQUIRE(c.oid && (!c.host || c.o32), "null output");
    }
    if (!c.host) return ix->search(c, P);
    float* host_scores = c.o32;
    i64* host_ids = c.oid;
    const size_t n = (size_t)c.nq * c.k;
    if ((rc = ix->o32.reserve(n * sizeof(float))) || (rc = ix->oid.reserve(n * sizeof(i64)))) return rc;
    c.o32 = ix->o32.as<float>();
    c.oid = ix->oid.as<i64>();
    if ((rc = ix->search(c, P))) return rc;
    HR_CHECK_HIP(hipMemcpy(host_scores, c.o32, n * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(host_ids, c.oid, n * sizeof(i64), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// The entries (include/hiprag.h) fill the descriptor: {scoped, weighted, host, terms, weights, q_offsets, nq, k, the four
// scope arguments, scores64, scores, ids, stream}.
int32_t hipbm25_search_dev(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                           double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    return run_search(h, {false, false, false, term_ids_host, nullptr, q_offsets_host, nq, k, nullptr, nullptr, 0, nullptr,
                          out_scores64_dev, out_scores_dev, (i64*)out_ids_dev, (hipStream_t)stream});
}

int32_t hipbm25_search(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                       float* out_scores, int64_t* out_ids)
{
    return run_search(h, {false, false, true, term_ids_host, nullptr, q_offsets_host, nq, k, nullptr, nullptr, 0, nullptr,
                          nullptr, out_scores, (i64*)out_ids, nullptr});
}

// Scoped search: the BM25 top k of the documents in the ranges of the query's scope (include/hiprag.h).
int32_t hipbm25_search_scoped_dev(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                                  const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                  const int32_t* scope_of_query_host, double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev,
                                  void* stream)
{
    return run_search(h, {true, false, false, term_ids_host, nullptr, q_offsets_host, nq, k, ranges_host, scope_offsets_host, n_scopes,
                          scope_of_query_host, out_scores64_dev, out_scores_dev, (i64*)out_ids_dev, (hipStream_t)stream});
}

int32_t hipbm25_search_scoped(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                              const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                              const int32_t* scope_of_query_host, float* out_scores, int64_t* out_ids)
{
    return run_search(h, {true, false, true, term_ids_host, nullptr, q_offsets_host, nq, k, ranges_host, scope_offsets_host, n_scopes,
                          scope_of_query_host, nullptr, out_scores, (i64*)out_ids, nullptr});
}

// Weighted forms (include/hiprag.h): the entries above with one weight per query-term slot.
int32_t hipbm25_search_weighted_dev(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host, const int32_t* q_offsets_host,
                                    int32_t nq, int32_t k, double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    return run_search(h, {false, true, false, term_ids_host, term_weights_host, q_offsets_host, nq, k, nullptr, nullptr, 0, nullptr,
                          out_scores64_dev, out_scores_dev, (i64*)out_ids_dev, (hipStream_t)stream});
}

int32_t hipbm25_search_weighted(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host, const int32_t* q_offsets_host,
                                int32_t nq, int32_t k, float* out_scores, int64_t* out_ids)
{
    return run_search(h, {false, true, true, term_ids_host, term_weights_host, q_offsets_host, nq, k, nullptr, nullptr, 0, nullptr,
                          nullptr, out_scores, (i64*)out_ids, nullptr});
}

int32_t hipbm25_search_scoped_weighted_dev(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                                           const int32_t* q_offsets_host, int32_t nq, int32_t k, const int64_t* ranges_host,
                                           const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                           double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    return run_search(h, {true, true, false, term_ids_host, term_weights_host, q_offsets_host, nq, k, ranges_host, scope_offsets_host,
                          n_scopes, scope_of_query_host, out_scores64_dev, out_scores_dev, (i64*)out_ids_dev, (hipStream_t)stream});
}

int32_t hipbm25_search_scoped_weighted(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host, const int32_t* q_offsets_host,
                                       int32_t nq, int32_t k, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                       const int32_t* scope_of_query_host, float* out_scores, int64_t* out_ids)
{
    return run_search(h, {true, true, true, term_ids_host, term_weights_host, q_offsets_host, nq, k, ranges_host, scope_offsets_host,
                          n_scopes, scope_of_query_host, nullptr, out_scores, (i64*)out_ids, nullptr});
}

// { documents per tile, work items of the last scoped call, tiles of its largest scope, its chunks }; synchronises
int32_t hipbm25_scoped_info(uint64_t h, int64_t* out4)
{
    GET_BM25(h);
    HR_REQUIRE(out4, "out4 is null");
    HR_CHECK_HIP(hipDeviceSynchronize());
    out4[0] = kTileDocs;
    out4[1] = ix->sc_items;
    out4[2] = ix->sc_max_tiles;
    out4[3] = ix->sc_chunks;
    return HIPRAG_OK;
}

int32_t hipbm25_get_stats(uint64_t h, hipbm25_stats* out)
{
    GET_BM25(h);
    HR_REQUIRE(out, "null out");
    out->queries = ix->queries;
    out->postings_touched = ix->postings_touched;
    out->bytes_algorithmic = ix->bytes_alg;
    return HIPRAG_OK;
}

}  // extern "C"
