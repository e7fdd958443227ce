// ivf_scoped.hip -- scoped IVF-Flat search (hipivf_search_scoped*): the top k of the rows that are in a probed list AND
// whose original id lies in a range of the query's scope.  The coarse step, the inversion of the probe table, the work
// items, the prefill and the merge are the list-major batch search's (ivf_search.hip, group_partials.hip); the scope
// tables are scope_plan.h's and go up as the flat scoped search's do (dense_scoped.hip).  The kernel that scores rows is this file's.
// HIPIVF_PROBE_SCOPE (hipivf_search_scoped_probe*) replaces the coarse step alone: ivf_scope_member_kernel decides which
// lists hold a row of which scope, ivf_scope_coarse_kernel scores the centroids of those lists, and the canonical merge
// picks every query's probes among them.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "ivf_internal.h"
#include "scope_plan.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// ivf_scoped_kernel is ivf_batch_kernel (ivf_search.hip) with a MEMBERSHIP step: the same work items (list, slice of 256
// stored rows, group of up to 16 of the (q, j) pairs that probe the list -- queries of different scopes share an item and
// its reads), the same 512 threads = 8 waves, the same register shape of the scoring (rescore_load8 x 2, rescore_acc8,
// rescore_reduce16: a row's score is the bits hipivf_search_dev and the flat finish give), the same wave-per-member selection
// and single writer per slot of the partial lists [nprobe x smax][nq][k].
//
// New, per item: once the slice's 256 original ids are in LDS, every (row, member) pair is decided -- the id bisected in
// the ranges of the member's scope (device tables, L2-resident; padding rows, id -1, are never members; a member that
// names the scope of the member the wave looked at before it reuses that answer) -- and kept as a 256-bit ROW MASK per
// member (a wave ballot per 64 rows: no atomics).  Wave 0 ORs the masks per quad (aligned group of 4 stored rows) and
// compacts the quads that hold any member into a list; the waves stride over THAT list, so a quad outside every member's
// scope is never loaded, and the in-scope rows of a list -- usually one contiguous run, ids ascend within a built list --
// are spread over all 8 waves.  No ascending order is assumed: any id may be in any row.  A member whose mask is zero on
// a quad skips the fp64 work for it; a key is written only where the member's bit is set, and the selection reads a key
// only there (anything else is key 0, "empty").  An item without a member row ends after the membership step: it loads
// neither queries nor rows.  rows_read += 4 per loaded quad: one integer atomic per item, no float atomics anywhere --
// the same bits from run to run.
// LDS: ivf_batch_kernel's G x (d_pad floats + 256 keys) + 256 ids + 2 G ints, plus G scopes, G x 8 mask words, the 64-entry
// quad list and its length = 98.9 KiB at d = 1024 (0.8 KiB over ivf_batch_kernel): one workgroup = 8 waves per CU.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950), both metrics: 205 VGPRs, no scratch, no VGPR spill (31
// SGPRs are parked in VGPR lanes, 13 in ivf_batch_kernel), occupancy 2 waves / SIMD = one workgroup per CU, as the LDS allows.
// Bound: not measured yet (tools/bench_ivf_scoped.py writes profiles/ivf_scoped_1m.json); by construction a full
// group on a full slice does ivf_batch_kernel's fp64 work, and an item outside every scope costs 2 KiB of ids and up to
// 8 bisections per thread.
// ------------------------------------------------------------------------------------------------------
constexpr int kIvfRows = 256;            // rows per slice (ivf_search.hip)
constexpr int kIvfScopedG = 16;          // queries per work item
constexpr int kIvfScopedThreads = 512;
constexpr int kIvfScopedMaxK = 256;      // the partial list of a slice holds its best k <= rows of a slice
constexpr i64 kIvfScopedBudget = 512ll << 20;   // bytes of partial lists per chunk of queries (include/hiprag.h)
constexpr int kIvfScopedMaxChunk = 16384;       // queries per chunk at most

struct IvfScopedArgs {
    const float4* xb;
    const float* q;          // [nq, d]
    const i64* offs;         // [nlist + 1] first stored row of every list
    const i64* orig;         // [stored rows] original id, -1 for padding
    const i64* pair_offs;    // [nlist + 1] first entry of every list in `order`
    const i64* order;        // the pairs q * nprobe + j, sorted by probed list (stable)
    const i64* item_start;   // [nlist + 1] work items of the lists before l; [nlist] = the item count
    const i64* ranges;       // [n_ranges][2] half-open ranges of original ids
    const i64* scope_off;    // [n_scopes + 1] first range of every scope
    const i64* scope_of_q;   // [nq] scope of every query of the chunk
    double* ps;              // [nprobe * smax][nq][k] partial scores (ivf_probe_kernel's layout)
    i64* pi;
    unsigned long long* rows_read;
    int d, P, k, nq, nprobe, smax, nlist;
};

template <int METRIC>
__global__ __launch_bounds__(kIvfScopedThreads) void ivf_scoped_kernel(IvfScopedArgs a)
{
    constexpr int G = kIvfScopedG, S = kIvfRows, NW = kIvfScopedThreads / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_scoped_smem[];
    const int dpad = a.P * 8;
    float* qv = reinterpret_cast<float*>(ivf_scoped_smem);     // [G][dpad]
    u64* keys = reinterpret_cast<u64*>(qv + (size_t)G * dpad); // [G][S]
    i64* ids = reinterpret_cast<i64*>(keys + G * S);           // [S]
    int* mq = reinterpret_cast<int*>(ids + S);                 // [G] query of a group member
    int* mj = mq + G;                                          // [G] its probe rank j
    int* ms = mj + G;                                          // [G] its scope
    u32* mask = reinterpret_cast<u32*>(ms + G);                // [G][S / 32] bit r = row r of the slice is a member's
    int* qlist = reinterpret_cast<int*>(mask + G * (S / 32));  // [S / 4] the quads that hold a row of any member
    int* nquads = qlist + S / 4;                               // [1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane & 3, hh = (lane >> 2) & 1, pq = lane >> 3;
    const i64 nitems = a.item_start[a.nlist];
    for (i64 item = blockIdx.x; item < nitems; item += gridDim.x) {
        int l = 0, lh = a.nlist;                 // item_start[l] <= item < item_start[lh]
        while (lh - l > 1) {
            const int mid = (l + lh) >> 1;
            if (a.item_start[mid] <= item) l = mid; else lh = mid;
        }
        const i64 p0 = a.pair_offs[l], cnt = a.pair_offs[l + 1] - p0;
        const int ngroups = (int)((cnt + G - 1) / G);
        const i64 within = item - a.item_start[l];
        const int sl = (int)(within / ngroups), grp = (int)(within - (i64)sl * ngroups);
        const int gn = (int)min((i64)G, cnt - (i64)grp * G);          // 1..G members
        const i64 lo = a.offs[l] + (i64)sl * S, hi = min(a.offs[l + 1], lo + S);
        const int n = (int)(hi - lo);                                 // 1..S rows (lists start on 32-row blocks: quad-aligned)
        if (tid < gn) {
            const i64 pair = a.order[p0 + (i64)grp * G + tid];
            const int qi = (int)(pair / a.nprobe);
            mq[tid] = qi;
            mj[tid] = (int)(pair % a.nprobe);
            ms[tid] = (int)a.scope_of_q[qi];
        }
        for (int c = tid; c < S; c += kIvfScopedThreads) ids[c] = c < n ? a.orig[lo + c] : -1;
        __syncthreads();
        {   // membership: wave w decides rows (w & 3) * 64 + lane for members w >> 2, (w >> 2) + 2, ...
            const int part = wave & 3;
            const i64 id = ids[part * 64 + lane];
            int prev_scope = -1;
            bool in = false;
            for (int g = wave >> 2; g < gn; g += 2) {
                const int sc = ms[g];
                if (sc != prev_scope) {
                    prev_scope = sc;
                    i64 j = a.scope_off[sc], jh = a.scope_off[sc + 1];
                    in = false;
                    if (id >= 0 && jh > j) {     // the last range that starts at or before id: the only one that can hold it
                        while (jh - j > 1) {
                            const i64 mid = (j + jh) >> 1;
                            if (a.ranges[2 * mid] <= id) j = mid; else jh = mid;
                        }
                        in = a.ranges[2 * j] <= id && id < a.ranges[2 * j + 1];
                    }
                }
                const u64 b = __ballot(in);
                if (lane == 0) {
                    mask[g * (S / 32) + part * 2] = (u32)b;
                    mask[g * (S / 32) + part * 2 + 1] = (u32)(b >> 32);
                }
            }
        }
        __syncthreads();
        if (wave == 0) {                         // lane = quad: the union over the members, compacted
            u32 any = 0;
            for (int g = 0; g < gn; ++g) any |= (mask[g * (S / 32) + (lane >> 3)] >> ((lane & 7) * 4)) & 0xFu;
            const u64 b = __ballot(any != 0);
            if (any) qlist[__popcll(b & ((1ull << lane) - 1ull))] = lane;
            if (lane == 0) {
                const int c = __popcll(b);
                nquads[0] = c;
                if (c) atomicAdd(a.rows_read, (unsigned long long)(4 * c));   // integer: independent of arrival order
            }
        }
        __syncthreads();
        const int nqd = nquads[0];               // workgroup-uniform
        if (nqd > 0) {
            for (int g = 0; g < gn; ++g) {
                const float* src = a.q + (i64)mq[g] * a.d;
                for (int c = tid; c < dpad; c += kIvfScopedThreads) qv[g * dpad + c] = c < a.d ? src[c] : 0.f;
            }
            __syncthreads();
            for (int qi = wave; qi < nqd; qi += NW) {
                const int g4 = __builtin_amdgcn_readfirstlane(qlist[qi]);
                const i64 row0 = lo + (i64)g4 * 4;
                const float4* src = a.xb + (row0 / kRowsPerBlock) * a.P * kPieceVec4 + piece_slot(hh, (int)(row0 % kRowsPerBlock) + rr);
                float4 x0[8], x1[8];
                rescore_load8<0>(x0, src, pq, a.P);
                rescore_load8<1>(x1, src, pq, a.P);
                for (int g = 0; g < gn; ++g) {
                    const u32 mb = __builtin_amdgcn_readfirstlane((mask[g * (S / 32) + (g4 >> 3)] >> ((g4 & 7) * 4)) & 0xFu);
                    if (mb == 0) continue;       // wave-uniform: no row of this quad is the member's
                    double acc = 0.0;
                    rescore_acc8<METRIC, 0>(acc, x0, pq, hh, a.P, qv + g * dpad);
                    rescore_acc8<METRIC, 1>(acc, x1, pq, hh, a.P, qv + g * dpad);
                    const double s = rescore_reduce16(acc);
                    if (lane < 4 && ((mb >> lane) & 1u)) keys[g * S + g4 * 4 + lane] = ord64(METRIC == HIPRAG_METRIC_IP ? s : -s);
                }
            }
            __syncthreads();
            for (int g = wave; g < gn; g += NW) {
                u64 kk[S / 64];
                i64 ii[S / 64];
#pragma unroll
                for (int t = 0; t < S / 64; ++t) {
                    const int pos = t * 64 + lane;
                    const bool member = (mask[g * (S / 32) + t * 2 + (lane >> 5)] >> (lane & 31)) & 1u;
                    kk[t] = member ? keys[g * S + pos] : 0ull;
                    ii[t] = ids[pos];
                }
                const i64 o = ((i64)(mj[g] * a.smax + sl) * a.nq + mq[g]) * a.k;
                for (int r = 0; r < a.k; ++r) {
                    KeyId best;
                    best.key = 0;
                    best.id = 0x7FFFFFFFFFFFFFFFll;
                    best.pos = -1;
#pragma unroll
                    for (int t = 0; t < S / 64; ++t)
                        if (kk[t] != 0 && key_before(kk[t], ii[t], best.key, best.id)) { best.key = kk[t]; best.id = ii[t]; best.pos = t * 64 + lane; }
                    const KeyId w = wave_best(best);
                    if (w.key == 0) break;            // exhausted (wave-uniform); the remaining ranks keep their padding
                    if (lane == 0) {
                        a.ps[o + r] = METRIC == HIPRAG_METRIC_IP ? unord64(w.key) : -unord64(w.key);
                        a.pi[o + r] = w.id;
                    }
#pragma unroll
                    for (int t = 0; t < S / 64; ++t)
                        if (w.pos == t * 64 + lane) kk[t] = 0;
                }
            }
        }
        __syncthreads();                          // the next item overwrites the LDS
    }
}

size_t ivf_scoped_lds(int P)
{
    return (size_t)kIvfScopedG * P * 8 * 4 + (size_t)kIvfScopedG * kIvfRows * 8 + (size_t)kIvfRows * 8 + 3 * kIvfScopedG * 4 +
           (size_t)kIvfScopedG * (kIvfRows / 32) * 4 + (kIvfRows / 4) * 4 + 16;
}

// ------------------------------------------------------------------------------------------------------
// Scope-aware probing, step 1.  member[s][l] = 1 when list l stores a row whose id lies in a range of scope s.  Ids ascend
// within a list (ensure_lens has checked it) and len[l] excludes the padding, so the rows of a range [lo, hi) in a list are
// one run: the first member at or above lo (one bisection, as ivf_range_pos_kernel's) is in the range iff it is below hi.
// One thread per (scope, list) loops over the scope's ranges and stops at the first hit; every thread writes its own byte.
// pairs += the member pairs: a wave ballot and one integer atomic per wave (a count: the arrival order cannot matter).
// The loop bound is uniform over the workgroup so that the ballot sees whole waves.
// Cost: n_scopes x nlist threads x (ranges of the scope x log2(list length)) reads of `orig`; no LDS.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): 32 VGPRs, no scratch, no LDS, occupancy 8 waves / SIMD.  Bound: not measured yet
// (tools/bench_ivf_scope_probe.py).
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ivf_scope_member_kernel(const i64* __restrict__ orig, const i64* __restrict__ offs,
                                                               const i64* __restrict__ len, const i64* __restrict__ ranges,
                                                               const i64* __restrict__ scope_off, int n_scopes, int nlist, int nl4,
                                                               unsigned char* __restrict__ member, unsigned long long* __restrict__ pairs)
{
    const i64 total = (i64)n_scopes * nlist;
    for (i64 base = (i64)blockIdx.x * 256; base < total; base += (i64)gridDim.x * 256) {
        const i64 t = base + threadIdx.x;
        bool m = false;
        if (t < total) {
            const int s = (int)(t / nlist), l = (int)(t - (i64)s * nlist);
            const i64* ids = orig + offs[l];
            const i64 L = len[l];
            const i64 jh = scope_off[s + 1];
            for (i64 j = scope_off[s]; j < jh && !m && L > 0; ++j) {
                const i64 rlo = ranges[2 * j], rhi = ranges[2 * j + 1];
                if (rhi <= rlo) continue;
                i64 lo = 0, hi = L;             // ids[lo - 1] < rlo <= ids[hi]
                while (lo < hi) {
                    const i64 mid = (lo + hi) >> 1;
                    if (ids[mid] < rlo) lo = mid + 1; else hi = mid;
                }
                m = lo < L && ids[lo] < rhi;
            }
            member[(i64)s * nl4 + l] = m ? 1 : 0;
        }
        const u64 b = __ballot(m);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(pairs, (unsigned long long)__popcll(b));
    }
}

// ------------------------------------------------------------------------------------------------------
// Scope-aware probing, step 2: the MASKED coarse step.  ivf_scoped_kernel with the centroid index as the one list every
// query of the chunk probes: a work item is (group of up to 16 consecutive queries of the chunk, slice of 256 centroids),
// 512 threads = 8 waves, the queries in LDS, a quad of centroids in registers (rescore_load8 x 2) scored against every
// query of the group that has a member among its 4 lists (rescore_acc8 x 2, rescore_reduce16: the bits the flat coarse step
// gives for that centroid).  The centroid rows are read once per group, not once per query, and only the quads that hold
// a member list of at least one query of the group; an item without one loads neither queries nor centroids.
// Output: the candidate table [nq][nl4] -- (fp64 score, list) for a member list of the query's scope, (worst score, -1)
// for every other slot, the columns nlist..nl4-1 included -- which hiprag_merge_topk_dev turns into the probe table in
// canonical order (better score, then the lower list).  Every slot has exactly one writer: the padding pass skips the
// slots whose member byte is set, the scoring pass writes only those.  rows_read += 4 per loaded quad: one integer atomic
// per item, no float atomics -- the same bits from run to run.
// LDS: 16 x d_pad floats + 16 scopes + the 64-entry quad list and its length = 64.4 KiB at d = 1024.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950), both metrics: 209 VGPRs, no scratch, no VGPR spill (2 SGPRs
// are parked in VGPR lanes), occupancy 2 waves / SIMD = one workgroup per CU.
// Bound: not measured yet (tools/bench_ivf_scope_probe.py writes profiles/ivf_scope_probe_1m.json); by construction a
// group of 16 queries reads at most the centroid bytes once (4 MiB at 1024 lists x 1024, L2-resident) and does 16 x
// nlist x d fp64 multiply-adds at most.
// ------------------------------------------------------------------------------------------------------
struct IvfCoarseArgs {
    const float4* cb;            // the centroid index's blocked rows
    const float* q;              // [nq, d]
    const unsigned char* member; // [n_scopes][nl4]
    const i64* scope_of_q;       // [nq] scope of every query of the chunk
    double* cs;                  // [nq][nl4] candidate scores
    i64* ci;                     // [nq][nl4] candidate lists
    unsigned long long* rows_read;
    int d, P, nq, nlist, nl4;
};

template <int METRIC>
__global__ __launch_bounds__(kIvfScopedThreads) void ivf_scope_coarse_kernel(IvfCoarseArgs a)
{
    constexpr int G = kIvfScopedG, S = kIvfRows, NW = kIvfScopedThreads / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_coarse_smem[];
    const int dpad = a.P * 8;
    float* qv = reinterpret_cast<float*>(ivf_coarse_smem);     // [G][dpad]
    int* ms = reinterpret_cast<int*>(qv + (size_t)G * dpad);   // [G] scope of a group member
    int* qlist = ms + G;                                       // [S / 4] the quads that hold a member list of any query
    int* nquads = qlist + S / 4;                               // [1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane & 3, hh = (lane >> 2) & 1, pq = lane >> 3;
    const int nslices = (a.nl4 + S - 1) / S;
    const i64 nitems = (i64)((a.nq + G - 1) / G) * nslices;
    for (i64 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int grp = (int)(item / nslices), sl = (int)(item - (i64)grp * nslices);
        const int q0 = grp * G, gn = min(G, a.nq - q0);               // 1..G queries
        const int r0 = sl * S, n = min(S, a.nl4 - r0);                // 4..S columns, a multiple of 4
        if (tid < gn) ms[tid] = (int)a.scope_of_q[q0 + tid];
        __syncthreads();
        for (int c = tid; c < gn * S; c += kIvfScopedThreads) {       // padding for every slot that is not a member's
            const int g = c / S, r = c - g * S;
            if (r < n && !a.member[(i64)ms[g] * a.nl4 + r0 + r]) {
                const i64 o = (i64)(q0 + g) * a.nl4 + r0 + r;
                a.cs[o] = METRIC == HIPRAG_METRIC_IP ? -DBL_MAX : DBL_MAX;
                a.ci[o] = -1;
            }
        }
        if (wave == 0) {                         // lane = quad: the union over the queries, compacted
            u32 any = 0;
            if (lane * 4 < n)
                for (int g = 0; g < gn; ++g) any |= *reinterpret_cast<const u32*>(a.member + (i64)ms[g] * a.nl4 + r0 + lane * 4);
            const u64 b = __ballot(any != 0);
            if (any) qlist[__popcll(b & ((1ull << lane) - 1ull))] = lane;
            if (lane == 0) {
                const int c = __popcll(b);
                nquads[0] = c;
                if (c) atomicAdd(a.rows_read, (unsigned long long)(4 * c));   // integer: independent of arrival order
            }
        }
        __syncthreads();
        const int nqd = nquads[0];               // workgroup-uniform
        if (nqd > 0) {
            for (int g = 0; g < gn; ++g) {
                const float* src = a.q + (i64)(q0 + g) * a.d;
                for (int c = tid; c < dpad; c += kIvfScopedThreads) qv[g * dpad + c] = c < a.d ? src[c] : 0.f;
            }
            __syncthreads();
            for (int qi = wave; qi < nqd; qi += NW) {
                const int g4 = __builtin_amdgcn_readfirstlane(qlist[qi]);
                const int row0 = r0 + g4 * 4;    // < nlist: the quad holds a member list
                const float4* src = a.cb + (i64)(row0 / kRowsPerBlock) * a.P * kPieceVec4 + piece_slot(hh, row0 % kRowsPerBlock + rr);
                float4 x0[8], x1[8];
                rescore_load8<0>(x0, src, pq, a.P);
                rescore_load8<1>(x1, src, pq, a.P);
                for (int g = 0; g < gn; ++g) {
                    const u32 mw = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const u32*>(a.member + (i64)ms[g] * a.nl4 + row0));
                    if (mw == 0) continue;       // wave-uniform: none of the 4 lists is a member list of this query's scope
                    double acc = 0.0;
                    rescore_acc8<METRIC, 0>(acc, x0, pq, hh, a.P, qv + g * dpad);
                    rescore_acc8<METRIC, 1>(acc, x1, pq, hh, a.P, qv + g * dpad);
                    const double s = rescore_reduce16(acc);
                    if (lane < 4 && ((mw >> (8 * lane)) & 0xFFu)) {
                        const i64 o = (i64)(q0 + g) * a.nl4 + row0 + lane;
                        a.cs[o] = s;
                        a.ci[o] = row0 + lane;
                    }
                }
            }
        }
        __syncthreads();                          // the next item overwrites the LDS
    }
}

size_t ivf_coarse_lds(int P) { return (size_t)kIvfScopedG * P * 8 * 4 + kIvfScopedG * 4 + (kIvfRows / 4) * 4 + 16; }

// slots += the entries of the probe table that name a list (the others are the empty slots of a scope with fewer member
// lists than nprobe): a wave ballot and one integer atomic per wave, uniform loop bound as in ivf_scope_member_kernel
__global__ __launch_bounds__(256) void ivf_count_probes_kernel(const i64* __restrict__ probe, i64 n, unsigned long long* __restrict__ slots)
{
    for (i64 base = (i64)blockIdx.x * 256; base < n; base += (i64)gridDim.x * 256) {
        const i64 t = base + threadIdx.x;
        const u64 b = __ballot(t < n && probe[t] >= 0);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(slots, (unsigned long long)__popcll(b));
    }
}

const char* const kCannotProbeScope = "it can be searched with HIPIVF_PROBE_ANY but not with HIPIVF_PROBE_SCOPE";

// hipivf_search_scoped_dev and hipivf_search_scoped_probe_dev under the handle's mutex (include/hiprag.h).  Every check runs before anything is enqueued.
int32_t ivf_scoped_search_dev(IvfIndex& iv, const float* q_dev, int nq, int k, int nprobe, int probe_mode, const int64_t* ranges,
                              const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query, double* out64, float* out32,
                              int64_t* out_ids, hipStream_t st)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(probe_mode == HIPIVF_PROBE_ANY || probe_mode == HIPIVF_PROBE_SCOPE, "probe_mode must be HIPIVF_PROBE_ANY (0) or "
               "HIPIVF_PROBE_SCOPE (1) (got %d)", probe_mode);
    HR_REQUIRE(k >= 1 && k <= kIvfScopedMaxK, "k must be in 1..%d (got %d)", kIvfScopedMaxK, k);
    HR_REQUIRE(nprobe >= 1 && nprobe <= kMaxK, "nprobe must be in 1..%d (got %d)", kMaxK, nprobe);
    HR_REQUIRE(n_scopes >= 1, "n_scopes must be at least 1 (got %d)", n_scopes);
    HR_REQUIRE(q_dev, "q is null");
    HR_REQUIRE(out64, "out_scores64 is null");
    HR_REQUIRE(out_ids, "out_ids is null");
    int32_t rc;
    if ((rc = check_scope_tables(ranges, scope_offsets, n_scopes, scope_of_query, nq, iv.n_rows, "n"))) return rc;
    ScopeImage im;   // the lean form: ranges | scope_off | scope of every query
    build_scope_image(ranges, scope_offsets, n_scopes, scope_of_query, nq, 0, 1, im);
    const size_t o_off = im.o_off, o_soq = im.o_soq;

    DenseIndex& R = *iv.rows;
    DenseIndex& C = *iv.cents;
    HR_CHECK_HIP(hipSetDevice(R.device));
    ScopeUpload& S = iv.sc;
    GroupWorkspace& W = iv.gw;                   // the batch search's: the calls of a handle are serialised by its mutex
    const int nlist = iv.nlist;
    const bool by_scope = probe_mode == HIPIVF_PROBE_SCOPE;
    const int nl4 = (nlist + 3) / 4 * 4;         // columns of the candidate table and of the member table
    const int np = std::min(nprobe, nlist);
    const int smax = (int)std::max<i64>(1, (iv.maxlen + kIvfRows - 1) / kIvfRows);
    const int parts = np * smax;
    // PROBE_SCOPE: a query's row of the candidate table (score + list per column) counts against the budget as well
    const int qchunk = queries_per_chunk(nq, parts, k, kIvfScopedBudget, kIvfScopedMaxChunk, by_scope ? (i64)nl4 * 16 : 0);
    if (by_scope) {
        if ((rc = ensure_lens(iv, kCannotProbeScope))) return rc;   // the last check; synchronises on a handle's first call
        if ((rc = iv.member.reserve((size_t)n_scopes * nl4))) return rc;
        if ((rc = iv.cand_s.reserve((size_t)qchunk * nl4 * 8))) return rc;
        if ((rc = iv.cand_i.reserve((size_t)qchunk * nl4 * 8))) return rc;
        if ((rc = iv.sp_stat.reserve(32))) return rc;
    }
    if ((rc = iv.probe64.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = iv.probe_ids.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = W.ps.reserve((size_t)parts * qchunk * k * 8))) return rc;
    if ((rc = W.pi.reserve((size_t)parts * qchunk * k * 8))) return rc;
    if ((rc = W.order.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = W.items.reserve((size_t)(nlist + 1) * 8))) return rc;
    if ((rc = S.gw.stat.reserve(16))) return rc;   // [0] rows_read of this call, [1] group_item_scan's count of stored rows (unused)
    if ((rc = ensure_list_tab(iv))) return rc;
    const bool ip = R.metric == HIPRAG_METRIC_IP;
    const size_t lds = ivf_scoped_lds(R.P), clds = ivf_coarse_lds(R.P);
    const void* sk = ip ? reinterpret_cast<const void*>(ivf_scoped_kernel<HIPRAG_METRIC_IP>)
                        : reinterpret_cast<const void*>(ivf_scoped_kernel<HIPRAG_METRIC_L2>);
    if ((rc = ensure_lds(sk, lds))) return rc;
    if (by_scope) {
        const void* ck = ip ? reinterpret_cast<const void*>(ivf_scope_coarse_kernel<HIPRAG_METRIC_IP>)
                            : reinterpret_cast<const void*>(ivf_scope_coarse_kernel<HIPRAG_METRIC_L2>);
        if ((rc = ensure_lds(ck, clds))) return rc;
    }
    if ((rc = S.upload(im.img.data(), im.words, st))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(S.gw.stat.p, 0, 16, st));
    {
        std::lock_guard<std::mutex> gr(R.mu);
        if ((rc = R.wait_adds_stream(st))) return rc;
    }
    const i64* meta = S.meta.as<i64>();
    if (by_scope) {   // once per call: which list holds a row of which scope
        HR_CHECK_HIP(hipMemsetAsync(iv.sp_stat.p, 0, 32, st));
        HR_CHECK_HIP(hipMemsetAsync(iv.member.p, 0, (size_t)n_scopes * nl4, st));   // the columns nlist..nl4-1 stay 0
        const i64 total = (i64)n_scopes * nlist;
        const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>((total + 255) / 256, 4096));
        hipLaunchKernelGGL(ivf_scope_member_kernel, dim3(grid), dim3(256), 0, st, iv.orig.as<i64>(), iv.offs.as<i64>(), iv.lens_dev.as<i64>(),
                           meta, meta + o_off, n_scopes, nlist, nl4, iv.member.as<unsigned char>(), iv.sp_stat.as<unsigned long long>());
        HR_CHECK_HIP(hipGetLastError());
        std::lock_guard<std::mutex> gc(C.mu);
        if ((rc = C.wait_adds_stream(st))) return rc;
    }
    for (int o = 0; o < nq; o += qchunk) {
        const int m = std::min(qchunk, nq - o);
        const float* qo = q_dev + (i64)o * R.d;
        const i64 pairs = (i64)m * np;
        if (!by_scope) {   // coarse quantiser: the exact flat search of the query among the centroids, whatever the scope
            std::lock_guard<std::mutex> gc(C.mu);
            if ((rc = C.search_dev(qo, m, np, iv.probe64.as<double>(), nullptr, iv.probe_ids.as<int64_t>(), st))) return rc;
        } else {
            // the same scores for the centroids of the member lists of the query's scope alone, and the first np of them; a
            // scope with fewer member lists leaves EMPTY SLOTS (-1) in the probe table, which the counting sort below
            // drops (an entry outside 0..nlist-1 belongs to no list): no pair, no work item and no partial list come of
            // them, and nothing indexes a list with one
            IvfCoarseArgs c;
            c.cb = C.xb.as<float4>(); c.q = qo; c.member = iv.member.as<unsigned char>(); c.scope_of_q = meta + o_soq + o;
            c.cs = iv.cand_s.as<double>(); c.ci = iv.cand_i.as<i64>();
            c.rows_read = iv.sp_stat.as<unsigned long long>() + 2;
            c.d = R.d; c.P = R.P; c.nq = m; c.nlist = nlist; c.nl4 = nl4;
            const i64 nitems = (i64)((m + kIvfScopedG - 1) / kIvfScopedG) * ((nl4 + kIvfRows - 1) / kIvfRows);
            const unsigned cgrid = (unsigned)std::max<i64>(1, std::min<i64>(nitems, (i64)R.n_cu));   // one resident workgroup per CU
            if (ip) hipLaunchKernelGGL(ivf_scope_coarse_kernel<HIPRAG_METRIC_IP>, dim3(cgrid), dim3(kIvfScopedThreads), clds, st, c);
            else hipLaunchKernelGGL(ivf_scope_coarse_kernel<HIPRAG_METRIC_L2>, dim3(cgrid), dim3(kIvfScopedThreads), clds, st, c);
            HR_CHECK_HIP(hipGetLastError());
            if ((rc = hiprag_merge_topk_dev(iv.cand_s.as<double>(), iv.cand_i.as<int64_t>(), 1, m, nl4, np, 0, R.metric, iv.probe64.as<double>(),
                                            nullptr, iv.probe_ids.as<int64_t>(), st)))
                return rc;
            const unsigned pgrid = (unsigned)std::max<i64>(1, std::min<i64>((pairs + 255) / 256, 4096));
            hipLaunchKernelGGL(ivf_count_probes_kernel, dim3(pgrid), dim3(256), 0, st, iv.probe_ids.as<i64>(), pairs,
                               iv.sp_stat.as<unsigned long long>() + 1);
            HR_CHECK_HIP(hipGetLastError());
        }
        if ((rc = ivf_counting_sort(iv.probe_ids.as<i64>(), pairs, nlist, 1, W.tiles, W.len, W.offs, W.chunks, W.order.as<i64>(), st))) return rc;
        if ((rc = group_item_scan(W.len.as<i64>(), iv.list_tab.as<i64>(), iv.list_tab.as<i64>() + nlist, kIvfScopedG, false, nlist,
                                  W.items.as<i64>(), S.gw.stat.as<i64>() + 1, st)))
            return rc;
        if ((rc = fill_partials(R.metric, W.ps.as<double>(), W.pi.as<i64>(), (i64)parts * m * k, st))) return rc;
        IvfScopedArgs a;
        a.xb = R.xb.as<float4>(); a.q = qo; a.offs = iv.offs.as<i64>(); a.orig = iv.orig.as<i64>();
        a.pair_offs = W.offs.as<i64>(); a.order = W.order.as<i64>(); a.item_start = W.items.as<i64>();
        a.ranges = meta; a.scope_off = meta + o_off; a.scope_of_q = meta + o_soq + o;
        a.ps = W.ps.as<double>(); a.pi = W.pi.as<i64>();
        a.rows_read = S.gw.stat.as<unsigned long long>();
        a.d = R.d; a.P = R.P; a.k = k; a.nq = m; a.nprobe = np; a.smax = smax; a.nlist = nlist;
        // items <= (pairs / G + lists with a pair) x slices of the longest list; the grid strides over the device-side count
        const i64 bound = (pairs / kIvfScopedG + std::min<i64>(nlist, pairs)) * smax;
        const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>(bound, (i64)R.n_cu));   // one resident workgroup per CU
        if (ip) hipLaunchKernelGGL(ivf_scoped_kernel<HIPRAG_METRIC_IP>, dim3(grid), dim3(kIvfScopedThreads), lds, st, a);
        else hipLaunchKernelGGL(ivf_scoped_kernel<HIPRAG_METRIC_L2>, dim3(grid), dim3(kIvfScopedThreads), lds, st, a);
        HR_CHECK_HIP(hipGetLastError());
        if ((rc = hiprag_merge_topk_dev(W.ps.as<double>(), W.pi.as<int64_t>(), parts, m, k, k, (int64_t)m * k, R.metric, out64 + (i64)o * k,
                                        out32 ? out32 + (i64)o * k : nullptr, out_ids + (i64)o * k, st)))
            return rc;
    }
    iv.searches += nq;
    S.gw.chunk = qchunk;
    S.gw.chunks_n = (nq + qchunk - 1) / qchunk;
    if (by_scope) iv.sp_chunks = S.gw.chunks_n;
    return HIPRAG_OK;
}

}  // namespace

int32_t ivf_make_device_current(uint64_t h)
{
    GET_IVF(h);
    HR_CHECK_HIP(hipSetDevice(iv->rows->device));
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

// Scoped IVF search: the top k of the rows of the probed lists whose id lies in the query's scope (include/hiprag.h).
int32_t hipivf_search_scoped_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe, const int64_t* ranges_host,
                                 const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                 double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    return ivf_scoped_search_dev(*iv, q_dev, nq, k, nprobe, HIPIVF_PROBE_ANY, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                                 out_scores64_dev, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

// The scoped search with the rule that picks the probed lists as an argument: HIPIVF_PROBE_ANY is the entry above,
// HIPIVF_PROBE_SCOPE probes the nprobe best lists among those that hold a row of the query's scope (include/hiprag.h).
int32_t hipivf_search_scoped_probe_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe, int32_t probe_mode,
                                       const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                       const int32_t* scope_of_query_host, double* out_scores64_dev, float* out_scores_dev,
                                       int64_t* out_ids_dev, void* stream)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    return ivf_scoped_search_dev(*iv, q_dev, nq, k, nprobe, probe_mode, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                                 out_scores64_dev, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int32_t hipivf_search_scoped(uint64_t h, const float* q_host, int32_t nq, int32_t k, int32_t nprobe, const int64_t* ranges_host,
                             const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                             double* out_scores64, float* out_scores, int64_t* out_ids)
{
    return hipivf_search_scoped_probe(h, q_host, nq, k, nprobe, HIPIVF_PROBE_ANY, ranges_host, scope_offsets_host, n_scopes,
                                      scope_of_query_host, out_scores64, out_scores, out_ids);
}

int32_t hipivf_search_scoped_probe(uint64_t h, const float* q_host, int32_t nq, int32_t k, int32_t nprobe, int32_t probe_mode,
                                   const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                   const int32_t* scope_of_query_host, double* out_scores64, float* out_scores, int64_t* out_ids)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(k >= 1 && k <= kIvfScopedMaxK, "k must be in 1..%d (got %d)", kIvfScopedMaxK, k);
    HR_REQUIRE(q_host, "q is null");
    HR_REQUIRE(out_scores64, "out_scores64 is null");
    HR_REQUIRE(out_ids, "out_ids is null");
    const int d = iv->rows->d;
    HR_CHECK_HIP(hipSetDevice(iv->rows->device));
    int32_t rc;
    if ((rc = iv->hq.reserve((size_t)nq * d * sizeof(float)))) return rc;
    if ((rc = iv->ho64.reserve((size_t)nq * k * sizeof(double)))) return rc;
    if ((rc = iv->ho32.reserve((size_t)nq * k * sizeof(float)))) return rc;
    if ((rc = iv->hoid.reserve((size_t)nq * k * sizeof(int64_t)))) return rc;
    HR_CHECK_HIP(hipMemcpy(iv->hq.p, q_host, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = ivf_scoped_search_dev(*iv, iv->hq.as<float>(), nq, k, nprobe, probe_mode, ranges_host, scope_offsets_host, n_scopes,
                                    scope_of_query_host, iv->ho64.as<double>(), iv->ho32.as<float>(), iv->hoid.as<int64_t>(), nullptr)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(out_scores64, iv->ho64.p, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost));
    if (out_scores) HR_CHECK_HIP(hipMemcpy(out_scores, iv->ho32.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, iv->hoid.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// { queries per work item, queries per chunk of the last scoped call, its chunks, 4 x the quads its work items loaded }; synchronises
int32_t hipivf_scoped_info(uint64_t h, int64_t* out4)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_REQUIRE(out4, "out4 is null");
    out4[0] = kIvfScopedG;
    out4[1] = iv->sc.gw.chunk;
    out4[2] = iv->sc.gw.chunks_n;
    out4[3] = 0;
    if (iv->sc.gw.stat.p) {
        HR_CHECK_HIP(hipSetDevice(iv->rows->device));
        HR_CHECK_HIP(hipDeviceSynchronize());
        HR_CHECK_HIP(hipMemcpy(&out4[3], iv->sc.gw.stat.p, 8, hipMemcpyDeviceToHost));
    }
    return HIPRAG_OK;
}

// { member (scope, list) pairs, (query, probe) slots probed, chunks, centroid rows read } of the last HIPIVF_PROBE_SCOPE call;
// synchronises
int32_t hipivf_scope_probe_info(uint64_t h, int64_t* out4)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_REQUIRE(out4, "out4 is null");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (iv->sp_stat.p) {
        HR_CHECK_HIP(hipSetDevice(iv->rows->device));
        HR_CHECK_HIP(hipDeviceSynchronize());
        int64_t v[3];
        HR_CHECK_HIP(hipMemcpy(v, iv->sp_stat.p, 24, hipMemcpyDeviceToHost));
        out4[0] = v[0];
        out4[1] = v[1];
        out4[2] = iv->sp_chunks;
        out4[3] = v[2];
    }
    return HIPRAG_OK;
}

}  // extern "C"
