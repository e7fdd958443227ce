// dense_scan.h -- K1 of the flat index (overview: dense_index.hip): what a scan leaves behind (ScanArgs, Cand), the
// in-register / in-LDS tail both narrow kernels share, the query staging, qtile_kernel, scan_bf16_kernel and
// scan_split_kernel; scan_wide.h, included at the end, adds scan_wide_kernel.  Device text for ONE translation unit:
// dense_index.hip includes it inside its namespaces (hiprag, then the unnamed one), so every kernel is compiled once.  The
// policy constants (kClasses, kStageHalf, kThetaBack, kNoFilterGroups, ...) come from dense_plan.h.
#pragma once

// ------------------------------------------------------------------------------------------------------
// K1: the scan
// ------------------------------------------------------------------------------------------------------
// What a scan leaves behind (round 3).  A GROUP is the 16 rows one lane holds of a block's 32 x 32 score tile: rows
// 32*blk + 8g + 4h + j (g, j in 0..3) for lane half h; group id = 2*blk + h.  Per group the scan knows
//   first  = the largest maximum of its four row QUADS (quad g = rows 8g + 4h + 0..3), the quad number in its two low
//            mantissa bits, and
//   second = the largest quad maximum of the other three quads.
// Rounds 1-2 wrote both for EVERY group (N/16 floats x 2 per query: 256 MB per 512-query launch at 1M rows) and a
// selector read them back to keep a few dozen -- 1.6 % of the launch's bytes and 7-20 % of its time, depending on where the
// buffers had landed.  Now the scan keeps the few that matter itself:
//   * PUBLISH.  Every wave publishes the maximum `first` of each chunk it finishes (after the first block of its range, then
//     every kPublish blocks), per query, with one atomicMax into one of 64 class slots of that query (class = a mix of wave
//     and workgroup index, so that every class has members on every XCD and in every wave slot; one coalesced 256-byte
//     memory-side atomic per wave and chunk).
//   * BOUND.  theta(query) = min over the class slots: 64 distinct groups reach it, and on average ~4.5 x 64 groups of the
//     whole index do.  The waves of a workgroup take turns recomputing it, kRecompute blocks behind a publish; the result
//     goes into thetac[query] (global, atomicMax: it only ever rises) and into the workgroup's LDS copy.
//   * TEST.  A group's values stay in registers (shift chains) for kAge more blocks and are then tested against the LDS
//     copy of their query's bound: first >= bound -> staged in LDS (LDS atomics return on lgkmcnt: the hand-counted vmcnt
//     ring never sees them), else dropped.  A wave that gets there before the bound of the pass exists waits for it (bounded).
//   * FLUSH.  In the pass prologues (and at the end) the staged entries are tested again, against bounds refreshed
//     memory-side, and appended to the per-query CANDIDATE LISTS in global memory, one global atomicAdd per entry: ~350
//     entries per query at 1M rows, 3 MB per launch instead of 256.
// Exactness never depends on timing: every value that was dropped was below a bound that had been folded into thetac, so
// the FINAL thetac[q] bounds everything that is not on q's list -- a late publisher makes lists longer, never wrong.  The
// finish (fin_kernel) ranks a query's list, re-scores its best groups in fp64 and extends the re-scored prefix until nothing
// on the list can still reach the top k; the certificate takes the final thetac as the bound of the unseen rows.
constexpr int kCandCap = 4096;    // candidate-list entries per query in global memory (overflow -> exhaustive path)
constexpr int kPublish = 4;       // blocks per published chunk
constexpr int kDelay = 4;         // blocks between the end of a value's chunk and its test (publishers of other workgroups catch up)
constexpr int kAge = kPublish - 1 + kDelay;   // chain position at which a value is tested
constexpr int kRecompute = 2;     // blocks between a chunk's publish and the recomputation of theta by the wave whose turn it is

struct Cand {       // one candidate group of one query, 16 bytes: staging entry and global list entry
    u64 key;        // pack_key(first, group id): ord32(first) << 32 | ~group
    float sec;      // second
    u32 q;          // query index inside the launch (staging only)
};
static_assert(sizeof(Cand) == kCandBytes, "dense_plan.h sizes the staging area by kCandBytes");

struct ScanArgs {
    const float4* xb;     // blocked fp32 rows (q64 mode)
    const void* xh;       // bf16 filter copy (bf16 mode)
    const float* q;       // [nq, d] row-major queries
    const void* qtile;    // bf16 mode, multi-pass launches: the passes' LDS tile images, made by qtile_kernel (else null)
    const float* norms;   // [rows] squared norms (L2 only)
    u32* slots;           // [passes][kClasses][64]: published chunk maxima (ord32 images), query = 64 * pass + lane
    u32* thetac;          // [Q] current bound per query (ord32 image; 0 = none yet)
    u32* count;           // [Q] appended candidates per query
    Cand* list;           // [Q][kCandCap]
    int64_t nblocks;
    int64_t ntotal;
    int nq, d, P;
    int filter;           // 0: list every group (small indexes)
    int ncls;             // theta classes in use: min(kClasses, waves that own blocks) -- every class needs a publisher, or theta never forms
    unsigned long long* stamps;  // timing only (else null): [waves][2] wall-clock ticks at wave entry / exit
    // start gate (hipidx_gate_tail_dev): every workgroup counts itself in when it starts; the one that completes the launch
    // (started == target: every workgroup of the grid holds its CU) writes the launch's sequence number into the signal word
    // the tail streams of the PREVIOUS launch wait on
    unsigned long long* started;
    unsigned long long target, seq;
    unsigned long long* gate;     // the gate word (device memory)
    // the wide kernel's fold schedule (wide_fold, dense_plan.h): N, a power of two, and the counter of fold tiles
    int fold_every;
    unsigned long long* folds;
};

__host__ __device__ __forceinline__ int64_t scan_blocks_per_wave(int64_t nblocks, int64_t nwaves)
{
    return (nblocks + nwaves - 1) / nwaves;   // equal contiguous ranges: every active wave ends at the same time
}

// A group's 16 rows are four QUADS of 4 consecutive rows (quad g = rows 8g + 4h + 0..3: 64 contiguous bytes of every
// fp32 piece, the unit the fp64 re-score reads).  Replacing two mantissa bits by the quad number moves a value by
// < 2^-21 |v|: the certificate's eps carries that term (kTagSlack).
// L2: scores are 2<x,q> - |x|^2.  Padded tail rows get -FLT_MAX (finite, so the tag cannot turn it into a NaN).
__device__ __forceinline__ float tag_quad(float v, unsigned g) { return __uint_as_float((__float_as_uint(v) & ~3u) | g); }

template <int METRIC>
__device__ __forceinline__ float block_lane_top2(const f32x16& acc, const f32x4 (&nrm)[4], int64_t blk, int h, const ScanArgs& a,
                                                 float& second)
{
    float sc[16];
    if (METRIC == HIPRAG_METRIC_L2) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            sc[4 * g + 0] = 2.f * acc[4 * g + 0] - nrm[g][0];
            sc[4 * g + 1] = 2.f * acc[4 * g + 1] - nrm[g][1];
            sc[4 * g + 2] = 2.f * acc[4 * g + 2] - nrm[g][2];
            sc[4 * g + 3] = 2.f * acc[4 * g + 3] - nrm[g][3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[i] = acc[i];
    }
    if ((blk + 1) * kRowsPerBlock > a.ntotal) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t row = blk * kRowsPerBlock + 8 * (i >> 2) + 4 * h + (i & 3);
            if (row >= a.ntotal) sc[i] = -FLT_MAX;
        }
    }
    float qm[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        qm[g] = tag_quad(fmaxf(fmaxf(sc[4 * g], sc[4 * g + 1]), fmaxf(sc[4 * g + 2], sc[4 * g + 3])), (unsigned)g);
    float m1 = fmaxf(qm[0], qm[1]), m2 = fminf(qm[0], qm[1]);
    m2 = __builtin_amdgcn_fmed3f(m1, m2, qm[2]);   // new runner-up = median(best, runner-up, newcomer)
    m1 = fmaxf(m1, qm[2]);
    m2 = __builtin_amdgcn_fmed3f(m1, m2, qm[3]);
    m1 = fmaxf(m1, qm[3]);
    second = m2;
    return m1;
}

// ---- the in-register / in-LDS tail of both scan kernels --------------------------------------------------------------
// LDS behind the query tile: Cand stage[2][kStageHalf] (the passes alternate between the halves: the appends of pass p go to
// half p & 1 and are flushed in the prologue of pass p + 1, beside the staging of that pass's query tile) | u32 ctl[16] (ctl[h] =
// appends into half h since the launch began -- never reset, every thread remembers what has been flushed; ctl[4 + s] = tag of
// bound slot s)
// | u32 bound[kThetaBack][64] -- the workgroup's copy of the bounds of the last kThetaBack passes (slot = pass & 7, tag =
// pass + 1), which is what the in-loop test reads: NO global load sits in the block loop.  (A per-block global read of
// thetac did, at first: those lines are rewritten memory-side all the time, so the read misses L2, and because loads return
// in order every ring re-arm issued behind it waited for it -- 0.43 ms of a 2.6 ms launch.)
struct TailLds {
    Cand* stage;
    u32* ctl;
    u32* bound;
};
struct ScanTail {
    float cf[2][kAge + 1], cs[2][kAge + 1];   // [query tile][age]: first / second of the last kAge + 1 blocks (shift chains)
    float pm0, pm1;                           // running maximum of `first` over the current chunk, per tile
    int t;                                    // blocks this wave has finished, over all passes
    int pa, ja;                               // pass and block offset of the value that is tested next
    int ev;                                   // publish events so far (the waves of a workgroup take turns recomputing theta)
    int rc_due, rc_pass;                      // pending recomputation of theta: when (in blocks of this wave) and for which pass
    u32 flushed0, flushed1;                   // appends of each stage half that have been flushed (the same in every thread;
                                              // two scalars, not an array: a dynamically indexed array would live in scratch memory,
                                              // whose accesses count in vmcnt and drained the load ring -- 2.6 -> 3.5 ms per launch)

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int i = 0; i <= kAge; ++i) { cf[0][i] = cf[1][i] = -FLT_MAX; cs[0][i] = cs[1][i] = -FLT_MAX; }
        pm0 = pm1 = -INFINITY;
        t = 0; pa = 0; ja = 0; ev = 0; rc_due = -1; rc_pass = 0; flushed0 = flushed1 = 0;
    }
};

__device__ __forceinline__ u32 load_agent_u32(const u32* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// memory-side read (a returning atomic): never served from an XCD's L2, hence never stale; ~88 requests per microsecond
// and 64-byte line chip-wide, so only for rare paths
__device__ __forceinline__ u32 load_memside_u32(u32* p)
{
    return __hip_atomic_fetch_or(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the workgroup's LDS copy of a pass's bound: lane = query; raises, never lowers, the copy of the same pass
__device__ __forceinline__ void lds_put_bound(const TailLds& L, int pass, int lane, u32 v)
{
    const int slot = pass & (kThetaBack - 1);
    if (L.ctl[4 + slot] == (u32)pass + 1u) {
        if (v) atomicMax(L.bound + slot * 64 + lane, v);
    } else {
        L.bound[slot * 64 + lane] = v;
        if (lane == 0) L.ctl[4 + slot] = (u32)pass + 1u;
    }
}
__device__ __forceinline__ u32 lds_get_bound(const TailLds& L, int pass, int q_in_pass)
{
    const int slot = pass & (kThetaBack - 1);
    return L.ctl[4 + slot] == (u32)pass + 1u ? L.bound[slot * 64 + q_in_pass] : 0u;
}

// theta of the 64 queries of `pass` from their class slots (lane = query), folded into thetac and into the LDS copy.
// FRESH = memory-side reads (never stale, slow); otherwise sc1 loads, which the XCD's L2 may serve from a copy it fetched
// earlier -- an older, LOWER maximum: still a valid bound, only less tight; an empty class means no update.
template <bool FRESH>
__device__ __forceinline__ u32 recompute_theta(const ScanArgs& a, const TailLds& L, int pass, int lane)
{
    u32* s = a.slots + (size_t)pass * kClasses * 64 + lane;
    u32 m = 0xFFFFFFFFu;
#pragma unroll 16
    for (int c = 0; c < a.ncls; ++c) m = min(m, FRESH ? load_memside_u32(s + c * 64) : load_agent_u32(s + c * 64));
    if (pass * 64 + lane >= a.nq) m = 0;
    if (m != 0) atomicMax(a.thetac + pass * 64 + lane, m);   // BEFORE anything is dropped against m: the final thetac bounds every drop
    lds_put_bound(L, pass, lane, m);
    return m;
}

// A wave that reaches the test of a pass's values before that pass's bound exists -- waves are not in lockstep, the front
// runners of a launch are several blocks ahead of the rest -- would stage everything it holds (measured: a fifth of all
// tests in multi-pass launches, 13 k entries per query).  It waits instead, bounded (60 us): it is ahead of the publishers
// it waits for.  Polls are memory-side reads; the waiting wave recomputes theta itself, so the bound appears as soon as
// every class has a publisher.
__device__ __forceinline__ void wait_for_theta(const ScanArgs& a, const TailLds& L, int pass, int lane)
{
    const bool live = pass * 64 + lane < a.nq;
    const unsigned long long t0 = wall_clock64();
    for (int it = 0;; ++it) {
        u32 v = load_memside_u32(a.thetac + pass * 64 + lane);    // another workgroup may have formed it already
        if (__ballot(live && v == 0) && it) v = recompute_theta<true>(a, L, pass, lane);
        if (!__ballot(live && v == 0)) { lds_put_bound(L, pass, lane, v); break; }
        if (wall_clock64() - t0 > 6000ull) break;
        if (it) __builtin_amdgcn_s_sleep(127);
    }
}

// publish this wave's chunk maxima of `pass` (lane l ends up with the maximum of query 64 * pass + l)
__device__ __forceinline__ void publish_chunk(const ScanArgs& a, ScanTail& T, int pass, int lane, int cls, bool my_turn)
{
    const float x0 = fmaxf(T.pm0, __shfl_xor(T.pm0, 32)), x1 = fmaxf(T.pm1, __shfl_xor(T.pm1, 32));
    const float v = lane < 32 ? x0 : x1;
    if (pass * 64 + lane < a.nq) atomicMax(a.slots + ((size_t)pass * kClasses + cls) * 64 + lane, ord32(v));
    T.pm0 = T.pm1 = -INFINITY;
    // theta is recomputed kRecompute blocks LATER: every workgroup publishes a chunk at about the same moment, and a
    // recomputation right behind one's own publish finds classes whose publishers' atomics have not landed yet
    if (my_turn) { T.rc_due = T.t + kRecompute; T.rc_pass = pass; }
    ++T.ev;
}

__device__ __forceinline__ void append_direct(const ScanArgs& a, u64 key, float sec, u32 q)
{
    const u32 p = atomicAdd(a.count + q, 1u);
    if (p < (u32)kCandCap) a.list[(size_t)q * kCandCap + p] = Cand{key, sec, q};
}

__device__ __forceinline__ void stage_append(const ScanArgs& a, const TailLds& L, int half, u32 flushed, u64 key, float sec, u32 q)
{
    const u32 p = atomicAdd(L.ctl + half, 1u) - flushed;      // LDS atomic: returns on lgkmcnt, the hand-counted vmcnt ring never sees it
    if (p < (u32)kStageHalf) L.stage[half * kStageHalf + p] = Cand{key, sec, q};
    else append_direct(a, key, sec, q);
}

// test one parked value pair (block b0 + T.ja of pass T.pa) against the bounds th0 / th1 of its two queries; advance (pa, ja)
__device__ __forceinline__ void test_aged(const ScanArgs& a, ScanTail& T, const TailLds& L, int half, float f0, float s0, float f1, float s1,
                                          u32 th0, u32 th1, int lane, int64_t b0, int nbw)
{
    const int b = lane & 31, h = lane >> 5;
    const int q0 = T.pa * 64 + b, q1 = q0 + 32;
    const bool p0 = q0 < a.nq && ord32(f0) >= th0;
    const bool p1 = q1 < a.nq && ord32(f1) >= th1;
    if (__ballot(p0 || p1)) {   // wave-uniform: most blocks append nothing
        const u32 gid = (u32)(2 * (b0 + T.ja) + h);
        const u32 fl = half ? T.flushed1 : T.flushed0;
        if (p0) stage_append(a, L, half, fl, pack_key(f0, gid), s0, (u32)q0);
        if (p1) stage_append(a, L, half, fl, pack_key(f1, gid), s1, (u32)q1);
    }
    if (++T.ja == nbw) { T.ja = 0; ++T.pa; }
}

// one finished block: park its four values, publish at chunk ends, test the value that has reached kAge
__device__ __forceinline__ void tail_block(const ScanArgs& a, ScanTail& T, const TailLds& L, float f0, float s0, float f1, float s1,
                                           int pass, int j, int nbw, int lane, int wave, int nwaves, int cls, int64_t b0)
{
#pragma unroll
    for (int i = kAge; i > 0; --i) {
        T.cf[0][i] = T.cf[0][i - 1]; T.cs[0][i] = T.cs[0][i - 1];
        T.cf[1][i] = T.cf[1][i - 1]; T.cs[1][i] = T.cs[1][i - 1];
    }
    T.cf[0][0] = f0; T.cs[0][0] = s0; T.cf[1][0] = f1; T.cs[1][0] = s1;
    if (a.filter) {
        T.pm0 = fmaxf(T.pm0, f0);
        T.pm1 = fmaxf(T.pm1, f1);
        // after the FIRST block of a range (the bound of a pass can form as early as possible), then every kPublish blocks
        if ((j & (kPublish - 1)) == 0 || j == nbw - 1) publish_chunk(a, T, pass, lane, cls, T.ev % nwaves == wave);
    }
    if (T.t >= kAge) {
        const int b = lane & 31;
        u32 th0 = 0, th1 = 0;
        if (a.filter) {
            th0 = lds_get_bound(L, T.pa, b);
            th1 = lds_get_bound(L, T.pa, 32 + b);
            if (__ballot((th0 == 0 && T.pa * 64 + b < a.nq) || (th1 == 0 && T.pa * 64 + 32 + b < a.nq))) {
                wait_for_theta(a, L, T.pa, lane);
                th0 = lds_get_bound(L, T.pa, b);
                th1 = lds_get_bound(L, T.pa, 32 + b);
            }
        }
        test_aged(a, T, L, pass & 1, T.cf[0][kAge], T.cs[0][kAge], T.cf[1][kAge], T.cs[1][kAge], th0, th1, lane, b0, nbw);
    }
    if (T.rc_due >= 0 && T.t >= T.rc_due) { recompute_theta<false>(a, L, T.rc_pass, lane); T.rc_due = -1; }
    ++T.t;
}

// The workgroup's bounds of the last kThetaBack passes, refreshed from global memory (memory-side: fresh whatever the XCD's
// L2 holds) -- once per workgroup and pass, in the pass prologue.  (Read per staged entry instead, 150 k same-line atomics
// per pass saturated the four lines the bounds of a pass live on: ~88 requests per microsecond and line.)
__device__ __forceinline__ void refresh_bounds(const ScanArgs& a, const TailLds& L, int pass_now, int wave, int nwaves, int lane)
{
    if (!a.filter) return;
    for (int w = wave; w < kThetaBack; w += nwaves) {
        const int p = pass_now - w;
        if (p >= 0) lds_put_bound(L, p, lane, load_memside_u32(a.thetac + p * 64 + lane));
    }
}
// staged appends of one half -> the queries' global lists (whole workgroup; the half is not appended to meanwhile).  Every
// entry is tested AGAIN, against what its query's bound has become since it was staged: the in-loop test runs a few blocks
// behind the publishers, when the bound of a pass is still forming (a wave that runs ahead tests against the publishes of the
// other fast waves only -- measured 0.6-1.1 k staged entries per query at 1M rows where the final bound admits 0.3 k); the
// flush runs a pass later, or at the end of the launch.  Two phases, so that the round trip of the list counters' atomics
// hides behind whatever the caller does in between (the pass prologue stages the next query tile there).
struct FlushTicket {
    Cand e;
    u32 pos;
    bool live;
};
template <int NT>
__device__ __forceinline__ FlushTicket flush_begin(const ScanArgs& a, const TailLds& L, int half, int n, int tid)
{
    FlushTicket f;
    f.live = false;
    f.pos = 0;
    if (tid < n) {
        f.e = L.stage[half * kStageHalf + tid];
        f.live = (u32)(f.e.key >> 32) >= lds_get_bound(L, (int)(f.e.q >> 6), (int)(f.e.q & 63));
        if (f.live) f.pos = atomicAdd(a.count + f.e.q, 1u);
    }
    return f;
}
template <int NT>
__device__ __forceinline__ void flush_end(const ScanArgs& a, const TailLds& L, const FlushTicket& f, int half, int n, int tid)
{
    if (f.live && f.pos < (u32)kCandCap) a.list[(size_t)f.e.q * kCandCap + f.pos] = f.e;
    for (int i = tid + NT; i < n; i += NT) {     // more entries than threads: the front runners of a launch
        const Cand e = L.stage[half * kStageHalf + i];
        if ((u32)(e.key >> 32) >= lds_get_bound(L, (int)(e.q >> 6), (int)(e.q & 63))) append_direct(a, e.key, e.sec, e.q);
    }
}

// after the last block of the last pass: test what is still in the chains against the bound as it stands (no rendezvous: a
// wave that ends early misses the last chunks of the late ones -- a slightly lower bound, a few per cent more entries)
__device__ __forceinline__ void tail_drain(const ScanArgs& a, ScanTail& T, const TailLds& L, int half, int lane, int64_t b0, int nbw)
{
    const int R = T.t < kAge ? T.t : kAge;   // values still untested: chain positions R - 1 .. 0
    if (a.filter && T.rc_due >= 0) { recompute_theta<true>(a, L, T.rc_pass, lane); T.rc_due = -1; }
    int pa_loaded = -1;
    const int b = lane & 31;
#pragma unroll
    for (int pos = kAge - 1; pos >= 0; --pos) {
        if (pos < R) {
            if (a.filter && T.pa != pa_loaded) {   // the flush tests every staged entry again, against a refreshed copy
                lds_put_bound(L, T.pa, lane, load_memside_u32(a.thetac + T.pa * 64 + lane));
                pa_loaded = T.pa;
            }
            const u32 th0 = a.filter ? lds_get_bound(L, T.pa, b) : 0u, th1 = a.filter ? lds_get_bound(L, T.pa, 32 + b) : 0u;
            test_aged(a, T, L, half, T.cf[0][pos], T.cs[0][pos], T.cf[1][pos], T.cs[1][pos], th0, th1, lane, b0, nbw);
        }
    }
}

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split_pair(float v0, float v1, unsigned& hi, unsigned& lo)
{
    const bf16x2 h = __builtin_convertvector(f32x2{v0, v1}, bf16x2);  // v_cvt_pk_bf16_f32 (RNE)
    hi = __builtin_bit_cast(unsigned, h);
    const float r0 = v0 - __uint_as_float(hi << 16);
    const float r1 = v1 - __uint_as_float(hi & 0xFFFF0000u);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
}

// Query tile of one pass in LDS, bf16, for BOTH scan kernels: piece p (16 k-values), lane (h, b): Q^[b][16p + 8h + 0..7] for
// queries qbase + 0..31, then the same for queries qbase + 32..63 -- the B fragment of v_mfma_f32_32x32x16_bf16.  This
// form converts the (L2-resident) row-major fp32 queries in the workgroup: one-pass launches and the q64 kernel; multi-pass
// launches of the bf16 kernel copy images made by qtile_kernel (below).
template <int NT>
__device__ __forceinline__ void stage_query_tile(const ScanArgs& a, bf16x8* qw, int P2, int qbase, int tid)
{
    const bool vec_ok = (a.d & 3) == 0;
    // opaque copy of the thread index: left visible, hipcc hoists this address arithmetic out of the pass loop and keeps ~60
    // registers of it alive through the ring loop
    int tid_p = tid;
    asm volatile("" : "+v"(tid_p));
    int idx0 = tid_p;
    if (vec_ok && a.d >= 4) {
        // four fragments per step, their eight 16-B loads issued together and UNCONDITIONALLY (clamped query and column,
        // masked afterwards): predicated, each load was a branch + load + s_waitcnt vmcnt(0) -- 32 dependent L2 round trips
        // per thread and pass
        constexpr int UQ = 4;
        for (; idx0 + (UQ - 1) * NT < 2 * P2 * 64; idx0 += UQ * NT) {
            float4 t0[UQ], t1[UQ];
#pragma unroll
            for (int u4 = 0; u4 < UQ; ++u4) {
                const int idx = idx0 + u4 * NT;
                const int tile = idx >= P2 * 64;
                const int u = idx - tile * P2 * 64;
                const int p = u >> 6, l = u & 63;
                const int b = min(qbase + (l & 31) + 32 * tile, a.nq - 1);
                const int col = 16 * p + 8 * (l >> 5);
                const float* qp = a.q + (int64_t)b * a.d;
                t0[u4] = *reinterpret_cast<const float4*>(qp + min(col, a.d - 4));
                t1[u4] = *reinterpret_cast<const float4*>(qp + min(col + 4, a.d - 4));
            }
#pragma unroll
            for (int u4 = 0; u4 < UQ; ++u4) {
                const int idx = idx0 + u4 * NT;
                const int tile = idx >= P2 * 64;
                const int u = idx - tile * P2 * 64;
                const int p = u >> 6, l = u & 63;
                const int b = qbase + (l & 31) + 32 * tile;
                const int col = 16 * p + 8 * (l >> 5);
                const bool ok0 = b < a.nq && col + 3 < a.d, ok1 = b < a.nq && col + 7 < a.d;
                bf16x8 o;
                o[0] = (__bf16)(ok0 ? t0[u4].x : 0.f); o[1] = (__bf16)(ok0 ? t0[u4].y : 0.f);
                o[2] = (__bf16)(ok0 ? t0[u4].z : 0.f); o[3] = (__bf16)(ok0 ? t0[u4].w : 0.f);
                o[4] = (__bf16)(ok1 ? t1[u4].x : 0.f); o[5] = (__bf16)(ok1 ? t1[u4].y : 0.f);
                o[6] = (__bf16)(ok1 ? t1[u4].z : 0.f); o[7] = (__bf16)(ok1 ? t1[u4].w : 0.f);
                qw[idx] = o;
            }
        }
    }
    for (int idx = idx0; idx < 2 * P2 * 64; idx += NT) {
        const int tile = idx >= P2 * 64;
        const int u = idx - tile * P2 * 64;
        const int p = u >> 6, l = u & 63;
        const int b = qbase + (l & 31) + 32 * tile;
        const int col = 16 * p + 8 * (l >> 5);
        float v[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int c = col + 4 * half;
            if (b < a.nq && vec_ok && c + 3 < a.d) {
                const float4 t = *reinterpret_cast<const float4*>(a.q + (int64_t)b * a.d + c);
                v[4 * half + 0] = t.x; v[4 * half + 1] = t.y; v[4 * half + 2] = t.z; v[4 * half + 3] = t.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * half + j] = (b < a.nq && c + j < a.d) ? a.q[(int64_t)b * a.d + c + j] : 0.f;
            }
        }
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
        qw[idx] = o;
    }
}

// The same tile images for EVERY pass of a launch, written once by a small kernel ahead of the scan (multi-pass launches of
// the bf16 kernel): out[pass][idx] = what stage_query_tile puts at qw[idx] for qbase = 64 pass.  The scan's workgroups then
// copy a finished 128 KiB image per pass instead of each converting it from the fp32 queries: with 512 threads the
// conversion was four dependent L2 round trips per pass, with the 256 threads of a small-shard workgroup eight -- 10 us of
// a 50 us pass at 125 k rows per GPU, sixteen times per launch.
__global__ __launch_bounds__(256) void qtile_kernel(const float* __restrict__ q, int nq, int d, int P2, bf16x8* __restrict__ out)
{
    const int per_pass = 2 * P2 * 64;
    const int pass = blockIdx.y, qbase = pass * 64;
    const bool vec_ok = (d & 3) == 0;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < per_pass; idx += gridDim.x * 256) {
        const int tile = idx >= P2 * 64;
        const int u = idx - tile * P2 * 64;
        const int p = u >> 6, l = u & 63;
        const int b = qbase + (l & 31) + 32 * tile;
        const int col = 16 * p + 8 * (l >> 5);
        float v[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int c = col + 4 * half;
            if (b < nq && vec_ok && c + 3 < d) {
                const float4 t = *reinterpret_cast<const float4*>(q + (int64_t)b * d + c);
                v[4 * half + 0] = t.x; v[4 * half + 1] = t.y; v[4 * half + 2] = t.z; v[4 * half + 3] = t.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * half + j] = (b < nq && c + j < d) ? q[(int64_t)b * d + c + j] : 0.f;
            }
        }
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
        out[(size_t)pass * per_pass + idx] = o;
    }
}

// copy of one pass's image into LDS by LDS-DMA: a wave instruction moves 64 consecutive 16-B fragments (1 KiB, lane-linear on
// both sides), every wave issues its whole share before anyone waits -- one round trip per pass, no registers
typedef __attribute__((address_space(3))) void* scan_lds_ptr_t;
template <int NT>
__device__ __forceinline__ void stage_query_tile_image(const bf16x8* __restrict__ img, bf16x8* qw, int P2, int tid)
{
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nchunks = 2 * P2;                       // 1 KiB chunks in the image
    for (int c = wave; c < nchunks; c += NT / 64)
        __builtin_amdgcn_global_load_lds((const void*)(img + (size_t)c * 64 + lane), (scan_lds_ptr_t)(qw + (size_t)c * 64), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the image has landed (and, in order before it, whatever the ring had in flight)
}

// ------------------------------------------------------------------------------------------------------
// K1, the two operand modes (HIPRAG_SCAN_MODE).  Both answer 64 queries per pass against bf16 query tiles, run
// ceil(nq / 64) passes back to back inside one launch (barrier, re-stage the tile, stream the wave's block range again; the
// piece stream is CYCLIC -- the last re-arms of pass p already fetch the first pieces of pass p + 1 -- so HBM keeps
// streaming across the pass boundary and there is no kernel boundary, which would cost 35-60 us of idle GPU), and share the
// tail above.  The X stream is driven by hand: loads are inline asm (invisible to hipcc's waitcnt pass, which otherwise
// drains the queue with vmcnt(0) at the loop back-edge) and every use is fenced by a counted s_waitcnt that takes the ring
// slot as an in/out operand, so no consumer can be scheduled above its wait.  vmcnt(RING - 1) before slot i is exact when
// only the ring is in flight and merely conservative when other operations are queued behind it (loads return in order
// among themselves).  The ring is armed BEFORE the query tile is staged, so HBM is streaming while the prologue runs.
//
//   bf16 (default)  scan_bf16_kernel streams the bf16 FILTER COPY of the rows -- half the bytes of the fp32 rows: per 1 KiB
//                   piece two v_mfma_f32_32x32x16_bf16 (one per 32-query tile), no conversion work.  Both truncations are
//                   carried by the certificate (scan_eps, mode 3): |<x,q> - <x^,q^>| <= |x| |q - q^| + |x - x^| |q^|, both
//                   deviations computed exactly (per query at search time, maximum over rows at add time).
//   q64             scan_split_kernel streams the fp32 rows themselves (N*d*4 bytes per pass, SURVEY 8(d)'s price) and
//                   splits every value on the fly into hi = bf16(v), lo = bf16(v - hi): four MFMAs per pair of fp32
//                   pieces; only the query truncation is left in eps (mode 2).  No extra memory.
// The fp64 re-score and the exhaustive path read the fp32 rows, so both modes return the same exact results.
// ------------------------------------------------------------------------------------------------------
#define HIPRAG_SCAN_PROLOGUE(PIECES_PER_BLOCK, BASE_PTR)                                                                 \
    extern __shared__ float4 qs[];                                                                                       \
    constexpr int NT = NWAVES * 64;                                                                                      \
    const int tid = threadIdx.x;                                                                                         \
    const int lane = tid & 63;                                                                                           \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                           \
    const int P2 = a.P / 2;   /* 16-k-value pieces per block = LDS fragments per query tile */                           \
    /* statically partitioned: a CU that also hosts a tail workgroup of an earlier launch becomes the straggler of the   \
       whole launch, so let the scan's waves win issue arbitration */                                                    \
    __builtin_amdgcn_s_setprio(3);                                                                                       \
    const int64_t gw = (int64_t)blockIdx.x * NWAVES + wave;                                                              \
    const int64_t W = (int64_t)gridDim.x * NWAVES;                                                                       \
    const int64_t bpw = scan_blocks_per_wave(a.nblocks, W);                                                              \
    const int64_t b0 = min(gw * bpw, a.nblocks);                                                                         \
    const int64_t b1 = min(b0 + bpw, a.nblocks);                                                                         \
    const int nbw = (int)(b1 - b0);                                                                                      \
    const int S = nbw * (PIECES_PER_BLOCK);                                                                              \
    const float4* base = (BASE_PTR);                                                                                     \
    if (a.stamps && lane == 0) a.stamps[2 * gw] = wall_clock64();                                                        \
    if (a.gate && tid == 0) {                                                                                            \
        const unsigned long long was = __hip_atomic_fetch_add(a.started, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        if (was + 1 == a.target) __hip_atomic_fetch_max(a.gate, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       \
    }                                                                                                                    \
    TailLds L;                                                                                                           \
    L.stage = reinterpret_cast<Cand*>(reinterpret_cast<char*>(qs) + (size_t)a.P * 1024);                                 \
    L.ctl = reinterpret_cast<u32*>(L.stage + 2 * kStageHalf);                                                            \
    L.bound = L.ctl + 16;                                                                                                \
    if (tid < 16) L.ctl[tid] = 0;                                                                                        \
    const int cls = (int)((gw + blockIdx.x) % a.ncls); /* members of a class on every XCD and every wave slot */           \
    ScanTail T;                                                                                                          \
    T.init()

// pass prologue shared by both kernels: barriers, staged appends of the previous pass -> global lists, new query tile
// pass prologue of both kernels: STAGE_TILE is the statement that writes the pass's query tile
#define HIPRAG_PASS_PROLOGUE(STAGE_TILE)                                                                                 \
    const int qbase = pass * 64;                                                                                         \
    const bool wrap = pass + 1 < npass;                                                                                  \
    int nprev = 0;                                                                                                       \
    u32 total_prev = 0;                                                                                                  \
    if (pass) {                                                                                                          \
        refresh_bounds(a, L, pass - 1, wave, NWAVES, lane); /* its round trip overlaps the wait for the slower waves */  \
        __syncthreads(); /* every wave is done with the previous tile and with the previous pass's staged appends */     \
        total_prev = L.ctl[(pass - 1) & 1];                                                                              \
        nprev = (int)min(total_prev - (((pass - 1) & 1) ? T.flushed1 : T.flushed0), (u32)kStageHalf);                    \
    }                                                                                                                    \
    const FlushTicket ft = flush_begin<NT>(a, L, (pass - 1) & 1, nprev, tid);                                            \
    STAGE_TILE;                                                                                                          \
    flush_end<NT>(a, L, ft, (pass - 1) & 1, nprev, tid);                                                                 \
    if (pass) { if ((pass - 1) & 1) T.flushed1 = total_prev; else T.flushed0 = total_prev; }                             \
    __syncthreads()

#define HIPRAG_SCAN_EPILOGUE()                                                                                           \
    if (S > 0) tail_drain(a, T, L, (npass - 1) & 1, lane, b0, nbw);                                                      \
    refresh_bounds(a, L, npass - 1, wave, NWAVES, lane);                                                                 \
    __syncthreads();                                                                                                     \
    {                                                                                                                    \
        const int hl = (npass - 1) & 1;                                                                                  \
        const int nl = (int)min(L.ctl[hl] - (hl ? T.flushed1 : T.flushed0), (u32)kStageHalf);                            \
        const FlushTicket fl = flush_begin<NT>(a, L, hl, nl, tid);                                                       \
        flush_end<NT>(a, L, fl, hl, nl, tid);                                                                            \
    }                                                                                                                    \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the tail's clamped re-arms are still in flight */                \
    if (a.stamps && lane == 0) a.stamps[2 * gw + 1] = wall_clock64()

template <int METRIC, int NWAVES, int RING, bool MULTI>
__global__ __launch_bounds__(NWAVES * 64) void scan_bf16_kernel(ScanArgs a)
{
    HIPRAG_SCAN_PROLOGUE(P2, reinterpret_cast<const float4*>(a.xh) + b0 * P2 * kPieceVec4);
    const unsigned lane16 = (unsigned)lane * 16u;
    const int h = lane >> 5;
    f32x4 ring[RING];
    if (S > 0) {
#pragma unroll
        for (int i = 0; i < RING; ++i) {
            const unsigned voff = lane16 + (unsigned)min(i, S - 1) * 1024u;
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(ring[i]) : "v"(voff), "s"(base) : "memory");
        }
    }
    const int npass = MULTI ? (a.nq + 63) / 64 : 1;
    const bf16x8* q0 = reinterpret_cast<const bf16x8*>(qs);
    const bf16x8* q1 = q0 + P2 * 64;
    for (int pass = 0; pass < npass; ++pass) {
        HIPRAG_PASS_PROLOGUE(if (MULTI && a.qtile) stage_query_tile_image<NT>(reinterpret_cast<const bf16x8*>(a.qtile) + (size_t)pass * 2 * P2 * 64,
                                                                             reinterpret_cast<bf16x8*>(qs), P2, tid);
                             else stage_query_tile<NT>(a, reinterpret_cast<bf16x8*>(qs), P2, qbase, tid));
        if (S <= 0) continue;

        int s = 0;
        bf16x8 n0v = q0[lane], n1v = q1[lane];   // query fragments are read one piece ahead
        for (int j = 0; j < nbw; ++j) {
            const int64_t blk = b0 + j;
            f32x4 nrm[4];
            if (METRIC == HIPRAG_METRIC_L2) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float* np = a.norms + blk * kRowsPerBlock + 8 * g + 4 * h;
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(nrm[g]) : "v"(np) : "memory");
                }
            }
            f32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
            for (int pp = 0; pp < P2; pp += RING) {
#pragma unroll
                for (int i = 0; i < RING; ++i) {
                    // one step = one 1 KiB piece (16 k-values): two MFMAs (one per query tile), re-arm the ring slot
                    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ring[i]) : "n"(RING - 1) : "memory");
                    const bf16x8 av = __builtin_bit_cast(bf16x8, ring[i]);
                    const bf16x8 bv0 = n0v, bv1 = n1v;
                    int nx = pp + i + 1;
                    nx = nx == P2 ? 0 : nx;
                    n0v = q0[nx * 64 + lane];
                    n1v = q1[nx * 64 + lane];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv1, acc1, 0, 0, 0);
                    // re-arm: past the end of the range the stream wraps to the first pieces of the next pass (S >= RING
                    // whenever S > 0, so one subtraction is enough); the last pass repeats its final piece instead
                    int n0 = s + RING + i;
                    n0 = n0 < S ? n0 : (wrap ? n0 - S : S - 1);
                    const unsigned voff = lane16 + (unsigned)n0 * 1024u;
                    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(ring[i]) : "v"(voff), "s"(base) : "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
                s += RING;
            }
            if (METRIC == HIPRAG_METRIC_L2)   // the norms were issued before this block's P2 >= RING re-arms
                asm volatile("s_waitcnt vmcnt(%4)" : "+v"(nrm[0]), "+v"(nrm[1]), "+v"(nrm[2]), "+v"(nrm[3]) : "n"(RING) : "memory");
            float sec0, sec1;
            int lane_b = lane;
            asm volatile("" : "+v"(lane_b));   // (as in stage_query_tile: keeps the epilogue's lane arithmetic out of the ring loop's live set)
            const float fst0 = block_lane_top2<METRIC>(acc0, nrm, blk, lane_b >> 5, a, sec0);
            const float fst1 = block_lane_top2<METRIC>(acc1, nrm, blk, lane_b >> 5, a, sec1);
            tail_block(a, T, L, fst0, sec0, fst1, sec1, pass, j, nbw, lane_b, wave, NWAVES, cls, b0);
        }
    }  // pass
    HIPRAG_SCAN_EPILOGUE();
}

// query tile of the q64 kernel: for piece pair pp and lane (h, b) the bf16 images of Q[b][16pp + 4h + 0..3] and
// Q[b][16pp + 8 + 4h + 0..3] (the k order the A fragment gets from a PAIR of fp32 pieces), queries qbase + 0..31 then + 32..63;
// hi parts only: |q - bf16(q)| is in the certificate's eps
template <int NT>
__device__ __forceinline__ void stage_query_tile_split(const ScanArgs& a, u32x4* qw, int npairs, int qbase, int tid)
{
    const bool vec_ok = (a.d & 3) == 0;
    int tid_p = tid;
    asm volatile("" : "+v"(tid_p));
    for (int idx = tid_p; idx < 2 * npairs * 64; idx += NT) {
        const int tile = idx >= npairs * 64;
        const int u = idx - tile * npairs * 64;
        const int pp = u >> 6, l = u & 63;
        const int hh = l >> 5;
        const int b = qbase + (l & 31) + 32 * tile;
        float v[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = 8 * (2 * pp + half) + 4 * hh;
            if (b < a.nq && vec_ok && col + 3 < a.d) {
                const float4 t = *reinterpret_cast<const float4*>(a.q + (int64_t)b * a.d + col);
                v[4 * half + 0] = t.x; v[4 * half + 1] = t.y; v[4 * half + 2] = t.z; v[4 * half + 3] = t.w;
            } else {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    v[4 * half + jj] = (b < a.nq && col + jj < a.d) ? a.q[(int64_t)b * a.d + col + jj] : 0.f;
            }
        }
        unsigned h0, h1, h2, h3, l0, l1, l2, l3;
        split_pair(v[0], v[1], h0, l0);
        split_pair(v[2], v[3], h1, l1);
        split_pair(v[4], v[5], h2, l2);
        split_pair(v[6], v[7], h3, l3);
        (void)l0; (void)l1; (void)l2; (void)l3;
        qw[idx] = u32x4{h0, h1, h2, h3};
    }
}

// q64: the fp32 rows, split on the fly.  Data layout: block of 32 rows = P pieces of 1 KiB, piece p, lane slot
// piece_slot(h, r): X[32B + r][8p + 4h + 0..3]; a PAIR of pieces gives a lane the 8 k-values [16pp + 4h + 0..3] and
// [16pp + 8 + 4h + 0..3] of its row -- so the query tile of this kernel holds, for piece pair pp and lane (h, b), the
// bf16 images of Q[b][16pp + 4h + 0..3] and Q[b][16pp + 8 + 4h + 0..3] (k order of the A fragment), staged by its own
// prologue below (not stage_query_tile's 8-consecutive-values order).
template <int METRIC, int NWAVES, int RING, bool MULTI>
__global__ __launch_bounds__(NWAVES * 64) void scan_split_kernel(ScanArgs a)
{
    HIPRAG_SCAN_PROLOGUE(a.P, a.xb + b0 * a.P * kPieceVec4);
    const int npairs = P2;
    const unsigned lane16 = (unsigned)piece_slot(lane >> 5, lane & 31) * 16u;   // this lane's 16 bytes of a piece (A fragment of row lane & 31)
    const int h = lane >> 5;
    f32x4 ring[RING];
    if (S > 0) {
#pragma unroll
        for (int i = 0; i < RING; ++i) {
            const unsigned voff = lane16 + (unsigned)min(i, S - 1) * 1024u;
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(ring[i]) : "v"(voff), "s"(base) : "memory");
        }
    }
    const int npass = MULTI ? (a.nq + 63) / 64 : 1;
    const bf16x8* q0 = reinterpret_cast<const bf16x8*>(qs);
    const bf16x8* q1 = q0 + npairs * 64;
    for (int pass = 0; pass < npass; ++pass) {
        HIPRAG_PASS_PROLOGUE(stage_query_tile_split<NT>(a, reinterpret_cast<u32x4*>(qs), npairs, qbase, tid));
        if (S <= 0) continue;

        int s = 0;
        bf16x8 n0v = q0[lane], n1v = q1[lane];
        for (int j = 0; j < nbw; ++j) {
            const int64_t blk = b0 + j;
            f32x4 nrm[4];
            if (METRIC == HIPRAG_METRIC_L2) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float* np = a.norms + blk * kRowsPerBlock + 8 * g + 4 * h;
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(nrm[g]) : "v"(np) : "memory");
                }
            }
            f32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
            for (int pp = 0; pp < npairs; pp += RING / 2) {
#pragma unroll
                for (int i = 0; i < RING / 2; ++i) {
                    // one step = two 1 KiB pieces (16 k-values per lane half): split, 4 MFMAs, re-arm both ring slots
                    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(ring[2 * i]), "+v"(ring[2 * i + 1]) : "n"(RING - 2) : "memory");
                    const f32x4 v0 = ring[2 * i], v1 = ring[2 * i + 1];
                    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
                    split_pair(v0[0], v0[1], h0, l0);
                    split_pair(v0[2], v0[3], h1, l1);
                    split_pair(v1[0], v1[1], h2, l2);
                    split_pair(v1[2], v1[3], h3, l3);
                    const u32x4 ahi = {h0, h1, h2, h3}, alo = {l0, l1, l2, l3};
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, ahi), al = __builtin_bit_cast(bf16x8, alo);
                    const bf16x8 bv0 = n0v, bv1 = n1v;
                    int nx = pp + i + 1;
                    nx = nx == npairs ? 0 : nx;
                    n0v = q0[nx * 64 + lane];
                    n1v = q1[nx * 64 + lane];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bv0, acc0, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bv0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bv1, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bv1, acc1, 0, 0, 0);
                    int n0 = s + RING + 2 * i, n1 = n0 + 1;
                    n0 = n0 < S ? n0 : (wrap ? n0 - S : S - 1);
                    n1 = n1 < S ? n1 : (wrap ? n1 - S : S - 1);
                    const unsigned voff0 = lane16 + (unsigned)n0 * 1024u;
                    const unsigned voff1 = lane16 + (unsigned)n1 * 1024u;
                    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(ring[2 * i]) : "v"(voff0), "s"(base) : "memory");
                    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(ring[2 * i + 1]) : "v"(voff1), "s"(base) : "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
                s += RING;
            }
            if (METRIC == HIPRAG_METRIC_L2)
                asm volatile("s_waitcnt vmcnt(%4)" : "+v"(nrm[0]), "+v"(nrm[1]), "+v"(nrm[2]), "+v"(nrm[3]) : "n"(RING) : "memory");
            float sec0, sec1;
            int lane_b = lane;
            asm volatile("" : "+v"(lane_b));
            const float fst0 = block_lane_top2<METRIC>(acc0, nrm, blk, lane_b >> 5, a, sec0);
            const float fst1 = block_lane_top2<METRIC>(acc1, nrm, blk, lane_b >> 5, a, sec1);
            tail_block(a, T, L, fst0, sec0, fst1, sec1, pass, j, nbw, lane_b, wave, NWAVES, cls, b0);
        }
    }  // pass
    HIPRAG_SCAN_EPILOGUE();
}

#include "scan_wide.h"   // scan_wide_kernel: 256 queries per read of the filter copy (uses the declarations above)
