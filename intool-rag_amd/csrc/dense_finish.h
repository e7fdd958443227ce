// dense_finish.h -- K2 and K3 of the flat index (overview: dense_index.hip): the certificate's slack (scan_eps), fin_kernel
// (rank the candidate list, fp64 re-score, extension, certificate), flag_all_kernel, exhaustive_kernel for flagged queries
// and the start gate's wait.  Device text for ONE translation unit, included by dense_index.hip behind dense_scan.h (Cand,
// kCandCap) inside its namespaces.
#pragma once

constexpr int kSelThreads = 256;
constexpr int kExRows = 1024;      // rows per workgroup in the exhaustive path (16 KiB of LDS)

// Certificate slack: |scan value - exact score| <= eps for every row, on the scale the scan selects by (IP: <x,q>;
// L2: 2<x,q> - |x|^2 = |q|^2 - dist).  Terms: fp32 accumulation ((d_pad + 80) u, u = 2^-24, incl. the split's extra
// roundings), the operand truncations of the mode, and the quad tag in the two low mantissa bits (kTagSlack of the value's
// magnitude).
constexpr double kTagSlack = 4.76837158203125e-07;  // 2^-21
template <int METRIC>
__device__ __forceinline__ double scan_eps(int dpad, int mode, double qn2, double xn2, double dq2, double dx2)
{
    const double xn = sqrt(xn2), qn = sqrt(qn2);
    const double u = 5.9604644775390625e-08;  // 2^-24
    double eps = 1.05 * (double)(dpad + 80) * u * qn * xn;
    // q64: the scan sees q^ = bf16(q) and x^ = hi + lo.  |<x, q - q^>| <= |x| |q - q^| (Cauchy-Schwarz) with |q - q^| computed
    // exactly per query (dq2, same RNE conversion as the scan prologue) -- about 0.3 * 2^-9 |q| for ordinary data instead of the
    // element-wise worst case 2^-9 |q|; |<x - x^, q^>| <= 2^-17 |x| |q^| for the two-term split of the rows.
    if (mode == 2) eps += 7.62939453125e-06 * 1.01 * qn * xn + 1.0001 * sqrt(dq2) * xn;
    // bf16 filter copy: |<x, q> - <x^, q^>| <= |x| |q - q^| + |x - x^| |q^|, |q^| <= |q| + |q - q^|; dx2 = max over rows
    if (mode == 3) eps += 1.0001 * (sqrt(dq2) * xn + sqrt(dx2) * (qn + sqrt(dq2)));
    if (METRIC == HIPRAG_METRIC_IP) return eps + kTagSlack * (qn * xn + eps);
    eps = 2.0 * eps + 4.0 * u * (xn * xn + qn * xn) + 4.0 * u * qn2;  // 2 * acc - norm, and the rounding of |q|^2 - dist
    return eps + kTagSlack * (2.0 * qn * xn + xn * xn + eps);
}
// k-th exact score (ordered key) on the scan's scale; -inf while fewer than k rows are known
template <int METRIC>
__device__ __forceinline__ double kth_on_scan_scale(u64 kth_key, double qn2)
{
    if (kth_key == 0) return -INFINITY;
    return METRIC == HIPRAG_METRIC_IP ? unord64(kth_key) : qn2 - (-unord64(kth_key));
}

template <int METRIC>
__device__ __forceinline__ void write_result(double* out64, float* out32, int64_t* out_ids, int64_t o, u64 key, i64 id,
                                             int64_t id_base)
{
    double s;
    if (key == 0) {
        s = METRIC == HIPRAG_METRIC_IP ? -DBL_MAX : DBL_MAX;
        out_ids[o] = -1;
        if (out32) out32[o] = METRIC == HIPRAG_METRIC_IP ? -FLT_MAX : FLT_MAX;
    } else {
        s = METRIC == HIPRAG_METRIC_IP ? unord64(key) : -unord64(key);
        out_ids[o] = id + id_base;
        if (out32) out32[o] = (float)s;
    }
    out64[o] = s;
}

// ------------------------------------------------------------------------------------------------------
// K2: the finish -- ONE kernel, one 8-wave workgroup per query (rounds 1-2 took seven launches: select, re-score,
// final, three for "round B", exhaustive check):
//   1. the query's candidate list -> LDS, dropping entries below the final thetac (they cannot matter: either the
//      certificate holds with thetac as the bound of everything unseen, or the query goes to the exhaustive path);
//   2. rank by counting (keys are distinct: they carry the group id) -> sorted list;
//   3. re-score the tagged quad of the best R0 = k + max(8, k/2) groups in fp64 from the fp32 rows, exact top-k of those
//      rows under (score, id);
//   4. EXTEND: tau = (k-th exact score so far) - eps; every group on the list with first >= tau is re-scored as well
//      (the list is sorted, so that is a prefix; the k-th score only rises afterwards, so one extension suffices) -- what
//      rounds 1-2 did with a fixed K' and a second round of three kernels, and why k = 50 needed that round for every query;
//   5. groups whose `second` could still reach the k-th score get their other three quads re-scored (rare);
//   6. CERTIFICATE: every row that was not re-scored has scan value <= m = max(first of the best group not re-scored,
//      final thetac), hence exact score <= m + eps, eps a worst-case bound (scan_eps).  If the k-th exact score is not
//      > m + eps -- massive ties, e.g. the zero vector the reference returns for empty text (hf/embeddings.py:47-48), a list
//      that overflowed, or more than kMaxRescore groups within eps -- the query is flagged for the exhaustive path.
//   7. the workgroup leaves the query's scan state (count, thetac, class slots) zeroed for the next launch of the slot.
// ------------------------------------------------------------------------------------------------------
constexpr int kListLds = kNoFilterGroups;   // groups of one query the finish ranks in LDS
constexpr int kMaxRescore = 192;            // groups re-scored (tagged quads) per query
constexpr int kMaxExpand = 24;              // groups whose other three quads are re-scored
constexpr int kFinThreads = 512;            // 8 waves and <= 40 KiB of LDS, two workgroups per CU (see fin_kernel): the 1024 queries of a small-shard
                                            // launch are finished in ONE round of workgroups (16 waves / 55 KiB: two rounds, 0.14 ms)
constexpr int kCandRows = 4 * kMaxRescore + 12 * kMaxExpand;

struct FinArgs {
    const float4* xb;
    const float* q;            // [nq, d]
    const unsigned* max_norm2_bits;  // [0] max |x|^2, [1] max |x - bf16(x)|^2 (float bits)
    double* out64;             // [nq, k]
    float* out32;              // [nq, k] or null
    int64_t* out_ids;          // [nq, k]
    int* flags;                // [nq]
    int* host_flags;           // [nq] a copy of the flags in pinned host memory, or null (hipidx_search's one-query path)
    int* arrivals;             // [nq] exhaustive-path arrival counters, zeroed here
    unsigned long long* fallback_counter;   // queries sent to the exhaustive path
    unsigned long long* extend_counter;     // queries whose re-scored prefix had to be extended (step 4)
    unsigned long long* work_counters;      // [3] sums over queries: list entries written by the scan, entries ranked, groups re-scored
    u32* slots;
    u32* thetac;
    u32* count;
    const Cand* list;
    int64_t ntotal, id_base;
    int d, P, k, mode, filter;
};

// NT threads: 512 (8 waves) for shallow k, 1024 (16 waves) for k >= 32, where re-scoring k + k/2 groups one after the other
// in 8 waves is most of a finish workgroup's time (k = 50: 229 us per 256-query launch with 8 waves).
template <int METRIC, int NT>
// (NT, 4): four waves per SIMD, i.e. TWO of these 8-wave workgroups per CU.  Left alone the compiler takes 142
// VGPRs -- three waves per SIMD, ONE workgroup per CU -- and a finish workgroup is a ~0.15 ms chain of dependent steps
// that only other workgroups on the CU can hide: on the CUs the next scan leaves it the finish of 1024
// queries then lasted as long as the scan itself.  128 VGPRs cost 36 bytes of scratch per lane.
__global__ __launch_bounds__(NT, 4) void fin_kernel(FinArgs a)
{
    __shared__ float qv[kMaxDPad];
    // the unsorted list (lkey / lsec) is dead once it has been ranked into skey / ssec: the re-scored rows (ck / ci) overlay it
    constexpr int kOverlay = kCandRows * 16 > kListLds * 12 ? kCandRows * 16 : kListLds * 12;
    __shared__ __attribute__((aligned(16))) unsigned char overlay[kOverlay];
    u64* lkey = reinterpret_cast<u64*>(overlay);
    float* lsec = reinterpret_cast<float*>(overlay + kListLds * 8);
    u64* ck = reinterpret_cast<u64*>(overlay);
    i64* ci = reinterpret_cast<i64*>(overlay + kCandRows * 8);
    __shared__ u64 skey[kListLds];
    __shared__ float ssec[kListLds];
    __shared__ u64 tk[kMaxKFast];
    __shared__ i64 ti[kMaxKFast];
    __shared__ double dred[32];
    __shared__ int expand[kMaxExpand];
    __shared__ int s_n, s_r1, s_expand;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = blockIdx.x;
    const int dpad = a.P * 8;
    const int k = a.k;

    // query into LDS (zero padded), its exact |q|^2 and |q - bf16(q)|^2 (the scan's query tile holds bf16(q), RNE)
    double qpart = 0.0, dpart = 0.0;
    for (int c = tid; c < dpad; c += NT) {
        const float vf = c < a.d ? a.q[(int64_t)q * a.d + c] : 0.f;
        qv[c] = vf;
        const double v = (double)vf, dv = v - (double)(float)(__bf16)vf;
        qpart += v * v;
        dpart += dv * dv;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { qpart += __shfl_xor(qpart, off); dpart += __shfl_xor(dpart, off); }
    if (lane == 0) { dred[wave] = qpart; dred[16 + wave] = dpart; }   // NT / 64 <= 16 waves
    if (tid == 0) { s_n = 0; s_r1 = 0; s_expand = 0; }
    if (tid < k) { tk[tid] = 0; ti[tid] = -1; }
    const u32 cnt_raw = a.count[q];
    const u32 theta = a.filter ? a.thetac[q] : 0u;
    __syncthreads();
    double qn2 = 0.0, dq2 = 0.0;
    for (int w = 0; w < NT / 64; ++w) { qn2 += dred[w]; dq2 += dred[16 + w]; }
    const double eps = scan_eps<METRIC>(dpad, a.mode, qn2, (double)__uint_as_float(a.max_norm2_bits[0]), dq2,
                                        (double)__uint_as_float(a.max_norm2_bits[1]));

    // 1. list -> LDS
    const int n_in = (int)min(cnt_raw, (u32)kCandCap);
    const Cand* src = a.list + (size_t)q * kCandCap;
    for (int i = tid; i < n_in; i += NT) {
        const Cand e = src[i];
        if ((u32)(e.key >> 32) >= theta) {
            const int p = atomicAdd(&s_n, 1);
            if (p < kListLds) { lkey[p] = e.key; lsec[p] = e.sec; }
        }
    }
    __syncthreads();
    // 7. (early: everything of the scan state has been read) leave the slot clean for its next launch
    if (tid == 0) { a.count[q] = 0; a.thetac[q] = 0; }
    if (tid < kClasses) a.slots[((size_t)(q >> 6) * kClasses + tid) * 64 + (q & 63)] = 0;
    const int n = s_n;
    bool flag = cnt_raw > (u32)kCandCap || n > kListLds;
    int R = 0;
    bool extended = false;
    u64 kth_key = 0;

    // rows of groups [g0, g1) of the sorted list -> ck / ci[4j ..]
    auto rescore_groups = [&](int g0, int g1) {
        for (int j = g0 + wave; j < g1; j += NT / 64) {
            const u64 e = skey[j];
            const u32 gid = packed_index(e);
            const int g = (int)(__float_as_uint(packed_value(e)) & 3u);
            const int64_t blk = gid >> 1;
            const int r0 = 8 * g + 4 * (int)(gid & 1);
            const double s = rescore4<METRIC>(a.xb, a.P, blk, r0, qv);
            const i64 row = blk * kRowsPerBlock + r0 + (lane & 3);
            if (lane < 4) {
                ck[4 * j + lane] = row < a.ntotal ? ord64(METRIC == HIPRAG_METRIC_IP ? s : -s) : 0ull;
                ci[4 * j + lane] = row;
            }
        }
    };
    // exact top-k of ck / ci[0 .. nc) under (key desc, id asc) by counting -> tk / ti (cleared first); returns the k-th key
    auto topk_rows = [&](int nc) -> u64 {
        __syncthreads();
        if (tid < k) { tk[tid] = 0; ti[tid] = -1; }
        __syncthreads();
        for (int i = tid; i < nc; i += NT) {
            const u64 mk = ck[i];
            if (mk == 0) continue;
            const i64 mi = ci[i];
            int r = 0;
            for (int j = 0; j < nc; ++j) {
                const u64 ok = ck[j];
                r += (ok > mk || (ok == mk && ci[j] < mi)) ? 1 : 0;
            }
            if (r < k) { tk[r] = mk; ti[r] = mi; }
        }
        __syncthreads();
        return tk[k - 1];
    };

    if (!flag) {
        // 2. rank by counting
        for (int i = tid; i < n; i += NT) {
            const u64 mine = lkey[i];
            int r = 0;
            for (int j = 0; j < n; ++j) r += lkey[j] > mine ? 1 : 0;
            skey[r] = mine;
            ssec[r] = lsec[i];
        }
        __syncthreads();
        // 3. first batch
        const int R0 = min(n, k + max(8, k >> 1));
        rescore_groups(0, R0);
        R = R0;
        kth_key = topk_rows(4 * R);
        // 4. extend to every listed group that can still matter
        {
            const double t = kth_on_scan_scale<METRIC>(kth_key, qn2) - eps;
            float tf = t > -3.0e38 ? (float)t : -FLT_MAX;
            if ((double)tf > t) tf = nextafterf(tf, -INFINITY);
            for (int j = R0 + tid; j < n; j += NT)
                if (packed_value(skey[j]) >= tf) atomicMax(&s_r1, j + 1);
            __syncthreads();
            const int R1 = s_r1;
            if (R1 > R0) {
                extended = true;
                if (R1 > kMaxRescore) flag = true;
                else {
                    rescore_groups(R0, R1);
                    R = R1;
                    kth_key = topk_rows(4 * R);
                }
            }
        }
    }
    if (!flag) {
        // 5. other quads of groups whose `second` could still reach the k-th score
        const double kth = kth_on_scan_scale<METRIC>(kth_key, qn2);
        for (int j = tid; j < R; j += NT) {
            const float m2 = ssec[j];
            if (m2 > -1.0e38f && !(kth > (double)m2 + eps)) {
                const int p = atomicAdd(&s_expand, 1);
                if (p < kMaxExpand) expand[p] = j;
            }
        }
        __syncthreads();
        const int ne = s_expand;
        if (ne > kMaxExpand) flag = true;
        else if (ne > 0) {
            for (int x = wave; x < ne; x += NT / 64) {
                const u64 e = skey[expand[x]];
                const u32 gid = packed_index(e);
                const int tagged = (int)(__float_as_uint(packed_value(e)) & 3u);
                const int64_t blk = gid >> 1;
                int o = 4 * R + 12 * x;
                for (int g = 0; g < 4; ++g) {
                    if (g == tagged) continue;
                    const int r0 = 8 * g + 4 * (int)(gid & 1);
                    const double s = rescore4<METRIC>(a.xb, a.P, blk, r0, qv);
                    const i64 row = blk * kRowsPerBlock + r0 + (lane & 3);
                    if (lane < 4) {
                        ck[o + lane] = row < a.ntotal ? ord64(METRIC == HIPRAG_METRIC_IP ? s : -s) : 0ull;
                        ci[o + lane] = row;
                    }
                    o += 4;
                }
            }
            kth_key = topk_rows(4 * R + 12 * ne);
        }
    }
    if (!flag) {
        // 6. certificate
        float m = R < n ? packed_value(skey[R]) : -FLT_MAX;
        if (theta != 0) m = fmaxf(m, unord32(theta));
        if (m > -1.0e38f && !(kth_on_scan_scale<METRIC>(kth_key, qn2) > (double)m + eps)) flag = true;
    }
    if (tid < k) write_result<METRIC>(a.out64, a.out32, a.out_ids, (int64_t)q * k + tid, tk[tid], ti[tid], a.id_base);
    if (tid == 0) {
        a.flags[q] = flag ? 1 : 0;
        if (a.host_flags) a.host_flags[q] = flag ? 1 : 0;
        a.arrivals[q] = 0;
        if (flag) atomicAdd(a.fallback_counter, 1ull);
        else if (extended) atomicAdd(a.extend_counter, 1ull);
        atomicAdd(a.work_counters + 0, (unsigned long long)cnt_raw);
        atomicAdd(a.work_counters + 1, (unsigned long long)n);
        atomicAdd(a.work_counters + 2, (unsigned long long)R);
    }
}

// For k beyond what the finish holds every query goes straight to the exhaustive path: exact, just not fast -- k in the
// hundreds is outside anything the reference asks for (top_chunks = 50, page_retriever.py:81).
__global__ void flag_all_kernel(int* flags, int* arrivals, unsigned long long* fallback_counter, int nq)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) {
        flags[q] = 1;
        arrivals[q] = 0;
        atomicAdd(fallback_counter, 1ull);
    }
}

// ------------------------------------------------------------------------------------------------------
// K2c / K2d: exhaustive exact path for flagged queries (exit immediately otherwise)
// ------------------------------------------------------------------------------------------------------
struct ExArgs {
    const float4* xb;
    const float* q;
    const int* flags;
    int* arrivals;  // [nq] zeroed by the finish kernel of the same pass
    u64* ek;        // [nq, nslices*kk]
    i64* ei;
    double* out64;
    float* out32;
    int64_t* out_ids;
    int64_t ntotal, id_base;
    int d, P, k, kk, nslices, nq;
};

// One launch: workgroup s re-scores rows [s*kExRows, +kExRows) of every FLAGGED query in fp64 and publishes its best
// kk; the last workgroup to arrive for a query (device-scope counter behind __threadfence) merges the slices and
// overwrites the query's results.  Unflagged passes cost one tiny launch: every workgroup reads nq flags and exits.
template <int METRIC>
__global__ __launch_bounds__(kSelThreads) void exhaustive_kernel(ExArgs a)
{
    extern __shared__ unsigned char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    i64* ids = reinterpret_cast<i64*>(keys + kExRows);
    u64* selk = reinterpret_cast<u64*>(ids + kExRows);
    i64* seli = reinterpret_cast<i64*>(selk + a.k);
    KeyId* red = reinterpret_cast<KeyId*>(seli + a.k);
    float* qv = reinterpret_cast<float*>(red + 2 * (kSelThreads / 64));
    int* ticket = reinterpret_cast<int*>(qv + a.P * 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dpad = a.P * 8;
    int mine = 0;
    for (int q = tid; q < a.nq; q += kSelThreads) mine |= a.flags[q];
    if (!__syncthreads_or(mine)) return;  // the common case: a <= n_cu-workgroup launch that reads nq flags and leaves
    for (int slice = blockIdx.x; slice < a.nslices; slice += gridDim.x) {
        const int64_t row_base = (int64_t)slice * kExRows;
        const int nrows = (int)min((int64_t)kExRows, a.ntotal - row_base);
        for (int q = 0; q < a.nq; ++q) {
            if (!a.flags[q]) continue;  // uniform across the workgroup
            __syncthreads();
            for (int c = tid; c < dpad; c += kSelThreads) qv[c] = c < a.d ? a.q[(int64_t)q * a.d + c] : 0.f;
            __syncthreads();
            for (int g = wave; g * 4 < kExRows; g += kSelThreads / 64) {
                const int64_t row0 = row_base + (int64_t)g * 4;
                u64 key = 0;
                const int64_t row = row0 + (lane & 3);
                if (row0 < a.ntotal) {
                    const double s = rescore4<METRIC>(a.xb, a.P, row0 / kRowsPerBlock, (int)(row0 % kRowsPerBlock), qv);
                    if (row < a.ntotal) key = ord64(METRIC == HIPRAG_METRIC_IP ? s : -s);
                }
                if (lane < 4) { keys[g * 4 + lane] = key; ids[g * 4 + lane] = row; }
            }
            __syncthreads();
            const int64_t M = (int64_t)a.nslices * a.kk;
            u64* ok = a.ek + (int64_t)q * M + (int64_t)slice * a.kk;
            i64* oi = a.ei + (int64_t)q * M + (int64_t)slice * a.kk;
            wg_topk_rounds<kSelThreads>(keys, ids, max(nrows, 0), a.kk, red, [&](int r, u64 k, i64 id) { ok[r] = k; oi[r] = id; });
            // Publish this slice, then take a ticket (cdna_hip_programming.md Guideline 16, counter form): stores drained
            // by their wave -> workgroup barrier -> one lane: agent-scope release, explicit drain, relaxed agent atomic.
            // The last arriver acquires once, and the barrier after it holds every wave's loads behind the invalidate.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int t = __hip_atomic_fetch_add(a.arrivals + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t == a.nslices - 1) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                *ticket = t;
            }
            __syncthreads();
            if (*ticket == a.nslices - 1) {  // last arriver merges
                const u64* sk = a.ek + (int64_t)q * M;
                const i64* si = a.ei + (int64_t)q * M;
                wg_stream_topk<kSelThreads, kExRows>([&](i64 i, u64& k, i64& id) { k = sk[i]; id = si[i]; }, M, a.k, keys, ids,
                                                     red, selk, seli);
                for (int r = tid; r < a.k; r += kSelThreads)
                    write_result<METRIC>(a.out64, a.out32, a.out_ids, (int64_t)q * a.k + r, selk[r], seli[r], a.id_base);
            }
        }
    }
}

// The start gate's wait (hipidx_gate_tail_dev): one wave polls the gate word -- memory-side reads, a plain load could be
// served from a stale L2 line for ever -- until the awaited scan has raised it, or until the bound is up.  The bound is
// what makes the gate safe where kernels are serialised (a profiler collecting counters, AMD_SERIALIZE_KERNEL, a debugger):
// there the awaited scan cannot start while this kernel runs, and an unbounded wait (hipStreamWaitValue64, which this
// replaces: it hung a --pmc collection) would never end.  The gate opens ~30 us after the previous scan has ended -- which
// the stream has waited for before it gets here -- so 1 ms of the 100 MHz wall clock is far beyond any real wait; a gate that
// times out only costs the overlap it was there for.
constexpr unsigned long long kGateTimeoutTicks = 100000ull;
__global__ __launch_bounds__(64) void gate_wait_kernel(unsigned long long* gate, unsigned long long target)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_fetch_or(gate, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        if (wall_clock64() - t0 > kGateTimeoutTicks) break;
        __builtin_amdgcn_s_sleep(20);
    }
}
