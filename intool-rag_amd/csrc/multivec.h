// multivec.h -- struct MultiVecStore, shared by multivec.hip (the hipmv_* entries) and maxsim.hip (which reads the CSR and
// keeps the workspace of its calls here, because hipmaxsim_info is asked of the store).
//
// SIZE: a stored token costs 2 x dim bytes in the bf16 format (0): 100 k passages of 120 tokens at 1024-d take 24.6 GB, 1 M
// passages 245 GB, which do not fit beside the index.  The fp8 format (1) stores OCP e4m3fn codes with one power-of-two
// fp32 scale per vector, dim + 4 bytes per token: 12.3 GB and 123 GB for the same two collections.  The MXFP4 format (4)
// stores e2m1 codes with one e8m0 scale per 32 components, dim / 2 + dim / 32 bytes per token (544 at 1024-d): 6.5 GB and 65 GB.
//
// THE FP8 FORMAT, per stored vector v[dim] of bf16 values (hiprag.colbert.fp8_quantize_reference restates it in numpy):
//   amax = max_k |v_k|.  amax == 0: codes 0x00, scale 1.0f.  A non-finite component, or amax outside [2^-60, 2^60]: stored
//   as the zero vector with scale 1.0f, and counted (hipmv_format_info).  Otherwise e = 7 - floor(log2 amax), read off amax's
//   exponent bits; code_k = e4m3fn(v_k * 2^e), round to nearest even (the product is exact in fp32 and at most 256 < 448: no
//   saturation), a -0 code stored as 0x00; scale = 2^-e.  code * scale is exact in bf16.
//
// THE MXFP4 FORMAT (4: bits per element; OCP microscaling FP4), dim % 128 == 0 in 128..1024 so that a vector's scales are whole
// 32-bit words and its codes whole 16-byte pieces.  Per stored vector: codes uint8 [dim / 2], component 2i in the low nibble
// of byte i and component 2i + 1 in the high one, a nibble = sign | 2 exponent bits | 1 mantissa bit (e2m1: magnitudes 0, 0.5,
// 1, 1.5, 2, 3, 4, 6); scales uint8 [dim / 32], e8m0: byte s means 2^(s - 127).  dim / 2 + dim / 32 bytes per token: 544 at
// 1024-d, 6.5 GB for 100 k passages of 120 tokens and 65 GB for 1 M.  Quantisation of v[dim]
// (hiprag.colbert.mxfp4_quantize_reference restates it in numpy):
//   the vector guard is the fp8 format's: a non-finite component, or amax outside [2^-60, 2^60], stores the zero vector (codes
//   0x0, scale bytes 127) and is counted; amax == 0 gives the zero vector uncounted.  Otherwise per block of 32 consecutive
//   components: bmax == 0: codes 0, scale byte 127.  Else E = max(floor(log2 bmax) - 2, -100), the floor read off bmax's
//   exponent bits (a bmax below 2^-98, bf16 subnormals included, takes -100); scale byte = E + 127, in [27, 185];
//   code_k = e2m1(v_k * 2^-E), round to nearest, ties to the even mantissa, SATURATING at +-6 (the OCP MX rule: the scaled
//   block maximum lies in [4, 8), a value in [7, 8) becomes 6); a -0 code is stored as 0x0.
//   code * 2^E is exact in bf16 (2 significant bits, magnitude in [2^-101, 6 * 2^58]), so v_cvt_scalef32_pk_bf16_fp4 with the
//   fp32 scale of bits byte << 23 dequantises exactly.  |v - deq| <= max(|v| / 4, 2^(E - 2)).
#pragma once
#include "dense_internal.h"
#include "doc_store.h"

namespace hiprag {

constexpr int32_t kMvBf16 = 0, kMvFp8 = 1, kMvMxfp4 = 4;   // 2 and 3 are no formats

struct MaxsimSearchWs;
struct MaxsimPrunedWs;

// What both scoped MaxSim searches (maxsim_search.hip, which has the bodies, and maxsim_codes.hip) keep with the store, each in
// a workspace of its own made on first use.
struct MaxsimWsBase {
    ScopeUpload sc;
    DevBuf counters;            // uint64 {valid pairs, padding pairs, document vectors | codes read}
    DevBuf o64;                 // the merge's fp64 scores
    DevBuf hq, hc, hos, hoi;    // the host entry's device copies
    int n_cu = 0;
    // n_cu on first use; slice_begin (dense_internal.h) and three zero counters on `st`
    int32_t begin(int device, const SlicePlan& P, int qchunk, hipStream_t st);
    // the host entries' frame: q_vecs / q_counts into hq / hc, room for [nq][k] results in hos / hoi; behind the search, whose
    // result is rc (a failed one is synchronised, not copied), scores and ids back to the caller
    int32_t stage(const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride, int32_t nq, int32_t k, int32_t dim);
    int32_t give_back(int32_t rc, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids);
};
constexpr int kMaxsimMaxQStride = 512;
// the rules on a query batch both searches share, behind each one's own on nq and k
int32_t check_maxsim_shape(int32_t q_stride, int32_t n_scopes, int64_t id_base);

struct MultiVecStore {
    std::mutex mu;
    int device = 0;
    int32_t dim = 0;
    DocCsr csr{"multi-vector store"};         // items = vectors, doc_cap = max_doc_vectors
    int32_t format = 0;                       // kMvBf16, kMvFp8 or kMvMxfp4, fixed at creation
    DevBuf vecs;                              // format 0: bf16 [csr.cap_items][dim]
    DevBuf codes, scales;                     // format 1: uint8 [csr.cap_items][dim] | float [csr.cap_items]
                                              // format 4: uint8 [csr.cap_items][dim / 2] | uint8 [csr.cap_items][dim / 32]
    DevBuf guarded;                           // formats 1, 4: uint64 {vectors stored as zero by the domain guard since creation}

    // The per-vector arrays of this store's format, in the order of its file: all that capacity, removal, save and load know
    // of a format.  The last part is the large one.
    StoreParts parts()
    {
        if (format == kMvFp8) return StoreParts{2, {{&scales, sizeof(float)}, {&codes, (size_t)dim}}};
        if (format == kMvMxfp4) return StoreParts{2, {{&scales, (size_t)dim / 32}, {&codes, (size_t)dim / 2}}};
        return StoreParts{1, {{&vecs, (size_t)dim * 2}, {nullptr, 0}}};
    }

    // ---- centroid codes (maxsim_codes.hip), optional: ncent == 0 is a store without them --------------------------------
    int32_t ncent = 0;
    DevBuf centroids;                         // bf16 [ncent][dim]
    DevBuf cent_codes;                        // int32 [csr.cap_items]: the code of every stored vector, at the vectors' own offsets
    // What capacity and removal see: parts(), and in front of them the codes of an attached store, which grow and move with
    // the vectors.  Files and formats know parts() alone.
    StoreParts item_parts()
    {
        StoreParts p = parts();
        if (ncent == 0) return p;
        for (int i = p.n; i > 0; --i) p.p[i] = p.p[i - 1];
        p.p[0] = StorePart{&cent_codes, sizeof(int32_t)};
        ++p.n;
        return p;
    }
    std::shared_ptr<MaxsimPrunedWs> pruned_ws;   // workspace of hipmaxsim_search_pruned* (maxsim_codes.hip)

    // ---- workspace of the MaxSim calls on this store (maxsim.hip) ------------------------------------------------------
    DevBuf pair_scores;                       // float [pairs] when the caller wants none
    DevBuf counters;                          // uint64 {valid pairs, padding candidates, document vectors read}
    bool lds_opted_in = false;                // the kernel's dynamic LDS bound was raised on this device
    // workspace and counters of hipmaxsim_search_scoped* (maxsim_search.hip, which defines and makes it on first use)
    std::shared_ptr<MaxsimSearchWs> search_ws;
};

Registry<MultiVecStore>& mv_reg();   // multivec.hip

// maxsim_codes.hip: the codes of stored vectors [v0, v1) of an attached store into cent_codes, on `st`; the vectors are in
// place (an append calls it behind its quantisation, before it commits).  The store's mutex is held.
int32_t mv_code_range(MultiVecStore& s, int64_t v0, int64_t v1, hipStream_t st);
// maxsim.hip: hipmaxsim_dev under the store's mutex, for the exact stage of hipmaxsim_search_pruned*
int32_t maxsim_candidates(MultiVecStore& s, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                          const int64_t* cand_dev, int32_t depth, int64_t id_base, int32_t k, float* out_scores_dev,
                          int64_t* out_ids_dev, hipStream_t st);

#define GET_MV(var, h) HR_GET_HANDLE(var, mv_reg(), h, "unknown multi-vector store handle %llu", (unsigned long long)(h))

}  // namespace hiprag
