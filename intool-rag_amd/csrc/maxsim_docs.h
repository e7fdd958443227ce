// maxsim_docs.h -- the document side of the MaxSim kernels, one struct per format of the multi-vector store (multivec.h):
// how a stored row becomes the A operands of v_mfma_f32_32x32x16_bf16.  maxsim.hip (one query tile, dot_tile) and
// maxsim_search.hip (T query tiles per read of the row, load_chunk / mul_chunk) share them, so both feed the same MFMA the
// same values in the same k order per accumulator: a pair's score has the same bits whichever kernel formed it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "slice_items.h"

namespace hiprag {
namespace mvk {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kRowPad = 16;   // bytes behind every LDS row

__device__ __forceinline__ bf16x8 as_frag(const uint4& v)
{
    union { uint4 u; bf16x8 f; } c;
    c.u = v;
    return c.f;
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// Eight e4m3fn codes (two words, ascending k) times the row's power-of-two scale, as one bf16 MFMA fragment: four
// v_cvt_scalef32_pk_bf16_fp8, each exact (multivec.h), so the fragment holds the bits a bf16 store of the dequantised
// vectors would have given.
__device__ __forceinline__ bf16x8 dequant8(uint32_t w0, uint32_t w1, float scale)
{
    const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, false);
    const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, true);
    const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, false);
    const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, true);
    bf16x8 f;
    f[0] = p0[0]; f[1] = p0[1]; f[2] = p1[0]; f[3] = p1[1];
    f[4] = p2[0]; f[5] = p2[1]; f[6] = p3[0]; f[7] = p3[1];
    return f;
}

// The document side of maxsim_kernel, one struct per format of the store (multivec.h).  dot_tile adds to acc the products of
// stored vector v with the wave's 32 query rows over all of k; lane half h takes its half of every line of the row, against
// my_q, the lane's query row in LDS from byte 64h on.  k goes in one fixed order, chunks of 64 ascending; in chunk c, step t of
// lane half h multiplies k = 64c + 32h + 8t .. + 7.
//
// The multi-tile members (maxsim_scope_kernel) are dot_tile taken apart at its loop: load_chunk is the loads of one trip,
// mul_chunk its MFMAs, issued against each of T query tiles (tile t lies t * tile_bytes behind my_q) into T accumulators.
// Every accumulator sees dot_tile's products in dot_tile's order; the row is loaded once for all T, and the caller may
// hold the next trip's loads in flight while this one multiplies.
struct DocsBf16 {
    const uint16_t* vecs;   // [stored][dim]

    // a 128-byte line is one chunk: the two lanes of a row fetch its two 64-byte halves, four fragments each
    __device__ __forceinline__ void dot_tile(f32x16& acc, int64_t v, int h, const unsigned char* my_q, int dim) const
    {
        const uint4* dp = reinterpret_cast<const uint4*>(vecs) + v * (dim >> 3) + h * 4;
        const int n_chunks = dim >> 6;
        for (int c = 0; c < n_chunks; ++c) {
            const uint4 a0 = dp[c * 8 + 0], a1 = dp[c * 8 + 1], a2 = dp[c * 8 + 2], a3 = dp[c * 8 + 3];
            const uint4* qp = reinterpret_cast<const uint4*>(my_q + c * 128);
            const uint4 b0 = qp[0], b1 = qp[1], b2 = qp[2], b3 = qp[3];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a0), as_frag(b0), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a1), as_frag(b1), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a2), as_frag(b2), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a3), as_frag(b3), acc, 0, 0, 0);
        }
    }

    struct Chunk { uint4 a0, a1, a2, a3; };
    static __device__ __forceinline__ int n_chunks(int dim) { return dim >> 6; }
    __device__ __forceinline__ Chunk load_chunk(int64_t v, int h, int c, int dim) const
    {
        const uint4* dp = reinterpret_cast<const uint4*>(vecs) + v * (dim >> 3) + h * 4 + c * 8;
        return Chunk{dp[0], dp[1], dp[2], dp[3]};
    }
    template <int T>
    __device__ __forceinline__ void mul_chunk(f32x16 (&acc)[T], const Chunk& a, int c, const unsigned char* my_q, int tile_bytes) const
    {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint4* qp = reinterpret_cast<const uint4*>(my_q + t * tile_bytes + c * 128);
            const uint4 b0 = qp[0], b1 = qp[1], b2 = qp[2], b3 = qp[3];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a.a0), as_frag(b0), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a.a1), as_frag(b1), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a.a2), as_frag(b2), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(a.a3), as_frag(b3), acc[t], 0, 0, 0);
        }
    }
};

struct DocsFp8 {
    const unsigned char* codes;   // [stored][dim]
    const float* scales;          // [stored]

    // A 128-byte line holds 128 k-values, two chunks of 64: of every line lane half h reads bytes 32h .. 32h + 31 (chunk 2c)
    // and 64 + 32h .. 64 + 32h + 31 (chunk 2c + 1), four 16-byte loads, so the two lanes of a row still consume whole lines
    // between them, and step t of a chunk multiplies k = 64c + 32h + 8t .. + 7 exactly as DocsBf16 does: the accumulator sees
    // the same products in the same order, and the scores are bit for bit those over a bf16 store of the dequantised vectors.
    __device__ __forceinline__ void dot_tile(f32x16& acc, int64_t v, int h, const unsigned char* my_q, int dim) const
    {
        const uint4* dp = reinterpret_cast<const uint4*>(codes + v * dim) + h * 2;
        const float scale = scales[v];
        const int n_lines = dim >> 7;
        for (int l = 0; l < n_lines; ++l) {
            const uint4 x0 = dp[l * 8 + 0], x1 = dp[l * 8 + 1], y0 = dp[l * 8 + 4], y1 = dp[l * 8 + 5];
            const uint4* qp = reinterpret_cast<const uint4*>(my_q + l * 256);
            const uint4 b0 = qp[0], b1 = qp[1], b2 = qp[2], b3 = qp[3];
            const uint4 b4 = qp[8], b5 = qp[9], b6 = qp[10], b7 = qp[11];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(x0.x, x0.y, scale), as_frag(b0), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(x0.z, x0.w, scale), as_frag(b1), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(x1.x, x1.y, scale), as_frag(b2), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(x1.z, x1.w, scale), as_frag(b3), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(y0.x, y0.y, scale), as_frag(b4), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(y0.z, y0.w, scale), as_frag(b5), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(y1.x, y1.y, scale), as_frag(b6), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(y1.z, y1.w, scale), as_frag(b7), acc, 0, 0, 0);
        }
    }

    // one trip = one line = two chunks of 64 k-values; the row's scale travels with its codes
    struct Chunk { uint4 x0, x1, y0, y1; float scale; };
    static __device__ __forceinline__ int n_chunks(int dim) { return dim >> 7; }
    __device__ __forceinline__ Chunk load_chunk(int64_t v, int h, int l, int dim) const
    {
        const uint4* dp = reinterpret_cast<const uint4*>(codes + v * dim) + h * 2 + l * 8;
        return Chunk{dp[0], dp[1], dp[4], dp[5], scales[v]};
    }
    template <int T>
    __device__ __forceinline__ void mul_chunk(f32x16 (&acc)[T], const Chunk& a, int l, const unsigned char* my_q, int tile_bytes) const
    {
        const float scale = a.scale;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint4* qp = reinterpret_cast<const uint4*>(my_q + t * tile_bytes + l * 256);
            const uint4 b0 = qp[0], b1 = qp[1], b2 = qp[2], b3 = qp[3];
            const uint4 b4 = qp[8], b5 = qp[9], b6 = qp[10], b7 = qp[11];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.x0.x, a.x0.y, scale), as_frag(b0), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.x0.z, a.x0.w, scale), as_frag(b1), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.x1.x, a.x1.y, scale), as_frag(b2), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.x1.z, a.x1.w, scale), as_frag(b3), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.y0.x, a.y0.y, scale), as_frag(b4), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.y0.z, a.y0.w, scale), as_frag(b5), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.y1.x, a.y1.y, scale), as_frag(b6), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dequant8(a.y1.z, a.y1.w, scale), as_frag(b7), acc[t], 0, 0, 0);
        }
    }
};

// Eight e2m1 codes (one word, ascending k: component 2i in the low nibble of byte i) times their block's power-of-two
// scale, as one bf16 MFMA fragment: four v_cvt_scalef32_pk_bf16_fp4, one per byte, each exact (multivec.h).
__device__ __forceinline__ bf16x8 dequant8_fp4(uint32_t w, float scale)
{
    const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
    const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
    const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
    const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
    bf16x8 f;
    f[0] = p0[0]; f[1] = p0[1]; f[2] = p1[0]; f[3] = p1[1];
    f[4] = p2[0]; f[5] = p2[1]; f[6] = p3[0]; f[7] = p3[1];
    return f;
}

struct DocsMxfp4 {
    const unsigned char* codes;    // [stored][dim / 2]
    const unsigned char* scales;   // [stored][dim / 32], e8m0

    // The 32 k-values lane half h multiplies in chunk c, k = 64c + 32h .. + 31, are one MX block: block 2c + h of the row, the
    // 16 bytes of codes at 32c + 16h, word t of them step t.  A trip takes two chunks, 128 k-values, as DocsFp8 does: lane
    // half h loads the 16-byte pieces 4l + h and 4l + 2 + h of the row (the two lanes of a row take 64 consecutive bytes
    // between them) and word l of the row's scales, whose bytes h and 2 + h are the scales of its two blocks -- one aligned
    // 4-byte load per 128 k-values, the same address in both lanes, dim % 128 == 0 making a row's scales whole words.  Step t
    // of a chunk multiplies k = 64c + 32h + 8t .. + 7 exactly as DocsBf16 does: the same products in the same order.
    struct Chunk { uint4 x, y; uint32_t sw; };   // sw: the scale word shifted down by 8h, the lane's two bytes at 0 and 16
    static __device__ __forceinline__ int n_chunks(int dim) { return dim >> 7; }
    __device__ __forceinline__ Chunk load_chunk(int64_t v, int h, int l, int dim) const
    {
        const uint4* dp = reinterpret_cast<const uint4*>(codes + v * (dim >> 1)) + h + l * 4;
        return Chunk{dp[0], dp[2], reinterpret_cast<const uint32_t*>(scales + v * (dim >> 5))[l] >> (8 * h)};
    }

    template <int T>
    __device__ __forceinline__ void mul_chunk(f32x16 (&acc)[T], const Chunk& a, int l, const unsigned char* my_q, int tile_bytes) const
    {
        // the fp32 scales 2^(byte - 127) of the lane's block in the trip's first and second chunk: the byte as exponent field
        const float sx = __uint_as_float((a.sw & 0xFFu) << 23), sy = __uint_as_float(((a.sw >> 16) & 0xFFu) << 23);
        const bf16x8 a0 = dequant8_fp4(a.x.x, sx), a1 = dequant8_fp4(a.x.y, sx), a2 = dequant8_fp4(a.x.z, sx), a3 = dequant8_fp4(a.x.w, sx);
        const bf16x8 a4 = dequant8_fp4(a.y.x, sy), a5 = dequant8_fp4(a.y.y, sy), a6 = dequant8_fp4(a.y.z, sy), a7 = dequant8_fp4(a.y.w, sy);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint4* qp = reinterpret_cast<const uint4*>(my_q + t * tile_bytes + l * 256);
            const uint4 b0 = qp[0], b1 = qp[1], b2 = qp[2], b3 = qp[3];
            const uint4 b4 = qp[8], b5 = qp[9], b6 = qp[10], b7 = qp[11];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, as_frag(b0), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, as_frag(b1), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, as_frag(b2), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, as_frag(b3), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a4, as_frag(b4), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a5, as_frag(b5), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a6, as_frag(b6), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a7, as_frag(b7), acc[t], 0, 0, 0);
        }
    }

    // maxsim_kernel's one query tile: the trips of the row in turn
    __device__ __forceinline__ void dot_tile(f32x16& acc, int64_t v, int h, const unsigned char* my_q, int dim) const
    {
        f32x16 one[1] = {acc};
        const int n_lines = dim >> 7;
        for (int l = 0; l < n_lines; ++l) mul_chunk<1>(one, load_chunk(v, h, l, dim), l, my_q, 0);
        acc = one[0];
    }
};

// The prologue of a work item whose entries are documents (slice_items.h; maxsim_scope_kernel, interaction_kernel), before the
// kernel's barrier: thread g < members writes the query and the clamped vector count of member g ...
__device__ __forceinline__ void item_members(const SliceItem& it, const i64* order, const int32_t* q_counts, int q_stride, int tid,
                                             int* mq, int* mc)
{
    if (tid < it.members) {
        const int qi = (int)order[it.first + tid];
        mq[tid] = qi;
        mc[tid] = min(max(q_counts[qi], 0), q_stride);
    }
}
// ... and thread p < S the first stored vector and the vectors of document p of the slice, 0 vectors outside [p_lo, p_hi)
template <int S>
__device__ __forceinline__ void item_docs(const SliceItem& it, const i64* doc_off, int tid, i64* d_first, int* d_len)
{
    if (tid < S) {
        i64 d0 = 0;
        int ld = 0;
        if (tid >= it.p_lo && tid < it.p_hi) {     // hi <= documents: both offsets exist
            d0 = doc_off[it.base + tid];
            ld = (int)(doc_off[it.base + tid + 1] - d0);
        }
        d_first[tid] = d0;
        d_len[tid] = ld;
    }
}

}  // namespace mvk
}  // namespace hiprag
