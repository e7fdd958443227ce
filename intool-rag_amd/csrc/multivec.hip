// multivec.hip -- the multi-vector store (hipmv_*, include/hiprag.h): a device-resident CSR of the per-token (ColBERT)
// vectors of every chunk of a collection, document i = collection row i: offsets int64 [docs + 1] and the per-vector arrays
// of the store's format.  It is what the late-interaction call (maxsim.hip) scores candidates from.  It follows the
// collection as rows, IVF lists, postings, passage tokens and pages do -- append at the end, stable compaction on removal --
// as a DocCsr (doc_store.h), the token store's document CSR and mover.  Unlike tokens, these vectors cannot be
// rebuilt without encoding the collection again: the store has a file.  A store has one of three formats, fixed at creation
// (multivec.h): bf16 vectors (file HIPMV001), e4m3fn codes with one power-of-two scale per vector (file HIPMVQ81), or MXFP4,
// e2m1 codes with one e8m0 scale per block of 32 (file HIPMVQ41), quantised as they are appended.  Capacity, removal, save
// and load go over MultiVecStore::parts() and do not ask for the format; it is tested where the formats do different work:
// quantising, dequantising and validating a file's scales and codes.
#include <algorithm>
#include <cstring>

#include "multivec.h"

namespace hiprag {

Registry<MultiVecStore>& mv_reg()
{
    static Registry<MultiVecStore> r;
    return r;
}
size_t clear_multivec_registry() { return mv_reg().clear(); }

namespace {

constexpr int kPackThreads = 64;
constexpr int kMaxDim = 1024;
constexpr size_t kIoChunk = 64u << 20;   // bytes of host staging for save / load
constexpr char kMagic[8] = {'H', 'I', 'P', 'M', 'V', '0', '0', '1'};
constexpr int32_t kVersion = 1;

// The document of stored vector v of a batch: the last one with off[doc] <= v (`off` = the store's offsets from the first
// new document on, n_docs + 1 entries, already final).
__device__ __forceinline__ int64_t doc_of_vector(const int64_t* __restrict__ off, int64_t n_docs, int64_t v)
{
    int64_t lo = 0, hi = n_docs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One workgroup per stored vector v0 <= v < v1 of the batch: its source row is src[doc][v - off[doc]].  16 bytes per thread
// and step.
__global__ __launch_bounds__(kPackThreads) void mv_pack_kernel(const uint4* __restrict__ src, int64_t row_stride, int pieces,
                                                               const int64_t* __restrict__ off, int64_t n_docs, int64_t v0,
                                                               uint4* __restrict__ vecs)
{
    const int64_t v = v0 + blockIdx.x, lo = doc_of_vector(off, n_docs, v);
    const uint4* s = src + (lo * row_stride + (v - off[lo])) * pieces;
    uint4* d = vecs + v * pieces;
    for (int p = threadIdx.x; p < pieces; p += kPackThreads) d[p] = s[p];
}

// ---- the fp8 format (multivec.h) -----------------------------------------------------------------------------------------
constexpr char kMagicQ[8] = {'H', 'I', 'P', 'M', 'V', 'Q', '8', '1'};
constexpr uint32_t kAmaxLo = 67u << 7, kAmaxHi = 187u << 7;   // bf16 magnitude bits of 2^-60 and 2^60: the domain
constexpr uint32_t kScaleOne = 0x3F800000u;

// The e4m3fn (OCP) code of x, round to nearest even, in integer operations: |x| <= 256 and finite, so nothing saturates.
// A zero code loses its sign.
__device__ __forceinline__ uint32_t e4m3_rne(float x)
{
    const uint32_t f = __float_as_uint(x), sign = (f >> 24) & 0x80u, a = f & 0x7FFFFFFFu;
    uint32_t code;
    if (a >= 0x3C800000u) {   // |x| >= 2^-6, a normal code: exponent and three mantissa bits, the carry runs into the exponent
        const uint32_t keep = (a >> 20) - (120u << 3), rem = a & 0xFFFFFu;
        code = keep + ((rem > 0x80000u || (rem == 0x80000u && (keep & 1u))) ? 1u : 0u);
    } else {                  // multiples of 2^-9; 8 of them are the smallest normal code
        code = (uint32_t)rintf(__uint_as_float(a) * 512.f);
    }
    return code ? (sign | code) : 0u;
}

__device__ __forceinline__ float e4m3_value(uint32_t code)
{
    const uint32_t mag = code & 0x7Fu, ex = mag >> 3, man = mag & 7u;
    const float v = ex ? __uint_as_float(((ex + 120u) << 23) | (man << 20)) : (float)man * 0x1p-9f;
    return (code & 0x80u) ? -v : v;
}

__device__ __forceinline__ uint32_t max_mag2(uint32_t m, uint32_t w) { return max(m, max(w & 0x7FFFu, (w >> 16) & 0x7FFFu)); }

__device__ __forceinline__ uint32_t quant2(uint32_t w, float mul)   // two bf16 in a word -> two codes in the low 16 bits
{
    return e4m3_rne(__uint_as_float(w << 16) * mul) | (e4m3_rne(__uint_as_float(w & 0xFFFF0000u) * mul) << 8);
}

// One wave quantises one vector: lane l < dim / 16 takes 16 values (two 16-byte loads), the wave agrees on amax (a max of
// magnitude bits: it does not depend on order, and a non-finite component is above every finite one), each lane converts
// and stores its 16 codes in one 16-byte store, lane 0 writes the scale and counts a vector the domain guard zeroed.
__device__ __forceinline__ void quantise_vector(const uint4* __restrict__ s, int dim, uint4* __restrict__ d, float* __restrict__ scale,
                                                unsigned long long* __restrict__ guarded)
{
    const int lane = threadIdx.x, n16 = dim >> 4;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (lane < n16) { a = s[2 * lane]; b = s[2 * lane + 1]; }
    uint32_t amax = 0;
    amax = max_mag2(amax, a.x); amax = max_mag2(amax, a.y); amax = max_mag2(amax, a.z); amax = max_mag2(amax, a.w);
    amax = max_mag2(amax, b.x); amax = max_mag2(amax, b.y); amax = max_mag2(amax, b.z); amax = max_mag2(amax, b.w);
#pragma unroll
    for (int dist = 32; dist; dist >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, dist));
    const bool ok = amax >= kAmaxLo && amax <= kAmaxHi;
    const uint32_t ex = amax >> 7;                                     // e = 134 - ex
    const float mul = __uint_as_float(ok ? (261u - ex) << 23 : 0u);    // 2^e, or 0: every code 0x00
    if (lane < n16) {
        uint4 c;
        c.x = quant2(a.x, mul) | (quant2(a.y, mul) << 16);
        c.y = quant2(a.z, mul) | (quant2(a.w, mul) << 16);
        c.z = quant2(b.x, mul) | (quant2(b.y, mul) << 16);
        c.w = quant2(b.z, mul) | (quant2(b.w, mul) << 16);
        d[lane] = ok ? c : make_uint4(0u, 0u, 0u, 0u);   // the guard: a non-finite value times 0 is no code
    }
    if (lane == 0) {
        *scale = __uint_as_float(ok ? (ex - 7u) << 23 : kScaleOne);    // 2^-e
        if (!ok && amax != 0) atomicAdd(guarded, 1ull);
    }
}

// mv_pack_kernel for an fp8 store: the same grid, search and source row; packs and quantises in one pass.
__global__ __launch_bounds__(kPackThreads) void mv_quant_pack_kernel(const uint4* __restrict__ src, int64_t row_stride, int dim,
                                                                     const int64_t* __restrict__ off, int64_t n_docs, int64_t v0,
                                                                     uint4* __restrict__ codes, float* __restrict__ scales,
                                                                     unsigned long long* __restrict__ guarded)
{
    const int64_t v = v0 + blockIdx.x, lo = doc_of_vector(off, n_docs, v);
    quantise_vector(src + (lo * row_stride + (v - off[lo])) * (dim >> 3), dim, codes + v * (dim >> 4), scales + v, guarded);
}

// The same from packed rows: row blockIdx.x of src becomes stored vector v0 + blockIdx.x (the host append, hipmv_to_fp8).
__global__ __launch_bounds__(kPackThreads) void mv_quant_rows_kernel(const uint4* __restrict__ src, int dim, int64_t v0,
                                                                     uint4* __restrict__ codes, float* __restrict__ scales,
                                                                     unsigned long long* __restrict__ guarded)
{
    const int64_t v = v0 + blockIdx.x;
    quantise_vector(src + (int64_t)blockIdx.x * (dim >> 3), dim, codes + v * (dim >> 4), scales + v, guarded);
}

// code * scale as bf16 bits (exact: the product has 4 significant bits and its exponent is in range), four codes per thread
__global__ __launch_bounds__(256) void mv_dequant_kernel(const uint32_t* __restrict__ codes, const float* __restrict__ scales, int dim,
                                                         int64_t n_words, uint2* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    const uint32_t w = codes[i];
    const float s = scales[i / (dim >> 2)];
    const uint32_t b0 = __float_as_uint(e4m3_value(w) * s) >> 16, b1 = __float_as_uint(e4m3_value(w >> 8) * s) >> 16;
    const uint32_t b2 = __float_as_uint(e4m3_value(w >> 16) * s) >> 16, b3 = __float_as_uint(e4m3_value(w >> 24) * s) >> 16;
    out[i] = make_uint2(b0 | (b1 << 16), b2 | (b3 << 16));
}

// the NaN patterns, (b & 0x7F) == 0x7F, among n_words words of codes: one streaming pass of a load
__global__ __launch_bounds__(256) void mv_count_nan_kernel(const uint32_t* __restrict__ codes, int64_t n_words,
                                                           unsigned long long* __restrict__ count)
{
    unsigned n = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const uint32_t w = codes[i];
#pragma unroll
        for (int b = 0; b < 4; ++b) n += ((w >> (8 * b)) & 0x7Fu) == 0x7Fu ? 1u : 0u;
    }
    if (n) atomicAdd(count, (unsigned long long)n);
}

// ---- the MXFP4 format (multivec.h) ---------------------------------------------------------------------------------------
constexpr char kMagicQ4[8] = {'H', 'I', 'P', 'M', 'V', 'Q', '4', '1'};
constexpr uint32_t kScaleByteOne = 127u, kScaleByteLo = 27u, kScaleByteHi = 185u;   // 2^0; E = -100; E = 58 (amax = 2^60)

// The e2m1 code of x, round to nearest, ties to the even mantissa, saturating at 6: the code of a magnitude is the number of
// the seven midpoints between neighbouring codes it has passed, a midpoint itself passing where the code above it is even.
// A zero code loses its sign.
__device__ __forceinline__ uint32_t e2m1_rne(float x)
{
    const float a = fabsf(x);
    const uint32_t code = (a > 0.25f ? 1u : 0u) + (a >= 0.75f ? 1u : 0u) + (a > 1.25f ? 1u : 0u) + (a >= 1.75f ? 1u : 0u) +
                          (a > 2.5f ? 1u : 0u) + (a >= 3.5f ? 1u : 0u) + (a > 5.0f ? 1u : 0u);
    return code ? (((__float_as_uint(x) >> 28) & 8u) | code) : 0u;
}

__device__ __forceinline__ float e2m1_value(uint32_t code)
{
    const uint32_t ex = (code >> 1) & 3u, man = code & 1u;
    const float v = ex ? __uint_as_float(((ex + 126u) << 23) | (man << 22)) : 0.5f * (float)man;
    return (code & 8u) ? -v : v;
}

__device__ __forceinline__ uint32_t quant2_fp4(uint32_t w, float mul)   // two bf16 in a word -> one byte of codes
{
    return e2m1_rne(__uint_as_float(w << 16) * mul) | (e2m1_rne(__uint_as_float(w & 0xFFFF0000u) * mul) << 4);
}

// One wave quantises one vector, lane l < dim / 16 its 16 values as in the fp8 format: the wave agrees on amax for the guard,
// the two lanes of a block of 32 on bmax (maxima of magnitude bits: no order in them), each lane stores its 8 bytes of codes,
// the even lane of a block its scale byte, lane 0 counts a vector the guard zeroed.
__device__ __forceinline__ void quantise_vector_mxfp4(const uint4* __restrict__ s, int dim, uint2* __restrict__ d,
                                                      unsigned char* __restrict__ scale, unsigned long long* __restrict__ guarded)
{
    const int lane = threadIdx.x, n16 = dim >> 4;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (lane < n16) { a = s[2 * lane]; b = s[2 * lane + 1]; }
    uint32_t bmax = 0;
    bmax = max_mag2(bmax, a.x); bmax = max_mag2(bmax, a.y); bmax = max_mag2(bmax, a.z); bmax = max_mag2(bmax, a.w);
    bmax = max_mag2(bmax, b.x); bmax = max_mag2(bmax, b.y); bmax = max_mag2(bmax, b.z); bmax = max_mag2(bmax, b.w);
    bmax = max(bmax, (uint32_t)__shfl_xor((int)bmax, 1));
    uint32_t amax = bmax;
#pragma unroll
    for (int dist = 32; dist > 1; dist >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, dist));
    const bool ok = amax >= kAmaxLo && amax <= kAmaxHi;
    const bool some = ok && bmax != 0;
    const uint32_t byte = some ? max(bmax >> 7, kScaleByteLo + 2u) - 2u : kScaleByteOne;   // E + 127, E = max(ex - 129, -100)
    const float mul = __uint_as_float(some ? (254u - byte) << 23 : 0u);                    // 2^-E, or 0
    if (lane < n16) {
        uint2 c;
        c.x = quant2_fp4(a.x, mul) | (quant2_fp4(a.y, mul) << 8) | (quant2_fp4(a.z, mul) << 16) | (quant2_fp4(a.w, mul) << 24);
        c.y = quant2_fp4(b.x, mul) | (quant2_fp4(b.y, mul) << 8) | (quant2_fp4(b.z, mul) << 16) | (quant2_fp4(b.w, mul) << 24);
        d[lane] = some ? c : make_uint2(0u, 0u);   // the guard: a non-finite value times 0 is no code
        if ((lane & 1) == 0) scale[lane >> 1] = (unsigned char)byte;
    }
    if (lane == 0 && !ok && amax != 0) atomicAdd(guarded, 1ull);
}

// mv_quant_pack_kernel and mv_quant_rows_kernel for an MXFP4 store
__global__ __launch_bounds__(kPackThreads) void mv_quant4_pack_kernel(const uint4* __restrict__ src, int64_t row_stride, int dim,
                                                                      const int64_t* __restrict__ off, int64_t n_docs, int64_t v0,
                                                                      uint2* __restrict__ codes, unsigned char* __restrict__ scales,
                                                                      unsigned long long* __restrict__ guarded)
{
    const int64_t v = v0 + blockIdx.x, lo = doc_of_vector(off, n_docs, v);
    quantise_vector_mxfp4(src + (lo * row_stride + (v - off[lo])) * (dim >> 3), dim, codes + v * (dim >> 4), scales + v * (dim >> 5), guarded);
}

__global__ __launch_bounds__(kPackThreads) void mv_quant4_rows_kernel(const uint4* __restrict__ src, int dim, int64_t v0,
                                                                      uint2* __restrict__ codes, unsigned char* __restrict__ scales,
                                                                      unsigned long long* __restrict__ guarded)
{
    const int64_t v = v0 + blockIdx.x;
    quantise_vector_mxfp4(src + (int64_t)blockIdx.x * (dim >> 3), dim, codes + v * (dim >> 4), scales + v * (dim >> 5), guarded);
}

// code * 2^E as bf16 bits (exact, multivec.h), a word of eight codes per thread
__global__ __launch_bounds__(256) void mv_dequant4_kernel(const uint32_t* __restrict__ codes, const unsigned char* __restrict__ scales,
                                                          int64_t n_words, uint4* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    const uint32_t w = codes[i];
    const float s = __uint_as_float((uint32_t)scales[i >> 2] << 23);   // four words to a block of 32
    uint32_t b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = __float_as_uint(e2m1_value((w >> (4 * j)) & 15u) * s) >> 16;
    out[i] = make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
}

// the -0 nibbles, 0x8, among n_words words of codes: one streaming pass of a load
__global__ __launch_bounds__(256) void mv_count_neg_zero_kernel(const uint32_t* __restrict__ codes, int64_t n_words,
                                                                unsigned long long* __restrict__ count)
{
    unsigned n = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const uint32_t w = codes[i];
#pragma unroll
        for (int b = 0; b < 8; ++b) n += ((w >> (4 * b)) & 15u) == 8u ? 1u : 0u;
    }
    if (n) atomicAdd(count, (unsigned long long)n);
}

// hipmv_gather_f32_dev: one workgroup per gathered vector, out[blockIdx.x][k] = stored vector idx[blockIdx.x] as float --
// the bf16 value widened, or code * scale (exact in bf16, hence in fp32) of the two quantised formats.
__global__ __launch_bounds__(kPackThreads) void mv_gather_f32_kernel(const int64_t* __restrict__ idx, int dim, int format,
                                                                     const uint16_t* __restrict__ vecs, const unsigned char* __restrict__ codes,
                                                                     const void* __restrict__ scales, float* __restrict__ out)
{
    const int64_t v = idx[blockIdx.x];
    float* o = out + (int64_t)blockIdx.x * dim;
    for (int k = threadIdx.x; k < dim; k += kPackThreads) {
        float x;
        if (format == kMvFp8) {
            x = e4m3_value(codes[v * dim + k]) * reinterpret_cast<const float*>(scales)[v];
        } else if (format == kMvMxfp4) {
            const uint32_t byte = codes[v * (dim >> 1) + (k >> 1)];
            const uint32_t sb = reinterpret_cast<const unsigned char*>(scales)[v * (dim >> 5) + (k >> 5)];
            x = e2m1_value((k & 1) ? byte >> 4 : byte & 15u) * __uint_as_float(sb << 23);
        } else {
            x = __uint_as_float((uint32_t)vecs[v * dim + k] << 16);
        }
        o[k] = x;
    }
}

// launch(i0, m) for every piece [i0, i0 + m) of [0, n): one workgroup per element, at most 2^30 of them per launch
template <class Launch>
int32_t launch_chunked(int64_t n, Launch launch)
{
    constexpr int64_t kMaxGrid = 1ll << 30;
    for (int64_t i0 = 0; i0 < n; i0 += kMaxGrid) {
        launch(i0, dim3((unsigned)std::min(kMaxGrid, n - i0)));
        HR_CHECK_HIP(hipGetLastError());
    }
    return HIPRAG_OK;
}

// rows [0, n) of packed bf16 device memory -> stored vectors v0 .. on the null stream
int32_t launch_quant_rows(MultiVecStore& s, const void* rows_dev, int64_t n, int64_t v0)
{
    if (s.format == kMvMxfp4)
        return launch_chunked(n, [&](int64_t r0, dim3 grid) {
            hipLaunchKernelGGL(mv_quant4_rows_kernel, grid, dim3(kPackThreads), 0, nullptr,
                               (const uint4*)((const char*)rows_dev + (size_t)r0 * s.dim * 2), (int)s.dim, v0 + r0, s.codes.as<uint2>(),
                               s.scales.as<unsigned char>(), s.guarded.as<unsigned long long>());
        });
    return launch_chunked(n, [&](int64_t r0, dim3 grid) {
        hipLaunchKernelGGL(mv_quant_rows_kernel, grid, dim3(kPackThreads), 0, nullptr,
                           (const uint4*)((const char*)rows_dev + (size_t)r0 * s.dim * 2), (int)s.dim, v0 + r0, s.codes.as<uint4>(),
                           s.scales.as<float>(), s.guarded.as<unsigned long long>());
    });
}

int32_t check_shape(int32_t dim, int32_t max_doc_vectors, int32_t format = kMvBf16)
{
    HR_REQUIRE(format == kMvBf16 || format == kMvFp8 || format == kMvMxfp4, "format must be 0 (bf16), 1 (fp8) or 4 (mxfp4) (got %d)", format);
    HR_REQUIRE(dim >= 64 && dim <= kMaxDim && dim % 64 == 0, "dim must be a multiple of 64 in 64..%d (got %d)", kMaxDim, dim);
    HR_REQUIRE(format != kMvFp8 || dim % 128 == 0, "an fp8 store needs dim to be a multiple of 128 in 128..%d (got %d): a vector "
               "is a whole number of 128-byte lines", kMaxDim, dim);
    HR_REQUIRE(format != kMvMxfp4 || dim % 128 == 0, "an mxfp4 store needs dim to be a multiple of 128 in 128..%d (got %d): a vector's "
               "scales are whole 32-bit words", kMaxDim, dim);
    HR_REQUIRE(max_doc_vectors >= 1, "max_doc_vectors must be at least 1 (got %d)", max_doc_vectors);
    return HIPRAG_OK;
}

int32_t new_store(int32_t dim, int32_t max_doc_vectors, int32_t device, std::shared_ptr<MultiVecStore>* out, int32_t format = kMvBf16)
{
    HR_CHECK_HIP(hipSetDevice(device));
    auto s = std::make_shared<MultiVecStore>();
    s->device = device;
    s->dim = dim;
    s->format = format;
    int32_t rc;
    if ((rc = s->csr.init(max_doc_vectors))) return rc;
    if (format != kMvBf16) {
        if ((rc = s->guarded.reserve(sizeof(unsigned long long)))) return rc;
        HR_CHECK_HIP(hipMemset(s->guarded.p, 0, sizeof(unsigned long long)));
    }
    *out = s;
    return HIPRAG_OK;
}

struct FileCloser {
    FILE* f;
    ~FileCloser() { if (f) fclose(f); }
};

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipmv_create_ex(int32_t dim, int32_t max_doc_vectors, int32_t device, int32_t format, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "null out");
    int32_t rc;
    if ((rc = check_shape(dim, max_doc_vectors, format))) return rc;
    std::shared_ptr<MultiVecStore> s;
    if ((rc = new_store(dim, max_doc_vectors, device, &s, format))) return rc;
    *out_handle = mv_reg().put(s);
    return HIPRAG_OK;
}

int32_t hipmv_create(int32_t dim, int32_t max_doc_vectors, int32_t device, uint64_t* out_handle)
{
    return hipmv_create_ex(dim, max_doc_vectors, device, kMvBf16, out_handle);
}

int32_t hipmv_destroy(uint64_t h)
{
    GET_MV(s, h);
    {
        std::lock_guard<std::mutex> guard(s->mu);
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
    }
    mv_reg().erase(h);
    return HIPRAG_OK;
}

int32_t hipmv_append_dev(uint64_t h, const void* vecs_dev, int32_t row_stride, const int32_t* counts_host, int64_t n_docs,
                         void* stream)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    // every check before anything is touched
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(row_stride >= 1, "row_stride must be at least 1 (got %d)", row_stride);
    HR_REQUIRE(counts_host || n_docs == 0, "counts is null");
    HR_REQUIRE(vecs_dev || n_docs == 0, "vecs is null");
    HR_REQUIRE(((uintptr_t)vecs_dev & 15) == 0, "vecs must be aligned to 16 bytes");
    for (int64_t i = 0; i < n_docs; ++i)
        HR_REQUIRE(counts_host[i] >= 0 && counts_host[i] <= row_stride, "counts[%lld] = %d lies outside [0, row_stride = %d]",
                   (long long)i, counts_host[i], row_stride);
    HR_REQUIRE(s->csr.n_docs + n_docs < (1ll << 31), "the store would hold %lld documents: the limit is 2^31 - 1",
               (long long)(s->csr.n_docs + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    std::vector<int64_t> off;
    std::vector<int32_t> lens;
    s->csr.plan_append(n_docs, [&](int64_t i) { return counts_host[i]; }, off, lens);
    int32_t rc;
    if ((rc = s->csr.ensure_capacity(s->item_parts(), s->csr.n_docs + n_docs, off.back()))) return rc;
    HR_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));   // the producer of vecs_dev has finished
    if ((rc = s->csr.write_offsets(off))) return rc;
    const int64_t* new_off = s->csr.offsets.as<int64_t>() + s->csr.n_docs;
    const int32_t fmt = s->format;
    rc = launch_chunked(off.back() - s->csr.n_items, [&](int64_t v0, dim3 grid) {
        if (fmt == kMvMxfp4)
            hipLaunchKernelGGL(mv_quant4_pack_kernel, grid, dim3(kPackThreads), 0, nullptr, (const uint4*)vecs_dev, (int64_t)row_stride,
                               (int)s->dim, new_off, n_docs, s->csr.n_items + v0, s->codes.as<uint2>(), s->scales.as<unsigned char>(),
                               s->guarded.as<unsigned long long>());
        else if (fmt == kMvFp8)
            hipLaunchKernelGGL(mv_quant_pack_kernel, grid, dim3(kPackThreads), 0, nullptr, (const uint4*)vecs_dev, (int64_t)row_stride,
                               (int)s->dim, new_off, n_docs, s->csr.n_items + v0, s->codes.as<uint4>(), s->scales.as<float>(),
                               s->guarded.as<unsigned long long>());
        else
            hipLaunchKernelGGL(mv_pack_kernel, grid, dim3(kPackThreads), 0, nullptr, (const uint4*)vecs_dev, (int64_t)row_stride,
                               (int)(s->dim / 8), new_off, n_docs, s->csr.n_items + v0, s->vecs.as<uint4>());
    });
    if (rc) return rc;
    if (s->ncent && (rc = mv_code_range(*s, s->csr.n_items, off.back(), nullptr))) return rc;   // the codes of the new vectors, as stored
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    s->csr.commit_append(off, lens);
    return HIPRAG_OK;
}

int32_t hipmv_append(uint64_t h, const void* vecs_host, const int64_t* offsets_host, int64_t n_docs)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(offsets_host, "offsets is null");
    HR_REQUIRE(offsets_host[0] == 0, "offsets must start at 0 (got %lld)", (long long)offsets_host[0]);
    for (int64_t i = 0; i < n_docs; ++i)
        HR_REQUIRE(offsets_host[i] <= offsets_host[i + 1], "offsets descend at document %lld", (long long)i);
    HR_REQUIRE(vecs_host || offsets_host[n_docs] == 0, "vecs is null");
    HR_REQUIRE(s->csr.n_docs + n_docs < (1ll << 31), "the store would hold %lld documents: the limit is 2^31 - 1",
               (long long)(s->csr.n_docs + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    std::vector<int64_t> off;
    std::vector<int32_t> lens;
    s->csr.plan_append(n_docs, [&](int64_t i) { return offsets_host[i + 1] - offsets_host[i]; }, off, lens);
    int32_t rc;
    // Consecutive documents that lose nothing to the cap are one contiguous run of the source: one copy per run.
    const size_t vb = (size_t)s->dim * 2;
    const char* src = (const char*)vecs_host;
    const bool quantised = s->format != kMvBf16;   // fp8 or mxfp4
    DevBuf stage;   // the bf16 rows of a run go up in bounded pieces and the kernel of the device form quantises them
    const int64_t stage_rows = std::max<int64_t>(1, (int64_t)(kIoChunk / vb));
    if (quantised && off.back() > s->csr.n_items && (rc = stage.reserve((size_t)std::min(stage_rows, off.back() - s->csr.n_items) * vb))) return rc;
    if ((rc = s->csr.ensure_capacity(s->item_parts(), s->csr.n_docs + n_docs, off.back()))) return rc;
    char* dst = s->vecs.as<char>();
    for (int64_t i = 0; i < n_docs;) {
        int64_t j = i;
        while (j + 1 < n_docs && offsets_host[j + 1] - offsets_host[j] == lens[(size_t)j]) ++j;
        const int64_t n = offsets_host[j] - offsets_host[i] + lens[(size_t)j];
        if (n && quantised) {
            for (int64_t r0 = 0; r0 < n; r0 += stage_rows) {
                const int64_t m = std::min(stage_rows, n - r0);
                HR_CHECK_HIP(hipMemcpy(stage.p, src + (size_t)(offsets_host[i] + r0) * vb, (size_t)m * vb, hipMemcpyHostToDevice));
                if ((rc = launch_quant_rows(*s, stage.p, m, off[(size_t)i] + r0))) return rc;
            }
        } else if (n) {
            HR_CHECK_HIP(hipMemcpy(dst + (size_t)off[(size_t)i] * vb, src + (size_t)offsets_host[i] * vb, (size_t)n * vb, hipMemcpyHostToDevice));
        }
        i = j + 1;
    }
    if (s->ncent && (rc = mv_code_range(*s, s->csr.n_items, off.back(), nullptr))) return rc;   // the codes of the new vectors, as stored
    if (quantised || s->ncent) HR_CHECK_HIP(hipStreamSynchronize(nullptr));   // before the staging buffer goes
    if ((rc = s->csr.write_offsets(off))) return rc;
    s->csr.commit_append(off, lens);
    return HIPRAG_OK;
}

int32_t hipmv_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    RangeTable tab;
    int32_t rc;
    if ((rc = range_table(ranges_host, n_ranges, s->csr.n_docs, "n_docs", true, tab))) return rc;
    if (tab.empty()) return HIPRAG_OK;
    return s->csr.remove(s->item_parts(), tab);
}

int32_t hipmv_export(uint64_t h, int64_t* offsets, void* vecs)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    if (offsets) HR_CHECK_HIP(hipMemcpy(offsets, s->csr.offsets.p, (size_t)(s->csr.n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (vecs && s->csr.n_items && s->format != kMvBf16) {   // the dequantised bf16 bits, through a bounded staging buffer
        const bool q4 = s->format == kMvMxfp4;
        const size_t vb = (size_t)s->dim * 2;
        const int64_t rows = std::max<int64_t>(1, (int64_t)(kIoChunk / vb)), cw = s->dim / (q4 ? 8 : 4);   // words of codes per vector
        DevBuf stage;
        int32_t rc;
        if ((rc = stage.reserve((size_t)std::min(rows, s->csr.n_items) * vb))) return rc;
        for (int64_t v0 = 0; v0 < s->csr.n_items; v0 += rows) {
            const int64_t m = std::min(rows, s->csr.n_items - v0), n_words = m * cw;
            if (q4)
                hipLaunchKernelGGL(mv_dequant4_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, nullptr,
                                   (const uint32_t*)(s->codes.as<uint32_t>() + v0 * cw),
                                   (const unsigned char*)(s->scales.as<unsigned char>() + v0 * (s->dim / 32)), n_words, stage.as<uint4>());
            else
                hipLaunchKernelGGL(mv_dequant_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, nullptr,
                                   (const uint32_t*)(s->codes.as<uint32_t>() + v0 * cw), (const float*)(s->scales.as<float>() + v0),
                                   (int)s->dim, n_words, stage.as<uint2>());
            HR_CHECK_HIP(hipGetLastError());
            HR_CHECK_HIP(hipMemcpy((char*)vecs + (size_t)v0 * vb, stage.p, (size_t)m * vb, hipMemcpyDeviceToHost));
        }
    } else if (vecs && s->csr.n_items) {
        HR_CHECK_HIP(hipMemcpy(vecs, s->vecs.p, (size_t)s->csr.n_items * s->dim * 2, hipMemcpyDeviceToHost));
    }
    return HIPRAG_OK;
}

int32_t hipmv_export_fp8(uint64_t h, int64_t* offsets, void* codes, float* scales)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(s->format == kMvFp8, "the store is no fp8 store: it has no e4m3 codes and fp32 scales to export");
    if (offsets) HR_CHECK_HIP(hipMemcpy(offsets, s->csr.offsets.p, (size_t)(s->csr.n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (codes && s->csr.n_items) HR_CHECK_HIP(hipMemcpy(codes, s->codes.p, (size_t)s->csr.n_items * s->dim, hipMemcpyDeviceToHost));
    if (scales && s->csr.n_items) HR_CHECK_HIP(hipMemcpy(scales, s->scales.p, (size_t)s->csr.n_items * sizeof(float), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmv_export_mxfp4(uint64_t h, int64_t* offsets, void* codes, void* scales)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(s->format == kMvMxfp4, "the store is no mxfp4 store: it has no e2m1 codes and e8m0 scales to export");
    if (offsets) HR_CHECK_HIP(hipMemcpy(offsets, s->csr.offsets.p, (size_t)(s->csr.n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (codes && s->csr.n_items) HR_CHECK_HIP(hipMemcpy(codes, s->codes.p, (size_t)s->csr.n_items * (s->dim / 2), hipMemcpyDeviceToHost));
    if (scales && s->csr.n_items) HR_CHECK_HIP(hipMemcpy(scales, s->scales.p, (size_t)s->csr.n_items * (s->dim / 32), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmv_gather_f32_dev(uint64_t h, const int64_t* item_idx_host, int64_t n, float* out_f32_dev)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(n >= 0 && n < (1ll << 30), "n must be in 0..2^30 (got %lld)", (long long)n);
    HR_REQUIRE(item_idx_host || n == 0, "item_idx is null");
    HR_REQUIRE(out_f32_dev || n == 0, "out is null");
    for (int64_t i = 0; i < n; ++i)
        HR_REQUIRE(item_idx_host[i] >= 0 && item_idx_host[i] < s->csr.n_items, "item_idx[%lld] = %lld is no stored vector (the store holds %lld)",
                   (long long)i, (long long)item_idx_host[i], (long long)s->csr.n_items);
    if (n == 0) return HIPRAG_OK;
    DevBuf idx;
    int32_t rc;
    if ((rc = idx.reserve((size_t)n * sizeof(int64_t)))) return rc;
    HR_CHECK_HIP(hipMemcpy(idx.p, item_idx_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mv_gather_f32_kernel, dim3((unsigned)n), dim3(kPackThreads), 0, nullptr, (const int64_t*)idx.as<int64_t>(), (int)s->dim,
                       (int)s->format, (const uint16_t*)s->vecs.as<uint16_t>(), (const unsigned char*)s->codes.as<unsigned char>(),
                       (const void*)s->scales.p, out_f32_dev);
    HR_CHECK_HIP(hipGetLastError());
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));   // before the index buffer goes
    return HIPRAG_OK;
}

int32_t hipmv_format_info(uint64_t h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    unsigned long long guarded = 0;
    if (s->format != kMvBf16) {
        HR_CHECK_HIP(hipSetDevice(s->device));
        HR_CHECK_HIP(hipMemcpy(&guarded, s->guarded.p, sizeof(guarded), hipMemcpyDeviceToHost));
    }
    out4[0] = s->format;
    out4[1] = 0;
    for (const StorePart& part : s->parts()) out4[1] += (int64_t)part.bytes;
    out4[2] = (int64_t)guarded;
    out4[3] = 0;
    return HIPRAG_OK;
}

// hipmv_to_fp8 and hipmv_to_mxfp4: a new store of `format` from the bf16 store h, through the kernel of the host append
static int32_t quantised_copy(uint64_t h, int32_t format, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "null out");
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(s->format == kMvBf16, "the store is quantised already (format %d): only a bf16 store is converted", s->format);
    int32_t rc;
    if ((rc = check_shape(s->dim, s->csr.doc_cap, format))) return rc;
    std::shared_ptr<MultiVecStore> q;
    if ((rc = new_store(s->dim, s->csr.doc_cap, s->device, &q, format))) return rc;
    if ((rc = q->csr.ensure_capacity(q->parts(), s->csr.n_docs, s->csr.n_items))) return rc;
    HR_CHECK_HIP(hipDeviceSynchronize());   // whatever wrote the source has finished
    if ((rc = launch_quant_rows(*q, s->vecs.p, s->csr.n_items, 0))) return rc;
    HR_CHECK_HIP(hipMemcpy(q->csr.offsets.p, s->csr.offsets.p, (size_t)(s->csr.n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice));
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    q->csr.len_host = s->csr.len_host;
    q->csr.longest = s->csr.longest;
    q->csr.n_docs = s->csr.n_docs;
    q->csr.n_items = s->csr.n_items;
    *out_handle = mv_reg().put(q);
    return HIPRAG_OK;
}

int32_t hipmv_to_fp8(uint64_t h, uint64_t* out_handle) { return quantised_copy(h, kMvFp8, out_handle); }

int32_t hipmv_to_mxfp4(uint64_t h, uint64_t* out_handle) { return quantised_copy(h, kMvMxfp4, out_handle); }

int32_t hipmv_sizes(uint64_t h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    out4[0] = s->csr.n_docs;
    out4[1] = s->csr.n_items;
    out4[2] = s->dim;
    out4[3] = s->csr.longest;
    return HIPRAG_OK;
}

/* HIPMV001, little-endian, no gaps: char magic[8] | int32 version = 1 | int32 dim | int32 max_doc_vectors | int64 docs |
 * int64 stored vectors | int64 offsets[docs + 1] | bf16 vecs[stored][dim].
 * HIPMVQ81, the file of an fp8 store: char magic[8] | int32 version = 1 | int32 dim | int32 max_doc_vectors | int32 format = 1 |
 * int64 docs | int64 stored vectors | int64 offsets[docs + 1] | float scales[stored] | uint8 codes[stored][dim].
 * HIPMVQ41, the file of an MXFP4 store: HIPMVQ81's header with format = 4 | int64 offsets[docs + 1] |
 * uint8 scales[stored][dim / 32] | uint8 codes[stored][dim / 2]. */
int32_t hipmv_save(uint64_t h, const char* path)
{
    HR_REQUIRE(path, "null path");
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    std::vector<int64_t> off((size_t)s->csr.n_docs + 1);
    HR_CHECK_HIP(hipMemcpy(off.data(), s->csr.offsets.p, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    const std::string tmp = std::string(path) + ".tmp";
    bool ok;
    {
        FileCloser fc{fopen(tmp.c_str(), "wb")};
        if (!fc.f) { set_error("cannot open %s for writing", tmp.c_str()); return HIPRAG_E_IO; }
        const bool q = s->format != kMvBf16;
        const char* magic = s->format == kMvMxfp4 ? kMagicQ4 : q ? kMagicQ : kMagic;
        const int32_t head[4] = {kVersion, s->dim, s->csr.doc_cap, s->format};
        const int64_t counts[2] = {s->csr.n_docs, s->csr.n_items};
        ok = fwrite(magic, 1, 8, fc.f) == 8 && fwrite(head, 4, q ? 4 : 3, fc.f) == (q ? 4u : 3u) &&
             fwrite(counts, 8, 2, fc.f) == 2 && fwrite(off.data(), 8, off.size(), fc.f) == off.size();
        std::vector<char> buf(std::min((size_t)s->csr.n_items * s->dim * 2, kIoChunk));   // no part is larger
        for (const StorePart& part : s->parts())
            for (size_t o = 0, total = (size_t)s->csr.n_items * part.bytes; ok && o < total; o += kIoChunk) {
                const size_t n = std::min(kIoChunk, total - o);
                HR_CHECK_HIP(hipMemcpy(buf.data(), part.buf->as<char>() + o, n, hipMemcpyDeviceToHost));
                ok = fwrite(buf.data(), 1, n, fc.f) == n;
            }
        ok = ok && fflush(fc.f) == 0;
    }
    if (!ok || rename(tmp.c_str(), path) != 0) {
        (void)remove(tmp.c_str());
        set_error("write to %s failed", path);
        return HIPRAG_E_IO;
    }
    return HIPRAG_OK;
}

int32_t hipmv_load(const char* path, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(path && out_handle, "null argument");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) { set_error("cannot open %s", path); return HIPRAG_E_IO; }
    char magic[8];
    int32_t head[4] = {0, 0, 0, kMvBf16};
    int64_t counts[2];
    if (fread(magic, 1, 8, fc.f) != 8 || (memcmp(magic, kMagic, 8) != 0 && memcmp(magic, kMagicQ, 8) != 0 && memcmp(magic, kMagicQ4, 8) != 0)) {
        set_error("%s is neither a HIPMV001, a HIPMVQ81 nor a HIPMVQ41 file", path);
        return HIPRAG_E_IO;
    }
    // the kind is told by the magic
    const int32_t format = memcmp(magic, kMagicQ4, 8) == 0 ? kMvMxfp4 : memcmp(magic, kMagicQ, 8) == 0 ? kMvFp8 : kMvBf16;
    const bool q = format != kMvBf16, q4 = format == kMvMxfp4;
    const int64_t head_bytes = q ? 40 : 36;
    if (fread(head, 4, q ? 4 : 3, fc.f) != (q ? 4u : 3u) || fread(counts, 8, 2, fc.f) != 2) {
        set_error("%s: short header", path);
        return HIPRAG_E_IO;
    }
    // sizes and offsets are validated before anything is allocated on the device
    if (head[0] != kVersion) { set_error("%s: version %d is not supported", path, head[0]); return HIPRAG_E_IO; }
    if (q && head[3] != format) { set_error("%s: a %s file of format %d", path, q4 ? "HIPMVQ41" : "HIPMVQ81", head[3]); return HIPRAG_E_IO; }
    const int32_t dim = head[1], cap = head[2];
    const int64_t n_docs = counts[0], n_vecs = counts[1];
    if (dim < 64 || dim > kMaxDim || dim % (q ? 128 : 64) || cap < 1 || n_docs < 0 || n_docs >= (1ll << 31) || n_vecs < 0 ||
        n_vecs > n_docs * (int64_t)cap) {
        set_error("%s: bad header (dim %d, cap %d, %lld documents, %lld vectors)", path, dim, cap, (long long)n_docs, (long long)n_vecs);
        return HIPRAG_E_IO;
    }
    const int64_t body = head_bytes + (n_docs + 1) * 8 + n_vecs * (q4 ? dim / 2 + dim / 32 : q ? dim + 4 : dim * 2);
    if (fseek(fc.f, 0, SEEK_END) != 0 || (int64_t)ftell(fc.f) != body || fseek(fc.f, (long)head_bytes, SEEK_SET) != 0) {
        set_error("%s: the file does not have the %lld bytes its header asks for", path, (long long)body);
        return HIPRAG_E_IO;
    }
    std::vector<int64_t> off((size_t)n_docs + 1);
    if (fread(off.data(), 8, off.size(), fc.f) != off.size()) { set_error("%s: short read", path); return HIPRAG_E_IO; }
    std::vector<int32_t> lens((size_t)n_docs);
    bool ok = off[0] == 0 && off[(size_t)n_docs] == n_vecs;
    for (int64_t i = 0; ok && i < n_docs; ++i) {
        const int64_t len = off[(size_t)i + 1] - off[(size_t)i];
        ok = len >= 0 && len <= cap;
        lens[(size_t)i] = (int32_t)len;
    }
    if (!ok) { set_error("%s: the offsets do not start at 0, descend, exceed the cap or do not end at the vector count", path); return HIPRAG_E_IO; }
    std::shared_ptr<MultiVecStore> s;   // not registered before the end: a refused file keeps nothing
    int32_t rc;
    if ((rc = new_store(dim, cap, device, &s, format))) return rc;
    if ((rc = s->csr.ensure_capacity(s->parts(), n_docs, n_vecs))) return rc;
    std::vector<char> buf(std::min((size_t)n_vecs * dim * 2, kIoChunk));   // no part is larger
    DevBuf nan_count;
    if (q) {
        if ((rc = nan_count.reserve(sizeof(unsigned long long)))) return rc;
        HR_CHECK_HIP(hipMemset(nan_count.p, 0, sizeof(unsigned long long)));
    }
    for (const StorePart& part : s->parts())
        for (size_t o = 0, total = (size_t)n_vecs * part.bytes; o < total; o += kIoChunk) {
            const size_t n = std::min(kIoChunk, total - o);
            char* dst = part.buf->as<char>() + o;
            if (fread(buf.data(), 1, n, fc.f) != n) { set_error("%s: short read", path); return HIPRAG_E_IO; }
            if (part.buf == &s->scales && q4) {   // every scale byte: E + 127 with E in [-100, 58], and 127 itself
                const unsigned char* sc = reinterpret_cast<const unsigned char*>(buf.data());
                for (size_t i = 0; i < n; ++i)
                    if (sc[i] < kScaleByteLo || sc[i] > kScaleByteHi) {
                        set_error("%s: scale byte %zu of vector %zu is %u, outside [%u, %u]", path, (o + i) % (size_t)(dim / 32),
                                  (o + i) / (size_t)(dim / 32), (unsigned)sc[i], kScaleByteLo, kScaleByteHi);
                        return HIPRAG_E_IO;
                    }
            } else if (part.buf == &s->scales) {   // every scale: 1.0 is one of the positive powers of two inside the domain
                const uint32_t* sc = reinterpret_cast<const uint32_t*>(buf.data());
                for (size_t i = 0; i < n / 4; ++i)
                    if ((sc[i] & 0x807FFFFFu) != 0 || (sc[i] >> 23) < 60 || (sc[i] >> 23) > 180) {
                        set_error("%s: the scale of vector %zu is not a positive power of two in [2^-67, 2^53]", path, o / 4 + i);
                        return HIPRAG_E_IO;
                    }
            }
            HR_CHECK_HIP(hipMemcpy(dst, buf.data(), n, hipMemcpyHostToDevice));
            if (part.buf == &s->codes) {   // kIoChunk and dim are multiples of 4: whole words
                const int64_t n_words = (int64_t)(n / 4);
                hipLaunchKernelGGL(q4 ? mv_count_neg_zero_kernel : mv_count_nan_kernel, dim3((unsigned)std::min<int64_t>((n_words + 255) / 256, 4096)), dim3(256), 0, nullptr,
                                   (const uint32_t*)dst, n_words, nan_count.as<unsigned long long>());
                HR_CHECK_HIP(hipGetLastError());
            }
        }
    if (q) {
        unsigned long long nans = 0;
        HR_CHECK_HIP(hipMemcpy(&nans, nan_count.p, sizeof(nans), hipMemcpyDeviceToHost));
        if (nans) { set_error("%s: %llu codes are %s", path, nans, q4 ? "-0 nibbles (0x8)" : "NaN patterns"); return HIPRAG_E_IO; }
    }
    HR_CHECK_HIP(hipMemcpy(s->csr.offsets.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    std::vector<int64_t> end(1, n_vecs);
    s->csr.commit_append(end, lens);
    *out_handle = mv_reg().put(s);
    return HIPRAG_OK;
}

}  // extern "C"
