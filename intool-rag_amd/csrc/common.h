// common.h -- host-side plumbing shared by the libhiprag translation units (error state, handle registry).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>

#include "../../include/hiprag.h"

namespace hiprag {

void set_error(const char* fmt, ...);  // thread-local message, printf-style

#define HR_CHECK_HIP(expr)                                                                     \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            hiprag::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                              __LINE__);                                                       \
            return HIPRAG_E_HIP;                                                               \
        }                                                                                      \
    } while (0)

#define HR_REQUIRE(cond, ...)              \
    do {                                   \
        if (!(cond)) {                     \
            hiprag::set_error(__VA_ARGS__); \
            return HIPRAG_E_INVALID;       \
        }                                  \
    } while (0)

// The preamble of an entry point that takes a handle: `var` = the object behind h in `registry`, or the message and
// HIPRAG_E_HANDLE.
#define HR_GET_HANDLE(var, registry, h, ...)   \
    auto var = (registry).get(h);              \
    if (!var) {                                \
        hiprag::set_error(__VA_ARGS__);        \
        return HIPRAG_E_HANDLE;                \
    }

// Handle registry: uint64 -> shared_ptr<T>.  One registry per object kind.
template <typename T>
class Registry {
public:
    uint64_t put(std::shared_ptr<T> p)
    {
        std::lock_guard<std::mutex> g(mu_);
        uint64_t h = next_++;
        map_[h] = std::move(p);
        return h;
    }
    std::shared_ptr<T> get(uint64_t h)
    {
        std::lock_guard<std::mutex> g(mu_);
        auto it = map_.find(h);
        return it == map_.end() ? nullptr : it->second;
    }
    bool erase(uint64_t h)
    {
        std::lock_guard<std::mutex> g(mu_);
        return map_.erase(h) != 0;
    }
    size_t clear()   // drops every handle (hiprag_shutdown); objects die when their last user lets go
    {
        std::lock_guard<std::mutex> g(mu_);
        const size_t n = map_.size();
        map_.clear();
        return n;
    }

private:
    std::mutex mu_;
    std::unordered_map<uint64_t, std::shared_ptr<T>> map_;
    uint64_t next_ = 0x1000;
};

// RAII device buffer (never shrinks implicitly).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int32_t reserve(size_t want)
    {
        if (want <= bytes) return HIPRAG_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        HR_CHECK_HIP(hipMalloc(&p, want));
        bytes = want;
        return HIPRAG_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// Pinned host buffer (device-visible under the same address): staging for asynchronous copies that must not block the host,
// and a place kernels can write small results to directly.
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int32_t reserve(size_t want)
    {
        if (want <= bytes) return HIPRAG_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        if (want < 4096) want = 4096;
        HR_CHECK_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
        bytes = want;
        return HIPRAG_OK;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// hiprag_shutdown: every translation unit owns the registry of its handle type
size_t clear_dense_registry();
size_t clear_bm25_registry();
size_t clear_encoder_registry();
size_t clear_token_registry();
size_t clear_page_registry();
size_t clear_multivec_registry();

// hiphybrid_search_scoped*: a row of the dense index must be a document of the postings
int32_t bm25_n_docs(uint64_t h, int64_t* out_n);
// hipm3_score*: the legs must name the same documents by the same ids (bm25.hip, dense_api.hip), and the kernel behind
// them (m3_score.hip: combines the three components of every candidate and ranks them, one workgroup per query)
int32_t bm25_id_base(uint64_t h, int64_t* out_base);
int32_t dense_id_base(uint64_t h, int64_t* out_base);
struct M3Combine {
    const int64_t* cand;        // [nq][depth]
    const double* dense64;      // [nq][depth] hipidx_score_ids_dev's fp64 output, null: leg not run
    const float* dense32;       // its fp32 output
    const float* sparse32;      // [nq][depth] hipbm25_score_ids_dev's output, null: leg not run
    const float* maxsim32;      // [nq][depth] hipmaxsim_dev's pair scores, null: leg not run
    double w_dense, w_sparse, w_colbert, w_sum;
    int64_t id_base, ntotal;
    int depth, k, l2;
    float* out_parts;           // [nq][depth][3] or null
    double* out_pairs;          // [nq][depth] or null
    double* out_scores;         // [nq][k]
    int64_t* out_ids;           // [nq][k]
    int32_t* out_pos;           // [nq][k] or null
};
int32_t launch_m3_combine(const M3Combine& a, int nq, hipStream_t st);
// hiphybrid_search_ivf_scoped: makes the IVF index's device current on this thread (ivf_scoped.hip)
int32_t ivf_make_device_current(uint64_t h);

}  // namespace hiprag
