// dense_api.hip -- the C ABI of the flat index (hipidx_* of include/hiprag.h) and hiprag_scan_plan: argument checks, the
// handle registry, create, save / load and the statistics.  No kernel is compiled or launched here: every entry calls a
// DenseIndex method (dense_index.hip), and the launch policy it reports is dense_plan.h.
#include <cstring>
#include <vector>

#include "common.h"
#include "dense_internal.h"

namespace hiprag {

Registry<DenseIndex>& reg()
{
    static Registry<DenseIndex> r;
    return r;
}

int32_t create_dense(int32_t d, int32_t metric, int32_t device, std::shared_ptr<DenseIndex>& out)
{
    HR_REQUIRE(d > 0, "d must be positive (got %d)", d);
    HR_REQUIRE(metric == HIPRAG_METRIC_IP || metric == HIPRAG_METRIC_L2, "unknown metric %d", metric);
    const int P = ((d + 127) / 128) * 16;
    if ((size_t)P * 1024 > 128 * 1024) {
        set_error("d=%d needs %d KiB of LDS for the query tile; the scan supports d <= 1024 (128 KiB, leaving 32 KiB per CU "
                  "for the tail kernels of earlier passes)", d, P);
        return HIPRAG_E_UNSUPPORTED;
    }
    auto ix = std::make_shared<DenseIndex>();
    ix->device = device;
    ix->d = d;
    ix->P = P;
    ix->metric = metric;
    int32_t rc = ix->init();
    if (rc) return rc;
    out = ix;
    return HIPRAG_OK;
}

size_t clear_dense_registry() { clear_ivf_registry(); return reg().clear(); }

int32_t dense_id_base(uint64_t h, int64_t* out_base)
{
    GET_INDEX(h);
    *out_base = ix->id_base;
    return HIPRAG_OK;
}
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipidx_create(int32_t d, int32_t metric, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "out_handle is null");
    std::shared_ptr<DenseIndex> ix;
    int32_t rc = create_dense(d, metric, device, ix);
    if (rc) return rc;
    *out_handle = reg().put(ix);
    return HIPRAG_OK;
}

int32_t hipidx_destroy(uint64_t h)
{
    HR_GET_HANDLE(ix, reg(), h, "unknown dense index handle");
    {
        std::lock_guard<std::mutex> guard(ix->mu);
        (void)hipSetDevice(ix->device);
        (void)hipDeviceSynchronize();
    }
    reg().erase(h);
    return HIPRAG_OK;
}

int32_t hipidx_add(uint64_t h, const float* x_host, int64_t n)
{
    GET_INDEX(h);
    HR_REQUIRE(n >= 0 && (x_host || n == 0), "bad add arguments");
    return ix->add_host(x_host, n);
}

int32_t hipidx_add_dev(uint64_t h, const float* x_dev, int64_t n, void* stream)
{
    GET_INDEX(h);
    HR_REQUIRE(n >= 0 && (x_dev || n == 0), "bad add arguments");
    return ix->add_dev(x_dev, n, (hipStream_t)stream);
}

int32_t hipidx_ntotal(uint64_t h, int64_t* out_n)
{
    GET_INDEX(h);
    HR_REQUIRE(out_n, "null out");
    *out_n = ix->ntotal;
    return HIPRAG_OK;
}

int32_t hipidx_dim(uint64_t h, int32_t* out_d)
{
    GET_INDEX(h);
    HR_REQUIRE(out_d, "null out");
    *out_d = ix->d;
    return HIPRAG_OK;
}

int32_t hipidx_metric(uint64_t h, int32_t* out_metric)
{
    GET_INDEX(h);
    HR_REQUIRE(out_metric, "null out");
    *out_metric = ix->metric;
    return HIPRAG_OK;
}

int32_t hipidx_set_id_base(uint64_t h, int64_t id_base)
{
    GET_INDEX(h);
    ix->id_base = id_base;
    return HIPRAG_OK;
}

int32_t hipidx_pass_queries(uint64_t h, int32_t* out_n)
{
    GET_INDEX(h);
    HR_REQUIRE(out_n, "null out");
    *out_n = kPassQ;
    return HIPRAG_OK;
}

int32_t hipidx_launch_queries(uint64_t h, int32_t* out_n)
{
    GET_INDEX(h);
    HR_REQUIRE(out_n, "null out");
    *out_n = ix->launch_q;
    return HIPRAG_OK;
}

int32_t hipidx_set_spare_cus(uint64_t h, int32_t n)
{
    GET_INDEX(h);
    HR_REQUIRE(n >= 0 && n < ix->n_cu, "spare CUs must be in 0..%d", ix->n_cu - 1);
    // takes effect with the next launch: the finish reads a launch's lists and bounds, never its partition, and the stamp
    // buffer is sized for the whole chip
    ix->scan_cus = ix->n_cu - n;
    return HIPRAG_OK;
}

int32_t hipidx_gate_tail_dev(uint64_t h, int32_t slot, void* stream)
{
    GET_INDEX(h);
    HR_REQUIRE(slot >= 0 && slot < DenseIndex::kSlots, "slot must be in 0..7");
    return ix->gate_tail(slot, (hipStream_t)stream);
}

int32_t hipidx_get_spare_cus(uint64_t h, int32_t* out_n)
{
    GET_INDEX(h);
    HR_REQUIRE(out_n, "null out");
    *out_n = ix->n_cu - ix->scan_cus;
    return HIPRAG_OK;
}

int32_t hipidx_pipe_spare_cus(uint64_t h, int32_t* out_n)
{
    GET_INDEX(h);
    HR_REQUIRE(out_n, "null out");
    *out_n = ix->pipe_spare_cus();
    return HIPRAG_OK;
}

int32_t hipidx_scan_shape(uint64_t h, hipidx_scan_shape_t* out)
{
    GET_INDEX(h);
    HR_REQUIRE(out, "null out");
    *out = ix->shape();
    return HIPRAG_OK;
}

int32_t hiprag_scan_plan(const hipidx_scan_shape_t* shape, int32_t nq, int32_t k, int32_t cus, hipidx_scan_plan_t* out)
{
    HR_REQUIRE(shape && out, "null argument");
    HR_REQUIRE(shape->nblocks >= 0 && shape->P > 0 && shape->P % 16 == 0 && shape->n_cu > 0 && nq > 0 && k > 0 && cus > 0,
               "hiprag_scan_plan: nblocks >= 0, P a positive multiple of 16, n_cu, nq, k and cus positive");
    HR_REQUIRE(shape->mode == kScanBf16 || shape->mode == kScanQ64, "hiprag_scan_plan: mode must be 3 (bf16) or 2 (q64)");
    const ScanShape& s = *shape;
    const ScanPlan p = plan_scan(s, nq, k, cus);
    *out = {p.run, p.wide, p.waves, p.ring, p.multi_pass, p.filter, p.ncls, p.qtile_image, (int64_t)p.lds_bytes,
            launch_queries(s), pipe_spare_cus(s, launch_queries(s)), bytes_per_pass(s, HIPRAG_METRIC_IP, p.wide),
            bytes_per_pass(s, HIPRAG_METRIC_L2, p.wide)};
    return HIPRAG_OK;
}

int32_t hipidx_reserve_rows(uint64_t h, int64_t n_rows)
{
    GET_INDEX(h);
    HR_REQUIRE(n_rows >= 0, "n_rows < 0");
    return ix->grow((n_rows + kRowsPerBlock - 1) / kRowsPerBlock);
}

int32_t hipidx_reserve_search(uint64_t h, int32_t k)
{
    GET_INDEX(h);
    HR_REQUIRE(k > 0 && k <= kMaxK, "k must be in 1..%d (got %d)", kMaxK, k);
    return ix->reserve_slot(0, k);
}

int32_t hipidx_search_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, double* out_scores64_dev,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    GET_INDEX(h);
    HR_REQUIRE(nq >= 0, "nq < 0");
    HR_REQUIRE(k > 0 && k <= kMaxK, "k must be in 1..%d (got %d)", kMaxK, k);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_dev && out_scores64_dev && out_ids_dev, "null device pointer");
    return ix->search_dev(q_dev, nq, k, out_scores64_dev, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int32_t hipidx_search_begin_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t slot, void* stream)
{
    GET_INDEX(h);
    HR_REQUIRE(nq > 0 && nq <= ix->launch_q, "search_begin takes 1..%d queries (got %d)", ix->launch_q, nq);
    HR_REQUIRE(k > 0 && k <= kMaxK, "k must be in 1..%d (got %d)", kMaxK, k);
    HR_REQUIRE(slot >= 0 && slot < DenseIndex::kSlots, "slot must be in 0..7");
    HR_REQUIRE(q_dev, "null device pointer");
    int32_t rc = ix->prepare(k, slot);
    if (rc) return rc;
    return ix->begin_dev(q_dev, nq, k, slot, ix->scan_cus, (hipStream_t)stream);
}

int32_t hipidx_search_finish_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t slot,
                                 double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    GET_INDEX(h);
    HR_REQUIRE(nq > 0 && nq <= ix->launch_q, "search_finish takes 1..%d queries (got %d)", ix->launch_q, nq);
    HR_REQUIRE(slot >= 0 && slot < DenseIndex::kSlots, "slot must be in 0..7");
    HR_REQUIRE(k > 0 && k <= ix->ws[slot].k, "k=%d was not prepared by search_begin on slot %d", k, slot);
    HR_REQUIRE(q_dev && out_scores64_dev && out_ids_dev, "null device pointer");
    return ix->finish_dev(q_dev, nq, k, slot, out_scores64_dev, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int32_t hipidx_search(uint64_t h, const float* q_host, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids)
{
    GET_INDEX(h);
    HR_REQUIRE(nq >= 0, "nq < 0");
    HR_REQUIRE(k > 0 && k <= kMaxK, "k must be in 1..%d (got %d)", kMaxK, k);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_host && out_scores && out_ids, "null pointer");
    int32_t rc;
    if (nq <= DenseIndex::kFewQueries) return ix->search_few_host(q_host, nq, k, out_scores, out_ids);
    if ((rc = ix->qbuf.reserve((size_t)nq * ix->d * sizeof(float)))) return rc;
    if ((rc = ix->o64.reserve((size_t)nq * k * sizeof(double)))) return rc;
    if ((rc = ix->o32.reserve((size_t)nq * k * sizeof(float)))) return rc;
    if ((rc = ix->oid.reserve((size_t)nq * k * sizeof(int64_t)))) return rc;
    HR_CHECK_HIP(hipMemcpy(ix->qbuf.p, q_host, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice));
    rc = ix->search_dev(ix->qbuf.as<float>(), nq, k, ix->o64.as<double>(), ix->o32.as<float>(), ix->oid.as<int64_t>(),
                        nullptr);
    if (rc) return rc;
    HR_CHECK_HIP(hipMemcpy(out_scores, ix->o32.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, ix->oid.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipidx_reconstruct(uint64_t h, int64_t row, float* out_host)
{
    GET_INDEX(h);
    HR_REQUIRE(out_host, "null out");
    HR_REQUIRE(row >= 0 && row < ix->ntotal, "row %lld out of range [0,%lld)", (long long)row, (long long)ix->ntotal);
    DevBuf tmp;
    return read_rows_host(*ix, row, 1, tmp, out_host);
}

// File format "HIPIDX01": magic[8], int32 d, int32 metric, int64 ntotal, then ntotal*d fp32 row-major.
int32_t hipidx_save(uint64_t h, const char* path)
{
    GET_INDEX(h);
    HR_REQUIRE(path, "null path");
    { const int32_t wrc = ix->wait_adds_host(); if (wrc) return wrc; }
    FILE* f = fopen(path, "wb");
    if (!f) { set_error("cannot open %s for writing", path); return HIPRAG_E_IO; }
    const char magic[8] = {'H', 'I', 'P', 'I', 'D', 'X', '0', '1'};
    int32_t hd[2] = {ix->d, ix->metric};
    int64_t nt = ix->ntotal;
    bool ok = fwrite(magic, 1, 8, f) == 8 && fwrite(hd, 4, 2, f) == 2 && fwrite(&nt, 8, 1, f) == 1;
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(64ll << 20) / ((int64_t)ix->d * 4));
    DevBuf tmp;
    std::vector<float> host;
    if (ok && nt > 0) host.resize((size_t)std::min(chunk, nt) * ix->d);
    for (int64_t o = 0; ok && o < nt; o += chunk) {
        const int64_t m = std::min(chunk, nt - o);   // the first chunk is the largest: tmp is allocated once
        const int32_t rc = read_rows_host(*ix, o, m, tmp, host.data());
        if (rc) { fclose(f); return rc; }
        ok = fwrite(host.data(), sizeof(float), (size_t)m * ix->d, f) == (size_t)m * ix->d;
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) { set_error("write to %s failed", path); return HIPRAG_E_IO; }
    return HIPRAG_OK;
}

int32_t hipidx_load(const char* path, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(path && out_handle, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("cannot open %s", path); return HIPRAG_E_IO; }
    char magic[8];
    int32_t hd[2];
    int64_t nt = 0;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "HIPIDX01", 8) != 0 || fread(hd, 4, 2, f) != 2 ||
        fread(&nt, 8, 1, f) != 1 || nt < 0) {
        fclose(f);
        set_error("%s is not a HIPIDX01 file", path);
        return HIPRAG_E_IO;
    }
    uint64_t h = 0;
    int32_t rc = hipidx_create(hd[0], hd[1], device, &h);
    if (rc) { fclose(f); return rc; }
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(64ll << 20) / ((int64_t)hd[0] * 4));
    std::vector<float> host((size_t)std::min(chunk, std::max<int64_t>(nt, 1)) * hd[0]);
    for (int64_t o = 0; o < nt; o += chunk) {
        const int64_t m = std::min(chunk, nt - o);
        if (fread(host.data(), sizeof(float), (size_t)m * hd[0], f) != (size_t)m * hd[0]) {
            fclose(f);
            hipidx_destroy(h);
            set_error("%s is truncated", path);
            return HIPRAG_E_IO;
        }
        rc = hipidx_add(h, host.data(), m);
        if (rc) { fclose(f); hipidx_destroy(h); return rc; }
    }
    fclose(f);
    *out_handle = h;
    return HIPRAG_OK;
}

int32_t hipidx_enable_timing(uint64_t h, int32_t on)
{
    GET_INDEX(h);
    ix->timing.enable(on);
    return HIPRAG_OK;
}

int32_t hipidx_get_stats(uint64_t h, hipidx_stats* out)
{
    GET_INDEX(h);
    HR_REQUIRE(out, "null out");
    HR_CHECK_HIP(hipDeviceSynchronize());
    unsigned long long fb = 0;
    HR_CHECK_HIP(hipMemcpy(&fb, ix->fallback_counter(), sizeof(fb), hipMemcpyDeviceToHost));
    out->passes = ix->passes;
    out->launches = ix->launches;
    out->queries = ix->queries;
    out->fallback_queries = (int64_t)fb;
    {
        unsigned long long rbq = 0;
        HR_CHECK_HIP(hipMemcpy(&rbq, ix->extend_counter(), sizeof(rbq), hipMemcpyDeviceToHost));
        out->roundb_queries = (int64_t)rbq;
        unsigned long long wc[3] = {0, 0, 0};
        HR_CHECK_HIP(hipMemcpy(wc, ix->work_counters(), sizeof(wc), hipMemcpyDeviceToHost));
        out->list_entries = (int64_t)wc[0];
        out->ranked_entries = (int64_t)wc[1];
        out->rescored_groups = (int64_t)wc[2];
    }
    out->wide_launches = ix->wide_launches;
    {
        unsigned long long folds = 0;
        HR_CHECK_HIP(hipMemcpy(&folds, ix->fold_counter(), sizeof(folds), hipMemcpyDeviceToHost));
        out->wide_theta_folds = (int64_t)folds;
    }
    // per 64 queries of a launch_queries-sized launch: the wide kernel reads the filter copy and the norms once per 256 queries
    out->bytes_per_pass = bytes_per_pass(ix->shape(), ix->metric, ix->wide_launch(ix->launch_q));
    return ix->timing.summarise(ix->nblocks() > 0, out);
}

}  // extern "C"
